"""Host arithmetic of the towers' batch geometry: ops.Grid (same-size images) against the ragged plans' tables (ops.ImgSegs) for equal
sizes — a uniform and a ragged pass over the same images must agree on every level's size.  No GPU: the tables build on the CPU device."""
import pytest

from vlm_fo1_amd import ops
from vlm_fo1_amd.davit import DAVIT_LARGE, DaViT, RaggedAuxPlan
from vlm_fo1_amd.fpn import RaggedFpnPlan, SimpleFPN


def conv_ref(n, k, s, p):
    return (n + 2 * p - k) // s + 1


@pytest.mark.parametrize("H,W", [(97, 233), (61, 63), (7, 9), (480, 640)])
def test_grid_conv_out_for_davits_embeds_on_odd_extents(H, W):
    """DaViT's four ConvEmbeds: 7 / stride 4 / pad 3, then 3 / 2 / 1 three times."""
    g = ops.Grid(H, W, 3)
    for k, s, p in ((7, 4, 3), (3, 2, 1), (3, 2, 1), (3, 2, 1)):
        o = g.conv_out(k, k, s, p)
        assert (o.H, o.W, o.batch) == (conv_ref(g.H, k, s, p), conv_ref(g.W, k, s, p), 3)
        assert o.total_in == 3 * o.H * o.W and o.max_in == o.H * o.W and o.n == 3 and o.sizes == ((o.H, o.W),) * 3
        g = o
    assert (ops.Grid(97, 233).conv_out(7, 7, 4, 3).H, ops.Grid(97, 233).conv_out(7, 7, 4, 3).W) == (25, 59)
    assert (ops.Grid(25, 59).conv_out(3, 3, 2, 1).H, ops.Grid(25, 59).conv_out(3, 3, 2, 1).W) == (13, 30)


def test_grid_row_counts_of_the_spatial_operators():
    g = ops.Grid(13, 17, 2)
    assert g.rows_out(lambda x: x.windows(12)) == 2 * 24 * 24 and g.windows(12).sizes == ((24, 24),) * 2
    assert g.rows_out(lambda x: x.scaled(2)) == 2 * 26 * 34
    assert g.rows_out(lambda x: x.scaled(1, 2)) == 2 * 6 * 8
    assert g.args("in", 64, 12) == (13, 17, 64, 12, 2) == g.args("out", 64, 12)
    sg = ops.ImgSegs([(0, 13, 17, 0, 6, 8), (221, 4, 5, 48, 2, 2)], "cpu", 221, 241, 48, 52)
    assert sg.ragged and not g.ragged and (sg.n, sg.total_in, sg.rows_out(None)) == (2, 241, 52)
    assert sg.args("in", 64) == (sg.ptr, 2, 221, 241, 64) and sg.args("out", 64) == (sg.ptr, 2, 48, 52, 64)
    assert sg.dev.tolist()[1] == [221, 4, 5, 48, 2, 2, 0, 0]


@pytest.mark.parametrize("H,W,B", [(60, 64, 2), (97, 233, 3), (399, 500, 1)])
def test_uniform_davit_levels_equal_the_ragged_plan_of_equal_sizes(H, W, B):
    plan = RaggedAuxPlan([(H, W)] * B, DAVIT_LARGE, "cpu")
    tower = DaViT.__new__(DaViT)
    tower.cfg = DAVIT_LARGE
    levels = list(tower._uniform_levels(ops.Grid(H, W, B)))
    assert len(levels) == len(plan.levels) == 4
    prev = ops.Grid(H, W, B)
    for lv, rl, sizes in zip(levels, plan.levels, plan.sizes):
        assert list(lv["sizes"]) == list(sizes) == list(rl["sizes"])
        assert lv["conv"].sizes == prev.sizes and lv["pix"] is lv["win"] is lv["tok"]
        g = lv["pix"]
        assert (rl["pix"].n, rl["pix"].max_in, rl["pix"].total_in) == (g.n, g.max_in, g.total_in)
        assert (rl["conv"].total_in, rl["conv"].total_out) == (prev.total_in, g.total_in)
        assert rl["win"].total_out == g.windows(12).total_in and rl["win"].max_out == g.windows(12).max_in
        assert (rl["tok"].max_in, rl["tok"].total_in) == (g.max_in, g.total_in)
        prev = g


@pytest.mark.parametrize("gh,gw,B", [(4, 4, 2), (7, 9, 3), (34, 46, 1)])
def test_uniform_fpn_plan_equals_the_ragged_plan_of_equal_grids(gh, gw, B):
    ragged = RaggedFpnPlan([(gh, gw)] * B, [b * gh * gw for b in range(B)], "cpu")
    uni = SimpleFPN._uniform_plan(ops.Grid(gh, gw, B))
    assert [list(s) for s in uni.sizes] == [list(s) for s in ragged.sizes]
    for a, b in zip(uni.conv, ragged.conv):
        assert (a.total_in, a.max_in, a.n) == (b.total_in, b.max_in, b.n) and b.total_out == a.total_in
    for name, out in (("up_1a", lambda g: g.scaled(2)), ("up_1b", lambda g: g.scaled(2)), ("pool", lambda g: g.scaled(1, 2))):
        a, b = getattr(uni, name), getattr(ragged, name)
        assert (a.total_in, a.max_in, a.n) == (b.total_in, b.max_in, b.n) and a.rows_out(out) == b.total_out
