"""Prefill and window attention per launch route (csrc/attention.hip, csrc/window_attention.hip) against the fp64 reference of
tests/prefill_attention_cases.py.  Every output goes into a NaN-filled buffer with a padded row stride: every row an item covers must be
within the bound, every other row and every pad column must still be NaN.

  route      entry / kernel                                         cases
  fwd16      fo1_attention_bf16, attn_fwd_kernel<HD, 1/2/4>         HD 128 causal 16/2 (packed q|k|v), 12/2, 4/4; HD 80 16/16 (packed,
                                                                    head-major 256); HD 32 8/8 (packed); segments 1, 15, 16, 17, 63, 64,
                                                                    65, 127, 128, 129 (+ 1100 / 1030); each at q_block 16, 32 and 64
  fwd32      fo1_attention_bf16, attn_fwd32_kernel<HD, HPW>         HD 80 q_block 256 16/16 (packed) and 8/4; HD 128 q_block 128 16/2
                                                                    causal (packed), q_block 256 4/4 causal; segments 65, 191, 192, 193,
                                                                    255, 256, 257, 511, 20; ViT full 1564 + 300 (head-major 256)
  prefix16   fo1_attention_prefix_bf16, q_block 64                  HD 128 16/2 causal; prefixes 1, 63, 64, 65, 284, 408 and none,
  prefix32   fo1_attention_prefix_bf16, q_block 128                 own ranges 1, 64, 65, 252; the prefix rows themselves and the
                                                                    no-prefix items (empty ranges (0, 0) and start >= end) in one launch
  win1       fo1_attention_windows_bf16, attn_win1_kernel<80, 4>    16 heads; windows of 1, 4, 12, 63, 64 tokens; 1, 2, 3, 5, 8, 9 items;
                                                                    packed and head-major 256
  swin       fo1_attention_window_bias_bf16 (bias + shift mask)     HD 32; ws 12 / 7, shift 0 / ws // 2; 1x1, 1x3, 3x2, 2x2 windows, 1 or 2
                                                                    images stacked; 6 and 12 heads; q_block 64, 32, 16
  davit      fo1_window_attention_bf16 (win_attn32)                 8, 6, 32 heads; 1, 31, 32, 33, 37, 144, 160 tokens per window
  davit_map  fo1_window_attention_map_bf16                          2 x 13x25 (8 heads), 30x17 (6 heads); a non-zero pad row
  davit_var  fo1_window_attention_map_var_bf16                      40x30 + 13x25 + 7x5, 8 heads
  rowbase    fo1_attention_bf16 with *q_row_base = 0, 1, 1000       HD 128 16/2 causal, q_block 64; segments 1, 17, 64, 65, 130

and the bit-for-bit claims the host code relies on: run to run; a permuted item list; q_block 16 / 32 / 64 on the 16x16 form; attn_win1 ==
attn_fwd_kernel<80, 4>; an item with an empty prefix range == the same item launched without prefix ranges; a q_row_base launch == the
plain launch on row-shifted Q / O."""
import pytest
import torch

import prefill_attention_cases as C

pytestmark = pytest.mark.gpu

OPAD = 16           # pad columns of every output buffer (a multiple of 8: the 16-byte row stores)
WORST = {}          # route -> the worst max-row-error / (TOL * row max) seen


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit for bit, NaN fill included."""
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def _buf(d):
    c = d["case"]
    rows = d["N"] - c.row_base
    return torch.full((rows, c.Hq * c.HD + OPAD), float("nan"), dtype=torch.bfloat16, device="cuda")


def _items(rows: torch.Tensor, q_block: int, single_tile: bool = False) -> torch.Tensor:
    t = rows.contiguous().cuda()
    t.q_block = q_block
    if single_tile:
        t.single_tile = True
    return t


def _k3(c, dev):
    """The K rows as the [KV, rows, HD] cache view attention_strided takes (same memory)."""
    k = dev["k"]
    return k.as_strided((c.Hkv, k.shape[0], c.HD), (c.HD, k.stride(0), 1))


def _launch(d, dev, items=None, prefix="case", q_block=None, plain_base=False):
    """The case's entry into a NaN-filled buffer -> the buffer [rows, Hq*HD + OPAD].  prefix: the prefix ranges of `items` ("case": the
    case's own; None: launched without)."""
    from vlm_fo1_amd import ops
    c = d["case"]
    scale = c.HD ** -0.5
    qb = q_block or c.q_block
    if items is None and d.get("items") is not None:
        items = d["items"] if qb == c.q_block else ops.make_items(d["segs"], "cpu", causal=c.causal, block=qb)
    buf = _buf(d) if not plain_base else torch.full((d["N"], c.Hq * c.HD + OPAD), float("nan"), dtype=torch.bfloat16, device="cuda")
    out = buf[:, :c.Hq * c.HD]
    r = c.route
    if r in ("fwd16", "fwd32"):
        ops.attention(dev["q"], dev["k"], dev["vt"], _items(items, qb), c.Hq, c.Hkv, c.HD, scale, c.causal, out=out, qk_head_stride=dev["hs"])
    elif r in ("prefix16", "prefix32"):
        it = _items(items, qb)
        if isinstance(prefix, str):
            prefix = d["items_prefix"]
        pr = None if prefix is None else prefix.contiguous().cuda()
        ops.attention_strided(dev["q"], 0, _k3(c, dev), dev["vt"], it, c.Hq, c.Hkv, c.HD, scale, c.causal, out=out, prefix_ranges=pr)
    elif r == "rowbase":
        it = _items(items, qb)
        if plain_base:
            ops.attention_strided(dev["q"], 0, _k3(c, dev), dev["vt"], it, c.Hq, c.Hkv, c.HD, scale, c.causal, out=out)
        else:
            base = torch.tensor([c.row_base], dtype=torch.int32, device="cuda")
            ops.attention_strided(dev["q"][c.row_base:], 0, _k3(c, dev), dev["vt"], it, c.Hq, c.Hkv, c.HD, scale, c.causal, out=out, q_row_base=base)
    elif r == "win1":
        ops.attention_windows(dev["q"], dev["k"], dev["vt"], _items(items, 64, single_tile=True), c.Hq, c.HD, scale, qk_head_stride=dev["hs"], out=out)
    elif r == "swin":
        ops.attention_window_bias(dev["q"], dev["k"], dev["vt"], _items(items, qb), c.Hq, c.HD, scale, dev["bias"], c.ws, c.shift, c.nwy, c.nwx, out=out)
    elif r == "davit":
        ops.window_attention(dev["qkv"], c.Hq * c.HD, c.Hq, c.segs[0], scale, out=out)
    elif r == "davit_map":
        (H, W), B = c.sizes[0], len(c.sizes)
        ops.window_attention_map(dev["qkv"], c.Hq * c.HD, c.Hq, C.MAP_WS, ops.Grid(H, W, B), dev["pad_row"], scale, out=out)
    elif r == "davit_var":
        ws, rows, r0, w0 = C.MAP_WS, [], 0, 0
        for H, W in c.sizes:
            nwy, nwx = -(-H // ws), -(-W // ws)
            rows.append((r0, H, W, w0, nwy, nwx))
            r0 += H * W
            w0 += nwy * nwx * ws * ws
        sg = ops.ImgSegs(rows, "cuda", max(H * W for H, W in c.sizes), r0, max(a[4] * a[5] * ws * ws for a in rows), w0)
        ops.window_attention_map(dev["qkv"], c.Hq * c.HD, c.Hq, ws, sg, dev["pad_row"], scale, out=out)
    else:
        raise ValueError(r)
    torch.cuda.synchronize()
    return buf


def _record(c, ratio):
    WORST[c.route] = max(WORST.get(c.route, 0.0), ratio)
    print(f"\nWORST {c.route} {c.name}: {ratio:.3f} (route so far {WORST[c.route]:.3f})")


@pytest.mark.parametrize("case", C.SWEEP, ids=lambda c: c.name)
def test_prefill_attention_route_against_fp64_and_bitwise_invariants(case, product_library):
    d = C.build(case)
    dev = C.to_device(d)
    ref = C.reference(d)
    got = _launch(d, dev)
    _record(case, C.check(got, d, case.name, ref=ref))
    assert _same(_launch(d, dev), got), f"{case.name}: a second launch gives other bits"
    if d.get("items") is not None:
        items = d["items"]
        perm = torch.randperm(items.shape[0], generator=torch.Generator().manual_seed(case.seed))
        pr = d.get("items_prefix")
        again = _launch(d, dev, items=items[perm], prefix=None if pr is None else pr[perm])
        assert _same(again, got), f"{case.name}: a permuted item list gives other bits"
    if case.route == "fwd16":
        for qb in (16, 32):
            other = _launch(d, dev, q_block=qb)
            _record(case, C.check(other, d, f"{case.name} q_block {qb}", ref=ref))
            assert _same(other, got), f"{case.name}: q_block {qb} gives other bits than {case.q_block}"
    if case.route == "win1":
        from vlm_fo1_amd import ops
        fwd = _buf(d)
        ops.attention(dev["q"], dev["k"], dev["vt"], _items(d["items"], 64), case.Hq, case.Hkv, case.HD, case.HD ** -0.5, False,
                      out=fwd[:, :case.Hq * case.HD], qk_head_stride=dev["hs"])
        torch.cuda.synchronize()
        assert _same(fwd, got), f"{case.name}: attn_win1 differs from attn_fwd_kernel<80, 4>"
    if case.route in ("prefix16", "prefix32"):
        pr = d["items_prefix"]
        empty = pr[:, 0] >= pr[:, 1]
        assert empty.any() and (~empty).any()
        alone = _launch(d, dev, items=d["items"][empty], prefix=None)
        rows = torch.zeros(got.shape[0], dtype=torch.bool)
        for q0, q1, _, _ in d["items"][empty].tolist():
            rows[q0:q1] = True
        assert _same(alone[rows.cuda()], got[rows.cuda()]), f"{case.name}: empty-prefix items differ from the launch without prefix ranges"
        assert torch.isnan(alone[~rows.cuda()].float()).all()
    if case.route == "rowbase":
        plain = _launch(d, dev, plain_base=True)
        assert _same(plain[case.row_base:], got), f"{case.name}: the q_row_base launch differs from the plain launch on shifted rows"


def _attn_rows(launch):
    """One launch under the profile -> the names of its attn_ rows in first-launch order (each launched once)."""
    from vlm_fo1_amd import lib as L
    L.profile_rows()
    L.profile(True)
    try:
        launch()
        rows = [r for r in L.profile_rows() if r["name"].startswith("attn_")]
    finally:
        L.profile(False)
    assert all(r["calls"] == 1 for r in rows), rows
    return [r["name"] for r in rows]


def _case(name):
    return next(c for c in C.SWEEP if c.name == name)


# the smallest case of every route through attention.hip -> its one profile row
LAUNCH_ROWS = {"fwd16-hd128-12x2-causal": "attn_fwd", "prefix16-hd128-16x2-causal": "attn_fwd", "swin-ws12-s0-1x1-h6-q64": "attn_fwd",
               "rowbase-base0": "attn_fwd", "fwd32-hd128-q256-4x4-causal": "attn_fwd32", "prefix32-hd128-16x2-causal": "attn_fwd32",
               "win1-n1-packed": "attn_win1"}


def test_launch_rows_per_route(product_library):
    """The kernel each route launches, by its profile row: one launch of the smallest case of the route on the product library; then, on the
    test build with fo1_gemm_profile_shapes(1), the row of the 16x16 and of the 32x32 form states head dim, query block, item and head counts."""
    from vlm_fo1_amd import lib as L, ops
    for name, row in LAUNCH_ROWS.items():
        d = C.build(_case(name))
        dev = C.to_device(d)
        assert _attn_rows(lambda: _launch(d, dev)) == [row], name
    with L.use_ab() as ab:
        L.check(ab.fo1_gemm_profile_shapes(1), "profile_shapes")
        try:
            for name, kernel, qb in (("fwd16-hd128-12x2-causal", "attn_fwd", 16), ("fwd16-hd128-12x2-causal", "attn_fwd", 64),
                                     ("fwd32-hd128-q128-16x2-causal", "attn_fwd32", 128)):
                c = _case(name)
                d = C.build(c)
                dev = C.to_device(d)
                n = ops.make_items(d["segs"], "cpu", causal=c.causal, block=qb).shape[0]
                want = f"{kernel} hd{c.HD} q{qb} items{n} heads{c.Hq}" + (" causal" if c.causal else "")
                assert _attn_rows(lambda: _launch(d, dev, q_block=qb)) == [want], name
        finally:
            ab.fo1_gemm_profile_shapes(0)
