"""Decode attention per launch route (attention_decode_batch_impl, csrc/attention.hip) against the fp64 reference of
tests/decode_attention_cases.py, with the output pre-filled with NaN so that an unwritten row fails:

  route                                          B                max_kv_len
  <= 16 sequences, 64-key chunks + combine       1, 2, 16         65, 192, 1025, 2048
  <= 32 sequences, one chunk (n_chunks == 1)     1, 16, 17, 25, 32  1, 17, 63, 64
  17..32 sequences, two-tile items + combine     17, 25, 32       65, 128, 192, 2048, 2112
  > 32 sequences, one 1024-key chunk             33, 64, 128      1, 64, 1024
  > 32 sequences, 1024-key chunks + combine      33, 128          1025, 2048, 4096
  partials + fo1_gemv_attn_combine_bf16          1, 2             1, 64, 65, 2048
  fo1_attention_decode_bf16 (device length)      1                n = 1, 63, 64, 65, 1024, 4096

and the bit-for-bit claims of the host code: a sequence's row does not depend on the batch within a route, on the bound within a batch
class (one chunk vs split + combine: o / l == the combine of one partial), on the tiles per item at 17..32 sequences, nor on eager vs
graph replay after the state advanced on the device."""
import pytest
import torch

import decode_attention_cases as C

pytestmark = pytest.mark.gpu

HD = C.HD


def _run(dev, c, bound, B=None, rows=None):
    """attention_decode_batch into a NaN-filled output (padded stride where c.pad) -> [B, Hq*HD] view."""
    from vlm_fo1_amd import ops
    q, st = dev["q"], dev["state"]
    if rows is not None:
        q, st = q[rows[0]:rows[1]], st[rows[0]:rows[1]].contiguous()
    B = q.shape[0]
    buf = torch.full((B, c.Hq * HD + (64 if c.pad else 0)), float("nan"), dtype=torch.bfloat16, device="cuda")
    out = buf[:, :c.Hq * HD]
    ops.attention_decode_batch(q, dev["kc"], dev["vt"], st, bound, c.Hq, c.Hkv, HD, HD ** -0.5, out=out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", C.SWEEP, ids=lambda c: c.name)
def test_decode_attention_route_against_fp64_and_bitwise_invariants(case, product_library):
    d = C.build(case)
    dev = C.to_device(d)
    ref = C.reference(d)
    got = _run(dev, case, case.max_kv_len)
    C.check(got, d, f"{case.name}", ref=ref)
    # bound invariance: another bound of the same batch class (one chunk <-> split + combine, 64 <-> 2048 keys, 1024 <-> 4096)
    alt = C.bound_class_alternative(case)
    assert torch.equal(_run(dev, case, alt), got), f"{case.name}: max_kv_len {alt} gives other bits than {case.max_kv_len}"
    # batch invariance within the route: every sequence alone (B = 1) at the same bound
    if 16 <= case.B <= 32:
        for b in range(case.B):
            alone = _run(dev, case, case.max_kv_len, rows=(b, b + 1))
            assert torch.equal(alone[0], got[b]), f"{case.name}: sequence {b} (ctx {d['ctx'][b]}) alone differs from its row in the batch"
    elif case.B > 32:
        for lo, hi in ((0, 33), (case.B - 33, case.B)):
            assert torch.equal(_run(dev, case, case.max_kv_len, rows=(lo, hi)), got[lo:hi]), f"{case.name}: rows {lo}..{hi} as a batch of 33"


@pytest.mark.parametrize("case", C.GEMV_CASES, ids=lambda c: c.name)
def test_partials_and_o_projection_combine_equal_the_combine_launch_bitwise(case, product_library):
    """fo1_attention_decode_batch_partials_bf16 + fo1_gemv_attn_combine_bf16 (M <= 2: the o-projection sums the partials in its prologue) ==
    fo1_attention_decode_batch_bf16 + fo1_gemv_batch_bf16 at the same bound, bit for bit (one shared combine routine), at short bounds
    (1 and 64: one chunk; 65: two) and at 2048 — with the attention rows of the second form within the fp64 bound, so the first is pinned to the
    reference through them."""
    from vlm_fo1_amd import ops
    d = C.build(case)
    dev = C.to_device(d)
    H, KV, D = case.Hq, case.Hkv, 2048
    g = torch.Generator().manual_seed(77 + case.seed)
    wo = (torch.randn(D, H * HD, generator=g) * 0.03).bfloat16().cuda()
    res = torch.randn(case.B, D, generator=g).bfloat16().cuda()
    att = _run(dev, case, case.max_kv_len)
    C.check(att, d, case.name)
    want = ops.gemv_batch(att, wo, residual=res)
    part, pstride, chunk = ops.attention_decode_batch_partials(dev["q"], dev["kc"], dev["vt"], dev["state"], case.max_kv_len, H, KV, HD, HD ** -0.5)
    got = ops.gemv_attn_combine(part, pstride, dev["state"], chunk, H, KV, wo, residual=res)
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"{case.name}: fused o-projection differs from combine + gemv (max |d| {(got.float() - want.float()).abs().max().item():.4g})"


@pytest.mark.parametrize("case", C.SINGLE_CASES, ids=lambda c: c.name)
def test_single_sequence_decode_attention_against_fp64(case, product_library):
    """fo1_attention_decode_bf16 (keys [0, n), n on the device) at a 4096-key bound and at the bound n itself: same bits, within TOL."""
    from vlm_fo1_amd import ops
    d = C.build(case)
    dev = C.to_device(d)
    n = d["ctx"][0]
    kv_len = torch.tensor([n], dtype=torch.int32, device="cuda")
    q = dev["q"].contiguous()
    outs = []
    for bound in (case.max_kv_len, n):
        out = torch.full((1, case.Hq * HD), float("nan"), dtype=torch.bfloat16, device="cuda")
        ops.attention_decode(q, dev["kc"], dev["vt"], kv_len, bound, case.Hq, case.Hkv, HD, HD ** -0.5, out=out)
        torch.cuda.synchronize()
        outs.append(out)
    C.check(outs[0], d, case.name)
    assert torch.equal(outs[0], outs[1]), f"{case.name}: bound {case.max_kv_len} and {n} differ"


def _attn_rows(launch):
    """One launch under the profile -> the names of its attn_ rows in first-launch order (each launched once)."""
    from vlm_fo1_amd import lib as L
    L.profile_rows()
    L.profile(True)
    try:
        launch()
        torch.cuda.synchronize()
        rows = [r for r in L.profile_rows() if r["name"].startswith("attn_")]
    finally:
        L.profile(False)
    assert all(r["calls"] == 1 for r in rows), rows
    return [r["name"] for r in rows]


LAUNCH_ROWS = {"split64-B1-L65": ["attn_decode_split", "attn_decode_combine"], "two_tile-B17-L65": ["attn_decode_split", "attn_decode_combine"],
               "pool_split-B33-L1025": ["attn_decode_split", "attn_decode_combine"], "single-n1": ["attn_decode_split", "attn_decode_combine"],
               "one_chunk-B1-L1": ["attn_decode_one_chunk"], "pool_one-B33-L1": ["attn_decode_one_chunk"],
               "gemv-B1-L65": ["attn_decode_split"]}


def test_launch_rows_per_route(product_library):
    """The kernels each route launches, by their profile rows: the smallest case of every route (16 query / 2 KV heads), run once."""
    from vlm_fo1_amd import ops
    for prefix, want in LAUNCH_ROWS.items():
        c = next(c for c in C.ALL_CASES if c.name == prefix or c.name.startswith(prefix + "-h16x2"))
        dev = C.to_device(C.build(c))
        if c.route == "single":
            kv_len = torch.tensor([1], dtype=torch.int32, device="cuda")
            run = lambda: ops.attention_decode(dev["q"].contiguous(), dev["kc"], dev["vt"], kv_len, c.max_kv_len, c.Hq, c.Hkv, HD, HD ** -0.5)
        elif c.route == "gemv":
            run = lambda: ops.attention_decode_batch_partials(dev["q"], dev["kc"], dev["vt"], dev["state"], c.max_kv_len, c.Hq, c.Hkv, HD, HD ** -0.5)
        else:
            run = lambda: _run(dev, c, c.max_kv_len)
        assert _attn_rows(run) == want, c.name


def test_tiles_per_item_do_not_change_the_bits(ab_library):
    """At 25 sequences an item walks 1 / 2 / 3 / 8 tiles of 64 keys (fo1_attention_decode_set_small_chunk(1 .. 8)): the same bits, and within
    the fp64 bound, at one-chunk, odd and even chunk counts."""
    from vlm_fo1_amd import lib as L
    for c in C.TILES_CASES:
        bound = c.max_kv_len
        d = C.build(c)
        dev = C.to_device(d)
        outs = {}
        try:
            for t in (1, 2, 3, 8):
                L.check(L.load().fo1_attention_decode_set_small_chunk(t), "set_small_chunk")
                outs[t] = _run(dev, c, bound)
        finally:
            L.load().fo1_attention_decode_set_small_chunk(2)
        C.check(outs[2], d, f"{c.name} tiles 2")
        for t in (1, 3, 8):
            assert torch.equal(outs[t], outs[2]), f"{c.name}: {t} tiles per item differ from 2"


ALT_CASES = [c for c in C.SWEEP if c.Hq == 16 and c.Hkv == 2 and c.B in (1, 16, 25, 33)]


@pytest.mark.parametrize("case", ALT_CASES, ids=lambda c: c.name)
def test_alternative_decode_kernels_against_fp64(case, ab_library):
    """The A/B decode kernels (fo1_attention_decode_set_impl 1: one workgroup per (KV head, sequence), 2: wave-split tiles) and the 128- and
    1024-key small chunks meet the same fp64 bound (finished sequences: zero rows); with an A/B kernel selected the partials-only entry
    still gives the split kernel's partials."""
    from vlm_fo1_amd import lib as L
    d = C.build(case)
    dev = C.to_device(d)
    ref = C.reference(d)
    from vlm_fo1_amd import ops

    def partials():                     # the partials-only entry + the o-projection that sums them (M <= 2)
        part, pstride, chunk = ops.attention_decode_batch_partials(dev["q"], dev["kc"], dev["vt"], dev["state"], case.max_kv_len, case.Hq,
                                                                   case.Hkv, HD, HD ** -0.5)
        return ops.gemv_attn_combine(part, pstride, dev["state"], chunk, case.Hq, case.Hkv, wo).clone()

    if case.B <= 2:
        wo = (torch.randn(2048, case.Hq * HD, generator=torch.Generator().manual_seed(5)) * 0.03).bfloat16().cuda()
        want = partials()
    for impl in (1, 2):
        try:
            L.check(L.load().fo1_attention_decode_set_impl(impl), "set_impl")
            got = _run(dev, case, case.max_kv_len)
            if case.B <= 2:             # the A/B kernels serve the combine launch's form only: the partials keep the split kernel's layout
                assert torch.equal(partials(), want), f"{case.name} impl {impl}: the partials entry changed"
        finally:
            L.load().fo1_attention_decode_set_impl(0)
        C.check(got, d, f"{case.name} impl {impl}", ref=ref)
    if case.B <= 32:
        for keys in (128, 1024):
            try:
                L.check(L.load().fo1_attention_decode_set_small_chunk(keys), "set_small_chunk")
                got = _run(dev, case, case.max_kv_len)
            finally:
                L.load().fo1_attention_decode_set_small_chunk(64)
            C.check(got, d, f"{case.name} small chunk {keys}", ref=ref)


def test_graph_replay_after_the_state_advanced_on_the_device(product_library):
    """One attention_decode_batch at 25 sequences captured on a single stream; the state then advances on the device (contexts + 1 and + 64,
    one sequence finished): the replay gives the eager bits on the new state, within the fp64 bound."""
    from vlm_fo1_amd import ops
    c = C.GRAPH_CASE
    d = C.build(c)
    dev = C.to_device(d)
    H, KV = c.Hq, c.Hkv
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    buf = torch.full((c.B, H * HD + 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    out = buf[:, :H * HD]
    with torch.cuda.stream(s):      # warm-up on the capture stream: its workspace exists before the capture
        ops.attention_decode_batch(dev["q"], dev["kc"], dev["vt"], dev["state"], c.max_kv_len, H, KV, HD, HD ** -0.5, out=out)
    s.synchronize()
    C.check(out, d, "eager before capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.attention_decode_batch(dev["q"], dev["kc"], dev["vt"], dev["state"], c.max_kv_len, H, KV, HD, HD ** -0.5, out=out)
    st = dev["state"]
    adv = torch.tensor([1 if b % 2 == 0 else 64 for b in range(c.B)], dtype=torch.int32, device="cuda")
    st[:, 0] += adv
    st[3, 3] = 1
    st[7, 3] = 0                                        # a finished sequence comes back (its rows are live again)
    buf.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    new_state = st.cpu()
    eager = _run(dev, c, c.max_kv_len)
    assert torch.equal(replayed, eager), "graph replay differs from the eager launch on the advanced state"
    C.check(replayed, d, "replay on the advanced state", state=new_state)
