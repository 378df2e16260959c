"""The decode-step linears per launch route (csrc/decode_mfma.hip, csrc/gemv.hip), element by element against the fp64 reference of
tests/decode_linear_cases.py.

Every case of SWEEP runs into canary-framed buffers (NaN around the operands, the canary bit pattern in every output element and in the whole
K and V^T caches, padded strides, spare rows) and is held to:
  * the route: on the product library the profile row is the kernel name, on the A/B library with fo1_gemm_profile_shapes(1) it is the
    routing model's Route.shape_row() (column class by M, rows per unit, NB, 1p / mp, h / r / x; gemv.hip: ks0 / ks1); the four refusals
    return FO1_ERR_ARG and leave every buffer untouched;
  * the per-element bound |got - ref| <= bound for the output, the K-cache rows and the V^T columns (reference: float64 on the CPU);
  * the canary: nothing outside [0, M) x [0, n_out) written, nothing inside left unwritten; in the caches exactly the rows / columns
    state[m][0] of the M sequences, every element of them; no NaN anywhere;
  * a second launch gives the same bits; on the A/B library fo1_gemv_batch_set_impl(3) and (5) give the bits of the default.
Bitwise claims of the code: row m of a launch == the same row launched at every other M of M_LIST (all three column classes), on every
distinct shape of the sweep; the o-projection with the attention combine in its prologue == combine launch + fo1_gemv_batch_bf16.

Each case prints "ROUTE <label> <case>: <row> worst <max |got - ref| / bound>"; test_zz_route_summary prints the worst per route."""
from dataclasses import replace

import pytest
import torch

import decode_linear_cases as C

pytestmark = pytest.mark.gpu

WORST = {}          # label -> (worst ratio, row observed)
BATCH = [c for c in C.SWEEP if c.entry == "batch" and not c.refused]
GEMV = [c for c in C.SWEEP if c.entry in ("gemv", "handoff")]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16)


def _launch(d, dev, M=None):
    """One launch of the case's entry on its first M sequences into fresh canary buffers -> (out buffer, K cache, V^T cache)."""
    from vlm_fo1_amd import ops
    c = d["case"]
    M = c.M if M is None else M
    buf = dev["out"].clone()
    x, w = dev["x"][:M, :c.K], dev["W"][:c.N, :c.K]
    bias = dev["bias"][:c.N] if "bias" in dev else None
    res = dev["res"][:M, :c.N] if "res" in dev else None
    nw = dev["nw"][:c.K] if "nw" in dev else None
    kc = vt = None
    if c.entry == "batch":
        qkv = None
        if c.mode == C.QKV:
            kc, vt = dev["kc"].clone(), dev["vt"].clone()
            qkv = dict(n_q=c.n_q, n_kv=c.n_kv, cos=dev["cos"], sin=dev["sin"], state=dev["state"][:M].contiguous(), kcache=kc[:, :C.CACHE_ROWS],
                       vtcache=vt[:, :C.CACHE_ROWS])
        ops.gemv_batch(x, w, bias, res, c.mode, nw, C.NORM_EPS, out=buf[:M, :c.n_out], qkv=qkv)
    elif c.entry == "gemv":
        ops.gemv(x, w, bias, res, c.act, nw, C.NORM_EPS, out=buf[:M, :c.n_out])
    else:
        ops.gemm(x, w, bias, res, c.act, out=buf[:M, :c.n_out])
    torch.cuda.synchronize()
    return buf, kc, vt


def _profiled(fn):
    """-> (fn's result, [profile row names in first-launch order])."""
    from vlm_fo1_amd import lib as L
    L.profile_rows()
    L.profile(True)
    try:
        res = fn()
        rows = L.profile_rows()
    finally:
        L.profile(False)
    assert all(r["calls"] == 1 for r in rows), rows
    return res, [r["name"] for r in rows]


def _check(d, got3, what, refs):
    """Canary + no NaN + per-element bound on every output -> worst |got - ref| / bound."""
    c = d["case"]
    buf, kc, vt = got3
    C.check_canary(buf, d, what)
    if c.mode == C.QKV:
        C.check_cache_canary(kc, vt, d, what)
        assert not torch.isnan(kc).any() and not torch.isnan(vt).any(), f"{what}: NaN in a cache"
    assert not torch.isnan(buf).any(), f"{what}: NaN in the output buffer"
    if "rb" not in refs:
        refs["rb"] = C.reference_and_bound(d)
    got = C.gather_outputs(d, buf, kc, vt)
    worst = 0.0
    for name, (ref, bound) in refs["rb"].items():
        ratio = torch.nan_to_num((got[name] - ref).abs() / bound, nan=float("inf"))
        w = ratio.max().item()
        if w > 1.0:
            idx = ratio.flatten().argmax().item()
            where = [int(v) for v in torch.unravel_index(torch.tensor(idx), ratio.shape)]
            raise AssertionError(f"{what}: {int((ratio > 1).sum())} elements of '{name}' beyond the bound, worst {w:.3g} x at {where}: got "
                                 f"{got[name].flatten()[idx].item():.6g}, ref {ref.flatten()[idx].item():.6g}, bound {bound.flatten()[idx].item():.3g}")
        worst = max(worst, w)
    return worst


def _same(a3, b3, what):
    for a, b, name in zip(a3, b3, ("output", "K cache", "V^T cache")):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), f"{what}: other bits in the {name}"


def _record(c, row, worst):
    w, _ = WORST.get(c.claim, (0.0, None))
    WORST[c.claim] = (max(w, worst), row)
    print(f"\nROUTE {c.claim} {c.name}: {row} worst {worst:.3f} (route so far {WORST[c.claim][0]:.3f})")


def _restore(lib):
    lib.fo1_gemv_batch_set_impl(1)
    lib.fo1_gemm_profile_shapes(0)
    lib.fo1_profile_enable(0)


def _route_and_bound(case, impls):
    """The per-case body: product library (kernel name, bound, canary, determinism), then the A/B library (shape row, bound, half switches)."""
    from vlm_fo1_amd import lib as L
    d = C.build(case)
    r = d["route"]
    assert r.label() == case.claim
    dev = C.to_device(d)
    got, rows = _profiled(lambda: _launch(d, dev))
    assert rows == [r.product_row()], f"{case.name}: launched {rows}, the routing model predicts {[r.product_row()]}"
    refs = {}
    _record(case, rows[0], _check(d, got, case.name, refs))
    _same(_launch(d, dev), got, f"{case.name}: a second launch")
    with L.use_ab() as ab:
        try:
            L.check(ab.fo1_gemm_profile_shapes(1), "profile_shapes")
            agot, arows = _profiled(lambda: _launch(d, dev))
            want = r.shape_row(case.M, case.N, case.K, case.act)[:47]
            assert arows == [want], f"{case.name}: the A/B library launched {arows}, the routing model predicts {[want]}"
            _record(case, arows[0], _check(d, agot, case.name + " (A/B library)", refs))
            _same(agot, got, f"{case.name}: the A/B library against the product library")
            ab.fo1_gemm_profile_shapes(0)
            for impl in impls:
                L.check(ab.fo1_gemv_batch_set_impl(impl), "set_impl")
                _same(_launch(d, dev), got, f"{case.name}: fo1_gemv_batch_set_impl({impl})")
        finally:
            _restore(ab)


@pytest.mark.parametrize("case", BATCH, ids=lambda c: c.name)
def test_gemv_batch_route_against_fp64(case, product_library):
    _route_and_bound(case, (3, 5))


@pytest.mark.parametrize("case", GEMV, ids=lambda c: c.name)
def test_gemv_route_against_fp64(case, product_library):
    _route_and_bound(case, ())


@pytest.mark.parametrize("case", [c for c in C.SWEEP if c.refused], ids=lambda c: c.name)
def test_refused_shapes_return_err_arg_and_write_nothing(case, product_library):
    from vlm_fo1_amd import lib as L
    d = C.build(case)
    assert d["route"].kind == "refused" and d["route"].label() == case.claim
    dev = C.to_device(d)
    for lib_ctx in (None, L.use_ab):
        before = {k: dev[k].clone() for k in ("out", "kc", "vt") if k in dev}

        def run():
            with pytest.raises(L.Fo1Error, match=r"rc=-1"):       # FO1_ERR_ARG
                _launch_into(d, dev)

        if lib_ctx is None:
            run()
        else:
            with lib_ctx():
                run()
        torch.cuda.synchronize()
        for k, v in before.items():
            assert torch.equal(_bits(dev[k]), _bits(v)) and (_bits(dev[k]) == C.CANARY16).all(), f"{case.name}: the refused launch wrote into '{k}'"
    print(f"\nROUTE {case.claim} {case.name}: FO1_ERR_ARG, buffers untouched")


def _launch_into(d, dev):
    """As _launch, but into the buffers of `dev` themselves (the refusal test looks at them afterwards)."""
    from vlm_fo1_amd import ops
    c = d["case"]
    qkv = None
    if c.mode == C.QKV:
        qkv = dict(n_q=c.n_q, n_kv=c.n_kv, cos=dev["cos"], sin=dev["sin"], state=dev["state"], kcache=dev["kc"][:, :C.CACHE_ROWS], vtcache=dev["vt"][:, :C.CACHE_ROWS])
    ops.gemv_batch(dev["x"][:c.M, :c.K], dev["W"][:c.N, :c.K], dev["bias"][:c.N] if "bias" in dev else None, None, c.mode,
                   dev["nw"][:c.K] if "nw" in dev else None, C.NORM_EPS, out=dev["out"][:c.M, :c.n_out], qkv=qkv)


def _shapes():
    """Every distinct (mode, N, K, operands) of the batch cases, at the largest M the dispatch launches it with."""
    seen = {}
    for c in BATCH:
        key = (c.mode, c.N, c.K, c.norm, c.n_q)
        ms = [m for m in C.M_LIST if C.route_batch(m, c.N, c.K, c.mode, c.norm, 3, c.n_q, c.n_kv).kind == "mfma"]
        if key not in seen:
            seen[key] = replace(c, name=f"rows-{C.MODE_NAME[c.mode]}-{c.N}x{c.K}{'-norm' if c.norm else ''}", M=max(ms), bias=True,
                                res=c.mode == C.PLAIN, ldr_pad=4, ldc_pad=8)
    return list(seen.values())


@pytest.mark.parametrize("case", _shapes(), ids=lambda c: c.name)
def test_a_sequence_gets_the_same_bits_in_every_batch(case, product_library):
    """The K split is fixed by the shape alone: row m of a launch of M sequences has the bits of row m in every other launch — 8-, 16- and
    32-column classes, 8- / 16-row units, x in LDS or in registers, own-row staging (XR32)."""
    d = C.build(case)
    dev = C.to_device(d)
    ref = _launch(d, dev)
    labels = set()
    for M in C.M_LIST:
        r = C.route_batch(M, case.N, case.K, case.mode, case.norm, 3, case.n_q, case.n_kv)
        if r.kind != "mfma" or M > case.M:
            continue
        labels.add(r.label())
        got = _launch(d, dev, M)
        assert torch.equal(_bits(got[0][:M, :case.n_out]), _bits(ref[0][:M, :case.n_out])), \
            f"{case.name}: rows {(got[0][:M, :case.n_out] != ref[0][:M, :case.n_out]).any(1).nonzero().flatten().tolist()} at M = {M} ({r.label()}) differ from M = {case.M}"
        if case.mode == C.QKV:
            pos = d["state"][:M, 0].long().cuda()
            assert torch.equal(_bits(got[1][:, pos]), _bits(ref[1][:, pos])), f"{case.name}: K rows at M = {M} ({r.label()}) differ from M = {case.M}"
            assert torch.equal(_bits(got[2][:, pos]), _bits(ref[2][:, pos])), f"{case.name}: V^T columns at M = {M} ({r.label()}) differ from M = {case.M}"
    print(f"\n{case.name}: rows bit-identical across {sorted(labels)}")


@pytest.mark.parametrize("case", [c for c in C.SWEEP if c.entry == "combine"], ids=lambda c: c.name)
def test_o_projection_with_the_combine_in_its_prologue_against_fp64(case, product_library):
    """fo1_gemv_attn_combine_bf16 at N = 20: the fp64 projection of the rows fo1_attention_decode_batch_bf16 writes, and the bits of that
    launch followed by fo1_gemv_batch_bf16."""
    from vlm_fo1_amd import lib as L, ops
    d = C.build(case)
    r = d["route"]
    H, KV, HD, slot = case.n_q, case.n_kv, 128, 256
    g = torch.Generator().manual_seed(case.seed)
    lens = [65] if case.M == 1 else [1, 200]
    kc = torch.randn(KV, case.M * slot, HD, generator=g).bfloat16().cuda()
    vt = torch.randn(KV * HD, case.M * slot, generator=g).bfloat16().cuda()
    q = torch.randn(case.M, H * HD, generator=g).bfloat16().cuda()
    state = torch.zeros(case.M, 8, dtype=torch.int32)
    for b, n in enumerate(lens):
        state[b, 2] = b * slot
        state[b, 0] = b * slot + n - 1
    state = state.cuda()
    scale = HD ** -0.5
    att = ops.attention_decode_batch(q, kc, vt, state, slot, H, KV, HD, scale)
    torch.cuda.synchronize()
    d["x"] = att.cpu()
    dev = C.to_device(d)
    w, res = dev["W"][:case.N, :case.K], dev["res"][:case.M, :case.N]
    want = dev["out"].clone()
    ops.gemv_batch(att, w, residual=res, out=want[:case.M, :case.N])

    def fused():
        part, pstride, chunk = ops.attention_decode_batch_partials(q, kc, vt, state, slot, H, KV, HD, scale)
        L.profile_rows()           # (the partials launch is not what the row check is about)
        buf = dev["out"].clone()
        ops.gemv_attn_combine(part, pstride, state, chunk, H, KV, w, residual=res, out=buf[:case.M, :case.N])
        torch.cuda.synchronize()
        return buf

    got, rows = _profiled(fused)
    assert rows == [r.product_row()], rows
    refs = {}
    _record(case, rows[0], _check(d, (got, None, None), case.name, refs))
    _record(case, rows[0], _check(d, (want, None, None), case.name + " (combine launch + gemv_batch)", refs))
    assert torch.equal(_bits(got), _bits(want)), f"{case.name}: the fused o-projection differs from combine + gemv_batch"
    assert torch.equal(_bits(fused()), _bits(got)), f"{case.name}: a second launch gives other bits"
    with L.use_ab() as ab:
        try:
            L.check(ab.fo1_gemm_profile_shapes(1), "profile_shapes")
            agot, arows = _profiled(fused)
            assert arows == [r.shape_row(case.M, case.N, case.K)[:47]], arows
            assert torch.equal(_bits(agot), _bits(got))
        finally:
            _restore(ab)


def test_zz_route_summary():
    print()
    for label in sorted(WORST):
        w, row = WORST[label]
        print(f"SUMMARY {label}: {row} worst {w:.3f} of the bound")
    if WORST:      # (run alone, there is nothing to summarise)
        assert max(w for w, _ in WORST.values()) <= 1.0
    if len(WORST) >= 39:
        missing = {k for k in C.reachable_labels() if not k.startswith("refused")} - set(WORST)
        assert not missing, f"routes the sweep did not exercise: {missing}"
