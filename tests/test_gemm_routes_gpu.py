"""The bf16 tile GEMM per launch route (csrc/gemm.hip), element by element against the fp64 reference of tests/gemm_route_cases.py.

Every case of SWEEP runs into canary-framed buffers (NaN around the operands, a canary bit pattern in every output element, padded row
strides, spare rows / a spare plane) and is held to:
  * the route: the profile rows of the launch are the ones the routing model predicts — on the product library the kernel names
    (gemm_bt_ring<128,96,3>, gemm_bt_p4<256,256>, gemm_splitk_reduce exactly when planes are predicted, ...), and on the A/B library, without
    a pin and with fo1_gemm_profile_shapes(1), the row that states tile, split count and ring depth (the register kernels share one product
    row name; their tile is checked there).  Pinned cases run on the A/B library only, every switch restored afterwards;
  * the per-element bound |got - ref| <= bound[m, n] (gemm_route_cases.epilogue64), the reference computed in float64 on the device and its
    first, last and M-tile-boundary rows checked against the CPU's float64 product;
  * the canary: nothing outside [0, M) x [0, n_out) written, nothing inside left unwritten;
  * a second launch gives the same bits (fixed summation order).
Bit-for-bit claims of the code: fo1_gemm_bf16_wtiled == fo1_gemm_bf16 on the same tile; the <128, 96> SwiGLU tile == the 128 x 128 ring;
fo1_gemm_bf16 under split-K == the z-ordered fp32 sum of fo1_gemm_bf16_partials' planes through the same epilogue (no activation: bias,
residual, fp32 out) where both take the 64 x 128 ring with the same plane count.
The GEMV hand-off (M <= 4) is only asserted to happen here; tests/test_decode_linears_gpu.py (cases handoff-*) holds its results to the per-element bound.

Each case prints "ROUTE <claim> <case>: <profile rows> worst <max |got - ref| / bound>"; test_zz_route_summary prints the worst per route."""
import pytest
import torch

import gemm_route_cases as C

pytestmark = pytest.mark.gpu

WORST = {}          # claim -> (worst ratio, rows observed)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(d, dev, w_tiled=None):
    """One launch of the case's entry into a fresh canary buffer -> the buffer."""
    from vlm_fo1_amd import ops
    c = d["case"]
    buf = dev["out"].clone()
    a, w = dev["A"][:c.M, :c.K], dev["W"][:c.N, :c.K]
    bias = dev["bias"][:c.N] if "bias" in dev else None
    res = dev["res"][:c.M, :c.N] if "res" in dev else None
    if c.entry == "partials":
        eff = ops.gemm_partials(a, w, c.splits, buf)
        assert eff == d["route"].splits, f"{c.name}: {eff} planes, the model says {d['route'].splits}"
    elif c.entry == "wtiled":
        ops.gemm_wtiled(a, w_tiled if w_tiled is not None else ops.tile_weight(dev["W"][:c.N, :c.K].contiguous()), bias, res, c.act, out=buf[:c.M, :c.n_out])
    else:
        ops.gemm(a, w, bias, res, c.act, out=buf[:c.M, :c.n_out], out_f32=c.out_f32)
    torch.cuda.synchronize()
    return buf


def _profiled(d, dev):
    """-> (buffer, [profile row names in first-launch order])."""
    from vlm_fo1_amd import lib as L
    L.profile_rows()
    L.profile(True)
    try:
        buf = _run(d, dev)
        rows = L.profile_rows()
    finally:
        L.profile(False)
    assert all(r["calls"] == 1 for r in rows), rows
    return buf, [r["name"] for r in rows]


def _check(d, dev, buf, what, refs):
    """Canary + per-element bound -> worst |got - ref| / bound."""
    c = d["case"]
    C.check_canary(buf, d, what)
    if "ref" not in refs:
        ref, bound = C.reference_and_bound(d, device="cuda")
        rows = C.sample_rows(d)
        cref, cbound = C.reference_and_bound(d, device="cpu", rows=rows)
        off = ((ref[..., rows.cuda(), :].cpu() - cref).abs() / cbound).max().item()
        assert off <= 1e-3, f"{what}: the device's float64 reference is {off:.3g} of the bound off the CPU's on the sampled rows"
        refs["ref"], refs["bound"] = ref, bound
    ref, bound = refs["ref"], refs["bound"]
    got = (buf[:d["route"].splits] if c.entry == "partials" else buf[:c.M, :c.n_out]).double()
    ratio = (got - ref).abs() / bound
    worst = torch.nan_to_num(ratio, nan=float("inf")).max().item()
    if worst > 1.0:
        idx = torch.nan_to_num(ratio, nan=float("inf")).flatten().argmax().item()
        where = [int(x) for x in torch.unravel_index(torch.tensor(idx), ratio.shape)]
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} elements beyond the bound, worst {worst:.3g} x at {where}: got {got.flatten()[idx].item():.6g}, "
                             f"ref {ref.flatten()[idx].item():.6g}, bound {bound.flatten()[idx].item():.3g}")
    return worst


def _record(c, rows, worst):
    w, _ = WORST.get(c.claim, (0.0, None))
    WORST[c.claim] = (max(w, worst), rows)
    print(f"\nROUTE {c.claim} {c.name}: {rows} worst {worst:.3f} (route so far {WORST[c.claim][0]:.3f})")


def _set_pin(lib, pin):
    from vlm_fo1_amd import lib as L
    L.check(lib.fo1_gemm_set_variant(pin.staging, pin.tile), "variant")
    L.check(lib.fo1_gemm_set_splitk(pin.splitk), "splitk")
    L.check(lib.fo1_gemm_set_big_schedule(pin.sched), "schedule")
    L.check(lib.fo1_gemm_set_group_m(pin.group_m), "group_m")


def _restore(lib):
    lib.fo1_gemm_set_variant(0, 0)
    lib.fo1_gemm_set_splitk(0)
    lib.fo1_gemm_set_big_schedule(1)
    lib.fo1_gemm_set_group_m(0)
    lib.fo1_gemm_profile_shapes(0)
    lib.fo1_profile_enable(0)


def _shape_rows(d):
    c, r = d["case"], d["route"]
    return [r.shape_row(c.M, c.N, c.K)] + (["gemm_splitk_reduce"] if r.reduce else [])


def _plane_sum_epilogue(d, dev, planes):
    """The z-ordered fp32 plane sum through the no-activation epilogue, in torch (fp32 adds and round-to-nearest-even as the kernel's)."""
    c = d["case"]
    v = planes[0].clone()
    for z in range(1, planes.shape[0]):
        v += planes[z]
    if "bias" in dev:
        v += dev["bias"][:c.N].float()
    if c.out_f32:
        return v
    v = v.bfloat16()
    if "res" in dev:
        v = (v.float() + dev["res"][:c.M, :c.N].float()).bfloat16()
    return v


@pytest.mark.parametrize("case", [c for c in C.SWEEP if c.auto()], ids=lambda c: c.name)
def test_auto_dispatched_route_against_fp64(case, product_library):
    from vlm_fo1_amd import lib as L
    d = C.build(case)
    r = d["route"]
    assert C.claim_of(r) == case.claim
    dev = C.to_device(d)
    buf, rows = _profiled(d, dev)
    if r.kind == "gemv":
        assert rows and all("gemv" in n for n in rows), f"{case.name}: M <= 4 did not hand off to the GEMV: {rows}"
        C.check_canary(buf, d, case.name)
        _record(case, rows, 0.0)
        return
    assert rows == r.product_rows(), f"{case.name}: launched {rows}, the routing model predicts {r.product_rows()}"
    refs = {}
    _record(case, rows, _check(d, dev, buf, case.name, refs))
    assert torch.equal(_bits(_run(d, dev)), _bits(buf)), f"{case.name}: a second launch gives other bits"
    with L.use_ab() as ab:
        try:
            L.check(ab.fo1_gemm_profile_shapes(1), "profile_shapes")
            abuf, arows = _profiled(d, dev)
            assert arows == _shape_rows(d), f"{case.name}: the A/B library without pins launched {arows}, the routing model predicts {_shape_rows(d)}"
            _record(case, rows, _check(d, dev, abuf, case.name + " (A/B library)", refs))
            if (r.BM, r.BN) == (128, 96):
                ab.fo1_gemm_profile_shapes(0)
                _set_pin(ab, C.Pin(3, 1, 1))
                other = _run(d, dev)
                assert torch.equal(_bits(other), _bits(abuf)), f"{case.name}: the <128, 96> tile differs from the 128 x 128 ring"
        finally:
            _restore(ab)
    if r.reduce and case.act == C.ACT_NONE:
        pr = C.route_partials(case.M, case.N, case.K, r.splits)
        if (pr.BM, pr.BN, pr.splits, pr.kper) == (r.BM, r.BN, r.splits, r.kper):
            from vlm_fo1_amd import ops
            planes = torch.empty(r.splits, case.M, case.N, dtype=torch.float32, device="cuda")
            assert ops.gemm_partials(dev["A"][:case.M, :case.K], dev["W"][:case.N, :case.K], r.splits, planes) == r.splits
            want = _plane_sum_epilogue(d, dev, planes)
            assert torch.equal(_bits(want), _bits(buf[:case.M, :case.n_out].contiguous())), \
                f"{case.name}: split-K output differs from the z-ordered sum of fo1_gemm_bf16_partials' planes"
            print(f"{case.name}: == z-ordered sum of {r.splits} partial planes, bit for bit")


@pytest.mark.parametrize("case", [c for c in C.SWEEP if not c.auto()], ids=lambda c: c.name)
def test_pinned_route_against_fp64(case, ab_library):
    from vlm_fo1_amd import lib as L, ops
    d = C.build(case)
    r = d["route"]
    assert C.claim_of(r) == case.claim
    dev = C.to_device(d)
    lib = L.load()
    try:
        _set_pin(lib, case.pin)
        buf, rows = _profiled(d, dev)
        assert rows == r.product_rows(), f"{case.name}: launched {rows}, the routing model predicts {r.product_rows()}"
        refs = {}
        _record(case, rows, _check(d, dev, buf, case.name, refs))
        assert torch.equal(_bits(_run(d, dev)), _bits(buf)), f"{case.name}: a second launch gives other bits"
        L.check(lib.fo1_gemm_profile_shapes(1), "profile_shapes")
        sbuf, srows = _profiled(d, dev)
        assert srows == _shape_rows(d), f"{case.name}: launched {srows}, the routing model predicts {_shape_rows(d)}"
        assert torch.equal(_bits(sbuf), _bits(buf))
        if case.entry == "wtiled":
            lib.fo1_gemm_profile_shapes(0)
            _set_pin(lib, C.Pin(3, 1 if case.M > 64 else 2, 1))
            plain = dev["out"].clone()
            ops.gemm(dev["A"][:case.M, :case.K], dev["W"][:case.N, :case.K], dev["bias"][:case.N] if "bias" in dev else None,
                     dev["res"][:case.M, :case.N] if "res" in dev else None, case.act, out=plain[:case.M, :case.n_out])
            torch.cuda.synchronize()
            assert torch.equal(_bits(plain), _bits(buf)), f"{case.name}: fo1_gemm_bf16_wtiled differs from fo1_gemm_bf16 on the same tile"
    finally:
        _restore(lib)


def test_zz_route_summary():
    print()
    for claim in sorted(WORST):
        w, rows = WORST[claim]
        print(f"SUMMARY {claim}: {rows} worst {w:.3f} of the bound")
    if WORST:      # (run alone, there is nothing to summarise)
        assert max(w for w, _ in WORST.values()) <= 1.0
