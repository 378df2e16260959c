"""The fp8 GEMM and its two quantisers on the MI355X, case by case against the float64 references of tests/fp8_cases.py.

fo1_gemm_fp8, fo1_quantize_rows_e4m3 and fo1_rmsnorm_quant_e4m3 are called through the loaded library, so that the test owns every buffer: e4m3 NaN
bytes around the operands, NaN after the scales and the bias, the residual in a NaN frame with its own stride, canaries around every output.
  * GEMM, family `exact`: bf16(float64) bit for bit.  Families `xepi` and `quant`: |got - ref| <= bound per element (fp8_cases.reference_and_bound: the
    issue's terms plus, on `quant`, what the instruction's adders can drop from that element), and on a sample of rows the same bound without that term
    around the instruction's model.  The probes: the model's accumulator and the known answers, bit for bit.  Every case:
    the profile row of the product library, the shape-carrying row of the A/B library (whose output must be the same bits), canaries intact and no
    output element left unwritten, inputs unchanged, a second launch bit-identical.
  * fo1_quantize_rows_e4m3: bytes and scales equal to oracle.fp8_oracle.quantize_rows_e4m3.
  * fo1_rmsnorm_quant_e4m3: equal to the oracle quantiser on what fo1_rmsnorm_bf16 returned for the same rows, and within the float64 bounds of
    fp8_cases.rmsq_check.
  * ops.gemm / ops.norm_linear with a registered weight on either side of FP8_MIN_ROWS.
test_zz_summary prints one SUMMARY line per op and route with the worst fraction of the bound."""
import time

import pytest
import torch

import fp8_cases as C
import small_op_cases as S
from oracle import fp8_oracle as F

pytestmark = pytest.mark.gpu

WORST = {}
T0 = time.time()


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), v)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------------------------
# fo1_gemm_fp8
# ---------------------------------------------------------------------------------------------------------------------------------------
def _gemm_launch(lib, c, dev, out):
    from vlm_fo1_amd import lib as L
    rc = lib.fo1_gemm_fp8(dev["Aq"].data_ptr(), c.lda, dev["sa"].data_ptr(), dev["Wq"].data_ptr(), c.ldw, dev["sw"].data_ptr(), _ptr(dev.get("bias")),
                          _ptr(dev.get("res")), c.ldr if c.res else 0, out.data_ptr() + 2 * c.c_off, c.ldc, c.M, c.N, c.K, c.act, L.current_stream_ptr())
    assert rc == 0, f"{c.name}: rc {rc}: {lib.fo1_last_error().decode()}"
    torch.cuda.synchronize()


def _gemm_profiled(lib, c, dev, host):
    """One launch into a fresh canary buffer -> (the buffer on the CPU, the profile row names)."""
    from vlm_fo1_amd import lib as L
    assert L.load() is lib
    out = host["out"].cuda()
    L.profile_rows()
    L.profile(True)
    try:
        _gemm_launch(lib, c, dev, out)
        rows = L.profile_rows()
    finally:
        L.profile(False)
    assert all(r["calls"] == 1 for r in rows), rows
    return out.cpu(), [r["name"] for r in rows]


def _against_bound(d, got, model=False):
    """-> (worst |got - ref| / bound, a message naming the worst element).  model: fp8_cases.reference_and_bound(model = True)."""
    c = d["case"]
    ref, bound = C.reference_and_bound(d, model=model)
    ratio = torch.nan_to_num(torch.where(got.double() == ref, torch.zeros_like(ref), (got.double() - ref).abs() / bound.clamp_min(1e-300)), nan=float("inf"))
    worst = ratio.max().item()
    at = tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])
    return worst, (f"{c.name}: {int((ratio > 1).sum())} of {ratio.numel()} elements beyond the bound, worst {worst:.3g} x at {at}: got {got[at].item():.6g}, "
                   f"ref {ref[at].item():.6g}, bound {bound[at].item():.3g}")


@pytest.mark.parametrize("case", C.GEMM_CASES, ids=lambda c: c.name)
def test_gemm_fp8(case, product_library):
    from vlm_fo1_amd import lib as L
    d = C.build(case)
    r = d["route"]
    host = C.host_buffers(d)
    dev = {k: v.cuda() for k, v in host.items() if k != "out"}
    out, rows = _gemm_profiled(product_library, case, dev, host)
    assert rows == [C.PRODUCT_ROW], f"{case.name}: launched {rows}"
    C.check_canary(out, d, case.name)
    for k, v in dev.items():
        assert _same_bits(v.cpu(), host[k]), f"{case.name}: the input {k} changed"
    got = C.out_view(out, case)[:case.M, :case.n_out]
    key = f"gemm_fp8 {case.family} {r.epilogue()} act{case.act}"
    if case.family == "exact":
        want = C.exact_expected(d)
        diff = C.bits16(got.contiguous()) != C.bits16(want)
        print(f"\nCASE {case.name} {r.epilogue()} {C.loop_class(r.nk)} {r.tiles_m}x{r.tiles_n} tiles: {int(diff.sum())} of {diff.numel()} elements differ from bf16(float64)")
        assert not diff.any(), (f"{case.name}: {int(diff.sum())} elements are not bf16(float64), first at {diff.nonzero()[0].tolist()}: got "
                                f"{got[tuple(diff.nonzero()[0])].item()}, want {want[tuple(diff.nonzero()[0])].item()}")
        _note(key, 0.0)
    else:
        worst, msg = _against_bound(d, got)
        rows = C.sample_rows(case)
        near, msg_model = _against_bound(C.sub(d, rows), got[rows], model=True)
        print(f"\nCASE {case.name} {r.epilogue()} {C.loop_class(r.nk)} {r.tiles_m}x{r.tiles_n} tiles: worst {worst:.3f} of the bound, {near:.3f} of the bound around the "
              f"instruction's model ({rows.numel()} rows)")
        _note(key, worst)
        _note(key + " around the model", near)
        assert worst <= 1.0, msg
        assert near <= 1.0, "around the instruction's model, " + msg_model
    out2 = host["out"].cuda()
    _gemm_launch(product_library, case, dev, out2)
    assert _same_bits(out2.cpu(), out), f"{case.name}: a second launch gives other bits"
    with L.use_ab() as ab:
        try:
            L.check(ab.fo1_gemm_profile_shapes(1), "profile_shapes")
            aout, arows = _gemm_profiled(ab, case, dev, host)
        finally:
            ab.fo1_gemm_profile_shapes(0)
    assert arows == [r.shape_row(case)], f"{case.name}: the A/B library launched {arows}, expected {[r.shape_row(case)]}"
    assert _same_bits(aout, out), f"{case.name}: the A/B library gives other bits"


@pytest.mark.parametrize("d", C.probe_cases(), ids=lambda d: d["case"].name)
def test_gemm_fp8_probes(d, product_library):
    """Known answers of the instruction's adders (fp8_cases.probe_cases): the kernel returns the model's accumulator, bit for bit."""
    case = d["case"]
    host = C.host_buffers(d)
    dev = {k: v.cuda() for k, v in host.items() if k != "out"}
    out = host["out"].cuda()
    _gemm_launch(product_library, case, dev, out)
    out = out.cpu()
    C.check_canary(out, d, case.name)
    got = C.out_view(out, case)[:case.M, :case.n_out].float()
    bad = [(m, n, v, got[m, n].item()) for m, n, v in d["known"] if got[m, n].item() != v]
    print(f"\nCASE {case.name}: {len(bad)} of {len(d['known'])} known answers missed" + "".join(f"\n  row {m} column {n}: expected {v!r}, got {g!r}" for m, n, v, g in bad[:40]))
    want = C.emulate_acc(d, mfma=True)
    diff = got != want
    print(f"CASE {case.name}: {int(diff.sum())} of {diff.numel()} elements differ from the model" + "".join(
        f"\n  row {m} column {n}: model {want[m, n].item()!r}, got {got[m, n].item()!r}" for m, n in diff.nonzero()[:40].tolist()))
    assert not bad, f"{case.name}: {len(bad)} of {len(d['known'])} known answers missed, first (row, column, expected, got) {bad[0]}"
    assert not diff.any(), f"{case.name}: {int(diff.sum())} elements differ from the model, first at {diff.nonzero()[0].tolist()}"
    _note(f"gemm_fp8 {case.name}", 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# fo1_quantize_rows_e4m3
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.QUANT_CASES, ids=lambda c: c.name)
def test_quantize_rows(case, product_library):
    from vlm_fo1_amd import lib as L
    lib = product_library
    x = C.quant_input(case)
    M, K = x.shape
    host = C.quant_host_buffers(x, case.ldx, case.ldq)

    def launch():
        dev = {k: v.cuda() for k, v in host.items()}
        rc = lib.fo1_quantize_rows_e4m3(dev["x"].data_ptr(), case.ldx, M, K, dev["q"].data_ptr(), case.ldq, dev["scales"].data_ptr(), L.current_stream_ptr())
        assert rc == 0, f"{case.name}: rc {rc}: {lib.fo1_last_error().decode()}"
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in dev.items()}

    got = launch()
    assert _same_bits(got["x"], host["x"]), f"{case.name}: the input changed"
    C.check_quant_frames(got["q"], got["scales"], M, K, case.name)
    q_ref, s_ref = F.quantize_rows_e4m3(x.float())
    bad_s = got["scales"][:M].view(torch.int32) != s_ref.view(torch.int32)
    assert not bad_s.any(), f"{case.name}: scales of rows {bad_s.nonzero()[:, 0].tolist()} differ: {got['scales'][:M][bad_s].tolist()} for {s_ref[bad_s].tolist()}"
    bad = got["q"][:M, :K] != q_ref
    names = C.BUILT_ROWS if case.built else [str(i) for i in range(M)]
    assert not bad.any(), (f"{case.name}: {int(bad.sum())} bytes differ from the oracle, rows {[names[i] for i in bad.any(dim=1).nonzero()[:, 0].tolist()]}, first at "
                           f"{bad.nonzero()[0].tolist()}: x {x[tuple(bad.nonzero()[0])].item():.8g}, got {int(got['q'][tuple(bad.nonzero()[0])])}, want {int(q_ref[tuple(bad.nonzero()[0])])}")
    again = launch()
    assert _same_bits(again["q"], got["q"]) and _same_bits(again["scales"], got["scales"]), f"{case.name}: a second launch gives other bits"
    _note(f"quantize_rows {'built rows' if case.built else 'gaussian'} " + ("registers" if K <= C.QUANT_REG_CHUNKS * 2048 else "registers + re-read"), 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# fo1_rmsnorm_quant_e4m3
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.RMSQ_CASES, ids=lambda c: c.name)
def test_rmsnorm_quant(case, product_library):
    from vlm_fo1_amd import lib as L
    lib = product_library
    d = C.rmsq_inputs(case)
    M, D = case.M, case.D
    host = C.quant_host_buffers(d["x"], case.ldx, case.ldq)
    host["w"] = torch.cat([d["w"], torch.full((8,), float("nan"), dtype=torch.bfloat16)])
    host["y"] = torch.full((M + 1, D + 8), C.CANARY_BF, dtype=torch.bfloat16)

    def launch():
        dev = {k: v.cuda() for k, v in host.items()}
        st = L.current_stream_ptr()
        rc = lib.fo1_rmsnorm_quant_e4m3(dev["x"].data_ptr(), case.ldx, dev["w"].data_ptr(), M, D, S.RMS_EPS, dev["q"].data_ptr(), case.ldq, dev["scales"].data_ptr(), st)
        assert rc == 0, f"{case.name}: rc {rc}: {lib.fo1_last_error().decode()}"
        rc = lib.fo1_rmsnorm_bf16(dev["x"].data_ptr(), case.ldx, dev["w"].data_ptr(), dev["y"].data_ptr(), D + 8, M, D, S.RMS_EPS, st)
        assert rc == 0, f"{case.name}: rc {rc}: {lib.fo1_last_error().decode()}"
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in dev.items()}

    got = launch()
    assert _same_bits(got["x"], host["x"]) and _same_bits(got["w"], host["w"]), f"{case.name}: an input changed"
    C.check_quant_frames(got["q"], got["scales"], M, D, case.name)
    assert S.canary_intact(got["y"], M, D)
    q, s = got["q"][:M, :D], got["scales"][:M]
    q_two, s_two = F.quantize_rows_e4m3(got["y"][:M, :D].float())
    assert torch.equal(s.view(torch.int32), s_two.view(torch.int32)), f"{case.name}: scales {s.tolist()}, fo1_rmsnorm_bf16 + oracle quantiser {s_two.tolist()}"
    assert torch.equal(q, q_two), f"{case.name}: {int((q != q_two).sum())} bytes differ from fo1_rmsnorm_bf16 + oracle quantiser, first at {(q != q_two).nonzero()[0].tolist()}"
    fs, fq = C.rmsq_check(case, q, got["scales"])
    print(f"\nCASE {case.name}: scale {fs:.3f}, bytes {fq:.3f} of the float64 bound")
    assert fs <= 1.0, f"{case.name}: a row's scale at {fs:.3g} x its float64 bound"
    assert fq <= 1.0, f"{case.name}: a dequantised element at {fq:.3g} x its float64 bound"
    again = launch()
    assert _same_bits(again["q"], got["q"]) and _same_bits(again["scales"], got["scales"]), f"{case.name}: a second launch gives other bits"
    per = C.cdiv(D // 8, 64)
    _note(f"rmsnorm_quant {per} chunk{'s' if per > 1 else ''} per lane scale", fs)
    _note(f"rmsnorm_quant {per} chunk{'s' if per > 1 else ''} per lane bytes", fq)


# ---------------------------------------------------------------------------------------------------------------------------------------
# ops.gemm / ops.norm_linear on either side of FP8_MIN_ROWS
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_registered_weight_routes_at_fp8_min_rows(product_library):
    from vlm_fo1_amd import ops
    N, K, R = 72, 256, ops.FP8_MIN_ROWS
    g = torch.Generator().manual_seed(5)
    a = torch.randn(R, K, generator=g).bfloat16().cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16().cuda()
    nw = (1 + 0.1 * torch.randn(K, generator=g)).bfloat16().cuda()
    bias = C.bias_pattern(N).cuda()
    below, at = a[:R - 1], a
    assert not ops.fp8_routed(w, R)
    bf_gemm, bf_nl = ops.gemm(below, w, bias), ops.norm_linear(below, nw, 1e-6, w, bias)
    try:
        assert ops.register_fp8_weight(w)
        assert not ops.fp8_routed(w, R - 1) and ops.fp8_routed(w, R)
        fw = ops._fp8_weights[(w.data_ptr(), N, K)]
        assert _same_bits(ops.gemm(below, w, bias), bf_gemm), "M = FP8_MIN_ROWS - 1 with a registered weight: not the bf16 call"
        assert _same_bits(ops.norm_linear(below, nw, 1e-6, w, bias), bf_nl), "norm_linear at M = FP8_MIN_ROWS - 1: not the bf16 calls"
        aq, sa = ops.quantize_rows_fp8(at)
        assert _same_bits(ops.gemm(at, w, bias), ops.gemm_fp8(aq, sa, fw, bias)), "M = FP8_MIN_ROWS: not quantize_rows_fp8 + gemm_fp8"
        q, s = ops.rmsnorm_quant_fp8(at, nw, 1e-6)
        assert _same_bits(ops.norm_linear(at, nw, 1e-6, w, bias), ops.gemm_fp8(q, s, fw, bias)), "norm_linear at M = FP8_MIN_ROWS: not rmsnorm_quant_fp8 + gemm_fp8"
        assert not _same_bits(ops.gemm(at, w, bias)[:R - 1], bf_gemm), "the fp8 product equals the bf16 one: the route is not observable"
    finally:
        ops.clear_fp8_weights()
    assert not ops.fp8_routed(w, R)


def test_zz_summary():
    assert WORST, "run the whole file: the summary reports what the sweep measured"
    for key in sorted(WORST):
        exact = key.startswith("quantize_rows") or " exact " in key or " probe-" in key
        print(f"\nSUMMARY {key}: " + ("exact" if exact and WORST[key] == 0.0 else f"worst {WORST[key]:.3f} of the bound"), end="")
    print(f"\nSUMMARY wall time {time.time() - T0:.1f} s for {len(C.GEMM_CASES)} + {len(C.QUANT_CASES)} + {len(C.RMSQ_CASES)} cases")
    assert max(WORST.values()) <= 1.0
