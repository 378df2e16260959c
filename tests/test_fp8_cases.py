"""The fp8 sweep's cases, bounds, emulation and faults on the CPU (no GPU; tests/fp8_cases.py):
  * GEMM_CASES reach every label of REQUIRED_LABELS (coalesced and fragment epilogue, the latter by each of its four conditions alone, every
    activation with and without bias, the residual, every K-loop shape, one tile and many), the restated tile order is a bijection, the restated
    constants are the source's;
  * families `exact` and `xepi` are exactly representable (sum |products| 2^8 < 2^24, power-of-two scales; no product truncated, no sum rounded in
    either emulation) and `exact`'s emulation equals bf16(float64) bit for bit; `xepi` and `quant`: the fp32 emulation stays within the sharp bound
    (ACC8 / 4, the half ulp of each value's own binade) and its accumulation error within ACC8 / 4; the instruction's model stays within ACC8 / 4 x
    2^-24 S + the truncation term of float64 and its output within the bound; every applicable fault changes bits of `exact` or breaks the bound by 2 x;
  * the probe cases: the model gives the known answers, the plain fp32 product does not;
  * the quantiser's emulation equals the oracle on every case, the built rows hold what the issue lists, every quantiser fault changes bytes or scales;
  * the RMSNorm quantiser's emulation meets both assertions, every fault breaks one.
The figures come from cached functions, so every test, the summaries included, runs alone as well.  test_zz_summary prints them (RESULTS_CPU) and holds
ACC8 to the power of two next above 4 x the measured accumulation error."""
import pytest
import torch

import fp8_cases as C
from oracle import fp8_oracle as F

import functools


def test_constants_are_the_sources():
    k = C.source_constants()
    assert (k["kMaxChunksPerLane"], k["RC"], k["gm"]) == (C.K_MAX_CHUNKS_PER_LANE, C.QUANT_REG_CHUNKS, C.GROUP_M)
    assert C.RMSQ_D[-1] == 4096 and C.QUANT_REG_CHUNKS * 256 * 8 == 12288


def test_gemm_cases_cover_every_route_label():
    assert len({c.name for c in C.GEMM_CASES}) == len(C.GEMM_CASES)
    have = set()
    for c in C.GEMM_CASES:
        r = C.route(c)
        have |= r.labels(c)
        assert c.K % 128 == 0 and c.K <= 896 and c.M <= 520 and c.N <= 1028 and c.lda > c.K and c.ldw > c.K and c.lda % 16 == 0 and c.ldw % 16 == 0
        assert c.ldc > c.n_out and c.ldc % 4 == 0 and c.N % 4 == 0 and (not c.res or (c.ldr % 4 == 0 and c.ldr != c.ldc)) and c.c_off in (0, 4)
        assert c.act != 3 or (c.N % 32 == 0 and not c.res)
        assert c.family in ("quant", "xepi") or (c.act == 0 and not c.bias and not c.res)
    assert not C.REQUIRED_LABELS - have, f"labels no case reaches: {sorted(C.REQUIRED_LABELS - have)}"
    exact = [c for c in C.GEMM_CASES if c.family == "exact"]
    assert {c.K // 128 for c in exact} >= set(range(1, 8)) and {c.M for c in exact} >= {1, 255, 256, 257, 513} and {c.N for c in exact} >= {4, 12, 252, 256, 260, 516}
    alone = {C.route(c).why_fragment for c in C.GEMM_CASES if len(C.route(c).why_fragment) == 1}
    assert alone == {("n_out",), ("ldc",), ("C alignment",), ("ldr",)}, alone
    assert any(C.route(c).tiles_m == 3 and C.route(c).tiles_n == 3 for c in exact)


def test_tile_order_is_a_bijection():
    shapes = {(C.route(c).tiles_m, C.route(c).tiles_n) for c in C.GEMM_CASES} | {(tm, tn) for tm in range(1, 6) for tn in range(1, 12)}
    assert (3, 3) in shapes
    for tm, tn in shapes:
        order = C.tile_order(tm, tn)
        assert sorted(order) == [(i, j) for i in range(tm) for j in range(tn)], (tm, tn)
    order = C.tile_order(3, 3)           # nine workgroups: a ragged XCD split (XCD 0 runs two tiles), the last group one tile row short
    assert order == [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 0), (2, 1), (2, 2), (1, 0)]     # (by hand from tile_coords_grouped_id)


@functools.lru_cache(maxsize=None)
def gemm_figures(name):
    """What one GEMM case measures (computed once, whichever test asks first): the fp32 emulation's accumulation error and fraction of the bound and of
    the sharp bound, the model's worst error in units of its own allowance, every applicable fault's factor (None: family `exact`, bits)."""
    case = next(c for c in C.GEMM_CASES if c.name == name)
    d = C.build(case)
    ref, bound = C.reference_and_bound(d)
    assert torch.isfinite(ref).all() and (bound >= 0).all()
    emu = C.emulate(d)
    fig = dict(acc=C.acc_error(d), faults={}, emu=emu, ref=ref, bound=bound)
    ds = C.sub(d, C.sample_rows(case))               # the instruction's model: on a sample of the rows
    Z0, S0 = C.accumulators(ds)
    allow = C.ACC8 / 4 * C.F32_EPS * S0 + C.truncation_term(ds)
    err = (C.emulate_acc(ds, mfma=True).double() - Z0).abs()
    fig["model"] = torch.where(err == 0, torch.zeros_like(err), err / allow.clamp_min(1e-300)).max().item()
    fig["model_exact"] = bool((err == 0).all())
    if case.family != "exact":
        fig["emulate"] = C.worst_ratio(emu, ref, bound)
        fig["sharp"] = C.worst_ratio(emu, ref, C.reference_and_bound(d, acc=C.ACC8 / 4, exact_ulp=True)[1])
        refs, bounds = C.reference_and_bound(ds)
        fig["model_out"] = C.worst_ratio(C.emulate(ds, mfma=True), refs, bounds)
        refm, boundm = C.reference_and_bound(ds, model=True)
        fig["plain_vs_model"] = C.worst_ratio(C.emulate(ds), refm, boundm)
    for f in C.applicable_faults(d):
        mut = C.emulate(d, f)
        fig["faults"][f] = (not torch.equal(torch.nan_to_num(mut, nan=-1e30), emu)) if case.family == "exact" else C.worst_ratio(mut, ref, bound)
    return fig


@pytest.mark.parametrize("case", C.GEMM_CASES, ids=lambda c: c.name)
def test_gemm_bound_passes_the_emulation_and_fails_every_fault(case):
    d = C.build(case)
    fig = gemm_figures(case.name)
    faults = fig["faults"]
    assert len(faults) >= (6 if case.M > 1 and case.N >= 8 else 4), (case.name, list(faults))
    assert fig["acc"] <= C.ACC8 / 4, f"{case.name}: fp32 accumulation error {fig['acc']:.3f} x 2^-24 S: ACC8 = {C.ACC8} is not 4 x that"
    assert fig["model"] <= 1.0, f"{case.name}: the instruction's model is {fig['model']:.3f} of ACC8 / 4 x 2^-24 S + the truncation term off float64"
    if case.family != "quant":
        load = C.exactly_representable(d)
        assert load < 2.0 ** 24, f"{case.name}: sum |products| 2^8 = {load:.4g}"
        assert fig["acc"] == 0.0 and fig["model_exact"] and not C.truncation_term(d).any(), f"{case.name}: a product is truncated or a sum rounds"
    if case.family == "exact":
        want = C.exact_expected(d)
        assert torch.equal(C.bits16(fig["emu"].float().bfloat16()), C.bits16(want)), f"{case.name}: the emulation is not bf16(float64)"
        buf = C.host_buffers(d)["out"]
        with pytest.raises(AssertionError, match="never written"):
            C.check_canary(buf, d, case.name)
        C.out_view(buf, case)[:case.M, :case.n_out] = want
        C.check_canary(buf, d, case.name)
        buf[case.c_off + case.M * case.ldc] = 0
        with pytest.raises(AssertionError, match="written"):
            C.check_canary(buf, d, case.name)
        for f, changed in faults.items():
            assert changed, f"{case.name}: '{f}' changes no bit"
        return
    print(f"\n{case.name}: fp32 emulation {fig['emulate']:.3f} of the bound, {fig['sharp']:.3f} of the sharp bound, accumulation {fig['acc']:.3f} x 2^-24 S; the "
          f"model {fig['model']:.3f} of its allowance, its output {fig['model_out']:.3f} of the bound; fp32 emulation against the model {fig['plain_vs_model']:.3f}")
    assert fig["sharp"] <= 1.0, f"{case.name}: the emulation is {fig['sharp']:.3f} of the sharp bound off the float64 reference"
    assert fig["model_out"] <= 1.0, f"{case.name}: the model's output is {fig['model_out']:.3f} of the bound off the float64 reference"
    for f, fw in faults.items():
        assert fw >= 2.0, f"{case.name}: '{f}' moves no element by more than {fw:.3g} x the bound"


def test_zy_every_gemm_fault_runs_on_the_families_it_applies_to():
    seen = {}
    for c in C.GEMM_CASES:
        for f in C.applicable_faults(C.build(c)):
            seen.setdefault(f, set()).add("quant" if c.family == "xepi" else c.family)
    for f in C.GEMM_FAULTS:
        want = {"quant"} if f in ("bias_next_fragment", "res_ldc", "swiglu_swap") else {"exact", "quant"}
        assert seen.get(f) == want, (f, seen.get(f))


@pytest.mark.parametrize("d", C.probe_cases(), ids=lambda d: d["case"].name)
def test_probe_cases_known_answers(d):
    """The model gives the values that follow from the adders' widths alone, all of them bf16; the plain fp32 product does not."""
    assert torch.equal(C.DECODE[d["Aq"].long()].float(), d["A"]) and torch.equal(C.DECODE[d["Wq"].long()].float(), d["W"])
    acc = C.emulate_acc(d, mfma=True)
    assert torch.equal(acc.bfloat16().float(), acc)
    bad = [(m, n, v, acc[m, n].item()) for m, n, v in d["known"] if acc[m, n].item() != v]
    assert not bad, bad[:5]
    plain = C.emulate_acc(d)
    differ = sum(plain[m, n].item() != v for m, n, v in d["known"])
    assert differ > len(d["known"]) // 10 if d["case"].name == "probe-groups" else differ == 0      # (probe-accumulate: fp32 round-to-nearest in both)


# ---------------------------------------------------------------------------------------------------------------------------------------
def test_built_rows_hold_what_they_are_for():
    x = C.quant_built_rows(1024).float()
    q, s = F.quantize_rows_e4m3(x)
    row = dict(zip(C.BUILT_ROWS, range(len(C.BUILT_ROWS))))
    assert s[row["ties"]] == 1.0 and s[row["ties negated"]] == 1.0 and s[row["minus zero"]] == 1.0 and s[row["zero"]] == 1.0
    v = C.tie_values()
    grid, mid = C.E4M3_GRID.float(), C.E4M3_MID.float()
    qt = q[row["ties"], :v.numel()]
    assert torch.equal(qt[:127], torch.arange(127, dtype=torch.uint8)), "every non-negative e4m3 value maps to its own byte"
    ties = qt[127:127 + 126]
    assert torch.equal(ties, ((torch.arange(126) + 1) // 2 * 2).to(torch.uint8)), "every midpoint ties to the even byte"
    assert mid[0] == 2.0 ** -10 and ties[0] == 0
    assert torch.equal(qt[253:253 + 126], torch.arange(1, 127, dtype=torch.uint8)) and torch.equal(qt[379:379 + 126], torch.arange(126, dtype=torch.uint8))
    assert (qt[505:508] == 0).all() and qt[508] == 1                         # below 2^-10 -> 0; 1.5 x 2^-10 -> 2^-9
    assert torch.equal(q[row["ties negated"], :v.numel()], qt | 0x80)
    assert (q[row["minus zero"]] == 0x80).all() and (q[row["zero"]] == 0).all()
    neg = x[row["negative absmax"]]
    assert neg.abs().max() == 37.5 and neg.max() < 37.5 and (q[row["negative absmax"], ::5] == 0x80).all() and (q[row["negative absmax"]] == 0xFE).sum() == 1
    a = C.clamp_row_absmax()
    pre = x[row["clamp"]] / s[row["clamp"]]
    assert pre.max() > 448.0 and pre.min() < -448.0 and q[row["clamp"], 3] == 0x7E and q[row["clamp"], 1022] == 0xFE and a == x[row["clamp"]].max()
    sub = x[row["bf16 subnormals"]]
    assert 0 < sub.abs().max() < 2.0 ** -126 and 0 < s[row["bf16 subnormals"]] < 2.0 ** -126 and (q[row["bf16 subnormals"]] == 0x7E).sum() == 1
    assert len(set(q[row["bf16 subnormals"]].tolist())) > 40


@functools.lru_cache(maxsize=None)
def quant_fault_hits(name):
    case = next(c for c in C.QUANT_CASES if c.name == name)
    x = C.quant_input(case)
    q, s = F.quantize_rows_e4m3(x.float())
    return {f for f in C.QUANT_FAULTS if not all(torch.equal(a, b) for a, b in zip(C.quant_emulate(x, f), (q, s)))}


@pytest.mark.parametrize("case", C.QUANT_CASES, ids=lambda c: c.name)
def test_quantiser_emulation_is_the_oracle(case):
    x = C.quant_input(case)
    assert x.shape == ((len(C.BUILT_ROWS) if case.built else case.M), case.K) and case.ldx > case.K and case.ldq > case.K
    q, s = F.quantize_rows_e4m3(x.float())
    eq, es = C.quant_emulate(x)
    assert torch.equal(eq, q) and torch.equal(es, s)
    b = C.quant_host_buffers(x, case.ldx, case.ldq)
    C.check_quant_frames(b["q"], b["scales"], x.shape[0], case.K, case.name)
    b["q"][x.shape[0], 0] = 0
    with pytest.raises(AssertionError):
        C.check_quant_frames(b["q"], b["scales"], x.shape[0], case.K, case.name)


def test_every_quantiser_fault_shows_where_it_must():
    seen = {f: {c.name for c in C.QUANT_CASES if f in quant_fault_hits(c.name)} for f in C.QUANT_FAULTS}
    built = {"quant-built-k1024", "quant-built-k12296"}
    for f in C.QUANT_FAULTS:
        assert seen[f], f"'{f}' changes nothing on any case"
    for f in ("signed_max", "round_half_away", "flush_subnormals", "positive_zero"):
        assert built <= seen[f], (f, seen[f])
    assert {"quant-k2040-m1", "quant-k2048-m1", "quant-k2056-m1", "quant-k12288-m1", "quant-k12296-m1"} <= seen["absmax_skips_last_chunk"]
    assert {"quant-k12296-m1", "quant-k13312-m1"} <= seen["absmax_register_chunks_only"]
    assert "quant-k12288-m1" not in seen["absmax_register_chunks_only"]


# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rmsq_figures(name):
    """-> (scale fraction, byte fraction of the float64 bound, {fault: (breaks bit identity, breaks the float64 bound, must break one, must break the second)})"""
    case = next(c for c in C.RMSQ_CASES if c.name == name)
    d = C.rmsq_inputs(case)
    q0, s0 = C.rmsq_composition(case)
    q, s = C.rmsq_emulate(case)
    assert torch.equal(q, q0) and torch.equal(s[:case.M], s0), f"{case.name}: the emulation differs from rmsnorm emulation + oracle quantiser"
    fs, fq = C.rmsq_check(case, q, s)
    x = d["x"].float()
    live = bool((x.abs().amax(dim=1) > 0).any())
    zero_row = bool((x.abs().amax(dim=1) == 0).any())
    tail_only = bool(((x[:, :-8].abs().amax(dim=1) == 0) & (x.abs().amax(dim=1) > 0)).any()) if case.D > 8 else live
    out = {}
    for f in C.RMSQ_FAULTS:
        mq, ms = C.rmsq_emulate(case, f)
        one = not (torch.equal(mq, q0) and torch.equal(ms[:case.M], s0) and ms[case.M].view(torch.int32) == C.CANARY32)
        a, b = C.rmsq_check(case, mq, ms)
        must = (f == "scale_next_row" or (f == "no_eps" and zero_row) or (f == "absmax_skips_last_chunk" and tail_only)
                or (f == "absmax_unweighted" and live and case.D >= 504))
        out[f] = (one, not (a <= 1.0 and b <= 1.0), must, must and f in ("absmax_unweighted", "absmax_skips_last_chunk", "scale_next_row"))
    return fs, fq, out


@pytest.mark.parametrize("case", C.RMSQ_CASES, ids=lambda c: c.name)
def test_rmsnorm_quantiser_emulation_meets_both_assertions_and_faults_break_one(case):
    fs, fq, faults = rmsq_figures(case.name)
    assert fs <= 1.0 and fq <= 1.0, f"{case.name}: scale at {fs:.3f}, bytes at {fq:.3f} of the float64 bound"
    for f, (one, two, must, must_two) in faults.items():
        assert not must or one or two, f"{case.name}: '{f}' breaks neither assertion"
        assert not must_two or two, f"{case.name}: '{f}' passes the float64 assertion"


def test_zz_summary():
    for f in C.RMSQ_FAULTS:
        hits = [rmsq_figures(c.name)[2][f] for c in C.RMSQ_CASES]
        hits = [h for h in hits if h[0] or h[1]]
        assert hits, f"'{f}' breaks no assertion on any case"
        print(f"\nSUMMARY rmsnorm_quant fault {f}: {len(hits)} of {len(C.RMSQ_CASES)} cases, {sum(h[0] for h in hits)} by bit identity, {sum(h[1] for h in hits)} by the float64 bound", end="")
    figs = {c.name: gemm_figures(c.name) for c in C.GEMM_CASES}
    bounded = [c.name for c in C.GEMM_CASES if c.family != "exact"]
    load = max(C.exactly_representable(C.build(c)) for c in C.GEMM_CASES if c.family != "quant")
    acc = max(f["acc"] for f in figs.values())
    weakest = min((fw, f"{f} on {n}") for n in bounded for f, fw in figs[n]["faults"].items())
    print(f"\nSUMMARY gemm_fp8 exact, xepi: sum |products| 2^8 at most {load:.4g} = 2^{torch.log2(torch.tensor(load)).item():.2f} (< 2^24)")
    print(f"SUMMARY gemm_fp8 quant, xepi: fp32 emulation at most {max(figs[n]['emulate'] for n in bounded):.3f} of the bound, {max(figs[n]['sharp'] for n in bounded):.3f} of the "
          f"sharp bound; accumulation error at most {acc:.3f} x 2^-24 S, ACC8 = {C.ACC8:.0f}; the instruction's model at most {max(f['model'] for f in figs.values()):.3f} of "
          f"ACC8 / 4 x 2^-24 S + the truncation term, its output {max(figs[n]['model_out'] for n in bounded):.3f} of the bound; the fp32 emulation against the model "
          f"{max(figs[n]['plain_vs_model'] for n in bounded):.3f}; weakest fault {weakest[0]:.3g} x the bound ({weakest[1]})")
    print(f"SUMMARY rmsnorm_quant: emulation's scale at most {max(rmsq_figures(c.name)[0] for c in C.RMSQ_CASES):.3f}, bytes at most "
          f"{max(rmsq_figures(c.name)[1] for c in C.RMSQ_CASES):.3f} of the float64 bound")
    assert 4 * acc <= C.ACC8 < 8 * acc, f"ACC8 = {C.ACC8} is not the power of two next above 4 x {acc:.3f}"
