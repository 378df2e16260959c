"""The decode-linear sweep's routing model, bound, emulation and faults on the CPU (no GPU; tests/decode_linear_cases.py):
  * every label the two dispatches reach with the product defaults (refusals included) has a case, every case's claimed label is what the
    model computes, and the cases cover the edges the sweep is about;
  * on every case the emulated kernel arithmetic stays within the SHARP form of the per-element bound (every rounding point at the half ulp
    of the value's own binade, the accumulation term at ACC / 4, the rstd term at RSTD_REL / 4), its fp32 accumulation error within ACC / 4
    of 2^-24 (|x| |W|^T + |bias|) and its rstd within RSTD_REL / 4;
  * every applicable fault moves some element of every region it touches by at least twice the bound, no route is left without one, and the
    share of (case, fault) pairs that do not apply is printed;
  * the dropped k-step's multiple of the bound with and without the planted columns is printed; the canary checks pass a clean buffer and fail a dirtied one.
The summary test prints the figures ACC and RSTD_REL were set from."""
import pytest
import torch

import decode_linear_cases as C

RUN = [c for c in C.SWEEP if not c.refused]
WORST = {"emulate": 0.0, "acc": 0.0, "rstd": 0.0, "fault": float("inf"), "fault_at": "", "pairs": 0, "na": 0}
ROUTE_FAULTS = {}


def test_sweep_names_are_unique_and_every_claim_is_the_models_route():
    assert len({c.name for c in C.SWEEP}) == len(C.SWEEP)
    for c in C.SWEEP:
        assert C.case_route(c).label() == c.claim, f"{c.name}: the model routes it to {C.case_route(c).label()!r}, the table claims {c.claim!r}"
        assert c.ldc_pad > 0 and c.ldx_pad % 8 == 0 and c.ldw_pad % 8 == 0
        assert c.N * c.K * 2 <= 40 * 2 ** 20, f"{c.name}: weight matrix above 40 MB"
        if c.entry in ("batch", "combine"):
            assert c.ldr % 4 == 0 and c.N % 4 == 0          # (otherwise the entry leaves the MFMA kernel)


def test_cases_cover_every_label_the_dispatch_reaches():
    reachable = C.reachable_labels()
    covered = {c.claim for c in C.SWEEP}
    missing = {k: v for k, v in reachable.items() if k not in covered}
    assert not missing, f"labels reached by the dispatch with no case in SWEEP: {missing}"
    mfma = [k for k in reachable if k.split()[0] in ("plain", "swiglu", "qkv")]
    assert len(mfma) == 27, sorted(mfma)       # plain 6 + 6 + 5, SwiGLU 2 + 2 + 1, QKV 2 + 2 + 1
    assert len([k for k in reachable if k.startswith("gemv")]) == 12
    assert len([k for k in reachable if k.startswith("refused")]) == 4
    assert covered <= set(reachable), covered - set(reachable)


def test_refusals_are_predicted():
    ref = {c.name: C.case_route(c) for c in C.SWEEP if c.refused}
    assert len(ref) == 4 and all(r.kind == "refused" for r in ref.values())
    # one step inside every limit the dispatch does launch
    assert C.route_batch(16, 32, 2112, C.SWIGLU).kind == "mfma" and C.route_batch(17, 32, 2048, C.SWIGLU).kind == "mfma"
    assert C.route_batch(17, 8188, 2112).kind == "mfma" and C.route_batch(16, 8192, 2112).kind == "mfma"
    assert C.route_batch(5, 20, 2048, norm=True).kind == "mfma"
    assert C.route_batch(26, 4096, 2112).xr32 and not C.route_batch(27, 4096, 2112).xr32 and not C.route_batch(26, 4100, 2112).xr32


def test_sweep_covers_the_edges_the_issue_lists():
    batch = [c for c in C.SWEEP if c.entry == "batch" and not c.refused]
    assert {c.M for c in batch} >= set(C.M_LIST)
    assert {c.K for c in batch if c.mode == C.PLAIN} >= {72, 264, 2048, 2112, 3136, 4160, 4288}
    assert {c.N for c in batch if c.mode == C.PLAIN} >= {20, 2052, 4092, 4100, 8188, 8196, 16420}
    assert {c.N for c in batch if c.mode == C.SWIGLU} >= {32, 8224, 16448}
    assert {(c.n_q, c.n_kv) for c in batch if c.mode == C.QKV} == {(1, 1), (16, 2)}
    for mode in (C.PLAIN, C.SWIGLU, C.QKV):
        assert any(c.mode == mode and c.ldc % 4 for c in batch), f"mode {mode}: no case on the scalar-store arm"
        assert {C.case_route(c).cls for c in batch if c.mode == mode and c.norm} == {8, 16, 32}
    single = {c.claim for c in batch if not C.case_route(c).mp}
    assert single == {c.claim for c in batch if c.norm}, "fused norm on every single-piece route"
    for cls in (8, 16, 32):
        assert {(c.bias, c.res) for c in batch if c.mode == C.PLAIN and C.case_route(c).cls == cls} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c.res and c.ldr > c.N for c in batch) and any(c.ldx_pad for c in batch)
    assert any(C.case_route(c).units > 2 * 256 for c in batch if c.mode == C.PLAIN) and any(C.case_route(c).units > 2 * 256 for c in batch if c.mode == C.SWIGLU)
    gemv = [c for c in C.SWEEP if c.entry == "gemv"]
    assert {c.M for c in gemv} == {1, 2, 3, 4} and {c.act for c in gemv} == {0, 1, 2, 3, 5}
    assert {c.K for c in gemv} == {8, 520, 4096, 4104, 11008} and {c.N for c in gemv} == {1, 6, 130, 64}
    assert any(c.norm for c in gemv) and any(c.bias for c in gemv) and any(c.res for c in gemv)
    assert {c.M for c in C.SWEEP if c.entry == "combine"} == {1, 2}


@pytest.mark.parametrize("case", RUN, ids=lambda c: c.name)
def test_bound_passes_the_emulated_kernel_and_fails_every_fault(case):
    d = C.build(case)
    rb = C.reference_and_bound(d)
    emu = C.emulate(d)
    tight = C.reference_and_bound(d, acc=C.ACC / 4, exact_ulp=True, rstd_rel=C.RSTD_REL / 4)
    assert set(emu) == set(rb)
    e = over = 0.0
    for name, (ref, bound) in rb.items():
        assert torch.isfinite(ref).all() and (bound > 0).all()
        e = max(e, ((emu[name] - ref).abs() / bound).max().item())
        over = max(over, ((emu[name] - ref).abs() / tight[name][1]).max().item())
    acc = C.acc_error(d)
    rstd = C.rstd_error(d) if case.norm else 0.0
    WORST["emulate"], WORST["acc"], WORST["rstd"] = max(WORST["emulate"], e), max(WORST["acc"], acc), max(WORST["rstd"], rstd)
    print(f"\n{case.name}: emulation {e:.3f} of the bound ({over:.3f} of the sharp one); accumulation {acc:.3f} x 2^-24 S; rstd {rstd:.3f} x 2^-24")
    assert over <= 1.0, f"{case.name}: the emulated kernel is {over:.3f} of the sharp bound off the fp64 reference"
    assert acc <= C.ACC / 4, f"{case.name}: fp32 accumulation error {acc:.3f} x 2^-24 S: ACC = {C.ACC} is not 4 x that"
    assert rstd * 2.0 ** -24 <= C.RSTD_REL / 4, f"{case.name}: rstd error {rstd:.3f} x 2^-24: RSTD_REL is not 4 x that"
    faults = C.applicable_faults(d)
    WORST["pairs"] += len(C.FAULTS)
    WORST["na"] += len(C.FAULTS) - len(faults)
    ROUTE_FAULTS.setdefault(case.claim, set()).update(faults)
    assert faults, case.name
    for fault in faults:
        mut, regions = C.reference(d, fault)
        assert regions, f"{case.name}: '{fault}' touches nothing"
        for region in regions:
            w = C.region_worst(mut, rb, region)
            if w < WORST["fault"]:
                WORST["fault"], WORST["fault_at"] = w, f"{case.name} {fault} {region[0]}"
            assert w >= 2.0, f"{case.name}: '{fault}' moves region {region[0]} rows {region[1].tolist()} by only {w:.3g} x the bound"


def test_dropped_k_step_with_and_without_the_planted_columns(monkeypatch):
    """Measured, not assumed: under a per-element bound 64 dropped random products are already far beyond twice the bound somewhere in a
    unit, so at amplitude 0 the dropped k-step does not pass either (both figures are printed); the planted columns add a contribution of
    known size that does not depend on the draw."""
    for name in ("p8-h-k2048", "p16-r-mp4160", "p32-u16-mp-3136", "s8-mp2112"):
        case = next(c for c in C.SWEEP if c.name == name)
        w = {}
        for amp in (1.0, 0.0):
            monkeypatch.setattr(C, "PLANT", amp)
            d = C.build(case)
            rb = C.reference_and_bound(d)
            mut, regions = C.reference(d, "drop_wave_step")
            w[amp] = min(C.region_worst(mut, rb, r) for r in regions)
        print(f"\n{name}: dropped k-step {w[1.0]:.3g} x the bound with the planted columns, {w[0.0]:.3g} x without")
        assert w[1.0] >= 2.0


@pytest.mark.parametrize("name", ["p8-h-k72", "s8-oddldc", "g4-m3-gelu"])
def test_canary_check_passes_a_clean_buffer_and_fails_a_dirtied_one(name):
    d = C.build(next(c for c in C.SWEEP if c.name == name))
    c = d["case"]
    empty = C.host_buffers(d)["out"]
    with pytest.raises(AssertionError, match="never written"):
        C.check_canary(empty, d, name)
    buf = empty.clone()
    buf[:c.M, :c.n_out] = C.emulate(d)["out"].to(buf.dtype)
    C.check_canary(buf, d, name)
    for where in ((-1, -1), (0, -1)):
        dirty = buf.clone()
        dirty[where] = 0
        with pytest.raises(AssertionError, match="written"):
            C.check_canary(dirty, d, name)


def test_cache_canary_check_passes_exact_rows_and_fails_a_stray_or_missing_one():
    d = C.build(next(c for c in C.SWEEP if c.name == "q8-k72"))
    b = C.host_buffers(d)
    kc, vt = b["kc"].clone(), b["vt"].clone()
    with pytest.raises(AssertionError, match="never written"):
        C.check_cache_canary(kc, vt, d, "q")
    pos = d["state"][:, 0].long()
    kc[:, pos] = 1.0
    vt[:, pos] = 1.0
    C.check_cache_canary(kc, vt, d, "q")
    got = C.gather_outputs(d, b["out"], kc, vt)
    assert got["k"].shape == (1, 128) and got["v"].shape == (1, 128)
    for t, idx in ((kc, (0, int(pos[0]) + 1, 5)), (vt, (7, int(pos[0]) - 1))):
        t2 = t.clone()
        t2[idx] = 0
        with pytest.raises(AssertionError, match="other positions"):
            C.check_cache_canary(t2 if t is kc else kc, t2 if t is vt else vt, d, "q")


def test_zz_summary():
    print()
    if not WORST["pairs"]:
        return
    print(f"SUMMARY emulation at most {WORST['emulate']:.3f} of the bound; accumulation at most {WORST['acc']:.3f} x 2^-24 S (ACC = {C.ACC}); "
          f"rstd at most {WORST['rstd']:.3f} x 2^-24 (RSTD_REL = 2^{torch.log2(torch.tensor(C.RSTD_REL)).item():.0f}); "
          f"weakest fault {WORST['fault']:.3g} x the bound ({WORST['fault_at']}); {WORST['na']} of {WORST['pairs']} (case, fault) pairs "
          f"({100.0 * WORST['na'] / WORST['pairs']:.0f} %) not applicable")
    assert WORST["fault"] >= 2.0
    none = [k for k, v in ROUTE_FAULTS.items() if not v]
    assert not none, f"routes without an applicable fault: {none}"
    if len(ROUTE_FAULTS) == len({c.claim for c in RUN}):
        for f in C.FAULTS:
            assert any(f in v for v in ROUTE_FAULTS.values()), f"fault '{f}' applies to no case"
