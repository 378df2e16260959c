"""The GEMM sweep's routing model, bound and faults on the CPU (no GPU; tests/gemm_route_cases.py):
  * the routing model gives every case of SWEEP the route its row claims, and the automatically dispatched cases cover every route label —
    kernel, tile, ring depth, split-K plane count — that the model reaches over a grid of shapes (a reachable label without a case fails);
  * on every case, scaled down to two tiles each way with the original's route and K: the emulated kernel arithmetic stays within the
    SHARP form of the per-element bound — every rounding point at the half ulp of the value's own binade, the accumulation term at
    ACC / 4 — and within half the bound itself where the output has no bf16 rounding (fp32 out, partial planes; on bf16 outputs the
    bound's 2^-8 |v| is the exact worst case of round-to-nearest, which a correct kernel reaches); its fp32 accumulation error stays
    within ACC / 4 of 2^-24 S; and every applicable fault of FAULTS moves some element of every tile it touches by at least twice the
    bound, and touches at least one tile;
  * without the planted columns a dropped chunk passes; check_canary passes a clean buffer and fails a dirtied one.
Run time: under 10 s (tests/test_decode_attention_cases.py 19 s, tests/test_prefill_attention_cases.py 24 s)."""
import itertools

import pytest
import torch

import gemm_route_cases as C

GRID_M = (5, 33, 64, 65, 100, 128, 129, 200, 391, 515, 700, 1000, 1024, 1300, 1564, 2048, 4096, 8192, 16300)
GRID_N = (64, 128, 328, 512, 1024, 2048, 2560, 3424, 4096, 6656, 8192, 16768, 22016, 32768, 65536, 151936)
GRID_K = (64, 72, 128, 256, 1024, 1176, 2048, 4096, 5888, 11008)


def test_sweep_names_are_unique_and_every_claim_is_the_models_route():
    assert len({c.name for c in C.SWEEP}) == len(C.SWEEP)
    for c in C.SWEEP:
        assert C.claim_of(C.case_route(c)) == c.claim, f"{c.name}: the model routes it to {C.claim_of(C.case_route(c))}, the table claims {c.claim}"
        assert c.ldc_pad > 0 and c.lda_pad % 8 == 0 and c.ldw_pad % 8 == 0


def test_auto_cases_cover_every_route_the_heuristic_reaches():
    reachable = {}
    for M, N, K in itertools.product(GRID_M, GRID_N, GRID_K):
        for act, f32 in ((0, False), (0, True), (C.ACT_SWIGLU, False)):
            if act == C.ACT_SWIGLU and N % 32:
                continue
            reachable.setdefault(C.claim_of(C.route(M, N, K, act, f32)), (M, N, K, act, f32))
    for M, N, K in ((3, 512, 512), (1300, 6656, 256)):
        for mult in (8, 4, 1):      # the alignment of ldc and of the residual's ldr: coalesced / fragment epilogue / no 256 x 256 form
            reachable.setdefault(C.claim_of(C.route(M, N, K, ldc_mult=mult)), (M, N, K, "ldc multiple", mult))
            reachable.setdefault(C.claim_of(C.route(M, N, K, res=True, ldr_mult=mult)), (M, N, K, "ldr multiple", mult))
    covered = {c.claim for c in C.SWEEP if c.auto() and c.entry == "gemm"}
    missing = {k: v for k, v in reachable.items() if k not in covered}
    assert not missing, f"routes reached by automatic dispatch with no case in SWEEP: {missing}"
    assert len(reachable) >= 21, sorted(reachable)       # 3 register tiles, 4 two-stage, 4 rings, planes 2..8, p4, p4 frag, gemv
    partial = {c.claim.split(" splitk")[0] for c in C.SWEEP if c.entry == "partials" and c.pin.auto()}
    assert partial == {"ring<64,64,3>", "ring<64,128,3>", "glds<128,256>"}


def test_sweep_covers_the_edges_the_issue_lists():
    auto = [c for c in C.SWEEP if c.entry == "gemm" and C.case_route(c).kind != "gemv"]
    edges_m, edges_n, residues, k_tail = set(), set(), set(), set()
    for c in auto:
        r = C.case_route(c)
        edges_m.add("below" if c.M % r.BM == r.BM - 1 else ("at" if c.M % r.BM == 0 else ("above" if c.M % r.BM == 1 else "")))
        edges_n.add("below" if c.N % r.BN == r.BN - 1 else ("at" if c.N % r.BN == 0 else ("above" if c.N % r.BN == 1 else "")))
        if c.M < r.BM:
            edges_m.add("short")
        if (r.kind, r.BM, r.BN) == ("ring", 64, 64):
            residues.add(C.cdiv(c.M, 64) * C.cdiv(c.N, 64) % 8)
        if r.kind == "reg":
            k_tail.add(c.K % 64)
    assert {"below", "at", "above", "short"} <= edges_m and {"below", "at", "above"} <= edges_n
    assert residues == set(range(8)), residues
    assert {8, 24, 56} <= k_tail
    assert any(C.case_route(c).kind == "big" and C.cdiv(c.M, 256) % 2 == 1 for c in auto)
    assert any(C.case_route(c).kind == "ring" and c.K // 64 < C.case_route(c).ring_depth() for c in auto)
    for what in ("lda_pad", "ldw_pad", "ldr_pad"):
        assert any(getattr(c, what) for c in auto)
    assert any(c.res and c.ldr != c.ldc for c in auto)
    # every epilogue the entry accepts, on every family's epilogue code
    def family(c):
        r = C.case_route(c)
        if r.reduce:
            return "reduce"
        if r.kind == "big":
            return "coalesced" if r.coal else "fragment32"
        vec = c.ldc % 4 == 0 and c.N % 4 == 0 and not c.out_f32 and c.act != C.ACT_SWIGLU and (not c.res or c.ldr % 4 == 0)
        return "epilogue_vec" if vec else "epilogue"
    have = {}
    for c in auto:
        have.setdefault(family(c), set()).update({f"act{c.act}"} | ({"bias"} if c.bias else set()) | ({"res"} if c.res else set()) | ({"f32"} if c.out_f32 else set()))
    assert have["epilogue_vec"] >= {"act0", "act1", "act2", "act5", "bias", "res"}, have
    assert have["epilogue"] >= {"act0", "act1", "act2", "act3", "act5", "bias", "res", "f32"}, have
    assert have["reduce"] >= {"act0", "act1", "act2", "act5", "bias", "res", "f32"}, have
    assert have["coalesced"] >= {"act0", "act1", "act2", "act3", "bias", "res"}, have      # (ReLU: no 256 x 256 form, it falls back)
    assert have["fragment32"] >= {"act1", "act3", "bias", "res"}, have


WORST = {"emulate": 0.0, "acc": 0.0, "fault": float("inf")}


@pytest.mark.parametrize("case", [C.scale_down(c) for c in C.SWEEP if C.case_route(c).kind != "gemv"], ids=lambda c: c.name)
def test_bound_passes_the_emulated_kernel_and_fails_every_fault(case):
    d = C.build(case)
    assert C.claim_of(d["route"]) == case.claim
    ref, bound = C.reference_and_bound(d)
    assert torch.isfinite(ref).all() and (bound > 0).all()
    emu = ((C.emulate(d) - ref).abs() / bound).max().item()
    acc = C.acc_error(d)
    WORST["emulate"], WORST["acc"] = max(WORST["emulate"], emu), max(WORST["acc"], acc)
    print(f"\n{case.name}: emulation {emu:.3f} of the bound; accumulation {acc:.3f} x 2^-24 S (worst so far {WORST['emulate']:.3f}, {WORST['acc']:.3f})")
    tight = C.reference_and_bound(d, acc=C.ACC / 4, exact_ulp=True)[1]
    over = ((C.emulate(d) - ref).abs() / tight).max().item()
    assert over <= 1.0, f"{case.name}: the emulated kernel is {over:.3f} of the sharp bound (exact half ulps, ACC / 4) off the fp64 reference ({emu:.3f} of the bound)"
    if case.out_f32 or case.entry == "partials":
        assert emu <= 0.5, f"{case.name}: the emulated kernel is {emu:.3f} of the bound off the fp64 reference"
    assert acc <= C.ACC / 4, f"{case.name}: fp32 accumulation error {acc:.3f} x 2^-24 S: ACC = {C.ACC} is not 4 x that"
    faults = C.applicable_faults(d)
    assert len(faults) >= 6, (case.name, faults)
    for fault in faults:
        mut, regions = C.reference(d, fault)
        assert regions, f"{case.name}: '{fault}' touches no tile"
        for region in regions:
            w = C.region_worst(mut, ref, bound, region)
            WORST["fault"] = min(WORST["fault"], w)
            assert w >= 2.0, f"{case.name}: '{fault}' moves tile {region} by only {w:.3g} x the bound"
    print(f"{case.name}: {len(faults)} faults, weakest so far {WORST['fault']:.3g} x the bound")


@pytest.mark.parametrize("name, fault", [("glds64x128-silu-res", "drop_chunk:last"), ("glds128x128-relu-res", "drop_chunk:tile_hi"),
                                         ("glds128x256", "dup_chunk:tile_hi")])
def test_without_the_planted_columns_a_dropped_chunk_passes(name, fault, monkeypatch):
    """The planted columns are what makes these faults gross: at amplitude 0 the same fault stays under twice the bound."""
    case = C.scale_down(next(c for c in C.SWEEP if c.name == name))
    d = C.build(case)
    ref, bound = C.reference_and_bound(d)
    mut, regions = C.reference(d, fault)
    assert min(C.region_worst(mut, ref, bound, r) for r in regions) >= 2.0
    monkeypatch.setattr(C, "PLANT", 0.0)
    d = C.build(case)
    ref, bound = C.reference_and_bound(d)
    mut, regions = C.reference(d, fault)
    assert min(C.region_worst(mut, ref, bound, r) for r in regions) < 2.0


@pytest.mark.parametrize("name", ["reg64x64-tiny-silu-res", "ring64x64-swiglu", "reg64x64-f32", "partials64x64-fewer"])
def test_canary_check_passes_a_clean_buffer_and_fails_a_dirtied_one(name):
    d = C.build(next(c for c in C.SWEEP if c.name == name))
    c = d["case"]
    empty = C.host_buffers(d)["out"]
    with pytest.raises(AssertionError, match="never written"):
        C.check_canary(empty, d, name)
    buf = empty.clone()
    emu = C.emulate(d)
    if c.entry == "partials":
        buf[:d["route"].splits] = emu.float()
    else:
        buf[:c.M, :c.n_out] = emu.to(buf.dtype)
    C.check_canary(buf, d, name)
    for where in ((-1, -1), (0, -1)) if c.entry != "partials" else ((-1, 0, 0),):
        dirty = buf.clone()
        dirty[where] = 0
        with pytest.raises(AssertionError, match="written"):
            C.check_canary(dirty, d, name)
