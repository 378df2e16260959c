"""CPU half of the small-op sweep (tests/small_op_cases.py): the case tables reach every route, every float64 reference agrees with an independent
formulation, the emulated kernel arithmetic passes the bound with its measured term at a quarter, every planted fault fails it, and the constants
are 4 x (box_refine: 8 x) what the emulation measures.  Runs without a GPU; -s prints the figures recorded in the case module's docstring."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_op_cases as C

FAMILIES = list(C.CASES)


def test_case_names_are_unique_and_routes_covered():
    names = [c.name for c in C.ALL_CASES]
    assert len(names) == len(set(names))
    for op in ("rmsnorm", "layernorm", "layernorm_rows"):
        cases = [c for c in C.CASES["rownorm"] if c.op == op]
        assert {C.route(c.D) for c in cases} == set(C.ROUTES)
        for r in C.ROUTES:
            ds = sorted({c.D for c in cases if C.route(c.D) == r and c.ldx == c.D})
            lo, hi = ds[0], ds[-1]
            assert (lo == 8 or C.route(lo - 8) != r) and (hi == 4096 or C.route(hi + 8) != r), f"{op} {r}: both ends need a case, have {ds}"
            assert any(C.route(c.D) == r and c.ldx > c.D and c.ldy > c.D for c in cases), f"{op} {r}: no strided case"
        assert {c.M for c in cases} >= {1, 7, 9}
    assert [C.route(d) for d in C.ROW_D] == [r for r in C.ROUTES for _ in (0, 1)]
    assert {C.argmax_route(c.n) for c in C.CASES["argmax"]} == {"one", "two"}
    assert C.argmax_route(16383) == "one" and C.argmax_route(16384) == "two"
    assert {(c.C // c.G) for c in C.CASES["groupnorm"]} == {8, 16, 64}
    assert {-(-c.S // C.GN_TOK) for c in C.CASES["groupnorm"]} == {1, 2, 3}
    assert any(c.ldx > c.C for c in C.CASES["groupnorm"])


def test_inputs_are_representable_and_exact_adds_are_exact():
    for c in C.CASES["rownorm"] + C.CASES["groupnorm"]:
        d = C.inputs(c)
        assert d["x"].dtype == torch.bfloat16 and torch.isfinite(d["x"].float()).all()
    for c in C.CASES["swin"] + C.CASES["eltwise"]:
        d = C.inputs(c)
        if c.family == "swin" and c.op == "reverse_add":
            a, b = C.swin_reverse64(d["yw"].double(), c), d["x"].double()
        elif c.family == "eltwise" and c.op == "add":
            a, b = d["a"].double(), d["b"].double()
        else:
            continue
        assert torch.equal((a.float() + b.float()).double(), a + b), f"{c.name}: the fp32 sum is not exact"
    for c in C.CASES["groupnorm"]:
        d = C.inputs(c)
        x = d["x"].double().view(c.S, c.G, -1)
        if d["const"] is not None:
            assert x[:, d["const"]].std().item() == 0 and x[:, d["const"]].abs().max().item() <= 1
        ratio = x.mean(dim=(0, 2)).abs() / x.var(dim=(0, 2), unbiased=False).sqrt().clamp_min(1e-30)
        plain = [g for g in range(c.G) if g not in (d["const"], d["tiny"])]
        if c.S * (c.C // c.G) >= 2048:          # enough samples for the realised ratio to show the 16 sigma of the construction
            assert 14.0 <= ratio[plain].max().item() <= 17.5, c.name


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_agrees_with_an_independent_formulation(family):
    for c in C.CASES[family]:
        ref, d = C.reference(c), C.inputs(c)
        if family == "rownorm":
            x, w, b = d["x"].double(), d["w"].double(), d["b"].double()
            if c.op == "rmsnorm":     # Qwen2RMSNorm: weight * (x * rsqrt(mean(x^2) + eps))
                other = w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + C.RMS_EPS))
            else:
                other = F.layer_norm(x, (c.D,), w, b, C.LN_EPS)
            assert torch.allclose(ref, other, rtol=1e-12, atol=1e-12), c.name
        elif family == "groupnorm":
            x = d["x"].double().t()[None]                                     # [1, C, S]
            other = F.group_norm(x, c.G, d["w"].double(), d["b"].double(), C.GN_EPS)[0].t()
            assert torch.allclose(ref, other, rtol=1e-10, atol=1e-10), c.name
        elif family == "swin":
            # per image and per window, straight from the definition: window (wy, wx), local (iy, ix) <- rolled padded image
            nWy, nWx, Hp, Wp = C._swin_dims(c)
            ws = c.ws
            x = d["x"].float().view(c.B, c.H, c.W, c.C)
            xp = torch.zeros(c.B, Hp, Wp, c.C)
            xp[:, :c.H, :c.W] = x
            if c.op == "partition":
                other = torch.stack([xp[b, (wy * ws + iy + c.shift) % Hp, (wx * ws + ix + c.shift) % Wp]
                                     for b in range(c.B) for wy in range(nWy) for wx in range(nWx) for iy in range(ws) for ix in range(ws)])
                assert torch.equal(ref.float(), other), c.name
            else:
                yw = d["yw"].float().view(c.B, nWy, nWx, ws, ws, c.C)
                hh = (torch.arange(c.H) - c.shift) % Hp
                ww = (torch.arange(c.W) - c.shift) % Wp
                other = yw[:, hh[:, None] // ws, ww[None, :] // ws, hh[:, None] % ws, ww[None, :] % ws] + x
                assert torch.equal(ref.float(), other.reshape(-1, c.C).bfloat16().float()), c.name
                # partition then reverse with a zero shortcut is the identity on the H x W map
                assert torch.equal(C.swin_reverse64(C.swin_partition64(d["x"], c), c), d["x"]), c.name
        elif family == "patch_merge":
            x = d["x"].view(c.B, c.H, c.W, c.C)
            Ho, Wo = (c.H + 1) // 2, (c.W + 1) // 2
            other = torch.zeros(c.B, Ho, Wo, 4, c.C, dtype=torch.bfloat16)
            for q, (dh, dw) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                part = x[:, dh::2, dw::2]
                other[:, :part.shape[1], :part.shape[2], q] = part
            assert torch.equal(ref, other.reshape(-1, 4 * c.C)), c.name
        elif family == "sine_embed":
            from oracle import upn_oracle as O
            other = O.sine_embed(d["ref"].double())        # the oracle's dim_t is fp32: 1e-7 relative on the angle
            assert (ref - other.double()).abs().max().item() <= 4e-6, c.name
        elif family == "box_refine":
            dl, r = d["delta"].double(), d["ref"].double()
            if c.mode == 0:
                x = r.clamp(min=0, max=1)
                other = torch.sigmoid(dl + torch.log(x.clamp(min=1e-3) / (1 - x).clamp(min=1e-3)))
            else:
                other = dl + r if c.mode == 1 else torch.sigmoid(dl + r)
            fin = torch.isfinite(other)
            assert torch.equal(fin, torch.isfinite(ref)) and torch.equal(other[~fin], ref[~fin]), c.name
            assert torch.allclose(ref[fin], other[fin], rtol=2e-7, atol=0), c.name    # eps: float32(1e-3) in the kernel, 1e-3 here
            if c.mode == 1:
                assert (ref[torch.isinf(r)] == float("inf")).all()
        elif family == "topk":
            v = d["v"].tolist()
            other = sorted(range(c.n), key=lambda i: (math.isnan(v[i]), -v[i] if not math.isnan(v[i]) else 0.0))[:c.k]
            assert ref.tolist() == other, c.name
        elif family == "argmax":
            v = d["row"].float().tolist()
            assert ref.item() == v.index(max(v)), c.name
        elif family == "eltwise":
            if c.op == "swiglu":
                g, u = d["gu"][:, :c.D].double(), d["gu"][:, c.D:].double()
                assert torch.allclose(ref, F.silu(g) * u, rtol=1e-12, atol=1e-14), c.name
            elif c.op == "bias_act" and c.act == 1:
                v = d["x"].double() + (d["bias"].double() if c.bias else 0.0)
                assert torch.allclose(ref, F.gelu(v), rtol=1e-12, atol=1e-14), c.name
            elif c.op == "gather_rows":
                assert all(torch.equal(ref[i], d["table"][int(d["idx"][i])]) for i in range(c.M)), c.name
                assert len(set(d["idx"].tolist())) < c.M or c.M == 1
            elif c.op == "mask_rows":
                assert all(torch.equal(ref[m], d["x"][m] if int(d["keep"][m]) else torch.zeros(c.D, dtype=torch.bfloat16)) for m in range(c.M)), c.name
        elif family == "preprocess":
            assert torch.equal(ref.view(torch.int16), C.emulate(c).view(torch.int16)), c.name     # index walk vs slicing
            lut = d["lut"].view(torch.int16)
            assert lut.unique().numel() == 768 and torch.isfinite(d["lut"].float()).all()


WORST = {}


@pytest.mark.parametrize("family", FAMILIES)
def test_emulation_is_inside_the_quarter_bound(family):
    worst = 0.0
    for c in C.CASES[family]:
        ref, bnd, emu = C.reference(c), C.bound(c, quarter=True), C.emulate(c)
        if bnd is None:
            same = torch.equal(emu.view(torch.int16), ref.view(torch.int16)) if ref.dtype == torch.bfloat16 else torch.equal(emu, ref)
            assert same, f"{c.name}: the emulation of an exact op differs from its reference"
            continue
        w, at = C.worst_ratio(emu, ref, bnd)
        assert w <= 1.0, f"{c.name}: emulation at {w:.3f} of the quarter bound (flat index {at})"
        assert (C.bound(c) >= bnd).all()
        worst = max(worst, w)
    WORST[family] = worst
    print(f"\nEMULATION {family}: worst {worst:.3f} of the quarter bound over {len(C.CASES[family])} cases")


FAULT_MARGIN = {}


@pytest.mark.parametrize("family,fault", [(fam, f) for fam in C.FAULTS for f in C.FAULTS[fam]])
def test_every_fault_fails(family, fault):
    best, where = 0.0, None
    for c in C.CASES[family]:
        ref, bnd = C.reference(c), C.bound(c)
        bad = C.emulate(c, fault)
        if bnd is None or (family, fault) in C.BITWISE_FAULTS:
            good = C.emulate(c)
            bits = (lambda t: t.view(torch.int16)) if good.dtype == torch.bfloat16 else (lambda t: t)
            changed = bad.shape != good.shape or not torch.equal(bits(bad), bits(good))
            if bnd is None:
                wrong = bad.shape != ref.shape or not torch.equal(bits(bad), bits(ref if ref.dtype == good.dtype else ref.to(good.dtype)))
                changed = changed and wrong
            m = float("inf") if changed else 0.0
        else:
            m = C.worst_ratio(bad, ref, bnd)[0]
        if m > best:
            best, where = m, c.name
    FAULT_MARGIN[(family, fault)] = (best, where)
    print(f"\nFAULT {family} {fault}: moves an element by {best:.3g} x the bound ({where})")
    assert best >= 2.0, f"{family} / {fault} ({C.FAULTS[family][fault]}): no case fails, best {best:.3g} x the bound"


def test_rms_inner_rounding_fault_cannot_leave_the_bound():
    """The docstring's claim: without the inner rounding the result is within the bound of the reference on every case (it is closer to it)."""
    for c in C.CASES["rownorm"]:
        if c.op == "rmsnorm":
            assert C.worst_ratio(C._rownorm_emul(c, "rms_no_inner_round")[0], C.reference(c), C.bound(c))[0] <= 1.0


def test_layernorm_rows_map_is_a_permutation_with_gaps():
    for c in C.CASES["rownorm"]:
        if c.op == "layernorm_rows":
            d = C.inputs(c)
            rows = d["rows"].tolist()
            assert len(set(rows)) == c.M and max(rows) < d["y_rows"] and (c.M == 1 or rows != sorted(rows) or c.M < 3)
            twin = next(k for k in C.CASES["rownorm"] if k.op == "layernorm" and (k.D, k.M, k.ldx) == (c.D, c.M, c.ldx))
            assert torch.equal(C.inputs(twin)["x"].view(torch.int16), d["x"].view(torch.int16))


def test_zz_summary():
    m = C.measure()
    u = 2.0 ** -24
    print(f"\nSUMMARY rstd relative error of the emulation: rmsnorm {m['rmsnorm']:.3e} ({m['rmsnorm'] / u:.2f} x 2^-24), layernorm {m['layernorm']:.3e} "
          f"({m['layernorm'] / u:.2f} x 2^-24), groupnorm {m['groupnorm']:.3e} ({m['groupnorm'] / u:.1f} x 2^-24)")
    print(f"SUMMARY REL: rmsnorm 2^{math.log2(C.REL['rmsnorm']):.0f}, layernorm 2^{math.log2(C.REL['layernorm']):.0f}, groupnorm 2^{math.log2(C.REL['groupnorm']):.0f}")
    print(f"SUMMARY sine_embed fp32 chain vs fp64: {m['sine']:.3e}; SINE_T = 2^{math.log2(C.SINE_T):.0f} = {C.SINE_T:.3e}")
    print(f"SUMMARY box_refine fp32 chain vs fp64: relative {m['box_rel']:.3e}, absolute below 2^-10 {m['box_abs']:.3e}; BOX_REL = 2^{math.log2(C.BOX_REL):.0f}, "
          f"BOX_ABS = 2^{math.log2(C.BOX_ABS):.0f}")
    for key, const, mult in (("rmsnorm", C.REL["rmsnorm"], 4), ("layernorm", C.REL["layernorm"], 4), ("groupnorm", C.REL["groupnorm"], 4),
                             ("sine", C.SINE_T, 4), ("box_rel", C.BOX_REL, 8), ("box_abs", C.BOX_ABS, 8)):
        assert mult * m[key] <= const < 2 * mult * m[key], f"{key}: constant {const:.3e} is not the power of two next above {mult} x {m[key]:.3e}"   # (re-measure after changing a case)
    assert C.REL["layernorm_rows"] == C.REL["layernorm"]
