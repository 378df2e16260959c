"""CPU half of the DaViT channel-attention / depthwise-conv sweep (tests/davit_op_cases.py): the case tables reach every edge and route, the
restated workspace layout and routing match the library and the constants of vision_ops.hip, every float64 reference agrees with an independent
formulation, the emulated kernel arithmetic passes every stage bound with the measured terms at half (the LayerNorm statistics term at a quarter,
as tests/test_small_op_cases.py holds it), every planted fault breaks the bound of its stage by 2 x in every unit it touches, and the constants
are what measure() derives.  Runs without a GPU; -s prints the figures recorded in the case module's docstring."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import davit_op_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CA, DW = D.CASES["chattn"], D.CASES["dwconv"]
_EMU = {}


def _emu(c):
    if c.name not in _EMU:
        _EMU[c.name] = (D.ca_emulate if c.family == "chattn" else D.dw_emulate)(c)
    return _EMU[c.name]


def _bits(t):
    return torch.nan_to_num(t.float(), nan=-7.0).view(torch.int32)


def _ratio(got, ref, bnd):
    return D.worst_ratio(got, ref, bnd)[0]


def test_case_tables_reach_every_edge_and_route():
    names = [c.name for c in D.ALL_CASES]
    assert len(names) == len(set(names))
    assert {c.C // 32 for c in CA} == {1, 3, 5, 8}
    uni = [c for c in CA if not c.ragged]
    for C in D.CA_C:
        assert {c.sizes[0] for c in uni if c.C == C and len(c.sizes) == 1} >= {n for n in D.CA_N if n <= 300}
        assert any(len(c.sizes) == 3 for c in uni if c.C == C) and any(c.ragged for c in CA if c.C == C)
    assert {c.sizes[0] for c in uni if c.C == 32} == set(D.CA_N)
    assert {D.cdiv(n, D.CA_TOK) for n in D.CA_N} == {1, 2, 3, 5, 9}               # the 4-way sum, its tail, both, neither
    rag = [c for c in CA if c.ragged]
    assert all(max(c.sizes) != c.sizes[0] for c in rag), "the largest image first"
    assert any(1 in c.sizes for c in rag) and any(len(set(c.sizes)) < len(c.sizes) for c in rag)
    for c in rag:
        assert len({D.cdiv(n, D.CA_TOK) for n in c.sizes}) > 1, "every image has the chunks of the largest"
        ends = [r + n for r, n in zip(c.rows, c.sizes)]
        assert c.rows[0] > 0 and any(b > a for a, b in zip(ends, c.rows[1:])) and all(b >= a for a, b in zip(ends, c.rows[1:]))
    for N in D.CA_N:
        p = set(D.ca_planted(N))
        want = {0, N - 1} | {t for t in range(64, N, 64)} | {t - 1 for t in range(64, N + 1, 64)} | {t - 1 for t in range(32, N + 1, 32)}
        assert p == want and all(0 <= t < N for t in p)
    # depthwise conv: the routes of the issue's table
    assert [(C, D.dw_ppw(C // 8)) for C in D.DW_PIX_C] == [(8, 4), (96, 4), (128, 4), (192, 2), (256, 2), (384, 1), (512, 1), (768, 1), (1024, 1),
                                                            (1536, 1), (2048, 1)]
    assert [D.dw_run_template(C // 8) for C in D.DW_RUN_C] == [(4, 1, 8), (2, 1, 8), (1, 1, 8), (1, 2, 4)]
    idle = [C for C in D.DW_PIX_C if (C // 8) % (64 // D.dw_ppw(C // 8)) != 0]
    assert idle == [8, 96, 192, 384, 768], idle                                   # sub + i * LPP >= chunks for some lane
    for c in DW:
        chunks, px, tot = c.C // 8, max(h * w for h, w in c.sizes), sum(h * w for h, w in c.sizes)
        px = tot if not c.ragged else px
        assert D.dwln_form(chunks, px, tot, 1) == 0, "the product rule keeps maps this small on the per-pixel form"
        assert D.dwln_form(chunks, px, tot, 0) == 0
        assert D.dwln_form(chunks, px, tot, 2) == (chunks if c.C in D.DW_RUN_C else 0)
        assert c.route != "run" or c.C in D.DW_RUN_C
    assert D.dwln_form(128, (1 << 20) + 1, (1 << 20) + 1, 2) == 0 and D.dwln_form(128, 1 << 20, 1 << 20, 2) == 128     # the 2 GiB limit of the run form's stores
    assert D.dwln_form(64, 8 * 4096, 8 * 4096, 1) == 64 and D.dwln_form(64, 8 * 4096 - 1, 8 * 4096 - 1, 1) == 0
    for route, widths in (("sep", D.DW_SEP_C), ("pix", D.DW_PIX_C), ("run", D.DW_RUN_C)):
        assert {c.C for c in DW if c.route == route} == set(widths)
        for C in widths:                                                            # every width of every route sees the whole shape list, batch 1 and 3
            cs = [c for c in DW if c.route == route and c.C == C]
            assert {(c.sizes[0], len(c.sizes)) for c in cs if not c.ragged} == {(s, b) for s in D.DW_SHAPES for b in (1, 3)}, (route, C)
            assert route == "sep" or any(c.ragged and len(set(c.sizes)) == 3 for c in cs), (route, C)
            if route == "run":
                run = D.dw_run_template(C // 8)[2]
                ws = {c.sizes[0][1] for c in cs if not c.ragged}
                assert any(w < run for w in ws) and any(w > run and w % run for w in ws) and any(w % run == 0 for w in ws) and 1 in ws, (C, run)


def test_restated_layout_matches_the_library_and_the_kernel_constants():
    src = open(os.path.join(ROOT, "vlm_fo1_amd", "csrc", "vision_ops.hip")).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))

    assert (const("kCaTok"), const("kDwRun"), const("kDwLnChunks")) == (D.CA_TOK, D.DW_RUN, D.DW_LN_CHUNKS)
    assert "constexpr int NB = 4;" in src and D.CA_BLOCK == 32 * 4
    assert max(D.DW_PIX_C) == 64 * D.DW_LN_CHUNKS * 8
    from vlm_fo1_amd import lib as L
    lib = L.load()
    for c in CA:
        lay = D.ca_layout(len(c.sizes), max(c.sizes), c.C)
        assert lib.fo1_channel_attention_workspace_bytes(max(c.sizes), c.C, len(c.sizes)) == lay["bytes"], c.name
        assert lib.fo1_channel_attention_var_workspace_bytes(max(c.sizes), c.C, len(c.sizes)) == lay["bytes"], c.name
        assert lay["bytes"] == 4 * (lay["part_floats"] + lay["a_floats"]) and lay["part_floats"] == len(c.sizes) * lay["slots"] * lay["G"] * 1024
        for route in D.CA_ROUTES:
            g = D.ca_grids(route, max(c.sizes), c.C, len(c.sizes))
            per_wg = 4 if route == "mfma" else 1
            assert g["gram"][0] == lay["slots"] and g["gram"][1] * per_wg >= lay["G"] > (g["gram"][1] - 1) * per_wg
            assert g["apply"][0] * (128 if route == "mfma" else 256) >= max(c.sizes)      # (no case reaches the FMA kernel's grid-stride loop)


def test_inputs_are_representable_planted_and_poisoned():
    smax = 0.0
    for c in CA:
        d, r = D.inputs(c), D.ca_reference(c)
        qkv = d["qkv"]
        assert qkv.dtype == torch.bfloat16 and torch.isfinite(qkv.float()).all()
        own = torch.zeros(qkv.shape[0], dtype=torch.bool)
        for N, r0 in zip(c.sizes, c.rows):
            assert not own[r0:r0 + N].any()
            own[r0:r0 + N] = True
        assert (qkv[~own].float() == D.POISON).all() and (~own).sum() >= 4 and qkv[own].float().abs().max() < 64
        for z, (q, k, v) in enumerate(D.ca_images(c)):
            pl = D.ca_planted(c.sizes[z])
            nz = (q[pl] != 0).sum(-1) + (k[pl] != 0).sum(-1)
            assert (nz == 2).all(), "a planted token carries one q and one k value per group"
            ent = q[pl].abs().argmax(-1) * 32 + k[pl].abs().argmax(-1)                  # [planted, G]
            assert all(ent[:, g].unique().numel() == len(pl) for g in range(ent.shape[1])), f"{c.name}: planted entries of a group collide"
            assert (v.abs().amax(-1) > 0).all()
            smax = max(smax, r["S"][z].abs().max().item())
            rows = r["A"][z].amax(-1)
            assert rows.max() > 0.2 and rows.min() < 0.1, f"{c.name}: peaked and nearly flat softmax rows"
    print(f"\nINPUTS chattn: max |S| {smax:.2f}")
    assert smax < 8.0, "logits stay below the binade whose half bf16 ulp is 2^-5"
    for c in DW:
        d = D.inputs(c)
        x = d["x"].float()
        keep = D.dw_image_rows(c)
        assert torch.isfinite(x).all() and (x[:keep.numel()][~keep] == D.POISON).all() and (x[keep.numel():] == D.POISON).all()
        if c.C >= 24:
            assert (d["w9"][:, -8:].float() == 0).all() and (d["bias"][8:16].float() == 0).all() and torch.signbit(d["bias"][8:16].float()).sum() == 4
        means = [x[r0:r0 + h * w].mean().item() for (h, w), r0 in zip(c.sizes, c.rows)]
        assert len(c.sizes) == 1 or c.ragged or all(abs((b - a) - 32.0) < 8.0 for a, b in zip(means, means[1:])), (c.name, means)


def test_reference_agrees_with_an_independent_formulation():
    for c in CA:
        r = D.ca_reference(c)
        qkv = D.inputs(c)["qkv"].double()
        for z, (N, r0) in enumerate(zip(c.sizes, c.rows)):
            # modeling_davit.py ChannelAttention: [1, groups, N, 32]; (q N^-0.5)^T k -> softmax(-1) -> (attention v^T)^T
            t = qkv[r0:r0 + N].reshape(1, N, 3, c.C // 32, 32).permute(2, 0, 3, 1, 4)
            q, k, v = t[0], t[1], t[2]
            att = ((q * N ** -0.5).transpose(-1, -2) @ k).softmax(dim=-1)
            other = (att @ v.transpose(-1, -2)).transpose(-1, -2)[0].permute(1, 0, 2)     # [N, G, 32]
            assert torch.allclose(r["out"][z], other, rtol=1e-11, atol=1e-12), c.name
            live = D.cdiv(N, D.CA_TOK)
            assert torch.allclose(r["gram"][z, :live].sum(0) / math.sqrt(N), r["S"][z], rtol=1e-12, atol=1e-12)
            assert torch.isnan(r["gram"][z, live:]).all() and r["ntok"][z].sum() == N
    for c in DW:
        r, d = D.dw_reference(c), D.inputs(c)
        for (H, W), r0 in zip(c.sizes, c.rows):
            x = d["x"][r0:r0 + H * W].double().view(1, H, W, c.C).permute(0, 3, 1, 2)
            w = d["w9"].double().t().reshape(c.C, 1, 3, 3)
            other = x + F.conv2d(x, w, d["bias"].double(), padding=1, groups=c.C)
            assert torch.allclose(r["y"][r0:r0 + H * W], other[0].permute(1, 2, 0).reshape(H * W, c.C), rtol=1e-12, atol=1e-10), c.name
        assert torch.isnan(r["y"][~D.dw_image_rows(c)]).all()


WORST = {}


def test_emulation_is_inside_every_bound_with_the_measured_terms_at_half():
    w = dict(gram=0.0, matrix=0.0, out=0.0, e2e=0.0)
    for c in CA:
        emu, r = _emu(c), D.ca_reference(c)
        live = ~torch.isnan(r["gram"])
        assert (emu["part"][~live] == D.FILL).all(), f"{c.name}: a dead slot was written"
        g = _ratio(emu["part"][live], r["gram"][live], D.ca_gram_bound(c)[live])
        assert g <= 0.5, f"{c.name}: Gram at {g:.3f} of the bound"
        w["gram"] = max(w["gram"], g)
        for z, (_, _, v) in enumerate(D.ca_images(c)):
            half = D.ca_matrix_bound(c, z, D.MAT_REL / 2, D.SUM_REL / 2)
            m = _ratio(emu["A"][z], r["A"][z], half)
            ref, bnd = D.ca_apply_reference(emu["A"][z], v)
            o = _ratio(emu["out"][z], ref, bnd)
            e = D.ca_e2e_ratio(emu["out"][z], r["out"][z])
            assert m <= 1.0 and o <= 1.0 and e <= D.E2E / 2, f"{c.name} image {z}: matrix {m:.3f}, output {o:.3f} of the bound, end to end {e:.4f}"
            assert (D.ca_matrix_bound(c, z) >= half).all()
            w["matrix"], w["out"], w["e2e"] = max(w["matrix"], m), max(w["out"], o), max(w["e2e"], e)
    wy = wh = 0.0
    for c in DW:
        emu, r, keep = _emu(c), D.dw_reference(c), D.dw_image_rows(c)
        R = keep.numel()
        assert torch.isnan(emu["y"][:R][~keep]).all() and torch.isnan(emu["y"][R:]).all()
        y = _ratio(emu["y"][:R][keep], r["y"][keep], D.dw_y_bound(c)[keep])
        assert y <= 1.0, f"{c.name}: y at {y:.3f} of the bound"
        wy = max(wy, y)
        if c.route != "sep":
            ref, bnd = D.dw_h_reference(c, emu["y"][:R][keep].to(torch.bfloat16), quarter=True)
            h = _ratio(emu["h"][:R][keep], ref, bnd)
            assert h <= 1.0, f"{c.name}: h at {h:.3f} of the quarter bound"
            wh = max(wh, h)
    WORST.update(w, dw_y=wy, dw_h=wh)
    print(f"\nEMULATION chattn: Gram {w['gram']:.4f}, matrix {w['matrix']:.3f} (MAT_REL / 2, SUM_REL / 2), output {w['out']:.3f} of the bound, end to end {w['e2e']:.4f} of the "
          f"row maximum; dwconv: y {wy:.3f} of the bound, h {wh:.3f} of the quarter bound")


MARGIN = {}


@pytest.mark.parametrize("fault", list(D.CA_FAULTS))
def test_every_channel_attention_fault_fails_its_stage(fault):
    stage = D.CA_FAULTS[fault][0]
    weakest, where, n_units = float("inf"), None, 0
    for c in CA:
        applies = [D.ca_fault_applies(c, fault, z) for z in range(len(c.sizes))]
        if not any(applies):
            continue
        good, bad, r = _emu(c), D.ca_emulate(c, fault), D.ca_reference(c)
        imgs = D.ca_images(c)
        for z, N in enumerate(c.sizes):
            units = []                                           # (touched, ratio) per unit of the stage
            if stage == "gram":
                bnd = D.ca_gram_bound(c)
                for s in range(D.cdiv(N, D.CA_TOK)):
                    for g in range(c.C // 32):
                        units.append((not torch.equal(bad["part"][z, s, g], good["part"][z, s, g]),
                                      _ratio(bad["part"][z, s, g], r["gram"][z, s, g], bnd[z, s, g])))
            elif stage == "matrix":
                bnd = D.ca_matrix_bound(c, z)
                for g in range(c.C // 32):
                    touched = not torch.equal(bad["A"][z, g], good["A"][z, g])
                    units.append((touched, float("inf") if fault in D.CA_BITWISE and touched else _ratio(bad["A"][z, g], r["A"][z][g], bnd[g])))
            elif stage == "out":
                ref, bnd = D.ca_apply_reference(good["A"][z], imgs[z][2])
                for g in range(c.C // 32):
                    units.append((not torch.equal(bad["out"][z][:, g], good["out"][z][:, g]), _ratio(bad["out"][z][:, g], ref[:, g], bnd[:, g])))
            else:
                units.append((len(bad["spill"][z]) > 0, float("inf")))
            touched = [u for t, u in units if t]
            assert not touched or applies[z], f"{c.name} image {z}: {fault} is said not to apply and changes the result"
            assert not applies[z] or touched, f"{c.name} image {z}: {fault} applies and changes nothing"
            n_units += len(touched)
            for u in touched:
                if u < weakest:
                    weakest, where = u, f"{c.name} image {z}"
                assert u >= 2.0, f"{c.name} image {z}: {fault} ({D.CA_FAULTS[fault][1]}) moves a {stage} unit by only {u:.3g} x its bound"
    assert n_units > 0, f"{fault}: no case"
    MARGIN[("chattn", fault)] = weakest
    print(f"\nFAULT chattn {fault}: {n_units} units, the weakest at {weakest:.3g} x the {stage} bound ({where})")


def test_unrounded_logits_stay_inside_the_matrix_bound():
    """What makes no_logit_round a bitwise fault: without the rounding the matrix is within the bound of the reference on every case."""
    for c in CA:
        bad, r = D.ca_emulate(c, "no_logit_round"), D.ca_reference(c)
        assert all(_ratio(bad["A"][z], r["A"][z], D.ca_matrix_bound(c, z)) <= 1.0 for z in range(len(c.sizes))), c.name


@pytest.mark.parametrize("fault", list(D.DW_FAULTS))
def test_every_dwconv_fault_fails_its_stage(fault):
    stage = D.DW_FAULTS[fault][0]
    weakest, where, n_units = float("inf"), None, 0
    for c in DW:
        if stage == "h" and c.route == "sep":
            continue
        applies = [D.dw_fault_applies(c, fault, b) for b in range(len(c.sizes))]
        if not any(applies):
            continue
        good, bad, r, keep = _emu(c), D.dw_emulate(c, fault), D.dw_reference(c), D.dw_image_rows(c)
        R, bnd = keep.numel(), D.dw_y_bound(c)
        outside = torch.cat([~keep, torch.ones(D.DW_SPARE, dtype=torch.bool)])
        spilled = bool((~torch.isnan(bad["y"][outside])).any())                  # a row of no image was written: the canary
        assert spilled == (fault == "short_run_spill"), c.name
        any_touched = spilled
        for b, ((H, W), r0) in enumerate(zip(c.sizes, c.rows)):
            sl = slice(r0, r0 + H * W)
            t = not torch.equal(_bits(bad[stage][sl]), _bits(good[stage][sl]))
            assert not t or applies[b] or fault == "short_run_spill", f"{c.name} image {b}: {fault} is said not to apply and changes the result"
            if fault != "short_run_spill":
                assert not applies[b] or t, f"{c.name} image {b}: {fault} applies and changes nothing"
            if not t:
                continue
            any_touched = True
            u = float("inf") if fault in D.DW_BITWISE else _ratio(bad["y"][sl], r["y"][sl], bnd[sl])
            n_units += 1
            if u < weakest:
                weakest, where = u, f"{c.name} image {b}"
            assert u >= 2.0, f"{c.name} image {b}: {fault} ({D.DW_FAULTS[fault][1]}) moves y by only {u:.3g} x its bound"
        assert any_touched, f"{c.name}: {fault} applies and changes nothing"
    assert n_units > 0, f"{fault}: no case"
    MARGIN[("dwconv", fault)] = weakest
    print(f"\nFAULT dwconv {fault}: {n_units} images, the weakest at {weakest:.3g} x the bound ({where})")


def test_zz_summary():
    m = D.measure(_emu)
    print(f"\nSUMMARY chattn fp32 softmax chain, relative: {m['mat']:.3e}; MAT_REL = 2^{math.log2(D.MAT_REL):.0f} = {D.MAT_REL:.3e}")
    print(f"SUMMARY chattn fp32 logit sums, relative to N^-0.5 sum |q||k|: {m['sum']:.3e}; SUM_REL = 2^{math.log2(D.SUM_REL):.0f} = {D.SUM_REL:.3e}")
    print(f"SUMMARY chattn emulation end to end: {m['e2e']:.4f} of the row maximum; E2E = 2^{math.log2(D.E2E):.0f}")
    # 4 x the measured figure, rounded up to a power of two, as tests/test_small_op_cases.py holds REL and SINE_T: re-measure when a seed or a case changes
    assert 4 * m["mat"] <= D.MAT_REL < 8 * m["mat"], f"MAT_REL {D.MAT_REL:.3e} is not the power of two at or above 4 x {m['mat']:.3e}"
    assert 4 * m["sum"] <= D.SUM_REL < 8 * m["sum"], f"SUM_REL {D.SUM_REL:.3e} is not the power of two at or above 4 x {m['sum']:.3e}"
    assert 2 * m["e2e"] <= D.E2E < 4 * m["e2e"], f"E2E {D.E2E} is not the power of two at or above 2 x {m['e2e']:.4f}"
    for fam in ("chattn", "dwconv"):
        ms = {f: v for (a, f), v in MARGIN.items() if a == fam and math.isfinite(v)}
        if ms:
            f = min(ms, key=ms.get)
            print(f"SUMMARY weakest {fam} fault: {f} at {ms[f]:.3g} x its bound")
