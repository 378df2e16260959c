"""DaViT channel attention and depthwise 3x3 conv, launch route by launch route, against the float64 references of tests/davit_op_cases.py.

Channel attention goes through fo1_channel_attention_bf16 / fo1_channel_attention_var_bf16 directly, so that the test owns every buffer: qkv rows of
ld = 3C + 8 in a canary frame with poison in every row of no image, out rows of ldo = C + 8 in canary, a workspace of exactly
fo1_channel_attention_workspace_bytes followed by a canary tail and filled with 1e30 before every launch.  Each of the three kernels is then held
to its own bound: every live partial Gram against the float64 sum over that chunk's tokens (dead slots keep the fill), the matrix against the
float64 softmax, the output against float64 A_dev v with the matrix the same launch produced, and the whole against the unrounded float64 chain per
(token, group) row.  `mfma` is the product library's route, `fma` the A/B library's with fo1_channel_attention_set_impl(0).

The depthwise conv: fo1_dwconv3x3_bf16 (product library), and fo1_dwconv3x3_ln_bf16 / _var_bf16 in the A/B library with fo1_dwconv_ln_set_form(0)
(per pixel) and (2) (runs); y against float64 x + conv(x) + bias, h against the float64 LayerNorm of the y the same launch returned, canary rows
after the last pixel and between ragged images.  Which kernel a call reaches is restated in the case module (ca_grids, dwln_form, dw_ppw) and
checked there against the source's constants: the profile rows carry one name for all forms of an op, so the route cannot be read back here.

Every case: canaries intact, inputs unchanged, a second launch bit-identical.  test_zz_summary prints one SUMMARY line per op and route."""
import time

import pytest
import torch

import davit_op_cases as D
from small_op_cases import CANARY16, CANARY32, CANARY_BF, CANARY_F32

pytestmark = pytest.mark.gpu

WORST = {}
T0 = time.time()
CA, DW = D.CASES["chattn"], D.CASES["dwconv"]


def _b16(t):
    return t.view(torch.int16)


def _b32(t):
    return t.view(torch.int32)


def _note(key, **figures):
    w = WORST.setdefault(key, {})
    for k, v in figures.items():
        w[k] = max(w.get(k, 0.0), v)


def _segs(c, sizes):
    t = torch.zeros(len(sizes), 8, dtype=torch.int32)
    for i, (r0, (h, w)) in enumerate(zip(c.rows, sizes)):
        t[i, :3] = torch.tensor([r0, h, w], dtype=torch.int32)
    return t.cuda()


# ---------------------------------------------------------------------------------------------------------------------------------------
# channel attention
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ca_launch(lib, c):
    """One launch -> (out buffer, workspace, qkv buffer after the launch, qkv buffer as it was sent) on the CPU."""
    from vlm_fo1_amd import lib as L
    C, n_img, Nmax = c.C, len(c.sizes), max(c.sizes)
    src = D.inputs(c)["qkv"]
    R, ld, ldo = src.shape[0], 3 * C + 8, C + 8
    qkv = torch.full((R, ld), CANARY_BF, dtype=torch.bfloat16)
    qkv[:, :3 * C] = src
    qkv_d = qkv.cuda()
    out_d = torch.full((R, ldo), CANARY_BF, dtype=torch.bfloat16).cuda()
    lay = D.ca_layout(n_img, Nmax, C)
    need = lib.fo1_channel_attention_workspace_bytes(Nmax, C, n_img)
    assert need == lay["bytes"]
    ws_d = torch.full((need // 4 + 64,), D.FILL, dtype=torch.float32, device="cuda")
    ws_d[need // 4:] = CANARY_F32
    st = L.current_stream_ptr()
    if c.ragged:
        segs = _segs(c, [(n, 1) for n in c.sizes])
        rc = lib.fo1_channel_attention_var_bf16(qkv_d.data_ptr(), ld, segs.data_ptr(), n_img, Nmax, sum(c.sizes), C, out_d.data_ptr(), ldo, ws_d.data_ptr(),
                                                need, st)
    else:
        r0 = c.rows[0]                              # the images start CA_LEAD rows into both buffers: poison and canary before the first token
        assert c.rows == tuple(r0 + z * Nmax for z in range(n_img)) and r0 * ld % 8 == 0 and r0 * ldo % 8 == 0
        rc = lib.fo1_channel_attention_bf16(qkv_d.data_ptr() + 2 * r0 * ld, ld, Nmax, C, out_d.data_ptr() + 2 * r0 * ldo, ldo, n_img, ws_d.data_ptr(),
                                            need, st)
    assert rc == 0, f"{c.name}: rc {rc}: {lib.fo1_last_error().decode()}"
    torch.cuda.synchronize()
    return out_d.cpu(), ws_d.cpu(), qkv_d.cpu(), qkv


def _ca_check(lib, c, route):
    out, ws, qkv_after, qkv_before = _ca_launch(lib, c)
    C, G, n_img = c.C, c.C // 32, len(c.sizes)
    lay, r = D.ca_layout(n_img, max(c.sizes), C), D.ca_reference(c)
    assert torch.equal(_b16(qkv_after), _b16(qkv_before)), f"{c.name}: the input changed"
    assert (_b32(ws[lay["bytes"] // 4:]) == CANARY32).all(), f"{c.name}: the canary after the workspace changed"
    part = ws[:lay["part_floats"]].view(n_img, lay["slots"], G, 32, 32)
    A = ws[lay["part_floats"]:lay["bytes"] // 4].view(n_img, G, 32, 32)
    live = ~torch.isnan(r["gram"])
    assert torch.isfinite(part).all() and torch.isfinite(A).all()
    assert (part[~live] == D.FILL).all(), f"{c.name}: a chunk slot past an image's own chunks was written"
    fig = dict(gram=D.worst_ratio(part[live], r["gram"][live], D.ca_gram_bound(c)[live])[0], matrix=0.0, out=0.0, e2e=0.0)
    assert torch.equal(D.rb(A), A), f"{c.name}: the matrix holds values that are not bf16"
    own = torch.zeros(out.shape[0], dtype=torch.bool)
    for z, ((q, k, v), N, r0) in enumerate(zip(D.ca_images(c), c.sizes, c.rows)):
        own[r0:r0 + N] = True
        got = out[r0:r0 + N, :C].float().view(N, G, 32)
        ref, bnd = D.ca_apply_reference(A[z], v)
        fig["matrix"] = max(fig["matrix"], D.worst_ratio(A[z], r["A"][z], D.ca_matrix_bound(c, z))[0])
        fig["out"] = max(fig["out"], D.worst_ratio(got, ref, bnd)[0])
        fig["e2e"] = max(fig["e2e"], D.ca_e2e_ratio(got, r["out"][z]))
    print(f"\nCASE {c.name} {route}: Gram {fig['gram']:.4f}, matrix {fig['matrix']:.3f}, output {fig['out']:.3f} of the bound, end to end {fig['e2e']:.4f} of the row maximum")
    assert fig["gram"] <= 1.0, f"{c.name} {route}: a partial Gram at {fig['gram']:.3g} x its bound"
    assert fig["matrix"] <= 1.0, f"{c.name} {route}: the attention matrix at {fig['matrix']:.3g} x its bound"
    assert fig["out"] <= 1.0, f"{c.name} {route}: the output at {fig['out']:.3g} x its bound against A_dev v"
    assert fig["e2e"] <= D.E2E, f"{c.name} {route}: end to end {fig['e2e']:.4g} of the row maximum, tolerance {D.E2E}"
    canary = _b16(out).clone()
    canary[own, :C] = CANARY16
    assert (canary == CANARY16).all(), f"{c.name}: the canary around the output changed (gap columns, rows of no image)"
    out2, ws2, _, _ = _ca_launch(lib, c)
    assert torch.equal(_b16(out2), _b16(out)) and torch.equal(_b32(ws2), _b32(ws)), f"{c.name}: a second launch gives other bits"
    _note(f"chattn {route} {'ragged' if c.ragged else 'uniform'}", **fig)


@pytest.mark.parametrize("case", CA, ids=[c.name for c in CA])
def test_channel_attention_mfma(case, product_library):
    _ca_check(product_library, case, "mfma")


@pytest.mark.parametrize("case", CA, ids=[c.name for c in CA])
def test_channel_attention_fma(case, ab_library):
    ab_library.fo1_channel_attention_set_impl(0)
    try:
        _ca_check(ab_library, case, "fma")
    finally:
        ab_library.fo1_channel_attention_set_impl(1)


def test_channel_attention_argument_checks(product_library):
    """Plain calls with a return code; none launches anything."""
    lib = product_library
    N, C = 40, 64
    ld, ldo = 3 * C + 8, C + 8
    qkv = torch.zeros(N + 1, ld, dtype=torch.bfloat16, device="cuda")
    out = torch.full((N + 1, ldo), CANARY_BF, dtype=torch.bfloat16, device="cuda")
    need = lib.fo1_channel_attention_workspace_bytes(N, C, 1)
    assert need == D.ca_layout(1, N, C)["bytes"]
    ws = torch.full((need // 4 + 8,), D.FILL, dtype=torch.float32, device="cuda")
    segs = _segs(D.Case("chattn", "args", rows=(0,)), [(N, 1)])

    def uni(ld_=ld, C_=C, out_=out.data_ptr(), ldo_=ldo, bytes_=need):
        return lib.fo1_channel_attention_bf16(qkv.data_ptr(), ld_, N, C_, out_, ldo_, 1, ws.data_ptr(), bytes_, None)

    def var(ld_=ld, C_=C, out_=out.data_ptr(), ldo_=ldo, bytes_=need):
        return lib.fo1_channel_attention_var_bf16(qkv.data_ptr(), ld_, segs.data_ptr(), 1, N, N, C_, out_, ldo_, ws.data_ptr(), bytes_, None)

    for call in (uni, var):
        assert call(bytes_=need - 1) == -2, "FO1_ERR_WORKSPACE"
        assert call(C_=48) == -1 and call(ld_=3 * C - 8) == -1 and call(ld_=3 * C + 4) == -1 and call(ldo_=C + 4) == -1
        assert call(out_=out.data_ptr() + 2) == -1 and call(out_=out.data_ptr() + 8) == -1
    torch.cuda.synchronize()
    assert (_b16(out.cpu()) == CANARY16).all() and (ws.cpu() == D.FILL).all(), "a rejected call wrote something"
    assert uni() == 0 and var() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# depthwise conv
# ---------------------------------------------------------------------------------------------------------------------------------------
def _dw_launch(lib, c):
    from vlm_fo1_amd import lib as L
    d = D.inputs(c)
    C, R = c.C, D.dw_total_rows(c)
    x = d["x"].cuda()
    w9, bias, lw, lb = (d[k].cuda() for k in ("w9", "bias", "ln_w", "ln_b"))
    y = torch.full((R + D.DW_SPARE, C), CANARY_BF, dtype=torch.bfloat16).cuda()
    h = torch.full((R + D.DW_SPARE, C), CANARY_BF, dtype=torch.bfloat16).cuda()
    st = L.current_stream_ptr()
    (H, W), B = c.sizes[0], len(c.sizes)
    if c.route == "sep":
        rc = lib.fo1_dwconv3x3_bf16(x.data_ptr(), w9.data_ptr(), bias.data_ptr(), y.data_ptr(), H, W, C, B, st)
    elif c.ragged:
        segs = _segs(c, c.sizes)
        rc = lib.fo1_dwconv3x3_ln_var_bf16(x.data_ptr(), w9.data_ptr(), bias.data_ptr(), y.data_ptr(), lw.data_ptr(), lb.data_ptr(), D.LN_EPS, h.data_ptr(),
                                           segs.data_ptr(), B, max(a * b for a, b in c.sizes), sum(a * b for a, b in c.sizes), C, st)
    else:
        rc = lib.fo1_dwconv3x3_ln_bf16(x.data_ptr(), w9.data_ptr(), bias.data_ptr(), y.data_ptr(), lw.data_ptr(), lb.data_ptr(), D.LN_EPS, h.data_ptr(),
                                       H, W, C, B, st)
    assert rc == 0, f"{c.name}: rc {rc}: {lib.fo1_last_error().decode()}"
    torch.cuda.synchronize()
    assert torch.equal(_b16(x.cpu()), _b16(d["x"])), f"{c.name}: the input changed"
    return y.cpu(), h.cpu()


def _dw_check(lib, c):
    y, h = _dw_launch(lib, c)
    r, keep = D.dw_reference(c), D.dw_image_rows(c)
    R = keep.numel()
    rows = torch.cat([keep, torch.zeros(D.DW_SPARE, dtype=torch.bool)])
    assert (_b16(y[~rows]) == CANARY16).all(), f"{c.name}: a row of y that belongs to no image was written"
    assert torch.isfinite(y[rows].float()).all()
    fy = D.worst_ratio(y[rows].float(), r["y"][keep], D.dw_y_bound(c)[keep])[0]
    fh = 0.0
    if c.route == "sep":
        assert (_b16(h) == CANARY16).all()
    else:
        assert (_b16(h[~rows]) == CANARY16).all(), f"{c.name}: a row of h that belongs to no image was written"
        ref, bnd = D.dw_h_reference(c, y[rows])
        fh = D.worst_ratio(h[rows].float(), ref, bnd)[0]
    print(f"\nCASE {c.name}: y {fy:.3f}, h {fh:.3f} of the bound")
    assert fy <= 1.0, f"{c.name}: y at {fy:.3g} x its bound"
    assert fh <= 1.0, f"{c.name}: h at {fh:.3g} x its bound against the LayerNorm of the returned y"
    y2, h2 = _dw_launch(lib, c)
    assert torch.equal(_b16(y2), _b16(y)) and torch.equal(_b16(h2), _b16(h)), f"{c.name}: a second launch gives other bits"
    chunks = c.C // 8
    kernel = "separate" if c.route == "sep" else (f"pixel <{D.dw_ppw(chunks)}>" if c.route == "pix" else "run <%d,%d,%d>" % D.dw_run_template(chunks))
    _note(f"dwconv {kernel} {'ragged' if c.ragged else 'uniform'}", y=fy, h=fh)


DW_SEP = [c for c in DW if c.route == "sep"]
DW_FUSED = [c for c in DW if c.route != "sep"]


@pytest.mark.parametrize("case", DW_SEP, ids=[c.name for c in DW_SEP])
def test_dwconv_separate(case, product_library):
    _dw_check(product_library, case)


@pytest.mark.parametrize("case", DW_FUSED, ids=[c.name for c in DW_FUSED])
def test_dwconv_layernorm_fused(case, ab_library):
    ab_library.fo1_dwconv_ln_set_form(D.DW_SET_FORM[case.route])
    try:
        _dw_check(ab_library, case)
    finally:
        ab_library.fo1_dwconv_ln_set_form(1)


def test_zz_summary():
    assert WORST, "run the whole file: the summary reports what the sweep measured"
    for key in sorted(WORST):
        print(f"\nSUMMARY {key}: worst " + ", ".join(f"{k} {v:.4f}" if k in ("gram", "e2e") else f"{k} {v:.3f}" for k, v in WORST[key].items()), end="")
    print(f"\nSUMMARY wall time {time.time() - T0:.1f} s for {len(D.ALL_CASES)} cases ({2 * len(CA) + len(DW)} launches checked)")
