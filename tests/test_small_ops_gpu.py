"""The small exported kernels op by op against the float64 references of tests/small_op_cases.py: swin_ops.hip, upn_ops.hip, the six rownorm routes,
argmax's two routes, add / bias_act / swiglu and preprocess.hip.

Every case is built on the CPU, uploaded (strided operands as column views of a wider canary-filled buffer), run through vlm_fo1_amd.ops and held to
  * reference(case) under bound(case) element by element, or bit for bit where bound(case) is None;
  * the canary: nothing outside the written region of a strided output (or of a strided input) changed;
  * a second launch gives the same bits.
layernorm_rows: the rows named by the map equal layernorm of the same input bit for bit, every other row keeps the canary.
Each case feeds WORST; test_zz_summary prints one "SUMMARY <op> <route>: worst <fraction of bound>" line per op and route (exact ops: "exact")."""
import time

import pytest
import torch

import small_op_cases as C

pytestmark = pytest.mark.gpu

WORST = {}
T0 = time.time()


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _view(t: torch.Tensor, ld: int):
    """-> (device buffer [M + 1, ld] with the canary around t, its [M, D] view)."""
    buf = C.framed(t, ld).cuda()
    return buf, buf[:t.shape[0], :t.shape[1]]


def _out(M: int, D: int, ld: int, dtype=torch.bfloat16):
    buf = C.framed(torch.zeros(M, D, dtype=dtype), ld)
    buf[:] = C.CANARY_F32 if dtype == torch.float32 else C.CANARY_BF
    buf = buf.cuda()
    return buf, buf[:M, :D]


def _launch(c):
    """One launch -> (result on the CPU, [(buffer on the CPU, rows, columns written / holding the operand)])."""
    from vlm_fo1_amd import ops
    d, fam = C.inputs(c), c.family
    frames = []

    def track(buf, M, D):
        frames.append((buf, M, D))

    if fam == "rownorm":
        xb, x = _view(d["x"], c.ldx)
        w, b = d["w"].cuda(), d["b"].cuda()
        track(xb, c.M, c.D)
        if c.op == "layernorm_rows":
            R = d["y_rows"]
            yb, y = _out(R, c.D, c.ldy)
            ops.layernorm_rows(x, w, b, C.LN_EPS, y, d["rows"].cuda())
            named = y[d["rows"].long().cuda()].cpu()
            yb_cpu = yb.cpu()
            keep = torch.ones(R + 1, dtype=torch.bool)
            keep[d["rows"].long()] = False
            assert (_bits(yb_cpu[keep]) == C.CANARY16).all(), f"{c.name}: a row the map does not name was written"
            assert (_bits(yb_cpu[~keep][:, c.D:]) == C.CANARY16).all(), f"{c.name}: columns past D written"
            plain = ops.layernorm(x, w, b, C.LN_EPS).cpu()
            assert torch.equal(_bits(named), _bits(plain)), f"{c.name}: layernorm_rows differs from layernorm"
            res = named
        else:
            yb, y = _out(c.M, c.D, c.ldy)
            track(yb, c.M, c.D)
            if c.op == "rmsnorm":
                ops.rmsnorm(x, w, C.RMS_EPS, out=y)
            else:
                ops.layernorm(x, w, b, C.LN_EPS, out=y)
            res = y.cpu()
    elif fam == "groupnorm":
        xb, x = _view(d["x"], c.ldx)
        track(xb, c.S, c.C)
        res = ops.groupnorm_tokens(x, c.G, d["w"].cuda(), d["b"].cuda(), C.GN_EPS).cpu()
    elif fam == "swin":
        if c.op == "partition":
            res = ops.swin_window_partition(d["x"].cuda(), c.H, c.W, c.ws, c.shift, c.B).cpu()
        else:
            res = ops.swin_window_reverse_add(d["yw"].cuda(), d["x"].cuda(), c.H, c.W, c.ws, c.shift, c.B).cpu()
            zero = torch.zeros_like(d["x"]).cuda()
            back = ops.swin_window_reverse_add(ops.swin_window_partition(d["x"].cuda(), c.H, c.W, c.ws, c.shift, c.B), zero, c.H, c.W, c.ws, c.shift, c.B)
            # by value: x + 0 turns a -0.0 of x into +0.0
            assert torch.equal(back.cpu().float(), d["x"].float()), f"{c.name}: partition then reverse-add of zero is not the identity"
    elif fam == "patch_merge":
        res = ops.patch_merge(d["x"].cuda(), c.H, c.W, c.B).cpu()
    elif fam == "sine_embed":
        rb_ = d["buf"].cuda()
        res = ops.sine_embed(rb_[:, :c.dims], c.dims).cpu()
        assert torch.equal(_bits(rb_.cpu()), _bits(d["buf"]))
    elif fam == "box_refine":
        db, rbuf = d["delta_buf"].cuda(), d["ref_buf"].cuda()
        ob, o = _out(c.n, 4, c.ldo, torch.float32)
        track(ob, c.n, 4)
        ops.box_refine(db[:, :4], rbuf[:, :4], c.mode, out=o)
        res = o.cpu()
        assert torch.equal(_bits(db.cpu()), _bits(d["delta_buf"])) and torch.equal(_bits(rbuf.cpu()), _bits(d["ref_buf"]))
    elif fam == "topk":
        sc = d["scores"].cuda()
        idx, val = ops.topk_desc(sc, c.k, stride=c.stride, n=c.n)
        res = idx.cpu().long()
        want = d["v"][C.reference(c)]
        assert torch.equal(_bits(val.cpu()), _bits(want)), f"{c.name}: values are not scores[idx] of the expected order"
        assert torch.equal(_bits(sc.cpu()), _bits(d["scores"]))
    elif fam == "argmax":
        res = ops.argmax(d["row"].cuda()).cpu().long()
    elif fam == "eltwise":
        M, D = c.M, c.D
        if c.op == "add":
            ab, a = _view(d["a"], c.lda)
            bb, b = _view(d["b"], c.ldb)
            yb, y = _out(M, D, c.ldy)
            track(ab, M, D), track(bb, M, D), track(yb, M, D)
            ops.add(a, b, out=y)
            res = y.cpu()
        elif c.op == "bias_act":
            xb, x = _view(d["x"], c.ldx)
            yb, y = _out(M, D, c.ldy)
            track(xb, M, D), track(yb, M, D)
            ops.bias_act(x, d["bias"].cuda() if c.bias else None, c.act, out=y)
            res = y.cpu()
        elif c.op == "swiglu":
            gb, gu = _view(d["gu"], c.ldgu)
            yb, y = _out(M, D, c.ldy)
            track(gb, M, 2 * D), track(yb, M, D)
            ops.swiglu(gu, out=y)
            res = y.cpu()
        elif c.op == "mask_rows":
            xb, x = _view(d["x"], c.ldx)
            track(xb, M, D)
            res = ops.mask_rows(x, d["keep"].cuda()).cpu()
        else:
            tb, table = _view(d["table"], c.ldt)
            track(tb, d["table"].shape[0], D)
            res = ops.gather_rows_f32(table, d["idx"].cuda()).cpu()
    else:
        img, lut = d["img"].cuda(), d["lut"].cuda()
        if c.op == "normalize":
            res = ops.normalize_u8(img, lut).cpu()
        else:
            S = (c.H // 14) * (c.W // 14)
            ob, o = _out(S, 1176, c.ld)
            track(ob, S, 1176)
            ops.patchify_u8(img, lut, out=o)
            res = o.cpu()
    torch.cuda.synchronize()
    return res, [(buf.cpu(), M, D) for buf, M, D in frames]


def _check(c):
    got, frames = _launch(c)
    ref, bnd = C.reference(c), C.bound(c)
    assert got.shape == ref.shape, f"{c.name}: shape {tuple(got.shape)} for {tuple(ref.shape)}"
    if bnd is None:
        diff = _bits(got) != _bits(ref)
        assert not diff.any(), f"{c.name}: {int(diff.sum())} elements differ from the exact result, first at flat index {int(diff.flatten().float().argmax())}: " \
                               f"got {got.flatten()[:8].tolist()}, want {ref.flatten()[:8].tolist()}"
        w = 0.0
    else:
        assert not torch.isnan(got.float()).any(), f"{c.name}: NaN in the output"
        w, at = C.worst_ratio(got, ref, bnd)
        print(f"\nCASE {c.name}: worst {w:.3f} of the bound")
        assert w <= 1.0, f"{c.name}: {w:.3g} x the bound at flat index {at}: got {got.flatten()[at].item():.8g}, ref {ref.flatten()[at].item():.8g}, " \
                         f"bound {bnd.flatten()[at].item():.3g}"
    for buf, M, D in frames:
        assert C.canary_intact(buf, M, D), f"{c.name}: the canary around a {M} x {D} region changed"
    again, _ = _launch(c)
    assert torch.equal(_bits(again), _bits(got)), f"{c.name}: a second launch gives other bits"
    key = C.route_label(c)
    prev = WORST.get(key)
    WORST[key] = None if bnd is None and prev is None else max(prev or 0.0, w)


def _cases(family):
    return pytest.mark.parametrize("case", C.CASES[family], ids=[c.name for c in C.CASES[family]])


@_cases("rownorm")
def test_rownorm(case):
    _check(case)


@_cases("groupnorm")
def test_groupnorm_tokens(case):
    _check(case)


@_cases("swin")
def test_swin_window_movers(case):
    _check(case)


@_cases("patch_merge")
def test_patch_merge(case):
    _check(case)


@_cases("sine_embed")
def test_sine_embed(case):
    _check(case)


@_cases("box_refine")
def test_box_refine(case):
    _check(case)


@_cases("topk")
def test_topk_desc(case):
    _check(case)


@_cases("argmax")
def test_argmax(case):
    _check(case)


@_cases("eltwise")
def test_elementwise(case):
    _check(case)


@_cases("preprocess")
def test_preprocess(case):
    _check(case)


def test_zz_summary():
    assert WORST, "run the whole file: the summary reports what the sweep measured"
    for key in sorted(WORST):
        print(f"\nSUMMARY {key}: worst {'exact' if WORST[key] is None else format(WORST[key], '.3f')}", end="")
    print(f"\nSUMMARY wall time {time.time() - T0:.1f} s for {len(C.ALL_CASES)} cases")
