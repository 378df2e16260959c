"""CPU checks of the UPN device post-process: the numpy definition (tests/upn_post_cases.py) against the wrapper's host path
(UPNWrapper.postprocess + filter) and, where the reference tree is present, against the reference's own methods; the tie rule; the
constructed cases' known answers; the margin rule of the wrapper-level comparison; and the surface (include/fo1.h, exports.map's
library, lib.SIGNATURES, the argument checks, which run before any HIP call, and the Python entry points)."""
import os
import re

import numpy as np
import pytest

import upn_post_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_WRAPPER = "/root/reference/detect_tools/upn/inference_wrapper.py"


def distinct(case, scores=None):
    s = P.sigmoid_f32(case["logits"]) if scores is None else scores
    return len(np.unique(s)) == len(s)


def definition_as_filter(case, **kw):
    r = P.upn_post_ref(case["boxes"], case["logits"], case["H"], case["W"], case["min_score"], case["iou"], case["max_keep"], cap=case["cap"], **kw)
    return r, P.as_filter_output(r)


def host_scores(case):
    import torch
    return torch.from_numpy(case["logits"]).sigmoid().numpy()


def uncut(case):
    """Cases the host path can be asked about: no max_keep / cap cut (filter has none), more than one query (its squeeze breaks on one)."""
    return case["max_keep"] >= len(case["logits"]) and case["cap"] >= len(case["logits"]) and len(case["logits"]) > 1


def test_definition_equals_the_host_path_given_the_hosts_scores():
    """Same sigmoid in (torch's), so everything must be equal: boxes, 2-decimal scores, order — on every uncut case with distinct scores."""
    n = 0
    for case in P.all_cases() + P.wrapper_margin_cases():
        s = host_scores(case)
        if not (uncut(case) and distinct(case, s)):
            continue
        _, got = definition_as_filter(case, scores=s)
        want = P.host_path(case["boxes"], case["logits"], case["H"], case["W"], case["min_score"], case["iou"])
        assert got == (want[0], want[1]), case["name"]
        n += 1
    assert n >= 20


def test_definition_with_its_own_sigmoid_equals_the_host_path_inside_the_margin():
    """numpy's exp and torch's sigmoid may differ in the last bits; inside the margin (no score within 4 ulp of another, of min_score or
    of a rounding boundary) that cannot change the result.  Every seeded case must be inside it: none is left out."""
    for case in P.wrapper_margin_cases():
        assert P.margin_ok(case["boxes"], case["logits"], case["H"], case["W"], case["min_score"], case["iou"]), case["name"]
        s64 = 1.0 / (1.0 + np.exp(-case["logits"].astype(np.float64)))
        for s in (P.sigmoid_f32(case["logits"]), host_scores(case)):
            assert np.all(np.abs(s - s64) <= P.ULP4 * s64)
        r, got = definition_as_filter(case)
        want = P.host_path(case["boxes"], case["logits"], case["H"], case["W"], case["min_score"], case["iou"])
        assert got == (want[0], want[1]) and 0 < r["n_keep"] < r["n_cand"], case["name"]


def test_margin_rule_sees_each_kind_of_near_tie():
    b = P.pixel_boxes([[0, 0, 4, 4], [0, 0, 4, 2], [100, 100, 120, 130]])
    ok = dict(boxes=b, logits=np.asarray([1.0, 0.3, -0.4], dtype=P.F), H=256, W=256, min_score=0.3, iou_threshold=0.8)
    assert P.margin_ok(**ok)
    assert not P.margin_ok(**dict(ok, logits=np.asarray([1.0, 1.0, -0.4], dtype=P.F)))                              # two equal scores
    assert not P.margin_ok(**dict(ok, logits=np.asarray([1.0, np.nextafter(P.F(1.0), P.F(2)), -0.4], dtype=P.F)))    # one step apart
    assert not P.margin_ok(**dict(ok, min_score=float(P.sigmoid_f32([0.3])[0])))                                     # a score at min_score
    assert not P.margin_ok(**dict(ok, iou_threshold=0.5))                                                            # an iou at the threshold
    at_boundary = np.log(0.625 / 0.375)                                                                              # score 0.625: rounds at the third decimal
    assert not P.margin_ok(**dict(ok, logits=np.asarray([1.0, at_boundary, -0.4], dtype=np.float64)))


@pytest.mark.skipif(not os.path.isfile(REFERENCE_WRAPPER), reason="reference tree not present")
def test_definition_equals_the_reference_wrapper():
    """The reference's own UPNWrapper.postprocess / filter, loaded in place as tests/test_upn_host.py does (its torchvision.ops.nms replaced
    by this repository's restatement: torchvision is not installed)."""
    import sys
    import types
    import torch
    from detect_tools.upn import inference_wrapper as mine
    saved = {k: sys.modules.get(k) for k in ("mmengine", "torchvision", "torchvision.ops")}
    try:
        sys.modules["mmengine"] = types.SimpleNamespace(Config=None)
        tv = types.ModuleType("torchvision")
        tv.ops = types.ModuleType("torchvision.ops")
        tv.ops.nms = lambda b, s, t: torch.from_numpy(mine.nms(b.numpy(), s.numpy(), t))
        sys.modules["torchvision"], sys.modules["torchvision.ops"] = tv, tv.ops
        src = open(REFERENCE_WRAPPER).read()
        src = src.replace("import detect_tools.upn.transforms.transform as T", "T = None").replace("from detect_tools.upn import build_architecture", "")
        src = src.replace("from detect_tools.upn.models.module import nested_tensor_from_tensor_list", "")
        ns = {}
        exec(compile(src, "ref_inference_wrapper", "exec"), ns)
        Ref = ns["UPNWrapper"]
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    n = 0
    for case in P.all_cases() + P.wrapper_margin_cases():
        s = host_scores(case)
        if not (uncut(case) and distinct(case, s) and case["iou"] > 0):
            continue
        _, got = definition_as_filter(case, scores=s)
        want = P.host_path(case["boxes"], case["logits"], case["H"], case["W"], case["min_score"], case["iou"], wrapper_cls=Ref)
        assert got == (want[0], want[1]), case["name"]
        n += 1
    assert n >= 18


def test_tie_rule_and_known_answers():
    cases = {c["name"]: c for c in P.all_cases()}
    r, _ = definition_as_filter(cases["all_scores_equal"])
    assert r["order"].tolist() == list(range(200)) and r["keep_idx"].tolist() == sorted(r["keep_idx"].tolist()) and r["n_cand"] == 200
    c = cases["equal_scores_across_64"]
    r, _ = definition_as_filter(c)
    tied = np.flatnonzero(c["logits"] == np.sort(c["logits"])[::-1][64])
    at = [r["order"].tolist().index(i) for i in tied]
    assert len(tied) == 10 and at == list(range(at[0], at[0] + 10)) and at[0] < 64 <= at[-1]          # index order, across sorted position 64
    assert definition_as_filter(cases["chain"])[0]["keep_idx"].tolist() == [0, 2]
    assert definition_as_filter(cases["iou_equals_threshold"])[0]["keep_idx"].tolist() == [0, 1]
    assert definition_as_filter(cases["iou_one_step_above_threshold"])[0]["keep_idx"].tolist() == [0]
    assert definition_as_filter(cases["iou_one_step_below_threshold"])[0]["keep_idx"].tolist() == [0, 1]
    assert np.array_equal(P.decode_f32(cases["iou_equals_threshold"]["boxes"], 256, 256), np.asarray([[0, 0, 4, 4], [0, 0, 4, 2]], dtype=P.F))
    assert P.iou_row_f32(np.asarray([[0, 0, 4, 4], [0, 0, 4, 2]], dtype=P.F), 0)[1] == P.F(0.5)
    r = definition_as_filter(cases["empty_boxes"])[0]
    assert r["keep_idx"].tolist() == [0, 1, 2, 3, 4]                                                   # NaN and zero ious drop nothing
    assert definition_as_filter(cases["identical_boxes"])[0]["keep_idx"].tolist() == [0, 5]
    r = definition_as_filter(cases["threshold_above_every_score"])[0]
    assert r["n_cand"] == 0 and r["n_keep"] == 0
    assert definition_as_filter(cases["threshold_below_every_score"])[0]["n_cand"] == 200
    for name in ("no_nms_zero", "no_nms_negative"):
        r = definition_as_filter(cases[name])[0]
        assert r["n_keep"] == r["n_cand"] > 0 and r["keep_idx"].tolist() == r["order"][:r["n_cand"]].tolist()
    full = definition_as_filter(dict(cases["max_keep_1"], max_keep=200))[0]
    assert full["n_keep"] > 17
    for name, n in (("max_keep_1", 1), ("max_keep_between", 17), ("max_keep_Q_cap_binds", 9)):
        r = definition_as_filter(cases[name])[0]
        assert r["n_keep"] == n and r["keep_idx"].tolist() == full["keep_idx"][:n].tolist()
    r = definition_as_filter(cases["negative_coordinates"])[0]
    f, i = r["boxes_f32"], r["boxes_i32"]
    assert (f < 0).any() and np.array_equal(i, np.trunc(f).astype(np.int32)) and not np.array_equal(i, np.floor(f).astype(np.int32))
    assert [c["name"] for c in P.size_cases()] == [f"Q{q}" for q in P.Q_SIZES]
    for c in P.size_cases():
        r = definition_as_filter(c)[0]
        assert r["n_keep"] <= r["n_cand"] <= len(c["logits"]) and (len(c["logits"]) < 63 or 0 < r["n_keep"] < r["n_cand"])


def test_surface():
    from vlm_fo1_amd import lib as L
    names = ("fo1_upn_post_workspace_bytes", "fo1_upn_post_f32", "fo1_upn_post_batch_f32")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fo1.h")).read(), flags=re.S)
    exports = open(os.path.join(ROOT, "vlm_fo1_amd", "csrc", "exports.map")).read()
    assert "global: fo1_*;" in exports
    lib = L.load()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert "fo1_upn_post_params_t" in header and lib.fo1_abi_version() == 9
    assert len(L.SIGNATURES["fo1_upn_post_f32"][1]) == 15 and len(L.SIGNATURES["fo1_upn_post_batch_f32"][1]) == 19
    from detect_tools.upn.inference_wrapper import UPNWrapper
    from vlm_fo1_amd import ops
    from vlm_fo1_amd.upn import UPNEngine
    assert callable(ops.upn_post) and callable(UPNEngine.propose) and callable(UPNWrapper.propose) and callable(UPNWrapper.propose_device)
    assert "early" in UPNWrapper.propose.__doc__ and "empty" in UPNWrapper.propose.__doc__


def test_argument_errors_are_rejected_before_any_hip_call():
    """Fake 4096-aligned integers stand for device pointers; nothing is launched (there is no device here)."""
    from vlm_fo1_amd import lib as L
    lib = L.load()
    BX, LG, PR, NK, KI, BF, BI, SC = [4096 * (i + 1) for i in range(8)]
    need = lib.fo1_upn_post_workspace_bytes(900)
    assert need == lib.fo1_upn_post_workspace_bytes(1024) == 0          # the kernel keeps its state in LDS

    def one(**k):
        a = dict(boxes=BX, ldb=4, logits=LG, ldl=1, Q=900, params=PR, nk=NK, ki=KI, bf=BF, bi=BI, sc=SC, cap=900)
        a.update(k)
        return lib.fo1_upn_post_f32(a["boxes"], a["ldb"], a["logits"], a["ldl"], a["Q"], a["params"], a["nk"], a["ki"], a["bf"], a["bi"], a["sc"], a["cap"],
                                    None, 0, None)

    def batch(**k):
        a = dict(boxes=BX, ldb=4, logits=LG, ldl=1, Q=900, n=4, params=PR, nk=NK, cap=100, stride=1001)
        a.update(k)
        return lib.fo1_upn_post_batch_f32(a["boxes"], a["ldb"], 3600, a["logits"], a["ldl"], 900, a["Q"], a["n"], a["params"], a["nk"], KI, BF, BI, SC, a["cap"],
                                          a["stride"], None, 0, None)

    for call in (one, batch):
        for kw, word in ((dict(Q=0), b"Q=0"), (dict(Q=1025), b"Q=1025"), (dict(Q=-3), b"Q=-3"), (dict(cap=0), b"cap=0"), (dict(boxes=None), b"null"),
                         (dict(logits=None), b"null"), (dict(params=None), b"null"), (dict(nk=None), b"null"), (dict(ldb=3), b"strides"),
                         (dict(ldl=0), b"strides")):
            assert call(**kw) == -1, kw
            msg = lib.fo1_last_error()
            assert msg.startswith(b"upn_post:") and word in msg, msg
    for kw in (dict(ki=None), dict(bf=None), dict(bi=None), dict(sc=None)):
        assert one(**kw) == -1 and b"null" in lib.fo1_last_error()
    assert batch(n=0) == -1 and b"n_images=0" in lib.fo1_last_error()
    assert batch(stride=1000) == -1 and b"out_stride" in lib.fo1_last_error()
