"""The UPN post-process on the device (csrc/upn_post.hip) against its numpy definition (tests/upn_post_cases.py), and UPNWrapper.propose
against filter(inference(...)).

Entry level: the score (a sigmoid through expf) has a tolerance, everything after it is exact — so each case first reads the DEVICE's own
scores (a launch with no threshold and no NMS returns every query in order), checks them against fp64 to 2^-21 relative (4 ulp: expf
within 1 ulp, one rounded add, one correctly rounded divide, < 2 ulp in total, doubled) and then holds order, candidates, kept indices,
fp32 boxes, int32 boxes, scores and n_keep to the definition evaluated on those scores, bit for bit.  The outputs sit in one buffer
with guard words around each, prefilled with a sentinel, so a write past n_keep, cap or a buffer shows."""
import numpy as np
import pytest
import torch

import upn_post_cases as P

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
GUARD = 16
CASES = P.all_cases()


def _params(H, W, min_score, iou, max_keep):
    from vlm_fo1_amd import ops
    return ops.upn_post_params([(H, W)], min_score, iou, max_keep, "cuda")


def launch(case, min_score=None, iou=None, max_keep=None, cap=None):
    """One fo1_upn_post_f32 launch on the case's inputs (rows padded to its strides with +inf) -> dict of host arrays (whole buffers)."""
    from vlm_fo1_amd import lib as L
    Q = len(case["logits"])
    cap = case["cap"] if cap is None else cap
    ldb, ldl = case["ld_boxes"], case["ld_logits"]
    boxes = torch.full((Q, ldb), float("inf"), dtype=torch.float32)
    boxes[:, :4] = torch.from_numpy(case["boxes"])
    logits = torch.full((Q, ldl), float("inf"), dtype=torch.float32)
    logits[:, 0] = torch.from_numpy(case["logits"])
    boxes, logits = boxes.cuda(), logits.cuda()
    prm = _params(case["H"], case["W"], case["min_score"] if min_score is None else min_score, case["iou"] if iou is None else iou,
                  case["max_keep"] if max_keep is None else max_keep)
    sizes = dict(n_keep=1, keep_idx=cap, boxes_f32=4 * cap, boxes_i32=4 * cap, scores=cap)
    total = GUARD + sum(n + GUARD for n in sizes.values())
    buf = torch.full((total,), SENT, dtype=torch.int32, device="cuda")
    at, off = {}, GUARD
    for k, n in sizes.items():
        at[k] = (off, n)
        off += n + GUARD
    ptr = {k: buf.data_ptr() + 4 * o for k, (o, n) in at.items()}
    lib = L.load()
    rc = lib.fo1_upn_post_f32(boxes.data_ptr(), ldb, logits.data_ptr(), ldl, Q, prm.data_ptr(), ptr["n_keep"], ptr["keep_idx"], ptr["boxes_f32"],
                              ptr["boxes_i32"], ptr["scores"], cap, None, lib.fo1_upn_post_workspace_bytes(Q), L.current_stream_ptr())
    assert rc == 0, lib.fo1_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    covered = np.zeros(total, dtype=bool)
    out = {}
    for k, (o, n) in at.items():
        out[k] = host[o:o + n].copy()
        covered[o:o + n] = True
    assert np.all(host[~covered] == SENT), "a guard word was written"
    return out


def check_against(out, ref, cap):
    n = ref["n_keep"]
    assert int(out["n_keep"][0]) == n
    assert np.array_equal(out["keep_idx"][:n], ref["keep_idx"])
    assert np.array_equal(out["boxes_f32"].reshape(cap, 4)[:n], ref["boxes_f32"].view(np.int32))             # bit for bit
    assert np.array_equal(out["boxes_i32"].reshape(cap, 4)[:n], ref["boxes_i32"])
    assert np.array_equal(out["scores"][:n], ref["scores"].view(np.int32))
    for k in ("keep_idx", "scores"):
        assert np.all(out[k][n:] == SENT), f"{k} written past n_keep"
    for k in ("boxes_f32", "boxes_i32"):
        assert np.all(out[k][4 * n:] == SENT), f"{k} written past n_keep"


def device_scores(case):
    """Every query's score as the device computes it, and the order the device puts them in."""
    Q = len(case["logits"])
    out = launch(case, min_score=float("-inf"), iou=0.0, max_keep=Q, cap=Q)
    assert int(out["n_keep"][0]) == Q
    order = out["keep_idx"]
    assert sorted(order.tolist()) == list(range(Q))
    sc = np.empty(Q, dtype=np.float32)
    sc[order] = out["scores"].view(np.float32)
    return sc, order


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_entry_equals_the_definition(case):
    Q = len(case["logits"])
    sc, order = device_scores(case)
    s64 = 1.0 / (1.0 + np.exp(-case["logits"].astype(np.float64)))
    rel = np.abs(sc.astype(np.float64) - s64) / s64
    print(f"{case['name']}: max relative score error {rel.max():.3g} (bound {P.ULP4:.3g})")
    assert np.all(rel <= P.ULP4)
    ref = P.upn_post_ref(case["boxes"], case["logits"], case["H"], case["W"], case["min_score"], case["iou"], case["max_keep"], scores=sc, cap=case["cap"])
    assert np.array_equal(order, ref["order"])                                                           # order
    cand = launch(case, iou=0.0, max_keep=Q, cap=Q)                                                       # candidates: threshold, no NMS, no cut
    assert int(cand["n_keep"][0]) == ref["n_cand"] and np.array_equal(cand["keep_idx"][:ref["n_cand"]], ref["order"][:ref["n_cand"]])
    check_against(launch(case), ref, case["cap"])                                                          # the case as stated
    if ref["n_cand"] == 0:
        assert int(launch(case)["n_keep"][0]) == 0


def test_greedy_chain_and_threshold_steps_known_answers():
    cases = {c["name"]: c for c in CASES}
    assert launch(cases["chain"])["keep_idx"][:2].tolist() == [0, 2] and int(launch(cases["chain"])["n_keep"][0]) == 2
    for name, want in (("iou_equals_threshold", [0, 1]), ("iou_one_step_above_threshold", [0]), ("iou_one_step_below_threshold", [0, 1]),
                       ("empty_boxes", [0, 1, 2, 3, 4]), ("identical_boxes", [0, 5])):
        out = launch(cases[name])
        assert out["keep_idx"][:int(out["n_keep"][0])].tolist() == want, name
    out = launch(cases["negative_coordinates"])
    f, i = out["boxes_f32"].view(np.float32)[:16], out["boxes_i32"][:16]
    assert int(out["n_keep"][0]) == 4 and (f < 0).any() and np.array_equal(i, np.trunc(f).astype(np.int32))


def test_same_image_at_grid_index_0_and_3_gives_the_same_bytes():
    from vlm_fo1_amd import ops
    from vlm_fo1_amd.fixtures.upn_proposals import clustered_proposals
    a, la = clustered_proposals(900, 60, seed=31)
    b, lb = clustered_proposals(900, 0, seed=32)
    boxes = torch.from_numpy(np.stack([a, b, b[::-1].copy(), a])).cuda()
    logits = torch.from_numpy(np.stack([la, lb, lb[::-1].copy(), la])).cuda()
    sizes = [(480, 640), (399, 500), (1080, 1920), (480, 640)]
    cap = 300
    prm = ops.upn_post_params(sizes, 0.3, 0.7, 250, "cuda")
    prm[1, 2:4] = torch.tensor([0.1, 0.5]).view(torch.int32)                         # image 1: its own thresholds
    blk = torch.full((4, 1 + 10 * cap), SENT, dtype=torch.int32, device="cuda")
    r = ops.upn_post(boxes, logits, prm, cap=cap, out=blk)
    torch.cuda.synchronize()
    host = blk.cpu()
    assert torch.equal(host[0], host[3]) and not torch.equal(host[0], host[1]) and 0 < int(r.n_keep[0]) <= 250
    for i in range(4):                                                                # and each image equals its own single launch
        one = torch.full((1, 1 + 10 * cap), SENT, dtype=torch.int32, device="cuda")
        ops.upn_post(boxes[i], logits[i], prm[i:i + 1].contiguous(), cap=cap, out=one)
        assert torch.equal(one.cpu()[0], host[i]), i


def test_capture_and_replay_equals_eager_and_reads_params_on_the_device():
    from vlm_fo1_amd import ops
    from vlm_fo1_amd.fixtures.upn_proposals import clustered_proposals
    b, l = clustered_proposals(900, 60, seed=41)
    boxes, logits = torch.from_numpy(b).cuda(), torch.from_numpy(l).cuda()
    cap = 900
    prm = ops.upn_post_params([(480, 640)], 0.3, 0.8, 900, "cuda")
    eager = torch.full((1, 1 + 10 * cap), SENT, dtype=torch.int32, device="cuda")
    ops.upn_post(boxes, logits, prm, cap=cap, out=eager)
    static = torch.full((1, 1 + 10 * cap), SENT, dtype=torch.int32, device="cuda")
    g, _ = ops.capture_graph(lambda: ops.upn_post(boxes, logits, prm, cap=cap, out=static).block)
    static.fill_(SENT)
    ops.replay_graph(g)
    torch.cuda.synchronize()
    assert torch.equal(static, eager) and 0 < int(eager[0, 0]) < 900
    prm.copy_(ops.upn_post_params([(1080, 1920)], 0.5, 0.5, 40, "cuda"))             # new original size and thresholds: same graph
    eager2 = torch.full((1, 1 + 10 * cap), SENT, dtype=torch.int32, device="cuda")
    ops.upn_post(boxes, logits, prm, cap=cap, out=eager2)
    static.fill_(SENT)
    ops.replay_graph(g)
    torch.cuda.synchronize()
    assert torch.equal(static, eager2) and not torch.equal(eager2, eager) and int(eager2[0, 0]) == 40


def test_argument_errors_return_the_code_and_launch_nothing():
    from vlm_fo1_amd import lib as L
    lib = L.load()
    Q, cap = 64, 64
    boxes = torch.rand(Q, 4, device="cuda")
    logits = torch.randn(Q, device="cuda")
    prm = _params(480, 640, 0.0, 0.5, Q)
    out = torch.full((1 + 10 * cap,), SENT, dtype=torch.int32, device="cuda")
    p = out.data_ptr()
    ptrs = [p, p + 4, p + 4 * (1 + cap), p + 4 * (1 + 5 * cap), p + 4 * (1 + 9 * cap)]

    def call(boxes_ptr=boxes.data_ptr(), Q=Q, cap=cap, params=prm.data_ptr(), nk=ptrs[0]):
        return lib.fo1_upn_post_f32(boxes_ptr, 4, logits.data_ptr(), 1, Q, params, nk, ptrs[1], ptrs[2], ptrs[3], ptrs[4], cap, None, 0, L.current_stream_ptr())

    for kw in (dict(Q=0), dict(Q=1025), dict(cap=0), dict(boxes_ptr=None), dict(params=None), dict(nk=None)):
        assert call(**kw) == -1 and lib.fo1_last_error().startswith(b"upn_post:"), kw
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a rejected call wrote"
    assert call() == 0
    torch.cuda.synchronize()
    assert int(out[0]) > 0


# ---- wrapper level -------------------------------------------------------------------------------------------------------------------
N_QUERIES = 100


@pytest.fixture(scope="module")
def wrapper():
    """A reduced-depth UPN (tests/upn_cases.py) behind the drop-in wrapper.  Its random prompt embeddings give logits up to +-25, where
    fp32 sigmoids saturate to equal scores; scaled by 1/8 (exact in bf16) the scores are spread and distinct."""
    import upn_cases as C
    from detect_tools.upn import UPNWrapper
    state = C.upn_state(n_queries=N_QUERIES)
    for k in ("transformer.fine_grained_prompt.weight", "transformer.coarse_grained_prompt.weight"):
        state[k] = state[k] / 8
    return UPNWrapper(state, "cuda", depths=C.SWIN_DEPTHS_SMALL, heads=C.SWIN_HEADS, window=C.SWIN_WINDOW, n_enc=2, n_dec=2, n_queries=N_QUERIES)


def _image(seed, size):
    from PIL import Image
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (size[1] // 8, size[0] // 8, 3), dtype=np.uint8)
    return Image.fromarray(small, "RGB").resize(size, Image.BICUBIC)


def _raw_outputs(w, images):
    """The detector's raw outputs for the images, on the host (what both paths start from)."""
    xs, sizes = w.construct_input(images)
    out = w._inference(xs, "fine_grained_prompt")
    return out["pred_boxes"].float().cpu().numpy(), out["pred_logits"].float().cpu().numpy()[:, :, 0], sizes


MIN_SCORE, NMS = 0.35, 0.6


def test_propose_equals_filter_of_inference(wrapper):
    """One image, then two images of different original sizes that share one resized shape (640 x 480 and 320 x 240 -> 800 x 1066: one
    graph, two parameter blocks).  The host path takes torch's sigmoid and the device its own, so the comparison is exact inside the
    margin (tests/upn_post_cases.margin_ok, on the raw outputs both paths start from); these seeds are inside it — a seed outside it
    fails here, it is not skipped."""
    for images in ([_image(1, (640, 480))], [_image(2, (640, 480)), _image(3, (320, 240))]):
        boxes, logits, sizes = _raw_outputs(wrapper, images)
        for b, l, (H, W) in zip(boxes, logits, sizes):
            assert P.margin_ok(b, l, H, W, MIN_SCORE, NMS), "seed outside the margin: choose another"
        want = wrapper.filter(wrapper.inference(images), MIN_SCORE, NMS)
        got = wrapper.propose(images, MIN_SCORE, NMS)
        assert got == want and len(got["scores"]) == len(images)
        assert all(0 < len(s) < N_QUERIES for s in got["scores"])
        dev = wrapper.propose_device(images, MIN_SCORE, NMS)
        assert len(dev) == len(images) and all(r.boxes_i32.is_cuda and int(r.n_keep[0]) == len(s) for r, s in zip(dev, got["scores"]))
        for r, bx in zip(dev, got["original_xyxy_boxes"]):
            assert r.boxes_i32[0, :len(bx)].cpu().tolist() == bx


def test_inference_and_filter_are_untouched_by_propose(wrapper):
    images = [_image(2, (640, 480)), _image(3, (320, 240))]
    before = wrapper.inference(images)
    f_before = wrapper.filter(before, MIN_SCORE, NMS)
    wrapper.propose(images, MIN_SCORE, NMS, max_boxes=5)
    wrapper.propose(images, 0.9, 0.0, prompt_type="coarse_grained_prompt")
    after = wrapper.inference(images)
    assert np.array_equal(before["original_xyxy_boxes"].view(np.int32), after["original_xyxy_boxes"].view(np.int32))
    assert torch.equal(before["scores"].view(torch.int32), after["scores"].view(torch.int32))
    assert wrapper.filter(after, MIN_SCORE, NMS) == f_before


def test_max_boxes_cuts_and_an_empty_image_does_not_end_the_batch(wrapper):
    images = [_image(2, (640, 480)), _image(3, (320, 240))]
    full = wrapper.propose(images, MIN_SCORE, NMS)
    cut = wrapper.propose(images, MIN_SCORE, NMS, max_boxes=3)
    assert all(len(b) > 3 for b in full["original_xyxy_boxes"])
    assert cut["original_xyxy_boxes"] == [b[:3] for b in full["original_xyxy_boxes"]] and cut["scores"] == [s[:3] for s in full["scores"]]
    # a threshold between the two images' best scores: the first image is empty, the second is not
    res = wrapper.inference(images)
    top = [float(res["scores"][i, 0, 0]) for i in range(2)]
    if top[0] > top[1]:
        images, top = images[::-1], top[::-1]
    assert top[0] < top[1]
    between = (top[0] + top[1]) / 2
    got = wrapper.propose(images, between, NMS)
    assert got["original_xyxy_boxes"][0] == [] and got["scores"][0] == [] and len(got["original_xyxy_boxes"][1]) >= 1
    assert wrapper.filter(wrapper.inference(images), between, NMS) == {"original_xyxy_boxes": [], "scores": []}      # the host path's early return
    nothing = wrapper.propose(images, 2.0, NMS)
    assert nothing == {"original_xyxy_boxes": [[], []], "scores": [[], []]}
