"""UPN deformable-transformer stages on the GPU (vlm_fo1_amd/upn.py over msda.hip / gemm.hip) against goldens made by the
reference's own modules (tests/golden/make_upn_golden.py) and the CPU oracle; bf16 engine vs fp32 reference."""
import os

import numpy as np
import pytest
import torch

import upn_cases as C

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "upn_ref.npz"))


def stats(got, ref):
    got, ref = got.float().cpu().reshape(-1, got.shape[-1]), ref.float().reshape(-1, ref.shape[-1])
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    return cos.min().item(), (got - ref).abs().max().item() / ref.abs().max().item()


def test_msda_fused_matches_unfused_operator_and_oracle():
    """fo1_msda_fused_bf16 (softmax + sampling locations + gather from raw Linear outputs) against (a) the plain operator fed with
    torch-built locations / weights and (b) the fp32 oracle module, 2-d reference points (encoder) and 4-d reference boxes (decoder)."""
    from oracle import msda_oracle as MO
    from vlm_fo1_amd import ops
    M, L, P, D = C.N_HEADS, C.N_LEVELS, C.N_POINTS, 32
    shapes = C.ENC_SHAPES
    S = sum(h * w for h, w in shapes)
    g = torch.Generator().manual_seed(5)
    sh = torch.tensor(shapes).cuda()
    ls = torch.tensor(C.level_start(shapes)).cuda()
    for rd, Lq in ((2, S), (4, 90)):
        value = (torch.randn(1, S, M * D, generator=g)).bfloat16()
        off = torch.randn(1, Lq, M, L, P, 2, generator=g) * 2.0
        logit = torch.randn(1, Lq, M, L * P, generator=g)
        ref = torch.rand(1, Lq, L, rd, generator=g) * (0.4 if rd == 4 else 1.0) + (0.2 if rd == 4 else 0.0)
        ol = torch.cat([off.reshape(1, Lq, -1), logit.reshape(1, Lq, -1)], -1).contiguous()
        got = ops.msda_fused(value.cuda(), sh, ls, ol.cuda(), ref.cuda(), M, P).float().cpu()
        aw = torch.softmax(logit, -1).view(1, Lq, M, L, P)
        shf = torch.tensor(shapes, dtype=torch.float32)
        if rd == 2:
            loc = ref[:, :, None, :, None, :] + off / torch.stack([shf[:, 1], shf[:, 0]], -1)[None, None, None, :, None, :]
        else:
            loc = ref[:, :, None, :, None, :2] + off / P * ref[:, :, None, :, None, 2:] * 0.5
        want = MO.ms_deform_attn_forward(value.float().view(1, S, M, D), shapes, C.level_start(shapes), loc.contiguous(), aw.contiguous())
        err = (got - want).abs()
        assert (err <= 2.0 ** -8 * want.abs() + 2e-3).all(), f"ref_dim {rd}: max err {err.max():.4g}"
        plain = ops.ms_deform_attn(value.cuda().view(1, S, M, D), sh, ls, loc.contiguous().cuda(), aw.contiguous().cuda()).float().cpu()
        assert (got - plain).abs().max().item() <= 2e-2 * want.abs().max().item()


def test_deformable_encoder_matches_reference_modules():
    from vlm_fo1_amd.upn import DeformableEncoder
    state = C.encoder_state(2)
    src, pos = C.encoder_inputs()
    enc = DeformableEncoder(state, "", 2, "cuda")
    outs = []
    mem = enc.forward(src[0].bfloat16().cuda(), pos[0].bfloat16().cuda(), C.ENC_SHAPES, collect=outs)
    for got, key in ((outs[0], "enc.layer0"), (mem, "enc.memory")):
        cos, rel = stats(got, torch.from_numpy(G[key])[0])
        assert cos >= 0.9995 and rel <= 2.0 ** -5, f"{key}: min cos {cos:.6f}, rel {rel:.4g}"
    again = enc.forward(src[0].bfloat16().cuda(), pos[0].bfloat16().cuda(), C.ENC_SHAPES)
    assert torch.equal(again, mem), "two runs of the encoder differ"


def test_deformable_encoder_full_size_runs_and_is_finite():
    """UPN's real geometry: 800 x 1333 input -> 5 levels (22 300 tokens), 6 layers; timing printed for the record."""
    import time
    from vlm_fo1_amd.upn import DeformableEncoder
    shapes = [(100, 167), (50, 84), (25, 42), (13, 21), (7, 11)]
    S = sum(h * w for h, w in shapes)
    enc = DeformableEncoder(C.encoder_state(6, seed=9), "", 6, "cuda")
    g = torch.Generator().manual_seed(3)
    src = torch.randn(S, 256, generator=g).bfloat16().cuda()
    pos = (torch.randn(S, 256, generator=g) * 0.5).bfloat16().cuda()
    out = enc.forward(src, pos, shapes)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(5):
        out = enc.forward(src, pos, shapes)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) / 5 * 1e3
    print(f"\nUPN deformable encoder, 6 layers x {S} tokens: {ms:.2f} ms (eager launches)")
    assert torch.isfinite(out.float()).all() and out.shape == (S, 256)


def test_topk_kernel_matches_torch_topk():
    from vlm_fo1_amd import ops
    g = torch.Generator().manual_seed(8)
    for n, k, stride in ((257, 30, 1), (22300, 900, 8), (1000, 1000, 1), (5, 3, 2)):
        x = torch.randn(n * stride, generator=g)
        x[::max(1, n // 7) * stride] = float("inf")                    # invalid proposals carry +inf coordinates; scores may repeat
        got_i, got_v = ops.topk_desc(x.cuda(), k, stride=stride, n=n)
        want_v, want_i = torch.topk(x[::stride][:n], k)
        assert torch.equal(got_v.cpu(), want_v), (n, k)
        sel = x[::stride][got_i.cpu().long()]
        assert torch.equal(sel, want_v)                                # same values in the same order
        want_i = torch.sort(-x[::stride][:n].double(), stable=True).indices[:k]
        assert torch.equal(got_i.cpu().long(), want_i), (n, k)         # ties: lower index first, exactly (the kernel's contract; torch.topk leaves it open)


def test_query_selection_matches_reference_model():
    from vlm_fo1_amd.upn import QuerySelector
    state = C.transformer_state(2, 2, C.N_QUERIES_SMALL)
    memory = torch.from_numpy(G["tr.memory"])[0]
    sel = QuerySelector(state, "cuda", C.N_QUERIES_SMALL).forward(memory.bfloat16().cuda(), C.ENC_SHAPES)
    ref_scores = torch.from_numpy(G["tr.sel.scores"])[0]
    scores = sel["scores"][:, 0].cpu()
    assert (scores - ref_scores).abs().max().item() <= 0.02 * ref_scores.abs().max().item() + 0.05
    gc, coords = torch.from_numpy(G["tr.sel.coords"])[0], sel["coords"].cpu()
    fin = torch.isfinite(gc)
    assert torch.equal(fin, torch.isfinite(coords)) and (coords[fin] - gc[fin]).abs().max().item() <= 0.03
    # the selected set: identical up to swaps among tokens whose reference scores are closer than the bf16 noise
    want = torch.topk(ref_scores, C.N_QUERIES_SMALL)[1]
    got = sel["idx"].cpu().long()
    kth = ref_scores[want[-1]]
    for t in set(got.tolist()) ^ set(want.tolist()):
        assert abs(ref_scores[t] - kth) <= 0.1, f"token {t} selected / dropped with a clear margin"
    assert len(set(got.tolist()) & set(want.tolist())) >= C.N_QUERIES_SMALL - 3


def test_decoder_and_heads_match_reference_model():
    """Teacher-forced on the reference's selected reference boxes: hidden states per layer, refined boxes, final boxes and logits."""
    from vlm_fo1_amd.upn import DeformableDecoder
    state = C.transformer_state(2, 2, C.N_QUERIES_SMALL)
    memory = torch.from_numpy(G["tr.memory"])[0].bfloat16().cuda()
    dec = DeformableDecoder(state, 2, "cuda", C.N_QUERIES_SMALL)
    out = dec.forward(memory, C.ENC_SHAPES, torch.from_numpy(G["tr.sel.refpoints"])[0].cuda())
    for i in range(2):
        cos, rel = stats(out["hs"][i], torch.from_numpy(G["tr.hs"])[i, 0])
        assert cos >= 0.999 and rel <= 2.0 ** -4, f"hs[{i}]: min cos {cos:.6f}, rel {rel:.4g}"
    for i in range(3):
        assert (out["refs"][i].cpu() - torch.from_numpy(G["tr.refs"])[i, 0]).abs().max().item() <= 0.01, f"reference boxes after layer {i}"
    assert (out["pred_boxes"].cpu() - torch.from_numpy(G["tr.pred_boxes"])[0]).abs().max().item() <= 0.01
    lg = torch.from_numpy(G["tr.pred_logits"])[0, :, 0]
    assert (out["pred_logits"].cpu() - lg).abs().max().item() <= 0.02 * lg.abs().max().item() + 0.1


def test_swin_backbone_and_input_projection_match_reference_model():
    from vlm_fo1_amd.upn import InputProjection, SwinBackbone
    state = C.upn_state()
    bb = SwinBackbone(state, C.SWIN_DEPTHS_SMALL, C.SWIN_HEADS, C.SWIN_WINDOW, "cuda")
    feats, sizes = bb.forward(C.test_image().cuda())
    assert sizes == [(25, 34), (13, 17), (7, 9), (4, 5)]
    for l, f in enumerate(feats):
        cos, rel = stats(f, torch.from_numpy(G[f"full.swin{l}"]).float())
        assert cos >= 0.999 and rel <= 2.0 ** -4, f"swin stage {l}: min cos {cos:.6f}, rel {rel:.4g}"
    src, pos, shapes = InputProjection(state, "cuda").forward(feats, sizes)
    assert [list(s) for s in shapes] == G["full.shapes"].tolist()
    cos, rel = stats(src, torch.from_numpy(G["full.src"]).float())
    assert cos >= 0.999 and rel <= 2.0 ** -4, f"input_proj: min cos {cos:.6f}, rel {rel:.4g}"
    assert (pos.float().cpu() - torch.from_numpy(G["full.pos"]).float()).abs().max().item() <= 0.03


def test_whole_detector_boxes_match_reference_model():
    """Image in, boxes out (Swin-L widths at depths [2, 2, 2, 2], 2 + 2 transformer layers, 30 queries).  The i-th ranked proposal is
    decoded with the i-th learned query (deformable_transformer.py:319-331), so a swap of two near-tied scores legitimately changes
    two boxes; the comparison is therefore rank-aware: wherever the engine ranks the same token at the same place as the fp32
    oracle, its box must match the reference model's (<= 0.02 in normalised cx, cy, w, h) and its score must agree; and with the
    decoder teacher-forced on the oracle's ranked proposals over the ENGINE's own memory, every box must match."""
    from oracle import upn_oracle as O
    from vlm_fo1_amd.upn import UPNEngine
    state = C.upn_state()
    eng = UPNEngine(state, "cuda", C.SWIN_DEPTHS_SMALL, C.SWIN_HEADS, C.SWIN_WINDOW, 2, 2, C.N_QUERIES_SMALL)
    out = eng.forward(C.test_image().cuda())
    boxes, logits = out["pred_boxes"].cpu(), out["pred_logits"].cpu()
    rb, rl = torch.from_numpy(G["full.pred_boxes"]), torch.from_numpy(G["full.pred_logits"])
    assert boxes.shape == rb.shape and torch.isfinite(boxes).all() and (boxes >= 0).all() and (boxes <= 1).all()
    # the oracle's ranked selection (fp32, CPU) on its own memory
    feats, sizes = O.swin_forward(state, C.test_image(), C.SWIN_DEPTHS_SMALL, C.SWIN_HEADS, C.SWIN_WINDOW)
    src, pos, shapes = O.backbone_encoder_inputs(state, feats, sizes)
    enc_state = {k[len("transformer.encoder."):]: v for k, v in state.items() if k.startswith("transformer.encoder.")}
    memory = O.encoder(enc_state, src[None], pos[None], shapes, 2)[0]
    cos, rel = stats(out["memory"], memory)
    assert cos >= 0.998 and rel <= 2.0 ** -4, f"encoder memory: min cos {cos:.6f}, rel {rel:.4g}"
    _, _, ref_idx, ref_pts = O.query_selection(state, memory, shapes, C.N_QUERIES_SMALL)
    got_idx = out["selection"]["idx"].cpu().long()
    same = got_idx == ref_idx
    assert same.float().mean().item() >= 0.5 and len(set(got_idx.tolist()) & set(ref_idx.tolist())) >= C.N_QUERIES_SMALL - 4
    assert (boxes[same] - rb[same]).abs().max().item() <= 0.02, f"same-rank boxes: {(boxes[same] - rb[same]).abs().max(-1)[0]}"
    # scores: a 256-term dot product of the (unit-variance) decoder state with the N(0, 1) test prompt, |logit| up to 25 here: the
    # accumulated bf16 noise of backbone + encoder + decoder (hidden states at cos >= 0.998) shows as up to ~8 % of that range
    assert (logits[same] - rl[same]).abs().max().item() <= 0.12 * rl.abs().max().item()
    forced = eng.decoder.forward(out["memory"], shapes, ref_pts.cuda())
    assert (forced["pred_boxes"].cpu() - rb).abs().max().item() <= 0.02, "teacher-forced decoder over the engine's memory"
    again = eng.forward(C.test_image().cuda())
    assert torch.equal(again["pred_boxes"], out["pred_boxes"])


def test_upn_wrapper_contract_and_full_size_model():
    """The drop-in UPNWrapper at the reference's real configuration (configs/upn_large.py: Swin-L depths [2, 2, 18, 2], 6 + 6 layers, 900
    queries) on an 800-short-side image: inference() returns what the reference's does (boxes [1, 900, 4] in original pixels sorted by
    score, scores [1, 900, 1] in [0, 1]), filter() thresholds + NMS; timing printed for the record (random weights: no accuracy claim)."""
    import time
    from PIL import Image
    from detect_tools.upn import UPNWrapper
    state = C.upn_state(depths=[2, 2, 18, 2], n_enc=6, n_dec=6, n_queries=900)
    w = UPNWrapper(state, "cuda")
    rng = np.random.default_rng(5)
    img = Image.fromarray(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8), "RGB")
    res = w.inference([img], "fine_grained_prompt")
    assert res["original_xyxy_boxes"].shape == (1, 900, 4) and tuple(res["scores"].shape) == (1, 900, 1)
    sc = res["scores"][0, :, 0]
    assert torch.isfinite(sc).all() and (sc[:-1] >= sc[1:]).all() and 0 <= float(sc.min()) and float(sc.max()) <= 1
    assert np.isfinite(res["original_xyxy_boxes"]).all()
    flt = w.filter(res, min_score=float(sc[100]), nms_value=0.8)
    assert len(flt["original_xyxy_boxes"]) == 1 and 1 <= len(flt["original_xyxy_boxes"][0]) <= 101
    assert all(len(b) == 4 and all(isinstance(v, int) for v in b) for b in flt["original_xyxy_boxes"][0])
    assert flt["scores"][0] == sorted(flt["scores"][0], reverse=True)
    x = w.transform_image(img)
    assert tuple(x.shape) == (3, 800, 1066)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(3):
        w.model.forward(x)
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t) / 3 * 1e3
    ref = w.model.forward(x)
    ref = (ref["pred_boxes"].clone(), ref["pred_logits"].clone())
    for _ in range(3):                                     # sighting, capture, replay
        got = w.model.forward_graph(x)
    assert torch.equal(got["pred_boxes"], ref[0]) and torch.equal(got["pred_logits"], ref[1]), "graph replay != eager"
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(5):
        w.model.forward_graph(x)
    torch.cuda.synchronize()
    graph_ms = (time.perf_counter() - t) / 5 * 1e3
    print(f"\nUPN (Swin-L 2-2-18-2 + 6/6 deformable layers, 900 queries) on 800 x 1066: {eager_ms:.1f} ms per image eager, "
          f"{graph_ms:.1f} ms as one hipGraph replay")
    res2 = w.inference([img], "fine_grained_prompt")       # (second sighting of this size: captured; third: replayed)
    res3 = w.inference([img], "fine_grained_prompt")
    assert np.array_equal(res2["original_xyxy_boxes"], res["original_xyxy_boxes"]) and np.array_equal(res3["original_xyxy_boxes"], res["original_xyxy_boxes"])


def test_full_size_detector_parity_vs_oracle():
    """VERDICT r2 missing #6: parity (not just "runs, finite") at the reference's real configuration — Swin-L depths [2, 2, 18, 2],
    6 encoder + 6 decoder layers, 900 queries (detect_tools/upn/configs/upn_large.py) on an 800 x 1066 image — against the fp32 CPU
    oracle (oracle/upn_oracle.py, pinned to the reference's own UPN classes at reduced depth by tests/test_oracle_upn.py).  Rank-aware
    like the reduced-depth test: near-tied scores may swap ranks in a bf16 execution, and the i-th ranked proposal is decoded with the
    i-th learned query, so boxes are compared where engine and oracle rank the same token at the same place, and the decoder is
    also teacher-forced on the oracle's ranked proposals over the ENGINE's memory (that comparison covers all 900 boxes).  Metrics are
    printed and written to gpurun_out/upn_fullsize_metrics.json."""
    import json
    import time
    from oracle import upn_oracle as O
    from vlm_fo1_amd.upn import UPNEngine
    torch.set_num_threads(min(32, len(os.sched_getaffinity(0))))
    depths, n_enc, n_dec, nq = [2, 2, 18, 2], 6, 6, 900
    state = C.upn_state(depths=depths, n_enc=n_enc, n_dec=n_dec, n_queries=nq)
    img = C.test_image(hw=(800, 1066), seed=23)
    eng = UPNEngine(state, "cuda", depths, C.SWIN_HEADS, C.SWIN_WINDOW, n_enc, n_dec, nq)
    out = eng.forward(img.cuda())
    boxes, logits = out["pred_boxes"].float().cpu(), out["pred_logits"].float().cpu()
    assert boxes.shape == (nq, 4) and torch.isfinite(boxes).all() and (boxes >= 0).all() and (boxes <= 1).all()
    t0 = time.perf_counter()
    feats, sizes = O.swin_forward(state, img, depths, C.SWIN_HEADS, C.SWIN_WINDOW)
    src, pos, shapes = O.backbone_encoder_inputs(state, feats, sizes)
    enc_state = {k[len("transformer.encoder."):]: v for k, v in state.items() if k.startswith("transformer.encoder.")}
    memory = O.encoder(enc_state, src[None], pos[None], shapes, n_enc)[0]
    _, _, ref_idx, ref_pts = O.query_selection(state, memory, shapes, nq)
    _, _, rb, rl = O.decoder(state, memory, shapes, ref_pts, n_dec)
    rl = rl[:, 0]
    t_oracle = time.perf_counter() - t0
    cos, rel = stats(out["memory"], memory)
    got_idx = out["selection"]["idx"].cpu().long()
    same = got_idx == ref_idx
    overlap = len(set(got_idx.tolist()) & set(ref_idx.tolist())) / nq
    same_box = float((boxes[same] - rb[same]).abs().max()) if same.any() else 0.0
    same_logit = float((logits.reshape(nq, -1)[:, 0][same] - rl[same]).abs().max()) if same.any() else 0.0
    forced = eng.decoder.forward(out["memory"], shapes, ref_pts.cuda())
    fb = (forced["pred_boxes"].float().cpu() - rb).abs().max(-1)[0]
    M = dict(memory_min_cos=cos, memory_rel=rel, selection_overlap=overlap, same_rank_fraction=float(same.float().mean()),
             same_rank_box_max_err=same_box, same_rank_logit_max_err=same_logit, logit_range=float(rl.abs().max()),
             forced_box_err_max=float(fb.max()), forced_box_err_p99=float(fb.kthvalue(int(0.99 * nq))[0]), tokens=int(memory.shape[0]),
             oracle_seconds=round(t_oracle, 1))
    print("\nUPN full size vs oracle:", json.dumps(M))
    os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out"), exist_ok=True)
    json.dump(M, open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "upn_fullsize_metrics.json"), "w"), indent=1)
    # 24 Swin blocks + 6 encoder layers of bf16 rounding in front of the memory (the reduced-depth test has 8 + 2 at cos >= 0.998)
    assert cos >= 0.99 and rel <= 2.0 ** -3, f"encoder memory at full depth: min cos {cos:.5f}, rel {rel:.4g}"
    assert overlap >= 0.85, f"selected token sets overlap only {overlap:.3f}"
    assert same_box <= 0.03, f"same-rank boxes differ by {same_box:.4f}"
    assert M["forced_box_err_p99"] <= 0.03 and M["forced_box_err_max"] <= 0.1, f"teacher-forced decoder boxes: p99 {M['forced_box_err_p99']:.4f}, max {M['forced_box_err_max']:.4f}"
