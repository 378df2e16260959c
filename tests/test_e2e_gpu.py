"""End-to-end GPU parity: the whole hot path (ViT -> FPN, DaViT -> HFRE -> projectors -> splice -> mRoPE ->
LLM prefill -> first token) on the engine vs the composed CPU oracles, true channel widths, reduced depth
(ViT 4 blocks, LLM 2 layers, 4k vocab) so the CPU side finishes in seconds.

north_star tolerance for region tokens ("within a stated bf16 tolerance"): per-token cosine >= 0.999 and
max|delta| <= 2^-4 * max|ref| (they sit behind the full DaViT-L + 4 ViT blocks + FPN, whose intrinsic bf16
noise floor is measured in test_towers_gpu.py); image tokens the same; logits max|delta| <= 0.05 and the
greedy token equal whenever the oracle's top-1 margin exceeds 0.1."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def cpu_state(weights):
    return {k: {n: t.float().cpu() for n, t in sd.items()} for k, sd in weights.items()}


def mlp2(x, sd, prefix):
    h = F.gelu(F.linear(x, sd[prefix + "0.weight"], sd[prefix + "0.bias"]))
    return F.linear(h, sd[prefix + "2.weight"], sd[prefix + "2.bias"])


def test_full_hot_path_vs_oracle():
    from hfre_cases import box_fixtures
    from oracle import davit_oracle as DO, fpn_oracle as FO, hfre_oracle as HO, llm_oracle as LO, vit_oracle as VO
    from vlm_fo1_amd.llm import LLMConfig
    from vlm_fo1_amd.model import FO1Config, FO1Engine, random_weights, synthetic_prompt
    from vlm_fo1_amd.vit import ViTConfig
    cfg = FO1Config(vit=ViTConfig(depth=4, fullatt_block_indexes=(1, 3)), llm=LLMConfig(num_layers=2, vocab_size=4096, max_seq=1024))
    weights = random_weights(cfg, "cuda", seed=3)
    eng = FO1Engine(cfg, weights, "cuda")
    H, W = 399, 500          # the demo image geometry (aux tower: dynamic size, no resize)
    gh, gw = 28, 36
    g = torch.Generator().manual_seed(9)
    pix = torch.randn(gh * gw, 1176, generator=g).bfloat16()
    aux = torch.randn(3, H, W, generator=g).bfloat16()
    it = [x for x in box_fixtures()["countbench"] if len(x["bboxes"]) == 7][0]
    boxes = torch.tensor(it["bboxes"], dtype=torch.float32) * torch.tensor([W / it["extent"][0], H / it["extent"][1]] * 2)
    ids = synthetic_prompt(boxes.shape[0], vocab=4096, seed=1)
    out = eng.prefill(ids, pix.cuda(), (gh, gw), aux.cuda(), boxes.cuda())

    sd = cpu_state(weights)
    tokens, maps = VO.vit_forward(sd["vit"], pix.float(), gh, gw, depth=4, n_heads=16, fullatt=(1, 3))
    img_tok = mlp2(tokens, sd["proj"], "mm_projector.")
    fpn_in = maps[-1].bfloat16().float().reshape(gh, gw, 1280).permute(2, 0, 1).unsqueeze(0)
    fpn = [m.bfloat16() for m in FO.fpn_forward(sd["fpn"], fpn_in)]
    aux_maps, aux_sizes = DO.davit_forward(sd["davit"], aux.float().unsqueeze(0))
    aux_nchw = [m.bfloat16().reshape(h, w, -1).permute(2, 0, 1).unsqueeze(0) for m, (h, w) in zip(aux_maps, aux_sizes)]
    sw, sh = gw * 14 / W, gh * 14 / H
    vtb = boxes * torch.tensor([sw, sh, sw, sh])
    feat = HO.hfre_oracle(aux_nchw, boxes, fpn, vtb, region_dim=5888, grid_hw=(gh, gw), vt_strides=[3.5, 7, 14, 28])[0]
    reg_tok = mlp2(feat.bfloat16().float(), sd["proj"], "mm_projector_aux.")

    def check(got, ref, what, cos_min=0.999, rel_max=2 ** -4):
        got, ref = got.float().cpu(), ref.float()
        cos = F.cosine_similarity(got, ref, dim=-1)
        rel = (got - ref).abs().max() / ref.abs().max()
        assert cos.min() >= cos_min and rel <= rel_max, f"{what}: min cos {cos.min():.6f}, rel {rel:.4g}"

    check(out["image_tokens"], img_tok, "image tokens")
    check(out["region_tokens"], reg_tok, "region tokens")
    emb, nb, na = LO.splice(torch.tensor(ids), sd["llm"]["embed_tokens.weight"], img_tok, reg_tok)
    assert emb.shape == out["embeds"].shape
    pos, delta = LO.rope_index(nb, (gh // 2, gw // 2), na)
    assert torch.equal(pos, out["position_ids"]) and delta == out["rope_delta"]
    final = LO.llm_forward(sd["llm"], emb, pos, n_layers=2, n_heads=16, n_kv=2, head_dim=128, eps=1e-6, theta=1e6,
                           sections=(16, 24, 24))
    check(out["last_hidden"], final[-1:], "final hidden", cos_min=0.999)
    ref_logits = final[-1:] @ sd["llm"]["embed_tokens.weight"].t()
    err = (out["logits"].float().cpu() - ref_logits).abs().max()
    assert err <= 0.05, f"logits max err {err:.4g}"
    top2 = ref_logits[0].topk(2).values
    if top2[0] - top2[1] > 0.1:
        assert int(out["next_token"].item()) == int(ref_logits.argmax())
    # greedy decode runs and is deterministic
    a = eng.generate(ids, pix.cuda(), (gh, gw), aux.cuda(), boxes.cuda(), max_new_tokens=6)
    b = eng.generate(ids, pix.cuda(), (gh, gw), aux.cuda(), boxes.cuda(), max_new_tokens=6)
    assert a == b and len(a) == 6 and a[0] == int(out["next_token"].item())


def test_graph_replay_is_bit_identical_to_eager():
    """The hipGraph path must run the same kernels on the same data: outputs bit-identical to eager,
    also after the static input buffers are refreshed with a different image / boxes / prompt."""
    from vlm_fo1_amd.llm import LLMConfig
    from vlm_fo1_amd.model import FO1Config, FO1Engine, random_weights, synthetic_prompt
    from vlm_fo1_amd.vit import ViTConfig
    cfg = FO1Config(vit=ViTConfig(depth=2, fullatt_block_indexes=(1,)), llm=LLMConfig(num_layers=2, vocab_size=4096, max_seq=1024))
    eng = FO1Engine(cfg, random_weights(cfg, "cuda", seed=5), "cuda")
    gh, gw, H, W = 10, 14, 140, 196
    for trial in range(3):
        g = torch.Generator().manual_seed(100 + trial)
        pix = torch.randn(gh * gw, 1176, generator=g).bfloat16().cuda()
        aux = torch.randn(3, H, W, generator=g).bfloat16().cuda()
        boxes = (torch.rand(5, 4, generator=g) * 60 + torch.tensor([0., 0., 70., 70.])).cuda()
        ids = synthetic_prompt(5, vocab=4096, seed=trial)
        e = eng.prefill(ids, pix, (gh, gw), aux, boxes, use_graph=False)
        e = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in e.items()}
        r = eng.prefill(ids, pix, (gh, gw), aux, boxes, use_graph=True)
        for k in ("image_tokens", "region_tokens", "embeds", "last_hidden", "logits", "next_token"):
            assert torch.equal(e[k], r[k]), f"trial {trial}: {k} differs between eager and graph replay"
    assert len(eng._graphs) == 1, "one signature -> one captured graph"


def test_bench_two_ranks_control_flow(tmp_path):
    """`python bench.py --gpus 2` WITHOUT a launcher (the form the driver uses): bench.py runs itself, as a child process, under
    torch.distributed.run with 2 ranks (both on cuda:0 over gloo — a 1-GPU box cannot host two RCCL ranks): the barrier /
    max-over-ranks / rank-0-prints-one-line contract and hipGraph capture with a live process group."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FO1_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full", "--main-only", "--scale-items", "64"]
    p = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line from rank 0, got {len(lines)}"
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["scaling"] == "weak" and out["value"] > 0
    assert "cpu_baseline" not in out and out["roofline"]["bound"] in ("mfma", "hbm")
    # the `scale` block (round 5): evaluation/eval_coco.py's loop through sharded_eval.run_sharded ACROSS the two ranks — LPT shard, per-rank
    # prefetch + decode pool, ONE all_gather at the reducer — and the merged ids of a sample equal to what one rank computes alone
    sc = out["scale"]
    os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
    json.dump(sc, open(os.path.join(root, "gpurun_out", "scale_block_two_ranks_one_device.json"), "w"), indent=1)
    assert sc["world_size"] == 2 and sc["dist_world_size"] == 2 and sc["backend"] == "gloo" and sc["one_device_gloo_test_mode"] is True
    assert sc["items"] == 128 and sc["per_rank_items"] == [64, 64] and len(sc["per_rank_shard_seconds"]) == 2 and len(sc["gather_ms"]) == 2
    assert sc["images_per_sec"] > 0 and sc["predictions_file_written"] and sc["host_threads_for_this_run"] == 2 * sc["host_threads_per_gpu"]
    assert sc["items_failed"] == 0, sc
    assert sc["sample_ids_equal_to_one_rank_alone"] is True, sc.get("sample_difference")


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """`bench.py --dump-outputs DIR`: what the LAST timed step returned (step 2 of 2: the second engine replica's graph replay), written
    before anything else runs on the engines, equals one eager pass over the same seeded inputs in this process, array for array."""
    import os
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B = 2
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B), "--json-out", "",
           "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    sys.path.insert(0, root)
    import bench
    dev = torch.device("cuda", 0)
    cases = [bench.build_workload(dev, seed=1234 + i) for i in range(B)]
    outs = bench.Pipeline(cases[0], dev, inflight=1, batch=B, cases=cases).step(graph=False)
    torch.cuda.synchronize()
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in bench.DUMP_NAMES), "nothing sampled at this size"
    for name in bench.DUMP_NAMES:
        want = torch.cat([o[name] for o in outs], 0)
        want = (want.double() if name == "next_token" else want.float()).cpu().numpy()
        assert np.array_equal(np.load(tmp_path / f"{name}.npy"), want), name


def test_replicas_in_flight_match_sequential():
    """FO1Engine.replica(): shared weights, private per-request state.  Four engines, four different images, all submitted back
    to back on four streams (graph replays overlapping on the GPU) for many rounds, then from four host threads with greedy
    decoding: every result must be exactly what one engine gives for that image alone.  (Regression: a module-level argmax
    scratch and a per-module DaViT V^T buffer used to be shared between replicas.)"""
    import threading
    from vlm_fo1_amd.llm import LLMConfig
    from vlm_fo1_amd.model import FO1Config, FO1Engine, random_weights, synthetic_prompt
    from vlm_fo1_amd.vit import ViTConfig
    cfg = FO1Config(vit=ViTConfig(depth=2, fullatt_block_indexes=(1,)), llm=LLMConfig(num_layers=2, vocab_size=4096, max_seq=1024))
    eng = FO1Engine(cfg, random_weights(cfg, "cuda", seed=5), "cuda")
    R = 4
    engines = [eng] + [eng.replica() for _ in range(R - 1)]
    assert engines[1].llm.layers[0]["wqkv"].data_ptr() == eng.llm.layers[0]["wqkv"].data_ptr(), "weights must be shared"
    assert engines[1].llm.kcache.data_ptr() != eng.llm.kcache.data_ptr(), "KV cache must be private"
    gh, gw, H, W = 10, 14, 140, 196
    reqs = []
    for trial in range(R):
        g = torch.Generator().manual_seed(300 + trial)
        reqs.append(dict(pix=torch.randn(gh * gw, 1176, generator=g).bfloat16().cuda(), aux=torch.randn(3, H, W, generator=g).bfloat16().cuda(),
                         boxes=(torch.rand(5, 4, generator=g) * 60 + torch.tensor([0., 0., 70., 70.])).cuda(),
                         ids=synthetic_prompt(5, vocab=4096, seed=trial)))
    keys = ("image_tokens", "region_tokens", "last_hidden", "logits", "next_token")
    ref = []
    for r in reqs:   # sequential, one engine
        o = eng.prefill(r["ids"], r["pix"], (gh, gw), r["aux"], r["boxes"], use_graph=True)
        torch.cuda.synchronize()
        ref.append({k: o[k].clone() for k in keys})
        ref[-1]["gen"] = eng.generate(r["ids"], r["pix"], (gh, gw), r["aux"], r["boxes"], max_new_tokens=8, use_graph=True)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(R)]
    for rounds in range(12):   # overlapped: all in flight before any is read
        outs = []
        for e, s, r in zip(engines, streams, reqs):
            with torch.cuda.stream(s):
                outs.append(e.prefill(r["ids"], r["pix"], (gh, gw), r["aux"], r["boxes"], use_graph=True))
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            for k in keys:
                assert torch.equal(o[k], ref[i][k]), f"round {rounds}, request {i}: {k} differs with {R} images in flight"
    # host threads, prefill + decode from each engine's own cache
    for rounds in range(3):
        got = [None] * R

        def work(i):
            with torch.cuda.stream(streams[i]):
                r = reqs[i]
                got[i] = engines[i].generate(r["ids"], r["pix"], (gh, gw), r["aux"], r["boxes"], max_new_tokens=8, use_graph=True)

        th = [threading.Thread(target=work, args=(i,)) for i in range(R)]
        [t.start() for t in th]
        [t.join() for t in th]
        torch.cuda.synchronize()
        assert got == [rf["gen"] for rf in ref], f"threaded round {rounds}: {got} vs {[rf['gen'] for rf in ref]}"


def test_random_geometries_graph_equals_eager_and_finite():
    """Ragged everything: random image sizes (smart-resized to multiples of 28 for the primary tower, raw 'dynamic' size for the aux
    tower), random box counts / boxes incl. degenerate and out-of-image ones.  For every geometry the graph replay must equal the eager
    launches bit for bit, outputs must be finite, and a second request of another geometry must not disturb the first graph."""
    import random
    from vlm_fo1.model.image_processing import smart_resize
    from vlm_fo1_amd.llm import LLMConfig
    from vlm_fo1_amd.model import FO1Config, FO1Engine, random_weights, synthetic_prompt
    from vlm_fo1_amd.vit import ViTConfig
    cfg = FO1Config(vit=ViTConfig(depth=2, fullatt_block_indexes=(1,)), llm=LLMConfig(num_layers=2, vocab_size=4096, max_seq=2048))
    eng = FO1Engine(cfg, random_weights(cfg, "cuda", seed=11), "cuda")
    rnd = random.Random(2024)
    first = None
    for trial in range(7):
        W, H = rnd.choice([(500, 399), (333, 711), (64, 60), (640, 480), (97, 301), (420, 420), (801, 127)]) if trial < 7 else (0, 0)
        rh, rw = smart_resize(H, W, 28, 56 * 56, 2048 * 2048)
        gh, gw = rh // 14, rw // 14
        n = rnd.choice([1, 2, 7, 33, 100])
        g = torch.Generator().manual_seed(500 + trial)
        pix = torch.randn(gh * gw, 1176, generator=g).bfloat16().cuda()
        aux = torch.randn(3, H, W, generator=g).bfloat16().cuda()
        b = torch.rand(n, 4, generator=g)
        x1, y1 = b[:, 0] * W * 1.1 - 0.05 * W, b[:, 1] * H * 1.1 - 0.05 * H          # some boxes start outside the image
        boxes = torch.stack([x1, y1, x1 + b[:, 2] * W * 0.6, y1 + b[:, 3] * H * 0.6], 1)
        boxes[0, 2:] = boxes[0, :2]                                                    # a zero-area box
        boxes = boxes.cuda()
        ids = synthetic_prompt(n, vocab=4096, seed=trial)
        e = eng.prefill(ids, pix, (gh, gw), aux, boxes, use_graph=False)
        e = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in e.items()}
        r = eng.prefill(ids, pix, (gh, gw), aux, boxes, use_graph=True)
        for k in ("image_tokens", "region_tokens", "last_hidden", "logits", "next_token"):
            assert torch.isfinite(r[k].float()).all(), f"{W}x{H} n={n}: {k} not finite"
            assert torch.equal(e[k], r[k]), f"{W}x{H} n={n}: {k} differs between eager and graph replay"
        assert r["region_tokens"].shape == (n, 2048) and r["image_tokens"].shape == (gh * gw // 4, 2048)
        if first is None:
            first = (ids, pix, (gh, gw), aux, boxes, {k: r[k].clone() for k in ("region_tokens", "logits")})
    ids, pix, grid, aux, boxes, ref = first
    again = eng.prefill(ids, pix, grid, aux, boxes, use_graph=True)
    assert torch.equal(again["region_tokens"], ref["region_tokens"]) and torch.equal(again["logits"], ref["logits"])


def test_free_running_greedy_ids_vs_oracle():
    """north_star: "decoded text/box-index outputs are bit-identical".  K = 16 free-running greedy tokens from the engine
    (prefill + KV-cache decode, graph path) against the oracle's greedy decode (oracle/llm_oracle.greedy_decode: HF greedy
    search + the reference's decode fast path, omchat_qwen2_5_vl.py:143-155) on the reduced model (true widths, ViT 4 blocks,
    LLM 2 layers, 4k vocab).  The oracle is teacher-forced on the ENGINE's ids, so every one of the 16 steps is compared even
    after a near-tie: at step i the engine's token must BE the oracle's argmax whenever the oracle's top-1 margin exceeds
    2 x the logit tolerance (0.05), and must in any case score within that tolerance of the oracle's maximum.  The ids are
    compared exactly (integers); the number of margin-qualified steps is asserted to be most of them."""
    from hfre_cases import box_fixtures
    from oracle import davit_oracle as DO, fpn_oracle as FO, hfre_oracle as HO, llm_oracle as LO, vit_oracle as VO
    from vlm_fo1_amd.llm import LLMConfig
    from vlm_fo1_amd.model import FO1Config, FO1Engine, random_weights, synthetic_prompt
    from vlm_fo1_amd.vit import ViTConfig
    K = 16
    cfg = FO1Config(vit=ViTConfig(depth=4, fullatt_block_indexes=(1, 3)), llm=LLMConfig(num_layers=2, vocab_size=4096, max_seq=1024))
    weights = random_weights(cfg, "cuda", seed=21)
    # random N(0, 0.02) embeddings give a 4096-way near-uniform softmax: scale the tied head so top-1 margins are not all ties
    weights["llm"]["embed_tokens.weight"] = (weights["llm"]["embed_tokens.weight"].float() * 4).bfloat16()
    eng = FO1Engine(cfg, weights, "cuda")
    H, W, gh, gw = 399, 500, 28, 36
    g = torch.Generator().manual_seed(10)
    pix = torch.randn(gh * gw, 1176, generator=g).bfloat16()
    aux = torch.randn(3, H, W, generator=g).bfloat16()
    it = [x for x in box_fixtures()["countbench"] if len(x["bboxes"]) == 7][0]
    boxes = torch.tensor(it["bboxes"], dtype=torch.float32) * torch.tensor([W / it["extent"][0], H / it["extent"][1]] * 2)
    ids = synthetic_prompt(boxes.shape[0], vocab=4096, seed=2)
    got = {}
    for graph in (False, True):
        got[graph] = eng.generate(ids, pix.cuda(), (gh, gw), aux.cuda(), boxes.cuda(), max_new_tokens=K, use_graph=graph)
        assert len(got[graph]) == K
    assert got[False] == got[True], "eager and graph-replayed greedy decodes differ"
    sd = cpu_state(weights)
    tokens, maps = VO.vit_forward(sd["vit"], pix.float(), gh, gw, depth=4, n_heads=16, fullatt=(1, 3))
    img_tok = mlp2(tokens, sd["proj"], "mm_projector.")
    fpn = [m.bfloat16() for m in FO.fpn_forward(sd["fpn"], maps[-1].bfloat16().float().reshape(gh, gw, 1280).permute(2, 0, 1).unsqueeze(0))]
    aux_maps, aux_sizes = DO.davit_forward(sd["davit"], aux.float().unsqueeze(0))
    aux_nchw = [m.bfloat16().reshape(h, w, -1).permute(2, 0, 1).unsqueeze(0) for m, (h, w) in zip(aux_maps, aux_sizes)]
    sw, sh = gw * 14 / W, gh * 14 / H
    feat = HO.hfre_oracle(aux_nchw, boxes, fpn, boxes * torch.tensor([sw, sh, sw, sh]), region_dim=5888, grid_hw=(gh, gw),
                          vt_strides=[3.5, 7, 14, 28])[0]
    reg_tok = mlp2(feat.bfloat16().float(), sd["proj"], "mm_projector_aux.")
    emb, nb, na = LO.splice(torch.tensor(ids), sd["llm"]["embed_tokens.weight"], img_tok, reg_tok)
    pos, delta = LO.rope_index(nb, (gh // 2, gw // 2), na)
    kw = dict(n_layers=2, n_heads=16, n_kv=2, head_dim=128, eps=1e-6, theta=1e6, sections=(16, 24, 24))
    ref_ids, ref_logits = LO.greedy_decode(sd["llm"], emb, pos, delta, K, forced=got[True], **kw)
    tol = 0.05
    qualified = 0
    for i in range(K):
        top2 = ref_logits[i].topk(2).values
        margin = float(top2[0] - top2[1])
        t = got[True][i]
        assert float(ref_logits[i].max() - ref_logits[i][t]) <= 2 * tol, \
            f"step {i}: engine token {t} scores {float(ref_logits[i].max() - ref_logits[i][t]):.3g} below the oracle's maximum"
        if margin > 2 * tol:
            qualified += 1
            assert t == ref_ids[i], f"step {i}: engine id {t} != oracle greedy id {ref_ids[i]} (oracle margin {margin:.3g})"
    assert qualified >= K // 2, f"only {qualified} of {K} steps had an oracle margin > {2 * tol}: the test is not discriminating"
