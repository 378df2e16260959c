"""The trimmed last LLM layer (fo1_llm_prefill_tail, csrc/stages.hip; llm.QwenLLM._forward with `tail`): after the last layer's q/k/v
launch only each sequence's last real row is read, so attention runs over the query blocks that hold those rows and o-projection, MLP,
final norm, lm_head and ONE batched greedy pick (fo1_argmax_rows_bf16) run at M = number of sequences.

The reference side is always the all-row path of the same build (`collect` given), never the trimmed path against itself:
  * GEMM tile pinned (a row's k-order then does not depend on M): trimmed == all-row BIT for bit in last hidden, logits and ids, the KV
    cache of every layer is untouched, and decoding from it gives the same ids — packed ragged batch, one-image prefill, shared prefix;
  * automatic dispatch at the benchmark's 25 x 651 rows and full widths: the tail's products take another tile shape, i.e. another fp32
    summation order in ONE layer — the bound of test_batched_prefill_gpu.test_uniform_batch_auto_tiles_tolerance_and_graph;
  * fo1_argmax_rows_bf16 == the fo1_argmax_bf16 loop, first index among planted ties;
  * fo1_llm_prefill with and without hidden_out."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def llm_state(cfg, seed):
    """Seeded N(0, 0.02^2) projections and ~1 norms under the checkpoint's key names (the LLM part of model.random_weights)."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def w(*s):
        return (torch.randn(*s, generator=g, device="cuda", dtype=torch.float32) * 0.02).to(torch.bfloat16)

    def ones(n):
        return (1 + 0.02 * torch.randn(n, generator=g, device="cuda")).to(torch.bfloat16)

    d, hq, hk, ff = cfg.hidden_size, cfg.num_heads * cfg.head_dim, cfg.num_kv_heads * cfg.head_dim, cfg.intermediate_size
    sd = {"embed_tokens.weight": w(cfg.vocab_size, d), "norm.weight": ones(d)}
    for i in range(cfg.num_layers):
        p = f"layers.{i}."
        sd.update({p + "input_layernorm.weight": ones(d), p + "post_attention_layernorm.weight": ones(d),
                   p + "self_attn.q_proj.weight": w(hq, d), p + "self_attn.q_proj.bias": w(hq), p + "self_attn.k_proj.weight": w(hk, d),
                   p + "self_attn.k_proj.bias": w(hk), p + "self_attn.v_proj.weight": w(hk, d), p + "self_attn.v_proj.bias": w(hk),
                   p + "self_attn.o_proj.weight": w(d, hq), p + "mlp.gate_proj.weight": w(ff, d), p + "mlp.up_proj.weight": w(ff, d),
                   p + "mlp.down_proj.weight": w(d, ff)})
    return sd


def make_llm(seed=3, layers=2, vocab=4096, max_seq=4096):
    from vlm_fo1_amd.llm import LLMConfig, QwenLLM
    cfg = LLMConfig(num_layers=layers, vocab_size=vocab, max_seq=max_seq)
    return QwenLLM(cfg, llm_state(cfg, seed), "cuda")


def packed_inputs(llm, shapes, seed, vocab, shared=False):
    """shapes: [(merged grid, regions)] -> (plan_batch result, packed embedding rows): seeded image / region token rows spliced into seeded prompts.
    shared: every prompt reads ONE image and carries the same preamble (the first shape's grid)."""
    from vlm_fo1_amd.model import synthetic_prompt
    g = torch.Generator().manual_seed(seed)
    d = llm.cfg.hidden_size
    prompts = [synthetic_prompt(nb, vocab=vocab, seed=seed + k, lead_seed=seed if shared else None) for k, (_, nb) in enumerate(shapes)]
    grids = [shapes[0][0] if shared else gr for gr, _ in shapes]
    n_img = [gr[0] * gr[1] for gr in grids]
    hp = llm.plan_batch(prompts, n_img, [nb for _, nb in shapes], grids, img_base=[0] * len(shapes) if shared else None, share_prefix=shared)
    img = torch.randn(n_img[0] if shared else sum(n_img), d, generator=g).bfloat16().cuda()
    reg = torch.randn(sum(nb for _, nb in shapes), d, generator=g).bfloat16().cuda()
    llm.reserve(hp["rows"])
    return hp, llm.embed_rows(hp["plan"].cuda(), img, reg)


def run_packed(llm, hp, emb, all_rows):
    collect = [] if all_rows else None
    last, logits, toks = llm.prefill_packed(emb, hp["cos"].cuda(), hp["sin"].cuda(), hp["seqs"], hp["last"].cuda(), collect=collect)
    torch.cuda.synchronize()
    if all_rows:
        assert len(collect) == llm.cfg.num_layers and collect[-1].shape[0] == emb.shape[0]
    return last.clone(), logits.clone(), toks.clone(), llm.kcache[:, :, :hp["rows"]].clone(), llm.vtcache[:, :, :hp["rows"]].clone()


def decode_ids(llm, hp, first, steps=4):
    from vlm_fo1_amd.llm import BatchDecoder
    dec = BatchDecoder(llm)
    dec.start(hp["seqs"], hp["delta"], first, steps)
    return dec.run(steps, use_graph=False)


class pinned:
    """128 x 128 two-stage tiles for every GEMM, no split-K, no GEMV route: the pins of test_ragged_batch_equals_sequential_bitwise_with_pinned_tile."""

    def __enter__(self):
        from vlm_fo1_amd import lib as L
        L.check(L.load().fo1_gemm_set_variant(2, 1), "variant")
        L.check(L.load().fo1_gemm_set_splitk(1), "splitk")
        L.check(L.load().fo1_gemm_set_gemv(0), "gemv")

    def __exit__(self, *exc):
        from vlm_fo1_amd import lib as L
        L.load().fo1_gemm_set_variant(0, 0)
        L.load().fo1_gemm_set_splitk(0)
        L.load().fo1_gemm_set_gemv(1)
        return False


RAGGED = [((18, 13), 7), ((12, 25), 33), ((2, 2), 1), ((15, 15), 100)]
SHARED = [((17, 23), 40), ((17, 23), 40), ((17, 23), 11)]


@pytest.mark.parametrize("case", ["ragged", "shared_prefix"])
def test_packed_trimmed_equals_all_rows_bitwise_with_pinned_tile(ab_library, case):
    llm = make_llm()
    hp, emb = packed_inputs(llm, SHARED if case == "shared_prefix" else RAGGED, 21, 4096, shared=case == "shared_prefix")
    if case == "shared_prefix":
        assert all(len(sq) == 5 for sq in hp["seqs"]) and llm.packed_items(hp["seqs"])[2] is not None
    with pinned():
        ref = run_packed(llm, hp, emb, all_rows=True)
        ref_ids = decode_ids(llm, hp, ref[2])
        llm.kcache.zero_(); llm.vtcache.zero_()
        got = run_packed(llm, hp, emb, all_rows=False)
        got_ids = decode_ids(llm, hp, got[2])
    for name, a, b in zip(("last_hidden", "logits", "next ids", "kcache", "vtcache"), ref, got):
        assert torch.equal(a, b), f"{case}: {name} differs between the trimmed and the all-row pass"
    assert ref[0].shape == (len(hp["seqs"]), llm.cfg.hidden_size) and ref[2].dtype == torch.int32
    assert got_ids == ref_ids and all(len(x) == 4 for x in got_ids)


def test_one_image_prefill_trimmed_equals_all_rows_bitwise_with_pinned_tile(ab_library):
    llm = make_llm(seed=4)
    hp, emb = packed_inputs(llm, [((17, 23), 100)], 33, 4096)
    L_ = hp["seqs"][0][1]
    x, pos, delta = emb[:L_].contiguous(), hp["pos"][0], hp["delta"][0]
    assert L_ == 651

    def run(all_rows):
        llm.kcache.zero_(); llm.vtcache.zero_()
        last, logits, tok = llm.prefill(x, pos, delta, collect=[] if all_rows else None)
        out = [last.clone(), logits.clone(), tok.clone().view(-1), llm.kcache[:, :, :L_].clone(), llm.vtcache[:, :, :L_].clone()]
        ids = [int(tok.item())]
        for _ in range(3):
            _, _, tok = llm.decode_step(tok)
            ids.append(int(tok.item()))
        return out, ids

    with pinned():
        ref, ref_ids = run(True)
        got, got_ids = run(False)
    for name, a, b in zip(("last_hidden", "logits", "next id", "kcache", "vtcache"), ref, got):
        assert torch.equal(a, b), f"one image: {name} differs between the trimmed and the all-row pass"
    assert got_ids == ref_ids


AUTO_SEED = 1      # chosen on the REFERENCE side alone: this seed's all-row pass has 19 of 25 sequences above the id margin (seeds 0, 2, 3: 13, 10, 11;
                   # profiles/llm_last_layer_tail_ab.json) — with an iid N(0, 0.02) head the greedy pick is a 152k-way near-tie for the rest
AUTO_MIN_CLEAR = 13      # more than half of the batch, or the id check proves nothing


def test_bench_shape_auto_dispatch_within_the_packed_pass_tolerance():
    """25 x 651 rows at the model's widths and vocabulary, 2 layers, automatic dispatch: the all-row pass runs the last layer's three products
    on the 256 x 256 kernel at M = 16 300, the trimmed pass on the small-M kernels at M = 25 (split-K down projection).  Bound: that of a packed
    pass against one-image passes (test_batched_prefill_gpu) — min row cosine >= 0.9995, max deviation <= 2^-4 of the largest element,
    |dlogits| <= 0.05, equal ids wherever the reference's top-2 margin exceeds 0.1, which must be the case for at least half of the batch."""
    llm = make_llm(seed=AUTO_SEED, vocab=151936, max_seq=16384)
    hp, emb = packed_inputs(llm, [((17, 23), 100)] * 25, 1234, 151936)
    assert hp["rows"] == 25 * 652
    ref = run_packed(llm, hp, emb, all_rows=True)
    got = run_packed(llm, hp, emb, all_rows=False)
    assert torch.equal(ref[3], got[3]) and torch.equal(ref[4], got[4]), "the KV cache moved"
    x, y = ref[0].float(), got[0].float()
    cos = F.cosine_similarity(x, y, dim=-1).min().item()
    rel = ((x - y).abs().max() / x.abs().max()).item()
    err = (ref[1].float() - got[1].float()).abs().max().item()
    top2 = ref[1].float().topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0.1
    same = ref[2] == got[2]
    print(f"tail vs all rows: min cos {cos:.6f} rel {rel:.4g} max |dlogits| {err:.4g} clear margins {int(clear.sum())}/25 equal ids {int(same.sum())}/25")
    assert cos >= 0.9995 and rel <= 2 ** -4, f"last_hidden: min cos {cos:.6f} rel {rel:.4g}"
    assert err <= 0.05, f"logits differ by {err:.4g}"
    assert int(clear.sum()) >= AUTO_MIN_CLEAR, f"only {int(clear.sum())} of 25 reference rows have a top-2 margin above 0.1: the id check proves nothing"
    assert bool(same[clear].all()), f"ids differ at clear margins: {ref[2][clear & ~same].tolist()} vs {got[2][clear & ~same].tolist()}"


@pytest.mark.parametrize("V", [4096, 151936])
def test_argmax_rows_equals_the_row_loop_first_index_wins(V):
    from vlm_fo1_amd import ops
    B = 25
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(B, V, generator=g).bfloat16()
    per = (V + 127) // 128                            # slice of one stage-1 workgroup
    want = {}
    plant = [(0, [5, 6]), (1, [per - 1, per]), (2, [V - 1, 0]), (3, [3 * per + 7, 90 * per + 1, 127 * per]), (4, [V - 2, V - 1]), (24, [per, 2 * per, 64 * per])]
    for b, at in plant:
        logits[b, [i for i in at if i < V]] = 9.0     # above every random value: the tie is the maximum
        want[b] = min(i for i in at if i < V)
    logits[5] = 1.0                                   # a constant row: index 0
    want[5] = 0
    logits = logits.cuda()
    padded = torch.zeros(B, V + 8, dtype=torch.bfloat16, device="cuda")      # a row pitch wider than the vocabulary
    padded[:, V:] = 50.0
    padded[:, :V] = logits
    loop = torch.empty(B, dtype=torch.int32, device="cuda")
    for b in range(B):
        ops.argmax(logits[b], out=loop[b:b + 1])
    got = ops.argmax_rows(logits)
    got_p = ops.argmax_rows(padded[:, :V])
    assert got.dtype == torch.int32 and torch.equal(got, loop) and torch.equal(got_p, loop)
    for b, i in want.items():
        assert int(got[b]) == i, f"row {b}: {int(got[b])}, first of the tied maxima is {i}"


def test_stage_entry_with_and_without_hidden_out(ab_library):
    """fo1_llm_prefill: without hidden_out the last layer runs trimmed, with it every row — same head outputs under pinned tiles, equal to the
    Python path's, and hidden_out still holds the final residual stream of every row."""
    from vlm_fo1_amd import stage_abi
    llm = make_llm(seed=5)
    hp, emb = packed_inputs(llm, RAGGED, 44, 4096)
    cos, sin, last_plan = hp["cos"].cuda(), hp["sin"].cuda(), hp["last"].cuda()
    with pinned():
        collect = []
        py = llm.prefill_packed(emb, cos, sin, hp["seqs"], last_plan, collect=collect)
        py = [t.clone() for t in py] + [collect[-1].clone()]
        kc, vt = llm.kcache.clone(), llm.vtcache.clone()
        st = stage_abi.llm_stage(llm)
        llm.kcache.zero_(); llm.vtcache.zero_()
        full = [t.clone() for t in st.prefill_packed(emb, cos, sin, hp["seqs"], last_plan, want_hidden=True)]
        assert torch.equal(llm.kcache, kc) and torch.equal(llm.vtcache, vt)
        llm.kcache.zero_(); llm.vtcache.zero_()
        trim = [t.clone() for t in st.prefill_packed(emb, cos, sin, hp["seqs"], last_plan)]
        assert torch.equal(llm.kcache, kc) and torch.equal(llm.vtcache, vt)
    for name, a, b, c in zip(("last_hidden", "logits", "next ids"), py, full, trim):
        assert torch.equal(a, b), f"{name}: all-row stage entry vs the Python all-row path"
        assert torch.equal(a, c), f"{name}: trimmed stage entry vs the all-row path"
    assert torch.equal(full[3], py[3]), "hidden_out is not the final residual stream of every row"
