"""The device sampler on the MI355X (vlm_fo1_amd/csrc/sample.hip; cases, oracle and EPS: tests/sampling_cases.py).

  * every case through fo1_sample_rows_bf16 with its explicit draw: an "exact" draw returns the oracle's id, every other one satisfies the accept
    rule (the id is kept, u within EPS of its interval); rows with ld > V carry NaN past V, the id buffer a canary on both sides;
  * flat V = 4096 rows give id == x0 >> 20 for a grid of (seed, stream, counter): the device Philox and the fp64 comparison, bit for bit;
  * the id of a (row, parameters, seed, stream, counter) does not depend on its row b or on B, nor on the run;
  * fo1_decode_sample_accept: the counter is state[b][4] and advances, a sampled stop id and the budget finish a row, finished and all-NaN rows
    are inert (nothing recorded, state untouched, plan[1] = 0);
  * tiny model (2 layers, vocab 4096), 8 sequences x 16 tokens through BatchDecoder: each recorded id satisfies the accept rule on the logits
    step() returned for it; graph replay == eager; the same seed repeats, another seed changes at least one sequence; the single-sequence
    streamer path gives the ids of stream 0; generate(do_sample=True, temperature=0.7, top_p=0.9) returns [1, L_in + new].  The plug-in's
    streamer loop steps a one-sequence BatchDecoder (DESIGN.md section 14 says why), so that comparison checks the loop's plumbing; the
    sampled head of QwenLLM.decode_step / decode_step_graph is checked on its own steps' logits.

RESULTS_GPU (MI355X): every exact draw equal to the oracle's id and every other inside the accept rule."""
import numpy as np
import pytest
import torch

import sampling_cases as S

pytestmark = pytest.mark.gpu


def _dev_logits(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)


def test_every_case_exact_draws_equal_the_oracle_and_the_rest_meet_the_accept_rule():
    from vlm_fo1_amd import ops
    rows, batches = S.rows_and_batches()
    n_exact = n_rule = 0
    worst = 0.0
    for bt in batches:
        logits, params, us = S.batch_buffers(rows, bt)
        B, V = bt["B"], bt["V"]
        dl = _dev_logits(logits)[:, :V]
        out = torch.full((B + 16,), S.CANARY, dtype=torch.int32, device="cuda")
        ops.sample_rows(dl, ops.sample_params(params, "cuda"), u=torch.from_numpy(us).cuda(), out=out[8:8 + B])
        got = out.cpu().numpy()
        assert (got[:8] == S.CANARY).all() and (got[8 + B:] == S.CANARY).all(), "the id buffer's canary was overwritten"
        for b, (i, u) in enumerate(bt["items"]):
            o, g = rows[i]["oracle"], int(got[8 + b])
            assert S.accepts(o, u, g), (rows[i]["name"], bt["B"], b, u, g, S.pick(o, u))
            lo, hi = S.interval(o, g)
            worst = max(worst, lo - u, u - hi)
            if S.is_exact(o, u):
                n_exact += 1
                assert g == S.pick(o, u), (rows[i]["name"], bt["B"], b, u, g, S.pick(o, u))
            else:
                n_rule += 1
    print(f"\n{len(batches)} launches: {n_exact} exact draws equal the oracle, {n_rule} meet the accept rule; worst excursion out of the "
          f"interval {worst:.3g} = {worst / S.EPS:.3f} EPS")
    assert n_exact > n_rule > 0


def test_nucleus_of_one_equals_argmax_rows_and_bad_temperature_is_greedy():
    from vlm_fo1_amd import ops
    g = torch.Generator().manual_seed(3)
    V, B = 151936, 8
    logits = (torch.randn(B, V, generator=g) * 2).bfloat16()
    for b in range(B):
        logits[b, (b * 20011 + 17) % V] = 40.0
    dl = logits.cuda()
    want = ops.argmax_rows(dl).cpu()
    for T, top_p, top_k in ((1.0, 0.9, 0), (0.7, 0.9, 50), (0.0, 1.0, 0), (float("nan"), 1.0, 0), (-1.0, 0.5, 7), (1.0, 1.0, 1),
                            (1e-40, 1.0, 0), (float("inf"), 0.9, 0)):      # (1e-40: a denormal fp32, 1 / T overflows)
        got = ops.sample_rows(dl, ops.sample_params([(T, top_p, top_k, 11, b) for b in range(B)], "cuda")).cpu()
        assert torch.equal(got, want), (T, top_p, top_k, got, want)


def test_flat_rows_reproduce_the_philox_words_bit_for_bit():
    from vlm_fo1_amd import ops
    V = 4096
    grid = [(seed, stream, counter) for seed in (0, 1, 0xfedcba9876543210, (1 << 63) - 1) for stream in (0, 1, 31, 0xffffffff)
            for counter in (0, 1, 2, 4095, 0x7fffffff)]
    B = len(grid)
    logits = torch.full((B, V), 0.75, dtype=torch.bfloat16, device="cuda")
    counter = torch.tensor([c for _, _, c in grid], dtype=torch.int32, device="cuda")
    for top_p, top_k in ((1.0, 0), (0.9, 50)):      # (ties at the cut-offs are all kept: the flat row stays whole)
        params = ops.sample_params([(1.0, top_p, top_k, seed, stream) for seed, stream, _ in grid], "cuda")
        got = ops.sample_rows(logits, params, counter=counter).cpu().tolist()
        assert got == [S.philox_x0(c, st, seed) >> 20 for seed, st, c in grid]
    # counter = NULL is counter 0; a strided counter table reads element b * stride
    params = ops.sample_params([(1.0, 1.0, 0, 77, b) for b in range(4)], "cuda")
    assert ops.sample_rows(logits[:4], params).cpu().tolist() == [S.philox_x0(0, b, 77) >> 20 for b in range(4)]
    tab = torch.arange(32, dtype=torch.int32, device="cuda")
    assert ops.sample_rows(logits[:4], params, counter=tab, counter_stride=8).cpu().tolist() == [S.philox_x0(8 * b, b, 77) >> 20 for b in range(4)]


def test_id_is_independent_of_row_and_batch_and_repeats():
    from vlm_fo1_amd import ops
    g = torch.Generator().manual_seed(9)
    V = 32773
    row = (torch.randn(V, generator=g) * 3).bfloat16()
    par = (0.9, 0.9, 50, 0x5eed, 5)
    ids = set()
    for B, b in ((1, 0), (3, 2), (32, 17), (256, 255), (256, 0)):
        logits = (torch.randn(B, V, generator=g) * 3).bfloat16()
        logits[b] = row
        params = [(1.3, 1.0, 0, 1, i) for i in range(B)]
        params[b] = par
        counter = torch.full((B,), 3, dtype=torch.int32, device="cuda")
        dl, dp = logits.cuda(), ops.sample_params(params, "cuda")
        first = ops.sample_rows(dl, dp, counter=counter).cpu()
        again = ops.sample_rows(dl, dp, counter=counter).cpu()
        assert torch.equal(first, again), "two runs differ"
        ids.add(int(first[b]))
    assert len(ids) == 1, ids
    o = S.oracle(S.to_bits(row.float().numpy()), *par[:3])
    assert S.accepts(o, S.draw_u(3, 5, 0x5eed), ids.pop())


def test_decode_sample_accept_bookkeeping():
    from vlm_fo1_amd import ops
    V, B, CAP = 4096, 6, 8
    logits = torch.full((B, V), 0.5, dtype=torch.bfloat16)
    logits[4] = float("nan")                                  # row 4: finished, logits all NaN
    logits[5] = float("nan")                                  # row 5: live, no finite entry -> id 0
    dl = logits.cuda()
    seed = 0xabcdef
    params = ops.sample_params([(1.0, 1.0, 0, seed, b) for b in range(B)], "cuda")
    want0 = [S.philox_x0(1, b, seed) >> 20 for b in range(B)]         # counter 1 (one token generated by the prefill)
    want1 = [S.philox_x0(2, b, seed) >> 20 for b in range(B)]
    #          pos rope kv fin n_gen max
    state = torch.tensor([[10, 20, 0, 0, 1, 8, 0, 0],      # live
                          [11, 21, 0, 0, 1, 8, 0, 0],      # live; its first sampled id becomes the stop id below
                          [12, 22, 0, 0, 1, 2, 0, 0],      # budget 2: this step finishes it
                          [13, 23, 0, 1, 3, 8, 0, 0],      # finished before
                          [14, 24, 0, 1, 2, 8, 0, 0],      # finished, NaN logits
                          [15, 25, 0, 0, 1, 8, 0, 0]], dtype=torch.int32).cuda()
    before = state.clone()
    plan = torch.full((B, 2), 7, dtype=torch.int32, device="cuda")
    ids = torch.full((B, CAP), -1, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    stop = torch.tensor([want0[1]], dtype=torch.int32, device="cuda")
    ops.decode_sample_accept(dl, params, state, plan, ids, stop, done)
    st, pl, rec = state.cpu(), plan.cpu(), ids.cpu()
    assert rec[0, 1] == want0[0] and rec[1, 1] == want0[1] and rec[2, 1] == want0[2] and rec[5, 1] == 0
    assert (rec[:, 0] == -1).all() and (rec[3] == -1).all() and (rec[4] == -1).all()
    assert st[0].tolist() == [11, 21, 0, 0, 2, 8, 0, 0]                                  # the counter advanced with the position
    assert want0[0] != want0[1] != 0
    assert st[1, 3] == 1 and st[2, 3] == 1 and st[0, 3] == 0 and int(done.item()) == 2   # the sampled stop id and the budget finish a row
    assert torch.equal(st[3], before[3].cpu()) and torch.equal(st[4], before[4].cpu())   # finished rows: state untouched
    assert pl[:, 0].tolist() == [0] * B and pl[3, 1] == 0 and pl[4, 1] == 0 and pl[0, 1] == want0[0] and pl[5, 1] == 0
    ops.decode_sample_accept(dl, params, state, plan, ids, stop, done)                   # second step: counter 2 for the live rows
    rec, st = ids.cpu(), state.cpu()
    assert rec[0, 2] == want1[0] and st[0, 4] == 3 and rec[1, 2] == -1 and rec[2, 2] == -1 and st[1, 4] == 2
    assert int(done.item()) == 2 + (1 if want1[0] == want0[1] else 0)


def test_sampler_argument_errors_and_capture():
    from vlm_fo1_amd import lib as L, ops
    lib = L.load()
    n = lib.fo1_sample_rows_workspace_bytes(4096, 4)
    assert n > 0 and lib.fo1_sample_rows_workspace_bytes(4096, 0) == 0
    logits = torch.full((4, 4096), 0.25, dtype=torch.bfloat16, device="cuda")
    params = ops.sample_params([(1.0, 1.0, 0, 5, b) for b in range(4)], "cuda")
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    args = lambda **k: (k.get("logits", logits.data_ptr()), k.get("ld", 4096), k.get("V", 4096), k.get("B", 4), params.data_ptr(), None, 1, None,      # noqa: E731
                        out.data_ptr(), ws.data_ptr(), k.get("ws", 4096), None)
    assert lib.fo1_sample_rows_bf16(*args(B=0)) == -1 and b"B=0" in lib.fo1_last_error()
    assert lib.fo1_sample_rows_bf16(*args(B=257)) == -1 and b"B=257" in lib.fo1_last_error()
    assert lib.fo1_sample_rows_bf16(*args(ld=4095)) == -1 and b"ld_logits=4095" in lib.fo1_last_error()
    assert lib.fo1_sample_rows_bf16(*args(logits=None)) == -1 and b"NULL" in lib.fo1_last_error()
    assert lib.fo1_sample_rows_bf16(*args(ws=8)) == -2 and b"workspace" in lib.fo1_last_error()
    # capturable: the replayed launch reads the counter from device memory
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sample_rows(logits, params, counter=counter, counter_stride=0, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.sample_rows(logits, params, counter=counter, counter_stride=0, out=out)
    for c in (0, 5, 6):
        counter.fill_(c)
        g.replay()
        assert out.cpu().tolist() == [S.philox_x0(c, b, 5) >> 20 for b in range(4)]


# ---- the engine: tiny model (2 layers, vocab 4096), 8 sequences x 16 tokens ------------------------------------------------------------------
N_SEQ, N_TOK, SEED = 8, 16, 0x5a17ab1e5eed


@pytest.fixture(scope="module")
def tiny():
    from test_batched_decode_gpu import build
    from test_batched_prefill_gpu import make_request
    _, _, eng = build()
    reqs = [make_request(400 + i, 96 + 28 * (i % 3), 120 + 28 * (i % 2), 1 + (3 * i) % 5) for i in range(N_SEQ)]
    return eng, reqs


def _sampling(T=1.0, top_p=1.0, top_k=0, seed=SEED):
    return dict(temperature=T, top_p=top_p, top_k=top_k, seed=seed)


@pytest.mark.parametrize("T,top_k", [(1.0, 0), (0.7, 50)])
def test_every_recorded_id_meets_the_accept_rule_on_its_steps_logits(tiny, T, top_k):
    """(top_p = 1: a top-k cut-off is decided by exact counts; a nucleus cut-off on a model's logits may sit within EPS of top_p Z1, where the
    kept set itself is in doubt — the nucleus is checked on the constructed cases above.)"""
    from vlm_fo1_amd import ops
    eng, reqs = tiny
    samp = _sampling(T, 1.0, top_k)
    eng.prefill_batch(reqs, use_graph=False)
    hp = eng._last_batch
    logits = [eng._last_logits[:N_SEQ].clone()]
    table = ops.sample_params([(T, 1.0, top_k, SEED, b) for b in range(N_SEQ)], "cuda")
    first = ops.sample_rows(logits[0], table)
    dec = eng._decoder()
    dec.start(hp["seqs"], hp["delta"], first, N_TOK, (), sampling=samp)
    for _ in range(N_TOK - 1):
        logits.append(dec.step(use_graph=True)[:N_SEQ].clone())
    ids = dec.results()
    assert [len(r) for r in ids] == [N_TOK] * N_SEQ and [r[0] for r in ids] == first.cpu().tolist()
    n_exact = 0
    for t in range(N_TOK):
        bits = logits[t].view(torch.int16).cpu().numpy().view(np.uint16)
        for b in range(N_SEQ):
            o, u = S.oracle(bits[b], T, 1.0, top_k), S.draw_u(t, b, SEED)
            assert S.accepts(o, u, ids[b][t]), (t, b, u, ids[b][t], S.pick(o, u))
            if S.is_exact(o, u):
                n_exact += 1
                assert ids[b][t] == S.pick(o, u), (t, b, u)
    assert n_exact >= N_SEQ * N_TOK // 2
    # generate_batch draws the same: first tokens with counter 0, request i on stream i
    assert eng.generate_batch(reqs, max_new_tokens=N_TOK, use_graph=False, sampling=samp) == ids


def test_graph_equals_eager_seeds_repeat_and_differ(tiny):
    eng, reqs = tiny
    samp = _sampling()
    graph = eng.generate_batch(reqs, max_new_tokens=N_TOK, use_graph=True, sampling=samp)
    eager = eng.generate_batch(reqs, max_new_tokens=N_TOK, use_graph=False, sampling=samp)
    assert [len(r) for r in graph] == [N_TOK] * N_SEQ
    assert graph == eager, "eager and graph-replayed sampled decode differ"
    assert eng.generate_batch(reqs, max_new_tokens=N_TOK, use_graph=True, sampling=samp) == graph, "the same seed gave other ids"
    other = eng.generate_batch(reqs, max_new_tokens=N_TOK, use_graph=True, sampling=_sampling(seed=SEED + 1))
    assert any(a != b for a, b in zip(other, graph)), "another seed changed no sequence"
    greedy = eng.generate_batch(reqs, max_new_tokens=N_TOK, use_graph=True)
    assert greedy == eng.generate_batch(reqs, max_new_tokens=N_TOK, use_graph=True), "greedy decode is no longer reproducible"
    assert greedy != graph
    # a sampled stop id finishes its sequence right after it, the others go on
    stop = graph[3][5]
    cut = eng.generate_batch(reqs, max_new_tokens=N_TOK, stop_ids=[stop], use_graph=True, sampling=samp)
    for b in range(N_SEQ):
        n = graph[b].index(stop) + 1 if stop in graph[b] else N_TOK
        assert cut[b] == graph[b][:n], b


def test_single_sequence_step_head_meets_the_accept_rule_graph_and_eager(tiny):
    """QwenLLM.decode_step / decode_step_graph with set_sampling: the counter word advances on the device, each id meets the accept rule on
    the logits its own step returned, and the graph replays draw what the eager steps draw."""
    from vlm_fo1_amd import ops
    eng, reqs = tiny
    r, T, top_k = reqs[5], 1.0, 0
    runs = {}
    for graph in (False, True):
        out = eng.prefill(r["ids"], r["pix"], r["grid"], r["aux"], r["boxes"])
        eng.llm.reserve(eng.llm.kv_len + N_TOK)
        tok = ops.sample_rows(out["logits"], ops.sample_params([(T, 1.0, top_k, SEED, 0)], "cuda"))
        eng.llm.set_sampling(_sampling(T, 1.0, top_k), stream=0, counter=1)
        try:
            if graph:
                eng.llm.sync_decode_state()
            ids, logits = [int(tok.item())], [out["logits"].clone()]
            for i in range(N_TOK - 1):
                if graph:
                    lg, tok = eng.llm.decode_step_graph(tok if i == 0 else None)
                else:
                    _, lg, tok = eng.llm.decode_step(tok)
                logits.append(lg.clone())
                ids.append(int(tok.item()))
            assert int(eng.llm._sbuf["state"][0, 4].item()) == N_TOK
        finally:
            eng.llm.set_sampling(None)
        for t in range(N_TOK):
            o = S.oracle(logits[t].view(torch.int16).cpu().numpy().view(np.uint16)[0], T, 1.0, top_k)
            assert S.accepts(o, S.draw_u(t, 0, SEED), ids[t]), (graph, t, ids[t])
        runs[graph] = ids
    assert runs[False] == runs[True]
    # one step graph per head: a greedy step in between does not cost the sampled graph its capture
    sampled_graph = eng.llm._dgraph[True][0]
    out = eng.prefill(r["ids"], r["pix"], r["grid"], r["aux"], r["boxes"])
    eng.llm.reserve(eng.llm.kv_len + N_TOK)
    eng.llm.sync_decode_state()
    _, tok = eng.llm.decode_step_graph(out["next_token"])
    assert 0 <= int(tok.item()) < 4096 and eng.llm._dgraph[True][0] is sampled_graph and False in eng.llm._dgraph


class _Collect:
    def __init__(self):
        self.parts, self.ended = [], False

    def put(self, t):
        self.parts.append(t)

    def end(self):
        self.ended = True


def _generate_kwargs(r):
    gh, gw = r["grid"]
    return dict(inputs=torch.tensor([r["ids"]]), images=[r["pix"]], images_aux=[r["aux"]], image_grid_thws=[torch.tensor([[1, gh, gw]])],
                bbox_list=[r["boxes"]])


def test_streamer_path_draws_the_ids_of_batch_decoder_stream_0_and_generate_returns_the_hf_shape(tiny):
    from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig
    eng, reqs = tiny
    m = FO1ForCausalLM.from_engine(FO1HFConfig({}, {}), eng)
    r = reqs[2]
    kw = _generate_kwargs(r)
    L = kw["inputs"].shape[1]
    want = eng.generate_batch([r], max_new_tokens=N_TOK, use_graph=True, sampling=_sampling())[0]        # BatchDecoder, stream 0
    for use_graph in (True, False):
        m.use_graph = use_graph
        st = _Collect()
        out = m.generate(**kw, do_sample=True, temperature=1.0, top_p=1.0, top_k=0, seed=SEED, max_new_tokens=N_TOK, streamer=st)
        assert tuple(out.shape) == (1, L + N_TOK) and st.ended and len(st.parts) == 1 + N_TOK
        assert out[0, L:].tolist() == want, f"single-sequence loop (graph={use_graph}) != BatchDecoder stream 0"
        assert not eng.llm._sampled
    m.use_graph = True
    out = m.generate(**kw, do_sample=True, temperature=0.7, top_p=0.9, max_new_tokens=N_TOK)             # the device loop; seed from torch's generator
    assert tuple(out.shape) == (1, L + N_TOK) and out.dtype == kw["inputs"].dtype and out[0, :L].tolist() == r["ids"]
    assert int(out[0, L:].min()) >= 0 and int(out[0, L:].max()) < 4096
    torch.manual_seed(77)
    a = m.generate(**kw, do_sample=True, temperature=0.7, top_p=0.9, max_new_tokens=N_TOK)
    torch.manual_seed(77)
    assert torch.equal(a, m.generate(**kw, do_sample=True, temperature=0.7, top_p=0.9, max_new_tokens=N_TOK)), "torch.manual_seed does not reproduce a run"
    many = m.generate_many([dict(_generate_kwargs(q), do_sample=True, temperature=0.7, top_p=0.9, seed=SEED, max_new_tokens=6) for q in reqs[:3]])
    assert [tuple(o.shape) for o in many] == [(1, len(q["ids"]) + 6) for q in reqs[:3]]
    assert m.generate(**kw, do_sample=False, temperature=0.7, max_new_tokens=4).tolist() == m.generate(**kw, max_new_tokens=4).tolist()
    with pytest.raises(ValueError, match="at most 4096 tokens"):      # a sampled generation records its ids in the BatchDecoder's buffer
        m.generate(**kw, do_sample=True, temperature=1.0, max_new_tokens=4097)
    # a batch the device stop rule cannot take is decoded one by one: request i still draws on stream i of the one seed
    never = [lambda ids, scores: False]
    skw = dict(kw, do_sample=True, temperature=1.0, top_p=1.0, top_k=0, seed=SEED, max_new_tokens=N_TOK, stopping_criteria=never)
    one, two = m.generate_many([skw, skw])
    assert one[0, L:].tolist() == want and tuple(two.shape) == (1, L + N_TOK) and two[0, L:].tolist() != want
