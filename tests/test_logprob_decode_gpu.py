"""Log-probability records through the decode loops (vlm_fo1_amd.llm.BatchDecoder / DecodePool, serving.PoolService, FO1Engine, the plug-in;
DESIGN.md section 14) on the tiny engine of tests/test_batched_decode_gpu.py (V = 4096): 8 sequences, 16 tokens, a 64-slot pool, the request
mix of tests/test_pool_sampling_gpu.py (plain greedy, greedy + penalty, sampled, sampled + penalty), five of them asking for records with
different n, three not.

  * per-step parity: every recorded (lp, top ids, top lps) of every requesting sequence equals the fp64 oracle (tests/logprob_cases.py, ids
    exactly, values within EPS_LP) on THAT step's logits — what pool.step() / BatchDecoder.step() returns, and the prefill's logits for
    column 0 — whatever head picked the token;
  * ids unchanged: every sequence's ids are those of the same submission without `logprobs`, the non-requesting plain neighbour's those of an
    all-plain pool run;
  * graph replay == eager; a sequence's record is the same in slot 0 alone and in slot 37 among neighbours; after the last requesting
    sequence has been harvested the next step's graph key is graph_key(bucket) again; a pool that never saw a request holds no buffer;
  * the paths agree: generate_batch(logprobs=[...]) with the pool on, submit_batch's PoolHandle.logprobs() and the direct pool run return the
    same ids and the same records, bit for bit; generate_batch with the pool off returns those of the direct BatchDecoder run, bit for bit.
    The pool steps through the tile GEMMs and the BatchDecoder through the batched GEMV kernels: their logits differ in last bits
    (tests/test_pool_sampling_gpu.py), so across the two the greedy ids are equal and the records agree within what the logits allow:
    lp = l_c - logsumexp(l) and the k-th largest logit are 1-Lipschitz in the maximum norm, hence |lp_pool - lp_decoder| <= 2 max_i
    |l_pool_i - l_decoder_i| (+ 2 EPS_LP max(1, |lp|) for the two kernels' own error) on every step the two loops reached with the same ids;
  * the plug-in: generate(output_logprobs=True, top_logprobs=3) returns the object with the documented shapes, `.sequences` equal to the
    plain call's tensor, and the same ids and records with a streamer; generate_many takes a batch that mixes requesting and other requests,
    pool off and on."""
import numpy as np
import pytest
import torch

import logprob_cases as C
from test_pool_sampling_gpu import N_SEQ, N_TOK, _Collect, _generate_kwargs, _kinds

pytestmark = pytest.mark.gpu

WANTS = [3, 8, 0, 5, None, 1, None, 8]      # per sequence: the record's top-n, None = no record (kinds: b % 4 = plain, greedy + pen, sampled, sampled + pen)
REQ = [b for b, w in enumerate(WANTS) if w is not None]


class _Fx:
    pass


@pytest.fixture(scope="module")
def fx():
    from test_batched_decode_gpu import build
    from test_batched_prefill_gpu import make_request
    from vlm_fo1_amd.llm import DecodePool
    f = _Fx()
    _, _, f.eng = build()
    f.reqs = [make_request(400 + i, 96 + 28 * (i % 3), 120 + 28 * (i % 2), 1 + (3 * i) % 5) for i in range(N_SEQ)]
    f.per = _kinds()
    f.per_req = [None if sp is None else {k: v for k, v in sp.items() if k != "stream"} for sp in f.per]      # (request i draws on stream i)
    _prefill(f)
    f.logits0 = f.eng._last_logits[:N_SEQ].clone()
    f.first_greedy = f.eng._last_next_tokens[:N_SEQ].clone()
    f.first = f.eng._first_tokens(f.per, f.reqs).clone()
    f.first_lp = tuple(t.clone() for t in f.eng._first_logprobs(WANTS, f.first, N_SEQ))
    f.pool = DecodePool(f.eng.llm, slots=64)
    # before any request: the runs the others are compared with, and a pool that holds no record buffer
    f.plain_ids = _run(f, list(range(N_SEQ)), f.per, f.first, wants=None)[0]
    f.allg_ids = _run(f, list(range(N_SEQ)), None, f.first_greedy, wants=None)[0]
    assert f.pool.lpb is None and f.pool.n_logprob == 0, "a pool that never saw a request holds a logprob buffer"
    return f


def _prefill(f):
    """The requests' K / V^T rows back into the engine's prefill cache (another test's generate calls overwrite it)."""
    f.eng.prefill_batch(f.reqs, use_graph=False)
    f.hp = f.eng._last_batch


def _join(f, sel, per, first, wants=WANTS, budget=N_TOK):
    pool, eng = f.pool, f.eng
    lpa = {}
    if wants is not None:
        idx = torch.tensor(sel, device=f.first_lp[0].device)
        lpa = dict(logprobs=[wants[b] for b in sel], first_logprobs=tuple(t[idx] for t in f.first_lp))
    return pool.join(eng.llm.kcache, eng.llm.vtcache, [f.hp["seqs"][b] for b in sel], [f.hp["delta"][b] for b in sel],
                     torch.stack([first[b] for b in sel]), budget, (), tags=[("t", b) for b in sel],
                     sampling=None if per is None else [per[b] for b in sel], prompt_ids=[f.reqs[b]["ids"] for b in sel], **lpa)


def _run(f, sel, per, first, wants=WANTS, graph=True):
    """-> (ids per sequence of sel, records per sequence of sel)."""
    _prefill(f)
    _join(f, sel, per, first, wants)
    got = {tag[1]: (ids, rec) for _, tag, ids, rec in f.pool.drain(use_graph=graph, poll=5, records=True)}
    assert not f.pool.live and len(f.pool.free) == f.pool.P and f.pool.n_general == 0 and f.pool.n_logprob == 0
    return [got[b][0] for b in sel], [got[b][1] for b in sel]


def _bits(row: torch.Tensor) -> np.ndarray:
    return row.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _same(a, b) -> bool:
    """Two records (or None), bit for bit."""
    if a is None or b is None:
        return a is None and b is None
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
               for x, y in zip(a, b))


def _check_against_the_steps_logits(logits, ids, recs, who):
    """logits[t][b]: the row sequence b's token t was picked from.  Every requesting sequence's record against the oracle on it."""
    worst = 0.0
    for b in range(N_SEQ):
        rec, n = recs[b], WANTS[b]
        if n is None:
            assert rec is None, (who, b)
            continue
        assert tuple(rec.logprob.shape) == (N_TOK,) and rec.logprob.dtype == torch.float32
        assert tuple(rec.top_ids.shape) == (N_TOK, n) and rec.top_ids.dtype == torch.int32
        assert tuple(rec.top_logprobs.shape) == (N_TOK, n) and rec.top_logprobs.dtype == torch.float32
        for t in range(N_TOK):
            o = C.oracle(_bits(logits[t][b]), C.TOP_MAX)
            worst = max(worst, C.check_row((who, b, t), o, ids[b][t], n, rec.logprob[t].item(), rec.top_ids[t].numpy(), rec.top_logprobs[t].numpy()))
    print(f"\n{who}: {len(REQ)} sequences x {N_TOK} steps, worst |lp - lp_fp64| / max(1, |lp_fp64|) = {worst:.3g} = {worst / C.EPS_LP:.3f} EPS_LP")


def _pool_steps(f):
    """The mixed submission through the pool, step by step -> (logits per step [N_SEQ rows], ids, records); computed once."""
    if not hasattr(f, "pool_steps"):
        _prefill(f)
        slots = _join(f, list(range(N_SEQ)), f.per, f.first)
        assert f.pool.n_logprob == len(REQ) and f.pool.lpb is not None
        logits = [f.logits0]
        for _ in range(N_TOK - 1):
            logits.append(f.pool.step(use_graph=True)[slots].clone())
        assert any("logprobs" in k for k in f.pool._graphs)
        got = {tag[1]: (ids, rec) for _, tag, ids, rec in f.pool.harvest(f.pool.snapshot(), records=True)}
        assert not f.pool.live and f.pool.n_logprob == 0
        f.pool_steps = (logits, [got[b][0] for b in range(N_SEQ)], [got[b][1] for b in range(N_SEQ)])
    return f.pool_steps


def _decoder_steps(f):
    """The same through one BatchDecoder -> (logits per step, ids, records); computed once."""
    if not hasattr(f, "dec_steps"):
        _prefill(f)
        dec = f.eng._decoder()
        dec.start(f.hp["seqs"], f.hp["delta"], f.first, N_TOK, (), sampling=f.per, prompt_ids=[r["ids"] for r in f.reqs], logprobs=WANTS,
                  first_logprobs=f.first_lp)
        logits = [f.logits0]
        for _ in range(N_TOK - 1):
            logits.append(dec.step(use_graph=True)[:N_SEQ].clone())
        assert any("logprobs" in k for k in dec._graphs)
        f.dec_steps = (logits, dec.results(), dec.logprobs())
    return f.dec_steps


def test_every_record_equals_the_oracle_on_its_steps_logits_and_the_ids_are_unchanged(fx):
    f = fx
    logits, ids, recs = _pool_steps(f)
    assert [len(r) for r in ids] == [N_TOK] * N_SEQ and [r[0] for r in ids] == f.first.cpu().tolist()
    _check_against_the_steps_logits(logits, ids, recs, "pool")
    assert ids == f.plain_ids, "asking for log-probabilities changed a sequence's ids"
    assert ids[4] == f.allg_ids[4], "the non-requesting plain neighbour's ids are not those of an all-plain pool run"
    assert ids[0] == f.allg_ids[0]
    dl, dids, drecs = _decoder_steps(f)
    assert [len(r) for r in dids] == [N_TOK] * N_SEQ
    _check_against_the_steps_logits(dl, dids, drecs, "BatchDecoder")


def test_graph_equals_eager_slots_do_not_matter_and_the_key_falls_back(fx):
    f = fx
    pool = f.pool
    _, ids, recs = _pool_steps(f)
    eids, erecs = _run(f, list(range(N_SEQ)), f.per, f.first, graph=False)
    assert eids == ids and all(_same(a, b) for a, b in zip(erecs, recs)), "eager and graph-replayed steps differ"
    for b in (0, 3, 1):      # plain, sampled + penalty, greedy + penalty: alone in slot 0
        i1, r1 = _run(f, [b], f.per, f.first)
        assert i1 == [ids[b]] and _same(r1[0], recs[b]), f"sequence {b}'s record differs alone in slot 0"
    pool.free = list(range(37, 64))      # slot 37 with 7 neighbours behind it (the join takes the lowest free slots: hide 0 .. 36 from it)
    try:
        order = [3, 0, 1, 2, 4, 5, 6, 7]
        _prefill(f)
        slots = _join(f, order, f.per, f.first)
        assert slots[0] == 37
        got = {tag[1]: (i, r) for _, tag, i, r in pool.drain(use_graph=True, poll=5, records=True)}
    finally:
        pool.free = list(range(64))
    assert [got[b][0] for b in range(N_SEQ)] == ids and all(_same(got[b][1], recs[b]) for b in range(N_SEQ)), "a record depends on the slot"
    # a slot a requesting sequence has left is reused by a non-requesting one: its `want` word goes back to -1, nothing is recorded for it;
    # requesting sequences in flight beside plain ones, then gone: the step is the all-greedy one under graph_key(bucket) again
    _prefill(f)
    s_plain = _join(f, [4], None, f.first_greedy, wants=[None] * N_SEQ)
    assert pool.lp_dev[s_plain[0]] == -1 and pool.n_logprob == 0
    _join(f, [0, 5], f.per, f.first, budget=4)
    assert pool.n_logprob == 2 and pool.n_general == 1
    for _ in range(3):
        pool.step()
    got = {tag[1]: (i, r) for _, tag, i, r in pool.harvest(pool.snapshot(), records=True)}
    assert sorted(got) == [0, 5] and pool.n_logprob == 0 and pool.n_general == 0 and len(pool.live) == 1
    for b in (0, 5):
        assert got[b][0] == ids[b][:4]
        assert all(torch.equal(x.view(torch.int32), y[:4].contiguous().view(torch.int32)) for x, y in zip(got[b][1], recs[b]))
    pool._graphs.clear()
    pool.step()
    assert list(pool._graphs) == [pool.graph_key(pool.kv_bucket())], "with no requesting sequence live the step's graph key is not the all-greedy key"
    rest = pool.drain(poll=4, records=True)
    assert [(tag[1], i, r) for _, tag, i, r in rest] == [(4, f.allg_ids[4], None)]


def test_the_paths_agree(fx):
    f = fx
    eng = f.eng
    pl, ids, recs = _pool_steps(f)
    dl, dids, drecs = _decoder_steps(f)
    # pool on: the scheduler's pool and its handle == the direct pool run
    eng.enable_decode_pool(slots=64)
    try:
        gids, grecs = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=f.per_req, logprobs=WANTS)
        assert gids == ids and all(_same(a, b) for a, b in zip(grecs, recs)), "generate_batch (pool on) != the direct pool run"
        h = eng.submit_batch(f.reqs, N_TOK, (), True, sampling=f.per_req, logprobs=WANTS)
        assert h.result() == ids and all(_same(a, b) for a, b in zip(h.logprobs(), recs)), "PoolHandle.logprobs() != the direct pool run"
        assert eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=f.per_req) == ids      # (no argument: the list, as ever)
        assert eng._pool_svc.pool.n_logprob == 0
    finally:
        eng.disable_decode_pool()
    # pool off: the BatchDecoder group == the direct BatchDecoder run
    bids, brecs = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=f.per_req, logprobs=WANTS)
    assert bids == dids and all(_same(a, b) for a, b in zip(brecs, drecs)), "generate_batch (pool off) != the direct BatchDecoder run"
    assert eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=f.per_req) == dids
    # across the two kernel families (module docstring): equal greedy ids, records within 2 max |delta logit| wherever the histories agree
    assert dids[0] == ids[0] and dids[4] == ids[4], "the plain greedy ids of the pool and of the BatchDecoder differ"
    n_cmp = 0
    for b in REQ:
        for t in range(N_TOK):
            if dids[b][:t + 1] != ids[b][:t + 1]:
                break
            dmax = float((pl[t][b].float() - dl[t][b].float()).abs().max())
            for a, c in ((recs[b].logprob[t], drecs[b].logprob[t]), *zip(recs[b].top_logprobs[t], drecs[b].top_logprobs[t])):
                a, c = float(a), float(c)
                assert abs(a - c) <= 2 * dmax + 2 * C.EPS_LP * max(1.0, abs(a)), (b, t, a, c, dmax)
                n_cmp += 1
    assert n_cmp >= N_TOK * (1 + WANTS[0])


def test_plug_in_generate_and_generate_many(fx):
    from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig, GenerateLogprobsOutput
    f = fx
    eng = f.eng
    m = FO1ForCausalLM.from_engine(FO1HFConfig({}, {}), eng)
    kws = [dict(_generate_kwargs(r), max_new_tokens=6) for r in f.reqs[:4]]
    L = kws[2]["inputs"].shape[1]
    plain = m.generate(**kws[2])
    out = m.generate(**kws[2], output_logprobs=True, top_logprobs=3)
    assert isinstance(out, GenerateLogprobsOutput) and torch.equal(out.sequences, plain) and tuple(plain.shape) == (1, L + 6)
    assert tuple(out.logprobs.shape) == (1, 6) and out.logprobs.dtype == torch.float32
    assert tuple(out.top_ids.shape) == (1, 6, 3) and out.top_ids.dtype == torch.int64
    assert tuple(out.top_logprobs.shape) == (1, 6, 3) and out.top_logprobs.dtype == torch.float32
    # greedy: the chosen token is the most likely one, and its log-probability is the first top entry's
    assert out.top_ids[0, :, 0].tolist() == plain[0, L:].tolist() and torch.equal(out.top_logprobs[0, :, 0], out.logprobs[0])
    assert bool((out.logprobs <= 0).all()) and bool((out.top_logprobs[0, :, :-1] >= out.top_logprobs[0, :, 1:]).all())
    st = _Collect()
    so = m.generate(**kws[2], output_logprobs=True, top_logprobs=3, streamer=st)
    assert st.ended and torch.equal(so.sequences, plain)
    for a, b in ((so.logprobs, out.logprobs), (so.top_ids, out.top_ids), (so.top_logprobs, out.top_logprobs)):
        assert torch.equal(a, b), "the streamer loop's record differs from the device loop's"
    zero = m.generate(**kws[2], output_logprobs=True)
    assert tuple(zero.top_ids.shape) == (1, 6, 0) and torch.equal(zero.logprobs, out.logprobs)
    samp = dict(do_sample=True, temperature=0.7, top_p=0.9, seed=3)
    sp = m.generate(**kws[1], **samp)
    so = m.generate(**kws[1], **samp, output_logprobs=True, top_logprobs=8)
    assert torch.equal(so.sequences, sp) and tuple(so.top_ids.shape) == (1, 6, 8), "asking for log-probabilities changed a sampled generation"
    # generate_many: requesting and other requests in one batch; each result is the tensor or the object accordingly
    base = m.generate_many(kws[:3])
    batch = [kws[0], dict(kws[1], output_logprobs=True, top_logprobs=2), dict(kws[2], output_logprobs=True)]
    for pooled in (False, True):
        if pooled:
            eng.enable_decode_pool(slots=64)
            base = m.generate_many(kws[:3])
        try:
            outs = [m.generate_many(batch)] + ([m.generate_many_async(batch).result()] if pooled else [])
        finally:
            if pooled:
                eng.disable_decode_pool()
        for res in outs:
            assert torch.is_tensor(res[0]) and torch.equal(res[0], base[0])
            assert isinstance(res[1], GenerateLogprobsOutput) and isinstance(res[2], GenerateLogprobsOutput)
            assert torch.equal(res[1].sequences, base[1]) and torch.equal(res[2].sequences, base[2])
            assert tuple(res[1].logprobs.shape) == (1, 6) and tuple(res[1].top_ids.shape) == (1, 6, 2) and tuple(res[2].top_ids.shape) == (1, 6, 0)
            assert res[1].top_ids[0, :, 0].tolist() == base[1][0, kws[1]["inputs"].shape[1]:].tolist()
