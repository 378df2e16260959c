"""Per-request logit bias and frequency / presence penalties in the decode loops (vlm_fo1_amd.llm: BiasTable, the per-slot steer table and
count rows, the steered general head fo1_decode_head_steered_accept) on the tiny engine of
tests/test_batched_decode_gpu.py: 8 sequences, 24 tokens, a 64-slot pool.

  * every id of a steered greedy / sampled / penalised / constrained sequence is the definition's (tests/steer_cases.py) on THAT step's logits
    with the host's running counts and seen set: greedy rows exactly, sampled rows inside the accept rule, exact draws equal to the oracle's;
  * two properties the parent fails: a large presence penalty on a greedy request yields no repeated id within the budget, and a logit_bias
    of +B (B = twice the finite range of the first step's logits) on a non-argmax id makes it the first generated id;
  * plain greedy neighbours' ids are bitwise those of an all-plain pool; graph == eager; slot 0 alone == slot 37 among neighbours;
  * after the last steered sequence is harvested the step key is graph_key(bucket), no bias row has users, and alternating steered and plain
    submissions captures no further graph; a slot reused after a counting sequence starts from zero counts;
  * a 17th distinct bias fails a bare join with a RuntimeError and waits in PoolService._admit, then completes;
  * pool direct, generate_batch and PoolHandle.result() agree bit for bit; so do the BatchDecoder's graph and eager paths and the streamer
    loop; the plug-in's keywords reach the device."""
import numpy as np
import pytest
import torch

import penalty_cases as P
import sampling_cases as S
import steer_cases as ST

pytestmark = pytest.mark.gpu

N_SEQ, N_TOK, SEED, PEN = 8, 24, 0x57ee7ab1e5eed, 1.3
T, TOP_K = 0.7, 50
PRESENCE = 64.0


class _Fx:
    pass


def _join(f, sel, per, first, budget=N_TOK, stop=()):
    pool, eng = f.pool, f.eng
    return pool.join(eng.llm.kcache, eng.llm.vtcache, [f.hp["seqs"][b] for b in sel], [f.hp["delta"][b] for b in sel],
                     torch.stack([first[b] for b in sel]), budget, stop, tags=[("t", b) for b in sel],
                     sampling=None if per is None else [per[b] for b in sel], prompt_ids=[f.reqs[b]["ids"] for b in sel])


def _run(f, sel, per, first, graph=True, **kw):
    _join(f, sel, per, first, **kw)
    got = {tag[1]: ids for _, tag, ids in f.pool.drain(use_graph=graph, poll=5)}
    assert not f.pool.live and len(f.pool.free) == f.pool.P and f.pool.n_general == 0 and f.pool.n_steered == 0
    assert f.pool.btab is None or not any(f.pool.btab.users)
    return [got[b] for b in sel]


def _prefill(f):
    """The requests' K / V^T rows back into the engine's prefill cache (another test's generate calls overwrite it)."""
    f.eng.prefill_batch(f.reqs, use_graph=False)
    f.hp = f.eng._last_batch


def _bits(row: torch.Tensor) -> np.ndarray:
    return row.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def fx():
    from test_batched_decode_gpu import build
    from test_batched_prefill_gpu import make_request
    from vlm_fo1_amd.llm import DecodePool
    f = _Fx()
    _, _, f.eng = build()
    f.reqs = [make_request(400 + i, 96 + 28 * (i % 3), 120 + 28 * (i % 2), 1 + (3 * i) % 5) for i in range(N_SEQ)]
    f.V = f.eng.cfg.llm.vocab_size
    _prefill(f)
    f.logits0 = f.eng._last_logits[:N_SEQ].clone()
    f.first_greedy = f.eng._last_next_tokens[:N_SEQ].clone()
    f.pool = DecodePool(f.eng.llm, slots=64)
    f.plain = _run(f, list(range(N_SEQ)), None, f.first_greedy)
    samp = dict(temperature=T, top_p=1.0, top_k=TOP_K, seed=SEED)
    em = [sorted(set(ids)) for ids in f.plain]
    # the +B bias: a non-argmax id of row 5's first-step logits, B = twice their finite range
    x5 = S.from_bits(_bits(f.logits0[5]))
    fin = x5[np.isfinite(x5)]
    f.big = 2.0 * float(fin.max() - fin.min())
    f.target = int(np.argsort(x5)[len(x5) // 2])
    assert f.target != int(f.first_greedy[5]) and f.big > 0
    every8 = {int(i): 1.5 for i in range(0, f.V, 8)}
    f.per = [None,
             dict(greedy=True, presence_penalty=PRESENCE),
             dict(samp, bias=every8, frequency_penalty=0.25, presence_penalty=0.5),
             dict(samp, repetition_penalty=PEN, bias={t: -4.0 for t in em[3]}, frequency_penalty=0.75),
             None,
             dict(greedy=True, bias={f.target: f.big}),
             dict(samp, frequency_penalty=0.5),
             dict(greedy=True, repetition_penalty=PEN, bias=every8, presence_penalty=1.0, ban=em[1])]
    f.per = [None if sp is None else dict(sp, stream=b) for b, sp in enumerate(f.per)]
    _prefill(f)
    f.first = f.eng._first_tokens(f.per, f.reqs).clone()
    return f


def _mixed(f):
    if not hasattr(f, "mixed_ids"):
        _prefill(f)
        f.mixed_ids = _run(f, list(range(N_SEQ)), f.per, f.first)
    return f.mixed_ids


def test_every_id_is_the_definitions_on_its_steps_logits_with_the_hosts_running_counts(fx):
    f = fx
    _prefill(f)
    slots = _join(f, list(range(N_SEQ)), f.per, f.first)
    pool = f.pool
    assert pool.n_general == 6 and pool.n_steered == 6 and pool.btab is not None and pool.counts is not None
    # equal biases share a row: every8 is the bias of 2 and 7
    assert sum(pool.btab.users) == 4 and sum(u > 0 for u in pool.btab.users) == 3
    cnt0 = pool.counts[slots].cpu().numpy().view(np.uint16)
    first = f.first.cpu().tolist()
    for b in (1, 2, 3, 6, 7):      # a counting slot's row holds its first token, nothing else
        assert cnt0[b].sum() == 1 and cnt0[b, first[b]] == 1, b
    tables = (pool.btab.table.clone(), pool.btab.gate.clone(), pool.steers.clone())
    logits = [f.logits0]
    for _ in range(N_TOK - 1):
        logits.append(pool.step(use_graph=True)[slots].clone())
    assert any("steered" in k for k in pool._graphs)
    assert all(torch.equal(a, b) for a, b in zip(tables, (pool.btab.table, pool.btab.gate, pool.steers))), "a step wrote the bias table or the steers"
    cnt_dev = pool.counts[slots].cpu().numpy().view(np.uint16).astype(np.int64)
    got = {tag[1]: ids for _, tag, ids in pool.harvest(pool.snapshot())}
    ids = [got[b] for b in range(N_SEQ)]
    assert [len(r) for r in ids] == [N_TOK] * N_SEQ and [r[0] for r in ids] == first
    n_exact = n_draws = 0
    moved = [0] * N_SEQ
    for b in range(N_SEQ):
        sp = f.per[b] or {}
        pen = sp.get("repetition_penalty", 0.0)
        brow = ST.bias_bits(sp.get("bias"), f.V)
        fq = (sp.get("frequency_penalty", 0.0), sp.get("presence_penalty", 0.0))
        seen = [t for t in f.reqs[b]["ids"] if 0 <= t < f.V]
        cnt = np.zeros(f.V, np.int64)
        for t in range(N_TOK):
            raw = _bits(logits[t][b])
            sb = ST.steer(raw, brow, cnt, *fq, banned=sp.get("ban") or (), seen=seen, p=pen)
            if not f.per[b] or sp.get("greedy"):
                assert ids[b][t] == P.greedy_pick(sb), (b, t, ids[b][t], P.greedy_pick(sb))
                moved[b] += ids[b][t] != P.greedy_pick(P.penalise(raw, seen, pen))
            else:
                o, u = S.oracle(sb, T, 1.0, TOP_K), S.draw_u(t, b, SEED)
                assert S.accepts(o, u, ids[b][t]), (b, t, u, ids[b][t], S.pick(o, u))
                n_draws += 1
                if S.is_exact(o, u):
                    n_exact += 1
                    assert ids[b][t] == S.pick(o, u), (b, t, u)
            seen.append(ids[b][t])
            cnt[ids[b][t]] += 1
        if ST.count_on(*fq):      # the device's counts are the host's (the last step's pick is counted too)
            assert (cnt_dev[b, :f.V] == cnt).all(), b
    assert n_draws == 3 * N_TOK and n_exact >= n_draws // 2
    assert moved[1] >= 1 and moved[5] >= 1 and moved[7] >= 1 and moved[0] == moved[4] == 0, moved
    assert ids == _mixed(f), "the same submission decoded differently the second time"


def test_presence_penalty_stops_repeats_and_a_large_bias_picks_the_first_id(fx):
    f = fx
    mixed = _mixed(f)
    assert len(set(f.plain[1])) < N_TOK, "the plain run repeats no id: the property would show nothing"
    assert len(set(mixed[1])) == N_TOK, "a presence penalty of 64 left a repeated id"
    assert mixed[5][0] == f.target != f.plain[5][0], "a logit_bias of twice the logits' range did not pick its id"
    assert int(f.first[5]) == f.target


def test_plain_neighbours_graph_eager_slot_key_and_reused_slots(fx):
    f = fx
    pool = f.pool
    mixed = _mixed(f)
    assert mixed[0] == f.plain[0] and mixed[4] == f.plain[4], "a plain greedy sequence changed beside steered neighbours"
    assert all(mixed[b] != f.plain[b] for b in (1, 5, 7)), "a steer changed nothing"
    _prefill(f)
    assert _run(f, list(range(N_SEQ)), f.per, f.first, graph=False) == mixed, "eager and graph-replayed steps differ"
    for b in (1, 2, 3, 7):      # alone in slot 0 — which a counting sequence has just left: its count row starts from zero again
        assert _run(f, [b], f.per, f.first) == [mixed[b]], f"sequence {b} decodes differently alone in slot 0"
    pool.free = list(range(37, 64))      # slot 37 with 7 neighbours behind it
    try:
        order = [2, 0, 1, 3, 4, 5, 6, 7]
        slots = _join(f, order, f.per, f.first)
        assert slots[0] == 37
        got = {tag[1]: ids for _, tag, ids in pool.drain(use_graph=True, poll=5)}
    finally:
        pool.free = list(range(64))
    assert [got[b] for b in range(N_SEQ)] == mixed, "ids depend on the slot"
    # the last steered sequence harvested: today's key, no users; slot 0, left by a steered sequence, reused by a plain one
    assert pool.n_steered == 0 and not any(pool.btab.users)
    _join(f, [1], f.per, f.first, budget=3)
    assert pool.steer_dev[0] and "steered" in pool.step_key(pool.kv_bucket())
    for _ in range(3):
        pool.step()
    assert [tag[1] for _, tag, _ in pool.harvest(pool.snapshot())] == [1]
    assert pool.step_key(pool.kv_bucket()) == pool.graph_key(pool.kv_bucket())
    slots = _join(f, [0, 4], None, f.first_greedy)
    assert slots == [0, 1] and not pool.steer_dev[0] and pool.steers[0].tolist()[0] == -1
    got = {tag[1]: ids for _, tag, ids in pool.drain(poll=4)}
    assert [got[0], got[4]] == [f.plain[0], f.plain[4]]
    # steered and plain submissions alternating: the graphs captured so far serve them all
    n_graphs = len(pool._graphs)
    for _ in range(2):
        assert _run(f, [5, 1], f.per, f.first) == [mixed[5], mixed[1]]
        assert _run(f, [0, 4], None, f.first_greedy) == [f.plain[0], f.plain[4]]
    assert len(pool._graphs) == n_graphs, "alternating steered and plain submissions captured another graph"


def test_a_17th_distinct_bias_fails_a_bare_join_and_waits_in_the_service(fx):
    from vlm_fo1_amd.serving import PoolHandle, PoolService
    f = fx
    pool = f.pool
    _prefill(f)
    per = lambda j, n: {b: dict(greedy=True, bias={100 + 8 * j + b: 2.0}, stream=b) for b in range(n)}      # noqa: E731
    _join(f, list(range(8)), per(0, 8), f.first_greedy)
    _join(f, list(range(8)), per(1, 8), f.first_greedy)
    assert sum(u > 0 for u in pool.btab.users) == pool.MAX_BIAS == 16 and len(pool.live) == 16
    new, old = [dict(greedy=True, bias={3000: 2.0})], [dict(greedy=True, bias={100: 2.0})]
    counted = [dict(greedy=True, presence_penalty=1.0)]      # (a count penalty takes no bias row)
    assert not pool.can_take((), new, 1) and pool.can_take((), old, 1) and pool.can_take((), counted, 1) and pool.can_take((), None, 1)
    free = list(pool.free)
    with pytest.raises(RuntimeError, match="16 different logit-bias vectors are live"):
        _join(f, [0], {0: new[0]}, f.first_greedy)
    assert pool.free == free and len(pool.live) == 16 and sum(u > 0 for u in pool.btab.users) == 16
    # the service's admission: the submission waits (no error, still queued) while the table is full, and joins once rows are free
    h = PoolHandle(1)
    ev = torch.cuda.Event()
    ev.record()
    item = (h, f.eng.llm.kcache, f.eng.llm.vtcache, [f.hp["seqs"][0]], [f.hp["delta"][0]], f.first_greedy[:1], N_TOK, (), ev, new, [f.reqs[0]["ids"]], None, None)
    waiting = [item]
    svc = _Fx()
    svc.stats = dict(joined=0)
    PoolService._admit(svc, pool, waiting)
    assert waiting == [item] and h._error is None and not h._joined.is_set()
    _join(f, [1], {1: old[0]}, f.first_greedy)      # a bias that is live already shares its row
    assert len(pool.live) == 17 and sum(u > 0 for u in pool.btab.users) == 16
    pool.drain(poll=6)
    assert not any(pool.btab.users)
    _prefill(f)
    PoolService._admit(svc, pool, waiting)
    assert not waiting and h._joined.is_set() and h._error is None and pool.n_steered == 1
    done = pool.drain(poll=6)
    assert len(done) == 1 and len(done[0][2]) == N_TOK
    # a submission that alone needs more rows than the table has can never be taken: it is admitted, and fails its own handle
    assert pool.can_take((), [dict(greedy=True, bias={i: 1.0}) for i in range(17)], 17)


def test_pool_direct_generate_batch_and_handles_agree_and_so_do_the_batch_decoders_paths(fx):
    f = fx
    eng = f.eng
    mixed = _mixed(f)
    per = [None if sp is None else {k: v for k, v in sp.items() if k != "stream"} for sp in f.per]
    eng.enable_decode_pool(slots=64)
    try:
        assert eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=per) == mixed, "the scheduler's pool gave other ids than the direct run"
        h = eng.submit_batch(f.reqs, N_TOK, (), True, sampling=per)
        assert h.result() == mixed
    finally:
        eng.disable_decode_pool()
    bd = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=per)
    assert [len(r) for r in bd] == [N_TOK] * N_SEQ and [r[0] for r in bd] == [r[0] for r in mixed]
    assert bd == eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=False, sampling=per), "BatchDecoder steered head: graph != eager"
    # (other kernels than the pool's: the logits differ in last bits, the properties are the same)
    assert len(set(bd[1])) == N_TOK and bd[5][0] == f.target
    plain = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True)
    assert all(bd[b] != plain[b] for b in (1, 5, 7)) and bd[0] == plain[0] and bd[4] == plain[4]
    # a second start() of the same decoder: its count rows start from zero again
    assert eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True, sampling=per) == bd


def _generate_kwargs(r):
    gh, gw = r["grid"]
    return dict(inputs=torch.tensor([r["ids"]]), images=[r["pix"]], images_aux=[r["aux"]], image_grid_thws=[torch.tensor([[1, gh, gw]])],
                bbox_list=[r["boxes"]])


class _Collect:
    def __init__(self):
        self.parts, self.ended = [], False

    def put(self, t):
        self.parts.append(t)

    def end(self):
        self.ended = True


def test_plug_in_keywords(fx):
    from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig
    f = fx
    eng = f.eng
    m = FO1ForCausalLM.from_engine(FO1HFConfig({}, {"eos_token_id": 4095}), eng)
    kws = [dict(_generate_kwargs(r), max_new_tokens=N_TOK) for r in f.reqs[:4]]
    L = kws[0]["inputs"].shape[1]
    plain = m.generate(**kws[0])[0, L:].tolist()
    x0 = S.from_bits(_bits(f.logits0[0]))
    fin = x0[np.isfinite(x0)]
    big, target = 2.0 * float(fin.max() - fin.min()), int(np.argsort(x0)[len(x0) // 3])
    assert target != plain[0]
    got = m.generate(**kws[0], logit_bias={target: big})[0, L:].tolist()
    assert got[0] == target, "logit_bias was ignored"
    assert m.generate(**kws[0], sequence_bias={(target,): big})[0, L:].tolist() == got
    assert m.generate(**kws[0], sequence_bias=[[[target], big / 2]], logit_bias={str(target): big / 2})[0, L:].tolist() == got
    assert len(set(plain)) < N_TOK
    pres = m.generate(**kws[0], presence_penalty=PRESENCE)[0, L:].tolist()
    assert len(pres) == N_TOK and len(set(pres)) == N_TOK, "presence_penalty was ignored"
    freq = m.generate(**kws[0], frequency_penalty=PRESENCE)[0, L:].tolist()
    assert len(set(freq)) == N_TOK
    st = _Collect()      # with a streamer: a BatchDecoder of one, the same ids
    assert m.generate(**kws[0], presence_penalty=PRESENCE, streamer=st)[0, L:].tolist() == pres and st.ended
    assert m.generate(**kws[0], logit_bias={}, frequency_penalty=0, presence_penalty=None)[0, L:].tolist() == plain
    with pytest.raises(ValueError, match="outside"):
        m.generate(**kws[0], logit_bias={f.V: 1.0})
    with pytest.raises(NotImplementedError, match="single-token"):
        m.generate(**kws[0], sequence_bias={(1, 2): 1.0})
    with pytest.raises(ValueError, match="finite"):
        m.generate(**kws[0], presence_penalty=float("nan"))
    with pytest.raises(ValueError, match="draws at most"):
        m.generate(**dict(kws[0], max_new_tokens=5000), presence_penalty=1.0)
    # a batch mixed in the new keywords: refused without the pool, taken with it
    xs = S.from_bits(_bits(f.logits0[:4]))
    big_all = 2.0 * float(xs[np.isfinite(xs)].max() - xs[np.isfinite(xs)].min())      # (at least twice the range of any of the four rows)
    batch = [kws[0], dict(kws[1], logit_bias={target: big_all}), dict(kws[2], presence_penalty=PRESENCE), dict(kws[3], frequency_penalty=0.5, do_sample=True,
                                                                                                       temperature=T, seed=7)]
    with pytest.raises(ValueError, match="steering keywords"):
        m.generate_many(batch)
    same = m.generate_many([dict(k, presence_penalty=PRESENCE) for k in kws[:3]])      # a uniform steered batch needs no pool
    # (three sequences step through other GEMV kernels than one: last-bit differences of the logits may pick another of two near-equal
    # tokens late in the run — the property is what the batch shares with the single generation)
    for k, o in zip(kws[:3], same):
        new = o[0, k["inputs"].shape[1]:].tolist()
        assert len(new) == N_TOK and len(set(new)) == N_TOK
    assert same[0][0, L:L + 8].tolist() == pres[:8]
    eng.enable_decode_pool(slots=64)
    try:
        out = m.generate_many(batch)
        assert [tuple(o.shape) for o in out] == [(1, k["inputs"].shape[1] + N_TOK) for k in kws]
        assert out[0][0, L:L + 8].tolist() == plain[:8]      # (the pool's kernels against the single-sequence step's: see above)
        assert out[0].tolist() == m.generate_many(kws)[0].tolist(), "a plain request changed beside steered ones"      # (pool against pool: bitwise)
        assert out[1][0, kws[1]["inputs"].shape[1]] == target
        new2 = out[2][0, kws[2]["inputs"].shape[1]:].tolist()
        assert len(set(new2)) == N_TOK
        assert [o.tolist() for o in m.generate_many_async(batch).result()] == [o.tolist() for o in out]
    finally:
        eng.disable_decode_pool()
