"""Token guides in the decode loops (vlm_fo1_amd.llm: GuideTables, the per-slot guide table and automaton states, the guided general head
fo1_decode_head_guided_accept) on the tiny engine of tests/test_batched_decode_gpu.py: 8 sequences, 16 tokens, a 64-slot
pool.  The tiny vocabulary has no <ground> tokens: seven arbitrary distinct ids stand for the structural and region ids, and the guides are
built from what the unconstrained run emits, so that they bite.

  * every recorded id of a guided greedy / sampled / sampled + penalised sequence is allowed in the state the host replays from the recorded
    ids, and equals the oracle on THAT step's logits (greedy rows exactly, sampled rows inside the accept rule, exact draws the oracle's id);
  * a region_answer sequence forced through a whole structure emits a string the grammar accepts, with no region id at or beyond n_regions;
  * a ban_sequences guide built from bigrams the plain run emits: none of them occurs in the guided run, one word starting in the prompt;
  * plain neighbours are bitwise those of an all-plain pool; graph == eager — the test of the rollback: the first replayed step starts from
    the state join() set, not from the warm-up's; slot 0 alone == slot 37 among neighbours;
  * after the last guided sequence is harvested the step key is graph_key(bucket) and no mask or guide row has users; a slot a guided
    sequence left and a plain one reuses gives the plain ids;
  * a submission without table room fails a bare join and waits in PoolService;
  * pool direct, generate_batch and PoolHandle.result() agree; the BatchDecoder's graph and eager paths agree and keep to the guides;
  * generate(guide=g) at the plug-in returns only allowed ids (the parent swallowed the keyword and returned the unconstrained ids)."""
import numpy as np
import pytest
import torch

import constraint_cases as C
import guide_cases as G
import penalty_cases as P
import sampling_cases as S
import test_constraint_decode_gpu as D

pytestmark = pytest.mark.gpu

N_SEQ, N_TOK, SEED, PEN = D.N_SEQ, D.N_TOK, 0x6b1de5eed, 1.3
T, TOP_K = D.T, D.TOP_K


def _run(f, sel, per, first, graph=True, **kw):
    out = D._run(f, sel, per, first, graph=graph, **kw)
    assert f.pool.n_guided == 0 and (f.pool.gtab is None or f.pool.gtab.users() == 0)
    return out


@pytest.fixture(scope="module")
def fx():
    from test_batched_decode_gpu import build
    from test_batched_prefill_gpu import make_request
    from vlm_fo1_amd import guide as TG
    from vlm_fo1_amd.llm import DecodePool
    f = D._Fx()
    _, _, f.eng = build()
    f.reqs = [make_request(400 + i, 96 + 28 * (i % 3), 120 + 28 * (i % 2), 1 + (3 * i) % 5) for i in range(N_SEQ)]
    f.V = f.eng.cfg.llm.vocab_size
    D._prefill(f)
    f.logits0 = f.eng._last_logits[:N_SEQ].clone()
    f.first_greedy = f.eng._last_next_tokens[:N_SEQ].clone()
    f.pool = DecodePool(f.eng.llm, slots=64)
    f.plain = _run(f, list(range(N_SEQ)), None, f.first_greedy)
    em = sorted({t for ids in f.plain for t in ids})
    # The answer language over seven ids.  <ground>, </ground> and </objects> are the three ids the plain runs emit most often (the tiny model
    # repeats itself: their logits are high at every step), the rest ids they never emit.  Sequence 1's allow-list leaves it the seven ids and
    # ONE label token: every other id of its plain run is banned in OUT — the guide bites.  The tiny model likes to repeat its last token, which
    # would keep a label or a region list open for ever; a repetition penalty of 100 takes a token out of the race once it has been emitted.
    # Which of the frequent ids then wins in LABEL and OBJ is the model's business: the fixture tries the assignments of </ground> and
    # </objects> to frequent ids in a fixed order and keeps the first under which sequence 1 closes a structure (the model is deterministic:
    # the same one every run).
    import itertools
    flat = [t for ids in f.plain for t in ids]
    freq = sorted(set(flat) - set(f.reqs[1]["ids"]), key=lambda t: (-f.plain[1].count(t), -flat.count(t), t))[:5]
    spare = [t for t in range(100, f.V) if t not in em][:7]
    f.n_regions = 2
    for ge, oe in itertools.permutations(freq, 2):
        ground = [t for t in freq if t not in (ge, oe)][0]
        f.ids7 = dict(ground=ground, ground_end=ge, objects=spare[0], objects_end=oe, region=spare[1:4], stops=spare[4:5])
        f.struct = [ground, ge, spare[0], oe] + spare[1:4]
        f.region = TG.region_answer(f.V, *f.struct[:4], spare[1:4], f.n_regions, spare[4:5])
        f.forced = sorted(f.struct + [spare[5]])      # what sequence 1 may emit at all: the structure and one label token
        sp1 = dict(greedy=True, guide=f.region, allow=f.forced, repetition_penalty=100.0, stream=1)
        D._prefill(f)
        first = f.eng._first_tokens([dict(sp1) if b == 1 else None for b in range(N_SEQ)], f.reqs).clone()
        got = _run(f, [1], {1: sp1}, first)[0]
        if oe in got:
            break
    else:
        raise AssertionError("no assignment of the structural ids lets the tiny model close a structure")
    f.region3 = TG.region_answer(f.V, *f.struct[:4], spare[1:4], 3, spare[4:5])
    common = [f.ids7["ground"]]
    others = [t for t in em if t not in f.struct]      # what the plain runs emit besides
    # bigrams the plain runs emit (sequences 2, 3 and 6), and for sequence 6 a word whose first token ends its prompt
    f.bigrams = {b: sorted({(f.plain[b][t], f.plain[b][t + 1]) for t in range(N_TOK - 1)}) for b in (2, 3, 6)}
    w6 = [list(w) for w in f.bigrams[6]] + [[f.reqs[6]["ids"][-1], f.plain[6][0]], [f.reqs[6]["ids"][-2], f.reqs[6]["ids"][-1], f.plain[6][0]]]
    f.words = {2: [list(w) for w in f.bigrams[2]], 3: [list(w) for w in f.bigrams[3]] + [[f.plain[3][0]]], 6: w6}
    f.seq = {b: TG.ban_sequences(f.words[b], f.V) for b in (2, 3, 6)}
    samp = dict(temperature=T, top_p=1.0, top_k=TOP_K, seed=SEED)
    f.per = [None,
             dict(greedy=True, guide=f.region, allow=f.forced, repetition_penalty=100.0),
             dict(greedy=True, guide=f.seq[2]),
             dict(samp, guide=f.seq[3], repetition_penalty=PEN),
             None,
             dict(samp, guide=f.region3, ban=others[:40]),
             dict(samp, guide=f.seq[6]),
             dict(greedy=True, guide=f.region, ban=others, ban_first=[common[0]])]
    f.per = [None if sp is None else dict(sp, stream=b) for b, sp in enumerate(f.per)]
    D._prefill(f)
    f.first = f.eng._first_tokens([None if sp is None else dict(sp) for sp in f.per], f.reqs).clone()
    return f


def _mixed(f):
    if not hasattr(f, "mixed_ids"):
        D._prefill(f)
        f.mixed_ids = _run(f, list(range(N_SEQ)), f.per, f.first)
    return f.mixed_ids


def _own_bans(sp: dict, V: int, t: int) -> set:
    a = set(sp.get("ban") or [])
    if sp.get("allow") is not None:
        a |= set(range(V)) - set(sp["allow"])
    if t == 0:
        a |= set(sp.get("ban_first") or [])
    return a


def _check_ids(f, ids, logits):
    """Every recorded id against the oracle on its step's logits, in the state replayed on the host from the recorded ids."""
    n_exact = n_draws = 0
    for b in range(N_SEQ):
        sp = f.per[b]
        if sp is None:
            assert ids[b] == f.plain[b]
            continue
        g = sp["guide"]
        s = g.run(f.reqs[b]["ids"]) if g.from_prompt else g.start
        pen = sp.get("repetition_penalty", 0.0)
        seen = [t for t in f.reqs[b]["ids"] if 0 <= t < f.V]
        for t in range(N_TOK):
            banned = sorted(set(np.nonzero(g.banned_mask(s))[0].tolist()) | _own_bans(sp, f.V, t))
            assert ids[b][t] not in banned, (b, t, s, ids[b][t])
            rb = C.ruled(D._bits(logits[t][b]), banned, seen, pen)
            if sp.get("greedy"):
                assert ids[b][t] == P.greedy_pick(rb), (b, t, ids[b][t], P.greedy_pick(rb))
            else:
                o, u = S.oracle(rb, T, 1.0, TOP_K), S.draw_u(t, b, SEED)
                assert S.accepts(o, u, ids[b][t]), (b, t, u, ids[b][t], S.pick(o, u))
                n_draws += 1
                if S.is_exact(o, u):
                    n_exact += 1
                    assert ids[b][t] == S.pick(o, u), (b, t, u)
            s = g.advance(s, ids[b][t])
            seen.append(ids[b][t])
    assert n_draws == 3 * N_TOK and n_exact >= n_draws // 2


def test_every_id_is_allowed_in_the_replayed_state_and_equals_the_oracle(fx):
    f = fx
    D._prefill(f)
    slots = D._join(f, list(range(N_SEQ)), f.per, f.first)
    pool = f.pool
    assert pool.n_general == 6 and pool.n_guided == 6 and pool.gtab is not None and pool.gtab.users() == 6
    # equal guides share their entry (sequences 1 and 7 differ in their own bans: two entries, one class row, one transition span); the
    # two n_regions share the class row too; states with equal banned sets share mask rows
    assert len(pool.gtab.live) == 6 and sum(u > 0 for _, _, u in pool.gtab._cls.ent.values()) == 4
    assert sum(pool.masks.users) > sum(u > 0 for u in pool.masks.users)
    tables = [t.clone() for t in (pool.masks.table, pool.rules, pool.gtab.cls, pool.gtab.next, pool.gtab.state_row, pool.guides)]
    logits = [f.logits0]
    for _ in range(N_TOK - 1):
        logits.append(pool.step(use_graph=True)[slots].clone())
    assert any("guided" in k for k in pool._graphs)
    for t0, t1 in zip(tables, (pool.masks.table, pool.rules, pool.gtab.cls, pool.gtab.next, pool.gtab.state_row, pool.guides)):
        assert torch.equal(t0, t1), "a step wrote a table other than the automaton states"
    got = {tag[1]: ids for _, tag, ids in pool.harvest(pool.snapshot())}
    ids = [got[b] for b in range(N_SEQ)]
    assert [len(r) for r in ids] == [N_TOK] * N_SEQ and [r[0] for r in ids] == f.first.cpu().tolist()
    _check_ids(f, ids, logits)
    assert ids == _mixed(f), "the same submission decoded differently the second time"


def test_a_forced_structure_is_one_the_grammar_accepts(fx):
    f = fx
    ids = _mixed(f)[1]
    i7 = f.ids7
    gr = G.Grammar(f.V, i7["ground"], i7["ground_end"], i7["objects"], i7["objects_end"], i7["region"], f.n_regions, i7["stops"])
    assert ids != f.plain[1] and set(ids) <= set(f.forced)
    for t in range(N_TOK):
        assert ids[t] in gr.allowed(ids[:t]), (t, ids)
    assert i7["region"][2] not in ids and i7["objects"] in ids and i7["objects_end"] in ids and any(r in ids for r in i7["region"][:2]), ids
    # cut to its last complete structure the string passes the plug-in's own parsers (max_new_tokens may cut an answer short: DESIGN.md)
    done = max(t + 1 for t in range(N_TOK) if ids[t] == i7["objects_end"])
    assert gr.state(ids[:done]) == "OUT" and "<objects>" in gr.text(ids[:done])
    assert G.well_formed(gr.text(ids[:done]), f.n_regions), gr.text(ids[:done])
    assert not G.well_formed(gr.text(ids[:done - 1]), f.n_regions), "an <objects> that never closes does not parse"
    # sequence 7: <ground> banned at the first token only, every other id of the plain runs banned throughout
    ids7 = _mixed(f)[7]
    assert ids7[0] != i7["ground"] and all(ids7[t] in gr.allowed(ids7[:t]) for t in range(N_TOK))
    assert not set(ids7) & (set(f.per[7]["ban"]))
    # sequence 5 (sampled, three regions allowed): the grammar of n_regions = 3
    gr3 = G.Grammar(f.V, i7["ground"], i7["ground_end"], i7["objects"], i7["objects_end"], i7["region"], 3, i7["stops"])
    ids5 = _mixed(f)[5]
    assert all(ids5[t] in gr3.allowed(ids5[:t]) for t in range(N_TOK))


def test_banned_bigrams_never_occur_and_a_word_may_start_in_the_prompt(fx):
    f = fx
    mixed = _mixed(f)
    for b in (2, 3, 6):
        hist = list(f.reqs[b]["ids"]) + mixed[b]
        L = len(f.reqs[b]["ids"])
        for w in f.words[b]:
            for e in range(L, len(hist)):      # no word ends at a generated position
                assert hist[e - len(w) + 1:e + 1] != w, (b, w, e - L)
        assert mixed[b] != f.plain[b]
    assert mixed[6][0] != f.plain[6][0], "the word whose prefix ends the prompt did not ban the first token"
    assert mixed[3][0] != f.plain[3][0]


def test_plain_neighbours_graph_eager_slot_key_and_reuse(fx):
    f = fx
    pool = f.pool
    mixed = _mixed(f)
    assert mixed[0] == f.plain[0] and mixed[4] == f.plain[4], "a plain greedy sequence changed beside guided neighbours"
    assert all(mixed[b] != f.plain[b] for b in (1, 2, 3, 5, 6, 7)), "a guide changed nothing"
    # graph == eager, with the graphs captured afresh: the warm-up step advances the automaton states and must be rolled back
    pool._graphs.clear()
    D._prefill(f)
    assert _run(f, list(range(N_SEQ)), f.per, f.first, graph=True) == mixed
    D._prefill(f)
    assert _run(f, list(range(N_SEQ)), f.per, f.first, graph=False) == mixed, "eager and graph-replayed steps differ"
    for b in (1, 3, 6):
        pool._graphs.clear()
        assert _run(f, [b], f.per, f.first) == [mixed[b]], f"sequence {b} decodes differently alone in slot 0"
    pool.free = list(range(37, 64))      # slot 37 with 7 neighbours behind it
    try:
        order = [6, 0, 1, 3, 4, 5, 2, 7]
        slots = D._join(f, order, f.per, f.first)
        assert slots[0] == 37
        got = {tag[1]: ids for _, tag, ids in pool.drain(use_graph=True, poll=5)}
    finally:
        pool.free = list(range(64))
    assert [got[b] for b in range(N_SEQ)] == mixed, "ids depend on the slot"
    # the last guided sequence harvested: today's key, no users; slot 0, left by a guided sequence, reused by a plain one
    assert pool.n_guided == 0 and pool.gtab.users() == 0 and not pool.gtab.live and not any(pool.masks.users)
    D._join(f, [1], f.per, f.first, budget=3)
    assert pool.guided_dev[0] and "guided" in pool.step_key(pool.kv_bucket())
    for _ in range(3):
        pool.step()
    assert [tag[1] for _, tag, _ in pool.harvest(pool.snapshot())] == [1] and not any(pool.masks.users) and pool.gtab.users() == 0
    assert pool.step_key(pool.kv_bucket()) == pool.graph_key(pool.kv_bucket())
    slots = D._join(f, [0, 4], None, f.first_greedy)
    assert slots == [0, 1] and not pool.guided_dev[0] and pool.guides[0].tolist() == [-1, 0, 0, 0]
    pool._graphs.clear()
    pool.step()
    assert list(pool._graphs) == [pool.graph_key(pool.kv_bucket())]
    got = {tag[1]: ids for _, tag, ids in pool.drain(poll=4)}
    assert [got[0], got[4]] == [f.plain[0], f.plain[4]]
    # guided sequences in reused slots, the other way round
    assert _run(f, [3, 1], f.per, f.first) == [mixed[3], mixed[1]]


def test_without_table_room_a_bare_join_fails_and_the_service_waits(fx):
    from vlm_fo1_amd import guide as TG
    from vlm_fo1_amd.serving import PoolHandle, PoolService
    f = fx
    pool = f.pool
    D._prefill(f)
    # guides with distinct state bitmaps: 2-state guides that ban one id in state 0 and another in state 1 -> 2 mask rows each
    def two(j):
        cls = np.zeros(f.V, np.uint16)
        cls[[10 + 2 * j, 11 + 2 * j]] = [1, 2]
        return TG.TokenGuide(cls, np.array([[1, -1, 1], [0, 0, -1]], np.int32), 0, f.V)
    per = lambda j0, n: {b: dict(greedy=True, guide=two(j0 + b), stream=b) for b in range(n)}      # noqa: E731
    for j0 in range(0, 32, 8):
        D._join(f, list(range(8)), per(j0, 8), f.first_greedy)
    assert sum(u > 0 for u in pool.masks.users) == pool.MAX_MASKS == 64 and len(pool.live) == 32 and pool.n_guided == 32
    new, old = [dict(greedy=True, guide=two(40))], [dict(greedy=True, guide=two(3))]
    assert not pool.can_take((), new, 1) and pool.can_take((), old, 1) and pool.can_take(())
    free = list(pool.free)
    with pytest.raises(RuntimeError, match="wait for sequences to finish"):
        D._join(f, [0], {0: new[0]}, f.first_greedy)
    assert pool.free == free and len(pool.live) == 32 and pool.gtab.users() == 32
    h = PoolHandle(1)
    ev = torch.cuda.Event()
    ev.record()
    item = (h, f.eng.llm.kcache, f.eng.llm.vtcache, [f.hp["seqs"][0]], [f.hp["delta"][0]], f.first_greedy[:1], N_TOK, (), ev, new, [f.reqs[0]["ids"]], None, None)
    waiting = [item]
    svc = D._Fx()
    svc.stats = dict(joined=0)
    PoolService._admit(svc, pool, waiting)
    assert waiting == [item] and h._error is None and not h._joined.is_set()
    D._join(f, [1], {1: old[0]}, f.first_greedy)      # a guide that is live already shares everything
    assert len(pool.live) == 33 and sum(u > 0 for u in pool.masks.users) == 64
    pool.drain(poll=6)
    assert not any(pool.masks.users) and pool.gtab.users() == 0
    D._prefill(f)
    PoolService._admit(svc, pool, waiting)
    assert not waiting and h._joined.is_set() and h._error is None and pool.n_guided == 1
    pool.drain(poll=6)


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
    assert bd == eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=False, sampling=per), "BatchDecoder guided head: graph != eager"
    for b in range(N_SEQ):      # (other kernels than the pool's: the logits differ in last bits, the guides are the same)
        sp = per[b]
        if sp is None:
            continue
        g = sp["guide"]
        s = g.run(f.reqs[b]["ids"]) if g.from_prompt else g.start
        for t in range(N_TOK):
            assert not g.banned_mask(s)[bd[b][t]] and bd[b][t] not in _own_bans(sp, f.V, t), (b, t)
            s = g.advance(s, bd[b][t])


def test_plug_in_generate_with_a_guide(fx):
    from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig
    f = fx
    eng = f.eng
    m = FO1ForCausalLM.from_engine(FO1HFConfig({}, {"eos_token_id": 4095}), eng)
    kws = [dict(D._generate_kwargs(r), max_new_tokens=8) for r in f.reqs[:3]]
    L = kws[0]["inputs"].shape[1]
    plain = m.generate(**kws[0])[0, L:].tolist()
    from vlm_fo1_amd.guide import ban_sequences
    g = ban_sequences([[plain[0]], plain[1:3]], f.V)
    got = m.generate(**kws[0], guide=g)[0, L:].tolist()
    assert len(got) == 8 and got != plain and got[0] != plain[0], "the guide was ignored"
    s = g.run(f.reqs[0]["ids"])
    for t in got:
        assert not g.banned_mask(s)[t]
        s = g.advance(s, t)
    st = D._Collect()      # with a streamer: a BatchDecoder of one, the same ids
    assert m.generate(**kws[0], guide=g, streamer=st)[0, L:].tolist() == got and st.ended
    with pytest.raises(ValueError, match="TokenGuide"):
        m.generate(**kws[0], guide="regions")
    batch = [kws[0], dict(kws[1], guide=g), dict(kws[2], guide=f.region, allowed_token_ids=f.forced)]
    with pytest.raises(ValueError, match="unless the decode pool is enabled"):
        m.generate_many(batch)
    eng.enable_decode_pool(slots=64)
    try:
        out = m.generate_many(batch)
        assert out[0][0, L:].tolist() == plain
        new2 = out[2][0, kws[2]["inputs"].shape[1]:].tolist()
        assert set(new2) <= set(f.forced) and new2 != m.generate(**kws[2])[0, kws[2]["inputs"].shape[1]:].tolist()
    finally:
        eng.disable_decode_pool()
