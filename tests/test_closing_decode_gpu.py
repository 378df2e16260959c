"""Budget-aware token guides in the decode loops (vlm_fo1_amd.llm: the closing plans, GuideTables' close_row spans, the per-row / per-slot
fo1_guide_close_t tables, the closing head fo1_decode_head_closing_accept; FO1Engine._first_tokens' closing pick) on the
tiny engine of tests/test_batched_decode_gpu.py with a 64-slot pool.  The tiny vocabulary has no <ground> tokens: `<ground>` is the id a
sequence's prefill likes best, so that a greedy sequence opens a structure with its first token whenever the budget lets it, and the closing
tokens are ids the model never emits, so that nothing but the closing rule ever closes one.

  * budgets 1..12, greedy and sampled sequences, through the pool and the BatchDecoder, graph and eager: every answer is well-formed text,
    the host replay of the ids ends in OUT and equals the device's final state, every id is allowed at its (state, tokens left), every budget
    has picks at which the closing set differed from the plain one, and a greedy sequence with 6 or more tokens opens and closes a structure;
    the same guides without accepting states leave answers open (the control);
  * closing, guided, ruled and plain sequences in one pool: the plain one's ids are those of an all-greedy pool; after the harvest the step
    key is today's; a slot a closing sequence left gets depth = 0 back;
  * max_new_tokens below the start state's distance is a ValueError at join(), start() and generate_batch();
  * without mask rows or close_row room a bare join raises RuntimeError and PoolService waits;
  * generate(guide=region_guide(tok, n, close=True), max_new_tokens=k) at the plug-in gives the engine path's ids, with and without a streamer."""
import numpy as np
import pytest
import torch

import closing_cases as K
import guide_cases as G
import test_constraint_decode_gpu as D

pytestmark = pytest.mark.gpu

N_SEQ = D.N_SEQ
BUDGETS = tuple(range(1, 13))
SEED = 0xc105ed
N_REGIONS = 2


@pytest.fixture(scope="module")
def fx():
    from test_batched_decode_gpu import build
    from test_batched_prefill_gpu import make_request
    from vlm_fo1_amd.llm import DecodePool
    f = D._Fx()
    _, _, f.eng = build()
    f.reqs = [make_request(400 + i, 96 + 28 * (i % 3), 120 + 28 * (i % 2), 1 + (3 * i) % 5) for i in range(N_SEQ)]
    f.V = f.eng.cfg.llm.vocab_size
    D._prefill(f)
    f.first_greedy = f.eng._last_next_tokens[:N_SEQ].clone()
    f.pool = DecodePool(f.eng.llm, slots=64)
    f.plain = D._run(f, list(range(N_SEQ)), None, f.first_greedy)
    em = {t for ids in f.plain for t in ids}
    spare = [t for t in range(100, f.V - 1) if t not in em][:6]      # ids no plain run emits: </ground>, <objects>, </objects>, 3 x <regionK>
    fg = f.first_greedy.cpu().tolist()
    # sequences b and b + 4 share the guide whose <ground> is sequence b's favourite first token: at most 4 distinct guides, 9 mask rows each
    f.ids = [dict(ground=fg[b % 4], ground_end=spare[0], objects=spare[1], objects_end=spare[2], region=spare[3:6], stops=[f.V - 1]) for b in range(N_SEQ)]
    f.guide = [K.region_guide(N_REGIONS, close=True, V=f.V, ids=i) for i in f.ids]
    f.open_guide = [K.region_guide(N_REGIONS, close=False, V=f.V, ids=i) for i in f.ids]
    f.grammar = [G.Grammar(f.V, i["ground"], i["ground_end"], i["objects"], i["objects_end"], i["region"], N_REGIONS, i["stops"]) for i in f.ids]
    samp = dict(temperature=D.T, top_p=1.0, top_k=D.TOP_K, seed=SEED)
    f.mk = lambda guides: [dict(greedy=True, guide=guides[b], stream=b) if b < 4 else dict(samp, guide=guides[b], stream=b) for b in range(N_SEQ)]      # noqa: E731
    return f


def _first(f, per, budget):
    """The prefill again (another run's generate calls overwrite its cache) and the first tokens under `budget` -> (first, per with the state words)."""
    D._prefill(f)
    per = [dict(sp) for sp in per]
    return f.eng._first_tokens(per, f.reqs, budget).clone(), per


def _pool_run(f, guides, budgets, graph):
    """One join per budget, all in the pool together, drained -> {budget: (ids per sequence, final device states)}."""
    pool = f.pool
    slots = {}
    for n in budgets:
        first, per = _first(f, f.mk(guides), n)
        slots[n] = pool.join(f.eng.llm.kcache, f.eng.llm.vtcache, f.hp["seqs"], f.hp["delta"], first, n, (), tags=[(n, b) for b in range(N_SEQ)],
                             sampling=per, prompt_ids=[r["ids"] for r in f.reqs])
    closing = guides[0].accept is not None
    assert pool.n_closing == (len(budgets) * N_SEQ if closing else 0) and pool.n_guided == len(budgets) * N_SEQ
    assert ("closing" in pool.step_key(pool.kv_bucket())) == closing
    got = {tag: ids for _, tag, ids in pool.drain(use_graph=graph, poll=4)}
    states = pool.gstate.cpu().tolist()
    assert pool.n_closing == 0 and pool.n_guided == 0 and pool.gtab.users() == 0 and not any(pool.masks.users)
    assert pool.step_key(pool.kv_bucket()) == pool.graph_key(pool.kv_bucket())
    return {n: ([got[(n, b)] for b in range(N_SEQ)], [states[s] for s in slots[n]]) for n in budgets}


def _decoder_run(f, guides, budgets, graph):
    dec = f.eng._decoder()
    out = {}
    for n in budgets:
        first, per = _first(f, f.mk(guides), n)
        dec.start(f.hp["seqs"], f.hp["delta"], first, n, (), sampling=per, prompt_ids=[r["ids"] for r in f.reqs])
        assert dec.closing == (guides[0].accept is not None) and dec.guided
        ids = dec.run(n, use_graph=graph)
        out[n] = (ids, dec.gstate[:N_SEQ].cpu().tolist())
    return out


def _check(f, res, budgets):
    """The definition, replayed on the host: every id allowed at its (state, tokens left); the final state OUT and the device's; the text
    well-formed; per budget at least one pick whose closing set differed from the plain set; greedy rows open a structure when one fits."""
    structures = 0
    for n in budgets:
        ids, states = res[n]
        differed = 0
        for b in range(N_SEQ):
            g, gr, i = f.guide[b], f.grammar[b], f.ids[b]
            assert len(ids[b]) == n, (n, b, ids[b])      # no stop id is ever the pick here: the answer fills its budget
            s = g.start
            for c, t in enumerate(ids[b]):
                ok = K.allowed(g, s, n - c - 1)
                assert t in ok, (n, b, c, s, t)
                differed += len(ok) != len(K.allowed(g, s, None))
                s = g.advance(s, t)
            assert s == K.TG.OUT == states[b] and gr.state(ids[b]) == "OUT", (n, b, ids[b], s, states[b])
            assert G.well_formed(gr.text(ids[b]), N_REGIONS), (n, b, gr.text(ids[b]))
            if b < 4 and n >= 6:      # greedy: <ground> is the first logits' argmax and allowed with 5 or more tokens left
                assert ids[b][0] == i["ground"] and i["objects"] in ids[b] and i["objects_end"] in ids[b], (n, b, ids[b])
            structures += i["objects_end"] in ids[b]
        assert differed >= 1, n
    return structures


@pytest.mark.parametrize("path,graph", [("pool", True), ("pool", False), ("decoder", True), ("decoder", False)],
                         ids=["pool-graph", "pool-eager", "decoder-graph", "decoder-eager"])
def test_every_budget_closes_through_pool_and_decoder_graph_and_eager(fx, path, graph):
    f = fx
    run = _pool_run if path == "pool" else _decoder_run
    res = {}
    for part in (BUDGETS[:6], BUDGETS[6:]):      # 6 budgets x 8 sequences fill 48 of the pool's 64 slots
        res.update(run(f, f.guide, part, graph))
    structures = _check(f, res, BUDGETS)
    assert structures >= 4 * 7, structures      # the four greedy rows at budgets 6..12 at the least
    prev = getattr(f, "ids_of", {})
    if path in prev:
        assert prev[path] == {n: res[n][0] for n in BUDGETS}, "graph and eager steps differ"
    f.ids_of = {**prev, path: {n: res[n][0] for n in BUDGETS}}
    if path == "pool" and graph:      # the control: the same sequences under guides without accepting states end inside structures
        ctl = run(f, f.open_guide, (1, 4, 9), True)
        opened = sum(f.open_guide[b].run(ids) != K.TG.OUT for n in (1, 4, 9) for b, ids in enumerate(ctl[n][0]))
        assert opened >= 6, opened      # a greedy row opens with its first token, and only the model could close what it opened
        assert any(not G.well_formed(f.grammar[b].text(ids), N_REGIONS) for n in (1, 4, 9) for b, ids in enumerate(ctl[n][0]))


def test_closing_guided_ruled_and_plain_sequences_share_a_pool(fx):
    f = fx
    pool = f.pool
    per = [None,
           dict(greedy=True, guide=f.guide[1]),
           dict(greedy=True, guide=f.open_guide[2]),
           dict(greedy=True, ban=sorted(set(f.plain[3]))),
           None,
           dict(temperature=D.T, top_p=1.0, top_k=D.TOP_K, seed=SEED, guide=f.guide[5]),
           dict(greedy=True, guide=f.guide[6], ban=[f.plain[6][1]]),
           dict(greedy=True, repetition_penalty=1.3)]
    per = [None if sp is None else dict(sp, stream=b) for b, sp in enumerate(per)]
    n = 9
    first, per = _first_mixed(f, per, n)
    slots = pool.join(f.eng.llm.kcache, f.eng.llm.vtcache, f.hp["seqs"], f.hp["delta"], first, n, (), tags=[("m", b) for b in range(N_SEQ)],
                      sampling=per, prompt_ids=[r["ids"] for r in f.reqs])
    assert pool.n_closing == 3 and pool.n_guided == 4 and pool.n_ruled == 1 and pool.n_general == 6
    assert [pool.close_dev[s] for s in slots] == [False, True, False, False, False, True, True, False]
    assert pool.closes[slots[1]].tolist()[1] == 5 and pool.closes[slots[2]].tolist() == [0, 0, 0, 0]
    tables = [t.clone() for t in (pool.masks.table, pool.rules, pool.gtab.cls, pool.gtab.next, pool.gtab.state_row, pool.gtab.close_row, pool.guides,
                                  pool.closes)]
    got = {tag[1]: ids for _, tag, ids in pool.drain(use_graph=True, poll=4)}
    for t0, t1 in zip(tables, (pool.masks.table, pool.rules, pool.gtab.cls, pool.gtab.next, pool.gtab.state_row, pool.gtab.close_row, pool.guides,
                               pool.closes)):
        assert torch.equal(t0, t1), "a step wrote a table other than the automaton states"
    assert got[0] == f.plain[0][:n] and got[4] == f.plain[4][:n], "a plain greedy sequence changed beside closing neighbours"
    for b in (1, 5, 6):
        assert f.guide[b].run(got[b]) == K.TG.OUT and G.well_formed(f.grammar[b].text(got[b]), N_REGIONS), (b, got[b])
    assert f.plain[6][1] not in got[6]
    assert f.open_guide[2].run(got[2]) != K.TG.OUT      # the guided sequence without the rule opened with its first token and stays open
    assert pool.n_closing == 0 and pool.step_key(pool.kv_bucket()) == pool.graph_key(pool.kv_bucket())
    # slot of sequence 1, left by a closing sequence: a guided sequence without the rule gets depth = 0 back, and decodes as it does alone
    keep = list(pool.free)
    pool.free = [slots[1]]
    first2, per2 = _first_mixed(f, [None, None, dict(greedy=True, guide=f.open_guide[2], stream=2)] + [None] * 5, n)
    s2 = pool.join(f.eng.llm.kcache, f.eng.llm.vtcache, f.hp["seqs"][2:3], f.hp["delta"][2:3], first2[2:3], n, (), tags=[("m", 2)], sampling=per2[2:3],
                   prompt_ids=[f.reqs[2]["ids"]])
    assert s2 == [slots[1]] and not pool.close_dev[s2[0]] and pool.closes[s2[0]].tolist() == [0, 0, 0, 0] and pool.n_closing == 0
    assert "closing" not in pool.step_key(pool.kv_bucket()) and "guided" in pool.step_key(pool.kv_bucket())
    assert [ids for _, _, ids in pool.drain(poll=4)] == [got[2]]
    pool.free = sorted(keep)


def _first_mixed(f, per, budget):
    D._prefill(f)
    per = [None if sp is None else dict(sp) for sp in per]
    return f.eng._first_tokens(per, f.reqs, budget).clone(), per


def test_a_budget_below_the_start_states_distance_is_a_value_error(fx):
    f = fx
    pool, eng = f.pool, f.eng
    g = K.region_guide(N_REGIONS, close=True, start=K.TG.LABEL0, V=f.V, ids=f.ids[0])      # 5 tokens from OUT
    per = [dict(greedy=True, guide=g, stream=0)]
    D._prefill(f)
    free = list(pool.free)
    args = (eng.llm.kcache, eng.llm.vtcache, f.hp["seqs"][:1], f.hp["delta"][:1], f.first_greedy[:1])
    with pytest.raises(ValueError, match="5 tokens from an accepting state"):
        pool.join(*args, 4, (), sampling=per, prompt_ids=[f.reqs[0]["ids"]])
    assert pool.free == free and not pool.live and pool.n_closing == 0
    with pytest.raises(ValueError, match="5 tokens from an accepting state"):
        eng._decoder().start(f.hp["seqs"][:1], f.hp["delta"][:1], f.first_greedy[:1], 4, (), sampling=per, prompt_ids=[f.reqs[0]["ids"]])
    with pytest.raises(ValueError, match="5 tokens from an accepting state"):
        eng.generate_batch(f.reqs[:1], max_new_tokens=4, sampling=[dict(greedy=True, guide=g)])
    with pytest.raises(ValueError, match="budget"):      # a closing guide and no budget: _first_tokens cannot close it
        eng._first_tokens([dict(per[0])], f.reqs[:1])
    (ids,) = eng.generate_batch(f.reqs[:1], max_new_tokens=5, sampling=[dict(greedy=True, guide=g)])      # exactly enough: label, </ground>, ..., </objects>
    i = f.ids[0]
    assert len(ids) == 5 and ids[1:] == [i["ground_end"], i["objects"], ids[3], i["objects_end"]] and ids[3] in i["region"][:N_REGIONS], ids


def test_without_mask_rows_or_close_row_room_a_bare_join_fails_and_the_service_waits(fx):
    from vlm_fo1_amd import guide as TG
    from vlm_fo1_amd.serving import PoolHandle, PoolService
    f = fx
    pool = f.pool
    D._prefill(f)

    def two(j):      # 2-state guides with two distinct state bitmaps each -> 2 mask rows
        cls = np.zeros(f.V, np.uint16)
        cls[[10 + 2 * j, 11 + 2 * j]] = [1, 2]
        return TG.TokenGuide(cls, np.array([[1, -1, 1], [0, 0, -1]], np.int32), 0, f.V)
    for j0 in range(0, 28, 7):      # 28 guides: 56 of the 64 mask rows — room for a guided region_answer (6 rows), not for a closing one (9)
        D._join(f, list(range(7)), {b: dict(greedy=True, guide=two(j0 + b), stream=b) for b in range(7)}, f.first_greedy)
    assert sum(u > 0 for u in pool.masks.users) == 56 and pool.MAX_MASKS == 64
    new, old = [dict(greedy=True, guide=f.guide[0])], [dict(greedy=True, guide=f.open_guide[0])]
    assert not pool.can_take((), new, 1) and pool.can_take((), old, 1)
    free = list(pool.free)
    with pytest.raises(RuntimeError, match="wait for sequences to finish"):
        D._join(f, [0], {0: new[0]}, f.first_greedy)
    assert pool.free == free and len(pool.live) == 28 and pool.n_closing == 0

    def item(sampling):
        h = PoolHandle(1)
        ev = torch.cuda.Event()
        ev.record()
        return (h, f.eng.llm.kcache, f.eng.llm.vtcache, [f.hp["seqs"][0]], [f.hp["delta"][0]], f.first_greedy[:1], 8, (), ev, sampling, [f.reqs[0]["ids"]], None, None)
    waiting = [item(new)]
    h = waiting[0][0]
    svc = D._Fx()
    svc.stats = dict(joined=0)
    PoolService._admit(svc, pool, waiting)
    assert len(waiting) == 1 and h._error is None and not h._joined.is_set()
    pool.drain(poll=6)
    D._prefill(f)
    PoolService._admit(svc, pool, waiting)
    assert not waiting and h._joined.is_set() and h._error is None and pool.n_closing == 1
    # close_row room: with the table cut to 40 entries one closing guide (6 states x 5 = 30) fits and a second distinct one has to wait
    cap = pool.gtab._cr.cap
    pool.gtab._cr.cap = 40
    try:
        other = [dict(greedy=True, guide=K.region_guide(1, close=True, V=f.V, ids=f.ids[0]))]
        assert not pool.can_take((), other, 1) and pool.can_take((), new, 1)
        with pytest.raises(RuntimeError, match="closing rows.*wait for sequences to finish"):
            D._join(f, [0], {0: other[0]}, f.first_greedy)
        waiting = [item(other)]
        PoolService._admit(svc, pool, waiting)
        assert len(waiting) == 1 and waiting[0][0]._error is None
        pool.drain(poll=6)
        D._prefill(f)
        PoolService._admit(svc, pool, waiting)
        assert not waiting and pool.n_closing == 1
        pool.drain(poll=6)
    finally:
        pool.gtab._cr.cap = cap
    assert pool.n_closing == 0 and not any(pool.masks.users) and pool.gtab.users() == 0


class _Tok:
    """A tokenizer as far as region_guide asks: the structural and region tokens are single ids, everything else is unknown."""
    unk_token_id = 0

    def __init__(self, ids: dict):
        self.map = {"<ground>": ids["ground"], "</ground>": ids["ground_end"], "<objects>": ids["objects"], "</objects>": ids["objects_end"]}
        self.map.update({f"<region{k}>": t for k, t in enumerate(ids["region"])})

    def convert_tokens_to_ids(self, tok):
        return self.map.get(tok, self.unk_token_id)


def test_plug_in_generate_with_a_closing_region_guide_equals_the_engine_path(fx):
    from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig
    f = fx
    eng = f.eng
    m = FO1ForCausalLM.from_engine(FO1HFConfig({}, {"eos_token_id": f.V - 1}), eng)
    tok = _Tok(f.ids[0])
    g = m.region_guide(tok, N_REGIONS, close=True)
    assert g == f.guide[0] and m.region_guide(tok, N_REGIONS) == f.open_guide[0] and m.region_guide(tok, N_REGIONS, close=False).accept is None
    kw = D._generate_kwargs(f.reqs[0])
    L = kw["inputs"].shape[1]
    for k in (1, 5, 6, 9):
        got = m.generate(**kw, guide=g, max_new_tokens=k)[0, L:].tolist()
        (want,) = eng.generate_batch(f.reqs[:1], max_new_tokens=k, stop_ids=[f.V - 1], sampling=[dict(greedy=True, guide=g)])
        assert got == want and len(got) == k and g.run(got) == K.TG.OUT, (k, got, want)
        assert G.well_formed(f.grammar[0].text(got), N_REGIONS)
        assert (f.ids[0]["objects_end"] in got) == (k >= 6), (k, got)
        st = D._Collect()      # the streamer path: a BatchDecoder of one with the same budget
        assert m.generate(**kw, guide=g, max_new_tokens=k, streamer=st)[0, L:].tolist() == got and st.ended
    opened = m.generate(**kw, guide=m.region_guide(tok, N_REGIONS), max_new_tokens=5)[0, L:].tolist()
    assert f.open_guide[0].run(opened) != K.TG.OUT      # the control: without close=True the answer is cut inside its structure
