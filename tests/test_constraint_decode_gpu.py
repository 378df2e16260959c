"""Per-request token rules in the decode loops (vlm_fo1_amd.llm: TokenMasks, the per-slot rule table, the ruled general head
fo1_decode_head_ruled_accept) on the tiny engine of tests/test_batched_decode_gpu.py: 8 sequences, 16 tokens, a 64-slot
pool.  The rules are built from what the unconstrained run emits, so that they bite.

  * every id of a constrained greedy / sampled / sampled + penalised sequence meets its rule against the oracle on THAT step's logits (greedy
    rows exactly, sampled rows inside the accept rule, exact draws equal to the oracle's id); no banned id is ever recorded; a first-token
    ban gives the masked oracle's first token;
  * min_new_tokens: with the stop id the unconstrained run emits at step k and ban_until = (k + 3, [stop]) the run has at least k + 3 tokens
    and none before is the stop id;
  * plain greedy neighbours' ids are bitwise those of an all-plain pool; graph == eager; slot 0 alone == slot 37 among neighbours;
  * after the last non-plain sequence is harvested the step key is graph_key(bucket) and no mask row has users; a slot left by a constrained
    sequence and reused by a plain one gives the plain ids;
  * a 65th distinct mask fails a bare join with a RuntimeError and waits in PoolService._admit;
  * pool direct, generate_batch and PoolHandle.result() agree bit for bit; so do the BatchDecoder's graph and eager paths;
  * the plug-in: generate(suppress_tokens=[t0]) never returns t0 (the parent ignored the keyword); generate_many takes a batch mixed in the
    new keywords with the pool on and refuses it with the pool off."""
import numpy as np
import pytest
import torch

import constraint_cases as C
import penalty_cases as P
import sampling_cases as S

pytestmark = pytest.mark.gpu

N_SEQ, N_TOK, SEED, PEN = 8, 16, 0x5a17ab1e5eed, 1.3
T, TOP_K = 0.7, 50
UNTIL = 6


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
    assert not f.pool.live and len(f.pool.free) == f.pool.P and f.pool.n_general == 0 and f.pool.n_ruled == 0
    assert f.pool.masks is None or not any(f.pool.masks.users)
    return [got[b] for b in sel]


def _prefill(f):
    """The requests' K / V^T rows back into the engine's prefill cache (another test's generate calls overwrite it)."""
    f.eng.prefill_batch(f.reqs, use_graph=False)
    f.hp = f.eng._last_batch


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
    # the rules, from what the unconstrained run emits
    samp = dict(temperature=T, top_p=1.0, top_k=TOP_K, seed=SEED)
    em = [sorted(set(ids)) for ids in f.plain]
    allow = lambda b: sorted(set(range(7, f.V, 13)) - set(em[b]))      # noqa: E731  (an allow-list without the ids the plain run emits)
    f.per = [None,
             dict(greedy=True, ban=em[1]),
             dict(samp, ban_first=[f.plain[2][0]] + em[2][:3], ban=list(range(0, f.V, 8)) + [7, 9, 31, 33, f.V - 1]),
             dict(samp, repetition_penalty=PEN, ban_until=(UNTIL, em[3])),
             None,
             dict(greedy=True, allow=allow(5)),
             dict(samp, ban=em[6], ban_first=em[1]),
             dict(greedy=True, repetition_penalty=PEN, ban_until=(UNTIL, em[7]), ban_first=[f.plain[7][0]], ban=em[1])]
    f.per = [None if sp is None else dict(sp, stream=b) for b, sp in enumerate(f.per)]
    _prefill(f)
    f.first = f.eng._first_tokens(f.per, f.reqs).clone()
    return f


def _sets(sp: dict, V: int):
    a = set(sp.get("ban") or [])
    if sp.get("allow") is not None:
        a |= set(range(V)) - set(sp["allow"])
    n, e = sp.get("ban_until") or (0, [])
    return dict(always=sorted(a), early=list(e), until=n, first=list(sp.get("ban_first") or []))


def _mixed(f):
    if not hasattr(f, "mixed_ids"):
        _prefill(f)
        f.mixed_ids = _run(f, list(range(N_SEQ)), f.per, f.first)
    return f.mixed_ids


def _bits(row: torch.Tensor) -> np.ndarray:
    return row.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def test_every_id_meets_its_rule_on_its_steps_logits_and_no_banned_id_is_recorded(fx):
    f = fx
    _prefill(f)
    slots = _join(f, list(range(N_SEQ)), f.per, f.first)
    assert f.pool.n_general == 6 and f.pool.n_ruled == 6 and f.pool.masks is not None
    # equal sets share a row: em[1] is an always set of 1 and 7 and a first set of 6 (one bitmap, three users)
    assert sum(f.pool.masks.users) == sum(len(m) for m in f.pool.slot_masks) and sum(u > 0 for u in f.pool.masks.users) < sum(f.pool.masks.users)
    tables = (f.pool.masks.table.clone(), f.pool.rules.clone())
    logits = [f.logits0]
    for _ in range(N_TOK - 1):
        logits.append(f.pool.step(use_graph=True)[slots].clone())
    assert any("ruled" in k for k in f.pool._graphs)
    assert torch.equal(tables[0], f.pool.masks.table) and torch.equal(tables[1], f.pool.rules), "a step wrote the mask or the rule table"
    got = {tag[1]: ids for _, tag, ids in f.pool.harvest(f.pool.snapshot())}
    ids = [got[b] for b in range(N_SEQ)]
    assert [len(r) for r in ids] == [N_TOK] * N_SEQ and [r[0] for r in ids] == f.first.cpu().tolist()
    n_exact = n_draws = 0
    moved = [0] * N_SEQ
    for b in range(N_SEQ):
        sp = f.per[b]
        pen = (sp or {}).get("repetition_penalty", 0.0)
        rule = _sets(sp or {}, f.V)
        seen = [t for t in f.reqs[b]["ids"] if 0 <= t < f.V]
        for t in range(N_TOK):
            banned = C.banned_at(t, **rule)
            assert ids[b][t] not in banned, (b, t, ids[b][t])
            raw = _bits(logits[t][b])
            rb = C.ruled(raw, banned, seen, pen)
            if sp is None or sp.get("greedy"):
                assert ids[b][t] == P.greedy_pick(rb), (b, t, ids[b][t], P.greedy_pick(rb))
                moved[b] += ids[b][t] != P.greedy_pick(P.penalise(raw, seen, pen))
            else:
                o, u = S.oracle(rb, T, 1.0, TOP_K), S.draw_u(t, b, SEED)
                assert S.accepts(o, u, ids[b][t]), (b, t, u, ids[b][t], S.pick(o, u))
                n_draws += 1
                if S.is_exact(o, u):
                    n_exact += 1
                    assert ids[b][t] == S.pick(o, u), (b, t, u)
            seen.append(ids[b][t])
    assert n_draws == 3 * N_TOK and n_exact >= n_draws // 2
    # the rules bite: sequences 1 and 5 may not take the unconstrained first token (it is banned / not on the allow-list), plain ones never move
    assert moved[1] >= 1 and moved[5] >= 1 and moved[0] == moved[4] == 0, moved
    # a first-token ban: the masked oracle's first token, not the unconstrained one
    assert ids[7][0] != f.plain[7][0] and ids[2][0] != f.plain[2][0]
    assert ids == _mixed(f), "the same submission decoded differently the second time"


def test_min_new_tokens_keeps_the_stop_id_away_until_n(fx):
    f = fx
    b, k = 4, 3
    stop = f.plain[b][k]
    _prefill(f)
    short = _run(f, [b], None, f.first_greedy, stop=(stop,))[0]
    assert short == f.plain[b][:len(short)] and short[-1] == stop and len(short) <= k + 1
    per = {b: dict(greedy=True, ban_until=(k + 3, [stop]), stream=b)}
    from vlm_fo1_amd import ops
    # the first token, from row b of the prefill's logits under the same rule (counter 0)
    masks = torch.from_numpy(C.host_masks([[stop]], f.V).view(np.int32)).cuda()
    tok0 = ops.sample_rows(f.logits0[b:b + 1], ops.sample_params([ops.sampling_row(per[b])], "cuda"), general=True, masks=masks,
                           rules=ops.token_rules([(-1, 0, k + 3, -1)], "cuda"))
    firsts = {b: tok0[0]}
    long = _run(f, [b], per, firsts, stop=(stop,))[0]
    assert len(long) >= k + 3 and stop not in long[:k + 3], (long, stop)
    assert long[:len(short) - 1] == short[:-1]
    assert stop not in long[:-1] and (long[-1] == stop or len(long) == N_TOK)


def test_plain_neighbours_graph_eager_slot_and_key(fx):
    f = fx
    pool = f.pool
    mixed = _mixed(f)
    assert mixed[0] == f.plain[0] and mixed[4] == f.plain[4], "a plain greedy sequence changed beside constrained neighbours"
    assert all(mixed[b] != f.plain[b] for b in (1, 5, 7)), "a rule changed nothing"
    _prefill(f)
    assert _run(f, list(range(N_SEQ)), f.per, f.first, graph=False) == mixed, "eager and graph-replayed steps differ"
    for b in (1, 2, 3, 7):
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
    # the last non-plain sequence harvested: today's key, no users; slot 0, left by a constrained sequence, reused by a plain one
    assert pool.n_ruled == 0 and not any(pool.masks.users)
    _join(f, [1], f.per, f.first, budget=3)
    assert pool.ruled_dev[0] and "ruled" in pool.step_key(pool.kv_bucket())
    for _ in range(3):
        pool.step()
    assert [tag[1] for _, tag, _ in pool.harvest(pool.snapshot())] == [1] and not any(pool.masks.users)
    assert pool.step_key(pool.kv_bucket()) == pool.graph_key(pool.kv_bucket())
    slots = _join(f, [0, 4], None, f.first_greedy)
    assert slots == [0, 1] and not pool.ruled_dev[0] and pool.rules[0].tolist() == [-1, -1, 0, -1]
    pool._graphs.clear()
    pool.step()
    assert list(pool._graphs) == [pool.graph_key(pool.kv_bucket())]
    got = {tag[1]: ids for _, tag, ids in pool.drain(poll=4)}
    assert [got[0], got[4]] == [f.plain[0], f.plain[4]]
    # a penalised sequence beside a constrained one in a reused slot
    assert _run(f, [3, 1], f.per, f.first) == [mixed[3], mixed[1]]


def test_a_65th_distinct_mask_fails_a_bare_join_and_waits_in_the_service(fx):
    from vlm_fo1_amd.serving import PoolHandle, PoolService
    f = fx
    pool = f.pool
    _prefill(f)

    def per(j, n, only_ban=()):
        return {b: (dict(greedy=True, ban=[100 + 8 * j + b], stream=b) if b in only_ban else
                    dict(greedy=True, ban=[100 + 8 * j + b], ban_first=[500 + 8 * j + b], ban_until=(2, [900 + 8 * j + b]), stream=b)) for b in range(n)}
    _join(f, list(range(8)), per(0, 8), f.first_greedy)
    _join(f, list(range(8)), per(1, 8), f.first_greedy)
    _join(f, list(range(6)), per(2, 6, only_ban=(5,)), f.first_greedy)
    assert sum(u > 0 for u in pool.masks.users) == pool.MAX_MASKS == 64 and len(pool.live) == 22
    new, old = [dict(greedy=True, ban=[3000])], [dict(greedy=True, ban=[100])]
    assert not pool.can_take((), new, 1) and pool.can_take((), old, 1) and pool.can_take(()) and pool.can_take((), None, 1)
    free = list(pool.free)
    with pytest.raises(RuntimeError, match="64 different token masks are live"):
        _join(f, [0], {0: new[0]}, f.first_greedy)
    assert pool.free == free and len(pool.live) == 22 and sum(u > 0 for u in pool.masks.users) == 64
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
    _join(f, [1], {1: old[0]}, f.first_greedy)      # a set that is live already shares its row
    assert len(pool.live) == 23 and sum(u > 0 for u in pool.masks.users) == 64
    pool.drain(poll=6)
    assert not any(pool.masks.users)
    _prefill(f)
    PoolService._admit(svc, pool, waiting)
    assert not waiting and h._joined.is_set() and h._error is None and pool.n_ruled == 1
    pool.drain(poll=6)
    # a submission that alone needs more rows than the table has can never be taken: it is admitted, and fails its own handle
    assert pool.can_take((), [dict(greedy=True, ban=[i]) for i in range(65)], 65)


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
    assert bd == eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=False, sampling=per), "BatchDecoder ruled head: graph != eager"
    for b in range(N_SEQ):      # (other kernels than the pool's: the logits differ in last bits, the rules are the same)
        rule = _sets(per[b] or {}, f.V)
        assert all(bd[b][t] not in C.banned_at(t, **rule) for t in range(N_TOK)), b
    plain = eng.generate_batch(f.reqs, max_new_tokens=N_TOK, use_graph=True)
    assert all(bd[b] != plain[b] for b in (1, 5, 7))


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
    kws = [dict(_generate_kwargs(r), max_new_tokens=8) for r in f.reqs[:4]]
    L = kws[0]["inputs"].shape[1]
    plain = m.generate(**kws[0])[0, L:].tolist()
    t0 = plain[0]
    got = m.generate(**kws[0], suppress_tokens=[t0])[0, L:].tolist()
    assert len(got) == 8 and got[0] != t0 and t0 not in got, "suppress_tokens was ignored"
    assert got[0] == P.greedy_pick(C.mask(_bits(f.logits0[0]), [t0]))
    assert m.generate(**kws[0], bad_words_ids=[[t0]])[0, L:].tolist() == got
    begin = m.generate(**kws[0], begin_suppress_tokens=[t0])[0, L:].tolist()
    assert begin[0] == got[0] and begin != plain
    allowed = m.generate(**kws[0], allowed_token_ids=list(range(10, 40)))[0, L:].tolist()
    assert all(10 <= t < 40 for t in allowed)
    st = _Collect()      # with a streamer: a BatchDecoder of one, the same ids
    assert m.generate(**kws[0], suppress_tokens=[t0], streamer=st)[0, L:].tolist() == got and st.ended
    # min_new_tokens: the EOS id is the id the plain run emits at step 2 (k = its first occurrence: the tiny model repeats itself)
    eos = plain[2]
    k = plain.index(eos)
    m2 = FO1ForCausalLM.from_engine(FO1HFConfig({}, {"eos_token_id": eos}), eng)
    assert m2.generate(**kws[0])[0, L:].tolist() == plain[:k + 1]
    late = m2.generate(**kws[0], min_new_tokens=k + 3)[0, L:].tolist()
    assert len(late) >= k + 3 and eos not in late[:k + 3] and late[:k] == plain[:k]
    with pytest.raises(ValueError, match="outside"):
        m.generate(**kws[0], suppress_tokens=[f.V])
    with pytest.raises(ValueError, match="every one"):
        m.generate(**kws[0], allowed_token_ids=[5], suppress_tokens=[5])
    # a batch mixed in the new keywords: refused without the pool, taken with it
    batch = [kws[0], dict(kws[1], suppress_tokens=[t0, 17]), dict(kws[2], min_new_tokens=3, begin_suppress_tokens=[5]), dict(kws[3], allowed_token_ids=list(range(64, 512)))]
    with pytest.raises(ValueError, match="token-rule keywords"):
        m.generate_many(batch)
    same = m.generate_many([dict(k, suppress_tokens=[t0]) for k in kws[:3]])      # a uniform constrained batch needs no pool
    assert same[0][0, L:].tolist() == got
    eng.enable_decode_pool(slots=64)
    try:
        out = m.generate_many(batch)
        assert [tuple(o.shape) for o in out] == [(1, k["inputs"].shape[1] + 8) for k in kws]
        assert out[0][0, L:].tolist() == plain
        new1 = out[1][0, kws[1]["inputs"].shape[1]:].tolist()
        assert t0 not in new1 and 17 not in new1
        assert all(64 <= t < 512 for t in out[3][0, kws[3]["inputs"].shape[1]:].tolist())
        assert [o.tolist() for o in m.generate_many_async(batch).result()] == [o.tolist() for o in out]
    finally:
        eng.disable_decode_pool()
