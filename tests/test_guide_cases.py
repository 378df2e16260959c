"""CPU checks of the token guides' host side (vlm_fo1_amd/guide.py, the guide plumbing of vlm_fo1_amd/llm.py) and of the case set the GPU
tests use (tests/guide_cases.py):

  * ban_sequences against transformers' NoBadWordsLogitsProcessor: over seeded random id streams at V = 63 the banned set of the automaton's
    state equals the set HF sends to -inf, at every step of every stream — words of length 1 to 4, shared prefixes, a word that is a suffix
    of another, a word whose prefix ends the prompt;
  * region_answer against transformers' PrefixConstrainedLogitsProcessor driven by the naive restatement of the grammar
    (guide_cases.Grammar): equal banned sets along accepted strings, and every accepted string that ends in OUT passes the plug-in's own
    parsers with indices below n_regions;
  * TokenGuide's validation errors, content hashing, the folding of ban / allow, the dead-state refusals (min_new_tokens against a stop-only
    exit among them), the sharing of GuideTables' spans;
  * the head cases leave out at most 2 % of their (row, state) pairs."""
import inspect

import numpy as np
import pytest
import torch

import guide_cases as G
from vlm_fo1_amd import guide as TG
from vlm_fo1_amd import llm

V = 63


def _hf_banned(proc, ids) -> set:
    scores = torch.zeros(1, V)
    out = proc(torch.tensor([ids], dtype=torch.long), scores)
    return set(torch.nonzero(torch.isinf(out[0]) & (out[0] < 0)).view(-1).tolist())


def _guide_banned(g, s) -> set:
    return set(np.nonzero(TG.unpack_bits(g.banned(s), g.V))[0].tolist())


WORD_LISTS = [
    [[5], [7, 8], [7, 8, 9], [7, 9, 10, 11], [8, 9], [20, 21, 22, 23], [22, 23, 30], [9, 10]],      # lengths 1-4, shared prefixes, [8, 9] a suffix of [7, 8, 9]
    [[1, 2, 3, 4], [2, 3, 5], [3, 6], [4], [1, 2, 1, 2], [2, 1]],
    [[11, 11], [11, 11, 11], [12, 11, 11, 13], [40]],
]


@pytest.mark.parametrize("words", WORD_LISTS, ids=["mixed", "overlap", "repeats"])
def test_ban_sequences_equals_no_bad_words_at_every_step_of_every_stream(words):
    from transformers import NoBadWordsLogitsProcessor
    proc = NoBadWordsLogitsProcessor(words, eos_token_id=None)
    g = TG.ban_sequences(words, V)
    toks = sorted({t for w in words for t in w})
    rng = np.random.default_rng(4242)
    steps = 0
    for stream in range(40):
        # a prompt that ends in a word's prefix (every other stream), then ids drawn mostly from the words' tokens
        w = words[stream % len(words)]
        prompt = rng.integers(0, V, 5).tolist() + (list(w[:-1]) if stream % 2 == 0 else [])
        s = g.run(prompt)
        ids = list(prompt)
        for _ in range(30):
            hf = _hf_banned(proc, ids)
            assert _guide_banned(g, s) == hf, (ids, s)
            steps += 1
            pool = [t for t in (toks if rng.random() < 0.8 else range(V)) if t not in hf] or [t for t in range(V) if t not in hf]
            t = int(pool[rng.integers(len(pool))])
            assert g.advance(s, t) == g.run([t], s)
            s = g.advance(s, t)
            ids.append(t)
        # the prompt may hold whole banned words: the state after it is the one HF's suffix match sees
        ids2 = rng.choice(toks, 12).tolist()
        assert _guide_banned(g, g.run(ids2)) == _hf_banned(proc, ids2), ids2
    assert steps == 1200
    assert g.from_prompt and g.S == 1 + len({tuple(w[:k]) for w in words for k in range(1, len(w))})


IDS = dict(ground=50, ground_end=51, objects=52, objects_end=53, region=[40, 41, 42, 43, 44], stops=[60, 61])


def _region_guide(n):
    return TG.region_answer(V, IDS["ground"], IDS["ground_end"], IDS["objects"], IDS["objects_end"], IDS["region"], n, IDS["stops"])


@pytest.mark.parametrize("n", [1, 3, 5])
def test_region_answer_equals_the_prefix_constrained_processor_and_its_strings_parse(n):
    from transformers import PrefixConstrainedLogitsProcessor
    gr = G.Grammar(V, IDS["ground"], IDS["ground_end"], IDS["objects"], IDS["objects_end"], IDS["region"], n, IDS["stops"])
    g = _region_guide(n)
    hist = {}
    proc = PrefixConstrainedLogitsProcessor(lambda batch_id, sent: gr.allowed(sent.tolist()), num_beams=1)
    names = {TG.OUT: "OUT", TG.LABEL0: "LABEL0", TG.LABEL: "LABEL", TG.OPEN: "OPEN", TG.OBJ0: "OBJ0", TG.OBJ: "OBJ"}
    rng = np.random.default_rng(77 + n)
    special = [IDS["ground"], IDS["ground_end"], IDS["objects"], IDS["objects_end"]] + IDS["region"]
    ended_out = 0
    for _ in range(60):
        s, ids = g.start, []
        for _ in range(int(rng.integers(3, 40))):
            assert names[s] == gr.state(ids)
            hf = _hf_banned(proc, ids)
            assert _guide_banned(g, s) == hf == set(range(V)) - set(gr.allowed(ids)), (ids, s)
            ok = [t for t in range(V) if t not in hf]
            fav = [t for t in ok if t in special]      # structural tokens often, or the walk would rarely leave OUT
            t = int(rng.choice(fav)) if fav and rng.random() < 0.6 else int(rng.choice(ok))
            s = g.advance(s, t)
            ids.append(t)
            hist[names[s]] = hist.get(names[s], 0) + 1
            if t in IDS["stops"]:
                break
        if s == TG.OUT:
            ended_out += 1
            text = gr.text(ids)
            assert G.well_formed(text, n), text
    assert ended_out >= 10 and set(hist) == set(names.values()), hist
    # what the guide exists to prevent does not parse
    assert not G.well_formed("<ground>a</ground><objects><region0>", n) and not G.well_formed(f"<ground>a</ground><objects><region{n}></objects>", n)


def test_token_guide_validation_errors():
    cls = np.zeros(V, np.uint16)
    cls[5:] = 1
    nx = np.array([[0, 1], [1, -1]], np.int32)
    g = TG.TokenGuide(cls, nx, 0, V)
    assert (g.S, g.C, g.start) == (2, 2, 0) and g.advance(1, 7) == 1 and g.advance(0, 7) == 1 and g.run([7, 0, 9]) == 1
    assert TG.TokenGuide(cls, nx.astype(np.int16), 0, V) == g
    with pytest.raises(ValueError, match="uint16"):
        TG.TokenGuide(cls.astype(np.int32), nx, 0, V)
    with pytest.raises(ValueError, match="int16 or int32"):
        TG.TokenGuide(cls, nx.astype(np.int64), 0, V)
    with pytest.raises(ValueError, match="shape"):
        TG.TokenGuide(cls[:-1], nx, 0, V)
    with pytest.raises(ValueError, match="shape"):
        TG.TokenGuide(cls, nx.reshape(-1), 0, V)
    with pytest.raises(ValueError, match="class 2 outside"):
        TG.TokenGuide(np.full(V, 2, np.uint16), nx, 0, V)
    with pytest.raises(ValueError, match="state 2 outside"):
        TG.TokenGuide(cls, np.array([[0, 2], [1, -1]], np.int32), 0, V)
    for start in (-1, 2, 0.0, True):
        with pytest.raises(ValueError, match="start state"):
            TG.TokenGuide(cls, nx, start, V)
    with pytest.raises(ValueError, match="state 1 can be reached and bans all"):
        TG.TokenGuide(cls, np.array([[0, 1], [-1, -1]], np.int32), 0, V)
    TG.TokenGuide(cls, np.array([[0, -1], [-1, -1]], np.int32), 0, V)      # a dead state nobody reaches is no error
    with pytest.raises(ValueError, match="n_regions = 0"):
        _region_guide(0)
    with pytest.raises(ValueError, match="n_regions = 6"):
        _region_guide(6)
    with pytest.raises(ValueError, match="distinct"):
        TG.region_answer(V, 50, 50, 52, 53, [40], 1, [60])
    with pytest.raises(ValueError, match="outside"):
        TG.region_answer(V, 50, 51, 52, 53, [V], 1, [60])
    with pytest.raises(ValueError, match="empty word"):
        TG.ban_sequences([[1], []], V)
    with pytest.raises(ValueError, match="outside"):
        TG.ban_sequences([[1, V]], V)
    with pytest.raises(ValueError, match="bans all"):
        TG.ban_sequences([[t] for t in range(V)], V)


def test_content_hashing_and_shared_class_maps():
    a, b, c = _region_guide(3), _region_guide(3), _region_guide(4)
    assert a == b and hash(a) == hash(b) and a is not b and a != c and len({a, b, c}) == 2
    assert a.cls.tobytes() == c.cls.tobytes(), "guides that differ in n_regions only share their class map"
    assert a.banned(TG.OPEN) == c.banned(TG.OPEN) and a.banned(TG.LABEL) == c.banned(TG.LABEL) and a.banned(TG.OBJ) != c.banned(TG.OBJ)
    assert TG.ban_sequences([[1, 2], [3]], V) == TG.ban_sequences([[3], [1, 2]], V) != TG.ban_sequences([[1, 2]], V)
    assert len(a.banned(0)) == 4 * llm.ops.seen_words(V)
    with pytest.raises((ValueError, AttributeError)):
        a.next[0, 0] = 5


def test_folding_ban_and_allow_and_the_dead_state_refusals():
    g = _region_guide(2)
    tr = llm.sampling_rules([dict(greedy=True, guide=g, ban=[40, 7])], 1, V)
    (plan,) = llm.sampling_guides([dict(greedy=True, guide=g, ban=[40, 7])], 1, V, tr)
    assert plan.s0 == TG.OUT and plan.after_first is None and len(plan.bitmaps) == 6
    for s in range(6):
        assert set(np.nonzero(TG.unpack_bits(plan.bitmaps[s], V))[0]) == _guide_banned(g, s) | {40, 7}
    assert llm.unguided_rules(tr, [plan]) == [None], "the always-bans moved into the guide's state bitmaps"
    assert llm.sampling_table([dict(greedy=True, guide=g)], 1)[1] == ["general"]
    # ban_first / ban_until stay the rule's phases
    sp = dict(greedy=True, guide=g, ban_first=[3], ban_until=(2, [60, 61]))
    tr = llm.sampling_rules([sp], 1, V)
    plans = llm.sampling_guides([sp], 1, V, tr)
    (rest,) = llm.unguided_rules(tr, plans)
    assert rest.always is None and rest.first is not None and rest.early is not None and rest.until == 2
    assert plans[0].bitmaps[TG.LABEL] == g.banned(TG.LABEL)

    def refuse(sp, match):
        with pytest.raises(ValueError, match=match):
            llm.sampling_guides([sp], 1, V, llm.sampling_rules([sp], 1, V))

    refuse(dict(greedy=True, guide=g, ban=[40, 41]), "state 4")                    # both regions banned: OBJ0 has nothing left
    refuse(dict(greedy=True, guide=g, ban=[52]), "state 3")                        # <objects> banned: OPEN has nothing left
    refuse(dict(greedy=True, guide=g, allow=[50, 51, 52, 53, 40]), "state 1")      # no plain token on the allow-list: no label
    llm.sampling_guides([dict(greedy=True, guide=g, ban=[53])], 1, V, llm.sampling_rules([dict(greedy=True, guide=g, ban=[53])], 1, V))      # OBJ never closes, but always has a pick
    refuse(dict(greedy=True, guide="regions"), "TokenGuide")
    refuse(dict(greedy=True, guide=TG.region_answer(64, 50, 51, 52, 53, [40], 1, [60])), "64 tokens")
    # a guide whose only exit is a stop id that min_new_tokens bans
    cls = np.zeros(V, np.uint16)
    cls[60] = 1
    stop_only = TG.TokenGuide(cls, np.array([[1, -1], [-1, 1]], np.int32), 0, V)      # anything, then only the stop id
    ok = dict(greedy=True, guide=stop_only)
    llm.sampling_guides([ok], 1, V, llm.sampling_rules([ok], 1, V))
    refuse(dict(ok, ban_until=(3, [60])), "state 1 after 1 generated")
    refuse(dict(ok, ban_until=(1, [60]), ban=[60]), "state 1")
    llm.sampling_guides([dict(ok, ban_until=(1, [60]))], 1, V, llm.sampling_rules([dict(ok, ban_until=(1, [60]))], 1, V))      # n = 1 bans the first pick only
    # a ban_sequences guide starts in the prompt's state and needs the prompt
    bs = TG.ban_sequences([[7, 8, 9]], V)
    with pytest.raises(ValueError, match="prompt_ids"):
        llm.sampling_guides([dict(greedy=True, guide=bs)], 1, V, [None])
    (p,) = llm.sampling_guides([dict(greedy=True, guide=bs)], 1, V, [None], [[1, 7, 8]])
    assert p.s0 == bs.run([7, 8]) != bs.start and _guide_banned(bs, p.s0) == {9}


def test_spans_share_by_content_and_never_move_a_span_with_users():
    sp = llm._Spans(10)
    a, new = sp.acquire("a", 4)
    assert (a, new) == (0, True) and sp.acquire("a", 4) == (0, False)
    assert sp.acquire("b", 4) == (4, True) and not sp.room([("c", 3)]) and sp.room([("c", 2), ("a", 4)])
    with pytest.raises(RuntimeError):
        sp.acquire("c", 3)
    sp.release("b")
    assert sp.room([("c", 3)]) and sp.acquire("b", 4) == (4, False), "a span without users stays findable"
    sp.release("b")
    assert sp.acquire("c", 6) == (4, True) and "b" not in sp.ent, "its place was taken"
    sp.release("a"), sp.release("a")
    assert sp.acquire("d", 4) == (0, True) and "a" not in sp.ent


def _two_state_guide(j):
    cls = np.zeros(V, np.uint16)
    cls[[10 + 2 * j, 11 + 2 * j]] = [1, 2]
    return TG.TokenGuide(cls, np.array([[1, -1, 1], [0, 0, -1]], np.int32), 0, V)


def test_a_pass_holds_its_rule_rows_while_its_guides_take_theirs():
    """FO1Engine._first_tokens' scratch tables after many passes: every row of the mask table has held some bitmap, so a new bitmap takes the
    lowest row without users.  The pass's rule rows must still hold the rule's bitmaps when its guides have taken theirs."""
    def row_bytes(tm, r):
        return tm.table[r].numpy().tobytes()

    tm = llm.TokenMasks(6, V, "cpu")
    for t in range(6):      # saturate: six bitmaps that came and went
        tm.release(tm.acquire(llm.token_rule(dict(ban=[t]), V).always))
    assert not any(tm.users) and len(tm._row) == 6
    gt = llm.GuideTables(V, "cpu", tm)
    rule = llm.token_rule(dict(ban=[30], ban_first=[31], ban_until=(2, [32])), V)
    sp = dict(greedy=True, guide=_two_state_guide(0))
    (plan,) = llm.sampling_guides([sp], 1, V, [None])
    held = llm.PassTables(tm, gt, [rule, None], [None, plan])
    a, e, until, f = held.rules[0]
    assert held.rules[1] is None and until == 2 and held.guides[0] is None
    assert (row_bytes(tm, a), row_bytes(tm, e), row_bytes(tm, f)) == (rule.always, rule.early, rule.first), "a rule row was rewritten"
    crow, C, noff, roff = held.guides[1]
    srows = gt.state_row[roff:roff + 2].tolist()
    assert [row_bytes(tm, r) for r in srows] == list(plan.bitmaps) and len({a, e, f, *srows}) == 5
    assert gt.next[noff:noff + 2 * C].tolist() == plan.guide.next.reshape(-1).tolist()
    assert gt.cls[crow].numpy().view(np.uint16).tolist() == plan.guide.cls.tolist()
    assert sum(tm.users) == 5 and gt.users() == 1
    held.release()
    assert not any(tm.users) and gt.users() == 0 and not gt.live
    held.release()      # (idempotent)
    # an acquire that cannot finish gives back what it took: 3 rule rows + 2 x 2 state bitmaps do not fit 6 rows
    (plan2,) = llm.sampling_guides([dict(greedy=True, guide=_two_state_guide(1))], 1, V, [None])
    with pytest.raises(RuntimeError, match="mask table"):
        llm.PassTables(tm, gt, [rule, None, None], [None, plan, plan2])
    assert not any(tm.users) and gt.users() == 0
    # the bookkeeping alone answers for room before anything is allocated
    assert llm.GuideTables(V, None, None).room([plan, plan2]) and len(llm.GuideTables(V, None, None).new_bitmaps([plan, plan, plan2])) == 4


def test_the_fold_cache_is_read_once():
    g = _region_guide(2)
    maps = [g.state_bitmaps(bytes([k]) + bytes(len(g.banned(0)) - 1)) for k in range(1, 120)]      # more entries than the cache keeps
    assert maps[0] == g.state_bitmaps(bytes([1]) + bytes(len(g.banned(0)) - 1)) and g.banned(3) == g.banned(3)
    assert len(g._banned) <= 4 * g.S + 66


def test_head_cases_leave_out_at_most_two_percent():
    left, pairs = G.left_out()
    print(f"\n{len(left)} of {pairs} (row, state) pairs left out for their top-p margin: {left}")
    assert pairs == 570 and len(left) <= G.MAX_LEFT_OUT * pairs
    cs = G.head_cases()
    assert {c["state"] for c in cs} == set(range(5)) and {c["V"] for c in cs} == set(G.CASE_V)
    for V_ in G.CASE_V:
        g = G.head_guide(V_)
        assert (g.S, g.C) == (5, G.N_CLASSES) and g.classes_present().all()
        assert all((G.HEAD_NEXT[s] < 0).any() and (G.HEAD_NEXT[s] >= 0).any() for s in range(5))
    gc = G.greedy_head_cases()
    assert len(gc) == 45 and all(c["want"] not in c["banned"] for c in gc)
    assert any(a["want"] != b["want"] for a, b in zip(gc[0::5], gc[1::5])), "banning the argmax moved no greedy pick"


def test_plug_in_guide_keyword_and_plans():
    from vlm_fo1.model.fo1_model import FO1ForCausalLM
    sig = inspect.signature(FO1ForCausalLM.generate)
    assert "guide" in sig.parameters and sig.parameters["guide"].default is None
    from vlm_fo1.model.fo1_model import FO1HFConfig
    g, g2 = _region_guide(2), _region_guide(3)
    plan = FO1ForCausalLM._decode_plan
    assert plan({}) is None and plan(dict(guide=None)) is None
    assert plan(dict(guide=g)) == dict(greedy=True, guide=g)
    p = plan(dict(guide=g, do_sample=True, temperature=0.7, seed=3, suppress_tokens=[4]), None, (60,))
    assert p["guide"] is g and p["temperature"] == pytest.approx(0.7) and p["ban"] == (4,) and "greedy" not in p
    with pytest.raises(ValueError, match="TokenGuide"):
        plan(dict(guide="regions"))
    m = FO1ForCausalLM.__new__(FO1ForCausalLM)
    m.config = FO1HFConfig({}, {"eos_token_id": [60, 61]})
    base = dict(max_new_tokens=8)
    with pytest.raises(ValueError, match="inputs"):      # uniform in the guide (equal by content): the plan gets as far as the requests
        m._batch_plan([dict(base, guide=g), dict(base, guide=_region_guide(2))])
    for batch in ([base, dict(base, guide=g)], [dict(base, guide=g), dict(base, guide=g2)]):      # mixed: refused without the pool ...
        with pytest.raises(ValueError, match="the guide.*unless the decode pool is enabled"):
            m._batch_plan(batch)

    class _Eng:
        _pool_svc = object()
    m.engine = _Eng()
    with pytest.raises(ValueError, match="inputs"):      # ... and taken with it
        m._batch_plan([base, dict(base, guide=g), dict(base, guide=g2)])
    with pytest.raises(ValueError, match="TokenGuide"):
        m._batch_plan([base, dict(base, guide=5)])

    # region_guide: the ids come from the tokenizer, the stop ids from the config
    class _Tok:
        unk_token_id = 0
        names = {"<ground>": 50, "</ground>": 51, "<objects>": 52, "</objects>": 53, **{f"<region{k}>": 40 + k for k in range(5)}}

        def convert_tokens_to_ids(self, t):
            return self.names.get(t, self.unk_token_id)

    class _Cfg:
        class llm:
            vocab_size = V
    m.engine = type("E", (), dict(cfg=_Cfg))()
    assert m.region_guide(_Tok(), 3) == g2 and m.region_guide(_Tok(), 2) == g
    with pytest.raises(ValueError, match="5 <regionK> tokens"):
        m.region_guide(_Tok(), 6)
    bad = _Tok()
    bad.names = {k: v for k, v in _Tok.names.items() if k != "</objects>"}
    with pytest.raises(ValueError, match="single id"):
        m.region_guide(bad, 2)
    with pytest.raises(ValueError, match="n_regions = 0"):
        m.region_guide(_Tok(), 0)
