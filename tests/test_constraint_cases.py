"""CPU checks of the token rules (tests/constraint_cases.py): the oracle against transformers' SuppressTokens / NoBadWords /
MinNewTokensLength / SuppressTokensAtBegin processors chained in front of the warpers, the conditions the cases must meet (on the oracle
alone: at most 5 % of the (row, ban kind) pairs left out), llm.token_rule's normalisation and errors, TokenMasks' sharing and release, the C
ABI additions (argument checks run before any HIP call: fake pointers), generate()'s keywords, and the plan of a batch that differs only in them."""
import inspect

import numpy as np
import pytest
import torch

import constraint_cases as C
import penalty_cases as P
import sampling_cases as S
from vlm_fo1.model.fo1_model import FO1ForCausalLM, FO1HFConfig
from vlm_fo1_amd import lib as L


def test_oracle_matches_the_transformers_processors_in_front_of_the_warpers():
    """Tie-free rows (distinct fp64 logits), the three phases of a rule with all four processors: HF sets the banned scores to -inf, the
    oracle gives them no key — the same kept set after the warpers, and probabilities equal to 1e-12."""
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(11)
    n = 0
    for V in (1000, 4099):
        x = S.from_bits(S.to_bits(rng.standard_normal(V) * 3))
        _, first = np.unique(x, return_index=True)
        x = x[np.sort(first)]
        V = len(x)
        bits = S.to_bits(x)
        order = np.argsort(-x)
        suppress, words = order[[0, 5]].tolist(), [[int(order[2])], [int(order[9])]]       # SuppressTokens + NoBadWords: the `always` set
        eos, begin = order[[1, 20]].tolist(), order[[3, 4]].tolist()                        # MinNewTokensLength: `early`; AtBegin: `first`
        prompt_len, until = 6, 4
        procs = [lp.SuppressTokensLogitsProcessor(suppress), lp.NoBadWordsLogitsProcessor(words, eos_token_id=None),
                 lp.MinNewTokensLengthLogitsProcessor(prompt_len, until, eos), lp.SuppressTokensAtBeginLogitsProcessor(begin, prompt_len)]
        always = suppress + [w[0] for w in words]
        for c in (0, until - 1, until):
            banned = C.banned_at(c, always, eos, until, begin)
            assert len(banned) == {0: 8, until - 1: 6, until: 4}[c]
            ids = torch.zeros(1, prompt_len + c, dtype=torch.long)
            for T, top_p, top_k in ((0.7, 0.9, 50), (1.0, 1.0, 0), (1.5, 0.5, 0), (0.3, 1.0, 1)):
                o = S.oracle(C.mask(bits, banned), T, top_p, top_k)
                s = torch.tensor(x, dtype=torch.float64)[None]
                for pr in procs:
                    s = pr(ids, s)
                assert torch.isinf(s[0, banned]).all() and int(torch.isinf(s).sum()) == len(banned)
                s = lp.TemperatureLogitsWarper(float(np.float32(T)))(None, s)
                if top_k:
                    s = lp.TopKLogitsWarper(top_k)(None, s)
                if top_p < 1:
                    s = lp.TopPLogitsWarper(float(np.float32(top_p)))(None, s)
                prob = torch.softmax(s, -1)[0].numpy()
                assert ((prob > 0) == o.K).all() and not o.K[banned].any(), (V, c, T, top_p, top_k)
                assert np.abs(prob - o.w / o.z2).max() < 1e-12
                n += 1
    assert n == 24


def test_cases_leave_out_at_most_five_percent_and_cover_every_kind():
    cs = C.cases()
    left, pairs = C.left_out()
    print(f"\n{len(cs)} ruled rows; {len(left)} of {pairs} (row, ban kind) pairs left out for their top-p margin: {left}")
    assert pairs == 684 and len(left) <= C.MAX_LEFT_OUT * pairs
    for V in C.CASE_V:
        assert {c["kind"] for c in cs if c["V"] == V} == set(C.BAN_KINDS)
        assert any(P.penalty_on(c["p"]) and len(c["banned"]) for c in cs if c["V"] == V)
    assert sum(c["V"] == C.BIG_V for c in cs) == 3
    for c in cs:
        assert c["oracle"].margin >= S.EXACT_MARGIN * S.EPS and len(c["draws"]) >= 3, c["name"]
        assert c["oracle"].empty or not c["oracle"].K[c["banned"]].any(), c["name"]
    exact = sum(S.is_exact(c["oracle"], u) for c in cs for u in c["draws"])
    total = sum(len(c["draws"]) for c in cs)
    print(f"{total} draws of which {exact} exact")
    assert exact > total - exact > 0
    # the bans do something: most non-empty ones change the kept set
    plain = {(r["name"]): r["oracle"] for r in S.rows_and_batches()[0]}
    changed = [c for c in cs if len(c["banned"]) and not P.penalty_on(c["p"]) and c["V"] != C.BIG_V and
               (c["oracle"].empty or (c["oracle"].K != plain[c["name"].split("|")[0]].K).any())]
    assert len(changed) >= len(cs) // 3
    # the tail kind covers the unaligned last group, every8 the byte and word boundaries
    t = next(c for c in cs if c["V"] == 4099 and c["kind"] == "tail")
    assert t["banned"].tolist() == list(range(4088, 4099))
    e = next(c for c in cs if c["V"] == 4099 and c["kind"] == "every8")
    assert {0, 7, 8, 9, 31, 32, 33, 4096, 4098} <= set(e["banned"].tolist())


def test_greedy_and_phase_cases_say_what_they_claim():
    g = {c["name"]: c for c in C.greedy_cases()}
    for V in C.CASE_V:
        ties = sorted({7, V // 2, V - 1})
        assert g[f"V{V}-ties"]["want"] == ties[0] and g[f"V{V}-ties-first-banned"]["want"] == ties[1]
        assert g[f"V{V}-ties-all-but-last-banned"]["want"] == V - 1 and g[f"V{V}-ties-all-banned"]["want"] not in ties
        assert g[f"V{V}-banned-inf-nan"]["want"] == V - 1
        assert g[f"V{V}-all-but-one"]["want"] == V // 3 and g[f"V{V}-all-but-last"]["want"] == V - 1
        assert g[f"V{V}-everything-banned"]["want"] == 0
        assert g[f"V{V}-penalty-then-ban"]["want"] == ties[2] and g[f"V{V}-banned-and-seen"]["want"] == ties[1]
    ph = {c["name"]: c["want"] for c in C.phase_cases()}
    for V in C.CASE_V:
        f, e, a, rest = 9, V - 1, V // 2, 33
        assert [ph[f"V{V}-A-c{c}"] for c in (0, 4, 5)] == [f, f, f]            # the maximum (a) is banned at every pick
        assert [ph[f"V{V}-E-c{c}"] for c in (0, 4, 5)] == [f, f, e]            # ... (e) while c < 5
        assert [ph[f"V{V}-F-c{c}"] for c in (0, 4, 5)] == [e, f, f]            # ... (f) at c == 0
        assert [ph[f"V{V}-AEF-c{c}"] for c in (0, 4, 5)] == [rest, f, f]
    assert (C.banned_at(0, [1], [2], 3, [4]) == [1, 2, 4]).all() and (C.banned_at(2, [1], [2], 3, [4]) == [1, 2]).all()
    assert (C.banned_at(3, [1], [2], 3, [4]) == [1]).all()
    bm = C.host_masks([[0, 62]], 63, pad_ones=True)
    assert bm[0].tolist() == [0x00000001, 0xc0000000, 0xffffffff, 0xffffffff]


def test_token_rule_normalises_and_refuses():
    from vlm_fo1_amd import ops
    from vlm_fo1_amd.llm import has_rule, sampling_rules, sampling_table, token_rule
    V = 100
    W = ops.seen_words(V) * 4
    assert token_rule(None, V) is None and token_rule(dict(temperature=0.7), V) is None and not has_rule(dict(greedy=True, ban=None))

    def ids_of(bm):
        return [] if bm is None else np.nonzero(np.unpackbits(np.frombuffer(bm, np.uint8), bitorder="little"))[0].tolist()

    r = token_rule(dict(greedy=True, ban=[5, 3, 5], ban_first=[99], ban_until=(4, [7, 0])), V)
    assert len(r.always) == W and ids_of(r.always) == [3, 5] and ids_of(r.first) == [99] and ids_of(r.early) == [0, 7] and r.until == 4
    assert r.always == P.host_bitmap([[3, 5]], V).tobytes()      # the seen bitmap's layout
    r = token_rule(dict(allow=[1, 2, 3], ban=[2]), V)
    assert ids_of(r.always) == [t for t in range(V) if t not in (1, 3)] and r.early is None and r.first is None and r.until == 0
    assert token_rule(dict(ban_until=3), V, eos_ids=[9]).until == 3 and ids_of(token_rule(dict(ban_until=3), V, eos_ids=[9]).early) == [9]
    r = token_rule(dict(ban=[1], ban_until=(0, [2])), V)         # n = 0: no early phase
    assert r.early is None and r.until == 0
    assert token_rule(dict(ban=[1]), V) == token_rule(dict(ban=(1, 1)), V)
    for bad, word in ((dict(ban=[1.5]), "integers"), (dict(ban=[True]), "integers"), (dict(ban=["a"]), "integers"), (dict(ban=[V]), "outside"),
                      (dict(ban_first=[-1]), "outside"), (dict(allow=[]), "empty allow"), (dict(ban_until=(-1, [2])), "< 0"),
                      (dict(ban_until=(2, [V + 3])), "outside"), (dict(ban=list(range(V))), "every one"), (dict(allow=[4], ban=[4]), "every one"),
                      (dict(allow=[4], ban_first=[4]), "at the first token"), (dict(allow=[4, 5], ban_until=(3, [4, 5])), "before ban_until"),
                      (dict(ban=5), "list of token ids"), (dict(ban_until=(1, 2, 3)), "ban_until")):
        with pytest.raises(ValueError, match=word):
            token_rule(bad, V)
    # a dict with a rule key is a general sequence, greedy or sampled
    rows, kinds = sampling_table([None, dict(greedy=True, ban=[1]), dict(temperature=0.7, seed=1, ban_first=[2]), dict(temperature=0.7, seed=1)], 4)
    assert kinds == ["plain", "general", "general", "sampled"] and rows[1][5] and not rows[2][5]
    tr = sampling_rules(dict(greedy=True, ban=[1]), 3, V)
    assert len(tr) == 3 and tr[0] == tr[2] and tr[0] is not None
    assert sampling_rules(None, 2, V) == [None, None]
    with pytest.raises(ValueError, match="needs a temperature"):
        sampling_table(dict(ban=[1]), 1)
    assert ops.token_rules([None, (3, -1, 0, 2)]).tolist() == [[-1, -1, 0, -1], [3, -1, 0, 2]]


def test_token_masks_share_rows_and_release_them():
    from vlm_fo1_amd.llm import TokenMasks, token_rule
    V = 70
    tm = TokenMasks(4, V, "cpu")
    assert tuple(tm.table.shape) == (4, 4)
    a, b, c = (token_rule(dict(ban=ids), V).always for ids in ([1], [2, 33], [69]))
    ra, rb = tm.acquire(a), tm.acquire(b)
    assert ra != rb and tm.acquire(a) == ra and tm.users[ra] == 2 and tm.users[rb] == 1
    assert tm.table[ra].tolist() == [2, 0, 0, 0] and tm.table[rb].tolist() == [4, 2, 0, 0]
    row, held = tm.rule_row(token_rule(dict(ban=[1], ban_first=[69], ban_until=(3, [2, 33])), V))
    assert row == (ra, rb, 3, held[2]) and held[:2] == [ra, rb] and tm.users[ra] == 3
    rc = held[2]
    d = token_rule(dict(ban=[5]), V).always
    e = token_rule(dict(ban=[6]), V).always
    assert tm.room([d]) and not tm.room([d, e]) and tm.room([a, b, c, d])
    rd = tm.acquire(d)
    with pytest.raises(RuntimeError, match="4 different token masks are live"):
        tm.acquire(e)
    for r in (ra, ra, ra, rb, rb, rc):
        tm.release(r)
    assert sum(tm.users) == 1 and tm.users[rd] == 1
    before = tm.table[ra].clone()
    assert tm.acquire(a) == ra and torch.equal(tm.table[ra], before)          # a released row keeps its bitmap until it is needed
    tm.release(ra)
    re_ = tm.acquire(e)                                                        # ... and is rewritten only while it has no users
    assert re_ != rd and tm.table[re_].tolist() == [64, 0, 0, 0]
    with pytest.raises(ValueError, match="16 bytes"):
        tm.acquire(b"\0" * 8)


def test_abi_additions():
    for name in ("fo1_sample_rows_ruled_bf16", "fo1_decode_head_ruled_accept"):
        assert name in L.SIGNATURES and "_set_" not in name
    lib = L.load()
    assert lib.fo1_abi_version() == 9
    P_ = [4096 * (i + 1) for i in range(12)]      # fake device pointers: every call below is rejected before any HIP call
    LG, PAR, OUT, WS, SEEN, MASKS, RULES, ST, PLAN, IDS, DONE, _ = P_
    V = 4099                                       # ceil(V / 32) = 129 -> mask_ld_words >= 132

    def rows(**k):
        a = dict(logits=LG, ld=V, V=V, B=4, out=OUT, ldw=132, masks=MASKS, mask_rows=2, mld=132, rules=RULES)
        a.update(k)
        return lib.fo1_sample_rows_ruled_bf16(a["logits"], a["ld"], a["V"], a["B"], PAR, None, 1, None, a["out"], WS, 4096, SEEN, a["ldw"], a["masks"],
                                              a["mask_rows"], a["mld"], a["rules"], None)

    def accept(**k):
        a = dict(logits=LG, ld=V, V=V, B=4, state=ST, ldw=132, masks=MASKS, mask_rows=2, mld=132, rules=RULES)
        a.update(k)
        return lib.fo1_decode_head_ruled_accept(a["logits"], a["ld"], a["V"], a["B"], PAR, a["state"], PLAN, IDS, 8, None, 0, DONE, WS, 4096, SEEN,
                                                a["ldw"], a["masks"], a["mask_rows"], a["mld"], a["rules"], None)

    common = ((dict(B=0), b"B=0"), (dict(B=257), b"B=257"), (dict(ld=V - 1), b"ld_logits=4098"), (dict(V=0), b"n_vocab=0"), (dict(logits=None), b"NULL"),
              (dict(ldw=130), b"ld_words=130"), (dict(mld=129), b"mask_ld_words=129"), (dict(mld=130), b"mask_ld_words=130"), (dict(mld=128), b"mask_ld_words=128"),
              (dict(mld=0), b"mask_ld_words=0"), (dict(mask_rows=0), b"mask_rows=0"), (dict(mask_rows=-2), b"mask_rows=-2"), (dict(masks=MASKS + 2), b"4-byte aligned"))
    for call, prefix, own in ((rows, b"sample_rows_ruled", ((dict(out=None), b"NULL out"),)),
                              (accept, b"decode_head_ruled_accept", ((dict(state=None), b"bad arguments"),))):
        for kw, word in common + own:
            assert call(**kw) == -1, (prefix, kw)
            msg = lib.fo1_last_error()
            assert msg.startswith(prefix + b":") and word in msg, msg


def _model():
    m = FO1ForCausalLM.__new__(FO1ForCausalLM)
    m.config = FO1HFConfig({}, {"eos_token_id": [7, 9], "top_k": 20, "suppress_tokens": [1], "min_new_tokens": 5})
    return m


def test_generate_keywords_defaults_and_errors():
    sig = inspect.signature(FO1ForCausalLM.generate)
    for k in ("suppress_tokens", "begin_suppress_tokens", "bad_words_ids", "min_new_tokens", "allowed_token_ids"):
        assert sig.parameters[k].default is None, k
    rule, plan = FO1ForCausalLM._rule_plan, FO1ForCausalLM._decode_plan
    eos = (9, 7)
    assert rule({}, eos) is None and rule(dict(suppress_tokens=None, bad_words_ids=None, min_new_tokens=None), eos) is None
    assert rule(dict(min_new_tokens=0), eos) is None and rule(dict(suppress_tokens=[]), eos) is None
    assert plan({}, {"suppress_tokens": [1], "min_new_tokens": 5}, eos) is None       # the checkpoint's generation_config switches nothing on
    assert rule(dict(suppress_tokens=[5, 3, 5], bad_words_ids=[[8]]), eos) == dict(ban=(3, 5, 8))
    assert rule(dict(suppress_tokens=torch.tensor([4, 2])), eos) == dict(ban=(2, 4))
    assert rule(dict(begin_suppress_tokens=[2], allowed_token_ids=[4, 1], min_new_tokens=6), eos) == \
        dict(ban_first=(2,), allow=(1, 4), ban_until=(6, (7, 9)))                      # HF's rule: the EOS ids, not the stop keywords
    assert plan(dict(suppress_tokens=[3]), None, eos) == dict(greedy=True, ban=(3,))
    assert plan(dict(do_sample=True, temperature=0.7, seed=4, repetition_penalty=1.3, min_new_tokens=2), None, eos) == \
        dict(temperature=0.7, top_p=1.0, top_k=50, seed=4, repetition_penalty=1.3, ban_until=(2, (7, 9)))
    assert plan(dict(repetition_penalty=1.3), None, eos) == dict(greedy=True, repetition_penalty=1.3)
    with pytest.raises(NotImplementedError, match=r"\[4, 5\]"):
        rule(dict(bad_words_ids=[[3], [4, 5]]), eos)
    for bad, word in ((dict(min_new_tokens=-1), "min_new_tokens"), (dict(min_new_tokens=2.5), "min_new_tokens"), (dict(min_new_tokens=True), "min_new_tokens"),
                      (dict(suppress_tokens=[1.5]), "integers"), (dict(suppress_tokens=7), "list of token ids"), (dict(allowed_token_ids="ab"), "list of token ids")):
        with pytest.raises(ValueError, match=word):
            rule(bad, eos)
    m = _model()
    inp = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="single-token"):
        m.generate(inputs=inp, bad_words_ids=[[1, 2]])
    with pytest.raises(ValueError, match="min_new_tokens"):
        m.generate(inputs=inp, min_new_tokens=-3)
    with pytest.raises(ValueError, match="images"):      # a well-formed constrained call gets as far as an unconstrained one: to the request itself
        m.generate(inputs=inp, suppress_tokens=[3], min_new_tokens=2)


def test_batch_plan_on_batches_that_differ_only_in_the_new_keywords():
    m = _model()
    base = dict(max_new_tokens=8)
    # uniform in the keywords: every check of the plan passes, the requests themselves (there are none) are what fails
    for batch in ([dict(base, suppress_tokens=[3]), dict(base, suppress_tokens=[3])], [dict(base, min_new_tokens=2, bad_words_ids=[[3]])] * 2,
                  [dict(base, suppress_tokens=[3, 4]), dict(base, bad_words_ids=[[4], [3]])]):      # the same banned set, spelt differently
        with pytest.raises(ValueError, match="inputs"):
            m._batch_plan(batch)
    # mixed: refused without the pool ...
    for other in (dict(base, suppress_tokens=[3]), dict(base, begin_suppress_tokens=[3]), dict(base, min_new_tokens=2), dict(base, allowed_token_ids=[1, 2]),
                  dict(base, bad_words_ids=[[5]])):
        with pytest.raises(ValueError, match="token-rule keywords.*unless the decode pool is enabled"):
            m._batch_plan([base, other])
    with pytest.raises(ValueError, match="unless the decode pool is enabled"):
        m._batch_plan([dict(base, suppress_tokens=[3]), dict(base, suppress_tokens=[4])])
    # ... and taken with it (the plan gets as far as the requests)

    class _Eng:
        _pool_svc = object()
    m.engine = _Eng()
    with pytest.raises(ValueError, match="inputs"):
        m._batch_plan([base, dict(base, suppress_tokens=[3]), dict(base, min_new_tokens=2)])
    with pytest.raises(NotImplementedError, match="single-token"):
        m._batch_plan([base, dict(base, bad_words_ids=[[1, 2]])])


def test_the_loops_signatures_are_unchanged():
    from vlm_fo1_amd.llm import BatchDecoder, DecodePool
    from vlm_fo1_amd.model import FO1Engine
    from vlm_fo1_amd.serving import PoolGroup, PoolService
    assert list(inspect.signature(BatchDecoder.start).parameters) == ["self", "seqs", "deltas", "first_tokens", "max_new_tokens", "stop_ids", "sampling",
                                                                       "prompt_ids", "logprobs", "first_logprobs"]
    assert list(inspect.signature(DecodePool.join).parameters) == ["self", "kcache", "vtcache", "seqs", "deltas", "first_tokens", "max_new_tokens", "stop_ids",
                                                                    "tags", "sampling", "prompt_ids", "logprobs", "first_logprobs"]
    for fn in (PoolService.submit, PoolGroup.submit):
        assert list(inspect.signature(fn).parameters) == ["self", "src_llm", "seqs", "deltas", "first_tokens", "max_new_tokens", "stop_ids", "sampling",
                                                          "prompt_ids", "logprobs", "first_logprobs"]
    assert list(inspect.signature(FO1Engine.generate_batch).parameters)[-2:] == ["sampling", "logprobs"]
    assert list(inspect.signature(FO1Engine.submit_batch).parameters)[-3:] == ["sampling", "stream_base", "logprobs"]
    assert DecodePool.MAX_MASKS == 64
    assert inspect.signature(DecodePool.can_take).parameters["sampling"].default is None      # the old one-argument call still answers for stop sets
