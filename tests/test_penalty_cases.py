"""CPU checks of tests/penalty_cases.py and of the general head's parameter row: penalise() against HF's
RepetitionPenaltyLogitsProcessor, the conditions the cases must meet (on the oracle alone), the greedy pick, the host bitmap, and the packing
of ops.sample_params rows of 5 and of 7 fields."""
import struct

import numpy as np
import pytest

import penalty_cases as P
import sampling_cases as S


def test_penalise_matches_the_transformers_processor_rounded_to_bf16():
    """HF applies score < 0 ? score * p : score / p to the seen ids of fp32 scores and keeps the fp32 result; rounded to bf16 it is penalise():
    the same bits on every finite entry, hence the same kept set, and softmax probabilities equal to 1e-12 in fp64 from the rounded values."""
    torch = pytest.importorskip("torch")
    try:
        from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    except Exception as e:      # noqa: BLE001
        pytest.skip(f"transformers has no RepetitionPenaltyLogitsProcessor here ({e})")
    n = 0
    for c in P.cases():
        if c["V"] > 4099 or not len(c["seen"]):
            continue
        scores = torch.from_numpy(S.from_bits(c["bits"]).astype(np.float32)).unsqueeze(0)
        fin = np.isfinite(S.from_bits(c["bits"]))
        hf = RepetitionPenaltyLogitsProcessor(penalty=float(np.float32(c["p"])))(torch.from_numpy(c["seen"]).unsqueeze(0), scores.clone())[0]
        hf_bits = S.to_bits(hf.numpy())
        assert (hf_bits[fin] == c["pbits"][fin]).all(), c["name"]
        assert (c["pbits"][~fin] == c["bits"][~fin]).all(), c["name"]      # a non-finite entry is left alone
        # kept set and probabilities from the rounded values (non-finite entries have no weight on either side)
        theirs = np.where(fin, hf_bits, c["bits"])
        o, h = c["oracle"], S.oracle(theirs, c["T"], c["top_p"], c["top_k"])
        assert o.empty == h.empty
        if not o.empty:
            assert (o.K == h.K).all(), c["name"]
            assert np.abs(o.w / o.z2 - h.w / h.z2).max() <= 1e-12, c["name"]
        n += 1
    assert n >= 40


def test_cases_cover_every_pair_and_keep_the_top_p_margin():
    cs = P.cases()
    for V in P.CASE_V:
        have = {(c["name"].split("|")[1], c["p"]) for c in cs if c["V"] == V}
        assert have == set(P.PAIRS), (V, set(P.PAIRS) - have)
    assert any(c["V"] == P.BIG_V for c in cs)
    for c in cs:
        assert c["oracle"].margin >= S.EXACT_MARGIN * S.EPS, c["name"]
        assert len(c["draws"]) >= 3
    exact = sum(S.is_exact(c["oracle"], u) for c in cs for u in c["draws"])
    total = sum(len(c["draws"]) for c in cs)
    print(f"\n{len(cs)} penalised rows ({P._cache['skipped']} pairs replaced for their top-p margin), {total} draws of which {exact} exact")
    assert exact > total - exact > 0
    # the penalty does something: most cases with a non-empty seen set change bits, and some change the kept set
    changed = [c for c in cs if len(c["seen"]) and (c["pbits"] != c["bits"]).any()]
    assert len(changed) >= len([c for c in cs if len(c["seen"])]) * 3 // 4
    assert any((c["oracle"].K != S.oracle(c["bits"], c["T"], c["top_p"], c["top_k"]).K).any() for c in changed)


def test_penalise_definition():
    bits = S.to_bits(np.array([2.0, -2.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e38, 1.0, 1.0], np.float32))
    seen = [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, -200, 10, 15]      # duplicates and ids outside the row are fine
    got = S.from_bits(P.penalise(bits, seen, 2.0))
    assert got[:4].tolist() == [1.0, -4.0, 0.0, 0.0] and np.signbit(got[3]) and got[4] == np.inf and got[5] == -np.inf and np.isnan(got[6])
    assert got[7] == np.float64(np.float32(1.5e38).astype(np.float32)) or abs(got[7] - 1.5e38) / 1.5e38 < 2 ** -8
    assert got[8] == 0.5 and got[9] == 1.0
    assert np.isinf(S.from_bits(P.penalise(bits, seen, 0.5))[7])            # 3e38 / 0.5 overflows: counts as non-finite
    assert S.key(P.penalise(bits, seen, 0.5))[7] == -1
    for off in (0.0, 1.0, -1.3, float("nan"), float("inf")):
        assert (P.penalise(bits, seen, off) == bits).all() and not P.penalty_on(off)
    # rounding: 1 / 1.3 in fp32, to nearest even bf16
    one = S.to_bits(np.array([1.0], np.float32))
    q = np.float32(1.0) / np.float32(1.3)
    assert P.penalise(one, [0], 1.3)[0] == S.to_bits(np.array([q]))[0]
    assert P.greedy_pick(S.to_bits(np.array([1.0, 3.0, 3.0, np.inf, np.nan], np.float32))) == 1
    assert P.greedy_pick(S.to_bits(np.array([np.nan, -np.inf], np.float32))) == 0
    assert P.greedy_pick(S.to_bits(np.array([-0.0, 0.0, -1.0], np.float32))) == 0      # -0 = +0: the first


def test_greedy_cases_say_what_they_claim():
    g = {c["name"]: c for c in P.greedy_cases()}
    for V in (63, 4099, 32773):
        ties = sorted({7, V // 2, V - 1})
        assert g[f"V{V}-ties"]["want"] == ties[0] and g[f"V{V}-ties-first-seen"]["want"] == ties[1]
        assert g[f"V{V}-ties-all-seen"]["want"] == ties[0] and g[f"V{V}-ties-penalty-off"]["want"] == ties[0]
        assert g[f"V{V}-moves-argmax"]["want"] == ties[1] and g[f"V{V}-boost"]["want"] == ties[-1]
        assert g[f"V{V}-negative"]["want"] == V // 4
        assert g[f"V{V}-no-finite-entry"]["want"] == 0 and g[f"V{V}-overflow"]["want"] != 11
    assert len(g) >= 60


def test_host_bitmap_layout():
    bm = P.host_bitmap([[0, 31, 32, 33, 62, -200, 63, 64, 63], []], 63)
    assert bm.shape == (2, 4) and bm[0].tolist() == [0x80000001, 0x40000003, 0, 0] and not bm[1].any()
    assert P.seen_words(151936) == 4748 and P.seen_words(63) == 4 and P.seen_words(4099) == 132 and P.seen_words(128) == 4 and P.seen_words(129) == 8


def test_sample_params_rows_of_five_keep_their_bytes_and_rows_of_seven_fill_words_6_and_7():
    from vlm_fo1_amd import ops
    rows5 = [(0.7, 0.9, 50, 0xfedcba9876543210, 3), (1.5, 1.0, 0, 7, 0xffffffff)]
    want = b"".join(struct.pack("<ffiIIIII", t, p, k, seed & 0xffffffff, seed >> 32, st, 0, 0) for t, p, k, seed, st in rows5)
    tab = ops.sample_params(rows5)
    assert tab.shape == (2, 8) and tab.numpy().tobytes() == want
    tab7 = ops.sample_params([r + (False, None) for r in rows5] + [rows5[0] + (True, 1.3), rows5[1] + (False, 0.5), rows5[0] + (1, 0)])
    b7 = tab7.numpy().tobytes()
    assert b7[:64] == want                                                    # greedy off, no penalty: today's bytes
    w = np.frombuffer(b7, np.uint32).reshape(-1, 8)
    assert w[2, 6] == 1 and w[3, 6] == 0 and w[4, 6] == 1 and (w[2:, :6] == w[[0, 1, 0], :6]).all()
    f = np.frombuffer(b7, np.float32).reshape(-1, 8)
    assert f[2, 7] == np.float32(1.3) and f[3, 7] == 0.5 and f[4, 7] == 0.0
    with pytest.raises(ValueError):
        ops.sample_params([(1.0, 1.0, 0, 0, 0, True)])
    assert ops.sampling_row(None) == (0.0, 1.0, 0, 0, 0, True, 0.0)
    assert ops.sampling_row(dict(greedy=True, repetition_penalty=1.3), 5) == (0.0, 1.0, 0, 0, 5, True, 1.3)
    assert ops.sampling_row(dict(temperature=0.7, top_p=0.9, top_k=50, seed=9, stream=2), 5) == (0.7, 0.9, 50, 9, 2, False, 0.0)
    with pytest.raises(ValueError):
        ops.sampling_row(dict(top_k=5))
    assert ops.seen_words(151936) == P.seen_words(151936) and ops.seen_words(63) == 4
    assert [ops.penalty_on(p) for p in (None, 0, 1.0, 1.3, 0.5, float("nan"), float("inf"), -2.0)] == [False, False, False, True, True, False, False, False]


def test_plug_in_repetition_penalty_argument():
    from vlm_fo1.model.fo1_model import FO1ForCausalLM
    pen, plan = FO1ForCausalLM._penalty_plan, FO1ForCausalLM._decode_plan
    assert pen({}) is None and pen(dict(repetition_penalty=None)) is None and pen(dict(repetition_penalty=1.0)) is None
    assert pen(dict(repetition_penalty=1.3)) == 1.3 and pen(dict(repetition_penalty=np.float32(0.5))) == 0.5
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), True, "x", 1e39):
        with pytest.raises(ValueError, match="repetition_penalty"):
            pen(dict(repetition_penalty=bad))
    assert plan({}, {"repetition_penalty": 1.05}) is None                     # the checkpoint's generation_config does not switch it on
    assert plan(dict(repetition_penalty=1.3), None) == dict(greedy=True, repetition_penalty=1.3)
    assert plan(dict(do_sample=True, temperature=0.7, seed=4, repetition_penalty=1.3), None) == \
        dict(temperature=0.7, top_p=1.0, top_k=50, seed=4, repetition_penalty=1.3)
    assert plan(dict(do_sample=True, temperature=0.7, seed=4), None) == dict(temperature=0.7, top_p=1.0, top_k=50, seed=4)
