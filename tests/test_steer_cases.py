"""CPU checks of tests/steer_cases.py, the definition the steered decode head is held to on the MI355X: steer() against answers written out
by hand and against a plain scalar restatement, the bias step against HF's SequenceBiasLogitsProcessor, the contraction probe, the cap
on the pairs left out, and the case lists themselves."""
import numpy as np
import pytest

import constraint_cases as C
import penalty_cases as P
import sampling_cases as S
import steer_cases as T


def _bits(*xs):
    return S.to_bits(np.array(xs, np.float32))


def _vals(bits):
    return S.from_bits(bits).tolist()


def test_known_answers_written_out_by_hand():
    row = _bits(20.0, 18.5, 18.0, -1.0, 0.5)
    # bias: 20 - 2 = 18;  18 + 0.125 = 18.125 (a bf16 value);  -1 + 0.5 = -0.5
    assert _vals(T.steer(row, {0: -2.0, 2: 0.125, 3: 0.5})) == [18.0, 18.5, 18.125, -0.5, 0.5]
    # 18 + 2^-5 lies halfway between 18 and 18.0625 = 18 + 2^-4: ties to even, 18
    assert _vals(T.steer(row, {2: 0.03125}))[2] == 18.0
    # a bias is rounded to bf16 once, first: 0.1 -> 0.10009765625;  0.5 + 0.10009765625 = 0.60009765625 -> bf16 0.6015625
    assert _vals(T.steer(row, {4: 0.1}))[4] == 0.6015625
    # counts: f = 0.25, q = 0.5: n = 1 -> 0.75, n = 3 -> 1.25;  20 - 0.75 = 19.25, 18.5 - 1.25 = 17.25; n = 0 untouched
    assert _vals(T.steer(row, None, {0: 1, 1: 3}, 0.25, 0.5)) == [19.25, 17.25, 18.0, -1.0, 0.5]
    # presence only, frequency only, a negative penalty (a boost)
    assert _vals(T.steer(row, None, {0: 7}, 0.0, 1.0))[0] == 19.0
    assert _vals(T.steer(row, None, {0: 4}, 0.5, 0.0))[0] == 18.0
    assert _vals(T.steer(row, None, {3: 2}, -1.5, 0.0))[3] == 2.0
    # the order: bias, then the repetition penalty, then the counts: ((20 + 4) / 1.5) - (1 * 2 + 0.5) = 13.5
    assert _vals(T.steer(row, {0: 4.0}, {0: 2}, 1.0, 0.5, seen=[0], p=1.5))[0] == 13.5
    # (counts first and the penalty last would give (20 + 4 - 2.5) / 1.5 = 14.33; the penalty first and the bias second 20 / 1.5 + 4 - 2.5 = 14.83)
    # a negative logit: the bias can change the branch the penalty takes: -1 + 3 = 2 -> 2 / 2 = 1 (not -1 * 2 + 3)
    assert _vals(T.steer(row, {3: 3.0}, seen=[3], p=2.0))[3] == 1.0
    # off: a non-finite or an all-zero pair of penalties, zero entries of the bias (0 and -0)
    for f, q in ((np.nan, 1.0), (1.0, np.inf), (0.0, 0.0), (-0.0, 0.0)):
        assert (T.steer(row, None, {0: 3}, f, q) == row).all(), (f, q)
    assert (T.steer(row, {0: 0.0, 1: -0.0}) == row).all()
    # a ban comes first and stays: nothing touches a non-finite entry
    out = T.steer(row, {0: 50.0}, {0: 1}, 1.0, 1.0, banned=[0], seen=[0], p=2.0)
    assert out[0] == C.NAN_BITS and (out[1:] == row[1:]).all()


def test_non_finite_entries_and_overflow():
    row = np.array([0x7f80, 0xff80, 0x7fc0, 0xffc1], np.uint16)      # +inf, -inf, two NaNs
    row = np.concatenate([row, _bits(3.0e38, -3.0e38, 1.0)])
    out = T.steer(row, {i: 1.0 for i in range(4)}, {i: 2 for i in range(4)}, 1.0, 1.0)
    assert (out[:4] == row[:4]).all(), "a non-finite entry was touched"
    # sums that overflow: the result is not finite and has no key
    over = T.steer(row, {4: 3.0e38}, {5: 1}, 3.0e38, 0.0)
    assert S.key(over)[4] == -1 and S.key(over)[5] == -1 and S.key(over)[6] >= 0
    assert P.greedy_pick(over) == 6


def _scalar(l_bits, b_bits, n, f, q, seen, p, banned):
    """One entry, step by step, in numpy float32 scalars alone (no float64 anywhere) — a restatement that shares no code with steer()."""
    F = np.float32

    def val(h):
        return np.array([h << 16], np.uint32).view(np.float32)[0]

    def bf16(x):
        if np.isnan(x):
            return 0x7fc0
        u = int(np.array([x], np.float32).view(np.uint32)[0])
        return ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff

    def finite(h):
        return (h & 0x7f80) != 0x7f80

    h = l_bits
    if banned:
        return C.NAN_BITS
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if finite(h) and (b_bits & 0x7fff):
            h = bf16(val(h) + val(b_bits))
        if finite(h) and seen and P.penalty_on(p):
            x = val(h)
            h = bf16(x * F(p) if x < 0 else x / F(p))
        if finite(h) and n > 0 and T.count_on(f, q):
            t = F(f) * F(n)
            t = t + F(q)
            h = bf16(val(h) - t)
    return h


def test_steer_equals_a_scalar_restatement_on_random_rows():
    rng = np.random.default_rng(3)
    V = 257
    for trial in range(40):
        x = (rng.standard_normal(V) * (10.0 ** rng.integers(-3, 4))).astype(np.float32)
        x[rng.integers(0, V, 4)] = [np.inf, -np.inf, np.nan, 0.0]
        bits = S.to_bits(x)
        bias = {int(i): float(np.float32(rng.standard_normal() * 5)) for i in rng.choice(V, 60, replace=False)}
        counts = {int(i): int(rng.integers(1, 4097)) for i in rng.choice(V, 60, replace=False)}
        f, q = float(np.float32(rng.standard_normal())), float(np.float32(rng.standard_normal()))
        seen = rng.choice(V, 50, replace=False)
        banned = rng.choice(V, 20, replace=False)
        p = float(rng.choice([0.0, 0.5, 1.3, 2.0]))
        got = T.steer(bits, bias, counts, f, q, banned=banned, seen=seen, p=p)
        brow = T.bias_bits(bias, V)
        for i in range(V):
            want = _scalar(int(bits[i]), int(brow[i]), counts.get(i, 0), f, q, i in set(seen.tolist()), p, i in set(banned.tolist()))
            assert int(got[i]) == want, (trial, i)


def test_the_contraction_probe_tells_a_fused_multiply_add_from_the_definition():
    f, n, q, unfused, fused = T.contraction_probe()
    assert float(unfused) == 2.0 ** -21 and float(fused) == 1.5 * 2.0 ** -22
    for g in (g for g in T.greedy_cases() if g["name"].endswith("no-fused-multiply-add")):
        a = int(np.argmax(S.from_bits(g["bits"])))
        sb = T.steer(g["bits"], g["bias"], g["counts"], g["f"], g["q"])
        assert S.from_bits(sb)[a] == 0.0 and g["want"] != a and g["want"] == P.greedy_pick(sb)
        # what a contracted f * n + q would leave at `a`: 2^-21 - 1.5 * 2^-22 = 2^-23 > 2^-24, and `a` would win
        wrong = g["bits"].copy()
        wrong[a] = S.to_bits(np.float32(np.float32(unfused) - np.float32(fused)))
        assert P.greedy_pick(wrong) == a


def test_bias_step_equals_hf_sequence_bias_on_bf16_scores():
    torch = pytest.importorskip("torch")
    try:
        from transformers import SequenceBiasLogitsProcessor
    except Exception:
        pytest.skip("transformers does not import")
    rng = np.random.default_rng(11)
    V = 1000
    bits = S.to_bits((rng.standard_normal(V) * 4).astype(np.float32))
    bias = {int(i): float(S.from_bits(S.to_bits(np.float32(rng.standard_normal() * 3)))) for i in rng.choice(V, 100, replace=False)}
    proc = SequenceBiasLogitsProcessor(sequence_bias={(i,): v for i, v in bias.items()})
    scores = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).reshape(1, V)
    out = proc(torch.zeros(1, 3, dtype=torch.long), scores.float()).to(torch.bfloat16)      # fp32 add, one rounding to bf16
    want = out.view(torch.int16).numpy().view(np.uint16)[0]
    assert (T.steer(bits, bias) == want).all()


def test_at_most_five_percent_of_the_pairs_are_left_out():
    left, pairs = T.left_out()
    assert pairs == 6 * len([r for r in S.rows_and_batches()[0] if r["V"] in T.CASE_V]) == 684
    assert len(left) <= T.MAX_LEFT_OUT * pairs, left
    assert len(left) == 3 and all(n.startswith("V32773") for n in left), left
    print(f"\n{len(left)} of {pairs} pairs left out: {left}")


def test_case_lists():
    cs = T.cases()
    assert {c["kind"] for c in cs} == set(T.KINDS) and {c["V"] for c in cs} == set(T.CASE_V) | {T.BIG_V}
    assert sum(c["V"] == T.BIG_V for c in cs) == 2
    for c in cs:
        assert c["draws"] and c["oracle"].margin >= S.EXACT_MARGIN * S.EPS
        assert (c["sbits"] == T.steer(c["bits"], c["bias"], c["counts"], c["f"], c["q"], seen=c["seen"], p=c["p"])).all()
    moved = sum((c["sbits"] != c["bits"]).any() for c in cs)
    assert moved >= 0.98 * len(cs), "the steers change next to nothing"      # (a row without a finite entry stays as it is under every steer)
    every8 = next(c for c in cs if c["kind"] == "bias-every8" and c["V"] == 4099)
    assert {7, 8, 9, 31, 32, 33, 4098} <= set(every8["bias"])
    tail = next(c for c in cs if c["kind"] == "bias-tail" and c["V"] == 4099)
    assert sorted(tail["bias"]) == list(range(4088, 4099))
    top = next(c for c in cs if c["kind"] == "counts-top50" and c["V"] == 4099)
    assert len(top["counts"]) == 50 and set(top["counts"].values()) == {1, 2, 3} and (top["f"], top["q"]) == (0.25, 0.5)
    gs = T.greedy_cases()
    names = {g["name"].split("-", 1)[1] for g in gs}
    assert {"bias-moves-argmax", "tie-broken-by-bias", "count-n0", "count-n1", "bias-overflows", "nonfinite-biased", "banned-and-biased",
            "no-fused-multiply-add"} <= names
    by = {g["name"]: g for g in gs}
    for V in T.CASE_V:
        a, b = sorted({7, V // 2, V - 1})[:2]
        assert by[f"V{V}-plain"]["want"] == a == by[f"V{V}-count-n0"]["want"] == by[f"V{V}-tie-bias-rounds-away"]["want"]
        assert by[f"V{V}-bias-moves-argmax"]["want"] == b == by[f"V{V}-tie-broken-by-bias"]["want"] == by[f"V{V}-count-n1"]["want"]
        assert by[f"V{V}-banned-and-biased"]["want"] == b and by[f"V{V}-everything-banned"]["want"] == 0
        assert by[f"V{V}-bias-overflows"]["want"] == 12
