"""Definition, oracle and cases of the steered decode head: a per-row additive logit bias and frequency / presence penalties in
sample_rows_kernel's STEER instantiations (vlm_fo1_amd/csrc/sample.hip, behind fo1_sample_rows_steered_bf16 and
fo1_decode_head_steered_accept).  Shared by tests/test_steer_cases.py (CPU), tests/test_steer_head_gpu.py and
tests/test_steer_decode_gpu.py (MI355X).

Definition (steer()).  b_i: the bf16 bias of token i (a zero entry, 0 or -0: none); n_i: how often the sequence has generated token i; f, q:
the frequency and presence penalties, on iff both are finite fp32 values and not both zero.  For a finite bf16 logit l_i, in this order:
    1. ban        a banned token becomes NaN bits (constraint_cases.mask); no later step touches a non-finite entry;
    2. bias       b_i != 0:   x = bf16_rne(fp32(l_i) + fp32(b_i))                       one fp32 add, one rounding;
    3. penalty    the repetition penalty on x for the tokens of `seen` (penalty_cases.penalise);
    4. counts     n_i > 0:    t = fp32(f) * fp32(n_i);  t = t + fp32(q);  x = bf16_rne(x - t)   three fp32 operations, each rounded on its own.
A result that is not finite counts as a non-finite entry.  The sampler's definition (sampling_cases.oracle) or the greedy pick
(penalty_cases.greedy_pick) then applies to x.  Step 2 is HF's SequenceBiasLogitsProcessor (single-token sequences) in front of the
repetition penalty, with the score rounded back to bf16; step 4 is the OpenAI / vLLM formula l - f n - q [n > 0] over generated tokens.

Tolerance.  The device forms the same fixed-order fp32 partial sums as without a steer, over transformed keys: the accept rule and
EPS = 2^-17 of tests/sampling_cases.py hold unchanged.  As in constraint_cases, a (row, kind) pair whose steered oracle keeps less than
EXACT_MARGIN * EPS between the mass above a key and top_p Z1 is left out, decided on the oracle alone; at most MAX_LEFT_OUT = 5 % of the
pairs may be left out (left_out()).

Cases (cases()).  Every row of sampling_cases.rows_and_batches() at V in {63, 4099, 32773} crossed with the six kinds of KINDS: a bias of -4 on
the row's argmax; +1.5 on every 8th id and the byte / word boundaries 7, 8, 9, 31, 32, 33, V - 1; +8 on the unaligned last groups; counts
1 + id % 3 on the 50 largest with f = 0.25, q = 0.5; presence only (counts 1 on every 32nd id, f = 0, q = 1); and the second and fourth with a
repetition penalty of 1.3 on every 32nd id, all together.  Plus one N(0, 3) row at V = 151936 with the second and fourth kind.  Greedy rows:
greedy_cases()."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

import constraint_cases as C
import penalty_cases as P
import sampling_cases as S

KINDS = ("bias-argmax", "bias-every8", "bias-tail", "counts-top50", "presence-every32", "all-together")
CASE_V = (63, 4099, 32773)
BIG_V = 151936
MAX_LEFT_OUT = C.MAX_LEFT_OUT


def _f32(b) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def count_on(f, q) -> bool:
    f, q = np.float32(f), np.float32(q)
    return bool(np.isfinite(f) and np.isfinite(q) and (f != 0 or q != 0))


def bias_bits(bias: Optional[Dict[int, float]], V: int) -> np.ndarray:
    """A bias {id: value} as the row of the bias table: uint16 [V] bf16 bits, each value rounded once to bf16, 0 elsewhere."""
    row = np.zeros(V, np.uint16)
    for i, v in (bias or {}).items():
        row[int(i)] = S.to_bits(np.float32(v))
    return row


def add_bias(bits, brow) -> np.ndarray:
    """Step 2 on bf16 bits: brow is the bias row as bf16 bits."""
    bits, brow = np.asarray(bits, np.uint16), np.asarray(brow, np.uint16)
    l, b = _f32(bits), _f32(brow)
    with np.errstate(over="ignore", invalid="ignore"):
        x = (l + b).astype(np.float32)
    hit = np.isfinite(l) & ((brow & 0x7fff) != 0)
    return np.where(hit, S.to_bits(x), bits).astype(np.uint16)


def sub_counts(bits, counts, f, q) -> np.ndarray:
    """Step 4 on bf16 bits: counts is an integer array [V]."""
    bits = np.asarray(bits, np.uint16)
    n = np.asarray(counts, np.int64)
    if not count_on(f, q) or not (n > 0).any():
        return bits.copy()
    x = _f32(bits)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = (np.float32(f) * n.astype(np.float32)).astype(np.float32)
        t = (t + np.float32(q)).astype(np.float32)
        y = (x - t).astype(np.float32)
    hit = np.isfinite(x) & (n > 0)
    return np.where(hit, S.to_bits(y), bits).astype(np.uint16)


def counts_row(counts: Optional[Dict[int, int]], V: int) -> np.ndarray:
    row = np.zeros(V, np.int64)
    for i, n in (counts or {}).items():
        row[int(i)] = int(n)
    return row


def steer(bits, bias=None, counts=None, f=0.0, q=0.0, banned=(), seen=(), p=0.0) -> np.ndarray:
    """What every pass of the steered head keys: bias {id: value} (or a bias row as uint16 bits), counts {id: n} (or an integer array)."""
    bits = np.asarray(bits, np.uint16)
    V = len(bits)
    brow = bias if isinstance(bias, np.ndarray) else bias_bits(bias, V)
    crow = counts if isinstance(counts, np.ndarray) else counts_row(counts, V)
    x = add_bias(C.mask(bits, banned), brow)
    x = P.penalise(x, seen, p)
    return sub_counts(x, crow, f, q)


def kind_steer(kind: str, bits: np.ndarray) -> dict:
    """The steer of a case kind on a row: dict(bias={id: value}, counts={id: n}, f, q, seen, p)."""
    out = dict(bias={}, counts={}, f=0.0, q=0.0, seen=np.zeros(0, np.int64), p=0.0)
    if kind in ("bias-argmax",):
        out["bias"] = {P.greedy_pick(bits): -4.0}
    if kind in ("bias-every8", "all-together"):
        out["bias"] = {int(i): 1.5 for i in C.ban_set("every8", bits)}
    if kind == "bias-tail":
        out["bias"] = {int(i): 8.0 for i in C.ban_set("tail", bits)}
    if kind in ("counts-top50", "all-together"):
        out.update(counts={int(i): 1 + int(i) % 3 for i in C.ban_set("top50", bits)}, f=0.25, q=0.5)
    if kind == "presence-every32":
        out.update(counts={int(i): 1 for i in P.seen_set("every32", bits)}, f=0.0, q=1.0)
    if kind == "all-together":
        out.update(seen=P.seen_set("every32", bits), p=1.3)
    return out


_cache: dict = {}


def _case(name, bits, kind, T, top_p, top_k, rng, planted=False):
    st = kind_steer(kind, bits)
    sb = steer(bits, **st)
    o = S.oracle(sb, T, top_p, top_k)
    return dict(name=f"{name}|{kind}", V=len(bits), bits=bits, kind=kind, T=T, top_p=top_p, top_k=top_k, sbits=sb, oracle=o,
                draws=None if o.margin < S.EXACT_MARGIN * S.EPS else S._draws(o, len(bits), rng, planted), **st)


def cases() -> List[dict]:
    """dicts(name, V, bits, kind, bias, counts, f, q, seen, p, T, top_p, top_k, sbits = steer(bits, ...), oracle = the sampler's on it, draws)."""
    if "c" in _cache:
        return _cache["c"]
    rows, _ = S.rows_and_batches()
    out, pairs, left = [], 0, []
    for V in CASE_V:
        rng = np.random.default_rng(11000 + V)
        for r in (r for r in rows if r["V"] == V):
            for kind in KINDS:
                c = _case(r["name"], r["bits"], kind, r["T"], r["top_p"], r["top_k"], rng, "planted" in r["name"])
                pairs += 1
                if c["draws"] is None:      # the steered row's top-p cut-off sits within 16 EPS of top_p Z1: left out, and counted
                    left.append(c["name"])
                    continue
                out.append(c)
    rng = np.random.default_rng(11000 + BIG_V)
    x = (rng.standard_normal(BIG_V) * 3).astype(np.float32)
    for kind, top_k in (("bias-every8", 50), ("counts-top50", 0)):
        c = _case(f"V{BIG_V}-normal", S.to_bits(x), kind, 1.0, 1.0, top_k, rng)
        assert c["draws"] is not None
        out.append(c)
    _cache["c"] = out
    _cache["left"] = (left, pairs)
    return out


def left_out():
    """-> (names of the (row, kind) pairs left out for their top-p margin, number of pairs)."""
    cases()
    return _cache["left"]


def contraction_probe():
    """(f, n, q) with fma(f, n, q) != fl(fl(f * n) + q) in fp32, and both values as fp32: f * n = 3 + 3 * 2^-23 needs 25 bits and ties to even
    3 + 2^-21 (exact: 3 + 1.5 * 2^-22); with q = -3 the unfused sum is 2^-21 = 4.76837158e-07, the fused one 1.5 * 2^-22 = 3.57627869e-07."""
    f, n, q = np.float32(1 + 2.0 ** -23), 3, np.float32(-3.0)
    unfused = np.float32(np.float32(f * np.float32(n)) + q)
    fused = np.float32(np.float64(f) * n + np.float64(q))      # (exact in fp64: one rounding)
    assert unfused != fused
    return f, n, q, unfused, fused


def _gcase(name, x, bias=None, counts=None, f=0.0, q=0.0, banned=(), seen=(), p=0.0):
    bits = x if isinstance(x, np.ndarray) and x.dtype == np.uint16 else S.to_bits(np.asarray(x, np.float32))
    st = dict(bias=dict(bias or {}), counts=dict(counts or {}), f=f, q=q, banned=np.asarray(list(banned), np.int64),
              seen=np.asarray(list(seen), np.int64), p=p)
    return dict(name=name, V=len(bits), bits=bits, want=P.greedy_pick(steer(bits, **st)), **st)


def greedy_cases() -> List[dict]:
    """dicts(name, V, bits, bias, counts, f, q, banned, seen, p, want = greedy_pick(steer(bits, ...)))."""
    if "g" in _cache:
        return _cache["g"]
    out = []
    for V in CASE_V:
        rng = np.random.default_rng(11500 + V)
        x = (rng.standard_normal(V) * 2).astype(np.float32)
        a, b, c = sorted({7, V // 2, V - 1})
        y = x.copy()
        y[[a, b, c]] = [20.0, 18.5, 18.0]
        out.append(_gcase(f"V{V}-plain", y))
        out.append(_gcase(f"V{V}-bias-moves-argmax", y, {a: -2.0}))                                 # 18 < 18.5: the runner-up
        out.append(_gcase(f"V{V}-bias-raises-last", y, {c: 2.5}))                                   # 20.5 at V - 1, the unaligned tail
        out.append(_gcase(f"V{V}-bias-minus-zero", y, {a: -0.0, b: 0.0}))                           # zero entries: no bias
        t = x.copy()
        t[[a, b, c]] = 20.0
        out.append(_gcase(f"V{V}-tie-broken-by-bias", t, {b: 0.125}))                               # 20.125 is a bf16 value: the second tied id
        out.append(_gcase(f"V{V}-tie-bias-rounds-away", t, {b: 0.03125}))                           # 20 + 2^-5 ties to even 20: still the first
        out.append(_gcase(f"V{V}-count-n0", y, None, {}, 1.0, 1.0))                                 # nothing generated: the leader stays
        out.append(_gcase(f"V{V}-count-n1", y, None, {a: 1}, 1.0, 1.0))                             # 20 - 2 = 18 < 18.5
        out.append(_gcase(f"V{V}-count-frequency", y, None, {a: 3, b: 1}, 0.75, 0.0))               # 17.75 each: the untouched 18 wins
        out.append(_gcase(f"V{V}-count-off-nan", y, None, {a: 5}, np.nan, 1.0))                     # a non-finite penalty: off
        out.append(_gcase(f"V{V}-count-off-inf", y, None, {a: 5}, 1.0, np.inf))
        out.append(_gcase(f"V{V}-count-negative-boosts", y, None, {c: 2}, -1.5, 0.0))               # 18 + 3 = 21
        h = x.copy()
        h[11], h[12] = 3.0e38, 9.0
        out.append(_gcase(f"V{V}-bias-overflows", h, {11: 3.0e38}))                                 # inf: the entry drops out
        out.append(_gcase(f"V{V}-count-overflows", -h, None, {11: 1}, 3.0e38, 0.0))                 # -inf likewise
        w = y.copy()
        w[a], w[b], w[c] = np.nan, np.inf, -np.inf
        out.append(_gcase(f"V{V}-nonfinite-biased", w, {a: 1.0, b: -1.0, c: 1.0}, {a: 1, b: 1, c: 1}, 1.0, 1.0))
        out.append(_gcase(f"V{V}-banned-and-biased", y, {a: 50.0}, banned=[a]))                     # stays banned
        out.append(_gcase(f"V{V}-bias-penalty-counts", y, {a: 4.0}, {a: 2}, 1.0, 0.5, seen=[a], p=1.5))      # (24 / 1.5) - 2.5 = 13.5
        out.append(_gcase(f"V{V}-everything-banned", y, {a: 1.0}, {a: 1}, 1.0, 1.0, banned=np.arange(V)))    # id 0
        # the contraction probe: x = 2^-21 at `a`, 2^-24 at `b`.  The unfused t = 2^-21 leaves 0 at `a` and `b` wins; a fused multiply-add
        # would give t = 1.5 * 2^-22, leave 2^-23 at `a`, and `a` would win (tests/test_steer_cases.py checks both)
        f, n, q, unfused, fused = contraction_probe()
        z = np.full(V, -1.0, np.float32)
        z[a] = unfused
        z[b] = np.float32(2.0 ** -24)
        out.append(_gcase(f"V{V}-no-fused-multiply-add", z, None, {a: n}, float(f), float(q)))
    _cache["g"] = out
    return out
