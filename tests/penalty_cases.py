"""Definition, oracle and cases of the general decode head: the repetition penalty and the greedy row of sample_rows_kernel's PEN
instantiations (vlm_fo1_amd/csrc/sample.hip, behind fo1_sample_rows_seen_bf16 and fo1_decode_head_accept).  Shared by
tests/test_penalty_cases.py (CPU), tests/test_decode_head_gpu.py and tests/test_pool_sampling_gpu.py (MI355X).

Definition (penalise()).  For a row with the penalty p on (p finite, > 0, != 1), a seen token i and a finite logit l_i:
    l'_i = bf16_rne( l_i < 0 ? fp32(l_i) * p : fp32(l_i) / p )          (IEEE fp32 product / quotient, then round to nearest even)
unseen or non-finite entries are unchanged, a penalised value that is not finite counts as a non-finite entry (weight 0, never kept).  The
sampler's definition (sampling_cases.oracle) or the greedy pick (greedy_pick(): the first index, in vocabulary order, of the largest finite
entry; a row without one gives id 0) then applies to l' in place of l.  This is HF's RepetitionPenaltyLogitsProcessor in front of the warpers
with the score rounded back to bf16 (tests/test_penalty_cases.py compares).

Tolerance.  The device forms the same fixed-order fp32 partial sums as without a penalty, over transformed keys: the accept rule and
EPS = 2^-17 of tests/sampling_cases.py hold unchanged, and as there a case's top-p cut-off keeps 16 EPS between the mass above each key and
top_p Z1 — on the penalised oracle alone; a (seen set, p) pair that does not is replaced by the next pair of the cycle (cases()).

Cases (cases()).  Every row of sampling_cases.rows_and_batches() at V in {63, 4099, 32773} takes three of the 20 (seen set, p) pairs, cycling
so that each V sees every pair: seen sets = empty, one token, the row's argmax, every 32nd token plus the word-boundary neighbours 31, 32, 33,
V - 1, and all tokens; p in {0.5, 1.05, 1.3, 2.0}.  Plus one N(0, 3) row at V = 151936.  Greedy rows (greedy_cases()): the same rows with
their first pair, rows with ties at the maximum (the first index must win, also when the penalty removes the first of them), a row whose
penalty moves the argmax to the runner-up, an all-negative row (the penalty multiplies), rows with -inf, NaN and +inf entries, a row
without a finite entry, and a row whose penalised leader overflows to inf and drops out."""
from __future__ import annotations

from typing import List

import numpy as np

import sampling_cases as S

PENALTIES = (0.5, 1.05, 1.3, 2.0)
SEEN_KINDS = ("empty", "one", "argmax", "every32", "all")
CASE_V = (63, 4099, 32773)
BIG_V = 151936


def penalty_on(p) -> bool:
    p = np.float32(p)
    return bool(np.isfinite(p) and p > 0 and p != 1)


def penalise(bits, seen_ids, p) -> np.ndarray:
    """The penalised row as bf16 bits: fp32 arithmetic on the uint16 bit patterns, RNE back to bf16."""
    bits = np.asarray(bits, dtype=np.uint16)
    out = bits.copy()
    V = len(bits)
    idx = np.unique(np.asarray(list(seen_ids), dtype=np.int64))
    idx = idx[(idx >= 0) & (idx < V)]
    if not penalty_on(p) or not len(idx):
        return out
    l = (bits[idx].astype(np.uint32) << 16).view(np.float32)
    fin = np.isfinite(l)
    p32 = np.float32(p)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        r = np.where(l < 0, l * p32, l / p32).astype(np.float32)
    out[idx] = np.where(fin, S.to_bits(r), bits[idx])
    return out


def greedy_pick(bits) -> int:
    k = S.key(bits)
    return int(np.argmax(k)) if (k >= 0).any() else 0      # (argmax: the first index of the largest key)


def seen_words(V: int) -> int:
    return -(-(-(-V // 32)) // 4) * 4


def host_bitmap(seen_rows, V: int, ld_words: int = 0) -> np.ndarray:
    """uint32 [rows, ld_words]: bit t & 31 of word t >> 5 of row b set for every id t of seen_rows[b] inside [0, V)."""
    ldw = ld_words or seen_words(V)
    bm = np.zeros((len(seen_rows), ldw), np.uint32)
    for b, ids in enumerate(seen_rows):
        ids = np.asarray(list(ids), dtype=np.int64)
        ids = np.unique(ids[(ids >= 0) & (ids < V)])
        np.bitwise_or.at(bm[b], ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return bm


def seen_set(kind: str, bits: np.ndarray) -> np.ndarray:
    V = len(bits)
    if kind == "empty":
        return np.zeros(0, np.int64)
    if kind == "one":
        return np.array([(2 * V) // 3], np.int64)
    if kind == "argmax":
        return np.array([greedy_pick(bits)], np.int64)
    if kind == "every32":
        return np.unique(np.concatenate([np.arange(0, V, 32), [i for i in (31, 32, 33, V - 1) if i < V]]).astype(np.int64))
    assert kind == "all"
    return np.arange(V, dtype=np.int64)


PAIRS = [(k, p) for k in SEEN_KINDS for p in PENALTIES]      # 20
PER_ROW = 3
_cache: dict = {}


def _case(name, bits, kind, p, T, top_p, top_k, rng, planted=False):
    seen = seen_set(kind, bits)
    pb = penalise(bits, seen, p)
    o = S.oracle(pb, T, top_p, top_k)
    return dict(name=f"{name}|{kind}|p{p}", V=len(bits), bits=bits, seen=seen, p=p, T=T, top_p=top_p, top_k=top_k, pbits=pb, oracle=o,
                draws=None if o.margin < S.EXACT_MARGIN * S.EPS else S._draws(o, len(bits), rng, planted))


def cases() -> List[dict]:
    """dicts(name, V, bits, seen, p, T, top_p, top_k, pbits = the penalised row, oracle = the sampler's oracle on it, draws)."""
    if "c" in _cache:
        return _cache["c"]
    rows, _ = S.rows_and_batches()
    out, skipped = [], 0
    for V in CASE_V:
        rng = np.random.default_rng(9000 + V)
        at = 0
        for r in (r for r in rows if r["V"] == V):
            took = 0
            for _ in range(len(PAIRS)):      # (at most one turn of the cycle per row)
                kind, p = PAIRS[at % len(PAIRS)]
                at += 1
                c = _case(r["name"], r["bits"], kind, p, r["T"], r["top_p"], r["top_k"], rng, "planted" in r["name"])
                if c["draws"] is None:       # the penalised row's top-p cut-off sits within 16 EPS of top_p Z1: the next pair
                    skipped += 1
                    continue
                out.append(c)
                took += 1
                if took == PER_ROW:
                    break
    rng = np.random.default_rng(9000 + BIG_V)
    x = (rng.standard_normal(BIG_V) * 3).astype(np.float32)
    for kind, p, top_k in (("every32", 1.3, 50), ("all", 2.0, 0)):
        c = _case(f"V{BIG_V}-normal", S.to_bits(x), kind, p, 1.0, 1.0, top_k, rng)
        assert c["draws"] is not None
        out.append(c)
    _cache["c"] = out
    _cache["skipped"] = skipped
    return out


def _gcase(name, x, seen, p):
    bits = S.to_bits(np.asarray(x, np.float32))
    seen = np.asarray(list(seen), np.int64)
    return dict(name=name, V=len(bits), bits=bits, seen=seen, p=p, want=greedy_pick(penalise(bits, seen, p)))


def greedy_cases() -> List[dict]:
    """dicts(name, V, bits, seen, p, want = greedy_pick(penalise(bits, seen, p)))."""
    if "g" in _cache:
        return _cache["g"]
    out = []
    seen_names = set()
    for c in cases():
        base = c["name"].split("|")[0].rsplit("-T", 1)[0]      # (one greedy case per row shape: the sampling parameters do not matter)
        if base in seen_names:
            continue
        seen_names.add(base)
        out.append(dict(name=c["name"], V=c["V"], bits=c["bits"], seen=c["seen"], p=c["p"], want=greedy_pick(c["pbits"])))
    for V in (63, 4099, 32773):
        rng = np.random.default_rng(9500 + V)
        x = (rng.standard_normal(V) * 2).astype(np.float32)
        ties = sorted({7, V // 2, V - 1})
        x[ties] = 20.0
        out.append(_gcase(f"V{V}-ties", x, [], 0.0))                                   # the first of the tied maxima
        out.append(_gcase(f"V{V}-ties-first-seen", x, [ties[0]], 1.3))                 # ... removed by the penalty: the second
        out.append(_gcase(f"V{V}-ties-all-seen", x, ties, 2.0))                        # all penalised alike: the first again
        out.append(_gcase(f"V{V}-ties-penalty-off", x, ties, 1.0))
        y = x.copy()
        y[ties] = [20.0, 18.5, 18.0][:len(ties)]
        out.append(_gcase(f"V{V}-moves-argmax", y, [ties[0]], 1.3))                    # 20 / 1.3 < 18.5: the runner-up wins
        out.append(_gcase(f"V{V}-boost", y, [ties[-1]], 0.5))                          # p < 1 raises a seen token: 18 / 0.5 = 36
        z = -np.abs(x) - 1
        z[V // 3], z[V // 4] = -0.5, -0.75
        out.append(_gcase(f"V{V}-negative", z, [V // 3], 2.0))                         # -0.5 * 2 = -1 < -0.75
        w = x.copy()
        w[:5] = -np.inf
        w[V - 4:] = np.nan
        w[ties[1]] = np.inf
        out.append(_gcase(f"V{V}-nonfinite", w, np.arange(0, V, 3), 1.3))
        out.append(_gcase(f"V{V}-no-finite-entry", np.full(V, np.nan, np.float32), [0, 1], 1.3))
        h = x.copy()
        h[11] = 3.0e38
        out.append(_gcase(f"V{V}-overflow", h, [11], 0.5))                             # 3e38 / 0.5 = inf: the entry drops out
    _cache["g"] = out
    return out
