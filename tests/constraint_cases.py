"""Definition, oracle and cases of the ruled decode head: per-row token bans, allow-lists and a minimum length in sample_rows_kernel's RULE
instantiations (vlm_fo1_amd/csrc/sample.hip, behind fo1_sample_rows_ruled_bf16 and fo1_decode_head_ruled_accept).
Shared by tests/test_constraint_cases.py (CPU), tests/test_constraint_head_gpu.py and tests/test_constraint_decode_gpu.py (MI355X).

Definition.  A row's rule { always_row, early_row, early_until, first_row } names rows of a mask table (a set bit = token banned; a row index
outside the table = none).  With c the tokens generated so far, the banned set of a pick is masks[always_row], plus masks[early_row] while
c < early_until, plus masks[first_row] while c == 0 (banned_at()).  A banned token counts as a non-finite entry (mask(): NaN bits): no key,
weight 0, never kept.  The penalty (penalty_cases.penalise), the sampler's definition (sampling_cases.oracle) and the greedy pick
(penalty_cases.greedy_pick) then apply to mask(penalise(bits)); ban and penalty commute, a banned token has no key either way.  A row with
nothing left gives id 0.  This is HF's SuppressTokens / NoBadWords (single-token words) / MinNewTokensLength / SuppressTokensAtBegin
processors in front of the warpers (tests/test_constraint_cases.py compares).

Tolerance.  The device forms the same fixed-order fp32 partial sums as without a rule, with some weights replaced by 0: the accept rule and
EPS = 2^-17 of tests/sampling_cases.py hold unchanged.  As in penalty_cases, a (row, ban kind) pair whose masked oracle keeps less than
EXACT_MARGIN * EPS between the mass above a key and top_p Z1 is left out — decided on the oracle alone; at most 5 % of the pairs may be left
out (left_out()).

Cases (cases()).  Every row of sampling_cases.rows_and_batches() at V in {63, 4099, 32773} crossed with the six ban kinds of BAN_KINDS: empty;
the row's argmax; every 8th id plus 7, 8, 9, 31, 32, 33 and V - 1 (byte and word boundaries); all but 16 ids (an allow-list); the 50 largest;
the last two 8-token groups (the unaligned tail at V = 4099 and 32773).  A few of them again with a repetition penalty on top, and one
N(0, 3) row at V = 151936.  Greedy rows (greedy_cases()): ties at the maximum with the first tied id banned, a banned +inf / NaN entry, all
but one id banned, everything banned (id 0), ban + penalty moving the argmax.  Phases (phase_cases()): one row at c = 0, early_until - 1 and
early_until, with each of the three mask rows alone and all together."""
from __future__ import annotations

from typing import List

import numpy as np

import penalty_cases as P
import sampling_cases as S

BAN_KINDS = ("empty", "argmax", "every8", "allow16", "top50", "tail")
CASE_V = (63, 4099, 32773)
BIG_V = 151936
NAN_BITS = 0x7fc0
MAX_LEFT_OUT = 0.05


def mask(bits, banned) -> np.ndarray:
    """The row with the banned ids (those inside [0, V)) replaced by NaN bits."""
    out = np.asarray(bits, dtype=np.uint16).copy()
    idx = np.asarray(list(banned), dtype=np.int64)
    idx = idx[(idx >= 0) & (idx < len(out))]
    out[idx] = NAN_BITS
    return out


def ruled(bits, banned, seen=(), p=0.0) -> np.ndarray:
    """mask(penalise(bits)): what every pass of the ruled head keys."""
    return mask(P.penalise(bits, seen, p), banned)


def banned_at(c: int, always=(), early=(), until: int = 0, first=()) -> np.ndarray:
    """The banned ids of the pick after c generated tokens."""
    parts = [np.asarray(list(always), np.int64)]
    if c < until:
        parts.append(np.asarray(list(early), np.int64))
    if c == 0:
        parts.append(np.asarray(list(first), np.int64))
    return np.unique(np.concatenate(parts))


def ban_set(kind: str, bits: np.ndarray) -> np.ndarray:
    V = len(bits)
    if kind == "empty":
        return np.zeros(0, np.int64)
    if kind == "argmax":
        return np.array([P.greedy_pick(bits)], np.int64)
    if kind == "every8":
        return np.unique(np.concatenate([np.arange(0, V, 8), [i for i in (7, 8, 9, 31, 32, 33, V - 1) if i < V]]).astype(np.int64))
    if kind == "allow16":      # everything but 16 ids spread over the row, the last one included
        keep = np.unique(np.linspace(0, V - 1, 16).astype(np.int64))
        return np.setdiff1d(np.arange(V, dtype=np.int64), keep)
    if kind == "top50":        # the 50 largest entries (ties: the first in vocabulary order)
        k = S.key(bits)
        return np.sort(np.argsort(-k.astype(np.int64), kind="stable")[:min(50, V - 1)]).astype(np.int64)
    assert kind == "tail"      # the last two 8-token groups: at V = 4099 the ids 4088 .. 4098, the last group 3 tokens long
    return np.arange(((V - 1) // 8 - 1) * 8, V, dtype=np.int64)


_cache: dict = {}


def _case(name, bits, kind, T, top_p, top_k, rng, planted=False, seen=(), p=0.0):
    banned = ban_set(kind, bits)
    seen = np.asarray(list(seen), np.int64)
    rb = ruled(bits, banned, seen, p)
    o = S.oracle(rb, T, top_p, top_k)
    return dict(name=f"{name}|{kind}" + (f"|p{p}" if P.penalty_on(p) else ""), V=len(bits), bits=bits, kind=kind, banned=banned, seen=seen, p=p, T=T,
                top_p=top_p, top_k=top_k, rbits=rb, oracle=o, draws=None if o.margin < S.EXACT_MARGIN * S.EPS else S._draws(o, len(bits), rng, planted))


def cases() -> List[dict]:
    """dicts(name, V, bits, kind, banned, seen, p, T, top_p, top_k, rbits = mask(penalise(bits)), oracle = the sampler's oracle on it, draws)."""
    if "c" in _cache:
        return _cache["c"]
    rows, _ = S.rows_and_batches()
    out, pairs, left = [], 0, []
    for V in CASE_V:
        rng = np.random.default_rng(7000 + V)
        mine = [r for r in rows if r["V"] == V]
        for r in mine:
            for kind in BAN_KINDS:
                c = _case(r["name"], r["bits"], kind, r["T"], r["top_p"], r["top_k"], rng, "planted" in r["name"])
                pairs += 1
                if c["draws"] is None:      # the masked row's top-p cut-off sits within 16 EPS of top_p Z1: left out, and counted
                    left.append(c["name"])
                    continue
                out.append(c)
        # ban and penalty together: every 7th row with the byte-boundary bans and the penalty cases' word-boundary seen set
        for j, r in enumerate(mine[::7]):
            c = _case(r["name"], r["bits"], ("every8", "top50", "argmax")[j % 3], r["T"], r["top_p"], r["top_k"], rng, seen=P.seen_set("every32", r["bits"]),
                      p=(1.3, 0.5)[j % 2])
            if c["draws"] is not None:
                out.append(c)
    rng = np.random.default_rng(7000 + BIG_V)
    x = (rng.standard_normal(BIG_V) * 3).astype(np.float32)
    for kind, p, top_k in (("every8", 0.0, 50), ("allow16", 0.0, 0), ("top50", 1.3, 0)):
        c = _case(f"V{BIG_V}-normal", S.to_bits(x), kind, 1.0, 1.0, top_k, rng, seen=P.seen_set("every32", S.to_bits(x)) if p else (), p=p)
        assert c["draws"] is not None
        out.append(c)
    _cache["c"] = out
    _cache["left"] = (left, pairs)
    return out


def left_out():
    """-> (names of the (row, kind) pairs left out for their top-p margin, number of pairs)."""
    cases()
    return _cache["left"]


def _gcase(name, x, banned, seen=(), p=0.0):
    bits = S.to_bits(np.asarray(x, np.float32))
    banned, seen = np.asarray(list(banned), np.int64), np.asarray(list(seen), np.int64)
    return dict(name=name, V=len(bits), bits=bits, banned=banned, seen=seen, p=p, want=P.greedy_pick(ruled(bits, banned, seen, p)))


def greedy_cases() -> List[dict]:
    """dicts(name, V, bits, banned, seen, p, want = greedy_pick(mask(penalise(bits))))."""
    if "g" in _cache:
        return _cache["g"]
    out = []
    for V in CASE_V:
        rng = np.random.default_rng(7500 + V)
        x = (rng.standard_normal(V) * 2).astype(np.float32)
        ties = sorted({7, V // 2, V - 1})
        x[ties] = 20.0
        out.append(_gcase(f"V{V}-ties", x, []))
        out.append(_gcase(f"V{V}-ties-first-banned", x, [ties[0]]))                       # the second tied id
        out.append(_gcase(f"V{V}-ties-all-but-last-banned", x, ties[:-1]))                # V - 1: the unaligned tail's last token
        out.append(_gcase(f"V{V}-ties-all-banned", x, ties))                              # the runner-up
        w = x.copy()
        w[ties[0]], w[ties[1]] = np.inf, np.nan
        out.append(_gcase(f"V{V}-banned-inf-nan", w, [ties[0], ties[1]]))                 # banned non-finite entries stay without a key
        out.append(_gcase(f"V{V}-all-but-one", x, np.setdiff1d(np.arange(V), [V // 3])))
        out.append(_gcase(f"V{V}-all-but-last", x, np.arange(V - 1)))
        out.append(_gcase(f"V{V}-everything-banned", x, np.arange(V)))                    # id 0
        y = x.copy()
        y[ties] = [20.0, 18.5, 18.0][:len(ties)]
        out.append(_gcase(f"V{V}-penalty-then-ban", y, [ties[1]], [ties[0]], 1.3))        # 20 / 1.3 = 15.4 < 18 once 18.5 is banned: the third
        out.append(_gcase(f"V{V}-banned-and-seen", y, [ties[0]], [ties[0]], 0.5))         # banned wins over the boost: no key either way
        out.append(_gcase(f"V{V}-every8", x, ban_set("every8", S.to_bits(x))))
    _cache["g"] = out
    return out


def phase_cases() -> List[dict]:
    """One row per V and three disjoint mask sets A (always), E (early, until = 5), F (first): dicts(name, V, bits, always, early, until, first,
    c, want = the greedy pick at counter c).  The row's largest entries are planted so that every live mask row changes the pick."""
    if "p" in _cache:
        return _cache["p"]
    out = []
    for V in CASE_V:
        rng = np.random.default_rng(7700 + V)
        x = (rng.standard_normal(V) * 2).astype(np.float32)
        f, e, a, rest = 9, V - 1, V // 2, 33
        sets = dict(A=[a, 8], E=[e, 31], F=[f, 32])
        until = 5
        for combo in ("A", "E", "F", "AEF"):
            y = x.copy()
            y[[f, e, a, rest]] = [24.0, 23.0, 22.0, 21.0]
            y[dict(A=a, E=e, F=f, AEF=f)[combo]] = 25.0      # the combination's own first set holds the row's maximum
            bits = S.to_bits(y)
            rule = dict(always=sets["A"] if "A" in combo else [], early=sets["E"] if "E" in combo else [], until=until if "E" in combo else 0,
                        first=sets["F"] if "F" in combo else [])
            for c in (0, until - 1, until):
                out.append(dict(name=f"V{V}-{combo}-c{c}", V=V, bits=bits, c=c, want=P.greedy_pick(mask(bits, banned_at(c, **rule))), **rule))
    _cache["p"] = out
    return out


def host_masks(sets, V: int, ld_words: int = 0, pad_ones: bool = False) -> np.ndarray:
    """uint32 [rows, ld_words] mask table (penalty_cases.host_bitmap's layout); pad_ones: every bit for t >= V set too."""
    bm = P.host_bitmap(sets, V, ld_words)
    if pad_ones:
        t = np.arange(V, bm.shape[1] * 32, dtype=np.int64)
        for b in range(bm.shape[0]):
            np.bitwise_or.at(bm[b], t >> 5, (np.uint32(1) << (t & 31).astype(np.uint32)))
    return bm
