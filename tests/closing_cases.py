"""Definition, brute force and cases of the budget-aware token guides: a guide with accepting states closes its structure before the
sequence's token budget runs out (vlm_fo1_amd/guide.py: TokenGuide(accept=), distances, closing_bitmaps, check_pickable(budget=);
sample_rows_kernel's CLOSE instantiations in vlm_fo1_amd/csrc/sample.hip, behind fo1_sample_rows_closing_bf16 and
fo1_decode_head_closing_accept).  Shared by tests/test_closing_cases.py (CPU), tests/test_closing_head_gpu.py and
tests/test_closing_decode_gpu.py (MI355X).  Builds on guide_cases and changes nothing of it.

Definition.  dist[s] = the fewest tokens from s to an accepting state, over the classes some token outside the sequence's always-bans has.
At a pick made after c tokens under a budget N, r = N - c - 1 tokens may still follow; state s then bans
{ t : next[s][cls[t]] < 0 or dist[next[s][cls[t]]] > r } (and the always-bans).  The device reads the set of (s, r) from a table for
r < D (the largest finite distance of a reachable state) and the state's plain row from D on.

Brute force (allowed_by_enumeration).  The token strings themselves: t is allowed in (s, r) iff t is not always-banned, next[s][cls[t]] is a
state, and some string of at most r further tokens, none always-banned, each allowed by `next`, ends in an accepting state — found by trying
every class at every position, shortest strings first.  It shares nothing with guide.distances, which works backwards from the accepting states.

Walks (walk).  A sequence under budget N picks N tokens (no stop id among the uniform choices' winners ends it early here: a walk runs to
its budget, the worst case for closing); `far` always takes an allowed token whose next state is farthest from accepting."""
from __future__ import annotations

from functools import lru_cache
from typing import List, Optional

import numpy as np

from vlm_fo1_amd import guide as TG

V = 63
IDS = dict(ground=50, ground_end=51, objects=52, objects_end=53, region=[40, 41, 42, 43, 44, 45, 46, 47], stops=[60, 61])
N_ALLOWED = 5
DIST = {TG.OUT: 0, TG.LABEL0: 5, TG.LABEL: 4, TG.OPEN: 3, TG.OBJ0: 2, TG.OBJ: 1}      # region_answer(close=True)


def region_guide(n: int = N_ALLOWED, close: bool = True, start: Optional[int] = None, V: int = V, ids: dict = IDS):
    g = TG.region_answer(V, ids["ground"], ids["ground_end"], ids["objects"], ids["objects_end"], ids["region"], n, ids["stops"], close=close)
    if start is None:
        return g
    return TG.TokenGuide(g.cls, g.next, start, V, accept=g.accept)


def grammar(n: int = N_ALLOWED):
    import guide_cases as G
    return G.Grammar(V, IDS["ground"], IDS["ground_end"], IDS["objects"], IDS["objects_end"], IDS["region"], n, IDS["stops"])


def random_guides(count: int = 16, seed: int = 77) -> List[tuple]:
    """(guide, always) pairs: S <= 6 states, C <= 5 classes over V = 63, a class without a token in most, states without a path to an
    accepting one in most, an always-ban (which can empty a class) in every other one."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        S, C = int(rng.integers(2, 7)), int(rng.integers(2, 6))
        cls = rng.integers(0, C, V).astype(np.uint16)
        if C > 2:
            cls[cls == C - 1] = 0      # class C - 1 has no token
        nx = rng.integers(-1, S, (S, C)).astype(np.int32)
        nx[rng.random((S, C)) < 0.3] = -1
        if S > 2:      # a sink: reachable, never accepting, leads only to itself
            nx[S - 1, :] = S - 1
        accept = sorted(set(rng.integers(0, max(S - 1, 1), int(rng.integers(1, 3))).tolist()))
        try:
            g = TG.TokenGuide(cls, nx, 0, V, accept=accept)
        except ValueError:      # a reachable state that bans everything: not a guide
            continue
        always = None
        if len(out) % 2:
            m = np.zeros(V, dtype=bool)
            m[rng.integers(0, V, 6)] = True
            m[cls == int(rng.integers(0, C))] = True      # a whole class gone
            always = TG.pack_bits(m)
        out.append((g, always))
    return out


def allowed_by_enumeration(g, s: int, r: int, always: Optional[bytes] = None) -> set:
    """{ t : some token string of length <= r from next[s][cls[t]] ends accepting }, t itself and every token of the string outside `always`."""
    a = TG.unpack_bits(always, g.V)
    usable = sorted({int(c) for c in g.cls[~a]})      # classes a token string can use
    acc = set(g.accept or ())

    @lru_cache(maxsize=None)
    def closes(n: int, left: int) -> bool:
        if n in acc:
            return True
        if left == 0:
            return False
        return any(g.next[n, c] >= 0 and closes(int(g.next[n, c]), left - 1) for c in usable)

    out = set()
    for t in range(g.V):
        n = int(g.next[s, g.cls[t]])
        if not a[t] and n >= 0 and closes(n, r):
            out.add(t)
    return out


def allowed(g, s: int, r: Optional[int], always: Optional[bytes] = None) -> np.ndarray:
    """The ids the definition leaves at a pick in state s with r tokens left (None: no closing rule), as the device selects the set: the
    closing bitmap for r < D, the plain one otherwise."""
    D, rows = g.closing_bitmaps(always)
    if r is not None and rows is not None and 0 <= r < D:
        bm = rows[s][r]
    else:
        bm = g.state_bitmaps(always)[s]
    return np.nonzero(~TG.unpack_bits(bm, g.V))[0]


def walk(g, budget: int, rng, mode: str, closing: bool = True):
    """One sequence of `budget` picks from the start state -> (ids, final state, picks at which the closing set differed from the plain
    one).  mode "uniform": uniform over the allowed set; "far": an allowed token whose next state is farthest from accepting."""
    s, ids, differed = g.start, [], 0
    dist = g.distances()
    for c in range(budget):
        r = budget - c - 1
        ok = allowed(g, s, r if closing else None)
        assert len(ok), (s, c, r)
        differed += closing and len(ok) != len(allowed(g, s, None))
        if mode == "far":
            d = np.array([dist[g.advance(s, int(t))] for t in ok])
            ok = ok[d == d.max()]
        t = int(ok[rng.integers(len(ok))])
        ids.append(t)
        s = g.advance(s, t)
    return ids, s, differed
