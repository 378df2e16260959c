"""Token guides: the banned set of a pick as a function of a per-sequence automaton state (include/fo1.h
fo1_token_guide_t).  Host side: the automaton, its validation, its banned sets as bitmaps in the seen bitmap's layout, and two builders — the
FO1 answer language (region_answer) and multi-token banned sequences (ban_sequences).

A guide is a deterministic automaton over token CLASSES: cls[t] in [0, C) is the class of token t, next[s][c] the state after a token of class
c in state s, a negative entry = class c is not allowed in s.  The banned set of state s is { t : next[s][cls[t]] < 0 }; after the head accepts
token t in state s the state is next[s][cls[t]] (a negative entry keeps s: the "nothing left gives id 0" fall-back, which validation rules
out for every state the guide can reach).  The decode head keeps the state on the device and advances it itself (csrc/sample.hip)."""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence

import numpy as np

OUT, LABEL0, LABEL, OPEN, OBJ0, OBJ = range(6)      # the states of region_answer
INF = int(np.iinfo(np.int32).max)                   # distances(): no path to an accepting state


def _words(V: int) -> int:
    """Words per row of a seen bitmap (ops.seen_words: ceil(V / 32) rounded up to a multiple of 4)."""
    return -(-(-(-int(V) // 32)) // 4) * 4


def pack_bits(m: np.ndarray) -> bytes:
    """bool [V] -> the bitmap's bytes in the seen bitmap's layout (bit t & 31 of word t >> 5 = token t), the layout llm.token_rule packs."""
    out = np.zeros(_words(len(m)) * 4, dtype=np.uint8)
    pk = np.packbits(np.asarray(m, dtype=bool), bitorder="little")
    out[:pk.size] = pk
    return out.tobytes()


def unpack_bits(bitmap: Optional[bytes], V: int) -> np.ndarray:
    """pack_bits' inverse: bool [V] (None = nothing set)."""
    if bitmap is None:
        return np.zeros(V, dtype=bool)
    return np.unpackbits(np.frombuffer(bitmap, dtype=np.uint8), bitorder="little")[:V].astype(bool)


class TokenGuide:
    """TokenGuide(cls, next, start, V): cls uint16 [V], next int16 / int32 [S, C], start in [0, S).  Immutable, and hashable by content: equal
    guides compare equal, so they share their rows of the device tables.
    walk (optional, int [S, C], every entry a state): the transitions the PROMPT takes, which is not subject to the guide — run() follows it
    for a class that next bans; a guide with a walk table starts a sequence in run(prompt ids) instead of `start` (ban_sequences), and any of
    its states may be the first one.
    ValueError: shapes that do not match, a class outside [0, C), an entry of next >= S, a start state outside [0, S), or a state the guide can
    reach whose banned set is all V tokens.
    accept (optional, an iterable of states): the ACCEPTING states — an answer is closed when its guide is in one of them.  A guide with
    accepting states closes before the sequence's token budget runs out (closing_bitmaps; DESIGN.md section 14, "budget-aware guides");
    None is a guide without the rule, with the key, the hash and the tables it has without the keyword.  ValueError: a state outside
    [0, S), or no state at all."""
    __slots__ = ("V", "S", "C", "start", "cls", "next", "walk", "accept", "_key", "_hash", "_banned")

    def __init__(self, cls, next, start: int, V: int, walk=None, accept=None):
        V = int(V)
        c = np.asarray(cls)
        n = np.asarray(next)
        if c.dtype != np.uint16:
            raise ValueError(f"TokenGuide: cls is uint16 (got {c.dtype})")
        if n.dtype not in (np.dtype(np.int16), np.dtype(np.int32)):
            raise ValueError(f"TokenGuide: next is int16 or int32 (got {n.dtype})")
        if V < 1 or c.shape != (V,):
            raise ValueError(f"TokenGuide: cls has shape {c.shape}, V = {V}")
        if n.ndim != 2 or n.shape[0] < 1 or n.shape[1] < 1:
            raise ValueError(f"TokenGuide: next has shape {n.shape} ([S, C])")
        S, C = n.shape
        if int(c.max()) >= C:
            raise ValueError(f"TokenGuide: class {int(c.max())} outside [0, {C})")
        if int(n.max()) >= S:
            raise ValueError(f"TokenGuide: next names state {int(n.max())} outside [0, {S})")
        if isinstance(start, (bool, float)) or not hasattr(start, "__index__") or not 0 <= int(start) < S:
            raise ValueError(f"TokenGuide: start state {start!r} outside [0, {S})")
        self.V, self.S, self.C, self.start = V, S, C, int(start)
        self.cls = np.ascontiguousarray(c).copy()
        self.next = np.ascontiguousarray(n, dtype=np.int32).copy()
        self.cls.setflags(write=False)
        self.next.setflags(write=False)
        self.walk = None
        if walk is not None:
            w = np.ascontiguousarray(np.asarray(walk), dtype=np.int32).copy()
            if w.shape != (S, C) or int(w.min()) < 0 or int(w.max()) >= S:
                raise ValueError(f"TokenGuide: walk has shape {w.shape} or an entry outside [0, {S})")
            w.setflags(write=False)
            self.walk = w
        self.accept = None
        if accept is not None:
            acc = []
            for a in accept:
                if isinstance(a, (bool, float)) or not hasattr(a, "__index__") or not 0 <= int(a) < S:
                    raise ValueError(f"TokenGuide: accepting state {a!r} outside [0, {S})")
                acc.append(int(a))
            if not acc:
                raise ValueError("TokenGuide: accept names no state (None = a guide without accepting states)")
            self.accept = tuple(sorted(set(acc)))
        self._key = (V, S, C, self.start, self.cls.tobytes(), self.next.tobytes(), None if self.walk is None else self.walk.tobytes())
        if self.accept is not None:
            self._key += (self.accept,)
        self._hash = hash(self._key)
        self._banned: dict = {}
        for s in self.reachable():
            if (self.next[s][self.cls] < 0).all():
                raise ValueError(f"TokenGuide: state {s} can be reached and bans all {V} tokens")

    def __eq__(self, other):
        return isinstance(other, TokenGuide) and self._key == other._key

    def __hash__(self):
        return self._hash

    def __repr__(self):
        return f"TokenGuide(V={self.V}, S={self.S}, C={self.C}, start={self.start}{'' if self.accept is None else f', accept={list(self.accept)}'})"

    @property
    def from_prompt(self) -> bool:
        """The sequence starts in run(prompt ids), not in `start`."""
        return self.walk is not None

    def classes_present(self) -> np.ndarray:
        """bool [C]: some token has the class."""
        p = np.zeros(self.C, dtype=bool)
        p[self.cls] = True
        return p

    def reachable(self, starts: Optional[Iterable[int]] = None) -> List[int]:
        """The states the guide can be in: from `start` (every state when a prompt may leave it anywhere) over the allowed classes some token has."""
        if starts is None:
            starts = range(self.S) if self.from_prompt else [self.start]
        present = self.classes_present()
        seen, todo = set(), [int(s) for s in starts]
        while todo:
            s = todo.pop()
            if s in seen:
                continue
            seen.add(s)
            todo += [int(n) for n in self.next[s][present] if n >= 0 and int(n) not in seen]
        return sorted(seen)

    def banned_mask(self, s: int) -> np.ndarray:
        """bool [V]: the banned set of state s."""
        return self.next[int(s)][self.cls] < 0

    def banned(self, s: int) -> bytes:
        """The banned set of state s as a bitmap in the seen bitmap's layout (ops.seen_words(V) words)."""
        s = int(s)
        out = self._banned.get(s)
        if out is None:
            out = self._banned[s] = pack_bits(self.banned_mask(s))
        return out

    def advance(self, s: int, t: int) -> int:
        """The state after token t is accepted in state s (a banned token keeps the state, as the device does)."""
        n = int(self.next[int(s), int(self.cls[int(t)])])
        return n if n >= 0 else int(s)

    def run(self, ids: Sequence[int], s: Optional[int] = None) -> int:
        """The state after a list of ids (the prompt's: a class the guide bans follows the walk table when there is one, and an id outside
        [0, V) — an image placeholder — is part of no word: the walk starts over; without a walk table such an id is a ValueError)."""
        s = self.start if s is None else int(s)
        for t in ids:
            if not 0 <= int(t) < self.V:
                if self.walk is None:
                    raise ValueError(f"TokenGuide.run: token id {int(t)} outside [0, {self.V})")
                s = self.start
                continue
            c = int(self.cls[int(t)])
            n = int(self.next[s, c])
            if n < 0 and self.walk is not None:
                n = int(self.walk[s, c])
            s = n if n >= 0 else s
        return s

    def state_bitmaps(self, always: Optional[bytes] = None) -> List[Optional[bytes]]:
        """Every state's banned set with the sequence's own always-bans folded in -> one bitmap per state, None for an empty one."""
        out = self._banned.get(("fold", always))      # (threads share guides: an entry is read once and never read back after a store)
        if out is None:
            extra = unpack_bits(always, self.V)
            out = []
            for s in range(self.S):
                m = self.banned_mask(s) | extra
                out.append(pack_bits(m) if m.any() else None)
            if len(self._banned) > 4 * self.S + 64:      # (a cache, not a record: every entry can be recomputed)
                self._banned.clear()
            self._banned[("fold", always)] = out
        return list(out)

    def distances(self, always: Optional[bytes] = None) -> np.ndarray:
        """int64 [S]: the smallest number of tokens that lead from each state to an accepting one, over the classes that have a token the
        sequence's always-bans leave; 0 for an accepting state, INF for a state without a path (every state of a guide without accepting
        states)."""
        out = self._banned.get(("dist", always))
        if out is None:
            out = np.full(self.S, INF, dtype=np.int64)
            if self.accept is not None:
                ok = np.zeros(self.C, dtype=bool)
                ok[self.cls[~unpack_bits(always, self.V)]] = True
                out[list(self.accept)] = 0
                d, grew = 0, True
                while grew:      # breadth first from the accepting states, backwards: level d + 1 = a state with an edge into level d
                    near = out <= d
                    step = ((self.next >= 0) & ok[None, :] & near[np.maximum(self.next, 0)]).any(axis=1) & ~near
                    out[step] = d + 1
                    grew = bool(step.any())
                    d += 1
            out.setflags(write=False)
            self._banned[("dist", always)] = out
        return out

    def depth(self, always: Optional[bytes] = None) -> int:
        """D: the largest finite distance among the states the guide can reach — from D tokens left on, the closing rule bans nothing a
        sequence that check_pickable passed could take (0 for a guide without accepting states)."""
        d = self.distances(always)[self.reachable()]
        d = d[d < INF]
        return int(d.max()) if d.size else 0

    def closing_mask(self, s: int, r: int, always: Optional[bytes] = None) -> np.ndarray:
        """bool [V]: the banned set of state s at a pick that r tokens may still follow — { t : next[s][cls[t]] < 0 or
        dist[next[s][cls[t]]] > r }, with the sequence's always-bans folded in."""
        n = self.next[int(s)][self.cls]
        return (n < 0) | (self.distances(always)[np.maximum(n, 0)] > int(r)) | unpack_bits(always, self.V)

    def closing_bitmaps(self, always: Optional[bytes] = None):
        """-> (D, rows): rows[s][r], 0 <= r < D, is closing_mask(s, r, always) as a bitmap in the seen bitmap's layout (None = nothing
        banned); for r >= D the head reads the state's plain row (state_bitmaps), which holds the same set for every state that leads to no
        state without a path — check_pickable refuses a sequence that could enter one.  rows is None for a guide without accepting states
        and when D == 0."""
        if self.accept is None:
            return 0, None
        out = self._banned.get(("close", always))
        if out is None:
            D = self.depth(always)
            rows = None
            if D > 0:
                rows = []
                for s in range(self.S):
                    ms = [self.closing_mask(s, r, always) for r in range(D)]
                    rows.append(tuple(pack_bits(m) if m.any() else None for m in ms))
                rows = tuple(rows)
            out = self._banned[("close", always)] = (D, rows)
        return out

    def check_pickable(self, s0: int, always: Optional[bytes] = None, early: Optional[bytes] = None, until: int = 0,
                       first: Optional[bytes] = None, c0: int = 0, budget: Optional[int] = None) -> None:
        """ValueError when the sequence can reach a pick with nothing left: it starts in state s0 with c0 tokens generated; the pick after c
        tokens bans the state's set, `always`, `early` while c < until and `first` while c == 0 (llm.TokenRule).
        budget (N, for a guide with accepting states; None = no closing rule): the pick after c tokens, which r = N - c - 1 tokens may
        follow, also bans every token whose next state is more than r tokens from an accepting one (closing_mask), and a start further than
        N - c0 tokens from one is a ValueError, and so is a token the sequence may take into a state without a path to one.  The walk runs over (state, min(c, cap), min(r, D)): c and r are exact while c < cap or
        r < D, and the picks between (c >= cap and r >= D, all alike) are one node per state, left for r = D - 1 from every state they
        reach."""
        V = self.V
        a, e, f = (unpack_bits(m, V) for m in (always, early, first))
        until = int(until) if early is not None else 0
        s0, c0 = int(s0), int(c0)
        N = D = None
        if budget is not None and self.accept is not None:
            N, D = int(budget), self.depth(always)
            dist = self.distances(always)
            if dist[s0] > max(N - c0, 0):
                far = "no path" if dist[s0] >= INF else f"{int(dist[s0])} tokens"
                raise ValueError(f"token guide: state {s0} after {c0} generated tokens is {far} from an accepting state, the budget of {N} "
                                 f"tokens leaves {max(N - c0, 0)}")
            if N - c0 <= 0:
                return

        def avail(ban):      # bool [C]: the class has a token outside `ban`
            p = np.zeros(self.C, dtype=bool)
            p[self.cls[~ban]] = True
            return p

        cap = max(until, 1)      # counts from `cap` on are alike
        MID = -1                 # the node of every count c >= cap with (under a budget) r >= D

        def node(c):
            return c if c < cap or (N is not None and N - 1 - c < D) else MID

        phases = {}
        seen, todo = set(), [(s0, node(c0))]
        while todo:
            s, c = todo.pop()
            if (s, c) in seen:
                continue
            seen.add((s, c))
            ph = (c == 0, c != MID and c < until)
            if ph not in phases:
                phases[ph] = avail(a | (f if ph[0] else False) | (e if ph[1] else False))
            ok = (self.next[s] >= 0) & phases[ph]
            r = None if N is None or c == MID else N - 1 - c
            if r is not None and r < D:
                ok &= dist[np.maximum(self.next[s], 0)] <= r
            elif N is not None and (dist[self.next[s][ok]] >= INF).any():      # (from D tokens left on the head reads the state's plain row)
                raise ValueError(f"token guide: in state {s} the guide and the sequence's token rule allow a token into state "
                                 f"{int(self.next[s][ok][dist[self.next[s][ok]] >= INF][0])}, from which no path leads to an accepting state")
            if not ok.any():
                at = f"{cap}+" if c == MID else f"{c}"
                left = "" if N is None else f" with {f'{D}+' if r is None else r} tokens left of a budget of {N}"
                raise ValueError(f"token guide: in state {s} after {at} generated tokens{left} the guide{'' if N is None else ', its closing rule'} "
                                 f"and the sequence's token rule together ban all {V} tokens")
            if c == MID:
                nxt = [MID] if N is None or N - D - cap >= 2 else []
                if N is not None and D >= 1:
                    nxt.append(N - D)
            else:
                nxt = [node(c + 1)] if N is None or c + 1 <= N - 1 else []
            todo += [(int(n), k) for n in self.next[s][ok] for k in nxt]


def _ids(ids, V: int, what: str) -> List[int]:
    out = []
    for t in ids:
        if isinstance(t, (bool, float)) or not hasattr(t, "__index__") or not 0 <= int(t) < V:
            raise ValueError(f"{what}: token id {t!r} outside [0, {V})")
        out.append(int(t))
    return out


def region_answer(V: int, ground: int, ground_end: int, objects: int, objects_end: int, region_ids: Sequence[int], n_regions: int,
                  stop_ids: Sequence[int], close: bool = False) -> TokenGuide:
    """The FO1 answer language `<ground>label</ground><objects><region3><region7></objects>` with region indices below n_regions;
    region_ids[k] is the id of `<regionk>`.  States (OUT is the start):
      OUT     anything but </ground>, <objects>, </objects> and region_ids[n_regions:]; stop ids allowed; <ground> -> LABEL0
      LABEL0  one plain token (no structural token, no region token, no stop id) -> LABEL
      LABEL   plain tokens; </ground> -> OPEN
      OPEN    only <objects> -> OBJ0
      OBJ0    only region_ids[:n_regions] -> OBJ
      OBJ     region_ids[:n_regions]; </objects> -> OUT
    Every region id has a class of its own, so guides that differ in n_regions only share their class map.
    close=True: OUT is the accepting state — the answer closes its structure before the sequence's token budget runs out."""
    V = int(V)
    regions = _ids(region_ids, V, "region_answer: region_ids")
    struct = _ids([ground, ground_end, objects, objects_end], V, "region_answer: a structural id")
    stops = sorted(set(_ids(stop_ids, V, "region_answer: stop_ids")))
    n = int(n_regions)
    if n <= 0 or n > len(regions):
        raise ValueError(f"region_answer: n_regions = {n} (1 .. {len(regions)}, the region ids given)")
    named = struct + regions + stops
    if len(set(named)) != len(named):
        raise ValueError("region_answer: the structural, region and stop ids must be distinct")
    R = len(regions)
    PLAIN, G, GE, O, OE, REG0 = 0, 1, 2, 3, 4, 5
    STOP = REG0 + R
    C = STOP + 1
    if C > 65535:
        raise ValueError(f"region_answer: {R} region ids do not fit the 16-bit class map")
    cls = np.zeros(V, dtype=np.uint16)
    cls[struct] = [G, GE, O, OE]
    cls[regions] = np.arange(REG0, REG0 + R, dtype=np.uint16)
    cls[stops] = STOP
    nx = np.full((6, C), -1, dtype=np.int32)
    ok = slice(REG0, REG0 + n)
    nx[OUT, PLAIN] = nx[OUT, ok] = nx[OUT, STOP] = OUT
    nx[OUT, G] = LABEL0
    nx[LABEL0, PLAIN] = LABEL
    nx[LABEL, PLAIN] = LABEL
    nx[LABEL, GE] = OPEN
    nx[OPEN, O] = OBJ0
    nx[OBJ0, ok] = OBJ
    nx[OBJ, ok] = OBJ
    nx[OBJ, OE] = OUT
    if len(named) >= V:
        raise ValueError("region_answer: the vocabulary has no plain token left for a label")
    return TokenGuide(cls, nx, OUT, V, accept=(OUT,) if close else None)


def ban_sequences(words: Sequence[Sequence[int]], V: int) -> TokenGuide:
    """The Aho-Corasick automaton of a list of token-id sequences: a token is banned in a state exactly when taking it would complete a word —
    HF's NoBadWordsLogitsProcessor for words of any length.  States are the nodes of the trie of the words' proper prefixes with the failure
    links resolved into `next`; every token that occurs in a word has a class of its own, all others share class 0.  HF matches a word's
    prefix against the prompt too: the guide carries a walk table and a sequence starts in run(prompt ids)."""
    V = int(V)
    ws = []
    for w in words:
        w = _ids(w, V, "ban_sequences: a word")
        if not w:
            raise ValueError("ban_sequences: an empty word")
        ws.append(tuple(w))
    if not ws:
        raise ValueError("ban_sequences: no words")
    toks = sorted({t for w in ws for t in w})
    if len(toks) + 1 > 65535:
        raise ValueError(f"ban_sequences: {len(toks)} distinct tokens do not fit the 16-bit class map")
    cls = np.zeros(V, dtype=np.uint16)
    cls[toks] = np.arange(1, len(toks) + 1, dtype=np.uint16)
    C = len(toks) + 1
    # the trie of the proper prefixes w[:-1]; last[node] = the classes that complete a word whose prefix is the node's string
    child: List[dict] = [{}]
    last: List[set] = [set()]
    for w in ws:
        node = 0
        for t in w[:-1]:
            c = int(cls[t])
            if c not in child[node]:
                child[node][c] = len(child)
                child.append({})
                last.append(set())
            node = child[node][c]
        last[node].add(int(cls[w[-1]]))
    S = len(child)
    walk = np.zeros((S, C), dtype=np.int32)      # goto with the failure links resolved, breadth first (class 0 leads to the root)
    fail = [0] * S
    order = list(child[0].values())
    for c, n in child[0].items():
        walk[0, c] = n
    i = 0
    while i < len(order):
        node = order[i]
        i += 1
        last[node] |= last[fail[node]]      # a word whose prefix is a suffix of this node's string completes here too
        walk[node] = walk[fail[node]]
        for c, n in child[node].items():
            fail[n] = int(walk[fail[node], c])
            walk[node, c] = n
            order.append(n)
    nx = walk.copy()
    for node in range(S):
        for c in last[node]:
            nx[node, c] = -1
    return TokenGuide(cls, nx, 0, V, walk=walk)
