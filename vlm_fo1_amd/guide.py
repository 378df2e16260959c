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
    reach whose banned set is all V tokens."""
    __slots__ = ("V", "S", "C", "start", "cls", "next", "walk", "_key", "_hash", "_banned")

    def __init__(self, cls, next, start: int, V: int, walk=None):
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
        self._key = (V, S, C, self.start, self.cls.tobytes(), self.next.tobytes(), None if self.walk is None else self.walk.tobytes())
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
        return f"TokenGuide(V={self.V}, S={self.S}, C={self.C}, start={self.start})"

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

    def check_pickable(self, s0: int, always: Optional[bytes] = None, early: Optional[bytes] = None, until: int = 0,
                       first: Optional[bytes] = None, c0: int = 0) -> None:
        """ValueError when the sequence can reach a pick with nothing left: it starts in state s0 with c0 tokens generated; the pick after c
        tokens bans the state's set, `always`, `early` while c < until and `first` while c == 0 (llm.TokenRule)."""
        V = self.V
        a, e, f = (unpack_bits(m, V) for m in (always, early, first))
        until = int(until) if early is not None else 0

        def avail(ban):      # bool [C]: the class has a token outside `ban`
            p = np.zeros(self.C, dtype=bool)
            p[self.cls[~ban]] = True
            return p

        phases = {}
        cap = max(until, 1)      # counts from `cap` on are alike
        seen, todo = set(), [(int(s0), min(int(c0), cap))]
        while todo:
            s, c = todo.pop()
            if (s, c) in seen:
                continue
            seen.add((s, c))
            ph = (c == 0, c < until)
            if ph not in phases:
                phases[ph] = avail(a | (f if ph[0] else False) | (e if ph[1] else False))
            ok = (self.next[s] >= 0) & phases[ph]
            if not ok.any():
                raise ValueError(f"token guide: in state {s} after {c}{'+' if c == cap else ''} generated tokens the guide and the sequence's "
                                 f"token rule together ban all {V} tokens")
            todo += [(int(n), min(c + 1, cap)) for n in self.next[s][ok]]


def _ids(ids, V: int, what: str) -> List[int]:
    out = []
    for t in ids:
        if isinstance(t, (bool, float)) or not hasattr(t, "__index__") or not 0 <= int(t) < V:
            raise ValueError(f"{what}: token id {t!r} outside [0, {V})")
        out.append(int(t))
    return out


def region_answer(V: int, ground: int, ground_end: int, objects: int, objects_end: int, region_ids: Sequence[int], n_regions: int,
                  stop_ids: Sequence[int]) -> TokenGuide:
    """The FO1 answer language `<ground>label</ground><objects><region3><region7></objects>` with region indices below n_regions;
    region_ids[k] is the id of `<regionk>`.  States (OUT is the start):
      OUT     anything but </ground>, <objects>, </objects> and region_ids[n_regions:]; stop ids allowed; <ground> -> LABEL0
      LABEL0  one plain token (no structural token, no region token, no stop id) -> LABEL
      LABEL   plain tokens; </ground> -> OPEN
      OPEN    only <objects> -> OBJ0
      OBJ0    only region_ids[:n_regions] -> OBJ
      OBJ     region_ids[:n_regions]; </objects> -> OUT
    Every region id has a class of its own, so guides that differ in n_regions only share their class map."""
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
    return TokenGuide(cls, nx, OUT, V)


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
