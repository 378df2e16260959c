"""Definition, oracles and cases of the guided decode head: the banned set of a pick as a function of a per-row automaton state that the head
advances itself (sample_rows_kernel's GUIDE instantiations in vlm_fo1_amd/csrc/sample.hip, behind fo1_sample_rows_guided_bf16 and
fo1_decode_head_guided_accept; host side vlm_fo1_amd/guide.py).  Shared by tests/test_guide_cases.py (CPU),
tests/test_guide_head_gpu.py and tests/test_guide_decode_gpu.py (MI355X).  Builds on constraint_cases, penalty_cases and sampling_cases and
changes none of them.

Definition.  A guide is (cls[V], next[S][C], start): the banned set of state s is { t : next[s][cls[t]] < 0 }, held as a row of the mask table
that state_row names; a banned token is a non-finite entry, exactly as for a token rule (constraint_cases.mask), and everything else about the
pick is the ruled head's.  After the pick of token t in state s the state is next[s][cls[t]], or s when that entry is negative.

Tolerance.  The device forms the same fixed-order fp32 partial sums as without a guide, with some weights replaced by 0: the accept rule and
EPS = 2^-17 of tests/sampling_cases.py hold unchanged — no new tolerance.  A (row, state) pair whose masked oracle keeps less than
EXACT_MARGIN * EPS between the mass above a key and top_p Z1 is left out, decided on the oracle alone; at most 2 % of the pairs (left_out()).

Head cases (head_cases()).  Every row of sampling_cases.rows_and_batches() at V in {63, 4099, 32773} crossed with the five states of a guide
whose state bitmaps are constraint_cases' ban kinds HEAD_KINDS: empty; the row's argmax; every 8th id plus the byte and word boundaries; an
allow-list of 16; the unaligned tail.  At the head level the bitmaps and the transitions are independent operands (the kernel reads the one
from the mask table and the other from cls / next), so the head guide's class map is a fixed scatter of the ids over 6 classes and its
5 x 6 transition table (HEAD_NEXT) has negative entries in every state: `gstate` after a launch must equal head_guide(V).advance(s, id) —
a move for most picks, "the state stays" for the rest.

The FO1 answer language is restated naively here (Grammar) from the state table of guide.region_answer, as the reference the builder's
automaton, transformers' PrefixConstrainedLogitsProcessor and the decode test's replay are compared with."""
from __future__ import annotations

from typing import List

import numpy as np

import constraint_cases as C
import penalty_cases as P
import sampling_cases as S

HEAD_KINDS = ("empty", "argmax", "every8", "allow16", "tail")      # the banned set of head state s is constraint_cases.ban_set(HEAD_KINDS[s], row)
CASE_V = C.CASE_V
MAX_LEFT_OUT = 0.02
N_CLASSES = 6
# state after class c in state s; -1 = the state stays (at the head level the mask table, not this table, decides what is banned)
HEAD_NEXT = np.array([[1, 2, 3, 4, 0, -1],
                      [2, -1, 4, 0, 1, 3],
                      [-1, 3, 0, 1, 2, 4],
                      [4, 0, -1, 2, 3, 1],
                      [0, 1, 2, -1, 4, 3]], dtype=np.int32)


def head_cls(V: int) -> np.ndarray:
    """uint16 [V]: every class among any 8 consecutive ids' neighbourhood, the argmax's class differing from row to row."""
    t = np.arange(V, dtype=np.int64)
    return ((t * 5 + (t >> 3) + (t >> 7)) % N_CLASSES).astype(np.uint16)


_cache: dict = {}


def head_guide(V: int):
    """The head cases' TokenGuide over V tokens (start state 0)."""
    from vlm_fo1_amd.guide import TokenGuide
    if ("g", V) not in _cache:
        _cache[("g", V)] = TokenGuide(head_cls(V), HEAD_NEXT, 0, V)
    return _cache[("g", V)]


def head_cases() -> List[dict]:
    """constraint_cases' case dicts (name, V, bits, kind, banned, seen, p, T, top_p, top_k, rbits, oracle, draws) plus state = the guide state
    whose bitmap is `banned`, and row = the sampler row's name (the five states of a row share one guide)."""
    if "c" in _cache:
        return _cache["c"]
    rows, _ = S.rows_and_batches()
    out, pairs, left = [], 0, []
    for V in CASE_V:
        rng = np.random.default_rng(9000 + V)
        for r in (r for r in rows if r["V"] == V):
            for s, kind in enumerate(HEAD_KINDS):
                c = C._case(r["name"], r["bits"], kind, r["T"], r["top_p"], r["top_k"], rng, "planted" in r["name"])
                pairs += 1
                if c["draws"] is None:      # the masked row's top-p cut-off sits within 16 EPS of top_p Z1: left out, and counted
                    left.append(c["name"])
                    continue
                c["state"], c["row"] = s, r["name"]
                out.append(c)
    _cache["c"] = out
    _cache["left"] = (left, pairs)
    return out


def left_out():
    """-> (names of the (row, state) pairs left out for their top-p margin, number of pairs)."""
    head_cases()
    return _cache["left"]


def greedy_head_cases() -> List[dict]:
    """Greedy rows: dicts(name, V, bits, state, banned, want = the first index of the largest entry outside the state's banned set).  The
    row's three largest entries are tied, the first of them the argmax that state 1 bans and a multiple of 8 that state 2 bans."""
    if "gr" in _cache:
        return _cache["gr"]
    out = []
    for V in CASE_V:
        rng = np.random.default_rng(9500 + V)
        for j in range(3):
            x = (rng.standard_normal(V) * 2).astype(np.float32)
            x[sorted({8 * (1 + j), V // 2 + j, V - 1 - j})] = 20.0
            bits = S.to_bits(x)
            for s, kind in enumerate(HEAD_KINDS):
                banned = C.ban_set(kind, bits)
                out.append(dict(name=f"V{V}-ties{j}|{kind}", V=V, bits=bits, state=s, banned=banned, want=P.greedy_pick(C.mask(bits, banned))))
    _cache["gr"] = out
    return out


class Grammar:
    """The FO1 answer language, restated naively from guide.region_answer's state table: a scan of the ids generated so far names the state,
    and allowed() lists what may follow.  ids: the four structural ids, region[k] = the id of <regionk>, n = the request's boxes, stops."""

    def __init__(self, V, ground, ground_end, objects, objects_end, region, n, stops):
        self.V, self.g, self.ge, self.o, self.oe = V, ground, ground_end, objects, objects_end
        self.region, self.n, self.stops = list(region), n, set(stops)
        self.special = {ground, ground_end, objects, objects_end} | set(region) | self.stops

    def plain(self, t) -> bool:
        return t not in self.special

    def state(self, ids) -> str:
        st = "OUT"
        for t in ids:
            if st == "OUT":
                st = "LABEL0" if t == self.g else "OUT"
            elif st == "LABEL0":
                st = "LABEL"
            elif st == "LABEL":
                st = "OPEN" if t == self.ge else "LABEL"
            elif st == "OPEN":
                st = "OBJ0"
            elif st == "OBJ0":
                st = "OBJ"
            else:
                st = "OUT" if t == self.oe else "OBJ"
        return st

    def allowed(self, ids) -> List[int]:
        st = self.state(ids)
        good = self.region[:self.n]
        if st == "OUT":
            no = {self.ge, self.o, self.oe} | set(self.region[self.n:])
            return [t for t in range(self.V) if t not in no]
        if st == "LABEL0":
            return [t for t in range(self.V) if self.plain(t)]
        if st == "LABEL":
            return [t for t in range(self.V) if self.plain(t) or t == self.ge]
        if st == "OPEN":
            return [self.o]
        if st == "OBJ0":
            return sorted(good)
        return sorted(good + [self.oe])

    def text(self, ids) -> str:
        """The ids as the tokenizer would print them: structural tokens by name, <regionk>, a letter per plain id, nothing for a stop id."""
        names = {self.g: "<ground>", self.ge: "</ground>", self.o: "<objects>", self.oe: "</objects>"}
        names.update({t: f"<region{k}>" for k, t in enumerate(self.region)})
        return "".join("" if t in self.stops else names.get(t, chr(ord("a") + t % 26)) for t in ids)


def well_formed(text: str, n_regions: int) -> bool:
    """The plug-in's own parsers accept all of `text`: every structural token belongs to a <ground>label</ground><objects>...</objects> match
    with a non-empty label, at least one region, and no region index at or beyond n_regions anywhere."""
    from vlm_fo1.mm_utils import _GROUND_RE, _REGION_RE
    if any(int(k) >= n_regions for k in _REGION_RE.findall(text)):
        return False
    for label, body in _GROUND_RE.findall(text):
        if not label or "<" in label or not _REGION_RE.findall(body) or _REGION_RE.sub("", body):
            return False
    rest = _GROUND_RE.sub("", text)
    return not any(s in rest for s in ("<ground>", "</ground>", "<objects>", "</objects>"))
