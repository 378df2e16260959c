"""CPU checks of the budget-aware token guides' host side (vlm_fo1_amd/guide.py: accepting states, distances, closing_bitmaps,
check_pickable under a budget; the plans and table bookkeeping of vlm_fo1_amd/llm.py) against the brute force of tests/closing_cases.py:

  * distances and closing bitmaps of random automata (S <= 6, C <= 5, V = 63, empty classes, states without a path, always-bans) equal the
    plain enumeration of token strings for every (state, r <= 7);
  * from r = D on the closing set is the plain set — exactly for every state that leads to no state without a path, and the plain set plus
    the tokens into such states otherwise (check_pickable refuses a sequence that could take one);
  * accept=None is the guide built without the keyword: key, hash, bitmaps;
  * region_answer(close=True): the six distances, exactly three bitmaps beyond the plain ones that leave a token, two of them shared by
    guides that differ in n_regions only; the mask-row arithmetic of DESIGN.md section 14 (4 per box count + 5 shared);
  * 3900 walks under budgets 1..13, half uniform, half always as far from accepting as allowed: every one ends in OUT with well-formed text,
    while the same uniform walks without the rule leave answers open;
  * the dead ends check_pickable and llm.sampling_guides refuse."""
import numpy as np
import pytest

import closing_cases as K
import guide_cases as G
from vlm_fo1_amd import guide as TG
from vlm_fo1_amd import llm

V = K.V


def _ids(mask) -> set:
    return set(np.nonzero(~np.asarray(mask))[0].tolist())


def _bitmap_ids(bm) -> set:
    return _ids(TG.unpack_bits(bm, V))


def test_distances_and_closing_bitmaps_equal_the_enumeration_of_token_strings():
    guides = K.random_guides()
    n_inf = n_empty_class = n_sets = 0
    for g, always in guides:
        n_empty_class += not g.classes_present().all()
        dist = g.distances(always)
        D, rows = g.closing_bitmaps(always)
        assert D == max([int(dist[s]) for s in g.reachable() if dist[s] < TG.INF], default=0)
        assert (rows is None) == (D == 0)
        for s in range(g.S):
            # dist[s] by enumeration: the shortest string that closes, tried up to S tokens (a shortest path visits no state twice)
            want = 0 if s in g.accept else next((L for L in range(1, g.S + 1) if K.allowed_by_enumeration(g, s, L - 1, always)), TG.INF)
            assert dist[s] == want, (g, s, dist[s], want)
            n_inf += want == TG.INF
            for r in range(8):
                brute = K.allowed_by_enumeration(g, s, r, always)
                assert _ids(g.closing_mask(s, r, always)) == brute, (g, s, r)
                if r < D:
                    assert _bitmap_ids(rows[s][r]) == brute, (g, s, r)
                    assert (rows[s][r] is None) == (len(brute) == V)
                n_sets += 1
    assert n_inf > 0 and n_empty_class > 0 and n_sets > 400, (n_inf, n_empty_class, n_sets)


def test_from_depth_on_the_closing_set_is_the_plain_set():
    exact = widened = 0
    for g, always in K.random_guides() + [(K.region_guide(n), None) for n in (1, 5)]:
        dist, D = g.distances(always), g.depth(always)
        plain = g.state_bitmaps(always)
        present = np.zeros(g.C, dtype=bool)
        present[g.cls[~TG.unpack_bits(always, V)]] = True
        for s in g.reachable():
            into_dead = {int(c) for c in np.nonzero(present)[0] if g.next[s, c] >= 0 and dist[g.next[s, c]] >= TG.INF}
            for r in (D, D + 1, D + 5):
                got = g.closing_mask(s, r, always)
                if not into_dead:
                    assert TG.pack_bits(got) == (plain[s] or TG.pack_bits(np.zeros(V, bool))), (g, s, r)
                    exact += 1
                else:
                    dead = np.isin(g.cls, sorted(into_dead))
                    assert (got == (TG.unpack_bits(plain[s], V) | dead)).all(), (g, s, r)
                    widened += 1
                # what the device selects from D on is the plain row
                assert set(K.allowed(g, s, r, always).tolist()) == _bitmap_ids(plain[s])
    assert exact > 50 and widened > 0
    g = K.region_guide()
    assert all(g.closing_mask(s, r).tolist() == g.banned_mask(s).tolist() for s in range(6) for r in (5, 6, 40))


def test_accept_none_is_the_guide_without_the_keyword():
    g0 = K.region_guide(close=False)
    g1 = TG.TokenGuide(g0.cls, g0.next, g0.start, V, accept=None)
    g2 = TG.TokenGuide(g0.cls, g0.next, g0.start, V)
    assert g0.accept is None and g1._key == g2._key == g0._key and hash(g1) == hash(g2) == hash(g0) and g1 == g2 == g0
    always = TG.pack_bits(np.arange(V) % 9 == 0)
    assert g1.state_bitmaps() == g2.state_bitmaps() and g1.state_bitmaps(always) == g2.state_bitmaps(always)
    assert g1.closing_bitmaps() == (0, None) and (g1.distances() == TG.INF).all() and g1.depth() == 0
    gc = K.region_guide(close=True)
    assert gc != g0 and gc._key[:len(g0._key)] == g0._key and gc.accept == (TG.OUT,)
    assert gc.state_bitmaps() == g0.state_bitmaps()      # the plain tables are the same
    assert TG.TokenGuide(g0.cls, g0.next, 0, V, accept=[0, 0]) == gc and TG.TokenGuide(g0.cls, g0.next, 0, V, accept=iter((np.int64(0),))) == gc
    for bad in ([], [6], [-1], [0.0], [True], ["0"]):
        with pytest.raises(ValueError, match="accept"):
            TG.TokenGuide(g0.cls, g0.next, 0, V, accept=bad)
    wb = TG.ban_sequences([[7, 8], [9]], V)
    assert wb.accept is None and wb.closing_bitmaps() == (0, None)      # ban_sequences stays without accepting states


def _beyond_plain(g, always=None):
    """The closing bitmaps that are no plain bitmap of the guide and leave at least one token -> {bitmap: [(s, r), ...]}."""
    D, rows = g.closing_bitmaps(always)
    plain = set(g.state_bitmaps(always))
    full = TG.pack_bits(np.ones(V, bool))
    out = {}
    for s in range(g.S):
        for r in range(D):
            if rows[s][r] not in plain and rows[s][r] != full:
                out.setdefault(rows[s][r], []).append((s, r))
    return out


def test_region_answer_close_distances_bitmaps_and_mask_row_arithmetic():
    I = K.IDS
    g = K.region_guide(5)
    assert {s: int(d) for s, d in enumerate(g.distances())} == K.DIST and g.depth() == 5
    extra = _beyond_plain(g)
    assert len(extra) == 3
    by_where = {tuple(w): _bitmap_ids(bm) for bm, w in extra.items()}
    plain_out = _bitmap_ids(g.banned(TG.OUT))
    assert by_where[tuple((TG.OUT, r) for r in range(5))] == plain_out - {I["ground"]}      # OUT at r < 5 additionally bans <ground>
    assert by_where[((TG.LABEL, 3),)] == {I["ground_end"]}                                # LABEL at r = 3 allows only </ground>
    assert by_where[((TG.OBJ, 0),)] == {I["objects_end"]}                                 # OBJ at r = 0 allows only </objects>
    # every other (s, r) is the state's plain set, or a place no sequence can be in: more than r + 1 tokens from OUT, everything banned
    D, rows = g.closing_bitmaps()
    dist = g.distances()
    for s in range(6):
        for r in range(D):
            if (s, r) not in [w for ws in extra.values() for w in ws]:
                assert (rows[s][r] == g.state_bitmaps()[s]) if dist[s] <= r + 1 else (_bitmap_ids(rows[s][r]) == set()), (s, r)
    # guides that differ in n_regions only share two of the three
    g3 = K.region_guide(3)
    assert len(set(extra) & set(_beyond_plain(g3))) == 2 and len(_beyond_plain(g3)) == 3
    # the rows a pool spends (GuideTables.new_bitmaps over llm.guide_plan): 4 per distinct box count + 5 shared; 3 + 3 without the rule
    tab = llm.GuideTables(V, None, None)
    for close, per, shared in ((True, 4, 5), (False, 3, 3)):
        for ns in ([5], [5, 3], [1, 2, 3, 4, 5, 6, 7, 8]):
            plans = [llm.guide_plan(K.region_guide(n, close=close), None, TG.OUT) for n in ns]
            assert len(set(tab.new_bitmaps(plans))) == per * len(ns) + shared, (close, ns)
            assert tab.room(plans)
    p = llm.guide_plan(g, None, TG.OUT)
    assert p.depth == 5 and len(p.closing) == 30 and p.closing[TG.LABEL * 5 + 3] == rows[TG.LABEL][3]
    assert p.closing[TG.LABEL0 * 5 + 0] == p.bitmaps[TG.LABEL0]      # an unreachable place costs no row: the state's plain bitmap
    p0 = llm.guide_plan(K.region_guide(close=False), None, TG.OUT)
    assert p0.depth == 0 and p0.closing is None and p0.key != p.key
    # an always-ban is folded into every closing bitmap, as state_bitmaps folds it
    always = TG.pack_bits(np.isin(np.arange(V), [3, 40]))
    _, rows_a = g.closing_bitmaps(always)
    assert _bitmap_ids(rows_a[TG.OBJ][0]) == {I["objects_end"]} and _bitmap_ids(rows_a[TG.OUT][2]) == plain_out - {I["ground"], 3, 40}


def test_walks_under_every_budget_end_closed_and_the_control_does_not():
    g, gr = K.region_guide(), K.grammar()
    rng = np.random.default_rng(20261019)
    n = open_closing = open_control = 0
    for budget in range(1, 14):
        differed = 0
        for w in range(300):
            mode = "uniform" if w % 2 == 0 else "far"
            ids, s, d = K.walk(g, budget, rng, mode)
            differed += d
            n += 1
            open_closing += s != TG.OUT
            assert s == TG.OUT and len(ids) == budget and gr.state(ids) == "OUT", (budget, mode, ids)
            assert G.well_formed(gr.text(ids), K.N_ALLOWED), (budget, ids, gr.text(ids))
            if mode == "uniform":
                _, s0, _ = K.walk(g, budget, rng, mode, closing=False)
                open_control += s0 != TG.OUT
        assert differed > 0, budget      # the rule took part at every budget (OUT bans <ground> near the end even when nothing is open)
    assert n == 3900 and open_closing == 0
    assert open_control > 100, open_control      # the control: without the rule many of the 1950 uniform walks end inside a structure


def test_check_pickable_refuses_what_cannot_close():
    I = K.IDS
    g = K.region_guide()
    for s0 in range(6):      # a budget below dist[s0]
        d = K.DIST[s0]
        gs = K.region_guide(start=s0)
        gs.check_pickable(s0, budget=max(d, 1))
        gs.check_pickable(s0, budget=d + 7)
        if d > 1:
            with pytest.raises(ValueError, match=rf"state {s0} after 0 generated tokens is {d} tokens from an accepting state.*budget of {d - 1}"):
                gs.check_pickable(s0, budget=d - 1)
    # an always-ban of </objects>: OBJ never closes — no path from the start's successors
    no_close = TG.pack_bits(np.arange(V) == I["objects_end"])
    g.check_pickable(TG.OUT, always=no_close)      # without a budget: today's guide, which never runs dry
    with pytest.raises(ValueError, match="ban all 63 tokens|no path"):
        K.region_guide(start=TG.OBJ).check_pickable(TG.OBJ, always=no_close, budget=9)
    # ... and from OUT, where <ground> would lead into states that never close (no state but OUT has a distance: D = 0)
    with pytest.raises(ValueError, match="state 0 .* into state 1, from which no path leads to an accepting state"):
        g.check_pickable(TG.OUT, always=no_close, budget=9)
    assert g.distances(no_close)[TG.OBJ] == TG.INF and g.depth(no_close) == 0
    # a ban_first that removes the only closing token at N = dist[s0]
    first = TG.pack_bits(np.arange(V) == I["objects_end"])
    go = K.region_guide(start=TG.OBJ)
    go.check_pickable(TG.OBJ, first=first, budget=2)
    with pytest.raises(ValueError, match=r"in state 5 after 0 generated tokens with 0 tokens left of a budget of 1.*ban all 63"):
        go.check_pickable(TG.OBJ, first=first, budget=1)
    # min_new_tokens against the closing rule: stop ids are not the issue, a label too long for the budget is
    until = TG.pack_bits(np.isin(np.arange(V), [I["ground_end"]]))
    g.check_pickable(TG.OUT, early=until, until=3, budget=12)
    with pytest.raises(ValueError, match="ban all 63"):
        K.region_guide(start=TG.LABEL).check_pickable(TG.LABEL, early=until, until=3, budget=4)      # LABEL must close at c = 0
    # the plumbing: sampling_guides passes the budget, and refuses a closing guide without one
    sp = dict(greedy=True, guide=K.region_guide(start=TG.LABEL0))
    with pytest.raises(ValueError, match="5 tokens from an accepting state"):
        llm.sampling_guides([sp], 1, V, [None], budget=4)
    (plan,) = llm.sampling_guides([sp], 1, V, [None], budget=5)
    assert plan.depth == 5 and plan.s0 == TG.LABEL0
    with pytest.raises(ValueError, match="budget"):
        llm.sampling_guides([sp], 1, V, [None])
    spb = dict(greedy=True, guide=K.region_guide(start=TG.OBJ), ban=[I["objects_end"]])
    with pytest.raises(ValueError):
        llm.sampling_guides([spb], 1, V, llm.sampling_rules([spb], 1, V), budget=9)
    # without accepting states the budget changes nothing
    (p0,) = llm.sampling_guides([dict(greedy=True, guide=K.region_guide(close=False))], 1, V, [None], budget=1)
    assert p0.depth == 0 and p0.closing is None


def test_a_long_budget_and_a_token_rule_do_not_meet_where_they_cannot():
    """c and r are linked (c + r = N - 1): under a long budget the early phase (c < until) and the closing phase (r < D) never coincide, and
    the walk must not pretend they do."""
    I = K.IDS
    g = K.region_guide(start=TG.OBJ)
    until = TG.pack_bits(np.arange(V) == I["objects_end"])      # </objects> banned for the first 3 tokens
    g.check_pickable(TG.OBJ, early=until, until=3, budget=40)
    g.check_pickable(TG.OBJ, early=until, until=3, budget=4)      # c = 3 is the last pick: r = 0, </objects> allowed again
    with pytest.raises(ValueError, match="ban all 63"):
        g.check_pickable(TG.OBJ, early=until, until=3, budget=3)
