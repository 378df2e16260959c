"""The closing decode head on the MI355X, on bare logit rows (vlm_fo1_amd/csrc/sample.hip: the CLOSE instantiations behind
fo1_sample_rows_closing_bf16 and fo1_decode_head_closing_accept; definition and cases: tests/closing_cases.py, tests/guide_cases.py).

At the head level the mask table, state_row and close_row are independent operands, so the sampled and greedy cases of guide_cases are run
with a case's banned set planted as the row of (state, r) for r < depth = 3 and the NEXT ban kind planted as the state's plain row: with
r in {0, 1, 2} tokens left the pick must follow the case's own oracle, with r in {3, 7} the oracle of the case of the same logits row one
state further — the bitmap the definition selects.  V in {63, 4099}: byte and word boundaries, an unaligned tail, more than one slice.

  * rows form, explicit draws: every exact draw equals the selected oracle's id, every other one meets the accept rule at EPS = 2^-17
    unchanged; `gstate` equals head_guide(V).advance(s, id); every table sits in a canary frame that a second launch leaves intact;
  * accept form, Philox draws, r = min(state[b][5], ids_ld) - state[b][4] - 1, ids_ld binding for some launches;
  * greedy rows through both forms;
  * a region_answer(close=True) guide against logits that want `<ground>` most and the closing tokens least: budgets 1..8 in one sequence of
    8 launches, greedy and sampled rows — every row's ids are well-formed, end in OUT and fill the budget; the same rows through
    fo1_decode_head_guided_accept leave answers open (the control);
  * closes = NULL is bitwise the _guided entry; depth = 0, no guide, a finished row, close_off / depth past close_row: as defined, in one
    launch next to closing rows; the same row alone and at row 37 of 64; the accept form under graph replay equals eager.

RESULTS_GPU (MI355X): 59 x 2 launches of the rows form: 10275 exact draws equal the selected oracle's id, 4641 meet the accept rule; 8958 picks
behind a closing row, 5958 behind the plain row.  Through the accept form: 846 exact / 38 inside the accept rule with the budget binding, 839 / 45
with ids_ld binding.  The whole file runs in about 3 s."""
import numpy as np
import pytest
import torch

import closing_cases as K
import constraint_cases as C
import guide_cases as G
import penalty_cases as P
import sampling_cases as S
import test_constraint_head_gpu as H
import test_guide_head_gpu as GH

pytestmark = pytest.mark.gpu

CASE_V = (63, 4099)
DEPTH = 3
LEFT = (0, 1, 2, 3, 7)
CLOSE_OFF = 5
CANARY32 = GH.CANARY32


class CloseTables(GH.Tables):
    """GH.Tables plus the closing operands, each inside a canary frame: close_row (`close_rows` from CLOSE_OFF on), closes [B] and, for the
    rows form, budget [B]."""

    def __init__(self, ops, V, state_rows, guides, states, close_rows, closes, budget=None):
        super().__init__(ops, V, state_rows, guides, states)
        B = self.B
        cr = np.full(8 + CLOSE_OFF + len(close_rows) + 8, CANARY32, np.int64)
        cr[8 + CLOSE_OFF:8 + CLOSE_OFF + len(close_rows)] = close_rows
        self.h_cr = cr.astype(np.uint32)
        self.d_cr = GH._i32(cr)
        self.n_cr = CLOSE_OFF + len(close_rows)
        self.h_closes = ops.guide_closes(closes)
        cd = torch.full((B + 2, 4), 0x5a5a5a5a, dtype=torch.int32)
        cd[1:-1] = self.h_closes
        self.d_closes = cd.cuda()
        bd = torch.full((B + 16,), S.CANARY, dtype=torch.int32)
        if budget is not None:
            bd[8:8 + B] = torch.tensor(budget, dtype=torch.int32)
        self.h_budget = bd.clone()
        self.d_budget = bd.cuda()
        self.guided_op = self.op
        self.op = ops.GuideOperands(*self.op[:5], self.d_cr[8:8 + self.n_cr], self.d_closes[1:-1], self.d_budget[8:8 + B] if budget is not None else None)

    def assert_intact(self):
        super().assert_intact()
        assert (self.d_cr.cpu().numpy().view(np.uint32) == self.h_cr).all(), "the close-row table or its frame was written"
        cd = self.d_closes.cpu()
        assert torch.equal(cd[1:-1], self.h_closes) and (cd[0] == 0x5a5a5a5a).all() and (cd[-1] == 0x5a5a5a5a).all(), "the closing table was written"
        assert torch.equal(self.d_budget.cpu(), self.h_budget), "the budgets or their frame were written"


def _planted(rows_bits, V):
    """Per distinct logits row (group g): mask sets of the five ban kinds; state_row[5 g + s] = the row of kind s + 1 (the plain row is a
    DIFFERENT kind), close_row[(5 g + s) * DEPTH + r] = the row of kind s -> (sets, state_row entries, close_row entries)."""
    sets, kind_row = GH._group_tables(rows_bits, V)      # kind_row[5 g + k]: mask row of kind k (-1: the empty kind of an even group)
    sr = [kind_row[5 * (i // 5) + (i % 5 + 1) % 5] for i in range(len(kind_row))]
    cr = [kind_row[i] for i in range(len(kind_row)) for _ in range(DEPTH)]
    return sets, sr, cr


def _close_row(group: int):
    return (CLOSE_OFF + 5 * DEPTH * group, DEPTH)


def _selected(case_of, c, r):
    """The case whose banned set the definition selects for case c's row in state c.state with r tokens left (None: left out for its margin)."""
    return c if r < DEPTH else case_of.get((c["row"], (c["state"] + 1) % 5))


def test_sampled_rows_follow_the_bitmap_the_definition_selects_through_the_rows_form():
    from vlm_fo1_amd import ops
    cs = [c for c in G.head_cases() if c["V"] in CASE_V]
    case_of = {(c["row"], c["state"]): c for c in cs}
    n_exact = n_rule = n_close = n_plain = launches = 0
    for V in CASE_V:
        guide = G.head_guide(V)
        pr = []
        for c in (c for c in cs if c["V"] == V):
            for r in LEFT:
                e = _selected(case_of, c, r)
                if e is not None:
                    pr += [(c, e, r, u) for u in e["draws"]]
        for a in range(0, len(pr), 256):
            chunk = pr[a:a + 256]
            n = len(chunk)
            dl, seen = H._rows_buffer([(c["bits"], c["seen"]) for c, *_ in chunk], V)
            names = sorted({c["row"] for c, *_ in chunk})
            bits_of = {c["row"]: c["bits"] for c, *_ in chunk}
            sets, sr, cr = _planted([bits_of[k] for k in names], V)
            buf, masks, host = H._framed_masks(sets, V)
            ctr = [b % 5 for b in range(n)]
            t = CloseTables(ops, V, sr, [GH._guide_row(names.index(c["row"])) for c, *_ in chunk], [c["state"] for c, *_ in chunk], cr,
                            [_close_row(names.index(c["row"])) for c, *_ in chunk], [ctr[b] + r + 1 for b, (_, _, r, _) in enumerate(chunk)])
            params = ops.sample_params([(e["T"], e["top_p"], e["top_k"], 0, b, False, 0.0) for b, (_, e, _, _) in enumerate(chunk)], "cuda")
            out = torch.full((n + 16,), S.CANARY, dtype=torch.int32, device="cuda")
            u = torch.tensor([u for *_, u in chunk], dtype=torch.float32).cuda()
            rules = ops.token_rules([None] * n, "cuda")
            counter = torch.tensor(ctr, dtype=torch.int32).cuda()
            ops.sample_rows(dl, params, counter=counter, u=u, out=out[8:8 + n], seen=seen, masks=masks, rules=rules, guide=t.op)
            launches += 1
            got, after = out.cpu().numpy(), t.states()
            assert (got[:8] == S.CANARY).all() and (got[8 + n:] == S.CANARY).all(), "the id buffer's canary was overwritten"
            for b, (c, e, r, uu) in enumerate(chunk):
                o, g = e["oracle"], int(got[8 + b])
                assert S.accepts(o, uu, g), (c["name"], r, b, uu, g, S.pick(o, uu))
                assert o.empty or g not in e["banned"], (c["name"], r, b, g)
                if S.is_exact(o, uu):
                    n_exact += 1
                    assert g == S.pick(o, uu), (c["name"], r, b, uu, g, S.pick(o, uu))
                else:
                    n_rule += 1
                assert after[b] == guide.advance(c["state"], g), (c["name"], r, b, c["state"], g, after[b])
                n_close += r < DEPTH
                n_plain += r >= DEPTH
            ops.sample_rows(dl, params, counter=counter, u=u, out=out[8:8 + n], seen=seen, masks=masks, rules=rules, guide=t.op)
            t.assert_intact()
            assert (buf.cpu().numpy().view(np.uint32) == host).all(), "the mask table or its frame was written"
    print(f"\n{launches} x 2 launches: {n_exact} exact draws equal the selected oracle, {n_rule} meet the accept rule; {n_close} picks behind a "
          f"closing row, {n_plain} behind the plain row")
    assert n_exact > n_rule > 0 and n_close > n_plain > 0


@pytest.mark.parametrize("ld_binds", [False, True], ids=["budget", "ids_ld"])
def test_sampled_rows_through_the_accept_form_with_philox_draws(ld_binds):
    """r = min(state[b][5], ids_ld) - state[b][4] - 1: with ld_binds every row's state[b][5] is far away and ids_ld (one per launch) sets r."""
    from vlm_fo1_amd import ops
    seed = 0xc105e
    cs = [c for c in G.head_cases() if c["V"] in CASE_V]
    case_of = {(c["row"], c["state"]): c for c in cs}
    n_exact = n_rule = 0
    for V in CASE_V:
        guide = G.head_guide(V)
        for r in LEFT:
            pr = [(c, _selected(case_of, c, r)) for c in cs if c["V"] == V][r % 2::2][:256]
            pr = [(c, e) for c, e in pr if e is not None]
            n = len(pr)
            dl, seen = H._rows_buffer([(c["bits"], c["seen"]) for c, _ in pr], V)
            names = sorted({c["row"] for c, _ in pr})
            bits_of = {c["row"]: c["bits"] for c, _ in pr}
            sets, sr, cr = _planted([bits_of[k] for k in names], V)
            _, masks, _ = H._framed_masks(sets, V)
            states = [c["state"] for c, _ in pr]
            t = CloseTables(ops, V, sr, [GH._guide_row(names.index(c["row"])) for c, _ in pr], states, cr,
                            [_close_row(names.index(c["row"])) for c, _ in pr])
            params = ops.sample_params([(e["T"], e["top_p"], e["top_k"], seed, b, False, 0.0) for b, (_, e) in enumerate(pr)], "cuda")
            ctr = [4] * n if ld_binds else [b % 7 for b in range(n)]
            cap = 4 + r + 1 if ld_binds else 6 + r + 1 + 4
            st = torch.tensor([[5, 5, 0, 0, k, 1000 if ld_binds else k + r + 1, 0, 0] for k in ctr], dtype=torch.int32).cuda()
            plan = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
            ids = torch.full((n, cap), -1, dtype=torch.int32, device="cuda")
            done = torch.zeros(1, dtype=torch.int32, device="cuda")
            ops.decode_head_accept(dl, params, st, plan, ids, None, done, seen=seen, masks=masks, rules=ops.token_rules([None] * n, "cuda"), guide=t.op)
            rec, after, sth = ids.cpu(), t.states(), st.cpu()
            for b, (c, e) in enumerate(pr):
                o, g, u = e["oracle"], int(rec[b, ctr[b]]), S.draw_u(ctr[b], b, seed)
                assert S.accepts(o, u, g), (c["name"], r, b, u, g, S.pick(o, u))
                assert o.empty or g not in e["banned"], (c["name"], r, b, g)
                if S.is_exact(o, u):
                    n_exact += 1
                    assert g == S.pick(o, u), (c["name"], r, b, u, g, S.pick(o, u))
                else:
                    n_rule += 1
                assert after[b] == guide.advance(states[b], g) and int(sth[b, 4]) == ctr[b] + 1, (c["name"], b)
                assert int(sth[b, 3]) == (r == 0), (c["name"], r, b)      # the row finishes exactly when nothing may follow
            t.assert_intact()
    print(f"\naccept form ({'ids_ld' if ld_binds else 'budget'} binds): {n_exact} exact draws equal the selected oracle, {n_rule} meet the accept rule")
    assert n_exact > n_rule and n_exact + n_rule >= 500


def test_greedy_rows_through_both_forms_and_graph_replay_equals_eager():
    from vlm_fo1_amd import ops
    total = 0
    for V in CASE_V:
        guide = G.head_guide(V)
        base = [g for g in G.greedy_head_cases() if g["V"] == V]
        want_of = {(g["name"].split("|")[0], g["state"]): g["want"] for g in base}
        gs = [(g, r) for g in base for r in LEFT]
        B = len(gs)
        keys = sorted({g["name"].split("|")[0] for g, _ in gs})
        bits_of = {g["name"].split("|")[0]: g["bits"] for g, _ in gs}
        dl, _ = H._rows_buffer([(g["bits"], []) for g, _ in gs], V)
        sets, sr, cr = _planted([bits_of[k] for k in keys], V)
        buf, masks, host = H._framed_masks(sets, V)
        grp = [keys.index(g["name"].split("|")[0]) for g, _ in gs]
        guides, closes = [GH._guide_row(k) for k in grp], [_close_row(k) for k in grp]
        states = [g["state"] for g, _ in gs]
        want = [want_of[(g["name"].split("|")[0], g["state"] if r < DEPTH else (g["state"] + 1) % 5)] for g, r in gs]
        assert any(w != g["want"] for w, (g, r) in zip(want, gs) if r >= DEPTH), "the planted plain row moves no greedy pick"
        params = ops.sample_params([(0.3 + b, 0.5, 7, 99, b, True, 0.0) for b in range(B)], "cuda")
        rules = ops.token_rules([None] * B, "cuda")
        ctr = [b % 4 for b in range(B)]
        t = CloseTables(ops, V, sr, guides, states, cr, closes, [ctr[b] + r + 1 for b, (_, r) in enumerate(gs)])
        got = ops.sample_rows(dl, params, counter=torch.tensor(ctr, dtype=torch.int32).cuda(), masks=masks, rules=rules, guide=t.op).cpu().tolist()
        assert got == want, [(g["name"], r, x, w) for (g, r), x, w in zip(gs, got, want) if x != w]
        assert t.states() == [guide.advance(s, x) for s, x in zip(states, got)]
        t.assert_intact()
        # the accept form, eager: three steps with the budget three steps away for r = 2, ... — the first step is the one checked against `want`
        t = CloseTables(ops, V, sr, guides, states, cr, closes)
        cap = max(ctr) + max(LEFT) + 2
        state = torch.tensor([[5, 5, 0, 0, k, k + r + 1, 0, 0] for k, (_, r) in zip(ctr, gs)], dtype=torch.int32).cuda()
        plan, ids = torch.zeros(B, 2, dtype=torch.int32, device="cuda"), torch.full((B, cap), -1, dtype=torch.int32, device="cuda")
        done = torch.zeros(1, dtype=torch.int32, device="cuda")
        live = (state, plan, ids, done, t.d_gs)
        keep = [x.clone() for x in live]

        def step():
            ops.decode_head_accept(dl, params, state, plan, ids, None, done, masks=masks, rules=rules, guide=t.op)
        step()
        rec, after = ids.cpu(), t.states()
        for b in range(B):
            assert int(rec[b, ctr[b]]) == want[b] and after[b] == guide.advance(states[b], want[b]), (gs[b][0]["name"], gs[b][1], b)
        step()
        step()
        eager = [x.clone() for x in live]
        assert int(done.item()) == sum(r <= 2 for _, r in gs)      # rows with r = 0, 1, 2 have used their budgets up, the others not
        t.assert_intact()
        assert (buf.cpu().numpy().view(np.uint32) == host).all()
        # captured (the warm-up step rolled back: gstate is among what the step writes) and replayed three times from the start
        for x, x0 in zip(live, keep):
            x.copy_(x0)
        g, _ = ops.capture_graph(step, rollback=live)
        for x, x0 in zip(live, keep):
            assert torch.equal(x, x0)
        for _ in range(3):
            ops.replay_graph(g)
        torch.cuda.synchronize()
        for x, e, name in zip(live, eager, ("state", "plan", "ids", "done", "gstate")):
            assert torch.equal(x, e), name
        t.assert_intact()
        total += B
    assert total == 2 * 15 * len(LEFT)


def _region_tables(ops, g, n_rows, always=None):
    """Device tables of one region guide for n_rows rows that all carry it: the mask table from its bitmaps, one class row, next, state_row and
    close_row as llm.guide_plan flattens them."""
    from vlm_fo1_amd import llm
    plan = llm.guide_plan(g, always, g.start)
    maps = sorted({m for m in plan.bitmaps + (plan.closing or ()) if m is not None})
    row = {m: i for i, m in enumerate(maps)}
    masks = torch.from_numpy(np.stack([np.frombuffer(m, dtype=np.int32) for m in maps]).copy()).cuda()
    cls = torch.from_numpy(g.cls.view(np.int16).copy()).view(1, -1).cuda()
    nxt = torch.from_numpy(g.next.reshape(-1).copy()).cuda()
    sr = torch.tensor([-1 if m is None else row[m] for m in plan.bitmaps], dtype=torch.int32).cuda()
    cr = torch.tensor([-1 if m is None else row[m] for m in plan.closing], dtype=torch.int32).cuda()
    guides = ops.token_guides([(0, g.C, 0, 0)] * n_rows, "cuda")
    closes = ops.guide_closes([(0, plan.depth)] * n_rows, "cuda")
    return masks, cls, nxt, sr, cr, guides, closes


def test_adversarial_logits_close_under_every_budget_and_the_guided_head_does_not():
    """Budgets 1..8, a greedy and three sampled rows each, 8 launches of the accept form: the logits want <ground> most, then plain tokens,
    then region ids, and the closing tokens and stop ids least — every closing token is the head's last choice."""
    from vlm_fo1_amd import ops
    I, V = K.IDS, K.V
    g, gr = K.region_guide(), K.grammar()
    x = np.full(V, 2.0, np.float32) + np.linspace(0.0, 1.0, V, dtype=np.float32)      # plain tokens
    x[I["region"]] = 0.5
    x[[I["ground_end"], I["objects"], I["objects_end"]]] = -6.0
    x[I["stops"]] = -9.0
    x[I["ground"]] = 8.0
    budgets = [b for b in range(1, 9) for _ in range(4)]
    B = len(budgets)
    # T = 0.7: <ground> is 98 % of an OUT pick that allows it (52 plain tokens of weight <= exp(-5 / 0.7) beside it), a closing token or a stop
    # id 1e-9 of any pick — a sampled row behaves as a greedy one nearly always, and the bounds below leave room for the rest
    rows = [(0.7, 1.0, 0, 0xad0 + b, b, b % 4 == 0, 0.0) for b in range(B)]
    dl, _ = H._rows_buffer([(S.to_bits(x), [])] * B, V)
    params = ops.sample_params(rows, "cuda")
    masks, cls, nxt, sr, cr, guides, closes = _region_tables(ops, g, B)
    rules = ops.token_rules([None] * B, "cuda")
    stop = torch.tensor(I["stops"], dtype=torch.int32).cuda()

    def run(closing: bool):
        gstate = torch.full((B,), g.start, dtype=torch.int32, device="cuda")
        op = ops.GuideOperands(cls, nxt, sr, guides, gstate, *((cr, closes) if closing else ()))
        st = torch.tensor([[5, 5, 0, 0, 0, n, 0, 0] for n in budgets], dtype=torch.int32).cuda()
        plan, ids = torch.zeros(B, 2, dtype=torch.int32, device="cuda"), torch.full((B, 8), -1, dtype=torch.int32, device="cuda")
        done = torch.zeros(1, dtype=torch.int32, device="cuda")
        for _ in range(8):
            ops.decode_head_accept(dl, params, st, plan, ids, stop, done, masks=masks, rules=rules, guide=op)
        return ids.cpu().tolist(), gstate.cpu().tolist(), st.cpu().tolist(), int(done.item())

    ids, states, st, done = run(True)
    assert done == B
    grounded = 0
    for b, n in enumerate(budgets):
        got = ids[b][:n]
        assert st[b][4] == n and st[b][3] == 1 and all(t >= 0 for t in got) and all(t == -1 for t in ids[b][n:]), (b, n, ids[b])      # its length equals its budget
        assert states[b] == TG_OUT == g.run(got) and gr.state(got) == "OUT", (b, n, got, states[b])
        assert G.well_formed(gr.text(got), K.N_ALLOWED), (b, n, gr.text(got))
        grounded += I["ground"] in got
        assert (I["ground"] in got) == (n >= 6) or not rows[b][5], (b, n, got)      # a greedy row opens a structure whenever one fits (6 tokens)
    assert grounded >= 8, grounded      # of the 12 rows with 6 or more tokens: the 3 greedy ones, and each sampled one with probability 0.98
    ids0, states0, st0, _ = run(False)      # the control: the same rows through fo1_decode_head_guided_accept
    opened = [b for b, n in enumerate(budgets) if states0[b] != TG_OUT]
    assert len(opened) >= B // 2, (opened, states0)
    assert all(not G.well_formed(gr.text(ids0[b][:budgets[b]]), K.N_ALLOWED) or states0[b] == TG_OUT for b in range(B))


TG_OUT = 0      # guide.OUT


def _mixed_closing(V: int, B: int):
    """GH._mixed's rows (greedy / sampled x penalised or not x guided or not) with closing rows among the guided ones -> the close rows and
    tokens left per row: b % 4 == 3 has depth = 0, the others depth = 3 with r = b % 5."""
    bits, items, rows, guides, states, _, _ = GH._mixed(V, B)
    sets, sr, cr = _planted(list(bits), V)
    closes = [None if guides[b] is None else ((0, 0) if b % 4 == 3 else _close_row(b)) for b in range(B)]
    left = [b % 5 for b in range(B)]
    return bits, items, rows, guides, states, sets, sr, cr, closes, left


def _expect(bits, items, rows, kind):
    rb = C.ruled(bits, C.ban_set(kind, bits), items[1], rows[6])
    return rb


def test_rows_without_a_closing_rule_and_indices_past_close_row_behave_as_defined():
    from vlm_fo1_amd import lib as L, ops
    V, B = 4099, 16
    bits, items, rows, guides, states, sets, sr, cr, closes, left = _mixed_closing(V, B)
    guide = G.head_guide(V)
    dl, seen = H._rows_buffer(items, V)
    _, masks, _ = H._framed_masks(sets, V)
    params = ops.sample_params(rows, "cuda")
    ctr = [3 + b % 5 for b in range(B)]
    counter = torch.tensor(ctr, dtype=torch.int32).cuda()
    budget = [ctr[b] + left[b] + 1 for b in range(B)]
    rules = ops.token_rules([(sr[5 * b + 2], -1, 0, -1) for b in range(B)], "cuda")      # a rule of its own on every row, as in GH
    ruled = ops.sample_rows(dl, params, counter=counter, seen=seen, masks=masks, rules=rules).cpu().tolist()
    t = CloseTables(ops, V, sr, guides, states, cr, closes, budget)
    guided = ops.sample_rows(dl, params, counter=counter, seen=seen, masks=masks, rules=rules, guide=t.guided_op).cpu().tolist()
    after_guided = t.states()
    t = CloseTables(ops, V, sr, guides, states, cr, closes, budget)
    got = ops.sample_rows(dl, params, counter=counter, seen=seen, masks=masks, rules=rules, guide=t.op).cpu().tolist()
    after = t.states()
    moved = 0
    for b in range(B):
        if guides[b] is None:                                  # no guide: the _ruled entry's id, gstate untouched
            assert got[b] == ruled[b] and after[b] == states[b], b
        elif closes[b][1] == 0 or left[b] >= DEPTH:            # depth = 0, or r >= depth: the _guided entry's id and state (the plain row)
            assert got[b] == guided[b] and after[b] == after_guided[b], b
        else:                                                  # a closing row: the set of kind s (the plain row holds kind s + 1)
            rb = C.ruled(bits[b], C.ban_set(G.HEAD_KINDS[states[b]], bits[b]), items[b][1], rows[b][6])
            if rows[b][5]:
                assert got[b] == P.greedy_pick(rb), b
            else:
                assert S.accepts(S.oracle(rb, *rows[b][:3]), S.draw_u(ctr[b], rows[b][4], rows[b][3]), got[b]), b
            assert after[b] == guide.advance(states[b], got[b]), b
            moved += got[b] != guided[b]
    assert moved > 0, "the closing rows moved no pick"
    t.assert_intact()
    # closes = NULL: bitwise the _guided entry, through the C entry itself
    lib = L.load()
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    t = CloseTables(ops, V, sr, guides, states, cr, closes, budget)
    o = t.op

    def rows_entry(close_row, n_close_row, closes_p, budget_p):
        return lib.fo1_sample_rows_closing_bf16(dl.data_ptr(), dl.stride(0), V, B, params.data_ptr(), counter.data_ptr(), 1, None, out.data_ptr(), ws.data_ptr(),
                                                4096, seen.data_ptr(), seen.shape[1], masks.data_ptr(), masks.shape[0], masks.shape[1], rules.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream, o.cls.data_ptr(), o.cls.shape[0], o.cls.shape[1], o.next.data_ptr(),
                                                o.next.numel(), o.state_row.data_ptr(), o.state_row.numel(), o.guides.data_ptr(), o.gstate.data_ptr(),
                                                close_row, n_close_row, closes_p, budget_p)
    assert rows_entry(None, 0, None, None) == 0
    assert out.cpu().tolist() == guided and t.states() == after_guided
    # closing rules without the tables they need are an argument error, not a launch
    assert rows_entry(None, 0, o.closes.data_ptr(), o.budget.data_ptr()) == -1 and b"sample_rows_closing" in lib.fo1_last_error()
    assert rows_entry(o.close_row.data_ptr(), o.close_row.numel(), o.closes.data_ptr(), None) == -1 and b"budget" in lib.fo1_last_error()
    # close_off / depth pointing past close_row, a negative close_off, a negative state: the state's plain row, i.e. the _guided entry
    n_cr = CLOSE_OFF + len(cr)
    for bad in ((n_cr, DEPTH), (n_cr - 1, 1 << 20), (-4, DEPTH), (0x7ffffff0, 0x7fffffff)):
        closes2 = [None if guides[b] is None else bad for b in range(B)]
        t = CloseTables(ops, V, sr, guides, states, cr, closes2, [ctr[b] + 1 + (left[b] if bad[1] == DEPTH else 0) for b in range(B)])
        if bad == (n_cr - 1, 1 << 20):      # state 0 with r = 0 is the table's last entry, every other state lies past it
            got2 = ops.sample_rows(dl, params, counter=counter, seen=seen, masks=masks, rules=rules, guide=t.op).cpu().tolist()
            assert [got2[b] for b in range(B) if states[b] != 0 or guides[b] is None] == [guided[b] for b in range(B) if states[b] != 0 or guides[b] is None]
        else:
            got2 = ops.sample_rows(dl, params, counter=counter, seen=seen, masks=masks, rules=rules, guide=t.op).cpu().tolist()
            assert got2 == guided, (bad, got2, guided)
            assert t.states() == after_guided
        t.assert_intact()
    # the accept form in one launch: a finished row, a row without a guide, depth = 0 and closing rows side by side
    fin = (1, 8)
    t = CloseTables(ops, V, sr, guides, states, cr, closes)
    tg = GH.Tables(ops, V, sr, guides, states)
    res = []
    for op in (t.op, tg.op):
        st = torch.tensor([[5, 5, 0, int(b in fin), ctr[b], budget[b], 0, 0] for b in range(B)], dtype=torch.int32).cuda()
        plan, ids = torch.zeros(B, 2, dtype=torch.int32, device="cuda"), torch.full((B, 16), -1, dtype=torch.int32, device="cuda")
        done = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.decode_head_accept(dl, params, st, plan, ids, None, done, seen=seen.clone(), masks=masks, rules=rules, guide=op)
        res.append(ids.cpu())
    # closes = NULL through the accept form's C entry: bitwise the _guided entry's ids and states
    tn = GH.Tables(ops, V, sr, guides, states)
    o = tn.op
    st = torch.tensor([[5, 5, 0, int(b in fin), ctr[b], budget[b], 0, 0] for b in range(B)], dtype=torch.int32).cuda()
    plan, ids = torch.zeros(B, 2, dtype=torch.int32, device="cuda"), torch.full((B, 16), -1, dtype=torch.int32, device="cuda")
    done, seen2 = torch.zeros(1, dtype=torch.int32, device="cuda"), seen.clone()
    rc = lib.fo1_decode_head_closing_accept(dl.data_ptr(), dl.stride(0), V, B, params.data_ptr(), st.data_ptr(), plan.data_ptr(), ids.data_ptr(), 16, None, 0,
                                            done.data_ptr(), ws.data_ptr(), 4096, seen2.data_ptr(), seen2.shape[1], masks.data_ptr(), masks.shape[0],
                                            masks.shape[1], rules.data_ptr(), torch.cuda.current_stream().cuda_stream, o.cls.data_ptr(), o.cls.shape[0],
                                            o.cls.shape[1], o.next.data_ptr(), o.next.numel(), o.state_row.data_ptr(), o.state_row.numel(),
                                            o.guides.data_ptr(), o.gstate.data_ptr(), None, 0, None)
    assert rc == 0 and torch.equal(ids.cpu(), res[1]) and tn.states() == tg.states()
    for b in range(B):
        if b in fin:
            assert (res[0][b] == -1).all() and t.states()[b] == states[b], b
        elif guides[b] is not None and closes[b][1] > 0 and left[b] < DEPTH:
            assert int(res[0][b, ctr[b]]) == got[b] and t.states()[b] == after[b], b      # the rows form's pick: the same counter, stream and seed
        else:
            assert int(res[0][b, ctr[b]]) == int(res[1][b, ctr[b]]) and t.states()[b] == tg.states()[b], b
    t.assert_intact()


def test_the_same_row_alone_and_at_row_37_of_64():
    from vlm_fo1_amd import ops
    V, B = 4099, 64
    bits, items, rows, guides, states, sets, sr, cr, closes, left = _mixed_closing(V, B)
    dl, seen = H._rows_buffer(items, V)
    _, masks, _ = H._framed_masks(sets, V)
    ctr = [3 + b % 5 for b in range(B)]
    counter = torch.tensor(ctr, dtype=torch.int32).cuda()
    budget = [ctr[b] + left[b] + 1 for b in range(B)]
    t = CloseTables(ops, V, sr, guides, states, cr, closes, budget)
    rules = ops.token_rules([None] * B, "cuda")
    got = ops.sample_rows(dl, ops.sample_params(rows, "cuda"), counter=counter, seen=seen, masks=masks, rules=rules, guide=t.op).cpu().tolist()
    after = t.states()
    for b in (37, 0, 5, 42, 63):
        t1 = CloseTables(ops, V, sr, [guides[b]], [states[b]], cr, [closes[b]], [budget[b]])
        one = ops.sample_rows(dl[b:b + 1], ops.sample_params(rows[b:b + 1], "cuda"), counter=counter[b:b + 1], seen=seen[b:b + 1].contiguous(), masks=masks,
                              rules=rules[:1], guide=t1.op)
        assert int(one.item()) == got[b] and t1.states() == [after[b]], (b, rows[b])
    assert guides[37] is not None and closes[37][1] == DEPTH and left[37] < DEPTH      # row 37 is a closing row behind a closing bitmap
    assert after[37] == G.head_guide(V).advance(states[37], got[37])
