"""The guided decode head on the MI355X, on bare logit rows (vlm_fo1_amd/csrc/sample.hip: the GUIDE instantiations behind
fo1_sample_rows_guided_bf16 and fo1_decode_head_guided_accept; definition, oracle and cases: tests/guide_cases.py).

  * sampled rows in each of the five states of a guide whose state bitmaps are constraint_cases' ban kinds: every exact draw returns the
    oracle's id on the masked row, every other one meets the accept rule with EPS = 2^-17 unchanged; `gstate` after the launch equals
    advance(s, id) for every row, exactly; the class, transition, state-row, guide, state and mask tables are canary-framed, and after a
    second launch the frames and everything but `gstate` hold what they held;
  * greedy rows equal the masked oracle's first index exactly, through the rows form and the accept form;
  * every other sampled (row, state) pair again through the accept form, the draw being Philox(state[b][4], b; seed);
  * a row with cls_row = -1 gives the _ruled entry's id bit for bit and leaves `gstate` untouched, and so does guides = NULL; a finished row
    leaves `gstate` untouched; offsets that point past a table give "no mask" and "the state stays";
  * the same row gives the same id and state at b = 0 of B = 1 and at b = 37 of B = 64;
  * captured in a graph with `gstate` in the rollback and replayed, the accept form gives the eager ids and states.

RESULTS_GPU (MI355X): 20 x 2 launches of the sampled cases (3 of 570 (row, state) pairs left out for their top-p margin): 3456 exact draws equal
the oracle's id, 1551 meet the accept rule, worst excursion out of the id's interval 7.9e-8 = 0.010 EPS; the state moved 3382 times and stayed
1625 times, each as advance(s, id) says.  Through the accept form with Philox draws: 270 exact draws equal the oracle's id, 15 meet the accept rule."""
import numpy as np
import pytest
import torch

import constraint_cases as C
import guide_cases as G
import penalty_cases as P
import sampling_cases as S
import test_constraint_head_gpu as H

pytestmark = pytest.mark.gpu

CANARY16 = 0x5a5a
CANARY32 = 0x5a5a5a5a
NEXT_OFF, ROW_OFF, CLS_PAD = 7, 3, 5


def _i32(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32))).cuda()


class Tables:
    """The guide tables of one launch, each inside a canary frame: cls [2, V + CLS_PAD] (row 0 a decoy of class 5 everywhere, row 1 the head
    guide's map), next (HEAD_NEXT at NEXT_OFF), state_row (`groups` runs of 5 mask rows from ROW_OFF on), guides and gstate [B]."""

    def __init__(self, ops, V: int, state_rows, guides, states):
        B = len(guides)
        cls = np.full((4, V + CLS_PAD), CANARY16, np.uint16)
        cls[1, :] = 5
        cls[2, :V] = G.head_cls(V)
        self.h_cls = cls
        self.d_cls = torch.from_numpy(cls.view(np.int16)).cuda()
        nx = np.full(NEXT_OFF + G.HEAD_NEXT.size + 8, CANARY32, np.int64)
        nx[NEXT_OFF:NEXT_OFF + G.HEAD_NEXT.size] = G.HEAD_NEXT.reshape(-1)
        self.h_next = nx.astype(np.uint32)
        self.d_next = _i32(nx)
        sr = np.full(8 + ROW_OFF + len(state_rows) + 8, CANARY32, np.int64)
        sr[8 + ROW_OFF:8 + ROW_OFF + len(state_rows)] = state_rows
        self.h_sr = sr.astype(np.uint32)
        self.d_sr = _i32(sr)
        self.n_sr = ROW_OFF + len(state_rows)
        self.h_guides = ops.token_guides(guides)
        gd = torch.full((B + 2, 4), 0x5a5a5a5a, dtype=torch.int32)
        gd[1:-1] = self.h_guides
        self.d_guides = gd.cuda()
        gs = torch.full((B + 16,), S.CANARY, dtype=torch.int32)
        gs[8:8 + B] = torch.tensor(states, dtype=torch.int32)
        self.d_gs = gs.cuda()
        self.B = B
        self.op = ops.GuideOperands(self.d_cls[1:3], self.d_next[:NEXT_OFF + G.HEAD_NEXT.size], self.d_sr[8:8 + self.n_sr], self.d_guides[1:-1],
                                    self.d_gs[8:8 + B])

    def states(self):
        return self.d_gs[8:8 + self.B].cpu().tolist()

    def assert_intact(self):
        assert (self.d_cls.cpu().numpy().view(np.uint16) == self.h_cls).all(), "the class table or its frame was written"
        assert (self.d_next.cpu().numpy().view(np.uint32) == self.h_next).all(), "the transition table or its frame was written"
        assert (self.d_sr.cpu().numpy().view(np.uint32) == self.h_sr).all(), "the state-row table or its frame was written"
        gd = self.d_guides.cpu()
        assert torch.equal(gd[1:-1], self.h_guides) and (gd[0] == 0x5a5a5a5a).all() and (gd[-1] == 0x5a5a5a5a).all(), "the guide table was written"
        gs = self.d_gs.cpu()
        assert (gs[:8] == S.CANARY).all() and (gs[8 + self.B:] == S.CANARY).all(), "the state array's frame was written"


def _guide_row(group: int):
    """fo1_token_guide_t of a row whose five state bitmaps are run `group` of the state-row table (class row 1 of the two the head is given)."""
    return (1, G.N_CLASSES, NEXT_OFF, ROW_OFF + 5 * group)


def _group_tables(rows_bits, V: int):
    """Per distinct logits row its five banned sets -> (mask sets, state_row entries): the empty state names no row (-1) for even groups and a
    live all-zero row for odd ones."""
    sets, sr = [], []
    for g, bits in enumerate(rows_bits):
        for s, kind in enumerate(G.HEAD_KINDS):
            if s == 0 and g % 2 == 0:
                sr.append(-1)
                continue
            sets.append(C.ban_set(kind, bits))
            sr.append(len(sets) - 1)
    return sets, sr


def test_guided_sampled_rows_exact_draws_equal_the_oracle_and_the_state_advances():
    from vlm_fo1_amd import ops
    cs = G.head_cases()
    left, pairs = G.left_out()
    print(f"\n{len(left)} of {pairs} (row, state) pairs left out for their top-p margin")
    n_exact = n_rule = launches = moved = stayed = 0
    worst = 0.0
    for V in G.CASE_V:
        guide = G.head_guide(V)
        pr = [(c, u) for c in cs if c["V"] == V for u in c["draws"]]
        for a in range(0, len(pr), 256):
            chunk = pr[a:a + 256]
            n = len(chunk)
            dl, seen = H._rows_buffer([(c["bits"], c["seen"]) for c, _ in chunk], V)
            names = sorted({c["row"] for c, _ in chunk})
            bits_of = {c["row"]: c["bits"] for c, _ in chunk}
            sets, sr = _group_tables([bits_of[k] for k in names], V)
            buf, masks, host = H._framed_masks(sets, V)
            t = Tables(ops, V, sr, [_guide_row(names.index(c["row"])) for c, _ in chunk], [c["state"] for c, _ in chunk])
            params = ops.sample_params([(c["T"], c["top_p"], c["top_k"], 0, b, False, 0.0) for b, (c, _) in enumerate(chunk)], "cuda")
            out = torch.full((n + 16,), S.CANARY, dtype=torch.int32, device="cuda")
            u = torch.tensor([u for _, u in chunk], dtype=torch.float32).cuda()
            rules = ops.token_rules([None] * n, "cuda")
            ops.sample_rows(dl, params, u=u, out=out[8:8 + n], seen=seen, masks=masks, rules=rules, guide=t.op)
            launches += 1
            got, after = out.cpu().numpy(), t.states()
            assert (got[:8] == S.CANARY).all() and (got[8 + n:] == S.CANARY).all(), "the id buffer's canary was overwritten"
            for b, (c, uu) in enumerate(chunk):
                o, g = c["oracle"], int(got[8 + b])
                assert S.accepts(o, uu, g), (c["name"], b, uu, g, S.pick(o, uu))
                assert o.empty or g not in c["banned"], (c["name"], b, g)
                lo, hi = S.interval(o, g) if not o.empty else (uu, uu)
                worst = max(worst, lo - uu, uu - hi)
                if S.is_exact(o, uu):
                    n_exact += 1
                    assert g == S.pick(o, uu), (c["name"], b, uu, g, S.pick(o, uu))
                else:
                    n_rule += 1
                assert after[b] == guide.advance(c["state"], g), (c["name"], b, c["state"], g, after[b])
                moved += after[b] != c["state"]
                stayed += after[b] == c["state"]
            # a second launch from the advanced states: the frames and every table but gstate hold what they held
            ops.sample_rows(dl, params, u=u, out=out[8:8 + n], seen=seen, masks=masks, rules=rules, guide=t.op)
            t.assert_intact()
            assert (buf.cpu().numpy().view(np.uint32) == host).all(), "the mask table or its frame was written"
            assert all(0 <= s < 5 for s in t.states())
    print(f"{launches} x 2 launches: {n_exact} exact draws equal the oracle, {n_rule} meet the accept rule; worst excursion out of the interval "
          f"{worst:.3g} = {worst / S.EPS:.3f} EPS; the state moved {moved} times and stayed {stayed} times")
    assert n_exact > n_rule > 0 and moved > stayed > 0


def _accept_state(counters, finished=()):
    cap = max(counters) + 8      # room for the steps a test takes
    st = torch.tensor([[5, 5, 0, int(b in finished), c, cap, 0, 0] for b, c in enumerate(counters)], dtype=torch.int32).cuda()
    B = len(counters)
    return (st, torch.zeros(B, 2, dtype=torch.int32, device="cuda"), torch.full((B, cap), -1, dtype=torch.int32, device="cuda"),
            torch.zeros(1, dtype=torch.int32, device="cuda"))


def test_greedy_rows_through_both_forms_finished_rows_and_graph_replay():
    from vlm_fo1_amd import ops
    n = 0
    for V in G.CASE_V:
        guide = G.head_guide(V)
        gs = [g for g in G.greedy_head_cases() if g["V"] == V]
        B = len(gs)
        keys = sorted({g["name"].split("|")[0] for g in gs})
        bits_of = {g["name"].split("|")[0]: g["bits"] for g in gs}
        dl, _ = H._rows_buffer([(g["bits"], []) for g in gs], V)
        sets, sr = _group_tables([bits_of[k] for k in keys], V)
        buf, masks, host = H._framed_masks(sets, V)
        guides = [_guide_row(keys.index(g["name"].split("|")[0])) for g in gs]
        states = [g["state"] for g in gs]
        want = [g["want"] for g in gs]
        params = ops.sample_params([(0.3 + b, 0.5, 7, 99, b, True, 0.0) for b in range(B)], "cuda")
        rules = ops.token_rules([None] * B, "cuda")
        t = Tables(ops, V, sr, guides, states)
        got = ops.sample_rows(dl, params, masks=masks, rules=rules, guide=t.op).cpu().tolist()
        assert got == want, [(g["name"], x, w) for g, x, w in zip(gs, got, want) if x != w]
        assert t.states() == [guide.advance(s, x) for s, x in zip(states, got)]
        t.assert_intact()
        # the accept form: row 1 and the last row finished before the step
        fin = (1, B - 1)
        ctr = [b % 4 for b in range(B)]
        t = Tables(ops, V, sr, guides, states)
        state, plan, ids, done = _accept_state(ctr, fin)
        keep = [x.clone() for x in (state, plan, ids, done, t.d_gs)]
        ops.decode_head_accept(dl, params, state, plan, ids, None, done, masks=masks, rules=rules, guide=t.op)
        rec, after = ids.cpu(), t.states()
        for b in range(B):
            if b in fin:      # a finished row: nothing recorded, its guide state untouched
                assert (rec[b] == -1).all() and after[b] == states[b]
            else:
                assert int(rec[b, ctr[b]]) == want[b] and after[b] == guide.advance(states[b], want[b]), (gs[b]["name"], b)
        for _ in range(2):
            ops.decode_head_accept(dl, params, state, plan, ids, None, done, masks=masks, rules=rules, guide=t.op)
        eager = [x.clone() for x in (state, plan, ids, done, t.d_gs)]
        t.assert_intact()
        assert (buf.cpu().numpy().view(np.uint32) == host).all()
        # captured and replayed: the eager ids and states — gstate is among what the step writes, so it is in the rollback
        g, _ = ops.capture_graph(lambda: ops.decode_head_accept(dl, params, state, plan, ids, None, done, masks=masks, rules=rules, guide=t.op),
                                 rollback=(state, plan, ids, done, t.d_gs))
        for x, x0 in zip((state, plan, ids, done, t.d_gs), keep):
            x.copy_(x0)
        for _ in range(3):
            ops.replay_graph(g)
        torch.cuda.synchronize()
        for x, e, name in zip((state, plan, ids, done, t.d_gs), eager, ("state", "plan", "ids", "done", "gstate")):
            assert torch.equal(x, e), name
        n += B
    assert n == 45


def test_sampled_cases_through_the_accept_form_with_philox_draws():
    """One chunk of the sampled cases per V through fo1_decode_head_guided_accept: the draw is Philox(state[b][4], b; seed), the id is recorded
    at the row's counter, and the state advances as through the rows form."""
    from vlm_fo1_amd import ops
    seed = 0x9d1de
    n_exact = n_rule = 0
    for V in G.CASE_V:
        guide = G.head_guide(V)
        cs = [c for c in G.head_cases() if c["V"] == V][::2][:256]      # every other (row, state) pair: all five states, many rows
        n = len(cs)
        dl, seen = H._rows_buffer([(c["bits"], c["seen"]) for c in cs], V)
        names = sorted({c["row"] for c in cs})
        bits_of = {c["row"]: c["bits"] for c in cs}
        sets, sr = _group_tables([bits_of[k] for k in names], V)
        buf, masks, host = H._framed_masks(sets, V)
        states = [c["state"] for c in cs]
        t = Tables(ops, V, sr, [_guide_row(names.index(c["row"])) for c in cs], states)
        params = ops.sample_params([(c["T"], c["top_p"], c["top_k"], seed, b, False, 0.0) for b, c in enumerate(cs)], "cuda")
        ctr = [b % 7 for b in range(n)]
        state, plan, ids, done = _accept_state(ctr)
        ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=seen, masks=masks, rules=ops.token_rules([None] * n, "cuda"), guide=t.op)
        rec, after, st = ids.cpu(), t.states(), state.cpu()
        for b, c in enumerate(cs):
            o, g, u = c["oracle"], int(rec[b, ctr[b]]), S.draw_u(ctr[b], b, seed)
            assert S.accepts(o, u, g), (c["name"], b, u, g, S.pick(o, u))
            assert o.empty or g not in c["banned"], (c["name"], b, g)
            if S.is_exact(o, u):
                n_exact += 1
                assert g == S.pick(o, u), (c["name"], b, u, g, S.pick(o, u))
            else:
                n_rule += 1
            assert after[b] == guide.advance(states[b], g) and int(st[b, 4]) == ctr[b] + 1, (c["name"], b)
        t.assert_intact()
        assert (buf.cpu().numpy().view(np.uint32) == host).all(), "the mask table or its frame was written"
    print(f"\naccept form: {n_exact} exact draws equal the oracle, {n_rule} meet the accept rule")
    assert n_exact > n_rule and n_exact + n_rule >= 250


def _mixed(V: int, B: int):
    """B rows: greedy / sampled x penalised or not x guided or not, the guided ones spread over the five states."""
    rng = np.random.default_rng(97 + V)
    bits = S.to_bits((rng.standard_normal((B, V)) * 3).astype(np.float32))
    items, rows, guides, states = [], [], [], []
    for b in range(B):
        pen, greedy, guided = bool(b & 1), bool(b & 2), b % 8 < 6
        items.append((bits[b], P.seen_set("every32", bits[b]) if pen else np.zeros(0, np.int64)))
        rows.append((0.7, 1.0, 50, 0x5eed + b // 8, b, greedy, 1.3 if pen else 0.0))
        guides.append(_guide_row(b) if guided else None)
        states.append(b % 5)
    sets, sr = _group_tables(list(bits), V)
    return bits, items, rows, guides, states, sets, sr


def test_a_row_without_a_guide_is_the_ruled_heads_and_offsets_past_a_table_are_clamped():
    from vlm_fo1_amd import lib as L, ops
    V, B = 4099, 16
    bits, items, rows, guides, states, sets, sr = _mixed(V, B)
    dl, seen = H._rows_buffer(items, V)
    _, masks, _ = H._framed_masks(sets, V)
    params = ops.sample_params(rows, "cuda")
    ctr = torch.tensor([3 + b % 5 for b in range(B)], dtype=torch.int32).cuda()
    # every row carries a rule of its own too: its always_row is overridden by the guide's state row for a guided row, and stands for the others
    rules = ops.token_rules([(sr[5 * b + 2], -1, 0, -1) for b in range(B)], "cuda")
    ruled = ops.sample_rows(dl, params, counter=ctr, seen=seen, masks=masks, rules=rules)
    t = Tables(ops, V, sr, guides, states)
    got = ops.sample_rows(dl, params, counter=ctr, seen=seen, masks=masks, rules=rules, guide=t.op).cpu().tolist()
    after = t.states()
    guide = G.head_guide(V)
    for b in range(B):
        if guides[b] is None:      # cls_row = -1: the _ruled entry's id bit for bit, gstate untouched
            assert got[b] == int(ruled[b]) and after[b] == states[b], b
        else:
            rb = C.ruled(bits[b], C.ban_set(G.HEAD_KINDS[states[b]], bits[b]), items[b][1], rows[b][6])
            if rows[b][5]:
                assert got[b] == P.greedy_pick(rb), b
            else:
                assert S.accepts(S.oracle(rb, *rows[b][:3]), S.draw_u(int(ctr[b]), rows[b][4], rows[b][3]), got[b]), b
            assert after[b] == guide.advance(states[b], got[b]), b
    assert any(got[b] != int(ruled[b]) for b in range(B) if guides[b] is not None), "the guide moved no pick"
    # no row has a guide, and guides = NULL through the C entry itself: the _ruled entry
    t = Tables(ops, V, sr, [None] * B, states)
    assert torch.equal(ops.sample_rows(dl, params, counter=ctr, seen=seen, masks=masks, rules=rules, guide=t.op), ruled) and t.states() == states
    lib = L.load()
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = lib.fo1_sample_rows_guided_bf16(dl.data_ptr(), dl.stride(0), V, B, params.data_ptr(), ctr.data_ptr(), 1, None, out.data_ptr(), ws.data_ptr(), 4096,
                                         seen.data_ptr(), seen.shape[1], masks.data_ptr(), masks.shape[0], masks.shape[1], rules.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream, None, 0, 0, None, 0, None, 0, None, None)
    assert rc == 0 and torch.equal(out, ruled)
    # guides without the tables they need are an argument error, not a launch
    rc = lib.fo1_sample_rows_guided_bf16(dl.data_ptr(), dl.stride(0), V, B, params.data_ptr(), ctr.data_ptr(), 1, None, out.data_ptr(), ws.data_ptr(), 4096,
                                         seen.data_ptr(), seen.shape[1], masks.data_ptr(), masks.shape[0], masks.shape[1], rules.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream, None, 0, 0, None, 0, None, 0, t.op.guides.data_ptr(), None)
    assert rc == -1 and b"sample_rows_guided" in lib.fo1_last_error()
    # offsets past a table: row_off at the state-row table's end = no mask (the row's own always_row does not come back), next_off at the
    # transition table's end and a negative state = the state stays
    none = ops.token_rules([None] * B, "cuda")
    plain = ops.sample_rows(dl, params, counter=ctr, seen=seen).cpu().tolist()
    n_next = NEXT_OFF + G.HEAD_NEXT.size
    for guides2, states2 in (([(1, G.N_CLASSES, NEXT_OFF, ROW_OFF + len(sr))] * B, states), ([(1, G.N_CLASSES, n_next, ROW_OFF + len(sr))] * B, states),
                             ([(1, G.N_CLASSES, NEXT_OFF, ROW_OFF)] * B, [-1 - b for b in range(B)])):
        t = Tables(ops, V, sr, guides2, states2)
        got2 = ops.sample_rows(dl, params, counter=ctr, seen=seen, masks=masks, rules=none, guide=t.op).cpu().tolist()
        assert got2 == plain
        if guides2[0][2] == NEXT_OFF and states2[0] >= 0:
            assert t.states() == [guide.advance(s, x) for s, x in zip(states2, got2)]
        else:
            assert t.states() == states2
        t.assert_intact()


def test_the_same_row_alone_and_at_row_37_of_64():
    from vlm_fo1_amd import ops
    V, B = 32773, 64
    bits, items, rows, guides, states, sets, sr = _mixed(V, B)
    dl, seen = H._rows_buffer(items, V)
    _, masks, _ = H._framed_masks(sets, V)
    ctr = torch.tensor([3 + b % 5 for b in range(B)], dtype=torch.int32).cuda()
    t = Tables(ops, V, sr, guides, states)
    rules = ops.token_rules([None] * B, "cuda")
    got = ops.sample_rows(dl, ops.sample_params(rows, "cuda"), counter=ctr, seen=seen, masks=masks, rules=rules, guide=t.op).cpu().tolist()
    after = t.states()
    for b in (37, 0, 5, 63):
        assert guides[b] is not None or b == 63
        t1 = Tables(ops, V, sr, [guides[b]], [states[b]])
        one = ops.sample_rows(dl[b:b + 1], ops.sample_params(rows[b:b + 1], "cuda"), counter=ctr[b:b + 1], seen=seen[b:b + 1].contiguous(), masks=masks,
                              rules=rules[:1], guide=t1.op)
        assert int(one.item()) == got[b] and t1.states() == [after[b]], (b, rows[b])
    assert guides[37] is not None and after[37] == G.head_guide(V).advance(states[37], got[37])
