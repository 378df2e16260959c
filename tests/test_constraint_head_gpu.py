"""The ruled decode head on the MI355X, on bare logit rows (vlm_fo1_amd/csrc/sample.hip: the RULE instantiations behind
fo1_sample_rows_ruled_bf16 and fo1_decode_head_ruled_accept; definition, oracle and cases: tests/constraint_cases.py).

  * sampled rows with a ban (and some with a penalty too): every exact draw returns the oracle's id on mask(penalise(bits)), every other one
    meets the accept rule with EPS = 2^-17 unchanged; the row's mask rides in always_row, early_row or first_row in turn; the mask table and
    the id buffer are canary-framed;
  * greedy and phase cases match exactly, through the rows form (counter array) and the accept form (state[b][4]);
  * one mask row shared by all B rows gives the ids of B distinct equal rows; row index -1 and mask_rows + 3 both mean none; padding bits past
    V set to 1 change nothing;
  * a row alone equals the same row at another index of a batch of 32 that mixes greedy / sampled / penalised / ruled rows;
  * rules = NULL, and rules all -1, give bitwise the ids, state, plan, ids buffer and seen bitmap of the _seen_ / _head_accept entries;
  * a finished row leaves everything untouched; captured in a graph and replayed the head gives the eager ids.

RESULTS_GPU (MI355X): 27 launches of the ruled cases: 4028 exact draws equal the oracle's id, 2010 meet the accept rule, worst excursion out of
the id's interval 7.9e-8 = 0.010 EPS."""
import numpy as np
import pytest
import torch

import constraint_cases as C
import penalty_cases as P
import sampling_cases as S

pytestmark = pytest.mark.gpu

MASK_CANARY = 0x5a5a5a5a


def _dev_logits(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def _dev_words(bm: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bm).view(np.int32)).cuda()


def _ld(V: int) -> int:
    return S.LAYOUT[V][1] if V in S.LAYOUT else V


def _rows_buffer(items, V: int):
    """items [(bits, seen ids)] -> (device logits [B, V] view of a [B, ld] buffer with NaN past V, device seen bitmap [B, ld_words])."""
    logits = np.full((len(items), _ld(V)), 0x7fc0, np.uint16)
    for b, (bits, _) in enumerate(items):
        logits[b, :V] = bits
    return _dev_logits(logits)[:, :V], _dev_words(P.host_bitmap([s for _, s in items], V))


def _framed_masks(sets, V: int, pad_ones: bool = False):
    """The mask table of `sets` inside a buffer with a canary row in front and behind -> (the whole buffer, the table's view)."""
    bm = C.host_masks(sets, V, pad_ones=pad_ones)
    buf = np.full((len(sets) + 2, bm.shape[1]), MASK_CANARY, np.uint32)
    buf[1:-1] = bm
    dev = _dev_words(buf)
    return dev, dev[1:-1], buf


def _accept_run(ops, dl, params, counters, seen=None, **rule):
    """One step of the accept form with state[b][4] = counters[b] -> the accepted ids."""
    B = dl.shape[0]
    cap = max(counters) + 2
    state = torch.tensor([[5, 5, 0, 0, c, cap + 4, 0, 0] for c in counters], dtype=torch.int32).cuda()
    plan = torch.zeros(B, 2, dtype=torch.int32, device="cuda")
    ids = torch.full((B, cap), -1, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=seen, **rule)
    rec = ids.cpu()
    return [int(rec[b, c]) for b, c in enumerate(counters)]


def test_ruled_sampled_rows_exact_draws_equal_the_oracle_and_the_rest_meet_the_accept_rule():
    from vlm_fo1_amd import ops
    cs = C.cases()
    n_exact = n_rule = launches = 0
    worst = 0.0
    for V in C.CASE_V + (C.BIG_V,):
        pairs = [(c, u) for c in cs if c["V"] == V for u in c["draws"]]
        B = 16 if V == C.BIG_V else 256
        for a in range(0, len(pairs), B):
            chunk = pairs[a:a + B]
            n = len(chunk)
            dl, seen = _rows_buffer([(c["bits"], c["seen"]) for c, _ in chunk], V)
            names = sorted({c["name"] for c, _ in chunk})
            sets = {c["name"]: c["banned"] for c, _ in chunk}
            buf, masks, host = _framed_masks([sets[k] for k in names], V)
            # the row's mask in always_row, in early_row with the counter below early_until, or in first_row with counter 0 — and the other
            # two fields naming a live mask row that does not apply at this counter
            rules, ctr = [], []
            for b, (c, _) in enumerate(chunk):
                r, other = names.index(c["name"]), (names.index(c["name"]) + 1) % len(names)
                if b % 3 == 0:
                    rules.append((r, other, 4, other)), ctr.append(4 + b % 5)
                elif b % 3 == 1:
                    rules.append((-1, r, 7, other)), ctr.append(1 + b % 6)
                else:
                    rules.append((len(names) + b % 4, other, 0, r)), ctr.append(0)
            params = ops.sample_params([(c["T"], c["top_p"], c["top_k"], 0, b, False, c["p"]) for b, (c, _) in enumerate(chunk)], "cuda")
            out = torch.full((n + 16,), S.CANARY, dtype=torch.int32, device="cuda")
            ops.sample_rows(dl, params, counter=torch.tensor(ctr, dtype=torch.int32).cuda(), u=torch.tensor([u for _, u in chunk], dtype=torch.float32).cuda(),
                            out=out[8:8 + n], seen=seen, masks=masks, rules=ops.token_rules(rules, "cuda"))
            launches += 1
            got = out.cpu().numpy()
            assert (got[:8] == S.CANARY).all() and (got[8 + n:] == S.CANARY).all(), "the id buffer's canary was overwritten"
            assert (buf.cpu().numpy().view(np.uint32) == host).all(), "the mask table or its frame was written"
            for b, (c, u) in enumerate(chunk):
                o, g = c["oracle"], int(got[8 + b])
                assert S.accepts(o, u, g), (c["name"], b, u, g, S.pick(o, u))
                assert o.empty or g not in c["banned"], (c["name"], b, g)
                lo, hi = S.interval(o, g) if not o.empty else (u, u)
                worst = max(worst, lo - u, u - hi)
                if S.is_exact(o, u):
                    n_exact += 1
                    assert g == S.pick(o, u), (c["name"], b, u, g, S.pick(o, u))
                else:
                    n_rule += 1
    print(f"\n{launches} launches: {n_exact} exact draws equal the oracle, {n_rule} meet the accept rule; worst excursion out of the interval "
          f"{worst:.3g} = {worst / S.EPS:.3f} EPS")
    assert n_exact > n_rule > 0


def test_greedy_and_phase_cases_through_the_rows_form_and_the_accept_form():
    from vlm_fo1_amd import ops
    n = 0
    for V in C.CASE_V:
        gs = [g for g in C.greedy_cases() if g["V"] == V]
        ps = [p for p in C.phase_cases() if p["V"] == V]
        B = len(gs) + len(ps)
        dl, seen = _rows_buffer([(g["bits"], g["seen"]) for g in gs] + [(p["bits"], []) for p in ps], V)
        sets, rules, ctr = [], [], []
        for b, g in enumerate(gs):
            sets.append(g["banned"])
            rules.append((len(sets) - 1, -1, 0, -1))
            ctr.append(b % 4)
        for p in ps:      # three rows per case; an empty set stays a live (all-zero) mask row
            sets += [p["always"], p["early"], p["first"]]
            rules.append((len(sets) - 3, len(sets) - 2, p["until"], len(sets) - 1))
            ctr.append(p["c"])
        _, masks, _ = _framed_masks(sets, V)
        want = [g["want"] for g in gs] + [p["want"] for p in ps]
        # temperature, top_p, top_k and the Philox words are ignored by a greedy row
        params = ops.sample_params([(0.3 + b, 0.5, 7, 99, b, True, (gs[b]["p"] if b < len(gs) else 0.0)) for b in range(B)], "cuda")
        rt = ops.token_rules(rules, "cuda")
        got = ops.sample_rows(dl, params, counter=torch.tensor(ctr, dtype=torch.int32).cuda(), seen=seen, masks=masks, rules=rt).cpu().tolist()
        names = [g["name"] for g in gs] + [p["name"] for p in ps]
        assert got == want, [(k, x, w) for k, x, w in zip(names, got, want) if x != w]
        acc = _accept_run(ops, dl, params, ctr, seen=seen.clone(), masks=masks, rules=rt)
        assert acc == want, [(k, x, w) for k, x, w in zip(names, acc, want) if x != w]
        n += B
    assert n >= 60


def test_shared_row_none_indices_and_padding_bits():
    from vlm_fo1_amd import ops
    V, B = 4099, 12
    rng = np.random.default_rng(77)
    bits = S.to_bits((rng.standard_normal((B, V)) * 3).astype(np.float32))
    dl, _ = _rows_buffer([(bits[b], []) for b in range(B)], V)
    banned = C.ban_set("every8", bits[0])
    rows = [(0.7, 0.9, 50, 0x5eed, b, b % 2 == 0, 0.0) for b in range(B)]
    params = ops.sample_params(rows, "cuda")
    ctr = torch.tensor([b % 3 for b in range(B)], dtype=torch.int32).cuda()
    _, one, _ = _framed_masks([banned], V)
    _, many, _ = _framed_masks([banned] * B, V)
    shared = ops.sample_rows(dl, params, counter=ctr, masks=one, rules=ops.token_rules([(0, -1, 0, -1)] * B, "cuda")).cpu().tolist()
    own = ops.sample_rows(dl, params, counter=ctr, masks=many, rules=ops.token_rules([(b, -1, 0, -1) for b in range(B)], "cuda")).cpu().tolist()
    assert shared == own and not set(shared) & set(banned.tolist())
    for b in range(0, B, 2):
        assert shared[b] == P.greedy_pick(C.mask(bits[b], banned))
    # -1 and mask_rows + 3 both mean none: the ids of the general head without a rule
    plain = ops.sample_rows(dl, params, counter=ctr, general=True).cpu().tolist()
    for idx in (-1, 1 + 3, 2 ** 31 - 1, -2 ** 31):
        got = ops.sample_rows(dl, params, counter=ctr, masks=one, rules=ops.token_rules([(idx, idx, 9, idx)] * B, "cuda")).cpu().tolist()
        assert got == plain, idx
    assert plain != shared
    # padding bits past V set to 1 (words 128 .. 131 of a 132-word row hold tokens 4096 .. 4223)
    _, padded, host = _framed_masks([banned], V, pad_ones=True)
    assert host[1, 128] == 0xfffffffd and host[1, 131] == 0xffffffff      # 4096 and 4098 banned, every bit from 4099 on set
    assert ops.sample_rows(dl, params, counter=ctr, masks=padded, rules=ops.token_rules([(0, -1, 0, -1)] * B, "cuda")).cpu().tolist() == shared


def _mixed_rows(V: int, B: int):
    """B rows of eight kinds interleaved: greedy / sampled x penalised or not x ruled or not -> (items, parameter rows, counters, banned sets
    or None, rules over a table with one row per ruled sequence)."""
    rng = np.random.default_rng(41 + V)
    bits = S.to_bits((rng.standard_normal((B, V)) * 3).astype(np.float32))
    items, rows, sets, rules, bans = [], [], [], [], []
    for b in range(B):
        pen, greedy, rule = bool(b & 1), bool(b & 2), bool(b & 4)
        seen = P.seen_set("every32", bits[b]) if pen else np.zeros(0, np.int64)
        rows.append((0.7, 1.0, 50, 0x5eed + b // 8, b, greedy, 1.3 if pen else 0.0))
        items.append((bits[b], seen))
        if rule:
            sets.append(C.ban_set(("top50", "every8", "argmax", "tail")[(b >> 3) % 4], bits[b]))
            rules.append((len(sets) - 1, -1, 0, -1))
            bans.append(sets[-1])
        else:
            rules.append(None)
            bans.append(None)
    return items, rows, [3 + (b % 5) for b in range(B)], bans, sets, rules


def test_mixed_batch_every_row_gives_the_id_it_gives_alone_and_at_another_index():
    from vlm_fo1_amd import ops
    V, B = 32773, 32
    items, rows, counters, bans, sets, rules = _mixed_rows(V, B)
    dl, seen = _rows_buffer(items, V)
    _, masks, _ = _framed_masks(sets, V)
    ctr = torch.tensor(counters, dtype=torch.int32).cuda()
    got = ops.sample_rows(dl, ops.sample_params(rows, "cuda"), counter=ctr, seen=seen, masks=masks, rules=ops.token_rules(rules, "cuda")).cpu().tolist()
    for b in range(B):      # alone at B = 1, its mask in row 0 of a table of one (or a table it never names)
        _, m1, _ = _framed_masks([bans[b] if bans[b] is not None else sets[0]], V)
        one = ops.sample_rows(dl[b:b + 1], ops.sample_params(rows[b:b + 1], "cuda"), counter=ctr[b:b + 1], seen=seen[b:b + 1].contiguous(), masks=m1,
                              rules=ops.token_rules([(0, -1, 0, -1) if bans[b] is not None else None], "cuda"))
        assert int(one.item()) == got[b], (b, rows[b])
    rev = list(range(B))[::-1]      # at another row index: the batch reversed
    dl2, seen2 = _rows_buffer([items[b] for b in rev], V)
    got2 = ops.sample_rows(dl2, ops.sample_params([rows[b] for b in rev], "cuda"), counter=ctr[rev].contiguous(), seen=seen2, masks=masks,
                           rules=ops.token_rules([rules[b] for b in rev], "cuda")).cpu().tolist()
    assert got2 == [got[b] for b in rev]
    n_exact = 0      # and each id is the definition's
    for b, ((bits, sn), r) in enumerate(zip(items, rows)):
        rb = C.ruled(bits, bans[b] if bans[b] is not None else [], sn, r[6])
        if r[5]:
            assert got[b] == P.greedy_pick(rb), b
        else:
            o, u = S.oracle(rb, r[0], r[1], r[2]), S.draw_u(counters[b], r[4], r[3])
            assert S.accepts(o, u, got[b]), (b, u, got[b])
            if S.is_exact(o, u):
                n_exact += 1
                assert got[b] == S.pick(o, u), b
    assert n_exact >= B // 4
    unruled = ops.sample_rows(dl, ops.sample_params(rows, "cuda"), counter=ctr, seen=seen).cpu().tolist()
    assert [unruled[b] for b in range(B) if bans[b] is None] == [got[b] for b in range(B) if bans[b] is None]
    assert any(unruled[b] != got[b] for b in range(B) if bans[b] is not None), "the rules moved no pick"


def _accept_setup(V=4099, CAP=8):
    items, rows, _, bans, sets, rules = _mixed_rows(V, 8)
    #                      pos rope kv fin n_gen max
    state = torch.tensor([[10, 20, 0, 0, 1, 8, 0, 0],
                          [11, 21, 0, 0, 2, 8, 0, 0],
                          [12, 22, 0, 0, 1, 2, 0, 0],      # budget 2: this step finishes it
                          [13, 23, 0, 1, 3, 8, 0, 0],      # finished before
                          [14, 24, 0, 0, 0, 8, 0, 0],      # ruled rows from here on; this one at counter 0
                          [15, 25, 0, 1, 2, 8, 0, 0],      # finished before (a ruled row)
                          [16, 26, 0, 0, 4, 8, 0, 0],
                          [17, 27, 0, 0, 1, 8, 0, 0]], dtype=torch.int32).cuda()
    dl, seen = _rows_buffer(items, V)
    plan = torch.full((8, 2), 7, dtype=torch.int32, device="cuda")
    ids = torch.full((8, CAP), -1, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    # rows 4 .. 7 carry their set in always_row; row 4 also a first-token set, row 6 an early set that has run out (4 >= 3), row 7 a live one
    extra = [C.ban_set("top50", items[4][0]), C.ban_set("tail", items[6][0]), C.ban_set("top50", items[7][0])]
    rules = [None] * 4 + [(0, -1, 0, 4), (1, -1, 0, -1), (2, 5, 3, -1), (3, 6, 3, -1)]
    return items, rows, dl, seen, state, plan, ids, done, sets + extra, rules


def test_accept_form_bookkeeping_finished_rows_and_graph_replay():
    from vlm_fo1_amd import ops
    V = 4099
    items, rows, dl, seen, state, plan, ids, done, sets, rules = _accept_setup(V)
    buf, masks, host = _framed_masks(sets, V)
    params, rt = ops.sample_params(rows, "cuda"), ops.token_rules(rules, "cuda")
    rule = dict(masks=masks, rules=rt)
    keep = [t.clone() for t in (state, plan, ids, done, seen)]
    st0, bm0 = state.cpu(), seen.cpu().numpy().view(np.uint32).copy()
    want = ops.sample_rows(dl, params, counter=state[:, 4].contiguous(), seen=seen, **rule).cpu().tolist()
    # the definition, row by row: rows 4 .. 7 with the sets live at their counters
    live = {4: [sets[0], sets[4]], 5: [sets[1]], 6: [sets[2]], 7: [sets[3], sets[6]]}
    for b in (0, 1, 2, 4, 6, 7):
        rb = C.ruled(items[b][0], np.concatenate(live.get(b, [np.zeros(0, np.int64)])), items[b][1], rows[b][6])
        if rows[b][5]:
            assert want[b] == P.greedy_pick(rb), b
        else:
            assert S.accepts(S.oracle(rb, *rows[b][:3]), S.draw_u(int(st0[b, 4]), rows[b][4], rows[b][3]), want[b]), b
    ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=seen, **rule)
    st, pl, rec, bm1 = state.cpu(), plan.cpu(), ids.cpu(), seen.cpu().numpy().view(np.uint32)
    for b in range(8):
        if st0[b, 3]:      # a finished row: state, ids and its bitmap row untouched, plan[1] = 0
            assert torch.equal(st[b], st0[b]) and (rec[b] == -1).all() and (bm1[b] == bm0[b]).all() and pl[b].tolist() == [0, 0]
            continue
        n = int(st0[b, 4])
        assert rec[b, n] == want[b] and pl[b].tolist() == [0, want[b]]
        assert st[b, :3].tolist() == [st0[b, 0] + 1, st0[b, 1] + 1, 0] and st[b, 4] == n + 1
        exp = bm0[b].copy()
        exp[want[b] >> 5] |= np.uint32(1 << (want[b] & 31))
        assert (bm1[b] == exp).all(), b
    assert st[2, 3] == 1 and int(done.item()) == 1
    # row 4's first-token set applied at counter 0 only: the second step may pick from it again
    for _ in range(2):
        ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=seen, **rule)
    eager = [t.clone() for t in (state, plan, ids, done, seen)]
    assert (buf.cpu().numpy().view(np.uint32) == host).all() and torch.equal(rt.cpu(), ops.token_rules(rules)), "the step wrote the mask or rule table"
    # captured and replayed: the eager ids (the rollback holds what the step writes: the tables are not among it)
    g, _ = ops.capture_graph(lambda: ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=seen, **rule), rollback=(state, plan, ids, done, seen))
    for t, t0 in zip((state, plan, ids, done, seen), keep):
        t.copy_(t0)
    for _ in range(3):
        ops.replay_graph(g)
    torch.cuda.synchronize()
    for t, e, name in zip((state, plan, ids, done, seen), eager, ("state", "plan", "ids", "done", "seen")):
        assert torch.equal(t, e), name


def test_without_rules_the_ruled_entries_are_bitwise_the_general_heads():
    from vlm_fo1_amd import lib as L, ops
    V = 4099
    items, rows, dl, seen0, state0, plan0, ids0, done0, sets, _ = _accept_setup(V)
    _, masks, _ = _framed_masks(sets, V)
    params = ops.sample_params(rows, "cuda")
    none = ops.token_rules([None] * 8, "cuda")
    ctr = state0[:, 4].contiguous()
    base = ops.sample_rows(dl, params, counter=ctr, seen=seen0)
    assert torch.equal(ops.sample_rows(dl, params, counter=ctr, seen=seen0, masks=masks, rules=none), base)
    # rules = NULL / masks = NULL through the C entry itself
    lib = L.load()
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for mp, rp in ((masks.data_ptr(), None), (None, none.data_ptr()), (None, None)):
        out = torch.full((8,), -7, dtype=torch.int32, device="cuda")
        rc = lib.fo1_sample_rows_ruled_bf16(dl.data_ptr(), dl.stride(0), V, 8, params.data_ptr(), ctr.data_ptr(), 1, None, out.data_ptr(), ws.data_ptr(), 4096,
                                            seen0.data_ptr(), seen0.shape[1], mp, masks.shape[0], masks.shape[1], rp, torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and torch.equal(out, base)
    runs = []
    for form in ("general", "all -1", "NULL"):
        state, plan, ids, done, seen = (t.clone() for t in (state0, plan0, ids0, done0, seen0))
        for _ in range(3):
            if form == "NULL":
                rc = lib.fo1_decode_head_ruled_accept(dl.data_ptr(), dl.stride(0), V, 8, params.data_ptr(), state.data_ptr(), plan.data_ptr(), ids.data_ptr(),
                                                      ids.shape[1], None, 0, done.data_ptr(), ws.data_ptr(), 4096, seen.data_ptr(), seen.shape[1],
                                                      masks.data_ptr(), masks.shape[0], masks.shape[1], None, torch.cuda.current_stream().cuda_stream)
                assert rc == 0
            else:
                ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=seen, **(dict(masks=masks, rules=none) if form == "all -1" else {}))
        runs.append([t.cpu() for t in (state, plan, ids, done, seen)])
    for other in runs[1:]:
        for a, b, name in zip(runs[0], other, ("state", "plan", "ids", "done", "seen")):
            assert torch.equal(a, b), name
