"""The steered decode head on the MI355X, on bare logit rows (vlm_fo1_amd/csrc/sample.hip: the STEER instantiations behind
fo1_sample_rows_steered_bf16 and fo1_decode_head_steered_accept; definition, oracle and cases: tests/steer_cases.py).

  * greedy cases match exactly, through the rows form and the accept form, which also counts the accepted token;
  * sampled rows: every exact draw returns the oracle's id on steer(bits), every other one meets the accept rule with EPS = 2^-17 unchanged;
    the tables and the id buffer are canary-framed;
  * a steered launch whose rows are all unsteered gives bitwise the ids (and state, plan, ids buffer, seen bitmap) of the _seen_ / _ruled /
    _closing entries, with steers all "none", with steers == NULL, and with no bias / count table at all;
  * the same row and steer give the same id at any row index of any batch layout of sampling_cases.LAYOUT;
  * padding columns [V, ld) of the logits, the bias table, the counts and the gates are never read as data;
  * a bias_row outside the table means no bias; a gate bit without an entry behind it changes nothing;
  * fo1_count_mark with duplicate pairs, out-of-range ids and negative rows equals numpy; a finished row's counts stay untouched; captured in
    a graph and replayed the accept form gives the eager ids and counts."""
import numpy as np
import pytest
import torch

import constraint_cases as C
import penalty_cases as P
import sampling_cases as S
import steer_cases as T

pytestmark = pytest.mark.gpu

CANARY16 = 0x5a5a
INF_BITS = 0x7f80


def _dev16(a: np.ndarray, dtype=torch.int16) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()
    return t.view(torch.bfloat16) if dtype == torch.bfloat16 else t


def _dev_words(bm: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bm).view(np.int32)).cuda()


def _ld(V: int) -> int:
    return S.LAYOUT[V][1] if V in S.LAYOUT else V


def _logits(rows_bits, V: int, ld: int = 0, pad: int = 0x7fc0) -> torch.Tensor:
    buf = np.full((len(rows_bits), ld or _ld(V)), pad, np.uint16)
    for b, bits in enumerate(rows_bits):
        buf[b, :V] = bits
    return _dev16(buf, torch.bfloat16)[:, :V]


def _steer_tables(ops, steers, V: int, pad: bool = False, share: bool = True):
    """steers: one dict(bias={id: value}, counts={id: n}, f, q) per row -> (SteerOperands, host frames).  Equal biases share a row of the bias
    table (share=False: a row each); the tables sit between canary rows.  pad: rows longer than V, their padding entries +inf (bias), 0xffff
    (counts) and set gate bits."""
    B = len(steers)
    keys, brow_of = [], []
    for st in steers:
        k = tuple(sorted(st["bias"].items()))
        if not k:
            brow_of.append(-1)
            continue
        if not share or k not in keys:
            keys.append(k)
            brow_of.append(len(keys) - 1)
        else:
            brow_of.append(keys.index(k))
    R = max(len(keys), 1)
    ldb = V + 5 if pad else V
    ldc = V + V % 2 + (6 if pad else 0)
    bias = np.full((R + 2, ldb), INF_BITS if pad else 0, np.uint16)
    bias[0], bias[-1] = CANARY16, CANARY16
    bias[1:-1, :V] = 0
    for r, k in enumerate(keys):
        bias[1 + r, :V] = T.bias_bits(dict(k), V)
    cnt = np.full((B + 2, ldc), 0xffff if pad else 0, np.uint16)
    cnt[0], cnt[-1] = CANARY16, CANARY16
    cnt[1:-1, :V] = 0
    for b, st in enumerate(steers):
        cnt[1 + b, :V] = T.counts_row(st["counts"], V)
    bgate = C.host_masks([np.nonzero(bias[1 + r, :V] & 0x7fff)[0] for r in range(R)], V, pad_ones=pad)
    cgate = C.host_masks([np.nonzero(cnt[1 + b, :V])[0] for b in range(B)], V, pad_ones=pad)
    dbias, dcnt = _dev16(bias, torch.bfloat16), _dev16(cnt)
    table = ops.token_steers([(r, st["f"], st["q"]) for r, st in zip(brow_of, steers)], "cuda")
    so = ops.SteerOperands(table, dbias[1:-1], _dev_words(bgate), dcnt[1:-1], _dev_words(cgate))
    return so, (dbias, bias, dcnt, cnt)


def _unwritten(frames) -> bool:
    dbias, bias, dcnt, cnt = frames
    return (dbias.view(torch.int16).cpu().numpy().view(np.uint16) == bias).all() and (dcnt.cpu().numpy().view(np.uint16) == cnt).all()


def _accept_run(ops, dl, params, counters, seen=None, **kw):
    """One step of the accept form with state[b][4] = counters[b] -> the accepted ids."""
    B = dl.shape[0]
    cap = max(counters) + 2
    state = torch.tensor([[5, 5, 0, 0, c, cap + 4, 0, 0] for c in counters], dtype=torch.int32).cuda()
    plan = torch.zeros(B, 2, dtype=torch.int32, device="cuda")
    ids = torch.full((B, cap), -1, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=seen, **kw)
    rec = ids.cpu()
    return [int(rec[b, c]) for b, c in enumerate(counters)]


def test_greedy_cases_through_the_rows_form_and_the_accept_form():
    from vlm_fo1_amd import ops
    n = 0
    for V in T.CASE_V:
        gs = [g for g in T.greedy_cases() if g["V"] == V]
        B = len(gs)
        dl = _logits([g["bits"] for g in gs], V)
        seen = _dev_words(P.host_bitmap([g["seen"] for g in gs], V))
        masks = _dev_words(C.host_masks([g["banned"] for g in gs], V))
        rules = ops.token_rules([(b, -1, 0, -1) for b in range(B)], "cuda")
        so, frames = _steer_tables(ops, gs, V)
        want = [g["want"] for g in gs]
        names = [g["name"] for g in gs]
        # temperature, top_p, top_k and the Philox words are ignored by a greedy row
        params = ops.sample_params([(0.3 + b, 0.5, 7, 99, b, True, gs[b]["p"]) for b in range(B)], "cuda")
        got = ops.sample_rows(dl, params, seen=seen, masks=masks, rules=rules, steer=so).cpu().tolist()
        assert got == want, [(k, x, w) for k, x, w in zip(names, got, want) if x != w]
        assert _unwritten(frames), "the rows form wrote a steer table"
        ctr = [b % 4 for b in range(B)]
        cnt0 = so.counts.cpu().numpy().view(np.uint16).copy()
        acc = _accept_run(ops, dl, params, ctr, seen=seen.clone(), masks=masks, rules=rules, steer=so)
        assert acc == want, [(k, x, w) for k, x, w in zip(names, acc, want) if x != w]
        cnt1 = so.counts.cpu().numpy().view(np.uint16)
        exp = cnt0.copy()
        exp[np.arange(B), want] += 1      # the accept form counted the accepted token of every row, and nothing else
        assert (cnt1 == exp).all()
        gate = so.count_gate.cpu().numpy().view(np.uint32)
        assert (gate == C.host_masks([np.nonzero(exp[b, :V])[0] for b in range(B)], V)).all()
        n += B
    assert n >= 50


def test_steered_sampled_rows_exact_draws_equal_the_oracle_and_the_rest_meet_the_accept_rule():
    from vlm_fo1_amd import ops
    cs = T.cases()
    n_exact = n_rule = launches = 0
    worst = 0.0
    for V in T.CASE_V + (T.BIG_V,):
        pairs = [(c, u) for c in cs if c["V"] == V for u in c["draws"]]
        B = 16 if V == T.BIG_V else 256
        for a in range(0, len(pairs), B):
            chunk = pairs[a:a + B]
            n = len(chunk)
            dl = _logits([c["bits"] for c, _ in chunk], V)
            seen = _dev_words(P.host_bitmap([c["seen"] for c, _ in chunk], V))
            so, frames = _steer_tables(ops, [c for c, _ in chunk], V)
            params = ops.sample_params([(c["T"], c["top_p"], c["top_k"], 0, b, False, c["p"]) for b, (c, _) in enumerate(chunk)], "cuda")
            out = torch.full((n + 16,), S.CANARY, dtype=torch.int32, device="cuda")
            ops.sample_rows(dl, params, u=torch.tensor([u for _, u in chunk], dtype=torch.float32).cuda(), out=out[8:8 + n], seen=seen, steer=so)
            launches += 1
            got = out.cpu().numpy()
            assert (got[:8] == S.CANARY).all() and (got[8 + n:] == S.CANARY).all(), "the id buffer's canary was overwritten"
            assert _unwritten(frames), "a steer table or its frame was written"
            for b, (c, u) in enumerate(chunk):
                o, g = c["oracle"], int(got[8 + b])
                assert S.accepts(o, u, g), (c["name"], b, u, g, S.pick(o, u))
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


def _mixed(V: int, B: int):
    """B rows interleaving greedy / sampled, penalised or not, biased or not, counted or not."""
    rng = np.random.default_rng(43 + V)
    bits = S.to_bits((rng.standard_normal((B, V)) * 3).astype(np.float32))
    rows, seen, steers = [], [], []
    for b in range(B):
        pen, greedy, biased, counted = bool(b & 1), bool(b & 2), bool(b & 4), bool(b & 8)
        rows.append((0.7, 1.0 if b % 3 else 0.9, 50 if b % 5 else 0, 0x5eed + b // 8, b, greedy, 1.3 if pen else 0.0))
        seen.append(P.seen_set("every32", bits[b]) if pen else np.zeros(0, np.int64))
        st = T.kind_steer("bias-every8" if biased else "bias-argmax", bits[b]) if (biased or b % 7 == 0) else dict(bias={})
        ct = T.kind_steer("counts-top50", bits[b]) if counted else dict(counts={}, f=0.0, q=0.0)
        steers.append(dict(bias=st["bias"], counts=ct["counts"], f=ct["f"], q=ct["q"]))
    return bits, rows, seen, steers, [3 + b % 5 for b in range(B)]


def test_every_row_gives_the_id_of_the_definition_alone_and_at_any_index_of_any_layout():
    from vlm_fo1_amd import ops
    for V, (_, ld) in ((v, S.LAYOUT[v]) for v in (63, 4099, 32773)):
        B = 32
        bits, rows, seen, steers, counters = _mixed(V, B)
        ctr = torch.tensor(counters, dtype=torch.int32).cuda()

        def run(order, ld=ld, share=True):
            so, _ = _steer_tables(ops, [steers[b] for b in order], V, share=share)
            return ops.sample_rows(_logits([bits[b] for b in order], V, ld), ops.sample_params([rows[b] for b in order], "cuda"),
                                   counter=ctr[order].contiguous(), seen=_dev_words(P.host_bitmap([seen[b] for b in order], V)), steer=so).cpu().tolist()

        got = run(list(range(B)))
        n_exact = moved = 0
        for b in range(B):      # the definition's id
            sb = T.steer(bits[b], steers[b]["bias"], steers[b]["counts"], steers[b]["f"], steers[b]["q"], seen=seen[b], p=rows[b][6])
            pb = P.penalise(bits[b], seen[b], rows[b][6])
            if rows[b][5]:
                assert got[b] == P.greedy_pick(sb), (V, b)
                moved += got[b] != P.greedy_pick(pb)
            else:
                o, u = S.oracle(sb, *rows[b][:3]), S.draw_u(counters[b], rows[b][4], rows[b][3])
                assert S.accepts(o, u, got[b]), (V, b, u, got[b])
                if S.is_exact(o, u):
                    n_exact += 1
                    assert got[b] == S.pick(o, u), (V, b)
        assert n_exact >= B // 4 and moved > 0
        rev = list(range(B))[::-1]
        assert run(rev) == [got[b] for b in rev]                                   # at another row index
        assert run(rev, share=False) == [got[b] for b in rev]                      # whichever row of the bias table holds its bias
        assert run(list(range(B)), ld=ld + 8 + V % 2) == got                       # another row pitch (aligned or not)
        for b in (0, 5, 14, 31):                                                   # alone, B = 1
            assert run([b]) == [got[b]], (V, b)
        half = list(range(0, B, 2))                                                # a smaller batch of other neighbours
        assert run(half) == [got[b] for b in half]


def test_padding_columns_are_never_read_as_data():
    from vlm_fo1_amd import ops
    for V in (63, 4099, 32773):
        B = 16
        bits, rows, seen, steers, counters = _mixed(V, B)
        ctr = torch.tensor(counters, dtype=torch.int32).cuda()
        params = ops.sample_params(rows, "cuda")
        sn = _dev_words(P.host_bitmap(seen, V))
        so, _ = _steer_tables(ops, steers, V)
        base = ops.sample_rows(_logits(bits, V), params, counter=ctr, seen=sn, steer=so).cpu().tolist()
        # logits padded with +inf up to the next multiple of 8 and beyond; bias padding +inf, count padding 0xffff, every gate bit past V set
        ld = (V + 7) // 8 * 8 + 8
        sp, _ = _steer_tables(ops, steers, V, pad=True)
        assert sp.bias.shape[1] > V and sp.counts.shape[1] > V
        got = ops.sample_rows(_logits(bits, V, ld, pad=INF_BITS), params, counter=ctr, seen=sn, steer=sp).cpu().tolist()
        assert got == base, V
        assert all(g < V for g in got)


def test_bias_row_outside_the_table_and_stale_gate_bits_mean_no_bias():
    from vlm_fo1_amd import ops
    V, B = 4099, 12
    bits, rows, seen, steers, counters = _mixed(V, B)
    ctr = torch.tensor(counters, dtype=torch.int32).cuda()
    params = ops.sample_params(rows, "cuda")
    dl, sn = _logits(bits, V), _dev_words(P.host_bitmap(seen, V))
    plain = ops.sample_rows(dl, params, counter=ctr, seen=sn).cpu().tolist()
    one = dict(bias={int(i): 6.0 for i in C.ban_set("every8", bits[0])}, counts={}, f=0.0, q=0.0)
    so, _ = _steer_tables(ops, [one] * B, V)
    assert so.bias.shape[0] == 1
    steered = ops.sample_rows(dl, params, counter=ctr, seen=sn, steer=so).cpu().tolist()
    assert steered != plain
    for idx in (-1, 1, 4, 2 ** 31 - 1, -2 ** 31):
        st = so._replace(steers=ops.token_steers([(idx, 0.0, 0.0)] * B, "cuda"))
        assert ops.sample_rows(dl, params, counter=ctr, seen=sn, steer=st).cpu().tolist() == plain, idx
    # every gate bit set over an all-zero bias row and all-zero counts with the penalties on: zero entries change nothing
    zero = dict(bias={}, counts={}, f=0.5, q=0.5)
    sz, _ = _steer_tables(ops, [zero] * B, V)
    full = torch.full_like(sz.bias_gate, -1)
    sz = sz._replace(steers=ops.token_steers([(0, 0.5, 0.5)] * B, "cuda"), bias_gate=full, count_gate=torch.full_like(sz.count_gate, -1))
    assert ops.sample_rows(dl, params, counter=ctr, seen=sn, steer=sz).cpu().tolist() == plain


def _accept_setup(V=4099, CAP=8):
    bits, rows, seen, steers, _ = _mixed(V, 16)
    pick = [0, 1, 2, 3, 4, 5, 12, 15]
    #                      pos rope kv fin n_gen max
    state = torch.tensor([[10, 20, 0, 0, 1, 8, 0, 0],
                          [11, 21, 0, 0, 2, 8, 0, 0],
                          [12, 22, 0, 0, 1, 2, 0, 0],      # budget 2: this step finishes it
                          [13, 23, 0, 1, 3, 8, 0, 0],      # finished before
                          [14, 24, 0, 0, 0, 8, 0, 0],      # biased rows from here on
                          [15, 25, 0, 1, 2, 8, 0, 0],      # finished before (a biased row)
                          [16, 26, 0, 0, 4, 8, 0, 0],      # biased and counted
                          [17, 27, 0, 0, 1, 8, 0, 0]], dtype=torch.int32).cuda()
    plan = torch.full((8, 2), 7, dtype=torch.int32, device="cuda")
    ids = torch.full((8, CAP), -1, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    return [bits[b] for b in pick], [rows[b] for b in pick], [seen[b] for b in pick], [steers[b] for b in pick], state, plan, ids, done


def test_unsteered_rows_are_bitwise_the_earlier_entries():
    from vlm_fo1_amd import lib as L, ops
    V = 4099
    bits, rows, seen, steers, state0, plan0, ids0, done0 = _accept_setup(V)
    B = 8
    dl, seen0 = _logits(bits, V), _dev_words(P.host_bitmap(seen, V))
    params = ops.sample_params(rows, "cuda")
    ctr = state0[:, 4].contiguous()
    so, _ = _steer_tables(ops, steers, V)
    none = so._replace(steers=ops.token_steers([None] * B, "cuda"))
    bare = ops.SteerOperands(none.steers)
    masks = _dev_words(C.host_masks([C.ban_set("top50", bits[b]) for b in range(B)], V))
    rules = ops.token_rules([(b, -1, 0, -1) if b % 2 else None for b in range(B)], "cuda")
    for kw in ({}, dict(masks=masks, rules=rules)):
        base = ops.sample_rows(dl, params, counter=ctr, seen=seen0, **kw)
        for st in (none, bare):
            assert torch.equal(ops.sample_rows(dl, params, counter=ctr, seen=seen0, steer=st, **kw), base)
        # (the control: a bias of -60 on each row's own pick moves every one of them)
        strong, _ = _steer_tables(ops, [dict(bias={int(t): -60.0}, counts={}, f=0.0, q=0.0) for t in base.cpu().tolist()], V)
        assert not (ops.sample_rows(dl, params, counter=ctr, seen=seen0, steer=strong, **kw) == base).any(), "a steer moved no pick"
    # steers == NULL through the C entry itself: the _closing entry's fall-through to the general head
    lib = L.load()
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    nul9 = (None, 0, 0, None, 0, None, 0, None, None)
    rc = lib.fo1_sample_rows_steered_bf16(dl.data_ptr(), dl.stride(0), V, B, params.data_ptr(), ctr.data_ptr(), 1, None, out.data_ptr(), ws.data_ptr(), 4096,
                                          seen0.data_ptr(), seen0.shape[1], None, 0, 0, None, torch.cuda.current_stream().cuda_stream, *nul9,
                                          None, 0, None, None, so.bias.data_ptr(), so.bias_gate.data_ptr(), so.bias.shape[0], so.bias.shape[1],
                                          so.counts.data_ptr(), so.count_gate.data_ptr(), so.counts.shape[1], so.count_gate.shape[1], None)
    assert rc == 0 and torch.equal(out, ops.sample_rows(dl, params, counter=ctr, seen=seen0))
    runs = []
    for form in ("general", "none", "bare"):
        state, plan, ids, done, sn = (t.clone() for t in (state0, plan0, ids0, done0, seen0))
        for _ in range(3):
            ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=sn, **({} if form == "general" else dict(steer=none if form == "none" else bare)))
        runs.append([t.cpu() for t in (state, plan, ids, done, sn)])
    for other in runs[1:]:
        for a, b, name in zip(runs[0], other, ("state", "plan", "ids", "done", "seen")):
            assert torch.equal(a, b), name


def test_accept_form_counts_finished_rows_and_graph_replay():
    from vlm_fo1_amd import ops
    V = 4099
    bits, rows, seen, steers, state, plan, ids, done = _accept_setup(V)
    B = 8
    dl, sn = _logits(bits, V), _dev_words(P.host_bitmap(seen, V))
    params = ops.sample_params(rows, "cuda")
    so, frames = _steer_tables(ops, steers, V)
    written = (state, plan, ids, done, sn, so.counts, so.count_gate)
    keep = [t.clone() for t in written]
    st0 = state.cpu()
    cnt = so.counts.cpu().numpy().view(np.uint16).astype(np.int64)[:, :V]
    seen_run = [np.asarray(s, np.int64) for s in seen]
    want =ops.sample_rows(dl, params, counter=state[:, 4].contiguous(), seen=sn, steer=so).cpu().tolist()
    for step in range(3):      # the host's running counts follow the device's through three steps
        live = [b for b in range(B) if not int(state[b, 3].item())]
        n_gen = state[:, 4].cpu().tolist()
        ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=sn, steer=so)
        rec = ids.cpu()
        for b in live:
            tok = int(rec[b, n_gen[b]])
            if step == 0:
                assert tok == want[b], b
            sb = T.steer(bits[b], steers[b]["bias"], cnt[b], steers[b]["f"], steers[b]["q"], seen=seen_run[b], p=rows[b][6])
            if rows[b][5]:      # the definition on the host's running counts and seen set
                assert tok == P.greedy_pick(sb), (step, b)
            else:
                assert S.accepts(S.oracle(sb, *rows[b][:3]), S.draw_u(n_gen[b], rows[b][4], rows[b][3]), tok), (step, b)
            cnt[b, tok] += 1
            seen_run[b] = np.append(seen_run[b], tok)
        got = so.counts.cpu().numpy().view(np.uint16).astype(np.int64)[:, :V]
        assert (got == cnt).all(), step
    fin = [b for b in range(B) if st0[b, 3]]
    assert fin == [3, 5] and all((ids.cpu()[b] == -1).all() for b in fin)
    assert (frames[0].view(torch.int16).cpu().numpy().view(np.uint16) == frames[1]).all(), "the step wrote the bias table"
    eager = [t.clone() for t in written]
    g, _ = ops.capture_graph(lambda: ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=sn, steer=so), rollback=written)
    for t, t0 in zip(written, keep):
        t.copy_(t0)
    for _ in range(3):
        ops.replay_graph(g)
    torch.cuda.synchronize()
    for t, e, name in zip(written, eager, ("state", "plan", "ids", "done", "seen", "counts", "count_gate")):
        assert torch.equal(t, e), name


def test_count_mark_with_duplicates_and_out_of_range_ids_equals_numpy():
    from vlm_fo1_amd import ops
    V, R = 4099, 5
    ldc = ops.count_words(V)
    rng = np.random.default_rng(5)
    n = 3000
    rows = rng.integers(-1, R, n).astype(np.int32)
    ids = rng.integers(-3, V + 3, n).astype(np.int32)
    ids[:200] = 17            # 200 marks of one id, spread over the rows,
    rows[:120] = 2            # 120 of them in one row (one 32-bit word takes them all)
    ids[200:260] = V - 1      # the last id (the high half of the row's last used word)
    ids[260:300] = V          # just outside
    buf = torch.full((R + 2, ldc), CANARY16, dtype=torch.int16, device="cuda")
    buf[1:-1].zero_()
    gbuf = torch.full((R + 2, ops.seen_words(V)), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    gbuf[1:-1].zero_()
    ops.count_mark(buf[1:-1], gbuf[1:-1], V, torch.from_numpy(rows).cuda(), torch.from_numpy(ids).cuda())
    want = np.zeros((R, ldc), np.int64)
    ok = (rows >= 0) & (ids >= 0) & (ids < V)
    np.add.at(want, (rows[ok], ids[ok]), 1)
    got = buf.cpu().numpy().view(np.uint16)
    assert (got[1:-1] == want).all() and (got[0] == CANARY16).all() and (got[-1] == CANARY16).all()
    assert want[2, 17] >= 120 and (~ok).sum() > 100
    gate = gbuf.cpu().numpy().view(np.uint32)
    assert (gate[1:-1] == C.host_masks([np.nonzero(want[r, :V])[0] for r in range(R)], V)).all()
    assert (gate[0] == 0x5a5a5a5a).all() and (gate[-1] == 0x5a5a5a5a).all()
    assert torch.equal(ops.gate_of(buf[1:-1], V), gbuf[1:-1])      # the torch helper builds the same gate
