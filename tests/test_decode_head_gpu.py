"""The general decode head on the MI355X, on bare logit rows (vlm_fo1_amd/csrc/sample.hip: the PEN instantiations behind
fo1_sample_rows_seen_bf16 and fo1_decode_head_accept, and fo1_seen_mark; definition, oracle and cases: tests/penalty_cases.py).

  * sampled rows with a repetition penalty: every exact draw (sampling_cases.is_exact on the penalised bits) returns the oracle's id, every
    other one meets the accept rule with EPS = 2^-17 unchanged — the partial masses are the same fixed-order fp32 sums, over transformed keys;
  * greedy rows: without a penalty the ids of ops.argmax_rows and of decode_argmax_accept on the same rows, bitwise, ties and -inf included;
    with one, greedy_pick(penalise(...));
  * a batch of 32 with greedy, sampled and penalised rows interleaved: every row's id is the id of the same row alone and at another index;
  * fo1_seen_mark against the host's bitmap; ids -200, V and V + 5 are skipped, duplicates are fine;
  * fo1_decode_head_accept: the accepted token's bit is set, a finished row leaves state, ids and its bitmap row untouched with plan[1] = 0;
    captured in a graph and replayed it gives the eager ids; ld_words not a multiple of 4 or below ceil(V / 32) is FO1_ERR_ARG;
  * the same logits and parameters through fo1_decode_sample_accept and through the new entry with seen = NULL: identical ids, state, plan.

RESULTS_GPU (MI355X): 15 launches of the penalised cases: 2233 exact draws equal the oracle's id, 946 meet the accept rule, worst excursion out of
the id's interval 1.6e-8 = 0.002 EPS."""
import numpy as np
import pytest
import torch

import penalty_cases as P
import sampling_cases as S

pytestmark = pytest.mark.gpu


def _dev_logits(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def _dev_bitmap(bm: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bm.view(np.int32)).cuda()


def _ld(V: int) -> int:
    return S.LAYOUT[V][1] if V in S.LAYOUT else V


def _rows_buffer(items, V: int):
    """items [(bits, seen ids)] -> (device logits [B, V] view of a [B, ld] buffer with NaN past V, device bitmap [B, ld_words])."""
    ld = _ld(V)
    logits = np.full((len(items), ld), 0x7fc0, np.uint16)
    for b, (bits, _) in enumerate(items):
        logits[b, :V] = bits
    return _dev_logits(logits)[:, :V], _dev_bitmap(P.host_bitmap([s for _, s in items], V))


def test_penalised_sampled_rows_exact_draws_equal_the_oracle_and_the_rest_meet_the_accept_rule():
    from vlm_fo1_amd import ops
    cs = P.cases()
    n_exact = n_rule = launches = 0
    worst = 0.0
    for V in P.CASE_V + (P.BIG_V,):
        pairs = [(c, u) for c in cs if c["V"] == V for u in c["draws"]]
        B = 16 if V == P.BIG_V else 256
        for a in range(0, len(pairs), B):
            chunk = pairs[a:a + B]
            dl, bm = _rows_buffer([(c["bits"], c["seen"]) for c, _ in chunk], V)
            params = ops.sample_params([(c["T"], c["top_p"], c["top_k"], 0, b, False, c["p"]) for b, (c, _) in enumerate(chunk)], "cuda")
            n = len(chunk)
            out = torch.full((n + 16,), S.CANARY, dtype=torch.int32, device="cuda")
            ops.sample_rows(dl, params, u=torch.tensor([u for _, u in chunk], dtype=torch.float32).cuda(), out=out[8:8 + n], seen=bm)
            launches += 1
            got = out.cpu().numpy()
            assert (got[:8] == S.CANARY).all() and (got[8 + n:] == S.CANARY).all(), "the id buffer's canary was overwritten"
            for b, (c, u) in enumerate(chunk):
                o, g = c["oracle"], int(got[8 + b])
                assert S.accepts(o, u, g), (c["name"], b, u, g, S.pick(o, u))
                lo, hi = S.interval(o, g)
                worst = max(worst, lo - u, u - hi)
                if S.is_exact(o, u):
                    n_exact += 1
                    assert g == S.pick(o, u), (c["name"], b, u, g, S.pick(o, u))
                else:
                    n_rule += 1
    print(f"\n{launches} launches: {n_exact} exact draws equal the oracle, {n_rule} meet the accept rule; worst excursion out of the interval "
          f"{worst:.3g} = {worst / S.EPS:.3f} EPS")
    assert n_exact > n_rule > 0


def test_greedy_rows_equal_argmax_rows_and_the_penalised_greedy_pick():
    from vlm_fo1_amd import ops
    gs = P.greedy_cases()
    n = 0
    for V in sorted({g["V"] for g in gs}):
        mine = [g for g in gs if g["V"] == V]
        for a in range(0, len(mine), 64):
            chunk = mine[a:a + 64]
            B = len(chunk)
            dl, bm = _rows_buffer([(g["bits"], g["seen"]) for g in chunk], V)
            # with each case's penalty: greedy_pick(penalise(...)); temperature, top_p, top_k and the Philox words are ignored
            par = ops.sample_params([(0.3 + b, 0.5, 7, 99, b, True, g["p"]) for b, g in enumerate(chunk)], "cuda")
            got = ops.sample_rows(dl, par, seen=bm).cpu().tolist()
            assert got == [g["want"] for g in chunk], [(g["name"], x, g["want"]) for g, x in zip(chunk, got) if x != g["want"]]
            # without a penalty (the bitmap given or not): the first index of the largest finite entry = argmax_rows where no entry is +inf / NaN
            par0 = ops.sample_params([(1.0, 1.0, 0, 0, b, True, 0.0) for b in range(B)], "cuda")
            plain = ops.sample_rows(dl, par0, seen=bm).cpu().tolist()
            assert plain == ops.sample_rows(dl, par0, general=True).cpu().tolist() == [P.greedy_pick(g["bits"]) for g in chunk]
            ref = ops.argmax_rows(dl).cpu().tolist()
            state = torch.tensor([[5, 5, 0, 0, 1, 8, 0, 0]] * B, dtype=torch.int32).cuda()
            plan = torch.zeros(B, 2, dtype=torch.int32, device="cuda")
            ids = torch.full((B, 8), -1, dtype=torch.int32, device="cuda")
            done = torch.zeros(1, dtype=torch.int32, device="cuda")
            ops.decode_argmax_accept(dl, None, state, plan, ids, None, done)
            acc = ids[:, 1].cpu().tolist()
            for g, x, r, q in zip(chunk, plain, ref, acc):
                v = S.from_bits(g["bits"])
                if not (np.isnan(v).any() or (v == np.inf).any()):      # (the greedy row skips +inf and NaN, argmax_rows does not)
                    assert x == r == q, (g["name"], x, r, q)
                    n += 1
    assert n >= 40


def _mixed_rows(V: int, B: int):
    """B rows of four kinds interleaved: greedy, greedy + penalty, sampled, sampled + penalty -> (bits, seen, 7-field parameter rows, counters)."""
    rng = np.random.default_rng(31 + V)
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    bits = S.to_bits(x)
    items, rows = [], []
    for b in range(B):
        kind = b % 4
        seen = P.seen_set("every32", bits[b]) if kind in (1, 3) else np.zeros(0, np.int64)
        if kind == 1:
            seen = np.concatenate([seen, [P.greedy_pick(bits[b])]])
        p = 1.3 if kind in (1, 3) else 0.0
        rows.append((0.7, 1.0, 50, 0x5eed + b // 8, b, kind < 2, p))
        items.append((bits[b], seen))
    return items, rows, [3 + (b % 5) for b in range(B)]


def test_mixed_batch_every_row_gives_the_id_it_gives_alone_and_at_another_index():
    from vlm_fo1_amd import ops
    V, B = 32773, 32
    items, rows, counters = _mixed_rows(V, B)
    dl, bm = _rows_buffer(items, V)
    ctr = torch.tensor(counters, dtype=torch.int32).cuda()
    got = ops.sample_rows(dl, ops.sample_params(rows, "cuda"), counter=ctr, seen=bm).cpu().tolist()
    assert got == ops.sample_rows(dl, ops.sample_params(rows, "cuda"), counter=ctr, seen=bm).cpu().tolist(), "two runs differ"
    # alone at B = 1
    for b in range(B):
        one = ops.sample_rows(dl[b:b + 1], ops.sample_params(rows[b:b + 1], "cuda"), counter=ctr[b:b + 1], seen=bm[b:b + 1].contiguous())
        assert int(one.item()) == got[b], (b, rows[b])
    # at another row index: the batch reversed
    rev = list(range(B))[::-1]
    dl2, bm2 = _rows_buffer([items[b] for b in rev], V)
    got2 = ops.sample_rows(dl2, ops.sample_params([rows[b] for b in rev], "cuda"), counter=ctr[rev].contiguous(), seen=bm2).cpu().tolist()
    assert got2 == [got[b] for b in rev]
    # and each id is the definition's: greedy rows exactly, sampled rows inside the accept rule
    n_exact = 0
    for b, ((bits, seen), r) in enumerate(zip(items, rows)):
        pb = P.penalise(bits, seen, r[6])
        if r[5]:
            assert got[b] == P.greedy_pick(pb), b
        else:
            o, u = S.oracle(pb, r[0], r[1], r[2]), S.draw_u(counters[b], r[4], r[3])
            assert S.accepts(o, u, got[b]), (b, u, got[b])
            if S.is_exact(o, u):
                n_exact += 1
                assert got[b] == S.pick(o, u), b
    assert n_exact >= B // 4
    assert any(got[b] != P.greedy_pick(items[b][0]) for b in range(1, B, 4)), "the penalty moved no greedy row's pick"


def test_seen_mark_equals_the_host_bitmap():
    from vlm_fo1_amd import ops
    for V in (63, 4099, 151936):
        rng = np.random.default_rng(V)
        R = 5
        lists = [rng.integers(0, V, size=n).tolist() + [-200, V, V + 5, V - 1, 0, 31, 32, 33, 0, 0] for n in (0, 1, 40, 700, 3000)]
        rows = torch.tensor([r for r, l in enumerate(lists) for _ in l], dtype=torch.int32).cuda()
        ids = torch.tensor([t for l in lists for t in l], dtype=torch.int32).cuda()
        bm = torch.zeros(R + 1, ops.seen_words(V), dtype=torch.int32, device="cuda")
        ops.seen_mark(bm, V, rows, ids)
        got = bm.cpu().numpy().view(np.uint32)
        assert (got[:R] == P.host_bitmap(lists, V)).all() and not got[R].any()
        ops.seen_mark(bm, V, rows, ids)      # marking again changes nothing
        assert (bm.cpu().numpy().view(np.uint32) == got).all()
        # mark_prompts clears the named rows first and leaves the others alone
        ops.mark_prompts(bm, V, [1, 3], [[5, 6, -200], [V - 1]])
        after = bm.cpu().numpy().view(np.uint32)
        assert (after[[1, 3]] == P.host_bitmap([[5, 6], [V - 1]], V)).all() and (after[[0, 2, 4]] == got[[0, 2, 4]]).all()
        # a negative row is skipped
        ops.seen_mark(bm, V, torch.tensor([-1, 2], dtype=torch.int32).cuda(), torch.tensor([9, 9], dtype=torch.int32).cuda())
        again = bm.cpu().numpy().view(np.uint32)
        assert (again[[0, 1, 3, 4]] == after[[0, 1, 3, 4]]).all() and again[2, 0] & (1 << 9)


def _accept_setup(V=4099, CAP=8):
    items, rows, _ = _mixed_rows(V, 8)
    #          pos rope kv fin n_gen max
    state = torch.tensor([[10, 20, 0, 0, 1, 8, 0, 0],
                          [11, 21, 0, 0, 2, 8, 0, 0],
                          [12, 22, 0, 0, 1, 2, 0, 0],      # budget 2: this step finishes it
                          [13, 23, 0, 1, 3, 8, 0, 0],      # finished before
                          [14, 24, 0, 0, 1, 8, 0, 0],
                          [15, 25, 0, 1, 2, 8, 0, 0],      # finished before (a greedy + penalty row)
                          [16, 26, 0, 0, 4, 8, 0, 0],
                          [17, 27, 0, 0, 1, 8, 0, 0]], dtype=torch.int32).cuda()
    dl, bm = _rows_buffer(items, V)
    plan = torch.full((8, 2), 7, dtype=torch.int32, device="cuda")
    ids = torch.full((8, CAP), -1, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    return items, rows, dl, bm, state, plan, ids, done


def test_decode_head_accept_bookkeeping_and_seen_update():
    from vlm_fo1_amd import ops
    V = 4099
    items, rows, dl, bm, state, plan, ids, done = _accept_setup(V)
    params = ops.sample_params(rows, "cuda")
    st0, bm0 = state.cpu(), bm.cpu().numpy().view(np.uint32).copy()
    # what the rows form gives with counter = state[b][4]
    want = ops.sample_rows(dl, params, counter=state[:, 4].contiguous(), seen=bm).cpu().tolist()
    ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=bm)
    st, pl, rec, bm1 = state.cpu(), plan.cpu(), ids.cpu(), bm.cpu().numpy().view(np.uint32)
    for b in range(8):
        if st0[b, 3]:      # a finished row: state, ids and its bitmap row untouched, plan[1] = 0
            assert torch.equal(st[b], st0[b]) and (rec[b] == -1).all() and (bm1[b] == bm0[b]).all() and pl[b].tolist() == [0, 0]
            continue
        n = int(st0[b, 4])
        assert rec[b, n] == want[b] and pl[b].tolist() == [0, want[b]]
        assert st[b, :3].tolist() == [st0[b, 0] + 1, st0[b, 1] + 1, 0] and st[b, 4] == n + 1
        exp = bm0[b].copy()
        exp[want[b] >> 5] |= np.uint32(1 << (want[b] & 31))
        assert (bm1[b] == exp).all(), b                                       # exactly the accepted token's bit was added
    assert st[2, 3] == 1 and int(done.item()) == 1                            # the budget finished row 2
    # a second step: the counters moved on, and the penalised rows now also count the token they just produced
    want2 = ops.sample_rows(dl, params, counter=state[:, 4].contiguous(), seen=bm).cpu().tolist()
    ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=bm)
    rec2 = ids.cpu()
    assert rec2[0, 2] == want2[0] and rec2[1, 3] == want2[1] and rec2[2, 2] == -1 and rec2[4, 2] == want2[4]
    assert want2[1] != want[1], "the greedy + penalty row picked the token it had just penalised"
    b = 1
    pb = P.penalise(items[b][0], np.concatenate([items[b][1], [want[b]]]), rows[b][6])
    assert want2[b] == P.greedy_pick(pb)
    # a sampled stop id finishes its row, per-sequence sets included
    stop = torch.zeros(2, 17, dtype=torch.int32)
    stop[1, 0], stop[1, 1] = 1, int(ops.sample_rows(dl, params, counter=state[:, 4].contiguous(), seen=bm)[6].item())
    state[:, 6] = torch.tensor([0, 0, 0, 0, 0, 0, 1, 0], dtype=torch.int32).cuda()
    d0 = int(done.item())
    ops.decode_head_accept(dl, params, state, plan, ids, stop.cuda(), done, seen=bm, per_sequence_sets=True)
    assert int(state[6, 3].item()) == 1 and int(done.item()) == d0 + 1 and int(state[0, 3].item()) == 0


def test_decode_head_accept_captured_in_a_graph_gives_the_eager_ids():
    from vlm_fo1_amd import ops
    items, rows, dl, bm, state, plan, ids, done = _accept_setup()
    params = ops.sample_params(rows, "cuda")
    keep = [t.clone() for t in (state, plan, ids, done, bm)]
    for _ in range(3):
        ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=bm)
    eager = [t.clone() for t in (state, plan, ids, done, bm)]
    g, _ = ops.capture_graph(lambda: ops.decode_head_accept(dl, params, state, plan, ids, None, done, seen=bm), rollback=(state, plan, ids, done, bm))
    for t, t0 in zip((state, plan, ids, done, bm), keep):
        t.copy_(t0)
    for _ in range(3):
        ops.replay_graph(g)
    torch.cuda.synchronize()
    for t, e, name in zip((state, plan, ids, done, bm), eager, ("state", "plan", "ids", "done", "seen")):
        assert torch.equal(t, e), name


def test_argument_errors():
    from vlm_fo1_amd import lib as L, ops
    lib = L.load()
    V = 4099
    logits = torch.full((4, V), 0.25, dtype=torch.bfloat16, device="cuda")
    params = ops.sample_params([(1.0, 1.0, 0, 5, b, False, 1.3) for b in range(4)], "cuda")
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    seen = torch.zeros(4, 136, dtype=torch.int32, device="cuda")
    need = -(-V // 32)      # 129 -> ld_words >= 132 (a multiple of 4)
    rows_args = lambda ldw, **k: (logits.data_ptr(), V, V, k.get("B", 4), params.data_ptr(), None, 1, None, out.data_ptr(), ws.data_ptr(), 4096,      # noqa: E731
                                  seen.data_ptr(), ldw, None)
    state = torch.tensor([[5, 5, 0, 0, 1, 8, 0, 0]] * 4, dtype=torch.int32).cuda()
    plan = torch.zeros(4, 2, dtype=torch.int32, device="cuda")
    ids = torch.zeros(4, 8, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    acc_args = lambda ldw: (logits.data_ptr(), V, V, 4, params.data_ptr(), state.data_ptr(), plan.data_ptr(), ids.data_ptr(), 8, None, 0,      # noqa: E731
                            done.data_ptr(), ws.data_ptr(), 4096, seen.data_ptr(), ldw, None)
    mark = torch.zeros(2, dtype=torch.int32, device="cuda")
    for ldw in (need, need + 1, 130, 128, 124, 0, -4):      # not a multiple of 4, or below ceil(V / 32)
        assert lib.fo1_sample_rows_seen_bf16(*rows_args(ldw)) == -1 and b"ld_words" in lib.fo1_last_error(), ldw
        assert lib.fo1_decode_head_accept(*acc_args(ldw)) == -1 and b"ld_words" in lib.fo1_last_error(), ldw
        assert lib.fo1_seen_mark(seen.data_ptr(), ldw, V, mark.data_ptr(), mark.data_ptr(), 2, None) == -1 and b"ld_words" in lib.fo1_last_error(), ldw
    assert lib.fo1_sample_rows_seen_bf16(*rows_args(132, B=257)) == -1 and b"B=257" in lib.fo1_last_error()
    assert lib.fo1_seen_mark(None, 132, V, mark.data_ptr(), mark.data_ptr(), 2, None) == -1
    torch.cuda.synchronize()
    assert not state[:, 4].ne(1).any() and not seen.any(), "a refused call touched its operands"
    assert lib.fo1_sample_rows_seen_bf16(*rows_args(132)) == 0 and lib.fo1_sample_rows_seen_bf16(*rows_args(136)) == 0


def test_old_entry_and_new_entry_without_a_bitmap_give_identical_ids_state_and_plan():
    from vlm_fo1_amd import ops
    rows, batches = S.rows_and_batches()
    bt = next(b for b in batches if b["V"] == 4099)
    logits, params, _ = S.batch_buffers(rows, bt)
    B, V = bt["B"], bt["V"]
    dl = _dev_logits(logits)[:, :V]
    par = ops.sample_params([(t, p, k, 0xabc, b) for b, (t, p, k, _, _) in enumerate(params)], "cuda")
    runs = []
    for new in (False, True):
        state = torch.tensor([[10 + b, 20 + b, 0, int(b % 7 == 3), 1 + b % 3, 8, 0, 0] for b in range(B)], dtype=torch.int32).cuda()
        plan = torch.full((B, 2), 7, dtype=torch.int32, device="cuda")
        ids = torch.full((B, 8), -1, dtype=torch.int32, device="cuda")
        done = torch.zeros(1, dtype=torch.int32, device="cuda")
        for _ in range(3):
            if new:
                ops.decode_head_accept(dl, par, state, plan, ids, None, done, seen=None)
            else:
                ops.decode_sample_accept(dl, par, state, plan, ids, None, done)
        runs.append([t.cpu() for t in (state, plan, ids, done)])
    for a, b, name in zip(runs[0], runs[1], ("state", "plan", "ids", "done")):
        assert torch.equal(a, b), name
    ctr = torch.arange(B, dtype=torch.int32, device="cuda")
    assert torch.equal(ops.sample_rows(dl, par, counter=ctr), ops.sample_rows(dl, par, counter=ctr, general=True))
