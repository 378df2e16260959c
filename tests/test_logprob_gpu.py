"""The log-probability record on the MI355X (vlm_fo1_amd/csrc/logprob.hip; cases, oracle and EPS_LP: tests/logprob_cases.py).

  * every (case row, chosen id) of every size through fo1_logprob_rows_bf16 at B = 1, 3 and 256 and n = 0, 1, 5, 8, rows with NaN / huge / +inf
    planted past V: the top ids equal the oracle's exactly, order included; every finite value within EPS_LP; -inf where the oracle has it; no
    NaN anywhere;
  * a row's outputs are the same bits at b = 0 of B = 1 and at any row of B = 256 (row 200 among them), and the chosen lp at n = 0 has the bits
    it has at n = 8;
  * fo1_decode_logprob_record on hand-built state / ids / n_rec: only column n - 1 of the rows whose n > n_rec is written, with the bits of
    the rows form; want = -1, finished, empty and over-long rows stay byte for byte; n_rec advances for the written rows alone.

RESULTS_GPU (MI355X): see DESIGN.md section 14."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import logprob_cases as C

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=2)
def _device_entries(V: int):
    """Every entry of one size as a device batch [R, padded(V)] (bf16, padding planted) and its chosen ids int32 [R]."""
    ent = C.entries(V)
    bits = C.batch_bits(V, list(range(len(ent))))
    logits = torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    ids = torch.tensor([e.chosen for e in ent], dtype=torch.int32, device="cuda")
    return logits, ids


def _run(V: int, which, n: int):
    """The rows form on the entries `which` as one batch -> (lp, top_ids, top_lp) as numpy."""
    from vlm_fo1_amd import ops
    logits, ids = _device_entries(V)
    if which == list(range(which[0], which[0] + len(which))):
        lg, ch = logits[which[0]:which[0] + len(which)], ids[which[0]:which[0] + len(which)]
    else:
        sel = torch.tensor(which, device="cuda")
        lg, ch = logits[sel], ids[sel].contiguous()
    lp, ti, tl = ops.logprob_rows(lg[:, :V], ch, n)
    return lp.cpu().numpy(), ti.cpu().numpy(), tl.cpu().numpy()


def _groups(V: int, B: int):
    R = len(C.entries(V))
    if B == 1:
        return [[e] for e in range(R)]
    if B == 3:
        return [list(range(s, s + 3)) for s in range(0, R - 2, 3)] + [[R - 3, R - 2, R - 1]]
    return [[i % R for i in range(B)]]


@pytest.mark.parametrize("B", (1, 3, 256))
@pytest.mark.parametrize("V", C.SIZES)
def test_every_case_against_the_oracle(V, B):
    ent = C.entries(V)
    worst, rows = 0.0, 0
    for n in C.TOPS:
        for g in _groups(V, B):
            lp, ti, tl = _run(V, g, n)
            assert ti.shape == (len(g), n) and tl.shape == (len(g), n) and not np.isnan(lp).any() and not np.isnan(tl).any()
            for b, e in enumerate(g):
                worst = max(worst, C.check_row((V, B, n, b, ent[e].name), ent[e].row.oracle, ent[e].chosen, n, lp[b], ti[b], tl[b]))
                rows += 1
    print(f"\nV={V} B={B}: {rows} rows, worst |lp - lp_fp64| / max(1, |lp_fp64|) = {worst:.3g} = {worst / C.EPS_LP:.3f} EPS_LP")


@pytest.mark.parametrize("V", (8, 1025, 32773, 151936))
def test_a_rows_bits_do_not_depend_on_its_place_or_on_n(V):
    R = len(C.entries(V))
    which = [i % R for i in range(256)]
    big = _run(V, which, 8)
    big0 = _run(V, which, 0)
    assert np.array_equal(big[0].view(np.int32), big0[0].view(np.int32)), "the chosen lp at n = 0 differs from n = 8"
    for e in range(R):
        one = _run(V, [e], 8)
        for b in [b for b in range(256) if which[b] == e]:
            for got, ref in zip(big, one):
                assert np.array_equal(got[b].view(np.int32), ref[0].view(np.int32)), (V, e, b)
    assert which[200] == 200 % R


def test_the_record_form_writes_only_what_it_should():
    from vlm_fo1_amd import ops
    V, CAP, T = 1025, 16, C.TOP_MAX
    logits, _ = _device_entries(V)
    R = logits.shape[0]
    src = [0, 1, 2, 3, R - 1, 5]                          # the logits rows of the six sequences
    lg = logits[torch.tensor(src, device="cuda")][:, :V]
    #            want  n_gen  n_rec   what
    table = [(3, 5, 4),      # a step was accepted: column 4
             (-1, 5, 0),     # off
             (8, 3, 3),      # finished earlier: nothing new
             (0, 0, 0),      # an empty slot
             (8, 1, 0),      # its first recorded token: column 0
             (2, 17, 3)]     # more tokens than the ids buffer holds
    B = len(table)
    want = torch.tensor([t[0] for t in table], dtype=torch.int32, device="cuda")
    state = torch.zeros(B, 8, dtype=torch.int32)
    state[:, 4] = torch.tensor([t[1] for t in table])
    state[:, 3] = torch.tensor([0, 0, 1, 1, 0, 1])
    state = state.cuda()
    n_rec = torch.tensor([t[2] for t in table], dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V, (B, CAP), generator=g, dtype=torch.int32).cuda()
    lp = torch.full((B, CAP), 123.25, dtype=torch.float32, device="cuda")
    ti = torch.full((B, CAP, T), -777, dtype=torch.int32, device="cuda")
    tl = torch.full((B, CAP, T), 321.5, dtype=torch.float32, device="cuda")
    before = [t.clone() for t in (lp, ti, tl, state, ids, want)]
    ops.decode_logprob_record(lg, want, state, ids, n_rec, lp, ti, tl)
    torch.cuda.synchronize()
    assert n_rec.cpu().tolist() == [5, 0, 3, 0, 1, 3]
    for t, b4 in zip((state, ids, want), before[3:]):
        assert torch.equal(t, b4)
    written = {0: 4, 4: 0}
    for b in range(B):
        for col in range(CAP):
            if written.get(b) == col:
                continue
            for t, b4 in zip((lp, ti, tl), before):
                assert torch.equal(t[b, col], b4[b, col]), (b, col)
    for b, col in written.items():
        n = table[b][0]
        c = ids[b, col:col + 1].contiguous()
        rlp, rti, rtl = ops.logprob_rows(lg[b:b + 1], c, n)
        assert torch.equal(lp[b, col].view(torch.int32), rlp[0].view(torch.int32))
        assert torch.equal(ti[b, col, :n], rti[0]) and torch.equal(tl[b, col, :n].view(torch.int32), rtl[0].view(torch.int32))
        assert (ti[b, col, n:] == -1).all() and torch.isneginf(tl[b, col, n:]).all()
        o = C.entries(V)[src[b]].row.oracle
        C.check_row(("record", b), o, int(c.item()), n, lp[b, col].item(), ti[b, col].cpu().numpy(), tl[b, col].cpu().numpy())
