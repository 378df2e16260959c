"""CPU checks of tests/logprob_cases.py: the fp64 oracle against torch.log_softmax + a stable descending sort, what the case rows promise, and
EPS_LP from the emulation's measured error."""
import numpy as np
import torch

import logprob_cases as C


def test_oracle_is_log_softmax_and_a_stable_descending_sort():
    """Every case row whose entries are all finite: the same ids, in the same order, values to 1e-12."""
    seen = 0
    for V in C.SIZES:
        for r in C.rows(V):
            v = torch.from_numpy(C.from_bits(r.bits))
            if not bool(torch.isfinite(v).all()):
                continue
            seen += 1
            ref = torch.log_softmax(v, dim=0)
            assert float((torch.from_numpy(r.oracle.lp) - ref).abs().max()) <= 1e-12, (V, r.name)
            order = torch.sort(v, descending=True, stable=True).indices[:C.TOP_MAX]
            n = len(order)
            assert r.oracle.top_ids[:n].tolist() == order.tolist(), (V, r.name)
            assert float((torch.from_numpy(r.oracle.top_lp[:n]) - ref[order]).abs().max()) <= 1e-12
            assert (r.oracle.top_ids[n:] == -1).all() and np.isneginf(r.oracle.top_lp[n:]).all()
    assert seen >= 5 * len(C.SIZES)


def test_rows_that_are_not_all_finite():
    """-inf / +inf / NaN entries score -inf and never enter the top-n; the finite ones are the log-softmax over the finite ones alone."""
    for V in C.SIZES:
        for r in C.rows(V):
            v = C.from_bits(r.bits)
            fin = np.isfinite(v)
            o = r.oracle
            assert np.isneginf(o.lp[~fin]).all() and np.isfinite(o.lp[fin]).all()
            k = int(min(fin.sum(), C.TOP_MAX))
            assert (o.top_ids[:k] >= 0).all() and fin[o.top_ids[:k]].all() and (o.top_ids[k:] == -1).all() and np.isneginf(o.top_lp[k:]).all()
            if fin.any():
                ref = torch.log_softmax(torch.from_numpy(v[fin]), dim=0).numpy()
                assert np.abs(o.lp[fin] - ref).max() <= 1e-12
                assert abs(np.exp(o.lp[fin]).sum() - 1.0) <= 1e-9
            for c in (V, -1, 2 ** 31 - 1):
                assert C.chosen_lp(o, c) == -np.inf


def test_what_the_cases_promise():
    for V in C.SIZES:
        by = {r.name: r for r in C.rows(V)}
        flat = by["flat"].oracle
        assert np.abs(flat.lp + np.log(V)).max() <= 1e-12 and flat.top_ids[:min(V, C.TOP_MAX)].tolist() == list(range(min(V, C.TOP_MAX)))
        assert np.isneginf(by["none_finite"].oracle.lp).all() and (by["none_finite"].oracle.top_ids == -1).all()
        assert int(np.isfinite(by["few_finite"].oracle.lp).sum()) <= 3 < 5
        if V > 1:
            dom = by["dominant"].oracle
            assert dom.top_ids[0] == V // 2 and abs(dom.top_lp[0]) < 1e-12 and np.abs(np.delete(dom.lp, V // 2) + 80.0).max() < 1e-9
        # the planted maxima are equal, on both sides of each boundary of the layout, and the order among them is the index order
        b = C.boundaries(V)
        edges = sorted(set(i for v in b.values() for i in v))
        if edges:
            want = sorted(set(i for e in edges for i in (e - 1, e)))[:C.TOP_MAX]
            assert by["ties"].oracle.top_ids[:len(want)].tolist() == want
            assert by["ties_hi"].oracle.top_ids[:min(len(edges), C.TOP_MAX)].tolist() == edges[:C.TOP_MAX] and edges[0] > 0
        if V >= 151936:
            assert all(len(v) >= 3 for v in b.values())
        ent = C.entries(V)
        assert any(e.chosen >= V for e in ent) and any(e.chosen < 0 for e in ent)
        assert any(0 <= e.chosen < V and not np.isfinite(C.from_bits(e.row.bits)[e.chosen]) for e in ent) or V == 1
        pad = C.batch_bits(V, [0, 1])
        assert pad.shape[1] > V and not np.isfinite(C.from_bits(pad[:, V:])).all()


def test_eps_from_the_emulation():
    worst = C.measure_eps()
    n = sum(len(C.entries(V)) for V in C.SIZES)
    print(f"\nemulation: worst |lp - lp_fp64| / max(1, |lp_fp64|) = {worst:.3g} over {n} entries of {len(C.SIZES)} sizes; "
          f"EPS_LP = 2^{int(np.log2(C.EPS_LP))} = {C.EPS_LP:.3g}")
    assert C.EPS_LP == C.pow2ceil(4 * worst)
    assert abs(worst - C.MEASURED) <= 0.02 * C.MEASURED
