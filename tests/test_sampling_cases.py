"""CPU checks of tests/sampling_cases.py: the Philox known answers, the fp64 oracle against HF's logits warpers, the conditions every case
must meet (on the oracle alone), EPS from the emulation's measured error, the emulation inside the accept rule, and a chi-square test of the
oracle's own Philox draws."""
import numpy as np
import pytest

import sampling_cases as S


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join("%08x" % x for x in S.philox(ctr, key)) == want
    assert S.philox_x0(0, 0, 0) == 0x6627e8d5
    assert S.draw_u(0, 0, 0) == ((0x6627e8d5 >> 8) + 0.5) / 2 ** 24 and 0 < S.draw_u(7, 3, 1 << 40) < 1


def test_keys_are_order_preserving_and_invertible():
    bits = np.arange(65536, dtype=np.uint16)
    k, v = S.key(bits), S.from_bits(bits)
    fin = np.isfinite(v)
    assert ((k >= 0) == fin).all()
    order = np.argsort(v[fin], kind="stable")
    assert (np.diff(k[fin][order]) >= 0).all() and (np.diff(k[fin][order])[np.diff(v[fin][order]) > 0] > 0).all()
    assert S.key(np.uint16(0x8000)) == S.key(np.uint16(0)) == 0x8000
    assert (S.key_value(k[fin]) == v[fin]).all()
    assert S.region(151936) == 9728 and S.region(4096) == 512 and S.region(1) == 512 and S.region(32773) == 2560
    assert S.scan_ranges(0xffff) == (1, 0, 0) and S.scan_ranges(0x8000) == (1, 1023, 31) and S.scan_ranges(0x7fff) == (0, 0, 0)
    assert all(S.scan_ranges(S.scan_key(*r)) == r for r in S.KEYEDGE) and S.key_value(S.scan_key(1, 511, 31)) == 2.0 and S.key_value(S.scan_key(0, 512, 0)) == -2.0


def test_oracle_matches_the_transformers_warpers():
    """Without ties at a cut-off the oracle's kept set is HF's and the probabilities agree to 1e-12 (tie-free rows: distinct fp64 logits)."""
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(5)
    n = 0
    for V in (1000, 4099):
        x = S.from_bits(S.to_bits(rng.standard_normal(V) * 3))
        _, first = np.unique(x, return_index=True)
        x = x[np.sort(first)]                       # tie-free
        bits = S.to_bits(x)
        for T in (0.3, 0.7, 1.0, 1.5):
            for top_p in (0.05, 0.5, 0.9, 1.0):
                for top_k in (0, 1, 50):
                    o = S.oracle(bits, T, top_p, top_k)
                    s = torch.tensor(x, dtype=torch.float64)[None]
                    s = lp.TemperatureLogitsWarper(float(np.float32(T)))(None, s)
                    if top_k:
                        s = lp.TopKLogitsWarper(top_k)(None, s)
                    if top_p < 1:
                        s = lp.TopPLogitsWarper(float(np.float32(top_p)))(None, s)
                    prob = torch.softmax(s, -1)[0].numpy()
                    assert ((prob > 0) == o.K).all(), (V, T, top_p, top_k)
                    assert np.abs(prob - o.w / o.z2).max() < 1e-12
                    n += 1
    assert n == 96


def test_case_conditions_hold_on_the_oracle():
    rows, batches = S.rows_and_batches()
    assert {r["V"] for r in rows} == {1, 63, 1000, 4099, 32773, 151936}
    assert {b["B"] for b in batches} == {1, 3, 32, 256}
    assert any(b["ld"] > b["V"] for b in batches) and any(b["ld"] % 8 for b in batches)
    ks = {(0 if r["top_k"] == 0 else 1 if r["top_k"] == 1 else 50 if r["top_k"] == 50 else "V+1" if r["top_k"] == r["V"] + 1 else "other") for r in rows}
    assert {0, 1, 50, "V+1"} <= ks
    assert {0.05, 0.9, 1.0} == {r["top_p"] for r in rows} and {0.3, 1.0, 1.5} <= {r["T"] for r in rows}
    # every (row, draw) pair sits in a batch: no case is left out
    placed = {(i, u) for b in batches for i, u in b["items"]}
    assert all((i, u) in placed for i, r in enumerate(rows) for u in r["draws"])
    exact = 0
    for r in rows:
        o = r["oracle"]
        assert not o.empty and o.K.any(), r["name"]
        assert o.margin >= S.EXACT_MARGIN * S.EPS, (r["name"], o.margin)
        exact += sum(S.is_exact(o, u) for u in r["draws"])
        name = r["name"]
        shape = name.split("-")[1]
        if shape == "dominant":
            assert o.K.sum() == 1 and o.members[0] == int(np.argmax(np.where(S.key(r["bits"]) >= 0, S.from_bits(r["bits"]), -np.inf)))
        if shape == "equal" and r["top_k"] != 1:
            assert o.K.all()
        if shape == "equal":
            assert o.K.all()                      # ties at the top-k cut-off are all kept
        if shape == "negative":
            assert o.kcut < 0x8000 and S.key(r["bits"]).max() < 0x8000
        if shape == "mixed" and r["top_p"] == 0.9:
            assert o.kcut < 0x8000 <= S.key(r["bits"]).max(), name
        if shape == "neginf":
            assert o.members[0] >= r["V"] // 3 and o.members[-1] < r["V"] - r["V"] // 3
        if shape == "nan":
            assert not o.K[::7].any() and not o.K[r["V"] // 2]
        if shape.startswith("keyedge"):      # the cut-off key is the planted one: a range's first / last key, on a wave edge of the key scan
            half, t, pos = (int(v) for v in shape.split(".")[1:])
            assert S.scan_ranges(o.kcut) == (half, t, pos) and pos in (0, S.KPT - 1) and t % 64 in (0, 63), name
            assert o.K.sum() == 32 and S.scan_ranges(o.kcut + 1) != (half, t, pos + 1), name
        if shape == "planted":
            b = S.boundaries(r["V"])
            assert all(o.K[f - 1] and o.K[f] for kind in b.values() for f in kind)
            assert all(S.is_exact(o, float(np.float32(np.mean(S.interval(o, g))))) for kind in b.values() for f in kind for g in (f - 1, f)), name
    total = sum(len(r["draws"]) for r in rows)
    print(f"\n{len(rows)} rows, {len(batches)} launches, {total} draws, {exact} exact; smallest top-p margin "
          f"{min(r['oracle'].margin for r in rows):.3g} = {min(r['oracle'].margin for r in rows) / S.EPS:.0f} EPS")
    assert exact >= total // 2
    # an all-non-finite row has id 0
    assert S.pick(S.oracle(S.to_bits(np.array([np.nan, -np.inf, np.inf])), 1.0, 0.9, 5), 0.5) == 0


def test_eps_is_four_times_the_emulations_measured_error():
    rows, _ = S.rows_and_batches()
    worst = S.measure_eps(rows)
    print(f"\nemulation: worst relative error of a partial mass {worst:.3g}; EPS = 2^{int(np.log2(S.EPS))} = {S.EPS:.3g}")
    assert S.EPS == S.pow2ceil(4 * worst)


def test_emulation_stays_inside_the_accept_rule():
    rows, _ = S.rows_and_batches()
    for r in rows:
        o, e = r["oracle"], r["emu"]
        assert (e.member[:o.V] == o.K).all(), r["name"]
        for u in r["draws"]:
            g = S.emulate_pick(e, u)
            assert S.accepts(o, u, g), (r["name"], u, g)
            if S.is_exact(o, u):
                assert g == S.pick(o, u), (r["name"], u, g)


def test_philox_draws_pass_a_chi_square_test():
    """256 streams x 64 counters drawn through the oracle at V = 64 with fixed probabilities: Pearson's statistic under the 1 - 1e-6 quantile."""
    bound = 131.37      # chi-square quantile 1 - 1e-6 at 63 degrees of freedom (scipy.stats.chi2.ppf(1 - 1e-6, 63) = 131.3697...)
    V = 64
    bits = S.to_bits(np.linspace(-2.0, 2.0, V))
    o = S.oracle(bits, 1.0, 1.0, 0)
    counts = np.zeros(V)
    for stream in range(256):
        for counter in range(64):
            counts[S.pick(o, S.draw_u(counter, stream, 0x1234567890abcdef))] += 1
    expect = o.w / o.z2 * counts.sum()
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"\nchi2 = {chi2:.1f} at {V - 1} degrees of freedom; bound {bound}")
    assert chi2 < bound
