"""Cases, fp64 oracle, layout model, fp32 emulation and tolerance of the log-probability record: logprob_rows_kernel
(vlm_fo1_amd/csrc/logprob.hip, behind fo1_logprob_rows_bf16 and fo1_decode_logprob_record).  Shared by tests/test_logprob_cases.py (CPU),
tests/test_logprob_gpu.py and tests/test_logprob_decode_gpu.py (MI355X).

Definition (oracle(); include/fo1.h).  For a bf16 row l[0..V) with F = { i : l_i finite }: m = max_F l, S = sum_F exp(l_i - m),
lp_i = (l_i - m) - log S for i in F and -inf otherwise; a row with empty F gives -inf everywhere.  The log-softmax of the RAW logits.  Top-n:
the n entries of F with the largest l, descending, equal logits (-0 = +0) by smaller vocabulary index first, padded with (id = -1, lp = -inf).
A chosen id outside [0, V), or whose logit is not finite, scores -inf.

Layout model (what the kernel's comments state, restated here).  One workgroup of NT = 1024 threads per row; thread t visits the 8-token
chunks at t * 8 + k * STRIDE, k = 0, 1, ... (STRIDE = NT * 8 = 8192) — a lane owns 8 consecutive tokens (LANE), a wave 512 (WAVE), and the
threads wrap around every STRIDE tokens: boundaries().

emulate() restates the fp32 order of S: a thread's entries in the order it visits them, a Hillis-Steele scan over the 64 lanes of a wave (lane
63 holds the wave's sum), the 16 waves in order; exp and log in fp32 (numpy's, not the device's expf / logf: the emulation measures what the
ORDER and the fp32 roundings cost, not the intrinsics).

EPS_LP bounds |lp_device - lp_fp64| / max(1, |lp_fp64|): 4 x the emulation's worst value of that ratio against the fp64 oracle over every
finite lp of every case (measure_eps()), rounded up to a power of two; the margin of 4 covers the device's exp / log differing from numpy's by
an ulp or two.

Cases (rows(V)).  V in SIZES = {1, 7, 8, 1023, 1024, 1025, 4099, 32773, 151936}; per V: N(0, 1) and N(0, 8^2) rows, a flat row (lp = -log V,
top-n = ids 0 .. n - 1), equal maxima planted on both sides of every lane / wave / thread-stride boundary inside the row ("ties", and "ties_hi":
only the upper side of each, so the winner is not index 0), -inf over a prefix and scattered, +inf / NaN (quiet and signalling) scattered (the largest finite entry's
neighbours included), 3 finite entries in a row of -inf (fewer than n), a row without a finite entry, one dominant token with the rest 80
below it.  Chosen ids: the row's top entry, a seeded random one, the last index, a non-finite entry's, V, -1 and 2^31 - 1.

RESULTS_CPU (tests/test_logprob_cases.py -s, 9 s): the emulation's worst ratio is 2.85e-7 (90 rows, 310 entries over 9 sizes), hence
EPS_LP = 2^-19 = 1.91e-6 >= 4 x 2.85e-7.  The worst sits on short rows, where |lp| ~ 1 and S ~ 3: one ulp of S there is 2.4e-7.
RESULTS_GPU: see tests/test_logprob_gpu.py."""
from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace
from typing import Dict, List

import numpy as np

from sampling_cases import from_bits, key, pow2ceil, to_bits

EPS_LP = 2.0 ** -19          # 4 x the emulation's measured worst |lp - lp_fp64| / max(1, |lp_fp64|), rounded up to a power of two (RESULTS_CPU)
MEASURED = 2.85e-7           # that worst as recorded in RESULTS_CPU (test_logprob_cases.py asserts EPS_LP == pow2ceil(4 x measure_eps()) and prints the figure)
TOP_MAX = 8
NT, NW, LANE, WAVE, STRIDE = 1024, 16, 8, 512, 8192
SIZES = (1, 7, 8, 1023, 1024, 1025, 4099, 32773, 151936)
TOPS = (0, 1, 5, 8)
OUT_OF_RANGE = (None, -1, 2 ** 31 - 1)      # None = V


def boundaries(V: int) -> Dict[str, List[int]]:
    """First token after each kind of partition boundary that lies inside the row."""
    return dict(lane=[i for i in (LANE, 3 * LANE, WAVE + 5 * LANE, STRIDE + LANE) if i < V],
                wave=[i for i in (WAVE, 2 * WAVE, 15 * WAVE, STRIDE + WAVE) if i < V],
                stride=[i for i in (STRIDE, 2 * STRIDE, 18 * STRIDE) if i < V])


# ---- fp64 oracle -------------------------------------------------------------------------------------------------------------------------
def oracle(bits: np.ndarray, n: int = TOP_MAX) -> SimpleNamespace:
    """-> lp float64 [V]; top_ids int64 [n], top_lp float64 [n]."""
    v = from_bits(bits)
    fin = key(bits) >= 0
    V = len(bits)
    lp = np.full(V, -np.inf)
    top_ids = np.full(n, -1, dtype=np.int64)
    top_lp = np.full(n, -np.inf)
    if fin.any():
        m = v[fin].max()
        lp[fin] = (v[fin] - m) - np.log(np.exp(v[fin] - m).sum())
        idx = np.nonzero(fin)[0]
        order = idx[np.lexsort((idx, -v[idx]))][:n]      # descending value (-0.0 == 0.0), then ascending index
        top_ids[:len(order)] = order
        top_lp[:len(order)] = lp[order]
    return SimpleNamespace(lp=lp, top_ids=top_ids, top_lp=top_lp)


def chosen_lp(o: SimpleNamespace, c: int) -> float:
    return float(o.lp[c]) if 0 <= c < len(o.lp) else -np.inf


# ---- fp32 emulation of the kernel's order ------------------------------------------------------------------------------------------------
def emulate(bits: np.ndarray) -> np.ndarray:
    """lp float32 [V] with the kernel's summation order (NaN where the oracle has -inf is never produced: those stay -inf)."""
    f32 = np.float32
    V = len(bits)
    with np.errstate(invalid="ignore"):
        v = (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(f32)
    fin = key(bits) >= 0
    out = np.full(V, -np.inf, dtype=f32)
    if not fin.any():
        return out
    m = v[fin].max()
    w = np.zeros(-(-V // STRIDE) * STRIDE, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        w[:V][fin] = np.exp((v[fin] - m).astype(f32)).astype(f32)
    per_thread = w.reshape(-1, NT, LANE).transpose(1, 0, 2).reshape(NT, -1)      # thread t: chunk k = tokens t * 8 + k * STRIDE ...
    s = np.zeros(NT, dtype=f32)
    for j in range(per_thread.shape[1]):
        s = (s + per_thread[:, j]).astype(f32)
    q = s.reshape(NW, 64).copy()
    o = 1
    while o < 64:                                       # Hillis-Steele, lane order
        q[:, o:] = (q[:, o:] + q[:, :-o].copy()).astype(f32)
        o *= 2
    S = f32(0)
    for wv in range(NW):
        S = f32(S + q[wv, 63])
    log_s = f32(np.log(S))
    out[fin] = ((v[fin] - m).astype(f32) - log_s).astype(f32)
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _normal(rng, V, scale):
    return to_bits(rng.standard_normal(V).astype(np.float32) * np.float32(scale))


@lru_cache(maxsize=None)
def rows(V: int) -> List[SimpleNamespace]:
    """The case rows of one size: name, bits uint16 [V], chosen ids; built once, never modified."""
    rng = np.random.default_rng(7000 + V)
    out = []

    def add(name, bits, extra=()):
        bits = np.asarray(bits, dtype=np.uint16)
        bits.setflags(write=False)
        o = oracle(bits)
        top = int(o.top_ids[0]) if o.top_ids[0] >= 0 else 0
        chosen = list(dict.fromkeys([top, int(rng.integers(0, V)), V - 1, *extra]))
        out.append(SimpleNamespace(name=name, bits=bits, chosen=chosen, oracle=o))

    add("normal1", _normal(rng, V, 1.0), extra=[V, -1, 2 ** 31 - 1])
    add("normal8", _normal(rng, V, 8.0))
    add("flat", to_bits(np.full(V, 0.5, dtype=np.float32)))
    b = boundaries(V)
    edges = sorted(set(i for v in b.values() for i in v))
    for name, pick in (("ties", lambda e: (e - 1, e)), ("ties_hi", lambda e: (e,))):
        x = rng.standard_normal(V).astype(np.float32)
        for e in edges:
            for i in pick(e):
                x[i] = 9.0
        if not edges:
            x[V - 1] = 9.0
            x[0] = 9.0 if name == "ties" else x[0]
        add(name, to_bits(x))
    x = rng.standard_normal(V).astype(np.float32)
    x[:max(1, V // 3)] = -np.inf
    x[rng.integers(0, V, size=max(1, V // 50))] = -np.inf
    add("neg_inf", to_bits(x), extra=[0])          # (V = 1: the row without a finite entry, a second time)
    x = rng.standard_normal(V).astype(np.float32)
    top = int(np.argmax(x))
    bad = [i for i in (top - 1, top + 1, 0, V - 1) if 0 <= i < V and i != top]
    for j, i in enumerate(bad):
        x[i] = np.inf if j % 2 == 0 else np.nan
    sc = rng.integers(0, V, size=max(1, V // 40))
    sc = sc[sc != top]
    x[sc[::2]] = np.nan
    x[sc[1::2]] = np.inf
    bits = to_bits(x)
    for i, sn in zip([i for i in (V // 2 + 1, V // 3) if 0 <= i < V and i != top], (0x7f81, 0xffa5)):      # signalling NaNs, either sign
        bits[i] = sn
    add("nonfinite", bits, extra=bad[:2])
    x = np.full(V, -np.inf, dtype=np.float32)
    keep = sorted(set(int(i) for i in rng.integers(0, V, size=3)))
    x[keep] = rng.standard_normal(len(keep)).astype(np.float32)
    add("few_finite", to_bits(x), extra=[keep[0], (keep[0] + 1) % V])
    x = np.full(V, np.nan, dtype=np.float32)
    x[::3] = np.inf
    x[1::3] = -np.inf
    add("none_finite", to_bits(x))
    x = np.full(V, -40.0, dtype=np.float32)
    x[V // 2] = 40.0
    add("dominant", to_bits(x), extra=[0])
    return out


@lru_cache(maxsize=None)
def entries(V: int) -> List[SimpleNamespace]:
    """(row, chosen id) pairs of one size: one logits row of a device batch each."""
    return [SimpleNamespace(row=r, name=f"{r.name}/c={c}", chosen=c) for r in rows(V) for c in r.chosen]


def padded(V: int) -> int:
    """ld_logits of the device batches: past the row's end sit NaN / huge / +inf; rows of odd sizes start at odd addresses (the scalar path)."""
    return V + (8 if V % 8 == 0 else 3)


PAD_BITS = (0x7fc0, 0x7f7f, 0x7f80)      # NaN, the largest bf16, +inf


def batch_bits(V: int, which: List[int]) -> np.ndarray:
    """uint16 [len(which), padded(V)]: entry which[i] in row i, the padding planted."""
    ld = padded(V)
    ent = entries(V)
    out = np.empty((len(which), ld), dtype=np.uint16)
    for i, e in enumerate(which):
        out[i, :V] = ent[e].row.bits
        out[i, V:] = [PAD_BITS[(i + j) % 3] for j in range(ld - V)]
    return out


def measure_eps() -> float:
    """The emulation's worst |lp - lp_fp64| / max(1, |lp_fp64|) over every finite lp of every case row."""
    worst = 0.0
    for V in SIZES:
        for r in rows(V):
            fin = np.isfinite(r.oracle.lp)
            e = emulate(r.bits)
            assert np.array_equal(np.isfinite(e), fin) and not np.isnan(e).any(), (V, r.name)
            if fin.any():
                ref = r.oracle.lp[fin]
                worst = max(worst, float(np.max(np.abs(e[fin].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref)))))
    return worst


def check_row(name, o: SimpleNamespace, c: int, n: int, lp, top_ids, top_lp, eps: float = EPS_LP) -> float:
    """One device row against the oracle: the chosen lp, the n top ids exactly, every finite value within eps, -inf where the oracle has it,
    no NaN.  -> the worst ratio seen."""
    worst = 0.0

    def close(got, ref, what):
        nonlocal worst
        got = float(got)
        assert not np.isnan(got), (name, what, "NaN")
        if np.isinf(ref):
            assert got == ref, (name, what, got, ref)
            return
        r = abs(got - ref) / max(1.0, abs(ref))
        worst = max(worst, r)
        assert r <= eps, (name, what, got, ref, r)

    close(lp, chosen_lp(o, c), f"chosen {c}")
    assert [int(t) for t in top_ids[:n]] == [int(t) for t in o.top_ids[:n]], (name, n, list(top_ids[:n]), list(o.top_ids[:n]))
    for k in range(n):
        close(top_lp[k], o.top_lp[k], f"top {k}")
    return worst
