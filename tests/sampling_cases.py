"""Cases, fp64 oracle, Philox, partition model, fp32 emulation and tolerance of the device sampler: sample_rows_kernel
(vlm_fo1_amd/csrc/sample.hip, behind fo1_sample_rows_bf16 and fo1_decode_sample_accept).  Shared by tests/test_sampling_cases.py (CPU) and
tests/test_sampling_gpu.py (MI355X).

Definition (oracle()).  For a bf16 row l[0..V), T > 0, top_p in (0, 1], top_k >= 0: m = the largest finite l_i, w_i = exp((l_i - m) / T), a
non-finite entry has weight 0 and is never kept, a row without a finite entry gives id 0;
K1 = { i : top_k == 0 or #{ j : l_j > l_i } < top_k }, Z1 = sum_K1 w; K = { i in K1 : top_p >= 1 or sum_{j in K1, l_j > l_i} w_j < top_p Z1 };
the pick for a draw u is the smallest i in K, in vocabulary order, with sum_{j in K, j <= i} w_j > u Z2 (Z2 = sum_K w), else the last index of
K.  Tokens tied at a cut-off are all kept (-0 = +0).  A temperature that is not a positive finite number, or whose fp32 reciprocal is not finite,
means top_k = 1 at T = 1.  Without
ties this is HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax (tests/test_sampling_cases.py compares).
u = ((x0 >> 8) + 0.5) 2^-24, x0 = word 0 of Philox4x32-10 (philox()), ctr = {counter, stream, 0, 0}, key = {seed_lo, seed_hi}.

Partition model (what the kernel's comments state, restated here).  Keys: key() maps bf16 bits to 0..65535 in value order; the key scan gives
thread t of 1024 the 32 keys 32767 - 32 t .. 32736 - 32 t of a sign half (upper half first) — scan_ranges().  Pick: region(V) tokens per wave
(ceil(V / 16) rounded up to whole slices of 512), wave w owns [w region, (w + 1) region), a slice is 64 lanes x 8 tokens — boundaries().

emulate() restates the fp32 order: mass of a key = fp32(count) x exp(fp32((value - m) x fp32(1 / T))), 32 keys of a thread in descending order,
Hillis-Steele scan over the 64 threads of a wave, the waves (and the upper half's total) added in order; pick prefix of token i =
before_wave + (before_slice + (before_lane + within_lane)), each a running fp32 sum in vocabulary order with the same lane scan; the comparison
against u Z2 in fp64.  It is not bit-exact with the device (numpy's exp is not the device's expf): it measures what the ORDER costs.

EPS is a relative tolerance on a partial mass: 4 x the emulation's worst relative error of any prefix mass or above-cut-off mass against the
fp64 oracle over all cases (measure_eps()), rounded up to a power of two — the project's convention for ACC.  Accept rule for a draw u and a
returned id g: g in K and u in [c_{g-1} - EPS, c_g + EPS], c the oracle's normalised prefix.  A draw is "exact" when u lies at least 16 EPS
from both ends of the oracle pick's interval; the device must then return the oracle's id.  Every case's top-p cut-off keeps 16 EPS between
the mass above each key and top_p Z1 (asserted on the oracle alone), so K itself is never in doubt.

Cases (batches()).  V in {1, 63, 1000, 4099, 32773, 151936}; B in {1, 3, 32, 256}; ld = V (4099: rows at odd addresses, the scalar path),
V + 24 (1000), V + 3 (32773), V + 8 (151936, B = 32) with NaN past V; row shapes: dominant token, two near-equal leaders, all equal, all
negative, mixed sign with the cut-off in the negative half, -inf over a prefix and a suffix, scattered NaN, N(0, 3) at T 0.3 / 1 / 1.5, a
planted row whose heavy tokens sit on both sides of the lane (8), slice (512) and wave-region boundaries, "keyedge" rows (V = 4099, 32773)
whose top-k and top-p cut-off keys are the first / last key of a thread's range of the key scan and sit on a wave edge of it, in either sign
half (KEYEDGE); top_k in {0, 1, 3, 50, V + 1};
top_p in {0.05, 0.9, 1.0}; draws: 2^-25, fp32(1 - 2^-25) = 1, mid-interval of the first / last kept token, of a kept token just after a run
of excluded ones, of the tokens on each side of every partition boundary, and filler draws from a fixed generator.

RESULTS_CPU (tests/test_sampling_cases.py -s, 2 s): the emulation's worst relative error of a partial mass is 1.68e-6, hence EPS = 2^-17 =
7.6e-6 >= 4 x 1.68e-6 (170 rows, 1591 draws of which 1107 exact; the smallest top-p margin of a case is 1.03e-3 = 135 EPS; the emulation's
pick equals the oracle's on every exact draw and satisfies the accept rule on every other).  The order of 2^-14 was expected from an exp
argument rounded in fp32 at |argument| ~ 100; the cases' kept mass sits at |argument| < 25, where that term is ~1e-6, and the ~30 additions
behind a prefix add a few 1e-7.
RESULTS_GPU: see tests/test_sampling_gpu.py."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List

import numpy as np

EPS = 2.0 ** -17             # 4 x the emulation's measured worst relative error of a partial mass, rounded up to a power of two (RESULTS_CPU)
MEASURED = 1.68e-6           # that worst as recorded in RESULTS_CPU (test_sampling_cases.py asserts EPS == pow2ceil(4 x measure_eps()) and prints the figure)
EXACT_MARGIN = 16
NT, NW, HALF, KPT, SLICE, LANE = 1024, 16, 32768, 32, 512, 8
CANARY = -1234567


# ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------------------------
def philox(ctr, key):
    c, k = [int(x) for x in ctr], [int(x) for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return c


def philox_x0(counter: int, stream: int, seed: int) -> int:
    return philox((counter & 0xffffffff, stream & 0xffffffff, 0, 0), (seed & 0xffffffff, (seed >> 32) & 0xffffffff))[0]


def draw_u(counter: int, stream: int, seed: int) -> float:
    return ((philox_x0(counter, stream, seed) >> 8) + 0.5) * 2.0 ** -24


# ---- bf16 bits, keys ---------------------------------------------------------------------------------------------------------------------
def to_bits(x) -> np.ndarray:
    """float -> bf16 bits (round to nearest even; NaN / inf kept)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    r = np.where(nan, 0x7fc0, r)
    return r.astype(np.uint16)


def from_bits(b) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def key(b) -> np.ndarray:
    """bf16 bits -> order-preserving key 0..65535, -1 for inf / NaN (sp_key)."""
    b = np.asarray(b, dtype=np.uint16).astype(np.int64)
    b = np.where(b == 0x8000, 0, b)
    k = np.where(b & 0x8000, b ^ 0xffff, b | 0x8000)
    return np.where((b & 0x7f80) == 0x7f80, -1, k)


def key_value(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.int64)
    b = np.where(k >= 0x8000, k & 0x7fff, k ^ 0xffff)
    return from_bits(b.astype(np.uint16))


def effective(T, top_p, top_k):
    """The parameters the kernel acts on: (T, top_p or None, top_k)."""
    T = float(np.float32(T))
    top_k = max(int(top_k), 0)
    with np.errstate(over="ignore", divide="ignore"):
        usable = T > 0.0 and np.isfinite(T) and np.isfinite(np.float32(1.0) / np.float32(T))      # (a denormal T: fp32 1 / T overflows)
    if not usable:
        T, top_k = 1.0, 1
    p = float(np.float32(top_p))
    return T, (p if 0.0 < p < 1.0 else None), top_k


# ---- partition model ---------------------------------------------------------------------------------------------------------------------
def region(V: int) -> int:
    return -(-(-(-V // NW)) // SLICE) * SLICE


def boundaries(V: int) -> Dict[str, List[int]]:
    """First token after each kind of partition boundary that lies inside the row."""
    rg = region(V)
    return dict(lane=[i for i in (LANE, 3 * LANE, SLICE + 5 * LANE) if i < V],
                slice=[i for i in (SLICE, 2 * SLICE, rg + SLICE) if i < V],
                wave=[w * rg for w in range(1, NW) if w * rg < V])


def scan_ranges(k: int):
    """Key k (0..65535) -> (half: 1 upper, 0 negative; thread; position 0..31 from the top of the thread's range)."""
    half, local = (1, k - 0x8000) if k >= 0x8000 else (0, k)
    p = HALF - 1 - local
    return half, p // KPT, p % KPT


# ---- fp64 oracle -------------------------------------------------------------------------------------------------------------------------
def oracle(bits: np.ndarray, T, top_p, top_k) -> SimpleNamespace:
    T, p, top_k = effective(T, top_p, top_k)
    k = key(bits)
    fin = k >= 0
    V = len(bits)
    if not fin.any():
        return SimpleNamespace(empty=True, V=V, K=np.zeros(V, bool), margin=np.inf)
    cnt = np.bincount(k[fin], minlength=65536).astype(np.int64)
    ks = np.nonzero(cnt)[0][::-1]                       # distinct keys, descending
    vals = key_value(ks)
    m = vals[0]
    wk = np.exp((vals - m) / T)
    mass = cnt[ks] * wk
    n_above = np.concatenate([[0], np.cumsum(cnt[ks])[:-1]])
    in1 = np.ones(len(ks), bool) if top_k == 0 else n_above < top_k
    z1 = mass[in1].sum()
    m_above = np.concatenate([[0.0], np.cumsum(mass[in1])[:-1]])
    keep1 = ks[in1]
    if p is None:
        inp = np.ones(len(keep1), bool)
        margin = np.inf
    else:
        inp = m_above < p * z1
        margin = float(np.min(np.abs(m_above - p * z1)) / z1)
    kcut = int(keep1[inp].min())
    K = fin & (k >= kcut)
    wtab = np.zeros(65536)
    wtab[ks] = wk
    w = np.where(K, wtab[np.where(fin, k, 0)], 0.0)
    prefix = np.cumsum(w)
    above = dict(zip(keep1.tolist(), m_above.tolist()))
    return SimpleNamespace(empty=False, V=V, K=K, kcut=kcut, w=w, prefix=prefix, z2=float(prefix[-1]), z1=float(z1), margin=margin, m=m, T=T,
                           above=above, members=np.nonzero(K)[0])


def pick(o: SimpleNamespace, u: float) -> int:
    if o.empty:
        return 0
    hit = np.nonzero(o.K & (o.prefix > u * o.z2))[0]
    return int(hit[0]) if len(hit) else int(o.members[-1])


def interval(o: SimpleNamespace, g: int):
    return (o.prefix[g] - o.w[g]) / o.z2, o.prefix[g] / o.z2


def is_exact(o: SimpleNamespace, u: float) -> bool:
    if o.empty:
        return True
    lo, hi = interval(o, pick(o, u))
    return u - lo >= EXACT_MARGIN * EPS and hi - u >= EXACT_MARGIN * EPS


def accepts(o: SimpleNamespace, u: float, g: int, eps: float = EPS) -> bool:
    if o.empty:
        return g == 0
    if not (0 <= g < o.V and o.K[g]):
        return False
    lo, hi = interval(o, g)
    return lo - eps <= u <= hi + eps


# ---- fp32 emulation of the kernel's order ------------------------------------------------------------------------------------------------
f32 = np.float32


def _lane_scan(v: np.ndarray) -> np.ndarray:
    """Hillis-Steele inclusive scan over the last axis (64 lanes), fp32."""
    v = v.astype(f32).copy()
    o = 1
    while o < 64:
        t = v.copy()
        v[..., o:] = t[..., o:] + t[..., :-o]
        o <<= 1
    return v


def emulate(bits: np.ndarray, T, top_p, top_k) -> SimpleNamespace:
    T, p, top_k = effective(T, top_p, top_k)
    V = len(bits)
    k = key(bits)
    fin = k >= 0
    if not fin.any():
        return SimpleNamespace(empty=True)
    m = f32(key_value(k.max()))
    inv_t = f32(1.0) / f32(T)
    allk = np.arange(65536)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        wtab = np.exp(((key_value(allk).astype(f32) - m) * inv_t).astype(f32)).astype(f32)
    wtab[(allk < 0x0080) | (allk > 0xff7f)] = 0      # (keys no finite bf16 maps to)
    cnt = np.bincount(k[fin], minlength=65536).astype(np.int64)
    above: Dict[int, float] = {}
    kcut = 0
    if top_k > 0 or p is not None:
        summ = np.zeros(2 * NT + 1, f32)
        carry_c, carry_m = 0, f32(0)
        kcut_k, z1 = -1, None
        seq = {}
        for half, key0 in ((1, 0x8000), (0, 0)):
            keys = key0 + (HALF - 1 - np.arange(HALF)).reshape(NT, KPT)           # [thread, position], descending
            c = cnt[keys]
            with np.errstate(invalid="ignore", over="ignore"):
                mk = np.where(c > 0, c.astype(f32) * wtab[keys], 0).astype(f32)     # (the kernel skips empty keys: no 0 x inf above the maximum)
            part = np.zeros((NT, KPT + 1), f32)                                     # sequential partial sums inside a thread
            for j in range(KPT):
                part[:, j + 1] = part[:, j] + mk[:, j]
            mass = part[:, KPT]
            im = _lane_scan(mass.reshape(NW, 64))
            pm = np.concatenate([np.zeros((NW, 1), f32), im[:, :-1]], 1)
            ic = np.cumsum(c.sum(1))
            ex_c = carry_c + ic - c.sum(1)
            om = np.zeros(NW, f32)
            acc = f32(carry_m)
            for w in range(NW):
                om[w] = acc
                acc = f32(acc + im[w, 63])
            ex_m = (om[:, None] + pm).astype(f32).reshape(NT)
            r0 = 0 if half else NT
            summ[r0:r0 + NT] = ex_m
            run = ex_m[:, None].repeat(KPT + 1, 1).astype(f32)                      # mass above key (thread, position) as the crossing walk forms it
            for j in range(KPT):
                run[:, j + 1] = run[:, j] + mk[:, j]
            seq[half] = (keys, c, run)
            if top_k > 0 and kcut_k < 0:
                t = np.nonzero((ex_c < top_k) & (ex_c + c.sum(1) >= top_k))[0]
                if len(t):
                    t = int(t[0])
                    n = int(ex_c[t])
                    for j in range(KPT):
                        if c[t, j]:
                            n += int(c[t, j])
                            if n >= top_k:
                                kcut_k, z1 = int(keys[t, j]), run[t, j + 1]
                                break
            carry_c, carry_m = int(carry_c + c.sum()), acc
            if kcut_k >= 0:
                if half:
                    summ[NT:2 * NT] = carry_m
                break
        summ[2 * NT] = carry_m
        if kcut_k < 0:
            z1 = carry_m
        kcut_k = max(kcut_k, 0)
        for half, (keys, c, run) in seq.items():
            sel = (c > 0) & (keys >= kcut_k)
            above.update(zip(keys[sel].tolist(), run[:, :KPT][sel].tolist()))
        kcut_p = 0
        if p is not None:
            thr = f32(f32(p) * f32(z1))
            r = np.nonzero((summ[1:] >= thr) & ~(summ[:-1] >= thr))[0]
            if len(r):
                r = int(r[0])
                half, t = (1, r) if r < NT else (0, r - NT)
                keys, c, _ = seq[half]
                M = summ[r]
                kcut_p = int(keys[t, KPT - 1])
                for j in range(KPT):
                    if not c[t, j]:
                        continue
                    if not M < thr:
                        break
                    kcut_p = int(keys[t, j])
                    M = f32(M + f32(f32(c[t, j]) * wtab[keys[t, j]]))
        kcut = max(kcut_k, kcut_p)
    # the pick's prefix sums
    rg = region(V)
    n_sl = rg // SLICE
    member = np.zeros(NW * rg, bool)
    member[:V] = fin & (k >= kcut)
    wv = np.zeros(NW * rg, f32)
    wv[:V] = np.where(member[:V], wtab[np.where(fin, k, 0)], 0)
    wv = wv.reshape(NW, n_sl, 64, LANE)
    within = np.zeros((NW, n_sl, 64, LANE), f32)
    a = np.zeros((NW, n_sl, 64), f32)
    for j in range(LANE):
        a = (a + wv[..., j]).astype(f32)
        within[..., j] = a
    q = _lane_scan(a)
    qp = np.concatenate([np.zeros((NW, n_sl, 1), f32), q[..., :-1]], -1)
    total = q[..., 63]
    run_before = np.zeros((NW, n_sl), f32)
    r = np.zeros(NW, f32)
    for s in range(n_sl):
        run_before[:, s] = r
        r = (r + total[:, s]).astype(f32)
    before = np.zeros(NW, f32)
    z2 = f32(0)
    for w in range(NW):
        before[w] = z2
        z2 = f32(z2 + r[w])
    prefix = (before[:, None, None, None] + (run_before[:, :, None, None] + (qp[..., None] + within).astype(f32)).astype(f32)).astype(f32)
    return SimpleNamespace(empty=False, V=V, kcut=kcut, member=member, prefix=prefix.reshape(-1), z2=z2, above=above, before=before, wave_sum=r,
                           run_before=run_before, total=total, q=q, qp=qp, within=within, wv=wv, rg=rg, n_sl=n_sl)


def emulate_pick(e: SimpleNamespace, u: float) -> int:
    """The kernel's walk: wave region, slice, lane, token, each 'first whose inclusive prefix exceeds u Z2', with its fall-backs."""
    if e.empty:
        return 0
    target = float(u) * float(e.z2)
    mem = np.nonzero(e.member)[0]
    wsel, acc = -1, f32(0)
    for w in range(NW):
        acc = f32(acc + e.wave_sum[w])
        if float(acc) > target:
            wsel = w
            break
    if wsel < 0:
        return int(mem[-1])
    w = wsel
    in_region = mem[(mem >= w * e.rg) & (mem < (w + 1) * e.rg)]
    for s in range(e.n_sl):
        if float(f32(e.before[w] + f32(e.run_before[w, s] + e.total[w, s]))) > target:
            base = w * e.rg + s * SLICE
            hit = [l for l in range(64) if float(f32(e.before[w] + f32(e.run_before[w, s] + e.q[w, s, l]))) > target]
            in_slice = in_region[(in_region >= base) & (in_region < base + SLICE)]
            if not hit:
                return int(in_slice[-1])
            l = hit[0]
            i0 = base + l * LANE
            for j in range(LANE):
                if e.member[i0 + j] and float(f32(e.before[w] + f32(e.run_before[w, s] + f32(e.qp[w, s, l] + e.within[w, s, l, j])))) > target:
                    return i0 + j
            return int(in_slice[(in_slice >= i0) & (in_slice < i0 + LANE)][-1])
    return int(in_region[-1])


def measure_eps(rows) -> float:
    """Worst relative error of an emulated prefix mass or above-cut-off mass against the oracle, over `rows` (dicts with bits, T, top_p, top_k)."""
    worst = 0.0
    for r in rows:
        o, e = r["oracle"], r["emu"]
        if o.empty:
            continue
        assert (e.member[:o.V] == o.K).all(), (r["name"], e.kcut, o.kcut)
        idx = o.members
        rel = np.abs(e.prefix[idx].astype(np.float64) - o.prefix[idx]) / o.prefix[idx]
        worst = max(worst, float(rel.max()), abs(float(e.z2) - o.z2) / o.z2)
        for kk, ma in o.above.items():
            if ma > 0 and kk in e.above:
                worst = max(worst, abs(e.above[kk] - ma) / ma)
    return worst


def pow2ceil(x: float) -> float:
    return 2.0 ** int(np.ceil(np.log2(x)))


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def _row_shapes(V: int, rng: np.random.Generator):
    """name -> (values fp32 [V], [(T, top_p, top_k), ...])."""
    out = {}
    n = lambda s=1.0: rng.standard_normal(V).astype(np.float32) * s      # noqa: E731
    if V == 1:
        return {"single": (np.array([0.5], np.float32), [(0.7, 0.9, 50)])}
    x = n()
    x[V // 3] = 30.0
    out["dominant"] = (x, [(1.0, 0.9, 0), (1.0, 0.9, 50), (1.5, 0.05, V + 1)])
    x = n(0.5) - 8
    x[V // 5], x[(4 * V) // 5] = 5.0, 4.96875
    out["leaders"] = (x, [(1.0, 0.9, 0), (0.3, 1.0, 50), (1.0, 0.05, 0)])
    out["equal"] = (np.full(V, 1.5, np.float32), [(1.0, 0.9, 0), (0.7, 1.0, 50), (1.0, 1.0, V + 1), (1.0, 0.05, 1)])
    x = n() - 30
    for i, v in zip(np.linspace(1, V - 2, 5).astype(int), (-1.0, -1.5, -2.0, -2.5, -4.0)):
        x[i] = v
    out["negative"] = (x, [(1.0, 0.9, 0), (1.5, 1.0, 50), (0.0, 1.0, 0), (1.0, 0.9, 1)])
    x = n() - 40
    for i, v in zip(np.linspace(2, V - 3, 7).astype(int), (1.0, 0.5, 0.25, -0.5, -1.0, -1.75, -3.0)):
        x[i] = v
    out["mixed"] = (x, [(1.0, 0.9, 0), (1.0, 1.0, 0), (1.0, 0.9, V + 1)])
    if V >= 63:
        x = n(3.0)
        x[:V // 3] = -np.inf
        x[V - V // 3:] = -np.inf
        out["neginf"] = (x, [(1.0, 1.0, 0), (1.5, 1.0, 50)] + ([(0.3, 0.9, 0)] if V <= 4099 else []))
        x = n(3.0)
        x[::7] = np.nan
        x[V // 2] = np.inf
        out["nan"] = (x, [(1.0, 1.0, 0), (1.0, 1.0, 50)])
        x = n(3.0)
        out["normal"] = (x, [(0.3, 1.0, 0), (1.0, 1.0, 0), (1.5, 1.0, 50)] + ([(0.3, 0.9, 0), (0.3, 0.05, V + 1)] if V <= 1000 else [(0.3, 0.9, 50)]))
    if V >= 4099:      # heavy tokens on both sides of the lane / slice / wave-region boundaries, light ones between (runs of excluded tokens under top_k)
        x = n(0.25) - 12
        b = boundaries(V)
        pos = sorted({i for kind in b.values() for f in kind for i in (f - 1, f)} | {0, V - 1})
        for j, i in enumerate(pos):
            x[i] = 2.0 + 0.0625 * (j % 9)
        out["planted"] = (x, [(1.0, 1.0, 0), (1.0, 1.0, len(pos)), (0.7, 1.0, 0)])
    if V in KEYEDGE_V:     # cut-off keys on the key scan's partition: first / last key of a thread's 32-key range, a wave's first / last thread
        for half, t, pos in KEYEDGE:
            out[f"keyedge.{half}.{t}.{pos}"] = (_keyedge_row(V, half, t, pos), [(1.0, 0.9, 0), (1.0, 1.0, 3), (0.7, 0.9, 50)])
    return out


# (half, thread, position): the cut-off key.  Thread 511 is lane 63 of wave 7, thread 512 lane 0 of wave 8; positions 0 / 31 are a range's
# first / last key.  In the upper half these are the bf16 values 2.125 - 2^-7, 2.0 and 2.0 - 2^-7, in the negative half -(2.0 - 2^-7) and -2.0.
KEYEDGE = ((1, 511, 0), (1, 511, 31), (1, 512, 0), (0, 511, 31), (0, 512, 0))
KEYEDGE_V = (4099, 32773)


def scan_key(half: int, t: int, pos: int) -> int:
    """Inverse of scan_ranges()."""
    return (0x8000 if half else 0) + HALF - 1 - (t * KPT + pos)


def _keyedge_row(V: int, half: int, t: int, pos: int) -> np.ndarray:
    """One token on each of the two keys above the cut-off key X, 30 tokens tied on X, one on each of the two keys below, the rest of the row
    ~10 below: top_p = 0.9 cuts at X by mass (2 < 0.9 x 34 < 32 in units of one token's weight, which varies by < 4 % over the five keys),
    top_k = 3 cuts at X by count with its 30 ties kept, top_k = 50 with top_p = 0.9 cuts at X inside K1."""
    rng = np.random.default_rng(7000 + V + 97 * (2 * t + half) + pos)       # (its own generator: the other rows' values do not move)
    X = scan_key(half, t, pos)
    x = (rng.standard_normal(V) * 0.25 - 12).astype(np.float32)
    where = rng.permutation(V)[:34]
    for i, k in zip(where, [X + 2, X + 1] + [X] * 30 + [X - 1, X - 2]):
        x[i] = key_value(k)
    return x


def _draws(o: SimpleNamespace, V: int, rng: np.random.Generator, planted: bool) -> List[float]:
    us = [2.0 ** -25, 1.0 - 2.0 ** -25]
    if o.empty or V == 1:
        return us + [0.5]
    mem = o.members
    mid = lambda g: float(np.mean(interval(o, int(g))))      # noqa: E731
    us += [mid(mem[0]), mid(mem[-1])]
    gaps = np.nonzero(np.diff(mem) > 1)[0]
    if len(gaps):
        us.append(mid(mem[gaps[len(gaps) // 2] + 1]))           # a kept token just after a run of excluded ones
    if planted:
        for kind in boundaries(V).values():
            for f in kind:
                us += [mid(g) for g in (f - 1, f) if o.K[g]]
    us += rng.random(3).tolist()
    return [float(np.float32(u)) for u in us]


LAYOUT = {1: (1, 1), 63: (32, 63), 1000: (32, 1024), 4099: (32, 4099), 32773: (32, 32776), 151936: (256, 151936)}      # V -> (B, ld)
EXTRA_LAYOUT = {63: (3, 63), 151936: (32, 151944)}

_cache: dict = {}


def rows_and_batches():
    """-> (rows, batches).  rows: dicts(name, V, bits, T, top_p, top_k, oracle, emu, draws); batches: dicts(V, B, ld, items = [(row index, u)]) —
    every (row, draw) pair sits in a batch of its V; pairs past the last full batch are completed with filler draws of the same rows."""
    if "v" in _cache:
        return _cache["v"]
    rows, batches = [], []
    for V, (B, ld) in LAYOUT.items():
        rng = np.random.default_rng(1000 + V)
        first = len(rows)
        for name, (x, params) in _row_shapes(V, rng).items():
            bits = to_bits(x)
            for T, top_p, top_k in params:
                o = oracle(bits, T, top_p, top_k)
                rows.append(dict(name=f"V{V}-{name}-T{T}-p{top_p}-k{top_k}", V=V, bits=bits, T=T, top_p=top_p, top_k=top_k, oracle=o,
                                 emu=emulate(bits, T, top_p, top_k), draws=_draws(o, V, rng, name == "planted")))
        pairs = [(i, u) for i in range(first, len(rows)) for u in rows[i]["draws"]]
        layouts = [(B, ld)] + ([EXTRA_LAYOUT[V]] if V in EXTRA_LAYOUT else [])
        if V in EXTRA_LAYOUT:      # the second layout takes the planted rows' pairs again (the padded, aligned rows of a prefill head)
            b2, ld2 = EXTRA_LAYOUT[V]
            pl = [pr for pr in pairs if "planted" in rows[pr[0]]["name"] or V < 4099][:b2]
            pl += [(pl[j % len(pl)][0], float(np.float32(rng.random()))) for j in range(b2 - len(pl))]
            batches.append(dict(V=V, B=b2, ld=ld2, items=pl))
        for a in range(0, len(pairs), B):
            chunk = pairs[a:a + B]
            chunk += [(pairs[j % len(pairs)][0], float(np.float32(rng.random()))) for j in range(B - len(chunk))]
            batches.append(dict(V=V, B=B, ld=ld, items=chunk))
    _cache["v"] = (rows, batches)
    return rows, batches


def batch_buffers(rows, batch):
    """-> (logits uint16 [B, ld] with NaN past V, params rows [(T, top_p, top_k, seed, stream)], u fp32 [B])."""
    B, ld, V = batch["B"], batch["ld"], batch["V"]
    logits = np.full((B, ld), 0x7fc0, np.uint16)
    params, us = [], []
    for b, (i, u) in enumerate(batch["items"]):
        r = rows[i]
        logits[b, :V] = r["bits"]
        params.append((r["T"], r["top_p"], r["top_k"], 0, b))
        us.append(u)
    return logits, params, np.asarray(us, np.float32)
