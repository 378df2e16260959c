"""Seeded cases, the fp64 reference and the tolerance of the decode attention entries (fo1_attention_decode_batch_bf16, its partials-only
form, fo1_attention_decode_bf16), shared by tests/test_decode_attention_cases.py (CPU: the tolerance can fail) and
tests/test_decode_attention_gpu.py (the route sweep on the MI355X).

A case lays out what the batched entry reads: the K cache [KV][rows][128], the V^T cache [KV*128][rows] and q rows [B][Hq*128], each
optionally with a padded stride (k_head_stride, vt_row_stride, q_seq_stride as the pool's qkv[:, :Hq*128] view; the output stride is
padded by the GPU test), and the int32 [B][8] state {pos, -, kv_start, finished, ...}.  Slots lie in a shuffled order with a few spare
rows between them, so that nothing can assume slot = b * stride, and every key range has a row on either side.

Two kinds of planted data turn a wrong key range into a gross error rather than a statistical one:
  * planted keys: at positions 0 and ctx-1 of every context and on both sides of every 64-key (so also every 1024-key) boundary inside
    it, a K row along the mean query direction of its KV head's group (score about PLANT_SCORE) and a V row with a spike of +-SPIKE in a
    position-specific dimension;
  * poison rows: just outside each range (kv_start-1 and pos+1) a K row that scores higher still and a V row of +-POISON (finite: the
    kernel may read a V^T piece next to a zero weight, and 0 x finite = 0).
The rest are plain N(0, 1) rows; q is drawn at temperature 1 or 3 (3: random scores with std ~3, the running max moves between tiles).
One planted key per sequence (the "peak") scores higher than the others: in the first tile, the last tile, or on both sides of the 63/64
or 1023/1024 boundary.

Tolerance: one bound per (sequence, query head) row, max|got - ref| <= TOL * max|ref row|, ref in float64 on the bf16 inputs.  TOL = 2^-6
comes from emulate() — the kernel's roundings on the CPU (fp32 scores, base-2 running max per 64-key tile, P rounded to bf16 before PV,
fp32 sums of the unrounded P, bf16 output) — whose error is at most 0.41 TOL (0.0063 of the row maximum, at 1024..2112-key contexts
and temperature 1) over every case here; tests/test_decode_attention_cases.py asserts at most TOL / 2.  The kernels' own error at these shapes
is what the GPU sweep measures against it; the CPU test also shows that a dropped key, an included poison row, kv_start off by one or
a wrong KV head for a query head exceeds TOL at least twice on every live sequence of every case."""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

HD = 128
TOL = 2.0 ** -6
PLANT_SCORE = {1: 6.0, 3: 14.0}     # scaled score of a planted key, by q temperature (random keys at 4096: max ~3.5 / ~10.5)
PEAK_EXTRA = 1.0
POISON_EXTRA = 8.0
SPIKE = 16.0
POISON = 64.0
LOG2E = 1.4426950408889634


@dataclass
class Case:
    name: str
    B: int
    max_kv_len: int
    Hq: int = 16
    Hkv: int = 2
    pad: bool = False
    temp: int = 1
    peak: str = "last"                 # first | last | b64 | b1024
    seed: int = 0
    single: bool = False               # fo1_attention_decode_bf16: one sequence, keys [0, n), n = ctx[0]
    ctx: Optional[List[int]] = None    # explicit contexts (default: contexts(case))
    finished: Optional[Tuple[int, ...]] = None   # indices of finished sequences (None: one for B > 1; () for none)
    headroom: int = 0                  # spare rows after each context inside its slot (graph replay advances the contexts)
    route: str = ""


def contexts(c: Case) -> List[int]:
    """1, max_kv_len, max_kv_len - 1, multiples of 64 +-1 and random lengths; long random ones only for a few sequences of a pool."""
    if c.ctx is not None:
        return list(c.ctx)
    L = c.max_kv_len
    g = torch.Generator().manual_seed(1000 + c.seed)
    spec = [L, 1, max(1, L - 1)]
    for t in sorted({64, 128, 1024, (L // 64) * 64, 16 * 64}):
        for n in (t - 1, t, t + 1):
            if 1 <= n <= L and n not in spec:
                spec.append(n)
    out = spec[:c.B]
    while len(out) < c.B:
        hi = L if (len(out) < 12 or c.B <= 32) else min(L, 200)
        out.append(int(torch.randint(1, hi + 1, (1,), generator=g)))
    perm = torch.randperm(c.B, generator=g).tolist()
    return [out[i] for i in perm]


def finished_of(c: Case) -> Tuple[int, ...]:
    if c.finished is not None:
        return tuple(c.finished)
    return () if c.B == 1 else ((c.seed * 7 + 3) % c.B,)


def planted_positions(n: int, peak: str):
    """-> (relative positions of the planted keys, relative positions of the peak keys) of an n-key context."""
    pos = {0, n - 1}
    for t in range(64, n, 64):
        pos.update((t - 1, t))
    want = {"first": [0], "last": [n - 1], "b64": [63, 64], "b1024": [1023, 1024]}[peak]
    pk = [p for p in want if p < n] or [n - 1]
    return sorted(pos), pk


def build(c: Case) -> dict:
    """-> CPU tensors (strided views where c.pad) + layout: kc [KV][rows][HD], vt [KV*HD][rows], q [B][Hq*HD], state int32 [B][8]."""
    g = torch.Generator().manual_seed(20261016 + c.seed)
    B, Hq, KV = c.B, c.Hq, c.Hkv
    G = Hq // KV
    ctx = contexts(c)
    fin = finished_of(c)
    scale = HD ** -0.5
    # slots: sequence order shuffled in memory, kv_start 4 rows into the slot (a multiple of 4: the kernels read V^T in 4-key pieces)
    if c.single:
        assert B == 1
        starts, rows = [0], c.max_kv_len + 4
    else:
        order = torch.randperm(B, generator=g).tolist()
        starts, base = [0] * B, 0
        for b in order:
            starts[b] = base + 4
            base += 4 + -(-(ctx[b] + c.headroom + 1) // 4) * 4 + 4
        rows = base
    kpad, vpad = (40, 12) if c.pad else (0, 0)
    kbuf = torch.randn(KV, rows + kpad, HD, generator=g)
    vbuf = torch.randn(KV * HD, rows + vpad, generator=g)
    qw = (Hq + 2 * KV) * HD if c.pad else Hq * HD
    qbuf = torch.randn(B, qw, generator=g) * c.temp
    qbuf = qbuf.bfloat16().float()
    q = qbuf[:, :Hq * HD]
    plant = PLANT_SCORE[c.temp]
    for b in range(B):
        n, lo = ctx[b], starts[b]
        for kvh in range(KV):
            qg = q[b].view(Hq, HD)[kvh * G:(kvh + 1) * G]
            u = qg.sum(0)
            u = u / u.norm()
            dots = qg @ u
            unit = u / (dots.mean() * scale)            # K row = s * unit scores ~s (scaled) for the group's heads
            ps, pk = planted_positions(n, c.peak)
            for r in ps:
                kbuf[kvh, lo + r] = unit * (plant + (PEAK_EXTRA if r in pk else 0.0))
                col = vbuf[kvh * HD:(kvh + 1) * HD, lo + r]
                col.mul_(0.5)
                col[(37 * (lo + r) + 53 * kvh) % HD] = SPIKE if (lo + r + kvh) % 2 == 0 else -SPIKE
            sign = torch.tensor([1.0, -1.0]).repeat(HD // 2)
            for r in (lo - 1, lo + n):
                if 0 <= r < rows:
                    kbuf[kvh, r] = unit * (plant + POISON_EXTRA)
                    vbuf[kvh * HD:(kvh + 1) * HD, r] = POISON * sign
    kbuf, vbuf = kbuf.bfloat16(), vbuf.bfloat16()
    state = torch.zeros(B, 8, dtype=torch.int32)
    for b in range(B):
        state[b, 2] = starts[b]
        state[b, 0] = starts[b] + ctx[b] - 1
        state[b, 3] = 1 if b in fin else 0
    return dict(case=c, kbuf=kbuf, vbuf=vbuf, qbuf=qbuf.bfloat16(), kc=kbuf[:, :rows], vt=vbuf[:, :rows], q=qbuf.bfloat16()[:, :Hq * HD],
                state=state, ctx=ctx, rows=rows, scale=scale, G=G)


def reference(d: dict, state: Optional[torch.Tensor] = None, lo_delta: int = 0, hi_delta: int = 0, drop: Tuple[int, ...] = (),
              head_map=None, seqs=None) -> torch.Tensor:
    """fp64 softmax(q K^T * scale) V per sequence and query head -> [B, Hq, HD]; finished sequences exact zeros.  The keyword arguments
    are the CPU test's mutations: key range [kv_start + lo_delta, pos + hi_delta], relative positions `drop` left out, `head_map(h)`
    the KV head of query head h (default h // group); `seqs` limits the work to those sequences (the other rows stay zero)."""
    c = d["case"]
    st = d["state"] if state is None else state
    KV, Hq = c.Hkv, c.Hq
    kc, vt, q = d["kc"], d["vt"], d["q"]
    hm = head_map or (lambda h: h // d["G"])
    out = torch.zeros(c.B, Hq, HD, dtype=torch.float64)
    for b in (range(c.B) if seqs is None else seqs):
        if int(st[b, 3]):
            continue
        lo, hi = int(st[b, 2]) + lo_delta, int(st[b, 0]) + hi_delta
        idx = torch.arange(lo, hi + 1)
        if drop:
            keep = torch.ones(len(idx), dtype=torch.bool)
            for r in drop:
                if 0 <= r - lo_delta < len(idx):
                    keep[r - lo_delta] = False     # r: position relative to kv_start
            idx = idx[keep]
        if len(idx) == 0:
            continue
        qb = q[b].double().view(Hq, HD)
        for kvh in range(KV):
            heads = [h for h in range(Hq) if hm(h) == kvh]
            if not heads:
                continue
            keys = kc[kvh, idx].double()                          # [n, HD]
            vals = vt[kvh * HD:(kvh + 1) * HD, idx].double()      # [HD, n]
            p = torch.softmax(qb[heads] @ keys.t() * d["scale"], -1)
            out[b, heads] = p @ vals.t()
    return out


def emulate(d: dict) -> torch.Tensor:
    """The kernel's roundings on the CPU -> bf16-valued float [B, Hq, HD]: fp32 scores, base-2 running max per 64-key tile from kv_start,
    e = exp2(c1 s - m) in fp32, P = bf16(e) into PV, l = the fp32 sum of the unrounded e, output bf16(o / l)."""
    c = d["case"]
    st = d["state"]
    KV, Hq, G = c.Hkv, c.Hq, d["G"]
    out = torch.zeros(c.B, Hq, HD)
    c1 = torch.tensor(d["scale"] * LOG2E, dtype=torch.float32)
    for b in range(c.B):
        if int(st[b, 3]):
            continue
        lo, hi = int(st[b, 2]), int(st[b, 0])
        n = hi - lo + 1
        T = -(-n // 64)
        qb = d["q"][b].float().view(Hq, HD)
        for kvh in range(KV):
            keys = d["kc"][kvh, lo:hi + 1].float()
            vals = d["vt"][kvh * HD:(kvh + 1) * HD, lo:hi + 1].float().t()
            s = torch.full((G, T * 64), float("-inf"))
            s[:, :n] = (qb[kvh * G:(kvh + 1) * G] @ keys.t()) * c1
            s = s.view(G, T, 64)
            m = torch.cummax(s.amax(-1), -1).values               # running max after each tile
            e = torch.exp2(s - m.unsqueeze(-1))
            p = e.bfloat16().float().view(G, T * 64)[:, :n]
            w = torch.exp2(m - m[:, -1:])                         # each tile's rescale to the final max
            l = (e.sum(-1) * w).sum(-1)
            o = (p * w.repeat_interleave(64, dim=1)[:, :n]) @ vals
            out[b, kvh * G:(kvh + 1) * G] = (o / l.unsqueeze(-1)).bfloat16().float()
    return out


def row_ratios(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """max|got - ref| / max|ref| per (sequence, head) row -> [B, Hq] (rows of exact zeros: max|got|, so any nonzero value is a failure)."""
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs().amax(-1)
    den = ref.abs().amax(-1)
    return torch.where(den > 0, err / den.clamp_min(1e-300), err * 1e300)


def check(got: torch.Tensor, d: dict, what: str, ref: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None) -> float:
    """Asserts the per-row bound (and exact zeros for finished sequences); -> the worst ratio / TOL."""
    st = d["state"] if state is None else state
    ref = reference(d, state=st) if ref is None else ref
    got = got.float().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output (a row left unwritten?) in sequences " \
        f"{sorted(set(torch.nonzero(~torch.isfinite(got))[:, 0].tolist()))}"
    for b in range(ref.shape[0]):
        if int(st[b, 3]):
            assert got[b].abs().max().item() == 0.0, f"{what}: finished sequence {b} has a nonzero row"
    r = row_ratios(got, ref)
    worst = r.max().item()
    b, h = divmod(int(r.argmax()), ref.shape[1])
    assert worst <= TOL, f"{what}: sequence {b} (ctx {d['ctx'][b]}) head {h}: max|err| / max|ref| = {worst:.4g} > {TOL:.4g}"
    return worst / TOL


def _sweep() -> List[Case]:
    cases, k = [], 0
    peaks = ("first", "last", "b64", "b1024")

    def add(route, B, L, **kw):
        nonlocal k
        kw.setdefault("pad", k % 3 == 0)
        kw.setdefault("temp", 1 if k % 2 == 0 else 3)
        kw.setdefault("peak", peaks[k % 4])
        heads = kw.pop("heads", (16, 2))
        cases.append(Case(f"{route}-B{B}-L{L}-h{heads[0]}x{heads[1]}" + ("-pad" if kw["pad"] else ""), B, L, Hq=heads[0], Hkv=heads[1],
                          seed=k, route=route, **kw))
        k += 1

    for B in (1, 2, 16):                      # <= 16 sequences: 64-key chunks, one tile per item, split + combine
        for L in (65, 192, 1025, 2048):
            add("split64", B, L)
    add("split64", 2, 192, heads=(16, 16))
    add("split64", 16, 1025, heads=(12, 2), pad=True)
    for B in (1, 16, 17, 25, 32):             # <= 32 sequences, max_kv_len <= 64: one chunk, rows written by the split kernel itself
        for L in (1, 17, 63, 64):
            add("one_chunk", B, L)
    add("one_chunk", 25, 64, heads=(16, 16), pad=True)
    add("one_chunk", 17, 63, heads=(12, 2))
    for B in (17, 25, 32):                    # 17..32 sequences: two-tile items (odd and even chunk counts) + combine
        for L in (65, 128, 192, 2048, 2112):
            add("two_tile", B, L)
    add("two_tile", 25, 192, heads=(16, 16))
    add("two_tile", 25, 2112, heads=(12, 2), pad=True)
    for B in (33, 64, 128):                   # > 32 sequences, max_kv_len <= 1024: one 1024-key chunk
        for L in (1, 64, 1024):
            add("pool_one", B, L)
    add("pool_one", 64, 1024, heads=(12, 2), pad=True)
    for B in (33, 128):                       # > 32 sequences: 1024-key chunks + combine
        for L in (1025, 2048, 4096):
            add("pool_split", B, L)
    add("pool_split", 33, 1025, heads=(16, 16), pad=True)
    return cases


SWEEP = _sweep()

# partials + fo1_gemv_attn_combine_bf16 (o-projection with the combine in its prologue, M <= 2)
GEMV_CASES = [Case(f"gemv-B{B}-L{L}", B, L, seed=500 + i, temp=1 + 2 * (i % 2), peak=("first", "last", "b64", "b1024")[i % 4], pad=i % 3 == 0,
                   route="gemv", finished=(1,) if (B == 2 and L == 2048) else ())   # two live sequences at 1, 64, 65 keys
              for i, (B, L) in enumerate((B, L) for B in (1, 2) for L in (1, 64, 65, 2048))]

# fo1_attention_decode_bf16 (one sequence, device-side length): keys [0, n) of a cache of max_kv_len + 4 rows
SINGLE_CASES = [Case(f"single-n{n}", 1, 4096, ctx=[n], single=True, seed=600 + i, temp=1 + 2 * (i % 2), peak=("first", "last", "b64", "b1024")[i % 4],
                     route="single")
                for i, n in enumerate((1, 63, 64, 65, 1024, 4096))]

# 25 sequences at the bounds of the tiles-per-item test (fo1_attention_decode_set_small_chunk(1 .. 8)): one chunk, odd and even chunk counts
TILES_CASES = [Case(f"tiles-B25-L{L}", 25, L, seed=900 + L, pad=L == 192, route="tiles") for L in (64, 192, 2048, 2112)]

# graph replay: 25 sequences with 64 spare rows per slot; the test advances the contexts by 1 or 64 on the device
GRAPH_CASE = Case("graph-B25-L2048", 25, 2048, ctx=[1, 63, 64, 65, 127, 128, 700, 1023, 1024, 1025, 1900, 5, 333, 900, 1500, 77, 640, 641, 12,
                                                     1960, 512, 191, 192, 193, 1],
                  finished=(7,), headroom=64, seed=950, pad=True, route="graph")

ALL_CASES = SWEEP + GEMV_CASES + SINGLE_CASES + TILES_CASES + [GRAPH_CASE]


def bound_class_alternative(c: Case) -> int:
    """Another max_kv_len of the same batch class, at least every context: one chunk vs split + combine, 64 vs 2048 keys (<= 32 sequences),
    1024 vs 4096 (pools)."""
    if c.B > 32:
        return 4096 if c.max_kv_len <= 2048 else 1024 * 5
    return 2048 if c.max_kv_len < 2048 else 4096


def scale_down(c: Case, cap: int = 4096) -> Case:
    """The same case with at most `cap`-key contexts (the CPU self-check keeps its run short)."""
    if c.max_kv_len <= cap:
        return c
    ctx = None if c.ctx is None else [min(n, cap) for n in c.ctx]
    return Case(**{**c.__dict__, "max_kv_len": cap, "ctx": ctx, "name": c.name + f"-cap{cap}"})


def to_device(d: dict) -> dict:
    """The same views on cuda:0 (strides kept: the kernel reads what the reference read)."""
    c = d["case"]
    kbuf, vbuf, qbuf = d["kbuf"].cuda(), d["vbuf"].cuda(), d["qbuf"].cuda()
    return dict(kc=kbuf[:, :d["rows"]], vt=vbuf[:, :d["rows"]], q=qbuf[:, :c.Hq * HD], state=d["state"].cuda())


__all__ = ["HD", "TOL", "Case", "SWEEP", "GEMV_CASES", "SINGLE_CASES", "TILES_CASES", "GRAPH_CASE", "ALL_CASES", "build", "reference", "emulate", "check", "row_ratios",
           "contexts", "planted_positions", "bound_class_alternative", "scale_down", "to_device"]
