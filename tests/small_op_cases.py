"""Cases, fp64 references, per-element bounds, emulated kernel arithmetic and faults of the small exported kernels that had no operator-level
test: csrc/swin_ops.hip (window partition / reverse-add, PatchMerging gather, GroupNorm over tokens), csrc/upn_ops.hip (sine embedding, box
refinement, row masking, row gather, top-k), rownorm_kernel<MODE, NPER, LPR> behind fo1_rmsnorm_bf16 / fo1_layernorm_bf16 / fo1_layernorm_rows_bf16,
fo1_argmax_bf16, fo1_add_bf16, fo1_bias_act_bf16, fo1_swiglu_bf16 (csrc/norm_act.hip) and csrc/preprocess.hip.  Shared by
tests/test_small_op_cases.py (CPU) and tests/test_small_ops_gpu.py (the MI355X sweep).  HALF_ULP, the GELU slope and the canary pattern come from
tests/gemm_route_cases.py.

Per family: CASES[family] (named cases, the smallest shapes at which the kernel can still go wrong), inputs(case) (seeded, bf16-representable where
the kernel reads bf16), reference(case) (float64 on those inputs, no intermediate rounding), bound(case) (one number per element, None for a
bit-exact op), emulate(case, fault) (the kernel's fp32 order and bf16 rounding points in torch) and FAULTS[family] (one-line mutations of the
emulation).  route(D) restates launch_rownorm, argmax_route(n) restates fo1_argmax_bf16.

Bounds.  Pure copies (partition, patch_merge, mask_rows, gather_rows_f32, patchify, normalize, top-k and argmax indices) are bit-exact.  One fp32
add and one RNE cast (swin_window_reverse_add, add) is bit-exact against torch's fp32 add + .to(bfloat16): the inputs are multiples of 2^-6 below
4, so the fp32 sum is itself exact (asserted on the CPU).  Everything else:
    |got - exact| <= sum over the bf16 rounding points of half an ulp of the value's own binade, carried to the output by the later steps' slope
                     + 2^-24 |value| for every fp32 rounding of the output expression (format, not measured)
                     + the statistics term REL (|x| + |mean|) rstd |w|   (|mean| omitted for RMSNorm)
  * REL is 4 x the emulation's worst |rstd_fp32 - rstd_fp64| / rstd_fp64 over the cases, rounded up to a power of two (RESULTS_CPU); the CPU test
    holds the emulation to the bound with the statistics term at REL / 4.  GroupNorm's emulation is measured in both forms the compiler may emit
    for b / n - mean * mean (fused and unfused).
  * sine_embed: half a bf16 ulp + SINE_T, SINE_T = 4 x the worst |fp32 chain - fp64| (powf, the fp32 2 pi, the division, sinf / cosf).
  * box_refine (fp32 out): BOX_REL |ref| + BOX_ABS, 8 x the worst relative error of the fp32 chain over all elements and 8 x its worst absolute
    error over the elements below 2^-10 (device logf / expf are specified to 1 - 2 ulp, glibc's are below 1: hence 8, not 4).
  * bias_act: bf16(x + bias) is a rounding point (slope of GELU 1.13); the erf-GELU of common.h is Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7 on
    erfc) on v_rcp_f32 / v_exp_f32 and five fmaf: 8 x 2^-24 more on erfc, so |v| 3.2e-7 on the output, plus two fp32 roundings.
  * swiglu: fo1_silu is v rcp(1 + exp2(-v log2 e)): the product -v log2 e rounds once (relative |v| 2^-24 on the exponential), rcp, exp and two
    more roundings a further 4 x 2^-24; then bf16(silu) and bf16(silu u) (the product of two bf16 values is exact in fp32).
No element gets a "rare fraction" allowance.

Inputs worth knowing.  rownorm rows cycle through unit gaussian x 3, mean 50 sigma, all zero, only the last chunk non-zero; GroupNorm groups have their
own mean in [-16 sigma, 16 sigma] and scale in [0.25, 4], the last token sits at mean + 3 sigma in every such group (a dropped last chunk of one token
moves the mean), one group is constant (variance 0) and, with 4 or more groups, one holds +-2^-9 only (variance 3.8e-6, next to eps: what tells eps
inside the sqrt from eps outside; added to the issue's list because the constant group cannot: x - mean is 0 there whatever rstd is).

One fault is not a bound violation and cannot be: RMSNorm without the inner bf16 rounding moves the result TOWARDS the float64 reference (it is at most
half an ulp away, inside any bound built from rounding points) and by at most |w| hu(x rstd) + 2 hu(out) < 2 x bound from the emulation.  FAULTS marks
it bitwise: it must change bits of the emulation, as for an exact op.  No GPU test can tell the two forms apart by a bound either (the <= 1.01 ulp of
tests/test_ops_gpu.py::test_rmsnorm_layernorm against the twice-rounded torch expression holds for both).

RESULTS_CPU (tests/test_small_op_cases.py -s; 462 cases, 6 s):
  worst |rstd_fp32 - rstd_fp64| / rstd_fp64 of the emulation: rmsnorm 1.04e-7 (1.74 x 2^-24), layernorm 4.99e-7 (8.36 x 2^-24), groupnorm 1.98e-5 (332 x 2^-24: the
  one-pass variance at a group mean of 16 sigma) -> REL = 2^-21 (rmsnorm), 2^-18 (layernorm, layernorm_rows), 2^-13 (groupnorm): the power of two next above
  4 x measured; sine_embed fp32 chain 7.61e-7 -> SINE_T = 2^-18 (3.8e-6 >= 4 x); box_refine fp32 chain 1.15e-6 relative (the sigmoid tails at |logit| = 19),
  2.7e-10 absolute below 2^-10 -> BOX_REL = 2^-16, BOX_ABS = 2^-28 (>= 8 x).  The figures move with the draw (another seeding gave 3.65 x 2^-24 for layernorm):
  after changing a case or a seed, measure again and reset the constants; test_zz_summary fails until they are the next power of two.
  The emulation reaches 1.000 of the quarter bound on rownorm and bias_act / swiglu and 0.999 on sine_embed (a near tie at a rounding point: the half ulp is the
  worst case of round-to-nearest and these inputs meet it), 0.990 on groupnorm, 0.043 on box_refine.  Weakest faults: unbiased GroupNorm variance 83 x the bound
  (S = 1, 8 elements per group), dropped last chunk 350 x, box_refine without the clamp 628 x, eps outside the sqrt 7e3 x (the +-2^-9 group); every other fault of a
  bounded op is beyond 8e4 x, every fault of an exact op changes elements or indices.
RESULTS_GPU (MI355X, tests/test_small_ops_gpu.py -s: 463 passed in 2.7 s, wall time 0.9 s for 462 cases; every canary intact, every second launch bit-identical).
Worst |got - ref| / bound per op and route ('-': one route; exact: bit for bit):
add - exact; argmax one exact; argmax two exact; bias_act - 1.000; box_refine mode0 0.057; box_refine mode1 0.004; box_refine mode2 0.020
gather_rows - exact; groupnorm cg16 0.911; groupnorm cg64 0.783; groupnorm cg8 0.971; layernorm (1,32) 0.998; layernorm (1,64) 1.000
layernorm (2,64) 0.998; layernorm (3,64) 1.000; layernorm (4,64) 1.000; layernorm (8,64) 1.000; layernorm_rows (1,32) 0.998
layernorm_rows (1,64) 1.000; layernorm_rows (2,64) 0.998; layernorm_rows (3,64) 1.000; layernorm_rows (4,64) 1.000; layernorm_rows (8,64) 1.000
mask_rows - exact; normalize - exact; partition - exact; patch_merge - exact; patchify - exact; reverse_add - exact; rmsnorm (1,32) 0.990
rmsnorm (1,64) 0.991; rmsnorm (2,64) 0.991; rmsnorm (3,64) 0.991; rmsnorm (4,64) 0.999; rmsnorm (8,64) 0.999; sine_embed - 0.998; swiglu - 1.000
topk - exact.
A bf16 output at 0.99 - 1.000 of its bound is an element next to a rounding tie: the bound's half ulp is the exact worst case of round-to-nearest, and what leaves
room is only the statistics term.  Before the f32_order fix the cases topk-n2-k2-s1, topk-n5-k3-s2 and topk-n1024-k1024-s1 failed on the MI355X (+0.0 ahead of the
-0.0 at the lower index); they pass with it."""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from gemm_route_cases import CANARY16, CANARY32, GELU_SLOPE, HALF_ULP  # noqa: F401

BF = torch.bfloat16
F32_EPS = 2.0 ** -24
REL = {"rmsnorm": 2.0 ** -21, "layernorm": 2.0 ** -18, "layernorm_rows": 2.0 ** -18, "groupnorm": 2.0 ** -13}
SINE_T = 2.0 ** -18
BOX_REL, BOX_ABS = 2.0 ** -16, 2.0 ** -28
RMS_EPS = float(np.float32(1e-6))
LN_EPS = float(np.float32(1e-5))
GN_EPS = float(np.float32(1e-5))
BOX_EPS = float(np.float32(1e-3))
CANARY_BF = torch.tensor([CANARY16], dtype=torch.int16).view(BF).item()
CANARY_F32 = torch.tensor([CANARY32], dtype=torch.int32).view(torch.float32).item()


class Case:
    def __init__(self, family: str, name: str, **p):
        self.family, self.name, self.p = family, name, p
        self.__dict__.update(p)

    def __repr__(self) -> str:
        return self.name


def _gen(*key) -> torch.Generator:
    seed = 7
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rb(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    return x.float().to(BF).float()


def half_ulp(v: torch.Tensor, e=0.0) -> torch.Tensor:
    """Half a bf16 ulp of the binade that a value known to within e of v can lie in."""
    return torch.exp2(torch.floor(torch.log2((v.abs() + e).clamp_min(2.0 ** -126))) - 8.0)


def rnd(e: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """Error after a bf16 rounding of a value v known to within e."""
    return e + half_ulp(v, e)


def grid_values(shape, g: torch.Generator) -> torch.Tensor:
    """randn-scale multiples of 2^-6 below 4: bf16-representable, and the fp32 sum of two of them is exact."""
    return ((torch.randn(shape, generator=g) * 64).round().clamp(-255, 255) / 64).to(BF)


def framed(t: torch.Tensor, ld: int, spare_rows: int = 1) -> torch.Tensor:
    """[M, D] -> a [M + spare, ld] canary buffer holding t in its first M rows and D columns."""
    M, D = t.shape
    can = CANARY_F32 if t.dtype == torch.float32 else CANARY_BF
    buf = torch.full((M + spare_rows, ld), can, dtype=t.dtype)
    buf[:M, :D] = t
    return buf


def canary_intact(buf: torch.Tensor, M: int, D: int) -> bool:
    bits = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16).clone()
    can = CANARY32 if buf.dtype == torch.float32 else CANARY16
    bits[:M, :D] = can
    return bool((bits == can).all())


_INPUTS: Dict[str, dict] = {}
CASES: Dict[str, List[Case]] = {}
FAULTS: Dict[str, Dict[str, str]] = {}
BITWISE_FAULTS = {("rownorm", "rms_no_inner_round")}


def inputs(c: Case) -> dict:
    if c.name not in _INPUTS:
        _INPUTS[c.name] = _BUILD[c.family](c)
    return _INPUTS[c.name]


# ---------------------------------------------------------------------------------------------------------------------------------------
# rownorm: rmsnorm, layernorm, layernorm_rows
# ---------------------------------------------------------------------------------------------------------------------------------------
ROW_D = (8, 256, 264, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 4096)
ROW_M = (1, 7, 9)
ROUTES = ((1, 32), (1, 64), (2, 64), (3, 64), (4, 64), (8, 64))


def route(D: int) -> Tuple[int, int]:
    """launch_rownorm: (NPER, LPR) by the row's 16-byte chunks."""
    n = D >> 3
    if n <= 32:
        return (1, 32)
    if n <= 64:
        return (1, 64)
    if n <= 128:
        return (2, 64)
    if n <= 192:
        return (3, 64)
    if n <= 256:
        return (4, 64)
    return (8, 64)


def _rownorm_cases() -> List[Case]:
    out = []
    for op in ("rmsnorm", "layernorm", "layernorm_rows"):
        for D in ROW_D:
            for M in ROW_M:
                out.append(Case("rownorm", f"{op}-d{D}-m{M}", op=op, D=D, M=M, ldx=D, ldy=D))
        for D in (256, 512, 1024, 1536, 2048, 2056):      # one strided case per route (256 is the full end of (1, 32))
            out.append(Case("rownorm", f"{op}-d{D}-m7-strided", op=op, D=D, M=7, ldx=D + 8, ldy=D + 16))
    return out


def _rownorm_build(c: Case) -> dict:
    D, M = c.D, c.M
    g = _gen(D, M, 11)                      # the same input for the three ops: layernorm_rows is compared with layernorm bit for bit
    x = torch.zeros(M, D)
    for m in range(M):
        kind = (m + ROW_D.index(D)) % 4
        if kind == 0:
            x[m] = 3 * torch.randn(D, generator=g)
        elif kind == 1:
            x[m] = 150 + 3 * torch.randn(D, generator=g)        # mean 50 sigma
        elif kind == 3:
            x[m, -8:] = 3 * torch.randn(8, generator=g)          # only the last chunk
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(BF)
    b = (0.1 * torch.randn(D, generator=g)).to(BF)
    d = dict(x=x.to(BF), w=w, b=b)
    if c.op == "layernorm_rows":
        perm = torch.randperm(M, generator=g)
        d["rows"] = (2 * perm + 1).to(torch.int32)             # permuted, with gaps, into a y of 2 M + 2 rows
        d["y_rows"] = 2 * M + 2
    return d


def _rownorm_stats64(c: Case):
    d = inputs(c)
    x = d["x"].double()
    if c.op == "rmsnorm":
        mean = torch.zeros(c.M, 1, dtype=torch.float64)
        rstd = 1.0 / torch.sqrt(x.pow(2).mean(-1, keepdim=True) + RMS_EPS)
    else:
        mean = x.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt((x - mean).pow(2).mean(-1, keepdim=True) + LN_EPS)
    return x, mean, rstd


def _rownorm_ref(c: Case) -> torch.Tensor:
    d = inputs(c)
    x, mean, rstd = _rownorm_stats64(c)
    y = (x - mean) * rstd * d["w"].double()
    return y if c.op == "rmsnorm" else y + d["b"].double()


def _rownorm_bound(c: Case, quarter: bool = False) -> torch.Tensor:
    d = inputs(c)
    x, mean, rstd = _rownorm_stats64(c)
    w = d["w"].double().abs()
    rel = REL[c.op] * (0.25 if quarter else 1.0)
    stat = rel * (x.abs() + mean.abs()) * rstd
    if c.op == "rmsnorm":
        v1 = x * rstd                                            # fp32 product, then bf16
        e1 = rnd(stat + F32_EPS * v1.abs(), v1)
        return rnd(w * e1, v1 * d["w"].double())                 # bf16 x bf16 is exact in fp32; the store rounds
    v = (x - mean) * rstd * d["w"].double()
    out = v + d["b"].double()
    return rnd(stat * w + 2 * F32_EPS * v.abs() + F32_EPS * out.abs(), out)


def _seq_sum(v: torch.Tensor, square: bool) -> torch.Tensor:
    """Per-lane sequential fp32 sum (fmaf for the squares) over the last axis."""
    acc = torch.zeros(v.shape[:-1], dtype=torch.float32)
    for j in range(v.shape[-1]):
        t = v[..., j]
        acc = (acc.double() + t.double() * t.double()).float() if square else acc + t
    return acc


def _xor_tree(a: torch.Tensor, lanes: int) -> torch.Tensor:
    """v += shfl_xor(v, o) for o = lanes / 2 ... 1 over the last axis; every lane ends with the same sum."""
    idx = torch.arange(lanes)
    o = lanes // 2
    while o > 0:
        a = a + a[..., idx ^ o]
        o //= 2
    return a[..., 0]


def _rownorm_emul(c: Case, fault: Optional[str] = None):
    d = inputs(c)
    NPER, LPR = route(c.D)
    M, D, Wd = c.M, c.D, NPER * LPR * 8
    x = d["x"].float()
    pad = torch.zeros(M, Wd)
    pad[:, :D] = x
    ok = torch.zeros(Wd, dtype=torch.bool)
    ok[:D] = True
    if fault == "lanes_past_end":                                # the clamped loads (chunk 0) enter the sums
        pad.view(M, Wd // 8, 8)[:, D // 8:] = x[:, None, :8]
        ok[:] = True

    def lanes(t):
        return t.reshape(-1, NPER, LPR, 8).permute(0, 2, 1, 3).reshape(-1, LPR, NPER * 8)

    div = torch.tensor(float(Wd if fault == "var_padded_width" else D), dtype=torch.float32)
    okl = lanes(ok[None].expand(1, Wd))
    if c.op == "rmsnorm":
        mean = torch.zeros(M, 1)
        ss = _xor_tree(_seq_sum(lanes(pad), True), LPR)
        rstd = torch.rsqrt(ss / div + torch.tensor(RMS_EPS, dtype=torch.float32))
    else:
        s = _xor_tree(_seq_sum(lanes(pad), False), LPR)
        mean = (s / torch.tensor(float(D), dtype=torch.float32))[:, None]
        dv = torch.where(okl, lanes(pad) - mean[:, :, None], torch.zeros(()))
        q = _xor_tree(_seq_sum(dv, True), LPR)
        rstd = torch.rsqrt(q / div + torch.tensor(LN_EPS, dtype=torch.float32))
    rstd = rstd[:, None]
    if fault == "pair_stats" and LPR == 32 and M > 1:            # the wave's second row with the first row's statistics
        n2 = M // 2
        rstd[1::2] = rstd[0:2 * n2:2]
        mean[1::2] = mean[0:2 * n2:2]
    w, b = d["w"].float(), d["b"].float()
    if c.op == "rmsnorm":
        inner = x * rstd
        y = w * (inner if fault == "rms_no_inner_round" else rb(inner))
    else:
        y = (((x - mean) * rstd).double() * w.double() + b.double()).float()
    return rb(y), rstd[:, 0]


FAULTS["rownorm"] = {
    "lanes_past_end": "lanes past nchunk included in the sums",
    "var_padded_width": "variance divided by the padded width",
    "pair_stats": "second row of a wave pair uses the first row's statistics",
    "rms_no_inner_round": "RMSNorm without the inner bf16 rounding (bitwise: see the module docstring)",
}


# ---------------------------------------------------------------------------------------------------------------------------------------
# groupnorm_tokens
# ---------------------------------------------------------------------------------------------------------------------------------------
GN_TOK = 256


def _groupnorm_cases() -> List[Case]:
    shapes = [(1, 256, 32), (255, 256, 32), (256, 256, 32), (257, 256, 32), (513, 64, 4), (300, 128, 2), (40, 8, 1)]
    out = [Case("groupnorm", f"gn-s{S}-c{C}-g{G}", S=S, C=C, G=G, ldx=C) for S, C, G in shapes]
    out.append(Case("groupnorm", "gn-s257-c256-g32-strided", S=257, C=256, G=32, ldx=264))
    return out


def _groupnorm_build(c: Case) -> dict:
    S, C, G = c.S, c.C, c.G
    cg = C // G
    g = _gen(S, C, G, 5)
    x = torch.randn(S, G, cg, generator=g)
    gi = torch.arange(G, dtype=torch.float64)
    scale = 0.25 * 16.0 ** ((gi * 7 % G) / max(G - 1, 1))                     # [0.25, 4], both ends when G > 1
    mean = 16.0 * scale * (torch.linspace(-1, 1, G, dtype=torch.float64) if G > 1 else torch.ones(1, dtype=torch.float64))
    x = (x.double() * scale[None, :, None] + mean[None, :, None])
    if S > 1:
        x[-1] = (mean + 3 * scale)[:, None]                                    # the last token: what a dropped last chunk loses
    const = G // 2 if G > 1 else None
    tiny = 1 if G >= 4 else None
    if const is not None:
        x[:, const] = 0.75
    if tiny is not None:
        x[:, tiny] = torch.where(torch.rand(S, cg, generator=g) < 0.5, -1.0, 1.0).double() * 2.0 ** -9
    w = (1 + 0.25 * torch.randn(C, generator=g)).to(BF)
    b = (0.25 * torch.randn(C, generator=g)).to(BF)
    return dict(x=x.reshape(S, C).to(BF), w=w, b=b, const=const, tiny=tiny)


def _groupnorm_stats64(c: Case):
    d = inputs(c)
    x = d["x"].double().view(c.S, c.G, c.C // c.G)
    mean = x.mean(dim=(0, 2), keepdim=True)
    var = (x - mean).pow(2).mean(dim=(0, 2), keepdim=True)
    return x, mean, 1.0 / torch.sqrt(var + GN_EPS)


def _groupnorm_ref(c: Case) -> torch.Tensor:
    d = inputs(c)
    x, mean, rstd = _groupnorm_stats64(c)
    return ((x - mean) * rstd).reshape(c.S, c.C) * d["w"].double() + d["b"].double()


def _groupnorm_bound(c: Case, quarter: bool = False) -> torch.Tensor:
    d = inputs(c)
    x, mean, rstd = _groupnorm_stats64(c)
    w = d["w"].double()
    stat = (REL["groupnorm"] * (0.25 if quarter else 1.0) * (x.abs() + mean.abs()) * rstd).reshape(c.S, c.C) * w.abs()
    v = ((x - mean) * rstd).reshape(c.S, c.C) * w
    out = v + d["b"].double()
    return rnd(stat + 3 * F32_EPS * v.abs() + F32_EPS * out.abs(), out)   # x - mean, . rstd, . w, + b: four fp32 roundings at most


def _groupnorm_emul(c: Case, fault: Optional[str] = None, fused: bool = False):
    d = inputs(c)
    S, C, G = c.S, c.C, c.G
    cg, per = C // G, C // G // 8
    x = d["x"].float()
    xg = x.view(S, G, cg)
    if fault == "next_group":
        xg = xg.roll(-1, dims=1)
    n_chunks = -(-S // GN_TOK)
    a = torch.zeros(G, dtype=torch.float32)
    bq = torch.zeros(G, dtype=torch.float32)
    for k in range(n_chunks - 1 if (fault == "drop_last_chunk" and n_chunks > 1) else n_chunks):
        t = xg[k * GN_TOK:(k + 1) * GN_TOK]                                     # [T, G, cg]: item i = (token, 16-byte piece)
        items = t.permute(1, 0, 2).reshape(G, -1, 8)
        R = -(-items.shape[1] // 256)
        padded = torch.zeros(G, R * 256, 8)
        padded[:, :items.shape[1]] = items
        lanes = padded.view(G, R, 256, 8).permute(0, 2, 1, 3).reshape(G, 256, R * 8)
        pa = _xor_tree(_seq_sum(lanes, False).view(G, 4, 64), 64)
        pb = _xor_tree(_seq_sum(lanes, True).view(G, 4, 64), 64)
        a = a + ((pa[:, 0] + pa[:, 1]) + (pa[:, 2] + pa[:, 3]))
        bq = bq + ((pb[:, 0] + pb[:, 1]) + (pb[:, 2] + pb[:, 3]))
    n = torch.tensor(float(S) * float(cg), dtype=torch.float32)
    mean = a / n
    e2 = bq / (n - 1 if fault == "unbiased" else n)
    if fault == "unbiased":
        var = ((e2.double() * (n.double() - 1) - mean.double() * mean.double() * n.double()) / (n.double() - 1)).float() if n > 1 else e2 * 0
    elif fused:
        var = (e2.double() - mean.double() * mean.double()).float()
    else:
        var = e2 - mean * mean
    var = var.clamp_min(0.0)
    eps = torch.tensor(GN_EPS, dtype=torch.float32)
    rstd = 1.0 / (torch.sqrt(var) + eps) if fault == "eps_outside" else torch.rsqrt(var + eps)
    y = (x.view(S, G, cg) - mean[None, :, None]) * rstd[None, :, None]
    y = y.reshape(S, C) * d["w"].float() + d["b"].float()
    return rb(y), rstd


FAULTS["groupnorm"] = {
    "unbiased": "unbiased variance",
    "eps_outside": "eps outside the sqrt",
    "drop_last_chunk": "last token chunk dropped from the statistics",
    "next_group": "group g read at (g + 1) cg",
}


# ---------------------------------------------------------------------------------------------------------------------------------------
# swin_window_partition / swin_window_reverse_add / patch_merge
# ---------------------------------------------------------------------------------------------------------------------------------------
def _swin_cases() -> List[Case]:
    out = []
    for op in ("partition", "reverse_add"):
        for ws in (7, 12):
            for shift in (0, ws // 2, ws - 1):
                for H, W in ((ws, ws), (ws + 1, 2 * ws - 1), (5, 3), (2 * ws, ws + 5)):
                    for C in (8, 96):
                        for B in (1, 3):
                            out.append(Case("swin", f"{op}-ws{ws}-s{shift}-{H}x{W}-c{C}-b{B}", op=op, ws=ws, shift=shift, H=H, W=W, C=C, B=B))
    return out


def _swin_dims(c: Case):
    nWy, nWx = -(-c.H // c.ws), -(-c.W // c.ws)
    return nWy, nWx, nWy * c.ws, nWx * c.ws


def _swin_build(c: Case) -> dict:
    nWy, nWx, Hp, Wp = _swin_dims(c)
    g = _gen(c.ws, c.shift, c.H, c.W, c.C, c.B)
    d = dict(x=grid_values((c.B * c.H * c.W, c.C), g))
    if c.op == "reverse_add":
        d["yw"] = grid_values((c.B * Hp * Wp, c.C), g)
    return d


def swin_partition64(x: torch.Tensor, c: Case) -> torch.Tensor:
    """The reference's zero-pad to the window multiple, torch.roll(-shift), view / permute partition -> [B nW ws ws, C]."""
    nWy, nWx, Hp, Wp = _swin_dims(c)
    ws = c.ws
    xp = torch.zeros(c.B, Hp, Wp, c.C, dtype=x.dtype)
    xp[:, :c.H, :c.W] = x.view(c.B, c.H, c.W, c.C)
    xp = torch.roll(xp, shifts=(-c.shift, -c.shift), dims=(1, 2))
    return xp.view(c.B, nWy, ws, nWx, ws, c.C).permute(0, 1, 3, 2, 4, 5).reshape(-1, c.C)


def swin_reverse64(yw: torch.Tensor, c: Case) -> torch.Tensor:
    """window_reverse, roll(+shift), crop to H x W -> [B H W, C]."""
    nWy, nWx, Hp, Wp = _swin_dims(c)
    ws = c.ws
    y = yw.view(c.B, nWy, nWx, ws, ws, c.C).permute(0, 1, 3, 2, 4, 5).reshape(c.B, Hp, Wp, c.C)
    y = torch.roll(y, shifts=(c.shift, c.shift), dims=(1, 2))
    return y[:, :c.H, :c.W].reshape(-1, c.C)


def _swin_ref(c: Case) -> torch.Tensor:
    d = inputs(c)
    if c.op == "partition":
        return swin_partition64(d["x"], c)
    return (swin_reverse64(d["yw"].float(), c) + d["x"].float()).to(BF)


def _swin_emul(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    """The kernels' index arithmetic."""
    d = inputs(c)
    nWy, nWx, Hp, Wp = _swin_dims(c)
    ws, H, W, B = c.ws, c.H, c.W, c.B
    nW = nWy * nWx
    shift = -c.shift if fault == "shift_sign" else c.shift
    wrapH, wrapW = (H, W) if fault == "wrap_unpadded" else (Hp, Wp)
    img_stride = Hp * Wp if fault == "image_stride_padded" else H * W
    x = d["x"]
    if c.op == "partition":
        row = torch.arange(B * nW * ws * ws)
        gwin, inw = row // (ws * ws), row % (ws * ws)
        img, win = gwin // nW, gwin % nW
        wy, wx = win // nWx, win % nWx
        if fault == "window_transposed":
            wy, wx = win % nWy, win // nWy
        iy, ix = inw // ws, inw % ws
        h, w = wy * ws + iy + shift, wx * ws + ix + shift
        h = torch.where(h >= wrapH, h - wrapH, h)
        w = torch.where(w >= wrapW, w - wrapW, w)
        h = torch.where(h < 0, h + wrapH, h)
        w = torch.where(w < 0, w + wrapW, w)
        inside = (h >= 0) & (w >= 0) & (h < H) & (w < W)
        src = (img * img_stride + h * W + w) % x.shape[0]
        return torch.where(inside[:, None], x[src], torch.zeros((), dtype=BF))
    pix = torch.arange(B * H * W)
    img, lp = pix // (H * W), pix % (H * W)
    h, w = lp // W, lp % W
    hs, wsft = h - shift, w - shift
    hs = torch.where(hs < 0, hs + wrapH, hs)
    wsft = torch.where(wsft < 0, wsft + wrapW, wsft)
    hs = torch.where(hs >= wrapH, hs - wrapH, hs)
    wsft = torch.where(wsft >= wrapW, wsft - wrapW, wsft)
    wy, wx = hs // ws, wsft // ws
    widx = wx * nWy + wy if fault == "window_transposed" else wy * nWx + wx
    base = img * (H * W // (ws * ws) + 1 if fault == "image_stride_padded" else nW)
    row = ((base + widx) * ws * ws + (hs % ws) * ws + (wsft % ws)) % d["yw"].shape[0]
    return (d["yw"][row].float() + x.float()).to(BF)


FAULTS["swin"] = {
    "shift_sign": "shift sign flipped",
    "wrap_unpadded": "wrap at H / W instead of Hp / Wp",
    "window_transposed": "wy / wx transposed",
    "image_stride_padded": "image stride taken from the other (padded / unpadded) size",
}


def _patch_merge_cases() -> List[Case]:
    return [Case("patch_merge", f"pm-{H}x{W}-c{C}-b{B}", H=H, W=W, C=C, B=B)
            for H, W in ((1, 1), (2, 2), (3, 5), (4, 7), (7, 4)) for C in (8, 96) for B in (1, 3)]


def _patch_merge_build(c: Case) -> dict:
    return dict(x=grid_values((c.B * c.H * c.W, c.C), _gen(c.H, c.W, c.C, c.B, 3)))


def _patch_merge_ref(c: Case) -> torch.Tensor:
    """PatchMerging: pad to even, cat(x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2])."""
    x = inputs(c)["x"].view(c.B, c.H, c.W, c.C)
    xp = torch.zeros(c.B, c.H + c.H % 2, c.W + c.W % 2, c.C, dtype=BF)
    xp[:, :c.H, :c.W] = x
    return torch.cat([xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2]], -1).reshape(-1, 4 * c.C)


def _patch_merge_emul(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    x = inputs(c)["x"]
    H, W, C, B = c.H, c.W, c.C, c.B
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    r = torch.arange(B * Ho * Wo * 4)
    q, r4 = r % 4, r // 4
    img, lp = r4 // (Ho * Wo), r4 % (Ho * Wo)
    oi, oj = lp // Wo, lp % Wo
    dh, dw = (q >> 1, q & 1) if fault == "quadrant_swapped" else (q & 1, q >> 1)
    h, w = 2 * oi + dh, 2 * oj + dw
    inside = (h < H) & (w < W)
    if fault == "edge_clamped":
        h, w, inside = h.clamp_max(H - 1), w.clamp_max(W - 1), torch.ones_like(inside)
    src = (img * H * W + h * W + w) % x.shape[0]
    return torch.where(inside[:, None], x[src], torch.zeros((), dtype=BF)).reshape(-1, 4 * C)


FAULTS["patch_merge"] = {"quadrant_swapped": "q & 1 and q >> 1 swapped", "edge_clamped": "odd edge clamped instead of zeroed"}


# ---------------------------------------------------------------------------------------------------------------------------------------
# sine_embed / box_refine
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sine_cases() -> List[Case]:
    return [Case("sine_embed", f"sine-d{dims}-n{n}-ld{ld}", dims=dims, n=n, ld=ld) for dims in (2, 4) for n in (1, 257) for ld in (dims, dims + 3)]


def _sine_build(c: Case) -> dict:
    g = _gen(c.dims, c.n, c.ld, 17)
    ref = torch.rand(c.n, c.dims, generator=g)
    special = torch.tensor([[0.0, 1.0, 0.5, 0.25], [1.0, 0.5, 0.0, 0.75], [0.5, 0.0, 1.0, 0.125]])[:, :c.dims]
    ref[:min(3, c.n)] = special[:min(3, c.n)]
    buf = framed(ref, c.ld, 0)
    return dict(ref=ref, buf=buf)


def _sine_ref(c: Case) -> torch.Tensor:
    ref = inputs(c)["ref"].double()
    j = torch.arange(128)
    dim_t = 10000.0 ** (2.0 * (j // 2).double() / 128.0)
    blocks = []
    for src in ([1, 0, 2, 3][:c.dims]):
        a = ref[:, src, None] * (2.0 * math.pi) / dim_t
        blocks.append(torch.where(j % 2 == 1, torch.cos(a), torch.sin(a)))
    return torch.cat(blocks, -1)


def _sine_chain32(c: Case, fault: Optional[str] = None) -> np.ndarray:
    ref = inputs(c)["ref"].numpy().astype(np.float32)
    j = np.arange(128)
    ex = (j if fault == "exponent_unpaired" else 2 * (j // 2)).astype(np.float32) / np.float32(128.0)
    dim_t = np.power(np.float32(10000.0), ex, dtype=np.float32)
    order = [0, 1, 2, 3][:c.dims] if fault == "blocks_not_swapped" else [1, 0, 2, 3][:c.dims]
    odd = (j % 2 == 0) if fault == "parity_swapped" else (j % 2 == 1)
    blocks = []
    for src in order:
        a = (ref[:, src, None] * np.float32(6.283185307179586)) / dim_t
        blocks.append(np.where(odd, np.cos(a, dtype=np.float32), np.sin(a, dtype=np.float32)))
    return np.concatenate(blocks, -1).astype(np.float32)


def _sine_emul(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    return rb(torch.from_numpy(_sine_chain32(c, fault)))


def _sine_bound(c: Case, quarter: bool = False) -> torch.Tensor:
    t = SINE_T * (0.25 if quarter else 1.0)
    return rnd(torch.full_like(_sine_ref(c), t), _sine_ref(c))


FAULTS["sine_embed"] = {"blocks_not_swapped": "x / y blocks not swapped", "parity_swapped": "sin / cos parity swapped",
                        "exponent_unpaired": "exponent j / 128 instead of 2 floor(j / 2) / 128"}


def _box_cases() -> List[Case]:
    return [Case("box_refine", f"box-m{mode}-n{n}-{'strided' if s else 'contig'}", mode=mode, n=n, strided=s,
                 ldd=6 if s else 4, ldr=5 if s else 4, ldo=7 if s else 4) for mode in (0, 1, 2) for n in (1, 65) for s in (False, True)]


def _box_build(c: Case) -> dict:
    g = _gen(c.mode, c.n, int(c.strided), 23)
    delta = (torch.rand(c.n, 4, generator=g) * 24 - 12)
    delta.view(-1)[:2] = torch.tensor([-12.0, 12.0])
    if c.mode == 0:
        ref = torch.rand(c.n, 4, generator=g)
        sp = torch.tensor([0.0, 1.0, 1e-4, 1 - 1e-4, -0.01, 1.02, 1e-3, 0.999])
        ref.view(-1)[:min(sp.numel(), ref.numel())] = sp[:ref.numel()] if ref.numel() < sp.numel() else sp
        if c.n > 1:
            delta.view(-1)[8:16] = torch.tensor([12.0, -12.0, -12.0, 12.0, 3.0, -3.0, 12.0, -12.0])     # both tails on both clamps
            ref.view(-1)[8:16] = torch.tensor([0.0, 1.0, 1e-4, 1 - 1e-4, -0.01, 1.02, 0.0, 0.0])
    else:
        ref = torch.randn(c.n, 4, generator=g) * 3                # logits
        if c.mode == 1 and c.n > 1:
            ref[3] = float("inf")
            ref[c.n - 1] = float("inf")
        if c.mode == 1 and c.n == 1:
            ref[0, 2:] = float("inf")
    return dict(delta=delta, ref=ref, delta_buf=framed(delta, c.ldd, 0), ref_buf=framed(ref, c.ldr, 0))


def inverse_sigmoid64(x: torch.Tensor, eps: float = BOX_EPS) -> torch.Tensor:
    x = x.clamp(0.0, 1.0)
    return torch.log(x.clamp_min(eps) / (1.0 - x).clamp_min(eps))


def _box_ref(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    d = inputs(c)
    delta, ref = d["delta"].double(), d["ref"].double()
    if c.mode == 0:
        return 1.0 / (1.0 + torch.exp(-(delta + inverse_sigmoid64(ref))))
    if c.mode == 1:
        return delta + ref
    return 1.0 / (1.0 + torch.exp(-(delta + ref)))


def _box_emul(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    d = inputs(c)
    dl, r = d["delta"].numpy().astype(np.float32), d["ref"].numpy().astype(np.float32)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        if c.mode == 0:
            eps = np.float32(1e-5 if fault == "eps_1e-5" else 1e-3)
            x = r if fault == "no_clamp" else np.minimum(np.maximum(r, np.float32(0.0)), one)
            u = dl + np.log(np.maximum(x, eps) / np.maximum(one - x, eps), dtype=np.float32)
            out = one / (one + np.exp(-u, dtype=np.float32))
        elif c.mode == 1:
            out = dl + r
        else:
            out = one / (one + np.exp(-(dl + r), dtype=np.float32))
    return torch.from_numpy(out.astype(np.float32))


def _box_bound(c: Case, quarter: bool = False) -> torch.Tensor:
    s = 0.5 if quarter else 1.0          # 8 x the measured chain: the emulation (that chain) is held to half, i.e. 4 x
    ref = _box_ref(c)
    return torch.where(torch.isfinite(ref), s * (BOX_REL * ref.abs() + BOX_ABS), torch.zeros_like(ref))


FAULTS["box_refine"] = {"eps_1e-5": "eps 1e-5", "no_clamp": "no clamp to [0, 1]"}


# ---------------------------------------------------------------------------------------------------------------------------------------
# topk_desc / argmax
# ---------------------------------------------------------------------------------------------------------------------------------------
def _topk_cases() -> List[Case]:
    return [Case("topk", f"topk-n{n}-k{k}-s{s}", n=n, k=k, stride=s) for n, k, s in ((1, 1, 1), (2, 2, 1), (5, 3, 2), (1024, 1024, 1), (1025, 7, 1), (2049, 900, 8))]


def _topk_build(c: Case) -> dict:
    n, s = c.n, c.stride
    g = _gen(n, c.k, s, 29)
    levels = torch.tensor([-1.5, 0.0, 0.5, 2.0, 3.0])
    v = levels[torch.randint(0, 5, (n,), generator=g)]
    if n == 2:
        v = torch.tensor([-0.0, 0.0])
    if n >= 5:
        v[0], v[1], v[n - 1] = -0.0, 0.0, -0.0                    # -0.0 at the lower index, another behind every +0.0
        v[2] = float("inf") if n > 5 else 3.0
    if n >= 1024:
        v[7], v[n - 2] = float("inf"), float("inf")
        v[5], v[n - 3] = float("-inf"), float("-inf")
        v[100:108] = float("nan")                                   # one NaN block
        v[n // 2], v[n // 2 + 1] = -0.0, 0.0
    flat = torch.full((n * s,), 1e30)                               # a kernel that ignores the stride meets these
    flat[::s] = v
    return dict(scores=flat, v=v.clone())


def _topk_ref(c: Case) -> torch.Tensor:
    """Stable sort by (value descending, index ascending), NaN last: torch's stable sort of the negated scores (NaN compares greatest)."""
    v = inputs(c)["v"].double()
    return torch.sort(-v, stable=True).indices[:c.k]


def _f32_order(u: np.ndarray, fixed: bool = True, nan_first: bool = False) -> np.ndarray:
    u = u.astype(np.uint32)
    if fixed:
        u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    return np.where(nan, np.uint32(0xffffffff if nan_first else 0), key)


def _topk_emul(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    d = inputs(c)
    s = 1 if fault == "stride_ignored" else c.stride
    vals = d["scores"].numpy()[:c.n * s:s][:c.n]
    key = _f32_order(vals.view(np.uint32), fixed=fault != "signed_zero_keys", nan_first=fault == "nan_first").astype(np.uint64)
    i = np.arange(c.n, dtype=np.uint32)
    low = (i if fault == "ties_higher_index" else ~i).astype(np.uint64)
    words = np.sort((key << np.uint64(32)) | low)[::-1][:c.k]
    idx = (words & np.uint64(0xffffffff)).astype(np.uint32)
    idx = idx if fault == "ties_higher_index" else ~idx
    return torch.from_numpy(idx.astype(np.int64))


FAULTS["topk"] = {"ties_higher_index": "ties to the higher index", "nan_first": "NaN first", "stride_ignored": "stride ignored",
                  "signed_zero_keys": "+0.0 and -0.0 with different keys (f32_order before the fix)"}


ARGMAX_N = (1, 63, 1024, 1025, 16383, 16384, 16385, 20000)
ARGMAX_SLICES = 128


def argmax_route(n: int) -> str:
    """fo1_argmax_bf16 with a scratch buffer: one workgroup below 16384 elements, 128 slices + a final launch from there."""
    return "one" if n < 16384 else "two"


def _argmax_cases() -> List[Case]:
    out = []
    for n in ARGMAX_N:
        per = -(-n // ARGMAX_SLICES)
        kinds = {"first": [0], "last": [n - 1], "all_equal": None, "neg_inf_but_one": [n // 3]}
        if argmax_route(n) == "two":
            kinds["across_slices"] = [per - 1, per]
            kinds["far_apart"] = [3 * per + 5, n - 7]
            kinds["last_slice_start"] = [(-(-n // per) - 1) * per, n - 1]
        for kind, pos in kinds.items():
            if n == 1 and kind != "first":
                continue
            out.append(Case("argmax", f"argmax-n{n}-{kind}", n=n, kind=kind, pos=pos))
    return out


def _argmax_build(c: Case) -> dict:
    g = _gen(c.n, len(c.kind), 31)
    row = (torch.randn(c.n, generator=g).clamp(-4, 4)).to(BF)
    if c.kind == "all_equal":
        row[:] = 1.5
    elif c.kind == "neg_inf_but_one":
        row[:] = float("-inf")
        row[c.pos[0]] = -3.0
    else:
        for p in c.pos:
            row[p] = 8.0
    return dict(row=row)


def _argmax_ref(c: Case) -> torch.Tensor:
    v = inputs(c)["row"].double()
    return (v == v.max()).nonzero()[0, 0].reshape(1)


def _argmax_emul(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    v = inputs(c)["row"].float()

    def pick(lo, hi):
        if hi <= lo:
            return float("-inf"), 0x7fffffff
        s = v[lo:hi]
        hit = (s == s.max()).nonzero()[:, 0]
        return s.max().item(), lo + int(hit[-1] if fault == "last_tie" else hit[0])

    if argmax_route(c.n) == "one":
        return torch.tensor([pick(0, c.n)[1]])
    per = -(-c.n // ARGMAX_SLICES)
    parts = [pick(b * per, min(c.n, b * per + per - (1 if fault == "slice_off_by_one" else 0))) for b in range(ARGMAX_SLICES)]
    best = max(p[0] for p in parts)
    cands = [p[1] for p in parts if p[0] == best]
    return torch.tensor([max(cands) if fault == "last_tie" else min(cands)])


FAULTS["argmax"] = {"last_tie": "last index among ties", "slice_off_by_one": "slice boundary off by one"}


# ---------------------------------------------------------------------------------------------------------------------------------------
# add / bias_act / swiglu / mask_rows / gather_rows_f32
# ---------------------------------------------------------------------------------------------------------------------------------------
ELT_SHAPES = ((1, 8), (33, 24), (300, 640))


def _eltwise_cases() -> List[Case]:
    out = []
    for M, D in ELT_SHAPES:
        for s in (False, True):
            tag = f"m{M}-d{D}-{'strided' if s else 'contig'}"
            out.append(Case("eltwise", f"add-{tag}", op="add", M=M, D=D, strided=s, lda=D + 8 * s, ldb=D + 16 * s, ldy=D + 24 * s))
            for act, bias in ((0, True), (1, False), (1, True)):
                out.append(Case("eltwise", f"bias_act-a{act}b{int(bias)}-{tag}", op="bias_act", M=M, D=D, strided=s, act=act, bias=bias,
                                ldx=D + 8 * s, ldy=D + 16 * s))
            out.append(Case("eltwise", f"swiglu-{tag}", op="swiglu", M=M, D=D, strided=s, ldgu=2 * D + 8 * s, ldy=D + 16 * s))
            out.append(Case("eltwise", f"mask_rows-{tag}", op="mask_rows", M=M, D=D, strided=s, ldx=D + 8 * s))
            out.append(Case("eltwise", f"gather_rows-{tag}", op="gather_rows", M=M, D=D, strided=s, ldt=D + 3 * s))
    return out


def _eltwise_build(c: Case) -> dict:
    M, D = c.M, c.D
    g = _gen(M, D, len(c.name), 37)
    if c.op == "add":
        return dict(a=grid_values((M, D), g), b=grid_values((M, D), g))
    if c.op == "bias_act":
        x = (torch.randn(M, D, generator=g) * 1.5).to(BF)
        return dict(x=x, bias=torch.randn(D, generator=g).to(BF) if c.bias else None)
    if c.op == "swiglu":
        return dict(gu=(torch.randn(M, 2 * D, generator=g) * 2).to(BF))
    if c.op == "mask_rows":
        keep = torch.tensor([0, 2, 255, 1, 0, 128, 7], dtype=torch.uint8).repeat(-(-M // 7))[:M].contiguous()
        return dict(x=torch.randn(M, D, generator=g).to(BF), keep=keep)
    T = M + 5
    table = torch.randn(T, D, generator=g)
    idx = torch.arange(T - 1, T - 1 - M, -1, dtype=torch.int32)                      # descending ...
    idx[M // 2:] = idx[:M - M // 2].clone() if M > 1 else idx[M // 2:]             # ... and repeated
    return dict(table=table, idx=idx.contiguous())


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))


def _eltwise_ref(c: Case) -> torch.Tensor:
    d = inputs(c)
    if c.op == "add":
        return (d["a"].float() + d["b"].float()).to(BF)
    if c.op == "bias_act":
        v = d["x"].double() + (d["bias"].double() if c.bias else 0.0)
        return _gelu64(v) if c.act == 1 else v
    if c.op == "swiglu":
        g, u = d["gu"][:, :c.D].double(), d["gu"][:, c.D:].double()
        return g * torch.sigmoid(g) * u
    if c.op == "mask_rows":
        return torch.where((d["keep"] != 0)[:, None], d["x"], torch.zeros((), dtype=BF))
    return d["table"][d["idx"].long()]


def _eltwise_bound(c: Case, quarter: bool = False) -> Optional[torch.Tensor]:
    d = inputs(c)
    if c.op in ("add", "mask_rows", "gather_rows"):
        return None
    if c.op == "bias_act":
        v = d["x"].double() + (d["bias"].double() if c.bias else 0.0)
        e = rnd(F32_EPS * v.abs(), v) if c.bias else torch.zeros_like(v)
        if c.act == 0:
            return e if c.bias else None
        out = _gelu64(v)
        return rnd(GELU_SLOPE * e + 3.2e-7 * v.abs() + 2 * F32_EPS * out.abs(), out)
    g, u = d["gu"][:, :c.D].double(), d["gu"][:, c.D:].double()
    s = g * torch.sigmoid(g)
    e1 = rnd((g.abs() + 4.0) * F32_EPS * s.abs(), s)
    return rnd(u.abs() * e1, s * u)


def _eltwise_emul(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    d = inputs(c)
    if c.op == "add":
        return (d["a"].float() + d["b"].float()).to(BF)
    if c.op == "bias_act":
        f = d["x"].float()
        if c.bias:
            f = rb(f + d["bias"].float())
        if c.act == 1:
            x = f * 0.70710678118654752440
            ax = x.abs()
            t = 1.0 / (0.3275911 * ax + 1.0)
            poly = 1.061405429 * t - 1.453152027
            for k in (1.421413741, -0.284496736, 0.254829592):
                poly = poly * t + k
            e = poly * t * torch.exp(-ax * ax)
            f = 0.5 * f * torch.where(x >= 0, 2.0 - e, e)
        return f.to(BF) if (c.bias or c.act) else d["x"]
    if c.op == "swiglu":
        g, u = d["gu"][:, :c.D].float(), d["gu"][:, c.D:].float()
        return rb(rb(g * (1.0 / (1.0 + torch.exp(-g)))) * u)
    if c.op == "mask_rows":
        keep = (d["keep"] == 1) if fault == "keep_is_one" else (d["keep"] != 0)
        return torch.where(keep[:, None], d["x"], torch.zeros((), dtype=BF))
    return d["table"][d["idx"].long()]


FAULTS["eltwise"] = {"keep_is_one": "mask_rows keeps only bytes equal to 1"}


# ---------------------------------------------------------------------------------------------------------------------------------------
# patchify_u8 / normalize_u8
# ---------------------------------------------------------------------------------------------------------------------------------------
def _preprocess_cases() -> List[Case]:
    out = [Case("preprocess", f"patchify-{H}x{W}-ld{ld}", op="patchify", H=H, W=W, ld=ld) for H, W in ((28, 28), (28, 56), (56, 28)) for ld in (1176, 1184)]
    out += [Case("preprocess", f"normalize-{H}x{W}", op="normalize", H=H, W=W) for H, W in ((1, 1), (3, 7), (5, 8), (2, 17))]
    return out


def _preprocess_build(c: Case) -> dict:
    g = _gen(c.H, c.W, 41)
    img = torch.randint(0, 256, (c.H, c.W, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    lut = torch.stack([(0x100 + ch * 256 + torch.randperm(256, generator=g)) for ch in range(3)]).to(torch.int16).view(BF)   # injective, all finite
    return dict(img=img, lut=lut)


def _preprocess_ref(c: Case) -> torch.Tensor:
    """preprocess.hip's layout comment, as numpy index arithmetic (bit patterns)."""
    d = inputs(c)
    img, lut = d["img"].numpy(), d["lut"].view(torch.int16).numpy()
    H, W = c.H, c.W
    if c.op == "normalize":
        out = np.zeros((3, H, W), dtype=np.int16)
        for ch in range(3):
            out[ch] = lut[ch][img[:, :, ch]]
        return torch.from_numpy(out).view(BF)
    P, m = 14, 2
    gh, gw = H // P, W // P
    gwm = gw // m
    out = np.zeros((gh * gw, 6 * P * P), dtype=np.int16)
    for row in range(gh * gw):
        dx, dy, blk = row % m, (row // m) % m, row // (m * m)
        py, px = (blk // gwm) * m + dy, (blk % gwm) * m + dx
        for ch in range(3):
            patch = lut[ch][img[py * P:(py + 1) * P, px * P:(px + 1) * P, ch]].reshape(-1)
            for t in range(2):
                out[row, ch * 2 * P * P + t * P * P:ch * 2 * P * P + (t + 1) * P * P] = patch
    return torch.from_numpy(out).view(BF)


def _preprocess_emul(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    """The kernels' flat index walk."""
    d = inputs(c)
    img, lut = d["img"].long(), d["lut"].view(torch.int16)
    H, W = c.H, c.W
    if c.op == "normalize":
        cc, y, x = torch.meshgrid(torch.arange(3), torch.arange(H), torch.arange(W), indexing="ij")
        return lut[cc, img[y, x, cc]].view(BF)
    P, m = 14, 2
    gh, gw = H // P, W // P
    gwm = gw // m
    row, cc, t, y, x = torch.meshgrid(torch.arange(gh * gw), torch.arange(3), torch.arange(2), torch.arange(P), torch.arange(P), indexing="ij")
    dx, dy, blk = row % m, (row // m) % m, row // (m * m)
    if fault == "merge_transposed":
        dx, dy = dy, dx
    py, px = (blk // gwm) * m + dy, (blk % gwm) * m + dx
    return lut[cc, img[py * P + y, px * P + x, cc]].reshape(gh * gw, 6 * P * P).view(BF)


FAULTS["preprocess"] = {"merge_transposed": "dx / dy of the merge block swapped"}


# ---------------------------------------------------------------------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------------------------------------------------------------------
CASES.update(rownorm=_rownorm_cases(), groupnorm=_groupnorm_cases(), swin=_swin_cases(), patch_merge=_patch_merge_cases(), sine_embed=_sine_cases(),
             box_refine=_box_cases(), topk=_topk_cases(), argmax=_argmax_cases(), eltwise=_eltwise_cases(), preprocess=_preprocess_cases())
ALL_CASES: List[Case] = [c for fam in CASES.values() for c in fam]
_BUILD: Dict[str, Callable] = dict(rownorm=_rownorm_build, groupnorm=_groupnorm_build, swin=_swin_build, patch_merge=_patch_merge_build,
                                   sine_embed=_sine_build, box_refine=_box_build, topk=_topk_build, argmax=_argmax_build, eltwise=_eltwise_build,
                                   preprocess=_preprocess_build)
_REF: Dict[str, Callable] = dict(rownorm=_rownorm_ref, groupnorm=_groupnorm_ref, swin=_swin_ref, patch_merge=_patch_merge_ref, sine_embed=_sine_ref,
                                 box_refine=_box_ref, topk=_topk_ref, argmax=_argmax_ref, eltwise=_eltwise_ref, preprocess=_preprocess_ref)
_BOUND: Dict[str, Callable] = dict(rownorm=_rownorm_bound, groupnorm=_groupnorm_bound, sine_embed=_sine_bound, box_refine=_box_bound,
                                   eltwise=_eltwise_bound)
_EMUL: Dict[str, Callable] = dict(rownorm=lambda c, f=None: _rownorm_emul(c, f)[0], groupnorm=lambda c, f=None: _groupnorm_emul(c, f)[0],
                                  swin=_swin_emul, patch_merge=_patch_merge_emul, sine_embed=_sine_emul, box_refine=_box_emul, topk=_topk_emul,
                                  argmax=_argmax_emul, eltwise=_eltwise_emul, preprocess=_preprocess_emul)


def reference(c: Case) -> torch.Tensor:
    return _REF[c.family](c)


def bound(c: Case, quarter: bool = False) -> Optional[torch.Tensor]:
    """Per-element bound, or None for a bit-exact op.  quarter: the statistics / chain term at a quarter (what the emulation is held to)."""
    return _BOUND[c.family](c, quarter) if c.family in _BOUND else None


def emulate(c: Case, fault: Optional[str] = None) -> torch.Tensor:
    return _EMUL[c.family](c, fault)


def route_label(c: Case) -> str:
    """The '<op> <route>' under which the GPU sweep reports a case."""
    if c.family == "rownorm":
        return f"{c.op} ({route(c.D)[0]},{route(c.D)[1]})"
    if c.family == "argmax":
        return f"argmax {argmax_route(c.n)}"
    if c.family == "groupnorm":
        return f"groupnorm cg{c.C // c.G}"
    if c.family in ("swin", "eltwise", "preprocess"):
        return f"{c.op} -"
    if c.family == "box_refine":
        return f"box_refine mode{c.mode}"
    return f"{c.family} -"


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor) -> Tuple[float, int]:
    """max |got - ref| / bound (inf where a non-finite reference is not met exactly) and its flat position."""
    got, ref = got.double(), ref.double()
    fin = torch.isfinite(ref)
    diff = torch.where(fin, (got - torch.where(fin, ref, torch.zeros_like(ref))).abs(), torch.zeros_like(ref))
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bnd.clamp_min(1e-300))
    ratio = torch.where(fin, ratio, torch.where(got == ref, torch.zeros_like(ratio), torch.full_like(ratio, float("inf"))))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    return ratio.max().item(), int(ratio.flatten().argmax())


def measure() -> Dict[str, float]:
    """The measured quantities the constants are set from (tests/test_small_op_cases.py::test_zz_summary prints them)."""
    m = {"rmsnorm": 0.0, "layernorm": 0.0, "groupnorm": 0.0, "sine": 0.0, "box_rel": 0.0, "box_abs": 0.0}
    for c in CASES["rownorm"]:
        if c.op == "layernorm_rows":
            continue
        r64 = _rownorm_stats64(c)[2][:, 0]
        r32 = _rownorm_emul(c)[1].double()
        m[c.op] = max(m[c.op], ((r32 - r64).abs() / r64).max().item())
    for c in CASES["groupnorm"]:
        r64 = _groupnorm_stats64(c)[2].flatten()
        for fused in (False, True):
            r32 = _groupnorm_emul(c, fused=fused)[1].double()
            m["groupnorm"] = max(m["groupnorm"], ((r32 - r64).abs() / r64).max().item())
    for c in CASES["sine_embed"]:
        m["sine"] = max(m["sine"], (torch.from_numpy(_sine_chain32(c)).double() - _sine_ref(c)).abs().max().item())
    for c in CASES["box_refine"]:
        ref, got = _box_ref(c), _box_emul(c).double()
        fin = torch.isfinite(ref)
        err = (got[fin] - ref[fin]).abs()
        m["box_rel"] = max(m["box_rel"], (err / ref[fin].abs().clamp_min(1e-300)).max().item())
        small = ref[fin].abs() < 2.0 ** -10
        if small.any():
            m["box_abs"] = max(m["box_abs"], err[small].max().item())
    return m


# ---------------------------------------------------------------------------------------------------------------------------------------
# the row norms for other case modules (tests/fp8_cases.py: fo1_rmsnorm_quant_e4m3 is RMSNorm + quantiser)
# ---------------------------------------------------------------------------------------------------------------------------------------
gen, seq_sum, xor_tree = _gen, _seq_sum, _xor_tree


def rownorm_case(name: str, op: str, x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None, **p) -> Case:
    """A rownorm case over the caller's own rows x [M, D] (bf16), weight and bias; rownorm_reference / _bound / _emulate then serve it."""
    M, D = x.shape
    c = Case("rownorm", name, op=op, D=D, M=M, **p)
    _INPUTS[name] = dict(x=x, w=w, b=torch.zeros(D, dtype=BF) if b is None else b)
    return c


def rownorm_reference(c: Case) -> torch.Tensor:
    return _rownorm_ref(c)


def rownorm_bound(c: Case, quarter: bool = False) -> torch.Tensor:
    return _rownorm_bound(c, quarter)


def rownorm_emulate(c: Case, fault: Optional[str] = None):
    """-> (bf16-valued output, rstd) of the kernel's arithmetic."""
    return _rownorm_emul(c, fault)
