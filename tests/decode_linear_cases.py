"""Cases, routing model, fp64 reference, emulated kernel arithmetic, per-element bound and faults of the decode-step linears:
gemv_mfma_kernel<MM, MODE, NB, MP, HALF, R8> (vlm_fo1_amd/csrc/decode_mfma.hip, behind fo1_gemv_batch_bf16 and fo1_gemv_attn_combine_bf16) and
gemv_kernel<MM, SWIGLU, KSPLIT> (csrc/gemv.hip, behind fo1_gemv_bf16 and the M <= 4 hand-off of fo1_gemm_bf16).  Shared by
tests/test_decode_linear_cases.py (CPU) and tests/test_decode_linears_gpu.py (the per-route sweep on the MI355X).  What can be shared with the
tile GEMM's sweep is imported from tests/gemm_route_cases.py (HALF_ULP, the activation slopes, _act64, _rnd, epilogue64, the canary patterns,
check_canary, _levels).

Routing model.  route_batch() restates gemv_b_any / gemv_mfma_any / dispatch_gemv_mfma / launch_gemv_mfma: (M, N, K, mode, fused norm, half
switch) -> Route(column class 8 / 16 / 32, weight rows per unit, NB, single- / multi-piece K, HALF / R8 / XREG / XR32, unit count, grid, k-steps
per staged piece) or "refused"; route_gemv() restates launch_gemv: MM in {1, 2, 4}, SWIGLU, KSPLIT (K >= 4096).  Route.label() is what SWEEP
claims for a case and what the coverage test enumerates (27 MFMA labels with the product defaults, 12 of gemv.hip, 4 refusals);
Route.shape_row() is the A/B library's profile row under fo1_gemm_profile_shapes(1), Route.product_row() the kernel name otherwise.

Operands (build()).  x ~ 0.5 N(0, 1) r_m, W ~ 0.05 N(0, 1) in bf16, r_m in {1, 2, 0.5}[m % 3] (x 0.25 for m >= 16: the second column group), so
that neighbouring sequences have rstd's 2 x or more apart.  PLANTED columns at k = 0, 7, 8, K - 1, both sides of the k-step boundaries 1 (wave 0 | 1),
8 (stage 0 | 1 of wave 0), 16 (the second pair of the 8-row units), every staged-piece boundary of the route, the first k-step of wave 0's last
stage, the last k-step (the K % 64 tail), and for gemv.hip the K-split wave ranges and the 64-chunk lane stride: x[m, k] = +-2 s_m / c,
W[n, k] = 0.5 t_n, c the planted positions in the 16-byte chunk, the sign alternating from planted chunk to planted chunk (they cancel
pairwise).  s_m = levels(m) r_m differs between m, m +- 1 and m +- 16; t_n = levels(n) x (0.5 if n // 8 odd) x (1.5 if n // 16 odd) differs
between rows r, r + 4, r + 8, r + 16 (and r + 64, the rotary partner, through the random part).  The norm weight is 1 at planted positions.
Bias: a ramp with a jump at every 4-, 8-, 16- and 32-feature boundary.  Residual: gemm_route_cases' pattern.  QKV: cache row 5 + 13 m, rope-table
row 300 - 7 m of tables with independent random angles per row, K-cache head stride and V^T row stride larger than needed.

Buffers (host_buffers()) are framed: NaN in x rows past M, W rows past N, the columns K..ld, after bias and norm weight; the canary bit
pattern in the output (ldc > n_out, SPARE_ROWS rows past M) and in the WHOLE K and V^T caches.

Reference and bound.  reference_and_bound() is float64 on the bf16 inputs with no intermediate rounding; the bound is one number per element:
  * every bf16 rounding point costs 2^-8 |value there|, earlier errors pass through later steps by their first-order slopes (epilogue64 for
    plain / SwiGLU / gemv.hip; QKV: bf16(acc + bias), bf16(a cos), bf16(-+ b sin), bf16 of their sum, V: bf16(acc + bias) only);
  * fused RMSNorm: two rounding points per x element (bf16(x rstd), bf16(w .)) and RSTD_REL |x rstd| for the fp32 rstd, carried to the output
    as sum_k |W[n, k]| e[m, k].  This worst-case term (every one of K elements off by half an ulp the same way) DOMINATES on normed routes: it
    is about sqrt(K) times what independent roundings give, so a normed case shows small fractions of its bound;
  * the fp32 accumulation costs ACC 2^-24 (|x| |W|^T + |bias|).  ACC is four times the emulation's measured worst (RESULTS_CPU), rounded up
    to a power of two.
emulate() restates each kernel's fp32 order.  MFMA kernel: two 32-element MFMA steps per k-step, k-steps wave + 8 d into chain A (d even) and B
(d odd), A + B, the fixed 8-wave tree.  gemv.hip: per-lane FMA chains over the chunks lane + 64 j of the wave's range, the 64-lane xor tree,
(w0 + w1) + (w2 + w3) under KSPLIT.  The fused norm: per-lane sums of squares, xor tree, rsqrt in fp32.

FAULTS / reference(d, fault): one unit, one sequence or one edge each; see FAULTS.  With PLANT = 0 the dropped k-step does NOT pass: under a
per-element bound 64 dropped random products are already hundreds of bounds on the small elements of a unit (measured: 395 x at p8-h-k2048,
176 x at p16-r-mp4160 without the planted columns, 1580 x and 175 x with them).  What the planted columns add is a contribution of known
size, +-s_m t_n, that does not depend on the draw; tests/test_decode_linear_cases.py prints both figures and asserts the planted one only.

What this makes redundant (kept as they are): the whole-output bounds 2e-2 max |ref| of tests/test_batched_decode_gpu.py::_gemv_batch_cases and
test_gemv_mfma_qkv_matches_reference_and_dot2 (MFMA half), and of tests/test_ops_gpu.py::test_gemv_* assert less, on the same kernels.

RESULTS_CPU (tests/test_decode_linear_cases.py -s; 108 launched cases, 22 s): emulation at most 0.995 of the bound (inside the sharp bound on
every case); accumulation error at most 1.537 x 2^-24 S, hence ACC = 8 >= 4 x 1.537; fp32 rstd at most 2.078 x 2^-24 relative, hence
RSTD_REL = 2^-20 >= 4 x 2.078 x 2^-24; the weakest fault moves its region by 2.01 x the bound (norm weight skipped, gemv.hip at a normed
K = 4096, where the norm term makes the bound about 1); 66 % of the (case, fault) pairs do not apply (most faults belong to one mode or
need the norm, a residual, M >= 2 ...), no route is without one.
RESULTS_GPU (MI355X, tests/test_decode_linears_gpu.py -s: 154 passed, 7.6 s; every bitwise claim holds at the edge shapes, 35 shapes bit-identical
across their column classes).  Worst |got - ref| / bound per route, product and A/B library alike (the same bits):
gemv mm1 plain ks0 0.738; gemv mm1 plain ks1 0.704; gemv mm1 swiglu ks0 0.264; gemv mm1 swiglu ks1 0.454; gemv mm2 plain ks0 0.265; gemv mm2 plain ks1
0.673; gemv mm2 swiglu ks0 0.454; gemv mm2 swiglu ks1 0.571; gemv mm4 plain ks0 0.732; gemv mm4 plain ks1 0.421; gemv mm4 swiglu ks0 0.455; gemv mm4
swiglu ks1 0.514; plain c16 u16 1p 0.992; plain c16 u16 mp 0.974; plain c16 u32 1p 0.992; plain c16 u32 mp 0.986; plain c16 u8 1p r 0.991; plain c16
u8 mp r 0.979; plain c32 u16 1p 0.992; plain c32 u16 mp 0.991; plain c32 u32 1p 0.995; plain c32 u8 1p r 0.995; plain c32 u8 mp r x 0.980; plain c8
u16 1p 0.981; plain c8 u16 mp 0.975; plain c8 u32 1p 0.989; plain c8 u32 mp 0.986; plain c8 u8 1p h 0.984; plain c8 u8 mp h 0.967; qkv c16 u16 1p r
0.964; qkv c16 u16 mp r 0.984; qkv c32 u16 1p r 0.993; qkv c8 u16 1p h 0.984; qkv c8 u16 mp h 0.939; swiglu c16 u32 1p 0.771; swiglu c16 u32 mp 0.502;
swiglu c32 u32 1p 0.774; swiglu c8 u32 1p 0.718; swiglu c8 u32 mp 0.711.
The MFMA routes sit at 0.94 - 0.995 of the bound because the bound is sharp by construction (the planted columns), not because the kernels are near
failing: the emulation reaches 0.995 too.  Still not measured: ACC on real MFMA hardware in isolation, and which cases the two hand-injected
arithmetic faults (xsel dropped in the HALF variant; R8 reading fragment row fi where it should read fi ^ 8) make fail."""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch

import gemm_route_cases as G
from gemm_route_cases import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SILU, ACT_SWIGLU, CANARY16, HALF_ULP, SPARE_OPERAND_ROWS, SPARE_ROWS,  # noqa: F401
                              _act64, _levels, _rnd, cdiv, check_canary, epilogue64)

PLAIN, SWIGLU, QKV = 0, 1, 2
MODE_NAME = {0: "plain", 1: "swiglu", 2: "qkv"}
ACC = 8.0                    # 4 x the emulation's measured worst accumulation error, rounded up to a power of two (RESULTS_CPU)
RSTD_REL = 2.0 ** -20        # the same for the fp32 rstd of the fused norm
NORM_EPS = 1e-6
PLANT = 1.0
CACHE_ROWS = 448             # cache rows 5 + 13 m, m < 32
TABLE_ROWS = 320             # rope-table rows 300 - 7 m
KC_EXTRA_ROWS, VT_EXTRA_COLS = 8, 12
M_LIST = (1, 2, 5, 8, 9, 13, 16, 17, 26, 27, 32)
CANARY_F = torch.tensor([CANARY16], dtype=torch.int16).view(torch.bfloat16).double().item()


# ---------------------------------------------------------------------------------------------------------------------------------------
# routing model
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Route:
    kind: str                # mfma | gemv | refused
    mode: int = 0            # mfma: PLAIN / SWIGLU / QKV
    cls: int = 0             # mfma: column class (MM) 8 / 16 / 32; gemv: MM 1 / 2 / 4
    rows: int = 0            # weight rows per unit
    NB: int = 0
    mp: bool = False         # multi-piece K
    half: bool = False
    r8: bool = False
    units: int = 0
    grid: int = 0
    psteps: int = 0          # k-steps of x per staged piece
    swiglu: bool = False     # gemv
    ksplit: bool = False     # gemv
    why: str = ""            # refused

    @property
    def xreg(self) -> bool:
        return self.kind == "mfma" and self.cls == 32 and not self.mp

    @property
    def xr32(self) -> bool:
        return self.kind == "mfma" and self.cls == 32 and self.mp and self.r8

    @property
    def h8(self) -> bool:
        return self.half or self.r8

    def label(self) -> str:
        if self.kind == "refused":
            return "refused " + self.why
        if self.kind == "gemv":
            return f"gemv mm{self.cls} {'swiglu' if self.swiglu else 'plain'} ks{int(self.ksplit)}"
        return (f"{MODE_NAME[self.mode]} c{self.cls} u{self.rows} {'mp' if self.mp else '1p'}" + (" h" if self.half else "") + (" r" if self.r8 else "")
                + (" x" if self.xr32 else ""))

    def shape_row(self, M: int, N: int, K: int, act: int = 0) -> str:
        if self.kind == "gemv":
            return f"gemv {M}x{N}x{K} a{act} ks{int(self.ksplit)}"
        flags = ("h" if self.half else "") + ("r" if self.r8 else "") + ("x" if self.xr32 else "") or "-"
        return f"gemv_mfma m{M} {N}x{K} mode{self.mode} u{self.rows} nb{self.NB} {'mp' if self.mp else '1p'} {flags}"

    def product_row(self) -> str:
        if self.kind == "gemv":
            return "gemv_bf16"
        return {PLAIN: "gemv_mfma", SWIGLU: "gemv_mfma_swiglu", QKV: "gemv_mfma_qkv"}[self.mode]


def _mfma(mode: int, cls: int, NB: int, units: int, nsteps: int, half: bool = False, r8: bool = False, force_1p: bool = False,
          force_mp: bool = False) -> Route:
    mp = force_mp or (nsteps > 32 and not force_1p)
    h8 = half or r8
    pd = 2 if r8 else (2 if (half and not mp) else (2 if (cls == 32 and mp) else 4))
    return Route("mfma", mode, cls, NB * (8 if h8 else 16), NB, mp, half, r8, units, min(units, 256), (16 if h8 else 8) * pd)


def route_batch(M: int, N: int, K: int, mode: int = PLAIN, norm: bool = False, half: int = 3, n_q: int = 0, n_kv: int = 0) -> Route:
    """fo1_gemv_batch_bf16 -> gemv_b_any -> gemv_mfma_any -> dispatch_gemv_mfma<MM> (quad-aligned operands: N % 4 == 0, ldr % 4 == 0)."""
    assert 1 <= M <= 32 and N % 4 == 0 and K % 8 == 0
    cls = 8 if M <= 8 else (16 if M <= 16 else 32)
    nsteps = cdiv(K, 64)
    if norm and nsteps > 32:
        return Route("refused", why="norm K>2048")
    if cls == 32 and nsteps > 32 and (mode != PLAIN or N >= 8192):
        return Route("refused", why=f"c32 K>2048 {MODE_NAME[mode] if mode != PLAIN else 'plain N>=8192'}")
    if mode == SWIGLU:
        return _mfma(SWIGLU, cls, 2, N // 32, nsteps)
    qkv_units8, qkv_units16 = (n_q + n_kv) * 8 + n_kv * 8, (n_q + n_kv) * 4 + n_kv * 4
    if cls == 8 and half & 1:
        if mode == QKV:
            return _mfma(QKV, 8, 2, qkv_units8, nsteps, half=True)
        if N <= 4096:
            return _mfma(PLAIN, 8, 1, cdiv(N, 8), nsteps, half=True)
    if cls == 16 and half & 2:
        if mode == QKV:
            return _mfma(QKV, 16, 2, qkv_units8, nsteps, r8=True)
        if N <= 4096:
            return _mfma(PLAIN, 16, 1, cdiv(N, 8), nsteps, r8=True)
    if cls == 32 and half & 2:
        if nsteps <= 32 and mode == QKV:
            return _mfma(QKV, 32, 2, qkv_units8, nsteps, r8=True, force_1p=True)
        if nsteps <= 32 and N <= 4096:
            return _mfma(PLAIN, 32, 1, cdiv(N, 8), nsteps, r8=True, force_1p=True)
        if nsteps > 32 and N <= 4096 and M <= 26 and not norm:
            return _mfma(PLAIN, 32, 1, cdiv(N, 8), nsteps, r8=True, force_mp=True)
    if mode == QKV:
        return _mfma(QKV, cls, 2, qkv_units16, nsteps)
    if N >= 8192:
        return _mfma(PLAIN, cls, 2, cdiv(N, 32), nsteps)
    return _mfma(PLAIN, cls, 1, cdiv(N, 16), nsteps)


def route_gemv(M: int, N: int, K: int, act: int = 0) -> Route:
    """fo1_gemv_bf16 / gemv_dispatch -> launch_gemv<MM> -> launch_gemv2<MM, SW, KS>."""
    assert 1 <= M <= 4 and K % 8 == 0
    mm = M if M <= 2 else 4
    sw, ks = act == ACT_SWIGLU, K >= 4096
    units = cdiv(N // 2 if sw else N, 4)
    return Route("gemv", cls=mm, rows=8 if sw else 4, units=units, grid=units if ks else cdiv(units, 4), swiglu=sw, ksplit=ks)


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    claim: str
    entry: str               # batch (fo1_gemv_batch_bf16) | gemv (fo1_gemv_bf16) | handoff (fo1_gemm_bf16, M <= 4) | combine (fo1_gemv_attn_combine_bf16)
    M: int
    N: int
    K: int
    mode: int = PLAIN
    act: int = 0             # gemv / handoff
    bias: bool = False
    res: bool = False
    norm: bool = False
    n_q: int = 0
    n_kv: int = 0
    ldx_pad: int = 0
    ldw_pad: int = 0
    ldc_pad: int = 8
    ldr_pad: int = 0
    seed: int = 0
    out_f32: bool = False    # (epilogue64 / check_canary read it)

    @property
    def n_out(self) -> int:
        if self.mode == QKV:
            return self.n_q * 128
        return self.N // 2 if (self.mode == SWIGLU or self.act == ACT_SWIGLU) else self.N

    @property
    def ldc(self) -> int:
        return self.n_out + self.ldc_pad

    @property
    def ldr(self) -> int:
        return self.N + self.ldr_pad

    @property
    def refused(self) -> bool:
        return self.claim.startswith("refused")


def case_route(c: Case) -> Route:
    if c.entry in ("gemv", "handoff"):
        return route_gemv(c.M, c.N, c.K, c.act)
    return route_batch(c.M, c.N, c.K, c.mode, c.norm, 3, c.n_q, c.n_kv)


def _c(name, claim, entry, M, N, K, **kw) -> Case:
    return Case(name, claim, entry, M, N, K, seed=len(name) * 131 + M + 7 * N + 13 * K, **kw)


def _b(name, claim, M, N, K, **kw) -> Case:
    return _c(name, claim, "batch", M, N, K, **kw)


def _q(name, claim, M, n_q, n_kv, K, **kw) -> Case:
    return _c(name, claim, "batch", M, (n_q + 2 * n_kv) * 128, K, mode=QKV, n_q=n_q, n_kv=n_kv, **kw)


def _g(name, claim, M, N, K, **kw) -> Case:
    return _c(name, claim, "gemv", M, N, K, **kw)


_FLAG = {8: " h", 16: " r", 32: " r"}
SWEEP: List[Case] = [
    # ---- plain, 8-row units (N <= 4096): 20 = last unit half valid; 2052 = 257 units (one workgroup owns two); 4092 = 512 units -------------
    _b("p8-h-k72", "plain c8 u8 1p h", 1, 20, 72, bias=True, res=True, ldr_pad=4),
    _b("p8-h-k264", "plain c8 u8 1p h", 2, 2052, 264, bias=True, ldx_pad=8),
    _b("p8-h-k2048", "plain c8 u8 1p h", 5, 4092, 2048, res=True, ldw_pad=8),
    _b("p8-h-oddldc", "plain c8 u8 1p h", 8, 20, 264, bias=True, res=True, ldc_pad=3),
    _b("p8-h-mp2112", "plain c8 u8 mp h", 8, 20, 2112, bias=True),
    _b("p8-h-mp4160", "plain c8 u8 mp h", 5, 2052, 4160, bias=True, res=True, ldx_pad=8),
    _b("p8-h-mp4288", "plain c8 u8 mp h", 8, 4092, 4288, res=True),
    _b("p16-r-k72", "plain c16 u8 1p r", 9, 20, 72, bias=True, res=True, ldr_pad=4),
    _b("p16-r-k264", "plain c16 u8 1p r", 13, 2052, 264, bias=True, ldx_pad=8),
    _b("p16-r-k2048", "plain c16 u8 1p r", 16, 4092, 2048, res=True, ldw_pad=8),
    _b("p16-r-mp2112", "plain c16 u8 mp r", 9, 20, 2112, bias=True),
    _b("p16-r-mp4160", "plain c16 u8 mp r", 13, 2052, 4160, bias=True, res=True),
    _b("p16-r-mp4288", "plain c16 u8 mp r", 16, 4092, 4288, res=True, ldx_pad=8),
    _b("p32-r-k72", "plain c32 u8 1p r", 17, 20, 72, bias=True, res=True, ldr_pad=4),
    _b("p32-r-k264", "plain c32 u8 1p r", 26, 2052, 264, bias=True, ldx_pad=8),
    _b("p32-r-k264-m27", "plain c32 u8 1p r", 27, 20, 264, res=True),
    _b("p32-r-k2048", "plain c32 u8 1p r", 32, 4092, 2048, res=True, ldw_pad=8),
    # XR32: 17..26 sequences, deep K, the launch's own rows staged
    _b("p32-xr-2112", "plain c32 u8 mp r x", 17, 20, 2112, bias=True, res=True),
    _b("p32-xr-3136", "plain c32 u8 mp r x", 26, 2052, 3136, bias=True, res=True, ldr_pad=4, ldx_pad=8),
    _b("p32-xr-4288", "plain c32 u8 mp r x", 26, 4092, 4288, res=True),
    # 27..32 sequences with deep K keep the 16-row units (pieces of 16 k-steps)
    _b("p32-u16-mp-m27", "plain c32 u16 mp", 27, 20, 2112, bias=True, res=True),
    _b("p32-u16-mp-3136", "plain c32 u16 mp", 32, 2052, 3136, bias=True, res=True, ldx_pad=8),
    _b("p32-u16-mp-4288", "plain c32 u16 mp", 27, 4092, 4288, res=True),
    # ---- plain, 16-row units (4096 < N < 8192) --------------------------------------------------------------------------------------------
    _b("p8-u16-1p", "plain c8 u16 1p", 8, 4100, 264, bias=True, res=True),
    _b("p8-u16-mp", "plain c8 u16 mp", 2, 8188, 2112, res=True, ldr_pad=4),
    _b("p16-u16-1p", "plain c16 u16 1p", 16, 4100, 264, bias=True),
    _b("p16-u16-mp", "plain c16 u16 mp", 9, 8188, 2112, bias=True, res=True),
    _b("p32-u16-1p", "plain c32 u16 1p", 32, 4100, 264, bias=True, res=True),
    _b("p32-u16-1p-k72", "plain c32 u16 1p", 17, 8188, 72, res=True, ldc_pad=3),
    _b("p32-u16-mp-n4100", "plain c32 u16 mp", 17, 4100, 3136, bias=True),
    # ---- plain, 32-row units (N >= 8192); 16420 = 514 units: two workgroups own three (the reduction's unit-parity double buffer reused) -----
    _b("p8-u32-1p", "plain c8 u32 1p", 5, 8196, 72, bias=True),
    _b("p8-u32-3units", "plain c8 u32 1p", 8, 16420, 72, bias=True, res=True),
    _b("p8-u32-mp", "plain c8 u32 mp", 1, 8196, 2112, bias=True),
    _b("p16-u32-1p", "plain c16 u32 1p", 13, 8196, 72, res=True),
    _b("p16-u32-3units", "plain c16 u32 1p", 9, 16420, 264, bias=True),
    _b("p16-u32-mp", "plain c16 u32 mp", 16, 8196, 2112, bias=True, res=True),
    _b("p32-u32-1p", "plain c32 u32 1p", 27, 8196, 72, bias=True, res=True),
    _b("p32-u32-3units", "plain c32 u32 1p", 26, 16420, 72, bias=True),
] + [
    # bias x residual in all four combinations, once per class
    _b(f"p{cls}-combo-b{int(b)}r{int(r)}", f"plain c{cls} u8 1p{_FLAG[cls]}", M, 20, 264, bias=b, res=r, ldr_pad=4 * int(b))
    for cls, M in ((8, 5), (16, 13), (32, 26)) for b in (False, True) for r in (False, True)
] + [
    # fused RMSNorm on every single-piece route (K = 2048: the only K at which the norm's lane + 64 i sweep covers real data in every slot)
    _b("p8-h-norm", "plain c8 u8 1p h", 5, 2052, 2048, norm=True, bias=True),
    _b("p8-h-norm-k264", "plain c8 u8 1p h", 8, 20, 264, norm=True, res=True),
    _b("p8-u16-norm", "plain c8 u16 1p", 2, 4100, 2048, norm=True),
    _b("p8-u32-norm", "plain c8 u32 1p", 8, 8196, 2048, norm=True, bias=True),
    _b("p16-r-norm", "plain c16 u8 1p r", 16, 2052, 2048, norm=True, res=True),
    _b("p16-u16-norm", "plain c16 u16 1p", 9, 4100, 2048, norm=True, bias=True),
    _b("p16-u32-norm", "plain c16 u32 1p", 13, 8196, 2048, norm=True),
    _b("p32-r-norm", "plain c32 u8 1p r", 27, 2052, 2048, norm=True, bias=True),
    _b("p32-r-norm-k72", "plain c32 u8 1p r", 17, 20, 72, norm=True, res=True),
    _b("p32-u16-norm", "plain c32 u16 1p", 32, 4100, 2048, norm=True, res=True),
    _b("p32-u32-norm", "plain c32 u32 1p", 17, 8196, 2048, norm=True, bias=True),
    # ---- SwiGLU (32-row units: 16 gate rows + their 16 up partners) ------------------------------------------------------------------------
    _b("s8-k72", "swiglu c8 u32 1p", 1, 32, 72, mode=SWIGLU, bias=True),
    _b("s8-n8224", "swiglu c8 u32 1p", 8, 8224, 264, mode=SWIGLU),
    _b("s8-3units", "swiglu c8 u32 1p", 5, 16448, 264, mode=SWIGLU, bias=True, ldx_pad=8),
    _b("s8-norm", "swiglu c8 u32 1p", 2, 8224, 2048, mode=SWIGLU, norm=True),
    _b("s8-oddldc", "swiglu c8 u32 1p", 5, 32, 264, mode=SWIGLU, bias=True, ldc_pad=3),
    _b("s8-mp2112", "swiglu c8 u32 mp", 5, 32, 2112, mode=SWIGLU, bias=True),
    _b("s8-mp-n8224", "swiglu c8 u32 mp", 8, 8224, 2112, mode=SWIGLU),
    _b("s16-k72", "swiglu c16 u32 1p", 9, 32, 72, mode=SWIGLU),
    _b("s16-3units", "swiglu c16 u32 1p", 16, 16448, 264, mode=SWIGLU, bias=True),
    _b("s16-norm", "swiglu c16 u32 1p", 13, 8224, 2048, mode=SWIGLU, norm=True, bias=True),
    _b("s16-mp4160", "swiglu c16 u32 mp", 13, 32, 4160, mode=SWIGLU, bias=True),
    _b("s16-mp4288", "swiglu c16 u32 mp", 16, 32, 4288, mode=SWIGLU),
    _b("s32-k72", "swiglu c32 u32 1p", 17, 32, 72, mode=SWIGLU, bias=True),
    _b("s32-n8224", "swiglu c32 u32 1p", 26, 8224, 264, mode=SWIGLU),
    _b("s32-3units", "swiglu c32 u32 1p", 27, 16448, 264, mode=SWIGLU, bias=True),
    _b("s32-norm", "swiglu c32 u32 1p", 32, 8224, 2048, mode=SWIGLU, norm=True),
    # ---- QKV: (1, 1) = 3 heads, 24 units, below one wave of units; (16, 2) = 160 units ----------------------------------------------------
    _q("q8-k72", "qkv c8 u16 1p h", 1, 1, 1, 72),
    _q("q8-k264", "qkv c8 u16 1p h", 5, 16, 2, 264, bias=True, ldx_pad=8),
    _q("q8-norm", "qkv c8 u16 1p h", 8, 16, 2, 2048, norm=True, bias=True),
    _q("q8-oddldc", "qkv c8 u16 1p h", 2, 1, 1, 264, bias=True, ldc_pad=3),
    _q("q8-mp2112", "qkv c8 u16 mp h", 2, 1, 1, 2112, bias=True),
    _q("q16-k72", "qkv c16 u16 1p r", 9, 1, 1, 72, bias=True),
    _q("q16-k264", "qkv c16 u16 1p r", 13, 16, 2, 264),
    _q("q16-norm", "qkv c16 u16 1p r", 16, 16, 2, 2048, norm=True, bias=True),
    _q("q16-mp2112", "qkv c16 u16 mp r", 13, 1, 1, 2112, bias=True),
    _q("q32-k72", "qkv c32 u16 1p r", 17, 1, 1, 72, bias=True),
    _q("q32-k264", "qkv c32 u16 1p r", 26, 16, 2, 264, bias=True),
    _q("q32-k264-m27", "qkv c32 u16 1p r", 27, 1, 1, 264),
    _q("q32-norm", "qkv c32 u16 1p r", 32, 16, 2, 2048, norm=True, bias=True),
    # ---- the o-projection with the attention combine in its prologue (x = the rows fo1_attention_decode_batch_bf16 writes) ---------------
    _c("combine-m1", "plain c8 u8 1p h", "combine", 1, 20, 2048, res=True, n_q=16, n_kv=2),
    _c("combine-m2", "plain c8 u8 1p h", "combine", 2, 20, 2048, res=True, n_q=16, n_kv=2, ldr_pad=4),
    # ---- refusals: FO1_ERR_ARG, canary untouched ------------------------------------------------------------------------------------------
    _b("refuse-swiglu", "refused c32 K>2048 swiglu", 17, 32, 2112, mode=SWIGLU),
    _q("refuse-qkv", "refused c32 K>2048 qkv", 17, 1, 1, 2112, bias=True),
    _b("refuse-plain-wide", "refused c32 K>2048 plain N>=8192", 17, 8192, 2112),
    _b("refuse-norm-deep", "refused norm K>2048", 5, 20, 2112, norm=True),
    # ---- gemv.hip: M = 3 runs MM = 4 with a zero row; N = 1, 6, 130: the last unit clamped; K = 4104: the last K-split wave's range is empty;
    #      11008: it is short ---------------------------------------------------------------------------------------------------------------
    _g("g1-k8", "gemv mm1 plain ks0", 1, 1, 8, bias=True),
    _g("g1-gelu", "gemv mm1 plain ks0", 1, 130, 520, act=ACT_GELU, bias=True, res=True, ldr_pad=3),
    _g("g1-ks-silu", "gemv mm1 plain ks1", 1, 6, 4096, act=ACT_SILU, bias=True),
    _g("g1-ks-11008", "gemv mm1 plain ks1", 1, 130, 11008, res=True, ldx_pad=8),
    _g("g2-relu-norm", "gemv mm2 plain ks0", 2, 6, 520, act=ACT_RELU, bias=True, res=True, norm=True),
    _g("g2-ks-4104", "gemv mm2 plain ks1", 2, 130, 4104, bias=True, res=True, ldw_pad=8),
    _g("g2-ks-norm", "gemv mm2 plain ks1", 2, 130, 4096, norm=True),
    _g("g2-k520", "gemv mm2 plain ks0", 2, 1, 520, bias=True, res=True),
    _g("g4-m3-gelu", "gemv mm4 plain ks0", 3, 130, 520, act=ACT_GELU, bias=True, ldc_pad=3),
    _g("g4-k8", "gemv mm4 plain ks0", 4, 6, 8, res=True),
    _g("g4-m3-ks-silu", "gemv mm4 plain ks1", 3, 6, 11008, act=ACT_SILU, bias=True, res=True),
    _g("g4-ks-norm", "gemv mm4 plain ks1", 4, 130, 4104, norm=True, bias=True),
    _g("g1-swiglu", "gemv mm1 swiglu ks0", 1, 64, 520, act=ACT_SWIGLU, bias=True),
    _g("g1-swiglu-ks", "gemv mm1 swiglu ks1", 1, 64, 4104, act=ACT_SWIGLU),
    _g("g2-swiglu-k8", "gemv mm2 swiglu ks0", 2, 64, 8, act=ACT_SWIGLU),
    _g("g2-swiglu-ks", "gemv mm2 swiglu ks1", 2, 64, 11008, act=ACT_SWIGLU, bias=True),
    _g("g4-m3-swiglu-norm", "gemv mm4 swiglu ks0", 3, 64, 520, act=ACT_SWIGLU, norm=True),
    _g("g4-swiglu-ks-norm", "gemv mm4 swiglu ks1", 4, 64, 4096, act=ACT_SWIGLU, bias=True, norm=True),
    _g("g4-swiglu", "gemv mm4 swiglu ks0", 4, 64, 520, act=ACT_SWIGLU, bias=True),
    _g("g4-m3-swiglu-ks", "gemv mm4 swiglu ks1", 3, 64, 4096, act=ACT_SWIGLU, bias=True),
    # the M <= 4 hand-off of fo1_gemm_bf16 (results: here; that it happens: tests/test_gemm_routes_gpu.py)
    _c("handoff-m4", "gemv mm4 plain ks0", "handoff", 4, 130, 520, act=ACT_GELU, bias=True, res=True),
    _c("handoff-m1-ks", "gemv mm1 plain ks1", "handoff", 1, 6, 4104, bias=True),
]


def reachable_labels() -> Dict[str, tuple]:
    """Every label the two dispatches reach with the product defaults (half switch 3), refusals included."""
    out: Dict[str, tuple] = {}
    for M in range(1, 33):
        for K in (72, 2048, 2112, 4288):
            for norm in (False, True):
                for N in (20, 4096, 4100, 8188, 8192, 16420):
                    out.setdefault(route_batch(M, N, K, PLAIN, norm).label(), (M, N, K, "plain", norm))
                for N in (32, 8224):
                    out.setdefault(route_batch(M, N, K, SWIGLU, norm).label(), (M, N, K, "swiglu", norm))
                for n_q, n_kv in ((1, 1), (16, 2)):
                    out.setdefault(route_batch(M, (n_q + 2 * n_kv) * 128, K, QKV, norm, 3, n_q, n_kv).label(), (M, n_q, n_kv, K, "qkv", norm))
    for M in (1, 2, 3, 4):
        for K in (8, 4088, 4096, 11008):
            for act in (0, 1, 2, 3, 5):
                out.setdefault(route_gemv(M, 64, K, act).label(), (M, 64, K, act))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def planted(K: int, r: Route) -> Dict[int, int]:
    """-> {planted k: sign of its chunk}."""
    pos = {0, 7, 8, K - 1}
    nsteps = cdiv(K, 64)
    if r.kind == "gemv":
        bounds = {512}                                                  # the lane stride: 64 chunks
        if r.ksplit:
            kq = cdiv(cdiv(K // 8, 4), 64) * 64
            bounds |= {w * kq * 8 for w in (1, 2, 3)}
        bounds.add(K - 8)
    else:
        steps = {1, 8, 16, (nsteps - 1) // 8 * 8, nsteps - 1} | ({p for p in range(r.psteps, nsteps, r.psteps)} if r.psteps else set())
        bounds = {64 * s for s in steps}
    for b in bounds:
        if 0 < b < K:
            pos |= {b - 1, b}
    pos = {p for p in pos if 0 <= p < K}
    chunks = sorted({p // 8 for p in pos})
    free = [c for c in range(K // 8) if c not in chunks]
    if len(chunks) % 2 and free:
        pos.add(free[len(free) // 2] * 8 + 3)
        chunks = sorted({p // 8 for p in pos})
    sign = {c: (1 if i % 2 == 0 else -1) for i, c in enumerate(chunks)}
    return {p: sign[p // 8] for p in sorted(pos)}


def row_scale(M: int) -> torch.Tensor:
    m = torch.arange(M)
    return torch.tensor([1.0, 2.0, 0.5])[m % 3] * torch.where(m >= 16, 0.25, 1.0)


def s_levels(M: int) -> torch.Tensor:
    return _levels(M) * row_scale(M)


def t_levels(N: int) -> torch.Tensor:
    n = torch.arange(N)
    return _levels(N) * torch.where((n // 8) % 2 == 1, 0.5, 1.0) * torch.where((n // 16) % 2 == 1, 1.5, 1.0)


def bias_ramp(N: int) -> torch.Tensor:
    n = torch.arange(N)
    return (0.015625 * (n % 4) + 0.0625 * ((n // 4) % 2) + 0.125 * ((n // 8) % 2) + 0.5 * ((n // 16) % 5) - 1.0 + 0.25 * ((n // 32) % 2)).bfloat16()


def build(c: Case) -> dict:
    r = case_route(c)
    # (a refused case is built for the route it would take one class down: only its buffers are used)
    pr = r if r.kind != "refused" else route_batch(min(c.M, 16), c.N, 2048 if c.norm else c.K, c.mode, c.norm, 3, c.n_q, c.n_kv)
    g = torch.Generator().manual_seed(c.seed)
    rs = row_scale(c.M)
    x = (torch.randn(c.M, c.K, generator=g) * 0.5 * rs[:, None]).bfloat16()
    W = (torch.randn(c.N, c.K, generator=g) * 0.05).bfloat16()
    pos = planted(c.K, pr)
    per_chunk: Dict[int, int] = {}
    for p in pos:
        per_chunk[p // 8] = per_chunk.get(p // 8, 0) + 1
    s, t = s_levels(c.M), t_levels(c.N)
    for p, sg in pos.items():
        x[:, p] = (sg * 2.0 * PLANT / per_chunk[p // 8] * s).bfloat16()
        W[:, p] = (0.5 * t).bfloat16()
    d = dict(case=c, route=r, x=x, W=W, pos=pos, bias=None, res=None, nw=None)
    if c.bias:
        d["bias"] = bias_ramp(c.N)
    if c.res:
        m, n = torch.arange(c.M)[:, None], torch.arange(c.N)[None, :]
        d["res"] = ((((3 * m + 5 * n) % 7) - 3) * 0.25 + ((m + n) % 2) * 0.125).bfloat16()
    if c.norm:
        nw = ((1.0 + 0.1 * torch.randn(c.K, generator=g)) * torch.where((torch.arange(c.K) // 8) % 2 == 1, -1.0, 1.0)).bfloat16()
        nw[list(pos)] = 1.0
        d["nw"] = nw
    if c.mode == QKV:
        ang = torch.rand(TABLE_ROWS, 128, generator=g) * 6.28
        d["cos"], d["sin"] = ang.cos().bfloat16(), ang.sin().bfloat16()
        st = torch.zeros(c.M, 8, dtype=torch.int32)
        st[:, 0] = 5 + 13 * torch.arange(c.M)
        st[:, 1] = 300 - 7 * torch.arange(c.M)
        d["state"] = st
    return d


def host_buffers(d: dict) -> dict:
    """The over-allocated buffers of the launch, on the CPU: NaN around the operands, the canary in every output and cache element."""
    c = d["case"]
    nan, BF = float("nan"), torch.bfloat16
    x = torch.full((c.M + SPARE_OPERAND_ROWS, c.K + c.ldx_pad), nan, dtype=BF)
    W = torch.full((c.N + SPARE_OPERAND_ROWS, c.K + c.ldw_pad), nan, dtype=BF)
    x[:c.M, :c.K] = d["x"]
    W[:c.N, :c.K] = d["W"]
    b = dict(x=x, W=W, out=torch.full((c.M + SPARE_ROWS, c.ldc), CANARY16, dtype=torch.int16).view(BF))
    if d["bias"] is not None:
        b["bias"] = torch.cat([d["bias"], torch.full((16,), nan, dtype=BF)])
    if d["nw"] is not None:
        b["nw"] = torch.cat([d["nw"], torch.full((16,), nan, dtype=BF)])
    if d["res"] is not None:
        b["res"] = torch.full((c.M + SPARE_OPERAND_ROWS, c.ldr), nan, dtype=BF)
        b["res"][:c.M, :c.N] = d["res"]
    if c.mode == QKV:
        b["cos"], b["sin"], b["state"] = d["cos"], d["sin"], d["state"]
        b["kc"] = torch.full((c.n_kv, CACHE_ROWS + KC_EXTRA_ROWS, 128), CANARY16, dtype=torch.int16).view(BF)
        b["vt"] = torch.full((c.n_kv * 128, CACHE_ROWS + VT_EXTRA_COLS), CANARY16, dtype=torch.int16).view(BF)
    return b


def to_device(d: dict, device="cuda") -> dict:
    return {k: v.to(device) for k, v in host_buffers(d).items()}


def check_cache_canary(kc: torch.Tensor, vt: torch.Tensor, d: dict, what: str) -> None:
    """Exactly the K rows / V^T columns state[m][0] of the M sequences are written, every element of them, and nothing else."""
    pos = d["state"][:, 0].long().to(kc.device)
    kw = kc.view(torch.int16) != CANARY16            # [n_kv, rows, 128]
    vw = vt.view(torch.int16) != CANARY16            # [n_kv * 128, cols]
    want_k = torch.zeros(kc.shape[1], dtype=torch.bool, device=kc.device)
    want_k[pos] = True
    want_v = torch.zeros(vt.shape[1], dtype=torch.bool, device=kc.device)
    want_v[pos] = True
    assert kw[:, want_k].all(), f"{what}: {int((~kw[:, want_k]).sum())} K-cache elements of the sequences' rows never written"
    assert not kw[:, ~want_k].any(), f"{what}: K-cache rows of other positions written, first at {kw[:, ~want_k].nonzero()[0].tolist()}"
    assert vw[:, want_v].all(), f"{what}: {int((~vw[:, want_v]).sum())} V^T elements of the sequences' columns never written"
    assert not vw[:, ~want_v].any(), f"{what}: V^T columns of other positions written, first at {vw[:, ~want_v].nonzero()[0].tolist()}"


def gather_outputs(d: dict, out: torch.Tensor, kc: Optional[torch.Tensor] = None, vt: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The launch's results in the reference's form: out [M, n_out]; QKV: k [M, n_kv * 128] (the K rows), v [M, n_kv * 128] (the V^T columns)."""
    c = d["case"]
    res = {"out": out[:c.M, :c.n_out].double().cpu()}
    if c.mode == QKV:
        pos = d["state"][:, 0].long().to(kc.device)
        res["k"] = kc[:, pos, :].permute(1, 0, 2).reshape(c.M, c.n_kv * 128).double().cpu()
        res["v"] = vt[:, pos].t().double().cpu()
    return res


# ---------------------------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------------------------
class _exact:
    def __init__(self, on: bool):
        self.on = on

    def __enter__(self):
        self.old = G.EXACT_ULP
        G.EXACT_ULP = self.on or self.old

    def __exit__(self, *a):
        G.EXACT_ULP = self.old


def _inter(d: dict, rstd_rel: float = RSTD_REL, exact_ulp: bool = False, xn_from: Optional[torch.Tensor] = None) -> dict:
    """fp64 intermediates: the effective x (normalised when the norm is fused), its error e [M, K], W, Z, Sabs, E = e |W|^T, rstd."""
    c = d["case"]
    x, W = d["x"].double(), d["W"].double()
    it = dict(W=W, rstd=None, xr=None)
    en = None
    if c.norm:
        rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + NORM_EPS)
        xr = x * rstd
        with _exact(exact_ulp):
            e1 = _rnd(rstd_rel * xr.abs(), xr)
            xn = xr * d["nw"].double()
            en = _rnd(d["nw"].double().abs() * e1, xn)
        it.update(rstd=rstd, xr=xr)
    else:
        xn = x
    if xn_from is not None:
        xn, en = xn_from, None
    it.update(xn=xn, Z=xn @ W.t(), Sabs=xn.abs() @ W.abs().t(), E=None if en is None else en @ W.abs().t())
    return it


def _shim(c: Case):
    act = ACT_SWIGLU if c.mode == SWIGLU else c.act
    return SimpleNamespace(act=act, out_f32=False)


def _outputs(d: dict, Z, Sabs, E, bias, res, cosr, sinr, acc: float, exact_ulp: bool, rope_sign=None, v_twice: bool = False) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """{name: (output, bound)} in float64.  bias: [N] or [M, N] or None; cosr / sinr: [M, 128] (QKV)."""
    c = d["case"]
    S = Sabs if E is None else Sabs + E / (acc * 2.0 ** -24)          # (the carried norm error enters where the accumulation error does)
    if c.mode != QKV:
        y, e = epilogue64(_shim(c), Z, S, bias, res, acc, exact_ulp)
        return {"out": (y, e)}
    M, H, KV = c.M, c.n_q, c.n_kv
    with _exact(exact_ulp):
        x = Z if bias is None else Z + bias
        e = acc * 2.0 ** -24 * (S if bias is None else S + (bias.abs() if torch.is_tensor(bias) else 0.0))
        e = _rnd(e, x)
        hx, he = x[:, :(H + KV) * 128].reshape(M, H + KV, 2, 64), e[:, :(H + KV) * 128].reshape(M, H + KV, 2, 64)
        a, b, ea, eb = hx[:, :, 0], hx[:, :, 1], he[:, :, 0], he[:, :, 1]
        c1, c2, s1, s2 = cosr[:, None, :64], cosr[:, None, 64:], sinr[:, None, :64], sinr[:, None, 64:]
        sg = -torch.ones(M, H + KV, 64, dtype=torch.float64) if rope_sign is None else rope_sign
        t1, t2 = a * c1, sg * b * s1
        ya = t1 + t2
        eya = _rnd(_rnd(c1.abs() * ea, t1) + _rnd(s1.abs() * eb, t2), ya)
        u1, u2 = b * c2, a * s2
        yb = u1 + u2
        eyb = _rnd(_rnd(c2.abs() * eb, u1) + _rnd(s2.abs() * ea, u2), yb)
        rot = torch.stack([ya, yb], 2).reshape(M, (H + KV) * 128)
        erot = torch.stack([eya, eyb], 2).reshape(M, (H + KV) * 128)
        v, ev = x[:, (H + KV) * 128:], e[:, (H + KV) * 128:]
        if v_twice:
            zv = Z[:, (H + KV) * 128:]
            v = zv.bfloat16().double() + (bias[..., (H + KV) * 128:] if bias is not None else 0.0)
    return {"out": (rot[:, :H * 128], erot[:, :H * 128]), "k": (rot[:, H * 128:], erot[:, H * 128:]), "v": (v, ev)}


def _tables(d: dict):
    c = d["case"]
    if c.mode != QKV:
        return None, None
    tr = d["state"][:, 1].long()
    return d["cos"].double()[tr], d["sin"].double()[tr]


def reference_and_bound(d: dict, acc: float = ACC, exact_ulp: bool = False, rstd_rel: float = RSTD_REL) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    it = _inter(d, rstd_rel, exact_ulp)
    cosr, sinr = _tables(d)
    bias = None if d["bias"] is None else d["bias"].double()
    res = None if d["res"] is None else d["res"].double()
    return _outputs(d, it["Z"], it["Sabs"], it["E"], bias, res, cosr, sinr, acc, exact_ulp)


# ---------------------------------------------------------------------------------------------------------------------------------------
# emulation
# ---------------------------------------------------------------------------------------------------------------------------------------
def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.bfloat16().float()


def _fma(acc: torch.Tensor, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp32 fma of bf16 operands: the product is exact in float64, one rounding."""
    return (acc.double() + a.double() * b.double()).float()


def _xor_tree(v: torch.Tensor) -> torch.Tensor:
    """v [64, ...] -> the value every lane holds after v += shfl_xor(v, o), o = 32 .. 1."""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v[0]


def emulate_norm(d: dict) -> Tuple[torch.Tensor, torch.Tensor]:
    """(bf16 normalised x as float32 [M, K], fp32 rstd [M, 1]) in the kernel's order."""
    c, r = d["case"], d["route"]
    x = d["x"].float()
    K = c.K
    threads, slots = (64, 4) if r.kind != "gemv" else (256, cdiv(K // 8, 256))
    pad = threads * slots * 8
    xp = torch.zeros(c.M, pad)
    xp[:, :K] = x
    xp = xp.view(c.M, slots, threads, 8).permute(2, 1, 3, 0)         # [thread, slot, element, M]
    ss = torch.zeros(threads, c.M)
    for j in range(slots):
        for e in range(8):
            ss = _fma(ss, xp[:, j, e], xp[:, j, e])
    if r.kind != "gemv":
        tot = _xor_tree(ss)
    else:
        w = [_xor_tree(ss[64 * i:64 * i + 64]) for i in range(4)]
        tot = ((w[0] + w[1]) + w[2]) + w[3]
    rstd = torch.rsqrt(tot / float(K) + torch.tensor(NORM_EPS, dtype=torch.float32))[:, None]
    return _bf(d["nw"].float() * _bf(x * rstd)), rstd


def emulate_acc(d: dict, xn: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 accumulators [M, N] in the kernel's K order; xn: the (normalised) bf16 x as float32."""
    c, r = d["case"], d["route"]
    x = d["x"].float() if xn is None else xn
    W = d["W"].float()
    K = c.K
    if r.kind == "gemv":
        kch = K // 8
        kq = cdiv(cdiv(kch, 4), 64) * 64 if r.ksplit else kch
        waves = []
        for w in range(4 if r.ksplit else 1):
            c0, c1 = (w * kq, min(kch, w * kq + kq)) if r.ksplit else (0, kch)
            n = max(c1 - c0, 0)
            slots = cdiv(n, 64) if n else 0
            acc = torch.zeros(64, c.M, c.N)
            if slots:
                xp = torch.zeros(c.M, slots * 64 * 8)
                wp = torch.zeros(c.N, slots * 64 * 8)
                xp[:, :n * 8] = x[:, c0 * 8:c1 * 8]
                wp[:, :n * 8] = W[:, c0 * 8:c1 * 8]
                xp = xp.view(c.M, slots, 64, 8).permute(2, 1, 3, 0)       # [lane, slot, e, M]
                wp = wp.view(c.N, slots, 64, 8).permute(2, 1, 3, 0)       # [lane, slot, e, N]
                for j in range(slots):
                    for e in range(8):
                        acc = _fma(acc, wp[:, j, e][:, None, :], xp[:, j, e][:, :, None])
            waves.append(_xor_tree(acc))
        return (waves[0] + waves[1]) + (waves[2] + waves[3]) if r.ksplit else waves[0]
    nsteps = cdiv(K, 64)
    xp = torch.zeros(c.M, nsteps * 64)
    wp = torch.zeros(c.N, nsteps * 64)
    xp[:, :K] = x
    wp[:, :K] = W
    chains = torch.zeros(8, 2, c.M, c.N)
    for s in range(nsteps):
        wave, dd = s % 8, s // 8
        for h in range(2):
            k0 = s * 64 + h * 32
            chains[wave, dd & 1] += xp[:, k0:k0 + 32] @ wp[:, k0:k0 + 32].t()
    t = chains[:, 0] + chains[:, 1]
    return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))


def emulate(d: dict) -> Dict[str, torch.Tensor]:
    c = d["case"]
    xn = emulate_norm(d)[0] if c.norm else None
    v = emulate_acc(d, xn)
    if d["bias"] is not None:
        v = v + d["bias"].float()
    v = _bf(v) if c.mode != QKV else v
    if c.mode == QKV:
        H, KV, M = c.n_q, c.n_kv, c.M
        vv = _bf(v[:, (H + KV) * 128:])
        hx = _bf(v[:, :(H + KV) * 128]).reshape(M, H + KV, 2, 64)
        a, b = hx[:, :, 0], hx[:, :, 1]
        tr = d["state"][:, 1].long()
        cs, sn = d["cos"].float()[tr][:, None, :], d["sin"].float()[tr][:, None, :]
        ya = _bf(_bf(a * cs[..., :64]) + _bf(-b * sn[..., :64]))
        yb = _bf(_bf(b * cs[..., 64:]) + _bf(a * sn[..., 64:]))
        rot = torch.stack([ya, yb], 2).reshape(M, (H + KV) * 128).double()
        return {"out": rot[:, :H * 128], "k": rot[:, H * 128:], "v": vv.double()}
    act = ACT_SWIGLU if c.mode == SWIGLU else c.act
    if act == ACT_SWIGLU:
        v4 = v.view(c.M, c.N // 32, 2, 16)
        g, u = v4[:, :, 0], v4[:, :, 1]
        return {"out": _bf(_bf(_act64(g.double(), ACT_SILU).float()) * u).reshape(c.M, c.N // 2).double()}
    if act != ACT_NONE:
        v = _bf(_act64(v.double(), act).float())
    if d["res"] is not None:
        v = _bf(v + d["res"].float())
    return {"out": v.double()}


def acc_error(d: dict) -> float:
    """The emulation's worst fp32 accumulation error (bias add included) in units of 2^-24 (|x| |W|^T + |bias|), on the emulation's own x."""
    c = d["case"]
    xn = emulate_norm(d)[0] if c.norm else d["x"].float()
    v = emulate_acc(d, xn)
    Z = xn.double() @ d["W"].double().t()
    S = xn.double().abs() @ d["W"].double().abs().t()
    if d["bias"] is not None:
        v = v + d["bias"].float()
        Z, S = Z + d["bias"].double(), S + d["bias"].double().abs()
    return ((v.double() - Z).abs() / (2.0 ** -24 * S).clamp_min(1e-300)).max().item()


def rstd_error(d: dict) -> float:
    """The emulated fp32 rstd's worst relative error, in units of 2^-24."""
    x = d["x"].double()
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + NORM_EPS)
    return ((emulate_norm(d)[1].double() - rstd).abs() / rstd).max().item() * 2.0 ** 24


# ---------------------------------------------------------------------------------------------------------------------------------------
# faults
# ---------------------------------------------------------------------------------------------------------------------------------------
FAULTS = (
    "drop_wave_step",            # the last k-step of wave 0 dropped in the last unit (gemv.hip: the last chunk of wave 0's range / of K)
    "drop_tail",                 # the K % 64 tail dropped in the last unit
    "pair_second_for_first",     # 8-row units: x of k-step 8 read for k-step 0 in the last unit
    "seq_neighbour_x",           # sequence M - 1 reads x row M - 2
    "group1_reads_group0",       # 17..32 sequences: column group 1 reads group 0's x in the last unit
    "xr32_alias",                # XR32: column M - 1 clamped to row M - 2 in the first unit
    "w_row_off8",                # the first unit reads the weight rows 8 further
    "bias_shift4",               # the first unit's bias quads shifted by 4
    "res_neighbour_seq",         # sequence M - 1 adds the residual row of M - 2
    "swiglu_swap",               # gate and up swapped in the last unit
    "rope_sign",                 # the rotary partner with the wrong sign (head 0, d < 8)
    "rope_neighbour_row",        # sequence M - 1 takes the cos / sin row of M - 2
    "cache_neighbour_pos",       # sequence M - 1 writes its K row / V column at the neighbour's cache position
    "v_rounded_twice",           # V = bf16(bf16(acc) + bias)
    "norm_w_skipped",            # sequence M - 1: the norm weight skipped
    "rstd_neighbour",            # sequence M - 1 normalised with the rstd of M - 2
)


def unit_cols(d: dict, u: int) -> torch.Tensor:
    """The weight rows (= columns of Z) of unit u."""
    c, r = d["case"], d["route"]
    if r.kind == "gemv":
        nf = c.N // 2 if r.swiglu else c.N
        f = torch.arange(4 * u, min(4 * u + 4, nf))
        if r.swiglu:
            rows = (f // 16) * 32 + f % 16
            return torch.cat([rows, rows + 16])
        return f
    if r.mode == SWIGLU:
        return torch.arange(32 * u, 32 * u + 32)
    if r.mode == QKV:
        rb = 8 if r.h8 else 16
        uph = 64 // rb
        n_rope = (c.n_q + c.n_kv) * uph
        if u < n_rope:
            r0 = (u // uph) * 128 + (u % uph) * rb
            return torch.cat([torch.arange(r0, r0 + rb), torch.arange(r0 + 64, r0 + 64 + rb)])
        r0 = (c.n_q + c.n_kv) * 128 + (u - n_rope) * 2 * rb
        return torch.arange(r0, r0 + 2 * rb)
    return torch.arange(u * r.rows, min((u + 1) * r.rows, c.N))


def out_cols(d: dict, cols: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Columns of Z -> {output name: its columns}."""
    c = d["case"]
    if c.mode == QKV:
        a, b = c.n_q * 128, (c.n_q + c.n_kv) * 128
        out = {"out": cols[cols < a], "k": cols[(cols >= a) & (cols < b)] - a, "v": cols[cols >= b] - b}
        return {k: v for k, v in out.items() if v.numel()}
    if c.mode == SWIGLU or c.act == ACT_SWIGLU:
        return {"out": torch.unique((cols // 32) * 16 + cols % 16)}
    return {"out": cols}


def applicable_faults(d: dict) -> List[str]:
    c, r = d["case"], d["route"]
    nsteps = cdiv(c.K, 64)
    ok = {
        "drop_wave_step": True,
        "drop_tail": r.kind == "mfma" and c.K % 64 != 0 and nsteps > 1,
        "pair_second_for_first": r.kind == "mfma" and r.h8 and nsteps > 8,
        "seq_neighbour_x": c.M >= 2,
        "group1_reads_group0": r.kind == "mfma" and c.M > 16,
        "xr32_alias": r.xr32,
        "w_row_off8": c.N > 8,
        "bias_shift4": c.bias and c.N > 4,
        "res_neighbour_seq": c.res and c.M >= 2,
        "swiglu_swap": c.mode == SWIGLU or c.act == ACT_SWIGLU,
        "rope_sign": c.mode == QKV,
        "rope_neighbour_row": c.mode == QKV and c.M >= 2,
        "cache_neighbour_pos": c.mode == QKV,
        "v_rounded_twice": c.mode == QKV and c.bias,
        "norm_w_skipped": c.norm,
        "rstd_neighbour": c.norm and c.M >= 2,
    }
    if c.norm:
        # the norm term of the bound (worst case over K roundings) is above what the small-step faults move: they are judged on the route's
        # cases without the norm; gemv.hip with a deep normed K (bound about 1) keeps the norm's own faults and the sequence faults only
        for f in ("bias_shift4", "res_neighbour_seq", "v_rounded_twice", "swiglu_swap"):
            ok[f] = False
        if r.kind == "gemv" and c.K >= 4096:
            for f in ("drop_wave_step", "w_row_off8"):
                ok[f] = False
    return [f for f in FAULTS if ok[f]]


def reference(d: dict, fault: Optional[str] = None, acc: float = ACC):
    """The float64 outputs {name: tensor}.  With a fault: (the outputs the faulty kernel would leave — the canary value where it stores nothing
    — and the regions [(name, rows, columns)] the fault touches)."""
    c, r = d["case"], d["route"]
    if fault is None:
        return {k: v[0] for k, v in reference_and_bound(d, acc).items()}
    if "_inter" not in d:
        d["_inter"] = _inter(d)              # (shared by the faults of a case, never changed)
    it = d["_inter"]
    Z, Sabs, W, xn = it["Z"].clone(), it["Sabs"], it["W"], it["xn"]
    M, N, K = c.M, c.N, c.K
    bias = None if d["bias"] is None else d["bias"].double()[None, :].expand(M, N).clone()
    res = None if d["res"] is None else d["res"].double().clone()
    cosr, sinr = _tables(d)
    rope_sign, v_twice = None, False
    last, first = unit_cols(d, r.units - 1), unit_cols(d, 0)
    if r.kind == "gemv" and r.units > 4 and fault == "bias_shift4":
        first = unit_cols(d, 3)                 # features 12..15 -> 16..19: across the ramp's 16-feature jump
    last, first = last[last < N], first[first < N]
    allrows = torch.arange(M)
    rows, cols = allrows, None                 # region: rows x out_cols(cols); cols None = every output column
    post = None
    nsteps = cdiv(K, 64)
    if fault == "drop_wave_step":
        if r.kind == "gemv":
            kq = cdiv(cdiv(K // 8, 4), 64) * 64 if r.ksplit else K // 8
            k1 = min(K, kq * 8)
            k0 = k1 - 8
        else:
            k0 = (nsteps - 1) // 8 * 8 * 64
            k1 = min(K, k0 + 64)
        Z[:, last] -= xn[:, k0:k1] @ W[last, k0:k1].t()
        cols = last
    elif fault == "drop_tail":
        k0 = K - K % 64
        Z[:, last] -= xn[:, k0:] @ W[last, k0:].t()
        cols = last
    elif fault == "pair_second_for_first":
        x8 = torch.zeros(M, 64, dtype=torch.float64)
        k1 = min(K, 576)
        x8[:, :k1 - 512] = xn[:, 512:k1]
        Z[:, last] += (x8 - xn[:, :64]) @ W[last, :64].t()
        cols = last
    elif fault == "seq_neighbour_x":
        Z[M - 1] = Z[M - 2]
        rows = torch.tensor([M - 1])
    elif fault == "group1_reads_group0":
        Z[16:M, last[:, None]] = Z[0:M - 16, last[:, None]].clone()
        rows, cols = torch.arange(16, M), last
    elif fault == "xr32_alias":
        Z[M - 1, first] = Z[M - 2, first]
        rows, cols = torch.tensor([M - 1]), first
    elif fault == "w_row_off8":
        Z[:, first] = it["Z"][:, (first + 8).clamp_max(N - 1)]
        cols = first
    elif fault == "bias_shift4":
        bias[:, first] = d["bias"].double()[(first + 4).clamp_max(N - 1)][None, :]
        cols = first
    elif fault == "res_neighbour_seq":
        res[M - 1] = res[M - 2]
        rows = torch.tensor([M - 1])
    elif fault == "swiglu_swap":
        g, u = last[:len(last) // 2], last[len(last) // 2:]
        if r.kind != "gemv":
            g, u = last[:16], last[16:]
        Z[:, torch.cat([g, u])] = it["Z"][:, torch.cat([u, g])]
        if bias is not None:
            bias[:, torch.cat([g, u])] = d["bias"].double()[torch.cat([u, g])][None, :]
        cols = last
    elif fault == "rope_sign":
        rope_sign = -torch.ones(M, c.n_q + c.n_kv, 64, dtype=torch.float64)
        rope_sign[:, 0, :8] = 1.0
        cols = torch.arange(8)
    elif fault == "rope_neighbour_row":
        cosr, sinr = cosr.clone(), sinr.clone()
        cosr[M - 1], sinr[M - 1] = cosr[M - 2], sinr[M - 2]
        rows, cols = torch.tensor([M - 1]), torch.arange((c.n_q + c.n_kv) * 128)
    elif fault == "cache_neighbour_pos":
        rows, cols = torch.tensor([M - 1]), torch.arange(c.n_q * 128, N)

        def post(o):
            for name in ("k", "v"):
                if M >= 2:
                    o[name][M - 2] = o[name][M - 1]
                o[name][M - 1] = CANARY_F
    elif fault == "v_rounded_twice":
        v_twice = True
        cols = torch.arange((c.n_q + c.n_kv) * 128, N)
    elif fault == "norm_w_skipped":
        Z[M - 1] = it["xr"][M - 1] @ W.t()
        rows = torch.tensor([M - 1])
    elif fault == "rstd_neighbour":
        Z[M - 1] = Z[M - 1] * (it["rstd"][M - 2] / it["rstd"][M - 1])
        rows = torch.tensor([M - 1])
    else:
        raise ValueError(fault)
    outs = {k: v[0].clone() for k, v in _outputs(d, Z, Sabs, it["E"], bias, res, cosr, sinr, acc, False, rope_sign, v_twice).items()}
    if post is not None:
        post(outs)
    oc = out_cols(d, torch.arange(N) if cols is None else cols)
    return outs, [(name, rows, cc) for name, cc in oc.items()]


def region_worst(mut: Dict[str, torch.Tensor], rb: Dict[str, Tuple[torch.Tensor, torch.Tensor]], region) -> float:
    """The largest |mut - ref| / bound over a touched region (NaN counts as infinite)."""
    name, rows, cols = region
    ref, bound = rb[name]
    q = (mut[name][rows][:, cols] - ref[rows][:, cols]).abs() / bound[rows][:, cols]
    return torch.nan_to_num(q, nan=float("inf")).max().item()
