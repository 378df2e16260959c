"""Cases, routing model, fp64 reference, emulated kernel arithmetic, per-element bound and faults of the bf16 tile GEMM
(vlm_fo1_amd/csrc/gemm.hip: fo1_gemm_bf16 / _ws, fo1_gemm_bf16_partials, fo1_gemm_bf16_wtiled), shared by tests/test_gemm_route_cases.py (CPU:
the routing model covers what the heuristic reaches, the bound passes the emulation and fails every fault) and tests/test_gemm_routes_gpu.py
(the per-route sweep on the MI355X).

Routing model.  route() restates gemm_dispatch (and fo1_gemm_bf16_ws's GEMV hand-off, fo1_gemm_bf16_partials, fo1_gemm_bf16_wtiled) in plain
Python: (M, N, K, act, out_f32, workspace bytes, pins) -> Route(kind, BM, BN, ring depth, split count, K tiles per run, reduce launch).  The GPU
test checks it against the library: the product library's profile rows must be Route.product_rows(), and the A/B library's shape-carrying
row (fo1_gemm_profile_shapes) must be Route.shape_row(), which states tile, split count and ring depth.  fo1_gemm_set_gemv, the A/B
switch of the GEMV hand-off, is not modelled (no case turns it off).  Route.label() is what SWEEP claims for
a case and what the coverage test enumerates.

Operands (build()).  A ~ 0.5 N(0, 1), W ~ 0.05 N(0, 1) in bf16 as tests/test_ops_gpu.py, plus PLANTED columns: at k = 0, 7, 8, both sides of
the first K-tile boundary (63, 64), both sides of every split-K run boundary of the case's route, K - 9, K - 8, K - 1 and the first and last
element of the register route's K % 64 tail, A[m, k] = +-2 s_m / c and W[n, k] = +-0.5 t_n / c, with s_m, t_n in +-{1, 1.25, 1.5, 1.75} and c
the number of planted positions in that 16-byte chunk (8 elements: what one load instruction of a lane fetches).  A chunk so contributes
+-s_m t_n to every output element, exactly; the sign alternates from planted chunk to planted chunk (one filler chunk is added when their
number is odd), so the sum over all of them is zero and the output keeps the magnitude of the random part (about 0.025 sqrt K), while one
chunk missing, doubled or read from the neighbouring row moves every element of the tile by at least 1.  Bias: a per-column ramp with a jump
at every 16- and 32-column fragment boundary.  Residual: a pattern that differs between (m, n), (m, n +- 1) and (m +- 1, n).

Device buffers (to_device()) are over-allocated: operand rows past M / N and the columns K..lda / K..ldw hold NaN, the residual has its own
row stride; the output has ldc > n_out and SPARE_ROWS rows past M and is pre-filled with the CANARY bit pattern (0xC9C9 / 0xC9C9C9C9:
-1.65e6 in both formats); the partial planes (whose row stride the ABI fixes at N) are followed by a spare canary plane.  check_canary():
every element outside [0, M) x [0, n_out) still holds the canary and none inside does.

Reference and bound.  reference() is float64 on the bf16 inputs with no intermediate rounding; bound() is one number per ELEMENT, from the
fp64 intermediates (never from the output's maximum):
  * every bf16 rounding point costs half a bf16 ulp, at most 2^-8 |value there| (8 significand bits), and what arrives at that point from
    earlier ones passes through the later steps' first-order slope: GELU <= 1.13, SiLU <= 1.10 (the maxima of |gelu'| and |silu'|), ReLU and
    the residual add 1, SwiGLU |up| on the gate side and |silu(gate)| on the up side (plus the product of the two errors);
  * the fp32 accumulation costs ACC 2^-24 S[m, n], S = |A| |W|^T (+ |bias|) in fp64.  ACC = 16: tests/test_gemm_route_cases.py asserts that the
    emulation's accumulation error stays at or below ACC / 4 = 4 x 2^-24 S over SWEEP (measured worst: see RESULTS_CPU below);
  * fp32 output and the partial planes have no bf16 term: the accumulation term alone (a plane: S over its own K run), plus for the fp32
    GELU 2^-21 |x| (fo1_gelu_erf: Abramowitz-Stegun 7.1.26, 1.5e-7 absolute on erfc, and an approximate reciprocal).

emulate() restates the kernels' arithmetic: fp32 accumulation K tile by K tile (64; MFMA steps of 16 inside) in the route's K order, per
split-K run with the planes summed in z order as gemm_splitk_reduce_kernel does, then bf16(acc + bias), bf16(act), bf16(+ residual), or
bf16(bf16(silu(bf16 gate)) * bf16 up).

FAULTS / reference(d, fault): each changes one tile or one edge, which a whole-output norm does not see; see the list at FAULTS.

What this makes redundant in tests/test_ops_gpu.py (kept as they are): the whole-output bounds of test_gemm_variants, test_gemm_splitk,
test_gemm_p8_256x256 and test_gemm_p8_persistent assert less, on the same kernels, than the sweep's cases on those routes.

A consequence of the bf16 term being the exact worst case of round-to-nearest: a correct kernel reaches up to 1.0 of the bound on a bf16
output (an element just above a power of two), so "half the bound" separates nothing there.  What has room is the accumulation term; the CPU
test therefore holds the emulation to a SHARPER bound — every rounding point at the half ulp of the value's own binade,
2^(floor(log2 |v|) - 8), and the accumulation term at ACC / 4 — and to half the bound where there is no bf16 term; a route on the
GPU should show up to 1.0 on bf16 outputs and under 0.5 on fp32 outputs and planes.

RESULTS_CPU (printed by tests/test_gemm_route_cases.py -s; 85 cases): emulation at most 0.994 of the bound on bf16 outputs and 0.336 on
fp32 outputs / planes; accumulation error at most 2.68 x 2^-24 S (partials64x128; 2.02 outside the partial planes), hence ACC = 16 >=
4 x 2.68; the weakest fault moves its tile by 3.9 x the bound.
RESULTS_GPU: not recorded yet.  tests/test_gemm_routes_gpu.py prints one "SUMMARY <route>: <profile rows> worst <fraction>" line per route;
the figures of its first MI355X run belong here, as do the cases an injected kernel fault (the last split-K run one K tile short; the bias
of epilogue_vec one fragment over) makes fail."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

ACT_NONE, ACT_GELU, ACT_SILU, ACT_SWIGLU, ACT_RELU = 0, 1, 2, 3, 5
ACT_NAME = {0: "none", 1: "gelu", 2: "silu", 3: "swiglu", 5: "relu"}
WS_BYTES = 64 * 1024 * 1024          # ops._gemm_workspace: the split-K scratch every ops.gemm call passes
ACC = 16.0
GELU_SLOPE, SILU_SLOPE = 1.13, 1.10
HALF_ULP = 2.0 ** -8
CANARY16 = 0xC9C9 - 0x10000          # as int16
CANARY32 = 0xC9C9C9C9 - 0x100000000  # as int32
SPARE_ROWS = 3
SPARE_OPERAND_ROWS = 2


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------------
# routing model
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Pin:
    """The A/B library's switches (include/fo1_ab.h); all zero / default = automatic dispatch."""
    staging: int = 0       # fo1_gemm_set_variant: 0 auto, 1 register, 2 two-stage LDS-DMA, 3 / 4 / 5 / 6 ring of that depth
    tile: int = 0          # 0 auto, 1 128x128, 2 64x128, 3 64x64, 4 128x256, 5 256x256, 6 <128,96>, 7 <128,64>
    splitk: int = 0        # fo1_gemm_set_splitk
    sched: int = 1         # fo1_gemm_set_big_schedule: bit 0 two-phase, bit 1 fragment epilogue, bit 2 persistent loop
    group_m: int = 0       # fo1_gemm_set_group_m

    def auto(self) -> bool:
        return self == Pin()


@dataclass(frozen=True)
class Route:
    kind: str              # reg | glds | ring | wide | big | gemv
    BM: int = 0
    BN: int = 0
    stages: int = 0        # ring depth asked of the launcher (p.stages); 2 = two-stage, 0 = register staging
    splits: int = 1
    kper: int = 0          # K tiles per split-K run (splits > 1)
    reduce: bool = False   # gemm_splitk_reduce launched
    sched: int = 1         # big: the 256 x 256 schedule bits
    coal: bool = True      # big: coalesced LDS epilogue

    def ring_depth(self) -> int:
        """The depth of the ring kernel that runs (the launchers map a request onto the instantiated depths)."""
        if self.kind != "ring":
            return 0
        if (self.BM, self.BN) == (128, 96):
            return self.stages if self.stages in (3, 4) else 5
        if (self.BM, self.BN) == (128, 64):
            return self.stages if self.stages in (3, 4) else 6
        if self.stages in (3, 4):
            return self.stages
        return 6 if self.BM + self.BN <= 128 else 4

    def label(self) -> str:
        if self.kind == "gemv":
            return "gemv"
        if self.kind == "reg":
            return f"reg<{self.BM},{self.BN}>"
        if self.kind == "big":
            form = "p4p" if self.sched & 4 else ("p4" if self.sched & 1 else "p8")
            s = f"{form}<256,256>" + ("" if self.coal else " frag")
        elif self.kind == "ring":
            s = f"ring<{self.BM},{self.BN},{self.ring_depth()}>"
        else:
            s = f"glds<{self.BM},{self.BN}>"
        if self.splits > 1:
            s += f" splitk{'+reduce' if self.reduce else ' planes'}"
        return s

    def product_rows(self) -> List[str]:
        """Profile row names of the launch without fo1_gemm_profile_shapes (both libraries), in launch order."""
        if self.kind == "reg":
            rows = ["gemm_bf16_reg"]
        elif self.kind == "big":
            rows = ["gemm_bt_p4p<256,256>" if self.sched & 4 else ("gemm_bt_p4<256,256>" if self.sched & 1 else "gemm_bt_p8<256,256>")]
        elif self.kind == "ring":
            deep = (self.BM, self.BN) in ((128, 96), (128, 64))
            rows = [f"gemm_bt_ring<{self.BM},{self.BN},{self.stages if deep else self.ring_depth()}>"]
        else:
            rows = [f"gemm_bt_glds<{self.BM},{self.BN}>"]
        return rows + (["gemm_splitk_reduce"] if self.reduce else [])

    def shape_row(self, M: int, N: int, K: int) -> str:
        """The GEMM's row name under fo1_gemm_profile_shapes(1) (A/B library): tile, split count, ring depth."""
        s = f"gemm {M}x{N}x{K} t{self.BM}x{self.BN} s{self.splits}"
        if self.kind in ("wide", "big"):
            return s
        return s + f" r{self.stages}"


def big_tile_rule(M: int, N: int, K: int, pin: Pin = Pin()) -> bool:
    if K % 64 != 0 or pin.staging == 1:
        return False
    if pin.tile != 0:
        return pin.tile == 5
    t256 = cdiv(M, 256) * cdiv(N, 256)
    return K // 64 >= 4 and M >= 1024 and t256 >= 128 and t256 / (cdiv(t256, 256) * 256) >= 0.6


def route(M: int, N: int, K: int, act: int = 0, out_f32: bool = False, ws_bytes: int = WS_BYTES, pin: Pin = Pin(), ldc_mult: int = 8,
          res: bool = False, ldr_mult: int = 8) -> Route:
    """fo1_gemm_bf16_ws -> gemm_dispatch.  ldc_mult / ldr_mult: the largest power of two (up to 8) dividing ldc / ldr — the 256 x 256
    kernel's alignment conditions (the buffers themselves are 16-byte aligned here)."""
    # (fo1_gemm_set_gemv, the A/B switch of this hand-off, is not modelled: no case turns it off)
    if M <= 4 and not out_f32 and (4 if M > 2 else M) * K * 2 <= 150 * 1024 and (act != ACT_SWIGLU or N % 32 == 0):
        return Route("gemv")
    glds = K % 64 == 0 and pin.staging != 1
    assert not (pin.staging >= 2 and K % 64 != 0)
    t128 = cdiv(M, 128) * cdiv(N, 128)
    t64x128 = cdiv(M, 64) * cdiv(N, 128)
    t64 = cdiv(M, 64) * cdiv(N, 64)
    nk = K // 64
    tile, splits = pin.tile, pin.splitk
    can_split = glds and ws_bytes > 0 and N % 4 == 0 and act != ACT_SWIGLU
    auto_tile = tile == 0
    if auto_tile:
        tile = 1 if (t128 >= 768 and nk >= 16) else (2 if t64x128 >= 512 else 3)
        if glds and nk >= 16 and cdiv(M, 128) * cdiv(N, 256) >= 1024:
            tile = 4
        if splits == 0 and can_split and nk >= 64 and t64x128 < 512:
            tile = 2
        if glds and 64 < M <= 128 and t128 >= 128 and nk >= 16:
            tile = 1
        if glds and 64 < M <= 128 and nk >= 16 and act == ACT_SWIGLU and N >= 8192 and not out_f32:
            tile = 6
        if big_tile_rule(M, N, K, pin):
            tile = 5
    p_splits, kper = 1, nk + 1
    tiles = t64 if tile == 3 else (t64x128 if tile == 2 else (cdiv(M, 128) * cdiv(N, 64) if tile == 7 else t128))
    if can_split and tile != 6:
        if splits == 0:
            splits = 1
            if nk >= 64 and tiles < 512 and tile == 2:
                splits = min(8, cdiv(256, tiles))
        splits = min(splits, nk)
        while splits > 1 and splits * M * N * 4 > ws_bytes:
            splits -= 1
        if splits > 1:
            kper = cdiv(nk, splits)
            p_splits = cdiv(nk, kper)
    p8_ok = glds and not out_f32 and N % 4 == 0 and ldc_mult >= 4 and (not res or ldr_mult >= 4) and (act != ACT_SWIGLU or N % 32 == 0) and act <= ACT_SWIGLU
    if tile == 5 and p8_ok:
        nc = N // 2 if act == ACT_SWIGLU else N
        coal = not (pin.sched & 2) and nc % 8 == 0 and ldc_mult >= 8 and (not res or ldr_mult >= 8)
        sched = pin.sched & 5
        n_tiles = cdiv(M, 256) * cdiv(N, 256)
        if not (sched & 1 and sched & 4 and p_splits == 1 and coal and n_tiles > 256 and nk >= 2 and nk % 2 == 0):
            sched &= 1
        return Route("big", 256, 256, 2, p_splits, kper if p_splits > 1 else 0, p_splits > 1, sched, coal)
    if tile == 5:
        tile = 1
    if tile in (6, 7) and not (glds and not out_f32):
        tile = 1
    if tile == 6:
        return Route("ring", 128, 96, pin.staging if pin.staging >= 3 else 3, 1, 0, False)
    if tile == 7:
        return Route("ring", 128, 64, pin.staging if pin.staging >= 3 else (6 if p_splits > 1 else 3), p_splits, kper if p_splits > 1 else 0, p_splits > 1)
    if pin.staging >= 3:
        stages = pin.staging
    elif pin.staging == 0 and glds and ((tile == 3 and t64 <= 768) or (tile == 2 and tiles * p_splits < 512) or (tile == 1 and auto_tile and M <= 128)):
        stages = 3
    else:
        stages = 2
    kp = kper if p_splits > 1 else 0
    if tile == 4 and glds and stages == 2:
        return Route("wide", 128, 256, 2, p_splits, kp, p_splits > 1)
    if tile == 4:
        tile = 1
    BM, BN = {1: (128, 128), 2: (64, 128), 3: (64, 64)}[tile]
    if not glds:
        return Route("reg", BM, BN, 0, 1, 0, False)
    return Route("ring" if stages >= 3 else "glds", BM, BN, stages, p_splits, kp, p_splits > 1)


def route_partials(M: int, N: int, K: int, splits: int, pin: Pin = Pin()) -> Route:
    """fo1_gemm_bf16_partials: planes only, no reduce launch."""
    nk = K // 64
    assert K % 64 == 0 and N % 4 == 0 and 2 <= splits <= min(nk, 64)
    kper = cdiv(nk, splits)
    eff = cdiv(nk, kper)
    assert eff >= 2
    if pin.tile == 7 and 64 < M <= 128:
        return Route("ring", 128, 64, pin.staging if pin.staging >= 3 else 6, eff, kper, False)
    if 64 < M <= 128 and N >= 8192 and nk >= 16:
        return Route("wide", 128, 256, 3, eff, kper, False)
    if cdiv(M, 64) * cdiv(N, 128) * eff >= 256:
        return Route("ring", 64, 128, 3, eff, kper, False)
    return Route("ring", 64, 64, 3, eff, kper, False)


def route_wtiled(M: int, N: int, K: int) -> Route:
    assert 1 <= M <= 128 and N % 128 == 0 and K % 64 == 0
    return Route("ring", 128 if M > 64 else 64, 128, 3, 1, 0, False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    claim: str                      # the route label the table claims (Route.label(), + " s<planes>" under split-K)
    M: int
    N: int
    K: int
    act: int = 0
    bias: bool = False
    res: bool = False
    out_f32: bool = False
    entry: str = "gemm"             # gemm (fo1_gemm_bf16_ws through ops.gemm) | partials | wtiled
    splits: int = 0                 # partials: the requested plane count
    pin: Pin = Pin()                # not Pin(): runs on the A/B library
    lda_pad: int = 0                # lda = K + lda_pad, ldw = K + ldw_pad (multiples of 8)
    ldw_pad: int = 0
    ldc_pad: int = 8                # ldc = n_out + ldc_pad (> 0: the canary columns)
    ldr_pad: int = 0                # ldr = N + ldr_pad
    seed: int = 0
    M0: int = 0                     # scale_down(): the shape the route is taken from
    N0: int = 0

    @property
    def n_out(self) -> int:
        return self.N // 2 if self.act == ACT_SWIGLU else self.N

    @property
    def ldc(self) -> int:
        return self.n_out + self.ldc_pad

    @property
    def ldr(self) -> int:
        return self.N + self.ldr_pad

    def auto(self) -> bool:
        return self.pin.auto() and self.entry != "wtiled"


def _mult(x: int) -> int:
    return 8 if x % 8 == 0 else (4 if x % 4 == 0 else (2 if x % 2 == 0 else 1))


def case_route(c: Case) -> Route:
    M, N = c.M0 or c.M, c.N0 or c.N
    ldc = (N // 2 if c.act == ACT_SWIGLU else N) + c.ldc_pad
    if c.entry == "partials":
        return route_partials(M, N, c.K, c.splits, c.pin)
    if c.entry == "wtiled":
        return route_wtiled(M, N, c.K)
    return route(M, N, c.K, c.act, c.out_f32, WS_BYTES, c.pin, _mult(ldc), c.res, _mult(N + c.ldr_pad))


def claim_of(r: Route) -> str:
    return r.label() + (f" s{r.splits}" if r.splits > 1 else "")


def _c(name, claim, M, N, K, **kw) -> Case:
    return Case(name, claim, M, N, K, seed=len(name) * 131 + M + 7 * N + 13 * K, **kw)


G, S, R, SW = ACT_GELU, ACT_SILU, ACT_RELU, ACT_SWIGLU
SWEEP: List[Case] = [
    # ---- automatic dispatch (product library; the A/B library without pins confirms tile, planes and ring depth) --------------------------
    # register staging (K % 64 != 0): K % 64 = 24, 8, 56, 24; epilogue_vec and the general epilogue (N % 4 != 0, odd ldc; fp32 out)
    _c("reg64x64", "reg<64,64>", 200, 328, 1176, bias=True, lda_pad=8, ldw_pad=16),
    _c("reg64x64-tiny-silu-res", "reg<64,64>", 77, 130, 72, act=S, bias=True, res=True, ldc_pad=3, ldr_pad=5),
    _c("reg64x64-k8-gelu", "reg<64,64>", 65, 129, 8, act=G, bias=True, ldc_pad=1),
    _c("reg64x64-f32", "reg<64,64>", 63, 64, 120, bias=True, out_f32=True, ldc_pad=4),
    _c("reg64x64-relu-res", "reg<64,64>", 128, 191, 56, act=R, bias=True, res=True, ldr_pad=8),
    _c("reg64x128", "reg<64,128>", 1564, 3424, 72, bias=True, res=True, ldr_pad=16),
    _c("reg128x128", "reg<128,128>", 1564, 8192, 1176, act=G, bias=True),
    # two-stage LDS-DMA
    _c("glds64x64-k1", "glds<64,64>", 129, 16768, 64, bias=True, res=True, ldr_pad=8),
    _c("glds64x64-f32-gelu", "glds<64,64>", 129, 16772, 128, act=G, bias=True, out_f32=True, ldc_pad=4),
    _c("glds64x128", "glds<64,128>", 1564, 3424, 1280, act=G, bias=True, lda_pad=8),
    _c("glds64x128-silu-res", "glds<64,128>", 1537, 4225, 128, act=S, bias=True, res=True, ldc_pad=3, ldr_pad=7),
    _c("glds128x128", "glds<128,128>", 515, 22016, 1024, bias=True, ldw_pad=8),
    _c("glds128x128-relu-res", "glds<128,128>", 513, 24580, 1024, act=R, bias=True, res=True, ldc_pad=12, ldr_pad=4),
    _c("glds128x256", "glds<128,256>", 897, 32516, 1024, act=G, bias=True, ldc_pad=12),
    _c("glds128x256-res", "glds<128,256>", 1023, 32768, 1024, res=True, ldr_pad=8),
    # 3-deep ring, 64 x 64: tile counts in every residue mod 8 (the XCD swizzle of tile_coords): 7 x n tiles, n = 33 .. 40
    _c("ring64x64", "ring<64,64,3>", 391, 2560, 2048, bias=True, lda_pad=8, ldw_pad=8),
    _c("ring64x64-f32", "ring<64,64,3>", 700, 4096, 1280, out_f32=True, ldc_pad=4),
    _c("ring64x64-k1", "ring<64,64,3>", 5, 64, 64, bias=True, res=True, ldr_pad=8),
    _c("ring64x64-k2-gelu", "ring<64,64,3>", 63, 65, 128, act=G, bias=True, ldc_pad=7),
    _c("ring64x64-swiglu", "ring<64,64,3>", 64, 160, 256, act=SW, bias=True, ldc_pad=4),
] + [
    _c(f"ring64x64-t{7 * n}", "ring<64,64,3>", 385 + n, 64 * n - (n % 3) * 4, 192, act=(0, G, S, R)[n % 4], bias=n % 2 == 0, res=n % 3 == 0,
       ldr_pad=8 * (n % 2))
    for n in range(33, 41)
] + [
    # 3-deep ring, 64 x 128, split-K 2 .. 8 through gemm_splitk_reduce (and unsplit), ragged last runs
    _c("ring64x128-unsplit", "ring<64,128,3>", 5, 32768, 4096, act=S, bias=True),
    _c("splitk2", "ring<64,128,3> splitk+reduce s2", 5, 16768, 4096, bias=True, res=True, ldr_pad=8),
    _c("splitk3-down", "ring<64,128,3> splitk+reduce s3", 391, 2048, 11008, res=True, ldr_pad=24, lda_pad=8),
    _c("splitk3-silu", "ring<64,128,3> splitk+reduce s3", 65, 6656, 4096, act=S, bias=True),
    _c("splitk4-f32", "ring<64,128,3> splitk+reduce s4", 5, 8192, 4096, bias=True, out_f32=True),
    _c("splitk5-relu", "ring<64,128,3> splitk+reduce s5", 5, 6660, 4160, act=R, bias=True, res=True, ldc_pad=3, ldr_pad=1),
    _c("splitk6", "ring<64,128,3> splitk+reduce s6", 129, 2048, 4096, bias=True, ldw_pad=8),
    _c("splitk7-gelu-res", "ring<64,128,3> splitk+reduce s7", 127, 2560, 4224, act=G, bias=True, res=True),
    _c("splitk8-ragged", "ring<64,128,3> splitk+reduce s8", 100, 2048, 5888, act=G, bias=True),
    # 64 < M <= 128: 128 x 128 ring and the <128, 96> SwiGLU tile (N % 96 = 32, 64, 0)
    _c("ring128x128", "ring<128,128,3>", 100, 16768, 2048, bias=True, res=True, ldr_pad=8),
    _c("ring128x128-gelu", "ring<128,128,3>", 65, 16388, 1024, act=G, bias=True, ldc_pad=4),
    _c("ring128x96-pool", "ring<128,96,3>", 100, 22016, 2048, act=SW),
    _c("ring128x96-n64", "ring<128,96,3>", 65, 8224, 1024, act=SW, bias=True, ldc_pad=4),
    _c("ring128x96-n0", "ring<128,96,3>", 128, 8256, 1024, act=SW, bias=True, lda_pad=8),
    # 256 x 256 two-phase kernel: coalesced LDS epilogue, the 32 x 32 fragment epilogue (ldc % 8 = 4), and the fall-back to 128 x 128
    _c("big", "p4<256,256>", 1300, 6656, 2048, bias=True, res=True, ldr_pad=8, lda_pad=8, ldw_pad=8),
    _c("big-k4-gelu", "p4<256,256>", 1281, 6408, 256, act=G, bias=True),
    _c("big-swiglu", "p4<256,256>", 1300, 6688, 1024, act=SW, bias=True),
    _c("big-silu-res", "p4<256,256>", 1279, 7944, 320, act=S, bias=True, res=True, ldr_pad=16),
    _c("big-frag-gelu-res", "p4<256,256> frag", 1300, 6660, 320, act=G, bias=True, res=True, ldc_pad=4, ldr_pad=4),
    _c("big-frag-swiglu", "p4<256,256> frag", 1025, 8200 * 2 - 16, 256, act=SW, bias=True, ldc_pad=4),
    _c("big-f32-falls-back", "glds<128,128>", 1300, 6656, 2048, bias=True, out_f32=True),
    _c("big-oddldc-falls-back", "glds<128,128>", 1300, 6656, 256, act=R, bias=True, ldc_pad=3),
    # M <= 4: the GEMV hand-off (results: tests/test_decode_linears_gpu.py)
    _c("gemv-handoff", "gemv", 4, 512, 512, bias=True),
    # fo1_gemm_bf16_partials: planes only
    _c("partials64x64", "ring<64,64,3> splitk planes s4", 33, 512, 1088, entry="partials", splits=4),
    _c("partials64x64-fewer", "ring<64,64,3> splitk planes s3", 70, 260, 576, entry="partials", splits=4, lda_pad=8, ldw_pad=8),
    _c("partials64x64-k1", "ring<64,64,3> splitk planes s6", 65, 132, 384, entry="partials", splits=6),
    _c("partials64x128", "ring<64,128,3> splitk planes s16", 100, 2048, 2048, entry="partials", splits=16),
    _c("partials128x256", "glds<128,256> splitk planes s3", 100, 8196, 1024, entry="partials", splits=3),
    # ---- pinned (A/B library) ------------------------------------------------------------------------------------------------------------
    _c("t7-r3", "ring<128,64,3>", 130, 200, 256, act=G, bias=True, pin=Pin(0, 7, 1)),
    _c("t7-r4", "ring<128,64,4>", 129, 132, 128, bias=True, res=True, ldr_pad=8, pin=Pin(4, 7, 1)),
    _c("t7-r6", "ring<128,64,6>", 100, 192, 320, act=S, bias=True, pin=Pin(6, 7, 1)),
    _c("t7-r6-splitk3", "ring<128,64,6> splitk+reduce s3", 100, 196, 512, act=R, bias=True, res=True, pin=Pin(0, 7, 3)),
    _c("t7-r3-splitk2", "ring<128,64,3> splitk+reduce s2", 257, 64, 192, bias=True, pin=Pin(3, 7, 2)),
    _c("t7-r4-splitk4", "ring<128,64,4> splitk+reduce s4", 128, 68, 448, bias=True, ldc_pad=4, pin=Pin(4, 7, 4)),
    _c("t7-partials", "ring<128,64,6> splitk planes s3", 100, 260, 576, entry="partials", splits=3, pin=Pin(0, 7, 0)),
    _c("t6-r4-swiglu", "ring<128,96,4>", 129, 224, 256, act=SW, bias=True, ldc_pad=4, pin=Pin(4, 6, 0)),
    _c("t6-r5-swiglu", "ring<128,96,5>", 100, 288, 192, act=SW, pin=Pin(5, 6, 0)),
    _c("t6-r3-gelu-res", "ring<128,96,3>", 127, 196, 128, act=G, bias=True, res=True, ldr_pad=8, pin=Pin(0, 6, 0)),
    _c("t3-r4", "ring<64,64,4>", 65, 130, 256, act=G, bias=True, ldc_pad=2, pin=Pin(4, 3, 1)),
    _c("t3-r6-k2", "ring<64,64,6>", 64, 128, 128, bias=True, res=True, ldr_pad=8, pin=Pin(6, 3, 1)),
    _c("t3-r6-splitk2", "ring<64,64,6> splitk+reduce s2", 63, 132, 704, act=S, bias=True, pin=Pin(6, 3, 2)),
    _c("t2-r4", "ring<64,128,4>", 65, 260, 320, act=R, bias=True, res=True, pin=Pin(4, 2, 1)),
    _c("t2-r6", "ring<64,128,4>", 128, 256, 192, act=SW, bias=True, pin=Pin(6, 2, 1)),
    _c("t1-r4", "ring<128,128,4>", 129, 132, 256, bias=True, res=True, ldr_pad=8, pin=Pin(4, 1, 1)),
    _c("t1-r6", "ring<128,128,4>", 255, 260, 192, act=G, bias=True, pin=Pin(6, 1, 1)),
    _c("t1-glds-splitk2", "glds<128,128> splitk+reduce s2", 130, 256, 320, act=G, bias=True, res=True, pin=Pin(2, 1, 2)),
    _c("t4-wide-splitk3", "glds<128,256> splitk+reduce s3", 129, 516, 448, act=S, bias=True, pin=Pin(2, 4, 3)),
    _c("t5-splitk2", "p4<256,256> splitk+reduce s2", 300, 520, 320, act=G, bias=True, res=True, ldr_pad=8, pin=Pin(0, 5, 2)),
    _c("t5-splitk3", "p4<256,256> splitk+reduce s3", 769, 264, 448, bias=True, pin=Pin(0, 5, 3)),
    _c("t5-p8", "p8<256,256>", 770, 520, 256, act=S, bias=True, res=True, ldr_pad=8, pin=Pin(0, 5, 1, sched=0)),
    _c("t5-p8-swiglu", "p8<256,256>", 257, 544, 128, act=SW, bias=True, pin=Pin(0, 5, 1, sched=0)),
    _c("t5-frag", "p4<256,256> frag", 513, 776, 192, act=G, bias=True, res=True, ldr_pad=8, pin=Pin(0, 5, 1, sched=3)),
    _c("t5-small-k1", "p4<256,256>", 255, 256, 64, bias=True, pin=Pin(0, 5, 1)),
    _c("t5-group3", "p4<256,256>", 1100, 1288, 128, act=S, bias=True, pin=Pin(0, 5, 1, group_m=3)),
    _c("t5-persistent", "p4p<256,256>", 700, 21896, 128, act=G, bias=True, res=True, ldr_pad=8, pin=Pin(0, 5, 1, sched=5)),
    _c("wtiled128", "ring<128,128,3>", 100, 384, 256, act=G, bias=True, res=True, ldr_pad=8, entry="wtiled"),
    _c("wtiled64", "ring<64,128,3>", 33, 256, 192, act=SW, bias=True, entry="wtiled"),
]


def scale_down(c: Case) -> Case:
    """The same case with at most two tiles each way — one full, one as ragged as the original's last — and the original's route: what
    tests/test_gemm_route_cases.py can afford in float64 on the CPU.  K, and so the K order, is unchanged."""
    r = case_route(c)
    if r.kind == "gemv":
        return c
    M = c.M if c.M <= 2 * r.BM else r.BM + (c.M - 1) % r.BM + 1
    N = c.N if c.N <= 2 * r.BN else r.BN + (c.N - 1) % r.BN + 1
    return replace(c, M=M, N=N, M0=c.M, N0=c.N)


# ---------------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def planted(K: int, r: Route) -> Tuple[Dict[int, int], int]:
    """-> ({planted k: sign of its chunk}, k of the checkerboard column)."""
    pos = {0, 7, 8, K - 9, K - 8, K - 1}
    if K >= 128:
        pos |= {63, 64}
    if r.splits > 1:
        for z in range(1, r.splits):
            pos |= {z * r.kper * 64 - 1, z * r.kper * 64}
    if K % 64:
        pos |= {K - K % 64 - 1, K - K % 64}
    pos = {p for p in pos if 0 <= p < K}
    chunks = sorted({p // 8 for p in pos})
    free = [c for c in range(K // 8) if c not in chunks]
    if len(chunks) % 2 and free:
        pos.add(free[len(free) // 2] * 8 + 3)
        chunks = sorted({p // 8 for p in pos})
        free = [c for c in range(K // 8) if c not in chunks]
    sign = {c: (1 if i % 2 == 0 else -1) for i, c in enumerate(chunks)}
    return {p: sign[p // 8] for p in sorted(pos)}, (free[0] * 8 + 5 if free else -1)


def _levels(n: int) -> torch.Tensor:
    i = torch.arange(n)
    return (1.0 + (i % 4) / 4.0) * torch.where((i // 4) % 2 == 0, 1.0, -1.0)


PLANT = 1.0          # amplitude of the planted columns (tests/test_gemm_route_cases.py: at 0 the fault half fails)


def bias_pattern(N: int) -> torch.Tensor:
    """A per-column ramp with a jump at every 16- and 32-column fragment boundary."""
    n = torch.arange(N)
    return (0.015625 * (n % 16) + 0.5 * ((n // 16) % 5) - 1.0 + 0.25 * ((n // 32) % 2)).bfloat16()


def res_pattern(M: int, N: int) -> torch.Tensor:
    """Differs between (m, n), (m, n +- 1) and (m +- 1, n)."""
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    return ((((3 * m + 5 * n) % 7) - 3) * 0.25 + ((m + n) % 2) * 0.125).bfloat16()


def build(c: Case) -> dict:
    r = case_route(c)
    g = torch.Generator().manual_seed(c.seed)
    A = (torch.randn(c.M, c.K, generator=g) * 0.5).bfloat16()
    W = (torch.randn(c.N, c.K, generator=g) * 0.05).bfloat16()
    pos, checker = planted(c.K, r)
    per_chunk: Dict[int, int] = {}
    for p in pos:
        per_chunk[p // 8] = per_chunk.get(p // 8, 0) + 1
    s, t = _levels(c.M), _levels(c.N)
    for p, sg in pos.items():
        A[:, p] = (sg * 2.0 * PLANT / per_chunk[p // 8] * s).bfloat16()
        W[:, p] = (0.5 * t).bfloat16()
    if checker >= 0:
        A[:, checker] = (2.0 * PLANT * (1 - 2 * (torch.arange(c.M) % 2))).bfloat16()
        W[:, checker] = (0.5 * (1 - 2 * (torch.arange(c.N) % 2))).bfloat16()
    d = dict(case=c, route=r, A=A, W=W, pos=pos, checker=checker, bias=None, res=None)
    if c.bias:
        d["bias"] = bias_pattern(c.N)
    if c.res:
        d["res"] = res_pattern(c.M, c.N)
    return d


def host_buffers(d: dict) -> dict:
    """The over-allocated buffers of the launch, on the CPU: NaN outside the operands, the canary in every output element."""
    c = d["case"]
    nan = float("nan")
    A = torch.full((c.M + SPARE_OPERAND_ROWS, c.K + c.lda_pad), nan, dtype=torch.bfloat16)
    W = torch.full((c.N + SPARE_OPERAND_ROWS, c.K + c.ldw_pad), nan, dtype=torch.bfloat16)
    A[:c.M, :c.K] = d["A"]
    W[:c.N, :c.K] = d["W"]
    b = dict(A=A, W=W)
    if d["bias"] is not None:
        b["bias"] = torch.cat([d["bias"], torch.full((16,), nan, dtype=torch.bfloat16)])
    if d["res"] is not None:
        b["res"] = torch.full((c.M + SPARE_OPERAND_ROWS, c.ldr), nan, dtype=torch.bfloat16)
        b["res"][:c.M, :c.N] = d["res"]
    if c.entry == "partials":
        b["out"] = torch.full((d["route"].splits + 1, c.M, c.N), CANARY32, dtype=torch.int32).view(torch.float32)
    elif c.out_f32:
        b["out"] = torch.full((c.M + SPARE_ROWS, c.ldc), CANARY32, dtype=torch.int32).view(torch.float32)
    else:
        b["out"] = torch.full((c.M + SPARE_ROWS, c.ldc), CANARY16, dtype=torch.int16).view(torch.bfloat16)
    return b


def to_device(d: dict, device="cuda") -> dict:
    return {k: v.to(device) for k, v in host_buffers(d).items()}


def check_canary(buf: torch.Tensor, d: dict, what: str) -> None:
    c = d["case"]
    bits = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16)
    can = CANARY32 if buf.dtype == torch.float32 else CANARY16
    if c.entry == "partials":
        planes = d["route"].splits
        assert not (bits[:planes] == can).any(), f"{what}: {int((bits[:planes] == can).sum())} plane elements never written"
        assert (bits[planes:] == can).all(), f"{what}: the plane past the last one was written"
        return
    inside = bits[:c.M, :c.n_out] == can
    assert not inside.any(), f"{what}: {int(inside.sum())} output elements never written, first at {inside.nonzero()[0].tolist()}"
    out = bits != can
    out[:c.M, :c.n_out] = False
    assert not out.any(), f"{what}: {int(out.sum())} elements outside [0, {c.M}) x [0, {c.n_out}) written, first at {out.nonzero()[0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# reference, bound, emulation
# ---------------------------------------------------------------------------------------------------------------------------------------
def runs(d: dict) -> List[Tuple[int, int]]:
    """[k0, k1) of every split-K run (one run when unsplit)."""
    r, K = d["route"], d["case"].K
    if r.splits <= 1:
        return [(0, K)]
    return [(z * r.kper * 64, min(K, (z + 1) * r.kper * 64)) for z in range(r.splits)]


def _act64(x: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if act == ACT_SILU:
        return x * torch.sigmoid(x)
    if act == ACT_RELU:
        return x.clamp_min(0.0)
    return x


EXACT_ULP = False     # epilogue64(..., exact_ulp=True): the half ulp of the value's own binade instead of 2^-8 |value| (up to 2 x smaller)


def _rnd(e: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """Error after a bf16 rounding of a value v known to within e."""
    if EXACT_ULP:
        return e + torch.exp2(torch.floor(torch.log2((v.abs() + e).clamp_min(2.0 ** -126))) - 8.0)
    return e + HALF_ULP * (v.abs() + e)


def epilogue64(c: Case, Z: torch.Tensor, Sabs: torch.Tensor, bias, res, acc: float = ACC, exact_ulp: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(output, bound) in float64 from the accumulator Z = A W^T and Sabs = |A| |W|^T; bias [N] or [M, N], res [M, N] or None.
    exact_ulp (the CPU test's sharper form): every rounding point costs the half ulp of the binade the value lies in."""
    global EXACT_ULP
    if exact_ulp:
        EXACT_ULP = True
        try:
            return epilogue64(c, Z, Sabs, bias, res, acc)
        finally:
            EXACT_ULP = False
    x = Z if bias is None else Z + bias
    e = acc * 2.0 ** -24 * (Sabs if bias is None else Sabs + bias.abs())
    if c.out_f32:
        y = _act64(x, c.act)
        if c.act == ACT_GELU:
            e = GELU_SLOPE * e + 2.0 ** -21 * x.abs()
        elif c.act != ACT_NONE:
            raise ValueError("fp32 output: cases use no activation or GELU")
        return y, e
    e = _rnd(e, x)
    if c.act == ACT_SWIGLU:
        M, N = x.shape
        x4, e4 = x.view(M, N // 32, 2, 16), e.view(M, N // 32, 2, 16)
        g, u, eg, eu = x4[:, :, 0], x4[:, :, 1], e4[:, :, 0], e4[:, :, 1]
        sg = _act64(g, ACT_SILU)
        es = _rnd(SILU_SLOPE * eg, sg)
        y = sg * u
        e = _rnd(u.abs() * es + sg.abs() * eu + es * eu, y)
        return y.reshape(M, N // 2), e.reshape(M, N // 2)
    y = x
    if c.act != ACT_NONE:
        y = _act64(x, c.act)
        e = _rnd({ACT_GELU: GELU_SLOPE, ACT_SILU: SILU_SLOPE, ACT_RELU: 1.0}[c.act] * e, y)
    if res is not None:
        y = y + res
        e = _rnd(e, y)
    return y, e


def accumulators(d: dict, device="cpu", rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Z, Sabs) in float64: [M, N], or [planes, M, N] for the partials entry.  rows: a subset of A's rows."""
    c = d["case"]
    A = d["A"].to(device).double()
    W = d["W"].to(device).double()
    if rows is not None:
        A = A[rows.to(device)]
    if c.entry != "partials":
        return A @ W.t(), A.abs() @ W.abs().t()
    Z = torch.stack([A[:, k0:k1] @ W[:, k0:k1].t() for k0, k1 in runs(d)])
    Sabs = torch.stack([A[:, k0:k1].abs() @ W[:, k0:k1].abs().t() for k0, k1 in runs(d)])
    return Z, Sabs


def reference_and_bound(d: dict, device="cpu", rows: Optional[torch.Tensor] = None, acc: float = ACC, exact_ulp: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    c = d["case"]
    Z, Sabs = accumulators(d, device, rows)
    if c.entry == "partials":
        return Z, acc * 2.0 ** -24 * Sabs
    bias = None if d["bias"] is None else d["bias"].to(device).double()
    res = None if d["res"] is None else d["res"].to(device).double()
    if res is not None and rows is not None:
        res = res[rows.to(device)]
    return epilogue64(c, Z, Sabs, bias, res, acc, exact_ulp)


def sample_rows(d: dict) -> torch.Tensor:
    """First, last, and the rows on either side of every M-tile boundary: checked against the CPU product when the reference is the device's."""
    c, r = d["case"], d["route"]
    rows = {0, c.M - 1}
    for b in range(r.BM, c.M, r.BM):
        rows |= {b - 1, b}
    return torch.tensor(sorted(rows))


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.bfloat16().float()


def emulate_acc(d: dict) -> torch.Tensor:
    """fp32 accumulators in the kernels' K order: [planes, M, N] (one plane when unsplit)."""
    A, W = d["A"].float(), d["W"].float()
    planes = []
    for k0, k1 in runs(d):
        acc = torch.zeros(A.shape[0], W.shape[0])
        for k in range(k0, k1, 16):
            acc += A[:, k:min(k + 16, k1)] @ W[:, k:min(k + 16, k1)].t()
        planes.append(acc)
    return torch.stack(planes)


def emulate(d: dict) -> torch.Tensor:
    c = d["case"]
    P = emulate_acc(d)
    if c.entry == "partials":
        return P.double()
    v = P[0]
    for z in range(1, P.shape[0]):
        v = v + P[z]
    if d["bias"] is not None:
        v = v + d["bias"].float()
    if c.out_f32:
        return _act64(v.double(), c.act).float().double()
    v = _bf(v)
    if c.act == ACT_SWIGLU:
        v4 = v.view(c.M, c.N // 32, 2, 16)
        g, u = v4[:, :, 0], v4[:, :, 1]
        return _bf(_bf(_act64(g.double(), ACT_SILU).float()) * u).reshape(c.M, c.N // 2).double()
    if c.act != ACT_NONE:
        v = _bf(_act64(v.double(), c.act).float())
    if d["res"] is not None:
        v = _bf(v + d["res"].float())
    return v.double()


def acc_error(d: dict) -> float:
    """The emulation's worst fp32 accumulation error (after the z-ordered plane sum) in units of 2^-24 S."""
    c = d["case"]
    P = emulate_acc(d)
    Z, Sabs = accumulators(d)
    if c.entry != "partials":
        v = P[0]
        for z in range(1, P.shape[0]):
            v = v + P[z]
        P = v
    return ((P.double() - Z).abs() / (2.0 ** -24 * Sabs)).max().item()


# ---------------------------------------------------------------------------------------------------------------------------------------
# faults
# ---------------------------------------------------------------------------------------------------------------------------------------
FAULTS = (
    # one planted 16-byte K chunk of the last (ragged) tile dropped / read twice: the first and last chunk, either side of the first K-tile
    # boundary, either side of the last split-K run boundary, the first chunk of the register route's K % 64 tail
    "drop_chunk:first", "dup_chunk:first", "drop_chunk:last", "dup_chunk:last", "drop_chunk:tile_lo", "dup_chunk:tile_lo", "drop_chunk:tile_hi",
    "dup_chunk:tile_hi", "drop_chunk:run_lo", "dup_chunk:run_lo", "drop_chunk:run_hi", "dup_chunk:run_hi", "drop_chunk:tail", "dup_chunk:tail",
    "drop_last_plane", "dup_last_plane",        # the reduce leaves the last split-K plane out of the last tile's sum, or adds it twice
    "row_last_unwritten", "row_last_from_prev",     # row M - 1 not stored, or computed from A's row M - 2
    "col_last_unwritten", "col_last_from_prev",     # the last output column not stored, or computed from W's row N - 2
    "bias_shift16",             # the bias of the fragment 16 columns over (first column tile of the last tile row)
    "res_ldc",                  # the residual read with ldc for ldr (last tile row)
    "swiglu_swap", "swiglu_next_up",        # gate and up swapped inside a 32-column group; the up half taken from the next group
    "tile_transposed",          # tile (0, 1) stored at tile coordinate (1, 0)
    "lda_eq_K",                 # A read with lda = K when lda > K (last tile row)
)


def _chunk_of(d: dict, where: str) -> int:
    c, r = d["case"], d["route"]
    K = c.K
    if where == "first":
        return 0
    if where == "last":
        return (K - 1) // 8
    if where in ("tile_lo", "tile_hi"):
        return -1 if K < 128 else (7 if where == "tile_lo" else 8)
    if where in ("run_lo", "run_hi"):
        if r.splits <= 1:
            return -1
        b = (r.splits - 1) * r.kper * 64
        return (b - 1) // 8 if where == "run_lo" else b // 8
    if where == "tail":
        return -1 if K % 64 == 0 else (K - K % 64) // 8
    raise ValueError(where)


def tiles(d: dict) -> Tuple[int, int]:
    c, r = d["case"], d["route"]
    return cdiv(c.M, r.BM), cdiv(c.N, r.BN)


def _tile(d: dict, tm: int, tn: int) -> Tuple[slice, slice]:
    c, r = d["case"], d["route"]
    return slice(tm * r.BM, min(c.M, (tm + 1) * r.BM)), slice(tn * r.BN, min(c.N, (tn + 1) * r.BN))


def applicable_faults(d: dict) -> List[str]:
    c, r = d["case"], d["route"]
    tm, tn = tiles(d)
    part = c.entry == "partials"
    out = []
    for f in FAULTS:
        kind, _, where = f.partition(":")
        if kind in ("drop_chunk", "dup_chunk"):
            ok = _chunk_of(d, where) >= 0
        elif kind in ("drop_last_plane", "dup_last_plane"):
            ok = r.splits > 1 and not part
        elif kind == "row_last_from_prev":
            ok = c.M >= 2
        elif kind == "col_last_from_prev":
            ok = c.act != ACT_SWIGLU
        elif kind == "bias_shift16":
            ok = c.bias and c.N > 16
        elif kind == "res_ldc":
            ok = c.res and c.ldr != c.ldc and c.M >= 2
        elif kind in ("swiglu_swap", "swiglu_next_up"):
            ok = c.act == ACT_SWIGLU and (kind == "swiglu_swap" or c.N >= 64)
        elif kind == "tile_transposed":
            ok = tm >= 2 and tn >= 2
        elif kind == "lda_eq_K":
            ok = c.lda_pad > 0 and c.M >= 2
        else:
            ok = True
        if ok:
            out.append(f)
    return out


def reference(d: dict, fault: Optional[str] = None):
    """The float64 output.  With a fault: (the output the faulty kernel would leave — NaN where it reads the operands' NaN padding, the canary
    value where it stores nothing — and the tiles (row slice, column slice in OUTPUT columns; partials: plane too) the fault touches)."""
    c, r = d["case"], d["route"]
    if fault is None:
        return reference_and_bound(d)[0]
    Z, Sabs = accumulators(d)
    part = c.entry == "partials"
    ntm, ntn = tiles(d)
    bias = None if d["bias"] is None else d["bias"].double()[None, :].expand(c.M, c.N).clone()
    res = None if d["res"] is None else d["res"].double().clone()
    A, W = d["A"].double(), d["W"].double()
    unwritten = torch.zeros(c.M, c.N, dtype=torch.bool)
    touched: List[Tuple[int, int]] = []
    plane = None
    kind, _, where = fault.partition(":")
    rs, cs = _tile(d, ntm - 1, ntn - 1)
    last_row_tiles = [(ntm - 1, j) for j in range(ntn)]
    if kind in ("drop_chunk", "dup_chunk"):
        ch = _chunk_of(d, where)
        delta = A[rs, ch * 8:ch * 8 + 8] @ W[cs, ch * 8:ch * 8 + 8].t()
        sign = -1.0 if kind == "drop_chunk" else 1.0
        if part:
            plane = [z for z, (k0, k1) in enumerate(runs(d)) if k0 <= ch * 8 < k1][0]
            Z[plane, rs, cs] += sign * delta
        else:
            Z[rs, cs] += sign * delta
        touched = [(ntm - 1, ntn - 1)]
    elif kind in ("drop_last_plane", "dup_last_plane"):
        k0, k1 = runs(d)[-1]
        Z[rs, cs] += (-1.0 if kind == "drop_last_plane" else 1.0) * (A[rs, k0:k1] @ W[cs, k0:k1].t())
        touched = [(ntm - 1, ntn - 1)]
    elif kind == "row_last_unwritten":
        unwritten[c.M - 1, :] = True
        touched = last_row_tiles
    elif kind == "row_last_from_prev":
        Z[..., c.M - 1, :] = Z[..., c.M - 2, :]
        touched = last_row_tiles
    elif kind == "col_last_unwritten":
        unwritten[:, c.N - 1] = True
        if c.act == ACT_SWIGLU:
            unwritten[:, c.N - 17] = True
        touched = [(i, ntn - 1) for i in range(ntm)]
    elif kind == "col_last_from_prev":
        Z[..., :, c.N - 1] = Z[..., :, c.N - 2]
        touched = [(i, ntn - 1) for i in range(ntm)]
    elif kind == "bias_shift16":
        rs0, cs0 = _tile(d, ntm - 1, 0)
        idx = (torch.arange(cs0.start, cs0.stop) + 16).clamp_max(c.N - 1)
        bias[rs0, cs0] = d["bias"].double()[idx][None, :]
        touched = [(ntm - 1, 0)]
    elif kind == "res_ldc":
        flat = host_buffers(d)["res"].double().flatten()
        m = torch.arange(rs.start, rs.stop)[:, None]
        res[rs, :] = flat[(m * c.ldc + torch.arange(c.N)[None, :]).clamp_max(flat.numel() - 1)]
        touched = last_row_tiles
    elif kind == "swiglu_swap":
        n0 = (c.N - 1) // 32 * 32
        Z[rs, n0:n0 + 32] = torch.cat([Z[rs, n0 + 16:n0 + 32], Z[rs, n0:n0 + 16]], dim=1)
        if bias is not None:
            bias[rs, n0:n0 + 32] = torch.cat([bias[rs, n0 + 16:n0 + 32], bias[rs, n0:n0 + 16]], dim=1)
        touched = [(ntm - 1, ntn - 1)]
    elif kind == "swiglu_next_up":
        rs0, _ = _tile(d, ntm - 1, 0)
        Z[rs0, 16:32] = Z[rs0, 48:64]
        if bias is not None:
            bias[rs0, 16:32] = bias[rs0, 48:64]
        touched = [(ntm - 1, 0)]
    elif kind == "lda_eq_K":
        flat = host_buffers(d)["A"].double().flatten()
        m = torch.arange(rs.start, rs.stop)[:, None]
        Abad = flat[m * c.K + torch.arange(c.K)[None, :]]
        Zbad = Abad @ W.t()
        if part:
            Zbad = torch.stack([Abad[:, k0:k1] @ W[:, k0:k1].t() for k0, k1 in runs(d)])
        Z[..., rs, :] = Zbad
        touched = last_row_tiles
    elif kind == "tile_transposed":
        touched = [(0, 1), (1, 0)]
    else:
        raise ValueError(fault)
    canary = torch.tensor([CANARY32], dtype=torch.int32).view(torch.float32).double().item()
    if part:
        out = Z.clone()
    else:
        out = epilogue64(c, Z, Sabs, bias, res)[0]
    half = 2 if c.act == ACT_SWIGLU else 1

    def ocols(s: slice) -> slice:
        if c.act != ACT_SWIGLU:
            return s
        return slice(s.start // 2, s.start // 2 + (s.stop - s.start) // 2)

    if kind == "tile_transposed":
        (r0, c0), (r1, c1) = _tile(d, 0, 1), _tile(d, 1, 0)
        c0, c1 = ocols(c0), ocols(c1)
        src = out[..., r0, c0].clone()
        out[..., r0, c0] = canary
        h = min(src.shape[-2], r1.stop - r1.start)
        w = min(src.shape[-1], c1.stop - c1.start)
        out[..., r1.start:r1.start + h, c1.start:c1.start + w] = src[..., :h, :w]
    if unwritten.any():
        if c.act == ACT_SWIGLU:
            uw = unwritten.view(c.M, c.N // 32, 2, 16)[:, :, 0].reshape(c.M, c.N // 2) | unwritten.view(c.M, c.N // 32, 2, 16)[:, :, 1].reshape(c.M, c.N // 2)
        else:
            uw = unwritten
        out = torch.where(uw, torch.full_like(out, canary), out)
    regions = []
    for i, j in touched:
        rr, cc = _tile(d, i, j)
        regions.append((plane, rr, ocols(cc)))
    return out, regions


def region_worst(mut: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, region) -> float:
    """The largest |mut - ref| / bound over a touched tile (NaN counts as infinite)."""
    plane, rr, cc = region
    if plane is not None:
        mut, ref, bound = mut[plane], ref[plane], bound[plane]
    q = ((mut[..., rr, cc] - ref[..., rr, cc]).abs() / bound[..., rr, cc])
    return torch.nan_to_num(q, nan=float("inf")).max().item()
