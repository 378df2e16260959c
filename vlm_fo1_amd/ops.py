"""Thin torch-tensor front ends for the C-ABI ops in libfo1hip.so (include/fo1.h).

torch is only the allocator / stream owner here: every function validates layouts, allocates the
output with torch.empty and enqueues the HIP kernel(s) on the current stream.  No function has a
PyTorch fallback; a missing library or a CPU tensor raises."""
from __future__ import annotations

import math
import itertools
import os
import threading
from typing import NamedTuple, Optional, Sequence

import ctypes

import torch

from . import lib as _L

ACT_NONE, ACT_GELU, ACT_SILU, ACT_SWIGLU16, ACT_RELU = 0, 1, 2, 3, 5


def _chk(t: torch.Tensor, name: str, dtype=torch.bfloat16):
    if t.device.type != "cuda":
        raise _L.Fo1Error(f"{name}: expected a HIP device tensor, got {t.device}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _rows(t: torch.Tensor, name: str):
    """2-D view [M, D] with unit inner stride -> (ptr, ld, M, D)."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a 2-D row-major tensor, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr(), t.stride(0), t.shape[0], t.shape[1]


def _ptr(t: Optional[torch.Tensor]):
    """Optional tensor -> device pointer, or None (a NULL operand)."""
    return None if t is None else t.data_ptr()


def _residual(residual: Optional[torch.Tensor], check: bool = False):
    """Optional residual rows -> (pointer, row stride), (None, 0) without one."""
    if residual is None:
        return None, 0
    if check:
        _chk(residual, "residual")
    pr, ldr, _, _ = _rows(residual, "residual")
    return pr, ldr


def _out_rows(out: Optional[torch.Tensor], rows: int, cols: int, device) -> torch.Tensor:
    """A new [rows, cols] bf16 output, or the caller's `out` checked to be such a row-major view (its row stride may be padded)."""
    if out is None:
        return torch.empty(rows, cols, dtype=torch.bfloat16, device=device)
    _chk(out, "out")
    if tuple(out.shape) != (rows, cols) or out.stride(1) != 1:
        raise ValueError(f"out: need a row-major [{rows}, {cols}] view, got shape {tuple(out.shape)} strides {out.stride()}")
    return out


def _stream():
    return _L.current_stream_ptr()


# ---- caller-owned scratch (the library never allocates) ----------------------------------------------------------------
# One buffer per (kind, device, owner, size class).  `owner` is set by an engine for the duration of its device work
# (`workspace_scope`): replicas running on different streams — and the hipGraphs they captured, which hold raw pointers —
# must never share partial-sum scratch.  Outside any scope the key falls back to the current stream.  Buffers are never
# freed or resized in place: a captured graph may still reference them.
_ws_pool = {}
_ws_tls = threading.local()


class _CaptureLock:
    """hipGraph capture (and the eager warm-up pass before it) is exclusive; graph replays from other request threads are
    shared.  Concurrent stream captures from several host threads crash inside the runtime (segfault in capture_end on
    ROCm 7.2); replays only hold the lock for the host-side launch call, so the GPU work still overlaps."""

    def __init__(self):
        self._cond = threading.Condition()
        self._readers = 0
        self._writer = False

    class _Side:
        def __init__(self, enter, leave):
            self._enter, self._leave = enter, leave

        def __enter__(self):
            self._enter()

        def __exit__(self, *exc):
            self._leave()
            return False

    def _r_in(self):
        with self._cond:
            while self._writer:
                self._cond.wait()
            self._readers += 1

    def _r_out(self):
        with self._cond:
            self._readers -= 1
            if self._readers == 0:
                self._cond.notify_all()

    def _w_in(self):
        with self._cond:
            while self._writer or self._readers:
                self._cond.wait()
            self._writer = True

    def _w_out(self):
        with self._cond:
            self._writer = False
            self._cond.notify_all()

    def replay(self):
        return self._Side(self._r_in, self._r_out)

    def capture(self):
        return self._Side(self._w_in, self._w_out)


graph_lock = _CaptureLock()


def capture_graph(run, rollback: Sequence[torch.Tensor] = ()):
    """The one recipe every hipGraph of the package is captured with -> (graph, what the captured `run()` returned: static
    buffers of the graph).  `run` enqueues the work on the current stream and is called twice: an eager warm-up, then under
    capture.  `rollback` names the persistent tensors the work updates in place (a decode step's state, plan, ids, done
    counter): they are restored after the warm-up, so the capture starts from, and the caller's first replay executes, the
    step the caller asked for.  What `rollback` does not name stays as the warm-up left it.  Static INPUTS are the caller's:
    cloned before the call, under the caller's own torch.inference_mode(False), and refreshed in place before each replay.
    The helper owns no cache, and when `run` raises the lock and the mode are released and nothing else is undone."""
    # * graph_lock.capture(): exclusive against every other capture, warm-up and replay of the process (_CaptureLock).
    # * inference mode OFF: the CUDA generator's graph bookkeeping tensors are created by the first live capture and updated in
    #   place by later ones — if the first ran under the caller's torch.inference_mode() (the reference's inference.py:46) a
    #   later capture outside it fails ("Inplace update to inference tensor outside InferenceMode"); and what `run` returns
    #   must be ordinary tensors, the callers hand them out for the life of the graph.
    with graph_lock.capture(), torch.inference_mode(False):
        snap = [t.clone() for t in rollback]
        # warm-up on a fresh side stream: every lazily created scratch buffer (_workspace, zero_framed, plans) exists before
        # the capture — an allocation inside a capture would land in the graph's private pool, or fail it
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for t, t0 in zip(rollback, snap):      # once: the capture below executes nothing, so there is nothing to undo after it
            t.copy_(t0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):   # RCCL watchdog threads may touch the runtime meanwhile
            out = run()
    return g, out


def replay_graph(g) -> None:
    """Launch a captured graph on the current stream: shared with other replays, excluded by a capture (_CaptureLock)."""
    with graph_lock.replay():
        g.replay()


SEEN_MAX = 4096      # signatures whose sightings are remembered (a dataset has thousands of distinct image sizes)


def seen_enough(seen: dict, key, after: int) -> bool:
    """Capture policy of the engines' graph caches: is this sighting of `key` the one to capture on?  A signature runs eagerly
    `after` times (one-off shapes never pay a capture) and is captured on the next sighting — also every later one, should its
    graph have been evicted meanwhile.  `seen` counts the eager sightings; at SEEN_MAX keys the oldest is dropped."""
    n = seen.get(key, 0)
    if n >= after:
        return True
    if len(seen) >= SEEN_MAX:
        seen.pop(next(iter(seen)))
    seen[key] = n + 1
    return False


def lru_put(cache, key, value, cap: int):
    """Insert into an OrderedDict kept as an LRU of `cap` entries (a hit is cache.move_to_end(key)) -> value.  An evicted graph's
    private pool is released with it."""
    cache[key] = value
    while len(cache) > cap:
        cache.popitem(last=False)
    return value


class workspace_scope:
    def __init__(self, owner):
        self.owner = owner

    def __enter__(self):
        self.prev = getattr(_ws_tls, "owner", None)
        _ws_tls.owner = self.owner
        return self

    def __exit__(self, *exc):
        _ws_tls.owner = self.prev
        return False


class keep_scope:
    """While active on this thread, host objects that own device index tables handed to launches (plans evicted from bounded caches:
    Conv3x3Plan) are appended to `keep` — the list a packed pass returns with its result and a captured hipGraph of that pass is stored
    with, so the tables outlive their cache entry for as long as a graph can replay launches that point at them (ADVICE r3's rule for
    the ragged tower plans, applied to the uniform paths' convolution plans)."""

    def __init__(self, keep: list):
        self.keep = keep

    def __enter__(self):
        self.prev = getattr(_ws_tls, "keep", None)
        _ws_tls.keep = self.keep
        return self

    def __exit__(self, *exc):
        _ws_tls.keep = self.prev
        return False


def keep_alive(obj) -> None:
    keep = getattr(_ws_tls, "keep", None)
    if keep is not None and not any(o is obj for o in keep):
        keep.append(obj)


def _workspace(kind: str, device, nbytes: int) -> torch.Tensor:
    owner = getattr(_ws_tls, "owner", None)
    who = ("owner", owner) if owner is not None else ("stream", torch.cuda.current_stream().cuda_stream)
    size = 1 << max(12, int(nbytes - 1).bit_length())      # power-of-two size classes
    key = (kind, device, who, size)
    ws = _ws_pool.get(key)
    if ws is None:
        ws = torch.zeros(size, dtype=torch.uint8, device=device)   # zeroed once: decode attention keeps arrival counters in its tail
        _ws_pool[key] = ws
    return ws


_zero_framed_kinds: dict = {}
_zero_framed_lock = threading.Lock()
ZERO_FRAMED_MAX = 48       # distinct persistent zero-framed buffers per process (each lives as long as its owner: a captured pass holds its raw pointer)


def zero_framed(key: tuple, rows: int, cols: int, device) -> torch.Tensor:
    """[rows, cols] bf16 scratch whose elements the caller NEVER writes are zero — the frame of a zero-padded convolution input, the padding
    columns of a V^T map.  `key` must determine which elements get written (a plan's serial number, a shape): the buffer is then zeroed once,
    at its first use, instead of by a fill launch per pass (8 fills = 0.25 ms of the 25-image pass).  One buffer per (key, engine replica /
    stream) from the scratch pool; past ZERO_FRAMED_MAX distinct keys (a server seeing ever new geometries) a fresh torch.zeros, as before."""
    if os.environ.get("FO1_ZERO_FRAMED", "1") != "0":
        with _zero_framed_lock:
            kind = _zero_framed_kinds.get(key)
            if kind is None and len(_zero_framed_kinds) < ZERO_FRAMED_MAX:
                kind = _zero_framed_kinds[key] = f"zero_framed_{len(_zero_framed_kinds)}"
        if kind is not None:
            nbytes = rows * cols * 2
            return _workspace(kind, device, nbytes)[:nbytes].view(torch.bfloat16).view(rows, cols)
    return torch.zeros(rows, cols, dtype=torch.bfloat16, device=device)


def release_workspaces(owner) -> int:
    """Drop every scratch buffer keyed by `owner` (an engine / decoder that is gone: its graphs, the only other holders of the raw
    pointers, went with it).  Returns the number of buffers released."""
    dead = [k for k in _ws_pool if k[2] == ("owner", owner)]
    for k in dead:
        del _ws_pool[k]
    return len(dead)


def new_owner(holder):
    """A scratch-pool owner token whose buffers are released when `holder` (the engine / decoder using it) is collected: repeated
    engine or replica creation must not leak device memory."""
    import weakref
    token = object()
    weakref.finalize(holder, release_workspaces, token)
    return token


def _gemm_workspace(device) -> torch.Tensor:
    """fp32 scratch for split-K partials, 64 MiB."""
    return _workspace("gemm", device, 64 * 1024 * 1024)


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         act: int = ACT_NONE, out: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """out[M,N] = epilogue(a[M,K] @ w[N,K]^T)  (nn.Linear semantics, fo1_gemm_bf16)."""
    _chk(a, "a"); _chk(w, "w")
    pa, lda, M, K = _rows(a, "a")
    pw, ldw, N, K2 = _rows(w, "w")
    if K != K2:
        raise ValueError(f"gemm: K mismatch {K} vs {K2}")
    n_out = N // 2 if act == ACT_SWIGLU16 else N
    if out is None:
        out = torch.empty(M, n_out, dtype=torch.float32 if out_f32 else torch.bfloat16, device=a.device)
    po, ldc, Mo, No = _rows(out, "out")
    assert (Mo, No) == (M, n_out)
    pr, ldr = _residual(residual, check=True)
    assert residual is None or tuple(residual.shape) == (M, N)
    if bias is not None:
        _chk(bias, "bias")
        assert bias.numel() == N and bias.is_contiguous()
    if _fp8_weights and not out_f32 and M >= FP8_MIN_ROWS:
        fw = _fp8_weights.get((pw, N, K))
        if fw is not None:
            aq, sa = quantize_rows_fp8(a)
            return gemm_fp8(aq, sa, fw, bias, residual, act, out)
    ws = _gemm_workspace(a.device)
    rc = _L.load().fo1_gemm_bf16_ws(pa, lda, pw, ldw, _ptr(bias), pr, ldr, po, ldc,
                                    M, N, K, act, 1 if out_f32 else 0, ws.data_ptr(), ws.numel(), _stream())
    _L.check(rc, "fo1_gemm_bf16_ws")
    return out


# ---- fp8 linear (BASELINE configs[4]) ---------------------------------------------------------------------------------------
class Fp8Weight:
    """Per-output-channel e4m3 copy of an nn.Linear weight: q uint8 [N, K], scale fp32 [N].  `src` keeps the bf16 tensor it was made
    from alive: the routing table is keyed by that tensor's address, which must not be handed to another allocation meanwhile."""
    __slots__ = ("q", "scale", "src")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor, src: Optional[torch.Tensor] = None):
        self.q, self.scale, self.src = q, scale, src


_fp8_weights = {}            # (data_ptr, N, K) of a registered bf16 weight -> Fp8Weight
FP8_MIN_ROWS = 512           # below this the 256 x 256 fp8 tile is mostly padding: the bf16 kernels run


def quantize_rows_fp8(x: torch.Tensor, q: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None):
    """(q uint8 [M, K], scales fp32 [M]) = row-wise e4m3 quantisation of a bf16 matrix (fo1_quantize_rows_e4m3)."""
    _chk(x, "x")
    px, ldx, M, K = _rows(x, "x")
    if q is None:
        q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    if scales is None:
        scales = torch.empty(M, dtype=torch.float32, device=x.device)
    _L.check(_L.load().fo1_quantize_rows_e4m3(px, ldx, M, K, q.data_ptr(), q.stride(0), scales.data_ptr(), _stream()), "fo1_quantize_rows_e4m3")
    return q, scales


def gemm_fp8(aq: torch.Tensor, sa: torch.Tensor, w: Fp8Weight, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
             act: int = ACT_NONE, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M, N] = epilogue((aq @ w.q^T) * sa[:, None] * w.scale[None, :])  (fo1_gemm_fp8)."""
    M, K = aq.shape
    N = w.q.shape[0]
    if aq.dtype != torch.uint8 or w.q.dtype != torch.uint8 or w.q.shape[1] != K or not aq.is_cuda:
        raise ValueError("gemm_fp8: uint8 device operands with equal K")
    n_out = N // 2 if act == ACT_SWIGLU16 else N
    if out is None:
        out = torch.empty(M, n_out, dtype=torch.bfloat16, device=aq.device)
    po, ldc, Mo, No = _rows(out, "out")
    assert (Mo, No) == (M, n_out)
    pr, ldr = _residual(residual, check=True)
    assert residual is None or tuple(residual.shape) == (M, N)
    if bias is not None:
        _chk(bias, "bias")
        assert bias.numel() == N and bias.is_contiguous()
    rc = _L.load().fo1_gemm_fp8(aq.data_ptr(), aq.stride(0), sa.data_ptr(), w.q.data_ptr(), w.q.stride(0), w.scale.data_ptr(),
                                _ptr(bias), pr, ldr, po, ldc, M, N, K, act, _stream())
    _L.check(rc, "fo1_gemm_fp8")
    return out


def rmsnorm_quant_fp8(x: torch.Tensor, weight: torch.Tensor, eps: float):
    """(q uint8 [M, D], scales fp32 [M]) = quantize_rows_fp8(rmsnorm(x, weight, eps)) in one launch (fo1_rmsnorm_quant_e4m3)."""
    _chk(x, "x"); _chk(weight, "weight")
    px, ldx, M, D = _rows(x, "x")
    q = torch.empty(M, D, dtype=torch.uint8, device=x.device)
    scales = torch.empty(M, dtype=torch.float32, device=x.device)
    _L.check(_L.load().fo1_rmsnorm_quant_e4m3(px, ldx, weight.data_ptr(), M, D, float(eps), q.data_ptr(), q.stride(0), scales.data_ptr(), _stream()),
             "fo1_rmsnorm_quant_e4m3")
    return q, scales


def norm_linear(x: torch.Tensor, norm_w: torch.Tensor, eps: float, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
                act: int = ACT_NONE) -> torch.Tensor:
    """gemm(rmsnorm(x, norm_w, eps), w, bias, act=act): the RMSNorm -> nn.Linear pair of every ViT block / LLM layer
    (modeling_qwen2_5_vl.py:317-331, 1066-1090).  bf16: exactly those two calls.  When `w` is registered for fp8 and the product is
    large enough, the norm emits the e4m3 row + scale directly (no bf16 row, no separate quantiser launch)."""
    if _fp8_weights and x.shape[0] >= FP8_MIN_ROWS:
        pw, ldw, N, K = _rows(w, "w")
        fw = _fp8_weights.get((pw, N, K))
        if fw is not None:
            q, s = rmsnorm_quant_fp8(x, norm_w, eps)
            return gemm_fp8(q, s, fw, bias, None, act)
    return gemm(rmsnorm(x, norm_w, eps), w, bias, act=act)


def fp8_routed(w: torch.Tensor, rows: int) -> bool:
    """True when norm_linear / gemm would send a product of `rows` rows with this weight through the fp8 kernel."""
    if not _fp8_weights or rows < FP8_MIN_ROWS:
        return False
    pw, ldw, N, K = _rows(w, "w")
    return (pw, N, K) in _fp8_weights


def register_fp8_weight(w: torch.Tensor):
    """Quantise a bf16 [N, K] weight and let gemm() route large-M products with it through the fp8 kernel.  The bf16 tensor stays
    (decode and small-M products keep using it).  Returns the routing key (truthy), or None when the shape does not qualify
    (K % 128, N % 4)."""
    _chk(w, "w")
    pw, ldw, N, K = _rows(w, "w")
    if K % 128 or N % 4:
        return None
    q, s = quantize_rows_fp8(w)
    _fp8_weights[(pw, N, K)] = Fp8Weight(q, s, w)
    return (pw, N, K)


def clear_fp8_weights(keys=None) -> None:
    """Drop the given routing keys (an engine's own registrations), or every registration."""
    if keys is None:
        _fp8_weights.clear()
    else:
        for k in keys:
            _fp8_weights.pop(k, None)


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, "x"); _chk(weight, "weight")
    px, ldx, M, D = _rows(x, "x")
    if out is None:
        out = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
    po, ldy, _, _ = _rows(out, "out")
    _L.check(_L.load().fo1_rmsnorm_bf16(px, ldx, weight.data_ptr(), po, ldy, M, D, float(eps), _stream()), "fo1_rmsnorm_bf16")
    return out


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, "x"); _chk(weight, "weight"); _chk(bias, "bias")
    px, ldx, M, D = _rows(x, "x")
    if out is None:
        out = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
    po, ldy, _, _ = _rows(out, "out")
    _L.check(_L.load().fo1_layernorm_bf16(px, ldx, weight.data_ptr(), bias.data_ptr(), po, ldy, M, D, float(eps), _stream()),
             "fo1_layernorm_bf16")
    return out


def layernorm_rows(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, out: torch.Tensor, out_rows: torch.Tensor) -> torch.Tensor:
    """LayerNorm whose output row m goes to row out_rows[m] (int32) of `out` — the padded map of an implicit-GEMM convolution
    (fo1_layernorm_rows_bf16; same arithmetic as layernorm)."""
    _chk(x, "x"); _chk(weight, "weight"); _chk(bias, "bias"); _chk(out, "out")
    px, ldx, M, D = _rows(x, "x")
    po, ldy, _, _ = _rows(out, "out")
    assert out_rows.dtype == torch.int32 and out_rows.is_contiguous() and out_rows.numel() == M and out_rows.device == x.device
    _L.check(_L.load().fo1_layernorm_rows_bf16(px, ldx, weight.data_ptr(), bias.data_ptr(), po, ldy, out_rows.data_ptr(), M, D, float(eps), _stream()),
             "fo1_layernorm_rows_bf16")
    return out


_conv_plan_serial = itertools.count()


class Conv3x3Plan:
    """Index tables of a 3x3 / pad 1 convolution run as an implicit GEMM (fo1_conv3x3_gemm_bf16) over images packed row-wise: the zero-padded
    layout (one pixel per side, common row pitch Wp = widest image + 2), `rowmap` int32 [sum H W] = padded row of every input pixel (where
    layernorm_rows writes it), `a_rows` uint32 [sum Ho Wo] = byte offset of every output pixel's top-left tap.  Host-built once per
    (sizes, stride, channels) and cached (index bookkeeping belongs on the host)."""

    def __init__(self, sizes, stride: int, cin: int, device):
        import numpy as np
        Wp = max(w for _, w in sizes) + 2
        rowmap, a_rows, out_hw = [], [], []
        pb = 0
        for (H, W) in sizes:
            Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
            yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            rowmap.append((pb + (yy + 1) * Wp + (xx + 1)).reshape(-1))
            oy, ox = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
            a_rows.append(((pb + oy * stride * Wp + ox * stride).astype(np.int64) * (cin * 2)).reshape(-1))
            out_hw.append((Ho, Wo))
            pb += (H + 2) * Wp
        ar = np.concatenate(a_rows)
        assert pb * cin * 2 < 2 ** 32, "padded map exceeds the 32-bit byte offsets of the implicit-GEMM convolution"
        self.Wp, self.cin, self.pad_rows, self.out_hw = Wp, cin, pb, out_hw
        self.serial = next(_conv_plan_serial)      # (identifies the padded map's written rows: ops.zero_framed)
        self.uniform = len(set(tuple(t) for t in sizes)) == 1
        self.M_in, self.M_out = sum(h * w for h, w in sizes), int(ar.shape[0])
        self.rowmap = torch.from_numpy(np.concatenate(rowmap).astype(np.int32)).to(device)
        self.a_rows = torch.from_numpy(ar.astype(np.uint32).view(np.int32)).to(device)      # (uint32 bit patterns in an int32 tensor)


def conv3x3_padded(pl: "Conv3x3Plan", device) -> torch.Tensor:
    """The zero-framed map layernorm_rows writes for plan `pl`: persistent for same-size batches (the frame stays zero from pass to pass, the
    interior is rewritten by every pass), a fresh zero fill for ragged packs (their geometry rarely repeats)."""
    if pl.uniform:
        return zero_framed(("conv3x3", pl.serial), pl.pad_rows, pl.cin, device)
    return torch.zeros(pl.pad_rows, pl.cin, dtype=torch.bfloat16, device=device)


_conv_plans: dict = {}
_conv_plans_lock = threading.Lock()      # the cache is shared by every engine replica / worker thread: ragged packs add ~7 plans per pass


def conv3x3_plan(sizes, stride: int, cin: int, device) -> Conv3x3Plan:
    key = (tuple((int(h), int(w)) for h, w in sizes), int(stride), int(cin), str(device))
    with _conv_plans_lock:
        pl = _conv_plans.get(key)
        if pl is None:
            while len(_conv_plans) >= 64:
                _conv_plans.pop(next(iter(_conv_plans)), None)
            pl = _conv_plans[key] = Conv3x3Plan(key[0], stride, cin, device)
    keep_alive(pl)       # a captured pass holds rowmap / a_rows by raw pointer: it keeps the plan past this cache's eviction
    return pl


def conv3x3_implicit_ok(M_out: int, cout: int, cin: int, k: int, pad: int) -> bool:
    """The implicit-GEMM form (no im2col matrix) applies to 3x3 / pad 1 convolutions over >= 64 power-of-two channels whose GEMM runs on the
    256 x 256 kernel anyway (then both forms give the same bits).  FO1_CONV_IMPLICIT=0 turns it off (A/B)."""
    return (os.environ.get("FO1_CONV_IMPLICIT", "1") != "0" and k == 3 and pad == 1 and cin >= 64 and (cin & (cin - 1)) == 0 and cout % 8 == 0
            and bool(_L.load().fo1_gemm_takes_big_tile(int(M_out), int(cout), 9 * int(cin))))


def conv3x3_implicit_for(sizes, stride: int, cout: int, cin: int, k: int, pad: int) -> bool:
    """conv3x3_implicit_ok for images of `sizes` [(H, W)] packed row-wise (uniform or ragged), including the 32-bit byte offsets of the padded
    map (Conv3x3Plan): False sends the caller to im2col + GEMM, the same bits."""
    if k != 3 or pad != 1:
        return False
    Wp = max(int(w) for _, w in sizes) + 2
    if sum(int(h) + 2 for h, _ in sizes) * Wp * int(cin) * 2 >= 2 ** 32:
        return False
    M_out = sum(((int(h) + 2 - 3) // stride + 1) * ((int(w) + 2 - 3) // stride + 1) for h, w in sizes)
    return conv3x3_implicit_ok(M_out, cout, cin, k, pad)


def conv3x3_gemm(xpad: torch.Tensor, plan: Conv3x3Plan, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE) -> torch.Tensor:
    """3x3 convolution of the zero-padded map `xpad` [plan.pad_rows, Cin] (layernorm_rows wrote it) as an implicit GEMM: -> [plan.M_out, Cout]."""
    _chk(xpad, "xpad"); _chk(w, "w")
    assert xpad.is_contiguous() and xpad.shape == (plan.pad_rows, plan.cin)
    pw, ldw, N, K = _rows(w, "w")
    assert K == 9 * plan.cin
    out = torch.empty(plan.M_out, N, dtype=torch.bfloat16, device=xpad.device)
    rc = _L.load().fo1_conv3x3_gemm_bf16(xpad.data_ptr(), plan.a_rows.data_ptr(), plan.Wp, plan.cin, pw, ldw, _ptr(bias),
                                         out.data_ptr(), N, plan.M_out, N, int(act), _stream())
    _L.check(rc, "fo1_conv3x3_gemm_bf16")
    return out


def interleave_gate_up(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """[F, ...] gate and up -> [2F, ...] rows interleaved in 16-row groups [gate 16 | up 16 | ...], the weight/bias
    layout of the fused SwiGLU GEMM epilogue (act = ACT_SWIGLU16).  F must be a multiple of 16."""
    F = gate.shape[0]
    assert up.shape == gate.shape and F % 16 == 0
    g = gate.reshape(F // 16, 16, *gate.shape[1:])
    u = up.reshape(F // 16, 16, *up.shape[1:])
    return torch.stack([g, u], dim=1).reshape(2 * F, *gate.shape[1:]).contiguous()


def swiglu(gate_up: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(gate_up, "gate_up")
    p, ld, M, F2 = _rows(gate_up, "gate_up")
    F = F2 // 2
    if out is None:
        out = torch.empty(M, F, dtype=torch.bfloat16, device=gate_up.device)
    po, ldo, _, _ = _rows(out, "out")
    _L.check(_L.load().fo1_swiglu_bf16(p, ld, po, ldo, M, F, _stream()), "fo1_swiglu_bf16")
    return out


def bias_act(x: torch.Tensor, bias: Optional[torch.Tensor], act: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, "x")
    p, ld, M, D = _rows(x, "x")
    if out is None:
        out = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
    po, ldo, _, _ = _rows(out, "out")
    _L.check(_L.load().fo1_bias_act_bf16(p, ld, _ptr(bias), po, ldo, M, D, act, _stream()),
             "fo1_bias_act_bf16")
    return out


def argmax(row: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(row, "row")
    assert row.is_contiguous()
    if out is None:
        out = torch.empty(1, dtype=torch.int32, device=row.device)
    sc = _workspace("argmax", row.device, 4096)   # per-owner: concurrent requests must not share the two-stage partials
    _L.check(_L.load().fo1_argmax_bf16(row.data_ptr(), row.numel(), out.data_ptr(), sc.data_ptr(), _stream()), "fo1_argmax_bf16")
    return out


def argmax_rows(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [B]: greedy pick of every row of logits [B, V] bf16, first index among ties — the ids argmax() gives row by row, in one launch
    pair (fo1_argmax_rows_bf16)."""
    _chk(logits, "logits")
    pl, ld, B, V = _rows(logits, "logits")
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=logits.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == B
    sc = _workspace("argmax_rows", logits.device, 2 * 128 * B * 4)
    _L.check(_L.load().fo1_argmax_rows_bf16(pl, ld, V, B, out.data_ptr(), sc.data_ptr(), _stream()), "fo1_argmax_rows_bf16")
    return out


def _decode_operands(q: torch.Tensor, kcache: torch.Tensor, vtcache: torch.Tensor, size_fn, *size_args):
    """What the decode attention front ends share: the operand checks and the split-KV partials workspace of size_fn(*size_args) bytes ->
    (workspace, the cache arguments (K, k_tok_stride, k_head_stride, V^T, vt_row_stride) and the tail (workspace, its bytes, stream) of the C entry)."""
    _chk(q, "q"); _chk(kcache, "kcache"); _chk(vtcache, "vtcache")
    assert kcache.dim() == 3
    ws = _workspace("attn_decode", q.device, size_fn(*size_args))
    pv, ldv, _, _ = _rows(vtcache, "vtcache")
    return ws, (kcache.data_ptr(), kcache.stride(1), kcache.stride(0), pv, ldv), (ws.data_ptr(), ws.numel(), _stream())


def attention_decode(q: torch.Tensor, kcache: torch.Tensor, vtcache: torch.Tensor, kv_len_dev: torch.Tensor, max_kv_len: int,
                     n_q_heads: int, n_kv_heads: int, head_dim: int, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One new token (q [1, n_q_heads*head_dim]) against the cache; kv_len_dev = device int32 scalar holding the
    number of keys to attend (cache position + 1)."""
    assert kv_len_dev.dtype == torch.int32 and q.shape[0] == 1
    lib = _L.load()
    _, cache, tail = _decode_operands(q, kcache, vtcache, lib.fo1_attention_decode_workspace_bytes, max_kv_len, n_kv_heads, head_dim)
    if out is None:
        out = torch.empty(1, n_q_heads * head_dim, dtype=torch.bfloat16, device=q.device)
    rc = lib.fo1_attention_decode_bf16(q.data_ptr(), *cache, out.data_ptr(), kv_len_dev.data_ptr(), max_kv_len, n_q_heads, n_kv_heads, head_dim,
                                       float(scale), *tail)
    _L.check(rc, "fo1_attention_decode_bf16")
    return out


def rope_llm(qkv: torch.Tensor, n_heads: int, head_dim: int, cos: torch.Tensor, sin: torch.Tensor,
             kcache: Optional[torch.Tensor] = None, k_first_head: int = 0, pos0: int = 0, col0: int = 0,
             dyn_state: Optional[torch.Tensor] = None) -> None:
    """In place on heads [0,n_heads) (q heads then k heads) of qkv [L, ld]; cos/sin bf16 [L, head_dim] — or, with
    dyn_state (device int32: [cache position, table row]), full per-position tables indexed on the device."""
    _chk(qkv, "qkv"); _chk(cos, "cos"); _chk(sin, "sin")
    p, ld, L, _ = _rows(qkv, "qkv")
    assert cos.shape[1] == head_dim and cos.is_contiguous() and sin.is_contiguous()
    assert dyn_state is not None or cos.shape[0] == L
    kc_ptr, kc_stride = None, 0
    if kcache is not None:
        _chk(kcache, "kcache")
        assert kcache.dim() == 3 and kcache.shape[2] == head_dim and kcache.stride(2) == 1 and kcache.stride(1) == head_dim
        kc_ptr, kc_stride = kcache.data_ptr(), kcache.stride(0)
    _L.check(_L.load().fo1_rope_llm_bf16(p, ld, col0, n_heads, head_dim, cos.data_ptr(), sin.data_ptr(), L, kc_ptr,
                                         k_first_head, kc_stride, pos0, _ptr(dyn_state),
                                         _stream()), "fo1_rope_llm_bf16")


def rope_vit(qkv: torch.Tensor, n_heads: int, head_dim: int, cos: torch.Tensor, sin: torch.Tensor) -> None:
    _chk(qkv, "qkv"); _chk(cos, "cos", torch.float32); _chk(sin, "sin", torch.float32)
    p, ld, S, _ = _rows(qkv, "qkv")
    assert cos.shape == (S, head_dim // 2) and cos.is_contiguous() and sin.is_contiguous()
    _L.check(_L.load().fo1_rope_vit_bf16(p, ld, n_heads, head_dim, cos.data_ptr(), sin.data_ptr(), S, _stream()),
             "fo1_rope_vit_bf16")


def qkv_post_llm(qkv: torch.Tensor, n_q: int, n_kv: int, head_dim: int, cos: torch.Tensor, sin: torch.Tensor,
                 kcache: torch.Tensor, vtcache: torch.Tensor, pos0: int = 0) -> None:
    """Prefill, one launch: mRoPE on the q/k heads of qkv [L, (n_q+2 n_kv) hd] in place, K heads appended to
    kcache [n_kv, max_seq, hd] at pos0, V heads copied transposed into vtcache [n_kv*hd, max_seq] at column pos0."""
    _chk(qkv, "qkv"); _chk(cos, "cos"); _chk(sin, "sin"); _chk(kcache, "kcache"); _chk(vtcache, "vtcache")
    p, ld, L, _ = _rows(qkv, "qkv")
    assert cos.shape == (L, head_dim) and cos.is_contiguous() and sin.is_contiguous()
    assert kcache.dim() == 3 and kcache.shape[2] == head_dim and kcache.stride(2) == 1 and kcache.stride(1) == head_dim
    pv, ldv, Cv, _ = _rows(vtcache, "vtcache")
    assert Cv == n_kv * head_dim
    _L.check(_L.load().fo1_qkv_post_llm_bf16(p, ld, n_q, n_kv, head_dim, cos.data_ptr(), sin.data_ptr(), L, kcache.data_ptr(),
                                             kcache.stride(0), pv, ldv, pos0, _stream()), "fo1_qkv_post_llm_bf16")


def qkv_post_vit(qkv: torch.Tensor, n_heads: int, head_dim: int, cos: torch.Tensor, sin: torch.Tensor, vt: torch.Tensor) -> None:
    """ViT block, one launch: 2-D RoPE on the q/k heads of qkv [S, 3 d] in place + V -> vt [d, >= S]."""
    _chk(qkv, "qkv"); _chk(cos, "cos", torch.float32); _chk(sin, "sin", torch.float32); _chk(vt, "vt")
    p, ld, S, _ = _rows(qkv, "qkv")
    assert cos.shape == (S, head_dim // 2) and cos.is_contiguous() and sin.is_contiguous()
    pv, ldv, Cv, _ = _rows(vt, "vt")
    assert Cv == n_heads * head_dim
    _L.check(_L.load().fo1_qkv_post_vit_bf16(p, ld, n_heads, head_dim, cos.data_ptr(), sin.data_ptr(), S, pv, ldv, _stream()),
             "fo1_qkv_post_vit_bf16")


def qkv_fused_enabled() -> bool:
    """FO1_QKV_FUSED=0 turns the fused q/k/v epilogue off (A/B; both forms give the same bits)."""
    return os.environ.get("FO1_QKV_FUSED", "1") != "0"


def qkv_fused_for(M: int, N: int, K: int) -> bool:
    """Take the fused q/k/v form (qkv_proj_rope: always the 256 x 256 GEMM kernel) for a product that gemm() itself would run on that kernel
    — and only there: a row's fp32 sum order is the kernel's, so the fused and the two-launch form then agree bit for bit (also under the
    test build's tile pins, which fo1_gemm_takes_big_tile honours)."""
    return qkv_fused_enabled() and bool(_L.load().fo1_gemm_takes_big_tile(int(M), int(N), int(K)))


def qkv_proj_rope(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], mode: int, n_q: int, n_kv: int, cos: torch.Tensor, sin: torch.Tensor,
                  kcache: Optional[torch.Tensor], pos0: int, vt: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q/k/v projection + bias + RoPE + K-cache append + V^T write in one launch (fo1_qkv_proj_rope_bf16: the 256 x 256 GEMM with the fused
    epilogue).  mode 0 (LLM): w [(n_q + 2 n_kv) * 128, K], cos / sin bf16 [M, 128], kcache [n_kv, max_seq, 128]; returns [M, N] whose first
    n_q * 128 columns hold the rotated q heads (the k / v columns are not written).  mode 1 (ViT): w head-major [n_q * 256, K] (head_major_qkv),
    cos / sin fp32 [M, 40]; returns [M, n_q * 256] = per head [q 80 | k 80 | - | -] rotated.  vt: the V^T destination [heads * head_dim, ld]."""
    _chk(x, "x"); _chk(w, "w"); _chk(vt, "vt")
    px, ldx, M, K = _rows(x, "x")
    pw, ldw, N, Kw = _rows(w, "w")
    assert K == Kw
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    po, ldo, _, _ = _rows(out, "out")
    pv, ldv, _, _ = _rows(vt, "vt")
    if mode == 0:
        _chk(cos, "cos"); _chk(sin, "sin"); _chk(kcache, "kcache")
        assert cos.shape == (M, 128) and cos.is_contiguous() and sin.shape == (M, 128) and sin.is_contiguous()
        assert kcache.dim() == 3 and kcache.shape[2] == 128 and kcache.stride(2) == 1 and kcache.stride(1) == 128
        pk, ks = kcache.data_ptr(), kcache.stride(0)
    else:
        _chk(cos, "cos", torch.float32); _chk(sin, "sin", torch.float32)
        assert cos.shape == (M, 40) and cos.is_contiguous() and sin.shape == (M, 40) and sin.is_contiguous()
        pk, ks = None, 0
    rc = _L.load().fo1_qkv_proj_rope_bf16(px, ldx, pw, ldw, _ptr(bias), po, ldo, M, N, K, int(mode), int(n_q), int(n_kv),
                                          cos.data_ptr(), sin.data_ptr(), pk, ks, int(pos0), pv, ldv, _stream())
    _L.check(rc, "fo1_qkv_proj_rope_bf16")
    return out


def head_major_qkv(w: torch.Tensor, n_heads: int, head_dim: int = 80, tile: int = 256) -> torch.Tensor:
    """[3 * n_heads * head_dim, ...] rows ordered [q heads | k heads | v heads] -> [n_heads * tile, ...] rows ordered per head
    [q | k | v | zero pad] (qkv_proj_rope mode 1: one 256-column output tile per head).  Works for the weight [3 d, K] and the bias [3 d]."""
    d = n_heads * head_dim
    assert w.shape[0] == 3 * d and 3 * head_dim <= tile
    parts = w.reshape(3, n_heads, head_dim, *w.shape[1:]).transpose(0, 1)                     # [head, 3, head_dim, ...]
    out = torch.zeros(n_heads, tile, *w.shape[1:], dtype=w.dtype, device=w.device)
    out[:, :3 * head_dim] = parts.reshape(n_heads, 3 * head_dim, *w.shape[1:])
    return out.reshape(n_heads * tile, *w.shape[1:]).contiguous()


def transpose_into(src: torch.Tensor, dst: torch.Tensor, col0: int = 0, dyn_col0: Optional[torch.Tensor] = None) -> None:
    """dst[c, col0 + m] = src[m, c];  src [M, C] (C % 64 == 0), dst [C, >= col0 + M]; col0 read from the device int
    `dyn_col0` when given."""
    _chk(src, "src"); _chk(dst, "dst")
    p, ld, M, C = _rows(src, "src")
    pd, ldd, Cd, _ = _rows(dst, "dst")
    assert Cd == C
    _L.check(_L.load().fo1_transpose_bf16(p, ld, pd, ldd, col0, _ptr(dyn_col0), M, C,
                                          _stream()), "fo1_transpose_bf16")


def _gemv_operands(x: Optional[torch.Tensor], w: torch.Tensor, residual: Optional[torch.Tensor], out: Optional[torch.Tensor], M: int, n_out,
                   max_m: int):
    """What the decode-step linears share: x [M, K] (None: the rows come from elsewhere, M is given) and w [N, K] checked, `out` [M, n_out(N)]
    allocated unless given -> ((px, ldx), (pw, ldw), (pr, ldr), (po, ldc), (M, N, K), out)."""
    _chk(w, "w")
    pw, ldw, N, K = _rows(w, "w")
    px, ldx = None, 0
    if x is not None:
        _chk(x, "x")
        px, ldx, M, Kx = _rows(x, "x")
        assert K == Kx
    assert M <= max_m
    if out is None:
        out = torch.empty(M, n_out(N), dtype=torch.bfloat16, device=w.device)
    po, ldc, _, _ = _rows(out, "out")
    return (px, ldx), (pw, ldw), _residual(residual), (po, ldc), (M, N, K), out


def gemv(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         act: int = ACT_NONE, norm_weight: Optional[torch.Tensor] = None, norm_eps: float = 0.0,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode-step projection: out[M<=4, N] = epilogue(rmsnorm?(x) @ w^T) (fo1_gemv_bf16)."""
    xs, ws, rs, os_, shape, out = _gemv_operands(x, w, residual, out, 0, lambda N: N // 2 if act == ACT_SWIGLU16 else N, 4)
    rc = _L.load().fo1_gemv_bf16(*xs, *ws, _ptr(bias), *rs, *os_, *shape, act, _ptr(norm_weight), float(norm_eps), _stream())
    _L.check(rc, "fo1_gemv_bf16")
    return out


# ---- batched decode (decode.hip) ------------------------------------------------------------------------------------------
GB_PLAIN, GB_SWIGLU, GB_QKV = 0, 1, 2


def gemv_batch(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
               mode: int = GB_PLAIN, norm_weight: Optional[torch.Tensor] = None, norm_eps: float = 0.0,
               out: Optional[torch.Tensor] = None, qkv: Optional[dict] = None) -> torch.Tensor:
    """Decode-step projection for M <= 32 sequences (fo1_gemv_batch_bf16).  qkv (mode GB_QKV): dict(n_q, n_kv, cos, sin, state,
    kcache [n_kv, rows, 128], vtcache [n_kv*128, rows]) — `out` then receives only the rotated q rows [M, n_q*128]."""
    xs, ws, rs, os_, shape, out = _gemv_operands(x, w, residual, out, 0, lambda N: N // 2 if mode == GB_SWIGLU else (qkv["n_q"] * 128 if mode == GB_QKV else N), 32)
    if mode == GB_QKV:
        kc, vt = qkv["kcache"], qkv["vtcache"]
        _chk(kc, "kcache"); _chk(vt, "vtcache")
        assert kc.dim() == 3 and kc.stride(2) == 1 and kc.stride(1) == 128 and qkv["state"].dtype == torch.int32
        pv, ldv, _, _ = _rows(vt, "vtcache")
        extra = (qkv["n_q"], qkv["n_kv"], qkv["cos"].data_ptr(), qkv["sin"].data_ptr(), qkv["state"].data_ptr(), kc.data_ptr(), kc.stride(0), pv, ldv)
    else:
        extra = (0, 0, None, None, None, None, 0, None, 0)
    rc = _L.load().fo1_gemv_batch_bf16(*xs, *ws, _ptr(bias), *rs, *os_, *shape, mode, _ptr(norm_weight), float(norm_eps), *extra, _stream())
    _L.check(rc, "fo1_gemv_batch_bf16")
    return out


def attention_decode_batch(q: torch.Tensor, kcache: torch.Tensor, vtcache: torch.Tensor, state: torch.Tensor, max_kv_len: int,
                           n_q_heads: int, n_kv_heads: int, head_dim: int, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [B, n_q_heads*head_dim] (one new token per sequence) against the slots described by state int32 [B, 8]."""
    assert state.dtype == torch.int32 and state.is_contiguous()
    pq, ldq, B, _ = _rows(q, "q")
    lib = _L.load()
    _, cache, tail = _decode_operands(q, kcache, vtcache, lib.fo1_attention_decode_batch_workspace_bytes, max_kv_len, n_kv_heads, head_dim, B)
    if out is None:
        out = torch.empty(B, n_q_heads * head_dim, dtype=torch.bfloat16, device=q.device)
    po, ldo, _, _ = _rows(out, "out")
    rc = lib.fo1_attention_decode_batch_bf16(pq, ldq, *cache, po, ldo, state.data_ptr(), B, max_kv_len, n_q_heads, n_kv_heads, head_dim, float(scale), *tail)
    _L.check(rc, "fo1_attention_decode_batch_bf16")
    return out


def attention_decode_batch_partials(q: torch.Tensor, kcache: torch.Tensor, vtcache: torch.Tensor, state: torch.Tensor, max_kv_len: int,
                                    n_q_heads: int, n_kv_heads: int, head_dim: int, scale: float):
    """The split-KV half of attention_decode_batch alone -> (partials workspace, floats per sequence, keys per chunk) for gemv_attn_combine."""
    assert state.dtype == torch.int32 and state.is_contiguous()
    pq, ldq, B, _ = _rows(q, "q")
    lib = _L.load()
    ws, cache, (pws, ws_bytes, stream) = _decode_operands(q, kcache, vtcache, lib.fo1_attention_decode_batch_workspace_bytes, max_kv_len, n_kv_heads, head_dim, B)
    chunk, stride = ctypes.c_int(0), ctypes.c_longlong(0)
    rc = lib.fo1_attention_decode_batch_partials_bf16(pq, ldq, *cache, state.data_ptr(), B, max_kv_len, n_q_heads, n_kv_heads, head_dim, float(scale),
                                                      pws, ws_bytes, ctypes.byref(chunk), ctypes.byref(stride), stream)
    _L.check(rc, "fo1_attention_decode_batch_partials_bf16")
    return ws, stride.value, chunk.value


def gemv_attn_combine(part: torch.Tensor, part_seq_stride: int, state: torch.Tensor, kv_chunk: int, n_q_heads: int, n_kv_heads: int, w: torch.Tensor,
                      residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """o-projection of a decode step at <= 2 sequences, the attention combine in its prologue (fo1_gemv_attn_combine_bf16)."""
    _, ws, rs, os_, (M, N, K), out = _gemv_operands(None, w, residual, out, state.shape[0], lambda N: N, 2)
    assert K == n_q_heads * 128 and state.dtype == torch.int32 and state.is_contiguous()
    rc = _L.load().fo1_gemv_attn_combine_bf16(part.data_ptr(), int(part_seq_stride), state.data_ptr(), int(kv_chunk), n_q_heads, n_kv_heads, *ws, *rs,
                                              *os_, M, N, _stream())
    _L.check(rc, "fo1_gemv_attn_combine_bf16")
    return out


# ---- decode pool: 64 / 128 sequence slots per weight stream (llm.DecodePool) ---------------------------------------------------------
def pool_qkv_post(qkv: torch.Tensor, n_q: int, n_kv: int, head_dim: int, cos_table: torch.Tensor, sin_table: torch.Tensor, state: torch.Tensor,
                  kcache: torch.Tensor, vtcache: torch.Tensor) -> None:
    """mRoPE + cache append for the P rows of a pool step's fused q/k/v product (in place; fo1_pool_qkv_post_bf16)."""
    _chk(qkv, "qkv"); _chk(kcache, "kcache"); _chk(vtcache, "vtcache")
    p, ld, P, _ = _rows(qkv, "qkv")
    assert kcache.dim() == 3 and state.dtype == torch.int32 and state.is_contiguous() and state.shape[0] >= P
    pv, ldv, _, _ = _rows(vtcache, "vtcache")
    rc = _L.load().fo1_pool_qkv_post_bf16(p, ld, P, n_q, n_kv, head_dim, cos_table.data_ptr(), sin_table.data_ptr(), state.data_ptr(), kcache.data_ptr(),
                                          kcache.stride(0), pv, ldv, _stream())
    _L.check(rc, "fo1_pool_qkv_post_bf16")


def _need_ab(what: str) -> None:
    """Entry points of include/fo1_ab.h (measured no-gain kernel forms, instruments) exist in the test / bench build only."""
    if not _L.ab_build():
        raise _L.Fo1Error(f"{what} is part of include/fo1_ab.h: call it inside `with vlm_fo1_amd.lib.use_ab():` (or start the process with FO1_AB=1)")


def mfma_clock_probe(operands: int = 1, iters: int = 2000, workgroups: int = 256) -> dict:
    """Sustained clock / rate of a register-resident dense bf16 MFMA loop on this box (fo1_mfma_clock_probe, csrc/probe.hip):
    {clock_ghz (median over workgroups), tflops, us}.  operands 1 = pseudo-random bf16, 0 = zeros."""
    _need_ab("fo1_mfma_clock_probe")
    out = torch.zeros(workgroups, 2, dtype=torch.int64, device="cuda")
    sink = torch.zeros(1, dtype=torch.float32, device="cuda")
    for _ in range(2):          # the second launch is the measurement (the first ramps the clocks)
        _L.check(_L.load().fo1_mfma_clock_probe(int(operands), int(iters), int(workgroups), out.data_ptr(), sink.data_ptr(), _stream()), "fo1_mfma_clock_probe")
    torch.cuda.current_stream().synchronize()
    o = out.cpu().double()
    ghz = (o[:, 0] / (o[:, 1] * 10.0)).median().item()
    us = (o[:, 1] / 100.0).median().item()
    return dict(clock_ghz=round(ghz, 3), us=round(us, 1), tflops=round(workgroups * 8.0 * iters * 32.0 * 32768.0 / (us * 1e-6) / 1e12, 1))


def gemm_partials(a: torch.Tensor, w: torch.Tensor, splits: int, part: torch.Tensor) -> int:
    """Split-K planes of a @ w.T into part (fp32, >= splits * M * N elements): -> the effective number of planes [z, M, N] written
    (fo1_gemm_bf16_partials; no epilogue, no reduce — consumers: splitk_residual_rmsnorm, pool_qkv_post_partials)."""
    _chk(a, "a"); _chk(w, "w")
    pa, lda, M, K = _rows(a, "a")
    pw, ldw, N, Kw = _rows(w, "w")
    assert K == Kw and part.dtype == torch.float32 and part.is_contiguous() and part.numel() >= splits * M * N
    eff = ctypes.c_int(0)
    rc = _L.load().fo1_gemm_bf16_partials(pa, lda, pw, ldw, M, N, K, int(splits), part.data_ptr(), ctypes.byref(eff), _stream())
    _L.check(rc, "fo1_gemm_bf16_partials")
    return eff.value


def splitk_residual_rmsnorm(part: torch.Tensor, splits: int, residual: torch.Tensor, norm_weight: torch.Tensor, eps: float, x_out: torch.Tensor,
                            xn_out: torch.Tensor, bias: Optional[torch.Tensor] = None) -> None:
    """x_out = bf16(bf16(sum_z part[z] (+ bias)) + residual); xn_out = RMSNorm(x_out) * norm_weight — one launch (fo1_splitk_residual_rmsnorm_bf16).
    x_out may alias residual (each element is read and written by the same thread)."""
    _chk(residual, "residual"); _chk(x_out, "x_out"); _chk(xn_out, "xn_out")
    pr, ldr, M, N = _rows(residual, "residual")
    px, ldx, _, _ = _rows(x_out, "x_out")
    pn, ldn, _, _ = _rows(xn_out, "xn_out")
    assert part.dtype == torch.float32 and part.numel() >= splits * M * N and norm_weight.numel() == N
    rc = _L.load().fo1_splitk_residual_rmsnorm_bf16(part.data_ptr(), int(splits), M, N, _ptr(bias), pr, ldr, px, ldx,
                                                    norm_weight.data_ptr(), float(eps), pn, ldn, _stream())
    _L.check(rc, "fo1_splitk_residual_rmsnorm_bf16")


def tile_weight(w: torch.Tensor) -> torch.Tensor:
    """The [N / 128][K / 64][128][64] copy of a row-major weight [N, K] that fo1_gemm_bf16_wtiled streams (N % 128 == 0, K % 64 == 0)."""
    N, K = w.shape
    assert N % 128 == 0 and K % 64 == 0 and w.dtype == torch.bfloat16
    return w.view(N // 128, 128, K // 64, 64).permute(0, 2, 1, 3).contiguous()


def gemm_wtiled(a: torch.Tensor, w_tiled: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a @ W.T (+ epilogue) with W given as ops.tile_weight(W): the weight-streaming form for <= 128 rows (fo1_gemm_bf16_wtiled).  out: a
    row-major [M, N (N / 2 with SwiGLU)] bf16 view to write into (its row stride may be padded)."""
    _need_ab("fo1_gemm_bf16_wtiled")
    _chk(a, "a"); _chk(w_tiled, "w_tiled")
    pa, lda, M, K = _rows(a, "a")
    assert w_tiled.dim() == 4 and w_tiled.shape[2:] == (128, 64) and w_tiled.is_contiguous() and w_tiled.shape[1] * 64 == K
    N = w_tiled.shape[0] * 128
    out = _out_rows(out, M, N // 2 if act == ACT_SWIGLU16 else N, a.device)
    po, ldc, _, _ = _rows(out, "out")
    pr, ldr = _residual(residual, check=True)
    rc = _L.load().fo1_gemm_bf16_wtiled(pa, lda, w_tiled.data_ptr(), _ptr(bias), pr, ldr, po, ldc, M, N, K, int(act), _stream())
    _L.check(rc, "fo1_gemm_bf16_wtiled")
    return out


def splitk_swiglu(part: torch.Tensor, splits: int, M: int, N: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [M, N / 2] = SwiGLU over the split-K planes of a product against a 16-row interleaved gate/up weight (fo1_splitk_swiglu_bf16)."""
    _need_ab("fo1_splitk_swiglu_bf16")
    assert part.dtype == torch.float32 and part.numel() >= splits * M * N and part.is_cuda
    if out is None:
        out = torch.empty(M, N // 2, dtype=torch.bfloat16, device=part.device)
    po, ldo, _, _ = _rows(out, "out")
    _L.check(_L.load().fo1_splitk_swiglu_bf16(part.data_ptr(), int(splits), M, N, po, ldo, _stream()), "fo1_splitk_swiglu_bf16")
    return out


def pool_qkv_post_partials(part: torch.Tensor, splits: int, bias: Optional[torch.Tensor], q_out: torch.Tensor, n_q: int, n_kv: int, head_dim: int,
                           cos_table: torch.Tensor, sin_table: torch.Tensor, state: torch.Tensor, kcache: torch.Tensor, vtcache: torch.Tensor) -> None:
    """pool_qkv_post fed by the split-K planes of the q/k/v projection: rotated q rows -> q_out [P, >= n_q * head_dim], K / V^T -> caches."""
    _chk(q_out, "q_out"); _chk(kcache, "kcache"); _chk(vtcache, "vtcache")
    p, ld, P, _ = _rows(q_out, "q_out")
    assert kcache.dim() == 3 and state.dtype == torch.int32 and state.is_contiguous() and state.shape[0] >= P
    assert part.dtype == torch.float32 and part.numel() >= splits * P * (n_q + 2 * n_kv) * head_dim
    pv, ldv, _, _ = _rows(vtcache, "vtcache")
    rc = _L.load().fo1_pool_qkv_post_partials_bf16(part.data_ptr(), int(splits), _ptr(bias), p, ld, P, n_q, n_kv, head_dim,
                                                   cos_table.data_ptr(), sin_table.data_ptr(), state.data_ptr(), kcache.data_ptr(), kcache.stride(0), pv, ldv,
                                                   _stream())
    _L.check(rc, "fo1_pool_qkv_post_partials_bf16")


def decode_argmax_accept(logits: Optional[torch.Tensor], first_tokens: Optional[torch.Tensor], state: torch.Tensor, plan: torch.Tensor,
                         ids_out: torch.Tensor, stop_ids: torch.Tensor, done: torch.Tensor, per_sequence_sets: bool = False) -> None:
    """per_sequence_sets: stop_ids is a table int32 [sets, 17] = {count, ids[16]} and state[b, 6] names sequence b's row (decode pool)."""
    B = state.shape[0]
    assert state.dtype == plan.dtype == ids_out.dtype == done.dtype == torch.int32 and ids_out.is_contiguous() and plan.is_contiguous()
    sc = _workspace("argmax_rows", state.device, 2 * 128 * B * 4)
    n_stop = int(stop_ids.numel()) if stop_ids is not None else 0
    if per_sequence_sets:
        assert stop_ids is not None and stop_ids.dim() == 2 and stop_ids.shape[1] == 17 and stop_ids.is_contiguous() and stop_ids.dtype == torch.int32
        n_stop = -1
    if logits is not None:
        _chk(logits, "logits")
        pl, ldl, Bl, V = _rows(logits, "logits")
        assert Bl == B
    else:
        pl, ldl, V = None, 0, 0
        assert first_tokens is not None and first_tokens.dtype == torch.int32 and first_tokens.numel() == B
    rc = _L.load().fo1_decode_argmax_accept(pl, ldl, V, B, _ptr(first_tokens), state.data_ptr(),
                                            plan.data_ptr(), ids_out.data_ptr(), ids_out.shape[1], stop_ids.data_ptr() if n_stop else None, n_stop,
                                            done.data_ptr(), sc.data_ptr(), _stream())
    _L.check(rc, "fo1_decode_argmax_accept")


SAMPLE_GREEDY = 1      # fo1_sample_params_t.flags bit 0 (FO1_SAMPLE_GREEDY)


def sample_params(rows: Sequence[Sequence], device=None) -> torch.Tensor:
    """The fo1_sample_params_t table (int32 [B, 8] = 32 bytes per sequence) from rows of (temperature, top_p, top_k, seed, stream) or
    (temperature, top_p, top_k, seed, stream, greedy, repetition_penalty): seed is an integer of up to 64 bits (the Philox key), stream the
    sequence's index in its request list; greedy sets flags bit 0 and repetition_penalty (None = 0 = off) fills the last word, both read by the
    general head only (sample_rows(seen=...), decode_head_accept).  On `device` when given, else a host tensor."""
    import struct

    def pack(r):
        t, p, k, seed, stream = r[:5]
        if len(r) == 5:
            flags, rp = 0, 0.0
        elif len(r) == 7:
            flags, rp = (SAMPLE_GREEDY if r[5] else 0), float(r[6] or 0.0)
        else:
            raise ValueError("sample_params: a row has 5 fields, or 7 (..., greedy, repetition_penalty)")
        return struct.pack("<ffiIIIIf", float(t), float(p), int(k), int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff,
                           int(stream) & 0xffffffff, flags, rp)
    tab = torch.frombuffer(bytearray(b"".join(pack(r) for r in rows)), dtype=torch.int32).view(-1, 8)
    return tab if device is None else tab.to(device)


def sampling_row(s: Optional[dict], stream: int = 0):
    """One sequence's sampling dict (temperature, top_p, top_k, seed, stream — optional when greedy — plus greedy, repetition_penalty) -> the
    7-field row of sample_params; None = the plain greedy row.  `stream` is the default for a dict without one."""
    if s is None:
        return (0.0, 1.0, 0, 0, 0, True, 0.0)
    greedy = bool(s.get("greedy", False))
    if not greedy and "temperature" not in s:
        raise ValueError("a sampled sequence needs a temperature (or greedy=True)")
    return (s.get("temperature", 0.0), s.get("top_p", 1.0), s.get("top_k", 0), s.get("seed", 0), s.get("stream", stream), greedy,
            s.get("repetition_penalty") or 0.0)


def penalty_on(p) -> bool:
    """The device's rule: a repetition penalty is on iff it is finite, > 0 and != 1."""
    import math
    return p is not None and math.isfinite(float(p)) and float(p) > 0 and float(p) != 1.0


def seen_words(n_vocab: int) -> int:
    """Words per row of a seen bitmap: ceil(V / 32) rounded up to a multiple of 4."""
    return -(-(-(-int(n_vocab) // 32)) // 4) * 4


def seen_mark(seen: torch.Tensor, n_vocab: int, rows: torch.Tensor, ids: torch.Tensor) -> None:
    """Sets bit ids[i] of row rows[i] of the seen bitmap (int32 [R, ld_words], fo1_seen_mark); ids outside [0, n_vocab) are skipped."""
    assert seen.dtype == torch.int32 and seen.is_cuda and seen.dim() == 2 and seen.is_contiguous()
    assert rows.dtype == ids.dtype == torch.int32 and rows.is_cuda and ids.is_cuda and rows.is_contiguous() and ids.is_contiguous() and rows.numel() == ids.numel()
    rc = _L.load().fo1_seen_mark(seen.data_ptr(), seen.shape[1], int(n_vocab), _ptr(rows), _ptr(ids), rows.numel(), _stream())
    _L.check(rc, "fo1_seen_mark")


def mark_prompts(seen: torch.Tensor, n_vocab: int, rows: Sequence[int], prompts: Sequence[Sequence[int]]) -> list:
    """Clears the bitmap rows `rows` and marks row rows[k] with the ids of prompts[k] (ids outside [0, n_vocab) are skipped on the device) ->
    the host tensors of the asynchronous uploads, for the caller to keep alive."""
    r = torch.tensor([row for row, pr in zip(rows, prompts) for _ in pr], dtype=torch.int32)
    t = torch.tensor([int(x) for pr in prompts for x in pr], dtype=torch.int64).clamp_(-1, int(n_vocab)).to(torch.int32)
    for row in rows:
        seen[row].zero_()
    if r.numel():
        seen_mark(seen, n_vocab, r.to(seen.device, non_blocking=True), t.to(seen.device, non_blocking=True))
    return [r, t]


def _seen_operand(seen: Optional[torch.Tensor], B: int, V: int):
    if seen is None:
        return None, 0
    assert seen.dtype == torch.int32 and seen.is_cuda and seen.dim() == 2 and seen.is_contiguous() and seen.shape[0] >= B
    return seen.data_ptr(), seen.shape[1]


NO_RULE = (-1, -1, 0, -1)      # fo1_token_rule_t of a row without a rule


def token_rules(rows: Sequence, device=None) -> torch.Tensor:
    """The fo1_token_rule_t table (int32 [B, 4]) from rows of (always_row, early_row, early_until, first_row) — indices into a mask table, -1
    = none (include/fo1.h) — or None for a row without a rule.  On `device` when given, else a host tensor."""
    tab = torch.tensor([list(NO_RULE) if r is None else [int(x) for x in r] for r in rows], dtype=torch.int32).view(-1, 4)
    return tab if device is None else tab.to(device)


def _rule_operands(masks: Optional[torch.Tensor], rules: Optional[torch.Tensor], B: int, V: int):
    assert masks is not None and rules is not None, "a ruled head takes the mask table and the rule table together"
    assert masks.dtype == torch.int32 and masks.is_cuda and masks.dim() == 2 and masks.is_contiguous() and masks.shape[0] >= 1
    assert masks.shape[1] % 4 == 0 and masks.shape[1] * 32 >= V
    assert rules.dtype == torch.int32 and rules.is_cuda and rules.dim() == 2 and rules.shape[1] == 4 and rules.is_contiguous() and rules.shape[0] >= B
    return masks.data_ptr(), masks.shape[0], masks.shape[1], rules.data_ptr()


NO_GUIDE = (-1, 0, 0, 0)       # fo1_token_guide_t of a row without a guide


def token_guides(rows: Sequence, device=None) -> torch.Tensor:
    """The fo1_token_guide_t table (int32 [B, 4]) from rows of (cls_row, n_classes, next_off, row_off) — a row of the class table, the number of
    classes, the guide's offsets into the `next` and `state_row` tables (include/fo1.h) — or None for a row without a guide.  On `device` when
    given, else a host tensor."""
    tab = torch.tensor([list(NO_GUIDE) if r is None else [int(x) for x in r] for r in rows], dtype=torch.int32).view(-1, 4)
    return tab if device is None else tab.to(device)


NO_CLOSE = (0, 0, 0, 0)        # fo1_guide_close_t of a row without a closing rule (depth 0)


def guide_closes(rows: Sequence, device=None) -> torch.Tensor:
    """The fo1_guide_close_t table (int32 [B, 4]) from rows of (close_off, depth) — the guide's offset into the `close_row` table and its depth D
    (include/fo1.h) — or None for a row without a closing rule.  On `device` when given, else a host tensor."""
    tab = torch.tensor([list(NO_CLOSE) if r is None else [int(r[0]), int(r[1]), 0, 0] for r in rows], dtype=torch.int32).view(-1, 4)
    return tab if device is None else tab.to(device)


class GuideOperands(NamedTuple):
    """What a guided head takes besides masks and rules (include/fo1.h): cls int16 [rows, ld_cls >= V] holding the uint16 token classes, next
    int32 [n_next], state_row int32 [n_state_row] (mask-table row of every state, -1 = nothing banned), guides (token_guides, int32 [>= B, 4])
    and gstate int32 [>= B], the rows' automaton states — the one table the head writes.
    closes (guide_closes, int32 [>= B, 4]) with close_row int32 [n_close_row] (mask-table row of every (state, tokens left)): the closing
    head (fo1_sample_rows_closing_bf16 / fo1_decode_head_closing_accept); budget int32 [>= B]: the rows' token budgets, which the rows form
    needs (the accept form reads them from the decode state)."""
    cls: torch.Tensor
    next: torch.Tensor
    state_row: torch.Tensor
    guides: torch.Tensor
    gstate: torch.Tensor
    close_row: Optional[torch.Tensor] = None
    closes: Optional[torch.Tensor] = None
    budget: Optional[torch.Tensor] = None


def _guide_operands(g: GuideOperands, B: int, V: int):
    assert g.cls.dtype == torch.int16 and g.cls.is_cuda and g.cls.dim() == 2 and g.cls.is_contiguous() and g.cls.shape[0] >= 1 and g.cls.shape[1] >= V
    for t in (g.next, g.state_row, g.gstate):
        assert t.dtype == torch.int32 and t.is_cuda and t.dim() == 1 and t.is_contiguous() and t.numel() >= 1
    assert g.guides.dtype == torch.int32 and g.guides.is_cuda and g.guides.dim() == 2 and g.guides.shape[1] == 4 and g.guides.is_contiguous()
    assert g.guides.shape[0] >= B and g.gstate.numel() >= B
    return (g.cls.data_ptr(), g.cls.shape[0], g.cls.shape[1], g.next.data_ptr(), g.next.numel(), g.state_row.data_ptr(), g.state_row.numel(),
            g.guides.data_ptr(), g.gstate.data_ptr())


def _close_operands(g: GuideOperands, B: int, rows_form: bool):
    assert g.close_row is not None, "a closing head takes close_row and closes together"
    t = g.close_row
    assert t.dtype == torch.int32 and t.is_cuda and t.dim() == 1 and t.is_contiguous() and t.numel() >= 1
    assert g.closes.dtype == torch.int32 and g.closes.is_cuda and g.closes.dim() == 2 and g.closes.shape[1] == 4 and g.closes.is_contiguous()
    assert g.closes.shape[0] >= B
    out = (t.data_ptr(), t.numel(), g.closes.data_ptr())
    if rows_form:
        b = g.budget
        assert b is not None, "the rows form of the closing head takes the rows' budgets"
        assert b.dtype == torch.int32 and b.is_cuda and b.dim() == 1 and b.is_contiguous() and b.numel() >= B
        out += (b.data_ptr(),)
    return out


NO_STEER = (-1, 0.0, 0.0)      # fo1_token_steer_t of a row without a steer: no bias row, both penalties off


def token_steers(rows: Sequence, device=None) -> torch.Tensor:
    """The fo1_token_steer_t table (int32 [B, 4] holding int32, fp32, fp32, int32) from rows of (bias_row, frequency_penalty,
    presence_penalty) — a row of the bias table (-1 = none) and the two count penalties (include/fo1.h) — or None for a row without a steer.
    On `device` when given, else a host tensor."""
    import struct
    rows = [NO_STEER if r is None else r for r in rows]
    raw = b"".join(struct.pack("<iffi", int(r[0]), float(r[1] or 0.0), float(r[2] or 0.0), 0) for r in rows)
    tab = torch.frombuffer(bytearray(raw), dtype=torch.int32).view(-1, 4)
    return tab if device is None else tab.to(device)


def count_penalty_on(f, q) -> bool:
    """The device's rule: a row's count penalty is on iff both penalties are finite (as fp32) and not both zero."""
    import math
    f, q = (float(torch.tensor(float(x or 0.0), dtype=torch.float32)) for x in (f, q))      # (a value beyond fp32's range is inf there)
    return math.isfinite(f) and math.isfinite(q) and (f != 0.0 or q != 0.0)


def gate_of(table: torch.Tensor, n_vocab: int) -> torch.Tensor:
    """The gate bitmap (int32 [rows, seen_words(n_vocab)], the seen bitmap's layout) of a bias table (bf16) or a count table (int16 holding
    uint16) [rows, >= n_vocab]: bit i of a row set iff entry i < n_vocab of the table's row is not zero (-0 counts as zero)."""
    V = int(n_vocab)
    bits = table[:, :V].contiguous().view(torch.int16)
    nz = (bits & 0x7fff) != 0 if table.dtype == torch.bfloat16 else bits != 0
    pad = torch.zeros(nz.shape[0], seen_words(V) * 32, dtype=torch.int64, device=table.device)
    pad[:, :V] = nz
    w = (pad.view(nz.shape[0], -1, 32) << torch.arange(32, device=table.device)).sum(-1)      # < 2^32, the sign bit folded below
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


class SteerOperands(NamedTuple):
    """What a steered head takes (include/fo1.h): steers (token_steers, int32 [>= B, 4]); bias bf16 [bias rows, ld_bias >= V] with bias_gate
    (gate_of) int32 [bias rows, ld_words], or None for both; counts int16 [>= B, ld_counts >= V, even] holding the uint16 counts with
    count_gate int32 [>= B, ld_words], or None for both (then no row may have a count penalty on).  The accept form adds 1 to the accepted
    token's count and sets its gate bit."""
    steers: torch.Tensor
    bias: Optional[torch.Tensor] = None
    bias_gate: Optional[torch.Tensor] = None
    counts: Optional[torch.Tensor] = None
    count_gate: Optional[torch.Tensor] = None


def _steer_operands(s: SteerOperands, B: int, V: int):
    st = s.steers
    assert st.dtype == torch.int32 and st.is_cuda and st.dim() == 2 and st.shape[1] == 4 and st.is_contiguous() and st.shape[0] >= B
    ldg = 0
    pb = pg = pc = pcg = None
    rows_b = ld_b = ld_c = 0
    if s.bias is not None:
        b, g = s.bias, s.bias_gate
        assert g is not None, "a bias table comes with its gate bitmap (gate_of)"
        assert b.dtype == torch.bfloat16 and b.is_cuda and b.dim() == 2 and b.is_contiguous() and b.shape[0] >= 1 and b.shape[1] >= V
        assert g.dtype == torch.int32 and g.is_cuda and g.dim() == 2 and g.is_contiguous() and g.shape[0] >= b.shape[0]
        assert g.shape[1] % 4 == 0 and g.shape[1] * 32 >= V
        pb, pg, rows_b, ld_b, ldg = b.data_ptr(), g.data_ptr(), b.shape[0], b.shape[1], g.shape[1]
    if s.counts is not None:
        c, g = s.counts, s.count_gate
        assert g is not None, "a count table comes with its gate bitmap"
        assert c.dtype == torch.int16 and c.is_cuda and c.dim() == 2 and c.is_contiguous() and c.shape[0] >= B and c.shape[1] >= V and c.shape[1] % 2 == 0
        assert g.dtype == torch.int32 and g.is_cuda and g.dim() == 2 and g.is_contiguous() and g.shape[0] >= B
        assert g.shape[1] % 4 == 0 and g.shape[1] * 32 >= V and (ldg in (0, g.shape[1])), "the two gate bitmaps share one row length"
        pc, pcg, ld_c, ldg = c.data_ptr(), g.data_ptr(), c.shape[1], g.shape[1]
    return pb, pg, rows_b, ld_b, pc, pcg, ld_c, ldg, st.data_ptr()


def count_mark(counts: torch.Tensor, count_gate: torch.Tensor, n_vocab: int, rows: torch.Tensor, ids: torch.Tensor) -> None:
    """counts[rows[i], ids[i]] += 1 (int16 [R, ld_counts] holding uint16) and the matching bit of count_gate (int32 [R, ld_words]) set, duplicates
    included (fo1_count_mark); ids outside [0, n_vocab) and negative rows are skipped."""
    assert counts.dtype == torch.int16 and counts.is_cuda and counts.dim() == 2 and counts.is_contiguous()
    assert count_gate.dtype == torch.int32 and count_gate.is_cuda and count_gate.dim() == 2 and count_gate.is_contiguous()
    assert count_gate.shape[0] >= counts.shape[0]
    assert rows.dtype == ids.dtype == torch.int32 and rows.is_cuda and ids.is_cuda and rows.is_contiguous() and ids.is_contiguous() and rows.numel() == ids.numel()
    rc = _L.load().fo1_count_mark(counts.data_ptr(), counts.shape[1], count_gate.data_ptr(), count_gate.shape[1], int(n_vocab), _ptr(rows), _ptr(ids),
                                  rows.numel(), _stream())
    _L.check(rc, "fo1_count_mark")


def count_words(n_vocab: int) -> int:
    """Entries per row of a count table: n_vocab rounded up to a multiple of 8."""
    return -(-int(n_vocab) // 8) * 8


def _all_levels(masks, rules, guide, B: int, V: int, rows_form: bool):
    """The rule, guide and closing operands of a steered call, NULL for every level the caller left out."""
    ro = _rule_operands(masks, rules, B, V) if (masks is not None or rules is not None or guide is not None) else (None, 0, 0, None)
    go = _guide_operands(guide, B, V) if guide is not None else (None, 0, 0, None, 0, None, 0, None, None)
    if guide is not None and guide.closes is not None:
        co = _close_operands(guide, B, rows_form)
    else:
        co = (None, 0, None) + ((None,) if rows_form else ())
    return ro, go, co


def _sample_operands(logits: torch.Tensor, params: torch.Tensor):
    _chk(logits, "logits")
    pl, ld, B, V = _rows(logits, "logits")
    _chk(params, "params", torch.int32)
    assert params.is_contiguous() and params.dim() == 2 and params.shape[1] == 8 and params.shape[0] >= B
    n = _L.load().fo1_sample_rows_workspace_bytes(V, B)
    ws = _workspace("sample_rows", logits.device, max(int(n), 1))
    return (pl, ld, V, B, params.data_ptr()), (ws.data_ptr(), ws.numel(), _stream())


def sample_rows(logits: torch.Tensor, params: torch.Tensor, counter: Optional[torch.Tensor] = None, counter_stride: int = 1,
                u: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, seen: Optional[torch.Tensor] = None,
                general: bool = False, masks: Optional[torch.Tensor] = None, rules: Optional[torch.Tensor] = None,
                guide: Optional[GuideOperands] = None, steer: Optional[SteerOperands] = None) -> torch.Tensor:
    """int32 [B]: one sampled id per row of logits [B, V] bf16 (fo1_sample_rows_bf16): temperature / top-k / top-p per row from `params`
    (sample_params), draw = Philox(counter, stream; seed) with counter = counter[b * counter_stride] (device int32; None = 0), or the explicit
    u [B] fp32.  seen (int32 [>= B, ld_words] bitmap) or general=True: the general head (fo1_sample_rows_seen_bf16), which also honours a
    row's greedy flag and its repetition penalty; without a bitmap no row may have a penalty on.  masks (int32 [R, ld_words], a set bit = token
    banned) and rules (token_rules, int32 [>= B, 4]): the ruled head (fo1_sample_rows_ruled_bf16), the general head behind each row's bans.
    guide (GuideOperands, with masks and rules): the guided head (fo1_sample_rows_guided_bf16) — a guided row b picks in state guide.gstate[b]
    and the state after the pick is written back; with guide.closes the closing head (fo1_sample_rows_closing_bf16), where guide.budget[b] -
    counter - 1 tokens may follow row b's pick.  steer (SteerOperands): the steered head (fo1_sample_rows_steered_bf16) — each row's additive
    bias and count penalties on top of whichever of the forms above the other arguments select."""
    head, tail = _sample_operands(logits, params)
    B = head[3]
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=logits.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == B
    if counter is not None:
        assert counter.dtype == torch.int32 and counter.is_cuda and counter.numel() > (B - 1) * counter_stride
    if u is not None:
        assert u.dtype == torch.float32 and u.is_cuda and u.is_contiguous() and u.numel() == B
    if steer is not None:
        ps, ldw = _seen_operand(seen, B, head[2])
        ro, go, co = _all_levels(masks, rules, guide, B, head[2], True)
        rc = _L.load().fo1_sample_rows_steered_bf16(*head, _ptr(counter), int(counter_stride), _ptr(u), out.data_ptr(), *tail[:2], ps, ldw, *ro, tail[2],
                                                    *go, *co, *_steer_operands(steer, B, head[2]))
        _L.check(rc, "fo1_sample_rows_steered_bf16")
        return out
    if guide is not None and guide.closes is not None:
        ps, ldw = _seen_operand(seen, B, head[2])
        rc = _L.load().fo1_sample_rows_closing_bf16(*head, _ptr(counter), int(counter_stride), _ptr(u), out.data_ptr(), *tail[:2], ps, ldw,
                                                    *_rule_operands(masks, rules, B, head[2]), tail[2], *_guide_operands(guide, B, head[2]),
                                                    *_close_operands(guide, B, True))
        _L.check(rc, "fo1_sample_rows_closing_bf16")
        return out
    if guide is not None:
        ps, ldw = _seen_operand(seen, B, head[2])
        rc = _L.load().fo1_sample_rows_guided_bf16(*head, _ptr(counter), int(counter_stride), _ptr(u), out.data_ptr(), *tail[:2], ps, ldw,
                                                   *_rule_operands(masks, rules, B, head[2]), tail[2], *_guide_operands(guide, B, head[2]))
        _L.check(rc, "fo1_sample_rows_guided_bf16")
        return out
    if masks is not None or rules is not None:
        ps, ldw = _seen_operand(seen, B, head[2])
        rc = _L.load().fo1_sample_rows_ruled_bf16(*head, _ptr(counter), int(counter_stride), _ptr(u), out.data_ptr(), *tail[:2], ps, ldw,
                                                  *_rule_operands(masks, rules, B, head[2]), tail[2])
        _L.check(rc, "fo1_sample_rows_ruled_bf16")
        return out
    if seen is not None or general:
        ps, ldw = _seen_operand(seen, B, head[2])
        rc = _L.load().fo1_sample_rows_seen_bf16(*head, _ptr(counter), int(counter_stride), _ptr(u), out.data_ptr(), *tail[:2], ps, ldw, tail[2])
        _L.check(rc, "fo1_sample_rows_seen_bf16")
        return out
    rc = _L.load().fo1_sample_rows_bf16(*head, _ptr(counter), int(counter_stride), _ptr(u), out.data_ptr(), *tail)
    _L.check(rc, "fo1_sample_rows_bf16")
    return out


def decode_sample_accept(logits: torch.Tensor, params: torch.Tensor, state: torch.Tensor, plan: torch.Tensor, ids_out: torch.Tensor,
                         stop_ids: Optional[torch.Tensor], done: torch.Tensor) -> None:
    """The sampled head of a decode step (fo1_decode_sample_accept): decode_argmax_accept's bookkeeping around a draw whose counter is
    state[b, 4]."""
    B = state.shape[0]
    assert state.dtype == plan.dtype == ids_out.dtype == done.dtype == torch.int32 and ids_out.is_contiguous() and plan.is_contiguous()
    assert state.is_contiguous() and logits.shape[0] == B
    head, tail = _sample_operands(logits, params)
    n_stop = int(stop_ids.numel()) if stop_ids is not None else 0
    rc = _L.load().fo1_decode_sample_accept(*head, state.data_ptr(), plan.data_ptr(), ids_out.data_ptr(), ids_out.shape[1],
                                            stop_ids.data_ptr() if n_stop else None, n_stop, done.data_ptr(), *tail)
    _L.check(rc, "fo1_decode_sample_accept")


def decode_head_accept(logits: torch.Tensor, params: torch.Tensor, state: torch.Tensor, plan: torch.Tensor, ids_out: torch.Tensor,
                       stop_ids: Optional[torch.Tensor], done: torch.Tensor, seen: Optional[torch.Tensor] = None,
                       per_sequence_sets: bool = False, masks: Optional[torch.Tensor] = None, rules: Optional[torch.Tensor] = None,
                       guide: Optional[GuideOperands] = None, steer: Optional[SteerOperands] = None) -> None:
    """The general head of a decode step (fo1_decode_head_accept): decode_sample_accept with each row's greedy flag and repetition penalty
    honoured; the accepted token's bit is set in the row's `seen` bitmap (int32 [>= B, ld_words]; None only when no row has a penalty).
    per_sequence_sets: as decode_argmax_accept.  masks / rules (as sample_rows takes them): the ruled head (fo1_decode_head_ruled_accept), which
    reads both tables and writes neither.  guide (GuideOperands, with masks and rules): the guided head (fo1_decode_head_guided_accept), which
    also advances guide.gstate, the only guide table it writes; with guide.closes the closing head (fo1_decode_head_closing_accept).
    steer (SteerOperands): the steered head (fo1_decode_head_steered_accept) on top of whichever form the other arguments select; it counts
    the accepted token in steer.counts / steer.count_gate."""
    B = state.shape[0]
    assert state.dtype == plan.dtype == ids_out.dtype == done.dtype == torch.int32 and ids_out.is_contiguous() and plan.is_contiguous()
    assert state.is_contiguous() and logits.shape[0] == B
    head, tail = _sample_operands(logits, params)
    n_stop = int(stop_ids.numel()) if stop_ids is not None else 0
    if per_sequence_sets:
        assert stop_ids is not None and stop_ids.dim() == 2 and stop_ids.shape[1] == 17 and stop_ids.is_contiguous() and stop_ids.dtype == torch.int32
        n_stop = -1
    ps, ldw = _seen_operand(seen, B, head[2])
    if steer is not None:
        ro, go, co = _all_levels(masks, rules, guide, B, head[2], False)
        rc = _L.load().fo1_decode_head_steered_accept(*head, state.data_ptr(), plan.data_ptr(), ids_out.data_ptr(), ids_out.shape[1],
                                                      stop_ids.data_ptr() if n_stop else None, n_stop, done.data_ptr(), *tail[:2], ps, ldw, *ro, tail[2],
                                                      *go, *co, *_steer_operands(steer, B, head[2]))
        _L.check(rc, "fo1_decode_head_steered_accept")
        return
    if guide is not None and guide.closes is not None:
        rc = _L.load().fo1_decode_head_closing_accept(*head, state.data_ptr(), plan.data_ptr(), ids_out.data_ptr(), ids_out.shape[1],
                                                      stop_ids.data_ptr() if n_stop else None, n_stop, done.data_ptr(), *tail[:2], ps, ldw,
                                                      *_rule_operands(masks, rules, B, head[2]), tail[2], *_guide_operands(guide, B, head[2]),
                                                      *_close_operands(guide, B, False))
        _L.check(rc, "fo1_decode_head_closing_accept")
        return
    if guide is not None:
        rc = _L.load().fo1_decode_head_guided_accept(*head, state.data_ptr(), plan.data_ptr(), ids_out.data_ptr(), ids_out.shape[1],
                                                     stop_ids.data_ptr() if n_stop else None, n_stop, done.data_ptr(), *tail[:2], ps, ldw,
                                                     *_rule_operands(masks, rules, B, head[2]), tail[2], *_guide_operands(guide, B, head[2]))
        _L.check(rc, "fo1_decode_head_guided_accept")
        return
    if masks is not None or rules is not None:
        rc = _L.load().fo1_decode_head_ruled_accept(*head, state.data_ptr(), plan.data_ptr(), ids_out.data_ptr(), ids_out.shape[1],
                                                    stop_ids.data_ptr() if n_stop else None, n_stop, done.data_ptr(), *tail[:2], ps, ldw,
                                                    *_rule_operands(masks, rules, B, head[2]), tail[2])
        _L.check(rc, "fo1_decode_head_ruled_accept")
        return
    rc = _L.load().fo1_decode_head_accept(*head, state.data_ptr(), plan.data_ptr(), ids_out.data_ptr(), ids_out.shape[1],
                                          stop_ids.data_ptr() if n_stop else None, n_stop, done.data_ptr(), *tail[:2], ps, ldw, tail[2])
    _L.check(rc, "fo1_decode_head_accept")


LOGPROB_TOP_MAX = 8      # FO1_LOGPROB_TOP_MAX: top-n alternatives a log-probability record keeps per token


def logprob_rows(logits: torch.Tensor, ids: torch.Tensor, top_n: int = 0):
    """Log-probabilities of the chosen ids (int32 [B], device) on the rows of logits [B, V] bf16, and the top_n alternatives per row
    (fo1_logprob_rows_bf16: the log-softmax of the raw logits over their finite entries, include/fo1.h) ->
    (lp float32 [B], top_ids int32 [B, top_n], top_lp float32 [B, top_n])."""
    _chk(logits, "logits")
    pl, ld, B, V = _rows(logits, "logits")
    _chk(ids, "ids", torch.int32)
    assert ids.is_contiguous() and ids.numel() == B
    top_n = int(top_n)
    lp = torch.empty(B, dtype=torch.float32, device=logits.device)
    tid = torch.empty(B, max(top_n, 0), dtype=torch.int32, device=logits.device)
    tlp = torch.empty(B, max(top_n, 0), dtype=torch.float32, device=logits.device)
    rc = _L.load().fo1_logprob_rows_bf16(pl, ld, V, B, ids.data_ptr(), top_n, lp.data_ptr(), tid.data_ptr() if top_n > 0 else None,
                                         tlp.data_ptr() if top_n > 0 else None, max(top_n, 0), _stream())
    _L.check(rc, "fo1_logprob_rows_bf16")
    return lp, tid, tlp


def decode_logprob_record(logits: torch.Tensor, want: torch.Tensor, state: torch.Tensor, ids: torch.Tensor, n_rec: torch.Tensor,
                          lp: torch.Tensor, top_ids: torch.Tensor, top_lp: torch.Tensor) -> None:
    """The log-probability record of a decode step, launched after its head (fo1_decode_logprob_record): row b with want[b] >= 0 whose
    state[b, 4] = n has advanced past n_rec[b] scores ids[b, n - 1] on `logits` into column n - 1 of lp [B, ids_ld] and of top_ids / top_lp
    [B, ids_ld, LOGPROB_TOP_MAX], and sets n_rec[b] = n."""
    _chk(logits, "logits")
    pl, ld, B, V = _rows(logits, "logits")
    cap = ids.shape[1]
    assert want.dtype == state.dtype == ids.dtype == n_rec.dtype == top_ids.dtype == torch.int32 and lp.dtype == top_lp.dtype == torch.float32
    assert all(t.is_cuda and t.is_contiguous() for t in (want, state, ids, n_rec, lp, top_ids, top_lp))
    assert state.shape[0] == B and ids.shape[0] == B and want.numel() == B and n_rec.numel() == B
    assert tuple(lp.shape) == (B, cap) and tuple(top_ids.shape) == tuple(top_lp.shape) == (B, cap, LOGPROB_TOP_MAX)
    rc = _L.load().fo1_decode_logprob_record(pl, ld, V, B, want.data_ptr(), state.data_ptr(), ids.data_ptr(), cap, n_rec.data_ptr(),
                                             lp.data_ptr(), top_ids.data_ptr(), top_lp.data_ptr(), _stream())
    _L.check(rc, "fo1_decode_logprob_record")


def kv_relocate(ksrc: torch.Tensor, kdst: torch.Tensor, vsrc: torch.Tensor, vdst: torch.Tensor, seqs: torch.Tensor, max_len: int) -> None:
    """k*: [layers, n_kv, rows, 128]; v*: [layers, n_kv*128, rows]; seqs int32 [B, 4] = (src0, dst0, len, 0) on the device."""
    for t in (ksrc, kdst, vsrc, vdst):
        _chk(t, "cache")
    assert ksrc.dim() == 4 and vsrc.dim() == 3 and seqs.dtype == torch.int32 and seqs.is_contiguous()
    rc = _L.load().fo1_kv_relocate(ksrc.data_ptr(), kdst.data_ptr(), ksrc.stride(0), ksrc.stride(1), kdst.stride(0), kdst.stride(1),
                                   vsrc.data_ptr(), vdst.data_ptr(), vsrc.stride(0), vsrc.stride(1), vdst.stride(0), vdst.stride(1),
                                   seqs.data_ptr(), seqs.shape[0], int(max_len), ksrc.shape[1], ksrc.shape[0], _stream())
    _L.check(rc, "fo1_kv_relocate")


def decode_qkv_post(qkv_row: torch.Tensor, n_q_heads: int, n_kv_heads: int, head_dim: int, cos_table: torch.Tensor,
                    sin_table: torch.Tensor, state: torch.Tensor, kcache: torch.Tensor, vtcache: torch.Tensor) -> None:
    _chk(qkv_row, "qkv_row"); _chk(kcache, "kcache"); _chk(vtcache, "vtcache")
    assert qkv_row.shape[0] == 1 and qkv_row.stride(1) == 1 and kcache.dim() == 3 and state.dtype == torch.int32
    pv, ldv, _, _ = _rows(vtcache, "vtcache")
    rc = _L.load().fo1_decode_qkv_post_bf16(qkv_row.data_ptr(), n_q_heads, n_kv_heads, head_dim, cos_table.data_ptr(), sin_table.data_ptr(),
                                            state.data_ptr(), kcache.data_ptr(), kcache.stride(0), pv, ldv, _stream())
    _L.check(rc, "fo1_decode_qkv_post_bf16")


def decode_advance(state: torch.Tensor) -> None:
    assert state.dtype == torch.int32 and state.numel() >= 8 and state.is_contiguous()
    _L.check(_L.load().fo1_decode_advance(state.data_ptr(), _stream()), "fo1_decode_advance")


ATTN32_MAX_ROW_BYTES = 8192     # widest K row pitch of the engine (bytes): see pick_q_block


def _check_attn32_extent(q_block: int, rows: int, row_bytes: int) -> None:
    """fo1_attention_bf16 with q_block 128 / 256 builds 32-bit byte offsets from the K base: fail loudly instead of reading zeros."""
    if q_block >= 128 and rows * row_bytes >= 2 ** 32:
        raise ValueError(f"attention: q_block {q_block} addresses K rows with 32-bit byte offsets; {rows} rows x {row_bytes} B exceed 4 GiB — build the items with q_block 64")


def pick_q_block(segments: Sequence[Sequence[int]], n_heads: int, head_dim: int = 0, n_kv_heads: Optional[int] = None) -> int:
    """Query block of an attention work list.
    64 (/ 32 / 16) = the 16x16-MFMA kernel, 4 / 2 / 1 waves x 16 queries per workgroup — smaller blocks re-stage every K/V tile once
    per block and LOSE (LLM prefill L=515: 64 -> 1.9 ms, auto 16/32 -> 4.7 ms per image), so 64 is the floor.
    128 / 256 = the 32x32-MFMA kernel (attn_fwd32_kernel, head dim 80 / 128, round 5): 8 waves x 32 queries per workgroup —
    128 queries x the TWO query heads of one KV head when the model is grouped-query (LLM prefill: both heads share the staged
    K / V^T tile), 256 queries of one head otherwise (ViT full attention).  Short segments (ViT windows of 64 tokens, DaViT's 144-token
    windows at head dim 32, one-token extends) stay on the 64-query kernel.  FO1_ATTN32=0 turns the new form off (A/B)."""
    if head_dim in (80, 128) and os.environ.get("FO1_ATTN32", "1") != "0" and len(segments):
        # the 32x32 form addresses K / V^T rows through buffer descriptors with 32-bit byte offsets from the operand's base: the
        # last key row must stay below 2^32 bytes at the WIDEST row pitch the engine uses (head-major ViT q/k/v: 16 heads x 256 elements =
        # 8 KB per token) — 524k rows; past that the 16x16 kernel (64-bit addresses) takes the launch
        if max(int(e) for _, e, *_ in segments) * ATTN32_MAX_ROW_BYTES >= 2 ** 32:
            return 64
        longest = max(int(e) - int(s) for s, e, *_ in segments)
        group = n_heads // (n_kv_heads or n_heads)
        if head_dim == 128 and group % 2 == 0 and longest > 64:
            return 128
        if longest >= 192:
            return 256
    return 64


def order_items(rows, block: int, causal: bool, prefix=None):
    """Work-list order of the 32x32 attention form (q_block >= 128): descending cost = key tiles the item walks (its own range — up to its
    last query when causal — plus its second range).  The kernel's grid walks the items slowest, so this is longest-processing-time-first
    over the launch: the few-tile blocks fill the tail instead of a 48-tile block starting last (hires LLM: items of 2..48 tiles).
    A pure permutation of the work: every query's arithmetic is unchanged.  -> index permutation."""
    if block < 128:
        return list(range(len(rows)))
    def cost(i):
        q0, q1, k0, k1 = rows[i]
        own = (min(k1, q1) if causal else k1) - k0
        pre = 0 if prefix is None else max(0, prefix[i][1] - prefix[i][0])
        return -((own + 63) // 64 + (pre + 63) // 64)
    return sorted(range(len(rows)), key=cost)


def make_items(segments: Sequence[Sequence[int]], device, causal: bool = False, block: int = 64) -> torch.Tensor:
    """Host-side work list for fo1_attention_bf16: split every segment [start, end) into query blocks
    of <= block.  Index bookkeeping belongs on the host.  The block size rides along as
    attribute `q_block` of the returned tensor."""
    rows = []
    for s, e in segments:
        for q0 in range(s, e, block):
            rows.append((q0, min(q0 + block, e), s, e))
    rows = [rows[i] for i in order_items(rows, block, causal)]
    t = torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(device)
    t.q_block = block
    return t


def _qkv_rows(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor):
    """The checked q / k / V^T operands of the prefill attention front ends -> (rows of q, (q ptr, ld), (k ptr, ld), (V^T ptr, ld))."""
    _chk(q, "q"); _chk(k, "k"); _chk(vt, "vt")
    pq, ldq, L, _ = _rows(q, "q")
    pk, ldk, _, _ = _rows(k, "k")
    pv, ldv, _, _ = _rows(vt, "vt")
    return L, (pq, ldq), (pk, ldk), (pv, ldv)


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, items: torch.Tensor, n_q_heads: int, n_kv_heads: int,
              head_dim: int, scale: float, causal: bool, out: Optional[torch.Tensor] = None,
              flops: float = 0.0, qk_head_stride: Optional[int] = None) -> torch.Tensor:
    """q: [L, >= n_q_heads*head_dim] view (heads contiguous), k: [Lk, ...] view, vt: [n_kv_heads*head_dim, ld] (V^T).
    qk_head_stride: elements between consecutive heads of q and of k when they are not packed (the head-major q/k/v layout of
    qkv_proj_rope mode 1: 256).  Returns out [L, n_q_heads*head_dim]."""
    assert items.dtype == torch.int32 and items.is_contiguous() and items.device == q.device
    L, rq, rk, rv = _qkv_rows(q, k, vt)
    if out is None:
        out = torch.empty(L, n_q_heads * head_dim, dtype=torch.bfloat16, device=q.device)
    po, ldo, _, _ = _rows(out, "out")
    hs = head_dim if qk_head_stride is None else int(qk_head_stride)
    _check_attn32_extent(getattr(items, "q_block", 64), k.shape[0], rk[1] * 2)
    rc = _L.load().fo1_attention_bf16(*rq, hs, *rk, hs, *rv, po, ldo, head_dim,
                                      items.data_ptr(), items.shape[0], getattr(items, "q_block", 64), n_q_heads, n_kv_heads,
                                      head_dim, float(scale), 1 if causal else 0, None, float(flops), _stream())
    _L.check(rc, "fo1_attention_bf16")
    return out


def single_tile_items(segments: Sequence[Sequence[int]], head_dim: int) -> bool:
    """True when the work list of these segments can go to fo1_attention_windows_bf16: head dim 80 and every segment at most 64 tokens (make_items
    with block 64 then lists one item per segment).  FO1_WINATTN=0 turns it off (A/B)."""
    if head_dim != 80 or os.environ.get("FO1_WINATTN", "1") == "0" or not len(segments):
        return False
    return all(0 < int(e) - int(s) <= 64 for s, e, *_ in segments)


def attention_windows(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, items: torch.Tensor, n_heads: int, head_dim: int, scale: float,
                      flops: float = 0.0, qk_head_stride: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.attention (non-causal, q_block 64) for a work list of single-tile items (items.single_tile, see single_tile_items): the pipelined
    fo1_attention_windows_bf16, the same bits.  out: an optional [L, n_heads*head_dim] row-major view (any row stride) to write into."""
    assert items.dtype == torch.int32 and items.is_contiguous() and items.device == q.device and getattr(items, "single_tile", False)
    L, rq, rk, rv = _qkv_rows(q, k, vt)
    out = _out_rows(out, L, n_heads * head_dim, q.device)
    hs = head_dim if qk_head_stride is None else int(qk_head_stride)
    rc = _L.load().fo1_attention_windows_bf16(*rq, hs, *rk, hs, *rv, out.data_ptr(), out.stride(0), head_dim, L, items.data_ptr(), items.shape[0],
                                              n_heads, n_heads, head_dim, float(scale), float(flops), _stream())
    _L.check(rc, "fo1_attention_windows_bf16")
    return out


# ---- DaViT / SimpleFPN / splice helpers -----------------------------------------------------
# Every spatial op takes the geometry of its batch: a Grid (same-size images stacked along the rows, the `_bf16` entry) or an ImgSegs
# (images of different sizes packed row-wise, the `_var_bf16` entry reading a device table).  Both answer what a front end needs.
class Grid:
    """`batch` images of H x W pixels (or tokens) stacked along the row dimension ([batch*H*W, C]).  Host arithmetic only."""
    ragged = False

    def __init__(self, H: int, W: int, batch: int = 1):
        self.H, self.W, self.batch = int(H), int(W), int(batch)
        self.n, self.max_in, self.total_in = self.batch, self.H * self.W, self.batch * self.H * self.W

    @property
    def sizes(self):
        return ((self.H, self.W),) * self.batch

    def conv_out(self, KH: int, KW: int, stride: int, pad: int) -> "Grid":
        return Grid((self.H + 2 * pad - KH) // stride + 1, (self.W + 2 * pad - KW) // stride + 1, self.batch)

    def scaled(self, num: int, den: int = 1) -> "Grid":
        """The grid of a 2x transposed convolution (2) or of a 2 x 2 max-pool (1, 2)."""
        return Grid(self.H * num // den, self.W * num // den, self.batch)

    def windows(self, ws: int) -> "Grid":
        """Padded to whole ws x ws windows."""
        return Grid(-(-self.H // ws) * ws, -(-self.W // ws) * ws, self.batch)

    def rows_out(self, out_grid) -> int:
        return out_grid(self).total_in

    def args(self, side: str, *mid):
        """The geometry arguments of a uniform entry, around the operator's own `mid`."""
        return (self.H, self.W, *mid, self.batch)


class ImgSegs:
    """Per-operator geometry table of a ragged batch: host rows [(in_row0, H, W, out_row0, Ho, Wo)] -> device int32 [n, 8] + the sizes
    the launch needs (largest image, totals).  Built once per batch signature (the tower plans cache them).  include/fo1.h fo1_img_seg."""
    ragged = True

    def __init__(self, rows, device, max_in: int, total_in: int, max_out: int, total_out: int):
        t = torch.zeros(len(rows), 8, dtype=torch.int32)
        for i, r in enumerate(rows):
            t[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
        self.dev = t.to(device)
        self.n = len(rows)
        self.max_in, self.total_in, self.max_out, self.total_out = int(max_in), int(total_in), int(max_out), int(total_out)

    @property
    def ptr(self):
        return self.dev.data_ptr()

    def rows_out(self, out_grid) -> int:
        return self.total_out

    def args(self, side: str, *mid):
        """The geometry arguments of a ragged entry; `side` says whether it sizes its grid by the input or the output extents."""
        return (self.ptr, self.n, getattr(self, "max_" + side), getattr(self, "total_" + side), *mid)


def _packed(t: torch.Tensor, name: str, rows: int) -> None:
    _chk(t, name)
    assert t.is_contiguous() and t.shape[0] == rows, f"{name}: need {rows} contiguous rows, got shape {tuple(t.shape)} strides {t.stride()}"


def _new_rows(rows: int, cols: int, device, zero: bool = False) -> torch.Tensor:
    return (torch.zeros if zero else torch.empty)(rows, cols, dtype=torch.bfloat16, device=device)


def _spatial(entry: str, geom, head, geo_args, tail=()) -> None:
    """Launch the uniform (`<entry>_bf16`) or the ragged (`<entry>_var_bf16`) form of a spatial operator."""
    name = entry + ("_var_bf16" if geom.ragged else "_bf16")
    _L.check(getattr(_L.load(), name)(*head, *geo_args, *tail, _stream()), name)


def dwconv3x3_res(x: torch.Tensor, w9c: torch.Tensor, bias: torch.Tensor, H: int, W: int, batch: int = 1) -> torch.Tensor:
    """x [batch*H*W, C] token-major -> x + dwconv3x3(x) (+bias); w9c is the [9, C] tap-major weight."""
    _chk(x, "x"); _chk(w9c, "w9c"); _chk(bias, "bias")
    assert x.is_contiguous() and x.shape[0] == batch * H * W and w9c.shape == (9, x.shape[1]) and w9c.is_contiguous()
    y = torch.empty_like(x)
    _L.check(_L.load().fo1_dwconv3x3_bf16(x.data_ptr(), w9c.data_ptr(), bias.data_ptr(), y.data_ptr(), H, W, x.shape[1], batch, _stream()),
             "fo1_dwconv3x3_bf16")
    return y


def dwconv3x3_res_ln(x: torch.Tensor, w9c: torch.Tensor, bias: torch.Tensor, geom, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float):
    """-> (y = x + dwconv3x3(x) + bias, LayerNorm(y)) in one launch (fo1_dwconv3x3_ln[_var]_bf16), bit-identical to
    dwconv3x3_res followed by layernorm."""
    _packed(x, "x", geom.total_in); _chk(w9c, "w9c"); _chk(bias, "bias"); _chk(ln_w, "ln_w"); _chk(ln_b, "ln_b")
    assert w9c.shape == (9, x.shape[1]) and w9c.is_contiguous()
    y, h = torch.empty_like(x), torch.empty_like(x)
    _spatial("fo1_dwconv3x3_ln", geom, (x.data_ptr(), w9c.data_ptr(), bias.data_ptr(), y.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), float(eps),
                                        h.data_ptr()), geom.args("in", x.shape[1]))
    return y, h


def im2col(x: torch.Tensor, geom, KH: int, KW: int, stride: int, pad: int, ld: Optional[int] = None) -> torch.Tensor:
    """x [rows of geom, C] -> col [output pixels, ld>=KH*KW*C] (pad columns zero); a Grid's output grid is geom.conv_out(KH, KW, stride, pad)."""
    _packed(x, "x", geom.total_in)
    C = x.shape[1]
    K = KH * KW * C
    ld = ld or K
    col = _new_rows(geom.rows_out(lambda g: g.conv_out(KH, KW, stride, pad)), ld, x.device, zero=ld != K)
    _spatial("fo1_im2col", geom, (x.data_ptr(), col.data_ptr()), geom.args("out", C, KH, KW, stride, pad, ld))
    return col


def window_partition(x: torch.Tensor, geom, ws: int) -> torch.Tensor:
    _packed(x, "x", geom.total_in)
    xw = _new_rows(geom.rows_out(lambda g: g.windows(ws)), x.shape[1], x.device)
    _spatial("fo1_window_partition", geom, (x.data_ptr(), xw.data_ptr()), geom.args("out", x.shape[1], ws))
    return xw


def window_reverse_add(yw: torch.Tensor, shortcut: torch.Tensor, geom, ws: int) -> torch.Tensor:
    _packed(yw, "yw", geom.rows_out(lambda g: g.windows(ws))); _packed(shortcut, "shortcut", geom.total_in)
    y = torch.empty_like(shortcut)
    _spatial("fo1_window_reverse_add", geom, (yw.data_ptr(), shortcut.data_ptr(), y.data_ptr()), geom.args("in", shortcut.shape[1], ws))
    return y


WINDOW_ATTENTION_MAX_TOKENS = 160      # fo1_window_attention_bf16: tokens per window the head-dim-32 kernel is built for


def window_attention(qkv: torch.Tensor, C: int, n_heads: int, window_tokens: int, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qkv [n_windows * window_tokens, 3C] (the q/k/v GEMM's rows of window-partitioned tokens) -> softmax(q k^T * scale) v per window and
    head, [rows, C] (fo1_window_attention_bf16: head dim 32, DaViT's WindowAttention modeling_davit.py:225-282)."""
    _chk(qkv, "qkv")
    p, ld, n, _ = _rows(qkv, "qkv")
    assert C == n_heads * 32 and n % window_tokens == 0 and window_tokens <= WINDOW_ATTENTION_MAX_TOKENS
    out = _out_rows(out, n, C, qkv.device)
    _L.check(_L.load().fo1_window_attention_bf16(p, ld, C, n_heads, window_tokens, n // window_tokens, out.data_ptr(), out.stride(0), float(scale), _stream()),
             "fo1_window_attention_bf16")
    return out


WINDOW_ATTENTION_MAP_WINDOW = 12       # fo1_window_attention_map_bf16: the window side its token -> pixel arithmetic is built for


def window_attention_map(qkv: torch.Tensor, C: int, n_heads: int, window: int, geom, pad_row: torch.Tensor, scale: float,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Window attention on UN-partitioned rows: qkv [rows of geom, 3C] = the q/k/v projection of the images' pixels in raster order; the windows'
    tokens are found by arithmetic, tokens outside the image read `pad_row` (the layer's bf16 q/k/v bias = the projection of the reference's zero
    padding, modeling_davit.py:248-251).  -> [rows, C] in pixel order (fo1_window_attention_map[_var]_bf16; a ragged geom is the
    window-partition table: pixels row0, H, W, -, windows down / across)."""
    _chk(qkv, "qkv"); _chk(pad_row, "pad_row")
    p, ld, n, _ = _rows(qkv, "qkv")
    assert C == n_heads * 32 and n == geom.total_in and window == WINDOW_ATTENTION_MAP_WINDOW and pad_row.numel() == 3 * C and pad_row.is_contiguous()
    out = _out_rows(out, n, C, qkv.device)
    geo = (geom.ptr, geom.n, geom.max_out // (window * window), geom.total_in) if geom.ragged else geom.args("in")
    _spatial("fo1_window_attention_map", geom, (p, ld, C, n_heads, window), geo, (pad_row.data_ptr(), out.data_ptr(), out.stride(0), float(scale)))
    return out


def channel_attention(qkv: torch.Tensor, C: int, geom) -> torch.Tensor:
    """qkv [rows of geom, 3C]: per image, per 32-channel group attention over the image's own tokens (a Grid's H * W; a ragged geom's rows
    are (row0, N_i))."""
    _chk(qkv, "qkv")
    p, ld, NB, _ = _rows(qkv, "qkv")
    assert NB == geom.total_in
    need = _L.load().fo1_channel_attention_workspace_bytes(geom.max_in, C, geom.n)
    ws = _workspace("channel_attention", qkv.device, need)
    out = _new_rows(NB, C, qkv.device)
    geo = (geom.ptr, geom.n, geom.max_in, geom.total_in, C, out.data_ptr(), C) if geom.ragged else (geom.max_in, C, out.data_ptr(), C, geom.n)
    _spatial("fo1_channel_attention", geom, (p, ld), geo, (ws.data_ptr(), ws.numel()))
    return out


def pixel_shuffle2(src: torch.Tensor, geom, Co: int) -> torch.Tensor:
    _packed(src, "src", geom.total_in)
    assert src.shape[1] == 4 * Co
    dst = _new_rows(geom.rows_out(lambda g: g.scaled(2)), Co, src.device)
    _spatial("fo1_pixel_shuffle2", geom, (src.data_ptr(), dst.data_ptr()), geom.args("in", Co))
    return dst


def maxpool2(x: torch.Tensor, geom) -> torch.Tensor:
    _packed(x, "x", geom.total_in)
    y = _new_rows(geom.rows_out(lambda g: g.scaled(1, 2)), x.shape[1], x.device)
    _spatial("fo1_maxpool2", geom, (x.data_ptr(), y.data_ptr()), geom.args("out", x.shape[1]))
    return y


def nchw_to_hwc8(img: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """img [3,H,W] or [B,3,H,W] bf16/fp32 -> [B*H*W, 8] bf16 (into `out` when given: the image's rows of a packed ragged batch)."""
    if img.device.type != "cuda":
        raise _L.Fo1Error("nchw_to_hwc8: expected a HIP device tensor")
    if img.dim() == 3:
        img = img.unsqueeze(0)
    assert img.dim() == 4 and img.shape[1] == 3 and img.is_contiguous() and img.dtype in (torch.bfloat16, torch.float32)
    B, _, H, W = img.shape
    if out is None:
        out = torch.empty(B * H * W, 8, dtype=torch.bfloat16, device=img.device)
    else:
        assert out.shape == (B * H * W, 8) and out.is_contiguous() and out.dtype == torch.bfloat16
    _L.check(_L.load().fo1_nchw_to_hwc8_bf16(img.data_ptr(), 1 if img.dtype == torch.float32 else 0, out.data_ptr(), H, W, B, _stream()),
             "fo1_nchw_to_hwc8_bf16")
    return out


def gather_rows(plan: torch.Tensor, D: int, t0: torch.Tensor, t1: Optional[torch.Tensor] = None, t2: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None):
    """out[r, :D] = table[plan[r,0]][plan[r,1], :D];  plan int32 [R,2] (kind, index) on device.  `out` may be
    wider than D (its other columns are left untouched)."""
    assert plan.dtype == torch.int32 and plan.is_contiguous()
    R = plan.shape[0]
    if out is None:
        out = torch.empty(R, D, dtype=torch.bfloat16, device=plan.device)
    po, ldo, Ro, Do = _rows(out, "out")
    assert Ro == R and Do >= D

    def pl(t):
        if t is None:
            return None, 0
        _chk(t, "table")
        assert t.dim() == 2 and t.stride(1) == 1 and t.shape[1] >= D
        return t.data_ptr(), t.stride(0)

    p0, l0 = pl(t0); p1, l1 = pl(t1); p2, l2 = pl(t2)
    _L.check(_L.load().fo1_gather_rows_bf16(p0, l0, p1, l1, p2, l2, plan.data_ptr(), po, ldo, R, D, _stream()),
             "fo1_gather_rows_bf16")
    return out


def gather_rows_into(plan: torch.Tensor, D: int, table: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    return gather_rows(plan, D, table, out=out)


def attention_strided(q: torch.Tensor, q_row0: int, k: torch.Tensor, vt: torch.Tensor, items: torch.Tensor, n_q_heads: int,
                      n_kv_heads: int, head_dim: int, scale: float, causal: bool, flops: float = 0.0,
                      out: Optional[torch.Tensor] = None, q_row_base: Optional[torch.Tensor] = None, n_items: Optional[int] = None,
                      prefix_ranges: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention against a KV cache.  q [Lq, n_q_heads*head_dim] holds absolute positions q_row0 .. q_row0+Lq (the
    items index absolute positions) — or, with `q_row_base` (device int32 scalar), positions *q_row_base + row so a
    captured graph can serve every decode step.  k is the cache [n_kv, Lmax, head_dim], vt the transposed V cache
    [n_kv*head_dim, Lmax]; `items` may be a raw int32 view (n_items rows of 4)."""
    _chk(q, "q"); _chk(k, "k"); _chk(vt, "vt")
    assert items.dtype == torch.int32 and items.is_contiguous()
    pq, ldq, Lq, _ = _rows(q, "q")
    assert k.dim() == 3 and k.stride(2) == 1
    pv, ldv, _, _ = _rows(vt, "vt")
    if out is None:
        out = torch.empty(Lq, n_q_heads * head_dim, dtype=torch.bfloat16, device=q.device)
    po, ldo, _, _ = _rows(out, "out")
    if q_row_base is not None:
        q_row0 = 0
    _check_attn32_extent(getattr(items, "q_block", 64), k.shape[1], k.stride(1) * 2)
    lib = _L.load()
    operands = (pq - q_row0 * ldq * 2, ldq, head_dim, k.data_ptr(), k.stride(1), k.stride(0), pv, ldv, po - q_row0 * ldo * 2, ldo, head_dim, items.data_ptr())
    shape = (getattr(items, "q_block", 64), n_q_heads, n_kv_heads, head_dim, float(scale), 1 if causal else 0)
    if prefix_ranges is not None:      # items with a second (shared-prefix) key range: fo1_attention_prefix_bf16
        assert prefix_ranges.dtype == torch.int32 and prefix_ranges.is_contiguous() and prefix_ranges.shape == (items.shape[0], 2) and q_row_base is None
        _L.check(lib.fo1_attention_prefix_bf16(*operands, prefix_ranges.data_ptr(), items.shape[0], *shape, float(flops), _stream()), "fo1_attention_prefix_bf16")
    else:
        _L.check(lib.fo1_attention_bf16(*operands, n_items if n_items is not None else items.shape[0], *shape,
                                        _ptr(q_row_base), float(flops), _stream()), "fo1_attention_bf16")
    return out


# ---- image preprocessing (device side) -------------------------------------------------------------------------------------
def patchify_u8(image_hwc: torch.Tensor, lut: torch.Tensor, patch: int = 14, merge: int = 2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [H, W, 3] (device) -> bf16 [S, 6*patch^2] normalised patches in merge-block order (fo1_patchify_u8_bf16); `out` may be a
    column view of a wider buffer (row stride >= 6*patch^2)."""
    if image_hwc.dtype != torch.uint8 or not image_hwc.is_cuda or image_hwc.dim() != 3 or image_hwc.shape[2] != 3 or not image_hwc.is_contiguous():
        raise ValueError("patchify_u8: need a contiguous device uint8 [H, W, 3] tensor")
    _chk(lut, "lut")
    assert lut.shape == (3, 256) and lut.is_contiguous()
    H, W, _ = image_hwc.shape
    if out is None:
        out = torch.empty((H // patch) * (W // patch), 6 * patch * patch, dtype=torch.bfloat16, device=image_hwc.device)
    _chk(out, "out")
    assert tuple(out.shape) == ((H // patch) * (W // patch), 6 * patch * patch) and out.stride(1) == 1
    _L.check(_L.load().fo1_patchify_u8_bf16(image_hwc.data_ptr(), H, W, lut.data_ptr(), out.data_ptr(), out.stride(0), patch, merge,
                                            _stream()), "fo1_patchify_u8_bf16")
    return out


def normalize_u8(image_hwc: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """uint8 [H, W, 3] (device) -> bf16 [3, H, W] normalised, channels first (fo1_normalize_u8_bf16)."""
    if image_hwc.dtype != torch.uint8 or not image_hwc.is_cuda or image_hwc.dim() != 3 or image_hwc.shape[2] != 3 or not image_hwc.is_contiguous():
        raise ValueError("normalize_u8: need a contiguous device uint8 [H, W, 3] tensor")
    _chk(lut, "lut")
    assert lut.shape == (3, 256) and lut.is_contiguous()
    H, W, _ = image_hwc.shape
    out = torch.empty(3, H, W, dtype=torch.bfloat16, device=image_hwc.device)
    _L.check(_L.load().fo1_normalize_u8_bf16(image_hwc.data_ptr(), H, W, lut.data_ptr(), out.data_ptr(), _stream()),
             "fo1_normalize_u8_bf16")
    return out


# ---- multi-scale deformable attention (msda.hip; UPN proposal detector) ----------------------------------
def ms_deform_attn(value: torch.Tensor, spatial_shapes: torch.Tensor, level_start_index: torch.Tensor, sampling_locations: torch.Tensor,
                   attention_weights: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """value [N, S, M, D] (fp32 | fp64 | bf16), spatial_shapes int64 [L, 2] and level_start_index int64 [L] on the device,
    sampling_locations [N, Lq, M, L, P, 2], attention_weights [N, Lq, M, L, P] (value's dtype; fp32 when value is bf16)
    -> [N, Lq, M*D] in value's dtype (fo1_ms_deform_attn_forward)."""
    for t, name in ((value, "value"), (spatial_shapes, "spatial_shapes"), (level_start_index, "level_start_index"),
                    (sampling_locations, "sampling_locations"), (attention_weights, "attention_weights")):
        if not t.is_cuda:
            raise RuntimeError(f"ms_deform_attn: {name} must live on the GPU (no CPU path exists)")
        if not t.is_contiguous():
            raise ValueError(f"ms_deform_attn: {name} must be contiguous")
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise TypeError("ms_deform_attn: spatial_shapes / level_start_index must be int64 (as the reference passes them)")
    N, S, M, D = value.shape
    _, Lq, M2, L, P, two = sampling_locations.shape
    if M2 != M or two != 2 or tuple(attention_weights.shape) != (N, Lq, M, L, P) or tuple(spatial_shapes.shape) != (L, 2) or level_start_index.numel() != L:
        raise ValueError("ms_deform_attn: inconsistent shapes")
    if value.dtype == torch.float32:
        dt, lt = 0, torch.float32
    elif value.dtype == torch.float64:
        dt, lt = 1, torch.float64
    elif value.dtype == torch.bfloat16:
        dt, lt = 2, torch.float32
    else:
        raise TypeError(f"ms_deform_attn: value dtype {value.dtype} not built (float32, float64, bfloat16)")
    if sampling_locations.dtype != lt or attention_weights.dtype != lt:
        raise TypeError(f"ms_deform_attn: sampling_locations / attention_weights must be {lt} for {value.dtype} values")
    if out is None:
        out = torch.empty(N, Lq, M * D, dtype=value.dtype, device=value.device)
    rc = _L.load().fo1_ms_deform_attn_forward(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_locations.data_ptr(),
                                              attention_weights.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr(), dt, _stream())
    _L.check(rc, "fo1_ms_deform_attn_forward")
    return out


def msda_fused(value: torch.Tensor, spatial_shapes: torch.Tensor, level_start_index: torch.Tensor, offsets_logits: torch.Tensor,
               reference_points: torch.Tensor, n_heads: int, n_points: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused MSDeformAttn core (fo1_msda_fused_bf16): value bf16 [N, S, C]; offsets_logits fp32 [N, Lq, M*L*P*3]
    ([sampling_offsets | attention_weights] rows of one GEMM); reference_points fp32 [N, Lq, L or 1, 2 | 4] -> bf16 [N, Lq, C]."""
    _chk(value, "value")
    for t, name in ((offsets_logits, "offsets_logits"), (reference_points, "reference_points")):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError(f"msda_fused: {name} must be a contiguous fp32 GPU tensor")
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64 or not spatial_shapes.is_cuda or not level_start_index.is_cuda:
        raise TypeError("msda_fused: spatial_shapes / level_start_index must be int64 GPU tensors")
    N, S, C = value.shape
    _, Lq, RL, RD = reference_points.shape
    L = spatial_shapes.shape[0]
    M, P = n_heads, n_points
    D = C // M
    if not value.is_contiguous() or tuple(offsets_logits.shape) != (N, Lq, M * L * P * 3) or RL not in (1, L):
        raise ValueError("msda_fused: inconsistent shapes")
    if out is None:
        out = torch.empty(N, Lq, C, dtype=torch.bfloat16, device=value.device)
    rc = _L.load().fo1_msda_fused_bf16(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), offsets_logits.data_ptr(),
                                       reference_points.data_ptr(), RL, RD, N, S, M, D, L, Lq, P, out.data_ptr(), _stream())
    _L.check(rc, "fo1_msda_fused_bf16")
    return out


def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = bf16(a + b) over [M, D] rows (fo1_add_bf16)."""
    _chk(a, "a"); _chk(b, "b")
    pa, lda, M, D = _rows(a, "a")
    pb, ldb, Mb, Db = _rows(b, "b")
    assert (M, D) == (Mb, Db)
    if out is None:
        out = torch.empty(M, D, dtype=torch.bfloat16, device=a.device)
    po, ldo, _, _ = _rows(out, "out")
    _L.check(_L.load().fo1_add_bf16(pa, lda, pb, ldb, po, ldo, M, D, _stream()), "fo1_add_bf16")
    return out


# ---- UPN query selection / decoder helpers (upn_ops.hip) -------------------------------------------------------------------
def _f32(t: torch.Tensor, name: str):
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
        raise TypeError(f"{name} must be a 2-d fp32 GPU tensor with unit column stride")
    return t.data_ptr(), t.stride(0), t.shape[0], t.shape[1]


def sine_embed(ref: torch.Tensor, dims: int = 4) -> torch.Tensor:
    """fp32 [n, >= dims] (x, y[, w, h]) -> bf16 [n, dims*128] (fo1_sine_embed_bf16)."""
    p, ld, n, _ = _f32(ref, "ref")
    out = torch.empty(n, dims * 128, dtype=torch.bfloat16, device=ref.device)
    _L.check(_L.load().fo1_sine_embed_bf16(p, ld, n, dims, out.data_ptr(), out.stride(0), _stream()), "fo1_sine_embed_bf16")
    return out


def box_refine(delta: torch.Tensor, ref: torch.Tensor, mode: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mode 0: sigmoid(delta[:, :4] + inverse_sigmoid(ref)); mode 1: delta[:, :4] + ref; mode 2: sigmoid(delta[:, :4] + ref).
    fp32 [n, 4] (fo1_box_refine_f32)."""
    pd, ldd, n, _ = _f32(delta, "delta")
    pr, ldr, nr, _ = _f32(ref, "ref")
    assert n == nr
    if out is None:
        out = torch.empty(n, 4, dtype=torch.float32, device=delta.device)
    po, ldo, _, _ = _f32(out, "out")
    _L.check(_L.load().fo1_box_refine_f32(pd, ldd, pr, ldr, po, ldo, n, mode, _stream()), "fo1_box_refine_f32")
    return out


def mask_rows(x: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    _chk(x, "x")
    px, ldx, M, D = _rows(x, "x")
    assert keep.dtype == torch.uint8 and keep.is_cuda and keep.numel() == M and keep.is_contiguous()
    y = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
    _L.check(_L.load().fo1_mask_rows_bf16(px, ldx, keep.data_ptr(), y.data_ptr(), y.stride(0), M, D, _stream()), "fo1_mask_rows_bf16")
    return y


def topk_desc(scores: torch.Tensor, k: int, stride: int = 1, n: Optional[int] = None):
    """scores fp32 (flat; element i at i*stride) -> (indices int32 [k], values fp32 [k]) in descending order (fo1_topk_desc_f32)."""
    if not scores.is_cuda or scores.dtype != torch.float32 or not scores.is_contiguous():
        raise TypeError("topk_desc: scores must be a contiguous fp32 GPU tensor")
    n = scores.numel() // stride if n is None else n
    ws = _workspace("topk", scores.device, _L.load().fo1_topk_workspace_bytes(n))
    idx = torch.empty(k, dtype=torch.int32, device=scores.device)
    val = torch.empty(k, dtype=torch.float32, device=scores.device)
    _L.check(_L.load().fo1_topk_desc_f32(scores.data_ptr(), stride, n, k, idx.data_ptr(), val.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "fo1_topk_desc_f32")
    return idx, val


def gather_rows_f32(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    pt, ldt, _, D = _f32(table, "table")
    assert idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous()
    out = torch.empty(idx.numel(), D, dtype=torch.float32, device=table.device)
    _L.check(_L.load().fo1_gather_rows_f32(pt, ldt, idx.data_ptr(), out.data_ptr(), out.stride(0), idx.numel(), D, _stream()), "fo1_gather_rows_f32")
    return out


# ---- UPN post-process (upn_post.hip) -----------------------------------------------------------------------------------------------
class UPNPost(NamedTuple):
    """Views into ONE int32 device block [images, 1 + 10 * cap] (`block`: one device-to-host copy returns everything): per image
    n_keep | keep_idx [cap] | boxes_f32 [cap, 4] | boxes_i32 [cap, 4] | scores [cap]; entries past n_keep are unwritten."""
    block: torch.Tensor
    n_keep: torch.Tensor       # int32 [images]
    keep_idx: torch.Tensor     # int32 [images, cap]
    boxes_f32: torch.Tensor    # fp32 [images, cap, 4]
    boxes_i32: torch.Tensor    # int32 [images, cap, 4]
    scores: torch.Tensor       # fp32 [images, cap]


def upn_post_views(block: torch.Tensor, cap: int) -> UPNPost:
    """The UPNPost views of an int32 block [images, 1 + 10 * cap], on the device or after its copy to the host."""
    n = block.shape[0]
    return UPNPost(block, block[:, 0], block[:, 1:1 + cap], block[:, 1 + cap:1 + 5 * cap].view(torch.float32).view(n, cap, 4),
                   block[:, 1 + 5 * cap:1 + 9 * cap].view(n, cap, 4), block[:, 1 + 9 * cap:1 + 10 * cap].view(torch.float32))


def upn_post_params(sizes_hw, min_score: float, iou_threshold: float, max_keep: int, device) -> torch.Tensor:
    """fo1_upn_post_params_t per image as an int32 device tensor [images, 5]: (W, H, min_score, iou_threshold) as fp32 bits, max_keep."""
    import numpy as np
    p = np.zeros((len(sizes_hw), 5), dtype=np.int32)
    f = p.view(np.float32)
    for i, (H, W) in enumerate(sizes_hw):
        f[i, :4] = (W, H, min_score, iou_threshold)
        p[i, 4] = max_keep
    return torch.from_numpy(p).to(device)


def upn_post(boxes: torch.Tensor, logits: torch.Tensor, params: torch.Tensor, cap: Optional[int] = None, out: Optional[torch.Tensor] = None) -> UPNPost:
    """postprocess + filter of the UPN wrapper on the device (fo1_upn_post_batch_f32; the definition: include/fo1.h): boxes fp32
    [Q, >= 4] or [images, Q, >= 4] (cx, cy, w, h), logits fp32 [Q] / [images, Q] (any element stride, e.g. a column of the class
    GEMM's output), params = upn_post_params(...).  One launch, grid = images; `cap` (default Q) bounds the kept entries per image."""
    if boxes.dim() == 2:
        boxes, logits = boxes[None], logits[None]
    if not (boxes.is_cuda and boxes.dtype == torch.float32 and boxes.dim() == 3 and boxes.shape[2] >= 4 and boxes.stride(2) == 1):
        raise TypeError("upn_post: boxes must be an fp32 GPU tensor [images, Q, >= 4] with unit column stride")
    n, Q = boxes.shape[0], boxes.shape[1]
    if not (logits.is_cuda and logits.dtype == torch.float32 and tuple(logits.shape) == (n, Q)):
        raise TypeError("upn_post: logits must be an fp32 GPU tensor [images, Q]")
    if not (params.is_cuda and params.dtype == torch.int32 and tuple(params.shape) == (n, 5) and params.is_contiguous()):
        raise TypeError("upn_post: params must be upn_post_params(...) for the same images")
    cap = Q if cap is None else cap
    if out is None:
        out = torch.empty(n, 1 + 10 * cap, dtype=torch.int32, device=boxes.device)
    elif not (out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (n, 1 + 10 * cap) and out.is_contiguous()):
        raise TypeError("upn_post: out must be a contiguous int32 GPU tensor [images, 1 + 10 * cap]")
    r = upn_post_views(out, cap)
    lib = _L.load()
    need = lib.fo1_upn_post_workspace_bytes(Q)
    ws = _workspace("upn_post", boxes.device, need) if need else None
    _L.check(lib.fo1_upn_post_batch_f32(boxes.data_ptr(), boxes.stride(1) if Q > 1 else 4, boxes.stride(0) if n > 1 else 0, logits.data_ptr(), logits.stride(1) if Q > 1 else 1,
                                        logits.stride(0) if n > 1 else 0, Q, n, params.data_ptr(), r.n_keep.data_ptr(), r.keep_idx.data_ptr(),
                                        r.boxes_f32.data_ptr(), r.boxes_i32.data_ptr(), r.scores.data_ptr(), cap, out.stride(0), _ptr(ws),
                                        ws.numel() if ws is not None else 0, _stream()), "fo1_upn_post_batch_f32")
    return r


# ---- Swin backbone pieces (swin_ops.hip, attention.hip) ------------------------------------------------------------------------
def attention_window_bias(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, items: torch.Tensor, n_heads: int, head_dim: int, scale: float,
                          bias: torch.Tensor, ws: int, shift: int, nwy: int, nwx: int, flops: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Swin W-MSA / SW-MSA over consecutive windows of ws*ws tokens (fo1_attention_window_bias_bf16); bias fp32 [heads, ws*ws, ws*ws]."""
    wlen = ws * ws
    if not bias.is_cuda or bias.dtype != torch.float32 or tuple(bias.shape) != (n_heads, wlen, wlen) or not bias.is_contiguous():
        raise TypeError("attention_window_bias: bias must be a contiguous fp32 GPU tensor [heads, ws*ws, ws*ws]")
    L, rq, rk, rv = _qkv_rows(q, k, vt)
    out = _out_rows(out, L, n_heads * head_dim, q.device)
    rc = _L.load().fo1_attention_window_bias_bf16(*rq, head_dim, *rk, head_dim, *rv, out.data_ptr(), out.stride(0), head_dim, items.data_ptr(),
                                                  items.shape[0], getattr(items, "q_block", 64), n_heads, head_dim, float(scale), bias.data_ptr(), wlen, ws,
                                                  shift, nwy, nwx, float(flops), _stream())
    _L.check(rc, "fo1_attention_window_bias_bf16")
    return out


def swin_window_partition(x: torch.Tensor, H: int, W: int, ws: int, shift: int, batch: int = 1) -> torch.Tensor:
    _chk(x, "x")
    assert x.is_contiguous() and x.shape[0] == batch * H * W
    C = x.shape[1]
    nwy, nwx = -(-H // ws), -(-W // ws)
    xw = torch.empty(batch * nwy * nwx * ws * ws, C, dtype=torch.bfloat16, device=x.device)
    _L.check(_L.load().fo1_swin_window_partition_bf16(x.data_ptr(), xw.data_ptr(), H, W, C, ws, shift, batch, _stream()), "fo1_swin_window_partition_bf16")
    return xw


def swin_window_reverse_add(yw: torch.Tensor, shortcut: torch.Tensor, H: int, W: int, ws: int, shift: int, batch: int = 1) -> torch.Tensor:
    _chk(yw, "yw"); _chk(shortcut, "shortcut")
    assert yw.is_contiguous() and shortcut.is_contiguous() and shortcut.shape[0] == batch * H * W
    y = torch.empty_like(shortcut)
    _L.check(_L.load().fo1_swin_window_reverse_add_bf16(yw.data_ptr(), shortcut.data_ptr(), y.data_ptr(), H, W, shortcut.shape[1], ws, shift, batch, _stream()),
             "fo1_swin_window_reverse_add_bf16")
    return y


def patch_merge(x: torch.Tensor, H: int, W: int, batch: int = 1) -> torch.Tensor:
    _chk(x, "x")
    assert x.is_contiguous() and x.shape[0] == batch * H * W
    C = x.shape[1]
    out = torch.empty(batch * ((H + 1) // 2) * ((W + 1) // 2), 4 * C, dtype=torch.bfloat16, device=x.device)
    _L.check(_L.load().fo1_patch_merge_bf16(x.data_ptr(), out.data_ptr(), H, W, C, batch, _stream()), "fo1_patch_merge_bf16")
    return out


def groupnorm_tokens(x: torch.Tensor, groups: int, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    _chk(x, "x"); _chk(weight, "weight"); _chk(bias, "bias")
    px, ldx, S, C = _rows(x, "x")
    y = torch.empty(S, C, dtype=torch.bfloat16, device=x.device)
    ws = _workspace("groupnorm", x.device, _L.load().fo1_groupnorm_tokens_workspace_bytes(S, groups))
    _L.check(_L.load().fo1_groupnorm_tokens_bf16(px, ldx, S, C, groups, weight.data_ptr(), bias.data_ptr(), float(eps), y.data_ptr(), y.stride(0), ws.data_ptr(),
                                                 ws.numel(), _stream()), "fo1_groupnorm_tokens_bf16")
    return y
