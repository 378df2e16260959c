"""Qwen2.5-VL language-model half of the hot path on the MI355X engine.

Host code only orchestrates: every tensor op is a libfo1hip.so kernel (vlm_fo1_amd/ops.py).  Index
bookkeeping the reference does with device syncs (`get_rope_index`, sentinel search,
modeling_qwen2_5_vl.py:1546-1701, omchat_qwen2_5_vl.py:318-319) is done on the host from the
sentinel positions and the image grid before any launch.

Weights: fused at load time — q/k/v -> one [2560, 2048] GEMM, gate/up -> one [22016, 2048] GEMM
(rows interleaved [gate 16 | up 16 | ...] so SwiGLU runs in the GEMM epilogue) — checkpoint key names as in the reference state dict.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .guide import TokenGuide

IMAGE_TOKEN_INDEX = -200
DEFAULT_REGION_INDEX = -300


@dataclass
class LLMConfig:
    hidden_size: int = 2048
    num_layers: int = 36
    num_heads: int = 16
    num_kv_heads: int = 2
    head_dim: int = 128
    intermediate_size: int = 11008
    vocab_size: int = 151936
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1e6
    mrope_section: Tuple[int, int, int] = (16, 24, 24)
    max_seq: int = 8192


_ROPE_INDEX_CACHE: Dict[tuple, tuple] = {}


def rope_index_host(n_before: int, grid_hw_merged: Tuple[int, int], n_after: int):
    """[3, L] int64 position ids for <text><image gh x gw><text> and the rope delta
    (reference get_rope_index :1630-1697, single image, t = 1).  Memoised: a pure function of the prompt structure."""
    key = (int(n_before), int(grid_hw_merged[0]), int(grid_hw_merged[1]), int(n_after))
    hit = _ROPE_INDEX_CACHE.get(key)
    if hit is None:
        if len(_ROPE_INDEX_CACHE) >= 1024:
            _ROPE_INDEX_CACHE.pop(next(iter(_ROPE_INDEX_CACHE)))
        hit = _ROPE_INDEX_CACHE[key] = _rope_index_host(n_before, grid_hw_merged, n_after)
    return hit


def _rope_index_host(n_before: int, grid_hw_merged: Tuple[int, int], n_after: int):
    gh, gw = grid_hw_merged
    pre = torch.arange(n_before).view(1, -1).expand(3, -1)
    t_idx = torch.zeros(gh * gw, dtype=torch.long)
    h_idx = torch.arange(gh).view(-1, 1).expand(-1, gw).flatten()
    w_idx = torch.arange(gw).view(1, -1).expand(gh, -1).flatten()
    img = torch.stack([t_idx, h_idx, w_idx]) + n_before
    nxt = int(img.max()) + 1 if gh * gw > 0 else n_before
    post = torch.arange(n_after).view(1, -1).expand(3, -1) + nxt
    pos = torch.cat([pre, img, post], dim=1)
    return pos, int(pos.max()) + 1 - pos.shape[1]


_MROPE_CACHE: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def mrope_tables(pos: torch.Tensor, head_dim: int, theta: float, sections: Sequence[int]):
    """pos [3, L] (host) -> cos, sin [L, head_dim] bf16 (host): fp32 tables, section select, cast
    (reference :609-624, :675-681).  Memoised on the position ids: they depend only on the prompt structure (tokens before the
    image, merged grid, tokens after), which repeats from request to request, and the dozen small torch CPU ops below cost
    ~10 ms per call on a many-core host (intra-op thread-pool wake-ups) — more than half a GPU pass."""
    key = (pos.shape[1], head_dim, float(theta), tuple(sections), pos.numpy().tobytes())
    hit = _MROPE_CACHE.get(key)
    if hit is not None:
        return hit
    out = _mrope_tables(pos, head_dim, theta, sections)
    if len(_MROPE_CACHE) >= 256:
        _MROPE_CACHE.pop(next(iter(_MROPE_CACHE)))
    _MROPE_CACHE[key] = out
    return out


def _mrope_tables(pos: torch.Tensor, head_dim: int, theta: float, sections: Sequence[int]):
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    fr = pos.float()[:, :, None] * inv[None, None, :]
    emb = torch.cat([fr, fr], dim=-1)
    cos, sin = emb.cos(), emb.sin()
    sec = list(sections) * 2
    cs = torch.cat([m[i % 3] for i, m in enumerate(cos.split(sec, dim=-1))], dim=-1)
    sn = torch.cat([m[i % 3] for i, m in enumerate(sin.split(sec, dim=-1))], dim=-1)
    return cs.to(torch.bfloat16).contiguous(), sn.to(torch.bfloat16).contiguous()


def packed_item_rows(seqs, n_heads: int, head_dim: int, n_kv_heads: int):
    """HOST: the attention work list of a packed pass (plan_batch's `seqs`) -> (rows [[q0, q1, k0, k1]], second key range per row, query block,
    causal key-query pairs).  One segment per sequence and one per distinct shared prefix, split into query blocks, ordered for the launch."""
    segs = []                                  # (q0, q1, second range) — one per sequence, one per distinct shared prefix
    done = set()
    fl = 0.0
    for sq in seqs:
        o, _, Lp, *pre = sq
        if pre:
            po, P = pre
            if (po, P) not in done:
                done.add((po, P))
                segs.append((po, po + P, (0, 0)))
                fl += P * (P + 1) / 2.0
            segs.append((o, o + Lp, (po, po + P)))
            fl += Lp * (Lp + 1) / 2.0 + float(Lp) * P
        else:
            segs.append((o, o + Lp, (0, 0)))
            fl += Lp * (Lp + 1) / 2.0
    blk = ops.pick_q_block([(a, b) for a, b, _ in segs], n_heads, head_dim, n_kv_heads)
    rows = [[q0, min(q0 + blk, b), a, b] for a, b, _ in segs for q0 in range(a, b, blk)]
    rng = [list(r2) for a, b, r2 in segs for _ in range(a, b, blk)]
    order = ops.order_items(rows, blk, True, prefix=rng)           # 32x32 form: longest-processing-time-first over the launch
    return [rows[i] for i in order], [rng[i] for i in order], blk, fl


def last_rows_of(seqs) -> List[int]:
    """HOST: the packed row of every sequence's last real token (plan_batch's `last` plan names the same rows)."""
    return [sq[0] + sq[1] - (sq[4] if len(sq) > 3 else 0) - 1 for sq in seqs]


def tail_item_rows(rows, rng, needed: Sequence[int]):
    """HOST: the entries of a work list whose query block [q0, q1) holds a needed row, UNCHANGED (same block, same key range, same second
    range) and in the list's order: each needed row walks the tiles it walks in the full launch, so its attention output has the same bits.
    What the last decoder layer runs when only `needed` rows are read after it.  -> (rows, second ranges, causal key-query pairs kept)."""
    keep = [i for i, (q0, q1, _, _) in enumerate(rows) if any(q0 <= r < q1 for r in needed)]
    fl = sum((rows[i][1] - rows[i][0]) * ((rows[i][0] + rows[i][1] + 1) / 2.0 - rows[i][2] + max(0, rng[i][1] - rng[i][0])) for i in keep)
    return [rows[i] for i in keep], [rng[i] for i in keep], fl


class QwenLLM:
    def __init__(self, cfg: LLMConfig, state: Dict[str, torch.Tensor], device, lm_head: Optional[torch.Tensor] = None):
        self.cfg = cfg
        self.dev = torch.device(device)
        bf = torch.bfloat16

        def dv(t):
            return t.to(device=self.dev, dtype=bf).contiguous()

        self.embed = dv(state["embed_tokens.weight"])
        self.lm_head = dv(lm_head) if lm_head is not None else self.embed  # tied embeddings
        self.norm = dv(state["norm.weight"])
        self.layers = []
        for i in range(cfg.num_layers):
            p = f"layers.{i}."
            a = p + "self_attn."
            self.layers.append(dict(
                ln1=dv(state[p + "input_layernorm.weight"]),
                ln2=dv(state[p + "post_attention_layernorm.weight"]),
                wqkv=dv(torch.cat([state[a + "q_proj.weight"], state[a + "k_proj.weight"], state[a + "v_proj.weight"]], 0)),
                bqkv=dv(torch.cat([state[a + "q_proj.bias"], state[a + "k_proj.bias"], state[a + "v_proj.bias"]], 0)),
                wo=dv(state[a + "o_proj.weight"]),
                wgu=dv(ops.interleave_gate_up(state[p + "mlp.gate_proj.weight"], state[p + "mlp.up_proj.weight"])),
                wdown=dv(state[p + "mlp.down_proj.weight"]),
            ))
        c = cfg
        # KV cache: K [layer][kv_head][pos][head_dim]; V^T [layer][kv_head*head_dim][pos] (zeroed: the
        # attention kernel may read up to 3 finite columns past kv_end)
        self.capacity = c.max_seq
        self.cache_epoch = 0        # bumped whenever the caches are re-allocated: captured graphs hold the old pointers
        self.kcache = torch.zeros(c.num_layers, c.num_kv_heads, c.max_seq, c.head_dim, dtype=bf, device=self.dev)
        self.vtcache = torch.zeros(c.num_layers, c.num_kv_heads * c.head_dim, c.max_seq, dtype=bf, device=self.dev)
        self.kv_len = 0
        self.rope_delta = 0
        self._item_cache: Dict[Tuple[int, int], torch.Tensor] = {}
        # ---- decode-step graph state (fo1_decode_advance, include/fo1.h) ----
        # text positions have t = h = w, so one [max_seq, head_dim] table indexed by (cache position + rope delta)
        # covers every decode step; it is built on the host with the prefill's exact code path
        p = torch.arange(c.max_seq).view(1, -1).expand(3, -1)
        cos_t, sin_t = mrope_tables(p, c.head_dim, c.rope_theta, c.mrope_section)
        self.rope_cos, self.rope_sin = cos_t.to(self.dev), sin_t.to(self.dev)
        self.dstate = torch.zeros(8, dtype=torch.int32, device=self.dev)       # [pos, rope_row, -, -, item(4)]
        self.dplan = torch.zeros(1, 2, dtype=torch.int32, device=self.dev)     # gather plan of the one new token: (0, token id)
        self._dgraph = {}           # head (sampled?) -> (hipGraph, logits); emptied whenever the caches or the rope tables move
        self._dstate_keep = None
        self._sampled = False       # sampled head of the single-sequence step (set_sampling)
        self._sbuf = None
        self.rope_epoch = 0         # bumped whenever the rope tables are re-allocated (grow_rope): step graphs key on it
        self._rope_retired = []     # replaced tables, never freed (shared by the replicas: see grow_rope)
        self._ws_owner = ops.new_owner(self)   # scratch-buffer key (ops.workspace_scope); FO1Engine overrides it with its own token

    def reserve(self, n_positions: int) -> bool:
        """Make room for n_positions cache rows (prompt + the tokens a request may generate; a packed batch needs the sum).
        Grows geometrically and keeps the cached prefix; returns True when the caches moved (graphs that captured the old
        pointers — this object's decode graph, the engine's prefill graphs — are dropped by the epoch bump).  The reference's
        HF cache grows without bound (max_position_embeddings 32768+), so a long generation must not fail on a fixed size."""
        if n_positions <= self.capacity:
            return False
        c = self.cfg
        cap = self.capacity
        while cap < n_positions:
            cap *= 2
        bf = torch.bfloat16
        k = torch.zeros(c.num_layers, c.num_kv_heads, cap, c.head_dim, dtype=bf, device=self.dev)
        v = torch.zeros(c.num_layers, c.num_kv_heads * c.head_dim, cap, dtype=bf, device=self.dev)
        k[:, :, :self.capacity] = self.kcache
        v[:, :, :self.capacity] = self.vtcache
        self.kcache, self.vtcache, self.capacity = k, v, cap
        # (the text-position rope table is NOT grown here: the prefill does not read it — packed passes bring their own tables — and a
        # worker thread's reserve() must not re-allocate a table that the decode pool's graphs, replaying on another stream, still read
        # (ADVICE r4).  The decode paths grow it when THEY need the rows: _check_room, BatchDecoder._ensure, DecodePool.)
        self._dgraph = {}
        self._item_cache = {}
        self.cache_epoch += 1
        torch.cuda.current_stream().synchronize()
        return True

    def grow_rope(self, rows: int) -> None:
        """Text-position rope table (t = h = w) with at least `rows` rows.  Re-allocating it invalidates every captured graph that read
        the old table: the single-sequence decode graph is dropped here, callers drop their own (BatchDecoder._ensure)."""
        c = self.cfg
        if self.rope_cos.shape[0] >= rows:
            return
        p = torch.arange(rows).view(1, -1).expand(3, -1)
        cos_t, sin_t = mrope_tables(p, c.head_dim, c.rope_theta, c.mrope_section)
        # the old tables stay allocated for the life of the process (0.5 KB per row, geometric growth: at most twice the final size):
        # a step graph captured on another engine replica / the decode pool may still be replaying with their pointers on its own
        # stream, and nothing here can wait for it (the epoch / data_ptr graph keys only protect the NEXT capture)
        self._rope_retired.append((self.rope_cos, self.rope_sin))
        self.rope_cos, self.rope_sin = cos_t.to(self.dev), sin_t.to(self.dev)
        self._dgraph = {}
        self.rope_epoch += 1

    def replica(self) -> "QwenLLM":
        """Same weights and rope tables (shared, read-only), private per-request state: KV cache, decode state, decode graph.
        For several requests in flight on different streams (FO1Engine.replica)."""
        import copy
        r = copy.copy(self)
        c = self.cfg
        r.kcache = torch.zeros_like(self.kcache)
        r.vtcache = torch.zeros_like(self.vtcache)
        r.kv_len = 0
        r.rope_delta = 0
        r.dstate = torch.zeros_like(self.dstate)
        r.dplan = torch.zeros_like(self.dplan)
        r._dgraph = {}
        r._dstate_keep = None
        r._sampled, r._sbuf = False, None
        r._item_cache = {}
        r._ws_owner = ops.new_owner(r)
        # the zero-fills above ran on the creating thread's current stream; the replica is used from another thread / stream
        torch.cuda.current_stream().synchronize()
        return r

    # ---- splice ------------------------------------------------------------------------------
    def plan_inputs(self, input_ids: Sequence[int], n_img: int, n_regions: int, grid_hw_merged: Tuple[int, int]):
        """HOST part of the splice: sentinel ids -> (gather plan int32 [L',2] (cpu), pos [3,L'] (cpu), rope delta).
        One image per prompt (what prepare_inputs produces).  Vectorised: at > 100 images/s per GPU a Python loop over the ~650 rows of
        every prompt (3-4 ms each) is most of a worker thread's time under the GIL (profiles/r04_driver_level_host_profile_first.log)."""
        import numpy as np
        ids = np.asarray(input_ids, dtype=np.int64).reshape(-1)
        img_at = np.flatnonzero(ids == IMAGE_TOKEN_INDEX)
        if img_at.size > 1:
            raise ValueError("more than one <image> sentinel in the prompt")
        if img_at.size == 0:
            raise ValueError("prompt has no <image> sentinel")
        is_reg = ids == DEFAULT_REGION_INDEX
        if int(is_reg.sum()) > n_regions:
            # same failure the reference raises at omchat_qwen2_5_vl.py:361
            raise IndexError("prompt has more <regionfeat> placeholders than region features")
        text = ~is_reg
        text[img_at[0]] = False
        bad = ids[text]
        if bad.size and (int(bad.min()) < 0 or int(bad.max()) >= self.cfg.vocab_size):   # torch's embedding lookup raises the same way in the reference
            t = int(bad[(bad < 0) | (bad >= self.cfg.vocab_size)][0])
            raise IndexError(f"token id {t} is outside the embedding table (vocab_size {self.cfg.vocab_size})")
        if grid_hw_merged[0] * grid_hw_merged[1] != n_img:
            # reference modeling_qwen2_5_vl.py:1797-1800
            raise ValueError(f"Image features and image tokens do not match: tokens: {grid_hw_merged[0] * grid_hw_merged[1]}, features {n_img}")
        n_before = int(img_at[0])
        kind = np.where(is_reg, 2, 0).astype(np.int32)
        val = np.where(is_reg, np.cumsum(is_reg) - 1, ids).astype(np.int32)
        plan = np.empty((ids.size - 1 + n_img, 2), dtype=np.int32)
        plan[:n_before, 0], plan[:n_before, 1] = kind[:n_before], val[:n_before]
        plan[n_before:n_before + n_img, 0] = 1
        plan[n_before:n_before + n_img, 1] = np.arange(n_img, dtype=np.int32)
        plan[n_before + n_img:, 0], plan[n_before + n_img:, 1] = kind[n_before + 1:], val[n_before + 1:]
        n_after = plan.shape[0] - n_before - n_img
        pos, delta = rope_index_host(n_before, grid_hw_merged, n_after)
        return torch.from_numpy(plan), pos, delta

    def decode_weight_tensors(self):
        """The tensors one decode step streams once (projection weights + biases, norms, lm_head): the algorithmic bytes of the step's
        HBM roofline (bench.py `decode.roofline`)."""
        out = [self.lm_head, self.norm]
        for w in self.layers:
            out += [w["wqkv"], w["bqkv"], w["wo"], w["wgu"], w["wdown"], w["ln1"], w["ln2"]]
        return out

    def embed_rows(self, plan_dev: torch.Tensor, image_tokens: torch.Tensor, region_tokens: Optional[torch.Tensor]):
        """DEVICE part of the splice: one row gather over (embed table | image tokens | region tokens)."""
        return ops.gather_rows(plan_dev, self.cfg.hidden_size, self.embed, image_tokens, region_tokens)

    def build_inputs(self, input_ids: Sequence[int], image_tokens: torch.Tensor, region_tokens: Optional[torch.Tensor],
                     grid_hw_merged: Tuple[int, int]):
        """Sentinel ids -> (embeds [L', d] on device, pos [3, L'] host, rope delta)."""
        n_reg = 0 if region_tokens is None else region_tokens.shape[0]
        plan, pos, delta = self.plan_inputs(input_ids, image_tokens.shape[0], n_reg, grid_hw_merged)
        return self.embed_rows(plan.to(self.dev), image_tokens, region_tokens), pos, delta

    # ---- transformer -------------------------------------------------------------------------
    def _forward(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos0: int, collect: Optional[list] = None,
                 items: Optional[torch.Tensor] = None, flops: Optional[float] = None, prefix_ranges: Optional[torch.Tensor] = None,
                 tail: Optional[tuple] = None):
        """-> the residual stream after the last layer [L, d]; or, with `tail` = (gather plan int32 [B, 2] of the rows read after the last layer,
        reduced work items, their flop count, their second ranges), the head's (last hidden [B, d], logits [B, V], next ids [B]): the last layer
        then writes K / V^T of every row as always, attends over the reduced list only and leaves o-projection, MLP and head of the B rows to the
        native tail (fo1_llm_prefill_tail) — no other row of that layer is read by anyone.  `collect` keeps the all-row path."""
        c = self.cfg
        L = x.shape[0]
        H, KV, HD = c.num_heads, c.num_kv_heads, c.head_dim
        kv_end = pos0 + L
        if kv_end > self.capacity:
            raise ValueError(f"sequence {kv_end} exceeds the KV cache ({self.capacity}); call reserve() first")
        if items is None:
            items = self._items(pos0, kv_end)
        scale = 1.0 / math.sqrt(HD)
        if flops is None:
            flops = 4.0 * H * HD * (L * (pos0 + (L + 1) / 2.0))
        # (the C entry's own preconditions, mirrored — csrc/stages.hip takes the two-launch path on the same terms: N a multiple of the 256-column
        # tile, 16-byte aligned rope tables)
        fused = (HD == 128 and pos0 % 8 == 0 and self.capacity % 8 == 0 and ((H + 2 * KV) * HD) % 256 == 0
                 and cos.data_ptr() % 16 == 0 and sin.data_ptr() % 16 == 0 and cos.is_contiguous() and sin.is_contiguous()
                 and ops.qkv_fused_for(L, (H + 2 * KV) * HD, c.hidden_size) and not ops.fp8_routed(self.layers[0]["wqkv"], L))
        if collect is not None:
            tail = None
        for li, w in enumerate(self.layers):
            if tail is not None and li + 1 == len(self.layers):
                last_plan, items, flops, prefix_ranges = tail
            if fused:
                # q/k/v projection with mRoPE + K append + V^T in the GEMM's epilogue (ops.qkv_proj_rope mode 0): same bits, one launch less and no
                # second pass over the [L, 2560] activation
                qkv = ops.qkv_proj_rope(ops.rmsnorm(x, w["ln1"], c.rms_norm_eps), w["wqkv"], w["bqkv"], 0, H, KV, cos, sin, self.kcache[li], pos0, self.vtcache[li])
            else:
                qkv = ops.norm_linear(x, w["ln1"], c.rms_norm_eps, w["wqkv"], w["bqkv"])
                ops.qkv_post_llm(qkv, H, KV, HD, cos, sin, self.kcache[li], self.vtcache[li], pos0)   # mRoPE + K append + V^T, one launch
            att = ops.attention_strided(qkv[:, :H * HD], q_row0=pos0, k=self.kcache[li], vt=self.vtcache[li], items=items,
                                        n_q_heads=H, n_kv_heads=KV, head_dim=HD, scale=scale, causal=True, flops=flops, prefix_ranges=prefix_ranges)
            if tail is not None and li + 1 == len(self.layers):
                from . import stage_abi
                return stage_abi.llm_stage(self).prefill_tail(x, att, last_plan)
            x = ops.gemm(att, w["wo"], residual=x)
            a = ops.norm_linear(x, w["ln2"], c.rms_norm_eps, w["wgu"], act=ops.ACT_SWIGLU16)   # gate/up GEMM, SwiGLU in its epilogue
            x = ops.gemm(a, w["wdown"], residual=x)
            if collect is not None:
                collect.append(x)
        return x

    def _item_rows(self, pos0: int, kv_end: int):
        """HOST: work list of one sequence's rows [pos0, kv_end) against keys [0, kv_end) -> (rows, query block)."""
        blk = ops.pick_q_block([(pos0, kv_end)], self.cfg.num_heads, self.cfg.head_dim, self.cfg.num_kv_heads)
        rows = [[q0, min(q0 + blk, kv_end), 0, kv_end] for q0 in range(pos0, kv_end, blk)]
        return [rows[i] for i in ops.order_items(rows, blk, True)], blk      # 32x32 form: the blocks with the most key tiles first

    def _items(self, pos0: int, kv_end: int) -> torch.Tensor:
        key = (pos0, kv_end)
        it = self._item_cache.get(key)
        if it is None:
            # never evict: a captured prefill graph may hold this tensor's pointer (entries are a few hundred bytes each)
            rows, blk = self._item_rows(pos0, kv_end)
            it = torch.tensor(rows, dtype=torch.int32).to(self.dev)
            it.q_block = blk
            self._item_cache[key] = it
        return it

    def _tail(self, pos0: int, kv_end: int):
        """The `tail` of _forward for one sequence at rows [pos0, kv_end): its last row, and the one query block of _items that holds it."""
        key = ("tail", pos0, kv_end)
        hit = self._item_cache.get(key)
        if hit is None:
            rows, blk = self._item_rows(pos0, kv_end)
            rows, _, fl = tail_item_rows(rows, [[0, 0]] * len(rows), [kv_end - 1])
            it = torch.tensor(rows, dtype=torch.int32).to(self.dev)
            it.q_block = blk
            plan = torch.tensor([[0, kv_end - 1 - pos0]], dtype=torch.int32).to(self.dev)
            hit = self._item_cache[key] = (plan, it, 4.0 * self.cfg.num_heads * self.cfg.head_dim * fl, None)
        return hit

    def prefill(self, embeds: torch.Tensor, pos: torch.Tensor, rope_delta: int = 0, collect: Optional[list] = None,
                tables: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """embeds [L, d] bf16 device, pos [3, L] host -> (final-norm last hidden [1, d], logits [1, V], next id tensor).
        `tables` = device (cos, sin) [L, head_dim] bf16 when the caller already uploaded them (graph replay)."""
        c = self.cfg
        self.reserve(embeds.shape[0])
        if tables is None:
            cos, sin = mrope_tables(pos, c.head_dim, c.rope_theta, c.mrope_section)
            cos, sin = cos.to(self.dev), sin.to(self.dev)
        else:
            cos, sin = tables
        with ops.workspace_scope(self._ws_owner):
            out = self._forward(embeds, cos, sin, 0, collect, tail=self._tail(0, embeds.shape[0]))
            self.kv_len = embeds.shape[0]
            self.rope_delta = rope_delta
            return self._head(out) if collect is not None else out

    # ---- several prompts packed into one pass (the reference's batch-aware splice, omchat_qwen2_5_vl.py:380-416) ----
    PACK_ALIGN = 4   # the attention kernel reads V^T in 8-byte (4-key) pieces: every sequence starts at a multiple of 4

    SHARE_MIN_ROWS = 256     # a common prefix shorter than this is not worth a second key range per attention item

    def plan_batch(self, prompts: Sequence[Sequence[int]], n_img: Sequence[int], n_regions: Sequence[int],
                   grids_merged: Sequence[Tuple[int, int]], img_base: Optional[Sequence[int]] = None, share_prefix: bool = False):
        """HOST: B prompts -> one packed plan.  Sequence b owns rows [off_b, off_b + Lp_b), Lp_b = its row count rounded up to PACK_ALIGN
        with dummy rows (token 0) appended AFTER its real rows: causal attention keeps them invisible to every real row.  Image /
        region indices address the batch-concatenated token tables.  Returns dict(plan int32 [R,2], cos, sin bf16 [R, hd] (host),
        seqs, pos [per-sequence [3, L]], delta [per sequence], last int32 [B,2] gather plan of the last real rows).

        seqs[b] = (off, L, Lp) — or, with share_prefix, (off, L, Lp, poff, P) for prompts over ONE image (same img_base) whose first P
        rows are identical (system text + the image block, up to the first region): those P rows (a multiple of PACK_ALIGN, at
        [poff, poff + P)) run through every layer ONCE, `off` / `Lp` describe the prompt's remaining L - P rows, which attend
        [prefix | own rows] (fo1_attention_prefix_bf16).  In a causal model the prefix rows' states do not depend on what follows, so
        every prompt's rows are what its own full pass computes (the reference would run the whole model once per prompt)."""
        c = self.cfg
        A = self.PACK_ALIGN
        B = len(prompts)
        per = []
        img0 = reg0 = 0
        for b, (ids, ni, nr, gm) in enumerate(zip(prompts, n_img, n_regions, grids_merged)):
            if img_base is not None:      # several prompts over ONE image: they all address that image's rows of the token table
                img0 = int(img_base[b])
            pl, pos, delta = self.plan_inputs(ids, ni, nr, gm)
            pl = pl.clone()
            pl[:, 1] += (pl[:, 0] == 1).to(torch.int32) * img0 + (pl[:, 0] == 2).to(torch.int32) * reg0
            per.append((pl, pos, delta))
            img0 += ni; reg0 += nr
        # prompts that share a prefix: same image rows AND the same plan rows up to the first difference
        shared = {}                       # first member -> (P, members)
        member_of = [None] * B
        if share_prefix and img_base is not None:
            by_img = {}
            for b in range(B):
                by_img.setdefault(int(img_base[b]), []).append(b)
            for members in by_img.values():
                if len(members) < 2:
                    continue
                p0 = per[members[0]][0]
                P = p0.shape[0]
                for m in members[1:]:
                    pm = per[m][0]
                    n = min(P, pm.shape[0])
                    diff = (p0[:n] != pm[:n]).any(dim=1).nonzero()
                    P = int(diff[0]) if diff.numel() else n
                P = min(P, min(per[m][0].shape[0] for m in members) - 1) // A * A      # every prompt keeps >= 1 own row (its last row feeds the head)
                if P >= self.SHARE_MIN_ROWS:
                    shared[members[0]] = (P, members)
                    for m in members:
                        member_of[m] = members[0]
        plans, coss, sins, seqs, poss, deltas, last_rows = [], [], [], [None] * B, [], [], []
        prefix_at = {}
        off = 0
        for b in range(B):
            pl, pos, delta = per[b]
            L = pl.shape[0]
            P = shared[member_of[b]][0] if member_of[b] is not None else 0
            own = L - P
            Lp = (own + A - 1) // A * A
            if Lp > own:
                pl = torch.cat([pl, torch.zeros(Lp - own, 2, dtype=torch.int32)], 0)
                tail = int(pos.max()) + 1 + torch.arange(Lp - own).view(1, -1).expand(3, -1)
                pos_p = torch.cat([pos, tail], 1)
            else:
                pos_p = pos
            cs, sn = mrope_tables(pos_p, c.head_dim, c.rope_theta, c.mrope_section)
            if P and member_of[b] == b:   # the group's first prompt: its prefix rows are the group's
                plans.append(pl[:P]); coss.append(cs[:P]); sins.append(sn[:P])
                prefix_at[b] = off
                off += P
            plans.append(pl[P:]); coss.append(cs[P:]); sins.append(sn[P:])
            seqs[b] = (off, L, Lp) if not P else (off, L, Lp, prefix_at[member_of[b]], P)
            last_rows.append(off + own - 1)
            poss.append(pos); deltas.append(delta)
            off += Lp
        last = torch.tensor([[0, r] for r in last_rows], dtype=torch.int32).reshape(-1, 2)
        return dict(plan=torch.cat(plans, 0).contiguous(), cos=torch.cat(coss, 0).contiguous(), sin=torch.cat(sins, 0).contiguous(),
                    seqs=seqs, pos=poss, delta=deltas, last=last, rows=off)

    def packed_items(self, seqs):
        """-> (attention work items int32 [n, 4] on the device, flop count, prefix ranges int32 [n, 2] or None)."""
        key = ("packed", tuple(seqs))
        hit = self._item_cache.get(key)
        if hit is None:
            c = self.cfg
            rows, rng, blk, fl = packed_item_rows(seqs, c.num_heads, c.head_dim, c.num_kv_heads)
            it = torch.tensor(rows, dtype=torch.int32).to(self.dev)
            it.q_block = blk
            r2 = torch.tensor(rng, dtype=torch.int32).to(self.dev) if any(x[1] > x[0] for x in rng) else None
            hit = (it, 4.0 * c.num_heads * c.head_dim * fl, r2)
            self._item_cache[key] = hit
        return hit

    def packed_tail_items(self, seqs):
        """packed_items for the LAST layer of a pass whose head reads each sequence's last real row only: the entries of the full list that
        hold such a row (tail_item_rows) -> (items, flop count, prefix ranges — given exactly when the full list has them: the same kernel
        entry runs).  Kept like the full list: a captured graph holds the pointers."""
        key = ("packed_tail", tuple(seqs))
        hit = self._item_cache.get(key)
        if hit is None:
            c = self.cfg
            rows, rng, blk, _ = packed_item_rows(seqs, c.num_heads, c.head_dim, c.num_kv_heads)
            shared = any(x[1] > x[0] for x in rng)
            rows, rng, fl = tail_item_rows(rows, rng, last_rows_of(seqs))
            it = torch.tensor(rows, dtype=torch.int32).to(self.dev)
            it.q_block = blk
            r2 = torch.tensor(rng, dtype=torch.int32).to(self.dev) if shared else None
            hit = (it, 4.0 * c.num_heads * c.head_dim * fl, r2)
            self._item_cache[key] = hit
        return hit

    def prefill_packed(self, embeds: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, seqs, last_plan: torch.Tensor,
                       collect: Optional[list] = None):
        """DEVICE: embeds [R, d] (packed rows of plan_batch), cos/sin [R, hd] device tables, last_plan int32 [B,2] (device).
        K / V^T land at cache positions = packed row indices.  Returns (final-norm last hidden [B, d], logits [B, V], next ids
        int32 [B]).  last_plan names each sequence's last real row (plan_batch's `last`): the last layer computes nothing else past its
        K / V^T entries unless `collect` asks for every row."""
        c = self.cfg
        items, flops, prefix_ranges = self.packed_items(seqs)
        from . import stage_abi
        if stage_abi.enabled() and collect is None and prefix_ranges is None:      # the same launches, sequenced by fo1_llm_prefill (csrc/stages.hip)
            if embeds.shape[0] > self.capacity:
                raise ValueError(f"sequence {embeds.shape[0]} exceeds the KV cache ({self.capacity}); call reserve() first")
            with ops.workspace_scope(self._ws_owner):
                return stage_abi.llm_stage(self).prefill_packed(embeds, cos, sin, seqs, last_plan)
        with ops.workspace_scope(self._ws_owner):
            if collect is None:
                return self._forward(embeds, cos, sin, 0, items=items, flops=flops, prefix_ranges=prefix_ranges,
                                     tail=(last_plan,) + self.packed_tail_items(seqs))
            x = self._forward(embeds, cos, sin, 0, collect, items=items, flops=flops, prefix_ranges=prefix_ranges)
            last = ops.rmsnorm(ops.gather_rows(last_plan, c.hidden_size, x), self.norm, c.rms_norm_eps)
            logits = ops.gemm(last, self.lm_head)
            return last, logits, ops.argmax_rows(logits)

    def _check_room(self):
        """The device-side decode state indexes the caches blindly: grow them on the host before a step would run past them."""
        if self.kv_len + 1 > self.capacity:
            self.reserve(self.kv_len + 1)
            self.sync_decode_state()
        if self.rope_cos.shape[0] < self.capacity:      # the step reads table row (position + rope delta) < capacity
            self.grow_rope(self.capacity)

    def sync_decode_state(self):
        """Publish (kv_len, rope row, first decode work item) to the device-side decode state."""
        n = self.kv_len
        st = torch.tensor([n, n + self.rope_delta, 0, 0, n, n + 1, 0, n + 1], dtype=torch.int32)
        self.dstate.copy_(st, non_blocking=True)
        self._dstate_keep = st      # keep the source alive until the next upload replaces it

    def _head(self, x: torch.Tensor):
        c = self.cfg
        last = ops.rmsnorm(x[-1:], self.norm, c.rms_norm_eps)
        logits = ops.gemm(last, self.lm_head)  # last row only: output-identical to the reference's all-row lm_head
        tok = ops.argmax(logits[0])
        return last, logits, tok

    def _decode_device(self):
        """One decode step whose every position-dependent quantity is read from device memory (self.dstate /
        self.dplan): capturable once, replayable for every token."""
        with ops.workspace_scope(self._ws_owner):
            return self._decode_device_impl()

    def _decode_device_impl(self):
        c = self.cfg
        H, KV, HD = c.num_heads, c.num_kv_heads, c.head_dim
        x = ops.gather_rows(self.dplan, c.hidden_size, self.embed)
        scale = 1.0 / math.sqrt(HD)
        pos_ptr = self.dstate[0:1]
        items = self.dstate[4:8].view(1, 4)
        for li, w in enumerate(self.layers):
            # 7 launches per layer: norms folded into the GEMV prologues, rope + K/V^T cache append in one kernel
            qkv = ops.gemv(x, w["wqkv"], w["bqkv"], norm_weight=w["ln1"], norm_eps=c.rms_norm_eps)
            ops.decode_qkv_post(qkv, H, KV, HD, self.rope_cos, self.rope_sin, self.dstate, self.kcache[li], self.vtcache[li])
            # split-KV decode attention: chunk count follows the device-side kv length (= dstate[7] = position + 1)
            att = ops.attention_decode(qkv[:, :H * HD], self.kcache[li], self.vtcache[li], self.dstate[7:8], self.capacity, H, KV, HD, scale)
            x = ops.gemv(att, w["wo"], residual=x)
            a = ops.gemv(x, w["wgu"], act=ops.ACT_SWIGLU16, norm_weight=w["ln2"], norm_eps=c.rms_norm_eps)
            x = ops.gemv(a, w["wdown"], residual=x)
        logits = ops.gemv(x, self.lm_head, norm_weight=self.norm, norm_eps=c.rms_norm_eps)
        if self._sampled:
            # sampled head: the draw's counter is the sampler's own device word (sstate[4], one more per step), the id lands in the plan
            sb = self._sbuf
            ops.decode_sample_accept(logits, sb["params"], sb["state"], self.dplan, sb["ids"], None, sb["done"])
        else:
            ops.argmax(logits[0], out=self.dplan.view(-1)[1:2])    # next token id lands in the gather plan of the next step
        ops.decode_advance(self.dstate)
        return logits

    SAMPLE_IDS = 1 << 16      # tokens one sampled single-sequence generation may draw (the sampler's bookkeeping records them)

    def set_sampling(self, sampling: Optional[dict], stream: int = 0, counter: int = 1) -> None:
        """Head of decode_step / decode_step_graph: None = greedy; dict(temperature, top_p, top_k, seed) = the device sampler
        (fo1_decode_sample_accept at B = 1) drawing Philox(counter, stream; seed), the counter starting at `counter` (the first token of a
        request is drawn from the prefill's logits with counter 0) and advancing on the device with every step."""
        if sampling is None:
            self._sampled = False
            return
        if self._sbuf is None:
            with torch.inference_mode(False):      # persistent, updated in place (see BatchDecoder.__init__)
                z = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=self.dev)      # noqa: E731
                self._sbuf = dict(params=z(1, 8), state=z(1, 8), ids=z(1, self.SAMPLE_IDS), done=z(1))
        params = ops.sample_params([(sampling["temperature"], sampling["top_p"], sampling["top_k"], sampling["seed"], stream)])
        state = torch.tensor([[0, 0, 0, 0, int(counter), 1 << 30, 0, 0]], dtype=torch.int32)
        self._sbuf["params"].copy_(params, non_blocking=True)
        self._sbuf["state"].copy_(state, non_blocking=True)
        self._sbuf["keep"] = (params, state)
        self._sample_left = self.SAMPLE_IDS - 1 - int(counter)
        self._sampled = True

    def _sample_room(self):
        if self._sampled:
            if self._sample_left <= 0:
                raise ValueError(f"a sampled generation draws at most {self.SAMPLE_IDS - 1} tokens")
            self._sample_left -= 1

    def decode_step_graph(self, token_id: Optional[torch.Tensor] = None):
        """Greedy step via one replayed hipGraph.  `token_id` (device int32 [1]) seeds the plan on the first step
        after a prefill; later steps reuse the id the previous replay wrote.  Returns (logits, next id tensor)."""
        self._check_room()
        self._sample_room()
        if token_id is not None:
            self.dplan.view(-1)[1:2].copy_(token_id.to(torch.int32).view(1), non_blocking=True)
        if self._sampled not in self._dgraph:      # one graph per head (greedy / sampled); the sampling values are data
            sb = [self._sbuf[k] for k in ("state", "ids", "done")] if self._sampled else []
            self._dgraph[self._sampled] = ops.capture_graph(self._decode_device, rollback=(self.dstate, self.dplan, *sb))
        g, logits = self._dgraph[self._sampled]
        ops.replay_graph(g)
        self.kv_len += 1
        return logits, self.dplan.view(-1)[1:2]

    def decode_step(self, token_id: torch.Tensor):
        """One greedy step with individually launched kernels (same device code as the graph path, so the two are
        bit-identical): token_id int32 [1] on device -> (last hidden placeholder, logits [1, V], next id tensor).
        Position = cache_position + rope_delta on all three axes (reference :1848-1860)."""
        self._check_room()
        self._sample_room()
        self.dplan.view(-1)[1:2].copy_(token_id.to(torch.int32).view(1), non_blocking=True)
        self.sync_decode_state()
        logits = self._decode_device()
        self.kv_len += 1
        return None, logits, self.dplan.view(-1)[1:2].clone()


def reloc_rows(seqs, dst0s):
    """kv_relocate entries [src0, dst0, len, 0] that move every sequence of a packed prefill to cache row dst0: one entry, or two for a
    sequence whose first P rows are a prefix shared with other prompts (plan_batch(share_prefix=True): (off, L, Lp, poff, P))."""
    rows = []
    for sq, d in zip(seqs, dst0s):
        o, L, _, *pre = sq
        if pre:
            po, P = pre
            rows += [[po, d, P, 0], [o, d + P, L - P, 0]]
        else:
            rows.append([o, d, L, 0])
    return rows


# ---- host bookkeeping of the decode classes (BatchDecoder, DecodePool).  No silent truncation: the HF-like contract is
# "exactly these stop ids, exactly this budget" ----
def stop_id_list(stop_ids, max_stop: int, who: str, hint: str = "") -> List[int]:
    """The sorted distinct stop ids; more than the device-side rule compares against is an error."""
    ids = sorted(set(int(t) for t in stop_ids))
    if len(ids) > max_stop:
        raise ValueError(f"{who} evaluates at most {max_stop} stop ids on the device (got {len(ids)}){hint}")
    return ids


def token_budget(max_new_tokens, cap: int, who: str, hint: str = "") -> int:
    """max_new_tokens as the device counts it (at least the first token); more than the ids buffer keeps is an error."""
    max_new = max(1, int(max_new_tokens))
    if max_new > cap:
        raise ValueError(f"{who} keeps at most {cap} generated ids per sequence (max_new_tokens={max_new}){hint}")
    return max_new


def live_state_rows(bases, seqs, deltas, max_new: int, set_row: int = 0):
    """Device state rows [next cache row, next rope row, first cache row, finished, generated, budget, stop set, 0] of sequences
    (off, L, ...) that were just relocated to cache rows `bases`."""
    return [[b + L, L + d, b, 0, 0, max_new, set_row, 0] for b, (_, L, *_), d in zip(bases, seqs, deltas)]


def empty_state_rows(bases):
    """State rows of empty slots = "finished": a step skips their attention and ignores their ids, and the K / V^T rows it still
    appends for them land inside their own slot (at `base`)."""
    return [[b, 0, b, 1, 0, 0, 0, 0] for b in bases]


def sampling_table(sampling, B: int):
    """The `sampling` argument of BatchDecoder.start / DecodePool.join -> (rows, kinds): the 7-field rows of ops.sample_params, one per
    sequence, and per sequence "plain" (None: greedy, no penalty), "sampled" (a draw, no penalty) or "general" (greedy flag or a penalty).
    sampling: None; one dict for the submission (temperature, top_p, top_k, seed — optional when greedy=True — plus greedy,
    repetition_penalty; sequence b draws on stream streams[b], or stream + b, default b); or a list with one such dict (its own `stream`,
    default b) or None per sequence.  A dict with a token-rule key (RULE_KEYS: ban, ban_first, allow, ban_until — token_rule) is "general"
    too: dict(greedy=True, ban=[...]) is a constrained greedy sequence; so is a dict with a guide (guide=TokenGuide: sampling_guides)."""
    per = _per_sequence(sampling, B)
    rows = [ops.sampling_row(sp, b) for b, sp in enumerate(per)]
    kinds = ["plain" if sp is None else ("general" if (r[5] or ops.penalty_on(r[6]) or has_rule(sp) or has_guide(sp) or has_steer(sp)) else "sampled")
             for sp, r in zip(per, rows)]
    return rows, kinds


def _per_sequence(sampling, B: int) -> list:
    """sampling_table's argument -> one dict or None per sequence."""
    if sampling is None:
        per = [None] * B
    elif isinstance(sampling, dict):
        streams = list(sampling.get("streams") or [int(sampling.get("stream", 0)) + b for b in range(B)])
        if len(streams) != B:
            raise ValueError(f"sampling: {len(streams)} streams for {B} sequences")
        per = [dict(sampling, stream=st) for st in streams]
    else:
        per = list(sampling)
        if len(per) != B:
            raise ValueError(f"sampling: {len(per)} entries for {B} sequences")
    return per


RULE_KEYS = ("ban", "ban_first", "allow", "ban_until")      # the token-rule keys of a sequence's sampling dict (token_rule)


def has_rule(sp: Optional[dict]) -> bool:
    return sp is not None and any(sp.get(k) is not None for k in RULE_KEYS)


def has_guide(sp: Optional[dict]) -> bool:
    return sp is not None and sp.get("guide") is not None


STEER_KEYS = ("bias", "frequency_penalty", "presence_penalty")      # the soft-steering keys of a sequence's sampling dict (token_steer)


def _penalty_value(v, what: str) -> float:
    """A frequency / presence penalty as the fp32 value the device reads: None = 0 = off; ValueError for a bool, a non-number or a value that
    is not finite as fp32."""
    if v is None:
        return 0.0
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: a finite number (got {v!r})")
    with np.errstate(over="ignore"):
        f = float(np.float32(v))
    if not math.isfinite(f):
        raise ValueError(f"{what}: a finite fp32 number (got {v!r})")
    return f


def has_steer(sp: Optional[dict]) -> bool:
    """Does the dict ask for a bias or a count penalty?  An empty or all-zero bias and penalties of 0 / None are "off": such a dict is planned
    exactly as one without the keys."""
    if sp is None:
        return False
    b = sp.get("bias")
    if b is not None and not hasattr(b, "items"):
        return True      # (token_steer raises on it)
    if b and any(isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != 0 for v in b.values()):
        return True
    return any(sp.get(k) is not None and (isinstance(sp.get(k), bool) or sp.get(k) != 0) for k in STEER_KEYS[1:])


class TokenSteer(NamedTuple):
    """A sequence's normalised steer (include/fo1.h, fo1_token_steer_t): `bias` is its row of the bias table — ops.count_words(V) bf16 bit
    patterns as bytes, each value rounded once to bf16, zero elsewhere — or None; f and q are the frequency and presence penalties as fp32."""
    bias: Optional[bytes]
    f: float
    q: float

    @property
    def counting(self) -> bool:
        return ops.count_penalty_on(self.f, self.q)


def bf16_bits(x) -> np.ndarray:
    """float32 values -> bf16 bit patterns, round to nearest even (NaN stays NaN)."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    return np.where(np.isnan(x), 0x7fc0, r).astype(np.uint16)


def token_steer(spec: Optional[dict], V: int) -> Optional[TokenSteer]:
    """The soft-steering keys of a sequence's sampling dict -> its TokenSteer, or None for a dict without one (has_steer):
      bias={id: value}        added to the token's logit before the repetition penalty: x = bf16(fp32(l) + fp32(bf16(value)));
      frequency_penalty=f     f times the number of times the sequence has generated the token is subtracted, after the penalty;
      presence_penalty=q      q is subtracted once the sequence has generated the token at all.
    ValueError: an id that is not an integer or lies outside [0, V), a value that is not a number or not finite once rounded to bf16 (to
    forbid a token use `ban`, to force one `allow`), a penalty that is a bool or not finite as fp32."""
    if not has_steer(spec):
        return None
    V = int(V)
    b = spec.get("bias")
    row = None
    if b is not None:
        if not hasattr(b, "items"):
            raise ValueError(f"bias: a dict {{token id: value}} (got {type(b).__name__})")
        ids = _token_ids(list(b.keys()), V, "bias")
        vals = []
        for t, v in zip(ids, b.values()):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"bias: the value of token {t} is a number (got {v!r})")
            with np.errstate(over="ignore"):
                vals.append(np.float32(v))
        bits = bf16_bits(np.array(vals, dtype=np.float32))
        bad = [t for t, h in zip(ids, bits) if (int(h) & 0x7f80) == 0x7f80]
        if bad:
            raise ValueError(f"bias: the value of token {bad[0]} is not finite as bf16 ({b[list(b.keys())[ids.index(bad[0])]]!r}); "
                             f"to forbid a token use `ban`, to force a set of tokens `allow`")
        if any(int(h) & 0x7fff for h in bits):
            full = np.zeros(ops.count_words(V), dtype=np.uint16)
            full[ids] = bits
            row = full.tobytes()
    f = _penalty_value(spec.get("frequency_penalty"), "frequency_penalty")
    q = _penalty_value(spec.get("presence_penalty"), "presence_penalty")
    if row is None and not ops.count_penalty_on(f, q):
        return None
    return TokenSteer(row, f, q)


def sampling_steers(sampling, B: int, V: int) -> List[Optional[TokenSteer]]:
    """sampling_table's argument -> the TokenSteer (or None) of every sequence."""
    return [token_steer(sp, V) for sp in _per_sequence(sampling, B)]


class BiasTable:
    """Device side of the logit biases of a decoder's rows: the bias table bf16 [rows, count_words(V)], its gate bitmap int32 [rows,
    seen_words(V)] (a set bit = a non-zero entry) and a host map from a bias row's bytes to its table row with a user count.  Equal biases
    share a row; a row with users is never rewritten (a captured step reads the table, it never writes it).  Allocated by the first biased
    sequence, as the mask table is by the first constrained one.  dev=None keeps the bookkeeping alone (no tables)."""

    def __init__(self, rows: int, n_vocab: int, dev):
        self.rows, self.V = rows, int(n_vocab)
        self.table = self.gate = None
        if dev is not None:
            with torch.inference_mode(False):
                self.table = torch.zeros(rows, ops.count_words(n_vocab), dtype=torch.bfloat16, device=dev)
                self.gate = torch.zeros(rows, ops.seen_words(n_vocab), dtype=torch.int32, device=dev)
        self._row: Dict[bytes, int] = {}
        self.users = [0] * rows
        self._keep: list = []

    def room(self, biases: Sequence[bytes]) -> bool:
        """Is there a row for every one of these bias rows (its own, or one without users)?"""
        new = {m for m in biases if m not in self._row}
        taken = {self._row[m] for m in biases if m in self._row}
        return len(new) <= sum(1 for r in range(self.rows) if self.users[r] == 0 and r not in taken)

    def gate_of(self, bias: bytes) -> np.ndarray:
        """The gate bitmap of a bias row: uint32 [seen_words(V)], bit i set iff entry i is not zero (-0 counts as zero)."""
        nz = (np.frombuffer(bias, dtype=np.uint16)[:self.V] & 0x7fff) != 0
        out = np.zeros(ops.seen_words(self.V) * 4, dtype=np.uint8)
        pk = np.packbits(nz, bitorder="little")
        out[:pk.size] = pk
        return out.view(np.uint32)

    def acquire(self, bias: bytes) -> int:
        """The row holding `bias`, one user more; a new bias is uploaded (current stream) into a row without users."""
        if len(bias) != ops.count_words(self.V) * 2:
            raise ValueError(f"BiasTable: a bias row has {ops.count_words(self.V) * 2} bytes (got {len(bias)})")
        row = self._row.get(bias)
        if row is None:
            held = set(self._row.values())
            free = [r for r in range(self.rows) if self.users[r] == 0 and r not in held] or [r for r in range(self.rows) if self.users[r] == 0]
            if not free:
                raise RuntimeError(f"BiasTable: {self.rows} different logit-bias vectors are live; wait for sequences to finish")
            row = free[0]
            for k in [k for k, v in self._row.items() if v == row]:
                del self._row[k]
            if self.table is not None:
                host = torch.frombuffer(bytearray(bias), dtype=torch.int16).view(1, -1)
                gate = torch.from_numpy(self.gate_of(bias).view(np.int32).copy()).view(1, -1)
                self.table.view(torch.int16)[row:row + 1].copy_(host, non_blocking=True)
                self.gate[row:row + 1].copy_(gate, non_blocking=True)
                self._keep += [host, gate]
                if len(self._keep) > 4 * self.rows:
                    del self._keep[:len(self._keep) - 4 * self.rows]
            self._row[bias] = row
        self.users[row] += 1
        return row

    def release(self, row: int) -> None:
        if row >= 0:
            assert self.users[row] > 0
            self.users[row] -= 1


def new_counts(rows: int, n_vocab: int, dev):
    """(counts int16 [rows, count_words(V)] holding the uint16 counts, count_gate int32 [rows, seen_words(V)]), zeroed."""
    with torch.inference_mode(False):
        return (torch.zeros(rows, ops.count_words(n_vocab), dtype=torch.int16, device=dev),
                torch.zeros(rows, ops.seen_words(n_vocab), dtype=torch.int32, device=dev))


class TokenRule(NamedTuple):
    """A sequence's normalised token rule (include/fo1.h, fo1_token_rule_t): up to three banned sets as bitmaps in the seen bitmap's layout
    (bytes of ops.seen_words(V) words; None = empty) — `always` at every pick, `early` while fewer than `until` tokens have been generated,
    `first` at the first token."""
    always: Optional[bytes]
    early: Optional[bytes]
    until: int
    first: Optional[bytes]

    def bitmaps(self) -> list:
        return [m for m in (self.always, self.early, self.first) if m is not None]


def _token_ids(ids, V: int, what: str) -> List[int]:
    if isinstance(ids, (str, bytes)) or not hasattr(ids, "__iter__"):
        raise ValueError(f"{what}: a list of token ids (got {ids!r})")
    out = []
    for t in ids:
        if isinstance(t, (bool, float)) or not hasattr(t, "__index__"):
            raise ValueError(f"{what}: token ids are integers (got {t!r})")
        t = int(t)
        if not 0 <= t < V:
            raise ValueError(f"{what}: token id {t} outside [0, {V})")
        out.append(t)
    return out


def token_rule(spec: Optional[dict], V: int, eos_ids: Sequence[int] = ()) -> Optional[TokenRule]:
    """The token-rule keys of a sequence's sampling dict -> its TokenRule, or None for a dict without one:
      ban=ids           never picked;
      allow=ids         only these may be picked: everything else is banned, unioned with `ban`;
      ban_first=ids     not picked as the first generated token;
      ban_until=(n, ids)  not picked among the first n generated tokens (HF's min_new_tokens with ids = the EOS ids; a bare n takes eos_ids).
    ValueError: an id that is not an integer or lies outside [0, V), an empty allow, n < 0, or a phase of the sequence (first token, tokens
    before n, tokens from n on) whose union bans all V tokens."""
    if not has_rule(spec):
        return None
    V = int(V)

    def bits(ids):
        m = np.zeros(V, dtype=bool)
        m[ids] = True
        return m

    always = bits(_token_ids(spec.get("ban") or (), V, "ban"))
    if spec.get("allow") is not None:
        allow = _token_ids(spec["allow"], V, "allow")
        if not allow:
            raise ValueError("allow: an empty allow-list leaves no token to pick")
        always |= ~bits(allow)
    first = bits(_token_ids(spec.get("ban_first") or (), V, "ban_first"))
    early, until = np.zeros(V, dtype=bool), 0
    if spec.get("ban_until") is not None:
        bu = spec["ban_until"]
        n, ids = (bu, eos_ids) if not hasattr(bu, "__len__") else (bu if len(bu) == 2 else (None, None))
        if isinstance(n, (bool, float)) or not hasattr(n, "__index__"):
            raise ValueError(f"ban_until: (n, ids) with an integer n (got {bu!r})")
        if int(n) < 0:
            raise ValueError(f"ban_until: n = {int(n)} < 0")
        until = int(n)
        if until > 0:
            early = bits(_token_ids(ids, V, "ban_until"))
    for what, m in (("at every token", always), ("before ban_until's n tokens", always | early), ("at the first token", always | early | first)):
        if m.all():
            raise ValueError(f"token rule: every one of the {V} tokens is banned {what}")

    def pack(m):
        if not m.any():
            return None
        out = np.zeros(ops.seen_words(V) * 4, dtype=np.uint8)
        pk = np.packbits(m, bitorder="little")
        out[:pk.size] = pk
        return out.tobytes()

    e = pack(early)
    return TokenRule(pack(always), e, until if e is not None else 0, pack(first))


def sampling_rules(sampling, B: int, V: int, eos_ids: Sequence[int] = ()) -> List[Optional[TokenRule]]:
    """sampling_table's argument -> the TokenRule (or None) of every sequence."""
    return [token_rule(sp, V, eos_ids) for sp in _per_sequence(sampling, B)]


class TokenMasks:
    """Device side of the token rules of a decoder's rows: the mask table int32 [rows, seen_words(V)] (a set bit = token banned) and a host map
    from a bitmap's bytes to its row with a user count.  Equal sets share a row; a row with users is never rewritten (a captured step reads
    the table, it never writes it).  Allocated by the first constrained sequence, as the seen bitmap is by the first penalised one."""

    def __init__(self, rows: int, n_vocab: int, dev):
        with torch.inference_mode(False):
            self.table = torch.zeros(rows, ops.seen_words(n_vocab), dtype=torch.int32, device=dev)
        self.rows = rows
        self._row: Dict[bytes, int] = {}
        self.users = [0] * rows
        self._keep: list = []

    def room(self, bitmaps: Sequence[bytes]) -> bool:
        """Is there a row for every one of these bitmaps (its own, or one without users)?"""
        new = {m for m in bitmaps if m not in self._row}
        taken = {self._row[m] for m in bitmaps if m in self._row}
        return len(new) <= sum(1 for r in range(self.rows) if self.users[r] == 0 and r not in taken)

    def acquire(self, bitmap: bytes) -> int:
        """The row holding `bitmap`, one user more; a new bitmap is uploaded (current stream) into a row without users."""
        if len(bitmap) != self.table.shape[1] * 4:
            raise ValueError(f"TokenMasks: a bitmap has {self.table.shape[1] * 4} bytes (got {len(bitmap)})")
        row = self._row.get(bitmap)
        if row is None:
            held = set(self._row.values())
            free = [r for r in range(self.rows) if self.users[r] == 0 and r not in held] or [r for r in range(self.rows) if self.users[r] == 0]
            if not free:
                raise RuntimeError(f"TokenMasks: {self.rows} different token masks are live; wait for sequences to finish")
            row = free[0]
            for k in [k for k, v in self._row.items() if v == row]:
                del self._row[k]
            host = torch.frombuffer(bytearray(bitmap), dtype=torch.int32).view(1, -1)
            self.table[row:row + 1].copy_(host, non_blocking=True)
            self._keep.append(host)
            if len(self._keep) > 2 * self.rows:
                del self._keep[:len(self._keep) - 2 * self.rows]
            self._row[bitmap] = row
        self.users[row] += 1
        return row

    def release(self, row: int) -> None:
        if row >= 0:
            assert self.users[row] > 0
            self.users[row] -= 1

    def rule_row(self, rule: TokenRule):
        """Acquires the rows of a sequence's rule -> (its fo1_token_rule_t row, the rows to release when it leaves)."""
        a, e, f = (-1 if m is None else self.acquire(m) for m in (rule.always, rule.early, rule.first))
        return (a, e, rule.until, f), [r for r in (a, e, f) if r >= 0]


class GuidePlan(NamedTuple):
    """What a guided sequence asks of the tables: its guide, the always-bans of its token rule (folded into every state's bitmap: the head
    reads the state's mask row in always_row's place), the resulting bitmap of every state (None = nothing banned), the state its first token
    is picked in, and — when the caller picked the first token on the device — the device int32 word holding the state after it.
    A guide with accepting states adds its closing rule (guide.closing_bitmaps): depth = D > 0 and closing = the S * D bitmaps of (state s,
    r < D tokens left), entry s * D + r.  A (state, tokens left) pair no checked sequence can be in — more than r + 1 tokens from an accepting
    state, every token banned — holds the state's plain bitmap instead, so it costs no mask row of its own."""
    guide: TokenGuide
    always: Optional[bytes]
    bitmaps: tuple
    s0: int
    after_first: Optional[torch.Tensor]
    depth: int = 0
    closing: Optional[tuple] = None

    @property
    def key(self):
        return (self.guide, self.always)


def guide_plan(g: TokenGuide, always: Optional[bytes], s0: int, after_first=None) -> GuidePlan:
    """The GuidePlan of a sequence with guide g and always-bans `always` that picks its first token in state s0."""
    plain = tuple(g.state_bitmaps(always))
    D, rows = g.closing_bitmaps(always)
    if rows is None:
        return GuidePlan(g, always, plain, s0, after_first)
    dist = g.distances(always)
    closing = tuple(plain[s] if dist[s] > r + 1 else rows[s][r] for s in range(g.S) for r in range(D))
    return GuidePlan(g, always, plain, s0, after_first, D, closing)


def sampling_guides(sampling, B: int, V: int, trules: Sequence[Optional[TokenRule]], prompt_ids=None,
                    budget: Optional[int] = None) -> List[Optional[GuidePlan]]:
    """sampling_table's argument -> the GuidePlan (or None) of every sequence; trules: sampling_rules' result for the same argument.
    A sequence's `guide` key holds a TokenGuide over V tokens; a guide built by ban_sequences starts in guide.run(prompt ids), so it needs
    prompt_ids.  The optional key `guide_state` holds a device int32 tensor of one element, the state after the first token, when the caller
    picked that token with the guided head (FO1Engine._first_tokens).  ValueError: not a TokenGuide, another vocabulary size, or a state the
    sequence can reach in which the guide and its token rule together leave nothing to pick (a guide whose only exit is a stop id that
    ban_until still bans is one such case).
    budget: the sequences' effective token budget N (max_new_tokens, capped by the ids the decoder keeps).  A guide with accepting states
    closes under it (guide.closing_bitmaps); a start state more than N tokens from an accepting one, or a pick at which the guide, its
    closing rule and the token rule leave nothing, is a ValueError.  Without a budget such a guide is a ValueError too."""
    out = []
    for b, sp in enumerate(_per_sequence(sampling, B)):
        if not has_guide(sp):
            out.append(None)
            continue
        g = sp["guide"]
        if not isinstance(g, TokenGuide):
            raise ValueError(f"guide: a vlm_fo1_amd.guide.TokenGuide (got {type(g).__name__})")
        if g.V != int(V):
            raise ValueError(f"guide: built for {g.V} tokens, the model has {int(V)}")
        if g.from_prompt:
            if prompt_ids is None or len(prompt_ids) != B:
                raise ValueError("guide: a guide that starts in the prompt's state needs prompt_ids, one list per sequence")
            s0 = g.run(prompt_ids[b])
        else:
            s0 = g.start
        t = trules[b]
        always = t.always if t is not None else None
        if g.accept is not None and budget is None:
            raise ValueError("guide: a guide with accepting states needs the sequence's token budget")
        if t is None:
            g.check_pickable(s0, budget=budget)
        else:
            g.check_pickable(s0, t.always, t.early, t.until, t.first, budget=budget)
        out.append(guide_plan(g, always, s0, sp.get("guide_state")))
    return out


def unguided_rules(trules: Sequence[Optional[TokenRule]], gplans: Sequence[Optional[GuidePlan]]) -> List[Optional[TokenRule]]:
    """The rules whose mask rows the sequences take themselves: a guided sequence's always-bans live in its guide's state bitmaps."""
    out = []
    for t, g in zip(trules, gplans):
        if t is not None and g is not None:
            t = t._replace(always=None)
            if not t.bitmaps():
                t = None
        out.append(t)
    return out


class _Spans:
    """First-fit spans of a flat table, keyed by content, with user counts: equal contents share a span, a span with users is never rewritten
    or moved, one without users stays findable until its place is taken."""

    def __init__(self, cap: int):
        self.cap = cap
        self.ent: Dict[object, list] = {}      # key -> [offset, length, users]

    def _place(self, n: int, busy: list) -> int:
        at = 0
        for o, l in sorted(busy):
            if o - at >= n:
                return at
            at = max(at, o + l)
        return at if self.cap - at >= n else -1

    def room(self, needs: Sequence[tuple]) -> bool:
        """Is there a span for every (key, length) of `needs` (its own, or a place no live span covers)?"""
        busy = [(o, l) for o, l, u in self.ent.values() if u > 0]
        for key, n in dict(needs).items():
            if key in self.ent:
                if self.ent[key][2] == 0:
                    busy.append(tuple(self.ent[key][:2]))
                continue
            at = self._place(n, busy)
            if at < 0:
                return False
            busy.append((at, n))
        return True

    def acquire(self, key, n: int):
        """-> (offset, new): the span holding `key`, one user more; new = the caller has to write its n entries."""
        e = self.ent.get(key)
        if e is not None:
            e[2] += 1
            return e[0], False
        at = self._place(n, [(o, l) for o, l, u in self.ent.values() if u > 0])
        if at < 0:
            raise RuntimeError("no room in a token-guide table; wait for sequences to finish")
        for k in [k for k, (o, l, u) in self.ent.items() if o < at + n and at < o + l]:      # (spans without users whose place is taken)
            del self.ent[k]
        self.ent[key] = [at, n, 1]
        return at, True

    def release(self, key, drop: bool = False) -> None:
        e = self.ent[key]
        assert e[2] > 0
        e[2] -= 1
        if drop and e[2] == 0:
            del self.ent[key]


class GuideTables:
    """Device side of the token guides of a decoder's rows (include/fo1.h, fo1_token_guide_t): the class table cls int16 [CLS_ROWS, V] (the
    uint16 classes), the transition table next int32 [N_NEXT] and the state-row table state_row int32 [N_STATE_ROW], which names the mask row
    (of the decoder's TokenMasks) holding each state's banned set.  Content-keyed sharing with user counts: equal class maps share a row, equal
    transition tables a span, equal (guide, always-bans) pairs everything — region_answer guides for different n_regions share their class
    row — and states with equal banned sets share mask rows within and across guides, since the bitmaps are acquired through TokenMasks.
    A row or span with users is never rewritten.  The step reads all three and writes none.  Allocated by the first guided sequence.
    A fourth table, close_row int32 [N_CLOSE_ROW], names the mask row of every (state, tokens left) of a plan with a closing rule (S * D
    entries, include/fo1.h fo1_guide_close_t); a (guide, always-bans) pair shares its span, and its bitmaps go through TokenMasks too."""
    CLS_ROWS = 64
    N_NEXT = 1 << 14
    N_STATE_ROW = 1 << 10
    N_CLOSE_ROW = 1 << 12

    def __init__(self, n_vocab: int, dev, masks: Optional[TokenMasks]):
        """dev = None: the bookkeeping alone, without device tables — what room() and new_bitmaps() answer from before anything is allocated."""
        self.masks = masks
        self.cls = self.next = self.state_row = self.close_row = None
        if dev is not None:
            with torch.inference_mode(False):
                self.cls = torch.zeros(self.CLS_ROWS, int(n_vocab), dtype=torch.int16, device=dev)
                self.next = torch.full((self.N_NEXT,), -1, dtype=torch.int32, device=dev)
                self.state_row = torch.full((self.N_STATE_ROW,), -1, dtype=torch.int32, device=dev)
                self.close_row = torch.full((self.N_CLOSE_ROW,), -1, dtype=torch.int32, device=dev)
        self._cls, self._next, self._sr = _Spans(self.CLS_ROWS), _Spans(self.N_NEXT), _Spans(self.N_STATE_ROW)
        self._cr = _Spans(self.N_CLOSE_ROW)
        self.live: Dict[tuple, dict] = {}      # GuidePlan.key -> dict(users, row = the fo1_token_guide_t fields, mask_rows)
        self._keep: list = []

    @staticmethod
    def _keys(plan: GuidePlan):
        g = plan.guide
        return g.cls.tobytes(), (g.C, g.next.tobytes()), plan.key

    def new_bitmaps(self, plans: Sequence[Optional[GuidePlan]]) -> list:
        """The state bitmaps the plans would acquire mask rows for (those of pairs that are not live yet)."""
        return [m for p in {q.key: q for q in plans if q is not None}.values() if p.key not in self.live
                for m in p.bitmaps + (p.closing or ()) if m is not None]

    def room(self, plans: Sequence[Optional[GuidePlan]]) -> bool:
        """Is there a class row, a transition span, a state-row span and (for a closing rule) a close-row span for every plan?  (The mask
        rows: TokenMasks.room over new_bitmaps.)"""
        new = [p for p in {q.key: q for q in plans if q is not None}.values() if p.key not in self.live]
        ks = [self._keys(p) for p in new]
        return (self._cls.room([(k[0], 1) for k in ks]) and self._next.room([(k[1], p.guide.S * p.guide.C) for k, p in zip(ks, new)])
                and self._sr.room([(k[2], p.guide.S) for k, p in zip(ks, new)])
                and self._cr.room([(k[2], p.guide.S * p.depth) for k, p in zip(ks, new) if p.depth > 0]))

    def _upload(self, dst: torch.Tensor, host: torch.Tensor) -> None:
        dst.copy_(host, non_blocking=True)
        self._keep.append(host)
        if len(self._keep) > 256:
            del self._keep[:len(self._keep) - 256]

    def acquire(self, plan: GuidePlan) -> tuple:
        """One user more of the plan's tables -> its fo1_token_guide_t fields (cls_row, n_classes, next_off, row_off); a new (guide,
        always-bans) pair uploads what is not there yet (current stream) and takes a mask row per distinct state bitmap."""
        e = self.live.get(plan.key)
        if e is None:
            g = plan.guide
            kc, kn, ks = self._keys(plan)
            got = []
            try:
                crow, new = self._cls.acquire(kc, 1)
                got.append((self._cls, kc))
                if new:
                    self._upload(self.cls[crow], torch.from_numpy(g.cls.view(np.int16).copy()))
                noff, new = self._next.acquire(kn, g.S * g.C)
                got.append((self._next, kn))
                if new:
                    self._upload(self.next[noff:noff + g.S * g.C], torch.from_numpy(g.next.reshape(-1).copy()))
                roff, _ = self._sr.acquire(ks, g.S)
                got.append((self._sr, ks))
                coff = 0
                if plan.depth > 0:
                    coff, _ = self._cr.acquire(ks, g.S * plan.depth)
                    got.append((self._cr, ks))
                rows = []
                try:
                    for m in plan.bitmaps + (plan.closing or ()):
                        rows.append(-1 if m is None else self.masks.acquire(m))
                except BaseException:
                    for r in rows:
                        self.masks.release(r)
                    raise
            except BaseException:
                for sp, k in got:
                    sp.release(k, drop=sp is self._sr or sp is self._cr)
                raise
            self._upload(self.state_row[roff:roff + g.S], torch.tensor(rows[:g.S], dtype=torch.int32))
            if plan.depth > 0:
                self._upload(self.close_row[coff:coff + g.S * plan.depth], torch.tensor(rows[g.S:], dtype=torch.int32))
            e = self.live[plan.key] = dict(users=0, row=(crow, g.C, noff, roff), mask_rows=rows, keys=(kc, kn, ks),
                                           close=(coff, plan.depth) if plan.depth > 0 else None)
        e["users"] += 1
        return e["row"]

    def release(self, key) -> None:
        e = self.live[key]
        assert e["users"] > 0
        e["users"] -= 1
        if e["users"] == 0:      # its mask rows may be rewritten from here on: the state-row span goes with them, class row and transitions stay findable
            for r in e["mask_rows"]:
                self.masks.release(r)
            kc, kn, ks = e["keys"]
            self._cls.release(kc)
            self._next.release(kn)
            self._sr.release(ks, drop=True)
            if e["close"] is not None:
                self._cr.release(ks, drop=True)
            del self.live[key]

    def users(self) -> int:
        return sum(e["users"] for e in self.live.values())

    def close_of(self, key) -> Optional[tuple]:
        """(close_off, depth) of a live plan: its fo1_guide_close_t fields; None without a closing rule."""
        return self.live[key]["close"]

    def operands(self, guides: torch.Tensor, gstate: torch.Tensor, closes: Optional[torch.Tensor] = None,
                 budget: Optional[torch.Tensor] = None) -> "ops.GuideOperands":
        """closes (ops.guide_closes): the closing form, with the rows' budgets in the rows form."""
        if closes is None:
            return ops.GuideOperands(self.cls, self.next, self.state_row, guides, gstate)
        return ops.GuideOperands(self.cls, self.next, self.state_row, guides, gstate, self.close_row, closes, budget)

    def pointers(self) -> tuple:
        return self.cls.data_ptr(), self.next.data_ptr(), self.state_row.data_ptr()


class PassTables:
    """The mask and guide rows one launch over a pass's rows needs, held together until the launch is enqueued (FO1Engine._first_tokens'
    scratch tables): the rules' rows stay held while the guides acquire theirs — a released row may be rewritten by the next new bitmap, and
    the rule table handed to the kernel would still name it.  rules / guides: the rows of ops.token_rules / ops.token_guides (guides: None
    when no sequence has a guide).  release() gives everything back; an acquire that fails part-way gives back what it took and raises."""

    def __init__(self, masks: "TokenMasks", gtab, trules: Sequence[Optional[TokenRule]], gplans: Sequence[Optional[GuidePlan]] = ()):
        self.masks, self.gtab = masks, gtab
        self._rows: List[int] = []
        self._keys: list = []
        self.rules, self.guides, self.closes = [], None, None      # closes: the rows of ops.guide_closes, None when no guide closes
        try:
            for t in trules:
                row, held = (None, []) if t is None else masks.rule_row(t)
                self.rules.append(row)
                self._rows += held
            if any(g is not None for g in gplans):
                if not gtab.room(gplans):
                    raise RuntimeError("the token guides of one pass do not fit the guide tables")
                if not masks.room(gtab.new_bitmaps(gplans)):
                    raise RuntimeError("the state bitmaps of one pass's token guides do not fit the mask table")
                self.guides = []
                for g in gplans:
                    self.guides.append(None if g is None else gtab.acquire(g))
                    if g is not None:
                        self._keys.append(g.key)
                if any(g is not None and g.depth > 0 for g in gplans):
                    self.closes = [None if g is None else gtab.close_of(g.key) for g in gplans]
        except BaseException:
            self.release()
            raise

    def release(self) -> None:
        for k in self._keys:
            self.gtab.release(k)
        for r in self._rows:
            self.masks.release(r)
        self._keys, self._rows = [], []


def guide_states_host(gplans: Sequence[Optional[GuidePlan]], first_tokens: torch.Tensor) -> List[int]:
    """The state after the first token of every guided sequence whose plan brings no device word for it (one host read of the first tokens)."""
    need = [k for k, p in enumerate(gplans) if p is not None and p.after_first is None]
    if not need:
        return [0] * len(gplans)
    first = first_tokens.to(torch.int32).cpu().tolist()
    return [p.guide.advance(p.s0, first[k]) if k in need else 0 for k, p in enumerate(gplans)]


def new_seen(rows: int, n_vocab: int, dev) -> torch.Tensor:
    """A cleared seen bitmap int32 [rows, ld_words] (csrc/sample.hip: bit t & 31 of word t >> 5 of row b = token t occurs in sequence b)."""
    with torch.inference_mode(False):
        return torch.zeros(rows, ops.seen_words(n_vocab), dtype=torch.int32, device=dev)


class LogprobRecord(NamedTuple):
    """What a request with `logprobs=n` gets back per sequence (host tensors; `new` = generated tokens, the first included): the
    log-probability of each generated token under the model's own distribution (the log-softmax of the raw logits) and
    the n most likely tokens of each step with theirs, descending, (id = -1, -inf) where a step had fewer than n finite logits."""
    logprob: torch.Tensor          # float32 [new]
    top_ids: torch.Tensor          # int32 [new, n]
    top_logprobs: torch.Tensor     # float32 [new, n]


def logprob_wants(logprobs, B: int) -> List[int]:
    """The `logprobs` argument of BatchDecoder.start / DecodePool.join -> per sequence -1 (off) or its top-n (0 .. ops.LOGPROB_TOP_MAX).
    logprobs: None; one int for every sequence; or a list with None or an int per sequence."""
    per = [logprobs] * B if logprobs is None or isinstance(logprobs, int) else list(logprobs)
    if len(per) != B:
        raise ValueError(f"logprobs: {len(per)} entries for {B} sequences")
    out = []
    for w in per:
        if w is None:
            out.append(-1)
            continue
        if isinstance(w, bool) or int(w) != w or not 0 <= int(w) <= ops.LOGPROB_TOP_MAX:
            raise ValueError(f"logprobs: top-n must be an integer in 0..{ops.LOGPROB_TOP_MAX} or None (got {w!r})")
        out.append(int(w))
    return out


class LogprobBuffers:
    """Device side of the log-probability records of a decoder's rows: lp [rows, cap], top_ids / top_lp [rows, cap, LOGPROB_TOP_MAX], the
    per-row request `want` (-1 = off) and the per-row count of recorded tokens `n_rec` (fo1_decode_logprob_record).  Allocated by the first
    requesting sequence, as the seen bitmap is by the first penalised one."""

    def __init__(self, rows: int, cap: int, dev):
        T = ops.LOGPROB_TOP_MAX
        with torch.inference_mode(False):
            self.lp = torch.zeros(rows, cap, dtype=torch.float32, device=dev)
            self.top_ids = torch.zeros(rows, cap, T, dtype=torch.int32, device=dev)
            self.top_lp = torch.zeros(rows, cap, T, dtype=torch.float32, device=dev)
            self.want = torch.full((rows,), -1, dtype=torch.int32, device=dev)
            self.n_rec = torch.zeros(rows, dtype=torch.int32, device=dev)

    def written(self):
        """What a step writes: part of a capture's rollback tuple."""
        return self.lp, self.top_ids, self.top_lp, self.n_rec

    def set_rows(self, rows: Sequence[int], wants: Sequence[int], first, src: Sequence[int]) -> list:
        """Rows `rows` get the requests `wants`; a requesting row's column 0 is the first token's record — row src[k] of first = (lp [B],
        top_ids [B, n], top_lp [B, n]), the rows form's output on the prefill's logits — and its n_rec = 1.  -> the uploads' host tensors."""
        dev = self.lp.device
        r = torch.tensor(list(rows), dtype=torch.int64)
        w = torch.tensor(list(wants), dtype=torch.int32)
        rd = r.to(dev, non_blocking=True)
        self.want[rd] = w.to(dev, non_blocking=True)
        keep = [r, w]
        req = [k for k, x in enumerate(wants) if x >= 0]
        if req:
            lp0, tid0, tlp0 = first
            n = tid0.shape[1]
            if n < max(wants):
                raise ValueError(f"logprobs: the first tokens were scored with top-{n}, a sequence asks for top-{max(wants)}")
            rr = torch.tensor([rows[k] for k in req], dtype=torch.int64)
            sr = torch.tensor([src[k] for k in req], dtype=torch.int64)
            keep += [rr, sr]
            rr, sr = rr.to(dev, non_blocking=True), sr.to(dev, non_blocking=True)
            self.lp[rr, 0] = lp0[sr]
            self.top_ids[rr, 0] = torch.nn.functional.pad(tid0[sr], (0, ops.LOGPROB_TOP_MAX - n), value=-1)
            self.top_lp[rr, 0] = torch.nn.functional.pad(tlp0[sr], (0, ops.LOGPROB_TOP_MAX - n), value=float("-inf"))
            self.n_rec[rr] = 1
        return keep

    @staticmethod
    def record(lp, top_ids, top_lp, row: int, n: int, want: int) -> LogprobRecord:
        """Row `row` of host copies of the three tables -> the record of its first n tokens."""
        return LogprobRecord(lp[row, :n].clone(), top_ids[row, :n, :want].clone(), top_lp[row, :n, :want].clone())


class BatchDecoder:
    """Greedy decode of up to 32 sequences at once: the weights are streamed ONCE per step for all sequences
    (fo1_gemv_batch_bf16), 5 launches per layer, and the whole step — embedding gather, 36 layers, lm_head, argmax, stop check,
    position bookkeeping — replays as one hipGraph with no host read inside the loop (the host polls a device-side `done` counter
    every few steps).  Reference semantics: HF greedy search over the 1-token fast path of omchat_qwen2_5_vl.py:143-155;
    positions = cache position + rope delta (modeling_qwen2_5_vl.py:1848-1860); a sequence stops AFTER its EOS / keyword id has
    been appended, or at max_new_tokens (mm_utils.py:137-181, 640-654)."""
    MAX_BATCH = 32          # 17..32 sequences: two 16-column groups per weight fragment (decode_mfma.hip, MM = 32)
    FUSED_COMBINE_MAX = 2   # up to this many sequences the o-projection combines the split-KV attention partials itself (0 = always the combine launch; A/B)
    IDS_CAP = 4096          # generated ids kept per sequence (every reference caller uses max_new_tokens <= 4096)
    MAX_STOP = 16           # stop ids the device-side rule compares against

    def __init__(self, llm: QwenLLM):
        self.llm = llm
        dev = llm.dev
        B = self.MAX_BATCH
        # persistent buffers are updated in place for the life of the engine: ordinary tensors even when the first request arrives
        # under the caller's torch.inference_mode() (the reference's inference.py:46)
        with torch.inference_mode(False):
            self.state = torch.zeros(B, 8, dtype=torch.int32, device=dev)
            self.plan = torch.zeros(B, 2, dtype=torch.int32, device=dev)
            self.ids = torch.zeros(B, self.IDS_CAP, dtype=torch.int32, device=dev)
            self.done = torch.zeros(1, dtype=torch.int32, device=dev)
            self.stop = torch.zeros(self.MAX_STOP, dtype=torch.int32, device=dev)
            self.reloc = torch.zeros(2 * B, 4, dtype=torch.int32, device=dev)      # (a shared-prefix sequence moves in two pieces)
            self.sparams = torch.zeros(B, 8, dtype=torch.int32, device=dev)        # fo1_sample_params_t per sequence (sampled head)
        self.sampled = False       # the step ends in a head that reads self.sparams (the sampled or the general one)
        self.general = False       # ... in the general head: some row has the greedy flag or a repetition penalty
        self.seen = None           # seen bitmap [MAX_BATCH, ld_words], allocated by the first start() with a penalty
        self.lpb = None            # log-probability records (LogprobBuffers), allocated by the first start() that asks for them
        self.masks = None          # token rules: the mask table (TokenMasks) and the per-row rule table, allocated by the first start() with a rule
        self.rules = None
        self.ruled = False         # some row of the current start() has a rule: the general head runs in its ruled form
        self._mask_rows: List[int] = []      # mask rows the current start() holds
        self.gtab = None           # token guides: the guide tables (GuideTables), the per-row guide table and the rows' automaton states,
        self.guides = None         # allocated by the first start() with a guide
        self.gstate = None
        self.guided = False        # some row of the current start() has a guide: the general head runs in its guided form
        self._guide_keys: list = []          # guide-table entries the current start() holds
        self.closes = None         # budget-aware guides: the per-row fo1_guide_close_t table, allocated by the first start() with a closing guide
        self.closing = False       # some row of the current start() has a closing rule: the guided head runs in its closing form
        self.btab = None           # soft steering: the bias table (BiasTable) and the per-row fo1_token_steer_t table, allocated by the first
        self.steers = None         # start() with a steer; the count table and its gate by the first start() with a count penalty
        self.counts = self.count_gate = None
        self.steered = False       # some row of the current start() has a steer: the general head runs in its steered form
        self._bias_rows: List[int] = []      # bias rows the current start() holds
        self.lp_want: List[int] = []       # per sequence of the current start(): -1 = no record, else its top-n
        self.n_stop = 0
        self.dk = self.dvt = None
        self.rows = 0
        self.slot = 0
        self.B = 0
        self._graphs: Dict[tuple, tuple] = {}
        self._keep: list = []
        self._ws_owner = ops.new_owner(self)

    def _ensure(self, rows: int, slot: int):
        c = self.llm.cfg
        if rows > self.rows:
            bf = torch.bfloat16
            with torch.inference_mode(False):
                self.dk = torch.zeros(c.num_layers, c.num_kv_heads, rows, c.head_dim, dtype=bf, device=self.llm.dev)
                self.dvt = torch.zeros(c.num_layers, c.num_kv_heads * c.head_dim, rows, dtype=bf, device=self.llm.dev)
            self.rows = rows
            self._graphs = {}
        # The rope table is indexed by POSITION (state[1] = L + rope delta + steps < slot), never by cache row: it needs `slot` rows,
        # not B * slot.  When it does grow, every graph that baked the old pointers in goes: this decoder's and the
        # single-sequence decode graph of the llm (the streamer path would otherwise replay against freed memory).
        if self.llm.rope_cos.shape[0] < slot:
            self.llm.grow_rope(slot)
            self._graphs = {}

    def start(self, seqs, deltas, first_tokens: torch.Tensor, max_new_tokens: int, stop_ids: Sequence[int] = (), sampling=None,
              prompt_ids: Optional[Sequence[Sequence[int]]] = None, logprobs=None, first_logprobs=None):
        """seqs: [(cache row offset, L, ...)] of the packed prefill that just ran on llm.kcache / llm.vtcache; first_tokens: device
        int32 [B] (the prefill's picks: greedy, or drawn with counter 0).  Moves every sequence to its own slot and accepts the first tokens
        on the device.  sampling: None = greedy steps; dict(temperature, top_p, top_k, seed[, streams]) = every step ends in the device
        sampler (fo1_decode_sample_accept), sequence b drawing Philox(tokens generated so far, streams[b]; seed) — streams defaults to
        0 .. B - 1, the sequence's index in its request list.  A dict with greedy=True or a repetition_penalty, or a list with one dict or
        None per sequence (sampling_table), ends every step in the general head (fo1_decode_head_accept); a penalty needs prompt_ids, the
        ids each request passed: they and the first tokens seed the sequence's seen set (the caller picked the first tokens with it).
        A dict's token-rule keys (ban, allow, ban_first, ban_until: token_rule) restrict that sequence's picks on the device; the rows of the
        mask table they take are held until the next start().  A dict's guide (guide=TokenGuide: sampling_guides) makes the banned set a
        function of the sequence's automaton state, which the head advances on the device; its table rows are held until the next start() too.
        A guide with accepting states closes before max_new_tokens runs out (guide.closing_bitmaps): the head reads the tokens left from the
        row's decode state; a start state further from an accepting one than the budget is a ValueError.
        A dict's steer keys (bias, frequency_penalty, presence_penalty: token_steer) bias that sequence's logits on the device and penalise
        the tokens it has generated, the first token included, by their counts (the head keeps them); the bias rows are held until the next
        start().
        logprobs (logprob_wants): None, one int or a list with None / int per sequence = the top-n of the log-probability record kept for that
        sequence (logprobs()); orthogonal to `sampling`: the record launch follows whichever head the step ends in.  first_logprobs: the first
        tokens' records, ops.logprob_rows on the prefill's logits with the largest requested n (FO1Engine._first_logprobs)."""
        llm = self.llm
        B = len(seqs)
        wants = logprob_wants(logprobs, B)
        if any(w >= 0 for w in wants) and first_logprobs is None:
            raise ValueError("BatchDecoder: logprobs needs first_logprobs, the first tokens' records")
        if B > self.MAX_BATCH:
            raise ValueError(f"BatchDecoder handles at most {self.MAX_BATCH} sequences")
        stop_ids = stop_id_list(stop_ids, self.MAX_STOP, "BatchDecoder", "; use the host loop")
        max_new = token_budget(max_new_tokens, self.IDS_CAP, "BatchDecoder", "; use the host loop")
        need = max(L for _, L, *_ in seqs) + max_new + 1
        slot = 1024
        while slot < need:
            slot *= 2
        self._ensure(max(B * slot, self.rows), slot)
        rope_id = (llm.rope_epoch, llm.rope_cos.data_ptr())
        if rope_id != getattr(self, "_rope_id", rope_id):
            self._graphs = {}              # graphs of the previous table are unreachable by key: release them and their pools
        self._rope_id = rope_id
        self.B, self.slot = B, slot
        self.len0, self.steps = max(L for _, L, *_ in seqs), 0      # host-side bound on any sequence's keys: len0 + steps + 1
        reloc = torch.tensor(reloc_rows(seqs, [b * slot for b in range(B)]), dtype=torch.int32)
        nr = reloc.shape[0]
        state = torch.tensor(live_state_rows([b * slot for b in range(B)], seqs, deltas, max_new), dtype=torch.int32)
        stop = torch.tensor(stop_ids + [0] * (self.MAX_STOP - len(stop_ids)), dtype=torch.int32)
        self.n_stop = len(stop_ids)
        self.reloc[:nr].copy_(reloc, non_blocking=True)
        self.state[:B].copy_(state, non_blocking=True)
        self.stop.copy_(stop, non_blocking=True)
        self._keep = [reloc, state, stop]                 # sources of the async uploads stay alive
        srows, kinds = sampling_table(sampling, B)
        trules = sampling_rules(sampling, B, llm.cfg.vocab_size)
        gplans = sampling_guides(sampling, B, llm.cfg.vocab_size, trules, prompt_ids, budget=max_new)
        tsteers = sampling_steers(sampling, B, llm.cfg.vocab_size)
        self.sampled = any(k != "plain" for k in kinds)
        self.general = self.sampled and any(k != "sampled" for k in kinds)
        penalised = any(ops.penalty_on(r[6]) for r in srows)
        if penalised and (prompt_ids is None or len(prompt_ids) != B):
            raise ValueError("BatchDecoder: a repetition penalty needs prompt_ids, one list per sequence")
        self._start_rules(unguided_rules(trules, gplans), gplans, first_tokens)
        self._start_steers(tsteers)
        if self.sampled:
            sp = ops.sample_params(srows)
            self.sparams[:B].copy_(sp, non_blocking=True)
            self._keep.append(sp)
        if penalised and self.seen is None:
            self.seen = new_seen(self.MAX_BATCH, llm.cfg.vocab_size, llm.dev)
        self.lp_want = wants
        if any(w >= 0 for w in wants):
            if self.lpb is None:
                self.lpb = LogprobBuffers(self.MAX_BATCH, self.IDS_CAP, llm.dev)
            self._keep += self.lpb.set_rows(list(range(B)), wants, first_logprobs, list(range(B)))
        self.done.zero_()
        first = first_tokens.to(torch.int32).contiguous()
        with ops.workspace_scope(self._ws_owner):
            ops.kv_relocate(llm.kcache, self.dk, llm.vtcache, self.dvt, self.reloc[:nr], max(L for _, L, *_ in seqs))
            ops.decode_argmax_accept(None, first, self.state[:B], self.plan[:B], self.ids[:B], self.stop[:self.n_stop], self.done)
            if penalised:      # the seen sets: the prompts' ids, then the first tokens
                self._keep += ops.mark_prompts(self.seen, llm.cfg.vocab_size, list(range(B)), prompt_ids)
                rt = torch.arange(B, dtype=torch.int32)
                self._keep.append(rt)
                ops.seen_mark(self.seen, llm.cfg.vocab_size, rt.to(first.device, non_blocking=True), first)
            if self.steered and any(t is not None and t.counting for t in tsteers):      # the counts: zero, then the first tokens
                self.counts[:B].zero_()
                self.count_gate[:B].zero_()
                ct = torch.arange(B, dtype=torch.int32)
                self._keep.append(ct)
                ops.count_mark(self.counts, self.count_gate, llm.cfg.vocab_size, ct.to(first.device, non_blocking=True), first)

    GUIDE_MASKS = 64         # mask rows kept for the guides' state bitmaps, beside the 3 per sequence of the rules

    def _start_rules(self, trules, gplans=(), first_tokens=None):
        """The previous run's mask and guide rows go back; this run's rules take theirs (3 rows per sequence at most: there is always room),
        then its guides (RuntimeError when their state bitmaps or tables do not fit)."""
        if self.gtab is not None:
            for k in self._guide_keys:
                self.gtab.release(k)
        self._guide_keys = []
        if self.masks is not None:
            for r in self._mask_rows:
                self.masks.release(r)
        self._mask_rows = []
        self.guided = any(g is not None for g in gplans)
        self.closing = False
        self.ruled = self.guided or any(t is not None for t in trules)
        if not self.ruled:
            return
        if self.masks is None:
            self.masks = TokenMasks(3 * self.MAX_BATCH + self.GUIDE_MASKS, self.llm.cfg.vocab_size, self.llm.dev)
            with torch.inference_mode(False):
                self.rules = ops.token_rules([None] * self.MAX_BATCH, self.llm.dev)
        table = []
        for t in trules:
            row, held = (None, []) if t is None else self.masks.rule_row(t)
            table.append(row)
            self._mask_rows += held
        rt = ops.token_rules(table)
        self.rules[:len(table)].copy_(rt, non_blocking=True)
        self._keep.append(rt)
        if self.guided:
            self._start_guides(gplans, first_tokens)

    def _start_steers(self, tsteers):
        """The previous run's bias rows go back; this run's steers take theirs (one row per sequence at most: there is always room).  The
        count table is allocated by the first run with a count penalty; start() zeroes its rows and counts the first tokens."""
        if self.btab is not None:
            for r in self._bias_rows:
                self.btab.release(r)
        self._bias_rows = []
        self.steered = any(t is not None for t in tsteers)
        if not self.steered:
            return
        V, dev = self.llm.cfg.vocab_size, self.llm.dev
        if self.btab is None:
            self.btab = BiasTable(self.MAX_BATCH, V, dev)
            with torch.inference_mode(False):
                self.steers = ops.token_steers([None] * self.MAX_BATCH, dev)
        if self.counts is None and any(t is not None and t.counting for t in tsteers):
            self.counts, self.count_gate = new_counts(self.MAX_BATCH, V, dev)
        table = []
        for t in tsteers:
            if t is None:
                table.append(None)
                continue
            row = -1 if t.bias is None else self.btab.acquire(t.bias)
            if row >= 0:
                self._bias_rows.append(row)
            table.append((row, t.f, t.q))
        st = ops.token_steers(table)
        self.steers[:len(table)].copy_(st, non_blocking=True)
        self._keep.append(st)

    def _steer_args(self) -> dict:
        if not self.steered:
            return {}
        return dict(steer=ops.SteerOperands(self.steers[:self.B], self.btab.table, self.btab.gate, self.counts, self.count_gate))

    def _start_guides(self, gplans, first_tokens):
        if self.gtab is None:
            self.gtab = GuideTables(self.llm.cfg.vocab_size, self.llm.dev, self.masks)
            with torch.inference_mode(False):
                self.guides = ops.token_guides([None] * self.MAX_BATCH, self.llm.dev)
                self.gstate = torch.zeros(self.MAX_BATCH, dtype=torch.int32, device=self.llm.dev)
        if not (self.gtab.room(gplans) and self.masks.room(self.gtab.new_bitmaps(gplans))):
            self.guided = self.ruled = False
            raise RuntimeError("BatchDecoder: the token guides of this batch do not fit the guide tables or the mask table")
        table = []
        for g in gplans:
            table.append(None if g is None else self.gtab.acquire(g))
            if g is not None:
                self._guide_keys.append(g.key)
        gt = ops.token_guides(table)
        gs = torch.tensor(guide_states_host(gplans, first_tokens), dtype=torch.int32)
        self.guides[:len(table)].copy_(gt, non_blocking=True)
        self.gstate[:len(table)].copy_(gs, non_blocking=True)
        self._keep += [gt, gs]
        for k, g in enumerate(gplans):
            if g is not None and g.after_first is not None:      # the caller picked the first token with the guided head: its state word
                self.gstate[k:k + 1].copy_(g.after_first.view(1), non_blocking=True)
        if any(g is not None and g.depth > 0 for g in gplans):      # every row's entry is written: a row without the rule gets depth 0
            if self.closes is None:
                with torch.inference_mode(False):
                    self.closes = ops.guide_closes([None] * self.MAX_BATCH, self.llm.dev)
            ct = ops.guide_closes([None if g is None else self.gtab.close_of(g.key) for g in gplans])
            self.closes[:len(table)].copy_(ct, non_blocking=True)
            self._keep.append(ct)
            self.closing = True

    def _rule_args(self) -> dict:
        if not self.ruled:
            return {}
        guide = {}
        if self.guided:
            guide = dict(guide=self.gtab.operands(self.guides[:self.B], self.gstate[:self.B], self.closes[:self.B] if self.closing else None))
        return dict(masks=self.masks.table, rules=self.rules[:self.B], **guide)

    KV_BUCKET = 2048

    def kv_bucket(self) -> int:
        """Upper bound on the keys any sequence attends in the coming step, rounded up to KV_BUCKET rows (capped by the slot): the
        attention launch geometry follows it (one workgroup per KV head and sequence up to 2048 keys), so a 4096-token budget does
        not make every step pay the long-context split.  A new bucket means a new captured graph, once per 2048 generated tokens."""
        need = self.len0 + self.steps + 1
        return min(self.slot, -(-need // self.KV_BUCKET) * self.KV_BUCKET)

    def _step_device(self):
        llm, B = self.llm, self.B
        c = llm.cfg
        H, KV, HD = c.num_heads, c.num_kv_heads, c.head_dim
        scale = 1.0 / math.sqrt(HD)
        st = self.state[:B]
        from . import stage_abi
        if stage_abi.enabled() and not self.sampled and not self.recording:      # the same launches, sequenced by fo1_llm_decode_step (csrc/stages.hip: the greedy head, no records)
            with ops.workspace_scope(self._ws_owner):
                return stage_abi.llm_stage(llm).decode_step(self)
        with ops.workspace_scope(self._ws_owner):
            x = ops.gather_rows(self.plan[:B], c.hidden_size, llm.embed)
            for li, w in enumerate(llm.layers):
                q = ops.gemv_batch(x, w["wqkv"], w["bqkv"], mode=ops.GB_QKV, norm_weight=w["ln1"], norm_eps=c.rms_norm_eps,
                                   qkv=dict(n_q=H, n_kv=KV, cos=llm.rope_cos, sin=llm.rope_sin, state=st, kcache=self.dk[li], vtcache=self.dvt[li]))
                if B <= self.FUSED_COMBINE_MAX and H * HD <= 2048 and c.hidden_size <= 4096:
                    # one or two sequences (the reference's own batch-1 loop): the o-projection sums the split-KV partials in its prologue — same
                    # bits as the combine launch (one shared routine, csrc/decode_common.h), one launch less per layer
                    part, pstride, chunk = ops.attention_decode_batch_partials(q, self.dk[li], self.dvt[li], st, self.kv_bucket(), H, KV, HD, scale)
                    x = ops.gemv_attn_combine(part, pstride, st, chunk, H, KV, w["wo"], residual=x)
                else:
                    att = ops.attention_decode_batch(q, self.dk[li], self.dvt[li], st, self.kv_bucket(), H, KV, HD, scale)
                    x = ops.gemv_batch(att, w["wo"], residual=x)
                a = ops.gemv_batch(x, w["wgu"], mode=ops.GB_SWIGLU, norm_weight=w["ln2"], norm_eps=c.rms_norm_eps)
                x = ops.gemv_batch(a, w["wdown"], residual=x)
            logits = ops.gemv_batch(x, llm.lm_head, norm_weight=llm.norm, norm_eps=c.rms_norm_eps)
            if self.general:
                ops.decode_head_accept(logits, self.sparams[:B], st, self.plan[:B], self.ids[:B], self.stop[:self.n_stop], self.done, seen=self.seen,
                                       **self._rule_args(), **self._steer_args())
            elif self.sampled:
                ops.decode_sample_accept(logits, self.sparams[:B], st, self.plan[:B], self.ids[:B], self.stop[:self.n_stop], self.done)
            else:
                ops.decode_argmax_accept(logits, None, st, self.plan[:B], self.ids[:B], self.stop[:self.n_stop], self.done)
            if self.recording:      # after the head, whichever it was: the accepted ids' log-probabilities on this step's raw logits
                lb = self.lpb
                ops.decode_logprob_record(logits, lb.want[:B], st, self.ids[:B], lb.n_rec[:B], lb.lp[:B], lb.top_ids[:B], lb.top_lp[:B])
            return logits

    @property
    def recording(self) -> bool:
        """Some sequence of the current start() asked for log-probabilities: every step ends in the record launch."""
        return any(w >= 0 for w in self.lp_want)

    def step(self, use_graph: bool = True):
        """One token for every live sequence."""
        if not use_graph:
            out = self._step_device()
            self.steps += 1
            return out
        # the rope tables' identity is part of the key: QwenLLM.reserve() on a larger later batch or a sibling decoder may re-allocate
        # them (grow_rope) while this decoder's graphs survive — a replay would read the freed table
        key = (self.B, self.slot, self.n_stop, self.kv_bucket(), self.llm.rope_epoch, self.llm.rope_cos.data_ptr(), self.sampled)
        seen = ()
        if self.general:     # (one more form; the bitmap's identity is baked into its graph, and the warm-up step sets bits in it)
            seen = () if self.seen is None else (self.seen,)
            key += ("general", self.seen.data_ptr() if seen else 0)
            if self.ruled:   # (the ruled form reads the mask and rule tables and writes neither: identity in the key, nothing more to roll back)
                key += ("ruled", self.masks.table.data_ptr(), self.rules.data_ptr())
            if self.guided:  # (the guided form advances the rows' automaton states: they join the rollback, or the first replay would start
                key += ("guided", *self.gtab.pointers(), self.guides.data_ptr(), self.gstate.data_ptr())      # from the warm-up step's states)
                seen += (self.gstate,)
            if self.closing:  # (the closing form reads two more tables and writes neither: nothing more to roll back)
                key += ("closing", self.gtab.close_row.data_ptr(), self.closes.data_ptr())
            if self.steered:  # (the steered form reads the bias table and the steers and counts the accepted tokens: the counts join the rollback)
                key += ("steered", self.btab.table.data_ptr(), self.steers.data_ptr(), self.counts.data_ptr() if self.counts is not None else 0)
                if self.counts is not None:
                    seen += (self.counts, self.count_gate)
        if self.recording:   # (and one more: the record launch bakes the buffers' identity in, and the warm-up step writes them)
            key += ("logprobs", self.lpb.lp.data_ptr())
            seen += self.lpb.written()
        ent = self._graphs.get(key)
        if ent is None:      # (ops.capture_graph: the warm-up step is rolled back)
            ent = self._graphs[key] = ops.capture_graph(self._step_device, rollback=(self.state, self.plan, self.ids, self.done, *seen))
        ops.replay_graph(ent[0])
        self.steps += 1
        return ent[1]

    def results(self) -> List[List[int]]:
        """Generated ids per sequence so far (first token included)."""
        B = self.B
        n = self.state[:B, 4].cpu().tolist()
        ids = self.ids[:B, :max(n)].cpu().tolist()
        return [row[:k] for row, k in zip(ids, n)]

    def logprobs(self) -> List[Optional[LogprobRecord]]:
        """The log-probability record of every sequence so far (first token included); None for a sequence that did not ask."""
        B = self.B
        if not self.recording:
            return [None] * B
        n = self.state[:B, 4].cpu().tolist()
        lb = self.lpb
        lp, ti, tl = (t[:B, :max(n)].cpu() for t in (lb.lp, lb.top_ids, lb.top_lp))
        return [None if w < 0 else LogprobBuffers.record(lp, ti, tl, b, n[b], w) for b, w in enumerate(self.lp_want)]

    def run(self, max_new_tokens: int, use_graph: bool = True, poll: int = 8) -> List[List[int]]:
        """Decode until every sequence has stopped (or max_new_tokens).  Returns the generated ids per sequence, the first
        token (from the prefill) included."""
        B = self.B
        max_new = max(1, min(int(max_new_tokens), self.IDS_CAP))      # start() has already refused a larger budget
        for i in range(max_new - 1):
            if i % poll == 0 and int(self.done.item()) >= B:     # the only host read in the loop, every `poll` steps
                break
            self.step(use_graph)
        return self.results()


def run_decoders(decs: Sequence["BatchDecoder"], streams: Sequence, max_new_tokens: int, use_graph: bool = True, poll: int = 8) -> List[List[List[int]]]:
    """Several started decode groups advanced TOGETHER, each on its own HIP stream: a step of one group is a chain of ~180 short
    kernels (5 per layer) with launch gaps between them and ~2.5 TB/s of an 8 TB/s memory system in use — the chains of two groups
    interleave on the GPU, so a pass of 25 sequences (13 + 12) finishes its 64 tokens in about the time one group of 16 takes alone
    instead of the sum of two (bench.py `end_to_end`).  Per sequence nothing changes: same kernels, same sums, same ids.
    -> [ids per sequence] per group."""
    max_new = max(1, min(int(max_new_tokens), BatchDecoder.IDS_CAP))
    live = list(range(len(decs)))
    for i in range(max_new - 1):
        if i % poll == 0:      # the only host reads: each group's `done` counter on the group's own stream, every `poll` steps
            still = []
            for k in live:
                with torch.cuda.stream(streams[k]):
                    if int(decs[k].done.item()) < decs[k].B:
                        still.append(k)
            live = still
            if not live:
                break
        for k in live:
            with torch.cuda.stream(streams[k]):
                decs[k].step(use_graph)
    out = []
    for k, d in enumerate(decs):
        with torch.cuda.stream(streams[k]):
            out.append(d.results())
    return out


class DecodePool:
    """Continuous batching for the greedy decode loop: a pool of 64 / 128 sequence SLOTS that advance together,
    one token per step, through ONE stream of the weights.  Sequences JOIN whenever a packed prefill pass has finished (their K / V^T
    rows are relocated out of that pass's cache into free slots, first tokens accepted on the device) and LEAVE individually when their
    stop rule fires (device-side, as in BatchDecoder); the step itself always computes all P rows — empty and finished slots are rows
    nobody reads, their attention is skipped on the device.  Every position-dependent quantity lives in device memory, so one captured
    hipGraph per (kv-length bucket) serves every step whatever the occupancy.

    Past 32 sequences the step's projections are skinny GEMMs C[P, N] = x[P, K] W[N, K]^T: the prefill's LDS-DMA tile kernels at M = P
    (fo1_gemm_bf16: 64 x 64 / 64 x 128 rings for the few-row shapes, 128 x 128 for gate/up and lm_head), RMSNorm and the q/k/v
    post-processing (mRoPE at each slot's position + cache append, fo1_pool_qkv_post_bf16) as their own launches, the split-KV decode
    attention with 256 keys per workgroup.  A dedicated weights-to-VGPR streaming kernel was built and measured first
    (profiles/r04_pool_gemm_stream_kernel_vs_tile_kernels.json: 1.3-1.6x SLOWER than the tile kernels on every shape — two K tiles of
    register prefetch cannot cover the HBM latency that a 3-4 stage LDS ring does) and is not in the tree.

    Reference semantics per sequence: HF greedy search over the 1-token fast path of omchat_qwen2_5_vl.py:143-155; positions = cache
    position + rope delta (modeling_qwen2_5_vl.py:1848-1860); stop AFTER the EOS / keyword id has been appended, or at max_new_tokens
    (mm_utils.py:137-181, 640-654).  A sequence's ids do not depend on its slot or on its neighbours (every kernel's per-row fp32 sum
    order is a function of the launch shape only, and the shape is always P rows; tests/test_decode_pool_gpu.py)."""
    IDS_CAP = 4096
    MAX_STOP = 16
    MAX_SETS = 32            # distinct stop-id sets live in the pool at once
    MAX_MASKS = 64           # distinct token masks (rows of the mask table) live in the pool at once
    MAX_BIAS = 16            # distinct logit-bias vectors (rows of the bias table) live in the pool at once
    KV_BUCKET = 256          # the attention launch geometry follows the longest live context rounded up to this many keys

    def __init__(self, llm: QwenLLM, slots: int = 128, slot_rows: int = 1024):
        if slots not in (64, 128):
            raise ValueError("a decode pool has 64 or 128 slots")
        self.llm, self.P = llm, slots
        dev = llm.dev
        P = slots
        with torch.inference_mode(False):
            self.state = torch.tensor(empty_state_rows([0] * P), dtype=torch.int32).to(dev)      # every slot starts empty (_ensure places them)
            self.plan = torch.zeros(P, 2, dtype=torch.int32, device=dev)
            self.ids = torch.zeros(P, self.IDS_CAP, dtype=torch.int32, device=dev)
            self.done = torch.zeros(1, dtype=torch.int32, device=dev)
            # per-sequence stop rules (round 5): a table of stop-id sets {count, ids[16]}; state[slot][6] names a slot's set, so submissions
            # with different stop ids / templates share the pool (before: one set per pool, anything else waited for a full drain)
            self.stop = torch.zeros(self.MAX_SETS, 1 + self.MAX_STOP, dtype=torch.int32, device=dev)
            self.reloc = torch.zeros(2 * P, 4, dtype=torch.int32, device=dev)     # (a shared-prefix sequence moves in two pieces)
            # per-slot fo1_sample_params_t rows, read by the general head only: a plain slot rides as a greedy row without penalty
            self.sparams = ops.sample_params([ops.sampling_row(None)] * P, dev)
        self.seen = None                               # seen bitmap [P, ld_words], allocated when the first penalised sequence joins
        self.kind = ["plain"] * P                      # what each slot's sparams row holds: "plain", "sampled" or "general"
        self.n_general = 0                             # live slots that are not plain: > 0 ends the step in the general head
        self.masks = None                              # token rules: the mask table (TokenMasks) and the per-slot rule table, allocated when
        self.rules = None                              # the first constrained sequence joins
        self.ruled_dev = [False] * P                   # does the slot's rule row on the device hold a rule (tracked as `kind` is)
        self.slot_masks: List[List[int]] = [[] for _ in range(P)]      # mask rows a live slot holds
        self.n_ruled = 0                               # live slots with a rule: > 0 runs the general head in its ruled form
        self.gtab = None                               # token guides: the guide tables (GuideTables), the per-slot guide table and the slots'
        self.guides = None                             # automaton states, allocated when the first guided sequence joins
        self.gstate = None
        self.guided_dev = [False] * P                  # does the slot's guide row on the device hold a guide (tracked as `kind` is)
        self.slot_guide: list = [None] * P             # the guide-table entry a live slot holds
        self.n_guided = 0                              # live slots with a guide: > 0 runs the general head in its guided form
        self.closes = None                             # budget-aware guides: the per-slot fo1_guide_close_t table, allocated when the first
        self.close_dev = [False] * P                   # closing sequence joins; does the slot's row on the device hold depth > 0 (as `kind`)
        self.slot_close = [False] * P                  # a live slot's guide has a closing rule
        self.n_closing = 0                             # live slots with a closing rule: > 0 runs the guided head in its closing form
        self.btab = None                               # soft steering: the bias table (BiasTable) and the per-slot fo1_token_steer_t table, allocated
        self.steers = None                             # when the first steered sequence joins; the count table and its gate when the first
        self.counts = self.count_gate = None           # sequence with a count penalty does
        self.steer_dev = [False] * P                   # does the slot's steer row on the device hold a steer (tracked as `kind` is)
        self.slot_bias = [-1] * P                      # the bias row a live slot holds
        self.slot_steer = [False] * P                  # a live slot has a steer
        self.n_steered = 0                             # live slots with a steer: > 0 runs the general head in its steered form
        self.lpb = None                                # log-probability records (LogprobBuffers), allocated when the first requesting sequence joins
        self.lp_want = [-1] * P                        # a live slot's request: -1 = no record, else its top-n
        self.lp_dev = [-1] * P                         # what each slot's `want` word on the device holds (tracked as `kind` is)
        self.n_logprob = 0                             # live requesting slots: > 0 adds the record launch to the step
        self._sets: Dict[tuple, int] = {}              # stop-id tuple -> row of self.stop
        self._set_users = [0] * self.MAX_SETS          # live slots per row (a row with users is never rewritten)
        self.slot_set = [0] * P
        self.slot_rows = 0
        self.dk = self.dvt = None
        self.free = list(range(P))                     # host view of the slots
        self.bound = [0] * P                           # upper bound of the keys a live slot attends in the coming step
        self.budget = [0] * P
        self.live: Dict[int, object] = {}              # slot -> caller's tag
        self.steps_run = 0
        self._graphs: Dict[tuple, tuple] = {}
        self._keep: list = []
        self._ws_owner = ops.new_owner(self)
        self._ensure(slot_rows)
        self._tiled()

    # ---- memory ----------------------------------------------------------------------------------------------------------------
    def _ensure(self, slot_rows: int):
        """Slots of at least slot_rows cache rows each (power of two).  Re-allocation is only possible while the pool is empty."""
        rows = 1024
        while rows < slot_rows:
            rows *= 2
        if rows > self.slot_rows:
            if self.live:
                raise RuntimeError("DecodePool: slots can only grow while the pool is empty")
            c = self.llm.cfg
            bf = torch.bfloat16
            with torch.inference_mode(False):
                self.dk = self.dvt = None
                self.dk = torch.zeros(c.num_layers, c.num_kv_heads, self.P * rows, c.head_dim, dtype=bf, device=self.llm.dev)
                self.dvt = torch.zeros(c.num_layers, c.num_kv_heads * c.head_dim, self.P * rows, dtype=bf, device=self.llm.dev)
            self.slot_rows = rows
            self._graphs = {}
            # an empty / finished slot still runs every step: its (ignored) K / V^T rows must land inside ITS OWN slot — row 0 of the
            # cache is slot 0's first prompt token
            with torch.inference_mode(False):
                self.state.copy_(torch.tensor(empty_state_rows([s * rows for s in range(self.P)]), dtype=torch.int32))
        if self.llm.rope_cos.shape[0] < self.slot_rows:
            self.llm.grow_rope(self.slot_rows)
            self._graphs = {}

    def fits(self, seqs, max_new_tokens: int) -> bool:
        return max(L for _, L, *_ in seqs) + max(1, int(max_new_tokens)) + 1 <= self.slot_rows

    # ---- join ------------------------------------------------------------------------------------------------------------------
    def join(self, kcache: torch.Tensor, vtcache: torch.Tensor, seqs, deltas, first_tokens: torch.Tensor, max_new_tokens: int,
             stop_ids: Sequence[int] = (), tags: Optional[Sequence] = None, sampling=None,
             prompt_ids: Optional[Sequence[Sequence[int]]] = None, logprobs=None, first_logprobs=None) -> List[int]:
        """seqs [(cache row offset, L, ...)] of a packed prefill that ran on (kcache, vtcache); first_tokens device int32 [B].  Enqueues,
        on the CURRENT stream (the pool's), the relocation of every sequence into a free slot and the on-device accept of its first
        token.  Returns the slots.  Raises if there is no room (callers check `len(pool.free)` / `fits()` first).
        sampling (sampling_table): None = plain greedy sequences, which join exactly as they always have; one dict for the submission or a
        list with one dict or None per sequence = that sequence's row of the per-slot parameter table — temperature / top-k / top-p draws
        on Philox(tokens generated so far, stream; seed), greedy=True, repetition_penalty.  A penalty needs prompt_ids (the ids each request
        passed): the slot's seen-bitmap row is cleared and marked with them and with the first token, which the caller picked with the
        prompt's set.  While any live slot is not plain the step ends in the general head (step()).  A dict's token-rule keys (ban, allow,
        ban_first, ban_until: token_rule) restrict that sequence's picks on the device: equal banned sets share a row of the mask table, at
        most MAX_MASKS distinct ones are live at once (can_take), and the rows are released when the sequence is harvested.
        A dict's guide (guide=TokenGuide: sampling_guides) makes the banned set a function of the sequence's automaton state, which the head
        advances on the device: the slot's state word is set here to the state after the first token (the dict's guide_state word when the
        caller picked that token with the guided head, else computed on the host from first_tokens — one host read), every state's bitmap
        takes a mask row (equal ones are shared, within and across guides), and the rows are released when the sequence is harvested.
        A guide with accepting states closes before max_new_tokens runs out (guide.closing_bitmaps): its (state, tokens left) bitmaps take
        mask rows too, the head reads the tokens left from the slot's decode state, and a start state further from an accepting one than
        the budget is a ValueError.  While no such sequence is live the step is the guided (or ruled, or general, or greedy) one.
        A dict's steer keys (bias, frequency_penalty, presence_penalty: token_steer) bias that sequence's logits and penalise the tokens it
        has generated by their counts: equal bias vectors share a row of the bias table, at most MAX_BIAS distinct ones are live at once
        (can_take), and the row is released when the sequence is harvested; the slot's count row is zeroed here and the first token counted.
        While no steered sequence is live the step is the one it was.
        logprobs / first_logprobs: as BatchDecoder.start takes them; while any live slot asks for a record the record launch follows the head
        (step()), and harvest(records=True) hands the finished slots' records out.  A pool no requesting sequence ever joined holds no
        record buffer and issues exactly the launches and copies it always has."""
        B = len(seqs)
        wants = logprob_wants(logprobs, B)
        if any(w >= 0 for w in wants) and first_logprobs is None:
            raise ValueError("DecodePool: logprobs needs first_logprobs, the first tokens' records")
        srows, kinds = sampling_table(sampling, B)
        trules = sampling_rules(sampling, B, self.llm.cfg.vocab_size)
        max_new = token_budget(max_new_tokens, self.IDS_CAP, "DecodePool")
        gplans = sampling_guides(sampling, B, self.llm.cfg.vocab_size, trules, prompt_ids, budget=max_new)
        trules = unguided_rules(trules, gplans)
        tsteers = sampling_steers(sampling, B, self.llm.cfg.vocab_size)
        penalised = [ops.penalty_on(r[6]) for r in srows]
        if any(penalised) and (prompt_ids is None or len(prompt_ids) != B):
            raise ValueError("DecodePool: a repetition penalty needs prompt_ids, one list per sequence")
        full = self._table_without_room(trules, gplans, tsteers)
        if full is not None:
            raise RuntimeError(f"DecodePool: {full}; wait for sequences to finish")
        set_row = self._stop_set_row(tuple(stop_id_list(stop_ids, self.MAX_STOP, "DecodePool")))
        if B > len(self.free):
            raise RuntimeError(f"DecodePool: {B} sequences, {len(self.free)} free slots")
        if not self.fits(seqs, max_new):
            self._ensure(max(L for _, L, *_ in seqs) + max_new + 1)      # raises unless the pool is empty
        self.free.sort()
        slots = [self.free.pop(0) for _ in range(B)]
        try:
            self._join_slots(slots, kcache, vtcache, seqs, deltas, first_tokens, max_new, set_row)
            self._join_sampling(slots, srows, kinds, penalised, first_tokens, prompt_ids)
            self._join_rules(slots, trules)
            self._join_guides(slots, gplans, first_tokens)
            self._join_steers(slots, tsteers, first_tokens)
            self._join_logprobs(slots, wants, first_logprobs)
        except BaseException:
            # nothing of this submission is live: its slots go back (their device state may be half written — the next occupant's
            # join rewrites state, plan and K / V^T rows; until then the slot is marked finished so that no step reads it)
            done = torch.tensor(empty_state_rows([s * self.slot_rows for s in slots]), dtype=torch.int32)
            self._keep.append(done)
            try:
                for k, sl in enumerate(slots):
                    self.state[sl:sl + 1].copy_(done[k:k + 1], non_blocking=True)
            except BaseException:
                pass
            self.free += slots
            for s in slots:
                self._release_masks(s)
                self._release_guide(s)
                self._release_bias(s)
            raise
        for k, s in enumerate(slots):
            # a tag identifies ONE occupancy of a slot: harvest() compares it by identity against an older snapshot, so the default must
            # be unique per join (with None, `None is None` handed a re-joined slot's new occupant the old occupant's ids — ADVICE r4)
            self.live[s] = tags[k] if tags is not None else object()
            self.bound[s] = seqs[k][1] + 1
            self.budget[s] = max_new
            self.slot_set[s] = set_row
            self._set_users[set_row] += 1
            self.n_general += kinds[k] != "plain"
            self.n_ruled += trules[k] is not None
            self.n_guided += gplans[k] is not None
            self.slot_close[s] = gplans[k] is not None and gplans[k].depth > 0
            self.n_closing += self.slot_close[s]
            self.slot_steer[s] = tsteers[k] is not None
            self.n_steered += self.slot_steer[s]
            self.lp_want[s] = wants[k]
            self.n_logprob += wants[k] >= 0
        return slots

    def _join_logprobs(self, slots, wants, first_logprobs):
        """The record requests of a submission's slots.  Nothing is enqueued for a non-requesting sequence whose slot's `want` word is off
        already: a slot a requesting sequence has left gets -1 back when a non-requesting one reuses it."""
        write = [k for k, s in enumerate(slots) if wants[k] >= 0 or self.lp_dev[s] >= 0]
        if not write:
            return
        if self.lpb is None:      # (graphs captured before are unreachable for a recording step: its key holds the buffers' identity)
            self.lpb = LogprobBuffers(self.P, self.IDS_CAP, self.llm.dev)
        self._keep += self.lpb.set_rows([slots[k] for k in write], [wants[k] for k in write], first_logprobs, write)
        for k in write:
            self.lp_dev[slots[k]] = wants[k]

    def _table_without_room(self, trules, gplans=(), tsteers=()) -> Optional[str]:
        """None when there is a mask row for every banned set of the rules and every state bitmap of the guides, room in the guide tables and
        a bias row for every bias vector of the steers; else which table is full."""
        biases = [t.bias for t in tsteers if t is not None and t.bias is not None]
        if biases and not (self.btab.room(biases) if self.btab is not None else len(set(biases)) <= self.MAX_BIAS):
            return f"{self.MAX_BIAS} different logit-bias vectors are live"
        maps = [m for t in trules if t is not None for m in t.bitmaps()]
        if any(g is not None for g in gplans):      # (nothing allocated yet: the same answers from the bookkeeping alone)
            gtab = self.gtab if self.gtab is not None else GuideTables(self.llm.cfg.vocab_size, None, None)
            if not gtab.room(gplans):
                return "the token-guide tables (class rows, transitions, state rows, closing rows) are full"
            maps += gtab.new_bitmaps(gplans)
        if not maps or (self.masks.room(maps) if self.masks is not None else len(set(maps)) <= self.MAX_MASKS):
            return None
        return f"{self.MAX_MASKS} different token masks are live"

    def _mask_room(self, trules, gplans=(), tsteers=()) -> bool:
        return self._table_without_room(trules, gplans, tsteers) is None

    def _join_steers(self, slots, tsteers, first_tokens):
        """The steer rows, bias rows and count rows of a submission's slots.  Nothing is enqueued for a sequence without a steer whose slot
        holds none: a slot a steered sequence has left gets the "none" row back when an unsteered one reuses it."""
        write = [k for k, s in enumerate(slots) if tsteers[k] is not None or self.steer_dev[s]]
        if not write:
            return
        V, dev = self.llm.cfg.vocab_size, self.llm.dev
        if self.btab is None:      # (graphs captured before are unreachable for a steered step: its key holds the tables' identity)
            self.btab = BiasTable(self.MAX_BIAS, V, dev)
            with torch.inference_mode(False):
                self.steers = ops.token_steers([None] * self.P, dev)
        counting = [k for k in write if tsteers[k] is not None and tsteers[k].counting]
        if counting and self.counts is None:
            self.counts, self.count_gate = new_counts(self.P, V, dev)
        table = []
        for k in write:
            t = tsteers[k]
            if t is None:
                table.append(None)
                continue
            row = -1 if t.bias is None else self.btab.acquire(t.bias)
            self.slot_bias[slots[k]] = row
            table.append((row, t.f, t.q))
        st = ops.token_steers(table)
        self._keep.append(st)
        for j, k in enumerate(write):
            self.steers[slots[k]:slots[k] + 1].copy_(st[j:j + 1], non_blocking=True)
            self.steer_dev[slots[k]] = tsteers[k] is not None
        if counting:      # a counting slot's row starts from zero, then its first token
            for k in counting:
                self.counts[slots[k]].zero_()
                self.count_gate[slots[k]].zero_()
            first = first_tokens.to(torch.int32).contiguous()
            rt = torch.tensor([slots[k] if k in counting else -1 for k in range(len(slots))], dtype=torch.int32)      # (row -1: skipped)
            self._keep.append(rt)
            with ops.workspace_scope(self._ws_owner):
                ops.count_mark(self.counts, self.count_gate, V, rt.to(first.device, non_blocking=True), first)

    def _release_bias(self, slot: int) -> None:
        if self.slot_bias[slot] >= 0:
            self.btab.release(self.slot_bias[slot])
            self.slot_bias[slot] = -1

    def _ensure_masks(self):
        if self.masks is None:      # (graphs captured before are unreachable for a ruled step: its key holds the tables' identity)
            self.masks = TokenMasks(self.MAX_MASKS, self.llm.cfg.vocab_size, self.llm.dev)
            with torch.inference_mode(False):
                self.rules = ops.token_rules([None] * self.P, self.llm.dev)

    def _join_guides(self, slots, gplans, first_tokens):
        """The guide rows and automaton states of a submission's slots.  Nothing is enqueued for a sequence without a guide whose slot holds
        none: a slot a guided sequence has left gets cls_row = -1 back when an unguided one reuses it."""
        write = [k for k, s in enumerate(slots) if gplans[k] is not None or self.guided_dev[s]]
        if not write:
            return
        self._ensure_masks()
        if self.gtab is None:
            self.gtab = GuideTables(self.llm.cfg.vocab_size, self.llm.dev, self.masks)
            with torch.inference_mode(False):
                self.guides = ops.token_guides([None] * self.P, self.llm.dev)
                self.gstate = torch.zeros(self.P, dtype=torch.int32, device=self.llm.dev)
        table = []
        for k in write:
            table.append(None if gplans[k] is None else self.gtab.acquire(gplans[k]))
            if gplans[k] is not None:
                self.slot_guide[slots[k]] = gplans[k].key
        gt = ops.token_guides(table)
        gs = torch.tensor(guide_states_host(gplans, first_tokens), dtype=torch.int32)
        self._keep += [gt, gs]
        for j, k in enumerate(write):
            s = slots[k]
            self.guides[s:s + 1].copy_(gt[j:j + 1], non_blocking=True)
            self.guided_dev[s] = gplans[k] is not None
            if gplans[k] is not None:
                src = gplans[k].after_first
                self.gstate[s:s + 1].copy_(gs[k:k + 1] if src is None else src.view(1), non_blocking=True)
        self._join_closes(slots, gplans)

    def _join_closes(self, slots, gplans):
        """The closing rows of a submission's slots.  Nothing is enqueued for a sequence without a closing rule whose slot holds none: a slot
        a closing sequence has left gets depth = 0 back when a sequence without the rule reuses it."""
        closing = [g is not None and g.depth > 0 for g in gplans]
        write = [k for k, s in enumerate(slots) if closing[k] or self.close_dev[s]]
        if not write:
            return
        if self.closes is None:      # (graphs captured before are unreachable for a closing step: its key holds the table's identity)
            with torch.inference_mode(False):
                self.closes = ops.guide_closes([None] * self.P, self.llm.dev)
        ct = ops.guide_closes([self.gtab.close_of(gplans[k].key) if closing[k] else None for k in write])
        self._keep.append(ct)
        for j, k in enumerate(write):
            self.closes[slots[k]:slots[k] + 1].copy_(ct[j:j + 1], non_blocking=True)
            self.close_dev[slots[k]] = closing[k]

    def _release_guide(self, slot: int) -> None:
        if self.slot_guide[slot] is not None:
            self.gtab.release(self.slot_guide[slot])
            self.slot_guide[slot] = None

    def _join_rules(self, slots, trules):
        """The rule rows of a submission's slots.  Nothing is enqueued for a sequence without a rule whose slot holds none: a slot a
        constrained sequence has left gets -1 back when an unconstrained one reuses it."""
        write = [k for k, s in enumerate(slots) if trules[k] is not None or self.ruled_dev[s]]
        if not write:
            return
        self._ensure_masks()
        table = []
        for k in write:
            row, held = (None, []) if trules[k] is None else self.masks.rule_row(trules[k])
            table.append(row)
            self.slot_masks[slots[k]] += held
        rt = ops.token_rules(table)
        self._keep.append(rt)
        for j, k in enumerate(write):
            self.rules[slots[k]:slots[k] + 1].copy_(rt[j:j + 1], non_blocking=True)
            self.ruled_dev[slots[k]] = trules[k] is not None

    def _release_masks(self, slot: int) -> None:
        for r in self.slot_masks[slot]:
            self.masks.release(r)
        self.slot_masks[slot] = []

    def _join_sampling(self, slots, srows, kinds, penalised, first_tokens, prompt_ids):
        """The parameter rows and seen sets of a submission's slots.  Nothing is enqueued for a plain sequence whose slot still holds the
        plain row: a pool that only ever sees plain sequences issues exactly the launches it always has."""
        write = [k for k, s in enumerate(slots) if kinds[k] != "plain" or self.kind[s] != "plain"]
        if write:
            sp = ops.sample_params([srows[k] for k in write])
            self._keep.append(sp)
            for j, k in enumerate(write):
                self.sparams[slots[k]:slots[k] + 1].copy_(sp[j:j + 1], non_blocking=True)
                self.kind[slots[k]] = kinds[k]
        pen = [k for k in range(len(slots)) if penalised[k]]
        if pen:
            V = self.llm.cfg.vocab_size
            if self.seen is None:      # (a general-head graph captured without the bitmap is unreachable from here on: its key holds the pointer)
                self.seen = new_seen(self.P, V, self.llm.dev)
            first = first_tokens.to(torch.int32).contiguous()
            rt = torch.tensor([slots[k] if penalised[k] else -1 for k in range(len(slots))], dtype=torch.int32)      # (row -1: skipped)
            self._keep.append(rt)
            with ops.workspace_scope(self._ws_owner):
                self._keep += ops.mark_prompts(self.seen, V, [slots[k] for k in pen], [prompt_ids[k] for k in pen])
                ops.seen_mark(self.seen, V, rt.to(first.device, non_blocking=True), first)

    def can_take(self, stop_ids: Sequence[int], sampling=None, B: int = 0) -> bool:
        """Is there a table row for this stop-id set (its own, or one no live slot uses) — and, for a submission of B sequences with
        `sampling`, a mask-table row for every banned set of its token rules and a bias-table row for every bias vector of its steers?  (A
        malformed rule or steer answers True: join() raises it.)"""
        key = tuple(sorted(set(int(t) for t in stop_ids)))
        if not (key in self._sets or any(u == 0 for u in self._set_users)):
            return False
        if sampling is None:
            return True
        try:      # (a submission that finds no room in a table nobody uses never will: join() raises that too)
            trules = sampling_rules(sampling, B, self.llm.cfg.vocab_size)
            gplans = []      # (the tables a guide takes do not depend on the state it starts in: no prompt ids needed here)
            for sp, t in zip(_per_sequence(sampling, B), trules):
                g, always = (sp.get("guide") if sp is not None else None), (t.always if t is not None else None)
                if g is not None and not isinstance(g, TokenGuide):
                    raise ValueError("guide: not a TokenGuide")
                gplans.append(None if g is None else guide_plan(g, always, g.start))
            tsteers = sampling_steers(sampling, B, self.llm.cfg.vocab_size)
            if self._table_without_room((), (), tsteers) is not None and self.btab is not None and any(self.btab.users):
                return False
            return self._mask_room(unguided_rules(trules, gplans), gplans) or self.masks is None or not any(self.masks.users)
        except ValueError:
            return True

    def _stop_set_row(self, stop_ids: tuple) -> int:
        row = self._sets.get(stop_ids)
        if row is None:
            free = [r for r in range(self.MAX_SETS) if self._set_users[r] == 0 and r not in self._sets.values()] or \
                   [r for r in range(self.MAX_SETS) if self._set_users[r] == 0]
            if not free:
                raise RuntimeError(f"DecodePool: {self.MAX_SETS} different stop-id sets are live; wait for sequences to finish")
            row = free[0]
            for k in [k for k, v in self._sets.items() if v == row]:
                del self._sets[k]
            sv = torch.tensor([[len(stop_ids)] + list(stop_ids) + [0] * (self.MAX_STOP - len(stop_ids))], dtype=torch.int32)
            self.stop[row:row + 1].copy_(sv, non_blocking=True)
            self._keep.append(sv)
            self._sets[stop_ids] = row
        return row

    def _join_slots(self, slots, kcache, vtcache, seqs, deltas, first_tokens, max_new, set_row):
        B = len(slots)
        R = self.slot_rows
        state = torch.tensor(live_state_rows([s * R for s in slots], seqs, deltas, max_new, set_row), dtype=torch.int32)
        first = first_tokens.to(torch.int32).contiguous()
        self._keep += [state]
        if len(self._keep) > 64:
            del self._keep[:len(self._keep) - 64]
        # contiguous runs of slots: one relocate + one accept launch per run
        i = 0
        with ops.workspace_scope(self._ws_owner):
            while i < B:
                j = i
                while j + 1 < B and slots[j + 1] == slots[j] + 1:
                    j += 1
                a, n = slots[i], j - i + 1
                reloc = torch.tensor(reloc_rows(seqs[i:j + 1], [s * R for s in slots[i:j + 1]]), dtype=torch.int32)
                nr = reloc.shape[0]                      # <= 2 n: the run's entries live at rows [2 a, 2 a + nr) of the device table
                self._keep.append(reloc)
                self.reloc[2 * a:2 * a + nr].copy_(reloc, non_blocking=True)
                self.state[a:a + n].copy_(state[i:j + 1], non_blocking=True)
                ops.kv_relocate(kcache, self.dk, vtcache, self.dvt, self.reloc[2 * a:2 * a + nr], max(L for _, L, *_ in seqs[i:j + 1]))
                ops.decode_argmax_accept(None, first[i:j + 1], self.state[a:a + n], self.plan[a:a + n], self.ids[a:a + n],
                                         self.stop, self.done, per_sequence_sets=True)
                i = j + 1

    # ---- step ------------------------------------------------------------------------------------------------------------------
    def kv_bucket(self) -> int:
        need = max((self.bound[s] for s in self.live), default=1)
        return min(self.slot_rows, -(-need // self.KV_BUCKET) * self.KV_BUCKET)

    # Split-K planes + fused consumers for the few-tile projections (q/k/v: 80 output tiles, o: 64, down: 32 on 256 CUs): the GEMM writes
    # fp32 planes from >= 256 workgroups and the kernel that needs the result anyway sums them — q/k/v in the RoPE / cache-append kernel, o and
    # down in ONE kernel with the residual add and the NEXT RMSNorm (9 launches per layer instead of 11, none of them on a quarter of the chip).
    FUSED_SPLITK = True
    # gateup 0 = one GEMM with the SwiGLU epilogue (172 tiles of 128 x 128: 34 us); as 2 / 3 / 4 planes of 128 x 256 tiles + fo1_splitk_swiglu_bf16 it
    # measured 36 / 49 / 46 us (profiles/r04_pool_step_splitk_sweep.json) — the planes path stays available, parity-tested, unused
    SPLITS = dict(qkv=4, o=4, down=8, gateup=0)
    # TILED_WEIGHTS: gate/up and lm_head read a copy pre-tiled as [N / 128][K / 64][128][64] (ops.tile_weight, fo1_gemm_bf16_wtiled: a K tile is one
    # contiguous 16 KB block; 3.8 GB at the 3B shapes).  Bit-identical, and the weight stream ALONE gains 15 % that way (profiles/r04_hbm_stream_patterns.jsonl),
    # but the step does not: 3.872 vs 3.888 ms (profiles/r04_pool_step_tiled_weights_ab.json) — the activations on the same DMA path are what the tile waits for.  Off.
    TILED_WEIGHTS = False

    def _tiled(self):
        """(per-layer tiled gate/up copies, tiled lm_head) or None; built once per LLM, in DecodePool.__init__ (never inside a graph capture)."""
        if not self.TILED_WEIGHTS:
            return None
        t = self.llm.__dict__.get("_pool_tiled_w")          # on the LLM: every pool over these weights shares the copies
        if t is None:
            def tile(w):
                return ops.tile_weight(w) if (w.shape[0] % 128 == 0 and w.shape[1] % 64 == 0) else None
            with torch.inference_mode(False):
                t = ([tile(w["wgu"]) for w in self.llm.layers], tile(self.llm.lm_head))
            self.llm._pool_tiled_w = t
        return t

    def graph_key(self, bucket: int) -> tuple:
        """Key of the all-greedy step's graph (the general head's key is this plus a flag and the bitmap's identity)."""
        # (the step's form is part of the key: FUSED_SPLITK / SPLITS may be set per pool, scripts/pool_bench.py and the A/B test do)
        return (self.slot_rows, bucket, self.llm.rope_epoch, self.llm.rope_cos.data_ptr(), bool(self.FUSED_SPLITK), tuple(sorted(self.SPLITS.items())), bool(self.TILED_WEIGHTS))

    def step_key(self, bucket: int) -> tuple:
        """Key of the graph the coming step replays: graph_key(bucket), plus a flag and the buffers' identity per extra launch form."""
        key = self.graph_key(bucket)
        if self.n_general > 0:
            key += ("general", self.seen.data_ptr() if self.seen is not None else 0)
            if self.n_ruled > 0:      # (the ruled form reads the mask and rule tables and never writes them: nothing joins the rollback)
                key += ("ruled", self.masks.table.data_ptr(), self.rules.data_ptr())
            if self.n_guided > 0:     # (the guided form advances the slots' automaton states: gstate joins the rollback in step())
                key += ("guided", self.masks.table.data_ptr(), self.rules.data_ptr(), *self.gtab.pointers(), self.guides.data_ptr(), self.gstate.data_ptr())
            if self.n_closing > 0:    # (the closing form reads two more tables and writes neither: nothing more joins the rollback)
                key += ("closing", self.gtab.close_row.data_ptr(), self.closes.data_ptr())
            if self.n_steered > 0:    # (the steered form reads the bias table and the steers and counts the accepted tokens: the counts join the rollback)
                key += ("steered", self.btab.table.data_ptr(), self.steers.data_ptr(), self.counts.data_ptr() if self.counts is not None else 0)
        if self.n_logprob > 0:
            key += ("logprobs", self.lpb.lp.data_ptr())
        return key

    def _step_device(self, bucket: int, general: bool = False, record: bool = False):
        llm, P = self.llm, self.P
        c = llm.cfg
        H, KV, HD = c.num_heads, c.num_kv_heads, c.head_dim
        scale = 1.0 / math.sqrt(HD)
        st = self.state
        with ops.workspace_scope(self._ws_owner):
            x = ops.gather_rows(self.plan, c.hidden_size, llm.embed)
            if self.FUSED_SPLITK:
                eps, D = c.rms_norm_eps, c.hidden_size
                NGU = llm.layers[0]["wgu"].shape[0]
                part = torch.empty(max(self.SPLITS["qkv"] * (H + 2 * KV) * HD, max(self.SPLITS["o"], self.SPLITS["down"]) * D, self.SPLITS["gateup"] * NGU) * P, dtype=torch.float32,
                                   device=x.device)
                xn = ops.rmsnorm(x, llm.layers[0]["ln1"], eps)
                q = torch.empty(P, H * HD, dtype=torch.bfloat16, device=x.device)
                for li, w in enumerate(llm.layers):
                    s = ops.gemm_partials(xn, w["wqkv"], self.SPLITS["qkv"], part)
                    ops.pool_qkv_post_partials(part, s, w["bqkv"], q, H, KV, HD, llm.rope_cos, llm.rope_sin, st, self.dk[li], self.dvt[li])
                    att = ops.attention_decode_batch(q, self.dk[li], self.dvt[li], st, bucket, H, KV, HD, scale)
                    s = ops.gemm_partials(att, w["wo"], self.SPLITS["o"], part)
                    ops.splitk_residual_rmsnorm(part, s, x, w["ln2"], eps, x, xn)
                    if self.SPLITS["gateup"] >= 2:
                        s = ops.gemm_partials(xn, w["wgu"], self.SPLITS["gateup"], part)
                        a = ops.splitk_swiglu(part, s, P, NGU)
                    elif self._tiled() is not None and self._tiled()[0][li] is not None:
                        a = ops.gemm_wtiled(xn, self._tiled()[0][li], act=ops.ACT_SWIGLU16)
                    else:
                        a = ops.gemm(xn, w["wgu"], act=ops.ACT_SWIGLU16)
                    s = ops.gemm_partials(a, w["wdown"], self.SPLITS["down"], part)
                    ops.splitk_residual_rmsnorm(part, s, x, llm.layers[li + 1]["ln1"] if li + 1 < len(llm.layers) else llm.norm, eps, x, xn)
                logits = ops.gemm_wtiled(xn, self._tiled()[1]) if (self._tiled() is not None and self._tiled()[1] is not None) else ops.gemm(xn, llm.lm_head)
            else:
                for li, w in enumerate(llm.layers):
                    qkv = ops.gemm(ops.rmsnorm(x, w["ln1"], c.rms_norm_eps), w["wqkv"], w["bqkv"])
                    ops.pool_qkv_post(qkv, H, KV, HD, llm.rope_cos, llm.rope_sin, st, self.dk[li], self.dvt[li])
                    att = ops.attention_decode_batch(qkv[:, :H * HD], self.dk[li], self.dvt[li], st, bucket, H, KV, HD, scale)
                    x = ops.gemm(att, w["wo"], residual=x)
                    a = ops.gemm(ops.rmsnorm(x, w["ln2"], c.rms_norm_eps), w["wgu"], act=ops.ACT_SWIGLU16)
                    x = ops.gemm(a, w["wdown"], residual=x)
                logits = ops.gemm(ops.rmsnorm(x, llm.norm, c.rms_norm_eps), llm.lm_head)
            if general:      # plain slots ride as greedy rows without penalty; empty and finished slots return early, as in the greedy head
                rule = dict(masks=self.masks.table, rules=self.rules) if self.n_ruled > 0 or self.n_guided > 0 else {}
                if self.n_guided > 0:
                    rule["guide"] = self.gtab.operands(self.guides, self.gstate, self.closes if self.n_closing > 0 else None)
                if self.n_steered > 0:
                    rule["steer"] = ops.SteerOperands(self.steers, self.btab.table, self.btab.gate, self.counts, self.count_gate)
                ops.decode_head_accept(logits, self.sparams, st, self.plan, self.ids, self.stop, self.done, seen=self.seen, per_sequence_sets=True, **rule)
            else:
                ops.decode_argmax_accept(logits, None, st, self.plan, self.ids, self.stop, self.done, per_sequence_sets=True)
            if record:       # after the head, whichever it was; rows whose `want` is off, finished and empty slots return at once
                lb = self.lpb
                ops.decode_logprob_record(logits, lb.want, st, self.ids, lb.n_rec, lb.lp, lb.top_ids, lb.top_lp)
            return logits

    def step(self, use_graph: bool = True):
        """One token for every live sequence (all P rows are computed).  The head: fo1_decode_argmax_accept while every live slot is plain
        greedy, else the general head over all P rows (fo1_decode_head_accept); while a live slot asks for log-probabilities the record
        launch follows it (fo1_decode_logprob_record) — both counts change in join() and harvest() only, so a bucket has at most four
        graphs, and with both at zero the step is the all-greedy one under graph_key(bucket)."""
        bucket = self.kv_bucket()
        general = self.n_general > 0
        record = self.n_logprob > 0
        if not use_graph:
            out = self._step_device(bucket, general, record)
        else:
            # (ops.capture_graph: the warm-up step is rolled back; the K / V^T rows it appended are the ones the first replay rewrites
            # with the same values.  The warm-up of a general step also sets bits of the bitmap, that of a recording step writes the
            # record buffers: rolled back with the rest)
            key = self.step_key(bucket)
            roll = (self.state, self.plan, self.ids, self.done)
            if general and self.seen is not None:
                roll += (self.seen,)
            if general and self.n_guided > 0:      # or the first replay would start from the warm-up step's states, not the ones join() set
                roll += (self.gstate,)
            if general and self.n_steered > 0 and self.counts is not None:      # the warm-up step counted its picks
                roll += (self.counts, self.count_gate)
            if record:
                roll += self.lpb.written()
            ent = self._graphs.get(key)
            if ent is None:
                ent = self._graphs[key] = ops.capture_graph(lambda: self._step_device(bucket, general, record), rollback=roll)
            ops.replay_graph(ent[0])
            out = ent[1]
        self.steps_run += 1
        for s in self.live:
            self.bound[s] += 1
        return out

    # ---- leave -----------------------------------------------------------------------------------------------------------------
    def snapshot(self, pinned: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """Asynchronous copy of (state, generated ids) to pinned host memory on the current stream -> (state, ids, event, live slots)."""
        cols = min(self.IDS_CAP, max((self.budget[s] for s in self.live), default=1))
        if pinned is None or pinned[1].numel() < self.P * cols:
            pinned = (torch.empty(self.P, 8, dtype=torch.int32).pin_memory(), torch.empty(self.P * max(cols, 64), dtype=torch.int32).pin_memory())
        pinned[0].copy_(self.state, non_blocking=True)
        host_ids = pinned[1][:self.P * cols].view(self.P, cols)            # contiguous on both sides: a plain asynchronous memcpy
        host_ids.copy_(self.ids[:, :cols].contiguous(), non_blocking=True)
        recs = None
        if self.n_logprob > 0:      # the record tables ride along while a requesting slot is live (pinned beside the ids, same columns)
            T = ops.LOGPROB_TOP_MAX
            if len(pinned) < 5 or pinned[2].numel() < self.P * cols:
                n = self.P * max(cols, 64)
                pinned = (pinned[0], pinned[1], torch.empty(n, dtype=torch.float32).pin_memory(), torch.empty(n * T, dtype=torch.int32).pin_memory(),
                          torch.empty(n * T, dtype=torch.float32).pin_memory())
            lb = self.lpb
            recs = (pinned[2][:self.P * cols].view(self.P, cols), pinned[3][:self.P * cols * T].view(self.P, cols, T),
                    pinned[4][:self.P * cols * T].view(self.P, cols, T))
            for host, devt in zip(recs, (lb.lp, lb.top_ids, lb.top_lp)):
                host.copy_(devt[:, :cols].contiguous(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return pinned[0], host_ids, ev, dict(self.live), pinned, recs

    def harvest(self, snap, records: bool = False) -> List[tuple]:
        """Sequences that had finished when `snap` was taken (and have not been collected yet): [(slot, tag, ids)]; their slots are free again.
        records=True: [(slot, tag, ids, LogprobRecord or None)] — a requesting sequence's record, None for the others."""
        st, ids, ev, live_then = snap[:4]
        recs = snap[5] if len(snap) > 5 else None
        ev.synchronize()
        fin, ngen = st[:, 3].tolist(), st[:, 4].tolist()          # one host read of the pinned snapshot, not two per live slot
        out = []
        for s, tag in live_then.items():
            if s in self.live and self.live[s] is tag and fin[s] == 1:
                item = (s, tag, ids[s, :ngen[s]].tolist())
                if records:
                    item += (LogprobBuffers.record(*recs, s, ngen[s], self.lp_want[s]) if self.lp_want[s] >= 0 else None,)
                out.append(item)
                self.n_logprob -= self.lp_want[s] >= 0
                self.lp_want[s] = -1
                del self.live[s]
                self.free.append(s)
                self._set_users[self.slot_set[s]] -= 1
                self.n_general -= self.kind[s] != "plain"
                self.n_ruled -= bool(self.slot_masks[s])
                self._release_masks(s)
                self.n_guided -= self.slot_guide[s] is not None
                self._release_guide(s)
                self.n_closing -= self.slot_close[s]
                self.slot_close[s] = False
                self.n_steered -= self.slot_steer[s]
                self.slot_steer[s] = False
                self._release_bias(s)
        return out

    def drain(self, use_graph: bool = True, poll: int = 8, records: bool = False) -> List[tuple]:
        """Step until every live sequence has stopped (synchronous convenience for tests / one-shot callers); records: as harvest."""
        out = []
        while self.live:
            for _ in range(poll):
                self.step(use_graph)
            out += self.harvest(self.snapshot(), records=records)
        return out
