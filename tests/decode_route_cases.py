"""LLM-only greedy-decode cases, the teacher-forced CPU oracle and the one logit bound shared by tests/test_decode_route_cases.py (CPU: the
bound can fail) and tests/test_decode_routes_gpu.py (every decode route of vlm_fo1_amd/llm.py on the MI355X).

Model: the shape tests/test_batched_decode_gpu.build() uses — hidden 2048, 16 query / 2 KV heads of 128, 2 layers, vocab 4096, the
embedding table x4 (tied lm_head: real top-1 margins) — from oracle.llm_oracle.random_llm_state on the CPU, so both tests hold the same
weights bit for bit.  The q and k rows of every layer's projection (weights and bias) are scaled by QK_SCALE = 1.5: with the std-0.02
weights alone the decode scores have a standard deviation below 1 and the softmax over hundreds of keys is flat, so a wrong key or position
reaches the logits diluted by the context length.  At x1.5 the largest attention weight of a (layer, head, decode step) of s40 / s250 /
s1000 is 32x uniform (1 / keys) at the median and at least 8x uniform in 93 % of them (x1: 7.6x and 46 %).  x2 peaks harder but doubles
the bf16 noise (0.38 against 0.23) for little gain in the faults' effect.

Inputs: seeded bf16 rows for the image block, text tokens from the embedding table, mRoPE positions from LO.rope_index (one image, so the
rope delta is non-zero); no vision towers.  SEQS lists the ragged sequences; the first four are the ones every route decodes:
  * "s40":   40 keys, <= 64 through the whole run;
  * "s250":  250 keys: crosses the pool's 256-key bucket (DecodePool.KV_BUCKET) during the decode steps;
  * "s1000": about a thousand keys;
  * "s2040": 2040 keys: crosses BatchDecoder.KV_BUCKET = 2048 at decode step 8, so that route changes its graph in mid-run.
then short fillers up to 32 sequences, and a pair over one image whose first PREFIX_ROWS rows are identical (the shared-prefix prefill,
relocated in two pieces).

Reference: LO.greedy_decode teacher-forced on a route's own ids (Oracle.logits: the same LO.llm_forward_cached calls, with the prefill cache
computed once per sequence and the steps memoised by id prefix, since most routes emit the same ids).

BOUND: one absolute bound on |route logit - oracle logit| for every route, calibrated on the CPU by tests/test_decode_route_cases.py (an
absolute bound: the bf16 noise does not follow the row's magnitude, which is ~15-20 on every row):
  * noise: `forward(..., bf16=True)` — the oracle with bf16 rounding at the engine's rounding points (normed rows, q/k/v after bias,
    RoPE output, P, attention output, every residual, SwiGLU, logits) — stays within BOUND / 2 of the fp32 oracle on every case;
  * sensitivity: each fault of FAULTS injected into the oracle's decode step moves some logit row by at least 2 x BOUND.
A float64 run of one case differs from the fp32 oracle by far less than BOUND."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from oracle import llm_oracle as LO

N_LAYERS, D, H, KV, HD, D_FF, VOCAB = 2, 2048, 16, 2, 128, 11008, 4096
EPS, THETA, SECTIONS = 1e-6, 1e6, (16, 24, 24)
KW = dict(n_layers=N_LAYERS, n_heads=H, n_kv=KV, head_dim=HD, eps=EPS, theta=THETA, sections=SECTIONS)
SEED = 31
EMBED_SCALE = 4.0
QK_SCALE = 1.5
STEPS = 12                   # ids per sequence: the prefill's pick + 11 decode steps
BOUND = 0.625                # absolute, on logit rows whose largest magnitude is ~15-20 (see the module docstring)
PREFIX_ROWS = 284            # rows the shared-prefix pair has in common (>= QwenLLM.SHARE_MIN_ROWS, a multiple of PACK_ALIGN)
FAULTS = ("rope_delta", "no_self", "drop_key", "neighbour", "stale_k")


@dataclass(frozen=True)
class Seq:
    name: str
    n_before: int
    grid: Tuple[int, int]      # merged image grid
    n_after: int
    seed: int
    image: int = -1            # image rows' seed (default: the sequence's own)
    text_seed: int = -1        # text ids' seed (default: the sequence's own)
    share_after: int = 0       # with text_seed: keep this many text-after ids of that seed, then the sequence's own

    @property
    def L(self) -> int:
        return self.n_before + self.grid[0] * self.grid[1] + self.n_after


KEY = [Seq("s40", 6, (4, 4), 18, 1), Seq("s250", 10, (12, 16), 48, 2), Seq("s1000", 14, (24, 32), 218, 3),
       Seq("s2040", 20, (40, 48), 100, 4)]
FILL = [Seq(f"f{i}", 3 + i % 7, (2 + i % 5, 3 + (i * 3) % 5), 6 + (i * 37) % 150, 100 + i) for i in range(28)]
SHARED = [Seq("shA", 8, (16, 16), 40, 200), Seq("shB", 8, (16, 16), 50, 201, image=200, text_seed=200, share_after=20)]
SEQS = KEY + FILL + SHARED
BY_NAME = {s.name: s for s in SEQS}


@functools.lru_cache(maxsize=1)
def state() -> Dict[str, torch.Tensor]:
    sd = LO.random_llm_state(N_LAYERS, D, H, KV, HD, D_FF, VOCAB, seed=SEED)
    sd["embed_tokens.weight"] = (sd["embed_tokens.weight"].float() * EMBED_SCALE).bfloat16()
    for i in range(N_LAYERS):
        for w in ("q_proj", "k_proj"):
            for p in ("weight", "bias"):
                k = f"layers.{i}.self_attn.{w}.{p}"
                sd[k] = (sd[k].float() * QK_SCALE).bfloat16()
    return sd


def _ids(seed: int, n: int) -> List[int]:
    return torch.randint(0, VOCAB, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


@functools.lru_cache(maxsize=None)
def prompt(name: str):
    """-> (text ids before the image, text ids after it, image rows bf16 [gh * gw, D])."""
    s = BY_NAME[name]
    ts = s.text_seed if s.text_seed >= 0 else s.seed
    before = _ids(7000 + ts, s.n_before)
    after = _ids(8000 + ts, s.share_after) + _ids(8000 + s.seed + 50000, s.n_after - s.share_after) if s.share_after else \
        _ids(8000 + ts, s.n_after)
    im = s.image if s.image >= 0 else s.seed
    n_img = s.grid[0] * s.grid[1]
    img = (torch.randn(n_img, D, generator=torch.Generator().manual_seed(9000 + im)) * 0.5).bfloat16()
    return before, after, img


def prompt_ids(name: str) -> List[int]:
    """The prompt as the engine's splice reads it: text ids and one <image> sentinel."""
    before, after, _ = prompt(name)
    return before + [LO.IMAGE_TOKEN_INDEX] + after


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """-> (embeddings bf16 [L, D], mRoPE positions [3, L], rope delta)."""
    s = BY_NAME[name]
    before, after, img = prompt(name)
    emb = state()["embed_tokens.weight"]
    x = torch.cat([emb[torch.tensor(before, dtype=torch.long)], img, emb[torch.tensor(after, dtype=torch.long)]], 0)
    pos, delta = LO.rope_index(s.n_before, s.grid, s.n_after)
    assert x.shape[0] == s.L and delta != 0
    return x, pos, delta


# ---- the oracle with rounding points and faults ---------------------------------------------------------------------------------------
def forward(x: torch.Tensor, pos: torch.Tensor, cache: Optional[list] = None, *, bf16: bool = False, dtype=torch.float32,
            fault: Optional[str] = None, key: int = 0, neighbour: Optional[list] = None, peaks: Optional[list] = None):
    """LO.llm_forward_cached restated with hooks: x [Ln, D] new rows at positions pos [3, Ln] after `cache` (per layer (K with RoPE, V)).
    bf16: round where the engine rounds.  dtype: float64 for the precision check.  fault (decode steps only, Ln = 1, every layer):
      rope_delta  the caller passes the position without the rope delta (nothing to do here);
      no_self     the new token's K/V row is missing from its own step's attention (it still lands in the cache);
      drop_key    past key `key` is dropped;
      neighbour   past key `key` reads K/V row `key` of another sequence's cache `neighbour`;
      stale_k     the previous step's K row is left at the current position (and stays in the cache).
    peaks: a list that collects the largest attention weight x keys of every head (decode steps).
    Returns (final-norm hidden [Ln, D] in `dtype`, new cache)."""
    sd = state()
    rb = (lambda t: t.bfloat16().to(dtype)) if bf16 else (lambda t: t)

    def W(n):
        return sd[n].to(dtype)

    def norm(v, w):
        return W(w) * (v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + EPS))

    Ln = x.shape[0]
    cos, sin = LO.mrope_cos_sin(pos, HD, THETA, SECTIONS)
    cos, sin = cos.bfloat16().to(dtype), sin.bfloat16().to(dtype)
    h = x.to(dtype)
    past = 0 if cache is None else cache[0][0].shape[0]
    mask = torch.arange(past + Ln)[None, :] <= torch.arange(past, past + Ln)[:, None]
    if fault is not None:
        assert Ln == 1 and past > 0, "faults are decode-step faults"
        if fault == "no_self":
            mask[0, past] = False
        elif fault == "drop_key":
            mask[0, key] = False
    rep = H // KV
    new_cache = []
    for i in range(N_LAYERS):
        p = f"layers.{i}."
        r = rb(norm(h, p + "input_layernorm.weight"))
        a = p + "self_attn."
        q = rb(r @ W(a + "q_proj.weight").t() + W(a + "q_proj.bias")).view(Ln, H, HD)
        k = rb(r @ W(a + "k_proj.weight").t() + W(a + "k_proj.bias")).view(Ln, KV, HD)
        v = rb(r @ W(a + "v_proj.weight").t() + W(a + "v_proj.bias")).view(Ln, KV, HD)
        q = rb(q * cos[:, None] + LO.rotate_half(q) * sin[:, None])
        k = rb(k * cos[:, None] + LO.rotate_half(k) * sin[:, None])
        if fault == "stale_k":
            k = cache[i][0][-1:].to(dtype)
        if cache is not None:
            k = torch.cat([cache[i][0].to(dtype), k], 0)
            v = torch.cat([cache[i][1].to(dtype), v], 0)
        new_cache.append((k, v))
        ka, va = k, v
        if fault == "neighbour":
            ka, va = k.clone(), v.clone()
            ka[key], va[key] = neighbour[i][0][key].to(dtype), neighbour[i][1][key].to(dtype)
        qg = q.view(Ln, KV, rep, HD)
        s = torch.einsum("qgrd,kgd->grqk", qg, ka) / math.sqrt(HD)
        s = s.masked_fill(~mask, float("-inf"))
        e = torch.exp(s - s.amax(-1, keepdim=True))
        if peaks is not None:
            peaks += (e.amax(-1) / e.sum(-1) * mask.sum()).flatten().tolist()
        o = torch.einsum("grqk,kgd->qgrd", rb(e), va) / e.sum(-1).permute(2, 0, 1)[..., None]
        o = rb(o.reshape(Ln, H * HD))
        h = rb(h + o @ W(a + "o_proj.weight").t())
        r = rb(norm(h, p + "post_attention_layernorm.weight"))
        g = rb(r @ W(p + "mlp.gate_proj.weight").t())
        u = rb(r @ W(p + "mlp.up_proj.weight").t())
        h = rb(h + rb(rb(torch.nn.functional.silu(g)) * u) @ W(p + "mlp.down_proj.weight").t())
    return rb(norm(h, "norm.weight")), new_cache


def head(hid: torch.Tensor, bf16: bool = False) -> torch.Tensor:
    lg = hid[-1] @ state()["embed_tokens.weight"].to(hid.dtype).t()
    return lg.bfloat16().to(hid.dtype) if bf16 else lg


def run(name: str, ids: Sequence[int], *, bf16: bool = False, dtype=torch.float32, fault: Optional[str] = None, key: int = 0,
        neighbour: Optional[str] = None, prefill: Optional[tuple] = None, peaks: Optional[list] = None) -> torch.Tensor:
    """forward() teacher-forced on `ids` -> logits [len(ids), VOCAB] in `dtype` (row t: after ids[:t]).  `prefill`: a (hidden, cache) of
    this sequence's prompt from an earlier forward() call with the same bf16 / dtype; the fault applies to every decode step."""
    x, pos, delta = inputs(name)
    hid, cache = prefill if prefill is not None else forward(x, pos, None, bf16=bf16, dtype=dtype)
    nb = Oracle.get().prefill(neighbour)[1] if neighbour is not None else None
    emb = state()["embed_tokens.weight"]
    out = [head(hid, bf16)]
    for t in ids[:-1]:
        n = cache[0][0].shape[0]
        p = n + (0 if fault == "rope_delta" else delta)
        kk = (n - 1 if key < 0 else key) if fault in ("drop_key", "neighbour") else 0
        hid, cache = forward(emb[t:t + 1], torch.full((3, 1), p, dtype=torch.long), cache, bf16=bf16, dtype=dtype,
                             fault=None if fault == "rope_delta" else fault, key=kk, neighbour=nb, peaks=peaks)
        out.append(head(hid, bf16))
    return torch.stack(out)


class Oracle:
    """LO.greedy_decode(sd, embeds, pos, delta, n, forced=ids) of every sequence, memoised: the prefill cache once per sequence, each
    teacher-forced step once per id prefix."""
    _one: Optional["Oracle"] = None

    @classmethod
    def get(cls) -> "Oracle":
        if cls._one is None:
            cls._one = cls()
        return cls._one

    def __init__(self):
        self._pre: Dict[str, tuple] = {}
        self._memo: Dict[tuple, tuple] = {}

    def prefill(self, name: str):
        """-> (final-norm hidden of the last row [1, D], cache) of LO.llm_forward_cached over the prompt."""
        if name not in self._pre:
            x, pos, _ = inputs(name)
            hid, cache = LO.llm_forward_cached(state(), x, pos, None, **KW)
            self._pre[name] = (hid[-1:], cache)
        return self._pre[name]

    def logits(self, name: str, ids: Sequence[int]) -> torch.Tensor:
        """fp32 oracle logits [len(ids), VOCAB] teacher-forced on ids (row 0 from the prefill)."""
        sd = state()
        headw = sd["embed_tokens.weight"].float()
        _, _, delta = inputs(name)
        last, cache = self.prefill(name)
        rows = [(last @ headw.t())[0]]
        for t in range(1, len(ids)):
            k = (name, tuple(int(i) for i in ids[:t]))
            hit = self._memo.get(k)
            if hit is None:
                fed = int(ids[t - 1])
                p = cache[0][0].shape[0] + delta
                last, cache = LO.llm_forward_cached(sd, sd["embed_tokens.weight"][fed:fed + 1].float(), torch.full((3, 1), p, dtype=torch.long),
                                                    cache, **KW)
                hit = self._memo[k] = ((last @ headw.t())[0], cache)
            rows.append(hit[0])
            cache = hit[1]
        return torch.stack(rows)

    def greedy(self, name: str, n: int = STEPS) -> List[int]:
        """The oracle's own greedy ids."""
        ids: List[int] = []
        for _ in range(n):
            ids.append(int(self.logits(name, ids + [0])[-1].argmax()))
        return ids


def margin(row: torch.Tensor) -> float:
    top = row.float().topk(2).values
    return float(top[0] - top[1])


def peak_stats(names: Sequence[str]) -> Tuple[float, float]:
    """Largest attention weight x keys of every (layer, head, decode step) along the oracle's greedy ids -> (median, fraction >= 8)."""
    vals: List[float] = []
    for name in names:
        run(name, Oracle.get().greedy(name), prefill=Oracle.get().prefill(name), peaks=vals)
    v = torch.tensor(vals)
    return float(v.median()), float((v >= 8).float().mean())
