"""Seeded cases, the fp64 reference, the emulated kernel roundings and the tolerance of the prefill and window attention entries
(fo1_attention_bf16 on both MFMA forms, fo1_attention_prefix_bf16, fo1_attention_windows_bf16, fo1_attention_window_bias_bf16, the q_row_base
operand and the head-dim-32 window attention fo1_window_attention_bf16 / _map_bf16 / _map_var_bf16), shared by
tests/test_prefill_attention_cases.py (CPU: the tolerance can fail) and tests/test_prefill_attention_gpu.py (the route sweep on the MI355X).

A case lays out what its entry reads, in one logical row space: q [N][Hq][HD], k [N][KV][HD] and v [N][KV][HD] (bf16 values), from which
to_device() builds the entry's operands — separate Q / K rows, one fused q|k|v row (`packed`), the head-major rows of the ViT (`head_major`:
head h's q, k, v at h*256, h*256+HD, h*256+2*HD, so qk_head_stride = 256), the q/k/v GEMM rows of the head-dim-32 window attention, and
V^T [KV*HD][columns] for every entry that reads V transposed.  Rows N and N+1 are the map form's pad row (the q/k/v bias, read for a
window token outside the image) and a zero row (the `pad_zero` fault only).

A case is a list of units, each a set of queries with one key walk: a packed segment (its own causal or full range), a segment behind a
shared prefix (the prefix range walked first, in full), a window.  Segments and windows of the item routes lie GAP rows apart, so every key
range has a row on either side that belongs to none (the Swin and head-dim-32 windows are consecutive, as those entries require: a key leaked
there is a neighbour window's).  Planted data makes a wrong key range a gross error, not a statistical one:
  * queries share a direction per KV head: q = temp * (A u_kvh + z), z ~ N(0, 1);
  * planted keys: at each unit's first and last key and on both sides of every key-tile boundary of it (64 keys; 32 in win_attn32) a K row
    along u_kvh that scores about PLANT_SCORE for every query of the group, and a V row with a +-SPIKE in a position-specific dimension;
  * poison rows: every row outside all key ranges (so kv_start - 1, kv_end and both sides of every prefix range) scores higher still, and
    its V row is +-POISON — finite, as the decode module explains: the kernels read V^T in 4-key pieces next to zero weights;
  * the map form's pad row (non-zero) is a key along u of every head too, PAD_BELOW under a planted key: the padded tokens of a window weigh
    about as much as its planted keys together.
The remaining rows are N(0, 1); temperature 3 makes random scores of std ~3, so the running maximum moves between tiles.  Then every K row
moves by -SCORE_SHIFT along u_kvh: each query's scores all drop by the same amount (the softmax is unchanged), and a zero K row — what a
guarded load past a range reads — outscores every real key: a missing mask is a gross error too (fault zero_key).

emulate() is the kernels' arithmetic on the CPU, the same for every entry up to the key tile (attn_fwd_kernel, attention.hip:278-336;
attn_win1_kernel, one tile per item; attn_fwd32_kernel, whose per-lane partial row sums are only fp32 re-association; win_attn32_kernel,
window_attention.hip:125-163, with 32-key tiles): fp32 scores; a base-2 running maximum m = max(m, c1 * tile max) per key tile, tiles taken
from the prefix range's first key, then from the own range's first key (kv_start); e = exp2(c1 s - m) in fp32, P = bf16(e) into the PV
product, l = the fp32 sum of the unrounded e, output bf16(o / l).  c1 = scale * log2 e; with a bias (Swin) the score is
fp32(s * scale + bias) [- 100 across shift regions] and c1 = log2 e.

Tolerance: one bound per (query row, head): max|got - ref| <= TOL * max|ref row|, ref in float64 on the bf16 inputs.  The decode value
2^-6 does not hold here with half of it to spare: the emulation reaches 0.514 x 2^-6 (0.0080 of the row maximum, at davit_map-1x30x17-h6,
output row 271, head 1, window 3, temperature 1; 0.511 x 2^-6 at davit_var, 0.499 x 2^-6 at prefix16: rows whose +-16 value spikes
largely cancel, while the bf16 roundings of P do not).  So TOL is the next power of two, 2^-5: the emulation stays within 0.257 TOL
on every case here, and tests/test_prefill_attention_cases.py asserts at most TOL / 2.  That test also shows that every fault of
FAULTS that applies to a case moves some row of every unit it touches by at least 2 TOL."""
from dataclasses import dataclass, replace
from typing import List, Optional, Tuple

import torch

TOL = 2.0 ** -5
PLANT_SCORE = {1: 6.0, 3: 14.0}     # scaled score of a planted key, by q temperature
POISON_EXTRA = 8.0
SPIKE = 16.0
POISON = 64.0
PAD_BELOW = 3.0                     # the map form's pad row scores this much below a planted key (a window has up to 143 padded tokens)
A_DIR = 4.0                         # q = temp * (A_DIR u + z)
SCORE_SHIFT = 32.0                  # every K row (the pad row too) scores this much lower: a zero K row (a load past a range) dominates
GAP = 2                             # rows between the key ranges of the item routes
LOG2E = 1.4426950408889634
MAP_WS = 12                         # the map form's window side
SPARE = 64                          # device row buffers: finite rows past the last logical one


@dataclass
class Case:
    name: str
    route: str                           # fwd16 | fwd32 | prefix16 | prefix32 | win1 | swin | davit | davit_map | davit_var | rowbase
    Hq: int
    Hkv: int
    HD: int
    segs: Tuple[int, ...] = ()           # fwd / rowbase: segment lengths; win1: window lengths; davit: (tokens per window, windows)
    causal: bool = False
    q_block: int = 64
    packed: bool = False                 # Q / K (/ V) from one fused q|k|v row
    head_major: bool = False             # qk_head_stride 256 (ViT)
    temp: int = 1
    seed: int = 0
    prefix: Tuple[Tuple[int, Tuple[int, ...]], ...] = ()   # prefix routes: (prefix length, own segment lengths behind it); length 0: empty ranges
    ws: int = 0                          # swin: window side, shift, windows down / across, images stacked
    shift: int = 0
    nwy: int = 0
    nwx: int = 0
    images: int = 1
    sizes: Tuple[Tuple[int, int], ...] = ()   # davit_map / davit_var: image H x W (davit_map: all the same)
    row_base: int = 0                    # rowbase: *q_row_base (Q / O rows = query index - row_base)


@dataclass
class Unit:
    """Queries with one key walk.  qrows: logical q rows; qidx: their causal index; orows: output rows; keys: logical key rows in walk order;
    tile: walk-order tile of each key; own: the causal mask applies (the own range, not the prefix); kpos / qpos: position in the own range
    (window) — planted positions, the Swin bias and region index; win: the window's index inside its image (Swin regions)."""
    label: str
    qrows: torch.Tensor
    qidx: torch.Tensor
    orows: torch.Tensor
    keys: torch.Tensor
    tile: torch.Tensor
    own: torch.Tensor
    kpos: torch.Tensor
    qpos: torch.Tensor
    W: int
    n_own: int
    causal: bool = False
    win: int = 0
    prefix: Tuple[int, int] = (0, 0)     # the prefix range [start, end) walked first (empty: none)


def _seg_unit(label, s, e, W, causal, base=0, prefix=(0, 0)):
    own = torch.arange(s, e)
    pk = torch.arange(prefix[0], prefix[1]) if prefix[1] > prefix[0] else torch.zeros(0, dtype=torch.long)
    tp = -(-len(pk) // W)
    keys = torch.cat([pk, own])
    tile = torch.cat([(pk - prefix[0]) // W if len(pk) else pk, (own - s) // W + tp])
    return Unit(label, own, own, own - base, keys, tile, torch.cat([torch.zeros(len(pk), dtype=torch.bool), torch.ones(len(own), dtype=torch.bool)]),
                torch.cat([torch.full((len(pk),), -1), own - s]), own - s, W, e - s, causal, 0, tuple(prefix))


def swin_regions(ws: int, shift: int, nwy: int, nwx: int, boundary_delta: int = 0) -> torch.Tensor:
    """Region id of every token of every window [nwy*nwx, ws*ws]: BasicLayer.forward's img_mask over the padded Hp x Wp image, slices
    (0, -ws), (-ws, -shift), (-shift, None) along both axes, window-partitioned.  boundary_delta moves the Hp - shift boundary (a fault)."""
    Hp, Wp = nwy * ws, nwx * ws
    img = torch.zeros(Hp, Wp, dtype=torch.long)
    hb = Hp - shift + boundary_delta
    h_sl = (slice(0, Hp - ws), slice(Hp - ws, hb), slice(hb, None))
    w_sl = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
    cnt = 0
    for h in h_sl:
        for w in w_sl:
            img[h, w] = cnt
            cnt += 1
    return img.view(nwy, ws, nwx, ws).permute(0, 2, 1, 3).reshape(nwy * nwx, ws * ws)


def map_windows(sizes, row0s, ws=MAP_WS):
    """-> per window (image, window index, token rows [ws*ws] with -1 outside the image) of images stacked in raster order."""
    out = []
    for im, ((H, W), r0) in enumerate(zip(sizes, row0s)):
        nwy, nwx = -(-H // ws), -(-W // ws)
        for w in range(nwy * nwx):
            wy, wx = divmod(w, nwx)
            t = torch.arange(ws * ws)
            y, x = wy * ws + t // ws, wx * ws + t % ws
            rows = torch.where((y < H) & (x < W), r0 + y * W + x, torch.full_like(t, -1))
            out.append((im, w, rows))
    return out


def _layout(c: Case):
    """-> (N logical rows, units, segments for ops.make_items, prefix ranges per segment (prefix routes))."""
    units, segs, pref = [], [], []
    if c.route in ("fwd16", "fwd32", "win1", "rowbase"):
        W, pos = 64, c.row_base + GAP
        for i, L in enumerate(c.segs):
            units.append(_seg_unit(f"seg{i}[{pos},{pos + L})", pos, pos + L, W, c.causal, base=c.row_base))
            segs.append((pos, pos + L))
            pos += L + GAP
        return pos, units, segs, None
    if c.route in ("prefix16", "prefix32"):
        pos = GAP
        for gi, (P, owns) in enumerate(c.prefix):
            pr = (0, 0)
            if P:
                units.append(_seg_unit(f"prefix{gi}[{pos},{pos + P})", pos, pos + P, 64, c.causal))
                segs.append((pos, pos + P))
                pref.append((0, 0))
                pr = (pos, pos + P)
                pos += P + GAP
            for j, L in enumerate(owns):
                units.append(_seg_unit(f"own{gi}.{j}[{pos},{pos + L})+P{P}", pos, pos + L, 64, c.causal, prefix=pr))
                segs.append((pos, pos + L))
                # an empty second range in two spellings: (0, 0) and start >= end
                pref.append(pr if P else ((pos + 3, pos + 1) if j % 2 else (0, 0)))
                pos += L + GAP
        return pos, units, segs, pref
    if c.route == "swin":
        wl, nw = c.ws * c.ws, c.nwy * c.nwx
        for w in range(c.images * nw):
            u = _seg_unit(f"img{w // nw}.win{w % nw}", w * wl, (w + 1) * wl, 64, False)
            u.win = w % nw
            units.append(u)
            segs.append((w * wl, (w + 1) * wl))
        return c.images * nw * wl, units, segs, None
    if c.route == "davit":
        wt, nwin = c.segs
        for w in range(nwin):
            units.append(_seg_unit(f"win{w}", w * wt, (w + 1) * wt, 32, False))
        return wt * nwin, units, None, None
    if c.route in ("davit_map", "davit_var"):
        row0s, r = [], 0
        for H, W in c.sizes:
            row0s.append(r)
            r += H * W
        N = r
        for im, w, rows in map_windows(c.sizes, row0s):
            t = torch.arange(MAP_WS * MAP_WS)
            real = rows >= 0
            keys = torch.where(real, rows, torch.full_like(rows, N))      # row N = the pad row
            units.append(Unit(f"img{im}.win{w}", rows[real], rows[real], rows[real], keys, t // 32, torch.zeros(len(t), dtype=torch.bool),
                              t, t[real], 32, len(t), False, w))
        return N, units, None, None
    raise ValueError(c.route)


def planted_positions(n: int, W: int):
    pos = {0, n - 1}
    for t in range(W, n, W):
        pos.update((t - 1, t))
    return sorted(pos)


def _spike_dim(row: int, kvh: int, HD: int) -> int:
    return (37 * row + 53 * kvh) % HD


def build(c: Case) -> dict:
    """-> logical CPU tensors q/k/v [N + 2][heads][HD] (bf16 values in float), the Swin bias, the units, the entry's operands as CPU tensors
    (operands()) and its int32 item list (ops.make_items) with, on the prefix routes, the [items][2] prefix ranges."""
    N, units, segs, pref = _layout(c)
    g = torch.Generator().manual_seed(20261017 + c.seed)
    Hq, KV, HD = c.Hq, c.Hkv, c.HD
    G = Hq // KV
    scale = HD ** -0.5
    R = N + 2
    u = torch.randn(KV, HD, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    kvh_of = torch.arange(Hq) // G
    q = c.temp * (A_DIR * u[kvh_of].unsqueeze(0) + torch.randn(R, Hq, HD, generator=g))
    k = torch.randn(R, KV, HD, generator=g)
    v = torch.randn(R, KV, HD, generator=g)
    plant = PLANT_SCORE[c.temp]
    unit_k = u / (c.temp * A_DIR * scale)            # q . unit_k * scale ~ 1 for the group's queries
    sign = torch.tensor([1.0, -1.0]).repeat(HD // 2)
    in_range = torch.zeros(R, dtype=torch.bool)
    for un in units:
        own = un.keys[un.own] if c.route not in ("davit_map", "davit_var") else un.keys
        in_range[own[own < N]] = True
    if c.route in ("fwd16", "fwd32", "win1", "rowbase", "prefix16", "prefix32"):
        for r in torch.nonzero(~in_range[:N]).flatten().tolist():      # poison: every row outside all key ranges
            k[r] = unit_k * (plant + POISON_EXTRA)
            v[r] = POISON * sign
    for un in units:
        okeys = un.keys[un.own] if un.own.any() else un.keys
        opos = un.kpos[un.own] if un.own.any() else un.kpos
        for p in planted_positions(un.n_own, un.W):
            hit = torch.nonzero(opos == p).flatten()
            if not len(hit):
                continue
            r = int(okeys[hit[0]])
            if r >= N:                                   # a padded token: the pad row (planted below)
                continue
            k[r] = unit_k * plant
            v[r] *= 0.5
            for kvh in range(KV):
                v[r, kvh, _spike_dim(r, kvh, HD)] = SPIKE if (r + kvh) % 2 == 0 else -SPIKE
    if c.route in ("davit_map", "davit_var"):            # the pad row: a planted key of every head, e^-PAD_BELOW of a planted key's weight
        k[N] = unit_k * (plant - PAD_BELOW)
        v[N] *= 0.5
        for kvh in range(KV):
            v[N, kvh, (7 * kvh + 3) % HD] = SPIKE if kvh % 2 == 0 else -SPIKE
    k[:N + 1] -= SCORE_SHIFT * unit_k                    # every score of a query moves by the same amount: the softmax does not see it
    q[N + 1] = 0.0
    k[N + 1] = 0.0
    v[N + 1] = 0.0
    q, k, v = q.bfloat16().float(), k.bfloat16().float(), v.bfloat16().float()
    d = dict(case=c, N=N, units=units, segs=segs, prefix_ranges=pref, q=q, k=k, v=v, scale=scale, G=G)
    if c.route == "swin":
        wl = c.ws * c.ws
        d["bias"] = torch.randn(Hq, wl, wl, generator=g) * 1.5        # fp32, not symmetric, per head
        d["regions"] = swin_regions(c.ws, c.shift, c.nwy, c.nwx) if c.shift else None
    d["operands"] = operands(d)
    if segs is not None:
        from vlm_fo1_amd import ops
        d["items"] = ops.make_items(segs, "cpu", causal=c.causal, block=c.q_block)
        if pref is not None:
            # one row per item: the prefix range of the item's segment
            seg_of = {s: i for i, (s, _) in enumerate(segs)}
            d["items_prefix"] = torch.tensor([pref[seg_of[int(it[2])]] for it in d["items"]], dtype=torch.int32).reshape(-1, 2)
    return d


# ---- reference, faults, emulation ----------------------------------------------------------------------------------------------------

FAULTS = ("drop_first", "drop_last", "drop_tile_lo", "drop_tile_hi", "leak_after", "leak_before", "zero_key", "causal_ahead", "no_self", "head_map",
          "prefix_end+1", "prefix_end-1", "prefix_skip", "swin_no_mask", "swin_region_off", "bias_transposed", "bias_head", "pad_zero", "pad_drop",
          "row_base_off")


def applicable_faults(c: Case, d: dict) -> List[str]:
    out = ["drop_first", "drop_last", "zero_key"]
    if any(un.n_own > un.W for un in d["units"]):       # some range crosses a key-tile boundary
        out += ["drop_tile_lo", "drop_tile_hi"]
    if c.route in ("fwd16", "fwd32", "win1", "rowbase", "prefix16", "prefix32"):
        out.append("leak_before")
        if not c.causal:                     # (a causal range's kv_end lies past every query: the mask hides it)
            out.append("leak_after")
    if c.causal:
        out += ["causal_ahead", "no_self"]
    if c.Hq != c.Hkv:
        out.append("head_map")
    if c.route in ("prefix16", "prefix32"):
        out += ["prefix_end+1", "prefix_end-1", "prefix_skip"]
    if c.route == "swin":
        out += ["bias_transposed", "bias_head"]
        if c.shift:
            out += ["swin_no_mask", "swin_region_off"]
    if c.route in ("davit_map", "davit_var"):
        out += ["pad_zero", "pad_drop"]
    if c.route == "rowbase":
        out.append("row_base_off")
    return out


def _mutate(un: Unit, fault: Optional[str], d: dict) -> Tuple[Unit, dict]:
    """-> the unit as the faulty kernel would compute it, and per-unit options (head map, bias / mask changes)."""
    opt = {}
    if fault is None:
        return un, opt
    N = d["N"]
    if fault.startswith("drop_"):
        p = {"drop_first": 0, "drop_last": un.n_own - 1, "drop_tile_lo": un.W - 1, "drop_tile_hi": un.W}[fault]
        if p >= un.n_own:
            return un, opt
        keep = un.kpos != p
        if (un.keys[~keep] == N).all():      # a padded token (one of many copies of the pad row): pad_drop's business
            return un, opt
        return replace(un, keys=un.keys[keep], tile=un.tile[keep], own=un.own[keep], kpos=un.kpos[keep]), opt
    if fault in ("leak_after", "leak_before"):
        okeys = un.keys[un.kpos >= 0]
        r = int(okeys[-1]) + 1 if fault == "leak_after" else int(okeys[0]) - 1
        t = int(un.tile[-1]) if fault == "leak_after" else int(un.tile[un.kpos >= 0][0])
        kp = un.n_own if fault == "leak_after" else -2
        if fault == "leak_after":
            return replace(un, keys=torch.cat([un.keys, torch.tensor([r])]), tile=torch.cat([un.tile, torch.tensor([t])]),
                           own=torch.cat([un.own, torch.tensor([True])]), kpos=torch.cat([un.kpos, torch.tensor([kp])])), opt
        i = int(torch.nonzero(un.kpos >= 0)[0])
        cat = lambda a, x: torch.cat([a[:i], x, a[i:]])
        return replace(un, keys=cat(un.keys, torch.tensor([r])), tile=cat(un.tile, torch.tensor([t])), own=cat(un.own, torch.tensor([True])),
                       kpos=cat(un.kpos, torch.tensor([kp]))), opt
    if fault == "zero_key":        # one more key past the range with a zero K row and a zero V column, not masked
        return replace(un, keys=torch.cat([un.keys, torch.tensor([N + 1])]), tile=torch.cat([un.tile, un.tile[-1:]]),
                       own=torch.cat([un.own, torch.tensor([False])]), kpos=torch.cat([un.kpos, torch.tensor([un.n_own])])), opt
    if fault == "causal_ahead":
        return replace(un, qidx=un.qidx + 1), opt
    if fault == "no_self":
        return replace(un, qidx=un.qidx - 1), opt
    if fault == "head_map":
        KV = d["case"].Hkv
        opt["head_map"] = lambda h: h % KV
        return un, opt
    if fault.startswith("prefix_"):
        s, e = un.prefix
        if e <= s:
            return un, opt
        e2 = {"prefix_end+1": e + 1, "prefix_end-1": e - 1, "prefix_skip": s}[fault]
        pk = torch.arange(s, e2)
        own = un.kpos >= 0
        tp = -(-len(pk) // un.W)
        keys = torch.cat([pk, un.keys[own]])
        tile = torch.cat([(pk - s) // un.W, un.tile[own] - int(un.tile[own][0]) + tp])
        return replace(un, keys=keys, tile=tile, own=torch.cat([torch.zeros(len(pk), dtype=torch.bool), un.own[own]]),
                       kpos=torch.cat([torch.full((len(pk),), -1), un.kpos[own]]), prefix=(s, e2)), opt
    if fault in ("swin_no_mask", "swin_region_off", "bias_transposed", "bias_head"):
        opt[fault] = True
        return un, opt
    if fault == "pad_zero":
        return replace(un, keys=torch.where(un.keys == N, torch.full_like(un.keys, N + 1), un.keys)), opt
    if fault == "pad_drop":
        keep = un.keys != N
        return replace(un, keys=un.keys[keep], tile=un.tile[keep], own=un.own[keep], kpos=un.kpos[keep]), opt
    if fault == "row_base_off":
        # *q_row_base + 1: query index i reads Q row and writes O row i - base - 1, so O row j holds Q row j against keys <= j + base + 1;
        # the segment's last row is never written (NaN) and the row before its first is (the GPU test's NaN check)
        opt["last_row_nan"] = True
        return replace(un, qidx=un.qidx + 1), opt
    raise ValueError(fault)


def _swin_terms(d: dict, un: Unit, h: int, opt: dict):
    """-> (the fp32 bias [nq, nk] of head h, where the shift-region mask adds -100 [nq, nk] or None); (None, None) off Swin."""
    if "bias" not in d:
        return None, None
    c = d["case"]
    hb = (h + 1) % c.Hq if opt.get("bias_head") else h
    b = d["bias"][hb]
    if opt.get("bias_transposed"):
        b = b.t()
    kp = un.kpos.clamp(0, b.shape[1] - 1)      # (zero_key's extra key: the last position's bias)
    bias = b[un.qpos][:, kp]
    if not c.shift or opt.get("swin_no_mask"):
        return bias, None
    reg = swin_regions(c.ws, c.shift, c.nwy, c.nwx, -1) if opt.get("swin_region_off") else d["regions"]
    r = reg[un.win]
    return bias, r[un.qpos][:, None] != r[kp][None, :]


def _mask(un: Unit) -> torch.Tensor:
    """[nq, nk] True where the key is visible."""
    if not un.causal:
        return torch.ones(len(un.qrows), len(un.keys), dtype=torch.bool)
    return (~un.own)[None, :] | (un.keys[None, :] <= un.qidx[:, None])


def reference(d: dict, fault: Optional[str] = None) -> torch.Tensor:
    """fp64 softmax(q k^T * scale [+ bias + mask]) v per query row and head -> [output rows, Hq, HD], NaN on rows no unit writes."""
    c = d["case"]
    out = torch.full((_out_rows(d), c.Hq, c.HD), float("nan"), dtype=torch.float64)
    for un in d["units"]:
        m, opt = _mutate(un, fault, d)
        _ref_unit(d, m, opt, out)
    return out


def _out_rows(d: dict) -> int:
    return d["N"] - d["case"].row_base


def _ref_unit(d, un, opt, out):
    c = d["case"]
    hm = opt.get("head_map") or (lambda h: h // d["G"])
    mask = _mask(un)
    q, k, v = d["q"], d["k"], d["v"]
    for h in range(c.Hq):
        kvh = hm(h)
        s = (q[un.qrows, h].double() @ k[un.keys, kvh].double().t()) * d["scale"]
        bias, other_region = _swin_terms(d, un, h, opt)
        if bias is not None:
            s = s + bias.double()
        if other_region is not None:
            s = s - 100.0 * other_region.double()
        s = s.masked_fill(~mask, float("-inf"))
        p = torch.softmax(s, -1)
        o = p @ v[un.keys, kvh].double()
        o = torch.where(mask.any(-1, keepdim=True), o, torch.zeros_like(o))     # no visible key: zeros
        out[un.orows, h] = o
    if opt.get("last_row_nan"):
        out[un.orows[-1]] = float("nan")


def emulate(d: dict) -> torch.Tensor:
    """The kernels' roundings on the CPU (module docstring) -> bf16-valued float64 [output rows, Hq, HD], NaN on rows no unit writes."""
    c = d["case"]
    out = torch.full((_out_rows(d), c.Hq, c.HD), float("nan"), dtype=torch.float64)
    sc32 = torch.tensor(d["scale"], dtype=torch.float32)
    for un in d["units"]:
        mask = _mask(un)
        T = int(un.tile.max()) + 1
        tile = un.tile
        for h in range(c.Hq):
            kvh = h // d["G"]
            s = d["q"][un.qrows, h] @ d["k"][un.keys, kvh].t()                  # fp32
            bias, other_region = _swin_terms(d, un, h, {})
            if bias is not None:
                s = (s.double() * float(sc32) + bias.double()).float()         # fp32(s * scale + bias), one rounding (fma)
                if other_region is not None:
                    s = torch.where(other_region, s + torch.tensor(-100.0), s)
                c1 = torch.tensor(LOG2E, dtype=torch.float32)
            else:
                c1 = sc32 * torch.tensor(LOG2E, dtype=torch.float32)
            s = s.masked_fill(~mask, float("-inf"))
            nq = s.shape[0]
            mt = torch.full((nq, T), float("-inf")).scatter_reduce(1, tile.expand(nq, -1), s, "amax", include_self=True) * c1
            m = torch.cummax(mt, -1).values                                     # running maximum after each tile
            m_use = torch.where(m == float("-inf"), torch.zeros_like(m), m)
            mk = m_use.gather(1, tile.expand(nq, -1))
            e = torch.exp2((s.double() * float(c1) - mk.double()).float())     # exp2(fma(s, c1, -m))
            p = e.bfloat16().float()
            w = torch.exp2(m_use - m_use[:, -1:])                               # each tile's rescale to the final maximum
            l = (torch.zeros(nq, T).scatter_add(1, tile.expand(nq, -1), e) * w).sum(-1)
            o = (p * w.gather(1, tile.expand(nq, -1))) @ d["v"][un.keys, kvh]
            o = torch.where(l[:, None] > 0, o / l[:, None], torch.zeros_like(o))
            out[un.orows, h] = o.bfloat16().double()
    return out


def row_ratios(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """max|got - ref| / max|ref| per (row, head) -> [rows, Hq]; rows where ref is NaN give NaN, a NaN in got alone gives inf."""
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs().amax(-1)
    err = torch.where(torch.isnan(got).any(-1) & ~torch.isnan(ref).any(-1), torch.full_like(err, float("inf")), err)
    den = ref.abs().amax(-1)
    return torch.where(den > 0, err / den.clamp_min(1e-300), err * 1e300)


def check(buf: torch.Tensor, d: dict, what: str, ref: Optional[torch.Tensor] = None) -> float:
    """buf: the NaN-filled output buffer [output rows, >= Hq*HD] (pad columns included).  Asserts the per-row bound on every row a unit
    covers, and NaN on every other row and every pad column; -> the worst ratio / TOL."""
    c = d["case"]
    ref = reference(d) if ref is None else ref
    buf = buf.float().cpu()
    C = c.Hq * c.HD
    assert torch.isnan(buf[:, C:]).all(), f"{what}: a store landed in the pad columns (rows {torch.nonzero(~torch.isnan(buf[:, C:]).all(-1)).flatten()[:8].tolist()})"
    covered = ~torch.isnan(ref).any(-1).any(-1)
    stray = ~torch.isnan(buf[~covered, :C]).all(-1)
    assert not stray.any(), f"{what}: rows no item covers were written: {torch.nonzero(~covered).flatten()[stray][:8].tolist()}"
    got = buf[:, :C].reshape(-1, c.Hq, c.HD)
    unwritten = torch.isnan(got[covered]).any(-1).any(-1)
    assert not unwritten.any(), f"{what}: covered rows left unwritten (NaN): {torch.nonzero(covered).flatten()[unwritten][:8].tolist()}"
    r = row_ratios(got[covered], ref[covered])
    worst = r.max().item()
    i, h = divmod(int(r.argmax()), c.Hq)
    row = int(torch.nonzero(covered).flatten()[i])
    assert worst <= TOL, f"{what}: output row {row} head {h}: max|err| / max|ref| = {worst:.4g} > {TOL:.4g}"
    return worst / TOL


def unit_worst(mut: torch.Tensor, ref: torch.Tensor, un: Unit) -> Tuple[bool, float]:
    """-> (the fault changed the unit's rows at all, its worst row ratio / TOL)."""
    a, b = mut[un.orows], ref[un.orows]
    changed = bool((torch.isnan(a) != torch.isnan(b)).any() or (a[~torch.isnan(a)] != b[~torch.isnan(a)]).any())
    r = row_ratios(a, b)
    return changed, r.max().item() / TOL


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------

_LENS16 = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)
_LENS32 = (65, 191, 192, 193, 255, 256, 257, 511, 20)


def _sweep() -> List[Case]:
    cases, k = [], 0

    def add(route, name, **kw):
        nonlocal k
        kw.setdefault("temp", 1 if k % 2 == 0 else 3)
        cases.append(Case(f"{route}-{name}", route, seed=k, **kw))
        k += 1

    # 16x16 form (the GPU test launches q_block 16, 32 and 64 of each)
    add("fwd16", "hd128-16x2-causal-packed", Hq=16, Hkv=2, HD=128, segs=_LENS16 + (1100,), causal=True, packed=True)
    add("fwd16", "hd128-12x2-causal", Hq=12, Hkv=2, HD=128, segs=_LENS16, causal=True)
    add("fwd16", "hd128-4x4-causal", Hq=4, Hkv=4, HD=128, segs=_LENS16 + (1100,), causal=True)
    add("fwd16", "hd80-16x16-packed", Hq=16, Hkv=16, HD=80, segs=_LENS16 + (1100,), packed=True)
    add("fwd16", "hd80-16x16-headmajor", Hq=16, Hkv=16, HD=80, segs=_LENS16, head_major=True)
    add("fwd16", "hd32-8x8", Hq=8, Hkv=8, HD=32, segs=_LENS16 + (1030,), packed=True)
    # 32x32 form
    add("fwd32", "hd80-q256-16x16", Hq=16, Hkv=16, HD=80, segs=_LENS32, q_block=256, packed=True)
    add("fwd32", "hd80-q256-8x4", Hq=8, Hkv=4, HD=80, segs=_LENS32, q_block=256)
    add("fwd32", "hd128-q128-16x2-causal", Hq=16, Hkv=2, HD=128, segs=_LENS32, q_block=128, causal=True, packed=True)
    add("fwd32", "hd128-q256-4x4-causal", Hq=4, Hkv=4, HD=128, segs=_LENS32, q_block=256, causal=True)
    add("fwd32", "hd80-q256-vitfull-headmajor", Hq=16, Hkv=16, HD=80, segs=(1564, 300), q_block=256, head_major=True)
    # shared prefix: prefix lengths 1, 63, 64, 65, 284, 408 (and none) with own ranges 1, 64, 65, 252
    groups = ((1, (1, 64)), (63, (65,)), (64, (252,)), (0, (64, 1)), (65, (1, 65)), (284, (64, 252)), (408, (65, 1)), (0, (252,)))
    add("prefix16", "hd128-16x2-causal", Hq=16, Hkv=2, HD=128, prefix=groups, causal=True, q_block=64)
    add("prefix32", "hd128-16x2-causal", Hq=16, Hkv=2, HD=128, prefix=groups, causal=True, q_block=128)
    # single-tile windows (attn_win1, 4 items per workgroup)
    wl = (64, 1, 63, 4, 12, 64, 63, 1, 12)
    for i, n in enumerate((1, 2, 3, 5, 8, 9)):
        hm = i % 2 == 1
        add("win1", f"n{n}-" + ("headmajor" if hm else "packed"), Hq=16, Hkv=16, HD=80, segs=tuple(wl[(i + j) % len(wl)] for j in range(n)),
            packed=not hm, head_major=hm)
    # Swin windows with a bias (and the shifted-window mask)
    for ws, sh, nwy, nwx, imgs, H, qb in ((12, 0, 1, 1, 1, 6, 64), (12, 6, 1, 3, 1, 12, 64), (12, 6, 3, 2, 1, 6, 32), (12, 6, 2, 2, 2, 12, 64),
                                          (12, 6, 2, 2, 2, 6, 16), (7, 3, 3, 2, 1, 6, 16), (7, 0, 1, 3, 1, 12, 32), (7, 3, 1, 1, 2, 12, 64)):
        add("swin", f"ws{ws}-s{sh}-{nwy}x{nwx}" + (f"x{imgs}img" if imgs > 1 else "") + f"-h{H}-q{qb}", Hq=H, Hkv=H, HD=32, ws=ws, shift=sh,
            nwy=nwy, nwx=nwx, images=imgs, q_block=qb, packed=True)
    # DaViT window attention (head dim 32): partition form, map form, ragged map form
    for wt, nwin, H in ((1, 3, 8), (31, 3, 6), (32, 2, 32), (33, 3, 8), (37, 2, 6), (144, 3, 32), (160, 2, 8), (144, 2, 6)):
        add("davit", f"wtok{wt}-x{nwin}-h{H}", Hq=H, Hkv=H, HD=32, segs=(wt, nwin))
    add("davit_map", "2x13x25-h8", Hq=8, Hkv=8, HD=32, sizes=((13, 25), (13, 25)))
    add("davit_map", "1x30x17-h6", Hq=6, Hkv=6, HD=32, sizes=((30, 17),))
    add("davit_var", "40x30+13x25+7x5-h8", Hq=8, Hkv=8, HD=32, sizes=((40, 30), (13, 25), (7, 5)))
    # q_row_base (decode-graph form of fo1_attention_bf16): Q / O rows = query index - *q_row_base
    for base in (0, 1, 1000):
        add("rowbase", f"base{base}", Hq=16, Hkv=2, HD=128, segs=(1, 17, 64, 65, 130), causal=True, row_base=base)
    return cases


SWEEP = _sweep()


def scale_down(c: Case, cap: int = 1100) -> Case:
    """The same case with segments of at most `cap` rows (the CPU self-check keeps its run short)."""
    if not c.segs or c.route in ("davit",) or max(c.segs) <= cap:
        return c
    return replace(c, segs=tuple(min(n, cap) for n in c.segs), name=c.name + f"-cap{cap}")


def operands(d: dict, device="cpu") -> dict:
    """The entry's operands on `device`, laid out as the case says: q / k row views into one row buffer where packed or head-major (hs: the
    qk_head_stride, None = packed heads), V^T [KV*HD][columns]; for head dim 32 the q|k|v GEMM rows + the pad row; the Swin bias."""
    c = d["case"]
    N, Hq, KV, HD = d["N"], c.Hq, c.Hkv, c.HD
    # SPARE finite rows past the last one in every row buffer: the 32x32 form's K tile loads and the V^T pieces may reach past a range's end
    spare = torch.randn(SPARE, max(Hq, KV), HD, generator=torch.Generator().manual_seed(5))
    q, k, v = (torch.cat([t[:N], spare[:, :t.shape[1]]]).bfloat16() for t in (d["q"], d["k"], d["v"]))
    out = {}
    M = N + SPARE
    if c.route.startswith("davit"):
        C = Hq * HD
        out["qkv"] = torch.cat([q.reshape(M, C), k.reshape(M, C), v.reshape(M, C)], 1).contiguous().to(device)[:N]
        out["pad_row"] = torch.cat([d["q"][N], d["k"][N], d["v"][N]]).reshape(-1).bfloat16().contiguous().to(device)
        return out
    if c.head_major:
        assert Hq == KV
        rows = torch.zeros(M, Hq, 256, dtype=torch.bfloat16)
        rows[:, :, :HD], rows[:, :, HD:2 * HD], rows[:, :, 2 * HD:3 * HD] = q, k, v
        rows = rows.reshape(M, Hq * 256).to(device)[:N]
        out["q"], out["k"], out["hs"] = rows, rows[:, HD:], 256
    elif c.packed:
        rows = torch.cat([q.reshape(M, Hq * HD), k.reshape(M, KV * HD), v.reshape(M, KV * HD)], 1).contiguous().to(device)[:N]
        out["q"], out["k"], out["hs"] = rows[:, :Hq * HD], rows[:, Hq * HD:(Hq + KV) * HD], None
    else:
        out["q"], out["k"], out["hs"] = q.reshape(M, Hq * HD).contiguous().to(device)[:N], k.reshape(M, KV * HD).contiguous().to(device)[:N], None
    # V^T [KV*HD][columns]: 64 finite columns past the last row (the 4-key pieces and tiles the kernels read past a range)
    cols = (N + 64 + 7) // 8 * 8
    vt = torch.randn(KV * HD, cols, generator=torch.Generator().manual_seed(7)).bfloat16()
    vt[:, :N] = v[:N].permute(1, 2, 0).reshape(KV * HD, N)
    out["vt"] = vt.to(device)
    if "bias" in d:
        out["bias"] = d["bias"].contiguous().to(device)
    return out


def to_device(d: dict) -> dict:
    """operands() on cuda:0 (strides kept: the kernel reads what build() laid out)."""
    return operands(d, "cuda")


__all__ = ["TOL", "Case", "Unit", "SWEEP", "FAULTS", "build", "reference", "operands", "emulate", "check", "row_ratios", "unit_worst",
           "applicable_faults", "swin_regions", "map_windows", "planted_positions", "scale_down", "to_device"]
