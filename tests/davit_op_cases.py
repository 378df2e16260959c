"""Cases, fp64 references, bounds, emulated kernel arithmetic and faults of the two DaViT kernel families of vlm_fo1_amd/csrc/vision_ops.hip that
had no test against an independent reference: channel attention (chattn_gram[_mfma]_kernel, chattn_softmax_kernel, chattn_apply[_mfma]_kernel behind
fo1_channel_attention_bf16 / fo1_channel_attention_var_bf16) and the depthwise 3x3 conv (dwconv3x3_kernel, dwconv3x3_ln_kernel<PPW>,
dwconv3x3_ln_run_kernel<PPW, NCH, RUN> behind fo1_dwconv3x3_bf16 / fo1_dwconv3x3_ln_bf16 / fo1_dwconv3x3_ln_var_bf16).  Shared by
tests/test_davit_op_cases.py (CPU) and tests/test_davit_ops_gpu.py (the MI355X sweep).  Helpers, the canary pattern and the LayerNorm bound come
from tests/small_op_cases.py.

Restated host code.  ca_layout() is the workspace of channel_attention(): part[image][chunk slot][G][32][32] fp32, then A[image][G][32][32] fp32 holding
bf16 values, cdiv(N_largest, 256) slots per image; the CPU test compares its size with fo1_channel_attention[_var]_workspace_bytes and CA_TOK, DW_RUN,
DW_LN_CHUNKS and the apply kernel's NB with the constants in vision_ops.hip.  ca_grids() restates the three launches, dwln_form() / dw_ppw() /
dw_run_template() the choice between dwconv3x3_ln_kernel<PPW> and dwconv3x3_ln_run_kernel<PPW, NCH, RUN>.  Routes are restated only: FO1_LAUNCH records
"chattn_gram" / "chattn_apply" / "dwconv3x3_ln" for every form, so the profile rows cannot tell them apart; the GPU test selects a form with
fo1_channel_attention_set_impl and fo1_dwconv_ln_set_form, and the CPU test asserts that the product rule (setting 1) keeps every case here on the
per-pixel form, that setting 2 gives <4,1,8>, <2,1,8>, <1,1,8>, <1,2,4> at C = 128, 256, 512, 1024 and nothing elsewhere.

Channel attention, one bound per kernel (the GPU test owns the workspace, so it sees all three results of a launch):
  * Gram: every live chunk slot against the float64 sum over exactly that chunk's tokens, F32_EPS n sum |q||k| per element (products of bf16 values are exact in
    fp32, only the additions round: format, any order).  Slots past an image's own chunk count keep the 1e30 the workspace was filled with.
  * matrix: A against float64 softmax(S), S = Gram N_i^-0.5 unrounded.  ca_matrix_bound(): half a bf16 ulp of S through the softmax slope, exact not linearised;
    half a bf16 ulp of A; and the measured term for expf and the fp32 sums in its two places: SUM_REL N^-0.5 sum |q||k| on the logit before its rounding (the token
    and chunk sums and the scale; it matters where it tips a logit over a rounding tie) and MAT_REL |A| after it (expf, the 32-term sum, the division).  Both are
    relative because those errors are: an absolute term would swamp the half ulp of the small entries.  No worst-case format term for the sums: N roundings of
    F32_EPS each would double the bound at the 5- and 9-chunk cases, which exist for the 4-way unrolled sum and its tail.
  * output: against float64 A_dev v with the matrix the same launch produced: 32 F32_EPS sum |A||v| plus half a bf16 ulp.  The softmax's rounding flips stay out.
  * end to end: against the unrounded float64 chain, per (token, group) row as a fraction of the row's max |ref|, E2E.
The emulation is within HALF of the measured terms (MAT_REL / 2, SUM_REL / 2, E2E / 2) and of the Gram bound; the format terms stay whole, because half an ulp is
the exact worst case of round-to-nearest and these inputs meet it (matrix 0.944, output 0.999 of the bound).  No element and no row gets a rare-fraction allowance.

Channel-attention inputs.  Background N(0, 1), q at temperature TEMPS[(c + g) % 2] per q channel.  Planted tokens (ca_planted: first and last of every image, both sides
of every 64-token tile boundary and so of every 256-token chunk boundary, the last token of every 32- and so every 128-token apply block) have q = k = 0 except one
(c, c') pair per group that puts LOGITS[j % 4] on an entry particular to the position, the group and the image; the pairs sit on the TEMPS[0] rows only, so the other
rows stay nearly flat, and j -> entry is one to one (asserted).  max |S| is 4.70 (logits above 4 cost half a bf16 ulp of 2^-6 on S, which is what E2E mostly is).  Every
qkv row of no image (CA_LEAD = 3 before the first, uniform cases included: that entry is handed the address of row 3; between ragged images; 4 after the last) holds
2^40 in q, k and v; in a uniform batch the rows next to an image are its neighbours' planted first / last tokens.  Cases: C = 32 / 96 / 160 / 256 (G = 1, 3, 5, 8) x N of CA_N up to 300, N = 513 / 1025 / 2100 at C = 32 (2, 3, 5, 9 chunks), batch 3 at
five N, three ragged tables (largest not first, a 1-token image, fewer chunks than the largest, equal sizes, in_row0 with gaps of 0 / 1 / 2 rows after 3 leading ones).

Depthwise conv.  y against float64 x + conv(x) + bias: half a bf16 ulp of the conv value from its own binade, half a bf16 ulp of y, 10 F32_EPS (|bias| + sum |x||w|).
h against the float64 LayerNorm of the y the same launch returned, with small_op_cases' layernorm reference, bound (REL["layernorm"]) and emulation, reached by
handing y to them as a rownorm case.  Inputs: 4 x grid_values + 32 b for image b, the top / bottom rows and left / right columns shifted by +96 / -80 / +112 / -104, the
last chunk's weights zero and chunk 1's bias +-0 (C >= 24), 2^40 in every x row of no image, canary in every such row of y and h and in DW_SPARE rows after the last
pixel.  Every width of every route runs all eight shapes of DW_SHAPES at batch 1 and 3, and every fused width two ragged tables of three different sizes (asserted
per route and width).  The separate kernel has no ragged entry.

Faults are one-line mutations of the emulation; the CPU test shows that each breaks the bound of the stage it belongs to by at least 2 x in EVERY unit it touches
(Gram: image x chunk x group; matrix and output: image x group; dwconv: image) and that it touches every unit ca_fault_applies / dw_fault_applies names.  "A token >= N
stored" and "a short run's last pixels stored into the next row" write rows of no image: the canary.  Two faults move the result towards the reference and are bitwise
(they must change bits of the emulation): logits not rounded before the exponential (test_unrounded_logits_stay_inside_the_matrix_bound shows it cannot leave the
bound), and LayerNorm fed the fp32 conv value.  "Residual taken from the rounded conv" is read as y = bf16(conv) without x; "chunk sub + LPP read for chunk sub" as every
chunk c with c + LPP < chunks computed from chunk c + LPP's x, weights and bias (C = 768, 1024, 1536, 2048).

Not covered: the FMA apply kernel's grid-stride loop (it starts above 131072 tokens), maps over 2 GiB (dwln_form's first test is restated and checked at the limit, no
case runs it), the product rule's switch to the run form at 4096 waves (restated and checked at the threshold only).

RESULTS_CPU (tests/test_davit_op_cases.py -s; 86 + 334 cases, 33 s):
  fp32 softmax chain against float64 on the same bf16 logits, worst relative error 2.355e-7 -> MAT_REL = 2^-20 (4 x is 9.42e-7, 1.2 % under 2^-20: re-measure when a
  seed or a case changes, as small_op_cases prescribes).  fp32 logit before its rounding against the float64 S, worst 2.957e-7 of N^-0.5 sum |q||k| -> SUM_REL = 2^-19
  (4 x is 1.18e-6); with it the matrix bound is at the 5- and 9-chunk cases at most 1.012 x what it is without any term for those sums (1.37 x at one
  element of C = 96, N = 31, whose logit lies within the term of a power of two and so takes the upper binade's half ulp).  Emulation end
  to end 0.0214 of the row maximum -> E2E = 2^-4 (the power of two at or above 2 x).  Emulation: Gram 0.089 of its bound, matrix 0.944 (MAT_REL / 2, SUM_REL / 2),
  output 0.999, dwconv y 1.000, h 1.000 of the quarter bound.
  Weakest faults, channel attention: swapped apply halves 2.43 x (C = 160, N = 1: one token, whose two halves of a flat row differ little), scale of the largest image
  22.3 x, image 0's matrices 23.2 x, A transposed 69.7 x, softmax axis 89.8 x, chunk count of the largest 96.7 x, group g - 4 in the apply 341 x, every Gram fault beyond
  1.7e4 x.  Depthwise conv: bias dropped 14.8 x, tap across an image boundary 37.1 x, every other beyond 240 x.
RESULTS_GPU (MI355X, tests/test_davit_ops_gpu.py -s: 508 passed in 4.4 s, wall time 2.4 s for 506 checked launches; every canary intact, every input unchanged, every
second launch bit-identical, no kernel defect found).  Worst fraction of the bound per op and route (end to end: of the row maximum, tolerance 0.0625):
  chattn mfma uniform  Gram 0.048  matrix 0.935  output 0.999  end to end 0.0214        chattn mfma ragged  Gram 0.045  matrix 0.944  output 0.999  end to end 0.0184
  chattn fma  uniform  Gram 0.089  matrix 0.935  output 0.999  end to end 0.0214        chattn fma  ragged  Gram 0.057  matrix 0.944  output 0.999  end to end 0.0184
  (matrix at N = 513 / 1025 / 2100 and the tables with 5 and 9 chunks: 0.874 - 0.901 on both routes)
  dwconv separate y 1.000; per-pixel <4>, <2>, <1> and run <4,1,8>, <2,1,8>, <1,1,8>, <1,2,4>, uniform and ragged each: y 1.000, h 0.998 - 1.000.
  A bf16 output at 0.999 - 1.000 of its bound is an element next to a rounding tie, as in small_op_cases."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

import small_op_cases as S
from small_op_cases import BF, CANARY_BF, CANARY_F32, F32_EPS, LN_EPS, Case, _gen, _xor_tree, grid_values, half_ulp, rb, worst_ratio  # noqa: F401

# ---------------------------------------------------------------------------------------------------------------------------------------
# channel attention
# ---------------------------------------------------------------------------------------------------------------------------------------
CA_TOK = 256            # kCaTok: tokens per partial-Gram chunk
CA_TILE = 64            # tokens per staged tile of the Gram kernels
CA_BLOCK = 128          # tokens per wave of chattn_apply_mfma_kernel (NB = 4 blocks of 32)
FILL = 1e30             # what the workspace holds before every launch: a slot read without having been written gives a gross error
POISON = 2.0 ** 40      # q, k and v of every qkv row that belongs to no image (finite, and so are its products)
MAT_REL = 2.0 ** -20    # expf, the 32-term fp32 sum and the division of the softmax kernel, relative to A (measure(): 4 x the chain's worst, rounded up to a power of two)
SUM_REL = 2.0 ** -19    # the fp32 token and chunk sums and the scale, on the logit, relative to N^-0.5 sum |q||k| (measure(): 4 x the emulation's worst, rounded up likewise)
E2E = 2.0 ** -4         # end to end, per (token, group) row, as a fraction of the row's max |ref| (measure(): 2 x the emulation's worst)
CA_LEAD = 3             # poison rows before the first image of every case: the uniform entry is handed the address of row CA_LEAD
CA_C = (32, 96, 160, 256)
CA_N = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513, 1025, 2100)
CA_ROUTES = ("mfma", "fma")
TEMPS = (0.5, 0.25)     # q temperatures: peaked and nearly flat softmax rows, alternating over the q channels of every group
LOGITS = (3.0, 2.5, -3.0, 2.0)


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def ca_layout(n_img: int, n_largest: int, C: int) -> dict:
    """The workspace of channel_attention() (vision_ops.hip, `float* part = (float*)workspace; float* A = part + n * chunks * G * 1024` and
    fo1_channel_attention_workspace_bytes): part[image][chunk slot][G][32][32] fp32, then A[image][G][32][32] fp32 holding bf16 values; the
    slot count is that of the LARGEST image."""
    G, slots = C // 32, cdiv(n_largest, CA_TOK)
    part = n_img * slots * G * 1024
    return dict(G=G, slots=slots, part_floats=part, a_floats=n_img * G * 1024, bytes=4 * (part + n_img * G * 1024))


def ca_grids(route: str, n_largest: int, C: int, n_img: int) -> dict:
    """The three launches of channel_attention() (restated only: the profile rows carry one name for both forms)."""
    G, slots = C // 32, cdiv(n_largest, CA_TOK)
    if route == "mfma":
        return dict(gram=(slots, cdiv(G, 4), n_img), softmax=(G, n_img), apply=(cdiv(n_largest, CA_BLOCK), cdiv(G, 4), n_img))
    return dict(gram=(slots, G, n_img), softmax=(G, n_img), apply=(min(cdiv(n_largest, 256), 512), G, n_img))


def _ca_cases() -> List[Case]:
    out = []
    for C in CA_C:
        for N in CA_N:
            if N > 300 and C != 32:
                continue
            out.append(Case("chattn", f"ca-c{C}-n{N}", C=C, sizes=(N,), rows=(CA_LEAD,), ragged=False))
        for N in (1, 65, 129, 257, 300) + ((513,) if C == 32 else ()):
            out.append(Case("chattn", f"ca-c{C}-n{N}-b3", C=C, sizes=(N,) * 3, rows=(CA_LEAD, CA_LEAD + N, CA_LEAD + 2 * N), ragged=False))
    tables = {"t1": (33, 300, 1, 257, 257), "t2": (64, 1025, 256, 513, 1025), "t3": (129, 2100, 31)}
    for C in CA_C:
        for name, sizes in tables.items():
            if name != "t1" and C != 32:
                continue
            rows, r = [], CA_LEAD                           # in_row0 with gaps: 3 poison rows first, 0 / 1 / 2 between the images
            for i, n in enumerate(sizes):
                rows.append(r)
                r += n + i % 3
            out.append(Case("chattn", f"ca-c{C}-{name}-ragged", C=C, sizes=sizes, rows=tuple(rows), ragged=True))
    return out


def ca_planted(N: int) -> List[int]:
    """First and last token, both sides of every 64-token tile boundary (every 256-token chunk boundary is one), the last token of every 32-token
    apply block (every 128-token one is one)."""
    p = {0, N - 1}
    p.update(t for t in range(CA_TILE, N, CA_TILE))
    p.update(t - 1 for t in range(32, N + 1, 32))
    return sorted(p)


def ca_total_rows(c: Case) -> int:
    return c.rows[-1] + c.sizes[-1] + 4                    # spare poison rows after the last image


def _ca_build(c: Case) -> dict:
    C, G = c.C, c.C // 32
    R = ca_total_rows(c)
    g = _gen(C, sum(c.sizes), len(c.sizes), 3)
    qkv = torch.full((R, 3 * C), POISON)
    temp = torch.tensor([TEMPS[(ch + ch // 32) % 2] for ch in range(C)])
    for z, (N, r0) in enumerate(zip(c.sizes, c.rows)):
        x = torch.randn(N, 3 * C, generator=g)
        x[:, :C] *= temp
        pl = ca_planted(N)
        assert len(pl) <= 512
        amp_scale = math.sqrt(math.sqrt(N))
        for j, p in enumerate(pl):
            x[p, :2 * C] = 0.0
            L = LOGITS[j % 4]
            a = math.sqrt(abs(L)) * amp_scale
            for gi in range(G):
                # 37 is odd: j -> e is one to one below 512, no two planted entries of a group collide.  Only the q channels at temperature
                # TEMPS[0] take planted entries ((c + g) even): the others keep nearly flat softmax rows
                e = (j * 37 + gi * 101 + z * 17 + 1) % 512
                x[p, gi * 32 + 2 * (e // 32) + gi % 2] = a
                x[p, C + gi * 32 + e % 32] = math.copysign(a, L)
        qkv[r0:r0 + N] = x
    return dict(qkv=qkv.to(BF))


def ca_images(c: Case):
    """-> per image (q, k, v) as float64 [N, G, 32]."""
    qkv, C, G = inputs(c)["qkv"].double(), c.C, c.C // 32
    return [tuple(qkv[r0:r0 + N, i * C:(i + 1) * C].reshape(N, G, 32) for i in range(3)) for N, r0 in zip(c.sizes, c.rows)]


_REF: Dict[str, dict] = {}


def ca_reference(c: Case) -> dict:
    """float64, nothing rounded: per image the Gram of every live chunk (gram, NaN in dead slots), sum |q||k| of it (gram_abs), its token count
    (ntok), S = Gram N^-0.5, A = softmax over the k channel, out = A v; s_abs = N^-0.5 sum over all tokens of |q||k|."""
    if c.name in _REF:
        return _REF[c.name]
    lay = ca_layout(len(c.sizes), max(c.sizes), c.C)
    G, slots = lay["G"], lay["slots"]
    gram = torch.full((len(c.sizes), slots, G, 32, 32), float("nan"), dtype=torch.float64)
    gabs, ntok = torch.zeros_like(gram), torch.zeros(len(c.sizes), slots)
    Ss, As, outs, sabs = [], [], [], []
    for z, (q, k, v) in enumerate(ca_images(c)):
        N = q.shape[0]
        for s in range(cdiv(N, CA_TOK)):
            a, b = s * CA_TOK, min(N, (s + 1) * CA_TOK)
            gram[z, s] = torch.einsum("ngc,ngd->gcd", q[a:b], k[a:b])
            gabs[z, s] = torch.einsum("ngc,ngd->gcd", q[a:b].abs(), k[a:b].abs())
            ntok[z, s] = b - a
        Sm = torch.einsum("ngc,ngd->gcd", q, k) / math.sqrt(N)
        A = torch.softmax(Sm, dim=-1)
        Ss.append(Sm), As.append(A), outs.append(torch.einsum("gcd,ngd->ngc", A, v))
        sabs.append(torch.einsum("ngc,ngd->gcd", q.abs(), k.abs()) / math.sqrt(N))
    _REF[c.name] = dict(gram=gram, gram_abs=gabs, ntok=ntok, S=Ss, A=As, out=outs, s_abs=sabs)
    return _REF[c.name]


def ca_gram_bound(c: Case) -> torch.Tensor:
    """F32_EPS n sum |q||k|: products of bf16 values are exact in fp32, only the n additions round (format bound, any order)."""
    r = ca_reference(c)
    return F32_EPS * r["ntok"][:, :, None, None, None].double() * r["gram_abs"]


def ca_matrix_bound(c: Case, z: int, mat_rel: float = MAT_REL, sum_rel: float = SUM_REL) -> torch.Tensor:
    """|A - softmax(S)|.  The logit the kernel exponentiates is bf16(fp32 sum x fp32 scale): off by e = half a bf16 ulp of S plus the fp32 sums'
    own error, the measured sum_rel N^-0.5 sum |q||k| (no worst-case format term: N roundings of F32_EPS each would double the bound at
    nine chunks).  A_i' / A_i = exp(d_i) / sum_j A_j exp(d_j) with |d_j| <= e_j, so it lies between exp(-e_i) / sum_j A_j exp(e_j) and
    exp(e_i) / sum_j A_j exp(-e_j): the softmax slope, not linearised.  Then mat_rel |A| for expf, the 32-term sum and the division, and half
    a bf16 ulp of A."""
    r = ca_reference(c)
    Sm, A = r["S"][z], r["A"][z]
    eS = sum_rel * r["s_abs"][z]
    e = eS + half_ulp(Sm, eS)
    up = torch.exp(e) / (A * torch.exp(-e)).sum(-1, keepdim=True) - 1.0
    dn = 1.0 - torch.exp(-e) / (A * torch.exp(e)).sum(-1, keepdim=True)
    slope = torch.maximum(up, dn)
    d = A * (slope + mat_rel * (1.0 + slope))
    return d + half_ulp(A, d)


def ca_apply_reference(A_dev: torch.Tensor, v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fp64 A_dev v, its bound) for the matrix [G, 32, 32] a launch produced (exact bf16 values) and v [N, G, 32]: 32 F32_EPS sum |A||v| for the
    fp32 sums of exact products, and half a bf16 ulp of the result."""
    ref = torch.einsum("gcd,ngd->ngc", A_dev.double(), v)
    e = 32 * F32_EPS * torch.einsum("gcd,ngd->ngc", A_dev.double().abs(), v.abs())
    return ref, e + half_ulp(ref, e)


def ca_e2e_ratio(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max over the (token, group) rows of max |got - ref| / max |ref| ([N, G, 32] each)."""
    return ((got.double() - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)).max().item()


CA_FAULTS = {
    "drop_last_chunk": ("gram", "last partial chunk dropped"),
    "drop_last_tile": ("gram", "last partial tile of a chunk dropped"),
    "no_zero_past_end": ("gram", "rows past n_end not zeroed: the re-read last row is counted again"),
    "qk_swapped": ("gram", "q and k exchanged (transposed Gram)"),
    "gram_group_minus_4": ("gram", "group g >= 4 mapped onto group g - 4 in the Gram kernel"),
    "softmax_wrong_axis": ("matrix", "softmax over the q channel"),
    "scale_of_largest": ("matrix", "scale taken from the largest image's N"),
    "chunks_of_largest": ("matrix", "chunk count of the largest image used for a smaller one (fill pattern summed in)"),
    "no_logit_round": ("matrix", "logits not rounded to bf16 before the exponential (bitwise: it moves the result towards the reference)"),
    "a_transposed": ("out", "A applied transposed"),
    "image0_matrix": ("out", "image z reading image 0's matrices"),
    "apply_group_minus_4": ("out", "group g >= 4 mapped onto group g - 4 in the apply kernel"),
    "halves_swapped": ("out", "the two 16-channel halves of the apply exchange swapped"),
    "store_past_n": ("canary", "a token >= N stored"),
}
CA_BITWISE = {"no_logit_round"}


def ca_fault_applies(c: Case, fault: str, z: int) -> bool:
    """Whether the fault changes what image z's units hold."""
    N, G, Nmax = c.sizes[z], c.C // 32, max(c.sizes)
    if fault == "drop_last_chunk":
        return N % CA_TOK != 0
    if fault in ("drop_last_tile", "no_zero_past_end"):
        return N % CA_TILE != 0
    if fault in ("gram_group_minus_4", "apply_group_minus_4"):
        return G > 4
    if fault == "scale_of_largest":
        return N != Nmax
    if fault == "chunks_of_largest":
        return cdiv(N, CA_TOK) != cdiv(Nmax, CA_TOK)
    if fault == "image0_matrix":
        return z > 0
    if fault == "store_past_n":
        return N % CA_BLOCK != 0
    return True


def ca_emulate(c: Case, fault: Optional[str] = None) -> dict:
    """The kernels' fp32 arithmetic and bf16 rounding points in the order of the fp32-FMA pair (one fmaf chain over a chunk's tokens, one over the
    32 channels; the matrix-core kernels add the same exact products in another order, inside the same format bounds).
    -> part [n_img, slots, G, 32, 32] fp32 (FILL in dead slots), A [n_img, G, 32, 32], logit: the fp32 logits before their bf16 rounding, out: per
    image [N, G, 32], spill: per image the tokens >= N that were stored."""
    lay = ca_layout(len(c.sizes), max(c.sizes), c.C)
    G, slots, n_img, Nmax = lay["G"], lay["slots"], len(c.sizes), max(c.sizes)
    part = torch.full((n_img, slots, G, 32, 32), FILL, dtype=torch.float32)
    imgs = [tuple(t.float() for t in qkv) for qkv in ca_images(c)]
    for z, (q, k, _) in enumerate(imgs):
        N = q.shape[0]
        live = cdiv(N, CA_TOK)
        qp, kp = torch.zeros(live * CA_TOK, G, 32), torch.zeros(live * CA_TOK, G, 32)
        qp[:N], kp[:N] = q, k
        tile_end = cdiv(N, CA_TILE) * CA_TILE
        if fault == "no_zero_past_end":
            qp[N:tile_end], kp[N:tile_end] = q[N - 1], k[N - 1]
        if fault == "drop_last_tile" and N % CA_TILE:
            qp[tile_end - CA_TILE:], kp[tile_end - CA_TILE:] = 0.0, 0.0
        if fault == "drop_last_chunk" and N % CA_TOK:
            qp[(live - 1) * CA_TOK:], kp[(live - 1) * CA_TOK:] = 0.0, 0.0
        if fault == "qk_swapped":
            qp, kp = kp, qp
        if fault == "gram_group_minus_4" and G > 4:
            qp, kp = qp.clone(), kp.clone()
            qp[:, 4:], kp[:, 4:] = qp[:, :G - 4].clone(), kp[:, :G - 4].clone()
        qp, kp = qp.view(live, CA_TOK, G, 32), kp.view(live, CA_TOK, G, 32)
        acc = torch.zeros(live, G, 32, 32)
        for t in range(min(CA_TOK, tile_end)):
            acc = acc + qp[:, t, :, :, None] * kp[:, t, :, None, :]        # the product is exact in fp32: one rounding, as fmaf
        part[z, :live] = acc
    A, logit = torch.zeros(n_img, G, 32, 32), torch.zeros(n_img, G, 32, 32)
    for z in range(n_img):
        N = c.sizes[z]
        nch = slots if fault == "chunks_of_largest" else cdiv(N, CA_TOK)
        s = [torch.zeros(G, 32, 32) for _ in range(4)]
        kk = 0
        while kk + 4 <= nch:
            for u in range(4):
                s[u] = s[u] + part[z, kk + u]
            kk += 4
        while kk < nch:
            s[0] = s[0] + part[z, kk]
            kk += 1
        scale = torch.tensor(1.0) / torch.sqrt(torch.tensor(float(Nmax if fault == "scale_of_largest" else N)))
        sv = ((s[0] + s[1]) + (s[2] + s[3])) * scale
        logit[z] = sv
        if fault != "no_logit_round":
            sv = rb(sv)
        if fault == "softmax_wrong_axis":
            sv = sv.transpose(-1, -2)
        ex = torch.exp(sv - sv.amax(-1, keepdim=True))
        a = rb(ex / _xor_tree(ex, 32)[..., None])
        A[z] = a.transpose(-1, -2) if fault == "softmax_wrong_axis" else a
    outs, spill = [], []
    for z, (_, _, v) in enumerate(imgs):
        a = A[0 if fault == "image0_matrix" else z]
        if fault == "a_transposed":
            a = a.transpose(-1, -2)
        if fault == "apply_group_minus_4" and G > 4:
            a, v = a.clone(), v.clone()
            a[4:], v[:, 4:] = a[:G - 4].clone(), v[:, :G - 4].clone()
        acc = torch.zeros(v.shape[0], G, 32)
        for d in range(32):
            acc = acc + a[None, :, :, d] * v[:, :, d, None]
        o = rb(acc)
        if fault == "halves_swapped":
            o = torch.cat([o[..., 16:], o[..., :16]], -1)
        outs.append(o)
        N = c.sizes[z]
        spill.append(list(range(N, cdiv(N, CA_BLOCK) * CA_BLOCK)) if fault == "store_past_n" else [])
    return dict(part=part, A=A, logit=logit, out=outs, spill=spill)


def ca_logit_sum_error(c: Case, emu: Optional[dict] = None) -> float:
    """Worst error of the emulation's fp32 logit before its bf16 rounding (the fmaf chain over a chunk's tokens, the chunk sum, the scale)
    against the float64 S, relative to N^-0.5 sum |q||k|.  This is what SUM_REL stands for."""
    emu, r = emu or ca_emulate(c), ca_reference(c)
    return max(((emu["logit"][z].double() - r["S"][z]).abs() / r["s_abs"][z].clamp_min(1e-300)).max().item() for z in range(len(c.sizes)))


def ca_fp32_chain_error(c: Case, emu: Optional[dict] = None) -> float:
    """Worst relative error of the softmax kernel's fp32 chain after the logit rounding and before the rounding of A: expf(s - m), the 32-term sum
    and the division in fp32 against float64 on the same bf16 logits.  This is what MAT_REL stands for.  (With the two roundings in, the
    emulation's error stays below the two rounding terms at every element, so there is no excess to measure; taken out, what is left is this
    and ca_logit_sum_error.)"""
    part = (emu or ca_emulate(c))["part"]
    worst = 0.0
    for z, N in enumerate(c.sizes):
        sv = rb(part[z, :cdiv(N, CA_TOK)].sum(0) * (torch.tensor(1.0) / torch.sqrt(torch.tensor(float(N)))))
        ex = torch.exp(sv - sv.amax(-1, keepdim=True))
        a = ex / _xor_tree(ex, 32)[..., None]
        want = torch.softmax(sv.double(), -1)
        worst = max(worst, ((a.double() - want).abs() / want).max().item())
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------
# depthwise 3x3 conv + residual (+ LayerNorm)
# ---------------------------------------------------------------------------------------------------------------------------------------
DW_RUN = 8                # kDwRun
DW_LN_CHUNKS = 4          # kDwLnChunks: C <= 64 * 4 * 8
DW_SHAPES = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 7), (5, 8), (4, 17), (3, 33))
DW_PIX_C = (8, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048)
DW_RUN_C = (128, 256, 512, 1024)
DW_SEP_C = (8, 96, 256, 768)
DW_ROUTES = ("sep", "pix", "run")
DW_SET_FORM = {"pix": 0, "run": 2}       # fo1_dwconv_ln_set_form; 1 is the product rule


def dw_ppw(chunks: int) -> int:
    """Pixels per wave of both fused forms (dwconv3x3_ln(): chunks <= 16 -> 4, <= 32 -> 2, else 1)."""
    return 4 if chunks <= 16 else (2 if chunks <= 32 else 1)


def dwln_form(chunks: int, map_pixels: int, total_pixels: int, setting: int = 1) -> int:
    """dwln_form() of vision_ops.hip: the run form's width in chunks, or 0 for the per-pixel form (restated only: the profile rows carry one name
    for both forms)."""
    if not setting or map_pixels * chunks * 16 > (1 << 31):
        return 0
    if chunks not in (16, 32, 64, 128):
        return 0
    waves = total_pixels // (4 if chunks == 128 else DW_RUN) // dw_ppw(chunks)
    return chunks if waves >= 4096 or setting == 2 else 0


def dw_run_template(chunks: int) -> Tuple[int, int, int]:
    """<PPW, NCH, RUN> of dwconv3x3_ln_run_kernel."""
    return (dw_ppw(chunks), 2 if chunks == 128 else 1, 4 if chunks == 128 else DW_RUN)


def _dw_cases() -> List[Case]:
    out = []
    for route, widths in (("sep", DW_SEP_C), ("pix", DW_PIX_C), ("run", DW_RUN_C)):
        for C in widths:
            for H, W in DW_SHAPES:
                for B in (1, 3):
                    rows = tuple(b * H * W for b in range(B))
                    out.append(Case("dwconv", f"dw-{route}-c{C}-{H}x{W}-b{B}", route=route, C=C, sizes=((H, W),) * B, rows=rows, ragged=False))
            if route != "sep":                  # (the separate kernel has no ragged entry)
                for name, sizes in (("r1", ((3, 7), (1, 9), (4, 17))), ("r2", ((9, 1), (1, 1), (3, 33)))):
                    rows, r = [], 2
                    for i, (H, W) in enumerate(sizes):
                        rows.append(r)
                        r += H * W + i
                    out.append(Case("dwconv", f"dw-{route}-c{C}-{name}-ragged", route=route, C=C, sizes=sizes, rows=tuple(rows), ragged=True))
    return out


def dw_total_rows(c: Case) -> int:
    H, W = c.sizes[-1]
    return c.rows[-1] + H * W


DW_SPARE = 10             # canary rows after the last pixel of y and h (a short run's dropped stores would land there)
BORDER = dict(top=96.0, bottom=-80.0, left=112.0, right=-104.0)


def _dw_build(c: Case) -> dict:
    C, chunks = c.C, c.C // 8
    g = _gen(C, sum(h * w for h, w in c.sizes), len(c.sizes), 9)
    x = torch.full((dw_total_rows(c) + DW_SPARE, C), POISON)
    for b, ((H, W), r0) in enumerate(zip(c.sizes, c.rows)):
        m = 4.0 * grid_values((H, W, C), g).float() + 32.0 * b
        m[0] += BORDER["top"]
        m[-1] += BORDER["bottom"]
        m[:, 0] += BORDER["left"]
        m[:, -1] += BORDER["right"]
        x[r0:r0 + H * W] = m.reshape(H * W, C)
    w9 = 0.25 * grid_values((9, C), g).float()
    bias = 4.0 * grid_values((C,), g).float()
    if chunks >= 3:
        w9[:, (chunks - 1) * 8:] = 0.0
        bias[8:16] = torch.tensor([0.0, -0.0] * 4)
    lw = (1 + 0.1 * torch.randn(C, generator=g)).to(BF)
    lb = (0.1 * torch.randn(C, generator=g)).to(BF)
    return dict(x=x.to(BF), w9=w9.to(BF), bias=bias.to(BF), ln_w=lw, ln_b=lb)


def dw_reference(c: Case) -> dict:
    """float64 on the bf16 inputs: conv = bias + sum x w per image (zero outside), y = x + conv, mag = |bias| + sum |x||w|; [rows, C] each, NaN in
    the rows of no image."""
    if c.name in _REF:
        return _REF[c.name]
    d = inputs(c)
    x, w9, bias = d["x"].double(), d["w9"].double(), d["bias"].double()
    R = dw_total_rows(c)
    conv, mag = torch.full((R, c.C), float("nan"), dtype=torch.float64), torch.full((R, c.C), float("nan"), dtype=torch.float64)
    for (H, W), r0 in zip(c.sizes, c.rows):
        m = x[r0:r0 + H * W].view(H, W, c.C)
        pad = torch.zeros(H + 2, W + 2, c.C, dtype=torch.float64)
        pad[1:-1, 1:-1] = m
        cv, mg = bias.expand(H, W, c.C).clone(), bias.abs().expand(H, W, c.C).clone()
        for t in range(9):
            sl = pad[t // 3:t // 3 + H, t % 3:t % 3 + W]
            cv += sl * w9[t]
            mg += sl.abs() * w9[t].abs()
        conv[r0:r0 + H * W], mag[r0:r0 + H * W] = cv.reshape(-1, c.C), mg.reshape(-1, c.C)
    _REF[c.name] = dict(conv=conv, mag=mag, y=x[:R] + conv)
    return _REF[c.name]


def dw_y_bound(c: Case) -> torch.Tensor:
    """Half a bf16 ulp of the conv value from its own binade, carried at slope 1, half a bf16 ulp of y, and 10 F32_EPS (|bias| + sum |x||w|) for
    the fmaf chain."""
    r = dw_reference(c)
    e = 10 * F32_EPS * r["mag"]
    e = e + half_ulp(r["conv"], e)
    return e + half_ulp(r["y"], e)


def dw_image_rows(c: Case) -> torch.Tensor:
    keep = torch.zeros(dw_total_rows(c), dtype=torch.bool)
    for (H, W), r0 in zip(c.sizes, c.rows):
        keep[r0:r0 + H * W] = True
    return keep


def _ln_case(c: Case, y: torch.Tensor) -> Case:
    """The rows of y (bf16 [M, C]) as a layernorm case of small_op_cases, so that its reference, bound and emulation are the ones used here."""
    d = inputs(c)
    k = Case("rownorm", f"davit-ln-{c.name}", op="layernorm", D=c.C, M=y.shape[0], ldx=c.C, ldy=c.C)
    S._INPUTS[k.name] = dict(x=y, w=d["ln_w"], b=d["ln_b"])
    return k


def dw_h_reference(c: Case, y: torch.Tensor, quarter: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fp64 LayerNorm of the y the same launch returned, small_op_cases' layernorm bound for it)."""
    k = _ln_case(c, y)
    try:
        return S._rownorm_ref(k), S._rownorm_bound(k, quarter)
    finally:
        S._INPUTS.pop(k.name, None)


DW_FAULTS = {
    "tap_across_image": ("y", "tap across an image boundary"),
    "clamp_keeps_weight": ("y", "clamped tap with its weight kept"),
    "short_run_spill": ("y", "the last pixels of a short run stored into the next row"),
    "edge_off_by_one": ("y", "H - 1 or W - 1 edge off by one"),
    "bias_dropped": ("y", "bias dropped"),
    "residual_from_conv": ("y", "residual taken from the rounded conv, not from x"),
    "chunk_plus_lpp": ("y", "chunk sub + LPP read for chunk sub (widths with more chunks than lanes per pixel)"),
    "ln_from_fp32": ("h", "LayerNorm fed the fp32 conv value, not the stored bf16 (bitwise)"),
}
DW_BITWISE = {"ln_from_fp32"}


def dw_fault_applies(c: Case, fault: str, b: int) -> bool:
    (H, W), chunks = c.sizes[b], c.C // 8
    if fault == "tap_across_image":
        return c.rows[b] > 0 or c.rows[b] + H * W < dw_total_rows(c)       # rows of the buffer before or after the image
    if fault == "clamp_keeps_weight":
        return True
    if fault == "short_run_spill":
        return c.route == "run" and W % dw_run_template(chunks)[2] != 0
    if fault == "edge_off_by_one":
        return H > 1 or W > 1
    if fault == "chunk_plus_lpp":
        return c.route != "sep" and chunks > 64 // dw_ppw(chunks)
    return True


def dw_emulate(c: Case, fault: Optional[str] = None) -> dict:
    """The kernels' arithmetic: acc = bias, nine fmaf in tap order (a tap outside the map meets a zero weight, or is skipped: the same sum),
    y = bf16(x + bf16(acc)), h = LayerNorm of the stored bf16 y (small_op_cases' rownorm emulation).  -> y, h as fp32 [rows + DW_SPARE, C] with NaN
    in the rows nothing wrote."""
    d = inputs(c)
    C, chunks = c.C, c.C // 8
    xall, w9, bias = d["x"].float(), d["w9"].float(), d["bias"].float()
    R = dw_total_rows(c)
    y = torch.full((R + DW_SPARE, C), float("nan"))
    pre = torch.full((R + DW_SPARE, C), float("nan"))
    lpp = 64 // dw_ppw(chunks)
    src = torch.arange(C)
    if fault == "chunk_plus_lpp" and chunks > lpp and c.route != "sep":
        ch = torch.arange(chunks)
        ch = torch.where(ch + lpp < chunks, ch + lpp, ch)
        src = (ch[:, None] * 8 + torch.arange(8)[None]).reshape(-1)
    for (H, W), r0 in zip(c.sizes, c.rows):
        hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        acc = torch.zeros(H, W, C) if fault == "bias_dropped" else bias[src].expand(H, W, C).clone()
        He, We = (H - 1, W - 1) if fault == "edge_off_by_one" else (H, W)
        for t in range(9):
            h2, w2 = hh + t // 3 - 1, ww + t % 3 - 1
            ok = (h2 >= 0) & (h2 < He) & (w2 >= 0) & (w2 < We)
            if fault == "edge_off_by_one":
                ok |= (h2 == hh) & (w2 == ww)
            if fault == "tap_across_image":               # the row test of the whole batch instead of the image's: linear addresses past the image
                lin = r0 + h2 * W + w2
                inside = (lin >= 0) & (lin < R) & (w2 >= 0) & (w2 < W)
                xv = xall[lin.clamp(0, R - 1)][:, :, src]
                ok = inside
            else:
                xv = xall[r0 + h2.clamp(0, H - 1) * W + w2.clamp(0, W - 1)][:, :, src]
            wv = w9[t][src].expand(H, W, C)
            if fault != "clamp_keeps_weight":
                wv = torch.where(ok[:, :, None], wv, torch.zeros(()))
            acc = acc + xv * wv                            # bf16 x bf16 is exact in fp32: one rounding, as fmaf
        ctr = xall[r0:r0 + H * W][:, src].view(H, W, C)
        conv = rb(acc)
        full = conv if fault == "residual_from_conv" else ctr + conv
        y[r0:r0 + H * W] = rb(full).reshape(-1, C)
        pre[r0:r0 + H * W] = full.reshape(-1, C)
    run = dw_run_template(chunks)[2]
    for (H, W), r0 in zip(c.sizes, c.rows):
        if fault == "short_run_spill" and c.route == "run" and W % run:
            n_sp = cdiv(W, run) * run - W                 # pixels w >= W of every row's last run land on the next row's first pixels
            for r in range(H):
                a = r0 + (r + 1) * W
                y[a:a + n_sp] = y[a - 1]
    keep = torch.zeros(R + DW_SPARE, dtype=torch.bool)
    keep[:R] = dw_image_rows(c)
    if fault == "short_run_spill":
        keep = ~torch.isnan(y[:, 0])
    h = torch.full((R + DW_SPARE, C), float("nan"))
    if c.route != "sep":
        k = _ln_case(c, (pre if fault == "ln_from_fp32" else y)[keep].to(torch.float32 if fault == "ln_from_fp32" else BF))
        try:
            h[keep] = S._rownorm_emul(k)[0]
        finally:
            S._INPUTS.pop(k.name, None)
    return dict(y=y, h=h)


# ---------------------------------------------------------------------------------------------------------------------------------------
_INPUTS: Dict[str, dict] = {}
_BUILD = {"chattn": _ca_build, "dwconv": _dw_build}
CASES: Dict[str, List[Case]] = {"chattn": _ca_cases(), "dwconv": _dw_cases()}
ALL_CASES = CASES["chattn"] + CASES["dwconv"]


def inputs(c: Case) -> dict:
    if c.name not in _INPUTS:
        _INPUTS[c.name] = _BUILD[c.family](c)
    return _INPUTS[c.name]


def measure(emulated=None) -> dict:
    """What the constants are derived from: the fp32 softmax chain's worst relative error (MAT_REL) and the fp32 logit sums' worst error relative to
    N^-0.5 sum |q||k| (SUM_REL), each times 4 and rounded up to a power of two, and the emulation's worst end-to-end fraction of the row maximum
    (E2E = the power of two at or above 2 x).  emulated: case -> ca_emulate(case), to reuse results already computed."""
    mat, sm, e2e = 0.0, 0.0, 0.0
    for c in CASES["chattn"]:
        emu, ref = (emulated(c) if emulated else ca_emulate(c)), ca_reference(c)
        mat, sm = max(mat, ca_fp32_chain_error(c, emu)), max(sm, ca_logit_sum_error(c, emu))
        for z in range(len(c.sizes)):
            e2e = max(e2e, ca_e2e_ratio(emu["out"][z], ref["out"][z]))
    return dict(mat=mat, sum=sm, e2e=e2e)
