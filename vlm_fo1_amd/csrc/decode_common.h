// decode_common.h — types shared by the decode-step translation units (decode.hip: v_dot2 GEMV, bookkeeping; decode_mfma.hip:
// MFMA skinny GEMV; attention.hip: decode attention).  Device state per sequence: int32[8] =
// { pos, rope_row, kv_start, finished, n_gen, max_new, -, - } (see decode.hip).
#pragma once
#include "common.h"

namespace fo1 {

enum { GB_PLAIN = 0, GB_SWIGLU = 1, GB_QKV = 2 };

struct GemvBParams {
    const uint16_t* X = nullptr;       // [M, ldx]
    const uint16_t* W = nullptr;       // [N, ldw]
    const uint16_t* bias = nullptr;    // [N] or null
    const uint16_t* res = nullptr;     // [M, ldr] or null (plain mode)
    uint16_t* C = nullptr;             // [M, ldc]: plain out | SwiGLU out | rotated q rows (QKV mode)
    int M = 0, N = 0, K = 0, ldx = 0, ldw = 0, ldc = 0, ldr = 0;
    const uint16_t* norm_w = nullptr;  // optional fused RMSNorm on x
    float norm_eps = 0.f;
    int kp_chunks = 0;                 // (dot2 kernel) 16-B chunks of K staged in LDS at a time
    int canon_chunks = 0;              // (dot2 kernel) canonical K segment (chunks)
    // QKV mode
    int n_q = 0, n_kv = 0;             // heads (head_dim 128)
    const uint16_t* cos_t = nullptr; const uint16_t* sin_t = nullptr;   // [rows, 128] bf16 tables
    const int* state = nullptr;        // [M][8]
    uint16_t* kcache = nullptr; long long kc_head_stride = 0;      // [n_kv][rows][128]
    uint16_t* vtcache = nullptr; long long vt_row_stride = 0;      // [n_kv*128][rows]
    // x = the decode attention's output, combined HERE from its split-KV partials (round 6: M <= 2, plain mode, K = heads x 128 <= 2048):
    // the rows attn_decode_combine_kernel would write never exist and its launch is not made
    const float* attn_part = nullptr;                // [M][chunks][n_kv][16][130] fp32 (attn_fwd_kernel PARTIAL)
    long long attn_part_seq_stride = 0;
    const int* attn_state = nullptr;                 // [M][8]: keys = state[0] + 1 - state[2], state[3] = finished
    int attn_chunk = 0, attn_n_kv = 0, attn_group = 0;
    // what every entry fills: operands, strides, shape and the norm (the mode's own fields stay at their defaults until the entry sets them)
    GemvBParams(const void* x, int ldx, const void* W, int ldw, const void* bias, const void* res, int ldr, void* C, int ldc, int M, int N, int K,
                const void* norm_w, float norm_eps)
        : X((const uint16_t*)x), W((const uint16_t*)W), bias((const uint16_t*)bias), res((const uint16_t*)res), C((uint16_t*)C), M(M), N(N), K(K),
          ldx(ldx), ldw(ldw), ldc(ldc), ldr(ldr), norm_w((const uint16_t*)norm_w), norm_eps(norm_eps) {}
};

// Units (the weight rows one work item owns) of a launch, for kernel, dispatcher and launcher alike.  rows = weight rows per unit: plain = that many
// consecutive features; SwiGLU = rows / 2 gate rows + their up partners (N / 2 features); QKV = rows / 2 rotary pairs of a q / k head (64 pairs per
// head), then rows consecutive dims of the v heads (128 each).
__host__ __device__ constexpr int gemv_units(int mode, int rows, int N, int n_q, int n_kv) {
    return mode == GB_SWIGLU ? N / rows : mode == GB_QKV ? (n_q + n_kv) * (128 / rows) + n_kv * (128 / rows) : (N + rows - 1) / rows;
}

// What fo1_gemv_bf16 and fo1_gemv_batch_bf16 check alike (`operands`: the entry's own NULL test; max_m: the rows its kernels take)
inline int check_gemv_operands(const char* who, bool operands, int max_m, const void* x, int ldx, const void* W, int ldw, const void* norm_weight,
                               int M, int N, int K) {
    FO1_CHECK_ARG(operands, "%s: NULL operand", who);
    FO1_CHECK_ARG(M >= 1 && M <= max_m && N > 0 && K > 0 && K % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0, "%s: bad shape M=%d (1..%d) N=%d K=%d", who, M,
                  max_m, N, K);
    FO1_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)norm_weight & 15) == 0, "%s: misaligned operand", who);
    return FO1_OK;
}

// Geometry of gemv_mfma_kernel<MM, MODE, NB, MP, HALF, R8> (decode_mfma.hip), read by the kernel and by its launcher.
constexpr int GM_NW = 8;                                                 // waves per workgroup
template <int MM, int NB, bool MP, bool HALF, bool R8>
struct GemvMfmaGeom {
    static constexpr int NG = MM == 32 ? 2 : 1;                          // column groups of 16 sequences
    static constexpr bool XREG = MM == 32 && !MP;                        // x fragments live in registers (single-piece K)
    static constexpr bool H8 = HALF || R8;                               // 8-row blocks, a stage = the k-step pair (s, s + 8)
    static constexpr int PD = R8 ? 2 : ((HALF && !MP) ? 2 : ((MM == 32 && MP) ? 2 : 4));   // register stages per wave = stages per staged piece
    static constexpr int SSTEP = H8 ? 16 : 8;                            // k-step distance between a wave's consecutive stages
    static constexpr int PSTEPS = SSTEP * PD;                            // k-steps of x staged at a time: 32 (64: HALF && MP)
    static constexpr int XPITCH = PSTEPS * 128 + 32;                     // bytes per staged x row (= 32 mod 256)
    // XR32 (round 6): 17..26 sequences, deep K (`down`), 8-row units — 32 staged rows of a 32-k-step piece (132 KB) do not fit beside the scratch and the
    // reduction buffers, M rows do up to M = 26: only the launch's own rows are staged, the column slots past them read the last staged row (never stored)
    static constexpr bool XR32 = MM == 32 && MP && R8;
    __host__ __device__ static constexpr int x_rows(int M) { return XR32 ? M : MM; }                      // staged x rows
    static constexpr int SCRATCH_BYTES = GM_NW * NB * 2048;              // [GM_NW][NB][2048] weight scratch (wave-private)
    static constexpr int RED_BYTES = 2 * NG * GM_NW * NB * 1024;         // [2][NG][GM_NW][NB][64][4] fp32 partial sums, double-buffered by unit parity
    // XREG: the scratch and the reduction buffers reuse the x image once its fragments sit in registers; the 128 B hold the rows' rstd
    static constexpr size_t lds_bytes(int M) {
        return XREG ? (size_t)MM * XPITCH + 128 : (size_t)x_rows(M) * XPITCH + SCRATCH_BYTES + RED_BYTES + 128;
    }
};

// The split-KV partials of the decode attention, fp32 [chunks][n_kv_heads][ATTN_PART_ROWS][head_dim + 2] per sequence: a row per query head
// of the KV head's group (the MFMA's 16 query columns: at most 16 query heads per KV head) = the unnormalised O row, then m (base 2) and l.
// Written by attn_fwd_kernel<128, 4, PARTIAL> (and the A/B attn_decode_wg_kernel), read by attn_combine_row's two callers.
constexpr int ATTN_PART_ROWS = 16;
constexpr int attn_part_row_floats(int head_dim) { return head_dim + 2; }
constexpr long long attn_part_seq_floats(int chunks, int n_kv_heads, int head_dim) {
    return (long long)chunks * n_kv_heads * ATTN_PART_ROWS * attn_part_row_floats(head_dim);
}

// One (query head, 8 consecutive head-dim elements) of the split-KV combine: out[d] = sum_s exp(m_s - M) O_s[d] / sum_s exp(m_s - M) l_s over
// the chunks in ascending order — THE arithmetic of attn_decode_combine_kernel (attention.hip), which calls it with ND = 1; the decode GEMV's
// fused prologue calls it with ND = 8.  Explicit fmaf: both callers round identically whatever the contraction setting.
//   pr0 = the (head's slot) row of chunk 0, cstride = floats between consecutive chunks' rows; m_s / l_s at pr[128], pr[129].
template <int ND>
__device__ __forceinline__ void attn_combine_row(const float* __restrict__ pr0, long long cstride, int n_valid, int d0, float (&out)[ND]) {
    // loads in batches, every address of a batch known up front (a load inside `for s` is load -> wait -> use per chunk: ~0.5 us each, see the
    // round-2 note in attention.hip); indices past the last chunk are clamped and enter with weight exactly 0 (fmaf(0, finite, x) = x)
    float M = -INFINITY;
    for (int s0 = 0; s0 < n_valid; s0 += 8) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = pr0[(long long)min(s0 + j, n_valid - 1) * cstride + 128];
#pragma unroll
        for (int j = 0; j < 8; ++j) M = fmaxf(M, t[j]);
    }
    float num[ND], den = 0.f;
#pragma unroll
    for (int j = 0; j < ND; ++j) num[j] = 0.f;
    for (int s0 = 0; s0 < n_valid; s0 += 4) {
        float mm[4], ll[4], v[4][ND];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* pr = pr0 + (long long)min(s0 + u, n_valid - 1) * cstride;
            mm[u] = pr[128];
            ll[u] = pr[129];
#pragma unroll
            for (int j = 0; j < ND; ++j) v[u][j] = pr[d0 + j];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float w = s0 + u < n_valid ? __expf(mm[u] - M) : 0.f;
#pragma unroll
            for (int j = 0; j < ND; ++j) num[j] = __builtin_fmaf(w, v[u][j], num[j]);
            den = __builtin_fmaf(w, ll[u], den);
        }
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) out[j] = den > 0.f ? num[j] / den : 0.f;
}

// (decode.hip: the greedy head; sample.hip: the sampled head)  Greedy-search bookkeeping for sequence b given its next token: record it, test the stop rule (EOS / keyword ids, or the
// max_new_tokens budget: HF stops AFTER appending the stop token), advance the device state, publish the token as the next
// step's embedding-gather plan entry.  A finished sequence keeps its state frozen: later steps recompute harmlessly in place.
__device__ __forceinline__ void accept_token(int tok, int* st, int* plan, int* ids_out, int ids_ld, const int* stop_ids, int n_stop, int* done) {
    plan[0] = 0;
    // a finished (or never-started) slot keeps stepping with whatever its rows hold: publish a valid embedding row for it — its
    // logits may be stale or non-finite (the pool skips its attention), and an argmax over NaN rows leaves the index at INT_MAX
    plan[1] = st[3] ? 0 : tok;
    if (st[3]) return;
    const int n = st[4];
    ids_out[n] = tok;
    st[4] = n + 1;
    bool stop = (n + 1 >= st[5]) || (n + 1 >= ids_ld);
    if (n_stop < 0) {       // per-sequence stop sets (the decode pool admits submissions with different sets): row st[6] of a table [sets][1 + 16] = {n, ids...}
        stop_ids += st[6] * 17;
        n_stop = min(stop_ids[0], 16);
        ++stop_ids;
    }
    for (int i = 0; i < n_stop; ++i) stop = stop || (tok == stop_ids[i]);
    if (stop) {
        st[3] = 1;
        atomicAdd(done, 1);
    }
}

// ---- what the heads that read a bf16 logits row share (sample.hip: the sampled / general head; logprob.hip: the log-probability record) ----
// bf16 bits -> order-preserving key 0 .. 65535 (larger value = larger key; -0 = +0), -1 for inf / NaN
__device__ __forceinline__ int sp_key(uint32_t b) {
    if ((b & 0x7f80u) == 0x7f80u) return -1;
    if (b == 0x8000u) b = 0;
    return (int)((b & 0x8000u) ? (b ^ 0xffffu) : (b | 0x8000u));
}
__device__ __forceinline__ float sp_val(int key) {
    const uint32_t b = key >= 0x8000 ? (uint32_t)(key & 0x7fff) : ((uint32_t)key ^ 0xffffu);
    return __uint_as_float(b << 16);
}
// one 16-byte chunk of a row -> its 8 entries as bf16 bits
__device__ __forceinline__ void sp_unpack8(const uint4& v, uint32_t (&e)[8]) {
    e[0] = v.x & 0xffffu; e[1] = v.x >> 16; e[2] = v.y & 0xffffu; e[3] = v.y >> 16;
    e[4] = v.z & 0xffffu; e[5] = v.z >> 16; e[6] = v.w & 0xffffu; e[7] = v.w >> 16;
}
// tokens [i0, i0 + 8) of the row as bf16 bits; past the row's end: NaN (no key).  `vec`: the row is 16-byte aligned.
__device__ __forceinline__ void sp_load8(const uint16_t* __restrict__ row, int i0, int V, bool vec, uint32_t (&e)[8]) {
    if (vec && i0 + 8 <= V) {
        sp_unpack8(*reinterpret_cast<const uint4*>(row + i0), e);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = i0 + j < V ? (uint32_t)row[i0 + j] : 0x7fc0u;
    }
}

// inclusive scan over the 64 lanes of a wave, lane order (Hillis-Steele: a fixed tree, the same bits every run)
__device__ __forceinline__ float sp_scan_f(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// decode_mfma.hip
#ifdef FO1_ENABLE_AB
extern int g_gemv_half;   // decode_mfma.hip: bit 0 = 8-row units at M <= 8 (HALF), bit 1 = at 9..32 sequences (R8)
#else
[[maybe_unused]] static constexpr int g_gemv_half = 3;
#endif
int gemv_mfma_any(GemvBParams& p, int mode, hipStream_t st);

}  // namespace fo1
