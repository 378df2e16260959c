// upn_post.hip — the UPN detector's post-process on the device for gfx950: box decode, score sort, score threshold, greedy NMS and the
// compacted outputs, one workgroup of 1024 threads per image, one launch, no host read (include/fo1.h has the definition).
// Reference: detect_tools/upn/inference_wrapper.py (postprocess :138-185, filter :187-237, torchvision.ops.nms).
//
// Form: thread t decodes query t; a 1024-wide bitonic sort of 64-bit (score key, ~index) words runs in registers (partner distances
// below 64 are wave shuffles, the ten larger ones go through LDS with one barrier each); the sorted boxes are laid out in LDS; every
// wave fills words of the suppression bit matrix (bit j of word (i, j / 64) = candidate j > i has iou(i, j) > threshold) with one
// ballot per 64 pairs; wave 0 resolves the greedy scan 64 candidates at a time from scalar registers (the block's diagonal words sit
// one per lane, so the serial part is a count-trailing-zeros and two v_readlane per KEPT box) and ORs the kept rows into the words of
// the later blocks; every thread then ranks its own candidate by a popcount prefix and writes it.
// LDS: 128 KB matrix (its head doubles as the sort's exchange buffers) + 16 KB boxes + 4 KB scores + the kept words = 151 696 B of
// the CU's 160 KB.  A matrix row is 128 B, so the 16 diagonal-word reads of the scan are 16-way bank conflicts — 16 reads per image.
#include "common.h"

namespace fo1 {

constexpr int UP_NT = 1024;                              // threads = the largest Q
constexpr int UP_WORDS = UP_NT / 64;                     // 64-bit words per matrix row
constexpr int UP_MASK_BYTES = UP_NT * UP_WORDS * 8;
constexpr int UP_SMEM = UP_MASK_BYTES + UP_NT * 16 + UP_NT * 4 + UP_WORDS * 8;
static_assert(UP_SMEM <= 160 * 1024, "LDS per workgroup");

struct UpnPostArgs {
    const float* boxes; int ld_boxes; long long img_boxes;
    const float* logits; int ld_logits; long long img_logits;
    int Q;
    const fo1_upn_post_params_t* params;
    int32_t* n_keep; int32_t* keep_idx; float* boxes_f32; int32_t* boxes_i32; float* scores;
    int cap; long long out_stride;
};

// The definition's arithmetic: every operation rounds once (DESIGN §14 "No fused multiply-add").
__device__ __forceinline__ float4 up_decode(float cx, float cy, float w, float h, float W, float H) {
#pragma clang fp contract(off)
    const float x0 = cx - w / 2.0f, y0 = cy - h / 2.0f;
    const float x1 = x0 + w, y1 = y0 + h;
    return float4{x0 * W, y0 * H, x1 * W, y1 * H};
}
__device__ __forceinline__ float up_sigmoid(float logit) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-logit));
}
__device__ __forceinline__ float up_area(const float4& b) {
#pragma clang fp contract(off)
    return (b.z - b.x) * (b.w - b.y);
}
// iou(i, j) > thr.  With thr > 0 (the only case that asks) an intersection that is not > 0 gives iou = 0 or NaN, never above thr, so the
// division runs only where two boxes overlap — the result is the definition's for every input.
__device__ __forceinline__ bool up_iou_above(const float4& a, float area_a, const float4& b, float area_b, float thr) {
#pragma clang fp contract(off)
    const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.0f);
    const float ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.0f);
    const float inter = iw * ih;
    if (!(inter > 0.0f)) return false;
    return inter / ((area_a + area_b) - inter) > thr;
}

// order-preserving key of an fp32 score, NaN below everything (the map fo1_topk_desc_f32 sorts by)
__device__ __forceinline__ unsigned int up_key(float f) {
    unsigned int u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long up_shfl_xor64(unsigned long long v, int j) {
    const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)v, j, 64), hi = (unsigned int)__shfl_xor((int)(unsigned int)(v >> 32), j, 64);
    return ((unsigned long long)hi << 32) | lo;
}
// lane l's 64-bit value in every lane, as scalars (l is the same in every lane)
__device__ __forceinline__ unsigned long long up_readlane64(unsigned long long v, int l) {
    l = __builtin_amdgcn_readfirstlane(l);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, l), hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(UP_NT) void upn_post_kernel(const UpnPostArgs a) {
    extern __shared__ __align__(16) unsigned char up_smem[];
    unsigned long long* const mask = reinterpret_cast<unsigned long long*>(up_smem);                 // [1024][16]
    float4* const sbox = reinterpret_cast<float4*>(up_smem + UP_MASK_BYTES);                          // [1024]
    float* const ssc = reinterpret_cast<float*>(up_smem + UP_MASK_BYTES + UP_NT * 16);                // [1024]
    unsigned long long* const keptw = reinterpret_cast<unsigned long long*>(up_smem + UP_MASK_BYTES + UP_NT * 20);   // [16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.x;
    const int Q = a.Q;
    const fo1_upn_post_params_t prm = a.params[img];

    // ---- decode query tid; sort word = (score key, ~index): larger word = earlier; padding (0) sorts last ----
    float4 bx = float4{0.f, 0.f, 0.f, 0.f};
    float sc = 0.f;
    unsigned long long v = 0ull;
    if (tid < Q) {
        const float* b = a.boxes + img * a.img_boxes + (long long)tid * a.ld_boxes;
        bx = up_decode(b[0], b[1], b[2], b[3], prm.W, prm.H);
        sc = up_sigmoid(a.logits[img * a.img_logits + (long long)tid * a.ld_logits]);
        v = ((unsigned long long)up_key(sc) << 32) | (unsigned int)~(unsigned int)tid;
    }
    sbox[tid] = bx;
    ssc[tid] = sc;

    // ---- descending bitonic sort, one word per thread (every loop bound is the same in all threads) ----
    int xs = 0;
    for (int kk = 2; kk <= UP_NT; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            unsigned long long p;
            if (j >= 64) {                                          // partner in another wave: through LDS, two buffers in turn (one barrier per stage)
                unsigned long long* const buf = mask + (xs & 1) * UP_NT;
                buf[tid] = v;
                __syncthreads();
                p = buf[tid ^ j];
                ++xs;
            } else {
                p = up_shfl_xor64(v, j);
            }
            const bool take_max = ((tid & kk) == 0) == ((tid & j) == 0);
            v = take_max ? (v > p ? v : p) : (v < p ? v : p);
        }
    }
    __syncthreads();                                                // sbox / ssc written; the exchange buffers are free (they alias the matrix)

    // ---- rank tid: its query, box and score; candidates = the prefix with score >= min_score ----
    const int idx = (int)(~(unsigned int)v) & (UP_NT - 1);          // (padding ranks, tid >= Q, read slot 1023 and are never used)
    const float4 mb = sbox[idx];
    const float msc = ssc[idx];
    const bool cand = tid < Q && msc >= prm.min_score;
    const int n_cand = __builtin_amdgcn_readfirstlane(__syncthreads_count(cand));   // (the barrier also puts every read above before the writes below)
    sbox[tid] = mb;
    __syncthreads();

    const float thr = prm.iou_threshold;
    const bool do_nms = thr > 0.0f;
    const int nw = (n_cand + 63) >> 6;

    // ---- suppression matrix: word (i, w), rows i < min(n_cand, 64 w + 64), bits j = 64 w + lane > i ----
    if (do_nms) {
        for (int w = 0; w < nw; ++w) {
            const int j = w * 64 + lane;
            const float4 bj = sbox[j];
            const float aj = up_area(bj);
            const int iend = n_cand < w * 64 + 64 ? n_cand : w * 64 + 64;
            for (int i = wave; i < iend; i += UP_WORDS) {
                const float4 bi = sbox[i];
                const bool hit = j < n_cand && j > i && up_iou_above(bi, up_area(bi), bj, aj, thr);
                const unsigned long long m = __ballot(hit);
                if (lane == 0) mask[i * UP_WORDS + w] = m;
            }
        }
    }
    __syncthreads();

    // ---- greedy scan by wave 0: lane l < 16 carries word l of the dropped set ----
    if (wave == 0) {
        unsigned long long dropped = 0ull;
        for (int b = 0; b < nw; ++b) {
            const int nb = n_cand - 64 * b < 64 ? n_cand - 64 * b : 64;
            const unsigned long long valid = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
            unsigned long long kept = valid;
            if (do_nms) {
                const unsigned long long diag = lane < nb ? mask[(64 * b + lane) * UP_WORDS + b] : 0ull;
                unsigned long long alive = ~up_readlane64(dropped, b) & valid;
                kept = 0ull;
                while (alive) {                                     // scalar: the next surviving candidate is kept and drops its row's bits
                    const int i = __builtin_ctzll(alive);
                    kept |= 1ull << i;
                    alive &= ~(1ull << i);
                    alive &= ~up_readlane64(diag, i);
                }
                for (unsigned long long k = kept; k; k &= k - 1ull) {   // kept rows into the later blocks' words (independent loads)
                    const int i = __builtin_ctzll(k);
                    if (lane > b && lane < nw) dropped |= mask[(64 * b + i) * UP_WORDS + lane];
                }
            }
            if (lane == 0) keptw[b] = kept;
        }
        if (lane >= nw && lane < UP_WORDS) keptw[lane] = 0ull;
    }
    __syncthreads();

    // ---- outputs in keep order: rank = kept candidates before this one ----
    const int lim = prm.max_keep < a.cap ? prm.max_keep : a.cap;
    const long long ob = img * a.out_stride;
    if (tid < n_cand) {
        const unsigned long long kw = keptw[wave];
        if ((kw >> lane) & 1ull) {
            int rank = __popcll(kw & ((1ull << lane) - 1ull));
            for (int x = 0; x < wave; ++x) rank += __popcll(keptw[x]);
            if (rank < lim) {
                a.keep_idx[ob + rank] = idx;
                float* const of = a.boxes_f32 + ob + 4ll * rank;
                int32_t* const oi = a.boxes_i32 + ob + 4ll * rank;
                of[0] = mb.x; of[1] = mb.y; of[2] = mb.z; of[3] = mb.w;
                oi[0] = (int32_t)mb.x; oi[1] = (int32_t)mb.y; oi[2] = (int32_t)mb.z; oi[3] = (int32_t)mb.w;
                a.scores[ob + rank] = msc;
            }
        }
    }
    if (tid == 0) {
        int total = 0;
        for (int x = 0; x < UP_WORDS; ++x) total += __popcll(keptw[x]);
        total = total < lim ? total : lim;
        a.n_keep[ob] = total > 0 ? total : 0;
    }
}

}  // namespace fo1

extern "C" {

size_t fo1_upn_post_workspace_bytes(int Q) {
    (void)Q;
    return 0;                                                       // everything lives in LDS
}

int fo1_upn_post_batch_f32(const float* boxes, int ld_boxes, long long img_boxes, const float* logits, int ld_logits, long long img_logits, int Q, int n_images,
                           const fo1_upn_post_params_t* params, int32_t* n_keep, int32_t* keep_idx, float* boxes_f32, int32_t* boxes_i32, float* scores, int cap,
                           long long out_stride, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace fo1;
    FO1_CHECK_ARG(Q >= 1 && Q <= UP_NT, "upn_post: Q=%d outside [1, %d]", Q, UP_NT);
    FO1_CHECK_ARG(cap >= 1 && n_images >= 1 && n_images <= 65535, "upn_post: cap=%d, n_images=%d", cap, n_images);
    FO1_CHECK_ARG(boxes && logits && params && n_keep && keep_idx && boxes_f32 && boxes_i32 && scores, "upn_post: null pointer");
    FO1_CHECK_ARG(ld_boxes >= 4 && ld_logits >= 1 && img_boxes >= 0 && img_logits >= 0 && out_stride >= 0, "upn_post: bad strides");
    FO1_CHECK_ARG(n_images == 1 || out_stride >= 10ll * cap + 1, "upn_post: out_stride %lld < the %lld words of one image's outputs", out_stride, 10ll * cap + 1);
    const size_t need = fo1_upn_post_workspace_bytes(Q);
    FO1_CHECK_ARG(workspace || need == 0, "upn_post: null workspace");
    if (workspace_bytes < need) return set_err(FO1_ERR_WORKSPACE, "upn_post: workspace %zu B < %zu B", workspace_bytes, need);
    const UpnPostArgs a{boxes, ld_boxes, img_boxes, logits, ld_logits, img_logits, Q, params, n_keep, keep_idx, boxes_f32, boxes_i32, scores, cap, out_stride};
    FO1_DYNAMIC_LDS_ONCE(UP_SMEM, upn_post_kernel);
    FO1_LAUNCH("upn_post", (double)n_images * Q * 24.0, upn_post_kernel, dim3(n_images), dim3(UP_NT), UP_SMEM, (hipStream_t)stream, a);
    return FO1_OK;
}

int fo1_upn_post_f32(const float* boxes, int ld_boxes, const float* logits, int ld_logits, int Q, const fo1_upn_post_params_t* params, int32_t* n_keep,
                     int32_t* keep_idx, float* boxes_f32, int32_t* boxes_i32, float* scores, int cap, void* workspace, size_t workspace_bytes, void* stream) {
    return fo1_upn_post_batch_f32(boxes, ld_boxes, 0, logits, ld_logits, 0, Q, 1, params, n_keep, keep_idx, boxes_f32, boxes_i32, scores, cap, 0, workspace,
                                  workspace_bytes, stream);
}

}  // extern "C"
