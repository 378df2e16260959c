// logprob.hip — log-probability of the chosen token and of the top-n alternatives of a bf16 logits row, on the device.
//
// Definition (include/fo1.h): F = the finite entries of the row, m = max_F l, S = sum_F exp(l_i - m) in fp32 in a fixed order,
// lp_i = (l_i - m) - log S for i in F, -inf otherwise (a row with empty F: -inf everywhere).  The RAW logits: before temperature, top-k / top-p
// and the repetition penalty — the record does not depend on the head that picked the token.  Top-n (n <= 8): the n finite entries with the
// largest l, descending, equal logits by smaller vocabulary index first, padded with (id = -1, lp = -inf).
//
// One workgroup of 1024 threads (16 waves of 64) per row, integer atomics only, no host read, one launch whatever the data:
//   1. one pass over the row: m, as a float max over the finite entries (bf16 values are fp32 values).  n > 0: the n-th largest of the 16 WAVE maxima is a lower bound `floor` of the row's n-th
//      largest entry — n entries at least that large exist, in n different waves — and on ordinary rows only a dozen entries reach it;
//   2. second pass (the row is in L2 now): S, summed in a fixed order (a thread's entries in the order it visits them, shuffle scan over the
//      64 lanes, the 16 waves in order).  n > 0: an entry >= floor enters its thread's sorted list of 8 packed 64-bit words — sp_key of the
//      value in the high half, complement of the index in the low half, so one unsigned compare is "larger value, else smaller index".  The
//      lists are exact whatever passes the gate;
//   3. the threads push their list entries to an LDS array; when at most 256 arrived (ordinary rows) each computes its rank by counting the
//      larger ones and the first n ranks are the answer; else (a flat row: thousands of equal maxima) n rounds of a workgroup max over the
//      threads' list heads, popping the winner's.  Words are distinct, so either way the order is exact and the same every run.
// Both passes keep 8 16-byte loads per thread in flight (lp_for_row) and spend ~13 VALU cycles-per-lane on an entry: exp is v_exp_f32 with
// the argument's rounding error folded back in (lp_exp), and -|l - m| clamped at -200 maps NaN, -inf and +inf to weight 0 without a test
// per entry.  n = 0 skips floor, gate, lists and step 3.  The same row gives the same bits whatever row b or batch B it sits in: nothing
// depends on either.  Columns [V, ld_logits) of a row are never read as data (lp_for_row stops at V, sp_load8 substitutes NaN past it).
#include "decode_common.h"

namespace fo1 {

constexpr int LP_NT = 1024;                       // threads per workgroup
constexpr int LP_NW = LP_NT / 64;                 // waves
constexpr int LP_TOP = FO1_LOGPROB_TOP_MAX;       // entries of a thread's list = the largest n
constexpr int LP_CAND = 256;                      // list entries the rank form of step 3 takes
constexpr int LP_MLP = 8;                         // 16-byte loads a thread has in flight

struct LogprobArgs {
    const uint16_t* logits; long long ld; int V;
    float* lp; int* top_ids; float* top_lp;
    // rows form: the chosen ids [B], one n for all rows, outputs lp[B] and [B][top_ld]
    const int* ids; int top_n; long long top_ld;
    // record form: per-row n (want[b], -1 = off), the decode state [B][8], the ids buffer [B][ids_ld], the rows' record counters;
    // outputs lp[B][ids_ld] and [B][ids_ld][LP_TOP]
    const int* want; const int* state; const int* gen_ids; int ids_ld; int* n_rec;
};

__device__ __forceinline__ unsigned long long lp_wave_max64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ float lp_wave_maxf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Every 16-byte chunk of the row this thread owns (tokens tid * 8 + k * LP_NT * 8 ...), in ascending order, as f(first index, 8 x bf16 bits).
// LP_MLP chunks are loaded before the first is used: with one load in flight per thread a pass over a 300 KB row is a chain of 19 round
// trips to memory; a workgroup keeps 16 waves x 64 lanes x LP_MLP x 16 bytes in flight instead.
template <class F>
__device__ __forceinline__ void lp_for_row(const uint16_t* __restrict__ row, int V, bool vec, F f) {
    constexpr int STEP = LP_NT * 8;
    int i0 = threadIdx.x * 8;
    if (vec) {
        for (; (long long)i0 + (LP_MLP - 1) * STEP + 8 <= V; i0 += LP_MLP * STEP) {
            uint4 q[LP_MLP];
#pragma unroll
            for (int u = 0; u < LP_MLP; ++u) q[u] = *reinterpret_cast<const uint4*>(row + i0 + u * STEP);
#pragma unroll
            for (int u = 0; u < LP_MLP; ++u) {
                uint32_t e[8];
                sp_unpack8(q[u], e);
                f(i0 + u * STEP, e);
            }
        }
    }
    for (; i0 < V; i0 += STEP) {
        uint32_t e[8];
        sp_load8(row, i0, V, vec, e);
        f(i0, e);
    }
}

__device__ __forceinline__ bool lp_finite(uint32_t e) { return (e & 0x7f80u) != 0x7f80u; }
__device__ __forceinline__ float lp_value(uint32_t e) { return __uint_as_float(e << 16); }

// exp(-|d|) for d = l - m, 0 for a d that is NaN or +-inf (fmaxf drops the NaN, the clamp at -200 underflows), about one ulp: v_exp_f32 of
// the fp32 product x log2(e), with the product's rounding error and the rest of log2(e) folded back in as exp2(ph + pl) = exp2(ph) (1 + pl ln 2)
// — expf's core without its range selects
__device__ __forceinline__ float lp_weight(float d) {
    const float x = fmaxf(-fabsf(d), -200.f);
    const float ph = x * 0x1.715476p+0f;
    float pl = __builtin_fmaf(x, 0x1.715476p+0f, -ph);
    pl = __builtin_fmaf(x, 0x1.4ae0cp-26f, pl);
    const float e = __builtin_amdgcn_exp2f(ph);
    return __builtin_fmaf(e, pl * 0x1.62e43p-1f, e);
}

// a value's place among the wave maxima / an entry's among the candidates: larger value first, then (for entries) smaller index
__device__ __forceinline__ int lp_wave_word(float v, int wave) { return v == -INFINITY ? 0 : (((sp_key(__float_as_uint(v) >> 16) + 1) << 4) | (LP_NW - 1 - wave)); }
__device__ __forceinline__ unsigned long long lp_word(uint32_t e, int i) { return ((unsigned long long)(uint32_t)(sp_key(e) + 1) << 32) | (uint32_t)~(uint32_t)i; }

// w into the descending list t (an empty place is 0; every word of an entry is > 0)
__device__ __forceinline__ void lp_insert(unsigned long long (&t)[LP_TOP], unsigned long long w) {
    if (w > t[LP_TOP - 1]) {
        t[LP_TOP - 1] = w;
#pragma unroll
        for (int j = LP_TOP - 1; j > 0; --j) {
            const unsigned long long a = t[j - 1], c = t[j];
            t[j - 1] = c > a ? c : a;
            t[j] = c > a ? a : c;
        }
    }
}

template <bool RECORD>
__global__ __launch_bounds__(LP_NT) void logprob_rows_kernel(LogprobArgs a) {
    __shared__ float s_wf[LP_NW];
    __shared__ unsigned long long s_w64[2][LP_NW], s_top[LP_TOP], s_cand[LP_CAND];
    __shared__ int s_floor, s_cnt;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V;
    int n, c;
    [[maybe_unused]] int n_done = 0;
    long long o_lp, o_top;      // where this row's outputs go
    int n_write;                // top entries written (those past n: padding)
    if constexpr (RECORD) {
        const int want = a.want[b];
        if (want < 0) return;                                        // off: the row's logits are not touched
        const int gen = a.state[b * 8 + 4];
        if (gen < 1 || gen <= a.n_rec[b] || gen > a.ids_ld) return;  // nothing accepted this step (finished earlier, empty slot)
        n = min(want, LP_TOP);
        c = a.gen_ids[(long long)b * a.ids_ld + gen - 1];
        o_lp = (long long)b * a.ids_ld + gen - 1;
        o_top = o_lp * LP_TOP;
        n_write = LP_TOP;
        n_done = gen;                        // n_rec[b] is written at the very end: every thread of the row has to see the old value here
    } else {
        n = a.top_n;
        c = a.ids[b];
        o_lp = b;
        o_top = (long long)b * a.top_ld;
        n_write = n;
    }
    const uint16_t* row = a.logits + (long long)b * a.ld;
    const bool vec = ((uintptr_t)row & 15) == 0;
    if (tid == 0) { s_floor = -1; s_cnt = 0; }
    if (tid < LP_TOP) s_top[tid] = 0ull;

    // 1. m (the finite test is spelled out: a max alone would drop a quiet NaN but not +inf, and a signalling NaN poisons it)
    float tm = -INFINITY;
    lp_for_row(row, V, vec, [&](int, const uint32_t (&e)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) tm = fmaxf(tm, lp_finite(e[j]) ? lp_value(e[j]) : -INFINITY);
    });
    tm = lp_wave_maxf(tm);
    if (lane == 0) s_wf[wave] = tm;
    __syncthreads();
    float m = s_wf[0];
    for (int w = 1; w < LP_NW; ++w) m = fmaxf(m, s_wf[w]);
    if (m == -INFINITY) {      // no finite entry: -inf everywhere
        if (tid == 0) {
            a.lp[o_lp] = -INFINITY;
            if constexpr (RECORD) a.n_rec[b] = n_done;
        }
        if (tid < n_write) { a.top_ids[o_top + tid] = -1; a.top_lp[o_top + tid] = -INFINITY; }
        return;
    }
    // floor: the n-th largest wave maximum (made distinct by the wave's number); fewer than n waves with a finite entry: none, every entry passes
    if (n > 0 && tid < LP_NW) {
        const int own = lp_wave_word(s_wf[tid], tid);
        int rank = 0;
        for (int w = 0; w < LP_NW; ++w) rank += lp_wave_word(s_wf[w], w) > own;
        if (own != 0 && rank == n - 1) s_floor = (own >> 4) - 1;
    }
    __syncthreads();           // (s_wf is reused for the sum)

    // 2. S (+ the threads' lists)
    unsigned long long t[LP_TOP];
#pragma unroll
    for (int j = 0; j < LP_TOP; ++j) t[j] = 0ull;
    float s = 0.f;
    if (n > 0) {
        const float fl = s_floor < 0 ? -INFINITY : sp_val(s_floor);
        lp_for_row(row, V, vec, [&](int i0, const uint32_t (&e)[8]) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = lp_value(e[j]);
                s += lp_weight(v - m);
                if (v >= fl && lp_finite(e[j])) lp_insert(t, lp_word(e[j], i0 + j));
            }
        });
#pragma unroll
        for (int j = 0; j < LP_TOP; ++j)
            if (t[j] != 0ull) {
                const int slot = atomicAdd(&s_cnt, 1);
                if (slot < LP_CAND) s_cand[slot] = t[j];
            }
    } else {
        lp_for_row(row, V, vec, [&](int, const uint32_t (&e)[8]) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s += lp_weight(lp_value(e[j]) - m);
        });
    }
    {
        const float q = sp_scan_f(s, lane);
        if (lane == 63) s_wf[wave] = q;
    }
    __syncthreads();
    float S = 0.f;
    for (int w = 0; w < LP_NW; ++w) S += s_wf[w];
    const float log_s = logf(S);

    // 3. the top-n, in order
    if (n > 0) {
        const int cnt = s_cnt;
        if (cnt <= LP_CAND) {
            if (tid < cnt) {
                const unsigned long long w = s_cand[tid];
                int rank = 0;
                for (int j = 0; j < cnt; ++j) rank += s_cand[j] > w;
                if (rank < n) s_top[rank] = w;
            }
        } else {
            for (int r = 0; r < n; ++r) {
                const unsigned long long wm = lp_wave_max64(t[0]);
                if (lane == 0) s_w64[r & 1][wave] = wm;
                __syncthreads();
                unsigned long long win = s_w64[r & 1][0];
                for (int w = 1; w < LP_NW; ++w) win = s_w64[r & 1][w] > win ? s_w64[r & 1][w] : win;
                if (tid == 0) s_top[r] = win;
                if (win != 0ull && t[0] == win) {      // one thread: an index sits in one thread's list
#pragma unroll
                    for (int j = 0; j + 1 < LP_TOP; ++j) t[j] = t[j + 1];
                    t[LP_TOP - 1] = 0ull;
                }
            }
        }
        __syncthreads();
    }
    if (tid < n_write) {
        const unsigned long long w = tid < n ? s_top[tid] : 0ull;
        const bool have = w != 0ull;
        a.top_ids[o_top + tid] = have ? (int)~(uint32_t)w : -1;
        a.top_lp[o_top + tid] = have ? (sp_val((int)(w >> 32) - 1) - m) - log_s : -INFINITY;
    }
    if (tid == 0) {
        float lp = -INFINITY;
        if (c >= 0 && c < V) {      // an id outside the row is never a read
            const uint32_t e = row[c];
            if (lp_finite(e)) lp = (lp_value(e) - m) - log_s;
        }
        a.lp[o_lp] = lp;
        if constexpr (RECORD) a.n_rec[b] = n_done;
    }
}

template <bool RECORD>
static int launch_logprob(const LogprobArgs& a, int B, hipStream_t st) {
    FO1_LAUNCH(RECORD ? "logprob_record" : "logprob_rows", (double)B * a.V * 4.0, (logprob_rows_kernel<RECORD>), dim3(B), dim3(LP_NT), 0, st, a);
    return FO1_OK;
}

static int check_logprob(const char* who, const void* logits, long long ld, int V, int B, bool operands) {
    FO1_CHECK_ARG(logits && operands, "%s: NULL operand", who);
    FO1_CHECK_ARG(B >= 1 && B <= 256, "%s: B=%d (1..256)", who, B);
    FO1_CHECK_ARG(V >= 1 && ld >= V, "%s: n_vocab=%d ld_logits=%lld", who, V, ld);
    return FO1_OK;
}

}  // namespace fo1

extern "C" {

// The rows form (see the head of this file and include/fo1.h): row b's chosen id is ids[b]; top_n entries per row to top_*_out[b * top_ld + k].
int fo1_logprob_rows_bf16(const void* logits, long long ld_logits, int n_vocab, int B, const int32_t* ids, int top_n, float* lp_out,
                          int32_t* top_ids_out, float* top_lp_out, long long top_ld, void* stream) {
    using namespace fo1;
    if (int rc = check_logprob("logprob_rows", logits, ld_logits, n_vocab, B, ids && lp_out)) return rc;
    FO1_CHECK_ARG(top_n >= 0 && top_n <= LP_TOP, "logprob_rows: top_n=%d (0..%d)", top_n, LP_TOP);
    FO1_CHECK_ARG(top_n == 0 || (top_ids_out && top_lp_out), "logprob_rows: NULL top output with top_n=%d", top_n);
    FO1_CHECK_ARG(top_n == 0 || top_ld >= top_n, "logprob_rows: top_ld=%lld < top_n=%d", top_ld, top_n);
    LogprobArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.lp = lp_out; a.top_ids = (int*)top_ids_out; a.top_lp = top_lp_out;
    a.ids = (const int*)ids; a.top_n = top_n; a.top_ld = top_ld;
    return launch_logprob<false>(a, B, (hipStream_t)stream);
}

// The decode form: launched after the step's head on the same stream.  Row b with want[b] >= 0 whose state[b][4] = n has advanced past
// n_rec[b] (and n <= ids_ld) scores ids[b][n - 1] on this step's logits into column n - 1 of lp / top_ids / top_lp and sets n_rec[b] = n;
// every other row writes nothing.
int fo1_decode_logprob_record(const void* logits, long long ld_logits, int n_vocab, int B, const int32_t* want, const int32_t* state,
                              const int32_t* ids, int ids_ld, int32_t* n_rec, float* lp, int32_t* top_ids, float* top_lp, void* stream) {
    using namespace fo1;
    if (int rc = check_logprob("decode_logprob_record", logits, ld_logits, n_vocab, B, want && state && ids && n_rec && lp && top_ids && top_lp))
        return rc;
    FO1_CHECK_ARG(ids_ld > 0, "decode_logprob_record: ids_ld=%d", ids_ld);
    LogprobArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.lp = lp; a.top_ids = (int*)top_ids; a.top_lp = top_lp;
    a.want = (const int*)want; a.state = (const int*)state; a.gen_ids = (const int*)ids; a.ids_ld = ids_ld; a.n_rec = (int*)n_rec;
    return launch_logprob<true>(a, B, (hipStream_t)stream);
}

}  // extern "C"
