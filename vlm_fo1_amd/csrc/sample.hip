// sample.hip — temperature / top-k / top-p sampling of one token per bf16 logits row, on the device.
//
// Reference: HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax -> multinomial, which the reference's
// generate runs whenever temperature != 0 (mm_utils.py:632-650).  Definition (the same distribution; ties at a cut-off are all kept, the
// generator is Philox4x32-10): with m the largest finite logit and w_i = exp((l_i - m) / T) (0 for a non-finite entry, which is never kept),
//   K1 = { i : top_k == 0 or #{ j : l_j > l_i } < top_k },  Z1 = sum_K1 w,
//   K  = { i in K1 : top_p >= 1 or sum_{j in K1, l_j > l_i} w_j < top_p Z1 },  Z2 = sum_K w,
//   pick = the smallest i in K, in vocabulary order, with sum_{j in K, j <= i} w_j > u Z2 (else the last index of K).
//
// One workgroup of 1024 threads (16 waves of 64) per row, everything in LDS, no float atomics, no host read, one launch whatever the data:
//   1. one pass over the row: the largest finite key, and a count per order-preserving 16-bit key of the non-negative half (LDS integer atomics;
//      bf16 has 65 536 values, one sign half = 32 768 counters = 128 KB of the 160 KB);
//   2. key scan from the top key down: thread t owns 32 consecutive keys, mass of a key = count x exp((value - m) / T) (the count is an exact
//      integer, one exp per key), fixed-order sums (32 keys in a thread, shuffle scan over the 64 threads of a wave, the 16 waves in order) — the
//      top-k cut-off key falls out of the counts exactly, and the exclusive mass in front of every 32-key range is kept;
//   3. unless the top-k cut-off already fell in the upper half: the same for the negative half (second pass over the row);
//   4. the top-p cut-off: the 32-key range whose masses straddle top_p Z1, then the key inside it (from the counts still in LDS, or from a
//      32-counter pass over the row when they belong to the half that was overwritten);
//   5. the pick, in vocabulary order: wave w owns a contiguous region, walks it in slices of 512 tokens (8 per lane), sums the kept weights
//      (8 in a lane in order, shuffle scan over the lanes, slices in order), the 16 regions in order give Z2; the wave whose region straddles
//      u Z2 walks it again to the slice, the lane and the token.  Prefixes are fp32, the comparison against u Z2 is made in fp64 (u has 25
//      significant bits: its product with an fp32 Z2 is exact there), so flat rows reproduce floor(u V) bit for bit.
// top_k == 0 and top_p >= 1 skip 1's counters and 2-4 altogether.
//
// The general head (PEN instantiations: fo1_sample_rows_seen_bf16, fo1_decode_head_accept) reads two more words of a row's parameters.  A
// repetition penalty p (on iff finite, > 0, != 1) replaces the logit of every token whose bit is set in the row's `seen` bitmap by
// l' = bf16_rne(l < 0 ? l * p : l / p) wherever a pass reads a key (sp_load8p: a lane's 8 logits and the matching byte of the bitmap), so every
// pass still works on the 65 536 bf16 values; a penalised value that is not finite has no key.  A row with FO1_SAMPLE_GREEDY takes pass 1 without
// counters and a first-index reduction, then leaves: the first index, in vocabulary order, of the largest (penalised) finite entry.  Both are
// behind the template parameter: the plain instantiations compile to the code they were before it existed.
//
// The ruled head (RULE instantiations: fo1_sample_rows_ruled_bf16, fo1_decode_head_ruled_accept) reads one fo1_token_rule_t per row and resolves
// it, once per workgroup, to the rows of the mask table live at this pick, at most three (bitmaps in the seen bitmap's layout, a set bit = token banned): `always_row`,
// `early_row` while the row's counter c < early_until, `first_row` while c == 0; a row index outside the table means none.  Wherever a pass loads
// a lane's 8 logits it also loads the matching byte of each active mask row, ORs them and replaces the banned entries by a NaN (no key) BEFORE
// the penalty and the keying: a banned token is a non-finite entry to every pass — weight 0, never kept, never the greedy pick.  A row with
// nothing left gives id 0, as a row without a finite entry does.  Behind a template parameter of its own, as the penalty is.
//
// The guided head (GUIDE instantiations: fo1_sample_rows_guided_bf16, fo1_decode_head_guided_accept) adds a per-row automaton state gstate[b]
// and one fo1_token_guide_t per row.  For a guided row (cls_row inside the class table) the mask row state_row[row_off + gstate[b]] takes
// `always_row`'s place among the three mask pointers, resolved once per workgroup as the rule is; every pass is the ruled head's.  After the
// pick thread 0 loads cls[tok] and next[next_off + s * C + cls], issues the accept, and stores the new state (a negative entry keeps the old
// one).  Every index read from a table is checked against the table's size first: a corrupt table gives a row without a mask or a state that
// stays, never a read out of range.  A finished row and a row without a guide leave gstate alone.
//
// The closing head (CLOSE instantiations: fo1_sample_rows_closing_bf16, fo1_decode_head_closing_accept) reads one fo1_guide_close_t per row.
// With r = budget - c - 1 tokens still to follow this pick, a guided row with 0 <= r < depth takes close_row[close_off + s * depth + r] as its
// state's mask row instead of state_row[row_off + s]: two more scalar table reads where the guide is resolved, nothing else.  An index outside
// close_row keeps the plain row.
//
// The steered head (STEER instantiations: fo1_sample_rows_steered_bf16, fo1_decode_head_steered_accept) reads one fo1_token_steer_t per row
// { bias_row, frequency_penalty f, presence_penalty q } and resolves it, once per workgroup, to a row of the bias table (bf16, a zero entry =
// no bias; bias_row outside the table: none) and, when f and q are both finite and not both zero, the row's generated-token counts (uint16).
// Each table has a gate bitmap beside it in the seen bitmap's layout — a set bit = the entry may be non-zero — so a pass pays one byte per 8
// tokens and loads an entry only behind a set bit.  For a finite logit l, in this order (sp_load8p, after the ban):
//   bias (b != 0):    x = bf16_rne(fp32(l) + fp32(b));           then the repetition penalty on x, as above;
//   counts (n > 0):   t = f * n, t = t + q, x = bf16_rne(x - t)  — three separately rounded fp32 operations, no fused multiply-add.
// A result that is not finite has no key, and no later step touches it.  In the accept form thread 0 adds 1 to the accepted token's count
// (saturating) and sets its gate bit where it sets the seen bit.
#include "decode_common.h"

namespace fo1 {

constexpr int SP_NT = 1024;                 // threads per workgroup
constexpr int SP_NW = SP_NT / 64;           // waves
constexpr int SP_HALF = 32768;              // keys per sign half
constexpr int SP_KPT = SP_HALF / SP_NT;     // keys per thread in the key scan (32)
constexpr int SP_SLICE = 512;               // tokens per wave slice of the pick: 8 per lane
constexpr int SP_SMEM = SP_HALF * 4 + (2 * SP_NT + 4) * 4;      // counters + the exclusive mass in front of every 32-key range (+ the total)

// counter slot of a half's key: rotated inside each thread's 32-key range, so the 64 threads of a wave walking their ranges hit 32 banks
__device__ __forceinline__ int sp_slot(int local) { return (local & ~31) | ((local + (local >> 5)) & 31); }

__device__ __forceinline__ float sp_weight(int key, float m, float inv_t) { return expf((sp_val(key) - m) * inv_t); }

// what the penalty needs of a row: its seen bitmap (bytes: bit j of byte i0 / 8 = token i0 + j, i0 a multiple of 8) and p; seen == NULL: off
struct SpPen {
    const uint8_t* seen;
    float p;
};

// the penalised logit of a seen token with a finite logit: bf16_rne(l < 0 ? l * p : l / p), IEEE fp32 arithmetic
__device__ __forceinline__ uint32_t sp_penalise(uint32_t b, float p) {
    if ((b & 0x7f80u) == 0x7f80u) return b;
    const float l = __uint_as_float(b << 16);
    return (uint32_t)f32_to_bf16(l < 0.f ? l * p : __fdiv_rn(l, p));
}

// what the rule needs of a row: the mask rows live at this pick (bytes, as SpPen::seen).  live == false: none; else all three pointers are
// valid — a field without a live row repeats a live one (OR is idempotent), so a pass issues its three byte loads without a branch between them
struct SpRule {
    const uint8_t* m[3];
    bool live;
};

// what thread 0 of a guided row needs after the pick: the class row, the state's row of `next`, its entries inside the table (0: no advance)
struct SpGuide {
    const uint16_t* cls;
    const int* next;
    int cmax;
};

// what the steer needs of a row: its bias row with the gate bitmap (bgate == NULL: no bias) and its count row with the gate bitmap and the
// two penalties (cgate == NULL: the count penalty is off).  Gates are bytes, as SpPen::seen
struct SpSteer {
    const uint16_t* bias;
    const uint8_t* bgate;
    const uint16_t* cnt;
    const uint8_t* cgate;
    float f, q;
    bool bvec, cvec;      // the bias row / the count row is 16-byte aligned (sp_load8's vector path)
};

// the biased logit: bf16_rne(fp32(l) + fp32(b)); a non-finite entry and a zero bias (0 or -0) leave the entry alone
__device__ __forceinline__ uint32_t sp_bias(uint32_t e, uint32_t b) {
    if ((e & 0x7f80u) == 0x7f80u || (b & 0x7fffu) == 0u) return e;
    return (uint32_t)f32_to_bf16(__fadd_rn(__uint_as_float(e << 16), __uint_as_float(b << 16)));
}

// the count-penalised logit of a token generated n > 0 times: bf16_rne(x - (f * n + q)), every operation rounded on its own.  hipcc contracts
// a * b + c into a fused multiply-add by default, also through __fmul_rn / __fadd_rn (plain operators in this toolchain): the pragma takes
// the licence away from the operations of this block, and the product is rounded before the sum sees it
__device__ __forceinline__ uint32_t sp_count(uint32_t e, float f, float q, uint32_t n) {
#pragma clang fp contract(off)
    if ((e & 0x7f80u) == 0x7f80u || n == 0u) return e;
    float t = f * (float)n;
    t = t + q;
    return (uint32_t)f32_to_bf16(__uint_as_float(e << 16) - t);
}

// sp_load8; RULE: banned tokens come back as a NaN (no key); STEER: biased tokens come back as their biased logit, tokens generated before as
// their count-penalised one; PEN: seen tokens come back as their penalised logit, so every pass keys the same
// 16-bit values
template <bool PEN, bool RULE, bool STEER = false>
__device__ __forceinline__ void sp_load8p(const uint16_t* __restrict__ row, const SpPen& pen, const SpRule& rule, const SpSteer& steer, int i0,
                                          int V, bool vec, uint32_t (&e)[8]) {
    uint32_t ban = 0u;
    [[maybe_unused]] uint32_t bbits = 0u, cbits = 0u;
    if constexpr (STEER) {     // the gate bytes, in front of the logits' load as the mask bytes are: one latency, not three in a row
        const int i = min(i0, V - 1) >> 3;      // (byte < ceil(V / 8) <= 4 gate_ld_words: inside the gate row)
        if (steer.bgate) bbits = steer.bgate[i];
        if (steer.cgate) cbits = steer.cgate[i];
    }
    if constexpr (RULE) {      // in front of the logits' load: the loads are in flight together
        if (rule.live) {
            const int i = min(i0, V - 1) >> 3;      // (byte < ceil(V / 8) <= 4 mask_ld_words: inside the mask row; past the row's end the entries are NaN already)
            ban = (uint32_t)rule.m[0][i] | rule.m[1][i] | rule.m[2][i];
        }
    }
    sp_load8(row, i0, V, vec, e);
    if constexpr (RULE) {
        if (ban) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((ban >> j) & 1u) e[j] = 0x7fc0u;
        }
    }
    if constexpr (STEER) {
        if (bbits) {      // some entry of this group may be non-zero: the group's 8 entries in one load (past the row's end the logits are NaN already)
            uint32_t bv[8];
            sp_load8(steer.bias, i0, V, steer.bvec, bv);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((bbits >> j) & 1u) e[j] = sp_bias(e[j], bv[j]);      // (an entry behind a clear bit counts as zero)
        }
    }
    if constexpr (PEN) {
        if (pen.seen) {
            const uint32_t bits = i0 < V ? pen.seen[i0 >> 3] : 0u;
            if (bits) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if ((bits >> j) & 1u) e[j] = sp_penalise(e[j], pen.p);
            }
        }
    }
    if constexpr (STEER) {
        if (cbits) {
            uint32_t cv[8];
            sp_load8(steer.cnt, i0, V, steer.cvec, cv);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((cbits >> j) & 1u) e[j] = sp_count(e[j], steer.f, steer.q, cv[j]);
        }
    }
}

// every key of the row, 8 tokens per thread and step (any order: the callers count or take a maximum)
template <bool PEN, bool RULE, bool STEER, class F>
__device__ __forceinline__ void sp_for_row(const uint16_t* __restrict__ row, const SpPen& pen, const SpRule& rule, const SpSteer& steer, int V,
                                           bool vec, F f) {
    for (int i0 = threadIdx.x * 8; i0 < V; i0 += SP_NT * 8) {
        uint32_t e[8];
        sp_load8p<PEN, RULE, STEER>(row, pen, rule, steer, i0, V, vec, e);
#pragma unroll
        for (int j = 0; j < 8; ++j) f(sp_key(e[j]));
    }
}

__device__ __forceinline__ int sp_scan_i(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
__device__ __forceinline__ int sp_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int sp_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// word 0 of Philox4x32-10 (Salmon et al., SC'11) for ctr = {c0, c1, 0, 0}, key = {k0, k1}
__device__ __forceinline__ uint32_t sp_philox_x0(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1) {
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

struct SampleArgs {
    const uint16_t* logits; long long ld; int V;
    const fo1_sample_params_t* params;
    const int* counter; int counter_stride;     // rows form: NULL = 0
    const float* u;                             // rows form: explicit draws, NULL = Philox
    int* out;                                   // rows form: [B]
    int* state; int* plan; int* ids_out; int ids_ld; const int* stop_ids; int n_stop; int* done;     // accept form
    uint32_t* seen; long long ld_words;         // general head: the seen bitmap [rows][ld_words] (NULL: no row has a penalty)
    const uint32_t* masks; int mask_rows; long long mask_ld_words; const fo1_token_rule_t* rules;      // ruled head: the mask table and the rows' rules
    const uint16_t* cls; int cls_rows; long long ld_cls; const int* next; long long n_next;            // guided head: token classes, transitions,
    const int* state_row; long long n_state_row; const fo1_token_guide_t* guides; int* gstate;         // state -> mask row, the rows' guides and states
    const int* close_row; long long n_close_row; const fo1_guide_close_t* closes; const int* budget;   // closing head: (state, tokens left) -> mask row, the rows' closing rules, rows form: their budgets
    const uint16_t* bias; const uint32_t* bias_gate; int bias_rows; long long ld_bias;                 // steered head: the bias table and its gate bitmaps,
    uint16_t* counts; uint32_t* count_gate; long long ld_counts; long long gate_ld_words;              // the rows' counts [rows][ld_counts] and their gate bitmaps,
    const fo1_token_steer_t* steers;                                                                   // the rows' steers
};

// Key scan of the half whose counters sit in `hist` (keys key0 .. key0 + 32767), top key down.  carry_c / carry_m: tokens and mass of the
// keys above this half.  Writes the exclusive mass in front of every thread's 32-key range to summ[0 .. 1024); at a top-k crossing (the key
// where the token count reaches top_k) its thread writes the key and the mass down to and including it.  Returns the half's totals.
__device__ __forceinline__ void sp_key_scan(const uint32_t* hist, int key0, int carry_c, float carry_m, float m, float inv_t, int top_k,
                                            float* summ, int* s_wc, float* s_wm, int* s_kcut_k, float* s_z1, int& tot_c, float& tot_m) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int top = SP_HALF - 1 - tid * SP_KPT;     // this thread's largest local key
    int cnt = 0;
    float mass = 0.f;
    for (int j = 0; j < SP_KPT; ++j) {
        const uint32_t c = hist[sp_slot(top - j)];
        if (c) { cnt += (int)c; mass += (float)c * sp_weight(key0 + top - j, m, inv_t); }
    }
    const int ic = sp_scan_i(cnt, lane);
    const float im = sp_scan_f(mass, lane);
    float pm = __shfl_up(im, 1, 64);
    if (lane == 0) pm = 0.f;
    if (lane == 63) { s_wc[wave] = ic; s_wm[wave] = im; }
    __syncthreads();
    int oc = carry_c;
    float om = carry_m;
    for (int w = 0; w < wave; ++w) { oc += s_wc[w]; om += s_wm[w]; }
    const int ex_c = oc + (ic - cnt);
    const float ex_m = om + pm;
    summ[tid] = ex_m;
    tot_c = carry_c;
    tot_m = carry_m;
    for (int w = 0; w < SP_NW; ++w) { tot_c += s_wc[w]; tot_m += s_wm[w]; }
    if (top_k > 0 && ex_c < top_k && ex_c + cnt >= top_k) {      // one thread at most: the counts are exact
        int n = ex_c;
        float M = ex_m;
        for (int j = 0; j < SP_KPT; ++j) {
            const uint32_t c = hist[sp_slot(top - j)];
            if (!c) continue;
            M += (float)c * sp_weight(key0 + top - j, m, inv_t);
            n += (int)c;
            if (n >= top_k) { *s_kcut_k = key0 + top - j; *s_z1 = M; break; }
        }
    }
    __syncthreads();
}

template <bool ACCEPT, bool PEN, bool RULE = false, bool GUIDE = false, bool CLOSE = false, bool STEER = false>
__global__ __launch_bounds__(SP_NT) void sample_rows_kernel(SampleArgs a) {
    extern __shared__ __align__(16) unsigned char sp_smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(sp_smem);
    float* summ = reinterpret_cast<float*>(sp_smem + SP_HALF * 4);      // [2][1024] + total
    __shared__ int s_wi[SP_NW], s_wl[SP_NW], s_wc[SP_NW];
    __shared__ float s_wm[SP_NW];
    __shared__ int s_kcut_k, s_range, s_kcut_p, s_tok;
    __shared__ float s_z1;
    [[maybe_unused]] __shared__ SpGuide s_gd;      // GUIDE only (thread 0 writes and reads it)

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V;
    int* st = ACCEPT ? a.state + b * 8 : nullptr;
    if (ACCEPT && st[3]) {      // a finished row: nothing recorded, state untouched, a valid embedding row published (whatever its logits hold)
        if (tid == 0) accept_token(0, st, a.plan + 2 * b, a.ids_out + (long long)b * a.ids_ld, a.ids_ld, a.stop_ids, a.n_stop, a.done);
        return;
    }
    const uint16_t* row = a.logits + (long long)b * a.ld;
    const bool vec = ((uintptr_t)row & 15) == 0;
    const fo1_sample_params_t P = a.params[b];
    float T = P.temperature;
    int top_k = P.top_k < 0 ? 0 : P.top_k;
    if (!(T > 0.f) || !(T < INFINITY) || !(1.0f / T < INFINITY)) { T = 1.f; top_k = 1; }      // not a temperature (or one so small that 1 / T overflows): the greedy pick
    const bool use_p = P.top_p > 0.f && P.top_p < 1.f;               // anything else (NaN included): no nucleus cut
    const float inv_t = 1.0f / T;
    const bool greedy = PEN && (P.flags & FO1_SAMPLE_GREEDY);
    const bool cut = !greedy && (top_k > 0 || use_p);
    SpPen pen{nullptr, 1.f};
    if constexpr (PEN) {
        const float rp = P.repetition_penalty;
        if (a.seen && rp > 0.f && rp < INFINITY && rp != 1.f) {
            pen.seen = reinterpret_cast<const uint8_t*>(a.seen + (long long)b * a.ld_words);
            pen.p = rp;
        }
    }
    SpSteer steer{nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, false, false};
    if constexpr (STEER) {      // the row's bias row and count row (uniform per row); a bias_row outside the table: no bias
        const fo1_token_steer_t S = a.steers[b];
        if (a.bias && a.bias_gate && S.bias_row >= 0 && S.bias_row < a.bias_rows) {
            steer.bias = a.bias + (long long)S.bias_row * a.ld_bias;
            steer.bgate = reinterpret_cast<const uint8_t*>(a.bias_gate + (long long)S.bias_row * a.gate_ld_words);
            steer.bvec = ((uintptr_t)steer.bias & 15) == 0;
        }
        const float f = S.frequency_penalty, q = S.presence_penalty;
        if (a.counts && a.count_gate && fabsf(f) < INFINITY && fabsf(q) < INFINITY && (f != 0.f || q != 0.f)) {
            steer.cnt = a.counts + (long long)b * a.ld_counts;
            steer.cgate = reinterpret_cast<const uint8_t*>(a.count_gate + (long long)b * a.gate_ld_words);
            steer.cvec = ((uintptr_t)steer.cnt & 15) == 0;
            steer.f = f;
            steer.q = q;
        }
    }
    SpRule rule{{nullptr, nullptr, nullptr}, false};
    if constexpr (GUIDE) {
        if (tid == 0) s_gd.cmax = 0;
    }
    if constexpr (RULE) {      // the mask rows live at this pick (uniform per row); an index outside the table: none
        const fo1_token_rule_t R = a.rules[b];
        const int c = ACCEPT ? st[4] : (a.counter ? a.counter[(long long)b * a.counter_stride] : 0);
        int row0 = R.always_row;
        if constexpr (GUIDE) {      // a guided row: the mask row of its state instead (the host folded the sequence's own bans into it)
            const fo1_token_guide_t G = a.guides[b];
            if (G.cls_row >= 0 && G.cls_row < a.cls_rows && G.n_classes > 0 && G.next_off >= 0 && G.row_off >= 0) {
                const int gs = a.gstate[b];
                const long long ri = (long long)G.row_off + gs;
                row0 = gs >= 0 && ri < a.n_state_row ? a.state_row[ri] : -1;
                if constexpr (CLOSE) {      // fewer than `depth` tokens may follow this pick: the row of (state, tokens left) instead
                    if (!STEER || a.closes) {      // (the steered head also takes a batch without closing rules)
                        const fo1_guide_close_t K = a.closes[b];
                        const int left = (ACCEPT ? min(st[5], a.ids_ld) : a.budget[b]) - c - 1;
                        if (K.depth > 0 && K.close_off >= 0 && gs >= 0 && left >= 0 && left < K.depth) {
                            const long long ci = (long long)K.close_off + (long long)gs * K.depth + left;
                            if (ci < a.n_close_row) row0 = a.close_row[ci];
                        }
                    }
                }
                // what thread 0 needs after the pick waits in LDS, not in registers across the passes: the token's class row, the state's
                // row of `next` and how many of its entries lie inside the table (0: the state stays)
                const long long nb = (long long)G.next_off + (long long)gs * G.n_classes;
                if (tid == 0 && gs >= 0 && nb < a.n_next) {
                    s_gd.cls = a.cls + (long long)G.cls_row * a.ld_cls;
                    s_gd.next = a.next + nb;
                    s_gd.cmax = (int)min((long long)G.n_classes, a.n_next - nb);
                }
            }
        }
        const int rows3[3] = {row0, c < R.early_until ? R.early_row : -1, c == 0 ? R.first_row : -1};
        int any = -1;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (rows3[r] >= 0 && rows3[r] < a.mask_rows) any = rows3[r];
        rule.live = any >= 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int k = rows3[r] >= 0 && rows3[r] < a.mask_rows ? rows3[r] : any;
            if (rule.live) rule.m[r] = reinterpret_cast<const uint8_t*>(a.masks + (long long)k * a.mask_ld_words);
        }
    }

    // 1. largest finite key (+ the non-negative half's counters)
    if (tid == 0) { s_kcut_k = -1; s_range = 0x7fffffff; s_kcut_p = 0; s_tok = 0; s_z1 = 0.f; }
    if (cut)
        for (int i = tid; i < SP_HALF; i += SP_NT) hist[i] = 0;
    __syncthreads();
    int kmax = -1;
    if (cut)
        sp_for_row<PEN, RULE, STEER>(row, pen, rule, steer, V, vec, [&](int k) {
            kmax = max(kmax, k);
            if (k >= 0x8000) atomicAdd(&hist[sp_slot(k & 0x7fff)], 1u);
        });
    else
        sp_for_row<PEN, RULE, STEER>(row, pen, rule, steer, V, vec, [&](int k) { kmax = max(kmax, k); });
    kmax = sp_wave_max(kmax);
    if (lane == 0) s_wi[wave] = kmax;
    __syncthreads();
    kmax = s_wi[0];
    for (int w = 1; w < SP_NW; ++w) kmax = max(kmax, s_wi[w]);
    int tok = 0;
    if (greedy) {         // the first index, in vocabulary order, of the largest key (a row without a finite entry: id 0)
        if (kmax >= 0) {
            int first = 0x7fffffff;
            for (int i0 = tid * 8; i0 < V; i0 += SP_NT * 8) {
                uint32_t e[8];
                sp_load8p<PEN, RULE, STEER>(row, pen, rule, steer, i0, V, vec, e);
#pragma unroll
                for (int j = 7; j >= 0; --j)
                    if (sp_key(e[j]) == kmax) first = min(first, i0 + j);
            }
            first = sp_wave_min(first);
            if (lane == 0) s_wl[wave] = first;
            __syncthreads();
            tok = s_wl[0];
            for (int w = 1; w < SP_NW; ++w) tok = min(tok, s_wl[w]);
        }
    } else if (kmax >= 0) {      // (a row without a finite entry: id 0)
        const float m = sp_val(kmax);
        int kcut = 0;
        if (cut) {
            // 2. / 3. key scans, upper half first
            int tot_c = 0;
            float tot_m = 0.f;
            int built = 1;      // the half whose counters are in LDS
            sp_key_scan(hist, 0x8000, 0, 0.f, m, inv_t, top_k, summ, s_wc, s_wm, &s_kcut_k, &s_z1, tot_c, tot_m);
            if (s_kcut_k < 0) {      // no top-k cut-off yet: the negative half (uniform: shared value read after the scan's barrier)
                for (int i = tid; i < SP_HALF; i += SP_NT) hist[i] = 0;
                __syncthreads();
                sp_for_row<PEN, RULE, STEER>(row, pen, rule, steer, V, vec, [&](int k) {
                    if (k >= 0 && k < 0x8000) atomicAdd(&hist[sp_slot(k)], 1u);
                });
                __syncthreads();
                sp_key_scan(hist, 0, tot_c, tot_m, m, inv_t, top_k, summ + SP_NT, s_wc, s_wm, &s_kcut_k, &s_z1, tot_c, tot_m);
                built = 0;
            } else {
                summ[SP_NT + tid] = tot_m;      // (never straddled: top_p Z1 < Z1 <= the upper half's mass)
            }
            if (tid == 0) summ[2 * SP_NT] = tot_m;
            __syncthreads();
            const int kcut_k = max(s_kcut_k, 0);
            const float z1 = s_kcut_k < 0 ? tot_m : s_z1;
            // 4. top-p: the first 32-key range (top down) whose end mass reaches top_p Z1, then the key inside it
            if (use_p) {
                const float thr = P.top_p * z1;
                for (int r = tid; r < 2 * SP_NT; r += SP_NT)
                    if (summ[r + 1] >= thr && !(summ[r] >= thr)) atomicMin(&s_range, r);
                __syncthreads();
                const int r = s_range;
                if (r != 0x7fffffff) {
                    const int half = r < SP_NT ? 1 : 0;
                    const int lo = SP_HALF - SP_KPT - (r & (SP_NT - 1)) * SP_KPT;      // the range's lowest local key
                    const int key_lo = (half ? 0x8000 : 0) + lo;
                    const bool resident = half == built;
                    uint32_t* mini = hist;      // 32 counters, plain order
                    if (!resident) {
                        if (tid < SP_KPT) mini[tid] = 0;
                        __syncthreads();
                        sp_for_row<PEN, RULE, STEER>(row, pen, rule, steer, V, vec, [&](int k) {
                            if (k >= key_lo && k < key_lo + SP_KPT) atomicAdd(&mini[k - key_lo], 1u);
                        });
                        __syncthreads();
                    }
                    if (tid == 0) {
                        float M = summ[r];
                        int kp = key_lo;      // (a range without a token, picked by a last-bit step of the scan: every key above it)
                        for (int j = SP_KPT - 1; j >= 0; --j) {
                            const uint32_t c = resident ? hist[sp_slot(lo + j)] : mini[j];
                            if (!c) continue;
                            if (!(M < thr)) break;
                            kp = key_lo + j;
                            M += (float)c * sp_weight(key_lo + j, m, inv_t);
                        }
                        s_kcut_p = kp;
                    }
                    __syncthreads();
                }
            }
            kcut = max(kcut_k, s_kcut_p);
        }

        // 5. the pick.  u: explicit, or word 0 of Philox(counter, stream; seed)
        double u;
        if (!ACCEPT && a.u) {
            u = (double)a.u[b];
        } else {
            const uint32_t ctr = ACCEPT ? (uint32_t)st[4] : (a.counter ? (uint32_t)a.counter[(long long)b * a.counter_stride] : 0u);
            u = ((double)(sp_philox_x0(ctr, P.stream, P.seed_lo, P.seed_hi) >> 8) + 0.5) * (1.0 / 16777216.0);
        }
        const int region = (((V + SP_NW - 1) / SP_NW) + SP_SLICE - 1) / SP_SLICE * SP_SLICE;      // tokens per wave: whole slices
        const int r0 = wave * region;
        float run = 0.f;
        int lastm = -1;
        for (int s0 = r0; s0 < r0 + region && s0 < V; s0 += SP_SLICE) {
            uint32_t e[8];
            const int i0 = s0 + lane * 8;
            sp_load8p<PEN, RULE, STEER>(row, pen, rule, steer, i0, V, vec, e);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = sp_key(e[j]);
                if (k >= kcut) { s += sp_weight(k, m, inv_t); lastm = i0 + j; }
            }
            run += __shfl(sp_scan_f(s, lane), 63, 64);
        }
        lastm = sp_wave_max(lastm);
        if (lane == 0) { s_wm[wave] = run; s_wl[wave] = lastm; }
        __syncthreads();
        float z2 = 0.f;
        for (int w = 0; w < SP_NW; ++w) z2 += s_wm[w];
        const double target = u * (double)z2;
        int wsel = -1;
        float before = 0.f, acc = 0.f;
        int last_all = -1;
        for (int w = 0; w < SP_NW; ++w) {
            last_all = max(last_all, s_wl[w]);
            if (wsel < 0) {
                before = acc;
                acc += s_wm[w];
                if ((double)acc > target) wsel = w;
            }
        }
        if (wsel < 0) {
            if (tid == 0) s_tok = last_all;      // u Z2 rounds to Z2 (u = 1 - 2^-25 given as fp32): the last index of K
        } else if (wave == wsel) {
            int pick = -1;
            run = 0.f;
            for (int s0 = r0; s0 < r0 + region && s0 < V && pick < 0; s0 += SP_SLICE) {
                uint32_t e[8];
                const int i0 = s0 + lane * 8;
                sp_load8p<PEN, RULE, STEER>(row, pen, rule, steer, i0, V, vec, e);
                float wj[8], s = 0.f;
                int lm = -1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = sp_key(e[j]);
                    wj[j] = k >= kcut ? sp_weight(k, m, inv_t) : -1.f;
                    if (k >= kcut) { s += wj[j]; lm = i0 + j; }
                }
                const float q = sp_scan_f(s, lane);
                const float total = __shfl(q, 63, 64);
                if ((double)(before + (run + total)) > target) {      // this slice (the same sums as above: the last slice ends at `acc`)
                    float qp = __shfl_up(q, 1, 64);
                    if (lane == 0) qp = 0.f;
                    const unsigned long long hit = __ballot((double)(before + (run + q)) > target);
                    if (hit == 0) {
                        pick = sp_wave_max(lm);      // (a rounding gap between the scan's last lane and `total`: none by construction)
                    } else {
                        const int l0 = __ffsll((long long)hit) - 1;
                        int mine = -1;
                        if (lane == l0) {
                            float r8 = 0.f;
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                if (wj[j] < 0.f || mine >= 0) continue;
                                r8 += wj[j];
                                if ((double)(before + (run + (qp + r8))) > target) mine = i0 + j;
                            }
                            if (mine < 0) mine = lm;      // the lane's sum and the scan's value differ in the last bit: its last kept token
                        }
                        pick = __shfl(mine, l0, 64);
                    }
                }
                run += total;
            }
            if (pick < 0) pick = s_wl[wave];
            if (lane == 0) s_tok = pick;
        }
        __syncthreads();
        tok = s_tok;
    }
    if (tid == 0) {
        [[maybe_unused]] int ns = -1;
        if constexpr (GUIDE) {      // the state after `tok`: both loads in front of the accept's stores (tok < V <= ld_cls: inside the class row)
            const int cmax = s_gd.cmax;
            if (cmax > 0) {
                const int c = s_gd.cls[tok];
                if (c < cmax) ns = s_gd.next[c];
            }
        }
        if (ACCEPT) {
            // the step that produced this token consumed row `pos`: the NEXT fed token goes one row further (as the greedy head does)
            st[0] += 1; st[1] += 1;
            accept_token(tok, st, a.plan + 2 * b, a.ids_out + (long long)b * a.ids_ld, a.ids_ld, a.stop_ids, a.n_stop, a.done);
            if constexpr (PEN) {      // the accepted token joins the row's seen set (tok < V: an index of the row)
                if (a.seen) atomicOr(a.seen + (long long)b * a.ld_words + (tok >> 5), 1u << (tok & 31));
            }
            if constexpr (STEER) {    // ... and its count goes up by one (this workgroup is the row's only writer; tok < V <= ld_counts)
                if (a.counts && a.count_gate) {
                    uint16_t* cn = a.counts + (long long)b * a.ld_counts + tok;
                    const uint16_t n = *cn;
                    if (n != 0xffffu) *cn = (uint16_t)(n + 1);
                    atomicOr(a.count_gate + (long long)b * a.gate_ld_words + (tok >> 5), 1u << (tok & 31));
                }
            }
        } else {
            a.out[b] = tok;
        }
        if constexpr (GUIDE) {
            if (ns >= 0) a.gstate[b] = ns;      // (a negative entry: the "nothing left gives id 0" fall-back took a banned token, the state stays)
        }
    }
}

constexpr size_t SP_WORKSPACE = 256;      // the one-workgroup-per-row kernel keeps everything in LDS; the argument stays for a split form

template <bool ACCEPT, bool PEN, bool RULE = false, bool GUIDE = false, bool CLOSE = false, bool STEER = false>
static int launch_sample(const SampleArgs& a, int B, hipStream_t st) {
    FO1_DYNAMIC_LDS_ONCE(SP_SMEM, sample_rows_kernel<ACCEPT, PEN, RULE, GUIDE, CLOSE, STEER>);
    FO1_LAUNCH(STEER ? (ACCEPT ? "head_steered_accept" : "sample_rows_steered")
               : CLOSE ? (ACCEPT ? "head_closing_accept" : "sample_rows_closing")
               : GUIDE ? (ACCEPT ? "head_guided_accept" : "sample_rows_guided")
               : RULE ? (ACCEPT ? "head_ruled_accept" : "sample_rows_ruled")
                      : PEN ? (ACCEPT ? "head_accept" : "sample_rows_seen") : (ACCEPT ? "sample_accept" : "sample_rows"),
               (double)B * a.V * 2.0, (sample_rows_kernel<ACCEPT, PEN, RULE, GUIDE, CLOSE, STEER>), dim3(B), dim3(SP_NT), SP_SMEM, st, a);
    return FO1_OK;
}

// (row, id) pairs -> bits of the seen bitmap; ids outside [0, V) and negative rows are skipped
__global__ __launch_bounds__(256) void seen_mark_kernel(uint32_t* __restrict__ seen, long long ld_words, int V, const int* __restrict__ rows,
                                                             const int* __restrict__ ids, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = rows[i], t = ids[i];
    if (r < 0 || t < 0 || t >= V) return;
    atomicOr(seen + (long long)r * ld_words + (t >> 5), 1u << (t & 31));
}

static int check_seen(const char* who, const void* seen, long long ld_words, int V) {
    FO1_CHECK_ARG(!seen || (ld_words % 4 == 0 && ld_words >= ((long long)V + 31) / 32), "%s: ld_words=%lld (a multiple of 4, >= ceil(n_vocab / 32) = %d)", who,
                  ld_words, (V + 31) / 32);
    FO1_CHECK_ARG(!seen || ((uintptr_t)seen & 3) == 0, "%s: seen must be 4-byte aligned", who);
    return FO1_OK;
}

static int check_masks(const char* who, const void* masks, int mask_rows, long long mask_ld_words, int V) {
    FO1_CHECK_ARG(!masks || (mask_ld_words % 4 == 0 && mask_ld_words >= ((long long)V + 31) / 32),
                  "%s: mask_ld_words=%lld (a multiple of 4, >= ceil(n_vocab / 32) = %d)", who, mask_ld_words, (V + 31) / 32);
    FO1_CHECK_ARG(!masks || mask_rows > 0, "%s: mask_rows=%d with a mask table (>= 1)", who, mask_rows);
    FO1_CHECK_ARG(!masks || ((uintptr_t)masks & 3) == 0, "%s: masks must be 4-byte aligned", who);
    return FO1_OK;
}

static int check_guides(const char* who, const void* masks, const void* rules, const void* cls, int cls_rows, long long ld_cls, const void* next,
                        long long n_next, const void* state_row, long long n_state_row, const void* gstate, int V) {
    FO1_CHECK_ARG(masks && rules, "%s: guides need the mask table and the rule table", who);
    FO1_CHECK_ARG(cls && next && state_row && gstate, "%s: guides with a NULL class, transition, state-row or state table", who);
    FO1_CHECK_ARG(cls_rows > 0 && ld_cls >= V, "%s: cls_rows=%d ld_cls=%lld (>= 1 rows of >= n_vocab = %d classes)", who, cls_rows, ld_cls, V);
    FO1_CHECK_ARG(n_next > 0 && n_state_row > 0, "%s: n_next=%lld n_state_row=%lld (>= 1 each)", who, n_next, n_state_row);
    FO1_CHECK_ARG(((uintptr_t)cls & 1) == 0 && (((uintptr_t)next | (uintptr_t)state_row | (uintptr_t)gstate) & 3) == 0, "%s: misaligned guide table", who);
    return FO1_OK;
}

static int check_closes(const char* who, const void* close_row, long long n_close_row, const void* closes) {
    FO1_CHECK_ARG(close_row && n_close_row > 0, "%s: closing rules with close_row=%p n_close_row=%lld (a table of >= 1 entries)", who, close_row, n_close_row);
    FO1_CHECK_ARG((((uintptr_t)close_row | (uintptr_t)closes) & 3) == 0, "%s: misaligned closing table", who);
    return FO1_OK;
}

// (row, id) pairs -> + 1 in the count table and the bit of the gate bitmap; ids outside [0, V) and negative rows are skipped.  Two counts share
// a 32-bit word (rows start on a word: ld_counts is even), so duplicates add up through the word's atomic; a count stays far below 65 536
// (at most IDS_CAP marks reach a row between two clears), so the low half never carries into the high one
__global__ __launch_bounds__(256) void count_mark_kernel(uint32_t* __restrict__ counts, long long ld_count_words, uint32_t* __restrict__ gate,
                                                              long long gate_ld_words, int V, const int* __restrict__ rows, const int* __restrict__ ids,
                                                              int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = rows[i], t = ids[i];
    if (r < 0 || t < 0 || t >= V) return;
    atomicAdd(counts + (long long)r * ld_count_words + (t >> 1), 1u << (16 * (t & 1)));
    atomicOr(gate + (long long)r * gate_ld_words + (t >> 5), 1u << (t & 31));
}

static int check_steers(const char* who, const void* bias, const void* bias_gate, int bias_rows, long long ld_bias, const void* counts,
                        const void* count_gate, long long ld_counts, long long gate_ld_words, int V) {
    FO1_CHECK_ARG(!bias == !bias_gate && !counts == !count_gate, "%s: a bias table and a count table come with their gate bitmaps", who);
    FO1_CHECK_ARG(!(bias || counts) || (gate_ld_words % 4 == 0 && gate_ld_words >= ((long long)V + 31) / 32),
                  "%s: gate_ld_words=%lld (a multiple of 4, >= ceil(n_vocab / 32) = %d)", who, gate_ld_words, (V + 31) / 32);
    FO1_CHECK_ARG(!bias || (bias_rows > 0 && ld_bias >= V), "%s: bias_rows=%d ld_bias=%lld (>= 1 rows of >= n_vocab = %d entries)", who, bias_rows, ld_bias, V);
    FO1_CHECK_ARG(!counts || (ld_counts >= V && ld_counts % 2 == 0), "%s: ld_counts=%lld (even, >= n_vocab = %d)", who, ld_counts, V);
    FO1_CHECK_ARG(((uintptr_t)bias & 1) == 0 && (((uintptr_t)bias_gate | (uintptr_t)counts | (uintptr_t)count_gate) & 3) == 0, "%s: misaligned steer table", who);
    return FO1_OK;
}

static int check_sample(const char* who, const void* logits, long long ld, int V, int B, const void* params, const void* ws, size_t ws_bytes) {
    FO1_CHECK_ARG(logits && params, "%s: NULL operand", who);
    FO1_CHECK_ARG(B >= 1 && B <= 256, "%s: B=%d (1..256)", who, B);
    FO1_CHECK_ARG(V >= 1 && ld >= V, "%s: n_vocab=%d ld_logits=%lld", who, V, ld);
    if (!ws || ws_bytes < SP_WORKSPACE) return set_err(FO1_ERR_WORKSPACE, "%s: workspace %zu bytes < %zu", who, ws ? ws_bytes : (size_t)0, SP_WORKSPACE);
    return FO1_OK;
}

}  // namespace fo1

extern "C" {

size_t fo1_sample_rows_workspace_bytes(int n_vocab, int B) { return n_vocab >= 1 && B >= 1 && B <= 256 ? fo1::SP_WORKSPACE : 0; }

// One sampled id per logits row (see the head of this file).  counter: device int32, element b * counter_stride (NULL = 0);
// u: device fp32 [B] explicit draws instead of Philox (tests).
int fo1_sample_rows_bf16(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, const int32_t* counter,
                         int counter_stride, const float* u, int32_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace fo1;
    if (int rc = check_sample("sample_rows", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    FO1_CHECK_ARG(out != nullptr, "sample_rows: NULL out");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params; a.counter = (const int*)counter;
    a.counter_stride = counter_stride; a.u = u; a.out = (int*)out;
    return launch_sample<false, false>(a, B, (hipStream_t)stream);
}

// The sampled head of a decode step: pick (counter = state[b][4], the number of tokens generated so far) + the bookkeeping of
// fo1_decode_argmax_accept (accept_token).  A finished row records nothing, leaves its state alone and publishes plan[1] = 0.
int fo1_decode_sample_accept(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, int32_t* state,
                             int32_t* plan, int32_t* ids_out, int ids_ld, const int32_t* stop_ids, int n_stop, int32_t* done, void* workspace,
                             size_t workspace_bytes, void* stream) {
    using namespace fo1;
    if (int rc = check_sample("decode_sample_accept", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    FO1_CHECK_ARG(state && plan && ids_out && done && ids_ld > 0 && n_stop >= -1 && (n_stop == 0 || stop_ids), "decode_sample_accept: bad arguments");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params;
    a.state = (int*)state; a.plan = (int*)plan; a.ids_out = (int*)ids_out; a.ids_ld = ids_ld; a.stop_ids = (const int*)stop_ids; a.n_stop = n_stop;
    a.done = (int*)done;
    return launch_sample<true, false>(a, B, (hipStream_t)stream);
}

// fo1_sample_rows_bf16 through the general head: a row's flags (FO1_SAMPLE_GREEDY) and repetition penalty are honoured.  seen: the bitmap
// [rows >= B][ld_words]; NULL is allowed only when no row has the penalty on (the rows are device data: the host cannot check it — a row with
// a penalty and no bitmap is sampled without it).
int fo1_sample_rows_seen_bf16(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, const int32_t* counter,
                              int counter_stride, const float* u, int32_t* out, void* workspace, size_t workspace_bytes, const uint32_t* seen,
                              long long ld_words, void* stream) {
    using namespace fo1;
    if (int rc = check_sample("sample_rows_seen", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen("sample_rows_seen", seen, ld_words, n_vocab)) return rc;
    FO1_CHECK_ARG(out != nullptr, "sample_rows_seen: NULL out");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params; a.counter = (const int*)counter;
    a.counter_stride = counter_stride; a.u = u; a.out = (int*)out; a.seen = const_cast<uint32_t*>(seen); a.ld_words = ld_words;
    return launch_sample<false, true>(a, B, (hipStream_t)stream);
}

// The general head of a decode step: fo1_decode_sample_accept's pick and bookkeeping with the row's flags and penalty honoured; the accepted
// token's bit is set in row b of `seen` (when given).  A finished row touches nothing, its bitmap row included.
int fo1_decode_head_accept(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, int32_t* state,
                           int32_t* plan, int32_t* ids_out, int ids_ld, const int32_t* stop_ids, int n_stop, int32_t* done, void* workspace,
                           size_t workspace_bytes, uint32_t* seen, long long ld_words, void* stream) {
    using namespace fo1;
    if (int rc = check_sample("decode_head_accept", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen("decode_head_accept", seen, ld_words, n_vocab)) return rc;
    FO1_CHECK_ARG(state && plan && ids_out && done && ids_ld > 0 && n_stop >= -1 && (n_stop == 0 || stop_ids), "decode_head_accept: bad arguments");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params;
    a.state = (int*)state; a.plan = (int*)plan; a.ids_out = (int*)ids_out; a.ids_ld = ids_ld; a.stop_ids = (const int*)stop_ids; a.n_stop = n_stop;
    a.done = (int*)done; a.seen = seen; a.ld_words = ld_words;
    return launch_sample<true, true>(a, B, (hipStream_t)stream);
}

// fo1_sample_rows_seen_bf16 with the rows' token rules honoured (the head of this file; include/fo1.h).  rules == NULL or masks == NULL: no row
// has a rule, and the call is fo1_sample_rows_seen_bf16's.
int fo1_sample_rows_ruled_bf16(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, const int32_t* counter,
                               int counter_stride, const float* u, int32_t* out, void* workspace, size_t workspace_bytes, const uint32_t* seen,
                               long long ld_words, const uint32_t* masks, int mask_rows, long long mask_ld_words, const fo1_token_rule_t* rules,
                               void* stream) {
    using namespace fo1;
    if (int rc = check_sample("sample_rows_ruled", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen("sample_rows_ruled", seen, ld_words, n_vocab)) return rc;
    if (int rc = check_masks("sample_rows_ruled", masks, mask_rows, mask_ld_words, n_vocab)) return rc;
    FO1_CHECK_ARG(out != nullptr, "sample_rows_ruled: NULL out");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params; a.counter = (const int*)counter;
    a.counter_stride = counter_stride; a.u = u; a.out = (int*)out; a.seen = const_cast<uint32_t*>(seen); a.ld_words = ld_words;
    if (!masks || !rules) return launch_sample<false, true>(a, B, (hipStream_t)stream);
    a.masks = masks; a.mask_rows = mask_rows; a.mask_ld_words = mask_ld_words; a.rules = rules;
    return launch_sample<false, true, true>(a, B, (hipStream_t)stream);
}

// fo1_decode_head_accept with the rows' token rules honoured (counter = state[b][4]).  rules == NULL or masks == NULL: fo1_decode_head_accept.
// The step reads the mask table and the rules, it never writes them.
int fo1_decode_head_ruled_accept(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, int32_t* state,
                                 int32_t* plan, int32_t* ids_out, int ids_ld, const int32_t* stop_ids, int n_stop, int32_t* done, void* workspace,
                                 size_t workspace_bytes, uint32_t* seen, long long ld_words, const uint32_t* masks, int mask_rows,
                                 long long mask_ld_words, const fo1_token_rule_t* rules, void* stream) {
    using namespace fo1;
    if (int rc = check_sample("decode_head_ruled_accept", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen("decode_head_ruled_accept", seen, ld_words, n_vocab)) return rc;
    if (int rc = check_masks("decode_head_ruled_accept", masks, mask_rows, mask_ld_words, n_vocab)) return rc;
    FO1_CHECK_ARG(state && plan && ids_out && done && ids_ld > 0 && n_stop >= -1 && (n_stop == 0 || stop_ids), "decode_head_ruled_accept: bad arguments");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params;
    a.state = (int*)state; a.plan = (int*)plan; a.ids_out = (int*)ids_out; a.ids_ld = ids_ld; a.stop_ids = (const int*)stop_ids; a.n_stop = n_stop;
    a.done = (int*)done; a.seen = seen; a.ld_words = ld_words;
    if (!masks || !rules) return launch_sample<true, true>(a, B, (hipStream_t)stream);
    a.masks = masks; a.mask_rows = mask_rows; a.mask_ld_words = mask_ld_words; a.rules = rules;
    return launch_sample<true, true, true>(a, B, (hipStream_t)stream);
}

// fo1_sample_rows_ruled_bf16 with the rows' token guides honoured (the head of this file; include/fo1.h): row b picks in state gstate[b] and the
// state after the pick is written back.  guides == NULL: fo1_sample_rows_ruled_bf16.
int fo1_sample_rows_guided_bf16(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, const int32_t* counter,
                                int counter_stride, const float* u, int32_t* out, void* workspace, size_t workspace_bytes, const uint32_t* seen,
                                long long ld_words, const uint32_t* masks, int mask_rows, long long mask_ld_words, const fo1_token_rule_t* rules,
                                void* stream, const uint16_t* cls, int cls_rows, long long ld_cls, const int32_t* next, long long n_next,
                                const int32_t* state_row, long long n_state_row, const fo1_token_guide_t* guides, int32_t* gstate) {
    using namespace fo1;
    if (!guides)
        return fo1_sample_rows_ruled_bf16(logits, ld_logits, n_vocab, B, params, counter, counter_stride, u, out, workspace, workspace_bytes, seen, ld_words,
                                          masks, mask_rows, mask_ld_words, rules, stream);
    if (int rc = check_sample("sample_rows_guided", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen("sample_rows_guided", seen, ld_words, n_vocab)) return rc;
    if (int rc = check_masks("sample_rows_guided", masks, mask_rows, mask_ld_words, n_vocab)) return rc;
    if (int rc = check_guides("sample_rows_guided", masks, rules, cls, cls_rows, ld_cls, next, n_next, state_row, n_state_row, gstate, n_vocab)) return rc;
    FO1_CHECK_ARG(out != nullptr, "sample_rows_guided: NULL out");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params; a.counter = (const int*)counter;
    a.counter_stride = counter_stride; a.u = u; a.out = (int*)out; a.seen = const_cast<uint32_t*>(seen); a.ld_words = ld_words;
    a.masks = masks; a.mask_rows = mask_rows; a.mask_ld_words = mask_ld_words; a.rules = rules;
    a.cls = cls; a.cls_rows = cls_rows; a.ld_cls = ld_cls; a.next = (const int*)next; a.n_next = n_next; a.state_row = (const int*)state_row;
    a.n_state_row = n_state_row; a.guides = guides; a.gstate = (int*)gstate;
    return launch_sample<false, true, true, true>(a, B, (hipStream_t)stream);
}

// fo1_decode_head_ruled_accept with the rows' token guides honoured: the step reads the guide tables and writes gstate, nothing else of them.
// guides == NULL: fo1_decode_head_ruled_accept.
int fo1_decode_head_guided_accept(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, int32_t* state,
                                  int32_t* plan, int32_t* ids_out, int ids_ld, const int32_t* stop_ids, int n_stop, int32_t* done, void* workspace,
                                  size_t workspace_bytes, uint32_t* seen, long long ld_words, const uint32_t* masks, int mask_rows,
                                  long long mask_ld_words, const fo1_token_rule_t* rules, void* stream, const uint16_t* cls, int cls_rows,
                                  long long ld_cls, const int32_t* next, long long n_next, const int32_t* state_row, long long n_state_row,
                                  const fo1_token_guide_t* guides, int32_t* gstate) {
    using namespace fo1;
    if (!guides)
        return fo1_decode_head_ruled_accept(logits, ld_logits, n_vocab, B, params, state, plan, ids_out, ids_ld, stop_ids, n_stop, done, workspace,
                                            workspace_bytes, seen, ld_words, masks, mask_rows, mask_ld_words, rules, stream);
    if (int rc = check_sample("decode_head_guided_accept", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen("decode_head_guided_accept", seen, ld_words, n_vocab)) return rc;
    if (int rc = check_masks("decode_head_guided_accept", masks, mask_rows, mask_ld_words, n_vocab)) return rc;
    if (int rc = check_guides("decode_head_guided_accept", masks, rules, cls, cls_rows, ld_cls, next, n_next, state_row, n_state_row, gstate, n_vocab)) return rc;
    FO1_CHECK_ARG(state && plan && ids_out && done && ids_ld > 0 && n_stop >= -1 && (n_stop == 0 || stop_ids), "decode_head_guided_accept: bad arguments");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params;
    a.state = (int*)state; a.plan = (int*)plan; a.ids_out = (int*)ids_out; a.ids_ld = ids_ld; a.stop_ids = (const int*)stop_ids; a.n_stop = n_stop;
    a.done = (int*)done; a.seen = seen; a.ld_words = ld_words;
    a.masks = masks; a.mask_rows = mask_rows; a.mask_ld_words = mask_ld_words; a.rules = rules;
    a.cls = cls; a.cls_rows = cls_rows; a.ld_cls = ld_cls; a.next = (const int*)next; a.n_next = n_next; a.state_row = (const int*)state_row;
    a.n_state_row = n_state_row; a.guides = guides; a.gstate = (int*)gstate;
    return launch_sample<true, true, true, true>(a, B, (hipStream_t)stream);
}

// fo1_sample_rows_guided_bf16 with the rows' closing rules honoured (the head of this file; include/fo1.h): a guided row b with fewer than
// closes[b].depth tokens left of budget[b] picks behind the mask row of (state, tokens left).  closes == NULL: fo1_sample_rows_guided_bf16.
int fo1_sample_rows_closing_bf16(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, const int32_t* counter,
                                 int counter_stride, const float* u, int32_t* out, void* workspace, size_t workspace_bytes, const uint32_t* seen,
                                 long long ld_words, const uint32_t* masks, int mask_rows, long long mask_ld_words, const fo1_token_rule_t* rules,
                                 void* stream, const uint16_t* cls, int cls_rows, long long ld_cls, const int32_t* next, long long n_next,
                                 const int32_t* state_row, long long n_state_row, const fo1_token_guide_t* guides, int32_t* gstate,
                                 const int32_t* close_row, long long n_close_row, const fo1_guide_close_t* closes, const int32_t* budget) {
    using namespace fo1;
    if (!closes)
        return fo1_sample_rows_guided_bf16(logits, ld_logits, n_vocab, B, params, counter, counter_stride, u, out, workspace, workspace_bytes, seen, ld_words,
                                           masks, mask_rows, mask_ld_words, rules, stream, cls, cls_rows, ld_cls, next, n_next, state_row, n_state_row,
                                           guides, gstate);
    FO1_CHECK_ARG(guides != nullptr, "sample_rows_closing: closing rules need the rows' guides");
    if (int rc = check_sample("sample_rows_closing", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen("sample_rows_closing", seen, ld_words, n_vocab)) return rc;
    if (int rc = check_masks("sample_rows_closing", masks, mask_rows, mask_ld_words, n_vocab)) return rc;
    if (int rc = check_guides("sample_rows_closing", masks, rules, cls, cls_rows, ld_cls, next, n_next, state_row, n_state_row, gstate, n_vocab)) return rc;
    if (int rc = check_closes("sample_rows_closing", close_row, n_close_row, closes)) return rc;
    FO1_CHECK_ARG(out != nullptr, "sample_rows_closing: NULL out");
    FO1_CHECK_ARG(budget && ((uintptr_t)budget & 3) == 0, "sample_rows_closing: closing rules need the rows' budgets (device int32 [B])");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params; a.counter = (const int*)counter;
    a.counter_stride = counter_stride; a.u = u; a.out = (int*)out; a.seen = const_cast<uint32_t*>(seen); a.ld_words = ld_words;
    a.masks = masks; a.mask_rows = mask_rows; a.mask_ld_words = mask_ld_words; a.rules = rules;
    a.cls = cls; a.cls_rows = cls_rows; a.ld_cls = ld_cls; a.next = (const int*)next; a.n_next = n_next; a.state_row = (const int*)state_row;
    a.n_state_row = n_state_row; a.guides = guides; a.gstate = (int*)gstate;
    a.close_row = (const int*)close_row; a.n_close_row = n_close_row; a.closes = closes; a.budget = (const int*)budget;
    return launch_sample<false, true, true, true, true>(a, B, (hipStream_t)stream);
}

// fo1_decode_head_guided_accept with the rows' closing rules honoured: tokens left = min(state[b][5], ids_ld) - state[b][4] - 1.  The step
// reads close_row and closes, it never writes them.  closes == NULL: fo1_decode_head_guided_accept.
int fo1_decode_head_closing_accept(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, int32_t* state,
                                   int32_t* plan, int32_t* ids_out, int ids_ld, const int32_t* stop_ids, int n_stop, int32_t* done, void* workspace,
                                   size_t workspace_bytes, uint32_t* seen, long long ld_words, const uint32_t* masks, int mask_rows,
                                   long long mask_ld_words, const fo1_token_rule_t* rules, void* stream, const uint16_t* cls, int cls_rows,
                                   long long ld_cls, const int32_t* next, long long n_next, const int32_t* state_row, long long n_state_row,
                                   const fo1_token_guide_t* guides, int32_t* gstate, const int32_t* close_row, long long n_close_row,
                                   const fo1_guide_close_t* closes) {
    using namespace fo1;
    if (!closes)
        return fo1_decode_head_guided_accept(logits, ld_logits, n_vocab, B, params, state, plan, ids_out, ids_ld, stop_ids, n_stop, done, workspace,
                                             workspace_bytes, seen, ld_words, masks, mask_rows, mask_ld_words, rules, stream, cls, cls_rows, ld_cls, next,
                                             n_next, state_row, n_state_row, guides, gstate);
    FO1_CHECK_ARG(guides != nullptr, "decode_head_closing_accept: closing rules need the rows' guides");
    if (int rc = check_sample("decode_head_closing_accept", logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen("decode_head_closing_accept", seen, ld_words, n_vocab)) return rc;
    if (int rc = check_masks("decode_head_closing_accept", masks, mask_rows, mask_ld_words, n_vocab)) return rc;
    if (int rc = check_guides("decode_head_closing_accept", masks, rules, cls, cls_rows, ld_cls, next, n_next, state_row, n_state_row, gstate, n_vocab)) return rc;
    if (int rc = check_closes("decode_head_closing_accept", close_row, n_close_row, closes)) return rc;
    FO1_CHECK_ARG(state && plan && ids_out && done && ids_ld > 0 && n_stop >= -1 && (n_stop == 0 || stop_ids), "decode_head_closing_accept: bad arguments");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params;
    a.state = (int*)state; a.plan = (int*)plan; a.ids_out = (int*)ids_out; a.ids_ld = ids_ld; a.stop_ids = (const int*)stop_ids; a.n_stop = n_stop;
    a.done = (int*)done; a.seen = seen; a.ld_words = ld_words;
    a.masks = masks; a.mask_rows = mask_rows; a.mask_ld_words = mask_ld_words; a.rules = rules;
    a.cls = cls; a.cls_rows = cls_rows; a.ld_cls = ld_cls; a.next = (const int*)next; a.n_next = n_next; a.state_row = (const int*)state_row;
    a.n_state_row = n_state_row; a.guides = guides; a.gstate = (int*)gstate;
    a.close_row = (const int*)close_row; a.n_close_row = n_close_row; a.closes = closes;
    return launch_sample<true, true, true, true, true>(a, B, (hipStream_t)stream);
}

// fo1_sample_rows_closing_bf16 with the rows' steers honoured (the head of this file; include/fo1.h): an additive bias row and the frequency /
// presence penalties against the rows' counts.  steers == NULL: fo1_sample_rows_closing_bf16.  With steers, the rule / guide / closing tables
// are optional, each level needing the one before it: no rules, rules, rules + guides, rules + guides + closing rules.
int fo1_sample_rows_steered_bf16(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, const int32_t* counter,
                                 int counter_stride, const float* u, int32_t* out, void* workspace, size_t workspace_bytes, const uint32_t* seen,
                                 long long ld_words, const uint32_t* masks, int mask_rows, long long mask_ld_words, const fo1_token_rule_t* rules,
                                 void* stream, const uint16_t* cls, int cls_rows, long long ld_cls, const int32_t* next, long long n_next,
                                 const int32_t* state_row, long long n_state_row, const fo1_token_guide_t* guides, int32_t* gstate,
                                 const int32_t* close_row, long long n_close_row, const fo1_guide_close_t* closes, const int32_t* budget,
                                 const void* bias, const uint32_t* bias_gate, int bias_rows, long long ld_bias, const uint16_t* counts,
                                 const uint32_t* count_gate, long long ld_counts, long long gate_ld_words, const fo1_token_steer_t* steers) {
    using namespace fo1;
    if (!steers)
        return fo1_sample_rows_closing_bf16(logits, ld_logits, n_vocab, B, params, counter, counter_stride, u, out, workspace, workspace_bytes, seen, ld_words,
                                            masks, mask_rows, mask_ld_words, rules, stream, cls, cls_rows, ld_cls, next, n_next, state_row, n_state_row,
                                            guides, gstate, close_row, n_close_row, closes, budget);
    const char* who = "sample_rows_steered";
    if (int rc = check_sample(who, logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen(who, seen, ld_words, n_vocab)) return rc;
    if (int rc = check_masks(who, masks, mask_rows, mask_ld_words, n_vocab)) return rc;
    if (int rc = check_steers(who, bias, bias_gate, bias_rows, ld_bias, counts, count_gate, ld_counts, gate_ld_words, n_vocab)) return rc;
    FO1_CHECK_ARG(out != nullptr && ((uintptr_t)steers & 3) == 0, "sample_rows_steered: NULL out or misaligned steers");
    FO1_CHECK_ARG(!closes || guides, "sample_rows_steered: closing rules need the rows' guides");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params; a.counter = (const int*)counter;
    a.counter_stride = counter_stride; a.u = u; a.out = (int*)out; a.seen = const_cast<uint32_t*>(seen); a.ld_words = ld_words;
    a.bias = (const uint16_t*)bias; a.bias_gate = bias_gate; a.bias_rows = bias_rows; a.ld_bias = ld_bias; a.counts = const_cast<uint16_t*>(counts);
    a.count_gate = const_cast<uint32_t*>(count_gate); a.ld_counts = ld_counts; a.gate_ld_words = gate_ld_words; a.steers = steers;
    if (!guides && (!masks || !rules)) return launch_sample<false, true, false, false, false, true>(a, B, (hipStream_t)stream);
    a.masks = masks; a.mask_rows = mask_rows; a.mask_ld_words = mask_ld_words; a.rules = rules;
    if (!guides) return launch_sample<false, true, true, false, false, true>(a, B, (hipStream_t)stream);
    if (int rc = check_guides(who, masks, rules, cls, cls_rows, ld_cls, next, n_next, state_row, n_state_row, gstate, n_vocab)) return rc;
    a.cls = cls; a.cls_rows = cls_rows; a.ld_cls = ld_cls; a.next = (const int*)next; a.n_next = n_next; a.state_row = (const int*)state_row;
    a.n_state_row = n_state_row; a.guides = guides; a.gstate = (int*)gstate;
    if (closes) {
        if (int rc = check_closes(who, close_row, n_close_row, closes)) return rc;
        FO1_CHECK_ARG(budget && ((uintptr_t)budget & 3) == 0, "sample_rows_steered: closing rules need the rows' budgets (device int32 [B])");
        a.close_row = (const int*)close_row; a.n_close_row = n_close_row; a.closes = closes; a.budget = (const int*)budget;
    }
    return launch_sample<false, true, true, true, true, true>(a, B, (hipStream_t)stream);
}

// fo1_decode_head_closing_accept with the rows' steers honoured: the step reads the bias table, its gate and the steers and writes none of
// them; it adds 1 to the accepted token's count of row b and sets its gate bit (when counts are given) — a finished row touches nothing.
// steers == NULL: fo1_decode_head_closing_accept.
int fo1_decode_head_steered_accept(const void* logits, long long ld_logits, int n_vocab, int B, const fo1_sample_params_t* params, int32_t* state,
                                   int32_t* plan, int32_t* ids_out, int ids_ld, const int32_t* stop_ids, int n_stop, int32_t* done, void* workspace,
                                   size_t workspace_bytes, uint32_t* seen, long long ld_words, const uint32_t* masks, int mask_rows,
                                   long long mask_ld_words, const fo1_token_rule_t* rules, void* stream, const uint16_t* cls, int cls_rows,
                                   long long ld_cls, const int32_t* next, long long n_next, const int32_t* state_row, long long n_state_row,
                                   const fo1_token_guide_t* guides, int32_t* gstate, const int32_t* close_row, long long n_close_row,
                                   const fo1_guide_close_t* closes, const void* bias, const uint32_t* bias_gate, int bias_rows, long long ld_bias,
                                   uint16_t* counts, uint32_t* count_gate, long long ld_counts, long long gate_ld_words,
                                   const fo1_token_steer_t* steers) {
    using namespace fo1;
    if (!steers)
        return fo1_decode_head_closing_accept(logits, ld_logits, n_vocab, B, params, state, plan, ids_out, ids_ld, stop_ids, n_stop, done, workspace,
                                              workspace_bytes, seen, ld_words, masks, mask_rows, mask_ld_words, rules, stream, cls, cls_rows, ld_cls, next,
                                              n_next, state_row, n_state_row, guides, gstate, close_row, n_close_row, closes);
    const char* who = "decode_head_steered_accept";
    if (int rc = check_sample(who, logits, ld_logits, n_vocab, B, params, workspace, workspace_bytes)) return rc;
    if (int rc = check_seen(who, seen, ld_words, n_vocab)) return rc;
    if (int rc = check_masks(who, masks, mask_rows, mask_ld_words, n_vocab)) return rc;
    if (int rc = check_steers(who, bias, bias_gate, bias_rows, ld_bias, counts, count_gate, ld_counts, gate_ld_words, n_vocab)) return rc;
    FO1_CHECK_ARG(state && plan && ids_out && done && ids_ld > 0 && n_stop >= -1 && (n_stop == 0 || stop_ids), "decode_head_steered_accept: bad arguments");
    FO1_CHECK_ARG(((uintptr_t)steers & 3) == 0, "decode_head_steered_accept: misaligned steers");
    FO1_CHECK_ARG(!closes || guides, "decode_head_steered_accept: closing rules need the rows' guides");
    SampleArgs a{};
    a.logits = (const uint16_t*)logits; a.ld = ld_logits; a.V = n_vocab; a.params = params;
    a.state = (int*)state; a.plan = (int*)plan; a.ids_out = (int*)ids_out; a.ids_ld = ids_ld; a.stop_ids = (const int*)stop_ids; a.n_stop = n_stop;
    a.done = (int*)done; a.seen = seen; a.ld_words = ld_words;
    a.bias = (const uint16_t*)bias; a.bias_gate = bias_gate; a.bias_rows = bias_rows; a.ld_bias = ld_bias; a.counts = counts;
    a.count_gate = count_gate; a.ld_counts = ld_counts; a.gate_ld_words = gate_ld_words; a.steers = steers;
    if (!guides && (!masks || !rules)) return launch_sample<true, true, false, false, false, true>(a, B, (hipStream_t)stream);
    a.masks = masks; a.mask_rows = mask_rows; a.mask_ld_words = mask_ld_words; a.rules = rules;
    if (!guides) return launch_sample<true, true, true, false, false, true>(a, B, (hipStream_t)stream);
    if (int rc = check_guides(who, masks, rules, cls, cls_rows, ld_cls, next, n_next, state_row, n_state_row, gstate, n_vocab)) return rc;
    a.cls = cls; a.cls_rows = cls_rows; a.ld_cls = ld_cls; a.next = (const int*)next; a.n_next = n_next; a.state_row = (const int*)state_row;
    a.n_state_row = n_state_row; a.guides = guides; a.gstate = (int*)gstate;
    if (closes) {
        if (int rc = check_closes(who, close_row, n_close_row, closes)) return rc;
        a.close_row = (const int*)close_row; a.n_close_row = n_close_row; a.closes = closes;
    }
    return launch_sample<true, true, true, true, true, true>(a, B, (hipStream_t)stream);
}

// Adds 1 to counts[rows[i]][ids[i]] and sets the matching gate bit for i < n (device int32 each; duplicates add up).  Ids outside [0, n_vocab)
// and negative rows are skipped; the caller vouches for rows[i] < the tables' rows.
int fo1_count_mark(uint16_t* counts, long long ld_counts, uint32_t* count_gate, long long gate_ld_words, int n_vocab, const int32_t* rows,
                   const int32_t* ids, int n, void* stream) {
    using namespace fo1;
    FO1_CHECK_ARG(counts && count_gate && n >= 0 && n_vocab >= 1 && (n == 0 || (rows && ids)), "count_mark: bad arguments");
    if (int rc = check_steers("count_mark", nullptr, nullptr, 0, 0, counts, count_gate, ld_counts, gate_ld_words, n_vocab)) return rc;
    if (n == 0) return FO1_OK;
    FO1_LAUNCH("count_mark", (double)n * 16.0, count_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
               reinterpret_cast<uint32_t*>(counts), ld_counts / 2, count_gate, gate_ld_words, n_vocab, (const int*)rows, (const int*)ids, n);
    return FO1_OK;
}

// Sets bit ids[i] of row rows[i] of the seen bitmap for i < n (device int32 each; duplicates are fine).  Ids outside [0, n_vocab) and negative
// rows are skipped; the caller vouches for rows[i] < the bitmap's rows.
int fo1_seen_mark(uint32_t* seen, long long ld_words, int n_vocab, const int32_t* rows, const int32_t* ids, int n, void* stream) {
    using namespace fo1;
    FO1_CHECK_ARG(seen && n >= 0 && n_vocab >= 1 && (n == 0 || (rows && ids)), "seen_mark: bad arguments");
    if (int rc = check_seen("seen_mark", seen, ld_words, n_vocab)) return rc;
    if (n == 0) return FO1_OK;
    FO1_LAUNCH("seen_mark", (double)n * 12.0, seen_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seen, ld_words,
               n_vocab, (const int*)rows, (const int*)ids, n);
    return FO1_OK;
}

}  // extern "C"
