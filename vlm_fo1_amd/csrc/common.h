// common.h — shared helpers for the libfo1hip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fo1.h"
#include "ab.h"   // test / bench build: include/fo1_ab.h (its declarations carry the export visibility)

namespace fo1 {

// thread-local error text (fo1_last_error)
char* err_buf();
int set_err(int code, const char* fmt, ...);

#define FO1_CHECK_ARG(cond, ...)                                   \
    do {                                                           \
        if (!(cond)) return fo1::set_err(FO1_ERR_ARG, __VA_ARGS__); \
    } while (0)

#define FO1_CHECK_HIP(expr)                                                                  \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return fo1::set_err((int)_e, "%s failed: %s", #expr, hipGetErrorString(_e));     \
    } while (0)

#define FO1_CHECK_LAUNCH()                                                                        \
    do {                                                                                          \
        hipError_t _e = hipGetLastError();                                                        \
        if (_e != hipSuccess)                                                                     \
            return fo1::set_err((int)_e, "kernel launch failed at %s:%d: %s", __FILE__, __LINE__, \
                                hipGetErrorString(_e));                                           \
    } while (0)

// bf16 <-> f32 bit helpers (round-to-nearest-even on the way down, like torch)
__device__ __forceinline__ float bf16_lo(uint32_t packed) { return __uint_as_float(packed << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t packed) { return __uint_as_float(packed & 0xffff0000u); }
__device__ __forceinline__ float bf16_to_f32(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
// gfx950 converts in hardware (v_cvt_pk_bf16_f32, round-to-nearest-even): one instruction where the bit-twiddled form costs six
// and a branch; every epilogue in the library goes through these two.
__device__ __forceinline__ uint16_t f32_to_bf16(float f) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) float fo1_f32x2;
    typedef __attribute__((ext_vector_type(2))) __bf16 fo1_bf16x2;
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(fo1_f32x2{lo, hi}, fo1_bf16x2));
}
// the fp32 value of what a bf16 store would hold (the reference's intermediate tensors are bf16)
__device__ __forceinline__ float round_bf16(float v) { return bf16_to_f32(f32_to_bf16(v)); }
// 8 bf16 (one 16-byte chunk) <-> 8 floats
__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
    f[0] = bf16_lo(u.x); f[1] = bf16_hi(u.x); f[2] = bf16_lo(u.y); f[3] = bf16_hi(u.y);
    f[4] = bf16_lo(u.z); f[5] = bf16_hi(u.z); f[6] = bf16_lo(u.w); f[7] = bf16_hi(u.w);
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
    return uint4{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
}
// sum over the 64 lanes of a wave (xor shuffles: every lane gets the total, the same bits in each)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// acc + the dot product of two 16-byte chunks of bf16 as four v_dot2_f32_bf16 (pairs summed in fp32, in element order)
__device__ __forceinline__ float dot8_dot2(const uint4& a, const uint4& b, float acc) {
    typedef __attribute__((ext_vector_type(2))) __bf16 fo1_bf16x2;
    acc = __builtin_amdgcn_fdot2_f32_bf16(*reinterpret_cast<const fo1_bf16x2*>(&a.x), *reinterpret_cast<const fo1_bf16x2*>(&b.x), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(*reinterpret_cast<const fo1_bf16x2*>(&a.y), *reinterpret_cast<const fo1_bf16x2*>(&b.y), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(*reinterpret_cast<const fo1_bf16x2*>(&a.z), *reinterpret_cast<const fo1_bf16x2*>(&b.z), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(*reinterpret_cast<const fo1_bf16x2*>(&a.w), *reinterpret_cast<const fo1_bf16x2*>(&b.w), acc, false);
    return acc;
}
// streamed-once weights: non-temporal 16-byte load (MI355X_MICROARCH "nt-weights": -18 % issue-to-landed on a decode weight stream)
__device__ __forceinline__ uint4 load_nt16(const uint16_t* p) {
    typedef __attribute__((ext_vector_type(4))) unsigned int fo1_u32x4;
    const fo1_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const fo1_u32x4*>(p));
    return uint4{v.x, v.y, v.z, v.w};
}
// One 16-byte chunk of Qwen2RMSNorm (modeling_qwen2_5_vl.py:126-140) given the row's rstd (fp32 variance): bf16(x * rstd), then * weight -> bf16 —
// the reference's rounding points, which is why the decode linears' three fused prologues (gemv.hip, decode.hip, decode_mfma.hip) share this one.
__device__ __forceinline__ uint4 rmsnorm_chunk(const uint4& v, const uint4& w, float rstd) {
    uint4 o;
    o.x = pack_bf16x2(bf16_lo(w.x) * round_bf16(bf16_lo(v.x) * rstd), bf16_hi(w.x) * round_bf16(bf16_hi(v.x) * rstd));
    o.y = pack_bf16x2(bf16_lo(w.y) * round_bf16(bf16_lo(v.y) * rstd), bf16_hi(w.y) * round_bf16(bf16_hi(v.y) * rstd));
    o.z = pack_bf16x2(bf16_lo(w.z) * round_bf16(bf16_lo(v.z) * rstd), bf16_hi(w.z) * round_bf16(bf16_hi(v.z) * rstd));
    o.w = pack_bf16x2(bf16_lo(w.w) * round_bf16(bf16_lo(v.w) * rstd), bf16_hi(w.w) * round_bf16(bf16_hi(v.w) * rstd));
    return o;
}

// Activations of the fused epilogues.  Their result is rounded to bf16 (8 significant bits) right away, so the hardware
// approximations (v_exp_f32, v_rcp_f32: ~1 ulp of fp32) replace the library's expf / erff / IEEE division — ~6 instructions per
// element instead of ~25-40, in epilogues that run 128 elements per lane (DaViT fc1 + GELU ran at 564 TFLOP/s for that reason).
// SiLU (Qwen2MLP act_fn, modeling_qwen2_5_vl.py:636):  v * sigmoid(v).
__device__ __forceinline__ float fo1_silu(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
// erf-GELU (nn.GELU(): modeling_davit.py:57, simple_fpn.py:145, multimodal_projector/builder.py:69,108, merger): 0.5 v (1 + erf(v / sqrt 2))
// with erfc(|x|) from Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7 absolute); 1 + erf(x) is formed as erfc(|x|) on the negative
// side (no cancellation) and 2 - erfc(x) on the positive side.
__device__ __forceinline__ float fo1_gelu_erf(float v) {
    const float x = v * 0.70710678118654752440f, ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float e = poly * t * __expf(-ax * ax);
    return 0.5f * v * (x >= 0.f ? 2.0f - e : e);
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// A launch with more than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize on that kernel instantiation.  Set once per
// process: the function-local static is initialised by the first call (host threads that make it together — engine replicas, the decode
// pool's thread, the prefetch helpers — see one hipFuncSetAttribute and all of them its result; later launches read a guard byte, no
// lock).  The first call of an instantiation is never inside a stream capture: passes run eagerly first.
template <auto KERNEL, int BYTES>
inline hipError_t dynamic_lds_once() {
    static const hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, BYTES);
    return e;
}
#define FO1_DYNAMIC_LDS_ONCE(bytes, ...) FO1_CHECK_HIP((fo1::dynamic_lds_once<__VA_ARGS__, bytes>()))   // (kernel last: its template arguments carry commas)

// ---- optional per-kernel timing (fo1_profile_*) ---------------------------------------
// When enabled every FO1_LAUNCH goes through hipExtLaunchKernelGGL with a start/stop event pair, which the runtime fills
// from the dispatch packet's own begin/end timestamps (the clocks rocprofv3's kernel trace reads), so a row's time is
// kernel execution only -- no inter-packet latency.  Disabled (the default, and always during throughput timing and
// graph capture) it is a plain launch.
bool profile_enabled();
void profile_events(const char* name, double work, hipEvent_t* e0, hipEvent_t* e1);

#define FO1_LAUNCH(name, work, kernel, grid, block, shmem, st, ...)                                   \
    do {                                                                                              \
        if (fo1::profile_enabled()) {                                                                 \
            hipEvent_t _e0, _e1;                                                                      \
            fo1::profile_events(name, (double)(work), &_e0, &_e1);                                    \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, st, _e0, _e1, 0, __VA_ARGS__);          \
        } else {                                                                                      \
            hipLaunchKernelGGL(kernel, grid, block, shmem, st, __VA_ARGS__);                          \
        }                                                                                             \
        FO1_CHECK_LAUNCH();                                                                           \
    } while (0)

}  // namespace fo1
