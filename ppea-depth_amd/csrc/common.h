// Shared device/host helpers for libppea_depth.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PPEA_ABI_VERSION 32
#define PPEA_ERR_UNSUPPORTED (-1)
#define PPEA_ERR_ARG (-2)
#define WAVE 64

// bf16 <-> f32 (storage type uint16_t).  Plain casts through __hip_bfloat16 would pull in
// headers we do not need; round-to-nearest-even on the bit pattern, NaN kept a NaN.
__device__ __forceinline__ float bf16_to_f32(uint16_t v) {
    return __uint_as_float(((uint32_t)v) << 16);
}
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);  // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// The same conversions as the hardware does them (a shift; a cast through __bf16, which the compiler pairs into
// v_cvt_pk_bf16_f32), used by the MFMA kernels' epilogues.  bf16_to_f32 / f32_to_bf16 above are integer arithmetic behind
// ld_f32 / st_f32; the two pairs differ in NaN payloads and in generated code and are NOT interchangeable bit for bit.
__device__ __forceinline__ float bf2f(uint16_t v) { return __builtin_bit_cast(float, (uint32_t)v << 16); }
__device__ __forceinline__ uint16_t f2bf(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float dgelu_f(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

template <typename T> __device__ __forceinline__ float ld_f32(const T* p);
template <> __device__ __forceinline__ float ld_f32<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ld_f32<uint16_t>(const uint16_t* p) { return bf16_to_f32(*p); }
template <typename T> __device__ __forceinline__ void st_f32(T* p, float v);
template <> __device__ __forceinline__ void st_f32<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void st_f32<uint16_t>(uint16_t* p, float v) { *p = f32_to_bf16(v); }

// 64-lane sum via DPP-backed shuffles; result valid in every lane.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

static inline int launch_status() { return (int)hipGetLastError(); }
