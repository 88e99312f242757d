// bf16_dev.h -- bf16 as the reduced-precision study modes use it (kernels_gemm32.hip, kernels_bf16e.hip; TNML_BF16 / TNML_BF16X3): fp32 -> bf16
// by round to nearest even, the hi + lo split x = hi + lo with hi = bf16(x) FIRST and lo = bf16(x - hi), and pairs of bf16 packed into the
// 32-bit words the LDS tiles and the converted-once copies are written in.  tests/rp_model.py restates the rounding and the split.
// The helpers are scalar on purpose: with one that takes or returns the arrays of a 4- or 8-value pack the compiler no longer packs with
// v_perm_b32 (k_bgemm on the bf16 pipe: + 10 % instructions and an occupancy step), so a call site keeps its unsigned short arrays local.
#pragma once
#include <hip/hip_runtime.h>

typedef short bf16x8 __attribute__((ext_vector_type(8)));      // an A / B fragment of v_mfma_f32_16x16x32_bf16: 8 consecutive reduction indices
typedef float f32x4 __attribute__((ext_vector_type(4)));       // a C fragment: col = lane & 15, row = 4 (lane >> 4) + reg

static __device__ __forceinline__ unsigned short f2bf(float x) {
    const unsigned u = __float_as_uint(x);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static __device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

// the split x = hi + lo: hi = f2bf(x) FIRST, then lo = bf_lo(x, hi) = bf16(x - hi)
static __device__ __forceinline__ unsigned short bf_lo(float x, unsigned short hi) { return f2bf(x - bf2f(hi)); }
// two consecutive bf16 as one 32-bit word, a in the low half
static __device__ __forceinline__ unsigned bf_pack(unsigned short a, unsigned short b) { return (unsigned)a | ((unsigned)b << 16); }
