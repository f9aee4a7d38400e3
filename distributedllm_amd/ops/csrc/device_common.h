// Device-side helpers shared by the kernel translation units
// (mfma_gemm.hip, attention.hip, scalar_ops.hip): wave/block constants,
// MFMA fragment types, packed-f16 bit casts, wave reductions, and the two
// pieces of layout/arithmetic that producers and consumers must agree on —
// the xprep side-channel index and the RoPE pair rotation.
//
// Change with care: xprep_index IS the B-fragment gather layout of
// wave_tile_kloop (mfma_gemm.hip) and of the host-side buffer sizing in
// engine_ext.cpp; rope_rotate's expression order fixes the floating-point
// contraction every q/k row goes through.
//
// Wavefront = 64 (CDNA); blocks are 256 threads = 4 waves.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#define WAVE 64
#define NWAVES 4
#define BLOCK 256

// ----------------------------------------------------- MFMA fragment types

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

union ABFrag {
    uint32_t u[4];
    f16x8 v;
};

// packed-f16 helpers for the MFMA side-channels / dequant
__device__ __forceinline__ uint32_t pack_f16(float lo, float hi) {
    union { __half2 h; uint32_t u; } c;
    c.h = __floats2half2_rn(lo, hi);
    return c.u;
}
__device__ __forceinline__ __half2 u2h2(uint32_t w) {
    union { uint32_t u; __half2 h; } c;
    c.u = w;
    return c.h;
}
__device__ __forceinline__ uint32_t h22u(__half2 h) {
    union { __half2 h; uint32_t u; } c;
    c.h = h;
    return c.u;
}

// ---------------------------------------------------------------- reductions

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;  // valid in lane 0
}

// ------------------------------------------------------ xprep side channel
// f16 activations in MFMA B-fragment order: element e of token t lives at
// [e/8][t/16 of jtw token tiles][t%16][e%8], so one lane's 16 B load is a
// ready B fragment (8 consecutive k for one token column).
__device__ __forceinline__ size_t xprep_index(int e, int t, int jtw) {
    return (((size_t)(e >> 3) * jtw + (t >> 4)) * 16 + (t & 15)) * 8 +
           (e & 7);
}

// --------------------------------------------------------------------- RoPE
// GGML mode 0: rotate the adjacent pair (x0, x1) by theta = pos *
// base^(-2i/D), given (sn, cs) = sincos(theta).
__device__ __forceinline__ void rope_rotate(float x0, float x1, float sn,
                                            float cs, float& o0, float& o1) {
    o0 = x0 * cs - x1 * sn;
    o1 = x0 * sn + x1 * cs;
}
