// The arg-max key of logprobs.hip, shared with the lm_head scoring epilogue
// (mfma_gemm.hip k_lmhead_score -> logprobs.hip k_score_finish): the
// order-preserving u32 image of an f32 in the high word, the bit-inverted
// vocabulary index in the low word. The largest key is the largest value
// and, among equal values, the smallest index; -0.0 is keyed as +0.0.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned long long logprobs_key(float v, int i) {
    if (v == 0.0f) v = 0.0f;  // -0.0 -> +0.0
    union { float f; uint32_t u; } c;
    c.f = v;
    const uint32_t o = (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
    return ((unsigned long long)o << 32) | (uint32_t)(~i);
}

// the f32 a key was packed from (exact inverse of the high word)
__device__ __forceinline__ float logprobs_key_value(unsigned long long k) {
    const uint32_t o = (uint32_t)(k >> 32);
    union { uint32_t u; float f; } c;
    c.u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    return c.f;
}

// the vocabulary index a key was packed from
__device__ __forceinline__ int logprobs_key_index(unsigned long long k) {
    return (int)~(uint32_t)k;
}
