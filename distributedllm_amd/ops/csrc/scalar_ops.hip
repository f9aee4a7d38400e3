// Scalar (non-MFMA) kernels of the slice engine (gfx950): the embedding
// gather, the two-stage argmax, and the legacy f32 layer path used by
// f32-weight test models — RMSNorm plus a wave-per-row GEMV family
// (qkv + RoPE + KV append, gemv + residual, w1/w3 SwiGLU). SURVEY.md §2.5
// maps each reference op K1-K15 to a kernel; the section comments below
// name them.
//
// The GEMV family is f32-only: quantized and f16 layers always take the
// MFMA path (mfma_gemm.hip), and the engine builds legacy matrices only
// from f32 tensors. k_embed alone keeps all four weight types, because
// the embedding table arrives as q4_0, q4_1, f16 or f32 in the SoA layout
// whatever path the layers take.

#include "device_common.h"
#include "kernels.h"

// --------------------------------------------------------------- row x vec
// One WAVE computes dot(row r of W, x_t) for T tokens (T <= TMAX).
// x: [T][cols] f32 (row-major, ld = cols). Results valid in lane 0.
//
// Coalescing is the whole game here (decode GEMV = HBM-bound weight
// stream): every lane covers 4 CONSECUTIVE weights, so the wave's weight
// and x loads are each one contiguous 1 KiB float4 transaction. (The
// naive block-per-lane layout put each lane's x on its own cache line
// — 64 transactions per wave instruction — and measured 25x off the
// bandwidth roofline; rocprof evidence in profiles/.)

template <int TMAX>
__device__ __forceinline__ void wave_row_dot_f32(
    const float* __restrict__ data, int row, int cols,
    const float* __restrict__ x, int T, float* __restrict__ acc) {
    const float* wrow = data + (size_t)row * cols;
    const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int t = 0; t < TMAX; ++t) acc[t] = 0.0f;
    const int niter = (cols + 255) >> 8;
    for (int g = 0; g < niter; ++g) {
        const int c = g * 256 + lane * 4;
        float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < cols)
            w4 = *reinterpret_cast<const float4*>(wrow + c);
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t >= T) continue;
            float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < cols)
                xv = *reinterpret_cast<const float4*>(
                    x + (size_t)t * cols + c);
            float s = fmaf(w4.x, xv.x, 0.0f);
            s = fmaf(w4.y, xv.y, s);
            s = fmaf(w4.z, xv.z, s);
            s = fmaf(w4.w, xv.w, s);
            acc[t] += s;
        }
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
        if (t < T) acc[t] = wave_reduce_sum(acc[t]);
}

// ------------------------------------------------------------------ RMSNorm
// y[t] = x[t] * rsqrt(mean(x[t]^2) + eps) * w     (K2 of SURVEY §2.5;
// reference: ggml_rms_norm + ggml_mul, tensor_processor.cpp:555-570)

__global__ void k_rmsnorm(const float* __restrict__ x,
                          const float* __restrict__ w,
                          float* __restrict__ y, int E, float eps) {
    const int t = blockIdx.x;
    const float* xt = x + (size_t)t * E;
    float* yt = y + (size_t)t * E;
    __shared__ float red[NWAVES];

    float ss = 0.0f;
    for (int i = threadIdx.x; i < (E >> 2); i += BLOCK) {
        const float4 v = reinterpret_cast<const float4*>(xt)[i];
        ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    ss = wave_reduce_sum(ss);
    const int wid = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) red[wid] = ss;
    __syncthreads();
    float total = 0.0f;
#pragma unroll
    for (int i = 0; i < NWAVES; ++i) total += red[i];
    const float scale = rsqrtf(total / (float)E + eps);

    for (int i = threadIdx.x; i < (E >> 2); i += BLOCK) {
        const float4 v = reinterpret_cast<const float4*>(xt)[i];
        const float4 g = reinterpret_cast<const float4*>(w)[i];
        float4 o;
        o.x = v.x * scale * g.x;
        o.y = v.y * scale * g.y;
        o.z = v.z * scale * g.z;
        o.w = v.w * scale * g.w;
        reinterpret_cast<float4*>(yt)[i] = o;
    }
}

// ------------------------------------------------- QKV + RoPE + KV append
// Fuses K3+K4+K5 of SURVEY §2.5 (reference: ggml_mul_mat wq/wk/wv +
// ggml_rope_inplace + ggml_cpy into cache, tensor_processor.cpp:579-622).
// Grid: (3E/4) blocks; block computes 4 consecutive rows of one of
// {wq, wk, wv}. RoPE (GGML mode 0: rotate adjacent pairs (2i, 2i+1) within
// each head, theta = pos * base^(-2i/D)) is applied in the epilogue to q and
// k rows; k/v rows are converted to f16 and appended to the cache at
// [seq[t]][pos[t]].

template <int TMAX>
__global__ void k_qkv_rope_append(
    WMat wq, WMat wk, WMat wv, const float* __restrict__ xn,
    float* __restrict__ q_buf, __half* __restrict__ k_cache,
    __half* __restrict__ v_cache, const int* __restrict__ pos,
    const int* __restrict__ seq, const float* __restrict__ inv_freq,
    int E, int D, int n_ctx, int T) {
    const int r_global = blockIdx.x * 4;  // in [0, 3E)
    const int mat = r_global / E;         // 0=q 1=k 2=v
    const int row0 = r_global % E;
    const int wid = threadIdx.x / WAVE;
    const int row = row0 + wid;

    float acc[TMAX];
    const WMat& w = (mat == 0) ? wq : (mat == 1) ? wk : wv;
    wave_row_dot_f32<TMAX>((const float*)w.data, row, w.cols, xn, T, acc);

    __shared__ float ybuf[4][TMAX];
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
            if (t < T) ybuf[wid][t] = acc[t];
    }
    __syncthreads();

    if (mat == 2) {
        // v rows: straight f16 append, thread handles (row r, token t)
        const int idx = threadIdx.x;
        if (idx < 4 * T) {
            const int rr = idx / T, t = idx % T;
            const int e = row0 + rr;
            __half* dst = v_cache +
                ((size_t)seq[t] * n_ctx + pos[t]) * E + e;
            *dst = __float2half(ybuf[rr][t]);
        }
        return;
    }
    // q/k rows: rope on pairs (row0+2p, row0+2p+1)
    const int idx = threadIdx.x;
    if (idx < 2 * T) {
        const int p = idx / T, t = idx % T;
        const int e = row0 + 2 * p;
        const int d = e % D;
        const float theta = (float)pos[t] * inv_freq[d >> 1];
        float c, s;
        __sincosf(theta, &s, &c);
        const float x0 = ybuf[2 * p][t], x1 = ybuf[2 * p + 1][t];
        float o0, o1;
        rope_rotate(x0, x1, s, c, o0, o1);
        if (mat == 0) {
            q_buf[(size_t)t * E + e] = o0;
            q_buf[(size_t)t * E + e + 1] = o1;
        } else {
            __half* dst = k_cache +
                ((size_t)seq[t] * n_ctx + pos[t]) * E + e;
            dst[0] = __float2half(o0);
            dst[1] = __float2half(o1);
        }
    }
}

// --------------------------------------------------------------- GEMV(+res)
// K9/K10/K13/K14 of SURVEY §2.5: output projection / FFN down / lm_head,
// with the residual add fused into the epilogue.

template <int TMAX, bool RES>
__global__ void k_gemv(WMat w, const float* __restrict__ x,
                       const float* __restrict__ res,
                       float* __restrict__ y, int T) {
    const int row = blockIdx.x * 4 + threadIdx.x / WAVE;
    float acc[TMAX];
    wave_row_dot_f32<TMAX>((const float*)w.data, row, w.cols, x, T, acc);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t >= T) continue;
            float v = acc[t];
            if (RES) v += res[(size_t)t * w.rows + row];
            y[(size_t)t * w.rows + row] = v;
        }
    }
}

// ------------------------------------------------------------ w1/w3 SwiGLU
// K11+K12 of SURVEY §2.5 (reference: ggml_mul_mat w1/w3 + ggml_silu +
// ggml_mul, tensor_processor.cpp:732-751): g = silu(w1·x) * (w3·x).

template <int TMAX>
__global__ void k_ffn_gate(WMat w1, WMat w3, const float* __restrict__ xn,
                           float* __restrict__ g, int T) {
    const int row = blockIdx.x * 4 + threadIdx.x / WAVE;
    float a1[TMAX], a3[TMAX];
    wave_row_dot_f32<TMAX>((const float*)w1.data, row, w1.cols, xn, T, a1);
    wave_row_dot_f32<TMAX>((const float*)w3.data, row, w3.cols, xn, T, a3);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t >= T) continue;
            const float v1 = a1[t];
            const float silu = v1 / (1.0f + __expf(-v1));
            g[(size_t)t * w1.rows + row] = silu * a3[t];
        }
    }
}

// -------------------------------------------------------- embedding gather
// K1 of SURVEY §2.5 (ggml_get_rows, tensor_processor.cpp:1767): dequantize
// row tok[t] of the embedding table into f32 activations.

template <int WT>
__global__ void k_embed(WMat tab, const int* __restrict__ tokens,
                        float* __restrict__ out, int E) {
    const int t = blockIdx.x;
    const int row = tokens[t];
    float* dst = out + (size_t)t * E;
    if (WT == W_Q4_0) {
        const int nb = E >> 5;
        const __half* srow = (const __half*)tab.scales + (size_t)row * nb;
        const uint8_t* qrow = (const uint8_t*)tab.data + (size_t)row * nb * 16;
        for (int b = threadIdx.x; b < nb; b += BLOCK) {
            const float d = __half2float(srow[b]);
            const uint4 packed = *reinterpret_cast<const uint4*>(qrow + b * 16);
            const uint32_t w[4] = {packed.x, packed.y, packed.z, packed.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int lo = (int)((w[i] >> (8 * j)) & 0xF) - 8;
                    const int hi = (int)((w[i] >> (8 * j + 4)) & 0xF) - 8;
                    dst[(b << 5) + i * 4 + j] = d * (float)lo;
                    dst[(b << 5) + 16 + i * 4 + j] = d * (float)hi;
                }
            }
        }
    } else if (WT == W_Q4_1) {
        const int nb = E >> 5;
        const __half* srow = (const __half*)tab.scales + (size_t)row * nb * 2;
        const uint8_t* qrow = (const uint8_t*)tab.data + (size_t)row * nb * 16;
        for (int b = threadIdx.x; b < nb; b += BLOCK) {
            const float d = __half2float(srow[b * 2]);
            const float mm = __half2float(srow[b * 2 + 1]);
            const uint4 packed = *reinterpret_cast<const uint4*>(qrow + b * 16);
            const uint32_t w[4] = {packed.x, packed.y, packed.z, packed.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int lo = (int)((w[i] >> (8 * j)) & 0xF);
                    const int hi = (int)((w[i] >> (8 * j + 4)) & 0xF);
                    dst[(b << 5) + i * 4 + j] = d * (float)lo + mm;
                    dst[(b << 5) + 16 + i * 4 + j] = d * (float)hi + mm;
                }
            }
        }
    } else if (WT == W_F16) {
        const __half* wrow = (const __half*)tab.data + (size_t)row * E;
        for (int i = threadIdx.x; i < E; i += BLOCK)
            dst[i] = __half2float(wrow[i]);
    } else {
        const float* wrow = (const float*)tab.data + (size_t)row * E;
        for (int i = threadIdx.x; i < E; i += BLOCK) dst[i] = wrow[i];
    }
}

// ------------------------------------------------------------------- argmax
// K15 of SURVEY §2.5 (sample_next_token greedy argmax,
// tensor_processor.cpp:1894-1908), on-device so greedy decode never copies
// the [V] logits to host.

// Two-stage: grid (T, NPART) partial blocks each reduce a V/NPART chunk
// and atomicMax a packed u64 key (ordered-f32 ‖ bit-inverted index — the
// index inversion makes ties resolve to the SMALLEST index, matching the
// reference's first-max scan); a tiny decode kernel unpacks. One block per
// row (the previous form) used only T CUs of 256 and measured 40 µs at
// T=4, V=32000.
__device__ __forceinline__ uint32_t ordered_f32(float v) {
    union { float f; uint32_t u; } c;
    c.f = v;
    return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}

__global__ void k_argmax_part(const float* __restrict__ logits,
                              unsigned long long* __restrict__ keys, int V) {
    const int t = blockIdx.x;
    const float* lt = logits + (size_t)t * V;
    const int chunk = (V + gridDim.y - 1) / gridDim.y;
    const int i0 = blockIdx.y * chunk;
    const int i1 = min(V, i0 + chunk);
    float best = -INFINITY;
    int bi = i0;
    for (int i = i0 + threadIdx.x; i < i1; i += BLOCK) {
        const float v = lt[i];
        if (v > best || (v == best && i < bi)) {
            best = v;
            bi = i;
        }
    }
    unsigned long long key =
        ((unsigned long long)ordered_f32(best) << 32) | (uint32_t)(~bi);
    __shared__ unsigned long long sk[BLOCK];
    sk[threadIdx.x] = key;
    __syncthreads();
    for (int stride = BLOCK / 2; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride)
            sk[threadIdx.x] = max(sk[threadIdx.x], sk[threadIdx.x + stride]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(keys + t, sk[0]);
}

__global__ void k_argmax_finish(const unsigned long long* __restrict__ keys,
                                int* __restrict__ out, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < T) out[t] = (int)~(uint32_t)(keys[t] & 0xFFFFFFFFu);
}

// ============================================================== launchers

static inline int pick_tmax(int T) {
    if (T <= 1) return 1;
    if (T <= 2) return 2;
    if (T <= 4) return 4;
    if (T <= 8) return 8;
    return 16;
}

void launch_rmsnorm(hipStream_t s, const float* x, const float* w, float* y,
                    int T, int E, float eps) {
    hipLaunchKernelGGL(k_rmsnorm, dim3(T), dim3(BLOCK), 0, s, x, w, y, E, eps);
}

#define DISPATCH_TMAX(TMAXV, ...)        \
    switch (TMAXV) {                     \
        case 1: {                        \
            constexpr int TMc = 1;       \
            __VA_ARGS__;                 \
            break;                       \
        }                                \
        case 2: {                        \
            constexpr int TMc = 2;       \
            __VA_ARGS__;                 \
            break;                       \
        }                                \
        case 4: {                        \
            constexpr int TMc = 4;       \
            __VA_ARGS__;                 \
            break;                       \
        }                                \
        case 8: {                        \
            constexpr int TMc = 8;       \
            __VA_ARGS__;                 \
            break;                       \
        }                                \
        default: {                       \
            constexpr int TMc = 16;      \
            __VA_ARGS__;                 \
            break;                       \
        }                                \
    }

void launch_qkv_rope_append(hipStream_t s, const WMat& wq, const WMat& wk,
                            const WMat& wv, const float* xn, float* q_buf,
                            __half* k_cache_layer, __half* v_cache_layer,
                            const int* pos, const int* seq,
                            const float* inv_freq, int E, int D, int n_ctx,
                            int T) {
    const int tmax = pick_tmax(T);
    const dim3 grid(3 * E / 4);
    DISPATCH_TMAX(
        tmax, hipLaunchKernelGGL((k_qkv_rope_append<TMc>), grid,
                                 dim3(BLOCK), 0, s, wq, wk, wv, xn, q_buf,
                                 k_cache_layer, v_cache_layer, pos, seq,
                                 inv_freq, E, D, n_ctx, T));
}

void launch_gemv(hipStream_t s, const WMat& w, const float* x,
                 const float* res, float* y, int T) {
    const int tmax = pick_tmax(T);
    const dim3 grid(w.rows / 4);
    if (res != nullptr) {
        DISPATCH_TMAX(
            tmax, hipLaunchKernelGGL((k_gemv<TMc, true>), grid,
                                     dim3(BLOCK), 0, s, w, x, res, y, T));
    } else {
        DISPATCH_TMAX(
            tmax, hipLaunchKernelGGL((k_gemv<TMc, false>), grid,
                                     dim3(BLOCK), 0, s, w, x, res, y, T));
    }
}

void launch_ffn_gate(hipStream_t s, const WMat& w1, const WMat& w3,
                     const float* xn, float* g, int T) {
    const int tmax = pick_tmax(T);
    const dim3 grid(w1.rows / 4);
    DISPATCH_TMAX(
        tmax, hipLaunchKernelGGL((k_ffn_gate<TMc>), grid, dim3(BLOCK),
                                 0, s, w1, w3, xn, g, T));
}

void launch_embed(hipStream_t s, const WMat& tab, const int* tokens,
                  float* out, int T, int E) {
    switch (tab.wtype) {
        case W_Q4_0:
            hipLaunchKernelGGL((k_embed<W_Q4_0>), dim3(T), dim3(BLOCK), 0, s,
                               tab, tokens, out, E);
            break;
        case W_Q4_1:
            hipLaunchKernelGGL((k_embed<W_Q4_1>), dim3(T), dim3(BLOCK), 0, s,
                               tab, tokens, out, E);
            break;
        case W_F16:
            hipLaunchKernelGGL((k_embed<W_F16>), dim3(T), dim3(BLOCK), 0, s,
                               tab, tokens, out, E);
            break;
        default:
            hipLaunchKernelGGL((k_embed<W_F32>), dim3(T), dim3(BLOCK), 0, s,
                               tab, tokens, out, E);
            break;
    }
}

void launch_argmax(hipStream_t s, const float* logits,
                   unsigned long long* keys, int* out, int T, int V) {
    (void)hipMemsetAsync(keys, 0, sizeof(unsigned long long) * T, s);
    const int npart = min(32, (V + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(k_argmax_part, dim3(T, npart), dim3(BLOCK), 0, s,
                       logits, keys, V);
    hipLaunchKernelGGL(k_argmax_finish, dim3((T + 63) / 64), dim3(64), 0,
                       s, keys, out, T);
}
