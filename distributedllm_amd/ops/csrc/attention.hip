// Attention kernels of the slice engine (gfx950): the streaming
// online-softmax decode kernel `k_attention` (optionally fused with the qkv
// split-K finish: slab sum + RoPE + KV append in its prologue) and the
// matrix-core prefill flash kernel `k_attn_prefill_mfma`, and the GQA decode
// kernel `k_attn_gqa` (+ `k_attn_gqa_merge`), and shared-prefix attention
// `k_attn_prefix` + `k_attn_prefix_tail`, with their launchers. All cover head dims D <= 128 only; the SliceEngine
// constructor rejects anything larger, so there is no fallback kernel.
//
// Not to be changed casually: k_attention's streaming loop (load order,
// shuffle butterflies, two-group iteration) and everything inside
// k_attn_prefill_mfma's tile loop were tuned against rocprofv3 counters
// (docs/kernels.md); both must stay bit-reproducible run to run.

#include <algorithm>

#include "attn_common.h"
#include "device_common.h"
#include "kernels.h"

// ------------------------------------------------------ streaming attention
// Fuses K6+K7+K8 of SURVEY §2.5 (reference: ggml_mul_mat KxQ + scale +
// diag_mask_inf + soft_max + VxP, tensor_processor.cpp:645-700) into one
// online-softmax kernel: O(1) memory in context length, never materializes
// the [P+N, N, H] score tensor. Grid: (T, H); token t attends over cache
// entries [0, pos[t]] of sequence seq[t] — causality for prefill rows comes
// from their per-row positions.

// 8 halves [d0, d0+8) of `row` as floats — UNCONDITIONAL 16 B load
// (the KV allocation carries 16 halves of tail pad, and a lane-varying
// tail branch would execute BOTH paths with exec masking — the guarded
// first version added 8 masked scalar loads to every wide load and
// measured slower than 2 B loads). Elements past D return whatever the
// next row holds: always finite (the cache is zero-initialized and only
// ever written with real values); callers discard d >= D.
__device__ __forceinline__ void load_voct(const __half* __restrict__ row,
                                          int d0, float f[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(row + d0);
    const __half2* h2 = reinterpret_cast<const __half2*>(&u);
    const float2 a = __half22float2(h2[0]);
    const float2 b = __half22float2(h2[1]);
    const float2 c = __half22float2(h2[2]);
    const float2 d = __half22float2(h2[3]);
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
    f[4] = c.x; f[5] = c.y; f[6] = d.x; f[7] = d.y;
}

// FUSEQKV (decode only — every token its own sequence, so no block needs
// another token's new KV row): the prologue sums the qkv split-K slabs
// for this (token, head) slice, applies RoPE, appends the K/V cache row
// itself and stages q in LDS — replacing the separate k_qkv_finish pass
// (each such small kernel costs ~5 us at this chain shape).
template <bool FUSEQKV>
__global__ void k_attention(
    const float* __restrict__ q_buf, const __half* __restrict__ k_cache,
    __half* __restrict__ v_cache, float* __restrict__ out,
    unsigned short* __restrict__ out_prep, const int* __restrict__ pos,
    const int* __restrict__ seq, int E, int Ekv, int D, int n_ctx,
    int jtw, const float* __restrict__ qkv_slab, int ks,
    const float* __restrict__ inv_freq) {
    const int t = blockIdx.x;
    const int h = blockIdx.y;
    const int J = pos[t] + 1;
    // GQA: q head h reads kv head h / (H / Hkv); KV rows are Ekv wide
    const int grp = (int)gridDim.y / (Ekv / D);
    const int hk = h / grp;
    const size_t base = (size_t)seq[t] * n_ctx * Ekv + hk * D;
    const float inv_sqrt_d = rsqrtf((float)D);

    extern __shared__ float smem[];
    float* lds_q = smem;          // [D]
    float* lds_p = smem + D;      // [BLOCK]
    float* lds_red = lds_p + BLOCK;  // [NWAVES]

    if (FUSEQKV) {
        // qkv_slab layout: f32[(E + 2*Ekv)/16 gtiles][ks][64 tok][16
        // rows]; q rows then k rows then v rows. With GQA the `grp`
        // blocks sharing a kv head all append the SAME row bytes —
        // redundant but benign.
        const int p = J - 1;
        const size_t koff = (size_t)(E >> 4) * ks * 64 * 16;
        const size_t voff = koff + (size_t)(Ekv >> 4) * ks * 64 * 16;
        __half* kv_k =
            const_cast<__half*>(k_cache) + base + (size_t)p * Ekv;
        __half* kv_v = v_cache + base + (size_t)p * Ekv;
        for (int d = threadIdx.x; d < D; d += BLOCK) {
            const int e = h * D + d;        // row in q space
            const int ek = hk * D + d;      // row in kv space
            float q = 0.f, k = 0.f, v = 0.f;
            for (int c = 0; c < ks; ++c) {
                q += qkv_slab[(((size_t)(e >> 4) * ks + c) * 64 + t) * 16 +
                              (e & 15)];
                const size_t offk =
                    (((size_t)(ek >> 4) * ks + c) * 64 + t) * 16 +
                    (ek & 15);
                k += qkv_slab[koff + offk];
                v += qkv_slab[voff + offk];
            }
            lds_q[d] = q;
            lds_p[d] = k;  // staged for the pair rotation below
            kv_v[d] = __float2half(v);
        }
        __syncthreads();
        // RoPE on (even, odd) pairs; h*D is even so e % D == d
        for (int d2 = threadIdx.x; d2 < D / 2; d2 += BLOCK) {
            const int d0 = 2 * d2;
            const float theta = (float)p * inv_freq[d2];
            float sn, cs;
            __sincosf(theta, &sn, &cs);
            const float q0 = lds_q[d0], q1 = lds_q[d0 + 1];
            const float k0 = lds_p[d0], k1 = lds_p[d0 + 1];
            float qr0, qr1, kr0, kr1;
            rope_rotate(q0, q1, sn, cs, qr0, qr1);
            rope_rotate(k0, k1, sn, cs, kr0, kr1);
            lds_q[d0] = qr0 * inv_sqrt_d;
            lds_q[d0 + 1] = qr1 * inv_sqrt_d;
            kv_k[d0] = __float2half(kr0);
            kv_k[d0 + 1] = __float2half(kr1);
        }
        // zero-pad lds_q to the score loop's octet width
        for (int d = D + (int)threadIdx.x; d < ((D + 7) & ~7); d += BLOCK)
            lds_q[d] = 0.0f;
        // same-block visibility of the new K/V row: stores above are this
        // CU's own L1 write-through; __syncthreads orders them before the
        // scan loop's loads (cross-CU coherence is not needed — decode
        // tokens are distinct sequences, no other block reads this row)
        __syncthreads();
    } else {
        const int Dp = (D + 7) & ~7;  // scores read whole octets
        for (int d = threadIdx.x; d < Dp; d += BLOCK)
            lds_q[d] = (d < D)
                ? q_buf[(size_t)t * E + h * D + d] * inv_sqrt_d
                : 0.0f;
        __syncthreads();
    }

    // Flash-style per-wave streaming (zero __syncthreads in the loop):
    // wave w owns 4-row groups g ≡ w (mod 4); within the wave, lane
    // (sub = lane>>4, oct = lane&15) covers row (g*4 + sub)'s d-octet
    // oct*8 — one 16 B load each for K and V per row, the row's dot
    // reduced by a 4-step in-16 shuffle butterfly, q held in registers.
    // Each wave keeps private (m, l, o8) partials; one flash merge at
    // the end. (The earlier block-synchronized form paid 3 barriers +
    // 2 cross-wave reductions per 256-row chunk and scalar-width V
    // loads before that — the deep-decode ladder in
    // profiles/r2_deep_decode_ladder.md tracks the steps.)
    const int wid = threadIdx.x / WAVE;
    const int lane0 = threadIdx.x & (WAVE - 1);
    const int sub0 = lane0 >> 4;        // row within the 4-row group
    const int oct0 = lane0 & 15;        // d-octet within the row
    const int d0 = oct0 * 8;
    float q8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int d = d0 + e;
        if (FUSEQKV) {
            q8[e] = (d < D) ? lds_q[d] : 0.0f;  // prescaled in prologue
        } else {
            q8[e] = (d < D)
                ? q_buf[(size_t)t * E + h * D + d] * inv_sqrt_d
                : 0.0f;
        }
    }
    float m = -INFINITY, l = 0.0f;
    float o8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = 0.0f;

    // two 4-row groups per iteration: both K loads issue before either
    // dot needs them, and the 8 rows share one max/rescale pass
    for (int g = wid; g * 4 < J; g += 2 * NWAVES) {
        const int j1 = g * 4 + sub0;
        const int g2i = g + NWAVES;
        const int j2 = g2i * 4 + sub0;
        const bool ok1 = j1 < J;
        const bool ok2 = (g2i * 4 < J) && (j2 < J);
        float s1 = 0.0f, s2 = 0.0f;
        if (d0 < D) {
            float f1[8], f2[8];
            load_voct(k_cache + base + (size_t)(ok1 ? j1 : 0) * Ekv, d0,
                      f1);
            load_voct(k_cache + base + (size_t)(ok2 ? j2 : 0) * Ekv, d0,
                      f2);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s1 = fmaf(f1[e], q8[e], s1);
                s2 = fmaf(f2[e], q8[e], s2);
            }
        }
        // full dots: butterfly over the 16 octet lanes
#pragma unroll
        for (int sh = 1; sh <= 8; sh <<= 1) {
            s1 += __shfl_xor(s1, sh);
            s2 += __shfl_xor(s2, sh);
        }
        if (!ok1) s1 = -INFINITY;
        if (!ok2) s2 = -INFINITY;
        // max over all 8 rows (sub groups at lane bits 4-5)
        float gm = fmaxf(s1, s2);
        gm = fmaxf(gm, __shfl_xor(gm, 16));
        gm = fmaxf(gm, __shfl_xor(gm, 32));
        if (gm > m) {  // rescale partials (wave-uniform branch)
            const float alpha = (m == -INFINITY) ? 0.0f : __expf(m - gm);
#pragma unroll
            for (int e = 0; e < 8; ++e) o8[e] *= alpha;
            l *= alpha;
            m = gm;
        }
        const float p1 = ok1 ? __expf(s1 - m) : 0.0f;
        const float p2 = ok2 ? __expf(s2 - m) : 0.0f;
        float psum = (p1 + p2) + __shfl_xor(p1 + p2, 16);
        psum += __shfl_xor(psum, 32);
        l += psum;
        if (d0 < D) {
            float f1[8], f2[8];
            // masked rows contribute p = 0 (V row 0 is a safe address)
            load_voct(v_cache + base + (size_t)(ok1 ? j1 : 0) * Ekv, d0,
                      f1);
            load_voct(v_cache + base + (size_t)(ok2 ? j2 : 0) * Ekv, d0,
                      f2);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o8[e] = fmaf(p1, f1[e], o8[e]);
                o8[e] = fmaf(p2, f2[e], o8[e]);
            }
        }
    }

    // flash merge of the 4 waves' (m, l) x 16 (wave, sub) o8 partials
    {
        float* lds_m = lds_red;               // [NWAVES]
        float* lds_l = lds_red + NWAVES;      // [NWAVES]
        float* lds_o = lds_l + NWAVES;        // [16][128]
        const int gidx = wid * 4 + sub0;
#pragma unroll
        for (int e = 0; e < 8; ++e) lds_o[gidx * 128 + d0 + e] = o8[e];
        if (lane0 == 0) {
            lds_m[wid] = m;
            lds_l[wid] = l;
        }
        __syncthreads();
        if (threadIdx.x < D) {
            const int d = threadIdx.x;
            float mstar = -INFINITY;
#pragma unroll
            for (int w = 0; w < NWAVES; ++w)
                mstar = fmaxf(mstar, lds_m[w]);
            float lstar = 0.0f, num = 0.0f;
#pragma unroll
            for (int w = 0; w < NWAVES; ++w) {
                const float mw = lds_m[w];
                const float sc =
                    (mw == -INFINITY) ? 0.0f : __expf(mw - mstar);
                lstar += lds_l[w] * sc;
                num += sc * (lds_o[(w * 4 + 0) * 128 + d] +
                             lds_o[(w * 4 + 1) * 128 + d] +
                             lds_o[(w * 4 + 2) * 128 + d] +
                             lds_o[(w * 4 + 3) * 128 + d]);
            }
            const float v = num / lstar;
            const int e = h * D + d;
            out[(size_t)t * E + e] = v;
            if (out_prep != nullptr) {
                // f16 B-layout side-channel for the wo MFMA consumer
                union { __half h; unsigned short u; } c;
                c.h = __float2half(v);
                out_prep[xprep_index(e, t, jtw)] = c.u;
            }
        }
    }
}

// --------------------------------------- prefill flash attention (MFMA)
// Matrix-core flash attention for the large-M prefill path (D <= 128):
// one block = one (16-query tile, head); each of the 4 waves streams a
// strided subset of the 16-row KV tiles FULLY IN REGISTERS — scores via
// mfma_f32_16x16x32_f16 (A = K tile, B = the staged Q tile, C rows = j,
// cols = q), online softmax on the 4 score rows each lane holds, then
// PV via mfma_f32_16x16x16_f16 where the score C-layout (lane: q =
// l&15, j = (l>>4)*4+jj) IS the B-operand layout (cols q, k-dim j) —
// no transpose, no LDS, no syncs in the inner loop. Partial (m, l, O)
// merge across waves once at the end. Mixed admission streams: a query
// tile may span several sequences; the block processes each same-seq
// segment separately (causality per token via its own pos, exactly like
// k_attention). (The VALU kernel this replaced measured ~25x off the
// issue roofline — 16x16 tiles of dot products belong on MFMA.)

// 8 halves [d0, d0+8) of `row`, zero-padded past D
__device__ __forceinline__ f16x8 load_kfrag8(const __half* __restrict__ row,
                                             int d0, int D) {
    ABFrag a;
    if (d0 + 8 <= D) {
        const uint4 u = *reinterpret_cast<const uint4*>(row + d0);
        a.u[0] = u.x; a.u[1] = u.y; a.u[2] = u.z; a.u[3] = u.w;
    } else {
        __half tmp[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            tmp[e] = (d0 + e < D) ? row[d0 + e] : __half(0.0f);
        const uint4 u = *reinterpret_cast<const uint4*>(tmp);
        a.u[0] = u.x; a.u[1] = u.y; a.u[2] = u.z; a.u[3] = u.w;
    }
    return a.v;
}

__global__ __launch_bounds__(BLOCK) void k_attn_prefill_mfma(
    const float* __restrict__ q_buf, const __half* __restrict__ k_cache,
    const __half* __restrict__ v_cache, float* __restrict__ out,
    unsigned short* __restrict__ out_prep, const int* __restrict__ pos,
    const int* __restrict__ seq, int E, int Ekv, int D, int n_ctx,
    int jtw, int T) {
    constexpr int QT = 16;
    constexpr int DCMAX = 8;            // D <= 128 = 8 chunks of 16
    const int t0 = blockIdx.x * QT;
    const int h = blockIdx.y;
    const int nq = min(QT, T - t0);
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;
    const int lq = lane & 15;           // this lane's query column
    const int lg = lane >> 4;           // lane group (j/k sub-span)
    const int ndc = (D + 15) >> 4;      // 16-wide d chunks (PV / output)
    const float inv_sqrt_d = rsqrtf((float)D);

    __shared__ int lds_pos[QT];
    __shared__ int lds_seq[QT];
    // per-wave partials for the final merge
    __shared__ float lds_m[NWAVES][QT];
    __shared__ float lds_l[NWAVES][QT];
    __shared__ float lds_o[NWAVES][QT][DCMAX * 16];

    if (tid < QT) {
        lds_pos[tid] = (t0 + tid < T) ? pos[t0 + tid] : 0;
        lds_seq[tid] = (t0 + tid < T) ? seq[t0 + tid] : -1;
    }
    __syncthreads();

    // stage Q as score-MFMA B fragments: lane (col q=lq, k-span lg*8
    // within each 32-d chunk), prescaled by 1/sqrt(D), zero past D/nq
    ABFrag qf[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        __half tmp[8];
        const int d0 = c * 32 + lg * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = 0.0f;
            if (t0 + lq < T && d0 + e < D)
                v = q_buf[(size_t)(t0 + lq) * E + h * D + d0 + e] *
                    inv_sqrt_d;
            tmp[e] = __float2half(v);
        }
        const uint4 u = *reinterpret_cast<const uint4*>(tmp);
        qf[c].u[0] = u.x; qf[c].u[1] = u.y;
        qf[c].u[2] = u.z; qf[c].u[3] = u.w;
    }

    float m = -INFINITY, l = 0.0f;      // running state for column lq
    f32x4 oacc[DCMAX];
#pragma unroll
    for (int dc = 0; dc < DCMAX; ++dc)
        oacc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int pos_q = lds_pos[min(lq, nq - 1)];
    int a = 0;
    while (a < nq) {  // same-sequence segments of the query tile
        const int sseq = lds_seq[a];
        int b = a + 1;
        while (b < nq && lds_seq[b] == sseq) ++b;
        int jmax = 0;
        for (int q = a; q < b; ++q) jmax = max(jmax, lds_pos[q]);
        const int J = jmax + 1;
        const bool active = (lq >= a && lq < b);
        const int hk = h / ((int)gridDim.y / (Ekv / D));  // GQA kv head
        const size_t base = (size_t)sseq * n_ctx * Ekv + hk * D;

        // wave w streams tiles w, w+4, w+8, ... of this segment
        for (int tj = wid * 16; tj < J; tj += NWAVES * 16) {
            // scores: A = K rows (lane: row j=lq of the tile, k-span lg)
            const bool jrow_ok = (tj + lq) < J;  // tile tail: no OOB read
            const __half* krow =
                k_cache + base + (size_t)(jrow_ok ? tj + lq : 0) * Ekv;
            f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c * 32 >= D) break;
                f16x8 kf = load_kfrag8(krow, c * 32 + lg * 8, D);
                if (!jrow_ok) kf = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
                sc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[c].v,
                                                            sc, 0, 0, 0);
            }
            // lane now holds s[j = tj + lg*4 + jj][q = lq]; mask + max
            float s[4], tm = -INFINITY;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = tj + lg * 4 + jj;
                s[jj] = (active && j < J && j <= pos_q) ? sc[jj]
                                                        : -INFINITY;
                tm = fmaxf(tm, s[jj]);
            }
            tm = fmaxf(tm, __shfl_xor(tm, 16));
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            // wave-uniform skip only (divergent MFMA is illegal); lanes
            // whose q saw nothing yet keep (m=-inf, l=0, o=0) via
            // dead-lane handling below — never compute -inf - -inf
            if (!__any(tm != -INFINITY)) continue;
            const float m_new = fmaxf(m, tm);
            const bool dead = (m_new == -INFINITY);
            const float alpha =
                (dead || m == -INFINITY) ? (dead ? 1.0f : 0.0f)
                                         : __expf(m - m_new);
            BFrag4 p;
            float ts = 0.0f;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float pv = dead ? 0.0f : __expf(s[jj] - m_new);
                ts += pv;
                reinterpret_cast<__half*>(p.u)[jj] = __float2half(pv);
            }
            ts += __shfl_xor(ts, 16);
            ts += __shfl_xor(ts, 32);
            l = l * alpha + ts;
            m = m_new;
#pragma unroll
            for (int dc = 0; dc < DCMAX; ++dc) {
                if (dc >= ndc) break;
                oacc[dc][0] *= alpha; oacc[dc][1] *= alpha;
                oacc[dc][2] *= alpha; oacc[dc][3] *= alpha;
            }
            // PV: A = V^T (lane: row d = dc*16+lq, k-span j = lg*4+e);
            // B = p (exactly the score C layout). Masked j rows carry
            // p = 0; KV memory is zero-initialized so V rows past J
            // are finite.
#pragma unroll
            for (int dc = 0; dc < DCMAX; ++dc) {
                if (dc >= ndc) break;
                const int d = dc * 16 + lq;
                BFrag4 vt;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = tj + lg * 4 + e;
                    __half v(0.0f);
                    if (d < D && j < J)
                        v = v_cache[base + (size_t)j * Ekv + d];
                    reinterpret_cast<__half*>(vt.u)[e] = v;
                }
                oacc[dc] = __builtin_amdgcn_mfma_f32_16x16x16f16(
                    vt.v, p.v, oacc[dc], 0, 0, 0);
            }
        }
        a = b;
    }

    // merge the 4 waves' partials (each lane group holds redundant
    // copies of (m, l) for its q; group 0 writes)
    if (lg == 0) {
        lds_m[wid][lq] = m;
        lds_l[wid][lq] = l;
    }
#pragma unroll
    for (int dc = 0; dc < DCMAX; ++dc) {
        if (dc >= ndc) break;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            lds_o[wid][lq][dc * 16 + lg * 4 + jj] = oacc[dc][jj];
    }
    __syncthreads();
    // thread (q, d) recombines: 256 threads cover 16 q x 16 d per pass
    const int qq = tid >> 4;
    for (int d = tid & 15; d < D; d += 16) {
        if (qq >= nq) break;
        float mstar = -INFINITY;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w)
            mstar = fmaxf(mstar, lds_m[w][qq]);
        if (mstar == -INFINITY) mstar = 0.0f;  // no unmasked rows
        float lstar = 0.0f, ostar = 0.0f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) {
            const float mw = lds_m[w][qq];
            const float sc = (mw == -INFINITY) ? 0.0f
                                               : __expf(mw - mstar);
            lstar += lds_l[w][qq] * sc;
            ostar += lds_o[w][qq][d] * sc;
        }
        const float v = ostar / fmaxf(lstar, 1e-20f);
        const int e = h * D + d;
        const int t = t0 + qq;
        out[(size_t)t * E + e] = v;
        if (out_prep != nullptr) {
            union { __half h; unsigned short u; } cvt;
            cvt.h = __float2half(v);
            out_prep[xprep_index(e, t, jtw)] = cvt.u;
        }
    }
}

// ------------------------------------------- GQA decode attention (MFMA)
// Decode attention whose unit of work is (token, KV head): the grp = H/Hkv
// query heads that share a KV head are the 16 columns of one MFMA tile, so
// every K/V row is read once per group instead of once per query head.
// Grid (T, Hkv * ceil(grp/16), S): block (t, y, s) owns up to 16 query
// heads of KV head y / ceil(grp/16) over rows [s*chunk, min(J, (s+1)*chunk))
// of the token's context. Operand geometry is k_attn_prefill_mfma's (scores
// A = K tile, B = Q; PV A = V^T, B = p in the score C layout); what differs
// is how the operands arrive: K and V are both fetched as 16-byte row-major
// loads one tile ahead of the MFMAs, and V reaches its A layout through a
// wave-private LDS tile (gqa_stage_v) - no block barrier inside the loop.
//
// A wave's first tile has at least one attended row, so its running max is
// finite from then on and no -inf - -inf can occur; columns past grp carry
// q = 0 (uniform p, finite) and are never stored.
//
// These kernels are compiled without packed-f32 VALU instructions: GQA_FN
// and the gqa_ helpers on compiler builtins, attn_common.h.

constexpr int GQA_MIN_CHUNK = 256;  // rows per split, lower bound (unmeasured)
constexpr int GQA_MAX_SPLITS = 8;   // splits of a full context (unmeasured)

int attn_gqa_chunk(int n_ctx) {
    const int per = (n_ctx + GQA_MAX_SPLITS - 1) / GQA_MAX_SPLITS;
    return std::max(GQA_MIN_CHUNK, (per + 63) & ~63);
}

int attn_gqa_splits(int n_ctx, int T) {
    if (T > 64) return 1;  // wide decode fills the chip by itself
    const int chunk = attn_gqa_chunk(n_ctx);
    return (n_ctx + chunk - 1) / chunk;
}

int attn_route(int H, int Hkv, int T, int decode, int gqa_attention) {
    if (T > 64 && !decode) return 1;
    const int grp = H / Hkv;
    return (gqa_attention && grp >= 2 && grp <= 64) ? 2 : 0;
}

// GqaTile, gqa_stage_v and gqa_tile_step: attn_common.h (shared with
// attention_paged.hip).
//
// Sixteen-byte loads with no branch around them, so that the compiler can
// keep the next tile's loads in flight behind the current tile's (vmcnt
// counts only straight-line loads). The scheduling barrier at the end pins
// them above whatever the caller does next. Every address is valid: rows at or past
// `jend` read row 0 (masked by the caller) and spans that start at or past D
// read span 0 (K: multiplied by q = 0; V: lands in columns >= D, which are
// never stored). A span that straddles D reads into the next head or the
// 16-half pad: finite, and dropped the same way.
template <int NKC>
GQA_FN __device__ __forceinline__ void gqa_load_tile(
    GqaTile<NKC>& t, const __half* __restrict__ kb,
    const __half* __restrict__ vb, int tj, int jend, int Ekv, int D, int lq,
    int lg) {
    const int jk = tj + lq;
    const __half* krow = kb + (size_t)(jk < jend ? jk : 0) * Ekv;
#pragma unroll
    for (int c = 0; c < NKC; ++c) {
        const int d0 = c * 32 + lg * 8;
        t.k[c] = *reinterpret_cast<const uint4*>(krow + (d0 < D ? d0 : 0));
    }
    const int dv = (lq * 8 < D) ? lq * 8 : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int jv = tj + lg * 4 + e;
        const __half* vrow = vb + (size_t)(jv < jend ? jv : 0) * Ekv;
        t.v[e] = *reinterpret_cast<const uint4*>(vrow + dv);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// DC = 16-wide d chunks of the PV product, a power of two >= D/16; the
// score product runs NKC = max(1, DC/2) 32-wide chunks. Chunks past D work
// on zero q (scores) or produce columns that are never stored (PV).
template <int DC>
GQA_FN __global__ __launch_bounds__(BLOCK) void k_attn_gqa(
    const float* __restrict__ q_buf, const __half* __restrict__ k_cache,
    const __half* __restrict__ v_cache, float* __restrict__ out,
    unsigned short* __restrict__ out_prep, const int* __restrict__ pos,
    const int* __restrict__ seq, float* __restrict__ ws, int H, int grp,
    int E, int Ekv, int D, int n_ctx, int jtw, int chunk) {
    constexpr int NKC = DC > 1 ? DC / 2 : 1;
    constexpr int QW = NKC * 32;        // staged q row, halves
    const int t = blockIdx.x;
    const int J = pos[t] + 1;
    const int cs = (int)blockIdx.z * chunk;
    if (cs >= J) return;                // block-uniform
    const int ce = min(J, cs + chunk);
    const int ntile = (grp + 15) >> 4;  // column tiles per KV head
    const int hk = (int)blockIdx.y / ntile;
    const int c0 = ((int)blockIdx.y % ntile) * 16;  // first column's head
    const int ncol = min(16, grp - c0);
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);  // scalar
    const int lq = lane & 15;
    const int lg = lane >> 4;
    const float inv_sqrt_d = rsqrtf((float)D);
    const size_t base = (size_t)seq[t] * n_ctx * Ekv + hk * D;
    const __half* kb = k_cache + base;
    const __half* vb = v_cache + base;

    // One LDS region, used twice: the waves' V tiles and the staged Q while
    // streaming, the waves' O partials [w][col][OSTR] after it (OSTR skews
    // the 16 columns by 4 banks each).
    constexpr int OSTR = DC * 16 + 4;
    constexpr int VT_BYTES = NWAVES * 4 * GQA_VSTRIDE * (int)sizeof(uint2);
    constexpr int Q_BYTES = 16 * (QW + 8) * (int)sizeof(_Float16);
    constexpr int O_BYTES = NWAVES * 16 * OSTR * (int)sizeof(float);
    constexpr int LDS_BYTES =
        VT_BYTES + Q_BYTES > O_BYTES ? VT_BYTES + Q_BYTES : O_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    __shared__ float lds_m[NWAVES][16];
    __shared__ float lds_l[NWAVES][16];
    uint2* vt = reinterpret_cast<uint2*>(lds_raw) + wid * 4 * GQA_VSTRIDE;
    _Float16 (*lds_q)[QW + 8] =
        reinterpret_cast<_Float16 (*)[QW + 8]>(lds_raw + VT_BYTES);
    float* lds_o = reinterpret_cast<float*>(lds_raw);

    // Q tile -> LDS as f16, prescaled by 1/sqrt(D), zero past D and past
    // the group's last head (the factor, not a branch, does the masking:
    // the loads stay independent). The ncol heads are contiguous in q_buf.
    {
        const float* qt = q_buf + (size_t)t * E + (size_t)(hk * grp + c0) * D;
#pragma unroll
        for (int i = 0; i < 16 * QW / BLOCK; ++i) {
            const int idx = tid + i * BLOCK;
            const int col = idx / QW;
            const int d = idx % QW;
            const bool ok = col < ncol && d < D;
            const float v = qt[ok ? col * D + d : 0] *
                            (ok ? inv_sqrt_d : 0.0f);
            lds_q[col][d] = (_Float16)v;
        }
    }
    gqa_block_sync();
    // score-MFMA B fragments: lane (column lq, k-span lg*8 of 32-d chunk c)
    ABFrag qf[NKC];
#pragma unroll
    for (int c = 0; c < NKC; ++c) {
        const uint4 u =
            *reinterpret_cast<const uint4*>(&lds_q[lq][c * 32 + lg * 8]);
        qf[c].u[0] = u.x; qf[c].u[1] = u.y;
        qf[c].u[2] = u.z; qf[c].u[3] = u.w;
    }

    float m = -INFINITY, l = 0.0f;      // running state of column lq
    f32x4 oacc[DC];
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) oacc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Wave w streams tiles w, w+4, ... of the chunk, two per iteration in
    // two buffers that swap roles (a copy would wait for the loads it is
    // meant to keep in flight). Every tile's loads are issued one tile
    // ahead, before the previous tile's MFMAs, and nothing but that tile's
    // arithmetic lies between a load and its use: no branch the loads could
    // sink below. The price is that an odd tile count ends with one tile
    // wholly past the chunk, which reads row 0, is masked and changes
    // nothing. The first tile's loads follow the Q staging.
    int tj = cs + wid * 16;
    if (tj < ce) {                      // wave-uniform, scalar
        GqaTile<NKC> cur, alt;
        gqa_load_tile(cur, kb, vb, tj, ce, Ekv, D, lq, lg);
        do {
            gqa_load_tile(alt, kb, vb, tj + NWAVES * 16, ce, Ekv, D, lq, lg);
            gqa_tile_step<DC, NKC>(cur, qf, vt, tj, ce, lane, m, l, oacc);
            gqa_load_tile(cur, kb, vb, tj + 2 * NWAVES * 16, ce, Ekv, D, lq,
                          lg);
            gqa_tile_step<DC, NKC>(alt, qf, vt, tj + NWAVES * 16, ce, lane,
                                   m, l, oacc);
            tj += 2 * NWAVES * 16;
        } while (tj < ce);
    }
    gqa_block_sync();                   // V tiles and Q are dead: reuse LDS

    // merge the 4 waves' partials in wave order (lane group 0 holds the
    // column's (m, l); oacc[dc][jj] is O[d = dc*16 + lg*4 + jj][column lq])
    if (lg == 0) {
        lds_m[wid][lq] = m;
        lds_l[wid][lq] = l;
    }
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            lds_o[(wid * 16 + lq) * OSTR + dc * 16 + lg * 4 + jj] =
                oacc[dc][jj];
    }
    gqa_block_sync();
    const int col = tid >> 4;
    if (col >= ncol) return;
    const int h = hk * grp + c0 + col;
    float mstar = -INFINITY;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) mstar = fmaxf(mstar, lds_m[w][col]);
    float wsc[NWAVES], lstar = 0.0f;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const float mw = lds_m[w][col];         // -inf: wave had no tile
        wsc[w] = (mw == -INFINITY) ? 0.0f : __expf(mw - mstar);
        lstar += lds_l[w][col] * wsc[w];
    }
    const bool whole = J <= chunk;      // the token's only chunk: final
    float* part = ws + (((size_t)t * H + h) * gridDim.z + blockIdx.z) *
                           (size_t)(D + 2);
    if (!whole && (tid & 15) == 0) {
        part[0] = mstar;
        part[1] = lstar;
    }
    for (int d = tid & 15; d < D; d += 16) {
        float ostar = 0.0f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w)
            ostar += lds_o[(w * 16 + col) * OSTR + d] * wsc[w];
        if (!whole) {
            part[2 + d] = ostar;
            continue;
        }
        gqa_store_out(ostar / lstar, h * D + d, t, E, jtw, out, out_prep);
    }
}

// Combines the ceil(J/chunk) partials (m, l, o[D]) of one (token, head) in
// split order; tokens whose context fits one chunk were finished by
// k_attn_gqa. Grid (T, H), one thread per d.
GQA_FN __global__ void k_attn_gqa_merge(
    const float* __restrict__ ws, float* __restrict__ out,
    unsigned short* __restrict__ out_prep, const int* __restrict__ pos,
    int H, int E, int D, int jtw, int chunk, int S) {
    const int t = blockIdx.x;
    const int h = blockIdx.y;
    const int d = threadIdx.x;
    const int J = pos[t] + 1;
    if (J <= chunk || d >= D) return;
    const int n = (J + chunk - 1) / chunk;      // <= S
    const float* part = ws + ((size_t)t * H + h) * S * (size_t)(D + 2);
    float mstar = -INFINITY;
    for (int i = 0; i < n; ++i)
        mstar = fmaxf(mstar, part[(size_t)i * (D + 2)]);
    float lstar = 0.0f, ostar = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float* pi = part + (size_t)i * (D + 2);
        const float sc = __expf(pi[0] - mstar);
        lstar += pi[1] * sc;
        ostar += pi[2 + d] * sc;
    }
    gqa_store_out(ostar / lstar, h * D + d, t, E, jtw, out, out_prep);
}

// ------------------------------------------ shared-prefix attention (MFMA)
// Token t attends rows [0, pfx[t]) of slot `pslot` followed by rows
// [pfx[t], pos[t]] of its own slot seq[t]; pfx[t] is 0 or the common prefix
// length P. k_attn_prefix covers the prefix rows: the 16 tokens of a tile are
// the 16 MFMA columns of one (tile, query head, prefix chunk) block, so every
// prefix row is read once per 16 tokens. The streaming loop is k_attn_gqa's
// (same helpers, same two-buffer prefetch, no barrier and no branch around a
// load); what differs is the Q tile (16 tokens of one head instead of 16
// heads of one token), the K/V base (the prefix slot) and the epilogue, which
// always writes un-normalised partials (m, l, o[D]) to ws [T][H][S][D + 2].
// Columns without a prefix (pfx = 0, or past T) stream with q = 0: their
// arithmetic stays finite and is dropped, and the epilogue writes the empty
// partial (m = -inf, l = 0, o = 0) for those with t < T. MFMA columns are
// independent, so a token's partial does not depend on its tile mates or on
// its column. k_attn_prefix_tail then streams the token's own rows in f32
// (k_attention's per-wave form), folds the prefix partials in, normalises
// and stores.
constexpr int PFX_MIN_CHUNK = 256;  // prefix rows per split, lower bound (unmeasured)
constexpr int PFX_MAX_SPLITS = 8;   // splits of a full context (unmeasured)

int attn_prefix_chunk(int n_ctx) {
    const int per = (n_ctx + PFX_MAX_SPLITS - 1) / PFX_MAX_SPLITS;
    return std::max(PFX_MIN_CHUNK, (per + 63) & ~63);
}

int attn_prefix_splits(int n_ctx, int T) {
    if (T > 64) return 1;  // more than 4 tiles per head fill the chip
    const int chunk = attn_prefix_chunk(n_ctx);
    return (n_ctx + chunk - 1) / chunk;
}

template <int DC>
GQA_FN __global__ __launch_bounds__(BLOCK) void k_attn_prefix(
    const float* __restrict__ q_buf, const __half* __restrict__ k_cache,
    const __half* __restrict__ v_cache, const int* __restrict__ pfx,
    float* __restrict__ ws, int pslot, int P, int T, int grp, int E, int Ekv,
    int D, int n_ctx, int chunk) {
    constexpr int NKC = DC > 1 ? DC / 2 : 1;
    constexpr int QW = NKC * 32;        // staged q row, halves
    const int cs = (int)blockIdx.z * chunk;
    if (cs >= P) return;                // block-uniform: chunk past the prefix
    const int ce = min(P, cs + chunk);
    const int t0 = (int)blockIdx.x * 16;
    const int h = blockIdx.y;
    const int H = gridDim.y;
    const int hk = h / grp;             // GQA kv head
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);  // scalar
    const int lq = lane & 15;
    const int lg = lane >> 4;
    const float inv_sqrt_d = rsqrtf((float)D);
    const size_t base = (size_t)pslot * n_ctx * Ekv + hk * D;
    const __half* kb = k_cache + base;
    const __half* vb = v_cache + base;

    // LDS as in k_attn_gqa: V tiles + staged Q while streaming, the waves'
    // O partials [w][col][OSTR] after it
    constexpr int OSTR = DC * 16 + 4;
    constexpr int VT_BYTES = NWAVES * 4 * GQA_VSTRIDE * (int)sizeof(uint2);
    constexpr int Q_BYTES = 16 * (QW + 8) * (int)sizeof(_Float16);
    constexpr int O_BYTES = NWAVES * 16 * OSTR * (int)sizeof(float);
    constexpr int LDS_BYTES =
        VT_BYTES + Q_BYTES > O_BYTES ? VT_BYTES + Q_BYTES : O_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    __shared__ float lds_m[NWAVES][16];
    __shared__ float lds_l[NWAVES][16];
    __shared__ int lds_act[16];         // column's token shares the prefix
    uint2* vt = reinterpret_cast<uint2*>(lds_raw) + wid * 4 * GQA_VSTRIDE;
    _Float16 (*lds_q)[QW + 8] =
        reinterpret_cast<_Float16 (*)[QW + 8]>(lds_raw + VT_BYTES);
    float* lds_o = reinterpret_cast<float*>(lds_raw);

    if (tid < 16) {
        const int tc = t0 + tid;
        lds_act[tid] = (tc < T && pfx[tc < T ? tc : t0] > 0) ? 1 : 0;
    }
    gqa_block_sync();
    int nact = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) nact += lds_act[c];

    if (nact > 0) {                     // block-uniform
        // Q tile -> LDS as f16, prescaled by 1/sqrt(D); zero past D and in
        // columns without a prefix (the factor does the masking)
        {
            const float* qt = q_buf + (size_t)h * D;
#pragma unroll
            for (int i = 0; i < 16 * QW / BLOCK; ++i) {
                const int idx = tid + i * BLOCK;
                const int col = idx / QW;
                const int d = idx % QW;
                const bool ok = lds_act[col] != 0 && d < D;
                const float v =
                    qt[ok ? (size_t)(t0 + col) * E + d : (size_t)t0 * E] *
                    (ok ? inv_sqrt_d : 0.0f);
                lds_q[col][d] = (_Float16)v;
            }
        }
        gqa_block_sync();
        // score-MFMA B fragments: lane (column lq, k-span lg*8 of chunk c)
        ABFrag qf[NKC];
#pragma unroll
        for (int c = 0; c < NKC; ++c) {
            const uint4 u =
                *reinterpret_cast<const uint4*>(&lds_q[lq][c * 32 + lg * 8]);
            qf[c].u[0] = u.x; qf[c].u[1] = u.y;
            qf[c].u[2] = u.z; qf[c].u[3] = u.w;
        }

        float m = -INFINITY, l = 0.0f;  // running state of column lq
        f32x4 oacc[DC];
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) oacc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

        // wave w streams tiles w, w+4, ... of the chunk, two per iteration
        // (k_attn_gqa's loop: loads one tile ahead, a last tile wholly past
        // the chunk reads row 0 and is masked)
        int tj = cs + wid * 16;
        if (tj < ce) {                  // wave-uniform, scalar
            GqaTile<NKC> cur, alt;
            gqa_load_tile(cur, kb, vb, tj, ce, Ekv, D, lq, lg);
            do {
                gqa_load_tile(alt, kb, vb, tj + NWAVES * 16, ce, Ekv, D, lq,
                              lg);
                gqa_tile_step<DC, NKC>(cur, qf, vt, tj, ce, lane, m, l, oacc);
                gqa_load_tile(cur, kb, vb, tj + 2 * NWAVES * 16, ce, Ekv, D,
                              lq, lg);
                gqa_tile_step<DC, NKC>(alt, qf, vt, tj + NWAVES * 16, ce,
                                       lane, m, l, oacc);
                tj += 2 * NWAVES * 16;
            } while (tj < ce);
        }
        gqa_block_sync();               // V tiles and Q are dead: reuse LDS

        if (lg == 0) {
            lds_m[wid][lq] = m;
            lds_l[wid][lq] = l;
        }
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                lds_o[(wid * 16 + lq) * OSTR + dc * 16 + lg * 4 + jj] =
                    oacc[dc][jj];
        }
        gqa_block_sync();
    }

    // thread (col, d mod 16) writes the column's partial: the 4 waves merged
    // in wave order, or the empty partial
    const int col = tid >> 4;
    const int tc = t0 + col;
    if (tc >= T) return;
    float* part = ws + (((size_t)tc * H + h) * gridDim.z + blockIdx.z) *
                           (size_t)(D + 2);
    if (lds_act[col] == 0) {
        if ((tid & 15) == 0) {
            part[0] = -INFINITY;
            part[1] = 0.0f;
        }
        for (int d = tid & 15; d < D; d += 16) part[2 + d] = 0.0f;
        return;
    }
    float mstar = -INFINITY;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) mstar = fmaxf(mstar, lds_m[w][col]);
    float wsc[NWAVES], lstar = 0.0f;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const float mw = lds_m[w][col];         // -inf: wave had no tile
        wsc[w] = (mw == -INFINITY) ? 0.0f : __expf(mw - mstar);
        lstar += lds_l[w][col] * wsc[w];
    }
    if ((tid & 15) == 0) {
        part[0] = mstar;
        part[1] = lstar;
    }
    for (int d = tid & 15; d < D; d += 16) {
        float ostar = 0.0f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w)
            ostar += lds_o[(w * 16 + col) * OSTR + d] * wsc[w];
        part[2 + d] = ostar;
    }
}

// 8 halves at `p` as floats, one unconditional 16-byte load (load_voct's
// contract: whatever lies past D is finite and dropped by the caller)
GQA_FN __device__ __forceinline__ void pfx_load8(const __half* __restrict__ p,
                                                 float f[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    ABFrag a;
    a.u[0] = u.x; a.u[1] = u.y; a.u[2] = u.z; a.u[3] = u.w;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)a.v[e];
}

// One block per (token, head): rows [r0, pos[t]] of the token's own slot in
// f32 with r0 = P where pfx[t] > 0, else 0 (k_attention's streaming loop:
// wave w owns 4-row groups g = w mod 4, lane (sub, oct) one row's d-octet,
// two groups per iteration), then one merge of the ceil(P/chunk) prefix
// partials in ascending chunk order and of the 4 waves' partials in wave
// order. The own span holds at least row pos[t], so the sum is never empty.
GQA_FN __global__ __launch_bounds__(BLOCK) void k_attn_prefix_tail(
    const float* __restrict__ q_buf, const __half* __restrict__ k_cache,
    const __half* __restrict__ v_cache, float* __restrict__ out,
    unsigned short* __restrict__ out_prep, const int* __restrict__ pos,
    const int* __restrict__ seq, const int* __restrict__ pfx,
    const float* __restrict__ ws, int P, int grp, int E, int Ekv, int D,
    int n_ctx, int jtw, int chunk, int S) {
    const int t = blockIdx.x;
    const int h = blockIdx.y;
    const int H = gridDim.y;
    const int hk = h / grp;
    const int r0 = pfx[t] > 0 ? P : 0;
    const int J = pos[t] + 1 - r0;      // own rows r0 + [0, J)
    const size_t base =
        ((size_t)seq[t] * n_ctx + r0) * Ekv + (size_t)hk * D;
    const __half* kb = k_cache + base;
    const __half* vb = v_cache + base;
    const float inv_sqrt_d = rsqrtf((float)D);

    __shared__ float lds_m[NWAVES];
    __shared__ float lds_l[NWAVES];
    __shared__ float lds_o[16][128];

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;
    const int sub = lane >> 4;          // row within the 4-row group
    const int d0 = (lane & 15) * 8;     // d-octet within the row
    const bool dok = d0 < D;
    const int dl = dok ? d0 : 0;        // octets past D load octet 0, q = 0
    float q8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int d = d0 + e;
        q8[e] = (d < D) ? q_buf[(size_t)t * E + h * D + d] * inv_sqrt_d
                        : 0.0f;
    }
    float m = -INFINITY, l = 0.0f;
    float o8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = 0.0f;

    for (int g = wid; g * 4 < J; g += 2 * NWAVES) {
        const int j1 = g * 4 + sub;
        const int j2 = (g + NWAVES) * 4 + sub;
        const bool ok1 = j1 < J;
        const bool ok2 = j2 < J;
        float f1[8], f2[8];
        // masked rows read row 0 of the span: a valid address, dropped below
        pfx_load8(kb + (size_t)(ok1 ? j1 : 0) * Ekv + dl, f1);
        pfx_load8(kb + (size_t)(ok2 ? j2 : 0) * Ekv + dl, f2);
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            s1 = fmaf(f1[e], q8[e], s1);
            s2 = fmaf(f2[e], q8[e], s2);
        }
#pragma unroll
        for (int sh = 1; sh <= 8; sh <<= 1) {
            s1 += gqa_shfl_xor(s1, lane, sh);
            s2 += gqa_shfl_xor(s2, lane, sh);
        }
        if (!ok1) s1 = -INFINITY;
        if (!ok2) s2 = -INFINITY;
        float gm = fmaxf(s1, s2);
        gm = fmaxf(gm, gqa_shfl_xor(gm, lane, 16));
        gm = fmaxf(gm, gqa_shfl_xor(gm, lane, 32));
        // gm is finite: the group's first row is inside the span
        const float m_new = fmaxf(m, gm);
        const float alpha = __expf(m - m_new);      // 0 on the first group
#pragma unroll
        for (int e = 0; e < 8; ++e) o8[e] *= alpha;
        const float p1 = __expf(s1 - m_new);        // 0 for masked rows
        const float p2 = __expf(s2 - m_new);
        float psum = p1 + p2;
        psum += gqa_shfl_xor(psum, lane, 16);
        psum += gqa_shfl_xor(psum, lane, 32);
        l = l * alpha + psum;
        m = m_new;
        pfx_load8(vb + (size_t)(ok1 ? j1 : 0) * Ekv + dl, f1);
        pfx_load8(vb + (size_t)(ok2 ? j2 : 0) * Ekv + dl, f2);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o8[e] = fmaf(p1, f1[e], o8[e]);
            o8[e] = fmaf(p2, f2[e], o8[e]);
        }
    }

    if (dok) {
#pragma unroll
        for (int e = 0; e < 8; ++e) lds_o[wid * 4 + sub][d0 + e] = o8[e];
    }
    if (lane == 0) {
        lds_m[wid] = m;
        lds_l[wid] = l;
    }
    gqa_block_sync();
    const int d = tid;
    if (d >= D) return;
    const int n = r0 > 0 ? (P + chunk - 1) / chunk : 0;     // <= S
    const float* part = ws + ((size_t)t * H + h) * S * (size_t)(D + 2);
    float mstar = -INFINITY;
    for (int i = 0; i < n; ++i)
        mstar = fmaxf(mstar, part[(size_t)i * (D + 2)]);
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) mstar = fmaxf(mstar, lds_m[w]);
    float lstar = 0.0f, num = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float* pi = part + (size_t)i * (D + 2);
        const float sc = (pi[0] == -INFINITY) ? 0.0f : __expf(pi[0] - mstar);
        lstar += pi[1] * sc;
        num += pi[2 + d] * sc;
    }
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const float mw = lds_m[w];              // -inf: wave had no group
        const float sc = (mw == -INFINITY) ? 0.0f : __expf(mw - mstar);
        lstar += lds_l[w] * sc;
        num += sc * (lds_o[w * 4 + 0][d] + lds_o[w * 4 + 1][d] +
                     lds_o[w * 4 + 2][d] + lds_o[w * 4 + 3][d]);
    }
    gqa_store_out(num / lstar, h * D + d, t, E, jtw, out, out_prep);
}

// ============================================================== launchers

void launch_attn_prefix(hipStream_t s, const float* q_buf,
                        const __half* k_cache_layer,
                        const __half* v_cache_layer, float* out,
                        unsigned short* out_prep, const int* pos,
                        const int* seq, const int* pfx, int pslot, int P,
                        int T, int H, int Hkv, int E, int Ekv, int D,
                        int n_ctx, float* ws) {
    const int grp = H / Hkv;
    const int S = attn_prefix_splits(n_ctx, T);
    // one split covers the whole prefix, whatever its length
    const int chunk = (S == 1) ? std::max(n_ctx, PFX_MIN_CHUNK)
                               : attn_prefix_chunk(n_ctx);
    auto kern = D <= 16 ? k_attn_prefix<1> : D <= 32 ? k_attn_prefix<2>
              : D <= 64 ? k_attn_prefix<4> : k_attn_prefix<8>;
    hipLaunchKernelGGL(kern, dim3((T + 15) / 16, H, S), dim3(BLOCK), 0, s,
                       q_buf, k_cache_layer, v_cache_layer, pfx, ws, pslot, P,
                       T, grp, E, Ekv, D, n_ctx, chunk);
    hipLaunchKernelGGL(k_attn_prefix_tail, dim3(T, H), dim3(BLOCK), 0, s,
                       q_buf, k_cache_layer, v_cache_layer, out, out_prep,
                       pos, seq, pfx, ws, P, grp, E, Ekv, D, n_ctx,
                       jt_width(T), chunk, S);
}

void launch_attn_gqa(hipStream_t s, const float* q_buf,
                     const __half* k_cache_layer,
                     const __half* v_cache_layer, float* out,
                     unsigned short* out_prep, const int* pos,
                     const int* seq, int T, int H, int Hkv, int E, int Ekv,
                     int D, int n_ctx, float* ws) {
    const int grp = H / Hkv;
    const int S = attn_gqa_splits(n_ctx, T);
    // one split covers the whole context, whatever its length
    const int chunk = (S == 1) ? std::max(n_ctx, GQA_MIN_CHUNK)
                               : attn_gqa_chunk(n_ctx);
    const int jtw = jt_width(T);
    const dim3 grid(T, Hkv * ((grp + 15) / 16), S);
    auto kern = D <= 16 ? k_attn_gqa<1> : D <= 32 ? k_attn_gqa<2>
              : D <= 64 ? k_attn_gqa<4> : k_attn_gqa<8>;
    hipLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, s, q_buf, k_cache_layer,
                       v_cache_layer, out, out_prep, pos, seq, ws, H, grp, E,
                       Ekv, D, n_ctx, jtw, chunk);
    if (S > 1)
        launch_attn_gqa_merge(s, ws, out, out_prep, pos, T, H, E, D, jtw,
                              chunk, S);
}

void launch_attn_gqa_merge(hipStream_t s, const float* ws, float* out,
                           unsigned short* out_prep, const int* pos, int T,
                           int H, int E, int D, int jtw, int chunk, int S) {
    hipLaunchKernelGGL(k_attn_gqa_merge, dim3(T, H), dim3(128), 0, s, ws,
                       out, out_prep, pos, H, E, D, jtw, chunk, S);
}

void launch_attention(hipStream_t s, const float* q_buf,
                      const __half* k_cache_layer, __half* v_cache_layer,
                      float* out, unsigned short* out_prep, const int* pos,
                      const int* seq, int T, int H, int E, int Ekv, int D,
                      int n_ctx, const float* qkv_slab, int ks,
                      const float* inv_freq) {
    const dim3 grid(T, H);
    // lds_q[D] + prologue stage[BLOCK] + lds_m/lds_l[2*NWAVES] +
    // merge area [16][128]
    const size_t lds =
        (D + BLOCK + 2 * NWAVES + 16 * 128) * sizeof(float);
    if (qkv_slab != nullptr) {
        hipLaunchKernelGGL(k_attention<true>, grid, dim3(BLOCK), lds, s,
                           q_buf, k_cache_layer, v_cache_layer, out,
                           out_prep, pos, seq, E, Ekv, D, n_ctx,
                           jt_width(T), qkv_slab, ks, inv_freq);
        return;
    }
    hipLaunchKernelGGL(k_attention<false>, grid, dim3(BLOCK), lds, s, q_buf,
                       k_cache_layer, v_cache_layer, out, out_prep, pos, seq,
                       E, Ekv, D, n_ctx, jt_width(T), qkv_slab, ks,
                       inv_freq);
}

void launch_attn_prefill(hipStream_t s, const float* q_buf,
                         const __half* k_cache_layer,
                         const __half* v_cache_layer, float* out,
                         unsigned short* out_prep, const int* pos,
                         const int* seq, int T, int H, int E, int Ekv,
                         int D, int n_ctx) {
    // D <= 128 (DCMAX chunks of 16) is the SliceEngine constructor's check
    const dim3 grid((T + 15) / 16, H);
    hipLaunchKernelGGL(k_attn_prefill_mfma, grid, dim3(BLOCK), 0, s, q_buf,
                       k_cache_layer, v_cache_layer, out, out_prep, pos,
                       seq, E, Ekv, D, n_ctx, jt_width(T), T);
}
