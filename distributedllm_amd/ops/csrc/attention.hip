// Attention kernels of the slice engine (gfx950): the streaming
// online-softmax decode kernel `k_attention` (optionally fused with the qkv
// split-K finish: slab sum + RoPE + KV append in its prologue) and the
// matrix-core prefill flash kernel `k_attn_prefill_mfma`, with their two
// launchers. Both cover head dims D <= 128 only; the SliceEngine
// constructor rejects anything larger, so there is no fallback kernel.
//
// Not to be changed casually: k_attention's streaming loop (load order,
// shuffle butterflies, two-group iteration) and everything inside
// k_attn_prefill_mfma's tile loop were tuned against rocprofv3 counters
// (docs/kernels.md); both must stay bit-reproducible run to run.

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
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

union BFrag4 {
    uint32_t u[2];
    f16x4 v;
};

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

// ============================================================== launchers

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
