// MFMA dequant-GEMM family of the slice engine (gfx950) — the production
// path for every quantized / f16 layer, decode (T <= 64) and large-M
// prefill / wide decode (T > 64: `k_qkv16<…, true>`, `k_ffn16<…, true>`,
// `k_gemm16_mt`), plus the lm_head of prompt scoring at any T
// (`k_lmhead_score`: large-M grid, log-sum-exp epilogue, no logits). One
// launcher per layer op covers every T (launch_qkv16, launch_ffn16,
// launch_gemm16_residual); the route selectors above them pick the kernel.
// Design notes with the measurements that drove each choice:
// docs/kernels.md.
//
// Matrix cores do the FLOPs; the VALU only unpacks. One
// `mfma_f32_16x16x32_f16` consumes one 32-weight K-block of a 16-row tile.
// Weights are dequantized to f16 A fragments in exact packed-f16 VALU:
//   * q4_0/q4_1 nibbles: 0x6400 | n is exactly f16(1024 + n), so
//     w = alpha * ((1024+n) - c) + beta with one v_pk_add + one v_pk_fma
//     per word (a_frag_q4);
//   * the byte stream W_Q8B / W_Q8B16 (q8_0, q5_x and the k-quants,
//     re-biased to u8 at repack): 0x6400 | b == f16(1024 + b) likewise
//     (a_frag_q8), with (alpha, beta) per 32 or per 16 weights;
//   * W_F16 tiles load straight into the fragment.
// Activations ride an f16 side channel ("xprep", layout
// [cols/8][jtw][16][8] = exactly the B-fragment gather, see xprep_index)
// written by the producing kernel's epilogue; the f32 residual stream
// stays f32. RMSNorm is fused into the consumers' B-fragment build via a
// sumsq side channel written by the previous residual epilogue.
//
// A decode layer is 7-9 launches depending on model size: qkv (fused, or
// RT=2 slab split-K whose finish is either k_qkv_finish or the attention
// prologue), attention, wo (slab split-K + k_reduce_prep, or the fused
// GM_RES_SQ epilogue when E/16 is odd: gemm16_res_route), ffn gate (w1/w3
// + SwiGLU), w2 (like wo). A prefill layer is 5: large-M qkv, attention,
// wo, ffn, w2.
//
// Weight layout in HBM (repacked at load; python side in
// engine/repack.py::repack_mfma), R = rows/16 row tiles:
//   q4   : data   u32[R][nbp/4][4 ws][16 i][4 kb]  (one dwordx4 per lane
//          covers 4 consecutive K-blocks; nbp = nb padded to 4)
//          scales f16 (alpha, beta)[R][nbp/4][16 i][4 kb]
//   bytes: data   two u32 per lane per K-block in the same group order,
//          scales as q4 (W_Q8B16: two half-planes per block)
//   f16  : data   f16[R][cols/8][16 i][8]
// plus one prefetch batch of tail slack on every allocation.
//
// Block = 4 waves; each wave owns a quarter of the K blocks of its row
// tile(s); partial accumulators combine through LDS; wave 0 runs the
// fused epilogue. Decode and large-M differ only in how a block finds its
// (row tile, token tile): k_qkv16 and k_ffn16 take that as the template
// flag MTK; k_gemm16 / k_gemm16_mt stay two kernels (see k_gemm16_mt).
//
// Not to be changed casually: the bodies of wave_tile_kloop and
// combine_acc, the grid decoders of the kernels, and — less obviously —
// the shape of the epilogues (see "tile epilogues" below). Every line of
// the K loop's pipeline was settled against SQ counters and the emitted
// waits; merging kernels, turning template parameters into runtime
// values, or refactoring an epilogue changes the K loop's code generation.
// Compare per-kernel assembly and register counts before and after:
// tools/kernel_isa_diff.py OLD.hip NEW.hip does that without a GPU.

#include <type_traits>

#include "device_common.h"
#include "kernels.h"
#include "logprobs_key.h"

// k_gemm16 modes (described at the kernel). The values are template
// arguments — keep them stable. (0 and 3 were a plain store and an atomic
// split-K.)
enum GemmMode { GM_RES_SQ = 1, GM_NORM_PLAIN = 2, GM_SLAB = 4 };

// write-through 16 B store (sc0 sc1): the split-K slab publish leaves no
// dirty lines in the writer XCD's L2, so the consumer kernel's reads are
// not cross-XCD dirty-line snoops (write-through slab stores measured
// faster than plain stores + a boundary flush)
__device__ __forceinline__ void store_f4_wt(float* addr, float4 v) {
    f32x4 w = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1"
                 :: "v"(addr), "v"(w) : "memory");
}

// Per-wave state for the K loop: lane (i = l&15 row, ks = l>>4 k-span).
// For q4 weights every wave range is aligned to the 4-K-block load group
// (the repacked layout packs 4 consecutive K-blocks per dwordx4); ranges
// live in the PADDED block count (repack zero-pads nb to a multiple of 4
// with alpha=beta=0 blocks that contribute exact zeros).
struct KLoop {
    int lane, i, ks;
    int kb0, kb1;  // this wave's K-block range
    // split a [b0, b1) block range (grid-level split-K) across the waves;
    // align=4 for q4 group loads, 1 for f16
    __device__ void init_range(int b0, int b1, int align, int nwaves = NWAVES) {
        lane = threadIdx.x & (WAVE - 1);
        i = lane & 15;
        ks = lane >> 4;
        const int wid = threadIdx.x / WAVE;
        const int am = align - 1;
        int per = (b1 - b0 + nwaves - 1) / nwaves;
        per = (per + am) & ~am;
        // readfirstlane: wid is wave-uniform but derived from threadIdx,
        // so without this the compiler treats every K loop bounded by
        // kb0/kb1 as lane-divergent and wraps each iteration in exec-mask
        // bookkeeping (saveexec/or/andn2 + implicit-def accvgpr moves)
        kb0 = __builtin_amdgcn_readfirstlane(min(b1, b0 + wid * per));
        kb1 = __builtin_amdgcn_readfirstlane(min(b1, kb0 + per));
    }
};

// Dequantize one repacked nibble word into an f16 A fragment with pure
// packed-f16 VALU (no unpack-to-f32 shift/and per half — the bf16 variant
// of this dequant measured VALU-issue-bound):
//   0x6400 | n is EXACTLY the f16 value 1024+n, so
//   q4_0: w = alpha * ((1024+n) - 1032)        (n-8 exact in f16)
//   q4_1: w = alpha * ((1024+n) - 1024) + beta (beta = m)
// per word: and/shr/or unpack + one v_pk_add_f16 + one v_pk_fma_f16; the
// result is the correctly-rounded f16 of the true q4 value (single
// rounding). ab = (beta_f16 << 16) | alpha_f16 per (row, block).
template <int WT>
__device__ __forceinline__ void a_frag_q4(uint32_t q, uint32_t ab,
                                          ABFrag& a) {
    const __half2 abh = u2h2(ab);
    const __half2 alpha2 = __half2half2(__low2half(abh));
    const __half2 beta2 = __half2half2(__high2half(abh));
    // f16 bit patterns: -1032 = 0xE408, -1024 = 0xE400
    const uint32_t csub = (WT == W_Q4_0) ? 0xE408E408u : 0xE400E400u;
    const __half2 c2 = u2h2(csub);
    uint32_t w[4];
    w[0] = 0x64006400u | (q & 0x000F000Fu);
    w[1] = 0x64006400u | ((q >> 4) & 0x000F000Fu);
    w[2] = 0x64006400u | ((q >> 8) & 0x000F000Fu);
    w[3] = 0x64006400u | ((q >> 12) & 0x000F000Fu);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const __half2 v = __hadd2(u2h2(w[i]), c2);
        a.u[i] = h22u(__hfma2(v, alpha2, beta2));
    }
}

// Byte-stream A fragment (W_Q8B): 8 re-biased u8 weights arrive as two
// u32 with byte order [w0,w2,w1,w3] / [w4,w6,w5,w7], so the same mask
// trick as q4 yields f16 pairs: 0x6400|b == f16(1024+b) exactly for
// b in [0,255], then w = alpha*((1024+b) - 1152) + beta (csub -1152 =
// 0xE480; repack re-biases q8_0 by +128 and q5_x by +112 so one csub
// serves all three formats).
__device__ __forceinline__ void a_frag_q8(uint32_t qA, uint32_t qB,
                                          uint32_t ab, ABFrag& a) {
    const __half2 abh = u2h2(ab);
    const __half2 alpha2 = __half2half2(__low2half(abh));
    const __half2 beta2 = __half2half2(__high2half(abh));
    const __half2 c2 = u2h2(0xE480E480u);  // f16 -1152
    uint32_t w[4];
    w[0] = 0x64006400u | (qA & 0x00FF00FFu);
    w[1] = 0x64006400u | ((qA >> 8) & 0x00FF00FFu);
    w[2] = 0x64006400u | (qB & 0x00FF00FFu);
    w[3] = 0x64006400u | ((qB >> 8) & 0x00FF00FFu);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const __half2 v = __hadd2(u2h2(w[i]), c2);
        a.u[i] = h22u(__hfma2(v, alpha2, beta2));
    }
}

// One wave's software-pipelined K loop over NM matrices sharing the B
// panel (NM=2 for the FFN's w1/w3) and JT 16-token column tiles sharing
// the A (weight) stream. JT is THE batched-decode lever: the HBM weight
// stream and the dequant VALU are paid once for JT*16 tokens, so decode
// tokens/s scales nearly linearly in JT while the kernel wall barely
// moves (memory-bound).
//
// Pipeline shape (all learned from SQ counters / emitted waits):
//  * rotated two-deep UNCONDITIONAL prefetch of the weight batch — a
//    branch around loads makes hipcc drain vmcnt inside the body; the
//    last iteration overreads ONE batch (tail slack in every allocation),
//  * the (L2-resident) B-panel loads of batch g issue BEFORE the HBM
//    weight loads of batch g+1: vmcnt retires in issue order, so B loads
//    issued after the prefetch could not complete before it,
//  * per-batch pointers advance by constant strides (no per-load 64-bit
//    address math),
//  * wave-uniform loop bounds via readfirstlane (no exec-mask loop),
//  * accumulation is MFMA C-chained over two alternating accumulator
//    sets (covers dependent-accumulator latency).
// acc[n][jt][jj] ends with rows (l>>4)*4+jj, col jt*16 + (l&15).
// RT = row tiles per wave: the wave's B fragments feed RT A-tile streams,
// dividing the (L2-heavy) B-panel re-read traffic and the B-build VALU by
// RT. acc[rt][n][jt][jj].
// jtw/jt0: token-panel stride and first 16-token tile of this block in the
// xprep side channel (layout [kc][jtw][16][8]). Decode callers pass
// (JT, 0); the large-M kernels tile a T-wide panel with jtw = ceil(T/16)
// padded to the 4-tile group and jt0 = mtile*JT.
template <int WT, bool NORM, int NM, int JT, int RT = 1, int PF = 4,
          int NW = NWAVES>
__device__ __forceinline__ void wave_tile_kloop(
    const WMat2* const* ws, int tile_row,
    const unsigned short* __restrict__ xprep,
    const unsigned short* __restrict__ normprep,
    const float* __restrict__ ss_in, float eps,
    float acc[RT][NM][JT][4], int b0, int b1, int jtw = JT, int jt0 = 0) {
    KLoop kl;
    kl.init_range(b0, b1, (WT == W_F16) ? 1 : 4, NW);
    const int nb0 = ws[0]->cols >> 5;
    const int nb = (WT == W_F16) ? nb0 : ((nb0 + 3) & ~3);  // padded count
    // u32 per lane per K-block: 1 for q4 nibbles, 2 for the byte stream
    constexpr int QW = (WT == W_Q8B || WT == W_Q8B16) ? 2 : 1;
    // scale planes: W_Q8B16 carries one (alpha, beta) pair per 16
    // weights — lane k-span ks selects its half-plane (ks >> 1)
    constexpr int ABW = (WT == W_Q8B16) ? 2 : 1;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // With >=4 independent MFMAs per K-block (JT/NM/RT product) the
    // accumulator reuse distance already covers the MFMA dependent
    // latency — and the runtime `parity ? c1 : c0` reference select is
    // poison: the compiler materialized it as per-MFMA cndmask + AGPR
    // read/write round-trips (338 of 445 inner-loop instructions in the
    // JT=4 ffn kernel). Only the low-parallelism shapes keep the pair.
    constexpr int NP = (NM * JT * RT >= 4) ? 1 : 2;
    f32x4 c0[RT][NM][JT], c1[NP == 2 ? RT : 1][NM][JT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int n = 0; n < NM; ++n)
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                c0[rt][n][jt] = zero;
                if (NP == 2) c1[rt][n][jt] = zero;
            }

    // per-column-tile RMSNorm scale, hoisted (column j = lane&15 of tile jt)
    __half2 scale2[JT];
    if (NORM) {
        const float inv_cols = 1.0f / (float)ws[0]->cols;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
            scale2[jt] = __float2half2_rn(
                rsqrtf(ss_in[(jt0 + jt) * 16 + kl.i] * inv_cols + eps));
    }

    const uint32_t* qp[RT][NM];
    const uint32_t* abp[RT][NM];
    const unsigned short* tp[RT][NM];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int n = 0; n < NM; ++n) {
            const int tr = tile_row * RT + rt;
            qp[rt][n] = (const uint32_t*)ws[n]->data +
                        ((size_t)tr * nb + kl.kb0) * 64 * QW +
                        (kl.ks * 16 + kl.i) * 4 * QW;
            abp[rt][n] = (const uint32_t*)ws[n]->scales +
                         ((size_t)tr * nb + kl.kb0) * 16 * ABW +
                         (ABW == 2 ? (kl.ks >> 1) * 64 : 0) + kl.i * 4;
            tp[rt][n] = (const unsigned short*)ws[n]->data +
                        ((size_t)tr * (ws[n]->cols >> 3)) * 128 +
                        ((size_t)(kl.kb0 * 4 + kl.ks) * 16 + kl.i) * 8;
        }
    // xprep layout: element (kc, jt, j, e) at ((kc*jtw + jt)*16 + j)*8 + e
    const unsigned short* xp =
        xprep + ((size_t)(kl.kb0 * 4 + kl.ks) * jtw + jt0) * 128 + kl.i * 8;
    const unsigned short* np =
        normprep + (NORM ? (size_t)(kl.kb0 * 4 + kl.ks) * 8 : 0);

    struct Batch {  // weight stream only (HBM, nt, double-buffered)
        u32x4 q[(PF / 4) * QW][RT][NM], ab[PF / 4][RT][NM];
        uint4 aw[PF][RT][NM];
    };
    // NAMED buffers, never indexed by a runtime value (a runtime select
    // sends the array to scratch: measured 240-336 B/lane and 3x slower).
    Batch bufA, bufB;
    struct XPanel {  // B-panel side channel (L2-resident, per iteration)
        uint4 xb[PF][JT];
        uint4 nbv[PF];
    };

    auto load_w = [&](Batch& bt) {
#pragma unroll
        for (int u4 = 0; u4 < PF / 4; ++u4) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int n = 0; n < NM; ++n) {
                    if (WT == W_F16) {
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            bt.aw[u4 * 4 + v][rt][n] =
                                *reinterpret_cast<const uint4*>(
                                    tp[rt][n] + (u4 * 4 + v) * 512);
                    } else {
#pragma unroll
                        for (int qi = 0; qi < QW; ++qi)
                            bt.q[u4 * QW + qi][rt][n] =
                                __builtin_nontemporal_load(
                                    reinterpret_cast<const u32x4*>(
                                        qp[rt][n]) + u4 * 64 * QW + qi);
                        bt.ab[u4][rt][n] = __builtin_nontemporal_load(
                            reinterpret_cast<const u32x4*>(abp[rt][n]) +
                            u4 * 16 * ABW);
                    }
                }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int n = 0; n < NM; ++n) {
                if (WT == W_F16) {
                    tp[rt][n] += PF * 512;
                } else {
                    qp[rt][n] += PF * 64 * QW;
                    abp[rt][n] += PF * 16 * ABW;
                }
            }
    };

    auto load_x = [&](XPanel& px) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
                px.xb[u][jt] = *reinterpret_cast<const uint4*>(
                    xp + ((size_t)u * 4 * jtw + jt) * 128);  // 4 kc per kb
            if (NORM)
                px.nbv[u] = *reinterpret_cast<const uint4*>(np + u * 32);
        }
        xp += (size_t)PF * 4 * jtw * 128;
        if (NORM) np += PF * 32;
    };

    auto compute_one = [&](int parity, const uint32_t q[RT][NM][QW],
                           const uint32_t ab[RT][NM],
                           const uint4 aw[RT][NM], const uint4 xb[JT],
                           const uint4& nbv) {
        ABFrag b[JT];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            if (NORM) {
                const uint32_t xw[4] = {xb[jt].x, xb[jt].y, xb[jt].z,
                                        xb[jt].w};
                const uint32_t nw[4] = {nbv.x, nbv.y, nbv.z, nbv.w};
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const __half2 v = __hmul2(u2h2(xw[w]), u2h2(nw[w]));
                    b[jt].u[w] = h22u(__hmul2(v, scale2[jt]));
                }
            } else {
                b[jt].u[0] = xb[jt].x;
                b[jt].u[1] = xb[jt].y;
                b[jt].u[2] = xb[jt].z;
                b[jt].u[3] = xb[jt].w;
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int n = 0; n < NM; ++n) {
                ABFrag a;
                if (WT == W_F16) {
                    a.u[0] = aw[rt][n].x; a.u[1] = aw[rt][n].y;
                    a.u[2] = aw[rt][n].z; a.u[3] = aw[rt][n].w;
                } else if (WT == W_Q8B || WT == W_Q8B16) {
                    a_frag_q8(q[rt][n][0], q[rt][n][QW - 1], ab[rt][n],
                              a);
                } else {
                    a_frag_q4<WT>(q[rt][n][0], ab[rt][n], a);
                }
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) {
                    f32x4& c = (NP == 2 && parity) ? c1[rt][n][jt]
                                                   : c0[rt][n][jt];
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v, b[jt].v,
                                                               c, 0, 0, 0);
                }
            }
    };

    auto compute_batch = [&](Batch& bt, XPanel& px) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            uint32_t q[RT][NM][QW], ab[RT][NM];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int n = 0; n < NM; ++n) {
                    if (WT == W_Q8B || WT == W_Q8B16) {
                        // lane's 8 u32 per group: [blk0.A, blk0.B, ...]
                        q[rt][n][0] = bt.q[u / 2][rt][n][(u % 2) * 2];
                        q[rt][n][QW - 1] =
                            bt.q[u / 2][rt][n][(u % 2) * 2 + 1];
                    } else {
                        q[rt][n][0] = bt.q[u / 4][rt][n][u % 4];
                    }
                    ab[rt][n] = bt.ab[u / 4][rt][n][u % 4];
                }
            compute_one(u & 1, q, ab, bt.aw[u], px.xb[u], px.nbv[u]);
        }
    };

    // Per iteration: [load B-panel (L2) -> prefetch next weights (HBM) ->
    // compute]. The B-panel loads retire first (vmcnt is in-order and they
    // are issued before the HBM batch), so compute's wait never drains the
    // prefetch; one live XPanel keeps register pressure down (a fully
    // double-buffered B panel measured 9% SLOWER end to end).
    const int nfull = (kl.kb1 - kl.kb0) / PF;
    if (nfull > 0) {
        load_w(bufA);
        int it = 0;
        while (true) {
            XPanel pxA;
            load_x(pxA);
            load_w(bufB);        // prefetch next weights (may overread 1)
            compute_batch(bufA, pxA);
            if (++it == nfull) break;
            XPanel pxB;
            load_x(pxB);
            load_w(bufA);
            compute_batch(bufB, pxB);
            if (++it == nfull) break;
        }
        // load_w ran nfull+1 times (the trailing prefetch) but only
        // nfull batches were consumed — rewind one batch so the tail
        // loop reads the right K-blocks. (Latent until the large-M
        // kernels: 4-aligned q4 ranges never leave a tail, and the f16
        // slab kernels' per-wave ranges are < PF so nfull == 0.)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int n = 0; n < NM; ++n) {
                if (WT == W_F16) {
                    tp[rt][n] -= PF * 512;
                } else {
                    qp[rt][n] -= PF * 64 * QW;
                    abp[rt][n] -= PF * 16 * ABW;
                }
            }
    }
    for (int g = kl.kb0 + nfull * PF; g < kl.kb1; ++g) {
        uint32_t q[RT][NM][QW], ab[RT][NM];
        uint4 aw[RT][NM];
        uint4 xb[JT], nbv;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
            xb[jt] = *reinterpret_cast<const uint4*>(xp + jt * 128);
        xp += (size_t)4 * jtw * 128;
        if (NORM) {
            nbv = *reinterpret_cast<const uint4*>(np);
            np += 32;
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int n = 0; n < NM; ++n) {
                if (WT == W_F16) {
                    aw[rt][n] = *reinterpret_cast<const uint4*>(tp[rt][n]);
                    tp[rt][n] += 512;
                } else {
#pragma unroll
                    for (int qi = 0; qi < QW; ++qi)
                        q[rt][n][qi] =
                            __builtin_nontemporal_load(qp[rt][n] + qi);
                    qp[rt][n] += 64 * QW;
                    ab[rt][n] = __builtin_nontemporal_load(abp[rt][n]);
                    abp[rt][n] += 16;
                }
            }
        compute_one(g & 1, q, ab, aw, xb, nbv);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int n = 0; n < NM; ++n)
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    acc[rt][n][jt][jj] =
                        (NP == 2) ? c0[rt][n][jt][jj] + c1[rt][n][jt][jj]
                                  : c0[rt][n][jt][jj];
}

// LDS combine of the NW waves' partial accumulators; wave 0 ends with
// the full 16x16 tile (4 rows x 1 col per lane). NACC = accumulator sets.
template <int NACC, int NW = NWAVES>
__device__ __forceinline__ void combine_acc(float acc[NACC][4],
                                            float* lds /* (NW-1)*64*4*NACC */) {
    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    if (wid > 0) {
        float* dst = lds + (((wid - 1) * 64 + lane) * 4) * NACC;
#pragma unroll
        for (int n = 0; n < NACC; ++n)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) dst[n * 4 + jj] = acc[n][jj];
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
        for (int w = 0; w < NW - 1; ++w) {
            const float* src = lds + ((w * 64 + lane) * 4) * NACC;
#pragma unroll
            for (int n = 0; n < NACC; ++n)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[n][jj] += src[n * 4 + jj];
        }
    }
}

// ---------------------------------------------------------- tile epilogues
// Wave 0 holds the finished tile: lane (j = l&15, l>>4) owns the 4
// consecutive rows [r0, r0+4), r0 = tile*16 + (l>>4)*4, of token column
// t (j2 in the kernels: jt*16 + j in k_gemm16, (mtile*JT + jt)*16 + j in
// k_gemm16_mt and in k_qkv16 / k_ffn16, whose decode half has mtile = 0).
//
// The epilogues share rope_rotate and slab_tile_store, but the q/k/v,
// residual+sumsq+xprep and SwiGLU->gprep bodies stay written out in each
// kernel, and they spell the side-channel index out as
//   (((size_t)(r0 >> 3) * jtw + tile) * 16 + j) * 8 + (r0 & 7)
// (== xprep_index(r0, j2, jtw), tile = j2 >> 4) instead of calling it.
// This is deliberate: hipcc runs its early scalar passes on a kernel
// BEFORE always-inline helpers are expanded, and moving these bodies or
// that arithmetic behind a call changed register allocation and the
// schedule INSIDE wave_tile_kloop (the large-M k_ffn16 went from 92 to 120
// VGPRs, occupancy 4 -> 3). Re-check the K loop's assembly before factoring
// them.

// Split-K partial store: the lane's 4 rows of one token column into its
// slot of a slab tile (f32[64 tok][16 rows]: dst = tile + tok*16 +
// (lane>>4)*4), write-through. No T bound: the slab holds all 64 columns
// and the reducers read only t < T.
__device__ __forceinline__ void slab_tile_store(float* dst,
                                                const float v[4]) {
    store_f4_wt(dst, make_float4(v[0], v[1], v[2], v[3]));
}

// ------------------------------------------------------------- k_prep_x
// sumsq + f16 xprep of an incoming f32 activation block (forward entry,
// split-K gemm epilogue, logits entry). Grid: (T, C) — C column chunks per
// row so the launch fills more than T CUs; ss[t] accumulates via atomics
// and MUST be zeroed before the launch (a T-block single-chunk version
// measured 4.6 µs — launch+latency bound on 16 CUs of 256).
__global__ void k_prep_x(const float* __restrict__ x,
                         unsigned short* __restrict__ xprep,
                         float* __restrict__ ss, int cols, int jtw) {
    const int t = blockIdx.x;
    const float* xt = x + (size_t)t * cols;
    __shared__ float red[NWAVES];
    const int nkc = cols >> 3;
    const int per = (nkc + gridDim.y - 1) / gridDim.y;
    const int kc0 = blockIdx.y * per;
    const int kc1 = min(nkc, kc0 + per);
    float sum = 0.0f;
    for (int kc = kc0 + threadIdx.x; kc < kc1; kc += BLOCK) {
        const float4 a = *reinterpret_cast<const float4*>(xt + kc * 8);
        const float4 b = *reinterpret_cast<const float4*>(xt + kc * 8 + 4);
        sum += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
        sum += b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
        uint4 o;
        o.x = pack_f16(a.x, a.y);
        o.y = pack_f16(a.z, a.w);
        o.z = pack_f16(b.x, b.y);
        o.w = pack_f16(b.z, b.w);
        // xprep_index(kc * 8, t, jtw), spelled out (see the epilogue note)
        *reinterpret_cast<uint4*>(
            xprep + (((size_t)kc * jtw + (t >> 4)) * 16 + (t & 15)) * 8) = o;
    }
    sum = wave_reduce_sum(sum);
    const int wid = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) red[wid] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(ss + t, red[0] + red[1] + red[2] + red[3]);
}

// ------------------------------------------------------- k_reduce_prep
// Split-K reducer + side-channel prep in one pass: y[t] += sum of the KS
// slab partials, then sumsq + f16 xprep of the result (replaces atomic
// split-K partials + a separate k_prep_x — the 819K atomicAdd/kernel of
// the atomic form dominated at JT=4). Grid (T, C); ss zeroed upstream.
__global__ void k_reduce_prep(float* __restrict__ y,
                              const float* __restrict__ slab, int ks,
                              unsigned short* __restrict__ xprep,
                              float* __restrict__ ss, int cols, int jtw) {
    const int t = blockIdx.x;
    float* yt = y + (size_t)t * cols;
    __shared__ float red[NWAVES];
    const int nkc = cols >> 3;
    const int per = (nkc + gridDim.y - 1) / gridDim.y;
    const int kc0 = blockIdx.y * per;
    const int kc1 = min(nkc, kc0 + per);
    float sum = 0.0f;
    for (int kc = kc0 + threadIdx.x; kc < kc1; kc += BLOCK) {
        float4 a = *reinterpret_cast<const float4*>(yt + kc * 8);
        float4 b = *reinterpret_cast<const float4*>(yt + kc * 8 + 4);
        const int e0 = kc * 8;            // 8 consecutive rows
        const int tile = e0 >> 4;         // 16-row tile
        const int i0 = e0 & 15;           // 0 or 8 within the tile
        const float* sbase =
            slab + ((size_t)tile * ks * 64 + t) * 16 + i0;
        const size_t kstride = (size_t)64 * 16;
        for (int k = 0; k < ks; ++k) {
            const float4 p0 = *reinterpret_cast<const float4*>(
                sbase + k * kstride);
            const float4 p1 = *reinterpret_cast<const float4*>(
                sbase + k * kstride + 4);
            a.x += p0.x; a.y += p0.y; a.z += p0.z; a.w += p0.w;
            b.x += p1.x; b.y += p1.y; b.z += p1.z; b.w += p1.w;
        }
        *reinterpret_cast<float4*>(yt + kc * 8) = a;
        *reinterpret_cast<float4*>(yt + kc * 8 + 4) = b;
        sum += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
        sum += b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
        uint4 o;
        o.x = pack_f16(a.x, a.y);
        o.y = pack_f16(a.z, a.w);
        o.z = pack_f16(b.x, b.y);
        o.w = pack_f16(b.z, b.w);
        *reinterpret_cast<uint4*>(xprep + xprep_index(kc * 8, t, jtw)) = o;
    }
    sum = wave_reduce_sum(sum);
    const int wid = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) red[wid] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(ss + t, red[0] + red[1] + red[2] + red[3]);
}

// ------------------------------------------------------------- k_gemm16
// One weight matrix against the B panel, JT <= 4 column tiles (T <= 64).
//   GM_SLAB       grid-level split-K for wo / w2, whose rows/16 alone
//                 cannot fill 256 CUs: gridDim.y blocks per row tile each
//                 cover nb/gridDim.y K-blocks and store their partial tile
//                 into a slab; k_reduce_prep sums the slabs into the
//                 residual stream and rebuilds the side channels.
//   GM_RES_SQ     unsplit wo / w2 with the fused residual + sumsq + xprep
//                 epilogue (taken when E/16 is odd, or by DLLM_NO_SPLITK).
//   GM_NORM_PLAIN lm_head: input RMSNorm fused, plain f32 store.
template <int WT, int MODE, int JT, int RT = 1>
__global__ __launch_bounds__(BLOCK) void k_gemm16(
    WMat2 w, const unsigned short* __restrict__ bprep,
    const unsigned short* __restrict__ normprep,
    const float* __restrict__ ss_in, float eps, float* __restrict__ y,
    unsigned short* __restrict__ xprep_out, float* __restrict__ ss_out,
    int T) {
    constexpr bool NORM = (MODE == GM_NORM_PLAIN);
    const int lane = threadIdx.x & (WAVE - 1);
    const int j = lane & 15;
    float acc[RT][1][JT][4];
    const WMat2* ws[1] = {&w};
    const int nbt = w.cols >> 5;
    const int nbk = (WT == W_F16) ? nbt : ((nbt + 3) & ~3);  // padded
    int b0 = 0, b1 = nbk;
    if (MODE == GM_SLAB) {
        // split in 4-aligned units so q4 group loads stay whole
        int per = (nbk + gridDim.y - 1) / gridDim.y;
        per = (per + 3) & ~3;
        b0 = min(nbk, (int)blockIdx.y * per);
        b1 = min(nbk, b0 + per);
    }
    wave_tile_kloop<WT, NORM, 1, JT, RT>(ws, blockIdx.x, bprep, normprep,
                                         ss_in, eps, acc, b0, b1);
    __shared__ float lds[3 * 64 * 4 * JT * RT];
    combine_acc<RT * JT>(reinterpret_cast<float(*)[4]>(acc), lds);
    if (threadIdx.x >= WAVE) return;
    if (MODE == GM_SLAB) {
        // write-through-store the partial tile(s); k_reduce_prep sums the
        // KS slices at the next kernel boundary (no atomics, no
        // pre-zeroing). Slab layout: f32[R][KS][kMaxTok][16 rows]; `y` is
        // reused as the slab base. With RT>1 a block covers RT row tiles
        // sharing its B-panel reads.
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float* slab = y +
                ((size_t)(blockIdx.x * RT + rt) * gridDim.y + blockIdx.y) *
                    64 * 16;
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                const int j2 = jt * 16 + j;
                slab_tile_store(slab + ((size_t)j2 * 16) + (lane >> 4) * 4,
                                acc[rt][0][jt]);
            }
        }
        return;
    }
    // wave-0 fused epilogue: rows r0..r0+3 per row tile, col jt*16+j
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
    const int r0 = (blockIdx.x * RT + rt) * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        const int j2 = jt * 16 + j;
        float sq = 0.0f;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int row = r0 + jj;
            float v = acc[rt][0][jt][jj];
            if (MODE == GM_RES_SQ) {
                if (j2 < T) {
                    v += y[(size_t)j2 * w.rows + row];
                    y[(size_t)j2 * w.rows + row] = v;
                    sq += v * v;
                }
            } else {
                if (j2 < T) y[(size_t)j2 * w.rows + row] = v;
            }
            acc[rt][0][jt][jj] = v;
        }
        if (MODE == GM_RES_SQ && xprep_out != nullptr && j2 < T) {
            // 4 consecutive rows -> one aligned 8 B f16x4 chunk of xprep
            uint2 o;
            o.x = pack_f16(acc[rt][0][jt][0], acc[rt][0][jt][1]);
            o.y = pack_f16(acc[rt][0][jt][2], acc[rt][0][jt][3]);
            *reinterpret_cast<uint2*>(
                xprep_out + (((size_t)(r0 >> 3) * JT + jt) * 16 + j) * 8 +
                (r0 & 7)) = o;
        }
        if (MODE == GM_RES_SQ && ss_out != nullptr) {
            float s2 = sq;
            s2 += __shfl_xor(s2, 16);
            s2 += __shfl_xor(s2, 32);
            if (lane < 16 && j2 < T) atomicAdd(ss_out + j2, s2);
        }
    }
    }
}

// ------------------------------------------------------ slab qkv variant
// For models whose qkv tile count underfills the chip (3B: 600 tiles),
// the fused kernel runs at ~2.3 blocks/CU with the full B panel re-read
// per tile. This variant uses RT=2 row tiles per wave (halves the B-panel
// L2 traffic and B-build VALU) plus grid-level split-K into slabs; the
// finish — k_qkv_finish, or k_attention's fused prologue in decode — sums
// the slabs and runs the rope/cache epilogue. (The same construction for
// the ffn gate measured slower at every split/occupancy combination tried
// and was removed; k_ffn16 stays fused.)

template <int WT, int JT, int RT>
__global__ __launch_bounds__(BLOCK) void k_qkv16_slab(
    WMat2 wq, WMat2 wk, WMat2 wv, const unsigned short* __restrict__ xprep,
    const unsigned short* __restrict__ normprep,
    const float* __restrict__ ss_in, float eps, float* __restrict__ slab,
    int E, int Ekv, int T) {
    const int tq = (E >> 4) / RT;
    const int tk = (Ekv >> 4) / RT;
    const int mat = (blockIdx.x < tq) ? 0
                    : (blockIdx.x < tq + tk) ? 1 : 2;
    const int stile = blockIdx.x - ((mat == 0) ? 0 : (mat == 1) ? tq
                                                                : tq + tk);
    const WMat2& w = (mat == 0) ? wq : (mat == 1) ? wk : wv;
    const int lane = threadIdx.x & (WAVE - 1);
    const int j = lane & 15;
    float acc[RT][1][JT][4];
    const WMat2* ws[1] = {&w};
    const int nbe = (WT == W_F16) ? (E >> 5) : (((E >> 5) + 3) & ~3);
    int per = (nbe + gridDim.y - 1) / gridDim.y;
    per = (per + 3) & ~3;
    const int b0 = min(nbe, (int)blockIdx.y * per);
    const int b1 = min(nbe, b0 + per);
    wave_tile_kloop<WT, true, 1, JT, RT>(ws, stile, xprep, normprep, ss_in,
                                         eps, acc, b0, b1);
    __shared__ float lds[3 * 64 * 4 * RT * JT];
    combine_acc<RT * JT>(reinterpret_cast<float(*)[4]>(acc), lds);
    if (threadIdx.x >= WAVE) return;
    // slab gtile space: q rows [0, E/16) then k, v rows [.., +Ekv/16)
    const int gbase = (mat == 0) ? 0
                      : (mat == 1) ? (E >> 4)
                                   : (E >> 4) + (Ekv >> 4);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const size_t gtile = (size_t)gbase + stile * RT + rt;
        float* sl = slab + ((gtile * gridDim.y + blockIdx.y) * 64) * 16;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const int j2 = jt * 16 + j;
            slab_tile_store(sl + (size_t)j2 * 16 + (lane >> 4) * 4,
                            acc[rt][0][jt]);
        }
    }
}

// Sum the qkv slabs, apply RoPE, write q_buf / KV caches. One thread per
// (mat, 8-row chunk, token): vectorized float4 slab reads and uint4/f16x8
// stores (scalar 2-4 B accesses made the first version a 5 us kernel).
__global__ void k_qkv_finish(const float* __restrict__ slab, int ks,
                             float* __restrict__ q_buf,
                             __half* __restrict__ k_cache,
                             __half* __restrict__ v_cache,
                             const int* __restrict__ pos,
                             const int* __restrict__ seq,
                             const float* __restrict__ inv_freq, int E,
                             int Ekv, int D, int n_ctx, int T) {
    const int nchunks = (E + 2 * Ekv) / 8;
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= nchunks * T) return;
    const int chunk = idx % nchunks;
    const int t = idx / nchunks;
    const int r = 8 * chunk;  // global row in the [E | Ekv | Ekv] space
    const int mat = (r < E) ? 0 : (r < E + Ekv) ? 1 : 2;
    const int e = (mat == 0) ? r : (mat == 1) ? r - E : r - E - Ekv;
    const size_t gt0 = ((size_t)(r >> 4)) * ks;  // 8-aligned within mat
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
    for (int k = 0; k < ks; ++k) {
        const float* sl = slab + ((gt0 + k) * 64 + t) * 16 + (e & 15);
        const float4 a = *reinterpret_cast<const float4*>(sl);
        const float4 b = *reinterpret_cast<const float4*>(sl + 4);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
        v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
    }
    const int p = pos[t];
    if (mat == 2) {
        __half* dst = v_cache + ((size_t)seq[t] * n_ctx + p) * Ekv + e;
        uint4 o;
        o.x = pack_f16(v[0], v[1]);
        o.y = pack_f16(v[2], v[3]);
        o.z = pack_f16(v[4], v[5]);
        o.w = pack_f16(v[6], v[7]);
        *reinterpret_cast<uint4*>(dst) = o;
        return;
    }
    float o[8];
#pragma unroll
    for (int q2 = 0; q2 < 4; ++q2) {
        const int d = (e + 2 * q2) % D;
        const float theta = (float)p * inv_freq[d >> 1];
        float sn, cs;
        __sincosf(theta, &sn, &cs);
        rope_rotate(v[2 * q2], v[2 * q2 + 1], sn, cs, o[2 * q2],
                    o[2 * q2 + 1]);
    }
    if (mat == 0) {
        float* dst = q_buf + (size_t)t * E + e;
        *reinterpret_cast<float4*>(dst) =
            make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(dst + 4) =
            make_float4(o[4], o[5], o[6], o[7]);
    } else {
        __half* dst = k_cache + ((size_t)seq[t] * n_ctx + p) * Ekv + e;
        uint4 w;
        w.x = pack_f16(o[0], o[1]);
        w.y = pack_f16(o[2], o[3]);
        w.z = pack_f16(o[4], o[5]);
        w.w = pack_f16(o[6], o[7]);
        *reinterpret_cast<uint4*>(dst) = w;
    }
}

// ================================================== prefill (large-M) path
// Hand-written large-M dequant-GEMM: retires the rocBLAS-over-detiled-f16
// prefill path (q4/byte/f16 tiles read DIRECTLY, no f16 weight copy) and
// the 64-token host tiling. One launch covers all T tokens: the grid is
// (gtile row-tiles) x (MT 64-token groups), flattened with an XCD-aware
// decode so all MT token-groups of one row tile land on the SAME XCD
// back-to-back — the row tile's weight stream is read from HBM once and
// re-served to the other groups from that XCD's L2 (blockIdx -> XCD is
// round-robin on dispatch order, 8 XCDs).
//
// Returns (gtile, mtile); gtile may be past the last row tile (pad block
// -> caller exits).
__device__ __forceinline__ void xcd_decode(int MT, int& gtile, int& mtile) {
    const int xcd = blockIdx.x & 7;
    const int q = blockIdx.x >> 3;
    mtile = q % MT;
    gtile = (q / MT) * 8 + xcd;
}

static inline int xcd_grid(int GT, int MT) {
    return ((GT + 7) & ~7) * MT;
}

// -------------------------------------------------- k_qkv16 and k_ffn16
// One template serves decode and large-M; MTK picks how a block finds its
// (row tile, token tile):
//   MTK = false  decode, T <= 64: block = row tile, one token panel of JT
//                tiles (mtile = 0, jtw = JT); launched with MT = jtw_rt = 0.
//   MTK = true   large-M, T > 64: xcd_decode over (row tiles) x (MT 64-token
//                groups), panel stride jtw = jtw_rt = jt_width(T); JT = 4.
// Everything after that is one body with the tokens indexed globally.
// Written so that both halves compile to the code of the two separate
// kernels each used to be — keep the expressions as they stand (a
// `jt0 = mtile * JT` temporary already costs the large-M ffn kernels 4
// instructions and up to 4 VGPRs; see tools/kernel_isa_diff.py).

// QKV projections on MFMA + fused input RMSNorm + RoPE + KV append.
// GQA: wk/wv have Ekv = Hkv*D rows (< E); KV cache rows are Ekv wide.
// Tile space is [0, E/16) for wq then [.., +Ekv/16) each for wk/wv.
// RT row tiles per wave share the B panel (its load + norm-build cost).
template <int WT, int JT, int RT = 1, bool MTK = false>
__global__ __launch_bounds__(BLOCK) void k_qkv16(
    WMat2 wq, WMat2 wk, WMat2 wv, const unsigned short* __restrict__ xprep,
    const unsigned short* __restrict__ normprep,
    const float* __restrict__ ss_in, float eps, float* __restrict__ q_buf,
    __half* __restrict__ k_cache, __half* __restrict__ v_cache,
    const int* __restrict__ pos, const int* __restrict__ seq,
    const float* __restrict__ inv_freq, int E, int Ekv, int D, int n_ctx,
    int T, int MT, int jtw_rt) {
    int gtile, mtile, jtw;
    const int tq = (E >> 4) / RT;
    const int tk = (Ekv >> 4) / RT;
    if (MTK) {
        const int GT = tq + 2 * tk;
        xcd_decode(MT, gtile, mtile);
        if (gtile >= GT) return;
        jtw = jtw_rt;
    } else {
        gtile = blockIdx.x;
        mtile = 0;
        jtw = JT;
    }
    // the decode half compares the block index unsigned, as blockIdx.x is
    using TileIdx = typename std::conditional<MTK, int, unsigned>::type;
    const TileIdx gt = gtile;
    const int mat = (gt < tq) ? 0 : (gt < tq + tk) ? 1 : 2;
    const int tile = gt - ((mat == 0) ? 0 : (mat == 1) ? tq : tq + tk);
    const WMat2& w = (mat == 0) ? wq : (mat == 1) ? wk : wv;
    const int lane = threadIdx.x & (WAVE - 1);
    const int j = lane & 15;
    float acc[RT][1][JT][4];
    const WMat2* ws[1] = {&w};
    const int nbe = (WT == W_F16) ? (E >> 5) : (((E >> 5) + 3) & ~3);
    wave_tile_kloop<WT, true, 1, JT, RT>(ws, tile, xprep, normprep, ss_in,
                                         eps, acc, 0, nbe, jtw,
                                         mtile * JT);
    __shared__ float lds[3 * 64 * 4 * JT * RT];
    combine_acc<RT * JT>(reinterpret_cast<float(*)[4]>(acc), lds);
    if (threadIdx.x >= WAVE) return;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
    const int r0 = (tile * RT + rt) * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        const int j2 = (mtile * JT + jt) * 16 + j;
        if (j2 >= T) continue;
        const int p = pos[j2];
        if (mat == 2) {  // V rows: straight f16 cache append
            __half* dst =
                v_cache + ((size_t)seq[j2] * n_ctx + p) * Ekv + r0;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                dst[jj] = __float2half(acc[rt][0][jt][jj]);
            continue;
        }
        // q/k: RoPE on in-lane pairs (rows r0+2q2, r0+2q2+1)
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
            const int e = r0 + 2 * q2;
            const int d = e % D;
            const float theta = (float)p * inv_freq[d >> 1];
            float sn, cs;
            __sincosf(theta, &sn, &cs);
            float o0, o1;
            rope_rotate(acc[rt][0][jt][2 * q2], acc[rt][0][jt][2 * q2 + 1],
                        sn, cs, o0, o1);
            if (mat == 0) {
                q_buf[(size_t)j2 * E + e] = o0;
                q_buf[(size_t)j2 * E + e + 1] = o1;
            } else {
                __half* dst =
                    k_cache + ((size_t)seq[j2] * n_ctx + p) * Ekv + e;
                dst[0] = __float2half(o0);
                dst[1] = __float2half(o1);
            }
        }
    }
    }
}

// Large-M GEMM with the fused residual + sumsq + xprep epilogue of
// k_gemm16<GM_RES_SQ> (wo / w2).
// Not folded into k_gemm16 the way k_qkv16 / k_ffn16 are: giving the decode
// modes this epilogue moved all 75 decode kernels (lm_head JT=4 RT=4: 2392
// -> 2209 instructions, 220 -> 192 VGPRs; GM_RES_SQ JT=4: 1020 -> 829).
template <int WT, int JT = 4, int RT = 1>
__global__ __launch_bounds__(BLOCK) void k_gemm16_mt(
    WMat2 w, const unsigned short* __restrict__ bprep,
    float* __restrict__ y, unsigned short* __restrict__ xprep_out,
    float* __restrict__ ss_out, int T, int MT, int jtw) {
    int gtile, mtile;
    const int GT = (w.rows >> 4) / RT;
    xcd_decode(MT, gtile, mtile);
    if (gtile >= GT) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int j = lane & 15;
    float acc[RT][1][JT][4];
    const WMat2* ws[1] = {&w};
    const int nbt = w.cols >> 5;
    const int nbk = (WT == W_F16) ? nbt : ((nbt + 3) & ~3);
    wave_tile_kloop<WT, false, 1, JT, RT>(ws, gtile, bprep, nullptr,
                                          nullptr, 0.f, acc, 0, nbk, jtw,
                                          mtile * JT);
    __shared__ float lds[3 * 64 * 4 * JT * RT];
    combine_acc<RT * JT>(reinterpret_cast<float(*)[4]>(acc), lds);
    if (threadIdx.x >= WAVE) return;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
    const int r0 = (gtile * RT + rt) * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        const int j2 = (mtile * JT + jt) * 16 + j;
        if (j2 >= T) continue;
        float sq = 0.0f;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            float v = acc[rt][0][jt][jj];
            v += y[(size_t)j2 * w.rows + r0 + jj];
            sq += v * v;
            y[(size_t)j2 * w.rows + r0 + jj] = v;
            acc[rt][0][jt][jj] = v;
        }
        if (xprep_out != nullptr) {
            uint2 o;
            o.x = pack_f16(acc[rt][0][jt][0], acc[rt][0][jt][1]);
            o.y = pack_f16(acc[rt][0][jt][2], acc[rt][0][jt][3]);
            *reinterpret_cast<uint2*>(
                xprep_out +
                (((size_t)(r0 >> 3) * jtw + mtile * JT + jt) * 16 + j) * 8 +
                (r0 & 7)) = o;
        }
        if (ss_out != nullptr) {
            float s2 = sq;
            s2 += __shfl_xor(s2, 16);
            s2 += __shfl_xor(s2, 32);
            if (lane < 16) atomicAdd(ss_out + j2, s2);
        }
    }
    }
}

// w1 + w3 against the same B panel + fused input RMSNorm + SwiGLU; emits
// the gate product straight into gprep (f16 B-layout over F).
template <int WT, int JT, int RT = 1, bool MTK = false>
__global__ __launch_bounds__(BLOCK) void k_ffn16(
    WMat2 w1, WMat2 w3, const unsigned short* __restrict__ xprep,
    const unsigned short* __restrict__ normprep,
    const float* __restrict__ ss_in, float eps,
    unsigned short* __restrict__ gprep, int T, int MT, int jtw_rt) {
    int gtile, mtile, jtw;
    if (MTK) {
        const int GT = (w1.rows >> 4) / RT;
        xcd_decode(MT, gtile, mtile);
        if (gtile >= GT) return;
        jtw = jtw_rt;
    } else {
        gtile = blockIdx.x;
        mtile = 0;
        jtw = JT;
    }
    const int lane = threadIdx.x & (WAVE - 1);
    const int j = lane & 15;
    float acc[RT][2][JT][4];
    const WMat2* ws[2] = {&w1, &w3};
    const int nbf = (WT == W_F16) ? (w1.cols >> 5)
                                  : (((w1.cols >> 5) + 3) & ~3);
    wave_tile_kloop<WT, true, 2, JT, RT>(ws, gtile, xprep, normprep, ss_in,
                                         eps, acc, 0, nbf, jtw,
                                         mtile * JT);
    __shared__ float lds[3 * 64 * 4 * 2 * JT * RT];
    combine_acc<RT * 2 * JT>(reinterpret_cast<float(*)[4]>(acc), lds);
    if (threadIdx.x >= WAVE) return;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
    const int r0 = (gtile * RT + rt) * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        const int j2 = (mtile * JT + jt) * 16 + j;
        if (j2 >= T) continue;
        float g[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const float v1 = acc[rt][0][jt][jj];
            const float silu = v1 / (1.0f + __expf(-v1));
            g[jj] = silu * acc[rt][1][jt][jj];
        }
        uint2 o;
        o.x = pack_f16(g[0], g[1]);
        o.y = pack_f16(g[2], g[3]);
        *reinterpret_cast<uint2*>(
            gprep + (((size_t)(r0 >> 3) * jtw + mtile * JT + jt) * 16 + j)
                        * 8 + (r0 & 7)) = o;
    }
    }
}

// ------------------------------------------------------- k_lmhead_score
// Large-M lm_head for prompt scoring: k_gemm16_mt's grid, the fused final
// RMSNorm of k_gemm16<GM_NORM_PLAIN>, and an epilogue that stores NO
// logits. A block owns 16*RT vocabulary rows x 64 tokens; per token column
// wave 0 reduces its rows (4 lanes x 4 jj x RT) to one log-sum-exp partial
//   pkey[t][gtile] = largest logprobs_key (tile max and its arg-max, ties
//                    to the smaller index),
//   psum[t][gtile] = sum exp(v - tile max),
// and the one lane that holds row targets[t] stores that logit to
// tgt_logit[t] (one writer per token). k_score_finish (logprobs.hip) merges
// the P = V / (16*RT) partials of a token. Fixed reduction shape, no
// atomics: the result depends on the inputs alone.
template <int WT, int RT>
__global__ __launch_bounds__(BLOCK) void k_lmhead_score(
    WMat2 w, const unsigned short* __restrict__ bprep,
    const unsigned short* __restrict__ normprep,
    const float* __restrict__ ss_in, float eps,
    const int* __restrict__ targets, unsigned long long* __restrict__ pkey,
    float* __restrict__ psum, float* __restrict__ tgt_logit, int T, int MT,
    int jtw) {
    constexpr int JT = 4;
    int gtile, mtile;
    const int GT = (w.rows >> 4) / RT;
    xcd_decode(MT, gtile, mtile);
    if (gtile >= GT) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int j = lane & 15;
    float acc[RT][1][JT][4];
    const WMat2* ws[1] = {&w};
    const int nbt = w.cols >> 5;
    const int nbk = (WT == W_F16) ? nbt : ((nbt + 3) & ~3);
    wave_tile_kloop<WT, true, 1, JT, RT>(ws, gtile, bprep, normprep, ss_in,
                                         eps, acc, 0, nbk, jtw, mtile * JT);
    __shared__ float lds[3 * 64 * 4 * JT * RT];
    combine_acc<RT * JT>(reinterpret_cast<float(*)[4]>(acc), lds);
    if (threadIdx.x >= WAVE) return;
    // first of this lane's rows in row tile 0 of the block
    const int rbase = gtile * RT * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        const int j2 = (mtile * JT + jt) * 16 + j;
        // every lane runs the reductions (dead columns hold finite
        // garbage); only the stores are bounded by T
        unsigned long long best = 0;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const unsigned long long k = logprobs_key(
                    acc[rt][0][jt][jj], rbase + rt * 16 + jj);
                best = k > best ? k : best;
            }
        {
            unsigned long long o = __shfl_xor(best, 16);
            best = o > best ? o : best;
            o = __shfl_xor(best, 32);
            best = o > best ? o : best;
        }
        const float m = logprobs_key_value(best);
        float sum = 0.0f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                sum += expf(acc[rt][0][jt][jj] - m);
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        if (!(m > -INFINITY)) sum = 0.0f;  // all -inf tile: no mass
        if (j2 >= T) continue;
        // target logit: rel = target row relative to this lane's first row
        const int rel = targets[j2] - rbase;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (rel == rt * 16 + jj) tgt_logit[j2] = acc[rt][0][jt][jj];
        if (lane < 16) {
            pkey[(size_t)j2 * GT + gtile] = best;
            psum[(size_t)j2 * GT + gtile] = sum;
        }
    }
}

// ============================================================== launchers

// column-tile count for a token batch T (1, 2 or 4 tiles of 16)
static inline int pick_jt(int T) {
    if (T <= 16) return 1;
    if (T <= 32) return 2;
    return 4;
}

// xprep token-panel width in 16-token tiles: the decode path packs up to
// 4 tiles; the prefill path packs ceil(T/16) padded to whole 4-tile
// groups (JT=4 kernels read whole groups; pad tiles are dead columns)
int jt_width(int T) {
    if (T <= 64) return pick_jt(T);
    return (((T + 15) >> 4) + 3) & ~3;
}

// ------------------------------------------------- MFMA-path launchers

// (T, chunks) grid of k_prep_x / k_reduce_prep: chunk columns so the
// launch spreads over ~256 CUs even at T=16 (a T-block launch measured
// 4.6 us on 16 CUs). ~128 blocks total: a microbenchmark of this kernel
// shape (see profiles/microbench_small_kernel.hip) shows larger grids
// LOSE — launch/ramp overhead outweighs the parallelism for ~1 MB of work
static inline dim3 prep_grid(int cols, int T) {
    const int want = (128 + T - 1) / max(T, 1);
    return dim3(T, max(1, min(want, (cols >> 3) / 64)));
}

// jtw: jt_width(T) for the layer path and the lm_head, score_jt_width(T)
// for prompt scoring; ss zeroed upstream
void launch_prep_x(hipStream_t s, const float* x, unsigned short* xprep,
                   float* ss, int cols, int T, int jtw) {
    hipLaunchKernelGGL(k_prep_x, prep_grid(cols, T), dim3(BLOCK), 0, s, x,
                       xprep, ss, cols, jtw);
}

#define DISPATCH_JT(JTV, ...)            \
    switch (JTV) {                       \
        case 1: {                        \
            constexpr int JTc = 1;       \
            __VA_ARGS__;                 \
            break;                       \
        }                                \
        case 2: {                        \
            constexpr int JTc = 2;       \
            __VA_ARGS__;                 \
            break;                       \
        }                                \
        default: {                       \
            constexpr int JTc = 4;       \
            __VA_ARGS__;                 \
            break;                       \
        }                                \
    }

#define DISPATCH_WT2(WTV, ...)                   \
    switch (WTV) {                               \
        case W_Q4_0: {                           \
            constexpr int WTc = W_Q4_0;          \
            __VA_ARGS__;                         \
            break;                               \
        }                                        \
        case W_Q4_1: {                           \
            constexpr int WTc = W_Q4_1;          \
            __VA_ARGS__;                         \
            break;                               \
        }                                        \
        case W_Q8B: {                            \
            constexpr int WTc = W_Q8B;           \
            __VA_ARGS__;                         \
            break;                               \
        }                                        \
        case W_Q8B16: {                          \
            constexpr int WTc = W_Q8B16;         \
            __VA_ARGS__;                         \
            break;                               \
        }                                        \
        default: {                               \
            constexpr int WTc = W_F16;           \
            __VA_ARGS__;                         \
            break;                               \
        }                                        \
    }

// Row tiles per wave: RT2 instantiates {1, 2}, RT4 {1, 2, 4} (lm_head and
// scoring only). Each case is a set of kernels — add none without a route
// selector that returns it.
#define DISPATCH_RT2(RTV, ...)       \
    if ((RTV) == 2) {                \
        constexpr int RTc = 2;       \
        __VA_ARGS__;                 \
    } else {                         \
        constexpr int RTc = 1;       \
        __VA_ARGS__;                 \
    }

#define DISPATCH_RT4(RTV, ...)       \
    if ((RTV) == 4) {                \
        constexpr int RTc = 4;       \
        __VA_ARGS__;                 \
    } else                           \
        DISPATCH_RT2(RTV, __VA_ARGS__)

// RT=2 (two row tiles per wave share one B panel: half the panel re-reads
// and norm-build VALU per MFMA) is taken when the tile count is even and
// the halved grid still fills the chip. MT = 64-token groups per row tile
// (1 in decode).
static inline bool rt2_fills(int tiles, int MT) {
    return tiles % 2 == 0 && (tiles / 2) * MT >= 512;
}

int qkv16_ks(int E, int Ekv) {
    const int tiles3 = (E + 2 * Ekv) >> 4;
    int ks = 1;
    while ((tiles3 / 2) * ks < 512 && ks < 8) ks <<= 1;
    return ks;
}

int gemm16_ks(int rows) {
    const int R = rows / 16;
    int ks = 1;
    while (R * ks < 512 && ks < 8) ks <<= 1;
    // the slab path runs RT=2 (half the blocks) — keep at least ks=2 so
    // big-E models (65B: R=512) still land >=512 blocks
    if (ks < 2) ks = 2;
    return ks;
}

// ------------------------------------------------------ route selectors
// Which instantiation a launcher runs depends on the matrix and token
// counts alone. The rules live here, one plain function each, so the
// launchers and the tests (which export them) read the same decision.

// lm_head (GM_NORM_PLAIN): thousands of row tiles re-read the same B
// panel; RT divides that L2 traffic while the grid still fills
int gemm16_plain_rt(int rows) {
    const int R = rows / 16;
    if (R % 4 == 0 && R / 4 >= 448) return 4;
    if (R % 2 == 0 && R >= 1024) return 2;
    return 1;
}

// ffn gate, decode (T <= 64) and large-M
int ffn16_rt(int rows, int T) {
    const int MT = (T <= 64) ? 1 : (T + 63) >> 6;
    return rt2_fills(rows / 16, MT) ? 2 : 1;
}

// wo / w2 large-M (T > 64)
int gemm16_mt_rt(int rows, int T) {
    return rt2_fills(rows >> 4, (T + 63) >> 6) ? 2 : 1;
}

// wo / w2 (launch_gemm16_residual). The tile count rows/16 alone underfills
// 256 CUs in decode, so: 0 = split K across grid.y into plain-stored slabs
// at RT=2 (needs an even tile count), then one reduce + residual + sumsq +
// xprep pass (no atomics; the kernel boundary provides slab visibility) —
// wins at every model size tested; 1 = unsplit fused GM_RES_SQ; 2 = large-M
// k_gemm16_mt (T > 64), RT from gemm16_mt_rt. split_ok = the caller has a
// slab and did not disable the split.
int gemm16_res_route(int rows, int T, int split_ok) {
    if (T > 64) return 2;
    return (split_ok && (rows / 16) % 2 == 0) ? 0 : 1;
}

// RT=2 needs an even tile count in each of the three matrices
static inline bool qkv_rt2_ok(int E, int Ekv) {
    return ((E >> 4) % 2 == 0) && ((Ekv >> 4) % 2 == 0);
}

// decode qkv (T <= 64): 0 = RT=2 slab split-K when the fused grid would
// underfill the chip, 2 = fused RT=2 (big models: halves the B-panel
// re-read while the halved grid still fills), 1 = fused RT=1
int qkv16_route(int E, int Ekv, int T, int has_slab) {
    (void)T;  // the decode routes do not depend on the token count
    const int tiles3 = (E + 2 * Ekv) >> 4;
    const bool rt2_ok = qkv_rt2_ok(E, Ekv);
    if (has_slab && tiles3 < 1024 && rt2_ok) return 0;
    if (rt2_ok && rt2_fills(tiles3, 1)) return 2;
    return 1;
}

// large-M qkv: RT=2 halves the B-panel reads + norm-build VALU per MFMA
// as long as the halved grid still fills the chip
int qkv16_mt_rt(int E, int Ekv, int T) {
    const int tiles3 = (E + 2 * Ekv) >> 4;
    return (qkv_rt2_ok(E, Ekv) && rt2_fills(tiles3, (T + 63) >> 6)) ? 2 : 1;
}

// ------------------------------------------------------------ launchers
// One per layer op, every T. Each branch below is taken on a selector's
// value; T > 64 (the line gemm16_res_route and jt_width also draw) picks
// between a selector's decode and large-M kernels: large-M covers all T
// tokens in one launch on the XCD-aware (row tile x 64-token group) grid,
// side channels at the jt_width(T) panel stride.

int launch_qkv16(hipStream_t s, const WMat2& wq, const WMat2& wk,
                 const WMat2& wv, const unsigned short* xprep,
                 const unsigned short* normprep, const float* ss_in,
                 float eps, float* q_buf, __half* k_cache_layer,
                 __half* v_cache_layer, const int* pos, const int* seq,
                 const float* inv_freq, int E, int Ekv, int D, int n_ctx,
                 int T, float* slab, int skip_finish) {
    const int tiles3 = (E + 2 * Ekv) >> 4;
    if (T > 64) {
        const int MT = (T + 63) >> 6;
        const int jtw = jt_width(T);
        DISPATCH_RT2(qkv16_mt_rt(E, Ekv, T), DISPATCH_WT2(wq.wtype,
            hipLaunchKernelGGL(
                (k_qkv16<WTc, 4, RTc, true>),
                dim3(xcd_grid(tiles3 / RTc, MT)), dim3(BLOCK), 0, s, wq, wk,
                wv, xprep, normprep, ss_in, eps, q_buf, k_cache_layer,
                v_cache_layer, pos, seq, inv_freq, E, Ekv, D, n_ctx, T, MT,
                jtw)));
        return 0;
    }
    const int route = qkv16_route(E, Ekv, T, slab != nullptr);
    if (route == 0) {  // slab split-K + RT=2
        // RT=2 measured best (RT=4 loses ~3%: fill drops below 2/CU)
        const int ks = qkv16_ks(E, Ekv);
        const dim3 grid(tiles3 / 2, ks);
        DISPATCH_WT2(wq.wtype, DISPATCH_JT(pick_jt(T), hipLaunchKernelGGL(
            (k_qkv16_slab<WTc, JTc, 2>), grid, dim3(BLOCK), 0, s, wq, wk,
            wv, xprep, normprep, ss_in, eps, slab, E, Ekv, T)));
        if (!skip_finish) {
            const int total = ((E + 2 * Ekv) / 8) * T;
            hipLaunchKernelGGL(k_qkv_finish,
                               dim3((total + BLOCK - 1) / BLOCK),
                               dim3(BLOCK), 0, s, slab, ks, q_buf,
                               k_cache_layer, v_cache_layer, pos, seq,
                               inv_freq, E, Ekv, D, n_ctx, T);
        }
        return 1;
    }
    // the fused routes 1 and 2 are named by their RT
    DISPATCH_RT2(route, DISPATCH_WT2(wq.wtype, DISPATCH_JT(pick_jt(T),
        hipLaunchKernelGGL(
            (k_qkv16<WTc, JTc, RTc>), dim3(tiles3 / RTc), dim3(BLOCK), 0, s,
            wq, wk, wv, xprep, normprep, ss_in, eps, q_buf, k_cache_layer,
            v_cache_layer, pos, seq, inv_freq, E, Ekv, D, n_ctx, T, 0, 0))));
    return 0;
}

// ffn stays fused at every T: a slab+finish variant measured slower at
// every split/occupancy combination tried and was removed
void launch_ffn16(hipStream_t s, const WMat2& w1, const WMat2& w3,
                  const unsigned short* xprep,
                  const unsigned short* normprep, const float* ss_in,
                  float eps, unsigned short* gprep, int T) {
    const int tilesF = w1.rows / 16;
    const int rt = ffn16_rt(w1.rows, T);
    if (T > 64) {
        const int MT = (T + 63) >> 6;
        const int jtw = jt_width(T);
        DISPATCH_RT2(rt, DISPATCH_WT2(w1.wtype, hipLaunchKernelGGL(
            (k_ffn16<WTc, 4, RTc, true>), dim3(xcd_grid(tilesF / RTc, MT)),
            dim3(BLOCK), 0, s, w1, w3, xprep, normprep, ss_in, eps, gprep, T,
            MT, jtw)));
        return;
    }
    DISPATCH_RT2(rt, DISPATCH_WT2(w1.wtype, DISPATCH_JT(pick_jt(T),
        hipLaunchKernelGGL(
            (k_ffn16<WTc, JTc, RTc>), dim3(tilesF / RTc), dim3(BLOCK), 0, s,
            w1, w3, xprep, normprep, ss_in, eps, gprep, T, 0, 0))));
}

void launch_gemm16_residual(hipStream_t s, const WMat2& w,
                            const unsigned short* bprep, float* y,
                            unsigned short* xprep_out, float* ss_out, int T,
                            float* slab, int split_ok) {
    const int R = w.rows / 16;
    switch (gemm16_res_route(w.rows, T, split_ok)) {
        case 0: {
            // split K so R*KS lands near 2-3 blocks/CU (256 CUs); RT=2
            // halves the B-panel re-read
            const int ks = gemm16_ks(w.rows);
            DISPATCH_WT2(w.wtype, DISPATCH_JT(pick_jt(T), hipLaunchKernelGGL(
                (k_gemm16<WTc, GM_SLAB, JTc, 2>), dim3(R / 2, ks),
                dim3(BLOCK), 0, s, w, bprep, nullptr, nullptr, 0.f, slab,
                nullptr, nullptr, T)));
            // y[t] += sum of the ks partials, then sumsq + xprep of y
            hipLaunchKernelGGL(k_reduce_prep, prep_grid(w.rows, T),
                               dim3(BLOCK), 0, s, y, slab, ks, xprep_out,
                               ss_out, w.rows, pick_jt(T));
            break;
        }
        case 1:
            DISPATCH_WT2(w.wtype, DISPATCH_JT(pick_jt(T), hipLaunchKernelGGL(
                (k_gemm16<WTc, GM_RES_SQ, JTc, 1>), dim3(R), dim3(BLOCK), 0,
                s, w, bprep, nullptr, nullptr, 0.f, y, xprep_out, ss_out,
                T)));
            break;
        default: {
            const int MT = (T + 63) >> 6;
            const int jtw = jt_width(T);
            DISPATCH_RT2(gemm16_mt_rt(w.rows, T), DISPATCH_WT2(w.wtype,
                hipLaunchKernelGGL(
                    (k_gemm16_mt<WTc, 4, RTc>), dim3(xcd_grid(R / RTc, MT)),
                    dim3(BLOCK), 0, s, w, bprep, y, xprep_out, ss_out, T, MT,
                    jtw)));
        }
    }
}

void launch_lmhead(hipStream_t s, const WMat2& w,
                   const unsigned short* bprep,
                   const unsigned short* normprep, const float* ss_in,
                   float eps, float* y, int T) {
    const int R = w.rows / 16;
    const int rt = gemm16_plain_rt(w.rows);
    DISPATCH_RT4(rt, DISPATCH_WT2(w.wtype, DISPATCH_JT(pick_jt(T),
        hipLaunchKernelGGL(
            (k_gemm16<WTc, GM_NORM_PLAIN, JTc, RTc>), dim3(R / RTc),
            dim3(BLOCK), 0, s, w, bprep, normprep, ss_in, eps, y, nullptr,
            nullptr, T))));
}

// ------------------------------------------------------ prompt scoring
// token-panel stride of the scoring path: whole 4-tile groups at EVERY T
// (k_lmhead_score is JT=4 only, so unlike jt_width it never packs 1 or 2)
int score_jt_width(int T) {
    return (((T + 15) >> 4) + 3) & ~3;
}

// Row tiles per wave of k_lmhead_score: the lm_head rule gemm16_plain_rt
// (RT=4 from 448 blocks, RT=2 from 512) with the block count taken over
// the MT token groups the way rt2_fills does for the other large-M kernels.
int lmhead_score_rt(int V, int T) {
    const int R = V >> 4;
    const int MT = (T + 63) >> 6;
    if (R % 4 == 0 && (R / 4) * MT >= 448) return 4;
    if (rt2_fills(R, MT)) return 2;
    return 1;
}

void launch_lmhead_score(hipStream_t s, const WMat2& w,
                         const unsigned short* bprep,
                         const unsigned short* normprep, const float* ss_in,
                         float eps, const int* targets,
                         unsigned long long* pkey, float* psum,
                         float* tgt_logit, int T) {
    const int MT = (T + 63) >> 6;
    const int jtw = score_jt_width(T);
    const int R = w.rows >> 4;
    const int rt = lmhead_score_rt(w.rows, T);
    DISPATCH_RT4(rt, DISPATCH_WT2(w.wtype, hipLaunchKernelGGL(
        (k_lmhead_score<WTc, RTc>), dim3(xcd_grid(R / RTc, MT)), dim3(BLOCK),
        0, s, w, bprep, normprep, ss_in, eps, targets, pkey, psum, tgt_logit,
        T, MT, jtw)));
}
