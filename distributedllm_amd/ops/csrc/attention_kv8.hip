// Int8 KV cache (kv_dtype = "q8", gfx950): the quantising append
// `k_kv8_append`, the matrix-core attention kernel `k_attn_kv8` over the
// byte caches, its Q-tiled prefill sibling `k_attn_kv8_prefill` and the
// shared-prefix pair `k_attn_kv8_prefix` + `k_attn_kv8_prefix_tail`, with
// their launchers (formats and semantics: kernels.h).
//
// A cache row of one KV head is D bytes u = q + 128, q in [-127, 127], and
// one f16 scale s: x ~ s * q. 0x6400 | u is exactly the f16 value 1024 + u
// (the byte-stream GEMMs' expansion, mfma_gemm.hip), so one v_perm_b32 and
// one packed-f16 add of -1152 turn two bytes into two exact integer-valued
// halves q: no convert instruction, and no value a byte could hold is
// anything but a finite half.
//
// k_attn_kv8 has k_attn_gqa's work split (attention.hip): one block per
// (token, KV head, up to 16 query heads of its group, KV chunk), the group's
// query heads as the 16 MFMA columns, four waves that stream the chunk's
// tiles with two tile buffers and merge once at the end; split partials go
// to k_attn_gqa_merge unchanged. What differs is the data path:
//   * a wave's tile is 32 rows, not 16: a 16-byte load brings 16 elements,
//     so the same number of loads per lane as the f16 kernel (4 K + 4 V at
//     D = 128) keeps the same bytes in flight and covers twice the rows;
//   * scores: lane (row lq, lg) loads the 16 bytes d = c*64 + lg*16 .. + 15
//     of its row for each 64-wide chunk c and feeds them to two
//     mfma_f32_16x16x32_f16 as the k-span lg of each (the contraction index
//     is permuted; the staged Q fragments follow the same permutation). The
//     f32 score is then multiplied by s_k[row] / sqrt(D): the K scale is
//     never applied per element;
//   * PV: one mfma_f32_16x16x32_f16 per 16 d over all 32 rows. The B operand
//     is P~ = p * s_v[row] / R packed to f16, in the score C layout of the
//     tile's two 16-row halves (k-slot e of lane group lg is row
//     (e / 4) * 16 + lg * 4 + e % 4); the A operand is the integer-valued
//     V^T. R is the wave's running maximum of s_v over the attended rows it
//     has seen, carried like the running score maximum: when it rises the
//     accumulators are rescaled by R_old / R_new together with the softmax
//     correction, and the wave's partial is multiplied by R once at the end.
//     So P~ lies in [0, 1] whatever the magnitude of V, and its f16 rounding
//     is that of the f16 p of the other matrix-core kernels (docs/kernels.md,
//     "Int8 KV cache", has the bound);
//   * V transpose for 1-byte elements: lane (quad g = lane / 8, span
//     sp = lane % 8) loads rows g*4 .. g*4+3, bytes sp*16 .. +15, transposes
//     the four 4x4 byte blocks in registers (8 v_perm_b32 each) into one
//     u32 per d that holds the quad's four rows, and writes them as four
//     16-byte LDS stores to vt[g][d]. The consumer lane (lq, lg) of d-chunk
//     dc reads vt[lg][dc*16 + lq] and vt[4 + lg][dc*16 + lq]: its eight
//     k-slots. KV8_VSTRIDE = 144 words puts the lane groups' 16-word reads
//     on disjoint banks (144 mod 64 = 16);
//   * the 32 K scales and 32 V scales of a tile arrive as one 2-byte load
//     per lane and are redistributed through 128 bytes of wave-private LDS.
// Every load is unconditional and every address valid, as in gqa_load_tile:
// rows at or past the chunk end read row 0 and are masked, spans that start
// at or past D read span 0 (K: multiplied by q = 0; V: columns that are
// never stored), a span that straddles D reads into the next head or the
// 16-byte pad. Head starts are multiples of 4 bytes (D % 4 == 0), which is
// all a 16-byte global load needs.
//
// G = H / Hkv = 1 (MHA) runs the same kernel with one live MFMA column: the
// kernel is bound by the byte stream and the expansion of the bytes, both of
// which a VALU dot would pay as well, and one code path serves every G.

#include <algorithm>

#include "attn_common.h"
#include "kernels.h"

typedef __attribute__((ext_vector_type(2))) _Float16 kv8_f16x2;
typedef __attribute__((ext_vector_type(4))) _Float16 kv8_f16x4;
// 16 bytes at 4-byte alignment
typedef uint32_t kv8_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int KV8_MIN_CHUNK = 256;  // rows per split, lower bound (unmeasured)
constexpr int KV8_MAX_SPLITS = 8;   // splits of a full context (unmeasured)
constexpr int KV8_VSTRIDE = 144;    // u32 per row quad of a V tile

int attn_kv8_chunk(int n_ctx) {
    const int per = (n_ctx + KV8_MAX_SPLITS - 1) / KV8_MAX_SPLITS;
    return std::max(KV8_MIN_CHUNK, (per + 63) & ~63);
}

int attn_kv8_splits(int n_ctx, int T) {
    if (T > 64) return 1;  // wide launches fill the chip by themselves
    const int chunk = attn_kv8_chunk(n_ctx);
    return (n_ctx + chunk - 1) / chunk;
}

// ------------------------------------------------------------------ append
// Wave = (token, KV head); lanes 0..31 quantise the K row of the head, lanes
// 32..63 the V row, four elements each (D <= 128). amax is reduced inside
// the half wave, the bytes leave as one 4-byte store per lane.
GQA_FN __global__ __launch_bounds__(BLOCK) void k_kv8_append(
    const __half* __restrict__ k_stage, const __half* __restrict__ v_stage,
    uint8_t* __restrict__ k8, uint8_t* __restrict__ v8,
    __half* __restrict__ k_scale, __half* __restrict__ v_scale,
    const int* __restrict__ pos, const int* __restrict__ seq, int T, int Hkv,
    int D, int n_ctx) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int unit = (int)blockIdx.x * NWAVES + (int)threadIdx.x / WAVE;
    if (unit >= T * Hkv) return;        // wave-uniform
    const int t = unit / Hkv;
    const int hk = unit % Hkv;
    const bool isv = lane >= 32;
    const int d0 = (lane & 31) * 4;
    const bool dok = d0 < D;
    const size_t row = (size_t)seq[t] * n_ctx + pos[t];
    const size_t off = row * ((size_t)Hkv * D) + (size_t)hk * D +
                       (dok ? d0 : 0);  // lanes past D reread the head start
    const uint2 raw =
        *reinterpret_cast<const uint2*>((isv ? v_stage : k_stage) + off);
    const kv8_f16x4 h = __builtin_bit_cast(kv8_f16x4, raw);
    float x[4], amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[i] = dok ? (float)h[i] : 0.0f;
        amax = fmaxf(amax, fabsf(x[i]));
    }
#pragma unroll
    for (int sh = 1; sh <= 16; sh <<= 1)
        amax = fmaxf(amax, gqa_shfl_xor(amax, lane, sh));
    const _Float16 s16 = (_Float16)(amax / 127.0f);
    const float s = (float)s16;
    uint32_t packed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float q = (s > 0.0f) ? __builtin_rintf(x[i] / s) : 0.0f;
        q = fminf(fmaxf(q, -127.0f), 127.0f);
        packed |= (uint32_t)((int)q + 128) << (8 * i);
    }
    if (dok)
        *reinterpret_cast<uint32_t*>((isv ? v8 : k8) + off) = packed;
    if ((lane & 31) == 0)
        reinterpret_cast<unsigned short*>(isv ? v_scale : k_scale)
            [row * Hkv + hk] = __builtin_bit_cast(unsigned short, s16);
}

// --------------------------------------------------------------- attention

// Four bytes of w -> exact integer-valued halves (b0 - 128, b1 - 128) and
// (b2 - 128, b3 - 128): 0x64bb is f16(1024 + b)
GQA_FN __device__ __forceinline__ void kv8_expand4(uint32_t w, uint32_t& lo,
                                                   uint32_t& hi) {
    const kv8_f16x2 c = {(_Float16)-1152.0f, (_Float16)-1152.0f};
    const uint32_t a = __builtin_amdgcn_perm(0x64646464u, w, 0x04010400u);
    const uint32_t b = __builtin_amdgcn_perm(0x64646464u, w, 0x04030402u);
    lo = __builtin_bit_cast(uint32_t, __builtin_bit_cast(kv8_f16x2, a) + c);
    hi = __builtin_bit_cast(uint32_t, __builtin_bit_cast(kv8_f16x2, b) + c);
}

// One 32-row tile of one wave as loaded: K in score-A order (lane: rows lq
// and 16 + lq, 16 bytes of each 64-d chunk), V row-major (lane: rows
// (lane/8)*4 + e, bytes (lane%8)*16 .. +15), and one scale (lanes 0..31 the
// K scale of row lane, lanes 32..63 the V scale of row lane - 32).
template <int NSC>
struct Kv8Tile {
    kv8_u32x4 k[2][NSC];
    kv8_u32x4 v[4];
    unsigned short sc;
};

// gqa_load_tile's rules: straight-line loads with no branch around them,
// every address valid, pinned above the caller's next step.
template <int NSC>
GQA_FN __device__ __forceinline__ void kv8_load_tile(
    Kv8Tile<NSC>& t, const uint8_t* __restrict__ kb,
    const uint8_t* __restrict__ vb, const unsigned short* __restrict__ ksb,
    const unsigned short* __restrict__ vsb, int tj, int jend, int Ekv,
    int Hkv, int D, int lane) {
    const int lq = lane & 15;
    const int lg = lane >> 4;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int jk = tj + r * 16 + lq;
        const uint8_t* krow = kb + (size_t)(jk < jend ? jk : 0) * Ekv;
#pragma unroll
        for (int c = 0; c < NSC; ++c) {
            const int d0 = c * 64 + lg * 16;
            t.k[r][c] = *reinterpret_cast<const kv8_u32x4*>(
                krow + (d0 < D ? d0 : 0));
        }
    }
    const int dv = ((lane & 7) * 16 < D) ? (lane & 7) * 16 : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int jv = tj + (lane >> 3) * 4 + e;
        const uint8_t* vrow = vb + (size_t)(jv < jend ? jv : 0) * Ekv;
        t.v[e] = *reinterpret_cast<const kv8_u32x4*>(vrow + dv);
    }
    const int js = tj + (lane & 31);
    t.sc = (lane < 32 ? ksb : vsb)[(size_t)(js < jend ? js : 0) * Hkv];
    __builtin_amdgcn_sched_barrier(0);
}

// V transpose (file header). The lane holds V[g*4 + e][sp*16 + i], e = 0..3,
// i = 0..15; word w of its four rows is a 4x4 byte block that two rounds of
// v_perm_b32 turn into four words {V[g*4 + 0..3][d]}, d = sp*16 + 4w + 0..3.
GQA_FN __device__ __forceinline__ void kv8_stage_v(
    uint32_t* __restrict__ vt, const kv8_u32x4 v[4], int lane) {
    uint4* dst = reinterpret_cast<uint4*>(
        vt + (lane >> 3) * KV8_VSTRIDE + (lane & 7) * 16);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t t01l = __builtin_amdgcn_perm(v[1][w], v[0][w],
                                                    0x05010400u);
        const uint32_t t01h = __builtin_amdgcn_perm(v[1][w], v[0][w],
                                                    0x07030602u);
        const uint32_t t23l = __builtin_amdgcn_perm(v[3][w], v[2][w],
                                                    0x05010400u);
        const uint32_t t23h = __builtin_amdgcn_perm(v[3][w], v[2][w],
                                                    0x07030602u);
        uint4 o;
        o.x = __builtin_amdgcn_perm(t23l, t01l, 0x05040100u);   // d = 4w
        o.y = __builtin_amdgcn_perm(t23l, t01l, 0x07060302u);
        o.z = __builtin_amdgcn_perm(t23h, t01h, 0x05040100u);
        o.w = __builtin_amdgcn_perm(t23h, t01h, 0x07060302u);
        dst[w] = o;
    }
}

// One 32-row tile of one wave: scores, online softmax on the score C layout
// of the two 16-row halves, V transpose, PV. (m, l) are the running max and
// sum of column lq, R the running maximum of the V scales (wave-uniform).
template <int DC, int NSC>
GQA_FN __device__ __forceinline__ void kv8_tile_step(
    const Kv8Tile<NSC>& tile, const ABFrag (&qf)[2 * NSC], uint32_t* vt,
    _Float16* st, int tj, int ce, int lane, float qk_scale, float& m,
    float& l, float& R, f32x4 (&oacc)[DC]) {
    const int lq = lane & 15;
    const int lg = lane >> 4;
    f32x4 sc[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        sc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NSC; ++c) {
            ABFrag ka, kb;
            kv8_expand4(tile.k[r][c][0], ka.u[0], ka.u[1]);
            kv8_expand4(tile.k[r][c][1], ka.u[2], ka.u[3]);
            kv8_expand4(tile.k[r][c][2], kb.u[0], kb.u[1]);
            kv8_expand4(tile.k[r][c][3], kb.u[2], kb.u[3]);
            sc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                ka.v, qf[2 * c].v, sc[r], 0, 0, 0);
            sc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                kb.v, qf[2 * c + 1].v, sc[r], 0, 0, 0);
        }
    }
    reinterpret_cast<unsigned short*>(st)[lane] = tile.sc;
    kv8_stage_v(vt, tile.v, lane);
    gqa_wave_sync();                        // scales, V tile written -> read

    // lane holds s[j = tj + r*16 + lg*4 + jj][column lq] as slot r*4 + jj
    float s[8], sv[8], tm = -INFINITY, svm = 0.0f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const kv8_f16x4 ks =
            *reinterpret_cast<const kv8_f16x4*>(st + r * 16 + lg * 4);
        const kv8_f16x4 vs =
            *reinterpret_cast<const kv8_f16x4*>(st + 32 + r * 16 + lg * 4);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const bool ok = tj + r * 16 + lg * 4 + jj < ce;
            s[r * 4 + jj] = ok ? sc[r][jj] * ((float)ks[jj] * qk_scale)
                               : -INFINITY;
            sv[r * 4 + jj] = ok ? (float)vs[jj] : 0.0f;
            tm = fmaxf(tm, s[r * 4 + jj]);
            svm = fmaxf(svm, sv[r * 4 + jj]);
        }
    }
    tm = fmaxf(tm, gqa_shfl_xor(tm, lane, 16));
    tm = fmaxf(tm, gqa_shfl_xor(tm, lane, 32));
    svm = fmaxf(svm, gqa_shfl_xor(svm, lane, 16));
    svm = fmaxf(svm, gqa_shfl_xor(svm, lane, 32));
    // finite: the wave's first tile has an attended row. A tile wholly past
    // the chunk (tm = -inf, svm = 0) leaves m, l, R and oacc as they are.
    const float m_new = fmaxf(m, tm);
    const float R_new = fmaxf(R, svm);
    const float inv_r = (R_new > 0.0f) ? __builtin_amdgcn_rcpf(R_new) : 0.0f;
    const float alpha = __expf(m - m_new);  // 0 on the first tile
    // accumulators are in units of R: exactly 1 while R stands
    const float alpha_o = alpha * ((R_new == R) ? 1.0f : R * inv_r);
    float ts = 0.0f, pt[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float p = __expf(s[e] - m_new);   // 0 for masked rows
        ts += p;
        pt[e] = p * (sv[e] * inv_r);            // P~ in [0, 1]
    }
    ABFrag p;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        p.u[i] = gqa_pack_f16(pt[2 * i], pt[2 * i + 1]);
    ts += gqa_shfl_xor(ts, lane, 16);
    ts += gqa_shfl_xor(ts, lane, 32);
    l = l * alpha + ts;
    m = m_new;
    R = R_new;

    // the accumulators leave the MFMA register file only when some column's
    // factor is not 1 (wave-uniform branch; x * 1 is x)
    if (__builtin_amdgcn_ballot_w64(alpha_o != 1.0f) != 0) {
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) {
            oacc[dc][0] *= alpha_o; oacc[dc][1] *= alpha_o;
            oacc[dc][2] *= alpha_o; oacc[dc][3] *= alpha_o;
        }
    }
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
        ABFrag vf;
        kv8_expand4(vt[lg * KV8_VSTRIDE + dc * 16 + lq], vf.u[0], vf.u[1]);
        kv8_expand4(vt[(4 + lg) * KV8_VSTRIDE + dc * 16 + lq], vf.u[2],
                    vf.u[3]);
        oacc[dc] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf.v, p.v,
                                                          oacc[dc], 0, 0, 0);
    }
    gqa_wave_sync();                        // read -> next tile's write
}

// DC = 16-wide d chunks of the PV product, a power of two >= D/16; the score
// product runs NSC = max(1, DC/4) 64-wide chunks of two MFMAs each. Chunks
// past D work on zero q (scores) or produce columns that are never stored.
template <int DC>
GQA_FN __global__ __launch_bounds__(BLOCK) void k_attn_kv8(
    const float* __restrict__ q_buf, const uint8_t* __restrict__ k8,
    const uint8_t* __restrict__ v8, const __half* __restrict__ k_scale,
    const __half* __restrict__ v_scale, float* __restrict__ out,
    unsigned short* __restrict__ out_prep, const int* __restrict__ pos,
    const int* __restrict__ seq, float* __restrict__ ws, int H, int grp,
    int E, int Ekv, int D, int n_ctx, int jtw, int chunk) {
    constexpr int NSC = DC > 4 ? DC / 4 : 1;
    constexpr int QW = NSC * 64;        // staged q row, halves
    const int t = blockIdx.x;
    const int J = pos[t] + 1;
    const int cs = (int)blockIdx.z * chunk;
    if (cs >= J) return;                // block-uniform
    const int ce = min(J, cs + chunk);
    const int ntile = (grp + 15) >> 4;  // column tiles per KV head
    const int hk = (int)blockIdx.y / ntile;
    const int c0 = ((int)blockIdx.y % ntile) * 16;  // first column's head
    const int ncol = min(16, grp - c0);
    const int Hkv = Ekv / D;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);  // scalar
    const int lq = lane & 15;
    const int lg = lane >> 4;
    const size_t row0 = (size_t)seq[t] * n_ctx;
    const uint8_t* kb = k8 + row0 * Ekv + hk * D;
    const uint8_t* vb = v8 + row0 * Ekv + hk * D;
    const unsigned short* ksb =
        reinterpret_cast<const unsigned short*>(k_scale) + row0 * Hkv + hk;
    const unsigned short* vsb =
        reinterpret_cast<const unsigned short*>(v_scale) + row0 * Hkv + hk;

    // One LDS region, used twice: the waves' V tiles and scales and the
    // staged Q while streaming, the waves' O partials [w][col][OSTR] after
    // it (OSTR skews the 16 columns by 4 banks each).
    constexpr int OSTR = DC * 16 + 4;
    constexpr int VT_BYTES = NWAVES * 8 * KV8_VSTRIDE * (int)sizeof(uint32_t);
    constexpr int SC_BYTES = NWAVES * 64 * (int)sizeof(_Float16);
    constexpr int Q_BYTES = 16 * (QW + 8) * (int)sizeof(_Float16);
    constexpr int O_BYTES = NWAVES * 16 * OSTR * (int)sizeof(float);
    constexpr int S_BYTES = VT_BYTES + SC_BYTES + Q_BYTES;
    constexpr int LDS_BYTES = S_BYTES > O_BYTES ? S_BYTES : O_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    __shared__ float lds_m[NWAVES][16];
    __shared__ float lds_l[NWAVES][16];
    uint32_t* vt = reinterpret_cast<uint32_t*>(lds_raw) +
                   wid * 8 * KV8_VSTRIDE;
    _Float16* st = reinterpret_cast<_Float16*>(lds_raw + VT_BYTES) + wid * 64;
    _Float16 (*lds_q)[QW + 8] = reinterpret_cast<_Float16 (*)[QW + 8]>(
        lds_raw + VT_BYTES + SC_BYTES);
    float* lds_o = reinterpret_cast<float*>(lds_raw);

    // Q tile -> LDS as f16, zero past D and past the group's last head (the
    // factor, not a branch, does the masking: the loads stay independent).
    // The ncol heads are contiguous in q_buf. 1/sqrt(D) joins the K scale.
    {
        const float* qt = q_buf + (size_t)t * E + (size_t)(hk * grp + c0) * D;
#pragma unroll
        for (int i = 0; i < 16 * QW / BLOCK; ++i) {
            const int idx = tid + i * BLOCK;
            const int col = idx / QW;
            const int d = idx % QW;
            const bool ok = col < ncol && d < D;
            const float v = qt[ok ? col * D + d : 0] * (ok ? 1.0f : 0.0f);
            lds_q[col][d] = (_Float16)v;
        }
    }
    gqa_block_sync();
    // score-MFMA B fragments: lane (column lq, lg) holds d = c*64 + lg*16 +
    // 0..7 for the first MFMA of chunk c and + 8..15 for the second
    ABFrag qf[2 * NSC];
#pragma unroll
    for (int c = 0; c < 2 * NSC; ++c) {
        const uint4 u = *reinterpret_cast<const uint4*>(
            &lds_q[lq][(c >> 1) * 64 + lg * 16 + (c & 1) * 8]);
        qf[c].u[0] = u.x; qf[c].u[1] = u.y;
        qf[c].u[2] = u.z; qf[c].u[3] = u.w;
    }
    const float qk_scale = rsqrtf((float)D);

    float m = -INFINITY, l = 0.0f;      // running state of column lq
    float R = 0.0f;                     // running max of the V scales
    f32x4 oacc[DC];
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) oacc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Wave w streams tiles w, w+4, ... of the chunk, two per iteration in
    // two buffers that swap roles; every tile's loads are issued one tile
    // ahead (k_attn_gqa's loop). An odd tile count ends with one tile wholly
    // past the chunk, which reads row 0, is masked and changes nothing.
    constexpr int STEP = NWAVES * 32;
    int tj = cs + wid * 32;
    if (tj < ce) {                      // wave-uniform, scalar
        Kv8Tile<NSC> cur, alt;
        kv8_load_tile(cur, kb, vb, ksb, vsb, tj, ce, Ekv, Hkv, D, lane);
        do {
            kv8_load_tile(alt, kb, vb, ksb, vsb, tj + STEP, ce, Ekv, Hkv, D,
                          lane);
            kv8_tile_step<DC, NSC>(cur, qf, vt, st, tj, ce, lane, qk_scale,
                                   m, l, R, oacc);
            kv8_load_tile(cur, kb, vb, ksb, vsb, tj + 2 * STEP, ce, Ekv, Hkv,
                          D, lane);
            kv8_tile_step<DC, NSC>(alt, qf, vt, st, tj + STEP, ce, lane,
                                   qk_scale, m, l, R, oacc);
            tj += 2 * STEP;
        } while (tj < ce);
    }
    gqa_block_sync();                   // tiles and Q are dead: reuse LDS

    // merge the 4 waves' partials in wave order (lane group 0 holds the
    // column's (m, l); oacc[dc][jj] * R is O[d = dc*16 + lg*4 + jj][col lq])
    if (lg == 0) {
        lds_m[wid][lq] = m;
        lds_l[wid][lq] = l;
    }
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            lds_o[(wid * 16 + lq) * OSTR + dc * 16 + lg * 4 + jj] =
                oacc[dc][jj] * R;
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

// ----------------------------------------------------- prefill attention
// k_attn_kv8_prefill: k_attn_kv8 with the consumers of a KV row changed, the
// step k_attn_prefix made from k_attn_gqa. One block per (16-query tile,
// query head), grid (ceil(T/16), H): the 16 MFMA columns are the tile's 16
// queries for one head, so a KV row is read and expanded from bytes once per
// 16 queries, not once per query. No split-KV, no workspace: prefill
// launches are wide. The tile's same-seq segments are walked as in
// k_attn_prefill_mfma: for a segment the block streams rows [0, jmax + 1) of
// its slot with the loop of k_attn_kv8 (Kv8Tile, kv8_load_tile, kv8_stage_v,
// kv8_expand4 as they are), and score slot (row j, column c) is live iff
// j < lim[c], lim = pos + 1 for a column of the segment and 0 for any other.
//
// The running state (m, l, R) is per column, and "the wave's first tile has
// an attended row" does not hold per column: a column can be outside the
// segment, past T, or have every row of this wave's tiles above its pos.
// Such a column is `dead` (m_new = -inf): p = 0, alpha = 1, R stays 0, so it
// keeps (m = -inf, l = 0, o = 0) and no -inf - -inf is ever formed. A tile
// that is masked for a column that has state leaves that state bit for bit:
// tm = -inf and svm = 0 give m_new = m, R_new = R, alpha = expf(0) = 1 and
// P~ = 0. R is the running maximum of the V scales over the rows the COLUMN
// attends, carried like m, so P~ = p * s_v / R <= 1 per token and a token's
// bits do not depend on its tile mates. Row 0 is attended by every token and
// belongs to wave 0's first tile, so the merge sees l > 0 for every t < T.

// kv8_tile_step with a per-column row limit and dead-column handling
template <int DC, int NSC>
GQA_FN __device__ __forceinline__ void kv8_tile_step_q(
    const Kv8Tile<NSC>& tile, const ABFrag (&qf)[2 * NSC], uint32_t* vt,
    _Float16* st, int tj, int lim, int lane, float qk_scale, float& m,
    float& l, float& R, f32x4 (&oacc)[DC]) {
    const int lq = lane & 15;
    const int lg = lane >> 4;
    f32x4 sc[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        sc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NSC; ++c) {
            ABFrag ka, kb;
            kv8_expand4(tile.k[r][c][0], ka.u[0], ka.u[1]);
            kv8_expand4(tile.k[r][c][1], ka.u[2], ka.u[3]);
            kv8_expand4(tile.k[r][c][2], kb.u[0], kb.u[1]);
            kv8_expand4(tile.k[r][c][3], kb.u[2], kb.u[3]);
            sc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                ka.v, qf[2 * c].v, sc[r], 0, 0, 0);
            sc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                kb.v, qf[2 * c + 1].v, sc[r], 0, 0, 0);
        }
    }
    reinterpret_cast<unsigned short*>(st)[lane] = tile.sc;
    kv8_stage_v(vt, tile.v, lane);
    gqa_wave_sync();                        // scales, V tile written -> read

    // lane holds s[j = tj + r*16 + lg*4 + jj][column lq] as slot r*4 + jj
    float s[8], sv[8], tm = -INFINITY, svm = 0.0f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const kv8_f16x4 ks =
            *reinterpret_cast<const kv8_f16x4*>(st + r * 16 + lg * 4);
        const kv8_f16x4 vs =
            *reinterpret_cast<const kv8_f16x4*>(st + 32 + r * 16 + lg * 4);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const bool ok = tj + r * 16 + lg * 4 + jj < lim;
            s[r * 4 + jj] = ok ? sc[r][jj] * ((float)ks[jj] * qk_scale)
                               : -INFINITY;
            sv[r * 4 + jj] = ok ? (float)vs[jj] : 0.0f;
            tm = fmaxf(tm, s[r * 4 + jj]);
            svm = fmaxf(svm, sv[r * 4 + jj]);
        }
    }
    tm = fmaxf(tm, gqa_shfl_xor(tm, lane, 16));
    tm = fmaxf(tm, gqa_shfl_xor(tm, lane, 32));
    // a tile above every column's limit (the odd tile past the segment end):
    // wave-uniform skip, nothing changes
    if (__builtin_amdgcn_ballot_w64(tm != -INFINITY) == 0) {
        gqa_wave_sync();                    // read -> next tile's write
        return;
    }
    svm = fmaxf(svm, gqa_shfl_xor(svm, lane, 16));
    svm = fmaxf(svm, gqa_shfl_xor(svm, lane, 32));
    const float m_new = fmaxf(m, tm);
    const float R_new = fmaxf(R, svm);
    const bool dead = m_new == -INFINITY;   // column has attended no row yet
    const float inv_r = (R_new > 0.0f) ? __builtin_amdgcn_rcpf(R_new) : 0.0f;
    // m = -inf: l = 0 and oacc = 0, any finite factor will do; 1 keeps a
    // dead column out of the rescale below
    const float alpha = (m == -INFINITY) ? (dead ? 1.0f : 0.0f)
                                         : __expf(m - m_new);
    // accumulators are in units of R: exactly 1 while R stands
    const float alpha_o = alpha * ((R_new == R) ? 1.0f : R * inv_r);
    float ts = 0.0f, pt[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float p = dead ? 0.0f : __expf(s[e] - m_new);  // 0 if masked
        ts += p;
        pt[e] = p * (sv[e] * inv_r);            // P~ in [0, 1]
    }
    ABFrag p;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        p.u[i] = gqa_pack_f16(pt[2 * i], pt[2 * i + 1]);
    ts += gqa_shfl_xor(ts, lane, 16);
    ts += gqa_shfl_xor(ts, lane, 32);
    l = l * alpha + ts;
    m = m_new;
    R = R_new;

    // wave-uniform branch; x * 1 is x, so a column whose factor is 1 keeps
    // its bits whatever the other columns do
    if (__builtin_amdgcn_ballot_w64(alpha_o != 1.0f) != 0) {
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) {
            oacc[dc][0] *= alpha_o; oacc[dc][1] *= alpha_o;
            oacc[dc][2] *= alpha_o; oacc[dc][3] *= alpha_o;
        }
    }
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
        ABFrag vf;
        kv8_expand4(vt[lg * KV8_VSTRIDE + dc * 16 + lq], vf.u[0], vf.u[1]);
        kv8_expand4(vt[(4 + lg) * KV8_VSTRIDE + dc * 16 + lq], vf.u[2],
                    vf.u[3]);
        oacc[dc] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf.v, p.v,
                                                          oacc[dc], 0, 0, 0);
    }
    gqa_wave_sync();                        // read -> next tile's write
}

int attn_kv8_route(int T, int decode, int kv8_prefill) {
    return (T > 64 && !decode && kv8_prefill) ? 1 : 0;
}

template <int DC>
GQA_FN __global__ __launch_bounds__(BLOCK) void k_attn_kv8_prefill(
    const float* __restrict__ q_buf, const uint8_t* __restrict__ k8,
    const uint8_t* __restrict__ v8, const __half* __restrict__ k_scale,
    const __half* __restrict__ v_scale, float* __restrict__ out,
    unsigned short* __restrict__ out_prep, const int* __restrict__ pos,
    const int* __restrict__ seq, int T, int grp, int E, int Ekv, int D,
    int n_ctx, int jtw) {
    constexpr int NSC = DC > 4 ? DC / 4 : 1;
    constexpr int QW = NSC * 64;        // staged q row, halves
    const int t0 = (int)blockIdx.x * 16;
    const int h = blockIdx.y;
    const int hk = h / grp;             // GQA kv head
    const int nq = min(16, T - t0);
    const int Hkv = Ekv / D;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);  // scalar
    const int lq = lane & 15;
    const int lg = lane >> 4;

    // LDS as in k_attn_kv8: the waves' V tiles and scales and the staged Q
    // while streaming, the waves' O partials [w][col][OSTR] after it
    constexpr int OSTR = DC * 16 + 4;
    constexpr int VT_BYTES = NWAVES * 8 * KV8_VSTRIDE * (int)sizeof(uint32_t);
    constexpr int SC_BYTES = NWAVES * 64 * (int)sizeof(_Float16);
    constexpr int Q_BYTES = 16 * (QW + 8) * (int)sizeof(_Float16);
    constexpr int O_BYTES = NWAVES * 16 * OSTR * (int)sizeof(float);
    constexpr int S_BYTES = VT_BYTES + SC_BYTES + Q_BYTES;
    constexpr int LDS_BYTES = S_BYTES > O_BYTES ? S_BYTES : O_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    __shared__ float lds_m[NWAVES][16];
    __shared__ float lds_l[NWAVES][16];
    __shared__ int lds_pos[16];
    __shared__ int lds_seq[16];         // -1 past T
    uint32_t* vt = reinterpret_cast<uint32_t*>(lds_raw) +
                   wid * 8 * KV8_VSTRIDE;
    _Float16* st = reinterpret_cast<_Float16*>(lds_raw + VT_BYTES) + wid * 64;
    _Float16 (*lds_q)[QW + 8] = reinterpret_cast<_Float16 (*)[QW + 8]>(
        lds_raw + VT_BYTES + SC_BYTES);
    float* lds_o = reinterpret_cast<float*>(lds_raw);

    if (tid < 16) {
        const bool ok = tid < nq;
        lds_pos[tid] = ok ? pos[t0 + (ok ? tid : 0)] : 0;
        lds_seq[tid] = ok ? seq[t0 + (ok ? tid : 0)] : -1;
    }
    // Q tile -> LDS as plain f16, zero past D and past T (the factor does
    // the masking). 1/sqrt(D) joins the K scale.
    {
        const float* qt = q_buf + (size_t)t0 * E + (size_t)h * D;
#pragma unroll
        for (int i = 0; i < 16 * QW / BLOCK; ++i) {
            const int idx = tid + i * BLOCK;
            const int col = idx / QW;
            const int d = idx % QW;
            const bool ok = col < nq && d < D;
            const float v = qt[ok ? (size_t)col * E + d : 0] *
                            (ok ? 1.0f : 0.0f);
            lds_q[col][d] = (_Float16)v;
        }
    }
    gqa_block_sync();
    // score-MFMA B fragments in k_attn_kv8's permuted contraction order:
    // lane (column lq, lg) holds d = c*64 + lg*16 + 0..7 for the first MFMA
    // of chunk c and + 8..15 for the second
    ABFrag qf[2 * NSC];
#pragma unroll
    for (int c = 0; c < 2 * NSC; ++c) {
        const uint4 u = *reinterpret_cast<const uint4*>(
            &lds_q[lq][(c >> 1) * 64 + lg * 16 + (c & 1) * 8]);
        qf[c].u[0] = u.x; qf[c].u[1] = u.y;
        qf[c].u[2] = u.z; qf[c].u[3] = u.w;
    }
    const float qk_scale = rsqrtf((float)D);
    const int pos_q = lds_pos[lq];

    float m = -INFINITY, l = 0.0f;      // running state of column lq
    float R = 0.0f;                     // running max of its rows' V scales
    f32x4 oacc[DC];
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) oacc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

    constexpr int STEP = NWAVES * 32;
    int a = 0;
    while (a < nq) {                    // same-seq segments, block-uniform
        const int sseq = __builtin_amdgcn_readfirstlane(lds_seq[a]);
        int b = a + 1;
        while (b < nq && __builtin_amdgcn_readfirstlane(lds_seq[b]) == sseq)
            ++b;
        int jmax = 0;
        for (int c = a; c < b; ++c)
            jmax = max(jmax, __builtin_amdgcn_readfirstlane(lds_pos[c]));
        const int J = jmax + 1;         // rows streamed: [0, J) of slot sseq
        const int lim = (lq >= a && lq < b) ? pos_q + 1 : 0;
        const size_t row0 = (size_t)sseq * n_ctx;
        const uint8_t* kb = k8 + row0 * Ekv + hk * D;
        const uint8_t* vb = v8 + row0 * Ekv + hk * D;
        const unsigned short* ksb =
            reinterpret_cast<const unsigned short*>(k_scale) + row0 * Hkv +
            hk;
        const unsigned short* vsb =
            reinterpret_cast<const unsigned short*>(v_scale) + row0 * Hkv +
            hk;
        // k_attn_kv8's loop: wave w streams tiles w, w+4, ..., two per
        // iteration in two buffers, loads one tile ahead; rows at or past J
        // read row 0 and are above every lim
        int tj = wid * 32;
        if (tj < J) {                   // wave-uniform, scalar
            Kv8Tile<NSC> cur, alt;
            kv8_load_tile(cur, kb, vb, ksb, vsb, tj, J, Ekv, Hkv, D, lane);
            do {
                kv8_load_tile(alt, kb, vb, ksb, vsb, tj + STEP, J, Ekv, Hkv,
                              D, lane);
                kv8_tile_step_q<DC, NSC>(cur, qf, vt, st, tj, lim, lane,
                                         qk_scale, m, l, R, oacc);
                kv8_load_tile(cur, kb, vb, ksb, vsb, tj + 2 * STEP, J, Ekv,
                              Hkv, D, lane);
                kv8_tile_step_q<DC, NSC>(alt, qf, vt, st, tj + STEP, lim,
                                         lane, qk_scale, m, l, R, oacc);
                tj += 2 * STEP;
            } while (tj < J);
        }
        a = b;
    }
    gqa_block_sync();                   // tiles and Q are dead: reuse LDS

    // merge the 4 waves' partials in wave order (lane group 0 holds the
    // column's (m, l); oacc[dc][jj] * R is O[d = dc*16 + lg*4 + jj][col lq])
    if (lg == 0) {
        lds_m[wid][lq] = m;
        lds_l[wid][lq] = l;
    }
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            lds_o[(wid * 16 + lq) * OSTR + dc * 16 + lg * 4 + jj] =
                oacc[dc][jj] * R;
    }
    gqa_block_sync();
    const int col = tid >> 4;
    if (col >= nq) return;
    float mstar = -INFINITY;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) mstar = fmaxf(mstar, lds_m[w][col]);
    float wsc[NWAVES], lstar = 0.0f;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const float mw = lds_m[w][col];         // -inf: no row of this wave
        wsc[w] = (mw == -INFINITY) ? 0.0f : __expf(mw - mstar);
        lstar += lds_l[w][col] * wsc[w];
    }
    for (int d = tid & 15; d < D; d += 16) {
        float ostar = 0.0f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w)
            ostar += lds_o[(w * 16 + col) * OSTR + d] * wsc[w];
        gqa_store_out(ostar / lstar, h * D + d, t0 + col, E, jtw, out,
                      out_prep);
    }
}

// ------------------------------------------- shared-prefix attention (q8)
// launch_attn_prefix's semantics over the byte caches (kv8_prefix): token t
// attends rows [0, pfx[t]) of slot `pslot`, then rows [pfx[t], pos[t]] of its
// own slot seq[t]; pfx[t] is 0 or P.
//
// k_attn_kv8_prefix covers the prefix rows. It is k_attn_kv8_prefill with one
// segment, slot pslot, cut into chunks: one block per (16-token tile, query
// head, prefix chunk [cs, ce)), the tile's tokens as the MFMA columns, so a
// prefix row is read and expanded from bytes once per 16 tokens. The stream
// is kv8_tile_step_q as it is, with the per-column limit min(pfx[c], ce)
// (0 past T): a column without a prefix is dead and keeps (m = -inf, l = 0,
// o = 0, R = 0) for the whole stream. Every sharing column attends every row
// of every tile of the chunk, so each wave that has a tile has state for it.
// The epilogue merges the four waves in wave order and always writes the
// un-normalised partial (m, l, o[D]), o already multiplied by the column's
// R, to ws [T][H][S][D + 2]; (-inf, 0, 0) for a column without a prefix. A
// tile with no sharing token writes its empty partials and streams nothing.
//
// k_attn_kv8_prefix_tail covers the own rows. It is k_attn_kv8 over the row
// window [r0, pos[t]] of slot seq[t], r0 = P for a sharing token and 0
// otherwise: one block per (token, KV head, up to 16 query heads of its
// group), the heads as columns, kv8_tile_step as it is, all four waves, no
// split (own spans are short where the prefix is long, and a token that does
// not share is the rare one). The cache bases are advanced by r0 rows and
// the loop runs j in [0, J), J = pos[t] + 1 - r0: rows are addressed as
// r0 + j and masked on j, so r0 need not be a multiple of the tile and the
// masked rows read row r0, which is inside the window. The epilogue folds,
// per head, first the ceil(P / chunk) prefix partials in ascending chunk
// order and then the four waves in wave order, against one common maximum,
// normalises and stores. Row pos[t] is always in the window: l > 0.
//
// MFMA columns are independent and all running state is per column (prefix
// pass) or wave-uniform and a function of the rows alone (tail: R), so a
// token's bits depend on neither its tile mates, its column, the other
// heads of its group nor, for T <= 64, on T.
constexpr int KV8P_MIN_CHUNK = 256;  // prefix rows per split (unmeasured)
constexpr int KV8P_MAX_SPLITS = 8;   // splits of a full context (unmeasured)

int attn_kv8_prefix_chunk(int n_ctx) {
    const int per = (n_ctx + KV8P_MAX_SPLITS - 1) / KV8P_MAX_SPLITS;
    return std::max(KV8P_MIN_CHUNK, (per + 63) & ~63);
}

int attn_kv8_prefix_splits(int n_ctx, int T) {
    if (T > 64) return 1;  // more than 4 tiles per head fill the chip
    const int chunk = attn_kv8_prefix_chunk(n_ctx);
    return (n_ctx + chunk - 1) / chunk;
}

template <int DC>
GQA_FN __global__ __launch_bounds__(BLOCK) void k_attn_kv8_prefix(
    const float* __restrict__ q_buf, const uint8_t* __restrict__ k8,
    const uint8_t* __restrict__ v8, const __half* __restrict__ k_scale,
    const __half* __restrict__ v_scale, const int* __restrict__ pfx,
    float* __restrict__ ws, int pslot, int P, int T, int grp, int E, int Ekv,
    int D, int n_ctx, int chunk) {
    constexpr int NSC = DC > 4 ? DC / 4 : 1;
    constexpr int QW = NSC * 64;        // staged q row, halves
    const int cs = (int)blockIdx.z * chunk;
    if (cs >= P) return;                // block-uniform: chunk past the prefix
    const int ce = min(P, cs + chunk);
    const int t0 = (int)blockIdx.x * 16;
    const int h = blockIdx.y;
    const int H = gridDim.y;
    const int hk = h / grp;             // GQA kv head
    const int nq = min(16, T - t0);
    const int Hkv = Ekv / D;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);  // scalar
    const int lq = lane & 15;
    const int lg = lane >> 4;

    // LDS as in k_attn_kv8_prefill
    constexpr int OSTR = DC * 16 + 4;
    constexpr int VT_BYTES = NWAVES * 8 * KV8_VSTRIDE * (int)sizeof(uint32_t);
    constexpr int SC_BYTES = NWAVES * 64 * (int)sizeof(_Float16);
    constexpr int Q_BYTES = 16 * (QW + 8) * (int)sizeof(_Float16);
    constexpr int O_BYTES = NWAVES * 16 * OSTR * (int)sizeof(float);
    constexpr int S_BYTES = VT_BYTES + SC_BYTES + Q_BYTES;
    constexpr int LDS_BYTES = S_BYTES > O_BYTES ? S_BYTES : O_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    __shared__ float lds_m[NWAVES][16];
    __shared__ float lds_l[NWAVES][16];
    __shared__ int lds_lim[16];         // min(pfx, ce); 0: no prefix, past T
    uint32_t* vt = reinterpret_cast<uint32_t*>(lds_raw) +
                   wid * 8 * KV8_VSTRIDE;
    _Float16* st = reinterpret_cast<_Float16*>(lds_raw + VT_BYTES) + wid * 64;
    _Float16 (*lds_q)[QW + 8] = reinterpret_cast<_Float16 (*)[QW + 8]>(
        lds_raw + VT_BYTES + SC_BYTES);
    float* lds_o = reinterpret_cast<float*>(lds_raw);

    if (tid < 16) {
        const bool ok = tid < nq;
        lds_lim[tid] = ok ? min(pfx[t0 + (ok ? tid : 0)], ce) : 0;
    }
    gqa_block_sync();
    int nact = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) nact += lds_lim[c] > 0 ? 1 : 0;

    if (nact > 0) {                     // block-uniform
        // Q tile -> LDS as plain f16, zero past D and past T (the factor
        // does the masking). 1/sqrt(D) joins the K scale.
        {
            const float* qt = q_buf + (size_t)t0 * E + (size_t)h * D;
#pragma unroll
            for (int i = 0; i < 16 * QW / BLOCK; ++i) {
                const int idx = tid + i * BLOCK;
                const int col = idx / QW;
                const int d = idx % QW;
                const bool ok = col < nq && d < D;
                const float v = qt[ok ? (size_t)col * E + d : 0] *
                                (ok ? 1.0f : 0.0f);
                lds_q[col][d] = (_Float16)v;
            }
        }
        gqa_block_sync();
        // score-MFMA B fragments in k_attn_kv8's permuted contraction order
        ABFrag qf[2 * NSC];
#pragma unroll
        for (int c = 0; c < 2 * NSC; ++c) {
            const uint4 u = *reinterpret_cast<const uint4*>(
                &lds_q[lq][(c >> 1) * 64 + lg * 16 + (c & 1) * 8]);
            qf[c].u[0] = u.x; qf[c].u[1] = u.y;
            qf[c].u[2] = u.z; qf[c].u[3] = u.w;
        }
        const float qk_scale = rsqrtf((float)D);
        const int lim = lds_lim[lq];
        const size_t row0 = (size_t)pslot * n_ctx;
        const uint8_t* kb = k8 + row0 * Ekv + hk * D;
        const uint8_t* vb = v8 + row0 * Ekv + hk * D;
        const unsigned short* ksb =
            reinterpret_cast<const unsigned short*>(k_scale) + row0 * Hkv +
            hk;
        const unsigned short* vsb =
            reinterpret_cast<const unsigned short*>(v_scale) + row0 * Hkv +
            hk;

        float m = -INFINITY, l = 0.0f;  // running state of column lq
        float R = 0.0f;                 // running max of its rows' V scales
        f32x4 oacc[DC];
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) oacc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

        // k_attn_kv8's loop over the chunk: wave w streams tiles w, w+4,
        // ..., two per iteration in two buffers, loads one tile ahead; rows
        // at or past ce read row 0 of the slot and are above every lim
        constexpr int STEP = NWAVES * 32;
        int tj = cs + wid * 32;
        if (tj < ce) {                  // wave-uniform, scalar
            Kv8Tile<NSC> cur, alt;
            kv8_load_tile(cur, kb, vb, ksb, vsb, tj, ce, Ekv, Hkv, D, lane);
            do {
                kv8_load_tile(alt, kb, vb, ksb, vsb, tj + STEP, ce, Ekv, Hkv,
                              D, lane);
                kv8_tile_step_q<DC, NSC>(cur, qf, vt, st, tj, lim, lane,
                                         qk_scale, m, l, R, oacc);
                kv8_load_tile(cur, kb, vb, ksb, vsb, tj + 2 * STEP, ce, Ekv,
                              Hkv, D, lane);
                kv8_tile_step_q<DC, NSC>(alt, qf, vt, st, tj + STEP, lim,
                                         lane, qk_scale, m, l, R, oacc);
                tj += 2 * STEP;
            } while (tj < ce);
        }
        gqa_block_sync();               // tiles and Q are dead: reuse LDS

        if (lg == 0) {
            lds_m[wid][lq] = m;
            lds_l[wid][lq] = l;
        }
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                lds_o[(wid * 16 + lq) * OSTR + dc * 16 + lg * 4 + jj] =
                    oacc[dc][jj] * R;
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
    if (lds_lim[col] == 0) {
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

template <int DC>
GQA_FN __global__ __launch_bounds__(BLOCK) void k_attn_kv8_prefix_tail(
    const float* __restrict__ q_buf, const uint8_t* __restrict__ k8,
    const uint8_t* __restrict__ v8, const __half* __restrict__ k_scale,
    const __half* __restrict__ v_scale, float* __restrict__ out,
    unsigned short* __restrict__ out_prep, const int* __restrict__ pos,
    const int* __restrict__ seq, const int* __restrict__ pfx,
    const float* __restrict__ ws, int P, int H, int grp, int E, int Ekv,
    int D, int n_ctx, int jtw, int chunk, int S) {
    constexpr int NSC = DC > 4 ? DC / 4 : 1;
    constexpr int QW = NSC * 64;        // staged q row, halves
    const int t = blockIdx.x;
    const int r0 = pfx[t] > 0 ? P : 0;
    const int J = pos[t] + 1 - r0;      // own rows r0 + [0, J), J >= 1
    const int ntile = (grp + 15) >> 4;  // column tiles per KV head
    const int hk = (int)blockIdx.y / ntile;
    const int c0 = ((int)blockIdx.y % ntile) * 16;  // first column's head
    const int ncol = min(16, grp - c0);
    const int Hkv = Ekv / D;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);  // scalar
    const int lq = lane & 15;
    const int lg = lane >> 4;
    // bases at row r0 of the slot: j = 0 is the window's first row
    const size_t row0 = (size_t)seq[t] * n_ctx + r0;
    const uint8_t* kb = k8 + row0 * Ekv + hk * D;
    const uint8_t* vb = v8 + row0 * Ekv + hk * D;
    const unsigned short* ksb =
        reinterpret_cast<const unsigned short*>(k_scale) + row0 * Hkv + hk;
    const unsigned short* vsb =
        reinterpret_cast<const unsigned short*>(v_scale) + row0 * Hkv + hk;

    // LDS as in k_attn_kv8
    constexpr int OSTR = DC * 16 + 4;
    constexpr int VT_BYTES = NWAVES * 8 * KV8_VSTRIDE * (int)sizeof(uint32_t);
    constexpr int SC_BYTES = NWAVES * 64 * (int)sizeof(_Float16);
    constexpr int Q_BYTES = 16 * (QW + 8) * (int)sizeof(_Float16);
    constexpr int O_BYTES = NWAVES * 16 * OSTR * (int)sizeof(float);
    constexpr int S_BYTES = VT_BYTES + SC_BYTES + Q_BYTES;
    constexpr int LDS_BYTES = S_BYTES > O_BYTES ? S_BYTES : O_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    __shared__ float lds_m[NWAVES][16];
    __shared__ float lds_l[NWAVES][16];
    uint32_t* vt = reinterpret_cast<uint32_t*>(lds_raw) +
                   wid * 8 * KV8_VSTRIDE;
    _Float16* st = reinterpret_cast<_Float16*>(lds_raw + VT_BYTES) + wid * 64;
    _Float16 (*lds_q)[QW + 8] = reinterpret_cast<_Float16 (*)[QW + 8]>(
        lds_raw + VT_BYTES + SC_BYTES);
    float* lds_o = reinterpret_cast<float*>(lds_raw);

    // Own spans are short where the prefix is long (one tile per wave or
    // none), so the kernel is a chain of latencies: the wave's first tile is
    // requested before the Q tile, and the two round trips overlap. A wave
    // without a tile (tj >= J) loads row r0 and drops it.
    constexpr int STEP = NWAVES * 32;
    int tj = wid * 32;
    Kv8Tile<NSC> cur, alt;
    kv8_load_tile(cur, kb, vb, ksb, vsb, tj, J, Ekv, Hkv, D, lane);

    // Q tile -> LDS as f16, zero past D and past the group's last head (the
    // factor does the masking). 1/sqrt(D) joins the K scale.
    {
        const float* qt = q_buf + (size_t)t * E + (size_t)(hk * grp + c0) * D;
#pragma unroll
        for (int i = 0; i < 16 * QW / BLOCK; ++i) {
            const int idx = tid + i * BLOCK;
            const int col = idx / QW;
            const int d = idx % QW;
            const bool ok = col < ncol && d < D;
            const float v = qt[ok ? col * D + d : 0] * (ok ? 1.0f : 0.0f);
            lds_q[col][d] = (_Float16)v;
        }
    }
    gqa_block_sync();
    ABFrag qf[2 * NSC];
#pragma unroll
    for (int c = 0; c < 2 * NSC; ++c) {
        const uint4 u = *reinterpret_cast<const uint4*>(
            &lds_q[lq][(c >> 1) * 64 + lg * 16 + (c & 1) * 8]);
        qf[c].u[0] = u.x; qf[c].u[1] = u.y;
        qf[c].u[2] = u.z; qf[c].u[3] = u.w;
    }
    const float qk_scale = rsqrtf((float)D);

    float m = -INFINITY, l = 0.0f;      // running state of column lq
    float R = 0.0f;                     // running max of the V scales
    f32x4 oacc[DC];
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) oacc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

    // k_attn_kv8's loop over j in [0, J): rows at or past J read row r0.
    // The loads stay unconditional; the step of a tile wholly past J, which
    // would change nothing (kv8_tile_step), is skipped by a scalar branch.
    if (tj < J) {                       // wave-uniform, scalar
        do {
            kv8_load_tile(alt, kb, vb, ksb, vsb, tj + STEP, J, Ekv, Hkv, D,
                          lane);
            kv8_tile_step<DC, NSC>(cur, qf, vt, st, tj, J, lane, qk_scale, m,
                                   l, R, oacc);
            kv8_load_tile(cur, kb, vb, ksb, vsb, tj + 2 * STEP, J, Ekv, Hkv,
                          D, lane);
            if (tj + STEP < J)
                kv8_tile_step<DC, NSC>(alt, qf, vt, st, tj + STEP, J, lane,
                                       qk_scale, m, l, R, oacc);
            tj += 2 * STEP;
        } while (tj < J);
    }
    gqa_block_sync();                   // tiles and Q are dead: reuse LDS

    if (lg == 0) {
        lds_m[wid][lq] = m;
        lds_l[wid][lq] = l;
    }
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            lds_o[(wid * 16 + lq) * OSTR + dc * 16 + lg * 4 + jj] =
                oacc[dc][jj] * R;
    }
    gqa_block_sync();
    // thread (col, d mod 16): the prefix partials in ascending chunk order,
    // then the 4 waves in wave order, against one common maximum
    const int col = tid >> 4;
    if (col >= ncol) return;
    const int h = hk * grp + c0 + col;
    const int n = r0 > 0 ? (P + chunk - 1) / chunk : 0;     // <= S
    const float* part = ws + ((size_t)t * H + h) * S * (size_t)(D + 2);
    float mstar = -INFINITY;
    for (int i = 0; i < n; ++i)
        mstar = fmaxf(mstar, part[(size_t)i * (D + 2)]);
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) mstar = fmaxf(mstar, lds_m[w][col]);
    // mstar is finite (row pos[t]); a sharing token's partials are too
    float lstar = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float* pi = part + (size_t)i * (D + 2);
        lstar += pi[1] * __expf(pi[0] - mstar);
    }
    float wsc[NWAVES];
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const float mw = lds_m[w][col];         // -inf: wave had no tile
        wsc[w] = (mw == -INFINITY) ? 0.0f : __expf(mw - mstar);
        lstar += lds_l[w][col] * wsc[w];
    }
    for (int d = tid & 15; d < D; d += 16) {
        float num = 0.0f;
        for (int i = 0; i < n; ++i) {
            const float* pi = part + (size_t)i * (D + 2);
            num += pi[2 + d] * __expf(pi[0] - mstar);
        }
#pragma unroll
        for (int w = 0; w < NWAVES; ++w)
            num += lds_o[(w * 16 + col) * OSTR + d] * wsc[w];
        gqa_store_out(num / lstar, h * D + d, t, E, jtw, out, out_prep);
    }
}

// ============================================================== launchers

void launch_kv8_append(hipStream_t s, const __half* k_stage,
                       const __half* v_stage, uint8_t* k8_layer,
                       uint8_t* v8_layer, __half* k_scale_layer,
                       __half* v_scale_layer, const int* pos, const int* seq,
                       int T, int Hkv, int D, int n_ctx) {
    hipLaunchKernelGGL(k_kv8_append, dim3((T * Hkv + NWAVES - 1) / NWAVES),
                       dim3(BLOCK), 0, s, k_stage, v_stage, k8_layer,
                       v8_layer, k_scale_layer, v_scale_layer, pos, seq, T,
                       Hkv, D, n_ctx);
}

void launch_attn_kv8(hipStream_t s, const float* q_buf,
                     const uint8_t* k8_layer, const uint8_t* v8_layer,
                     const __half* k_scale_layer,
                     const __half* v_scale_layer, float* out,
                     unsigned short* out_prep, const int* pos,
                     const int* seq, int T, int H, int Hkv, int E, int Ekv,
                     int D, int n_ctx, float* ws) {
    const int grp = H / Hkv;
    const int S = attn_kv8_splits(n_ctx, T);
    // one split covers the whole context, whatever its length
    const int chunk = (S == 1) ? std::max(n_ctx, KV8_MIN_CHUNK)
                               : attn_kv8_chunk(n_ctx);
    const int jtw = jt_width(T);
    const dim3 grid(T, Hkv * ((grp + 15) / 16), S);
    auto kern = D <= 16 ? k_attn_kv8<1> : D <= 32 ? k_attn_kv8<2>
              : D <= 64 ? k_attn_kv8<4> : k_attn_kv8<8>;
    hipLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, s, q_buf, k8_layer,
                       v8_layer, k_scale_layer, v_scale_layer, out, out_prep,
                       pos, seq, ws, H, grp, E, Ekv, D, n_ctx, jtw, chunk);
    if (S > 1)
        launch_attn_gqa_merge(s, ws, out, out_prep, pos, T, H, E, D, jtw,
                              chunk, S);
}

void launch_attn_kv8_prefill(hipStream_t s, const float* q_buf,
                             const uint8_t* k8_layer, const uint8_t* v8_layer,
                             const __half* k_scale_layer,
                             const __half* v_scale_layer, float* out,
                             unsigned short* out_prep, const int* pos,
                             const int* seq, int T, int H, int Hkv, int E,
                             int Ekv, int D, int n_ctx) {
    auto kern = D <= 16 ? k_attn_kv8_prefill<1>
              : D <= 32 ? k_attn_kv8_prefill<2>
              : D <= 64 ? k_attn_kv8_prefill<4> : k_attn_kv8_prefill<8>;
    hipLaunchKernelGGL(kern, dim3((T + 15) / 16, H), dim3(BLOCK), 0, s, q_buf,
                       k8_layer, v8_layer, k_scale_layer, v_scale_layer, out,
                       out_prep, pos, seq, T, H / Hkv, E, Ekv, D, n_ctx,
                       jt_width(T));
}

template <int DC>
static void kv8_prefix_launch(hipStream_t s, const float* q_buf,
                              const uint8_t* k8, const uint8_t* v8,
                              const __half* ksc, const __half* vsc,
                              float* out, unsigned short* out_prep,
                              const int* pos, const int* seq, const int* pfx,
                              int pslot, int P, int T, int H, int Hkv, int E,
                              int Ekv, int D, int n_ctx, float* ws, int chunk,
                              int S) {
    const int grp = H / Hkv;
    hipLaunchKernelGGL(k_attn_kv8_prefix<DC>, dim3((T + 15) / 16, H, S),
                       dim3(BLOCK), 0, s, q_buf, k8, v8, ksc, vsc, pfx, ws,
                       pslot, P, T, grp, E, Ekv, D, n_ctx, chunk);
    hipLaunchKernelGGL(k_attn_kv8_prefix_tail<DC>,
                       dim3(T, Hkv * ((grp + 15) / 16)), dim3(BLOCK), 0, s,
                       q_buf, k8, v8, ksc, vsc, out, out_prep, pos, seq, pfx,
                       ws, P, H, grp, E, Ekv, D, n_ctx, jt_width(T), chunk,
                       S);
}

void launch_attn_kv8_prefix(hipStream_t s, const float* q_buf,
                            const uint8_t* k8_layer, const uint8_t* v8_layer,
                            const __half* k_scale_layer,
                            const __half* v_scale_layer, float* out,
                            unsigned short* out_prep, const int* pos,
                            const int* seq, const int* pfx, int pslot, int P,
                            int T, int H, int Hkv, int E, int Ekv, int D,
                            int n_ctx, float* ws) {
    const int S = attn_kv8_prefix_splits(n_ctx, T);
    // one split covers the whole prefix, whatever its length
    const int chunk = (S == 1) ? std::max(n_ctx, KV8P_MIN_CHUNK)
                               : attn_kv8_prefix_chunk(n_ctx);
    auto fn = D <= 16 ? kv8_prefix_launch<1> : D <= 32 ? kv8_prefix_launch<2>
            : D <= 64 ? kv8_prefix_launch<4> : kv8_prefix_launch<8>;
    fn(s, q_buf, k8_layer, v8_layer, k_scale_layer, v_scale_layer, out,
       out_prep, pos, seq, pfx, pslot, P, T, H, Hkv, E, Ekv, D, n_ctx, ws,
       chunk, S);
}
