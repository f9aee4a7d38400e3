// Paged KV cache (kv_layout = paged, gfx950): `k_paged_rows`, which turns
// (block table, pos, seq) into the pool row every new K/V row is written to,
// `k_attn_paged` (+ k_attn_gqa_merge), decode-shaped attention over the page
// pools, and its Q-tiled prefill sibling `k_attn_paged_prefill`. This file is compiled wholly without packed-f32 VALU
// instructions (NO_PACKED_F32 in ops/build.py).
//
// Layout. A page is PAGE_ROWS = 16 rows of Ekv halves, one MFMA row tile, so
// a KV tile never straddles a page. Per layer the K and V pools are f16
// [kv_pages * 16, Ekv] (+ 16 halves of tail pad on the allocation). One block
// table, i32 [slots, ceil(n_ctx / 16)], serves every layer: row r of slot s
// lives at pool row table[s][r / 16] * 16 + r % 16. Page 0 is never assigned
// and unassigned table entries are 0, so every table entry is a valid page:
// what lands in page 0 is finite and is only ever read under a mask, and no
// kernel has a branch for "no page".
//
// k_attn_paged has k_attn_gqa's work split and arithmetic (attn_common.h:
// gqa_stage_v, gqa_tile_step): one block per (token, KV head, 16 query heads,
// KV chunk), the query heads as the 16 MFMA columns, four waves on tiles
// w, w+4, ... of the chunk, a merge in wave order and then across splits.
// What is new is how a tile arrives. The block first copies the chunk's page
// ids from the table row of seq[t] into LDS, coalesced. In the stream a wave
// holds the page id of a tile in a register two tiles ahead: it is read from
// LDS before the loads of the tile in front of it are issued, so the global
// loads of tile n+1 never wait on a table load and the two-buffer structure
// (loads one tile ahead, no branch between a load and its use) is k_attn_gqa's.
// Rows at or past the chunk end read the chunk's first row (attended, hence
// written) and are masked; memory that is unread or masked only needs to be
// finite.

#include <algorithm>

#include "attn_common.h"
#include "device_common.h"
#include "kernels.h"

constexpr int PAGE_ROWS = 16;
constexpr int PAGED_MIN_CHUNK = 256;  // rows per split, lower bound (unmeasured)
constexpr int PAGED_MAX_SPLITS = 8;   // splits of a full context (unmeasured)

int kv_page_rows() { return PAGE_ROWS; }

int attn_paged_chunk(int n_ctx) {
    const int per = (n_ctx + PAGED_MAX_SPLITS - 1) / PAGED_MAX_SPLITS;
    return std::max(PAGED_MIN_CHUNK, (per + 63) & ~63);
}

int attn_paged_splits(int n_ctx, int T) {
    if (T > 64) return 1;  // wide decode fills the chip by itself
    const int chunk = attn_paged_chunk(n_ctx);
    return (n_ctx + chunk - 1) / chunk;
}

// kv_row[t] = pool row of (seq[t], pos[t]): once per forward, every layer's
// qkv kernels write through it
__global__ void k_paged_rows(const int* __restrict__ table,
                             const int* __restrict__ pos,
                             const int* __restrict__ seq,
                             int* __restrict__ kv_row, int T, int npg) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= T) return;
    const int p = pos[t];
    kv_row[t] = table[(size_t)seq[t] * npg + (p >> 4)] * PAGE_ROWS + (p & 15);
}

// The page of the tile at row tj of a chunk that starts at cs, as a scalar.
// A tile wholly past the chunk end takes the chunk's first page: its rows
// are all masked, and the index stays inside the ids the block loaded.
__device__ __forceinline__ int paged_tile_page(const int* lds_pg, int tj,
                                               int cs, int ce) {
    return __builtin_amdgcn_readfirstlane(
        lds_pg[tj < ce ? (tj - cs) >> 4 : 0]);
}

// gqa_load_tile over a page: sixteen-byte loads with no branch around them.
// Row r of the tile is pool row pg * 16 + r; rows at or past `ce` read pool
// row pg0 * 16, the chunk's first row. The d spans follow gqa_load_tile:
// spans that start at or past D read span 0, and a span that straddles D
// reads into the next head or the pad; both are dropped by the caller.
template <int NKC>
__device__ __forceinline__ void paged_load_tile(
    GqaTile<NKC>& t, const __half* __restrict__ kb,
    const __half* __restrict__ vb, int pg, int pg0, int tj, int ce, int Ekv,
    int D, int lq, int lg) {
    const int r0 = pg0 * PAGE_ROWS;
    const int rt = pg * PAGE_ROWS;
    const __half* krow = kb + (size_t)(tj + lq < ce ? rt + lq : r0) * Ekv;
#pragma unroll
    for (int c = 0; c < NKC; ++c) {
        const int d0 = c * 32 + lg * 8;
        t.k[c] = *reinterpret_cast<const uint4*>(krow + (d0 < D ? d0 : 0));
    }
    const int dv = (lq * 8 < D) ? lq * 8 : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int jr = lg * 4 + e;
        const __half* vrow = vb + (size_t)(tj + jr < ce ? rt + jr : r0) * Ekv;
        t.v[e] = *reinterpret_cast<const uint4*>(vrow + dv);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// DC = 16-wide d chunks of the PV product, a power of two >= D/16; the
// score product runs NKC = max(1, DC/2) 32-wide chunks. Dynamic LDS: the
// chunk's page ids, ceil(chunk / 16) ints.
template <int DC>
__global__ __launch_bounds__(BLOCK) void k_attn_paged(
    const float* __restrict__ q_buf, const __half* __restrict__ k_pool,
    const __half* __restrict__ v_pool, const int* __restrict__ table,
    float* __restrict__ out, unsigned short* __restrict__ out_prep,
    const int* __restrict__ pos, const int* __restrict__ seq,
    float* __restrict__ ws, int H, int grp, int E, int Ekv, int D, int npg,
    int jtw, int chunk) {
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
    const __half* kb = k_pool + (size_t)hk * D;
    const __half* vb = v_pool + (size_t)hk * D;

    // LDS as in k_attn_gqa (V tiles + staged Q while streaming, the waves' O
    // partials after it), plus the page ids, which live through the stream
    constexpr int OSTR = DC * 16 + 4;
    constexpr int VT_BYTES = NWAVES * 4 * GQA_VSTRIDE * (int)sizeof(uint2);
    constexpr int Q_BYTES = 16 * (QW + 8) * (int)sizeof(_Float16);
    constexpr int O_BYTES = NWAVES * 16 * OSTR * (int)sizeof(float);
    constexpr int LDS_BYTES =
        VT_BYTES + Q_BYTES > O_BYTES ? VT_BYTES + Q_BYTES : O_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    __shared__ float lds_m[NWAVES][16];
    __shared__ float lds_l[NWAVES][16];
    extern __shared__ int lds_pg[];     // [ceil(chunk / 16)]
    uint2* vt = reinterpret_cast<uint2*>(lds_raw) + wid * 4 * GQA_VSTRIDE;
    _Float16 (*lds_q)[QW + 8] =
        reinterpret_cast<_Float16 (*)[QW + 8]>(lds_raw + VT_BYTES);
    float* lds_o = reinterpret_cast<float*>(lds_raw);

    // the chunk's page ids: entries cs/16 .. (ce - 1)/16 of the slot's table
    // row (chunk % 16 == 0 whenever cs > 0), consecutive ints
    {
        const int* trow = table + (size_t)seq[t] * npg + (cs >> 4);
        const int n = (ce - cs + PAGE_ROWS - 1) >> 4;
        for (int i = tid; i < n; i += BLOCK) lds_pg[i] = trow[i];
    }
    // Q tile -> LDS as f16, prescaled by 1/sqrt(D), zero past D and past
    // the group's last head (the factor does the masking)
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
    // two buffers that swap roles (k_attn_gqa's loop). pn is the page of the
    // tile whose loads come next and is already in a register when they are
    // issued; the id for the tile after it is read from LDS first. An odd
    // tile count ends with a tile wholly past the chunk: first page, masked.
    constexpr int STEP = NWAVES * PAGE_ROWS;
    int tj = cs + wid * PAGE_ROWS;
    if (tj < ce) {                      // wave-uniform, scalar
        const int pg0 = __builtin_amdgcn_readfirstlane(lds_pg[0]);
        GqaTile<NKC> cur, alt;
        int pn = paged_tile_page(lds_pg, tj + STEP, cs, ce);
        paged_load_tile(cur, kb, vb, paged_tile_page(lds_pg, tj, cs, ce),
                        pg0, tj, ce, Ekv, D, lq, lg);
        do {
            const int p2 = paged_tile_page(lds_pg, tj + 2 * STEP, cs, ce);
            paged_load_tile(alt, kb, vb, pn, pg0, tj + STEP, ce, Ekv, D, lq,
                            lg);
            gqa_tile_step<DC, NKC>(cur, qf, vt, tj, ce, lane, m, l, oacc);
            pn = paged_tile_page(lds_pg, tj + 3 * STEP, cs, ce);
            paged_load_tile(cur, kb, vb, p2, pg0, tj + 2 * STEP, ce, Ekv, D,
                            lq, lg);
            gqa_tile_step<DC, NKC>(alt, qf, vt, tj + STEP, ce, lane, m, l,
                                   oacc);
            tj += 2 * STEP;
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

// ----------------------------------------------------- prefill attention
// k_attn_paged_prefill: k_attn_paged with the consumers of a KV row changed,
// the step k_attn_kv8_prefill made from k_attn_kv8. One block per (16-query
// tile, query head), grid (ceil(T/16), H): the 16 MFMA columns are the
// tile's 16 queries for one head, so a K/V row is read once per 16 queries,
// not once per query. No split-KV, no workspace: prefill launches are wide.
// The tile's same-seq segments are walked as in k_attn_prefill_mfma. For a
// segment with slot s and J = jmax + 1 the block copies the ceil(J / 16)
// page ids of table row s into LDS (the segment loop is block-uniform, so
// the copy sits between two block barriers and the tile loop has none), then
// streams rows [0, J) with k_attn_paged's loop (paged_tile_page,
// paged_load_tile, GqaTile as they are, cs = 0, ce = J). Score slot (row j,
// column c) is live iff j < lim[c], lim = pos + 1 for a column of the
// segment and 0 for any other: gqa_tile_step_q (attn_common.h), which also
// holds the dead-column rules. Columns past T read no pos, seq or table
// entry. Row 0 is attended by every token and belongs to wave 0's first
// tile, so the merge sees l > 0 for every t < T.

int attn_paged_route(int T, int decode, int paged_prefill) {
    return (T > 64 && !decode && paged_prefill) ? 1 : 0;
}

// Dynamic LDS: one table row of page ids, ceil(n_ctx / 16) ints.
template <int DC>
__global__ __launch_bounds__(BLOCK) void k_attn_paged_prefill(
    const float* __restrict__ q_buf, const __half* __restrict__ k_pool,
    const __half* __restrict__ v_pool, const int* __restrict__ table,
    float* __restrict__ out, unsigned short* __restrict__ out_prep,
    const int* __restrict__ pos, const int* __restrict__ seq, int T, int grp,
    int E, int Ekv, int D, int npg, int jtw) {
    constexpr int NKC = DC > 1 ? DC / 2 : 1;
    constexpr int QW = NKC * 32;        // staged q row, halves
    const int t0 = (int)blockIdx.x * 16;
    const int h = blockIdx.y;
    const int hk = h / grp;             // GQA kv head
    const int nq = min(16, T - t0);
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);  // scalar
    const int lq = lane & 15;
    const int lg = lane >> 4;
    const float inv_sqrt_d = rsqrtf((float)D);
    const __half* kb = k_pool + (size_t)hk * D;
    const __half* vb = v_pool + (size_t)hk * D;

    // LDS as in k_attn_paged: V tiles + staged Q while streaming, the waves'
    // O partials [w][col][OSTR] after it, and the segment's page ids
    constexpr int OSTR = DC * 16 + 4;
    constexpr int VT_BYTES = NWAVES * 4 * GQA_VSTRIDE * (int)sizeof(uint2);
    constexpr int Q_BYTES = 16 * (QW + 8) * (int)sizeof(_Float16);
    constexpr int O_BYTES = NWAVES * 16 * OSTR * (int)sizeof(float);
    constexpr int LDS_BYTES =
        VT_BYTES + Q_BYTES > O_BYTES ? VT_BYTES + Q_BYTES : O_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    __shared__ float lds_m[NWAVES][16];
    __shared__ float lds_l[NWAVES][16];
    __shared__ int lds_pos[16];
    __shared__ int lds_seq[16];         // -1 past T
    extern __shared__ int lds_pg[];     // [npg]
    uint2* vt = reinterpret_cast<uint2*>(lds_raw) + wid * 4 * GQA_VSTRIDE;
    _Float16 (*lds_q)[QW + 8] =
        reinterpret_cast<_Float16 (*)[QW + 8]>(lds_raw + VT_BYTES);
    float* lds_o = reinterpret_cast<float*>(lds_raw);

    if (tid < 16) {
        const bool ok = tid < nq;
        lds_pos[tid] = ok ? pos[t0 + (ok ? tid : 0)] : 0;
        lds_seq[tid] = ok ? seq[t0 + (ok ? tid : 0)] : -1;
    }
    // Q tile -> LDS as f16, prescaled by 1/sqrt(D), zero past D and past T
    // (the factor does the masking)
    {
        const float* qt = q_buf + (size_t)t0 * E + (size_t)h * D;
#pragma unroll
        for (int i = 0; i < 16 * QW / BLOCK; ++i) {
            const int idx = tid + i * BLOCK;
            const int col = idx / QW;
            const int d = idx % QW;
            const bool ok = col < nq && d < D;
            const float v = qt[ok ? (size_t)col * E + d : 0] *
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
    const int pos_q = lds_pos[lq];

    float m = -INFINITY, l = 0.0f;      // running state of column lq
    f32x4 oacc[DC];
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) oacc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

    constexpr int STEP = NWAVES * PAGE_ROWS;
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
        // the segment's page ids: entries 0 .. (J - 1)/16 of the slot's
        // table row. The barrier that ended the previous segment (or the Q
        // staging) lets them be overwritten.
        {
            const int* trow = table + (size_t)sseq * npg;
            const int n = (J + PAGE_ROWS - 1) >> 4;
            for (int i = tid; i < n; i += BLOCK) lds_pg[i] = trow[i];
        }
        gqa_block_sync();
        // k_attn_paged's loop: wave w streams tiles w, w+4, ..., two per
        // iteration in two buffers, loads one tile ahead, a tile's page id in
        // a register before the loads of the tile in front of it are issued;
        // rows at or past J read the slot's row 0 and are above every lim
        int tj = wid * PAGE_ROWS;
        if (tj < J) {                   // wave-uniform, scalar
            const int pg0 = __builtin_amdgcn_readfirstlane(lds_pg[0]);
            GqaTile<NKC> cur, alt;
            int pn = paged_tile_page(lds_pg, tj + STEP, 0, J);
            paged_load_tile(cur, kb, vb, paged_tile_page(lds_pg, tj, 0, J),
                            pg0, tj, J, Ekv, D, lq, lg);
            do {
                const int p2 = paged_tile_page(lds_pg, tj + 2 * STEP, 0, J);
                paged_load_tile(alt, kb, vb, pn, pg0, tj + STEP, J, Ekv, D,
                                lq, lg);
                gqa_tile_step_q<DC, NKC>(cur, qf, vt, tj, lim, lane, m, l,
                                         oacc);
                pn = paged_tile_page(lds_pg, tj + 3 * STEP, 0, J);
                paged_load_tile(cur, kb, vb, p2, pg0, tj + 2 * STEP, J, Ekv,
                                D, lq, lg);
                gqa_tile_step_q<DC, NKC>(alt, qf, vt, tj + STEP, lim, lane, m,
                                         l, oacc);
                tj += 2 * STEP;
            } while (tj < J);
        }
        // page ids are dead; after the last segment so are V tiles and Q
        gqa_block_sync();
        a = b;
    }

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

// ============================================================== launchers

void launch_paged_rows(hipStream_t s, const int* table, const int* pos,
                       const int* seq, int* kv_row, int T, int n_ctx) {
    const int npg = (n_ctx + PAGE_ROWS - 1) / PAGE_ROWS;
    hipLaunchKernelGGL(k_paged_rows, dim3((T + BLOCK - 1) / BLOCK),
                       dim3(BLOCK), 0, s, table, pos, seq, kv_row, T, npg);
}

void launch_attn_paged(hipStream_t s, const float* q_buf,
                       const __half* k_pool_layer,
                       const __half* v_pool_layer, const int* table,
                       float* out, unsigned short* out_prep, const int* pos,
                       const int* seq, int T, int H, int Hkv, int E, int Ekv,
                       int D, int n_ctx, float* ws) {
    const int grp = H / Hkv;
    const int S = attn_paged_splits(n_ctx, T);
    // one split covers the whole context, whatever its length
    const int chunk = (S == 1) ? std::max(n_ctx, PAGED_MIN_CHUNK)
                               : attn_paged_chunk(n_ctx);
    const int npg = (n_ctx + PAGE_ROWS - 1) / PAGE_ROWS;
    const int jtw = jt_width(T);
    const dim3 grid(T, Hkv * ((grp + 15) / 16), S);
    // a block never holds more ids than a table row has
    const size_t lds = sizeof(int) *
        (size_t)std::min(npg, (chunk + PAGE_ROWS - 1) / PAGE_ROWS);
    auto kern = D <= 16 ? k_attn_paged<1> : D <= 32 ? k_attn_paged<2>
              : D <= 64 ? k_attn_paged<4> : k_attn_paged<8>;
    hipLaunchKernelGGL(kern, grid, dim3(BLOCK), lds, s, q_buf, k_pool_layer,
                       v_pool_layer, table, out, out_prep, pos, seq, ws, H,
                       grp, E, Ekv, D, npg, jtw, chunk);
    if (S > 1)
        launch_attn_gqa_merge(s, ws, out, out_prep, pos, T, H, E, D, jtw,
                              chunk, S);
}

void launch_attn_paged_prefill(hipStream_t s, const float* q_buf,
                               const __half* k_pool_layer,
                               const __half* v_pool_layer, const int* table,
                               float* out, unsigned short* out_prep,
                               const int* pos, const int* seq, int T, int H,
                               int Hkv, int E, int Ekv, int D, int n_ctx) {
    const int npg = (n_ctx + PAGE_ROWS - 1) / PAGE_ROWS;
    auto kern = D <= 16 ? k_attn_paged_prefill<1>
              : D <= 32 ? k_attn_paged_prefill<2>
              : D <= 64 ? k_attn_paged_prefill<4> : k_attn_paged_prefill<8>;
    hipLaunchKernelGGL(kern, dim3((T + 15) / 16, H), dim3(BLOCK),
                       sizeof(int) * (size_t)npg, s, q_buf, k_pool_layer,
                       v_pool_layer, table, out, out_prep, pos, seq, T,
                       H / Hkv, E, Ekv, D, npg, jt_width(T));
}
