// Launch API of the CDNA4 kernel library: mfma_gemm.hip (MFMA dequant-GEMM
// family), attention.hip, scalar_ops.hip (embed, argmax, legacy f32 path),
// sampling.hip and logprobs.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

// W_Q8B is the BYTE-stream quant path: q8_0 weights re-biased to u8 at
// repack, and q5_0/q5_1/q4_K/q5_K expanded to re-biased bytes — all
// share one kernel form (w = alpha*((1024+u) - 1152) + beta in packed
// f16, (alpha, beta) per 32-weight block). W_Q8B16 is the same byte
// stream with per-16-weight (alpha, beta) planes — the k-quant formats
// whose sub-block scales have 16-weight granularity (q2_K/q3_K/q6_K).
enum WType { W_F32 = 0, W_F16 = 1, W_Q4_0 = 2, W_Q4_1 = 3, W_Q8B = 8,
             W_Q8B16 = 9 };

// One row-major weight matrix resident in HBM, SoA (scalar_ops.hip): the
// embedding table in any of its four types, and the f32 matrices of the
// legacy layer path (the GEMV kernels read `data` as f32 only).
struct WMat {
    const void* data;    // f16/f32 values, or u8 nibbles for q4_*
    const void* scales;  // q4_0: f16[rows][nb]; q4_1: f16[rows][nb*2] (d,m)
    int rows;
    int cols;
    int wtype;  // WType
};

// MFMA-tiled weight matrix (the production path); the layouts are given
// in the mfma_gemm.hip header.
struct WMat2 {
    const void* data;
    const void* scales;
    int rows;
    int cols;
    int wtype;  // WType (W_F32 never appears here — legacy path)
};

// ------------------------------------------------ MFMA layer launchers
// One launcher per layer op, every T. Decode (T <= 64) runs the 1/2/4
// column-tile kernels; large-M (T > 64: prefill and wide decode) covers all
// T tokens in one launch on an XCD-aware (row-tile x 64-token-group) grid:
// k_qkv16<…, true>, k_ffn16<…, true>, k_gemm16_mt. Side channels use the
// jt_width(T) token-panel stride.
int jt_width(int T);

// Route selectors: which instantiation each launcher runs, as plain host
// functions of the matrix and token counts (exported to the tests). No
// launcher branches on anything else.
//   gemm16_plain_rt   launch_lmhead: row tiles per wave, 1 | 2 | 4
//   ffn16_rt          launch_ffn16: 1 | 2
//   gemm16_res_route  launch_gemm16_residual: 0 slab split-K (RT=2) +
//                     reduce/prep pass (T <= 64, split_ok, rows/16 even),
//                     1 fused residual epilogue (T <= 64 otherwise),
//                     2 large-M k_gemm16_mt (T > 64)
//   gemm16_mt_rt      route 2 of the above: 1 | 2
//   qkv16_route       launch_qkv16 (T <= 64): 0 slab split-K (RT=2),
//                     1 fused RT=1, 2 fused RT=2
//   qkv16_mt_rt       launch_qkv16 (T > 64): 1 | 2
int gemm16_plain_rt(int rows);
int ffn16_rt(int rows, int T);
int gemm16_res_route(int rows, int T, int split_ok);
int gemm16_mt_rt(int rows, int T);
int qkv16_route(int E, int Ekv, int T, int has_slab);
int qkv16_mt_rt(int E, int Ekv, int T);

// split-K factors of the slab routes: wo / w2 (shared with the reducer) and
// qkv (shared with the fused-attention consumer)
int gemm16_ks(int rows);
int qkv16_ks(int E, int Ekv);

// RMSNorm over the side channels. The NORM kernels (qkv, ffn, lm_head,
// scoring) read an xprep that already holds f16(x) * norm_w and apply only
// the per-token 1/rms from ss_in. So every producer of an xprep takes
// `normprep`, the padded f16 norm plane (pad_normprep) of the kernel that
// will READ that xprep: launch_prep_x and launch_gemm16_residual below.
// nullptr stores the plain f16(x). The sumsq is always of the f32 x.

// x [T, cols] -> f16 xprep panel of width jtw + sumsq (ss zeroed upstream)
void launch_prep_x(hipStream_t s, const float* x, unsigned short* xprep,
                   float* ss, int cols, int T, int jtw,
                   const unsigned short* normprep);

// T <= 64: slab != nullptr enables the RT=2 + split-K slab path for small
// models; returns 1 when the slab path ran. skip_finish=1 leaves the slabs
// un-combined for a fused-attention consumer (decode only). T > 64 ignores
// slab and skip_finish and returns 0. kv_row = nullptr: token t's K/V row is
// row seq[t] * n_ctx + pos[t] of the layer's caches. Otherwise it is row
// kv_row[t] (device i32 [T], the paged layout's launch_paged_rows); the
// fused-attention consumer knows no kv_row, so skip_finish must be 0 then.
int launch_qkv16(hipStream_t s, const WMat2& wq, const WMat2& wk,
                 const WMat2& wv, const unsigned short* xprep,
                 const float* ss_in, float eps, float* q_buf,
                 __half* k_cache_layer,
                 __half* v_cache_layer, const int* pos, const int* seq,
                 const float* inv_freq, int E, int Ekv, int D, int n_ctx,
                 int T, float* slab, int skip_finish,
                 const int* kv_row = nullptr);

void launch_ffn16(hipStream_t s, const WMat2& w1, const WMat2& w3,
                  const unsigned short* xprep, const float* ss_in,
                  float eps, unsigned short* gprep, int T);

// wo / w2: y += w . b, then sumsq of y into ss_out and f16(y) (times
// normprep, the next NORM kernel's plane, unless nullptr) into xprep_out.
// slab (rows/16 * gemm16_ks(rows) * 64 * 16 floats) is touched by route 0
// only; split_ok = 0 needs none.
void launch_gemm16_residual(hipStream_t s, const WMat2& w,
                            const unsigned short* bprep, float* y,
                            unsigned short* xprep_out, float* ss_out, int T,
                            float* slab, int split_ok,
                            const unsigned short* normprep);

// lm_head, T <= 64: y = w . rmsnorm(b), plain f32 store
void launch_lmhead(hipStream_t s, const WMat2& w,
                   const unsigned short* bprep, const float* ss_in,
                   float eps, float* y, int T);

void launch_rmsnorm(hipStream_t s, const float* x, const float* w, float* y,
                    int T, int E, float eps);

void launch_qkv_rope_append(hipStream_t s, const WMat& wq, const WMat& wk,
                            const WMat& wv, const float* xn, float* q_buf,
                            __half* k_cache_layer, __half* v_cache_layer,
                            const int* pos, const int* seq,
                            const float* inv_freq, int E, int D, int n_ctx,
                            int T);

// qkv_slab != nullptr: decode-fused variant — the attention prologue
// sums the un-combined qkv slabs, applies RoPE and appends the KV row
// (valid only when every token is its own sequence)
void launch_attention(hipStream_t s, const float* q_buf,
                      const __half* k_cache_layer, __half* v_cache_layer,
                      float* out, unsigned short* out_prep, const int* pos,
                      const int* seq, int T, int H, int E, int Ekv, int D,
                      int n_ctx, const float* qkv_slab, int ks,
                      const float* inv_freq);

// ------------------------------------------------ GQA decode attention
// Same semantics as launch_attention without the fused prologue, for
// 2 <= H/Hkv <= 64: one block per (token, KV head, 16 query heads, KV chunk)
// on the matrix cores, every K/V row read once per group. Long contexts are
// cut into attn_gqa_splits chunks of attn_gqa_chunk rows whose partials
// k_attn_gqa_merge combines in fixed order; both are functions of n_ctx
// alone for T <= 64 (a token's bits do not depend on T or on the other
// tokens), and T > 64 runs one split. ws: f32 [64][H][S][D + 2] with
// S = attn_gqa_splits(n_ctx, 1); untouched when S = 1.
//   attn_route   0 launch_attention, 1 launch_attn_prefill (T > 64 and not
//                decode), 2 launch_attn_gqa
int attn_gqa_chunk(int n_ctx);
int attn_gqa_splits(int n_ctx, int T);
int attn_route(int H, int Hkv, int T, int decode, int gqa_attention);

void launch_attn_gqa(hipStream_t s, const float* q_buf,
                     const __half* k_cache_layer,
                     const __half* v_cache_layer, float* out,
                     unsigned short* out_prep, const int* pos,
                     const int* seq, int T, int H, int Hkv, int E, int Ekv,
                     int D, int n_ctx, float* ws);

// k_attn_gqa_merge alone: combines the ceil((pos[t] + 1) / chunk) partials
// (m, l, o[D]) of every (token, head) in ws [T][H][S][D + 2] in split order;
// tokens whose context fits one chunk are left alone. Shared by
// launch_attn_gqa and launch_attn_kv8.
void launch_attn_gqa_merge(hipStream_t s, const float* ws, float* out,
                           unsigned short* out_prep, const int* pos, int T,
                           int H, int E, int D, int jtw, int chunk, int S);

// ------------------------------------------------ int8 KV cache (q8)
// attention_kv8.hip. A cache row of one KV head is D re-biased bytes
// u = q + 128, q in [-127, 127], and one f16 scale s = f16(amax / 127):
// x ~ s * q. K and V caches: u8 [B, n_ctx, Ekv] per layer (+ 16 bytes of
// tail pad on the whole allocation), scales f16 [B, n_ctx, Hkv]. D % 4 == 0.
//   launch_kv8_append  k_kv8_append: quantises the T rows that the qkv
//                      kernels wrote to the f16 stages [B, n_ctx, Ekv] at
//                      (seq[t], pos[t]) into the byte caches and scale
//                      planes; one wave per (token, KV head), K and V in
//                      its two halves
//   launch_attn_kv8    k_attn_kv8 (+ k_attn_gqa_merge): launch_attention's
//                      semantics without the fused prologue, for every
//                      1 <= H/Hkv <= 64 and every T, over the byte caches.
//                      One block per (token, KV head, 16 query heads, KV
//                      chunk) on the matrix cores. Splits follow the GQA
//                      rule (functions of n_ctx alone for T <= 64, one
//                      split for T > 64). ws: f32 [64][H][S][D + 2] with
//                      S = attn_kv8_splits(n_ctx, 1); untouched when S = 1.
//   launch_attn_kv8_prefill  k_attn_kv8_prefill: launch_attn_prefill's
//                      semantics over the byte caches, any T >= 1 and any
//                      1 <= H/Hkv <= 64. One block per (16-query tile, query
//                      head), the tile's queries as the MFMA columns: a K/V
//                      row is read and expanded once per 16 queries.
//                      Mixed-seq tiles segment internally; running max, sum
//                      and V-scale maximum are per query, so a token's bits
//                      do not depend on its tile mates. No split, no ws.
//   attn_kv8_route     which of the two the engine runs: 1 (Q-tiled) iff
//                      T > 64, not decode and kv8_prefill; else 0
//                      (launch_attn_kv8, wide decode included)
int attn_kv8_chunk(int n_ctx);
int attn_kv8_splits(int n_ctx, int T);
int attn_kv8_route(int T, int decode, int kv8_prefill);

void launch_kv8_append(hipStream_t s, const __half* k_stage,
                       const __half* v_stage, uint8_t* k8_layer,
                       uint8_t* v8_layer, __half* k_scale_layer,
                       __half* v_scale_layer, const int* pos, const int* seq,
                       int T, int Hkv, int D, int n_ctx);

void launch_attn_kv8(hipStream_t s, const float* q_buf,
                     const uint8_t* k8_layer, const uint8_t* v8_layer,
                     const __half* k_scale_layer,
                     const __half* v_scale_layer, float* out,
                     unsigned short* out_prep, const int* pos,
                     const int* seq, int T, int H, int Hkv, int E, int Ekv,
                     int D, int n_ctx, float* ws);

void launch_attn_kv8_prefill(hipStream_t s, const float* q_buf,
                             const uint8_t* k8_layer, const uint8_t* v8_layer,
                             const __half* k_scale_layer,
                             const __half* v_scale_layer, float* out,
                             unsigned short* out_prep, const int* pos,
                             const int* seq, int T, int H, int Hkv, int E,
                             int Ekv, int D, int n_ctx);

// Shared-prefix attention over the byte caches (kv8_prefix): the semantics
// and argument contract of launch_attn_prefix below, for 1 <= H/Hkv <= 64.
// Two launches on one stream, any T:
//   k_attn_kv8_prefix       one block per (16-token tile, head, prefix
//                           chunk), the tile's tokens as MFMA columns:
//                           un-normalised partials ws [T][H][S][D + 2]
//   k_attn_kv8_prefix_tail  one block per (token, KV head, 16 query heads):
//                           the own rows [r0, pos[t]] on the matrix cores,
//                           the prefix partials folded in ascending chunk
//                           order, then the four waves; out and out_prep
// attn_kv8_prefix_chunk / _splits follow the GQA rule (functions of n_ctx
// alone for T <= 64, S = 1 for T > 64). ws holds T * H * S * (D + 2) floats.
int attn_kv8_prefix_chunk(int n_ctx);
int attn_kv8_prefix_splits(int n_ctx, int T);

void launch_attn_kv8_prefix(hipStream_t s, const float* q_buf,
                            const uint8_t* k8_layer, const uint8_t* v8_layer,
                            const __half* k_scale_layer,
                            const __half* v_scale_layer, float* out,
                            unsigned short* out_prep, const int* pos,
                            const int* seq, const int* pfx, int pslot, int P,
                            int T, int H, int Hkv, int E, int Ekv, int D,
                            int n_ctx, float* ws);

// ------------------------------------------------ paged KV cache
// attention_paged.hip. A page is kv_page_rows() = 16 rows of Ekv halves (one
// MFMA row tile). K and V pools: f16 [kv_pages * 16, Ekv] per layer (+ 16
// halves of tail pad on the whole allocation). table: device i32
// [slots, ceil(n_ctx / 16)], shared by all layers; row r of slot s is pool
// row table[s][r / 16] * 16 + r % 16. Every entry is a page id in
// [0, kv_pages): page 0 is never assigned and stands for "no page" (written
// and read like any other, its rows only ever masked).
//   launch_paged_rows  k_paged_rows: kv_row[t] = pool row of (seq[t],
//                      pos[t]), the `kv_row` argument of launch_qkv16
//   launch_attn_paged  k_attn_paged (+ k_attn_gqa_merge): launch_attn_kv8's
//                      contract over the f16 pools: every 1 <= H/Hkv <= 64
//                      and every T, one block per (token, KV head, 16 query
//                      heads, KV chunk) on the matrix cores. Token t attends
//                      rows [0, pos[t]] of slot seq[t] through the table.
//                      Splits follow the GQA rule (functions of n_ctx alone
//                      for T <= 64, one split for T > 64): a token's bits do
//                      not depend on T, on the other tokens or on which
//                      pages hold its rows. ws: f32 [64][H][S][D + 2] with
//                      S = attn_paged_splits(n_ctx, 1); untouched when S = 1.
//                      Dynamic LDS holds ceil(chunk / 16) page ids: callers
//                      keep n_ctx <= 65536.
//   launch_attn_paged_prefill  k_attn_paged_prefill: launch_attn_prefill's
//                      semantics over the pools, any T >= 1, 1 <= H/Hkv <= 64,
//                      D even and <= 128. One block per (16-query tile, query
//                      head), the tile's queries as the MFMA columns, so a
//                      K/V row is read once per 16 queries. No split-KV, no
//                      workspace. A token's bits do not depend on its tile
//                      mates, its column, T or which pages hold its rows.
//                      Dynamic LDS holds one table row, ceil(n_ctx / 16)
//                      page ids: callers keep n_ctx <= 65536.
//   attn_paged_route   which of the two the engine runs: 1 (Q-tiled) iff
//                      T > 64, not decode and paged_prefill, else 0.
int kv_page_rows();
int attn_paged_chunk(int n_ctx);
int attn_paged_splits(int n_ctx, int T);
int attn_paged_route(int T, int decode, int paged_prefill);

void launch_paged_rows(hipStream_t s, const int* table, const int* pos,
                       const int* seq, int* kv_row, int T, int n_ctx);

void launch_attn_paged(hipStream_t s, const float* q_buf,
                       const __half* k_pool_layer,
                       const __half* v_pool_layer, const int* table,
                       float* out, unsigned short* out_prep, const int* pos,
                       const int* seq, int T, int H, int Hkv, int E, int Ekv,
                       int D, int n_ctx, float* ws);

void launch_attn_paged_prefill(hipStream_t s, const float* q_buf,
                               const __half* k_pool_layer,
                               const __half* v_pool_layer, const int* table,
                               float* out, unsigned short* out_prep,
                               const int* pos, const int* seq, int T, int H,
                               int Hkv, int E, int Ekv, int D, int n_ctx);

// ------------------------------------------------ shared-prefix attention
// Token t attends rows [0, pfx[t]) of slot `pslot`, then rows
// [pfx[t], pos[t]] of slot seq[t]. pfx is a device i32 [T] whose entries are
// 0 (plain attention over the token's own rows) or P; pos[t] >= pfx[t];
// 0 <= pslot < slots and 1 <= P < n_ctx. Two launches on one stream, any T:
//   k_attn_prefix       one block per (16-token tile, head, prefix chunk) on
//                       the matrix cores, the tile's tokens as MFMA columns:
//                       un-normalised partials ws [T][H][S][D + 2]
//   k_attn_prefix_tail  one block per (token, head): the own rows in f32,
//                       the prefix partials folded in ascending chunk order,
//                       out and the f16 out_prep side channel
// Chunking follows the GQA rule: attn_prefix_chunk rows per split and
// S = attn_prefix_splits splits, functions of n_ctx alone for T <= 64 (a
// token's bits do not depend on T, its tile mates or its column), S = 1 for
// T > 64. ws holds T * H * S * (D + 2) floats.
int attn_prefix_chunk(int n_ctx);
int attn_prefix_splits(int n_ctx, int T);

void launch_attn_prefix(hipStream_t s, const float* q_buf,
                        const __half* k_cache_layer,
                        const __half* v_cache_layer, float* out,
                        unsigned short* out_prep, const int* pos,
                        const int* seq, const int* pfx, int pslot, int P,
                        int T, int H, int Hkv, int E, int Ekv, int D,
                        int n_ctx, float* ws);

void launch_gemv(hipStream_t s, const WMat& w, const float* x,
                 const float* res, float* y, int T);

void launch_ffn_gate(hipStream_t s, const WMat& w1, const WMat& w3,
                     const float* xn, float* g, int T);

void launch_embed(hipStream_t s, const WMat& tab, const int* tokens,
                  float* out, int T, int E);

void launch_argmax(hipStream_t s, const float* logits,
                   unsigned long long* keys, int* out, int T, int V);

// sampling.hip: one workgroup per entry of rows[R] samples logits[rows[r]]
// with that entry's (u, temperature, penalty, top_k, top_p); reads and
// updates the repetition bitmap seen[n_slots][ceil(V/32)] at slots[r]
// (slots distinct within a launch). Out-of-range rows/slots yield id -1.
void launch_sample(hipStream_t s, const float* logits, const int* rows,
                   const int* slots, const float* u,
                   const float* temperature, const float* penalty,
                   const int* top_k, const float* top_p, uint32_t* seen,
                   int* ids, int R, int T, int V, int n_slots);

// logprobs.hip: one workgroup per entry of rows[R] writes the raw
// log-softmax value of token ids[r] in logits[rows[r]] to lp[r], and the
// top_n largest logits of that row (descending, ties to the smaller
// index) as top_ids[r][top_n] / top_lp[r][top_n]. ids is a device array.
// An out-of-range rows[r] or ids[r] yields lp[r] = NaN and no other write.
constexpr int LOGPROBS_MAX_TOP = 8;
void launch_logprobs(hipStream_t s, const float* logits, const int* rows,
                     const int* ids, float* lp, int* top_ids, float* top_lp,
                     int R, int T, int V, int top_n);

// ------------------------------------------------------- prompt scoring
// Log-probability of targets[t] under the lm_head applied to row t of a
// [T, E] activation block, plus the row's arg-max, without ever forming
// [T, V] logits. Three launches on one stream:
//   launch_prep_x        at the scoring panel width score_jt_width(T)
//                        (whole 4-tile groups at every T) with the final
//                        norm plane; ss zeroed upstream, ss must hold T
//                        rounded up to 64 floats
//   launch_lmhead_score k_lmhead_score: fused final norm + lm_head with a
//                        log-sum-exp epilogue -> P = V / (16 * RT) partials
//                        per token, pkey/psum [T][P], and tgt_logit [T]
//   launch_score_finish  k_score_finish: lp[t], top_id[t], top_lp[t]
// A target outside [0, V) gives lp = NaN; top_id / top_lp are still
// written. RT = lmhead_score_rt(V, T).
int lmhead_score_rt(int V, int T);
int score_jt_width(int T);

void launch_lmhead_score(hipStream_t s, const WMat2& w,
                         const unsigned short* bprep, const float* ss_in,
                         float eps, const int* targets,
                         unsigned long long* pkey, float* psum,
                         float* tgt_logit, int T);

void launch_score_finish(hipStream_t s, const unsigned long long* pkey,
                         const float* psum, const float* tgt_logit,
                         const int* targets, float* lp, int* top_id,
                         float* top_lp, int T, int P, int V);

// ---------------------------------------------------- prefill attention
// Q-tiled (16 queries/block) matrix-core flash attention for prefill: each
// K/V row is read once per 16 queries; mixed-seq tiles segment internally.
// Requires D <= 128 (checked by the SliceEngine constructor).
void launch_attn_prefill(hipStream_t s, const float* q_buf,
                         const __half* k_cache_layer,
                         const __half* v_cache_layer, float* out,
                         unsigned short* out_prep, const int* pos,
                         const int* seq, int T, int H, int E, int Ekv,
                         int D, int n_ctx);
