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

// x [T, cols] -> f16 xprep panel of width jtw + sumsq (ss zeroed upstream)
void launch_prep_x(hipStream_t s, const float* x, unsigned short* xprep,
                   float* ss, int cols, int T, int jtw);

// T <= 64: slab != nullptr enables the RT=2 + split-K slab path for small
// models; returns 1 when the slab path ran. skip_finish=1 leaves the slabs
// un-combined for a fused-attention consumer (decode only). T > 64 ignores
// slab and skip_finish and returns 0.
int launch_qkv16(hipStream_t s, const WMat2& wq, const WMat2& wk,
                 const WMat2& wv, const unsigned short* xprep,
                 const unsigned short* normprep, const float* ss_in,
                 float eps, float* q_buf, __half* k_cache_layer,
                 __half* v_cache_layer, const int* pos, const int* seq,
                 const float* inv_freq, int E, int Ekv, int D, int n_ctx,
                 int T, float* slab, int skip_finish);

void launch_ffn16(hipStream_t s, const WMat2& w1, const WMat2& w3,
                  const unsigned short* xprep,
                  const unsigned short* normprep, const float* ss_in,
                  float eps, unsigned short* gprep, int T);

// wo / w2: y += w . b, then sumsq of y into ss_out and f16(y) into
// xprep_out. slab (rows/16 * gemm16_ks(rows) * 64 * 16 floats) is touched
// by route 0 only; split_ok = 0 needs none.
void launch_gemm16_residual(hipStream_t s, const WMat2& w,
                            const unsigned short* bprep, float* y,
                            unsigned short* xprep_out, float* ss_out, int T,
                            float* slab, int split_ok);

// lm_head, T <= 64: y = w . rmsnorm(b), plain f32 store
void launch_lmhead(hipStream_t s, const WMat2& w,
                   const unsigned short* bprep,
                   const unsigned short* normprep, const float* ss_in,
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
//                        (whole 4-tile groups at every T); ss zeroed
//                        upstream, ss must hold T rounded up to 64 floats
//   launch_lmhead_score k_lmhead_score: fused final norm + lm_head with a
//                        log-sum-exp epilogue -> P = V / (16 * RT) partials
//                        per token, pkey/psum [T][P], and tgt_logit [T]
//   launch_score_finish  k_score_finish: lp[t], top_id[t], top_lp[t]
// A target outside [0, V) gives lp = NaN; top_id / top_lp are still
// written. RT = lmhead_score_rt(V, T).
int lmhead_score_rt(int V, int T);
int score_jt_width(int T);

void launch_lmhead_score(hipStream_t s, const WMat2& w,
                         const unsigned short* bprep,
                         const unsigned short* normprep, const float* ss_in,
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
