// Per-token log-probabilities for R entries of a [T, V] f32 logits tensor
// in one launch: the log-softmax value of a chosen id and the top_n most
// likely tokens of its row, so a serving step that reports logprobs never
// copies logits to the host.
//
// Semantics are engine/sampler.py::logprobs_reference: raw logits, full
// vocabulary, no temperature / penalty / filter.
//
// One workgroup per entry, no sort over V and no per-thread candidate
// list. Every pass re-reads the row from global memory with scalar dword
// loads (row bases are only 4-byte aligned when V % 4 != 0); the row stays
// L2-resident for the workgroup's lifetime.
//
//   1. arg-max key                  (block max of ordered_f32 ‖ ~index;
//                                    its value is the row max, and it is
//                                    top-n entry 0)
//   2. sum exp(x - max)             (block sum, fixed shape)
//   3. top_n - 1 further arg-max rounds, each restricted to keys strictly
//      below the previous winner
//
// The key is the one k_argmax_part packs: the order-preserving u32 image
// of the f32 in the high word, the bit-inverted index in the low word, so
// the largest key is the largest logit and, among equal logits, the
// smallest index. Keys are distinct within a row, hence "strictly below
// the previous winner" removes exactly the tokens already reported. -0.0
// is keyed as +0.0 (they compare equal in the reference). The ids involve
// no arithmetic and equal the reference's exactly.
//
// Determinism: each thread sums its strided elements in index order, a
// wave combines its 64 partials with a xor-butterfly (every lane computes
// the same tree: f32 addition is commutative), and every thread adds the
// wave partials from LDS in wave order. No atomics; identical inputs give
// bit-identical lp and top_lp.
#include "kernels.h"
#include "logprobs_key.h"

namespace {

constexpr int LBLOCK = 1024;
constexpr int LWAVES = LBLOCK / 64;

typedef unsigned long long u64;

struct LogprobsSmem {
    u64 wkey[LWAVES];
    float wsum[LWAVES];
};

// the largest key of the row that is < below (0 if there is none)
__device__ u64 logprobs_best(const float* __restrict__ lg, int V, u64 below,
                             LogprobsSmem& sm) {
    const int tid = threadIdx.x;
    u64 best = 0;
    for (int i = tid; i < V; i += LBLOCK) {
        const u64 k = logprobs_key(lg[i], i);
        if (k < below && k > best) best = k;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const u64 o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
    }
    __syncthreads();  // previous readers of wkey are done
    if ((tid & 63) == 0) sm.wkey[tid >> 6] = best;
    __syncthreads();
    best = sm.wkey[0];
    for (int w = 1; w < LWAVES; ++w) {
        const u64 o = sm.wkey[w];
        best = o > best ? o : best;
    }
    return best;
}

__global__ __launch_bounds__(LBLOCK) void k_logprobs(
    const float* __restrict__ logits, const int* __restrict__ rows,
    const int* __restrict__ ids, float* __restrict__ lp,
    int* __restrict__ top_ids, float* __restrict__ top_lp, int T, int V,
    int top_n) {
    __shared__ LogprobsSmem sm;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int row = rows[b];
    const int id = ids[b];
    if (row < 0 || row >= T || id < 0 || id >= V) {
        if (tid == 0) lp[b] = NAN;  // uniform per block: no barrier skipped
        return;
    }
    const float* lg = logits + (size_t)row * V;

    // 1. arg-max key; V >= 1 and keys are non-zero, so there is a winner
    // (0 only if the row is one all-ones NaN at index 0: read index 0)
    u64 win = logprobs_best(lg, V, ~0ull, sm);
    const float m = lg[win ? (int)~(uint32_t)win : 0];

    // 2. log-sum-exp
    float part = 0.0f;
    for (int i = tid; i < V; i += LBLOCK) part += expf(lg[i] - m);
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
    if ((tid & 63) == 0) sm.wsum[tid >> 6] = part;
    __syncthreads();
    float sum = sm.wsum[0];
    for (int w = 1; w < LWAVES; ++w) sum += sm.wsum[w];
    const float lse = m + logf(sum);
    if (tid == 0) lp[b] = lg[id] - lse;

    // 3. top-n: entry 0 is the arg-max, then one round per further entry
    const int n = top_n < V ? top_n : V;
    for (int j = 0; j < n; ++j) {
        if (j) win = logprobs_best(lg, V, win, sm);
        if (tid == 0) {
            const int ti = win ? (int)~(uint32_t)win : -1;
            top_ids[(size_t)b * top_n + j] = ti;
            top_lp[(size_t)b * top_n + j] = ti >= 0 ? lg[ti] - lse : NAN;
        }
    }
}

// ------------------------------------------------------- k_score_finish
// Second half of prompt scoring (first half: k_lmhead_score in
// mfma_gemm.hip). Per token t the lm_head pass left P vocabulary-tile
// partials: the tile's arg-max key pkey[t][p] and psum[t][p] = sum over
// the tile of exp(v - tile max), plus the target's logit tgt_logit[t]
// (written only when the target lies in [0, V)). One wave per token:
//   M, top id  the largest key (value / index it was packed from)
//   S          sum_p psum[p] * exp(m_p - M)
//   lse = M + log S;  lp = tgt_logit - lse (NaN for a target outside the
//   vocabulary), top_lp = M - lse.
// Each lane takes partials p = lane, lane + 64, ... in index order and the
// wave combines with the xor-butterfly of k_logprobs: fixed shape, no
// atomics, bit-identical results for identical partials.
__global__ __launch_bounds__(64) void k_score_finish(
    const u64* __restrict__ pkey, const float* __restrict__ psum,
    const float* __restrict__ tgt_logit, const int* __restrict__ targets,
    float* __restrict__ lp, int* __restrict__ top_id,
    float* __restrict__ top_lp, int P, int V) {
    const int t = blockIdx.x;
    const int lane = threadIdx.x;
    const u64* kt = pkey + (size_t)t * P;
    const float* st = psum + (size_t)t * P;
    u64 best = 0;
    for (int p = lane; p < P; p += 64) {
        const u64 k = kt[p];
        best = k > best ? k : best;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const u64 o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
    }
    const float M = logprobs_key_value(best);
    float part = 0.0f;
    for (int p = lane; p < P; p += 64) {
        const float s = st[p];
        // an all -inf tile has s == 0 and contributes nothing
        if (s > 0.0f) part += s * expf(logprobs_key_value(kt[p]) - M);
    }
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
    if (lane != 0) return;
    const float lse = M + logf(part);
    const int tg = targets[t];
    lp[t] = (tg >= 0 && tg < V) ? tgt_logit[t] - lse : NAN;
    top_id[t] = logprobs_key_index(best);
    top_lp[t] = M - lse;
}

}  // namespace

void launch_score_finish(hipStream_t s, const unsigned long long* pkey,
                         const float* psum, const float* tgt_logit,
                         const int* targets, float* lp, int* top_id,
                         float* top_lp, int T, int P, int V) {
    if (T <= 0 || P <= 0) return;
    hipLaunchKernelGGL(k_score_finish, dim3(T), dim3(64), 0, s, pkey, psum,
                       tgt_logit, targets, lp, top_id, top_lp, P, V);
}

void launch_logprobs(hipStream_t s, const float* logits, const int* rows,
                     const int* ids, float* lp, int* top_ids, float* top_lp,
                     int R, int T, int V, int top_n) {
    if (R <= 0 || V <= 0) return;
    if (top_n < 0) top_n = 0;
    if (top_n > LOGPROBS_MAX_TOP) top_n = LOGPROBS_MAX_TOP;
    hipLaunchKernelGGL(k_logprobs, dim3(R), dim3(LBLOCK), 0, s, logits, rows,
                       ids, lp, top_ids, top_lp, T, V, top_n);
}
