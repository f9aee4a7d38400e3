// Batched on-device sampling: temperature, repetition penalty, top-k,
// top-p and the categorical pick for R rows of a [T, V] f32 logits tensor
// in one launch, so sampled decode never copies logits to the host.
//
// Semantics are engine/sampler.py::sample_reference. The only randomness
// is one host-drawn uniform per row.
//
// One workgroup per row, no sort over V. Every pass re-reads the row from
// global memory (it stays L2-resident for the workgroup's lifetime) and
// recomputes z_i = logit_i / (pen_i * (T + 1e-5)) with the same f32
// expression, so every pass sees bit-identical values.
//
//   1. zmax                         (block max)
//   2. top-k threshold key          (radix descent by COUNT over the
//                                    order-preserving u32 key of z)
//   3. S_k = mass{key >= K_k}       (block sum)
//   4. top-p threshold key          (radix descent by MASS among the
//                                    top-k survivors, target top_p * S_k)
//   5. pick                         (each thread owns a contiguous index
//                                    chunk; block exclusive scan over the
//                                    chunk sums; the owner rescans)
//
// Determinism: a token's mass is exp(z - zmax) scaled by 2^40 and
// truncated to a u64. All sums, histograms and comparisons are integer,
// hence independent of the order in which atomics or reductions land:
// identical inputs give identical ids. 2^17 terms of at most 2^40 cannot
// overflow. A token whose mass truncates to zero (p < 2^-40 of the
// largest) is never returned: the pick only stops on a non-zero mass.
//
// Repetition state is a device bitmap seen[slots][ceil(V/32)]; the kernel
// reads it for the penalty and sets the chosen token's bit (one lane, one
// vector atomic OR), so no id list is uploaded per step.
#include "kernels.h"

namespace {

constexpr int SBLOCK = 1024;
constexpr int SWAVES = SBLOCK / 64;
constexpr float MASS_SCALE = 1099511627776.0f;  // 2^40

typedef unsigned long long u64;

struct SampleSmem {
    u64 hist[256];
    u64 wsum[SWAVES];
    float wmax[SWAVES];
    u64 sel_excl;
    int sel_digit;
    int result;
};

struct SampleRow {
    const float* lg;
    const uint32_t* seen;
    float den, den_pen;  // (T + 1e-5), penalty * (T + 1e-5)
    float zmax;
    int V;
};

__device__ __forceinline__ uint32_t sample_key(float v) {
    union { float f; uint32_t u; } c;
    c.f = v;
    return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}

__device__ __forceinline__ float sample_z(const SampleRow& r, int i) {
    const bool s = (r.seen[i >> 5] >> (i & 31)) & 1u;
    return r.lg[i] / (s ? r.den_pen : r.den);
}

__device__ __forceinline__ u64 sample_mass(const SampleRow& r, float z) {
    float e = expf(z - r.zmax);
    if (!(e >= 0.0f)) e = 0.0f;  // NaN logits carry no mass
    if (e > 1.0f) e = 1.0f;
    return (u64)(e * MASS_SCALE);
}

// exclusive prefix sum of v in thread order; *total = block sum
__device__ u64 sample_scan(u64 v, SampleSmem& sm, u64* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();  // previous readers of wsum are done
    if (lane == 63) sm.wsum[wave] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
    for (int w = 0; w < SWAVES; ++w) {
        const u64 s = sm.wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// The largest key K such that weight{key >= K, key >= kmin} >= target,
// where weight is the element count (by_mass = false) or the fixed-point
// mass. Four 8-bit digits, most significant first; the histogram of each
// level covers the elements that match the digits chosen so far.
__device__ uint32_t sample_select(const SampleRow& r, bool by_mass,
                                  uint32_t kmin, u64 target,
                                  SampleSmem& sm) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0;
    u64 rem = target;
    for (int level = 0; level < 4; ++level) {
        const int shift = 24 - 8 * level;
        const uint32_t pmask =
            level == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
        if (tid < 256) sm.hist[tid] = 0;
        __syncthreads();  // also: the previous level's selection is read
        if (tid == 0) {
            // target beyond the total weight: fall to the lowest digit,
            // which keeps every element
            sm.sel_digit = 0;
            sm.sel_excl = 0;
        }
        for (int i = tid; i < r.V; i += SBLOCK) {
            const float z = sample_z(r, i);
            const uint32_t key = sample_key(z);
            if (((key ^ prefix) & pmask) == 0 && key >= kmin) {
                const u64 w = by_mass ? sample_mass(r, z) : 1ull;
                if (w) atomicAdd(&sm.hist[(key >> shift) & 255], w);
            }
        }
        __syncthreads();
        // scan digits from the top: thread t holds digit 255 - t
        const u64 v = tid < 256 ? sm.hist[255 - tid] : 0;
        u64 tot;
        const u64 excl = sample_scan(v, sm, &tot);
        if (tid < 256 && excl < rem && rem <= excl + v) {
            sm.sel_digit = 255 - tid;
            sm.sel_excl = excl;
        }
        __syncthreads();
        prefix |= (uint32_t)sm.sel_digit << shift;
        rem -= sm.sel_excl;
    }
    return prefix;
}

__global__ __launch_bounds__(SBLOCK) void k_sample(
    const float* __restrict__ logits, const int* __restrict__ rows,
    const int* __restrict__ slots, const float* __restrict__ uni,
    const float* __restrict__ temperature,
    const float* __restrict__ penalty, const int* __restrict__ top_k,
    const float* __restrict__ top_p, uint32_t* __restrict__ seen,
    int* __restrict__ ids, int T, int V, int n_slots, int words) {
    __shared__ SampleSmem sm;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int row = rows[b];
    const int slot = slots[b];
    if (row < 0 || row >= T || slot < 0 || slot >= n_slots) {
        if (tid == 0) ids[b] = -1;  // uniform per block: no barrier skipped
        return;
    }
    SampleRow r;
    r.lg = logits + (size_t)row * V;
    r.seen = seen + (size_t)slot * words;
    r.den = temperature[b] + 1e-5f;
    r.den_pen = penalty[b] * r.den;
    r.V = V;

    // 1. zmax
    float m = -INFINITY;
    for (int i = tid; i < V; i += SBLOCK) m = fmaxf(m, sample_z(r, i));
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if ((tid & 63) == 0) sm.wmax[tid >> 6] = m;
    __syncthreads();
    m = sm.wmax[0];
    for (int w = 1; w < SWAVES; ++w) m = fmaxf(m, sm.wmax[w]);
    r.zmax = m;

    // 2. top-k threshold (0 or >= V: off, every key kept)
    const int k = top_k[b];
    uint32_t kmin = 0;
    if (k > 0 && k < V) kmin = sample_select(r, false, 0u, (u64)k, sm);

    // 3 + 4. top-p threshold among the survivors (>= 1: off)
    const float tp = top_p[b];
    if (tp < 1.0f) {
        u64 part = 0;
        for (int i = tid; i < V; i += SBLOCK) {
            const float z = sample_z(r, i);
            if (sample_key(z) >= kmin) part += sample_mass(r, z);
        }
        u64 sk;
        sample_scan(part, sm, &sk);
        // mass{key >= tau} >= top_p * S_k, at least one unit so the cut
        // always lands on a token with non-zero mass
        const double want = (double)fmaxf(tp, 0.0f) * (double)sk;
        u64 target = (u64)want;
        if ((double)target < want) ++target;
        if (target < 1) target = 1;
        if (target > sk) target = sk;
        const uint32_t tau = sample_select(r, true, kmin, target, sm);
        kmin = tau > kmin ? tau : kmin;
    }

    // 5. pick: first index, in index order, whose cumulative kept mass
    // exceeds u * total
    const int chunk = (V + SBLOCK - 1) / SBLOCK;
    const int c0 = min(V, tid * chunk);
    const int c1 = min(V, c0 + chunk);
    u64 mine = 0;
    for (int i = c0; i < c1; ++i) {
        const float z = sample_z(r, i);
        if (sample_key(z) >= kmin) mine += sample_mass(r, z);
    }
    if (tid == 0) sm.result = -1;
    u64 total;
    const u64 excl = sample_scan(mine, sm, &total);  // orders sm.result
    u64 t = (u64)((double)uni[b] * (double)total);
    if (total && t >= total) t = total - 1;
    if (mine && excl <= t && t < excl + mine) {
        u64 acc = excl;
        for (int i = c0; i < c1; ++i) {
            const float z = sample_z(r, i);
            if (sample_key(z) < kmin) continue;
            const u64 w = sample_mass(r, z);
            if (w && acc + w > t) {
                sm.result = i;
                break;
            }
            acc += w;
        }
    }
    __syncthreads();
    const int found = sm.result;
    __syncthreads();  // everyone has read it before the fallback writes
    if (found < 0) {
        // unreachable for finite logits (t < total by construction);
        // non-finite rows fall back to the last kept token with mass,
        // else to the last index
        int last = -1;
        for (int i = c0; i < c1; ++i) {
            const float z = sample_z(r, i);
            if (sample_key(z) >= kmin && sample_mass(r, z)) last = i;
        }
        if (last >= 0) atomicMax(&sm.result, last);
        __syncthreads();
        if (tid == 0 && sm.result < 0) sm.result = V - 1;
        __syncthreads();
    }
    if (tid == 0) {
        const int id = sm.result;
        ids[b] = id;
        atomicOr(seen + (size_t)slot * words + (id >> 5), 1u << (id & 31));
    }
}

}  // namespace

void launch_sample(hipStream_t s, const float* logits, const int* rows,
                   const int* slots, const float* u,
                   const float* temperature, const float* penalty,
                   const int* top_k, const float* top_p, uint32_t* seen,
                   int* ids, int R, int T, int V, int n_slots) {
    if (R <= 0) return;
    const int words = (V + 31) / 32;
    hipLaunchKernelGGL(k_sample, dim3(R), dim3(SBLOCK), 0, s, logits, rows,
                       slots, u, temperature, penalty, top_k, top_p, seen,
                       ids, T, V, n_slots, words);
}
