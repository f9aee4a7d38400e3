// Torch-extension binding of the native slice engine.
//
// MI355X-native replacement of the reference's CPython extension `llm.so`
// (/root/reference/distllm/tensor_processor.cpp:2238-2260 exposed 9 functions
// around a global TransformerSlice). This engine instead:
//   * is an explicit object (no global mutable slice, SURVEY.md §5.2 hazard),
//   * keeps weights resident in HBM3E in MFMA-tiled layouts (mfma_gemm.hip),
//   * exchanges activations as torch tensors (DLPack-compatible device
//     buffers), never per-element Python lists,
//   * is stateless w.r.t. generation: positions/sequence ids are explicit
//     device tensors, so the decode step is hipGraph-capturable and the KV
//     "clear_context" is a host-side position reset.
//
// Decode layer = 7-9 kernels depending on model size: QKV (fused, or
// RT=2 slab split-K + rope/cache finish), attention, WO (slab split-K),
// fused reduce+residual+sumsq+xprep, FFN gate (fused SwiGLU), W2 (slab) +
// reduce — RMSNorm rides the sumsq side-channel into the consumers'
// B-fragment builds. f32-weight models (test configs) take a legacy
// scalar path with explicit RMSNorm kernels.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "kernels.h"

namespace {

constexpr int kMaxTokens = 64;  // per-forward token cap (4 MFMA col tiles)

// Tail slack appended to every MFMA-path allocation: the pipelined K loop
// prefetches ONE load batch past its range (mfma_gemm.hip wave_tile_kloop).
// engine/repack.py TAIL_SLACK_* are the Python side of the first four.
constexpr int64_t kTailSlackQ = 256;     // int32 elements (1 KiB)
constexpr int64_t kTailSlackQ8 = 512;    // int32 elements (byte stream)
constexpr int64_t kTailSlackAB = 128;    // f16 elements (256 B)
constexpr int64_t kTailSlackF16 = 2048;  // f16 elements (4 KiB)
constexpr int64_t kTailSlackSide = 8192; // int16 elements (16 KiB)

// Buffer sizing rules of the MFMA path, shared by the engine and the test
// hooks. Side channel [kc][jtw][16][8] f16 for a K dimension of `cols` at
// panel width jtw: the PADDED K-block count (q4 wide-load groups of 4).
int64_t side_numel(int64_t cols, int64_t jtw) {
    return ((cols / 32 + 3) & ~(int64_t)3) * 512 * jtw + kTailSlackSide;
}
// split-K partial slabs f32 [tiles][ks][64][16]; allocations take the
// maximum split of 8
constexpr int64_t kMaxSplit = 8;
int64_t slab_numel(int64_t tiles, int64_t ks = kMaxSplit) {
    return tiles * ks * kMaxTokens * 16;
}
// sumsq channel of a T-token launch: whole 64-token groups
int64_t sumsq_numel(int64_t T) { return (T + 63) & ~(int64_t)63; }

struct DevMat {  // legacy scalar-path matrix (W_F32 models)
    torch::Tensor data, scales;
    WMat w{};
};

struct DevMat2 {  // MFMA-tiled matrix
    torch::Tensor data, scales;
    WMat2 w{};
};

struct Layer {
    torch::Tensor attn_norm, ffn_norm;           // f32 [E] (legacy path)
    torch::Tensor attn_normprep, ffn_normprep;   // f16 [E+pad] (MFMA path)
    // legacy (f32 models)
    DevMat wq, wk, wv, wo, w1, w2, w3;
    // MFMA path
    DevMat2 mq, mk, mv, mo, m1, m2, m3;
    bool mfma = false;
};

DevMat make_devmat_f32(torch::Tensor data, int64_t rows, int64_t cols) {
    TORCH_CHECK(data.is_cuda() && data.is_contiguous() &&
                    data.scalar_type() == torch::kFloat32 &&
                    data.numel() == rows * cols,
                "f32 weight tensor mismatch");
    DevMat m;
    m.data = data;
    m.w = WMat{data.data_ptr(), nullptr, (int)rows, (int)cols, W_F32};
    return m;
}

DevMat2 make_devmat2(torch::Tensor data, torch::Tensor scales, int64_t wtype,
                     int64_t rows, int64_t cols) {
    TORCH_CHECK(data.is_cuda() && data.is_contiguous(),
                "weight data must be contiguous on device");
    TORCH_CHECK(rows % 16 == 0, "rows must be a multiple of 16");
    TORCH_CHECK(cols % 32 == 0, "cols must be a multiple of 32");
    const int64_t R = rows / 16, nb = cols / 32;
    DevMat2 m;
    m.data = data;
    m.w.rows = (int)rows;
    m.w.cols = (int)cols;
    m.w.wtype = (int)wtype;
    m.w.data = data.data_ptr();
    const int64_t nbp = (nb + 3) & ~3;  // K-blocks padded to load groups
    if (wtype == W_Q4_0 || wtype == W_Q4_1) {
        TORCH_CHECK(data.scalar_type() == torch::kInt32 &&
                        data.numel() == R * nbp * 64 + kTailSlackQ,
                    "q4 tiled data must be u32[R][nbp/4][4][16][4] + slack");
        TORCH_CHECK(scales.defined() && scales.is_cuda() &&
                        scales.is_contiguous() &&
                        scales.scalar_type() == torch::kFloat16 &&
                        scales.numel() == R * nbp * 16 * 2 + kTailSlackAB,
                    "q4 tiled scales must be f16 (a,b)[R][nbp/4][16][4] "
                    "+ slack");
        m.scales = scales;
        m.w.scales = scales.data_ptr();
    } else if (wtype == W_Q8B || wtype == W_Q8B16) {
        const int64_t abw = (wtype == W_Q8B16) ? 2 : 1;  // scale planes
        TORCH_CHECK(data.scalar_type() == torch::kInt32 &&
                        data.numel() == R * nbp * 128 + kTailSlackQ8,
                    "byte-quant tiled data must be u32[R][nbp/4][4][16][8]"
                    " + slack");
        TORCH_CHECK(scales.defined() && scales.is_cuda() &&
                        scales.is_contiguous() &&
                        scales.scalar_type() == torch::kFloat16 &&
                        scales.numel() ==
                            R * nbp * 16 * 2 * abw + kTailSlackAB,
                    "byte-quant scales must be f16 (a,b)[R][nbp/4]"
                    "[planes][16][4] + slack");
        m.scales = scales;
        m.w.scales = scales.data_ptr();
    } else {
        TORCH_CHECK(wtype == W_F16, "unsupported tiled wtype");
        TORCH_CHECK(data.scalar_type() == torch::kInt16 ||
                        data.scalar_type() == torch::kHalf,
                    "f16 weights must arrive as f16 tiles");
        TORCH_CHECK(data.numel() == rows * cols + kTailSlackF16,
                    "f16 tile size mismatch (tail slack missing)");
        m.w.scales = nullptr;
    }
    return m;
}

torch::Tensor check_f32(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                    t.scalar_type() == torch::kFloat32,
                name, " must be a contiguous f32 device tensor");
    return t;
}

torch::Tensor check_i32(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                    t.scalar_type() == torch::kInt32,
                name, " must be a contiguous i32 device tensor");
    return t;
}

unsigned short* u16p(torch::Tensor& t) {
    return reinterpret_cast<unsigned short*>(t.data_ptr());
}

// f16 norm-weight side channel, zero-padded to the q4 load-group multiple
torch::Tensor pad_normprep(const torch::Tensor& w) {
    auto h = w.to(torch::kHalf).contiguous();
    const int64_t n = h.numel();
    // group-pad plus one prefetch batch of slack (4 groups x 32 shorts)
    const int64_t padded = ((n / 32 + 3) & ~(int64_t)3) * 32 + 128;
    return torch::constant_pad_nd(h, {0, padded - n}, 0).contiguous();
}

class SliceEngine {
 public:
    SliceEngine(int64_t n_embd, int64_t n_head, int64_t n_layers,
                int64_t n_ff, int64_t n_ctx, int64_t max_batch, double eps,
                double rope_base, int64_t max_prefill = 1024,
                int64_t n_head_kv = 0)
        : E_((int)n_embd),
          H_((int)n_head),
          D_((int)(n_embd / n_head)),
          F_((int)n_ff),
          L_((int)n_layers),
          ctx_((int)n_ctx),
          B_((int)max_batch),
          eps_((float)eps) {
        TORCH_CHECK(E_ % H_ == 0, "n_embd not divisible by n_head");
        TORCH_CHECK(D_ % 2 == 0, "head_dim must be even for RoPE pairs");
        TORCH_CHECK(D_ <= 128, "head_dim > 128 unsupported (the "
                    "attention kernels cover d < 128 per lane pair)");
        TORCH_CHECK(E_ % 16 == 0 && F_ % 16 == 0, "E/F must be 16-aligned");
        // GQA: n_head_kv query-head groups share each KV head
        HK_ = (n_head_kv > 0) ? (int)n_head_kv : H_;
        TORCH_CHECK(H_ % HK_ == 0, "n_head not divisible by n_head_kv");
        EK_ = HK_ * D_;
        TORCH_CHECK(EK_ % 16 == 0, "kv width must be 16-aligned");
        // prefill token cap per forward call: side channels and q/attn
        // buffers scale with it (a few hundred MB at 2048 on 65B shapes)
        maxP_ = std::max((int)max_prefill, kMaxTokens);
        ssw_ = maxP_;  // per-layer stride of the sumsq side channels
        layers_.resize(L_);
        loaded_.assign(L_, false);
        auto dev = torch::TensorOptions().device(torch::kCUDA);
        auto f32 = dev.dtype(torch::kFloat32);
        auto f16 = dev.dtype(torch::kFloat16);
        auto u16 = dev.dtype(torch::kInt16);
        // KV cache: [L, B, ctx, Ekv] f16 — the HBM3E-resident analog of
        // the reference's kv_cache_init (tensor_processor.cpp:1089-1132);
        // Ekv = Hkv*D < E under GQA. 16 halves of tail pad let the
        // attention kernels read whole 16 B octets unconditionally at
        // the last row (no divergent tail-load branches).
        const int64_t kv_elems = (int64_t)L_ * B_ * ctx_ * EK_;
        kv_store_k_ = torch::zeros({kv_elems + 16}, f16);
        kv_store_v_ = torch::zeros({kv_elems + 16}, f16);
        k_cache_ = kv_store_k_.narrow(0, 0, kv_elems)
                       .view({L_, B_, ctx_, EK_});
        v_cache_ = kv_store_v_.narrow(0, 0, kv_elems)
                       .view({L_, B_, ctx_, EK_});
        // RoPE pair frequencies: theta_i = pos * base^(-2i/D)
        inv_freq_ = torch::pow(
            (float)rope_base,
            torch::arange(0, D_ / 2, f32) * (-2.0f / (float)D_))
            .contiguous();
        xn_ = torch::empty({kMaxTokens, E_}, f32);
        qb_ = torch::empty({maxP_, E_}, f32);
        ab_ = torch::empty({maxP_, E_}, f32);
        ffb_ = torch::empty({kMaxTokens, F_}, f32);
        // MFMA-path side channels (side_numel), zero-filled: the pad
        // region is consumed by alpha=0 weight blocks but must hold finite
        // f16 values. Token-panel width = jt_width(maxP_) 16-token tiles —
        // the decode path uses the first 4 tiles of the same buffers
        const int64_t jtwp = jt_width(maxP_);
        xprep_ = torch::zeros({side_numel(E_, jtwp)}, u16);
        aprep_ = torch::zeros({side_numel(E_, jtwp)}, u16);
        gprep_ = torch::zeros({side_numel(F_, jtwp)}, u16);
        ss_attn_ = torch::zeros({(int64_t)(L_ + 1) * ssw_}, f32);
        ss_ffn_ = torch::zeros({(int64_t)L_ * ssw_}, f32);
        ss_tmp_ = torch::zeros({sumsq_numel(kMaxTokens)}, f32);
        argmax_keys_ = torch::zeros({maxP_}, dev.dtype(torch::kInt64));
        // split-K partial slabs: sized for the largest user — qkv
        // (3E/16 tiles), ffn (2F/16), wo/w2 (E/16)
        slab_ = torch::zeros({slab_numel(std::max<int64_t>(
            {3 * (E_ / 16), 2 * (F_ / 16), E_ / 16}))}, f32);
    }

    void set_layer(int64_t li, torch::Tensor attn_norm,
                   torch::Tensor ffn_norm, py::list mats) {
        TORCH_CHECK(li >= 0 && li < L_, "layer index out of range");
        TORCH_CHECK(mats.size() == 7, "expected 7 matrices (q,k,v,o,1,2,3)");
        Layer& l = layers_[li];
        l.attn_norm = check_f32(attn_norm, "attn_norm");
        l.ffn_norm = check_f32(ffn_norm, "ffn_norm");
        l.attn_normprep = pad_normprep(attn_norm);
        l.ffn_normprep = pad_normprep(ffn_norm);
        const int64_t rows[7] = {E_, EK_, EK_, E_, F_, E_, F_};
        const int64_t cols[7] = {E_, E_, E_, E_, E_, F_, E_};
        auto first = mats[0].cast<py::tuple>();
        const int64_t wt0 = first[2].cast<int64_t>();
        l.mfma = (wt0 != W_F32);
        TORCH_CHECK(l.mfma || EK_ == E_,
                    "the legacy f32 path does not support GQA");
        DevMat* slots[7] = {&l.wq, &l.wk, &l.wv, &l.wo, &l.w1, &l.w2, &l.w3};
        DevMat2* slots2[7] = {&l.mq, &l.mk, &l.mv, &l.mo, &l.m1, &l.m2,
                              &l.m3};
        for (size_t i = 0; i < 7; ++i) {
            auto tup = mats[i].cast<py::tuple>();
            const int64_t wt = tup[2].cast<int64_t>();
            TORCH_CHECK((wt == W_F32) == !l.mfma,
                        "all matrices of a layer must share the path");
            if (l.mfma)
                *slots2[i] = make_devmat2(tup[0].cast<torch::Tensor>(),
                                          tup[1].cast<torch::Tensor>(), wt,
                                          rows[i], cols[i]);
            else
                *slots[i] = make_devmat_f32(tup[0].cast<torch::Tensor>(),
                                            rows[i], cols[i]);
        }
        loaded_[li] = true;
    }

    void set_extra(torch::Tensor tok_data, torch::Tensor tok_scales,
                   int64_t tok_wtype, torch::Tensor norm_w,
                   torch::Tensor out_data, torch::Tensor out_scales,
                   int64_t out_wtype, int64_t n_vocab) {
        V_ = (int)n_vocab;
        final_norm_ = check_f32(norm_w, "norm_w");
        final_normprep_ = pad_normprep(norm_w);
        // the embedding table always arrives in the legacy SoA layout
        // (gather kernel), the lm_head in the layout its path needs
        tok_ = DevMat{};
        tok_.data = tok_data;
        tok_.w.rows = V_;
        tok_.w.cols = E_;
        tok_.w.wtype = (int)tok_wtype;
        tok_.w.data = tok_data.data_ptr();
        if (tok_wtype == W_Q4_0 || tok_wtype == W_Q4_1) {
            tok_.scales = tok_scales;
            tok_.w.scales = tok_scales.data_ptr();
        }
        out_mfma_ = (out_wtype != W_F32);
        if (out_mfma_)
            mout_ = make_devmat2(out_data, out_scales, out_wtype, V_, E_);
        else
            out_ = make_devmat_f32(out_data, V_, E_);
        has_extra_ = true;
    }

    // x: [T, E] f32 (modified in place and returned), pos/seq: [T] i32.
    // decode=true asserts every token is a distinct sequence (batched
    // decode), enabling the qkv-slab + fused-attention path.
    torch::Tensor forward(torch::Tensor x, torch::Tensor pos,
                          torch::Tensor seq, bool decode = false) {
        check_f32(x, "x");
        check_i32(pos, "pos");
        check_i32(seq, "seq");
        const int T = (int)x.size(0);
        TORCH_CHECK(x.dim() == 2 && x.size(1) == E_, "x must be [T, E]");
        const bool mfma = layers_.empty() ? false : layers_[0].mfma;
        const int tcap = mfma ? maxP_ : kMaxTokens;
        TORCH_CHECK(T >= 1 && T <= tcap,
                    "forward handles at most ", tcap,
                    " tokens per call; tile larger batches host-side");
        TORCH_CHECK(pos.numel() == T && seq.numel() == T, "pos/seq size");
        // Opt-in backstop against out-of-bounds KV writes (an oversized
        // request that slipped past host-side validation). Costs a host
        // sync per forward and is illegal under graph capture, so it is
        // env-gated rather than always-on.
        static const bool bounds_check = [] {
            const char* v = std::getenv("DLLM_BOUNDS_CHECK");
            return v && v[0] == '1';
        }();
        if (bounds_check) {
            const int64_t pmax = pos.max().item<int64_t>();
            const int64_t smax = seq.max().item<int64_t>();
            TORCH_CHECK(pmax < ctx_, "position ", pmax, " >= n_ctx ", ctx_);
            TORCH_CHECK(smax < B_, "sequence id ", smax, " >= max_batch ",
                        B_);
        }
        for (int li = 0; li < L_; ++li)
            TORCH_CHECK(loaded_[li], "layer ", li, " not loaded");
        hipStream_t s = c10::hip::getCurrentHIPStream().stream();
        float* xp = x.data_ptr<float>();
        const int* pp = pos.data_ptr<int>();
        const int* sp = seq.data_ptr<int>();
        const size_t layer_stride = (size_t)B_ * ctx_ * EK_;
        __half* kbase = reinterpret_cast<__half*>(k_cache_.data_ptr());
        __half* vbase = reinterpret_cast<__half*>(v_cache_.data_ptr());
        const float* ifr = inv_freq_.data_ptr<float>();
        float* qb = qb_.data_ptr<float>();
        float* ab = ab_.data_ptr<float>();

        if (!layers_[0].mfma) {
            forward_legacy(s, xp, pp, sp, T, kbase, vbase, ifr, layer_stride);
            return x;
        }
        unsigned short* xprep = u16p(xprep_);
        unsigned short* aprep = u16p(aprep_);
        unsigned short* gprep = u16p(gprep_);
        float* ssa = ss_attn_.data_ptr<float>();
        float* ssf = ss_ffn_.data_ptr<float>();
        // zero the atomic sumsq slots, then stage x into the side channel
        (void)hipMemsetAsync(ssa, 0, sizeof(float) * (L_ + 1) * ssw_, s);
        (void)hipMemsetAsync(ssf, 0, sizeof(float) * L_ * ssw_, s);
        launch_prep_x(s, xp, xprep, ssa, E_, T, jt_width(T));
        // One layer loop for every T, sequenced here in C++ — no host
        // tiling, no library GEMMs, q4 tiles read directly. The launchers
        // pick decode or large-M kernels by T; large-M (more than 64 tokens)
        // serves BOTH prompt prefill and wide batched decode (decode=true:
        // every token its own sequence — weights and dequant are paid
        // ONCE for the whole batch instead of once per 64-token lane).
        static const bool split_ok = !std::getenv("DLLM_NO_SPLITK");
        // per-launch error probe; must not be set under graph capture
        // (it synchronizes the stream)
        static const bool dbg_sync = [] {
            const char* v = std::getenv("DLLM_DEBUG_SYNC");
            return v && v[0] == '1';
        }();
        auto ck = [&](const char* what, int li) {
            if (!dbg_sync) return;
            hipError_t e = hipStreamSynchronize(s);
            fprintf(stderr, "[dbg] L%d %s: %s\n", li, what,
                    hipGetErrorString(e));
        };
        float* slab = slab_.data_ptr<float>();
        for (int li = 0; li < L_; ++li) {
            Layer& l = layers_[li];
            __half* kc = kbase + (size_t)li * layer_stride;
            __half* vc = vbase + (size_t)li * layer_stride;
            const int slab_used = launch_qkv16(
                s, l.mq.w, l.mk.w, l.mv.w, xprep, u16p(l.attn_normprep),
                ssa + li * ssw_, eps_, qb, kc, vc, pp, sp, ifr, E_, EK_,
                D_, ctx_, T, slab, /*skip_finish=*/decode ? 1 : 0);
            ck("qkv", li);
            // 16-query tiles are spans for prefill; the distinct-sequence
            // decode shape streams per token at any T, fused with the
            // un-combined qkv slabs when the slab route ran
            if (T > kMaxTokens && !decode) {
                launch_attn_prefill(s, qb, kc, vc, ab, aprep, pp, sp, T, H_,
                                    E_, EK_, D_, ctx_);
            } else {
                const bool fuse = decode && slab_used;
                launch_attention(s, qb, kc, vc, ab, aprep, pp, sp, T, H_,
                                 E_, EK_, D_, ctx_, fuse ? slab : nullptr,
                                 fuse ? qkv16_ks(E_, EK_) : 0, ifr);
            }
            ck("attn", li);
            launch_gemm16_residual(s, l.mo.w, aprep, xp, xprep,
                                   ssf + li * ssw_, T, slab, split_ok);
            ck("wo", li);
            launch_ffn16(s, l.m1.w, l.m3.w, xprep, u16p(l.ffn_normprep),
                         ssf + li * ssw_, eps_, gprep, T);
            ck("ffn", li);
            launch_gemm16_residual(s, l.m2.w, gprep, xp, xprep,
                                   ssa + (li + 1) * ssw_, T, slab, split_ok);
            ck("w2", li);
        }
        return x;
    }

    torch::Tensor embed(torch::Tensor tokens) {
        TORCH_CHECK(has_extra_, "extra layers not loaded");
        check_i32(tokens, "tokens");
        const int T = (int)tokens.numel();
        auto out = torch::empty(
            {T, E_},
            torch::TensorOptions().device(torch::kCUDA).dtype(torch::kFloat32));
        hipStream_t s = c10::hip::getCurrentHIPStream().stream();
        launch_embed(s, tok_.w, tokens.data_ptr<int>(),
                     out.data_ptr<float>(), T, E_);
        return out;
    }

    // Final RMSNorm + lm_head (reference: get_llm_output,
    // tensor_processor.cpp:1787-1892). all_logits=false returns only the
    // last row's logits.
    torch::Tensor logits(torch::Tensor x, bool all_logits) {
        TORCH_CHECK(has_extra_, "extra layers not loaded");
        check_f32(x, "x");
        TORCH_CHECK(x.dim() == 2 && x.size(1) == E_, "x must be [T, E]");
        torch::Tensor xin = all_logits ? x : x.slice(0, x.size(0) - 1);
        xin = xin.contiguous();
        const int T = (int)xin.size(0);
        TORCH_CHECK(T <= kMaxTokens, "logits: too many rows per call");
        hipStream_t s = c10::hip::getCurrentHIPStream().stream();
        auto lg = torch::empty(
            {T, V_},
            torch::TensorOptions().device(torch::kCUDA).dtype(torch::kFloat32));
        if (out_mfma_) {
            (void)hipMemsetAsync(ss_tmp_.data_ptr(), 0, sizeof(float) * T, s);
            launch_prep_x(s, xin.data_ptr<float>(), u16p(xprep_),
                          ss_tmp_.data_ptr<float>(), E_, T, jt_width(T));
            launch_lmhead(s, mout_.w, u16p(xprep_), u16p(final_normprep_),
                          ss_tmp_.data_ptr<float>(), eps_,
                          lg.data_ptr<float>(), T);
        } else {
            launch_rmsnorm(s, xin.data_ptr<float>(),
                           final_norm_.data_ptr<float>(),
                           xn_.data_ptr<float>(), T, E_, eps_);
            launch_gemv(s, out_.w, xn_.data_ptr<float>(), nullptr,
                        lg.data_ptr<float>(), T);
        }
        return lg;
    }

    torch::Tensor argmax(torch::Tensor lg) {
        check_f32(lg, "logits");
        const int T = (int)lg.size(0);
        auto out = torch::empty(
            {T},
            torch::TensorOptions().device(torch::kCUDA).dtype(torch::kInt32));
        TORCH_CHECK(T <= maxP_, "argmax: too many rows");
        hipStream_t s = c10::hip::getCurrentHIPStream().stream();
        launch_argmax(
            s, lg.data_ptr<float>(),
            reinterpret_cast<unsigned long long*>(argmax_keys_.data_ptr()),
            out.data_ptr<int>(), T, (int)lg.size(1));
        return out;
    }

    // Batched sampling of R rows of lg in one launch (sampling.hip).
    // params is one packed i32 [7, R] device tensor — rows, slots,
    // u, temperature, penalty (f32 bits), top_k, top_p (f32 bits) — so a
    // step costs one upload; seen is the [slots, ceil(V/32)] repetition
    // bitmap (i32 storage), updated in place. row_max/slot_max are the
    // host-side maxima of params[0]/params[1] (the values themselves live
    // on the device; the kernel additionally refuses out-of-range ones).
    torch::Tensor sample(torch::Tensor lg, torch::Tensor params,
                         torch::Tensor seen, int64_t row_max,
                         int64_t slot_max) {
        check_f32(lg, "logits");
        check_i32(params, "params");
        check_i32(seen, "seen");
        TORCH_CHECK(lg.dim() == 2, "sample: logits must be [T, V]");
        const int T = (int)lg.size(0);
        const int V = (int)lg.size(1);
        TORCH_CHECK(params.dim() == 2 && params.size(0) == 7,
                    "sample: params must be [7, R]");
        const int R = (int)params.size(1);
        TORCH_CHECK(R >= 1 && R <= maxP_, "sample: too many rows");
        TORCH_CHECK(seen.dim() == 2 && seen.size(1) == (V + 31) / 32,
                    "sample: seen must be [slots, ceil(V/32)]");
        TORCH_CHECK(row_max >= 0 && row_max < T,
                    "sample: row index out of range");
        TORCH_CHECK(slot_max >= 0 && slot_max < seen.size(0),
                    "sample: slot index out of range");
        auto out = torch::empty(
            {R},
            torch::TensorOptions().device(torch::kCUDA).dtype(torch::kInt32));
        hipStream_t s = c10::hip::getCurrentHIPStream().stream();
        const int* p = params.data_ptr<int>();
        const float* pf = reinterpret_cast<const float*>(p);
        launch_sample(s, lg.data_ptr<float>(), p, p + R, pf + 2 * R,
                      pf + 3 * R, pf + 4 * R, p + 5 * R, pf + 6 * R,
                      reinterpret_cast<uint32_t*>(seen.data_ptr<int>()),
                      out.data_ptr<int>(), R, T, V, (int)seen.size(0));
        return out;
    }

    // Log-probabilities of R chosen tokens in one launch (logprobs.hip).
    // rows is a device i32 [R] tensor uploaded by the caller (row_max is
    // its host-side maximum), ids a device i32 [R] tensor that may come
    // straight from argmax/sample. Returns (lp [R] f32, top_ids
    // [R, top_n] i32, top_lp [R, top_n] f32).
    std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> logprobs(
        torch::Tensor lg, torch::Tensor rows, torch::Tensor ids,
        int64_t top_n, int64_t row_max) {
        check_f32(lg, "logits");
        check_i32(rows, "rows");
        check_i32(ids, "ids");
        TORCH_CHECK(lg.dim() == 2, "logprobs: logits must be [T, V]");
        const int T = (int)lg.size(0);
        const int V = (int)lg.size(1);
        TORCH_CHECK(rows.dim() == 1 && ids.dim() == 1 &&
                        rows.size(0) == ids.size(0) && rows.size(0) >= 1,
                    "logprobs: rows and ids must be [R], R >= 1");
        const int R = (int)rows.size(0);
        TORCH_CHECK(top_n >= 0 && top_n <= LOGPROBS_MAX_TOP && top_n <= V,
                    "logprobs: top_n out of range");
        TORCH_CHECK(row_max >= 0 && row_max < T,
                    "logprobs: row index out of range");
        auto f32 = torch::TensorOptions().device(torch::kCUDA).dtype(
            torch::kFloat32);
        auto lp = torch::empty({R}, f32);
        auto top_lp = torch::empty({R, top_n}, f32);
        auto top_ids = torch::empty({R, top_n}, f32.dtype(torch::kInt32));
        hipStream_t s = c10::hip::getCurrentHIPStream().stream();
        launch_logprobs(s, lg.data_ptr<float>(), rows.data_ptr<int>(),
                        ids.data_ptr<int>(), lp.data_ptr<float>(),
                        top_ids.data_ptr<int>(), top_lp.data_ptr<float>(), R,
                        T, V, (int)top_n);
        return {lp, top_ids, top_lp};
    }

    // Prompt scoring: log-probability of targets[t] under final norm +
    // lm_head of row t, and the row's arg-max, with no [T, V] logits (the
    // kernels.h "prompt scoring" sequence, all on the current stream). x is
    // [T, E] f32 with T <= max_prefill, targets a device i32 [T]; a target
    // outside [0, V) marks "no target": lp NaN, top still written. Returns
    // (lp [T] f32, top_id [T] i32, top_lp [T] f32).
    std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> score(
        torch::Tensor x, torch::Tensor targets) {
        TORCH_CHECK(has_extra_, "extra layers not loaded");
        TORCH_CHECK(out_mfma_, "score: the lm_head is not on the MFMA path");
        check_f32(x, "x");
        check_i32(targets, "targets");
        TORCH_CHECK(x.dim() == 2 && x.size(1) == E_, "x must be [T, E]");
        const int T = (int)x.size(0);
        TORCH_CHECK(T >= 1 && T <= maxP_, "score handles at most ", maxP_,
                    " rows per call; tile larger inputs host-side");
        TORCH_CHECK(targets.dim() == 1 && targets.size(0) == T,
                    "score: targets must be [T]");
        auto dev = torch::TensorOptions().device(torch::kCUDA);
        auto f32 = dev.dtype(torch::kFloat32);
        if (!score_key_.defined()) {
            // first use: engines that never score allocate nothing. The
            // partial count is largest where RT is smallest, at T = 1.
            const int64_t pmax = V_ / (16 * lmhead_score_rt(V_, 1));
            ss_score_ = torch::zeros({sumsq_numel(maxP_)}, f32);
            score_key_ = torch::zeros({(int64_t)maxP_ * pmax},
                                      dev.dtype(torch::kInt64));
            score_sum_ = torch::zeros({(int64_t)maxP_ * pmax}, f32);
            score_tgt_ = torch::zeros({(int64_t)maxP_}, f32);
        }
        const int P = V_ / (16 * lmhead_score_rt(V_, T));
        TORCH_CHECK((int64_t)T * P <= score_key_.numel(),
                    "score: partials buffer too small");
        auto lp = torch::empty({T}, f32);
        auto top_lp = torch::empty({T}, f32);
        auto top_id = torch::empty({T}, dev.dtype(torch::kInt32));
        hipStream_t s = c10::hip::getCurrentHIPStream().stream();
        float* ss = ss_score_.data_ptr<float>();
        auto* pkey =
            reinterpret_cast<unsigned long long*>(score_key_.data_ptr());
        (void)hipMemsetAsync(ss, 0, sizeof(float) * ss_score_.numel(), s);
        launch_prep_x(s, x.data_ptr<float>(), u16p(xprep_), ss, E_, T,
                      score_jt_width(T));
        launch_lmhead_score(s, mout_.w, u16p(xprep_), u16p(final_normprep_),
                            ss, eps_, targets.data_ptr<int>(), pkey,
                            score_sum_.data_ptr<float>(),
                            score_tgt_.data_ptr<float>(), T);
        launch_score_finish(s, pkey, score_sum_.data_ptr<float>(),
                            score_tgt_.data_ptr<float>(),
                            targets.data_ptr<int>(), lp.data_ptr<float>(),
                            top_id.data_ptr<int>(), top_lp.data_ptr<float>(),
                            T, P, V_);
        return {lp, top_id, top_lp};
    }

    bool out_mfma() const { return out_mfma_; }

    int64_t max_tokens() const { return kMaxTokens; }
    int64_t max_prefill() const { return maxP_; }
    int64_t n_ctx() const { return ctx_; }
    int64_t max_batch() const { return B_; }
    // the per-layer KV tensors ([L, B, ctx, E] f16)
    torch::Tensor k_cache() const { return k_cache_; }
    torch::Tensor v_cache() const { return v_cache_; }

 private:
    void forward_legacy(hipStream_t s, float* xp, const int* pp,
                        const int* sp, int T, __half* kbase, __half* vbase,
                        const float* ifr, size_t layer_stride) {
        float* xn = xn_.data_ptr<float>();
        float* qb = qb_.data_ptr<float>();
        float* ab = ab_.data_ptr<float>();
        float* ffb = ffb_.data_ptr<float>();
        for (int li = 0; li < L_; ++li) {
            Layer& l = layers_[li];
            __half* kc = kbase + (size_t)li * layer_stride;
            __half* vc = vbase + (size_t)li * layer_stride;
            launch_rmsnorm(s, xp, l.attn_norm.data_ptr<float>(), xn, T, E_,
                           eps_);
            launch_qkv_rope_append(s, l.wq.w, l.wk.w, l.wv.w, xn, qb, kc, vc,
                                   pp, sp, ifr, E_, D_, ctx_, T);
            launch_attention(s, qb, kc, vc, ab, nullptr, pp, sp, T, H_, E_,
                             EK_, D_, ctx_, nullptr, 0, ifr);
            launch_gemv(s, l.wo.w, ab, /*res=*/xp, xp, T);
            launch_rmsnorm(s, xp, l.ffn_norm.data_ptr<float>(), xn, T, E_,
                           eps_);
            launch_ffn_gate(s, l.w1.w, l.w3.w, xn, ffb, T);
            launch_gemv(s, l.w2.w, ffb, /*res=*/xp, xp, T);
        }
    }

    int E_, H_, D_, F_, L_, ctx_, B_;
    int HK_ = 0, EK_ = 0;    // GQA kv heads / kv projection width
    int maxP_ = kMaxTokens;  // prefill token cap per forward call
    int ssw_ = kMaxTokens;   // per-layer sumsq side-channel stride
    int V_ = 0;
    float eps_;
    std::vector<Layer> layers_;
    std::vector<bool> loaded_;
    torch::Tensor kv_store_k_, kv_store_v_;
    torch::Tensor k_cache_, v_cache_, inv_freq_;
    torch::Tensor xn_, qb_, ab_, ffb_;
    torch::Tensor xprep_, aprep_, gprep_, ss_attn_, ss_ffn_, ss_tmp_;
    torch::Tensor argmax_keys_, slab_;
    // prompt scoring, allocated by the first score() call
    torch::Tensor ss_score_, score_key_, score_sum_, score_tgt_;
    bool has_extra_ = false;
    bool out_mfma_ = false;
    DevMat tok_, out_;
    DevMat2 mout_;
    torch::Tensor final_norm_, final_normprep_;
};

// ------------------------------------------------------------ test hooks
// Direct entry points to the attention launchers for tests/
// test_gpu_attention.py. NOT serving API: they allocate per call, sync the
// host to validate pos/seq, and exist so each kernel can be compared with
// a float64 reference on its own. Every argument that could send a kernel
// out of bounds is refused here.

struct AttnDims {
    int T, H, Hkv, D, E, Ekv, ctx, slots;
};

torch::Tensor check_f16_store(const torch::Tensor& t, const AttnDims& d,
                              const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 1 &&
                    t.scalar_type() == torch::kFloat16,
                name, " must be a flat contiguous f16 device tensor");
    // the engine's own allocation rule: the 16-half pad is mandatory
    // (load_voct reads whole octets past the last head)
    TORCH_CHECK(t.numel() == (int64_t)d.slots * d.ctx * d.Ekv + 16, name,
                " must hold exactly n_slots*n_ctx*Ekv + 16 halves");
    return t;
}

AttnDims check_attn_args(int64_t T, int64_t n_head, int64_t n_head_kv,
                         int64_t head_dim, int64_t n_ctx, int64_t n_slots,
                         const torch::Tensor& k_store,
                         const torch::Tensor& v_store,
                         const torch::Tensor& pos,
                         const torch::Tensor& seq) {
    TORCH_CHECK(T >= 1 && T <= 4096, "token count out of range");
    TORCH_CHECK(n_head >= 1 && n_head_kv >= 1 && n_head <= 1024 &&
                    n_head % n_head_kv == 0,
                "n_head must be a positive multiple of n_head_kv");
    TORCH_CHECK(head_dim >= 2 && head_dim % 2 == 0 && head_dim <= 128,
                "head_dim must be even and <= 128");
    TORCH_CHECK(n_ctx >= 1 && n_slots >= 1 &&
                    n_ctx * n_slots <= ((int64_t)1 << 24),
                "n_ctx/n_slots out of range");
    AttnDims d;
    d.T = (int)T;
    d.H = (int)n_head;
    d.Hkv = (int)n_head_kv;
    d.D = (int)head_dim;
    d.E = d.H * d.D;
    d.Ekv = d.Hkv * d.D;
    d.ctx = (int)n_ctx;
    d.slots = (int)n_slots;
    TORCH_CHECK(d.E % 16 == 0 && d.Ekv % 16 == 0,
                "E and Ekv must be multiples of 16");
    check_f16_store(k_store, d, "k_store");
    check_f16_store(v_store, d, "v_store");
    check_i32(pos, "pos");
    check_i32(seq, "seq");
    TORCH_CHECK(pos.dim() == 1 && seq.dim() == 1 && pos.numel() == T &&
                    seq.numel() == T,
                "pos and seq must be [T]");
    // host-side range check (a sync is fine in a test hook)
    TORCH_CHECK(pos.min().item<int64_t>() >= 0 &&
                    pos.max().item<int64_t>() < n_ctx,
                "pos out of [0, n_ctx)");
    TORCH_CHECK(seq.min().item<int64_t>() >= 0 &&
                    seq.max().item<int64_t>() < n_slots,
                "seq out of [0, n_slots)");
    return d;
}

using AttnResult = std::tuple<torch::Tensor, torch::Tensor, int64_t>;

// (out [T, E] f32, zero-filled out_prep i16 [(E/8)*jtw*128], jtw)
AttnResult alloc_attn_result(const AttnDims& d) {
    auto dev = torch::TensorOptions().device(torch::kCUDA);
    const int jtw = jt_width(d.T);
    TORCH_CHECK(jtw * 16 >= d.T, "jt_width does not cover T");
    auto out = torch::zeros({d.T, d.E}, dev.dtype(torch::kFloat32));
    auto prep = torch::zeros({(int64_t)(d.E / 8) * jtw * 128},
                             dev.dtype(torch::kInt16));
    return {out, prep, (int64_t)jtw};
}

const __half* h16c(const torch::Tensor& t) {
    return reinterpret_cast<const __half*>(t.data_ptr());
}
__half* h16(torch::Tensor& t) {
    return reinterpret_cast<__half*>(t.data_ptr());
}

AttnDims check_q_args(const torch::Tensor& q, int64_t n_head,
                      int64_t n_head_kv, int64_t n_ctx, int64_t n_slots,
                      const torch::Tensor& k_store,
                      const torch::Tensor& v_store,
                      const torch::Tensor& pos, const torch::Tensor& seq) {
    check_f32(q, "q");
    TORCH_CHECK(q.dim() == 2 && q.size(0) >= 1, "q must be [T, E]");
    TORCH_CHECK(n_head >= 1 && q.size(1) % n_head == 0,
                "E not divisible by n_head");
    return check_attn_args(q.size(0), n_head, n_head_kv,
                           q.size(1) / n_head, n_ctx, n_slots, k_store,
                           v_store, pos, seq);
}

AttnResult attention_decode(torch::Tensor q, torch::Tensor k_store,
                            torch::Tensor v_store, torch::Tensor pos,
                            torch::Tensor seq, int64_t n_head,
                            int64_t n_head_kv, int64_t n_ctx,
                            int64_t n_slots) {
    const AttnDims d = check_q_args(q, n_head, n_head_kv, n_ctx, n_slots,
                                    k_store, v_store, pos, seq);
    AttnResult r = alloc_attn_result(d);
    hipStream_t s = c10::hip::getCurrentHIPStream().stream();
    launch_attention(s, q.data_ptr<float>(), h16c(k_store), h16(v_store),
                     std::get<0>(r).data_ptr<float>(), u16p(std::get<1>(r)),
                     pos.data_ptr<int>(), seq.data_ptr<int>(), d.T, d.H,
                     d.E, d.Ekv, d.D, d.ctx, nullptr, 0, nullptr);
    return r;
}

// appends row pos[t] of slot seq[t] to k_store / v_store in place
AttnResult attention_decode_fused(torch::Tensor slab, torch::Tensor k_store,
                                  torch::Tensor v_store, torch::Tensor pos,
                                  torch::Tensor seq, torch::Tensor inv_freq,
                                  int64_t n_head, int64_t n_head_kv,
                                  int64_t head_dim, int64_t n_ctx,
                                  int64_t n_slots) {
    check_i32(pos, "pos");
    const int64_t T = pos.numel();
    TORCH_CHECK(T <= kMaxTokens, "the fused variant takes at most ",
                kMaxTokens, " tokens (slab token width)");
    const AttnDims d = check_attn_args(T, n_head, n_head_kv, head_dim,
                                       n_ctx, n_slots, k_store, v_store,
                                       pos, seq);
    // every block appends its own row and reads only its own sequence
    auto sorted = std::get<0>(seq.to(torch::kCPU).to(torch::kInt64).sort());
    for (int64_t i = 1; i < T; ++i)
        TORCH_CHECK(sorted[i].item<int64_t>() !=
                        sorted[i - 1].item<int64_t>(),
                    "seq values must be pairwise distinct");
    const int ks = qkv16_ks(d.E, d.Ekv);
    check_f32(slab, "slab");
    TORCH_CHECK(slab.numel() == slab_numel((d.E + 2 * d.Ekv) / 16, ks),
                "slab must be f32[(E+2Ekv)/16][ks][64][16]");
    check_f32(inv_freq, "inv_freq");
    TORCH_CHECK(inv_freq.numel() == d.D / 2, "inv_freq must be [D/2]");
    AttnResult r = alloc_attn_result(d);
    hipStream_t s = c10::hip::getCurrentHIPStream().stream();
    launch_attention(s, nullptr, h16c(k_store), h16(v_store),
                     std::get<0>(r).data_ptr<float>(), u16p(std::get<1>(r)),
                     pos.data_ptr<int>(), seq.data_ptr<int>(), d.T, d.H,
                     d.E, d.Ekv, d.D, d.ctx, slab.data_ptr<float>(), ks,
                     inv_freq.data_ptr<float>());
    return r;
}

AttnResult attention_prefill(torch::Tensor q, torch::Tensor k_store,
                             torch::Tensor v_store, torch::Tensor pos,
                             torch::Tensor seq, int64_t n_head,
                             int64_t n_head_kv, int64_t n_ctx,
                             int64_t n_slots) {
    const AttnDims d = check_q_args(q, n_head, n_head_kv, n_ctx, n_slots,
                                    k_store, v_store, pos, seq);
    AttnResult r = alloc_attn_result(d);
    hipStream_t s = c10::hip::getCurrentHIPStream().stream();
    launch_attn_prefill(s, q.data_ptr<float>(), h16c(k_store),
                        h16c(v_store), std::get<0>(r).data_ptr<float>(),
                        u16p(std::get<1>(r)), pos.data_ptr<int>(),
                        seq.data_ptr<int>(), d.T, d.H, d.E, d.Ekv, d.D,
                        d.ctx);
    return r;
}

// ----------------------------------------------- dequant-GEMM test hooks
// Direct entry points to the launchers of mfma_gemm.hip for tests/
// test_gpu_gemm.py, in the spirit of the attention hooks above: every
// buffer is allocated per call by the engine's own sizing rules (tiled
// matrices through make_devmat2, side channels by side_numel at panel
// width jt_width(T), norm weights through pad_normprep, sumsq buffers by
// sumsq_numel, the slab by slab_numel at the maximum split), and everything
// that could send a kernel out of bounds is refused. The hooks call the
// launchers the engine calls, so the route code under test is the engine's.
//
// dead_fill: after the input panel is staged with launch_prep_x, the dead
// token columns t in [T, 16*jtw) of the live rows kc < cols/8 are
// overwritten with this f16 bit pattern. Live outputs must not depend on
// it. The K-pad rows stay zero as in the engine (they meet alpha = beta = 0
// blocks and must be finite).

constexpr int64_t kHookMaxT = 4096;

DevMat2 mat_arg(const py::tuple& m, const char* name) {
    TORCH_CHECK(m.size() == 5, name,
                " must be (data, scales, wtype, rows, cols)");
    const int64_t wt = m[2].cast<int64_t>();
    const int64_t rows = m[3].cast<int64_t>();
    const int64_t cols = m[4].cast<int64_t>();
    TORCH_CHECK(rows >= 16 && rows <= ((int64_t)1 << 20) && cols >= 32 &&
                    cols <= ((int64_t)1 << 16),
                name, ": rows/cols out of range");
    return make_devmat2(m[0].cast<torch::Tensor>(),
                        m[1].cast<torch::Tensor>(), wt, rows, cols);
}

int check_panel_input(const torch::Tensor& x, int64_t cols,
                      const char* name) {
    check_f32(x, name);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == cols, name,
                " must be [T, cols] with the matrix's cols");
    TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= kHookMaxT,
                "token count out of range");
    return (int)x.size(0);
}

int16_t check_dead_fill(int64_t dead_fill) {
    TORCH_CHECK(dead_fill >= -32768 && dead_fill <= 65535,
                "dead_fill must be a 16-bit pattern");
    return (int16_t)(uint16_t)(dead_fill & 0xFFFF);
}

torch::Tensor check_norm_w(const torch::Tensor& w, int64_t cols) {
    check_f32(w, "norm_w");
    TORCH_CHECK(w.dim() == 1 && w.numel() == cols, "norm_w must be [cols]");
    return pad_normprep(w);
}

struct Panel {
    torch::Tensor prep, ss;
    int jtw;
};

// x [T, cols] -> f16 panel + sumsq, then the dead columns filled
Panel stage_panel(hipStream_t s, const torch::Tensor& x, int cols, int T,
                  int16_t fill) {
    auto dev = torch::TensorOptions().device(torch::kCUDA);
    Panel p;
    p.jtw = jt_width(T);
    TORCH_CHECK(p.jtw * 16 >= T, "jt_width does not cover T");
    p.prep = torch::zeros({side_numel(cols, p.jtw)}, dev.dtype(torch::kInt16));
    p.ss = torch::zeros({sumsq_numel(T)}, dev.dtype(torch::kFloat32));
    launch_prep_x(s, x.data_ptr<float>(), u16p(p.prep),
                  p.ss.data_ptr<float>(), cols, T, p.jtw);
    if (T < p.jtw * 16)
        p.prep.narrow(0, 0, (int64_t)(cols / 8) * p.jtw * 128)
            .view({cols / 8, (int64_t)p.jtw * 16, 8})
            .slice(1, T, (int64_t)p.jtw * 16)
            .fill_(fill);
    return p;
}

torch::Tensor zero_side(int64_t cols, int64_t jtw) {
    return torch::zeros(
        {side_numel(cols, jtw)},
        torch::TensorOptions().device(torch::kCUDA).dtype(torch::kInt16));
}

// y = y_in + mat . b through launch_gemm16_residual, split passed as
// split_ok. split = true is refused unless gemm16_res_route then takes the
// slab route 0 (T <= 64 and rows/16 even), so split names the route.
// -> (y [T, rows] f32, xprep_out i16 flat, ss_out f32 [T up to 64], jtw)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, int64_t>
gemm_residual(py::tuple mat, torch::Tensor b, torch::Tensor y_in, bool split,
              int64_t dead_fill) {
    DevMat2 m = mat_arg(mat, "mat");
    const int T = check_panel_input(b, m.w.cols, "b");
    check_f32(y_in, "y_in");
    TORCH_CHECK(y_in.dim() == 2 && y_in.size(0) == T &&
                    y_in.size(1) == m.w.rows,
                "y_in must be [T, rows]");
    const int16_t fill = check_dead_fill(dead_fill);
    TORCH_CHECK(!split || gemm16_res_route(m.w.rows, T, 1) == 0,
                "split-K is a decode route (T <= 64), taken only when "
                "rows/16 is even");
    TORCH_CHECK(gemm16_ks(m.w.rows) <= kMaxSplit,
                "split factor out of range");
    auto f32 = torch::TensorOptions().device(torch::kCUDA).dtype(
        torch::kFloat32);
    hipStream_t s = c10::hip::getCurrentHIPStream().stream();
    Panel p = stage_panel(s, b, m.w.cols, T, fill);
    auto y = y_in.clone();
    auto xo = zero_side(m.w.rows, p.jtw);
    auto sso = torch::zeros({sumsq_numel(T)}, f32);
    torch::Tensor slab;
    if (split) slab = torch::zeros({slab_numel(m.w.rows / 16)}, f32);
    launch_gemm16_residual(s, m.w, u16p(p.prep), y.data_ptr<float>(),
                           u16p(xo), sso.data_ptr<float>(), T,
                           split ? slab.data_ptr<float>() : nullptr,
                           split ? 1 : 0);
    return {y, xo, sso, (int64_t)p.jtw};
}

// logits [T, rows] = mat . rmsnorm(x) * norm_w: launch_prep_x +
// launch_lmhead, T <= 64
torch::Tensor gemm_lmhead(py::tuple mat, torch::Tensor x,
                          torch::Tensor norm_w, double eps,
                          int64_t dead_fill) {
    DevMat2 m = mat_arg(mat, "mat");
    const int T = check_panel_input(x, m.w.cols, "x");
    TORCH_CHECK(T <= kMaxTokens, "the lm_head takes at most ", kMaxTokens,
                " rows per launch");
    auto normprep = check_norm_w(norm_w, m.w.cols);
    const int16_t fill = check_dead_fill(dead_fill);
    hipStream_t s = c10::hip::getCurrentHIPStream().stream();
    Panel p = stage_panel(s, x, m.w.cols, T, fill);
    auto lg = torch::zeros(
        {T, m.w.rows},
        torch::TensorOptions().device(torch::kCUDA).dtype(torch::kFloat32));
    launch_lmhead(s, m.w, u16p(p.prep), u16p(normprep),
                  p.ss.data_ptr<float>(), (float)eps, lg.data_ptr<float>(),
                  T);
    return lg;
}

// gprep = f16(silu(m1 . n) * (m3 . n)), n = rmsnorm(x) * norm_w, in the
// side-channel layout: launch_ffn16.
// -> (gprep i16 flat, jtw)
std::tuple<torch::Tensor, int64_t> ffn_gate(py::tuple m1, py::tuple m3,
                                            torch::Tensor x,
                                            torch::Tensor norm_w, double eps,
                                            int64_t dead_fill) {
    DevMat2 a = mat_arg(m1, "m1");
    DevMat2 c = mat_arg(m3, "m3");
    TORCH_CHECK(a.w.rows == c.w.rows && a.w.cols == c.w.cols &&
                    a.w.wtype == c.w.wtype,
                "m1 and m3 must agree in rows, cols and wtype");
    const int T = check_panel_input(x, a.w.cols, "x");
    auto normprep = check_norm_w(norm_w, a.w.cols);
    const int16_t fill = check_dead_fill(dead_fill);
    hipStream_t s = c10::hip::getCurrentHIPStream().stream();
    Panel p = stage_panel(s, x, a.w.cols, T, fill);
    auto g = zero_side(a.w.rows, p.jtw);
    launch_ffn16(s, a.w, c.w, u16p(p.prep), u16p(normprep),
                 p.ss.data_ptr<float>(), (float)eps, u16p(g), T);
    return {g, (int64_t)p.jtw};
}

// q [T, E] = rope(mq . n); rows pos[t] of slot seq[t] of k_store / v_store
// get rope(mk . n) / mv . n in place. launch_qkv16 with a slab and
// skip_finish = 0 (T <= 64: slab route + k_qkv_finish, or a fused route,
// as qkv16_route decides; T > 64: large-M, the slab unused).
torch::Tensor qkv_project(py::tuple mq, py::tuple mk, py::tuple mv,
                          torch::Tensor x, torch::Tensor norm_w, double eps,
                          torch::Tensor k_store, torch::Tensor v_store,
                          torch::Tensor pos, torch::Tensor seq,
                          torch::Tensor inv_freq, int64_t n_head,
                          int64_t n_head_kv, int64_t n_ctx, int64_t n_slots,
                          int64_t dead_fill) {
    DevMat2 q = mat_arg(mq, "mq");
    DevMat2 k = mat_arg(mk, "mk");
    DevMat2 v = mat_arg(mv, "mv");
    const int E = q.w.rows;
    TORCH_CHECK(q.w.cols == E && k.w.cols == E && v.w.cols == E,
                "mq must be [E, E], mk and mv [Ekv, E]");
    TORCH_CHECK(k.w.rows == v.w.rows, "mk and mv must agree in rows");
    TORCH_CHECK(k.w.wtype == q.w.wtype && v.w.wtype == q.w.wtype,
                "mq, mk and mv must share one wtype");
    const int T = check_panel_input(x, E, "x");
    TORCH_CHECK(n_head >= 1 && E % n_head == 0, "E not divisible by n_head");
    const AttnDims d = check_attn_args(T, n_head, n_head_kv, E / n_head,
                                       n_ctx, n_slots, k_store, v_store,
                                       pos, seq);
    TORCH_CHECK(d.E == E && d.Ekv == k.w.rows,
                "head counts do not match the matrices");
    // two tokens must not write the same cache row
    {
        auto key = (seq.to(torch::kCPU).to(torch::kInt64) * n_ctx +
                    pos.to(torch::kCPU).to(torch::kInt64));
        auto sorted = std::get<0>(key.sort());
        for (int64_t i = 1; i < T; ++i)
            TORCH_CHECK(sorted[i].item<int64_t>() !=
                            sorted[i - 1].item<int64_t>(),
                        "(seq, pos) pairs must be pairwise distinct");
    }
    check_f32(inv_freq, "inv_freq");
    TORCH_CHECK(inv_freq.numel() == d.D / 2, "inv_freq must be [D/2]");
    auto normprep = check_norm_w(norm_w, E);
    const int16_t fill = check_dead_fill(dead_fill);
    auto f32 = torch::TensorOptions().device(torch::kCUDA).dtype(
        torch::kFloat32);
    hipStream_t s = c10::hip::getCurrentHIPStream().stream();
    Panel p = stage_panel(s, x, E, T, fill);
    auto qb = torch::zeros({T, E}, f32);
    TORCH_CHECK(qkv16_ks(E, d.Ekv) <= kMaxSplit, "split factor out of range");
    auto slab = torch::zeros({slab_numel((E + 2 * d.Ekv) / 16)}, f32);
    launch_qkv16(s, q.w, k.w, v.w, u16p(p.prep), u16p(normprep),
                 p.ss.data_ptr<float>(), (float)eps, qb.data_ptr<float>(),
                 h16(k_store), h16(v_store), pos.data_ptr<int>(),
                 seq.data_ptr<int>(), inv_freq.data_ptr<float>(), E, d.Ekv,
                 d.D, d.ctx, T, slab.data_ptr<float>(), /*skip_finish=*/0);
    return qb;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    // test hooks (see above), not serving API
    m.def("gemm_residual", &gemm_residual, py::arg("mat"), py::arg("b"),
          py::arg("y_in"), py::arg("split"), py::arg("dead_fill"));
    m.def("gemm_lmhead", &gemm_lmhead, py::arg("mat"), py::arg("x"),
          py::arg("norm_w"), py::arg("eps"), py::arg("dead_fill"));
    m.def("ffn_gate", &ffn_gate, py::arg("m1"), py::arg("m3"), py::arg("x"),
          py::arg("norm_w"), py::arg("eps"), py::arg("dead_fill"));
    m.def("qkv_project", &qkv_project, py::arg("mq"), py::arg("mk"),
          py::arg("mv"), py::arg("x"), py::arg("norm_w"), py::arg("eps"),
          py::arg("k_store"), py::arg("v_store"), py::arg("pos"),
          py::arg("seq"), py::arg("inv_freq"), py::arg("n_head"),
          py::arg("n_head_kv"), py::arg("n_ctx"), py::arg("n_slots"),
          py::arg("dead_fill"));
    m.def("gemm16_ks", [](int64_t rows) {
        return (int64_t)gemm16_ks((int)rows);
    }, py::arg("rows"));
    m.def("gemm16_plain_rt", [](int64_t rows) {
        return (int64_t)gemm16_plain_rt((int)rows);
    }, py::arg("rows"));
    m.def("ffn16_rt", [](int64_t rows, int64_t T) {
        return (int64_t)ffn16_rt((int)rows, (int)T);
    }, py::arg("rows"), py::arg("T"));
    m.def("gemm16_mt_rt", [](int64_t rows, int64_t T) {
        return (int64_t)gemm16_mt_rt((int)rows, (int)T);
    }, py::arg("rows"), py::arg("T"));
    m.def("gemm16_res_route", [](int64_t rows, int64_t T, bool split_ok) {
        return (int64_t)gemm16_res_route((int)rows, (int)T,
                                         split_ok ? 1 : 0);
    }, py::arg("rows"), py::arg("T"), py::arg("split_ok"));
    m.def("qkv16_route", [](int64_t E, int64_t Ekv, int64_t T,
                            bool has_slab) {
        return (int64_t)qkv16_route((int)E, (int)Ekv, (int)T,
                                    has_slab ? 1 : 0);
    }, py::arg("E"), py::arg("Ekv"), py::arg("T"), py::arg("has_slab"));
    m.def("qkv16_mt_rt", [](int64_t E, int64_t Ekv, int64_t T) {
        return (int64_t)qkv16_mt_rt((int)E, (int)Ekv, (int)T);
    }, py::arg("E"), py::arg("Ekv"), py::arg("T"));
    m.def("attention_decode", &attention_decode, py::arg("q"),
          py::arg("k_store"), py::arg("v_store"), py::arg("pos"),
          py::arg("seq"), py::arg("n_head"), py::arg("n_head_kv"),
          py::arg("n_ctx"), py::arg("n_slots"));
    m.def("attention_decode_fused", &attention_decode_fused,
          py::arg("slab"), py::arg("k_store"), py::arg("v_store"),
          py::arg("pos"), py::arg("seq"), py::arg("inv_freq"),
          py::arg("n_head"), py::arg("n_head_kv"), py::arg("head_dim"),
          py::arg("n_ctx"), py::arg("n_slots"));
    m.def("attention_prefill", &attention_prefill, py::arg("q"),
          py::arg("k_store"), py::arg("v_store"), py::arg("pos"),
          py::arg("seq"), py::arg("n_head"), py::arg("n_head_kv"),
          py::arg("n_ctx"), py::arg("n_slots"));
    m.def("qkv16_ks", [](int64_t E, int64_t Ekv) {
        return (int64_t)qkv16_ks((int)E, (int)Ekv);
    }, py::arg("E"), py::arg("Ekv"));
    m.def("lmhead_score_rt", [](int64_t V, int64_t T) {
        return (int64_t)lmhead_score_rt((int)V, (int)T);
    }, py::arg("V"), py::arg("T"));
    m.def("jt_width", [](int64_t T) { return (int64_t)jt_width((int)T); },
          py::arg("T"));
    m.doc() = "MI355X-native layer-slice inference engine (CDNA4 HIP kernels)";
    py::class_<SliceEngine, std::shared_ptr<SliceEngine>>(m, "SliceEngine")
        .def(py::init<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                      double, double, int64_t, int64_t>(),
             py::arg("n_embd"), py::arg("n_head"), py::arg("n_layers"),
             py::arg("n_ff"), py::arg("n_ctx"), py::arg("max_batch"),
             py::arg("eps"), py::arg("rope_base"),
             py::arg("max_prefill") = 1024, py::arg("n_head_kv") = 0)
        .def("set_layer", &SliceEngine::set_layer)
        .def("set_extra", &SliceEngine::set_extra)
        .def("forward", &SliceEngine::forward, py::arg("x"),
             py::arg("pos"), py::arg("seq"), py::arg("decode") = false)
        .def("embed", &SliceEngine::embed)
        .def("logits", &SliceEngine::logits, py::arg("x"),
             py::arg("all_logits") = false)
        .def("argmax", &SliceEngine::argmax)
        .def("sample", &SliceEngine::sample, py::arg("logits"),
             py::arg("params"), py::arg("seen"), py::arg("row_max"),
             py::arg("slot_max"))
        .def("logprobs", &SliceEngine::logprobs, py::arg("logits"),
             py::arg("rows"), py::arg("ids"), py::arg("top_n"),
             py::arg("row_max"))
        .def("score", &SliceEngine::score, py::arg("x"), py::arg("targets"))
        .def_property_readonly("out_mfma", &SliceEngine::out_mfma)
        .def_property_readonly("max_tokens", &SliceEngine::max_tokens)
        .def_property_readonly("max_prefill", &SliceEngine::max_prefill)
        .def_property_readonly("n_ctx", &SliceEngine::n_ctx)
        .def_property_readonly("max_batch", &SliceEngine::max_batch)
        .def_property_readonly("k_cache", &SliceEngine::k_cache)
        .def_property_readonly("v_cache", &SliceEngine::v_cache);
}
