"""Slice engines: the HIP/CDNA4 production engine and a CPU torch twin.

Both expose the same *stateless* interface (positions and sequence ids are
explicit per-token arrays), which is what makes the decode step
graph-capturable and the pipeline testable on CPU:

    forward(x[T,E] f32, pos[T] i32, seq[T] i32) -> x'   (KV appended)
    embed(tokens[T]) -> x[T,E]
    logits(x[T,E], all_logits=False) -> [T|1, V]

``clear_context`` in the reference (tensor_processor.cpp:1512-1521 destroys
and recreates the llama_context) is here simply "start writing positions
from 0 again" — cache slots are overwritten, nothing to reset.

The HIP engine repacks on-disk tensors into the MFMA tile layouts the
kernels stream once at load, on the GPU (engine/repack.py).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from ..formats import ggml
from ..models.llama import RMS_EPS, ROPE_BASE, rms_norm, rope_interleaved
from .repack import (W_F32, _BYTE_GTYPES, _upload_mat, random_tiles,
                     repack_mfma)
from .sampler import LOGPROBS_MAX_TOP


class HIPSliceEngine:
    """Production engine: CDNA4 kernels, weights resident in HBM3E."""

    def __init__(self, hp: ggml.Hparams, n_layers: int, first_layer: int,
                 n_ctx: int = 2048, max_batch: int = 16,
                 max_prefill: Optional[int] = None):
        from .. import ops
        core = ops.core()
        self.hp = hp
        self.first_layer = first_layer
        self.n_layers = n_layers
        self.n_ctx = n_ctx
        self.max_batch = max_batch
        # prefill token cap per forward call (side channels scale with it;
        # larger prompts tile host-side in max_prefill chunks)
        if max_prefill is None:
            max_prefill = max(64, min(n_ctx, 2048))
        self._eng = core.SliceEngine(
            n_embd=hp.n_embd, n_head=hp.n_head, n_layers=n_layers,
            n_ff=hp.n_ff, n_ctx=n_ctx, max_batch=max_batch,
            eps=RMS_EPS, rope_base=ROPE_BASE, max_prefill=max_prefill,
            n_head_kv=hp.kv_heads if hp.is_gqa else 0)
        self.device = "cuda"
        self.has_extra = False
        # weight-tensor references for clone_shared (filled by .random()
        # or load_layers/attach_extra; the C++ engine holds references to
        # the same device tensors, so clones share HBM)
        self._layers_cache = None
        self._extra_cache = None

    @classmethod
    def from_ggml(cls, f: ggml.GGMLFile, n_ctx: int = 2048,
                  max_batch: int = 16) -> "HIPSliceEngine":
        hp = f.hparams
        first = hp.first_layer if hp.first_layer is not None else 0
        eng = cls(hp, hp.n_layer, first, n_ctx, max_batch)
        eng.load_layers(f)
        return eng

    @classmethod
    def random(cls, hp: ggml.Hparams, n_layers: int, first_layer: int = 0,
               n_ctx: int = 2048, max_batch: int = 16, seed: int = 0,
               with_extra: bool = True,
               max_prefill: Optional[int] = None) -> "HIPSliceEngine":
        """Random-init engine straight on the GPU (synthetic benchmarking).

        Generates weights directly in the repacked kernel layout — identical
        compute and HBM traffic to a real checkpoint of this architecture,
        without materializing a multi-GB GGML file on disk.
        """
        eng = cls(hp, n_layers, first_layer, n_ctx, max_batch,
                  max_prefill=max_prefill)
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        E, F, V = hp.n_embd, hp.n_ff, hp.n_vocab
        wt = ggml._FTYPE_TO_GGML[hp.ftype]

        def mat(rows: int, cols: int):
            return random_tiles(wt, rows, cols, g)

        def norm_w(n: int):
            return (1.0 + torch.randn(n, device="cuda", generator=g) *
                    0.01).contiguous()

        Ekv = hp.n_embd_kv  # K/V projection rows (GQA: Hkv*D < E)
        shapes = [(E, E), (Ekv, E), (Ekv, E), (E, E), (F, E), (E, F),
                  (F, E)]
        eng._layers_cache = []
        for li in range(n_layers):
            mats = [mat(r, c) for r, c in shapes]
            an, fn = norm_w(E), norm_w(E)
            eng._layers_cache.append((an, fn, mats))
            eng._eng.set_layer(li, an, fn, mats)
        eng._extra_cache = None
        if with_extra:
            # the embedding table uses the legacy SoA layout (gather kernel)
            if wt in _BYTE_GTYPES:
                tok_d = (torch.randn(V, E, device="cuda", generator=g,
                                     dtype=torch.float32) * 0.02).to(
                    torch.float16)
                tok_s, tok_t = torch.empty(0), ggml.GGML_TYPE_F16
            elif wt in (ggml.GGML_TYPE_Q4_0, ggml.GGML_TYPE_Q4_1):
                nb = E // 32
                per = 2 if wt == ggml.GGML_TYPE_Q4_1 else 1
                tok_d = torch.randint(0, 256, (V, nb * 16),
                                      dtype=torch.uint8, device="cuda",
                                      generator=g)
                tok_s = ((torch.rand(V, nb * per, device="cuda",
                                     generator=g) * 0.5 + 0.75) *
                         0.003).to(torch.float16)
                tok_t = wt
            elif wt == ggml.GGML_TYPE_F16:
                tok_d = (torch.randn(V, E, device="cuda", generator=g) *
                         0.02).to(torch.float16)
                tok_s, tok_t = torch.empty(0), wt
            else:
                tok_d = (torch.randn(V, E, device="cuda", generator=g) *
                         0.02)
                tok_s, tok_t = torch.empty(0), wt
            out_d, out_s, out_t = mat(V, E)
            fin = norm_w(E)
            eng._extra_cache = (tok_d, tok_s, tok_t, fin, out_d, out_s,
                                out_t, V)
            eng._eng.set_extra(tok_d, tok_s, tok_t, fin, out_d, out_s,
                               out_t, V)
            eng.has_extra = True
        return eng

    def clone_shared(self) -> "HIPSliceEngine":
        """A second engine over the SAME weight tensors (HBM shared) with
        its own KV cache and side-channel buffers — lets independent
        micro-batches run concurrently on separate HIP streams without
        duplicating the model."""
        assert getattr(self, "_layers_cache", None) is not None, \
            "clone_shared requires an engine built by .random()/.from_ggml"
        twin = HIPSliceEngine(self.hp, self.n_layers, self.first_layer,
                              self.n_ctx, self.max_batch,
                              max_prefill=int(self._eng.max_prefill))
        for li, (an, fn, mats) in enumerate(self._layers_cache):
            twin._eng.set_layer(li, an, fn, mats)
        twin._layers_cache = self._layers_cache  # enables further clones
        if self._extra_cache is not None:
            twin._extra_cache = self._extra_cache
            twin._eng.set_extra(*self._extra_cache)
            twin.has_extra = True
        return twin

    def load_layers(self, f: ggml.GGMLFile) -> None:
        tm = f.tensor_map()
        self._layers_cache = []
        for li in range(self.n_layers):
            gi = li + self.first_layer
            pre = f"layers.{gi}."
            attn_norm = torch.from_numpy(
                tm[pre + "attention_norm.weight"].to_f32()).to(self.device)
            ffn_norm = torch.from_numpy(
                tm[pre + "ffn_norm.weight"].to_f32()).to(self.device)
            mats = []
            for nm in ("attention.wq.weight", "attention.wk.weight",
                       "attention.wv.weight", "attention.wo.weight",
                       "feed_forward.w1.weight", "feed_forward.w2.weight",
                       "feed_forward.w3.weight"):
                mats.append(repack_mfma(tm[pre + nm], self.device))
            self._layers_cache.append((attn_norm, ffn_norm, mats))
            self._eng.set_layer(li, attn_norm, ffn_norm, mats)

    def attach_extra(self, f: ggml.GGMLFile) -> None:
        tm = f.tensor_map()
        # embedding table: legacy SoA layout (row-gather kernel);
        # lm_head: MFMA tiles (it is a GEMV like any other)
        tok_d, tok_s, tok_t = _upload_mat(tm["tok_embeddings.weight"],
                                          self.device)
        out_d, out_s, out_t = repack_mfma(tm["output.weight"], self.device)
        norm = torch.from_numpy(tm["norm.weight"].to_f32()).to(self.device)
        self._extra_cache = (tok_d, tok_s, tok_t, norm, out_d, out_s,
                             out_t, self.hp.n_vocab)
        self._eng.set_extra(*self._extra_cache)
        self.has_extra = True

    def forward(self, x: torch.Tensor, pos: torch.Tensor,
                seq: torch.Tensor, decode: bool = False) -> torch.Tensor:
        """decode=True asserts every token is a distinct sequence
        (batched decode) — enables the qkv-slab + fused-attention path.

        T > 64 (prefill) runs the native large-M path: hand-written
        XCD-grouped dequant-GEMM kernels over all T tokens, the layer
        loop sequenced in C++ (replaced the round-1 rocBLAS-over-
        detiled-f16 path — no f16 weight copy, mixed multi-span
        admission streams handled natively)."""
        T = x.shape[0]
        # the large-M path serves decode too (wide batched decode pays
        # the weight stream + dequant once for the whole batch)
        cap = self._eng.max_prefill if self._mfma_path() \
            else self._eng.max_tokens
        if T <= cap:
            return self._eng.forward(x, pos, seq, decode=decode)
        # token-tile larger inputs; KV order is preserved because tile
        # i's cache rows are written before tile i+1 attends.
        outs = []
        for t0 in range(0, T, cap):
            t1 = min(T, t0 + cap)
            outs.append(self._eng.forward(
                x[t0:t1].contiguous(), pos[t0:t1].contiguous(),
                seq[t0:t1].contiguous(), decode=decode))
        return torch.cat(outs, dim=0)

    def _mfma_path(self) -> bool:
        if not self._layers_cache:
            return False
        return all(m[2] != W_F32
                   for (_, _, mats) in self._layers_cache for m in mats)

    def embed(self, tokens: torch.Tensor) -> torch.Tensor:
        return self._eng.embed(tokens.to(self.device, torch.int32))

    def logits(self, x: torch.Tensor, all_logits: bool = False) -> torch.Tensor:
        if not all_logits:
            return self._eng.logits(x, False)
        mt = self._eng.max_tokens
        if x.shape[0] <= mt:
            return self._eng.logits(x, True)
        return torch.cat([self._eng.logits(x[t0:t0 + mt].contiguous(), True)
                          for t0 in range(0, x.shape[0], mt)], dim=0)

    def argmax(self, lg: torch.Tensor) -> torch.Tensor:
        return self._eng.argmax(lg)

    # ---- on-device sampling (ops/csrc/sampling.hip) ----

    def new_seen_state(self, n_slots: Optional[int] = None) -> torch.Tensor:
        """Zeroed repetition bitmap [slots, ceil(V/32)]: bit i of slot s is
        set once token i was sampled by the request in that slot."""
        n = self.max_batch if n_slots is None else int(n_slots)
        return torch.zeros(n, (self.hp.n_vocab + 31) // 32,
                           dtype=torch.int32, device=self.device)

    def reset_seen(self, seen: torch.Tensor, slot: int) -> None:
        seen[slot].zero_()

    def sample(self, lg: torch.Tensor, rows, slots, u, temperature,
               repeat_penalty, top_k, top_p,
               seen: torch.Tensor) -> torch.Tensor:
        """Sample lg[rows[r]] for every r in ONE launch on the current
        stream; per-row host sequences u (uniforms in [0, 1)),
        temperature, repeat_penalty, top_k, top_p. Slots must be
        distinct; seen[slots[r]] supplies the penalty set and gains the
        chosen bit. One packed upload, returns device i32 ids [R] —
        semantics of engine.sampler.sample_reference."""
        R = len(rows)
        rows = np.asarray(rows, dtype=np.int64)
        slots = np.asarray(slots, dtype=np.int64)
        if R == 0 or not (len(slots) == len(u) == len(temperature) ==
                          len(repeat_penalty) == len(top_k) ==
                          len(top_p) == R):
            raise ValueError("sample: per-row arguments must share one "
                             "non-zero length")
        if rows.min() < 0 or rows.max() >= lg.shape[0]:
            raise ValueError("sample: row index out of range")
        if slots.min() < 0 or slots.max() >= seen.shape[0]:
            raise ValueError("sample: slot index out of range")
        if len(np.unique(slots)) != R:
            raise ValueError("sample: slots must be distinct")
        packed = np.empty((7, R), dtype=np.int32)
        fl = packed.view(np.float32)
        packed[0] = rows
        packed[1] = slots
        # the kernel's pick needs u < 1 after the f32 rounding
        fl[2] = np.minimum(np.asarray(u, dtype=np.float64).astype(
            np.float32), np.float32(1.0 - 2.0 ** -24))
        fl[3] = np.asarray(temperature, dtype=np.float32)
        fl[4] = np.asarray(repeat_penalty, dtype=np.float32)
        packed[5] = np.clip(np.asarray(top_k, dtype=np.int64), 0,
                            2 ** 31 - 1)
        fl[6] = np.asarray(top_p, dtype=np.float32)
        params = torch.from_numpy(packed).to(self.device)
        return self._eng.sample(lg, params, seen, int(rows.max()),
                                int(slots.max()))

    # ---- per-token log-probabilities (ops/csrc/logprobs.hip) ----

    def logprobs(self, lg: torch.Tensor, rows, ids: torch.Tensor,
                 top_n: int = 0):
        """Raw log-softmax value of token ids[r] in lg[rows[r]] plus the
        top_n most likely tokens of that row, for every r in ONE launch
        on the current stream. `rows` is a host sequence (one packed
        upload); `ids` a device i32 tensor [R] - the output of `argmax`
        or `sample` goes in without leaving the GPU. Returns device
        tensors (lp [R] f32, top_ids [R, top_n] i32, top_lp [R, top_n]
        f32) - semantics of engine.sampler.logprobs_reference. An id
        outside the vocabulary yields lp = NaN."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        R = len(rows)
        top_n = int(top_n)
        if R == 0 or ids.dim() != 1 or ids.shape[0] != R:
            raise ValueError("logprobs: rows and ids must share one "
                             "non-zero length")
        if rows.min() < 0 or rows.max() >= lg.shape[0]:
            raise ValueError("logprobs: row index out of range")
        if not 0 <= top_n <= LOGPROBS_MAX_TOP:
            raise ValueError(
                f"logprobs: top_n must be in 0..{LOGPROBS_MAX_TOP}")
        if top_n > lg.shape[1]:
            raise ValueError("logprobs: top_n exceeds the vocabulary")
        rows_dev = torch.from_numpy(rows.astype(np.int32)).to(self.device)
        return self._eng.logprobs(lg, rows_dev, ids, top_n,
                                  int(rows.max()))

    # ---- prompt scoring (mfma_gemm.hip k_lmhead_score + logprobs.hip
    # k_score_finish) ----

    def score(self, x: torch.Tensor, targets):
        """Score activation rows against their next tokens on the current
        stream: the log-probability of targets[t] under final norm +
        lm_head of x[t], and that row's arg-max, without forming [T, V]
        logits. `targets` is a host sequence or a device i32 tensor [T]; a
        target outside the vocabulary means "no target" (lp = NaN, the top
        entry is still reported). Returns device tensors (lp [T] f32,
        top_id [T] i32, top_lp [T] f32) - semantics of
        engine.sampler.score_reference. Inputs longer than max_prefill are
        tiled. A legacy f32 lm_head composes logits() + logprobs()
        instead."""
        if x.dim() != 2 or x.shape[0] < 1:
            raise ValueError("score: x must be [T, E] with T >= 1")
        T = x.shape[0]
        if isinstance(targets, torch.Tensor):
            tg = targets.to(self.device, torch.int32).reshape(-1)
        else:
            tg = torch.from_numpy(np.asarray(
                targets, dtype=np.int64).reshape(-1).astype(np.int32)).to(
                self.device)
        if tg.shape[0] != T:
            raise ValueError("score: one target per row of x")
        if self._eng.out_mfma:
            cap = int(self._eng.max_prefill)
            parts = [self._eng.score(x[t0:t0 + cap].contiguous(),
                                     tg[t0:t0 + cap].contiguous())
                     for t0 in range(0, T, cap)]
        else:
            cap = int(self._eng.max_tokens)
            V = self.hp.n_vocab
            parts = []
            for t0 in range(0, T, cap):
                lg = self._eng.logits(x[t0:t0 + cap].contiguous(), True)
                t = tg[t0:t0 + cap]
                ok = (t >= 0) & (t < V)
                lp, ti, tl = self.logprobs(
                    lg, range(lg.shape[0]),
                    torch.where(ok, t, torch.zeros_like(t)), 1)
                parts.append((torch.where(ok, lp, torch.full_like(
                    lp, float("nan"))), ti[:, 0], tl[:, 0]))
        if len(parts) == 1:
            return parts[0]
        return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


class TorchSliceEngine:
    """CPU twin with the identical stateless interface (fp32 torch math).

    Used for CPU tests, the gloo pipeline path, and machines without a GPU.
    Never selected automatically when CUDA is available — the HIP engine is
    the only GPU path.
    """

    def __init__(self, hp: ggml.Hparams, weights: Dict[str, torch.Tensor],
                 n_layers: int, first_layer: int, n_ctx: int = 512,
                 max_batch: int = 4, device: str = "cpu"):
        self.hp = hp
        self.w = weights
        self.first_layer = first_layer
        self.n_layers = n_layers
        self.n_ctx = n_ctx
        self.max_batch = max_batch
        self.device = device
        d = hp.head_dim
        hkv = hp.kv_heads
        self.k_cache = torch.zeros(n_layers, max_batch, n_ctx, hkv, d)
        self.v_cache = torch.zeros(n_layers, max_batch, n_ctx, hkv, d)
        self.has_extra = all(
            k in weights for k in
            ("tok_embeddings.weight", "norm.weight", "output.weight"))

    @classmethod
    def from_ggml(cls, f: ggml.GGMLFile, n_ctx: int = 512,
                  max_batch: int = 4) -> "TorchSliceEngine":
        from ..models.llama import weights_from_ggml
        hp = f.hparams
        first = hp.first_layer if hp.first_layer is not None else 0
        return cls(hp, weights_from_ggml(f), hp.n_layer, first, n_ctx,
                   max_batch)

    def attach_extra(self, f: ggml.GGMLFile) -> None:
        from ..models.llama import weights_from_ggml
        self.w.update(weights_from_ggml(f))
        self.has_extra = True

    def forward(self, x: torch.Tensor, pos: torch.Tensor,
                seq: torch.Tensor, decode: bool = False) -> torch.Tensor:
        hp = self.hp
        T, E = x.shape
        h, d = hp.n_head, hp.head_dim
        hkv = hp.kv_heads
        kv_map = torch.arange(h) // (h // hkv)  # GQA head sharing
        pos_l = pos.tolist()
        seq_l = seq.tolist()
        for li in range(self.n_layers):
            gi = li + self.first_layer
            pre = f"layers.{gi}."
            a = rms_norm(x) * self.w[pre + "attention_norm.weight"]
            q = a @ self.w[pre + "attention.wq.weight"].T
            k = a @ self.w[pre + "attention.wk.weight"].T
            v = a @ self.w[pre + "attention.wv.weight"].T
            o = torch.empty_like(x)
            for t in range(T):  # per-row positions (prefill/decode unified)
                p, b = pos_l[t], seq_l[t]
                qt = rope_interleaved(q[t:t + 1].view(1, h, d), p)[0]
                kt = rope_interleaved(k[t:t + 1].view(1, hkv, d), p)[0]
                self.k_cache[li, b, p] = kt
                self.v_cache[li, b, p] = v[t].view(hkv, d)
                keys = self.k_cache[li, b, :p + 1][:, kv_map]
                vals = self.v_cache[li, b, :p + 1][:, kv_map]
                att = torch.einsum("hd,jhd->hj", qt, keys) / math.sqrt(d)
                prob = torch.softmax(att, dim=-1)
                o[t] = torch.einsum("hj,jhd->hd", prob, vals).reshape(E)
            x = x + o @ self.w[pre + "attention.wo.weight"].T
            f = rms_norm(x) * self.w[pre + "ffn_norm.weight"]
            g = torch.nn.functional.silu(
                f @ self.w[pre + "feed_forward.w1.weight"].T)
            u = f @ self.w[pre + "feed_forward.w3.weight"].T
            x = x + (g * u) @ self.w[pre + "feed_forward.w2.weight"].T
        return x

    def embed(self, tokens: torch.Tensor) -> torch.Tensor:
        idx = tokens.to(torch.long)
        return self.w["tok_embeddings.weight"][idx]

    def logits(self, x: torch.Tensor, all_logits: bool = False) -> torch.Tensor:
        y = rms_norm(x) * self.w["norm.weight"]
        lg = y @ self.w["output.weight"].T
        return lg if all_logits else lg[-1:]

    def argmax(self, lg: torch.Tensor) -> torch.Tensor:
        return lg.argmax(dim=-1).to(torch.int32)

    # ---- sampling twin: same interface as HIPSliceEngine, float64
    # sample_reference per row, seen state as a plain bool tensor ----

    def new_seen_state(self, n_slots: Optional[int] = None) -> torch.Tensor:
        n = self.max_batch if n_slots is None else int(n_slots)
        return torch.zeros(n, self.hp.n_vocab, dtype=torch.bool)

    def reset_seen(self, seen: torch.Tensor, slot: int) -> None:
        seen[slot].zero_()

    def sample(self, lg: torch.Tensor, rows, slots, u, temperature,
               repeat_penalty, top_k, top_p,
               seen: torch.Tensor) -> torch.Tensor:
        from .sampler import sample_reference
        if len(set(int(s) for s in slots)) != len(rows):
            raise ValueError("sample: slots must be distinct")
        lg64 = lg.detach().to(torch.float64).numpy()
        out = []
        for r in range(len(rows)):
            slot = int(slots[r])
            prev = torch.nonzero(seen[slot]).reshape(-1).numpy()
            tid, _ = sample_reference(
                lg64[int(rows[r])], float(u[r]), prev,
                float(temperature[r]), float(repeat_penalty[r]),
                int(top_k[r]), float(top_p[r]))
            seen[slot, tid] = True
            out.append(tid)
        return torch.tensor(out, dtype=torch.int32)

    def logprobs(self, lg: torch.Tensor, rows, ids: torch.Tensor,
                 top_n: int = 0):
        """Twin of HIPSliceEngine.logprobs: float64 logprobs_reference
        per row, rounded to the f32 / i32 result tensors."""
        from .sampler import logprobs_reference
        R = len(rows)
        top_n = int(top_n)
        if R == 0 or ids.dim() != 1 or ids.shape[0] != R:
            raise ValueError("logprobs: rows and ids must share one "
                             "non-zero length")
        if min(rows) < 0 or max(rows) >= lg.shape[0]:
            raise ValueError("logprobs: row index out of range")
        if not 0 <= top_n <= LOGPROBS_MAX_TOP:
            raise ValueError(
                f"logprobs: top_n must be in 0..{LOGPROBS_MAX_TOP}")
        if top_n > lg.shape[1]:
            raise ValueError("logprobs: top_n exceeds the vocabulary")
        lg64 = lg.detach().to(torch.float64).numpy()
        lp = np.empty(R, dtype=np.float32)
        top_ids = np.empty((R, top_n), dtype=np.int32)
        top_lp = np.empty((R, top_n), dtype=np.float32)
        for r in range(R):
            lp[r], top_ids[r], top_lp[r] = logprobs_reference(
                lg64[int(rows[r])], int(ids[r]), top_n)
        return (torch.from_numpy(lp), torch.from_numpy(top_ids),
                torch.from_numpy(top_lp))

    def score(self, x: torch.Tensor, targets):
        """Twin of HIPSliceEngine.score: f32 logits, f32 `log_softmax` and
        a gather (the arithmetic of the perplexity command); the arg-max
        takes the smaller index on a tie."""
        if x.dim() != 2 or x.shape[0] < 1:
            raise ValueError("score: x must be [T, E] with T >= 1")
        if isinstance(targets, torch.Tensor):
            tg = targets.detach().cpu().numpy()
        else:
            tg = np.asarray(targets)
        tg = tg.astype(np.int64).reshape(-1)
        if tg.shape[0] != x.shape[0]:
            raise ValueError("score: one target per row of x")
        lg = self.logits(x, all_logits=True)
        logp = torch.log_softmax(lg.float().cpu(), dim=-1).numpy()
        rows = np.arange(len(tg))
        ok = (tg >= 0) & (tg < logp.shape[1])
        lp = np.full(len(tg), np.nan, dtype=np.float32)
        lp[ok] = logp[rows[ok], tg[ok]]
        # numpy's argmax returns the first (smallest) index of the maximum
        top_id = lg.float().cpu().numpy().argmax(axis=1)
        top_lp = logp[rows, top_id]
        return (torch.from_numpy(lp),
                torch.from_numpy(top_id.astype(np.int32)),
                torch.from_numpy(top_lp.astype(np.float32)))


def engine_for_slice(f: ggml.GGMLFile, n_ctx: int, max_batch: int,
                     device: Optional[str] = None):
    """Pick the engine for this machine: HIP when a GPU is present."""
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if device == "cuda":
        return HIPSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=max_batch)
    return TorchSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=max_batch)
