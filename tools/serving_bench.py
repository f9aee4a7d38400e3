#!/usr/bin/env python3
"""Continuous-batching serving benchmark (GPU): N requests with random
prompts served concurrently through serving.ContinuousBatcher on one
engine — measures end-to-end serving tokens/s including scheduling,
logits and sampling (bench.py measures the raw decode pipeline)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))

import torch

from distributedllm_amd.engine import HIPSliceEngine
from distributedllm_amd.engine.sampler import Sampler
from distributedllm_amd.formats import ggml
from distributedllm_amd.models.llama import PRESETS
from distributedllm_amd.serving import ContinuousBatcher


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="open_llama_3b")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--prompt-len", type=int, default=32)
    ap.add_argument("--num-tokens", type=int, default=64)
    ap.add_argument("--slots", type=int, default=64,
                    help="KV slots per lane")
    ap.add_argument("--lanes", type=int, default=1,
                    help="concurrent stream lanes (weight-sharing "
                         "clones); total slots = slots x lanes")
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--prefill-chunk", type=int, default=0,
                    help="chunked-prefill bound (0 = unbounded)")
    ap.add_argument("--long-requests", type=int, default=0,
                    help="long-prompt requests arriving mid-run (QoS "
                         "experiment: how much do they stall in-flight "
                         "decodes?)")
    ap.add_argument("--long-prompt", type=int, default=512)
    ap.add_argument("--speculate", type=int, default=0,
                    help="in-batcher prompt-lookup speculation (greedy "
                         "requests, K drafts; token-exact). NOTE: "
                         "random-init synthetic text repeats "
                         "unrealistically often — acceptance rates here "
                         "overstate real-text gains")
    ap.add_argument("--temperature", type=float, default=None,
                    help="sample every request at this temperature "
                         "(default: greedy device argmax)")
    ap.add_argument("--repeat-penalty", type=float, default=1.1)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0,
                    help="request i samples with seed + i")
    ap.add_argument("--device-sampling", action="store_true",
                    help="sample on the GPU (one batched launch per lane "
                         "and step) instead of the per-request host "
                         "Sampler over logits copied to the host")
    ap.add_argument("--logprobs", type=int, default=None,
                    help="ask for per-token log-probabilities with this "
                         "many top alternatives (0..8) on every request "
                         "(default: off)")
    args = ap.parse_args()
    if args.device_sampling and args.temperature is None:
        ap.error("--device-sampling needs --temperature")

    hp = PRESETS[args.model].hparams(ggml.FTYPE_MOSTLY_Q4_0)
    eng = HIPSliceEngine.random(hp, n_layers=hp.n_layer, n_ctx=args.ctx,
                                max_batch=args.slots, with_extra=True)
    lanes = None
    if args.lanes > 1:
        lanes = [eng] + [eng.clone_shared()
                         for _ in range(args.lanes - 1)]
    g = torch.Generator().manual_seed(1)
    bat = ContinuousBatcher(eng, engines=lanes,
                            prefill_chunk=args.prefill_chunk or None,
                            spec_ngram=3 if args.speculate else 0,
                            spec_k=args.speculate,
                            device_sampling=args.device_sampling)
    n_sub = [0]

    def sampler():
        """Per-request sampler (None = greedy), seeded seed + i."""
        if args.temperature is None:
            return None
        n_sub[0] += 1
        return Sampler(args.temperature, args.repeat_penalty,
                       seed=args.seed + n_sub[0] - 1, top_k=args.top_k,
                       top_p=args.top_p)

    reqs = [bat.submit(torch.randint(3, hp.n_vocab, (args.prompt_len,),
                                     generator=g).tolist(),
                       args.num_tokens, sampler=sampler(),
                       logprobs=args.logprobs)
            for _ in range(args.requests)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 0
    done_at = {}
    long_at = max(1, args.num_tokens // 4)
    stalls = []  # per-step wall time after the long arrivals
    while bat.pending:
        ts = time.perf_counter()
        fin = bat.step()
        if fin:
            torch.cuda.synchronize()
            now = time.perf_counter() - t0
            for r in fin:
                done_at[r.rid] = now
        steps += 1
        if args.long_requests and steps >= long_at:
            torch.cuda.synchronize()
            stalls.append(time.perf_counter() - ts)
        if args.long_requests and steps == long_at:
            for _ in range(args.long_requests):
                reqs.append(bat.submit(
                    torch.randint(3, hp.n_vocab, (args.long_prompt,),
                                  generator=g).tolist(), args.num_tokens,
                    sampler=sampler(), logprobs=args.logprobs))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    total = sum(len(r.out) for r in reqs)
    lat = sorted(done_at.values())
    p = lambda q: lat[min(len(lat) - 1, int(q * len(lat)))]
    mode = "greedy" if args.temperature is None else (
        f"sampled on {'device' if args.device_sampling else 'host'} "
        f"T={args.temperature} rp={args.repeat_penalty} "
        f"top_k={args.top_k} top_p={args.top_p}")
    mode += (", logprobs off" if args.logprobs is None
             else f", logprobs on (top {args.logprobs})")
    if args.logprobs is not None:
        assert all(len(r.out_logprobs) == len(r.out) for r in reqs)
    print(f"[{mode}] "
          f"{args.requests} requests x {args.num_tokens} new tokens "
          f"(prompt {args.prompt_len}, {bat.n_slots} slots on "
          f"{len(bat.lanes)} lanes): "
          f"{total} tokens in {dt:.2f}s = {total/dt:.0f} tok/s, "
          f"{steps} decode steps; completion p50={p(0.5):.2f}s "
          f"p95={p(0.95):.2f}s max={lat[-1]:.2f}s")
    if stalls:
        ss = sorted(stalls)
        print(f"per-step wall after long arrivals (stall = decode "
              f"starvation): p50={ss[len(ss)//2]*1e3:.0f}ms "
              f"max={ss[-1]*1e3:.0f}ms over {len(ss)} steps "
              f"(chunk={args.prefill_chunk or 'unbounded'})")


if __name__ == "__main__":
    main()
