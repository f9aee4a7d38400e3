#!/usr/bin/env python3
"""Flagship benchmark: OpenLLaMA-3B q4_0 batched decode, layer-sliced
across N MI355X GPUs (RCCL pipeline stages over xGMI).

Driver contract: `python bench.py --gpus N --steps K --warmup W`; for N>1
launched via torch.distributed.run with one rank per GPU. Rank 0 prints one
JSON line with the whole-job tokens/sec.

Metric: tokens generated per second across the whole node (every sequence
advances one token per step; tokens/step = global_batch). Weak scaling:
global batch = 64 sequences per micro-batch x k stream lanes x N stages,
so per-GPU work per step is constant as N grows (each stage holds ~L/N
layers but serves N micro-batches per lane per step). Synthetic setup: random-init weights of the real
architecture generated directly on-device in the engine's q4_0 layout
(identical compute + HBM traffic to a real checkpoint; no network for real
weights — BASELINE.md).

A plain run does only what the headline needs: set up, fill the KV, warm
up, time `--steps` steps, print the JSON line. `--dump-outputs DIR` also
writes what the last timed step computed (DIR/tokens.npy, hidden.npy,
logits.npy, float32) so two builds can be compared output for output:
weights and start tokens both derive from `--seed`, so equal arguments
give equal inputs. `--full` is where measurements beyond the headline belong
(none exist yet: every figure of the result line comes from the timed
steps themselves).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

from distributedllm_amd.formats import ggml
from distributedllm_amd.models.llama import PRESETS
from distributedllm_amd.parallel.pipeline import (
    DecodePipeline, PipelineConfig, partition_layers, timed_decode)

FTYPES = {"q4_0": ggml.FTYPE_MOSTLY_Q4_0, "q4_1": ggml.FTYPE_MOSTLY_Q4_1,
          "q5_0": ggml.FTYPE_MOSTLY_Q5_0, "q5_1": ggml.FTYPE_MOSTLY_Q5_1,
          "q8_0": ggml.FTYPE_MOSTLY_Q8_0,
          # k-quants ride the W_Q8B/W_Q8B16 byte streams in HBM (1 B
          # per weight + scale planes), so their decode throughput is
          # the byte-path number regardless of the smaller disk size
          "q2_K": ggml.FTYPE_MOSTLY_Q2_K, "q3_K": ggml.FTYPE_MOSTLY_Q3_K_M,
          "q4_K": ggml.FTYPE_MOSTLY_Q4_K_M,
          "q5_K": ggml.FTYPE_MOSTLY_Q5_K_M, "q6_K": ggml.FTYPE_MOSTLY_Q6_K,
          "f16": ggml.FTYPE_MOSTLY_F16, "f32": ggml.FTYPE_ALL_F32}

DUMP_BUDGET = 64 * 10**6  # bytes, all --dump-outputs files together


def dump_outputs(pipe: DecodePipeline, out_dir: str) -> None:
    """Write what the last timed step handed its caller, as float32 .npy:
    rank 0 the sampled token ids [global_batch]; the last rank the final
    hidden state [global_batch, E] and the logits [global_batch, V] those
    ids were sampled from (rows in micro-batch order). An array over its
    share of DUMP_BUDGET keeps a fixed, seeded sample of its rows."""
    import numpy as np
    arrays = {}
    if pipe.is_first:
        arrays["tokens"] = pipe.current_tokens().reshape(-1)
    if pipe.is_last:
        arrays["hidden"] = torch.cat([o[0] for o in pipe.last_out])
        arrays["logits"] = torch.cat([o[1] for o in pipe.last_out])
    os.makedirs(out_dir, exist_ok=True)
    # the token ids (4 bytes per sequence) may live on another rank
    budget = DUMP_BUDGET - 4 * pipe.cfg.global_batch
    for name, t in arrays.items():
        a = t.detach().to("cpu", torch.float32).numpy()
        if name != "tokens":
            if a.nbytes > budget:
                rows = max(1, budget // (a.nbytes // a.shape[0]))
                keep = np.random.default_rng(0).choice(
                    a.shape[0], size=rows, replace=False)
                a = a[np.sort(keep)]
            budget -= a.nbytes
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--model", default="open_llama_3b")
    ap.add_argument("--ftype", default="q4_0", choices=list(FTYPES))
    ap.add_argument("--mbs", type=int, default=None,
                    help="sequences per micro-batch (default 64 = one "
                         "engine decode tile; decode is HBM-bound so "
                         "tokens/s scales ~linearly with batch). When "
                         "the KV fit forces a single lane and --mbs is "
                         "not given, the lane auto-widens (WIDE decode: "
                         "one T-token forward pays the weight stream "
                         "once for the whole batch)")
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--lanes", "--single-gpu-mbs", dest="lanes",
                    type=int, default=5,
                    help="concurrent stream lanes per GPU (weight-"
                         "sharing engine clones, one HIP stream each; "
                         "with N>1 GPUs each lane is a full pipeline). "
                         "Auto-capped by HBM fit; 5 measured best on "
                         "3B: +47%% over one stream, 6 regresses")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--backend", default="auto",
                    choices=["auto", "nccl", "gloo"],
                    help="auto = nccl(RCCL) on GPU, gloo on CPU. "
                         "gloo + GPU = host-staged hops: lets world>1 "
                         "run on ONE physical GPU (RCCL refuses "
                         "duplicate devices) for pipeline shakeout")
    ap.add_argument("--prefill-depth", type=int, default=512,
                    help="untimed decode steps that fill the KV before "
                         "timing, so the headline is a steady-state "
                         "number over a ~this-deep KV, not a cold-cache "
                         "one (VERDICT r1). 0 = shallow/cold timing")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's "
                         "outputs (token ids, final hidden state, "
                         "logits) to DIR/<name>.npy as float32, at most "
                         "64 MB in all; same arguments = same inputs, "
                         "so two builds can be compared array by array")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements that are not part "
                         "of the headline figure (baselines, other "
                         "precisions or sizes, reference comparisons). "
                         "None exist yet, so this adds nothing to a "
                         "plain run; new ones go behind this flag")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = max(args.gpus, world)

    import torch.distributed as dist
    device = "cuda" if torch.cuda.is_available() else "cpu"
    # --steps is never cut short (only the untimed prefill shrinks to
    # fit, below), so a run that would step past the KV cache even with
    # no prefill is refused before anything is allocated
    cap_steps = 2 if device == "cuda" else 0  # capture_graphs' warmup
    if cap_steps + args.warmup + args.steps > args.ctx:
        ap.error(f"--warmup {args.warmup} + --steps {args.steps} (+ "
                 f"{cap_steps} graph-capture steps) exceed --ctx "
                 f"{args.ctx}")
    backend = ("nccl" if device == "cuda" else "gloo") \
        if args.backend == "auto" else args.backend
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    if device == "cuda":
        # modulo: lets world=2 share one GPU (RCCL-path shakeout on a
        # 1-GPU box) while the driver's 8-GPU launch maps 1:1
        torch.cuda.set_device(local_rank % torch.cuda.device_count())

    preset = PRESETS[args.model]
    hp = preset.hparams(FTYPES[args.ftype])
    parts = partition_layers(preset.n_layer, world)
    first, count = parts[rank]

    # Concurrency structure:
    #  * world > 1: one pipeline lane = `world` micro-batches in flight
    #    (keeps every stage busy); k lanes run concurrently per rank on
    #    separate HIP streams over SHARED weights (weight-sharing engine
    #    clones, one per lane), so each GPU gets the same multi-stream
    #    overlap the single-GPU config has.
    #  * world == 1: k lanes of one micro-batch each.
    # Weak scaling: global batch grows with N, per-GPU work fixed.
    # Lane count: 2 streams measured a net LOSS on every model
    # (contention without enough overlap) while 3-5 won, so multi-stream
    # only when >=3 lanes' KV sets fit in HBM next to the model weights
    # (~260 GB usable of 288). All ranks must agree on k: size with the
    # largest per-rank slice (rank 0 holds the most layers).
    mbs_explicit = args.mbs is not None
    if args.mbs is None:
        args.mbs = 64
    n_lanes = args.lanes
    if n_lanes > 1:
        max_layers = parts[0][1]
        kv_bytes = (max_layers * world * args.mbs * args.ctx *
                    preset.n_embd * 4)  # per-lane clone, f16 K+V
        E, F, V = preset.n_embd, preset.n_ff, 32000
        n_weights = (max_layers * (4 * E * E + 3 * E * F) + 2 * V * E)
        bpw = {"q4_0": 0.5625, "q4_1": 0.625, "q5_0": 1.125,
               "q5_1": 1.125, "q8_0": 1.125,
               "q2_K": 1.25, "q3_K": 1.25, "q4_K": 1.125, "q5_K": 1.125,
               "q6_K": 1.25, "f16": 2.0,
               "f32": 4.0}[args.ftype]  # HBM-resident bytes/weight
        #         (byte formats incl. k-quants: 1B + scale planes)
        w_bytes = n_weights * bpw * 1.1  # repack padding/scales margin
        fit = max(1, int((260e9 - w_bytes) // max(kv_bytes, 1)))
        if fit >= n_lanes:
            pass                      # explicit/default count fits
        elif fit >= 3:
            n_lanes = fit             # auto-shrink (3-5 measured best)
        else:
            n_lanes = 1               # 2 lanes always lost at mbs 64
            if device == "cuda" and not mbs_explicit:
                # WIDE single-lane decode (BASELINE.md WIDE rows): use
                # the KV room for one wide batch instead of stream
                # lanes — measured +14-45% on the 7B-70B ladder
                per_seq = kv_bytes // max(args.mbs, 1)
                wide = int((260e9 - w_bytes) // max(per_seq, 1))
                args.mbs = max(args.mbs,
                               min(320, (wide // 64) * 64))
    n_mb = n_lanes * max(world, 1) if world > 1 else n_lanes
    cfg = PipelineConfig(mbs=args.mbs, n_mb=n_mb, device=device)

    engines = None
    if device == "cuda":
        from distributedllm_amd.engine import HIPSliceEngine
        # each lane clone holds KV for its lane's in-flight micro-
        # batches: `world` of them per lane (1 on a single GPU)
        slots = args.mbs * (n_mb // n_lanes)
        eng = HIPSliceEngine.random(hp, n_layers=count, first_layer=first,
                                    n_ctx=args.ctx, max_batch=slots,
                                    seed=args.seed, with_extra=True)
        if n_lanes > 1:
            engines = [eng] + [eng.clone_shared()
                               for _ in range(n_lanes - 1)]
    else:  # CPU fallback so the contract is testable without a GPU
        from distributedllm_amd.engine import TorchSliceEngine
        from distributedllm_amd.formats import synthetic
        from distributedllm_amd.models.llama import weights_from_ggml
        tiny = PRESETS["tiny"]
        hp = tiny.hparams(FTYPES[args.ftype])
        parts = partition_layers(tiny.n_layer, world)
        first, count = parts[rank]
        f = synthetic.build_model(tiny, seed=args.seed,
                                  ftype=ggml.FTYPE_MOSTLY_F16)
        w = weights_from_ggml(f)
        eng = TorchSliceEngine(hp, w, n_layers=count, first_layer=first,
                               n_ctx=args.ctx, max_batch=cfg.global_batch)
        preset = tiny

    if device == "cpu":
        # the CPU path exists to keep the driver contract testable; a
        # deep steady-state KV is a GPU-measurement concern
        args.prefill_depth = min(args.prefill_depth, 8)
    # KV-depth guard: prefill + warmup + steps all advance positions —
    # and so do capture_graphs' 2 eager warmup steps on the CUDA path
    # (at a clamped-to-ctx config, forgetting them writes the last KV
    # rows at pos >= n_ctx: out of bounds)
    depth_end = cap_steps + args.prefill_depth + args.warmup + args.steps
    if depth_end > args.ctx:
        args.prefill_depth = max(0, args.ctx - args.warmup - args.steps
                                 - cap_steps)
        depth_end = (cap_steps + args.prefill_depth + args.warmup +
                     args.steps)
    # the pipeline draws its start tokens from torch's global generator,
    # which a fresh process seeds at random: pin it so equal arguments
    # give equal inputs
    torch.manual_seed(args.seed)
    pipe = DecodePipeline(eng, cfg, rank=rank, world=world,
                          engines=engines)
    pipe.keep_outputs = args.dump_outputs is not None
    # the prefill steps run as extra (graph-replayed) warmup: real decode
    # work filling the KV with real activations — nothing in the timed
    # region is skipped or cached, it just starts at a stated depth
    # DLLM_NO_GRAPH=1: eager launches instead of hipGraph replay —
    # needed under rocprofv3 --pmc (per-dispatch counter instrumentation
    # crashes on graph-replayed kernels); timing loses the launch-bound
    # overlap, so only use for counter collection, not headline numbers
    elapsed = timed_decode(
        pipe, args.steps, args.warmup + args.prefill_depth, device,
        use_graphs=os.environ.get("DLLM_NO_GRAPH", "0") != "1")

    # MAX over ranks
    t = torch.tensor([elapsed], dtype=torch.float64,
                     device=device if backend == "nccl" else "cpu")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    if args.dump_outputs is not None:
        dump_outputs(pipe, args.dump_outputs)

    tokens = args.steps * cfg.global_batch
    toks_per_s = tokens / elapsed
    if rank == 0:
        result = {
            "metric": "tokens/sec (whole node), "
                      f"{preset.name} {args.ftype} sliced across "
                      f"{n_gpus} MI355X",
            "value": round(toks_per_s, 2),
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.ftype,
            "data": "synthetic (random-init weights, random prompt ids)",
            "config": {
                "model": preset.name,
                "global_batch": cfg.global_batch,
                "seq_len": depth_end,
                "prefill_depth": args.prefill_depth,
                "kv_depth_timed": [depth_end - args.steps, depth_end],
                "n_ctx": args.ctx,
                "parallelism": f"pp{n_gpus}",
                "micro_batches": n_mb,
                "lanes": n_lanes,
                "mbs": args.mbs,
                "device": device,
                "backend": backend if world > 1 else None,
            },
        }
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
