#!/usr/bin/env python3
"""Prompt scoring, two routes over the same prefill output y [T, E]:

  (a) parent   what `manager.py perplexity` ran before score() existed:
               logits(y, all_logits=True) in 64-row tiles, the [T, V] f32
               logits copied to the host, log_softmax and the gather there
  (b) score    eng.score(y, targets): k_lmhead_score + k_score_finish, T
               floats copied back

Both end in the same float: exp(mean NLL). The forward that produces y is
common to the two routes and is not timed (--layers keeps it small). The
routes alternate, --runs times each, with a device synchronisation before
and after every timed region. One JSON line per prompt length."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import json
import time

import numpy as np
import torch

from distributedllm_amd.engine import HIPSliceEngine
from distributedllm_amd.formats import ggml
from distributedllm_amd.models.llama import PRESETS

FTYPES = {"q4_0": ggml.FTYPE_MOSTLY_Q4_0, "q8_0": ggml.FTYPE_MOSTLY_Q8_0,
          "f16": ggml.FTYPE_MOSTLY_F16}


def route_parent(eng, y, targets):
    lg = eng.logits(y, all_logits=True)
    logp = torch.log_softmax(lg.float().cpu(), dim=-1).numpy()
    nll = [-logp[i, targets[i]] for i in range(len(targets))]
    return float(np.exp(np.mean(nll)))


def route_score(eng, y, targets):
    lp, _, _ = eng.score(y, targets)
    return float(np.exp(np.mean(-lp.float().cpu().numpy())))


def timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v = fn(*a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, v


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="open_llama_3b")
    ap.add_argument("--ftype", default="q4_0", choices=list(FTYPES))
    ap.add_argument("--lengths", default="512,2048",
                    help="prompt lengths (tokens scored = length - 1)")
    ap.add_argument("--layers", type=int, default=1,
                    help="transformer layers of the untimed forward")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    p = PRESETS[args.model]
    hp = p.hparams(FTYPES[args.ftype])
    lengths = [int(s) for s in args.lengths.split(",")]
    ctx = max(lengths)
    eng = HIPSliceEngine.random(hp, n_layers=args.layers, n_ctx=ctx,
                                max_batch=1, seed=0, with_extra=True,
                                max_prefill=ctx)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for n in lengths:
        toks = torch.randint(3, hp.n_vocab, (n,), dtype=torch.int32,
                             device="cuda", generator=g)
        T = n - 1
        pos = torch.arange(T, dtype=torch.int32, device="cuda")
        seq = torch.zeros(T, dtype=torch.int32, device="cuda")
        y = eng.forward(eng.embed(toks[:-1]), pos, seq).contiguous()
        targets = toks[1:].cpu().tolist()
        for _ in range(args.warmup):
            route_parent(eng, y, targets)
            route_score(eng, y, targets)
        ms = {"parent": [], "score": []}
        val = {}
        for _ in range(args.runs):
            for name, fn in (("parent", route_parent),
                             ("score", route_score)):
                t, val[name] = timed(fn, eng, y, targets)
                ms[name].append(round(t, 3))
        out = {"model": p.name, "ftype": args.ftype, "prompt_len": n,
               "rows": T, "runs": args.runs}
        for name in ms:
            out[name + "_ms"] = ms[name]
            out[name + "_ms_mean"] = round(float(np.mean(ms[name])), 3)
            out[name + "_ppl"] = val[name]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
