"""Pipeline correctness: gloo 2-rank layer-sliced decode == single engine.

Runs here on CPU (world_size=2, backend gloo, 127.0.0.1 rendezvous); the
same DecodePipeline code path is what bench.py runs over RCCL on GPUs.
"""
import json
import multiprocessing as mp
import os

import pytest
import torch

from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.formats import slicer, synthetic
from distributedllm_amd.parallel.pipeline import (
    DecodePipeline, PipelineConfig, partition_layers)

STEPS = 3
MBS = 2


def test_partition_layers():
    assert partition_layers(26, 8) == [
        (0, 4), (4, 4), (8, 3), (11, 3), (14, 3), (17, 3), (20, 3), (23, 3)]
    assert partition_layers(3, 1) == [(0, 3)]
    assert partition_layers(4, 2) == [(0, 2), (2, 2)]


SEEDS = [[5, 9], [11, 3], [4, 8], [13, 2],
         [6, 1], [9, 7], [2, 12], [10, 5]]  # start tokens per micro-batch


def _seed_tokens(pipe, n_mb):
    for m in range(n_mb):
        pipe.tok[m] = torch.tensor(SEEDS[m], dtype=torch.int32)


def _single_reference_tokens(n_mb=1, n_layer=None):
    f = synthetic.build_model("tiny", seed=0, n_layer=n_layer)
    ex = slicer.make_extra_layers(f)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=MBS * n_mb)
    eng.attach_extra(ex)
    cfg = PipelineConfig(mbs=MBS, n_mb=n_mb, device="cpu")
    pipe = DecodePipeline(eng, cfg, rank=0, world=1)
    _seed_tokens(pipe, n_mb)
    pipe.run_steps(STEPS)
    return pipe.current_tokens().tolist()


def _rank_main(rank, world, port, n_mb, q, n_lanes=1, n_layer=None):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    f = synthetic.build_model("tiny", seed=0, n_layer=n_layer)
    ex = slicer.make_extra_layers(f)
    parts = partition_layers(f.hparams.n_layer, world)
    first, count = parts[rank]
    sl = slicer.make_slice(f, first, first + count - 1)
    per_lane = MBS * ((n_mb + n_lanes - 1) // n_lanes)
    engines = None
    if n_lanes > 1:
        engines = []
        for _ in range(n_lanes):
            e = TorchSliceEngine.from_ggml(sl, n_ctx=32,
                                           max_batch=per_lane)
            e.attach_extra(ex)
            engines.append(e)
        eng = engines[0]
    else:
        eng = TorchSliceEngine.from_ggml(sl, n_ctx=32,
                                         max_batch=MBS * n_mb)
        eng.attach_extra(ex)
    cfg = PipelineConfig(mbs=MBS, n_mb=n_mb, device="cpu")
    pipe = DecodePipeline(eng, cfg, rank=rank, world=world,
                          engines=engines)
    _seed_tokens(pipe, n_mb)
    pipe.run_steps(STEPS)
    if rank == 0:
        q.put(pipe.current_tokens().tolist())
    dist.destroy_process_group()


def _run_cluster(world, port, n_mb, n_lanes=1, n_layer=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main,
                         args=(r, world, port, n_mb, q, n_lanes, n_layer))
             for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=100)
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    return got


@pytest.mark.timeout(120)
def test_two_stage_pipeline_matches_single():
    assert _run_cluster(2, 29531, 1) == _single_reference_tokens(1)


@pytest.mark.timeout(120)
def test_two_stage_overlapped_micro_batches_match():
    """n_mb=2 exercises the overlapped isend/irecv driver: stage 0
    computes micro-batch 1 while micro-batch 0's activations are in
    flight."""
    assert _run_cluster(2, 29532, 2) == _single_reference_tokens(2)


def _rank_gen(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from distributedllm_amd.parallel.pipeline import pipeline_generate
    f = synthetic.build_model("tiny", seed=0)
    ex = slicer.make_extra_layers(f)
    parts = partition_layers(f.hparams.n_layer, world)
    first, count = parts[rank]
    sl = slicer.make_slice(f, first, first + count - 1) if world > 1 else f
    eng = TorchSliceEngine.from_ggml(sl, n_ctx=32, max_batch=MBS)
    eng.attach_extra(ex)
    cfg = PipelineConfig(mbs=MBS, n_mb=1, device="cpu")
    pipe = DecodePipeline(eng, cfg, rank=rank, world=world)
    toks = pipeline_generate(pipe, [5, 9, 3], max_steps=4)
    if rank == 0:
        q.put(toks.tolist())
    dist.destroy_process_group()


def _single_generate_reference():
    f = synthetic.build_model("tiny", seed=0)
    ex = slicer.make_extra_layers(f)
    from distributedllm_amd.parallel.pipeline import pipeline_generate
    eng = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=MBS)
    eng.attach_extra(ex)
    cfg = PipelineConfig(mbs=MBS, n_mb=1, device="cpu")
    pipe = DecodePipeline(eng, cfg, rank=0, world=1)
    return pipeline_generate(pipe, [5, 9, 3], max_steps=4).tolist()


def test_multi_engine_micro_batches_match_shared_engine():
    """Per-micro-batch engine clones (bench.py's single-GPU multi-stream
    mode) use LOCAL sequence ids into each clone's own KV cache; the
    decoded tokens must be identical to one shared engine partitioning
    its KV slots across micro-batches. On CPU this runs the same
    DecodePipeline code minus the per-stream scheduling."""
    f = synthetic.build_model("tiny", seed=0)
    ex = slicer.make_extra_layers(f)
    n_mb = 2
    engines = []
    for _ in range(n_mb):
        e = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=MBS)
        e.attach_extra(ex)
        engines.append(e)
    cfg = PipelineConfig(mbs=MBS, n_mb=n_mb, device="cpu")
    pipe = DecodePipeline(engines[0], cfg, rank=0, world=1,
                          engines=engines)
    assert pipe.seq[1].tolist() == [0, 1]  # local ids, not [2, 3]
    _seed_tokens(pipe, n_mb)
    pipe.run_steps(STEPS)
    assert pipe.current_tokens().tolist() == _single_reference_tokens(n_mb)


@pytest.mark.timeout(120)
def test_two_stage_two_lane_pipeline_matches_single():
    """2 ranks x 2 lanes (weight-sharing clones per rank, n_mb=4):
    micro-batch m runs on lane m%2 with lane-local KV slots; tokens
    must match one engine running all 4 micro-batches."""
    assert _run_cluster(2, 29534, 4, n_lanes=2) == \
        _single_reference_tokens(4)


@pytest.mark.timeout(120)
def test_pipeline_generate_prompt_conditioned():
    """Prefill + greedy decode through 2 pipeline stages must produce the
    same continuations as the single-engine pipeline."""
    ref = _single_generate_reference()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_gen, args=(r, 2, 29533, q))
             for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=100)
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    assert got == ref
    # both sequences of a micro-batch got identical prompts -> identical
    # greedy continuations; and they continue the prompt deterministically
    assert got[0] == got[1]


@pytest.mark.timeout(180)
def test_bench_driver_contract():
    """`python bench.py --steps K --warmup W` must print exactly one JSON
    line with the driver-contract fields (the round driver parses this)."""
    import subprocess
    import sys
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=150,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in r, key
    assert r["steps"] == 2 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["unit"] == "tokens/s" and r["higher_is_better"] is True
    assert r["scaling"] == "weak" and "synthetic" in r["data"]
    assert r["value"] > 0
    assert {"model", "global_batch", "seq_len",
            "parallelism"} <= set(r["config"])


def _run_bench(*extra, timeout=150):
    import subprocess
    import sys
    return subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", *extra],
        capture_output=True, text=True, timeout=timeout,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.timeout(300)
def test_bench_dump_outputs_reproducible(tmp_path):
    """`--dump-outputs DIR` writes the last timed step's outputs as
    float32 .npy files; two runs with the same arguments (one of them
    with `--full`, which adds nothing to the timed path) write identical
    arrays, and the token ids are the argmax of the dumped logits. A
    shallow KV keeps both runs short on any device."""
    import numpy as np
    small = ["--steps", "3", "--warmup", "1", "--ctx", "64",
             "--prefill-depth", "4"]
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        out = _run_bench(*small, *extra, "--dump-outputs", str(d))
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout
        r = json.loads(lines[0])
        assert r["steps"] == 3 and r["ms_per_step"] > 0
        assert sorted(p.name for p in d.iterdir()) == \
            ["hidden.npy", "logits.npy", "tokens.npy"]
        arrs = {p.stem: np.load(p) for p in d.iterdir()}
        B = r["config"]["global_batch"]
        assert arrs["tokens"].shape == (B,)
        assert arrs["hidden"].shape[0] == B and arrs["hidden"].ndim == 2
        assert arrs["logits"].shape[0] == B and arrs["logits"].ndim == 2
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 10**6
        for a in arrs.values():
            assert a.dtype == np.float32 and np.isfinite(a).all()
        assert np.array_equal(arrs["tokens"],
                              arrs["logits"].argmax(axis=1))
        dumps.append(arrs)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


def test_bench_refuses_steps_past_context():
    """--steps is never cut short: a run whose warmup + timed steps
    cannot fit the KV cache exits with an error instead of stepping
    past it (or quietly timing fewer steps)."""
    out = _run_bench("--steps", "40", "--warmup", "30", "--ctx", "64")
    assert out.returncode != 0
    assert "exceed --ctx" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_pipeline_generate_temperature_sampling():
    """temperature > 0 switches the last rank to softmax sampling:
    deterministic under a fixed torch seed, tokens within vocab, and a
    near-zero temperature reproduces the greedy continuation."""
    from distributedllm_amd.parallel.pipeline import pipeline_generate
    f = synthetic.build_model("tiny", seed=0)
    ex = slicer.make_extra_layers(f)

    def run(temp, seed=123):
        eng = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=MBS)
        eng.attach_extra(ex)
        cfg = PipelineConfig(mbs=MBS, n_mb=1, device="cpu")
        pipe = DecodePipeline(eng, cfg, rank=0, world=1)
        torch.manual_seed(seed)
        return pipeline_generate(pipe, [5, 9, 3], max_steps=4,
                                 temperature=temp).tolist()

    V = f.hparams.n_vocab
    a = run(0.8)
    assert all(0 <= t < V for row in a for t in row)
    assert a == run(0.8)              # same seed -> same sample
    assert run(1e-4) == run(0.0)      # temp -> 0 degenerates to greedy


def test_prime_matches_reference_generation_semantics():
    """pipeline_generate must equal the canonical loop (the TCP client's
    semantics): prefill the prompt, sample from the LAST prompt
    position's logits, then feed only sampled tokens — no duplicated
    last-prompt-token position in KV."""
    from distributedllm_amd.parallel.pipeline import pipeline_generate
    f = synthetic.build_model("tiny", seed=0)
    ex = slicer.make_extra_layers(f)
    prompt, steps = [5, 9, 3], 4

    # canonical single-sequence loop
    eng = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=1)
    eng.attach_extra(ex)
    want = []
    cur, n_past = list(prompt), 0
    for _ in range(steps):
        toks = torch.tensor(cur, dtype=torch.int32)
        pos = torch.arange(n_past, n_past + len(cur), dtype=torch.int32)
        seq = torch.zeros(len(cur), dtype=torch.int32)
        y = eng.forward(eng.embed(toks), pos, seq)
        lg = eng.logits(y[-1:].contiguous(), all_logits=True)
        tid = int(torch.argmax(lg[0]).item())
        want.append(tid)
        n_past += len(cur)
        cur = [tid]

    eng2 = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=MBS)
    eng2.attach_extra(ex)
    cfg = PipelineConfig(mbs=MBS, n_mb=1, device="cpu")
    pipe = DecodePipeline(eng2, cfg, rank=0, world=1)
    got = pipeline_generate(pipe, prompt, max_steps=steps).tolist()
    assert got[0] == want and got[1] == want


def test_prime_with_lane_engines_matches_shared_engine():
    """prime() must write each micro-batch's prompt KV into ITS lane's
    engine (lane-local seq ids) — with 2 lane clones, prompt-conditioned
    generation must equal the single shared-engine pipeline (ADVICE r1:
    prime() previously sent every micro-batch through lane 0)."""
    from distributedllm_amd.parallel.pipeline import pipeline_generate
    f = synthetic.build_model("tiny", seed=0)
    ex = slicer.make_extra_layers(f)
    prompt, steps, n_mb, n_lanes = [5, 9, 3], 4, 4, 2

    def run(lanes):
        if lanes:
            per_lane = MBS * ((n_mb + n_lanes - 1) // n_lanes)
            engines = []
            for _ in range(n_lanes):
                e = TorchSliceEngine.from_ggml(f, n_ctx=32,
                                               max_batch=per_lane)
                e.attach_extra(ex)
                engines.append(e)
            eng = engines[0]
        else:
            engines = None
            eng = TorchSliceEngine.from_ggml(f, n_ctx=32,
                                             max_batch=MBS * n_mb)
            eng.attach_extra(ex)
        cfg = PipelineConfig(mbs=MBS, n_mb=n_mb, device="cpu")
        pipe = DecodePipeline(eng, cfg, rank=0, world=1, engines=engines)
        return pipeline_generate(pipe, prompt, max_steps=steps).tolist()

    assert run(lanes=True) == run(lanes=False)


def test_four_stage_two_lane_pipeline_matches_single():
    """4 ranks x 2 lanes x 8 micro-batches: the deepest posting-order
    stress the CPU rig can give the isend/irecv schedule before the
    driver's first 8-GPU run (per-pair FIFO matching must hold at any
    rank count)."""
    assert _run_cluster(4, 29544, 8, n_lanes=2, n_layer=4) == \
        _single_reference_tokens(8, n_layer=4)


def test_bench_driver_contract_world2():
    """The driver's N>1 launch shape (torch.distributed.run, one rank
    per GPU) must work end-to-end: rendezvous on 127.0.0.1, gloo on
    CPU, per-rank layer partition, MAX-over-ranks timing, ONE JSON line
    from rank 0 with the world-2 aggregate.

    This is the CPU/gloo shape by design (it asserts the gloo backend),
    so the ranks are started with the GPUs hidden: on a machine with a
    single GPU both ranks would otherwise land on it with a full-size
    KV set each and run out of memory."""
    import subprocess
    import sys
    port = str(29500 + os.getpid() % 500)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", port, "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=300, env=env,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["value"] > 0
    assert r["config"]["parallelism"] == "pp2"
    assert r["config"]["backend"] == "gloo"
    # weak scaling: per-rank work fixed, global batch grows with N
    assert r["config"]["global_batch"] == \
        r["config"]["mbs"] * r["config"]["micro_batches"]


def test_pipeline_generate_context_overflow_rejected():
    from distributedllm_amd.parallel.pipeline import pipeline_generate
    f = synthetic.build_model("tiny", seed=0)
    ex = slicer.make_extra_layers(f)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=16, max_batch=2)
    eng.attach_extra(ex)
    pipe = DecodePipeline(eng, PipelineConfig(mbs=2, n_mb=1, device="cpu"))
    with pytest.raises(ValueError, match="context"):
        pipeline_generate(pipe, list(range(3, 13)), max_steps=10)
