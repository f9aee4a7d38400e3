"""CPU side of the int8 KV cache (kv_dtype="q8"): the numpy quantiser the
GPU tests use as their reference, the CPU twin's fake-quantisation, and the
public switches. The kernels are tested in test_gpu_kv8.py.

Q8_TWIN_DRIFT is the largest rel-RMS distance between the twin with a q8
cache and the twin with an f16 cache over the steps of ENGINE_RUNS, measured
on the CPU (2.74e-3, rounded up). It is what quantising the cache costs; the
device is compared with the q8 twin, not the f16 one (test_gpu_kv8.py).
"""
import numpy as np
import pytest
import torch

from distributedllm_amd.cli import build_parser
from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.engine.slice_engine import quantize_kv_rows
from distributedllm_amd.formats import ggml, slicer, synthetic
from distributedllm_amd.serving import ContinuousBatcher

Q8_TWIN_DRIFT = 3e-3
# (preset, n_ctx, prompt tokens, prompt in one forward call)
ENGINE_RUNS = [("small", 256, 24, False), ("small_gqa", 256, 24, False),
               ("small_gqa", 320, 280, False), ("small_gqa", 256, 100, True)]


def quantize_q8(x, D):
    """x [..., n*D] -> (q in [-127, 127], same shape, int32; s f16 [..., n]):
    per D-wide head s = f16(amax / 127), q = clamp(rint(x / s)), in f32;
    q = 0 where s == 0. The cache stores the byte q + 128."""
    x = np.asarray(x, dtype=np.float32)
    h = x.reshape(x.shape[:-1] + (-1, D))
    s = (np.abs(h).max(axis=-1) / np.float32(127)).astype(np.float16)
    sf = s.astype(np.float32)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(sf > 0, np.rint(h / sf), 0.0)
    return np.clip(q, -127, 127).astype(np.int32).reshape(x.shape), s


def engine_steps(preset, T, single):
    """The step pattern of test_gpu_attention_gqa._engine_run: a T-token
    prompt in pieces of at most 64 (or in one piece), then three batched
    decode steps -> (model file, [(x, pos, seq, decode)])."""
    f = synthetic.build_model(preset, ftype=ggml.FTYPE_MOSTLY_Q4_0, seed=0)
    g = torch.Generator().manual_seed(21)
    E = f.hparams.n_embd
    piece = T if single else 64
    steps = [(torch.randn(min(piece, T - a), E, generator=g) * 0.5,
              torch.arange(a, min(a + piece, T), dtype=torch.int32),
              torch.zeros(min(piece, T - a), dtype=torch.int32), False)
             for a in range(0, T, piece)]
    for i in range(3):
        steps.append((torch.randn(4, E, generator=g) * 0.5,
                      torch.tensor([T + i, i, i, i], dtype=torch.int32),
                      torch.arange(4, dtype=torch.int32), True))
    return f, steps


def rel_rms(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_quantisers_agree():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((40, 4 * 24)).astype(np.float32)
    x[3] = 0.0
    x[4, :24] *= 1e-7
    x[5, 30] = 1000.0
    q, s = quantize_q8(x, 24)
    want = (s.astype(np.float32)[..., None] * q.reshape(40, 4, 24))
    got = quantize_kv_rows(torch.from_numpy(x).view(40, 4, 24)).numpy()
    assert np.array_equal(got, want)
    assert np.abs(q).max() == 127 and not q[3].any()


@pytest.mark.parametrize("preset,n_ctx,T,single", ENGINE_RUNS)
def test_twin_q8_against_f16(preset, n_ctx, T, single):
    f, steps = engine_steps(preset, T, single)
    q8 = TorchSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=4,
                                    kv_dtype="q8")
    f16 = TorchSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=4)
    worst, differ = 0.0, False
    for x, pos, seq, _ in steps:
        a, b = q8.forward(x.clone(), pos, seq), f16.forward(x.clone(), pos, seq)
        worst = max(worst, rel_rms(a, b))
        differ = differ or not torch.equal(a, b)
    print("%s n_ctx %d T %d: q8 vs f16 twin rel-RMS %.3g" %
          (preset, n_ctx, T, worst))
    assert differ and worst <= Q8_TWIN_DRIFT


def test_public_switches():
    f = synthetic.build_model("tiny", seed=0)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=3, kv_dtype="q8")
    eng.attach_extra(slicer.make_extra_layers(f))
    bat = ContinuousBatcher(eng)                # unchanged on a q8 engine
    r = bat.submit([5, 9, 3], 4)
    bat.run_all(max_steps=16)
    assert len(r.out) == 4
    with pytest.raises(ValueError, match="shared_prefix.*kv_dtype"):
        ContinuousBatcher(eng, shared_prefix=[5, 9, 3])
    with pytest.raises(ValueError):
        TorchSliceEngine.from_ggml(f, kv_dtype="q4")
    for argv in (["serve_http", "m.bin"], ["batch_generate", "m.bin"],
                 ["run_node"]):
        assert build_parser().parse_args(argv).kv_dtype == "f16"
        assert build_parser().parse_args(
            argv + ["--kv-dtype", "q8"]).kv_dtype == "q8"
