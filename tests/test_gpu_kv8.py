"""The int8 KV cache on the device (ops/csrc/attention_kv8.hip): the
quantising append `k_kv8_append`, the attention kernel `k_attn_kv8` through
their hooks, and `kv_dtype="q8"` in the engine.

Attention is compared with the float64 reference of attention_reference.py
over the DEQUANTISED cache (s * q in float64), so the quantisation itself is
not under test; the bound is `tol_prefill`, the project's bound for f16 Q and
f16 P, with sabs / vmax taken from the dequantised cache. Folding the V scale
into the probability adds no term: the kernel packs P~ = p * s_v / R with R
the largest s_v among the attended rows, so P~ <= 1 carries the relative f16
rounding 2^-11 that p itself carries in the other matrix-core kernels, and a
P~ below the f16 normal range errs by at most 2^-25 R per row, that is
127 * 2^-25 R <= 2^-25 vmax in the output, the same as a subnormal f16 p.

Engine runs are compared with the CPU twin, which quantises f32 rows where the
device quantises the f16 rows of its qkv kernels, so a value near a half
integer can land on different bytes. The device measured at most 1.9e-3
rel-RMS from the q8 twin on these runs, inside the 8e-3 that the f16 engine
tests allow against the same twin, so ENGINE_BOUND is that bound unchanged
(the twin's own q8-versus-f16 distance, 2.7e-3, is not added to it).
"""
import functools

import numpy as np
import pytest
import torch

import attention_reference as R
from test_kv8_reference import (ENGINE_RUNS, engine_steps, quantize_q8,
                                rel_rms)

pytestmark = pytest.mark.gpu

SHAPES = [(16, 8, 2), (100, 8, 4), (128, 16, 2), (64, 4, 4), (100, 4, 4),
          (32, 24, 1)]
KINDS = ["sweep", "uniform", "triangle_shuffled", "peaky", "last_row", "deep"]
# the f16 engines' bound against the same twin (test_gpu_engine.py)
ENGINE_BOUND = 8e-3


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    return ops.core()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(kind, D, H, Hkv):
    """decode_case with its K/V quantised: byte stores (pad 0xFF), scale
    planes, and reference / sabs / vmax over the dequantised cache."""
    c = R.decode_case(kind, D, H, Hkv)
    st, deq = [], []
    for a in (c.K, c.V):
        q, s = quantize_q8(a, D)
        st.append(np.concatenate([(q + 128).astype(np.uint8).reshape(-1),
                                  np.full(16, 255, np.uint8)]))
        st.append(s.reshape(-1))
        deq.append((s.astype(np.float64)[..., None] *
                    q.reshape(s.shape + (D,))).reshape(a.shape))
    ref, sabs, vmax = R._attend(c.q, deq[0], deq[1], c.pos, c.seq, H, Hkv)
    return c, st, ref, R.tol_prefill(sabs, vmax)


def _run(core, c, st, rows=slice(None)):
    """One launch on fresh copies -> (out, prep u16, jtw) as numpy; caches
    and scales must come back unchanged."""
    dev = [_dev(a) for a in st]
    out, prep, jtw = core.attention_kv8(
        _dev(c.q[rows]), dev[0], dev[2], dev[1], dev[3], _dev(c.pos[rows]),
        _dev(c.seq[rows]), c.H, c.Hkv, c.n_ctx, c.n_slots)
    torch.cuda.synchronize()
    for d, a in zip(dev, st):
        assert np.array_equal(d.cpu().numpy().view(np.uint8),
                              a.view(np.uint8))
    return out.cpu().numpy(), prep.cpu().numpy().view(np.uint16), int(jtw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_attention_kv8(core, D, H, Hkv, kind):
    c, st, ref, tol = _case(kind, D, H, Hkv)
    out, prep, jtw = _run(core, c, st)
    out2, prep2, _ = _run(core, c, st)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), \
        c.name + ": two launches differ"
    assert np.array_equal(prep, prep2)
    R.check_attention(c, out, prep, jtw, ref=ref, tol=tol)


@pytest.mark.parametrize("D,H,Hkv", [(128, 16, 2), (64, 4, 4), (32, 24, 1)])
def test_batch_invariance(core, D, H, Hkv):
    """A token alone (T = 1) has the bits of its row in the full launch."""
    c, st, _, _ = _case("sweep", D, H, Hkv)
    full, _, _ = _run(core, c, st)
    for J in (16, 129, 257):
        i = R.SWEEP_J.index(J)
        alone, _, _ = _run(core, c, st, slice(i, i + 1))
        assert np.array_equal(alone[0].view(np.uint32),
                              full[i].view(np.uint32)), "J = %d" % J


def test_selectors(core):
    for n_ctx, chunk, S in [(272, 256, 2), (2048, 256, 8), (4096, 512, 8)]:
        assert core.attn_kv8_chunk(n_ctx) == chunk
        assert core.attn_kv8_splits(n_ctx, 64) == S
        assert core.attn_kv8_splits(n_ctx, 65) == 1


@pytest.mark.parametrize("D,Hkv", [(16, 2), (100, 4), (128, 2)])
def test_append(core, D, Hkv):
    """With s the device's scale: s within one f16 ulp of amax / 127,
    |q| <= 127, and |s q - x| <= s (0.5 + 2^-10) + max(amax 2^-11,
    127 * 2^-25): half a step of rint plus the rounding of x / s, and the
    clamp when s was rounded down, 127 times the rounding error of s. That
    error is amax / 127 * 2^-11 for a normal s and at most 2^-25 for a
    subnormal one (the row of subnormals; s = 0 and q = 0 included).
    Everything outside the written rows keeps its poison."""
    rng = np.random.default_rng(R._seed("kv8_append", D, Hkv))
    n_ctx, n_slots, Ekv = 12, 3, Hkv * D
    pos = np.array([0, n_ctx - 1, 3, 7], dtype=np.int32)
    seq = np.array([1, n_slots - 1, n_slots - 1, 0], dtype=np.int32)
    stage = []
    for _ in range(2):
        flat, a = R.stores(n_slots, n_ctx, Ekv)
        a[:] = rng.standard_normal(a.shape)
        a[seq[0], pos[0], :D] = 0.0                       # all-zero head
        a[seq[1], pos[1], -D:] *= 1e-3
        a[seq[1], pos[1], -3] = 1.0                       # 1000 x the rest
        a[seq[2], pos[2]] = (rng.integers(1, 1024, Ekv) * 2.0 ** -24 *
                             rng.choice([-1.0, 1.0], Ekv))
        stage.append((flat, a))
    st8 = [torch.full((n_slots * n_ctx * Ekv + 16,), 0xAB, dtype=torch.uint8,
                      device="cuda") for _ in range(2)]
    sc = [torch.full((n_slots * n_ctx * Hkv,), 77.0, dtype=torch.float16,
                     device="cuda") for _ in range(2)]
    core.kv8_append(_dev(stage[0][0]), _dev(stage[1][0]), st8[0], st8[1],
                    sc[0], sc[1], _dev(pos), _dev(seq), Hkv, n_ctx, n_slots)
    torch.cuda.synchronize()
    for (_, a), b8, s16 in zip(stage, st8, sc):
        b8 = b8.cpu().numpy()
        assert (b8[-16:] == 0xAB).all()
        b8 = b8[:-16].reshape(n_slots, n_ctx, Hkv, D)
        s = s16.cpu().numpy().astype(np.float64).reshape(n_slots, n_ctx, Hkv)
        hit = np.zeros((n_slots, n_ctx), dtype=bool)
        hit[seq, pos] = True
        assert (b8[~hit] == 0xAB).all() and (s[~hit] == 77.0).all()
        x = a.astype(np.float64).reshape(n_slots, n_ctx, Hkv, D)[hit]
        q, s = b8[hit].astype(np.float64) - 128, s[hit][..., None]
        amax = np.abs(x).max(axis=-1, keepdims=True)
        ulp = np.spacing(np.abs(amax / 127).astype(np.float16)).astype(
            np.float64)
        assert (np.abs(s - amax / 127) <= ulp).all()
        assert np.abs(q).max() <= 127
        bound = s * (0.5 + 2.0 ** -10) + np.maximum(amax * 2.0 ** -11,
                                                    127 * 2.0 ** -25)
        err = np.abs(s * q - x)
        print("D %d: worst error / bound = %.3g" % (D, (err / bound).max()))
        assert (err <= bound).all()


@pytest.mark.parametrize("preset,n_ctx,T,single", ENGINE_RUNS)
def test_engine_q8_matches_twin(preset, n_ctx, T, single):
    """n_ctx = 320, T = 280 crosses the split; T = 100 in one call runs the
    per-token kernel at T > 64."""
    from distributedllm_amd.engine import HIPSliceEngine, TorchSliceEngine
    f, steps = engine_steps(preset, T, single)
    hip = HIPSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=4, kv_dtype="q8")
    cpu = TorchSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=4,
                                     kv_dtype="q8")
    assert hip._eng.k_cache.dtype == torch.uint8
    assert hip._eng.k_scale.shape == (f.hparams.n_layer, 4, n_ctx,
                                      f.hparams.kv_heads)
    for x, pos, seq, decode in steps:
        got = hip.forward(x.cuda(), pos.cuda(), seq.cuda(),
                          decode=decode).cpu()
        err = rel_rms(got, cpu.forward(x.clone(), pos, seq))
        print("%s T %d: rel-RMS %.3g" % (preset, x.shape[0], err))
        assert err <= ENGINE_BOUND
    x, pos, seq, _ = steps[-1]
    with pytest.raises(RuntimeError, match="prefix"):
        hip.forward(x.cuda(), pos.cuda(), seq.cuda(),
                    prefix=(0, 1, torch.zeros(4, dtype=torch.int32).cuda()))


def test_default_is_f16_bit_for_bit():
    from distributedllm_amd.engine import HIPSliceEngine
    f, steps = engine_steps("small_gqa", 24, False)
    a = HIPSliceEngine.from_ggml(f, n_ctx=256, max_batch=4)
    b = HIPSliceEngine.from_ggml(f, n_ctx=256, max_batch=4, kv_dtype="f16")
    assert a._eng.k_cache.dtype == torch.float16
    for x, pos, seq, decode in steps:
        assert torch.equal(
            a.forward(x.cuda(), pos.cuda(), seq.cuda(), decode=decode),
            b.forward(x.cuda(), pos.cuda(), seq.cuda(), decode=decode))
