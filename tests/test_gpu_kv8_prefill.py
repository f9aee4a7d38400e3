"""Q-tiled q8 prefill attention (`k_attn_kv8_prefill`, ops/csrc/
attention_kv8.hip) through its hook, and `kv8_prefill=` in the engine.

As in test_gpu_kv8.py the float64 reference runs over the DEQUANTISED cache
and the bound is `tol_prefill` with sabs / vmax of that cache, for every kind
(the q = 0 kinds included: P~ is f16). The V-scale maximum R is kept per
query, so P~ = p * s_v / R <= 1 holds per token and the bound needs no term
beyond those of test_gpu_kv8.py.
"""
import functools

import numpy as np
import pytest
import torch

import attention_reference as R
from test_kv8_prefill_reference import EDGE_J, edge_case, quantized
from test_kv8_reference import engine_steps, rel_rms

pytestmark = pytest.mark.gpu

SHAPES = [(16, 8, 2), (100, 8, 4), (128, 16, 2), (64, 4, 4), (32, 24, 1)]
KINDS = [k for k in R.PREFILL_KINDS if k != "edges"]
ENGINE_BOUND = 8e-3     # test_gpu_kv8.py: the f16 engines' bound, unchanged


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    return ops.core()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(kind, D, H, Hkv):
    c = edge_case(D, H, Hkv) if kind == "edges8" else R.prefill_case(
        kind, D, H, Hkv)
    return (c,) + quantized(c)


def _run(core, c, st, rows=slice(None)):
    """One launch on fresh copies -> (out, prep u16, jtw) as numpy; caches
    and scales must come back unchanged."""
    dev = [_dev(a) for a in st]
    out, prep, jtw = core.attention_kv8_prefill(
        _dev(c.q[rows]), dev[0], dev[2], dev[1], dev[3], _dev(c.pos[rows]),
        _dev(c.seq[rows]), c.H, c.Hkv, c.n_ctx, c.n_slots)
    torch.cuda.synchronize()
    for d, a in zip(dev, st):
        assert np.array_equal(d.cpu().numpy().view(np.uint8),
                              a.view(np.uint8))
    return out.cpu().numpy(), prep.cpu().numpy().view(np.uint16), int(jtw)


def _check(core, kind, D, H, Hkv):
    c, st, ref, tol = _case(kind, D, H, Hkv)
    out, prep, jtw = _run(core, c, st)
    out2, prep2, _ = _run(core, c, st)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), \
        c.name + ": two launches differ"
    assert np.array_equal(prep, prep2)
    R.check_attention(c, out, prep, jtw, ref=ref, tol=tol)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_attention_kv8_prefill(core, D, H, Hkv, kind):
    _check(core, kind, D, H, Hkv)


@pytest.mark.parametrize("D,H,Hkv", [(100, 8, 4), (128, 16, 2)])
def test_own_tile_edges(core, D, H, Hkv):
    """Six 16-query tiles whose jmax + 1 is EDGE_J: the 32-row tile, the
    128-row pass of four waves and the 256-row double-buffer iteration."""
    assert EDGE_J == (33, 127, 128, 129, 256, 257)
    _check(core, "edges8", D, H, Hkv)


@pytest.mark.parametrize("D,H,Hkv", [(128, 16, 2), (32, 24, 1)])
def test_tile_mate_invariance(core, D, H, Hkv):
    """A token alone (T = 1) has the bits of its row in the full launch."""
    c, st, _, _ = _case("span37_T40", D, H, Hkv)
    full, _, _ = _run(core, c, st)
    for t in (0, 15, 39):
        alone, _, _ = _run(core, c, st, slice(t, t + 1))
        assert np.array_equal(alone[0].view(np.uint32),
                              full[t].view(np.uint32)), "token %d" % t


def test_route(core):
    assert core.attn_kv8_route(64, 0, 1) == 0
    assert core.attn_kv8_route(65, 0, 1) == 1
    assert core.attn_kv8_route(65, 1, 1) == 0
    assert core.attn_kv8_route(65, 0, 0) == 0


@pytest.mark.parametrize("preset", ["small", "small_gqa"])
def test_engine_kv8_prefill(preset):
    """A 100-token prompt in one call, then decode: the Q-tiled route and the
    per-token route each against the q8 CPU twin."""
    from distributedllm_amd.engine import HIPSliceEngine, TorchSliceEngine
    f, steps = engine_steps(preset, 100, True)
    cpu = TorchSliceEngine.from_ggml(f, n_ctx=256, max_batch=4, kv_dtype="q8")
    hip = [HIPSliceEngine.from_ggml(f, n_ctx=256, max_batch=4, kv_dtype="q8",
                                    kv8_prefill=on) for on in (True, False)]
    for x, pos, seq, decode in steps:
        want = cpu.forward(x.clone(), pos, seq)
        err = [rel_rms(e.forward(x.cuda(), pos.cuda(), seq.cuda(),
                                 decode=decode).cpu(), want) for e in hip]
        print("%s T %d: rel-RMS Q-tiled %.3g, per-token %.3g" %
              (preset, x.shape[0], err[0], err[1]))
        assert max(err) <= ENGINE_BOUND
