"""Q-tiled prefill attention over the page pools (`k_attn_paged_prefill`,
ops/csrc/attention_paged.hip) through its hook, and `paged_prefill=` in the
engine.

The arithmetic is k_attn_paged's (f16 Q, f16 P on the matrix cores), so the
bound is the one test_gpu_paged.py applies: `tol_prefill`, and the case's own
bound for the `uniform` kinds. Pools are built as test_gpu_paged.py::_pools
builds them: the case's K and V scattered through a seeded page permutation,
+-30000 in every unassigned row and in page 0.
"""
import functools

import numpy as np
import pytest
import torch

import attention_reference as R
from test_gpu_paged import ENGINE_BOUND, PG, _dev, _reserve_scrambled, _rowmap
from test_kv8_prefill_reference import EDGE_J, edge_case
from test_kv8_reference import engine_steps, rel_rms

pytestmark = pytest.mark.gpu

SHAPES = [(16, 8, 2), (100, 8, 4), (128, 16, 2), (64, 4, 4), (32, 24, 1)]


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    assert ops.core().kv_page_rows() == PG
    return ops.core()


@functools.lru_cache(maxsize=4)
def _pools(kind, D, H, Hkv, identity=False):
    """-> (case, table i32 [slots, pages per slot], K pool, V pool): flat f16
    [pages * 16 * Ekv + 16], poison wherever no row of the case landed."""
    c = edge_case(D, H, Hkv) if kind == "edges16" else R.prefill_case(
        kind, D, H, Hkv)
    npg = -(-c.n_ctx // PG)
    order = np.arange(c.n_slots * npg)
    if not identity:
        order = np.random.default_rng(R._seed("pages", kind, D)).permutation(
            order)
        assert (order != np.arange(order.size)).any()
    table = (1 + order).reshape(c.n_slots, npg).astype(np.int32)
    rows = _rowmap(table, c.n_ctx).reshape(-1)
    pools = []
    for a, val in ((c.K, 30000.0), (c.V, -30000.0)):
        Ekv = a.shape[-1]
        flat = np.full((1 + order.size) * PG * Ekv + 16, val, np.float16)
        flat[:-16].reshape(-1, Ekv)[rows] = a.reshape(-1, Ekv)
        pools.append(flat)
    return c, table, pools[0], pools[1]


def _run(core, c, table, kp, vp, rows=slice(None)):
    """One launch on fresh copies -> out, prep u16, jtw; the pools must come
    back unchanged."""
    k, v = _dev(kp), _dev(vp)
    out, prep, jtw = core.attention_paged_prefill(
        _dev(c.q[rows]), k, v, _dev(table), _dev(c.pos[rows]),
        _dev(c.seq[rows]), c.H, c.Hkv, c.n_ctx)
    torch.cuda.synchronize()
    for d, a in ((k, kp), (v, vp)):
        assert np.array_equal(d.cpu().numpy().view(np.uint16),
                              a.view(np.uint16))
    return out.cpu().numpy(), prep.cpu().numpy().view(np.uint16), int(jtw)


def _check(core, kind, D, H, Hkv):
    c, table, kp, vp = _pools(kind, D, H, Hkv)
    out, prep, jtw = _run(core, c, table, kp, vp)
    out2, prep2, _ = _run(core, c, table, kp, vp)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), \
        c.name + ": two launches differ"
    assert np.array_equal(prep, prep2)
    tol = (c.tol if c.tolkind == "uniform" else
           R.tol_prefill(c.sabs, c.vmax))
    R.check_attention(c, out, prep, jtw, tol=tol)
    return out


@pytest.mark.parametrize("kind", R.PREFILL_KINDS)
@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_attention_paged_prefill(core, D, H, Hkv, kind):
    _check(core, kind, D, H, Hkv)


@pytest.mark.parametrize("D,H,Hkv", [(100, 8, 4), (128, 16, 2)])
def test_deep_edges(core, D, H, Hkv):
    """16-query tiles whose jmax + 1 is 127, 128, 256 and 257 (among others)
    at n_ctx 272: the odd tile past the segment end and the second
    double-buffer iteration."""
    assert {127, 128, 256, 257} <= set(EDGE_J)
    _check(core, "edges16", D, H, Hkv)


@pytest.mark.parametrize("kind", ["mixed", "edges"])
@pytest.mark.parametrize("D,H,Hkv", [(100, 8, 4), (64, 4, 4)])
def test_placement_invariance(core, D, H, Hkv, kind):
    out = _check(core, kind, D, H, Hkv)
    ident, _, _ = _run(core, *_pools(kind, D, H, Hkv, True))
    assert np.array_equal(out.view(np.uint32), ident.view(np.uint32)), \
        "the bits depend on the page placement"


@pytest.mark.parametrize("D,H,Hkv", [(128, 16, 2), (32, 24, 1)])
def test_tile_mate_invariance(core, D, H, Hkv):
    """A token alone (T = 1) has the bits of its row in the full launch."""
    c, table, kp, vp = _pools("span37_T40", D, H, Hkv)
    full, _, _ = _run(core, c, table, kp, vp)
    for t in (0, 15, 39):
        alone, _, _ = _run(core, c, table, kp, vp, slice(t, t + 1))
        assert np.array_equal(alone[0].view(np.uint32),
                              full[t].view(np.uint32)), "token %d" % t


def test_route(core):
    assert core.attn_paged_route(64, 0, 1) == 0
    assert core.attn_paged_route(65, 0, 1) == 1
    assert core.attn_paged_route(65, 1, 1) == 0
    assert core.attn_paged_route(65, 0, 0) == 0


@pytest.mark.parametrize("preset", ["small", "small_gqa"])
def test_engine_paged_prefill(preset):
    """A 100-token prompt in one call, then decode: the Q-tiled route and the
    per-token route each against the CPU twin."""
    from distributedllm_amd.engine import HIPSliceEngine, TorchSliceEngine
    f, steps = engine_steps(preset, 100, True)
    cpu = TorchSliceEngine.from_ggml(f, n_ctx=256, max_batch=4)
    hip = [HIPSliceEngine.from_ggml(f, n_ctx=256, max_batch=4,
                                    kv_layout="paged", paged_prefill=on)
           for on in (True, False)]
    for e in hip:
        _reserve_scrambled(e, 256)
    for x, pos, seq, decode in steps:
        want = cpu.forward(x.clone(), pos, seq)
        err = [rel_rms(e.forward(x.cuda(), pos.cuda(), seq.cuda(),
                                 decode=decode).cpu(), want) for e in hip]
        print("%s T %d: rel-RMS Q-tiled %.3g, per-token %.3g" %
              (preset, x.shape[0], err[0], err[1]))
        assert max(err) <= ENGINE_BOUND
