"""The paged KV cache on the device (ops/csrc/attention_paged.hip):
`k_attn_paged` and `k_paged_rows` through their hooks against the float64
reference of attention_reference.py, `kv_layout="paged"` in the engine, and
page reservation in the batcher.

The kernel's arithmetic is k_attn_gqa's (f16 Q, f16 P on the matrix cores),
so the bound is the one test_gpu_attention_gqa.py applies: `tol_prefill`, and
the case's own bound for `uniform`. The case's K and V, poisoned above every
filled row, are scattered into pools through a seeded page permutation; the
rest of the pools, page 0 included, holds the poison values too.
"""
import functools

import numpy as np
import pytest
import torch

import attention_reference as R
from test_kv8_reference import ENGINE_RUNS, engine_steps, rel_rms

pytestmark = pytest.mark.gpu

SHAPES = [(16, 8, 2), (100, 8, 4), (128, 16, 2), (64, 4, 4), (100, 4, 4),
          (32, 24, 1)]
KINDS = ["sweep", "uniform", "triangle_shuffled", "peaky", "last_row", "deep"]
ENGINE_BOUND = 8e-3     # the f16 engines' bound against the same twin
PG = 16


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    assert ops.core().kv_page_rows() == PG
    return ops.core()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rowmap(table, n_ctx):
    """[slots, n_ctx]: the pool row of every logical row."""
    r = np.arange(n_ctx)
    return table[:, r // PG] * PG + r % PG


@functools.lru_cache(maxsize=4)
def _pools(kind, D, H, Hkv, identity=False):
    """-> (case, table i32 [slots, pages per slot], K pool, V pool): flat f16
    [pages * 16 * Ekv + 16], poison wherever no row of the case landed."""
    c = R.decode_case(kind, D, H, Hkv)
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


def _run(core, c, table, kp, vp, rows=slice(None), pos=None, seq=None):
    """One launch on fresh copies -> out, prep u16, jtw; the pools must come
    back unchanged and k_paged_rows must agree with the table."""
    pos = c.pos[rows] if pos is None else pos
    seq = c.seq[rows] if seq is None else seq
    k, v, tb = _dev(kp), _dev(vp), _dev(table)
    out, prep, jtw = core.attention_paged(_dev(c.q[rows]), k, v, tb,
                                          _dev(pos), _dev(seq), c.H, c.Hkv,
                                          c.n_ctx)
    got_rows = core.paged_rows(tb, _dev(pos), _dev(seq), c.n_ctx)
    torch.cuda.synchronize()
    assert np.array_equal(got_rows.cpu().numpy(),
                          _rowmap(table, c.n_ctx)[seq, pos])
    for d, a in ((k, kp), (v, vp)):
        assert np.array_equal(d.cpu().numpy().view(np.uint16),
                              a.view(np.uint16))
    return out.cpu().numpy(), prep.cpu().numpy().view(np.uint16), int(jtw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_attention_paged(core, D, H, Hkv, kind):
    c, table, kp, vp = _pools(kind, D, H, Hkv)
    out, prep, jtw = _run(core, c, table, kp, vp)
    out2, prep2, _ = _run(core, c, table, kp, vp)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), \
        c.name + ": two launches differ"
    assert np.array_equal(prep, prep2)
    tol = (c.tol if c.tolkind == "uniform" else
           R.tol_prefill(c.sabs, c.vmax))
    R.check_attention(c, out, prep, jtw, tol=tol)
    ident, _, _ = _run(core, *_pools(kind, D, H, Hkv, True))
    assert np.array_equal(out.view(np.uint32), ident.view(np.uint32)), \
        c.name + ": the bits depend on the page placement"


@pytest.mark.parametrize("D,H,Hkv", [(128, 16, 2), (64, 4, 4), (32, 24, 1)])
def test_batch_invariance(core, D, H, Hkv):
    """A token alone (T = 1) has the bits of its row in the full launch."""
    c, table, kp, vp = _pools("sweep", D, H, Hkv)
    full, _, _ = _run(core, c, table, kp, vp)
    for J in (16, 17, 257):
        i = R.SWEEP_J.index(J)
        alone, _, _ = _run(core, c, table, kp, vp, slice(i, i + 1))
        assert np.array_equal(alone[0].view(np.uint32),
                              full[i].view(np.uint32)), "J = %d" % J


def test_aliasing(core):
    """Slot b shares slot a's first 8 pages (rows 0..127) and owns row 128:
    the bits of b holding its own copy of those rows."""
    c, table, kp, vp = _pools("sweep", 64, 4, 4)
    i = R.SWEEP_J.index(257)
    a, b = int(c.seq[i]), int(c.seq[R.SWEEP_J.index(1)])
    pos, seq = np.array([256, 128], np.int32), np.array([a, b], np.int32)
    rows = np.array([i, i])
    rm = _rowmap(table, c.n_ctx)
    copy = [p.copy() for p in (kp, vp)]
    for p in copy:
        v = p[:-16].reshape(-1, c.Hkv * c.D)
        v[rm[b, :129]] = v[rm[a, :129]]
    shared = table.copy()
    shared[b, :8] = table[a, :8]
    want, _, _ = _run(core, c, table, copy[0], copy[1], rows, pos, seq)
    got, _, _ = _run(core, c, shared, copy[0], copy[1], rows, pos, seq)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got[0], got[1])


def test_selectors(core):
    for n_ctx, chunk, S in [(272, 256, 2), (2048, 256, 8), (4096, 512, 8)]:
        assert core.attn_paged_chunk(n_ctx) == chunk
        for T in (1, 64):
            assert core.attn_paged_splits(n_ctx, T) == S
        assert core.attn_paged_splits(n_ctx, 65) == 1


def _reserve_scrambled(eng, n_ctx):
    for n in range(PG, n_ctx + PG, PG):
        for s in (2, 0, 3, 1):
            assert eng.kv_reserve(s, min(n, n_ctx))


@pytest.mark.parametrize("preset,n_ctx,T,single", ENGINE_RUNS)
def test_engine_paged_matches_twin(preset, n_ctx, T, single):
    """n_ctx = 320, T = 280 crosses the split; T = 100 in one call runs the
    per-token kernel at T > 64. On the GQA preset the layer-0 rows are those
    of the contiguous engine: the same qkv kernels on the same input."""
    from distributedllm_amd.engine import HIPSliceEngine, TorchSliceEngine
    f, steps = engine_steps(preset, T, single)
    hip = HIPSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=4,
                                   kv_layout="paged")
    flat = HIPSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=4)
    cpu = TorchSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=4)
    start = hip.kv_free_pages
    assert start == 4 * -(-n_ctx // PG) == hip.kv_pages - 1
    _reserve_scrambled(hip, n_ctx)
    assert hip.kv_free_pages == 0
    for x, pos, seq, decode in steps:
        got = hip.forward(x.cuda(), pos.cuda(), seq.cuda(),
                          decode=decode).cpu()
        flat.forward(x.cuda(), pos.cuda(), seq.cuda(), decode=decode)
        err = rel_rms(got, cpu.forward(x.clone(), pos, seq))
        print("%s T %d: rel-RMS %.3g" % (preset, x.shape[0], err))
        assert err <= ENGINE_BOUND
    table = hip._eng.block_table.cpu().numpy()
    assert (np.diff(np.sort(table.reshape(-1))) == 1).all() and table.min() == 1
    if f.hparams.is_gqa:
        rm = torch.from_numpy(_rowmap(table, n_ctx))
        for pool, cache in ((hip._eng.k_cache, flat._eng.k_cache),
                            (hip._eng.v_cache, flat._eng.v_cache)):
            for s, n in ((0, T + 3), (1, 3), (2, 3), (3, 3)):
                assert torch.equal(pool[0].cpu()[rm[s, :n]],
                                   cache[0, s, :n].cpu())
    x, pos, seq, _ = steps[-1]
    with pytest.raises(RuntimeError, match="prefix"):
        hip.forward(x.cuda(), pos.cuda(), seq.cuda(),
                    prefix=(0, 1, torch.zeros(4, dtype=torch.int32).cuda()))
    for s in range(4):
        hip.kv_release(s)
    assert hip.kv_free_pages == start
    assert not hip._eng.block_table.any()


def test_refusals_and_default():
    from distributedllm_amd.engine import HIPSliceEngine
    from distributedllm_amd.formats import ggml, synthetic
    f, steps = engine_steps("small_gqa", 24, False)
    with pytest.raises((ValueError, RuntimeError), match="kv_dtype"):
        HIPSliceEngine.from_ggml(f, kv_layout="paged", kv_dtype="q8")
    with pytest.raises((ValueError, RuntimeError), match="kv_pages"):
        HIPSliceEngine.from_ggml(f, kv_layout="paged", kv_pages=1)
    with pytest.raises(ValueError, match="kv_layout"):
        HIPSliceEngine.from_ggml(f, kv_layout="blocked")
    f32 = synthetic.build_model("tiny", ftype=ggml.FTYPE_ALL_F32, seed=0)
    with pytest.raises(RuntimeError, match="kv_layout paged"):
        HIPSliceEngine.from_ggml(f32, n_ctx=32, max_batch=2,
                                 kv_layout="paged")
    a = HIPSliceEngine.from_ggml(f, n_ctx=256, max_batch=4)
    b = HIPSliceEngine.from_ggml(f, n_ctx=256, max_batch=4,
                                 kv_layout="contiguous")
    assert a.kv_layout == "contiguous" and a.kv_free_pages == 0
    assert a._eng.k_cache.shape == (f.hparams.n_layer, 4, 256,
                                    f.hparams.n_embd_kv)
    for x, pos, seq, decode in steps:
        assert torch.equal(
            a.forward(x.cuda(), pos.cuda(), seq.cuda(), decode=decode),
            b.forward(x.cuda(), pos.cuda(), seq.cuda(), decode=decode))


@pytest.mark.parametrize("spec_k", [0, 4])
def test_batcher_waits_for_pages(spec_k):
    """Six greedy requests of 1..3 pages on a pool of 3: the tokens of the
    run with ample pages, every page back afterwards."""
    from distributedllm_amd.engine import HIPSliceEngine
    from distributedllm_amd.formats import slicer, synthetic
    from distributedllm_amd.serving import ContinuousBatcher
    f = synthetic.build_model("tiny", seed=0)
    ex = slicer.make_extra_layers(f)
    prompts = [[5, 9, 3], list(range(2, 30)), [7], [2, 11, 4, 6, 1] * 4,
               [3, 3, 3, 3, 3, 3, 3, 3, 3], list(range(40, 10, -1))]
    new = [6, 8, 20, 5, 12, 9]

    def run(kv_pages):
        eng = HIPSliceEngine.from_ggml(f, n_ctx=64, max_batch=4,
                                       kv_layout="paged", kv_pages=kv_pages)
        eng.attach_extra(ex)
        bat = ContinuousBatcher(eng, spec_ngram=2 if spec_k else 0,
                                spec_k=spec_k)
        start = eng.kv_free_pages
        if kv_pages:                                # 64 rows: 4 pages
            with pytest.raises(ValueError, match="KV pages"):
                bat.submit(list(range(1, 41)), 24)
        reqs = [bat.submit(p, n) for p, n in zip(prompts, new)]
        gone = bat.submit([1, 2, 3], 40)
        bat.step()
        assert bat.cancel(gone)
        bat.run_all(max_steps=400)
        torch.cuda.synchronize()
        assert all(r.done and len(r.out) == n for r, n in zip(reqs, new))
        assert eng.kv_free_pages == start
        return [r.out for r in reqs]

    assert run(4) == run(None)
