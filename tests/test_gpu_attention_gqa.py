"""Direct tests of the GQA decode attention kernel (k_attn_gqa and
k_attn_gqa_merge, ops/csrc/attention.hip) through the `attention_decode_gqa`
hook, against the float64 reference and the poisoned inputs of
attention_reference.py, and of its routing in the engine.

The bound is the project's derived bound for f16 Q and f16 P
(`tol_prefill`), which is this kernel's arithmetic; `uniform` (q = 0) uses
the case's own bound. n_ctx = 272 gives chunk 256 and two splits, n_ctx =
4096 chunk 512 and eight, so `sweep`/`peaky` (J = 255/256/257) and `deep`
(J = 2048, 1610, 4095, 4096) cross the split-KV merge.
"""
import os

import numpy as np
import pytest
import torch

import attention_reference as R
from distributedllm_amd.formats import ggml, synthetic

pytestmark = pytest.mark.gpu

SHAPES = [(16, 8, 2), (100, 8, 4), (128, 16, 2), (64, 16, 1), (32, 24, 1)]
KINDS = ["sweep", "uniform", "triangle_shuffled", "peaky", "last_row", "deep"]


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    return ops.core()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(core, case, rows=None):
    """One launch on fresh copies of the case (or of its tokens `rows`)
    -> (out, prep u16, jtw) as numpy; the caches must come back unchanged."""
    rows = slice(None) if rows is None else rows
    k, v = _dev(case.Kf), _dev(case.Vf)
    out, prep, jtw = core.attention_decode_gqa(
        _dev(case.q[rows]), k, v, _dev(case.pos[rows]), _dev(case.seq[rows]),
        case.H, case.Hkv, case.n_ctx, case.n_slots)
    torch.cuda.synchronize()
    assert np.array_equal(k.cpu().numpy().view(np.uint16),
                          case.Kf.view(np.uint16))
    assert np.array_equal(v.cpu().numpy().view(np.uint16),
                          case.Vf.view(np.uint16))
    return out.cpu().numpy(), prep.cpu().numpy().view(np.uint16), int(jtw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_decode_gqa(core, D, H, Hkv, kind):
    case = R.decode_case(kind, D, H, Hkv)
    out, prep, jtw = _run(core, case)
    out2, prep2, _ = _run(core, case)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), \
        case.name + ": two launches differ"
    assert np.array_equal(prep, prep2)
    tol = (case.tol if case.tolkind == "uniform" else
           R.tol_prefill(case.sabs, case.vmax))
    R.check_attention(case, out, prep, jtw, tol=tol)


@pytest.mark.parametrize("D,H,Hkv", [(128, 16, 2), (32, 24, 1)])
def test_batch_invariance(core, D, H, Hkv):
    """A token alone (T = 1) has the bits of its row in the full launch."""
    case = R.decode_case("sweep", D, H, Hkv)
    full, _, _ = _run(core, case)
    for J in (16, 257, 129):
        i = R.SWEEP_J.index(J)
        alone, _, _ = _run(core, case, slice(i, i + 1))
        assert np.array_equal(alone[0].view(np.uint32),
                              full[i].view(np.uint32)), "J = %d" % J


def test_selectors(core):
    for n_ctx, chunk, S in [(272, 256, 2), (2048, 256, 8), (4096, 512, 8),
                            (8192, 1024, 8)]:
        assert core.attn_gqa_chunk(n_ctx) == chunk
        for T in (1, 7, 64):
            assert core.attn_gqa_splits(n_ctx, T) == S
        assert core.attn_gqa_splits(n_ctx, 65) == 1
    route = core.attn_route
    assert route(32, 32, 8, True, True) == 0          # MHA
    assert route(64, 8, 8, True, True) == 2           # grp 8
    assert route(64, 8, 8, False, True) == 2
    assert route(64, 8, 8, True, False) == 0          # switched off
    assert route(128, 1, 8, True, True) == 0          # grp 128 > 64
    assert route(64, 8, 65, True, True) == 2          # wide decode
    assert route(64, 8, 65, False, True) == 1         # prefill
    assert route(32, 32, 65, False, True) == 1
    assert route(32, 32, 65, True, True) == 0


def _engine_run(preset, n_ctx=256, T=24, **kw):
    """Prefill of T tokens in pieces of at most 64, then 3 batched decode
    steps -> (list of the HIP outputs, list of the TorchSliceEngine
    outputs)."""
    from distributedllm_amd.engine import HIPSliceEngine, TorchSliceEngine
    f = synthetic.build_model(preset, ftype=ggml.FTYPE_MOSTLY_Q4_0, seed=0)
    hip = HIPSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=4, **kw)
    cpu = TorchSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=4)
    g = torch.Generator().manual_seed(21)
    E = f.hparams.n_embd
    steps = [(torch.randn(min(64, T - a), E, generator=g) * 0.5,
              torch.arange(a, min(a + 64, T), dtype=torch.int32),
              torch.zeros(min(64, T - a), dtype=torch.int32), False)
             for a in range(0, T, 64)]
    for i in range(3):
        steps.append((torch.randn(4, E, generator=g) * 0.5,
                      torch.tensor([T + i, i, i, i], dtype=torch.int32),
                      torch.arange(4, dtype=torch.int32), True))
    got, want = [], []
    for x, pos, seq, decode in steps:
        got.append(hip.forward(x.cuda(), pos.cuda(), seq.cuda(),
                               decode=decode).cpu())
        want.append(cpu.forward(x.clone(), pos, seq))
    return got, want


def _rel_rms(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_engine_gqa_route_matches_cpu():
    got, want = _engine_run("small_gqa", gqa_attention=True)
    for a, b in zip(got, want):
        assert _rel_rms(a, b) <= 8e-3


def test_engine_split_kv():
    """n_ctx = 320: chunk 256, two splits. The engine's own workspace and
    the merge launch serve the last prefill piece (rows 256..279 of a
    280-token prompt) and the decode steps of that sequence behind it."""
    got, want = _engine_run("small_gqa", n_ctx=320, T=280,
                            gqa_attention=True)
    for a, b in zip(got, want):
        assert _rel_rms(a, b) <= 8e-3


def test_engine_flag_off_is_the_streaming_path():
    """gqa_attention=False: k_attention, fused prologue included. The golden
    file holds the outputs y0..y3 of this very run (`_engine_run("small_gqa")`
    without the argument) on the commit before k_attn_gqa existed. The
    comparison is bit for bit, so a compiler or torch change that moves
    k_attention's bits needs the file recorded again: run that call on a
    checkout of that commit and save the four arrays with np.savez."""
    got, want = _engine_run("small_gqa", gqa_attention=False)
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden",
                                "gqa_off_small_gqa.npz"))
    for i, (a, b) in enumerate(zip(got, want)):
        assert _rel_rms(a, b) <= 8e-3
        assert np.array_equal(a.numpy().view(np.uint32),
                              gold["y%d" % i].view(np.uint32))
    on, _ = _engine_run("small_gqa", gqa_attention=True)
    assert any(not torch.equal(a, b) for a, b in zip(on, got))


def test_engine_mha_ignores_the_flag():
    on, _ = _engine_run("small", gqa_attention=True)
    off, _ = _engine_run("small", gqa_attention=False)
    for a, b in zip(on, off):
        assert torch.equal(a, b)
