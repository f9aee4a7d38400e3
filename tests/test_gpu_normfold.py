"""The RMSNorm weight folded into the activation panel (ops/csrc/
mfma_gemm.hip): the producer of an xprep stores f16(x) * f16(norm_w), the
NORM kernels apply only the per-token scale.

Shapes: cols = 96 is three K-blocks, so the q4 / byte-stream kernels run
into the zero-scaled fourth block of the 4-block load group; cols = 160 is
five (the non-power-of-two 3200-style width, two groups with three pad
blocks). T = 1, 16, 17, 64 are one token, a full tile, a tile plus one
token and the full decode panel (panel widths 1, 1, 2, 4). Formats: q4_0
(nibble stream) and q8_0 (byte stream).

  * the consumers - the qkv slab route, k_ffn16, the lm_head - against the
    float64 reference of gemm_reference.py at the bounds test_gpu_gemm.py
    holds them to (tol_norm and what is derived from it);
  * the producers, to the bit: k_prep_x, k_reduce_prep (split), the fused
    residual epilogue and the large-M epilogue (T = 70) store
    f16(f16(x) * f16(norm_w)) at xprep_index, and f16(x) - the bytes from
    before the fold - when they get no norm plane; everything else in the
    channel stays zero, and the sumsq channel is of the un-normalised x.

The norm weights are uniform(0.5, 1.5) draws, different from element to
element, so a slip between the plane's index kc*8 + e and the channel
layout cannot hide.
"""
import functools

import numpy as np
import pytest
import torch

import gemm_reference as G
from distributedllm_amd.engine import repack as RP

pytestmark = pytest.mark.gpu

GNAMES = ("q4_0", "q8_0")
COLS = (96, 160)
TS = (1, 16, 17, 64)
HEADS = {96: 6, 160: 5}           # head_dim 16 / 32, Ekv = E: even tile counts
GRID = [(g, c, T) for g in GNAMES for c in COLS for T in TS]


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    return ops.core()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _devmat(gname, rows, cols, tag):
    t, cpu, _ = G.operand(gname, rows, cols, tag)
    data, scales, wt = RP.repack_mfma(t, "cuda")
    assert torch.equal(data.cpu(), cpu[0])
    return data, scales, wt, rows, cols


def _id(a):
    return "-".join(str(x) for x in a)


def _fold_bits(v, nw):
    """u16 bits of f16(f16(v) * f16(nw)): the product of two f16 values is
    exact in f32, so numpy's f16 multiply rounds once, like the device's."""
    return (v.astype(np.float16) * nw.astype(np.float16)[None, :]).view(
        np.uint16)


def _check_channel(prep, jtw, rows, T, want_bits, what):
    prep = np.asarray(prep).view(np.uint16).reshape(-1)
    assert jtw == G.jt_width(T) and prep.size == G.side_numel(rows, jtw), what
    live, clean = G.prep_values(prep, rows, T, jtw)
    assert np.array_equal(live, want_bits), what + ": live elements"
    assert clean, what + ": dead columns / K-pad rows / slack not zero"


def test_norm_planes_are_not_periodic():
    """f16 has 1536 values in [0.5, 1.5], so a few of the draws coincide;
    what the index checks need is that no shift of a plane looks like the
    plane: every shift moves more than 9 elements in 10."""
    for c in COLS:
        for key in ("lm", "ffn", "qkv", "fold"):
            nw = G.norm_weights(key, c).astype(np.float16)
            for s in range(1, c):
                assert (np.roll(nw, s) != nw).mean() > 0.9


@pytest.mark.parametrize("args", GRID, ids=_id)
def test_qkv_slab(core, args):
    gname, E, T = args
    H = HEADS[E]
    assert core.qkv16_route(E, E, T, True) == 0
    c = G.qkv_case(gname, E, H, H, T)
    mats = [_devmat(gname, E, E, tag) for tag in ("wq", "wk", "wv")]
    k, v = _dev(c.Kf), _dev(c.Vf)
    q = core.qkv_project(*mats, _dev(c.x), _dev(c.nw), G.EPS, k, v,
                         _dev(c.pos), _dev(c.seq), _dev(c.inv_freq), H, H,
                         c.n_ctx, c.n_slots, 0)
    r = G.check(c, {"q": _np(q), "k": _np(k), "v": _np(v)})
    print(c.name, "worst / bound:", r)


@pytest.mark.parametrize("args", GRID, ids=_id)
def test_ffn(core, args):
    gname, cols, T = args
    c = G.ffn_case(gname, 96, cols, T)
    g, jtw = core.ffn_gate(_devmat(gname, 96, cols, "w1"),
                           _devmat(gname, 96, cols, "w3"), _dev(c.x),
                           _dev(c.nw), G.EPS, 0)
    r = G.check(c, {"gprep": _np(g).view(np.uint16), "jtw": int(jtw)})
    print(c.name, "worst / bound:", r)


@pytest.mark.parametrize("args", GRID, ids=_id)
def test_lmhead(core, args):
    gname, cols, T = args
    c = G.lmhead_case(gname, 512, cols, T)
    lg = core.gemm_lmhead(_devmat(gname, 512, cols, "lm"), _dev(c.x),
                          _dev(c.nw), G.EPS, 0)
    r = G.check(c, {"logits": _np(lg)})
    print(c.name, "worst / bound:", r)


@pytest.mark.parametrize("args", [(c, T) for c in COLS for T in TS + (70,)],
                         ids=_id)
def test_prep_x_bits(core, args):
    """k_prep_x: no plane -> f16(x), the bytes from before the fold; with a
    plane -> f16(f16(x) * f16(nw)); the sumsq is of x either way."""
    cols, T = args
    x = G.activations("fold", T, cols)
    nw = G.norm_weights("fold", cols)
    want_ss = (x.astype(np.float64) ** 2).sum(axis=1)
    for plane, bits in ((None, x.astype(np.float16).view(np.uint16)),
                        (_dev(nw), _fold_bits(x, nw))):
        prep, ss, jtw = core.prep_panel(_dev(x), plane)
        what = "prep cols=%d T=%d plane=%s" % (cols, T, plane is not None)
        _check_channel(_np(prep), int(jtw), cols, T, bits, what)
        ss = _np(ss).astype(np.float64)
        # f32 sum of cols squares, grouped by chunk / wave / atomics
        assert (np.abs(ss[:T] - want_ss) <=
                (cols + 64) * 2.0 ** -23 * want_ss).all(), what
        assert not ss[T:].any(), what


@pytest.mark.parametrize(
    "args", [(g, r, T, split) for g in GNAMES for r in COLS
             for T, split in [(t, s) for t in TS for s in (True, False)] +
             [(70, False)]], ids=_id)
def test_residual_producers_bits(core, args):
    """k_reduce_prep (split), the GM_RES_SQ epilogue (fused) and the
    k_gemm16_mt epilogue (T = 70). rows is the width of the xprep they
    write, so the consumer's K axis: 96 or 160."""
    gname, rows, T, split = args
    c = G.residual_case(gname, rows, 64, T, split)
    mat = _devmat(gname, rows, 64, "res")
    nw = G.norm_weights("fold", rows)
    b, y_in = _dev(c.b), _dev(c.y_in)
    # no plane: every check of test_gpu_gemm.py, xprep == f16(y) included
    y0, xp0, ss0, jtw0 = core.gemm_residual(mat, b, y_in, split, 0)
    G.check(c, {"y": _np(y0), "xprep": _np(xp0).view(np.uint16),
                "ss": _np(ss0), "jtw": int(jtw0)})
    y1, xp1, ss1, jtw1 = core.gemm_residual(mat, b, y_in, split, 0,
                                            _dev(nw))
    # the plane changes the side channel alone
    assert torch.equal(y1, y0)
    # ... and the sumsq stays that of the un-normalised y
    want = (_np(y1).astype(np.float64) ** 2).sum(axis=1)
    ss = _np(ss1).astype(np.float64)
    assert (np.abs(ss[:T] - want) <= (rows + 64) * 2.0 ** -23 * want).all()
    assert not ss[T:].any()
    _check_channel(_np(xp1), int(jtw1), rows, T, _fold_bits(_np(y1), nw),
                   c.name + " with a plane")
