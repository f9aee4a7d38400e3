"""Direct tests of the MFMA dequant-GEMM family (ops/csrc/mfma_gemm.hip)
through the test hooks of the extension - gemm_residual, gemm_lmhead,
ffn_gate, qkv_project - against the float64 reference in
gemm_reference.py.

Weights are normal(0, 0.02) matrices quantised by the formats layer and
tiled on the device by repack_mfma; the reference sees the tiles through
detile_mfma(float64), rounded to f16 once. Every case
  * holds each output to its derived bound (gemm_reference.py,
    docs/kernels.md) and prints worst error / bound,
  * checks the relations among the kernel's own outputs: the f16 side
    channel bit-equal to f16(y) and zero everywhere else, the sumsq
    channel against the float64 sum of squares of the device's y, every
    cache element outside the written rows untouched,
  * runs the launch twice and demands bit-identical results (the sumsq
    channel excepted: its atomics commute only approximately),
  * repeats it with the dead token columns of the input panel holding f16
    NaN and 65504 and demands the same bits again.
The inputs, bounds and helpers are the ones tests/test_gemm_reference.py
proves to reject all twelve mutant kernels.

Worst error / bound measured on an MI355X (also in docs/kernels.md,
"Direct kernel tests"): residual y 3.1 %, ss 1.0 %, lm_head logits 38 %,
gprep 26 %, q 24 %, K rows 33 %, V rows 40 %; the E = 5504 case 1.4 % /
1.8 % / 2.8 %. The CPU simulator lands on the same figures.

The launchers' route selectors decide by model size; the shapes here are
the smallest that reach every value they can return
(test_every_route_variant_is_covered).
"""
import functools

import numpy as np
import pytest
import torch

import gemm_reference as G
from distributedllm_amd.engine import repack as RP
from distributedllm_amd.formats import ggml

pytestmark = pytest.mark.gpu

FILLS = (0x7E00, 0x7BFF)          # f16 NaN, 65504


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    return ops.core()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _devmat(gname, rows, cols, tag):
    """(data, scales, wtype, rows, cols) tiled on the device; the same
    bytes as the CPU tiles the reference was read from."""
    t, cpu, _ = G.operand(gname, rows, cols, tag)
    data, scales, wt = RP.repack_mfma(t, "cuda")
    assert wt == cpu[2] == G.WTYPE[gname]
    assert torch.equal(data.cpu(), cpu[0])
    assert torch.equal(scales.cpu(), cpu[1])
    return data, scales, wt, rows, cols


def _np(t):
    return t.cpu().numpy()


def _run(core, c, fill):
    if c.route == "residual":
        y, xp, ss, jtw = core.gemm_residual(
            _devmat(c.gname, c.rows, c.cols, "res"), _dev(c.b),
            _dev(c.y_in), c.split, fill)
        return {"y": _np(y), "xprep": _np(xp).view(np.uint16),
                "ss": _np(ss), "jtw": int(jtw)}
    if c.route == "lmhead":
        lg = core.gemm_lmhead(_devmat(c.gname, c.rows, c.cols, "lm"),
                              _dev(c.x), _dev(c.nw), G.EPS, fill)
        return {"logits": _np(lg)}
    if c.route == "ffn":
        g, jtw = core.ffn_gate(_devmat(c.gname, c.rows, c.cols, "w1"),
                               _devmat(c.gname, c.rows, c.cols, "w3"),
                               _dev(c.x), _dev(c.nw), G.EPS, fill)
        return {"gprep": _np(g).view(np.uint16), "jtw": int(jtw)}
    mats = c.devmats if hasattr(c, "devmats") else [
        _devmat(c.gname, r, c.E, tag) for r, tag in
        ((c.E, "wq"), (c.Ekv, "wk"), (c.Ekv, "wv"))]
    k, v = _dev(c.Kf), _dev(c.Vf)
    q = core.qkv_project(*mats, _dev(c.x), _dev(c.nw), G.EPS, k, v,
                         _dev(c.pos), _dev(c.seq), _dev(c.inv_freq), c.H,
                         c.Hkv, c.n_ctx, c.n_slots, fill)
    return {"q": _np(q), "k": _np(k), "v": _np(v)}


def _same_bits(a, b, what):
    for key in a:
        if key == "ss":
            continue
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.shape == y.shape and np.array_equal(
            x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8)), \
            "%s: %s differs" % (what, key)


def _direct(core, c):
    first = _run(core, c, 0)
    _same_bits(first, _run(core, c, 0), c.name + ": two launches")
    r = G.check(c, first)
    print(c.name, "worst / bound:",
          {k: float("%.3g" % v) for k, v in r.items() if v})
    for key in ("y", "logits", "q"):
        if key in first:
            assert np.isfinite(first[key]).all()
    for fill in FILLS:
        _same_bits(first, _run(core, c, fill),
                   "%s: dead columns = %#x" % (c.name, fill))
    torch.cuda.synchronize()


def _id(a):
    return "-".join(str(x) for x in a)


def test_restated_host_functions_match_the_extension(core):
    """init_range and xprep_index are device functions with nothing to
    call from here: the restated xprep_index is held to the device's by
    every side-channel check below (k_prep_x writes the panel the GEMMs
    read; the epilogues write the channels read back), init_range by the
    unmutated simulator agreeing with the kernels inside the same
    bounds."""
    for T in list(range(1, 70)) + [100, 127, 128, 129, 330, 480, 1000]:
        assert core.jt_width(T) == G.jt_width(T)
    rows = [16 * r for r in list(range(1, 40)) + [
        127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1026,
        1791, 1792, 1793, 1796, 2000, 2048, 4096]]
    for r in rows:
        assert core.gemm16_ks(r) == G.gemm16_ks(r)
        assert core.gemm16_plain_rt(r) == G.gemm16_plain_rt(r)
        for T in (1, 17, 64, 65, 128, 129, 480, 4096):
            assert core.ffn16_rt(r, T) == G.ffn16_rt(r, T)
            if T > 64:
                assert core.gemm16_mt_rt(r, T) == G.gemm16_mt_rt(r, T)
        for T in (1, 17, 64, 65, 128, 4096):
            for ok in (False, True):
                assert core.gemm16_res_route(r, T, ok) == \
                    G.gemm16_res_route(r, T, ok)
    for E, Ekv in [(64, 64), (64, 32), (64, 16), (96, 48), (256, 64),
                   (672, 336), (1024, 1024), (4096, 1024), (5504, 5504),
                   (5472, 5472), (8192, 1024), (5120, 5120), (5136, 5136)]:
        for has_slab in (False, True):
            assert core.qkv16_route(E, Ekv, 17, has_slab) == \
                G.qkv16_route(E, Ekv, 17, has_slab)
        for T in (65, 130, 330, 4096):
            assert core.qkv16_mt_rt(E, Ekv, T) == G.qkv16_mt_rt(E, Ekv, T)
        assert core.qkv16_ks(E, Ekv) == G.AR.qkv16_ks_ref(E, Ekv)


def test_every_route_variant_is_covered(core):
    """The selectors, evaluated on the case list, return every value they
    can return; every (wtype, route) pair runs at a decode T and, where
    the route has one, at a large-M T."""
    res, lm = G.residual_cases(), G.lmhead_cases()
    ffn, qkv = G.ffn_cases(), G.qkv_cases() + [G.BIG_QKV]
    assert {core.gemm16_plain_rt(a[1]) for a in lm} == {1, 2, 4}
    assert {core.gemm16_mt_rt(a[1], a[3]) for a in res if a[3] > 64} == \
        {1, 2}
    assert {core.ffn16_rt(a[1], a[3]) for a in ffn if a[3] <= 64} == {1, 2}
    assert {core.ffn16_rt(a[1], a[3]) for a in ffn if a[3] > 64} == {1, 2}
    ekv = lambda a: a[1] // a[2] * a[3]
    assert {core.qkv16_route(a[1], ekv(a), a[4], True) for a in qkv
            if a[4] <= 64} == {0, 1, 2}
    assert {core.qkv16_mt_rt(a[1], ekv(a), a[4]) for a in qkv
            if a[4] > 64} == {1, 2}
    # decode residual: GM_SLAB (rows/16 even), GM_RES_SQ at odd and even
    assert {(a[1] // 16 % 2, a[4]) for a in res if a[3] <= 64} == \
        {(1, False), (0, True), (0, False)}
    # the residual hook passes split as split_ok; T > 64 cases have it off
    assert {core.gemm16_res_route(a[1], a[3], a[4]) for a in res} == \
        {0, 1, 2}
    assert {a[1] // 16 % 2 for a in res if a[3] <= 64
            and core.gemm16_res_route(a[1], a[3], a[4]) == 1} == {0, 1}
    assert all(core.gemm16_res_route(a[1], a[3], False) == 1
               for a in res if a[3] <= 64)
    assert {core.gemm16_ks(a[1]) for a in res if a[4]} == {8}
    wtypes = set(G.WTYPE.values())
    for cases, ti in ((res, 3), (ffn, 3), (qkv, 4)):
        assert {G.WTYPE[a[0]] for a in cases if a[ti] <= 64} == wtypes
        assert {G.WTYPE[a[0]] for a in cases if a[ti] > 64} == wtypes
    assert {G.WTYPE[a[0]] for a in lm} == wtypes


@pytest.mark.parametrize("args", G.residual_cases(), ids=_id)
def test_residual(core, args):
    _direct(core, G.residual_case(*args))


@pytest.mark.parametrize("args", G.lmhead_cases(), ids=_id)
def test_lmhead(core, args):
    _direct(core, G.lmhead_case(*args))


@pytest.mark.parametrize("args", G.ffn_cases(), ids=_id)
def test_ffn_gate(core, args):
    _direct(core, G.ffn_case(*args))


@pytest.mark.parametrize("args", G.qkv_cases(), ids=_id)
def test_qkv(core, args):
    _direct(core, G.qkv_case(*args))


def test_qkv_fused_decode_rt2(core):
    """k_qkv16<…, JT, 2>, the fused decode route of 30B-class models:
    (E + 2 Ekv)/16 = 1032 >= 1024 row tiles. About 60 MB of q4_0 weights,
    drawn in the tile layout on the device; the reference product runs in
    torch.float64 on the device, in row chunks."""
    gname, E, H, Hkv, T = G.BIG_QKV
    assert core.qkv16_route(E, E // H * Hkv, T, True) == 2
    c = G.NS(route="qkv", name="qkv-%s-E%d-T%d" % (gname, E, T),
             gname=gname, E=E, H=H, Hkv=Hkv, T=T)
    G.qkv_inputs(c)
    gen = torch.Generator(device="cuda").manual_seed(7)
    B = G.panel_norm(c.x, c.nw)
    Bd = _dev(B)
    c.devmats, res = [], []
    for rows in (E, c.Ekv, c.Ekv):
        data, sc, wt = RP.random_tiles(ggml.GGML_TYPE_Q4_0, rows, E, gen)
        c.devmats.append((data, sc, wt, rows, E))
        val = np.empty((T, rows))
        sabs = np.empty((T, rows))
        amax = 0.0
        for r0 in range(0, rows, 1376):           # 4 chunks of 86 tiles
            r1 = min(rows, r0 + 1376)
            R0, R1, nbp = r0 // 16, r1 // 16, RP.padded_blocks(E // 32)
            part = (data[R0 * nbp * 64:R1 * nbp * 64],
                    sc[R0 * nbp * 32:R1 * nbp * 32], wt)
            A = (RP.detile_mfma(part, r1 - r0, E, torch.float64)
                 .to(torch.half).to(torch.float64))
            val[:, r0:r1] = _np(Bd @ A.T)
            sabs[:, r0:r1] = _np(Bd.abs() @ A.abs().T)
            amax = max(amax, float(A.abs().max()))
        res.append((val, G.tol_norm(E, sabs, amax, np.abs(B).max())))
    G.qkv_reference(c, res[0][0], res[1][0], res[2][0], res[0][1],
                    res[1][1], res[2][1])
    _direct(core, c)


def test_hooks_refuse_what_could_go_out_of_bounds(core):
    c = G.residual_case("q4_0", 64, 64, 17, True)
    mat = _devmat("q4_0", 64, 64, "res")
    b, y = _dev(c.b), _dev(c.y_in)
    core.gemm_residual(mat, b, y, True, 0)
    data, sc, wt, rows, cols = mat

    def res(mat=mat, b=b, y=y, split=True, fill=0):
        return core.gemm_residual(mat, b, y, split, fill)

    bad = [
        dict(mat=(data[:-1].contiguous(), sc, wt, rows, cols)),   # slack
        dict(mat=(data, sc[:-1].contiguous(), wt, rows, cols)),
        dict(mat=(data.cpu(), sc, wt, rows, cols)),
        dict(mat=(data.float(), sc, wt, rows, cols)),
        dict(mat=(data, sc.float(), wt, rows, cols)),
        dict(mat=(data, sc, RP.W_Q8B, rows, cols)),               # wtype
        dict(mat=(data, sc, RP.W_F32, rows, cols)),
        dict(mat=(data, sc, wt, rows + 8, cols)),                 # rows % 16
        dict(mat=(data, sc, wt, rows, cols + 16)),                # cols % 32
        dict(mat=(data, sc, wt, rows + 16, cols)),                # numel
        dict(mat=(data, sc, wt, rows, cols)[:4]),
        dict(b=b.double()), dict(b=b.cpu()), dict(y=y.half()),
        dict(b=b.repeat(1, 2)[:, ::2]),                           # strided
        dict(b=b.repeat(1, 2)),                                   # cols
        dict(b=b[:, :32].contiguous()),
        dict(y=y[:-1].contiguous()),                              # T
        dict(y=y[:, :48].contiguous()),                           # rows
        dict(b=b[:0].contiguous(), y=y[:0].contiguous()),         # T = 0
        dict(b=torch.zeros(4097, cols, device="cuda"),
             y=torch.zeros(4097, rows, device="cuda"), split=False),
        dict(b=torch.zeros(65, cols, device="cuda"),              # split is
             y=torch.zeros(65, rows, device="cuda")),             # decode
        dict(fill=1 << 16), dict(fill=-(1 << 15) - 1),
    ]
    for kw in bad:
        with pytest.raises((RuntimeError, TypeError)):
            res(**kw)
    # split-K needs an even tile count: the engine's rule
    odd = G.residual_case("q4_0", 48, 64, 17, False)
    m48 = _devmat("q4_0", 48, 64, "res")
    core.gemm_residual(m48, _dev(odd.b), _dev(odd.y_in), False, 0)
    with pytest.raises(RuntimeError):
        core.gemm_residual(m48, _dev(odd.b), _dev(odd.y_in), True, 0)

    lm = G.lmhead_case("q4_0", 512, 64, 17)
    m = _devmat("q4_0", 512, 64, "lm")
    x, nw = _dev(lm.x), _dev(lm.nw)
    core.gemm_lmhead(m, x, nw, G.EPS, 0)
    for args in ((m, x, nw[:-1].contiguous(), G.EPS, 0),
                 (m, x, nw.double(), G.EPS, 0),
                 (m, x.repeat(1, 2), nw, G.EPS, 0),
                 (m, torch.zeros(65, 64, device="cuda"), nw, G.EPS, 0),
                 (m, x.cpu(), nw, G.EPS, 0)):
        with pytest.raises(RuntimeError):
            core.gemm_lmhead(*args)

    f = G.ffn_case("q4_0", 96, 64, 17)
    m1, m3 = _devmat("q4_0", 96, 64, "w1"), _devmat("q4_0", 96, 64, "w3")
    x, nw = _dev(f.x), _dev(f.nw)
    core.ffn_gate(m1, m3, x, nw, G.EPS, 0)
    for args in ((m1, m48, x, nw, G.EPS, 0),                      # rows
                 (m1, _devmat("q4_0", 96, 672, "w3"), x, nw, G.EPS, 0),
                 (m1, _devmat("q4_1", 96, 64, "w3"), x, nw, G.EPS, 0),
                 (m1, m3, x, nw[:-1].contiguous(), G.EPS, 0),
                 (m1, m3, x[:, :32].contiguous(), nw, G.EPS, 0)):
        with pytest.raises(RuntimeError):
            core.ffn_gate(*args)

    q = G.qkv_case("q4_0", 64, 4, 2, 17)
    mats = [_devmat("q4_0", r, 64, tag) for r, tag in
            ((64, "wq"), (32, "wk"), (32, "wv"))]

    def qkv(mats=mats, x=q.x, nw=q.nw, kf=q.Kf, vf=q.Vf, pos=q.pos,
            seq=q.seq, inv=q.inv_freq, H=q.H, Hkv=q.Hkv, ctx=q.n_ctx,
            slots=q.n_slots):
        return core.qkv_project(*mats, _dev(x), _dev(nw), G.EPS, _dev(kf),
                                _dev(vf), _dev(pos), _dev(seq), _dev(inv),
                                H, Hkv, ctx, slots, 0)

    qkv()
    dup_pos, dup_seq = q.pos.copy(), q.seq.copy()
    dup_pos[3], dup_seq[3] = dup_pos[9], dup_seq[9]
    wq4 = _devmat("q4_0", 64, 64, "wq")
    bad = [
        dict(kf=q.Kf[:-16]), dict(vf=q.Vf[:-1]),                  # pad
        dict(kf=q.Kf.astype(np.float32)),
        dict(pos=q.pos + 64), dict(pos=q.pos - 64),               # ranges
        dict(seq=q.seq + q.n_slots),
        dict(pos=q.pos.astype(np.int64)),
        dict(pos=dup_pos, seq=dup_seq),                           # same row
        dict(pos=q.pos[:-1]), dict(inv=q.inv_freq[:-1]),
        dict(nw=q.nw[:-1]), dict(x=q.x[:, :32]),
        dict(Hkv=3), dict(Hkv=4), dict(H=8, Hkv=4),               # heads
        dict(mats=[mats[0], wq4, mats[2]]),                       # Ekv
        dict(mats=[mats[0], _devmat("q4_1", 32, 64, "wk"), mats[2]]),
        dict(mats=[_devmat("q4_0", 64, 672, "res"), mats[1], mats[2]]),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            qkv(**kw)
    torch.cuda.synchronize()
