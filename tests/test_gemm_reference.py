"""CPU checks of tests/gemm_reference.py: the float64 reference agrees with
the formats layer's dequantised weights, the simulator's own reading of
the tile layouts agrees with detile_mfma bit for bit, the unmutated
simulator (f32 accumulation in the kernels' order) passes every check of
the GPU case matrix, and each of the twelve mutants is rejected by the
same inputs, bounds and helpers wherever it touches live data. That last
part is what keeps tests/test_gpu_gemm.py honest: a kernel that computed a
mutant would fail it."""
import math

import numpy as np
import pytest
import torch

import gemm_reference as G
from distributedllm_amd.engine import repack as RP

CASES = G.all_cases()
# the mutants run where every type and route appears: T = 17 and the
# large-M T of each type, plus the RT = 2 / RT = 4 and eight-slice shapes
MUTANT_CASES = [(r, a) for r, a in CASES
                if (a[4] if r == "qkv" else a[3]) in (17, 70, 130, 330, 480)]


def _id(ra):
    return ra[0] + "-" + "-".join(str(x) for x in ra[1])


@pytest.mark.parametrize("gname", G.NONK + G.KQ)
def test_reference_agrees_with_the_formats_layer(gname):
    rows, cols = 48, 768
    t, mat, A = G.operand(gname, rows, cols, "fmt")
    W = t.to_f32().astype(np.float64)
    # the repack tolerance of test_detile_inverts_repack
    wtol = 4e-3 * np.abs(W).max() + 1e-6
    assert np.abs(A - W).max() <= wtol
    B = G.panel_plain(G.activations("fmt", 17, cols))
    val, sabs = G.product(A, B)
    assert (np.abs(val - B @ W.T) <=
            wtol * np.abs(B).sum(axis=1)[:, None]).all()
    assert (sabs >= np.abs(val) - 1e-12).all()
    # the simulator's independent reading of the tiles: the same f16 values
    dec = G.decode_tiles(mat, rows, cols)
    Af = G.a_fragments(dec).reshape(rows, -1)
    assert np.array_equal(Af[:, :cols].astype(np.float64), A)
    assert not Af[:, cols:].any()          # pad blocks are exact zeros


def test_norm_panel_is_the_rms_norm():
    x = G.activations("n", 5, 64)
    nw = G.norm_weights("n", 64)
    want = (x.astype(np.float64) /
            np.sqrt((x.astype(np.float64) ** 2).mean(1) + G.EPS)[:, None]
            * nw)
    got = G.panel_norm(x, nw)
    assert np.abs(got - want).max() <= 3 * G.U16 * np.abs(want).max()
    sim = G.sim_norm_panel(x, nw, 5)
    assert np.abs(sim - got).max() <= 2 * G.U16 * np.abs(want).max()


def test_init_range_partitions_the_block_range():
    for b0, b1 in ((0, 2), (0, 4), (0, 21), (0, 24), (4, 8), (20, 21),
                   (24, 24), (0, 172)):
        for align in (1, 4):
            if align == 4 and (b0 % 4 or b1 % 4):
                continue
            rs = [G.init_range(b0, b1, align, w) for w in range(4)]
            assert rs[0][0] == b0 and rs[-1][1] == b1
            for (a0, a1), (c0, _) in zip(rs, rs[1:]):
                assert a0 <= a1 == c0
            assert all(a0 % align == 0 for a0, _ in rs)
    # the shapes the issue names: 6/6/6/3 (f16, cols = 672), three empty
    # waves at cols = 64
    assert [G.init_range(0, 21, 1, w) for w in range(4)] == \
        [(0, 6), (6, 12), (12, 18), (18, 21)]
    assert [G.init_range(0, 4, 4, w) for w in range(4)] == \
        [(0, 4), (4, 4), (4, 4), (4, 4)]
    assert G._slices(4, 8) == [(0, 4)] + [(4, 4)] * 7
    assert all(b1 > b0 for b0, b1 in G._slices(32, 8))


def test_case_matrix_reaches_every_route_variant():
    res = [G.residual_case(*a) for a in G.residual_cases() if a[0] == "q4_0"
           and a[3] in (17, 65, 480)]
    assert {G.gemm16_mt_rt(c.rows, c.T) for c in res if c.T > 64} == {1, 2}
    assert {G.gemm16_plain_rt(a[1]) for a in G.lmhead_cases()} == {1, 2, 4}
    ffn = G.ffn_cases()
    assert {G.ffn16_rt(a[1], a[3]) for a in ffn if a[3] <= 64} == {1, 2}
    assert {G.ffn16_rt(a[1], a[3]) for a in ffn if a[3] > 64} == {1, 2}
    qkv = G.qkv_cases() + [G.BIG_QKV]
    ekv = lambda a: a[1] // a[2] * a[3]
    assert {G.qkv16_route(a[1], ekv(a), a[4], True) for a in qkv
            if a[4] <= 64} == {0, 1, 2}
    assert {G.qkv16_mt_rt(a[1], ekv(a), a[4]) for a in qkv
            if a[4] > 64} == {1, 2}


@pytest.mark.parametrize("ra", CASES, ids=_id)
def test_simulator_passes_every_check(ra):
    c = G.make_case(*ra)
    r = G.check(c, G.simulate(c))
    print(c.name, "worst / bound:",
          {k: round(v, 4) for k, v in r.items() if v})


@pytest.mark.parametrize("m", sorted(G.MUTANTS))
def test_mutant_is_rejected(m):
    """Every case the mutant applies to rejects it; it applies on every
    route it can exist on. Prints how far over the bound it lands."""
    pad_fill = 1.0 if m == 5 else 0.0
    worst = {}
    for ra in MUTANT_CASES:
        c = G.make_case(*ra)
        if not G.mutant_applies(c, m):
            continue
        if m == 5:
            # Pad blocks meet K-pad panel rows, which the engine keeps
            # at zero: 0 * anything finite is 0 and the mutant cannot be
            # seen. The contract is only that those rows are FINITE, so
            # they hold 1.0 here: the true kernel is unmoved by that
            # (alpha = beta = 0 gives exact zeros) ...
            a, b = G.simulate(c), G.simulate(c, 0, pad_fill)
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]))
        r = G.ratios(c, G.simulate(c, m, pad_fill))
        over = max(r.values())
        assert over > 1.0, (m, G.MUTANTS[m], c.name, r)
        worst.setdefault(c.route, []).append(over)
    routes = {1: 4, 2: 4, 3: 4, 4: 4, 5: 4, 6: 4, 7: 2, 8: 1, 9: 3, 10: 1,
              11: 2, 12: 4}
    assert len(worst) == routes[m], (m, sorted(worst))
    for route, v in sorted(worst.items()):
        fin = [x for x in v if math.isfinite(x)]
        print("mutant %2d (%s) %-8s %3d cases, error / bound >= %s%s" % (
            m, G.MUTANTS[m], route, len(v),
            "%.3g" % min(fin) if fin else "-",
            ", %d fail an exact relation" % (len(v) - len(fin))
            if len(fin) < len(v) else ""))
