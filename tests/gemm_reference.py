"""float64 reference of the MFMA dequant-GEMM family (ops/csrc/
mfma_gemm.hip) with the inputs, derived bounds and assertion helpers that
tests/test_gpu_gemm.py (the kernels) and tests/test_gemm_reference.py (a
CPU simulator and its twelve mutants) share. numpy only, no GPU.

Reference. Operands are emulated exactly where the kernel's rounding is
deterministic, everything after that is float64:
  A       float16 of detile_mfma(..., float64): ONE rounding of
          alpha * n + beta, what a_frag_q4 / a_frag_q8 claim to compute
  panel   float16(x)
  NORM    v = float16(x16 * float16(norm_w)); the column scale
          s = 1 / sqrt(mean(x^2) + eps) in float64 from the f32 x, not
          rounded; b = v * s
Alongside each product the reference returns S_abs[t, r] =
sum_k |A[r, k] b[k, t]|, the quantity all bounds scale with.

Bounds (derivation: docs/kernels.md, "Direct kernel tests"):
  tol_acc = 2 (cols + 16) 2^-24 S_abs + cols 2^-24 max|A| max|b|
  NORM    + (2 * 2^-11 + 2^-20) S_abs
  y       + 2^-23 |y|;  f16 outputs + 2^-11 |value|
  gprep   1.1 tol_1 |v3| + |silu(v1)| tol_3 + 1e-6 |g| + 2^-11 |g|
  q / K   sqrt(2) tol + 2^-21 |row|  (+ 2^-11 |value| for K), pos <= 63

Simulator. `simulate(case, mutant)` runs the same operands through the
kernels' own order in float32: per-wave K ranges from a restated
init_range, the two alternating accumulators of the low-parallelism
shapes, the 4-wave combine, the split-K slices and their reducer, the
two f16 roundings of the NORM build, f32 SwiGLU and RoPE. It decodes the
tiles on its own (`decode_tiles`), independently of detile_mfma. The
mutants are switches of that simulator (MUTANTS).
"""
import functools
import math
import zlib
from types import SimpleNamespace as NS

import numpy as np
import torch

import attention_reference as AR
from distributedllm_amd.engine import repack as RP
from distributedllm_amd.formats import ggml

U32 = 2.0 ** -24          # unit roundoff of f32
U16 = 2.0 ** -11          # unit roundoff of f16
TOL_NORM = 2 * U16 + 2.0 ** -20
EPS = 1e-5
N_CTX = 64                # cache rows per slot in the qkv cases (pos <= 63)
POISON = 30000.0          # finite fill of every cache row

GTYPES = {"q4_0": ggml.GGML_TYPE_Q4_0, "q4_1": ggml.GGML_TYPE_Q4_1,
          "q8_0": ggml.GGML_TYPE_Q8_0, "q5_1": ggml.GGML_TYPE_Q5_1,
          "q4_K": ggml.GGML_TYPE_Q4_K, "q2_K": ggml.GGML_TYPE_Q2_K,
          "q6_K": ggml.GGML_TYPE_Q6_K, "f16": ggml.GGML_TYPE_F16}
WTYPE = {"q4_0": RP.W_Q4_0, "q4_1": RP.W_Q4_1, "q8_0": RP.W_Q8B,
         "q5_1": RP.W_Q8B, "q4_K": RP.W_Q8B, "q2_K": RP.W_Q8B16,
         "q6_K": RP.W_Q8B16, "f16": RP.W_F16}
NONK = ["q4_0", "q4_1", "q8_0", "q5_1", "f16"]
KQ = ["q4_K", "q2_K", "q6_K"]

MUTANTS = {
    1: "last K-block of the last non-empty wave range dropped",
    2: "(alpha, beta) of block kb ^ 1",
    3: "W_Q8B16: half-plane 0 for all four k-spans",
    4: "beta dropped",
    5: "q4/byte pad blocks scaled like the neighbouring real block",
    6: "column T-1 masked",
    7: "split-K reducer stops at ks-1",
    8: "residual not added",
    9: "NORM scale of token tile 0 applied to every tile",
    10: "w1 and w3 swapped in SwiGLU",
    11: "large-M side-channel write with panel stride 4",
    12: "f16 tail after full batches restarts one batch late",
}


def f16(a):
    """Round float64/float32 to f16 once, returned as float64."""
    return np.asarray(a).astype(np.float16).astype(np.float64)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------ host functions, restated
# (compared with the extension in test_gpu_gemm.py)

def pick_jt(T):
    return 1 if T <= 16 else 2 if T <= 32 else 4


jt_width = AR.jt_width_ref
xprep_index = AR.xprep_index


def init_range(b0, b1, align, wid, nwaves=4):
    """KLoop::init_range: wave wid's [kb0, kb1) of the block range."""
    per = (b1 - b0 + nwaves - 1) // nwaves
    per = (per + align - 1) & ~(align - 1)
    kb0 = min(b1, b0 + wid * per)
    return kb0, min(b1, kb0 + per)


def gemm16_ks(rows):
    R, ks = rows // 16, 1
    while R * ks < 512 and ks < 8:
        ks <<= 1
    return max(ks, 2)


def _rt2_fills(tiles, MT):
    return tiles % 2 == 0 and (tiles // 2) * MT >= 512


def _mt(T):
    return (T + 63) >> 6


def gemm16_plain_rt(rows):
    R = rows // 16
    if R % 4 == 0 and R // 4 >= 448:
        return 4
    return 2 if R % 2 == 0 and R >= 1024 else 1


def ffn16_rt(rows, T):
    return 2 if _rt2_fills(rows // 16, 1 if T <= 64 else _mt(T)) else 1


def gemm16_mt_rt(rows, T):
    return 2 if _rt2_fills(rows // 16, _mt(T)) else 1


def gemm16_res_route(rows, T, split_ok):
    """wo / w2: 0 slab split-K + reduce pass, 1 fused, 2 large-M."""
    if T > 64:
        return 2
    return 0 if split_ok and rows // 16 % 2 == 0 else 1


def _qkv_rt2_ok(E, Ekv):
    return (E >> 4) % 2 == 0 and (Ekv >> 4) % 2 == 0


def qkv16_route(E, Ekv, T, has_slab):
    tiles3 = (E + 2 * Ekv) >> 4
    ok = _qkv_rt2_ok(E, Ekv)
    if has_slab and tiles3 < 1024 and ok:
        return 0
    return 2 if ok and _rt2_fills(tiles3, 1) else 1


def qkv16_mt_rt(E, Ekv, T):
    return 2 if (_qkv_rt2_ok(E, Ekv) and
                 _rt2_fills((E + 2 * Ekv) >> 4, _mt(T))) else 1


def side_numel(cols, jtw):
    """The engine's side(cols) rule at panel width jtw."""
    return RP.padded_blocks(cols // 32) * 512 * jtw + 8192


# ------------------------------------------------------------- operands

@functools.lru_cache(maxsize=None)
def weight(gname, rows, cols, tag):
    a = _rng("w", gname, rows, cols, tag).normal(0.0, 0.02, (rows, cols))
    return ggml.GGMLTensor.from_f32("w", a.astype(np.float32), GTYPES[gname])


@functools.lru_cache(maxsize=None)
def operand(gname, rows, cols, tag):
    """-> (GGMLTensor, its CPU tiles, A [rows, cols] float64 holding f16
    values: one rounding of the float64 detile)."""
    t = weight(gname, rows, cols, tag)
    mat = RP.repack_mfma(t, "cpu")
    A = f16(RP.detile_mfma(mat, rows, cols, torch.float64).numpy())
    return t, mat, A


def activations(key, T, cols):
    """normal(0, 0.5); tokens 1 and T-1 scaled by 8 so that the column
    scales of the NORM routes differ between token tiles."""
    x = _rng("x", key, T, cols).normal(0.0, 0.5, (T, cols))
    x[T - 1] *= 8.0
    if T >= 3:
        x[1] *= 8.0
    return x.astype(np.float32)


def norm_weights(key, cols):
    return _rng("n", key, cols).uniform(0.5, 1.5, cols).astype(np.float32)


def panel_plain(b):
    return f16(b)


def panel_norm(x, nw, eps=EPS):
    v = f16(f16(x) * f16(nw)[None, :])
    s = 1.0 / np.sqrt((x.astype(np.float64) ** 2).mean(axis=1) + eps)
    return v * s[:, None]


def product(A, B):
    """B [T, cols], A [rows, cols] -> (B A^T, |B| |A|^T), float64."""
    return B @ A.T, np.abs(B) @ np.abs(A).T


def tol_acc(cols, sabs, amax, bmax):
    return 2 * (cols + 16) * U32 * sabs + cols * U32 * amax * bmax


def tol_norm(cols, sabs, amax, bmax):
    return tol_acc(cols, sabs, amax, bmax) + TOL_NORM * sabs


def silu(v):
    return v / (1.0 + np.exp(-v))


def tol_gate(v1, v3, t1, t3):
    g = silu(v1) * v3
    return (1.1 * t1 * np.abs(v3) + np.abs(silu(v1)) * t3 +
            1e-6 * np.abs(g) + U16 * np.abs(g))


def tol_rope(tol, pre, D, is_k, rot):
    """Bound of a rotated row from the bound `tol` of the unrotated one:
    each output is x0 c -+ x1 s with c^2 + s^2 = 1, so its error is at
    most sqrt(e0^2 + e1^2) <= sqrt(2) max(e0, e1); the sin/cos and the
    two f32 products add 2^-21 of the largest pair norm of the row."""
    pair = np.maximum(tol[:, 0::2], tol[:, 1::2])
    pair = np.repeat(pair, 2, axis=1)
    norm = np.sqrt(pre[:, 0::2] ** 2 + pre[:, 1::2] ** 2).max(axis=1)
    out = math.sqrt(2.0) * pair + 2.0 ** -21 * norm[:, None]
    return out + U16 * np.abs(rot) if is_k else out


# ---------------------------------------------------------------- cases

def _finish(c):
    c.jtw = jt_width(c.T)
    c.wtype = WTYPE[c.gname]
    return c


@functools.lru_cache(maxsize=None)
def residual_case(gname, rows, cols, T, split):
    t, mat, A = operand(gname, rows, cols, "res")
    c = NS(route="residual", name="res-%s-%dx%d-T%d-%s" % (
        gname, rows, cols, T, "split" if split else "fused"),
        gname=gname, rows=rows, cols=cols, T=T, split=split, t=t, mat=mat)
    c.b = activations("res", T, cols)
    c.y_in = _rng("y", rows, T).normal(0.0, 1.0, (T, rows)).astype(np.float32)
    B = panel_plain(c.b)
    c.prod, sabs = product(A, B)
    c.ref = c.y_in.astype(np.float64) + c.prod
    c.tol = (tol_acc(cols, sabs, np.abs(A).max(), np.abs(B).max()) +
             2.0 ** -23 * np.abs(c.ref))
    return _finish(c)


@functools.lru_cache(maxsize=None)
def lmhead_case(gname, rows, cols, T):
    t, mat, A = operand(gname, rows, cols, "lm")
    c = NS(route="lmhead", name="lm-%s-%dx%d-T%d" % (gname, rows, cols, T),
           gname=gname, rows=rows, cols=cols, T=T, t=t, mat=mat)
    c.x = activations("lm", T, cols)
    c.nw = norm_weights("lm", cols)
    B = panel_norm(c.x, c.nw)
    c.ref, sabs = product(A, B)
    c.tol = tol_norm(cols, sabs, np.abs(A).max(), np.abs(B).max())
    return _finish(c)


@functools.lru_cache(maxsize=None)
def ffn_case(gname, rows, cols, T):
    t1, mat1, A1 = operand(gname, rows, cols, "w1")
    t3, mat3, A3 = operand(gname, rows, cols, "w3")
    c = NS(route="ffn", name="ffn-%s-%dx%d-T%d" % (gname, rows, cols, T),
           gname=gname, rows=rows, cols=cols, T=T, t=t1, t3=t3, mat=mat1,
           mat3=mat3)
    c.x = activations("ffn", T, cols)
    c.nw = norm_weights("ffn", cols)
    B = panel_norm(c.x, c.nw)
    bmax = np.abs(B).max()
    v1, s1 = product(A1, B)
    v3, s3 = product(A3, B)
    c.ref = silu(v1) * v3
    c.tol = tol_gate(v1, v3, tol_norm(cols, s1, np.abs(A1).max(), bmax),
                     tol_norm(cols, s3, np.abs(A3).max(), bmax))
    return _finish(c)


def qkv_positions(T):
    """Distinct (seq, pos) pairs, pos <= 63, neither in token order."""
    r = _rng("pos", T)
    n_slots = (T + N_CTX - 1) // N_CTX + 1
    flat = r.permutation(n_slots * N_CTX)[:T]
    return ((flat % N_CTX).astype(np.int32), (flat // N_CTX).astype(np.int32),
            n_slots)


def qkv_reference(c, xq, xk, xv, tq, tk, tv):
    """Fill c.q_ref / c.k_ref / c.v_ref and their bounds from the
    unrotated float64 products and their NORM-route bounds."""
    c.q_ref = AR.rope_ref(xq, c.pos, c.D)
    c.k_ref = AR.rope_ref(xk, c.pos, c.D)
    c.v_ref = xv
    c.q_tol = tol_rope(tq, xq, c.D, False, c.q_ref)
    c.k_tol = tol_rope(tk, xk, c.D, True, c.k_ref)
    c.v_tol = tv + U16 * np.abs(xv)
    return c


def qkv_inputs(c):
    c.D = c.E // c.H
    c.Ekv = c.Hkv * c.D
    c.rows, c.cols = c.E + 2 * c.Ekv, c.E
    c.x = activations("qkv", c.T, c.E)
    c.nw = norm_weights("qkv", c.E)
    c.pos, c.seq, c.n_slots = qkv_positions(c.T)
    c.n_ctx = N_CTX
    c.inv_freq = AR.inv_freq_f32(c.D)
    c.Kf = np.full(c.n_slots * N_CTX * c.Ekv + 16, POISON, dtype=np.float16)
    c.Vf = np.full(c.n_slots * N_CTX * c.Ekv + 16, -POISON, dtype=np.float16)
    return _finish(c)


@functools.lru_cache(maxsize=None)
def qkv_case(gname, E, H, Hkv, T):
    c = NS(route="qkv", name="qkv-%s-E%d-H%d-Hkv%d-T%d" % (gname, E, H, Hkv,
                                                           T),
           gname=gname, E=E, H=H, Hkv=Hkv, T=T)
    qkv_inputs(c)
    ops = [operand(gname, r, E, tag) for r, tag in
           ((E, "wq"), (c.Ekv, "wk"), (c.Ekv, "wv"))]
    c.ts = [o[0] for o in ops]
    c.mats = [o[1] for o in ops]
    B = panel_norm(c.x, c.nw)
    bmax = np.abs(B).max()
    res = []
    for _, _, A in ops:
        v, s = product(A, B)
        res.append((v, tol_norm(E, s, np.abs(A).max(), bmax)))
    return qkv_reference(c, res[0][0], res[1][0], res[2][0], res[0][1],
                         res[1][1], res[2][1])


# ------------------------------------------------------ the case matrix

DECODE_T = [1, 15, 16, 17, 33, 64]
LARGE_T = [65, 130]


def _type_grid():
    """(gname, cols, decode Ts, large-M Ts): the full T sweep at q4_0,
    T = 17 and T = 70 at every other type."""
    for g in NONK + KQ:
        for cols in ((64, 672) if g in NONK else (256, 768)):
            if g == "q4_0":
                yield g, cols, DECODE_T, LARGE_T
            else:
                yield g, cols, [17], [70]


def residual_cases():
    out = []
    for g, cols, dts, lts in _type_grid():
        for T in dts:
            out += [(g, 48, cols, T, False), (g, 64, cols, T, True),
                    (g, 64, cols, T, False)]
        for T in lts:
            out += [(g, 48, cols, T, False), (g, 64, cols, T, False)]
    # k_gemm16_mt RT = 2
    out.append(("q4_0", 2048, 64, 480, False))
    # cols = 1024 is the smallest width at which all eight split-K slices
    # of a rows = 64 matrix are non-empty (per = 4 blocks): the narrower
    # shapes above leave slice ks-1 empty
    out += [("q4_0", 64, 1024, 17, True), ("f16", 64, 1024, 17, True)]
    return out


def lmhead_cases():
    out = [(g, 512, cols, T) for g, cols, dts, _ in _type_grid()
           for T in dts]
    return out + [("q4_0", 16416, 64, 17), ("q4_0", 28672, 64, 17)]


def ffn_cases():
    out = [(g, 96, cols, T) for g, cols, dts, lts in _type_grid()
           for T in dts + lts]
    return out + [("q4_0", 16384, 64, 17), ("q4_0", 2048, 64, 480)]


def qkv_cases():
    """(gname, E, H, Hkv, T). E = 64 takes the slab route; E = 96 with
    Hkv = 3 has Ekv/16 = 3 odd, which rules RT = 2 out: fused RT = 1 (a
    48-wide model cannot exist: cols % 32 is refused); the k-quants need
    256-wide rows; E = 1024 at T = 17 is the slab route with all eight
    slices live, at T = 330 large-M RT = 2."""
    out = []
    for T in DECODE_T + LARGE_T:
        out += [("q4_0", 64, 4, 4, T), ("q4_0", 64, 4, 2, T),
                ("q4_0", 96, 6, 3, T)]
    for g in NONK[1:]:
        for T in (17, 70):
            out += [(g, 64, 4, 2, T), (g, 96, 6, 3, T)]
    for g in KQ:
        for T in (17, 70):
            out += [(g, 256, 4, 2, T), (g, 256, 4, 1, T)]
    # f16 at 21 K-blocks outside the slab route (Ekv/16 = 21 is odd): the
    # 6 / 6 / 6 / 3 wave ranges, a full batch plus a tail
    out += [("f16", 672, 6, 3, 17), ("f16", 672, 6, 3, 70)]
    return out + [("q4_0", 1024, 8, 8, 17), ("q4_0", 1024, 8, 8, 330)]


BIG_QKV = ("q4_0", 5504, 43, 43, 17)    # fused decode RT = 2, GPU only


# -------------------------------------------------------------- checks
# Every helper returns {check name: worst error / bound}; a relation that
# must hold exactly reports 0 or inf. `check` asserts all of them <= 1.

def _ratio(got, ref, tol):
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - ref) / tol).max())


def _exact(ok):
    return 0.0 if ok else math.inf


def prep_values(prep, rows, T, jtw):
    """Live elements [T, rows] of a side channel, and whether everything
    else (dead columns, K-pad rows, slack) is still zero."""
    prep = np.asarray(prep).view(np.uint16).reshape(-1)
    r, t = np.meshgrid(np.arange(rows), np.arange(T))
    idx = xprep_index(r, t, jtw)
    live = prep[idx]
    rest = prep.copy()
    rest[idx] = 0
    return live, not rest.any()


def residual_ratios(c, got):
    y = np.asarray(got["y"])
    out = {"y": _ratio(y, c.ref, c.tol)}
    prep = np.asarray(got["xprep"])
    out["xprep size"] = _exact(int(got["jtw"]) == c.jtw and
                               prep.size == side_numel(c.rows, c.jtw))
    if out["xprep size"] == 0.0:
        live, clean = prep_values(prep, c.rows, c.T, c.jtw)
        out["xprep == f16(y)"] = _exact(np.array_equal(
            live, y.astype(np.float16).view(np.uint16)))
        out["xprep elsewhere zero"] = _exact(clean)
    ss = np.asarray(got["ss"], dtype=np.float64)
    want = (y.astype(np.float64) ** 2).sum(axis=1)
    out["ss"] = _ratio(ss[:c.T], want, (c.rows + 64) * 2.0 ** -23 * want)
    out["ss elsewhere zero"] = _exact(not ss[c.T:].any())
    return out


def lmhead_ratios(c, got):
    return {"logits": _ratio(got["logits"], c.ref, c.tol)}


def ffn_ratios(c, got):
    prep = np.asarray(got["gprep"])
    ok = int(got["jtw"]) == c.jtw and prep.size == side_numel(c.rows, c.jtw)
    out = {"gprep size": _exact(ok)}
    if ok:
        live, clean = prep_values(prep, c.rows, c.T, c.jtw)
        out["gprep"] = _ratio(live.view(np.float16), c.ref, c.tol)
        out["gprep elsewhere zero"] = _exact(clean)
    return out


def qkv_ratios(c, got):
    out = {"q": _ratio(got["q"], c.q_ref, c.q_tol)}
    for name, flat, ref, tol, fill in (
            ("K", got["k"], c.k_ref, c.k_tol, POISON),
            ("V", got["v"], c.v_ref, c.v_tol, -POISON)):
        flat = np.asarray(flat).view(np.float16)
        st = flat[:-16].reshape(c.n_slots, c.n_ctx, c.Ekv)
        out[name + " rows"] = _ratio(st[c.seq, c.pos], ref, tol)
        rest = st.copy()
        rest[c.seq, c.pos] = fill
        out[name + " elsewhere unchanged"] = _exact(
            (rest == np.float16(fill)).all() and
            (flat[-16:] == np.float16(fill)).all())
    return out


RATIOS = {"residual": residual_ratios, "lmhead": lmhead_ratios,
          "ffn": ffn_ratios, "qkv": qkv_ratios}


def ratios(c, got):
    return RATIOS[c.route](c, got)


def check(c, got):
    r = ratios(c, got)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, "%s: over the bound: %r (all: %r)" % (c.name, bad, r)
    return r


# ----------------------------------------------------------- simulator

def decode_tiles(mat, rows, cols):
    """The simulator's own reading of the tile layouts (mfma_gemm.hip
    header): -> NS(v [rows, nbk, 32] integer weights with the format's
    offset removed, alpha, beta [rows, nbk, 2] per 16-weight half, nb,
    nbk); for f16 v holds the values and alpha = 1, beta = 0."""
    data, sc, wt = mat
    data = data.numpy()
    R, nb = rows // 16, cols // 32
    if wt == RP.W_F16:
        v = (data[:rows * cols].view(np.float16).astype(np.float64)
             .reshape(R, cols // 8, 16, 8).transpose(0, 2, 1, 3)
             .reshape(rows, nb, 32))
        one = np.ones((rows, nb, 2))
        return NS(v=v, alpha=one, beta=0 * one, nb=nb, nbk=nb, wt=wt)
    nbk = (nb + 3) & ~3
    g4 = nbk // 4
    sc = sc.numpy().astype(np.float64)
    if wt == RP.W_Q8B16:
        ab = (sc[:R * nbk * 64].reshape(R, g4, 2, 16, 4, 2)
              .transpose(0, 3, 1, 4, 2, 5).reshape(rows, nbk, 2, 2))
    else:
        ab = (sc[:R * nbk * 32].reshape(R, g4, 16, 4, 2)
              .transpose(0, 2, 1, 3, 4).reshape(rows, nbk, 1, 2))
        ab = np.repeat(ab, 2, axis=2)
    if wt in (RP.W_Q4_0, RP.W_Q4_1):
        qw = data[:R * nbk * 64].view(np.uint32).reshape(R, g4, 4, 16, 4)
        # a_frag_q4: word w holds weights (2w, 2w+1) at bits 4w, 4w + 16
        sh = np.array([(j % 2) * 16 + (j // 2) * 4 for j in range(8)],
                      dtype=np.uint32)
        n = ((qw[..., None] >> sh) & 0xF).astype(np.float64)
        v = n.transpose(0, 3, 1, 4, 2, 5).reshape(rows, nbk, 32)
        if wt == RP.W_Q4_0:
            v = v - 8.0
    else:
        qw = data[:R * nbk * 128].view(np.uint32).reshape(R, g4, 4, 16, 4, 2)
        # a_frag_q8: bytes [w0, w2, w1, w3] of each of the two words
        sh = np.array([0, 16, 8, 24], dtype=np.uint32)
        u = ((qw[..., None] >> sh) & 0xFF).astype(np.float64)
        v = (u.transpose(0, 3, 1, 4, 2, 5, 6).reshape(rows, nbk, 32)
             - 128.0)
    return NS(v=v, alpha=ab[..., 0], beta=ab[..., 1], nb=nb, nbk=nbk, wt=wt)


def a_fragments(dec, mutant=0):
    """f32 [rows, nbk, 32]: one f16 rounding of alpha * v + beta."""
    if dec.wt == RP.W_F16:
        return dec.v.astype(np.float32)
    al, be = dec.alpha.copy(), dec.beta.copy()
    if mutant == 2:
        idx = np.arange(dec.nbk) ^ 1
        al, be = al[:, idx], be[:, idx]
    if mutant == 3:
        al, be = al[:, :, [0, 0]], be[:, :, [0, 0]]
    if mutant == 4:
        be = 0 * be
    if mutant == 5 and dec.nbk > dec.nb:
        al[:, dec.nb:] = al[:, dec.nb - 1:dec.nb]
        be[:, dec.nb:] = be[:, dec.nb - 1:dec.nb]
    w = np.repeat(al, 16, axis=2) * dec.v + np.repeat(be, 16, axis=2)
    return w.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _decoded(gname, rows, cols, tag):
    return decode_tiles(operand(gname, rows, cols, tag)[1], rows, cols)


def b_panel(b16, nbk, pad_fill=0.0):
    """f16 values [T, cols] -> f32 [nbk, 32, T] with the K-pad rows."""
    T, cols = b16.shape
    p = np.full((nbk * 32, T), pad_fill, dtype=np.float32)
    p[:cols] = b16.T
    return p.reshape(nbk, 32, T)


def sim_norm_panel(x, nw, T, mutant=0, eps=EPS):
    """The NORM B-fragment build: f32 sumsq (k_prep_x), rsqrtf, the scale
    rounded to f16, then two f16 multiplies."""
    x16 = x.astype(np.float16)
    ss = (x * x).sum(axis=1, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(x.shape[1])
    sc = (np.float32(1.0) / np.sqrt(ss * inv + np.float32(eps))
          ).astype(np.float16)
    if mutant == 9:
        sc = sc[np.arange(T) % 16]
    v = (x16.astype(np.float64) * f16(nw)[None, :]).astype(np.float16)
    return (v.astype(np.float64) * sc.astype(np.float64)[:, None]
            ).astype(np.float16).astype(np.float64)


def kloop(Af, Bp, b0, b1, align, NP, mutant=0):
    """One block of 4 waves over K-blocks [b0, b1): f32 accumulation in
    the kernel's order, then combine_acc. Af [rows, nbk, 32], Bp
    [nbk, 32, T] -> [rows, T] f32."""
    rows, nbk, _ = Af.shape
    T = Bp.shape[2]
    ranges = [init_range(b0, b1, align, w) for w in range(4)]
    live = [w for w, (a, b) in enumerate(ranges) if b > a]
    parts = []
    for w, (kb0, kb1) in enumerate(ranges):
        c = [np.zeros((rows, T), dtype=np.float32) for _ in range(2)]
        nfull = (kb1 - kb0) // 4
        for g in range(kb0, kb1):
            if mutant == 1 and w == live[-1] and g == kb1 - 1:
                continue
            tail = g >= kb0 + nfull * 4
            par = ((g & 1) if tail else ((g - kb0) & 1)) if NP == 2 else 0
            ga = g
            if mutant == 12 and tail and nfull > 0:
                ga = g + 4         # the weight pointers were not rewound
            if ga < nbk:
                a = Af[:, ga]
            else:                  # runs on into the next row tile / slack
                a = np.zeros((rows, 32), dtype=np.float32)
                a[:rows - 16] = Af[16:, ga - nbk]
            c[par] = c[par] + a @ Bp[g]
        parts.append(c[0] + c[1] if NP == 2 else c[0])
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


def _np_of(nm, jt, rt):
    return 1 if nm * jt * rt >= 4 else 2


def _align(gname):
    return 1 if gname == "f16" else 4


def _slices(nbk, ks):
    per = ((nbk + ks - 1) // ks + 3) & ~3
    return [(min(nbk, k * per), min(nbk, min(nbk, k * per) + per))
            for k in range(ks)]


def _mask(acc, T, mutant):
    """-> the live token columns (all but T-1 under mutant 6)."""
    return T - 1 if mutant == 6 else T


def _side(values, rows, T, jtw, live_T, mutant=0):
    """u16 side channel the epilogue writes for values [T, rows] f32."""
    prep = np.zeros(side_numel(rows, jtw), dtype=np.uint16)
    r, t = np.meshgrid(np.arange(rows), np.arange(live_T))
    stride = 4 if mutant == 11 and T > 64 else jtw
    prep[xprep_index(r, t, stride)] = (
        values[:live_T].astype(np.float16).view(np.uint16))
    return prep


def sim_residual(c, mutant=0, pad_fill=0.0):
    dec = _decoded(c.gname, c.rows, c.cols, "res")
    Af = a_fragments(dec, mutant)
    Bp = b_panel(panel_plain(c.b), dec.nbk, pad_fill)
    T, rows = c.T, c.rows
    jt = 4 if T > 64 else pick_jt(T)
    y = c.y_in.copy()
    live = _mask(None, T, mutant)
    if c.split:
        ks = gemm16_ks(rows)
        NP = _np_of(1, jt, 2)
        slabs = [kloop(Af, Bp, b0, b1, _align(c.gname), NP, mutant)
                 for b0, b1 in _slices(dec.nbk, ks)]
        v = np.zeros_like(y) if mutant == 8 else y.copy()
        for s in slabs[:ks - 1 if mutant == 7 else ks]:
            v = v + s.T
    else:
        rt = gemm16_mt_rt(rows, T) if T > 64 else 1
        acc = kloop(Af, Bp, 0, dec.nbk, _align(c.gname), _np_of(1, jt, rt),
                    mutant)
        v = acc.T if mutant == 8 else acc.T + y
    y[:live] = v[:live]
    ss = np.zeros((T + 63) & ~63, dtype=np.float32)
    ss[:live] = (v[:live] * v[:live]).sum(axis=1, dtype=np.float32)
    return {"y": y, "xprep": _side(v, rows, T, c.jtw, live, mutant),
            "ss": ss, "jtw": c.jtw}


def sim_lmhead(c, mutant=0, pad_fill=0.0):
    dec = _decoded(c.gname, c.rows, c.cols, "lm")
    Bp = b_panel(sim_norm_panel(c.x, c.nw, c.T, mutant), dec.nbk, pad_fill)
    NP = _np_of(1, pick_jt(c.T), gemm16_plain_rt(c.rows))
    acc = kloop(a_fragments(dec, mutant), Bp, 0, dec.nbk, _align(c.gname),
                NP, mutant)
    lg = np.zeros((c.T, c.rows), dtype=np.float32)
    live = _mask(None, c.T, mutant)
    lg[:live] = acc.T[:live]
    return {"logits": lg}


def sim_ffn(c, mutant=0, pad_fill=0.0):
    d1 = _decoded(c.gname, c.rows, c.cols, "w1")
    d3 = _decoded(c.gname, c.rows, c.cols, "w3")
    Bp = b_panel(sim_norm_panel(c.x, c.nw, c.T, mutant), d1.nbk, pad_fill)
    jt = 4 if c.T > 64 else pick_jt(c.T)
    NP = _np_of(2, jt, ffn16_rt(c.rows, c.T))
    v1, v3 = [kloop(a_fragments(d, mutant), Bp, 0, d.nbk, _align(c.gname),
                    NP, mutant).T for d in (d1, d3)]
    if mutant == 10:
        v1, v3 = v3, v1
    g = (v1 / (np.float32(1.0) + np.exp(-v1))) * v3
    return {"gprep": _side(g.astype(np.float32), c.rows, c.T, c.jtw,
                           _mask(None, c.T, mutant), mutant),
            "jtw": c.jtw}


def _sim_rope(v, pos, inv_freq, D):
    """rope_rotate in f32 with f32 theta and sin/cos rounded to f32."""
    T, n = v.shape
    d = (np.arange(n) % D) >> 1
    theta = pos.astype(np.float32)[:, None] * inv_freq[d][None, :]
    sn = np.sin(theta.astype(np.float64)).astype(np.float32)
    cs = np.cos(theta.astype(np.float64)).astype(np.float32)
    out = np.empty_like(v)
    x0, x1 = v[:, 0::2], v[:, 1::2]
    out[:, 0::2] = x0 * cs[:, 0::2] - x1 * sn[:, 0::2]
    out[:, 1::2] = x0 * sn[:, 0::2] + x1 * cs[:, 0::2]
    return out


def sim_qkv(c, mutant=0, pad_fill=0.0):
    T, E, Ekv = c.T, c.E, c.Ekv
    decs = [_decoded(c.gname, r, E, tag) for r, tag in
            ((E, "wq"), (Ekv, "wk"), (Ekv, "wv"))]
    Bp = b_panel(sim_norm_panel(c.x, c.nw, T, mutant), decs[0].nbk, pad_fill)
    al = _align(c.gname)
    route = qkv16_route(E, Ekv, T, True) if T <= 64 else None
    vals = []
    for dec in decs:
        Af = a_fragments(dec, mutant)
        if route == 0:
            ks = AR.qkv16_ks_ref(E, Ekv)
            NP = _np_of(1, pick_jt(T), 2)
            v = np.zeros((T, dec.v.shape[0]), dtype=np.float32)
            sl = _slices(dec.nbk, ks)
            for b0, b1 in sl[:ks - 1 if mutant == 7 else ks]:
                v = v + kloop(Af, Bp, b0, b1, al, NP, mutant).T
        else:
            rt = qkv16_mt_rt(E, Ekv, T) if T > 64 else route
            jt = 4 if T > 64 else pick_jt(T)
            v = kloop(Af, Bp, 0, dec.nbk, al, _np_of(1, jt, rt), mutant).T
        vals.append(v)
    live = _mask(None, T, mutant)
    q = np.zeros((T, E), dtype=np.float32)
    q[:live] = _sim_rope(vals[0], c.pos, c.inv_freq, c.D)[:live]
    k, v = c.Kf.copy(), c.Vf.copy()
    ks_, vs_ = (a[:-16].reshape(c.n_slots, c.n_ctx, Ekv) for a in (k, v))
    ks_[c.seq[:live], c.pos[:live]] = _sim_rope(
        vals[1], c.pos, c.inv_freq, c.D)[:live].astype(np.float16)
    vs_[c.seq[:live], c.pos[:live]] = vals[2][:live].astype(np.float16)
    return {"q": q, "k": k, "v": v}


SIMS = {"residual": sim_residual, "lmhead": sim_lmhead, "ffn": sim_ffn,
        "qkv": sim_qkv}


def simulate(c, mutant=0, pad_fill=0.0):
    return SIMS[c.route](c, mutant, pad_fill)


def wave_ranges(c):
    """[(b0, b1) of every kernel block's K range] of a case, nbk, nb."""
    nb = c.cols // 32
    nbk = nb if c.gname == "f16" else (nb + 3) & ~3
    if c.route == "residual" and c.split:
        return _slices(nbk, gemm16_ks(c.rows)), nbk, nb
    if (c.route == "qkv" and c.T <= 64 and
            qkv16_route(c.E, c.Ekv, c.T, True) == 0):
        return _slices(nbk, AR.qkv16_ks_ref(c.E, c.Ekv)), nbk, nb
    return [(0, nbk)], nbk, nb


def mutant_applies(c, m):
    """Whether mutant m changes arithmetic on live data of case c (a
    mutant that only moves exact zeros cannot be seen by any test)."""
    sl, nbk, nb = wave_ranges(c)
    al = _align(c.gname)
    norm = c.route != "residual"
    if m == 1:      # the dropped block must be a real one
        for b0, b1 in sl:
            rs = [init_range(b0, b1, al, w) for w in range(4)]
            rs = [r for r in rs if r[1] > r[0]]
            if rs and rs[-1][1] - 1 < nb:
                return True
        return False
    if m == 2:
        return c.gname != "f16"
    if m == 3:
        return c.gname in ("q2_K", "q6_K")
    if m == 4:
        return c.gname in ("q4_1", "q5_1", "q4_K", "q2_K")
    if m == 5:
        return nbk > nb
    if m == 6:
        return True
    if m == 7:      # the last slice must hold real blocks
        return len(sl) > 1 and sl[-1][1] > sl[-1][0] and sl[-1][0] < nb
    if m == 8:
        return c.route == "residual"
    if m == 9:
        return norm and c.T > 16
    if m == 10:
        return c.route == "ffn"
    if m == 11:
        return c.route in ("residual", "ffn") and c.T > 64
    if m == 12:
        if c.gname != "f16":
            return False
        for b0, b1 in sl:
            for w in range(4):
                k0, k1 = init_range(b0, b1, 1, w)
                if k1 - k0 >= 4 and (k1 - k0) % 4:
                    return True
        return False
    raise KeyError(m)


def make_case(route, args):
    return {"residual": residual_case, "lmhead": lmhead_case,
            "ffn": ffn_case, "qkv": qkv_case}[route](*args)


def all_cases():
    return ([("residual", a) for a in residual_cases()] +
            [("lmhead", a) for a in lmhead_cases()] +
            [("ffn", a) for a in ffn_cases()] +
            [("qkv", a) for a in qkv_cases()])
