"""Float64 reference for the attention kernels and RoPE, the inputs of the
direct kernel tests, and the assertion helpers both test files share.

Plain numpy, no GPU. tests/test_gpu_attention.py and test_gpu_kv_writes.py
feed device results into the `check_*` helpers below;
tests/test_attention_reference.py feeds the *mutant* references through the
very same helpers and inputs and demands that each one is rejected - that
is what shows the GPU tests would notice a subtly wrong kernel.

Cache layout (engine_ext.cpp): one layer's K or V store is a flat f16 array
of n_slots * n_ctx * Ekv + 16 halves, the last 16 a mandatory pad; `stores`
returns the flat array and its [n_slots, n_ctx, Ekv] view.

Tolerances (derived, see docs/kernels.md "Direct kernel tests"), with
S_abs = max over attended rows of sum_d |q_d k_d| / sqrt(D):

    decode   4 * ((D + 2) * 2**-24 * S_abs + 2**-20) * max|V|
    prefill  4 * 2**-11 * (S_abs + 1) * max|V|
    uniform  1e-5 * max|V|                      (q = 0: every p is 1)
"""
import functools
import math
import zlib

import numpy as np

ROPE_BASE = 10000.0
ROPE_DOMAIN = 512 * math.pi     # |theta| the ISA manuals call valid

# the mutant references; 1-6 attention, 7-8 RoPE
MUTANTS = {
    1: "drop row J-1",
    2: "drop row 0",
    3: "also attend row J",
    4: "count the last row of a 4-row group twice",
    5: "kv head = h % Hkv",
    6: "no rescale of the output when the running max rises",
    7: "RoPE sin=0, cos=1 for |theta| > 512 pi",
    8: "RoPE pairs (d, d + D/2)",
}


# ----------------------------------------------------------- references

def _attend(q, K, V, pos, seq, H, Hkv, mutant=None):
    """-> (out [T, E] f64, S_abs, max|V| over the attended rows).
    q [T, E]; K, V [n_slots, n_ctx, Ekv]."""
    q = np.asarray(q, dtype=np.float64)
    T, E = q.shape
    D = E // H
    grp = H // Hkv
    hk = np.arange(H) % Hkv if mutant == 5 else np.arange(H) // grp
    out = np.zeros((T, E))
    sabs, vmax = 0.0, 0.0
    for t in range(T):
        J = int(pos[t]) + 1
        lo, hi = 0, J
        if mutant == 1:
            hi = J - 1
        elif mutant == 2:
            lo = 1
        elif mutant == 3:
            hi = min(J + 1, K.shape[1])
        if hi <= lo:
            continue
        k = K[int(seq[t]), lo:hi].astype(np.float64).reshape(-1, Hkv, D)
        v = V[int(seq[t]), lo:hi].astype(np.float64).reshape(-1, Hkv, D)
        k, v = k[:, hk], v[:, hk]                      # [J, H, D]
        qt = q[t].reshape(H, D)
        s = np.einsum("hd,jhd->hj", qt, k) / math.sqrt(D)
        if mutant is None:
            sabs = max(sabs, float(
                np.einsum("hd,jhd->hj", np.abs(qt), np.abs(k)).max()
                / math.sqrt(D)))
            vmax = max(vmax, float(np.abs(v).max()))
        m = s.max(axis=1, keepdims=True)
        p = np.exp(s - m)                              # [H, J]
        l = p.sum(axis=1)
        if mutant == 4:
            w = np.where((np.arange(lo, hi) % 4 == 3), 2.0, 1.0)
            p = p * w
            l = p.sum(axis=1)
        elif mutant == 6:
            # row j enters with the running max of its time and is
            # never rescaled afterwards; l is kept right
            p = np.exp(s - np.maximum.accumulate(s, axis=1))
        out[t] = (np.einsum("hj,jhd->hd", p, v) / l[:, None]).reshape(E)
    return out, sabs, vmax


def attention_ref(q, K, V, pos, seq, H, Hkv, mutant=None):
    """Token t attends over rows [0, pos[t]] of slot seq[t]; kv head is
    h // (H // Hkv); scores q.k / sqrt(D). float64 throughout."""
    return _attend(q, K, V, pos, seq, H, Hkv, mutant)[0]


def rope_ref(x, pos, D, base=ROPE_BASE, mutant=None):
    """Rotate adjacent pairs (x[2i], x[2i+1]) of every D-wide head of
    x [T, n*D] by theta = pos * base**(-2i/D), in float64."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    xh = x.reshape(T, -1, D)
    half = D // 2
    theta = (np.asarray(pos, dtype=np.float64)[:, None] *
             base ** (-2.0 * np.arange(half) / D)[None, :])   # [T, half]
    sn, cs = np.sin(theta), np.cos(theta)
    if mutant == 7:
        lost = np.abs(theta) > ROPE_DOMAIN
        sn, cs = np.where(lost, 0.0, sn), np.where(lost, 1.0, cs)
    sn, cs = sn[:, None, :], cs[:, None, :]
    out = np.empty_like(xh)
    if mutant == 8:
        x0, x1 = xh[..., :half], xh[..., half:]
        out[..., :half] = x0 * cs - x1 * sn
        out[..., half:] = x0 * sn + x1 * cs
    else:
        x0, x1 = xh[..., 0::2], xh[..., 1::2]
        out[..., 0::2] = x0 * cs - x1 * sn
        out[..., 1::2] = x0 * sn + x1 * cs
    return out.reshape(x.shape)


def inv_freq_f32(D, base=ROPE_BASE):
    return (base ** (-2.0 * np.arange(D // 2) / D)).astype(np.float32)


def xprep_index(e, t, jtw):
    """device_common.h: element e of token t lives at
    [e/8][t/16 of jtw token tiles][t%16][e%8]."""
    return (((e >> 3) * jtw + (t >> 4)) * 16 + (t & 15)) * 8 + (e & 7)


def make_prep(out, jtw):
    """The side channel a correct kernel leaves for `out` [T, E] f32:
    u16 flat [(E/8) * jtw * 128], zero wherever no (t, e) lands."""
    T, E = out.shape
    prep = np.zeros((E // 8) * jtw * 128, dtype=np.uint16)
    e, t = np.meshgrid(np.arange(E), np.arange(T))
    prep[xprep_index(e, t, jtw)] = out.astype(np.float16).view(np.uint16)
    return prep


def jt_width_ref(T):
    """mfma_gemm.hip jt_width, restated only for the CPU tests (the GPU
    tests take jtw from the extension)."""
    if T <= 64:
        return 1 if T <= 16 else 2 if T <= 32 else 4
    return (((T + 15) >> 4) + 3) & ~3


def qkv16_ks_ref(E, Ekv):
    """mfma_gemm.hip qkv16_ks, restated only for the CPU tests."""
    ks = 1
    while (((E + 2 * Ekv) >> 4) // 2) * ks < 512 and ks < 8:
        ks <<= 1
    return ks


# --------------------------------------------------------- input builders

def stores(n_slots, n_ctx, Ekv):
    """-> (flat f16 [n_slots*n_ctx*Ekv + 16], its [n_slots, n_ctx, Ekv]
    view)."""
    flat = np.zeros(n_slots * n_ctx * Ekv + 16, dtype=np.float16)
    return flat, flat[:-16].reshape(n_slots, n_ctx, Ekv)


def poison(K, V, pos, seq):
    """Fill every row above pos (per slot: above the largest pos of its
    tokens; pos = -1 poisons the whole slot), every unused slot and the
    16-half pad with large FINITE values, K = +30000, V = -30000. Never
    NaN/Inf: the kernels' contract is that unread or masked cache memory
    is finite (masked rows are multiplied by 0). K, V are the views
    returned by `stores`."""
    top = np.full(K.shape[0], -1, dtype=np.int64)
    for p, s in zip(pos, seq):
        top[int(s)] = max(top[int(s)], int(p))
    for a, val in ((K, 30000.0), (V, -30000.0)):
        flat = a.base
        assert flat is not None and flat.size == a.size + 16
        for s in range(a.shape[0]):
            a[s, top[s] + 1:] = val
        flat[-16:] = val


def build_qkv_slab(q, k, v, ks, rng):
    """Split-K partials whose sum is (about) q [T, E], k, v [T, Ekv], in
    the layout k_attention<true> reads: f32[(E + 2 Ekv)/16][ks][64][16],
    q rows, then k rows, then v rows. Returns (slab flat f32, qsum, ksum,
    vsum): the sums are the partials' sequential f32 sums over
    c = 0..ks-1 starting from 0.f, exactly as the kernel prologue adds
    them, so they are the bit-exact pre-RoPE values. Token columns
    T..63 hold random values no launch may read."""
    T, E = q.shape
    Ekv = k.shape[1]
    rows = np.concatenate([q, k, v], axis=1).astype(np.float32)  # [T, R]
    R = E + 2 * Ekv
    part = rng.standard_normal((ks, 64, R)).astype(np.float32)
    if ks > 1:
        part[ks - 1, :T] = rows - part[:ks - 1, :T].sum(axis=0,
                                                        dtype=np.float32)
    else:
        part[0, :T] = rows
    acc = np.zeros((T, R), dtype=np.float32)
    for c in range(ks):
        acc = (acc + part[c, :T]).astype(np.float32)
    slab = np.ascontiguousarray(
        part.reshape(ks, 64, R // 16, 16).transpose(2, 0, 1, 3))
    return (slab.reshape(-1), acc[:, :E].copy(), acc[:, E:E + Ekv].copy(),
            acc[:, E + Ekv:].copy())


# ------------------------------------------------------------- tolerances

def tol_decode(D, sabs, vmax):
    return 4 * ((D + 2) * 2.0 ** -24 * sabs + 2.0 ** -20) * vmax


def tol_prefill(sabs, vmax):
    return 4 * 2.0 ** -11 * (sabs + 1) * vmax


def tol_uniform(vmax):
    return 1e-5 * vmax


ROPE_ANGLE = 1e-3       # angle budget (rad) at pos <= 4095, see kv tests


def tol_kv_rows(ref, pos, is_k):
    """Per-row bound of the engine-level cache check: V 3*2**-11 *
    rowmax, K that plus the 1e-3 angle budget at pos > 0."""
    rowmax = np.abs(ref).max(axis=1)
    c = 3 * 2.0 ** -11
    if is_k:
        c = c + ROPE_ANGLE * (np.asarray(pos) > 0)
    return c * rowmax


# ------------------------------------------------------------------ cases

SHAPES = [(16, 4, 4), (16, 8, 2), (24, 4, 4), (24, 8, 2), (64, 4, 4),
          (64, 8, 2), (100, 4, 4), (100, 8, 4), (128, 4, 4), (128, 8, 2)]
SWEEP_J = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127,
           128, 129, 255, 256, 257]
PREFILL_T = [1, 15, 16, 17, 40, 100]
DECODE_KINDS = ["sweep", "uniform", "triangle", "triangle_shuffled",
                "peaky"]
PREFILL_KINDS = (["span0_T%d" % t for t in PREFILL_T] +
                 ["span37_T%d" % t for t in PREFILL_T] +
                 ["edges", "mixed", "uniform_span", "uniform_mixed"])
FUSED_POS = [0, 1, 31, 32, 1607, 1609, 2047, 4095]
# T = 8 holds every position of FUSED_POS once, at every shape; T = 64
# needs 64 slots of 4096 rows: only at the narrowest kv widths
FUSED_CASES = ([(s, T) for s in SHAPES for T in (1, 5, 8)] +
               [((16, 4, 4), 64), ((16, 8, 2), 64), ((24, 8, 2), 64)])


def _seed(*key):
    return zlib.crc32(repr(key).encode())


class Case(dict):
    __getattr__ = dict.__getitem__


def _finish(name, tolkind, D, H, Hkv, n_ctx, n_slots, q, Kf, K, Vf, V,
            pos, seq, filled):
    """Poison everything above `filled` rows, attach reference + tol."""
    pos = np.asarray(pos, dtype=np.int32)
    seq = np.asarray(seq, dtype=np.int32)
    poison(K, V, filled, seq)
    ref, sabs, vmax = _attend(q, K, V, pos, seq, H, Hkv)
    tol = {"decode": tol_decode(D, sabs, vmax),
           "prefill": tol_prefill(sabs, vmax),
           "uniform": tol_uniform(vmax)}[tolkind]
    return Case(name=name, D=D, H=H, Hkv=Hkv, n_ctx=n_ctx, n_slots=n_slots,
                q=np.ascontiguousarray(q, dtype=np.float32), Kf=Kf, K=K,
                Vf=Vf, V=V, pos=pos, seq=seq, ref=ref, sabs=sabs,
                vmax=vmax, tol=tol, tolkind=tolkind)


def _random_kv(rng, n_slots, n_ctx, Ekv, uniform=False):
    Kf, K = stores(n_slots, n_ctx, Ekv)
    Vf, V = stores(n_slots, n_ctx, Ekv)
    K[:] = rng.standard_normal(K.shape)
    if uniform:
        V[:] = (rng.uniform(0.5, 1.0, V.shape) *
                rng.choice([-1.0, 1.0], V.shape))
    else:
        V[:] = rng.standard_normal(V.shape)
    return Kf, K, Vf, V


@functools.lru_cache(maxsize=None)
def decode_case(kind, D, H, Hkv):
    rng = np.random.default_rng(_seed("decode", kind, D, H, Hkv))
    E, Ekv = H * D, Hkv * D
    uniform = kind == "uniform"
    if kind in ("sweep", "uniform"):
        n_ctx, n_slots, T = 272, 26, len(SWEEP_J)
        pos = np.array(SWEEP_J) - 1
        seq = rng.permutation(n_slots)[:T]
        assert (seq != np.arange(T)).any()
    elif kind in ("triangle", "triangle_shuffled"):
        # the <= 64-token prefill shape that also runs on k_attention
        n_ctx, n_slots, T = 40, 3, 33
        pos = np.arange(T)
        if kind == "triangle_shuffled":
            pos = rng.permutation(T)
            assert (pos != np.arange(T)).any()
        seq = np.full(T, 1)
    elif kind == "peaky":
        n_ctx, n_slots, T = 272, 5, 4
        pos = np.array([33, 33, 257, 257]) - 1
        seq = np.array([3, 0, 4, 1])
    elif kind == "last_row":
        # seq = n_slots-1, pos = n_ctx-1: the last kv head's last octet
        # (D = 100) reads into the pad - inside the allocation
        n_ctx, n_slots, T = 48, 3, 1
        pos, seq = np.array([n_ctx - 1]), np.array([n_slots - 1])
    else:
        assert kind == "deep"
        n_ctx, n_slots, T = 4096, 4, 4
        pos, seq = np.array([4094, 4095, 2047, 1609]), np.array([2, 0, 3, 1])
    Kf, K, Vf, V = _random_kv(rng, n_slots, n_ctx, Ekv, uniform)
    q = rng.standard_normal((T, E)).astype(np.float32)
    if uniform:
        q[:] = 0.0
    if kind == "peaky":
        # scores run -60 .. +60 along j: ascending (the max rises on
        # every iteration; tokens 0, 2) or descending (fixed after the
        # first row; tokens 1, 3)
        hk = np.arange(H) // (H // Hkv)
        u = rng.standard_normal((Hkv, D))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        for t in range(T):
            J = int(pos[t]) + 1
            a = np.linspace(-1.0, 1.0, J)
            if t % 2:
                a = a[::-1]
            rows = (a[:, None, None] * u[None] +
                    0.01 * rng.standard_normal((J, Hkv, D)))
            K[seq[t], :J] = rows.reshape(J, Ekv)
            q[t] = (60.0 * math.sqrt(D) * u[hk]).reshape(E)
    return _finish("decode/%s/D%d_H%d_%d" % (kind, D, H, Hkv), "uniform"
                   if uniform else "decode", D, H, Hkv, n_ctx, n_slots, q,
                   Kf, K, Vf, V, pos, seq, pos)


@functools.lru_cache(maxsize=None)
def prefill_case(kind, D, H, Hkv):
    rng = np.random.default_rng(_seed("prefill", kind, D, H, Hkv))
    E, Ekv = H * D, Hkv * D
    uniform = kind.startswith("uniform")
    if kind.startswith("span") or kind == "uniform_span":
        # one span at offset 0, or a continuation over 37 earlier rows
        off, T = ((37, 40) if uniform else
                  (int(kind[4:kind.index("_")]), int(kind.split("T")[1])))
        n_ctx, n_slots = 144, 3
        pos, seq = off + np.arange(T), np.full(T, 1)
    elif kind == "edges":
        # four 16-query tiles, each its own sequence, whose jmax + 1 is
        # 63, 64, 65 (the 64-row pass of 4 waves) and 129
        n_ctx, n_slots = 144, 5
        pos = np.concatenate([o + np.arange(16) for o in (47, 48, 49, 113)])
        seq = np.repeat([2, 0, 3, 1], 16)
    else:
        assert kind in ("mixed", "uniform_mixed")
        # segments of 1..7 tokens of 3 sequences: boundaries fall inside
        # the 16-query tiles, pos restarts per segment and is not
        # monotone within one
        n_ctx, n_slots = 32, 4
        pos, seq, last = [], [], -1
        while len(pos) < 40:
            s = int(rng.choice([x for x in range(3) if x != last]))
            n = int(rng.integers(1, 8))
            pos += [int(p) for p in rng.integers(0, 30, n)]
            seq += [s] * n
            last = s
        pos, seq = np.array(pos[:40]), np.array(seq[:40])
    T = len(pos)
    Kf, K, Vf, V = _random_kv(rng, n_slots, n_ctx, Ekv, uniform)
    q = rng.standard_normal((T, E)).astype(np.float32)
    if uniform:
        q[:] = 0.0
    return _finish("prefill/%s/D%d_H%d_%d" % (kind, D, H, Hkv), "uniform"
                   if uniform else "prefill", D, H, Hkv, n_ctx, n_slots, q,
                   Kf, K, Vf, V, pos, seq, pos)


@functools.lru_cache(maxsize=2)
def fused_case(D, H, Hkv, T, ks):
    """k_attention<true>: slabs in, row pos[t] of slot seq[t] appended.
    Rows [0, pos) are pre-filled, everything else poisoned (the row to be
    appended included)."""
    rng = np.random.default_rng(_seed("fused", D, H, Hkv, T))
    E, Ekv = H * D, Hkv * D
    n_ctx, n_slots = 4096, T + 1
    pos = np.array([FUSED_POS[(t * 5 + 7) % 8] if T > 1 else 1609
                    for t in range(T)], dtype=np.int32)
    if T >= 8:
        assert set(pos.tolist()) == set(FUSED_POS)
    seq = rng.permutation(n_slots)[:T].astype(np.int32)
    Kf, K = stores(n_slots, n_ctx, Ekv)
    Vf, V = stores(n_slots, n_ctx, Ekv)
    for t in range(T):
        K[seq[t], :pos[t]] = rng.standard_normal((pos[t], Ekv))
        V[seq[t], :pos[t]] = rng.standard_normal((pos[t], Ekv))
    poison(K, V, pos - 1, seq)
    slab, qs, ksum, vs = build_qkv_slab(
        rng.standard_normal((T, E)), rng.standard_normal((T, Ekv)),
        rng.standard_normal((T, Ekv)), ks, rng)
    return Case(name="fused/D%d_H%d_%d_T%d" % (D, H, Hkv, T), D=D, H=H,
                Hkv=Hkv, n_ctx=n_ctx, n_slots=n_slots, T=T, ks=ks,
                slab=slab, qsum=qs, ksum=ksum, vsum=vs, Kf=Kf, K=K, Vf=Vf,
                V=V, pos=pos, seq=seq, inv_freq=inv_freq_f32(D))


# ------------------------------------------------------ assertion helpers

def check_attention(case, out, prep, jtw, ref=None, tol=None):
    """Device (or mutant) result of one launch against the case's
    reference: `out` [T, E] f32 within the case's tolerance, and the
    side channel `prep` (u16 flat) bit-equal to f16(out) at
    xprep_index(e, t, jtw), zero everywhere else. Returns worst
    error / tol; raises AssertionError."""
    ref = case.ref if ref is None else ref
    tol = case.tol if tol is None else tol
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert np.isfinite(out).all(), case.name + ": non-finite output"
    ratio = float((np.abs(out.astype(np.float64) - ref) / tol).max())
    print("%s: worst error / tol = %.3g" % (case.name, ratio))
    assert ratio <= 1.0, "%s: error %.3g x the bound" % (case.name, ratio)
    prep = np.asarray(prep).view(np.uint16).reshape(-1)
    want = make_prep(out, jtw)
    assert prep.size >= want.size
    assert np.array_equal(prep[:want.size], want), \
        case.name + ": side channel differs from f16(out)"
    assert not prep[want.size:].any()
    return ratio


def fused_expected(case, mutant=None):
    """What a correct (or mutant) k_attention<true> leaves behind:
    (K flat after, V flat after, rotated q [T, E] f64, K row refs f64)."""
    Kf, Vf = case.Kf.copy(), case.Vf.copy()
    K = Kf[:-16].reshape(case.K.shape)
    V = Vf[:-16].reshape(case.V.shape)
    krow = rope_ref(case.ksum, case.pos, case.D, mutant=mutant)
    for t in range(case.T):
        K[case.seq[t], case.pos[t]] = krow[t]
        V[case.seq[t], case.pos[t]] = case.vsum[t]   # RN f16, bit-exact
    return Kf, Vf, rope_ref(case.qsum, case.pos, case.D,
                            mutant=mutant), krow


def simulate_fused(case, mutant=None):
    """(out, prep, jtw, K after, V after) of a device that computes the
    float64 (mutant) reference - stands in for the GPU on the CPU."""
    Kf, Vf, qrot, _ = fused_expected(case, mutant)
    K = Kf[:-16].reshape(case.K.shape)
    V = Vf[:-16].reshape(case.V.shape)
    out = attention_ref(qrot, K, V, case.pos, case.seq, case.H, case.Hkv,
                        mutant=mutant).astype(np.float32)
    jtw = jt_width_ref(case.T)
    return out, make_prep(out, jtw), jtw, Kf, Vf


def fused_out_ratios(case, out, Ka, Va):
    """Per-token worst |out - ref| / tol of a fused launch, with ref =
    attention_ref on the caches as read back (views Ka, Va) and on
    rope_ref of the slab's q sums, and tol the decode bound of the case.
    -> (ratios [T], ref, tol)."""
    qrot = rope_ref(case.qsum, case.pos, case.D)
    ref, sabs, vmax = _attend(qrot, Ka, Va, case.pos, case.seq, case.H,
                              case.Hkv)
    tol = tol_decode(case.D, sabs, vmax)
    err = np.abs(np.asarray(out, dtype=np.float64) - ref).max(axis=1) / tol
    return err, ref, tol


def check_fused(case, out, prep, jtw, k_after, v_after):
    """Fused decode: the appended V row is bit-exact f16 of the slab
    sum; the appended K row is rope_ref of the slab sum within the RoPE
    row tolerance; no other cache element changed (whole-tensor
    compare); `out` matches attention_ref on the cache as read back and
    rope_ref(q).

    `out` is held to the plain decode bound of the case: the kernel
    rotates q itself, so the angle error of that rotation (measured
    3.2e-4 rad at theta = 4095, see check_angle) is part of the error
    and has to fit inside it. Returns (worst K-row ratio, worst out
    ratio)."""
    k_after = np.asarray(k_after).view(np.float16).reshape(-1)
    v_after = np.asarray(v_after).view(np.float16).reshape(-1)
    Kexp, Vexp, qrot, krow = fused_expected(case)
    assert np.array_equal(v_after.view(np.uint16), Vexp.view(np.uint16)), \
        case.name + ": V store differs (appended row must be bit-exact " \
        "f16 of the f32 slab sum, nothing else may change)"
    Ka = k_after[:-16].reshape(case.K.shape)
    got = np.stack([Ka[case.seq[t], case.pos[t]]
                    for t in range(case.T)]).astype(np.float64)
    assert np.isfinite(got).all()
    rowtol = tol_kv_rows(krow, case.pos, True)
    kratio = float((np.abs(got - krow).max(axis=1) / rowtol).max())
    print("%s: worst K row error / tol = %.3g" % (case.name, kratio))
    assert kratio <= 1.0, "%s: K row error %.3g x the bound" % (
        case.name, kratio)
    # everything but the appended rows is unchanged
    patched = Kexp.copy()
    Kp = patched[:-16].reshape(case.K.shape)
    for t in range(case.T):
        Kp[case.seq[t], case.pos[t]] = Ka[case.seq[t], case.pos[t]]
    assert np.array_equal(k_after.view(np.uint16),
                          patched.view(np.uint16)), \
        case.name + ": K store changed outside the appended rows"
    Va = v_after[:-16].reshape(case.V.shape)
    err, ref, tol = fused_out_ratios(case, out, Ka, Va)
    print("%s: out error / tol per pos %s" % (case.name, " ".join(
        "%d:%.3g" % (p, err[case.pos == p].max())
        for p in sorted(set(case.pos.tolist())))))
    ratio = check_attention(case, out, prep, jtw, ref=ref, tol=tol)
    return kratio, ratio


def check_kv_rows(name, k_got, v_got, k_ref, v_ref, pos):
    """Engine-level cache rows [n, Ekv] at `pos` against the float
    reference rows, per-row bounds of tol_kv_rows. Returns the worst
    (K, V) ratios."""
    res = []
    for tag, got, ref, is_k in (("K", k_got, k_ref, True),
                                ("V", v_got, v_ref, False)):
        got = np.asarray(got, dtype=np.float64)
        ref = np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape and np.isfinite(got).all()
        ratio = np.abs(got - ref).max(axis=1) / tol_kv_rows(ref, pos, is_k)
        w = int(ratio.argmax())
        print("%s %s rows: worst error / tol = %.3g (pos %d); at pos %s: %s"
              % (name, tag, ratio[w], pos[w], list(map(int, pos[:8])),
                 " ".join("%.3g" % r for r in ratio[:8])))
        res.append(float(ratio.max()))
    assert res[0] <= 1.0, "%s: K row error %.3g x the bound" % (name, res[0])
    assert res[1] <= 1.0, "%s: V row error %.3g x the bound" % (name, res[1])
    return tuple(res)


# -------------------------------------------- engine-level KV-write cases

KV_POS = [0, 1, 511, 1607, 1609, 2047, 3000, 4095]
KV_PRODUCERS = ["k_qkv_finish", "k_attention_fused", "k_qkv16_unsplit",
                "k_qkv16_large_m", "legacy_f32"]


def kv_case(producer):
    """One forward whose layer-0 cache rows come from `producer` (one
    layer is built: layer 0 depends only on the input). Decode shapes
    put every token in its own sequence; prefill shapes use one sequence
    and a position list that contains KV_POS."""
    from distributedllm_amd.formats import ggml, synthetic
    from distributedllm_amd.models.llama import LlamaPreset
    preset, ftype, decode, T = {
        # slab path + separate finish pass: tiny, T <= 64, decode=False
        "k_qkv_finish": ("tiny", ggml.FTYPE_MOSTLY_Q4_0, False, 8),
        # slab path, finish fused into the attention prologue
        "k_attention_fused": ("tiny", ggml.FTYPE_MOSTLY_Q4_0, True, 8),
        # Ekv = 16 * odd makes launch_qkv16's rt2_ok false, so neither
        # the slab path nor RT = 2 runs. (The RT = 2 instantiation of
        # k_qkv16 needs E + 2 Ekv >= 16384, out of reach at test size;
        # it shares the epilogue source with this unsplit one.)
        "k_qkv16_unsplit": (LlamaPreset("kv_unsplit", 256, 128, 32, 8, 1,
                                        n_head_kv=1),
                            ggml.FTYPE_MOSTLY_Q4_0, False, 8),
        # T > 64: k_qkv16<…, true> (large-M)
        "k_qkv16_large_m": ("small", ggml.FTYPE_MOSTLY_Q4_0, False, 100),
        # f32 weights: launch_qkv_rope_append
        "legacy_f32": ("tiny", ggml.FTYPE_ALL_F32, False, 8),
    }[producer]
    f = synthetic.build_model(preset, ftype=ftype, seed=3, n_layer=1)
    rng = np.random.default_rng(_seed("kv", producer))
    rest = [p for p in range(2, 2 + 2 * T) if p not in KV_POS]
    pos = np.array((KV_POS + rest)[:T], dtype=np.int32)
    assert len(set(pos.tolist())) == T
    seq = (rng.permutation(T) if decode else np.zeros(T)).astype(np.int32)
    x = rng.standard_normal((T, f.hparams.n_embd)).astype(np.float32)
    return Case(name="kv/" + producer, file=f, decode=decode, x=x, pos=pos,
                seq=seq, n_ctx=4096, max_batch=T if decode else 1)


def kv_reference(case):
    """TorchSliceEngine forward of the case -> layer-0 (K rows, V rows)
    [T, Ekv] f32 at the written (seq, pos), plus the un-rotated K rows
    (for the RoPE mutants)."""
    import torch
    from distributedllm_amd.engine.slice_engine import TorchSliceEngine
    from distributedllm_amd.models.llama import rms_norm
    eng = TorchSliceEngine.from_ggml(case.file, n_ctx=case.n_ctx,
                                     max_batch=case.max_batch)
    x = torch.from_numpy(case.x)
    eng.forward(x.clone(), torch.from_numpy(case.pos),
                torch.from_numpy(case.seq), decode=case.decode)
    T = len(case.pos)
    s, p = case.seq.astype(np.int64), case.pos.astype(np.int64)
    k = eng.k_cache[0, s, p].reshape(T, -1).numpy()
    v = eng.v_cache[0, s, p].reshape(T, -1).numpy()
    a = rms_norm(x) * eng.w["layers.0.attention_norm.weight"]
    k_pre = (a @ eng.w["layers.0.attention.wk.weight"].T).numpy()
    return k, v, k_pre


# ------------------------------------------- the RoPE angle, measured in f32

ANGLE_POS = [1, 511, 1607, 1609, 2047, 3000, 4095]
ANGLE_D, ANGLE_H = 128, 4       # pairs 0..3 of D = 128: the largest thetas


def angle_case(comp, ks):
    """A fused-decode launch whose f32 output reveals the angle the
    kernel's RoPE applied to q, without passing through f16: head h has
    q pair h = (sqrt(D), 0) before rotation and attends a row 0 whose K is
    the unit vector of element 2h + comp and whose V is 1 at d = 0; every
    other row, the appended one included, has K = 0, V = 0. Then
    out[t, h, 0] = e^s / (e^s + pos) with s = cos(theta) (comp 0) or
    sin(theta) (comp 1)."""
    D, H = ANGLE_D, ANGLE_H
    E = H * D
    T = len(ANGLE_POS)
    pos = np.array(ANGLE_POS, dtype=np.int32)
    seq = np.arange(T, dtype=np.int32)[::-1].copy()
    Kf, K = stores(T, 4096, E)
    Vf, V = stores(T, 4096, E)
    for h in range(H):
        K[:, 0, h * D + 2 * h + comp] = 1.0
        V[:, 0, h * D] = 1.0
    poison(K, V, pos - 1, seq)
    rows = np.zeros((T, 3 * E), dtype=np.float32)
    for h in range(H):
        rows[:, h * D + 2 * h] = math.sqrt(D)
    part = np.zeros((ks, 64, 3 * E), dtype=np.float32)
    part[0, :T] = rows          # the other partials are 0: exact sums
    slab = np.ascontiguousarray(
        part.reshape(ks, 64, 3 * E // 16, 16).transpose(2, 0, 1, 3))
    return Case(name="angle/comp%d" % comp, D=D, H=H, Hkv=H, n_ctx=4096,
                n_slots=T, T=T, ks=ks, slab=slab.reshape(-1),
                qsum=rows[:, :E], ksum=rows[:, E:2 * E],
                vsum=rows[:, 2 * E:], Kf=Kf, K=K, Vf=Vf, V=V, pos=pos,
                seq=seq, inv_freq=inv_freq_f32(D))


def check_angle(out_cos, out_sin):
    """Outputs of the two angle_case launches -> the applied angle per
    (token, pair), compared with pos * base**(-2i/D) in float64. Bound:
    the ROPE_ANGLE budget of the KV-row checks (theta is an f32 product
    with an f32-rounded inv_freq, then an f32 multiply by 1/2pi: about
    3 * theta * 2**-24 = 7e-4 rad at theta = 4095). The read-out itself
    resolves about 1e-6 rad (f32 output, one expf). Returns the worst
    error in rad."""
    D, H = ANGLE_D, ANGLE_H
    p = np.array(ANGLE_POS, dtype=np.float64)[:, None]
    s = []
    for out in (out_cos, out_sin):
        o = np.asarray(out, dtype=np.float64).reshape(len(ANGLE_POS), H,
                                                      D)[:, :, 0]
        assert np.isfinite(o).all() and (o > 0).all() and (o < 1).all()
        s.append(np.log(o * p / (1 - o)))
    theta = p * ROPE_BASE ** (-2.0 * np.arange(H) / D)[None, :]
    err = np.arctan2(s[1], s[0]) - theta
    err = np.abs((err + math.pi) % (2 * math.pi) - math.pi)
    rad = np.hypot(s[0], s[1])
    for i, pp in enumerate(ANGLE_POS):
        print("angle: pos %4d worst error %.3g rad (pair %d), |rot q|/|q| "
              "in [%.7f, %.7f]" % (pp, err[i].max(), err[i].argmax(),
                                   rad[i].min(), rad[i].max()))
    worst = float(err.max())
    print("angle: worst error / budget = %.3g" % (worst / ROPE_ANGLE))
    assert worst <= ROPE_ANGLE, "RoPE angle off by %.3g rad" % worst
    return worst
