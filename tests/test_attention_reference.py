"""CPU checks of tests/attention_reference.py: the float64 reference agrees
with the project's torch twin, and - on the exact inputs, bounds and
assertion helpers the GPU tests use - the true reference rounded to f32
passes every case while each of the eight mutant references is rejected.
That second part is what keeps test_gpu_attention.py and
test_gpu_kv_writes.py honest: a kernel that computed a mutant would fail
them."""
import math

import numpy as np
import pytest
import torch

import attention_reference as R


def _rejects(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def _as_device(ref):
    out = ref.astype(np.float32)
    jtw = R.jt_width_ref(out.shape[0])
    return out, R.make_prep(out, jtw), jtw


# ------------------------------------------- reference vs the torch twin

@pytest.mark.parametrize("preset", ["tiny_gqa", "tiny_oddhead"])
def test_reference_agrees_with_the_torch_engine(preset):
    """One layer with wo = I and w2 = 0, so forward(x) - x is the
    attention output and the engine's caches are the rotated K / V."""
    from distributedllm_amd.engine.slice_engine import TorchSliceEngine
    from distributedllm_amd.formats import ggml
    from distributedllm_amd.models.llama import (PRESETS, rms_norm,
                                                 rope_interleaved)
    p = PRESETS[preset]
    hp = p.hparams(ggml.FTYPE_ALL_F32)
    E, Ekv, F, D = p.n_embd, p.n_embd_kv, p.n_ff, p.n_embd // p.n_head
    g = torch.Generator().manual_seed(5)
    pre = "layers.0."
    w = {pre + "attention_norm.weight": 1 + 0.1 * torch.randn(E, generator=g),
         pre + "attention.wq.weight": torch.randn(E, E, generator=g) / 8,
         pre + "attention.wk.weight": torch.randn(Ekv, E, generator=g) / 8,
         pre + "attention.wv.weight": torch.randn(Ekv, E, generator=g) / 8,
         pre + "attention.wo.weight": torch.eye(E),
         pre + "ffn_norm.weight": torch.ones(E),
         pre + "feed_forward.w1.weight": torch.randn(F, E, generator=g) / 8,
         pre + "feed_forward.w3.weight": torch.randn(F, E, generator=g) / 8,
         pre + "feed_forward.w2.weight": torch.zeros(E, F)}
    n_ctx, slots = 600, 3
    eng = TorchSliceEngine(hp, w, 1, 0, n_ctx=n_ctx, max_batch=slots)
    # rows written in increasing pos per sequence, sequences interleaved
    pos = np.array([0, 0, 1, 1, 2, 3, 2, 511, 4, 512], dtype=np.int32)
    seq = np.array([0, 2, 0, 2, 0, 0, 2, 2, 0, 2], dtype=np.int32)
    # slot 2 jumps to row 511: fill the gap so every attended row is real
    eng.k_cache[0, 2, 3:511] = torch.randn(508, p.kv_heads, D, generator=g)
    eng.v_cache[0, 2, 3:511] = torch.randn(508, p.kv_heads, D, generator=g)
    x = torch.randn(len(pos), E, generator=g)
    y = eng.forward(x.clone(), torch.from_numpy(pos), torch.from_numpy(seq))
    att = (y - x).numpy().astype(np.float64)

    a = (rms_norm(x) * w[pre + "attention_norm.weight"]).double()
    q_pre = (a @ w[pre + "attention.wq.weight"].double().T).numpy()
    k_pre = (a @ w[pre + "attention.wk.weight"].double().T).numpy()
    k_rot = R.rope_ref(k_pre, pos, D)
    # rope_ref vs rope_interleaved, position by position
    for t in range(len(pos)):
        want = rope_interleaved(
            torch.from_numpy(k_pre[t:t + 1]).float().view(1, -1, D),
            int(pos[t])).reshape(-1).numpy()
        assert np.abs(want - k_rot[t]).max() <= 4e-7 * np.abs(k_rot[t]).max()
    K = eng.k_cache[0].reshape(slots, n_ctx, Ekv).numpy()
    V = eng.v_cache[0].reshape(slots, n_ctx, Ekv).numpy()
    got_k = K[seq, pos]
    assert np.abs(got_k - k_rot).max() <= 1e-5 * np.abs(k_rot).max()
    ref = R.attention_ref(R.rope_ref(q_pre, pos, D), K, V, pos, seq,
                          p.n_head, p.kv_heads)
    # y - x cancels: its rounding is relative to |x| + |att|
    bound = 1e-5 * (np.abs(ref).max() + float(x.abs().max()))
    assert np.abs(att - ref).max() <= bound


def test_rope_ref_is_a_rotation_by_pos_times_inv_freq():
    D = 8
    x = np.zeros((1, D))
    x[0, 0::2] = 1.0                                 # every pair = (1, 0)
    out = R.rope_ref(x, [3000], D).reshape(-1, 2)
    theta = 3000 * 10000.0 ** (-2.0 * np.arange(D // 2) / D)
    assert np.allclose(out[:, 0], np.cos(theta), atol=1e-12)
    assert np.allclose(out[:, 1], np.sin(theta), atol=1e-12)


def test_xprep_index_layout():
    # [e/8][t/16 of jtw][t%16][e%8]
    jtw = 4
    lay = np.arange(5 * jtw * 16 * 8).reshape(5, jtw, 16, 8)
    for e, t in ((0, 0), (7, 0), (8, 0), (3, 15), (3, 16), (39, 63)):
        assert R.xprep_index(e, t, jtw) == lay[e // 8, t // 16, t % 16, e % 8]
    prep = R.make_prep(np.ones((17, 16), dtype=np.float32), 2)
    assert prep.size == 2 * 2 * 128 and (prep != 0).sum() == 17 * 16


def test_poison_is_finite_and_leaves_the_attended_rows():
    Kf, K = R.stores(3, 8, 16)
    Vf, V = R.stores(3, 8, 16)
    R.poison(K, V, [2, 5], [1, 1])
    assert np.isfinite(Kf).all() and np.isfinite(Vf).all()
    assert (K[1, :6] == 0).all() and (K[1, 6:] == 30000).all()
    assert (K[0] == 30000).all() and (V[2] == -30000).all()
    assert (Kf[-16:] == 30000).all() and (Vf[-16:] == -30000).all()


def test_slab_sums_are_sequential_f32_sums():
    rng = np.random.default_rng(0)
    T, E, Ekv, ks = 5, 32, 16, 4
    q, k, v = (rng.standard_normal((T, n)) for n in (E, Ekv, Ekv))
    slab, qs, ksum, vs = R.build_qkv_slab(q, k, v, ks, rng)
    s4 = slab.reshape((E + 2 * Ekv) // 16, ks, 64, 16)
    for t, e in ((0, 0), (4, 31), (2, 17)):
        acc = np.float32(0)
        for c in range(ks):
            acc = np.float32(acc + s4[e >> 4, c, t, e & 15])
        assert acc == qs[t, e]
    e = E + Ekv + 5                                   # a v row
    acc = np.float32(0)
    for c in range(ks):
        acc = np.float32(acc + s4[e >> 4, c, 3, e & 15])
    assert acc == vs[3, 5]
    assert np.abs(qs - q).max() < 1e-5 and np.abs(ksum - k).max() < 1e-5


# ------------------------------------- the GPU tests' inputs have teeth

def _attention_cases(kernel, shapes=R.SHAPES):
    """The case of every launch test_gpu_attention.py makes on `kernel`,
    cheapest-to-reject first."""
    if kernel == "decode":
        for kind in ("uniform", "peaky", "sweep", "triangle",
                     "triangle_shuffled"):
            for s in shapes:
                yield R.decode_case(kind, *s)
        for s in shapes:
            if s[0] == 100:
                yield R.decode_case("last_row", *s)
        yield R.decode_case("deep", 128, 8, 2)
    else:
        for kind in (["uniform_mixed", "uniform_span", "mixed", "edges"] +
                     [k for k in R.PREFILL_KINDS if k.startswith("span")]):
            for s in shapes:
                yield R.prefill_case(kind, *s)


@pytest.mark.parametrize("D,H,Hkv", R.SHAPES)
@pytest.mark.parametrize("kernel", ["decode", "prefill"])
def test_true_reference_passes_every_attention_case(kernel, D, H, Hkv):
    n = 0
    for case in _attention_cases(kernel, [(D, H, Hkv)]):
        if (case.D, case.H, case.Hkv) != (D, H, Hkv):
            continue                        # the one deep case
        R.check_attention(case, *_as_device(case.ref))
        n += 1
    assert n >= 5


@pytest.mark.parametrize("kernel", ["decode", "prefill"])
@pytest.mark.parametrize("mutant", [1, 2, 3, 4, 5, 6])
def test_attention_mutant_is_rejected(kernel, mutant):
    """Each attention mutant fails the assertion helper on at least one
    case of the decode launches and one of the prefill launches (both
    kernels need the teeth)."""
    for case in _attention_cases(kernel):
        bad = R.attention_ref(case.q, case.K, case.V, case.pos, case.seq,
                              case.H, case.Hkv, mutant=mutant)
        if _rejects(R.check_attention, case, *_as_device(bad)):
            return
    pytest.fail("mutant %d (%s) passes every %s case" % (
        mutant, R.MUTANTS[mutant], kernel))


@pytest.mark.parametrize("mutant", [1, 2, 3, 4])
@pytest.mark.parametrize("D,H,Hkv", R.SHAPES)
def test_row_count_mutants_fail_the_uniform_sweep_of_every_shape(
        D, H, Hkv, mutant):
    """A missing, extra or doubled row costs >= 0.5/257 of max|V| against
    a 1e-5 bound - at every head dim, not just somewhere."""
    case = R.decode_case("uniform", D, H, Hkv)
    bad = R.attention_ref(case.q, case.K, case.V, case.pos, case.seq, H,
                          Hkv, mutant=mutant)
    assert _rejects(R.check_attention, case, *_as_device(bad))


# every fused launch of the GPU test but two of the three T = 64 ones
# (64 slots of 4096 rows; one of them shows the helper handles T = 64)
FUSED_CPU = [c for c in R.FUSED_CASES if c[1] < 64] + [((16, 8, 2), 64)]


@pytest.mark.parametrize("shape,T", FUSED_CPU)
def test_true_reference_passes_the_fused_cases(shape, T):
    D, H, Hkv = shape
    case = R.fused_case(D, H, Hkv, T, R.qkv16_ks_ref(H * D, Hkv * D))
    R.check_fused(case, *R.simulate_fused(case))


@pytest.mark.parametrize("D,H,Hkv", R.SHAPES)
def test_fused_out_bound_has_teeth_token_by_token(D, H, Hkv):
    """The fused T = 8 launch holds one token at each of pos 0, 1, 31,
    32, 1607, 1609, 2047, 4095. With the ratios check_fused asserts on:
    a dropped first or last row, a doubled row and a missing rescale
    are each over the bound at pos 31 AND at pos 32 (the 32-row edge),
    and a doubled row and a missing rescale at every deep token too.
    (One dropped row of thousands has a weight of a few 1e-4 and is at
    the bound itself at depth for D >= 64; what a single row costs at
    depth is pinned by the q = 0 decode sweep and the bit-exact append
    checks.) kv head h % Hkv is over the bound at every token under
    GQA, an attended row J wherever its score is not hugely negative
    for every head."""
    case = R.fused_case(D, H, Hkv, 8, R.qkv16_ks_ref(H * D, Hkv * D))
    assert sorted(case.pos.tolist()) == R.FUSED_POS
    out, _, _, Kf, Vf = R.simulate_fused(case)
    Ka = Kf[:-16].reshape(case.K.shape)
    Va = Vf[:-16].reshape(case.V.shape)
    assert R.fused_out_ratios(case, out, Ka, Va)[0].max() < 0.01
    at = {int(p): t for t, p in enumerate(case.pos)}
    deep = [1607, 1609, 2047, 4095]
    ratios = {}
    for mutant in (1, 2, 3, 4, 5, 6):
        bad = R.simulate_fused(case, mutant)[0]
        ratios[mutant] = R.fused_out_ratios(case, bad, Ka, Va)[0]
    for mutant, where in ((1, [0, 1, 31, 32]), (2, [0, 1, 31, 32]),
                          (4, [31, 32] + deep), (6, [1, 31, 32] + deep)):
        for p in where:
            assert ratios[mutant][at[p]] > 10, (mutant, p)
    if H != Hkv:
        assert (ratios[5] > 10).all()
    assert (ratios[3] > 10).sum() >= 4


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_fused_case_rejects_every_mutant(mutant):
    case = R.fused_case(16, 8, 2, 5, R.qkv16_ks_ref(128, 32))
    assert _rejects(R.check_fused, case, *R.simulate_fused(case, mutant))


def test_fused_case_notices_a_touched_neighbour_and_an_inexact_v_row():
    case = R.fused_case(16, 8, 2, 5, R.qkv16_ks_ref(128, 32))
    out, prep, jtw, Kf, Vf = R.simulate_fused(case)
    t = 2
    K2 = Kf.copy()
    K2[:-16].reshape(case.K.shape)[case.seq[t], case.pos[t] + 1, 0] = 1.0
    assert _rejects(R.check_fused, case, out, prep, jtw, K2, Vf)
    V2 = Vf.copy()
    row = V2[:-16].reshape(case.V.shape)[case.seq[t], case.pos[t]]
    row[3] = np.nextafter(row[3], np.float16(np.inf))        # one f16 ulp
    assert _rejects(R.check_fused, case, out, prep, jtw, Kf, V2)
    p2 = prep.copy()
    p2[np.flatnonzero(p2 == 0)[0]] = 1                 # stray side write
    assert _rejects(R.check_fused, case, out, p2, jtw, Kf, Vf)


def test_angle_read_out_recovers_the_rotation_and_rejects_rope_mutants():
    ks = R.qkv16_ks_ref(512, 512)
    cases = [R.angle_case(c, ks) for c in (0, 1)]
    outs = [R.simulate_fused(c)[0] for c in cases]
    assert R.check_angle(*outs) < 2e-6
    for mutant in (7, 8):
        bad = [R.simulate_fused(c, mutant)[0] for c in cases]
        assert _rejects(R.check_angle, *bad)


# ------------------------------------------------- engine-level KV rows

def test_kv_positions_rotate_pair_0_visibly():
    """theta of pair 0 is pos itself: none of the deep positions sits
    near a multiple of 2 pi, so a lost rotation moves pair 0 by
    2 |sin(pos / 2)| of its length."""
    for p in R.KV_POS:
        if p > R.ROPE_DOMAIN:
            assert 2 * abs(math.sin(p / 2)) > 0.4, p
    assert sum(p > R.ROPE_DOMAIN for p in R.KV_POS) == 4
    assert 1607 < R.ROPE_DOMAIN < 1609


@pytest.mark.parametrize("producer", R.KV_PRODUCERS)
def test_kv_rows_reject_the_rope_mutants(producer):
    case = R.kv_case(producer)
    k, v, k_pre = R.kv_reference(case)
    D = case.file.hparams.head_dim
    pos = case.pos
    # rope_ref on the un-rotated rows is the engine's cache row
    assert np.abs(R.rope_ref(k_pre, pos, D) - k).max() <= \
        1e-5 * np.abs(k).max()
    f16 = lambda a: np.asarray(a, np.float32).astype(np.float16)  # noqa
    R.check_kv_rows(case.name, f16(k), f16(v), k, v, pos)
    for mutant in (7, 8):
        bad = f16(R.rope_ref(k_pre, pos, D, mutant=mutant))
        assert _rejects(R.check_kv_rows, case.name, bad, f16(v), k, v, pos)
    # mutant 7 is caught at each deep position on its own
    for i, p in enumerate(pos):
        if p > R.ROPE_DOMAIN:
            bad = f16(R.rope_ref(k_pre[i:i + 1], pos[i:i + 1], D, mutant=7))
            assert _rejects(R.check_kv_rows, case.name, bad, f16(v[i:i + 1]),
                            k[i:i + 1], v[i:i + 1], pos[i:i + 1])
    # a V row off by 4 f16 ulps of its largest element is caught too
    bad_v = f16(v).copy()
    j = np.abs(v[0]).argmax()
    bad_v[0, j] = np.float16(v[0, j] * (1 + 4 * 2.0 ** -10))
    assert _rejects(R.check_kv_rows, case.name, f16(k), bad_v, k, v, pos)
