"""Direct tests of the attention kernels (ops/csrc/attention.hip) through
the test hooks of the extension, against the float64 reference in
attention_reference.py.

K and V are random, rounded to f16; the reference sees the same rounded
values, so cache rounding is not in the error. Q is f32. Every row above a
token's pos, every unused slot and the 16-half pad hold +30000 (K) /
-30000 (V): a kernel that reads one row too many, the wrong slot or the
wrong kv head is far outside every bound. Every case runs the same launch
twice and demands bit-identical results, and checks the f16 side channel
element by element (`check_attention`).

The bounds are derived (attention_reference.py, docs/kernels.md), not
tuned; every case prints its worst error / bound. The inputs, bounds and
assertion helpers are the ones tests/test_attention_reference.py proves to
reject all eight mutant references.

Worst error / bound measured on an MI355X (also in docs/kernels.md,
"Direct kernel tests"): decode 0.5 % (peaky, D = 16), decode with q = 0
0.3 %, prefill 2.1 % (T = 17, D = 24), prefill with q = 0 0.3 %, fused
appended K row 32 %, fused V row bit-exact, fused out 11 % of the plain
decode bound (D = 16, T = 64, pos 4095), RoPE angle of q 3.2e-4 rad =
32 % of the 1e-3 budget (pos 4095, pair 0). Positions above 1608 rotate
correctly: gfx950's sin/cos have no 512 pi domain cut.
"""
import numpy as np
import pytest
import torch

import attention_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    return ops.core()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _launch(fn, case):
    """Two launches of `fn` on fresh copies of the case's inputs; asserts
    they are bit-identical and that the caches are unchanged; returns
    (out, prep, jtw) of the first as numpy."""
    res = []
    for _ in range(2):
        k, v = _dev(case.Kf), _dev(case.Vf)
        out, prep, jtw = fn(_dev(case.q), k, v, _dev(case.pos),
                            _dev(case.seq), case.H, case.Hkv, case.n_ctx,
                            case.n_slots)
        torch.cuda.synchronize()
        assert np.array_equal(k.cpu().numpy().view(np.uint16),
                              case.Kf.view(np.uint16))
        assert np.array_equal(v.cpu().numpy().view(np.uint16),
                              case.Vf.view(np.uint16))
        res.append((out.cpu().numpy(), prep.cpu().numpy().view(np.uint16),
                    int(jtw)))
    (o1, p1, j1), (o2, p2, j2) = res
    assert j1 == j2 and np.array_equal(p1, p2)
    assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32)), \
        case.name + ": two launches differ"
    return o1, p1, j1


def test_restated_host_functions_match_the_extension(core):
    for T in list(range(1, 70)) + [100, 127, 128, 129, 1000]:
        assert core.jt_width(T) == R.jt_width_ref(T)
    for D, H, Hkv in R.SHAPES + [(128, 32, 32), (128, 64, 8)]:
        assert core.qkv16_ks(H * D, Hkv * D) == \
            R.qkv16_ks_ref(H * D, Hkv * D)


@pytest.mark.parametrize("kind", R.DECODE_KINDS)
@pytest.mark.parametrize("D,H,Hkv", R.SHAPES)
def test_decode(core, D, H, Hkv, kind):
    case = R.decode_case(kind, D, H, Hkv)
    out, prep, jtw = _launch(core.attention_decode, case)
    R.check_attention(case, out, prep, jtw)


@pytest.mark.parametrize("D,H,Hkv", [s for s in R.SHAPES if s[0] == 100])
def test_decode_last_addressable_row(core, D, H, Hkv):
    case = R.decode_case("last_row", D, H, Hkv)
    out, prep, jtw = _launch(core.attention_decode, case)
    R.check_attention(case, out, prep, jtw)


def test_decode_deep(core):
    case = R.decode_case("deep", 128, 8, 2)
    out, prep, jtw = _launch(core.attention_decode, case)
    R.check_attention(case, out, prep, jtw)


@pytest.mark.parametrize("kind", R.PREFILL_KINDS)
@pytest.mark.parametrize("D,H,Hkv", R.SHAPES)
def test_prefill(core, D, H, Hkv, kind):
    case = R.prefill_case(kind, D, H, Hkv)
    out, prep, jtw = _launch(core.attention_prefill, case)
    R.check_attention(case, out, prep, jtw)
    # the same inputs through the streaming kernel: within the decode
    # bound of the reference, hence within the prefill bound of the above
    dout, dprep, djtw = _launch(core.attention_decode, case)
    tol = (case.tol if case.tolkind == "uniform" else
           R.tol_decode(D, case.sabs, case.vmax))
    R.check_attention(case, dout, dprep, djtw, tol=tol)
    assert (np.abs(dout.astype(np.float64) - out) <= case.tol).all()


@pytest.mark.parametrize("shape,T", R.FUSED_CASES)
def test_fused_decode(core, shape, T):
    D, H, Hkv = shape
    case = R.fused_case(D, H, Hkv, T, int(core.qkv16_ks(H * D, Hkv * D)))
    res = []
    for _ in range(2):
        k, v = _dev(case.Kf), _dev(case.Vf)
        out, prep, jtw = core.attention_decode_fused(
            _dev(case.slab), k, v, _dev(case.pos), _dev(case.seq),
            _dev(case.inv_freq), H, Hkv, D, case.n_ctx, case.n_slots)
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), prep.cpu().numpy().view(np.uint16),
                    int(jtw), k.cpu().numpy(), v.cpu().numpy()))
    a, b = res
    for x, y in zip(a[:2] + a[3:], b[:2] + b[3:]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), \
            case.name + ": two launches differ"
    R.check_fused(case, *a)


def test_fused_rope_angle_at_deep_positions(core):
    """The angle k_attention<true> rotates q by, read out of the f32
    output to about 1e-6 rad (attention_reference.angle_case), at
    positions on both sides of the 512 pi input domain older ISA manuals
    give for the hardware sin/cos."""
    D, H = R.ANGLE_D, R.ANGLE_H
    ks = int(core.qkv16_ks(H * D, H * D))
    outs = []
    for comp in (0, 1):
        case = R.angle_case(comp, ks)
        out, _, _ = core.attention_decode_fused(
            _dev(case.slab), _dev(case.Kf), _dev(case.Vf), _dev(case.pos),
            _dev(case.seq), _dev(case.inv_freq), H, H, D, case.n_ctx,
            case.n_slots)
        outs.append(out.cpu().numpy())
    R.check_angle(*outs)


def test_hooks_refuse_what_could_go_out_of_bounds(core):
    case = R.decode_case("last_row", 100, 4, 4)
    q, k, v = _dev(case.q), _dev(case.Kf), _dev(case.Vf)
    pos, seq = _dev(case.pos), _dev(case.seq)
    H, Hkv, ctx, slots = case.H, case.Hkv, case.n_ctx, case.n_slots
    for fn in (core.attention_decode, core.attention_prefill):
        fn(q, k, v, pos, seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):      # pad missing
            fn(q, k[:-16].contiguous(), v, pos, seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):
            fn(q, k, v[:-1].contiguous(), pos, seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):      # pos == n_ctx
            fn(q, k, v, pos + 1, seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):
            fn(q, k, v, pos - ctx, seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):      # seq == n_slots
            fn(q, k, v, pos, seq + 1, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):      # dtypes / device
            fn(q.double(), k, v, pos, seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):
            fn(q, k.float(), v, pos, seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):
            fn(q, k, v, pos.long(), seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):
            fn(q.cpu(), k, v, pos, seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):      # non-contiguous q
            fn(q.repeat(1, 2)[:, ::2], k, v, pos, seq, H, Hkv, ctx, slots)
        with pytest.raises(RuntimeError):      # heads that do not divide
            fn(q, k, v, pos, seq, H, 3, ctx, slots)
        with pytest.raises(RuntimeError):      # T mismatch
            fn(q, k, v, pos.repeat(2), seq.repeat(2), H, Hkv, ctx, slots)
    # D = 130 > 128, and an odd D (E = 4 * 25 is no multiple of 16 either)
    for D in (130, 25):
        qq = torch.zeros(1, 4 * D, device="cuda")
        kk = torch.zeros(slots * ctx * 4 * D + 16, device="cuda",
                         dtype=torch.float16)
        with pytest.raises(RuntimeError):
            core.attention_decode(qq, kk, kk.clone(), pos, seq, 4, 4, ctx,
                                  slots)
    # D = 8, H = 2: even and small, but E = 16, Ekv = 8 is not 16-aligned
    qq = torch.zeros(1, 16, device="cuda")
    kk = torch.zeros(slots * ctx * 8 + 16, device="cuda",
                     dtype=torch.float16)
    with pytest.raises(RuntimeError):
        core.attention_decode(qq, kk, kk.clone(), pos, seq, 2, 1, ctx, slots)

    D, H, Hkv = 16, 4, 4
    fc = R.fused_case(D, H, Hkv, 5, int(core.qkv16_ks(H * D, Hkv * D)))

    def fused(slab=fc.slab, pos=fc.pos, seq=fc.seq, inv=fc.inv_freq,
              kf=fc.Kf):
        return core.attention_decode_fused(
            _dev(slab), _dev(kf), _dev(fc.Vf), _dev(pos), _dev(seq),
            _dev(inv), H, Hkv, D, fc.n_ctx, fc.n_slots)

    fused()
    with pytest.raises(RuntimeError):          # slab size
        fused(slab=fc.slab[:-1])
    with pytest.raises(RuntimeError):          # repeated sequence
        fused(seq=np.array([0, 1, 2, 3, 0], dtype=np.int32))
    with pytest.raises(RuntimeError):          # pos == n_ctx
        fused(pos=np.array([0, 1, 2, 3, fc.n_ctx], dtype=np.int32))
    with pytest.raises(RuntimeError):          # inv_freq length
        fused(inv=fc.inv_freq[:-1])
    with pytest.raises(RuntimeError):          # pad missing
        fused(kf=fc.Kf[:-16])
    with pytest.raises(RuntimeError):          # T = 65 > 64
        core.attention_decode_fused(
            _dev(fc.slab), torch.zeros(66 * 8 * 64 + 16, device="cuda",
                                       dtype=torch.float16),
            torch.zeros(66 * 8 * 64 + 16, device="cuda",
                        dtype=torch.float16),
            torch.zeros(65, dtype=torch.int32, device="cuda"),
            torch.arange(65, dtype=torch.int32, device="cuda"),
            _dev(fc.inv_freq), H, Hkv, D, 8, 66)
    torch.cuda.synchronize()
