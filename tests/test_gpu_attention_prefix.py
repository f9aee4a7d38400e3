"""Direct tests of shared-prefix attention (k_attn_prefix and
k_attn_prefix_tail, ops/csrc/attention.hip) through the `attention_prefix`
hook, and of `forward(..., prefix=)` in the engine.

Definition under test: token t attends rows [0, pfx[t]) of slot `pslot`, then
rows [pfx[t], pos[t]] of its own slot. The float64 reference is
`attention_reference.attention_ref` on a second K/V in which the prefix rows
have been copied into each sharing token's own slot. In the stores the kernel
sees, those own rows [0, P) are poisoned, like everything above the filled
ranges: the kernel must never read them.

The bound is `tol_prefill` (f16 Q and f16 P on the matrix cores: this
kernel's arithmetic). The merge needs no extra term: the output is a convex
combination of the normalised prefix partials, each within that bound, and of
the tighter f32 tail; the weights carry f32 rounding only.

n_ctx = 272 gives chunk 256 and two splits, so P = 257 crosses the first
chunk; T = 19 fills one 16-token tile and leaves a ragged second; tokens 3
and 17 have no prefix. Tails pos - P cycle over 0, 1, 40, capped by the end
of the context (14 at P = 257).
"""
import functools

import numpy as np
import pytest
import torch

import attention_reference as R
from distributedllm_amd.formats import ggml, synthetic

pytestmark = pytest.mark.gpu

N_CTX = 272
SHAPES = [(16, 4, 4), (100, 8, 4), (128, 8, 2)]
PREFIXES = [1, 15, 16, 17, 257]


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    return ops.core()


@functools.lru_cache(maxsize=None)
def prefix_case(D, H, Hkv, P, T=19, share=True):
    rng = np.random.default_rng(R._seed("prefix", D, H, Hkv, P, T, share))
    E, Ekv = H * D, Hkv * D
    n_slots = T + 1
    perm = rng.permutation(n_slots)
    seq, pslot = perm[:T].astype(np.int32), int(perm[T])
    tails = np.minimum(np.array([0, 1, 40])[np.arange(T) % 3], N_CTX - 1 - P)
    pos = (P + tails).astype(np.int32)
    pfx = np.full(T, P if share else 0, dtype=np.int32)
    pfx[[i for i in (3, 17) if i < T]] = 0
    Kf, K, Vf, V = R._random_kv(rng, n_slots, N_CTX, Ekv)
    R.poison(K, V, list(pos) + [P - 1], list(seq) + [pslot])
    # the reference's stores: prefix rows copied into the sharing slots
    Kr, Vr = K.copy(), V.copy()
    for t in np.flatnonzero(pfx):
        Kr[seq[t], :P], Vr[seq[t], :P] = K[pslot, :P], V[pslot, :P]
        K[seq[t], :P], V[seq[t], :P] = 30000.0, -30000.0
    q = rng.standard_normal((T, E)).astype(np.float32)
    ref, sabs, vmax = R._attend(q, Kr, Vr, pos, seq, H, Hkv)
    return R.Case(name="prefix/D%d_H%d_%d_P%d_T%d%s" % (
        D, H, Hkv, P, T, "" if share else "_plain"), D=D, H=H, Hkv=Hkv,
        n_ctx=N_CTX, n_slots=n_slots, q=q, Kf=Kf, Vf=Vf, pos=pos, seq=seq,
        pfx=pfx, pslot=pslot, P=P, ref=ref,
        tol=R.tol_prefill(sabs, vmax))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(core, case, rows=None):
    """One launch on fresh copies of the case (or of its tokens `rows`);
    the caches must come back unchanged."""
    rows = slice(None) if rows is None else rows
    k, v = _dev(case.Kf), _dev(case.Vf)
    out, prep, jtw = core.attention_prefix(
        _dev(case.q[rows]), k, v, _dev(case.pos[rows]), _dev(case.seq[rows]),
        _dev(case.pfx[rows]), case.pslot, case.P, case.H, case.Hkv,
        case.n_ctx, case.n_slots)
    torch.cuda.synchronize()
    assert np.array_equal(k.cpu().numpy().view(np.uint16),
                          case.Kf.view(np.uint16))
    assert np.array_equal(v.cpu().numpy().view(np.uint16),
                          case.Vf.view(np.uint16))
    return out.cpu().numpy(), prep.cpu().numpy().view(np.uint16), int(jtw)


@pytest.mark.parametrize("P", PREFIXES)
@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_prefix(core, D, H, Hkv, P):
    case = prefix_case(D, H, Hkv, P)
    out, prep, jtw = _run(core, case)
    out2, prep2, _ = _run(core, case)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), \
        case.name + ": two launches differ"
    assert np.array_equal(prep, prep2)
    R.check_attention(case, out, prep, jtw)
    # a token alone (T = 1) has the bits of its row in the full launch
    for i in (0, 3, 15, 16, 18):
        alone, _, _ = _run(core, case, slice(i, i + 1))
        assert np.array_equal(alone[0].view(np.uint32),
                              out[i].view(np.uint32)), "token %d" % i


def test_prefix_wide(core):
    """T = 70: one split over the whole prefix, five tiles."""
    assert core.attn_prefix_chunk(N_CTX) == 256
    assert [core.attn_prefix_splits(N_CTX, T) for T in (1, 19, 70)] == [2, 2, 1]
    case = prefix_case(100, 8, 4, 257, T=70)
    out, prep, jtw = _run(core, case)
    R.check_attention(case, out, prep, jtw)


@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_no_prefix_is_plain_attention(core, D, H, Hkv):
    case = prefix_case(D, H, Hkv, 257, share=False)
    assert not case.pfx.any()
    out, prep, jtw = _run(core, case)
    R.check_attention(case, out, prep, jtw)


# ------------------------------------------------------------------ engine

def _rel_rms(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("preset", ["small", "small_gqa"])
def test_engine_prefix_matches_cpu(preset):
    """A 40-token prefix in slot 3; slots 0..2 prefill 5 suffix tokens each
    and decode 3 steps with prefix=, against the TorchSliceEngine twin."""
    from distributedllm_amd.engine import HIPSliceEngine, TorchSliceEngine
    f = synthetic.build_model(preset, ftype=ggml.FTYPE_MOSTLY_Q4_0, seed=0)
    hip = HIPSliceEngine.from_ggml(f, n_ctx=256, max_batch=4)
    cpu = TorchSliceEngine.from_ggml(f, n_ctx=256, max_batch=4)
    g = torch.Generator().manual_seed(22)
    E, P = f.hparams.n_embd, 40
    i32 = dict(dtype=torch.int32)
    steps = [(P, torch.arange(P, **i32), torch.full((P,), 3, **i32), False,
              None),
             (15, torch.arange(P, P + 5, **i32).repeat(3),
              torch.arange(3, **i32).repeat_interleave(5), False, P)]
    for i in range(3):
        steps.append((3, torch.full((3,), P + 5 + i, **i32),
                      torch.arange(3, **i32), True, P))
    for T, pos, seq, decode, pf in steps:
        x = torch.randn(T, E, generator=g) * 0.5
        pfx = None if pf is None else torch.full((T,), pf, **i32)
        got = hip.forward(
            x.cuda(), pos.cuda(), seq.cuda(), decode=decode,
            prefix=None if pf is None else (3, P, pfx.cuda())).cpu()
        want = cpu.forward(x.clone(), pos, seq,
                           prefix=None if pf is None else (3, P, pfx))
        assert _rel_rms(got, want) <= 8e-3
    x = torch.randn(1, E, generator=g).cuda()
    one = torch.full((1,), P, **i32).cuda()
    zero = torch.zeros(1, **i32).cuda()
    for pslot, plen in [(4, P), (-1, P), (3, 0), (3, 256)]:
        with pytest.raises(RuntimeError):
            hip.forward(x, one, zero, prefix=(pslot, plen, one))


def test_engine_legacy_path_refuses_prefix():
    from distributedllm_amd.engine import HIPSliceEngine
    f = synthetic.build_model("tiny", ftype=ggml.FTYPE_ALL_F32, seed=0)
    hip = HIPSliceEngine.from_ggml(f, n_ctx=64, max_batch=2)
    x = torch.zeros(1, f.hparams.n_embd).cuda()
    one = torch.ones(1, dtype=torch.int32).cuda()
    with pytest.raises(RuntimeError):
        hip.forward(x, one, one - 1, prefix=(1, 1, one))
