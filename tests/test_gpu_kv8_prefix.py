"""Shared-prefix attention over the int8 KV cache (k_attn_kv8_prefix and
k_attn_kv8_prefix_tail, ops/csrc/attention_kv8.hip) through the
`attention_kv8_prefix` hook, and `kv8_prefix=` in the engine.

The setup is test_gpu_attention_prefix.py's (n_ctx = 272: chunk 256, two
splits; T = 19; tokens 3 and 17 without a prefix; tails 0, 1, 40) on the
quantised stores of test_kv8_prefill_reference.py. The float64 reference runs
over the DEQUANTISED cache with the prefix rows copied into each sharing
token's own slot, and the bound is `tol_prefill` with that cache's sabs and
vmax: both passes have the matrix-core arithmetic the bound covers (f16 Q,
f16 P~ <= 1), and the merge is a convex combination of the normalised parts
whose weights carry f32 rounding only. Every row the definition forbids (own
rows [0, P) of sharing slots, rows above pos, rows >= P of pslot) holds bytes
0xFF with scale 60000 in the stores the kernel sees, about 7.6e6 per element:
one wrong row breaks the bound.
"""
import functools

import numpy as np
import pytest
import torch

import attention_reference as R
from distributedllm_amd.formats import ggml, synthetic
from test_kv8_prefill_reference import dequantized
from test_kv8_reference import rel_rms

pytestmark = pytest.mark.gpu

N_CTX = 272
SHAPES = [(16, 4, 4), (100, 8, 4), (128, 16, 2), (32, 24, 1)]
PREFIXES = [1, 31, 32, 33, 257]
ENGINE_BOUND = 8e-3     # test_gpu_kv8.py: the f16 engines' bound, unchanged


@pytest.fixture(scope="module")
def core():
    from distributedllm_amd import ops
    return ops.core()


@functools.lru_cache(maxsize=None)
def prefix_case(D, H, Hkv, P, T=19, share=True):
    rng = np.random.default_rng(R._seed("kv8_prefix", D, H, Hkv, P, T, share))
    Ekv, n_slots = Hkv * D, T + 1
    perm = rng.permutation(n_slots)
    seq, pslot = perm[:T].astype(np.int32), int(perm[T])
    tails = np.minimum(np.array([0, 1, 40])[np.arange(T) % 3], N_CTX - 1 - P)
    pos = (P + tails).astype(np.int32)
    pfx = np.full(T, P if share else 0, dtype=np.int32)
    pfx[[i for i in (3, 17) if i < T]] = 0
    _, K, _, V = R._random_kv(rng, n_slots, N_CTX, Ekv)
    st, Kd, Vd = dequantized(R.Case(K=K, V=V, D=D))
    # poison, in the byte domain, of the stores the kernel sees
    bad = np.zeros((n_slots, N_CTX), dtype=bool)
    bad[pslot, P:] = True
    for t in range(T):
        bad[seq[t], pos[t] + 1:] = True
        bad[seq[t], :pfx[t]] = True
    for b8, sc in ((st[0], st[1]), (st[2], st[3])):
        b8[:-16].reshape(n_slots, N_CTX, Ekv)[bad] = 0xFF
        sc.reshape(n_slots, N_CTX, Hkv)[bad] = np.float16(60000)
    # the reference's cache: prefix rows copied into the sharing slots
    for t in np.flatnonzero(pfx):
        Kd[seq[t], :P], Vd[seq[t], :P] = Kd[pslot, :P], Vd[pslot, :P]
    q = rng.standard_normal((T, H * D)).astype(np.float32)
    ref, sabs, vmax = R._attend(q, Kd, Vd, pos, seq, H, Hkv)
    return R.Case(name="kv8_prefix/D%d_H%d_%d_P%d_T%d%s" % (
        D, H, Hkv, P, T, "" if share else "_plain"), D=D, H=H, Hkv=Hkv,
        n_ctx=N_CTX, n_slots=n_slots, q=q, st=st, pos=pos, seq=seq, pfx=pfx,
        pslot=pslot, P=P, ref=ref, tol=R.tol_prefill(sabs, vmax))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(core, c, rows=slice(None)):
    """One launch on fresh copies of the case (or of its tokens `rows`);
    caches and scales must come back unchanged."""
    dev = [_dev(a) for a in c.st]
    out, prep, jtw = core.attention_kv8_prefix(
        _dev(c.q[rows]), dev[0], dev[2], dev[1], dev[3], _dev(c.pos[rows]),
        _dev(c.seq[rows]), _dev(c.pfx[rows]), c.pslot, c.P, c.H, c.Hkv,
        c.n_ctx, c.n_slots)
    torch.cuda.synchronize()
    for d, a in zip(dev, c.st):
        assert np.array_equal(d.cpu().numpy().view(np.uint8),
                              a.view(np.uint8))
    return out.cpu().numpy(), prep.cpu().numpy().view(np.uint16), int(jtw)


@pytest.mark.parametrize("P", PREFIXES)
@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_kv8_prefix(core, D, H, Hkv, P):
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


def test_kv8_prefix_wide(core):
    """T = 70: one split over the whole prefix, five tiles."""
    assert core.attn_kv8_prefix_chunk(N_CTX) == 256
    assert [core.attn_kv8_prefix_splits(N_CTX, T)
            for T in (1, 19, 70)] == [2, 2, 1]
    case = prefix_case(100, 8, 4, 257, T=70)
    out, prep, jtw = _run(core, case)
    R.check_attention(case, out, prep, jtw)


@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_no_prefix_is_plain_attention(core, D, H, Hkv):
    case = prefix_case(D, H, Hkv, 257, share=False)
    assert not case.pfx.any()
    out, prep, jtw = _run(core, case)
    R.check_attention(case, out, prep, jtw)


@pytest.mark.parametrize("preset", ["small", "small_gqa"])
def test_engine_kv8_prefix_matches_twin(preset):
    """test_engine_prefix_matches_cpu's steps on q8 engines with kv8_prefix:
    a 40-token prefix in slot 3; slots 0..2 prefill 5 suffix tokens each and
    decode 3 steps with prefix=, against the q8 TorchSliceEngine twin."""
    from distributedllm_amd.engine import HIPSliceEngine, TorchSliceEngine
    f = synthetic.build_model(preset, ftype=ggml.FTYPE_MOSTLY_Q4_0, seed=0)
    kw = dict(n_ctx=256, max_batch=4, kv_dtype="q8", kv8_prefix=True)
    hip = HIPSliceEngine.from_ggml(f, **kw)
    cpu = TorchSliceEngine.from_ggml(f, **kw)
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
        err = rel_rms(got, want)
        print("%s T %d prefix %s: rel-RMS %.3g" % (preset, T, pf, err))
        assert err <= ENGINE_BOUND
    x = torch.randn(1, E, generator=g).cuda()
    one = torch.full((1,), P, **i32).cuda()
    zero = torch.zeros(1, **i32).cuda()
    for pslot, plen in [(4, P), (-1, P), (3, 0), (3, 256)]:
        with pytest.raises(RuntimeError):
            hip.forward(x, one, zero, prefix=(pslot, plen, one))
