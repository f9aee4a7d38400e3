"""Device log-probability kernel (ops/csrc/logprobs.hip) against the
float64 `logprobs_reference` on the same f32 logits tensor.

Top-n ids involve no arithmetic (raw f32 order, ties to the smaller
index) and must equal the reference's exactly. For the values,

    |got - ref| <= 4 * V * 2**-24 + 1e-5 * (1 + |ref|)

The first term is the worst-case relative error of an f32 sum of V
non-negative terms in any order, entering the log once, with the 4x
head-room test_gpu_sampling.py uses for the same sum; the second covers
the f32 roundings of expf, the log and the final subtraction at
magnitudes up to ~40. It is a derived bound, not a measurement.

Every row gets a seed of its own (randn * 5), an exact tie of two logits
at ranks t, t+1 inside the top 8 (t varies per row, so the tie straddles
top_n = 1 and top_n = 5 on some rows, and either index order occurs),
and the first entry's row carries a block of -inf (at V = 33 a block so
wide that fewer than 8 finite logits remain). The chosen ids mix the
arg-max, a mid-rank token, the least likely finite token and, on the
-inf row, a token inside the block."""
import functools

import numpy as np
import pytest
import torch

from distributedllm_amd.engine.sampler import logprobs_reference

pytestmark = pytest.mark.gpu

VOCABS = [33, 256, 1000, 32003]
RS = [1, 5, 70]
TOPS = [0, 1, 5, 8]
EXTRA_T = 7       # logits rows that no launch entry points at


def _bound(V, ref):
    return 4 * V * 2.0 ** -24 + 1e-5 * (1 + np.abs(ref))


@functools.lru_cache(maxsize=None)
def _case(V, R):
    """A launch of R entries over a [R + EXTRA_T, V] logits tensor, with
    the reference computed once at top_n = 8 (a smaller top_n is its
    prefix)."""
    vi = VOCABS.index(V)
    rng = np.random.default_rng(20_000 * vi + R)
    Tn = R + EXTRA_T
    rows = rng.permutation(Tn)[:R].tolist()
    lg = np.empty((Tn, V), dtype=np.float32)
    for t in range(Tn):
        lg[t] = (np.random.default_rng(1_000_000 * (vi + 1) + 1000 * R + t)
                 .standard_normal(V) * 5).astype(np.float32)
    # -inf block on the first entry's row
    nb = V - 5 if V == 33 else V // 3
    lg[rows[0], 3:3 + nb] = -np.inf
    ids, pairs = [], []
    for r, t in enumerate(rows):
        order = np.argsort(-lg[t].astype(np.float64), kind="stable")
        n_fin = int(np.isfinite(lg[t]).sum())
        rank = min(t % 7, n_fin - 2)
        a, b = int(order[rank]), int(order[rank + 1])
        lg[t, a] = lg[t, b] = lg[t, a]          # exact tie at rank, rank+1
        pairs.append((rank, a, b))
        order = np.argsort(-lg[t].astype(np.float64), kind="stable")
        if r == 0:
            ids.append(3 + nb // 2)             # inside the -inf block
        else:
            ids.append(int(order[[0, n_fin // 2, n_fin - 1][r % 3]]))
    ref = [logprobs_reference(lg[t], i, 8) for t, i in zip(rows, ids)]
    return dict(V=V, R=R, rows=rows, ids=ids, lg=lg, pairs=pairs,
                lp=np.array([x[0] for x in ref]),
                top_ids=np.array([x[1] for x in ref], dtype=np.int64),
                top_lp=np.array([x[2] for x in ref]))


@pytest.fixture(scope="module")
def eng():
    from distributedllm_amd.engine import HIPSliceEngine
    from distributedllm_amd.formats import slicer, synthetic
    f = synthetic.build_model("tiny", seed=0)
    e = HIPSliceEngine.from_ggml(f, n_ctx=128, max_batch=3)
    e.attach_extra(slicer.make_extra_layers(f))
    return e


def _ids_dev(case):
    return torch.tensor(case["ids"], dtype=torch.int32, device="cuda")


def _check(case, n, lp, top_ids, top_lp, skip=()):
    V, R = case["V"], case["R"]
    lp, top_ids, top_lp = (lp.cpu().numpy(), top_ids.cpu().numpy(),
                           top_lp.cpu().numpy())
    assert lp.shape == (R,) and lp.dtype == np.float32
    assert top_ids.shape == (R, n) and top_ids.dtype == np.int32
    assert top_lp.shape == (R, n) and top_lp.dtype == np.float32
    keep = [r for r in range(R) if r not in skip]
    assert np.array_equal(top_ids[keep], case["top_ids"][keep, :n])
    worst = 0.0
    for got, ref in ((lp[keep], case["lp"][keep]),
                     (top_lp[keep], case["top_lp"][keep, :n])):
        inf = np.isneginf(ref)
        assert np.array_equal(np.isneginf(got), inf)    # -inf stays -inf
        assert np.isfinite(got[~inf]).all()
        if (~inf).any():
            err = np.abs(got[~inf].astype(np.float64) - ref[~inf])
            worst = max(worst, float((err / _bound(V, ref[~inf])).max()))
    print(f"V={V} R={R} top_n={n}: worst error / bound = {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("n", TOPS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("V", VOCABS)
def test_matches_reference(eng, V, R, n):
    case = _case(V, R)
    assert np.isneginf(case["lp"][0])
    if V == 33:
        assert np.isneginf(case["top_lp"][0, 5:]).all()
    lg = torch.from_numpy(case["lg"]).cuda()
    lp, top_ids, top_lp = eng.logprobs(lg, case["rows"], _ids_dev(case), n)
    _check(case, n, lp, top_ids, top_lp)
    # the logits, the rows no entry points at included, are unmodified
    assert np.array_equal(lg.cpu().numpy().view(np.uint32),
                          case["lg"].view(np.uint32))


def test_tie_cases_cover_both_index_orders_and_both_boundaries():
    """About the inputs, from the reference alone: among the R = 70 rows
    the tied pair sits across the top_n = 1 and the top_n = 5 cut, and
    the pair appears in both index orders (the smaller index must win
    either way)."""
    for V in VOCABS:
        case = _case(V, 70)
        lg = case["lg"]
        for r, (t, (rank, a, b)) in enumerate(zip(case["rows"],
                                                  case["pairs"])):
            top = case["top_ids"][r]
            assert lg[t, a] == lg[t, b] and rank + 1 < 8
            assert (top[rank], top[rank + 1]) == (min(a, b), max(a, b))
        assert {0, 4} <= {p[0] for p in case["pairs"]}
        assert {True, False} == {p[1] < p[2] for p in case["pairs"]}


@pytest.mark.parametrize("V,R,n", [(32003, 5, 8), (1000, 70, 5), (33, 5, 8)])
def test_two_launches_are_bit_identical(eng, V, R, n):
    case = _case(V, R)
    lg = torch.from_numpy(case["lg"]).cuda()
    ids = _ids_dev(case)
    a = eng.logprobs(lg, case["rows"], ids, n)
    b = eng.logprobs(lg, case["rows"], ids, n)
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1])
    for x, y in ((a[0], b[0]), (a[2], b[2])):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_greedy_entry_equals_first_top_entry(eng):
    """The chosen token's value and the same token's top-n value come
    from one expression: the batcher relies on their being identical."""
    case = _case(1000, 70)
    lg = torch.from_numpy(case["lg"]).cuda()
    rows = list(range(lg.shape[0]))
    ids = eng.argmax(lg)
    lp, top_ids, top_lp = eng.logprobs(lg, rows, ids, 1)
    assert torch.equal(top_ids[:, 0], ids)
    assert torch.equal(lp.view(torch.int32),
                       top_lp[:, 0].contiguous().view(torch.int32))


def test_ids_from_argmax_and_sample_stay_on_the_device(eng):
    """ids produced by engine.argmax / engine.sample go straight into the
    launch; the result equals that of the same ids uploaded from the
    host, and the reference's."""
    case = _case(1000, 5)
    V = case["V"]
    lg = torch.from_numpy(case["lg"]).cuda()
    Tn = lg.shape[0]
    rows = list(range(Tn))
    ids = eng.argmax(lg)
    assert ids.is_cuda and ids.dtype == torch.int32
    got = eng.logprobs(lg, rows, ids, 5)
    host = torch.tensor(ids.cpu().tolist(), dtype=torch.int32,
                        device="cuda")
    want = eng.logprobs(lg, rows, host, 5)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    ref = [logprobs_reference(case["lg"][t], int(i), 5)
           for t, i in zip(rows, ids.cpu().tolist())]
    assert np.array_equal(got[1].cpu().numpy(),
                          np.array([x[1] for x in ref]))
    lp_ref = np.array([x[0] for x in ref])
    assert (np.abs(got[0].cpu().numpy() - lp_ref) <=
            _bound(V, lp_ref)).all()

    srows = case["rows"]
    R = len(srows)
    seen = torch.zeros(R, (V + 31) // 32, dtype=torch.int32, device="cuda")
    sids = eng.sample(lg, srows, list(range(R)), [0.1, 0.3, 0.5, 0.7, 0.9],
                      [0.8] * R, [1.1] * R, [0] * R, [1.0] * R, seen)
    assert sids.is_cuda and sids.dtype == torch.int32
    got = eng.logprobs(lg, srows, sids, 5)
    sl = sids.cpu().tolist()
    assert all(0 <= i < V for i in sl)
    host = torch.tensor(sl, dtype=torch.int32, device="cuda")
    want = eng.logprobs(lg, srows, host, 5)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    lp_ref = np.array([logprobs_reference(case["lg"][t], i, 0)[0]
                       for t, i in zip(srows, sl)])
    fin = np.isfinite(lp_ref)
    assert fin.all()      # a sampled token has non-zero probability
    assert (np.abs(got[0].cpu().numpy() - lp_ref) <=
            _bound(V, lp_ref)).all()


def test_id_outside_the_vocabulary_gives_nan(eng):
    case = _case(256, 5)
    lg = torch.from_numpy(case["lg"]).cuda()
    ids = list(case["ids"])
    ids[1], ids[3] = case["V"], -1
    lp, top_ids, top_lp = eng.logprobs(
        lg, case["rows"],
        torch.tensor(ids, dtype=torch.int32, device="cuda"), 5)
    assert torch.isnan(lp[[1, 3]]).all().item()
    _check(case, 5, lp, top_ids, top_lp, skip=(1, 3))


def test_bad_arguments_are_refused(eng):
    case = _case(33, 5)
    lg = torch.from_numpy(case["lg"]).cuda()
    ids = _ids_dev(case)
    rows = case["rows"]
    with pytest.raises(ValueError):
        eng.logprobs(lg, rows, ids[:4], 0)                 # length mismatch
    with pytest.raises(ValueError):
        eng.logprobs(lg, rows[:4], ids, 0)
    with pytest.raises(ValueError):
        eng.logprobs(lg, [], ids[:0], 0)
    with pytest.raises(ValueError):
        eng.logprobs(lg, [0, 1, 2, 3, lg.shape[0]], ids, 0)  # row range
    with pytest.raises(ValueError):
        eng.logprobs(lg, [0, 1, 2, 3, -1], ids, 0)
    with pytest.raises(ValueError):
        eng.logprobs(lg, rows, ids, 9)                     # top_n range
    with pytest.raises(ValueError):
        eng.logprobs(lg, rows, ids, -1)
    small = lg[:, :4].contiguous()
    with pytest.raises(ValueError):
        eng.logprobs(small, rows, torch.zeros_like(ids), 5)  # top_n > V
    eng.logprobs(small, rows, torch.zeros_like(ids), 4)
    # the extension refuses what the wrapper would have caught, and ids
    # that are not a device i32 tensor
    rows_dev = torch.tensor(rows, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        eng._eng.logprobs(lg, rows_dev, ids, 9, max(rows))
    with pytest.raises(RuntimeError):
        eng._eng.logprobs(lg, rows_dev, ids, 0, lg.shape[0])
    with pytest.raises(RuntimeError):
        eng._eng.logprobs(lg, rows_dev, ids.cpu(), 0, max(rows))
    with pytest.raises(RuntimeError):
        eng._eng.logprobs(lg, rows_dev, ids.long(), 0, max(rows))
    torch.cuda.synchronize()
