"""`logprobs_reference`: the float64 definition of per-token
log-probabilities (raw logits, full vocabulary, ties to the smaller
index) and its CPU-engine twin `TorchSliceEngine.logprobs`."""
import numpy as np
import pytest
import torch

from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.engine.sampler import logprobs_reference
from distributedllm_amd.formats import slicer, synthetic


@pytest.mark.parametrize("V", [1, 2, 33, 1000, 32003])
def test_matches_float64_log_softmax(V):
    rng = np.random.default_rng(V)
    x = (rng.standard_normal(V) * 5).astype(np.float32)
    want = torch.log_softmax(torch.from_numpy(x).double(), dim=-1).numpy()
    n = min(8, V)
    for tid in {0, V // 2, V - 1, int(np.argmax(x)), int(np.argmin(x))}:
        lp, top_ids, top_lp = logprobs_reference(x, tid, n)
        assert abs(lp - want[tid]) <= 1e-12
        assert top_ids.shape == (n,) and top_lp.shape == (n,)
        assert np.abs(top_lp - want[top_ids]).max() <= 1e-12
        # descending, and nothing outside the list beats its last entry
        assert (np.diff(x[top_ids]) <= 0).all()
        rest = np.delete(x, top_ids)
        assert rest.size == 0 or rest.max() <= x[top_ids[-1]]
    assert abs(np.exp(want).sum() - 1) < 1e-9


def test_sampler_settings_do_not_enter():
    """The signature takes raw logits only; a scaled row (what a
    temperature would produce) gives a different answer, so the value is
    a function of the raw row alone."""
    x = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    a, _, _ = logprobs_reference(x, 2)
    b, _, _ = logprobs_reference(x / 0.5, 2)
    x64 = x.astype(np.float64)
    assert a == pytest.approx(np.log(np.exp(3.0) / np.exp(x64).sum()),
                              abs=1e-12)
    assert a != b


def test_ties_resolve_to_the_smaller_index():
    x = np.full(12, -3.0, dtype=np.float32)
    x[[7, 2, 9]] = 4.0          # duplicated maxima
    x[[5, 1]] = 1.5             # a tied pair below them
    x[[10, 3, 6]] = 0.25        # a tied triple straddling top_n = 6
    _, ids, lp = logprobs_reference(x, 0, 6)
    assert ids.tolist() == [2, 7, 9, 1, 5, 3]   # 6 and 10 are cut
    assert lp[0] == lp[1] == lp[2] and lp[3] == lp[4]
    _, ids, _ = logprobs_reference(x, 0, 7)
    assert ids.tolist() == [2, 7, 9, 1, 5, 3, 6]
    _, ids, _ = logprobs_reference(x, 0, 2)     # cut inside the maxima
    assert ids.tolist() == [2, 7]
    _, ids, _ = logprobs_reference(x, 0, 12)
    assert ids.tolist() == [2, 7, 9, 1, 5, 3, 6, 10, 0, 4, 8, 11]


def test_minus_inf_entries():
    x = np.array([0.5, -np.inf, 2.0, -np.inf, 1.0], dtype=np.float32)
    want = torch.log_softmax(torch.from_numpy(x).double(), dim=-1).numpy()
    lp, ids, tlp = logprobs_reference(x, 1, 5)
    assert lp == -np.inf
    assert ids.tolist() == [2, 4, 0, 1, 3]
    assert np.abs(tlp[:3] - want[[2, 4, 0]]).max() <= 1e-12
    assert tlp[3] == -np.inf and tlp[4] == -np.inf
    lp, _, _ = logprobs_reference(x, 2, 0)
    assert abs(lp - want[2]) <= 1e-12 and np.isfinite(lp)


def test_top_n_zero_returns_only_the_logprob():
    x = np.arange(6, dtype=np.float32)
    lp, ids, tlp = logprobs_reference(x, 3, 0)
    assert isinstance(lp, float) and ids.shape == (0,) and tlp.shape == (0,)
    assert logprobs_reference(x, 3)[0] == lp      # top_n defaults to 0


def test_bad_arguments_raise():
    x = np.arange(6, dtype=np.float32)
    with pytest.raises(ValueError):
        logprobs_reference(x, 0, 7)               # top_n > V
    logprobs_reference(x, 0, 6)                   # == V is legal
    with pytest.raises(ValueError):
        logprobs_reference(x, 0, -1)
    with pytest.raises(ValueError):
        logprobs_reference(x, 6, 0)
    with pytest.raises(ValueError):
        logprobs_reference(x, -1, 0)


def test_torch_engine_twin_agrees_exactly():
    f = synthetic.build_model("tiny", seed=0)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=2)
    eng.attach_extra(slicer.make_extra_layers(f))
    V = eng.hp.n_vocab
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(6, V, generator=g) * 5
    lg[4, 10] = lg[4, 3] = lg[4].max() + 1        # tie at the top
    lg[1, 5:9] = -float("inf")
    rows = [4, 1, 5, 1]
    ids = torch.tensor([10, 6, int(lg[5].argmax()), 0], dtype=torch.int32)
    keep = lg.clone()
    for n in (0, 1, 5, 8):
        lp, top_ids, top_lp = eng.logprobs(lg, rows, ids, n)
        assert lp.dtype == torch.float32 and lp.shape == (4,)
        assert top_ids.dtype == torch.int32 and top_ids.shape == (4, n)
        assert top_lp.dtype == torch.float32 and top_lp.shape == (4, n)
        for r in range(4):
            w_lp, w_ids, w_tlp = logprobs_reference(
                lg[rows[r]].numpy(), int(ids[r]), n)
            assert float(lp[r]) == float(np.float32(w_lp))
            assert top_ids[r].tolist() == w_ids.tolist()
            assert np.array_equal(top_lp[r].numpy(),
                                  w_tlp.astype(np.float32))
        assert float(lp[1]) == -float("inf")
        if n:
            assert top_ids[0, 0].item() == 3      # smaller index of the tie
    assert torch.equal(lg, keep)
    assert eng.logprobs(lg, rows, ids)[1].shape == (4, 0)
    with pytest.raises(ValueError):
        eng.logprobs(lg, rows, ids[:3], 0)
    with pytest.raises(ValueError):
        eng.logprobs(lg, [0, 1, 2, 6], ids, 0)
    with pytest.raises(ValueError):
        eng.logprobs(lg, rows, ids, 9)
    with pytest.raises(ValueError):
        eng.logprobs(lg, rows, ids, -1)
    with pytest.raises(ValueError):
        eng.logprobs(lg[:, :4].contiguous(), rows,
                     torch.zeros(4, dtype=torch.int32), 5)   # top_n > V
