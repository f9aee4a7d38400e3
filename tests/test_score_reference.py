"""Prompt scoring on the host: the float64 definition `score_reference`,
the CPU twin's `score()`, and the perplexity command that is built on it."""
import numpy as np
import pytest
import torch

from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.engine.sampler import (logprobs_reference,
                                               score_reference)
from distributedllm_amd.formats import slicer, synthetic


def _rows(T=9, V=40, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, V)) * 4).astype(np.float32)


def test_score_reference_is_float64_log_softmax():
    lg = _rows()
    T, V = lg.shape
    tg = np.random.default_rng(1).integers(0, V, T)
    lp, top_id, top_lp = score_reference(lg, tg)
    want = torch.log_softmax(torch.from_numpy(lg).double(), dim=-1).numpy()
    assert lp.dtype == np.float64 and top_lp.dtype == np.float64
    assert np.allclose(lp, want[np.arange(T), tg], rtol=0, atol=1e-12)
    assert np.array_equal(top_id, lg.argmax(axis=1))
    assert np.allclose(top_lp, want.max(axis=1), rtol=0, atol=1e-12)


def test_score_reference_is_logprobs_reference_at_top_1():
    lg = _rows(seed=4)
    T, V = lg.shape
    tg = np.random.default_rng(2).integers(0, V, T)
    lp, top_id, top_lp = score_reference(lg, tg)
    for t in range(T):
        v, ids, lps = logprobs_reference(lg[t], tg[t], 1)
        assert lp[t] == v and top_id[t] == ids[0] and top_lp[t] == lps[0]


def test_tie_goes_to_the_smaller_index_and_bad_target_gives_nan():
    lg = _rows(seed=5)
    T, V = lg.shape
    lg[0, 7] = lg[0, 30] = lg[0].max() + 1      # either order of writing
    lg[1, 33] = lg[1, 2] = lg[1].max() + 1
    tg = np.arange(T) % V
    tg[2], tg[3] = -1, V
    lp, top_id, top_lp = score_reference(lg, tg)
    assert top_id[0] == 7 and top_id[1] == 2
    assert np.isnan(lp[[2, 3]]).all()
    assert np.isfinite(np.delete(lp, [2, 3])).all()
    assert np.isfinite(top_lp).all()            # still written
    with pytest.raises(ValueError):
        score_reference(lg, tg[:-1])
    with pytest.raises(ValueError):
        score_reference(lg[0], tg[:1])


def _twin(n_ctx=32):
    f = synthetic.build_model("tiny", seed=0)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=1)
    eng.attach_extra(slicer.make_extra_layers(f))
    return eng


def _prefill(eng, toks):
    n = len(toks)
    return eng.forward(eng.embed(torch.tensor(toks, dtype=torch.int32)),
                       torch.arange(n, dtype=torch.int32),
                       torch.zeros(n, dtype=torch.int32))


def test_twin_score_matches_the_reference():
    eng = _twin()
    V = eng.hp.n_vocab
    y = _prefill(eng, [5, 9, 3, 200, 17, 42, 8])
    lg = eng.logits(y, all_logits=True).numpy()
    tg = [9, 3, 200, -1, 42, V, 0]
    for targets in (tg, torch.tensor(tg, dtype=torch.int32)):
        lp, top_id, top_lp = eng.score(y, targets)
        assert lp.dtype == torch.float32 and top_id.dtype == torch.int32
        assert top_lp.dtype == torch.float32
        r_lp, r_id, r_tlp = score_reference(lg, tg)
        assert np.array_equal(top_id.numpy(), r_id)
        assert np.array_equal(np.isnan(lp.numpy()), np.isnan(r_lp))
        ok = ~np.isnan(r_lp)
        # f32 log_softmax of f32 logits against the float64 one
        assert np.allclose(lp.numpy()[ok], r_lp[ok], rtol=0, atol=1e-5)
        assert np.allclose(top_lp.numpy(), r_tlp, rtol=0, atol=1e-5)
    with pytest.raises(ValueError):
        eng.score(y, tg[:-1])


def test_twin_score_tie_goes_to_the_smaller_index():
    eng = _twin()
    # two identical lm_head rows that win: rows 11 and 200 of the weights
    w = eng.w["output.weight"]
    y = _prefill(eng, [5, 9, 3])
    yn = eng.logits(y, all_logits=True)
    big = w[int(yn[0].argmax())].clone()
    w[200] = big * 2
    w[11] = big * 2
    lg = eng.logits(y, all_logits=True)
    assert lg[0, 11] == lg[0, 200] == lg[0].max()
    _, top_id, _ = eng.score(y, [0, 0, 0])
    assert int(top_id[0]) == 11


def test_local_perplexity_value_is_unchanged(tmp_path, monkeypatch):
    """The perplexity command on the CPU twin returns, bit for bit, what
    it computed from full logits and a host log_softmax."""
    # the command picks the HIP engine where there is a GPU: pin the twin
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from distributedllm_amd.cli.commands import _local_perplexity
    from distributedllm_amd.engine import engine_for_slice
    from distributedllm_amd.engine.tokenizer import Tokenizer
    from distributedllm_amd.formats import ggml

    f = synthetic.build_model("tiny", seed=0)
    path = tmp_path / "tiny.bin"
    f.save(str(path))
    text = "hello world, this is a perplexity probe"
    got = _local_perplexity(str(path), text)

    f = ggml.GGMLFile.load(str(path), extended=ggml.sniff_extended(str(path)))
    tokens = Tokenizer(f.vocab).encode(text, bos=True)
    assert len(tokens) > 4
    eng = engine_for_slice(f, n_ctx=max(len(tokens) + 1, 16), max_batch=1,
                           device="cpu")
    eng.attach_extra(slicer.make_extra_layers(f))
    n = len(tokens) - 1
    y = eng.forward(eng.embed(torch.tensor(tokens[:-1], dtype=torch.int32)),
                    torch.arange(n, dtype=torch.int32),
                    torch.zeros(n, dtype=torch.int32))
    lg = eng.logits(y, all_logits=True)
    logp = torch.log_softmax(lg.float().cpu(), dim=-1).numpy()
    nll = [-logp[i, tokens[i + 1]] for i in range(n)]
    want = float(np.exp(np.mean(nll)))
    assert np.float64(got).tobytes() == np.float64(want).tobytes()
