"""Prompt scoring through the continuous batcher on the CPU twin:
`submit(..., logprobs=n, echo=True)` and the pure scoring request
`max_new=0`."""
import numpy as np
import pytest
import torch

from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.engine.sampler import (Sampler, logprobs_reference,
                                               score_reference)
from distributedllm_amd.formats import slicer, synthetic
from distributedllm_amd.serving import ContinuousBatcher

F = synthetic.build_model("tiny", seed=0)
PROMPTS = [[5, 9, 3, 17, 200, 42, 8], [7], [2, 11, 4, 6, 1, 90, 33, 21, 60],
           [8, 2]]
ATOL = 2e-5   # f32 forward in chunks against one f32 forward of the prompt


def _engine(max_batch=2, n_ctx=32):
    eng = TorchSliceEngine.from_ggml(F, n_ctx=n_ctx, max_batch=max_batch)
    eng.attach_extra(slicer.make_extra_layers(F))
    return eng


def _direct(prompt, n):
    """score_reference (and the n-entry top list) over one direct forward
    of the whole prompt body."""
    eng = _engine(1)
    T = len(prompt) - 1
    if T == 0:
        return [None], [None]
    y = eng.forward(eng.embed(torch.tensor(prompt[:-1], dtype=torch.int32)),
                    torch.arange(T, dtype=torch.int32),
                    torch.zeros(T, dtype=torch.int32))
    lg = eng.logits(y, all_logits=True).numpy()
    lp, _, _ = score_reference(lg, prompt[1:])
    tops = []
    for t in range(T):
        _, ids, lps = logprobs_reference(lg[t], prompt[t + 1], n)
        tops.append(list(zip(ids.tolist(), lps.tolist())))
    return [None] + lp.tolist(), [None] + tops


def _check(r, n):
    lp, tops = _direct(r.prompt, n)
    assert len(r.prompt_logprobs) == len(r.prompt_top) == len(r.prompt)
    assert r.prompt_logprobs[0] is None and r.prompt_top[0] is None
    assert np.allclose(r.prompt_logprobs[1:], lp[1:], rtol=0, atol=ATOL)
    for got, want in zip(r.prompt_top[1:], tops[1:]):
        assert len(got) == n
        assert [i for i, _ in got] == [i for i, _ in want]
        assert np.allclose([p for _, p in got], [p for _, p in want],
                           rtol=0, atol=ATOL)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("chunk", [1, 3, None])
@pytest.mark.parametrize("n", [0, 1, 5])
def test_prompt_records_equal_the_reference(n, chunk, lanes):
    """Four prompts over two slots: echo and non-echo requests share
    admission streams, slots get recycled, and both top-alternative routes
    run (n <= 1 from score() alone, n = 5 through logits + logprobs)."""
    engs = [_engine(1) for _ in range(lanes)]
    bat = ContinuousBatcher(engs[0], max_slots=2, prefill_chunk=chunk,
                            engines=engs if lanes > 1 else None)
    echo = [True, True, False, True]
    reqs = [bat.submit(p, 3, logprobs=n, echo=e)
            for p, e in zip(PROMPTS, echo)]
    bat.run_all(max_steps=200)
    for r, e in zip(reqs, echo):
        assert r.done and len(r.out) == 3
        if e:
            _check(r, n)
        else:
            assert r.prompt_logprobs == [] and r.prompt_top == []


def test_generation_does_not_depend_on_echo():
    def run(echo):
        bat = ContinuousBatcher(_engine(2), max_slots=2, prefill_chunk=3)
        reqs = [bat.submit(p, 4, logprobs=2, echo=echo,
                           sampler=Sampler(0.8, 1.1, seed=3) if i == 2
                           else None)
                for i, p in enumerate(PROMPTS)]
        bat.run_all(max_steps=200)
        return reqs
    for a, b in zip(run(False), run(True)):
        assert a.out == b.out and len(a.out) == 4
        assert a.out_logprobs == b.out_logprobs and a.out_top == b.out_top
        assert a.prompt_logprobs == [] and len(b.prompt_logprobs) == \
            len(b.prompt)


def test_pure_scoring_requests():
    bat = ContinuousBatcher(_engine(1), max_slots=1, prefill_chunk=4)
    a = bat.submit(PROMPTS[2], 0, logprobs=1, echo=True)
    b = bat.submit(PROMPTS[1], 0, logprobs=1, echo=True)   # one token
    c = bat.submit(PROMPTS[0], 2, logprobs=1, echo=True)
    done = bat.step()                    # 4 of a's 8 body tokens
    assert done == [] and not a.done and len(a.prompt_logprobs) == 5
    done = bat.step()
    assert done == [a] and a.done and a.out == [] and a.slot == -1
    assert bat.free == [0] and not bat.active
    _check(a, 1)
    done = bat.step()                    # b finishes at admission; c admits
    assert b in done and b.done and b.out == []
    assert b.prompt_logprobs == [None] and b.prompt_top == [None]
    rest = bat.run_all(max_steps=50)
    assert c in done + rest and len(c.out) == 2
    _check(c, 1)
    assert bat.pending == 0 and bat.free == [0]


def test_cancel_during_a_chunked_echo_prefill():
    bat = ContinuousBatcher(_engine(1), max_slots=1, prefill_chunk=3)
    r = bat.submit(PROMPTS[2], 2, logprobs=5, echo=True)
    bat.step()
    bat.step()
    assert r.slot in bat.prefilling and r._pf_pos == 6
    assert bat.cancel(r)
    assert len(r.prompt_logprobs) == len(r.prompt_top) == 1 + 6
    lp, tops = _direct(PROMPTS[2], 5)
    assert np.allclose(r.prompt_logprobs[1:], lp[1:7], rtol=0, atol=ATOL)
    assert [[i for i, _ in t] for t in r.prompt_top[1:]] == \
        [[i for i, _ in t] for t in tops[1:7]]
    assert bat.free == [0] and bat.pending == 0


class _NoScore:
    """An engine facade without score() (the pipeline facade's shape)."""

    def __init__(self, eng):
        self._e = eng
        for name in ("forward", "embed", "logits", "argmax", "logprobs",
                     "n_ctx", "max_batch", "device"):
            setattr(self, name, getattr(eng, name))


def test_every_value_error():
    bat = ContinuousBatcher(_engine(1))
    with pytest.raises(ValueError, match="echo needs logprobs"):
        bat.submit(PROMPTS[0], 2, echo=True)
    with pytest.raises(ValueError, match="max_new must be >= 1"):
        bat.submit(PROMPTS[0], 0)                      # as before
    with pytest.raises(ValueError, match="max_new must be >= 1"):
        bat.submit(PROMPTS[0], 0, logprobs=1)          # needs echo
    with pytest.raises(ValueError, match="max_new must be >= 1"):
        bat.submit(PROMPTS[0], -1, logprobs=1, echo=True)
    with pytest.raises(ValueError, match="at least one token"):
        bat.submit([], 0, logprobs=1, echo=True)
    with pytest.raises(ValueError, match="logprobs must be an integer"):
        bat.submit(PROMPTS[0], 1, logprobs=9, echo=True)
    with pytest.raises(ValueError, match="exceeds n_ctx"):
        bat.submit(list(range(1, 34)), 0, logprobs=1, echo=True)
    assert bat.pending == 0 and bat.free == [0]       # no slot was taken
    bat.submit(list(range(1, 33)), 0, logprobs=1, echo=True)  # fits exactly
    bat.run_all(max_steps=5)
    plain = ContinuousBatcher(_NoScore(_engine(1)))
    with pytest.raises(ValueError, match="echo needs an engine with score"):
        plain.submit(PROMPTS[0], 2, logprobs=1, echo=True)
    plain.submit(PROMPTS[0], 2, logprobs=1)            # logprobs alone: fine
    plain.run_all(max_steps=20)


class _Counting:
    def __init__(self, eng):
        self._e = eng
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self._e, name)

    def score(self, *a, **k):
        self.calls += 1
        return self._e.score(*a, **k)


def test_no_echo_request_never_scores():
    eng = _Counting(_engine(2))
    bat = ContinuousBatcher(eng, max_slots=2, prefill_chunk=3)
    for p in PROMPTS:
        bat.submit(p, 3, logprobs=2)
    bat.run_all(max_steps=200)
    assert eng.calls == 0
    r = bat.submit(PROMPTS[0], 0, logprobs=0, echo=True)
    bat.run_all(max_steps=20)
    assert eng.calls == 2 and r.done          # 6 body tokens in chunks of 3
    assert all(t == [] for t in r.prompt_top[1:])
