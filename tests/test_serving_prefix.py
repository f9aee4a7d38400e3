"""`ContinuousBatcher(shared_prefix=ids)` on the CPU twin: every request
produces the tokens the plain batcher produces for the same prompt, whether
it shares the prefix slot or not."""
import pytest

from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.formats import slicer, synthetic
from distributedllm_amd.serving import ContinuousBatcher

PREFIX = [5, 9, 3, 12, 7, 2]
# sharing (long and one-token suffixes), not sharing (other start, the bare
# prefix, a short prompt)
PROMPTS = [PREFIX + [4, 11, 6, 1, 8, 3, 9], PREFIX + [10], [2, 11, 4, 6, 1],
           list(PREFIX), PREFIX + [3, 3, 4, 3, 3, 4, 3], [7]]
STEPS = [5, 4, 5, 3, 6, 3]


def _engine(max_batch):
    f = synthetic.build_model("tiny", seed=0)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=max_batch)
    eng.attach_extra(slicer.make_extra_layers(f))
    return eng


def _plain(prompt, steps):
    bat = ContinuousBatcher(_engine(1))
    r = bat.submit(prompt, steps)
    bat.run_all(max_steps=64)
    return r.out


@pytest.mark.parametrize("kw", [{}, {"prefill_chunk": 4},
                                {"spec_ngram": 2, "spec_k": 2},
                                {"lanes": 2}])
def test_tokens_match_the_plain_batcher(kw):
    kw = dict(kw)
    n_lanes = kw.pop("lanes", 1)
    lanes = [_engine(3) for _ in range(n_lanes)]
    bat = ContinuousBatcher(lanes[0], engines=lanes, shared_prefix=PREFIX,
                            **kw)
    assert bat.n_slots == 2 * n_lanes       # one slot per lane reserved
    calls = []
    for e in lanes:
        def fwd(*a, _f=e.forward, **k):
            calls.append("prefix" in k)
            return _f(*a, **k)
        e.forward = fwd
    reqs = [bat.submit(p, s) for p, s in zip(PROMPTS, STEPS)]
    shares = [True, True, False, False, True, False]
    while bat.pending:
        bat.step()
        for r in reqs:
            # the reserved slot (the last of each lane) is never handed out
            assert r.slot < bat.n_slots
    for r, p, s, sh in zip(reqs, PROMPTS, STEPS, shares):
        assert r.done and r.out == _plain(p, s)
        assert r._pfx == (len(PREFIX) if sh else 0)
    assert any(calls) and not all(calls[n_lanes:])
    assert sorted(bat.free) == list(range(bat.n_slots))


def test_cancel_mid_prefill_and_echo():
    bat = ContinuousBatcher(_engine(3), shared_prefix=PREFIX,
                            prefill_chunk=2)
    victim = bat.submit(PROMPTS[0], 5)
    other = bat.submit(PROMPTS[4], 6)
    echo = bat.submit(PROMPTS[0], 5, logprobs=1, echo=True)
    bat.step()
    assert victim.slot in bat.prefilling and bat.cancel(victim)
    late = bat.submit(PROMPTS[1], 4)        # reuses the cancelled slot
    bat.run_all(max_steps=64)
    assert other.out == _plain(PROMPTS[4], 6)
    assert late.out == _plain(PROMPTS[1], 4)
    plain = ContinuousBatcher(_engine(1))
    want = plain.submit(PROMPTS[0], 5, logprobs=1, echo=True)
    plain.run_all(max_steps=64)
    assert echo._pfx == 0 and echo.out == want.out
    assert echo.prompt_logprobs[1:] == pytest.approx(want.prompt_logprobs[1:],
                                                     abs=1e-5)


def test_construction_errors():
    class NoPrefix:
        max_batch, n_ctx, device = 3, 32, "cpu"

        def forward(self, x, pos, seq, decode=False):
            return x

    with pytest.raises(ValueError):
        ContinuousBatcher(NoPrefix(), shared_prefix=PREFIX)
    ContinuousBatcher(NoPrefix())
    with pytest.raises(ValueError):
        ContinuousBatcher(_engine(3), shared_prefix=[1] * 32)   # >= n_ctx
    eng = _engine(3)
    eng.prefill_cap = len(PREFIX) - 1
    with pytest.raises(ValueError):
        ContinuousBatcher(eng, shared_prefix=PREFIX)
    with pytest.raises(ValueError):
        ContinuousBatcher(_engine(1), shared_prefix=PREFIX)     # no slot left
