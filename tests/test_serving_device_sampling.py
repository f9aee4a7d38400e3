"""`ContinuousBatcher(device_sampling=True)` on the CPU twin: the engine's
batched `sample` replaces the per-request host `Sampler.__call__` and
yields exactly the same tokens."""
import pytest
import torch

from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.engine.sampler import Sampler
from distributedllm_amd.formats import slicer, synthetic
from distributedllm_amd.serving import ContinuousBatcher


def _engine(max_batch):
    f = synthetic.build_model("tiny", seed=0)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=max_batch)
    eng.attach_extra(slicer.make_extra_layers(f))
    return eng


PROMPTS = [[5, 9, 3], [7], [2, 11, 4, 6, 1], [8, 2]]
STEPS = [6, 4, 3, 6]


def _samplers():
    # two sampled requests with different settings, one greedy, and a
    # fourth sampled one that has to wait for a slot
    return [Sampler(0.8, 1.1, seed=42, top_k=40, top_p=0.95),
            Sampler(1.3, 1.5, seed=7),
            None,
            Sampler(1.0, 2.0, seed=3, top_k=12)]


def _run(device_sampling, max_slots):
    bat = ContinuousBatcher(_engine(3), max_slots=max_slots,
                            device_sampling=device_sampling)
    samplers = _samplers()
    reqs = [bat.submit(p, s, sampler=sm)
            for p, s, sm in zip(PROMPTS, STEPS, samplers)]
    bat.run_all(max_steps=100)
    assert all(r.done for r in reqs)
    return reqs, samplers


@pytest.mark.parametrize("max_slots", [3, 2])
def test_device_sampling_matches_host_path(monkeypatch, max_slots):
    """Mixed batch (two sampled settings + greedy) with a queued request
    that reuses a finished request's slot: a missing reset of the slot's
    repetition state would change the reused slot's tokens."""
    want, want_s = _run(False, max_slots)

    def _boom(self, logits):
        raise AssertionError("Sampler.__call__ ran under device_sampling")

    monkeypatch.setattr(Sampler, "__call__", _boom)
    got, got_s = _run(True, max_slots)
    for w, g in zip(want, got):
        assert g.out == w.out and len(g.out) > 0
    for ws, gs in zip(want_s, got_s):
        if ws is not None:
            assert gs.previous_ids == ws.previous_ids


def test_slot_reuse_resets_repetition_state():
    """The second request lands in the slot the first one used; with a
    strong penalty at a low temperature its tokens depend on whether the
    first request's ids leaked into its penalty set."""
    def run(device_sampling):
        bat = ContinuousBatcher(_engine(1), device_sampling=device_sampling)
        a = bat.submit(PROMPTS[0], 8, sampler=Sampler(0.1, 4.0, seed=1))
        b = bat.submit(PROMPTS[0], 8, sampler=Sampler(0.1, 4.0, seed=1))
        bat.run_all(max_steps=100)
        return a.out, b.out

    assert run(True) == run(False)
    a, b = run(True)
    assert a == b  # same prompt, seed and (reset) state


def test_greedy_sampler_object_uses_argmax():
    bat = ContinuousBatcher(_engine(2), device_sampling=True)
    s = Sampler(greedy=True)
    r0 = bat.submit(PROMPTS[0], 4, sampler=s)
    r1 = bat.submit(PROMPTS[0], 4)
    bat.run_all(max_steps=50)
    assert r0.out == r1.out == s.previous_ids


def test_engine_without_sample_is_rejected():
    class _NoSample:
        max_batch = 2
        n_ctx = 32
        device = "cpu"

    with pytest.raises(ValueError):
        ContinuousBatcher(_NoSample(), device_sampling=True)
    ContinuousBatcher(_NoSample())  # the default path needs none


def test_twin_sample_matches_host_sampler_on_same_logits():
    eng = _engine(2)
    V = eng.hp.n_vocab
    g = torch.Generator().manual_seed(0)
    seen = eng.new_seen_state()
    host = Sampler(0.9, 1.4, seed=11, top_k=9, top_p=0.9)
    drv = Sampler(0.9, 1.4, seed=11, top_k=9, top_p=0.9)
    for _ in range(6):
        lg = torch.randn(3, V, generator=g) * 3
        want = host(lg[2].numpy())
        u, t, pen, k, p = drv.draw_params()
        got = eng.sample(lg, [2], [1], [u], [t], [pen], [k], [p], seen)
        assert got.dtype == torch.int32 and int(got[0]) == want
    assert torch.nonzero(seen[1]).reshape(-1).tolist() == sorted(
        set(host.previous_ids))
    assert not seen[0].any()
    eng.reset_seen(seen, 1)
    assert not seen.any()
