"""`sample_reference` — the pure, uniform-driven form of `Sampler` that the
device sampling kernel is checked against — reproduces `Sampler.__call__`
token for token when fed `Generator.random()` from an equally seeded RNG."""
import numpy as np
import pytest

from distributedllm_amd.engine.sampler import Sampler, sample_reference

VOCABS = [256, 1000, 32003]
SETTINGS = [(0.7, 1.1, 0, 1.0), (1.0, 1.3, 40, 1.0), (0.8, 1.1, 0, 0.9),
            (0.8, 1.1, 50, 0.95), (1.5, 1.0, 7, 0.5)]
SEEDS = [0, 1, 2, 3, 4, 5]
STEPS = 5


def _host_probs(logits, prev, T, pen, top_k, top_p):
    """The host sampler's final distribution, captured from the `p=` it
    hands to `Generator.choice`."""
    s = Sampler(T, pen, seed=0, top_k=top_k, top_p=top_p)
    s.previous_ids = list(prev)
    seen = {}

    class _Spy:
        def choice(self, size, p):
            seen["p"] = np.array(p)
            return 0

    s.rng = _Spy()
    s(logits)
    return seen["p"]


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("setting", SETTINGS)
def test_matches_host_sampler(V, setting):
    T, pen, top_k, top_p = setting
    for seed in SEEDS:
        host = Sampler(T, pen, seed=seed, top_k=top_k, top_p=top_p)
        rng = np.random.default_rng(seed)
        data = np.random.default_rng(1000 + seed)
        prev = []
        for _ in range(STEPS):
            logits = (data.standard_normal(V) * 3).astype(np.float32)
            want_p = _host_probs(logits, prev, T, pen, top_k, top_p)
            want = host(logits)
            tid, kept = sample_reference(logits, rng.random(), prev, T, pen,
                                         top_k, top_p)
            assert tid == want
            assert np.array_equal(kept, want_p > 0)
            prev.append(tid)
        assert prev == host.previous_ids


def test_draw_params_is_the_sampler_stream():
    s = Sampler(0.8, 1.2, seed=9, top_k=5, top_p=0.9)
    rng = np.random.default_rng(9)
    for _ in range(3):
        assert s.draw_params() == (rng.random(), 0.8, 1.2, 5, 0.9)
    assert s.previous_ids == []


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("setting", SETTINGS)
def test_extreme_uniforms_stay_in_kept_set(V, setting):
    T, pen, top_k, top_p = setting
    logits = (np.random.default_rng(V).standard_normal(V) * 3).astype(
        np.float32)
    prev = [3, 17, V - 1]
    for u in (0.0, 1.0 - 2.0 ** -53):
        tid, kept = sample_reference(logits, u, prev, T, pen, top_k, top_p)
        assert kept[tid]
    lo, kept = sample_reference(logits, 0.0, prev, T, pen, top_k, top_p)
    hi, _ = sample_reference(logits, 1.0 - 2.0 ** -53, prev, T, pen, top_k,
                             top_p)
    idx = np.flatnonzero(kept)
    assert lo == idx[0] and hi == idx[-1]


@pytest.mark.parametrize("V", VOCABS)
def test_top_k_one_is_argmax(V):
    logits = (np.random.default_rng(7).standard_normal(V) * 3).astype(
        np.float32)
    for u in (0.0, 0.3, 0.999):
        tid, kept = sample_reference(logits, u, [], 0.9, 1.0, 1, 1.0)
        assert tid == int(np.argmax(logits)) and kept.sum() == 1


def test_ties_at_the_thresholds_are_kept():
    logits = np.array([2.0, 1.0, 2.0, 1.0, 0.0, 1.0], dtype=np.float32)
    _, kept = sample_reference(logits, 0.5, [], 1.0, 1.0, 3, 1.0)
    assert kept.tolist() == [True, True, True, True, False, True]
    _, kept = sample_reference(logits, 0.5, [], 1.0, 1.0, 0, 0.7)
    # the two 2.0 entries hold 0.62 < 0.7 of the mass; the cut lands on the 1.0
    # tie, which is kept whole
    assert kept.tolist() == [True, True, True, True, False, True]
