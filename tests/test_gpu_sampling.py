"""Device sampling kernel (ops/csrc/sampling.hip) against the float64
`sample_reference` on the same logits tensor.

Exact-token checks use constructed uniforms. `need = 4 * V * 2**-24` is
the worst-case relative error of an f32 sum of V non-negative terms in
any order, times 4 (softmax denominator, top-k mass, top-p mass, and the
division). Every kept token with reference probability >= 2*need is a
target; u is placed at 25/50/75 % of its CDF interval, which leaves a
margin of at least need/2 to either boundary, and the kernel must return
exactly that token. top_p of the top-p rows is the midpoint between the
sorted cumulative masses on either side of a cut token that itself has
probability >= 2*need, so the cut decision has the same margin.

Each row's logits come from a seed of its own; a seed whose reference
distribution does not meet the preconditions (two targets, a top-k
boundary gap > 1e-4 relative, a cut token distinct from its successor) is
replaced by the next one — decided from the reference alone, before the
kernel runs."""
import copy
import functools

import numpy as np
import pytest
import torch

from distributedllm_amd.engine.sampler import (Sampler, reference_probs,
                                               sample_reference)

pytestmark = pytest.mark.gpu

VOCABS = [33, 256, 1000, 32003]
RS = [1, 5, 70]
KINDS = ["none", "top_k", "top_p", "both", "low_t", "no_pen"]
EXTRA_T = 7       # logits rows that no launch entry points at
EXTRA_SLOTS = 3   # slots that no launch entry points at
U_MAX32 = float(np.float32(1.0 - 2.0 ** -24))


def _f32(x):
    return float(np.float32(x))


def _row_case(V, kind, seed):
    """One row's inputs and targets, or None if `seed` misses a
    precondition. Everything here is float64 reference arithmetic on the
    f32-rounded parameters the kernel receives."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal(V) * 5).astype(np.float32)
    prev = sorted(rng.choice(V, size=5, replace=False).tolist())
    need = 4 * V * 2.0 ** -24
    T, pen, k, top_p = {
        "none": (0.8, 1.1, 0, 1.0),
        "top_k": (1.0, 1.3, min(40, V // 2), 1.0),
        "top_p": (0.8, 1.1, 0, None),
        "both": (0.8, 1.1, min(50, V // 2), None),
        "low_t": (0.01, 1.1, 0, 1.0),
        "no_pen": (0.7, 1.0, 0, 1.0),
    }[kind]
    T, pen = _f32(T), _f32(pen)
    if k:
        mask = np.zeros(V, dtype=bool)
        mask[prev] = True
        z = logits.astype(np.float64) / ((mask * pen + ~mask) *
                                         (T + Sampler.EPS))
        zs = np.sort(z)[::-1]
        gap = (zs[k - 1] - zs[k]) / max(abs(zs[k - 1]), abs(zs[k]))
        if not gap > 1e-4:
            return None
    if top_p is None:
        pk = reference_probs(logits, prev, T, pen, k, 1.0)
        srt = np.sort(pk)[::-1]
        csum = np.cumsum(srt)
        big = int((srt >= 2 * need).sum())
        c = max(1, big // 2)
        if big < 2 or c + 1 >= V or srt[c] == srt[c + 1]:
            return None
        top_p = _f32(0.5 * (csum[c - 1] + csum[c]))
        if not (csum[c - 1] + need / 2 < top_p < csum[c] - need / 2):
            return None
    probs = reference_probs(logits, prev, T, pen, k, top_p)
    cdf = np.cumsum(probs)
    cdf = cdf / cdf[-1]
    targets = np.flatnonzero(probs >= 2 * need)
    if len(targets) < 2:
        return None
    us, want = [], []
    for t in targets:
        lo = cdf[t - 1] if t else 0.0
        for f in (0.25, 0.5, 0.75):
            u = _f32(lo + f * (cdf[t] - lo))
            assert sample_reference(logits, u, prev, T, pen, k,
                                    top_p)[0] == t
            us.append(u)
            want.append(int(t))
    return dict(logits=logits, prev=prev, T=T, pen=pen, k=k, top_p=top_p,
                kept=probs > 0, us=us, want=want, n_targets=len(targets),
                kind=kind)


def _bitmap(n_slots, V, slot_prev):
    bm = np.zeros((n_slots, (V + 31) // 32), dtype=np.uint32)
    for s, ids in slot_prev.items():
        for i in ids:
            bm[s, i >> 5] |= np.uint32(1 << (i & 31))
    return bm


def _bits(bm_row, V):
    return [i for i in range(V) if (int(bm_row[i >> 5]) >> (i & 31)) & 1]


@functools.lru_cache(maxsize=None)
def _case(V, R):
    """A launch of R entries over a [R + EXTRA_T, V] logits tensor: rows
    a shuffled subset, slots distinct and not in row order, settings
    mixed per entry."""
    vi = VOCABS.index(V)
    rng = np.random.default_rng(10_000 * vi + R)
    Tn, n_slots = R + EXTRA_T, R + EXTRA_SLOTS
    rows = rng.permutation(Tn)[:R].tolist()
    slots = rng.permutation(n_slots)[:R].tolist()
    lg = (np.random.default_rng(77 + vi).standard_normal((Tn, V)) *
          5).astype(np.float32)
    entries = []
    for r in range(R):
        kind = KINDS[(r + R + vi) % len(KINDS)]
        base = 1_000_000 * (vi + 1) + 10_000 * R + 100 * r
        for attempt in range(2000):
            e = _row_case(V, kind, base * 100 + attempt)
            if e is not None:
                break
        assert e is not None, (V, R, r, kind)
        assert e["n_targets"] >= 2
        lg[rows[r]] = e["logits"]
        entries.append(e)
    seen = _bitmap(n_slots, V, {slots[r]: entries[r]["prev"]
                                for r in range(R)})
    return dict(V=V, R=R, rows=rows, slots=slots, entries=entries,
                lg=lg, seen=seen, n_slots=n_slots)


@pytest.fixture(scope="module")
def eng():
    from distributedllm_amd.engine import HIPSliceEngine
    from distributedllm_amd.formats import slicer, synthetic
    f = synthetic.build_model("tiny", seed=0)
    # n_ctx also sizes the engine's per-call row cap (>= the R = 70 case)
    e = HIPSliceEngine.from_ggml(f, n_ctx=128, max_batch=3)
    e.attach_extra(slicer.make_extra_layers(f))
    return e


def _dev(case):
    lg = torch.from_numpy(case["lg"]).cuda()
    seen = torch.from_numpy(case["seen"].view(np.int32)).cuda()
    return lg, seen


def _launch(eng, case, lg, seen, us):
    es = case["entries"]
    return eng.sample(lg, case["rows"], case["slots"], us,
                      [e["T"] for e in es], [e["pen"] for e in es],
                      [e["k"] for e in es], [e["top_p"] for e in es], seen)


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("R", RS)
def test_constructed_uniforms_give_exact_tokens(eng, V, R):
    case = _case(V, R)
    es = case["entries"]
    lg, seen0 = _dev(case)
    n = max(len(e["us"]) for e in es)
    outs = []
    for j in range(n):
        us = [e["us"][j % len(e["us"])] for e in es]
        outs.append(_launch(eng, case, lg, seen0.clone(), us))
    got = torch.stack(outs).cpu().numpy()
    want = np.array([[e["want"][j % len(e["want"])] for e in es]
                     for j in range(n)])
    bad = np.argwhere(got != want)
    print(f"V={V} R={R}: targets/row "
          f"{min(e['n_targets'] for e in es)}.."
          f"{max(e['n_targets'] for e in es)}, "
          f"{sum(len(e['us']) for e in es)} constructed u, "
          f"{len(bad)} mismatches")
    for j, r in bad[:10]:
        print("  mismatch", es[r]["kind"], "u", es[r]["us"][j % len(
            es[r]["us"])], "want", want[j, r], "got", got[j, r])
    assert len(bad) == 0


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("R", RS)
def test_result_is_always_in_the_kept_set(eng, V, R):
    """Strict: for random and extreme u the id has non-zero reference
    probability after filtering."""
    case = _case(V, R)
    es = case["entries"]
    lg, seen0 = _dev(case)
    rng = np.random.default_rng(5)
    ulist = [np.zeros(R), np.full(R, U_MAX32)] + [rng.random(R)
                                                  for _ in range(64)]
    outs = [_launch(eng, case, lg, seen0.clone(), u.tolist())
            for u in ulist]
    got = torch.stack(outs).cpu().numpy()
    assert got.min() >= 0 and got.max() < V
    for r, e in enumerate(es):
        assert e["kept"][got[:, r]].all(), (e["kind"], r)


@pytest.mark.parametrize("V", [33, 32003])
def test_seen_state_is_updated_and_reset(eng, V):
    R = 5
    case = _case(V, R)
    es = case["entries"]
    lg, seen = _dev(case)
    first = _launch(eng, case, lg, seen, [e["us"][1] for e in es])
    first = first.cpu().tolist()
    after = seen.cpu().numpy().view(np.uint32)
    assert first == [e["want"][1] for e in es]
    used = set(case["slots"])
    for s in range(case["n_slots"]):
        if s not in used:
            assert not after[s].any()
    prev2 = []
    for r, e in enumerate(es):
        want_bits = sorted(set(e["prev"]) | {first[r]})
        assert _bits(after[case["slots"][r]], V) == want_bits
        prev2.append(want_bits)

    def mid_u(e, prev):
        # centre of the most probable token's interval under `prev`
        probs = reference_probs(e["logits"], prev, e["T"], e["pen"],
                                e["k"], e["top_p"])
        t = int(np.argmax(probs))
        cdf = np.cumsum(probs) / probs.sum()
        lo = cdf[t - 1] if t else 0.0
        u = _f32(lo + 0.5 * (cdf[t] - lo))
        return u, sample_reference(e["logits"], u, prev, e["T"], e["pen"],
                                   e["k"], e["top_p"])[0]

    # second launch on the same state: penalty set now includes the
    # first pick (top_p stays as constructed; the most probable token's
    # interval is far wider than the f32 error)
    pairs = [mid_u(e, p) for e, p in zip(es, prev2)]
    second = _launch(eng, case, lg, seen, [u for u, _ in pairs])
    assert second.cpu().tolist() == [t for _, t in pairs]
    # reset: the reference with an empty list
    for s in case["slots"]:
        eng.reset_seen(seen, s)
    assert not seen.any().item()
    pairs = [mid_u(e, []) for e in es]
    third = _launch(eng, case, lg, seen, [u for u, _ in pairs])
    third = third.cpu().tolist()
    assert third == [t for _, t in pairs]
    after = seen.cpu().numpy().view(np.uint32)
    for r in range(R):
        assert _bits(after[case["slots"][r]], V) == [third[r]]


def test_identical_inputs_give_identical_ids(eng):
    case = _case(32003, 70)
    lg, seen0 = _dev(case)
    us = np.random.default_rng(11).random(70).tolist()
    runs = []
    for _ in range(3):
        seen = seen0.clone()
        ids = _launch(eng, case, lg, seen, us).cpu().numpy()
        runs.append((ids, seen.cpu().numpy()))
    for ids, seen in runs[1:]:
        assert np.array_equal(ids, runs[0][0])
        assert np.array_equal(seen, runs[0][1])


def test_bad_arguments_are_refused(eng):
    case = _case(33, 5)
    lg, seen = _dev(case)
    args = ([0.5] * 5, [0.8] * 5, [1.1] * 5, [0] * 5, [1.0] * 5)
    with pytest.raises(ValueError):
        eng.sample(lg, [0, 1, 2, 3, lg.shape[0]], case["slots"], *args,
                   seen)
    with pytest.raises(ValueError):
        eng.sample(lg, case["rows"], [0, 1, 2, 3, seen.shape[0]], *args,
                   seen)
    with pytest.raises(ValueError):
        eng.sample(lg, case["rows"], [0, 1, 2, 3, 3], *args, seen)
    params = torch.zeros(7, 5, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        eng._eng.sample(lg, params, seen[:, :-1].contiguous(), 0, 0)
    with pytest.raises(RuntimeError):
        eng._eng.sample(lg, params, seen, lg.shape[0], 0)
    with pytest.raises(RuntimeError):
        eng._eng.sample(lg, params, seen, 0, seen.shape[0])
    too_many = int(eng._eng.max_prefill) + 1
    params = torch.zeros(7, too_many, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        eng._eng.sample(lg, params, seen, 0, 0)


class _Recording(Sampler):
    """Host sampler that notes, before each draw, how far its next
    uniform lies from the nearest CDF boundary of the reference
    distribution."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.margins = []

    def __call__(self, logits):
        u = copy.deepcopy(self.rng).random()
        probs = reference_probs(logits, self.previous_ids, self.T,
                                self.penalty, self.top_k, self.top_p)
        cdf = np.cumsum(probs) / probs.sum()
        self.margins.append(float(np.abs(cdf[probs > 0] - u).min()))
        return super().__call__(logits)


def test_batcher_device_sampling_matches_host_path_on_gpu(eng):
    """Tiny preset, two sampled requests of different settings and one
    greedy, six tokens each: the device-sampling batcher equals the
    default batcher on the same engine. Precondition on the seeds: every
    host-path uniform is >= 1e-4 from a CDF boundary, so neither f32
    arithmetic nor run-to-run logit noise can flip a pick and a mismatch
    is a bug."""
    from distributedllm_amd.serving import ContinuousBatcher
    prompts = [[5, 9, 3], [7], [2, 11, 4, 6, 1]]
    settings = [dict(temperature=0.8, repeat_penalty=1.1, seed=42,
                     top_k=40, top_p=0.95),
                dict(temperature=1.2, repeat_penalty=1.3, seed=7),
                None]

    def run(device_sampling, cls):
        bat = ContinuousBatcher(eng, device_sampling=device_sampling)
        samplers = [cls(**s) if s else None for s in settings]
        reqs = [bat.submit(p, 6, sampler=sm)
                for p, sm in zip(prompts, samplers)]
        bat.run_all(max_steps=50)
        torch.cuda.synchronize()
        return [r.out for r in reqs], samplers

    want, host = run(False, _Recording)
    margins = [m for s in host if s is not None for m in s.margins]
    print("host-path u margins: min", min(margins), "n", len(margins))
    assert len(margins) == 12 and min(margins) >= 1e-4
    got, dev = run(True, Sampler)
    assert got == want
    for h, d in zip(host, dev):
        if h is not None:
            assert d.previous_ids == h.previous_ids
