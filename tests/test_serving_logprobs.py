"""Per-token log-probabilities through the serving layers: the
continuous batcher (`submit(..., logprobs=n)`), the HTTP endpoints, and
the same batcher invariants on the HIP engine."""
import json
import math

import numpy as np
import pytest
import torch

from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.engine.sampler import Sampler, logprobs_reference
from distributedllm_amd.engine.tokenizer import Tokenizer
from distributedllm_amd.formats import ggml, slicer, synthetic
from distributedllm_amd.models.llama import PRESETS
from distributedllm_amd.serving import ContinuousBatcher


def _engine(max_batch, n_ctx=32):
    f = synthetic.build_model("tiny", seed=0)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=n_ctx, max_batch=max_batch)
    eng.attach_extra(slicer.make_extra_layers(f))
    return eng


PROMPTS = [[5, 9, 3], [7], [2, 11, 4, 6, 1], [8, 2]]
STEPS = [6, 4, 3, 6]


def _samplers(device_sampling):
    # greedy, two sampled settings, and (device sampling only) a greedy
    # Sampler object, which the batcher serves through argmax
    return [None,
            Sampler(0.8, 1.1, seed=42, top_k=40, top_p=0.95),
            Sampler(1.3, 1.5, seed=7),
            Sampler(greedy=True) if device_sampling else None]


def _aligned(r):
    assert len(r.out_logprobs) == len(r.out_top) == len(r.out)
    assert all(len(t) == r.logprobs for t in r.out_top)
    assert all(v <= 0 for v in r.out_logprobs)
    for top in r.out_top:
        lps = [p for _, p in top]
        assert lps == sorted(lps, reverse=True)


# ------------------------------------------------------------ CPU batcher

@pytest.mark.parametrize("device_sampling", [False, True])
@pytest.mark.parametrize("ask", [(3, 3, 3, 3), (3, None, 0, None),
                                 (None, 8, None, 1)])
def test_tokens_do_not_depend_on_logprobs(device_sampling, ask):
    """Greedy and sampled requests mixed in one batcher (two slots for
    four requests, so one lane step mixes kinds and slots get reused):
    asking for logprobs, by all or by a subset, changes no token."""
    def run(asks):
        bat = ContinuousBatcher(_engine(2), max_slots=2,
                                device_sampling=device_sampling)
        reqs = [bat.submit(p, s, sampler=sm, logprobs=a)
                for p, s, sm, a in zip(PROMPTS, STEPS,
                                       _samplers(device_sampling), asks)]
        bat.run_all(max_steps=100)
        return reqs

    want = run((None,) * 4)
    got = run(ask)
    for w, g, a in zip(want, got, ask):
        assert g.out == w.out and len(g.out) > 0
        assert w.out_logprobs == [] and w.out_top == []
        if a is None:
            assert g.out_logprobs == [] and g.out_top == []
        else:
            assert g.logprobs == a
            _aligned(g)


def test_lengths_stay_aligned_through_eos_cancel_and_slot_reuse():
    plain = ContinuousBatcher(_engine(1))
    full = plain.submit(PROMPTS[0], 6)
    plain.run_all(max_steps=50)
    eos = full.out[2]
    cut = full.out.index(eos) + 1

    bat = ContinuousBatcher(_engine(1), max_slots=1)
    a = bat.submit(PROMPTS[0], 6, eos_id=eos, logprobs=2)   # ends at eos
    b = bat.submit(PROMPTS[2], 9, logprobs=2)               # cancelled
    c = bat.submit(PROMPTS[3], 4, logprobs=5)               # reused slot
    assert len(bat.queue) == 3
    while not a.done:
        bat.step()
    assert a.out == full.out[:cut] and a.out[-1] == eos
    for _ in range(3):
        bat.step()
    assert 0 < len(b.out) < 9 and c.slot == -1 and not c.done
    assert bat.cancel(b)
    bat.run_all(max_steps=50)
    assert c.done and len(c.out) == 4 and b.done and len(b.out) < 9
    for r in (a, b, c):
        _aligned(r)
    # the queued request's values are those of a run of its own
    solo = ContinuousBatcher(_engine(1))
    s = solo.submit(PROMPTS[3], 4, logprobs=5)
    solo.run_all(max_steps=50)
    assert s.out == c.out
    assert np.allclose(s.out_logprobs, c.out_logprobs, atol=1e-4)


def test_chunked_prefill_needs_no_change():
    def run(chunk):
        bat = ContinuousBatcher(_engine(2), prefill_chunk=chunk)
        reqs = [bat.submit(p, s, logprobs=2)
                for p, s in zip(PROMPTS[:2] + [list(range(3, 15))],
                                [5, 5, 4])]
        bat.run_all(max_steps=100)
        return reqs

    for w, g in zip(run(None), run(3)):
        _aligned(g)
        assert g.out == w.out
        assert np.allclose(g.out_logprobs, w.out_logprobs, atol=1e-4)


@pytest.mark.parametrize("spec", [False, True])
def test_greedy_top_entry_is_the_chosen_token(spec):
    """Greedy: the first top entry is the emitted token with the emitted
    value, exactly. With speculation on, the repeating prompt makes the
    drafts accept, so most tokens come from draft rows."""
    prompts = [[7, 7, 7, 7], [5, 9, 3], [4, 8, 2, 4, 8, 2, 4, 8]]
    steps = [12, 8, 10]
    kw = dict(spec_ngram=2, spec_k=4) if spec else {}
    plain = ContinuousBatcher(_engine(3))
    p_reqs = [plain.submit(p, s) for p, s in zip(prompts, steps)]
    plain.run_all(max_steps=100)
    bat = ContinuousBatcher(_engine(3), **kw)
    reqs = [bat.submit(p, s, logprobs=n)
            for p, s, n in zip(prompts, steps, (3, 1, 8))]
    bat.run_all(max_steps=100)
    if spec:
        assert bat.tokens_out > bat.steps_run     # drafts were accepted
    else:
        assert bat.tokens_out >= bat.steps_run
    for r, w in zip(reqs, p_reqs):
        assert r.out == w.out
        _aligned(r)
        for i in range(len(r.out)):
            assert r.out_top[i][0] == (r.out[i], r.out_logprobs[i])
    if spec:
        # and the values are those of the non-speculative run
        base = ContinuousBatcher(_engine(3))
        b_reqs = [base.submit(p, s, logprobs=n)
                  for p, s, n in zip(prompts, steps, (3, 1, 8))]
        base.run_all(max_steps=100)
        for r, b in zip(reqs, b_reqs):
            assert np.allclose(r.out_logprobs, b.out_logprobs, atol=1e-4)
            assert [[t for t, _ in top] for top in r.out_top] == \
                [[t for t, _ in top] for top in b.out_top]


def _solo_logits(prompt_and_out):
    """Last-position logits of a fresh single-sequence forward."""
    eng = _engine(1)
    n = len(prompt_and_out)
    y = eng.forward(eng.embed(torch.tensor(prompt_and_out,
                                           dtype=torch.int32)),
                    torch.arange(n, dtype=torch.int32),
                    torch.zeros(n, dtype=torch.int32))
    return eng.logits(y[-1:].contiguous(), all_logits=True)[0].numpy()


def test_host_sampled_values_match_an_independent_forward():
    """Host-`Sampler` request next to a greedy one: each value equals
    the reference on a recomputed forward of prompt + out[:i]. Both sides
    are f32 forwards of the same CPU engine over different batch
    compositions; 1e-4 absolute is the margin allowed for that (the
    difference printed below measures ~2e-7)."""
    bat = ContinuousBatcher(_engine(2))
    r = bat.submit(PROMPTS[0], 6, sampler=Sampler(0.8, 1.1, seed=42),
                   logprobs=4)
    g = bat.submit(PROMPTS[2], 5, logprobs=0)
    bat.run_all(max_steps=50)
    _aligned(r)
    _aligned(g)
    worst = 0.0
    for q in (r, g):
        for i in range(len(q.out)):
            lg = _solo_logits(q.prompt + q.out[:i])
            lp, ids, tlp = logprobs_reference(lg, q.out[i], q.logprobs)
            worst = max(worst, abs(lp - q.out_logprobs[i]))
            assert [t for t, _ in q.out_top[i]] == ids.tolist()
            if q.logprobs:
                worst = max(worst, float(np.abs(
                    tlp - [p for _, p in q.out_top[i]]).max()))
    print("worst |batched - solo| logprob difference:", worst)
    assert worst <= 1e-4
    # sampler settings do not enter: the value of the sampled token is
    # that of the raw distribution, not the temperature-scaled one
    lg = _solo_logits(r.prompt)
    assert abs(r.out_logprobs[0] -
               logprobs_reference(lg, r.out[0], 0)[0]) <= 1e-4


def test_host_sampled_requests_add_no_device_launch(monkeypatch):
    eng = _engine(2)
    calls = []
    orig = eng.logprobs
    monkeypatch.setattr(eng, "logprobs",
                        lambda *a, **k: calls.append(1) or orig(*a, **k))
    bat = ContinuousBatcher(eng)
    r = bat.submit(PROMPTS[0], 4, sampler=Sampler(0.8, 1.1, seed=1),
                   logprobs=2)
    bat.run_all(max_steps=50)
    _aligned(r)
    assert calls == []
    # nobody asks: no launch either; a greedy asker: one per step
    bat.submit(PROMPTS[0], 4)
    bat.run_all(max_steps=50)
    assert calls == []
    bat.submit(PROMPTS[0], 4, logprobs=0)
    bat.run_all(max_steps=50)
    assert len(calls) == 4


def test_submit_validation():
    bat = ContinuousBatcher(_engine(1))
    for bad in (-1, 9, 99, 2.0, "3", True):
        with pytest.raises(ValueError):
            bat.submit(PROMPTS[0], 4, logprobs=bad)
    assert not bat.queue
    for ok in (None, 0, 8):
        assert bat.submit(PROMPTS[0], 2, logprobs=ok).logprobs == ok


def test_engine_without_logprobs_is_rejected():
    class _NoLogprobs:
        max_batch = 2
        n_ctx = 32
        device = "cpu"

    bat = ContinuousBatcher(_NoLogprobs())
    with pytest.raises(ValueError):
        bat.submit(PROMPTS[0], 4, logprobs=0)
    assert not bat.queue
    bat.submit(PROMPTS[0], 4)        # the default path needs none


# ------------------------------------------------------------------- HTTP

@pytest.fixture()
def client():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from distributedllm_amd.serving import build_http_app
    f = synthetic.build_model("tiny", seed=0)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=64, max_batch=2)
    eng.attach_extra(slicer.make_extra_layers(f))
    app, worker = build_http_app(ContinuousBatcher(eng),
                                 Tokenizer(f.vocab))
    with TestClient(app) as c:
        yield c
    worker.stop()


def test_generate_without_the_field_is_unchanged(client):
    r = client.post("/generate", json={"prompt": "hello", "num_tokens": 5})
    assert r.status_code == 200
    assert sorted(r.json()) == ["text", "tokens"]
    r2 = client.post("/generate", json={"prompt": "hello", "num_tokens": 5,
                                        "logprobs": None})
    assert r2.content == r.content


def test_generate_with_the_field_has_aligned_arrays(client):
    base = client.post("/generate",
                       json={"prompt": "hello", "num_tokens": 5}).json()
    out = client.post("/generate", json={"prompt": "hello", "num_tokens": 5,
                                         "logprobs": 3}).json()
    assert out["tokens"] == base["tokens"] and out["text"] == base["text"]
    lp = out["logprobs"]
    assert sorted(lp) == ["token_logprobs", "top_logprobs"]
    assert len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == 5
    for tok, v, top in zip(out["tokens"], lp["token_logprobs"],
                           lp["top_logprobs"]):
        assert v <= 0 and len(top) == 3
        assert sorted(top[0]) == ["id", "logprob", "token"]
        assert top[0]["id"] == tok and top[0]["logprob"] == v   # greedy
        assert isinstance(top[0]["token"], str)
    zero = client.post("/generate", json={"prompt": "hello", "num_tokens": 5,
                                          "logprobs": 0}).json()["logprobs"]
    assert zero["top_logprobs"] == [[]] * 5
    assert zero["token_logprobs"] == lp["token_logprobs"]


def test_arrays_are_trimmed_at_a_stop_string(client):
    full = client.post("/generate", json={"prompt": "hello", "num_tokens": 12,
                                          "logprobs": 1}).json()
    mid = len(full["text"]) // 2
    stop = full["text"][mid:mid + 2]
    assert stop and stop in full["text"]
    r = client.post("/generate", json={"prompt": "hello", "num_tokens": 12,
                                       "stop": [stop], "logprobs": 1}).json()
    n = len(r["tokens"])
    assert n < 12 and stop not in r["text"]
    assert len(r["logprobs"]["token_logprobs"]) == n
    assert len(r["logprobs"]["top_logprobs"]) == n
    assert r["logprobs"]["token_logprobs"] == \
        full["logprobs"]["token_logprobs"][:n]


def test_v1_completions_logprobs(client):
    body = {"prompt": "hello", "max_tokens": 6}
    none = client.post("/v1/completions", json=body).json()
    assert none["choices"][0]["logprobs"] is None
    out = client.post("/v1/completions", json={**body, "logprobs": 2}).json()
    ch = out["choices"][0]
    assert ch["text"] == none["choices"][0]["text"]
    lp = ch["logprobs"]
    assert sorted(lp) == ["text_offset", "token_logprobs", "tokens",
                          "top_logprobs"]
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == \
        len(lp["top_logprobs"]) == len(lp["text_offset"]) == 6
    assert "".join(lp["tokens"]) == ch["text"]
    assert lp["text_offset"][0] == 0
    assert lp["text_offset"] == sorted(lp["text_offset"])
    for piece, v, top in zip(lp["tokens"], lp["token_logprobs"],
                             lp["top_logprobs"]):
        assert v <= 0
        assert isinstance(top, dict) and 1 <= len(top) <= 2
        assert all(x <= 0 for x in top.values())
        assert top[piece] == v                    # greedy: the best entry
    r = client.post("/v1/completions", json={**body, "logprobs": 99})
    assert r.status_code == 422
    r = client.post("/v1/completions", json={**body, "logprobs": "2"})
    assert r.status_code == 400


def test_stream_events_carry_logprob(client):
    want = client.post("/generate", json={"prompt": "hello", "num_tokens": 5,
                                          "logprobs": 2}).json()

    def stream(body):
        events = []
        with client.stream("POST", "/generate_stream", json=body) as r:
            assert r.status_code == 200
            kind = None
            for line in r.iter_lines():
                if line.startswith("event:"):
                    kind = line.split(":", 1)[1].strip()
                elif line.startswith("data:"):
                    if kind != "done":
                        events.append(json.loads(line.split(":", 1)[1]))
                    kind = None
        return events

    ev = stream({"prompt": "hello", "num_tokens": 5, "logprobs": 2})
    assert [e["token"] for e in ev] == want["tokens"]
    assert [e["logprob"] for e in ev] == want["logprobs"]["token_logprobs"]
    assert [e["top_logprobs"] for e in ev] == \
        want["logprobs"]["top_logprobs"]
    ev = stream({"prompt": "hello", "num_tokens": 5, "logprobs": 0})
    assert all("logprob" in e and "top_logprobs" not in e for e in ev)
    ev = stream({"prompt": "hello", "num_tokens": 5})
    assert all(sorted(e) == ["piece", "token"] for e in ev)


def test_out_of_range_logprobs_is_422(client):
    for path in ("/generate", "/generate_stream"):
        for bad in (99, -1):
            r = client.post(path, json={"prompt": "hello", "num_tokens": 3,
                                        "logprobs": bad})
            assert r.status_code == 422, (path, bad)
    assert client.get("/health").json()["pending"] == 0


def test_minus_inf_serialises_as_null():
    from distributedllm_amd.serving.http import _json_lp
    assert _json_lp(-math.inf) is None and _json_lp(math.nan) is None
    assert _json_lp(np.float32(-1.5)) == -1.5
    assert json.dumps({"v": _json_lp(-math.inf)}) == '{"v": null}'


# -------------------------------------------------------------------- GPU

def _kernel_bound(V, ref):
    # tests/test_gpu_logprobs.py derives it
    return 4 * V * 2.0 ** -24 + 1e-5 * (1 + np.abs(ref))


@pytest.mark.gpu
def test_batcher_invariants_on_the_hip_engine():
    """Two lanes, device sampling, logprobs on a subset of a mixed batch
    under slot pressure: tokens equal the run with logprobs off; a greedy
    request's first top entry is its token; and every recorded value is
    within the kernel's bound of the reference on the very logits row the
    step used (engine.logits of each lane is wrapped to keep them)."""
    from distributedllm_amd.engine import HIPSliceEngine
    hp = PRESETS["tiny"].hparams(ggml.FTYPE_MOSTLY_Q4_0)
    V = hp.n_vocab
    prompts = PROMPTS + [[4, 8, 2, 4, 8, 2], [9]]
    steps = STEPS + [7, 5]
    asks = (3, 8, None, 0, 5, None)

    def samplers():
        return [None, Sampler(0.8, 1.1, seed=42, top_k=40, top_p=0.95),
                Sampler(1.3, 1.5, seed=7), Sampler(greedy=True), None,
                Sampler(1.0, 1.2, seed=5)]

    def batcher():
        eng = HIPSliceEngine.random(hp, n_layers=hp.n_layer, n_ctx=64,
                                    max_batch=2, seed=0)
        lanes = [eng, eng.clone_shared()]
        return ContinuousBatcher(eng, engines=lanes, device_sampling=True)

    plain = batcher()
    want = [plain.submit(p, s, sampler=sm)
            for p, s, sm in zip(prompts, steps, samplers())]
    plain.run_all(max_steps=100)
    torch.cuda.synchronize()

    bat = batcher()
    assert bat.n_slots == 4 and len(bat.lanes) == 2
    lgs, advs = [], []
    for e in bat.lanes:
        def logits(x, all_logits=False, _orig=e.logits):
            lg = _orig(x, all_logits)
            lgs.append(lg)
            return lg
        e.logits = logits
    orig_advance = bat._advance

    def advance(reqs, drafts, *a, **k):
        advs.append([(r, len(r.out)) for r in reqs])
        assert not any(drafts)
        return orig_advance(reqs, drafts, *a, **k)
    bat._advance = advance

    got = [bat.submit(p, s, sampler=sm, logprobs=a)
           for p, s, sm, a in zip(prompts, steps, samplers(), asks)]
    worst, n_checked, n_steps = 0.0, 0, 0
    while bat.pending:
        del lgs[:], advs[:]
        bat.step()
        n_steps += 1
        assert n_steps < 100 and len(lgs) == len(advs)
        for lg, lane in zip(lgs, advs):
            lg = lg.float().cpu().numpy()
            assert lg.shape[0] == len(lane)
            for row, (r, before) in enumerate(lane):
                if r.logprobs is None:
                    continue
                assert len(r.out) == before + 1
                lp, ids, tlp = logprobs_reference(lg[row], r.out[before],
                                                  r.logprobs)
                assert [t for t, _ in r.out_top[before]] == ids.tolist()
                g = np.array([r.out_logprobs[before]] +
                             [p for _, p in r.out_top[before]])
                w = np.concatenate([[lp], tlp])
                worst = max(worst, float(
                    (np.abs(g - w) / _kernel_bound(V, w)).max()))
                n_checked += 1
    torch.cuda.synchronize()
    print(f"{n_checked} tokens checked, worst error / bound = {worst:.3g}")
    assert n_checked == sum(s for s, a in zip(steps, asks) if a is not None)
    assert worst <= 1.0
    for w, g, a in zip(want, got, asks):
        assert g.done and g.out == w.out
        if a is None:
            assert g.out_logprobs == [] and g.out_top == []
            continue
        _aligned(g)
        if g.sampler is None or g.sampler.greedy:
            for i in range(len(g.out)):
                if a:
                    assert g.out_top[i][0] == (g.out[i], g.out_logprobs[i])
