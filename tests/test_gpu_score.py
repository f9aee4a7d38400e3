"""Prompt scoring on the device: `HIPSliceEngine.score` (k_lmhead_score +
k_score_finish) against a float64 reference that shares no code with the
kernels, with the tolerance measured on the route it replaces.

truth   float64 `W . rmsnorm(y)` with W and the norm weight dequantised by
        the formats layer (`to_f32()`), then `score_reference`.
parent  existing code only, same rows: `eng.logits(y, all_logits=True)`
        then `eng.logprobs(..., 1)`.

Both routes run the same GEMM arithmetic (f16 activations, f32
accumulation, the same K split), so their errors against truth are draws
from one distribution:

    |fused - truth| <= 2 * max|parent - truth| + 4 V 2**-24
                       + 1e-5 (1 + |truth|)

for `lp` and for `top_lp`; the last two terms are the derived summation
bound of test_gpu_logprobs.py. The factor 2 is head-room for the maximum
of a few hundred samples; on the MI355X no case needed it (the two maxima
agree to three digits, table in docs/kernels.md). `top_id`: with g = twice the largest
|parent logit - truth logit| of the row, the reported token's truth logit
is within g of the row maximum, and equals truth's arg-max wherever
truth's top two logits are further apart than g (at least 90 % of the rows
of every case).

y is a real prefill output of the engine. Targets cycle through
vocabulary ids 0 and V-1, one id in each of the RT row sub-tiles of one
block, the row's own arg-max, and -1 / V (lp must be NaN, the top entry
still written)."""
import functools

import numpy as np
import pytest
import torch

from distributedllm_amd.engine.sampler import score_reference
from distributedllm_amd.formats import ggml, slicer, synthetic
from distributedllm_amd.models.llama import PRESETS, RMS_EPS, LlamaPreset

pytestmark = pytest.mark.gpu

Q4_0, Q4_1 = ggml.FTYPE_MOSTLY_Q4_0, ggml.FTYPE_MOSTLY_Q4_1
Q8_0, F16 = ggml.FTYPE_MOSTLY_Q8_0, ggml.FTYPE_MOSTLY_F16
Q6_K = ggml.FTYPE_MOSTLY_Q6_K

# one layer, E = 64: V = 32000 is R = 2000 row tiles (RT = 4, P = 500
# partials); V = 16416 is R = 1026, even but no multiple of 4 (RT = 2)
WIDE = LlamaPreset("wide_vocab", 32000, 64, 32, 4, 1)
WIDE2 = LlamaPreset("wide_vocab2", 16416, 64, 32, 4, 1)
MODELS = {"tiny": PRESETS["tiny"], "small_k": PRESETS["small_k"],
          "wide": WIDE, "wide2": WIDE2}

# (model, ftype, T, max_prefill): tiny's T reach a masked partial column
# tile (1, 15, 17), a full group (64), a second group (65) and a last
# group with one live column tile (130); 67 on a max_prefill = 64 engine
# is the Python tiling
CASES = [("tiny", Q4_0, T, None) for T in (1, 15, 17, 64, 65, 130)] + [
    ("tiny", Q4_1, 17, None), ("tiny", Q4_1, 130, None),
    ("tiny", Q8_0, 17, None), ("tiny", Q8_0, 130, None),
    ("tiny", F16, 17, None), ("tiny", F16, 130, None),
    ("small_k", Q6_K, 70, None),
    ("wide", Q4_0, 70, None), ("wide2", Q4_0, 70, None),
    ("tiny", Q4_0, 67, 64)]


@functools.lru_cache(maxsize=None)
def _model(name, ftype):
    return synthetic.build_model(MODELS[name], ftype=ftype, seed=11)


@functools.lru_cache(maxsize=None)
def _engine(name, ftype, max_prefill):
    from distributedllm_amd.engine import HIPSliceEngine
    f = _model(name, ftype)
    hp = f.hparams
    e = HIPSliceEngine(hp, hp.n_layer, 0, n_ctx=192, max_batch=1,
                       max_prefill=max_prefill)
    e.load_layers(f)
    e.attach_extra(slicer.make_extra_layers(f))
    return e


def _rt(V, T):
    from distributedllm_amd import ops
    return int(ops.core().lmhead_score_rt(V, T))


def _prefill(eng, toks):
    n = len(toks)
    t = torch.tensor(toks, dtype=torch.int32, device="cuda")
    pos = torch.arange(n, dtype=torch.int32, device="cuda")
    seq = torch.zeros(n, dtype=torch.int32, device="cuda")
    return eng.forward(eng.embed(t), pos, seq).contiguous()


def _truth_logits(f, y):
    tm = f.tensor_map()
    w = tm["output.weight"].to_f32().astype(np.float64)
    nw = tm["norm.weight"].to_f32().astype(np.float64)
    y = y.astype(np.float64)
    yn = y / np.sqrt((y * y).mean(axis=1, keepdims=True) + RMS_EPS) * nw
    return yn @ w.T


def _targets(V, T, rt, amax):
    """One target per row, cycling through the kinds of the docstring;
    the cycle starts at T so that short cases differ."""
    blk = 1 if V >= 32 * rt else 0          # second block if there is one
    kinds = [0, V - 1] + [blk * 16 * rt + s * 16 + 5 for s in range(rt)] + \
        ["amax", -1, V]
    out = []
    for t in range(T):
        k = kinds[(t + T) % len(kinds)]
        out.append(int(amax[t]) if k == "amax" else k)
    return out


@functools.lru_cache(maxsize=None)
def _case(name, ftype, T, max_prefill):
    """Everything a case needs, computed once: y, truth, the parent
    route's results and the fused route's."""
    eng = _engine(name, ftype, max_prefill)
    f = _model(name, ftype)
    V = f.hparams.n_vocab
    rng = np.random.default_rng(1000 * T + V)
    y = _prefill(eng, rng.integers(0, V, T).tolist())
    truth = _truth_logits(f, y.cpu().numpy())
    rt = _rt(V, min(T, int(eng._eng.max_prefill)))
    tg = _targets(V, T, rt, truth.argmax(axis=1))
    t_lp, t_id, t_tlp = score_reference(truth, tg)
    # parent route (out-of-range targets scored as id 0, then masked)
    lg = eng.logits(y, all_logits=True)
    ok = np.array([0 <= i < V for i in tg])
    ids = torch.tensor([i if o else 0 for i, o in zip(tg, ok)],
                       dtype=torch.int32, device="cuda")
    p_lp, p_id, p_tlp = eng.logprobs(lg, list(range(T)), ids, 1)
    lp, top_id, top_lp = eng.score(y, tg)
    torch.cuda.synchronize()
    return dict(eng=eng, V=V, T=T, rt=rt, y=y, tg=tg, ok=ok, truth=truth,
                t_lp=t_lp, t_id=t_id, t_tlp=t_tlp,
                lg=lg.cpu().numpy().astype(np.float64),
                p_lp=p_lp.cpu().numpy().astype(np.float64),
                p_tlp=p_tlp[:, 0].cpu().numpy().astype(np.float64),
                lp=lp.cpu().numpy(), top_id=top_id.cpu().numpy(),
                top_lp=top_lp.cpu().numpy())


def _ids(case):
    name, ftype, T, mp = case
    return f"{name}-ftype{ftype}-T{T}" + (f"-mp{mp}" if mp else "")


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_lp_and_top_lp_within_the_parent_routes_error(case):
    c = _case(*case)
    V, ok = c["V"], c["ok"]
    assert c["lp"].dtype == np.float32 and c["lp"].shape == (c["T"],)
    assert c["top_lp"].dtype == np.float32 and c["top_id"].dtype == np.int32
    # -1 and V: NaN lp, the top entry still written
    assert np.array_equal(np.isnan(c["lp"]), ~ok)
    assert np.isfinite(c["top_lp"]).all()
    assert ((c["top_id"] >= 0) & (c["top_id"] < V)).all()
    worst = 0.0
    for what, got, par, ref, m in (
            ("lp", c["lp"], c["p_lp"], c["t_lp"], ok),
            ("top_lp", c["top_lp"], c["p_tlp"], c["t_tlp"],
             np.ones_like(ok))):
        if not m.any():
            continue
        e_par = float(np.abs(par[m] - ref[m]).max())
        err = np.abs(got[m].astype(np.float64) - ref[m])
        e_fused = float(err.max())
        bound = 2 * e_par + 4 * V * 2.0 ** -24 + 1e-5 * (1 + np.abs(ref[m]))
        one = 1 * e_par + 4 * V * 2.0 ** -24 + 1e-5 * (1 + np.abs(ref[m]))
        print(f"{_ids(case)} RT={c['rt']} {what}: max|fused-truth|="
              f"{e_fused:.3g} max|parent-truth|={e_par:.3g} "
              f"needs-factor-2={bool((err > one).any())}")
        worst = max(worst, float((err / bound).max()))
    assert worst <= 1.0


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_top_id(case):
    c = _case(*case)
    truth = c["truth"]
    rows = np.arange(c["T"])
    g = 2 * np.abs(c["lg"] - truth).max(axis=1)
    top2 = np.sort(truth, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > g
    assert clear.mean() >= 0.9
    assert (truth[rows, c["top_id"]] >= truth.max(axis=1) - g).all()
    assert np.array_equal(c["top_id"][clear], c["t_id"][clear])


def test_every_instantiated_rt_is_covered():
    rts = {_case(*case)["rt"] for case in CASES}
    assert rts == {1, 2, 4}
    assert _rt(32000, 70) == 4 and 32000 // (16 * 4) == 500
    assert _rt(16416, 70) == 2 and (16416 // 16) % 4 != 0


@pytest.mark.parametrize("case", [CASES[5], CASES[13], CASES[14]], ids=_ids)
def test_two_calls_are_bit_identical(case):
    c = _case(*case)
    eng, y = c["eng"], c["y"]
    a, b = (eng.logits(y, all_logits=True) for _ in range(2))
    s1, s2 = (eng.score(y, c["tg"]) for _ in range(2))
    torch.cuda.synchronize()
    # E = 64 is one column chunk per token in k_prep_x: a single atomicAdd
    # per sumsq slot, so the side channel does not vary here
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(s1[1], s2[1])
    for u, v in ((s1[0], s2[0]), (s1[2], s2[2])):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_device_targets_and_bad_arguments():
    c = _case(*CASES[2])
    eng, y = c["eng"], c["y"]
    tg = torch.tensor(c["tg"], dtype=torch.int32, device="cuda")
    got = eng.score(y, tg)
    assert np.array_equal(got[1].cpu().numpy(), c["top_id"])
    assert np.allclose(got[0].cpu().numpy(), c["lp"], rtol=0, atol=1e-6,
                       equal_nan=True)
    with pytest.raises(ValueError):
        eng.score(y, c["tg"][:-1])
    with pytest.raises(ValueError):
        eng.score(y[0], c["tg"][:1])
    with pytest.raises(RuntimeError):
        eng._eng.score(y, tg.long())
    with pytest.raises(RuntimeError):
        eng._eng.score(y, tg[:-1].contiguous())
    with pytest.raises(RuntimeError):
        eng._eng.score(y.cpu(), tg)
    torch.cuda.synchronize()


def test_batcher_echo_on_the_hip_engine():
    """Echo with prefill_chunk = 3: the batcher's records against a direct
    score call over the same chunked prefill, within the bound above."""
    from distributedllm_amd.serving import ContinuousBatcher
    c = _case(*CASES[2])
    eng, V = c["eng"], c["V"]
    f = _model("tiny", Q4_0)
    prompt = np.random.default_rng(5).integers(1, V, 12).tolist()
    bat = ContinuousBatcher(eng, prefill_chunk=3)
    r = bat.submit(prompt, 2, logprobs=1, echo=True)
    bat.run_all(max_steps=20)
    assert r.done and len(r.out) == 2
    assert len(r.prompt_logprobs) == len(r.prompt_top) == len(prompt)
    assert r.prompt_logprobs[0] is None and r.prompt_top[0] is None
    # the same chunks by hand
    ys = []
    for p0 in range(0, len(prompt) - 1, 3):
        chunk = prompt[p0:min(p0 + 3, len(prompt) - 1)]
        n = len(chunk)
        ys.append(eng.forward(
            eng.embed(torch.tensor(chunk, dtype=torch.int32, device="cuda")),
            torch.arange(p0, p0 + n, dtype=torch.int32, device="cuda"),
            torch.zeros(n, dtype=torch.int32, device="cuda")).clone())
    y = torch.cat(ys)
    lp, top_id, top_lp = (t.cpu().numpy() for t in eng.score(y, prompt[1:]))
    truth = _truth_logits(f, y.cpu().numpy())
    t_lp, _, t_tlp = score_reference(truth, prompt[1:])
    lg = eng.logits(y, all_logits=True)
    p_lp, _, _ = eng.logprobs(
        lg, list(range(len(prompt) - 1)),
        torch.tensor(prompt[1:], dtype=torch.int32, device="cuda"), 1)
    e_par = float(np.abs(p_lp.cpu().numpy() - t_lp).max())
    bound = 2 * e_par + 4 * V * 2.0 ** -24 + 1e-5 * (1 + np.abs(t_lp))
    got = np.array(r.prompt_logprobs[1:])
    print(f"batcher echo: max|batcher-direct|={np.abs(got - lp).max():.3g} "
          f"max|parent-truth|={e_par:.3g}")
    assert (np.abs(got - lp) <= bound).all()
    assert [t[0][0] for t in r.prompt_top[1:]] == top_id.tolist()
    assert (np.abs(np.array([t[0][1] for t in r.prompt_top[1:]]) - top_lp)
            <= bound).all()


def test_local_perplexity_hip_against_the_cpu_twin(tmp_path, monkeypatch):
    """The relative tolerance of test_gpu_engine.py's end-to-end parity
    (rel_rms = 8e-3, the tighter of its two figures)."""
    from distributedllm_amd.cli.commands import _local_perplexity
    path = tmp_path / "tiny.bin"
    synthetic.build_model("tiny", seed=0).save(str(path))
    text = "hello world, this is a perplexity probe of some length"
    hip = _local_perplexity(str(path), text)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cpu = _local_perplexity(str(path), text)
    print(f"perplexity: hip={hip!r} cpu={cpu!r}")
    assert abs(hip - cpu) <= 8e-3 * cpu
