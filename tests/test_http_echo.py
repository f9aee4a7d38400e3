"""`echo` on the HTTP endpoints: /generate, /v1/completions (OpenAI
shape, `max_tokens: 0` included), the 422 cases, and a response without
the field that is byte for byte what it was."""
import json

import numpy as np
import pytest

from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.engine.tokenizer import Tokenizer
from distributedllm_amd.formats import slicer, synthetic
from distributedllm_amd.serving import ContinuousBatcher, build_http_app
from distributedllm_amd.serving.http import _json_lp, _top_entries

F = synthetic.build_model("tiny", seed=0)
TOK = Tokenizer(F.vocab)
PROMPT = "hello world of words"


def _batcher():
    eng = TorchSliceEngine.from_ggml(F, n_ctx=64, max_batch=2)
    eng.attach_extra(slicer.make_extra_layers(F))
    return ContinuousBatcher(eng)


@pytest.fixture()
def client():
    from fastapi.testclient import TestClient
    app, worker = build_http_app(_batcher(), TOK)
    with TestClient(app) as c:
        yield c
    worker.stop()


def _scored(n, max_new):
    """The batcher's own records for PROMPT (tested in
    test_serving_echo.py)."""
    bat = _batcher()
    r = bat.submit(TOK.encode(PROMPT, bos=True), max_new, logprobs=n,
                   echo=True)
    bat.run_all(max_steps=100)
    return r


def test_generate_with_echo(client):
    want = _scored(2, 3)
    r = client.post("/generate", json={"prompt": PROMPT, "num_tokens": 3,
                                       "logprobs": 2, "echo": True})
    assert r.status_code == 200
    out = r.json()
    assert out["tokens"] == want.out
    lp = out["logprobs"]
    assert list(lp) == ["token_logprobs", "top_logprobs",
                        "prompt_token_logprobs", "prompt_top_logprobs"]
    n = len(want.prompt)
    assert n > 3 and len(lp["prompt_token_logprobs"]) == n
    assert lp["prompt_token_logprobs"][0] is None
    assert lp["prompt_top_logprobs"][0] is None
    assert np.allclose(lp["prompt_token_logprobs"][1:],
                       want.prompt_logprobs[1:], rtol=0, atol=1e-6)
    for got, top in zip(lp["prompt_top_logprobs"][1:], want.prompt_top[1:]):
        assert [e["id"] for e in got] == [i for i, _ in top]
        assert [e["token"] for e in got] == [TOK.decode_token(i)
                                             for i, _ in top]
    assert np.allclose(lp["token_logprobs"], want.out_logprobs, rtol=0,
                       atol=1e-6)


def test_generate_pure_scoring(client):
    r = client.post("/generate", json={"prompt": PROMPT, "num_tokens": 0,
                                       "logprobs": 0, "echo": True})
    assert r.status_code == 200
    out = r.json()
    assert out["tokens"] == [] and out["text"] == ""
    assert out["logprobs"]["token_logprobs"] == []
    n = len(TOK.encode(PROMPT, bos=True))
    assert len(out["logprobs"]["prompt_token_logprobs"]) == n
    assert out["logprobs"]["prompt_top_logprobs"][1:] == [[]] * (n - 1)


@pytest.mark.parametrize("max_tokens", [0, 2])
def test_v1_completions_echo(client, max_tokens):
    want = _scored(1, max_tokens)
    r = client.post("/v1/completions", json={
        "prompt": PROMPT, "max_tokens": max_tokens, "logprobs": 1,
        "echo": True})
    assert r.status_code == 200
    body = r.json()
    ch = body["choices"][0]
    ids = want.prompt + want.out
    assert ch["text"] == TOK.decode(want.prompt) + TOK.decode(want.out)
    lp = ch["logprobs"]
    assert lp["tokens"] == [TOK.decode_token(t) for t in ids]
    assert len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == \
        len(lp["text_offset"]) == len(ids)
    assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    assert np.allclose(lp["token_logprobs"][1:],
                       want.prompt_logprobs[1:] + want.out_logprobs,
                       rtol=0, atol=1e-6)
    for got, top in zip(lp["top_logprobs"][1:],
                        want.prompt_top[1:] + want.out_top):
        assert list(got) == [TOK.decode_token(top[0][0])]
    offs = lp["text_offset"]
    assert offs == sorted(offs) and offs[0] == 0
    assert all(0 <= o <= len(ch["text"]) for o in offs)
    assert body["usage"]["completion_tokens"] == max_tokens
    assert body["usage"]["prompt_tokens"] == len(want.prompt)
    assert ch["finish_reason"] == "length"


def test_invalid_combinations_are_422(client):
    post = client.post
    # echo needs logprobs
    assert post("/generate", json={"prompt": PROMPT, "num_tokens": 2,
                                   "echo": True}).status_code == 422
    assert post("/v1/completions", json={"prompt": PROMPT, "max_tokens": 2,
                                         "echo": True}).status_code == 422
    # no tokens asked for without echo
    assert post("/generate", json={"prompt": PROMPT, "num_tokens": 0,
                                   "logprobs": 1}).status_code == 422
    assert post("/v1/completions", json={"prompt": PROMPT, "max_tokens": 0,
                                         "logprobs": 1}).status_code == 422
    assert post("/v1/completions", json={"prompt": PROMPT,
                                         "max_tokens": 0}).status_code == 422
    # negative counts stay invalid with echo
    assert post("/generate", json={"prompt": PROMPT, "num_tokens": -1,
                                   "logprobs": 1,
                                   "echo": True}).status_code == 422
    # echo must be a boolean
    assert post("/v1/completions", json={"prompt": PROMPT, "max_tokens": 2,
                                         "logprobs": 1,
                                         "echo": "yes"}).status_code == 422
    assert post("/generate", json={"prompt": PROMPT, "num_tokens": 2,
                                   "logprobs": 1,
                                   "echo": [1]}).status_code == 422
    # streaming does not echo
    assert post("/generate_stream", json={"prompt": PROMPT, "num_tokens": 2,
                                          "logprobs": 1,
                                          "echo": True}).status_code == 422
    assert post("/generate_stream", json={"prompt": PROMPT,
                                          "num_tokens": 2}).status_code == 200
    assert client.get("/health").json()["pending"] == 0


def test_response_without_echo_is_byte_identical(client):
    """Built here from a batcher run of its own, in the key order and the
    JSON rendering the endpoint had before `echo` existed."""
    bat = _batcher()
    req = bat.submit(TOK.encode(PROMPT, bos=True), 4, logprobs=2)
    bat.run_all(max_steps=100)
    want = {"text": TOK.decode(req.out), "tokens": list(req.out),
            "logprobs": {
                "token_logprobs": [_json_lp(v) for v in req.out_logprobs],
                "top_logprobs": [_top_entries(TOK, t)
                                 for t in req.out_top]}}
    raw = json.dumps(want, ensure_ascii=False, allow_nan=False,
                     separators=(",", ":")).encode("utf-8")
    body = {"prompt": PROMPT, "num_tokens": 4, "logprobs": 2}
    a = client.post("/generate", json=body)
    b = client.post("/generate", json=dict(body, echo=False))
    assert a.status_code == 200 and a.content == raw and b.content == raw
    plain = client.post("/generate", json={"prompt": PROMPT,
                                           "num_tokens": 4})
    assert plain.content == json.dumps(
        {"text": want["text"], "tokens": want["tokens"]},
        ensure_ascii=False, separators=(",", ":")).encode("utf-8")
    v1 = client.post("/v1/completions", json={
        "prompt": PROMPT, "max_tokens": 4, "logprobs": 2}).json()
    ch = v1["choices"][0]
    assert ch["text"] == want["text"]
    assert len(ch["logprobs"]["tokens"]) == 4
    assert None not in ch["logprobs"]["top_logprobs"]
