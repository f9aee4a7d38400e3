"""CPU side of `kv8_prefix`: the q8 twin serves `prefix=` behind the switch,
the batcher accepts `shared_prefix` on such an engine, and the CLI parsers
take `--kv-dtype q8` with `--shared-prefix-file`. The kernels are tested in
test_gpu_kv8_prefix.py; the default refusals in test_kv8_reference.py."""
import torch

from distributedllm_amd.cli import build_parser
from distributedllm_amd.cli.commands import _wants_kv8_prefix
from distributedllm_amd.engine import TorchSliceEngine
from distributedllm_amd.formats import slicer, synthetic
from distributedllm_amd.serving import ContinuousBatcher

PREFIX = [5, 9, 3, 12, 7, 2]


def _twin(max_batch, **kw):
    f = synthetic.build_model("tiny", seed=0)
    eng = TorchSliceEngine.from_ggml(f, n_ctx=32, max_batch=max_batch,
                                     kv_dtype="q8", **kw)
    eng.attach_extra(slicer.make_extra_layers(f))
    return eng


def test_batcher_tokens_match_the_plain_batcher():
    prompts = [PREFIX + [4, 11, 6, 1, 8, 3, 9], [2, 11, 4, 6, 1]]
    bat = ContinuousBatcher(_twin(3, kv8_prefix=True), shared_prefix=PREFIX)
    reqs = [bat.submit(p, 5) for p in prompts]
    bat.run_all(max_steps=64)
    assert [r._pfx for r in reqs] == [len(PREFIX), 0]
    for r, p in zip(reqs, prompts):
        plain = ContinuousBatcher(_twin(1))
        want = plain.submit(p, 5)
        plain.run_all(max_steps=64)
        assert r.done and r.out == want.out


def test_twin_prefix_equals_own_copy_of_the_prefix():
    """forward(prefix=) against a twin whose sharing slots were prefilled
    with the prefix themselves: the stored rows are equal, so the outputs
    are, exactly."""
    a, b = _twin(3, kv8_prefix=True), _twin(3)
    g = torch.Generator().manual_seed(3)
    E, P = a.hp.n_embd, len(PREFIX)
    i32 = dict(dtype=torch.int32)
    xp = torch.randn(P, E, generator=g) * 0.5
    a.forward(xp.clone(), torch.arange(P, **i32), torch.full((P,), 2, **i32))
    for slot in (0, 2):     # slot 1 does not share
        b.forward(xp.clone(), torch.arange(P, **i32),
                  torch.full((P,), slot, **i32))
    assert torch.equal(a.k_cache[:, 2, :P], b.k_cache[:, 0, :P])
    # slot 0 continues the prefix, slot 1 starts a sequence of its own
    steps = [(torch.tensor([P, P + 1, 0, 1], **i32),
              torch.tensor([0, 0, 1, 1], **i32)),
             (torch.tensor([P + 2, 2], **i32), torch.tensor([0, 1], **i32))]
    for pos, seq in steps:
        x = torch.randn(len(pos), E, generator=g) * 0.5
        pfx = torch.where(seq == 0, P, 0).to(torch.int32)
        got = a.forward(x.clone(), pos, seq, prefix=(2, P, pfx))
        assert torch.equal(got, b.forward(x.clone(), pos, seq))


def test_cli_accepts_both_flags():
    for cmd in ("serve_http", "batch_generate"):
        args = build_parser().parse_args(
            [cmd, "m.bin", "--kv-dtype", "q8", "--shared-prefix-file", "p"])
        assert _wants_kv8_prefix(args)
        for argv in (["--kv-dtype", "q8"], ["--shared-prefix-file", "p"]):
            assert not _wants_kv8_prefix(
                build_parser().parse_args([cmd, "m.bin"] + argv))
