"""CPU side of `paged_prefill`: the `--paged-prefill` flag of serve_http and
batch_generate, and the engine factories' refusal without the paged layout.
The kernel is tested in test_gpu_paged_prefill.py."""
import pytest

from distributedllm_amd.cli import build_parser
from distributedllm_amd.engine import TorchSliceEngine, engine_for_slice
from distributedllm_amd.formats import synthetic


@pytest.mark.parametrize("cmd", ["serve_http", "batch_generate"])
def test_flag(cmd):
    argv = [cmd, "m.bin"]
    assert build_parser().parse_args(argv).paged_prefill is False
    a = build_parser().parse_args(argv + ["--kv-layout", "paged",
                                          "--paged-prefill"])
    assert a.paged_prefill is True and a.kv_layout == "paged"


def test_needs_paged_layout():
    f = synthetic.build_model("tiny", seed=0)
    with pytest.raises(ValueError, match="paged_prefill"):
        TorchSliceEngine.from_ggml(f, paged_prefill=True)
    with pytest.raises(ValueError, match="paged_prefill"):
        engine_for_slice(f, 32, 2, device="cpu", paged_prefill=True)
    for eng in (TorchSliceEngine.from_ggml(f, kv_layout="paged",
                                           paged_prefill=True),
                engine_for_slice(f, 32, 2, device="cpu", kv_layout="paged",
                                 paged_prefill=True)):
        assert isinstance(eng, TorchSliceEngine)
