"""Native C++ tooling: byte-compatibility with the Python formats layer.

The reference ships C++ `slice_model` and a vendored `quantize` binary
(SURVEY §2.2 N2/N4); ours live in tools/ and must produce files that are
byte-identical to the Python slicer/codec — the Python side is the tested
canon, the C++ side must match it exactly.
"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from distributedllm_amd.formats import ggml, q4, slicer, synthetic

TOOLS = Path(__file__).resolve().parent.parent / "tools"


@pytest.fixture(scope="module")
def bins(tmp_path_factory):
    subprocess.run(["make", "-C", str(TOOLS)], check=True,
                   capture_output=True)
    return TOOLS / "bin"


@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("native")
    f = synthetic.build_model("tiny", ftype=ggml.FTYPE_MOSTLY_F16, seed=7)
    path = d / "model_f16.bin"
    f.save(str(path))
    return f, path


def test_slice_model_matches_python(bins, model_file, tmp_path):
    f, path = model_file
    out_cpp = tmp_path / "slice_cpp.bin"
    subprocess.run([str(bins / "slice_model"), "slice", str(path), "1", "2",
                    str(out_cpp)], check=True, capture_output=True)
    out_py = tmp_path / "slice_py.bin"
    slicer.make_slice(f, 1, 2).save(str(out_py))
    assert out_cpp.read_bytes() == out_py.read_bytes()


def test_extra_layers_matches_python(bins, model_file, tmp_path):
    f, path = model_file
    out_cpp = tmp_path / "extra_cpp.bin"
    subprocess.run([str(bins / "slice_model"), "extra_layers", str(path),
                    str(out_cpp)], check=True, capture_output=True)
    out_py = tmp_path / "extra_py.bin"
    slicer.make_extra_layers(f).save(str(out_py))
    assert out_cpp.read_bytes() == out_py.read_bytes()


def test_sliced_file_loads_and_runs(bins, model_file, tmp_path):
    """A C++-produced slice loads through the normal engine path."""
    _, path = model_file
    out = tmp_path / "s.bin"
    subprocess.run([str(bins / "slice_model"), "slice", str(path), "0", "1",
                    str(out)], check=True, capture_output=True)
    sf = ggml.GGMLFile.load(str(out), extended=True)
    assert sf.hparams.first_layer == 0
    assert sf.hparams.n_layer == 2
    from distributedllm_amd.engine import TorchSliceEngine
    import torch
    eng = TorchSliceEngine.from_ggml(sf, n_ctx=16, max_batch=1)
    x = torch.randn(2, sf.hparams.n_embd)
    y = eng.forward(x, torch.tensor([0, 1], dtype=torch.int32),
                    torch.zeros(2, dtype=torch.int32))
    assert torch.isfinite(y).all()


QUANTS = {
    "q4_0": (ggml.FTYPE_MOSTLY_Q4_0, q4.quantize_q4_0),
    "q4_1": (ggml.FTYPE_MOSTLY_Q4_1, q4.quantize_q4_1),
    "q5_0": (ggml.FTYPE_MOSTLY_Q5_0, q4.quantize_q5_0),
    "q5_1": (ggml.FTYPE_MOSTLY_Q5_1, q4.quantize_q5_1),
    "q8_0": (ggml.FTYPE_MOSTLY_Q8_0, q4.quantize_q8_0),
}


@pytest.mark.parametrize("target", list(QUANTS))
def test_quantize_matches_python_codec(bins, model_file, tmp_path, target):
    f, path = model_file
    out_cpp = tmp_path / f"model_{target}.bin"
    subprocess.run([str(bins / "quantize"), str(path), str(out_cpp), target],
                   check=True, capture_output=True)
    got = ggml.GGMLFile.load(str(out_cpp), extended=False)
    ftype, quant = QUANTS[target]
    assert got.hparams.ftype == ftype
    for t in f.tensors:
        g = got.tensor_map()[t.name]
        if len(t.ne) == 1:
            assert g.raw == t.raw  # 1-D stays f32
            continue
        want = quant(t.to_f32()).tobytes()
        assert g.raw == want, f"{t.name}: q4 bytes differ from Python codec"


KQUANTS = {
    "q2_K": (ggml.FTYPE_MOSTLY_Q2_K, "q2_K"),
    "q3_K": (ggml.FTYPE_MOSTLY_Q3_K_M, "q3_K"),
    "q4_K": (ggml.FTYPE_MOSTLY_Q4_K_M, "q4_K"),
    "q5_K": (ggml.FTYPE_MOSTLY_Q5_K_M, "q5_K"),
    "q6_K": (ggml.FTYPE_MOSTLY_Q6_K, "q6_K"),
}


@pytest.fixture(scope="module")
def model_file_k(tmp_path_factory):
    """f16 model whose E and F are multiples of QK_K=256 (small_k)."""
    d = tmp_path_factory.mktemp("native_k")
    f = synthetic.build_model("small_k", ftype=ggml.FTYPE_MOSTLY_F16, seed=9)
    path = d / "model_k_f16.bin"
    f.save(str(path))
    return f, path


@pytest.mark.parametrize("target", list(KQUANTS))
def test_quantize_kquant_matches_python_codec(bins, model_file_k, tmp_path,
                                              target):
    from distributedllm_amd.formats import kquants
    f, path = model_file_k
    out_cpp = tmp_path / f"model_{target}.bin"
    subprocess.run([str(bins / "quantize"), str(path), str(out_cpp), target],
                   check=True, capture_output=True)
    got = ggml.GGMLFile.load(str(out_cpp), extended=False)
    ftype, name = KQUANTS[target]
    assert got.hparams.ftype == ftype
    _, quant, _ = kquants.CODECS[name]
    for t in f.tensors:
        g = got.tensor_map()[t.name]
        if len(t.ne) == 1:
            assert g.raw == t.raw
            continue
        want = quant(t.to_f32().reshape(-1, t.ne[0])).tobytes()
        assert g.raw == want, f"{t.name}: {target} bytes != Python codec"


def test_quantize_kquant_fallback_rows(bins, model_file, tmp_path):
    """Rows not divisible by 256 fall back per-tensor like the Python
    provisioner (q4_K -> q5_0, q6_K -> q8_0); tiny has n_embd=64."""
    f, path = model_file  # tiny: every 2-D tensor has cols % 256 != 0
    for target, fb_quant, fb_gt in [
            ("q4_K", q4.quantize_q5_0, ggml.GGML_TYPE_Q5_0),
            ("q6_K", q4.quantize_q8_0, ggml.GGML_TYPE_Q8_0)]:
        out_cpp = tmp_path / f"model_fb_{target}.bin"
        subprocess.run([str(bins / "quantize"), str(path), str(out_cpp),
                        target], check=True, capture_output=True)
        got = ggml.GGMLFile.load(str(out_cpp), extended=False)
        for t in f.tensors:
            g = got.tensor_map()[t.name]
            if len(t.ne) == 1:
                assert g.raw == t.raw
                continue
            assert g.gtype == fb_gt
            assert g.raw == fb_quant(t.to_f32()).tobytes()


def test_cpp_kquant_dequant_roundtrip(bins, model_file_k, tmp_path):
    """C++ to_f32 of a k-quant file: requantizing q4_K -> q8_0 through
    the native tool matches Python dequant -> Python q8_0."""
    from distributedllm_amd.formats import kquants
    f, path = model_file_k
    kfile = tmp_path / "m_q4K.bin"
    subprocess.run([str(bins / "quantize"), str(path), str(kfile), "q4_K"],
                   check=True, capture_output=True)
    out = tmp_path / "m_q8.bin"
    subprocess.run([str(bins / "quantize"), str(kfile), str(out), "q8_0"],
                   check=True, capture_output=True)
    got = ggml.GGMLFile.load(str(out), extended=False)
    kf = ggml.GGMLFile.load(str(kfile), extended=False)
    for t in kf.tensors:
        g = got.tensor_map()[t.name]
        if len(t.ne) == 1:
            continue
        deq = kquants.dequantize_q4_K(
            np.frombuffer(t.raw, dtype=np.uint8).reshape(t.shape_rows_cols[0], -1),
            t.ne[0]).astype(np.float32)
        assert g.raw == q4.quantize_q8_0(deq).tobytes()


def test_quantize_edge_case_blocks_match_python(bins, tmp_path):
    """Degenerate block contents (all-zero, constant, subnormal-amax,
    near-f16-max) must produce identical bytes from the C++ tool and the
    Python codecs — these hit the safe_inv/zero-scale paths."""
    from distributedllm_amd.formats import kquants, synthetic
    rows, cols = 16, 512          # k-quant compatible (cols % 256 == 0)
    rng = np.random.default_rng(11)
    w = (rng.standard_normal((rows, cols)) * 0.02).astype(np.float32)
    w[0, :] = 0.0                               # all-zero rows
    w[1, :] = 1.0                               # constant row
    w[2, :] = -1.0
    w[3, :256] = 1e-42                          # subnormal amax
    w[4, :] = 3.0e4                             # near f16 max after /q
    w[5, ::2] = -2.5e4
    w[6, :32] = 0.0                             # zero block inside a row
    f = synthetic.build_model("tiny", ftype=ggml.FTYPE_MOSTLY_F16, seed=1)
    t = ggml.GGMLTensor.from_f32("edge.weight", w, ggml.GGML_TYPE_F16)
    f.tensors.append(t)
    path = tmp_path / "edge_f16.bin"
    f.save(str(path))
    w = w.astype(np.float16).astype(np.float32)  # what the file stores
    classic = {"q4_0": q4.quantize_q4_0, "q4_1": q4.quantize_q4_1,
               "q5_0": q4.quantize_q5_0, "q5_1": q4.quantize_q5_1,
               "q8_0": q4.quantize_q8_0}
    for target, quant in classic.items():
        out = tmp_path / f"edge_{target}.bin"
        subprocess.run([str(bins / "quantize"), str(path), str(out),
                        target], check=True, capture_output=True)
        got = ggml.GGMLFile.load(str(out), extended=False)
        g = got.tensor_map()["edge.weight"]
        assert g.raw == quant(w).tobytes(), target
    for target in ("q2_K", "q3_K", "q4_K", "q5_K", "q6_K"):
        out = tmp_path / f"edge_{target}.bin"
        subprocess.run([str(bins / "quantize"), str(path), str(out),
                        target], check=True, capture_output=True)
        got = ggml.GGMLFile.load(str(out), extended=False)
        g = got.tensor_map()["edge.weight"]
        _, quant, _ = kquants.CODECS[target]
        assert g.raw == quant(w).tobytes(), target


def test_torch_repack_edge_case_bits(tmp_path):
    """Same degenerate contents (all-zero row, subnormal amax, near
    f16 max; q5_0, q8_0, q4_K, q6_K) through the repack: tiles, scales
    and wtype equal the golden ones recorded from the numpy repack, bit
    for bit (inf/nan f16 scale patterns from random-byte files are also
    covered by the GPU load bench)."""
    import repack_cases as RC
    from distributedllm_amd.engine.repack import repack_mfma
    cases = RC.cases("edge")
    assert len(cases) == 4
    for case_id, t in cases:
        RC.check(case_id, t, repack_mfma(t, "cpu"))


def test_pmc_summary_tool(tmp_path):
    """tools/pmc_summary.py aggregates rocprofv3 counter CSVs (the
    format used for profiles/r2_pmc_decode.md)."""
    import sys
    d = tmp_path / "pmc" / "run"
    d.mkdir(parents=True)
    csv = d / "1_counter_collection.csv"
    csv.write_text(
        '"Dispatch_Id","Kernel_Name","Counter_Name","Counter_Value"\n'
        '1,"void k_attention<false>(float const*)","SQ_WAVE_CYCLES",100\n'
        '1,"void k_attention<false>(float const*)","FETCH_SIZE",7\n'
        '2,"void k_attention<false>(float const*)","SQ_WAVE_CYCLES",50\n'
        '3,"k_ffn16","SQ_WAVE_CYCLES",30\n')
    out = subprocess.run(
        [sys.executable, str(TOOLS / "pmc_summary.py"),
         str(tmp_path / "pmc")],
        capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split()[:2] == ["kernel", "calls"]
    attn = next(ln for ln in lines if ln.startswith("k_attention"))
    assert attn.split()[1] == "2"              # distinct dispatch ids
    assert "1.500e+02" in attn                 # WAVE_CYCLES summed
    total = next(ln for ln in lines if ln.startswith("TOTAL"))
    assert "1.800e+02" in total
