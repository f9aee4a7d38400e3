"""Tensors and golden digests that pin the MFMA tile layouts.

tests/golden/repack_digests.json holds, per case, the sha256 of the
input bytes and of the (data, scales) that `repack_mfma` must produce,
plus wtype and both numels. The digests were recorded from the numpy
repack implementation that lived in engine/slice_engine.py up to the
commit named in the file's `parent_commit`, which the torch
implementation matched bit for bit there; that numpy copy is gone, the
digests are what remains of it as an oracle.

`cases(group)` rebuilds the inputs; `check` compares one repack result
with its golden entry. A drifted builder (input digest mismatch) is a
failure, never a skip: it means the fixture no longer tests anything.
"""
import functools
import hashlib
import json
from pathlib import Path

import numpy as np

from distributedllm_amd.formats import ggml, kquants, q4, synthetic

GOLDEN = Path(__file__).resolve().parent / "golden" / "repack_digests.json"

F = ggml
_CLASSIC = (F.FTYPE_MOSTLY_Q4_0, F.FTYPE_MOSTLY_Q4_1, F.FTYPE_MOSTLY_Q5_0,
            F.FTYPE_MOSTLY_Q5_1, F.FTYPE_MOSTLY_Q8_0, F.FTYPE_MOSTLY_F16)
_KQUANT = (F.FTYPE_MOSTLY_Q2_K, F.FTYPE_MOSTLY_Q3_K_M, F.FTYPE_MOSTLY_Q4_K_M,
           F.FTYPE_MOSTLY_Q5_K_M, F.FTYPE_MOSTLY_Q6_K)

# group -> [(preset, seed, ftypes, tensor-name stems)]
_MODEL_GROUPS = {
    "q4": [("small", 3, _CLASSIC[0:2], ("attention.wq",))],
    "byte": [("small", 5, _CLASSIC[2:5], ("attention.wq",))],
    "f16": [("small", 6, _CLASSIC[5:6], ("feed_forward.w1",))],
    "kquant": [("small_k", 8, _KQUANT,
                ("attention.wq", "feed_forward.w1"))],
    # K-blocks padded to the load group of 4: E=64 (nb=2), E=96 (nb=3)
    "padded": [("tiny", 0, _CLASSIC, ("attention.wq",)),
               ("tiny_oddhead", 0, _CLASSIC, ("attention.wq",))],
}
GROUPS = tuple(_MODEL_GROUPS) + ("edge",)


@functools.lru_cache(maxsize=None)
def _model(preset, seed, ftype):
    return synthetic.build_model(preset, seed=seed, ftype=ftype)


def _edge_cases():
    """Degenerate rows (all-zero, subnormal amax, near f16 max)."""
    rows, cols = 16, 512
    rng = np.random.default_rng(12)
    w = (rng.standard_normal((rows, cols)) * 0.02).astype(np.float32)
    w[0, :] = 0.0
    w[3, :256] = 1e-42
    w[4, :] = 3.0e4
    for gt, quant in [(F.GGML_TYPE_Q5_0, q4.quantize_q5_0),
                      (F.GGML_TYPE_Q8_0, q4.quantize_q8_0),
                      (F.GGML_TYPE_Q4_K, kquants.quantize_q4_K),
                      (F.GGML_TYPE_Q6_K, kquants.quantize_q6_K)]:
        yield (f"edge/{F.TYPE_NAMES[gt]}",
               F.GGMLTensor(name="e", ne=(cols, rows), gtype=gt,
                            raw=quant(w).tobytes()))


def cases(group):
    """[(case id, GGMLTensor)] of one group, in a fixed order."""
    if group == "edge":
        return list(_edge_cases())
    out = []
    for preset, seed, ftypes, stems in _MODEL_GROUPS[group]:
        for ft in ftypes:
            f = _model(preset, seed, ft)
            for stem in stems:
                t = next(x for x in f.tensors
                         if x.name.endswith(stem + ".weight"))
                out.append((f"{preset}-s{seed}/{F.TYPE_NAMES[t.gtype]}/"
                            f"{stem}", t))
    return out


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def digest(t, mat):
    """The golden record of one (input tensor, repack result)."""
    data, scales, wtype = mat
    return {
        "input_sha256": _sha(bytes(t.raw)),
        "data_sha256": _sha(data.cpu().contiguous().numpy().tobytes()),
        "scales_sha256": _sha(scales.cpu().contiguous().numpy().tobytes()),
        "wtype": int(wtype),
        "data_numel": data.numel(),
        "scales_numel": scales.numel(),
    }


@functools.lru_cache(maxsize=None)
def golden():
    return json.loads(GOLDEN.read_text())["cases"]


def check(case_id, t, mat):
    want = golden()[case_id]
    got = digest(t, mat)
    assert got["input_sha256"] == want["input_sha256"], (
        f"{case_id}: the test-tensor builder drifted (input bytes differ "
        "from the recorded ones); the golden digests no longer apply")
    for k in ("wtype", "data_numel", "scales_numel", "data_sha256",
              "scales_sha256"):
        assert got[k] == want[k], (case_id, k, got[k], want[k])
