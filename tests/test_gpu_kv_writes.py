"""What each QKV producer actually puts in the KV cache, at positions up to
4095: layer 0 of the HIP engine's k_cache / v_cache against the torch
twin's, row by row, built from the same model bytes. Layer 0 depends only
on the input, so nothing else is in the comparison.

One case per producer (attention_reference.kv_case): k_qkv_finish,
k_attention<true>, k_qkv16 (unsplit), k_qkv16<…, true> (large-M) and the
legacy f32
launch_qkv_rope_append. Every case writes rows at pos 0, 1, 511, 1607,
1609, 2047, 3000 and 4095 - on both sides of the 512 pi (about 1608 rad)
input domain older ISA manuals give for the hardware sin/cos, where pair 0
(theta = pos) would lose its rotation.

Per-row bounds (attention_reference.tol_kv_rows): V 3 * 2**-11 * rowmax
(f16 store + f16 activation panel), K that plus a 1e-3 angle budget at
pos > 0 (theta is an f32 product, inv_freq comes from two pow
implementations, the multiply by 1/2pi adds about as much again). A lost
rotation is an O(|k|) error; tests/test_attention_reference.py shows these
assertions reject it at every deep position.

Worst error / bound measured on an MI355X: K rows 52 % (k_qkv16<…, true>),
V rows 73 % (k_attention<true>); no producer loses the rotation above
pos 1608.
"""
import numpy as np
import pytest
import torch

import attention_reference as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("producer", R.KV_PRODUCERS)
def test_cache_rows_match_the_torch_engine(producer):
    from distributedllm_amd.engine import HIPSliceEngine
    case = R.kv_case(producer)
    hip = HIPSliceEngine.from_ggml(case.file, n_ctx=case.n_ctx,
                                   max_batch=case.max_batch)
    pos = torch.from_numpy(case.pos).cuda()
    seq = torch.from_numpy(case.seq).cuda()
    y = hip.forward(torch.from_numpy(case.x).cuda(), pos, seq,
                    decode=case.decode)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all().item()
    s, p = seq.long(), pos.long()
    k_got = hip._eng.k_cache[0, s, p].float().cpu().numpy()
    v_got = hip._eng.v_cache[0, s, p].float().cpu().numpy()
    k_ref, v_ref, _ = R.kv_reference(case)
    R.check_kv_rows(case.name, k_got, v_got, k_ref, v_ref, case.pos)
    # nothing but the written rows of layer 0 was touched
    mask = torch.ones(hip._eng.k_cache.shape[1:3], dtype=torch.bool,
                      device="cuda")
    mask[s, p] = False
    assert not hip._eng.k_cache[0][mask].any().item()
    assert not hip._eng.v_cache[0][mask].any().item()
