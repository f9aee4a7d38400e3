"""CPU side of test_gpu_kv8_prefill.py: the edge case at the tile sizes of
`k_attn_kv8_prefill`, the quantised stores both files share, and the check
that these inputs have teeth: a reference with a row dropped, added or
counted twice exceeds the bound the device is held to."""
import functools

import numpy as np
import pytest

import attention_reference as R
from test_kv8_reference import quantize_q8

# jmax + 1 of the six tiles: one row past the 32-row tile, around the 128-row
# pass of four waves, at and past the 256-row double-buffer iteration
EDGE_J = (33, 127, 128, 129, 256, 257)


@functools.lru_cache(maxsize=None)
def edge_case(D, H, Hkv):
    """Six 16-query tiles, each its own sequence, in six of seven slots (the
    seventh stays poisoned)."""
    rng = np.random.default_rng(R._seed("kv8_prefill_edges", D, H, Hkv))
    n_ctx, n_slots = 272, 7
    pos = np.concatenate([J - 16 + np.arange(16) for J in EDGE_J])
    seq = np.repeat(rng.permutation(n_slots)[:len(EDGE_J)], 16)
    Kf, K, Vf, V = R._random_kv(rng, n_slots, n_ctx, Hkv * D)
    q = rng.standard_normal((len(pos), H * D)).astype(np.float32)
    return R._finish("kv8_prefill/edges/D%d_H%d_%d" % (D, H, Hkv), "prefill",
                     D, H, Hkv, n_ctx, n_slots, q, Kf, K, Vf, V, pos, seq,
                     pos)


def dequantized(c):
    """-> (stores [k8, k_scale, v8, v_scale] flat, byte pad 0xFF; K and V of
    the quantised cache, s * q in float64)."""
    st, deq = [], []
    for a in (c.K, c.V):
        q, s = quantize_q8(a, c.D)
        st.append(np.concatenate([(q + 128).astype(np.uint8).reshape(-1),
                                  np.full(16, 255, np.uint8)]))
        st.append(s.reshape(-1))
        deq.append((s.astype(np.float64)[..., None] *
                    q.reshape(s.shape + (c.D,))).reshape(a.shape))
    return st, deq[0], deq[1]


def quantized(c):
    """-> (stores, float64 reference over the dequantised cache, bound)."""
    st, K, V = dequantized(c)
    ref, sabs, vmax = R._attend(c.q, K, V, c.pos, c.seq, c.H, c.Hkv)
    return st, ref, R.tol_prefill(sabs, vmax)


@pytest.mark.parametrize("mutant", [1, 3, 4])
@pytest.mark.parametrize("kind", ["edges", "mixed"])
def test_mutants_exceed_the_bound(kind, mutant):
    c = (edge_case(100, 8, 4) if kind == "edges" else
         R.prefill_case("mixed", 100, 8, 4))
    _, K, V = dequantized(c)
    _, ref, tol = quantized(c)
    bad = R._attend(c.q, K, V, c.pos, c.seq, c.H, c.Hkv, mutant=mutant)[0]
    ratio = np.abs(bad - ref).max() / tol
    print("%s mutant %d (%s): error / bound = %.3g" %
          (c.name, mutant, R.MUTANTS[mutant], ratio))
    assert ratio > 1.0
