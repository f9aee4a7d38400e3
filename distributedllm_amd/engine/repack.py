"""On-disk tensors -> the MFMA tile layouts the kernels stream.

One torch implementation, device-agnostic: on the GPU only the
compressed bytes cross PCIe and the bit work runs at HBM rate (a numpy
host repack measured 0.2 GB/s on a 30B q4_0 load - BASELINE.md); on the
CPU the same code is what the tests check. The byte-stream formats go
through two stages:

  expand   raw blocks -> (vals u8 [rows, nb, 32], alpha, beta) with
           w = alpha*(u - 128) + beta; alpha/beta are [rows, nb], or
           [rows, nb, 2] for the formats scaled per 16 weights
  pack     (vals, alpha, beta) -> (data, scales, wtype) tiles

q4_0/q4_1 pack their nibbles directly and f16 is a tile transpose.
`detile_mfma` is the inverse of every layout, `random_tiles` draws
weights directly in them. tests/golden/repack_digests.json pins the
exact bytes.

Layouts, R = rows/16 row tiles, nb = cols/32 K-blocks padded to nbp (a
multiple of the 4-block load group; pad blocks carry alpha = beta = 0
and contribute exact zeros):
  q4    data   u32[R][nbp/4][4 ws][16 i][4 kb]: word ws of a block packs
               its 8 weights at bits (j%2)*16 + (j//2)*4 (the order
               a_frag_q4 unpacks into an f16x8 A fragment); one dwordx4
               per lane covers 4 consecutive K-blocks
        scales f16 (alpha, beta)[R][nbp/4][16 i][4 kb]; the kernel
               computes alpha*(n - 8) (q4_0) or alpha*n + beta (q4_1)
  bytes data   u32[R][nbp/4][4 ws][16 i][4 kb][2]: 8 weights per (block,
               ws) in byte order [w0,w2,w1,w3, w4,w6,w5,w7], so the
               kernel's 0x00FF00FF masks yield the (even, odd) f16 pairs
               of the A fragment (a_frag_q8)
        scales W_Q8B as q4; W_Q8B16 [R][nbp/4][2 hp][16 i][4 kb], where
               half-plane hp = ws >> 1 scales weights 16*hp .. 16*hp+15
  f16   data   f16[R][cols/8][16 i][8]
Every allocation ends in one prefetch batch of tail slack (the kernels'
K loop overreads one batch).
"""
from __future__ import annotations

import numpy as np
import torch

from ..formats import ggml
from ..formats import kquants as KQ

# kernels.h WType; the first four equal the ggml type ids
W_F32, W_F16, W_Q4_0, W_Q4_1, W_Q8B, W_Q8B16 = 0, 1, 2, 3, 8, 9

# Tail slack in elements. ops/csrc/engine_ext.cpp kTailSlack* is the other
# side: make_devmat2 refuses any tensor whose numel is not exact.
TAIL_SLACK_Q4 = 256     # int32, q4 data
TAIL_SLACK_Q8 = 512     # int32, byte-stream data
TAIL_SLACK_AB = 128     # f16, (alpha, beta) scales
TAIL_SLACK_F16 = 2048   # f16 tiles

_Q4_GTYPES = (ggml.GGML_TYPE_Q4_0, ggml.GGML_TYPE_Q4_1)
_BYTE_GTYPES = (ggml.GGML_TYPE_Q5_0, ggml.GGML_TYPE_Q5_1,
                ggml.GGML_TYPE_Q8_0)
# k-quants with per-32 affine sub-blocks ride W_Q8B; per-16 formats ride
# W_Q8B16 (two scale planes)
_K32_GTYPES = (ggml.GGML_TYPE_Q4_K, ggml.GGML_TYPE_Q5_K)
_K16_GTYPES = (ggml.GGML_TYPE_Q2_K, ggml.GGML_TYPE_Q3_K,
               ggml.GGML_TYPE_Q6_K)

# bit position of weight j in a q4 word
_Q4_SHIFTS = [(j % 2) * 16 + (j // 2) * 4 for j in range(8)]


def padded_blocks(nb: int) -> int:
    """K-blocks padded to the load group of 4."""
    return (nb + 3) & ~3


def _raw(t: ggml.GGMLTensor, device, dtype=np.uint8) -> torch.Tensor:
    return torch.tensor(np.frombuffer(t.raw, dtype), device=device)


def _f16_field(b: torch.Tensor, lo: int) -> torch.Tensor:
    """The f16 at bytes [lo, lo+2) of every block of b [rows, n, bs]."""
    return (b[:, :, lo:lo + 2].contiguous().view(torch.half)
            .view(b.shape[0], b.shape[1]).float())


# ---- expansion stage ----

def expand_byte_quant(t: ggml.GGMLTensor, device="cpu"):
    """q5_0/q5_1/q8_0 -> (vals, alpha, beta), re-biased for the kernel's
    w = alpha*((1024+u) - 1152) + beta:
      q8_0: u = q + 128   alpha = d, beta = 0
      q5_0: u = q5 + 112  alpha = d, beta = 0   (q5 - 16 exact)
      q5_1: u = q5 + 112  alpha = d, beta = m + 16*d
    """
    rows, cols = t.shape_rows_cols
    nb = cols // 32
    raw = _raw(t, device)
    if t.gtype == ggml.GGML_TYPE_Q8_0:
        a = raw.view(rows, nb, 34)
        alpha = _f16_field(a, 0)
        return a[:, :, 2:] ^ 0x80, alpha, torch.zeros_like(alpha)
    q5_0 = t.gtype == ggml.GGML_TYPE_Q5_0
    assert q5_0 or t.gtype == ggml.GGML_TYPE_Q5_1, t.gtype
    hoff = 2 if q5_0 else 4
    a = raw.view(rows, nb, hoff + 20)
    qs = a[:, :, hoff + 4:]
    qh = a[:, :, hoff:hoff + 4].contiguous().view(torch.int32).view(rows, nb)
    # 5th bits: arithmetic >> keeps bit k at position 0 after & 1
    bits = ((qh.unsqueeze(-1) >>
             torch.arange(32, device=device, dtype=torch.int32)) & 1
            ).to(torch.uint8)
    lo = (qs & 0xF) | (bits[:, :, :16] << 4)
    hi = (qs >> 4) | (bits[:, :, 16:] << 4)
    vals = torch.cat([lo, hi], dim=-1) + 112          # <= 143
    alpha = _f16_field(a, 0)
    beta = (torch.zeros_like(alpha) if q5_0
            else _f16_field(a, 2) + 16.0 * alpha)
    return vals, alpha, beta


def _k4_affine(b: torch.Tensor):
    """q4_K/q5_K super-blocks [rows, nsb, bs] -> (alpha, beta)
    [rows, nsb*8] from d, dmin and the 6-bit (scale, min) pairs packed
    as in kquants._unpack_scales_k4."""
    rows, nsb = b.shape[:2]
    d, dmin = _f16_field(b, 0), _f16_field(b, 2)
    p = b[:, :, 4:16]
    sc = torch.empty(rows, nsb, 8, dtype=torch.uint8, device=b.device)
    mn = torch.empty_like(sc)
    sc[..., 0:4] = p[..., 0:4] & 63
    mn[..., 0:4] = p[..., 4:8] & 63
    sc[..., 4:8] = (p[..., 8:12] & 0xF) | ((p[..., 0:4] >> 6) << 4)
    mn[..., 4:8] = (p[..., 8:12] >> 4) | ((p[..., 4:8] >> 6) << 4)
    alpha = (d.unsqueeze(-1) * sc.float()).reshape(rows, nsb * 8)
    beta = (-(dmin.unsqueeze(-1) * mn.float())).reshape(rows, nsb * 8)
    return alpha, beta


def expand_kquant(t: ggml.GGMLTensor, device="cpu"):
    """q2_K..q6_K super-blocks -> (vals, alpha, beta) per 32-weight
    block; alpha/beta are [rows, nb] for q4_K/q5_K and [rows, nb, 2]
    (16-weight halves) for q2_K/q3_K/q6_K."""
    rows, cols = t.shape_rows_cols
    nsb = cols // KQ.QK_K
    raw = _raw(t, device)
    if t.gtype == ggml.GGML_TYPE_Q4_K:
        b = raw.view(rows, nsb, KQ.Q4_K_BLOCK_BYTES)
        qs = b[:, :, 16:144].reshape(rows, nsb, 4, 32)
        q = torch.empty(rows, nsb, 8, 32, dtype=torch.uint8, device=device)
        q[:, :, 0::2] = qs & 0xF
        q[:, :, 1::2] = qs >> 4
        return ((q + 128).reshape(rows, nsb * 8, 32),) + _k4_affine(b)
    if t.gtype == ggml.GGML_TYPE_Q5_K:
        b = raw.view(rows, nsb, KQ.Q5_K_BLOCK_BYTES)
        qh = b[:, :, 16:48]
        ql = b[:, :, 48:176].reshape(rows, nsb, 4, 32)
        q = torch.empty(rows, nsb, 8, 32, dtype=torch.uint8, device=device)
        for j in range(4):
            q[:, :, 2 * j] = (ql[:, :, j] & 0xF) | \
                (((qh >> (2 * j)) & 1) << 4)
            q[:, :, 2 * j + 1] = (ql[:, :, j] >> 4) | \
                (((qh >> (2 * j + 1)) & 1) << 4)
        return ((q + 128).reshape(rows, nsb * 8, 32),) + _k4_affine(b)
    if t.gtype == ggml.GGML_TYPE_Q6_K:
        b = raw.view(rows, nsb, KQ.Q6_K_BLOCK_BYTES)
        ql = b[:, :, 0:128].reshape(rows, nsb, 2, 2, 32)
        qh = b[:, :, 128:192].reshape(rows, nsb, 2, 32)
        sc = (b[:, :, 192:208].contiguous().view(torch.int8)
              .view(rows, nsb, 16).float())
        d = _f16_field(b, 208)
        q = torch.empty(rows, nsb, 2, 4, 32, dtype=torch.int16,
                        device=device)
        q[:, :, :, 0] = ((ql[:, :, :, 0] & 0xF) |
                         (((qh >> 0) & 3) << 4)).to(torch.int16)
        q[:, :, :, 1] = ((ql[:, :, :, 1] & 0xF) |
                         (((qh >> 2) & 3) << 4)).to(torch.int16)
        q[:, :, :, 2] = ((ql[:, :, :, 0] >> 4) |
                         (((qh >> 4) & 3) << 4)).to(torch.int16)
        q[:, :, :, 3] = ((ql[:, :, :, 1] >> 4) |
                         (((qh >> 6) & 3) << 4)).to(torch.int16)
        # u = (q - 32) + 128
        vals = (q + 96).to(torch.uint8).reshape(rows, nsb * 8, 32)
        alpha = (d.unsqueeze(-1) * sc).reshape(rows, nsb * 8, 2)
        return vals, alpha, torch.zeros_like(alpha)
    if t.gtype == ggml.GGML_TYPE_Q2_K:
        b = raw.view(rows, nsb, KQ.Q2_K_BLOCK_BYTES)
        sc = (b[:, :, 0:16] & 0xF).float()
        mn = (b[:, :, 0:16] >> 4).float()
        qs = b[:, :, 16:80].reshape(rows, nsb, 2, 32)
        d, dmin = _f16_field(b, 80), _f16_field(b, 82)
        q = torch.empty(rows, nsb, 2, 4, 32, dtype=torch.uint8,
                        device=device)
        for j in range(4):
            q[:, :, :, j] = (qs >> (2 * j)) & 3
        vals = (q + 128).reshape(rows, nsb * 8, 32)
        alpha = (d.unsqueeze(-1) * sc).reshape(rows, nsb * 8, 2)
        beta = (-(dmin.unsqueeze(-1) * mn)).reshape(rows, nsb * 8, 2)
        return vals, alpha, beta
    assert t.gtype == ggml.GGML_TYPE_Q3_K, t.gtype
    b = raw.view(rows, nsb, KQ.Q3_K_BLOCK_BYTES)
    hm = b[:, :, 0:32]
    qs = b[:, :, 32:96].reshape(rows, nsb, 2, 32)
    p = b[:, :, 96:108]
    # 6-bit scales, packed as in kquants._unpack_scales_q3
    sc = torch.empty(rows, nsb, 16, dtype=torch.int16, device=device)
    a0, a1, tt = p[..., 0:4], p[..., 4:8], p[..., 8:12]
    sc[..., 0:4] = ((a0 & 0xF) | (((tt >> 0) & 3) << 4)).to(torch.int16)
    sc[..., 4:8] = ((a1 & 0xF) | (((tt >> 2) & 3) << 4)).to(torch.int16)
    sc[..., 8:12] = ((a0 >> 4) | (((tt >> 4) & 3) << 4)).to(torch.int16)
    sc[..., 12:16] = ((a1 >> 4) | (((tt >> 6) & 3) << 4)).to(torch.int16)
    sc = (sc - 32).float()
    d = _f16_field(b, 108)
    q = torch.empty(rows, nsb, 2, 4, 32, dtype=torch.int16, device=device)
    for half in range(2):
        for j in range(4):
            low = ((qs[:, :, half] >> (2 * j)) & 3).to(torch.int16)
            hi = ((hm >> (half * 4 + j)) & 1).to(torch.int16)
            q[:, :, half, j] = low - torch.where(
                hi != 0, torch.zeros_like(hi), torch.full_like(hi, 4))
    vals = (q + 128).to(torch.uint8).reshape(rows, nsb * 8, 32)
    alpha = (d.unsqueeze(-1) * sc).reshape(rows, nsb * 8, 2)
    return vals, alpha, torch.zeros_like(alpha)


# ---- pack stage ----

def _tile_scales(alpha: torch.Tensor, beta: torch.Tensor, R: int,
                 nbp: int) -> torch.Tensor:
    """(alpha, beta) f32 [rows, nb or nbp] (one plane) or [.., 2] (two
    half-planes) -> flat f16 scale tiles, blocks zero-padded to nbp,
    plus tail slack."""
    ab = torch.stack([alpha, beta], dim=-1)
    if ab.shape[1] < nbp:
        pad = ab.new_zeros((ab.shape[0], nbp - ab.shape[1]) + ab.shape[2:])
        ab = torch.cat([ab, pad], dim=1)
    ab = ab.to(torch.float16)
    if alpha.dim() == 2:
        sc = (ab.view(R, 16, nbp // 4, 4, 2)          # [R][i][g4][kb][2]
              .permute(0, 2, 1, 3, 4))                # [R][g4][i][kb][2]
    else:
        sc = (ab.view(R, 16, nbp // 4, 4, 2, 2)       # [R][i][g4][kb][hp][2]
              .permute(0, 2, 4, 1, 3, 5))             # [R][g4][hp][i][kb][2]
    return torch.cat([sc.reshape(-1),
                      torch.zeros(TAIL_SLACK_AB, dtype=torch.float16,
                                  device=ab.device)])


def _pack_bytes(vals: torch.Tensor, alpha: torch.Tensor,
                beta: torch.Tensor):
    """Expansion-stage output -> (data, scales, wtype) byte-stream
    tiles: W_Q8B16 when alpha/beta carry two half-planes, else W_Q8B."""
    rows, nb = vals.shape[:2]
    device = vals.device
    R, nbp = rows // 16, padded_blocks(nb)
    perm = torch.tensor([0, 2, 1, 3, 4, 6, 5, 7], device=device)
    vp = torch.zeros(rows, nbp, 4, 8, dtype=torch.uint8, device=device)
    vp[:, :nb] = vals.reshape(rows, nb, 4, 8)[:, :, :, perm]
    shifts = torch.tensor([0, 8, 16, 24], device=device, dtype=torch.int32)
    # disjoint byte fields -> sum == OR
    q32 = (vp.view(rows, nbp, 4, 2, 4).to(torch.int32) << shifts
           ).sum(dim=-1, dtype=torch.int64).to(torch.int32)
    qs2 = (q32.view(R, 16, nbp // 4, 4, 4, 2)     # [R][i][g4][kb][ws][2]
           .permute(0, 2, 4, 1, 3, 5))            # [R][g4][ws][i][kb][2]
    data = torch.cat([qs2.reshape(-1),
                      torch.zeros(TAIL_SLACK_Q8, dtype=torch.int32,
                                  device=device)])
    return (data, _tile_scales(alpha, beta, R, nbp),
            W_Q8B16 if alpha.dim() == 3 else W_Q8B)


def _repack_q4_tiles(t: ggml.GGMLTensor, device):
    rows, cols = t.shape_rows_cols
    R, nb = rows // 16, cols // 32
    nbp = padded_blocks(nb)
    q4_0 = t.gtype == ggml.GGML_TYPE_Q4_0
    bs = 18 if q4_0 else 20
    a = _raw(t, device).view(rows, nb, bs)
    qs = a[:, :, bs - 16:]
    # weight j sits at nibble j (low) / j+16 (high) of the 16 qs bytes
    n = torch.cat([(qs & 0xF), (qs >> 4)], dim=-1).to(torch.int32)
    n = n.view(rows, nb, 4, 8)                    # [rows][block][ws][j]
    shifts = torch.tensor(_Q4_SHIFTS, device=device, dtype=torch.int32)
    # disjoint 4-bit fields -> sum == OR
    qword = (n << shifts).sum(dim=-1, dtype=torch.int64).to(torch.int32)
    qp = torch.zeros(rows, nbp, 4, dtype=torch.int32, device=device)
    qp[:, :nb] = qword
    qs2 = (qp.view(R, 16, nbp // 4, 4, 4)         # [R][i][g4][kb][ws]
           .permute(0, 2, 4, 1, 3))               # [R][g4][ws][i][kb]
    data = torch.cat([qs2.reshape(-1),
                      torch.zeros(TAIL_SLACK_Q4, dtype=torch.int32,
                                  device=device)])
    alpha = _f16_field(a, 0)
    beta = torch.zeros_like(alpha) if q4_0 else _f16_field(a, 2)
    return data, _tile_scales(alpha, beta, R, nbp), t.gtype


def _repack_f16_tiles(t: ggml.GGMLTensor, device):
    rows, cols = t.shape_rows_cols
    w = _raw(t, device, np.int16)
    tile = w.view(rows // 16, 16, cols // 8, 8).permute(0, 2, 1, 3)
    data = torch.cat([tile.reshape(-1),
                      torch.zeros(TAIL_SLACK_F16, dtype=torch.int16,
                                  device=device)])
    return data, torch.empty(0), W_F16


def repack_mfma(t: ggml.GGMLTensor, device):
    """On-disk tensor -> (data, scales, wtype) in the MFMA tile layout
    of its format (module docstring). f32 stays plain [rows, cols] for
    the legacy scalar path."""
    rows, cols = t.shape_rows_cols
    assert rows % 16 == 0 and cols % 32 == 0, (t.name, rows, cols)
    if t.gtype == ggml.GGML_TYPE_F32:
        a = np.frombuffer(t.raw, np.float32).reshape(rows, cols)
        return torch.from_numpy(a.copy()).to(device), torch.empty(0), W_F32
    if t.gtype == ggml.GGML_TYPE_F16:
        return _repack_f16_tiles(t, device)
    if t.gtype in _Q4_GTYPES:
        return _repack_q4_tiles(t, device)
    if t.gtype in _BYTE_GTYPES:
        return _pack_bytes(*expand_byte_quant(t, device))
    return _pack_bytes(*expand_kquant(t, device))


def detile_mfma(mat, rows: int, cols: int,
                dtype=torch.half) -> torch.Tensor:
    """Inverse of repack_mfma: tiled weights -> plain [rows, cols].
    Test/debug utility, the independent reading of the layouts.

    dtype = torch.half (default): alpha*n + beta computed in f32, then
    rounded to f16 - two roundings. dtype = torch.float64: the same
    expression in float64, not rounded (the products of an f16 scale and
    an 8-bit integer plus an f16 offset are exact there), so a caller can
    apply the single f16 rounding of the kernel's v_pk_fma_f16 itself."""
    assert dtype in (torch.half, torch.float64), dtype
    f = torch.float64 if dtype == torch.float64 else torch.float32
    data, sc, wt = mat
    if wt == W_F16:
        t = data[:rows * cols].view(torch.half)
        return (t.view(rows // 16, cols // 8, 16, 8)
                .permute(0, 2, 1, 3).reshape(rows, cols)).to(dtype)
    R, nbp = rows // 16, padded_blocks(cols // 32)
    if wt == W_Q8B16:
        # [R,g4,hp,i,kb,2]: half-plane hp serves word-spans 2hp, 2hp+1
        ab = (sc[:R * nbp * 64].view(R, nbp // 4, 2, 16, 4, 2).to(f)
              .repeat_interleave(2, dim=2))
    else:
        ab = sc[:R * nbp * 32].view(R, nbp // 4, 1, 16, 4, 2).to(f)
    alpha = ab[..., 0].unsqueeze(-1)              # [R,g4,ws|1,i,kb,1]
    beta = ab[..., 1].unsqueeze(-1)
    if wt in (W_Q4_0, W_Q4_1):
        qw = data[:R * nbp * 64].view(R, nbp // 4, 4, 16, 4)
        shifts = torch.tensor(_Q4_SHIFTS, device=data.device,
                              dtype=torch.int32)
        n = ((qw.unsqueeze(-1) >> shifts) & 0xF).to(f)
        w = alpha * (n - 8.0) if wt == W_Q4_0 else alpha * n + beta
        # [R,g4,ws,i,kb,8] -> [R,i,g4,kb,ws,8] -> [rows, nbp*32]
        w = w.permute(0, 3, 1, 4, 2, 5).reshape(rows, nbp * 32)
        return w[:, :cols].to(dtype)
    assert wt in (W_Q8B, W_Q8B16), wt
    # u32 bytes are [w0,w2,w1,w3]: weight jj sits at byte [0,2,1,3][jj]
    qw = data[:R * nbp * 128].view(R, nbp // 4, 4, 16, 4, 2)
    bshift = torch.tensor([0, 16, 8, 24], device=data.device,
                          dtype=torch.int32)
    u = ((qw.unsqueeze(-1) >> bshift) & 0xFF).to(f)
    w = alpha.unsqueeze(-1) * (u - 128.0) + beta.unsqueeze(-1)
    # [R,g4,ws,i,kb,2,4] -> [R,i,g4,kb,ws,2,4] -> [rows, nbp*32]
    w = w.permute(0, 3, 1, 4, 2, 5, 6).reshape(rows, nbp * 32)
    return w[:, :cols].to(dtype)


def random_tiles(wt: int, rows: int, cols: int, g: torch.Generator):
    """Random weights of ggml type wt directly in the tile layouts, on
    g's device: the same compute and HBM traffic as a real checkpoint.
    Any random bits are valid quant words (the dequant masks them into
    finite f16 values), so the data stream needs no pad handling; pad
    scale blocks are (0, 0) => exact zeros. Draw order per matrix: data,
    then alpha (seeded benchmark weights depend on it)."""
    dev = g.device
    if wt == ggml.GGML_TYPE_F16:
        data = torch.randn(rows * cols + TAIL_SLACK_F16, device=dev,
                           generator=g, dtype=torch.float32) * 0.02
        return (data.to(torch.float16).view(torch.int16), torch.empty(0),
                W_F16)
    if wt not in _Q4_GTYPES + _BYTE_GTYPES + _K32_GTYPES + _K16_GTYPES:
        data = torch.randn(rows, cols, device=dev, generator=g,
                           dtype=torch.float32) * 0.02
        return data.contiguous(), torch.empty(0), wt
    R, nb = rows // 16, cols // 32
    nbp = padded_blocks(nb)
    if wt in _Q4_GTYPES:
        n_data, wtype = R * nbp * 64 + TAIL_SLACK_Q4, wt
    else:
        n_data = R * nbp * 128 + TAIL_SLACK_Q8
        wtype = W_Q8B16 if wt in _K16_GTYPES else W_Q8B
    data = torch.randint(-2**31, 2**31 - 1, (n_data,), dtype=torch.int32,
                         device=dev, generator=g)
    shape = (rows, nbp, 2) if wtype == W_Q8B16 else (rows, nbp)
    alpha = (torch.rand(shape, device=dev, generator=g) * 0.5 + 0.75
             ) * 0.003
    alpha[:, nb:] = 0.0
    beta = (alpha * 0.1
            if wt in (ggml.GGML_TYPE_Q4_1, ggml.GGML_TYPE_Q5_1)
            else torch.zeros_like(alpha))
    return data, _tile_scales(alpha, beta, R, nbp), wtype


# ---- embedding table: legacy SoA layout (row-gather kernel) ----

def _repack_q4(t: ggml.GGMLTensor):
    rows, cols = t.shape_rows_cols
    nb = cols // 32
    if t.gtype == ggml.GGML_TYPE_Q4_0:
        a = np.frombuffer(t.raw, np.uint8).reshape(rows, nb, 18)
        scales = np.ascontiguousarray(a[:, :, :2]).view(np.float16)
        scales = scales.reshape(rows, nb)
        qs = np.ascontiguousarray(a[:, :, 2:]).reshape(rows, nb * 16)
    else:  # q4_1: 20-byte blocks, (d, m) f16 pairs
        a = np.frombuffer(t.raw, np.uint8).reshape(rows, nb, 20)
        scales = np.ascontiguousarray(a[:, :, :4]).view(np.float16)
        scales = scales.reshape(rows, nb * 2)
        qs = np.ascontiguousarray(a[:, :, 4:]).reshape(rows, nb * 16)
    return scales, qs


def _upload_mat(t: ggml.GGMLTensor, device: str):
    """-> (data, scales, wtype) device tensors in the kernel layout."""
    rows, cols = t.shape_rows_cols
    if t.gtype in (ggml.GGML_TYPE_Q4_0, ggml.GGML_TYPE_Q4_1):
        scales, qs = _repack_q4(t)
        d = torch.from_numpy(qs).to(device)
        s = torch.from_numpy(scales.copy()).to(device)
        return d, s, t.gtype
    if t.gtype in _BYTE_GTYPES or t.gtype in _K32_GTYPES or \
            t.gtype in _K16_GTYPES:
        # embedding gather for q5/q8/k-quant tables: dequantize once to
        # f16 (the gather kernel has no byte path; 2 B/weight)
        a = t.to_f32().astype(np.float16)
        return (torch.from_numpy(a).to(device), torch.empty(0),
                ggml.GGML_TYPE_F16)
    if t.gtype == ggml.GGML_TYPE_F16:
        a = np.frombuffer(t.raw, np.float16).reshape(rows, cols)
        return torch.from_numpy(a.copy()).to(device), torch.empty(0), t.gtype
    a = np.frombuffer(t.raw, np.float32).reshape(rows, cols)
    return torch.from_numpy(a.copy()).to(device), torch.empty(0), t.gtype
