"""Host model of the producer row of the two-plane residual stream (csrc/common.h: planes_decode8, planes_split8, granule_stats8 /
granule_stats16), restated in numpy float32 operation by operation.  A plain module: tests/test_residual_row_model.py pins it on the CPU,
tests/test_gpu_residual_row.py compares every producer site with it bit for bit.

    r  = fl32(hi + lo)                                   planes_decode8
    v  = fl32(st + r), fp16: clamped to +-65504          the caller's add, split_planes2's clamp (the statistics are of the clamped v)
    hi = round16(v), lo = round16(fl32(v - hi))          split_planes2
    s1 = the pairwise tree over the granule's 64 values  chunk8_sum, then chunk pairs, pairs of pairs, the two halves
    s2 = sum (v - s1 / 64)^2 on the same tree            chunk8_m2: the chain s2 = fma(d, d, s2) in column order per 8-column chunk

The 16-bit conversions are torch's (round to nearest even, gradual underflow); the signs of zeros are part of the bits.  fmaf is emulated
through float64 (d * d is exact there; the sum is rounded twice), so s2 is a close model, not a bit-exact one."""
import numpy as np
import torch

F32 = np.float32
F16_MAX = F32(65504.0)


def _tdt(dtype):
    return torch.float16 if dtype in ('fp16', 'f16') else torch.bfloat16


def to_bits(x, dtype):
    """fp32 -> the 16-bit code (uint16), round to nearest even; no clamp (above the fp16 range: inf)"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(_tdt(dtype))
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def from_bits(bits, dtype):
    """the 16-bit code -> the fp32 value it stands for (exact)"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    return torch.from_numpy(b.view(np.int16)).view(_tdt(dtype)).float().numpy()


def decode(hi_bits, lo_bits, dtype):
    return (from_bits(hi_bits, dtype) + from_bits(lo_bits, dtype)).astype(F32)


def split(x, dtype):
    """what planes_split8 does to fp32 values x: (clamped x, hi bits, lo bits)"""
    v = np.ascontiguousarray(x, dtype=F32)
    if dtype in ('fp16', 'f16'):
        v = np.clip(v, -F16_MAX, F16_MAX)
    hi_bits = to_bits(v, dtype)
    lo_bits = to_bits((v - from_bits(hi_bits, dtype)).astype(F32), dtype)
    return v, hi_bits, lo_bits


def row(st, r, dtype):
    """v = st + r through the row: (v as stored, hi bits, lo bits)"""
    return split((np.asarray(st, dtype=F32) + np.asarray(r, dtype=F32)).astype(F32), dtype)


def _tree(c):
    """[..., 8] chunk values -> chunk pairs, pairs of pairs, the two halves"""
    p = (c[..., 0::2] + c[..., 1::2]).astype(F32)
    q = (p[..., 0::2] + p[..., 1::2]).astype(F32)
    return (q[..., 0] + q[..., 1]).astype(F32)


def _granules(v):
    v = np.ascontiguousarray(v, dtype=F32)
    assert v.shape[-1] % 64 == 0
    return v.reshape(v.shape[:-1] + (v.shape[-1] // 64, 8, 8))


def granule_s1(v):
    """[..., N] -> [..., N / 64]"""
    g = _granules(v)
    a = (g[..., 0::2] + g[..., 1::2]).astype(F32)              # (v0+v1), (v2+v3), (v4+v5), (v6+v7)
    b = (a[..., 0::2] + a[..., 1::2]).astype(F32)
    return _tree((b[..., 0] + b[..., 1]).astype(F32))


def granule_m2(v, s1):
    g = _granules(v)
    mg = (np.asarray(s1, dtype=F32) * F32(1.0 / 64.0)).astype(F32)[..., None]
    s2 = np.zeros(g.shape[:-1], F32)
    for e in range(8):
        d = (g[..., e] - mg).astype(F32)
        s2 = (d.astype(np.float64) * d.astype(np.float64) + s2.astype(np.float64)).astype(F32)
    return _tree(s2)


def m2_fp64(v):
    """(M2, mean) of every granule of the stored values, in float64"""
    g = np.asarray(v, dtype=np.float64).reshape(v.shape[:-1] + (v.shape[-1] // 64, 64))
    mean = g.mean(-1)
    return ((g - mean[..., None]) ** 2).sum(-1), mean


def m2_bound(m2, mean):
    """the bound on |s2 - M2| per granule: at most 11 roundings of 2^-24 on the chain and its merges, and the granule mean good to 2^-22 |mean|"""
    return 2.0 ** -20 * m2 + 64.0 * (2.0 ** -22 * np.abs(mean)) ** 2


def m2_one_pass(v):
    """the textbook float32 one-pass form the row must NOT be: sum(v^2) - s1^2 / 64 (negative control)"""
    g = np.ascontiguousarray(v, dtype=F32).reshape(v.shape[:-1] + (v.shape[-1] // 64, 64))
    s1 = g.sum(-1, dtype=F32)
    return ((g * g).astype(F32).sum(-1, dtype=F32) - (s1 * s1).astype(F32) * F32(1.0 / 64.0)).astype(F32)
