"""The seeded inputs of the patch gather tests (tests/test_patch_gather_host.py on the CPU, tests/test_gpu_patch_gather.py on the device).  Every case is three
crops (a test takes the first n_src of them); every value is finite, and stays finite in the operand type it is made for.

fp32 input, f32_cases(dtype)[name] = float32 [3, 3, 256, 192]:
    gauss       N(0, 1.5) crops
    position    crop 0: every (y, x) of a channel carries its own 16-bit code -- pixel i = y * 192 + x (rotated by 16 384 c in channel c, so that the channels differ
                too) takes the i-th code of the sequence "positive normal codes upwards, then negative normal codes upwards"; 49 152 pixels fit into the 61 440
                normal codes of fp16 and the 65 024 of bf16, and no pixel is zero: any wrong source pixel, and a border that is not zero, changes the output.
                crops 1 and 2 code the channel and the crop index (1 + c + 4 k, constant over the image): a wrong crop or channel shows on every element.
    edges       the rounding edges of the conversion on a Gaussian background, walked cyclically over every pixel next to a border: the two columns on either side
                of every patch boundary (x = 16 k - 4 .. 16 k - 1), the image's own first and last two columns, and the same rows -- the image corners included.
                Both types: ties to even of fp16 and of bf16 (and their float32 neighbours), -0.0, fp16's subnormal range (2^-24, the tie 3 * 2^-25, the tie
                2^-25 and the float just above it, 2^-14 - 2^-25), +-1e6, 65520.  fp16 only: +-65504, the float just below 65520, FLT_MAX (all clamped).
                bf16 only: large values up to the bf16 maximum 0x7F7F.
uint8 input, u8_cases()[name] = uint8 [3, 256, 192, 3]:
    allbytes    crop 0: byte `off` of row y is (12 y + off // 48 + 37 (off % 48)) % 256.  off % 48 fixes both the position e = off % 16 inside a 16-byte piece
                and the channel off % 3, and 12 y + off // 48 runs over 0 .. 3071: every byte value occurs at every (e, channel) phase, 12 times.  crops 1, 2 random
    const       all 0, all 255, random"""
import functools

import numpy as np

import patch_gather_model as PM
import residual_row_model as RM

F32 = np.float32
DTYPES = ('fp16', 'bf16')
F32_CASES = ('gauss', 'position', 'edges')
U8_CASES = ('allbytes', 'const')
FIRST_NORMAL = {'fp16': 0x0400, 'bf16': 0x0080}
FLT_MAX = np.finfo(F32).max


def _position_crop(dtype):
    i = np.arange(PM.H * PM.W, dtype=np.int64)
    half = i.size // 2
    seq = np.where(i < half, FIRST_NORMAL[dtype] + i, 0x8000 + FIRST_NORMAL[dtype] + (i - half)).astype(np.uint16)
    codes = np.stack([np.roll(seq, -16384 * c) for c in range(3)]).reshape(3, PM.H, PM.W)
    v = RM.from_bits(codes, dtype)
    assert np.isfinite(v).all() and (v != 0).all() and np.array_equal(PM.to16(v, dtype), codes)
    return v


def edge_values(dtype):
    up = lambda a: np.nextafter(F32(a), F32(np.inf))
    dn = lambda a: np.nextafter(F32(a), F32(-np.inf))
    e = []
    for t in (1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11, 2049.0, 2051.0, 1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8, 257.0, 259.0):   # ties of fp16 (first four) and bf16
        e += [t, -t, up(t), dn(t), -up(t)]
    e += [-0.0, 0.0, 2.0 ** -24, -2.0 ** -24, 3.0 * 2.0 ** -25, 2.0 ** -25, -2.0 ** -25, up(2.0 ** -25), dn(2.0 ** -25), 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14,
          5.0 * 2.0 ** -25, 1e6, -1e6, 65520.0, -65520.0]
    if dtype == 'fp16':
        e += [65504.0, -65504.0, dn(65520.0), up(65504.0), FLT_MAX, -FLT_MAX, 1e30]
    else:
        top = RM.from_bits(np.array([0x7F7F], np.uint16), 'bf16')[0]
        e += [top, -top, dn(top), 1e38, -1e38, 3e38, 65504.0, dn(65520.0)]
    return np.array(e, F32)


def border_mask():
    """the pixels next to a border: two columns / rows on either side of every patch boundary, and the image's own first and last two"""
    near = lambda n: np.isin((np.arange(n) + 2) % 16, (15, 0, 1, 14)) | (np.arange(n) < 2) | (np.arange(n) >= n - 2)
    return near(PM.H)[:, None] | near(PM.W)[None, :]


@functools.lru_cache(maxsize=None)
def f32_cases(dtype):
    rng = np.random.default_rng(31 + (dtype == 'bf16'))
    out = {'gauss': (rng.standard_normal((3, 3, PM.H, PM.W)) * 1.5).astype(F32)}
    coded = np.stack([np.full((3, PM.H, PM.W), 0, F32) + (1 + np.arange(3, dtype=F32)[:, None, None] + 4 * k) for k in (1, 2)])
    out['position'] = np.concatenate([_position_crop(dtype)[None], coded]).astype(F32)
    ev, mask = edge_values(dtype), border_mask()
    x = rng.standard_normal((3, 3, PM.H, PM.W)).astype(F32)
    n = int(mask.sum())
    for k in range(3):
        for c in range(3):
            x[k, c][mask] = ev[(np.arange(n) + 7 * c + 3 * k) % len(ev)]
    out['edges'] = x
    for v in out.values():
        assert v.dtype == F32 and np.isfinite(v).all() and np.isfinite(RM.from_bits(PM.to16(v, dtype), dtype)).all()
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def u8_cases():
    rng = np.random.default_rng(47)
    rand = lambda: rng.integers(0, 256, (PM.H, PM.W, 3), dtype=np.uint8)
    y, off = np.arange(PM.H)[:, None], np.arange(PM.W * 3)[None, :]
    allb = ((12 * y + off // 48 + 37 * (off % 48)) % 256).astype(np.uint8).reshape(PM.H, PM.W, 3)
    out = {'allbytes': np.stack([allb, rand(), rand()]),
           'const': np.stack([np.zeros((PM.H, PM.W, 3), np.uint8), np.full((PM.H, PM.W, 3), 255, np.uint8), rand()])}
    for v in out.values():
        v.setflags(write=False)
    return out


def phase_coverage(crop):
    """uint8 crop [256, 192, 3] -> bool [256 values, 16 positions in a 16-byte piece, 3 channels]: which (value, e, channel) occur"""
    off = np.arange(PM.W * 3)
    seen = np.zeros((256, 16, 3), bool)
    rows = crop.reshape(PM.H, PM.W * 3)
    seen[rows, np.broadcast_to(off % 16, rows.shape), np.broadcast_to(off % 3, rows.shape)] = True
    return seen
