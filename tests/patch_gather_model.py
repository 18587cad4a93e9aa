"""Host model of the patch gather (csrc/elementwise.hip: im2col_kernel, plain and FLIP, and im2col_twin_kernel), in numpy.  A plain module:
tests/test_patch_gather_host.py pins it on the CPU against the convolution it stands for, tests/test_gpu_patch_gather.py compares the twelve kernel
instantiations with it bit for bit.

    PatchEmbed = Conv2d(3, D, k = 16, s = 16, padding = 2): patch (py, px) covers rows 16 py - 2 .. 16 py + 13 and columns 16 px - 2 .. 16 px + 13 of the
    256 x 192 crop, zero outside it.  Row b * 192 + py * 12 + px of the patch matrix, column c * 256 + ky * 16 + kx (the flattening of the conv weight
    [D, 3, 16, 16]) holds pixel (16 py - 2 + ky, 16 px - 2 + kx) of channel c as a 16-bit code of the operand type, code 0 (+0.0) outside the crop.
    mode 0   output crop b reads source crop min(b, n_src - 1)                          (the rows of a padded encoder batch repeat the last crop)
    mode 1   the same, the crop mirrored left-right first                               (the zero border is the MIRROR image's left border)
    mode 2   r = min(b, 2 n_src - 1): source crop r >> 1, mirrored when r & 1           (the flip-test twin: crop, mirror, crop, mirror, ..., padding)

The conversion to the operand type is round to nearest even; fp16 clamps to +-65504 first (common.h to_bits<F16> / pack2<F16>), bf16 does not.  The uint8 input is
normalised as pre_img does it: float32((float64(u) / 255 - mean_c) / std_c)."""
import numpy as np

import residual_row_model as RM

F32, F64 = np.float32, np.float64
MEAN = np.array([0.485, 0.456, 0.406], F64)
STD = np.array([0.229, 0.224, 0.225], F64)
H, W, P, GY, GX = 256, 192, 16, 16, 12          # crop, patch side, patches per column / row
F16_MAX = F32(65504.0)


def normalise_u8(u8):
    """uint8 [..., 3] (channel last) -> float32 of the same shape"""
    return ((np.asarray(u8).astype(F64) / 255.0 - MEAN) / STD).astype(F32)


def nchw(x):
    """[n, 256, 192, 3] -> [n, 3, 256, 192]"""
    return np.ascontiguousarray(np.moveaxis(x, -1, 1))


def to16(x, dtype):
    """float32 -> the 16-bit code (uint16): round to nearest even, fp16 clamped to +-65504 first"""
    x = np.array(x, F32)                                  # a copy: the cases are read-only arrays
    if dtype in ('fp16', 'f16'):
        x = np.clip(x, -F16_MAX, F16_MAX)
    return RM.to_bits(x, dtype)


def patches(img, border=2):
    """one crop [3, 256, 192] of codes -> its patch rows [192, 768]; the pixel behind column (c, ky, kx) of patch (py, px) is (16 py - border + ky, 16 px - border + kx)"""
    pad = np.zeros((3, H + border + P, W + border + P), np.uint16)
    pad[:, border:border + H, border:border + W] = img
    win = pad[:, :H, :W].reshape(3, GY, P, GX, P)                        # (c, py, ky, px, kx)
    return np.ascontiguousarray(win.transpose(1, 3, 0, 2, 4)).reshape(GY * GX, 3 * P * P)


def source(b, n_src, mode):
    """output crop b -> (source crop, mirrored)"""
    if mode == 2:
        r = min(b, 2 * n_src - 1)
        return r >> 1, bool(r & 1)
    return min(b, n_src - 1), mode == 1


def gather(x16_bits, B, n_src, mode, patches=patches, source=source):
    """codes [n, 3, 256, 192] (n >= n_src) -> the patch matrix [B * 192, 768] (uint16).  patches / source: the pieces, replaceable by the wrong variants of
    tests/test_patch_gather_host.py"""
    x = np.asarray(x16_bits, np.uint16)
    assert x.shape[1:] == (3, H, W) and 1 <= n_src <= x.shape[0]
    cache = {}
    out = np.empty((B, GY * GX, 3 * P * P), np.uint16)
    for b in range(B):
        key = source(b, n_src, mode)
        if key not in cache:
            s, m = key
            cache[key] = patches(x[s][..., ::-1] if m else x[s])
        out[b] = cache[key]
    return out.reshape(B * GY * GX, 3 * P * P)


def decode(bits, dtype):
    """codes -> the values they stand for, float64"""
    return RM.from_bits(bits, dtype).astype(F64)
