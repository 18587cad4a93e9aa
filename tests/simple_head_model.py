"""Host model of the simple decoder's head (csrc/simplehead.hip on the weight image of csrc/simpleheadgeom.h), in numpy float64 on the operands the device
multiplies.  A plain module that shares no code with the package: tests/test_simple_head_model.py pins it on the CPU against torch's float64 F.interpolate +
F.conv2d and shows the wrong models below failing the bound, tests/test_gpu_simple_head.py and tests/test_gpu_simple_decoder.py compare the kernel with it per element.

The model is the LITERAL form -- not the commuted one the kernel runs:
    r = relu(x)                                       x [B, 192, D] = [B, 16, 12, D], values of the operand type
    U(r) = Uy r Ux^T                                  the x 4 bilinear upsample to 64 x 48 as two matrices built from PyTorch's align_corners = False rule:
                                                      s = max((u + 0.5) / 4 - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, n - 1), l = s - i0
    v[k, y, x] = b[k] + sum over (ky, kx, c) of W[k, c, ky, kx] U(r)[c, y + ky - 1, x + kx - 1]      U(r) zero outside 64 x 48
    W = hi + lo, hi = round16(w), lo = round16(w - hi)                                                  what the weight image holds
Beside each value it returns the magnitude sum the bound is stated in: S = sum |U(r)| |W| + |b| per output element (U(r) >= 0 already).

The bound (tests assert it per element, none exempt):
    |hm - v| <= (2 D + 32) (2^-24 S + 2^-126)
        2 D 2^-24 S     a tap's value at a token is 2 D products (hi and lo rows) accumulated in fp32 in any order: each partial sum is at most that tap's share of S
                        and each add rounds once.  The upsample is linear with non-negative weights that sum to one, so an error of e per token magnitude becomes at
                        most e per upsampled magnitude: the shares add up to S.
        16 2^-24 S      the stencil: each of the two interpolation stages is a + l (b - a) as one subtraction and one fused multiply-add.  With e1, e2 the two
                        roundings the error is at most 2^-24 (l (|a| + |b|) + |(1 - l) a + l b|) <= 2^-24 (|a| + 2 l |b|) <= 8 2^-24 ((1 - l) |a| + l |b|) for
                        l <= 7 / 8: eight half-ulps of the interpolated MAGNITUDE per stage, two stages.
        9 2^-24 S       nine additions onto the bias, each partial sum at most S.
        7 2^-24 S       room for the second-order terms of the above.
        2^-126 each     an fp32 result below the normal range may be flushed to zero by any of these operations.
    against the un-split float32 weights: + u^2 S + 2^-25 sum |U(r)|, u = 2^-11 fp16 / 2^-8 bf16 (bound(..., unsplit=True)): |w - (hi + lo)| <= u |lo| <= u^2 |w|,
        and where lo falls among the fp16 subnormals its rounding is at most half their spacing, 2^-25.
Nothing is fitted.  NaN and inf inputs are out of scope."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
U16 = {'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8}
GRID_H, GRID_W, UP = 16, 12, 4
HM_H, HM_W = UP * GRID_H, UP * GRID_W
# the wrong models a kernel or the packer could be (tests/test_simple_head_model.py: each fails the bound on at least one case family)
WRONG = ('align_corners', 'relu_after_upsample', 'border_clamp', 'kykx_transposed', 'bias_dropped', 'lo_dropped')


def round16(x, dtype):
    """fp32 -> the operand type and back, round to nearest even; fp16 saturates at +-65504 as the host packer does"""
    x = np.ascontiguousarray(x, F32)
    if dtype == 'fp16':
        x = np.clip(x, -65504.0, 65504.0)
    return torch.from_numpy(x).to(torch.float16 if dtype == 'fp16' else torch.bfloat16).float().numpy()


def split(w, dtype):
    """(hi, lo) as float32 values of the operand type"""
    w = np.asarray(w, F32)
    hi = round16(w, dtype)
    return hi, round16((w - hi).astype(F32), dtype)


def upsample_matrix(n, wrong=None):
    """[4 n, n] float64: row u holds (1 - l) at i0 and l at i1 of the align_corners = False rule"""
    m = np.zeros((UP * n, n), F64)
    for u in range(UP * n):
        if wrong == 'align_corners':
            s = u * (n - 1) / (UP * n - 1)
        else:
            s = max((u + 0.5) / UP - 0.5, 0.0)
        i0 = int(np.floor(s))
        i1 = min(i0 + 1, n - 1)
        l = s - i0
        m[u, i0] += 1.0 - l
        m[u, i1] += l
    return m


def _conv(up, W, wrong=None):
    """up [B, 64, 48, D] float64, W [K, D, 3, 3] float64 -> [B, K, 64, 48]: the 3 x 3 convolution with zero padding from its definition, one matrix product per tap"""
    B, H, Wd, D = up.shape
    pad = np.pad(up, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='edge' if wrong == 'border_clamp' else 'constant')
    out = np.zeros((B, H, Wd, W.shape[0]), F64)
    for ky in range(3):
        for kx in range(3):
            wt = W[:, :, kx, ky] if wrong == 'kykx_transposed' else W[:, :, ky, kx]
            out += pad[:, ky:ky + H, kx:kx + Wd, :] @ wt.T
    return out.transpose(0, 3, 1, 2)


def upsampled(x, wrong=None):
    """relu then U (or, wrong, U then relu) of x [B, 192, D] -> [B, 64, 48, D] float64"""
    x = np.asarray(x, F64).reshape(-1, GRID_H, GRID_W, x.shape[-1])
    uy, ux = upsample_matrix(GRID_H, wrong), upsample_matrix(GRID_W, wrong)
    if wrong != 'relu_after_upsample':
        x = np.maximum(x, 0.0)
    up = np.einsum('yi,bijd->byjd', uy, x)
    up = np.einsum('xj,byjd->byxd', ux, up)
    return np.maximum(up, 0.0) if wrong == 'relu_after_upsample' else up


def model(x, w, b, dtype, wrong=None, unsplit=False):
    """x [B, 192, D] (values of the operand type), w [K, D, 3, 3], b [K] float32 -> (v [B, K, 64, 48] float64, S); unsplit: the float32 weights themselves, not hi + lo"""
    hi, lo = split(w, dtype)
    W = np.asarray(w, F64) if unsplit else hi.astype(F64) + (0.0 if wrong == 'lo_dropped' else lo.astype(F64))
    bb = np.zeros(len(b), F64) if wrong == 'bias_dropped' else np.asarray(b, F64)
    up = upsampled(x, wrong)
    v = _conv(up, W, wrong) + bb[None, :, None, None]
    S = _conv(np.abs(up), np.abs(W)) + np.abs(np.asarray(b, F64))[None, :, None, None]
    return v, S


def upsampled_sum(x):
    """sum over (taps, channels) of |U(r)| per output pixel [B, 1, 64, 48]: the factor of the absolute term of the un-split bound"""
    up = upsampled(x)
    return _conv(up, np.ones((1, up.shape[-1], 3, 3), F64))


def bound(S, D, dtype=None, unsplit=False, x=None):
    b = (2 * D + 32) * (2.0 ** -24 * S + 2.0 ** -126)
    if unsplit:
        b = b + U16[dtype] ** 2 * S + 2.0 ** -25 * upsampled_sum(x)
    return b


def ratio(got, ref, bnd):
    """|got - ref| / bound per element; inf where got is not finite or the bound is 0 and missed"""
    got = np.asarray(got, F64)
    with np.errstate(all='ignore'):
        err = np.abs(got - ref)
        r = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(got) & np.isfinite(r), r, np.inf)


def emulate(x, w, b, dtype):
    """one order a kernel may take, in float32: the commuted form -- per tap the hi and lo products into one accumulator 32 channels at a time, the interpolation as
    a + l (b - a) rows first, the nine taps added onto the bias in order -- what the bound must admit"""
    hi, lo = split(w, dtype)
    x = np.maximum(np.asarray(x, F32), F32(0)).reshape(-1, GRID_H * GRID_W, x.shape[-1])
    B, T, D = x.shape
    K = hi.shape[0]
    out = np.broadcast_to(np.asarray(b, F32)[None, :, None, None], (B, K, HM_H, HM_W)).copy()

    def lerp_axis(p, n, axis, shift):
        """p sampled at positions u + shift - 1 for u in [0, 4 n) along `axis`, zero outside"""
        idx0, idx1, lam, ok = [], [], [], []
        for u in range(UP * n):
            uu = u + shift - 1
            s = max((uu + 0.5) / UP - 0.5, 0.0)
            i0 = min(int(np.floor(s)), n - 1)
            idx0.append(i0), idx1.append(min(i0 + 1, n - 1)), lam.append(s - int(np.floor(s))), ok.append(0 <= uu < UP * n)
        a, c = np.take(p, idx0, axis), np.take(p, idx1, axis)
        shp = [1] * p.ndim
        shp[axis] = -1
        l = np.asarray(lam, F32).reshape(shp)
        r = (a + (l * (c - a).astype(F32)).astype(F32)).astype(F32)
        return r * np.asarray(ok, F32).reshape(shp)

    for ky in range(3):
        for kx in range(3):
            acc = np.zeros((B, T, K), F32)
            for k0 in range(0, D, 32):
                acc = (acc + x[..., k0:k0 + 32] @ hi[:, k0:k0 + 32, ky, kx].T).astype(F32)
                acc = (acc + x[..., k0:k0 + 32] @ lo[:, k0:k0 + 32, ky, kx].T).astype(F32)
            p = acc.reshape(B, GRID_H, GRID_W, K).transpose(0, 3, 1, 2)
            out = (out + lerp_axis(lerp_axis(p, GRID_H, 2, ky), GRID_W, 3, kx)).astype(F32)
    return out
