"""Host model of the keypoint head's GEMMs (csrc/gemm.hip EPI_DECONV / EPI_DECONV_FINAL / EPI_HEATMAP on operands packed by csrc/weights.hip pack_deconv and
upload_final), in numpy float64 on the operands the device multiplies.  A plain module: tests/test_head_model.py pins it on the CPU against torch's float64
modules and shows the wrong models below failing the bounds, tests/test_gpu_head.py compares the kernels with it per element.

The transposed convolution is written from its definition,
    out[n, oy, ox, o] = sum over (c, ky, kx, iy, ix) of x[n, iy, ix, c] w[c, o, ky, kx]   with  oy = 2 iy - 1 + ky,  ox = 2 ix - 1 + kx,
one matrix product per (ky, kx) scattered to the rows and columns it reaches -- not the four output-parity GEMMs the kernel runs.  Tensors are NHWC as on the device.

    fold        scale = gamma / sqrt(var + 1e-5f), bias = beta - mean scale, w scale: all float32 as pack_deconv computes them, then ONE rounding to the operand
                type (host_to_bits: fp16 saturates at +-65504)
    stage 0     v = relu(z + bias); fp16: min(v, 65504) (pack2<F16>'s clamp: the project's semantics; bf16 has none); one rounding to the storage type
    final conv  W_eff = hi + lo, hi = round16(w), lo = round16(w - hi) (upload_final); heatmaps = a . W_eff + b in fp32
Beside each value the model returns the magnitude sum the bounds are stated in: S = sum |x| |w_folded| + |bias| and S2 = sum |a| |W_eff| + |b|.

The bounds (u = 2^-11 fp16, 2^-8 bf16; tests/test_gpu_head.py asserts them per element, none exempt):
    stage 0 against this model          |got - v| <= u |v| + 4 Cin 2^-24 S + 2^-25
        u |v|: the one round-to-nearest store; 4 Cin 2^-24 S: K = 4 Cin products accumulated in fp32 in any order (each partial sum is at most S, each add rounds
        once) and the bias add; 2^-25: half the spacing of the fp16 subnormals, where u |v| no longer covers the store.  relu and the clamp do not expand an error.
    ... against the un-folded module    + 2 u S: the folded weights are rounded once to the operand type (u sum |x| |w scale| <= u S) and scale, w scale and bias
        are float32 results (a few 2^-24 S, inside the second u S)
    final conv on the device's own activation bits      |hm - ref| <= 258 2^-24 S2: 256 products per plane in fp32, the hi + lo add and the bias add
NaN and inf inputs are out of scope."""
import numpy as np

import residual_row_model as RM

F32, F64 = np.float32, np.float64
U = {'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8}
F16_MAX = 65504.0
BN_EPS = F32(1e-5)
# the wrong models a kernel or the packer could be (tests/test_head_model.py: each fails the bounds on at least one case)
WRONG_STAGE0 = ('ky_swap', 'parity_transposed', 'border_clamp', 'seam', 'no_relu', 'plus_mean', 'no_clamp', 'round_before_fold')
WRONG_FINAL = ('lo_dropped',)


def round16(x, dtype):
    """fp32 -> the operand type and back as the host packer rounds (host_to_bits: nearest even; fp16 saturates at +-65504)"""
    x = np.asarray(x, F32)
    if dtype == 'fp16':
        x = np.clip(x, -F16_MAX, F16_MAX)
    return RM.from_bits(RM.to_bits(x, dtype), dtype)


def fold(w, gamma, beta, mean, var, dtype, wrong=None):
    """pack_deconv: (w_folded [Cin,256,4,4] as float32 values of the operand type, bias [256] float32)"""
    w, gamma, beta, mean, var = (np.asarray(a, F32) for a in (w, gamma, beta, mean, var))
    scale = (gamma / np.sqrt((var + BN_EPS).astype(F32))).astype(F32)
    ms = (mean * scale).astype(F32)
    bias = (beta + ms if wrong == 'plus_mean' else beta - ms).astype(F32)
    if wrong == 'round_before_fold':
        return round16((round16(w, dtype) * scale[None, :, None, None]).astype(F32), dtype), bias
    return round16((w * scale[None, :, None, None]).astype(F32), dtype), bias


def deconv(x, w, wrong=None, dt=F64):
    """ConvTranspose2d(Cin, O, 4, stride 2, padding 1, no bias) from its definition: x [B,H,W,Cin], w [Cin,O,4,4] -> [B,2H,2W,O] in `dt`"""
    x, w = np.asarray(x, dt), np.asarray(w, dt)
    if wrong == 'seam':            # the image index lost in the row arithmetic: the batch is one tall image, row -1 of image n is the last row of image n - 1
        B, H, W, C = x.shape
        return deconv(x.reshape(1, B * H, W, C), w, None, dt).reshape(B, 2 * H, 2 * W, -1)
    if wrong == 'border_clamp':    # a tap that leaves the image reads the clamped row / column instead of zero
        return deconv(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='edge'), w, None, dt)[:, 2:-2, 2:-2]
    B, H, W, C = x.shape
    out = np.zeros((B, 2 * H, 2 * W, w.shape[1]), dt)
    xf = x.reshape(-1, C)
    wt = np.ascontiguousarray(w.transpose(2, 3, 0, 1))                    # [ky, kx] -> a contiguous [Cin, O] matrix
    iy, ix = np.arange(H), np.arange(W)
    for ky in range(4):
        oy = 2 * iy - 1 + ky
        vy = (oy >= 0) & (oy < 2 * H)
        kw = {1: 3, 3: 1}.get(ky, ky) if wrong == 'ky_swap' else ky       # even output rows: the weights of ky = 1 and ky = 3 exchanged
        for kx in range(4):
            ox = 2 * ix - 1 + kx
            vx = (ox >= 0) & (ox < 2 * W)
            t = (xf @ wt[kw, kx]).reshape(B, H, W, -1)
            out[:, oy[vy][:, None], ox[vx][None, :]] += t[:, iy[vy][:, None], ix[vx][None, :]]
    if wrong == 'parity_transposed':   # parity (a, b) stored at (b, a) of its 2 x 2 block
        out[:, 1::2, 0::2], out[:, 0::2, 1::2] = out[:, 0::2, 1::2].copy(), out[:, 1::2, 0::2].copy()
    return out


def conv_parts(x16, wf16, wrong=None):
    """(z, A): z = deconv(x, w_folded) and A = deconv(|x|, |w_folded|) in float64 -- the two products every stage-0 reference of a case shares"""
    return deconv(x16, wf16, wrong), deconv(np.abs(x16), np.abs(wf16))


def stage0(z, A, bias, dtype, wrong=None):
    """z + bias -> (v, stored, S): v = the float64 value in front of the store (relu, fp16 clamp), stored = v rounded once to the storage type, S = A + |bias|"""
    bias = np.asarray(bias, F64)
    v = z + bias
    if wrong != 'no_relu':
        v = np.maximum(v, 0.0)
    if dtype == 'fp16' and wrong != 'no_clamp':
        v = np.clip(v, -F16_MAX, F16_MAX)
    with np.errstate(over='ignore'):
        stored = RM.from_bits(RM.to_bits(v.astype(F32), dtype), dtype).astype(F64)     # no clamp of its own: beyond the fp16 range this is inf
    return v, stored, A + np.abs(bias)


def module(x, w, gamma, beta, mean, var, dtype):
    """the un-folded float64 module on the same input: relu(BatchNorm2d(eval, eps 1e-5)(ConvTranspose2d(x))), with the project's fp16 store clamp"""
    g, b, m, s = (np.asarray(a, F64) for a in (gamma, beta, mean, var))
    v = np.maximum((deconv(x, w) - m) / np.sqrt(s + 1e-5) * g + b, 0.0)
    return np.minimum(v, F16_MAX) if dtype == 'fp16' else v


def bound0(v, S, Cin, dtype, unfolded=False):
    b = U[dtype] * np.abs(v) + 4 * Cin * 2.0 ** -24 * S + 2.0 ** -25
    return b + 2 * U[dtype] * S if unfolded else b


def split_final(w, dtype):
    """upload_final: (hi, lo) as float32 values of the operand type"""
    w = np.asarray(w, F32)
    hi = round16(w, dtype)
    return hi, round16((w - hi).astype(F32), dtype)


def final(a, w_fin, b_fin, dtype, wrong=None):
    """a [B,H,W,256] (values of the storage type), w_fin [Kp,256], b_fin [Kp] -> (heatmaps [B,Kp,H,W] float64, S2)"""
    hi, lo = split_final(w_fin, dtype)
    W = hi.astype(F64) + (0.0 if wrong == 'lo_dropped' else lo.astype(F64))
    a, b = np.asarray(a, F64), np.asarray(b_fin, F64)
    hm = a @ W.T + b
    S2 = np.abs(a) @ np.abs(W).T + np.abs(b)
    return hm.transpose(0, 3, 1, 2), S2.transpose(0, 3, 1, 2)


def bound_final(S2):
    return 258 * 2.0 ** -24 * S2


def ratio(got, ref, bound):
    """|got - ref| / bound per element; inf where got is not finite or the bound is 0 and missed"""
    got = np.asarray(got, F64)
    with np.errstate(all='ignore'):
        err = np.abs(got - ref)
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(got) & np.isfinite(r), r, np.inf)


def emulate_stage0(x16, wf16, bias, dtype):
    """one of the orders a kernel may take: the definition in float32 (numpy's float32 products), + bias, relu, clamp, one rounding -- what the bounds must admit"""
    v = np.maximum(deconv(x16, wf16, dt=F32) + np.asarray(bias, F32), F32(0))
    if dtype == 'fp16':
        v = np.minimum(v, F32(F16_MAX))
    return RM.from_bits(RM.to_bits(v, dtype), dtype)


def emulate_final(a, w_fin, b_fin, dtype):
    """hi and lo products in separate float32 accumulators, hi + lo, + bias"""
    hi, lo = split_final(w_fin, dtype)
    a = np.asarray(a, F32)
    return (((a @ hi.T).astype(F32) + (a @ lo.T).astype(F32)).astype(F32) + np.asarray(b_fin, F32)).astype(F32).transpose(0, 3, 1, 2)
