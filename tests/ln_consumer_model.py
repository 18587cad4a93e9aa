"""Host model of the consumer half of the fused LayerNorm (csrc/common.h: ln_merge, ln_fold; csrc/quant8.hip: the normalise step of ln_quant_kernel with
the block scale and code packing of csrc/mx8.h), restated in numpy float32 operation by operation.  A plain module: tests/test_ln_consumer_model.py pins it on
the CPU, tests/test_gpu_ln_consumer.py compares the kernels with it.

    s1   = ((0 + s_0) + s_1) + ...                          one rounding per add, in granule order
    mean = fl(s1 * inv_d), inv_d = fl(1 / D)                as the host computes inv_d (1.0f / (float)D)
    d_g  = fma(s_g, 1/64, -mean)                            1/64 is a float32 constant; ONE rounding
    m2   = (...(0 + fma(64 d_0, d_0, M2_0)) + ...)          64 d is exact
    var  = fma(m2, inv_d, 1e-6f)
    rstd = rsqrt(var)                                       here: fl(1 / sqrt(var)) from float64, i.e. correctly rounded; the device's rsqrtf may differ by an ulp
    fold = fma(fma(-mean, s, acc), rstd, b)
    quant: y = fma(x, rstd, fl(-mean * rstd)); per 32 columns E = max(exponent field of amax - 7, 0), code = e4m3(y * 2^(127 - E))

fma is exact here (fma32): the product of two float32 is exact in float64, the sum is rounded to ODD in float64 (TwoSum gives the sign of what the float64 sum
lost) and then to float32 -- round-to-odd at 53 bits followed by round-to-nearest at 24 is the correctly rounded result."""
import numpy as np
import torch

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24                      # unit roundoff of float32
EPS32 = F32(1e-6)
INV64 = F32(1.0 / 64.0)


def inv_d(D):
    return F32(1.0) / F32(D)


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise on float32 arrays"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    t = a.astype(F64) * b.astype(F64)                # exact: 48 bits
    c = c.astype(F64)
    s = t + c
    bb = s - t
    e = (t - (s - bb)) + (c - bb)                    # TwoSum: t + c == s + e exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)     # the odd one of the two float64 that bracket t + c
    return s.astype(F32)


def merge(p, D):
    """ln_merge on partials p [..., T, 2] (float32) -> (mean, rstd, var), float32"""
    p = np.asarray(p, F32)
    T = p.shape[-2]
    iv = inv_d(D)
    s1 = np.zeros(p.shape[:-2], F32)
    for t in range(T):
        s1 = (s1 + p[..., t, 0]).astype(F32)
    mean = (s1 * iv).astype(F32)
    m2 = np.zeros_like(s1)
    for t in range(T):
        d = fma32(p[..., t, 0], INV64, -mean)
        m2 = (m2 + fma32((F32(64.0) * d).astype(F32), d, p[..., t, 1])).astype(F32)
    var = fma32(m2, iv, EPS32)
    rstd = (1.0 / np.sqrt(var.astype(F64))).astype(F32)
    return mean, rstd, var


def fold(acc, mean, s, rstd, b):
    """ln_fold: rstd * (acc - mean * s) + b as two fused multiply-adds"""
    return fma32(fma32(-np.asarray(mean, F32), s, acc), rstd, b)


def quant_normalise(x, mean, rstd):
    """ln_quant_kernel's normalise step on x [M, D] (the hi plane as float32), mean / rstd [M]"""
    mean, rstd = np.asarray(mean, F32)[:, None], np.asarray(rstd, F32)[:, None]
    sh = (-mean * rstd).astype(F32)
    return fma32(x, rstd, sh)


def mx_quantise(y):
    """mx8.h on y [M, D]: (E8M0 bytes [M, D / 32], e4m3 codes [M, D] as uint8, the scaled values the codes round)"""
    M, D = y.shape
    amax = np.abs(y).reshape(M, D // 32, 32).max(-1).astype(F32)
    ex = ((amax.view(np.uint32) >> 23) & 0xff).astype(np.int64)
    E = np.where(ex > 7, ex - 7, 0)
    inv = ((254 - E).astype(np.uint32) << 23).view(F32)
    scaled = (y * np.repeat(inv, 32, axis=1)).astype(F32)
    codes = torch.from_numpy(scaled).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return E.astype(np.uint8), codes, scaled


# ---- the partials of a stored row, and the float64 references -----------------------------------------------------------------------------------------------

def partials_fp64(v):
    """(sum, M2 about the granule's own mean) of every 64-column granule of v [..., D], evaluated in float64 and rounded to float32: [..., D / 64, 2]"""
    g = np.asarray(v, F64).reshape(v.shape[:-1] + (v.shape[-1] // 64, 64))
    s = g.sum(-1)
    m2 = ((g - g.mean(-1, keepdims=True)) ** 2).sum(-1)
    return np.stack([s, m2], -1).astype(F32)


def merge_fp64(p, D):
    """the same merge identity on the same float32 partials, in float64: (mean, M2, rstd)"""
    p = np.asarray(p, F64)
    mean = p[..., 0].sum(-1) / D
    m2 = (p[..., 1] + 64.0 * (p[..., 0] / 64.0 - mean[..., None]) ** 2).sum(-1)
    return mean, m2, 1.0 / np.sqrt(m2 / D + F64(EPS32))


def two_pass_fp64(v):
    """mean, M2 and rstd of the stored row, two passes in float64 (eps = 1e-6, the real number)"""
    v = np.asarray(v, F64)
    mean = v.mean(-1)
    m2 = ((v - mean[..., None]) ** 2).sum(-1)
    return mean, m2, 1.0 / np.sqrt(m2 / v.shape[-1] + 1e-6)


def bounds(p, D, mean_ref, m2_ref, partials_rounded=False, rsqrt_rel=U):
    """Bounds on |mean - mean_ref| and on |rstd - rstd_ref| / rstd_ref, from the operation sequence of ln_merge (u = 2^-24, every count rounded up;
    g_k = k u / (1 - k u)).  p: the float32 partials [..., T, 2]; (mean_ref, m2_ref): the float64 reference.

    mean.   s1 takes T - 1 roundings (0 + s_0 is exact), each at most u times a partial sum that is at most A = sum |s_g|; inv_d = (1 / D)(1 + u) and the
            product add one each:  |mean - mean*| <= g_{T+1} A / D =: Em.
    d_g.    fma(s_g, 1/64, -mean) is fl(s_g / 64 - mean), ONE rounding:  d_g = (d*_g - e)(1 + u_g) with e = mean - mean* common to the row, |e| <= Em.
    m2.     The error of d enters 64 d^2 as 2 * 64 |d| dd + 64 dd^2.  Its common part e does so only in second order: sum_g d*_g = 0 (d* is centred about the
            reference mean), hence 64 sum_g (d*_g - e)^2 = 64 sum d*^2 + D e^2 -- the first-order terms 2 * 64 d*_g e cancel over the row, and D Em^2 remains.
            Its own part dd_g = u (|d*_g| + Em) per granule is kept as 2 * 64 (|d*_g| + Em) dd_g + 64 dd_g^2.  fma(64 d, d, M2_g) rounds once and the T - 1 adds
            of the chain once each, every one at most u times a partial sum of non-negative terms, at most M2*:
            |m2 - M2*| <= D Em^2 + sum_g (128 (|d*_g| + Em) dd_g + 64 dd_g^2) + g_{T+1} M2* =: EM.
    var.    fma(m2, inv_d, eps): inv_d's rounding u M2* / D, the fma's own u var*:  |var - var*| <= EM / D + u M2* / D + u var* =: Ev.
    rstd.   1 / sqrt is monotone, and var >= eps (1 - 2u) whatever the errors are (M2_g >= 0: m2 is a sum of non-negative terms):
            rstd / rstd* lies in [(var* / (var* + Ev))^1/2, (var* / max(var* - Ev, eps (1 - 2u)))^1/2]; the bound is the larger deviation from 1 (about Ev / 2 var*),
            plus the reciprocal square root's own rsqrt_rel (u for the model's correctly rounded one; the device's documented 1 ulp and the final rounding:
            2 ulps <= 2^-22).  On a constant row of a large value the bound is wide for a reason: one ulp of mean is a d of 2^-24 |mean|, and at |mean| = 1000 its
            square is already 0.4 % of eps.
    partials_rounded: the reference is the stored row itself and the partials are its float64 statistics rounded to float32 -- s_g and M2_g each carry u:
            Em grows by u A / D, dd_g by u |s_g| / 64, EM by u sum M2_g, and eps = 1e-6f differs from 1e-6 by at most u 1e-6."""
    p = np.asarray(p, F64)
    T = p.shape[-2]
    g = lambda k: k * U / (1.0 - k * U)
    A = np.abs(p[..., 0]).sum(-1)
    Em = g(T + 1) * A / D + (U * A / D if partials_rounded else 0.0)
    dstar = np.abs(p[..., 0] / 64.0 - np.asarray(mean_ref, F64)[..., None]) + Em[..., None]        # |d*_g - e| at most
    dd = U * dstar
    if partials_rounded:
        q = U * np.abs(p[..., 0]) / 64.0
        dstar = dstar + q
        dd = q + U * dstar
    EM = D * Em * Em + (128.0 * dstar * dd + 64.0 * dd * dd).sum(-1) + g(T + 1) * m2_ref + (U * p[..., 1].sum(-1) if partials_rounded else 0.0)
    var = m2_ref / D + 1e-6
    Ev = EM / D + U * m2_ref / D + U * var + (U * 1e-6 if partials_rounded else 0.0)
    rel = np.maximum(np.sqrt(var / np.maximum(var - Ev, 1e-6 * (1.0 - 2.0 * U))) - 1.0, 1.0 - np.sqrt(var / (var + Ev))) + rsqrt_rel
    return Em, rel


# ---- the wrong formulas (negative controls) -----------------------------------------------------------------------------------------------------------------

def _rstd_of(m2, D):
    var = fma32(np.asarray(m2, F32), inv_d(D), EPS32)
    with np.errstate(all='ignore'):
        return (1.0 / np.sqrt(np.maximum(var.astype(F64), 0.0))).astype(F32)


def rstd_one_pass(p, D):
    """sum_g (M2_g + s_g^2 / 64) - s1^2 / D in float32"""
    p = np.asarray(p, F32)
    s1 = np.zeros(p.shape[:-2], F32)
    q = np.zeros_like(s1)
    for t in range(p.shape[-2]):
        s = p[..., t, 0]
        s1 = (s1 + s).astype(F32)
        q = (q + fma32((s * INV64).astype(F32), s, p[..., t, 1])).astype(F32)
    with np.errstate(all='ignore'):
        return _rstd_of((q - ((s1 * s1).astype(F32) * inv_d(D)).astype(F32)).astype(F32), D)


def rstd_no_between(p, D):
    """the merge without the 64 d^2 term: sum_g M2_g"""
    p = np.asarray(p, F32)
    m2 = np.zeros(p.shape[:-2], F32)
    for t in range(p.shape[-2]):
        m2 = (m2 + p[..., t, 1]).astype(F32)
    return _rstd_of(m2, D)


def merge_two_roundings(p, D):
    """d = fl(fl(s_g * 1/64) - mean) instead of the fma: (mean, rstd)"""
    p = np.asarray(p, F32)
    mean, _, _ = merge(p, D)
    m2 = np.zeros_like(mean)
    for t in range(p.shape[-2]):
        d = ((p[..., t, 0] * INV64).astype(F32) - mean).astype(F32)
        m2 = (m2 + fma32((F32(64.0) * d).astype(F32), d, p[..., t, 1])).astype(F32)
    return mean, _rstd_of(m2, D)


# ---- the fold in a GEMM epilogue: float64 reference and per-element bound ------------------------------------------------------------------------------------

U16 = {'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8}         # unit roundoff of the 16-bit output
GELU_FIT = 1.2e-6                                     # |gelu_core - GELU| in float32 (csrc/common.h)
GELU_LIP = 1.13                                       # max |GELU'| = 1.1290 (at x = 1.414): what an error of GELU's argument can grow by


def gelu64(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def fold_reference(hi, W, ln_s, bias, mean, rstd, epi, dtype):
    """float64 rstd (sum_k hi_k W'_k - mean s_n) + b_n (GELU for epi 1) on the float32 statistics given, and the bound on |device - reference| per element:

        E  = rstd (K 2^-24 sum_k |hi_k W'_k| + 2^-23 |mean s_n|) + 2^-24 |v|      v = the pre-GELU value
             (any-order float32 accumulation of K exact products, MFMA-internal alignment included; the two roundings the inner fma's result carries
              relative to mean s_n and acc; the outer fma's rounding)
        epi 1: E <- 1.13 E + 1.2e-6        (GELU's Lipschitz constant carries the argument's error, then the fit's own error)
        bound = E + u16 (|ref| + E) + eta  (one rounding to the 16-bit output; eta = 2^-25 where fp16 is subnormal, 0 for bf16)"""
    hi64, W64 = np.asarray(hi, F64), np.asarray(W, F64)
    K = hi64.shape[1]
    mean, rstd = np.asarray(mean, F64)[:, None], np.asarray(rstd, F64)[:, None]
    s, b = np.asarray(ln_s, F64)[None, :], np.asarray(bias, F64)[None, :]
    acc = hi64 @ W64.T
    mag = np.abs(hi64) @ np.abs(W64).T
    v = rstd * (acc - mean * s) + b
    E = rstd * (K * U * mag + 2.0 * U * np.abs(mean * s)) + U * np.abs(v)
    ref = v
    if epi == 1:
        ref = gelu64(v)
        E = GELU_LIP * E + GELU_FIT
    bound = E + U16[dtype] * (np.abs(ref) + E) + (2.0 ** -25 if dtype == 'fp16' else 0.0)
    return ref, bound, mag


def layernorm_reference(v, hi, W, bias, epi, dtype, fold_bound, rstd):
    """float64 LayerNorm(hi + lo) W'^T + b (gamma and beta live in W' and b) and the bound on |device - it|: the fold normalises x rounded to 16 bits (the hi
    plane), so it differs from the true LayerNorm's product by at most rstd u16 sum_k |v_k| |W'_k| (|hi - v| <= u16 |v|), on top of the fold's own bound."""
    v64, W64 = np.asarray(v, F64), np.asarray(W, F64)
    mean, _, rs = two_pass_fp64(v64)
    ref = ((v64 - mean[:, None]) * rs[:, None]) @ W64.T + np.asarray(bias, F64)[None, :]
    extra = np.asarray(rstd, F64)[:, None] * U16[dtype] * (np.abs(v64) @ np.abs(W64).T)
    if epi == 1:
        ref = gelu64(ref)
        extra = GELU_LIP * extra
    return ref, fold_bound + extra * (1.0 + U16[dtype])
