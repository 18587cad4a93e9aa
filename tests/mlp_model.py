"""Host model of the MLP pair's own arithmetic (csrc/common.h: gelu_core / gelu_sat behind fc1, the 16-bit conversion of `hid`; the accumulation and the
producer row behind fc2).  A plain module: tests/test_mlp_model.py pins it on the CPU, tests/test_gpu_mlp.py compares every GELU site and both GEMMs with it.

    a = |x|, q = (((c4 a + c3) a + c2) a + c1) a + c0     four fmas, the float32 coefficients of common.h
    h = exp2(fma(-q, a, -1))                              v_exp_f32: the factor 1/2 rides in the exponent
    r = fma(-a, h, relu)                                  relu = max(x, 0); fp16: med3(x, 0, 65504)
    out = round16(r)                                      round to nearest even, fp16 subnormals kept; no clamp left to do

fit64 is that function with every operation exact (float64); the device may differ from it by the float32 evaluation alone, at most

    E32 = a h (ln2 2^-23 (5 a |q| + 1) + 2^-21) + 2^-23 |r|

every rounding counted as a whole float32 ulp 2^-23 of its result (twice the unit roundoff):
    q          four fma roundings, each at most 2^-23 |q| (the partial sums of the Horner chain stay below |q|: c3 < 0 is the one negative coefficient, and the
               chain runs from the small terms to the large), carried into the exponent by the factor a:  4 a |q| 2^-23
    e          e = fma(-q, a, -1) rounds once, |e| = a |q| + 1:  (a |q| + 1) 2^-23.  Together |de| <= 2^-23 (5 a |q| + 1), and h = 2^e moves by ln2 |de| h
    exp2       v_exp_f32 against an exact exp2 of the float32 argument: 4 ulp = 2^-21 h (the documented 1 ulp with room for the denormal-result range)
    r          both enter r scaled by a; the last fma rounds once: 2^-23 |r|
    denormal h where 2^-150 <= h < 2^-126 (a from 11.4 to 12.5) the result of exp2 is a float32 denormal: rounded to a multiple of 2^-149, or flushed to 0 by a
               device that does not keep denormal results -- an absolute a 2^-126 covers both (1e-37: below every 16-bit value here)
The constants are pinned on the CPU (tests/test_mlp_model.py): the float32 emulation emu32 -- numpy float32 fmas, an exact exp2 -- stays within 0.5 E32 on
every sweep input of both types, which leaves the other half for the hardware's exp2 and for contraction differences.

Two ranges in which float32 leaves NOTHING open; the continuous form above would call every 16-bit tie in them undecided, and the sweep is full of such ties
(s = 1.5 times a pattern with an odd significand is a tie of the type: 1.6 % of the bf16 inputs below 1e-6, 1 % of the fp16 inputs above 16):
    tiny     a q <= 2^-25: the exact exponent -1 - a q lies within half an ulp of -1, so e = fma(-q, a, -1) IS -1; h = exp2(-1) = 1/2 (supposed of v_exp_f32:
             exact on an integer argument), and r = fma(-a, 1/2, relu) = x / 2 exactly (a float32 wherever x is one: a power-of-two scaling; below 2^-148 one
             denormal rounding, which no 16-bit value sees).  The device's value is x / 2, not fit64's x / 2 (1 + 0.8 a): out == round16(x / 2), ties to even.
    far      a q + 1 >= 151: h < 2^-150, half the smallest float32 denormal; the exponent's error (<= 2^-23 (5 a q + 1), 1e-4 at the most) does not bring it
             back, so exp2 returns 0 (or a few denormal ulps: a 2^-147 is far below half an ulp of relu = a) and r = relu exactly:
             out == round16(min(x, 65504)) (fp16) / round16(x) (bf16) for x > 0 -- this is where the saturation branch and bf16's rows of 2 w are decided.
In both ranges centre() is the exact value and E32 is 0.

Acceptance of a 16-bit output (rounding is monotone):  round16(centre - E32) <= got <= round16(centre + E32), zeros equal whatever their sign.  Where the two
ends agree the output bits are decided."""
import numpy as np

import ln_consumer_model as LM
import residual_row_model as RM

F32, F64 = np.float32, np.float64
C = tuple(F32(c) for c in (5.204574411e-04, -7.397505390e-03, 5.256122897e-02, 4.592546873e-01, 1.151091354e+00))     # common.h::gelu_core, highest degree first
F16_MAX = 65504.0
LN2 = float(np.log(2.0))
PREC = {'fp16': (11, -14), 'bf16': (8, -126)}        # significand bits, exponent of the smallest normal


def is16(dtype):
    return dtype in ('fp16', 'f16')


def round16(v, dtype):
    """float64 -> the nearest value of the 16-bit type (ties to even, gradual underflow), as float64; fp16 clamps at +-65504, bf16 overflows to inf"""
    v = np.asarray(v, F64)
    p, emin = PREC[dtype]
    with np.errstate(all='ignore'):
        _, e = np.frexp(v)                                                  # v = m 2^e, 0.5 <= |m| < 1
        q = np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))                # the spacing of the type at v
        r = np.rint(v / q) * q                                              # v / q is exact (a power of two, no underflow: q >= 2^-133)
    if is16(dtype):
        return np.clip(r, -F16_MAX, F16_MAX)
    big = float(RM.from_bits(np.array([0x7f7f], np.uint16), 'bf16')[0])
    return np.where(np.abs(r) > big, np.copysign(np.inf, r), r)


def _relu(x, dtype):
    return np.clip(x, 0.0, F16_MAX) if is16(dtype) else np.maximum(x, 0.0)


def parts64(x, dtype):
    """(a, q, h, r) of the fit with every operation exact"""
    x = np.asarray(x, F64)
    a = np.abs(x)
    with np.errstate(all='ignore'):
        q = np.full_like(a, float(C[0]))
        for c in C[1:]:
            q = q * a + float(c)
        h = np.exp2(-q * a - 1.0)
        r = _relu(x, dtype) - a * h
    return a, q, h, r


def fit64(x, dtype):
    return parts64(x, dtype)[3]


def ranges(x):
    """(tiny, far): the two ranges in which the float32 evaluation is exact (module docstring)"""
    a, q, _, _ = parts64(x, 'bf16')
    with np.errstate(all='ignore'):
        return a * q <= 2.0 ** -25, a * q + 1.0 >= 151.0


def centre(x, dtype):
    """what the device evaluates, exactly: fit64, and x / 2 in the tiny range"""
    x = np.asarray(x, F64)
    return np.where(ranges(x)[0], 0.5 * x, fit64(x, dtype))


def e32(x, dtype):
    a, q, h, r = parts64(x, dtype)
    tiny, far = ranges(x)
    with np.errstate(all='ignore'):
        ah = np.where(h > 0, a * h, 0.0)
        E = ah * (LN2 * 2.0 ** -23 * (5.0 * a * np.abs(q) + 1.0) + 2.0 ** -21) + 2.0 ** -23 * np.abs(r) + np.where(h < 2.0 ** -126, a * 2.0 ** -126, 0.0)
    return np.where(tiny | (far & (np.asarray(x) > 0)), 0.0, np.where(far, a * 2.0 ** -147, E))


def emu32(x, dtype, relu=None, exp2=None):
    """gelu_core in float32: numpy float32 fmas (LM.fma32: one rounding each) and an exact exp2 rounded to float32; relu / exp2: a mutant's own"""
    x = np.asarray(x, F32)
    a = np.abs(x)
    with np.errstate(all='ignore'):
        q = LM.fma32(a, C[0], C[1])
        for c in C[2:]:
            q = LM.fma32(q, a, c)
        e = LM.fma32(-q, a, F32(-1.0))
        h = (exp2 or (lambda t: np.exp2(t.astype(F64)).astype(F32)))(e)
        rl = _relu(x, dtype).astype(F32) if relu is None else relu(x)
        return LM.fma32(-a, h, rl)


def interval(x, dtype):
    """(lo, hi): the 16-bit values an output may take for the float32 pre-activation x"""
    f, E = centre(x, dtype), e32(x, dtype)
    return round16(f - E, dtype), round16(f + E, dtype)


def implied_ratio(x, got, dtype):
    """What a 16-bit output tells of the float32 value behind it: the least |r - centre| / E32 over the r that round to got (0 where centre itself rounds to got;
    inf where E32 = 0 and it does not), for x >= -8; the tail is 0.  <= 1 everywhere is the interval acceptance; the worst value is the figure DESIGN quotes."""
    x64, got = np.asarray(x, F32).astype(F64), np.asarray(got, F32)
    b = RM.to_bits(got, dtype).astype(np.int64)
    k = np.where(b & 0x8000, -(b & 0x7fff), b & 0x7fff)                     # the patterns in value order; both zeros are 0
    back = lambda s: RM.from_bits(np.where(s < 0, 0x8000 | -s, s).astype(np.uint16), dtype).astype(F64)
    g = got.astype(F64)
    with np.errstate(all='ignore'):
        below, above = (g + back(k - 1)) / 2.0, (g + back(k + 1)) / 2.0     # the rounding boundaries of got (fp16 at 65504: above = inf, the clamp)
        if is16(dtype):
            above = np.where(g >= F16_MAX, np.inf, above)
            below = np.where(g <= -F16_MAX, -np.inf, below)
        c, E = centre(x64, dtype), e32(x64, dtype)
        d = np.maximum(np.maximum(below - c, c - above), 0.0)
        r = np.where(d == 0, 0.0, np.where(E > 0, d / E, np.inf))
    return np.where(x64 < -8.0, 0.0, r)


def to16(r, dtype):
    """the device's conversion of the float32 result: round to nearest even to the type (fp16 keeps subnormals; r is already inside the fp16 range)"""
    return RM.from_bits(RM.to_bits(np.asarray(r, F32), dtype), dtype)


def accept(x, got, dtype):
    """The whole acceptance of part A on pre-activations x (finite float32) and outputs got, elementwise -> (bad, undecided share on x >= -8).
    x < -8: -1e-14 <= got <= 0 and nothing more.  fp16, x > 65504: got == 65504.  bf16, x > 16: got == round16(x).  Elsewhere the interval."""
    x = np.asarray(x, F32).astype(F64)
    got = np.asarray(got, F64)
    lo, hi = interval(x, dtype)
    with np.errstate(all='ignore'):
        bad = ~((got >= lo) & (got <= hi))
        tail = x < -8.0
        bad = np.where(tail, ~((got >= -1e-14) & (got <= 0.0)), bad)
        if is16(dtype):
            bad |= (x > F16_MAX) & (got != F16_MAX)
        else:
            bad |= (x > 16.0) & (got != round16(x, dtype))
        bad |= ~np.isfinite(got)
    return bad, float((lo != hi)[~tail].mean())


def monotone(x, got):
    """over the sorted x: equal x give equal outputs, outputs non-decreasing for x >= -0.7 and non-increasing for x <= -0.8 -> number of violations"""
    x, got = np.asarray(x, F64).ravel(), np.asarray(got, F64).ravel()
    o = np.argsort(x, kind='stable')
    xs, g = x[o], got[o]
    d, same = np.diff(g), np.diff(xs) == 0
    up, down = xs[:-1] >= -0.7, xs[1:] <= -0.8
    return int((same & (d != 0)).sum() + (up & (d < 0)).sum() + (down & (d > 0)).sum())


# ---- the mutants (negative controls): what a kernel could run instead, as (float32 result, 16-bit output) ---------------------------------------------------

def _sig(t):
    return 1.0 / (1.0 + np.exp(-t))


def mutants(x, dtype):
    """name -> the 16-bit outputs (as float64) of a subtly wrong kernel on the float32 pre-activations x"""
    x = np.asarray(x, F32)
    x64 = x.astype(F64)
    good = emu32(x, dtype)
    out = {}
    with np.errstate(all='ignore'):
        sat = lambda v: np.clip(v, -np.inf, F16_MAX) if is16(dtype) else v
        t = 0.5 * x64 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x64 + 0.044715 * x64 ** 3)))
        out['tanh-approximate GELU'] = to16(sat(np.where(np.abs(x64) > 30, np.maximum(x64, 0.0), t)).astype(F32), dtype)
        out['x sigmoid(1.702 x)'] = to16(sat(x64 * _sig(1.702 * x64)).astype(F32), dtype)
        out['0 for x < -3.5'] = to16(np.where(x < -3.5, F32(0), good), dtype)
        if is16(dtype):
            unclamped = emu32(x, dtype, relu=lambda v: np.maximum(v, F32(0)))
            out['max(x, 0) without the fp16 clamp'] = RM.from_bits(RM.to_bits(unclamped, dtype), dtype).astype(F64)          # to_bits does not clamp: inf at 131008
        out['truncating conversion'] = truncate16(good, dtype)
        if is16(dtype):
            c = to16(good, dtype).astype(F64)
            out['fp16 subnormals flushed'] = np.where(np.abs(c) < 2.0 ** -14, 0.0, c)
        out['one fused rounding'] = fused16(x, dtype)
    return {k: np.asarray(v, F64) for k, v in out.items()}


def truncate16(r, dtype):
    """round toward zero to the type"""
    r = np.asarray(r, F64)
    p, emin = PREC[dtype]
    _, e = np.frexp(r)
    q = np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))
    return np.trunc(r / q) * q


def fused16(x, dtype):
    """v_fma_mix*: fma(-a, h, relu) rounded ONCE to 16 bits, from the float32 a, h and relu of the emulation"""
    x = np.asarray(x, F32)
    a = np.abs(x)
    with np.errstate(all='ignore'):
        q = LM.fma32(a, C[0], C[1])
        for c in C[2:]:
            q = LM.fma32(q, a, c)
        h = np.exp2(LM.fma32(-q, a, F32(-1.0)).astype(F64)).astype(F32)
        exact = _relu(x, dtype).astype(F64) - a.astype(F64) * h.astype(F64)     # 24 x 24 bits + one add: exact in float64 but for a last bit that no 16-bit tie sees
    return round16(exact, dtype)


# ---- fc2: float64 reference and per-element bound ----------------------------------------------------------------------------------------------------------

def fc2_reference(A, W, bias, resid, dtype):
    """float64 A W^T + b + (hi + lo) with the residual as the two planes hold it, and the bound on |device (hi + lo) - reference| per element:

        K 2^-24 sum_k |a_k w_k|           any-order float32 accumulation of K exact products
      + 2^-24 |st|                        st = fl32(acc + b)                          (residual_row_model: the caller's add)
      + 2^-24 |v|                         v = fl32(st + r); r = fl32(hi + lo) is exact for planes that a split wrote
      + u16^2 |v| + eta                   lo = round16(v - hi) with |v - hi| <= u16 |v|; eta = 2^-25 where fp16's lo is subnormal, 0 for bf16
    all times (1 + 2^-10) for the second-order terms (|st| and |v| are taken from the reference)."""
    A64, W64 = np.asarray(A, F64), np.asarray(W, F64)
    K = A64.shape[1]
    hi = RM.from_bits(RM.to_bits(resid, dtype), dtype)
    lo = RM.from_bits(RM.to_bits((np.asarray(resid, F32) - hi).astype(F32), dtype), dtype)
    st = A64 @ W64.T + np.asarray(bias, F64)[None, :]
    ref = st + (hi.astype(F64) + lo.astype(F64))
    mag = np.abs(A64) @ np.abs(W64).T
    u16 = LM.U16[dtype]
    bound = (K * LM.U * mag + LM.U * np.abs(st) + LM.U * np.abs(ref) + u16 * u16 * np.abs(ref) + (2.0 ** -25 if is16(dtype) else 0.0)) * (1.0 + 2.0 ** -10)
    return ref, bound
