"""The inputs of the producer-row tests (tests/test_residual_row_model.py on the CPU, tests/test_gpu_residual_row.py on the device): ONE problem
of 512 x 1280 per 16-bit type; every site runs a prefix [M, N] of it at its own K, so all sites see the same (st, r) on their common rows.

Operands.  st must be known exactly whatever order a kernel accumulates in: A is k / 8 with |k| <= 16 (four significant bits, so MXFP8 holds it
too), W is sparse in {+-1/8, +-1/4} with one +-7/16 per row (the fp8 packer's scale amax / 448 is then 2^-10), so every partial sum is exact in
fp32 and acc is the same number at every site; the many-bit part is the fp32 bias: st = fl32(acc + bias), one modelled rounding.  The 64
columns of the base problem sit at k = j K / 64 of a site's K; the other k carry zeros in W.

Columns (n % 64; `quiet` = a zero row of W, st = bias on every row):
    n % 8 == 5      quiet, bias +0: v = r exactly, whatever the planes hold (n % 64 == 13: bias -0, and st is +0 all the same)
    n % 8 == 3      quiet, bias = a full fp32 significand at 2^-3 .. 2^-26: st itself is the small many-bit value
    n % 64 == 6     quiet, bias 16: a positive st under hi = 65504
    n % 8 == 2      bias k / 16: st has few bits, so that r = -st exists as planes (full cancellation)
    granules 4, 10, 16: quiet with bias +0 on all 64 columns (v = r): the only place where 64 values can be made EQUAL whatever st is
    5 columns of every ODD granule: quiet, bias = a huge value (fp16: the saturation list up to 3e38; bf16: up to 1e18)
    n % 64 == 20 of every odd granule: a dense row of W (7/8, 1/2, 1/2, ...): 2048 x 32.4 in the huge rows
Rows (m % 8; the variant m // 8 walks the lists):
    0 ordinary N(0, 2)      1 saturation / large values through r      2, 3 common offset +c / -c, one constant granule      4 small magnitudes
    5 r = -st (cancellation), zeros of both signs      6 association: st + (hi + lo) != (st + hi) + lo in the plane bits      7 arbitrary finite plane bits
    m % 64 in (40, 41): A = 2048 on the whole row (a huge st from powers of two)
The even granules hold no huge-bias column: the offset rows keep a small M2 there.  Rows 2, 3 (bf16: and 1, with +-1e30) hold one constant in the quiet granules."""
import functools

import numpy as np

import residual_row_model as RM

F32 = np.float32
M_MAX, N_MAX, K0 = 512, 1280, 64
HUGE_COLS = (7, 23, 40, 55, 60)
DENSE_COL = 20
OFFSETS = {'fp16': (250.0, 1000.0, 30000.0), 'bf16': (250.0, 1000.0, 1e5)}
SAT = {'fp16': (65504.0, 65519.9, 65520.0, 7e4, 1e6, 3e38, 65503.9),                 # through the bias (a huge st)
       'bf16': (7e4, 1e6, 1e9, 1e12, 1e15, 1e18, 3e4)}
# through the planes (hi = 65504 and a positive rest).  fp16 planes hold |hi + lo| <= 131008, so 1e6 and 3e38 are reached through the bias only (SAT);
# 1e5 and 65535 stand in their place here
SAT_R = {'fp16': (65504.0, 65519.9, 65520.0, 7e4, 65503.9, 1e5, 65535.0),
         'bf16': (7e4, 1e6, 1e9, 1e12, 1e15, 1e18, 3e4)}
BF16_CONST = 1e30                                                                       # bf16: a whole granule of it (M2 of a mixed granule, 1e60, has no fp32)
QUIET_GRANULES = (4, 10, 16)                                                            # wholly quiet with bias +0 (v = r on every row): the constant granules live here


def _signed(lst, i):
    return lst[i % len(lst)] * (1.0 if (i // len(lst)) % 2 == 0 else -1.0)


@functools.lru_cache(maxsize=None)
def operands():
    """A0 [512, 64], W0 [1280, 64], acc [512, 1280] (exact), the unit every |a||w| of a row is a multiple of"""
    rng = np.random.default_rng(20260101)
    A0 = (rng.integers(-16, 17, size=(M_MAX, K0)) / 8.0).astype(F32)
    huge = np.isin(np.arange(M_MAX) % 64, (40, 41))
    A0[huge] = 2048.0
    W0 = (rng.choice([0.125, -0.125, 0.25, -0.25], size=(N_MAX, K0)) * (rng.random((N_MAX, K0)) < 0.25)).astype(F32)
    W0[np.arange(N_MAX), rng.integers(0, K0, N_MAX)] = rng.choice([7.0 / 16, -7.0 / 16], N_MAX)
    n = np.arange(N_MAX)
    odd = (n // 64) % 2 == 1
    quiet = (n % 8 == 5) | (n % 8 == 3) | (n % 64 == 6) | (odd & np.isin(n % 64, HUGE_COLS)) | np.isin(n // 64, QUIET_GRANULES)
    W0[quiet] = 0.0
    dense = odd & (n % 64 == DENSE_COL)
    W0[dense] = 0.5
    W0[dense, 0] = 7.0 / 8
    acc = (A0.astype(np.float64) @ W0.astype(np.float64).T) + 0.0      # + 0.0: a zero accumulator is +0
    unit = np.where(huge, 2048.0, 1.0 / 8)[:, None] * (1.0 / 16)
    return A0, W0, acc, unit, huge


def site_operands(M, N, K, fill_seed=0):
    """A [M, K], W [N, K] of a site: the base columns at k = j K / 64; elsewhere W is zero and A carries more k / 8 (2048 in the huge rows)"""
    A0, W0, _, _, huge = operands()
    s = K // K0
    rng = np.random.default_rng(1000 + K + fill_seed)
    A = (rng.integers(-16, 17, size=(M, K)) / 8.0).astype(F32)
    A[huge[:M]] = 2048.0
    A[:, ::s] = A0[:M]
    W = np.zeros((N, K), F32)
    W[:, ::s] = W0[:N]
    return A, W


def _planes_of(x, dtype):
    """the planes a producer would have written for x (fp16: saturating both planes), as bits"""
    x = np.asarray(x, dtype=np.float64)
    lim = 65504.0 if dtype == 'fp16' else 3.0e38
    hi = RM.to_bits(np.clip(x, -lim, lim).astype(F32), dtype)
    lo = RM.to_bits(np.clip(x - RM.from_bits(hi, dtype).astype(np.float64), -lim, lim).astype(F32), dtype)
    return hi, lo


@functools.lru_cache(maxsize=None)
def problem(dtype):
    """dict: bias [N], st [M, N] (fp32, exact model of acc + bias), r_hi / r_lo bits [M, N], the class masks and the constant-granule table"""
    A0, W0, acc, unit, huge = operands()
    rng = np.random.default_rng(7 if dtype == 'fp16' else 8)
    m = np.arange(M_MAX)[:, None]
    n = np.arange(N_MAX)[None, :]
    cls, var = m % 8, m // 8
    gran = n // 64
    odd = gran % 2 == 1
    # ---- bias
    bias = (rng.standard_normal(N_MAX) * 0.3).astype(F32)
    n1 = n[0]
    few = n1 % 8 == 2
    bias[few] = (rng.integers(-32, 33, few.sum()) / 16.0).astype(F32)
    bias[n1 % 8 == 5] = 0.0
    tiny_b = n1 % 8 == 3
    bias[tiny_b] = (np.exp2(-(3.0 + (n1[tiny_b] // 8) % 24)) * (1.0 + rng.random(tiny_b.sum())) * rng.choice([-1.0, 1.0], tiny_b.sum())).astype(F32)
    bias[n1 % 64 == 6] = 16.0
    bias[np.isin(n1 // 64, QUIET_GRANULES)] = 0.0
    bias[(n1 % 64 == 13) & ~np.isin(n1 // 64, QUIET_GRANULES)] = -0.0   # the nearest a site comes to v = -0: acc (+0) + bias (-0) = +0, so r = -0 must still give +0
    hb = np.zeros(N_MAX, bool)
    for j, col in enumerate(HUGE_COLS):
        sel = ((n1 // 64) % 2 == 1) & (n1 % 64 == col)
        idx = (n1[sel] // 128) * len(HUGE_COLS) + j
        bias[sel] = np.array([_signed(SAT[dtype], int(i)) for i in idx], F32)
        hb |= sel
    st = (acc + bias.astype(np.float64)[None, :]).astype(F32)           # fl32(acc + bias): acc is exact, one rounding
    # ---- the value each element aims at; r = planes of (target - st)
    target = rng.standard_normal((M_MAX, N_MAX)) * 2.0                   # classes 0, 6, 7 and whatever a class leaves alone
    # 1: saturation / large values through the planes
    c1 = (cls == 1) & ((n % 8 == 1) | (n % 8 == 5) | (n % 64 == 6))
    t1 = np.array([_signed(SAT_R[dtype], i) for i in range(2 * len(SAT_R[dtype]))])[(n // 8 + var) % (2 * len(SAT_R[dtype]))]
    target = np.where(c1, t1, target)
    # 2, 3: common offset
    off = np.array(OFFSETS[dtype])[var % 3] * np.where(cls == 2, 1.0, -1.0)
    isoff = (cls == 2) | (cls == 3)
    target = np.where(isoff, off + rng.standard_normal((M_MAX, N_MAX)), target)
    # 4: small magnitudes, 2^-3 .. 2^-26 with a full fp32 significand
    small = np.exp2(-(3.0 + (n // 8 + var) % 24)) * (1.0 + rng.random((M_MAX, N_MAX))) * rng.choice([-1.0, 1.0], (M_MAX, N_MAX))
    target = np.where(cls == 4, small.astype(F32).astype(np.float64), target)
    # 5: cancellation
    target = np.where(cls == 5, 0.0, target)
    # the constant granules: offset rows (the offset itself) and, bf16, class 1 rows (1e30)
    rows = np.arange(M_MAX)
    const_rows = np.isin(rows % 8, (2, 3)) | ((rows % 8 == 1) if dtype == 'bf16' else False)
    cmask = const_rows[:, None] & np.isin(gran, QUIET_GRANULES)
    cval = np.where(isoff, off, BF16_CONST * np.where(var % 2 == 0, 1.0, -1.0))
    target = np.where(cmask, cval, target)
    r_hi, r_lo = _planes_of(target - st.astype(np.float64), dtype)
    # 5: zeros of both signs and the smallest codes on the quiet columns (st = +0: v = r)
    z = (cls == 5) & (n % 8 == 5)
    zi = (n // 8 + var) % 4
    tiny = 0x0001 if dtype == 'fp16' else 0x2B80      # fp16: the smallest subnormal; bf16: 2^-40 (its smallest codes are fp32 subnormals, whose squares no fp32 M2 holds)
    r_hi = np.where(z, np.choose(zi, [0x0000, 0x8000, tiny, 0x8000 | tiny]), r_hi).astype(np.uint16)
    r_lo = np.where(z, np.choose(zi, [0x0000, 0x8000, 0x8000 | tiny, 0x0000]), r_lo).astype(np.uint16)
    # 4: ... and v = st itself on the tiny-bias columns: all 24 bits at every magnitude down to 2^-26
    z4 = (cls == 4) & (n % 8 == 3)
    r_hi = np.where(z4, 0, r_hi).astype(np.uint16)
    r_lo = np.where(z4, 0, r_lo).astype(np.uint16)
    # 7: arbitrary finite plane bits (no producer wrote them): any sign, exponent field up to 2^5, any significand
    c7 = np.broadcast_to(cls == 7, (M_MAX, N_MAX))
    if dtype == 'fp16':
        rb = lambda: (rng.integers(0, 2, (M_MAX, N_MAX)) << 15) | (rng.integers(0, 21, (M_MAX, N_MAX)) << 10) | rng.integers(0, 1024, (M_MAX, N_MAX))
    else:
        rb = lambda: (rng.integers(0, 2, (M_MAX, N_MAX)) << 15) | (rng.integers(100, 133, (M_MAX, N_MAX)) << 7) | rng.integers(0, 128, (M_MAX, N_MAX))
    r_hi = np.where(c7, rb(), r_hi).astype(np.uint16)
    r_lo = np.where(c7, rb(), r_lo).astype(np.uint16)
    # 6: association -- a fixed-seed search for planes where (st + hi) + lo gives other plane bits than st + (hi + lo).  The two orders differ where a
    # rounding of st + hi (or of hi + lo) falls differently, and the planes show it where lo of the OUTPUT resolves one fp32 ulp of v.  Three rounds of four:
    # hi = 2^u |st| (u from where st loses bits in the sum up to where v - hi still fits lo's significand) under a lo of a few ulps of the sum; the
    # fourth: the planes of V - st for a V that 16 bits hold.
    rows6 = np.flatnonzero(rows % 8 == 6)
    st6 = st[rows6]
    sh = st6.shape
    h6, l6 = r_hi[rows6].copy(), r_lo[rows6].copy()
    found6 = np.zeros(sh, bool)
    u_lo, u_hi, lim = (2, 13, 6e4) if dtype == 'fp16' else (16, 22, 1e15)
    for it in range(48):
        if it % 4:
            H = np.abs(st6) * np.exp2(rng.integers(u_lo, u_hi, sh)) * (1.0 + rng.random(sh)) * rng.choice([-1.0, 1.0], sh)
            ch = RM.to_bits(np.clip(H, -lim, lim).astype(F32), dtype)
            cl = RM.to_bits((RM.from_bits(ch, dtype) * np.exp2(-(18.0 + 6.0 * rng.random(sh))) * rng.choice([-1.0, 1.0], sh)).astype(F32), dtype)
        else:
            V = RM.from_bits(RM.to_bits((rng.standard_normal(sh) * np.exp2(rng.integers(-2, 9, sh))).astype(F32), dtype), dtype)
            ch, cl = _planes_of(V.astype(np.float64) - st6.astype(np.float64), dtype)
        _, h_ok, l_ok = RM.row(st6, RM.decode(ch, cl, dtype), dtype)
        _, h_w, l_w = wrong_association(st6, ch, cl, dtype)
        hit = ~found6 & ((h_ok != h_w) | (l_ok != l_w))
        h6[hit], l6[hit] = ch[hit], cl[hit]
        found6 |= hit
    r_hi[rows6], r_lo[rows6] = h6, l6
    found = np.zeros((M_MAX, N_MAX), bool)
    found[rows6] = found6
    return dict(bias=bias, st=st, r_hi=np.ascontiguousarray(r_hi), r_lo=np.ascontiguousarray(r_lo), cls=np.broadcast_to(cls, (M_MAX, N_MAX)),
                assoc=found, const_rows=const_rows, huge_bias=hb, offset=np.where(isoff[:, 0], off[:, 0], 0.0), quiet0=(n1 % 8 == 5), tiny_bias=tiny_b, neg0_bias=np.signbit(bias) & (bias == 0))


def wrong_association(st, hi_bits, lo_bits, dtype):
    """the row with (st + hi) + lo instead of st + (hi + lo) (negative control)"""
    x = ((np.asarray(st, F32) + RM.from_bits(hi_bits, dtype)).astype(F32) + RM.from_bits(lo_bits, dtype)).astype(F32)
    return RM.split(x, dtype)


@functools.lru_cache(maxsize=None)
def model(dtype):
    """the model's answer on the whole problem: v, hi, lo bits, s1, s2 (model), fp64 M2 and mean, its bound"""
    p = problem(dtype)
    v, hi, lo = RM.row(p['st'], RM.decode(p['r_hi'], p['r_lo'], dtype), dtype)
    return _stats(v, hi, lo)


def _stats(v, hi, lo):
    s1 = RM.granule_s1(v)
    m2, mean = RM.m2_fp64(v)
    return dict(v=v, hi=hi, lo=lo, s1=s1, s2=RM.granule_m2(v, s1), m2=m2, mean=mean, bound=RM.m2_bound(m2, mean))


@functools.lru_cache(maxsize=None)
def model_pos(dtype, M, N):
    """patch embed (EPI_POS_LN): no bias, r = the fp32 pos[m % 192]; pos is what the planes of the problem stand for on its first 192 rows"""
    p = problem(dtype)
    _, _, acc, _, _ = operands()
    pos = RM.decode(p['r_hi'][:192, :N], p['r_lo'][:192, :N], dtype)
    v, hi, lo = RM.row(acc[:M, :N].astype(F32), pos[np.arange(M) % 192], dtype)
    return pos, _stats(v, hi, lo)
