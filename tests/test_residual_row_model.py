"""CPU: the host model of the residual producer row (tests/residual_row_model.py) and the inputs the device test feeds it
(tests/residual_row_cases.py), pinned before any GPU time is spent: the planes hold v, the tree statistics meet their bounds against fp64, the
two wrong formulas the device test must catch (one-pass M2, the other association) demonstrably fail here, and the operands are exact."""
import numpy as np
import pytest

import residual_row_cases as RC
import residual_row_model as RM

F32 = np.float32
DTYPES = ('fp16', 'bf16')
SMALL = (slice(0, 200), slice(0, 384))          # the smallest site's part of the problem: every class must live there


def _ratio(err, bound):
    with np.errstate(all='ignore'):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


@pytest.mark.parametrize('dtype', DTYPES)
def test_planes_hold_v(dtype):
    """hi + lo reproduces the stored v on every class: to 2^-18 |v| (fp16: 11 + 11 bits leave 2^-22; below 2^-7 the lo plane is a subnormal of spacing
    2^-24, so half of that) / 2^-14 |v| (bf16: 8 + 8 bits leave 2^-18), and exactly where v has no more bits than the two planes."""
    m = RC.model(dtype)
    v = m['v'].astype(np.float64)
    back = RM.from_bits(m['hi'], dtype).astype(np.float64) + RM.from_bits(m['lo'], dtype).astype(np.float64)
    tol = np.maximum(2.0 ** -18 * np.abs(v), 2.0 ** -25) if dtype == 'fp16' else 2.0 ** -14 * np.abs(v)
    assert (np.abs(back - v) <= tol).all(), f'worst {_ratio(np.abs(back - v), tol).max():.3f}'
    bits = m['v'].view(np.uint32)
    few = (bits & (0x3 if dtype == 'fp16' else 0xff)) == 0                 # 22 / 16 significant bits at most
    if dtype == 'fp16':
        few &= np.abs(m['v']) >= 2.0 ** -3                                 # ... all of them on fp16's grid
    assert few.sum() > 50000 and (back[few] == v[few]).all()
    for cls in range(8):
        assert few[RC.problem(dtype)['cls'] == cls].sum() > 100, cls
    assert np.isfinite(back).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_tree_statistics_against_fp64(dtype):
    """s1: six levels of pairwise adds, each within 2^-24 of a partial sum of at most sum |v|; s2: the bound the device test asserts (m2_bound)."""
    m = RC.model(dtype)
    g = m['v'].astype(np.float64).reshape(RC.M_MAX, -1, 64)
    assert (np.abs(m['s1'] - g.sum(-1)) <= 6 * 2.0 ** -24 * np.abs(g).sum(-1)).all()
    r = _ratio(np.abs(m['s2'].astype(np.float64) - m['m2']), m['bound'])
    print(f'[residual row model {dtype}] worst s2 ratio {r.max():.3f}')
    assert r.max() <= 1.0
    assert np.isfinite(m['s1']).all() and np.isfinite(m['s2']).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_pass_m2_fails_the_bound_on_offset_rows(dtype):
    """Negative control: sum(v^2) - s1^2 / 64 in float32 misses the M2 bound on EVERY granule of the common-offset rows that holds offset + N(0, 1)
    (the even granules outside the quiet ones), at every offset; the tree meets it there."""
    p, m = RC.problem(dtype), RC.model(dtype)
    gr = [g for g in range(0, RC.N_MAX // 64, 2) if g not in RC.QUIET_GRANULES]
    with np.errstate(all='ignore'):
        one = RM.m2_one_pass(m['v']).astype(np.float64)
    for c in RC.OFFSETS[dtype]:
        for sign in (1.0, -1.0):
            rows = np.flatnonzero(p['offset'] == sign * c)
            assert len(rows) >= 8 and (rows < 200).sum() >= 2
            sub = np.ix_(rows, gr)
            assert (np.abs(one[sub] - m['m2'][sub]) > m['bound'][sub]).all(), c
            assert (np.abs(m['s2'][sub].astype(np.float64) - m['m2'][sub]) <= m['bound'][sub]).all()
            assert (m['m2'][sub] < 64 * 4.0 * (1.0 + (c * 2.0 ** -8 if dtype == 'bf16' else 0.0)) ** 2).all()       # the variance is the noise's, not the offset's


@pytest.mark.parametrize('dtype', DTYPES)
def test_other_association_gives_other_plane_bits(dtype):
    """Negative control: (st + hi) + lo differs from st + (hi + lo) in the plane bits on at least 1000 elements inside the smallest site."""
    p, m = RC.problem(dtype), RC.model(dtype)
    _, h_w, l_w = RC.wrong_association(p['st'], p['r_hi'], p['r_lo'], dtype)
    differs = (h_w != m['hi']) | (l_w != m['lo'])
    assert (differs[p['assoc']]).all()
    assert (differs & p['assoc'])[SMALL].sum() >= 1000
    assert np.isfinite(m['v'][p['assoc']]).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_constant_granules(dtype):
    """64 equal values: s2 == 0.0 and s1 == 64 v exactly (offset rows: +-c; bf16 also +-1e30)."""
    p, m = RC.problem(dtype), RC.model(dtype)
    rows = np.flatnonzero(p['const_rows'])
    seen = set()
    for g in RC.QUIET_GRANULES:
        vv = m['v'][rows, g * 64:(g + 1) * 64]
        assert (vv == vv[:, :1]).all() and (vv[:, 0] != 0).all()
        assert (m['s2'][rows, g] == 0.0).all() and (m['s1'][rows, g] == F32(64.0) * vv[:, 0]).all()
        seen |= set(np.abs(vv[:, 0]).tolist())
    assert set(float(c) for c in RC.OFFSETS[dtype]) <= seen and (any(abs(x / RC.BF16_CONST - 1.0) < 2.0 ** -14 for x in seen) == (dtype == 'bf16'))   # 1e30 as 16 bits hold it
    # and on the model alone, any value
    for x in (F32(1.0000001), F32(-3.3e-5), F32(65504.0)):
        v = np.full((1, 64), x, F32)
        s1 = RM.granule_s1(v)
        assert s1[0, 0] == F32(64.0) * x and RM.granule_m2(v, s1)[0, 0] == 0.0


def test_operands_are_exact():
    """sum_k |a||w| in units of the row's common binade is an integer below 2^24 (every partial sum is then exact in fp32, in any order); A has four
    significant bits at most; every weight row's amax / 448 is a power of two; a site's operands give the base problem's acc at every K."""
    A0, W0, acc, unit, huge = RC.operands()
    S = (np.abs(A0).astype(np.float64) @ np.abs(W0).astype(np.float64).T) / unit
    assert (S == np.round(S)).all() and S.max() < 2 ** 24
    mant = np.abs(A0) / np.exp2(np.floor(np.log2(np.maximum(np.abs(A0), 1e-30))))
    assert ((mant * 8) % 1 == 0).all()
    amax = np.abs(W0).max(1)
    sc = amax[amax > 0] / F32(448.0)
    assert sc.dtype == F32 and (np.log2(sc) % 1 == 0).all()
    assert np.signbit(acc[acc == 0]).sum() == 0
    for M, N, K in ((200, 384, 64), (512, 768, 256), (512, 1280, 512)):
        A, W = RC.site_operands(M, N, K)
        assert np.array_equal(A.astype(np.float64) @ W.astype(np.float64).T + 0.0, acc[:M, :N])
        for dt in DTYPES:
            assert np.array_equal(RM.from_bits(RM.to_bits(A, dt), dt), A) and np.array_equal(RM.from_bits(RM.to_bits(W, dt), dt), W)
    assert (acc[huge] >= 65536.0).any()


def test_saturation_class_fp16():
    """|st + r| > 65504 stores 0x7BFF / 0xFBFF with lo = +0 and statistics of the clamped value; every listed value is reached through a huge st (bias)
    and through the planes (hi = 65504 and a positive rest); 65503.9 leaves a negative, non-zero lo."""
    p, m = RC.problem('fp16'), RC.model('fp16')
    raw = (p['st'].astype(np.float64) + RM.decode(p['r_hi'], p['r_lo'], 'fp16').astype(np.float64))
    sat = np.abs(raw) > 65504.0
    assert sat[SMALL].sum() > 500
    assert (m['hi'][sat] == np.where(raw[sat] > 0, 0x7BFF, 0xFBFF)).all() and (m['lo'][sat] == 0).all()
    assert np.abs(m['v']).max() == 65504.0
    assert np.isfinite(RM.from_bits(m['hi'], 'fp16')).all() and np.isfinite(RM.from_bits(m['lo'], 'fp16')).all()
    unclamped = (p['st'] + RM.decode(p['r_hi'], p['r_lo'], 'fp16')).astype(F32)
    for x in RC.SAT['fp16']:
        for sgn in (1.0, -1.0):
            cols = np.flatnonzero(p['bias'] == F32(sgn * x))
            assert len(cols) and cols.min() < 384, x                                             # through the bias, inside the smallest site
            assert (np.abs(p['st'][:, cols]) >= 6e4).all()
    for x in RC.SAT_R['fp16']:
        for sgn in (1.0, -1.0):
            hit = (unclamped == F32(sgn * x)) & (np.abs(p['st']) < 4096.0)
            assert hit[SMALL].any(), x                                                            # through the planes
    e = (m['v'] == F32(65503.9)) & (p['cls'] == 1)
    assert e.any() and (m['hi'][e] == 0x7BFF).all() and (RM.from_bits(m['lo'][e], 'fp16') < 0).all()
    e = (unclamped == F32(65520.0)) & (p['st'] == 16.0)
    assert e.any() and (p['r_hi'][e] == 0x7BFF).all()                                             # hi = 65504 plus a positive st


def test_large_values_bf16():
    """bf16: no clamp; values up to 1e18 beside ordinary ones and whole granules of 1e30 keep finite planes and finite statistics.  (Values that bf16
    rounds to inf, above 3.39e38, are out of scope, and so is 1e30 beside O(1) values: that granule's M2, 1e60, has no fp32.)"""
    p, m = RC.problem('bf16'), RC.model('bf16')
    assert np.isfinite(RM.from_bits(m['hi'], 'bf16')).all() and np.isfinite(RM.from_bits(m['lo'], 'bf16')).all()
    a = np.abs(m['v'])
    assert (a[SMALL] > 5e17).any() and (a[SMALL] > 0.9999e30).any() and a.max() < 1.0001e30
    for x in RC.SAT['bf16']:
        assert (np.abs(p['bias'][:384]) == F32(x)).any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_small_magnitudes_zeros_and_cancellation(dtype):
    p, m = RC.problem(dtype), RC.model(dtype)
    v = m['v']
    c4 = (p['cls'] == 4) & p['tiny_bias'][None, :]                                                # v = st = the tiny many-bit bias
    for e in range(3, 27):
        sel = c4 & (np.abs(v) >= 2.0 ** -e) & (np.abs(v) < 2.0 ** (1 - e))
        assert sel[SMALL].sum() >= 3, e
        assert ((v[sel].view(np.uint32) & 0xf) != 0).any()                                       # 20 or more significant bits
    if dtype == 'fp16':
        sub = lambda b: ((b & 0x7c00) == 0) & ((b & 0x3ff) != 0)
        assert sub(m['lo'])[SMALL].sum() > 5000 and sub(m['hi'])[SMALL].sum() > 200
        assert (sub(m['hi']) & (np.abs(v) >= 2.0 ** -14)).sum() == 0
    zero = (v == 0)
    assert (m['hi'][zero] & 0x7fff == 0).all() and (m['lo'][zero] == 0).all()
    c5 = p['cls'] == 5
    neg_zero_in = c5 & (p['r_hi'] == 0x8000) & (p['r_lo'] == 0x8000)
    assert neg_zero_in[SMALL].sum() >= 10 and (m['hi'][neg_zero_in] == 0).all()                   # st is +0 there: (+0) + (-0) = +0
    nz = neg_zero_in & p['neg0_bias'][None, :]                                                    # bias -0 under r = -0: st = (+0) + (-0) is +0, and so is v
    assert p['neg0_bias'][:384].sum() >= 3 and nz[SMALL].sum() >= 3 and not np.signbit(p['st'][:, p['neg0_bias']]).any()
    assert (m['hi'][nz] == 0).all() and (m['lo'][nz] == 0).all()
    assert (zero & c5 & (p['st'] != 0))[SMALL].sum() >= 100                                       # st = -(hi + lo) exactly
    # the signs of zeros are part of the model: a -0 sum (no site can produce one: st = acc + bias is never -0) stays -0 in hi, and lo = (-0) - (-0) = +0
    _, h, l = RM.row(np.array([-0.0], F32), np.array([-0.0], F32), dtype)
    assert h[0] == 0x8000 and l[0] == 0x0000
