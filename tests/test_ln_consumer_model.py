"""CPU: the host model of the LayerNorm consumer side (tests/ln_consumer_model.py: ln_merge, ln_fold, the ln_quant normalise step) on the row families the
device test runs (tests/ln_consumer_cases.py), pinned before any GPU time is spent.

The bounds (LM.bounds, derived there from the operation sequence, u = 2^-24, T = D / 64 granules, A = sum |s_g|):
    |mean - mean*|          <= g_{T+1} A / D                                       one rounding per add of s1, inv_d's, the product's
    d_g = (d*_g - e)(1 + u_g)                                                      d = fma(s_g, 1/64, -mean): ONE rounding; e = mean - mean*, common to the row
    |m2 - M2*|              <= D Em^2 + sum_g (2 * 64 |d_g| dd_g + 64 dd_g^2) + g_{T+1} M2*   the error of d enters 64 d^2 as 2 * 64 |d| dd; the common part e only
                                                                                   as D e^2 (sum_g d*_g = 0); dd_g = u |d_g|; the fma and the chain's adds round once each
    |var - var*|            <= that / D + u M2* / D + u var* =: Ev
    |rstd - rstd*| / rstd*  <= about Ev / 2 var*, + u                              the last u: the model's correctly rounded 1 / sqrt
against (1) the float64 evaluation of the same merge identity on the same float32 partials and (2) the float64 two-pass mean and variance of the stored row
(then s_g and M2_g, float64 statistics rounded to float32, carry u each: partials_rounded).  The model must stay inside with a factor of 2 to spare.

The wrong formulas a kernel could run instead, on the same data against the same bounds:
    one pass       sum_g (M2_g + s_g^2 / 64) - s1^2 / D
    no between     the merge without the 64 d^2 term
    two roundings  d = fl(fl(s_g / 64) - mean) instead of the fma.  This one CANNOT fail: 1/64 is a power of two, s_g / 64 is exact, and the two forms are
                   the same float32 -- asserted bit for bit below, so the fma in d is not what the merge's accuracy rests on.
Every family (over its D and types) must see one of the first two fail, or it would not exercise the merge.  The zero row alone is exact in every formula; it
stays for what it pins downstream (rstd = rsqrt(eps), the fold returns the bias)."""
import fractions

import numpy as np
import pytest

import ln_consumer_cases as LC
import ln_consumer_model as LM

F32, F64 = np.float32, np.float64


def _worst(err, bound):
    with np.errstate(all='ignore'):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


def test_fma32_is_one_rounding():
    """fma32 against exact rational arithmetic, on products that cancel against c (where two roundings differ from one)"""
    rng = np.random.default_rng(5)
    a = rng.standard_normal(400).astype(F32)
    b = rng.standard_normal(400).astype(F32)
    c = (-(a.astype(F64) * b.astype(F64)) * (1.0 + rng.standard_normal(400) * 2.0 ** rng.integers(-30, 1, 400))).astype(F32)
    got = LM.fma32(a, b, c)
    differs = 0
    for x, y, z, g in zip(a, b, c, got):
        exact = fractions.Fraction(float(x)) * fractions.Fraction(float(y)) + fractions.Fraction(float(z))
        lo, hi = np.nextafter(g, F32(-np.inf)), np.nextafter(g, F32(np.inf))
        assert abs(exact - fractions.Fraction(float(g))) <= min(abs(exact - fractions.Fraction(float(lo))), abs(exact - fractions.Fraction(float(hi))))
        differs += g != F32(F32(x * y) + z)
    assert differs > 50                                   # the sample does tell one rounding from two


@pytest.mark.parametrize('dtype', LC.DTYPES)
@pytest.mark.parametrize('D', LC.DS)
def test_model_against_fp64(dtype, D):
    """(mean, rstd) of the model against both float64 references, every family, inside the bounds with a factor of 2 to spare"""
    R, p = LC.rows(dtype, D), LC.partials(dtype, D)
    mean, rstd, _ = LM.merge(p, D)
    assert np.isfinite(mean).all() and np.isfinite(rstd).all()
    for name, (mr, m2r, rr), rounded in (('merge identity', LM.merge_fp64(p, D), False), ('two-pass', LM.two_pass_fp64(R['v']), True)):
        Em, rel = LM.bounds(p, D, mr, m2r, partials_rounded=rounded)
        rm = _worst(np.abs(mean - mr), Em)
        rs = _worst(np.abs(rstd - rr) / rr, rel)
        vmax = np.abs(R['v']).max(-1)
        print(f'[ln consumer model {dtype} D={D} vs {name}] worst ratio mean {rm.max():.3f} rstd {rs.max():.3f}; '
              f'|mean err| / max|v| {np.max(np.abs(mean - mr) / np.maximum(vmax, 1e-30)):.2e}, rstd rel err {np.max(np.abs(rstd - rr) / rr):.2e}, '
              f'rstd bound (median / max) {np.median(rel):.2e} / {rel.max():.2e}')
        assert rm.max() <= 0.5, (name, R['family'][int(rm.argmax())], rm.max())
        assert rs.max() <= 0.5, (name, R['family'][int(rs.argmax())], rs.max())


def _fails(dtype, D):
    """per row: does the wrong formula's rstd miss the bound against the float64 merge identity"""
    p = LC.partials(dtype, D)
    mr, m2r, rr = LM.merge_fp64(p, D)
    _, rel = LM.bounds(p, D, mr, m2r)
    bad = lambda r: ~(np.abs(r.astype(F64) - rr) / rr <= rel)          # NaN (a negative variance) fails
    return bad(LM.rstd_one_pass(p, D)), bad(LM.rstd_no_between(p, D))


def test_wrong_formulas_fail_the_bounds():
    seen = {f: [False, False] for f in LC.FAMILIES}
    for dtype in LC.DTYPES:
        for D in LC.DS:
            fam = np.array(LC.rows(dtype, D)['family'])
            one, nob = _fails(dtype, D)
            for f in LC.FAMILIES:
                seen[f][0] |= bool(one[fam == f].any())
                seen[f][1] |= bool(nob[fam == f].any())
            # one pass: every row with an offset of 64 or more, and the bf16 limit rows (an offset of 1e5 / 3e4)
            sel = np.isin(fam, ('offset64', 'offset1000') + (('limit',) if dtype == 'bf16' else ()))
            assert one[sel].all(), (dtype, D, fam[sel & ~one])
            # no between-granule term: wherever the granule means differ
            sel = np.isin(fam, ('gauss', 'offset8', 'offset64', 'offset1000', 'sigma1e-4', 'sigma1e-3', 'outlier', 'granconst', 'granconst_noise'))
            assert nob[sel].all(), (dtype, D, fam[sel & ~nob])
    print('[ln consumer model] family: one-pass fails, no-between fails:', {f: tuple(v) for f, v in seen.items()})
    for f, (a, b) in seen.items():
        assert a or b or f == 'const0', f
    assert seen['const'][0] and not seen['const'][1]       # a constant row: only the one-pass form is wrong (s1^2 / D against sum s_g^2 / 64, where 1 / D is inexact)


@pytest.mark.parametrize('dtype', LC.DTYPES)
def test_two_roundings_in_d_are_the_same_float(dtype):
    for D in LC.DS:
        p = LC.partials(dtype, D)
        mean, rstd, _ = LM.merge(p, D)
        m2, r2 = LM.merge_two_roundings(p, D)
        assert np.array_equal(mean, m2) and np.array_equal(rstd, r2)
        hp, _ = LC.handmade_partials(D // 64)
        assert np.array_equal(LM.merge(hp, D)[1], LM.merge_two_roundings(hp, D)[1])


def test_exact_rows():
    """the zero row: mean 0, var = eps exactly, rstd = fl(1 / sqrt(1e-6f)); a constant row of a few-bit value at a power-of-two D: mean == the value, var == eps"""
    for dtype in LC.DTYPES:
        for D in LC.DS:
            R, p = LC.rows(dtype, D), LC.partials(dtype, D)
            mean, rstd, var = LM.merge(p, D)
            z = LC.family_rows(dtype, D, ('const0',))
            assert (mean[z] == 0).all() and (var[z] == LM.EPS32).all() and (rstd[z] == F32(1.0 / np.sqrt(F64(LM.EPS32)))).all()
            if D in (1024, 256, 128):
                c = LC.family_rows(dtype, D, ('const',))
                assert np.array_equal(mean[c], R['v'][c, 0]) and (var[c] == LM.EPS32).all()
    hp, names = LC.handmade_partials(12)
    mean, rstd, var = LM.merge(hp, 768)
    assert (var[[n == 'all_zero' for n in names]] == LM.EPS32).all() and np.isfinite(rstd).all()


@pytest.mark.parametrize('dtype', LC.DTYPES)
@pytest.mark.parametrize('epi', (0, 1))
def test_fold_bound_with_a_float32_emulation(dtype, epi):
    """The per-element bound the device test asserts on the fold, checked here first: float32 accumulation (k blocks of 32, numpy's float32 product inside a block:
    one of the orders a kernel may take) + the model's two fmas (+ a float64 GELU rounded to float32) + one rounding to 16 bits, against the float64 reference on
    the same float32 statistics.  And the zero row returns round16(bias) exactly."""
    import residual_row_model as RM
    D, N = 384, 64
    R, p = LC.rows(dtype, D), LC.partials(dtype, D)
    rng = np.random.default_rng(11)
    W = RM.from_bits(RM.to_bits((rng.standard_normal((N, D)) * 0.05 + 0.02 * (np.arange(N)[:, None] % 5 - 1)).astype(F32), dtype), dtype)
    ln_s = W.astype(F64).sum(1).astype(F32)
    bias = (rng.standard_normal(N) * 0.3).astype(F32)
    hi = RM.from_bits(R['hi'], dtype)
    mean, rstd, _ = LM.merge(p, D)
    acc = np.zeros((hi.shape[0], N), F32)
    for k in range(0, D, 32):
        acc = (acc + hi[:, k:k + 32] @ W[:, k:k + 32].T).astype(F32)
    v = LM.fold(acc, mean[:, None], ln_s[None, :], rstd[:, None], bias[None, :])
    if epi == 1:
        v = LM.gelu64(v.astype(F64)).astype(F32)
    got = RM.from_bits(RM.to_bits(v, dtype), dtype).astype(F64)
    ref, bound, _ = LM.fold_reference(hi, W, ln_s, bias, mean, rstd, epi, dtype)
    r = _worst(np.abs(got - ref), bound)
    print(f'[ln consumer model {dtype} epi {epi}] fold: worst |err| / bound {r.max():.3f} ({R["family"][int(r.max(1).argmax())]})')
    assert r.max() <= 1.0
    z = LC.family_rows(dtype, D, ('const0',))
    b16 = bias if epi == 0 else LM.gelu64(bias.astype(F64)).astype(F32)
    assert np.array_equal(got[z[0]], RM.from_bits(RM.to_bits(b16, dtype), dtype).astype(F64))
    # ... and the fold against the true LayerNorm of hi + lo: the hi plane's rounding on top
    ref_ln, bound_ln = LM.layernorm_reference(R['v'], hi, W, bias, epi, dtype, bound, rstd)
    r_ln = _worst(np.abs(got - ref_ln), bound_ln)
    print(f'[ln consumer model {dtype} epi {epi}] fold vs LayerNorm(hi + lo): worst |err| / bound {r_ln.max():.3f}')
    assert r_ln.max() <= 1.0
    # a non-fused acc - mean s (two roundings) is another float32: what the bit-for-bit comparisons between kernels see (the float64 bound allows 2u |mean s|, it stays inside)
    v2 = ((acc - (mean[:, None] * ln_s[None, :]).astype(F32)).astype(F32) * rstd[:, None]).astype(F32) + bias[None, :]
    assert (v2 != LM.fold(acc, mean[:, None], ln_s[None, :], rstd[:, None], bias[None, :])).any()


@pytest.mark.parametrize('dtype', LC.DTYPES)
def test_quant_model(dtype):
    """the ln_quant normalise step + mx8.h: a constant row is an all-zero block (scale byte 0, codes 0) wherever hi == mean; every other block's scaled amax lies in
    [128, 256); a wrong shift (mean instead of mean * rstd) changes the codes"""
    import residual_row_model as RM
    D = 768
    R, p = LC.rows(dtype, D), LC.partials(dtype, D)
    hi = RM.from_bits(R['hi'], dtype)
    mean, rstd, _ = LM.merge(p, D)
    y = LM.quant_normalise(hi, mean, rstd)
    E, codes, scaled = LM.mx_quantise(y)
    assert np.isfinite(y).all()
    z = LC.family_rows(dtype, D, ('const0',))
    assert (E[z] == 0).all() and (codes[z] == 0).all()
    am = np.abs(scaled).reshape(len(y), D // 32, 32).max(-1)
    nz = E > 0
    assert nz.sum() > 100 and (am[nz] >= 128).all() and (am[nz] < 256).all()
    wrong = LM.fma32(hi, rstd[:, None], -mean[:, None])
    off = LC.family_rows(dtype, D, ('offset64',))
    assert (LM.mx_quantise(wrong)[1][off] != codes[off]).mean() > 0.5
