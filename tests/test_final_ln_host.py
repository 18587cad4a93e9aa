"""CPU: the bound of the standalone LayerNorm pass (tests/final_ln_model.py) pinned before any GPU time is spent.

(1) The float32 emulation of layernorm_kernel in its own order -- fused and unfused, rstd correctly rounded and an ulp to either side -- stays inside C * E on every
    row family of tests/ln_consumer_cases.py, D = 384 / 768 / 1024 / 1280, both types, both affine sets, with the factor of 2 the constant was chosen with; the worst
    ratio |emulation - reference| / E per family is printed and must still be what final_ln_model's docstring says (within a few per cent).
(2) The wrong formulas a kernel could run instead fail the same bound on named families: one-pass E[x^2] - mean^2, eps = 1e-5, the lo plane dropped, division by D - 1,
    the row sum divided by the plane's row count."""
import itertools

import numpy as np
import pytest

import final_ln_model as FM
import ln_consumer_cases as LC
import residual_row_model as RM

F32, F64 = np.float32, np.float64


def _emulated_worst(dtype, D):
    R = LC.rows(dtype, D)
    fam = np.array(R['family'])
    worst = {f: 0.0 for f in LC.FAMILIES}
    for kind in FM.AFFINES:
        g, b = FM.affine(D, kind)
        ref, bnd = FM.reference(R['v'], g, b)[0], FM.bound(R['v'], g, b, C=1.0)
        for fs, fo, ru in itertools.product((True, False), (True, False), (0, 1, -1)):
            r = FM.ratio(FM.emulate(R['v'], g, b, fs, fo, ru), ref, bnd).max(-1)
            for f in LC.FAMILIES:
                worst[f] = max(worst[f], float(r[fam == f].max()))
    return worst


def test_emulation_inside_the_bound_and_the_constant():
    worst = {f: 0.0 for f in LC.FAMILIES}
    for dtype in LC.DTYPES:
        for D in FM.DS:
            for f, r in _emulated_worst(dtype, D).items():
                worst[f] = max(worst[f], r)
    print('[final ln model] worst |emulation - fp64| / E per family:', {f: round(r, 3) for f, r in worst.items()})
    top = max(worst.values())
    assert 2.0 * top <= FM.C_BOUND, (top, FM.C_BOUND)              # the margin of 2 the constant was chosen with
    assert FM.C_BOUND <= 2.0 * top * 1.05                          # ... and no more: the docstring's figures are still the measured ones
    assert abs(top - 0.930) < 0.01


def test_affine_sets_have_structure():
    for D in FM.DS:
        g, b = FM.affine(D, 'structured')
        assert (g > 0).sum() > D // 4 and (g < 0).sum() > D // 4 and (b > 0).any() and (b < 0).any()
        assert np.isclose(np.abs(g).min(), 0.05) and np.isclose(np.abs(g).max(), 3.0)
        g, b = FM.affine(D, 'identity')
        assert (g == 1).all() and (b == 0).all()


def test_cases_sum_exactly():
    """hi + lo is exact in float32 on every row (what lets the PLANES = false kernel on v stand for the planes kernel bit for bit)"""
    for dtype in LC.DTYPES:
        for D in FM.DS:
            R = LC.rows(dtype, D)
            assert np.array_equal(R['v'].astype(F64), RM.from_bits(R['hi'], dtype).astype(F64) + RM.from_bits(R['lo'], dtype).astype(F64))


WRONG = {                                    # formula -> the families on which EVERY row must miss the bound (fp16 and bf16, every D)
    'one_pass': ('offset1000',),
    'eps_1e-5': ('sigma1e-4', 'sigma1e-3'),
    'no_lo': ('gauss', 'offset8', 'outlier'),
    'unbiased': ('gauss', 'offset8', 'offset64', 'granconst_noise'),
    'mean_divisor': ('offset8', 'offset64', 'offset1000', 'granconst'),
}


@pytest.mark.parametrize('dtype', LC.DTYPES)
@pytest.mark.parametrize('D', FM.DS)
def test_wrong_formulas_fail_the_bound(dtype, D):
    R = LC.rows(dtype, D)
    fam = np.array(R['family'])
    g, b = FM.affine(D, 'structured')
    ref, bnd = FM.reference(R['v'], g, b)[0], FM.bound(R['v'], g, b)
    plane_rows = len(fam) + 7
    got = {'one_pass': FM.wrong_one_pass(R['v'], g, b), 'eps_1e-5': FM.wrong_eps(R['v'], g, b), 'no_lo': FM.wrong_no_lo(RM.from_bits(R['hi'], dtype), g, b),
           'unbiased': FM.wrong_unbiased(R['v'], g, b), 'mean_divisor': FM.wrong_mean_divisor(R['v'], g, b, plane_rows)}
    for name, fams in WRONG.items():
        bad = FM.ratio(got[name], ref, bnd).max(-1) > 1.0
        sel = np.isin(fam, fams)
        assert bad[sel].all(), (name, dtype, D, fam[sel & ~bad])
    # and the right formula in float64 passes, by a wide margin
    assert FM.ratio(ref, ref, bnd).max() == 0


def test_symbols_exported():
    from easy_vitpose_amd import _capi as capi
    lib = capi.load_library()
    for name in ('vp_dbg_im2col', 'vp_dbg_layernorm_planes'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
