"""GPU: the producer row of the two-plane residual stream (csrc/common.h: planes_decode8, planes_split8, granule_stats8 / granule_stats16) at every
site that runs it, on edge values, against the exact host model of tests/residual_row_model.py.

The other GEMM tests draw Gaussians and see hi + lo summed; here the taps vp_dbg_gemm_case_planes / vp_dbg_gemm_fp8_case_planes take and return plane
BITS, and the operands (tests/residual_row_cases.py) make st = fl32(acc + bias) known exactly whatever order a kernel accumulates in.  One problem,
every site a prefix of it, so all sites see the same (st, r).  Rows: ordinary values; fp16 saturation (v in +-{65504, 65519.9, 65520, 7e4, 1e6, 3e38},
through a huge st and through hi = 65504 plus a positive st; 65503.9 with its negative lo) / bf16 values up to 1e18 beside ordinary ones and whole
granules of 1e30 (bf16 does not clamp; values it rounds to inf, above 3.39e38, are out of scope, and so is 1e30 beside O(1) values, whose M2 of 1e60
no fp32 statistic holds); a common offset of +-{250, 1000, 30000 | 1e5} with a granule of 64 equal values; magnitudes from 2^-3 down to 2^-26 with
full significands (fp16: lo, then hi, are subnormals), zeros of both signs in r, st = -(hi + lo); elements where (st + hi) + lo would give other bits;
arbitrary finite plane bits.  (v = -0 cannot occur at any site: st = acc + bias is never -0.  The nearest case runs here: a bias of -0 on a column
whose acc is +0, under r = -0, must store +0 in both planes.  The model's own -0 is pinned on the CPU.)

Per launch, on every element: both planes and s1 bit-equal to the model; |s2 - M2| <= 2^-20 M2 + 64 (2^-22 |mean|)^2 against the fp64 M2 of the stored
values; s2 == 0.0 on a constant granule; in place (out == aux, as the forward runs it) the same bits as out of place.  Across sites: identical planes,
s1 AND s2 bits on the common rows.

Measured on an MI355X, all 13 (fp16) / 11 (bf16) sites and the four patch-embed tiles: every plane and every s1 bit-equal; worst |s2 - M2| / bound
0.263 (fp16) and 0.473 (bf16), the very figures of the float32 model on the CPU, and the sites agree in s2 bit for bit.  The device keeps fp16
subnormals in both planes.

The 8-phase kernel's LDS-staged 256 x 192 tile cannot take N = 1280 (not a multiple of 192): its second width is N = 1152, 18 granules."""
import functools

import numpy as np
import pytest

import residual_row_cases as RC
import residual_row_model as RM
from easy_vitpose_amd import _capi as capi

pytestmark = pytest.mark.gpu

F32 = np.float32
DTYPES = ('fp16', 'bf16')

# site -> (kind, variant, M, N, K, split-K S)
SITES = {
    'gemm cfg9': ('gemm', 9, 200, 384, 64, 0), 'gemm cfg11': ('gemm', 11, 200, 384, 64, 0), 'gemm cfg1': ('gemm', 1, 200, 384, 64, 0),
    'gemm cfg3': ('gemm', 3, 200, 384, 64, 0),                                     # ragged last m-tile; cfg3's second 256-column tile is half outside N
    'gemm8 256x192 (LDS-staged)': ('gemm', 17, 512, 768, 256, 0), 'gemm8 256x192, N 1152': ('gemm', 17, 512, 1152, 256, 0),
    'gemm8 256x256 (register-direct)': ('gemm', 16, 512, 1024, 256, 0), 'gemm8 256x256, N 1280': ('gemm', 16, 512, 1280, 256, 0),
    'gemm8 192x256 (register-direct)': ('gemm', 18, 384, 1024, 256, 0),
    'split-K 2 + reduce': ('gemm', 12, 200, 384, 512, 2), 'split-K 4 + reduce': ('gemm', 12, 200, 384, 512, 4),
    'gemm8f 256x192 (LDS-staged)': ('fp8', 17, 512, 768, 512, 0), 'gemm8f 256x256 (register-direct)': ('fp8', 16, 512, 1024, 512, 0),
}
POS_SITES = {f'gemm cfg{v} patch embed': v for v in (9, 11, 1, 3)}


def _ptr(a):
    return None if a is None else a.ctypes.data


@functools.lru_cache(maxsize=None)
def _run(site, dtype, in_place):
    """one launch of a site on its prefix of the problem: (hi bits, lo bits, stats)"""
    kind, variant, M, N, K, S = SITES[site]
    p = RC.problem(dtype)
    A, W = RC.site_operands(M, N, K)
    bias = np.ascontiguousarray(p['bias'][:N])
    r_hi, r_lo = np.ascontiguousarray(p['r_hi'][:M, :N]), np.ascontiguousarray(p['r_lo'][:M, :N])
    o_hi, o_lo = np.empty((M, N), np.uint16), np.empty((M, N), np.uint16)
    stats = np.empty((M, N // 64, 2), F32)
    lib = capi.load_library()
    if kind == 'fp8':
        a_deq, w_deq = np.empty_like(A), np.empty_like(W)
        rc = lib.vp_dbg_gemm_fp8_case_planes(0, M, N, K, _ptr(A), _ptr(W), _ptr(bias), _ptr(r_hi), _ptr(r_lo), int(in_place), _ptr(o_hi), _ptr(o_lo),
                                             _ptr(stats), _ptr(a_deq), _ptr(w_deq))
        assert rc == 0, capi.last_error()
        # the operands were exact: the codes and scales stand for A and W themselves
        assert np.array_equal(a_deq.view(np.uint32), A.view(np.uint32)) and np.array_equal(w_deq.view(np.uint32), W.view(np.uint32)), f'{site}: MXFP8 operands not exact'
    else:
        gm = 8 if 16 <= variant <= 18 else 0
        rc = lib.vp_dbg_gemm_case_planes(0, capi.DTYPES[dtype], 6, variant, gm, S << 8, M, N, K, _ptr(A), _ptr(W), _ptr(bias), _ptr(r_hi), _ptr(r_lo), None,
                                         int(in_place), _ptr(o_hi), _ptr(o_lo), _ptr(stats))
        assert rc == 0, capi.last_error()
    return o_hi, o_lo, stats


@functools.lru_cache(maxsize=None)
def _run_pos(site, dtype):
    variant = POS_SITES[site]
    M, N, K = 200, 384, 64
    A, W = RC.site_operands(M, N, K)
    pos, _ = RC.model_pos(dtype, M, N)
    pos = np.ascontiguousarray(pos)
    bias = np.zeros(N, F32)
    o_hi, o_lo = np.empty((M, N), np.uint16), np.empty((M, N), np.uint16)
    stats = np.empty((M, N // 64, 2), F32)
    rc = capi.load_library().vp_dbg_gemm_case_planes(0, capi.DTYPES[dtype], 7, variant, 0, 0, M, N, K, _ptr(A), _ptr(W), _ptr(bias), None, None, _ptr(pos), 0,
                                                     _ptr(o_hi), _ptr(o_lo), _ptr(stats))
    assert rc == 0, capi.last_error()
    return o_hi, o_lo, stats


def _check(what, got, m, dtype, const=None):
    """every element of one launch against the model m (dict of [M, N] / [M, N / 64] arrays)"""
    hi, lo, stats = got
    assert np.array_equal(hi, m['hi']), f'{what}: hi plane differs from the model in {(hi != m["hi"]).sum()} elements, first at {np.argwhere(hi != m["hi"])[0]}'
    assert np.array_equal(lo, m['lo']), f'{what}: lo plane differs from the model in {(lo != m["lo"]).sum()} elements, first at {np.argwhere(lo != m["lo"])[0]}'
    assert np.isfinite(RM.from_bits(hi, dtype)).all() and np.isfinite(RM.from_bits(lo, dtype)).all(), f'{what}: inf or NaN in a plane'
    s1, s2 = np.ascontiguousarray(stats[..., 0]), np.ascontiguousarray(stats[..., 1])
    bad = s1.view(np.uint32) != m['s1'].view(np.uint32)
    assert not bad.any(), f'{what}: s1 differs from the tree in {bad.sum()} granules, first at {np.argwhere(bad)[0]}'
    err = np.abs(s2.astype(np.float64) - m['m2'])
    with np.errstate(all='ignore'):
        ratio = np.where(m['bound'] > 0, err / m['bound'], np.where(err == 0, 0.0, np.inf))
    print(f'[residual row] {what} {dtype}: worst |s2 - M2| / bound = {ratio.max():.3f}')
    assert ratio.max() <= 1.0, f'{what}: s2 misses the bound at {np.argwhere(ratio > 1.0)[0]} (ratio {ratio.max():.3f})'
    if const is not None:
        assert const.any() and (s2[const] == 0.0).all(), f'{what}: s2 != 0 on a constant granule'
    return float(ratio.max())


def _model_for(dtype, M, N):
    m = RC.model(dtype)
    sub = {k: a[:M, :N] for k, a in m.items() if k in ('v', 'hi', 'lo')}
    sub.update({k: a[:M, :N // 64] for k, a in m.items() if k in ('s1', 's2', 'm2', 'mean', 'bound')})
    const = np.zeros((M, N // 64), bool)
    for g in RC.QUIET_GRANULES:
        if g < N // 64:
            const[RC.problem(dtype)['const_rows'][:M], g] = True
    return sub, const


def _site_params():
    return [(s, d) for s in SITES for d in DTYPES if not (SITES[s][0] == 'fp8' and d == 'bf16')]


@pytest.mark.parametrize('site,dtype', _site_params())
def test_residual_row_site(site, dtype):
    """one site, out of place and in place: planes, s1 bit-equal to the model, s2 inside its bound, constant granules, in place == out of place"""
    _, _, M, N, _, S = SITES[site]
    m, const = _model_for(dtype, M, N)
    out = _run(site, dtype, False)
    _check(site, out, m, dtype, const)
    inp = _run(site, dtype, True)
    _check(site + ' in place', inp, m, dtype, const)
    for a, b, name in zip(out, inp, ('hi', 'lo', 'stats')):
        assert np.array_equal(a.view(np.uint16 if a.dtype == np.uint16 else np.uint32), b.view(np.uint16 if b.dtype == np.uint16 else np.uint32)), \
            f'{site}: in place differs from out of place in {name}'


@pytest.mark.parametrize('site,dtype', [(s, d) for s in POS_SITES for d in DTYPES])
def test_residual_row_patch_embed(site, dtype):
    """EPI_POS_LN: no bias, r = the fp32 pos[m % 192] (the values the problem's planes stand for); rows 192 .. 199 meet pos rows 0 .. 7 with another acc"""
    _, m = RC.model_pos(dtype, 200, 384)
    _check(site, _run_pos(site, dtype), m, dtype)
    first = _run_pos(next(iter(POS_SITES)), dtype)
    for a, b in zip(first, _run_pos(site, dtype)):
        assert a.tobytes() == b.tobytes(), f'{site}: differs from {next(iter(POS_SITES))}'


@pytest.mark.parametrize('dtype', DTYPES)
def test_residual_row_sites_agree(dtype):
    """Every site fed the same (st, r) gives identical planes and statistics on the common rows and granules -- s2 bit for bit too: the register-direct sites
    (granule_stats16) against the LDS-staged ones and the split-K reduction (granule_stats8), the MXFP8 kernel against the 16-bit ones."""
    sites = [s for s, d in _site_params() if d == dtype]
    ref_site = 'gemm8 256x256, N 1280'
    ref = _run(ref_site, dtype, True)
    for s in sites:
        _, _, M, N, _, _ = SITES[s]
        got = _run(s, dtype, True)
        rows = min(M, SITES[ref_site][2])
        for a, b, name in zip(got, ref, ('hi', 'lo', 'stats')):
            cols = N if name != 'stats' else N // 64
            x, y = np.ascontiguousarray(a[:rows, :cols]), np.ascontiguousarray(b[:rows, :cols])
            assert x.tobytes() == y.tobytes(), f'{s} differs from {ref_site} in {name} ({dtype})'
