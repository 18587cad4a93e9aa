"""GPU: the simple decoder's head kernel (csrc/simplehead.hip) through vp_dbg_simple_head_case, which runs the launch head_chunk builds on host data, on the case
families of tests/simple_head_cases.py against the float64 model of tests/simple_head_model.py:

    taps        bit for bit the model's values (exact by construction: a wrong tap, shift, ky / kx swap, border or neighbour is readable from the value)
    edges, corners, relu, relu_sub, lo_plane, random      per element, none exempt: |hm - v| <= (2 D + 32) (2^-24 S + 2^-126), derived in the model's docstring
    map counts  Kp in {1, 14, 16, 17, 33, 133}: slab boundaries and ragged slabs;  widths  Cin in {64, 384, 768, 1024, 1280} at B = 1, Kp = 17;  fp16 and bf16
    seams       crop i of a batch of 3 has the bits of the same crop alone, at every position; two runs give the same bits
    the output was filled with 0xFF bytes: no element comes back unwritten, and the 16 planes of guard behind it still hold the fill
tests/test_simple_head_model.py pins the model and the bound on the CPU and shows the wrong models failing it.  No number in this file comes from the kernel under
test.  NaN and inf inputs are out of scope."""
import numpy as np
import pytest

import simple_head_cases as SC
import simple_head_model as SM
from easy_vitpose_amd import _capi as capi

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = ('fp16', 'bf16')
KPS = (1, 14, 16, 17, 33, 133)
WIDTHS = (64, 384, 768, 1024, 1280)
FAMILIES = {'edges': SC.edges, 'corners': lambda *a: SC.edges(*a, variant='corners'), 'relu': SC.relu, 'relu_sub': lambda *a: SC.relu(*a, variant='sub'),
            'lo_plane': SC.lo_plane, 'random': SC.random}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _call(dtype, x, w, b):
    """one vp_dbg_simple_head_case call -> (rc, out, guard); out keeps its NaN fill where the tap refuses"""
    x, w, b = (np.ascontiguousarray(a, F32) for a in (x, w, b))
    B, _, Cin = x.shape
    Kp = w.shape[0]
    out, guard = np.full((B, Kp, 64, 48), np.nan, F32), np.zeros(16 * 3072 * 4, np.uint8)
    rc = capi.load_library().vp_dbg_simple_head_case(0, capi.DTYPES[dtype], B, Cin, x.ctypes.data, w.ctypes.data, b.ctypes.data, Kp, out.ctypes.data, guard.ctypes.data)
    return rc, out, guard


def _ok(dtype, case, crops=None):
    x = case['x'] if crops is None else case['x'][crops]
    rc, out, guard = _call(dtype, x, case['w'], case['b'])
    assert rc == 0, capi.last_error()
    assert not np.isnan(out).any(), f'{np.isnan(out).sum()} of {out.size} elements unwritten'
    assert (guard == 0xff).all(), f'{(guard != 0xff).sum()} guard bytes behind the heatmaps overwritten'
    return out


def _where(r):
    return tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))


def _check(dtype, case, got, tag):
    D = case['x'].shape[-1]
    v, S = SM.model(case['x'], case['w'], case['b'], dtype)
    r = SM.ratio(got, v, SM.bound(S, D))
    at = _where(r)
    print(f'[simple head {tag} {dtype} B {case["x"].shape[0]} Cin {D} Kp {case["w"].shape[0]}] worst err / bound {r.max():.4f} at (crop, map, y, x) = {at}')
    assert r.max() <= 1, (at, got[at], v[at], S[at])
    return r


def _taps(dtype, D, Kp, tokens=SC.TAP_TOKENS):
    case = SC.taps(dtype, D, Kp, tokens)
    got = _ok(dtype, case)
    v, _ = SM.model(case['x'], case['w'], case['b'], dtype)
    exp = v.astype(F32)
    assert np.array_equal(exp.astype(F64), v)
    bad = np.argwhere(got != exp)
    assert np.array_equal(got, exp), (f'{len(bad)} of {exp.size} elements wrong; first (crop, map, y, x) = {tuple(bad[0])}: got {got[tuple(bad[0])]}, expected '
                                      f'{exp[tuple(bad[0])]} (crop n holds 2.0 at token {tokens[bad[0][0]]}; map k reads tap k % 9 with weight 2^-(1 + k % 3), bias k % 3 - 1)')


@pytest.mark.parametrize('Kp', KPS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_taps_bit_for_bit(dtype, Kp):
    _taps(dtype, 64, Kp)


@pytest.mark.parametrize('family', tuple(FAMILIES))
@pytest.mark.parametrize('dtype', DTYPES)
def test_families_per_element(dtype, family):
    case = FAMILIES[family](dtype, 384, 17)
    got = _ok(dtype, case)
    _check(dtype, case, got, family)
    if family == 'relu':
        # the negative, -0.0 and negative-subnormal channels carry weights of 25 .. 2^40: without them the result is the same to the last bit only if they gave exactly 0
        rest = dict(case, x=case['x'].copy())
        rest['x'][..., :24] = 0.0
        assert np.array_equal(_bits(_ok(dtype, rest)), _bits(got))
    if family == 'relu_sub':
        assert np.abs(got).max() > 0          # subnormal inputs are multiplied, not flushed


@pytest.mark.parametrize('Kp', KPS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_map_counts(dtype, Kp):
    case = SC.random(dtype, 64, Kp)
    _check(dtype, case, _ok(dtype, case), 'map count')


@pytest.mark.parametrize('Cin', WIDTHS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_widths(dtype, Cin):
    case = SC.random(dtype, Cin, 17, B=1)
    _check(dtype, case, _ok(dtype, case), 'width')
    _taps(dtype, Cin, 17, SC.TAP_TOKENS[3:9:2])      # a corner, an edge, the interior: the k loop's length is what changes here


@pytest.mark.parametrize('dtype', DTYPES)
def test_seams_and_run_to_run(dtype):
    case = SC.seams(dtype, 384, 17)
    got = _ok(dtype, case)
    _check(dtype, case, got, 'seams')
    assert np.array_equal(_bits(_ok(dtype, case)), _bits(got)), 'run-to-run difference'
    for i in range(3):
        alone = _ok(dtype, case, crops=[i])
        assert np.array_equal(_bits(alone[0]), _bits(got[i])), f'crop {i} alone differs from crop {i} at position {i} of the batch'
    for perm in ([2, 0, 1], [1, 2, 0]):
        moved = _ok(dtype, case, crops=perm)
        for pos, i in enumerate(perm):
            assert np.array_equal(_bits(moved[pos]), _bits(got[i])), f'crop {i} at position {pos} differs from itself at position {i}'


def test_the_checker_can_fail():
    """negative control: the outputs of the wrong models, handed to the checker in place of the device's, fail it where the device passes"""
    dtype = 'fp16'
    for wrong, family in (('border_clamp', 'edges'), ('kykx_transposed', 'random'), ('lo_dropped', 'lo_plane'), ('relu_after_upsample', 'relu')):
        case = FAMILIES[family](dtype, 384, 17)
        _check(dtype, case, _ok(dtype, case), f'control {family}')
        bad, _ = SM.model(case['x'], case['w'], case['b'], dtype, wrong=wrong)
        with pytest.raises(AssertionError):
            _check(dtype, case, bad.astype(F32), f'control {wrong}')


def test_refusals_come_back_as_errors():
    case = SC.random('fp16', 64, 3, B=1)
    rc, out, _ = _call('fp16', case['x'][..., :48], case['w'][:, :48], case['b'])       # Cin not a multiple of 32
    assert rc == capi.VP_ERR_INVALID and np.isnan(out).all()
    x, w, b = (np.ascontiguousarray(a, F32) for a in (case['x'], case['w'], case['b']))
    out, guard = np.full((1, 3, 64, 48), np.nan, F32), np.zeros(16 * 3072 * 4, np.uint8)
    lib = capi.load_library()
    assert lib.vp_dbg_simple_head_case(0, capi.VP_DTYPE_FP8, 1, 64, x.ctypes.data, w.ctypes.data, b.ctypes.data, 3, out.ctypes.data, guard.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_simple_head_case(0, 0, 1, 64, x.ctypes.data, None, b.ctypes.data, 3, out.ctypes.data, guard.ctypes.data) == capi.VP_ERR_INVALID
    assert np.isnan(out).all()
