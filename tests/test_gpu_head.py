"""GPU: the keypoint head's GEMMs -- EPI_DECONV on every tile the selection rule can put a deconv on (and on the fused stage's 256 x 256 tile), in both launch orders
of the four output parities; EPI_DECONV_FINAL; EPI_DECONV + EPI_HEATMAP -- each through vp_dbg_head_case, which launches them with the arguments the forward
builds, on the case families of tests/head_cases.py against the float64 model of tests/head_model.py:

    taps        bit for bit the gathered source codes (a wrong tap, parity, border row, image seam or channel is readable from the value)
    edges, relu_clamp, onehot      per element, none exempt: |got - v| <= u |v| + 4 Cin 2^-24 S + 2^-25 against the folded-then-rounded model, + 2 u S against the
                un-folded float64 module (derived in head_model's docstring; nothing is fitted)
    stage 0     the same bits on every tile and in both parity orders (one k order by construction), and run to run
    final       the fused kernel == the two launches bit for bit for every Kp, the two launches' 16-bit tensor == stage 0's, |hm - ref| <= 258 2^-24 S2 against
                float64 on the device's own activation bits
    every output was filled with 0xFF bytes: no element comes back unwritten, and the 16 image planes of guard behind it still hold the fill
tests/test_head_model.py pins the model and the bounds on the CPU, shows the wrong models failing them and derives the tile list.  No number in this file comes
from the kernels under test.  NaN and inf inputs are out of scope."""
import ctypes as C

import numpy as np
import pytest

import head_cases as HC
import head_model as HM
from easy_vitpose_amd import _capi as capi

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TILES = HC.STAGE0_TILES + (HC.FUSED_TILE,)
NAMES = {'w': 'keypoint_head.deconv_layers.0.weight', 'gamma': 'keypoint_head.deconv_layers.1.weight', 'beta': 'keypoint_head.deconv_layers.1.bias',
         'mean': 'keypoint_head.deconv_layers.1.running_mean', 'var': 'keypoint_head.deconv_layers.1.running_var'}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _head(dtype, stage, variant, parity_fast, case, fin=None):
    """one vp_dbg_head_case call -> (rc, dict(out, guard[, mid, mid_guard])); the outputs keep their NaN fill where the tap refuses"""
    x = np.ascontiguousarray(case['x'], F32)
    B, H, W, Cin = x.shape
    keep = {NAMES[k]: np.ascontiguousarray(case[k], F32) for k in NAMES}
    descs = (capi.vp_tensor_desc * len(keep))(*[capi.vp_tensor_desc(k.encode(), v.ctypes.data_as(C.POINTER(C.c_float)), v.size) for k, v in keep.items()])
    opix, Kp = 4 * H * W, 0
    wf = bf = None
    if fin is not None:
        wf, bf = np.ascontiguousarray(fin['w_fin'], F32), np.ascontiguousarray(fin['b_fin'], F32)
        Kp = wf.shape[0]
    act = lambda: (np.full((B, 2 * H, 2 * W, 256), np.nan, F32), np.zeros(16 * opix * 2, np.uint8))
    r = {}
    if stage == 0:
        r['out'], r['guard'] = act()
    else:
        r['out'], r['guard'] = np.full((B, Kp, 2 * H, 2 * W), np.nan, F32), np.zeros(16 * opix * 4, np.uint8)
    if stage == 2:
        r['mid'], r['mid_guard'] = act()
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = capi.load_library().vp_dbg_head_case(0, capi.DTYPES[dtype], stage, variant, parity_fast, B, H, W, Cin, x.ctypes.data, descs, len(keep), Kp, ptr(wf), ptr(bf),
                                              ptr(r['out']), ptr(r['guard']), ptr(r.get('mid')), ptr(r.get('mid_guard')))
    return rc, r


def _ok(dtype, stage, variant, parity_fast, case, fin=None):
    """... that must succeed, with every output element written and every guard byte still the fill"""
    rc, r = _head(dtype, stage, variant, parity_fast, case, fin)
    assert rc == 0, (stage, variant, parity_fast, capi.last_error())
    for o, g in (('out', 'guard'), ('mid', 'mid_guard')):
        if o in r:
            assert not np.isnan(r[o]).any(), f'stage {stage} tile {variant} parity_fast {parity_fast}: {np.isnan(r[o]).sum()} elements of {o} unwritten'
            assert (r[g] == 0xff).all(), f'stage {stage} tile {variant} parity_fast {parity_fast}: {(r[g] != 0xff).sum()} guard bytes behind {o} overwritten'
    return r


def _stage0_everywhere(dtype, case):
    """stage 0 on every tile in both parity orders, and once more: one result, bit for bit"""
    ref = _ok(dtype, 0, TILES[0], 1, case)['out']
    for variant in TILES:
        for pf in (1, 0):
            got = _ok(dtype, 0, variant, pf, case)['out']
            assert _same(got, ref), (f'tile {variant} parity_fast {pf}: {(_bits(got) != _bits(ref)).sum()} of {ref.size} elements differ from tile {TILES[0]}; first at '
                                     f'{tuple(np.argwhere(_bits(got) != _bits(ref))[0])} (img, oy, ox, channel)')
    return ref


def _check_stage0(got, v, S, Cin, dtype, unfolded=False):
    """the checker of the per-element stage-0 bound: err / bound per element (inf where got is not finite)"""
    return HM.ratio(got, v, HM.bound0(v, S, Cin, dtype, unfolded))


def _check_final(hm, a, fin, dtype):
    """... of the final conv against float64 on the activation bits a"""
    ref, S2 = HM.final(a, fin['w_fin'], fin['b_fin'], dtype)
    return HM.ratio(hm, ref, HM.bound_final(S2))


def _where(r):
    return tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))


FAMILIES = {'edges': (HC.edges, HC.edges_parts), 'relu_clamp': (HC.relu_clamp, HC.relu_parts), 'onehot': (HC.onehot, HC.onehot_parts)}


@pytest.mark.parametrize('shape', HC.DECONV1 + HC.DECONV2, ids=str)
@pytest.mark.parametrize('rot', (0, 1))
def test_taps_are_the_source_codes(shape, rot):
    case = HC.taps(*shape, rot)
    got = _stage0_everywhere(shape[0], case)
    exp = HC.taps_expected(case)
    bad = np.argwhere(got != exp)
    assert np.array_equal(got, exp), (f'{len(bad)} of {exp.size} elements wrong; first (img, oy, ox, channel) = {tuple(bad[0])}: got {got[tuple(bad[0])]}, expected '
                                      f'{exp[tuple(bad[0])]} (channel c % 4 of the source carries i + 1, j + 1, img + 1, (c // 4) % 64 + 1)')


@pytest.mark.parametrize('family', tuple(FAMILIES))
@pytest.mark.parametrize('shape', HC.DECONV1 + HC.DECONV2, ids=str)
def test_stage0_per_element(family, shape):
    dtype, Cin = shape[0], shape[4]
    case, p = FAMILIES[family][0](*shape), FAMILIES[family][1](*shape)
    got = _stage0_everywhere(dtype, case)
    v, stored, S = HM.stage0(p['z'], p['A'], p['bias'], dtype)
    mod = HM.module(case['x'], case['w'], case['gamma'], case['beta'], case['mean'], case['var'], dtype)
    r, rm = _check_stage0(got, v, S, Cin, dtype), _check_stage0(got, mod, S, Cin, dtype, unfolded=True)
    print(f'[head {family} {shape}] tiles {TILES} x both parity orders, one result; worst err / bound {r.max():.3f} at {_where(r)} vs the model, {rm.max():.3f} vs the module; '
          f'{(got != stored).mean():.2%} of the elements are not the model\'s own rounded value')
    assert np.isfinite(got).all()
    assert r.max() <= 1, (_where(r), got[_where(r)], v[_where(r)])
    assert rm.max() <= 1, (_where(rm), got[_where(rm)], mod[_where(rm)])
    if family == 'relu_clamp':
        assert not got[..., HC.NEG].any()                                            # far negative: stored exactly 0
        if dtype == 'fp16':
            assert (got[..., HC.BIG] == 65504).all()                                 # the store clamp: 65504 exactly, finite
            assert ((got[..., HC.TINY] > 0) & (got[..., HC.TINY] < 2.0 ** -14)).all()   # subnormal outputs are kept


@pytest.mark.parametrize('dtype,B', [('fp16', 1), ('fp16', 3), ('bf16', 3)])
def test_fused_tile_on_deconv1_geometry(dtype, B):
    """EPI_DECONV_FINAL's own gather and epilogue where 192 rows are less than one 256-row tile (B = 1) and where image seams lie inside the tiles and the last tile is
    ragged (B = 3): heatmaps against float64 on stage 0's bits, taps data included (a seam or border leak moves the codes, far outside the bound)"""
    shape = (dtype, B, 16, 12, 384)
    fin = HC.final(dtype, 17)
    for case in (HC.edges(*shape), HC.taps(*shape, 1)):
        a = _ok(dtype, 0, HC.STAGE0_TILES[0], 1, case)['out']
        for pf in (1, 0):
            hm = _ok(dtype, 1, -1, pf, case, fin)['out']
            r = _check_final(hm, a, fin, dtype)
            print(f'[head fused {shape} parity_fast {pf}] worst err / bound {r.max():.3f}')
            assert r.max() <= 1, _where(r)


@pytest.mark.parametrize('Kp', HC.KPS)
@pytest.mark.parametrize('dtype,B', [(s[0], s[1]) for s in HC.FUSED])
def test_final_fused_is_the_two_launches(dtype, B, Kp):
    shape = (dtype, B, 32, 24, 256)
    case, fin = HC.edges(*shape), HC.final(dtype, Kp)
    a = _ok(dtype, 0, -1, 1, case)['out']
    ref_hm = None
    for pf in (1, 0):
        one = _ok(dtype, 1, -1, pf, case, fin)
        two = _ok(dtype, 2, -1, pf, case, fin)
        assert _same(two['mid'], a), f'parity_fast {pf}: the un-fused head\'s 16-bit tensor differs from stage 0 in {(_bits(two["mid"]) != _bits(a)).sum()} elements'
        d = _bits(one['out']) != _bits(two['out'])
        assert not d.any(), f'parity_fast {pf}: {d.sum()} of {d.size} heatmap elements differ between the fused kernel and the two launches; first at {tuple(np.argwhere(d)[0])}'
        ref_hm = one['out'] if ref_hm is None else ref_hm
        assert _same(one['out'], ref_hm), 'the two parity orders differ'
    assert _same(_ok(dtype, 1, -1, 1, case, fin)['out'], ref_hm), 'run-to-run difference'
    r = _check_final(ref_hm, a, fin, dtype)
    print(f'[head final {shape} Kp {Kp}] fused == two launches, both parity orders; worst err / bound {r.max():.3f} at {_where(r)}')
    assert r.max() <= 1, _where(r)
    if Kp >= 16:
        assert _same(ref_hm[:, 3], np.broadcast_to(fin['b_fin'][3], ref_hm[:, 3].shape))       # the zero row returns its bias exactly


def test_the_checker_can_fail():
    """negative control: the model output of `lo plane dropped` and of `seam leak`, handed to the checkers in place of the device's, must fail them"""
    dtype, shape = 'fp16', ('fp16', 2, 32, 24, 256)
    case, p, fin = HC.edges(*shape), HC.edges_parts(*shape), HC.final('fp16', 17)
    v, _, S = HM.stage0(p['z'], p['A'], p['bias'], dtype)
    got = _ok(dtype, 0, -1, 1, case)['out']
    assert _check_stage0(got, v, S, 256, dtype).max() <= 1
    seam = HM.stage0(HM.deconv(case['x'], p['wf'], 'seam'), 0.0, p['bias'], dtype)[1]
    r = _check_stage0(seam, v, S, 256, dtype)
    assert r.max() > 1 and (r[0, -1] > 1).any() and (r[1, 0] > 1).any() and not (r[:, 1:-1] > 1).any()    # the rows at the seam, and only they
    hm = _ok(dtype, 1, -1, 1, case, fin)['out']
    assert _check_final(hm, got, fin, dtype).max() <= 1
    assert _check_final(HM.final(got, fin['w_fin'], fin['b_fin'], dtype, 'lo_dropped')[0], got, fin, dtype).max() > 1


def test_refusals_come_back_as_errors():
    """a tile without a kernel for the epilogue, the fused epilogue off its 256 x 256 tile, the un-fused pair off deconv2's geometry: an error each, nothing launched"""
    case, fin = HC.taps('fp16', 1, 16, 12, 384, 0), HC.final('fp16', 17)
    for stage, variant, f in ((0, 7, None), (0, 16, None), (1, 8, fin), (1, 1, fin), (2, -1, fin)):
        rc, r = _head('fp16', stage, variant, 1, case, f)
        assert rc != 0 and ('invalid' in capi.last_error().lower() or 'head case' in capi.last_error()), (stage, variant, rc, capi.last_error())
        assert np.isnan(r['out']).all()
    rc, _ = _head('fp16', 1, -1, 1, case, None)                    # the final conv's operands missing
    assert rc == capi.VP_ERR_INVALID
