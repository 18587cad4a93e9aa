"""CPU: the training-protocol affine crop route without a device -- its geometry (csrc/affinegeom.h through the host-only tap vp_dbg_box_cs, and the numpy
restatement cropprep.box_to_cs) against the reference's own centres and scales (tests/golden/affine.npz), the inverse map against the reference's warp
matrix, exact anchors of the fixed-point sampling, the host twin against the independent scalar model (tests/affine_model.py), the band plan of the
host-frames entry and every refusal that needs no handle."""
import numpy as np
import pytest

import affine_cases as AC
import affine_model as AM
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.cropprep import Frame, affine_back_map, affine_crops_host, affine_map, box_to_cs, check_cs, rgb_to_nv12
from easy_vitpose_amd.engine import VitPoseHip, affine_plan_host, box_cs_host


@pytest.fixture(scope='module')
def golden(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, 'affine.npz'))


# ------------------------------------------------------------------------------------------------------------------ 1. geometry
def test_box_cs_equals_reference_bit_for_bit(golden):
    """every golden box: the header (vp_dbg_box_cs), the numpy twin and the scalar model give the reference's centre and scale * 200, all 32 bits"""
    assert str(golden['numpy_version']).startswith('2.'), 'the goldens record the float32 widths of numpy 2'
    boxes = golden['boxes']
    assert len(boxes) >= 40
    want = np.concatenate([golden['center'], golden['scale200']], 1)
    cs, st = box_cs_host(boxes)
    assert (st == 0).all()
    assert np.array_equal(cs.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(box_to_cs(boxes).view(np.uint32), want.view(np.uint32))
    mine = np.array([AM.box_cs(b) for b in boxes], dtype=np.float32)
    assert np.array_equal(mine.view(np.uint32), want.view(np.uint32))
    # the named cases are what they claim to be
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    assert w[0] > 0.75 * h[0] and w[1] < 0.75 * h[1] and w[2] == 0.75 * h[2] and (w[3], h[3]) == (2, 3) and (w[4], h[4]) == (3000, 3900)
    assert np.allclose(want[:, 2] / want[:, 3], 0.75, rtol=1e-6)   # every crop is 3:4


def test_box_cs_other_scales_and_row_stride():
    """box_scale other than 1.25, and boxes in a detector's [n, 6] layout: header == numpy twin"""
    rng = np.random.default_rng(5)
    b6 = np.concatenate([AC.geometry_boxes(), rng.uniform(0, 1, (40, 2)).astype(np.float32)], 1)
    for s in (1.0, 1.1, 1.25, 2.5):
        cs, st = box_cs_host(b6, box_scale=s)
        assert (st == 0).all() and np.array_equal(cs.view(np.uint32), box_to_cs(b6, s).view(np.uint32))


def test_box_cs_statuses_in_order():
    """1 bad frame index, 2 not finite, 3 w <= 0 or h <= 0 -- in that order of precedence; such rows are all zero.  A huge finite box is clamped, not refused"""
    nan, inf = np.nan, np.inf
    boxes = np.array([[10, 10, 50, 60], [nan, 10, 50, 60], [10, 10, inf, 60], [50, 10, 50, 60], [10, 60, 50, 10], [nan, 0, 0, 0], [10, 10, 50, 60],
                      [-1e30, -1e30, 1e30, 1e30], [0, 0, 1e-45, 1e-45]], dtype=np.float32)
    fidx = np.array([0, 0, 1, 0, 1, 7, -1, 0, 0], dtype=np.int32)
    cs, st = box_cs_host(boxes, fidx, n_frames=2)
    assert st.tolist() == [0, 2, 2, 3, 3, 1, 1, 0, 3]
    assert (cs[st != 0] == 0).all() and (cs[0] != 0).all()
    assert cs[7, 2] == 2 ** 24 and cs[7, 3] == 2 ** 24 and np.isfinite(cs[7]).all()   # clamped per side
    for bad in ([[nan, 10, 50, 60]], [[50, 10, 50, 60]], [[0, 0, 1e-45, 1e-45]]):
        with pytest.raises(ValueError):
            box_to_cs(np.array(bad, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------ 2. the map
def test_inverse_map_inverts_the_reference_warp(golden):
    """The reference's forward matrix M = get_warp_matrix(0, c 2, [191, 255], S) composed with the contract's inverse map at the four crop corners.
    Exactly, M maps src_x(ox) back to ox: m00 = 191 / S_w, m02 = m00 (S_w / 2 - cx), so m00 src_x + m02 = ox.  The reference stores both entries as
    float32: each carries a relative error of at most u = 2^-24, so the composed error is at most u (|m00 src_x| + |m02|) = u (191 / S_w)(|src_x| + |cx - S_w / 2|)
    -- a few ulp32 of the largest frame coordinate times the magnification -- and twice that is asserted (the reference evaluates the entries in float64
    before the float32 store; the float64 arithmetic of this test is 2^-29 of that).  Likewise y with 255 and S_h."""
    cs = np.concatenate([golden['center'], golden['scale200']], 1)
    u = 2.0 ** -24
    worst = 0.0
    for row, M in zip(cs, golden['warp'].astype(np.float64)):
        assert M[0, 1] == 0 and M[1, 0] == 0   # no rotation
        a_x, b_x, a_y, b_y = affine_map(row)
        cx, cy, sw, sh = (float(v) for v in row)
        for ox in (0, 191):
            for oy in (0, 255):
                sx, sy = ox * a_x + b_x, oy * a_y + b_y
                dx, dy = M[0, 0] * sx + M[0, 2] - ox, M[1, 1] * sy + M[1, 2] - oy
                bx = 2 * u * (191.0 / sw) * (abs(sx) + abs(cx - sw / 2))
                by = 2 * u * (255.0 / sh) * (abs(sy) + abs(cy - sh / 2))
                assert abs(dx) <= bx + 1e-12 and abs(dy) <= by + 1e-12, (row, ox, oy, dx, bx, dy, by)
                worst = max(worst, abs(dx), abs(dy))
    print(f'inverse map o forward matrix: worst corner error {worst:.3e} crop px')


# ------------------------------------------------------------------------------------------------------------------ 3. exact anchors
def test_exact_anchors():
    f = AC.frame_rgb((520, 400), 81)
    fi = f.astype(np.int64)
    one = affine_crops_host(f, [[95.5, 127.5, 191, 255]])[0]
    assert np.array_equal(one, f[0:256, 0:192])                                         # A = 1, B = 0: the frame itself
    two = affine_crops_host(f, [[191, 255, 382, 510]])[0]
    assert np.array_equal(two, f[0:512:2, 0:384:2])                                     # A = 2, B = 0: every second pixel
    half = affine_crops_host(f, [[47.75, 63.75, 95.5, 127.5]])[0].astype(np.int64)      # A = 1 / 2: source pixels and midpoints alternate
    assert np.array_equal(half[0::2, 0::2], fi[0:128, 0:96])
    assert np.array_equal(half[0::2, 1::2], (fi[0:128, 0:96] + fi[0:128, 1:97] + 1) >> 1)
    assert np.array_equal(half[1::2, 0::2], (fi[0:128, 0:96] + fi[1:129, 0:96] + 1) >> 1)
    assert np.array_equal(half[1::2, 1::2], (fi[0:128, 0:96] + fi[0:128, 1:97] + fi[1:129, 0:96] + fi[1:129, 1:97] + 2) >> 2)
    assert not affine_crops_host(f, [[-300.0, -400.0, 191, 255]]).any()                 # wholly outside
    assert not affine_crops_host(f, [[1e6, 50.0, 30, 40]]).any()
    corner = affine_crops_host(f, [[95.5 - 10, 127.5 - 20, 191, 255]])[0]               # A = 1, B = (-10, -20): over the top-left corner
    assert not corner[:20].any() and not corner[:, :10].any()
    assert np.array_equal(corner[20:, 10:], f[0:236, 0:182])
    far = affine_crops_host(f[:100, :80], [[95.5 + 30, 127.5 + 40, 191, 255]])[0]       # over the bottom-right corner of a small frame
    assert np.array_equal(far[:60, :50], f[40:100, 30:80]) and not far[60:].any() and not far[:, 50:].any()
    # the scalar model at two of them
    rows = AM.frame_to_rgb_rows('rgb', (f,))
    assert np.array_equal(AM.crop(rows, (95.5, 127.5, 191, 255)), one)
    assert np.array_equal(AM.crop(rows, (95.5 - 10, 127.5 - 20, 191, 255)), corner)


# ------------------------------------------------------------------------------------------------------------------ 4. host routes agree
def _layouts():
    """frame B in every layout the entries take: (name, Frame for the product, (kind, planes, matrix) for the scalar model)"""
    _, fb = AC.frames()
    h, w = fb.shape[:2]
    wide = np.zeros((h, w + 7, 3), np.uint8)
    wide[:, :w] = fb
    y, uv = rgb_to_nv12(fb, 'bt709')
    ywide = np.zeros((h, w + 12), np.uint8)
    ywide[:, :w] = y
    bgr = np.ascontiguousarray(fb[..., ::-1])
    return [('rgb', Frame.rgb(fb), ('rgb', (fb,), None)),
            ('bgr', Frame.bgr(bgr), ('bgr', (bgr,), None)),
            ('rgb pitched', Frame.rgb(wide[:, :w]), ('rgb', (wide[:, :w],), None)),
            ('nv12 bt709', Frame.nv12(y, uv, 'bt709'), ('nv12', (y, uv), 'bt709')),
            ('nv12 pitched bt601', Frame.nv12(ywide[:, :w], uv, 'bt601'), ('nv12', (ywide[:, :w], uv), 'bt601'))]


def test_host_twin_equals_the_scalar_model():
    """affine_crops_host == tests/affine_model.py bit for bit on RGB, BGR, NV12 and pitched frames: crops that magnify, reduce and cross the border"""
    boxes, fidx = AC.e2e_boxes()
    cs = box_to_cs(boxes[fidx == 1])
    cs = np.concatenate([cs, [[40.0, 30.0, 400.0, 533.0], [131.0, 95.0, 9.0, 12.0]]]).astype(np.float32)   # the whole frame inside the crop; 9 x 12 px at its corner
    for name, frame, (kind, planes, matrix) in _layouts():
        rows = AM.frame_to_rgb_rows(kind, planes, matrix) if matrix else AM.frame_to_rgb_rows(kind, planes)
        got = affine_crops_host(frame, cs)
        for i, row in enumerate(cs):
            assert np.array_equal(got[i], AM.crop(rows, row)), (name, i)
    fa, _ = AC.frames()
    rows = AM.frame_to_rgb_rows('rgb', (fa,))
    csa = box_to_cs(boxes[fidx == 0])
    got = affine_crops_host(fa, csa)
    for i in (0, 2):
        assert np.array_equal(got[i], AM.crop(rows, csa[i]))


def test_back_map_equals_the_scalar_model():
    rng = np.random.default_rng(9)
    cs = box_to_cs(AC.geometry_boxes())
    kp = np.stack([rng.uniform(-1, 63, (40, 5)), rng.uniform(-1, 47, (40, 5)), rng.uniform(0, 1, (40, 5))], -1).astype(np.float32)
    got = affine_back_map(kp, cs)
    for i in range(40):
        for k in range(5):
            x, y = AM.back_map(float(kp[i, k, 1]), float(kp[i, k, 0]), cs[i])
            assert got[i, k, 0] == y and got[i, k, 1] == x and got[i, k, 2] == kp[i, k, 2]


# ------------------------------------------------------------------------------------------------------------------ 5. the band plan
def test_band_plan():
    """vp_dbg_affine_plan: per frame the union of the rows its crops tap -- rows sy(0) .. sy(255) + 1 of the scalar model's axis function, clipped to the
    frame -- {0, 0} for a frame without crops or whose crops lie outside; every layout"""
    fa, fb = AC.frames()
    boxes, fidx = AC.e2e_boxes()
    cs = box_to_cs(boxes)
    y, uv = rgb_to_nv12(fb)
    spare = np.zeros((50, 60, 3), np.uint8)
    for frames in ([fa, fb, spare], [Frame.bgr(np.ascontiguousarray(fa[..., ::-1])), Frame.nv12(y, uv), spare]):
        bands = affine_plan_host(frames, fidx, cs)
        want = np.zeros((3, 2), np.int64)
        for f, hh in ((0, fa.shape[0]), (1, fb.shape[0])):
            lo, hi = [], []
            for row in cs[fidx == f]:
                _, _, a_y, b_y = AM.inverse_map(row)
                lo.append(min(max(AM.axis(0, a_y, b_y)[0], 0), hh))
                hi.append(min(max(AM.axis(255, a_y, b_y)[0] + 2, 0), hh))
            want[f] = (min(lo), max(hi))
        assert np.array_equal(bands, want), (bands, want)
        assert bands[0, 0] == 0 and bands[0, 1] == 240      # a box over the top edge and one to the bottom
    # one crop inside a tall frame: only its rows; crops outside (above, below, and beside) add nothing
    tall = np.zeros((1000, 64, 3), np.uint8)
    b = affine_plan_host([tall], None, [[32.0, 500.5, 30.0, 40.0], [32.0, -500.0, 30.0, 40.0], [32.0, 5000.0, 30.0, 40.0]])
    assert b.tolist() == [[480, 522]]                        # src_y(0) = 480.5, src_y(255) = 520.5: rows 480 .. 521
    assert affine_plan_host([tall], None, [[32.0, -500.0, 30.0, 40.0]]).tolist() == [[0, 0]]
    assert affine_plan_host([tall], None, np.zeros((0, 4), np.float32)).tolist() == [[0, 0]]


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def _plan_rc(images, n_images, fidx, cs, n):
    lib = capi.load_library()
    return lib.vp_dbg_affine_plan(images, n_images, None if fidx is None else fidx.ctypes.data, None if cs is None else cs.ctypes.data, n, None)


def test_plan_refusals():
    """everything vp_infer_images_affine refuses before it touches the device (vp_dbg_affine_plan runs the same function)"""
    f = np.zeros((64, 48, 3), np.uint8)
    im = (capi.vp_image * 1)()
    im[0] = capi.vp_image((capi.C.c_void_p * 2)(f.ctypes.data, None), (capi.C.c_int64 * 2)(144, 0), 64, 48, 0, 0)
    ok = np.array([[24, 32, 30, 40]], np.float32)
    assert _plan_rc(im, 1, None, ok, 1) == capi.VP_OK
    for bad in ([np.nan, 32, 30, 40], [24, np.inf, 30, 40], [24, 32, 0, 40], [24, 32, 30, -1], [24, 32, np.nan, 40], [24, 32, 30, 2.0 ** 25], [24, 32, np.inf, 40]):
        assert _plan_rc(im, 1, None, np.array([bad], np.float32), 1) == capi.VP_ERR_INVALID, bad
        assert 'crop 0' in capi.last_error()
        with pytest.raises(ValueError):
            check_cs([bad])
    for fi in (-1, 1):
        assert _plan_rc(im, 1, np.array([fi], np.int32), ok, 1) == capi.VP_ERR_INVALID and 'frame index' in capi.last_error()
    assert _plan_rc(im, 1, None, None, 1) == capi.VP_ERR_INVALID
    assert _plan_rc(None, 1, None, ok, 1) == capi.VP_ERR_INVALID
    assert _plan_rc(im, 0, None, ok, 1) == capi.VP_ERR_INVALID
    assert _plan_rc(im, 1, None, ok, -1) == capi.VP_ERR_INVALID
    for field, value in (('format', 9), ('h', 0), ('w', 1 << 25)):
        bad_im = (capi.vp_image * 1)()
        bad_im[0] = capi.vp_image((capi.C.c_void_p * 2)(f.ctypes.data, None), (capi.C.c_int64 * 2)(144, 0), 64, 48, 0, 0)
        setattr(bad_im[0], field, value)
        assert _plan_rc(bad_im, 1, None, ok, 1) == capi.VP_ERR_INVALID, field
    small_pitch = (capi.vp_image * 1)()
    small_pitch[0] = capi.vp_image((capi.C.c_void_p * 2)(f.ctypes.data, None), (capi.C.c_int64 * 2)(100, 0), 64, 48, 0, 0)
    assert _plan_rc(small_pitch, 1, None, ok, 1) == capi.VP_ERR_INVALID and 'pitch' in capi.last_error()
    nv = (capi.vp_image * 1)()
    nv[0] = capi.vp_image((capi.C.c_void_p * 2)(f.ctypes.data, None), (capi.C.c_int64 * 2)(48, 48), 64, 48, capi.VP_PIX_NV12, 0)
    assert _plan_rc(nv, 1, None, ok, 1) == capi.VP_ERR_INVALID and 'UV plane' in capi.last_error()


def test_box_cs_tap_refusals():
    lib = capi.load_library()
    b = np.array([[1, 2, 30, 40]], np.float32)
    cs, st = np.zeros((1, 4), np.float32), np.zeros(1, np.int32)
    call = lambda stride, scale, n=1, ptr=b.ctypes.data: lib.vp_dbg_box_cs(ptr, stride, None, 1, n, scale, cs.ctypes.data, st.ctypes.data)
    assert call(4, 1.25) == capi.VP_OK
    assert call(3, 1.25) == capi.VP_ERR_INVALID and 'row_stride' in capi.last_error()
    for s in (0.0, -1.0, float('nan'), float('inf')):
        assert call(4, s) == capi.VP_ERR_INVALID and 'box_scale' in capi.last_error()
        with pytest.raises(ValueError):
            box_to_cs(b, s)
    assert call(4, 1.25, n=-1) == capi.VP_ERR_INVALID
    assert call(4, 1.25, ptr=None) == capi.VP_ERR_INVALID


def test_python_refusals():
    """what the Python layers refuse before any library call: the combinations that are out of scope for the affine route, and unknown crop names"""
    from easy_vitpose_amd import VitInference
    from easy_vitpose_amd.posenms import PoseNms
    bare = VitPoseHip.__new__(VitPoseHip)   # no handle: every refusal below comes before the library is used
    bare.device_id = 0
    with pytest.raises(ValueError, match='nms'):
        bare.infer_boxes([], None, crop='affine', nms=PoseNms())
    with pytest.raises(ValueError, match='datasets'):
        bare.infer_boxes([], None, crop='affine', datasets=['coco'])
    with pytest.raises(ValueError, match='crop params'):
        bare.infer_boxes([], None, crop='affine', crop_params=True)
    for s in (0, -2.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='box_scale'):
            bare.infer_boxes([], None, crop='affine', box_scale=s)
    with pytest.raises(ValueError, match="cs=True"):
        bare.infer_boxes([], None, cs=True)
    with pytest.raises(ValueError, match="'pad' or 'affine'"):
        bare.infer_boxes([], None, crop='warp')
    with pytest.raises(ValueError, match="'pad' or 'affine'"):
        bare.infer_frames([], np.zeros((0, 9), np.int32), crop='rotate')
    with pytest.raises(ValueError, match='datasets'):
        bare.infer_frames([], np.zeros((0, 5)), datasets=['coco'], crop='affine')
    with pytest.raises(ValueError, match='whole frame index'):
        bare.infer_frames([], np.array([[0.5, 1, 2, 3, 4]]), crop='affine')
    det = lambda img: np.zeros((0, 5))
    with pytest.raises(ValueError, match='pose_nms'):
        VitInference({}, det, 's', dataset='coco', crop='affine', pose_nms=PoseNms())
    with pytest.raises(ValueError, match="'pad' or 'affine'"):
        VitInference({}, det, 's', dataset='coco', crop='udp')
    with pytest.raises(ValueError, match='box_scale'):
        VitInference({}, det, 's', dataset='coco', crop='affine', box_scale=0)
    assert not hasattr(__import__('easy_vitpose_amd').VitPoseGroup, 'infer_frames')   # the group has no frames entry: nothing to half-support


def test_cli_arguments():
    from easy_vitpose_amd.cli import build_parser
    ap = build_parser()
    base = ['--input', 'x.png', '--synthetic', 's', '--boxes', 'b.json']
    a = ap.parse_args(base)
    assert a.crop == 'pad' and a.box_scale == 1.25                      # the default at every layer
    a = ap.parse_args(base + ['--crop', 'affine', '--box-scale', '1.1'])
    assert a.crop == 'affine' and a.box_scale == 1.1
    with pytest.raises(SystemExit):
        ap.parse_args(base + ['--crop', 'rotate'])


def test_abi_declares_the_route():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vitpose_hip.h')).read()
    assert '#define VP_HAS_AFFINE_CROP 1' in header and '#define VP_ABI_VERSION 4' in header
    lib = capi.load_library()
    assert lib.vp_abi_version() == 4
    for name in ['vp_infer_images_affine', 'vp_infer_boxes_affine_stream', 'vp_dbg_box_cs', 'vp_dbg_affine_plan', 'vp_dbg_crop_affine', 'vp_dbg_decode_affine',
                 'vp_dbg_decode_affine_flip']:
        assert name in capi.SYMBOLS and hasattr(lib, name) and name in header


def test_fp64_decode_model_within_the_gpu_bound(golden):
    """The bound the GPU decode test asserts, checked on the CPU first: the fp64 model (the oracle's DARK step + affine_model.back_map) against the reference's
    own keypoints.  bound = 2e-3 max(1, S_w / 192) + 4 ulp32(max(|coord|, S)) per axis (tests/test_gpu_affine.py states its derivation)."""
    from cases import peaked_heatmaps
    from test_gpu_affine import decode_bound
    cs = np.concatenate([golden['center'], golden['scale200']], 1)
    for K, seed in AC.DECODE_SEEDS.items():
        exp = golden[f'decode_k{K}']
        got = AM.decode(peaked_heatmaps(len(cs), K, seed), cs)
        assert np.array_equal(got[..., 2], exp[..., 2])
        d = np.abs(got[..., :2].astype(np.float64) - exp[..., :2])
        bound = decode_bound(exp, cs)
        print(f'K = {K}: fp64 model vs reference max {d.max():.3e} px, worst ratio to the bound {(d / bound).max():.3f}')
        assert (d <= bound).all()
