"""CPU: the orient stage's host side (csrc/orientgeom.h through the tap vp_dbg_orient_host, vp_orient_plan, easy_vitpose_amd/devorient.py, VitInference(rotate=),
the CLI's --rotate-on) against models that do not share its code: the numpy twin written by slicing, np.rot90 and slices written here, Pillow's transposes, the
algebra of the eight codes, and the NV12 property to_rgb(orient(f)) == orient(to_rgb(f)).  A permutation of bytes: equal means equal bytes, canaries included."""
from __future__ import annotations

import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.cropprep import Frame, rgb_to_nv12, to_rgb
from easy_vitpose_amd.devletterbox import IMAGE_DTYPE, image_table
from easy_vitpose_amd.devorient import (INVERSE, MAX_IMAGES, ORIENT_CODES, DeviceOrient, HostOrient, orient_host_numpy, orient_plan, oriented_hw, rotate_code)
from orient_cases import CANARY, EXTENTS, T, buffers, expected_parents, frames_equal, named_cases, same_bits, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = named_cases()


def ptr(table):
    return C.cast(table.ctypes.data, C.POINTER(capi.vp_image)) if len(table) else None


def rgb(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def nv12(h, w, seed, matrix='bt601'):
    rng = np.random.default_rng(seed)
    return Frame.nv12(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8), matrix)


def by_hand(a, code):
    """the table of the contract in np.rot90 and slices, written here"""
    return {1: lambda: a, 2: lambda: a[:, ::-1], 3: lambda: np.rot90(a, 2), 4: lambda: a[::-1], 5: lambda: np.swapaxes(a, 0, 1), 6: lambda: np.rot90(a, -1),
            7: lambda: np.swapaxes(np.rot90(a, 2), 0, 1), 8: lambda: np.rot90(a, 1)}[code]()


def test_surface_symbols_macros_and_build_lists():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    for name in ('vp_orient_plan', 'vp_orient_stream', 'vp_orient', 'vp_dbg_orient_host'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r'VP_API\s+int\s+' + name + r'\s*\(', hdr), name
    assert re.search(r'#define\s+VP_HAS_ORIENT\s+1\b', hdr) and re.search(r'#define\s+VP_ORIENT_MAX_IMAGES\s+64\b', hdr)
    for name, value in (('IDENTITY', 1), ('MIRROR', 2), ('ROT180', 3), ('FLIP', 4), ('TRANSPOSE', 5), ('CW90', 6), ('TRANSVERSE', 7), ('CCW90', 8)):
        assert re.search(r'#define\s+VP_ORIENT_%s\s+%d\b' % (name, value), hdr) and ORIENT_CODES[name.lower()] == value, name
    assert MAX_IMAGES == 64 and IMAGE_DTYPE.itemsize == C.sizeof(capi.vp_image) == 48
    geom = open(os.path.join(ROOT, 'easy_vitpose_amd', 'csrc', 'orientgeom.h')).read()
    assert re.search(r'ORIENT_TILE\s*=\s*%d\b' % T, geom), 'the cases are built around the kernel\'s tile edge'
    build = __import__('easy_vitpose_amd.build', fromlist=['SOURCES'])
    assert 'orient.hip' in build.SOURCES and 'orientgeom.h' in build.HEADERS
    assert lib.vp_abi_version() == 4


def test_what_the_cases_cover():
    specs = [s for v in CASES.values() for s in v]
    for fmt in ('rgb', 'bgr', 'nv12'):
        mine = [s for s in specs if s.fmt == fmt]
        assert {s.code for s in mine} == set(range(1, 9))
        assert {s.pitch for s in mine} == {s.dpitch for s in mine} == {'tight', 'p1', 'p13', 'a256'} and {s.offset for s in mine} == {s.doffset for s in mine} == {0, 1, 5}
    assert {(s.h, s.w) for s in specs if s.fmt == 'rgb'} >= {(h, w) for h in EXTENTS for w in EXTENTS} and EXTENTS == (1, 2, T - 1, T, T + 1, 2 * T + 1)
    assert any(s.fmt == 'nv12' and s.h % 2 and s.w % 2 and s.code == 5 for s in specs) and any(s.fmt == 'nv12' and s.h % 2 and s.code == 1 for s in specs)
    assert any((3 * s.w) % 4 for s in specs if s.fmt != 'nv12') and any((3 * s.w) % 16 and not (3 * s.w) % 4 for s in specs if s.fmt != 'nv12')
    assert len(CASES['mixed_64']) == 64 and len(CASES['frames_33']) == 33 and CASES['n_0'] == []
    m = CASES['mixed_64']
    assert len({(s.h, s.w) for s in m}) > 40 and {s.fmt for s in m} == {'rgb', 'bgr', 'nv12'} and {s.code for s in m} == set(range(1, 9))


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_tap_equals_the_numpy_twin_and_touches_nothing_else(name):
    """values, and every byte outside the row bytes of the destination rows (pitch gaps included), and every source byte"""
    specs = CASES[name]
    b = buffers(specs)
    before = [p.copy() for p in b.src_parents]
    out = HostOrient().orient(b.src, b.codes, out=b.dst)
    want = [orient_host_numpy(f, s.code) for f, s in zip(b.tight, specs)]
    assert all(o is d for o, d in zip(out, b.dst))
    for k, (got, exp) in enumerate(zip(b.dst_parents, expected_parents(specs, want))):
        assert same_bits(got, exp), f'destination plane {k} or the bytes around it'
    assert all(same_bits(p, q) for p, q in zip(b.src_parents, before)), 'a source byte changed'
    fresh = HostOrient().orient(b.src, b.codes)   # tight planes of its own
    assert all(frames_equal(g, w) for g, w in zip(fresh, want))


@pytest.mark.parametrize('code', range(1, 9))
def test_rgb_against_rot90_slices_and_pillow(code):
    for h, w in ((1, 1), (5, 7), (T + 1, 3), (2, T + 1)):
        a = rgb(h, w, code + h)
        want = np.ascontiguousarray(by_hand(a, code))
        for make in (Frame.rgb, Frame.bgr):
            got = HostOrient().orient([make(a)], code)[0]
            assert (got.h, got.w) == oriented_hw((h, w), code) == want.shape[:2] and same_bits(got.planes[0], want)
        assert same_bits(orient_host_numpy(a, code).planes[0], want)
        y = a[..., 0].copy()   # a one-byte plane through the twin's plane function
        assert same_bits(by_hand(y, code), by_hand(a, code)[..., 0])
    try:
        from PIL import Image
    except ImportError:   # Pillow is an independent witness where it is installed, not a requirement
        Image = None
    if Image is not None and code > 1:
        T_ = getattr(Image, 'Transpose', Image)
        method = {2: T_.FLIP_LEFT_RIGHT, 3: T_.ROTATE_180, 4: T_.FLIP_TOP_BOTTOM, 5: T_.TRANSPOSE, 6: T_.ROTATE_270, 7: T_.TRANSVERSE, 8: T_.ROTATE_90}[code]
        a = rgb(9, 14, 77)
        assert same_bits(HostOrient().orient([Frame.rgb(a)], code)[0].planes[0], np.asarray(Image.fromarray(a).transpose(method)))


def test_the_algebra_of_the_codes():
    tap = HostOrient()
    for f in (Frame.rgb(rgb(6, 11, 1)), Frame.bgr(rgb(T + 1, 5, 2)), nv12(6, 10, 3, 'bt709'), nv12(2 * T + 2, 4, 4)):
        g = f
        for _ in range(4):
            g = tap.orient([g], 8)[0]
        assert frames_equal(g, f), 'code 8 four times'
        assert frames_equal(tap.orient(tap.orient([f], 8), 6)[0], f), '6 after 8'
        for code in range(1, 9):
            assert frames_equal(tap.orient(tap.orient([f], code), INVERSE[code])[0], f), f'code {code} and its inverse {INVERSE[code]}'
        assert frames_equal(tap.orient(tap.orient([f], 2), 4)[0], tap.orient([f], 3)[0]) and frames_equal(tap.orient(tap.orient([f], 5), 3)[0], tap.orient([f], 7)[0])
    assert INVERSE == {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}


def test_nv12_orientation_commutes_with_the_conversion_to_rgb():
    """to_rgb(orient(f)) == orient(to_rgb(f)) for every admitted (code, size); what is not admitted is refused by the tap and by the twin"""
    tap = HostOrient()
    seen = refused = 0
    for h in (1, 2, 3, 4, 7, 8, T, T + 1):
        for w in (1, 2, 3, 6, 9, T + 2):
            for code in range(1, 9):
                f = nv12(h, w, 100 * h + w, ('bt601', 'bt709', 'bt601_full')[(h + w) % 3])
                rev_row, rev_col = code in (3, 4, 6, 7), code in (2, 3, 7, 8)
                if (rev_row and h % 2) or (rev_col and w % 2):
                    with pytest.raises(capi.VpError, match=rf'frame 0 is NV12 of {h} x {w}: code {code} reverses an axis of odd length'):
                        tap.orient([f], code)
                    with pytest.raises(ValueError, match='reverses an axis of odd length'):
                        orient_host_numpy(f, code)
                    refused += 1
                    continue
                got = tap.orient([f], code)[0]
                assert got.matrix == f.matrix and same_bits(to_rgb(got), by_hand(to_rgb(f), code)), (h, w, code)
                seen += 1
    assert seen > 200 and refused > 100
    # and the frames rgb_to_nv12 makes
    f = Frame.nv12(*rgb_to_nv12(rgb(10, 12, 5)))
    assert all(same_bits(to_rgb(tap.orient([f], c)[0]), by_hand(to_rgb(f), c)) for c in range(1, 9))


def test_plan_sizes_against_integers():
    for fmt, es in (('rgb', 3), ('bgr', 3), ('nv12', None)):
        for h, w in ((1, 1), (4, 6), (3, 7), (T + 1, 2), (1080, 1920)):
            for code in range(1, 9):
                if fmt == 'nv12' and code not in (1, 5) and (h % 2 or w % 2):
                    continue
                oh, ow = (w, h) if code >= 5 else (h, w)
                rows = (oh, (oh + 1) // 2 if fmt == 'nv12' else 0)
                row_bytes = (ow, 2 * ((ow + 1) // 2)) if fmt == 'nv12' else (3 * ow, 0)
                hw, pitch, nbytes = orient_plan([(h, w)], code, fmt)
                assert hw.tolist() == [[oh, ow]] and pitch.tolist() == [list(row_bytes)]
                assert nbytes.tolist() == [[(r - 1) * p + p if r else 0 for r, p in zip(rows, row_bytes)]]
                keep = (row_bytes[0] + 13, 512 if fmt == 'nv12' and row_bytes[1] <= 512 else 0)
                hw, pitch, nbytes = orient_plan([(h, w)], code, fmt, pitch=[keep])
                want_pitch = [keep[0], keep[1] or row_bytes[1]]
                assert pitch.tolist() == [want_pitch] and nbytes.tolist() == [[(r - 1) * p + rb if r else 0 for r, p, rb in zip(rows, want_pitch, row_bytes)]]
    # the plan leaves plane pointers alone, fills format and matrix, takes 64 frames and none
    src, dst = image_table([nv12(4, 6, 1, 'bt709')]), np.zeros(1, IMAGE_DTYPE)
    dst['plane'] = (123, 456)
    codes = np.array([6], np.int32)
    lib = capi.load_library()
    assert lib.vp_orient_plan(ptr(src), codes.ctypes.data, 1, ptr(dst), None) == capi.VP_OK
    assert dst['plane'].tolist() == [[123, 456]] and (dst['h'][0], dst['w'][0], dst['format'][0], dst['matrix'][0]) == (6, 4, capi.VP_PIX_NV12, capi.VP_YUV_BT709)
    assert len(orient_plan([(2, 2)] * 64, 3)[0]) == 64 and len(orient_plan(np.zeros((0, 2)), [])[0]) == 0
    assert lib.vp_orient_plan(None, None, 0, None, None) == capi.VP_OK and lib.vp_dbg_orient_host(None, None, None, 0) == capi.VP_OK


def test_refusals_of_the_c_entries_name_the_frame_and_write_nothing():
    lib = capi.load_library()
    specs = [spec('rgb', 5, 7, 6, 'p13', 1, seed=1), spec('nv12', 6, 8, 3, 'p1', 5, seed=2)]
    b = buffers(specs)
    src0, dst0, codes0 = image_table(b.src), image_table(b.dst), b.codes.copy()
    NV, RGB = capi.VP_PIX_NV12, capi.VP_PIX_RGB24

    def refused(match, src=None, dst=None, codes=None, n=2, plan_too=True):
        s, d, c = (src0 if src is None else src), (dst0 if dst is None else dst), (codes0 if codes is None else codes)
        entries = [lambda: lib.vp_dbg_orient_host(ptr(s) if s is not False else None, c.ctypes.data if c is not False else None, ptr(d) if d is not False else None, n)]
        if plan_too:
            entries.append(lambda: lib.vp_orient_plan(ptr(s) if s is not False else None, c.ctypes.data if c is not False else None, n, ptr(d.copy()) if d is not False else None, None))
        for call in entries:
            assert call() == capi.VP_ERR_INVALID
            assert re.search(match, capi.last_error()), capi.last_error()
        assert all((p == CANARY).all() for p in b.dst_parents), 'a refused call wrote'

    def edit(tab, i, **kw):
        t = tab.copy()
        for k, v in kw.items():
            t[k][i] = v
        return t

    refused('null src, codes or dst with n > 0', src=False)
    refused('null src, codes or dst with n > 0', codes=False)
    refused('null src, codes or dst with n > 0', dst=False)
    refused(r'n = -1 outside 0\.\.64', n=-1)
    refused(r'n = 65 outside 0\.\.64', n=65)
    for bad in (0, 9, -3):
        refused(rf'frame 1 has orientation code {bad} outside 1\.\.8', codes=np.array([6, bad], np.int32))
    refused('frame 1 has an unknown pixel format 3', src=edit(src0, 1, format=3))
    refused('frame 1 has an unknown YUV matrix 7', src=edit(src0, 1, matrix=7))
    refused('frame 0 has a negative pitch', src=edit(src0, 0, pitch=(-21, 0)))
    refused(r'frame 0 has pitch\[0\] 20 below its 21 row bytes', src=edit(src0, 0, pitch=(20, 0)))
    refused(r'frame 1 has pitch\[1\] 7 below the 8 bytes of a UV row', src=edit(src0, 1, pitch=(9, 7)))
    refused('frame 1 has a non-positive size 0 x 8', src=edit(src0, 1, h=0))
    refused('frame 0 has a non-positive size 5 x -2', src=edit(src0, 0, w=-2))
    refused('frame 1 is NV12 of 5 x 8: code 3 reverses an axis of odd length', src=edit(src0, 1, h=5))
    refused('frame 1 is NV12 of 6 x 7: code 8 reverses an axis of odd length', src=edit(src0, 1, w=7, pitch=(9, 9)), codes=np.array([6, 8], np.int32))
    refused(r'frame 0: dst pitch\[0\] 14 is below its 15 row bytes', dst=edit(dst0, 0, pitch=(14, 0)))
    refused(r'frame 1: dst pitch\[1\] 6 is below its 8 row bytes', dst=edit(dst0, 1, pitch=(9, 6)))
    # what only the entries that move pixels refuse: the plan reads no pointer and accepts what it is about to overwrite
    refused(r'frame 0 has no data \(src plane\[0\] is null\)', src=edit(src0, 0, plane=(0, 0)), plan_too=False)
    refused(r'frame 1 has no data \(src plane\[1\] is null\)', src=edit(src0, 1, plane=(src0['plane'][1][0], 0)), plan_too=False)
    refused(r'frame 1 has nowhere to go \(dst plane\[1\] is null\)', dst=edit(dst0, 1, plane=(dst0['plane'][1][0], 0)), plan_too=False)
    refused('frame 0: dst is 5 x 7 format 0 matrix 0, the plan says 7 x 5 format 0 matrix 0', dst=edit(dst0, 0, h=5, w=7, pitch=(34, 0)), plan_too=False)
    refused('frame 0: dst is 7 x 5 format 1 matrix 0, the plan says 7 x 5 format 0', dst=edit(dst0, 0, format=1), plan_too=False)
    refused('frame 1: dst is 6 x 8 format 2 matrix 1, the plan says 6 x 8 format 2 matrix 0', dst=edit(dst0, 1, matrix=1), plan_too=False)
    # overlap: in place, a destination inside a source of another frame, two destinations one byte into each other
    same = buffers([spec('rgb', 4, 4, 3, seed=3), spec('rgb', 4, 4, 2, seed=4)])
    s2, d2 = image_table(same.src), image_table(same.dst)
    for tab_s, tab_d, match in ((s2, edit(d2, 1, plane=(s2['plane'][1][0], 0)), 'a dst plane of frame 1 overlaps a src plane of frame 1'),
                                (s2, edit(d2, 0, plane=(s2['plane'][1][0] + 47, 0)), 'a dst plane of frame 0 overlaps a src plane of frame 1'),
                                (s2, edit(d2, 1, plane=(d2['plane'][0][0] + 47, 0)), 'a dst plane of frame [01] overlaps a dst plane of frame [01]')):
        before = [p.copy() for p in same.src_parents + same.dst_parents]
        assert lib.vp_dbg_orient_host(ptr(tab_s), same.codes.ctypes.data, ptr(tab_d), 2) == capi.VP_ERR_INVALID
        assert re.search(match + r' \(there is no in-place orientation\)', capi.last_error()), capi.last_error()
        assert all(same_bits(p, q) for p, q in zip(same.src_parents + same.dst_parents, before))
    # two frames may share a source; planes that touch without sharing a byte are apart
    shared = edit(s2, 1, plane=(s2['plane'][0][0], 0))
    assert lib.vp_dbg_orient_host(ptr(shared), same.codes.ctypes.data, ptr(d2), 2) == capi.VP_OK
    # the good call goes through after all of that
    assert lib.vp_dbg_orient_host(ptr(src0), codes0.ctypes.data, ptr(dst0), 2) == capi.VP_OK
    assert all(frames_equal(Frame(d.format, tuple(np.ascontiguousarray(p) for p in d.planes), d.matrix), orient_host_numpy(f, s.code)) for d, f, s in zip(b.dst, b.tight, specs))


def test_rotate_code_and_the_python_refusals():
    assert [rotate_code(a) for a in (0, 90, 180, 270)] == [1, 8, 3, 6]
    a = rgb(4, 6, 1)
    for angle in (90, 180, 270):   # the reference's rotation_map: counter-clockwise degrees
        assert same_bits(orient_host_numpy(a, rotate_code(angle)).planes[0], np.rot90(a, angle // 90))
    for bad in (45, -90, 360, 90.0, '90', None, True):
        with pytest.raises(ValueError, match='rotate: one of 0, 90, 180, 270 expected'):
            rotate_code(bad)
    assert oriented_hw((3, 5), 4) == (3, 5) and oriented_hw((3, 5), 'cw90') == (5, 3)
    tap = HostOrient()
    f = Frame.rgb(a)
    for bad in (0, 9, 2.0, 'sideways', None, True):
        with pytest.raises(ValueError, match=r'frame 1: an orientation code in 1\.\.8'):
            tap.orient([f, f], [1, bad])
    with pytest.raises(ValueError, match='orient: 3 codes for 2 frames'):
        tap.orient([f, f], [1, 2, 3])
    with pytest.raises(ValueError, match='orient: 65 frames, a call takes 64'):
        tap.orient([f] * 65, 1)
    with pytest.raises(ValueError, match='out: 1 frames for 2 frames'):
        tap.orient([f, f], 1, out=[Frame.rgb(np.zeros((4, 6, 3), np.uint8))])
    with pytest.raises(TypeError, match='out 0: a Frame expected, got ndarray'):
        tap.orient([f], 1, out=[np.zeros((4, 6, 3), np.uint8)])
    with pytest.raises(ValueError, match=r'out 0: a rgb frame of 6 x 4 \(bt601\) expected, got rgb 4 x 6'):
        tap.orient([f], 6, out=[Frame.rgb(np.zeros((4, 6, 3), np.uint8))])
    with pytest.raises(ValueError, match=r'out 0: a rgb frame of 4 x 6 \(bt601\) expected, got bgr 4 x 6'):
        tap.orient([f], 1, out=[Frame.bgr(np.zeros((4, 6, 3), np.uint8))])
    with pytest.raises(ValueError, match=r'out 0: a nv12 frame of 4 x 6 \(bt709\) expected, got nv12 4 x 6 \(bt601\)'):
        tap.orient([nv12(4, 6, 1, 'bt709')], 1, out=[nv12(4, 6, 2)])
    ro = np.zeros((4, 6, 3), np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError, match='out 0: writeable planes expected'):
        tap.orient([f], 1, out=[Frame.rgb(ro)])
    # the device layer's refusals that come before any device call: the engine is a stand-in without a library
    dev = DeviceOrient(types.SimpleNamespace(lib=None, device_id=0, _h=None))
    with pytest.raises(TypeError, match='frame 0: torch uint8 CUDA tensors expected'):
        dev.orient([f], 1)
    with pytest.raises(ValueError, match='orient: 65 frames, a call takes 64'):
        dev.orient_host([f] * 65, 1)
    with pytest.raises(ValueError, match=r'frame 0: an orientation code in 1\.\.8'):
        dev.orient_host([f], 12)
    from easy_vitpose_amd.engine import VitPoseHip
    assert callable(VitPoseHip.orient)


def test_vitinference_refuses_a_bad_angle_before_anything_is_loaded():
    from easy_vitpose_amd.inference import VitInference
    for bad in (45, 360, -90, '90', 1.5):
        with pytest.raises(ValueError, match='rotate: one of 0, 90, 180, 270 expected'):
            VitInference('/no/such/checkpoint.pth', lambda img: None, dataset='coco', rotate=bad)
    with pytest.raises(AssertionError, match='does not exist'):   # a good angle gets as far as the file
        VitInference('/no/such/checkpoint.pth', lambda img: None, dataset='coco', rotate=270)


def test_vitinference_rotate_route_against_fake_stages():
    """the frame goes up once as captured, the orient stage turns it, the letterbox stage and the pose call read the upright device frame; a callable detector
    and draw()'s image get np.rot90 of the frame"""
    from easy_vitpose_amd.inference import VitInference
    log = []

    class FakeOrient:
        def upload(self, img):
            log.append(('upload', img.shape))
            return Frame.rgb(img)

        def orient(self, frames, code):
            log.append(('orient', len(frames), code))
            return HostOrient().orient(frames, code)

    class FakePose:
        K = 17

        def infer_frames(self, frames, p9, crop='pad'):
            log.append(('pose', [type(f).__name__ for f in frames], [f.shape for f in frames], crop))
            self.frames = frames
            return np.zeros((len(p9), 17, 3), np.float32)

    seen = []

    def yolo(img):
        seen.append(img)
        return np.array([[2, 3, 9, 12, 0.9]])

    imgs = [rgb(20, 30, 1), rgb(20, 30, 2)]
    for angle, k, code in ((90, 1, 8), (270, 3, 6), (180, 2, 3)):
        m = VitInference.__new__(VitInference)
        m.yolo, m._letterbox, m._detector, m.tracker, m.frame_counter, m.yolo_step, m.crop, m._pose_nms, m._smoother, m.save_state = yolo, None, None, None, 0, 1, 'pad', None, None, True
        m._orient, m._rot_code, m._rot_k, m._vit_pose = FakeOrient(), rotate_code(angle), k, FakePose()
        log.clear(), seen.clear()
        res = m.inference_frames(imgs)
        up = [np.rot90(a, k) for a in imgs]
        assert [e[0] for e in log] == ['upload', 'upload', 'orient', 'pose'] and log[2][1:] == (2, code)
        assert log[0][1] == (20, 30, 3), 'uploaded as captured'
        assert log[3][1] == ['Frame', 'Frame'] and log[3][2] == [u.shape for u in up]
        assert all(same_bits(f.planes[0], u) for f, u in zip(m._vit_pose.frames, up)), 'the pose call reads the upright frame'
        assert len(seen) == 2 and all(same_bits(s, u) and s.flags.c_contiguous for s, u in zip(seen, up)), 'the host detector sees the same bytes'
        assert same_bits(m._img, up[-1]) and len(res) == 2 and list(res[0]) == [0]
    # rotate=0: no stage, the frames as they are
    m = VitInference.__new__(VitInference)
    m.yolo, m._letterbox, m._detector, m.tracker, m.frame_counter, m.yolo_step, m.crop, m._pose_nms, m._smoother, m.save_state = yolo, None, None, None, 0, 1, 'pad', None, None, True
    m._orient, m._rot_code, m._rot_k, m._vit_pose = None, 1, 0, FakePose()
    log.clear()
    m.inference_frames(imgs)
    assert [e[0] for e in log] == ['pose'] and log[0][1] == ['ndarray', 'ndarray'] and m._img is imgs[-1]


def test_cli_rotate_on(monkeypatch):
    from easy_vitpose_amd import cli
    base = ['--input', 'x.npy', '--synthetic', 's', '--boxes', 'b.json']
    parse = cli.build_parser().parse_args
    assert parse(base).rotate_on == 'host' and cli.rotate_arguments(parse(base)) == (0, 0)
    assert cli.rotate_arguments(parse(base + ['--rotate', '90'])) == (90, 0), 'the default is the host route, as before'
    assert cli.rotate_arguments(parse(base + ['--rotate', '270', '--rotate-on', 'host'])) == (270, 0)
    assert cli.rotate_arguments(parse(base + ['--rotate', '270', '--rotate-on', 'device'])) == (0, 270)
    with pytest.raises(SystemExit):
        parse(base + ['--rotate-on', 'gpu'])
    with pytest.raises(SystemExit):
        parse(base + ['--rotate', '45'])
    built = {}

    class FakeModel:
        dataset = 'coco'

        def __init__(self, model, yolo, *a, **kw):
            built['rotate'] = kw.get('rotate')
            self._vit_pose = types.SimpleNamespace(K=17)

        def inference_frames(self, batch):
            return [{} for _ in batch]

    import easy_vitpose_amd
    import json
    monkeypatch.setattr(easy_vitpose_amd, 'VitInference', FakeModel)
    monkeypatch.setattr(cli, '_read_frames', lambda path, rotate: (built.update(read=rotate) or [np.zeros((8, 8, 3), np.uint8)] * 2, True))
    monkeypatch.setattr(json, 'load', lambda f: [[0, 0, 4, 4, 0.9]])
    monkeypatch.setattr('builtins.open', lambda *a, **k: None)
    assert cli.main(base + ['--rotate', '90']) == 0 and built == {'read': 90, 'rotate': 0}
    assert cli.main(base + ['--rotate', '90', '--rotate-on', 'device']) == 0 and built == {'read': 0, 'rotate': 90}
    assert cli.main(base) == 0 and built == {'read': 0, 'rotate': 0}
    assert 'keeps the canvas' in cli.__doc__ and 'rotate-on' in cli.__doc__
