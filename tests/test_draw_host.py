"""CPU: the skeleton overlay contract (csrc/drawgeom.h) through the host tap vp_dbg_draw_host -- the functions the kernels of vp_draw_poses_stream run -- against
anchors that need no model, against its two restatements (easy_vitpose_amd/draw.py in numpy, tests/draw_model.py in scalar loops, a gather where the other two
paint), the order rule, the write set, the NV12 colours, the tables against the reference's (tests/golden/draw_tables.npz), every refusal of the C entries and of
the Python layer.  The device is compared with this host model in tests/test_gpu_draw.py."""
from __future__ import annotations

import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd import draw as D
from easy_vitpose_amd.cropprep import Frame, nv12_to_rgb
from easy_vitpose_amd.draw import COCO17_SKELETON, LIMB_COLORS, POINT_COLORS, DrawStyle, draw_poses_model_host, draw_poses_numpy, load_skeleton, resolve_skeleton, rgb_to_yuv
import draw_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dc.host_cases()


@functools.lru_cache(maxsize=None)
def pictures(name):
    """(tap, numpy, model, written) of a case, computed once"""
    cs = CASES[name]
    model, written = dc.run_model(cs)
    return dc.run_tap(cs), dc.run_numpy(cs), model, written


def test_surface_symbols_macros_and_abi_version():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    for name in ('vp_draw_poses_stream', 'vp_draw_poses', 'vp_dbg_draw_host'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r'VP_API\s+int\s+' + name + r'\s*\(', hdr), name
    assert re.search(r'#define\s+VP_HAS_DRAW\s+1\b', hdr)
    assert re.search(r'#define\s+VP_DRAW_MAX_LIMBS\s+256\b', hdr) and D.DRAW_MAX_LIMBS == 256
    assert re.search(r'#define\s+VP_DRAW_MAX_COLORS\s+32\b', hdr) and D.DRAW_MAX_COLORS == 32
    assert re.search(r'#define\s+VP_DRAW_MAX_RECORDS\s+65536\b', hdr) and D.DRAW_MAX_RECORDS == 65536
    assert re.search(r'#define\s+VP_ABI_VERSION\s+4\b', hdr) and lib.vp_abi_version() == 4
    assert C.sizeof(capi.vp_draw_cfg) == 56   # a float, 3 int32, then three (int32, pointer) pairs at 8-byte alignment


# ---- anchors that need no model
def on_black(kp, style, boxes=None, hw=(48, 64)):
    """the set of (x, y) the tap touches on a black RGB frame, and the frame"""
    img = np.zeros(hw + (3,), np.uint8)
    kp = np.asarray(kp, np.float32)[None]
    draw_poses_model_host([img], kp, np.zeros(1, np.int32), style, boxes=None if boxes is None else np.asarray(boxes, np.float32)[None])
    ys, xs = np.nonzero(img.any(-1))
    return set(zip(xs.tolist(), ys.tolist())), img


WHITE = dict(point_colors=[(255, 255, 255)], limb_colors=[(200, 200, 200)])


def test_anchor_limb_of_65_pixels():
    got, _ = on_black([(20, 10, 1), (20, 30, 1)], DrawStyle(skeleton=[(0, 1)], thickness=2, radius=1, **WHITE))
    want = {(x, y) for y in (19, 20, 21) for x in range(10, 31)} | {(9, 20), (31, 20)}
    assert len(want) == 65 and got == want   # (the r = 1 disks of its two joints lie inside it)


def test_anchor_radius_one_is_the_five_pixel_plus():
    got, img = on_black([(7, 9, 1)], DrawStyle(skeleton=(), radius=1, **WHITE))
    assert got == {(9, 7), (8, 7), (10, 7), (9, 6), (9, 8)}
    got0, _ = on_black([(7, 9, 1)], DrawStyle(skeleton=(), radius=0, **WHITE))   # radius 0 on a 48 x 64 frame: max(1, 48 // 150) = 1
    assert got0 == got


def test_anchor_degenerate_limb_leaves_the_caps():
    got, _ = on_black([(20, 30, 1), (20.9, 30.9, 1)], DrawStyle(skeleton=[(0, 1)], thickness=4, radius=1, **WHITE))   # both joints on pixel (30, 20)
    assert got == {(30 + dx, 20 + dy) for dx in range(-2, 3) for dy in range(-2, 3) if dx * dx + dy * dy <= 4} and len(got) == 13


def test_anchor_rectangle_outline():
    hidden = [(5, 5, 0.0)]
    got, _ = on_black(hidden, DrawStyle(skeleton=(), thickness=1, **WHITE), boxes=(10, 5, 20, 12))
    assert got == {(x, y) for x in range(10, 21) for y in range(5, 13) if x in (10, 20) or y in (5, 12)} and len(got) == 34
    got, _ = on_black(hidden, DrawStyle(skeleton=(), thickness=2, **WHITE), boxes=(10.9, 5.2, 20.5, 12.99))
    assert got == {(x, y) for x in range(9, 22) for y in range(4, 14) if not (11 <= x <= 19 and 6 <= y <= 11)} and len(got) == 13 * 10 - 9 * 6
    got, _ = on_black(hidden, DrawStyle(skeleton=(), thickness=3, **WHITE), boxes=(20, 12, 10, 5))   # corners in any order; o = 1: columns 9, 10, 11 ...
    assert got == {(x, y) for x in range(9, 22) for y in range(4, 14) if not (12 <= x <= 18 and 7 <= y <= 10)}


# ---- the three statements
@pytest.mark.parametrize('name', sorted(CASES))
def test_tap_numpy_and_scalar_model_agree_bit_for_bit(name):
    tap, twin, model, _ = pictures(name)
    assert dc.same(tap, twin), 'vp_dbg_draw_host != draw_poses_numpy'
    assert dc.same(tap, model), 'vp_dbg_draw_host != tests/draw_model.py'
    _, before = dc.build_frames(CASES[name]['specs'], CASES[name]['seed'])
    assert not dc.same(tap, before), 'the case draws nothing'


@pytest.mark.parametrize('name', sorted(CASES))
def test_write_set_every_other_byte_is_unchanged(name):
    """outside the union of covered pixels and chroma samples, as the scalar model gives it, no byte changes: pitch padding and rows of other frames included"""
    tap, _, _, written = pictures(name)
    cs = CASES[name]
    _, before = dc.build_frames(cs['specs'], cs['seed'])
    b = 0
    for (h, w, fmt, matrix, pad), wr in zip(cs['specs'], written):
        planes = 2 if fmt == 'nv12' else 1
        for p in range(planes):
            may = np.zeros(before[b + p].shape, bool)
            rc = np.array([(r, c) for q, r, c in wr if q == p], dtype=np.int64).reshape(-1, 2)
            may[rc[:, 0], rc[:, 1]] = True
            assert np.array_equal(tap[b + p][~may], before[b + p][~may]), f'{name}: plane {p} changed outside the write set'
        b += planes


def test_no_row_frame_is_untouched_and_padding_survives():
    tap = pictures('no_row_frame')[0]
    _, before = dc.build_frames(CASES['no_row_frame']['specs'], CASES['no_row_frame']['seed'])
    assert np.array_equal(tap[1], before[1]) and np.array_equal(tap[2], before[2])   # frame 1 (NV12): no row names it
    assert not np.array_equal(tap[3], before[3])                                    # frame 2 has one
    for name in ('rgb_pitched', 'nv12_pitched'):
        cs = CASES[name]
        _, before = dc.build_frames(cs['specs'], cs['seed'])
        w_bytes = [3 * 131] if name == 'rgb_pitched' else [131, 2 * 66]
        for got, was, wb in zip(pictures(name)[0], before, w_bytes):
            assert np.array_equal(got[:, wb:], was[:, wb:]) and not np.array_equal(got[:, :wb], was[:, :wb])


def test_rows_of_two_frames_interleaved_equal_each_frame_drawn_alone():
    cs = CASES['two_frames']
    both = pictures('two_frames')[0]
    ids = np.arange(len(cs['kp']), dtype=np.int32)   # the colour of a row is its index in the combined call
    for f, planes in ((0, [0]), (1, [1, 2])):
        alone = dict(cs, fi=np.where(cs['fi'] == f, cs['fi'], -1).astype(np.int32), ids=ids)
        got = dc.run_tap(alone)
        _, before = dc.build_frames(cs['specs'], cs['seed'])
        for p in range(3):
            assert np.array_equal(got[p], both[p] if p in planes else before[p])


def test_gates_of_the_edge_rows():
    """what the edge rows must and must not leave, read off the picture: conf == thr and NaN invisible, the next float above visible; +-16383.x usable (a limb from
    there reaches the frame), +-16384 not"""
    kp = CASES['edges_rgb']['kp']
    one = np.zeros(1, np.int32)
    img = np.zeros((97, 131, 3), np.uint8)
    draw_poses_model_host([img], kp[:1], one, DrawStyle(skeleton=()))
    for j, vis in ((0, False), (1, True), (2, False), (3, False), (4, True), (5, False), (6, True)):   # conf 0.5, next above, next below, NaN, +inf, -inf, 0.9
        y, x = int(kp[0, j, 0]), int(kp[0, j, 1])
        assert tuple(img[y, x]) == (POINT_COLORS[j % 10] if vis else (0, 0, 0)), j
    # row 2: joints 0 (x = 16383.5) and 1 (x = -16383.9) are visible and far off the frame; the limb between them crosses it along y = 40
    img = np.zeros((97, 131, 3), np.uint8)
    draw_poses_model_host([img], kp[2:3], one, DrawStyle(skeleton=[(0, 1)], limb_colors=[(1, 2, 3)]))
    assert (img[39:42] == (1, 2, 3)).all() and not (img[:39] == (1, 2, 3)).all(-1).any() and not (img[42:] == (1, 2, 3)).all(-1).any()
    img = np.zeros((97, 131, 3), np.uint8)
    draw_poses_model_host([img], kp[2:3], one, DrawStyle(skeleton=[(2, 3), (0, 2), (1, 3)], limb_colors=[(1, 2, 3)]))   # joints 2 and 3 sit at +-16384: no limb
    assert not (img == (1, 2, 3)).all(-1).any()
    # row 3: truncation toward zero puts (-0.9, -0.9) on pixel (0, 0) and (96.99, 130.99) on the last pixel
    img = np.zeros((97, 131, 3), np.uint8)
    draw_poses_model_host([img], kp[3:4], one, DrawStyle(skeleton=()))
    assert tuple(img[0, 0]) == POINT_COLORS[0] and tuple(img[96, 130]) == POINT_COLORS[1]


# ---- order
def order_case():
    K = 6
    A, B = np.zeros((K, 3), np.float32), np.zeros((K, 3), np.float32)
    for kp, pts in ((A, {0: (30, 40), 1: (70, 40), 2: (50, 50), 3: (60, 30), 4: (35, 55)}), (B, {0: (60, 10), 1: (60, 70), 2: (40, 40), 3: (20, 50), 5: (35, 55)})):
        for j, (x, y) in pts.items():
            kp[j] = (y, x, 1.0)
    boxes = np.array([[20, 20, 80, 60], [50, 20, 90, 60]], np.float32)
    return np.stack([A, B]), boxes


def test_order_the_later_row_lies_over_the_earlier_one_for_every_pair_of_primitive_types():
    kp, boxes = order_case()
    ids = np.array([0, 5], np.int32)
    la, lb = LIMB_COLORS[0], LIMB_COLORS[5]
    P = POINT_COLORS
    # (x, y): colour with B later, colour with A later
    probes = {(50, 20): (lb, la),      # box over box
              (50, 40): (lb, la),      # B's box over A's limb | A's limb over B's box
              (50, 50): (lb, P[2]),    # B's box over A's joint 2 | A's joint over B's box
              (60, 20): (lb, la),      # B's limb over A's box
              (60, 40): (lb, la),      # limb over limb
              (60, 30): (lb, P[3]),    # B's limb over A's joint 3
              (40, 40): (P[2], la),    # B's joint 2 over A's limb
              (20, 50): (P[3], la),    # B's joint 3 over A's box
              (35, 55): (P[5], P[4]),  # joint over joint
              (30, 40): (P[0], P[0]),  # A's joint 0 over its own limb, in either order
              (60, 10): (P[0], P[0])}  # B's joint 0 over its own limb
    style = DrawStyle(skeleton=[(0, 1)])
    for which, order in ((0, [0, 1]), (1, [1, 0])):
        img = np.zeros((97, 131, 3), np.uint8)
        draw_poses_model_host([img], kp[order], np.zeros(2, np.int32), style, ids=ids[order], boxes=boxes[order])
        twin = np.zeros((97, 131, 3), np.uint8)
        draw_poses_numpy([twin], kp[order], np.zeros(2, np.int32), style, ids=ids[order], boxes=boxes[order])
        assert np.array_equal(img, twin)
        for (x, y), want in probes.items():
            assert tuple(img[y, x]) == want[which], ((x, y), which)


# ---- NV12 colours
def fp64_forward(matrix):
    """(offsets, 3 x 3) of RGB -> YUV from the standards' definitions"""
    kr, kb = (0.2126, 0.0722) if matrix == 'bt709' else (0.299, 0.114)
    ys, cs, yoff = (1.0, 1.0, 0.0) if matrix == 'bt601_full' else (219.0 / 255.0, 224.0 / 255.0, 16.0)
    kg = 1.0 - kr - kb
    m = np.array([[kr * ys, kg * ys, kb * ys],
                  [-kr / (2 * (1 - kb)) * cs, -kg / (2 * (1 - kb)) * cs, 0.5 * cs],
                  [0.5 * cs, -kg / (2 * (1 - kr)) * cs, -kb / (2 * (1 - kr)) * cs]])
    return np.array([yoff, 128.0, 128.0]), m


def back(yuv, matrix):
    yuv = np.asarray(yuv, np.uint8).reshape(-1, 3)
    return np.stack([nv12_to_rgb(p[:1].reshape(1, 1), p[1:].reshape(1, 1, 2), matrix)[0, 0] for p in yuv]).astype(np.int64)


def test_nv12_colours_round_trip_within_the_quantisation_bound():
    """Every palette colour through drawgeom.h's integer forward matrix and back through pixfmt.h's yuv_to_rgb.  The bound is measured here on the reference path --
    the fp64 forward matrix, rounded to 8 bits, then the same yuv_to_rgb -- plus one code for the 8-bit matrix coefficients: 8-bit quantisation twice.
    Measured: the fp64 path's worst channel error over the 18 palette colours and the three matrices is 1 code, so the bound is 2 codes; the integer path's own
    worst is 2."""
    colours = np.array(LIMB_COLORS + POINT_COLORS, np.int64)
    worst_ref = worst = 0
    for matrix in ('bt601', 'bt709', 'bt601_full'):
        off, m = fp64_forward(matrix)
        assert np.array_equal(np.rint(m * 256).astype(int), np.array(D.RGB_YUV_COEFS[matrix][1:])), matrix   # the table IS round(x 2^8) of the standard matrix
        assert D.RGB_YUV_COEFS[matrix][0] == off[0]
        ref = np.clip(np.rint(colours @ m.T + off), 0, 255)
        worst_ref = max(worst_ref, int(np.abs(back(ref, matrix) - colours).max()))
        worst = max(worst, int(np.abs(back(rgb_to_yuv(colours, matrix), matrix) - colours).max()))
    print(f'fp64 forward + yuv_to_rgb: worst {worst_ref} codes; integer forward + yuv_to_rgb: worst {worst} codes')
    assert worst <= worst_ref + 1


def test_rgb_to_yuv_twin_equals_the_header_on_every_palette_colour():
    """a disk per colour on an NV12 frame, Y, U, V read back"""
    for matrix in ('bt601', 'bt709', 'bt601_full'):
        for rgb in LIMB_COLORS + POINT_COLORS + ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)):
            y, uv = np.full((4, 4), 7, np.uint8), np.full((2, 2, 2), 9, np.uint8)
            draw_poses_model_host([Frame.nv12(y, uv, matrix)], np.array([[[2, 2, 1]]], np.float32), np.zeros(1, np.int32), DrawStyle(skeleton=(), radius=1, point_colors=[rgb]))
            assert (int(y[2, 2]), int(uv[1, 1, 0]), int(uv[1, 1, 1])) == tuple(int(v) for v in rgb_to_yuv(np.array(rgb), matrix)), (matrix, rgb)


# ---- tables
def test_tables_equal_the_reference_fixture():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'draw_tables.npz'))
    assert np.array_equal(np.array(COCO17_SKELETON), g['coco'])
    assert np.array_equal(np.array(LIMB_COLORS), g['limb_colors']) and np.array_equal(np.array(POINT_COLORS), g['point_colors'])
    assert np.array_equal(resolve_skeleton('coco', 17), g['coco'])
    with pytest.raises(ValueError, match='needs its own'):
        resolve_skeleton('wholebody', 133)
    with pytest.raises(ValueError, match='needs its own'):
        resolve_skeleton('coco', 25)
    assert np.array_equal(resolve_skeleton('wholebody', 133, g['wholebody']), g['wholebody'])
    assert np.array_equal(resolve_skeleton('wholebody', 133, g['wholebody'].tolist()), g['wholebody'])
    with pytest.raises(ValueError, match='names joint'):
        resolve_skeleton('coco', 17, g['wholebody'])


def test_load_skeleton(tmp_path):
    p = tmp_path / 's.json'
    p.write_text(json.dumps([[0, 1], [1, 2]]))
    assert load_skeleton(str(p)) == ((0, 1), (1, 2))
    for bad in ([[0, 1, 2]], [0, 1], {'a': 1}, [[0, 1.5]], [[0, 256]], [[True, 1]]):
        p.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            load_skeleton(str(p))


# ---- refusals
def tap_call(images=True, n_images=1, kpts=True, n=2, k=17, fidx=True, frame_stride=1, boxes=False, box_stride=4, cfg=True, image=None, **over):
    """one vp_dbg_draw_host call with one argument made bad: (status, message)"""
    lib = capi.load_library()
    img = np.zeros((16, 16, 3), np.uint8)
    y, uv = np.zeros((16, 16), np.uint8), np.zeros((8, 8, 2), np.uint8)
    fields = dict(plane=(img.ctypes.data, None), pitch=(48, 0), h=16, w=16, format=0, matrix=0)
    if image:
        if image.get('format') == 2:
            fields.update(plane=(y.ctypes.data, uv.ctypes.data), pitch=(16, 16))
        fields.update(image)
    table = (capi.vp_image * 1)(capi.vp_image((C.c_void_p * 2)(*fields['plane']), (C.c_int64 * 2)(*fields['pitch']), fields['h'], fields['w'], fields['format'], fields['matrix']))
    kp = np.zeros((max(n, 1), max(k, 1), 3), np.float32)
    fi = np.zeros(max(n, 1) * max(frame_stride, 1), np.int32)
    bx = np.zeros((max(n, 1), 4), np.float32)
    limbs = np.array(over.pop('limbs', COCO17_SKELETON), np.uint8).reshape(-1, 2)
    pc, lc = np.array(POINT_COLORS, np.uint8), np.array(LIMB_COLORS, np.uint8)
    c = dict(conf_thr=0.5, radius=0, thickness=2, n_limbs=len(limbs), limbs=limbs.ctypes.data, n_point_colors=10, point_colors=pc.ctypes.data, n_limb_colors=8,
             limb_colors=lc.ctypes.data)
    if over.pop('null_limbs', False):
        c['limbs'] = None
    c.update(over)
    cfg_s = capi.vp_draw_cfg(*(c[f] for f, _ in capi.vp_draw_cfg._fields_))
    rc = lib.vp_dbg_draw_host(table if images else None, n_images, kp.ctypes.data if kpts else None, n, k, fi.ctypes.data if fidx else None, frame_stride, None, None,
                              bx.ctypes.data if boxes else None, box_stride, C.byref(cfg_s) if cfg else None)
    return rc, capi.last_error(None)


REFUSALS = {
    'null cfg': dict(cfg=False),
    'negative n': dict(n=-1),
    'null images': dict(images=False),
    'null keypoints': dict(kpts=False),
    'null frame index': dict(fidx=False),
    'no frames': dict(n_images=0),
    'k = 0': dict(k=0, limbs=[]),
    'k = 257': dict(k=257),
    'n_limbs above the limit': dict(n_limbs=257),
    'negative n_limbs': dict(n_limbs=-1),
    'limb index >= k': dict(k=16),
    'null limb table': dict(null_limbs=True),
    'no point colours': dict(n_point_colors=0),
    '33 point colours': dict(n_point_colors=33),
    'no limb colours': dict(n_limb_colors=0),
    '33 limb colours': dict(n_limb_colors=33),
    'null colours': dict(point_colors=None),
    'conf_thr NaN': dict(conf_thr=float('nan')),
    'conf_thr inf': dict(conf_thr=float('inf')),
    'radius -1': dict(radius=-1),
    'radius 65': dict(radius=65),
    'thickness 0': dict(thickness=0),
    'thickness 17': dict(thickness=17),
    'frame stride 0': dict(frame_stride=0),
    'box stride 0': dict(boxes=True, box_stride=0),
    'too many records': dict(n=65536 // 36 + 1),
    'h above 8192': dict(image=dict(h=8193)),
    'w above 8192': dict(image=dict(w=8193, pitch=(3 * 8193, 0))),
    'no data': dict(image=dict(plane=(None, None))),
    'h = 0': dict(image=dict(h=0)),
    'unknown format': dict(image=dict(format=3)),
    'unknown matrix': dict(image=dict(format=2, matrix=3)),
    'negative pitch': dict(image=dict(pitch=(-48, 0))),
    'pitch below the row': dict(image=dict(pitch=(47, 0))),
    'NV12 without UV': dict(image=dict(format=2, plane=(1, None))),
    'UV pitch below the row': dict(image=dict(format=2, pitch=(16, 15))),
}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_of_the_c_entry(what):
    rc, msg = tap_call(**REFUSALS[what])
    assert rc == capi.VP_ERR_INVALID and msg.startswith('draw: '), (what, rc, msg)


def test_accepted_calls_of_the_c_entry():
    assert tap_call()[0] == capi.VP_OK
    assert tap_call(n=0, images=False, kpts=False, fidx=False, n_images=0)[0] == capi.VP_OK     # n = 0: nothing needed
    assert tap_call(n=65536 // 36)[0] == capi.VP_OK                                               # exactly the workspace limit
    assert tap_call(n_limbs=0, limbs=[])[0] == capi.VP_OK
    assert tap_call(radius=64, thickness=16, boxes=True)[0] == capi.VP_OK
    assert tap_call(image=dict(format=2, matrix=2))[0] == capi.VP_OK


def test_refusals_of_the_python_layer():
    for kw in (dict(conf_thr=float('nan')), dict(conf_thr='x'), dict(radius=-1), dict(radius=65), dict(radius=1.5), dict(thickness=0), dict(thickness=17),
               dict(skeleton=[(0, 256)]), dict(skeleton=[(0, 1, 2)]), dict(skeleton=[(0, 1)] * 257), dict(skeleton=5), dict(point_colors=[]), dict(point_colors=[(0, 0, 256)]),
               dict(limb_colors=[(1, 2)]), dict(limb_colors=[(0, 0, 0)] * 33), dict(thickness=True)):
        with pytest.raises(ValueError):
            DrawStyle(**kw)
    img = np.zeros((16, 16, 3), np.uint8)
    kp = np.zeros((2, 17, 3), np.float32)
    for fn in (draw_poses_numpy, draw_poses_model_host):
        with pytest.raises(ValueError, match='needs its own'):
            fn([img], np.zeros((2, 133, 3), np.float32), np.zeros(2, np.int32))
        with pytest.raises(ValueError, match='names joint'):
            fn([img], kp, np.zeros(2, np.int32), DrawStyle(skeleton=[(0, 17)]))
        with pytest.raises(ValueError):
            fn([img], kp[0], np.zeros(2, np.int32))
        with pytest.raises(ValueError):
            fn([img], kp, np.zeros(3, np.int32))
        with pytest.raises(ValueError):
            fn([img], kp, np.zeros(2, np.int32), boxes=np.zeros((2, 3)))
        with pytest.raises(TypeError):
            fn([img], kp, np.zeros(2, np.int32), style=dict(thickness=2))
        with pytest.raises((TypeError, ValueError)):
            fn([img.astype(np.float32)], kp, np.zeros(2, np.int32))
    with pytest.raises(ValueError, match='records'):
        draw_poses_numpy([img], np.zeros((65536 // 36 + 1, 17, 3), np.float32), np.zeros(65536 // 36 + 1, np.int32))


def test_vitinference_draw_before_inference_and_the_cli_surface():
    from easy_vitpose_amd import cli
    from easy_vitpose_amd.inference import VitInference
    import inspect
    m = VitInference.__new__(VitInference)   # no device: draw() must say what is missing before it touches the engine
    m._img = m._keypoints = None
    with pytest.raises(RuntimeError, match='call inference'):
        m.draw()
    assert inspect.signature(VitInference.__init__).parameters['skeleton'].default is None
    assert list(inspect.signature(VitInference.draw).parameters)[1:] == ['show_yolo', 'show_raw_yolo', 'confidence_threshold']
    args = cli.build_parser().parse_args(['--input', 'x.png', '--synthetic', 's', '--boxes', 'b.json', '--output-path', 'o', '--save-img', '--skeleton', 's.json'])
    assert args.save_img and args.skeleton == 's.json'
    with pytest.raises(AssertionError, match='preview'):
        cli.main(['--input', 'x.png', '--synthetic', 's', '--boxes', 'b.json', '--show'])
    with pytest.raises(AssertionError, match='output path'):
        cli.main(['--input', 'x.png', '--synthetic', 's', '--boxes', 'b.json', '--save-img'])
    with pytest.raises(AssertionError, match='--save-img'):
        cli.main(['--input', 'x.png', '--synthetic', 's', '--boxes', 'b.json', '--skeleton', 's.json'])
