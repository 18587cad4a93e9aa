"""CPU: the label stage contract (csrc/labelgeom.h) through the host taps vp_dbg_draw_labels_host, vp_dbg_label_text and vp_dbg_label_glyph -- the functions the
kernels of vp_draw_labels_stream run -- against Python's own number formatter, anchors that need no model, its two restatements (easy_vitpose_amd/draw.py in
numpy, tests/label_model.py in scalar loops, a gather where the other two paint), the write set, every refusal of the C entries and of the Python layer, and the
layering under the skeleton overlay.  The device is compared with this host model in tests/test_gpu_label.py."""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd import draw as D
from easy_vitpose_amd.draw import (LABEL_ALPHABET, LABEL_GLYPHS, LIMB_COLORS, DrawStyle, LabelStyle, draw_labels_model_host, draw_labels_numpy, draw_poses_model_host,
                                   draw_poses_numpy, label_text)
import draw_cases as dc
import label_cases as lc
from label_model import FONT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = lc.host_cases()


@functools.lru_cache(maxsize=None)
def pictures(name):
    """(tap, numpy, model, written) of a case, computed once"""
    cs = CASES[name]
    model, written = lc.run_model(cs)
    return lc.run_tap(cs), lc.run_numpy(cs), model, written


def test_surface_symbols_macros_and_abi_version():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    for name in ('vp_draw_labels_stream', 'vp_draw_labels', 'vp_dbg_draw_labels_host', 'vp_dbg_label_text', 'vp_dbg_label_glyph'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r'VP_API\s+\w+\s+' + name + r'\s*\(', hdr), name
    assert re.search(r'#define\s+VP_HAS_DRAW_LABELS\s+1\b', hdr)
    assert re.search(r'#define\s+VP_LABEL_MAX_ROWS\s+8192\b', hdr) and D.LABEL_MAX_ROWS == 8192
    assert re.search(r'#define\s+VP_ABI_VERSION\s+4\b', hdr) and lib.vp_abi_version() == 4
    assert C.sizeof(capi.vp_label_cfg) == 32   # two int32, a pointer, an int32, three bytes and one of padding, an int32, four bytes of padding
    build = __import__('easy_vitpose_amd.build', fromlist=['SOURCES'])
    assert 'label.hip' in build.SOURCES and 'label.hip' not in build.SOURCE_FLAGS and 'labelgeom.h' in build.HEADERS


# ---- text
def tap_text(id_, score=None):
    buf = C.create_string_buffer(25)
    assert capi.load_library().vp_dbg_label_text(int(id_), 0 if score is None else 1, C.c_float(0.0 if score is None else score), buf) == capi.VP_OK
    return buf.value.decode()


def check_scores(values, id_=7):
    """tap, Python twin and Python's formatter on every float32 of `values` (all inside (-1000, 1000)); returns the count"""
    values = np.asarray(values, np.float32)
    lib = capi.load_library()
    buf = C.create_string_buffer(25)
    bad = []
    for v in values:
        want = f'#{id_}: {float(v):.2f}'
        lib.vp_dbg_label_text(id_, 1, C.c_float(v), buf)
        if buf.value.decode() != want or label_text(id_, v) != want:
            bad.append((float(v), buf.value.decode(), label_text(id_, v), want))
    assert not bad, bad[:5]
    return len(values)


def test_score_text_equals_pythons_formatter_on_seeded_samples():
    rng = np.random.default_rng(1)
    unit = rng.random(100000, dtype=np.float32)
    wide = rng.uniform(-1000, 1000, 100000).astype(np.float32)
    wide = wide[np.abs(wide) < 1000]
    assert len(wide) > 99900
    assert check_scores(unit) + check_scores(wide) > 199900


def test_score_text_on_every_eighth():
    """k / 8 is exact in float32: the .125 / .375 / .625 / .875 ties go to the even hundredth"""
    assert check_scores(np.arange(-7999, 8000, dtype=np.float64) / 8) == 15999
    assert tap_text(7, 0.125) == '#7: 0.12' and tap_text(7, 0.375) == '#7: 0.38' and tap_text(7, -0.625) == '#7: -0.62' and tap_text(7, 2.875) == '#7: 2.88'


def test_score_text_beside_every_sampled_decimal_tie():
    """the float32 nearest (k + 0.5) / 100 and both its neighbours: where a double-rounding or a float multiply would go wrong"""
    k = np.arange(0, 100000, 7, dtype=np.float64)
    mid = ((k + 0.5) / 100).astype(np.float32)
    vals = np.concatenate([mid, np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))])
    vals = vals[np.abs(vals) < 1000]
    assert check_scores(vals) >= 3 * len(k) - 3
    assert check_scores(-vals) >= 3 * len(k) - 3


def test_score_text_special_values_and_ids():
    f32 = np.float32
    below = np.nextafter(f32(1000), f32(0))
    assert tap_text(1, below) == label_text(1, below) == '#1: 1000.00' == f'#1: {float(below):.2f}'
    assert tap_text(1, -below) == label_text(1, -below) == '#1: -1000.00'
    assert tap_text(1, 0.0) == label_text(1, 0.0) == '#1: 0.00'
    assert tap_text(1, -0.0) == label_text(1, -0.0) == '#1: -0.00' == f'#1: {-0.0:.2f}'
    tiny = np.array([1, 0x7fffff, 0x800000], np.uint32).view(np.float32)   # the smallest and the largest denormal, the smallest normal
    for v in tiny:
        assert tap_text(1, v) == label_text(1, v) == '#1: 0.00' and tap_text(1, -v) == label_text(1, -v) == '#1: -0.00' == f'#1: {float(-v):.2f}'
    assert check_scores([0.005, 0.015, 0.004999999, 0.0050000004, 1e-30, 999.99, 999.995, 0.994999, 0.995]) == 9
    for v in (1000.0, -1000.0, float('nan'), float('inf'), float('-inf'), 1e30):   # outside (-1000, 1000): the id alone
        assert tap_text(3, v) == label_text(3, v) == '#3', v
    for i in (0, 7, -1, 2 ** 31 - 1, -2 ** 31):
        assert tap_text(i) == label_text(i) == f'#{i}'
        assert tap_text(i, 0.5) == label_text(i, 0.5) == f'#{i}: 0.50'
    assert len(tap_text(-2 ** 31, -below)) == 22 == D.LABEL_MAX_TEXT
    with pytest.raises(ValueError):
        label_text(2 ** 31)


# ---- glyphs
def test_glyph_words_of_the_header_equal_the_python_table_and_the_pictures():
    lib = capi.load_library()
    assert len(LABEL_GLYPHS) == 16 and len(LABEL_ALPHABET) == 16 and LABEL_ALPHABET[:11] == '#0123456789'
    for code, ch in enumerate(LABEL_ALPHABET):
        word = lib.vp_dbg_label_glyph(code)
        assert word == LABEL_GLYPHS[code], (code, hex(word))
        pic = sum(1 << (5 * r + c) for r in range(7) for c in range(5) if FONT[ch][r][c] == '#')
        assert word == pic and word < 1 << 35, ch
    assert lib.vp_dbg_label_glyph(-1) == 0 and lib.vp_dbg_label_glyph(16) == 0
    assert len(set(LABEL_GLYPHS)) == 16


# ---- anchors that need no model
def on_black(box, style, hw=(48, 64), **kw):
    img = np.zeros(hw + (3,), np.uint8)
    draw_labels_model_host([img], np.asarray(box, np.float32)[None], np.zeros(1, np.int32), style, **kw)
    return img


def pixel_set(mask):
    ys, xs = np.nonzero(mask)
    return set(zip(xs.tolist(), ys.tolist()))


def test_anchor_block_of_hash_7_is_13_by_9_and_the_ink_of_the_7_is_a_literal():
    img = on_black((20, 30, 50, 44), LabelStyle(scale=1, colors=[(200, 10, 10)], ink=(1, 2, 3)), ids=np.array([7], np.int32))
    assert pixel_set(img.any(-1)) == {(x, y) for x in range(20, 33) for y in range(21, 30)}   # 13 x 9, its last row just above y1 = 30
    ink = pixel_set((img == (1, 2, 3)).all(-1))
    seven = {(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 1), (3, 2), (2, 3), (1, 4), (1, 5), (1, 6)}   # the glyph '7', (col, row)
    hash_ = {(1, r) for r in range(7)} | {(3, r) for r in range(7)} | {(c, 2) for c in range(5)} | {(c, 4) for c in range(5)}
    assert ink == {(21 + c, 22 + r) for c, r in hash_} | {(27 + c, 22 + r) for c, r in seven}
    assert ((img == (200, 10, 10)).all(-1) | (img == (1, 2, 3)).all(-1) | ~img.any(-1)).all()


def test_anchor_scale_three_turns_every_bit_into_a_3_by_3_square():
    one = on_black((2, 30, 50, 44), LabelStyle(scale=1, colors=[(9, 9, 9)], ink=(255, 255, 255)), ids=np.array([-4], np.int32))
    three = on_black((2, 40, 50, 44), LabelStyle(scale=3, colors=[(9, 9, 9)], ink=(255, 255, 255)), ids=np.array([-4], np.int32), hw=(60, 90))
    assert np.array_equal(np.kron(one[21:30, 2:21], np.ones((3, 3, 1), np.uint8)), three[13:40, 2:59])   # '#-4': 19 x 9 bits
    assert not three[:13].any() and not three[40:].any() and not three[:, 59:].any() and not three[:, :2].any()


def test_anchor_scale_zero_follows_the_frame():
    for hw, s in (((48, 64), 1), ((799, 900), 1), ((800, 810), 2), ((1300, 1250), 3)):
        img = on_black((5, hw[0] - 1, 50, hw[0]), LabelStyle(scale=0, colors=[(9, 9, 9)]), hw=hw, ids=np.array([1], np.int32))
        ys, xs = np.nonzero(img.any(-1))
        assert (xs.min(), xs.max() + 1, ys.max() + 1 - ys.min()) == (5, 5 + 13 * s, 9 * s), (hw, s)
        twin = np.zeros(hw + (3,), np.uint8)
        draw_labels_numpy([twin], np.array([[5, hw[0] - 1, 50, hw[0]]], np.float32), np.zeros(1, np.int32), LabelStyle(scale=0, colors=[(9, 9, 9)]), ids=np.array([1], np.int32))
        assert np.array_equal(img, twin)


def test_anchor_above_or_inside_rule():
    st = LabelStyle(scale=2, colors=[(9, 9, 9)])
    for y1, rows in ((17, (17, 35)), (18, (0, 18)), (19, (1, 19))):
        ys, _ = np.nonzero(on_black((4, y1, 40, 45), st).any(-1))
        assert (ys.min(), ys.max() + 1) == rows, y1


def test_anchor_auto_ink_is_black_on_light_and_white_on_dark():
    for k, want in enumerate(((0, 0, 0), (255, 255, 255), (0, 0, 0), (255, 255, 255))):
        img = on_black((4, 20, 40, 45), LabelStyle(scale=1, colors=lc.LIGHT_DARK), ids=np.array([k], np.int32))
        assert tuple(img[11, 4]) == lc.LIGHT_DARK[k] and tuple(img[12, 6]) == want, k   # the block's corner; a bit of '#'


# ---- the three statements
@pytest.mark.parametrize('name', sorted(CASES))
def test_tap_numpy_and_scalar_model_agree_bit_for_bit(name):
    tap, twin, model, _ = pictures(name)
    assert lc.same(tap, twin), 'vp_dbg_draw_labels_host != draw_labels_numpy'
    assert lc.same(tap, model), 'vp_dbg_draw_labels_host != tests/label_model.py'
    _, before = lc.build_frames(CASES[name]['specs'], CASES[name]['seed'])
    assert not lc.same(tap, before), 'the case writes nothing'


@pytest.mark.parametrize('name', sorted(CASES))
def test_write_set_every_other_byte_is_unchanged(name):
    """outside the union of covered pixels and chroma samples, as the scalar model gives it, no byte changes: pitch padding and rows of other frames included"""
    tap, _, _, written = pictures(name)
    cs = CASES[name]
    _, before = lc.build_frames(cs['specs'], cs['seed'])
    b = 0
    for (h, w, fmt, matrix, pad), wr in zip(cs['specs'], written):
        planes = 2 if fmt == 'nv12' else 1
        for p in range(planes):
            may = np.zeros(before[b + p].shape, bool)
            rc = np.array([(r, c) for q, r, c in wr if q == p], dtype=np.int64).reshape(-1, 2)
            may[rc[:, 0], rc[:, 1]] = True
            assert np.array_equal(tap[b + p][~may], before[b + p][~may]), f'{name}: plane {p} changed outside the write set'
        b += planes


@pytest.mark.parametrize('fmt', ['rgb', 'nv12'])
def test_crowd_of_600_overlapping_tags(fmt):
    cs = lc.crowd_case(fmt)
    tap = lc.run_tap(cs)
    assert lc.same(tap, lc.run_numpy(cs)) and lc.same(tap, lc.run_model(cs)[0])


def test_gates_leave_exactly_the_rows_that_pass():
    """rows 0, 6 and 7 of the `gates` case pass; the masked, absent, NaN and +-16384 rows leave nothing: the picture equals the one of those three rows alone"""
    cs = CASES['gates']
    keep = [0, 6, 7]
    alone = dict(cs, boxes=cs['boxes'][keep], fi=cs['fi'][keep], rank=cs['rank'][keep], ids=cs['ids'][keep], scores=cs['scores'][keep])
    assert lc.same(pictures('gates')[0], lc.run_tap(alone))
    none = dict(cs, rank=np.where(np.isin(np.arange(9), keep), -1, cs['rank']).astype(np.int32))
    _, before = lc.build_frames(cs['specs'], cs['seed'])
    assert lc.same(lc.run_tap(none), before)


def test_scores_absent_show_score_off_and_unprintable_scores_print_the_id_alone():
    assert lc.same(pictures('no_scores')[0], pictures('show_score_off')[0])
    cs = CASES['odd_scores']
    for row, text in enumerate(('#0', '#7: -0.00', '#-1', '#2147483647: 1000.00', '#-2147483648: -1000.00')):
        assert label_text(cs['ids'][row], cs['scores'][row]) == text
    img = on_black((4, 20, 40, 45), LabelStyle(scale=1), scores=np.array([np.nan], np.float32))
    assert np.array_equal(img, on_black((4, 20, 40, 45), LabelStyle(scale=1)))


def test_later_row_wins_and_the_order_of_rows_matters():
    cs = CASES['overlap3_rgb']
    flipped = dict(cs, boxes=cs['boxes'][::-1], ids=cs['ids'][::-1])
    a, b = pictures('overlap3_rgb')[0], lc.run_tap(flipped)
    assert not lc.same(a, b)
    img = a[0].reshape(64, 96, 3)
    # the blocks are x 5..30 / y 12..29, x 12..37 / y 19..36 and x 9..34 / y 23..40: row 2's corner lies over rows 0 and 1, row 1's corner over row 0
    assert tuple(img[23, 9]) == LIMB_COLORS[4] and tuple(img[19, 12]) == LIMB_COLORS[1] and tuple(img[12, 5]) == LIMB_COLORS[7]
    # (12, 28) lies in all three blocks, on background in the first and the last of them: rows reversed, the first box's tag is the last one
    assert tuple(img[28, 12]) == LIMB_COLORS[4] and tuple(b[0].reshape(64, 96, 3)[28, 12]) == LIMB_COLORS[7]


def test_rows_of_two_frames_interleaved_equal_each_frame_written_alone():
    cs = CASES['two_frames']
    both = pictures('two_frames')[0]
    ids = np.arange(len(cs['boxes']), dtype=np.int32)   # the colour and the text of a row follow its index in the combined call
    for f, planes in ((0, [0]), (1, [1, 2])):
        alone = dict(cs, fi=np.where(cs['fi'] == f, cs['fi'], -1).astype(np.int32), ids=ids)
        got = lc.run_tap(alone)
        _, before = lc.build_frames(cs['specs'], cs['seed'])
        for p in range(3):
            assert np.array_equal(got[p], both[p] if p in planes else before[p])


def test_n_zero_writes_nothing():
    img = np.full((16, 16, 3), 7, np.uint8)
    for fn in (draw_labels_model_host, draw_labels_numpy):
        fn([img], np.zeros((0, 4), np.float32), np.zeros(0, np.int32))
        assert (img == 7).all()


# ---- refusals
def tap_call(images=True, n_images=1, boxes=True, n=2, box_stride=4, fidx=True, frame_stride=1, scores=False, score_stride=1, cfg=True, image=None, **over):
    """one vp_dbg_draw_labels_host call with one argument made bad: (status, message)"""
    lib = capi.load_library()
    img = np.zeros((16, 16, 3), np.uint8)
    y, uv = np.zeros((16, 16), np.uint8), np.zeros((8, 8, 2), np.uint8)
    fields = dict(plane=(img.ctypes.data, None), pitch=(48, 0), h=16, w=16, format=0, matrix=0)
    if image:
        if image.get('format') == 2:
            fields.update(plane=(y.ctypes.data, uv.ctypes.data), pitch=(16, 16))
        fields.update(image)
    table = (capi.vp_image * 1)(capi.vp_image((C.c_void_p * 2)(*fields['plane']), (C.c_int64 * 2)(*fields['pitch']), fields['h'], fields['w'], fields['format'], fields['matrix']))
    m = max(n, 1) if n <= 10000 else 1   # a refused n is never read
    bx = np.zeros((m, max(box_stride, 4)), np.float32)
    fi = np.zeros(m * max(frame_stride, 1), np.int32)
    sc = np.zeros(m * max(score_stride, 1), np.float32)
    col = np.array(LIMB_COLORS, np.uint8)
    c = dict(scale=0, n_colors=8, colors=col.ctypes.data, auto_ink=1, ink=(C.c_uint8 * 3)(0, 0, 0), show_score=1)
    c.update(over)
    cfg_s = capi.vp_label_cfg(*(c[f] for f, _ in capi.vp_label_cfg._fields_))
    rc = lib.vp_dbg_draw_labels_host(table if images else None, n_images, bx.ctypes.data if boxes else None, box_stride, n, fi.ctypes.data if fidx else None, frame_stride,
                                     None, None, sc.ctypes.data if scores else None, score_stride, C.byref(cfg_s) if cfg else None)
    return rc, capi.last_error(None)


REFUSALS = {
    'null cfg': dict(cfg=False),
    'negative n': dict(n=-1),
    'n above the workspace': dict(n=8193),
    'null images': dict(images=False),
    'null boxes': dict(boxes=False),
    'null frame index': dict(fidx=False),
    'no frames': dict(n_images=0),
    'negative n_images': dict(n_images=-1),
    'scale -1': dict(scale=-1),
    'scale 9': dict(scale=9),
    'no colours': dict(n_colors=0),
    '33 colours': dict(n_colors=33),
    'null colours': dict(colors=None),
    'box stride 0': dict(box_stride=0),
    'frame stride 0': dict(frame_stride=0),
    'score stride 0': dict(scores=True, score_stride=0),
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
    assert rc == capi.VP_ERR_INVALID and msg.startswith('labels: '), (what, rc, msg)


def test_accepted_calls_of_the_c_entry():
    assert tap_call()[0] == capi.VP_OK
    assert tap_call(n=0, images=False, boxes=False, fidx=False, n_images=0)[0] == capi.VP_OK   # n = 0: nothing needed
    assert tap_call(n=8192)[0] == capi.VP_OK                                                   # exactly the workspace limit
    assert tap_call(scale=8, n_colors=1, auto_ink=0, show_score=0, scores=True, score_stride=3, box_stride=6)[0] == capi.VP_OK
    assert tap_call(score_stride=0)[0] == capi.VP_OK                                           # without scores their stride is not looked at
    assert tap_call(image=dict(format=2, matrix=2))[0] == capi.VP_OK
    assert capi.load_library().vp_dbg_label_text(1, 0, C.c_float(0), None) == capi.VP_ERR_INVALID


def test_refusals_of_the_python_layer():
    for kw in (dict(scale=-1), dict(scale=9), dict(scale=1.5), dict(scale=True), dict(colors=[]), dict(colors=[(0, 0, 256)]), dict(colors=[(0, 0, 0)] * 33), dict(colors=5),
               dict(ink=(1, 2)), dict(ink=(0, 0, 256)), dict(ink=7), dict(show_score=1)):
        with pytest.raises(ValueError, match='LabelStyle'):
            LabelStyle(**kw)
    with pytest.raises(dataclasses_frozen_error()):
        LabelStyle().scale = 2
    img = np.zeros((16, 16, 3), np.uint8)
    bx = np.zeros((2, 4), np.float32)
    for fn in (draw_labels_numpy, draw_labels_model_host):
        with pytest.raises(ValueError, match='boxes are required'):
            fn([img], None, np.zeros(2, np.int32))
        with pytest.raises(ValueError):
            fn([img], bx[:, :3], np.zeros(2, np.int32))
        with pytest.raises(ValueError):
            fn([img], bx, np.zeros(3, np.int32))
        with pytest.raises(ValueError):
            fn([img], bx, np.zeros(2, np.int32), scores=np.zeros(3))
        with pytest.raises(ValueError, match='8192'):
            fn([img], np.zeros((8193, 4), np.float32), np.zeros(8193, np.int32))
        with pytest.raises(TypeError):
            fn([img], bx, np.zeros(2, np.int32), style=dict(scale=2))
        with pytest.raises((TypeError, ValueError)):
            fn([img.astype(np.float32)], bx, np.zeros(2, np.int32))
    kp = np.zeros((2, 17, 3), np.float32)
    for fn in (draw_poses_numpy, draw_poses_model_host):
        with pytest.raises(ValueError, match='boxes are required'):
            fn([img], kp, np.zeros(2, np.int32), labels=LabelStyle())
        with pytest.raises(TypeError):
            fn([img], kp, np.zeros(2, np.int32), boxes=bx, labels=True)


def dataclasses_frozen_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


# ---- layering
def test_draw_poses_with_labels_equals_labels_followed_by_poses():
    """on the overlay's own cases that carry boxes: tags first, skeletons over them, the tags in the overlay's limb palette"""
    rng = np.random.default_rng(4)
    for name in ('nv12_bt709_97x131', 'rgb_pitched', 'two_frames', 'style_t5_r7'):
        cs = dc.host_cases()[name]
        n = len(cs['kp'])
        scores = rng.uniform(0, 1, n).astype(np.float32)
        labels = LabelStyle(scale=1)
        for fn, lab in ((draw_poses_numpy, draw_labels_numpy), (draw_poses_model_host, draw_labels_model_host)):
            f1, one = dc.build_frames(cs['specs'], cs['seed'])
            fn(f1, cs['kp'], cs['fi'], cs['style'], rank=cs['rank'], ids=cs['ids'], boxes=cs['boxes'], labels=labels, scores=scores)
            f2, two = dc.build_frames(cs['specs'], cs['seed'])
            palette = cs['style'].limb_colors
            lab(f2, cs['boxes'], cs['fi'], LabelStyle(scale=1, colors=palette), rank=cs['rank'], ids=cs['ids'], scores=scores)
            fn(f2, cs['kp'], cs['fi'], cs['style'], rank=cs['rank'], ids=cs['ids'], boxes=cs['boxes'])
            assert dc.same(one, two), name
            f3, none = dc.build_frames(cs['specs'], cs['seed'])
            fn(f3, cs['kp'], cs['fi'], cs['style'], rank=cs['rank'], ids=cs['ids'], boxes=cs['boxes'], labels=None)
            assert dc.same(none, dc.run_tap(cs)) and not dc.same(none, one), name
    f1, one = dc.build_frames(cs['specs'], cs['seed'])
    f2, two = dc.build_frames(cs['specs'], cs['seed'])
    draw_poses_numpy(f1, cs['kp'], cs['fi'], cs['style'], boxes=cs['boxes'], labels=labels, scores=scores)
    draw_poses_model_host(f2, cs['kp'], cs['fi'], cs['style'], boxes=cs['boxes'], labels=labels, scores=scores)
    assert dc.same(one, two)


def test_vitinference_and_cli_surface():
    from easy_vitpose_amd import cli
    from easy_vitpose_amd.inference import VitInference
    import inspect
    assert inspect.signature(VitInference.__init__).parameters['labels'].default is False
    assert list(inspect.signature(VitInference.draw).parameters)[1:] == ['show_yolo', 'show_raw_yolo', 'confidence_threshold']
    assert 'NOT provided: text labels' not in VitInference.draw.__doc__ and 'tag' in VitInference.draw.__doc__
    with pytest.raises(TypeError, match='labels'):
        VitInference({}, lambda img: np.empty((0, 5)), 's', dataset='coco', labels='yes')
    base = ['--input', 'x.png', '--synthetic', 's', '--boxes', 'b.json']
    args = cli.build_parser().parse_args(base + ['--output-path', 'o', '--save-img', '--labels', '--label-scale', '3'])
    assert args.labels and args.label_scale == 3
    args = cli.build_parser().parse_args(base)
    assert not args.labels and args.label_scale is None
    with pytest.raises(AssertionError, match='--save-img'):
        cli.main(base + ['--labels'])
    with pytest.raises(AssertionError, match='--save-img'):
        cli.main(base + ['--label-scale', '2'])
    from easy_vitpose_amd import VitPoseHip
    for fn in (VitPoseHip.draw_poses, VitPoseHip.draw_poses_host):
        p = inspect.signature(fn).parameters
        assert p['labels'].default is None and p['scores'].default is None
    assert list(inspect.signature(VitPoseHip.draw_labels).parameters)[1:] == ['frames', 'boxes', 'frame_index', 'style', 'rank', 'ids', 'scores']
