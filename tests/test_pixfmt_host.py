"""CPU: the host side of the pixel formats of the frames and boxes entries (vp_image: NV12, BGR, pitched rows) -- the colour conversion of
cropprep against plain Python integers, the Frame type, the struct and the header, and the plan over vp_image (vp_dbg_image_plan) with every refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import Frame
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.cropprep import nv12_to_rgb, rgb_to_nv12, to_rgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (yoff, cy, crv, cgu, cgv, cbu): restated here from the contract, not imported
TABLE = {
    'bt601': (16, 1220542, 1673527, -409993, -852492, 2116026),
    'bt709': (16, 1220945, 1879825, -223607, -558796, 2215014),
    'bt601_full': (0, 1048576, 1470104, -360853, -748826, 1858077),
}


def scalar_rgb(matrix, Y, U, V):
    """one sample in plain Python integers (>> floors, as the contract's arithmetic shift does)"""
    yoff, cy, crv, cgu, cgv, cbu = TABLE[matrix]
    y, u, v = max(Y - yoff, 0), U - 128, V - 128
    clip = lambda x: min(max(x, 0), 255)
    return (clip((cy * y + crv * v + (1 << 19)) >> 20), clip((cy * y + cgu * u + cgv * v + (1 << 19)) >> 20), clip((cy * y + cbu * u + (1 << 19)) >> 20))


LATTICE = sorted(set(list(range(0, 256, 17)) + [128, 255]))   # 17 values, 0, 128 and 255 among them


@pytest.mark.parametrize('matrix', sorted(TABLE))
def test_nv12_to_rgb_equals_the_scalar_restatement(matrix):
    assert len(LATTICE) == 17 and {0, 128, 255} <= set(LATTICE)
    # one frame: row = the (U, V) pair (repeated, so that each pair owns a chroma row), column = Y
    pairs = [(u, v) for u in LATTICE for v in LATTICE]
    y = np.tile(np.arange(256, dtype=np.uint8), (2 * len(pairs), 1))
    uv = np.zeros((len(pairs), 128, 2), np.uint8)
    for r, (u, v) in enumerate(pairs):
        uv[r] = (u, v)
    got = nv12_to_rgb(y, uv, matrix)
    assert got.dtype == np.uint8 and got.shape == (2 * len(pairs), 256, 3)
    want = np.array([[scalar_rgb(matrix, Y, u, v) for Y in range(256)] for (u, v) in pairs], np.uint8)
    assert np.array_equal(got[0::2], want) and np.array_equal(got[1::2], want)


@pytest.mark.parametrize('matrix', sorted(TABLE))
def test_chroma_indexing_on_an_odd_frame(matrix):
    rng = np.random.default_rng(3)
    h, w = 5, 7
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    uv = rng.integers(0, 256, (3, 4, 2), dtype=np.uint8)
    got = nv12_to_rgb(y, uv, matrix)
    for r in range(h):
        for c in range(w):
            assert tuple(got[r, c]) == scalar_rgb(matrix, int(y[r, c]), int(uv[r >> 1, c >> 1, 0]), int(uv[r >> 1, c >> 1, 1])), (r, c)
    with pytest.raises(AssertionError):
        nv12_to_rgb(y, uv[:2], matrix)


def test_grey_axis_landmarks():
    grey = np.arange(256, dtype=np.uint8)[None]
    uv = np.full((1, 128, 2), 128, np.uint8)
    for matrix in ('bt601', 'bt709'):
        g = nv12_to_rgb(grey, uv, matrix)[0]
        assert (g[..., 0] == g[..., 1]).all() and (g[..., 1] == g[..., 2]).all()
        assert g[16, 0] == 0 and g[235, 0] == 255 and (g[:16] == 0).all() and (g[235:] == 255).all()
        assert (np.diff(g[:, 0].astype(int)) >= 0).all()
    full = nv12_to_rgb(grey, uv, 'bt601_full')[0]
    assert np.array_equal(full, np.repeat(grey[0][:, None], 3, 1))   # grey is the identity on the full-range row
    # the largest intermediate of the whole (Y, U, V) cube fits int32 (the extremes sit at its corners: every term is monotone in each variable)
    for yoff, cy, crv, cgu, cgv, cbu in TABLE.values():
        worst = cy * (255 - yoff) + (1 << 19) + max(abs(crv), abs(cbu), abs(cgu) + abs(cgv)) * 128
        assert worst < 2 ** 31 and worst < 5.8e8


def test_to_rgb_of_bgr_and_strided_views():
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    assert np.array_equal(to_rgb(Frame.bgr(a)), a[..., ::-1])
    assert np.array_equal(to_rgb(Frame.rgb(a)), a) and np.array_equal(to_rgb(a), a)
    wide = rng.integers(0, 256, (12, 40, 3), dtype=np.uint8)
    view = wide[2:11, 5:16]                                   # rows at a pitch of 120 bytes
    f = Frame.rgb(view)
    assert f.pitch == (120, 0) and (f.h, f.w) == (9, 11) and f.pointers()[0] == view.ctypes.data and not f.on_device
    assert np.array_equal(to_rgb(f), np.ascontiguousarray(view)) and to_rgb(f).flags.c_contiguous
    assert np.array_equal(to_rgb(Frame.bgr(view)), np.ascontiguousarray(view)[..., ::-1])
    # NV12 planes inside one surface: Y pitch 16, UV behind an aligned height at pitch 24
    surf = rng.integers(0, 256, 16 * 16 + 8 * 24, dtype=np.uint8)
    y = surf[:16 * 16].reshape(16, 16)[:9, :11]
    uv = surf[16 * 16:].reshape(8, 12, 2)[:5, :6]
    f = Frame.nv12(y, uv, 'bt709')
    assert f.pitch == (16, 24) and f.shape == (9, 11, 3)
    assert np.array_equal(to_rgb(f), nv12_to_rgb(np.ascontiguousarray(y), np.ascontiguousarray(uv), 'bt709'))


def test_rgb_to_nv12_is_deterministic_and_roughly_inverts():
    rng = np.random.default_rng(5)
    smooth = np.repeat(np.repeat(rng.integers(30, 226, (4, 5, 3), dtype=np.uint8), 2, 0), 2, 1)[:7, :9]   # constant 2 x 2 blocks, odd size
    for matrix in sorted(TABLE):
        y, uv = rgb_to_nv12(smooth, matrix)
        y2, uv2 = rgb_to_nv12(smooth.copy(), matrix)
        assert y.shape == (7, 9) and uv.shape == (4, 5, 2) and y.dtype == uv.dtype == np.uint8
        assert np.array_equal(y, y2) and np.array_equal(uv, uv2)
        back = nv12_to_rgb(y, uv, matrix).astype(int)
        assert np.abs(back - smooth.astype(int)).max() <= 3     # 8-bit YUV quantisation, nothing more


def test_frame_construction_errors():
    a = np.zeros((6, 8, 3), np.uint8)
    y, uv = np.zeros((5, 7), np.uint8), np.zeros((3, 4, 2), np.uint8)
    Frame.nv12(y, uv)
    with pytest.raises(TypeError):
        Frame.rgb(a.astype(np.float32))
    with pytest.raises(TypeError):
        Frame.nv12(y, uv.astype(np.int16))
    with pytest.raises(TypeError):
        Frame.rgb([[[0, 0, 0]]])
    for bad_uv in (np.zeros((2, 4, 2), np.uint8), np.zeros((3, 3, 2), np.uint8), np.zeros((3, 4), np.uint8), np.zeros((3, 8), np.uint8)):
        with pytest.raises(ValueError):
            Frame.nv12(y, bad_uv)
    with pytest.raises(ValueError):
        Frame.rgb(np.zeros((6, 8, 4), np.uint8))
    with pytest.raises(ValueError):
        Frame.rgb(a[..., ::-1])                                # last-dimension stride -1
    with pytest.raises(ValueError):
        Frame.bgr(np.zeros((6, 8, 6), np.uint8)[..., ::2])     # last-dimension stride 2
    with pytest.raises(ValueError):
        Frame.rgb(a[:, ::2])                                   # pixels 6 bytes apart
    with pytest.raises(ValueError):
        Frame.nv12(np.zeros((5, 14), np.uint8)[:, ::2], uv)
    with pytest.raises(ValueError):
        Frame.nv12(y, np.zeros((3, 4, 4), np.uint8)[..., ::2])
    with pytest.raises(ValueError):
        Frame.rgb(a[::-1])                                     # reversed rows: a negative pitch
    with pytest.raises(ValueError):
        Frame.nv12(y, uv, matrix='bt2020')


def test_struct_header_and_symbols():
    assert C.sizeof(capi.vp_image) == 48
    assert (capi.vp_image.plane.offset, capi.vp_image.pitch.offset, capi.vp_image.h.offset, capi.vp_image.w.offset, capi.vp_image.format.offset,
            capi.vp_image.matrix.offset) == (0, 16, 32, 36, 40, 44)
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    assert re.search(r'#define\s+VP_HAS_IMAGE_ENTRIES\s+1', hdr) and re.search(r'#define\s+VP_ABI_VERSION\s+4\b', hdr)
    for name, val in (('VP_PIX_RGB24', 0), ('VP_PIX_BGR24', 1), ('VP_PIX_NV12', 2), ('VP_YUV_BT601', 0), ('VP_YUV_BT709', 1), ('VP_YUV_BT601_FULL', 2)):
        assert re.search(r'#define\s+' + name + r'\s+' + str(val) + r'\b', hdr), name
        assert getattr(capi, name) == val
    lib = capi.load_library()
    for name in ('vp_infer_images', 'vp_infer_boxes_images_stream', 'vp_dbg_image_plan', 'vp_dbg_crop_prep_image'):
        assert re.search(r'VP_API\s+int\s+' + name + r'\s*\(', hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.vp_infer_images(None, None, 0, 0, None, 0, None, None) == capi.VP_ERR_INVALID
    assert lib.vp_infer_boxes_images_stream(None, None, 0, None, 4, None, 0, 10, None, None, None, None, None) == capi.VP_ERR_INVALID


# ---- vp_dbg_image_plan
_DUMMY = np.zeros(16, np.uint8)   # the plan never reads pixels
PTR = _DUMMY.ctypes.data
SIZES = [(720, 1280), (1080, 1920), (481, 333), (256, 192), (40, 30)]
GOOD = (1, 10, 20, 30, 40, 0, 5, 30, 50)


def image(h, w, fmt=capi.VP_PIX_RGB24, matrix=0, p0=PTR, p1=None, pitch0=None, pitch1=None):
    nv12 = fmt == capi.VP_PIX_NV12
    if pitch0 is None:
        pitch0 = w if nv12 else 3 * w
    if pitch1 is None:
        pitch1 = 2 * ((w + 1) // 2) if nv12 else 0
    if nv12 and p1 is None:
        p1 = PTR
    return capi.vp_image((C.c_void_p * 2)(p0, p1 if p1 != 0 else None), (C.c_int64 * 2)(pitch0, pitch1), h, w, fmt, matrix)


def iplan(images, p9):
    lib = capi.load_library()
    p9 = np.ascontiguousarray(p9, dtype=np.int32).reshape(-1, 9)
    t = (capi.vp_image * max(len(images), 1))(*images)
    bands = np.full((max(len(images), 1), 2), -7, np.int32)
    rc = lib.vp_dbg_image_plan(t, len(images), p9.ctypes.data if len(p9) else None, len(p9), bands.ctypes.data)
    return rc, bands[:len(images)], capi.last_error()


def test_image_plan_bands_equal_frame_plan_on_rgb_frames():
    lib = capi.load_library()
    rng = np.random.default_rng(8)
    rows = []
    for f, (h, w) in enumerate(SIZES):
        for _ in range(0 if f == 3 else 4):
            cw, ch = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
            rows.append((f, int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch, 1, 2, cw + 3, ch + 4))
    p9 = np.array(rows, np.int32)[rng.permutation(len(rows))]
    frames = (capi.vp_frame * len(SIZES))(*[capi.vp_frame(PTR, h, w) for h, w in SIZES])
    want = np.zeros((len(SIZES), 2), np.int32)
    p9c = np.ascontiguousarray(p9)
    assert lib.vp_dbg_frame_plan(frames, len(SIZES), p9c.ctypes.data, len(p9c), want.ctypes.data) == capi.VP_OK
    for fmt in (capi.VP_PIX_RGB24, capi.VP_PIX_BGR24, capi.VP_PIX_NV12):   # the bands are frame rows whatever the layout
        rc, bands, msg = iplan([image(h, w, fmt, pitch0=3 * w + 64 if fmt != capi.VP_PIX_NV12 else w + 64) for h, w in SIZES], p9)
        assert rc == capi.VP_OK, msg
        assert np.array_equal(bands, want) and tuple(bands[3]) == (0, 0)


def test_image_plan_accepts_odd_nv12_at_the_minimum_pitches():
    h, w = 481, 333
    p9 = np.array([[0, 0, 0, w, h, 0, 0, w, h], [0, w - 1, h - 1, 1, 1, 0, 0, 1, 1], [0, 331, 479, 2, 2, 0, 0, 2, 2]], np.int32)
    for matrix in (0, 1, 2):
        rc, bands, msg = iplan([image(h, w, capi.VP_PIX_NV12, matrix, pitch0=333, pitch1=334)], p9)
        assert rc == capi.VP_OK, msg
        assert bands.tolist() == [[0, h]]
    assert iplan([image(5, 7, capi.VP_PIX_NV12, pitch0=7, pitch1=8)], [[0, 6, 4, 1, 1, 0, 0, 1, 1]])[0] == capi.VP_OK
    # the matrix is read for NV12 only
    assert iplan([image(5, 7, capi.VP_PIX_BGR24, matrix=99)], [[0, 6, 4, 1, 1, 0, 0, 1, 1]])[0] == capi.VP_OK


@pytest.mark.parametrize('case,bad', [
    ('unknown format', dict(fmt=3)),
    ('negative format', dict(fmt=-1)),
    ('unknown matrix', dict(fmt=capi.VP_PIX_NV12, matrix=3)),
    ('negative matrix', dict(fmt=capi.VP_PIX_NV12, matrix=-1)),
    ('RGB pitch below 3 w', dict(pitch0=3 * 1920 - 1)),
    ('BGR pitch below 3 w', dict(fmt=capi.VP_PIX_BGR24, pitch0=1920)),
    ('Y pitch below w', dict(fmt=capi.VP_PIX_NV12, pitch0=1919)),
    ('NV12 without a UV plane', dict(fmt=capi.VP_PIX_NV12, p1=0)),
    ('UV pitch below 2 ceil(w/2)', dict(fmt=capi.VP_PIX_NV12, pitch1=1919)),
    ('negative pitch', dict(pitch0=-3 * 1920)),
    ('negative UV pitch', dict(fmt=capi.VP_PIX_NV12, pitch1=-1920)),
    ('no data', dict(p0=None)),
    ('non-positive size', dict(h=0)),
])
def test_image_plan_refuses_bad_images_where_referenced(case, bad):
    kw = dict(h=1080, w=1920)
    kw.update(bad)
    images = [image(h, w) for h, w in SIZES]
    images[1] = image(**kw)
    p9 = np.array([(0,) + GOOD[1:], GOOD, GOOD], np.int32)
    rc, _, msg = iplan(images, p9)
    assert rc == capi.VP_ERR_INVALID, case
    assert 'crop 1' in msg and 'frame 1' in msg, msg        # the first crop that names the frame, and the frame
    assert iplan(images, np.array([(0,) + GOOD[1:]], np.int32))[0] == capi.VP_OK   # a frame without crops is never looked at
    images[1] = image(1080, 1920)
    assert iplan(images, p9)[0] == capi.VP_OK


def test_image_plan_odd_width_uv_pitch_counts_the_ceil():
    ok = image(5, 7, capi.VP_PIX_NV12, pitch0=7, pitch1=8)
    short = image(5, 7, capi.VP_PIX_NV12, pitch0=7, pitch1=7)    # 2 * floor(7 / 2) + 1: the last pair would leave the row
    row = [[0, 0, 0, 7, 5, 0, 0, 7, 5]]
    assert iplan([ok], row)[0] == capi.VP_OK
    rc, _, msg = iplan([short], row)
    assert rc == capi.VP_ERR_INVALID and 'frame 0' in msg and 'pitch[1]' in msg


@pytest.mark.parametrize('row', [
    (-1,) + GOOD[1:], (5,) + GOOD[1:], (1, -1) + GOOD[2:], (1, 1920 - 29) + GOOD[2:], (1, 10, 1080 - 39) + GOOD[3:], (1, 10, 20, 0, 40, 0, 0, 30, 40),
    (1, 10, 20, 30, 40, -1, 0, 30, 40), (1, 10, 20, 30, 40, 0, 11, 30, 50), (1, 2 ** 31 - 10, 20, 30, 40, 0, 0, 30, 40)])
def test_image_plan_refuses_what_frame_plan_refuses(row):
    images = [image(h, w, capi.VP_PIX_NV12) for h, w in SIZES]
    rc, _, msg = iplan(images, np.array([GOOD, row, GOOD], np.int32))
    assert rc == capi.VP_ERR_INVALID and 'crop 1' in msg, msg
    lib = capi.load_library()
    p9 = np.array([GOOD], np.int32)
    t = (capi.vp_image * len(images))(*images)
    assert lib.vp_dbg_image_plan(t, 0, p9.ctypes.data, 1, None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_image_plan(None, 5, p9.ctypes.data, 1, None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_image_plan(t, 5, None, 1, None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_image_plan(t, 5, p9.ctypes.data, -1, None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_image_plan(t, 5, p9.ctypes.data, 1, None) == capi.VP_OK
    assert lib.vp_dbg_image_plan(None, 0, None, 0, None) == capi.VP_OK
