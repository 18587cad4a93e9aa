"""CPU: the letterbox stage of csrc/lbgeom.h through the host tap vp_dbg_letterbox_host -- the same functions the kernel of vp_letterbox_stream runs -- against a
numpy twin written from the contract (devletterbox.letterbox_host_numpy), against the independent C restatement of the resize (oracle/resize_ref.c), against
plain-integer geometry written here, every refusal of the C entries and of the Python layer, the two tables on the grid of the contract, and the Python routes
(VitInference(letterbox=), --det-engine) against a fake engine.  The device is compared with this host model in tests/test_gpu_letterbox.py."""
from __future__ import annotations

import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.cropprep import Frame, to_rgb
from easy_vitpose_amd.devdetect import DetectCfg, HostDetector, image_table as det_image_table, letterbox_params
from easy_vitpose_amd.devletterbox import (DTYPES, IMAGE_DTYPE, MAX_IMAGES, MAX_SIDE, NP_DTYPES, DeviceLetterbox, HostLetterbox, LetterboxCfg, c_config, image_table,
                                           letterbox_geometry, letterbox_host_numpy, letterbox_plan)
from letterbox_cases import CANARY, named_cases, nv12_frame, rgb_frame, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = named_cases()
GRID_INPUTS = ((640, 640), (320, 320), (32, 32), (48, 40), (384, 640))


def integer_geometry(h, w, in_h, in_w, scaleup=True):
    """(left, top, new_w, new_h) in integers alone: r = a / b with (a, b) = (in_h, h) or (in_w, w), whichever is smaller; round(s a / b) half to even"""
    a, b = (in_h, h) if in_h * w <= in_w * h else (in_w, w)
    if not scaleup and a > b:
        a, b = 1, 1

    def rnd(num, den):   # round(num / den), half to even, num >= 0
        q, r = divmod(num, den)
        return q + (1 if 2 * r > den or (2 * r == den and q % 2) else 0)

    new_w, new_h = rnd(w * a, b), rnd(h * a, b)
    # round(d / 2 - 0.1) for an integer d >= 0: d even -> d / 2 (x.9 rounds up), d odd -> (d - 1) / 2 (x.4 rounds down)
    return (in_w - new_w) // 2, (in_h - new_h) // 2, new_w, new_h


def test_surface_symbols_macros_and_build_flags():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    for name in ('vp_letterbox_plan', 'vp_letterbox_stream', 'vp_letterbox', 'vp_dbg_letterbox_host'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r'VP_API\s+int\s+' + name + r'\s*\(', hdr), name
    assert re.search(r'#define\s+VP_HAS_LETTERBOX\s+1\b', hdr) and re.search(r'#define\s+VP_LB_MAX_IMAGES\s+64\b', hdr)
    for name, value in DTYPES.items():
        assert re.search(r'#define\s+VP_LB_%s\s+%d\b' % ({'fp32': 'F32', 'fp16': 'F16', 'u8': 'U8'}[name], value), hdr), name
    assert (MAX_IMAGES, MAX_SIDE) == (64, 8192)
    assert C.sizeof(capi.vp_letterbox_cfg) == 28 and [f[0] for f in capi.vp_letterbox_cfg._fields_] == ['in_h', 'in_w', 'dtype', 'layout', 'order', 'pad_value', 'scaleup']
    assert IMAGE_DTYPE.itemsize == C.sizeof(capi.vp_image) == 48
    build = __import__('easy_vitpose_amd.build', fromlist=['SOURCES'])
    assert 'letterbox.hip' in build.SOURCES and build.SOURCE_FLAGS['letterbox.hip'] == ['-ffp-contract=off'] and 'lbgeom.h' in build.HEADERS
    assert lib.vp_abi_version() == 4


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_tap_equals_the_numpy_twin(name):
    cfg, frames = CASES[name]
    out, det, placement = HostLetterbox(cfg).letterbox(frames)
    assert out.shape == cfg.shape(len(frames)) and out.dtype == NP_DTYPES[cfg.dtype] and det.shape == (len(frames), 5) and placement.shape == (len(frames), 4)
    for i, f in enumerate(frames):
        want, row, place = letterbox_host_numpy(f, cfg)
        assert same_bits(out[i], want), f'frame {i}: tensor differs'
        assert same_bits(det[i], row) and same_bits(placement[i], place), f'frame {i}: {det[i]} {row} {placement[i]} {place}'


@pytest.mark.parametrize('name', sorted(n for n in CASES if not n.startswith('out_') or n.startswith('out_u8')))
def test_interior_equals_the_c_restatement_and_the_rest_is_pad(name):
    """the placed interior against oracle/resize_ref.c on the host-converted RGB frame, the placement against integers, every other element the pad"""
    from oracle.resize_ref import resize_linear_u8 as ref
    cfg, frames = CASES[name]
    u8 = LetterboxCfg(cfg.input_hw, 'u8', 'nhwc', 'rgb', cfg.pad_value, cfg.scaleup)
    out, det, placement = HostLetterbox(u8).letterbox(frames)
    in_h, in_w = cfg.input_hw
    for i, f in enumerate(frames):
        left, top, new_w, new_h = integer_geometry(f.h, f.w, in_h, in_w, cfg.scaleup)
        assert placement[i].tolist() == [left, top, new_w, new_h], (placement[i], (left, top, new_w, new_h))
        assert 0 <= left and left + new_w <= in_w and 0 <= top and top + new_h <= in_h
        assert (in_w - new_w - left) - left in (0, 1) and (in_h - new_h - top) - top in (0, 1), 'the odd pixel of pad goes right / below'
        rgb = to_rgb(f)
        inner = rgb if (new_w, new_h) == (f.w, f.h) else ref(rgb, (new_w, new_h))
        assert np.array_equal(out[i, top:top + new_h, left:left + new_w], inner), f'frame {i}: interior'
        mask = np.ones((in_h, in_w), bool)
        mask[top:top + new_h, left:left + new_w] = False
        assert (out[i][mask] == cfg.pad_value).all(), f'frame {i}: pad'


def test_what_the_named_cases_show():
    place = {name: HostLetterbox(cfg).letterbox(frames)[2] for name, (cfg, frames) in CASES.items()}
    assert place['identity'].tolist() == [[0, 0, 32, 32]] and place['box_2x'].tolist() == [[0, 0, 32, 32]]
    assert place['two_x_on_one_axis_and_half_up'].tolist() == [[15, 0, 2, 32]] and place['half_to_even_down'].tolist() == [[15, 0, 2, 32]]
    assert place['odd_pad_5x7'].tolist() == [[0, 4, 32, 23]], 'top 4, bottom 5'
    assert place['no_scaleup_small'].tolist() == [[9, 11, 13, 10], [10, 11, 11, 9]] and place['no_scaleup_large'].tolist() == [[0, 4, 32, 23]]
    assert place['wide'][0, 0] == 0 and place['wide'][0, 1] > 0 and place['tall'][0, 1] == 0 and place['tall'][0, 0] > 0
    cfg, frames = CASES['two_x_on_one_axis_and_half_up']
    out = HostLetterbox(LetterboxCfg(cfg.input_hw, 'u8', 'nhwc')).letterbox(frames)[0][0]
    rgb = to_rgb(frames[0]).astype(np.int64)
    box = (rgb[0::2, 0:1] + rgb[1::2, 0:1] + rgb[0::2, 1:2] + rgb[1::2, 1:2] + 2) >> 2
    assert not np.array_equal(out[:, 15:16], box), '2 x on one axis alone is no box average'
    cfg, frames = CASES['no_scaleup_small']
    det = HostLetterbox(cfg).letterbox(frames)[1]
    assert det.tolist() == [[1.0, 9.0, 11.0, 13.0, 10.0], [1.0, 10.0, 11.0, 11.0, 9.0]], 'a clamped r: (1, left, top) and the frame size'
    det640, place640 = letterbox_plan([(5, 7), (1, 6)], LetterboxCfg((640, 640)))
    assert place640[:, 1].tolist() == [91, 266] and det640[:, 2].tolist() == [91.0, 267.0], 'the two conventions of the contract'


def test_value_tables_for_all_256_bytes():
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    frame = Frame.rgb(np.ascontiguousarray(np.stack([ramp, ramp, ramp], -1)))
    f32 = np.arange(256, dtype=np.float32) / np.float32(255)
    for dtype, want in (('fp32', f32), ('fp16', f32.astype(np.float16)), ('u8', np.arange(256, dtype=np.uint8))):
        out = HostLetterbox(LetterboxCfg((16, 16), dtype=dtype)).letterbox([frame])[0]
        assert same_bits(out[0, 0].ravel(), want) and same_bits(out[0, 2].ravel(), want), dtype
    assert f32[255] == 1 and f32[0] == 0 and len(set(f32.astype(np.float16).tolist())) == 256


def double_geometry(h, w, in_h, in_w):
    """the contract's geometry on Python floats (doubles; `round` is half to even)"""
    r = min(in_h / h, in_w / w)
    new_w, new_h = round(w * r), round(h * r)
    return round((in_w - new_w) / 2 - 0.1), round((in_h - new_h) / 2 - 0.1), new_w, new_h


def grid_sizes():
    hh, ww = np.meshgrid(np.arange(1, 400), np.arange(1, 400), indexing='ij')
    return np.stack([hh.ravel(), ww.ravel()], 1)


def test_the_two_tables_on_the_grid_of_the_contract():
    """h, w in 1..399 into the five inputs: a size is refused iff its new_w or new_h is 0; on every other size the undo table is letterbox_params bit for bit
    and the placement the contract's double arithmetic; the two disagree by one pixel of pad on exactly 119 408 of the 796 005 sizes (refused sizes never do).
    The contract rounds the DOUBLE product w * r: on four sizes of the grid (352 x 55, 99, 187, 231 into 48 x 40) r = 40 / w' is inexact and the product lands
    just below an exact half (7.499999999999999 for 15 / 2), so new_w is one less than rounding the exact quotient gives; everywhere else the two agree."""
    hw = grid_sizes()
    total = disagree = refused = 0
    inexact_halves = []
    for in_h, in_w in GRID_INPUTS:
        cfg = LetterboxCfg((in_h, in_w))
        want_place = np.array([double_geometry(h, w, in_h, in_w) for h, w in hw.tolist()], np.int32)
        exact = np.array([integer_geometry(h, w, in_h, in_w) for h, w in hw.tolist()], np.int32)
        inexact_halves += [(in_h, in_w, h, w) for h, w in hw[(exact != want_place).any(1)].tolist()]
        ok = (want_place[:, 2] >= 1) & (want_place[:, 3] >= 1)
        for h, w in hw[~ok][:: max(1, int((~ok).sum()) // 40)].tolist():
            with pytest.raises(capi.VpError, match='scales to an empty image'):
                letterbox_plan([(h, w)], cfg)
            with pytest.raises(ValueError, match='scales to an empty image'):
                letterbox_geometry((h, w), cfg)
        det, place = letterbox_plan(hw[ok], cfg)
        assert np.array_equal(place, want_place[ok]), (in_h, in_w)
        assert place[:, 0].min() >= 0 and (place[:, 0] + place[:, 2]).max() <= in_w and place[:, 1].min() >= 0 and (place[:, 1] + place[:, 3]).max() <= in_h
        params = np.array([letterbox_params(s, (in_h, in_w)) for s in hw[ok].tolist()]).astype(np.float32)
        assert same_bits(det[:, :3], params), (in_h, in_w)
        assert np.array_equal(det[:, 3], hw[ok][:, 1]) and np.array_equal(det[:, 4], hw[ok][:, 0])
        diff = (det[:, 1] != place[:, 0]) | (det[:, 2] != place[:, 1])
        assert (np.abs(det[:, 1] - place[:, 0]) <= 1).all() and (np.abs(det[:, 2] - place[:, 1]) <= 1).all()
        disagree += int(diff.sum())
        refused += int((~ok).sum())
        total += len(hw)
    assert (total, disagree, refused) == (796005, 119408, 3552)
    assert inexact_halves == [(48, 40, 352, w) for w in (55, 99, 187, 231)]


def test_letterbox_params_has_not_changed():
    assert letterbox_params((1080, 1920), (640, 640)) == (1 / 3, 0.0, 140.0) and letterbox_params((720, 1280), (384, 640)) == (0.5, 0.0, 12.0)
    assert letterbox_params((5, 7), (640, 640)) == (640 / 7, 0.0, 91.0) and letterbox_params((1, 6), (640, 640)) == (640 / 6, 0.0, 267.0)


def test_letterboxcfg_validation_and_the_python_refusals():
    d = LetterboxCfg()
    assert (d.input_hw, d.dtype, d.layout, d.order, d.pad_value, d.scaleup) == ((640, 640), 'fp16', 'nchw', 'rgb', 114, True)
    assert LetterboxCfg(320).input_hw == (320, 320) and LetterboxCfg([384, 640]).shape(2) == (2, 3, 384, 640) and LetterboxCfg((4, 5), layout='nhwc').shape(3) == (3, 4, 5, 3)
    c = c_config(LetterboxCfg((384, 640), 'u8', 'nhwc', 'bgr', 0, False))
    assert (c.in_h, c.in_w, c.dtype, c.layout, c.order, c.pad_value, c.scaleup) == (384, 640, 2, 1, 1, 0, 0)
    for bad in (dict(input_hw=(0, 640)), dict(input_hw=(640, 8193)), dict(input_hw=(640,)), dict(input_hw=(640.0, 640)), dict(input_hw=None), dict(input_hw=(True, 4)),
                dict(dtype='bf16'), dict(layout='chw'), dict(layout=0), dict(order='gbr'), dict(pad_value=-1), dict(pad_value=256), dict(pad_value=1.5), dict(scaleup=1)):
        with pytest.raises(ValueError, match='LetterboxCfg'):
            LetterboxCfg(**bad)
    with pytest.raises(TypeError, match='a LetterboxCfg expected'):
        c_config(dict())
    h = HostLetterbox(LetterboxCfg((16, 16)))
    with pytest.raises(ValueError, match='65 frames'):
        h.letterbox([rgb_frame(4, 4, 0)] * 65)
    with pytest.raises(TypeError, match='a Frame'):
        image_table([np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(ValueError, match='a frame of 0 x 5'):
        letterbox_geometry((0, 5), LetterboxCfg((16, 16)))
    with pytest.raises(ValueError, match='float32 \\[2, 5\\]'):
        det_image_table(np.zeros((2, 4), np.float32), None, 2)
    with pytest.raises(ValueError, match='float32 \\[1, 5\\]'):
        det_image_table(np.zeros((1, 5), np.float64), None, 1)
    tab = det_image_table(np.array([[0.5, 1, 2, 30, 40]], np.float32), None, 1)
    assert (tab[0].gain, tab[0].pad_x, tab[0].pad_y, tab[0].frame_w, tab[0].frame_h) == (0.5, 1, 2, 30, 40)


def test_refusals_of_the_c_entries():
    lib = capi.load_library()
    good = LetterboxCfg((16, 16))
    frames = [rgb_frame(9, 12, 1), nv12_frame(7, 5, 2)]
    images = image_table(frames)
    out = np.zeros(good.shape(2), np.float16)
    det, placement = np.zeros((2, 5), np.float32), np.zeros((2, 4), np.int32)

    def ptr(tab):
        return C.cast(tab.ctypes.data, C.POINTER(capi.vp_image))

    def call(cfg=None, tab=images, n=2, out_p=out.ctypes.data, host=True):
        c = c_config(good) if cfg is None else cfg
        args = [C.byref(c) if c is not False else None, ptr(tab) if tab is not None else None, n]
        tabs = [C.cast(det.ctypes.data, C.POINTER(capi.vp_det_image)), placement.ctypes.data]
        return lib.vp_dbg_letterbox_host(*args, out_p, *tabs) if host else lib.vp_letterbox_plan(*args, *tabs)

    def refused(why, host_only=False, **kw):
        for host in ((True,) if host_only else (True, False)):
            assert call(host=host, **kw) == capi.VP_ERR_INVALID, why
            assert capi.last_error().startswith('letterbox: ') and why in capi.last_error(), (why, capi.last_error())

    assert call() == capi.VP_OK and call(host=False) == capi.VP_OK
    assert call(n=0, tab=None, out_p=None) == capi.VP_OK and call(n=0, tab=None, host=False) == capi.VP_OK, 'n_images = 0 is legal'
    assert lib.vp_dbg_letterbox_host(C.byref(c_config(good)), ptr(images), 2, out.ctypes.data, None, None) == capi.VP_OK, 'det and placement may be NULL'
    filled = (det.copy(), placement.copy())
    assert filled[0][:, 0].min() > 0 and filled[1][:, 2].min() > 0
    det[:], placement[:] = -5, -5   # every refusal below leaves the two tables as they are: checked at the end

    def cfg_with(**kw):
        c = c_config(good)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    refused('null cfg', cfg=False)
    refused('input 0 x 16', cfg=cfg_with(in_h=0))
    refused('input 16 x 8193', cfg=cfg_with(in_w=8193))
    refused('dtype = 3', cfg=cfg_with(dtype=3))
    refused('dtype = -1', cfg=cfg_with(dtype=-1))
    refused('layout = 2', cfg=cfg_with(layout=2))
    refused('order = 2', cfg=cfg_with(order=2))
    refused('pad_value = 256', cfg=cfg_with(pad_value=256))
    refused('pad_value = -1', cfg=cfg_with(pad_value=-1))
    refused('scaleup = 2', cfg=cfg_with(scaleup=2))
    refused('n_images = 65', n=65)
    refused('n_images = -1', n=-1)
    refused('null images', tab=None)
    refused('null output', host_only=True, out_p=None)
    refused('not aligned', host_only=True, out_p=out.ctypes.data + 1)

    def image_with(i, **kw):
        t = images.copy()
        for k, v in kw.items():
            t[k][i] = v
        return t

    refused('frame 0 has a non-positive size 0 x 12', tab=image_with(0, h=0))
    refused('frame 1 has a non-positive size 7 x -1', tab=image_with(1, w=-1))
    refused('frame 0 has an unknown pixel format 3', tab=image_with(0, format=3))
    refused('frame 1 has an unknown YUV matrix 3', tab=image_with(1, matrix=3))
    refused('frame 0 has a negative pitch', tab=image_with(0, pitch=(-36, 0)))
    refused('frame 0 has pitch[0] 35 below its 36 row bytes', tab=image_with(0, pitch=(35, 0)))
    refused('frame 1 is NV12 without a UV plane', tab=image_with(1, plane=(images['plane'][1, 0], 0)))
    refused('frame 1 has pitch[1] 5 below the 6 bytes of a UV row', tab=image_with(1, pitch=(5, 5)))
    refused('frame 0 has no data', host_only=True, tab=image_with(0, plane=(0, 0)))
    assert (det == -5).all() and (placement == -5).all()
    assert call(tab=image_with(0, plane=(0, 0)), host=False) == capi.VP_OK, 'the plan reads sizes and layout only'
    det[:], placement[:] = -5, -5
    refused('frame 1 of 1280 x 1 scales to an empty image in 16 x 16', tab=image_with(1, h=1280, w=1, format=0, pitch=(3, 0)))
    big = np.zeros(1, IMAGE_DTYPE)
    big['h'], big['w'], big['pitch'] = 1280, 1, (3, 0)
    c640 = c_config(LetterboxCfg((640, 640)))
    assert lib.vp_letterbox_plan(C.byref(c640), ptr(big), 1, None, None) == capi.VP_ERR_INVALID and '1280 x 1 scales to an empty image in 640 x 640' in capi.last_error()
    assert (det == -5).all() and (placement == -5).all(), 'a refused call writes neither table, not even the rows of the frames in front of the refused one'
    assert call(tab=image_with(0, plane=(0, 0)), host=False) == capi.VP_OK and same_bits(det, filled[0]) and same_bits(placement, filled[1])
    # the handle entries refuse a missing handle before anything else
    assert lib.vp_letterbox_stream(None, C.byref(c640), ptr(big), 1, None, None, None, None) == capi.VP_ERR_INVALID
    assert lib.vp_letterbox(None, C.byref(c640), ptr(big), 1, None, None, None) == capi.VP_ERR_INVALID


def test_pitched_views_leave_the_parent_alone():
    cfg, frames = CASES['pitched']
    parents = [p.base if p.base is not None else p for f in frames for p in f.planes]
    before = [np.array(b, copy=True) for b in parents]
    out = HostLetterbox(cfg).letterbox(frames)[0]
    dense = [Frame(f.format, tuple(np.ascontiguousarray(p) for p in f.planes), f.matrix) for f in frames]
    assert all(f.pitch[0] > d.pitch[0] for f, d in zip(frames, dense))
    assert same_bits(out, HostLetterbox(cfg).letterbox(dense)[0])
    assert all(np.array_equal(a, b) for a, b in zip(before, parents)) and all((np.asarray(b) == CANARY).any() for b in parents)


# ---- the Python routes against a fake engine: the host taps stand in for the device stages, everything else is the product's code
class FakeLetterbox:
    """DeviceLetterbox's interface over the host tap"""

    def __init__(self, cfg, log):
        self.cfg, self.log, self.host = cfg, log, HostLetterbox(cfg)

    def upload(self, img):
        self.log.append(('upload', img.shape))
        return Frame.rgb(np.ascontiguousarray(img))

    def letterbox(self, frames, out=None, stream=None):
        tensor, table, placement = self.host.letterbox(frames)
        self.log.append(('letterbox', tensor.shape, table.copy()))
        return tensor, table, placement


class FakeDetector:
    """DeviceDetector's interface over the host tap"""

    def __init__(self, cfg, log):
        self.cfg, self.log, self.host = cfg, log, HostDetector(cfg)

    def detect_host(self, pred, frames_hw, input_hw=None, n_out=None):
        self.log.append(('detect', pred.shape, np.array(frames_hw, copy=True), input_hw))
        return self.host.detect(pred, frames_hw, input_hw, n_out)


def person_head(box, table, nc=80, A=50):
    """an fp16 head [4 + nc, A] holding `box` (frame pixels) as class 0 in the letterboxed input that `table` undoes"""
    gain, px, py = (float(v) for v in table[0, :3])
    p = np.zeros((4 + nc, A), np.float32)
    p[:4] = 5
    x1, y1, x2, y2 = box[0] * gain + px, box[1] * gain + py, box[2] * gain + px, box[3] * gain + py
    p[:4, 7] = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1)
    p[4, 7] = 0.9
    return p.astype(np.float16)


def test_vitinference_letterbox_route_against_a_fake_engine():
    from easy_vitpose_amd.inference import VitInference
    lcfg, dcfg = LetterboxCfg((64, 96)), DetectCfg(classes='human', max_images=1)
    log = []
    seen = {}

    def engine(tensor):
        log.append(('engine', tensor.shape, tensor.dtype))
        seen['tensor'] = tensor
        return person_head((20, 10, 60, 70), log[-2][2])

    m = VitInference.__new__(VitInference)   # the stages are what the constructor would build on the device
    m.yolo, m._letterbox, m._detector = engine, FakeLetterbox(lcfg, log), FakeDetector(dcfg, log)
    img = to_rgb(rgb_frame(97, 131, 5))
    rows = m._letterbox_rows(img)
    assert [e[0] for e in log] == ['upload', 'letterbox', 'engine', 'detect'], 'frame up, letterbox, the engine on the tensor, the detector stage'
    assert log[0][1] == (97, 131, 3) and log[1][1] == (1, 3, 64, 96) and log[2][1:] == ((1, 3, 64, 96), np.float16) and log[3][1] == (1, 84, 50)
    want_tensor, want_row, _ = letterbox_host_numpy(img, lcfg)
    assert same_bits(seen['tensor'][0], want_tensor)
    assert log[3][3] is None and same_bits(log[3][2], log[1][2]) and same_bits(log[3][2][0], want_row), "the detector stage got the letterbox stage's own table"
    assert rows.shape == (1, 5) and np.abs(rows[0, :4] - np.array([20, 10, 60, 70])).max() < 1.0 and rows[0, 4] > 0.35
    with pytest.raises(TypeError, match='letterbox: None or a LetterboxCfg'):
        VitInference({}, engine, dataset='coco', detect=dcfg, letterbox=dict())
    with pytest.raises(ValueError, match='give detect='):
        VitInference({}, engine, dataset='coco', letterbox=lcfg)


def test_cli_det_engine_argument_and_main(monkeypatch):
    from easy_vitpose_amd import cli
    calls = []
    mod = types.ModuleType('fake_det_engine')

    def make():
        def engine(tensor):
            calls.append(tuple(tensor.shape))
            return np.zeros((7, 10), np.float32)
        engine.nc, engine.head_dtype = 3, 'fp32'
        return engine
    mod.make, mod.not_a_factory = make, (lambda: 5)
    monkeypatch.setitem(sys.modules, 'fake_det_engine', mod)
    base = ['--input', 'x.npy', '--synthetic', 's']
    engine, detect, letterbox = cli.det_engine_argument(cli.build_parser().parse_args(base + ['--det-engine', 'fake_det_engine:make', '--det-input', '384', '640']))
    assert (letterbox.input_hw, letterbox.dtype, letterbox.layout, letterbox.order) == ((384, 640), 'fp16', 'nchw', 'rgb')
    assert (detect.nc, detect.dtype, detect.classes, detect.max_images) == (3, 'fp32', (0, 1, 2), 1) and callable(engine)
    args = cli.build_parser().parse_args(base + ['--det-engine', 'fake_det_engine:make', '--det-input-dtype', 'fp32', '--det-conf', '0.5'])
    engine, detect, letterbox = cli.det_engine_argument(args)
    assert letterbox.dtype == 'fp32' and letterbox.input_hw == (640, 640) and detect.conf_thr == 0.5
    for extra in (['--yolo', 'y.pt'], ['--boxes', 'b.json'], ['--det-heads', 'h.npz']):
        with pytest.raises(ValueError, match='--det-engine replaces --yolo / --boxes / --det-heads'):
            cli.det_engine_argument(cli.build_parser().parse_args(base + ['--det-engine', 'fake_det_engine:make'] + extra))
        with pytest.raises(ValueError, match='--det-engine replaces --yolo / --boxes / --det-heads'):
            cli.main(base + ['--det-engine', 'fake_det_engine:make'] + extra)
    with pytest.raises(ValueError, match='MODULE:FACTORY'):
        cli.det_engine_argument(cli.build_parser().parse_args(base + ['--det-engine', 'fake_det_engine']))
    with pytest.raises(TypeError, match='not a callable'):
        cli.det_engine_argument(cli.build_parser().parse_args(base + ['--det-engine', 'fake_det_engine:not_a_factory']))

    # main(): the model it builds gets the engine as its detector, detect= and letterbox=
    built = {}

    class FakeModel:
        dataset = 'coco'

        def __init__(self, model, yolo, *a, **kw):
            built.update(yolo=yolo, detect=kw.get('detect'), letterbox=kw.get('letterbox'))
            self._vit_pose = types.SimpleNamespace(K=17)

        def inference_frames(self, batch):
            if built['letterbox'] is not None:
                built['yolo'](np.zeros((1, 3) + built['letterbox'].input_hw, np.float16))
            return [{} for _ in batch]

    import easy_vitpose_amd
    monkeypatch.setattr(easy_vitpose_amd, 'VitInference', FakeModel)
    monkeypatch.setattr(cli, '_read_frames', lambda path, rotate: ([np.zeros((8, 8, 3), np.uint8)] * 2, True))
    assert cli.main(base + ['--det-engine', 'fake_det_engine:make', '--det-input', '32', '48']) == 0
    assert built['letterbox'] == LetterboxCfg((32, 48)) and built['detect'].nc == 3 and calls == [(1, 3, 32, 48)] * 2
    built.clear()
    monkeypatch.setattr(cli, 'detect_argument', lambda args: ([np.zeros((7, 10), np.float32)], DetectCfg(nc=3, dtype='fp32')))
    assert cli.main(base + ['--det-heads', 'h.npz']) == 0 and built['letterbox'] is None, 'without --det-engine nothing changes'
    with pytest.raises(AssertionError, match='--det-input-dtype belongs to --det-engine'):
        cli.main(base + ['--det-heads', 'h.npz', '--det-input-dtype', 'fp32'])


def test_device_letterbox_refusals_that_come_before_any_device_call():
    """the engine is a stand-in without a library: a call that got past its refusal would fail on it in another way.  The refusals that need a device tensor
    (another device, `out`, a device frame given to letterbox_host) are in tests/test_gpu_letterbox.py."""
    dev = DeviceLetterbox(types.SimpleNamespace(lib=None, device_id=0, _h=None), LetterboxCfg((16, 16)))
    with pytest.raises(ValueError, match='letterbox: 65 frames, a call takes 64'):
        dev.letterbox_host([rgb_frame(4, 4, 0)] * 65)
    with pytest.raises(ValueError, match='letterbox: 65 frames, a call takes 64'):
        dev.letterbox([rgb_frame(4, 4, 0)] * 65)
    with pytest.raises(TypeError, match='frame 0: torch uint8 CUDA tensors expected'):
        dev.letterbox([rgb_frame(4, 4, 0)])
    with pytest.raises(TypeError, match='frame 0: torch uint8 CUDA tensors expected'):
        dev.letterbox([nv12_frame(5, 4, 1), rgb_frame(4, 4, 0)])
