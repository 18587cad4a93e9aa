"""CPU: the detector stage of csrc/detgeom.h through the host tap vp_dbg_detect_host -- the same functions the kernels of vp_detect_stream run -- against the
reference's own box NMS (tests/golden/detect_nms.npz), against a numpy twin written from the contract (tests/detect_cases.py), every refusal of the C entries
and of the Python layer, and the letterbox geometry.  The device is compared with this host model in tests/test_gpu_detect.py."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.devdetect import (FLAG_BAD_BOX, FLAG_CAND, FLAG_ROWS, MAX_CAND, MAX_CLASSES, MAX_DET, MAX_IMAGES, DetectCfg, HostDetector, c_config, image_table,
                                        letterbox_params)
from detect_cases import SIZES, named_cases, same_bits, size_case, size_id, twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rows', 'image', 'anchor', 'count', 'flags')
CASES = named_cases()


def tap(case):
    cfg, pred, frames_hw, input_hw, n_out = case
    return HostDetector(cfg).detect(pred, frames_hw, input_hw, n_out)


def test_surface_symbols_macros_and_build_flags():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    for name in ('vp_detector_create', 'vp_detector_destroy', 'vp_detect_stream', 'vp_detect', 'vp_dbg_detect_host', 'vp_tracker_update_counted_stream'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r'VP_API\s+int\s+' + name + r'\s*\(', hdr), name
    assert re.search(r'#define\s+VP_HAS_DETECT\s+1\b', hdr)
    for macro, value in (('VP_DET_MAX_IMAGES', MAX_IMAGES), ('VP_DET_MAX_CLASSES', MAX_CLASSES), ('VP_DET_MAX_CAND', MAX_CAND), ('VP_DET_MAX_DET', MAX_DET)):
        assert re.search(r'#define\s+%s\s+%d\b' % (macro, value), hdr), macro
    assert (MAX_IMAGES, MAX_CLASSES, MAX_CAND, MAX_DET) == (64, 256, 2048, 1024)
    assert C.sizeof(capi.vp_det_cfg) == 72 and C.sizeof(capi.vp_det_image) == 20
    build = __import__('easy_vitpose_amd.build', fromlist=['SOURCES'])
    assert 'detect.hip' in build.SOURCES and build.SOURCE_FLAGS['detect.hip'] == ['-ffp-contract=off'] and 'detgeom.h' in build.HEADERS
    assert lib.vp_abi_version() == 4


def test_host_tap_reproduces_the_reference_nms(golden_dir):
    """The reference's `nms` (pixel convention: extent 1, class-agnostic) on float32 rows: every keep list exactly, order included, and the kept boxes bit for
    bit, through the real head format ([1, 5, n]: cx, cy, w, h, score).  No case is left out and no margin is taken around the threshold."""
    g = np.load(os.path.join(golden_dir, 'detect_nms.npz'))
    assert g['sizes'].tolist() == [1, 2, 7, 33, 70, 300] and g['thrs'].tolist() == [0.3, 0.5, 0.7]
    suppressed = 0
    for n in g['sizes']:
        dets = g[f'n{n}_dets']
        assert dets.dtype == np.float32 and dets.shape == (n, 5)
        x1, y1, x2, y2, s = dets.T
        pred = np.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, s])[None]
        assert pred.dtype == np.float32
        assert np.array_equal(pred[0, 0] - pred[0, 2] * np.float32(0.5), x1) and np.array_equal(pred[0, 1] + pred[0, 3] * np.float32(0.5), y2)
        for ti, thr in enumerate(g['thrs']):
            keep = g[f'n{n}_t{ti}_keep']
            cfg = DetectCfg(nc=1, dtype='fp32', conf_thr=0.0, iou_thr=thr, extent=1.0, agnostic=True, max_det=1024)
            rows, image, anchor, count, flags = HostDetector(cfg).detect(pred, (1024, 1024), (1024, 1024))
            m = int(count[-1])
            assert m == len(keep) and anchor[:m].tolist() == keep.tolist(), (n, thr)
            assert same_bits(rows[:m, :5], dets[keep]) and (rows[:m, 5] == 0).all() and flags.tolist() == [0], (n, thr)
            suppressed += n - m
    assert suppressed > 300, 'the goldens exercise the suppression'


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_tap_equals_the_numpy_twin(name):
    got, want = tap(CASES[name]), twin(*CASES[name])
    for what, a, b in zip(NAMES, got, want):
        assert same_bits(a, b), f'{what} differs\n{a}\n{b}'


@pytest.mark.parametrize('i', range(len(SIZES)), ids=[size_id(s) for s in SIZES])
def test_host_tap_equals_the_numpy_twin_on_the_kernel_sizes(i):
    case = size_case(i)
    got, want = tap(case), twin(*case)
    for what, a, b in zip(NAMES, got, want):
        assert same_bits(a, b), f'{what} differs'
    cand = SIZES[i][1]
    assert [bool(f & FLAG_CAND) for f in got[4]] == [c > MAX_CAND for c in cand]
    assert all(got[3][k] == 0 for k, c in enumerate(cand) if c > MAX_CAND or c == 0) and all(got[3][k] > 0 for k, c in enumerate(cand) if 0 < c <= MAX_CAND)


def test_what_the_named_cases_show():
    out = {name: tap(CASES[name]) for name in CASES}
    rows, image, anchor, count, flags = out['class_mask']
    assert anchor[:count[-1]].tolist() == [1], 'a person box that a masked class out-scores is no candidate'
    for dtype in ('fp16', 'fp32'):
        rows, image, anchor, count, flags = out[f'class_tie_{dtype}']
        assert anchor[:count[-1]].tolist() == [0] and rows[0, 5] == 0, 'the first class of a tie wins'
    for key in ('nan_inf_l0_fp16', 'nan_inf_l1_fp32'):
        rows, image, anchor, count, flags = out[key]
        assert flags.tolist() == [FLAG_BAD_BOX, FLAG_BAD_BOX] and count.tolist() == [2, 1, 3]
        assert anchor[:3].tolist() == [2, 0, 7] and np.isinf(rows[0, 4]) and rows[:3, 5].tolist() == [1, 1, 2]
    rows, image, anchor, count, flags = out['score_at_thr']
    assert anchor[:count[-1]].tolist() == [1]
    rows, image, anchor, count, flags = out['iou_at_thr']
    assert anchor[:count[-1]].tolist() == [0, 1], 'an IoU equal to the threshold is kept, the next one up is suppressed'
    assert out['agnostic_0'][2][:3].tolist() == [0, 1, 3] and out['agnostic_1'][2][:2].tolist() == [0, 3] and out['agnostic_1'][3].tolist() == [2, 2]
    rows, image, anchor, count, flags = out['max_det_cut']
    assert anchor.tolist() == [9, 8, 7] and count.tolist() == [3, 3] and flags.tolist() == [0]
    rows, image, anchor, count, flags = out['n_out_cut']
    assert count.tolist() == [3, 3, 3, 9] and flags.tolist() == [0, FLAG_ROWS, FLAG_ROWS] and image.tolist() == [0, 0, 0, 1] and len(rows) == 4
    rows, image, anchor, count, flags = out['n_out_zero']
    assert count.tolist() == [3, 3, 3, 9] and flags.tolist() == [FLAG_ROWS] * 3 and len(rows) == 0
    rows, image, anchor, count, flags = out['cand_cap']
    assert flags.tolist() == [FLAG_CAND, 0] and count[0] == 0 and 0 < count[1] == count[2] <= 1024 and (image[:count[2]] == 1).all()
    rows, image, anchor, count, flags = out['letterbox_640']
    assert count[-1] == 6 and flags.tolist() == [0]
    byanchor = {int(a): r for a, r in zip(anchor[:6], rows[:6])}
    assert byanchor[0][0] == 0 and byanchor[1][2] == 1920 and byanchor[2][1] == 0 and byanchor[3][3] == 1080, 'clipped at the four frame edges'
    assert byanchor[5][1] == 0 and byanchor[5][3] == 0
    want = (np.array([250.25, 260.5, 291.75, 333.25], np.float32) - np.array([0, 140, 0, 140], np.float32)) / np.float32(1 / 3)
    assert same_bits(byanchor[4][:4], want)
    rows, image, anchor, count, flags = out['empty_between']
    assert count[0] > 0 and count[1] == 0 and count[2] > 0 and sorted(set(image[:count[-1]].tolist())) == [0, 2]
    absent = slice(int(count[-1]), None)
    assert np.isnan(rows[absent, :4]).all() and (rows[absent, 4] == 0).all() and (rows[absent, 5] == -1).all() and (image[absent] == -1).all() and (anchor[absent] == -1).all()


def test_letterbox_params_against_hand_computed_values():
    assert letterbox_params((1080, 1920), (640, 640)) == (1 / 3, 0.0, 140.0)       # round((640 - 360) / 2 - 0.1) = round(139.9)
    assert letterbox_params((1080, 1920), (320, 320)) == (1 / 6, 0.0, 70.0)
    assert letterbox_params((1920, 1080), (640, 640)) == (1 / 3, 140.0, 0.0)
    assert letterbox_params((480, 640), (640, 640)) == (1.0, 0.0, 80.0)
    assert letterbox_params((720, 1280), (384, 640)) == (0.5, 0.0, 12.0)
    assert letterbox_params((100, 333), (640, 640)) == (640 / 333, 0.0, round((640 - 100 * (640 / 333)) / 2 - 0.1))
    assert letterbox_params((1024, 1024), (1024, 1024)) == (1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        letterbox_params((0, 10), (640, 640))
    tab = image_table([(1080, 1920), (480, 640)], (640, 640), 2)
    assert (tab[0].gain, tab[0].pad_x, tab[0].pad_y, tab[0].frame_w, tab[0].frame_h) == (np.float32(1 / 3), 0, 140, 1920, 1080)
    assert (tab[1].gain, tab[1].pad_y, tab[1].frame_w, tab[1].frame_h) == (1, 80, 640, 480)
    with pytest.raises(ValueError):
        image_table([(1, 2)] * 3, (640, 640), 2)


def test_detectcfg_validation():
    d = DetectCfg()
    assert (d.conf_thr, d.iou_thr, d.extent, d.agnostic, d.max_det, d.nc) == (float(np.float32(0.35)), float(np.float32(0.7)), 0.0, False, 300, 80)
    assert d.classes == tuple(range(80)) and DetectCfg(classes='human').classes == (0,) and DetectCfg(classes='animals').classes == tuple(range(15, 24))
    assert DetectCfg(classes=[5, 3, 5]).classes == (3, 5)
    m = c_config(DetectCfg(nc=40, classes=[0, 33])).class_mask
    assert list(m) == [1, 2, 0, 0, 0, 0, 0, 0]
    for bad in (dict(nc=0), dict(nc=257), dict(nc=True), dict(dtype='bf16'), dict(layout=2), dict(conf_thr=-0.1), dict(conf_thr=float('nan')), dict(conf_thr=float('inf')),
                dict(iou_thr=1.5), dict(iou_thr=-0.1), dict(iou_thr=float('nan')), dict(extent=-1.0), dict(extent=float('inf')), dict(agnostic=1), dict(max_det=0),
                dict(max_det=1025), dict(max_det=2.5), dict(classes=[]), dict(classes=[80]), dict(classes=[-1]), dict(classes='unicorn'), dict(classes=[0.5]),
                dict(max_anchors=0), dict(max_anchors=(1 << 20) + 1), dict(max_images=0), dict(max_images=65)):
        with pytest.raises(ValueError):
            DetectCfg(**bad)
    with pytest.raises(TypeError):
        c_config(dict())
    h = HostDetector(DetectCfg(nc=2, dtype='fp32', max_images=2, max_anchors=16))
    for pred in (np.zeros((1, 5, 4), np.float32), np.zeros((3, 6, 4), np.float32), np.zeros((1, 6, 17), np.float32), np.zeros((1, 6, 0), np.float32), np.zeros((6, 4), np.float32)):
        with pytest.raises(ValueError):
            h.detect(pred, (10, 10), (10, 10))
    with pytest.raises(TypeError):
        h.detect(np.zeros((1, 6, 4), np.float16), (10, 10), (10, 10))


def test_cli_det_heads_argument(tmp_path):
    from easy_vitpose_amd.cli import build_parser, detect_argument
    stack = np.zeros((3, 84, 100), np.float16)
    np.savez(tmp_path / 'stack.npz', heads=stack)
    np.savez(tmp_path / 'frames.npz', f000=np.zeros((7, 50), np.float32), f001=np.ones((7, 50), np.float32))
    np.savez(tmp_path / 'bad.npz', a=np.zeros((7, 50), np.float32), b=np.ones((7, 51), np.float32))
    base = ['--input', 'x.npy', '--synthetic', 's']
    args = build_parser().parse_args(base + ['--det-heads', str(tmp_path / 'stack.npz')])
    heads, cfg = detect_argument(args)
    assert len(heads) == 3 and heads[0].shape == (84, 100) and args.det_input == [640, 640]
    assert (cfg.nc, cfg.dtype, cfg.classes, cfg.conf_thr, cfg.iou_thr, cfg.max_anchors) == (80, 'fp16', (0,), float(np.float32(0.35)), float(np.float32(0.7)), 100)
    args = build_parser().parse_args(base + ['--det-heads', str(tmp_path / 'frames.npz'), '--det-input', '384', '640', '--det-conf', '0.5', '--det-iou', '0.45'])
    heads, cfg = detect_argument(args)
    assert len(heads) == 2 and heads[1][0, 0] == 1 and args.det_input == [384, 640]
    assert (cfg.nc, cfg.dtype, cfg.classes, cfg.conf_thr, cfg.iou_thr) == (3, 'fp32', (0, 1, 2), 0.5, float(np.float32(0.45)))
    with pytest.raises(ValueError):
        detect_argument(build_parser().parse_args(base + ['--det-heads', str(tmp_path / 'bad.npz')]))


def test_refusals_of_the_c_entry():
    lib = capi.load_library()
    good = DetectCfg(nc=2, dtype='fp32', max_images=2, max_anchors=16)
    pred = np.zeros((2, 6, 8), np.float32)
    rows, image, anchor, count, flags = np.zeros((4, 6), np.float32), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(3, np.int32), np.zeros(2, np.int32)
    tab = image_table((10, 10), (10, 10), 2)

    def call(cfg=None, pred_p=pred.ctypes.data, A=8, images=tab, n=2, rows_p=rows.ctypes.data, image_p=image.ctypes.data, anchor_p=anchor.ctypes.data, n_out=4,
             count_p=count.ctypes.data):
        c = c_config(good) if cfg is None else cfg
        return lib.vp_dbg_detect_host(C.byref(c) if c is not False else None, pred_p, A, images, n, rows_p, image_p, anchor_p, n_out, count_p, flags.ctypes.data)

    def refused(why, **kw):
        assert call(**kw) == capi.VP_ERR_INVALID, why
        assert capi.last_error().startswith('detector: ') and why in capi.last_error(), (why, capi.last_error())

    assert call() == capi.VP_OK and call(n=0, pred_p=None, images=None) == capi.VP_OK and count.tolist()[0] == 0

    def cfg_with(**kw):
        c = c_config(good)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    refused('null cfg', cfg=False)
    refused('nc = 0', cfg=cfg_with(nc=0))
    refused('nc = 257', cfg=cfg_with(nc=257))
    refused('max_anchors', cfg=cfg_with(max_anchors=0))
    refused('max_anchors', cfg=cfg_with(max_anchors=(1 << 20) + 1))
    refused('max_images', cfg=cfg_with(max_images=65))
    refused('dtype', cfg=cfg_with(dtype=2))
    refused('layout', cfg=cfg_with(layout=-1))
    refused('conf_thr', cfg=cfg_with(conf_thr=float('nan')))
    refused('conf_thr', cfg=cfg_with(conf_thr=-1.0))
    refused('iou_thr', cfg=cfg_with(iou_thr=float('nan')))
    refused('iou_thr', cfg=cfg_with(iou_thr=1.25))
    refused('extent', cfg=cfg_with(extent=-1.0))
    refused('agnostic', cfg=cfg_with(agnostic=2))
    refused('max_det = 0', cfg=cfg_with(max_det=0))
    refused('max_det = 1025', cfg=cfg_with(max_det=1025))
    refused('class_mask', cfg=cfg_with(class_mask=(C.c_uint32 * 8)(4, 0, 0, 0, 0, 0, 0, 0)))
    refused('n_images = 3', n=3)
    refused('n_images = -1', n=-1)
    refused('negative n_out', n_out=-1)
    refused('A = 0', A=0)
    refused('A = 17', A=17)
    refused('null count', count_p=None)
    refused('null rows', rows_p=None)
    refused('null rows', anchor_p=None)
    refused('null pred', pred_p=None)
    refused('null images', images=None)
    refused('aligned', pred_p=pred.ctypes.data + 2)
    assert call(rows_p=None, image_p=None, anchor_p=None, n_out=0) == capi.VP_OK
    for field, value, why in (('gain', 0.0, 'gain'), ('gain', float('nan'), 'gain'), ('pad_x', float('inf'), 'pad'), ('frame_h', -1.0, 'frame size'),
                              ('frame_w', float('nan'), 'frame size')):
        t = image_table((10, 10), (10, 10), 2)
        setattr(t[1], field, value)
        refused('image 1: ' + why, images=t)
    assert dataclasses.is_dataclass(good)
