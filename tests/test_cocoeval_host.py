"""CPU: the COCO keypoint evaluator's contract (csrc/cocogeom.h) through the host taps vp_dbg_cocoeval_update_host / vp_dbg_cocoeval_accumulate_host -- against the
numpy twin (a transcription of COCOeval's loops) on every byte of the state, of the result blob and of `match`, and against anchors written as literals.  The device
is tested against these taps in tests/test_gpu_cocoeval.py; the margin condition that comparison rests on is asserted here for every case."""
from __future__ import annotations

import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd import build
from easy_vitpose_amd import devcoco as dc
from easy_vitpose_amd.devcoco import (CocoEvalCfg, cocoeval_numpy_accumulate, cocoeval_numpy_update, cocoeval_tap, cocoeval_tap_accumulate, finish, new_state)
import cocoeval_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['vp_cocoeval_create', 'vp_cocoeval_destroy', 'vp_cocoeval_reset_stream', 'vp_cocoeval_update_stream', 'vp_cocoeval_update', 'vp_cocoeval_accumulate_stream',
       'vp_cocoeval_accumulate', 'vp_cocoeval_state_bytes', 'vp_cocoeval_result_bytes', 'vp_cocoeval_download_state', 'vp_dbg_cocoeval_update_host',
       'vp_dbg_cocoeval_accumulate_host']
CASES = cc.host_cases()
F32, F64, I32 = np.float32, np.float64, np.int32
EPS = 2.0 ** -52


def test_surface():
    lib = capi.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes and re.search(r'VP_API int %s\(' % name, hdr), name
    assert re.search(r'#define\s+VP_HAS_COCOEVAL\s+1\b', hdr) and re.search(r'#define\s+VP_ABI_VERSION\s+4\b', hdr) and lib.vp_abi_version() == 4
    assert C.sizeof(capi.vp_cocoeval_cfg) == 16
    assert 'cocoeval.hip' in build.SOURCES and build.SOURCE_FLAGS['cocoeval.hip'] == ['-ffp-contract=off'] and 'cocogeom.h' in build.HEADERS
    assert dc.state_bytes(CocoEvalCfg(17, 5)) == 128 + 16 * 5 and dc.RESULT.itemsize == 128 + 8 * 3060 and dc.RECORD.itemsize == 16


def test_the_threshold_tables_equal_numpy_linspace_bit_for_bit():
    assert dc.OKS_THRS.tobytes() == np.linspace(.5, .95, 10).tobytes() and dc.OKS_THRS[8] == 0.8999999999999999
    assert dc.REC_THRS.tobytes() == np.linspace(0, 1, 101).tobytes()
    assert (np.arange(101) / 100.0).tobytes() != dc.REC_THRS.tobytes()   # why the contract writes k * (1.0 / 100.0)
    # the C++ tables, read through an accumulate: one gt, detections at OKS just above a threshold ... the literal anchors below pin them through their outcomes


def run(cs):
    """every call of a case through the tap and the twin -> (tap state, twin state)"""
    a, b = new_state(cs['cfg']), new_state(cs['cfg'])
    for i, call in enumerate(cs['calls']):
        ma = cocoeval_tap(a, cs['cfg'], **cc.inputs(call))
        mb = cocoeval_numpy_update(b, cs['cfg'], **cc.inputs(call))
        assert ma.tobytes() == mb.tobytes(), f'match of call {i}'
    return a, b


@pytest.mark.parametrize('name', sorted(CASES))
def test_tap_equals_the_numpy_twin_on_every_byte(name):
    cs = CASES[name]
    a, b = run(cs)
    for f in a.dtype.names:
        assert a[f].tobytes() == b[f].tobytes(), f'{name}: state field {f}'
    ra, rb = cocoeval_tap_accumulate(a, cs['cfg']), cocoeval_numpy_accumulate(b)
    for f in ra.dtype.names:
        assert ra[f].tobytes() == rb[f].tobytes(), f'{name}: result field {f}'
    assert int(a['calls']) == len(cs['calls']) and int(a['kept']) == int(a['records']) + int(a['dropped'])
    if name.startswith('total_'):
        assert int(a['records']) == int(name.split('_')[1]) and int(a['dropped']) == 0
    if name == 'one_short':
        assert int(a['records']) == 64 and int(a['dropped']) == 1
        with pytest.raises(RuntimeError, match='did not fit'):
            finish(ra)
    if name == 'dets_and_gts_per_image':
        assert int(a['gt_overflow']) == 1 and int(a['gts']) == 1 + 2 + 64 + 128 + 128 and int(a['kept']) == 1 + 19 + 20 + 20 + 20
    if name == 'nonfinite':
        assert int(a['nonfinite']) > 0
    if name == 'frames_256':
        assert int(a['images']) == 256 and (a['table']['image'][:int(a['records'])] < 256).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_margin_condition(name):
    """no finite OKS within 1e-9 of a threshold; two OKS values a detection could take are equal by construction or 1e-9 apart"""
    thr_gap, pair_gap = cc.margins(CASES[name])
    assert thr_gap >= cc.MARGIN and pair_gap >= cc.MARGIN, (name, thr_gap, pair_gap)


def test_the_rules_case_reaches_every_rule():
    cs = CASES['rules']
    call = cs['calls'][0]
    st = new_state(cs['cfg'])
    m = cocoeval_tap(st, cs['cfg'], **cc.inputs(call))
    rec = st['table'][:int(st['records'])]
    by_image = lambda i: rec[rec['image'] == i]
    ALL = np.uint32((1 << 30) - 1)
    # 0: the crowd takes both detections while their OKS reaches the threshold; they are ignored, the third is a false positive
    r = by_image(0)
    assert r['matched'][0] & 0x3ff == 0x0ff and r['matched'][1] & 0x3ff == 0x03f and r['matched'][2] == 0
    assert r['ignored'][0] & 0x3ff == 0x0ff and r['ignored'][2] & 0x3ff == 0
    assert m[0, 0] == 0 and m[1, 0] == 0 and m[2, 0] == -1
    # 1: inside the doubled box the OKS is exactly 1: matched at every threshold, and ignored because the gt has no labelled joint
    r = by_image(1)
    assert r['matched'][0] == ALL and r['ignored'][0] == ALL and r['matched'][1] == 0
    # 2: up to 0.70 the not-ignored gt (row 3, oks 0.72) is taken and the walk stops at the crowd although its oks is 0.93; above, the not-ignored one is
    #    out of reach and the crowd (row 2) is taken up to 0.90
    assert list(m[5]) == [3, 3, 3, 3, 3, 2, 2, 2, 2, -1]
    # 3: the not-ignored gt (row 5) at 0.88 wins over the crowd (row 4) at 0.62; the other detection reaches only the crowd
    assert list(m[6]) == [5] * 8 + [-1, -1] and list(m[7]) == [4] * 6 + [-1] * 4
    # 4: a tie goes to the later gt of the walk (`oks < best` skips, equality takes), the next detection takes the one left, the third finds none
    assert list(m[8]) == [7] * 10 and list(m[9]) == [6] * 10 and list(m[10]) == [-1] * 10 and list(m[11]) == [8] * 10
    # 5: area 96^2 is inside medium and large; one float32 step above is outside medium
    r = by_image(5)
    #    (detection 0 matches up to 0.85, detection 1 up to 0.75; unmatched, their own area 60 x 80 decides: inside medium, outside large)
    assert r['matched'][0] == 0x0ff | 0x0ff << 10 | 0x0ff << 20 and r['matched'][1] == 0x03f | 0x03f << 10 | 0x03f << 20
    assert (r['ignored'][0] >> 10) & 0x3ff == 0 and (r['ignored'][0] >> 20) & 0x3ff == 0x300
    assert (r['ignored'][1] >> 10) & 0x3ff == 0x03f and (r['ignored'][1] >> 20) & 0x3ff == 0x3c0
    assert list(st['npig']) == [7, 5, 3]


def test_the_area_edges():
    cs = CASES['areas']
    st = new_state(cs['cfg'])
    cocoeval_tap(st, cs['cfg'], **cc.inputs(cs['calls'][0]))
    rec = st['table'][:int(st['records'])]
    med = (rec['ignored'] >> 10) & 1
    lar = (rec['ignored'] >> 20) & 1
    # frame 0 in score order: gt areas 32^2 -, =, +, 96^2 -, =, +  (matched: the gt's flag); frame 1: detection areas the same way (unmatched: their own)
    assert list(med) == [1, 0, 0, 0, 0, 1] * 2 and list(lar) == [1, 1, 1, 1, 0, 0] * 2
    assert (rec['ignored'] & 1 == 0).all() and list(st['npig']) == [6, 4, 2]


def _anchor(dets, n_gt=2):
    """gts 0 and 1 (area 5000: medium) far apart; dets = ['tp0' | 'tp1' | 'fp'] in descending score order, exact copies of a gt or far from both"""
    K = 3
    g0, g1 = cc._grid(K, 100, 100, 50, 50), cc._grid(K, 400, 100, 50, 50)
    box = np.array([100, 100, 50, 50], F32)
    kp = {'tp0': g0, 'tp1': g1, 'fp': cc._grid(K, 800, 500, 50, 50)}
    call = cc._hand(K, 1, [(0, kp[d], 0.9 - 0.1 * i) for i, d in enumerate(dets)], [(0, g, box, F32(5000.0), 0) for g in (g0, g1)[:n_gt]])
    cfg = CocoEvalCfg(K, 8, (0.05,) * K)
    a, b = new_state(cfg), new_state(cfg)
    cocoeval_tap(a, cfg, **cc.inputs(call))
    cocoeval_numpy_update(b, cfg, **cc.inputs(call))
    ra, rb = cocoeval_tap_accumulate(a, cfg), cocoeval_numpy_accumulate(b)
    assert ra.tobytes() == rb.tobytes()
    fa, fb = finish(ra), finish(rb)
    assert fa.stats.tobytes() == fb.stats.tobytes()
    return fa


def test_anchor_tp_fp_tp():
    # two gts, records TP, FP, TP at every threshold (the OKS of a copy is 1): rc = .5, .5, 1; pr = 1/(1+e), 1/(2+e), 2/(3+e), enveloped to p0, 2/(3+e), 2/(3+e).
    # Recall thresholds 0..0.50 (51 of them) read position 0, 0.51..1 (50) read position 2.
    r = _anchor(['tp0', 'fp', 'tp1'])
    ap = (51 + 50 * 2 / (3 + EPS)) / 101
    assert abs(ap - 0.834983498349835) < 1e-12
    assert abs(r.stats[0] - ap) < 1e-12 and abs(r.stats[1] - ap) < 1e-12 and abs(r.stats[2] - ap) < 1e-12 and abs(r.stats[3] - ap) < 1e-12
    assert r.stats[5] == 1.0 and r.stats[6] == 1.0 and r.stats[8] == 1.0
    assert r.precision[0, 0, 50] == 1 / (1 + EPS) and r.precision[0, 0, 51] == 2 / (3 + EPS)


def test_anchor_tp_fp():
    # two gts, records TP, FP: rc = .5, .5; thresholds up to 0.50 read p0 = 1/(1+e), the other 50 find no position: 0
    r = _anchor(['tp0', 'fp'])
    ap = 51 * (1 / (1 + EPS)) / 101
    assert abs(r.stats[0] - ap) < 1e-12 and r.stats[5] == 0.5
    assert r.precision[0, 3, 50] == 1 / (1 + EPS) and r.precision[0, 3, 51] == 0.0


def test_anchor_a_perfect_run_is_not_one():
    # one gt, one record.  (With two records the second precision is 2 / (2 + 2^-52) == 1.0, because 2 + 2^-52 rounds to 2, and the envelope lifts the first.)
    r = _anchor(['tp0'], n_gt=1)
    assert (r.precision[0] == 0.9999999999999998).all() and 1 / (1 + EPS) == 0.9999999999999998 and 2 / (2 + EPS) == 1.0
    assert (_anchor(['tp0', 'tp1']).precision[0] == 1.0).all()
    assert abs(r.stats[0] - 0.9999999999999998) < 1e-12 and r.stats[0] < 1.0 and r.stats[5] == 1.0


def test_anchor_a_range_without_gts_gives_minus_one():
    r = _anchor(['tp0', 'fp', 'tp1'])
    assert r.npig == (2, 2, 0) and r.stats[4] == -1.0 and r.stats[9] == -1.0 and (r.precision[2] == -1).all() and (r.recall[2] == -1).all()
    # no gt at all: every figure -1; no record but a gt: 0
    cfg = CocoEvalCfg(3, 8, (0.05,) * 3)
    st = new_state(cfg)
    assert (finish(cocoeval_tap_accumulate(st, cfg)).stats == -1).all()
    r0 = _anchor([], n_gt=1)
    assert r0.stats[0] == 0.0 and r0.stats[5] == 0.0 and r0.stats[4] == -1.0


def test_every_refusal_by_message():
    lib = capi.load_library()
    K = 3
    cfg = CocoEvalCfg(K, 8, (0.05,) * K)
    c, sig = dc.c_config(cfg)
    st = new_state(cfg)
    kp, sc = np.zeros((1, K, 3), F32), np.zeros(1, F32)
    box, area = np.zeros((1, 4), F32), np.ones(1, F32)
    P = lambda a: None if a is None else a.ctypes.data

    def upd(cfgp=None, sigmas=sig, kpts=kp, score=sc, n=1, gk=kp, gb=box, ga=area, g=1, n_frames=1, state=st):
        return lib.vp_dbg_cocoeval_update_host(P(state), C.byref(c) if cfgp is None else cfgp, P(sigmas), P(kpts), P(score), None, None, n, P(gk), P(gb), P(ga), None, None, g,
                                               n_frames, None)

    def refused(rc, text):
        assert rc == capi.VP_ERR_INVALID and text in lib.vp_last_error(None).decode(), (rc, lib.vp_last_error(None))
    refused(upd(cfgp=C.POINTER(capi.vp_cocoeval_cfg)()), 'null cfg')
    refused(upd(kpts=None), 'null kpts or score')
    refused(upd(score=None), 'null kpts or score')
    refused(upd(gk=None), 'null gt_kpts, gt_box or gt_area')
    refused(upd(gb=None), 'null gt_kpts, gt_box or gt_area')
    refused(upd(ga=None), 'null gt_kpts, gt_box or gt_area')
    refused(upd(n=-1), 'n = -1 outside 0..8192')
    refused(upd(n=8193), 'n = 8193 outside')
    refused(upd(g=-1), 'g = -1 outside')
    refused(upd(g=8193), 'g = 8193 outside')
    refused(upd(n_frames=0), 'n_frames = 0 outside 1..256')
    refused(upd(n_frames=257), 'n_frames = 257 outside')
    refused(upd(sigmas=None), 'null sigmas')
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused(upd(sigmas=np.array([0.05, bad, 0.05], F64)), 'sigma[1] not finite or <= 0')
    for nj in (0, 257):
        refused(upd(cfgp=C.byref(capi.vp_cocoeval_cfg(nj, 8, (C.c_int32 * 2)(0, 0)))), f'n_joints = {nj} outside 1..256')
    for mr in (0, (1 << 20) + 1):
        refused(upd(cfgp=C.byref(capi.vp_cocoeval_cfg(K, mr, (C.c_int32 * 2)(0, 0)))), f'max_records = {mr} outside')
    refused(upd(state=None), 'null state')
    res = np.zeros((), dc.RESULT)
    refused(lib.vp_dbg_cocoeval_accumulate_host(st.ctypes.data, C.byref(c), None), 'null accumulate destination')
    refused(lib.vp_dbg_cocoeval_accumulate_host(st.ctypes.data, None, res.ctypes.data), 'null cfg')
    assert st.tobytes() == new_state(cfg).tobytes()   # a refusal writes nothing
    assert upd(n=0, g=0, kpts=None, score=None, gk=None, gb=None, ga=None) == 0 and int(st['calls']) == 1   # both ends of the ranges pass
    with pytest.raises(ValueError):
        CocoEvalCfg(18)
    with pytest.raises(ValueError):
        CocoEvalCfg(3, 8, (0.05, 0.0, 0.05))
    with pytest.raises(ValueError):
        dc.coco_sigmas('mpii')
    assert len(dc.coco_sigmas('coco')) == 17 and dc.coco_sigmas()[0] == .26 / 10.0 and dc.coco_sigmas()[11] == 1.07 / 10.0


def test_load_annotations_and_results_json(tmp_path):
    K = 17
    rng = np.random.default_rng(3)
    anns, images = [], []
    for image_id in (42, 7, 19):   # not ascending in the file
        images.append({'id': image_id, 'file_name': f'{image_id:012d}.jpg', 'width': 64, 'height': 48})
    truth = {}
    for i, image_id in enumerate((7, 7, 42)):
        kp = np.round(rng.uniform(0, 40, (K, 3)))
        kp[:, 2] = rng.integers(0, 3, K)
        anns.append({'id': 100 + i, 'image_id': image_id, 'category_id': 1, 'keypoints': [float(v) for v in kp.reshape(-1)], 'num_keypoints': int((kp[:, 2] > 0).sum()),
                     'bbox': [1.0 + i, 2.0, 30.0, 40.0], 'area': 1200.0 + i, 'iscrowd': int(i == 1)})
        truth.setdefault(image_id, []).append(kp)
    anns.append({'id': 999, 'image_id': 7, 'category_id': 2, 'bbox': [0, 0, 1, 1], 'area': 1.0, 'iscrowd': 0})   # another category: left out
    path = tmp_path / 'ann.json'
    path.write_text(json.dumps({'images': images, 'annotations': anns, 'categories': [{'id': 1, 'name': 'person'}]}))
    a = dc.load_annotations(str(path))
    assert a.image_ids == [7, 19, 42] and a.file_names[0] == '000000000007.jpg' and a.sizes[0] == (64, 48) and a.n_joints == K
    assert [len(v) for v in a.gt_area] == [2, 0, 1] and list(a.gt_flags[0]) == [0, 1] and a.gt_kpts[1].shape == (0, K, 3)
    want = np.array(truth[7], F32)
    assert np.array_equal(a.gt_kpts[0][:, :, 0], want[:, :, 1]) and np.array_equal(a.gt_kpts[0][:, :, 1], want[:, :, 0]) and np.array_equal(a.gt_kpts[0][:, :, 2], want[:, :, 2])
    assert list(a.gt_box[2][0]) == [3.0, 2.0, 30.0, 40.0] and a.gt_area[2][0] == F32(1202.0)
    b = a.batch([0, 1, 2])
    assert b['n_frames'] == 3 and list(b['gt_frame']) == [0, 0, 2] and b['gt_kpts'].shape == (3, K, 3) and b['gt_kpts'].dtype == F32
    # the batch feeds the evaluator as it is: the gts as detections give a perfect run on the not-ignored ones
    cfg = CocoEvalCfg(K, 16)
    st = new_state(cfg)
    cocoeval_tap(st, cfg, b['gt_kpts'], np.array([0.9, 0.8, 0.7], F32), frame=b['gt_frame'], **b)
    r = finish(cocoeval_tap_accumulate(st, cfg))
    assert r.images == 3 and r.gts == 3 and r.npig[0] == 2 and r.stats[5] == 1.0 and abs(r.stats[0] - 1.0) < 1e-12
    assert 'Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = 1.000' in r.summary() and len(r.summary().splitlines()) == 10
    # the results file of the reference script: [x, y, 0] per joint, rounded to whole pixels
    kp = np.array([[[10.4, 20.6, 0.9]] * K], F32)
    out = dc.results_json(str(tmp_path / 'res.json'), [42], kp, [0.5])
    assert json.loads((tmp_path / 'res.json').read_text()) == out
    assert out[0]['image_id'] == 42 and out[0]['category_id'] == 1 and out[0]['bbox'] == [] and out[0]['keypoints'][:3] == [21.0, 10.0, 0] and len(out[0]['keypoints']) == 3 * K
    assert dc.results_json(None, [42], kp, [0.5], rounded=False)[0]['keypoints'][:2] == [float(F32(20.6)), float(F32(10.4))]
