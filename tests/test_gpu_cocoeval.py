"""GPU: the COCO keypoint evaluator on the device (vp_cocoeval_update / _update_stream / _accumulate / _accumulate_stream, VitPoseHip.cocoeval) against the host
model of the same header (vp_dbg_cocoeval_update_host / _accumulate_host, pinned on the CPU against its numpy twin and literal anchors: tests/test_cocoeval_host.py).
The state, `match` and the result blob are compared byte for byte: the OKS goes through the device's exp(), and the CPU test asserts for every case that no OKS
lies within 1e-9 of a threshold or of a competing OKS, so no decision can differ."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

from easy_vitpose_amd import VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd import devcoco as dc
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devcoco import (CocoEvalCfg, cocoeval_numpy_accumulate, cocoeval_numpy_update, cocoeval_tap, cocoeval_tap_accumulate, finish, new_state, parse_result)
from easy_vitpose_amd.synth import synthetic_state_dict
import cocoeval_cases as cc

pytestmark = pytest.mark.gpu
CASES = cc.host_cases()
F32, I32 = np.float32, np.int32


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def same(got, want, tag=''):
    for f in want.dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), (tag, f)


def to_device(call):
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in cc.inputs(call).items()}


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_host_model_on_the_cpu_cases(eng, name):
    cs = CASES[name]
    ev = eng.cocoeval(cs['cfg'])
    want = new_state(cs['cfg'])
    for i, call in enumerate(cs['calls']):
        got = ev.update_host(**cc.inputs(call))
        assert got.tobytes() == cocoeval_tap(want, cs['cfg'], **cc.inputs(call)).tobytes(), (name, i)
    same(ev.state(), want, name)
    same(ev.accumulate_host(), cocoeval_tap_accumulate(want, cs['cfg']), name)
    ev.close()


@pytest.mark.parametrize('rank,rows,gts', [(r, n, g) for r in (True, False) for n in (True, False) for g in (True, False)],
                         ids=lambda v: 'given' if v else 'absent')
def test_host_arrays_with_every_combination_of_rank_rows_and_gts(eng, rank, rows, gts):
    """vp_cocoeval_update on host arrays with rank given or null, with and without rows, with and without ground truths (7 rows, 3 gts: the margin-checked
    `null_optionals` call), twice: match, the state and the result equal the host tap byte for byte"""
    call = dict(cc.inputs(CASES['null_optionals']['calls'][0]))
    if rank:
        call['rank'] = np.array([0, -1, 2, 1, -1, 0, 3], I32)
    if not rows:
        call.update(kpts=None, score=None, frame=None, rank=np.zeros(0, I32) if rank else None)
    if not gts:
        call.update(gt_kpts=None, gt_box=None, gt_area=None, gt_flags=None, gt_frame=None)
    cfg = CocoEvalCfg(17, 64)
    ev, want = eng.cocoeval(cfg), new_state(cfg)
    for i in range(2):
        assert ev.update_host(**call).tobytes() == cocoeval_tap(want, cfg, **call).tobytes(), i
    same(ev.state(), want)
    same(ev.accumulate_host(), cocoeval_tap_accumulate(want, cfg))
    ev.close()


def test_stream_entries_with_reset_and_calls_without_rows_or_gts(eng):
    import torch
    cs = CASES['frames_256']
    cfg, call = cs['cfg'], cs['calls'][0]
    kw = to_device(call)
    n = len(call['kpts'])
    ev = eng.cocoeval(cfg)
    want = new_state(cfg)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    match = torch.empty((n, 10), dtype=torch.int32, device='cuda')
    with torch.cuda.stream(side):
        ev.update(**kw)
        ev.reset()
        for _ in range(2):
            ev.update(**kw, match=match)
        ev.update(kw['kpts'][:0], kw['score'][:0], gt_kpts=kw['gt_kpts'], gt_box=kw['gt_box'], gt_area=kw['gt_area'], gt_frame=kw['gt_frame'], n_frames=256)   # n = 0
        ev.update(kw['kpts'], kw['score'], frame=kw['frame'], n_frames=256)                                                                                  # g = 0
        res = ev.accumulate()
    side.synchronize()
    for _ in range(2):
        wm = cocoeval_tap(want, cfg, **cc.inputs(call))
    cocoeval_tap(want, cfg, None, None, gt_kpts=call['gt_kpts'], gt_box=call['gt_box'], gt_area=call['gt_area'], gt_frame=call['gt_frame'], n_frames=256)
    cocoeval_tap(want, cfg, call['kpts'], call['score'], frame=call['frame'], n_frames=256)
    assert int(want['calls']) == 4 and match.cpu().numpy().tobytes() == wm.tobytes()
    same(ev.state(), want)
    same(parse_result(res.cpu().numpy()), cocoeval_tap_accumulate(want, cfg))
    with torch.cuda.stream(side):
        ev.reset()
    side.synchronize()
    assert ev.state().tobytes() == bytes(dc.state_dtype(cfg).itemsize)
    ev.close()


def test_capture_of_update_and_accumulate_replayed_with_new_inputs(eng):
    import torch
    frames = [(3, 2), (20, 3), (25, 1), (0, 1), (2, 0)] * 8
    a, b = (cc._call(np.random.default_rng(seed), 17, frames, quantise=32) for seed in (900, 901))
    cfg = CocoEvalCfg(17, 5000)   # a sort network of 8192 keys: strides in global memory and in LDS
    kw = to_device(a)
    ev = eng.cocoeval(cfg)
    res = torch.zeros((dc.RESULT.itemsize,), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ev.update(**kw)   # warm-up outside the capture
        ev.accumulate(out=res)
        ev.reset()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ev.update(**kw)
        ev.accumulate(out=res)
    want = new_state(cfg)
    for call in (a, b):
        for k, v in cc.inputs(call).items():
            if isinstance(v, np.ndarray):
                kw[k].copy_(torch.from_numpy(np.ascontiguousarray(v)).cuda())
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        cocoeval_tap(want, cfg, **cc.inputs(call))
        same(parse_result(res.cpu().numpy()), cocoeval_tap_accumulate(want, cfg))
    same(ev.state(), want)
    assert int(want['calls']) == 2 and int(want['records']) > 400
    ev.close()


def test_65537_records_three_times_byte_identical(eng):
    cs = CASES['total_65537']
    outs = []
    for _ in range(3):
        ev = eng.cocoeval(cs['cfg'])
        for call in cs['calls']:
            ev.update_host(**cc.inputs(call))
        outs.append((ev.state().tobytes(), ev.accumulate_host().tobytes()))
        ev.close()
    assert outs[0] == outs[1] == outs[2]


def test_one_real_forward(eng, golden_dir):
    """eight peaked crops through infer_device, each an image of its own with the fixture's keypoints as its ground truth: the device's figures equal the twin's on
    the downloaded keypoints"""
    import torch
    from cases import peaked_crops
    z = np.load(os.path.join(golden_dir, 'peaked_s_coco.npz'))
    n = int(z['n'])
    assert n == 8
    crops = torch.from_numpy(peaked_crops(n)).cuda()
    gt = np.ascontiguousarray(z['keypoints'], dtype=F32)
    gt[:, :, 2] = 2
    box = np.tile(np.array([[0, 0, 192, 256]], F32), (n, 1))
    area = np.full(n, 256.0 * 192.0, F32)
    frame = np.arange(n, dtype=I32)
    cfg = CocoEvalCfg(17, 64)
    ev = eng.cocoeval(cfg)
    kp = torch.empty((n, 17, 3), dtype=torch.float32, device='cuda')
    eng.infer_device(crops, kp, sync=False)
    score = kp[:, :, 2].mean(dim=1).contiguous()
    dev = lambda a: torch.from_numpy(a).cuda()
    ev.update(kp, score, frame=dev(frame), gt_kpts=dev(gt), gt_box=dev(box), gt_area=dev(area), gt_frame=dev(frame), n_frames=n)
    torch.cuda.synchronize()
    twin = new_state(cfg)
    cocoeval_numpy_update(twin, cfg, kp.cpu().numpy(), score.cpu().numpy(), frame=frame, gt_kpts=gt, gt_box=box, gt_area=area, gt_frame=frame, n_frames=n)
    want = finish(cocoeval_numpy_accumulate(twin))
    r = ev.result()
    print('peaked s/coco, 8 crops: ' + ', '.join(f'{k} {v:.4f}' for k, v in zip(dc.STAT_NAMES, r.stats)))
    assert r.npig == (8, 0, 8) and r.records == 8
    assert r.stats.tobytes() == want.stats.tobytes() and r.stats[3] == -1 and r.stats[0] > 0.9
    ev.close()


def test_refusals_come_before_anything_is_enqueued(eng):
    import torch
    ev = eng.cocoeval(CocoEvalCfg(17, 16))
    kp = torch.zeros((2, 17, 3), device='cuda')
    sc = torch.zeros((2,), device='cuda')
    box = torch.zeros((2, 4), device='cuda')
    ev.update(kp, sc)
    torch.cuda.synchronize()
    before = ev.state()
    P = lambda t: t.data_ptr()
    for args, msg in (((P(kp), P(sc), None, None, 8193, None, None, None, None, None, 0, 1), 'n = 8193 outside 0..8192'),
                      ((P(kp), P(sc), None, None, 2, None, None, None, None, None, -1, 1), 'g = -1 outside 0..8192'),
                      ((P(kp), P(sc), None, None, 2, None, None, None, None, None, 0, 257), 'n_frames = 257 outside 1..256'),
                      ((None, P(sc), None, None, 2, None, None, None, None, None, 0, 1), 'null kpts or score with n > 0'),
                      ((P(kp), P(sc), None, None, 2, P(kp), P(box), None, None, None, 2, 1), 'null gt_kpts, gt_box or gt_area with g > 0')):
        rc = eng.lib.vp_cocoeval_update_stream(ev._e, *args, None, None)
        assert rc == capi.VP_ERR_INVALID and capi.last_error(eng._h) == 'cocoeval: ' + msg
    assert eng.lib.vp_cocoeval_accumulate_stream(ev._e, None, None) == capi.VP_ERR_INVALID and capi.last_error(eng._h) == 'cocoeval: null accumulate destination'
    h = C.c_void_p()
    bad = capi.vp_cocoeval_cfg(300, 16, (C.c_int32 * 2)(0, 0))
    sig = np.full(300, 0.05)
    assert eng.lib.vp_cocoeval_create(eng._h, C.byref(bad), sig.ctypes.data, C.byref(h)) == capi.VP_ERR_INVALID and not h.value
    assert capi.last_error(eng._h) == 'cocoeval: n_joints = 300 outside 1..256'
    ok = capi.vp_cocoeval_cfg(17, 16, (C.c_int32 * 2)(0, 0))
    assert eng.lib.vp_cocoeval_create(eng._h, C.byref(ok), None, C.byref(h)) == capi.VP_ERR_INVALID and capi.last_error(eng._h) == 'cocoeval: null sigmas'
    with pytest.raises(TypeError, match='kpts'):
        ev.update(np.zeros((2, 17, 3), F32), sc)
    with pytest.raises(ValueError, match='gt_box'):
        ev.update(kp, sc, gt_kpts=kp, gt_box=torch.zeros((3, 4), device='cuda'), gt_area=sc)
    torch.cuda.synchronize()
    assert ev.state().tobytes() == before.tobytes()
    ev.close()


def test_the_evaluation_tool_on_a_tiny_annotation_file(tmp_path):
    """tools/evaluation_on_coco.py --synthetic s --gt-boxes on three images and an annotation file written here (no data set and no checkpoint are available): the
    figures equal the twin's on the results file the tool writes"""
    import json
    import sys
    from PIL import Image
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import evaluation_on_coco as tool
    rng = np.random.default_rng(11)
    K = 17
    images, anns = [], []
    for image_id, people in ((30, 2), (4, 1), (17, 0)):   # not ascending in the file; one image without a person
        name = f'{image_id:012d}.jpg'
        Image.fromarray(rng.integers(0, 255, (240, 320, 3), dtype=np.uint8)).save(tmp_path / name)
        images.append({'id': image_id, 'file_name': name, 'width': 320, 'height': 240})
        for p in range(people):
            x, y, w, h = 20.0 + 150 * p, 30.0, 90.0, 160.0
            kp = np.stack([x + rng.uniform(0, w, K), y + rng.uniform(0, h, K), np.full(K, 2.0)], axis=1)
            anns.append({'id': len(anns) + 1, 'image_id': image_id, 'category_id': 1, 'keypoints': [float(v) for v in np.round(kp).reshape(-1)], 'num_keypoints': K,
                         'bbox': [x, y, w, h], 'area': w * h * 0.5, 'iscrowd': 0})
    (tmp_path / 'ann.json').write_text(json.dumps({'images': images, 'annotations': anns, 'categories': [{'id': 1, 'name': 'person'}]}))
    res = tmp_path / 'results.json'
    r = tool.evaluation_on_coco(tool.parse_arguments(['--synthetic', 's', '--gt-boxes', '--img_folder_path', str(tmp_path), '--annFile', str(tmp_path / 'ann.json'), '--batch', '2',
                                                      '--max-records', '64', '--results', str(res)]))
    out = json.loads(res.read_text())
    assert r.images == 3 and r.gts == 3 and r.records == 3 and r.calls == 2 and [e['image_id'] for e in out] == [4, 30, 30]
    ann = dc.load_annotations(str(tmp_path / 'ann.json'))
    kp = np.array([e['keypoints'] for e in out], F32).reshape(3, K, 3)[:, :, [1, 0, 2]]
    cfg = CocoEvalCfg(K, 64)
    twin = new_state(cfg)
    b = ann.batch([0, 1, 2])
    cocoeval_numpy_update(twin, cfg, kp, np.array([e['score'] for e in out], F32), frame=np.array([ann.image_ids.index(e['image_id']) for e in out], I32), **b)
    assert finish(cocoeval_numpy_accumulate(twin)).stats.tobytes() == r.stats.tobytes()
