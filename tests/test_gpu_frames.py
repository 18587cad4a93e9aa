"""GPU: the crops of several frames in one call (vp_infer_frames, VitPoseHip.infer_frames, VitInference.inference_frames, the CLI's
--frame-batch).  Against vp_infer on the host-prepared crops bit for bit (fp16, bf16, host and device frames, a ViTPose+ expert), against
per-frame calls of the caller-level loop, and against the reference golden.  Only valid inputs reach the library here: the refusals are
tested on the CPU through the plan function (tests/test_frames_host.py)."""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest

from easy_vitpose_amd import VitInference, VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.cropprep import crop_params, prepare_crops_host
from easy_vitpose_amd.synth import synthetic_moe_state_dict, synthetic_state_dict
from helpers import CONF_TOL, KP_TOL_PX, argmax_margin, dark_offset_px, oracle_heatmaps, weights
from oracle import vitpose_cpu as O

pytestmark = pytest.mark.gpu

SIZES = [(720, 1280), (1080, 1920), (481, 333), (256, 192), (40, 30)]


def _boxes(rows):
    b = np.asarray(rows, dtype=np.float64)
    return np.concatenate([b, np.ones((len(b), 1))], 1)


@functools.lru_cache(maxsize=1)
def matrix():
    """Five frames of different sizes + a sixth entry that is frame 2 again; 0-6 crops per frame (frame 3 has none); an exact-2x crop,
    crops on every border, whole-frame crops, a crop listed twice; the rows interleaved across frames."""
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    frames.append(frames[2])
    per = {
        0: [[0, 0, 1280, 720], [0, 200, 150, 500], [400, 0, 600, 180], [1100, 300, 1280, 650], [700, 500, 900, 720], [500, 200, 700, 500]],
        1: [[0, 0, 1920, 1080], [800, 300, 1100, 900], [1700, 900, 1920, 1080], [20, 40, 260, 400]],
        2: [[0, 0, 333, 481], [250, 380, 333, 481], [100, 100, 112, 109]],
        4: [[0, 0, 30, 40], [12, 20, 15, 25]],
        5: [[30, 60, 200, 300]],
    }
    rows = []
    for f, b in per.items():
        p = crop_params(_boxes(b), frames[f].shape[:2], 10)
        rows.append(np.concatenate([np.full((len(p), 1), f), p], 1))
    p9 = np.concatenate(rows).astype(np.int32)
    p9[5] = (0, 500, 200, 384, 512, 0, 0, 384, 512)   # exactly 2x -> the box-average path
    p9 = np.concatenate([p9, p9[7:8]])                # the same crop twice
    p9 = p9[np.random.default_rng(5).permutation(len(p9))]
    assert len(set(p9[:, 0].tolist())) == 5 and 3 not in p9[:, 0]
    return frames, np.ascontiguousarray(p9)


def host_crops(frames, p9):
    return np.concatenate([prepare_crops_host(frames[p[0]], p[None, 1:]) for p in p9])


@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_infer_frames_equals_vp_infer_on_host_prepared_crops(dtype):
    import torch
    frames, p9 = matrix()
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=dtype, max_batch=4)   # chunks straddle frames
    want = eng.infer(host_crops(frames, p9), p9[:, 7:9])
    got = eng.infer_frames(frames, p9)
    assert got.shape == want.shape == (len(p9), 17, 3)
    assert np.array_equal(got, want), f'{(got != want).sum()} differing values'
    # device frames: read in place, the same bits
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    got_d = eng.infer_frames(d_frames, p9)
    assert np.array_equal(got_d, want)
    # vp_infer_frame is the one-frame case of the same path
    sel = p9[p9[:, 0] == 1]
    assert np.array_equal(eng.infer_frame(frames[1], sel[:, 1:]), eng.infer_frames([frames[1]], np.concatenate([0 * sel[:, :1], sel[:, 1:]], 1)))
    with pytest.raises(TypeError):
        eng.infer_frames([frames[0], d_frames[1]], p9[:1])
    eng.close()


def test_infer_frames_on_a_vitpose_plus_expert():
    shp = model_shape('s', 'coco')
    frames, p9 = matrix()
    eng = VitPoseHip(shp, synthetic_moe_state_dict(shp, 192, seed=0, peaked=True), dtype='fp16', max_batch=8)
    eng.set_dataset('aic')
    got = eng.infer_frames(frames, p9)
    want = eng.infer(host_crops(frames, p9), p9[:, 7:9])
    assert got.shape == (len(p9), 14, 3) and np.array_equal(got, want)
    eng.close()


def test_empty_calls():
    frames, _ = matrix()
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype='fp16', max_batch=4)
    lib = capi.load_library()
    table = (capi.vp_frame * 2)(capi.vp_frame(frames[3].ctypes.data, 256, 192), capi.vp_frame(frames[4].ctypes.data, 40, 30))
    out = np.full((2, 17, 3), 7.0, np.float32)
    assert lib.vp_infer_frames(eng._h, table, 2, 0, None, 0, out.ctypes.data) == capi.VP_OK
    assert (out == 7.0).all()
    assert eng.infer_frames(frames, np.zeros((0, 9), np.int32)).shape == (0, 17, 3)
    eng.close()
    sd = synthetic_state_dict(shp, 0)
    people = _boxes([[60, 40, 200, 230]])
    for found in ([False, False, False], [True, False, True]):
        it = iter(found)
        model = VitInference(sd, lambda img: people.copy() if next(it) else np.zeros((0, 5)), model_name='s', dataset='coco', max_batch=4)
        res = model.inference_frames([frames[0], frames[1], frames[2]])
        assert [len(r) for r in res] == [int(x) for x in found]
        assert all(r[0].shape == (17, 3) for r in res if r)


def _clip():
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (7, 360, 480, 3), dtype=np.uint8)
    frames[:, 0, 0, 0] = np.arange(7)   # the detector reads the frame number from the first pixel
    boxes = [_boxes([[40 + 6 * f, 60, 160 + 6 * f, 300], [300 - 5 * f, 80, 400 - 5 * f, 320], [200, 10 + 3 * f, 260, 90 + 3 * f]][:2 + f % 2])
             for f in range(7)]
    return list(frames), boxes


def _run(frames, boxes, chunks, video):
    calls = []

    def det(img):
        f = int(img[0, 0, 0])
        calls.append(f)
        return boxes[f].copy()

    sd = synthetic_state_dict(model_shape('s', 'coco'), 0, peaked=True)
    model = VitInference(sd, det, model_name='s', dataset='coco', is_video=video, yolo_step=2, max_batch=16)
    res = []
    if chunks is None:
        res = [model.inference(f) for f in frames]
    else:
        s = 0
        for c in chunks:
            res += model.inference_frames(frames[s:s + c])
            s += c
    return res, calls, model


@pytest.mark.parametrize('video', [True, False])
def test_inference_frames_equals_per_frame_inference(one_launch_family, video):
    frames, boxes = _clip()
    a, calls_a, ma = _run(frames, boxes, [3, 4], video)
    b, calls_b, mb = _run(frames, boxes, None, video)
    assert calls_a == calls_b
    if video:
        assert calls_a != list(range(7))   # yolo_step = 2 skipped some frames
    assert len(a) == len(b) == 7
    assert sum(len(r) for r in a) >= 14
    for ra, rb in zip(a, b):
        assert list(ra.keys()) == list(rb.keys())
        for k in ra:
            assert np.array_equal(ra[k], rb[k])
    ta, tb = ma._tracker_res, mb._tracker_res
    assert np.array_equal(np.asarray(ta[0]), np.asarray(tb[0])) and list(ta[1]) == list(tb[1]) and list(ta[2]) == list(tb[2])
    assert list(ma._keypoints) == list(mb._keypoints) and all(np.array_equal(ma._keypoints[k], mb._keypoints[k]) for k in ma._keypoints)
    assert ma._img is frames[-1] and ma.frame_counter == mb.frame_counter == 7


def _check_against_golden(res, g, frame, boxes):
    assert sorted(res.keys()) == g['ids'].tolist()
    kp = np.stack([res[i] for i in g['ids']])
    ref = g['keypoints']
    assert np.abs(kp[..., 2] - ref[..., 2]).max() < CONF_TOL
    det = boxes[boxes[:, 4] > 0.35]
    p = crop_params(det[:, :4].round().astype(int), frame.shape[:2], 10)
    ref_hm = oracle_heatmaps('s', 'coco', prepare_crops_host(frame, p))
    ok = (argmax_margin(ref_hm) > 5e-3) & (dark_offset_px(O.decode_per_crop(ref_hm, p[:, 6:8]), ref_hm, p[:, 6:8]) < 1.5)
    assert ok.sum() >= 10
    tol_y = (KP_TOL_PX * np.maximum(p[:, 7] / 256.0, 1.0))[:, None] * np.ones_like(ok, dtype=np.float64)
    tol_x = (KP_TOL_PX * np.maximum(p[:, 6] / 192.0, 1.0))[:, None] * np.ones_like(ok, dtype=np.float64)
    dy, dx = np.abs(kp[..., 0] - ref[..., 0]), np.abs(kp[..., 1] - ref[..., 1])
    assert (dy[ok] < tol_y[ok]).all() and (dx[ok] < tol_x[ok]).all()


def test_inference_frames_matches_reference_golden(golden_dir):
    from cases import frame_case
    g = np.load(os.path.join(golden_dir, 'frame_inference.npz'))
    frame, boxes = frame_case()
    other = np.ascontiguousarray(np.random.default_rng(9).integers(0, 256, (300, 500, 3), dtype=np.uint8))
    other_boxes = _boxes([[10, 20, 150, 280], [200, 50, 480, 290]])
    _, sd, _ = weights('s', 'coco')
    model = VitInference(sd, lambda img: (boxes if img.shape == frame.shape else other_boxes).copy(), model_name='s', dataset='coco', max_batch=4)
    res = model.inference_frames([frame.copy(), other, frame.copy()])
    assert len(res) == 3 and sorted(res[1].keys()) == [0, 1]
    _check_against_golden(res[0], g, frame, boxes)
    _check_against_golden(res[2], g, frame, boxes)
    assert np.array_equal(np.asarray(model._tracker_res[0]), g['padded_boxes']) and model._keypoints is res[2]


def test_cli_frame_batch_writes_the_same_json(tmp_path, monkeypatch):
    from easy_vitpose_amd import cli
    monkeypatch.setenv('VP_SPLITK', '0')
    frames, boxes = _clip()
    np.save(tmp_path / 'clip.npy', np.stack(frames))
    (tmp_path / 'boxes.json').write_text(json.dumps([b.tolist() for b in boxes]))
    outs = []
    for fb in ('4', '1'):
        out = tmp_path / f'out{fb}'
        rc = cli.main(['--input', str(tmp_path / 'clip.npy'), '--synthetic', 's', '--dataset', 'coco', '--boxes', str(tmp_path / 'boxes.json'),
                       '--output-path', str(out), '--save-json', '--max-batch', '8', '--frame-batch', fb])
        assert rc == 0
        outs.append((out / 'clip.npy' / 'clip_result.json').read_text())
    assert outs[0] == outs[1]
    assert len(json.loads(outs[0])['keypoints']) == 7
