"""GPU: detector boxes on device frames -> frame keypoints on the device, ordered on the caller's stream (vp_infer_boxes_stream,
VitPoseHip.infer_boxes).  Bit for bit against the host route it replaces (frames_crop_params + infer_frames + the offsets of
VitInference.inference_frames), the reference golden, the stream ordering without host blocking, invalid rows, graph replay, a ViTPose+ expert
and the empty call.  The geometry alone is pinned on the CPU (tests/test_boxes_host.py)."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

from easy_vitpose_amd import VitPoseHip
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.cropprep import frames_crop_params
from easy_vitpose_amd.synth import synthetic_moe_state_dict, synthetic_state_dict

pytestmark = pytest.mark.gpu

SIZES = [(720, 1280), (1080, 1920), (481, 333), (40, 30)]


@functools.lru_cache(maxsize=1)
def scene():
    """Four frames of different sizes and 19 float32 boxes in the detector's [n, 6] layout, interleaved across frames: border boxes, whole-frame
    boxes, .5 ties, a box whose padded crop is exactly 192 x 256, one listed twice."""
    rng = np.random.default_rng(31)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    per = [(0, [0, 0, 1280, 720]), (1, [800.5, 300.5, 1100.5, 900.5]), (2, [0, 0, 333, 481]), (0, [1100, 300, 1290, 650]),
           (3, [2, 3, 20, 30]), (1, [1700, 900, 1920, 1080]), (0, [-20, 200, 150, 500]), (2, [250.5, 380.5, 340, 490]),
           (1, [20, 40, 260, 400]), (0, [510, 210, 692, 456]), (3, [0, 0, 30, 40]), (1, [20.5, 41.5, 259.5, 399.5]),
           (2, [100, 100, 112, 109]), (0, [700, 500, 900, 720]), (1, [0, 0, 1920, 1080]), (0, [400, 0, 600, 180]),
           (2, [30, 60, 200, 300]), (1, [1000, 10, 1300, 410]), (0, [400, 0, 600, 180])]
    fidx = np.array([f for f, _ in per], np.int32)
    boxes = np.zeros((len(per), 6), np.float32)
    boxes[:, :4] = [b for _, b in per]
    boxes[:, 4] = 0.9
    return frames, boxes, fidx


def host_route(eng, d_frames, boxes, fidx, pad=10):
    """Today's device route: boxes to the host, frames_crop_params on the float64 boxes, infer_frames on device frames, the offsets added on
    the host as VitInference.inference_frames adds them.  Returns (keypoints in frame pixels, p9)."""
    p9 = np.concatenate([np.zeros((0, 9), np.int32)] + [frames_crop_params([b[None, :4].astype(np.float64)], [tuple(d_frames[f].shape)], pad)
                                                        for b, f in zip(boxes, fidx)])
    p9[:, 0] = fidx
    kps = eng.infer_frames(d_frames, p9)
    for k, p in zip(kps, p9[:, 1:]):
        k[:, :2] += np.array([p[1] - p[5], p[0] - p[4]])
    return kps, p9


def to_dev(frames, boxes, fidx):
    import torch
    return [torch.from_numpy(f).cuda() for f in frames], torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda()


@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_infer_boxes_equals_the_host_route(dtype):
    import torch
    frames, boxes, fidx = scene()
    d_frames, d_boxes, d_fidx = to_dev(frames, boxes, fidx)
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=dtype, max_batch=8)   # 19 boxes: chunks of 8, 8, 3 on the handle's stream
    want, p9 = host_route(eng, d_frames, boxes, fidx)
    for sel in (slice(None), slice(0, 7), slice(4, 5)):                              # and the caller-stream path (<= 16 boxes)
        out, cp, st = eng.infer_boxes(d_frames, d_boxes[sel], d_fidx[sel], crop_params=True, status=True)
        torch.cuda.current_stream().synchronize()
        assert out.shape == (len(boxes[sel]), 17, 3)
        assert (st.cpu().numpy() == 0).all()
        assert np.array_equal(cp.cpu().numpy(), p9[sel])
        got = out.cpu().numpy()
        if sel == slice(None):
            assert np.array_equal(got, want), f'{(got != want).sum()} differing values'
        else:   # a different batch: its own host route (same chunks, same plan)
            assert np.array_equal(got, host_route(eng, d_frames, boxes[sel], fidx[sel])[0])
    # frame_index=None: every box on frame 0
    sel0 = np.flatnonzero(fidx == 0)
    got0 = eng.infer_boxes(d_frames, d_boxes[torch.from_numpy(sel0).cuda()]).cpu().numpy()
    assert np.array_equal(got0, host_route(eng, d_frames, boxes[sel0], fidx[sel0])[0])
    with pytest.raises(TypeError):
        eng.infer_boxes([frames[0]], d_boxes)
    with pytest.raises(TypeError):
        eng.infer_boxes(d_frames, d_boxes.double())
    with pytest.raises(ValueError):
        eng.infer_boxes(d_frames, d_boxes[:, :3])
    with pytest.raises(TypeError):
        eng.infer_boxes(d_frames, d_boxes, d_fidx.long())
    eng.close()


def test_infer_boxes_matches_reference_golden(golden_dir):
    import torch
    from cases import frame_case
    from helpers import weights
    from test_gpu_frames import _check_against_golden
    g = np.load(os.path.join(golden_dir, 'frame_inference.npz'))
    frame, boxes = frame_case()
    det = boxes[boxes[:, 4] > 0.35]
    _, sd, _ = weights('s', 'coco')
    eng = VitPoseHip(model_shape('s', 'coco'), sd, dtype='fp16', max_batch=4)
    out, cp = eng.infer_boxes([torch.from_numpy(frame).cuda()], torch.from_numpy(det.astype(np.float32)).cuda(), crop_params=True)
    kp, cp = out.cpu().numpy(), cp.cpu().numpy()
    _check_against_golden({i: kp[i] for i in range(len(kp))}, g, frame, boxes)
    padded = np.stack([cp[:, 1], cp[:, 2], cp[:, 1] + cp[:, 3], cp[:, 2] + cp[:, 4]], 1)   # the reference's in-place box update
    assert np.array_equal(padded, g['padded_boxes'])
    eng.close()


@pytest.mark.parametrize('n', [12, 20])
def test_infer_boxes_is_stream_ordered_without_host_blocking(n):
    """A long producer on the current stream, the frames and boxes produced behind it: infer_boxes returns while the stream is still busy, and a
    consumer queued right after sees the finished keypoints.  12 boxes run on the caller's stream, 20 on the handle's stream behind two events."""
    import torch
    frames, boxes, fidx = scene()
    boxes, fidx = np.concatenate([boxes, boxes])[:n], np.concatenate([fidx, fidx])[:n]
    src_frames, src_boxes, src_fidx = to_dev(frames, boxes, fidx)
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype='fp16', max_batch=32)
    torch.cuda.synchronize()
    want = eng.infer_boxes(src_frames, src_boxes, src_fidx)
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    out = torch.empty((n, 17, 3), device='cuda')   # one output buffer: the graph of the 12-box chunk is captured once and replayed
    for _ in range(3):
        cur = torch.cuda.current_stream()
        torch.cuda._sleep(1_000_000_000)                                  # a long producer in front of everything (a few hundred ms)
        d_frames = [f.clone() for f in src_frames]                        # produced behind it
        d_boxes = src_boxes.clone() + 0.0
        d_fidx = src_fidx.clone()
        out.fill_(float('nan'))
        eng.infer_boxes(d_frames, d_boxes, d_fidx, out=out)
        assert not cur.query(), 'the call blocked the host until the stream drained'
        total = out.sum()                                                 # a consumer on the same stream
        cur.synchronize()
        assert torch.isfinite(total).item()
        assert np.array_equal(out.cpu().numpy(), want)
    # a side-stream call, then a default-stream call on the same handle: the library orders the second behind the first
    side = torch.cuda.Stream()
    o1, o2 = torch.full_like(out, float('nan')), torch.full_like(out, float('nan'))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(300_000_000)
        eng.infer_boxes(src_frames, src_boxes, src_fidx, out=o1)
        s1 = o1.sum()
    eng.infer_boxes(src_frames, src_boxes, src_fidx, out=o2)
    s2 = o2.sum()
    torch.cuda.synchronize()
    assert torch.isfinite(s1).item() and torch.isfinite(s2).item()
    assert np.array_equal(o1.cpu().numpy(), want) and np.array_equal(o2.cpu().numpy(), want)
    eng.close()


def test_invalid_rows_get_a_status_and_zero_keypoints(one_launch_family):
    import torch
    frames, boxes, fidx = scene()
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype='fp16', max_batch=16)
    good = np.arange(6)
    bad_boxes = np.array([[10, 10, 50, 50, 1, 0], [np.nan, 10, 50, 50, 1, 0], [10, 10, 50, np.inf, 1, 0], [-300, 10, -100, 50, 1, 0],
                          [300, 300, 250, 250, 1, 0]], np.float32)
    bad_fidx = np.array([7, 0, 1, 0, 2], np.int32)
    mixed_b = np.concatenate([boxes[:3], bad_boxes[:2], boxes[3:6], bad_boxes[2:]])
    mixed_f = np.concatenate([fidx[:3], bad_fidx[:2], fidx[3:6], bad_fidx[2:]])
    is_good = np.array([1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0], bool)
    out, cp, st = eng.infer_boxes(d_frames, torch.from_numpy(mixed_b).cuda(), torch.from_numpy(mixed_f).cuda(), crop_params=True, status=True)
    ref = eng.infer_boxes(d_frames, torch.from_numpy(boxes[good]).cuda(), torch.from_numpy(fidx[good]).cuda())
    torch.cuda.synchronize()
    out, cp, st, ref = out.cpu().numpy(), cp.cpu().numpy(), st.cpu().numpy(), ref.cpu().numpy()
    assert st.tolist() == [0, 0, 0, 1, 2, 0, 0, 0, 2, 3, 3]
    assert (out[~is_good] == 0).all() and (cp[~is_good] == 0).all()
    assert np.array_equal(out[is_good], ref)
    eng.close()


def test_repeated_small_calls_are_identical():
    """First sighting (eager), capture, replay: the same bits each time."""
    import torch
    frames, boxes, fidx = scene()
    d_frames, d_boxes, d_fidx = to_dev(frames, boxes[:5], fidx[:5])
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype='fp16', max_batch=8)
    out = torch.empty((5, 17, 3), device='cuda')
    runs = []
    for _ in range(3):
        eng.infer_boxes(d_frames, d_boxes, d_fidx, out=out)
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    assert np.array_equal(runs[0], host_route(eng, d_frames, boxes[:5], fidx[:5])[0])
    eng.close()


def test_infer_boxes_on_a_vitpose_plus_expert():
    frames, boxes, fidx = scene()
    d_frames, d_boxes, d_fidx = to_dev(frames, boxes, fidx)
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_moe_state_dict(shp, 192, seed=0, peaked=True), dtype='fp16', max_batch=8)
    eng.set_dataset('aic')
    got = eng.infer_boxes(d_frames, d_boxes, d_fidx).cpu().numpy()
    want, _ = host_route(eng, d_frames, boxes, fidx)
    assert got.shape == (len(boxes), 14, 3) and np.array_equal(got, want)
    eng.close()


def test_empty_call_writes_nothing():
    import torch
    frames, _, _ = scene()
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype='fp16', max_batch=4)
    sentinel = torch.full((1, 17, 3), 7.0, device='cuda')
    out = eng.infer_boxes(d_frames, torch.zeros((0, 6), device='cuda'), out=sentinel[:0])
    assert out.shape == (0, 17, 3)
    rc = eng.lib.vp_infer_boxes_stream(eng._h, None, 0, None, 4, None, 0, 10, sentinel.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and (sentinel == 7.0).all().item()
    eng.close()
