"""GPU: the detector stage on the device (vp_detect_stream / vp_detect, VitPoseHip.detector, VitInference(detect=)) and the tracker's counted entry
(vp_tracker_update_counted_stream) against the host model of csrc/detgeom.h (vp_dbg_detect_host, pinned on the CPU against the reference's box NMS and a numpy
twin: tests/test_detect_host.py).  The header fixes every operation, the sort key fixes the order: equal means equal bytes -- rows, image, anchor, count, flags."""
from __future__ import annotations

import os
import warnings

import numpy as np
import pytest

from easy_vitpose_amd import Frame, VitInference, VitPoseHip
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devdetect import FLAG_CAND, DetectCfg, DeviceDetector, HostDetector, letterbox_params
from easy_vitpose_amd.devtracker import DeviceTracker, TrackCfg
from easy_vitpose_amd.draw import DrawStyle
from easy_vitpose_amd.posenms import PoseNms
from easy_vitpose_amd.synth import synthetic_state_dict
from detect_cases import SIZES, named_cases, random_head, same_bits, size_case, size_id

pytestmark = pytest.mark.gpu
CASES = named_cases()
NAMES = ('rows', 'image', 'anchor', 'count', 'flags')


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def on_stream(dev, pred, frames_hw, input_hw, n_out, offset=0):
    """vp_detect_stream on a device copy of pred (`offset` elements into a larger buffer: a start that is misaligned for 16-byte loads), downloaded"""
    import torch
    flat = torch.empty(pred.size + 8, dtype=torch.float16 if pred.dtype == np.float16 else torch.float32, device='cuda')
    view = flat[offset:offset + pred.size].view(pred.shape)
    view.copy_(torch.from_numpy(pred))
    assert view.is_contiguous() and (offset == 0 or view.data_ptr() % 16 != 0)
    out = dev.detect(view, frames_hw, input_hw, n_out)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check(eng, case, offsets=(0,)):
    cfg, pred, frames_hw, input_hw, n_out = case
    want = HostDetector(cfg).detect(pred, frames_hw, input_hw, n_out)
    dev = DeviceDetector(eng, cfg)
    routes = [('vp_detect', dev.detect_host(pred, frames_hw, input_hw, n_out))]
    routes += [(f'vp_detect_stream+{o}', on_stream(dev, pred, frames_hw, input_hw, n_out, o)) for o in offsets]
    dev.close()
    for route, got in routes:
        for what, g, w in zip(NAMES, got, want):
            assert same_bits(g, w), f'{route}: {what} differs\n{g}\n{w}'
    return want


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_host_tap_on_the_cases(eng, name):
    check(eng, CASES[name])


@pytest.mark.parametrize('i', range(len(SIZES)), ids=[size_id(s) for s in SIZES])
def test_device_equals_the_host_tap_on_the_kernel_sizes(eng, i):
    """every A, candidate count and image count at which the kernels take another path; a start one element into the buffer takes the scalar loads"""
    want = check(eng, size_case(i), offsets=(0, 1))
    assert [bool(f & FLAG_CAND) for f in want[4]] == [c > 2048 for c in SIZES[i][1]]


def test_goldens_through_the_real_entry(eng, golden_dir):
    g = np.load(os.path.join(golden_dir, 'detect_nms.npz'))
    for n in g['sizes']:
        dets = g[f'n{n}_dets']
        x1, y1, x2, y2, s = dets.T
        pred = np.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, s])[None]
        for ti, thr in enumerate(g['thrs']):
            keep = g[f'n{n}_t{ti}_keep']
            cfg = DetectCfg(nc=1, dtype='fp32', conf_thr=0.0, iou_thr=thr, extent=1.0, agnostic=True, max_det=1024)
            rows, image, anchor, count, flags = check(eng, (cfg, pred, (1024, 1024), (1024, 1024), None))
            m = int(count[-1])
            assert anchor[:m].tolist() == keep.tolist() and same_bits(rows[:m, :5], dets[keep]), (n, thr)


def test_back_to_back_calls_and_a_replayed_graph_give_identical_bytes(eng):
    """the counters are re-zeroed on the stream: a second call, and every replay of a captured call, starts from zero"""
    import torch
    cfg = DetectCfg(nc=3, dtype='fp16')
    pred = random_head(21, [300, 0, 2049, 70], 3, 8400)
    want = HostDetector(cfg).detect(pred, (1080, 1920), (640, 640), 400)
    dev = DeviceDetector(eng, cfg)
    d_pred = torch.from_numpy(pred).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        first = dev.detect(d_pred, (1080, 1920), (640, 640), 400)
        second = dev.detect(d_pred, (1080, 1920), (640, 640), 400)
    side.synchronize()
    for out in (first, second):
        for what, g, w in zip(NAMES, out, want):
            assert same_bits(g.cpu().numpy(), w), f'back to back: {what}'
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = dev.detect(d_pred, (1080, 1920), (640, 640), 400)
    for replay in range(2):
        for t in captured:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for what, g, w in zip(NAMES, captured, want):
            assert same_bits(g.cpu().numpy(), w), f'replay {replay}: {what}'
    del graph
    dev.close()


def test_tracker_counted_entry_equals_the_plain_entry_on_the_first_rows(eng):
    import torch
    rng = np.random.default_rng(3)
    cfg = TrackCfg(1, 1, 0.3, 3)
    counted, plain = DeviceTracker(eng, cfg), DeviceTracker(eng, cfg)
    base = np.array([[10, 8, 60, 90, 0.9, 0], [70, 12, 125, 93, 0.8, 0], [30, 5, 100, 88, 0.7, 0], [200, 50, 260, 150, 0.6, 0], [15, 200, 90, 300, 0.5, 0]], np.float32)
    cap = 9
    for call, m in enumerate((5, 3, 0, 5, 12, -2)):
        dets = np.full((cap, 6), np.nan, np.float32)   # rows from m on: NaN boxes and streams outside the table
        fidx = np.full(cap, 99, np.int32)
        k = max(0, min(m, cap, len(base)))
        dets[:k] = base[:k] + rng.uniform(-2, 2, (k, 6)).astype(np.float32)
        fidx[:k] = np.arange(k) % 3
        used = max(0, min(m, cap))
        if used > k:   # m beyond the filled rows (the cap decides): finite rows of stream 1
            dets[k:used] = base[:used - k] + 300
            fidx[k:used] = 1
        d_dets, d_fidx = torch.from_numpy(dets).cuda(), torch.from_numpy(fidx).cuda()
        got = counted.update(d_dets, d_fidx, n_out=16, n_dets=torch.tensor([m], dtype=torch.int32, device='cuda'))
        want = plain.update(d_dets[:used].contiguous(), d_fidx[:used].contiguous(), n_out=16)
        torch.cuda.synchronize()
        for what, g, w in zip(('rows', 'ids', 'stream', 'count', 'flags'), got, want):
            assert same_bits(g.cpu().numpy(), w.cpu().numpy()), f'call {call} (m = {m}): {what}'
        assert got[4].cpu().tolist() == [0, 0, 0], 'the rows beyond the count raise nothing'
        assert counted.state().tobytes() == plain.state().tobytes(), f'call {call}: state'
    assert counted.state()['next_id'].sum() > 5
    with pytest.raises(TypeError):
        counted.update(d_dets, d_fidx, n_out=16, n_dets=np.array([1], np.int32))
    with pytest.raises(ValueError):
        counted.update(d_dets, d_fidx, n_out=16, n_dets=torch.zeros(2, dtype=torch.int32, device='cuda'))
    counted.close()
    plain.close()


def people_head(boxes, frame_hw, input_hw, A=300, nc=80, jitter=0.0):
    """an fp16 head [1, 4 + nc, A] that holds `boxes` [n, 5] (frame pixels, score) as class 0, each with a weaker duplicate, and a class-5 box on top of the first"""
    gain, pad_x, pad_y = letterbox_params(frame_hw, input_hw)
    p = np.zeros((1, 4 + nc, A), np.float32)
    p[:, :4] = 10
    for k, b in enumerate(boxes):
        x1, y1, x2, y2 = b[0] * gain + pad_x + jitter, b[1] * gain + pad_y, b[2] * gain + pad_x + jitter, b[3] * gain + pad_y
        for a, ds, dx in ((7 + 13 * k, 0.0, 0.0), (9 + 13 * k, -0.05, 1.5)):
            p[0, :4, a] = ((x1 + x2) / 2 + dx, (y1 + y2) / 2, x2 - x1, y2 - y1)
            p[0, 4, a] = b[4] + ds
    p[0, :4, 200] = p[0, :4, 7]
    p[0, 4 + 5, 200] = 0.95
    return p.astype(np.float16)


def test_the_chain_from_the_head_to_the_drawing_on_one_stream(eng):
    """detect -> counted tracker -> infer_boxes(nms=) -> draw_poses, two time steps of 3 frames (one tracker stream each) on a side stream with ONE synchronisation
    at the end, against the same chain with the host route in the middle (synchronise, download the rows, upload the first count of them to the plain entry)"""
    import torch
    rng = np.random.default_rng(8)
    rgb = [rng.integers(0, 256, (97, 131, 3), dtype=np.uint8) for _ in range(3)]
    boxes = [np.array([[10, 8, 60, 90, 0.9], [70, 12, 125, 93, 0.8]], np.float32), np.array([[30, 5, 100, 88, 0.7]], np.float32), np.zeros((0, 5), np.float32)]
    heads = [np.concatenate([people_head(b, (97, 131), (160, 224), jitter=j) for b in boxes]) for j in (0.0, 1.0)]
    dcfg, tcfg, ncfg, style, n_det, n_trk = DetectCfg(classes='human'), TrackCfg(1, 1, 0.3, 3), PoseNms(oks_thr=0.5), DrawStyle(conf_thr=0.0, thickness=2), 8, 8
    det = eng.detector(dcfg)
    d_heads = [torch.from_numpy(h).cuda() for h in heads]

    def chain(host_route):
        trk = eng.tracker(tcfg)
        fr = [Frame.rgb(torch.from_numpy(f).cuda()) for f in rgb]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for d_head in d_heads:
                rows, image, anchor, count, flags = det.detect(d_head, (97, 131), (160, 224), n_det)
                if host_route:
                    side.synchronize()
                    m = int(count[-1].item())
                    t_rows = torch.from_numpy(rows.cpu().numpy()[:m].copy()).cuda()
                    t_image = torch.from_numpy(image.cpu().numpy()[:m].copy()).cuda()
                    trows, ids, stream, tcount, tflags = trk.update(t_rows, t_image, n_out=n_trk)
                else:
                    trows, ids, stream, tcount, tflags = trk.update(rows, image, n_out=n_trk, n_dets=count[-1:])
            out, score, rank, kept, cp, st = eng.infer_boxes(fr, trows, stream, nms=ncfg, crop_params=True, status=True)
            eng.draw_poses(fr, out, stream, style, rank=rank, ids=ids, boxes=trows)
        side.synchronize()
        res = [t.cpu().numpy() for t in (rows, image, anchor, count, flags, trows, ids, stream, tcount, tflags, out, score, rank, st)] + [f.planes[0].cpu().numpy() for f in fr]
        state = trk.state().tobytes()
        trk.close()
        return res, state

    (dev, dev_state), (host, host_state) = chain(False), chain(True)
    det.close()
    for k, (a, b) in enumerate(zip(dev, host)):
        assert same_bits(a, b), f'output {k}'
    assert dev_state == host_state
    rows, image, anchor, count, flags, trows, ids, stream, tcount = dev[:9]
    assert count.tolist() == [2, 1, 0, 3] and flags.tolist() == [0, 0, 0] and image.tolist() == [0, 0, 1] + [-1] * 5, 'the duplicates and the other class are gone'
    assert (rows[:3, 5] == 0).all() and tcount.tolist() == [2, 1, 0, 3] and sorted(ids[:3].tolist()) == [1, 1, 2]
    assert dev[13].tolist() == [0, 0, 0] + [1] * 5 and np.abs(dev[10][:3]).max() > 0 and not any(np.array_equal(f, r) for f, r in zip(dev[14:16], rgb[:2]))
    assert np.array_equal(dev[16], rgb[2]), 'a frame without a person stays as it was'


def test_vitinference_with_the_detector_stage_equals_the_host_taps_boxes():
    from cases import frame_case
    from helpers import weights
    frame, boxes = frame_case()
    _, sd, _ = weights('s', 'coco')
    head = people_head(boxes, frame.shape[:2], (640, 640), A=8400)[0]
    cfg = DetectCfg(classes='human')
    rows, _, _, count, _ = HostDetector(cfg).detect(head[None], frame.shape[:2], (640, 640))
    tap_boxes = rows[:int(count[-1]), :5].astype(np.float64)
    assert len(tap_boxes) == 3 and (tap_boxes[:, 4] > 0.35).all() and np.abs(tap_boxes[:, :4] - boxes[:3, :4]).max() < 1.0
    res = {}
    for which in ('stage', 'boxes'):
        kw = dict(detect=cfg) if which == 'stage' else {}
        yolo = (lambda img: (head, (640, 640))) if which == 'stage' else (lambda img: tap_boxes.copy())
        model = VitInference(sd, yolo, model_name='s', dataset='coco', max_batch=8, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res[which] = [model.inference(frame.copy())] + model.inference_frames([frame.copy(), frame.copy()])
    assert all(len(r) == 3 for r in res['boxes'])
    for a, b in zip(res['boxes'], res['stage']):
        assert list(a.keys()) == list(b.keys()) and all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(TypeError):
        VitInference(sd, lambda img: None, model_name='s', dataset='coco', detect=dict())
