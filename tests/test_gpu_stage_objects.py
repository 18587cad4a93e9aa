"""GPU: the lifetime the six stage objects share (csrc/stageobj.h, easy_vitpose_amd/_stage.py): the tracker, the smoother, the metrics and COCO evaluators, the
detector stage and the YOLO network, each at the smallest configuration its case module provides.  Two objects of a kind alive on one handle with their calls
interleaved, each against its own host tap bit for bit (a base that shared memory between objects would mix them); close twice, then a third object; a fresh
object's state is all zero bytes; a masked reset leaves the other streams' bytes alone.  The YOLO network has no host tap: its reference is the same checkpoint on
an object that was alone on the handle.  The metrics cases carry no sigmas: the OKS sum goes through the device's exp() and is not bit-exact
(tests/test_gpu_metrics.py bounds it), every other word is."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from easy_vitpose_amd import VitPoseHip
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devcoco import CocoEvalCfg, cocoeval_tap
from easy_vitpose_amd.devcoco import new_state as coco_state
from easy_vitpose_amd.devdetect import DeviceDetector, HostDetector
from easy_vitpose_amd.devmetrics import metrics_tap
from easy_vitpose_amd.devmetrics import new_state as metrics_state
from easy_vitpose_amd.devsmooth import DeviceSmoother, HostSmoother, SmoothCfg
from easy_vitpose_amd.devtracker import DeviceTracker, HostTracker, TrackCfg
from easy_vitpose_amd.devyolo import DeviceYolo, synth_yolo
from easy_vitpose_amd.synth import synthetic_state_dict
import cocoeval_cases as cc
import detect_cases as dc
import metrics_cases as mc
import track_cases as tc
import yolo_cases as YC

pytestmark = pytest.mark.gpu
KINDS = ('tracker', 'smoother', 'metrics', 'cocoeval', 'detector', 'yolo')
STATEFUL = KINDS[:4]


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def _kpts(seed, n, K=2):
    rng = np.random.default_rng(seed)
    kp = rng.uniform(5, 90, (n, K, 3)).astype(np.float32)
    kp[..., 2] = rng.uniform(0.3, 1.0, (n, K))
    return kp


class Pair:
    """One object of a kind with its host model: `make(eng, which)` -> Pair; `step(i)` runs call i on both and asserts the outputs bit for bit; `check()` asserts
    the whole state (the kinds that have one)."""

    def __init__(self, dev, step, state=None):
        self.dev, self.step, self.check = dev, step, (lambda: None) if state is None else (lambda: _same(dev.state(), state()))


def _same(got, want):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _tracker(eng, which):   # 3 streams, 3 detections a call, one per stream
    cfg = TrackCfg(1, 1, tc.IOU_THRESHOLD, 3)
    dev, tap = DeviceTracker(eng, cfg), HostTracker(cfg)
    dets, fi = tc.far_people(3, 20 + which, x0=50.0 * which), np.arange(3, dtype=np.int32)

    def step(i):
        d = dets + np.float32(2 * i) * np.array([1, 0, 1, 0, 0], np.float32)
        for g, w in zip(dev.update_host(d, frame_index=fi, n_out=8), tap.update(d, frame_index=fi, n_out=8)):
            assert tc.same_bits(g, w)
    return Pair(dev, step, tap.state)


def _smoother(eng, which):   # K = 2, 2 rows, 3 streams
    cfg = SmoothCfg(n_streams=3)
    dev, tap = DeviceSmoother(eng, 2, cfg), HostSmoother(2, cfg)
    ids, stream = np.array([7, 9], np.int32), np.array([0, 2], np.int32) if which else np.array([1, 2], np.int32)

    def step(i):
        kp = _kpts(100 * which + i, 2)
        got, want = dev.update_host(kp, ids, stream), tap.update(kp, ids, stream)
        assert tc.same_bits(got[0], want[0]) and got[1].tolist() == want[1].tolist()
    return Pair(dev, step, tap.state)


def _metrics(eng, which):   # K = 2, 3 rows
    cs = mc.case(700 + which, 3, 2, oks=False)
    dev, want = eng.metrics(cs['cfg']), metrics_state(cs['cfg'])

    def step(i):
        dist, _ = dev.update_host(**mc.inputs(cs))
        assert dist.tobytes() == metrics_tap(want, cs['cfg'], **mc.inputs(cs))[0].tobytes()
    return Pair(dev, step, lambda: want)


def _cocoeval(eng, which):   # K = 2, max_records 8
    cs = cc._totals(3 + which, K=2, max_records=8)
    dev, want = eng.cocoeval(cs['cfg']), coco_state(cs['cfg'])

    def step(i):
        call = cc.inputs(cs['calls'][0])
        assert dev.update_host(**call).tobytes() == cocoeval_tap(want, cs['cfg'], **call).tobytes()
    return Pair(dev, step, lambda: want)


def _detector(eng, which):   # one image; A = 1, the smallest anchor count of the kernel sizes, and A = 63 on the second object
    cfg, pred, frames_hw, input_hw, n_out = dc.size_case(2 * which)
    pred = pred[:1]
    dev, want = DeviceDetector(eng, cfg), HostDetector(cfg).detect(pred, frames_hw, input_hw, n_out)

    def step(i):
        for g, w in zip(dev.detect_host(pred, frames_hw, input_hw, n_out), want):
            assert dc.same_bits(g, w)
    return Pair(dev, step)


def _yolo_state(which):
    return YC.state('n_32x32x1') if which == 0 else synth_yolo('n', 80, 40 + which)


_YOLO_ALONE = {}


def _yolo(eng, which):   # the smallest synthetic checkpoint, 32 x 32, one image
    x = torch.from_numpy(YC.images('n_32x32x1')).cuda()
    if which not in _YOLO_ALONE:   # the reference: this checkpoint on an object that is alone on the handle (the callers ask for it before they hold another one)
        alone = DeviceYolo(eng, _yolo_state(which), (32, 32))
        _YOLO_ALONE[which] = alone(x).clone()
        alone.close()
    dev = DeviceYolo(eng, _yolo_state(which), (32, 32))

    def step(i):
        assert torch.equal(dev(x), _YOLO_ALONE[which])
    return Pair(dev, step)


MAKE = dict(tracker=_tracker, smoother=_smoother, metrics=_metrics, cocoeval=_cocoeval, detector=_detector, yolo=_yolo)


@pytest.mark.parametrize('kind', KINDS)
def test_two_objects_on_one_handle_with_interleaved_calls(eng, kind):
    if kind == 'yolo':
        for which in (0, 1):   # both references first, each from an object alone on the handle
            MAKE[kind](eng, which).dev.close()
        assert not torch.equal(_YOLO_ALONE[0], _YOLO_ALONE[1])
    a, b = MAKE[kind](eng, 0), MAKE[kind](eng, 1)
    for i in range(3):
        a.step(i)
        b.step(i)
        a.check()
        b.check()
    b.dev.close()
    a.step(3)   # the survivor still owns its memory
    a.check()
    a.dev.close()


@pytest.mark.parametrize('kind', KINDS)
def test_close_twice_then_a_third_object(eng, kind):
    first, second = MAKE[kind](eng, 0), MAKE[kind](eng, 1)
    for p in (first, second):
        p.dev.close()
        assert p.dev._obj is None
        p.dev.close()   # nothing left to destroy: a no-op
        assert p.dev._obj is None
    third = MAKE[kind](eng, 0)
    third.step(0)
    third.check()
    third.dev.close()


@pytest.mark.parametrize('kind', STATEFUL)
def test_a_fresh_object_starts_from_zero_bytes(eng, kind):
    used = MAKE[kind](eng, 1)   # a used object freed first: the next allocation may be handed its memory
    used.step(0)
    used.dev.close()
    fresh = MAKE[kind](eng, 0)
    assert not fresh.dev.state().tobytes().strip(b'\0')
    fresh.dev.close()


@pytest.mark.parametrize('kind', ('tracker', 'smoother'))
def test_masked_reset_of_stream_1_leaves_streams_0_and_2_alone(eng, kind):
    """tests/test_gpu_track.py and test_gpu_smooth.py assert single fields of the three streams after reset([1]); this is every byte"""
    p = MAKE[kind](eng, 0)
    if kind == 'smoother':   # rows on all three streams
        kp = _kpts(5, 3)
        p.dev.update_host(kp, np.array([1, 2, 3], np.int32), np.array([0, 1, 2], np.int32))
    else:
        p.step(0)
    before = p.dev.state()
    assert all(before[s].tobytes().strip(b'\0') for s in range(3))
    p.dev.reset([1])
    torch.cuda.synchronize()
    after = p.dev.state()
    assert after[0].tobytes() == before[0].tobytes() and after[2].tobytes() == before[2].tobytes() and not after[1].tobytes().strip(b'\0')
    p.dev.close()
