"""CPU: what the stage classes share (easy_vitpose_amd/_stage.py).  Part one: every refusal the device entries of the stages make in Python, before any C call,
with its exception type and its whole message written out.  The stages are built without a library (`object.__new__` plus the attributes the checks read) on a
stand-in engine, so a call that got past its refusal would fail in another way; a tensor "on the device" is a CPU tensor whose class reports a CUDA device, which is
all the checks look at.  The refusals behind an allocation on the device (the tracker's `n_dets`) are not reachable here.  Part two: `mask_of`, `ptr` and the
stream of a stage."""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

from easy_vitpose_amd import _stage
from easy_vitpose_amd.cropprep import Frame
from easy_vitpose_amd.devcoco import CocoEvalCfg, DeviceCocoEval
from easy_vitpose_amd.devdetect import DetectCfg, DeviceDetector
from easy_vitpose_amd.devletterbox import DeviceLetterbox, LetterboxCfg
from easy_vitpose_amd.devmetrics import DeviceMetrics, MetricsCfg
from easy_vitpose_amd.devorient import DeviceOrient
from easy_vitpose_amd.devsmooth import DeviceSmoother, SmoothCfg
from easy_vitpose_amd.devtracker import DeviceTracker, RowBound, TrackCfg, mask_of
from easy_vitpose_amd.devyolo import DeviceYolo

F32, I32, F16, U8 = torch.float32, torch.int32, torch.float16, torch.uint8


class OnCuda(torch.Tensor):
    """a CPU tensor that says it lives on cuda:`_index`"""
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device('cuda', getattr(self, '_index', 0)))


def cuda(t, index=0):
    t = t.as_subclass(OnCuda)
    t._index = index
    return t


def z(*shape, dtype=F32, index=0):
    return cuda(torch.zeros(shape, dtype=dtype), index)


def stage(cls, **attrs):
    s = object.__new__(cls)
    s.engine = types.SimpleNamespace(lib=None, device_id=0, _h=None, K=17)
    s.lib = None
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


TRK = stage(DeviceTracker, cfg=TrackCfg(n_streams=2), _bound=RowBound(1, 2))
SMO = stage(DeviceSmoother, cfg=SmoothCfg(n_streams=2), K=17)
MET = stage(DeviceMetrics, cfg=MetricsCfg(n_joints=17), nbytes=4096)
COCO = stage(DeviceCocoEval, cfg=CocoEvalCfg(17, 64))
DET = stage(DeviceDetector, cfg=DetectCfg(nc=3, dtype='fp16', max_anchors=8, max_images=2))
YOLO = stage(DeviceYolo, in_hw=(32, 32), input_layout='nchw', max_images=2)
LB = DeviceLetterbox(types.SimpleNamespace(lib=None, device_id=0, _h=None), LetterboxCfg((16, 16)))
ORI = DeviceOrient(types.SimpleNamespace(lib=None, device_id=0, _h=None))
KP, KP1 = z(2, 17, 3), z(2, 17, 3, index=1)
HOST_RGB = Frame.rgb(np.zeros((4, 6, 3), np.uint8))
DEV_RGB, DEV1_RGB = Frame.rgb(z(4, 6, 3, dtype=U8)), Frame.rgb(z(4, 6, 3, dtype=U8, index=1))

REFUSALS = [
    # ---- tracker update
    ('track dets numpy', lambda: TRK.update(np.zeros((3, 5), np.float32)), TypeError, 'dets: a float32 torch CUDA tensor expected'),
    ('track dets cpu', lambda: TRK.update(torch.zeros(3, 5)), TypeError, 'dets: a float32 torch CUDA tensor expected'),
    ('track dets dtype', lambda: TRK.update(z(3, 5, dtype=torch.float64)), TypeError, 'dets: a float32 torch CUDA tensor expected'),
    ('track dets columns', lambda: TRK.update(z(3, 4)), ValueError, 'dets: [n, >= 5] with contiguous rows on cuda:0 expected, got (3, 4) on cuda:0'),
    ('track dets ndim', lambda: TRK.update(z(5)), ValueError, 'dets: [n, >= 5] with contiguous rows on cuda:0 expected, got (5,) on cuda:0'),
    ('track dets rows', lambda: TRK.update(cuda(torch.zeros(6, 3).t())), ValueError, 'dets: [n, >= 5] with contiguous rows on cuda:0 expected, got (3, 6) on cuda:0'),
    ('track dets device', lambda: TRK.update(z(3, 5, index=1)), ValueError, 'dets: [n, >= 5] with contiguous rows on cuda:0 expected, got (3, 5) on cuda:1'),
    ('track frame_index cpu', lambda: TRK.update(z(3, 5), torch.zeros(3, dtype=I32)), TypeError, 'frame_index: an int32 torch CUDA tensor expected'),
    ('track frame_index dtype', lambda: TRK.update(z(3, 5), z(3)), TypeError, 'frame_index: an int32 torch CUDA tensor expected'),
    ('track frame_index shape', lambda: TRK.update(z(3, 5), z(2, dtype=I32)), ValueError, 'frame_index: contiguous [3] on cuda:0 expected, got (2,) on cuda:0'),
    ('track frame_index view', lambda: TRK.update(z(3, 5), z(6, dtype=I32)[::2]), ValueError, 'frame_index: contiguous [3] on cuda:0 expected, got (3,) on cuda:0'),
    ('track frame_index device', lambda: TRK.update(z(3, 5), z(3, dtype=I32, index=1)), ValueError, 'frame_index: contiguous [3] on cuda:0 expected, got (3,) on cuda:1'),
    ('track step', lambda: TRK.update(z(3, 5), step=[2]), ValueError, 'a stream beyond n_streams = 2 in [2]'),
    ('track n_out', lambda: TRK.update(z(3, 5), n_out=-1), ValueError, 'n_out < 0'),
    # ---- smoother update
    ('smooth kpts cpu', lambda: SMO.update(torch.zeros(2, 17, 3), z(2, dtype=I32)), TypeError, 'kpts: a float32 torch CUDA tensor expected'),
    ('smooth kpts joints', lambda: SMO.update(z(2, 16, 3), z(2, dtype=I32)), ValueError, 'kpts: contiguous [n, 17, 3] on cuda:0 expected, got (2, 16, 3) on cuda:0'),
    ('smooth kpts view', lambda: SMO.update(z(4, 17, 3)[::2], z(2, dtype=I32)), ValueError, 'kpts: contiguous [n, 17, 3] on cuda:0 expected, got (2, 17, 3) on cuda:0'),
    ('smooth kpts device', lambda: SMO.update(KP1, z(2, dtype=I32)), ValueError, 'kpts: contiguous [n, 17, 3] on cuda:0 expected, got (2, 17, 3) on cuda:1'),
    ('smooth ids none', lambda: SMO.update(KP, None), TypeError, 'ids: an int32 torch CUDA tensor expected'),
    ('smooth ids dtype', lambda: SMO.update(KP, z(2)), TypeError, 'ids: an int32 torch CUDA tensor expected'),
    ('smooth ids shape', lambda: SMO.update(KP, z(3, dtype=I32)), ValueError, 'ids: contiguous [2] on cuda:0 expected, got (3,) on cuda:0'),
    ('smooth stream cpu', lambda: SMO.update(KP, z(2, dtype=I32), torch.zeros(2, dtype=I32)), TypeError, 'stream: an int32 torch CUDA tensor expected'),
    ('smooth stream view', lambda: SMO.update(KP, z(2, dtype=I32), z(4, dtype=I32)[::2]), ValueError, 'stream: contiguous [2] on cuda:0 expected, got (2,) on cuda:0'),
    ('smooth rank shape', lambda: SMO.update(KP, z(2, dtype=I32), None, z(2, 1, dtype=I32)), ValueError, 'rank: contiguous [2] on cuda:0 expected, got (2, 1) on cuda:0'),
    ('smooth out', lambda: SMO.update(KP, z(2, dtype=I32), out=z(2, 17, 2)), ValueError, 'out: a contiguous float32 tensor like kpts on cuda:0 expected'),
    ('smooth out type', lambda: SMO.update(KP, z(2, dtype=I32), out=np.zeros((2, 17, 3), np.float32)), ValueError, 'out: a contiguous float32 tensor like kpts on cuda:0 expected'),
    # ---- metrics update / snapshot
    ('metrics pred numpy', lambda: MET.update(np.zeros((2, 17, 3), np.float32), KP), TypeError, 'pred: a float32 torch CUDA tensor [n, K, 3] expected'),
    ('metrics pred ndim', lambda: MET.update(z(2, 51), KP), TypeError, 'pred: a float32 torch CUDA tensor [n, K, 3] expected'),
    ('metrics pred cpu', lambda: MET.update(torch.zeros(2, 17, 3), KP), TypeError, 'pred: a float32 torch CUDA tensor expected'),
    ('metrics pred joints', lambda: MET.update(z(2, 16, 3), KP), ValueError, 'pred: contiguous [2, 17, 3] on cuda:0 expected, got (2, 16, 3) on cuda:0'),
    ('metrics gt none', lambda: MET.update(KP, None), TypeError, 'gt: a float32 torch CUDA tensor expected'),
    ('metrics gt rows', lambda: MET.update(KP, z(3, 17, 3)), ValueError, 'gt: contiguous [2, 17, 3] on cuda:0 expected, got (3, 17, 3) on cuda:0'),
    ('metrics gt device', lambda: MET.update(KP, KP1), ValueError, 'gt: contiguous [2, 17, 3] on cuda:0 expected, got (2, 17, 3) on cuda:1'),
    ('metrics norm shape', lambda: MET.update(KP, KP, norm=z(2)), ValueError, 'norm: contiguous [2, 2] on cuda:0 expected, got (2,) on cuda:0'),
    ('metrics area dtype', lambda: MET.update(KP, KP, area=z(2, dtype=I32)), TypeError, 'area: a float32 torch CUDA tensor expected'),
    ('metrics rank dtype', lambda: MET.update(KP, KP, rank=z(2)), TypeError, 'rank: an int32 torch CUDA tensor expected'),
    ('metrics set view', lambda: MET.update(KP, KP, set=z(4, dtype=I32)[::2]), ValueError, 'set: contiguous [2] on cuda:0 expected, got (2,) on cuda:0'),
    ('metrics dist shape', lambda: MET.update(KP, KP, dist=z(2, 16)), ValueError, 'dist: contiguous [2, 17] on cuda:0 expected, got (2, 16) on cuda:0'),
    ('metrics oks cpu', lambda: MET.update(KP, KP, oks=torch.zeros(2)), TypeError, 'oks: a float32 torch CUDA tensor expected'),
    ('metrics snapshot out', lambda: MET.snapshot(z(4095, dtype=U8)), ValueError, 'out: a contiguous uint8 tensor of 4096 bytes on cuda:0 expected'),
    ('metrics snapshot type', lambda: MET.snapshot(z(4096)), ValueError, 'out: a contiguous uint8 tensor of 4096 bytes on cuda:0 expected'),
    # ---- cocoeval update / accumulate
    ('coco kpts ndim', lambda: COCO.update(z(2, 51), z(2)), TypeError, 'kpts: a float32 torch CUDA tensor [n, K, 3] expected'),
    ('coco kpts cpu', lambda: COCO.update(torch.zeros(2, 17, 3), z(2)), TypeError, 'kpts: a float32 torch CUDA tensor expected'),
    ('coco kpts joints', lambda: COCO.update(z(2, 16, 3), z(2)), ValueError, 'kpts: contiguous [2, 17, 3] on cuda:0 expected, got (2, 16, 3) on cuda:0'),
    ('coco score none', lambda: COCO.update(KP, None), TypeError, 'score: a float32 torch CUDA tensor expected'),
    ('coco score shape', lambda: COCO.update(KP, z(3)), ValueError, 'score: contiguous [2] on cuda:0 expected, got (3,) on cuda:0'),
    ('coco frame dtype', lambda: COCO.update(KP, z(2), frame=z(2)), TypeError, 'frame: an int32 torch CUDA tensor expected'),
    ('coco rank device', lambda: COCO.update(KP, z(2), rank=z(2, dtype=I32, index=1)), ValueError, 'rank: contiguous [2] on cuda:0 expected, got (2,) on cuda:1'),
    ('coco gt_kpts joints', lambda: COCO.update(KP, z(2), gt_kpts=z(1, 16, 3)), ValueError, 'gt_kpts: contiguous [1, 17, 3] on cuda:0 expected, got (1, 16, 3) on cuda:0'),
    ('coco gt_box needed', lambda: COCO.update(KP, z(2), gt_kpts=z(1, 17, 3)), TypeError, 'gt_box: a float32 torch CUDA tensor expected'),
    ('coco gt_box shape', lambda: COCO.update(KP, z(2), gt_kpts=z(1, 17, 3), gt_box=z(1, 5)), ValueError, 'gt_box: contiguous [1, 4] on cuda:0 expected, got (1, 5) on cuda:0'),
    ('coco gt_area needed', lambda: COCO.update(KP, z(2), gt_kpts=z(1, 17, 3), gt_box=z(1, 4)), TypeError, 'gt_area: a float32 torch CUDA tensor expected'),
    ('coco gt_flags shape', lambda: COCO.update(KP, z(2), gt_kpts=z(1, 17, 3), gt_box=z(1, 4), gt_area=z(1), gt_flags=z(2, dtype=I32)), ValueError,
     'gt_flags: contiguous [1] on cuda:0 expected, got (2,) on cuda:0'),
    ('coco gt_frame dtype', lambda: COCO.update(KP, z(2), gt_kpts=z(1, 17, 3), gt_box=z(1, 4), gt_area=z(1), gt_frame=z(1)), TypeError, 'gt_frame: an int32 torch CUDA tensor expected'),
    ('coco match shape', lambda: COCO.update(KP, z(2), match=z(2, 9, dtype=I32)), ValueError, 'match: contiguous [2, 10] on cuda:0 expected, got (2, 9) on cuda:0'),
    ('coco accumulate out', lambda: COCO.accumulate(z(8, dtype=U8)), ValueError, None),   # the text carries the result blob's size: checked below
    # ---- detector detect
    ('detect pred cpu', lambda: DET.detect(torch.zeros(1, 7, 5, dtype=F16), (4, 4), (8, 8)), TypeError, 'pred: a float16 torch CUDA tensor expected'),
    ('detect pred dtype', lambda: DET.detect(z(1, 7, 5), (4, 4), (8, 8)), TypeError, 'pred: a float16 torch CUDA tensor expected'),
    ('detect pred view', lambda: DET.detect(z(1, 7, 10, dtype=F16)[:, :, ::2], (4, 4), (8, 8)), ValueError, 'pred: a contiguous tensor on cuda:0 expected, got (1, 7, 5) on cuda:0'),
    ('detect pred device', lambda: DET.detect(z(1, 7, 5, dtype=F16, index=1), (4, 4), (8, 8)), ValueError, 'pred: a contiguous tensor on cuda:0 expected, got (1, 7, 5) on cuda:1'),
    ('detect pred channels', lambda: DET.detect(z(1, 6, 5, dtype=F16), (4, 4), (8, 8)), ValueError, 'pred: [n, 7, A] expected, got (1, 6, 5)'),
    ('detect pred images', lambda: DET.detect(z(3, 7, 5, dtype=F16), (4, 4), (8, 8)), ValueError, 'pred: 3 images, the detector takes 2'),
    ('detect pred anchors', lambda: DET.detect(z(1, 7, 9, dtype=F16), (4, 4), (8, 8)), ValueError, 'pred: A = 9 outside 1..8'),
    ('detect n_out', lambda: DET.detect(z(1, 7, 5, dtype=F16), (4, 4), (8, 8), n_out=-1), ValueError, 'n_out < 0'),
    # ---- YOLO forward
    ('yolo cpu', lambda: YOLO(torch.zeros(1, 3, 32, 32, dtype=F16)), TypeError, "DeviceYolo: an fp16 torch CUDA tensor expected (the letterbox stage's fp16 output)"),
    ('yolo dtype', lambda: YOLO(z(1, 3, 32, 32)), TypeError, "DeviceYolo: an fp16 torch CUDA tensor expected (the letterbox stage's fp16 output)"),
    ('yolo view', lambda: YOLO(z(1, 3, 32, 64, dtype=F16)[..., ::2]), ValueError, 'DeviceYolo: a contiguous tensor on cuda:0 expected'),
    ('yolo device', lambda: YOLO(z(1, 3, 32, 32, dtype=F16, index=1)), ValueError, 'DeviceYolo: a contiguous tensor on cuda:0 expected'),
    ('yolo images', lambda: YOLO(z(3, 3, 32, 32, dtype=F16)), ValueError, "DeviceYolo: ('n', 3, 32, 32) with n <= 2 expected, got (3, 3, 32, 32)"),
    ('yolo layout', lambda: YOLO(z(1, 32, 32, 3, dtype=F16)), ValueError, "DeviceYolo: ('n', 3, 32, 32) with n <= 2 expected, got (1, 32, 32, 3)"),
    ('yolo ndim', lambda: YOLO(z(3, 32, 32, dtype=F16)), ValueError, "DeviceYolo: ('n', 3, 32, 32) with n <= 2 expected, got (3, 32, 32)"),
    # ---- letterbox
    ('letterbox count', lambda: LB.letterbox([DEV_RGB] * 65), ValueError, 'letterbox: 65 frames, a call takes 64'),
    ('letterbox host count', lambda: LB.letterbox_host([HOST_RGB] * 65), ValueError, 'letterbox: 65 frames, a call takes 64'),
    ('letterbox host frame', lambda: LB.letterbox([DEV_RGB, HOST_RGB]), TypeError, 'frame 1: torch uint8 CUDA tensors expected'),
    ('letterbox device frame', lambda: LB.letterbox_host([HOST_RGB, DEV_RGB]), TypeError, 'frame 1: host planes (numpy arrays) expected'),
    ('letterbox other device', lambda: LB.letterbox([DEV_RGB, DEV1_RGB]), ValueError, 'frame 1 lives on cuda:1, the handle on cuda:0'),
    ('letterbox out cpu', lambda: LB.letterbox([], out=torch.zeros(0, 3, 16, 16, dtype=F16)), TypeError, 'out: a fp16 torch CUDA tensor expected'),
    ('letterbox out dtype', lambda: LB.letterbox([], out=z(0, 3, 16, 16)), TypeError, 'out: a fp16 torch CUDA tensor expected'),
    ('letterbox out shape', lambda: LB.letterbox([], out=z(1, 3, 16, 16, dtype=F16)), ValueError,
     'out: a contiguous tensor of shape (0, 3, 16, 16) on cuda:0 expected, got (1, 3, 16, 16) on cuda:0'),
    ('letterbox out device', lambda: LB.letterbox([], out=z(0, 3, 16, 16, dtype=F16, index=1)), ValueError,
     'out: a contiguous tensor of shape (0, 3, 16, 16) on cuda:0 expected, got (0, 3, 16, 16) on cuda:1'),
    # ---- orient
    ('orient count', lambda: ORI.orient([DEV_RGB] * 65, 1), ValueError, 'orient: 65 frames, a call takes 64'),
    ('orient host count', lambda: ORI.orient_host([HOST_RGB] * 65, 1), ValueError, 'orient: 65 frames, a call takes 64'),
    ('orient host frame', lambda: ORI.orient([HOST_RGB], 1), TypeError, 'frame 0: torch uint8 CUDA tensors expected'),
    ('orient device frame', lambda: ORI.orient_host([DEV_RGB], 1), TypeError, 'frame 0: host planes (numpy arrays) expected'),
    ('orient other device', lambda: ORI.orient([DEV1_RGB], 1), ValueError, 'frame 0 lives on cuda:1, the handle on cuda:0'),
    ('orient codes', lambda: ORI.orient([DEV_RGB], [1, 2]), ValueError, 'orient: 2 codes for 1 frames'),
    ('orient code', lambda: ORI.orient([DEV_RGB], 9), ValueError, None),   # the text lists the code names: checked below
    ('orient out count', lambda: ORI.orient([DEV_RGB], 1, out=[]), ValueError, 'out: 0 frames for 1 frames'),
    ('orient out type', lambda: ORI.orient([DEV_RGB], 1, out=[np.zeros((4, 6, 3), np.uint8)]), TypeError, 'out 0: a Frame expected, got ndarray'),
    ('orient out host', lambda: ORI.orient([DEV_RGB], 1, out=[HOST_RGB]), TypeError, 'out 0: torch uint8 CUDA tensors expected'),
    ('orient out size', lambda: ORI.orient([DEV_RGB], 6, out=[DEV_RGB]), ValueError, 'out 0: a rgb frame of 6 x 4 (bt601) expected, got rgb 4 x 6 (bt601)'),
    ('orient out other device', lambda: ORI.orient([DEV_RGB], 1, out=[DEV1_RGB]), ValueError, 'out 0 lives on cuda:1, the handle on cuda:0'),
]


@pytest.mark.parametrize('call,exc,message', [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusal_of_a_device_entry_by_type_and_message(call, exc, message):
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc
    if message is not None:
        assert str(e.value) == message


def test_the_two_refusals_whose_text_carries_a_table():
    from easy_vitpose_amd.devcoco import RESULT
    from easy_vitpose_amd.devorient import ORIENT_CODES
    with pytest.raises(ValueError) as e:
        COCO.accumulate(z(8, dtype=U8))
    assert str(e.value) == f'out: a contiguous uint8 tensor of {RESULT.itemsize} bytes on cuda:0 expected'
    with pytest.raises(ValueError) as e:
        ORI.orient([DEV_RGB], 9)
    assert str(e.value) == f'frame 0: an orientation code in 1..8 (or one of {sorted(ORIENT_CODES)}) expected, got 9'


def test_check_tensor_passes_what_the_entries_accept():
    dev = torch.device('cuda', 0)
    _stage.check_tensor('a', None, F32, (2,), dev)                                   # absent and not needed
    _stage.check_tensor('a', z(0, 17, 3), F32, ('n', 17, 3), dev, True)              # any row count, none included
    _stage.check_tensor('a', z(3, 6)[:, 4], F32, (3,), dev, True, contiguous=False)  # a column view
    _stage.check_tensor('a', z(1, 6)[:, 4], F32, (1,), dev, True, contiguous=False)  # one element: its stride is never used
    _stage.check_tensor('a', z(2, 7, 5, dtype=F16), F16, None, dev, True)            # any shape
    with pytest.raises(ValueError) as e:
        _stage.check_tensor('a', z(3).expand(2, 3)[:, 0], F32, (2,), dev, True, contiguous=False)   # stride 0
    assert str(e.value) == 'a: [2] with a positive stride on cuda:0 expected, got (2,) on cuda:0'
    with pytest.raises(TypeError) as e:
        _stage.check_tensor('a', None, U8, (2,), dev, True)
    assert str(e.value) == 'a: a uint8 torch CUDA tensor expected'


def test_mask_of():
    assert mask_of(None, 1) == 1 and mask_of(None, 3) == 7 and mask_of(None, 64) == (1 << 64) - 1
    assert mask_of(5, 3) == 5 and mask_of(np.int64(2), 2) == 2 and mask_of(0, 1) == 0
    assert mask_of([0, 2], 3) == 5 and mask_of((63,), 64) == 1 << 63 and mask_of([], 3) == 0 and mask_of(np.array([1, 1]), 2) == 2
    for step, n, text in ((8, 3, 'a stream beyond n_streams = 3 in 8'), (-1, 3, 'a stream beyond n_streams = 3 in -1'), ([3], 3, 'a stream beyond n_streams = 3 in [3]'),
                          ([64], 64, 'stream 64 outside 0..63'), ([-1], 3, 'stream -1 outside 0..63')):
        with pytest.raises(ValueError) as e:
            mask_of(step, n)
        assert str(e.value) == text
    with pytest.raises(TypeError):
        mask_of(True, 3)   # a bool is no mask and no iterable


def test_ptr():
    a, t = np.zeros(3, np.float32), torch.zeros(3)
    assert _stage.ptr(None) is None and _stage.ptr(None, 3) is None
    assert _stage.ptr(a) == a.ctypes.data and _stage.ptr(a, 3) == a.ctypes.data and _stage.ptr(t) == t.data_ptr() and _stage.ptr(t, 3) == t.data_ptr()
    assert _stage.ptr(a, 0) is None and _stage.ptr(t, 0) is None, 'a call without rows passes no address'
    assert _stage.ptr(np.zeros((0, 3), np.float32)) is None, 'an empty numpy array passes no address'


def test_stream_and_close_of_a_stage_on_stubs(monkeypatch):
    asked = []
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda dev=None: asked.append(dev) or types.SimpleNamespace(cuda_stream=1234))
    assert TRK._dev == torch.device('cuda', 0)
    assert TRK._stream() == TRK._stream(None) == 1234 and asked == [torch.device('cuda', 0)] * 2
    assert TRK._stream(types.SimpleNamespace(cuda_stream=77)) == 77 and len(asked) == 2, 'a given stream is taken as it is'
    assert LB._stream() == 1234 and _stage.stream_of(torch.device('cuda', 1)) == 1234 and asked[-1] == torch.device('cuda', 1)
    # create, the per-class alias, close twice, a closed engine
    destroyed = []
    lib = types.SimpleNamespace(create=lambda h, arg, out: out._obj.__setattr__('value', 99) or 0, vp_tracker_destroy=lambda o: destroyed.append(o.value) or 0)
    s = stage(DeviceTracker)
    s.engine._h, s.lib = 5, lib
    assert s._obj is None and s._t is None
    s._create(lib.create, 'cfg')
    assert s._obj.value == 99 and s._t is s._obj
    s.close()
    s.close()
    assert destroyed == [99] and s._obj is None and s._t is None
    s._create(lib.create, 'cfg')
    s.engine._h = None   # the engine was closed first: the object is not destroyed behind it
    s.close()
    assert destroyed == [99] and s._obj is None
