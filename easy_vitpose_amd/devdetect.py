"""The detector stage on the device (vp_detect_stream; semantics in csrc/detgeom.h): a detector's raw head tensor to the [n, 6] box rows the tracker and the boxes
entries take in place -- best-class pick, confidence threshold, class filter, greedy box NMS, letterbox undone.  Configuration, the ctypes layer, ``DeviceDetector``
and ``HostDetector`` (the host tap vp_dbg_detect_host: the model the device is tested against, never a fallback).

``DeviceDetector.detect`` is stream-ordered on torch's current stream and never synchronises: its rows, image index and ``count[-1:]`` pass in place to
``DeviceTracker.update(rows, image, n_dets=count[-1:])``.  Rows beyond the total are "absent" (box NaN, score 0, class -1, image -1, anchor -1).

The detector network itself stays third-party.  The letterboxing of a frame into its input is the letterbox stage (``devletterbox``): ``detect`` takes the
undo table that stage returned in place of ``frames_hw, input_hw``; ``letterbox_params`` computes the same numbers (ultralytics' scale_boxes) from the sizes alone.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import numbers

import numpy as np

from . import _capi as capi
from ._stage import DeviceStage, check_tensor, handle_alias

MAX_IMAGES = 64
MAX_CLASSES = 256
MAX_CAND = 2048
MAX_DET = 1024
MAX_ANCHORS = 1 << 20
FLAG_CAND, FLAG_ROWS, FLAG_BAD_BOX = 1, 4, 8
DTYPES = {'fp32': 0, 'fp16': 1}
NP_DTYPES = {'fp32': np.float32, 'fp16': np.float16}


def _integer(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))


def _real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_)) and math.isfinite(v)


@dataclasses.dataclass(frozen=True)
class DetectCfg:
    """``nc``: classes of the head ([4 + nc] channels); ``dtype``: 'fp16' or 'fp32'; ``layout``: 0 = [n, 4 + nc, A] (YOLOv8's export), 1 = [n, A, 4 + nc];
    ``conf_thr``, ``iou_thr``, ``extent``: the float32 values the device compares with (extent 0: ultralytics' continuous IoU, 1: the reference's pixel
    convention); ``agnostic``: boxes of different classes suppress each other; ``max_det``: picks per image; ``classes``: None (all), a list of class indices or a
    ``det_class`` name of ``inference.DETC_TO_YOLO_YOLOC``; ``max_anchors`` / ``max_images``: the largest call."""
    nc: int = 80
    dtype: str = 'fp16'
    layout: int = 0
    conf_thr: float = 0.35
    iou_thr: float = 0.7
    extent: float = 0.0
    agnostic: bool = False
    max_det: int = 300
    classes: object = None
    max_anchors: int = MAX_ANCHORS
    max_images: int = MAX_IMAGES

    def __post_init__(self):
        if not (_integer(self.nc) and 1 <= self.nc <= MAX_CLASSES):
            raise ValueError(f'DetectCfg: nc in 1..{MAX_CLASSES} expected, got {self.nc!r}')
        if self.dtype not in DTYPES:
            raise ValueError(f"DetectCfg: dtype 'fp16' or 'fp32' expected, got {self.dtype!r}")
        if not (_integer(self.layout) and self.layout in (0, 1)):
            raise ValueError(f'DetectCfg: layout 0 or 1 expected, got {self.layout!r}')
        if not (_real(self.conf_thr) and float(np.float32(self.conf_thr)) >= 0.0 and math.isfinite(float(np.float32(self.conf_thr)))):
            raise ValueError(f'DetectCfg: a finite conf_thr >= 0 expected, got {self.conf_thr!r}')
        if not (_real(self.iou_thr) and 0.0 <= float(np.float32(self.iou_thr)) <= 1.0):
            raise ValueError(f'DetectCfg: iou_thr in [0, 1] expected, got {self.iou_thr!r}')
        if not (_real(self.extent) and float(np.float32(self.extent)) >= 0.0 and math.isfinite(float(np.float32(self.extent)))):
            raise ValueError(f'DetectCfg: a finite extent >= 0 expected, got {self.extent!r}')
        if not isinstance(self.agnostic, (bool, np.bool_)):
            raise ValueError(f'DetectCfg: agnostic True or False expected, got {self.agnostic!r}')
        if not (_integer(self.max_det) and 1 <= self.max_det <= MAX_DET):
            raise ValueError(f'DetectCfg: max_det in 1..{MAX_DET} expected, got {self.max_det!r}')
        if not (_integer(self.max_anchors) and 1 <= self.max_anchors <= MAX_ANCHORS):
            raise ValueError(f'DetectCfg: max_anchors in 1..{MAX_ANCHORS} expected, got {self.max_anchors!r}')
        if not (_integer(self.max_images) and 1 <= self.max_images <= MAX_IMAGES):
            raise ValueError(f'DetectCfg: max_images in 1..{MAX_IMAGES} expected, got {self.max_images!r}')
        cl = self.classes
        if isinstance(cl, str):
            from .inference import DETC_TO_YOLO_YOLOC
            if cl not in DETC_TO_YOLO_YOLOC:
                raise ValueError(f'DetectCfg: classes: unknown det_class {cl!r}')
            cl = DETC_TO_YOLO_YOLOC[cl]
        if cl is None:
            cl = range(int(self.nc))
        cl = tuple(cl)
        if not cl or not all(_integer(c) and 0 <= c < self.nc for c in cl):
            raise ValueError(f'DetectCfg: classes: a non-empty list of class indices in 0..{int(self.nc) - 1} expected, got {self.classes!r}')
        for name in ('nc', 'layout', 'max_det', 'max_anchors', 'max_images'):
            object.__setattr__(self, name, int(getattr(self, name)))
        for name in ('conf_thr', 'iou_thr', 'extent'):   # the values the device compares with
            object.__setattr__(self, name, float(np.float32(getattr(self, name))))
        object.__setattr__(self, 'agnostic', bool(self.agnostic))
        object.__setattr__(self, 'classes', tuple(sorted(set(int(c) for c in cl))))


def c_config(cfg: DetectCfg):
    if not isinstance(cfg, DetectCfg):
        raise TypeError(f'a DetectCfg expected, got {type(cfg).__name__}')
    mask = (C.c_uint32 * 8)()
    for c in cfg.classes:
        mask[c >> 5] |= 1 << (c & 31)
    return capi.vp_det_cfg(cfg.nc, cfg.max_anchors, cfg.max_images, DTYPES[cfg.dtype], cfg.layout, cfg.conf_thr, cfg.iou_thr, cfg.extent, int(cfg.agnostic), cfg.max_det, mask)


def letterbox_params(frame_hw, input_hw):
    """(gain, pad_x, pad_y) of a frame of (h, w) letterboxed into a detector input of (in_h, in_w), as ultralytics' scale_boxes computes them:
    gain = min(in_h / h, in_w / w), pad = round((in - side * gain) / 2 - 0.1)."""
    h, w = (int(v) for v in frame_hw)
    in_h, in_w = (int(v) for v in input_hw)
    if min(h, w, in_h, in_w) < 1:
        raise ValueError(f'letterbox_params: positive sizes expected, got {frame_hw!r} into {input_hw!r}')
    gain = min(in_h / h, in_w / w)
    return gain, float(round((in_w - w * gain) / 2 - 0.1)), float(round((in_h - h * gain) / 2 - 0.1))


def image_table(frames_hw, input_hw, n_images: int):
    """the C table of a call: `frames_hw` = one (h, w) for every image or [n_images] of them; with `input_hw` None, `frames_hw` is the table itself as the
    letterbox stage returned it (float32 [n_images, 5] rows of (gain, pad_x, pad_y, frame_w, frame_h))"""
    if input_hw is None:
        rows = np.asarray(frames_hw)
        if rows.dtype != np.float32 or rows.shape != (n_images, 5):
            raise ValueError(f'table: float32 [{n_images}, 5] rows (gain, pad_x, pad_y, frame_w, frame_h) expected, got {rows.dtype} {rows.shape}')
        tab = (capi.vp_det_image * max(n_images, 1))()
        for i in range(n_images):
            tab[i] = capi.vp_det_image(*(float(v) for v in rows[i]))
        return tab
    hw = np.asarray(frames_hw, dtype=np.int64)
    if hw.shape == (2,):
        hw = np.broadcast_to(hw, (n_images, 2))
    if hw.shape != (n_images, 2):
        raise ValueError(f'frames_hw: (h, w) or [{n_images}, 2] expected, got shape {hw.shape}')
    tab = (capi.vp_det_image * max(n_images, 1))()
    for i in range(n_images):
        g, px, py = letterbox_params(hw[i], input_hw)
        tab[i] = capi.vp_det_image(g, px, py, float(hw[i, 1]), float(hw[i, 0]))
    return tab


def _pred_shape(cfg: DetectCfg, shape):
    """(n_images, A) of a head tensor of `shape`"""
    C_ = 4 + cfg.nc
    want = '[n, %d, A]' % C_ if cfg.layout == 0 else '[n, A, %d]' % C_
    if len(shape) != 3 or shape[1 if cfg.layout == 0 else 2] != C_:
        raise ValueError(f'pred: {want} expected, got {tuple(shape)}')
    n, A = int(shape[0]), int(shape[2 if cfg.layout == 0 else 1])
    if n > cfg.max_images:
        raise ValueError(f'pred: {n} images, the detector takes {cfg.max_images}')
    if not 1 <= A <= cfg.max_anchors:
        raise ValueError(f'pred: A = {A} outside 1..{cfg.max_anchors}')
    return n, A


def _host_out(n_out: int, n_images: int):
    return (np.empty((n_out, 6), np.float32), np.empty(n_out, np.int32), np.empty(n_out, np.int32), np.empty(n_images + 1, np.int32), np.empty(n_images, np.int32))


def _host_pred(cfg: DetectCfg, pred):
    pred = np.asarray(pred)
    if pred.dtype != NP_DTYPES[cfg.dtype]:
        raise TypeError(f'pred: {cfg.dtype} expected, got {pred.dtype}')
    return np.ascontiguousarray(pred)


class HostDetector:
    """csrc/detgeom.h run serially through the tap vp_dbg_detect_host: the model the device is tested against, never a fallback."""

    def __init__(self, cfg: DetectCfg):
        self.cfg, self._c = cfg, c_config(cfg)
        self.lib = capi.load_library()

    def detect(self, pred, frames_hw, input_hw=None, n_out=None):
        pred = _host_pred(self.cfg, pred)
        n, A = _pred_shape(self.cfg, pred.shape)
        n_out = n * self.cfg.max_det if n_out is None else int(n_out)
        out = _host_out(max(n_out, 0), n)
        capi.check(self.lib.vp_dbg_detect_host(C.byref(self._c), pred.ctypes.data if n else None, A, image_table(frames_hw, input_hw, n), n,
                                               *[a.ctypes.data for a in out[:3]], n_out, out[3].ctypes.data, out[4].ctypes.data))
        return out


class DeviceDetector(DeviceStage):
    _destroy, _d = 'vp_detector_destroy', handle_alias

    def __init__(self, engine, cfg: DetectCfg = DetectCfg()):
        super().__init__(engine)
        self.cfg, self._c = cfg, c_config(cfg)
        self._create(self.lib.vp_detector_create, C.byref(self._c))

    def detect(self, pred, frames_hw, input_hw=None, n_out=None):
        """The head `pred` (a contiguous torch CUDA tensor of the configured dtype and layout, n images) on torch's current stream, no synchronisation.
        `frames_hw`: (h, w) of the frames, one pair or one per image; `input_hw`: the detector's input size -- or `detect(pred, table)` with the undo table
        `DeviceLetterbox.letterbox` returned (float32 [n, 5]).  Returns (rows float32 [n_out, 6] =
        (x1, y1, x2, y2, score, class) in frame pixels, image int32 [n_out], anchor int32 [n_out], count int32 [n + 1], flags int32 [n]) device tensors;
        n_out defaults to n * max_det, which cuts nothing."""
        import torch
        dev = self._dev
        check_tensor('pred', pred, torch.float16 if self.cfg.dtype == 'fp16' else torch.float32, None, dev, True)
        n, A = _pred_shape(self.cfg, pred.shape)
        n_out = n * self.cfg.max_det if n_out is None else int(n_out)
        if n_out < 0:
            raise ValueError('n_out < 0')
        rows = torch.empty((n_out, 6), dtype=torch.float32, device=dev)
        image = torch.empty((n_out,), dtype=torch.int32, device=dev)
        anchor = torch.empty((n_out,), dtype=torch.int32, device=dev)
        count = torch.empty((n + 1,), dtype=torch.int32, device=dev)
        flags = torch.empty((n,), dtype=torch.int32, device=dev)
        self._check(self.lib.vp_detect_stream(self._obj, pred.data_ptr() if n else None, A, image_table(frames_hw, input_hw, n), n, rows.data_ptr(), image.data_ptr(),
                                              anchor.data_ptr(), n_out, count.data_ptr(), flags.data_ptr(), self._stream()))
        return rows, image, anchor, count, flags

    def detect_host(self, pred, frames_hw, input_hw=None, n_out=None):
        """`detect` on numpy arrays (vp_detect: upload, the same kernels, download, synchronous)."""
        pred = _host_pred(self.cfg, pred)
        n, A = _pred_shape(self.cfg, pred.shape)
        n_out = n * self.cfg.max_det if n_out is None else int(n_out)
        out = _host_out(max(n_out, 0), n)
        self._check(self.lib.vp_detect(self._obj, pred.ctypes.data if n else None, A, image_table(frames_hw, input_hw, n), n, *[a.ctypes.data for a in out[:3]], n_out,
                                       out[3].ctypes.data, out[4].ctypes.data))
        return out
