"""The letterbox stage on the device (vp_letterbox_stream; semantics in csrc/lbgeom.h): frames as their producer holds them -- NV12 decoder surfaces, BGR / RGB
buffers, pitched -- to the detector's input tensor: resize, pad, colour conversion, normalisation and transpose in one kernel, in front of the (third-party)
detector network.  Configuration, the ctypes layer, the numpy twin ``letterbox_host_numpy`` written from the contract, ``HostLetterbox`` (the host tap
vp_dbg_letterbox_host: the model the device is tested against, never a fallback) and ``DeviceLetterbox``.

``DeviceLetterbox.letterbox`` is stream-ordered and never synchronises.  It returns the tensor, the undo table -- float32 [n, 5] rows (gain, pad_x, pad_y,
frame_w, frame_h), what ``DeviceDetector.detect(pred, table)`` takes in place of ``frames_hw, input_hw`` -- and the placement int32 [n, 4] (left, top, new_w,
new_h).  The two are ultralytics' own conventions (scale_boxes and LetterBox) and differ by one pixel of pad for some sizes: the table undoes boxes the way
ultralytics does, the placement says where the pixels lie.  Against the ultralytics and OpenCV binaries PARITY UNPINNED (neither is installed here).
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _capi as capi
from ._stage import IMAGE_DTYPE, MAX_FRAMES as MAX_IMAGES, HandleStage, _images_ptr, device_frames, host_frames, image_table   # noqa: F401  (re-exported)
from .cropprep import resize_linear_u8, to_rgb
from .devdetect import _integer, letterbox_params

MAX_SIDE = 8192
DTYPES = {'fp32': 0, 'fp16': 1, 'u8': 2}                      # VP_LB_*
NP_DTYPES = {'fp32': np.float32, 'fp16': np.float16, 'u8': np.uint8}
LAYOUTS = {'nchw': 0, 'nhwc': 1}
ORDERS = {'rgb': 0, 'bgr': 1}


@dataclasses.dataclass(frozen=True)
class LetterboxCfg:
    """``input_hw``: the detector's input (in_h, in_w), 1..8192 each; ``dtype``: 'fp16' (`im.half() / 255`), 'fp32' (`im.float() / 255`) or 'u8' (the bytes, for
    engines that normalise inside the model); ``layout``: 'nchw' or 'nhwc'; ``order``: 'rgb' (ultralytics' model input) or 'bgr'; ``pad_value``: 0..255
    (ultralytics pads with 114); ``scaleup``: False never enlarges a frame."""
    input_hw: tuple = (640, 640)
    dtype: str = 'fp16'
    layout: str = 'nchw'
    order: str = 'rgb'
    pad_value: int = 114
    scaleup: bool = True

    def __post_init__(self):
        hw = self.input_hw
        if _integer(hw):
            hw = (hw, hw)
        try:
            hw = tuple(hw)
        except TypeError:
            hw = ()
        if not (len(hw) == 2 and all(_integer(v) and 1 <= v <= MAX_SIDE for v in hw)):
            raise ValueError(f'LetterboxCfg: input_hw = (in_h, in_w) in 1..{MAX_SIDE} expected, got {self.input_hw!r}')
        if self.dtype not in DTYPES:
            raise ValueError(f"LetterboxCfg: dtype 'fp16', 'fp32' or 'u8' expected, got {self.dtype!r}")
        if self.layout not in LAYOUTS:
            raise ValueError(f"LetterboxCfg: layout 'nchw' or 'nhwc' expected, got {self.layout!r}")
        if self.order not in ORDERS:
            raise ValueError(f"LetterboxCfg: order 'rgb' or 'bgr' expected, got {self.order!r}")
        if not (_integer(self.pad_value) and 0 <= self.pad_value <= 255):
            raise ValueError(f'LetterboxCfg: pad_value in 0..255 expected, got {self.pad_value!r}')
        if not isinstance(self.scaleup, (bool, np.bool_)):
            raise ValueError(f'LetterboxCfg: scaleup True or False expected, got {self.scaleup!r}')
        object.__setattr__(self, 'input_hw', (int(hw[0]), int(hw[1])))
        object.__setattr__(self, 'pad_value', int(self.pad_value))
        object.__setattr__(self, 'scaleup', bool(self.scaleup))

    def shape(self, n: int):
        """the tensor of n frames"""
        h, w = self.input_hw
        return (n, 3, h, w) if self.layout == 'nchw' else (n, h, w, 3)


def c_config(cfg: LetterboxCfg):
    if not isinstance(cfg, LetterboxCfg):
        raise TypeError(f'a LetterboxCfg expected, got {type(cfg).__name__}')
    return capi.vp_letterbox_cfg(cfg.input_hw[0], cfg.input_hw[1], DTYPES[cfg.dtype], LAYOUTS[cfg.layout], ORDERS[cfg.order], cfg.pad_value, int(cfg.scaleup))


def letterbox_plan(frames_hw, cfg: LetterboxCfg):
    """vp_letterbox_plan (host only) for frames of `frames_hw` = (h, w) or [n, 2]: (undo table float32 [n, 5] = (gain, pad_x, pad_y, frame_w, frame_h) as
    vp_detect_stream takes it, placement int32 [n, 4] = (left, top, new_w, new_h)).  Any number of frames (the C entry is called per 64)."""
    c = c_config(cfg)
    hw = np.asarray(frames_hw, dtype=np.int64).reshape(-1, 2)
    lib = capi.load_library()
    n = len(hw)
    images = np.zeros(n, IMAGE_DTYPE)   # packed RGB frames without data: the plan reads sizes and layout only
    images['h'], images['w'] = hw[:, 0], hw[:, 1]
    images['pitch'][:, 0] = 3 * np.maximum(hw[:, 1], 0)
    det, placement = np.empty((n, 5), np.float32), np.empty((n, 4), np.int32)
    for s in range(0, n, MAX_IMAGES):
        e = min(n, s + MAX_IMAGES)
        capi.check(lib.vp_letterbox_plan(C.byref(c), _images_ptr(images[s:e]), e - s, C.cast(det[s:e].ctypes.data, C.POINTER(capi.vp_det_image)), placement[s:e].ctypes.data))
    return det, placement


def letterbox_geometry(frame_hw, cfg: LetterboxCfg):
    """the contract's geometry in plain Python: ((left, top, new_w, new_h), (gain, pad_x, pad_y)).  `round` is Python's: half to even."""
    h, w = (int(v) for v in frame_hw)
    in_h, in_w = cfg.input_hw
    if h < 1 or w < 1:
        raise ValueError(f'letterbox: a frame of {h} x {w}')
    gain = min(in_h / h, in_w / w)
    clamped = not cfg.scaleup and gain > 1.0
    r = 1.0 if clamped else gain
    new_w, new_h = round(w * r), round(h * r)
    if new_w < 1 or new_h < 1:
        raise ValueError(f'letterbox: a frame of {h} x {w} scales to an empty image in {in_h} x {in_w}')
    left, top = round((in_w - new_w) / 2 - 0.1), round((in_h - new_h) / 2 - 0.1)
    undo = (1.0, float(left), float(top)) if clamped else letterbox_params((h, w), (in_h, in_w))
    return (left, top, new_w, new_h), undo


def letterbox_host_numpy(frame, cfg: LetterboxCfg):
    """The numpy twin of one frame, from the contract: `to_rgb`, `resize_linear_u8`, place, pad, order, normalise, transpose.  Returns (tensor [3, in_h, in_w] or
    [in_h, in_w, 3] of the configured dtype, undo row float32 [5], placement int32 [4])."""
    rgb = to_rgb(frame)
    h, w = rgb.shape[:2]
    (left, top, new_w, new_h), undo = letterbox_geometry((h, w), cfg)
    in_h, in_w = cfg.input_hw
    canvas = np.full((in_h, in_w, 3), cfg.pad_value, np.uint8)
    canvas[top:top + new_h, left:left + new_w] = resize_linear_u8(rgb, (new_w, new_h))
    if cfg.order == 'bgr':
        canvas = canvas[..., ::-1]
    if cfg.dtype == 'u8':
        out = canvas
    else:
        out = canvas.astype(np.float32) / np.float32(255)
        if cfg.dtype == 'fp16':
            out = out.astype(np.float16)
    if cfg.layout == 'nchw':
        out = out.transpose(2, 0, 1)
    return np.ascontiguousarray(out), np.array(undo + (w, h), np.float32), np.array((left, top, new_w, new_h), np.int32)


class HostLetterbox:
    """csrc/lbgeom.h run serially through the tap vp_dbg_letterbox_host: the model the device is tested against, never a fallback."""

    def __init__(self, cfg: LetterboxCfg):
        self.cfg, self._c = cfg, c_config(cfg)
        self.lib = capi.load_library()

    def letterbox(self, frames):
        """host `Frame`s -> (tensor ndarray, undo table float32 [n, 5], placement int32 [n, 4])"""
        frames = host_frames(frames, 'letterbox')
        n = len(frames)
        images = image_table(frames)
        out = np.empty(self.cfg.shape(n), NP_DTYPES[self.cfg.dtype])
        det, placement = np.empty((n, 5), np.float32), np.empty((n, 4), np.int32)
        capi.check(self.lib.vp_dbg_letterbox_host(C.byref(self._c), _images_ptr(images), n, out.ctypes.data if n else None,
                                                  C.cast(det.ctypes.data, C.POINTER(capi.vp_det_image)), placement.ctypes.data))
        return out, det, placement


class DeviceLetterbox(HandleStage):
    def __init__(self, engine, cfg: LetterboxCfg = LetterboxCfg()):
        super().__init__(engine)
        self.cfg, self._c = cfg, c_config(cfg)

    def _torch_dtype(self):
        import torch
        return {'fp32': torch.float32, 'fp16': torch.float16, 'u8': torch.uint8}[self.cfg.dtype]

    def letterbox(self, frames, out=None, stream=None):
        """`frames`: `Frame.nv12 / Frame.bgr / Frame.rgb` over torch CUDA planes of the handle's device (a bare uint8 CUDA tensor [H, W, 3] is RGB), read in place.
        Enqueues on `stream` (a torch stream; None: torch's current stream) and never synchronises.  `out`: a contiguous CUDA tensor of the configured dtype and
        shape to write into (it may be a view whose start is aligned to its element only); None allocates one.  Returns (tensor, undo table float32 [n, 5] -- what
        `DeviceDetector.detect(pred, table)` takes --, placement int32 [n, 4]); the two tables are host arrays, known when the call returns."""
        import torch
        dev = self._dev
        frames = device_frames(frames, dev, 'letterbox')
        n = len(frames)
        shape = self.cfg.shape(n)
        if out is None:
            out = torch.empty(shape, dtype=self._torch_dtype(), device=dev)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == self._torch_dtype()):
            raise TypeError(f'out: a {self.cfg.dtype} torch CUDA tensor expected')
        elif out.device != dev or not out.is_contiguous() or tuple(out.shape) != shape:
            raise ValueError(f'out: a contiguous tensor of shape {shape} on {dev} expected, got {tuple(out.shape)} on {out.device}')
        images = image_table(frames)
        det, placement = np.empty((n, 5), np.float32), np.empty((n, 4), np.int32)
        self._check(self.lib.vp_letterbox_stream(self.engine._h, C.byref(self._c), _images_ptr(images), n, out.data_ptr() if n else None,
                                                 C.cast(det.ctypes.data, C.POINTER(capi.vp_det_image)), placement.ctypes.data, self._stream(stream)))
        return out, det, placement

    def letterbox_host(self, frames):
        """`letterbox` on host `Frame`s (vp_letterbox: upload, the same kernel, download, synchronous) -> (ndarray, table, placement)"""
        frames = host_frames(frames, 'letterbox')
        n = len(frames)
        images = image_table(frames)
        out = np.empty(self.cfg.shape(n), NP_DTYPES[self.cfg.dtype])
        det, placement = np.empty((n, 5), np.float32), np.empty((n, 4), np.int32)
        self._check(self.lib.vp_letterbox(self.engine._h, C.byref(self._c), _images_ptr(images), n, out.ctypes.data if n else None,
                                          C.cast(det.ctypes.data, C.POINTER(capi.vp_det_image)), placement.ctypes.data))
        return out, det, placement
