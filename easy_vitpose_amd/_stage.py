"""What the device stages share on the Python side (DESIGN.md "Stage objects"): ``HandleStage``, a stage that runs on the engine's handle (letterbox, orient),
``DeviceStage``, a stage with an object of its own beside the handle (tracker, smoother, metrics, COCO evaluator, detector, YOLO network), and the argument checks
every stream-ordered entry makes before its C call: ``check_tensor`` / ``ptr`` for torch tensors, ``device_frames`` / ``host_frames`` / ``image_table`` for frames.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as capi
from .cropprep import PIX_FORMATS, YUV_MATRIX_IDS, Frame

MAX_FRAMES = 64   # of one call of a frame stage
IMAGE_DTYPE = np.dtype([('plane', np.uint64, 2), ('pitch', np.int64, 2), ('h', np.int32), ('w', np.int32), ('format', np.int32), ('matrix', np.int32)])   # vp_image


def stream_of(dev, stream=None):
    """the handle of `stream` (a torch stream), or of torch's current stream of `dev`"""
    import torch
    return (torch.cuda.current_stream(dev) if stream is None else stream).cuda_stream


def ptr(a, n=None):
    """the address of a torch tensor or numpy array for a C call; None for an absent array, an empty numpy array and a call of n == 0 rows"""
    if a is None or n == 0:
        return None
    if hasattr(a, 'data_ptr'):
        return a.data_ptr()
    return a.ctypes.data if a.size else None


def check_tensor(name, a, dtype, shape, dev, needed=False, contiguous=True):
    """`a` is a torch CUDA tensor of `dtype` (else TypeError) of `shape` on `dev` (else ValueError); None passes unless `needed`.  `shape`: a tuple whose str entries
    stand for any extent (('n', 'K', 3)), or None for any shape.  `contiguous=False`: any positive element stride (a column view such as `rows[:, 4]`)."""
    import torch
    if a is None and not needed:
        return
    dt = str(dtype).replace('torch.', '')
    if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == dtype):
        raise TypeError(f'{name}: {"an" if dt[0] in "aeio" else "a"} {dt} torch CUDA tensor expected')
    fits = shape is None or (a.ndim == len(shape) and all(isinstance(w, str) or w == g for w, g in zip(shape, a.shape)))
    laid = a.is_contiguous() if contiguous else a.numel() < 2 or all(s >= 1 for s in a.stride())
    if a.device != dev or not fits or not laid:
        want = 'tensor' if shape is None else '[' + ', '.join(str(w) for w in shape) + ']'
        want = ('a ' if shape is None else '') + ('contiguous ' + want if contiguous else want + ' with a positive stride')
        raise ValueError(f'{name}: {want} on {dev} expected, got {tuple(a.shape)} on {a.device}')


def frame_on(f: Frame, i: int, dev, what: str = 'frame'):
    """the planes of device frame i lie on the handle's device"""
    for p in f.planes:
        if p.device != dev:
            raise ValueError(f'{what} {i} lives on {p.device}, the handle on {dev}')


def check_count(n: int, stage: str):
    if n > MAX_FRAMES:
        raise ValueError(f'{stage}: {n} frames, a call takes {MAX_FRAMES}')


def device_frames(frames, dev, stage: str, what: str = 'frame'):
    """the frames of a device call as `Frame`s (a bare uint8 CUDA tensor [H, W, 3] is RGB): at most MAX_FRAMES, device planes, on `dev`"""
    frames = [f if isinstance(f, Frame) else Frame.rgb(f) for f in frames]
    check_count(len(frames), stage)
    for i, f in enumerate(frames):
        if not f.on_device:
            raise TypeError(f'{what} {i}: torch uint8 CUDA tensors expected')
        frame_on(f, i, dev, what)
    return frames


def host_frames(frames, stage: str):
    """the frames of a host call as `Frame`s (a bare array [H, W, 3] is RGB): at most MAX_FRAMES, host planes"""
    frames = [f if isinstance(f, Frame) else Frame.rgb(np.asarray(f)) for f in frames]
    check_count(len(frames), stage)
    for i, f in enumerate(frames):
        if f.on_device:
            raise TypeError(f'frame {i}: host planes (numpy arrays) expected')
    return frames


def image_table(frames) -> np.ndarray:
    """the vp_image table of `Frame`s as a numpy record array (the frames keep the planes alive)"""
    tab = np.zeros(len(frames), IMAGE_DTYPE)
    for i, f in enumerate(frames):
        if not isinstance(f, Frame):
            raise TypeError(f'frame {i}: a Frame (Frame.nv12 / Frame.bgr / Frame.rgb) expected, got {type(f).__name__}')
        p0, p1 = f.pointers()
        tab[i] = ((p0, p1 or 0), f.pitch, f.h, f.w, PIX_FORMATS[f.format], YUV_MATRIX_IDS[f.matrix])
    return tab


def _images_ptr(images: np.ndarray):
    return C.cast(images.ctypes.data, C.POINTER(capi.vp_image)) if len(images) else None


class HandleStage:
    """A stage on the engine's handle: the engine, its library, its device and stream."""

    def __init__(self, engine):
        self.engine, self.lib = engine, engine.lib

    @property
    def _dev(self):
        import torch
        return torch.device('cuda', self.engine.device_id)

    def _stream(self, stream=None):
        return stream_of(self._dev, stream)

    def _check(self, code):
        capi.check(code, self.engine._h)

    def upload(self, img):
        """a host uint8 [H, W, 3] RGB array as a device `Frame`"""
        import torch
        return Frame.rgb(torch.from_numpy(np.ascontiguousarray(img)).to(self._dev))


class DeviceStage(HandleStage):
    """A stage with an object of its own beside the handle.  A subclass names its destroy entry in `_destroy` and creates the object with `_create`; the object
    lives until `close` (idempotent) or the collection of the stage.  An engine closed first has freed nothing of the stage: the object is then left alone."""
    _destroy = None   # 'vp_tracker_destroy'
    _obj = None

    def _create(self, fn, *args):
        h = C.c_void_p()
        self._check(fn(self.engine._h, *args, C.byref(h)))
        self._obj = h

    def close(self):
        if self._obj and self.engine._h:
            getattr(self.lib, self._destroy)(self._obj)
        self._obj = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


handle_alias = property(lambda self: self._obj)   # the per-class names of the object (`_t`, `_s`, ...), which tests and tools pass to the library themselves
