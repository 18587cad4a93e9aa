"""The orient stage on the device (vp_orient_stream; semantics in csrc/orientgeom.h): frames as a decoder or a capture device leaves them -- a landscape surface
plus a rotation tag, a mirrored webcam, a ceiling camera -- made upright in device memory, in front of the letterbox stage and every other stage that reads a
frame.  The eight EXIF orientations of NV12 / RGB / BGR frames, pitched views on either side, a pure permutation of bytes: equal means equal bytes.  The codes,
the ctypes layer, the numpy twin ``orient_host_numpy`` written from the table by slicing, ``HostOrient`` (the host tap vp_dbg_orient_host: the model the device is
tested against, never a fallback) and ``DeviceOrient``.

    code  output                        size          code  output                                size
    1     a (a copy)                    h x w         5     a.T                                   w x h
    2     a[:, ::-1]                    h x w         6     np.rot90(a, -1)  (90 deg clockwise)   w x h
    3     a[::-1, ::-1]                 h x w         7     np.rot90(a, 2).T (transverse)         w x h
    4     a[::-1, :]                    h x w         8     np.rot90(a, 1)   (90 deg counter-cw)  w x h

``rotate_code(angle)`` maps the reference's ``--rotate`` angles (counter-clockwise degrees, its ``rotation_map``) to codes: 0 / 90 / 180 / 270 -> 1 / 8 / 3 / 6.
NV12: the UV plane takes the same code on (ceil(h / 2), ceil(w / 2)) pairs; a frame with an odd extent along an axis the code reverses is refused, since its chroma
siting would move (codes 1 and 5 take any size).  ``DeviceOrient.orient`` is stream-ordered and never synchronises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as capi
from ._stage import IMAGE_DTYPE, MAX_FRAMES as MAX_IMAGES, HandleStage, check_count, _images_ptr, device_frames, frame_on, host_frames, image_table
from .cropprep import PIX_FORMATS, Frame

ORIENT_CODES = {'identity': 1, 'mirror': 2, 'rot180': 3, 'flip': 4, 'transpose': 5, 'cw90': 6, 'transverse': 7, 'ccw90': 8}   # VP_ORIENT_*: the EXIF values
_ROTATE = {0: 1, 90: 8, 180: 3, 270: 6}
INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}   # orient(orient(f, c), INVERSE[c]) == f


def rotate_code(angle) -> int:
    """the orientation code of the reference's `--rotate` angle (counter-clockwise degrees): 0 / 90 / 180 / 270 -> 1 / 8 / 3 / 6"""
    if isinstance(angle, (bool, np.bool_)) or not isinstance(angle, (int, np.integer)) or int(angle) not in _ROTATE:
        raise ValueError(f'rotate: one of 0, 90, 180, 270 expected, got {angle!r}')
    return _ROTATE[int(angle)]


def check_code(code, i: int = 0) -> int:
    if isinstance(code, str) and code in ORIENT_CODES:
        return ORIENT_CODES[code]
    if isinstance(code, (bool, np.bool_)) or not isinstance(code, (int, np.integer)) or not 1 <= int(code) <= 8:
        raise ValueError(f'frame {i}: an orientation code in 1..8 (or one of {sorted(ORIENT_CODES)}) expected, got {code!r}')
    return int(code)


def oriented_hw(frame_hw, code):
    """(h, w) of a frame of `frame_hw` under `code`: swapped by codes 5..8"""
    h, w = (int(v) for v in frame_hw)
    return (w, h) if check_code(code) >= 5 else (h, w)


def _orient_plane(a: np.ndarray, code: int) -> np.ndarray:
    """one plane [h, w] or [h, w, c] by slicing, from the table; trailing axes (the bytes of an element) stay as they are"""
    t = (1, 0) + tuple(range(2, a.ndim))
    if code == 1:
        out = a
    elif code == 2:
        out = a[:, ::-1]
    elif code == 3:
        out = a[::-1, ::-1]
    elif code == 4:
        out = a[::-1, :]
    elif code == 5:
        out = a.transpose(t)
    elif code == 6:
        out = a[::-1, :].transpose(t)      # out[i, j] = a[h - 1 - j, i]
    elif code == 7:
        out = a[::-1, ::-1].transpose(t)   # out[i, j] = a[h - 1 - j, w - 1 - i]
    else:
        out = a[:, ::-1].transpose(t)      # out[i, j] = a[j, w - 1 - i]
    return np.ascontiguousarray(out)


def nv12_admitted(code: int, h: int, w: int) -> bool:
    """an NV12 frame of h x w takes `code`: every axis the code reverses has even length"""
    rev_row, rev_col = code in (3, 4, 6, 7), code in (2, 3, 7, 8)
    return not ((rev_row and h % 2) or (rev_col and w % 2))


def orient_host_numpy(frame, code) -> Frame:
    """The numpy twin of one host frame, written from the table by slicing, independent of csrc/orientgeom.h: a tight host `Frame` of the same format and matrix.
    A bare array [H, W, 3] is RGB."""
    code = check_code(code)
    if not isinstance(frame, Frame):
        frame = Frame.rgb(np.asarray(frame))
    if frame.on_device:
        raise TypeError('host planes (numpy arrays) expected')
    if frame.format == 'nv12' and not nv12_admitted(code, frame.h, frame.w):
        raise ValueError(f'an NV12 frame of {frame.h} x {frame.w}: code {code} reverses an axis of odd length')
    return Frame(frame.format, tuple(_orient_plane(p, code) for p in frame.planes), frame.matrix)


def _codes(codes, n: int) -> np.ndarray:
    if isinstance(codes, (int, np.integer, str)) and not isinstance(codes, (bool, np.bool_)):
        codes = [codes] * n
    codes = list(codes)
    if len(codes) != n:
        raise ValueError(f'orient: {len(codes)} codes for {n} frames')
    return np.array([check_code(c, i) for i, c in enumerate(codes)], dtype=np.int32).reshape(n)


def _plane_shapes(fmt: str, h: int, w: int):
    return ((h, w), ((h + 1) // 2, (w + 1) // 2, 2)) if fmt == 'nv12' else ((h, w, 3),)


def _out_frames(frames, codes, out, on_device: bool, alloc):
    """the destination frames of a call: `out` after the checks that need no library, or tight planes from `alloc(shape)`"""
    if out is None:
        return [Frame(f.format, tuple(alloc(s) for s in _plane_shapes(f.format, *oriented_hw((f.h, f.w), c))), f.matrix) for f, c in zip(frames, codes)]
    out = list(out)
    if len(out) != len(frames):
        raise ValueError(f'out: {len(out)} frames for {len(frames)} frames')
    for i, (f, c, o) in enumerate(zip(frames, codes, out)):
        if not isinstance(o, Frame):
            raise TypeError(f'out {i}: a Frame expected, got {type(o).__name__}')
        if o.on_device != on_device:
            raise TypeError(f'out {i}: ' + ('torch uint8 CUDA tensors expected' if on_device else 'host planes (numpy arrays) expected'))
        want = oriented_hw((f.h, f.w), c)
        if (o.h, o.w) != want or o.format != f.format or o.matrix != f.matrix:
            raise ValueError(f'out {i}: a {f.format} frame of {want[0]} x {want[1]} ({f.matrix}) expected, got {o.format} {o.h} x {o.w} ({o.matrix})')
        if not on_device and not all(p.flags.writeable for p in o.planes):
            raise ValueError(f'out {i}: writeable planes expected')
    return out


def orient_plan(frames_hw, codes, fmt: str = 'rgb', pitch=None):
    """vp_orient_plan (host only) for frames of `frames_hw` = (h, w) or [n, 2] of one format: (sizes int32 [n, 2] = (h, w), pitches int64 [n, 2], plane bytes
    int64 [n, 2]) of the destination frames.  `pitch` [n, 2] (or None): the destination pitches to keep where non-zero."""
    hw = np.asarray(frames_hw, dtype=np.int64).reshape(-1, 2)
    n = len(hw)
    check_count(n, 'orient')
    codes = _codes(codes, n)
    src, dst = np.zeros(n, IMAGE_DTYPE), np.zeros(n, IMAGE_DTYPE)
    src['h'], src['w'], src['format'] = hw[:, 0], hw[:, 1], PIX_FORMATS[fmt]
    w = np.maximum(hw[:, 1], 0)
    src['pitch'][:, 0] = w if fmt == 'nv12' else 3 * w
    src['pitch'][:, 1] = 2 * ((w + 1) // 2) if fmt == 'nv12' else 0
    if pitch is not None:
        dst['pitch'] = np.asarray(pitch, dtype=np.int64).reshape(n, 2)
    nbytes = np.zeros((n, 2), np.int64)
    capi.check(capi.load_library().vp_orient_plan(_images_ptr(src), codes.ctypes.data if n else None, n, _images_ptr(dst), nbytes.ctypes.data if n else None))
    return np.stack([dst['h'], dst['w']], 1).astype(np.int32), dst['pitch'].copy(), nbytes


class HostOrient:
    """csrc/orientgeom.h run serially through the tap vp_dbg_orient_host: the model the device is tested against, never a fallback."""

    def __init__(self):
        self.lib = capi.load_library()

    def orient(self, frames, codes, out=None):
        """host `Frame`s and one code each (or one for all) -> the oriented host `Frame`s (`out`, possibly pitched views, or tight new ones)"""
        frames = host_frames(frames, 'orient')
        n = len(frames)
        codes = _codes(codes, n)
        out = _out_frames(frames, codes, out, False, lambda s: np.empty(s, np.uint8))
        src, dst = image_table(frames), image_table(out)
        capi.check(self.lib.vp_dbg_orient_host(_images_ptr(src), codes.ctypes.data if n else None, _images_ptr(dst), n))
        return out


class DeviceOrient(HandleStage):
    def orient(self, frames, codes, out=None, stream=None):
        """`frames`: `Frame.nv12 / Frame.bgr / Frame.rgb` over torch CUDA planes of the handle's device (a bare uint8 CUDA tensor [H, W, 3] is RGB), read in place;
        `codes`: one orientation code per frame, or one for all.  Enqueues on `stream` (a torch stream; None: torch's current stream) and never synchronises.
        `out`: the destination `Frame`s (possibly pitched views into larger buffers: no byte outside their rows is touched); None allocates tight planes.  Returns
        the upright `Frame`s, which `letterbox`, `infer_boxes`, `infer_frames`, `draw_poses` and `draw_labels` take as they are."""
        import torch
        dev = self._dev
        frames = device_frames(frames, dev, 'orient')
        n = len(frames)
        codes = _codes(codes, n)
        out = _out_frames(frames, codes, out, True, lambda s: torch.empty(s, dtype=torch.uint8, device=dev))
        for i, f in enumerate(out):
            frame_on(f, i, dev, 'out')
        src, dst = image_table(frames), image_table(out)
        self._check(self.lib.vp_orient_stream(self.engine._h, _images_ptr(src), codes.ctypes.data if n else None, _images_ptr(dst), n, self._stream(stream)))
        return out

    def orient_host(self, frames, codes, out=None):
        """`orient` on host `Frame`s (vp_orient: upload, the same kernel, download of the destination rows, synchronous) -> host `Frame`s"""
        frames = host_frames(frames, 'orient')
        n = len(frames)
        codes = _codes(codes, n)
        out = _out_frames(frames, codes, out, False, lambda s: np.empty(s, np.uint8))
        src, dst = image_table(frames), image_table(out)
        self._check(self.lib.vp_orient(self.engine._h, _images_ptr(src), codes.ctypes.data if n else None, _images_ptr(dst), n))
        return out
