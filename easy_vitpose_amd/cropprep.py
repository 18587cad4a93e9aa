"""Crop preparation of `VitInference.inference` (easy_ViTPose/inference.py:259-266, :314-316):

    bbox (+10 px, clipped) -> crop -> zero-pad to 3:4 (pad_image) -> cv2.resize(.., (192,256), INTER_LINEAR)

`resize_linear_u8` restates OpenCV's 8-bit INTER_LINEAR (opencv-python 4.8, `resize.cpp`): half-pixel
centres, 11-bit fixed-point coefficients (`INTER_RESIZE_COEF_BITS`), horizontal pass into int32, vertical
pass `(((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2`, and the exact-2x case handled as the 2x2 box
average OpenCV switches to.  It is integer arithmetic, so the HIP kernel (`crop_resize_kernel`) reproduces
it bit for bit; against the real OpenCV binary it is PARITY UNPINNED (cv2 is not installed here).
"""
from __future__ import annotations

import numpy as np

from .configs import IMG_H, IMG_W

COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS


def _axis_coeffs(dsize: int, ssize: int):
    inv = float(dsize) / float(ssize)
    scale = 1.0 / inv                                     # OpenCV: scale_x = 1./inv_scale_x
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)      # computed in double, stored as float
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    f[lo] = 0; s[lo] = 0
    hi = s >= ssize - 1
    f[hi] = 0; s[hi] = ssize - 1
    a1 = np.rint(f * np.float32(COEF_ONE)).astype(np.int64)            # cvRound = round half to even
    a0 = np.rint((np.float32(1.0) - f) * np.float32(COEF_ONE)).astype(np.int64)
    s1 = np.minimum(s + 1, ssize - 1)                     # tap 1 has weight 0 where it would fall outside
    return s, s1, a0, a1, scale


def resize_linear_u8(src: np.ndarray, dsize_wh) -> np.ndarray:
    """`cv2.resize(src, (w, h), interpolation=cv2.INTER_LINEAR)` for uint8 HxWxC images."""
    dw, dh = int(dsize_wh[0]), int(dsize_wh[1])
    sh, sw = src.shape[:2]
    if (sw, sh) == (dw, dh):
        return src
    sx, sx1, ax0, ax1, scale_x = _axis_coeffs(dw, sw)
    sy, sy1, ay0, ay1, scale_y = _axis_coeffs(dh, sh)
    if scale_x == 2.0 and scale_y == 2.0:                 # INTER_LINEAR == fast INTER_AREA at exactly 2x
        s = src.astype(np.int64)
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    s = src.astype(np.int64)
    rows = s[:, sx] * ax0[None, :, None] + s[:, sx1] * ax1[None, :, None]          # [sh, dw, C], scale 2^11
    r0, r1 = rows[sy], rows[sy1]
    out = (((ay0[:, None, None] * (r0 >> 4)) >> 16) + ((ay1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def crop_params(bboxes: np.ndarray, frame_hw, pad_bbox: int = 10, aspect: float = 3 / 4) -> np.ndarray:
    """Per box int32 [x0, y0, cw, ch, left_pad, top_pad, pw, ph]: the padded+clipped box of
    inference.py:261-262 and the zero-pad geometry of `pad_image` (vit_utils/inference.py:41-70)."""
    H, W = frame_hw
    out = np.zeros((len(bboxes), 8), dtype=np.int32)
    for i, b in enumerate(np.asarray(bboxes)[:, :4].round().astype(int)):
        x0, x1 = np.clip([b[0] - pad_bbox, b[2] + pad_bbox], 0, W)
        y0, y1 = np.clip([b[1] - pad_bbox, b[3] + pad_bbox], 0, H)
        cw, ch = int(x1 - x0), int(y1 - y0)
        assert cw > 0 and ch > 0, 'empty box'
        left = top = 0
        pw, ph = cw, ch
        if cw / ch < aspect:
            pw = int(aspect * ch)
            left = (pw - cw) // 2
        else:
            ph = int(cw / aspect)
            top = (ph - ch) // 2
        out[i] = (x0, y0, cw, ch, left, top, pw, ph)
    return out


def frames_crop_params(boxes_per_frame, frame_shapes, pad_bbox: int = 10) -> np.ndarray:
    """The crops of several frames as one int32 [n, 9] table {frame, x0, y0, cw, ch, left_pad, top_pad, pw, ph} (vp_infer_frames):
    `crop_params` of each frame's boxes with the frame index in front, frame by frame; a frame without boxes adds no row."""
    rows = [np.zeros((0, 9), dtype=np.int32)]
    for f, (boxes, shape) in enumerate(zip(boxes_per_frame, frame_shapes)):
        if len(boxes) == 0:
            continue
        p = crop_params(boxes, tuple(shape)[:2], pad_bbox)
        rows.append(np.concatenate([np.full((len(p), 1), f, dtype=np.int32), p], axis=1))
    return np.concatenate(rows)


def prepare_crops_host(frame: np.ndarray, params: np.ndarray) -> np.ndarray:
    """Host restatement of the crop path -> uint8 [n, 256, 192, 3] (what the HIP kernel must reproduce)."""
    out = np.empty((len(params), IMG_H, IMG_W, 3), dtype=np.uint8)
    for i, (x0, y0, cw, ch, left, top, pw, ph) in enumerate(params):
        canvas = np.zeros((ph, pw, 3), dtype=np.uint8)
        canvas[top:top + ch, left:left + cw] = frame[y0:y0 + ch, x0:x0 + cw]
        out[i] = resize_linear_u8(canvas, (IMG_W, IMG_H))
    return out


# ---- pixel formats of the frames and boxes entries (include/vitpose_hip.h vp_image; the one device definition is csrc/pixfmt.h) ----------------
PIX_FORMATS = {'rgb': 0, 'bgr': 1, 'nv12': 2}                      # VP_PIX_*
YUV_MATRIX_IDS = {'bt601': 0, 'bt709': 1, 'bt601_full': 2}         # VP_YUV_*
# (yoff, cy, crv, cgu, cgv, cbu) at shift 20.  bt601: the integers of 1.164 / 1.596 / 0.391 / 0.813 / 2.018, the constants of OpenCV's
# cvtColor(COLOR_YUV2RGB_NV12) -- against that binary PARITY UNPINNED (cv2 is not installed here); the others round(x * 2^20) of the standard matrices
YUV_COEFS = {
    'bt601': (16, 1220542, 1673527, -409993, -852492, 2116026),
    'bt709': (16, 1220945, 1879825, -223607, -558796, 2215014),
    'bt601_full': (0, 1048576, 1470104, -360853, -748826, 1858077),
}
YUV_SHIFT = 20


def _matrix_name(matrix) -> str:
    if isinstance(matrix, str):
        if matrix not in YUV_COEFS:
            raise ValueError(f'unknown YUV matrix {matrix!r}: one of {sorted(YUV_COEFS)}')
        return matrix
    for name, i in YUV_MATRIX_IDS.items():
        if i == matrix:
            return name
    raise ValueError(f'unknown YUV matrix {matrix!r}')


def _is_tensor(a) -> bool:
    return hasattr(a, 'data_ptr')


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if _is_tensor(a) else np.asarray(a)


def nv12_to_rgb(y, uv, matrix='bt601') -> np.ndarray:
    """NV12 planes (y uint8 [h, w], uv uint8 [ceil(h/2), ceil(w/2), 2] = U, V pairs) -> uint8 [h, w, 3] RGB: the host restatement of the crop
    kernel's pixel fetch.  int32, arithmetic shifts; chroma replicated (pixel (r, c) reads the pair (r >> 1, c >> 1))."""
    y, uv = _host(y), _host(uv)
    h, w = y.shape
    assert uv.shape == ((h + 1) // 2, (w + 1) // 2, 2), f'uv {uv.shape} for y {y.shape}'
    yoff, cy, crv, cgu, cgv, cbu = (np.int32(v) for v in YUV_COEFS[_matrix_name(matrix)])
    yy = np.maximum(y.astype(np.int32) - yoff, 0) * cy + np.int32(1 << (YUV_SHIFT - 1))
    c = uv[np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1].astype(np.int32) - np.int32(128)
    u, v = c[..., 0], c[..., 1]
    rgb = np.stack([(yy + crv * v) >> YUV_SHIFT, (yy + cgu * u + cgv * v) >> YUV_SHIFT, (yy + cbu * u) >> YUV_SHIFT], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


_RGB2YUV = {   # (yoff, rows of Y, U, V over R, G, B): the forward matrices the tables above invert
    'bt601': (16, ((0.256788, 0.504129, 0.097906), (-0.148223, -0.290993, 0.439216), (0.439216, -0.367788, -0.071427))),
    'bt709': (16, ((0.182586, 0.614231, 0.062007), (-0.100644, -0.338572, 0.439216), (0.439216, -0.398942, -0.040274))),
    'bt601_full': (0, ((0.299, 0.587, 0.114), (-0.168736, -0.331264, 0.5), (0.5, -0.418688, -0.081312))),
}


def rgb_to_nv12(rgb, matrix='bt601'):
    """uint8 [h, w, 3] RGB -> (y [h, w], uv [ceil(h/2), ceil(w/2), 2]) uint8.  Makes NV12 content for tests and benchmarks from seeded RGB frames:
    deterministic (float64, round half to even, chroma = the mean of each 2 x 2 block with the last row / column repeated on odd sizes), NOT an oracle."""
    rgb = _host(rgb).astype(np.float64)
    h, w = rgb.shape[:2]
    yoff, (my, mu, mv) = _RGB2YUV[_matrix_name(matrix)]
    y = np.clip(np.rint(rgb @ np.array(my) + yoff), 0, 255).astype(np.uint8)
    pad = np.pad(rgb, ((0, h & 1), (0, w & 1), (0, 0)), mode='edge')
    blk = (pad[0::2, 0::2] + pad[0::2, 1::2] + pad[1::2, 0::2] + pad[1::2, 1::2]) / 4.0
    uv = np.stack([blk @ np.array(mu), blk @ np.array(mv)], -1) + 128.0
    return y, np.clip(np.rint(uv), 0, 255).astype(np.uint8)


class Frame:
    """One frame of `VitPoseHip.infer_frames` / `infer_boxes` in the layout its producer holds it (vp_image): `Frame.rgb(a)`, `Frame.bgr(a)` for
    packed uint8 [H, W, 3], `Frame.nv12(y, uv, matrix)` for a decoder surface (y uint8 [H, W]; uv uint8 [ceil(H/2), ceil(W/2), 2], U then V).  The
    planes are numpy arrays (host) or torch CUDA tensors (device); rows may be pitched -- the strides are read from the array, nothing is
    copied, and the Frame keeps its planes alive.  Within a row the bytes must be dense (strides (pitch, 3, 1) / (pitch, 1) / (pitch, 2, 1))."""
    __slots__ = ('format', 'matrix', 'planes', 'h', 'w', 'pitch')

    def __init__(self, fmt: str, planes, matrix='bt601'):
        if fmt not in PIX_FORMATS:
            raise ValueError(f'unknown pixel format {fmt!r}: one of {sorted(PIX_FORMATS)}')
        self.format, self.matrix, self.planes = fmt, _matrix_name(matrix), tuple(planes)
        tens = [_is_tensor(p) for p in self.planes]
        if any(tens) and not all(tens):
            raise TypeError('the planes of a frame are all numpy arrays (host) or all torch CUDA tensors (device)')
        for p in self.planes:
            if _is_tensor(p):
                if not p.is_cuda:
                    raise TypeError('a tensor plane must be a torch CUDA tensor (host planes are numpy arrays)')
                if str(p.dtype) != 'torch.uint8':
                    raise TypeError(f'uint8 expected, got {p.dtype}')
            elif not isinstance(p, np.ndarray):
                raise TypeError(f'a numpy array or a torch CUDA tensor expected, got {type(p).__name__}')
            elif p.dtype != np.uint8:
                raise TypeError(f'uint8 expected, got {p.dtype}')
        a = self.planes[0]
        if fmt == 'nv12':
            if len(self.planes) != 2 or a.ndim != 2:
                raise ValueError(f'NV12: y [H, W] and uv [ceil(H/2), ceil(W/2), 2] expected, got y {tuple(a.shape)}')
            self.h, self.w = int(a.shape[0]), int(a.shape[1])
            uv = self.planes[1]
            if tuple(uv.shape) != ((self.h + 1) // 2, (self.w + 1) // 2, 2):
                raise ValueError(f'NV12: uv [{(self.h + 1) // 2}, {(self.w + 1) // 2}, 2] expected for y [{self.h}, {self.w}], got {tuple(uv.shape)}')
            self.pitch = (self._pitch(a, (1,), self.w), self._pitch(uv, (2, 1), 2 * ((self.w + 1) // 2)))
        else:
            if len(self.planes) != 1 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f'[H, W, 3] expected, got {tuple(a.shape)}')
            self.h, self.w = int(a.shape[0]), int(a.shape[1])
            self.pitch = (self._pitch(a, (3, 1), 3 * self.w), 0)

    @staticmethod
    def _strides(a):
        return tuple(int(s) for s in (a.stride() if _is_tensor(a) else a.strides))   # uint8: elements are bytes

    @classmethod
    def _pitch(cls, a, inner, row_bytes: int) -> int:
        """bytes per row of plane `a` whose strides behind the row axis must be `inner` (a dimension of one element has no stride to speak of)"""
        st = cls._strides(a)
        for dim, want in zip(range(1, a.ndim), inner):
            if a.shape[dim] > 1 and st[dim] != want:
                raise ValueError(f'strides {st} of a {tuple(a.shape)} plane: the bytes of a row must be dense (strides (pitch,) + {inner}); the last dimension has stride 1')
        if a.shape[0] <= 1:
            return row_bytes
        if st[0] < row_bytes:
            raise ValueError(f'row stride {st[0]} of a {tuple(a.shape)} plane is below its {row_bytes} row bytes (overlapping or reversed rows)')
        return st[0]

    @classmethod
    def rgb(cls, a):
        return cls('rgb', (a,))

    @classmethod
    def bgr(cls, a):
        return cls('bgr', (a,))

    @classmethod
    def nv12(cls, y, uv, matrix='bt601'):
        return cls('nv12', (y, uv), matrix)

    @property
    def on_device(self) -> bool:
        return _is_tensor(self.planes[0])

    @property
    def shape(self):
        return (self.h, self.w, 3)

    def pointers(self):
        """(plane 0, plane 1 or None) as integers"""
        ptr = [p.data_ptr() if _is_tensor(p) else p.ctypes.data for p in self.planes]
        return ptr[0], (ptr[1] if len(ptr) > 1 else None)

    def __repr__(self):
        return f'Frame.{self.format}({self.h} x {self.w}, pitch {self.pitch}, {"device" if self.on_device else "host"})'


def to_rgb(frame) -> np.ndarray:
    """Any frame the frames / boxes entries accept -> contiguous host uint8 [H, W, 3] RGB: what those entries see.  A bare array or tensor is RGB."""
    if not isinstance(frame, Frame):
        return np.ascontiguousarray(_host(frame))
    if frame.format == 'nv12':
        return nv12_to_rgb(frame.planes[0], frame.planes[1], frame.matrix)
    a = _host(frame.planes[0])
    return np.ascontiguousarray(a[..., ::-1] if frame.format == 'bgr' else a)


# ---- the training-protocol affine crop (csrc/affinegeom.h is the one device definition; include/vitpose_hip.h vp_infer_images_affine) ----------------
BOX_MAX_SIDE = 1 << 24
AFFINE_LIMIT = float(1 << 40)


def box_to_cs(boxes, box_scale: float = 1.25) -> np.ndarray:
    """float32 boxes [n, >= 4] (x1, y1, x2, y2) -> float32 [n, 4] (cx, cy, S_w, S_h): the centre and `scale * 200` of the reference's `_xywh2cs`
    (datasets/COCO.py:322-337) at its widths under numpy 2 -- float64 up to the centre and the 3:4 extension, float32 from `w / 200` on.  The box is
    extended to 3:4 with image content and scaled by `box_scale` (the reference's 1.25), not clipped to the frame; a side above 2^24 is clamped to 2^24.
    Raises ValueError for a box that is not finite, has w <= 0 or h <= 0, or whose side underflows to 0 (the device entry gives those a status instead)."""
    s = np.float32(box_scale)
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f'box_scale must be finite and > 0, got {box_scale!r}')
    b = np.ascontiguousarray(np.asarray(_host(boxes))[:, :4], dtype=np.float32).astype(np.float64)
    if not np.isfinite(b).all():
        raise ValueError('box_to_cs: a box coordinate is not finite')
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    if not ((w > 0).all() and (h > 0).all()):
        raise ValueError('box_to_cs: an empty box (w <= 0 or h <= 0)')
    cx, cy = (b[:, 0] + w * 0.5).astype(np.float32), (b[:, 1] + h * 0.5).astype(np.float32)
    t = 0.75 * h
    h2 = np.where(w > t, w / 0.75, h)
    w2 = np.where(w < t, h * 0.75, w)
    out = np.empty((len(b), 4), dtype=np.float32)
    out[:, 0], out[:, 1] = cx, cy
    with np.errstate(over='ignore'):
        for j, side in ((2, w2), (3, h2)):
            v = (side / 200.0).astype(np.float32)
            v = (v * s).astype(np.float32)
            v = (v * np.float32(200.0)).astype(np.float32)
            out[:, j] = np.minimum(v, np.float32(BOX_MAX_SIDE))
    if not (out[:, 2:] > 0).all():
        raise ValueError('box_to_cs: an empty box (a side underflows to 0)')
    return out


def _affine_axis(n_out: int, a: float, b: float):
    """source position and 1/32 fraction of every output index of one axis: Xq = floor((o a + b) 32 + 0.5), product and sum unfused in float64"""
    src = np.arange(n_out, dtype=np.float64) * np.float64(a) + np.float64(b)
    xq = np.floor(np.clip(src * 32.0 + 0.5, -AFFINE_LIMIT, AFFINE_LIMIT)).astype(np.int64)
    return xq >> 5, xq & 31


def affine_map(cs) -> tuple:
    """(A_x, B_x, A_y, B_y) of one (cx, cy, S_w, S_h): src_x(ox) = ox A_x + B_x, src_y(oy) = oy A_y + B_y, float64 -- the inverse of
    get_warp_matrix(0, c 2, [191, 255], S)"""
    cx, cy, sw, sh = (np.float64(np.float32(v)) for v in cs)
    return sw / 191.0, cx - sw * 0.5, sh / 255.0, cy - sh * 0.5


def check_cs(cs) -> np.ndarray:
    cs = np.ascontiguousarray(cs, dtype=np.float32).reshape(-1, 4)
    if not (np.isfinite(cs).all() and (cs[:, 2:] > 0).all() and (cs[:, 2:] <= BOX_MAX_SIDE).all()):
        raise ValueError('cs: finite (cx, cy, S_w, S_h) rows with 0 < S <= 2^24 expected')
    return cs


def affine_crops_host(frame, cs) -> np.ndarray:
    """The affine crop on the host -> uint8 RGB [n, 256, 192, 3] (what `crop_affine_kernel` must reproduce bit for bit).  `frame`: anything `to_rgb` takes;
    `cs` float32 [n, 4] (`box_to_cs`).  The project's own fixed-point contract: 1/32-pixel source positions, weights (32 - ax)(32 - ay) 32, ..., summing to 32768,
    out = (sum w p + 16384) >> 15 per channel on source pixels converted to RGB8, a tap outside the frame 0; integer from Xq on.  Modelled on OpenCV's 8-bit
    warpAffine(INTER_LINEAR, BORDER_CONSTANT 0); against that binary it is PARITY UNPINNED (cv2 is not installed here)."""
    rgb = to_rgb(frame)
    H, W = rgb.shape[:2]
    cs = check_cs(cs)
    padded = np.zeros((H + 2, W + 2, 3), dtype=np.int64)   # index 0 and H + 1 / W + 1: every position outside the frame
    padded[1:-1, 1:-1] = rgb
    out = np.empty((len(cs), IMG_H, IMG_W, 3), dtype=np.uint8)
    for i, row in enumerate(cs):
        a_x, b_x, a_y, b_y = affine_map(row)
        sx, ax = _affine_axis(IMG_W, a_x, b_x)
        sy, ay = _affine_axis(IMG_H, a_y, b_y)
        x0, x1 = np.clip(sx + 1, 0, W + 1), np.clip(sx + 2, 0, W + 1)
        y0, y1 = np.clip(sy + 1, 0, H + 1), np.clip(sy + 2, 0, H + 1)
        ax, ay = ax[None, :, None], ay[:, None, None]
        acc = ((32 - ax) * (32 - ay) * 32 * padded[y0[:, None], x0[None, :]] + ax * (32 - ay) * 32 * padded[y0[:, None], x1[None, :]]
               + (32 - ax) * ay * 32 * padded[y1[:, None], x0[None, :]] + ax * ay * 32 * padded[y1[:, None], x1[None, :]])
        out[i] = ((acc + 16384) >> 15).astype(np.uint8)
    return out


def affine_back_map(kp_hm, cs) -> np.ndarray:
    """Heatmap-pixel keypoints [n, K, 3] (y, x, conf) with x in [0, 47], y in [0, 63] -> frame pixels as the affine decode writes them: float64,
    x = rx (S_w / 47) + cx - S_w 0.5 step by step, rounded to float32 once (transform_preds(center, scale, use_udp=True))."""
    kp = np.asarray(kp_hm)
    cs = check_cs(cs).astype(np.float64)
    out = np.empty(kp.shape, dtype=np.float32)
    ry, rx = kp[..., 0].astype(np.float64), kp[..., 1].astype(np.float64)
    out[..., 1] = (rx * (cs[:, 2] / 47.0)[:, None] + cs[:, 0][:, None] - (cs[:, 2] * 0.5)[:, None]).astype(np.float32)
    out[..., 0] = (ry * (cs[:, 3] / 63.0)[:, None] + cs[:, 1][:, None] - (cs[:, 3] * 0.5)[:, None]).astype(np.float32)
    out[..., 2] = kp[..., 2]
    return out
