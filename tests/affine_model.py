"""An independent model of the affine crop route, scalar loops written from its contract (csrc/affinegeom.h) -- NOT the product's
cropprep.py: the golden generator makes the crops the reference model sees with it, and the CPU tests hold the product's host twin against it.

  box -> (cx, cy, S_w, S_h): float64 up to the centre and the 3:4 extension, float32 from w / 200 on
  src_x(ox) = ox (S_w / 191) + (cx - S_w / 2), src_y likewise with 255: float64, product and sum separate
  Xq = floor(src 32 + 0.5); s = Xq >> 5, a = Xq & 31; out = (sum w p + 16384) >> 15 with the four 15-bit weights; a tap outside the frame is 0
  taps are source pixels converted to RGB8 first (NV12: the integer matrices of csrc/pixfmt.h at shift 20, chroma replicated)
  back: x = (float32)(rx (S_w / 47) + cx - S_w 0.5), y with 63 and S_h, float64 step by step
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
YUV = {'bt601': (16, 1220542, 1673527, -409993, -852492, 2116026),
       'bt709': (16, 1220945, 1879825, -223607, -558796, 2215014),
       'bt601_full': (0, 1048576, 1470104, -360853, -748826, 1858077)}


def box_cs(box, box_scale=1.25):
    """one box (x1, y1, x2, y2) -> (cx, cy, S_w, S_h) as four np.float32"""
    x1, y1, x2, y2 = (float(F32(v)) for v in box)
    w, h = x2 - x1, y2 - y1
    cx, cy = F32(x1 + w * 0.5), F32(y1 + h * 0.5)
    if w > 0.75 * h:
        h = w / 0.75
    elif w < 0.75 * h:
        w = h * 0.75
    out = [cx, cy]
    for side in (w, h):
        s = F32(side / 200.0)
        s = F32(float(s) * float(F32(box_scale)))
        out.append(F32(min(float(F32(float(s) * 200.0)), 16777216.0)))
    return tuple(out)


def inverse_map(cs):
    cx, cy, sw, sh = (float(v) for v in cs)
    return sw / 191.0, cx - sw / 2.0, sh / 255.0, cy - sh / 2.0


def axis(o: int, a: float, b: float):
    prod = o * a
    src = prod + b
    q = min(max(src * 32.0 + 0.5, -float(1 << 40)), float(1 << 40))
    xq = math.floor(q)
    return xq >> 5, xq & 31


def _clip255(v):
    return 0 if v < 0 else (255 if v > 255 else v)


def frame_to_rgb_rows(kind: str, planes, matrix='bt601'):
    """the frame as nested lists [h][w] of (r, g, b) ints, every source pixel converted once.  kind 'rgb' / 'bgr': planes = (array [h, w, 3],), any strides;
    'nv12': planes = (y [h, w], uv [ceil(h/2), ceil(w/2), 2])"""
    a = planes[0]
    h, w = a.shape[:2]
    rows = []
    if kind == 'nv12':
        yoff, cy, crv, cgu, cgv, cbu = YUV[matrix]
        uv = planes[1]
        for r in range(h):
            row = []
            for c in range(w):
                y = max(int(a[r, c]) - yoff, 0) * cy + (1 << 19)
                u, v = int(uv[r >> 1, c >> 1, 0]) - 128, int(uv[r >> 1, c >> 1, 1]) - 128
                row.append((_clip255((y + crv * v) >> 20), _clip255((y + cgu * u + cgv * v) >> 20), _clip255((y + cbu * u) >> 20)))
            rows.append(row)
        return rows
    lst = a.tolist()
    for r in range(h):
        rows.append([tuple(p[::-1]) if kind == 'bgr' else tuple(p) for p in lst[r]])
    return rows


def crop(rows, cs) -> np.ndarray:
    """one crop uint8 [256, 192, 3] of a frame given as frame_to_rgb_rows"""
    h, w = len(rows), len(rows[0])
    a_x, b_x, a_y, b_y = inverse_map(cs)
    xs = [axis(ox, a_x, b_x) for ox in range(192)]
    out = np.zeros((256, 192, 3), dtype=np.uint8)
    zero = (0, 0, 0)
    for oy in range(256):
        sy, ay = axis(oy, a_y, b_y)
        r0 = rows[sy] if 0 <= sy < h else None
        r1 = rows[sy + 1] if 0 <= sy + 1 < h else None
        if r0 is None and r1 is None:
            continue
        line = out[oy]
        for ox, (sx, ax) in enumerate(xs):
            in0, in1 = 0 <= sx < w, 0 <= sx + 1 < w
            p00 = r0[sx] if (r0 is not None and in0) else zero
            p01 = r0[sx + 1] if (r0 is not None and in1) else zero
            p10 = r1[sx] if (r1 is not None and in0) else zero
            p11 = r1[sx + 1] if (r1 is not None and in1) else zero
            w00, w01, w10, w11 = (32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32, (32 - ax) * ay * 32, ax * ay * 32
            line[ox] = [(w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 16384) >> 15 for c in range(3)]
    return out


def back_map(rx: float, ry: float, cs):
    """heatmap pixel (rx, ry) -> frame pixel (x, y) as np.float32, float64 step by step"""
    cx, cy, sw, sh = (float(v) for v in cs)
    x = rx * (sw / 47.0)
    x = x + cx
    x = x - sw * 0.5
    y = ry * (sh / 63.0)
    y = y + cy
    y = y - sh * 0.5
    return F32(x), F32(y)


def decode(heatmaps: np.ndarray, cs) -> np.ndarray:
    """The fp64 model of the affine decode: the oracle's arg-max and DARK refinement (heatmap pixels, one crop at a time as the reference is called), then
    back_map.  heatmaps [n, K, 64, 48], cs [n, 4] -> [n, K, 3] (y, x, conf) float32 in frame pixels"""
    from oracle import vitpose_cpu as O
    n, K = heatmaps.shape[:2]
    out = np.empty((n, K, 3), dtype=np.float32)
    for i in range(n):
        hm = heatmaps[i:i + 1].astype(np.float32).copy()
        preds, maxvals = O.get_max_preds(hm)
        preds = O.post_dark_udp(preds, hm, kernel=11)
        for k in range(K):
            x, y = back_map(float(preds[0, k, 0]), float(preds[0, k, 1]), cs[i])
            out[i, k] = (y, x, maxvals[0, k, 0])
    return out
