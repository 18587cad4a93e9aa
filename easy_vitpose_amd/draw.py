"""Skeleton overlay (vp_draw_poses_stream; semantics in csrc/drawgeom.h): the style, the tables, their ctypes form and the numpy twin of the header.

Modelled on the reference's ``draw_points_and_skeleton`` (opaque colours, no anti-aliasing) with the palettes ``VitInference.draw`` asks for ('jet' sampled
at 8 for limbs, 'gist_rainbow' sampled at 10 for joints).  The rasterisation is this project's own integer one: parity against OpenCV's ``circle`` /
``line`` / ``rectangle`` is UNPINNED and not claimed.  The reference ships one skeleton per dataset; built in here is the public COCO-17 one, every other
joint layout needs its skeleton given.
"""
from __future__ import annotations

import dataclasses
import math
import numbers

import numpy as np

from . import _capi as capi
from .cropprep import PIX_FORMATS, YUV_MATRIX_IDS, Frame, _matrix_name

DRAW_MAX_LIMBS = 256
DRAW_MAX_COLORS = 32
DRAW_MAX_K = 256
DRAW_MAX_DIM = 8192
DRAW_MAX_RADIUS = 64
DRAW_MAX_THICKNESS = 16
DRAW_MAX_RECORDS = 65536
LABEL_MAX_ROWS = 8192
LABEL_MAX_SCALE = 8
LABEL_MAX_TEXT = 22

# the COCO keypoint skeleton (0-based joint pairs), in the order the limbs are drawn
COCO17_SKELETON = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10), (1, 2), (0, 1), (0, 2),
                   (1, 3), (2, 4), (0, 5), (0, 6))
# matplotlib's 'jet' at 8 samples and 'gist_rainbow' at 10, round(255 x), RGB
LIMB_COLORS = ((0, 0, 128), (0, 16, 255), (0, 164, 255), (64, 255, 183), (183, 255, 64), (255, 185, 0), (255, 48, 0), (128, 0, 0))
POINT_COLORS = ((255, 0, 41), (255, 110, 0), (249, 255, 0), (92, 255, 0), (0, 255, 59), (0, 255, 215), (0, 143, 255), (14, 0, 255), (167, 0, 255),
                (255, 0, 191))

# RGB -> YUV (yoff, rows of Y, U, V over R, G, B) as round(x * 2^8) of the standard matrices: csrc/drawgeom.h rgb_yuv_coef
RGB_YUV_COEFS = {
    'bt601': (16, (66, 129, 25), (-38, -74, 112), (112, -94, -18)),
    'bt709': (16, (47, 157, 16), (-26, -87, 112), (112, -102, -10)),
    'bt601_full': (0, (77, 150, 29), (-43, -85, 128), (128, -107, -21)),
}


def _number(v) -> bool:   # Python and numpy real scalars; a bool is not a number here
    return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_))


def _whole(v) -> bool:
    return _number(v) and int(v) == v


def _colors(v, name: str) -> tuple:
    try:
        rows = tuple(tuple(c) for c in v)
    except TypeError:
        raise ValueError(f'DrawStyle: {name} is a list of (R, G, B) rows') from None
    if not 1 <= len(rows) <= DRAW_MAX_COLORS or not all(len(c) == 3 and all(_whole(x) and 0 <= x <= 255 for x in c) for c in rows):
        raise ValueError(f'DrawStyle: {name} holds 1..{DRAW_MAX_COLORS} (R, G, B) rows of integers in 0..255')
    return tuple(tuple(int(x) for x in c) for c in rows)


def _pairs(v, what: str) -> tuple:
    try:
        rows = tuple(tuple(p) for p in v)
    except TypeError:
        raise ValueError(f'{what}: a list of [a, b] joint index pairs expected') from None
    if len(rows) > DRAW_MAX_LIMBS or not all(len(p) == 2 and all(_whole(x) and 0 <= x < DRAW_MAX_K for x in p) for p in rows):
        raise ValueError(f'{what}: at most {DRAW_MAX_LIMBS} [a, b] pairs of joint indices in 0..{DRAW_MAX_K - 1} expected')
    return tuple((int(a), int(b)) for a, b in rows)


@dataclasses.dataclass(frozen=True)
class DrawStyle:
    """``conf_thr``: joints at or below this confidence are not drawn (a limb needs both of its joints); ``radius``: of a joint's disk, 0 for
    ``max(1, min(h, w) // 150)`` of the frame; ``thickness``: of limbs and box outlines; ``skeleton``: the limb table, [a, b] joint pairs in draw order
    (None: the COCO-17 table, for that layout only); ``point_colors`` / ``limb_colors``: RGB rows (None: the reference's palettes)."""
    conf_thr: float = 0.5
    radius: int = 0
    thickness: int = 2
    skeleton: tuple | None = None
    point_colors: tuple | None = None
    limb_colors: tuple | None = None

    def __post_init__(self):
        if not (_number(self.conf_thr) and math.isfinite(self.conf_thr)):
            raise ValueError(f'DrawStyle: conf_thr is a finite number, got {self.conf_thr!r}')
        object.__setattr__(self, 'conf_thr', float(self.conf_thr))
        if not (_whole(self.radius) and 0 <= self.radius <= DRAW_MAX_RADIUS):
            raise ValueError(f'DrawStyle: radius in 0..{DRAW_MAX_RADIUS} expected, got {self.radius!r}')
        object.__setattr__(self, 'radius', int(self.radius))
        if not (_whole(self.thickness) and 1 <= self.thickness <= DRAW_MAX_THICKNESS):
            raise ValueError(f'DrawStyle: thickness in 1..{DRAW_MAX_THICKNESS} expected, got {self.thickness!r}')
        object.__setattr__(self, 'thickness', int(self.thickness))
        if self.skeleton is not None:
            object.__setattr__(self, 'skeleton', _pairs(self.skeleton, 'DrawStyle: skeleton'))
        if self.point_colors is not None:
            object.__setattr__(self, 'point_colors', _colors(self.point_colors, 'point_colors'))
        if self.limb_colors is not None:
            object.__setattr__(self, 'limb_colors', _colors(self.limb_colors, 'limb_colors'))


def resolve_skeleton(dataset, K: int, skeleton=None) -> np.ndarray:
    """The uint8 [n_limbs, 2] limb table of a `K`-joint model of `dataset`.  None stands for the COCO-17 skeleton and is accepted for that layout only; any
    other dataset needs its skeleton given (the policy of configs.resolve_flip_pairs and posenms.resolve_sigmas)."""
    if skeleton is None:
        if dataset != 'coco' or K != 17:
            raise ValueError(f'draw: the built-in skeleton is that of the 17-joint COCO layout; dataset {dataset!r} with {K} joints needs its own: '
                             'DrawStyle(skeleton=[[a, b], ...]) / VitInference(skeleton=...) / --skeleton FILE.json')
        skeleton = COCO17_SKELETON
    pairs = _pairs(np.asarray(skeleton).reshape(-1, 2).tolist() if isinstance(skeleton, np.ndarray) else skeleton, 'draw: skeleton')
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if a.size and a.max() >= K:
        raise ValueError(f'draw: the skeleton names joint {int(a.max())}, the model of dataset {dataset!r} has {K}')
    return np.ascontiguousarray(a, dtype=np.uint8)


def load_skeleton(path: str) -> tuple:
    """a JSON file holding a list of [a, b] joint index pairs (the CLI's --skeleton)"""
    import json
    with open(path) as f:
        v = json.load(f)
    if not isinstance(v, list) or not all(isinstance(p, list) and len(p) == 2 and all(isinstance(x, int) and not isinstance(x, bool) for x in p) for p in v):
        raise ValueError(f'{path}: a JSON list of [a, b] joint index pairs expected')
    return _pairs(v, path)


def style_tables(style: DrawStyle, skeleton: np.ndarray):
    """(limbs uint8 [n, 2], point colours uint8 [n, 3], limb colours uint8 [n, 3]) of a call"""
    if not isinstance(style, DrawStyle):
        raise TypeError(f'a DrawStyle expected, got {type(style).__name__}')
    return (np.ascontiguousarray(skeleton, dtype=np.uint8).reshape(-1, 2),
            np.ascontiguousarray(style.point_colors if style.point_colors is not None else POINT_COLORS, dtype=np.uint8).reshape(-1, 3),
            np.ascontiguousarray(style.limb_colors if style.limb_colors is not None else LIMB_COLORS, dtype=np.uint8).reshape(-1, 3))


def c_config(style: DrawStyle, skeleton: np.ndarray):
    """(vp_draw_cfg, the arrays its pointers read: keep them alive for the call)"""
    limbs, pc, lc = style_tables(style, skeleton)
    c = capi.vp_draw_cfg(float(style.conf_thr), int(style.radius), int(style.thickness), int(limbs.shape[0]), limbs.ctypes.data if limbs.size else None,
                         int(pc.shape[0]), pc.ctypes.data, int(lc.shape[0]), lc.ctypes.data)
    return c, (limbs, pc, lc)


def rgb_to_yuv(rgb, matrix='bt601') -> np.ndarray:
    """uint8 [..., 3] RGB -> uint8 [..., 3] (Y, U, V): the numpy twin of csrc/drawgeom.h rgb_to_yuv (int32, arithmetic shift, round(x 2^8) integers)."""
    yoff, my, mu, mv = RGB_YUV_COEFS[_matrix_name(matrix)]
    c = np.asarray(rgb).astype(np.int32)

    def row(m, off):
        return np.clip(off + ((m[0] * c[..., 0] + m[1] * c[..., 1] + m[2] * c[..., 2] + 128) >> 8), 0, 255)
    return np.stack([row(my, yoff), row(mu, 128), row(mv, 128)], -1).astype(np.uint8)


# ---- the numpy twin of csrc/drawgeom.h
def _usable(v) -> bool:
    v = np.float32(v)
    return bool(v > np.float32(-16384.0)) and bool(v < np.float32(16384.0))


def _visible(kp, j: int, thr) -> bool:
    return bool(kp[j, 2] > thr) and _usable(kp[j, 0]) and _usable(kp[j, 1])


def _cover_disk(px, py, cx, cy, r):
    return (px - cx) ** 2 + (py - cy) ** 2 <= r * r


def _cover_limb(px, py, ax, ay, bx, by, t):
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    qx, qy = px - ax, py - ay
    caps = (4 * (qx * qx + qy * qy) <= t * t) | (4 * ((px - bx) ** 2 + (py - by) ** 2) <= t * t)
    if L2 == 0:
        return caps
    dot, cross = qx * dx + qy * dy, qx * dy - qy * dx
    return caps | ((dot >= 0) & (dot <= L2) & (cross * cross <= (t * t * L2) // 4))


def _cover_box(px, py, x1, y1, x2, y2, t):
    o = t // 2
    outer = (px >= x1 - o) & (px <= x2 + o) & (py >= y1 - o) & (py <= y2 + o)
    inner = (px >= x1 - o + t) & (px <= x2 + o - t) & (py >= y1 - o + t) & (py <= y2 + o - t)
    return outer & ~inner


def host_frame(f, i: int) -> Frame:
    if not isinstance(f, Frame):
        f = Frame.rgb(f)
    if f.on_device:
        raise TypeError(f'frame {i}: host (numpy) planes expected')
    if not (1 <= f.h <= DRAW_MAX_DIM and 1 <= f.w <= DRAW_MAX_DIM):
        raise ValueError(f'frame {i}: h and w in 1..{DRAW_MAX_DIM} expected, got {f.h} x {f.w}')
    return f


def check_rows(keypoints, frame_index, rank, ids, boxes):
    """the row arrays of a host call, converted: (kpts float32 [n, K, 3], frame int32 [n], rank / ids int32 [n] or None, boxes float32 [n, 4] or None)"""
    kp = np.ascontiguousarray(keypoints, dtype=np.float32)
    if kp.ndim != 3 or kp.shape[2] != 3:
        raise ValueError(f'keypoints: [n, K, 3] expected, got {kp.shape}')
    n, K = kp.shape[0], kp.shape[1]
    if not 1 <= K <= DRAW_MAX_K:
        raise ValueError(f'keypoints: K in 1..{DRAW_MAX_K} expected, got {K}')
    fi = np.ascontiguousarray(frame_index, dtype=np.int32)
    rk = None if rank is None else np.ascontiguousarray(rank, dtype=np.int32)
    pid = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    bx = None if boxes is None else np.ascontiguousarray(boxes, dtype=np.float32)
    if fi.shape != (n,) or (rk is not None and rk.shape != (n,)) or (pid is not None and pid.shape != (n,)) or (bx is not None and bx.shape != (n, 4)):
        raise ValueError(f'frame_index [{n}], rank [{n}], ids [{n}] and boxes [{n}, 4] expected')
    return kp, fi, rk, pid, bx


def check_records(n: int, K: int, n_limbs: int, has_box: bool):
    if n * (int(has_box) + n_limbs + K) > DRAW_MAX_RECORDS:
        raise ValueError(f'draw: {n} rows of {int(has_box) + n_limbs + K} primitives exceed the {DRAW_MAX_RECORDS} records of one call')


def draw_poses_numpy(frames, keypoints, frame_index, style: DrawStyle = DrawStyle(), rank=None, ids=None, boxes=None, dataset='coco', labels=None, scores=None):
    """The numpy twin of csrc/drawgeom.h: draws in place on host `frames` (`Frame` objects over numpy planes, or bare [H, W, 3] RGB arrays) and returns
    them as `Frame`s.  Primitive by primitive in draw order, a later one overwriting an earlier one, which is the header's "last primitive that covers it".
    `labels`: a `LabelStyle` writes the tags of `draw_labels_numpy` first, under the skeletons (it needs `boxes`; `scores` are the tags' scores)."""
    if not isinstance(style, DrawStyle):
        raise TypeError(f'a DrawStyle expected, got {type(style).__name__}')
    frames = [host_frame(f, i) for i, f in enumerate(frames)]
    kp, fi, rk, pid, bx = check_rows(keypoints, frame_index, rank, ids, boxes)
    n, K = kp.shape[0], kp.shape[1]
    limbs, pcol, lcol = style_tables(style, resolve_skeleton(dataset, K, style.skeleton))
    check_records(n, K, limbs.shape[0], bx is not None)
    if labels is not None:
        draw_labels_numpy(frames, label_boxes(bx), fi, overlay_label_style(labels, style), rank=rk, ids=pid, scores=scores)
    thr, t = np.float32(style.conf_thr), int(style.thickness)
    for i in range(n):
        f = int(fi[i])
        if f < 0 or f >= len(frames) or (rk is not None and rk[i] < 0):
            continue
        fr = frames[f]
        h, w = fr.h, fr.w
        pid_i = int(pid[i]) if pid is not None else i

        def paint(rgb, x0, y0, x1, y1, cover):
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
            if x0 > x1 or y0 > y1:
                return
            py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
            m = cover(px, py)
            if fr.format == 'nv12':
                yuv = rgb_to_yuv(np.asarray(rgb, dtype=np.uint8), fr.matrix)
                fr.planes[0][y0:y1 + 1, x0:x1 + 1][m] = yuv[0]
                fr.planes[1][py[m] >> 1, px[m] >> 1] = yuv[1:]
            else:
                fr.planes[0][y0:y1 + 1, x0:x1 + 1][m] = rgb[::-1] if fr.format == 'bgr' else rgb
        lc = lcol[pid_i % lcol.shape[0]]   # Python's % is the mathematical mod
        if bx is not None and all(_usable(v) for v in bx[i]):
            xa, ya, xb, yb = (int(v) for v in bx[i])   # int(): truncation toward zero
            x1, x2, y1, y2 = min(xa, xb), max(xa, xb), min(ya, yb), max(ya, yb)
            o = t // 2
            paint(lc, x1 - o, y1 - o, x2 + o, y2 + o, lambda px, py: _cover_box(px, py, x1, y1, x2, y2, t))
        vis = [_visible(kp[i], j, thr) for j in range(K)]
        for a, b in limbs.tolist():
            if vis[a] and vis[b]:
                ax, ay, bx_, by_ = int(kp[i, a, 1]), int(kp[i, a, 0]), int(kp[i, b, 1]), int(kp[i, b, 0])
                o = (t + 1) // 2
                paint(lc, min(ax, bx_) - o, min(ay, by_) - o, max(ax, bx_) + o, max(ay, by_) + o,
                      lambda px, py: _cover_limb(px, py, ax, ay, bx_, by_, t))
        r = style.radius if style.radius > 0 else max(1, min(h, w) // 150)
        for j in range(K):
            if vis[j]:
                cx, cy = int(kp[i, j, 1]), int(kp[i, j, 0])
                paint(pcol[j % pcol.shape[0]], cx - r, cy - r, cx + r, cy + r, lambda px, py: _cover_disk(px, py, cx, cy, r))
    return frames


def image_table(frames):
    """the vp_image table of host `Frame`s (they keep the planes alive)"""
    import ctypes as C
    table = (capi.vp_image * max(len(frames), 1))()
    for i, f in enumerate(frames):
        p0, p1 = f.pointers()
        table[i] = capi.vp_image((C.c_void_p * 2)(p0, p1), (C.c_int64 * 2)(*f.pitch), f.h, f.w, PIX_FORMATS[f.format], YUV_MATRIX_IDS[f.matrix])
    return table


def draw_poses_model_host(frames, keypoints, frame_index, style: DrawStyle = DrawStyle(), rank=None, ids=None, boxes=None, dataset='coco', labels=None, scores=None):
    """vp_dbg_draw_host on host frames, in place: csrc/drawgeom.h run pixel by pixel in C++ on one core, no device.  A test and measurement tap, never a
    fallback of the device entry.  `labels`: a `LabelStyle` runs vp_dbg_draw_labels_host first (it needs `boxes`)."""
    import ctypes as C
    if not isinstance(style, DrawStyle):
        raise TypeError(f'a DrawStyle expected, got {type(style).__name__}')
    frames = [host_frame(f, i) for i, f in enumerate(frames)]
    kp, fi, rk, pid, bx = check_rows(keypoints, frame_index, rank, ids, boxes)
    c, keep = c_config(style, resolve_skeleton(dataset, kp.shape[1], style.skeleton))
    lib = capi.load_library()
    if labels is not None:
        draw_labels_model_host(frames, label_boxes(bx), fi, overlay_label_style(labels, style), rank=rk, ids=pid, scores=scores)
    capi.check(lib.vp_dbg_draw_host(image_table(frames), len(frames), kp.ctypes.data, kp.shape[0], kp.shape[1], fi.ctypes.data, 1,
                                    None if rk is None else rk.ctypes.data, None if pid is None else pid.ctypes.data,
                                    None if bx is None else bx.ctypes.data, 4, C.byref(c)))
    return frames


# ---- the label stage (vp_draw_labels_stream; semantics in csrc/labelgeom.h): the style, the text, the font and the numpy twin of the header
# Modelled on the reference's ``draw_bboxes`` (`#<id>: <score>` on a filled tag at the top-left corner of a tracked box).  The font is this project's own 5 x 7
# bitmap font over 16 symbols: parity against OpenCV's Hershey font is UNPINNED and not claimed.
LABEL_ALPHABET = '#0123456789:.- ?'   # code -> character; '?' stands for the spare symbol (a hollow box), which no text produces
# glyph g, bit 5 * row + col (row 0 the top one, col 0 the left one) set = ink: csrc/labelgeom.h label_glyph
LABEL_GLYPHS = (0x295f57d4a, 0x3a33ae62e, 0x3884210c4, 0x7c444422e, 0x3a304111f, 0x211f4a988, 0x3a3083c3f, 0x3a317844c, 0x08422221f, 0x3a317462e,
                0x1910f462e, 0x008401080, 0x18c000000, 0x0000f8000, 0x000000000, 0x7e318c63f)


@dataclasses.dataclass(frozen=True)
class LabelStyle:
    """``scale``: pixels per font bit, 1..8, 0 for ``max(1, min(h, w) // 400)`` of the frame (at most 8); ``colors``: RGB rows, the background of a tag is
    ``colors[id mod n]`` (None: the overlay's limb palette, so a tag has its person's colour); ``ink``: an (R, G, B) colour, None for black on a light
    background and white on a dark one; ``show_score``: print ``: <score>`` behind the id when scores are given."""
    scale: int = 0
    colors: tuple | None = None
    ink: tuple | None = None
    show_score: bool = True

    def __post_init__(self):
        if not (_whole(self.scale) and 0 <= self.scale <= LABEL_MAX_SCALE):
            raise ValueError(f'LabelStyle: scale in 0..{LABEL_MAX_SCALE} expected, got {self.scale!r}')
        object.__setattr__(self, 'scale', int(self.scale))
        if self.colors is not None:
            try:
                object.__setattr__(self, 'colors', _colors(self.colors, 'colors'))
            except ValueError as e:
                raise ValueError(str(e).replace('DrawStyle', 'LabelStyle')) from None
        if self.ink is not None:
            try:
                ink = tuple(self.ink)
            except TypeError:
                raise ValueError('LabelStyle: ink is an (R, G, B) colour or None') from None
            if len(ink) != 3 or not all(_whole(x) and 0 <= x <= 255 for x in ink):
                raise ValueError('LabelStyle: ink is an (R, G, B) colour of integers in 0..255 or None')
            object.__setattr__(self, 'ink', tuple(int(x) for x in ink))
        if not isinstance(self.show_score, (bool, np.bool_)):
            raise ValueError(f'LabelStyle: show_score is a bool, got {self.show_score!r}')
        object.__setattr__(self, 'show_score', bool(self.show_score))


def overlay_label_style(labels, style: DrawStyle):
    """the `LabelStyle` of draw_poses(labels=): without colours of its own it takes the overlay's limb palette"""
    if not isinstance(labels, LabelStyle):
        raise TypeError(f'labels: a LabelStyle or None expected, got {type(labels).__name__}')
    if labels.colors is None and style.limb_colors is not None:
        return dataclasses.replace(labels, colors=style.limb_colors)
    return labels


def label_boxes(boxes):
    if boxes is None:
        raise ValueError('labels: a tag sits at the corner of its box: boxes are required')
    return boxes


def label_colors(style: LabelStyle) -> np.ndarray:
    if not isinstance(style, LabelStyle):
        raise TypeError(f'a LabelStyle expected, got {type(style).__name__}')
    return np.ascontiguousarray(style.colors if style.colors is not None else LIMB_COLORS, dtype=np.uint8).reshape(-1, 3)


def label_c_config(style: LabelStyle):
    """(vp_label_cfg, the arrays its pointers read: keep them alive for the call)"""
    import ctypes as C
    col = label_colors(style)
    ink = style.ink if style.ink is not None else (0, 0, 0)
    c = capi.vp_label_cfg(int(style.scale), int(col.shape[0]), col.ctypes.data, int(style.ink is None), (C.c_uint8 * 3)(*ink), int(style.show_score))
    return c, (col,)


def label_hundredths(score) -> int:
    """hundredths of |score| for a float32 with |score| < 1000, rounded half-to-even on the exact binary value, in integers: csrc/labelgeom.h label_hundredths"""
    bits = int(np.array(score, dtype=np.float32).view(np.uint32))
    e, m = (bits >> 23) & 0xff, bits & 0x7fffff
    M, sh = (m | 0x800000, 150 - e) if e else (m, 149)
    v = 100 * M
    q, r = v >> sh, v & ((1 << sh) - 1)
    half = 1 << (sh - 1)
    return q + (1 if r > half or (r == half and q & 1) else 0)


def label_text(id, score=None) -> str:
    """The text of a tag: ``#<id>``, and ``: <score>`` with two decimals iff a score is given and -1000 < score < 1000 (never for NaN).  The integer statement
    of csrc/labelgeom.h label_format: equal to ``f'#{id}: {float(np.float32(score)):.2f}'`` for every such float32."""
    id = int(id)
    if not -2 ** 31 <= id < 2 ** 31:
        raise ValueError(f'label_text: an int32 id expected, got {id}')
    text = '#' + str(id)
    if score is None:
        return text
    s = np.float32(score)
    if not (s > np.float32(-1000.0) and s < np.float32(1000.0)):
        return text
    q = label_hundredths(s)
    return text + ': ' + ('-' if np.signbit(s) else '') + f'{q // 100}.{q % 100:02d}'


def label_glyph_bitmap(code: int) -> np.ndarray:
    """bool [7, 5] of glyph `code`"""
    g = LABEL_GLYPHS[code]
    return np.array([[(g >> (5 * r + c)) & 1 for c in range(5)] for r in range(7)], dtype=bool)


def check_label_rows(boxes, frame_index, rank, ids, scores):
    """the row arrays of a host label call, converted: (boxes float32 [n, 4], frame int32 [n], rank / ids int32 [n] or None, scores float32 [n] or None)"""
    if boxes is None:
        raise ValueError('labels: a tag sits at the corner of its box: boxes are required')
    bx = np.ascontiguousarray(boxes, dtype=np.float32)
    if bx.ndim != 2 or bx.shape[1] != 4:
        raise ValueError(f'boxes: [n, 4] expected, got {bx.shape}')
    n = bx.shape[0]
    if n > LABEL_MAX_ROWS:
        raise ValueError(f'labels: {n} rows exceed the {LABEL_MAX_ROWS} records of one call')
    fi = np.ascontiguousarray(frame_index, dtype=np.int32)
    rk = None if rank is None else np.ascontiguousarray(rank, dtype=np.int32)
    pid = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    sc = None if scores is None else np.ascontiguousarray(scores, dtype=np.float32)
    if fi.shape != (n,) or (rk is not None and rk.shape != (n,)) or (pid is not None and pid.shape != (n,)) or (sc is not None and sc.shape != (n,)):
        raise ValueError(f'frame_index [{n}], rank [{n}], ids [{n}] and scores [{n}] expected')
    return bx, fi, rk, pid, sc


def draw_labels_numpy(frames, boxes, frame_index, style: LabelStyle = LabelStyle(), rank=None, ids=None, scores=None):
    """The numpy twin of csrc/labelgeom.h: writes the tags in place on host `frames` and returns them as `Frame`s.  Row by row in order, the block of a tag
    in its background colour and then its ink, a later row overwriting an earlier one: the header's "highest order index that covers it"."""
    col = label_colors(style)
    frames = [host_frame(f, i) for i, f in enumerate(frames)]
    bx, fi, rk, pid, sc = check_label_rows(boxes, frame_index, rank, ids, scores)
    for i in range(bx.shape[0]):
        f = int(fi[i])
        if f < 0 or f >= len(frames) or (rk is not None and rk[i] < 0) or not all(_usable(v) for v in bx[i]):
            continue
        fr = frames[f]
        h, w = fr.h, fr.w
        xa, ya, xb, yb = (int(v) for v in bx[i])   # int(): truncation toward zero
        x1, y1 = min(xa, xb), min(ya, yb)
        pid_i = int(pid[i]) if pid is not None else i
        text = label_text(pid_i, sc[i] if sc is not None and style.show_score else None)
        s = style.scale if style.scale > 0 else min(max(1, min(h, w) // 400), LABEL_MAX_SCALE)
        by = y1 - 9 * s if y1 - 9 * s >= 0 else y1
        cells = np.zeros((9, 6 * len(text) + 1), dtype=bool)   # the tag at scale 1: a margin of one bit, glyph c at (1 + 6 c, 1)
        for c, ch in enumerate(text):
            cells[1:8, 1 + 6 * c:6 + 6 * c] = label_glyph_bitmap(LABEL_ALPHABET.index(ch))
        ink_mask = np.kron(cells, np.ones((s, s), dtype=bool))   # every bit an s x s square
        x0, y0, xe, ye = max(x1, 0), max(by, 0), min(x1 + ink_mask.shape[1], w), min(by + ink_mask.shape[0], h)
        if x0 >= xe or y0 >= ye:
            continue
        m = ink_mask[y0 - by:ye - by, x0 - x1:xe - x1]
        bg = col[pid_i % col.shape[0]]   # Python's % is the mathematical mod
        if style.ink is not None:
            ink = np.array(style.ink, dtype=np.uint8)
        else:
            ink = np.full(3, 0 if 77 * int(bg[0]) + 150 * int(bg[1]) + 29 * int(bg[2]) >= 32768 else 255, dtype=np.uint8)
        if fr.format == 'nv12':
            ybg, yink = rgb_to_yuv(bg, fr.matrix), rgb_to_yuv(ink, fr.matrix)
            fr.planes[0][y0:ye, x0:xe] = np.where(m, yink[0], ybg[0])
            fr.planes[1][y0 >> 1:((ye - 1) >> 1) + 1, x0 >> 1:((xe - 1) >> 1) + 1] = ybg[1:]
            py, px = np.nonzero(m)
            fr.planes[1][(py + y0) >> 1, (px + x0) >> 1] = yink[1:]
        else:
            a, b = (bg[::-1], ink[::-1]) if fr.format == 'bgr' else (bg, ink)
            fr.planes[0][y0:ye, x0:xe] = np.where(m[..., None], b, a)
    return frames


def draw_labels_model_host(frames, boxes, frame_index, style: LabelStyle = LabelStyle(), rank=None, ids=None, scores=None):
    """vp_dbg_draw_labels_host on host frames, in place: csrc/labelgeom.h run pixel by pixel in C++ on one core, no device.  A test and measurement tap, never
    a fallback of the device entry."""
    import ctypes as C
    c, keep = label_c_config(style)
    frames = [host_frame(f, i) for i, f in enumerate(frames)]
    bx, fi, rk, pid, sc = check_label_rows(boxes, frame_index, rank, ids, scores)
    lib = capi.load_library()
    capi.check(lib.vp_dbg_draw_labels_host(image_table(frames), len(frames), bx.ctypes.data, 4, bx.shape[0], fi.ctypes.data, 1,
                                           None if rk is None else rk.ctypes.data, None if pid is None else pid.ctypes.data,
                                           None if sc is None else sc.ctypes.data, 1, C.byref(c)))
    return frames
