"""The skeleton overlay contract (csrc/drawgeom.h) restated in plain scalar Python, as a GATHER: every primitive of the call gets its place in the draw
order, every pixel takes the highest-placed primitive that covers it, every chroma sample the highest-placed one among its up-to-four pixels.  The host tap and
the numpy twin are painters (a later primitive overwrites an earlier one); this file is the other formulation, so agreement of the three pins the order rule.

Plain Python integers (unbounded), float32 compares through numpy scalars; no bounding box of the header is used: a primitive is tested on a window that is
generous by construction (its extent plus its full thickness or radius on every side).
"""
import numpy as np

YUV = {   # matrix -> (yoff, Y row, U row, V row) over (R, G, B): round(x * 256) of the standard matrices, checked against fp64 in test_draw_host.py
    'bt601': (16, (66, 129, 25), (-38, -74, 112), (112, -94, -18)),
    'bt709': (16, (47, 157, 16), (-26, -87, 112), (112, -102, -10)),
    'bt601_full': (0, (77, 150, 29), (-43, -85, 128), (128, -107, -21)),
}


def clip255(v):
    return 0 if v < 0 else (255 if v > 255 else v)


def rgb_to_yuv(rgb, matrix):
    yoff, my, mu, mv = YUV[matrix]
    r, g, b = (int(c) for c in rgb)
    return (clip255(yoff + ((my[0] * r + my[1] * g + my[2] * b + 128) >> 8)),
            clip255(128 + ((mu[0] * r + mu[1] * g + mu[2] * b + 128) >> 8)),
            clip255(128 + ((mv[0] * r + mv[1] * g + mv[2] * b + 128) >> 8)))


def usable(v):
    v = float(v)
    return -16384.0 < v < 16384.0   # False for NaN and the infinities


def covers(prim, px, py):
    kind = prim[0]
    if kind == 'disk':
        _, cx, cy, r = prim
        return (px - cx) ** 2 + (py - cy) ** 2 <= r * r
    if kind == 'limb':
        _, ax, ay, bx, by, t = prim
        if 4 * ((px - ax) ** 2 + (py - ay) ** 2) <= t * t or 4 * ((px - bx) ** 2 + (py - by) ** 2) <= t * t:
            return True
        dx, dy = bx - ax, by - ay
        L2 = dx * dx + dy * dy
        if L2 == 0:
            return False
        qx, qy = px - ax, py - ay
        dot, cross = qx * dx + qy * dy, qx * dy - qy * dx
        return 0 <= dot <= L2 and cross * cross <= (t * t * L2) // 4
    _, x1, y1, x2, y2, t = prim
    o = t // 2
    if not (x1 - o <= px <= x2 + o and y1 - o <= py <= y2 + o):
        return False
    return not (x1 - o + t <= px <= x2 + o - t and y1 - o + t <= py <= y2 + o - t)


def window(prim):
    kind = prim[0]
    if kind == 'disk':
        _, cx, cy, r = prim
        return cx - r, cy - r, cx + r, cy + r
    _, ax, ay, bx, by, t = prim
    return min(ax, bx) - t, min(ay, by) - t, max(ax, bx) + t, max(ay, by) + t


def primitives(kp, frame_index, n_frames, hw, limbs, point_colors, limb_colors, conf_thr, radius, thickness, rank=None, ids=None, boxes=None):
    """[(frame, primitive, RGB colour)] of the call in draw order"""
    out = []
    thr = np.float32(conf_thr)
    for i in range(len(kp)):
        f = int(frame_index[i])
        if f < 0 or f >= n_frames or (rank is not None and int(rank[i]) < 0):
            continue
        pid = int(ids[i]) if ids is not None else i
        lc = tuple(limb_colors[pid % len(limb_colors)])
        if boxes is not None and all(usable(v) for v in boxes[i]):
            xa, ya, xb, yb = (int(float(v)) for v in boxes[i])
            out.append((f, ('box', min(xa, xb), min(ya, yb), max(xa, xb), max(ya, yb), thickness), lc))
        vis = [bool(np.float32(kp[i][j][2]) > thr) and usable(kp[i][j][0]) and usable(kp[i][j][1]) for j in range(len(kp[i]))]
        pix = [(int(float(kp[i][j][1])), int(float(kp[i][j][0]))) if vis[j] else None for j in range(len(kp[i]))]
        for a, b in limbs:
            if vis[a] and vis[b]:
                out.append((f, ('limb', pix[a][0], pix[a][1], pix[b][0], pix[b][1], thickness), lc))
        h, w = hw[f]
        r = radius if radius > 0 else max(1, min(h, w) // 150)
        for j in range(len(kp[i])):
            if vis[j]:
                out.append((f, ('disk', pix[j][0], pix[j][1], r), tuple(point_colors[j % len(point_colors)])))
    return out


def winners(prims, f, h, w):
    """win [h][w]: the place in `prims` of the last primitive of frame f that covers the pixel, -1 for none"""
    win = [[-1] * w for _ in range(h)]
    for place, (pf, prim, _) in enumerate(prims):
        if pf != f:
            continue
        x0, y0, x1, y1 = window(prim)
        for py in range(max(y0, 0), min(y1, h - 1) + 1):
            row = win[py]
            for px in range(max(x0, 0), min(x1, w - 1) + 1):
                if covers(prim, px, py):
                    row[px] = place   # places ascend, so the last assignment is the highest
    return win


def draw_model(frames, kp, frame_index, limbs, point_colors, limb_colors, conf_thr, radius, thickness, rank=None, ids=None, boxes=None):
    """Draws in place on `frames` (cropprep.Frame over numpy planes) byte by byte.  Returns per frame the list of (plane, row, byte column) it wrote."""
    prims = primitives(kp, frame_index, len(frames), [(fr.h, fr.w) for fr in frames], limbs, point_colors, limb_colors, conf_thr, radius, thickness, rank, ids, boxes)
    written = []
    for f, fr in enumerate(frames):
        win = winners(prims, f, fr.h, fr.w)
        wr = []
        if fr.format != 'nv12':
            for py in range(fr.h):
                for px in range(fr.w):
                    if win[py][px] >= 0:
                        rgb = prims[win[py][px]][2]
                        for c in range(3):
                            fr.planes[0][py, px, c] = rgb[2 - c] if fr.format == 'bgr' else rgb[c]
                            wr.append((0, py, 3 * px + c))
        else:
            for py in range(fr.h):
                for px in range(fr.w):
                    if win[py][px] >= 0:
                        fr.planes[0][py, px] = rgb_to_yuv(prims[win[py][px]][2], fr.matrix)[0]
                        wr.append((0, py, px))
            for cy in range((fr.h + 1) // 2):
                for cx in range((fr.w + 1) // 2):
                    best = max(win[py][px] for py in (2 * cy, 2 * cy + 1) if py < fr.h for px in (2 * cx, 2 * cx + 1) if px < fr.w)
                    if best >= 0:
                        _, u, v = rgb_to_yuv(prims[best][2], fr.matrix)
                        fr.planes[1][cy, cx, 0], fr.planes[1][cy, cx, 1] = u, v
                        wr += [(1, cy, 2 * cx), (1, cy, 2 * cx + 1)]
        written.append(wr)
    return written
