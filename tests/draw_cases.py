"""Seeded cases of the skeleton overlay (csrc/drawgeom.h) and the runners that draw one case through each statement of the contract: the host tap
vp_dbg_draw_host, the numpy twin, the scalar model of tests/draw_model.py, and the device (vp_draw_poses).  Shared by tests/test_draw_host.py and
tests/test_gpu_draw.py; a case is data only and is never modified: every runner draws on fresh frames built from the case's seed.

A frame is built inside a larger seeded buffer: rows at a pitch when the spec asks for it, so that the bytes beside the frame (the pitch padding) are a
sentinel, and a runner returns the WHOLE buffers -- comparing them checks the padding too.
"""
import numpy as np

from easy_vitpose_amd.cropprep import Frame
from easy_vitpose_amd.draw import COCO17_SKELETON, LIMB_COLORS, POINT_COLORS, DrawStyle, draw_poses_model_host, draw_poses_numpy

ODD, EVEN = (97, 131), (64, 96)


def build_frames(specs, seed):
    """specs: [(h, w, format, matrix, pad)] -> (frames, buffers): `Frame`s that are views of the seeded uint8 `buffers` (one per plane)"""
    rng = np.random.default_rng(seed)
    frames, buffers = [], []
    for h, w, fmt, matrix, pad in specs:
        if fmt == 'nv12':
            cw, ch = (w + 1) // 2, (h + 1) // 2
            by = rng.integers(0, 256, (h, w + pad), dtype=np.uint8)
            buv = rng.integers(0, 256, (ch, 2 * cw + pad), dtype=np.uint8)
            frames.append(Frame.nv12(by[:, :w], buv[:, :2 * cw].reshape(ch, cw, 2), matrix))
            buffers += [by, buv]
        else:
            b = rng.integers(0, 256, (h, 3 * w + pad), dtype=np.uint8)
            frames.append(Frame(fmt, (b[:, :3 * w].reshape(h, w, 3),)))
            buffers.append(b)
    return frames, buffers


def people(rng, n, K, h, w, spread=30.0):
    """n persons of K joints around seeded centres on an h x w frame, confidences on both sides of 0.5"""
    c = np.stack([rng.uniform(-5, h + 5, n), rng.uniform(-5, w + 5, n)], -1)
    kp = np.empty((n, K, 3), np.float32)
    kp[..., :2] = c[:, None, :] + rng.uniform(-spread, spread, (n, K, 2))
    kp[..., 2] = rng.uniform(0.25, 1.0, (n, K))
    return kp


def boxes_of(kp, rng):
    lo, hi = kp[..., :2].min(1), kp[..., :2].max(1)
    return np.stack([lo[:, 1] - 3, lo[:, 0] - 3, hi[:, 1] + 3, hi[:, 0] + 3], -1).astype(np.float32) + rng.uniform(0, 1, (len(kp), 4)).astype(np.float32)


def case(specs, kp, fi, style=DrawStyle(), rank=None, ids=None, boxes=None, seed=0):
    return dict(specs=specs, kp=np.asarray(kp, np.float32), fi=np.asarray(fi, np.int32), style=style, rank=None if rank is None else np.asarray(rank, np.int32),
                ids=None if ids is None else np.asarray(ids, np.int32), boxes=None if boxes is None else np.asarray(boxes, np.float32), seed=seed)


def skeleton133(seed=7):
    rng = np.random.default_rng(seed)
    return tuple(map(tuple, rng.integers(0, 133, (150, 2)).tolist()))


def edge_rows():
    """K = 17 rows on a 97 x 131 frame that exercise the gates: row 0 confidences at, just above and below 0.5 and a NaN; row 1 NaN / inf coordinates;
    row 2 coordinates at +-16383.x (usable) and +-16384 (not), joined by limbs; row 3 limbs that cross the whole frame from far outside"""
    kp = np.zeros((4, 17, 3), np.float32)
    kp[..., 2] = 0.9
    for i in range(4):
        kp[i, :, 0] = 20 + 3 * np.arange(17) + i
        kp[i, :, 1] = 15 + 6 * np.arange(17)
    kp[0, :6, 2] = [0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(0)), np.nan, np.inf, -np.inf]
    kp[1, 5, 0], kp[1, 6, 1], kp[1, 7, 0], kp[1, 8, 1], kp[1, 9, :2] = np.nan, np.nan, np.inf, -np.inf, (np.inf, np.nan)
    kp[2, 0, :2] = (40.7, 16383.5)                  # pixel x = 16383: visible, far right of the frame
    kp[2, 1, :2] = (40.2, -16383.9)                 # pixel x = -16383
    kp[2, 2, :2] = (16384.0, 50.0)                  # not usable
    kp[2, 3, :2] = (-16384.0, 50.0)                 # not usable
    kp[2, 5, :2] = (-16383.99, 60.0)
    kp[2, 6, :2] = (16383.99, 70.0)
    kp[2, 11, :2] = (np.float32(16384.0) - np.float32(0.001), 10.0)   # rounds to 16383.999: usable
    kp[3, 15, :2], kp[3, 13, :2] = (-9000.0, -16383.0), (9000.0, 16383.0)   # limb (15, 13): corner to corner and beyond
    kp[3, 16, :2], kp[3, 14, :2] = (48.0, -12000.0), (48.9, 12000.0)        # limb (16, 14): a horizontal line through the frame
    kp[3, 5, :2], kp[3, 7, :2] = (-7000.0, 65.0), (7000.0, 66.0)            # limb (5, 7): a near-vertical one
    kp[3, 0, :2], kp[3, 1, :2] = (-0.9, -0.9), (96.99, 130.99)              # truncation toward zero: pixel (0, 0), and the last pixel
    return kp


def host_cases():
    """name -> case: the CPU set (also the device's)"""
    out = {}
    rng = np.random.default_rng(11)
    for fmt, matrix in (('rgb', 'bt601'), ('bgr', 'bt601'), ('nv12', 'bt601'), ('nv12', 'bt709'), ('nv12', 'bt601_full')):
        for (h, w) in (ODD, EVEN):
            kp = people(rng, 4, 17, h, w)
            name = f'{fmt}_{matrix}_{h}x{w}'
            out[name] = case([(h, w, fmt, matrix, 0)], kp, np.zeros(4), ids=[3, -1, -9, 12], boxes=boxes_of(kp, rng) if h == 97 else None, seed=len(out))
    for fmt in ('rgb', 'nv12'):
        kp = people(rng, 3, 17, *ODD)
        out[f'{fmt}_pitched'] = case([(97, 131, fmt, 'bt709', 37)], kp, np.zeros(3), boxes=boxes_of(kp, rng), seed=40)
    kp = people(rng, 2, 133, *EVEN, spread=40.0)
    out['k133'] = case([(64, 96, 'rgb', 'bt601', 0)], kp, np.zeros(2), style=DrawStyle(skeleton=skeleton133()), seed=41)
    kp = people(rng, 2, 133, *ODD, spread=40.0)
    out['k133_nv12'] = case([(97, 131, 'nv12', 'bt601', 5)], kp, np.zeros(2), style=DrawStyle(skeleton=skeleton133(), thickness=3, radius=2), seed=42)
    kp = np.concatenate([people(rng, 3, 17, *ODD), people(rng, 3, 17, *EVEN)])[[0, 3, 1, 4, 2, 5]]
    out['two_frames'] = case([(97, 131, 'rgb', 'bt601', 0), (64, 96, 'nv12', 'bt709', 3)], kp, [0, 1, 0, 1, 0, 1], boxes=boxes_of(kp, rng), seed=43)
    kp = people(rng, 6, 17, *ODD)
    out['rank_mask'] = case([(97, 131, 'bgr', 'bt601', 0)], kp, np.zeros(6), rank=[0, -1, 2, -2, 1, -1], ids=[5, 6, 7, 8, 9, 10], seed=44)
    for fmt in ('rgb', 'nv12'):
        out[f'edges_{fmt}'] = case([(97, 131, fmt, 'bt601', 0)], edge_rows(), np.zeros(4), seed=45)
    bx = np.array([[10, 10, 60, 50], [np.nan, 0, 5, 5], [-16383.5, -16383.5, 16383.5, 16383.5], [16384, 0, 5, 5], [70.9, 40.9, 20.1, 5.1]], np.float32)
    out['edge_boxes'] = case([(97, 131, 'nv12', 'bt601_full', 0)], people(rng, 5, 17, *ODD), np.zeros(5), boxes=bx, style=DrawStyle(thickness=3), seed=46)
    kp = people(rng, 4, 17, *ODD)
    out['no_row_frame'] = case([(97, 131, 'rgb', 'bt601', 0), (64, 96, 'nv12', 'bt601', 0), (64, 96, 'bgr', 'bt601', 0)], kp, [0, -1, 3, 2], seed=47)
    for t, r in ((1, 1), (5, 7), (16, 64)):
        kp = people(rng, 2, 17, *ODD)
        out[f'style_t{t}_r{r}'] = case([(97, 131, 'nv12', 'bt601', 0)], kp, np.zeros(2), boxes=boxes_of(kp, rng),
                                      style=DrawStyle(thickness=t, radius=r, conf_thr=0.4, point_colors=[(1, 2, 3), (250, 128, 7)], limb_colors=[(9, 200, 30)]), seed=48 + t)
    return out


def lds_list_case(fmt):
    """300 rows of 17 joints on the same 20 x 20 region of a 64 x 96 frame: far more than 256 records per chunk, and more hits on one tile than the LDS list holds"""
    rng = np.random.default_rng(5)
    kp = np.empty((300, 17, 3), np.float32)
    kp[..., 0] = rng.uniform(30, 50, (300, 17))
    kp[..., 1] = rng.uniform(40, 60, (300, 17))
    kp[..., 2] = rng.uniform(0.3, 1.0, (300, 17))
    return case([(64, 96, fmt, 'bt601', 0)], kp, np.zeros(300), ids=rng.integers(-50, 50, 300), seed=60)


def chunk_boundary_case():
    """9 rows x (19 limbs + 17 joints) = 324 records; row 7 (records 252..287) straddles record 256, and every row's joints sit in one 32 x 8 tile region so that the
    tile's hits come from both chunks"""
    rng = np.random.default_rng(6)
    kp = np.empty((9, 17, 3), np.float32)
    kp[..., 0] = rng.uniform(16, 24, (9, 17))
    kp[..., 1] = rng.uniform(32, 64, (9, 17))
    kp[..., 2] = 0.9
    kp[:4, :, :2] += rng.uniform(-15, 30, (4, 17, 2)).astype(np.float32)   # some rows spread over the neighbouring tiles
    return case([(64, 96, 'rgb', 'bt601', 0)], kp, np.zeros(9), seed=61)


# ---- runners: draw a case on fresh frames, return the whole buffers
def _tables(cs):
    K = cs['kp'].shape[1]
    st = cs['style']
    limbs = st.skeleton if st.skeleton is not None else COCO17_SKELETON
    assert K == 17 or st.skeleton is not None
    return (limbs, st.point_colors if st.point_colors is not None else POINT_COLORS, st.limb_colors if st.limb_colors is not None else LIMB_COLORS)


def run_tap(cs):
    frames, buffers = build_frames(cs['specs'], cs['seed'])
    draw_poses_model_host(frames, cs['kp'], cs['fi'], cs['style'], rank=cs['rank'], ids=cs['ids'], boxes=cs['boxes'])
    return buffers


def run_numpy(cs):
    frames, buffers = build_frames(cs['specs'], cs['seed'])
    draw_poses_numpy(frames, cs['kp'], cs['fi'], cs['style'], rank=cs['rank'], ids=cs['ids'], boxes=cs['boxes'])
    return buffers


def run_model(cs):
    """(buffers, written): the scalar model's picture and, per frame, the bytes it wrote"""
    from draw_model import draw_model
    frames, buffers = build_frames(cs['specs'], cs['seed'])
    limbs, pc, lc = _tables(cs)
    st = cs['style']
    written = draw_model(frames, cs['kp'], cs['fi'], limbs, pc, lc, st.conf_thr, st.radius, st.thickness, rank=cs['rank'], ids=cs['ids'], boxes=cs['boxes'])
    return buffers, written


def run_device(cs, engine):
    frames, buffers = build_frames(cs['specs'], cs['seed'])
    engine.draw_poses_host(frames, cs['kp'], cs['fi'], cs['style'], rank=cs['rank'], ids=cs['ids'], boxes=cs['boxes'])
    return buffers


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
