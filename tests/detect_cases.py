"""Shared by tests/test_detect_host.py and tests/test_gpu_detect.py: a numpy twin of the detector stage (include/vitpose_hip.h, "The detector stage"), written
from the contract and not from csrc/detgeom.h, and the heads both suites run.  A case is (DetectCfg, pred, frames_hw, input_hw, n_out)."""
from __future__ import annotations

import functools

import numpy as np

from easy_vitpose_amd.devdetect import MAX_CAND, DetectCfg, letterbox_params

F32 = np.float32
NP = {'fp16': np.float16, 'fp32': np.float32}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the twin
def _iou_row(a, b, e):
    """float32 IoU of box a [4] against boxes b [m, 4], operation by operation as the contract states them"""
    lx, ly = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    hx, hy = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    iw, ih = (hx - lx) + e, (hy - ly) + e
    iw, ih = np.where(iw < 0, F32(0), iw), np.where(ih < 0, F32(0), ih)
    inter = iw * ih
    area_a = ((a[2] - a[0]) + e) * ((a[3] - a[1]) + e)
    area_b = ((b[:, 2] - b[:, 0]) + e) * ((b[:, 3] - b[:, 1]) + e)
    return inter / ((area_a + area_b) - inter)


def twin(cfg: DetectCfg, pred, frames_hw, input_hw, n_out=None):
    pred = np.asarray(pred)
    p = pred.astype(F32)
    if cfg.layout == 1:
        p = p.transpose(0, 2, 1)
    n, _, A = p.shape
    n_out = n * cfg.max_det if n_out is None else n_out
    hw = np.broadcast_to(np.asarray(frames_hw, np.int64), (n, 2))
    thr, iou_thr, e = F32(cfg.conf_thr), F32(cfg.iou_thr), F32(cfg.extent)
    allowed = np.zeros(cfg.nc, bool)
    allowed[list(cfg.classes)] = True
    rows, image, anchor = [], [], []
    count, flags = np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
    with np.errstate(all='ignore'):
        for img in range(n):
            box, sc = p[img, :4], p[img, 4:]
            best = np.argmax(np.where(np.isnan(sc), -np.inf, sc), axis=0)   # the first of the largest; a NaN never wins
            score = sc[best, np.arange(A)]
            cand = (score > thr) & allowed[best]
            fin = np.isfinite(box).all(axis=0)
            if (cand & ~fin).any():
                flags[img] |= 8
            idx = np.nonzero(cand & fin)[0]
            if len(idx) > MAX_CAND:
                flags[img] |= 1
                idx = idx[:0]
            idx = idx[np.lexsort((idx, -score[idx].astype(np.float64)))]
            half_w, half_h = box[2, idx] * F32(0.5), box[3, idx] * F32(0.5)
            b = np.stack([box[0, idx] - half_w, box[1, idx] - half_h, box[0, idx] + half_w, box[1, idx] + half_h], axis=1)
            cls = best[idx]
            live = np.ones(len(idx), bool)
            picks = []
            for i in range(len(idx)):
                if len(picks) >= cfg.max_det:
                    break
                if not live[i]:
                    continue
                picks.append(i)
                iou = _iou_row(b[i], b[i + 1:], e)
                kill = ~(iou <= iou_thr)
                if not cfg.agnostic:
                    kill &= cls[i + 1:] == cls[i]
                live[i + 1:] &= ~kill
            picks = np.array(picks, np.intp)
            gain, pad_x, pad_y = (F32(v) for v in letterbox_params(hw[img], input_hw))
            side = np.array([hw[img, 1], hw[img, 0], hw[img, 1], hw[img, 0]], F32)
            v = (b[picks] - np.array([pad_x, pad_y, pad_x, pad_y], F32)) / gain
            v = np.where(v < 0, F32(0), v)
            v = np.where(v < side, v, side)
            out = np.concatenate([v, score[idx][picks, None], cls[picks, None].astype(F32)], axis=1).astype(F32).reshape(-1, 6)
            if len(picks) and len(rows) + len(picks) > n_out:
                flags[img] |= 4
            count[img] = len(picks)
            rows += list(out)
            image += [img] * len(picks)
            anchor += list(idx[picks])
    count[n] = len(rows)
    R, I, An = np.empty((n_out, 6), F32), np.full(n_out, -1, np.int32), np.full(n_out, -1, np.int32)
    R[:, :4], R[:, 4], R[:, 5] = np.nan, 0, -1
    k = min(n_out, len(rows))
    if k:
        R[:k], I[:k], An[:k] = np.array(rows[:k], F32), image[:k], anchor[:k]
    return R, I, An, count, flags


# ---------------------------------------------------------------- heads
def empty_head(n_images, nc, A):
    """[n, 4 + nc, A] float32: every score 0, every box a 10-pixel square in the corner"""
    p = np.zeros((n_images, 4 + nc, A), F32)
    p[:, :4] = 10
    return p


def put(p, img, a, box, scores):
    """anchor a of image img: box (cx, cy, w, h), scores {class: score}"""
    p[img, :4, a] = box
    for c, s in scores.items():
        p[img, 4 + c, a] = s


def corners(p, img, a, x1, y1, x2, y2, scores):
    put(p, img, a, ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), scores)


def finish(p, layout, dtype):
    p = p.transpose(0, 2, 1) if layout == 1 else p
    with np.errstate(over='ignore'):
        return np.ascontiguousarray(p.astype(NP[dtype]))


def random_head(seed, n_cand, nc, A, layout=0, dtype='fp16'):
    """one image per entry of n_cand with exactly that many anchors over the threshold (scores in [0.4, 1), background below 0.3); about half of them are
    jittered copies of earlier ones.  In fp16 equal scores are common: the anchor order decides."""
    rng = np.random.default_rng(seed)
    n = len(n_cand)
    p = np.zeros((n, 4 + nc, A), F32)
    p[:, 4:] = rng.uniform(0.0, 0.3, (n, nc, A))
    p[:, 0], p[:, 1] = rng.uniform(40, 600, (n, A)), rng.uniform(40, 600, (n, A))
    p[:, 2], p[:, 3] = rng.uniform(8, 120, (n, A)), rng.uniform(8, 120, (n, A))
    for img, m in enumerate(n_cand):
        idx = rng.choice(A, m, replace=False)
        for k, a in enumerate(idx):
            if k > 0 and rng.random() < 0.5:
                src = idx[rng.integers(0, k)]
                p[img, :4, a] = p[img, :4, src] + rng.normal(0, float(rng.choice([0.5, 3.0, 10.0])), 4)
                p[img, 2:4, a] = np.maximum(p[img, 2:4, a], 1)
            p[img, 4 + rng.integers(0, nc), a] = rng.uniform(0.4, 1.0)
    return finish(p, layout, dtype)


HD, SQ = (1080, 1920), (640, 640)


def _named():
    cases = {}
    for layout in (0, 1):
        for dtype in ('fp16', 'fp32'):
            for nc in (1, 3, 80):
                cases[f'random_l{layout}_{dtype}_nc{nc}'] = (DetectCfg(nc=nc, dtype=dtype, layout=layout), random_head(nc + layout, [40, 25], nc, 257, layout, dtype), HD, SQ, None)
    # a masked class out-scores an allowed one: no candidate (anchor 0); the allowed class alone (anchor 1)
    p = empty_head(1, 3, 5)
    put(p, 0, 0, (100, 100, 40, 40), {0: 0.6, 1: 0.9})
    put(p, 0, 1, (300, 300, 40, 40), {0: 0.8, 1: 0.2})
    put(p, 0, 2, (200, 300, 40, 40), {2: 0.7})
    cases['class_mask'] = (DetectCfg(nc=3, dtype='fp32', classes=[0]), finish(p, 0, 'fp32'), SQ, SQ, None)
    # a tie between classes: the first wins
    p = empty_head(1, 3, 4)
    put(p, 0, 0, (100, 100, 40, 40), {0: 0.75, 2: 0.75})    # class 0: passes
    put(p, 0, 1, (300, 300, 40, 40), {1: 0.75, 2: 0.75})    # class 1: masked
    put(p, 0, 3, (200, 400, 40, 40), {0: 0.5, 1: 0.75, 2: 0.75})   # class 1 again
    for dtype in ('fp16', 'fp32'):
        cases[f'class_tie_{dtype}'] = (DetectCfg(nc=3, dtype=dtype, classes=[0, 2]), finish(p, 0, dtype), SQ, SQ, None)
    # NaN and inf
    nan, inf = float('nan'), float('inf')
    p = empty_head(2, 3, 12)
    put(p, 0, 0, (100, 100, 40, 40), {0: nan, 1: 0.6, 2: nan})          # the NaNs never win: class 1
    put(p, 0, 1, (200, 100, 40, 40), {0: nan, 1: nan, 2: nan})          # no candidate
    put(p, 0, 2, (300, 100, 40, 40), {0: 0.5, 1: inf, 2: 0.9})          # an infinite score sorts first
    put(p, 0, 3, (nan, 100, 40, 40), {0: 0.9})                          # flag 8
    put(p, 0, 4, (400, 100, 40, 40), {0: -inf, 1: -inf, 2: -inf})       # class 0 at -inf: below the threshold
    put(p, 0, 5, (302, 101, 40, 40), {1: 0.8})                          # suppressed by anchor 2
    put(p, 1, 0, (100, 100, inf, 40), {2: 0.9})                         # flag 8 on image 1
    put(p, 1, 1, (100, nan, 40, 40), {2: 0.1})                          # below the threshold: no flag
    put(p, 1, 7, (100, 100, 40, 40), {2: 0.9})
    for layout in (0, 1):
        for dtype in ('fp16', 'fp32'):
            cases[f'nan_inf_l{layout}_{dtype}'] = (DetectCfg(nc=3, dtype=dtype, layout=layout), finish(p, layout, dtype), SQ, SQ, None)
    # finite boxes whose corners overflow (fp32 only): inf corners, a NaN IoU suppresses
    p = empty_head(1, 1, 6)
    put(p, 0, 0, (3e38, 100, 3e38, 40), {0: 0.9})
    put(p, 0, 1, (-3e38, 100, 3e38, 40), {0: 0.85})
    put(p, 0, 2, (0, 100, 3.4e38, 40), {0: 0.8})     # x1 = -1.7e38, x2 = 1.7e38: its width overflows, area inf, IoU with itself-like boxes NaN
    put(p, 0, 3, (1, 101, 3.4e38, 40), {0: 0.7})
    put(p, 0, 4, (100, 100, 40, 40), {0: 0.6})
    cases['corner_overflow'] = (DetectCfg(nc=1, dtype='fp32'), finish(p, 0, 'fp32'), SQ, SQ, None)
    # a score equal to conf_thr is no candidate, the next float is
    t = F32(0.35)
    p = empty_head(1, 2, 4)
    put(p, 0, 0, (100, 100, 40, 40), {0: t})
    put(p, 0, 1, (200, 100, 40, 40), {1: np.nextafter(t, F32(1))})
    put(p, 0, 2, (300, 100, 40, 40), {1: np.nextafter(t, F32(0))})
    cases['score_at_thr'] = (DetectCfg(nc=2, dtype='fp32'), finish(p, 0, 'fp32'), SQ, SQ, None)
    # an IoU exactly equal to iou_thr is kept: b inside a with half its area (8 / 16); c with 10 / 16 is suppressed
    p = empty_head(1, 1, 4)
    corners(p, 0, 0, 100, 100, 104, 104, {0: 0.9})
    corners(p, 0, 1, 100, 100, 104, 102, {0: 0.8})
    corners(p, 0, 2, 100, 100, 104, 102.5, {0: 0.7})
    cases['iou_at_thr'] = (DetectCfg(nc=1, dtype='fp32', iou_thr=0.5), finish(p, 0, 'fp32'), SQ, SQ, None)
    # class-aware against agnostic on one head
    p = empty_head(1, 2, 6)
    corners(p, 0, 0, 100, 100, 200, 200, {0: 0.9})
    corners(p, 0, 1, 102, 101, 201, 203, {1: 0.8})     # another class on top of it
    corners(p, 0, 2, 101, 102, 202, 201, {0: 0.7})     # the same class on top of it
    corners(p, 0, 3, 400, 400, 450, 470, {1: 0.6})
    for ag in (False, True):
        cases[f'agnostic_{int(ag)}'] = (DetectCfg(nc=2, dtype='fp16', agnostic=ag), finish(p, 0, 'fp16'), SQ, SQ, None)
    # max_det cut
    p = empty_head(1, 1, 16)
    for a in range(10):
        corners(p, 0, a, 50 * a, 20, 50 * a + 30, 60, {0: 0.4 + 0.05 * a})
    cases['max_det_cut'] = (DetectCfg(nc=1, dtype='fp32', max_det=3), finish(p, 0, 'fp32'), SQ, SQ, None)
    # n_out cut: the second image's rows are cut (flag 4), the last count holds the true total; the third image has rows behind the cut too
    p = empty_head(3, 1, 8)
    for img in range(3):
        for a in range(3):
            corners(p, img, a, 50 * a, 20, 50 * a + 30, 60, {0: 0.5 + 0.1 * a})
    cases['n_out_cut'] = (DetectCfg(nc=1, dtype='fp32'), finish(p, 0, 'fp32'), SQ, SQ, 4)
    cases['n_out_zero'] = (DetectCfg(nc=1, dtype='fp32'), finish(p, 0, 'fp32'), SQ, SQ, 0)
    # 2049 candidates: flag 1 and zero rows; 2048: processed
    cases['cand_cap'] = (DetectCfg(nc=2, dtype='fp16', max_det=1024), random_head(7, [2049, 2048], 2, 4096), HD, SQ, None)
    # letterbox: 1920 x 1080 into 640 x 640 (gain 1 / 3, pad (0, 140)) and 320 x 320 (gain 1 / 6, pad (0, 70)); boxes over all four frame edges
    for name, inp, s in (('640', (640, 640), 1.0), ('320', (320, 320), 0.5)):
        p = empty_head(1, 1, 8)
        corners(p, 0, 0, -20 * s, 200 * s, 100 * s, 300 * s, {0: 0.9})          # over the left edge
        corners(p, 0, 1, 600 * s, 200 * s, 700 * s, 300 * s, {0: 0.85})         # over the right edge
        corners(p, 0, 2, 300 * s, 100 * s, 400 * s, 200 * s, {0: 0.8})          # into the top pad
        corners(p, 0, 3, 300 * s, 450 * s, 400 * s, 560 * s, {0: 0.75})         # into the bottom pad
        corners(p, 0, 4, 250.25 * s, 260.5 * s, 291.75 * s, 333.25 * s, {0: 0.7})   # inside
        corners(p, 0, 5, 10 * s, 10 * s, 60 * s, 100 * s, {0: 0.65})            # wholly inside the top pad: a zero-height box on the edge
        cases[f'letterbox_{name}'] = (DetectCfg(nc=1, dtype='fp32'), finish(p, 0, 'fp32'), HD, inp, None)
    # an image without candidates between two with some; frames of different sizes
    cases['empty_between'] = (DetectCfg(nc=3, dtype='fp16'), random_head(11, [9, 0, 5], 3, 65), [(1080, 1920), (720, 1280), (480, 640)], SQ, None)
    cases['extent_one'] = (DetectCfg(nc=3, dtype='fp32', extent=1.0, iou_thr=0.45, agnostic=True), random_head(12, [60], 3, 100, 0, 'fp32'), HD, SQ, None)
    return cases


@functools.lru_cache(maxsize=None)
def named_cases():
    return _named()


# the sizes that can break the kernels: (A, candidates per image, nc, layout, dtype).  A in {1, 63, 64, 65, 257, 8400}, candidates in {0, 1, 2, 64, 65, 257, 2048,
# 2049}, images in {1, 3, 64}; 63, 65 and 257 are no multiple of the vector width (8 halves, 4 floats), 64 and 8400 are
SIZES = [(1, [1], 1, 0, 'fp16'), (1, [0, 1, 1], 2, 1, 'fp32'), (63, [2, 0, 1], 3, 0, 'fp16'), (64, [64], 3, 0, 'fp16'), (64, [1, 64, 2], 3, 0, 'fp32'),
         (65, [65, 2, 64], 2, 0, 'fp32'), (65, [65], 2, 1, 'fp16'), (257, [257], 3, 0, 'fp16'), (257, [257, 65, 0], 3, 1, 'fp32'),
         (257, [(7 * i) % 66 for i in range(64)], 3, 0, 'fp16'), (260, [(5 * i) % 65 for i in range(64)], 2, 0, 'fp32'),
         (8400, [0], 80, 0, 'fp16'), (8400, [2048], 80, 0, 'fp16'), (8400, [2049, 257, 2048], 4, 0, 'fp32'), (8400, [65, 2049, 1], 4, 1, 'fp16')]


def size_id(s):
    A, cand, nc, layout, dtype = s
    return f'A{A}_c{max(cand)}_n{len(cand)}_nc{nc}_l{layout}_{dtype}'


@functools.lru_cache(maxsize=None)
def size_case(i):
    A, cand, nc, layout, dtype = SIZES[i]
    cfg = DetectCfg(nc=nc, dtype=dtype, layout=layout, max_det=1024 if max(cand) > 300 else 300)
    return cfg, random_head(100 + i, cand, nc, A, layout, dtype), HD, SQ, None
