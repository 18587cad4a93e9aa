"""Seeded cases of the COCO keypoint evaluator (csrc/cocogeom.h), shared by tests/test_cocoeval_host.py (tap == numpy twin) and tests/test_gpu_cocoeval.py
(device == tap).

A case = dict(cfg=CocoEvalCfg, calls=[inputs of one update, ...]); every call is a dict of the update entry's arguments (optional ones may be None).  Each case is
built to reach one rule of the contract; `margins(case)` measures the margin condition the device comparison rests on (the device's exp() is not the C library's):
the distance of every finite OKS from every threshold, and the distance between two unequal OKS values of one detection that could both be taken."""
from __future__ import annotations

import functools

import numpy as np

from easy_vitpose_amd.devcoco import CocoEvalCfg, OKS_THRS, cocoeval_numpy_oks

F32, I32 = np.float32, np.int32
MARGIN = 1e-9
KEYS = ('kpts', 'score', 'frame', 'rank', 'gt_kpts', 'gt_box', 'gt_area', 'gt_flags', 'gt_frame', 'n_frames')


def sigmas_for(K):
    return 'coco' if K == 17 else tuple(0.03 + 0.01 * (j % 7) for j in range(K))


def _person(rng, K, size=None):
    """a gt: keypoints (y, x, v) inside a box, the box (x, y, w, h), an area"""
    size = float(rng.choice([30.0, 60.0, 120.0, 250.0])) if size is None else size
    x0, y0 = rng.uniform(0, 500, 2)
    w, h = size * rng.uniform(0.5, 1.0), size
    kp = np.zeros((K, 3), F32)
    kp[:, 0] = y0 + rng.uniform(0, 1, K) * h
    kp[:, 1] = x0 + rng.uniform(0, 1, K) * w
    kp[:, 2] = rng.choice(np.array([0, 1, 2], F32), K, p=[0.2, 0.3, 0.5])
    kp[rng.integers(0, K), 2] = 2
    return kp, np.array([x0, y0, w, h], F32), F32(w * h * 0.6)


def _near(rng, kp, box, rel):
    """a detection: the gt's keypoints moved by rel * the box height, a confidence in the third column"""
    d = kp.copy()
    d[:, :2] += (rng.standard_normal((len(kp), 2)) * rel * float(box[3])).astype(F32)
    d[:, 2] = rng.uniform(0.1, 1.0, len(kp)).astype(F32)
    return d


def _call(rng, K, frames, shuffle=True, quantise=0, n_frames=None, stray=0, rank=False):
    """frames = [(n_det, n_gt), ...]: detections near a gt of their image at mixed distances, or anywhere when it has none"""
    kp, sc, fr, gk, gb, ga, gf, gfr = [], [], [], [], [], [], [], []
    for b, (nd, ng) in enumerate(frames):
        mine = []
        for _ in range(ng):
            k, box, area = _person(rng, K)
            mine.append((k, box))
            gk.append(k); gb.append(box); ga.append(area); gfr.append(b)
            gf.append(int(rng.uniform() < 0.15))
        for _ in range(nd):
            if mine and rng.uniform() < 0.8:
                k, box = mine[rng.integers(0, len(mine))]
                kp.append(_near(rng, k, box, float(rng.choice([0.004, 0.02, 0.05, 0.1, 0.3]))))
            else:
                k, box, _ = _person(rng, K)
                kp.append(_near(rng, k, box, 0.0))
            sc.append(rng.uniform(0.05, 1.0))
            fr.append(b)
    n, g = len(kp), len(gk)
    kpts = np.array(kp, F32).reshape(n, K, 3)
    score = np.array(sc, F32)
    if quantise:
        score = (np.round(score * quantise) / quantise).astype(F32)
    frame = np.array(fr, I32)
    if shuffle and n:
        p = rng.permutation(n)
        kpts, score, frame = kpts[p], score[p], frame[p]
    out = dict(kpts=kpts, score=score, frame=frame, rank=None, gt_kpts=np.array(gk, F32).reshape(g, K, 3), gt_box=np.array(gb, F32).reshape(g, 4),
               gt_area=np.array(ga, F32), gt_flags=np.array(gf, I32), gt_frame=np.array(gfr, I32), n_frames=len(frames) if n_frames is None else n_frames)
    if rank and n:
        out['rank'] = (rng.integers(0, 5, n) - 1).astype(I32)
    for _ in range(stray):   # frames outside [0, n_frames)
        if n:
            out['frame'][rng.integers(0, n)] = int(rng.choice([-1, out['n_frames'], out['n_frames'] + 44]))
        if g:
            out['gt_frame'][rng.integers(0, g)] = int(rng.choice([-7, out['n_frames']]))
    return out


def _hand(K, n_frames, dets, gts):
    """dets = [(frame, kpts [K, 3], score)], gts = [(frame, kpts [K, 3], box, area, flags)]"""
    return dict(kpts=np.array([d[1] for d in dets], F32).reshape(len(dets), K, 3), score=np.array([d[2] for d in dets], F32), frame=np.array([d[0] for d in dets], I32),
                rank=None, gt_kpts=np.array([g[1] for g in gts], F32).reshape(len(gts), K, 3), gt_box=np.array([g[2] for g in gts], F32).reshape(len(gts), 4),
                gt_area=np.array([g[3] for g in gts], F32), gt_flags=np.array([g[4] for g in gts], I32), gt_frame=np.array([g[0] for g in gts], I32), n_frames=n_frames)


def _grid(K, x0, y0, w, h, v=2.0):
    """K keypoints whose extent is exactly w x h: the corners first, the rest at the first corner"""
    kp = np.zeros((K, 3), F32)
    kp[:, 0], kp[:, 1], kp[:, 2] = y0, x0, v
    kp[1 % K, 1] = F32(x0) + F32(w)
    kp[2 % K, 0] = F32(y0) + F32(h)
    return kp


def _shift(kp, dx):
    d = kp.copy()
    d[:, 1] += F32(dx)
    return d


def _rules():
    """one image per matching rule, K = 4, sigma 0.05: oks = exp(-dx^2 / (2 * 0.01 * area)) for a detection shifted by dx as a whole"""
    K = 4
    A = F32(5000.0)                     # medium
    s = lambda oks: float(np.sqrt(-np.log(oks) * 2 * 0.01 * 5000.0))
    base = _grid(K, 100, 100, 60, 80)
    box = np.array([100, 100, 60, 80], F32)
    dets, gts = [], []
    # 0: a crowd gt matched by two detections, both ignored
    gts += [(0, base, box, A, 1)]
    dets += [(0, _shift(base, s(0.87)), 0.9), (0, _shift(base, s(0.77)), 0.8), (0, _shift(base, 500), 0.7)]
    # 1: a gt without a labelled joint (the box branch): one detection inside the doubled box (oks exactly 1), one outside it
    nolab = base.copy(); nolab[:, 2] = 0
    gts += [(1, nolab, box, A, 0)]
    dets += [(1, _shift(base, 30), 0.9), (1, _shift(base, 300), 0.8)]
    # 2: the stop rule: a not-ignored gt at 0.72, behind it an ignored crowd at 0.93: the walk stops at the crowd
    far = _grid(K, 100 + s(0.72) + s(0.93), 100, 60, 80)
    gts += [(2, far, box, A, 1), (2, base, box, A, 0)]          # the crowd comes first in call order
    dets += [(2, _shift(base, s(0.72)), 0.9)]
    # 3: a not-ignored gt that out-scores an earlier ignored one, and an ignored one that is all the detection reaches
    gts += [(3, base, box, A, 1), (3, _shift(base, s(0.62) + s(0.88)), box, A, 0)]
    dets += [(3, _shift(base, s(0.62)), 0.9), (3, _shift(base, -s(0.77)), 0.5)]
    # 4: detections identical to a gt (oks exactly 1.0) and a duplicated gt: COCOeval's `<` hands a tie to the LATER gt of the walk
    gts += [(4, base, box, A, 0), (4, base, box, A, 0), (4, _shift(base, 400), box, F32(20000.0), 0)]
    dets += [(4, base, 0.9), (4, base, 0.8), (4, base, 0.7), (4, _shift(base, 400), 0.6)]
    # 5: a gt ignored in one range only (large), its detection inherits the flag there
    gts += [(5, base, box, F32(9216.0), 0), (5, _shift(base, 300), box, np.nextafter(F32(9216.0), F32(1e9)), 0)]
    dets += [(5, _shift(base, s(0.81)), 0.9), (5, _shift(base, 300 + s(0.66)), 0.8)]
    return dict(cfg=CocoEvalCfg(K, 64, (0.05,) * K), calls=[_hand(K, 6, dets, gts)])


def _areas():
    """gt and detection areas exactly at 32^2 and 96^2 and one float32 step either side; the detections of frame 1 have no gt (their own area decides)"""
    K = 3
    dets, gts = [], []
    box = np.array([10, 10, 32, 32], F32)
    x = 0.0
    for edge in (32.0, 96.0):
        a = F32(edge * edge)
        for area in (np.nextafter(a, F32(0)), a, np.nextafter(a, F32(1e9))):
            kp = _grid(K, 10 + x, 10, 20, 20)
            gts.append((0, kp, box, area, 0))
            dets.append((0, kp, 0.9 - x / 1e4))
            x += 200.0
        for w in (np.nextafter(F32(edge), F32(0)), F32(edge), np.nextafter(F32(edge), F32(1e9))):
            dets.append((1, _grid(K, 0, 0, w, edge), 0.5))   # x from 0: x0 + w is exact
    return dict(cfg=CocoEvalCfg(K, 64, (0.05,) * K), calls=[_hand(K, 2, dets, gts)])


def _nonfinite():
    rng = np.random.default_rng(77)
    K = 17
    c = _call(rng, K, [(6, 3), (5, 4), (4, 2)], shuffle=False)
    c['kpts'][0, 3, 1] = np.nan
    c['kpts'][1, 0, 0] = np.nan        # the first joint: the area is NaN as well
    c['kpts'][7, 5, 0] = np.inf
    c['kpts'][8, 2, 1] = -np.inf
    c['gt_kpts'][1, 4, 0] = np.nan
    c['gt_kpts'][3, 0, 2] = np.nan     # a NaN v is not labelled
    c['gt_area'][5] = np.nan
    c['gt_area'][6] = -3.0
    c['gt_area'][7] = 0.0
    c['score'][2] = np.nan
    c['score'][9] = np.inf
    c['score'][10] = -np.inf
    return dict(cfg=CocoEvalCfg(K, 64), calls=[c])


def _totals(total, K=2, per_call=256 * 20, max_records=None, seed=5):
    """`total` records through calls of at most 256 images x 20 detections, one gt per image"""
    rng = np.random.default_rng(seed + total)
    calls, left = [], total
    while True:
        take = min(left, per_call)
        frames = [(20, 1)] * (take // 20) + ([(take % 20, 1)] if take % 20 else [])
        calls.append(_call(rng, K, frames or [(0, 1)], quantise=64))
        left -= take
        if left <= 0:
            break
    return dict(cfg=CocoEvalCfg(K, max(1, total + 3) if max_records is None else max_records, sigmas_for(K)), calls=calls)


@functools.lru_cache(maxsize=None)
def host_cases() -> dict:
    rng = np.random.default_rng(2024)
    cs = {}
    # detections per image 0, 1, 19, 20, 21, 65 against gts 1, 0, 2, 64, 128, 129 (the last overflows), equal scores across the cut at 20, a NaN score
    c = _call(rng, 17, [(0, 1), (1, 0), (19, 2), (20, 64), (21, 128), (65, 129), (0, 0)], quantise=8)
    c['score'][np.flatnonzero(c['frame'] == 5)[3]] = np.nan
    cs['dets_and_gts_per_image'] = dict(cfg=CocoEvalCfg(17, 256), calls=[c])
    cs['dets_1024'] = dict(cfg=CocoEvalCfg(17, 32), calls=[_call(rng, 17, [(1024, 3)], quantise=16)])
    for K in (1, 133, 256):
        cs[f'K{K}'] = dict(cfg=CocoEvalCfg(K, 64, sigmas_for(K)), calls=[_call(rng, K, [(5, 3), (3, 2)])])
    kinds = [(0, 0), (0, 2), (2, 0), (3, 2)]
    cs['frames_256'] = dict(cfg=CocoEvalCfg(17, 1024), calls=[_call(rng, 17, [kinds[i] for i in rng.integers(0, 4, 256)], stray=9, rank=True)])
    cs['null_optionals'] = dict(cfg=CocoEvalCfg(17, 64), calls=[dict(_call(rng, 17, [(7, 3)]), frame=None, gt_frame=None, gt_flags=None)])
    cs['no_rows'] = dict(cfg=CocoEvalCfg(17, 8), calls=[dict(_call(rng, 17, [(0, 2)]), kpts=None, score=None, frame=None)])
    cs['no_gts'] = dict(cfg=CocoEvalCfg(17, 8), calls=[dict(_call(rng, 17, [(3, 0)]), gt_kpts=None, gt_box=None, gt_area=None, gt_flags=None, gt_frame=None)])
    cs['rules'] = _rules()
    cs['areas'] = _areas()
    cs['nonfinite'] = _nonfinite()
    cs['calls_1_63_64_65'] = dict(cfg=CocoEvalCfg(17, 512), calls=[_call(rng, 17, [(int(rng.integers(0, 3)), int(rng.integers(0, 3))) for _ in range(f)])
                                                                   for f in (1, 63, 64, 65)])
    for total in (0, 1, 2, 63, 64, 65, 1025, 4097, 65537):
        cs[f'total_{total}'] = _totals(total)
    eq = _call(rng, 17, [(3, 2)] * 70)
    eq['score'][:] = 0.5
    cs['all_equal_scores'] = dict(cfg=CocoEvalCfg(17, 512), calls=[eq, dict(eq)])
    cs['one_short'] = _totals(65, K=17, max_records=64)
    return cs


def inputs(call) -> dict:
    return {k: call[k] for k in KEYS}


def margins(case):
    """(the least distance of a finite OKS from a threshold, the least distance between two unequal OKS values >= 0.5 - MARGIN of one detection)"""
    thr_gap, pair_gap = np.inf, np.inf
    for call in case['calls']:
        for m in cocoeval_numpy_oks(case['cfg'], **inputs(call)):
            v = m[np.isfinite(m)]
            if v.size:
                thr_gap = min(thr_gap, float(np.abs(v[:, None] - OKS_THRS[None, :]).min()))
            for row in m:
                r = np.unique(row[np.isfinite(row) & (row >= 0.5 - MARGIN)])
                if r.size > 1:
                    pair_gap = min(pair_gap, float(np.diff(r).min()))
    return thr_gap, pair_gap
