#!/usr/bin/env python
"""Generate tests/golden/pose_nms.npz by running THE REFERENCE's vit_utils/post_processing/nms.py in the build container.

    python tests/golden/make_golden_pose_nms.py

Like make_golden.py it runs only where the reference tree exists and copies nothing from it: the fixture holds seeded synthetic inputs and the
reference's numerical OUTPUTS (oks_iou matrices, oks_nms / soft_oks_nms keep lists, the score of every soft pick).

Inputs: seeded synthetic people.  About half of the rows are jittered copies of earlier rows of the same frame (keypoint noise of 0.2, 1 or 3 times
6 px, area +-5 %), conf in [0.05, 1], box scores in [0.35, 0.99], rows scattered over 1 to 3 frames.  One input set per (K, n), shared by the four
(oks_thr, vis_thr) combinations.  Keypoints are float32 (y, x, conf) rows -- oks_iou only ever forms dx^2 + dy^2, so the order of the two coordinates
does not matter to it -- scores reach the reference as Python floats (its `scores` array is then float64, as the kernel keeps them) and the sigmas as
the float64 values of the float32 table the library is given.

The generator asserts two conditions ON THE REFERENCE ALONE and moves on to the next seed when one fails (it never drops an element):
  * no pairwise OKS lies within 1e-4 of a threshold in use;
  * at every pick, hard or soft, the top two live scores differ, relative to the larger, by more than twice the soft-score bound
    (2 + 2 / oks_thr) * 2^-23 * picks_before_it (and by more than nothing at all at the first pick and under hard NMS).
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF_NMS = '/root/reference/easy_ViTPose/vit_utils/post_processing/nms.py'
OUT = os.path.join(HERE, 'pose_nms.npz')

from easy_vitpose_amd.posenms import COCO17_SIGMAS  # noqa: E402

CASES = [(17, 1), (17, 2), (17, 7), (17, 33), (17, 70), (133, 7), (133, 33)]
THRS = (0.5, 0.9)
VIS = (0.2, None)
MAX_DETS = 20
EPS = 2.0 ** -23


def import_reference():
    if not os.path.exists(REF_NMS):
        raise SystemExit(f'{REF_NMS} not found: the goldens are generated where the reference tree exists')
    spec = importlib.util.spec_from_file_location('ref_nms', REF_NMS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sigmas_for(K):
    s32 = np.asarray(COCO17_SIGMAS, dtype=np.float32) if K == 17 else np.full(K, 0.05, dtype=np.float32)
    return s32


def make_people(rng, K, n):
    n_frames = int(rng.integers(1, 4))
    kp = np.zeros((n, K, 3), np.float32)
    p9 = np.zeros((n, 9), np.int32)
    bs = rng.uniform(0.35, 0.99, n).astype(np.float32)
    for i in range(n):
        if i > 0 and rng.random() < 0.5:
            src = int(rng.integers(0, i))
            scale = float(rng.choice([0.2, 1.0, 3.0])) * 6.0
            kp[i, :, :2] = kp[src, :, :2] + rng.normal(0.0, scale, (K, 2)).astype(np.float32)
            kp[i, :, 2] = np.clip(kp[src, :, 2] + rng.normal(0.0, 0.1, K), 0.05, 1.0).astype(np.float32)
            p9[i] = p9[src]
            cw = max(1, int(round(p9[src, 3] * rng.uniform(0.95, 1.05))))
            p9[i, 3] = p9[i, 7] = cw
        else:
            f = int(rng.integers(0, n_frames))
            cw, ch = int(rng.integers(60, 220)), int(rng.integers(120, 400))
            x0, y0 = int(rng.integers(0, 1280 - cw)), int(rng.integers(0, 720 - ch))
            kp[i, :, 0] = rng.uniform(y0, y0 + ch, K).astype(np.float32)
            kp[i, :, 1] = rng.uniform(x0, x0 + cw, K).astype(np.float32)
            kp[i, :, 2] = rng.uniform(0.05, 1.0, K).astype(np.float32)
            p9[i] = [f, x0, y0, cw, ch, 0, 0, cw, ch]
    return kp, bs, p9, n_frames


def instance_scores(kp, bs, vis):
    out = np.zeros(len(kp), np.float32)
    for i in range(len(kp)):
        c = kp[i, :, 2]
        sel = c[c > np.float32(vis)] if vis is not None else c
        s = 0.0
        for v in sel:   # fp64, joint order
            s += float(v)
        out[i] = np.float32((s / len(sel) if len(sel) else 0.0) * float(bs[i]))
    return out


class Retry(Exception):
    pass


def gap_ok(top, second, bound):
    if top == second:
        return False
    return abs(top - second) > 2.0 * bound * max(abs(top), abs(second))


def run_case(ref, kp, scores, p9, n_frames, sig64, thr, vis):
    n = len(kp)
    areas = p9[:, 3].astype(np.float64) * p9[:, 4].astype(np.float64)
    flat = kp.reshape(n, -1)
    oks = np.stack([ref.oks_iou(flat[g], flat, areas[g], areas, sig64, vis) for g in range(n)])
    for t in THRS:
        if (np.abs(oks - np.float32(t)) < 1e-4).any():
            raise Retry(f'an OKS within 1e-4 of {t}')
    hard_rank = np.full(n, -1, np.int32)
    soft_rank = np.full(n, -1, np.int32)
    soft_score = np.full(n, np.nan, np.float64)
    min_gap = np.inf
    for f in range(n_frames):
        rows = np.nonzero(p9[:, 0] == f)[0]
        if not len(rows):
            continue
        db = [{'keypoints': kp[i], 'score': float(scores[i]), 'area': float(areas[i])} for i in rows]
        keep = ref.oks_nms(db, thr, sig64, vis)
        # hard: the live scores never change, so a tie anywhere among this frame's rows is what could make argsort's order show
        sc = np.sort(np.array([d['score'] for d in db]))
        if (np.diff(sc) == 0).any():
            raise Retry('equal scores on one frame')
        hard_rank[rows[np.asarray(keep, dtype=np.intp)]] = np.arange(len(keep), dtype=np.int32)
        soft_keep = ref.soft_oks_nms(db, thr, MAX_DETS, sig64, vis)
        # the reference's soft loop once more (nms.py:184-203) with its own oks_iou and _rescore, recording the score of every pick
        s = np.array([d['score'] for d in db])
        k = np.array([d['keypoints'].flatten() for d in db])
        a = np.array([d['area'] for d in db])
        order = s.argsort()[::-1]
        s = s[order]
        mine, cnt = [], 0
        while len(order) > 0 and cnt < MAX_DETS:
            bound = (2.0 + 2.0 / thr) * EPS * cnt
            if len(s) > 1:
                if not gap_ok(s[0], s[1], bound):
                    raise Retry('top two live scores too close')
                min_gap = min(min_gap, abs(s[0] - s[1]) / max(abs(s[0]), abs(s[1])))
            i = order[0]
            soft_score[rows[i]] = s[0]
            ov = ref.oks_iou(k[i], k[order[1:]], a[i], a[order[1:]], sig64, vis)
            order = order[1:]
            s = ref._rescore(ov, s[1:], thr)
            tmp = s.argsort()[::-1]
            order, s = order[tmp], s[tmp]
            mine.append(i)
            cnt += 1
        assert list(mine) == list(soft_keep), 'the replayed soft loop disagrees with soft_oks_nms'
        soft_rank[rows[np.asarray(soft_keep, dtype=np.intp)]] = np.arange(len(soft_keep), dtype=np.int32)
    return oks, hard_rank, soft_rank, soft_score, min_gap


def main():
    ref = import_reference()
    out = {'cases': np.array(CASES, np.int32), 'thrs': np.array(THRS, np.float64), 'vis': np.array([0.2, np.nan], np.float64),
           'max_dets': np.int32(MAX_DETS)}
    min_gap = np.inf
    for K, n in CASES:
        s32 = sigmas_for(K)
        sig64 = s32.astype(np.float64)
        seed = 1000 * K + n
        while True:
            rng = np.random.default_rng(seed)
            kp, bs, p9, n_frames = make_people(rng, K, n)
            try:
                res = {}
                for vi, vis in enumerate(VIS):
                    scores = instance_scores(kp, bs, vis)
                    for ti, thr in enumerate(THRS):
                        res[(ti, vi)] = (scores,) + run_case(ref, kp, scores, p9, n_frames, sig64, thr, vis)
                break
            except Retry as e:
                print(f'K={K} n={n} seed {seed}: {e}; next seed')
                seed += 100000
        tag = f'k{K}_n{n}'
        out[f'{tag}_kpts'], out[f'{tag}_box'], out[f'{tag}_p9'], out[f'{tag}_frames'], out[f'{tag}_sigmas'] = kp, bs, p9, np.int32(n_frames), s32
        out[f'{tag}_seed'] = np.int64(seed)
        for (ti, vi), (scores, oks, hr, sr, ss, g) in res.items():
            min_gap = min(min_gap, g)
            out[f'{tag}_v{vi}_score'] = scores
            out[f'{tag}_v{vi}_oks'] = oks
            out[f'{tag}_t{ti}_v{vi}_hard_rank'], out[f'{tag}_t{ti}_v{vi}_soft_rank'], out[f'{tag}_t{ti}_v{vi}_soft_score'] = hr, sr, ss
        print(f'K={K} n={n}: seed {seed}, {n_frames} frame(s), kept hard/soft at 0.5|vis: '
              f'{(res[(0, 0)][2] >= 0).sum()}/{(res[(0, 0)][3] >= 0).sum()}, at 0.9|vis: {(res[(1, 0)][2] >= 0).sum()}/{(res[(1, 0)][3] >= 0).sum()}')
    np.savez_compressed(OUT, **out)
    print(f'{OUT}: {os.path.getsize(OUT)} bytes, numpy {np.__version__}, smallest relative top-two gap {min_gap:.3e}')


if __name__ == '__main__':
    main()
