#!/usr/bin/env python
"""Generate tests/golden/detect_nms.npz by running THE REFERENCE's box NMS (vit_utils/post_processing/nms.py `nms`) in the build container.

    python tests/golden/make_golden_detect.py

Like make_golden_pose_nms.py it runs only where the reference tree exists and copies nothing from it: the fixture holds seeded synthetic float32 boxes and the
reference's keep lists.

Inputs: n in {1, 2, 7, 33, 70, 300} float32 rows (x1, y1, x2, y2, score); about half of the rows are jittered copies of earlier rows.  Every coordinate lies on
a quarter-pixel lattice in [0, 1024), so cx = (x1 + x2) / 2 and w = x2 - x1 are exact in float32 and cx -+ w / 2 returns the corners bit for bit: the same rows
pass through the detector stage's real head format.  One input set per n, shared by the thresholds 0.3, 0.5, 0.7.

The generator asserts ON THE REFERENCE ALONE that the scores are pairwise distinct and moves to the next seed otherwise (the reference's order among equal scores
is an artefact of its argsort); it never drops a row.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_NMS = '/root/reference/easy_ViTPose/vit_utils/post_processing/nms.py'
OUT = os.path.join(HERE, 'detect_nms.npz')
SIZES = (1, 2, 7, 33, 70, 300)
THRS = (0.3, 0.5, 0.7)


def import_reference():
    if not os.path.exists(REF_NMS):
        raise SystemExit(f'{REF_NMS} not found: the goldens are generated where the reference tree exists')
    spec = importlib.util.spec_from_file_location('ref_nms', REF_NMS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def lattice(v):
    return np.clip(np.round(np.asarray(v, np.float64) * 4) / 4, 0, 1023.75)


def make_boxes(rng, n):
    d = np.zeros((n, 5), np.float64)
    for i in range(n):
        if i > 0 and rng.random() < 0.5:
            src = d[int(rng.integers(0, i))]
            jit = rng.normal(0.0, float(rng.choice([1.0, 6.0, 20.0])), 4)
            x1, y1, x2, y2 = src[:4] + jit
        else:
            w, h = rng.uniform(20, 300), rng.uniform(20, 400)
            x1, y1 = rng.uniform(0, 1023 - w), rng.uniform(0, 1023 - h)
            x2, y2 = x1 + w, y1 + h
        x1, y1, x2, y2 = lattice([x1, y1, x2, y2])
        if x2 < x1 + 1:
            x2 = min(x1 + 1, 1023.75)
        if y2 < y1 + 1:
            y2 = min(y1 + 1, 1023.75)
        d[i] = [x1, y1, x2, y2, rng.uniform(0.36, 0.99)]
    return d.astype(np.float32)


def main():
    ref = import_reference()
    out = {'sizes': np.array(SIZES, np.int32), 'thrs': np.array(THRS, np.float64)}
    for n in SIZES:
        seed = 7000 + n
        while True:
            dets = make_boxes(np.random.default_rng(seed), n)
            if len(np.unique(dets[:, 4])) == n:
                break
            print(f'n={n} seed {seed}: equal scores; next seed')
            seed += 100000
        out[f'n{n}_dets'], out[f'n{n}_seed'] = dets, np.int64(seed)
        for ti, thr in enumerate(THRS):
            keep = np.asarray(ref.nms(dets, thr), np.int32)
            out[f'n{n}_t{ti}_keep'] = keep
            print(f'n={n} thr={thr}: seed {seed}, kept {len(keep)}')
    np.savez_compressed(OUT, **out)
    print(f'{OUT}: {os.path.getsize(OUT)} bytes, numpy {np.__version__}')


if __name__ == '__main__':
    main()
