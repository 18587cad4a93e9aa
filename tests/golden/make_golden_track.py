#!/usr/bin/env python
"""Generate tests/golden/sort_crowd.npz by running THE REFERENCE's tracker (sort.py Sort) on the seeded crowd sequences of tests/track_cases.py.

    python tests/golden/make_golden_track.py

Like make_golden.py it runs only where the reference tree exists and copies nothing from it: the fixture holds the reference's OUTPUT rows
(frame, x1, y1, x2, y2, score, id) per sequence.  The reference runs through make_golden's stubs -- the textbook KalmanFilter in place of the absent filterpy --
and through the scipy path of its linear_assignment (``lap`` is kept from importing), with KalmanBoxTracker.count = 0 per sequence and the float32
iou_threshold the device compares with.

These sequences enter the assignment branch (the four older sort_*.npz never do): the generator counts the calls of the solver and the assigned pairs
that fall under the threshold, and prints them.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), HERE):
    sys.path.insert(0, p)
OUT = os.path.join(HERE, 'sort_crowd.npz')


def main():
    import make_golden
    from track_cases import CROWDS, IOU_THRESHOLD, crowd, run_rows
    if not os.path.isdir(make_golden.REF):
        raise SystemExit(f'{make_golden.REF} not found: the goldens are generated where the reference tree exists')
    make_golden._install_stubs()
    sys.modules['lap'] = None   # the scipy path of linear_assignment
    sys.path.insert(0, make_golden.REF)
    warnings.simplefilter('ignore')
    from easy_ViTPose import sort as ref
    solver = ref.linear_assignment
    stats = {'calls': 0, 'under': 0}

    def counted(cost):
        pairs = solver(cost)
        stats['calls'] += 1
        stats['under'] += int(sum(-cost[a, b] < IOU_THRESHOLD for a, b in pairs))
        return pairs
    ref.linear_assignment = counted
    out = {}
    for seed, P, F, max_age, min_hits, skip in CROWDS:
        frames = crowd(seed, P, F, skip=skip)
        ref.KalmanBoxTracker.count = 0
        trk = ref.Sort(max_age=max_age, min_hits=min_hits, iou_threshold=IOU_THRESHOLD)
        stats['calls'] = stats['under'] = 0
        rows = run_rows(trk.update, frames)
        out[f'crowd{seed}'] = rows
        print(f'crowd seed {seed}: {P} persons, {F} frames, {len(rows)} rows, {stats["calls"]} frames in the assignment branch, '
              f'{stats["under"]} assigned pairs under the threshold, at most {max(len(d) for d in frames)} detections per frame, '
              f'{len(set(rows[:, 6].astype(int)))} ids')
    np.savez_compressed(OUT, **out)
    print(f'{OUT}: {os.path.getsize(OUT)} bytes, numpy {np.__version__}')


if __name__ == '__main__':
    main()
