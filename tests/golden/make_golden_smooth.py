#!/usr/bin/env python
"""Generate tests/golden/one_euro.npz by running THE REFERENCE's OneEuroFilter (vit_utils/post_processing/one_euro_filter.py) on seeded keypoint sequences.

    python tests/golden/make_golden_smooth.py

Like make_golden.py it runs only where the reference tree exists and copies nothing from it: the fixture holds the inputs (float32), the t_e of every frame,
the reference's OUTPUT rounded to float32 and its final x_prev / dx_prev (float64).  The filter is built with `fps` set: its realtime branch reads the wall clock
and cannot be pinned.  Per sequence `<tag>`: `<tag>_x` [T, K, 2] (frame 0 is the constructor's x0), `<tag>_te` [T] (entry 0 unused), `<tag>_out` [T, K, 2]
(frame 0 = x0 itself), `<tag>_xprev`, `<tag>_dxprev` [K, 2], and `tags`, `fps` for the list of sequences.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.path.join(HERE, 'one_euro.npz')
FRAMES = 40
JOINTS = (17, 133)
FPS = (30.0, 25.0, 59.94)
PATTERNS = {'steady': (1.0,), 'gaps': (1.0, 2.0, 0.5, 3.0)}


def main():
    import make_golden
    path = os.path.join(make_golden.REF, 'easy_ViTPose', 'vit_utils', 'post_processing', 'one_euro_filter.py')
    if not os.path.isfile(path):
        raise SystemExit(f'{path} not found: the goldens are generated where the reference tree exists')
    spec = importlib.util.spec_from_file_location('_ref_one_euro', path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(19)
    out, tags, fps_of, masked, total = {}, [], [], 0, 0
    for K in JOINTS:
        for fps in FPS:
            for name, pattern in PATTERNS.items():
                base = rng.uniform(-3, 400, size=(K, 2))   # some joints start at negative positions
                x = (base[None] + np.cumsum(rng.normal(0, 2.5, size=(FRAMES, K, 2)), 0)).astype(np.float32)
                x[rng.random(x.shape) < 0.03] = 0.0        # missing joints
                te = np.array([pattern[t % len(pattern)] for t in range(FRAMES)], np.float64)
                f = ref.OneEuroFilter(x[0], fps=fps)
                y = np.empty_like(x)
                y[0] = x[0]
                for t in range(1, FRAMES):
                    y[t] = f(x[t], t_e=float(te[t])).astype(np.float32)
                masked += int((x[1:] <= 0).sum())
                total += x[1:].size
                tag = f'k{K}_fps{fps:g}_{name}'.replace('.', 'p')
                tags.append(tag)
                fps_of.append(fps)
                out[tag + '_x'], out[tag + '_te'], out[tag + '_out'] = x, te, y
                out[tag + '_xprev'], out[tag + '_dxprev'] = np.asarray(f.x_prev, np.float64), np.asarray(f.dx_prev, np.float64)
    out['tags'], out['fps'] = np.array(tags), np.array(fps_of, np.float64)
    np.savez_compressed(OUT, **out)
    print(f'{OUT}: {len(tags)} sequences, {total} filtered coordinates, {masked} of them masked, {os.path.getsize(OUT)} bytes, numpy {np.__version__}')


if __name__ == '__main__':
    main()
