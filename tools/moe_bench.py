#!/usr/bin/env python3
"""ViTPose+ on the product library: one call of n crops through

  plain     a plain coco handle (the checkpoint model_split.py writes for coco),
  single    a ViTPose+ handle running one dataset (vp_set_expert: coco),
  mixed     a ViTPose+ handle running all six datasets in one call (vp_infer_experts, crop i -> dataset i % 6),
  split6    six split handles back to back, each on its share of the same crops (what a caller without expert handles runs).

Every configuration is the host path (crops in host memory, keypoints back to host), timed as the median wall clock of --iters calls after
--warmup; split-K and every rule at their defaults.  One JSON line per (variant, n, configuration).

    python tools/moe_bench.py [--variant b] [--sizes 256,8] [--iters 20]
    python tools/moe_bench.py --mixed-only --sizes 256 --iters 5     # the mixed step alone (rocprofv3 --kernel-trace --stats)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', default='b')
    ap.add_argument('--sizes', default='256,8')
    ap.add_argument('--part-features', type=int, default=192)
    ap.add_argument('--dtype', default='fp16')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--mixed-only', action='store_true')
    args = ap.parse_args()

    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.moe import DATASETS, split_vitpose_plus
    from easy_vitpose_amd.synth import synthetic_crops, synthetic_moe_state_dict

    sizes = [int(s) for s in args.sizes.split(',')]
    nmax = max(sizes)
    shp = model_shape(args.variant, 'coco')
    sd = synthetic_moe_state_dict(shp, args.part_features, seed=0)
    crops = synthetic_crops(nmax, 3, 'noise')
    plus = VitPoseHip(shp, sd, dtype=args.dtype, max_batch=nmax)

    def report(n, name, ms):
        print(json.dumps(dict(variant=args.variant, P=args.part_features, dtype=args.dtype, n=n, config=name,
                              ms_median=round(ms[0], 3), ms_min=round(ms[1], 3), crops_per_s=round(n / ms[0] * 1e3, 1))), flush=True)

    res = {}
    for n in sizes:
        ids = (np.arange(n) % 6).astype(np.int32)
        c = crops[:n]
        res[(n, 'mixed')] = timed(lambda: plus.infer_mixed(c, ids), args.warmup, args.iters)
        report(n, 'mixed', res[(n, 'mixed')])
        if args.mixed_only:
            continue
        plus.set_dataset('coco')
        res[(n, 'single')] = timed(lambda: plus.infer(c), args.warmup, args.iters)
        report(n, 'single', res[(n, 'single')])
    plus.close()
    if args.mixed_only:
        return
    plain = VitPoseHip(shp, split_vitpose_plus(sd, 'coco'), dtype=args.dtype, max_batch=nmax)
    for n in sizes:
        res[(n, 'plain')] = timed(lambda: plain.infer(crops[:n]), args.warmup, args.iters)
        report(n, 'plain', res[(n, 'plain')])
    plain.close()
    splits = [VitPoseHip(model_shape(args.variant, ds), split_vitpose_plus(sd, ds), dtype=args.dtype, max_batch=nmax) for ds in DATASETS]
    for n in sizes:
        shares = [crops[:n][np.arange(n) % 6 == e] for e in range(6)]

        def six():
            for h, s in zip(splits, shares):
                if len(s):
                    h.infer(s)
        res[(n, 'split6')] = timed(six, args.warmup, args.iters)
        report(n, 'split6', res[(n, 'split6')])
    for h in splits:
        h.close()
    for n in sizes:
        p, s, m, x = (res[(n, k)][0] for k in ('plain', 'single', 'mixed', 'split6'))
        print(f'# ViTPose-{args.variant.upper()} {n} crops: single / plain {s / p:.3f}, mixed / single {m / s:.3f}, split6 / mixed {x / m:.3f}', flush=True)


if __name__ == '__main__':
    main()
