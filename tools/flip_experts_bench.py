#!/usr/bin/env python3
"""Flip-test on a mixed-dataset batch of a ViTPose+ handle: one call under the per-dataset mode against the loop over datasets.

  mixed   set_flip_test_datasets once; per call infer_mixed(crops, ids): one encoder pass of 2 n rows, a head per dataset, one decode
  loop    what a caller ran before that mode existed: per dataset present, clear_flip_test + set_dataset + set_flip_test(its pairs) + infer(its crops)
          -- the single-table mode clears itself on a change of K, and a set waits for the handle's enqueued work

Both are the host path (pageable uint8 crops in, keypoints out), six datasets interleaved (crop i -> dataset i % 6), on one handle each in one process.
A block is a fresh process that times both routes at every size (median of --iters calls after --warmup); a figure is the median of the block medians,
its spread (max - min) / median over the blocks.

    python tools/flip_experts_bench.py [--variant b] [--sizes 8,16,64,128] [--blocks 3] [--out profiles/flip_experts.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def pair_tables(datasets, ks):
    """mirror pairs per dataset: COCO-17's where the dataset has 17 joints, else joint 2 i <-> 2 i + 1 (the time does not depend on the table)"""
    from easy_vitpose_amd.configs import COCO17_FLIP_PAIRS
    return {ds: [list(p) for p in COCO17_FLIP_PAIRS] if k == 17 else [[2 * i, 2 * i + 1] for i in range(k // 2)] for ds, k in zip(datasets, ks)}


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def block(args):
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.synth import synthetic_crops, synthetic_moe_state_dict
    sizes = [int(s) for s in args.sizes.split(',')]
    nmax = max(sizes)
    shp = model_shape(args.variant, 'coco')
    sd = synthetic_moe_state_dict(shp, args.part_features, seed=0)
    crops = synthetic_crops(nmax, 3, 'noise')
    mixed = VitPoseHip(shp, sd, dtype=args.dtype, max_batch=2 * nmax)
    loop = VitPoseHip(shp, sd, dtype=args.dtype, max_batch=2 * nmax)
    names = [d for d, _ in mixed.experts]
    pairs = pair_tables(names, [k for _, k in mixed.experts])
    mixed.set_flip_test_datasets(pairs)
    res = {}
    for n in sizes:
        ids = (np.arange(n) % len(names)).astype(np.int32)
        c = crops[:n]
        shares = [(ds, np.ascontiguousarray(c[ids == e])) for e, ds in enumerate(names) if (ids == e).any()]

        def per_dataset():
            out = []
            for ds, share in shares:
                loop.clear_flip_test()
                loop.set_dataset(ds)
                loop.set_flip_test(pairs[ds])
                out.append(loop.infer(share))
            return out

        got = mixed.infer_mixed(c, ids)[0]
        want = per_dataset()
        dconf = max(float(np.abs(got[ids == names.index(ds)][:, :w.shape[1], 2] - w[..., 2]).max()) for (ds, _), w in zip(shares, want))
        assert dconf < 2e-3, f'the two routes disagree: confidence max|diff| {dconf}'   # other batch sizes, other rounding points: not the bits
        res[f'mixed/{n}'] = timed(lambda: mixed.infer_mixed(c, ids), args.warmup, args.iters)
        res[f'loop/{n}'] = timed(per_dataset, args.warmup, args.iters)
    mixed.close()
    loop.close()
    print('BLOCK ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', default='b')
    ap.add_argument('--sizes', default='8,16,64,128')
    ap.add_argument('--part-features', type=int, default=192)
    ap.add_argument('--dtype', default='fp16')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--block', action='store_true', help='(internal) one block in this process')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.block:
        return block(args)
    blocks = []
    for b in range(args.blocks):
        cmd = [sys.executable, os.path.abspath(__file__), '--block', '--variant', args.variant, '--sizes', args.sizes, '--dtype', args.dtype,
               '--part-features', str(args.part_features), '--warmup', str(args.warmup), '--iters', str(args.iters)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith('BLOCK ')]
        if r.returncode or not line:
            raise SystemExit(f'block {b} failed (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
        blocks.append(json.loads(line[0][6:]))
        print(f'# block {b}: {line[0][6:]}', flush=True)

    def stat(key):
        v = np.array([blk[key] for blk in blocks])
        return float(np.median(v)), float((v.max() - v.min()) / np.median(v))

    out = [f'# flip_experts_bench: ViTPose-{args.variant.upper()} ViTPose+ (synthetic, P = {args.part_features}) {args.dtype}, six datasets interleaved (crop i -> dataset i % 6),',
           f'# host path; {args.blocks} blocks, each a fresh process; per block the median of {args.iters} calls after {args.warmup}; ms per call = median of the block medians,',
           '# spread = (max - min) / median over the blocks.  mixed = one infer_mixed call under set_flip_test_datasets; loop = per dataset clear_flip_test +',
           '# set_dataset + set_flip_test + infer on that dataset\'s crops (the only route before the per-dataset mode)',
           f'{"n":>4} {"mixed ms":>9} {"spread":>7} {"loop ms":>9} {"spread":>7} {"mixed / loop":>13}']
    for n in args.sizes.split(','):
        (m, sm), (l, sl) = stat(f'mixed/{n}'), stat(f'loop/{n}')
        out.append(f'{n:>4} {m:>9.3f} {100 * sm:>6.1f}% {l:>9.3f} {100 * sl:>6.1f}% {m / l:>13.3f}')
    print('\n'.join(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    main()
