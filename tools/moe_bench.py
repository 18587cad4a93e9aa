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

--entries: the per-crop dataset entries (vp_infer_experts_device_stream, vp_infer_boxes_experts_stream) against vp_infer_experts of a BASELINE checkout of
this repository (--baseline-root: a tree of the commit to compare against with its library built) on the same device.  Blocks alternate between the two
trees, each block a fresh process that times every configuration (median of --iters calls after --warmup, host clock around call + synchronisation); a figure
is the median of its block medians and its spread (max - min) / median over the blocks.  Configurations per batch size n, six datasets interleaved:
  mixed_host   infer_mixed (vp_infer_experts: host crops in, host keypoints out)        single_host  infer, one dataset, the same crops
  mixed_dev    infer_mixed_device (device crops in, device keypoints out) + synchronise   single_dev   infer_device, one dataset + synchronise
and per (P persons, F frames) cell of tools/boxes_bench.py, a dataset per box: boxes_host = boxes to the host, infer_frames(datasets=), host offsets;
boxes_dev = infer_boxes(datasets=) + synchronise.

    python tools/moe_bench.py --entries --baseline-root DIR [--blocks 5] [--sizes 8,16,256] [--out profiles/moe_entries.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get('VP_BENCH_ROOT') or HERE   # --entries: the tree a block's process imports the package (and its library) from
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, 'tools'))


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def entries_block(args):
    """one block in this process: a JSON line {config: ms} for the tree on sys.path"""
    import torch
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.synth import synthetic_crops, synthetic_moe_state_dict
    sizes = [int(s) for s in args.sizes.split(',')]
    nmax = max(sizes)
    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_moe_state_dict(shp, args.part_features, seed=0), dtype=args.dtype, max_batch=max(nmax, 256))
    crops = synthetic_crops(nmax, 3, 'noise')
    new = hasattr(eng, 'infer_mixed_device')
    res = {}

    def dev_sync(call):
        def run():
            call()
            eng.synchronize()
            torch.cuda.synchronize()
        return run

    for n in sizes:
        ids = (np.arange(n) % 6).astype(np.int32)
        c = crops[:n]
        d_c = torch.from_numpy(c).cuda()
        res[f'mixed_host/{n}'] = timed(lambda: eng.infer_mixed(c, ids), args.warmup, args.iters)[0]
        res[f'single_host/{n}'] = timed(lambda: eng.infer(c), args.warmup, args.iters)[0]
        d_one = torch.empty((n, eng.K, 3), device='cuda')
        res[f'single_dev/{n}'] = timed(dev_sync(lambda: eng.infer_device(d_c, d_one, sync=False)), args.warmup, args.iters)[0]
        if new:
            d_out = torch.empty((n, eng.Kmax, 3), device='cuda')
            res[f'mixed_dev/{n}'] = timed(dev_sync(lambda: eng.infer_mixed_device(d_c, ids, d_out)), args.warmup, args.iters)[0]
            assert np.array_equal(d_out.cpu().numpy(), eng.infer_mixed(c, ids)[0]), 'the device entry and infer_mixed differ'
    if new and args.persons:
        from easy_vitpose_amd.cropprep import frames_crop_params
        from frames_bench import person_boxes
        H, W = 1080, 1920
        Ps = [int(x) for x in args.persons.split(',')]
        Fs = [int(x) for x in args.frames.split(',')]
        rng = np.random.default_rng(0)
        dev = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(max(Fs))]
        for P in Ps:
            boxes = [person_boxes(np.random.default_rng(1000 * P + i), P, H, W) for i in range(max(Fs))]
            for F in Fs:
                n = P * F
                b6 = np.zeros((n, 6), np.float32)
                b6[:, :5] = np.concatenate(boxes[:F])
                d_boxes = torch.from_numpy(b6).cuda()
                d_fidx = torch.from_numpy(np.repeat(np.arange(F, dtype=np.int32), P)).cuda()
                ids = (np.arange(n) % 6).astype(np.int32)
                ks = eng.dataset_k(ids)
                out = torch.empty((n, eng.Kmax, 3), device='cuda')
                frames = dev[:F]

                def host_route():
                    b, fi = d_boxes.cpu().numpy(), d_fidx.cpu().numpy()
                    p9 = frames_crop_params([b[fi == f, :4].astype(np.float64) for f in range(F)], [tuple(f.shape) for f in frames])
                    kp, _ = eng.infer_frames(frames, p9, datasets=ids)
                    valid = np.arange(eng.Kmax)[None, :] < ks[:, None]
                    kp[:, :, 0] += np.where(valid, (p9[:, 2] - p9[:, 6])[:, None], 0)
                    kp[:, :, 1] += np.where(valid, (p9[:, 1] - p9[:, 5])[:, None], 0)
                    return kp

                want = host_route()
                eng.infer_boxes(frames, d_boxes, d_fidx, out=out, datasets=ids)
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), want), 'the boxes entry and its host route differ'
                res[f'boxes_host/{P}x{F}'] = timed(host_route, 3, args.box_iters)[0]
                res[f'boxes_dev/{P}x{F}'] = timed(dev_sync(lambda: eng.infer_boxes(frames, d_boxes, d_fidx, out=out, datasets=ids)), 3, args.box_iters)[0]
    eng.close()
    print('BLOCK ' + json.dumps(res), flush=True)


def entries(args):
    import subprocess
    trees = [('base', os.path.abspath(args.baseline_root))] if args.baseline_root else []
    trees.append(('new', HERE))
    blocks = {name: [] for name, _ in trees}
    for b in range(args.blocks):
        for name, root in trees:
            env = dict(os.environ, VP_BENCH_ROOT=root)
            cmd = [sys.executable, os.path.abspath(__file__), '--entries-block', '--variant', args.variant, '--sizes', args.sizes, '--dtype', args.dtype,
                   '--part-features', str(args.part_features), '--warmup', str(args.warmup), '--iters', str(args.iters), '--box-iters', str(args.box_iters),
                   '--persons', args.persons, '--frames', args.frames]
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith('BLOCK ')]
            if r.returncode or not line:
                raise SystemExit(f'block {b} of {name} failed (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
            blocks[name].append(json.loads(line[0][6:]))
            print(f'# block {b} {name}: {line[0][6:]}', flush=True)

    def stat(name, key):
        v = np.array([blk[key] for blk in blocks[name]])
        return float(np.median(v)), float((v.max() - v.min()) / np.median(v))

    out = [f'# moe_bench --entries: ViTPose-{args.variant.upper()} P = {args.part_features} {args.dtype}, six datasets interleaved (crop i -> dataset i % 6); {args.blocks} alternating blocks per tree,',
           f'# each a fresh process; per block the median of {args.iters} calls ({args.box_iters} for the boxes cells) after warm-up, host clock around call + synchronisation;',
           '# ms = median of the block medians, spread = (max - min) / median over the blocks.  base = the baseline tree (the parent commit), new = this tree',
           f'{"config":<22} {"tree":<5} {"ms":>9} {"spread":>7}']
    for name, _ in trees:
        for key in blocks[name][0]:
            m, sp = stat(name, key)
            out.append(f'{key:<22} {name:<5} {m:>9.3f} {100 * sp:>6.1f}%')
    out.append('# ratios (a / b; the larger of the two spreads beside it)')

    def ratio(label, a, b):
        (ma, sa), (mb, sb) = stat(*a), stat(*b)
        out.append(f'{label:<58} {ma / mb:>6.3f}   (spread {100 * max(sa, sb):.1f}%)')

    for n in args.sizes.split(','):
        if args.baseline_root:
            ratio(f'n={n}: new mixed_dev / base mixed_host (vp_infer_experts)', ('new', f'mixed_dev/{n}'), ('base', f'mixed_host/{n}'))
            ratio(f'n={n}: new mixed_host / base mixed_host', ('new', f'mixed_host/{n}'), ('base', f'mixed_host/{n}'))
            ratio(f'n={n}: base mixed_host / base single_host', ('base', f'mixed_host/{n}'), ('base', f'single_host/{n}'))
        ratio(f'n={n}: new mixed_host / new single_host', ('new', f'mixed_host/{n}'), ('new', f'single_host/{n}'))
        ratio(f'n={n}: new mixed_dev / new single_dev', ('new', f'mixed_dev/{n}'), ('new', f'single_dev/{n}'))
    for key in blocks['new'][0]:
        if key.startswith('boxes_dev/'):
            ratio(f'{key[10:]} (P x F): boxes_dev / boxes_host', ('new', key), ('new', 'boxes_host/' + key[10:]))
    print('\n'.join(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(out) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', default='b')
    ap.add_argument('--sizes', default='256,8')
    ap.add_argument('--part-features', type=int, default=192)
    ap.add_argument('--dtype', default='fp16')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--mixed-only', action='store_true')
    ap.add_argument('--entries', action='store_true')
    ap.add_argument('--entries-block', action='store_true', help='(internal) one block of --entries in this process')
    ap.add_argument('--baseline-root', default=None)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--persons', default='1,4,16')
    ap.add_argument('--frames', default='1,8,32')
    ap.add_argument('--box-iters', type=int, default=15)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.entries_block:
        return entries_block(args)
    if args.entries:
        if args.sizes == '256,8':
            args.sizes = '8,16,256'
        return entries(args)

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
