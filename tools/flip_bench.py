#!/usr/bin/env python3
"""Flip-test as a handle mode (vp_set_flip_test) against the two-pass vp_infer_flip and against the plain forward.

Per model (ViTPose-B / coco and ViTPose-L / coco_25, fp16) and per n = 1 ... 256 crops, on one device, in one process:

    (a) plain n    infer of n crops, mode off
    (b) plain 2n   infer of 2 n crops, mode off: the forward the mode runs, without the mirror gather and with the plain decode
    (c) two-pass   infer_flip of n crops: two forwards of n, two device copies of the heatmaps and a merge pass (not under the mode)
    (d) mode n     infer of n crops with the mode on: one forward of 2 n rows and the fused merge + decode
    (e) device n   the device-resident, stream-ordered entry (infer_device on torch's current stream) with the mode on

(a) - (d) are host calls: pageable uint8 crops up, keypoints down, a host clock around the synchronised call.  (e) is timed the same way around
the call + synchronize.  Two handles share the weights' seed, one that never has the mode set ((a) - (c)) and one with it on ((d), (e)), so no
timed call pays a graph capture.  Every path is warmed up (3 calls: first sighting, capture, replay), then `--blocks` blocks are timed with the
paths alternating inside each block; a block's figure is the median of its calls, the table shows the median over blocks and, for (c), the
block-to-block spread (max - min) that the two conditions are judged against:  (d) <= (c) beyond that spread, and the excess of (d) over (b).

    python tools/flip_bench.py [--models b:coco,l:coco_25] [--n 1,2,4,...] [--blocks 5] [--out profiles/flip_mode.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/flip_bench.py --models b:coco --n 8 --blocks 2 --only b,d     # who owns an excess
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COCO_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
PAIRS = {'coco': COCO_PAIRS, 'coco_25': COCO_PAIRS + [[17, 18], [19, 22], [20, 23], [21, 24]]}   # body pairs + feet: timing does not depend on the table


def sclk_note() -> str:
    try:
        o = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=20).stdout
        lines = [l.strip() for l in o.splitlines() if 'sclk' in l and 'GPU[0]' in l]
        return lines[0] if lines else 'sclk: not reported'
    except Exception as e:   # the tool goes on without the note
        return f'sclk: not read ({type(e).__name__})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='b:coco,l:coco_25')
    ap.add_argument('--n', default='1,2,4,8,16,32,64,128,256')
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.12, help='seconds of calls per path and block (at least 3 calls)')
    ap.add_argument('--only', default='a,b,c,d,e')
    ap.add_argument('--dtype', default='fp16')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), 'flip_bench needs a GPU: there is nothing to time without one'
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.synth import synthetic_crops, synthetic_state_dict

    ns = [int(v) for v in args.n.split(',')]
    only = args.only.split(',')
    max_batch = 2 * max(ns)
    pool = synthetic_crops(2 * max(ns), 5, 'blobs')
    lines = [f'# tools/flip_bench.py --models {args.models} --n {args.n} --blocks {args.blocks} --dtype {args.dtype}',
             f'# device: {torch.cuda.get_device_name(0)}; before: {sclk_note()}',
             '# ms per call: median over blocks of the per-block median; spread = max - min over blocks; max_batch = ' + str(max_batch),
             '# (a) plain n  (b) plain 2n  (c) two-pass infer_flip n  (d) mode n  (e) mode n, device-resident stream-ordered entry']

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for spec in args.models.split(','):
        variant, dataset = spec.split(':')
        shp = model_shape(variant, dataset)
        sd = synthetic_state_dict(shp, 0)
        plain = VitPoseHip(shp, sd, dtype=args.dtype, max_batch=max_batch)
        mode = VitPoseHip(shp, sd, dtype=args.dtype, max_batch=max_batch)
        mode.set_flip_test(PAIRS[dataset])
        del sd
        say(f'\n## ViTPose-{variant.upper()} / {dataset} {args.dtype}')
        say(f'{"n":>4} | {"(a) plain n":>11} {"(b) plain 2n":>12} {"(c) two-pass":>12} {"spread(c)":>9} {"(d) mode n":>11} {"spread(d)":>9} {"(e) device":>10} |'
            f' {"(d)/(c)":>7} {"(d)-(c)":>8} {"(d)-(b)":>8} {"spread(b)":>9} {"(d)/(a)":>7}')
        for n in ns:
            crops, crops2 = pool[:n], pool[:2 * n]
            d_crops = torch.from_numpy(crops).cuda()
            d_out = torch.empty((n, shp.num_keypoints, 3), device='cuda')

            def dev_call():
                mode.infer_device(d_crops, d_out, sync=True)

            paths = {'a': lambda: plain.infer(crops), 'b': lambda: plain.infer(crops2), 'c': lambda: plain.infer_flip(crops, PAIRS[dataset]),
                     'd': lambda: mode.infer(crops), 'e': dev_call}
            paths = {k: f for k, f in paths.items() if k in only}
            reps = {}
            for k, f in paths.items():          # warm-up, then the call count of a window from one more timed call
                for _ in range(3):
                    f()
                t0 = time.perf_counter()
                f()
                reps[k] = int(min(60, max(3, args.window / max(time.perf_counter() - t0, 1e-6))))
            per_block = {k: [] for k in paths}
            for _ in range(args.blocks):
                for k, f in paths.items():      # the paths alternate inside a block: drift hits them alike
                    ts = []
                    for _ in range(reps[k]):
                        t0 = time.perf_counter()
                        f()
                        ts.append(time.perf_counter() - t0)
                    per_block[k].append(float(np.median(ts)) * 1e3)
            med = {k: float(np.median(v)) for k, v in per_block.items()}
            spr = {k: float(max(v) - min(v)) for k, v in per_block.items()}
            g = lambda d, k: d.get(k, float('nan'))
            say(f'{n:4d} | {g(med, "a"):11.3f} {g(med, "b"):12.3f} {g(med, "c"):12.3f} {g(spr, "c"):9.3f} {g(med, "d"):11.3f} {g(spr, "d"):9.3f} {g(med, "e"):10.3f} |'
                f' {g(med, "d") / g(med, "c"):7.3f} {g(med, "d") - g(med, "c"):8.3f} {g(med, "d") - g(med, "b"):8.3f} {g(spr, "b"):9.3f} {g(med, "d") / g(med, "a"):7.3f}')
        plain.close()
        mode.close()
    lines.append(f'\n# after: {sclk_note()}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
