"""Timing figures of the simple decoder's head (csrc/simplehead.hip); writes profiles/simple_head.txt.

    python tools/simple_head_bench.py [--out profiles/simple_head.txt] [--reps 20] [--skip-h]

Part 1: the head alone.  A simple-decoder handle and a classic handle of the same backbone run the same crops with the head's kernel families timed by the
library's own per-launch events (vp_set_profiling: gemm_final = the simple head's one launch; gemm_deconv + gemm_final = the classic head's two or three): ViTPose-B
(K = 17) at 1, 8, 64 and 256 crops, ViTPose-H (K = 133) at 128.  Beside them the same simple-decoder weights through PyTorch on the same GPU, eager fp16:
F.interpolate(F.relu(x), scale_factor=4, mode='bilinear', align_corners=False) + F.conv2d(padding=1), between two device events.  Every figure is the median of
--reps timed calls after 3 warm-up calls, with its spread (max - min) / median.  Every cell where PyTorch's route is faster is named; nothing is promised.
Part 2: the whole step (device crops in, keypoints out, host clock around a synchronous call, profiling off) of the two ViTPose-B handles at 256 crops, alternating."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from easy_vitpose_amd import VitPoseHip  # noqa: E402
from easy_vitpose_amd.configs import model_shape  # noqa: E402
from easy_vitpose_amd.synth import synthetic_crops, synthetic_state_dict  # noqa: E402


def med(v):
    m = float(np.median(v))
    return m, (max(v) - min(v)) / m


def head_ms(eng, crops, families, reps):
    eng.set_profiling(families)
    for _ in range(3):
        eng.infer(crops)
    out = []
    for _ in range(reps):
        eng.reset_profile()
        eng.infer(crops)
        p = eng.profile()
        out.append(sum(p[f]['ms'] for f in families))
    eng.set_profiling(False)
    return med(out)


def torch_ms(sd, n, D, reps):
    w = torch.from_numpy(sd['keypoint_head.final_layer.weight']).cuda().half()
    b = torch.from_numpy(sd['keypoint_head.final_layer.bias']).cuda().half()
    x = torch.randn((n, D, 16, 12), device='cuda').half()
    fn = lambda: F.conv2d(F.interpolate(F.relu(x), scale_factor=4, mode='bilinear', align_corners=False), w, b, padding=1)   # noqa: E731
    with torch.no_grad():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(e))
    return med(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'simple_head.txt'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--skip-h', action='store_true')
    args = ap.parse_args()
    lines = ['# the simple decoder head on the device: tools/simple_head_bench.py on ' + torch.cuda.get_device_name(0), '',
             f'## the head alone, fp16, ms (median of {args.reps} calls after 3 warm-up calls; spread = (max - min) / median)',
             f'{"model":<6} {"K":>4} {"crops":>5} {"simple ms":>10} {"spread":>7} {"GF/s":>8} {"torch eager ms":>15} {"spread":>7} {"classic ms":>11} {"spread":>7} {"simple / torch":>15}']
    losses = []
    step = None
    plan = [('b', 'coco', (1, 8, 64, 256))] + ([] if args.skip_h else [('h', 'wholebody', (128,))])
    for variant, dataset, batches in plan:
        shp_c, shp_s = model_shape(variant, dataset), model_shape(variant, dataset, head='simple')
        sd_s = synthetic_state_dict(shp_s, 0, head='simple')
        sd_c = synthetic_state_dict(shp_c, 0)
        nmax = max(batches)
        crops = synthetic_crops(nmax, 3, 'noise')
        es = VitPoseHip(shp_s, sd_s, dtype='fp16', max_batch=nmax)
        ec = VitPoseHip(shp_c, sd_c, dtype='fp16', max_batch=nmax)
        del sd_c
        for n in batches:
            ts, ss = head_ms(es, crops[:n], ['gemm_final'], args.reps)
            tc, sc = head_ms(ec, crops[:n], ['gemm_deconv', 'gemm_final'], args.reps)
            tt, st = torch_ms(sd_s, n, shp_s.embed_dim, args.reps)
            gf = (2.0 * 192 * 9 * shp_s.num_keypoints * shp_s.embed_dim + 72.0 * shp_s.num_keypoints * 3072) * n / ts / 1e6
            lines.append(f'{variant:<6} {shp_s.num_keypoints:>4} {n:>5} {ts:>10.4f} {ss:>7.1%} {gf:>8.0f} {tt:>15.4f} {st:>7.1%} {tc:>11.4f} {sc:>7.1%} {ts / tt:>15.2f}')
            print(lines[-1], flush=True)
            if not ts <= tt:
                losses.append(f'{variant} x {n}')
        if variant == 'b':
            d_crops = torch.from_numpy(crops[:256]).cuda()
            d_out = torch.empty((256, 17, 3), dtype=torch.float32, device='cuda')
            ms = {'simple': [], 'classic': []}
            for name, e in (('simple', es), ('classic', ec)):
                for _ in range(3):
                    e.infer_device(d_crops, d_out)
            for _ in range(args.reps):
                for name, e in (('simple', es), ('classic', ec)):   # alternating
                    t0 = time.perf_counter()
                    e.infer_device(d_crops, d_out)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            step = {k: med(v) for k, v in ms.items()}
        es.close()
        ec.close()
    lines += ['', 'cells where the PyTorch route is faster than this kernel: ' + (', '.join(losses) if losses else 'none')]
    if step:
        lines += ['', f'## the whole step, ViTPose-B fp16, 256 device crops -> keypoints, synchronous call on the host clock, alternating, {args.reps} each',
                  f'simple decoder   {step["simple"][0]:.3f} ms (spread {step["simple"][1]:.1%})',
                  f'classic decoder  {step["classic"][0]:.3f} ms (spread {step["classic"][1]:.1%})']
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
