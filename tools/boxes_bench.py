#!/usr/bin/env python3
"""Device boxes to frame keypoints: the stream-ordered boxes entry (vp_infer_boxes_stream) against today's best device route.

Workload: ViTPose-B / coco, fp16, seeded 1920x1080 frames in device memory with P persons each (boxes on a jittered grid, as
tools/frames_bench.py), F frames per call; the detector's boxes are a float32 CUDA tensor [n, 6] with an int32 CUDA frame index.

    (a) host route   boxes .cpu() (a synchronisation), cropprep.frames_crop_params on the host, VitPoseHip.infer_frames on the device
                     frames (synchronises torch's stream, uploads the crop rows, downloads the keypoints), the frame offsets added on the host
    (b) infer_boxes  one VitPoseHip.infer_boxes call: geometry, crops, model, decode and offsets on the device, enqueued on torch's stream

Per cell: ms = host clock around one call followed by a device synchronisation (the keypoints complete: on the host for (a), on the device for
(b)), median of --reps calls after --warmup calls; kP/s = thousands of persons per second at that rate; host ms = host time spent inside the
call itself before that synchronisation (all of it for (a)).  Both routes' keypoints are checked to be bit-identical first.

    python tools/boxes_bench.py [--persons 1,4,16] [--frames 1,8,32] [--reps 15] [--max-batch 256] [--out FILE]

--crop affine: the pad route of infer_boxes against infer_boxes(crop='affine') (vp_infer_boxes_affine_stream) instead, INTERLEAVED -- rounds of one pad call and
one affine call, each followed by a device synchronisation -- so that both see the same clocks.  Per cell: median and the 10th .. 90th percentile of each route's
calls, and the im2col family of the handle's profile (box kernel + crop kernel + patch gather, the only launches that differ) from one profiled call per route.

    python tools/boxes_bench.py --crop affine --persons 1,8,64,256 --frames 1 --reps 40 --out profiles/affine_crop.txt
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from frames_bench import person_boxes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--persons', default='1,4,16')
    ap.add_argument('--frames', default='1,8,32')
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--dtype', default='fp16')
    ap.add_argument('--max-batch', type=int, default=256)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--out', default=None)
    ap.add_argument('--crop', default='pad', choices=['pad', 'affine'], help="affine: the pad route against crop='affine', interleaved")
    args = ap.parse_args()

    import torch
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.cropprep import frames_crop_params
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.synth import synthetic_state_dict

    Ps = [int(x) for x in args.persons.split(',')]
    Fs = [int(x) for x in args.frames.split(',')]
    H, W = args.height, args.width
    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=args.dtype, max_batch=args.max_batch)
    rng = np.random.default_rng(0)
    nF = max(Fs)
    dev = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(nF)]
    torch.cuda.synchronize()

    def route_a(frames, d_boxes, d_fidx):
        b = d_boxes.cpu().numpy()
        fi = d_fidx.cpu().numpy()
        p9 = frames_crop_params([b[fi == f, :4].astype(np.float64) for f in range(len(frames))], [tuple(f.shape) for f in frames])
        kp = eng.infer_frames(frames, p9)
        kp[:, :, 0] += (p9[:, 2] - p9[:, 6])[:, None]
        kp[:, :, 1] += (p9[:, 1] - p9[:, 5])[:, None]
        return kp

    def timed(call, reps):
        tot, host = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host.append(t1 - t0)
            tot.append(t2 - t0)
        return float(np.median(tot)) * 1e3, float(np.median(host)) * 1e3

    def affine_cells():
        """the pad route and the affine route of infer_boxes, interleaved"""
        lines = [f'# boxes_bench --crop affine: ViTPose-{args.variant.upper()} coco {args.dtype}, {W}x{H} device frames, max_batch {args.max_batch}; rounds of one pad call and '
                 f'one affine call, each followed by a device synchronisation (host clock), {args.reps} rounds after {args.warmup} warm-up rounds per cell',
                 '# ms = median [10th .. 90th percentile] of call + sync; im2col = the im2col family of one profiled call (box kernel + crop kernel + patch gather); '
                 'x = affine median / pad median',
                 f'{"P":>3} {"F":>3} {"crops":>5} | {"pad ms":>8} {"p10":>8} {"p90":>8} {"im2col":>7} | {"affine ms":>9} {"p10":>8} {"p90":>8} {"im2col":>7} | {"x":>6}']
        print('\n'.join(lines), flush=True)
        for P in Ps:
            boxes = [person_boxes(np.random.default_rng(1000 * P + i), P, H, W) for i in range(nF)]
            for F in Fs:
                b6 = np.zeros((P * F, 6), np.float32)
                b6[:, :5] = np.concatenate(boxes[:F])
                d_boxes = torch.from_numpy(b6).cuda()
                d_fidx = torch.from_numpy(np.repeat(np.arange(F, dtype=np.int32), P)).cuda()
                outs = {c: torch.empty((P * F, eng.K, 3), device='cuda') for c in ('pad', 'affine')}
                frames = dev[:F]
                calls = {c: (lambda c=c: eng.infer_boxes(frames, d_boxes, d_fidx, out=outs[c], crop=c)) for c in ('pad', 'affine')}
                ms = {'pad': [], 'affine': []}
                for r in range(args.warmup + args.reps):
                    for c in ('pad', 'affine'):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        calls[c]()
                        torch.cuda.synchronize()
                        if r >= args.warmup:
                            ms[c].append((time.perf_counter() - t0) * 1e3)
                fam = {}
                for c in ('pad', 'affine'):   # one profiled call per route, outside the timed rounds (profiling serialises the launches)
                    eng.set_profiling(['im2col'])
                    eng.reset_profile()
                    calls[c]()
                    torch.cuda.synchronize()
                    fam[c] = eng.profile()['im2col']['ms']
                    eng.set_profiling(False)
                q = {c: np.percentile(ms[c], [50, 10, 90]) for c in ms}
                row = (f'{P:>3} {F:>3} {P * F:>5} | {q["pad"][0]:>8.3f} {q["pad"][1]:>8.3f} {q["pad"][2]:>8.3f} {fam["pad"]:>7.3f} | '
                       f'{q["affine"][0]:>9.3f} {q["affine"][1]:>8.3f} {q["affine"][2]:>8.3f} {fam["affine"]:>7.3f} | {q["affine"][0] / q["pad"][0]:>6.3f}')
                print(row, flush=True)
                lines.append(row)
        return lines

    if args.crop == 'affine':
        lines = affine_cells()
        eng.close()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')
        return

    lines = [f'# boxes_bench: ViTPose-{args.variant.upper()} coco {args.dtype}, {W}x{H} device frames, max_batch {args.max_batch}, median of '
             f'{args.reps} calls, each followed by a device synchronisation (host clock), {args.warmup} warm-up calls per cell and route',
             '# (a) boxes .cpu() + frames_crop_params + infer_frames (device frames) + host offsets; (b) infer_boxes; ms = call + sync; '
             'kP/s = thousands of persons per second; host = ms inside the call before the sync; x = (a) ms / (b) ms',
             f'{"P":>3} {"F":>3} {"crops":>5} | {"(a) ms":>8} {"kP/s":>7} {"host":>7} | {"(b) ms":>8} {"kP/s":>7} {"host":>7} | {"x":>5}']
    print('\n'.join(lines), flush=True)
    for P in Ps:
        boxes = [person_boxes(np.random.default_rng(1000 * P + i), P, H, W) for i in range(nF)]
        for F in Fs:
            b6 = np.zeros((P * F, 6), np.float32)
            b6[:, :5] = np.concatenate(boxes[:F])
            d_boxes = torch.from_numpy(b6).cuda()
            d_fidx = torch.from_numpy(np.repeat(np.arange(F, dtype=np.int32), P)).cuda()
            out = torch.empty((P * F, eng.K, 3), device='cuda')
            frames = dev[:F]
            n = P * F
            want = route_a(frames, d_boxes, d_fidx)
            eng.infer_boxes(frames, d_boxes, d_fidx, out=out)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), 'routes (a) and (b) differ'
            res = {}
            for name, call in (('a', lambda: route_a(frames, d_boxes, d_fidx)), ('b', lambda: eng.infer_boxes(frames, d_boxes, d_fidx, out=out))):
                for _ in range(args.warmup):
                    call()
                torch.cuda.synchronize()
                res[name] = timed(call, args.reps)
            (ma, ha), (mb, hb) = res['a'], res['b']
            row = (f'{P:>3} {F:>3} {n:>5} | {ma:>8.3f} {n / ma:>7.2f} {ha:>7.3f} | {mb:>8.3f} {n / mb:>7.2f} {hb:>7.3f} | {ma / mb:>5.2f}')
            print(row, flush=True)
            lines.append(row)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
