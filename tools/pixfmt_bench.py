#!/usr/bin/env python3
"""NV12 frames on the boxes entry: what the pixel formats of vp_image cost and what they save.

Workload: ViTPose-B / coco, fp16, seeded 1920x1080 frames in device memory with P persons each (boxes on a jittered grid, as
tools/frames_bench.py), F frames per call; the detector's boxes are a float32 CUDA tensor [n, 6] with an int32 CUDA frame index.

    rgb      (a) packed RGB tensors through VitPoseHip.infer_boxes -- the call every earlier commit has, so the same script measures it on
             another tree:  --tree DIR  imports the package (and its library) from DIR instead of this checkout
    nv12     (b) the same content as NV12 surfaces (Y pitch 2048, UV in the same allocation behind 1088 rows) through infer_boxes on Frame.nv12
    convert  (c) the route without vp_image: a full-frame NV12 -> RGB conversion of every frame in torch ops (int32, the library's own arithmetic:
             its keypoints are checked to be (b)'s bit for bit), then (a)

Per cell: ms = host clock around one call followed by a device synchronisation, median of --reps calls after --warmup calls.

    python tools/pixfmt_bench.py [--routes rgb,nv12,convert] [--persons 8,64] [--frames 4] [--reps 15] [--tree DIR] [--label TEXT] [--out FILE] [--append]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y_PITCH, ALIGNED_H = 2048, 1088


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--routes', default='rgb,nv12,convert')
    ap.add_argument('--persons', default='8,64')
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--dtype', default='fp16')
    ap.add_argument('--max-batch', type=int, default=256)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--tree', default=ROOT, help='the checkout whose easy_vitpose_amd package (and built library) is measured')
    ap.add_argument('--label', default='this commit')
    ap.add_argument('--out', default=None)
    ap.add_argument('--append', action='store_true')
    args = ap.parse_args()

    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from frames_bench import person_boxes
    import torch
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.synth import synthetic_state_dict

    routes = args.routes.split(',')
    Ps = [int(x) for x in args.persons.split(',')]
    F, H, W = args.frames, args.height, args.width
    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=args.dtype, max_batch=args.max_batch)
    rng = np.random.default_rng(0)
    host_rgb = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(F)]

    nv12 = None
    if 'nv12' in routes or 'convert' in routes:
        from easy_vitpose_amd.cropprep import YUV_COEFS, Frame, rgb_to_nv12, to_rgb
        ch, cw = (H + 1) // 2, (W + 1) // 2
        surfaces, nv12 = [], []
        for a in host_rgb:
            y, uv = rgb_to_nv12(a, 'bt601')
            buf = np.zeros(Y_PITCH * ALIGNED_H + Y_PITCH * ch, np.uint8)
            buf[:Y_PITCH * H].reshape(H, Y_PITCH)[:, :W] = y
            buf[Y_PITCH * ALIGNED_H:].reshape(ch, Y_PITCH)[:, :2 * cw] = uv.reshape(ch, -1)
            d = torch.from_numpy(buf).cuda()   # a decoder surface: one allocation, UV at base + pitch * aligned_h
            surfaces.append(d)
            nv12.append(Frame.nv12(d[:Y_PITCH * H].reshape(H, Y_PITCH)[:, :W], d[Y_PITCH * ALIGNED_H:].reshape(ch, Y_PITCH)[:, :2 * cw].reshape(ch, cw, 2), 'bt601'))
        host_rgb = [to_rgb(f) for f in nv12]   # the three routes see the same pixels
        yoff, cy, crv, cgu, cgv, cbu = YUV_COEFS['bt601']

        def torch_convert(fr):
            y, uv = fr.planes
            yy = (y.to(torch.int32) - yoff).clamp_(min=0) * cy + (1 << 19)
            c = (uv.to(torch.int32) - 128).repeat_interleave(2, 0).repeat_interleave(2, 1)[:H, :W]
            u, v = c[..., 0], c[..., 1]
            return torch.stack([(yy + crv * v) >> 20, (yy + cgu * u + cgv * v) >> 20, (yy + cbu * u) >> 20], -1).clamp_(0, 255).to(torch.uint8)
    dev_rgb = [torch.from_numpy(a).cuda() for a in host_rgb]
    torch.cuda.synchronize()

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        tot = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            tot.append(time.perf_counter() - t0)
        return float(np.median(tot)) * 1e3

    lines = [f'# pixfmt_bench [{args.label}]: ViTPose-{args.variant.upper()} coco {args.dtype}, {F} device frames of {W}x{H}, max_batch {args.max_batch}, median ms of '
             f'{args.reps} calls (call + device synchronisation, host clock), {args.warmup} warm-up calls per cell']
    print(lines[0], flush=True)
    for P in Ps:
        b6 = np.zeros((P * F, 6), np.float32)
        b6[:, :5] = np.concatenate([person_boxes(np.random.default_rng(1000 * P + i), P, H, W) for i in range(F)])
        d_boxes = torch.from_numpy(b6).cuda()
        d_fidx = torch.from_numpy(np.repeat(np.arange(F, dtype=np.int32), P)).cuda()
        out = torch.empty((P * F, eng.K, 3), device='cuda')
        calls = {
            'rgb': lambda: eng.infer_boxes(dev_rgb, d_boxes, d_fidx, out=out),
            'nv12': lambda: eng.infer_boxes(nv12, d_boxes, d_fidx, out=out),
            'convert': lambda: eng.infer_boxes([torch_convert(f) for f in nv12], d_boxes, d_fidx, out=out),
        }
        want = None
        for r in routes:   # every route the same keypoints, bit for bit
            calls[r]()
            torch.cuda.synchronize()
            got = out.cpu().numpy().copy()
            assert want is None or np.array_equal(got, want), f'route {r} differs'
            want = got
        row = f'P={P:<3} crops={P * F:<4} ' + '  '.join(f'{r} {timed(calls[r]):8.3f} ms' for r in routes)
        print(row, flush=True)
        lines.append(row)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a' if args.append else 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
