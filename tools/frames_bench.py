#!/usr/bin/env python3
"""Crops of several frames per call (vp_infer_frames) against today's one call per frame (vp_infer_frame).

Workload: ViTPose-B / coco, fp16, seeded 1920x1080 frames with P persons each (boxes on a jittered grid, as tools/stream_bench.py),
F frames per call.  Four ways to run the same F frames:

    per-frame   F calls of vp_infer_frame, pageable host frames (what VitInference.inference does frame by frame)
    pageable    ONE vp_infer_frames call, pageable host frames (one upload of each frame's row band)
    pinned      ONE vp_infer_frames call, frames in page-locked memory (vp_host_alloc)
    device      ONE vp_infer_frames call, frames already in device memory (torch CUDA tensors, read in place)

Every shape is warmed up first; then a host clock around each synchronised call (the calls return with the keypoints on the host),
the median of --reps calls.  Also printed: the bytes one call uploads (sum of the row bands) next to the full frames' bytes.

    python tools/frames_bench.py [--persons 1,2,4,8,16] [--frames 1,4,16,32] [--reps 7] [--max-batch 256] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def person_boxes(rng, n, h, w):
    cols = int(np.ceil(np.sqrt(n * w / h)))
    rows = -(-n // cols)
    out = []
    for i in range(n):
        cx = (i % cols + 0.5) * w / cols + rng.uniform(-0.1, 0.1) * w / cols
        cy = (i // cols + 0.5) * h / rows + rng.uniform(-0.1, 0.1) * h / rows
        bw = rng.uniform(0.3, 0.6) * w / cols
        bh = rng.uniform(0.5, 0.8) * h / rows
        out.append([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2, 1.0])
    return np.asarray(out)


def band_bytes(frames, p9):
    from easy_vitpose_amd import _capi as capi
    lib = capi.load_library()
    t = (capi.vp_frame * len(frames))(*[capi.vp_frame(f.ctypes.data, f.shape[0], f.shape[1]) for f in frames])
    bands = np.zeros((len(frames), 2), np.int32)
    assert lib.vp_dbg_frame_plan(t, len(frames), p9.ctypes.data, len(p9), bands.ctypes.data) == capi.VP_OK
    return int(sum((b1 - b0) * f.shape[1] * 3 for (b0, b1), f in zip(bands, frames)))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--persons', default='1,2,4,8,16')
    ap.add_argument('--frames', default='1,4,16,32')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--dtype', default='fp16')
    ap.add_argument('--max-batch', type=int, default=256)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.cropprep import frames_crop_params
    from easy_vitpose_amd.engine import PinnedArray, VitPoseHip
    from easy_vitpose_amd.synth import synthetic_state_dict

    Ps = [int(x) for x in args.persons.split(',')]
    Fs = [int(x) for x in args.frames.split(',')]
    H, W = args.height, args.width
    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=args.dtype, max_batch=args.max_batch)
    rng = np.random.default_rng(0)
    nF = max(Fs)
    host = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(nF)]
    pinned = []
    for f in host:
        p = PinnedArray(f.shape, np.uint8)
        p.array[:] = f
        pinned.append(p)
    dev = [torch.from_numpy(f).cuda() for f in host]
    torch.cuda.synchronize()

    lines = [f'# frames_bench: ViTPose-{args.variant.upper()} coco {args.dtype}, {W}x{H} frames, max_batch {args.max_batch}, '
             f'median of {args.reps} synchronised calls (host clock), {args.warmup} warm-up calls per shape and case',
             f'# ms = one call over all F frames (per-frame: the loop of F vp_infer_frame calls); kP/s = thousands of persons per second; '
             f'x = per-frame loop time / batched time',
             f'{"P":>3} {"F":>3} {"crops":>5} {"band MB":>8} {"full MB":>8} | {"per-frame":>9} {"kP/s":>7} | {"pageable":>8} {"kP/s":>7} {"x":>5} | '
             f'{"pinned":>8} {"kP/s":>7} {"x":>5} | {"device":>8} {"kP/s":>7} {"x":>5}']
    print('\n'.join(lines), flush=True)
    for P in Ps:
        boxes = [person_boxes(np.random.default_rng(1000 * P + i), P, H, W) for i in range(nF)]
        for F in Fs:
            p9 = frames_crop_params(boxes[:F], [f.shape for f in host[:F]])
            per = [p9[p9[:, 0] == i, 1:] for i in range(F)]
            n = len(p9)
            cases = {
                'per-frame': lambda: [eng.infer_frame(host[i], per[i]) for i in range(F)],
                'pageable': lambda: eng.infer_frames(host[:F], p9),
                'pinned': lambda: eng.infer_frames([p.array for p in pinned[:F]], p9),
                'device': lambda: eng.infer_frames(dev[:F], p9),
            }
            ref = np.concatenate(cases['per-frame']())
            ms = {}
            for name, fn in cases.items():
                for _ in range(args.warmup):
                    fn()
                ms[name] = timed(fn, args.reps)
                if name != 'per-frame':   # the same crops: the bits may differ from the per-frame loop only through the chunk sizes (split-K at 1-2 crops)
                    got = fn()
                    assert got.shape == ref.shape and np.isfinite(got).all()
            bb = band_bytes(host[:F], p9)
            row = f'{P:>3} {F:>3} {n:>5} {bb / 1e6:>8.1f} {F * H * W * 3 / 1e6:>8.1f} | {ms["per-frame"]:>9.3f} {n / ms["per-frame"]:>7.2f} |'
            for name in ('pageable', 'pinned', 'device'):
                row += f' {ms[name]:>8.3f} {n / ms[name]:>7.2f} {ms["per-frame"] / ms[name]:>5.2f} |'
            print(row.rstrip(' |'), flush=True)
            lines.append(row.rstrip(' |'))
    for p in pinned:
        p.free()
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
