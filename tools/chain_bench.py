#!/usr/bin/env python3
"""The collect stage (vp_collect_stream) against the route a caller had before it.  The method of tools/label_bench.py (profiles/draw_labels.txt).

    collect   vp_collect_stream (through VitPoseHip.collect) between two device events around windows of back-to-back calls of at least --window-ms, ms per
              call, median and min .. max of --reps windows; against the route without it, host clock: synchronise, five downloads (keypoints, ids, rank,
              score, crop params) and the numpy filter, median and min .. max of --host-reps routes after 3 warm-up routes; n in {8, 64, 512, 8192} x K in
              {17, 133}, the 8192 rows on 64 frames.  Every shape is warmed up first, and the table of every shape is compared with the numpy twin.

    python tools/chain_bench.py [--reps 7] [--window-ms 50] [--host-reps 20] [--out profiles/device_chain.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

def med(v):
    v = sorted(v)
    return f'{v[len(v) // 2]:.4f} ({v[0]:.4f} .. {v[-1]:.4f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=50.0)
    ap.add_argument('--host-reps', type=int, default=20)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.devcollect import collect_bytes, collect_numpy
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.synth import synthetic_state_dict
    assert torch.cuda.is_available(), 'chain_bench measures on a GPU'
    shp = model_shape(args.variant, 'coco')
    sd = synthetic_state_dict(shp, 0, peaked=True)
    lines = ['# chain_bench: the collect stage on one MI355X, product library, ms: median (min .. max)']

    # ---- (a) collect alone
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=64)
    lines.append(f'# vp_collect_stream between two device events, windows of >= {args.window_ms:g} ms, {args.reps} windows; host route: sync, 5 downloads, numpy filter, '
                 f'{args.host_reps} routes')
    lines.append('| n | K | device ms | host route ms | ratio |')
    lines.append('|---|---|---|---|---|')
    rng = np.random.default_rng(1)
    for K in (17, 133):
        for n in (8, 64, 512, 8192):
            nf = 1 if n < 8192 else 64
            kp = torch.from_numpy(rng.uniform(0, 1000, (n, K, 3)).astype(np.float32)).cuda()
            ids = torch.arange(n, dtype=torch.int32, device='cuda')
            fr = torch.from_numpy((np.arange(n) % nf).astype(np.int32)).cuda()
            rank = torch.from_numpy(rng.integers(-1, 3, n).astype(np.int32)).cuda()
            score = torch.from_numpy(rng.uniform(0, 1, n).astype(np.float32)).cuda()
            cp = torch.from_numpy(rng.integers(0, 1000, (n, 9)).astype(np.int32)).cuda()
            out = torch.empty((collect_bytes(nf, K, n),), dtype=torch.uint8, device='cuda')
            call = lambda: eng.collect(kp, ids=ids, frame=fr, rank=rank, score=score, crop_params=cp, n_frames=nf, out=out)   # noqa: E731
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            calls = max(20, int(args.window_ms / 1e3 / max(time.perf_counter() - t0, 1e-5)))
            dev = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    call()
                b.record()
                b.synchronize()
                dev.append(a.elapsed_time(b) / calls)
            host = []
            for r in range(args.host_reps + 3):
                t0 = time.perf_counter()
                torch.cuda.synchronize()
                h = [t.cpu().numpy() for t in (kp, ids, rank, score, cp)]
                keep = h[2] >= 0
                _ = {int(i): k for i, k in zip(h[1][keep], h[0][keep])}
                if r >= 3:
                    host.append((time.perf_counter() - t0) * 1e3)
            lines.append(f'| {n} | {K} | {med(dev)} | {med(host)} | {sorted(host)[len(host) // 2] / sorted(dev)[len(dev) // 2]:.1f} |')
            want = collect_numpy(kp.cpu().numpy(), ids.cpu().numpy(), fr.cpu().numpy(), rank.cpu().numpy(), None, score.cpu().numpy(), cp.cpu().numpy(), nf, n)
            written = collect_bytes(nf, K, int(want.view(np.int32)[nf]))   # the header and the records that exist: the tail of the buffer is not written
            assert np.array_equal(out.cpu().numpy()[:written], want[:written])
    eng.close()

    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
