#!/usr/bin/env python3
"""The COCO keypoint evaluator (vp_cocoeval_update_stream, vp_cocoeval_accumulate_stream) against the route a validation loop had before it.  The method of
tools/metrics_bench.py.

    update      DeviceCocoEval.update between two device events around windows of back-to-back calls of at least --window-ms, ms per call, median and min .. max of
                --reps windows, at 8 / 64 / 256 images of 1 / 8 / 20 detections and as many gts each, K = 17 and 133.  The table holds 2^20 records; once it is full
                a window's later calls count their records as dropped -- the matching work of a call is the same, only the 16-byte stores fall away.  Against the
                host route, host clock: synchronise, download keypoints and scores, the numpy twin's update (ground truth already on the host), median and
                min .. max of --host-reps routes (3 from 64 images on) after one warm-up route.
    accumulate  DeviceCocoEval.accumulate the same way on a table of exactly 1 k / 16 k / 128 k / 1 M records (max_records = the count, so the sort network has that
                size); against synchronise, download the state, the numpy twin's accumulate.  The device result is compared with the host tap's first.

    python tools/cocoeval_bench.py [--reps 7] [--window-ms 50] [--host-reps 10] [--out profiles/cocoeval.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def stat(v):
    v = sorted(v)
    return v[len(v) // 2], f'{v[len(v) // 2]:.4f} ({v[0]:.4f} .. {v[-1]:.4f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=50.0)
    ap.add_argument('--host-reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import cocoeval_cases as cc
    from easy_vitpose_amd import devcoco as dc
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.synth import synthetic_state_dict
    assert torch.cuda.is_available(), 'cocoeval_bench measures on a GPU'
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    rng = np.random.default_rng(1)

    def window(call):
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        calls = max(10, int(args.window_ms / 1e3 / max(time.perf_counter() - t0, 1e-5)))
        dev = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                call()
            b.record()
            b.synchronize()
            dev.append(a.elapsed_time(b) / calls)
        return dev

    def to_device(call):
        return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in cc.inputs(call).items()}

    lines = ['# cocoeval_bench: the COCO keypoint evaluator on one MI355X, product library, ms: median (min .. max)',
             f'# update: vp_cocoeval_update_stream between two device events, windows of >= {args.window_ms:g} ms, {args.reps} windows; host route: sync, download '
             'keypoints and scores, numpy twin',
             '| images | detections = gts per image | K | device ms | host route ms | host / device |', '|---|---|---|---|---|---|']
    slower = []
    for K in (17, 133):
        cfg = dc.CocoEvalCfg(K, 1 << 20, cc.sigmas_for(K))
        ev = eng.cocoeval(cfg)
        for images in (8, 64, 256):
            for per in (1, 8, 20):
                h = cc._call(rng, K, [(per, per)] * images)
                d = to_device(h)
                dev = window(lambda: ev.update(**d))
                host, reps = [], (args.host_reps if images < 64 else min(args.host_reps, 3))
                for r in range(reps + 1):
                    st = dc.new_state(dc.CocoEvalCfg(K, images * per, cc.sigmas_for(K)))
                    t0 = time.perf_counter()
                    torch.cuda.synchronize()
                    kp, sc = d['kpts'].cpu().numpy(), d['score'].cpu().numpy()
                    dc.cocoeval_numpy_update(st, dc.CocoEvalCfg(K, images * per, cc.sigmas_for(K)), kp, sc, **{k: v for k, v in cc.inputs(h).items() if k not in ('kpts', 'score')})
                    if r >= 1:
                        host.append((time.perf_counter() - t0) * 1e3)
                (dm, ds), (hm, hs) = stat(dev), stat(host)
                lines.append(f'| {images} | {per} | {K} | {ds} | {hs} | {hm / dm:.1f} |')
                if dm > hm:
                    slower.append(f'update {images} x {per}, K = {K}')
                print(lines[-1], flush=True)
        ev.close()

    lines += [f'# accumulate: vp_cocoeval_accumulate_stream the same way on a table of exactly R records (max_records = R); host route: sync, download the state, numpy twin',
              '| records | device ms | host route ms | host / device |', '|---|---|---|---|']
    K = 17
    h = cc._call(rng, K, [(20, 2)] * 256, quantise=4096)
    d = to_device(h)
    for R in (1 << 10, 1 << 14, 1 << 17, 1 << 20):
        cfg = dc.CocoEvalCfg(K, R)
        ev = eng.cocoeval(cfg)
        for _ in range(-(-R // (256 * 20))):
            ev.update(**d)
        torch.cuda.synchronize()
        st = ev.state()
        assert int(st['records']) == R
        assert ev.accumulate_host().tobytes() == dc.cocoeval_tap_accumulate(st, cfg).tobytes(), R
        out = torch.empty((dc.RESULT.itemsize,), dtype=torch.uint8, device='cuda')
        dev = window(lambda: ev.accumulate(out=out))
        host = []
        for r in range(min(args.host_reps, 3) + 1):
            t0 = time.perf_counter()
            s = ev.state()
            dc.cocoeval_numpy_accumulate(s)
            if r >= 1:
                host.append((time.perf_counter() - t0) * 1e3)
        ev.close()
        (dm, ds), (hm, hs) = stat(dev), stat(host)
        lines.append(f'| {R} | {ds} | {hs} | {hm / dm:.1f} |')
        if dm > hm:
            slower.append(f'accumulate {R}')
        print(lines[-1], flush=True)
    lines.append('# cells where the device is slower than the host route: ' + (', '.join(slower) if slower else 'none'))
    eng.close()

    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
