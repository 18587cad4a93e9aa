#!/usr/bin/env python3
"""The metrics stage (vp_metrics_update_stream) against the route a validation loop had before it.  The method of tools/chain_bench.py.

    update    vp_metrics_update_stream (through DeviceMetrics.update, norm / area / rank given, PCK at three thresholds, AUC of 20 steps, OKS) between two device
              events around windows of back-to-back calls of at least --window-ms, ms per call, median and min .. max of --reps windows; against the host route,
              host clock: synchronise, download the predictions, the numpy twin on them (ground truth, normalisers and areas already on the host), median and
              min .. max of --host-reps routes (5 from 8192 rows on) after 2 warm-up routes; n in {8, 64, 512, 8192} x K in {17, 133}.  Every shape is warmed up
              first, and the state after the windows is compared with the host tap's after one call (every count = calls x the tap's).
    read rate the rows kernel at 8192 x 133: bytes the call reads (pred and gt rows, norm, area, rank) over the time of the whole update -- both kernels, so a
              LOWER bound of the rows kernel's rate -- and over that time minus the time of an update without rows (the finish kernel alone on no blocks; an
              upper estimate, the finish kernel over 128 blocks takes longer), with the OKS and the AUC on and with both off (the loads alone).

    python tools/metrics_bench.py [--reps 7] [--window-ms 50] [--host-reps 20] [--out profiles/metrics.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(v):
    v = sorted(v)
    return v[len(v) // 2], f'{v[len(v) // 2]:.4f} ({v[0]:.4f} .. {v[-1]:.4f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=50.0)
    ap.add_argument('--host-reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.devmetrics import MetricsCfg, metrics_numpy, metrics_tap, new_state
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.posenms import COCO17_SIGMAS
    from easy_vitpose_amd.synth import synthetic_state_dict
    assert torch.cuda.is_available(), 'metrics_bench measures on a GPU'
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    lines = ['# metrics_bench: the metrics stage on one MI355X, product library, ms: median (min .. max)',
             f'# vp_metrics_update_stream between two device events, windows of >= {args.window_ms:g} ms, {args.reps} windows; host route: sync, download pred, numpy twin',
             '| n | K | device ms | host route ms | host / device |', '|---|---|---|---|---|']
    rng = np.random.default_rng(1)

    def window(call):
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
        return dev, 5 + 1 + calls * args.reps

    def data(n, K):
        gt = rng.uniform(0, 250, (n, K, 3)).astype(np.float32)
        gt[:, :, 2] = rng.integers(0, 3, (n, K))
        pred = gt + rng.standard_normal((n, K, 3)).astype(np.float32) * 4
        norm = rng.uniform(50, 300, (n, 2)).astype(np.float32)
        area = (norm[:, 0] * norm[:, 1]).astype(np.float32)
        rank = rng.integers(-1, 4, n).astype(np.int32)
        return dict(pred=pred, gt=gt, norm=norm, area=area, rank=rank)

    slower = []
    for K in (17, 133):
        cfg = MetricsCfg(n_joints=K, sigmas=COCO17_SIGMAS if K == 17 else (0.05,) * K)
        for n in (8, 64, 512, 8192):
            h = data(n, K)
            d = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
            ev = eng.metrics(cfg)
            dev, total = window(lambda: ev.update(**d))
            got = ev.state()
            one = new_state(cfg)
            metrics_tap(one, cfg, **h)
            for f in ('counted', 'oks_rows', 'valid_norm', 'valid_px', 'pck_hits', 'auc_hits', 'oks_hits'):
                assert np.array_equal(got[f], one[f] * total), f
            assert int(got['calls']) == total
            ev.close()
            host, reps = [], (args.host_reps if n < 8192 else min(args.host_reps, 5))
            for r in range(reps + 2):
                st = new_state(cfg)
                t0 = time.perf_counter()
                torch.cuda.synchronize()
                p = d['pred'].cpu().numpy()
                metrics_numpy(st, cfg, p, h['gt'], norm=h['norm'], area=h['area'], rank=h['rank'])
                if r >= 2:
                    host.append((time.perf_counter() - t0) * 1e3)
            (dm, ds), (hm, hs) = stat(dev), stat(host)
            lines.append(f'| {n} | {K} | {ds} | {hs} | {hm / dm:.1f} |')
            if dm > hm:
                slower.append(f'n = {n}, K = {K}')
            print(lines[-1], flush=True)
    lines.append('# cells where the device is slower than the host route: ' + (', '.join(slower) if slower else 'none'))

    # ---- the read rate of the rows kernel at the cap
    n, K = 8192, 133
    h = data(n, K)
    d = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
    nbytes = 2 * n * K * 12 + n * (8 + 4 + 4)
    lines.append(f'# read rate at {n} x {K}: {nbytes / 1e6:.2f} MB read per call (pred, gt, norm, area, rank); lanes of a wave read 12-byte records {12 * K} bytes apart')
    lines.append('| configuration | update ms | update without rows ms | GB/s over the whole update (lower bound) | GB/s over the difference (upper estimate) |')
    lines.append('|---|---|---|---|---|')
    for name, cfg in (('PCK x 3, AUC 20, OKS', MetricsCfg(n_joints=K, sigmas=(0.05,) * K)),
                      ('PCK x 3 only (no AUC, no OKS)', MetricsCfg(n_joints=K, auc_steps=0)),
                      ('no PCK, no AUC, no OKS: the loads, two counts, two sums', MetricsCfg(n_joints=K, pck_thr=(), auc_steps=0))):
        ev = eng.metrics(cfg)
        full, _ = window(lambda: ev.update(**d))
        empty, _ = window(lambda: ev.update(d['pred'][:0], d['gt'][:0]))
        ev.close()
        (fm, fs), (em, es) = stat(full), stat(empty)
        lines.append(f'| {name} | {fs} | {es} | {nbytes / fm / 1e6:.0f} | {nbytes / max(fm - em, 1e-6) / 1e6:.0f} |')
        print(lines[-1], flush=True)
    eng.close()

    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
