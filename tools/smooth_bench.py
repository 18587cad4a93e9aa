#!/usr/bin/env python3
"""Keypoint smoothing on the device (vp_smooth_update_stream) against the route a video caller had before it, and what it adds behind infer_boxes(nms=).

Workload: seeded keypoint walks (tests/smooth_cases.py people: a random walk per joint, 3 % of the coordinates missing), P persons per call spread round-robin
over S streams, every stream stepped in every call, every person present in every frame (the steady state of a video: every row is an update).  A window
replays the 12 frames of the sequence in order, again and again, so the filter state keeps moving as it does on a video.

    device   vp_smooth_update_stream itself (ctypes, outputs allocated once): back-to-back calls between two device events, as many as fill --window-ms
             (at least --calls), ms per call; median and min .. max of --reps windows.  `enq` = host ms inside one call, no synchronisation
    host     the route without the entry, host clock: synchronise, download keypoints / ids / streams, the library's host model (vp_dbg_smooth_host, the
             same arithmetic in C++ on one core), upload the keypoints, synchronise; median and min .. max of --host-reps routes after 3 warm-up routes
    added    infer_boxes(nms=) -> update against infer_boxes(nms=) -> the host route, ViTPose-B fp16, 64 boxes on one 1920x1080 frame, alternating, each chain
             followed by a device synchronisation (host clock), median and min .. max of --host-reps

    python tools/smooth_bench.py [--reps 7] [--window-ms 50] [--host-reps 30] [--out profiles/smooth_device.txt]
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from smooth_cases import people  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=48)
    ap.add_argument('--window-ms', type=float, default=50.0)
    ap.add_argument('--host-reps', type=int, default=30)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from easy_vitpose_amd import _capi as capi
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.devsmooth import DeviceSmoother, HostSmoother, SmoothCfg
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.posenms import PoseNms
    from easy_vitpose_amd.synth import synthetic_state_dict
    from frames_bench import person_boxes
    assert torch.cuda.is_available(), 'smooth_bench measures on a GPU'

    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=64)
    lib = eng.lib
    lines = [f'# smooth_bench: vp_smooth_update_stream between two device events, windows of >= {args.window_ms:g} ms and >= {args.calls} back-to-back calls (the frames of a '
             f'12-frame sequence in order, repeated), ms per call: median (min .. max) of {args.reps} windows; enq = host ms inside one call, no synchronisation.',
             f'# host route (host clock): sync, download of keypoints / ids / streams, vp_dbg_smooth_host, upload of the keypoints, sync: median (min .. max) of '
             f'{args.host_reps} after 3 warm-up routes.',
             '# P persons per call spread over S streams, K joints, every row an update; ratio = host median / device median',
             f'{"P":>4} {"K":>4} {"S":>3} | {"device ms":>9} {"(min .. max)":>21} {"enq":>7} | {"host ms":>8} {"(min .. max)":>19} | {"ratio":>6}']
    print('\n'.join(lines), flush=True)
    F = 12
    for P in (1, 8, 64, 128):
        for K in (17, 133):
            for S in (1, 32):
                kp = people(np.random.default_rng(P * 1000 + K), P, K, F)
                ids = (1 + np.arange(P) // S).astype(np.int32)
                st = (np.arange(P) % S).astype(np.int32)
                cfg = SmoothCfg(fps=30.0, n_streams=S, max_rows=max(P, 1))
                dev, tap = DeviceSmoother(eng, K, cfg), HostSmoother(K, cfg)
                d_kp = [torch.from_numpy(np.ascontiguousarray(kp[f])).cuda() for f in range(F)]
                d_ids, d_st = torch.from_numpy(ids).cuda(), torch.from_numpy(st).cuda()
                d_out = torch.empty_like(d_kp[0])
                d_flags = torch.empty(S, dtype=torch.int32, device='cuda')
                stream = torch.cuda.current_stream().cuda_stream
                mask = (1 << S) - 1

                def call(k):
                    capi.check(lib.vp_smooth_update_stream(dev._s, d_kp[k % F].data_ptr(), d_ids.data_ptr(), d_st.data_ptr(), None, P, mask, None, d_out.data_ptr(),
                                                           d_flags.data_ptr(), stream), eng._h)
                for k in range(F):   # correctness, once over the sequence
                    call(k)
                    want, _ = tap.update(kp[k], ids, st)
                    assert d_out.cpu().numpy().tobytes() == want.tobytes(), 'device and host model disagree'
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for k in range(args.calls):
                    call(k)
                b.record()
                b.synchronize()
                calls = max(args.calls, int(np.ceil(args.window_ms / max(a.elapsed_time(b) / args.calls, 1e-4))))
                calls = (calls + F - 1) // F * F
                dev_ms, enq = [], []
                for _ in range(args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    t0 = time.perf_counter()
                    for k in range(calls):
                        call(k)
                    enq.append((time.perf_counter() - t0) * 1e3 / calls)
                    b.record()
                    b.synchronize()
                    dev_ms.append(a.elapsed_time(b) / calls)
                host_ms = []
                for k in range(args.host_reps + 3):
                    t0 = time.perf_counter()
                    torch.cuda.synchronize()
                    out, _ = tap.update(d_kp[k % F].cpu().numpy(), d_ids.cpu().numpy(), d_st.cpu().numpy())
                    up = torch.from_numpy(out).cuda()
                    torch.cuda.synchronize()
                    host_ms.append((time.perf_counter() - t0) * 1e3)
                host_ms = host_ms[3:]
                dm, hm = float(np.median(dev_ms)), float(np.median(host_ms))
                row = (f'{P:>4} {K:>4} {S:>3} | {dm:>9.4f} ({min(dev_ms):>8.4f} .. {max(dev_ms):>8.4f}) {float(np.median(enq)):>7.4f} | '
                       f'{hm:>8.4f} ({min(host_ms):>7.4f} .. {max(host_ms):>7.4f}) | {hm / dm:>6.2f}')
                print(row, flush=True)
                lines.append(row)
                dev.close()

    # what the stage adds behind the boxes entry
    H, W, n = 1080, 1920, 64
    rng = np.random.default_rng(7)
    frame = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    d5 = np.ascontiguousarray(person_boxes(np.random.default_rng(64000), n, H, W)[:, :5], dtype=np.float32)
    d_dets = torch.from_numpy(d5).cuda()
    d_ids = torch.arange(1, n + 1, dtype=torch.int32, device='cuda')
    cfg, nms = SmoothCfg(fps=30.0, max_rows=n), PoseNms()
    dev, tap = DeviceSmoother(eng, eng.K, cfg), HostSmoother(eng.K, cfg)

    def boxes_only():
        return eng.infer_boxes([frame], d_dets, nms=nms)

    def device_chain():
        out, score, rank, kept = eng.infer_boxes([frame], d_dets, nms=nms)[:4]
        return dev.update(out, d_ids, rank=rank, out=out)

    def host_chain():
        out, score, rank, kept = eng.infer_boxes([frame], d_dets, nms=nms)[:4]
        torch.cuda.synchronize()
        sm, _ = tap.update(out.cpu().numpy(), d_ids.cpu().numpy(), rank=rank.cpu().numpy())
        return torch.from_numpy(sm).cuda()
    chains = {'infer_boxes(nms=)': boxes_only, 'infer_boxes(nms=) + device smoother': device_chain, 'infer_boxes(nms=) + host smoother': host_chain}
    for c in chains.values():
        for _ in range(3):
            c()
    torch.cuda.synchronize()
    ms = {k: [] for k in chains}
    for _ in range(args.host_reps):
        for name, c in chains.items():   # alternating
            t0 = time.perf_counter()
            c()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    tail = [f'# added cost: ViTPose-{args.variant.upper()} fp16, {n} boxes on one {W}x{H} device frame, chain + device synchronisation (host clock), alternating, {args.host_reps} each']
    base = float(np.median(ms['infer_boxes(nms=)']))
    for name, v in ms.items():
        m = float(np.median(v))
        tail.append(f'{name:<38} {m:.3f} ms ({min(v):.3f} .. {max(v):.3f})   {m - base:+.3f} ms ({(m / base - 1) * 100:+.2f} %)')
    print('\n'.join(tail), flush=True)
    lines += tail
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
