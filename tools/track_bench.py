#!/usr/bin/env python3
"""The box tracker on the device (vp_tracker_update_stream) against the route a video caller had before it, and what it adds in front of infer_boxes.

Workload: seeded crowds (tests/track_cases.py crowd: persons moving at constant velocity with box jitter and misses), P persons on each of S streams, rows
interleaved over the streams.  Two kinds of crowd: `sparse` (persons spread over a field that grows with P, so that no two overlap: every frame takes the
shortcut branch) and `dense` (the 640 x 360 field of the tests: from 8 persons on the frames enter the assignment branch).  A window replays the frames of the
sequence in order, again and again, so the tracker state keeps moving as it does on a video.

    device   vp_tracker_update_stream itself (ctypes, outputs allocated once): back-to-back calls between two device events, as many as fill --window-ms
             (at least --calls), ms per call; median and min .. max of --reps windows.  `enq` = host ms inside one call, no synchronisation
    host     the route without the entry, host clock: synchronise, download the detector rows, the library's host model (vp_dbg_track_host, the same
             arithmetic in C++ on one core), upload rows, ids and streams, synchronise; median and min .. max of --host-reps routes after 3 warm-up routes
    added    update -> infer_boxes(nms=) against host tracker -> infer_boxes(nms=) (the host route above in front of it), ViTPose-B fp16, 64 boxes on one
             1920x1080 frame, alternating, each chain followed by a device synchronisation (host clock), median and min .. max of --host-reps

    python tools/track_bench.py [--reps 9] [--window-ms 50] [--host-reps 30] [--out profiles/track_device.txt]
"""
from __future__ import annotations

import argparse
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from track_cases import crowd  # noqa: E402


def sequence(P, S, kind, F=12):
    """per frame (dets float32 [n, 5], stream int32 [n]) with the rows of the streams interleaved"""
    side = 640 if kind == 'dense' else 640 + 400 * P
    per = [crowd(9000 + 100 * P + s, P, F, W=side, H=360 if kind == 'dense' else side, miss=0.05) for s in range(S)]
    rng = np.random.default_rng(P * 1000 + S)
    out = []
    for f in range(F):
        d = np.concatenate([per[s][f] for s in range(S)]).astype(np.float32)
        fi = np.concatenate([np.full(len(per[s][f]), s, np.int32) for s in range(S)])
        order = rng.permutation(len(d))
        out.append((np.ascontiguousarray(d[order]), np.ascontiguousarray(fi[order])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--calls', type=int, default=48)
    ap.add_argument('--window-ms', type=float, default=50.0)
    ap.add_argument('--host-reps', type=int, default=30)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from easy_vitpose_amd import _capi as capi
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.devtracker import DeviceTracker, HostTracker, TrackCfg
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.posenms import PoseNms
    from easy_vitpose_amd.synth import synthetic_state_dict
    from easy_vitpose_amd.tracker import Sort, iou_matrix
    from frames_bench import person_boxes
    assert torch.cuda.is_available(), 'track_bench measures on a GPU'

    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=64)
    lib = eng.lib
    lines = [f'# track_bench: vp_tracker_update_stream between two device events, windows of >= {args.window_ms:g} ms and >= {args.calls} back-to-back calls (the frames of a '
             f'12-frame sequence in order, repeated), ms per call: median (min .. max) of {args.reps} windows; enq = host ms inside one call, no synchronisation.',
             f'# host route (host clock): sync, detector-row download, vp_dbg_track_host, upload of rows / ids / streams, sync: median (min .. max) of {args.host_reps} after 3 warm-up routes.',
             '# P persons on each of S streams; sparse = no overlaps (shortcut branch), dense = 640 x 360 field (assignment branch); lsap = frames of the sequence whose '
             'stream 0 has an ambiguous IoU matrix; ratio = host median / device median',
             f'{"P":>4} {"S":>3} {"kind":>6} {"lsap":>5} | {"device ms":>9} {"(min .. max)":>21} {"enq":>7} | {"host ms":>8} {"(min .. max)":>19} | {"ratio":>6}']
    print('\n'.join(lines), flush=True)
    for P, S in ((1, 1), (8, 1), (32, 1), (64, 1), (128, 1), (16, 4), (16, 32)):
        for kind in ('sparse', 'dense'):
            seq = sequence(P, S, kind)
            cfg = TrackCfg(1, 3, 0.3, S)
            dev, tap = DeviceTracker(eng, cfg), HostTracker(cfg)
            d_seq = [(torch.from_numpy(d).cuda(), torch.from_numpy(fi).cuda()) for d, fi in seq]
            n_out = 128 * S
            d_rows, d_ids, d_st = torch.empty((n_out, 6), device='cuda'), torch.empty(n_out, dtype=torch.int32, device='cuda'), torch.empty(n_out, dtype=torch.int32, device='cuda')
            d_count, d_flags = torch.empty(S + 1, dtype=torch.int32, device='cuda'), torch.empty(S, dtype=torch.int32, device='cuda')
            stream = torch.cuda.current_stream().cuda_stream
            mask = (1 << S) - 1

            def call(k):
                d, fi = d_seq[k % len(d_seq)]
                capi.check(lib.vp_tracker_update_stream(dev._t, d.data_ptr(), 5, fi.data_ptr(), d.shape[0], mask, d_rows.data_ptr(), d_ids.data_ptr(), d_st.data_ptr(), n_out,
                                                        d_count.data_ptr(), d_flags.data_ptr(), stream), eng._h)
            # correctness, once over the sequence
            for k, (d, fi) in enumerate(seq):
                call(k)
                want = tap.update(d, frame_index=fi, n_out=n_out)
                assert d_rows.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(d_count.cpu().numpy(), want[3]), 'device and host model disagree'
            lsap = 0   # frames whose stream 0 enters the assignment branch, read off the Python twin
            twin = Sort(1, 3, cfg.iou_threshold)
            for d, fi in seq:
                d0 = d[fi == 0].astype(np.float64)
                probe = copy.deepcopy(twin)
                pred = np.array([t.predict() for t in probe.tracks]).reshape(-1, 4)
                if len(pred) and len(d0):
                    over = iou_matrix(d0, pred) > cfg.iou_threshold
                    lsap += int(over.sum(1).max() > 1 or over.sum(0).max() > 1)
                twin.update(d0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.calls):
                call(k)
            b.record()
            b.synchronize()
            calls = max(args.calls, int(np.ceil(args.window_ms / max(a.elapsed_time(b) / args.calls, 1e-4))))
            calls = (calls + len(seq) - 1) // len(seq) * len(seq)
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
                d, fi = d_seq[k % len(d_seq)]
                t0 = time.perf_counter()
                torch.cuda.synchronize()
                rows, ids, st, _, _ = tap.update(d.cpu().numpy(), frame_index=fi.cpu().numpy(), n_out=n_out)
                up = (torch.from_numpy(rows).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(st).cuda())
                torch.cuda.synchronize()
                host_ms.append((time.perf_counter() - t0) * 1e3)
            host_ms = host_ms[3:]
            dm, hm = float(np.median(dev_ms)), float(np.median(host_ms))
            row = (f'{P:>4} {S:>3} {kind:>6} {lsap:>2}/{len(seq):<2} | {dm:>9.4f} ({min(dev_ms):>8.4f} .. {max(dev_ms):>8.4f}) {float(np.median(enq)):>7.4f} | '
                   f'{hm:>8.4f} ({min(host_ms):>7.4f} .. {max(host_ms):>7.4f}) | {hm / dm:>6.2f}')
            print(row, flush=True)
            lines.append(row)
            dev.close()

    # what the stage adds in front of the boxes entry
    H, W, n = 1080, 1920, 64
    rng = np.random.default_rng(7)
    frame = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    d5 = np.ascontiguousarray(person_boxes(np.random.default_rng(64000), n, H, W)[:, :5], dtype=np.float32)
    d_dets = torch.from_numpy(d5).cuda()
    cfg, nms = TrackCfg(1, 3, 0.3, 1), PoseNms()
    dev, tap = DeviceTracker(eng, cfg), HostTracker(cfg)

    def device_chain():
        rows, ids, st, _, _ = dev.update(d_dets, n_out=n)
        return eng.infer_boxes([frame], rows, st, nms=nms)

    def host_chain():
        torch.cuda.synchronize()
        rows, ids, st, _, _ = tap.update(d_dets.cpu().numpy(), n_out=n)
        return eng.infer_boxes([frame], torch.from_numpy(rows).cuda(), torch.from_numpy(st).cuda(), nms=nms)

    def boxes_only():
        return eng.infer_boxes([frame], d_dets, nms=nms)
    chains = {'infer_boxes(nms=)': boxes_only, 'device tracker + infer_boxes(nms=)': device_chain, 'host tracker + infer_boxes(nms=)': host_chain}
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
        tail.append(f'{name:<36} {m:.3f} ms ({min(v):.3f} .. {max(v):.3f})   {m - base:+.3f} ms ({(m / base - 1) * 100:+.2f} %)')
    print('\n'.join(tail), flush=True)
    lines += tail
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
