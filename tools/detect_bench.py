#!/usr/bin/env python3
"""The detector stage on the device (vp_detect_stream) against the route a caller had before it, what its scan moves, and what it adds in front of the tracker.

Workload: seeded heads (tests/detect_cases.py random_head): [n, 84, 8400] (YOLOv8 at 640 pixels, 80 classes), a given number of anchors per image over the
threshold, about half of them jittered copies of earlier ones, the rest of the scores below 0.3.

    device   vp_detect_stream itself (ctypes, outputs allocated once): back-to-back calls between two device events, as many as fill --window-ms (at least
             --calls), ms per call; median and min .. max of --reps windows.  `enq` = host ms inside one call, no synchronisation.  GB/s = the head's bytes
             over the device median: the whole entry (three kernels), so a lower bound on what the scan kernel moves
    host     the route without the entry, host clock: synchronise, download the head, the library's host model (vp_dbg_detect_host, the same arithmetic in C++
             on one core), upload rows, image index and counts, synchronise; median and min .. max of --host-reps routes after 2 warm-up routes
    added    detect -> counted tracker -> infer_boxes(nms=) against tracker -> infer_boxes(nms=) on rows that are already on the device, and against the host
             route in front of the same tracker, ViTPose-B fp16, 64 boxes on one 1920x1080 frame, alternating, each chain followed by a device synchronisation
             (host clock), median and min .. max of --host-reps

    python tools/detect_bench.py [--reps 9] [--window-ms 50] [--host-reps 12] [--out profiles/detect_device.txt]
    python tools/detect_bench.py --scan-loop 200      # nothing but 64-image calls: the run a kernel trace is taken of
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

from detect_cases import random_head  # noqa: E402

A, NC, FRAME, INPUT = 8400, 80, (1080, 1920), (640, 640)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--calls', type=int, default=32)
    ap.add_argument('--window-ms', type=float, default=50.0)
    ap.add_argument('--host-reps', type=int, default=12)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--scan-loop', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from easy_vitpose_amd import _capi as capi
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.devdetect import DetectCfg, DeviceDetector, HostDetector, image_table, letterbox_params
    from easy_vitpose_amd.devtracker import DeviceTracker, TrackCfg
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.posenms import PoseNms
    from easy_vitpose_amd.synth import synthetic_state_dict
    from frames_bench import person_boxes
    assert torch.cuda.is_available(), 'detect_bench measures on a GPU'

    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=64)
    lib = eng.lib
    stream = torch.cuda.current_stream().cuda_stream

    def entry(dev, d_pred, n, n_out):
        out = (torch.empty((n_out, 6), device='cuda'), torch.empty(n_out, dtype=torch.int32, device='cuda'), torch.empty(n_out, dtype=torch.int32, device='cuda'),
               torch.empty(n + 1, dtype=torch.int32, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda'))
        tab = image_table(FRAME, INPUT, n)

        def call():
            capi.check(lib.vp_detect_stream(dev._d, d_pred.data_ptr(), A, tab, n, *[t.data_ptr() for t in out[:3]], n_out, out[3].data_ptr(), out[4].data_ptr(), stream), eng._h)
        return call, out

    if args.scan_loop:
        cfg = DetectCfg(nc=NC, dtype='fp16')
        dev = DeviceDetector(eng, cfg)
        for dtype in ('fp16', 'fp32'):
            dev.close()
            dev = DeviceDetector(eng, DetectCfg(nc=NC, dtype=dtype))
            d_pred = torch.from_numpy(random_head(1, [100] * 64, NC, A, 0, dtype)).cuda()
            call, _ = entry(dev, d_pred, 64, 64 * 300)
            for _ in range(args.scan_loop):
                call()
            torch.cuda.synchronize()
        dev.close()
        eng.close()
        return

    lines = [f'# detect_bench: vp_detect_stream between two device events, windows of >= {args.window_ms:g} ms and >= {args.calls} back-to-back calls, ms per call: median '
             f'(min .. max) of {args.reps} windows; enq = host ms inside one call, no synchronisation; GB/s = head bytes / device median (whole entry: three kernels).',
             f'# host route (host clock): sync, head download, vp_dbg_detect_host, upload of rows / image / count, sync: median (min .. max) of {args.host_reps} after 2 warm-up routes.',
             f'# heads [n, {4 + NC}, {A}], conf 0.35, iou 0.7, class-aware, max_det 300; cand = candidates per image, rows = rows of the call; ratio = host median / device median',
             f'{"n":>3} {"dtype":>5} {"cand":>5} {"rows":>6} | {"device ms":>9} {"(min .. max)":>21} {"enq":>7} {"GB/s":>7} | {"host ms":>9} {"(min .. max)":>21} | {"ratio":>7}']
    print('\n'.join(lines), flush=True)
    for dtype in ('fp16', 'fp32'):
        cfg = DetectCfg(nc=NC, dtype=dtype)
        dev, tap = DeviceDetector(eng, cfg), HostDetector(cfg)
        for n in (1, 4, 64):
            for cand in (10, 100, 1000):
                pred = random_head(1000 * n + cand, [cand] * n, NC, A, 0, dtype)
                d_pred = torch.from_numpy(pred).cuda()
                n_out = n * cfg.max_det
                call, out = entry(dev, d_pred, n, n_out)
                call()
                want = tap.detect(pred, FRAME, INPUT, n_out)
                assert all(t.cpu().numpy().tobytes() == w.tobytes() for t, w in zip(out, want)), 'device and host model disagree'
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.calls):
                    call()
                b.record()
                b.synchronize()
                calls = max(args.calls, int(np.ceil(args.window_ms / max(a.elapsed_time(b) / args.calls, 1e-4))))
                dev_ms, enq = [], []
                for _ in range(args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        call()
                    enq.append((time.perf_counter() - t0) * 1e3 / calls)
                    b.record()
                    b.synchronize()
                    dev_ms.append(a.elapsed_time(b) / calls)
                host_ms = []
                for _ in range(args.host_reps + 2):
                    t0 = time.perf_counter()
                    torch.cuda.synchronize()
                    rows, image, anchor, count, flags = tap.detect(d_pred.cpu().numpy(), FRAME, INPUT, n_out)
                    up = (torch.from_numpy(rows).cuda(), torch.from_numpy(image).cuda(), torch.from_numpy(count).cuda())
                    torch.cuda.synchronize()
                    host_ms.append((time.perf_counter() - t0) * 1e3)
                host_ms = host_ms[2:]
                dm, hm = float(np.median(dev_ms)), float(np.median(host_ms))
                row = (f'{n:>3} {dtype:>5} {cand:>5} {int(want[3][-1]):>6} | {dm:>9.4f} ({min(dev_ms):>8.4f} .. {max(dev_ms):>8.4f}) {float(np.median(enq)):>7.4f} '
                       f'{pred.nbytes / dm / 1e6:>7.1f} | {hm:>9.3f} ({min(host_ms):>8.3f} .. {max(host_ms):>8.3f}) | {hm / dm:>7.1f}')
                print(row, flush=True)
                lines.append(row)
        dev.close()

    # what the stage adds in front of the tracker and the boxes entry
    H, W, n = FRAME[0], FRAME[1], 64
    rng = np.random.default_rng(7)
    frame = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    boxes = person_boxes(np.random.default_rng(64000), n, H, W)[:, :5]
    gain, pad_x, pad_y = letterbox_params(FRAME, INPUT)
    head = np.zeros((1, 4 + NC, A), np.float32)
    head[:, :4] = 10
    head[0, 4:] = np.random.default_rng(3).uniform(0, 0.3, (NC, A))
    for k, b in enumerate(boxes):
        x1, y1, x2, y2 = b[0] * gain + pad_x, b[1] * gain + pad_y, b[2] * gain + pad_x, b[3] * gain + pad_y
        head[0, :4, 100 * k + 50] = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1)
        head[0, 4, 100 * k + 50] = 0.9 - 0.005 * k
    head = head.astype(np.float16)
    d_head = torch.from_numpy(head).cuda()
    dcfg, tcfg, nms = DetectCfg(nc=NC, dtype='fp16', classes='human'), TrackCfg(1, 1, 0.3, 1), PoseNms()
    det, tap = DeviceDetector(eng, dcfg), HostDetector(dcfg)
    rows0 = tap.detect(head, FRAME, INPUT, n)
    assert int(rows0[3][-1]) == n, 'the 64 boxes survive the stage'
    d_rows0, d_image0 = torch.from_numpy(rows0[0]).cuda(), torch.from_numpy(rows0[1]).cuda()
    trackers = [DeviceTracker(eng, tcfg) for _ in range(3)]

    def rows_ready():
        rows, ids, st, _, _ = trackers[0].update(d_rows0, d_image0, n_out=n)
        return eng.infer_boxes([frame], rows, st, nms=nms)

    def device_chain():
        rows, image, anchor, count, flags = det.detect(d_head, FRAME, INPUT, n)
        rows, ids, st, _, _ = trackers[1].update(rows, image, n_out=n, n_dets=count[-1:])
        return eng.infer_boxes([frame], rows, st, nms=nms)

    def host_chain():
        torch.cuda.synchronize()
        rows, image, anchor, count, flags = tap.detect(d_head.cpu().numpy(), FRAME, INPUT, n)
        m = int(count[-1])
        rows, ids, st, _, _ = trackers[2].update(torch.from_numpy(rows[:m]).cuda(), torch.from_numpy(image[:m]).cuda(), n_out=n)
        return eng.infer_boxes([frame], rows, st, nms=nms)
    chains = {'tracker + infer_boxes(nms=), rows on the device': rows_ready, 'detect + counted tracker + infer_boxes(nms=)': device_chain,
              'host detect route + tracker + infer_boxes(nms=)': host_chain}
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
    tail = [f'# added cost: ViTPose-{args.variant.upper()} fp16, {n} boxes on one {W}x{H} device frame, head [1, {4 + NC}, {A}] fp16, chain + device synchronisation (host clock), '
            f'alternating, {args.host_reps} each']
    base = float(np.median(ms['tracker + infer_boxes(nms=), rows on the device']))
    for name, v in ms.items():
        m = float(np.median(v))
        tail.append(f'{name:<50} {m:.3f} ms ({min(v):.3f} .. {max(v):.3f})   {m - base:+.3f} ms ({(m / base - 1) * 100:+.2f} %)')
    print('\n'.join(tail), flush=True)
    lines += tail
    for t in trackers:
        t.close()
    det.close()
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
