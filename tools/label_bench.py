#!/usr/bin/env python3
"""The label stage on the device (vp_draw_labels_stream) against the route a caller had before it, and what `labels=` adds behind infer_boxes + draw_poses.
The method of tools/draw_bench.py (profiles/draw_overlay.txt).

Workload: 1920 x 1080 device frames, RGB24 and NV12 (BT709); P seeded person boxes (tools/frames_bench.person_boxes) as tracker rows [P, 6] with the score in
column 4, read in place (box_stride = score_stride = 6), ids = the row index, scale 0 (2 at 1080p), the overlay's limb palette, automatic ink: `#<id>: <score>`
tags of 7 to 9 characters.  P = 1, 8, 64, 512 on one frame, and 64 rows spread over 4 frames.

    device   vp_draw_labels_stream itself (ctypes): back-to-back calls between two device events, as many as fill --window-ms (at least --calls), ms per call;
             median and min .. max of --reps windows.  enq = the host time of one call without any synchronisation: where it equals the device figure the cell
             measures how fast the host can enqueue two launches, not kernel time
    host     the route without the entry, host clock: synchronise, download the rows AND the frames, the library's host model (vp_dbg_draw_labels_host, the
             same arithmetic in C++ on one core), upload the frames, synchronise; median and min .. max of --host-reps routes after 3 warm-up routes
    added    infer_boxes(nms=) + draw_poses(labels=) against infer_boxes(nms=) + draw_poses, ViTPose-B fp16, 64 boxes on one 1920 x 1080 RGB frame, alternating,
             each followed by a device synchronisation (host clock), median and min .. max of --host-reps

    python tools/label_bench.py [--reps 7] [--window-ms 50] [--host-reps 20] [--out profiles/draw_labels.txt]
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

H, W = 1080, 1920


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--window-ms', type=float, default=50.0)
    ap.add_argument('--host-reps', type=int, default=20)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import ctypes as C

    import torch
    from easy_vitpose_amd import Frame
    from easy_vitpose_amd import _capi as capi
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.cropprep import rgb_to_nv12
    from easy_vitpose_amd.draw import DrawStyle, LabelStyle, image_table, label_c_config
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.posenms import PoseNms
    from easy_vitpose_amd.synth import synthetic_state_dict
    assert torch.cuda.is_available(), 'label_bench measures on a GPU'

    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=64)
    lib = eng.lib
    rgb = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, uv = rgb_to_nv12(rgb, 'bt709')
    c, keep = label_c_config(LabelStyle())

    lines = [f'# label_bench: vp_draw_labels_stream on {W} x {H} device frames between two device events, windows of >= {args.window_ms:g} ms and >= {args.calls} back-to-back '
             f'calls, ms per call: median (min .. max) of {args.reps} windows; enq = host ms inside one call, no synchronisation.',
             f'# host route (host clock): sync, row + frame download, vp_dbg_draw_labels_host, frame upload, sync: median (min .. max) of {args.host_reps} after 3 warm-up routes.',
             '# P = rows (tags) of the call, F = frames of the table; ratio = host median / device median (lowest .. highest: host min / device max .. host max / device min)',
             f'{"fmt":>5} {"F":>2} {"P":>4} | {"device ms":>9} {"(min .. max)":>19} {"enq":>7} | {"host ms":>8} {"(min .. max)":>19} | {"ratio":>6} {"(lowest .. highest)":>19}']
    print('\n'.join(lines), flush=True)
    for fmt in ('rgb', 'nv12'):
        for P, F in ((1, 1), (8, 1), (64, 1), (512, 1), (64, 4)):
            rng = np.random.default_rng(1000 * F + P)
            rows = np.zeros((P, 6), np.float32)
            rows[:, :5] = person_boxes(rng, P, H, W)
            rows[:, 4] = rng.uniform(0.35, 1.0, P)
            fi = (np.arange(P) % F).astype(np.int32)
            planes = [(rgb.copy(),) if fmt == 'rgb' else (y.copy(), uv.copy()) for _ in range(F)]
            d_planes = [[torch.from_numpy(p).cuda() for p in pl] for pl in planes]
            d_frames = [Frame.rgb(pl[0]) if fmt == 'rgb' else Frame.nv12(pl[0], pl[1], 'bt709') for pl in d_planes]
            table = eng._image_table(d_frames, device_only=True)
            d_rows, d_fi = torch.from_numpy(rows).cuda(), torch.from_numpy(fi).cuda()
            stream = torch.cuda.current_stream().cuda_stream

            def call():
                capi.check(lib.vp_draw_labels_stream(eng._h, table, F, d_rows.data_ptr(), 6, P, d_fi.data_ptr(), 1, None, None, d_rows.data_ptr() + 16, 6, C.byref(c), stream), eng._h)

            def host_model(h_rows, h_planes):
                fr = [Frame.rgb(pl[0]) if fmt == 'rgb' else Frame.nv12(pl[0], pl[1], 'bt709') for pl in h_planes]
                capi.check(lib.vp_dbg_draw_labels_host(image_table(fr), F, h_rows.ctypes.data, 6, P, fi.ctypes.data, 1, None, None, h_rows.ctypes.data + 16, 6, C.byref(c)))
            call()
            want = [[p.copy() for p in pl] for pl in planes]
            host_model(rows, want)
            for gp, wp in zip(d_planes, want):
                for g, w in zip(gp, wp):
                    assert np.array_equal(g.cpu().numpy(), w), 'device and host model disagree'
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
            for _ in range(args.host_reps + 3):
                t0 = time.perf_counter()
                torch.cuda.synchronize()
                h_planes = [[p.cpu().numpy() for p in pl] for pl in d_planes]
                host_model(d_rows.cpu().numpy(), h_planes)
                for dp, hp in zip(d_planes, h_planes):
                    for d, h in zip(dp, hp):
                        d.copy_(torch.from_numpy(h))
                torch.cuda.synchronize()
                host_ms.append((time.perf_counter() - t0) * 1e3)
            host_ms = host_ms[3:]
            dm, hm = float(np.median(dev_ms)), float(np.median(host_ms))
            row = (f'{fmt:>5} {F:>2} {P:>4} | {dm:>9.4f} ({min(dev_ms):>7.4f} .. {max(dev_ms):>7.4f}) {float(np.median(enq)):>7.4f} | '
                   f'{hm:>8.3f} ({min(host_ms):>7.3f} .. {max(host_ms):>7.3f}) | {hm / dm:>6.1f} ({min(host_ms) / max(dev_ms):>7.1f} .. {max(host_ms) / min(dev_ms):>7.1f})')
            print(row, flush=True)
            lines.append(row)

    # what labels= adds behind the boxes entry, the NMS and the overlay
    n = 64
    frame = torch.from_numpy(rgb).cuda()
    b6 = np.zeros((n, 6), np.float32)
    b6[:, :5] = person_boxes(np.random.default_rng(64000), n, H, W)
    d_boxes = torch.from_numpy(b6).cuda()
    out = torch.empty((n, eng.K, 3), device='cuda')
    cfg, style, labels = PoseNms(), DrawStyle(conf_thr=0.0), LabelStyle()

    def chain():
        o, score, rank, count, cp = eng.infer_boxes([frame], d_boxes, out=out, nms=cfg, crop_params=True)
        eng.draw_poses([frame], o, cp[:, 0], style, rank=rank, boxes=d_boxes)

    def chain_labels():
        o, score, rank, count, cp = eng.infer_boxes([frame], d_boxes, out=out, nms=cfg, crop_params=True)
        eng.draw_poses([frame], o, cp[:, 0], style, rank=rank, boxes=d_boxes, labels=labels, scores=d_boxes[:, 4])
    calls = {'chain': chain, 'chain+labels': chain_labels}
    for call in calls.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.host_reps):
        for name, call in calls.items():   # alternating
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    a, b = float(np.median(ms['chain'])), float(np.median(ms['chain+labels']))
    tail = [f'# added cost: ViTPose-{args.variant.upper()} fp16, {n} boxes on one {W}x{H} device RGB frame, call + device synchronisation (host clock), alternating, '
            f'{args.host_reps} calls each; draw_poses with the NMS ranks as the mask and the box outlines, labels= with the box scores read in place',
            f'infer_boxes(nms=) + draw_poses {a:.3f} ms ({min(ms["chain"]):.3f} .. {max(ms["chain"]):.3f})   with labels= {b:.3f} ms '
            f'({min(ms["chain+labels"]):.3f} .. {max(ms["chain+labels"]):.3f})   added {b - a:+.3f} ms ({(b / a - 1) * 100:+.2f} %)']
    print('\n'.join(tail), flush=True)
    lines += tail
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
