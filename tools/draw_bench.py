#!/usr/bin/env python3
"""The skeleton overlay on the device (vp_draw_poses_stream) against the route a caller had before it, and what it adds behind infer_boxes + pose_nms.

Workload: one 1920 x 1080 device frame, RGB24 and NV12 (BT709); P seeded persons whose joints lie in a box of 60..220 x 120..400 pixels, every joint confident;
K = 17 with the COCO skeleton (19 limbs) at P = 1, 8, 64, and K = 133 with a seeded 150-limb table at P = 64.  Default style (radius 7 at 1080p, thickness 2).

    device   vp_draw_poses_stream itself (ctypes): back-to-back calls between two device events, as many as fill --window-ms (at least --calls), ms per call;
             median and min .. max of --reps windows.  enq = the host time of one call without any synchronisation: where it equals the device figure the
             cell measures how fast the host can enqueue two launches, not kernel time
    host     the route without the entry, host clock: synchronise, download the keypoints AND the frame, the library's host model (vp_dbg_draw_host, the same
             arithmetic in C++ on one core), upload the frame, synchronise; median and min .. max of --host-reps routes after 3 warm-up routes
    added    infer_boxes(nms=) + draw_poses against infer_boxes(nms=) alone, ViTPose-B fp16, 64 boxes on one 1920 x 1080 RGB frame, alternating, each followed
             by a device synchronisation (host clock), median and min .. max of --host-reps

    python tools/draw_bench.py [--reps 9] [--window-ms 50] [--host-reps 20] [--out profiles/draw_overlay.txt]
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


def people(rng, n, K):
    kp = np.empty((n, K, 3), np.float32)
    for i in range(n):
        cw, ch = int(rng.integers(60, 220)), int(rng.integers(120, 400))
        x0, y0 = int(rng.integers(0, W - cw)), int(rng.integers(0, H - ch))
        kp[i, :, 0], kp[i, :, 1], kp[i, :, 2] = rng.uniform(y0, y0 + ch, K), rng.uniform(x0, x0 + cw, K), 0.9
    return kp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
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
    from easy_vitpose_amd.draw import COCO17_SKELETON, DrawStyle, c_config, image_table, resolve_skeleton
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.posenms import PoseNms
    from easy_vitpose_amd.synth import synthetic_state_dict
    assert torch.cuda.is_available(), 'draw_bench measures on a GPU'

    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=64)
    lib = eng.lib
    rgb = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, uv = rgb_to_nv12(rgb, 'bt709')
    limbs133 = tuple(map(tuple, np.random.default_rng(8).integers(0, 133, (150, 2)).tolist()))

    lines = [f'# draw_bench: vp_draw_poses_stream on one {W} x {H} device frame between two device events, windows of >= {args.window_ms:g} ms and >= {args.calls} back-to-back '
             f'calls, ms per call: median (min .. max) of {args.reps} windows; enq = host ms inside one call, no synchronisation.',
             f'# host route (host clock): sync, keypoint + frame download, vp_dbg_draw_host, frame upload, sync: median (min .. max) of {args.host_reps} after 3 warm-up routes.',
             '# recs = primitive records of the call; ratio = host median / device median (lowest .. highest: host min / device max .. host max / device min)',
             f'{"fmt":>5} {"K":>4} {"P":>4} {"recs":>6} | {"device ms":>9} {"(min .. max)":>19} {"enq":>7} | {"host ms":>8} {"(min .. max)":>19} | {"ratio":>6} {"(lowest .. highest)":>19}']
    print('\n'.join(lines), flush=True)
    for fmt in ('rgb', 'nv12'):
        for K, P in ((17, 1), (17, 8), (17, 64), (133, 64)):
            style = DrawStyle() if K == 17 else DrawStyle(skeleton=limbs133)
            kp = people(np.random.default_rng(100 * K + P), P, K)
            fi = np.zeros(P, np.int32)
            planes = (rgb,) if fmt == 'rgb' else (y, uv)
            d_planes = [torch.from_numpy(p).cuda() for p in planes]
            d_frame = Frame.rgb(d_planes[0]) if fmt == 'rgb' else Frame.nv12(d_planes[0], d_planes[1], 'bt709')
            table = eng._image_table([d_frame], device_only=True)
            d_kp, d_fi = torch.from_numpy(kp).cuda(), torch.from_numpy(fi).cuda()
            c, keep = c_config(style, resolve_skeleton('coco', K, style.skeleton))
            recs = P * (keep[0].shape[0] + K)
            stream = torch.cuda.current_stream().cuda_stream

            def call():
                capi.check(lib.vp_draw_poses_stream(eng._h, table, 1, d_kp.data_ptr(), P, K, d_fi.data_ptr(), 1, None, None, None, 4, C.byref(c), stream), eng._h)

            def host_model(h_kp, h_planes):
                fr = Frame.rgb(h_planes[0]) if fmt == 'rgb' else Frame.nv12(h_planes[0], h_planes[1], 'bt709')
                capi.check(lib.vp_dbg_draw_host(image_table([fr]), 1, h_kp.ctypes.data, P, K, fi.ctypes.data, 1, None, None, None, 4, C.byref(c)))
            call()
            want = [p.copy() for p in planes]
            host_model(kp, want)
            for g, w in zip(d_planes, want):
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
                h_planes = [p.cpu().numpy() for p in d_planes]
                host_model(d_kp.cpu().numpy(), h_planes)
                for d, hp in zip(d_planes, h_planes):
                    d.copy_(torch.from_numpy(hp))
                torch.cuda.synchronize()
                host_ms.append((time.perf_counter() - t0) * 1e3)
            host_ms = host_ms[3:]
            dm, hm = float(np.median(dev_ms)), float(np.median(host_ms))
            row = (f'{fmt:>5} {K:>4} {P:>4} {recs:>6} | {dm:>9.4f} ({min(dev_ms):>7.4f} .. {max(dev_ms):>7.4f}) {float(np.median(enq)):>7.4f} | '
                   f'{hm:>8.3f} ({min(host_ms):>7.3f} .. {max(host_ms):>7.3f}) | {hm / dm:>6.1f} ({min(host_ms) / max(dev_ms):>7.1f} .. {max(host_ms) / min(dev_ms):>7.1f})')
            print(row, flush=True)
            lines.append(row)

    # what the stage adds behind the boxes entry and the NMS
    n = 64
    frame = torch.from_numpy(rgb).cuda()
    b6 = np.zeros((n, 6), np.float32)
    b6[:, :5] = person_boxes(np.random.default_rng(64000), n, H, W)
    d_boxes = torch.from_numpy(b6).cuda()
    out = torch.empty((n, eng.K, 3), device='cuda')
    cfg, style = PoseNms(), DrawStyle(conf_thr=0.0)

    def chain():
        return eng.infer_boxes([frame], d_boxes, out=out, nms=cfg, crop_params=True)

    def chain_draw():
        o, score, rank, count, cp = chain()
        eng.draw_poses([frame], o, cp[:, 0], style, rank=rank, boxes=d_boxes)
    calls = {'chain': chain, 'chain+draw': chain_draw}
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
    a, b = float(np.median(ms['chain'])), float(np.median(ms['chain+draw']))
    tail = [f'# added cost: ViTPose-{args.variant.upper()} fp16, {n} boxes on one {W}x{H} device RGB frame, call + device synchronisation (host clock), alternating, '
            f'{args.host_reps} calls each; draw_poses with the NMS ranks as the mask and the box outlines',
            f'infer_boxes(nms=) {a:.3f} ms ({min(ms["chain"]):.3f} .. {max(ms["chain"]):.3f})   + draw_poses {b:.3f} ms '
            f'({min(ms["chain+draw"]):.3f} .. {max(ms["chain+draw"]):.3f})   added {b - a:+.3f} ms ({(b / a - 1) * 100:+.2f} %)']
    print('\n'.join(tail), flush=True)
    lines += tail
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
