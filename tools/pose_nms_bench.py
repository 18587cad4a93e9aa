#!/usr/bin/env python3
"""Person scores + OKS pose NMS on the device (vp_pose_nms_stream) against the route a caller had before it, and what it adds to infer_boxes.

Workload: seeded people (about half of them jittered copies of earlier ones, as the test fixtures), keypoints / box scores / crop params as float32 /
int32 CUDA tensors, P persons on each of F frames, K = 17 (COCO sigmas) and K = 133 (uniform sigmas 0.05), hard NMS (oks_thr 0.9: up to P picks per
frame) and soft NMS (max_dets 20 picks per frame).

    device   vp_pose_nms_stream itself (ctypes, outputs allocated once): back-to-back calls between two device events, as many as fill --window-ms
             (at least --calls), ms per call; median and min .. max of --reps windows.  In the smallest cells this is the rate at which the host can
             enqueue the launch, not kernel time: the two are told apart by `enq`, the host time of one call without any synchronisation
    host     the route without the entry, host clock: synchronise, download the keypoints, the library's host model (vp_dbg_pose_nms_host, the same
             arithmetic in C++ on one core; box scores and crop params are the caller's host copies), upload the keep mask, synchronise; median and
             min .. max of --host-reps routes after 3 warm-up routes
    added    infer_boxes(nms=) against infer_boxes alone, ViTPose-B fp16, 64 boxes on one 1920x1080 frame, alternating, each call followed by a
             device synchronisation (host clock), median and min .. max of --host-reps

    python tools/pose_nms_bench.py [--reps 9] [--window-ms 50] [--host-reps 30] [--out profiles/pose_nms.txt]
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


def people(rng, n_per_frame, n_frames, K):
    n = n_per_frame * n_frames
    kp, p9 = np.zeros((n, K, 3), np.float32), np.zeros((n, 9), np.int32)
    for i in range(n):
        f, first = i % n_frames, i < n_frames   # rows of the frames interleaved
        if not first and rng.random() < 0.5:
            src = int(rng.integers(0, i // n_frames)) * n_frames + f
            kp[i, :, :2] = kp[src, :, :2] + rng.normal(0.0, float(rng.choice([0.2, 1.0, 3.0])) * 6.0, (K, 2))
            kp[i, :, 2] = np.clip(kp[src, :, 2] + rng.normal(0.0, 0.1, K), 0.05, 1.0)
            p9[i] = p9[src]
        else:
            cw, ch = int(rng.integers(60, 220)), int(rng.integers(120, 400))
            x0, y0 = int(rng.integers(0, 1920 - cw)), int(rng.integers(0, 1080 - ch))
            kp[i, :, 0], kp[i, :, 1], kp[i, :, 2] = rng.uniform(y0, y0 + ch, K), rng.uniform(x0, x0 + cw, K), rng.uniform(0.05, 1.0, K)
            p9[i] = [f, x0, y0, cw, ch, 0, 0, cw, ch]
    return kp, rng.uniform(0.35, 0.99, n).astype(np.float32), p9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--window-ms', type=float, default=50.0)
    ap.add_argument('--host-reps', type=int, default=30)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import ctypes as C

    import torch
    from easy_vitpose_amd import _capi as capi
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.posenms import COCO17_SIGMAS, PoseNms, c_config
    from easy_vitpose_amd.synth import synthetic_state_dict
    assert torch.cuda.is_available(), 'pose_nms_bench measures on a GPU'

    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=64)
    lib = eng.lib

    def host_model(kp, bs, p9, F, c):   # vp_dbg_pose_nms_host: rank [n]
        n, K = kp.shape[0], kp.shape[1]
        score, rank, count = np.empty(n, np.float32), np.empty(n, np.int32), np.empty(F, np.int32)
        capi.check(lib.vp_dbg_pose_nms_host(kp.ctypes.data, n, K, bs.ctypes.data, 1, p9.ctypes.data, None, F, C.byref(c), score.ctypes.data, rank.ctypes.data,
                                            count.ctypes.data))
        return rank

    lines = [f'# pose_nms_bench: vp_pose_nms_stream between two device events, windows of >= {args.window_ms:g} ms and >= {args.calls} back-to-back calls, ms per call: '
             f'median (min .. max) of {args.reps} windows; enq = host ms inside one call, no synchronisation.',
             f'# host route (host clock): sync, keypoint download, vp_dbg_pose_nms_host, mask upload, sync: median (min .. max) of {args.host_reps} after 3 warm-up routes.',
             '# hard = oks_thr 0.9, soft = max_dets 20; kept = rows with rank >= 0; ratio = host median / device median (lowest .. highest: host min / device max .. host max / device min)',
             f'{"K":>4} {"P":>4} {"F":>2} {"mode":>5} {"kept":>5} | {"device ms":>8} {"(min .. max)":>19} {"enq":>7} | {"host ms":>8} {"(min .. max)":>19} | {"ratio":>6} {"(lowest .. highest)":>19}']
    print('\n'.join(lines), flush=True)
    for K in (17, 133):
        sig = np.asarray(COCO17_SIGMAS if K == 17 else (0.05,) * K, np.float32)
        for P, F in ((1, 1), (8, 1), (64, 1), (256, 1), (64, 4)):
            kp, bs, p9 = people(np.random.default_rng(1000 * K + 10 * P + F), P, F, K)
            n = len(kp)
            d_kp, d_bs, d_p9 = torch.from_numpy(kp).cuda(), torch.from_numpy(bs).cuda(), torch.from_numpy(p9).cuda()
            d_score, d_rank = torch.empty(n, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda')
            d_count = torch.empty(F, dtype=torch.int32, device='cuda')
            for mode, cfg in (('hard', PoseNms()), ('soft', PoseNms(soft=True))):
                c, keep = c_config(cfg, sig)
                stream = torch.cuda.current_stream().cuda_stream

                def call():
                    capi.check(lib.vp_pose_nms_stream(eng._h, d_kp.data_ptr(), n, K, d_bs.data_ptr(), 1, d_p9.data_ptr(), None, F, C.byref(c), d_score.data_ptr(),
                                                      d_rank.data_ptr(), d_count.data_ptr(), stream), eng._h)
                call()
                wr = host_model(kp, bs, p9, F, c)
                assert np.array_equal(d_rank.cpu().numpy(), wr), 'device and host model disagree'
                # one window to size the next ones
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
                    hr = host_model(d_kp.cpu().numpy(), bs, p9, F, c)
                    mask = torch.from_numpy(hr >= 0).cuda()
                    torch.cuda.synchronize()
                    host_ms.append((time.perf_counter() - t0) * 1e3)
                host_ms = host_ms[3:]
                dm, hm = float(np.median(dev_ms)), float(np.median(host_ms))
                row = (f'{K:>4} {P:>4} {F:>2} {mode:>5} {int((wr >= 0).sum()):>5} | {dm:>8.4f} ({min(dev_ms):>7.4f} .. {max(dev_ms):>7.4f}) {float(np.median(enq)):>7.4f} | '
                       f'{hm:>8.4f} ({min(host_ms):>7.4f} .. {max(host_ms):>7.4f}) | {hm / dm:>6.2f} ({min(host_ms) / max(dev_ms):>7.2f} .. {max(host_ms) / min(dev_ms):>7.2f})')
                print(row, flush=True)
                lines.append(row)

    # what the stage adds behind the boxes entry
    H, W, n = 1080, 1920, 64
    rng = np.random.default_rng(7)
    frame = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    b6 = np.zeros((n, 6), np.float32)
    b6[:, :5] = person_boxes(np.random.default_rng(64000), n, H, W)
    d_boxes = torch.from_numpy(b6).cuda()
    out = torch.empty((n, eng.K, 3), device='cuda')
    cfg = PoseNms()
    calls = {'infer_boxes': lambda: eng.infer_boxes([frame], d_boxes, out=out), 'infer_boxes(nms=)': lambda: eng.infer_boxes([frame], d_boxes, out=out, nms=cfg)}
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
    a, b = float(np.median(ms['infer_boxes'])), float(np.median(ms['infer_boxes(nms=)']))
    tail = [f'# added cost: ViTPose-{args.variant.upper()} fp16, {n} boxes on one {W}x{H} device frame, call + device synchronisation (host clock), alternating, {args.host_reps} calls each',
            f'infer_boxes {a:.3f} ms ({min(ms["infer_boxes"]):.3f} .. {max(ms["infer_boxes"]):.3f})   infer_boxes(nms=PoseNms()) {b:.3f} ms '
            f'({min(ms["infer_boxes(nms=)"]):.3f} .. {max(ms["infer_boxes(nms=)"]):.3f})   added {b - a:+.3f} ms ({(b / a - 1) * 100:+.2f} %)']
    print('\n'.join(tail), flush=True)
    lines += tail
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
