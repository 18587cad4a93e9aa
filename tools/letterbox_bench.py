#!/usr/bin/env python3
"""The letterbox stage on the device (vp_letterbox_stream) against the two routes a caller had before it, what it moves, and what it adds in front of the detector stage.

Workload: seeded frames on the device, 1920x1080 (3 x down into 640 x 640) and 1280x720 (exactly 2 x: the box average), NV12 (bt709) and RGB24, 1 / 8 / 64 frames
per call, into [n, 3, 640, 640] fp16 NCHW; fp32 and u8 at 64 frames.

    device   vp_letterbox_stream itself (ctypes, output allocated once): back-to-back calls between two device events, as many as fill --window-ms (at least
             --calls), ms per call; median and min .. max of --reps windows.  `enq` = host ms inside one call, no synchronisation.
    bytes    output bytes + the 128-byte lines of the source planes that hold a tap (counted from the coefficients, cropprep._axis_coeffs); TB/s = bytes over the
             device median; `of copy` = that over the float4 copy rate tools/peak.py measures in a child process of the same run (read + write bytes per second)
    torch    (a) what a caller writes in PyTorch on the device for RGB frames ([n, H, W, 3] uint8): permute, float, F.interpolate(bilinear, align_corners=False),
             F.pad(114), / 255, .half() -- other bits, time only; same windows and events.  NV12 has no such one-liner: '-'
    host     (b) the route without the entry, host clock: synchronise, download the planes, the library's host model (vp_dbg_letterbox_host, the same arithmetic
             in C++ on one core), upload the tensor, synchronise; median and min .. max of --host-reps routes after 1 warm-up route
    added    letterbox -> detect -> counted tracker -> infer_boxes(nms=) against the same chain without the letterbox, ViTPose-B fp16, 64 boxes on one 1920x1080
             NV12 device frame, alternating, each chain followed by a device synchronisation (host clock), median and min .. max of --chain-reps

    python tools/letterbox_bench.py [--reps 9] [--window-ms 50] [--host-reps 3] [--out profiles/letterbox.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

INPUT = (640, 640)
SIZES = {'1080p': (1080, 1920), '720p': (720, 1280)}
LINE = 128


def copy_rate_tbs():
    """the float4 copy rate of tools/peak.py (TB/s, read + write), measured by a child process of this run before this process opens the device"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'peak.py')], capture_output=True, text=True, timeout=600)
    m = re.search(r'float4 copy read\+write \(TB/s\): ([0-9.]+) rc=0', r.stdout)
    if not m:
        raise RuntimeError(f'tools/peak.py gave no copy rate:\n{r.stdout}\n{r.stderr}')
    return float(m.group(1))


def source_bytes(fmt, h, w, placement):
    """bytes of the 128-byte lines of one frame's planes that hold a tap (rows start on a line: 1920, 1280 and three times them are multiples of 128)"""
    from easy_vitpose_amd.cropprep import _axis_coeffs
    left, top, new_w, new_h = placement
    if (new_h, new_w) == (h // 2, w // 2) and h % 2 == 0 and w % 2 == 0:
        ys, xs = np.arange(h), np.arange(w)
    else:
        sy, sy1 = _axis_coeffs(new_h, h)[:2]
        sx, sx1 = _axis_coeffs(new_w, w)[:2]
        ys, xs = np.unique(np.concatenate([sy, sy1])), np.unique(np.concatenate([sx, sx1]))
    if fmt == 'rgb':
        return len(ys) * len(np.unique(np.concatenate([(3 * xs) // LINE, (3 * xs + 2) // LINE]))) * LINE
    return len(ys) * len(np.unique(xs // LINE)) * LINE + len(np.unique(ys >> 1)) * len(np.unique(((xs >> 1) * 2) // LINE)) * LINE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--calls', type=int, default=16)
    ap.add_argument('--window-ms', type=float, default=50.0)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--chain-reps', type=int, default=12)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    copy_tbs = copy_rate_tbs()

    import torch
    import torch.nn.functional as F
    from easy_vitpose_amd import _capi as capi
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.cropprep import Frame, rgb_to_nv12
    from easy_vitpose_amd.devdetect import DetectCfg, letterbox_params
    from easy_vitpose_amd.devletterbox import HostLetterbox, LetterboxCfg, c_config, image_table, letterbox_plan
    from easy_vitpose_amd.devtracker import TrackCfg
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.posenms import PoseNms
    from easy_vitpose_amd.synth import synthetic_state_dict
    from frames_bench import person_boxes
    assert torch.cuda.is_available(), 'letterbox_bench measures on a GPU'

    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=64)
    lib = eng.lib
    stream = torch.cuda.current_stream().cuda_stream
    tdt = {'fp16': torch.float16, 'fp32': torch.float32, 'u8': torch.uint8}
    seeded = {}   # size -> (8 seeded RGB frames, their NV12 planes), made once

    def make_frames(size, fmt, n):
        """n distinct device frames (8 seeded ones, then device copies shifted by a constant) and the stacked RGB tensor route (a) reads"""
        h, w = SIZES[size]
        if size not in seeded:
            rng = np.random.default_rng(h)
            base = rng.integers(0, 256, (8, h // 8, w // 8, 3), dtype=np.uint8).repeat(8, 1).repeat(8, 2)
            base = (base.astype(np.int16) + rng.integers(-16, 16, base.shape)).clip(0, 255).astype(np.uint8)
            seeded[size] = (base, [rgb_to_nv12(f, 'bt709') for f in base])
        base, planes = seeded[size][0][:min(n, 8)], seeded[size][1][:min(n, 8)]
        stack = torch.from_numpy(base).cuda()
        stack = torch.cat([stack + 3 * k for k in range((n + 7) // 8)])[:n].contiguous()
        if fmt == 'rgb':
            return [Frame.rgb(stack[i]) for i in range(n)], stack
        ys, uvs = torch.from_numpy(np.stack([p[0] for p in planes])).cuda(), torch.from_numpy(np.stack([p[1] for p in planes])).cuda()
        ys = torch.cat([ys + 3 * k for k in range((n + 7) // 8)])[:n].contiguous()
        uvs = torch.cat([uvs + k for k in range((n + 7) // 8)])[:n].contiguous()
        return [Frame.nv12(ys[i], uvs[i], 'bt709') for i in range(n)], None

    def windows(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        call()
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.calls):
            call()
        b.record()
        b.synchronize()
        calls = max(args.calls, int(np.ceil(args.window_ms / max(a.elapsed_time(b) / args.calls, 1e-4))))
        ms, enq = [], []
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
            ms.append(a.elapsed_time(b) / calls)
        return ms, float(np.median(enq))

    lines = [f'# letterbox_bench: vp_letterbox_stream between two device events, windows of >= {args.window_ms:g} ms and >= {args.calls} back-to-back calls, ms per call: median '
             f'(min .. max) of {args.reps} windows; enq = host ms inside one call, no synchronisation.',
             f'# MB = output bytes + 128-byte source lines that hold a tap; TB/s = MB / device median; of copy = TB/s over the float4 copy rate of tools/peak.py in this run: '
             f'{copy_tbs:.1f} TB/s (read + write).',
             '# torch (a): permute, float, F.interpolate(bilinear), F.pad(114), / 255, .half() on the stacked RGB frames, same windows (other bits: time only); a/dev = '
             'torch median / device median.',
             f'# host (b), host clock: sync, plane download, vp_dbg_letterbox_host, tensor upload, sync: median (min .. max) of {args.host_reps} after 1 warm-up; b/dev likewise.',
             '# kernel: a workgroup of 128 threads per output row: a lane per pixel into LDS, then a lane per 16 output bytes per channel plane (8 fp16 / 4 fp32 / 16 u8 '
             'adjacent x), dwordx4 stores; VGPRs 60 / 38 / 110 and 8 / 8 / 4 waves per SIMD for fp16 / fp32 / u8, no scratch (hipcc -Rpass-analysis=kernel-resource-usage).',
             f'{"n":>3} {"size":>5} {"fmt":>4} {"out":>4} | {"device ms":>9} {"(min .. max)":>21} {"enq":>7} {"MB":>7} {"TB/s":>6} {"of copy":>7} | {"torch ms":>9} {"(min .. max)":>21} '
             f'{"a/dev":>6} | {"host ms":>9} {"(min .. max)":>21} {"b/dev":>8}']
    print('\n'.join(lines), flush=True)
    cells = [(n, size, fmt, 'fp16') for size in SIZES for fmt in ('nv12', 'rgb') for n in (1, 8, 64)] + [(64, '1080p', fmt, dt) for dt in ('fp32', 'u8') for fmt in ('nv12', 'rgb')]
    verdict = []
    for n, size, fmt, dtype in cells:
        h, w = SIZES[size]
        cfg = LetterboxCfg(INPUT, dtype=dtype)
        frames, stack = make_frames(size, fmt, n)
        tab, c = image_table(frames), c_config(cfg)
        out = torch.empty(cfg.shape(n), dtype=tdt[dtype], device='cuda')
        ptr = C.cast(tab.ctypes.data, C.POINTER(capi.vp_image))

        def call():
            capi.check(lib.vp_letterbox_stream(eng._h, C.byref(c), ptr, n, out.data_ptr(), None, None, stream), eng._h)
        call()
        torch.cuda.synchronize()
        host_frames = [Frame(f.format, tuple(p.cpu().numpy() for p in f.planes), f.matrix) for f in frames[:2]]
        assert out[:2].cpu().numpy().tobytes() == HostLetterbox(cfg).letterbox(host_frames)[0].tobytes(), 'device and host model disagree'
        dev_ms, enq = windows(call)
        placement = letterbox_plan((h, w), cfg)[1][0]
        moved = n * (out[0].numel() * out.element_size() + source_bytes(fmt, h, w, placement.tolist()))
        torch_txt, ratio_a = f'{"-":>9} {"":>21} {"-":>6}', None
        if fmt == 'rgb' and dtype == 'fp16':
            left, top, new_w, new_h = placement.tolist()

            def torch_route():
                x = stack.permute(0, 3, 1, 2).float()
                x = F.interpolate(x, size=(new_h, new_w), mode='bilinear', align_corners=False)
                x = F.pad(x, (left, INPUT[1] - new_w - left, top, INPUT[0] - new_h - top), value=114.0)
                return (x / 255).half()
            t_ms, _ = windows(torch_route)
            ratio_a = float(np.median(t_ms)) / float(np.median(dev_ms))
            torch_txt = f'{float(np.median(t_ms)):>9.4f} ({min(t_ms):>8.4f} .. {max(t_ms):>8.4f}) {ratio_a:>6.1f}'
            verdict.append((n, size, fmt, dtype, 'a', float(np.median(dev_ms)), float(np.median(t_ms)), max(max(dev_ms) - min(dev_ms), max(t_ms) - min(t_ms))))
        tap, host_ms = HostLetterbox(cfg), []
        for _ in range(args.host_reps + 1):
            t0 = time.perf_counter()
            torch.cuda.synchronize()
            down = [Frame(f.format, tuple(p.cpu().numpy() for p in f.planes), f.matrix) for f in frames]
            up = torch.from_numpy(tap.letterbox(down)[0]).cuda()
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        host_ms = host_ms[1:]
        dm, hm = float(np.median(dev_ms)), float(np.median(host_ms))
        verdict.append((n, size, fmt, dtype, 'b', dm, hm, 0.0))
        tbs = moved / dm / 1e9
        row = (f'{n:>3} {size:>5} {fmt:>4} {dtype:>4} | {dm:>9.4f} ({min(dev_ms):>8.4f} .. {max(dev_ms):>8.4f}) {enq:>7.4f} {moved / 1e6:>7.1f} {tbs:>6.2f} {tbs / copy_tbs:>7.2f} | '
               f'{torch_txt} | {hm:>9.2f} ({min(host_ms):>8.2f} .. {max(host_ms):>8.2f}) {hm / dm:>8.0f}')
        print(row, flush=True)
        lines.append(row)
        del frames, stack, out, up
        torch.cuda.empty_cache()
    slower_a = [v for v in verdict if v[4] == 'a' and v[5] > v[6] + v[7]]
    slower_b = [v for v in verdict if v[4] == 'b' and v[5] > v[6]]
    tail = [f'# accept: no cell slower than torch (a) by more than the larger spread: {"yes" if not slower_a else "NO " + str(slower_a)}; no cell slower than the host route '
            f'(b): {"yes" if not slower_b else "NO " + str(slower_b)}']

    # what the stage adds in front of detect -> tracker -> infer_boxes(nms=)
    (H, W), n, A, NC = SIZES['1080p'], 64, 8400, 80
    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, uv = rgb_to_nv12(rgb, 'bt709')
    frame = Frame.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), 'bt709')
    boxes = person_boxes(np.random.default_rng(64000), n, H, W)[:, :5]
    gain, pad_x, pad_y = letterbox_params((H, W), INPUT)
    head = np.zeros((1, 4 + NC, A), np.float32)
    head[:, :4] = 10
    head[0, 4:] = np.random.default_rng(3).uniform(0, 0.3, (NC, A))
    for k, b in enumerate(boxes):
        x1, y1, x2, y2 = b[0] * gain + pad_x, b[1] * gain + pad_y, b[2] * gain + pad_x, b[3] * gain + pad_y
        head[0, :4, 100 * k + 50] = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1)
        head[0, 4, 100 * k + 50] = 0.9 - 0.005 * k
    d_head = torch.from_numpy(head.astype(np.float16)).cuda()
    lb, det, nms = eng.letterbox(LetterboxCfg(INPUT)), eng.detector(DetectCfg(nc=NC, dtype='fp16', classes='human')), PoseNms()
    trackers = [eng.tracker(TrackCfg(1, 1, 0.3, 1)) for _ in range(2)]
    lb_out = torch.empty((1, 3) + INPUT, dtype=torch.float16, device='cuda')

    def without():
        rows, image, anchor, count, flags = det.detect(d_head, (H, W), INPUT, n)
        rows, ids, st, _, _ = trackers[0].update(rows, image, n_out=n, n_dets=count[-1:])
        return eng.infer_boxes([frame], rows, st, nms=nms)

    def with_letterbox():
        tensor, table, _ = lb.letterbox([frame], out=lb_out)
        rows, image, anchor, count, flags = det.detect(d_head, table, n_out=n)
        rows, ids, st, _, _ = trackers[1].update(rows, image, n_out=n, n_dets=count[-1:])
        return eng.infer_boxes([frame], rows, st, nms=nms)
    chains = {'detect + counted tracker + infer_boxes(nms=)': without, 'letterbox + detect + counted tracker + infer_boxes(nms=)': with_letterbox}
    for ch in chains.values():
        for _ in range(3):
            ch()
    torch.cuda.synchronize()
    ms = {k: [] for k in chains}
    for _ in range(args.chain_reps):
        for name, ch in chains.items():   # alternating
            t0 = time.perf_counter()
            ch()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    tail.append(f'# added cost: ViTPose-{args.variant.upper()} fp16, {n} boxes on one {W}x{H} NV12 device frame, head [1, {4 + NC}, {A}] fp16, chain + device synchronisation '
                f'(host clock), alternating, {args.chain_reps} each')
    base = float(np.median(ms['detect + counted tracker + infer_boxes(nms=)']))
    for name, v in ms.items():
        m = float(np.median(v))
        tail.append(f'{name:<58} {m:.3f} ms ({min(v):.3f} .. {max(v):.3f})   {m - base:+.3f} ms ({(m / base - 1) * 100:+.2f} %)')
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
