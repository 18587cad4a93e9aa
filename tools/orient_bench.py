#!/usr/bin/env python3
"""The orient stage on the device (vp_orient_stream) against the two routes a caller had before it, what it moves, and what it adds in front of the chain.

Workload: seeded 1920x1080 frames on the device, NV12 (bt709) and RGB24, 1 and 64 frames per call, codes 1 (copy), 3 (180 degrees), 6 and 8 (the quarter turns),
source and destination at their tight pitches and at the next multiple of 256 bytes.

    device   vp_orient_stream itself (ctypes, destination allocated once): back-to-back calls between two device events, as many as fill --window-ms (at least
             --calls), ms per call; median and min .. max of --reps windows.  `enq` = host ms inside one call, no synchronisation.
    bytes    the row bytes of every source and destination plane (one read and one write of the frame); TB/s = bytes over the device median; `of copy` = that over
             the float4 copy rate tools/peak.py measures in a child process of the same run (read + write bytes per second)
    torch    (a) the same result made with PyTorch on the device, per plane of the stacked frames: .clone() / torch.flip(dims (1, 2)) / torch.rot90(k, (1, 2))
             .contiguous(); windows of the two routes ALTERNATE within a repetition, same events
    host     (b) the route without the entry, host clock, tight pitches only: synchronise, download the planes, np.rot90 / slices + ascontiguousarray, upload,
             synchronise; median and min .. max of --host-reps routes after 1 warm-up route
    added    orient -> letterbox -> detect -> counted tracker -> infer_boxes(nms=) against that chain on the upright frame, ViTPose-B fp16, 64 boxes on one
             1080 x 1920 NV12 device frame (captured as 1920 x 1080, code 6), alternating, each chain followed by a device synchronisation (host clock)

    python tools/orient_bench.py [--reps 7] [--window-ms 30] [--host-reps 3] [--out profiles/orient.txt]
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

H, W = 1080, 1920
INPUT = (640, 640)


def copy_rate_tbs():
    """the float4 copy rate of tools/peak.py (TB/s, read + write), measured by a child process of this run before this process opens the device"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'peak.py')], capture_output=True, text=True, timeout=600)
    m = re.search(r'float4 copy read\+write \(TB/s\): ([0-9.]+) rc=0', r.stdout)
    if not m:
        raise RuntimeError(f'tools/peak.py gave no copy rate:\n{r.stdout}\n{r.stderr}')
    return float(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=8)
    ap.add_argument('--window-ms', type=float, default=30.0)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--chain-reps', type=int, default=12)
    ap.add_argument('--variant', default='b')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    copy_tbs = copy_rate_tbs()

    import torch
    from easy_vitpose_amd import _capi as capi
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.cropprep import Frame, rgb_to_nv12
    from easy_vitpose_amd.devdetect import DetectCfg, letterbox_params
    from easy_vitpose_amd.devletterbox import LetterboxCfg, image_table
    from easy_vitpose_amd.devorient import HostOrient, oriented_hw
    from easy_vitpose_amd.devtracker import TrackCfg
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.posenms import PoseNms
    from easy_vitpose_amd.synth import synthetic_state_dict
    from frames_bench import person_boxes
    assert torch.cuda.is_available(), 'orient_bench measures on a GPU'

    shp = model_shape(args.variant, 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=64)
    lib = eng.lib
    stream = torch.cuda.current_stream().cuda_stream

    def pitched_stack(n, rows, row_bytes, inner, aligned):
        """a uint8 device tensor [n, rows, ...] whose rows lie `pitch` bytes apart: tight, or the next multiple of 256"""
        pitch = (row_bytes + 255) // 256 * 256 if aligned else row_bytes
        flat = torch.zeros((n, rows, pitch), dtype=torch.uint8, device='cuda')
        shape = (n, rows) + inner
        return torch.as_strided(flat, shape, (rows * pitch, pitch) + ((inner[1], 1) if len(inner) == 2 else (1,)))

    def planes(fmt, n, h, w, aligned):
        if fmt == 'rgb':
            return [pitched_stack(n, h, 3 * w, (w, 3), aligned)]
        return [pitched_stack(n, h, w, (w,), aligned), pitched_stack(n, h // 2, w, (w // 2, 2), aligned)]

    def frames_of(fmt, stacks, n):
        return [Frame.rgb(stacks[0][i]) if fmt == 'rgb' else Frame.nv12(stacks[0][i], stacks[1][i], 'bt709') for i in range(n)]

    rng = np.random.default_rng(H)
    base = rng.integers(0, 256, (8, H, W, 3), dtype=np.uint8)
    base_nv = [rgb_to_nv12(f, 'bt709') for f in base[:2]]

    def fill(fmt, stacks, n):
        for i in range(n):
            if fmt == 'rgb':
                stacks[0][i].copy_(torch.from_numpy(base[i % 8]).cuda() + (i // 8))
            else:
                stacks[0][i].copy_(torch.from_numpy(base_nv[i % 2][0]).cuda() + i)
                stacks[1][i].copy_(torch.from_numpy(base_nv[i % 2][1]).cuda() + i)

    def calls_per_window(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        call()
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.calls):
            call()
        b.record()
        b.synchronize()
        return max(args.calls, int(np.ceil(args.window_ms / max(a.elapsed_time(b) / args.calls, 1e-4))))

    def windows(routes):
        """{name: call} -> {name: (ms per call of every window, median host ms inside a call)}; the routes alternate within a repetition"""
        counts = {k: calls_per_window(c) for k, c in routes.items()}
        ms, enq = {k: [] for k in routes}, {k: [] for k in routes}
        for _ in range(args.reps):
            for k, call in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                t0 = time.perf_counter()
                for _ in range(counts[k]):
                    call()
                enq[k].append((time.perf_counter() - t0) * 1e3 / counts[k])
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b) / counts[k])
        return {k: (ms[k], float(np.median(enq[k]))) for k in routes}

    def torch_route(stacks, code):
        if code == 1:
            return [s.clone(memory_format=torch.contiguous_format) for s in stacks]
        if code == 3:
            return [torch.flip(s, (1, 2)) for s in stacks]
        return [torch.rot90(s, -1 if code == 6 else 1, (1, 2)).contiguous() for s in stacks]

    def numpy_route(a, code):
        return np.ascontiguousarray({1: lambda: a, 3: lambda: a[::-1, ::-1], 6: lambda: np.rot90(a, -1), 8: lambda: np.rot90(a, 1)}[code]())

    lines = [f'# orient_bench: vp_orient_stream between two device events, windows of >= {args.window_ms:g} ms and >= {args.calls} back-to-back calls, ms per call: median '
             f'(min .. max) of {args.reps} windows; enq = host ms inside one call, no synchronisation.  {W}x{H} frames.',
             f'# MB = row bytes of every source and destination plane; TB/s = MB / device median; of copy = TB/s over the float4 copy rate of tools/peak.py in this run: '
             f'{copy_tbs:.1f} TB/s (read + write).',
             '# torch (a): clone / torch.flip / torch.rot90(...).contiguous() per plane of the stacked frames, windows alternating with the device route; a/dev = torch median / '
             'device median.',
             f'# host (b), host clock, tight pitches: sync, plane download, numpy slices + ascontiguousarray, upload, sync: median (min .. max) of {args.host_reps} after 1 warm-up.',
             '# kernel: a workgroup of 256 threads per 64 x 64-element tile of a destination plane, a lane per four destination bytes (16-byte pieces for a run that keeps its byte order, three permuted words for four reversed RGB pixels); codes 5..8 through a padded LDS tile '
             '(12.25 KiB); 18 VGPRs, 8 waves per SIMD, no scratch (hipcc -Rpass-analysis=kernel-resource-usage).',
             f'{"n":>3} {"fmt":>4} {"code":>4} {"pitch":>6} | {"device ms":>9} {"(min .. max)":>21} {"enq":>7} {"MB":>7} {"TB/s":>6} {"of copy":>7} | {"torch ms":>9} {"(min .. max)":>21} '
             f'{"a/dev":>6} | {"host ms":>9} {"(min .. max)":>21} {"b/dev":>8}']
    print('\n'.join(lines), flush=True)
    slower = []
    for n in (1, 64):
        for fmt in ('nv12', 'rgb'):
            for aligned in (False, True):
                src = planes(fmt, n, H, W, aligned)
                fill(fmt, src, n)
                frames = frames_of(fmt, src, n)
                for code in (1, 3, 6, 8):
                    oh, ow = oriented_hw((H, W), code)
                    dst = planes(fmt, n, oh, ow, aligned)
                    out = frames_of(fmt, dst, n)
                    s_tab, d_tab, codes = image_table(frames), image_table(out), np.full(n, code, np.int32)
                    sp, dp = C.cast(s_tab.ctypes.data, C.POINTER(capi.vp_image)), C.cast(d_tab.ctypes.data, C.POINTER(capi.vp_image))

                    def call():
                        capi.check(lib.vp_orient_stream(eng._h, sp, codes.ctypes.data, dp, n, stream), eng._h)
                    call()
                    torch.cuda.synchronize()
                    want = HostOrient().orient([Frame(f.format, tuple(np.ascontiguousarray(p.cpu().numpy()) for p in f.planes), f.matrix) for f in frames[:1]], code)[0]
                    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(out[0].planes, want.planes)), 'device and host model disagree'
                    ref = torch_route(src, code)
                    assert all(torch.equal(r, d) for r, d in zip(ref, dst)), 'the torch route gives other bytes'
                    del ref
                    res = windows({'dev': call, 'torch': lambda: torch_route(src, code)})
                    (dev_ms, enq), (t_ms, _) = res['dev'], res['torch']
                    dm, tm = float(np.median(dev_ms)), float(np.median(t_ms))
                    moved = 2 * n * (H * W * 3 if fmt == 'rgb' else H * W * 3 // 2)
                    host_txt = f'{"-":>9} {"":>21} {"-":>8}'
                    if not aligned:
                        host_ms = []
                        for _ in range(args.host_reps + 1):
                            t0 = time.perf_counter()
                            torch.cuda.synchronize()
                            up = [torch.from_numpy(np.stack([numpy_route(a, code) for a in s.cpu().numpy()])).cuda() for s in src]
                            torch.cuda.synchronize()
                            host_ms.append((time.perf_counter() - t0) * 1e3)
                        del up
                        host_ms = host_ms[1:]
                        hm = float(np.median(host_ms))
                        host_txt = f'{hm:>9.2f} ({min(host_ms):>8.2f} .. {max(host_ms):>8.2f}) {hm / dm:>8.0f}'
                    if dm > tm + max(max(dev_ms) - min(dev_ms), max(t_ms) - min(t_ms)):
                        slower.append((n, fmt, code, 'a256' if aligned else 'tight', round(dm, 4), round(tm, 4)))
                    tbs = moved / dm / 1e9
                    row = (f'{n:>3} {fmt:>4} {code:>4} {"a256" if aligned else "tight":>6} | {dm:>9.4f} ({min(dev_ms):>8.4f} .. {max(dev_ms):>8.4f}) {enq:>7.4f} {moved / 1e6:>7.1f} {tbs:>6.2f} '
                           f'{tbs / copy_tbs:>7.2f} | {tm:>9.4f} ({min(t_ms):>8.4f} .. {max(t_ms):>8.4f}) {tm / dm:>6.2f} | {host_txt}')
                    print(row, flush=True)
                    lines.append(row)
                    del dst, out
                    torch.cuda.empty_cache()
                del src, frames
                torch.cuda.empty_cache()
    tail = [f'# cells slower than the torch route (a) by more than the larger spread: {"none" if not slower else slower}']

    # what the stage adds in front of letterbox -> detect -> tracker -> infer_boxes(nms=)
    n, A, NC = 64, 8400, 80
    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, uv = rgb_to_nv12(rgb, 'bt709')
    upright = Frame.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), 'bt709')
    captured = Frame.nv12(torch.from_numpy(np.ascontiguousarray(np.rot90(y, 1))).cuda(), torch.from_numpy(np.ascontiguousarray(np.rot90(uv, 1))).cuda(), 'bt709')   # code 6 undoes it
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
    ori, lb, det, nms = eng.orient(), eng.letterbox(LetterboxCfg(INPUT)), eng.detector(DetectCfg(nc=NC, dtype='fp16', classes='human')), PoseNms()
    trackers = [eng.tracker(TrackCfg(1, 1, 0.3, 1)) for _ in range(2)]
    lb_out = torch.empty((1, 3) + INPUT, dtype=torch.float16, device='cuda')
    turned = [Frame.nv12(torch.empty_like(upright.planes[0]), torch.empty_like(upright.planes[1]), 'bt709')]

    def chain(frame, trk):
        tensor, table, _ = lb.letterbox([frame], out=lb_out)
        rows, image, anchor, count, flags = det.detect(d_head, table, n_out=n)
        rows, ids, st, _, _ = trk.update(rows, image, n_out=n, n_dets=count[-1:])
        return eng.infer_boxes([frame], rows, st, nms=nms)

    def without():
        return chain(upright, trackers[0])

    def with_orient():
        return chain(ori.orient([captured], 6, out=turned)[0], trackers[1])
    a, b = without(), with_orient()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(turned[0].planes, upright.planes)) and all(torch.equal(p, q) for p, q in zip(a, b)), 'the two chains differ'
    chains = {'letterbox + detect + counted tracker + infer_boxes(nms=)': without, 'orient + letterbox + detect + counted tracker + infer_boxes(nms=)': with_orient}
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
    tail.append(f'# added cost: ViTPose-{args.variant.upper()} fp16, {n} boxes on one {W}x{H} NV12 device frame (captured {H}x{W}, code 6), head [1, {4 + NC}, {A}] fp16, chain + device '
                f'synchronisation (host clock), alternating, {args.chain_reps} each')
    base_ms = float(np.median(ms['letterbox + detect + counted tracker + infer_boxes(nms=)']))
    for name, v in ms.items():
        m = float(np.median(v))
        tail.append(f'{name:<67} {m:.3f} ms ({min(v):.3f} .. {max(v):.3f})   {m - base_ms:+.3f} ms ({(m / base_ms - 1) * 100:+.2f} %)')
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
