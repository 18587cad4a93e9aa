"""Timing and accuracy figures of the detector network (devyolo.DeviceYolo, vp_yolo_forward_stream); writes profiles/yolo_net.txt.

    python tools/yolo_bench.py [--out profiles/yolo_net.txt] [--scales n s] [--batches 1 8 64]

Part 1 (needs tests/ on the path): per whole-network case of tests/yolo_cases.py, the tolerance (from the oracle alone), the device's deviation from the oracle's
'stored' mode, and 'stored' against 'exact' -- the precision cost of fp16 activations, a result and not a gate.
Part 2: scales n and s at 640 x 640, fp16, batches 1, 8 and 64, against the same folded weights run through torch.nn.functional.conv2d in fp16 on the same GPU
(channels_last; the vendor's convolution route, with torch's SiLU, max_pool2d, interpolate and cat).  After a warm-up, a window is back-to-back calls between two
device events, sized to at least 50 ms; the figure is the median of 7 windows, the spread (max - min) / median.  The vendor route is timed twice: eager (about
150 operators per forward: at small batches that is host launch overhead) and replayed from a captured graph, which is the figure that says something about the
convolution kernels.  Nothing is promised: every cell where the vendor route wins is named.
Part 3: what the stage adds in front of detect -> counted tracker -> infer_boxes(nms=) at 64 boxes (the method of tools/letterbox_bench.py).
--trace SCALE BATCH runs a few forwards only, for a kernel-trace run of its own around this script (tools/yolo_trace_share.py turns its statistics into the
per-layer share)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from easy_vitpose_amd import VitPoseHip  # noqa: E402
from easy_vitpose_amd.configs import model_shape  # noqa: E402
from easy_vitpose_amd.devyolo import DeviceYolo, synth_yolo, yolo_fold, yolo_plan  # noqa: E402
from easy_vitpose_amd.synth import synthetic_state_dict  # noqa: E402


def windows(fn, min_ms=50.0, n_windows=7):
    """median ms per call and spread over n_windows windows of back-to-back calls, each at least min_ms long"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = 1
    while True:
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        if a.elapsed_time(b) >= min_ms or calls >= 1 << 14:
            break
        calls *= 2
    per = []
    for _ in range(n_windows):
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / calls)
    med = float(np.median(per))
    return med, (max(per) - min(per)) / med, calls


class TorchRoute:
    """the same folded fp16 weights through torch's fp16 convolutions (channels_last), float32 Detect outputs left in fp16: decode excluded on both sides' favour
    of the vendor route (it runs torch's softmax / sigmoid on the fp16 levels)"""

    def __init__(self, sd, hw):
        info, launches, _ = yolo_plan(sd, hw)
        self.launches = [l for l in launches if l['kind'] == 'conv']
        self.w = []
        for l in self.launches:
            w, b = yolo_fold(sd, hw, l['conv'])
            k = l['k']
            wt = torch.from_numpy(w.astype(np.float32).reshape(l['c_out'], k, k, l['c_in'])).permute(0, 3, 1, 2).contiguous()
            if not self.w:
                wt = wt[:, :3].contiguous()   # the stem: the three real input channels
            self.w.append((wt.cuda().half().contiguous(memory_format=torch.channels_last), torch.from_numpy(b).cuda().half(), k, l['s'], bool(l['act'])))
        self.i = 0
        self.d = info

    def conv(self, x, c_in=None):
        w, b, k, s, act = self.w[self.i]
        self.i += 1
        y = F.conv2d(x, w, b, stride=s, padding=k // 2)
        return F.silu(y) if act else y

    def c2f(self, x, n, shortcut):
        y = list(self.conv(x).chunk(2, 1))
        for _ in range(n):
            t = self.conv(self.conv(y[-1]))
            y.append(t + y[-1] if shortcut else t)
        return self.conv(torch.cat(y, 1))

    def __call__(self, x):
        self.i = 0
        d3, d6 = self.d['d3'], self.d['d6']
        up = lambda t: F.interpolate(t, scale_factor=2, mode='nearest')   # noqa: E731
        x = self.conv(self.conv(x))
        x = self.c2f(x, d3, True)
        x4 = self.c2f(self.conv(x), d6, True)
        x6 = self.c2f(self.conv(x4), d6, True)
        x = self.c2f(self.conv(x6), d3, True)
        y = [self.conv(x)]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], 5, 1, 2))
        x9 = self.conv(torch.cat(y, 1))
        x12 = self.c2f(torch.cat([up(x9), x6], 1), d3, False)
        x15 = self.c2f(torch.cat([up(x12), x4], 1), d3, False)
        x18 = self.c2f(torch.cat([self.conv(x15), x12], 1), d3, False)
        x21 = self.c2f(torch.cat([self.conv(x18), x9], 1), d3, False)
        out = []
        for f in (x15, x18, x21):
            box = self.conv(self.conv(self.conv(f)))
            cls = self.conv(self.conv(self.conv(f)))
            n = f.shape[0]
            dist = (box.reshape(n, 4, 16, -1).float().softmax(2) * torch.arange(16, device=f.device, dtype=torch.float32).view(1, 1, 16, 1)).sum(2)
            out.append(torch.cat([dist, cls.reshape(n, cls.shape[1], -1).float().sigmoid()], 1))
        return torch.cat(out, 2)


def added_cost(args):
    """what the stage adds in front of detect -> counted tracker -> infer_boxes(nms=): ViTPose-B fp16, 64 boxes on one 1920 x 1080 NV12 device frame.  Both chains
    feed the detector stage the same planted head (64 persons), so the work behind the network is the same; the second chain runs letterbox -> network first."""
    import time
    from easy_vitpose_amd.cropprep import Frame, rgb_to_nv12
    from easy_vitpose_amd.devdetect import DetectCfg, letterbox_params
    from easy_vitpose_amd.devletterbox import LetterboxCfg
    from easy_vitpose_amd.devtracker import TrackCfg
    from easy_vitpose_amd.posenms import PoseNms
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from frames_bench import person_boxes
    shp = model_shape('b', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=64)
    (H, W), n, A, NC, INPUT = (1080, 1920), 64, 8400, 80, (640, 640)
    rgb = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
    yp, uv = rgb_to_nv12(rgb, 'bt709')
    frame = Frame.nv12(torch.from_numpy(yp).cuda(), torch.from_numpy(uv).cuda(), 'bt709')
    boxes = person_boxes(np.random.default_rng(64000), n, H, W)[:, :5]
    gain, pad_x, pad_y = letterbox_params((H, W), INPUT)
    head = np.zeros((1, 4 + NC, A), np.float32)
    head[:, :4] = 10
    head[0, 4:] = np.random.default_rng(3).uniform(0, 0.3, (NC, A))
    for k, b in enumerate(boxes):
        x1, y1, x2, y2 = b[0] * gain + pad_x, b[1] * gain + pad_y, b[2] * gain + pad_x, b[3] * gain + pad_y
        head[0, :4, 100 * k + 50] = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1)
        head[0, 4, 100 * k + 50] = 0.9 - 0.005 * k
    d_head = torch.from_numpy(head).cuda()
    lb, det, nms = eng.letterbox(LetterboxCfg(INPUT)), eng.detector(DetectCfg(nc=NC, dtype='fp32', classes='human')), PoseNms()
    trackers = [eng.tracker(TrackCfg(1, 1, 0.3, 1)) for _ in range(3)]
    lb_out = torch.empty((1, 3) + INPUT, dtype=torch.float16, device='cuda')
    nets = {sc: DeviceYolo(eng, synth_yolo(sc, NC, 0), INPUT) for sc in args.scales}

    def behind(t, table=None):
        rows, image, anchor, count, flags = det.detect(d_head, (H, W), INPUT, n) if table is None else det.detect(d_head, table, n_out=n)
        rows, ids, st, _, _ = trackers[t].update(rows, image, n_out=n, n_dets=count[-1:])
        return eng.infer_boxes([frame], rows, st, nms=nms)

    def with_net(t, net):
        tensor, table, _ = lb.letterbox([frame], out=lb_out)
        net(tensor)
        return behind(t, table)
    chains = {'detect + counted tracker + infer_boxes(nms=)': lambda: behind(0)}
    for i, (sc, net) in enumerate(nets.items()):
        chains[f'letterbox + network {sc} + detect + counted tracker + infer_boxes(nms=)'] = lambda i=i, net=net: with_net(1 + i, net)
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
    out = ['', f'## added cost: ViTPose-B fp16, {n} boxes on one {W}x{H} NV12 device frame, chain + device synchronisation (host clock), alternating, {args.chain_reps} each']
    base = float(np.median(ms['detect + counted tracker + infer_boxes(nms=)']))
    for name, v in ms.items():
        m = float(np.median(v))
        out.append(f'{name:<72} {m:.3f} ms ({min(v):.3f} .. {max(v):.3f})   {m - base:+.3f} ms ({(m / base - 1) * 100:+.2f} %)')
    for t in trackers:
        t.close()
    for net in nets.values():
        net.close()
    det.close()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'yolo_net.txt'))
    ap.add_argument('--scales', nargs='+', default=['n', 's'])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 64])
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--trace', nargs=2, metavar=('SCALE', 'BATCH'), default=None)
    ap.add_argument('--chain-reps', type=int, default=15)
    args = ap.parse_args()
    if args.trace:
        shp = model_shape('s', 'coco')
        eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype='fp16', max_batch=4)
        n = int(args.trace[1])
        y = DeviceYolo(eng, synth_yolo(args.trace[0], 80, 0), (args.size, args.size), max_images=n)
        x = torch.rand((n, 3, args.size, args.size), device='cuda').half()
        for _ in range(10):
            y(x)
        torch.cuda.synchronize()
        y.close()
        eng.close()
        return
    lines = ['# the detector network on the device: tools/yolo_bench.py on ' + torch.cuda.get_device_name(0), '']
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype='fp16', max_batch=4)

    import yolo_cases as YC
    lines += ['## accuracy: tolerance (2 x the largest deviation of 8 perturbed stored runs, from the oracle alone) | the device against stored | stored against exact',
              f'{"case":<12} {"tol box px":>11} {"dev box px":>11} {"exact box px":>13} {"tol score":>10} {"dev score":>10} {"exact score":>12}']
    for name, (_, _, hw, n, _) in YC.CASES.items():
        y = DeviceYolo(eng, YC.state(name), hw, max_images=n)
        head = y(torch.from_numpy(YC.images(name)).cuda()).cpu().numpy()
        y.close()
        dev, cost, tol = YC.deviation(head, YC.oracle_head(name)), YC.deviation(YC.oracle_head(name), YC.oracle_head(name, 'exact')), YC.tolerance(name)
        lines.append(f'{name:<12} {tol[0]:>11.4g} {dev[0]:>11.4g} {cost[0]:>13.4g} {tol[1]:>10.4g} {dev[1]:>10.4g} {cost[1]:>12.4g}')
    lines += ['', f'## time per forward, {args.size} x {args.size}, fp16, ms (median of 7 windows of >= 50 ms; spread = (max - min) / median)',
              f'{"scale":<6} {"batch":>5} {"native ms":>10} {"spread":>7} {"img/s":>9} {"torch eager ms":>16} {"spread":>7} {"torch graph ms":>15} {"spread":>7} {"native / graph":>15}']
    losses = []
    for scale in args.scales:
        sd = synth_yolo(scale, 80, 0)
        ref = TorchRoute(sd, (args.size, args.size))
        for n in args.batches:
            y = DeviceYolo(eng, sd, (args.size, args.size), max_images=n)
            x = torch.rand((n, 3, args.size, args.size), device='cuda').half()
            xl = x.contiguous(memory_format=torch.channels_last)
            t, sp, _ = windows(lambda: y(x))
            with torch.no_grad():
                tr, spr, _ = windows(lambda: ref(xl))
                tg, spg = float('nan'), float('nan')
                try:   # the same route replayed from a captured graph: no host launch cost
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        for _ in range(3):
                            ref(xl)
                    torch.cuda.current_stream().wait_stream(side)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        ref(xl)
                    tg, spg, _ = windows(g.replay)
                    del g
                except Exception as e:   # reported, not hidden
                    print(f'graph capture of the torch route failed at {scale} x {n}: {e}', flush=True)
            y.close()
            lines.append(f'{scale:<6} {n:>5} {t:>10.4f} {sp:>7.1%} {n / t * 1e3:>9.0f} {tr:>16.4f} {spr:>7.1%} {tg:>15.4f} {spg:>7.1%} {t / tg:>15.2f}')
            if not t <= min(tr, tg):
                losses.append(f'{scale} x {n}')
            print(lines[-1], flush=True)
    lines += ['', 'cells where the vendor route (eager or graph) wins: ' + (', '.join(losses) if losses else 'none')]
    eng.close()
    lines += added_cost(args)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
