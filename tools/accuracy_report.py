#!/usr/bin/env python3
"""Accuracy of the inference modes as metrics, on the device: PCK@0.05 / 0.1 / 0.2, AUC, EPE and OKS recall of fp16, fp16 + flip-test and fp8 against the
reference's keypoints, for the BASELINE models whose goldens exist (tests/golden/full_*.npz: the peaked checkpoint at each configuration's own batch size;
full_content_*.npz: the content-dependent checkpoint, 64 crops).

The crops are the seeded ones the parity tests build (tests/golden/cases.py); they go through `infer_device` and the keypoints, still on the GPU, through
`VitPoseHip.metrics`.  Ground truth = the fixture's `keypoints` (what the reference produced crop by crop), a joint visible when its confidence column is above
vis_thr = 0.2 (the reference's data_cfg), norm = the crop's (h, w) = (256, 192), AUC normaliser 30 px over 20 steps, OKS area = 256 x 192 with the COCO-17
sigmas for the 17-joint COCO models and 0.05 for every other layout (as tests/golden/make_golden_metrics.py).  Flip-test needs the dataset's mirror pairs; the
project carries the COCO-17 table only, so the mode is reported for the coco models.  No threshold is attached to any figure.

    python tools/accuracy_report.py [--out profiles/accuracy_modes.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import cases
    from easy_vitpose_amd import _capi as capi
    from easy_vitpose_amd.configs import COCO17_FLIP_PAIRS, model_shape
    from easy_vitpose_amd.devmetrics import MetricsCfg
    from easy_vitpose_amd.engine import VitPoseHip
    from easy_vitpose_amd.synth import synthetic_state_dict
    assert torch.cuda.is_available(), 'accuracy_report runs on a GPU'
    lines = ['# accuracy_report: inference modes against the reference\'s keypoints, metrics accumulated on the device (one MI355X, product library)',
             '# gt = the golden\'s keypoints, visible when conf > 0.2; norm = (256, 192); AUC: 30 px, 20 steps; OKS: area 256 x 192, one candidate per instance (not COCO AP)',
             '# flip-test rows: the ground truth is the reference\'s keypoints WITHOUT flip-test, and the synthetic checkpoints are not mirror-equivariant (their peak',
             '# positions come from pos_embed or from the colour blobs of the crop), so the average with the mirrored pass moves the arg-max: these rows measure that',
             '# distance, not an error of the mode (its parity is pinned against the oracle doing the same: tests/test_gpu_parity.py)',
             '| golden | model | crops | mode | PCK@0.05 | PCK@0.1 | PCK@0.2 | AUC | EPE px | NME | OKS mean | OKS recall@0.5 | @0.75 | @0.95 | joints |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    jobs = [('full', v, d, n) for v, d, n in cases.fullbatch_plan()] + [('content', v, d, n) for v, d, n in cases.content_plan()]
    for kind, variant, dataset, n in jobs:
        path = os.path.join(GOLDEN, f'full_{variant}_{dataset}_{n}.npz' if kind == 'full' else f'full_content_{variant}_{dataset}.npz')
        if not os.path.exists(path):
            continue
        gt_np = np.ascontiguousarray(np.load(path)['keypoints'], dtype=np.float32)
        if kind == 'full':
            shp = model_shape(variant, dataset)
            sd, crops = synthetic_state_dict(shp, 0, peaked=True), cases.fullbatch_crops(n)
        else:
            (shp, sd), crops = cases.content_state_dict(variant, dataset), cases.content_crops(n)[0]
        K = shp.num_keypoints
        coco = dataset == 'coco' and K == 17
        cfg = MetricsCfg(n_joints=K, vis_thr=0.2, sigmas='coco' if coco else (0.05,) * K)
        d_crops = torch.from_numpy(np.ascontiguousarray(crops)).cuda()
        gt = torch.from_numpy(gt_np).cuda()
        norm = torch.tensor([[256.0, 192.0]], dtype=torch.float32, device='cuda').repeat(n, 1).contiguous()
        area = torch.full((n,), 256.0 * 192.0, dtype=torch.float32, device='cuda')
        for mode in ('fp16', 'fp16 + flip-test', 'fp8'):
            head = f'| {kind} | {variant}/{dataset} | {n} | {mode} |'
            if mode == 'fp16 + flip-test' and not coco:
                lines.append(head + ' no mirror-pair table for this layout in the project |' + ' |' * 10)
                continue
            try:
                eng = VitPoseHip(shp, sd, dtype='fp8' if mode == 'fp8' else 'fp16', device_id=0, max_batch=n)
            except capi.VpError as e:
                lines.append(head + f' refused: {e.msg} |' + ' |' * 10)
                continue
            if 'flip' in mode:
                eng.set_flip_test(COCO17_FLIP_PAIRS)
            ev = eng.metrics(cfg)
            kp = torch.empty((n, K, 3), dtype=torch.float32, device='cuda')
            eng.infer_device(d_crops, kp, sync=False)
            ev.update(kp, gt, norm=norm, area=area)
            r = ev.result()
            ev.close()
            eng.close()
            lines.append(head + f' {r.pck(0)[1]:.4f} | {r.pck(1)[1]:.4f} | {r.pck(2)[1]:.4f} | {r.auc:.4f} | {r.epe:.4f} | {r.nme:.6f} | {r.oks_mean:.4f} | '
                         f'{r.oks_recall[0]:.4f} | {r.oks_recall[5]:.4f} | {r.oks_recall[9]:.4f} | {int(r.state["valid_px"].sum())} |')
            print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
