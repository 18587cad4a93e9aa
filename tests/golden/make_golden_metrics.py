#!/usr/bin/env python
"""Generate tests/golden/metrics.npz by running THE REFERENCE's vit_utils/top_down_eval.py and post_processing/nms.py oks_iou in the build container.

    python tests/golden/make_golden_metrics.py

Like make_golden.py it runs only where the reference tree exists (it imports it by that file's recipe) and copies nothing from it: the fixture holds seeded
synthetic inputs and the reference's numerical OUTPUTS.

Two data sets, 700 x 17 and 130 x 133 rows of (y, x, v) float32: ground truth on a quarter-pixel grid, predictions = ground truth + float32 noise of 0.5 to 40 px
per row, about 20 % of the joints masked (v = 0) and one joint masked in every row, float32 normalisers (h, w) with rows that hold a zero and rows that hold a
negative component, areas h * w.  Stored per data set: _calc_distances (transposed to [n, K]), keypoint_pck_accuracy at thr 0.05 / 0.1 / 0.2 / 0.5 (acc, avg,
cnt), keypoint_auc (normalize 30, 20 steps), keypoint_epe, keypoint_nme (the pixel distances behind keypoint_epe are not stored: the test forms them from the stored
rows with the reference's own expression), and per row oks_iou(g, d[None], a, [a], sigmas, vis_thr=None) on the visible joints only
(-1 for a row without one); COCO-17 sigmas for K = 17, 0.05 for K = 133.

The generator asserts ON THE REFERENCE ALONE that no OKS lies within 1e-4 of a threshold in use (0.50, 0.55, ..., 0.95) and moves on to the next seed otherwise;
it never drops an element.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
OUT = os.path.join(HERE, 'metrics.npz')

from easy_vitpose_amd.posenms import COCO17_SIGMAS  # noqa: E402

SETS = [(700, 17), (130, 133)]
PCK_THRS = (0.05, 0.1, 0.2, 0.5)
AUC_NORM, AUC_STEPS = 30, 20
OKS_THRS = [np.float32(0.5 + 0.05 * t) for t in range(10)]


def import_reference():
    import make_golden as mg
    if not os.path.isdir(mg.REF):
        raise SystemExit(f'{mg.REF} not found: the goldens are generated where the reference tree exists')
    mg._install_stubs()
    sys.path.insert(0, mg.REF)
    import warnings
    warnings.simplefilter('ignore')
    from easy_ViTPose.vit_utils import top_down_eval as tde
    from easy_ViTPose.vit_utils.post_processing import nms as ref_nms
    return tde, ref_nms


def sigmas_for(K):
    return np.asarray(COCO17_SIGMAS, dtype=np.float32) if K == 17 else np.full(K, 0.05, dtype=np.float32)


def make_set(rng, n, K):
    h, w = rng.integers(80, 400, n).astype(np.float32), rng.integers(40, 250, n).astype(np.float32)
    gt = np.zeros((n, K, 3), np.float32)
    gt[:, :, 0] = np.round(rng.uniform(0, 1, (n, K)) * h[:, None] * 4) / 4
    gt[:, :, 1] = np.round(rng.uniform(0, 1, (n, K)) * w[:, None] * 4) / 4
    gt[:, :, 2] = np.where(rng.random((n, K)) < 0.2, 0, rng.integers(1, 3, (n, K))).astype(np.float32)
    gt[:, K // 3, 2] = 0                                  # a joint masked in every row
    scale = rng.choice([0.5, 3.0, 10.0, 40.0], n).astype(np.float32)
    pred = np.zeros_like(gt)
    pred[:, :, :2] = gt[:, :, :2] + (rng.standard_normal((n, K, 2)) * scale[:, None, None]).astype(np.float32)
    pred[:, :, 2] = 1                                     # no metric reads a prediction's confidence
    norm = np.stack([h, w], axis=1).astype(np.float32)
    special = rng.permutation(n)[:12]
    norm[special[0:3], 0] = 0                             # a zero component: the row is off for PCK / NME
    norm[special[3:6], 1] = 0
    norm[special[6:9], 0] = -norm[special[6:9], 0]        # a negative component becomes 1e6
    norm[special[9:12], 1] = -3
    area = (h * w).astype(np.float32)
    return pred, gt, norm, area


def run_set(tde, ref_nms, pred, gt, norm, area, sig32):
    n, K = pred.shape[:2]
    p2, g2 = np.ascontiguousarray(pred[:, :, :2]), np.ascontiguousarray(gt[:, :, :2])
    mask = gt[:, :, 2] > np.float32(0)
    out = {'dist': np.ascontiguousarray(tde._calc_distances(p2.copy(), g2.copy(), mask.copy(), norm.copy()).T)}
    for i, thr in enumerate(PCK_THRS):
        acc, avg, cnt = tde.keypoint_pck_accuracy(p2.copy(), g2.copy(), mask.copy(), thr, norm.copy())
        out[f'pck{i}_acc'], out[f'pck{i}_avg'], out[f'pck{i}_cnt'] = np.asarray(acc, np.float64), np.float64(avg), np.int64(cnt)
    out['auc'] = np.float64(tde.keypoint_auc(p2.copy(), g2.copy(), mask.copy(), AUC_NORM, AUC_STEPS))
    epe, nme = tde.keypoint_epe(p2.copy(), g2.copy(), mask.copy()), tde.keypoint_nme(p2.copy(), g2.copy(), mask.copy(), norm.copy())
    assert isinstance(epe, np.float32) and isinstance(nme, np.float32), 'the reference sums its float32 distance array'
    out['epe'], out['nme'] = epe, nme
    sig64 = sig32.astype(np.float64)
    oks = np.full(n, -1, np.float32)
    for i in range(n):
        v = mask[i]
        if not v.any():
            continue
        a = float(area[i])
        oks[i] = ref_nms.oks_iou(gt[i, v].reshape(-1), pred[i, v].reshape(1, -1), a, [a], sig64[v], None)[0]
    have = oks[oks >= 0]
    for t in OKS_THRS:
        if (np.abs(have - t) < 1e-4).any():
            return None
    out['oks'] = oks
    return out


def main():
    tde, ref_nms = import_reference()
    out = {'sets': np.array(SETS, np.int32), 'pck_thrs': np.array(PCK_THRS, np.float64), 'auc_norm': np.int64(AUC_NORM), 'auc_steps': np.int64(AUC_STEPS)}
    for n, K in SETS:
        seed = 7000 * K + n
        while True:
            pred, gt, norm, area = make_set(np.random.default_rng(seed), n, K)
            res = run_set(tde, ref_nms, pred, gt, norm, area, sigmas_for(K))
            if res is not None:
                break
            print(f'n={n} K={K} seed {seed}: an OKS within 1e-4 of a threshold; next seed')
            seed += 100000
        tag = f'k{K}'
        out[f'{tag}_pred'], out[f'{tag}_gt'], out[f'{tag}_norm'], out[f'{tag}_area'], out[f'{tag}_sigmas'], out[f'{tag}_seed'] = pred, gt, norm, area, sigmas_for(K), np.int64(seed)
        for k, v in res.items():
            out[f'{tag}_{k}'] = v
        print(f'n={n} K={K}: seed {seed}, pck avg {[float(res[f"pck{i}_avg"]) for i in range(4)]}, auc {float(res["auc"]):.4f}, epe {float(res["epe"]):.4f}, '
              f'nme {float(res["nme"]):.5f}, oks rows {(res["oks"] >= 0).sum()}, mean {res["oks"][res["oks"] >= 0].mean():.4f}')
    np.savez_compressed(OUT, **out)
    print(f'{OUT}: {os.path.getsize(OUT)} bytes, numpy {np.__version__}')


if __name__ == '__main__':
    main()
