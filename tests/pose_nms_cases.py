"""Shared by tests/test_pose_nms_host.py (CPU) and tests/test_gpu_pose_nms.py: the goldens of tests/golden/pose_nms.npz (the reference's
nms.py on seeded people, make_golden_pose_nms.py), the edge cases by construction, and thin callers of the four C entries."""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.posenms import COCO17_SIGMAS, PoseNms, c_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pose_nms.npz')
EPS = 2.0 ** -23


@functools.lru_cache(maxsize=1)
def golden():
    return np.load(GOLDEN)


def golden_cases():
    """(K, n, ti, vi) for every recorded combination"""
    return [(int(k), int(n), ti, vi) for k, n in golden()['cases'] for ti in range(2) for vi in range(2)]


def golden_case(K, n, ti, vi):
    g = golden()
    tag = f'k{K}_n{n}'
    vis = None if vi == 1 else float(g['vis'][0])
    return dict(kpts=g[f'{tag}_kpts'], box=g[f'{tag}_box'], p9=g[f'{tag}_p9'], n_frames=int(g[f'{tag}_frames']), sigmas=g[f'{tag}_sigmas'],
                thr=float(g['thrs'][ti]), vis=vis, max_dets=int(g['max_dets']), score=g[f'{tag}_v{vi}_score'], oks=g[f'{tag}_v{vi}_oks'],
                hard_rank=g[f'{tag}_t{ti}_v{vi}_hard_rank'], soft_rank=g[f'{tag}_t{ti}_v{vi}_soft_rank'], soft_score=g[f'{tag}_t{ti}_v{vi}_soft_score'])


def ulp_diff(a, b):
    """distance in float32 steps between two arrays of finite non-negative float32 values"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def soft_bound(rank, thr):
    """relative bound of a soft pick's score against the reference: the reference's float32 overlap**2 / thr and float32 exp per rescoring step,
    (2 + 2 / oks_thr) * 2^-23 per pick in front of it"""
    return (2.0 + 2.0 / thr) * EPS * np.maximum(rank, 0)


def nms_host(kpts, box, p9, n_frames, cfg: PoseNms, sigmas, status=None, score_stride=1, raw=False):
    """vp_dbg_pose_nms_host -- csrc/posenms.h on the host, the model the device entry is tested against (needs no device); raw=True returns the status code
    instead of raising"""
    lib = capi.load_library()
    kp = np.ascontiguousarray(kpts, np.float32)
    n, K = kp.shape[0], kp.shape[1]
    bs, p = np.ascontiguousarray(box, np.float32), np.ascontiguousarray(p9, np.int32)
    st = None if status is None else np.ascontiguousarray(status, np.int32)
    c, keep = c_config(cfg, sigmas)
    score, rank, count = np.full(n, np.nan, np.float32), np.full(n, -99, np.int32), np.full(max(n_frames, 0), -99, np.int32)
    rc = lib.vp_dbg_pose_nms_host(kp.ctypes.data, n, K, bs.ctypes.data, score_stride, p.ctypes.data, None if st is None else st.ctypes.data, n_frames,
                                  C.byref(c), score.ctypes.data, rank.ctypes.data, count.ctypes.data)
    if raw:
        return rc
    capi.check(rc)
    return score, rank, count


def oks_tap(device_id, kpts, p9, cfg: PoseNms, sigmas):
    lib = capi.load_library()
    kp = np.ascontiguousarray(kpts, np.float32)
    n, K = kp.shape[0], kp.shape[1]
    p = np.ascontiguousarray(p9, np.int32)
    c, keep = c_config(cfg, sigmas)
    out = np.full((n, n), np.nan, np.float32)
    capi.check(lib.vp_dbg_pose_oks(device_id, kp.ctypes.data, n, K, p.ctypes.data, C.byref(c), out.ctypes.data))
    return out


def people(n, K=17, n_frames=1, seed=0, dup=0.5):
    """seeded people in the golden's style (no reference needed): float32 kpts [n, K, 3], box scores [n], p9 [n, 9]"""
    rng = np.random.default_rng(seed)
    kp, p9 = np.zeros((n, K, 3), np.float32), np.zeros((n, 9), np.int32)
    bs = rng.uniform(0.35, 0.99, n).astype(np.float32)
    for i in range(n):
        if i > 0 and rng.random() < dup:
            src = int(rng.integers(0, i))
            kp[i, :, :2] = kp[src, :, :2] + rng.normal(0.0, float(rng.choice([0.2, 1.0, 3.0])) * 6.0, (K, 2)).astype(np.float32)
            kp[i, :, 2] = np.clip(kp[src, :, 2] + rng.normal(0.0, 0.1, K), 0.05, 1.0).astype(np.float32)
            p9[i] = p9[src]
        else:
            cw, ch = int(rng.integers(60, 220)), int(rng.integers(120, 400))
            x0, y0 = int(rng.integers(0, 1280 - cw)), int(rng.integers(0, 720 - ch))
            kp[i, :, 0] = rng.uniform(y0, y0 + ch, K)
            kp[i, :, 1] = rng.uniform(x0, x0 + cw, K)
            kp[i, :, 2] = rng.uniform(0.05, 1.0, K)
            p9[i] = [int(rng.integers(0, n_frames)), x0, y0, cw, ch, 0, 0, cw, ch]
    return kp, bs, p9


def sigmas17():
    return np.asarray(COCO17_SIGMAS, np.float32)


def edge_cases():
    """name -> (kpts, box, p9, n_frames, status or None): the inputs of the constructed edge cases that the device is compared with the host model on"""
    out = {}
    kp, bs, p9 = people(1, seed=1)
    out['one_row'] = (kp, bs, p9, 1, None)
    kp, bs, p9 = people(1, seed=2)
    out['two_identical'] = (np.concatenate([kp, kp]), np.concatenate([bs, bs]), np.concatenate([p9, p9]), 1, None)
    kp, bs, p9 = people(9, n_frames=1, seed=3)
    p9[:, 0] = 2
    out['frames_without_rows'] = (kp, bs, p9, 4, None)
    kp, bs, p9 = people(30, n_frames=3, seed=4)
    out['three_frames_interleaved'] = (kp, bs, p9, 3, None)
    kp, bs, p9 = people(12, n_frames=2, seed=5)
    st = np.zeros(12, np.int32)
    st[[1, 6]] = [3, 1]
    p9[3, 0], p9[8, 0] = 2, -1
    out['bad_status_and_frames'] = (kp, bs, p9, 2, st)
    kp, bs, p9 = people(4, seed=6)
    kp[2, :, 2] = 0.1
    out['no_visible_joint'] = (kp, bs, p9, 1, None)
    return out
