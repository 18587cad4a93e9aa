"""Seeded cases of the metrics stage (csrc/metricsgeom.h), shared by tests/test_metrics_host.py (tap == numpy twin) and tests/test_gpu_metrics.py (device == tap).

A case = dict(cfg=MetricsCfg, pred, gt, norm, area, rank, set, set_value); every optional input may be None.  With an OKS in play the generator stretches
the error of a row by 7 % until no OKS of the case lies within 1e-4 of a threshold (0.50 .. 0.95), judged on a plain fp64 numpy evaluation, so that the
device's own exp() cannot move a hit."""
from __future__ import annotations

import functools
import itertools
import os

import numpy as np

from easy_vitpose_amd.devmetrics import MetricsCfg
from easy_vitpose_amd.posenms import COCO17_SIGMAS

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics.npz')


def sigmas_for(K):
    return COCO17_SIGMAS if K == 17 else tuple([0.05] * K)


def _rows(seed, n, K, bad=False, odd_norm=True, odd_area=True):
    rng = np.random.default_rng(seed)
    h, w = rng.integers(80, 400, n).astype(F32), rng.integers(40, 250, n).astype(F32)
    gt = np.zeros((n, K, 3), F32)
    gt[:, :, 0] = rng.uniform(0, 1, (n, K)).astype(F32) * h[:, None]
    gt[:, :, 1] = rng.uniform(0, 1, (n, K)).astype(F32) * w[:, None]
    gt[:, :, 2] = rng.choice(np.array([0, 0.25, 1, 2], F32), (n, K), p=[0.2, 0.1, 0.35, 0.35])
    scale = rng.choice(np.array([0.5, 3.0, 10.0, 40.0], F32), n)
    pred = np.zeros_like(gt)
    pred[:, :, :2] = gt[:, :, :2] + rng.standard_normal((n, K, 2)).astype(F32) * scale[:, None, None]
    pred[:, :, 2] = rng.uniform(0.05, 1.0, (n, K)).astype(F32)
    norm = np.stack([h, w], axis=1).astype(F32)
    area = (h * w).astype(F32)
    if odd_norm and n:
        pick = rng.integers(0, n, 8)
        for k, v in enumerate([0.0, -0.0, -5.0, 1e-30, 0.0, -1e-3, 1e-38, 3e38]):   # zero / negative / tiny / huge normalisers
            norm[pick[k], k & 1] = v
    if odd_area and n:
        pick = rng.integers(0, n, 5)
        for k, v in enumerate([0.0, -4.0, np.inf, np.nan, 1e-20]):                # non-positive and non-finite areas, a tiny one
            area[pick[k]] = v
    if bad and n:
        for v in (np.nan, np.inf, -np.inf, 3e38, -3e38):                           # NaN / inf / overflowing predictions
            pred[rng.integers(0, n), rng.integers(0, K), rng.integers(0, 2)] = v
        gt[rng.integers(0, n), rng.integers(0, K), 2] = np.nan                     # a NaN v is not visible
        gt[rng.integers(0, n), rng.integers(0, K), 0] = np.inf
    rank = (rng.integers(0, 6, n) - 1).astype(np.int32)                            # about a sixth negative
    set_ = rng.integers(0, 3, n).astype(np.int32)                                  # three values
    return dict(pred=pred, gt=gt, norm=norm, area=area, rank=rank, set=set_, set_value=1)


def _oks_near(cs):
    """the rows whose OKS lies within 1e-4 of a threshold"""
    cfg = cs['cfg']
    if not cfg.use_oks or cs['area'] is None or not len(cs['pred']):
        return np.zeros(len(cs['pred']), bool)
    with np.errstate(all='ignore'):
        d = cs['pred'][:, :, :2].astype(np.float64) - cs['gt'][:, :, :2]
        vis = cs['gt'][:, :, 2] > cfg.vis_thr
        var = (2.0 * np.asarray(cfg.sigmas)) ** 2
        e = (d ** 2).sum(-1) / var / cs['area'].astype(np.float64)[:, None] / 2.0
        oks = np.where(vis, np.exp(-e), 0).sum(1) / np.maximum(vis.sum(1), 1)
        near = np.zeros(len(oks), bool)
        for t in range(10):
            near |= np.isfinite(oks) & (np.abs(oks - (0.5 + 0.05 * t)) < 1e-4)
        return near



def case(seed, n, K, use=('norm', 'area', 'rank', 'set'), oks=True, pck_thr=(0.05, 0.1, 0.2), auc_steps=20, auc_norm=30.0, vis_thr=0.0, **kw):
    cfg = MetricsCfg(n_joints=K, pck_thr=pck_thr, auc_steps=auc_steps, auc_norm=auc_norm, vis_thr=vis_thr, sigmas=sigmas_for(K) if oks else None)
    cs = _rows(seed, n, K, **kw)
    for name in ('norm', 'area', 'rank', 'set'):
        if name not in use:
            cs[name] = None
    cs['cfg'] = cfg
    for _ in range(50):   # a row too close to a threshold gets its error stretched by 7 % until it is not (a whole data set of thousands of rows never passes as drawn)
        near = _oks_near(cs)
        if not near.any():
            return cs
        with np.errstate(all='ignore'):
            cs['pred'][near, :, :2] = cs['gt'][near, :, :2] + (cs['pred'][near, :, :2] - cs['gt'][near, :, :2]) * F32(1.07)
    raise AssertionError('metrics_cases: an OKS stays within 1e-4 of a threshold')


@functools.lru_cache(maxsize=None)
def host_cases():
    c = {}
    for n in (0, 1, 63, 64, 65, 129, 1025, 8192):
        c[f'n{n}'] = case(100 + n, n, 17)
    for K in (1, 2, 133, 256):
        c[f'k{K}'] = case(200 + K, 129, K)
    c['k133_n1025'] = case(301, 1025, 133)
    c['vis03'] = case(302, 200, 17, vis_thr=0.3)
    c['pck0_auc0'] = case(303, 130, 17, pck_thr=(), auc_steps=0)
    c['pck8_auc32'] = case(304, 130, 17, pck_thr=(0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 1.0), auc_steps=32, auc_norm=17.5)
    c['bad_values'] = case(305, 300, 17, bad=True)
    c['bad_values_k133'] = case(306, 70, 133, bad=True)
    c['no_oks'] = case(307, 100, 17, oks=False)
    c['no_filters'] = case(308, 100, 17, use=('norm', 'area'))
    return c


def big_case():
    """8192 x 133: the cap of a call at the whole-body joint count"""
    return case(400, 8192, 133)


def null_combos():
    """every combination of NULL optional inputs on one data set"""
    out = {}
    for r in range(5):
        for use in itertools.combinations(('norm', 'area', 'rank', 'set'), r):
            out['+'.join(use) or 'none'] = case(500, 70, 17, use=use)
    return out


def inputs(cs):
    """the keyword arguments of metrics_tap / metrics_numpy / update_host"""
    return {k: cs[k] for k in ('pred', 'gt', 'norm', 'area', 'rank', 'set', 'set_value')}


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def ulp_diff(a, b):
    """distance in float32 steps between same-signed finite values"""
    a, b = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64), np.ascontiguousarray(b, F32).view(np.int32).astype(np.int64)
    return np.abs(a - b)
