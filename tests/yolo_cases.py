"""Shared by tests/test_yolo_host.py and tests/test_gpu_yolo.py: the whole-network cases of the detector network, their inputs, the oracle's heads (computed once
per process) and the tolerances, which come from the oracle alone (tests/yolo_model.py).

Tolerance of a case, per quantity (box values in pixels, class scores): the largest deviation of N_PERTURBED perturbed 'stored' runs from the unperturbed one,
times 2 -- eight runs under-sample the tail, and the device differs from 'stored' only where float32 summation order flips an fp16 rounding, a subset of what the
perturbation does.  tests/golden/yolo_sens.npz holds them with the cases' seeds (`python tests/yolo_cases.py` rewrites it); the CPU suite recomputes and compares.

The chain cases (letterbox -> network -> detector stage) pick conf_thr and iou_thr from GAPS in the oracle's own values, so that a deviation within the tolerance
cannot change which anchors survive: `chain_thresholds`."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # `python tests/yolo_cases.py` rewrites the golden file
import yolo_model as M  # noqa: E402
from easy_vitpose_amd.devyolo import synth_yolo  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'yolo_sens.npz')
N_PERTURBED = 8

# name: (scale, nc, (in_h, in_w), images, seed)
CASES = {
    'n_32x32x1': ('n', 80, (32, 32), 1, 11),
    'n_64x96x3': ('n', 80, (64, 96), 3, 12),
    'n_96x64x2': ('n', 80, (96, 64), 2, 13),
    's_64x64x2': ('s', 1, (64, 64), 2, 14),
    'm_64x64x1': ('m', 91, (64, 64), 1, 15),
}
# the chain cases: one synthetic frame (frame_h, frame_w, seed, class) per whole-network case; the detector stage keeps that class only (as VitInference's
# det_class does).  Seed and class are the first ones whose oracle head has the gaps `chain_thresholds` asks for.
CHAIN_FRAMES = {'n_32x32x1': (24, 32, 0, 36), 'n_64x96x3': (60, 80, 0, 76), 'n_96x64x2': (120, 70, 8, 58), 's_64x64x2': (64, 64, 0, 0), 'm_64x64x1': (50, 64, 3, 84)}


@functools.lru_cache(maxsize=None)
def state(name):
    scale, nc, _, _, seed = CASES[name]
    return synth_yolo(scale, nc, seed)


@functools.lru_cache(maxsize=None)
def images(name):
    """the input as the letterbox stage leaves it: fp16 [n, 3, H, W], values k / 255: smooth blobs plus noise"""
    _, _, (h, w), n, seed = CASES[name]
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, 3, h, w), np.float16)
    for i in range(n):
        for c in range(3):
            cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(4, 20)
            v = 90 + 120 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + rng.integers(0, 40, (h, w))
            out[i, c] = (np.clip(v, 0, 255).astype(np.uint8) / np.float32(255)).astype(np.float16)
    return out


@functools.lru_cache(maxsize=None)
def oracle_head(name, mode='stored'):
    """float64 [n, 4 + nc, A]; read-only"""
    h = M.forward(state(name), images(name), mode)
    h.setflags(write=False)
    return h


def deviation(a, b):
    """(box, score): the largest absolute difference of two heads [n, 4 + nc, A] per quantity"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(d[:, :4].max()), float(d[:, 4:].max())


def sensitivity(sd, x):
    """(tol_box, tol_score) of a network on an input: 2 x the largest deviation of N_PERTURBED perturbed stored runs from the unperturbed one"""
    base = M.forward(sd, x, 'stored')
    dev = [deviation(M.forward(sd, x, 'stored', perturb=7000 + r), base) for r in range(N_PERTURBED)]
    return 2 * max(d[0] for d in dev), 2 * max(d[1] for d in dev)


def compute_sens():
    out = {}
    for name, (_, _, _, _, seed) in CASES.items():
        out[name] = np.asarray(sensitivity(state(name), images(name)) + (float(seed),), np.float64)
        if name in CHAIN_FRAMES:
            out['chain_' + name] = np.asarray(sensitivity(state(name), chain_input(name)[0]) + (float(seed),), np.float64)
    return out


@functools.lru_cache(maxsize=None)
def golden_sens():
    with np.load(GOLDEN) as z:
        return {k: z[k].copy() for k in z.files}


def tolerance(name):
    """(tol_box in pixels, tol_score) of a case, from the committed file"""
    t = golden_sens()[name]
    return float(t[0]), float(t[1])


# ------------------------------------------------------------------ the chain
@functools.lru_cache(maxsize=None)
def chain_frame(name):
    """uint8 [h, w, 3] RGB"""
    fh, fw, seed, _ = CHAIN_FRAMES[name]
    rng = np.random.default_rng(2000 + seed)
    yy, xx = np.mgrid[0:fh, 0:fw]
    img = np.empty((fh, fw, 3), np.uint8)
    for c in range(3):
        cy, cx, s = rng.uniform(0, fh), rng.uniform(0, fw), rng.uniform(5, 25)
        img[..., c] = np.clip(60 + 150 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + rng.integers(0, 50, (fh, fw)), 0, 255).astype(np.uint8)
    return img


@functools.lru_cache(maxsize=None)
def chain_input(name):
    """(the letterboxed tensor fp16 [1, 3, H, W], the undo table float32 [1, 5]) of the case's frame, by the letterbox stage's host tap (the device stage equals it
    byte for byte: tests/test_gpu_letterbox.py)"""
    from easy_vitpose_amd.cropprep import Frame
    from easy_vitpose_amd.devletterbox import HostLetterbox, LetterboxCfg
    tensor, table, _ = HostLetterbox(LetterboxCfg(CASES[name][2])).letterbox([Frame.rgb(chain_frame(name))])
    return tensor, table


@functools.lru_cache(maxsize=None)
def chain_head(name):
    h = M.forward(state(name), chain_input(name)[0], 'stored')
    h.setflags(write=False)
    return h


def _corners(box):
    cx, cy, w, h = box
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])


def _iou_bounds(c, t):
    """(lowest, highest) IoU of every pair of the boxes c [4, k] (x1, y1, x2, y2) when every corner coordinate may move by t: the highest is the intersection of
    the boxes grown by t over the union of the boxes shrunk by t, the lowest the other way round"""
    def parts(g):
        q = np.stack([c[0] - g, c[1] - g, c[2] + g, c[3] + g])
        area = np.clip(q[2] - q[0], 0, None) * np.clip(q[3] - q[1], 0, None)
        ix = np.minimum(q[2][:, None], q[2][None]) - np.maximum(q[0][:, None], q[0][None])
        iy = np.minimum(q[3][:, None], q[3][None]) - np.maximum(q[1][:, None], q[1][None])
        return area, np.clip(ix, 0, None) * np.clip(iy, 0, None)
    (a_g, i_g), (a_s, i_s) = parts(t), parts(-t)
    hi = i_g / np.maximum(a_s[:, None] + a_s[None] - i_s, 1e-12)
    lo = i_s / np.maximum(a_g[:, None] + a_g[None] - i_g, 1e-12)
    return lo, np.minimum(hi, 1.0)


def _greedy(order_scores, over):
    """greedy NMS on candidates already in descending score order: the indices kept"""
    keep = []
    for i in range(len(order_scores)):
        if not any(over[g, i] for g in keep):
            keep.append(i)
    return keep


def chain_thresholds(name):
    """(conf_thr, iou_thr, k, m) from gaps in the oracle's head of the case's frame, or raises.  A deviation within the tolerance must not be able to change what the
    detector stage returns, rows and their order:
      * the k best anchors of the kept class, 5 <= k <= 200, with a score gap to the (k + 1)-th wider than 2 x tol_score around conf_thr;
      * the detector takes an anchor's best class over ALL classes first: the kept class wins every candidate anchor by more than 2 x tol_score, and on every
        other anchor it either loses by more than that or lies more than tol_score below conf_thr;
      * a certificate for the greedy NMS at iou_thr.  With K the m anchors the oracle keeps: the members of K differ pairwise by more than 2 x tol_score (their
        order is the order of the rows) and stay below iou_thr pairwise however their corners move; every other candidate has a suppressor in K that lies more
        than 2 x tol_score above it and stays above iou_thr with it.  By induction over any order consistent with these gaps the greedy walk keeps exactly K.
        Pairs of suppressed candidates need no gap: neither can suppress anything.
    Corners: a corner is cx +- w / 2, so a head within tol_box moves it by at most 1.5 x tol_box; the IoU bounds move every corner by twice that."""
    tol_box, tol_score = tolerance('chain_' + name)
    head = chain_head(name)[0]
    c = CHAIN_FRAMES[name][3]
    best = np.where(head[4:].argmax(0) == c, head[4:].max(0), 0.0)
    kept = head[4 + c]
    others = np.delete(head[4:], c, axis=0).max(0) if head.shape[0] > 5 else np.zeros_like(kept)
    order = np.argsort(-best, kind='stable')
    s = best[order]
    ks = [k for k in range(5, min(200, len(s) - 1) + 1) if s[k - 1] - s[k] > 2 * tol_score]
    if not ks:
        raise AssertionError(f'{name}: no score gap wider than {2 * tol_score:.3g} among the 5..200 best anchors')
    why = ''
    for k in sorted(ks, key=lambda q: s[q] - s[q - 1]):   # the widest gap first
        conf_thr = float(np.float32((s[k - 1] + s[k]) / 2))
        cand = np.zeros(len(best), bool)
        cand[order[:k]] = True
        if (kept[cand] - others[cand] <= 2 * tol_score).any():
            why = f'a candidate wins its anchor by less than {2 * tol_score:.3g}'
            continue
        if ((others[~cand] - kept[~cand] <= 2 * tol_score) & (kept[~cand] + tol_score >= conf_thr)).any():
            why = f'an anchor of another class could turn into a candidate within {2 * tol_score:.3g}'
            continue
        lo, hi = _iou_bounds(_corners(head[:4, order[:k]]), 2 * 1.5 * tol_box)
        mid, _ = _iou_bounds(_corners(head[:4, order[:k]]), 0.0)
        sep = np.abs(s[:k, None] - s[None, :k]) > 2 * tol_score
        found = None
        for thr in np.arange(0.05, 0.96, 0.01):
            thr = float(np.float32(thr))
            K = _greedy(s[:k], mid > thr)
            rest = [j for j in range(k) if j not in K]
            ok = all(hi[a_, b_] < thr and sep[a_, b_] for i_, a_ in enumerate(K) for b_ in K[i_ + 1:])
            ok = ok and all(any(lo[g, j] > thr and s[g] - s[j] > 2 * tol_score for g in K) for j in rest)
            if ok and (found is None or len(K) > found[1]):
                found = (thr, len(K))
        if found is None:
            why = f'no IoU threshold in 0.05..0.95 has a certificate for the greedy NMS of the {k} candidates'
            continue
        return conf_thr, found[0], k, found[1]
    raise AssertionError(f'{name}: {why}')


if __name__ == '__main__':
    sens = compute_sens()
    np.savez(GOLDEN, **sens)
    for k_, v_ in sens.items():
        print(k_, v_)
    for name_ in CHAIN_FRAMES:
        print(name_, chain_thresholds(name_))
