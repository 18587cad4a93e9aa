"""Detection sequences for the tracker tests (tests/test_track_host.py, tests/test_gpu_track.py) and their golden generator
(tests/golden/make_golden_track.py): the seeded crowd generator, the five crowd sequences, the four older sequences of tests/golden/cases.py, and the
seeded matrices of the assignment tests."""
from __future__ import annotations

import numpy as np

# (seed, persons, frames, max_age, min_hits, skipped frames)
CROWDS = [(1, 12, 30, 1, 3, ()),
          (2, 24, 30, 3, 3, (7, 8, 20)),
          (3, 40, 24, 2, 1, tuple(range(3, 24, 2))),
          (4, 100, 16, 1, 3, ()),
          (5, 120, 12, 1, 3, ())]
IOU_THRESHOLD = float(np.float32(0.3))   # the value the device compares with; the twin and the reference are run with the same number


def crowd(seed, P, F, W=640, H=360, miss=0.1, skip=()):
    """-> F arrays [n, 5] float64 (x1, y1, x2, y2, score), every value representable in float32"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform([0, 0], [W - 80, H - 160], (P, 2))
    vel = rng.normal(0, 6, (P, 2))
    size = rng.uniform([40, 90], [90, 200], (P, 2))
    entry = rng.integers(0, F // 2, P) * (rng.random(P) < 0.3)
    frames = []
    for f in range(F):
        rows = []
        for p in range(P):
            if f < entry[p]:
                continue
            if rng.random() < miss:
                continue
            c = pos[p] + vel[p] * (f - entry[p])
            box = np.array([c[0], c[1], c[0] + size[p, 0], c[1] + size[p, 1]]) + rng.normal(0, 2, 4)
            rows.append(np.concatenate([box, [0.4 + 0.5 * rng.random()]]))
        d = np.array(rows, dtype=np.float64).reshape(-1, 5)
        d = d[rng.permutation(len(d))]
        if f in skip:
            d = np.empty((0, 5))
        frames.append(d.astype(np.float32).astype(np.float64))
    return frames


def old_sequences():
    """(tag, frames, max_age, min_hits) of the four sequences behind tests/golden/sort_*.npz"""
    from cases import tracker_sequence, tracker_sequence_step
    f32 = lambda seq: [np.asarray(d, np.float64).reshape(-1, 5).astype(np.float32).astype(np.float64) for d in seq]   # noqa: E731
    return [('sort_age1', f32(tracker_sequence()), 1, 3), ('sort_age3', f32(tracker_sequence()), 3, 3),
            ('sort_step2', f32(tracker_sequence_step(2)), 2, 1), ('sort_step3', f32(tracker_sequence_step(3)), 3, 1)]


def all_sequences():
    return old_sequences() + [(f'crowd{seed}', crowd(seed, P, F, skip=skip), age, hits) for seed, P, F, age, hits, skip in CROWDS]


LSAP_SIZES = (1, 2, 7, 63, 64, 65, 128)
LSAP_DENSITIES = (0.05, 0.3, 1.0)


def lsap_matrix(nd, nt, density, seed=0):
    rng = np.random.default_rng(1000003 * nd + 1009 * nt + int(density * 100) + seed)
    m = rng.uniform(0.01, 0.99, (nd, nt))
    return np.ascontiguousarray(m * (rng.random((nd, nt)) < density))


def lsap_cases():
    return [(nd, nt, dens) for nd in LSAP_SIZES for nt in LSAP_SIZES for dens in LSAP_DENSITIES]


def associate_twin(iou, thr):
    """tracker.associate from the IoU matrix on: trk_of_det [nd]"""
    from scipy.optimize import linear_sum_assignment
    over = iou > thr
    if over.sum(1).max() <= 1 and over.sum(0).max() <= 1:
        pairs = np.argwhere(over)
    else:
        r, c = linear_sum_assignment(-iou)
        pairs = np.stack([r, c], 1)
    out = np.full(iou.shape[0], -1, np.int32)
    for d, t in pairs:
        if iou[d, t] >= thr:
            out[d] = t
    return out


def run_rows(tracker_update, frames):
    """the rows of a whole sequence as [(frame, x1, y1, x2, y2, score, id)] float64"""
    rows = []
    for i, d in enumerate(frames):
        o = np.asarray(tracker_update(d.copy()), dtype=np.float64).reshape(-1, 6)
        rows.append(np.concatenate([np.full((len(o), 1), i, dtype=np.float64), o], 1))
    return np.concatenate(rows)


def rows_with_state(tracker, frames, n_out=128):
    """A one-stream HostTracker (or anything with its update / state) over a sequence: ([(frame, box fp64 from the state, score, id)], the float32 rows per call)"""
    rows, calls = [], []
    for i, d in enumerate(frames):
        out = tracker.update(d, n_out=n_out)
        calls.append(out)
        n = int(out[3][-1])
        S = tracker.state()[0]
        assert S['n_rows'] == n
        rows.append(np.concatenate([np.full((n, 1), i, np.float64), S['rows'][:n], S['row_ids'][:n, None].astype(np.float64)], 1))
    return np.concatenate(rows), calls


def far_people(n, seed, x0=0.0):
    """n boxes 100 px apart (no pair overlaps), float32 [n, 5]"""
    rng = np.random.default_rng(seed)
    d = np.zeros((n, 5), np.float32)
    d[:, 0] = x0 + 100.0 * np.arange(n)
    d[:, 1] = rng.uniform(0, 50, n)
    d[:, 2] = d[:, 0] + rng.uniform(30, 60, n)
    d[:, 3] = d[:, 1] + rng.uniform(60, 120, n)
    d[:, 4] = rng.uniform(0.4, 0.9, n)
    return d


def edge_scenarios():
    """name -> ((max_age, min_hits, n_streams), [call]); a call = dict(dets=, frame_index=, n_out=, step=) for HostTracker.update / DeviceTracker.update_host"""
    call = lambda dets, fi=None, n_out=160, step=None: dict(dets=np.asarray(dets, np.float32).reshape(-1, 5), frame_index=fi, n_out=n_out, step=step)   # noqa: E731
    sc = {}
    sc['dets_128'] = ((1, 3, 1), [call(far_people(128, 1)), call(far_people(128, 1))])
    sc['dets_129'] = ((1, 3, 1), [call(far_people(129, 1)), call(far_people(129, 1))])
    d = np.concatenate([far_people(126, 2)[:120], far_people(5, 3, x0=20000.0)])
    sc['births_at_128'] = ((1, 3, 1), [call(far_people(126, 2)), call(d), call(d[:120]), call(d)])
    sc['n_out_one_short'] = ((1, 3, 1), [call(far_people(7, 4), n_out=6), call(far_people(7, 4), n_out=7), call(np.empty((0, 5)), n_out=6)])
    d = far_people(6, 5)
    d[1, 2] = np.nan
    d[4, 4] = np.inf
    sc['nan_rows_and_bad_streams'] = ((1, 3, 2), [call(d, [0, 0, 0, 1, 1, 1], 8), call(far_people(3, 6), [0, 2, -1], 4, [0]), call(d, [1, 1, 1, 0, 0, 7], 8)])
    z = np.array([[5, 5, 5, 5, 0.5], [10, 10, 50, 90, 0.9], [60, 10, 60, 90, 0.7], [100, 40, 150, 40, 0.6]], np.float32)
    sc['zero_area_boxes'] = ((2, 1, 1), [call(z), call(z), call(z[1:2]), call(np.empty((0, 5))), call(z)])
    sc['rows_cut_in_front_of_an_empty_stream'] = ((1, 3, 3), [call(far_people(5, 8), [0, 0, 0, 2, 2], 2), call(far_people(5, 8), [0, 0, 0, 2, 2], 4)])
    frames = crowd(7, 6, 6, miss=0.2, skip=(3,))
    sc['step_mask'] = ((2, 1, 3), [call(np.concatenate([f, f, f]), np.repeat([0, 1, 2], len(f)).astype(np.int32), 40, step) for f, step in
                                    zip(frames, (None, [0, 2], [1], None, [2], None))])
    return sc


def interleaved_streams(n_streams=64, persons=3, n_frames=4, seed=11):
    """per frame: (dets [n_streams * persons, 5] float32 interleaved over the streams in a seeded order, frame_index [..] int32); and the streams alone"""
    rng = np.random.default_rng(seed)
    per = [crowd(1000 + s, persons, n_frames, miss=0.15) for s in range(n_streams)]
    calls = []
    for f in range(n_frames):
        d = np.concatenate([per[s][f] for s in range(n_streams)])
        fi = np.concatenate([np.full(len(per[s][f]), s, np.int32) for s in range(n_streams)])
        order = rng.permutation(len(d))
        calls.append((d[order].astype(np.float32), fi[order]))
    return calls, per


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
