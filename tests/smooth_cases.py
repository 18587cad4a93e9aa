"""Keypoint sequences for the smoother tests (tests/test_smooth_host.py, tests/test_gpu_smooth.py): seeded multi-person call lists that exercise the lifecycle of
vp_smooth_update_stream -- ids appearing, vanishing and returning inside and beyond max_age, partial step masks, rank masks, duplicate ids, non-finite rows,
absent rows, rows naming a stream outside the table, ageing calls without rows, partial and full resets -- the table-full case and the 64-stream case.  A call is
a dict of `update` arguments (kpts, ids, stream, rank, t_e, step_mask) or {'reset': streams}."""
from __future__ import annotations

import functools

import numpy as np

FPS = (30.0, 25.0, 59.94)
# (seed, K, n_streams, max_age, missing)
SEQUENCES = [(1, 17, 1, 0, 'reference'), (2, 17, 1, 1, 'restart'), (3, 17, 3, 2, 'reference'), (4, 17, 3, 3, 'restart'),
             (5, 133, 1, 1, 'reference'), (6, 133, 3, 1, 'restart'), (7, 133, 3, 0, 'reference'), (8, 17, 1, 3, 'restart')]


def tag_of(case) -> str:
    seed, K, ns, age, missing = case
    return f'seed{seed}_k{K}_s{ns}_age{age}_{missing}'


def people(rng, P, K, frames):
    """[frames, P, K, 3] float32 (y, x, conf): a random walk per joint, some joints starting at negative positions, 3 % of the coordinates missing (0)"""
    base = rng.uniform(-3, 400, size=(P, K, 2))
    xy = (base[None] + np.cumsum(rng.normal(0, 2.5, size=(frames, P, K, 2)), 0)).astype(np.float32)
    xy[rng.random(xy.shape) < 0.03] = 0.0
    conf = rng.uniform(0.05, 1.0, size=(frames, P, K, 1)).astype(np.float32)
    return np.concatenate([xy, conf], axis=-1)


@functools.lru_cache(maxsize=None)
def sequence(case, frames=12, P=8):
    """-> (cfg kwargs, calls).  Person p lives on stream p % n_streams with id 1 + p // n_streams + (p % 2) * 40: the same id on different streams is two tracks."""
    seed, K, ns, max_age, missing = case
    rng = np.random.default_rng(100 + seed)
    cfg = dict(fps=FPS[seed % 3], max_age=max_age, n_streams=ns, missing=missing)
    kp = people(rng, P, K, frames)
    home = np.arange(P) % ns
    pid = 1 + np.arange(P) // ns + (np.arange(P) % 2) * 40
    # presence: runs of frames in and out, so that tracks vanish for 1..4 frames -- inside and beyond every max_age of the list
    present = np.ones((frames, P), bool)
    for p in range(P):
        f = int(rng.integers(0, 3))
        present[:f, p] = False
        while f < frames:
            f += int(rng.integers(1, 5))
            gap = int(rng.integers(1, 5))
            present[f:f + gap, p] = False
            f += gap
    calls = []
    for f in range(frames):
        if f == 5 and seed % 2:
            calls.append({'reset': [0] if ns > 1 else None})
        if f == 9 and seed % 3 == 0:
            calls.append({'reset': None})
        if f in (4, 8):   # an ageing call without rows
            calls.append(dict(kpts=np.zeros((0, K, 3), np.float32), ids=np.zeros(0, np.int32), stream=None, rank=None, t_e=None,
                              step_mask=None if f == 4 or ns == 1 else [ns - 1]))
        rows, ids, stream = [], [], []
        for p in np.flatnonzero(present[f]):
            rows.append(kp[f, p].copy()); ids.append(pid[p]); stream.append(home[p])
        if rows and rng.random() < 0.4:      # a duplicate id: the same person a second time, other keypoints
            k = int(rng.integers(len(rows)))
            rows.append(rows[k] + np.float32(1.5)); ids.append(ids[k]); stream.append(stream[k])
        if rows and rng.random() < 0.4:      # a non-finite row
            k = int(rng.integers(len(rows)))
            rows[k][int(rng.integers(K)), int(rng.integers(2))] = [np.nan, np.inf, -np.inf][int(rng.integers(3))]
        if rng.random() < 0.4:               # an absent row, as the tracker writes them
            rows.append(np.zeros((K, 3), np.float32)); ids.append(-1); stream.append(-1)
        if rng.random() < 0.2:               # a row that names a stream outside the table
            rows.append(kp[f, 0] + np.float32(3)); ids.append(77); stream.append(ns if rng.random() < 0.5 else -2)
        if rows and rng.random() < 0.3:      # a NaN in a confidence is no reason to skip the row
            rows[int(rng.integers(len(rows)))][0, 2] = np.nan
        order = rng.permutation(len(rows))
        kpts = np.array([rows[i] for i in order], np.float32).reshape(-1, K, 3)
        ids = np.array([ids[i] for i in order], np.int32)
        stream = np.array([stream[i] for i in order], np.int32)
        rank = None
        if f % 2 and len(ids):
            rank = np.where(rng.random(len(ids)) < 0.25, -1, rng.integers(0, 5, len(ids))).astype(np.int32)
        step = None
        if ns > 1 and f % 3 == 2:
            step = sorted(rng.choice(ns, size=int(rng.integers(1, ns)), replace=False).tolist())
        t_e = [None, 1.0, 2.0, 0.5, 3.0][f % 5] if f % 4 else rng.choice([1.0, 2.0, 0.5, 3.0], size=ns)
        if ns == 1 and stream.size and (stream == 0).all() and f % 2 == 0:
            stream = None                    # the NULL stream argument
        calls.append(dict(kpts=kpts, ids=ids, stream=stream, rank=rank, t_e=t_e, step_mask=step))
    return cfg, calls


@functools.lru_cache(maxsize=None)
def table_full(K=17):
    """129 ids on one stream: the 129th birth is dropped (flag 2) and passed through; the next call updates 128 of them, drops it again and bears nobody"""
    rng = np.random.default_rng(7)
    kp = people(rng, 129, K, 2)
    ids = np.arange(10, 139, dtype=np.int32)
    cfg = dict(fps=30.0, max_age=1, n_streams=1, missing='reference', max_rows=129)
    return cfg, [dict(kpts=kp[f], ids=ids, stream=None, rank=None, t_e=None, step_mask=None) for f in range(2)]


@functools.lru_cache(maxsize=None)
def interleaved_streams(K=17, frames=4):
    """64 streams x 2 persons in one call per frame, rows shuffled; ids 1 and 2 on every stream"""
    rng = np.random.default_rng(11)
    kp = people(rng, 128, K, frames)
    cfg = dict(fps=30.0, max_age=1, n_streams=64, missing='reference')
    calls = []
    for f in range(frames):
        order = rng.permutation(128)
        calls.append(dict(kpts=kp[f][order], ids=(1 + order // 64).astype(np.int32), stream=(order % 64).astype(np.int32), rank=None,
                          t_e=rng.choice([1.0, 2.0, 0.5], size=64), step_mask=None))
    return cfg, calls


def run(update, reset, calls):
    """the calls through update(**call) / reset(streams) -> the list of (out, flags) of the update calls"""
    outs = []
    for c in calls:
        if 'reset' in c:
            reset(c['reset'])
        else:
            outs.append(update(**c))
    return outs


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
