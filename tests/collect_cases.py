"""Seeded cases of the collect stage (csrc/collectgeom.h), shared by tests/test_collect_host.py (tap against the numpy twin) and tests/test_gpu_collect.py (device
against the tap).  A case is the keyword arguments of `collect_numpy` / `collect_tap` / `VitPoseHip.collect_host`."""
from __future__ import annotations

import functools
import itertools

import numpy as np

OPTIONAL = ('ids', 'frame', 'rank', 'status', 'score', 'crop_params')


def rows(seed, n, K, n_frames, *, drop=(), bad_frames=True, strided_score=False, nan=False):
    """n random rows: frames scattered through the call (a few outside the table), ids with -1 and duplicates, ranks and statuses that drop rows"""
    rng = np.random.default_rng(seed)
    kpts = rng.uniform(-50, 2000, (n, K, 3)).astype(np.float32)
    if nan and n:
        w = kpts.reshape(-1).view(np.uint32)
        at = rng.choice(len(w), size=max(1, len(w) // 7), replace=False)
        w[at] = np.where(rng.integers(0, 2, len(at)) == 1, 0x7fc00000, 0xffa00000).astype(np.uint32) | rng.integers(1, 1 << 20, len(at)).astype(np.uint32)
    lo, hi = (-1, n_frames + 1) if bad_frames else (0, n_frames)
    frame = rng.integers(lo, hi, n).astype(np.int32)
    ids = rng.integers(-1, max(2, n // 2), n).astype(np.int32)          # -1 (absent) and duplicates
    rank = rng.integers(-1, 4, n).astype(np.int32)
    status = (rng.integers(0, 5, n) == 0).astype(np.int32) * rng.integers(1, 4, n).astype(np.int32)
    if strided_score:
        table = rng.uniform(0, 1, (n, 6)).astype(np.float32)
        score = table[:, 4]                                             # column 4 of the tracker's rows, as the view it is
    else:
        score = rng.uniform(-1, 1, n).astype(np.float32)
    cp = rng.integers(-40, 3000, (n, 9)).astype(np.int32)
    cp[:, 0] = frame
    case = dict(kpts=kpts, ids=ids, frame=frame, rank=rank, status=status, score=score, crop_params=cp, n_frames=n_frames, max_records=None)
    for name in drop:
        case[name] = None
    return case


@functools.lru_cache(maxsize=None)
def host_cases():
    c = {}
    c['plain'] = rows(1, 37, 17, 3)
    c['k1'] = rows(2, 29, 1, 2)                                          # record stride 12 words
    c['k17'] = rows(3, 70, 17, 4)                                        # 60 words
    c['k133'] = rows(4, 41, 133, 3, nan=True)                            # 408 words
    c['k2_pad'] = rows(5, 19, 2, 1)                                      # 14 words, two of padding
    c['strided_score'] = rows(6, 33, 17, 2, strided_score=True)
    c['nan_payload'] = rows(7, 25, 17, 2, nan=True)
    c['n0'] = rows(8, 0, 17, 5)
    c['n1'] = rows(9, 1, 17, 1, bad_frames=False, drop=('rank', 'status'))
    c['one_frame_no_frame_ptr'] = rows(10, 65, 17, 1, drop=('frame',))
    c['ordinal_ids'] = rows(11, 90, 5, 6, drop=('ids',))
    c['ordinal_ids_no_frame'] = rows(12, 64, 3, 1, drop=('ids', 'frame'))
    c['empty_frames'] = rows(13, 50, 17, 9)
    c['empty_frames']['frame'] = np.where(c['empty_frames']['frame'] % 3 == 1, 4, c['empty_frames']['frame']).astype(np.int32)   # frames 1 and 7 get no row
    c['rank_all_negative'] = rows(14, 30, 17, 2)
    c['rank_all_negative']['rank'][:] = -1
    c['all_absent'] = rows(15, 12, 17, 1)
    c['all_absent']['ids'][:] = -1
    c['all_kept'] = rows(16, 130, 17, 2, bad_frames=False)
    for k, v in (('ids', 7), ('rank', 0), ('status', 0)):
        c['all_kept'][k][:] = v                                          # (one id on every row: duplicates are the caller's business)
    c['frames_descending'] = rows(17, 200, 17, 8, bad_frames=False)
    c['frames_descending']['frame'] = np.sort(c['frames_descending']['frame'])[::-1].copy()
    c['max_records_cut'] = dict(rows(18, 60, 17, 3), max_records=5)
    c['max_records_zero'] = dict(rows(19, 20, 17, 2), max_records=0)
    c['max_records_beyond'] = dict(rows(20, 20, 17, 2), max_records=50)
    c['frames64'] = rows(21, 300, 4, 64)
    c['chunk_600'] = rows(22, 600, 17, 2)                                # crosses any 256-row chunk boundary
    c['chunk_1025'] = rows(23, 1025, 3, 1, drop=('frame',))              # one row more than the plan's 16 waves x 64 lanes
    c['int32_wrap_box'] = rows(24, 9, 17, 1, bad_frames=False)
    c['int32_wrap_box']['crop_params'][:, 1:5] = np.array([2147483000, -2147483000, 5000, -5000], np.int32)
    c['cap_8192_on_64'] = rows(25, 8192, 17, 64)
    return c


@functools.lru_cache(maxsize=None)
def null_combos():
    """every combination of the six optional inputs being NULL, on 23 rows of K = 3 over 2 frames"""
    out = {}
    for bits in itertools.product((0, 1), repeat=len(OPTIONAL)):
        drop = tuple(n for n, b in zip(OPTIONAL, bits) if b)
        out['null_' + ''.join(map(str, bits))] = rows(100 + int(''.join(map(str, bits)), 2), 23, 3, 2, drop=drop)
    return out


def mask_rows(case):
    """the kept rows by a plain boolean mask, in record order (frame ascending, then call order), and the id of every row"""
    n, n_frames = len(case['kpts']), case['n_frames']
    frame = np.zeros(n, np.int32) if case['frame'] is None else case['frame']
    valid = (frame >= 0) & (frame < n_frames)
    keep = valid.copy()
    for name, ok in (('ids', lambda a: a >= 0), ('rank', lambda a: a >= 0), ('status', lambda a: a == 0)):
        if case[name] is not None:
            keep &= ok(case[name])
    if case['ids'] is not None:
        ids = case['ids']
    else:
        ids = np.zeros(n, np.int32)
        seen = {}
        for i in range(n):
            if valid[i]:
                ids[i] = seen.get(int(frame[i]), 0)
                seen[int(frame[i])] = ids[i] + 1
    order = sorted(np.nonzero(keep)[0].tolist(), key=lambda i: (int(frame[i]), i))
    return np.array(order, np.int64), ids, frame
