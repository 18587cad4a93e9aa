"""The plan of a chunk with per-crop experts under the per-expert flip-test mode, on the host (no GPU): vp_dbg_mix_plan_flip -- the pure function behind
vp_infer_experts and its twins while vp_set_flip_test_experts is on -- against a numpy restatement: a chunk of max_batch // 2 crops in stable expert order,
position j as forward rows 2 j (the crop) and 2 j + 1 (its mirror); the per-row ids with their padding; the four-field decode records; the hipGraph pattern,
which counts crops; the tile mlp.fc2 keeps on the doubled bounds; refusals."""
from __future__ import annotations

import os

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.moe import NUM_KEYPOINTS

E = 6
KS = np.array(NUM_KEYPOINTS, np.int32)   # 17, 14, 16, 17, 17, 133
KMAX = int(KS.max())
MAX_BATCHES = (2, 3, 5, 8, 16)
SIZES = range(0, 41)


def seeded_ids(n, max_batch):
    return np.random.default_rng(1000 * max_batch + n).integers(0, E, n).astype(np.int32)


def plan_flip(ids, max_batch, n_experts=E, ks=KS):
    """-> (rc, order [n], row_ids [chunks, B], counts [chunks, E], records [n, 4], pattern [chunks]) of the tap"""
    lib = capi.load_library()
    ids = np.ascontiguousarray(ids, np.int32)
    n = len(ids)
    chunks = -(-n // max(max_batch // 2, 1))
    B = (max_batch + 3) // 4 * 4
    order = np.full(n, -1, np.int32)
    rows = np.full((chunks, B), -1, np.int32)
    counts = np.full((chunks, n_experts), -1, np.int32)
    records = np.full((n, 4), -1, np.int32)
    pattern = np.zeros(chunks, np.uint64)
    rc = lib.vp_dbg_mix_plan_flip(ids.ctypes.data, n, n_experts, max_batch, ks.ctypes.data, order.ctypes.data, rows.ctypes.data, counts.ctypes.data,
                                  records.ctypes.data, pattern.ctypes.data)
    return rc, order, rows, counts, records, pattern


def plain_pattern(ids, max_batch):
    """vp_dbg_mix_plan's pattern per chunk of max_batch crops"""
    lib = capi.load_library()
    ids = np.ascontiguousarray(ids, np.int32)
    chunks = -(-len(ids) // max_batch)
    pattern = np.zeros(chunks, np.uint64)
    rc = lib.vp_dbg_mix_plan(ids.ctypes.data, len(ids), E, max_batch, None, None, None, None, None, pattern.ctypes.data)
    assert rc == chunks
    return pattern


def chunks_of(ids, max_batch):
    cap = max_batch // 2
    for c, off in enumerate(range(0, len(ids), cap)):
        yield c, off, ids[off:off + cap]


def segments(srt):
    """(start, count) of the run-length segments of sorted ids"""
    starts = np.flatnonzero(np.r_[True, srt[1:] != srt[:-1]])
    return list(zip(starts.tolist(), np.diff(np.r_[starts, len(srt)]).tolist()))


@pytest.mark.parametrize('max_batch', MAX_BATCHES)
def test_plan_against_numpy(max_batch):
    B = (max_batch + 3) // 4 * 4
    for n in SIZES:
        ids = seeded_ids(n, max_batch)
        rc, order, rows, counts, records, pattern = plan_flip(ids, max_batch)
        assert rc == -(-n // (max_batch // 2)), (n, max_batch)
        for c, off, chunk in chunks_of(ids, max_batch):
            nb = len(chunk)
            want = np.argsort(chunk, kind='stable').astype(np.int32)
            assert np.array_equal(order[off:off + nb], want)
            srt = chunk[want]
            want_rows = srt[np.minimum(np.arange(B) >> 1, nb - 1)]     # rows 2 j, 2 j + 1 = position j; the padding rows repeat the last row
            assert np.array_equal(rows[c], want_rows), (n, max_batch, c)
            assert np.array_equal(counts[c], np.bincount(chunk, minlength=E))
            want_rec = np.zeros((nb, 4), np.int32)
            for s0, cnt in segments(srt):
                e = srt[s0]
                for j in range(s0, s0 + cnt):
                    want_rec[j] = (2 * s0 * KMAX + 2 * (j - s0) * KS[e], KS[e], want[j], e)
            assert np.array_equal(records[off:off + nb], want_rec), (n, max_batch, c)
        # both count crops, not rows: the plain tap with chunks of max_batch // 2 crops
        assert np.array_equal(pattern, plain_pattern(ids, max_batch // 2)), (n, max_batch)


@pytest.mark.parametrize('max_batch', MAX_BATCHES)
def test_records_do_not_overlap_and_stay_inside_the_chunks_maps(max_batch):
    for n in SIZES:
        ids = seeded_ids(n, max_batch)
        _, _, _, _, records, _ = plan_flip(ids, max_batch)
        for c, off, chunk in chunks_of(ids, max_batch):
            nb = len(chunk)
            assert 2 * nb <= max_batch
            used = np.zeros(2 * nb * KMAX, np.int32)
            for first, K, dst, e in records[off:off + nb]:
                assert 0 <= first and first + 2 * K <= 2 * nb * KMAX and K == KS[e] and chunk[dst] == e
                used[first:first + 2 * K] += 1
            assert used.max() <= 1, 'two records share a map'
            assert sorted(records[off:off + nb, 2].tolist()) == list(range(nb)), 'every caller row exactly once'


@pytest.mark.parametrize('max_batch', MAX_BATCHES)
def test_fc2_tile_on_the_doubled_bounds(max_batch):
    """vp_dbg_expert_tile on the bounds mix_chunk_body hands the plan under the mode (the doubled segment starts): a 128-row tile never spans an expert change
    (2 b x 192 rows are a multiple of 128), a 256-row tile is kept exactly when every segment start is even -- which all-even crop counts give (the counts
    of all segments but the last decide: the last one ends the batch, not a segment)."""
    lib = capi.load_library()
    D = 768
    kept256 = changed256 = 0
    for n in SIZES:
        ids = seeded_ids(n, max_batch)
        for c, off, chunk in chunks_of(ids, max_batch):
            segs = segments(np.sort(chunk, kind='stable'))
            starts = [s0 for s0, _ in segs][1:]
            bounds = np.ascontiguousarray([2 * s for s in starts], np.int32)
            M = 2 * len(chunk) * 192
            ptr = bounds.ctypes.data if len(bounds) else None
            assert lib.vp_dbg_expert_tile(1, M, D, 0, ptr, len(bounds)) == 1
            assert lib.vp_dbg_expert_tile(1, M, D, 1, ptr, len(bounds)) == 1
            got = lib.vp_dbg_expert_tile(16, M, D, 1, ptr, len(bounds))
            all_starts_even = all(s % 2 == 0 for s in starts)
            assert (got == 16) == all_starts_even, (chunk.tolist(), got)
            if all(cnt % 2 == 0 for _, cnt in segs):
                assert got == 16
            kept256 += got == 16
            changed256 += got != 16
    assert kept256 > 0 and (changed256 > 0 or max_batch < 8)   # chunks of one or two crops rarely leave an odd start; from four crops on both sides occur


def test_refusals_name_the_crop():
    rc, *_ = plan_flip(seeded_ids(5, 8), 1)
    assert rc == capi.VP_ERR_INVALID and 'max_batch' in capi.last_error(None)
    for bad, at in (([0, 6], 1), ([-1, 0], 0), ([0] * 9 + [7], 9)):
        rc, *_ = plan_flip(np.array(bad, np.int32), 8)
        assert rc == capi.VP_ERR_INVALID
        assert f'of crop {at} ' in capi.last_error(None)


def test_new_symbols_are_bound_and_declared():
    lib = capi.load_library()
    header = open(os.path.join(os.path.dirname(capi.__file__), '..', 'include', 'vitpose_hip.h')).read()
    assert '#define VP_HAS_FLIP_TEST_EXPERTS 1' in header and '#define VP_ABI_VERSION 4' in header
    for name in ('vp_set_flip_test_experts', 'vp_dbg_mix_plan_flip', 'vp_dbg_decode_flip_mix'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and name in header
