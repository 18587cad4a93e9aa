"""The plan of a chunk with per-crop experts on the host (no GPU): vp_dbg_mix_plan -- the pure function behind vp_infer_experts_device_stream,
vp_infer_frames_experts and vp_infer_boxes_experts_stream -- against numpy's stable argsort and run-length segments; the padding rows; the decode's
records; the expert pattern of the hipGraph key; refusals."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.moe import NUM_KEYPOINTS
from test_gpu_moe import patterns

E = len(NUM_KEYPOINTS)
KS = np.array(NUM_KEYPOINTS, np.int32)
KMAX = int(KS.max())
NO_GRAPH = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix_plan(ids, max_batch, n_experts=E, ks=KS):
    """-> (chunks, order [n], ids_padded [chunks, B], counts [chunks, E], records [n, 3], pattern [chunks]) of the tap"""
    lib = capi.load_library()
    ids = np.ascontiguousarray(ids, np.int32)
    n = len(ids)
    chunks = -(-n // max_batch)
    B = (max_batch + 3) // 4 * 4
    order = np.full(n, -1, np.int32)
    padded = np.full((chunks, B), -1, np.int32)
    counts = np.full((chunks, n_experts), -1, np.int32)
    records = np.full((n, 3), -1, np.int32)
    pattern = np.zeros(chunks, np.uint64)
    rc = lib.vp_dbg_mix_plan(ids.ctypes.data, n, n_experts, max_batch, None if ks is None else ks.ctypes.data, order.ctypes.data, padded.ctypes.data,
                             counts.ctypes.data, None if ks is None else records.ctypes.data, pattern.ctypes.data)
    return rc, order, padded, counts, records, pattern


def check_against_numpy(ids, max_batch):
    ids = np.asarray(ids, np.int32)
    n = len(ids)
    rc, order, padded, counts, records, pattern = mix_plan(ids, max_batch)
    assert rc == -(-n // max_batch)
    for c, off in enumerate(range(0, n, max_batch)):
        chunk = ids[off:off + max_batch]
        nb = len(chunk)
        want = np.argsort(chunk, kind='stable').astype(np.int32)
        assert np.array_equal(order[off:off + nb], want)
        srt = chunk[want]
        assert np.array_equal(padded[c, :nb], srt)
        assert (padded[c, nb:] == srt[-1]).all(), 'the padding rows repeat the last id'
        assert np.array_equal(counts[c], np.bincount(chunk, minlength=E))
        # run-length segments of the sorted ids -> where each head writes its maps, which row each crop decodes into
        starts = np.flatnonzero(np.r_[True, srt[1:] != srt[:-1]])
        seg_of = np.searchsorted(starts, np.arange(nb), side='right') - 1
        first = starts[seg_of] * KMAX + (np.arange(nb) - starts[seg_of]) * KS[srt]
        assert np.array_equal(records[off:off + nb, 0], first)
        assert np.array_equal(records[off:off + nb, 1], KS[srt])
        assert np.array_equal(records[off:off + nb, 2], want)
        # the maps of two crops never overlap, and every crop's lie inside the [nb, Kmax] maps of the chunk's heatmap buffer
        ends = first + KS[srt]
        assert (first[1:] >= ends[:-1]).all() and ends[-1] <= nb * KMAX
        assert (pattern[c] == 0) == (len(starts) == 1)


def test_plan_equals_stable_argsort_for_every_size_up_to_64():
    rng = np.random.default_rng(11)
    for n in range(1, 65):
        for _ in range(4):
            check_against_numpy(rng.integers(0, E, size=n), 64)
        check_against_numpy(rng.integers(0, 2, size=n) * 5, 64)


@pytest.mark.parametrize('n', [1, 3, 8, 13, 16, 24, 37, 64, 100, 120, 256, 300])
def test_plan_of_the_gpu_suites_patterns(n):
    for _, ids in patterns(n):
        check_against_numpy(ids, 256)
        check_against_numpy(ids, 64)   # n > max_batch: chunked as the entries chunk


def test_chunked_plan_is_the_plan_of_each_chunk():
    rng = np.random.default_rng(5)
    ids = rng.integers(0, E, size=150).astype(np.int32)
    rc, order, padded, counts, records, pattern = mix_plan(ids, 64)
    assert rc == 3
    for c, off in enumerate((0, 64, 128)):
        _, o1, p1, c1, r1, k1 = mix_plan(ids[off:off + 64], 64)
        nb = len(o1)
        assert np.array_equal(order[off:off + nb], o1) and np.array_equal(padded[c], p1[0]) and np.array_equal(counts[c], c1[0])
        assert np.array_equal(records[off:off + nb], r1) and pattern[c] == k1[0]


def _count_vectors(total_max):
    for counts in itertools.product(range(total_max + 1), repeat=E):
        if 1 <= sum(counts) <= total_max:
            yield counts


def test_pattern_code_is_exact_over_all_count_vectors_of_up_to_16_crops():
    """every count vector of 1 .. 16 crops over the six experts (74 612 of them): one expert -> 0, otherwise a code no other vector has"""
    seen = {}
    n_single = 0
    for counts in _count_vectors(16):
        ids = np.repeat(np.arange(E), counts).astype(np.int32)
        rc, _, _, got, _, pattern = mix_plan(ids, 16, ks=None)
        assert rc == 1 and tuple(got[0]) == counts
        code = int(pattern[0])
        if sum(1 for v in counts if v) == 1:
            assert code == 0
            n_single += 1
            continue
        assert code != 0 and code != int(NO_GRAPH)
        assert code not in seen, f'{counts} and {seen[code]} share a code'
        seen[code] = counts
    assert n_single == 16 * E and len(seen) == 74612 - 16 * E


def test_pattern_code_ignores_the_permutation():
    rng = np.random.default_rng(3)
    for n in (2, 5, 8, 16, 40):
        ids = rng.integers(0, E, size=n).astype(np.int32)
        ids[:2] = (0, 5)
        base = mix_plan(ids, 64)[5][0]
        assert base != 0
        for _ in range(8):
            assert mix_plan(rng.permutation(ids), 64)[5][0] == base
        other = ids.copy()
        other[0] = 1   # one crop moves to another expert: another count vector
        assert mix_plan(other, 64)[5][0] != base


def test_pattern_that_does_not_fit_the_encoding_is_marked():
    ids = np.r_[np.zeros(255, np.int32), np.ones(3, np.int32)]
    assert mix_plan(ids, 512)[5][0] == NO_GRAPH            # 255 crops of one expert
    assert mix_plan(ids[1:], 512)[5][0] not in (0, NO_GRAPH)   # 254 fit
    nine = np.arange(9, dtype=np.int32)
    assert mix_plan(nine, 16, n_experts=9, ks=None)[5][0] == NO_GRAPH
    assert mix_plan(nine[:8], 16, n_experts=8, ks=None)[5][0] not in (0, NO_GRAPH)
    assert mix_plan(np.full(300, 2, np.int32), 512)[5][0] == 0   # one expert: the plain path, whatever the count


@pytest.mark.parametrize('bad,at', [([0, 6], 1), ([-1, 0], 0), ([0] * 70 + [7], 70)])
def test_invalid_ids_are_refused_naming_the_crop(bad, at):
    rc, *_ = mix_plan(np.array(bad, np.int32), 64)
    assert rc == capi.VP_ERR_INVALID
    assert f'of crop {at} ' in capi.last_error(None)


def test_new_symbols_are_bound_and_declared():
    lib = capi.load_library()
    import os
    header = open(os.path.join(os.path.dirname(capi.__file__), '..', 'include', 'vitpose_hip.h')).read()
    assert '#define VP_HAS_EXPERT_ENTRIES 1' in header and '#define VP_ABI_VERSION 4' in header
    for name in ('vp_infer_experts_device_stream', 'vp_infer_frames_experts', 'vp_infer_boxes_experts_stream', 'vp_dbg_mix_plan', 'vp_dbg_decode_mix'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and name in header
