"""GPU: the flip-test mode with one partner table per expert (vp_set_flip_test_experts, VitPoseHip.set_flip_test_datasets) -- what lets the per-crop expert
entries of a ViTPose+ handle run under the mode.  Every comparison is bit for bit: the fused decode<FLIP, MIX> alone against vp_dbg_decode_flip per crop; a
mixed call against the six split handles under the single-table mode with that dataset's pairs (the cross-batch identity of the one-launch family, as
tests/test_gpu_moe.py::test_mixed_batch_is_bit_identical_to_split_handles; a crop and its mirror keep their even / odd rows in both runs); a one-expert
chunk against set_dataset + infer under the same mode; the frames, boxes and device twins against infer_mixed; the 8-phase fc2 tiles on doubled bounds;
the mode's bookkeeping, its hipGraph keys and its refusals.

Parity against the reference is transitive: tests/test_gpu_flip_mode.py::test_mode_matches_oracle and the ViTPose+ goldens tie the split handles to the oracle."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.engine import decode_flip_heatmaps
from easy_vitpose_amd.moe import DATASETS, NUM_KEYPOINTS
from test_gpu_flip_mode import COCO_PAIRS, WB_PAIRS
from test_gpu_moe import check_mixed, expert_handle, patterns, pool, split_handle
from test_gpu_moe_entries import boxes_host_route, run_device

pytestmark = pytest.mark.gpu
E = len(DATASETS)
KMAX = max(NUM_KEYPOINTS)
AIC_PAIRS = [[0, 3], [1, 4], [2, 5], [6, 9], [7, 10], [8, 11]]          # tests/test_gpu_flip_mode.py::test_vitpose_plus_handle_under_the_mode
MPII_PAIRS = [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]
PAIRS = {'coco': COCO_PAIRS, 'aic': AIC_PAIRS, 'mpii': MPII_PAIRS, 'ap10k': COCO_PAIRS, 'apt36k': COCO_PAIRS, 'wholebody': WB_PAIRS}
assert set(PAIRS) == set(DATASETS)


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=1)
def crops48():
    """blobs and noise: the first 24 of each half of test_gpu_moe's pool"""
    p = pool()
    return np.ascontiguousarray(np.concatenate([p[:24], p[150:174]]))


@functools.lru_cache(maxsize=4)
def split_refs(shift: bool):
    """ref[e] = ViTPose-S split handle e's keypoints of crops48 under the single-table mode with that dataset's pairs (fp16, one-launch family: call it from a
    test that holds the one_launch_family fixture).  Computed once, shared, never written."""
    ref = {}
    for e, ds in enumerate(DATASETS):
        h = split_handle('s', ds, 'fp16', 16)
        h.set_flip_test(PAIRS[ds], shift_heatmap=shift)
        ref[e] = h.infer(crops48())
        ref[e].setflags(write=False)
        h.close()
    return ref


def mode_handle(variant='s', dtype='fp16', max_batch=16, shift=False, pairs=PAIRS):
    eng = expert_handle(variant, dtype, max_batch)
    eng.set_flip_test_datasets(pairs, shift_heatmap=shift)
    return eng


def partner_tables():
    lib = capi.load_library()
    tab = np.tile(np.arange(KMAX, dtype=np.int32), (E, 1))
    for e, ds in enumerate(DATASETS):
        p = np.ascontiguousarray(PAIRS[ds], np.int32)
        row = np.empty(NUM_KEYPOINTS[e], np.int32)
        assert lib.vp_dbg_flip_partner(NUM_KEYPOINTS[e], p.ctypes.data, len(p), row.ctypes.data) == capi.VP_OK
        tab[e, :NUM_KEYPOINTS[e]] = row
    return np.ascontiguousarray(tab)


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [False, True])
def test_fused_decode_of_a_mixed_chunk_equals_the_flip_decode_per_crop(shift):
    lib = capi.load_library()
    rng = np.random.default_rng(23)
    experts = np.array([0, 1, 1, 2, 4, 5, 5], np.int32)                   # 7 crops in expert order
    n = len(experts)
    ks = np.array([NUM_KEYPOINTS[e] for e in experts], np.int32)
    dst = rng.permutation(n).astype(np.int32)
    gaps = rng.integers(0, 9, size=n)
    first = (np.cumsum(np.r_[0, 2 * ks[:-1] + gaps[:-1]]) + 2).astype(np.int32)
    n_maps = int(first[-1] + 2 * ks[-1] + 4)
    hm = rng.normal(0.0, 0.05, size=(n_maps, 64, 48)).astype(np.float32)
    tab = partner_tables()
    corners = [(0, 0), (0, 47), (63, 0), (63, 47), (63, 46), (0, 1)]
    for j in range(n):
        K, part = ks[j], tab[experts[j]]
        for k in range(K):
            own, mir = hm[first[j] + k], hm[first[j] + K + part[k]]
            if (j * 5 + min(k, part[k])) % 7 == 0:                        # nowhere positive in the crop's map and in the mirror's map of its partner:
                own[...] = -np.abs(own) - 0.01                            # coordinates -1, the samples wrap into the neighbour joint (0 <-> K - 1 included)
                mir[...] = -np.abs(mir) - 0.01
            elif k % 3 == 0:                                              # a peak the mirror's noise cannot outvote, in a corner of the crop's own map
                y, x = corners[(j + k) % len(corners)]
                own[y, x] += 3.0 + 0.01 * k
    records = np.ascontiguousarray(np.stack([first, ks, dst, experts], 1), np.int32)
    wh = rng.integers(50, 2000, size=(n, 2)).astype(np.int32)
    out = np.full((n, KMAX, 3), np.nan, np.float32)
    capi.check(lib.vp_dbg_decode_flip_mix(0, hm.ctypes.data, n_maps, n, KMAX, records.ctypes.data, tab.ctypes.data, E, int(shift), wh.ctypes.data, out.ctypes.data))
    n_neg = 0
    for j in range(n):
        K = ks[j]
        pair = np.ascontiguousarray(hm[first[j]:first[j] + 2 * K].reshape(2, K, 64, 48))
        want = decode_flip_heatmaps(pair, PAIRS[DATASETS[experts[j]]], shift, wh[dst[j]][None])[0]
        assert np.array_equal(out[dst[j], :K].view(np.uint32), want.view(np.uint32)), f'crop {j} (expert {experts[j]})'   # the bits, whatever the values
        assert not out[dst[j], K:].view(np.uint32).any(), 'joints beyond K are written as +0'
        n_neg += int((want[:, 2] <= 0).sum())
    assert n_neg > 0                                                      # the negative-index wrap was exercised
    plain = np.empty((n, KMAX, 3), np.float32)
    rec3 = np.ascontiguousarray(records[:, :3])
    capi.check(lib.vp_dbg_decode_mix(0, hm.ctypes.data, n_maps, n, KMAX, rec3.ctypes.data, wh.ctypes.data, plain.ctypes.data))
    assert not np.array_equal(out, plain, equal_nan=True)                 # not the decode of the crops' own maps

    def refused(rec, n_experts=E):
        rec = np.ascontiguousarray(rec, np.int32)
        return lib.vp_dbg_decode_flip_mix(0, hm.ctypes.data, n_maps, n, KMAX, rec.ctypes.data, tab.ctypes.data, n_experts, int(shift), None, out.ctypes.data)

    bad = records.copy()
    bad[-1, 0] = n_maps - 2 * ks[-1] + 1                                  # the mirror's last map lies beyond the buffer
    assert refused(bad) == capi.VP_ERR_INVALID
    bad = records.copy()
    bad[0, 2] = n                                                         # a destination outside [0, n)
    assert refused(bad) == capi.VP_ERR_INVALID
    bad = records.copy()
    bad[0, 2] = bad[1, 2]                                                 # two records, one destination
    assert refused(bad) == capi.VP_ERR_INVALID
    bad = records.copy()
    bad[0, 3] = E                                                         # an expert outside the table
    assert refused(bad) == capi.VP_ERR_INVALID
    assert refused(records) == capi.VP_OK


# ---- 2. end to end against the split handles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [False, True])
def test_mixed_call_under_the_mode_is_bit_identical_to_split_handles(one_launch_family, shift):
    """max_batch 16: chunks of 8 crops, 16 forward rows.  3 crops (one chunk), 8 (a full one), 19 (8 + 8 + 3); every pattern; three calls each (eager, capture,
    replay) through infer_mixed and through infer_mixed_device on torch's default stream."""
    torch = _torch()
    crops = crops48()
    rng = np.random.default_rng(31)
    eng = mode_handle(shift=shift)
    assert eng.flip_test and eng.flip_test_per_dataset
    results = []
    for n in (3, 8, 19):
        d_out = torch.empty((n, KMAX, 3), device='cuda')
        for name, ids in patterns(n):
            idx = rng.choice(len(crops), size=n, replace=False)
            d_crops = torch.from_numpy(crops[idx]).cuda()
            for rep in range(3):
                out, ks = eng.infer_mixed(crops[idx], ids)
                results.append((f'host n={n} {name} call {rep}', ids, idx, out, ks))
            for rep in range(3):
                results.append((f'device n={n} {name} call {rep}', ids, idx, run_device(eng, d_crops, ids, d_out, None), eng.dataset_k(ids)))
    eng.close()
    ref = split_refs(shift)
    for what, ids, idx, out, ks in results:
        assert out.shape == (len(ids), KMAX, 3), what
        check_mixed(out, ks, ids, idx, ref)


# ---- 3. a chunk of one expert ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_one_expert_call_has_the_bits_of_set_dataset_and_infer(dtype):
    """the same n in both runs, so the same plan: no cross-batch identity is needed (bf16 has none)"""
    crops = crops48()
    eng = mode_handle(dtype=dtype, shift=True)
    for e in (1, 5):
        for n in (5, 11):                                                 # one chunk; 8 + 3
            out, ks = eng.infer_mixed(crops[:n], np.full(n, e, np.int32))
            eng.set_dataset(DATASETS[e])
            assert eng.flip_test_per_dataset and eng.K == NUM_KEYPOINTS[e]
            want = eng.infer(crops[:n])
            assert (ks == NUM_KEYPOINTS[e]).all() and np.array_equal(out[:, :NUM_KEYPOINTS[e]], want), (dtype, e, n)
            assert not out[:, NUM_KEYPOINTS[e]:].any()
    eng.close()


# ---- 4. the twins ------------------------------------------------------------------------------------------------------------------------------
def test_frames_and_device_twins_equal_infer_mixed_under_the_mode():
    torch = _torch()
    from oracle import vitpose_cpu as O
    from test_gpu_frames import host_crops, matrix
    frames, p9 = matrix()
    n = len(p9)
    eng = mode_handle(max_batch=8)                                        # chunks of 4 crops straddle frames
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    crops = host_crops(frames, p9)
    d_out = torch.empty((n, KMAX, 3), device='cuda')
    for name, ids in patterns(n):
        want, wk = eng.infer_mixed(crops, ids, p9[:, 7:9])
        for fr in (frames, d_frames):
            got, ks = eng.infer_frames(fr, p9, datasets=ids)
            assert got.shape == (n, KMAX, 3) and np.array_equal(ks, wk)
            assert np.array_equal(got, want), f'{name}: {(got != want).sum()} differing values'
        d_wh = torch.from_numpy(np.ascontiguousarray(p9[:, 7:9])).cuda()
        assert np.array_equal(run_device(eng, torch.from_numpy(crops).cuda(), ids, d_out, None, d_wh), want), name   # uint8 device crops
    f32 = np.ascontiguousarray(np.concatenate([O.pre_img(c)[0] for c in crops[:7]]), np.float32)                    # float32 crops, host and device
    ids = patterns(7)[1][1]
    want, _ = eng.infer_mixed(f32, ids)
    d7 = torch.empty((7, KMAX, 3), device='cuda')
    assert np.array_equal(run_device(eng, torch.from_numpy(f32).cuda(), ids, d7, None), want)
    assert want[:, :14, 2].any()
    eng.close()


def test_boxes_twin_equals_its_host_route_under_the_mode(one_launch_family):
    """19 boxes at max_batch 8 (chunks of 4 on the handle's stream), 7 and 1 on the caller's stream; then statuses 1, 2 and 3 between good rows of several
    datasets: zero rows for them, the good rows as the host route computes them without the bad ones (one-launch family)"""
    torch = _torch()
    from test_gpu_boxes import scene, to_dev
    frames, boxes, fidx = scene()
    d_frames, d_boxes, d_fidx = to_dev(frames, boxes, fidx)
    n = len(boxes)
    eng = mode_handle(max_batch=8)
    interleaved = patterns(n)[1][1]
    for name, ids in patterns(n)[1:3]:                                     # interleaved, blocks
        for sel in (slice(None), slice(0, 7), slice(4, 5)):
            want, p9 = boxes_host_route(eng, d_frames, boxes[sel], fidx[sel], ids[sel])
            for rep in range(3):
                out, cp, st = eng.infer_boxes(d_frames, d_boxes[sel], d_fidx[sel], crop_params=True, status=True, datasets=ids[sel])
                torch.cuda.current_stream().synchronize()
                got = out.cpu().numpy()
                assert np.array_equal(got, want), f'{name} {sel} call {rep}: {(got != want).sum()} differing values'
                assert np.array_equal(cp.cpu().numpy(), p9) and not st.any().item()
    bad_boxes = np.array([[10, 10, 50, 50, 1, 0], [np.nan, 10, 50, 50, 1, 0], [300, 300, 250, 250, 1, 0]], np.float32)
    bad_fidx = np.array([7, 0, 2], np.int32)
    mixed_b = np.concatenate([boxes[:3], bad_boxes[:2], boxes[3:6], bad_boxes[2:]])
    mixed_f = np.concatenate([fidx[:3], bad_fidx[:2], fidx[3:6], bad_fidx[2:]])
    is_good = np.array([1, 1, 1, 0, 0, 1, 1, 1, 0], bool)
    ids = np.array([5, 0, 3, 5, 1, 0, 5, 2, 4], np.int32)
    want, _ = boxes_host_route(eng, d_frames, mixed_b[is_good], mixed_f[is_good], ids[is_good])
    for rep in range(3):
        out, st = eng.infer_boxes(d_frames, torch.from_numpy(mixed_b).cuda(), torch.from_numpy(mixed_f).cuda(), status=True, datasets=ids)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert st.cpu().numpy().tolist() == [0, 0, 0, 1, 2, 0, 0, 0, 3]
        assert (got[~is_good] == 0).all() and np.array_equal(got[is_good], want), f'call {rep}'
    eng.clear_flip_test()
    off = eng.infer_boxes(d_frames, d_boxes, d_fidx, datasets=interleaved).cpu().numpy()
    eng.set_flip_test_datasets(PAIRS)
    on = eng.infer_boxes(d_frames, d_boxes, d_fidx, datasets=interleaved).cpu().numpy()
    assert not np.array_equal(on, off)
    eng.close()


# ---- 5. the 8-phase tile path --------------------------------------------------------------------------------------------------------------------
def test_vitpose_b_128_crops_on_the_8_phase_fc2_tiles(one_launch_family):
    """ViTPose-B, max_batch 256: 128 crops are one chunk of 256 forward rows.  All-even crop counts keep mlp.fc2's 256-row tile on the doubled bounds, an odd
    count moves it to the crop-aligned 192-row tile; both are the 8-phase kernel, and both equal the split handles."""
    p = pool()
    crops = np.ascontiguousarray(np.concatenate([p[:64], p[150:214]]))
    experts = (0, 1, 5)
    runs = {'even': np.repeat(experts, (44, 42, 42)).astype(np.int32), 'odd': np.repeat(experts, (43, 43, 42)).astype(np.int32)}
    rng = np.random.default_rng(5)
    for ids in runs.values():
        rng.shuffle(ids)
    eng = mode_handle('b', 'fp16', 256)
    got = {}
    for name, ids in runs.items():
        got[name] = eng.infer_mixed(crops, ids)
        assert 'gemm8_kernel' in eng.profile_kernel('gemm_fc2'), (name, eng.profile_kernel('gemm_fc2'))
    eng.close()
    ref = {}
    for e in experts:
        h = split_handle('b', DATASETS[e], 'fp16', 256)
        h.set_flip_test(PAIRS[DATASETS[e]])
        ref[e] = h.infer(crops)
        h.close()
    for name, ids in runs.items():
        check_mixed(got[name][0], got[name][1], ids, np.arange(len(ids)), ref)


# ---- 6. the mode's bookkeeping ---------------------------------------------------------------------------------------------------------------
def test_mode_bookkeeping(one_launch_family):
    torch = _torch()
    crops = crops48()
    ref = split_refs(False)
    ids = np.array([0, 5, 3, 5, 1], np.int32)
    eng = expert_handle('s', 'fp16', 16)
    plain = eng.infer(crops[:5])
    plain_mixed = eng.infer_mixed(crops[:5], ids)[0]
    assert not eng.flip_test and not eng.flip_test_per_dataset and eng.lib.vp_flip_test_enabled(eng._h) == 0
    eng.set_flip_test_datasets({e if e % 2 else ds: PAIRS[ds] for e, ds in enumerate(DATASETS)})   # names and expert indices
    assert eng.flip_test is True and eng.flip_test_per_dataset and eng.lib.vp_flip_test_enabled(eng._h) == 2
    for ds in ('coco', 'wholebody', 'aic'):                               # K = 17 -> 133 -> 14: the mode stays, each under its own table
        eng.set_dataset(ds)
        e = DATASETS.index(ds)
        assert eng.flip_test_per_dataset and eng.K == NUM_KEYPOINTS[e] and eng.dataset == ds
        assert np.array_equal(eng.infer(crops[:5]), ref[e][:5]), ds
    first = eng.infer_mixed(crops[:5], ids)
    assert eng.dataset == 'aic' and eng.K == 14                           # the active dataset survives a mixed call
    check_mixed(first[0], first[1], ids, np.arange(5), ref)
    for _ in range(3):                                                    # run to run (eager, capture, replay)
        assert np.array_equal(eng.infer_mixed(crops[:5], ids)[0], first[0])
    assert not np.array_equal(first[0], plain_mixed)
    # a second set with a changed table misses the graph captured under the first one
    d_crops, d_out = torch.from_numpy(crops[:5]).cuda(), torch.empty((5, KMAX, 3), device='cuda')
    for _ in range(3):
        assert np.array_equal(run_device(eng, d_crops, ids, d_out, None), first[0])
    other = dict(PAIRS, coco=[[0, 16], [5, 6]], wholebody=[[3, 90]])
    eng.set_flip_test_datasets(other)
    changed = [run_device(eng, d_crops, ids, d_out, None) for _ in range(3)]
    fresh = mode_handle(pairs=other)
    want = fresh.infer_mixed(crops[:5], ids)[0]
    fresh.close()
    assert all(np.array_equal(c, want) for c in changed) and not np.array_equal(want, first[0])
    assert np.array_equal(want[[2, 4]], first[0][[2, 4]])                # ap10k's and aic's tables did not change
    # clear: the plain bits again; the single-table mode afterwards refuses the per-crop entries as documented
    eng.clear_flip_test()
    assert not eng.flip_test and not eng.flip_test_per_dataset
    assert np.array_equal(eng.infer_mixed(crops[:5], ids)[0], plain_mixed)
    eng.set_dataset('coco')
    assert np.array_equal(eng.infer(crops[:5]), plain)
    eng.set_flip_test_datasets(PAIRS)
    eng.set_flip_test(COCO_PAIRS)
    assert eng.flip_test and not eng.flip_test_per_dataset and eng.lib.vp_flip_test_enabled(eng._h) == 1
    with pytest.raises(capi.VpError, match='one partner table per handle') as ei:
        eng.infer_mixed(crops[:5], ids)
    assert ei.value.code == capi.VP_ERR_STATE
    assert np.array_equal(eng.infer(crops[:5]), ref[0][:5])
    with pytest.raises(capi.VpError, match='cleared'):                    # and clears on a change of K, as before
        eng.set_dataset('wholebody')
    assert not eng.flip_test
    eng.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    crops = crops48()[:3]
    ids = np.array([0, 5, 1], np.int32)
    counts = np.array([len(PAIRS[ds]) for ds in DATASETS], np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(PAIRS[ds], np.int32).reshape(-1, 2) for ds in DATASETS]))
    plain = split_handle('s', 'coco', 'fp16', 4)
    before = plain.infer(crops)
    assert plain.lib.vp_set_flip_test_experts(plain._h, flat.ctypes.data, counts.ctypes.data, 0) == capi.VP_ERR_STATE
    assert 'plain' in capi.last_error(plain._h)
    with pytest.raises(capi.VpError) as ei:
        plain.set_flip_test_datasets(PAIRS)
    assert ei.value.code == capi.VP_ERR_STATE and not plain.flip_test and np.array_equal(plain.infer(crops), before)
    plain.close()

    one = expert_handle('s', 'fp16', 1)
    before = one.infer_mixed(crops, ids)[0]
    with pytest.raises(capi.VpError, match='max_batch') as ei:
        one.set_flip_test_datasets(PAIRS)
    assert ei.value.code == capi.VP_ERR_STATE and not one.flip_test and np.array_equal(one.infer_mixed(crops, ids)[0], before)
    one.close()

    eng = expert_handle('s', 'fp16', 8)
    lib, h = eng.lib, eng._h
    before = eng.infer_mixed(crops, ids)[0]

    def untouched():
        return not eng.flip_test and np.array_equal(eng.infer_mixed(crops, ids)[0], before)

    missing = {ds: PAIRS[ds] for ds in DATASETS if ds != 'mpii'}
    with pytest.raises(ValueError, match='mpii'):                         # before the C call: the library has no error to report
        eng.set_flip_test_datasets(missing)
    with pytest.raises(ValueError, match='coco_25'):
        eng.set_flip_test_datasets(dict(PAIRS, coco_25=[]))
    with pytest.raises(ValueError, match='twice'):
        eng.set_flip_test_datasets({**PAIRS, 0: COCO_PAIRS})
    assert untouched()
    with pytest.raises(capi.VpError, match=r'expert 1: flip pair 2 = \(2, 14\)') as ei:   # aic has 14 joints: 0 .. 13
        eng.set_flip_test_datasets(dict(PAIRS, aic=[[0, 3], [1, 4], [2, 14]]))
    assert ei.value.code == capi.VP_ERR_INVALID and untouched()
    neg = counts.copy()
    neg[2] = -1
    assert lib.vp_set_flip_test_experts(h, flat.ctypes.data, neg.ctypes.data, 0) == capi.VP_ERR_INVALID and 'expert 2' in capi.last_error(h)
    assert lib.vp_set_flip_test_experts(h, flat.ctypes.data, None, 0) == capi.VP_ERR_INVALID
    assert lib.vp_set_flip_test_experts(h, None, counts.ctypes.data, 0) == capi.VP_ERR_INVALID
    assert untouched()
    # a refused set while the mode is on leaves THAT mode on, with its table
    eng.set_flip_test_datasets(PAIRS)
    on = eng.infer_mixed(crops, ids)[0]
    assert lib.vp_set_flip_test_experts(h, flat.ctypes.data, neg.ctypes.data, 1) == capi.VP_ERR_INVALID
    assert eng.flip_test_per_dataset and np.array_equal(eng.infer_mixed(crops, ids)[0], on) and not np.array_equal(on, before)
    zero = np.zeros(E, np.int32)
    assert lib.vp_set_flip_test_experts(h, None, zero.ctypes.data, 0) == capi.VP_OK   # no pairs at all is a valid table per expert
    assert eng.flip_test_per_dataset
    eng.close()
