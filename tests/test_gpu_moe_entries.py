"""GPU: per-crop datasets on the production entries of a ViTPose+ handle -- vp_infer_experts_device_stream (VitPoseHip.infer_mixed_device),
vp_infer_frames_experts (infer_frames(datasets=)) and vp_infer_boxes_experts_stream (infer_boxes(datasets=)).  Every comparison is bit for bit, fp16:
against infer_mixed on the same crops, ids and max_batch (same chunks, same plan), across eager run, graph capture and replay, on three streams; a new
permutation under a captured graph; the fused decode's record route alone against vp_decode_only; datasets=None against the plain entries; refusals;
and the reference's keypoints within the suite's tolerance.  The plan itself is pinned on the CPU (tests/test_mix_plan_host.py).

vp_infer_experts (infer_mixed) is the host-staged caller of the same chunk body as these entries, so "entry == infer_mixed" compares one body under two
stagings.  The anchor of every per-crop entry is tests/test_gpu_moe.py's comparison of infer_mixed with the six split handles (and, for the device-stream
entry directly, test_device_stream_entry_is_bit_identical_to_split_handles below)."""
from __future__ import annotations

import os

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.cropprep import frames_crop_params
from easy_vitpose_amd.engine import PinnedArray, decode_heatmaps
from easy_vitpose_amd.moe import DATASETS, NUM_KEYPOINTS
from helpers import CONF_TOL, KP_TOL_PX
from test_gpu_moe import check_mixed, expert_handle, patterns, pool, split_handle

pytestmark = pytest.mark.gpu
KMAX = max(NUM_KEYPOINTS)


def _torch():
    import torch
    return torch


def streams_of(eng):
    """(name, stream argument) of the three kinds of caller stream: torch's default, a side stream, the handle's own"""
    torch = _torch()
    return [('default', None), ('side', torch.cuda.Stream()), ('own', int(eng.lib.vp_stream(eng._h)))]


def run_device(eng, d_crops, ids, d_out, stream, d_wh=None):
    torch = _torch()
    torch.cuda.synchronize()   # the inputs are complete whichever stream the call is ordered on
    d_out.fill_(float('nan'))
    torch.cuda.synchronize()
    eng.infer_mixed_device(d_crops, ids, d_out, org_wh=d_wh, stream=stream)
    eng.synchronize()
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


# ---- 1. the device-stream entry against infer_mixed ----------------------------------------------------------------------------------
@pytest.mark.parametrize('variant,sizes,max_batch', [('s', (1, 3, 8, 13, 16, 37, 64, 100), 64), ('b', (120, 256, 300), 256)])
def test_device_stream_entry_equals_infer_mixed(variant, sizes, max_batch):
    """same crops, ids and max_batch -> same chunks and plan: every row equal to infer_mixed's, three calls in a row per stream (chunks of <= 16 crops: eager,
    capture, replay), on torch's default stream, a side stream and the handle's own"""
    torch = _torch()
    crops = pool()
    rng = np.random.default_rng(7)
    eng = expert_handle(variant, 'fp16', max_batch)
    streams = streams_of(eng)
    for n in sizes:
        d_out = torch.empty((n, KMAX, 3), device='cuda')   # one output buffer per size: a repeated call meets the same graph key
        for name, ids in patterns(n):
            idx = rng.choice(len(crops), size=n, replace=False)
            wh = rng.integers(100, 900, size=(n, 2)).astype(np.int32) if name == 'interleaved' else None
            want, ks = eng.infer_mixed(crops[idx], ids, wh)
            d_crops = torch.from_numpy(crops[idx]).cuda()
            d_wh = None if wh is None else torch.from_numpy(wh).cuda()
            for sname, stream in streams:
                for rep in range(3):
                    got = run_device(eng, d_crops, ids, d_out, stream, d_wh)
                    assert np.array_equal(got, want), f'{variant} n={n} {name} stream={sname} call {rep}: {(got != want).sum()} differing values'
            assert np.array_equal(ks, eng.dataset_k(ids))
    eng.close()


def test_device_stream_entry_is_bit_identical_to_split_handles(one_launch_family):
    """the device-stream entry against the split model's six handles, not against its host-staged twin: 3 and 13 crops (one mixed chunk), 37 (two full
    chunks of 16 and a ragged 5) at max_batch 16, every pattern, three calls each on torch's default stream (eager, capture, replay)"""
    torch = _torch()
    crops = pool()
    rng = np.random.default_rng(11)
    eng = expert_handle('s', 'fp16', 16)
    results = []
    for n in (3, 13, 37):
        d_out = torch.empty((n, KMAX, 3), device='cuda')
        for name, ids in patterns(n):
            idx = rng.choice(len(crops), size=n, replace=False)
            d_crops = torch.from_numpy(crops[idx]).cuda()
            ks = eng.dataset_k(ids)
            results += [(n, name, rep, ids, idx, run_device(eng, d_crops, ids, d_out, None), ks) for rep in range(3)]
    eng.close()
    ref = {}
    for e, ds in enumerate(DATASETS):
        h = split_handle('s', ds, 'fp16', 16)
        ref[e] = h.infer(crops)
        h.close()
    for n, name, rep, ids, idx, out, ks in results:
        assert out.shape == (n, KMAX, 3), (n, name, rep)
        check_mixed(out, ks, ids, idx, ref)


# ---- 2. same counts, another permutation: the captured graph with new tables ------------------------------------------------------------
@pytest.mark.parametrize('n', [5, 8, 16])
def test_a_new_permutation_replays_the_graph_and_other_counts_do_not(n):
    torch = _torch()
    crops = pool()[:n]
    rng = np.random.default_rng(n)
    base = np.array([0, 5, 3, 5, 1, 2, 4, 0, 0, 3, 3, 5, 1, 1, 2, 0][:n], np.int32)
    perms = [rng.permutation(base).astype(np.int32) for _ in range(3)]
    other = base.copy()
    other[0] = 4   # one crop of coco becomes apt36k: other counts, other head segments
    one = np.full(n, 2, np.int32)
    eng = expert_handle('s', 'fp16', 16)
    seq = [base, base, base, perms[0], perms[1], other, perms[2], other, other, one, one, one, base[::-1].copy(), other[::-1].copy()]
    want = [eng.infer_mixed(crops, ids)[0] for ids in seq]
    d_crops = torch.from_numpy(crops).cuda()
    d_out = torch.empty((n, KMAX, 3), device='cuda')
    for i, ids in enumerate(seq):
        got = run_device(eng, d_crops, ids, d_out, None)
        assert np.array_equal(got, want[i]), f'call {i} ({ids.tolist()})'
        for r, e in enumerate(ids):
            assert not got[r, NUM_KEYPOINTS[e]:].any() and got[r, :NUM_KEYPOINTS[e], 2].any()
    eng.close()


# ---- 3. the frames entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_batch', [4, 8, 32])
def test_frames_entry_equals_infer_mixed_on_host_prepared_crops(max_batch):
    torch = _torch()
    from test_gpu_frames import host_crops, matrix
    frames, p9 = matrix()
    n = len(p9)
    eng = expert_handle('s', 'fp16', max_batch)
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    crops = host_crops(frames, p9)
    for name, ids in patterns(n):
        want, wk = eng.infer_mixed(crops, ids, p9[:, 7:9])
        for fr in (frames, d_frames, frames):
            got, ks = eng.infer_frames(fr, p9, datasets=ids)
            assert got.shape == (n, KMAX, 3) and np.array_equal(ks, wk)
            assert np.array_equal(got, want), f'max_batch {max_batch} {name}: {(got != want).sum()} differing values'
    got, _ = eng.infer_frames(frames, p9, datasets=[DATASETS[e] for e in patterns(n)[1][1]])   # names as well as indices
    assert np.array_equal(got, eng.infer_mixed(crops, patterns(n)[1][1], p9[:, 7:9])[0])
    eng.close()


# ---- 4. the boxes entry -----------------------------------------------------------------------------------------------------------------
def boxes_host_route(eng, d_frames, boxes, fidx, ids, pad=10):
    """boxes to the host, frames_crop_params, infer_frames(datasets=), the offsets added on the host as VitInference.inference_frames adds them"""
    p9 = np.concatenate([np.zeros((0, 9), np.int32)] + [frames_crop_params([b[None, :4].astype(np.float64)], [tuple(d_frames[f].shape)], pad)
                                                        for b, f in zip(boxes, fidx)])
    p9[:, 0] = fidx
    kps, ks = eng.infer_frames(d_frames, p9, datasets=ids)
    for k, p, K in zip(kps, p9[:, 1:], ks):
        k[:K, :2] += np.array([p[1] - p[5], p[0] - p[4]])
    return kps, p9


def test_boxes_entry_equals_the_host_route():
    torch = _torch()
    from test_gpu_boxes import scene, to_dev
    frames, boxes, fidx = scene()
    d_frames, d_boxes, d_fidx = to_dev(frames, boxes, fidx)
    n = len(boxes)
    eng = expert_handle('s', 'fp16', 8)   # 19 boxes: chunks of 8, 8, 3 on the handle's stream
    for name, ids in patterns(n):
        for sel in (slice(None), slice(0, 7), slice(4, 5)):   # and the caller-stream path (<= 16 boxes)
            want, p9 = boxes_host_route(eng, d_frames, boxes[sel], fidx[sel], ids[sel])
            plain_cp, plain_st = eng.infer_boxes(d_frames, d_boxes[sel], d_fidx[sel], crop_params=True, status=True)[1:]
            for rep in range(3):
                out, cp, st = eng.infer_boxes(d_frames, d_boxes[sel], d_fidx[sel], crop_params=True, status=True, datasets=ids[sel])
                torch.cuda.current_stream().synchronize()
                got = out.cpu().numpy()
                assert got.shape == (len(want), KMAX, 3)
                assert np.array_equal(got, want), f'{name} {sel} call {rep}: {(got != want).sum()} differing values'
                assert np.array_equal(cp.cpu().numpy(), p9) and torch.equal(cp, plain_cp) and torch.equal(st, plain_st) and not st.any().item()
    eng.close()


def test_boxes_entry_rows_with_a_status_inside_a_mix(one_launch_family):
    """statuses 1, 2 and 3 between good rows of several datasets: zero keypoints and params for them, the plain entry's params and status for all rows, and
    the good rows as the host route computes them without the bad ones (one-launch family: a crop's bits do not depend on its batch)"""
    torch = _torch()
    from test_gpu_boxes import scene
    frames, boxes, fidx = scene()
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    bad_boxes = np.array([[10, 10, 50, 50, 1, 0], [np.nan, 10, 50, 50, 1, 0], [10, 10, 50, np.inf, 1, 0], [-300, 10, -100, 50, 1, 0],
                          [300, 300, 250, 250, 1, 0]], np.float32)
    bad_fidx = np.array([7, 0, 1, 0, 2], np.int32)
    mixed_b = np.concatenate([boxes[:3], bad_boxes[:2], boxes[3:6], bad_boxes[2:]])
    mixed_f = np.concatenate([fidx[:3], bad_fidx[:2], fidx[3:6], bad_fidx[2:]])
    is_good = np.array([1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0], bool)
    ids = np.array([5, 0, 3, 5, 1, 0, 5, 2, 4, 0, 5], np.int32)
    for max_batch in (16, 4):
        eng = expert_handle('s', 'fp16', max_batch)
        d_b, d_f = torch.from_numpy(mixed_b).cuda(), torch.from_numpy(mixed_f).cuda()
        plain_cp, plain_st = eng.infer_boxes(d_frames, d_b, d_f, crop_params=True, status=True)[1:]
        want, _ = boxes_host_route(eng, d_frames, mixed_b[is_good], mixed_f[is_good], ids[is_good])
        for rep in range(3):
            out, cp, st = eng.infer_boxes(d_frames, d_b, d_f, crop_params=True, status=True, datasets=ids)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert st.cpu().numpy().tolist() == [0, 0, 0, 1, 2, 0, 0, 0, 2, 3, 3]
            assert torch.equal(cp, plain_cp) and torch.equal(st, plain_st)
            assert (got[~is_good] == 0).all() and (cp.cpu().numpy()[~is_good] == 0).all()
            assert np.array_equal(got[is_good], want), f'max_batch {max_batch} call {rep}'
        eng.close()


# ---- 5. the record route of the decode kernel alone -------------------------------------------------------------------------------------
def test_decode_record_route_equals_decode_only_per_crop():
    rng = np.random.default_rng(19)
    lib = capi.load_library()
    ks = np.array([133, 14, 17, 16, 133, 17, 14, 16, 17], np.int32)
    n = len(ks)
    dst = rng.permutation(n).astype(np.int32)
    gaps = rng.integers(0, 40, size=n)
    first = (np.cumsum(np.r_[0, ks[:-1] + gaps[:-1]]) + 3).astype(np.int32)
    n_maps = int(first[-1] + ks[-1] + 5)
    hm = rng.normal(0.0, 0.05, size=(n_maps, 64, 48)).astype(np.float32)
    for j in range(n):   # a peak per map; corners and edges, flat ties, and maps that are nowhere positive
        for k in range(ks[j]):
            m = hm[first[j] + k]
            y, x = [(0, 0), (63, 47), (0, 47), (63, 0), (rng.integers(64), rng.integers(48))][(j + k) % 5]
            if (j * 7 + k) % 11 == 0:
                m[...] = -np.abs(m) - 0.01 * ((j + k) % 3)   # max <= 0: the reference's coords = -1 and its wrap into the neighbouring map
            elif (j + k) % 13 == 0:
                m[...] = 0.25                                # all equal: the first index wins
            else:
                yy, xx = np.mgrid[0:64, 0:48]
                m += np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / 8.0).astype(np.float32)
    records = np.ascontiguousarray(np.stack([first, ks, dst], 1), np.int32)
    wh = rng.integers(50, 2000, size=(n, 2)).astype(np.int32)
    for org_wh in (None, wh):
        out = np.empty((n, KMAX, 3), np.float32)
        capi.check(lib.vp_dbg_decode_mix(0, hm.ctypes.data, n_maps, n, KMAX, records.ctypes.data, None if org_wh is None else org_wh.ctypes.data, out.ctypes.data))
        for j in range(n):
            maps = np.ascontiguousarray(hm[first[j]:first[j] + ks[j]][None])
            want = decode_heatmaps(maps, None if org_wh is None else org_wh[dst[j]][None])[0]
            assert np.array_equal(out[dst[j], :ks[j]].view(np.uint32), want.view(np.uint32)), f'crop {j} (K {ks[j]})'   # the bits, whatever the values
            assert not out[dst[j], ks[j]:].view(np.uint32).any(), 'joints beyond K are written as +0'
    bad = records.copy()
    bad[0, 2] = bad[1, 2]   # two crops into one row
    assert lib.vp_dbg_decode_mix(0, hm.ctypes.data, n_maps, n, KMAX, bad.ctypes.data, None, out.ctypes.data) == capi.VP_ERR_INVALID
    bad = records.copy()
    bad[-1, 0] = n_maps - 3   # maps beyond the buffer
    assert lib.vp_dbg_decode_mix(0, hm.ctypes.data, n_maps, n, KMAX, bad.ctypes.data, None, out.ctypes.data) == capi.VP_ERR_INVALID


# ---- 6. mode interactions and refusals --------------------------------------------------------------------------------------------------
def test_datasets_none_is_the_plain_entry_and_the_active_dataset_survives_a_mixed_call():
    torch = _torch()
    from test_gpu_boxes import scene, to_dev
    from test_gpu_frames import matrix
    frames, p9 = matrix()
    sframes, boxes, fidx = scene()
    d_sframes, d_boxes, d_fidx = to_dev(sframes, boxes, fidx)
    crops = pool()[:len(p9)]
    ids = (np.arange(len(p9)) % 6).astype(np.int32)
    eng = expert_handle('s', 'fp16', 8)
    eng.set_dataset('aic')
    lib, h, n, nb = eng.lib, eng._h, len(p9), len(boxes)

    def plain():
        table = (capi.vp_frame * len(frames))(*[capi.vp_frame(f.ctypes.data, f.shape[0], f.shape[1]) for f in frames])
        a = np.empty((n, 14, 3), np.float32)
        capi.check(lib.vp_infer_frames(h, table, len(frames), 0, p9.ctypes.data, n, a.ctypes.data), h)
        btable = (capi.vp_frame * len(d_sframes))(*[capi.vp_frame(f.data_ptr(), f.shape[0], f.shape[1]) for f in d_sframes])
        b = torch.empty((nb, 14, 3), device='cuda')
        capi.check(lib.vp_infer_boxes_stream(h, btable, len(d_sframes), d_boxes.data_ptr(), 6, d_fidx.data_ptr(), nb, 10, b.data_ptr(), None, None,
                                             torch.cuda.current_stream().cuda_stream), h)
        torch.cuda.synchronize()
        return a, b.cpu().numpy(), eng.infer(crops)

    before = plain()
    assert np.array_equal(eng.infer_frames(frames, p9), before[0]) and np.array_equal(eng.infer_frames(frames, p9, datasets=None), before[0])
    assert np.array_equal(eng.infer_boxes(d_sframes, d_boxes, d_fidx, datasets=None).cpu().numpy(), before[1])
    # a mixed call through each entry, then the plain entries again: dataset and K as before, the same bits
    d_out = torch.empty((n, KMAX, 3), device='cuda')
    run_device(eng, torch.from_numpy(crops).cuda(), ids, d_out, None)
    eng.infer_frames(frames, p9, datasets=ids)
    eng.infer_boxes(d_sframes, d_boxes, d_fidx, datasets=(np.arange(nb) % 6).astype(np.int32))
    torch.cuda.synchronize()
    assert eng.dataset == 'aic' and eng.K == 14
    after = plain()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(eng.infer_boxes(d_sframes, d_boxes, d_fidx).cpu().numpy(), before[1])
    eng.close()


def test_refusals():
    torch = _torch()
    from test_gpu_boxes import scene, to_dev
    from test_gpu_frames import matrix
    frames, p9 = matrix()
    p9 = np.ascontiguousarray(p9[:2])
    sframes, boxes, fidx = scene()
    d_sframes, d_boxes, d_fidx = to_dev(sframes, boxes[:2], fidx[:2])
    crops = pool()[:2]
    d_crops = torch.from_numpy(crops).cuda()
    d_out = torch.full((2, KMAX, 3), 7.0, device='cuda')
    out = np.full((2, KMAX, 3), 7.0, np.float32)
    table = (capi.vp_frame * len(frames))(*[capi.vp_frame(f.ctypes.data, f.shape[0], f.shape[1]) for f in frames])
    btable = (capi.vp_frame * len(d_sframes))(*[capi.vp_frame(f.data_ptr(), f.shape[0], f.shape[1]) for f in d_sframes])

    def calls(eng, ids):
        lib, h = eng.lib, eng._h
        p = None if ids is None else ids.ctypes.data
        return [lib.vp_infer_experts_device_stream(h, d_crops.data_ptr(), capi.VP_INPUT_U8_NHWC, 2, p, None, d_out.data_ptr(), None),
                lib.vp_infer_frames_experts(h, table, len(frames), 0, p9.ctypes.data, 2, p, out.ctypes.data),
                lib.vp_infer_boxes_experts_stream(h, btable, len(d_sframes), d_boxes.data_ptr(), 6, d_fidx.data_ptr(), 2, 10, p, d_out.data_ptr(), None, None, None)]

    def untouched():
        torch.cuda.synchronize()
        return (d_out == 7.0).all().item() and (out == 7.0).all()

    ok = np.array([0, 5], np.int32)
    plain = split_handle('s', 'coco', 'fp16', 4)
    assert calls(plain, ok) == [capi.VP_ERR_STATE] * 3 and 'plain' in capi.last_error(plain._h) and untouched()
    with pytest.raises(capi.VpError) as ei:
        plain.infer_frames(frames, p9, datasets=ok)
    assert ei.value.code == capi.VP_ERR_STATE
    plain.close()

    eng = expert_handle('s', 'fp16', 4)
    for bad, at in ((np.array([0, 6], np.int32), 1), (np.array([-1, 0], np.int32), 0)):
        for rc in calls(eng, bad):
            assert rc == capi.VP_ERR_INVALID and f'of crop {at} ' in capi.last_error(eng._h)
    assert calls(eng, None) == [capi.VP_ERR_INVALID] * 3
    with pytest.raises(capi.VpError):
        eng.infer_mixed_device(d_crops, ['coco', 'coco_25'], d_out)
    assert untouched()
    eng.set_flip_test([[1, 2], [3, 4]])
    assert calls(eng, ok) == [capi.VP_ERR_STATE] * 3 and 'flip-test' in capi.last_error(eng._h) and untouched()
    eng.clear_flip_test()
    pin = PinnedArray(crops.shape, np.uint8)
    pin.array[:] = crops
    res = np.zeros((2, 17, 3), np.float32)
    slot = eng.submit(pin.array, res)
    rcs = calls(eng, ok)
    eng.wait(slot)
    pin.free()
    assert rcs == [capi.VP_ERR_STATE] * 3 and untouched()
    assert calls(eng, ok) == [capi.VP_OK] * 3   # and the handle works afterwards
    eng.synchronize()
    torch.cuda.synchronize()
    assert not (d_out == 7.0).any().item() and not (out == 7.0).any()
    # n = 0: nothing is written, whatever the pointers
    lib, h = eng.lib, eng._h
    d_out.fill_(7.0)
    assert lib.vp_infer_experts_device_stream(h, None, capi.VP_INPUT_U8_NHWC, 0, None, None, d_out.data_ptr(), None) == capi.VP_OK
    assert lib.vp_infer_boxes_experts_stream(h, None, 0, None, 4, None, 0, 10, None, d_out.data_ptr(), None, None, None) == capi.VP_OK
    assert lib.vp_infer_frames_experts(h, None, 0, 0, None, 0, None, out.ctypes.data) == capi.VP_OK
    eng.synchronize()
    assert (d_out == 7.0).all().item()
    eng.close()


# ---- 7. accuracy against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['s', 'b'])
@pytest.mark.parametrize('splitk', ['0', None])
def test_every_dataset_within_tolerance_of_the_reference_through_the_device_entry(golden_dir, monkeypatch, variant, splitk):
    """what test_gpu_moe.test_every_dataset_within_tolerance_of_the_reference asserts through infer_mixed / infer, through vp_infer_experts_device_stream"""
    torch = _torch()
    if splitk is not None:
        monkeypatch.setenv('VP_SPLITK', splitk)
    from cases import peaked_crops
    gold = {ds: np.load(os.path.join(golden_dir, f'moe_{variant}_{ds}.npz')) for ds in DATASETS}
    n = int(gold['coco']['n'])
    crops = peaked_crops(n)
    eng = expert_handle(variant, 'fp16', 64)
    d_out = torch.empty((6 * n, KMAX, 3), device='cuda')
    out = run_device(eng, torch.from_numpy(np.concatenate([crops] * 6)).cuda(), np.repeat(np.arange(6), n), d_out, None)   # one call, all six datasets
    single = []
    d_one = torch.empty((1, KMAX, 3), device='cuda')
    for ds in ('coco', 'wholebody'):   # and a one-dataset chunk of a small batch (split-K at its default)
        e = DATASETS.index(ds)
        single.append((ds, run_device(eng, torch.from_numpy(crops[:1]).cuda(), [ds], d_one, None)[:, :NUM_KEYPOINTS[e]].copy()))
    eng.close()
    for e, ds in enumerate(DATASETS):
        K = NUM_KEYPOINTS[e]
        kp, ref = out[e * n:(e + 1) * n, :K], gold[ds]['keypoints']
        dpx = np.abs(kp[..., :2] - ref[..., :2]).max()
        dcf = np.abs(kp[..., 2] - ref[..., 2]).max()
        print(f'[{variant}/{ds} splitk={splitk}] coordinate max err {dpx:.4f} px, confidence max err {dcf:.3e}')
        assert dpx < KP_TOL_PX and dcf < CONF_TOL, ds
        assert not out[e * n:(e + 1) * n, K:].any()
    for ds, kp in single:
        ref = gold[ds]['keypoints'][:1]
        assert np.abs(kp[..., :2] - ref[..., :2]).max() < KP_TOL_PX and np.abs(kp[..., 2] - ref[..., 2]).max() < CONF_TOL
