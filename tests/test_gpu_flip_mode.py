"""GPU: flip-test as a mode of the handle (vp_set_flip_test).  The crops and their mirror images run as one interleaved forward batch and the decode
averages a joint's two maps on the fly; every entry that goes through the chunk runner inherits the mode.  Against the CPU oracle, against the
materialised average (bit for bit), against the two-pass vp_infer_flip, entry by entry against `infer` under the mode (bit for bit, as
tests/test_gpu_frames.py and tests/test_gpu_boxes.py compare those entries without the mode), and the hipGraph keys across set / clear.

Tolerances are the project's own: HM_MAX_ERR / HM_RMS_ERR of tests/test_gpu_parity.py for heatmaps against the fp32 oracle, CONF_TOL of
tests/helpers.py for confidences, and the 2e-3 of "the same network with other rounding points" (test_gpu_parity.py: fused against standalone
LayerNorm, the mirror symmetry of vp_infer_flip): n crops under the mode are a 2 n batch, so other tiles may run than in two passes of n."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from easy_vitpose_amd import PinnedArray, VitPoseGroup, VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.engine import decode_flip_heatmaps, decode_heatmaps
from easy_vitpose_amd.synth import synthetic_crops, synthetic_state_dict
from helpers import CONF_TOL, weights
from oracle import vitpose_cpu as O

pytestmark = pytest.mark.gpu

HM_MAX_ERR = {'fp16': 4e-3}    # tests/test_gpu_parity.py:26-27
HM_RMS_ERR = {'fp16': 6e-4}
SAME_NET_TOL = 2e-3            # tests/test_gpu_parity.py:457, 493

COCO_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
# wholebody's 133 joints: the first and the last joint paired with inner ones (the DARK samples of joint 0 / 132 wrap into joint 132 / 0, whose partners are
# 40 / 7), a pair of neighbours, a pair across the range -- and 123 joints that are their own partner
WB_PAIRS = [[0, 7], [132, 40], [1, 2], [60, 61], [5, 131]]


def merged_on_host(hm2, pairs, shift):
    """0.5 (crop + shifted flip_back(mirror)) of an interleaved [2 n, K, 64, 48] tensor in fp32: the same add and exact multiply as the device's"""
    a, b = hm2[0::2], O.flip_back(hm2[1::2], pairs).copy()
    if shift:
        b[..., 1:] = b.copy()[..., :-1]
    return np.float32(0.5) * (a + b)


# ------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize('shift', [False, True])
def test_mode_matches_oracle(shift):
    shp, sd, sdt = weights('s', 'coco')
    crops = synthetic_crops(5, 13, 'blobs')
    x = np.concatenate([O.pre_img(c)[0] for c in crops])
    ref_hm = O.flip_test_heatmaps(sdt, x, shp.depth, shp.num_heads, COCO_PAIRS, shift_heatmap=shift)
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)             # 5 crops -> chunks of 2 + 2 + 1 (a crop and its mirror share the batch)
    eng.set_flip_test(COCO_PAIRS, shift_heatmap=shift)
    assert eng.flip_test
    hm, kp = eng.heatmaps(crops), eng.infer(crops)
    eng.close()
    err = np.abs(hm - ref_hm)
    conf_err = np.abs(kp[..., 2] - O.decode_per_crop(ref_hm)[..., 2])
    print(f'flip mode (shift={shift}): heatmap max|err| {err.max():.3e} rms {np.sqrt((err ** 2).mean()):.3e} confidence max|err| {conf_err.max():.3e}')
    assert hm.shape == ref_hm.shape == (5, 17, 64, 48) and kp.shape == (5, 17, 3)
    assert err.max() < HM_MAX_ERR['fp16'] and np.sqrt((err ** 2).mean()) < HM_RMS_ERR['fp16']   # every joint of every crop
    assert conf_err.max() < CONF_TOL


# ------------------------------------------------------------------ 2. the fused decode is exact
@pytest.mark.parametrize('shift', [False, True])
@pytest.mark.parametrize('variant,dataset,pairs', [('s', 'coco', COCO_PAIRS), ('h', 'wholebody', WB_PAIRS)])
def test_fused_decode_equals_decode_of_the_materialised_average(variant, dataset, pairs, shift):
    shp, sd, _ = weights(variant, dataset)
    crops = synthetic_crops(5, 17, 'blobs')
    wh = np.array([[192, 256], [300, 411], [97, 130], [640, 480], [51, 64]], np.int32)
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)
    eng.set_flip_test(pairs, shift_heatmap=shift)
    kp, hm = eng.infer(crops, wh), eng.heatmaps(crops)
    eng.close()
    assert kp.shape == (5, shp.num_keypoints, 3)
    assert np.array_equal(kp, decode_heatmaps(hm, wh)), f'{(kp != decode_heatmaps(hm, wh)).sum()} values differ'


@pytest.mark.parametrize('shift', [False, True])
def test_fused_decode_where_the_dark_samples_wrap_across_joints(shift):
    """The kernel alone on crafted maps: peaks in the four corners (the 7 samples leave the joint's padded map into its neighbour's, joint 0's into
    joint K - 1's and back) and maps that are <= 0 everywhere (coordinates -1: the reference's negative-index wrap), on first, last, paired and
    unpaired joints of K = 133 -- the neighbour map AND its partner are read through the same indirection as the materialised average has them."""
    K, n = 133, 3
    rng = np.random.default_rng(3)
    hm2 = rng.normal(0.0, 0.05, (2 * n, K, 64, 48)).astype(np.float32)
    corners = [(0, 0), (0, 47), (63, 0), (63, 47), (63, 46), (0, 1)]
    for i in range(n):
        for j, k in enumerate([0, 1, 2, 7, 60, 61, 64, 99]):          # a peak the mirror's noise cannot outvote, in a corner of the crop's own map
            y, x = corners[(i + j) % len(corners)]
            hm2[2 * i, k, y, x] += 3.0 + 0.1 * j
        for k in (3, 100, 5, 131, 132, 40):                            # closed under the pairs: nowhere positive in the crop's and the mirror's maps
            hm2[2 * i, k] = -np.abs(hm2[2 * i, k]) - 0.01
            hm2[2 * i + 1, k] = -np.abs(hm2[2 * i + 1, k]) - 0.01
    wh = np.array([[192, 256], [333, 481], [64, 48]], np.int32)
    merged = merged_on_host(hm2, WB_PAIRS, shift)
    flat = merged.reshape(n, K, -1)
    assert (flat.max(-1)[:, [3, 100, 5, 131, 132, 40]] <= 0).all()                     # the negative-index wrap, on the last joint and on joint 132's partner too
    assert flat[0, 0].argmax() == 0 and flat[2, 1].argmax() == 3071                    # joint 0's samples reach back into joint 132, joint 1's forward into joint 2
    got = decode_flip_heatmaps(hm2, WB_PAIRS, shift, wh)
    want = decode_heatmaps(merged, wh)
    assert np.array_equal(got, want, equal_nan=True), f'{(got != want).sum()} values differ'
    assert not np.array_equal(got, decode_heatmaps(hm2[0::2].copy(), wh), equal_nan=True)


# ------------------------------------------------------------------ 3. the two-pass path
@pytest.mark.parametrize('shift', [False, True])
def test_mode_against_the_two_pass_path(shift):
    shp, sd, _ = weights('s', 'coco')
    crops = synthetic_crops(7, 19, 'blobs')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
    kp2, hm2 = eng.infer_flip(crops, COCO_PAIRS, shift_heatmap=shift, return_heatmaps=True)
    eng.set_flip_test(COCO_PAIRS, shift_heatmap=shift)
    hm, kp = eng.heatmaps(crops), eng.infer(crops)
    kp2b, hm2b = eng.infer_flip(crops, COCO_PAIRS, shift_heatmap=shift, return_heatmaps=True)   # unchanged by the mode
    eng.close()
    d = np.abs(hm - hm2).max()
    print(f'mode vs two passes (shift={shift}): heatmap max|diff| {d:.3e}, confidence max|diff| {np.abs(kp[..., 2] - kp2[..., 2]).max():.3e}')
    assert d < SAME_NET_TOL
    assert np.abs(kp[..., 2] - kp2[..., 2]).max() < CONF_TOL
    assert np.array_equal(hm2, hm2b) and np.array_equal(kp2, kp2b)


# ------------------------------------------------------------------ 4. every entry
@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_device_and_submit_entries_equal_infer_under_the_mode(dtype):
    import torch
    shp = model_shape('s', 'coco')
    crops = synthetic_crops(11, 23, 'blobs')
    wh = np.stack([np.arange(11) * 17 + 100, np.arange(11) * 13 + 140], 1).astype(np.int32)
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=dtype, max_batch=8)       # chunks of 4 + 4 + 3
    plain = eng.infer(crops, wh)
    eng.set_flip_test(COCO_PAIRS)
    want = eng.infer(crops, wh)
    assert not np.array_equal(want, plain)
    d_crops, d_wh = torch.from_numpy(crops).cuda(), torch.from_numpy(wh).cuda()
    for n in (11, 4, 3, 1):                                                             # 11: the handle's stream; <= 4: 2 n <= 16 rows on the caller's
        ref = want if n == 11 else eng.infer(crops[:n], wh[:n])
        out = torch.full((n, 17, 3), float('nan'), device='cuda')
        eng.infer_device(d_crops[:n], out, d_wh[:n], sync=True, ordered=False)          # vp_infer_device
        assert np.array_equal(out.cpu().numpy(), ref)
        side = torch.cuda.Stream()
        out2 = torch.full((n, 17, 3), float('nan'), device='cuda')
        torch.cuda.synchronize()
        with torch.cuda.stream(side):                                                   # vp_infer_device_stream on a side stream
            for _ in range(3):                                                          # first sighting, capture, replay
                eng.infer_device(d_crops[:n], out2, d_wh[:n], sync=False)
            total = out2.sum()
        side.synchronize()
        assert torch.isfinite(total).item() and np.array_equal(out2.cpu().numpy(), ref)
    # submit / wait: max_batch / 2 crops per call under the mode, two calls in flight
    pin = PinnedArray(crops.shape, np.uint8)
    pin.array[:] = crops
    outs = [np.zeros((4, 17, 3), np.float32), np.zeros((4, 17, 3), np.float32)]
    s0 = eng.submit(pin.array[0:4], outs[0], wh[0:4])
    s1 = eng.submit(pin.array[4:8], outs[1], wh[4:8])
    eng.wait(s0)
    eng.wait(s1)
    assert np.array_equal(np.concatenate(outs), want[:8])
    with pytest.raises(capi.VpError, match='max_batch / 2') as ei:
        eng.submit(pin.array[0:5], np.zeros((5, 17, 3), np.float32))
    assert ei.value.code == capi.VP_ERR_INVALID
    pin.free()
    eng.clear_flip_test()
    assert not eng.flip_test and np.array_equal(eng.infer(crops, wh), plain)
    eng.close()


@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_frame_entries_equal_infer_under_the_mode(dtype):
    import torch
    from test_gpu_frames import host_crops, matrix
    frames, p9 = matrix()
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=dtype, max_batch=4)       # chunks of 2 crops straddle frames
    plain = eng.infer_frames(frames, p9)
    eng.set_flip_test(COCO_PAIRS, shift_heatmap=True)
    want = eng.infer(host_crops(frames, p9), p9[:, 7:9])
    got = eng.infer_frames(frames, p9)
    assert got.shape == want.shape == (len(p9), 17, 3) and not np.array_equal(got, plain)
    assert np.array_equal(got, want), f'{(got != want).sum()} differing values'
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    assert np.array_equal(eng.infer_frames(d_frames, p9), want)                          # device frames, read in place
    sel = p9[p9[:, 0] == 1]
    assert np.array_equal(eng.infer_frame(frames[1], sel[:, 1:]), eng.infer(host_crops(frames, sel), sel[:, 7:9]))
    eng.close()


@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_boxes_entry_equals_the_host_route_under_the_mode(dtype):
    import torch
    from test_gpu_boxes import host_route, scene, to_dev
    frames, boxes, fidx = scene()
    d_frames, d_boxes, d_fidx = to_dev(frames, boxes, fidx)
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=dtype, max_batch=16)      # 19 boxes: chunks of 8, 8, 3
    plain = eng.infer_boxes(d_frames, d_boxes, d_fidx).cpu().numpy()
    eng.set_flip_test(COCO_PAIRS)
    want, p9 = host_route(eng, d_frames, boxes, fidx)                                   # infer_frames under the mode + the offsets
    for sel in (slice(None), slice(0, 7), slice(4, 5)):                                 # 7 and 1 boxes: 14 / 2 rows on the caller's stream
        for _ in range(3 if sel != slice(None) else 1):                                 # eager, capture, replay
            out, cp, st = eng.infer_boxes(d_frames, d_boxes[sel], d_fidx[sel], crop_params=True, status=True)
            torch.cuda.current_stream().synchronize()
            assert (st.cpu().numpy() == 0).all() and np.array_equal(cp.cpu().numpy(), p9[sel])
            got = out.cpu().numpy()
            if sel == slice(None):
                assert np.array_equal(got, want), f'{(got != want).sum()} differing values'
                assert not np.array_equal(got, plain)
            else:
                assert np.array_equal(got, host_route(eng, d_frames, boxes[sel], fidx[sel])[0])
    # invalid boxes still give a status and zero rows; the valid ones beside them what they give with valid boxes in those places (the same batch
    # size, so the same plan, and every kernel works crop by crop)
    bad_boxes = np.array([[10, 10, 50, 50, 1, 0], [np.nan, 10, 50, 50, 1, 0], [300, 300, 250, 250, 1, 0]], np.float32)
    bad_fidx = np.array([7, 0, 2], np.int32)
    mixed_b = np.concatenate([boxes[:2], bad_boxes[:2], boxes[2:5], bad_boxes[2:]])
    mixed_f = np.concatenate([fidx[:2], bad_fidx[:2], fidx[2:5], bad_fidx[2:]])
    is_good = np.array([1, 1, 0, 0, 1, 1, 1, 0], bool)
    valid_b, valid_f = mixed_b.copy(), mixed_f.copy()
    valid_b[~is_good], valid_f[~is_good] = boxes[5:8], fidx[5:8]
    out, st = eng.infer_boxes(d_frames, torch.from_numpy(mixed_b).cuda(), torch.from_numpy(mixed_f).cuda(), status=True)
    ref, st_ref = eng.infer_boxes(d_frames, torch.from_numpy(valid_b).cuda(), torch.from_numpy(valid_f).cuda(), status=True)
    torch.cuda.synchronize()
    out, st, ref = out.cpu().numpy(), st.cpu().numpy(), ref.cpu().numpy()
    assert st.tolist() == [0, 0, 1, 2, 0, 0, 0, 3] and (st_ref.cpu().numpy() == 0).all()
    assert (out[~is_good] == 0).all() and (ref[~is_good, :, 2] != 0).all()
    assert np.array_equal(out[is_good], ref[is_good])
    assert np.array_equal(ref, host_route(eng, d_frames, valid_b, valid_f)[0])
    eng.close()


def test_group_equals_single_handle_under_the_mode():
    import torch
    ndev = torch.cuda.device_count()
    shp, sd, _ = weights('s', 'coco')
    crops = synthetic_crops(11, 9, 'blobs')
    one = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)
    one.set_flip_test(COCO_PAIRS)
    ref = one.infer(crops)
    one.close()
    grp = VitPoseGroup(shp, sd, list(range(ndev)), dtype='fp16', max_batch=4)           # rounds of ndev x 2 crops
    plain = grp.infer(crops)
    grp.set_flip_test(COCO_PAIRS)
    got = grp.infer(crops)
    assert np.array_equal(got, ref) and not np.array_equal(got, plain)
    assert grp.infer(crops[:0]).shape == (0, 17, 3)
    # members that disagree on the mode: refused before anything is enqueued
    lib = capi.load_library()
    assert lib.vp_clear_flip_test(lib.vp_group_member(grp._g, 0)) == capi.VP_OK
    if ndev > 1:
        with pytest.raises(capi.VpError) as ei:
            grp.infer(crops)
        assert ei.value.code == capi.VP_ERR_STATE and 'disagree' in ei.value.msg
    grp.clear_flip_test()
    assert np.array_equal(grp.infer(crops), plain)
    grp.close()


# ------------------------------------------------------------------ 5. graph hygiene
def test_graphs_never_cross_modes(monkeypatch):
    import torch
    shp, sd, _ = weights('s', 'coco')
    crops = synthetic_crops(3, 29, 'blobs')
    other_pairs = [[0, 16], [5, 6]]

    def fresh(pairs):
        h = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
        if pairs is not None:
            h.set_flip_test(pairs)
        return h

    def sequence():
        """identical buffers through vp_infer_device: 3 x off, 3 x on, 3 x off, 3 x on with other pairs"""
        eng = fresh(None)
        d_crops = torch.from_numpy(crops).cuda()
        out = torch.empty((3, 17, 3), device='cuda')
        res = []
        for block in (None, COCO_PAIRS, None, other_pairs):
            if block is None:
                eng.clear_flip_test()
            else:
                eng.set_flip_test(block)
            for _ in range(3):
                out.fill_(float('nan'))
                eng.infer_device(d_crops, out, sync=True, ordered=False)
                res.append(out.cpu().numpy())
        eng.close()
        return res

    res = sequence()
    never, on_a, on_b = fresh(None), fresh(COCO_PAIRS), fresh(other_pairs)
    ref_off, ref_a, ref_b = never.infer(crops), on_a.infer(crops), on_b.infer(crops)
    for h in (never, on_a, on_b):
        h.close()
    for r in res[0:3] + res[6:9]:
        assert np.array_equal(r, ref_off)                        # off == a handle that never had the mode, before and after it was on
    for r in res[3:6]:
        assert np.array_equal(r, ref_a)
    assert not np.array_equal(res[3], res[0])
    for r in res[9:12]:
        assert np.array_equal(r, ref_b)                          # a changed table misses the graph captured under the first one
    assert not np.array_equal(ref_a, ref_b)
    monkeypatch.setenv('VP_GRAPH', '0')                          # no capture at all: the same bits
    eager = sequence()
    for a, b in zip(res, eager):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ 6. run to run
@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_run_to_run_identity_under_the_mode(dtype):
    shp = model_shape('s', 'coco')
    sd = synthetic_state_dict(shp, 0)
    pool = synthetic_crops(17, 31, 'blobs')
    for n in (1, 2, 3, 8, 17):
        eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=16)     # 17 crops: chunks of 8 + 8 + 1
        eng.set_flip_test(COCO_PAIRS)
        first_kp, first_hm = eng.infer(pool[:n]), eng.heatmaps(pool[:n])
        for _ in range(3):
            assert np.array_equal(eng.infer(pool[:n]), first_kp), f'n = {n}'
        assert np.array_equal(eng.heatmaps(pool[:n]), first_hm)
        eng.close()
        again = VitPoseHip(shp, sd, dtype=dtype, max_batch=16)
        again.set_flip_test(COCO_PAIRS)
        assert np.array_equal(again.infer(pool[:n]), first_kp)
        again.close()


# ------------------------------------------------------------------ 7. mirror symmetry
def test_mirrored_crops_give_the_flipped_back_average():
    shp, sd, _ = weights('s', 'coco')
    crops = synthetic_crops(4, 37, 'blobs')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
    eng.set_flip_test(COCO_PAIRS)
    hm = eng.heatmaps(crops)
    hm_m = eng.heatmaps(np.ascontiguousarray(crops[:, :, ::-1]))
    eng.close()
    d = np.abs(O.flip_back(hm_m, COCO_PAIRS) - hm).max()
    print(f'mirror symmetry: max|diff| {d:.3e}')
    assert d < SAME_NET_TOL


# ------------------------------------------------------------------ 8. chunking and edges
def test_chunking_and_edges():
    shp, sd, _ = weights('s', 'coco')
    pool = synthetic_crops(9, 43, 'blobs')
    ref_eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=2)    # one crop + its mirror per chunk
    ref_eng.set_flip_test(COCO_PAIRS)
    ref_hm = ref_eng.heatmaps(pool)
    ref_eng.close()
    for max_batch in (8, 5, 3):                                   # caps 4, 2, 1 -- odd max_batch: the spare row stays empty
        eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=max_batch)
        eng.set_flip_test(COCO_PAIRS)
        cap = max_batch // 2
        assert eng.infer(pool[:0]).shape == (0, 17, 3) and eng.heatmaps(pool[:0]).shape == (0, 17, 64, 48)
        for n in (cap, cap + 1, 9):
            kp, hm = eng.infer(pool[:n]), eng.heatmaps(pool[:n])
            assert kp.shape == (n, 17, 3) and np.array_equal(kp, decode_heatmaps(hm))
            assert np.abs(hm - ref_hm[:n]).max() < SAME_NET_TOL  # every crop where it belongs, whatever the chunking
        eng.close()


def test_refusals():
    lib = capi.load_library()
    shp, sd, _ = weights('s', 'coco')
    pairs = np.asarray(COCO_PAIRS, np.int32)
    # a created but unloaded handle
    cfg = capi.vp_config(shp.embed_dim, shp.depth, shp.num_heads, 17, capi.VP_DTYPE_F16, 0, 4)
    h = C.c_void_p()
    assert lib.vp_create(C.byref(h), C.byref(cfg)) == capi.VP_OK
    assert lib.vp_set_flip_test(h, pairs.ctypes.data, len(pairs), 0) == capi.VP_ERR_STATE
    assert 'not loaded' in capi.last_error(h)
    lib.vp_destroy(h)
    # max_batch = 1: no room for the mirror image, and no hidden two-pass fallback
    one = VitPoseHip(shp, sd, dtype='fp16', max_batch=1)
    with pytest.raises(capi.VpError, match='max_batch') as ei:
        one.set_flip_test(COCO_PAIRS)
    assert ei.value.code == capi.VP_ERR_STATE and not one.flip_test
    crops = synthetic_crops(2, 47, 'blobs')
    assert one.infer(crops).shape == (2, 17, 3)                               # and goes on working in the default mode
    one.close()
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)
    plain = eng.infer(crops)
    for bad, n_pairs in (([[0, 17]], 1), ([[-1, 2]], 1), (COCO_PAIRS, -1)):
        b = np.asarray(bad, np.int32)
        assert lib.vp_set_flip_test(eng._h, b.ctypes.data, n_pairs, 0) == capi.VP_ERR_INVALID
    assert lib.vp_set_flip_test(eng._h, None, 2, 0) == capi.VP_ERR_INVALID
    assert not eng.flip_test and np.array_equal(eng.infer(crops), plain)   # a refused set leaves the handle as it was
    eng.set_flip_test([])                                                   # no pairs at all is a valid table: every joint mirrors onto itself
    assert eng.flip_test
    eng.close()


def test_fp8_handle_runs_the_mode():
    """The mode sits above the encoder: an fp8 handle takes it as it is.  fp8 has no parity figures here; what must hold whatever the operand type is
    asserted -- the fused decode equals the decode of the materialised average, and a call repeats its bits."""
    shp = model_shape('b', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype='fp8', max_batch=8)
    crops = synthetic_crops(7, 3, 'blobs')
    eng.set_flip_test(COCO_PAIRS)
    kp, hm = eng.infer(crops), eng.heatmaps(crops)
    assert kp.shape == (7, 17, 3) and np.isfinite(kp).all()
    assert np.array_equal(kp, decode_heatmaps(hm)) and np.array_equal(kp, eng.infer(crops))
    eng.clear_flip_test()
    assert not np.array_equal(eng.infer(crops), kp)
    eng.close()


def test_vitpose_plus_handle_under_the_mode(one_launch_family):
    from test_gpu_moe import expert_handle, pool, split_handle
    crops = pool()[:7]
    aic_pairs = [[0, 3], [1, 4], [2, 5], [6, 9], [7, 10], [8, 11]]
    eng = expert_handle('s', 'fp16', 8)
    eng.set_dataset('aic')
    eng.set_flip_test(aic_pairs, shift_heatmap=True)
    got_kp, got_hm = eng.infer(crops), eng.heatmaps(crops)
    h = split_handle('s', 'aic', 'fp16', 8)
    h.set_flip_test(aic_pairs, shift_heatmap=True)
    want_kp, want_hm = h.infer(crops), h.heatmaps(crops)
    h.close()
    assert got_kp.shape == (7, 14, 3) and np.array_equal(got_kp, want_kp) and np.array_equal(got_hm, want_hm)
    # several datasets in one batch: out of the mode's scope, refused with the documented error
    with pytest.raises(capi.VpError, match='flip-test') as ei:
        eng.infer_mixed(crops, ['coco'] * 7)
    assert ei.value.code == capi.VP_ERR_STATE
    # a head with another K: the switch takes place, the mode is cleared and the call says so
    with pytest.raises(capi.VpError, match='cleared') as ei:
        eng.set_dataset('wholebody')
    assert ei.value.code == capi.VP_ERR_STATE and not eng.flip_test and eng.dataset == 'wholebody' and eng.K == 133
    assert eng.infer(crops).shape == (7, 133, 3)
    # a head with the same K keeps the mode (coco's 17 joints <-> ap10k's 17)
    eng.set_dataset('coco')
    eng.set_flip_test(COCO_PAIRS)
    eng.set_dataset('ap10k')
    assert eng.flip_test and eng.infer(crops).shape == (7, 17, 3)
    eng.close()
