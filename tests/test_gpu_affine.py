"""GPU: the training-protocol affine crop route on the device (ViTPose-S handles): the crop kernel against the host twin, the affine decode against the
reference's own keypoints, the chain boxes entry == frames entry == `infer` on the host twin's crops + the fp64 back-map (all 32 bits), the end-to-end
reference golden, and that the default pad route is untouched."""
import os

import numpy as np
import pytest

import affine_cases as AC
from cases import coco_flip_pairs, peaked_heatmaps
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd import VitPoseHip
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.cropprep import Frame, affine_back_map, affine_crops_host, box_to_cs, rgb_to_nv12
from easy_vitpose_amd.engine import box_cs_host, crop_affine_device, decode_affine_heatmaps
from easy_vitpose_amd.synth import synthetic_state_dict
from helpers import CONF_TOL, KP_TOL_PX

gpu = pytest.mark.gpu


def decode_bound(exp, cs):
    """Per coordinate of exp [n, K, 3] (y, x, conf): 2e-3 max(1, S / 192) + 4 ulp32(max(|coord|, S)).
    First term: 2e-3 crop pixels is what the existing decode test allows the DARK step between the device's float32 sums and the reference's (test_gpu_parity.py
    test_decode_matches_reference_golden), and a crop pixel is S_w / 192 frame pixels (S_h / 256, the same number: every crop is 3:4), never less than the bound
    of the unmagnified crop.  Second term: the reference evaluates transform_preds in float32 -- coords * scale_x + center - scale * 0.5, three roundings of values
    no larger than max(|coord|, S) -- and the device rounds its fp64 result once: at most 3 + 1/2 ulp32 of that magnitude apart."""
    cs = np.asarray(cs, dtype=np.float64)
    mag = 2e-3 * np.maximum(1.0, cs[:, 2] / 192.0)[:, None]
    ulp = lambda v: np.spacing(v.astype(np.float32)).astype(np.float64)
    by = mag + 4 * ulp(np.maximum(np.abs(exp[..., 0]), cs[:, 3][:, None]))
    bx = mag + 4 * ulp(np.maximum(np.abs(exp[..., 1]), cs[:, 2][:, None]))
    return np.stack([by, bx], -1)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'affine.npz'))


@pytest.fixture(scope='module')
def engines():
    """max_batch 8: a 17-crop call splits into 8 + 8 + 1; max_batch 32: its 17 crops are one chunk beyond the 16-crop graph path"""
    shp = model_shape('s', 'coco')
    sd = synthetic_state_dict(shp, 0, peaked=True)
    e8, e32 = VitPoseHip(shp, sd, dtype='fp16', device_id=0, max_batch=8), VitPoseHip(shp, sd, dtype='fp16', device_id=0, max_batch=32)
    yield e8, e32
    e8.close()
    e32.close()


@pytest.fixture(scope='module')
def scene():
    """frame A 240 x 320 RGB and frame B 96 x 132 NV12, on the host and on the device, with what the entries see of them (to_rgb)"""
    import torch
    fa, _ = AC.frames()
    y, uv = AC.frame_b_nv12()
    host = [Frame.rgb(fa), Frame.nv12(y, uv)]
    dev = [Frame.rgb(torch.from_numpy(fa).cuda()), Frame.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())]
    return host, dev


def seventeen():
    """17 valid boxes over the two frames: the end-to-end boxes, then seeded ones"""
    b, f = AC.e2e_boxes()
    rng = np.random.default_rng(91)
    x1, y1 = rng.uniform(-10, 80, 9), rng.uniform(-10, 50, 9)
    more = np.stack([x1, y1, x1 + rng.uniform(8, 60, 9), y1 + rng.uniform(8, 70, 9)], 1).astype(np.float32)
    return np.concatenate([b, more]), np.concatenate([f, rng.integers(0, 2, 9).astype(np.int32)])


def host_chain(eng, host_frames, boxes, fidx):
    """`infer` on the host twin's crops, then the fp64 back-map.  org_wh = (94, 126) makes the pad route's decode write exactly twice the heatmap-pixel
    position (x = rx (94 / 47) + 47 - 47), so rx, ry are recovered without a rounding and the back-map sees what the affine decode sees."""
    cs = box_to_cs(boxes)
    crops = np.empty((len(boxes), 256, 192, 3), np.uint8)
    for f in set(fidx.tolist()):
        crops[fidx == f] = affine_crops_host(host_frames[f], cs[fidx == f])
    kp = eng.infer(crops, np.tile(np.array([[94, 126]], np.int32), (len(boxes), 1)))
    kp[..., :2] *= 0.5
    return affine_back_map(kp, cs), cs


def frames_params(fidx, cs):
    return np.concatenate([fidx[:, None].astype(np.float64), cs.astype(np.float64)], 1)


# ------------------------------------------------------------------------------------------------------------------ 1. the crop kernel
@gpu
@pytest.mark.parametrize('fmt', ['rgb', 'bgr', 'nv12'])
def test_crop_kernel_equals_host_twin(golden, fmt):
    fa, _ = AC.frames()
    if fmt == 'nv12':
        frame = Frame.nv12(*rgb_to_nv12(fa, 'bt709'), 'bt709')
    else:
        frame = Frame.bgr(np.ascontiguousarray(fa[..., ::-1])) if fmt == 'bgr' else Frame.rgb(fa)
    anchors = [[95.5, 127.5, 191, 255], [191, 255, 382, 510], [47.75, 63.75, 95.5, 127.5], [-300, -400, 191, 255], [85.5, 107.5, 191, 255],
               [160.0, 120.0, 2000.0, 2666.0], [319.5, 239.5, 4.0, 5.0]]
    cs = np.concatenate([golden['center'], golden['scale200']], 1)
    cs = np.concatenate([cs, np.array(anchors, np.float32)])
    got = crop_affine_device(frame, cs)
    want = affine_crops_host(frame, cs)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=(1, 2, 3))).ravel()
    assert want[:9].any(axis=(1, 2, 3)).tolist() == [True, True, True, True, True, True, True, False, True]   # the crop wholly outside is black, the others are not


# ------------------------------------------------------------------------------------------------------------------ 2. the decode
@gpu
@pytest.mark.parametrize('K', [17, 133])
def test_decode_affine_vs_reference_golden(golden, K):
    """confidences bit equal, coordinates within decode_bound of the reference's keypoints_from_heatmaps(center, scale * 200, use_udp=True); the same bound holds
    for the fp64 model on the CPU (test_affine_host.py test_fp64_decode_model_within_the_gpu_bound)"""
    cs = np.concatenate([golden['center'], golden['scale200']], 1)
    hm = peaked_heatmaps(len(cs), K, AC.DECODE_SEEDS[K])
    got = decode_affine_heatmaps(hm, cs)
    exp = golden[f'decode_k{K}']
    assert np.array_equal(got[..., 2], exp[..., 2])
    d = np.abs(got[..., :2].astype(np.float64) - exp[..., :2])
    bound = decode_bound(exp, cs)
    print(f'affine decode K = {K}: max {d.max():.3e} px, worst ratio to the bound {(d / bound).max():.3f}')
    assert (d <= bound).all()


@gpu
def test_decode_affine_flip_equals_merged_decode():
    """the flip-test instantiation: the interleaved batch decoded on the fly == the plain affine decode of the averaged maps (the pad route's own identity)"""
    from oracle import vitpose_cpu as O
    cs = box_to_cs(AC.geometry_boxes()[:6])
    hm2 = peaked_heatmaps(12, 17, 63)
    pairs = coco_flip_pairs()
    merged = (hm2[0::2] + O.flip_back(hm2[1::2], pairs)) * np.float32(0.5)
    assert np.array_equal(decode_affine_heatmaps(hm2, cs, flip_pairs=pairs), decode_affine_heatmaps(merged.astype(np.float32), cs))


# ------------------------------------------------------------------------------------------------------------------ 3. the chain of bit identities
@gpu
@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('which,n', [(0, 9), (0, 17), (1, 17)])
def test_boxes_frames_and_host_chain_agree(engines, scene, flip, which, n):
    """infer_boxes(crop='affine') has the bits of infer_frames(crop='affine') on box_to_cs of the same boxes (host frames: the band upload), which has the bits of
    `infer` on the host twin's crops followed by the fp64 back-map; d_cs and d_status equal the host's.  9 crops: one graph-path chunk (max_batch 8: 8 + 1);
    17 crops: 8 + 8 + 1 on the max_batch 8 handle, one eager chunk of 17 (flip mode: 16 + 1) on the max_batch 32 handle."""
    import torch
    eng = engines[which]
    host, dev = scene
    boxes, fidx = seventeen()
    boxes, fidx = boxes[:n], fidx[:n]
    if flip:
        eng.set_flip_test(coco_flip_pairs())
    try:
        want, cs = host_chain(eng, host, boxes, fidx)
        via_frames = eng.infer_frames(host, frames_params(fidx, cs), crop='affine')
        out, d_cs, d_st = eng.infer_boxes(dev, torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda(), crop='affine', cs=True, status=True)
        torch.cuda.synchronize()
    finally:
        if flip:
            eng.clear_flip_test()
    assert np.array_equal(via_frames.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), via_frames.view(np.uint32))
    assert np.array_equal(d_cs.cpu().numpy().view(np.uint32), cs.view(np.uint32)) and not d_st.cpu().numpy().any()
    assert np.isfinite(want).all() and want[..., 2].min() > 0.05   # the peaked checkpoint: a real blob on every joint


@gpu
def test_refused_boxes_are_zero_rows(engines, scene):
    """rows with a non-zero status: zero keypoints, a zero cs row, the status of the host tap; the rows around them are the chain's (a refused box is a black crop in
    the same chunk)"""
    import torch
    eng = engines[0]
    host, dev = scene
    boxes, fidx = AC.e2e_boxes()
    boxes, fidx = boxes[:7].copy(), fidx[:7].copy()
    boxes[1, 0] = np.nan
    boxes[3, 2] = boxes[3, 0]
    fidx[5] = 2
    cs_h, st_h = box_cs_host(boxes, fidx, n_frames=2)
    assert st_h.tolist() == [0, 2, 0, 3, 0, 1, 0]
    out, d_cs, d_st = eng.infer_boxes(dev, torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda(), crop='affine', cs=True, status=True)
    out, d_cs, d_st = out.cpu().numpy(), d_cs.cpu().numpy(), d_st.cpu().numpy()
    assert np.array_equal(d_st, st_h) and np.array_equal(d_cs.view(np.uint32), cs_h.view(np.uint32))
    bad = st_h != 0
    assert not out[bad].any() and not d_cs[bad].any()
    crops = np.zeros((7, 256, 192, 3), np.uint8)
    for f in (0, 1):
        sel = (fidx == f) & ~bad
        crops[sel] = affine_crops_host(host[f], cs_h[sel])
    kp = eng.infer(crops, np.tile(np.array([[94, 126]], np.int32), (7, 1)))
    kp[..., :2] *= 0.5
    want = affine_back_map(kp[~bad], cs_h[~bad])
    assert np.array_equal(out[~bad].view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
@gpu
def test_end_to_end_vs_reference_golden(engines, scene, golden):
    """The reference ViTPose (S / coco, peaked checkpoint) on the independent model's crops, decoded with each box's centre and scale: the tolerances
    test_gpu_parity.py uses for the peaked checkpoint, +-0.5 px of the CROP -- max(1, S_w / 192) frame pixels, as its frames test scales them -- and 1e-3."""
    import torch
    host, dev = scene
    boxes, fidx = golden['e2e_boxes'], golden['e2e_frame']
    b, f = AC.e2e_boxes()
    assert np.array_equal(boxes, b) and np.array_equal(fidx, f)
    ref = golden['e2e_keypoints']
    tol = (KP_TOL_PX * np.maximum(1.0, golden['e2e_scale200'][:, 0] / 192.0))[:, None]
    got = engines[0].infer_boxes(dev, torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda(), crop='affine').cpu().numpy()
    dpx = np.abs(got[..., :2] - ref[..., :2]).max(-1)
    dcf = np.abs(got[..., 2] - ref[..., 2])
    print(f'affine end to end: coordinate max err {dpx.max():.4f} frame px (worst ratio to the tolerance {(dpx / tol).max():.3f}), confidence max err {dcf.max():.3e}')
    assert (dpx < tol).all() and dcf.max() < CONF_TOL
    cs = np.concatenate([golden['e2e_center'], golden['e2e_scale200']], 1)
    via_frames = engines[0].infer_frames(host, frames_params(fidx, cs), crop='affine')
    assert np.array_equal(via_frames.view(np.uint32), got.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ 5 / 6. the default route, repeats
@gpu
def test_default_route_untouched_and_calls_repeat(engines, scene):
    import torch
    eng = engines[0]
    _, dev = scene
    boxes, fidx = AC.e2e_boxes()
    inside = np.array([[40, 30, 160, 200], [100, 20, 300, 230], [10, 60, 70, 140], [20, 10, 100, 90], [60, 30, 120, 90]], np.float32)
    d_in, d_fi = torch.from_numpy(inside).cuda(), torch.from_numpy(np.array([0, 0, 0, 1, 1], np.int32)).cuda()
    d_b, d_f = torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda()
    pad_calls = [eng.infer_boxes(dev, d_in, d_fi, crop_params=True, status=True) for _ in range(2)]
    aff = [eng.infer_boxes(dev, d_b, d_f, crop='affine', cs=True, status=True) for _ in range(3)]   # eager, captured, replayed
    pad_calls += [eng.infer_boxes(dev, d_in, d_fi, crop_params=True, status=True), eng.infer_boxes(dev, d_in, d_fi, crop='pad', crop_params=True, status=True)]
    torch.cuda.synchronize()
    for later in pad_calls[1:]:
        for a, b in zip(pad_calls[0], later):
            assert torch.equal(a, b)
    for later in aff[1:]:
        for a, b in zip(aff[0], later):
            assert torch.equal(a, b)
    assert not torch.equal(pad_calls[0][0][:3], aff[0][0][:3])   # and the two routes are different crops


# ------------------------------------------------------------------------------------------------------------------ refusals on a handle
@gpu
def test_entry_refusals(engines, scene):
    """everything vp_infer_boxes_images_stream refuses, before anything is enqueued, and box_scale; the handle works afterwards"""
    import torch
    eng = engines[0]
    host, dev = scene
    boxes, fidx = AC.e2e_boxes()
    d_b, d_f = torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda()
    out = torch.empty((len(boxes), eng.K, 3), dtype=torch.float32, device='cuda')
    table = eng._image_table(dev, device_only=True)
    lib, h = eng.lib, eng._h
    call = lambda tab=table, nimg=2, b=d_b.data_ptr(), stride=4, n=len(boxes), scale=1.25, o=out.data_ptr(): lib.vp_infer_boxes_affine_stream(
        h, tab, nimg, b, stride, d_f.data_ptr(), n, scale, o, None, None, None)
    for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=float('inf')), dict(stride=3), dict(n=-1), dict(b=None), dict(o=None),
               dict(tab=None), dict(nimg=0), dict(tab=eng._image_table(host))):
        assert call(**kw) == capi.VP_ERR_INVALID, kw
    bad = eng._image_table(dev, device_only=True)
    bad[1].format = 7
    assert call(tab=bad) == capi.VP_ERR_INVALID
    with pytest.raises(capi.VpError):
        eng.infer_frames(host, np.array([[0, 10, 10, np.nan, 40]]), crop='affine')
    with pytest.raises(capi.VpError):
        eng.infer_frames(host, np.array([[2, 10, 10, 30, 40]]), crop='affine')
    assert call() == capi.VP_OK
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all()


@gpu
def test_vitinference_affine(scene):
    """VitInference(crop='affine'): the tracker's boxes through the affine route, keypoints in frame pixels with no offset added == the engine's frames entry"""
    from easy_vitpose_amd import VitInference
    fa, _ = AC.frames()
    dets = np.array([[40, 30, 160, 200, 0.9], [100, 20, 300, 230, 0.8], [5, 5, 60, 80, 0.2]], np.float64)
    shp = model_shape('s', 'coco')
    V = VitInference(synthetic_state_dict(shp, 0, peaked=True), lambda img: dets, 's', dataset='coco', max_batch=8, crop='affine')
    res = V.inference(fa)
    assert sorted(res) == [0, 1]
    cs = box_to_cs(dets[:2, :4].round().astype(np.float32))
    want = V._vit_pose.infer_frames([fa], frames_params(np.zeros(2, np.int32), cs), crop='affine')
    assert np.array_equal(res[0], want[0]) and np.array_equal(res[1], want[1])
    assert V._tracker_res[0].tolist() == dets[:2, :4].round().astype(int).tolist()   # the stored boxes stay the detector's
