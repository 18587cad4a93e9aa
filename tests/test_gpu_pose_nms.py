"""GPU: person scores and OKS pose NMS on the device (vp_pose_nms_stream / vp_pose_nms, VitPoseHip.pose_nms, infer_boxes(nms=), VitInference(pose_nms=))
against the host model of the same header (vp_dbg_pose_nms_host, pinned against the reference on the CPU: tests/test_pose_nms_host.py) and against
the reference's goldens directly.  Ranks and counts equal, hard scores bit-equal, OKS within one float32 step (the device's fp64 exp is not the host's),
soft scores within (2 + 2 / oks_thr) * 2^-23 per pick in front."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

from easy_vitpose_amd import VitInference, VitPoseHip
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.posenms import NMS_MAX_PER_FRAME, PoseNms
from easy_vitpose_amd.synth import synthetic_state_dict
from pose_nms_cases import edge_cases, golden_case, golden_cases, nms_host, oks_tap, people, sigmas17, soft_bound, ulp_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=32)
    yield e
    e.close()


def with_sigmas(cfg, sigmas):
    return dataclasses.replace(cfg, sigmas=tuple(float(s) for s in sigmas))


def check_against_host(eng, kp, bs, p9, nf, cfg, sigmas, status=None, tag=''):
    """device (vp_pose_nms) against the host model, hard and soft"""
    for soft in (False, True):
        c = with_sigmas(dataclasses.replace(cfg, soft=soft), sigmas)
        ws, wr, wc = nms_host(kp, bs, p9, nf, c, sigmas, status=status)
        gs, gr, gc = eng.pose_nms_host(kp, bs, p9, nf, c, status=status)
        assert np.array_equal(gr, wr), f'{tag} soft={soft}: ranks differ at rows {np.flatnonzero(gr != wr)[:8]}'
        assert np.array_equal(gc, wc), f'{tag} soft={soft}: counts {gc} != {wc}'
        if not soft:
            assert np.array_equal(gs.view(np.int32), ws.view(np.int32)), f'{tag}: hard scores are not bit-equal'
        else:
            picked = wr >= 0
            assert np.array_equal(gs[~picked].view(np.int32), ws[~picked].view(np.int32))
            g64, w64 = gs[picked].astype(np.float64), ws[picked].astype(np.float64)
            assert (np.abs(g64 - w64) <= soft_bound(wr[picked], c.oks_thr) * np.abs(w64)).all(), f'{tag}: soft score err {np.abs(g64 - w64).max():.2e}'


def test_device_equals_the_host_model_on_goldens_and_edge_cases(eng):
    for K, n, ti, vi in golden_cases():
        g = golden_case(K, n, ti, vi)
        check_against_host(eng, g['kpts'], g['box'], g['p9'], g['n_frames'], PoseNms(oks_thr=g['thr'], vis_thr=g['vis'], max_dets=g['max_dets']), g['sigmas'],
                           tag=f'golden K={K} n={n} thr={g["thr"]} vis={g["vis"]}')
    for name, (kp, bs, p9, nf, st) in edge_cases().items():
        for cfg in (PoseNms(), PoseNms(oks_thr=0.5, max_dets=3), PoseNms(vis_thr=None)):
            check_against_host(eng, kp, bs, p9, nf, cfg, sigmas17(), status=st, tag=name)
    s, r, c = eng.pose_nms_host(np.zeros((0, 17, 3), np.float32), np.zeros(0, np.float32), np.zeros((0, 9), np.int32), 2, PoseNms())
    assert c.tolist() == [0, 0] and len(s) == 0
    # ... and through vp_pose_nms_stream: only d_count is written, on the caller's stream
    import torch
    s, r, c = eng.pose_nms(torch.zeros((0, 17, 3), device='cuda'), torch.zeros((0,), device='cuda'), torch.zeros((0, 9), dtype=torch.int32, device='cuda'), 2, PoseNms())
    assert c.cpu().tolist() == [0, 0] and s.shape == (0,) and r.shape == (0,)


@pytest.mark.parametrize('n', [8, 1, 0])
@pytest.mark.parametrize('status', [True, False], ids=['status', 'no_status'])
def test_host_arrays_with_status_absent_and_with_zero_rows(eng, status, n):
    """vp_pose_nms on host arrays with status given or null, on 8 rows of 17 joints over two frames, on one row and on none: scores, ranks and counts
    against the host tap (hard scores bit for bit)"""
    kp, bs, p9 = people(8, n_frames=2, seed=7)
    st = np.array([0, 3, 0, 0, 1, 0, 0, 0], np.int32)[:n] if status else None
    check_against_host(eng, kp[:n], bs[:n], p9[:n], 2, PoseNms(oks_thr=0.5), sigmas17(), status=st, tag=f'n={n}')


@pytest.mark.parametrize('n', [65, 257, NMS_MAX_PER_FRAME])
def test_sizes_across_a_wave_a_workgroup_and_the_cap(eng, n):
    kp, bs, p9 = people(n, seed=100 + n)
    check_against_host(eng, kp, bs, p9, 1, PoseNms(oks_thr=0.5), sigmas17(), tag=f'n={n}')


def test_over_the_cap_frame_is_marked_and_the_other_frame_processed(eng):
    kp0, bs0, p0 = people(NMS_MAX_PER_FRAME + 1, seed=10, dup=0.0)
    kp1, bs1, p1 = people(5, seed=11)
    p1[:, 0] = 1
    order = np.random.default_rng(9).permutation(len(kp0) + 5)
    kp, bs, p9 = np.concatenate([kp0, kp1])[order], np.concatenate([bs0, bs1])[order], np.concatenate([p0, p1])[order]
    check_against_host(eng, kp, bs, p9, 2, PoseNms(), sigmas17(), tag='1025 + 5')
    s, r, c = eng.pose_nms_host(kp, bs, p9, 2, PoseNms())
    assert (r[p9[:, 0] == 0] == -2).all() and c[0] == 0 and c[1] > 0 and (r[p9[:, 0] == 1] >= -1).all()


def test_pairwise_oks_device_against_host_tap_and_reference(eng):
    for K, n, vi in sorted({(k, n, vi) for k, n, _, vi in golden_cases()}):
        g = golden_case(K, n, 0, vi)
        cfg = PoseNms(vis_thr=g['vis'])
        dev, host = oks_tap(eng.device_id, g['kpts'], g['p9'], cfg, g['sigmas']), oks_tap(-1, g['kpts'], g['p9'], cfg, g['sigmas'])
        d = ulp_diff(dev, host)
        print(f'K={K} n={n} vis={g["vis"]}: device vs host {int((d > 0).sum())} of {d.size} differ, max {int(d.max())} ulp; vs reference max {int(ulp_diff(dev, g["oks"]).max())} ulp')
        assert d.max() <= 1
    for name, (kp, bs, p9, nf, st) in edge_cases().items():
        for cfg in (PoseNms(), PoseNms(vis_thr=None)):
            dev, host = oks_tap(eng.device_id, kp, p9, cfg, sigmas17()), oks_tap(-1, kp, p9, cfg, sigmas17())
            assert ulp_diff(dev, host).max() <= 1, (name, cfg.vis_thr)
            if name == 'two_identical':   # d2 = 0 on every joint: exp(-0) = 1 exactly
                assert (dev == 1.0).all()
            if name == 'no_visible_joint' and cfg.vis_thr is not None:   # no joint counts: exactly 0 against every pick
                assert (dev[:, 2] == 0.0).all() and dev[2, 0] > 0.0
            if name == 'no_visible_joint' and cfg.vis_thr is None:
                assert dev[2, 2] == 1.0


@pytest.mark.parametrize('n,lanes', [(3, 64), (12, 16), (100, 2), (200, 1)])
def test_lane_split_sum_is_the_serial_sum(eng, n, lanes):
    """The kernel spreads a candidate's terms over L lanes (L from the frame's member count) and adds them in joint order with shuffles.  The device tap runs that
    same function with the L of n members, the host tap the serial loop: one float32 step at the most (the device's fp64 exp), at K = 17 and K = 133.  And the
    product kernel at the same L: its soft scores, which carry every OKS of every pick, against the host model."""
    L = 1
    while L < 64 and n * L * 2 <= 256:
        L *= 2
    assert L == lanes
    for K, sig in ((17, sigmas17()), (133, np.full(133, 0.05, np.float32))):
        kp, bs, p9 = people(n, K=K, seed=500 + n)
        for cfg in (PoseNms(oks_thr=0.5), PoseNms(oks_thr=0.5, vis_thr=None)):
            d = ulp_diff(oks_tap(eng.device_id, kp, p9, cfg, sig), oks_tap(-1, kp, p9, cfg, sig))
            print(f'n={n} L={L} K={K} vis={cfg.vis_thr}: {int((d > 0).sum())} of {d.size} differ, max {int(d.max())} ulp')
            assert d.max() <= 1
            check_against_host(eng, kp, bs, p9, 1, dataclasses.replace(cfg, max_dets=n), sig, tag=f'n={n} L={L} K={K}')


def test_keep_lists_of_the_reference_on_the_device(eng):
    for K, n, ti, vi in golden_cases():
        g = golden_case(K, n, ti, vi)
        cfg = with_sigmas(PoseNms(oks_thr=g['thr'], vis_thr=g['vis'], max_dets=g['max_dets']), g['sigmas'])
        s, r, c = eng.pose_nms_host(g['kpts'], g['box'], g['p9'], g['n_frames'], cfg)
        assert np.array_equal(r, g['hard_rank']) and np.array_equal(s.view(np.int32), g['score'].view(np.int32)), (K, n, ti, vi)
        s, r, c = eng.pose_nms_host(g['kpts'], g['box'], g['p9'], g['n_frames'], dataclasses.replace(cfg, soft=True))
        assert np.array_equal(r, g['soft_rank']), (K, n, ti, vi)


def test_run_to_run_identical_bits(eng):
    import torch
    kp, bs, p9 = people(300, n_frames=3, seed=77)
    d_kp, d_bs, d_p9 = torch.from_numpy(kp).cuda(), torch.from_numpy(bs).cuda(), torch.from_numpy(p9).cuda()
    for cfg in (PoseNms(oks_thr=0.5), PoseNms(oks_thr=0.5, soft=True, max_dets=50)):
        runs = []
        for _ in range(3):
            s, r, c = eng.pose_nms(d_kp, d_bs, d_p9, 3, cfg)
            runs.append((s.cpu().numpy().view(np.int32), r.cpu().numpy(), c.cpu().numpy()))
        for other in runs[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))
        ws, wr, wc = nms_host(kp, bs, p9, 3, cfg, sigmas17())
        assert np.array_equal(runs[0][1], wr) and np.array_equal(runs[0][2], wc)


@functools.lru_cache(maxsize=1)
def doubled_scene():
    """The scene of tests/test_gpu_boxes.py with every box once more, shifted by 2 px, and seeded box scores in column 4"""
    from test_gpu_boxes import scene
    frames, boxes, fidx = scene()
    boxes = np.concatenate([boxes, boxes + np.array([2, 2, 2, 2, 0, 0], np.float32)])
    boxes[:, 4] = np.random.default_rng(5).uniform(0.4, 0.95, len(boxes)).astype(np.float32)
    return frames, boxes, np.concatenate([fidx, fidx])


def person_groups(p9):
    """rows that show the same person: same frame, padded and clipped boxes within 4 px of each other.  That is every (box, shifted box) pair, and it merges
    what the scene itself repeats: the box it lists twice, the two boxes half a pixel apart, the two boxes of the 40 x 30 frame that clip to the whole frame."""
    group = np.arange(len(p9))
    for i in range(len(p9)):
        for j in range(i):
            if p9[i, 0] == p9[j, 0] and np.abs(p9[i, 1:5] - p9[j, 1:5]).max() <= 4:
                group[i] = group[j]
                break
    return group


def test_infer_boxes_with_nms_on_the_doubled_scene(eng):
    import torch
    frames, boxes, fidx = doubled_scene()
    n = len(boxes) // 2
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    d_boxes, d_fidx = torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda()
    cfg = PoseNms(oks_thr=0.5)
    plain = eng.infer_boxes(d_frames, d_boxes, d_fidx)
    out, score, rank, count, cp, st = eng.infer_boxes(d_frames, d_boxes, d_fidx, nms=cfg, crop_params=True, status=True)
    torch.cuda.synchronize()
    assert torch.equal(out, plain), 'out has the bits of the plain call'
    out, score, rank, count, cp, st = (t.cpu().numpy() for t in (out, score, rank, count, cp, st))
    assert (st == 0).all()
    ws, wr, wc = eng.pose_nms_host(out, boxes[:, 4].copy(), cp, len(frames), cfg, status=st)
    ms, mr, mc = nms_host(out, boxes[:, 4].copy(), cp, len(frames), cfg, sigmas17(), status=st)
    assert np.array_equal(rank, wr) and np.array_equal(score.view(np.int32), ws.view(np.int32)) and np.array_equal(count, wc)
    assert np.array_equal(rank, mr) and np.array_equal(score.view(np.int32), ms.view(np.int32)) and np.array_equal(count, mc)
    # box_scores= instead of column 4, and a 4-column box tensor without scores
    o2, s2, r2, c2 = eng.infer_boxes(d_frames, d_boxes[:, :4].contiguous(), d_fidx, nms=cfg, box_scores=d_boxes[:, 4].contiguous())
    assert torch.equal(torch.from_numpy(rank).cuda(), r2) and torch.equal(torch.from_numpy(score).cuda(), s2)
    with pytest.raises(ValueError, match='box scores'):
        eng.infer_boxes(d_frames, d_boxes[:, :4].contiguous(), d_fidx, nms=cfg)
    with pytest.raises(ValueError, match='datasets'):
        eng.infer_boxes(d_frames, d_boxes, d_fidx, nms=cfg, datasets=['coco'] * len(boxes))
    # exactly one of each pair survives
    oks = oks_tap(-1, out, cp, cfg, sigmas17())
    group = person_groups(cp)
    same = (group[:, None] == group[None, :]) & (cp[:, None, 0] == cp[None, :, 0])
    cross = (cp[:, None, 0] == cp[None, :, 0]) & ~same
    print(f'pairs (i, i + {n}): OKS min {min(oks[i, i + n] for i in range(n)):.3f}; same person min {oks[same].min():.3f}; different persons of a frame max {oks[cross].max():.3f}')
    for i in range(n):
        assert group[i] == group[i + n]
    for gid in np.unique(group):
        rows = np.flatnonzero(group == gid)
        assert (rank[rows] >= 0).sum() == 1, f'rows {rows.tolist()} show one person: ranks {rank[rows].tolist()}'
    assert count.sum() == len(np.unique(group))


@pytest.mark.parametrize('n', [12, 20])
def test_infer_boxes_with_nms_is_stream_ordered_without_host_blocking(n):
    """The pattern of test_infer_boxes_is_stream_ordered_without_host_blocking: a long producer in front, the call returns while the stream is busy, a
    consumer on the stream sees the finished ranks; then a side-stream call and a default-stream call on the same handle."""
    import torch
    frames, boxes, fidx = doubled_scene()
    sel = np.r_[0:n // 2, 19:19 + n // 2]   # boxes and their shifted copies
    boxes, fidx = boxes[sel], fidx[sel]
    src_frames = [torch.from_numpy(f).cuda() for f in frames]
    src_boxes, src_fidx = torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda()
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=32)
    cfg = PoseNms(oks_thr=0.5)
    torch.cuda.synchronize()
    want = [t.cpu().numpy() for t in eng.infer_boxes(src_frames, src_boxes, src_fidx, nms=cfg)]
    assert (want[2] < 0).any() and (want[2] >= 0).any()
    out = torch.empty((n, 17, 3), device='cuda')
    for _ in range(2):
        cur = torch.cuda.current_stream()
        torch.cuda._sleep(1_000_000_000)
        d_frames = [f.clone() for f in src_frames]
        d_boxes, d_fidx = src_boxes.clone() + 0.0, src_fidx.clone()
        out.fill_(float('nan'))
        _, score, rank, count = eng.infer_boxes(d_frames, d_boxes, d_fidx, out=out, nms=cfg)
        assert not cur.query(), 'the call blocked the host until the stream drained'
        kept = (rank >= 0).sum() + 0 * score.sum().long()   # a consumer on the same stream
        cur.synchronize()
        assert kept.item() == (want[2] >= 0).sum()
        for got, w in zip((out, score, rank, count), want):
            assert np.array_equal(got.cpu().numpy(), w)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(300_000_000)
        r1 = eng.infer_boxes(src_frames, src_boxes, src_fidx, nms=cfg)
    r2 = eng.infer_boxes(src_frames, src_boxes, src_fidx, nms=cfg)
    torch.cuda.synchronize()
    for got in (r1, r2):
        for t, w in zip(got, want):
            assert np.array_equal(t.cpu().numpy(), w)
    eng.close()


def test_vitinference_with_pose_nms():
    from helpers import weights
    from easy_vitpose_amd.synth import synthetic_crops
    shp, sd, _ = weights('s', 'coco')
    frame = np.zeros((480, 640, 3), np.uint8)
    crops = synthetic_crops(2, 4, 'blobs')
    frame[100:356, 50:242] = crops[0]
    frame[150:406, 400:592] = crops[1]
    boxes = np.array([[60, 110, 232, 346, 0.9], [410, 160, 582, 396, 0.8], [0, 0, 50, 50, 0.2]], dtype=np.float64)
    twice = np.repeat(boxes, 2, axis=0)   # the detector hands every box over twice
    plain = VitInference(sd, lambda img: twice.copy(), model_name='s', dataset='coco', max_batch=8)
    before = plain.inference(frame.copy())
    assert sorted(before.keys()) == [0, 1, 2, 3] and plain._scores_bbox == {0: 0.9, 1: 0.9, 2: 0.8, 3: 0.8}   # pose_nms=None: today's output
    cfg = PoseNms(oks_thr=0.5)
    model = VitInference(sd, lambda img: twice.copy(), model_name='s', dataset='coco', max_batch=8, pose_nms=cfg)
    res = model.inference(frame.copy())
    kp = np.stack([before[i] for i in range(4)])
    p9 = np.zeros((4, 9), np.int32)
    p9[:, 1:5] = [[b[0], b[1], b[2] - b[0], b[3] - b[1]] for b in model._tracker_res[0]]   # the padded, clipped boxes (the in-place box update)
    ws, wr, _ = nms_host(kp, np.array([0.9, 0.9, 0.8, 0.8], np.float32), p9, 1, cfg, sigmas17())
    kept = [i for i in range(4) if wr[i] >= 0]
    assert len(kept) == 2 and kept[0] in (0, 1) and kept[1] in (2, 3), 'one id per person'
    assert sorted(res.keys()) == kept
    for i in kept:
        assert np.array_equal(res[i], before[i])
    assert model._scores_bbox == {i: float(ws[i]) for i in kept} and 0 < ws[kept[1]] < 0.8
    assert model._keypoints is res
