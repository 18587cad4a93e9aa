"""GPU: the skeleton overlay on the device (vp_draw_poses_stream / vp_draw_poses, VitPoseHip.draw_poses / draw_poses_host, VitInference.draw) against the host
model of the same header (vp_dbg_draw_host, pinned on the CPU against two restatements: tests/test_draw_host.py).  Every comparison is over every byte of
every plane buffer, pitch padding included: integer arithmetic, so equal means equal."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from easy_vitpose_amd import Frame, VitInference, VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.draw import DrawStyle, c_config, draw_poses_numpy, resolve_skeleton
from easy_vitpose_amd.posenms import PoseNms
from easy_vitpose_amd.synth import synthetic_state_dict
import draw_cases as dc

pytestmark = pytest.mark.gpu
CASES = dc.host_cases()


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_host_model_on_the_cpu_cases(eng, name):
    got, want = dc.run_device(CASES[name], eng), dc.run_tap(CASES[name])
    for p, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f'{name}: buffer {p} differs in {int((g != w).sum())} bytes'


OPTIONAL = ('rank', 'ids', 'boxes')


@pytest.mark.parametrize('absent', [tuple(k for k, bit in zip(OPTIONAL, (1, 2, 4)) if m & bit) for m in range(8)], ids=lambda a: 'no_' + '_'.join(a) if a else 'all_given')
def test_host_arrays_with_every_combination_of_optional_inputs_absent(eng, absent):
    """vp_draw_poses on host arrays with every subset of rank, ids and boxes null: 8 rows of 17 joints on one pitched 32 x 48 frame per format, the whole buffers
    equal the host tap's byte for byte"""
    rng = np.random.default_rng(11)
    kp = dc.people(rng, 8, 17, 32, 48, spread=12.0)
    given = dict(rank=[0, -1, 2, 1, 3, -1, 4, 5], ids=[7, 3, 3, 250, 0, 12, 1, 99], boxes=dc.boxes_of(kp, rng))
    cs = dc.case([(32, 48, 'rgb', 'bt601', 5), (32, 48, 'nv12', 'bt709', 6)], kp, np.arange(8) % 2, seed=3, **{k: None if k in absent else v for k, v in given.items()})
    got, want = dc.run_device(cs, eng), dc.run_tap(cs)
    assert dc.same(got, want) and not dc.same(want, dc.build_frames(cs['specs'], cs['seed'])[1]), 'equal, and something was drawn'


@pytest.mark.parametrize('fmt', ['rgb', 'nv12'])
def test_more_hits_on_one_tile_than_the_lds_list_holds(eng, fmt):
    """300 rows x 36 primitives on one 20 x 20 region: chunks of 256 records in which every record hits the same tiles, so the list fills and is resolved many times"""
    cs = dc.lds_list_case(fmt)
    want = dc.run_tap(cs)
    runs = [dc.run_device(cs, eng) for _ in range(3)]
    assert dc.same(runs[0], want)
    assert dc.same(runs[1], runs[0]) and dc.same(runs[2], runs[0]), 'three runs on fresh copies of the frame are byte-identical'


def test_hits_of_a_tile_straddle_the_chunk_boundary(eng):
    cs = dc.chunk_boundary_case()
    assert cs['kp'].shape[0] * (19 + 17) == 324
    assert dc.same(dc.run_device(cs, eng), dc.run_tap(cs))


def test_n_zero_and_the_record_limit(eng):
    img = np.full((16, 16, 3), 7, np.uint8)
    eng.draw_poses_host([img], np.zeros((0, 17, 3), np.float32), np.zeros(0, np.int32))
    assert (img == 7).all()
    with pytest.raises(ValueError, match='records'):
        eng.draw_poses_host([img], np.zeros((65536 // 36 + 1, 17, 3), np.float32), np.zeros(65536 // 36 + 1, np.int32))
    with pytest.raises(ValueError, match='needs its own'):
        eng.draw_poses_host([img], np.zeros((1, 133, 3), np.float32), np.zeros(1, np.int32))


def test_stream_entry_refuses_host_planes(eng):
    import torch
    img = np.zeros((16, 16, 3), np.uint8)
    table = (capi.vp_image * 1)(capi.vp_image((C.c_void_p * 2)(img.ctypes.data, None), (C.c_int64 * 2)(48, 0), 16, 16, 0, 0))
    kp, fi = torch.zeros((1, 17, 3), device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    c, keep = c_config(DrawStyle(), resolve_skeleton('coco', 17))
    rc = eng.lib.vp_draw_poses_stream(eng._h, table, 1, kp.data_ptr(), 1, 17, fi.data_ptr(), 1, None, None, None, 4, C.byref(c), None)
    assert rc == capi.VP_ERR_INVALID and 'not device memory' in capi.last_error(eng._h)
    with pytest.raises(TypeError):
        eng.draw_poses([img], kp, fi)


def stream_scene():
    """two 120 x 160 frames (RGB and NV12), 5 boxes, boxes 0 and 1 one pixel apart: the same person twice"""
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)
    y, uv = rng.integers(0, 256, (120, 160), dtype=np.uint8), rng.integers(0, 256, (60, 80, 2), dtype=np.uint8)
    boxes = np.array([[20, 10, 90, 110, 0.9], [21, 11, 91, 111, 0.8], [100, 30, 150, 100, 0.7], [10, 10, 70, 100, 0.9], [80, 20, 150, 115, 0.6]], np.float32)
    return rgb, y, uv, boxes, np.array([0, 0, 0, 1, 1], np.int32)


def test_stream_entry_behind_infer_boxes_and_pose_nms_on_one_side_stream(eng):
    import torch
    rgb, y, uv, boxes, fidx = stream_scene()
    cfg, style = PoseNms(oks_thr=0.5), DrawStyle(conf_thr=0.0, thickness=3)
    d_boxes, d_fidx = torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda()

    def frames():
        return [Frame.rgb(torch.from_numpy(rgb).cuda()), Frame.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), 'bt709')]
    plain = eng.infer_boxes(frames(), d_boxes, d_fidx)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    fr = frames()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):   # nothing but launches between the three calls
        out, score, rank, count, cp = eng.infer_boxes(fr, d_boxes, d_fidx, nms=cfg, crop_params=True)
        eng.draw_poses(fr, out, cp[:, 0], style, rank=rank, boxes=d_boxes)   # the frame index read in place at stride 9, the boxes at stride 5
    side.synchronize()
    assert torch.equal(out, plain), 'the keypoints equal the call without drawing'
    kp, rk = out.cpu().numpy(), rank.cpu().numpy()
    assert (rk < 0).any() and (rk >= 0).sum() >= 3, rk
    want = [Frame.rgb(rgb.copy()), Frame.nv12(y.copy(), uv.copy(), 'bt709')]
    draw_poses_numpy(want, kp, fidx, style, rank=rk, boxes=boxes[:, :4])
    for f in range(2):
        for p, (g, w) in enumerate(zip(fr[f].planes, want[f].planes)):
            assert np.array_equal(g.cpu().numpy(), w), f'frame {f} plane {p}'
    assert not np.array_equal(want[0].planes[0], rgb) and not np.array_equal(want[1].planes[0], y) and not np.array_equal(want[1].planes[1], uv)
    # the suppressed row leaves nothing: drawing without the rank mask differs
    unmasked = [Frame.rgb(rgb.copy()), Frame.nv12(y.copy(), uv.copy(), 'bt709')]
    draw_poses_numpy(unmasked, kp, fidx, style, boxes=boxes[:, :4])
    assert not np.array_equal(unmasked[0].planes[0], want[0].planes[0])


def test_device_planes_that_are_views_of_a_larger_buffer(eng):
    import torch
    cs = CASES['nv12_bt709_97x131']
    rng = np.random.default_rng(9)
    big = {k: rng.integers(0, 256, s, dtype=np.uint8) for k, s in (('rgb', (140, 200, 3)), ('y', (140, 200)), ('uv', (80, 100, 2)))}
    dev = {k: torch.from_numpy(v).cuda() for k, v in big.items()}
    d_frames = [Frame.rgb(dev['rgb'][30:127, 40:171]), Frame.nv12(dev['y'][30:127, 40:171], dev['uv'][20:69, 30:96], 'bt709')]
    h_frames = [Frame.rgb(big['rgb'][30:127, 40:171]), Frame.nv12(big['y'][30:127, 40:171], big['uv'][20:69, 30:96], 'bt709')]
    kp = np.concatenate([cs['kp'], cs['kp']])
    fi = np.array([0] * 4 + [1] * 4, np.int32)
    bx = np.concatenate([cs['boxes'], cs['boxes']])
    eng.draw_poses(d_frames, torch.from_numpy(kp).cuda(), torch.from_numpy(fi).cuda(), boxes=torch.from_numpy(bx).cuda())
    torch.cuda.synchronize()
    before = {k: v.copy() for k, v in big.items()}
    draw_poses_numpy(h_frames, kp, fi, boxes=bx)   # on the views of the host buffers: `big` now holds the expected whole buffers
    for k in big:
        assert np.array_equal(dev[k].cpu().numpy(), big[k]), f'{k}: the view or the bytes around it differ'
        assert not np.array_equal(big[k], before[k])


def test_vitinference_draw_returns_the_host_twins_picture():
    from helpers import weights
    from easy_vitpose_amd.synth import synthetic_crops
    shp, sd, _ = weights('s', 'coco')
    frame = np.zeros((240, 320, 3), np.uint8)
    crop = synthetic_crops(1, 4, 'blobs')[0]
    frame[20:220:1, 30:180] = crop[:200, :150]
    frame[30:230, 170:310] = crop[40:240, 40:180]
    boxes = np.array([[40, 30, 170, 210, 0.9], [180, 40, 300, 220, 0.8]], dtype=np.float64)
    for video in (False, True):
        model = VitInference(sd, lambda img: boxes.copy(), model_name='s', dataset='coco', max_batch=8, is_video=video)
        res = model.inference(frame.copy())
        assert len(res) == 2
        pic = model.draw(confidence_threshold=0.0)
        assert pic.shape == frame.shape and pic.dtype == np.uint8 and np.array_equal(model._img, frame), 'a copy is drawn on'
        ids = list(res.keys())
        want = frame.copy()
        bx = None
        if video:   # a tracker is on: box outlines under the skeletons
            box_of = dict(zip(model._tracker_res[1], model._tracker_res[0]))
            bx = np.array([box_of[i] for i in ids], np.float32)
        draw_poses_numpy([want], np.stack([res[i] for i in ids]), np.zeros(2, np.int32), DrawStyle(conf_thr=0.0), ids=np.array(ids, np.int32), boxes=bx)
        assert np.array_equal(pic, want) and not np.array_equal(pic, frame)
        if video:
            assert not np.array_equal(pic, model.draw(show_yolo=False, confidence_threshold=0.0))
    wb = VitInference(synthetic_state_dict(model_shape('s', 'wholebody'), 0, peaked=True), lambda img: boxes.copy(), model_name='s', dataset='wholebody', max_batch=8)
    wb.inference(frame.copy())
    with pytest.raises(ValueError, match='needs its own'):
        wb.draw()
