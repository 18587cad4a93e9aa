"""GPU: the label stage on the device (vp_draw_labels_stream / vp_draw_labels, VitPoseHip.draw_labels / draw_labels_host, draw_poses(labels=),
VitInference(labels=)) against the host model of the same header (vp_dbg_draw_labels_host, pinned on the CPU against two restatements and Python's formatter:
tests/test_label_host.py).  Every comparison is over every byte of every plane buffer, pitch padding included: integer arithmetic, so equal means equal."""
from __future__ import annotations

import ctypes as C
import types

import numpy as np
import pytest

from easy_vitpose_amd import Frame, VitInference, VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devtracker import TrackCfg
from easy_vitpose_amd.draw import DrawStyle, LabelStyle, draw_labels_model_host, draw_labels_numpy, draw_poses_numpy, label_c_config
from easy_vitpose_amd.posenms import PoseNms
from easy_vitpose_amd.synth import synthetic_state_dict
import label_cases as lc

pytestmark = pytest.mark.gpu
CASES = lc.host_cases()


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_host_model_on_the_cpu_cases(eng, name):
    got, want = lc.run_device(CASES[name], eng), lc.run_tap(CASES[name])
    for p, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f'{name}: buffer {p} differs in {int((g != w).sum())} bytes'


OPTIONAL = ('rank', 'ids', 'scores')


@pytest.mark.parametrize('absent', [tuple(k for k, bit in zip(OPTIONAL, (1, 2, 4)) if m & bit) for m in range(8)], ids=lambda a: 'no_' + '_'.join(a) if a else 'all_given')
def test_host_arrays_with_every_combination_of_optional_inputs_absent(eng, absent):
    """vp_draw_labels on host arrays with every subset of rank, ids and scores null: 8 rows on one pitched 32 x 48 frame per format, the whole buffers equal the
    host tap's byte for byte"""
    rng = np.random.default_rng(12)
    given = dict(rank=[0, -1, 2, 1, 3, -1, 4, 5], ids=[7, 3, -3, 250, 0, 12, 1, 99], scores=rng.uniform(0, 1, 8))
    cs = lc.case([(32, 48, 'rgb', 'bt601', 5), (32, 48, 'nv12', 'bt709', 6)], lc.crowd(rng, 8, 24, 40), np.arange(8) % 2, LabelStyle(scale=1), seed=4,
                 **{k: None if k in absent else v for k, v in given.items()})
    got, want = lc.run_device(cs, eng), lc.run_tap(cs)
    assert lc.same(got, want) and not lc.same(want, lc.build_frames(cs['specs'], cs['seed'])[1]), 'equal, and something was drawn'


def test_three_runs_are_bit_identical(eng):
    for name in ('overlap3', 'edges_nv12'):
        runs = [lc.run_device(CASES[name], eng) for _ in range(3)]
        assert lc.same(runs[0], lc.run_tap(CASES[name])) and lc.same(runs[1], runs[0]) and lc.same(runs[2], runs[0]), name


@pytest.mark.parametrize('fmt', ['rgb', 'nv12'])
def test_more_later_rows_than_one_chunk_of_the_scan(eng, fmt):
    """600 overlapping tags on one 64 x 96 frame: the later rows of a tile come in up to three chunks of 256 records"""
    cs = lc.crowd_case(fmt)
    want = lc.run_tap(cs)
    runs = [lc.run_device(cs, eng) for _ in range(2)]
    assert lc.same(runs[0], want) and lc.same(runs[1], runs[0])


def test_n_zero_and_the_row_limit(eng):
    img = np.full((16, 16, 3), 7, np.uint8)
    eng.draw_labels_host([img], np.zeros((0, 4), np.float32), np.zeros(0, np.int32))
    assert (img == 7).all()
    with pytest.raises(ValueError, match='8192'):
        eng.draw_labels_host([img], np.zeros((8193, 4), np.float32), np.zeros(8193, np.int32))
    with pytest.raises(ValueError, match='boxes are required'):
        eng.draw_labels_host([img], None, np.zeros(0, np.int32))


def test_33_frames_cross_the_launch_boundary(eng):
    """the table runs 32 frames per launch: rows of frames 31 and 32 sit in different launches, and the records of one launch are empty in the other"""
    rng = np.random.default_rng(8)

    def frames():
        r = np.random.default_rng(9)
        out = []
        for f in range(33):
            if f % 2:
                out.append(Frame.nv12(r.integers(0, 256, (16, 16), dtype=np.uint8), r.integers(0, 256, (8, 8, 2), dtype=np.uint8), 'bt601'))
            else:
                out.append(Frame.rgb(r.integers(0, 256, (16, 16, 3), dtype=np.uint8)))
        return out
    fi = np.concatenate([np.arange(33), [31, 32, 0, 32, 31]]).astype(np.int32)[::-1].copy()   # descending, so the second launch's rows come first
    bx = np.stack([rng.uniform(-3, 6, 38), rng.uniform(8, 15, 38), np.full(38, 20.0), np.full(38, 20.0)], -1).astype(np.float32)
    ids, sc = rng.integers(-9, 99, 38).astype(np.int32), rng.uniform(0, 1, 38).astype(np.float32)
    got, want = frames(), frames()
    eng.draw_labels_host(got, bx, fi, LabelStyle(scale=1), ids=ids, scores=sc)
    draw_labels_model_host(want, bx, fi, LabelStyle(scale=1), ids=ids, scores=sc)
    before = frames()
    for f in range(33):
        for p, (g, w, b) in enumerate(zip(got[f].planes, want[f].planes, before[f].planes)):
            assert np.array_equal(g, w), f'frame {f} plane {p}'
            assert not np.array_equal(w, b), f'frame {f} plane {p}: nothing written'


def test_stream_entry_on_strided_views(eng):
    """scores read in place from column 4 of the [n, 6] rows, the frame index from column 0 of an [n, 9] tensor, the frames ROI views of larger buffers: the
    views and every byte around them equal the numpy twin's"""
    import torch
    rng = np.random.default_rng(9)
    big = {k: rng.integers(0, 256, s, dtype=np.uint8) for k, s in (('rgb', (140, 200, 3)), ('y', (140, 200)), ('uv', (80, 100, 2)))}
    dev = {k: torch.from_numpy(v).cuda() for k, v in big.items()}
    d_frames = [Frame.rgb(dev['rgb'][30:127, 40:171]), Frame.nv12(dev['y'][30:127, 40:171], dev['uv'][20:69, 30:96], 'bt709')]
    h_frames = [Frame.rgb(big['rgb'][30:127, 40:171]), Frame.nv12(big['y'][30:127, 40:171], big['uv'][20:69, 30:96], 'bt709')]
    n = 8
    rows = np.zeros((n, 6), np.float32)
    rows[:, :4] = np.concatenate([lc.crowd(rng, 4, 97, 131), lc.crowd(rng, 4, 97, 131)])
    rows[:, 4] = [0.125, 0.375, 0.5, -0.0, 0.87, np.nan, 999.99994, 0.004]
    rows[:, 5] = 77.0
    rows[5, :4] = np.nan   # an absent tracker row
    p9 = np.full((n, 9), 5, np.int32)
    p9[:, 0] = [0, 1, 0, 1, 0, 1, 1, 0]
    ids = np.array([1, 2, 3, -4, 5, -1, 70, 8], np.int32)
    rank = np.array([0, 1, -1, 2, 3, 0, 4, 5], np.int32)
    d_rows, d_p9 = torch.from_numpy(rows).cuda(), torch.from_numpy(p9).cuda()
    style = LabelStyle(scale=2)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eng.draw_labels(d_frames, d_rows, d_p9[:, 0], style, rank=torch.from_numpy(rank).cuda(), ids=torch.from_numpy(ids).cuda(), scores=d_rows[:, 4])
    side.synchronize()
    before = {k: v.copy() for k, v in big.items()}
    draw_labels_numpy(h_frames, rows[:, :4], p9[:, 0], style, rank=rank, ids=ids, scores=rows[:, 4])   # on the views of the host buffers
    for k in big:
        assert np.array_equal(dev[k].cpu().numpy(), big[k]), f'{k}: the view or the bytes around it differ'
        assert not np.array_equal(big[k], before[k])
    assert np.array_equal(d_rows.cpu().numpy(), rows, equal_nan=True) and np.array_equal(d_p9.cpu().numpy(), p9)


def test_the_chain_on_one_side_stream_without_a_synchronisation(eng):
    """tracker.update -> infer_boxes(nms=) -> draw_poses(labels=, ids=, boxes=rows): two 97 x 131 frames, 3 persons and 2 absent rows"""
    import torch
    rng = np.random.default_rng(5)
    rgb = [rng.integers(0, 256, (97, 131, 3), dtype=np.uint8) for _ in range(2)]
    dets = [np.array([[10, 18, 60, 90, 0.9], [70, 22, 125, 93, 0.8], [30, 15, 100, 88, 0.7]], np.float32),
            np.array([[12, 19, 62, 91, 0.85], [69, 21, 124, 92, 0.75], [32, 16, 102, 89, 0.65]], np.float32)]
    fidx = np.array([0, 0, 1], np.int32)
    cfg, style, labels, n_out = PoseNms(oks_thr=0.5), DrawStyle(conf_thr=0.0, thickness=2), LabelStyle(scale=1), 5
    trk = eng.tracker(TrackCfg(1, 3, 0.3, 2))
    d_dets = [torch.from_numpy(d).cuda() for d in dets]
    d_fidx = torch.from_numpy(fidx).cuda()
    fr = [Frame.rgb(torch.from_numpy(f).cuda()) for f in rgb]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):   # nothing but launches from the first tracker call to the drawing
        trk.update(d_dets[0], d_fidx, n_out=n_out)
        rows, ids, stream, count, flags = trk.update(d_dets[1], d_fidx, n_out=n_out)
        out, score, rank, kept, cp = eng.infer_boxes(fr, rows, stream, nms=cfg, crop_params=True)
        eng.draw_poses(fr, out, stream, style, rank=rank, ids=ids, boxes=rows, labels=labels, scores=rows[:, 4])
    side.synchronize()
    rows_h, ids_h, stream_h = rows.cpu().numpy(), ids.cpu().numpy(), stream.cpu().numpy()
    assert stream_h.tolist() == [0, 0, 1, -1, -1] and np.isnan(rows_h[3:, :4]).all() and (ids_h[3:] == -1).all() and (ids_h[:3] >= 0).all()
    # the same entries on the downloaded rows, call by call
    fr2 = [Frame.rgb(torch.from_numpy(f).cuda()) for f in rgb]
    rows2, stream2, ids2 = torch.from_numpy(rows_h).cuda(), torch.from_numpy(stream_h).cuda(), torch.from_numpy(ids_h).cuda()
    out2, score2, rank2, kept2, cp2 = eng.infer_boxes(fr2, rows2, stream2, nms=cfg, crop_params=True)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(rank, rank2)
    eng.draw_labels(fr2, rows2, stream2, labels, rank=rank2, ids=ids2, scores=rows2[:, 4])
    eng.draw_poses(fr2, out2, stream2, style, rank=rank2, ids=ids2, boxes=rows2)
    torch.cuda.synchronize()
    kp, rk = out.cpu().numpy(), rank.cpu().numpy()
    assert (rk[3:] == -1).all() and (rk[:3] >= 0).sum() >= 2
    host = [Frame.rgb(f.copy()) for f in rgb]
    draw_poses_numpy(host, kp, stream_h, style, rank=rk, ids=ids_h, boxes=rows_h[:, :4], labels=labels, scores=rows_h[:, 4])
    plain = [Frame.rgb(f.copy()) for f in rgb]
    draw_poses_numpy(plain, kp, stream_h, style, rank=rk, ids=ids_h, boxes=rows_h[:, :4])
    for f in range(2):
        got = fr[f].planes[0].cpu().numpy()
        assert np.array_equal(got, fr2[f].planes[0].cpu().numpy()), f'frame {f}: the chain and the entries one by one'
        assert np.array_equal(got, host[f].planes[0]), f'frame {f}: the device and the numpy twin'
        assert not np.array_equal(got, plain[f].planes[0]), f'frame {f}: no tag written'
    trk.close()


def test_host_pointers_and_frames_of_another_device_are_refused_before_anything_is_enqueued(eng):
    import torch
    img = np.full((16, 16, 3), 7, np.uint8)
    table = (capi.vp_image * 1)(capi.vp_image((C.c_void_p * 2)(img.ctypes.data, None), (C.c_int64 * 2)(48, 0), 16, 16, 0, 0))
    bx, fi = torch.tensor([[1.0, 12.0, 9.0, 15.0]], device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    c, keep = label_c_config(LabelStyle())
    rc = eng.lib.vp_draw_labels_stream(eng._h, table, 1, bx.data_ptr(), 4, 1, fi.data_ptr(), 1, None, None, None, 1, C.byref(c), None)
    assert rc == capi.VP_ERR_INVALID and 'not device memory' in capi.last_error(eng._h) and capi.last_error(eng._h).startswith('labels: ')
    torch.cuda.synchronize()
    assert (img == 7).all()
    with pytest.raises(TypeError, match='frame 0'):
        eng.draw_labels([img], bx, fi)
    with pytest.raises(TypeError, match='boxes'):
        eng.draw_labels([torch.zeros((16, 16, 3), dtype=torch.uint8, device='cuda')], bx.cpu().numpy(), fi)
    with pytest.raises(ValueError, match='boxes are required'):
        eng.draw_poses([torch.zeros((16, 16, 3), dtype=torch.uint8, device='cuda')], torch.zeros((1, 17, 3), device='cuda'), fi, labels=LabelStyle())
    # a handle of another device: the Python layer refuses the frame (and the row tensors) before the library is reached -- lib is None here
    d_img = torch.full((16, 16, 3), 7, dtype=torch.uint8, device='cuda')
    elsewhere = types.SimpleNamespace(device_id=eng.device_id + 1, lib=None, _h=None, _as_frame=VitPoseHip._as_frame)
    elsewhere._image_table = types.MethodType(VitPoseHip._image_table, elsewhere)
    with pytest.raises(ValueError, match=rf'frame 0 lives on cuda:{eng.device_id}, the handle on cuda:{eng.device_id + 1}'):
        elsewhere._image_table([Frame.rgb(d_img)], device_only=True)
    with pytest.raises(ValueError, match=f'on cuda:{eng.device_id + 1} expected'):
        VitPoseHip.draw_labels(elsewhere, [d_img], bx, fi)
    if torch.cuda.device_count() > 1:   # the C entry's own check, where a second device exists
        other = torch.full((16, 16, 3), 7, dtype=torch.uint8, device=f'cuda:{(eng.device_id + 1) % torch.cuda.device_count()}')
        table = (capi.vp_image * 1)(capi.vp_image((C.c_void_p * 2)(other.data_ptr(), None), (C.c_int64 * 2)(48, 0), 16, 16, 0, 0))
        rc = eng.lib.vp_draw_labels_stream(eng._h, table, 1, bx.data_ptr(), 4, 1, fi.data_ptr(), 1, None, None, None, 1, C.byref(c), None)
        assert rc == capi.VP_ERR_INVALID and 'not device memory of device' in capi.last_error(eng._h)
        assert (other == 7).all()
    torch.cuda.synchronize()
    assert (d_img == 7).all()


def test_vitinference_labels_on_the_frame_goldens_video_loop():
    """VitInference(labels=True).draw() equals the twin (tags from the tracker's result, under the skeletons); labels=False, the default, leaves today's picture"""
    from cases import frame_case
    from helpers import weights
    frame, boxes = frame_case()
    _, sd, _ = weights('s', 'coco')
    pics = {}
    for which in (False, True, LabelStyle(scale=2, show_score=False)):
        model = VitInference(sd, lambda img: boxes.copy(), model_name='s', dataset='coco', max_batch=8, is_video=True, labels=which)
        for _ in range(3):
            res = model.inference(frame.copy())
        assert len(res) >= 2
        pic = model.draw(confidence_threshold=0.0)
        ids = list(res.keys())
        box_of, score_of = dict(zip(model._tracker_res[1], model._tracker_res[0])), dict(zip(model._tracker_res[1], model._tracker_res[2]))
        bx = np.array([box_of[i] for i in ids], np.float32)
        sc = np.array([score_of[i] for i in ids], np.float32)
        want = frame.copy()
        draw_poses_numpy([want], np.stack([res[i] for i in ids]), np.zeros(len(ids), np.int32), DrawStyle(conf_thr=0.0), ids=np.array(ids, np.int32), boxes=bx,
                         labels=None if which is False else (LabelStyle() if which is True else which), scores=sc)
        assert np.array_equal(pic, want) and not np.array_equal(pic, frame), which
        if which is not False:   # without show_yolo there is no box, and no tag
            assert np.array_equal(model.draw(show_yolo=False, confidence_threshold=0.0), pics['plain_no_yolo'])
        else:
            pics['plain_no_yolo'] = model.draw(show_yolo=False, confidence_threshold=0.0)
        pics[str(which)] = pic
    assert not np.array_equal(pics['False'], pics['True']) and not np.array_equal(pics['True'], pics[str(LabelStyle(scale=2, show_score=False))])
    # the keyword left out: the picture of the overlay alone, as before the label stage existed
    model = VitInference(sd, lambda img: boxes.copy(), model_name='s', dataset='coco', max_batch=8, is_video=True)
    for _ in range(3):
        res = model.inference(frame.copy())
    assert np.array_equal(model.draw(confidence_threshold=0.0), pics['False'])


def test_cli_labels_write_the_tags_into_the_saved_frames(tmp_path):
    import json
    from PIL import Image
    from easy_vitpose_amd import cli
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, size=(2, 120, 160, 3), dtype=np.uint8)
    boxes = [[[20, 30, 70, 110, 0.9], [90, 25, 150, 105, 0.8]]] * 2
    np.save(tmp_path / 'clip.npy', frames)
    (tmp_path / 'boxes.json').write_text(json.dumps(boxes))
    base = ['--input', str(tmp_path / 'clip.npy'), '--synthetic', 's', '--dataset', 'coco', '--boxes', str(tmp_path / 'boxes.json'), '--max-batch', '4', '--save-img']
    pics = {}
    for name, extra in (('plain', []), ('labels', ['--labels']), ('scale2', ['--label-scale', '2'])):
        assert cli.main(base + ['--output-path', str(tmp_path / name)] + extra) == 0
        pics[name] = np.asarray(Image.open(tmp_path / name / 'clip.npy' / 'clip_1.png'))
        assert pics[name].shape == (120, 160, 3)
    assert not np.array_equal(pics['plain'], pics['labels']) and not np.array_equal(pics['labels'], pics['scale2'])
    diff = (pics['plain'] != pics['labels']).any(-1)
    ys, xs = np.nonzero(diff)
    # the boxes VitInference keeps are the detector's plus 10 px on every side: their top-left corners are (10, 20) and (80, 15), the tags sit above them
    assert ys.max() < 20 and xs.min() >= 10 and ys.min() >= 15 - 9, 'nothing but the tags changes'
    with pytest.raises(ValueError, match='LabelStyle'):
        cli.main(base + ['--output-path', str(tmp_path / 'bad'), '--label-scale', '9'])
