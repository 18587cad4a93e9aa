"""GPU: the box tracker on the device (vp_tracker_update_stream / vp_tracker_update, VitPoseHip.tracker, VitInference(tracker='device')) against the host model
of the same header (vp_dbg_track_host / vp_dbg_lsap(-1), pinned on the CPU against the Python twin, the reference and scipy: tests/test_track_host.py).  The
header fixes every operation's order, so equal means equal bits: rows, ids, streams, counts, flags and the whole state."""
from __future__ import annotations

import warnings

import numpy as np
import pytest

from easy_vitpose_amd import Frame, VitInference, VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devtracker import FLAG_BAD_ROW, FLAG_BIRTHS, FLAG_DETS, FLAG_ROWS, DeviceTracker, HostTracker, TrackCfg
from easy_vitpose_amd.draw import DrawStyle, draw_poses_numpy
from easy_vitpose_amd.posenms import PoseNms
from easy_vitpose_amd.synth import synthetic_state_dict
from easy_vitpose_amd.tracker import Sort
from track_cases import IOU_THRESHOLD, LSAP_DENSITIES, LSAP_SIZES, all_sequences, edge_scenarios, interleaved_streams, lsap_matrix, same_bits

pytestmark = pytest.mark.gpu
SEQUENCES = {tag: (frames, age, hits) for tag, frames, age, hits in all_sequences()}
SCENARIOS = edge_scenarios()
NAMES = ('rows', 'ids', 'stream', 'count', 'flags')


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def both(eng, cfg, calls):
    """the calls on a device tracker (the synchronous twin) and on the host tap: every output of every call and the final state, bit for bit; -> the tap's outputs"""
    dev, tap = DeviceTracker(eng, cfg), HostTracker(cfg)
    outs = []
    for i, c in enumerate(calls):
        got, want = dev.update_host(**c), tap.update(**c)
        for name, g, w in zip(NAMES, got, want):
            assert same_bits(g, w), f'call {i}: {name} differs\n{g}\n{w}'
        outs.append(want)
    assert dev.state().tobytes() == tap.state().tobytes(), 'the state after the last call'
    dev.close()
    return outs


@pytest.mark.parametrize('tag', list(SEQUENCES))
def test_device_equals_the_host_tap_on_the_sequences(eng, tag):
    frames, age, hits = SEQUENCES[tag]
    outs = both(eng, TrackCfg(age, hits, IOU_THRESHOLD, 1), [dict(dets=d, n_out=128) for d in frames])
    assert sum(int(o[3][-1]) for o in outs) > 50 and all(o[4][0] == 0 for o in outs)


@pytest.mark.parametrize('n_dets', [8, 0], ids=['dets_8', 'dets_0'])
@pytest.mark.parametrize('frame_index', [True, False], ids=['frame_index', 'no_frame_index'])
def test_host_arrays_with_frame_index_absent_and_with_zero_rows(eng, frame_index, n_dets):
    """vp_tracker_update on host arrays with frame_index given or null, with at most 8 detections or none, with and without room for output rows: every output
    and the final state equal the host tap bit for bit"""
    frames, age, hits = SEQUENCES[next(iter(SEQUENCES))]
    calls = [dict(dets=d[:n_dets], frame_index=np.zeros(len(d[:n_dets]), np.int32) if frame_index else None, n_out=n_out) for d, n_out in zip(frames[:4], (8, 8, 0, 8))]
    both(eng, TrackCfg(age, hits, IOU_THRESHOLD, 1), calls)


def lsap(device_id, iou, thr):
    out = np.full(iou.shape[0], -7, np.int32)
    capi.check(capi.load_library().vp_dbg_lsap(device_id, iou.ctypes.data, iou.shape[0], iou.shape[1], thr, out.ctypes.data))
    return out


@pytest.mark.parametrize('nd', LSAP_SIZES)
def test_assignment_on_the_device_equals_the_host(nd):
    """63, 64 and 65 straddle a wave, 128 is the capacity; both the assignment (a threshold under every entry) and the shortcut / filter at 0.3"""
    paired = 0
    for nt in LSAP_SIZES:
        for dens in LSAP_DENSITIES:
            iou = lsap_matrix(nd, nt, dens)
            for thr in (1e-30, IOU_THRESHOLD):
                got, want = lsap(0, iou, thr), lsap(-1, iou, thr)
                assert np.array_equal(got, want), (nd, nt, dens, thr)
                paired += int((want >= 0).sum())
    assert paired > 0


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_edge_calls_against_the_tap(eng, name):
    (age, hits, ns), calls = SCENARIOS[name]
    outs = both(eng, TrackCfg(age, hits, IOU_THRESHOLD, ns), calls)
    flags = [o[4].tolist() for o in outs]
    if name == 'dets_128':
        assert flags == [[0], [0]] and outs[1][3].tolist() == [128, 128]
    if name == 'dets_129':
        assert flags == [[FLAG_DETS], [FLAG_DETS]] and outs[1][3].tolist() == [128, 128]
    if name == 'births_at_128':
        assert flags == [[0], [FLAG_BIRTHS], [0], [0]] and outs[1][3][-1] == 122
    if name == 'n_out_one_short':
        assert flags == [[FLAG_ROWS], [0], [FLAG_ROWS]] and [o[3].tolist() for o in outs] == [[7, 7], [7, 7], [7, 7]], 'the count keeps the true total'
    if name == 'nan_rows_and_bad_streams':
        assert flags == [[FLAG_BAD_ROW, FLAG_BAD_ROW], [FLAG_BAD_ROW, 0], [FLAG_BAD_ROW, FLAG_BAD_ROW]]
    if name == 'rows_cut_in_front_of_an_empty_stream':   # stream 1 has no row: it is not flagged, whatever was cut in front of it
        assert flags == [[FLAG_ROWS, 0, FLAG_ROWS], [0, 0, FLAG_ROWS]] and [o[3].tolist() for o in outs] == [[3, 0, 2, 5]] * 2
    if name == 'zero_area_boxes':
        assert np.isnan(outs[0][0][:4, :4]).any() and not np.isnan(outs[0][0][2, :4]).any()


def test_streams_interleaved_equal_the_streams_alone(eng):
    calls, per = interleaved_streams()
    cfg = TrackCfg(1, 1, IOU_THRESHOLD, 64)
    outs = both(eng, cfg, [dict(dets=d, frame_index=fi, n_out=64 * 3 + 5) for d, fi in calls])
    dev = DeviceTracker(eng, cfg)
    for s in range(64):   # stream s alone on stream slot s of a fresh tracker: the same rows, the same state bytes
        for f, (d, fi) in enumerate(calls):
            rows, ids, stream, count, flags = dev.update_host(d[fi == s], frame_index=fi[fi == s], n_out=8, step=[s])
            sel = outs[f][2] == s
            assert count[s] == sel.sum() == count[-1] and same_bits(rows[:count[-1]], outs[f][0][sel]) and (stream[:count[-1]] == s).all()
    tap = HostTracker(cfg)
    for d, fi in calls:
        tap.update(d, frame_index=fi, n_out=0)
    st = dev.state()
    assert all(st[s].tobytes() == tap.state()[s].tobytes() for s in range(64)) and (st['frame_count'] == len(calls)).all()
    dev.close()


def test_step_mask_reset_and_run_to_run_identity(eng):
    import torch
    (age, hits, ns), calls = SCENARIOS['step_mask']
    cfg = TrackCfg(age, hits, IOU_THRESHOLD, ns)
    dev = DeviceTracker(eng, cfg)
    runs = []
    for run in range(3):
        outs = []
        for c in calls:
            before = dev.state()
            outs.append(dev.update_host(**c))
            after = dev.state()
            stepped = range(ns) if c['step'] is None else c['step']
            for s in range(ns):
                assert (after[s].tobytes() == before[s].tobytes()) == (s not in stepped), f'stream {s}'
        runs.append(outs)
        assert max(int(o[1].max()) for o in outs) > 3
        dev.reset()   # all streams: the next run starts from ids 1 again
        torch.cuda.synchronize()
        assert not dev.state().tobytes().strip(b'\0')
    for outs in runs[1:]:
        assert all(same_bits(a, b) for o, p in zip(outs, runs[0]) for a, b in zip(o, p)), 'three runs are bit-identical, ids included'
    dev.update_host(**calls[0])
    dev.reset([1])
    torch.cuda.synchronize()
    st = dev.state()
    assert st[1]['next_id'] == 0 and st[1]['n_tracks'] == 0 and st[0]['next_id'] > 0 and st[2]['next_id'] > 0
    rows, ids, stream, count, flags = dev.update_host(**calls[0])
    assert sorted(ids[stream == 1].tolist()) == list(range(1, int(count[1]) + 1)), 'a reset stream numbers from 1 again'
    # a partial reset and the default n_out: streams 0 and 2 keep their tracks and coast on an empty call; no row is cut
    dev.reset([1])
    assert dev.row_bound(0) == dev.row_bound(0) == 3 * 128, 'asking does not record'
    rows, ids, stream, count, flags = dev.update_host(np.empty((0, 5), np.float32))
    assert len(rows) == 3 * 128 and flags.tolist() == [0, 0, 0] and count[0] > 0 and count[1] == 0 and count[2] > 0 and count[-1] == (stream >= 0).sum()
    dev.close()


def test_the_chain_on_one_side_stream_without_a_synchronisation(eng):
    import torch
    rng = np.random.default_rng(5)
    rgb = [rng.integers(0, 256, (97, 131, 3), dtype=np.uint8) for _ in range(2)]
    dets = [np.array([[10, 8, 60, 90, 0.9], [70, 12, 125, 93, 0.8], [30, 5, 100, 88, 0.7]], np.float32),
            np.array([[12, 9, 62, 91, 0.85], [69, 11, 124, 92, 0.75], [32, 6, 102, 89, 0.65]], np.float32)]
    fidx = np.array([0, 0, 1], np.int32)
    cfg, style, n_out = PoseNms(oks_thr=0.5), DrawStyle(conf_thr=0.0, thickness=2), 5
    trk = eng.tracker(TrackCfg(1, 3, IOU_THRESHOLD, 2))
    d_dets = [torch.from_numpy(d).cuda() for d in dets]
    d_fidx = torch.from_numpy(fidx).cuda()
    fr = [Frame.rgb(torch.from_numpy(f).cuda()) for f in rgb]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):   # nothing but launches from the first tracker call to the drawing
        trk.update(d_dets[0], d_fidx, n_out=n_out)
        rows, ids, stream, count, flags = trk.update(d_dets[1], d_fidx, n_out=n_out)
        out, score, rank, kept, cp, st = eng.infer_boxes(fr, rows, stream, nms=cfg, crop_params=True, status=True)
        eng.draw_poses(fr, out, stream, style, rank=rank, ids=ids, boxes=rows)
    side.synchronize()
    rows_h, ids_h, stream_h = rows.cpu().numpy(), ids.cpu().numpy(), stream.cpu().numpy()
    assert count.cpu().tolist() == [2, 1, 3] and flags.cpu().tolist() == [0, 0] and stream_h.tolist() == [0, 0, 1, -1, -1]
    # the host route: tracker.Sort per stream on the same detections
    want = []
    for s in range(2):
        twin = Sort(1, 3, IOU_THRESHOLD)
        twin.update(dets[0][fidx == s].astype(np.float64))
        want.append(twin.update(dets[1][fidx == s].astype(np.float64)))
    want = np.concatenate(want)
    assert np.array_equal(ids_h[:3], want[:, 5].astype(np.int32)) and np.abs(rows_h[:3, :5] - want[:, :5]).max() < 1e-4
    assert np.isnan(rows_h[3:, :4]).all() and (ids_h[3:] == -1).all()
    # ... then the same entries on the downloaded rows, call by call
    fr2 = [Frame.rgb(torch.from_numpy(f).cuda()) for f in rgb]
    out2, score2, rank2, kept2, cp2, st2 = eng.infer_boxes(fr2, torch.from_numpy(rows_h).cuda(), torch.from_numpy(stream_h).cuda(), nms=cfg, crop_params=True, status=True)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(rank, rank2) and torch.equal(score, score2)
    kp, rk = out.cpu().numpy(), rank.cpu().numpy()
    assert st.cpu().tolist() == [0, 0, 0, 1, 1] and (kp[3:] == 0).all() and (rk[3:] == -1).all() and (rk[:3] >= 0).sum() >= 2 and np.abs(kp[:3]).max() > 0
    host = [Frame.rgb(f.copy()) for f in rgb]
    draw_poses_numpy(host, kp, stream_h, style, rank=rk, ids=ids_h, boxes=rows_h[:, :4])
    for f in range(2):
        assert np.array_equal(fr[f].planes[0].cpu().numpy(), host[f].planes[0]) and not np.array_equal(host[f].planes[0], rgb[f]), f'frame {f}'
    trk.close()


def test_vitinference_with_the_device_tracker_equals_the_default():
    from cases import frame_case
    from helpers import weights
    frame, boxes = frame_case()
    _, sd, _ = weights('s', 'coco')
    res = {}
    for which in (None, 'device'):
        model = VitInference(sd, lambda img: boxes.copy(), model_name='s', dataset='coco', max_batch=8, is_video=True, yolo_step=2, tracker=which)
        assert type(model.tracker).__name__ == ('Sort' if which is None else 'DeviceSort')
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res[which] = [model.inference(frame.copy()) for _ in range(5)] + model.inference_frames([frame.copy(), frame.copy()])
        model.reset()
        assert type(model.tracker).__name__ == ('Sort' if which is None else 'DeviceSort')
    assert sum(len(r) for r in res[None]) >= 7
    for a, b in zip(res[None], res['device']):
        assert list(a.keys()) == list(b.keys()) and all(np.array_equal(a[k], b[k]) for k in a)
