"""GPU: One-Euro keypoint smoothing on the device (vp_smooth_update_stream / vp_smooth_update, VitPoseHip.smoother, VitInference(smooth=)) against the host model
of the same header (vp_dbg_smooth_host, pinned on the CPU against the reference and the numpy twin: tests/test_smooth_host.py).  The header fixes every
operation's order, so equal means equal bits: keypoints, flags and the whole state."""
from __future__ import annotations

import warnings

import numpy as np
import pytest

from easy_vitpose_amd import Frame, VitInference, VitPoseHip
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devsmooth import FLAG_FULL, DeviceSmoother, HostSmoother, SmoothCfg
from easy_vitpose_amd.devtracker import TrackCfg
from easy_vitpose_amd.draw import DrawStyle, draw_poses_numpy
from easy_vitpose_amd.posenms import PoseNms
from easy_vitpose_amd.smooth import OneEuro
from easy_vitpose_amd.synth import synthetic_state_dict
from smooth_cases import SEQUENCES, interleaved_streams, same_bits, sequence, table_full, tag_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def both(eng, K, cfg_kw, calls, in_place=False):
    """the calls on a device smoother and on the host tap: keypoints and flags of every call, the state after every call, bit for bit; -> the tap's outputs.
    `in_place`: the device runs through the stream entry on torch tensors with out = kpts."""
    import torch
    cfg = SmoothCfg(**cfg_kw)
    dev, tap = DeviceSmoother(eng, K, cfg), HostSmoother(K, cfg)
    outs = []
    for i, c in enumerate(calls):
        if 'reset' in c:
            dev.reset(c['reset'])
            torch.cuda.synchronize()   # the reset is ordered on torch's stream, the synchronous twin runs on the handle's own
            tap.reset(c['reset'])
            continue
        want = tap.update(**c)
        if in_place:
            t = {k: None if c[k] is None else torch.from_numpy(c[k]).cuda() for k in ('kpts', 'ids', 'stream', 'rank')}
            out, flags = dev.update(t['kpts'], t['ids'], t['stream'], t['rank'], t_e=c['t_e'], step_mask=c['step_mask'], out=t['kpts'])
            assert out is t['kpts']
            got = (out.cpu().numpy(), flags.cpu().numpy())
        else:
            got = dev.update_host(**c)
        assert same_bits(got[0], want[0]), f'call {i}: keypoints differ'
        assert got[1].tolist() == want[1].tolist(), f'call {i}: flags'
        assert dev.state().tobytes() == tap.state().tobytes(), f'call {i}: state'
        outs.append(want)
    dev.close()
    return outs


@pytest.mark.parametrize('case', SEQUENCES, ids=tag_of)
def test_device_equals_the_host_tap_on_the_sequences(eng, case):
    cfg_kw, calls = sequence(case)
    outs = both(eng, case[1], cfg_kw, calls)
    assert sum(not same_bits(o, c['kpts']) for (o, _), c in zip(outs, [c for c in calls if 'reset' not in c])) >= 5


@pytest.mark.parametrize('case', [SEQUENCES[2], SEQUENCES[5]], ids=tag_of)
def test_in_place_equals_out_of_place(eng, case):
    cfg_kw, calls = sequence(case)
    both(eng, case[1], cfg_kw, calls, in_place=True)   # against the tap, which `both` without in_place equals too: in place == out of place


OPTIONAL = ('stream', 'rank', 't_e')


@pytest.mark.parametrize('absent', [tuple(k for k, bit in zip(OPTIONAL, (1, 2, 4)) if m & bit) for m in range(8)], ids=lambda a: 'no_' + '_'.join(a) if a else 'all_given')
def test_host_arrays_with_every_combination_of_optional_inputs_absent(eng, absent):
    """vp_smooth_update on host arrays with every subset of stream, rank and t_e null, on calls of at most 8 rows of 17 joints and on one without rows:
    keypoints, flags and the state after every call equal the host tap bit for bit"""
    cfg_kw, seq = sequence(SEQUENCES[0])   # one stream: a null stream argument means the same table
    calls = []
    for c in [c for c in seq if 'reset' not in c and len(c['ids'])][:3]:
        n = min(len(c['ids']), 8)
        given = dict(kpts=c['kpts'][:n], ids=c['ids'][:n], stream=np.zeros(n, np.int32), rank=(np.arange(n, dtype=np.int32) % 3) - 1, t_e=2.0, step_mask=None)
        calls.append({k: None if k in absent else v for k, v in given.items()})
    calls.append({**calls[-1], 'kpts': np.zeros((0, 17, 3), np.float32), 'ids': np.zeros(0, np.int32), 'stream': None if 'stream' in absent else np.zeros(0, np.int32),
                  'rank': None if 'rank' in absent else np.zeros(0, np.int32)})
    both(eng, 17, cfg_kw, calls)


def test_table_full_on_the_device(eng):
    cfg_kw, calls = table_full()
    outs = both(eng, 17, cfg_kw, calls)
    assert [f.tolist() for _, f in outs] == [[FLAG_FULL], [FLAG_FULL]] and same_bits(outs[1][0][128], calls[1]['kpts'][128])


def test_streams_interleaved_equal_the_streams_alone(eng):
    cfg_kw, calls = interleaved_streams()
    outs = both(eng, 17, cfg_kw, calls)
    cfg = SmoothCfg(**cfg_kw)
    dev, tap = DeviceSmoother(eng, 17, cfg), HostSmoother(17, cfg)
    for c in calls:
        tap.update(**c)
    for s in range(64):   # stream s alone on table s of a fresh smoother: the same keypoints, the same state bytes
        for f, c in enumerate(calls):
            sel = c['stream'] == s
            out, flags = dev.update_host(c['kpts'][sel], c['ids'][sel], c['stream'][sel], t_e=c['t_e'], step_mask=[s])
            assert same_bits(out, outs[f][0][sel]) and not flags.any()
    st = dev.state()
    assert all(st[s].tobytes() == tap.state()[s].tobytes() for s in range(64)) and (st['frame_count'] == len(calls)).all()
    dev.close()


def test_step_mask_reset_and_run_to_run_identity(eng):
    import torch
    case = SEQUENCES[3]
    cfg_kw, calls = sequence(case)
    cfg = SmoothCfg(**cfg_kw)
    dev = DeviceSmoother(eng, case[1], cfg)
    ns, runs = cfg.n_streams, []
    for run in range(3):
        outs = []
        for c in calls:
            if 'reset' in c:
                dev.reset(c['reset'])
                torch.cuda.synchronize()
                continue
            before = dev.state()
            outs.append(dev.update_host(**c))
            after = dev.state()
            stepped = range(ns) if c['step_mask'] is None else c['step_mask']
            for s in range(ns):
                assert (after[s].tobytes() == before[s].tobytes()) == (s not in stepped), f'stream {s}'
        runs.append(outs)
        dev.reset()
        torch.cuda.synchronize()
        assert not dev.state().tobytes().strip(b'\0')
    assert any(c.get('step_mask') is not None for c in calls)
    for outs in runs[1:]:
        assert all(same_bits(a, b) for o, p in zip(outs, runs[0]) for a, b in zip(o, p)), 'three runs are bit-identical'
    first = next(c for c in calls if 'reset' not in c and len(c['ids']))
    dev.update_host(**{**first, 'step_mask': None})
    dev.reset([1])
    torch.cuda.synchronize()
    st = dev.state()
    assert st[1]['frame_count'] == 0 and not st[1]['last_seen'].any() and st[0]['frame_count'] == 1 and st[2]['frame_count'] == 1
    dev.close()


def test_the_chain_on_one_side_stream_without_a_synchronisation(eng):
    import torch
    rng = np.random.default_rng(5)
    rgb = [rng.integers(0, 256, (97, 131, 3), dtype=np.uint8) for _ in range(2)]
    base = np.array([[10, 8, 60, 90, 0.9], [70, 12, 125, 93, 0.8], [30, 5, 100, 88, 0.7]], np.float32)
    dets = [base + np.array([2 * t, t, 2 * t, t, -0.02 * t], np.float32) for t in range(4)]
    fidx = np.array([0, 0, 1], np.int32)
    nms, style, n_out = PoseNms(oks_thr=0.5), DrawStyle(conf_thr=0.0, thickness=2), 5
    scfg = SmoothCfg(fps=30.0, n_streams=2, max_rows=n_out)
    trk, smo = eng.tracker(TrackCfg(1, 3, 0.3, 2)), eng.smoother(scfg)
    d_dets = [torch.from_numpy(d).cuda() for d in dets]
    d_fidx = torch.from_numpy(fidx).cuda()
    frames = [[Frame.rgb(torch.from_numpy(f).cuda()) for f in rgb] for _ in range(4)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    with torch.cuda.stream(side):   # nothing but launches from the first tracker call to the last drawing
        for t in range(4):
            rows, ids, stream, count, flags = trk.update(d_dets[t], d_fidx, n_out=n_out)
            out, score, rank, kept, cp, st = eng.infer_boxes(frames[t], rows, stream, nms=nms, crop_params=True, status=True)
            smooth, sflags = smo.update(out, ids, stream, rank=rank)
            eng.draw_poses(frames[t], smooth, stream, style, rank=rank, ids=ids, boxes=rows)
            got.append((rows, ids, stream, out, rank, smooth, sflags))
    side.synchronize()
    tap = HostSmoother(eng.K, scfg)
    changed = 0
    for t, (rows, ids, stream, out, rank, smooth, sflags) in enumerate(got):
        rows_h, ids_h, stream_h = rows.cpu().numpy(), ids.cpu().numpy(), stream.cpu().numpy()
        assert stream_h.tolist() == [0, 0, 1, -1, -1] and ids_h[3:].tolist() == [-1, -1]
        # the same entries on the downloaded arrays, call by call
        fr2 = [Frame.rgb(torch.from_numpy(f).cuda()) for f in rgb]
        out2, score2, rank2, kept2, cp2, st2 = eng.infer_boxes(fr2, torch.from_numpy(rows_h).cuda(), torch.from_numpy(stream_h).cuda(), nms=nms, crop_params=True, status=True)
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(rank, rank2)
        kp, rk = out2.cpu().numpy(), rank2.cpu().numpy()
        want, wflags = tap.update(kp, ids_h, stream_h, rank=rk)
        assert same_bits(smooth.cpu().numpy(), want) and sflags.cpu().tolist() == wflags.tolist() == [0, 0], f'video frame {t}'
        assert same_bits(want[3:], kp[3:]) and same_bits(want[rk < 0], kp[rk < 0]), 'absent and suppressed rows pass through'
        changed += int(not same_bits(want, kp))
        host = [Frame.rgb(f.copy()) for f in rgb]
        draw_poses_numpy(host, want, stream_h, style, rank=rk, ids=ids_h, boxes=rows_h[:, :4])
        for f in range(2):
            assert np.array_equal(frames[t][f].planes[0].cpu().numpy(), host[f].planes[0]) and not np.array_equal(host[f].planes[0], rgb[f]), f'video frame {t}, frame {f}'
    assert changed >= 2, 'the filter moved keypoints'
    assert smo.state().tobytes() == tap.state().tobytes()
    trk.close()
    smo.close()


def test_vitinference_smooth_equals_the_twin_on_the_unsmoothed_run():
    from cases import frame_case
    from helpers import weights
    frame, boxes = frame_case()
    _, sd, _ = weights('s', 'coco')
    res, custom = {}, SmoothCfg(fps=25.0, missing='restart', max_age=2)
    for which in (None, True, custom):
        calls = [0]

        def det(img):
            calls[0] += 1
            b = boxes.copy()
            b[:, :4] += 2 * (calls[0] % 3)   # the crops move, so the keypoints of a person differ from frame to frame
            return b
        model = VitInference(sd, det, model_name='s', dataset='coco', max_batch=8, is_video=True, yolo_step=2, smooth=which)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res[which] = [model.inference(frame.copy()) for _ in range(5)] + model.inference_frames([frame.copy(), frame.copy()])
    assert sum(len(r) for r in res[None]) >= 7
    for which in (True, custom):
        cfg = SmoothCfg() if which is True else which
        twin = OneEuro(17, cfg.min_cutoff, cfg.beta, cfg.d_cutoff, cfg.max_age, 1, cfg.missing)
        changed = 0
        for raw, got in zip(res[None], res[which]):
            ids = list(raw.keys())
            assert list(got.keys()) == ids
            kp = np.stack([raw[i] for i in ids]).astype(np.float32) if ids else np.zeros((0, 17, 3), np.float32)
            want, _ = twin.update(kp, np.array(ids, np.int32))
            for k, i in enumerate(ids):
                assert same_bits(np.asarray(got[i], np.float32), want[k]), (which, i)
            changed += int(not same_bits(want, kp))
        assert changed >= 2
    # without is_video there are no ids: smooth= has no effect
    plain = VitInference(sd, lambda img: boxes.copy(), model_name='s', dataset='coco', max_batch=8, smooth=True)
    base = VitInference(sd, lambda img: boxes.copy(), model_name='s', dataset='coco', max_batch=8)
    for _ in range(2):
        a, b = plain.inference(frame.copy()), base.inference(frame.copy())
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
