"""GPU: the metrics stage on the device (vp_metrics_update / vp_metrics_update_stream, VitPoseHip.metrics) against the host model of the same header
(vp_dbg_metrics_host, pinned on the CPU against its numpy twin, the reference's outputs and literal anchors: tests/test_metrics_host.py).  The state, counts and
fp64 sums alike, and `dist` are compared byte for byte; the OKS goes through the device's exp(): within one float32 step of the tap (the NMS's precedent), its
hits equal (the cases keep every OKS 1e-4 away from a threshold), its sum within oks_rows * 2^-24."""
from __future__ import annotations

import os

import numpy as np
import pytest

from easy_vitpose_amd import VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devmetrics import MetricsCfg, metrics_tap, new_state, parse_state
from easy_vitpose_amd.synth import synthetic_state_dict
import metrics_cases as mc

pytestmark = pytest.mark.gpu
CASES = mc.host_cases()
F32 = np.float32


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def same_state(got, want, tag=''):
    """every word equal but oks_sum, which carries the device's exp(): within oks_rows * 2^-24"""
    for f in want.dtype.names:
        if f == 'oks_sum':
            assert abs(float(got[f]) - float(want[f])) <= int(want['oks_rows']) * 2.0 ** -24, (tag, f)
        else:
            assert got[f].tobytes() == want[f].tobytes(), (tag, f)


def same_oks(got, want, tag=''):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got == -1, want == -1), tag
    if fin.any():
        assert mc.ulp_diff(got[fin], want[fin]).max() <= 1, tag


def to_device(cs):
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in mc.inputs(cs).items()}


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_host_model_on_the_cpu_cases(eng, name):
    cs = CASES[name]
    ev = eng.metrics(cs['cfg'])
    want = new_state(cs['cfg'])
    for _ in range(2):   # the second call accumulates
        dist, oks = ev.update_host(**mc.inputs(cs))
        wd, wo = metrics_tap(want, cs['cfg'], **mc.inputs(cs))
        assert dist.tobytes() == wd.tobytes(), name
        same_oks(oks, wo, name)
    same_state(ev.state(), want, name)
    ev.close()


def test_every_combination_of_null_inputs(eng):
    for name, cs in mc.null_combos().items():
        ev = eng.metrics(cs['cfg'])
        want = new_state(cs['cfg'])
        dist, oks = ev.update_host(**mc.inputs(cs))
        wd, wo = metrics_tap(want, cs['cfg'], **mc.inputs(cs))
        assert dist.tobytes() == wd.tobytes(), name
        same_oks(oks, wo, name)
        same_state(ev.state(), want, name)
        ev.close()


def test_stream_entry_snapshot_reset_and_a_call_without_rows(eng):
    import torch
    cs = CASES['n129']
    cfg = cs['cfg']
    kw = to_device(cs)
    ev = eng.metrics(cfg)
    want = new_state(cfg)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    dist = torch.empty((129, 17), dtype=torch.float32, device='cuda')
    oks = torch.empty((129,), dtype=torch.float32, device='cuda')
    with torch.cuda.stream(side):
        for _ in range(3):
            ev.update(**kw, dist=dist, oks=oks)
        snap = ev.snapshot()
        ev.update(kw['pred'][:0], kw['gt'][:0])
        after = ev.snapshot()
        ev.reset()
        zero = ev.snapshot()
    side.synchronize()
    for _ in range(3):
        wd, wo = metrics_tap(want, cfg, **mc.inputs(cs))
    same_state(parse_state(snap.cpu().numpy(), cfg), want)
    assert dist.cpu().numpy().tobytes() == wd.tobytes()
    same_oks(oks.cpu().numpy(), wo)
    metrics_tap(want, cfg, cs['pred'][:0], cs['gt'][:0])
    assert int(want['calls']) == 4
    same_state(parse_state(after.cpu().numpy(), cfg), want)
    assert not zero.cpu().numpy().any() and ev.state().tobytes() == bytes(ev.nbytes)
    ev.close()


def test_capture_of_update_and_snapshot_replayed_with_new_inputs(eng):
    import torch
    a, b = mc.case(700, 200, 17), mc.case(701, 200, 17)
    cfg = a['cfg']
    kw = to_device(a)
    ev = eng.metrics(cfg)
    snap = torch.zeros((ev.nbytes,), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ev.update(**kw)   # warm-up outside the capture
        ev.reset()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ev.update(**kw)
        ev.snapshot(out=snap)
    want = new_state(cfg)
    for cs in (a, b):
        for k, v in mc.inputs(cs).items():
            if isinstance(v, np.ndarray):
                kw[k].copy_(torch.from_numpy(np.ascontiguousarray(v)).cuda())
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        metrics_tap(want, cfg, **mc.inputs(cs))
        same_state(parse_state(snap.cpu().numpy(), cfg), want)
    assert int(want['calls']) == 2
    ev.close()


def test_8192_rows_of_133_joints_three_times_bit_identical(eng):
    cs = mc.big_case()
    kw = to_device(cs)
    import torch
    states = []
    for _ in range(3):
        ev = eng.metrics(cs['cfg'])
        ev.update(**kw)
        torch.cuda.synchronize()
        states.append(ev.state())
        ev.close()
    assert states[0].tobytes() == states[1].tobytes() == states[2].tobytes()
    assert int(states[0]['rows']) == 8192 and int(states[0]['oks_rows']) > 1000


def test_one_real_forward(eng, golden_dir):
    """eight peaked crops through infer_device, metrics against the fixture's keypoints: the device state equals the tap on the downloaded keypoints, and the
    end-point error sits inside the project's parity bar of half a pixel"""
    import torch
    from cases import peaked_crops
    z = np.load(os.path.join(golden_dir, 'peaked_s_coco.npz'))
    n = int(z['n'])
    assert n == 8
    crops = torch.from_numpy(peaked_crops(n)).cuda()
    gt = np.ascontiguousarray(z['keypoints'], dtype=F32)
    cfg = MetricsCfg(n_joints=17, sigmas='coco')
    norm = np.tile(np.array([[256, 192]], F32), (n, 1))
    area = np.full(n, 256.0 * 192.0, F32)
    ev = eng.metrics(cfg)
    kp = torch.empty((n, 17, 3), dtype=torch.float32, device='cuda')
    eng.infer_device(crops, kp, sync=False)
    ev.update(kp, torch.from_numpy(gt).cuda(), norm=torch.from_numpy(norm).cuda(), area=torch.from_numpy(area).cuda())
    torch.cuda.synchronize()
    want = new_state(cfg)
    metrics_tap(want, cfg, kp.cpu().numpy(), gt, norm=norm, area=area)
    same_state(ev.state(), want)
    r = ev.result()
    print(f'peaked s/coco, 8 crops: EPE {r.epe:.4f} px, NME {r.nme:.5f}, PCK@0.05 {r.pck(0)[1]:.4f}, AUC {r.auc:.4f}, OKS mean {r.oks_mean:.4f}')
    assert r.counted == 8 and r.epe < 0.5
    ev.close()


def test_refusals_come_before_anything_is_enqueued(eng):
    import torch
    cs = CASES['n65']
    ev = eng.metrics(cs['cfg'])
    ev.update_host(**mc.inputs(cs))
    before = ev.state()
    kp = torch.zeros((2, 17, 3), device='cuda')
    for n, pred, msg in ((8193, kp.data_ptr(), 'n = 8193 outside 0..8192'), (-1, kp.data_ptr(), 'n = -1 outside 0..8192'), (2, None, 'null pred or gt with n > 0')):
        rc = eng.lib.vp_metrics_update_stream(ev._m, pred, kp.data_ptr(), None, None, None, None, 0, n, None, None, None)
        assert rc == capi.VP_ERR_INVALID and capi.last_error(eng._h) == 'metrics: ' + msg
    assert eng.lib.vp_metrics_snapshot_stream(ev._m, None, None) == capi.VP_ERR_INVALID
    bad = capi.vp_metrics_cfg(30.0, (np.ctypeslib.ctypes.c_float * 8)(), 0.0, 300, 0, 0, 0, 0)
    h = np.ctypeslib.ctypes.c_void_p()
    assert eng.lib.vp_metrics_create(eng._h, np.ctypeslib.ctypes.byref(bad), None, np.ctypeslib.ctypes.byref(h)) == capi.VP_ERR_INVALID and not h.value
    assert capi.last_error(eng._h) == 'metrics: n_joints = 300 outside 1..256'
    with pytest.raises(TypeError, match='pred'):
        ev.update(np.zeros((2, 17, 3), F32), kp)
    with pytest.raises(ValueError, match='norm'):
        ev.update(kp, kp, norm=torch.zeros((3, 2), device='cuda'))
    torch.cuda.synchronize()
    assert ev.state().tobytes() == before.tobytes()
    ev.close()
