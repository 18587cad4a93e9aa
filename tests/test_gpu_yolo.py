"""GPU: the detector network on the device (vp_yolo_*, devyolo.DeviceYolo, VitInference(yolo=state)) against the float64 oracle of tests/yolo_model.py.

Per launch, through vp_dbg_yolo_activation: every launch of a forward is recomputed in float64 from the fp16 operands the device itself read (the producer's
buffer, the folded weights) and compared element by element.  The weights are random and asymmetric, so an MFMA lane map that is off by a transposition or a
permutation of k fails the bound by orders of magnitude.  Whole network: against the oracle's 'stored' mode within the tolerances of tests/yolo_cases.py, which
come from the oracle alone (tests/golden/yolo_sens.npz)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolo_cases as YC
from easy_vitpose_amd import VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devdetect import DetectCfg, HostDetector
from easy_vitpose_amd.devletterbox import LetterboxCfg
from easy_vitpose_amd.devyolo import DeviceYolo, synth_yolo, yolo_fold, yolo_plan
from easy_vitpose_amd.synth import synthetic_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def run(eng, name, **kw):
    """(DeviceYolo, the head as numpy) of a case"""
    _, _, hw, n, _ = YC.CASES[name]
    y = DeviceYolo(eng, YC.state(name), hw, max_images=n, **kw)
    x = YC.images(name)
    if kw.get('input_layout') == 'nhwc':
        x = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    head = y(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    return y, head.cpu().numpy()


# ------------------------------------------------------------------ per launch
def silu64(v):
    return v / (1 + np.exp(-v))


def check_launches(eng, sd, hw, n, seed):
    """every launch of one forward against float64 on the operands the device read; returns the launches seen as (kind, k, s, h_in, w_in, c_in, c_out, flags).
    The per-element bound of a convolution, term by term: the float32 accumulation of K products, K 2^-24 sum |a w|; the bias add, one float32 rounding of the
    sum, 2^-24 |pre| (the issue's budget leaves it out; it matters where |bias| is large against sum |a w|); both carried through SiLU, slope <= 1.1, plus 4
    float32 ulps for the SiLU itself; the shortcut add, one float32 rounding, 2^-24 |sum|; one rounding of the result to its format."""
    info, launches, bufs = yolo_plan(sd, hw, max_images=n)
    y = DeviceYolo(eng, sd, hw, max_images=n, keep_activations=True)
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 256, (n, 3) + tuple(hw)).astype(np.float32) / np.float32(255)).astype(np.float16)
    y(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    act = {0: x.transpose(0, 2, 3, 1)}   # buffer id -> [n, h, w, c] as the device holds it after the forward
    for i, l in enumerate(launches[:-1]):
        if l['out_buf'] not in act:
            act[l['out_buf']] = y.activation(i, n, bufs[l['out_buf']])
    seen = []
    for i, l in enumerate(launches[:-1]):
        src = act[l['in_buf']][..., l['in_off']:l['in_off'] + l['c_in']]
        got = act[l['out_buf']][..., l['out_off']:l['out_off'] + l['c_out']]
        what = f"launch {i} ({l['kind']}, model.{l['layer']}, {l['k']}x{l['k']} s{l['s']}, {l['h_in']}x{l['w_in']}x{l['c_in']} -> {l['c_out']})"
        if l['kind'] == 'pack':
            want = np.zeros(got.shape, np.float16)
            want[..., :3] = src
            assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), what
        elif l['kind'] == 'pool':
            want = F.max_pool2d(torch.from_numpy(src.astype(np.float32)).permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1).numpy().astype(np.float16)
            assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), what
        elif l['kind'] == 'up':
            want = src.repeat(2, axis=1).repeat(2, axis=2)
            assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), what
        else:
            w, b = yolo_fold(sd, hw, l['conv'])
            k, s = l['k'], l['s']
            wt = torch.from_numpy(w.astype(np.float64).reshape(l['c_out'], k, k, l['c_in'])).permute(0, 3, 1, 2)
            xt = torch.from_numpy(src.astype(np.float64)).permute(0, 3, 1, 2)
            pre = F.conv2d(xt, wt, torch.from_numpy(b.astype(np.float64)), stride=s, padding=k // 2).permute(0, 2, 3, 1).numpy()
            mag = F.conv2d(xt.abs(), wt.abs(), None, stride=s, padding=k // 2).permute(0, 2, 3, 1).numpy()
            K = k * k * l['c_in']
            bound = K * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(pre)
            want = pre
            if l['act']:
                want = silu64(pre)
                bound = 1.1 * bound + 4 * 2.0 ** -23 * np.abs(want)   # SiLU's slope is <= 1.1; 4 float32 ulps for the SiLU itself
            if l['res_buf'] >= 0:
                res = act[l['res_buf']][..., l['res_off']:l['res_off'] + l['c_out']].astype(np.float64)
                want = want + res
                bound = bound + 2.0 ** -24 * np.abs(want)
            if l['f32_out']:
                bound = bound + 2.0 ** -24 * np.abs(want)
            else:
                bound = bound + np.maximum(2.0 ** -11 * np.abs(want), 2.0 ** -25)   # one fp16 rounding of the result (half a subnormal step near zero)
            err = np.abs(got.astype(np.float64) - want)
            bad = ~(err <= bound)   # a NaN (an element nothing wrote: the buffers are pre-filled with 0xFF) fails
            assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} elements outside the bound, first at {np.argwhere(bad)[0]}: got {got[bad][0]}, want {want[bad][0]}'
        flags = ('res',) * (l['res_buf'] >= 0) + ('f32',) * bool(l['f32_out']) + ('in_off',) * (l['in_off'] > 0) + ('out_off',) * (l['out_off'] > 0)
        seen.append((l['kind'], l['k'], l['s'], l['h_in'], l['w_in'], l['c_in'], l['c_out'], flags))
    # every buffer element is written by some launch: nothing of the 0xFF fill is left in the images that ran
    for b_, a in act.items():
        assert not np.isnan(a.astype(np.float32)).any(), f'buffer {b_}: elements nothing wrote'
    y.close()
    return seen


def test_every_launch_against_float64_scale_n_at_32x32(eng):
    """P5 is 1 x 1: 3 x 3 stride 2 on 2 x 2, 3 x 3 stride 1 on 1 x 1 (every tap but the centre is halo), the pools and the copies on one pixel"""
    seen = check_launches(eng, YC.state('n_32x32x1'), (32, 32), 1, 1)
    assert any(k == 'conv' and kk == 3 and s == 2 and (h, w) == (2, 2) for k, kk, s, h, w, _, _, _ in seen)
    assert any(k == 'conv' and kk == 3 and s == 1 and (h, w) == (1, 1) for k, kk, s, h, w, _, _, _ in seen)
    assert any(k == 'conv' and c_in == 8 and kk == 3 for k, kk, s, h, w, c_in, _, _ in seen)   # the stem: 3 channels packed to 8
    assert any(k == 'conv' and 'f32' in f for k, *_, f in seen) and any(k == 'conv' and 'res' in f for k, *_, f in seen)


def test_every_launch_against_float64_scale_n_at_96x160_two_images(eng):
    """3 x 3 stride 2 on 6 x 10; more than one workgroup and a partial last tile; 1 x 1 into a concatenation slice (output offset), 3 x 3 out of one (input offset)"""
    seen = check_launches(eng, YC.state('n_64x96x3'), (96, 160), 2, 2)
    assert any(k == 'conv' and kk == 3 and s == 2 and (h, w) == (6, 10) for k, kk, s, h, w, _, _, _ in seen)
    assert any(k == 'conv' and kk == 1 and 'out_off' in f for k, kk, *_, f in seen)
    assert any(k == 'conv' and kk == 3 and 'in_off' in f for k, kk, *_, f in seen)


def test_every_launch_against_float64_scale_m_nc_91(eng):
    """C_out = 91: the class branch runs on 96 channels (five zero ones) and its last convolution writes 91 float32 channels at an odd stride"""
    seen = check_launches(eng, YC.state('m_64x64x1'), (64, 64), 1, 3)
    assert any(k == 'conv' and c_out == 91 and 'f32' in f for k, _, _, _, _, _, c_out, f in seen)
    assert any(k == 'conv' and c_out == 96 for k, _, _, _, _, _, c_out, _ in seen)


# ------------------------------------------------------------------ the whole network
@pytest.mark.parametrize('name', sorted(YC.CASES))
def test_whole_network_within_the_oracles_sensitivity(eng, name):
    y, head = run(eng, name)
    y.close()
    box, score = YC.deviation(head, YC.oracle_head(name))
    tol_box, tol_score = YC.tolerance(name)
    print(f'{name}: box {box:.4g} px (tolerance {tol_box:.4g}), score {score:.4g} (tolerance {tol_score:.4g})')
    assert np.isfinite(head).all()
    assert box <= tol_box and score <= tol_score


@pytest.mark.parametrize('kw', [dict(input_layout='nhwc'), dict(head_layout=1), dict(head_dtype='fp16'), dict(head_dtype='fp16', head_layout=1)], ids=str)
def test_layouts_and_dtypes_hold_the_same_numbers(eng, kw):
    name = 'n_64x96x3'
    y0, base = run(eng, name)
    y1, head = run(eng, name, **kw)
    y0.close()
    y1.close()
    if kw.get('head_layout') == 1:
        head = head.transpose(0, 2, 1)
    if kw.get('head_dtype') == 'fp16':
        assert head.dtype == np.float16 and np.array_equal(head, base.astype(np.float16))   # the same float32 values, rounded once
    else:
        assert head.dtype == np.float32 and np.array_equal(head.view(np.uint32), base.view(np.uint32))


def test_three_forwards_are_bit_identical_and_images_do_not_mix(eng):
    name = 'n_64x96x3'
    hw, n = YC.CASES[name][2], YC.CASES[name][3]
    y = DeviceYolo(eng, YC.state(name), hw, max_images=n)
    x = torch.from_numpy(YC.images(name)).cuda()
    heads = [y(x).clone() for _ in range(3)]
    assert torch.equal(heads[0], heads[1]) and torch.equal(heads[0], heads[2])
    kept = DeviceYolo(eng, YC.state(name), hw, max_images=n, keep_activations=True)   # the same bits with and without reuse of the buffers' regions
    assert torch.equal(kept(x), heads[0]) and kept.device_bytes > y.device_bytes
    kept.close()
    assert y(x[:0]).shape[0] == 0                         # n_images 0: nothing enqueued
    one = y(x[1:2].contiguous()).clone()                  # below max_images
    assert torch.equal(one[0], heads[0][1])
    y.close()


def test_capture_and_replay_with_new_pixels(eng):
    name = 'n_96x64x2'
    hw, n = YC.CASES[name][2], YC.CASES[name][3]
    y = DeviceYolo(eng, YC.state(name), hw, max_images=n)
    a = torch.from_numpy(YC.images(name)).cuda()
    b = a.flip(0).contiguous()
    want_a, want_b = y(a).clone(), y(b).clone()
    x = a.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        head = y(x)
    x.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(head, want_b)
    x.copy_(a)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(head, want_a)
    y.close()


def test_refusals_come_before_anything_is_enqueued(eng):
    sd = YC.state('n_32x32x1')
    y = DeviceYolo(eng, sd, (32, 32), max_images=2)
    x = torch.zeros((3, 3, 32, 32), dtype=torch.float16, device='cuda')
    with pytest.raises(ValueError, match='n <= 2'):
        y(x)
    with pytest.raises(TypeError, match='fp16'):
        y(x[:1].float())
    before = y._head.clone()
    rc = eng.lib.vp_yolo_forward_stream(y._y, x.data_ptr(), 3, y._head.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == capi.VP_ERR_INVALID and 'n_images = 3 outside 0..2' in capi.last_error(eng._h)
    rc = eng.lib.vp_yolo_forward_stream(y._y, None, 1, y._head.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == capi.VP_ERR_INVALID and 'null input or head' in capi.last_error(eng._h)
    torch.cuda.synchronize()
    assert torch.equal(before, y._head)
    y.close()
    with pytest.raises(capi.VpError, match='multiples of 32'):
        DeviceYolo(eng, sd, (40, 32))
    with pytest.raises(capi.VpError, match='max_images = 65'):
        DeviceYolo(eng, sd, (32, 32), max_images=65)
    broken = dict(sd)
    del broken['model.4.m.1.cv2.bn.bias']
    with pytest.raises(capi.VpError, match='missing tensor model.4.m.1.cv2.bn.bias'):
        DeviceYolo(eng, broken, (32, 32))


def test_host_twin_equals_the_stream_entry(eng):
    name = 'n_32x32x1'
    y, head = run(eng, name)
    got = y.forward_host(YC.images(name))
    y.close()
    assert np.array_equal(got.view(np.uint32), head.view(np.uint32))


# ------------------------------------------------------------------ through the chain
@pytest.mark.parametrize('name', sorted(YC.CHAIN_FRAMES))
def test_letterbox_network_detect_chain_against_the_oracle(eng, name):
    """letterbox -> DeviceYolo -> vp_detect_stream on the case's frame against vp_dbg_detect_host on the oracle's head, at thresholds that sit in gaps of the
    oracle's own values (tests/yolo_cases.py chain_thresholds): the same anchors in the same order, cx, cy, w, h within the tolerance
    scaled by 1 / gain."""
    scale, nc, hw, _, _ = YC.CASES[name]
    conf_thr, iou_thr, k, m_want = YC.chain_thresholds(name)
    tol_box, tol_score = YC.tolerance('chain_' + name)
    cfg = DetectCfg(nc=nc, dtype='fp32', classes=[YC.CHAIN_FRAMES[name][3]], conf_thr=conf_thr, iou_thr=iou_thr, max_images=1)
    tensor_want, table_want = YC.chain_input(name)
    want = HostDetector(cfg).detect(YC.chain_head(name).astype(np.float32), table_want)
    lb, net, det = eng.letterbox(LetterboxCfg(hw)), DeviceYolo(eng, YC.state(name), hw), eng.detector(cfg)
    tensor, table, _ = lb.letterbox([lb.upload(YC.chain_frame(name))])
    head = net(tensor)
    rows, image, anchor, count, flags = det.detect(head, table)
    torch.cuda.synchronize()
    assert np.array_equal(tensor.cpu().numpy().view(np.uint16), tensor_want.view(np.uint16)) and np.array_equal(table, table_want)
    m = int(want[3][-1])
    assert m == m_want >= 1 and int(count.cpu()[-1]) == m and int(flags.cpu()[0]) == 0
    rows, anchor, head = rows.cpu().numpy(), anchor.cpu().numpy(), head.cpu().numpy()
    assert anchor[:m].tolist() == want[2][:m].tolist(), 'other anchors, or another order'
    # cx, cy, w, h of the surviving anchors: the head is in input pixels, a frame pixel is 1 / gain of them, so |d| / gain <= tol_box / gain
    gain = float(table[0, 0])
    err = float(np.abs(head[0, :4, anchor[:m]].astype(np.float64) - YC.chain_head(name)[0, :4, anchor[:m]]).max()) / gain
    print(f'{name}: {m} boxes of {k} candidates, box error {err:.4g} frame px (tolerance {tol_box / gain:.4g})')
    assert err <= tol_box / gain
    assert np.abs(rows[:m, 4] - want[0][:m, 4]).max() <= tol_score
    # ... and the rows are the detector stage's on that head, byte for byte (its own contract: tests/test_gpu_detect.py)
    again = HostDetector(cfg).detect(head, table)
    assert np.array_equal(rows.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(anchor, again[2])
    net.close()
    det.close()


def test_vitinference_builds_the_native_detector_from_a_state_dict(eng):
    """VitInference(yolo=state) is letterbox -> DeviceYolo -> detect with the default configurations: the same dictionary as the explicit wiring"""
    from easy_vitpose_amd import VitInference
    shp = model_shape('s', 'coco')
    pose = synthetic_state_dict(shp, 0, peaked=True)
    sd = synth_yolo('n', 80, 5)
    frame = np.random.default_rng(9).integers(0, 256, (120, 160, 3), dtype=np.uint8)
    a = VitInference(pose, sd, model_name='s', yolo_size=96, dataset='coco', is_video=False)
    got = a.inference(frame)
    b_net = DeviceYolo(a._vit_pose, sd, (96, 96))
    b = VitInference(pose, b_net, model_name='s', yolo_size=96, dataset='coco', is_video=False, letterbox=LetterboxCfg((96, 96)),
                     detect=DetectCfg(nc=80, dtype='fp32', classes='human'))
    want = b.inference(frame)
    assert list(got.keys()) == list(want.keys()) and all(np.array_equal(got[k_], want[k_]) for k_ in got)


# ------------------------------------------------------------------ one launch on views the plan never forms
def conv_case(eng, n, hw, k, s_, act, f32, c_in, in_off, in_stride, c_out, out_off, out_stride, x, w, b, res=None):
    """vp_dbg_yolo_conv_case: x fp16 [n, h, w, in_stride], w fp16 [c_out, k, k, c_in], b float32 [c_out] -> the whole output buffer [n, ho, wo, out_stride]"""
    h, wd = hw
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // s_ + 1, (wd + 2 * pad - k) // s_ + 1
    l = capi.vp_yolo_launch()
    l.kind, l.k, l.s, l.act, l.f32_out = 1, k, s_, act, int(f32)
    l.h_in, l.w_in, l.h_out, l.w_out, l.c_in, l.c_out = h, wd, ho, wo, c_in, c_out
    l.in_off, l.in_stride, l.out_off, l.out_stride = in_off, in_stride, out_off, out_stride
    l.res_buf = -1
    if res is not None:
        l.res_buf, l.res_off, l.res_stride = 0, 0, res.shape[-1]
    out = np.empty((n, ho, wo, out_stride), np.float32 if f32 else np.float16)
    x, w, b = np.ascontiguousarray(x, np.float16), np.ascontiguousarray(w, np.float16), np.ascontiguousarray(b, np.float32)
    capi.check(eng.lib.vp_dbg_yolo_conv_case(eng._h, C.byref(l), n, x.ctypes.data, w.ctypes.data, b.ctypes.data,
                                             None if res is None else np.ascontiguousarray(res, np.float16).ctypes.data, out.ctypes.data), eng._h)
    return out


def conv_ref(x, w, b, k, s_, in_off):
    c_in = w.shape[-1]
    xt = torch.from_numpy(x[..., in_off:in_off + c_in].astype(np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)
    return F.conv2d(xt, wt, torch.from_numpy(b.astype(np.float64)), stride=s_, padding=k // 2).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('k,s_', [(1, 1), (3, 1), (3, 2)])
def test_lane_maps_with_exact_integer_data_and_an_asymmetric_b(eng, k, s_):
    """Small integers, no activation, float32 out: every product and every partial sum is exact in float32, so the result equals the integer convolution on every
    bit.  The weights are a random (asymmetric) integer matrix and every input pixel and channel differs: a swapped or permuted A, B or C lane map, a wrong tap
    order or a wrong channel group changes some output.  3 x 3 x 40 channels = 360 columns: a partial last k step and k steps that straddle taps."""
    rng = np.random.default_rng(10 * k + s_)
    n, hw, c_in, c_out = 2, (5, 7), 40, 52
    x = rng.integers(-4, 5, (n,) + hw + (c_in,)).astype(np.float16)
    w = rng.integers(-3, 4, (c_out, k, k, c_in)).astype(np.float16)
    b = rng.integers(-9, 10, c_out).astype(np.float32)
    got = conv_case(eng, n, hw, k, s_, 0, True, c_in, 0, c_in, c_out, 0, c_out, x, w, b)
    assert np.array_equal(got.astype(np.float64), conv_ref(x, w, b, k, s_, 0))


@pytest.mark.parametrize('f32,c_out,out_off,out_stride', [(False, 24, 8, 48), (True, 21, 3, 29), (False, 21, 2, 27)])
def test_one_by_one_with_an_input_and_an_output_channel_offset(eng, f32, c_out, out_off, out_stride):
    """the one shape of the issue's list no network's plan forms: 1 x 1 reading channels [16, 40) of 56 and writing into the middle of a wider buffer -- on the
    vector store path (offsets in multiples of 4) and on the scalar one; integers again, so exact, and the 0xFF fill outside the written channels is intact"""
    rng = np.random.default_rng(c_out + out_off)
    n, hw, c_in, in_off, in_stride = 3, (6, 10), 24, 16, 56
    x = rng.integers(-4, 5, (n,) + hw + (in_stride,)).astype(np.float16)
    w = rng.integers(-3, 4, (c_out, 1, 1, c_in)).astype(np.float16)
    b = rng.integers(-9, 10, c_out).astype(np.float32)
    got = conv_case(eng, n, hw, 1, 1, 0, f32, c_in, in_off, in_stride, c_out, out_off, out_stride, x, w, b)
    assert np.array_equal(got[..., out_off:out_off + c_out].astype(np.float64), conv_ref(x, w, b, 1, 1, in_off))
    rest = np.delete(got, np.s_[out_off:out_off + c_out], axis=-1)
    assert (rest.view(np.uint32 if f32 else np.uint16) == (0xFFFFFFFF if f32 else 0xFFFF)).all(), 'a channel outside the view was written'


def test_cli_from_a_raw_frame_stack_to_keypoints_with_the_native_detector(tmp_path):
    """python -m easy_vitpose_amd.cli --input clip.npy --synthetic s --yolo synth_n.npz --save-json: letterbox -> DeviceYolo -> detect -> poses, nothing third-party"""
    import json
    from easy_vitpose_amd import cli
    rng = np.random.default_rng(3)
    np.save(tmp_path / 'clip.npy', rng.integers(0, 256, (3, 96, 128, 3), dtype=np.uint8))
    np.savez(tmp_path / 'synth_n.npz', **synth_yolo('n', 80, 5))
    rc = cli.main(['--input', str(tmp_path / 'clip.npy'), '--synthetic', 's', '--dataset', 'coco', '--yolo', str(tmp_path / 'synth_n.npz'), '--det-input', '96', '128',
                   '--det-class', 'cat', '--save-json', '--output-path', str(tmp_path / 'out')])
    assert rc in (0, None)
    files = [p for p in (tmp_path / 'out').rglob('*.json')]
    assert len(files) == 1
    assert 'keypoints' in json.load(open(files[0]))
