"""The detector network (vp_yolo_*, csrc/yologeom.h), everything of it that runs without a GPU: the exported surface, the plan against a literal table of the five
scales, the load step against the oracle's own fold on every bit, the decode against float64, the extent walk over every launch of every scale, the refusals by
message, the committed tolerances and the gaps the chain cases need."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import yolo_cases as YC
import yolo_model as M
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.devyolo import load_yolo_state, synth_yolo, yolo_decode_host, yolo_fold, yolo_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['vp_yolo_create', 'vp_yolo_destroy', 'vp_yolo_info', 'vp_yolo_forward_stream', 'vp_yolo_forward', 'vp_dbg_yolo_plan', 'vp_dbg_yolo_fold',
       'vp_dbg_yolo_decode_host', 'vp_dbg_yolo_activation', 'vp_dbg_yolo_conv_case']
# scale: (ch64, ch128, ch256, ch512, ch1024, d(3), d(6), Detect c2, Detect c3 at nc = 80), by hand from chX = 8 ceil(min(X, max_ch) width / 8), d(n) = max(round(n depth), 1)
TABLE = {'n': (16, 32, 64, 128, 256, 1, 2, 64, 80), 's': (32, 64, 128, 256, 512, 1, 2, 64, 128), 'm': (48, 96, 192, 384, 576, 2, 4, 64, 192),
         'l': (64, 128, 256, 512, 512, 3, 6, 64, 256), 'x': (80, 160, 320, 640, 640, 3, 6, 80, 320)}


@pytest.fixture(scope='module')
def states():
    return {s: synth_yolo(s, 80, 3) for s in TABLE}


def test_surface():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    assert '#define VP_HAS_YOLO 1' in hdr and lib.vp_abi_version() == 4
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes and re.search(r'VP_API int %s\(' % name, hdr), name
    assert C.sizeof(capi.vp_yolo_cfg) == 32 and C.sizeof(capi.vp_yolo_launch) == 96 and C.sizeof(capi.vp_yolo_buffer) == 16 and C.sizeof(capi.vp_yolo_tensor) == 48


@pytest.mark.parametrize('scale', sorted(TABLE))
def test_plan_against_the_literal_table(states, scale):
    info, launches, bufs = yolo_plan(states[scale], (640, 640))
    t = TABLE[scale]
    assert (info['ch64'], info['ch128'], info['ch256'], info['ch512'], info['ch1024'], info['d3'], info['d6'], info['det_c2'], info['det_c3']) == t
    assert info['scale'] == scale and info['nc'] == 80 and info['A'] == 8400
    d3, d6 = t[5], t[6]
    # convolutions: 2 + five stride-2 Convs, (2 + 2 n) per C2f, 2 in SPPF, 18 in Detect
    n_conv = 7 + sum(2 + 2 * n for n in (d3, d6, d6, d3, d3, d3, d3, d3)) + 2 + 18
    assert info['n_convs'] == n_conv == sum(l['kind'] == 'conv' for l in launches)
    kinds = [l['kind'] for l in launches]
    assert kinds[0] == 'pack' and kinds[-1] == 'decode' and kinds.count('pool') == 3 and kinds.count('up') == 2 and len(launches) == n_conv + 7
    # the three levels the decode reads: strides 8, 16, 32
    lv = launches[-1]['in_buf']
    assert [(bufs[lv + i]['h'], bufs[lv + i]['w'], bufs[lv + i]['c'], bufs[lv + i]['elem_bytes']) for i in range(3)] == [(80, 80, 144, 4), (40, 40, 144, 4), (20, 20, 144, 4)]
    # layer 0 .. 9 of the backbone: (layer, c_out of its last convolution, output side)
    last = {}
    for l in launches:
        if l['kind'] == 'conv':
            last[l['layer']] = (l['c_out'], l['h_out'])
    assert [last[i] for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 18, 19, 21)] == [
        (t[0], 320), (t[1], 160), (t[1], 160), (t[2], 80), (t[2], 80), (t[3], 40), (t[3], 40), (t[4], 20), (t[4], 20), (t[4], 20), (t[3], 40), (t[2], 80), (t[2], 40),
        (t[3], 40), (t[3], 20), (t[4], 20)]


def test_nc_shapes_the_class_branch():
    for nc, c3, c3_pad in ((1, 64, 64), (91, 91, 96), (100, 100, 104), (256, 100, 104)):
        info, launches, bufs = yolo_plan(synth_yolo('n', nc, 0), (32, 32))
        assert info['nc'] == nc and info['det_c3'] == c3
        cls = [l for l in launches if l['kind'] == 'conv' and l['f32_out'] and l['c_out'] == nc and l['out_off'] == 64]
        assert len(cls) == 3 and all(l['c_in'] == c3_pad and l['out_stride'] == 64 + nc for l in cls)


def test_fold_equals_the_oracles_fold_on_every_bit_and_a_fused_checkpoint_agrees():
    sd = synth_yolo('s', 91, 4)
    fused = M.fuse(sd)
    assert not any('.bn.' in k for k in fused)
    info, launches, _ = yolo_plan(sd, (32, 32))
    assert yolo_plan(fused, (32, 32))[1] == launches
    convs = [l for l in launches if l['kind'] == 'conv']
    order = M.conv_order(sd)
    assert len(order) == len(convs) == info['n_convs']
    twice = 0
    for i, (key, module) in enumerate(order):
        w, b = yolo_fold(sd, (32, 32), i)
        w_o, b_o = M.fold_image(sd, key, module, convs[i]['c_in'], convs[i]['c_out'])
        assert w.shape == w_o.shape and np.array_equal(w.view(np.uint16), w_o.view(np.uint16)), key
        assert np.array_equal(b.view(np.uint32), b_o.view(np.uint32)), key
        wf, bf = yolo_fold(fused, (32, 32), i)
        wf_o, bf_o = M.fold_image(fused, key, module, convs[i]['c_in'], convs[i]['c_out'])
        assert np.array_equal(wf.view(np.uint16), wf_o.view(np.uint16)) and np.array_equal(bf.view(np.uint32), bf_o.view(np.uint32)), key
        # a fused checkpoint holds float32(w'): the same fp16 weight except where that extra rounding crosses an fp16 tie, never more than one fp16 step, and
        # exactly where the oracle's own fold of the fused file says so (checked above); the biases are the same float32 numbers
        assert np.array_equal(bf.view(np.uint32), b.view(np.uint32)), key
        diff = wf.view(np.uint16) != w.view(np.uint16)
        twice += int(diff.sum())
        assert (np.abs(wf.view(np.int16).astype(np.int32) - w.view(np.int16).astype(np.int32))[diff] == 1).all(), key
    total = sum(l['c_out'] * l['k'] ** 2 * l['c_in'] for l in convs)
    assert twice <= total * 2.0 ** -10, f'{twice} of {total} weights differ between the fused and the unfused checkpoint'


def test_decode_host_against_float64():
    """vp_dbg_yolo_decode_host against the float64 decode on the same float32 logits: boxes within 64 float32 ulps of max(|value|, stride), scores within 8 ulps.
    The budget is that of a 16-term float32 softmax plus a division: 16 exponentials of up to 2 ulps whose arguments carry half an ulp of |z - m| <= 40 or so,
    two 16-term sums, the quotient, one subtraction and addition against the anchor, the mean and the product with the stride."""
    rng = np.random.default_rng(5)
    nc, hw, n = 7, (64, 96), 2
    levels = []
    for i in range(3):
        h, w = hw[0] >> (3 + i), hw[1] >> (3 + i)
        z = rng.standard_normal((n, h, w, 64 + nc)).astype(np.float32) * np.float32(4)
        z[0, 0, 0, :16] = 0            # a flat distribution
        z[0, 0, 0, 16:32] = -30
        z[0, 0, 0, 31] = 30            # all the mass in the last bin
        z[0, 0, 0, 32:48] = np.arange(16) * 5   # steep
        z[0, 0, 0, 64:] = np.linspace(-80, 80, nc)   # scores at both ends
        levels.append(z)
    want = M.decode([__import__('torch').from_numpy(l.astype(np.float64)).permute(0, 3, 1, 2) for l in levels])
    for layout in (0, 1):
        got = yolo_decode_host(levels, nc, hw, 'fp32', layout)
        got = got if layout == 0 else got.transpose(0, 2, 1)
        A0 = [0, 8 * 12, 8 * 12 + 4 * 6, 8 * 12 + 4 * 6 + 2 * 3]
        for i in range(3):
            sl = slice(A0[i], A0[i + 1])
            ref = np.maximum(np.abs(want[:, :4, sl]), 8 << i)
            ulps = np.abs(got[:, :4, sl] - want[:, :4, sl]) / (ref * 2.0 ** -23)
            assert ulps.max() <= 64, (layout, i, ulps.max())
        s_ulps = np.abs(got[:, 4:] - want[:, 4:]) / np.maximum(np.abs(want[:, 4:]) * 2.0 ** -23, 2.0 ** -149)
        assert s_ulps.max() <= 8, (layout, s_ulps.max())
    half = yolo_decode_host(levels, nc, hw, 'fp16', 0)
    with np.errstate(over='ignore'):
        assert np.array_equal(half, yolo_decode_host(levels, nc, hw, 'fp32', 0).astype(np.float16))


def walk(launches, bufs, n_images):
    """every address the plan's launches can form lies inside its buffer; slices tile their buffer without overlap; nothing is read before it is written"""
    written = {0: [(0, bufs[0]['c'])]}   # buffer -> channel ranges written so far (every launch writes all pixels of its range)
    for i, l in enumerate(launches):
        bi, bo = bufs[l['in_buf']], bufs[l['out_buf']]
        what = (i, l)
        if l['kind'] == 'decode':
            for q in range(3):
                b = bufs[l['in_buf'] + q]
                assert b['c'] == l['c_in'] == l['in_stride'] and b['elem_bytes'] == 4 and sorted(written[l['in_buf'] + q]) == [(0, 64), (64, b['c'])], what
            assert (bo['h'], bo['w'], bo['c']) == (1, sum(bufs[l['in_buf'] + q]['h'] * bufs[l['in_buf'] + q]['w'] for q in range(3)), l['c_out']), what
            continue
        assert l['in_stride'] == bi['c'] and l['out_stride'] == bo['c'] and (l['h_in'], l['w_in']) == (bi['h'], bi['w']) and (l['h_out'], l['w_out']) == (bo['h'], bo['w']), what
        # the highest element of the last pixel, by the address rule pixel * stride + off + c, against the extent
        for b, off, c, st in ((bi, l['in_off'], l['c_in'], l['in_stride']), (bo, l['out_off'], l['c_out'], l['out_stride'])):
            pixels = n_images * b['h'] * b['w']
            assert 0 <= off and off + c <= st and (pixels - 1) * st + off + c <= pixels * b['c'], what
        if l['kind'] != 'pack':
            assert l['c_in'] % 8 == 0 and l['in_off'] % 8 == 0 and l['in_stride'] % 8 == 0 and bi['elem_bytes'] == 2, what   # 16-byte loads
        if l['kind'] == 'conv':
            pad = l['k'] // 2
            assert l['k'] in (1, 3) and l['s'] in (1, 2) and l['h_out'] == (l['h_in'] + 2 * pad - l['k']) // l['s'] + 1 and l['w_out'] == (l['w_in'] + 2 * pad - l['k']) // l['s'] + 1, what
            assert bo['elem_bytes'] == (4 if l['f32_out'] else 2), what
            if l['res_buf'] >= 0:
                br = bufs[l['res_buf']]
                assert (br['h'], br['w']) == (l['h_out'], l['w_out']) and l['res_off'] + l['c_out'] <= br['c'] == l['res_stride'], what
                assert any(a <= l['res_off'] and l['res_off'] + l['c_out'] <= e for a, e in written[l['res_buf']]), what
        elif l['kind'] == 'pool':
            assert l['in_buf'] == l['out_buf'] and l['c_in'] == l['c_out'] and l['in_off'] + l['c_in'] <= l['out_off'], what
        elif l['kind'] == 'up':
            assert (l['h_out'], l['w_out']) == (2 * l['h_in'], 2 * l['w_in']) and l['c_in'] == l['c_out'], what
        # read after write: the input range is covered by what earlier launches wrote
        cover = np.zeros(bi['c'], bool)
        for a, e in written.get(l['in_buf'], []):
            cover[a:e] = True
        assert cover[l['in_off']:l['in_off'] + l['c_in']].all(), ('read before written', what)
        # written once: the output range overlaps nothing written before
        for a, e in written.get(l['out_buf'], []):
            assert e <= l['out_off'] or l['out_off'] + l['c_out'] <= a, ('written twice', what)
        written.setdefault(l['out_buf'], []).append((l['out_off'], l['out_off'] + l['c_out']))
    for b, ranges in written.items():   # the slices tile their buffer
        ranges = sorted(ranges)
        assert ranges[0][0] == 0 and ranges[-1][1] == bufs[b]['c'] and all(x[1] == y[0] for x, y in zip(ranges, ranges[1:])), (b, ranges)
    assert sorted(written) == list(range(len(bufs) - 1))   # every buffer but the head (the decode's) is written through a launch or is the input


@pytest.mark.parametrize('scale', sorted(TABLE))
def test_extent_walk(states, scale):
    for hw in ((32, 32), (64, 96), (640, 640), (1280, 1280)):
        info, launches, bufs = yolo_plan(states[scale], hw, max_images=64)
        for n in (1, 64):
            walk(launches, bufs, n)
            # element indices stay below 2^63 and every buffer of 64 images below 2^40 bytes: the kernels index with size_t
            assert max(64 * b['h'] * b['w'] * b['c'] * b['elem_bytes'] for b in bufs) < 2 ** 40


def test_refusals_by_message(tmp_path):
    sd = synth_yolo('n', 80, 0)

    def refused(state, hw=(64, 64), **kw):
        with pytest.raises(capi.VpError) as e:
            yolo_plan(state, hw, **kw)
        return e.value.msg
    assert 'multiples of 32' in refused(sd, (64, 72)) and 'multiples of 32' in refused(sd, (1312, 64)) and 'multiples of 32' in refused(sd, (0, 64))
    assert 'max_images = 0 outside 1..64' in refused(sd, max_images=0)
    assert 'head_layout = 2' in refused(sd, head_layout=2)
    big = dict(sd)
    big['model.22.cv3.0.2.weight'] = np.zeros((257, 100, 1, 1), np.float32)
    assert 'nc = 257 outside 1..256' in refused(big)
    miss = {k: v for k, v in sd.items() if k != 'model.9.cv2.bn.running_var'}
    assert 'missing tensor model.9.cv2.bn.running_var' in refused(miss)
    assert 'missing tensor model.0.conv.weight' in refused({k: v for k, v in sd.items() if k != 'model.0.conv.weight'})
    wrong = dict(sd)
    wrong['model.3.conv.weight'] = np.zeros((64, 32, 1, 1), np.float32)
    assert 'model.3.conv.weight: shape [64, 32, 1, 1] contradicts [64, 32, 3, 3]' in refused(wrong)
    odd = dict(sd)
    odd['model.0.conv.weight'] = np.zeros((24, 3, 3, 3), np.float32)
    assert 'the width of no YOLOv8 scale' in refused(odd)
    deep = dict(sd)
    for k in list(sd):
        if k.startswith('model.2.m.0.'):
            deep[k.replace('.m.0.', '.m.1.')] = sd[k]
    assert 'model.2: 2 Bottlenecks in the checkpoint, scale n has 1' in refused(deep)
    dfl = dict(sd)
    dfl['model.22.dfl.conv.weight'] = np.arange(16, dtype=np.float32)[::-1].reshape(1, 16, 1, 1).copy()
    assert 'model.22.dfl.conv.weight is not 0..15' in refused(dfl)
    # an ultralytics pickle (a whole model object, not a state dict) is refused with the exporter's name; a plain state dict .pt and an .npz load
    import pickle
    import torch
    p = tmp_path / 'yolov8n.pt'
    with open(p, 'wb') as f:
        pickle.dump({'model': walk, 'train_args': {}}, f)   # a pickled global, as an ultralytics checkpoint's DetectionModel is
    with pytest.raises(ValueError, match='tools/export_yolo_state.py'):
        load_yolo_state(p)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, tmp_path / 'plain.pt')
    np.savez(tmp_path / 'plain.npz', **sd)
    for name in ('plain.pt', 'plain.npz'):
        back = load_yolo_state(tmp_path / name)
        assert set(back) == set(sd) and all(np.array_equal(back[k], sd[k]) for k in sd)


def test_committed_tolerances_are_the_oracles_and_every_chain_case_has_its_gaps():
    """tests/golden/yolo_sens.npz holds what `python tests/yolo_cases.py` computes from the oracle alone; every entry is recomputed here.
    'stored' against 'exact' is the precision cost of fp16 activations: a result (profiles/yolo_net.txt), not a gate."""
    assert set(YC.golden_sens()) == set(YC.CASES) | {'chain_' + c for c in YC.CASES} and set(YC.CHAIN_FRAMES) == set(YC.CASES)
    again = YC.compute_sens()
    for key, v in YC.golden_sens().items():
        assert np.allclose(again[key], v, rtol=1e-9, atol=0), key
    for case, (_, _, _, _, seed) in YC.CASES.items():
        assert YC.golden_sens()[case][2] == seed
    for case in YC.CHAIN_FRAMES:
        assert YC.golden_sens()['chain_' + case][2] == YC.CASES[case][4]
        conf_thr, iou_thr, k, m = YC.chain_thresholds(case)
        assert 5 <= k <= 200 and 1 <= m <= k and 0 < conf_thr < 1 and 0 < iou_thr < 1


@pytest.mark.skipif(shutil.which('g++') is None and shutil.which('clang++') is None, reason='no host C++ compiler')
def test_host_code_under_the_sanitizers(tmp_path):
    """tools/yolo_host_asan.cpp: plan, fold and decode of csrc/yologeom.h on blocks of exact size under -fsanitize=address,undefined; a stand-alone program"""
    cxx = shutil.which('g++') or shutil.which('clang++')
    exe = str(tmp_path / 'yolo_host_asan')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'yolo_host_asan.cpp'), '-o', exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and 'yolo host ok' in r.stdout, r.stdout + r.stderr
