"""GPU: the orient stage on the device (vp_orient_stream / vp_orient, VitPoseHip.orient, VitInference(rotate=)) against the host model of csrc/orientgeom.h
(vp_dbg_orient_host, pinned on the CPU against independent models: tests/test_orient_host.py).  A permutation of bytes: every comparison is over every byte of
every parent buffer, the canaries around the planes and in the pitch gaps included.  No test provokes a fault: refusals are checked before anything is enqueued."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from easy_vitpose_amd import Frame, VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devletterbox import image_table
from easy_vitpose_amd.devorient import HostOrient, orient_host_numpy, rotate_code
from easy_vitpose_amd.synth import synthetic_state_dict
from orient_cases import CANARY, T, buffers, content, expected_parents, frames_equal, layout, make_frame, named_cases, out_hw, plane_shapes, same_bits, spec

pytestmark = pytest.mark.gpu
CASES = named_cases()


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def ptr(table):
    return C.cast(table.ctypes.data, C.POINTER(capi.vp_image)) if len(table) else None


def device_plane(shape, mode, offset, fill=None):
    """(parent, view): the layout of orient_cases.host_plane in device memory"""
    import torch
    size, start, strides = layout(shape, mode, offset)
    parent = torch.full((size,), CANARY, dtype=torch.uint8, device='cuda')
    view = torch.as_strided(parent, tuple(shape), strides, start)
    assert view.data_ptr() % 16 == offset
    if fill is not None:
        view.copy_(torch.from_numpy(fill))
    return parent, view


def device_buffers(specs):
    """(source Frames, destination Frames, source parents, destination parents) on the device, laid out as orient_cases.buffers lays them out on the host"""
    src, dst, sp, dp = [], [], [], []
    for s in specs:
        views = []
        for a in content(s):
            parent, view = device_plane(a.shape, s.pitch, s.offset, a)
            sp.append(parent)
            views.append(view)
        src.append(make_frame(s, views))
        views = []
        for shp in plane_shapes(s.fmt, *out_hw(s.h, s.w, s.code)):
            parent, view = device_plane(shp, s.dpitch, s.doffset)
            dp.append(parent)
            views.append(view)
        dst.append(make_frame(s, views))
    return src, dst, sp, dp


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_host_tap_on_the_cases(eng, name):
    """vp_orient and vp_orient_stream (torch's current stream, a side stream) on every case: the destination rows, every byte around and between them, and the
    sources afterwards"""
    import torch
    specs = CASES[name]
    b = buffers(specs)
    want = expected_parents(specs, HostOrient().orient(b.tight, b.codes))
    dev = eng.orient()
    src_before = [p.copy() for p in b.src_parents]
    dev.orient_host(b.src, b.codes, out=b.dst)
    for k, (g, w) in enumerate(zip(b.dst_parents, want)):
        assert same_bits(g, w), f'vp_orient: destination plane {k} or the bytes around it'
    assert all(same_bits(p, q) for p, q in zip(b.src_parents, src_before))
    for stream in (None, torch.cuda.Stream()):
        src, dst, sp, dp = device_buffers(specs)
        sp_before = [p.clone() for p in sp]
        torch.cuda.synchronize()
        if stream is None:
            out = dev.orient(src, b.codes, out=dst)
        else:
            with torch.cuda.stream(stream):
                out = dev.orient(src, b.codes, out=dst)
            stream.synchronize()
        torch.cuda.synchronize()
        assert all(o is d for o, d in zip(out, dst))
        for k, (g, w) in enumerate(zip(dp, want)):
            assert same_bits(g.cpu().numpy(), w), f'vp_orient_stream: destination plane {k} or the bytes around it'
        assert all(torch.equal(p, q) for p, q in zip(sp, sp_before)), 'a source byte changed'
    if specs:   # planes of the stage's own: tight
        fresh = dev.orient(src, b.codes)
        torch.cuda.synchronize()
        assert all(f.pitch[0] == f.planes[0].shape[1] * (3 if f.format != 'nv12' else 1) for f in fresh)
        for f, s, t in zip(fresh, specs, b.tight):
            assert frames_equal(Frame(f.format, tuple(p.cpu().numpy() for p in f.planes), f.matrix), orient_host_numpy(t, s.code))


def test_full_hd_frames_under_the_quarter_turns(eng):
    """one 1080 x 1920 NV12 frame and one RGB frame under each of codes 3, 6 and 8, one call"""
    import torch
    rng = np.random.default_rng(21)
    y, uv, rgb = rng.integers(0, 256, (1080, 1920), dtype=np.uint8), rng.integers(0, 256, (540, 960, 2), dtype=np.uint8), rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    host = [Frame.nv12(y, uv, 'bt709')] * 3 + [Frame.rgb(rgb)] * 3
    codes = [3, 6, 8, 3, 6, 8]
    want = HostOrient().orient(host, codes)
    d_nv, d_rgb = Frame.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), 'bt709'), Frame.rgb(torch.from_numpy(rgb).cuda())
    got = eng.orient().orient([d_nv] * 3 + [d_rgb] * 3, codes)
    torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g.h, g.w) == ((1080, 1920) if codes[k] == 3 else (1920, 1080))
        assert frames_equal(Frame(g.format, tuple(p.cpu().numpy() for p in g.planes), g.matrix), w), f'frame {k} (code {codes[k]})'
    assert same_bits(want[4].planes[0], np.rot90(rgb, -1)) and same_bits(want[5].planes[0], np.rot90(rgb, 1))


def test_back_to_back_calls_and_a_replayed_graph(eng):
    """two calls on one stream with no synchronisation between them (the second turns the first one's output back); the same captured into a graph and replayed
    twice, on changed source bytes the second time"""
    import torch
    specs = [spec('nv12', T + 2, 2 * T + 2, 6, 'p13', 1, seed=31), spec('rgb', T + 1, 5, 8, 'a256', 0, 'p1', 5, seed=32), spec('bgr', 3, T + 1, 2, seed=33)]
    back = [spec(s.fmt, *out_hw(s.h, s.w, s.code), {6: 8, 8: 6, 2: 2}[s.code], s.dpitch, s.doffset, s.pitch, s.offset, seed=s.seed) for s in specs]
    codes, codes_back = np.array([s.code for s in specs], np.int32), np.array([s.code for s in back], np.int32)
    dev = eng.orient()
    src, mid, sp, mp = device_buffers(specs)
    _, again, _, ap = device_buffers(back)
    tight = [make_frame(s, content(s)) for s in specs]
    want_mid = expected_parents(specs, HostOrient().orient(tight, codes))
    want_again = expected_parents(back, tight)

    def check(what):
        for k, (g, w) in enumerate(zip(mp, want_mid)):
            assert same_bits(g.cpu().numpy(), w), f'{what}: first call, plane {k}'
        for k, (g, w) in enumerate(zip(ap, want_again)):
            assert same_bits(g.cpu().numpy(), w), f'{what}: second call, plane {k}'

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dev.orient(src, codes, out=mid)
        dev.orient(mid, codes_back, out=again)
    side.synchronize()
    check('back to back')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.orient(src, codes, out=mid)
        dev.orient(mid, codes_back, out=again)
    for replay in range(2):
        if replay:   # new source bytes: the graph holds pointers, not pixels
            tight = [make_frame(s, [255 - a for a in content(s)]) for s in specs]
            for f, t in zip(src, tight):
                for p, a in zip(f.planes, t.planes):
                    p.copy_(torch.from_numpy(a))
            want_mid = expected_parents(specs, HostOrient().orient(tight, codes))
            want_again = expected_parents(back, tight)
        for parents in (mp, ap):
            for p in parents:
                p.fill_(CANARY)
        graph.replay()
        torch.cuda.synchronize()
        check(f'replay {replay}')
    del graph


def test_the_chain_with_the_later_stages(eng):
    """orient -> letterbox, orient -> infer_boxes and draw_poses on the oriented frames equal the same stages on the host-oriented frames"""
    import torch
    from easy_vitpose_amd.devletterbox import HostLetterbox, LetterboxCfg
    from easy_vitpose_amd.draw import DrawStyle, draw_poses_numpy
    rng = np.random.default_rng(41)
    captured = [Frame.nv12(rng.integers(0, 256, (96, 128), dtype=np.uint8), rng.integers(0, 256, (48, 64, 2), dtype=np.uint8), 'bt709'),
                Frame.rgb(rng.integers(0, 256, (97, 131, 3), dtype=np.uint8))]
    codes = [6, 8]
    upright = [orient_host_numpy(f, c) for f, c in zip(captured, codes)]
    assert [(f.h, f.w) for f in upright] == [(128, 96), (131, 97)]

    def to_device(frames):
        return [Frame(f.format, tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in f.planes), f.matrix) for f in frames]
    side = torch.cuda.Stream()
    d_captured, d_upright = to_device(captured), to_device(upright)
    boxes = torch.tensor([[10, 8, 80, 120, 0.9], [5, 20, 90, 125, 0.8]], dtype=torch.float32, device='cuda')
    fidx = torch.tensor([0, 1], dtype=torch.int32, device='cuda')
    lcfg = LetterboxCfg((48, 40))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):   # nothing but launches between the stages
        turned = eng.orient().orient(d_captured, codes)
        tensor, table, placement = eng.letterbox(lcfg).letterbox(turned)
        kp = eng.infer_boxes(turned, boxes, fidx)
    side.synchronize()
    want_tensor, want_table, want_placement = HostLetterbox(lcfg).letterbox(upright)
    assert same_bits(tensor.cpu().numpy(), want_tensor) and same_bits(table, want_table) and same_bits(placement, want_placement)
    kp_ref = eng.infer_boxes(d_upright, boxes, fidx)
    torch.cuda.synchronize()
    assert same_bits(kp.cpu().numpy(), kp_ref.cpu().numpy()) and np.abs(kp.cpu().numpy()).max() > 0
    pts = np.zeros((2, 17, 3), np.float32)
    pts[..., 0], pts[..., 1], pts[..., 2] = rng.uniform(5, 120, (2, 17)), rng.uniform(5, 90, (2, 17)), 0.9
    style = DrawStyle(conf_thr=0.0)
    eng.draw_poses(turned, torch.from_numpy(pts).cuda(), fidx, style)
    torch.cuda.synchronize()
    drawn = draw_poses_numpy([Frame(f.format, tuple(p.copy() for p in f.planes), f.matrix) for f in upright], pts, np.array([0, 1], np.int32), style)
    for f, (g, w) in enumerate(zip(turned, drawn)):
        assert frames_equal(Frame(g.format, tuple(p.cpu().numpy() for p in g.planes), g.matrix), w), f'frame {f}'
        assert not frames_equal(w, upright[f])


@pytest.mark.parametrize('route', ['pad', 'affine', 'letterbox'])
def test_vitinference_rotate_equals_the_upright_frames(route):
    """VitInference(rotate=90) and (rotate=270) on two frames as captured equal VitInference() on np.rot90 of those frames: every returned dict, the state and
    draw()"""
    import warnings

    import torch
    from cases import frame_case
    from easy_vitpose_amd import VitInference
    from easy_vitpose_amd.devdetect import DetectCfg
    from easy_vitpose_amd.devletterbox import LetterboxCfg
    from helpers import weights
    from test_gpu_detect import people_head
    frame, boxes = frame_case()
    upright = [frame, np.ascontiguousarray(frame[:, ::-1])]
    _, sd, _ = weights('s', 'coco')
    kw = dict(model_name='s', dataset='coco', max_batch=8)
    if route == 'letterbox':
        head = torch.from_numpy(people_head(boxes, frame.shape[:2], (640, 640), A=8400)[0]).cuda()
        yolo, kw = (lambda tensor: head), dict(kw, detect=DetectCfg(classes='human'), letterbox=LetterboxCfg((640, 640)))
    else:
        yolo, kw = (lambda img: boxes.copy()), dict(kw, crop=route)

    def run(model, frames):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = [model.inference(frames[0].copy())] + model.inference_frames([f.copy() for f in frames])
        return res, model.draw(confidence_threshold=0.0), model._tracker_res, model._img

    want, want_pic, want_trk, want_img = run(VitInference(sd, yolo, **kw), upright)
    assert len(want) == 3 and all(len(r) == 3 for r in want) and same_bits(want_img, upright[1])
    for angle in (90, 270):
        captured = [np.ascontiguousarray(np.rot90(f, -(angle // 90))) for f in upright]
        assert captured[0].shape == (640, 480, 3) and same_bits(np.rot90(captured[0], angle // 90), upright[0])
        got, pic, trk, img = run(VitInference(sd, yolo, rotate=angle, **kw), captured)
        for a, b in zip(want, got):
            assert list(a.keys()) == list(b.keys()) and all(same_bits(a[k], b[k]) for k in a), f'rotate={angle}'
        assert same_bits(pic, want_pic) and not same_bits(pic, upright[1]) and same_bits(img, want_img)
        assert same_bits(trk[0], want_trk[0]) and list(trk[1]) == list(want_trk[1]) and trk[2] == want_trk[2]


def test_refusals_that_need_a_device(eng):
    """a host pointer given as a device plane, a plane that runs past its allocation, a frame on another device, and host frames given to the stream entry: each
    refused before anything is enqueued"""
    import types

    import torch
    dev = eng.orient()
    s = spec('rgb', 6, 9, 6)
    b = buffers([s])
    src, dst, sp, dp = device_buffers([s])
    d_src, d_dst, h_src, h_dst = image_table(src), image_table(dst), image_table(b.src), image_table(b.dst)
    codes = np.array([6], np.int32)

    def refused(tab_s, tab_d, match):
        rc = eng.lib.vp_orient_stream(eng._h, ptr(tab_s), codes.ctypes.data, ptr(tab_d), 1, None)
        assert rc == capi.VP_ERR_INVALID and match in capi.last_error(eng._h), capi.last_error(eng._h)

    refused(h_src, d_dst, 'src frame 0 is not device memory')
    refused(d_src, h_dst, 'dst frame 0 is not device memory')
    # a plane whose rows, 128 MiB apart, leave its allocation: the other side lies below it in the same small buffer, so the two ranges stay apart
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device='cuda')
    low, high = buf.data_ptr(), buf.data_ptr() + 2048
    past_s, near_d = d_src.copy(), d_dst.copy()
    past_s['plane'], past_s['pitch'], near_d['plane'] = (high, 0), (1 << 27, 0), (low, 0)
    refused(past_s, near_d, 'src frame 0 is not device memory of device 0 (or runs past the end of its allocation)')
    near_s, past_d = d_src.copy(), d_dst.copy()
    near_s['plane'], past_d['plane'], past_d['pitch'] = (low, 0), (high, 0), (1 << 27, 0)
    refused(near_s, past_d, 'dst frame 0 is not device memory of device 0 (or runs past the end of its allocation)')
    torch.cuda.synchronize()
    assert all((p == CANARY).all() for p in dp) and (buf == CANARY).all(), 'a refused call wrote'
    with pytest.raises(TypeError, match='frame 0: torch uint8 CUDA tensors expected'):
        dev.orient(b.src, 6)
    with pytest.raises(TypeError, match='out 0: torch uint8 CUDA tensors expected'):
        dev.orient(src, 6, out=b.dst)
    with pytest.raises(TypeError, match=r'frame 0: host planes \(numpy arrays\) expected'):
        dev.orient_host(src, 6)
    elsewhere = eng.orient()
    elsewhere.engine = types.SimpleNamespace(device_id=eng.device_id + 1, lib=None, _h=None)   # a handle of another device: refused before the library is reached
    with pytest.raises(ValueError, match=rf'frame 0 lives on cuda:{eng.device_id}, the handle on cuda:{eng.device_id + 1}'):
        elsewhere.orient(src, 6, out=dst)
    with pytest.raises(capi.VpError, match='frame 0 is NV12 of 5 x 6: code 3 reverses an axis of odd length'):
        dev.orient([Frame.nv12(torch.zeros((5, 6), dtype=torch.uint8, device='cuda'), torch.zeros((3, 3, 2), dtype=torch.uint8, device='cuda'))], 3)
    out = dev.orient(src, 6, out=dst)   # and the good call goes through
    torch.cuda.synchronize()
    assert same_bits(out[0].planes[0].cpu().numpy(), np.rot90(content(s)[0], -1))
    assert rotate_code(270) == 6
