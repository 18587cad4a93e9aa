"""GPU: the letterbox stage on the device (vp_letterbox_stream / vp_letterbox, VitPoseHip.letterbox) against the host model of csrc/lbgeom.h (vp_dbg_letterbox_host,
pinned on the CPU against a numpy twin, the C restatement of the resize and integer geometry: tests/test_letterbox_host.py).  The header fixes every operation:
equal means equal bytes -- tensor, undo table, placement."""
from __future__ import annotations

import numpy as np
import pytest

from easy_vitpose_amd import Frame, VitPoseHip
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.cropprep import rgb_to_nv12
from easy_vitpose_amd.devdetect import DetectCfg, letterbox_params
from easy_vitpose_amd.devletterbox import HostLetterbox, LetterboxCfg
from easy_vitpose_amd.devtracker import TrackCfg
from easy_vitpose_amd.synth import synthetic_state_dict
from letterbox_cases import CANARY, named_cases, nv12_frame, rgb_frame, rgb_image, same_bits

pytestmark = pytest.mark.gpu
CASES = named_cases()
MARGIN = 64   # canary elements on either side of an output tensor


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def device_frame(f, parents=None):
    """host Frame -> device Frame with the same pitches, every plane a view into its own canary-filled parent (kept in `parents`)"""
    import torch
    planes = []
    for p, pitch in zip(f.planes, f.pitch):
        rows = p.shape[0]
        parent = torch.full(((rows + 2) * pitch + 16,), CANARY, dtype=torch.uint8, device='cuda')
        inner = (3, 1) if p.ndim == 3 and p.shape[2] == 3 else ((2, 1) if p.ndim == 3 else (1,))
        view = torch.as_strided(parent, tuple(p.shape), (pitch,) + inner, pitch + 5)
        view.copy_(torch.from_numpy(np.ascontiguousarray(p)))
        planes.append(view)
        if parents is not None:
            parents.append((parent, view))
    return Frame(f.format, tuple(planes), f.matrix)


def canary_out(cfg, n, offset=0):
    """(flat canary buffer, the output view `offset` elements behind the margin)"""
    import torch
    dt = {'fp32': torch.float32, 'fp16': torch.float16, 'u8': torch.uint8}[cfg.dtype]
    size = int(np.prod(cfg.shape(n)))
    flat = torch.full((size + 2 * MARGIN,), 7, dtype=dt, device='cuda')
    view = flat[MARGIN + offset:MARGIN + offset + size].view(cfg.shape(n))
    return flat, view


def check_stream(dev, cfg, d_frames, want, offset=0, stream=None):
    import torch
    flat, view = canary_out(cfg, len(d_frames), offset)
    if offset and view.numel():   # (an empty tensor has no address)
        assert view.data_ptr() % 16 != 0
    torch.cuda.synchronize()
    if stream is None:
        out, det, placement = dev.letterbox(d_frames, out=view)
    else:
        with torch.cuda.stream(stream):
            out, det, placement = dev.letterbox(d_frames, out=view)
        stream.synchronize()
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    got = flat.cpu().numpy()
    lo, size = MARGIN + offset, want[0].size
    assert same_bits(got[lo:lo + size].reshape(want[0].shape), want[0]), f'tensor differs (offset {offset})'
    assert (got[:lo] == 7).all() and (got[lo + size:] == 7).all(), 'a byte outside [n, 3, H, W] changed'
    assert same_bits(det, want[1]) and same_bits(placement, want[2])


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_host_tap_on_the_cases(eng, name):
    """vp_letterbox and vp_letterbox_stream (default stream, a side stream, and an output one element into its buffer: the element-store path) on every case"""
    import torch
    cfg, frames = CASES[name]
    want = HostLetterbox(cfg).letterbox(frames)
    dev = eng.letterbox(cfg)
    got = dev.letterbox_host(frames)
    for what, g, w in zip(('tensor', 'table', 'placement'), got, want):
        assert same_bits(g, w), f'vp_letterbox: {what} differs'
    parents = []
    d_frames = [device_frame(f, parents) for f in frames]
    check_stream(dev, cfg, d_frames, want)
    check_stream(dev, cfg, d_frames, want, stream=torch.cuda.Stream())
    check_stream(dev, cfg, d_frames, want, offset=1)
    for parent, view in parents:   # read-only: the frames and the canaries around them are as they were
        assert (parent == CANARY).sum().item() >= parent.numel() - view.numel()


def test_pitched_device_views_equal_their_contiguous_copies(eng):
    import torch
    cfg, frames = CASES['pitched']
    dev = eng.letterbox(cfg)
    d_pitched = [device_frame(f) for f in frames]
    d_dense = [Frame(f.format, tuple(p.contiguous() for p in f.planes), f.matrix) for f in d_pitched]
    assert all(a.pitch[0] > b.pitch[0] for a, b in zip(d_pitched, d_dense))
    a, b = dev.letterbox(d_pitched)[0], dev.letterbox(d_dense)[0]
    torch.cuda.synchronize()
    assert same_bits(a.cpu().numpy(), b.cpu().numpy()) and same_bits(a.cpu().numpy(), HostLetterbox(cfg).letterbox(frames)[0])
    # a frame that runs past its allocation, and one in host memory, are refused before anything is enqueued
    import ctypes as C
    from easy_vitpose_amd import _capi as capi
    from easy_vitpose_amd.devletterbox import c_config, image_table
    big = c_config(LetterboxCfg((8192, 8192), dtype='u8'))
    out = torch.zeros(16, dtype=torch.uint8, device='cuda')
    past = image_table([d_dense[0]])
    past['h'], past['w'], past['pitch'] = 65536, 4096, (3 * 4096, 0)   # 805 MB behind a pointer into a few hundred bytes
    on_host = image_table([frames[0]])
    for tab in (past, on_host):
        rc = eng.lib.vp_letterbox_stream(eng._h, C.byref(big), C.cast(tab.ctypes.data, C.POINTER(capi.vp_image)), 1, out.data_ptr(), None, None, None)
        assert rc == capi.VP_ERR_INVALID and 'frame 0 is not device memory' in capi.last_error(eng._h)
    torch.cuda.synchronize()
    assert (out == 0).all()


def test_back_to_back_calls_and_a_replayed_graph_give_identical_bytes(eng):
    """two calls on one stream into two buffers, one synchronise; the same captured into a torch graph and replayed twice.  The handle is the fixture's: it keeps
    the default queue count."""
    import torch
    cfg = LetterboxCfg((48, 40))
    frames = [nv12_frame(33, 21, 1), rgb_frame(64, 80, 2, extra=4), nv12_frame(96, 80, 3, 'bt709')]
    want = HostLetterbox(cfg).letterbox(frames)[0]
    dev = eng.letterbox(cfg)
    d_frames = [device_frame(f) for f in frames]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        first = dev.letterbox(d_frames)[0]
        second = dev.letterbox(d_frames)[0]
    side.synchronize()
    assert same_bits(first.cpu().numpy(), want) and same_bits(second.cpu().numpy(), want)
    bufs = [torch.empty(cfg.shape(3), dtype=torch.float16, device='cuda') for _ in range(2)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for b in bufs:
            dev.letterbox(d_frames, out=b)
    for replay in range(2):
        for b in bufs:
            b.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        for b in bufs:
            assert same_bits(b.cpu().numpy(), want), f'replay {replay}'
    del graph


def test_one_production_shape_against_the_host_tap(eng):
    """4 NV12 1080p frames into 640 x 640 fp16 NCHW"""
    import torch
    cfg = LetterboxCfg((640, 640))
    rng = np.random.default_rng(11)
    small = rgb_image(135, 240, 5)
    frames = []
    for i in range(4):
        rgb = np.repeat(np.repeat(small, 8, 0), 8, 1)
        rgb = (rgb.astype(np.int32) + rng.integers(-20, 20, rgb.shape)).clip(0, 255).astype(np.uint8)
        frames.append(Frame.nv12(*rgb_to_nv12(rgb, 'bt709'), 'bt709'))
    want = HostLetterbox(cfg).letterbox(frames)
    d_frames = [Frame.nv12(torch.from_numpy(f.planes[0]).cuda(), torch.from_numpy(f.planes[1]).cuda(), 'bt709') for f in frames]
    out, det, placement = eng.letterbox(cfg).letterbox(d_frames)
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), want[0]) and same_bits(det, want[1]) and same_bits(placement, want[2])
    assert placement.tolist() == [[0, 140, 640, 360]] * 4 and det[0].tolist() == [np.float32(1 / 3), 0.0, 140.0, 1920.0, 1080.0]


def test_the_chain_from_the_frame_to_the_poses_with_no_host_copy(eng):
    """letterbox -> a "network" that is a fixed device head tensor -> detect(table) -> counted tracker -> infer_boxes on one side stream with one synchronisation;
    the same rows as the chain whose detector stage is fed by letterbox_params"""
    import torch
    from test_gpu_detect import people_head
    rng = np.random.default_rng(8)
    rgb = [rng.integers(0, 256, (97, 131, 3), dtype=np.uint8) for _ in range(3)]
    boxes = [np.array([[10, 8, 60, 90, 0.9], [70, 12, 125, 93, 0.8]], np.float32), np.array([[30, 5, 100, 88, 0.7]], np.float32), np.zeros((0, 5), np.float32)]
    lcfg, dcfg, tcfg = LetterboxCfg((160, 224)), DetectCfg(classes='human'), TrackCfg(1, 1, 0.3, 3)
    d_head = torch.from_numpy(np.concatenate([people_head(b, (97, 131), (160, 224)) for b in boxes])).cuda()
    lb, det = eng.letterbox(lcfg), eng.detector(dcfg)
    seen = {}

    def network(tensor):   # kernel-free: the head is there already
        seen['shape'], seen['dtype'], seen['cuda'] = tuple(tensor.shape), tensor.dtype, tensor.is_cuda
        return d_head

    def chain(with_letterbox):
        trk = eng.tracker(tcfg)
        fr = [Frame.rgb(torch.from_numpy(f).cuda()) for f in rgb]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            if with_letterbox:
                tensor, table, placement = lb.letterbox(fr)
                rows, image, anchor, count, flags = det.detect(network(tensor), table, n_out=8)
            else:
                rows, image, anchor, count, flags = det.detect(d_head, (97, 131), (160, 224), 8)
            trows, ids, stream, tcount, tflags = trk.update(rows, image, n_out=8, n_dets=count[-1:])
            out = eng.infer_boxes(fr, trows, stream)
        side.synchronize()
        res = [t.cpu().numpy() for t in (rows, image, anchor, count, flags, trows, ids, stream, tcount, tflags, out)]
        trk.close()
        return res

    a, b = chain(True), chain(False)
    det.close()
    assert seen == {'shape': (3, 3, 160, 224), 'dtype': torch.float16, 'cuda': True}
    for k, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x, y), f'output {k}'
    assert a[3].tolist() == [2, 1, 0, 3] and np.abs(a[10][:3]).max() > 0
    g = letterbox_params((97, 131), (160, 224))
    assert same_bits(lb.letterbox([Frame.rgb(torch.from_numpy(rgb[0]).cuda())])[1][0], np.array(g + (131, 97), np.float32))


def test_vitinference_with_the_letterbox_stage_equals_the_detector_stage_alone():
    """VitInference(detect=, letterbox=): the engine callable gets the letterboxed device tensor and returns the head, left on the device or as an ndarray; the
    results are those of VitInference(detect=) fed the same head with the sizes"""
    import warnings

    import torch
    from cases import frame_case
    from easy_vitpose_amd import VitInference
    from helpers import weights
    from test_gpu_detect import people_head
    frame, boxes = frame_case()
    _, sd, _ = weights('s', 'coco')
    head = people_head(boxes, frame.shape[:2], (640, 640), A=8400)[0]
    cfg, lcfg = DetectCfg(classes='human'), LetterboxCfg((640, 640))
    want_tensor = HostLetterbox(lcfg).letterbox([Frame.rgb(np.ascontiguousarray(frame))])[0]
    seen = []

    def device_engine(tensor):
        seen.append(tensor)
        return torch.from_numpy(head).cuda()

    def host_engine(tensor):
        seen.append(tensor)
        return head
    res = {}
    for which, yolo, kw in (('sizes', lambda img: (head, (640, 640)), {}), ('device head', device_engine, dict(letterbox=lcfg)), ('host head', host_engine, dict(letterbox=lcfg))):
        model = VitInference(sd, yolo, model_name='s', dataset='coco', max_batch=8, detect=cfg, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res[which] = [model.inference(frame.copy())] + model.inference_frames([frame.copy(), frame.copy()])
    assert len(seen) == 6 and all(t.is_cuda and tuple(t.shape) == (1, 3, 640, 640) and t.dtype == torch.float16 for t in seen)
    assert same_bits(seen[0].cpu().numpy(), want_tensor)
    assert all(len(r) == 3 for r in res['sizes'])
    for which in ('device head', 'host head'):
        for a, b in zip(res['sizes'], res[which]):
            assert list(a.keys()) == list(b.keys()) and all(np.array_equal(a[k], b[k]) for k in a), which


def test_refusals_of_the_python_layer_that_need_a_device_tensor(eng):
    """each by its message, each before anything is enqueued; the table of a refused C call stays as it was"""
    import types

    import torch
    cfg = LetterboxCfg((16, 16))
    dev = eng.letterbox(cfg)
    d_frame = Frame.rgb(torch.zeros((8, 12, 3), dtype=torch.uint8, device='cuda'))
    h_frame = rgb_frame(8, 12, 1)
    with pytest.raises(TypeError, match='frame 1: torch uint8 CUDA tensors expected'):
        dev.letterbox([d_frame, h_frame])
    with pytest.raises(TypeError, match=r'frame 1: host planes \(numpy arrays\) expected'):
        dev.letterbox_host([h_frame, d_frame])
    with pytest.raises(TypeError, match=r'frame 0: host planes \(numpy arrays\) expected'):
        HostLetterbox(cfg).letterbox([d_frame])
    elsewhere = eng.letterbox(cfg)
    elsewhere.engine = types.SimpleNamespace(device_id=eng.device_id + 1, lib=None, _h=None)   # a handle of another device: refused before the library is reached
    with pytest.raises(ValueError, match=rf'frame 0 lives on cuda:{eng.device_id}, the handle on cuda:{eng.device_id + 1}'):
        elsewhere.letterbox([d_frame])
    for bad in (np.zeros(cfg.shape(1), np.float16), torch.zeros(cfg.shape(1), dtype=torch.float16), torch.zeros(cfg.shape(1), dtype=torch.float32, device='cuda')):
        with pytest.raises(TypeError, match='out: a fp16 torch CUDA tensor expected'):
            dev.letterbox([d_frame], out=bad)
    wide = torch.zeros((1, 3, 16, 32), dtype=torch.float16, device='cuda')
    for bad in (torch.zeros(cfg.shape(2), dtype=torch.float16, device='cuda'), wide[..., ::2], wide[..., :16]):
        with pytest.raises(ValueError, match=r'out: a contiguous tensor of shape \(1, 3, 16, 16\) on cuda:'):
            dev.letterbox([d_frame], out=bad)
    torch.cuda.synchronize()
    assert (wide == 0).all()
    out, det, placement = dev.letterbox([d_frame])
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), HostLetterbox(cfg).letterbox([Frame.rgb(np.zeros((8, 12, 3), np.uint8))])[0])
