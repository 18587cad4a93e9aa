"""GPU: NV12, BGR and pitched frames on the frames and boxes entries (vp_image: vp_infer_images, vp_infer_boxes_images_stream, vp_dbg_crop_prep_image;
VitPoseHip.infer_frames / infer_boxes on Frame objects).  The pixel fetch of the crop kernel converts each source pixel to RGB8 before the
interpolation, so every comparison here is equality of bits with the RGB route on the same frame converted on the host (cropprep.to_rgb)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from easy_vitpose_amd import Frame, VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.cropprep import prepare_crops_host, rgb_to_nv12, to_rgb
from easy_vitpose_amd.engine import crop_prep_device, crop_prep_image
from easy_vitpose_amd.synth import synthetic_moe_state_dict, synthetic_state_dict

pytestmark = pytest.mark.gpu

COCO_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
ALIGNED_H = 736   # frame 3: the UV plane of the 720-row surface starts behind this many rows of the Y pitch


def _surface(rgb, matrix, y_pitch, uv_pitch, aligned_h):
    """an NV12 decoder surface in ONE buffer: Y rows at y_pitch, the UV plane at base + y_pitch * aligned_h with rows at uv_pitch.  Returns
    (buffer, (y offset, uv offset) in bytes); the bytes between the rows are 0xEE: reading one of them changes a pixel"""
    y, uv = rgb_to_nv12(rgb, matrix)
    h, w = y.shape
    buf = np.full(y_pitch * aligned_h + uv_pitch * uv.shape[0], 0xEE, np.uint8)
    buf[:y_pitch * h].reshape(h, y_pitch)[:, :w] = y
    buf[y_pitch * aligned_h:].reshape(uv.shape[0], uv_pitch)[:, :2 * uv.shape[1]] = uv.reshape(uv.shape[0], -1)
    return buf, (0, y_pitch * aligned_h)


def _surface_frame(buf, offs, h, w, y_pitch, uv_pitch, matrix):
    """Frame.nv12 over the planes of such a buffer (numpy or torch: the same slicing)"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y = buf[offs[0]:offs[0] + y_pitch * h].reshape(h, y_pitch)[:, :w]
    uv = buf[offs[1]:offs[1] + uv_pitch * ch].reshape(ch, uv_pitch)[:, :2 * cw].reshape(ch, cw, 2)
    return Frame.nv12(y, uv, matrix)


@functools.lru_cache(maxsize=1)
def scene():
    """Six host frames from seeded RGB content and 18 crops, rows interleaved across frames.
      0  40 x 30 NV12 bt601          1  481 x 333 NV12 bt709 (odd both ways)        2  256 x 192 BGR
      3  720 x 1280 NV12 bt601_full, Y pitch 1344 and UV pitch 1408 in one allocation, UV behind an aligned height of 736 rows
      4  360 x 500 RGB at a pitch of 1920 bytes (a view of a 640-pixel-wide buffer)
      5  128 x 96 NV12 bt601, Y pitch 128 and UV pitch 160, the planes in two allocations"""
    rng = np.random.default_rng(21)
    rgb = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((40, 30), (481, 333), (256, 192), (720, 1280), (360, 500), (128, 96))]
    frames = [Frame.nv12(*rgb_to_nv12(rgb[0], 'bt601'), matrix='bt601'), Frame.nv12(*rgb_to_nv12(rgb[1], 'bt709'), matrix='bt709'),
              Frame.bgr(np.ascontiguousarray(rgb[2][..., ::-1]))]
    buf, offs = _surface(rgb[3], 'bt601_full', 1344, 1408, ALIGNED_H)
    frames.append(_surface_frame(buf, offs, 720, 1280, 1344, 1408, 'bt601_full'))
    wide = np.full((360, 640, 3), 0xEE, np.uint8)
    wide[:, 70:570] = rgb[4]
    frames.append(Frame.rgb(wide[:, 70:570]))
    y5, uv5 = rgb_to_nv12(rgb[5], 'bt601')
    yb, uvb = np.full((128, 128), 0xEE, np.uint8), np.full((64, 160), 0xEE, np.uint8)
    yb[:, :96], uvb[:, :96] = y5, uv5.reshape(64, 96)
    frames.append(Frame.nv12(yb[:, :96], uvb[:, :96].reshape(64, 48, 2), 'bt601'))
    assert frames[3].pitch == (1344, 1408) and frames[4].pitch == (1920, 0) and frames[5].pitch == (128, 160)
    p9 = np.array([
        (3, 101, 200, 150, 200, 0, 0, 150, 200),      # odd x0
        (3, 400, 301, 150, 200, 0, 0, 150, 200),      # odd y0
        (1, 31, 57, 120, 160, 0, 0, 120, 160),        # both odd
        (1, 0, 100, 90, 120, 0, 0, 90, 120),          # left border
        (1, 50, 0, 90, 120, 0, 0, 90, 120),           # top border
        (1, 250, 380, 83, 101, 0, 4, 83, 110),        # right and bottom border: the last column and row of the odd frame
        (0, 0, 0, 30, 40, 0, 0, 30, 40),              # whole frames
        (2, 0, 0, 192, 256, 0, 0, 192, 256),
        (1, 0, 0, 333, 481, 13, 0, 360, 481),
        (1, 101, 103, 12, 9, 0, 3, 12, 16),           # 12 x 9: upscales
        (3, 500, 200, 384, 512, 0, 0, 384, 512),      # exactly 2x, even origin
        (3, 501, 201, 384, 512, 0, 0, 384, 512),      # ... and odd origin
        (3, 896, 207, 384, 513, 0, 0, 384, 513),      # the right border of the pitched surface, down to its last row
        (4, 10, 20, 100, 120, 25, 30, 150, 200),      # left and top zero padding
        (4, 399, 239, 101, 121, 0, 0, 101, 134),      # the last column and row of the pitched RGB view
        (5, 1, 1, 95, 127, 0, 0, 96, 128),
        (5, 0, 0, 96, 128, 0, 0, 96, 128),
    ], np.int32)
    p9 = np.concatenate([p9, p9[2:3]])                # one crop listed twice
    p9 = np.ascontiguousarray(p9[np.random.default_rng(6).permutation(len(p9))])
    return frames, p9


def converted(frames):
    return [to_rgb(f) for f in frames]


def to_device(frames):
    """the same layouts in device memory: plane by plane, frame 3 as one allocation"""
    import torch
    out = []
    for i, f in enumerate(frames):
        if i == 3:
            base = f.planes[0].base
            while base.base is not None:
                base = base.base
            d = torch.from_numpy(base).cuda()
            out.append(_surface_frame(d, (0, 1344 * ALIGNED_H), 720, 1280, 1344, 1408, f.matrix))
            continue
        planes = []
        for p in f.planes:
            root = p
            while root.base is not None:
                root = root.base
            d = torch.from_numpy(root).cuda()   # the whole buffer, then the same view
            off = p.__array_interface__['data'][0] - root.__array_interface__['data'][0]
            planes.append(torch.as_strided(d.reshape(-1), p.shape, p.strides, off))
        out.append(Frame(f.format, planes, f.matrix))
    for f, d in zip(frames, out):
        assert d.on_device and d.pitch == f.pitch and (d.h, d.w) == (f.h, f.w)
    return out


def engine(dtype='fp16', max_batch=4):
    shp = model_shape('s', 'coco')
    return VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=dtype, max_batch=max_batch)   # chunks of 4 straddle frames and formats


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------------------
def test_crop_kernel_alone_equals_the_rgb_route_on_the_converted_frame():
    frames, p9 = scene()
    for f, fr in enumerate(frames):
        p8 = p9[p9[:, 0] == f][:, 1:]
        rgb = to_rgb(fr)
        want = crop_prep_device(rgb, p8)
        got = crop_prep_image(fr, p8)
        assert np.array_equal(got, want), f'frame {f} ({fr!r}): {(got != want).sum()} differing bytes'
        assert np.array_equal(want, prepare_crops_host(rgb, p8))      # ... which is the host restatement's
    # every matrix on one odd frame, and BGR / pitched RGB of the same content
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, (75, 53, 3), dtype=np.uint8)
    p8 = np.array([(0, 0, 53, 75, 0, 0, 57, 75), (1, 1, 52, 74, 0, 0, 56, 74), (21, 33, 12, 9, 0, 3, 12, 16), (52, 74, 1, 1, 0, 0, 1, 1), (7, 0, 39, 52, 0, 0, 39, 52)], np.int32)
    for matrix in ('bt601', 'bt709', 'bt601_full'):
        fr = Frame.nv12(*rgb_to_nv12(rgb, matrix), matrix=matrix)
        assert np.array_equal(crop_prep_image(fr, p8), crop_prep_device(to_rgb(fr), p8)), matrix
    assert not np.array_equal(to_rgb(Frame.nv12(*rgb_to_nv12(rgb, 'bt601'), matrix='bt601')), to_rgb(Frame.nv12(*rgb_to_nv12(rgb, 'bt601'), matrix='bt709')))
    want = crop_prep_device(rgb, p8)
    assert np.array_equal(crop_prep_image(Frame.bgr(np.ascontiguousarray(rgb[..., ::-1])), p8), want)
    wide = np.full((75, 90, 3), 0xEE, np.uint8)
    wide[:, 30:83] = rgb
    assert np.array_equal(crop_prep_image(Frame.rgb(wide[:, 30:83]), p8), want)
    assert np.array_equal(crop_prep_image(Frame.bgr(wide[:, 30:83]), p8), crop_prep_device(np.ascontiguousarray(rgb[..., ::-1]), p8))


# ---- 2. infer_frames ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_infer_frames_on_mixed_formats_equals_the_converted_frames(dtype):
    frames, p9 = scene()
    eng = engine(dtype)
    want = eng.infer_frames(converted(frames), p9)
    got = eng.infer_frames(frames, p9)                        # host frames: one upload per plane of each band
    assert got.shape == (len(p9), 17, 3) and np.array_equal(got, want), f'{(got != want).sum()} differing values'
    got_d = eng.infer_frames(to_device(frames), p9)           # device frames: read in place
    assert np.array_equal(got_d, want)
    if dtype == 'fp16':
        sub = p9[p9[:, 0] == 3][:1]                           # one crop deep inside the surface: a band of its rows only
        assert np.array_equal(eng.infer_frames(frames, sub), eng.infer_frames(converted(frames), sub))
        with pytest.raises(TypeError):
            eng.infer_frames([frames[0], to_device(frames)[1]], p9[:1])
    eng.close()


# ---- 3. infer_boxes -----------------------------------------------------------------------------------------------------------------------------
def boxes_of(frames):
    """float32 boxes [n, 6] + frame index: odd and .5 coordinates, border boxes, a whole frame, a bad frame index, an empty box"""
    per = [(3, [111, 210, 241, 390]), (1, [41.5, 67.5, 141.5, 207.5]), (0, [0, 0, 30, 40]), (2, [11, 13, 150, 201]), (4, [389, 229, 520, 380]),
           (5, [1, 1, 95, 127]), (3, [1001, 301, 1290, 730]), (len(frames), [10, 10, 50, 50]), (1, [260, 390, 333, 481]), (4, [300, 100, 200, 90]),
           (3, [511, 211, 865, 693]), (5, [20, 30, 60, 90]), (-1, [10, 10, 50, 50]), (1, [0, 0, 333, 481])]
    boxes = np.zeros((len(per), 6), np.float32)
    boxes[:, :4] = [b for _, b in per]
    return boxes, np.array([f for f, _ in per], np.int32)


def test_infer_boxes_on_device_frames_of_every_layout_equals_the_converted_frames():
    import torch
    frames, _ = scene()
    d_frames = to_device(frames)
    d_rgb = [torch.from_numpy(a).cuda() for a in converted(frames)]
    boxes, fidx = boxes_of(frames)
    d_boxes, d_fidx = torch.from_numpy(boxes).cuda(), torch.from_numpy(fidx).cuda()
    eng = engine()
    want = [t.cpu().numpy() for t in eng.infer_boxes(d_rgb, d_boxes, d_fidx, crop_params=True, status=True)]
    got = [t.cpu().numpy() for t in eng.infer_boxes(d_frames, d_boxes, d_fidx, crop_params=True, status=True)]
    assert want[2].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 3, 0, 0, 1, 0]
    for g, w, what in zip(got, want, ('keypoints', 'crop_params', 'status')):
        assert np.array_equal(g, w), what
    assert not got[0][7].any() and not got[0][9].any() and got[0][0].any()
    # a table of 65 entries that repeat the six frames: more than one launch window of the box kernel (64 frames)
    table = [d_frames[i % 6] for i in range(65)]
    table_rgb = [d_rgb[i % 6] for i in range(65)]
    fidx65 = np.where((fidx >= 0) & (fidx < 6), fidx + 6 * (np.arange(len(fidx)) % 10), fidx).astype(np.int32)
    fidx65[0], fidx65[1], fidx65[7] = 60 + fidx[0] + 0, 64, 65                     # the second window, its one frame (64 = frame 4's layout), and one past it
    boxes65 = boxes.copy()
    boxes65[1, :4] = (389, 229, 520, 380)
    d_boxes65, d_fidx65 = torch.from_numpy(boxes65).cuda(), torch.from_numpy(fidx65).cuda()
    want = [t.cpu().numpy() for t in eng.infer_boxes(table_rgb, d_boxes65, d_fidx65, crop_params=True, status=True)]
    got = [t.cpu().numpy() for t in eng.infer_boxes(table, d_boxes65, d_fidx65, crop_params=True, status=True)]
    assert want[2].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 3, 0, 0, 1, 0] and 64 in want[1][:, 0] and want[1][:, 0].max() == 64
    for g, w, what in zip(got, want, ('keypoints', 'crop_params', 'status')):
        assert np.array_equal(g, w), what
    with pytest.raises(TypeError):
        eng.infer_boxes(frames, d_boxes, d_fidx)              # host planes
    eng.close()


# ---- 4. ViTPose+ --------------------------------------------------------------------------------------------------------------------------------
def test_per_crop_datasets_on_nv12_frames():
    import torch
    frames, p9 = scene()
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_moe_state_dict(shp, 192, seed=0, peaked=True), dtype='fp16', max_batch=4)
    nv = [0, 1, 3, 5]                                          # the NV12 frames
    sel = np.concatenate([np.flatnonzero(p9[:, 0] == f)[:2] for f in nv])[:6]
    sub = np.ascontiguousarray(p9[np.sort(sel)])
    assert len(sub) == 6 and set(sub[:, 0].tolist()) <= set(nv)
    datasets = ['coco', 'aic', 'wholebody', 'aic', 'coco', 'wholebody']
    want, k = eng.infer_frames(converted(frames), sub, datasets=datasets)
    got, k2 = eng.infer_frames(frames, sub, datasets=datasets)
    assert np.array_equal(got, want) and np.array_equal(k, k2) and sorted(set(k.tolist())) == [14, 17, 133]
    got_d, _ = eng.infer_frames(to_device(frames), sub, datasets=datasets)
    assert np.array_equal(got_d, want)
    # the boxes entry, a dataset per box
    boxes, fidx = boxes_of(frames)
    keep = np.flatnonzero(np.isin(fidx, nv))[:6]
    d_boxes, d_fidx = torch.from_numpy(boxes[keep]).cuda(), torch.from_numpy(fidx[keep]).cuda()
    d_rgb = [torch.from_numpy(a).cuda() for a in converted(frames)]
    want = [t.cpu().numpy() for t in eng.infer_boxes(d_rgb, d_boxes, d_fidx, crop_params=True, status=True, datasets=datasets)]
    got = [t.cpu().numpy() for t in eng.infer_boxes(to_device(frames), d_boxes, d_fidx, crop_params=True, status=True, datasets=datasets)]
    assert got[0].shape == (6, 133, 3) and (want[2] == 0).all()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    eng.close()


# ---- 5. the flip-test mode ----------------------------------------------------------------------------------------------------------------------
def test_flip_test_mode_on_mixed_formats():
    frames, p9 = scene()
    eng = engine()
    plain = eng.infer_frames(converted(frames), p9)
    eng.set_flip_test(COCO_PAIRS)
    want = eng.infer_frames(converted(frames), p9)            # the mode's bits on the converted frames (chunks of 2)
    assert not np.array_equal(want, plain)
    assert np.array_equal(eng.infer_frames(frames, p9), want)
    assert np.array_equal(eng.infer_frames(to_device(frames), p9), want)
    eng.close()


# ---- 6. refusals that reach the device checks ---------------------------------------------------------------------------------------------------
def test_device_plane_checks_refuse_before_anything_is_enqueued():
    import torch
    lib = capi.load_library()
    frames, p9 = scene()
    eng = engine()
    d_frames = to_device(frames)
    sub = np.ascontiguousarray(p9[p9[:, 0] == 0][:1])         # one crop of frame 0 (40 x 30, NV12)
    want = eng.infer_frames(d_frames[:1], sub)
    y, uv = d_frames[0].planes
    d_box = torch.tensor([[2, 3, 20, 30]], dtype=torch.float32, device='cuda')
    want_b = eng.infer_boxes(d_frames[:1], d_box).cpu().numpy()
    out = np.full((1, 17, 3), 7.0, np.float32)
    d_out = torch.full((1, 17, 3), 7.0, device='cuda')
    torch.cuda.synchronize()

    def image(p0, p1, pitch1=30):
        return capi.vp_image((C.c_void_p * 2)(p0, p1), (C.c_int64 * 2)(30, pitch1), 40, 30, capi.VP_PIX_NV12, capi.VP_YUV_BT601)

    host_uv = np.ascontiguousarray(frames[0].planes[1])
    cases = {
        'the last UV row runs past its allocation': image(y.data_ptr(), uv.data_ptr(), 1 << 28),   # 19 rows of 256 MiB behind the first: past any allocation
        'the UV plane is on the host': image(y.data_ptr(), host_uv.ctypes.data),
        'the Y plane is on the host': image(np.ascontiguousarray(frames[0].planes[0]).ctypes.data, uv.data_ptr()),
    }
    for what, im in cases.items():
        rc = lib.vp_infer_images(eng._h, C.byref(im), 1, 1, sub.ctypes.data, 1, None, out.ctypes.data)
        assert rc == capi.VP_ERR_INVALID and 'frame 0' in capi.last_error(eng._h), what
        assert (out == 7.0).all()
        rc = lib.vp_infer_boxes_images_stream(eng._h, C.byref(im), 1, d_box.data_ptr(), 4, None, 1, 10, None, d_out.data_ptr(), None, None,
                                              torch.cuda.current_stream().cuda_stream)
        assert rc == capi.VP_ERR_INVALID and 'frame 0' in capi.last_error(eng._h), what
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 7.0).all(), what        # nothing was enqueued
        # ... and the handle is as good as before
        assert np.array_equal(eng.infer_frames(d_frames[:1], sub), want)
        assert np.array_equal(eng.infer_boxes(d_frames[:1], d_box).cpu().numpy(), want_b)
    ok = image(y.data_ptr(), uv.data_ptr())
    assert lib.vp_infer_images(eng._h, C.byref(ok), 1, 1, sub.ctypes.data, 1, None, out.ctypes.data) == capi.VP_OK
    assert np.array_equal(out, want)
    eng.close()


# ---- 7. bare strided tensors --------------------------------------------------------------------------------------------------------------------
def test_a_strided_device_tensor_is_read_in_place():
    import torch
    rng = np.random.default_rng(13)
    wide = torch.from_numpy(rng.integers(0, 256, (300, 520, 3), dtype=np.uint8)).cuda()
    view = wide[11:291, 37:460]                                # [280, 423, 3] at a pitch of 1560 bytes
    assert not view.is_contiguous() and view.stride() == (1560, 3, 1)
    copy = view.contiguous()
    p9 = np.array([(0, 1, 1, 150, 200, 0, 0, 150, 200), (0, 0, 0, 423, 280, 0, 142, 423, 564), (0, 333, 179, 90, 101, 0, 9, 90, 120)], np.int32)
    eng = engine()
    want = eng.infer_frames([copy], p9)
    assert np.array_equal(eng.infer_frames([view], p9), want)
    host_view = wide.cpu().numpy()[11:291, 37:460]             # a host view passes in place as well
    assert np.array_equal(eng.infer_frames([host_view], p9), want)
    assert np.array_equal(eng.infer_frames([host_view[..., ::-1]], p9), eng.infer_frames([np.ascontiguousarray(host_view[..., ::-1])], p9))   # not a vp_image: copied, as before
    d_boxes = torch.tensor([[11, 11, 141, 191], [0, 0, 423, 280], [343, 189, 430, 290]], dtype=torch.float32, device='cuda')
    want_b = [t.cpu().numpy() for t in eng.infer_boxes([copy], d_boxes, crop_params=True)]
    got_b = [t.cpu().numpy() for t in eng.infer_boxes([view], d_boxes, crop_params=True)]
    assert np.array_equal(got_b[0], want_b[0]) and np.array_equal(got_b[1], want_b[1])
    with pytest.raises(ValueError):
        eng.infer_boxes([wide[:, ::2]], d_boxes)               # pixels 6 bytes apart: no vp_image describes it
    eng.close()
