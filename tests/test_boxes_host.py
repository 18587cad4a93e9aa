"""CPU: the box geometry of the stream-ordered boxes entry (vp_infer_boxes_stream) through its host-only tap vp_dbg_box_geometry, which runs the
function the device kernel runs (csrc/boxgeom.h): row for row against cropprep.frames_crop_params on float32 boxes widened to float64, the status
codes, and the host-argument refusals -- none of which needs a device."""
import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.cropprep import frames_crop_params

SIZES = [(40, 30), (480, 640), (1080, 1920), (720, 1280), (256, 192), (601, 451)]


def tap(boxes, frame_idx, sizes, pad, row_stride=None, n_frames=None):
    """vp_dbg_box_geometry on host arrays -> (rc, rows [n, 9], status [n])"""
    lib = capi.load_library()
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    n = boxes.shape[0]
    hw = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
    fi = None if frame_idx is None else np.ascontiguousarray(frame_idx, dtype=np.int32)
    out9 = np.full((n, 9), -7, np.int32)
    st = np.full(n, -7, np.int32)
    rc = lib.vp_dbg_box_geometry(boxes.ctypes.data if n else None, boxes.shape[1] if row_stride is None else row_stride,
                                 None if fi is None else fi.ctypes.data, hw.ctypes.data, len(hw) if n_frames is None else n_frames,
                                 n, pad, out9.ctypes.data, st.ctypes.data)
    return rc, out9, st


def host_rows(boxes, frame_idx, sizes, pad):
    """What the host path computes per box: frames_crop_params on the float64 box (status 3 where it asserts 'empty box')."""
    rows = np.zeros((len(boxes), 9), np.int32)
    status = np.zeros(len(boxes), np.int32)
    for i, (b, f) in enumerate(zip(np.asarray(boxes, np.float32), frame_idx)):
        if not 0 <= f < len(sizes):
            status[i] = 1
        elif not np.isfinite(b[:4]).all():
            status[i] = 2
        else:
            try:
                p = frames_crop_params([b[None, :4].astype(np.float64)], [sizes[f]], pad)
            except AssertionError as e:
                assert 'empty box' in str(e)
                status[i] = 3
                continue
            rows[i] = p[0]
            rows[i, 0] = f
    return rows, status


def sweep_boxes(seed, n=10_500):
    """Seeded float32 boxes over SIZES: random ones (inverted, beyond every border, negative), exact .5 ties on even and odd integers, padded crops of
    exactly 192 x 256 / 384 x 512 (for each pad), cw / ch exactly 0.75 and its integer neighbours (300/400, 299/400, 301/400, ...) -- both pad_image
    branches -- in the detector's [n, 6] layout (score and class columns behind the box)."""
    rng = np.random.default_rng(seed)
    fidx = rng.integers(0, len(SIZES), n).astype(np.int32)
    hw = np.asarray(SIZES, np.float64)[fidx]
    H, W = hw[:, 0], hw[:, 1]
    b = np.stack([rng.uniform(-0.3, 1.3, n) * W, rng.uniform(-0.3, 1.3, n) * H, rng.uniform(-0.3, 1.3, n) * W, rng.uniform(-0.3, 1.3, n) * H], 1)
    order = rng.random(n) < 0.8   # most boxes ordered, the rest possibly inverted
    b[order] = np.stack([np.minimum(b[order, 0], b[order, 2]), np.minimum(b[order, 1], b[order, 3]),
                         np.maximum(b[order, 0], b[order, 2]), np.maximum(b[order, 1], b[order, 3])], 1)
    ties = rng.random(n) < 0.3    # k + 0.5 on even and odd k
    b[ties] = np.floor(b[ties]) + 0.5
    big = iter([i for i in range(n) if SIZES[fidx[i]][0] >= 1000])
    for pad in (0, 10, 37):       # boxes whose padded crop (under that pad) is exactly cw x ch, inside the frame
        for cw, ch in ((192, 256), (384, 512), (300, 400), (299, 400), (301, 400), (3, 4), (600, 800), (599, 800), (601, 800), (450, 600)):
            for _ in range(3):
                i = next(big)
                h, w = SIZES[fidx[i]]
                x0, y0 = int(rng.integers(pad, w - cw - pad + 1)), int(rng.integers(pad, h - ch - pad + 1))
                b[i] = (x0 + pad, y0 + pad, x0 + cw - pad, y0 + ch - pad)
    out = np.zeros((n, 6), np.float32)
    out[:, :4] = b
    out[:, 4] = rng.random(n)
    out[:, 5] = rng.integers(0, 80, n)
    return out, fidx


@pytest.mark.parametrize('pad', [0, 10, 37])
def test_box_geometry_equals_frames_crop_params_row_for_row(pad):
    boxes, fidx = sweep_boxes(100 + pad)
    rc, rows, st = tap(boxes, fidx, SIZES, pad)
    assert rc == capi.VP_OK, capi.last_error()
    want, want_st = host_rows(boxes, fidx, SIZES, pad)
    assert np.array_equal(st, want_st), np.flatnonzero(st != want_st)[:10]
    assert np.array_equal(rows, want), np.flatnonzero((rows != want).any(1))[:10]
    ok = want_st == 0
    assert ok.sum() > 7000 and (want_st == 3).sum() > 100                         # both outcomes are exercised
    p = want[ok]
    assert ((p[:, 5] > 0) & (p[:, 6] == 0)).sum() > 100 and ((p[:, 6] > 0) & (p[:, 5] == 0)).sum() > 100   # both pad_image branches
    for cw, ch in ((192, 256), (384, 512)):
        assert ((p[:, 7] == cw) & (p[:, 8] == ch)).sum() >= 3
    # the row stride is honoured: the same boxes packed as [n, 4]
    rc4, rows4, st4 = tap(np.ascontiguousarray(boxes[:, :4]), fidx, SIZES, pad)
    assert rc4 == capi.VP_OK and np.array_equal(rows4, rows) and np.array_equal(st4, st)


def test_box_geometry_ties_round_half_to_even():
    # x1 = 2.5 / 3.5 round to 2 / 4 (numpy's round), y likewise; pad 0 on a large frame
    boxes = np.array([[2.5, 2.5, 102.5, 302.5], [3.5, 3.5, 103.5, 303.5], [-0.5, -1.5, 50.5, 51.5]], np.float32)
    rc, rows, st = tap(boxes, [0, 0, 0], [(1080, 1920)], 0)
    assert rc == capi.VP_OK and (st == 0).all()
    assert rows[0, 1:5].tolist() == [2, 2, 100, 300] and rows[1, 1:5].tolist() == [4, 4, 100, 300]
    assert rows[2, 1:5].tolist() == [0, 0, 50, 52]
    want, _ = host_rows(boxes, [0, 0, 0], [(1080, 1920)], 0)
    assert np.array_equal(rows, want)


def test_box_geometry_status_codes_and_zero_rows():
    sizes = [(480, 640), (40, 30)]
    good = [[100, 50, 300, 400], [2, 3, 20, 30], [600.5, 400.5, 700, 500]]
    rows_in = good + [[10, 10, 50, 50], [10, 10, 50, 50],                                   # frame index -1 / n_frames
                      [np.nan, 10, 50, 50], [10, np.inf, 50, 50], [10, 10, -np.inf, 50],   # not finite
                      [-200, 10, -100, 50], [10, 500, 50, 600], [300, 300, 250, 250],      # left of / below the frame, inverted
                      [np.nan, 10, 50, 50]]                                                # not finite AND a bad frame: the frame wins
    fidx = [0, 1, 0, -1, 2, 0, 1, 0, 0, 0, 1, 5]
    boxes = np.array(rows_in, np.float32)
    rc, rows, st = tap(boxes, fidx, sizes, 10)
    assert rc == capi.VP_OK
    assert st.tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 1]
    assert (rows[3:] == 0).all()
    want, want_st = host_rows(boxes[:3], fidx[:3], sizes, 10)
    assert np.array_equal(rows[:3], want) and (want_st == 0).all()
    # huge finite coordinates are clipped like any others: -1e30 .. 1e30 is the full frame; a box entirely beyond the right border is empty
    rc, rows, st = tap(np.array([[-1e30, -1e30, 1e30, 1e30], [3e38, 0, 3.4e38, 10]], np.float32), [0, 0], sizes, 10)
    assert rc == capi.VP_OK and st.tolist() == [0, 3]
    ph = int(640 / 0.75)
    assert rows[0].tolist() == [0, 0, 0, 640, 480, 0, (ph - 480) // 2, 640, ph] and (rows[1] == 0).all()
    # no frame index table: every box on frame 0
    rc0, rows0, st0 = tap(boxes[:3], None, sizes, 10)
    rc1, rows1, st1 = tap(boxes[:3], [0, 0, 0], sizes, 10)
    assert rc0 == rc1 == capi.VP_OK and np.array_equal(rows0, rows1) and np.array_equal(st0, st1)


def test_box_argument_refusals_without_a_device():
    lib = capi.load_library()
    boxes = np.zeros((2, 6), np.float32)
    boxes[:, 2:4] = 50
    assert tap(boxes, [0, 0], SIZES, 10)[0] == capi.VP_OK
    assert tap(boxes, [0, 0], SIZES, 10, row_stride=3)[0] == capi.VP_ERR_INVALID
    assert 'row_stride' in capi.last_error()
    assert tap(boxes, [0, 0], SIZES, -1)[0] == capi.VP_ERR_INVALID
    assert tap(boxes, [0, 0], SIZES, 10, n_frames=0)[0] == capi.VP_ERR_INVALID
    assert tap(boxes, [0, 0], [(0, 30)], 10)[0] == capi.VP_ERR_INVALID                 # a frame without pixels
    assert tap(boxes, [0, 0], [(40, 1 << 25)], 10)[0] == capi.VP_ERR_INVALID           # a side beyond 2^24
    hw = np.array([[40, 30]], np.int32)
    assert lib.vp_dbg_box_geometry(None, 4, None, hw.ctypes.data, 1, 2, 10, None, None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_box_geometry(None, 4, None, None, 0, 0, 10, None, None) == capi.VP_OK   # n = 0: nothing to check, nothing written
    # the entry point itself: a NULL handle, whatever else is passed
    table = (capi.vp_frame * 1)(capi.vp_frame(None, 40, 30))
    for n_frames, stride, pad in ((1, 4, 10), (1, 3, 10), (1, 4, -1), (0, 4, 10)):
        assert lib.vp_infer_boxes_stream(None, table, n_frames, boxes.ctypes.data, stride, None, 2, pad, boxes.ctypes.data, None, None,
                                         None) == capi.VP_ERR_INVALID
