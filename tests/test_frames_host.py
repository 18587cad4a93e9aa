"""CPU: the host side of the many-frames entry (vp_infer_frames) -- its plan (vp_dbg_frame_plan: the bands each frame uploads and
every refusal, all before a copy or a launch), the null handle, and the frames crop table of cropprep."""
import ctypes as C

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.cropprep import crop_params, frames_crop_params

SIZES = [(720, 1280), (1080, 1920), (481, 333), (256, 192), (40, 30)]
_DUMMY = np.zeros(16, np.uint8)   # the plan never reads pixels: any non-NULL pointer stands for a frame


def frame_table(sizes, null=()):
    t = (capi.vp_frame * max(len(sizes), 1))()
    for i, (h, w) in enumerate(sizes):
        t[i] = capi.vp_frame(None if i in null else _DUMMY.ctypes.data, h, w)
    return t


def plan(sizes, p9, n_frames=None, null=()):
    lib = capi.load_library()
    p9 = np.ascontiguousarray(p9, dtype=np.int32).reshape(-1, 9)
    nf = len(sizes) if n_frames is None else n_frames
    bands = np.full((max(len(sizes), 1), 2), -7, np.int32)
    rc = lib.vp_dbg_frame_plan(frame_table(sizes, null), nf, p9.ctypes.data if len(p9) else None, len(p9), bands.ctypes.data)
    return rc, bands[:len(sizes)]


def random_table(rng, sizes, per_frame, empty):
    rows = []
    for f, (h, w) in enumerate(sizes):
        if f == empty:
            continue
        for _ in range(per_frame[f]):
            cw, ch = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
            x0, y0 = int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1))
            left, top = int(rng.integers(0, 5)), int(rng.integers(0, 5))
            rows.append((f, x0, y0, cw, ch, left, top, left + cw + int(rng.integers(0, 9)), top + ch + int(rng.integers(0, 9))))
    p9 = np.array(rows, np.int32).reshape(-1, 9)
    return p9[rng.permutation(len(p9))]   # interleaved across frames


@pytest.mark.parametrize('seed', range(6))
def test_frame_plan_bands_are_min_max_of_each_frames_crops(seed):
    rng = np.random.default_rng(seed)
    empty = seed % len(SIZES)
    p9 = random_table(rng, SIZES, rng.integers(1, 7, len(SIZES)), empty)
    rc, bands = plan(SIZES, p9)
    assert rc == capi.VP_OK, capi.last_error()
    for f in range(len(SIZES)):
        q = p9[p9[:, 0] == f]
        want = (0, 0) if len(q) == 0 else (q[:, 2].min(), (q[:, 2] + q[:, 4]).max())
        assert tuple(bands[f]) == tuple(want)
    assert tuple(bands[empty]) == (0, 0)


def test_frame_plan_whole_frame_and_border_crops():
    h, w = 481, 333
    p9 = np.array([[0, 0, 0, w, h, 0, 0, w, h],               # the whole frame
                   [1, w - 7, 0, 7, 9, 3, 0, 12, 9],          # top-right corner
                   [1, 0, h - 5, 4, 5, 0, 2, 4, 8]], np.int32)  # bottom-left corner
    rc, bands = plan([(h, w), (h, w), (h, w)], p9)
    assert rc == capi.VP_OK
    assert bands.tolist() == [[0, h], [0, h], [0, 0]]


def test_frame_plan_empty_call():
    assert plan(SIZES, np.zeros((0, 9), np.int32))[0] == capi.VP_OK
    assert plan([], np.zeros((0, 9), np.int32))[0] == capi.VP_OK


GOOD = (1, 10, 20, 30, 40, 0, 5, 30, 50)


@pytest.mark.parametrize('case,row', [
    ('frame index below 0', (-1,) + GOOD[1:]),
    ('frame index past the last frame', (len(SIZES),) + GOOD[1:]),
    ('x0 < 0', (1, -1) + GOOD[2:]),
    ('y0 < 0', (1, 10, -1) + GOOD[3:]),
    ('past the right border', (1, 1920 - 29) + GOOD[2:]),
    ('past the bottom border', (1, 10, 1080 - 39) + GOOD[3:]),
    ('past the right border of a small frame', (4, 10, 0, 21, 20, 0, 0, 21, 28)),
    ('zero width', (1, 10, 20, 0, 40, 0, 0, 30, 40)),
    ('negative height', (1, 10, 20, 30, -4, 0, 0, 30, 40)),
    ('zero canvas', (1, 10, 20, 30, 40, 0, 0, 0, 0)),
    ('left pad < 0', (1, 10, 20, 30, 40, -1, 0, 30, 40)),
    ('top pad < 0', (1, 10, 20, 30, 40, 0, -1, 30, 40)),
    ('outside the canvas width', (1, 10, 20, 30, 40, 1, 0, 30, 40)),
    ('outside the canvas height', (1, 10, 20, 30, 40, 0, 11, 30, 50)),
    ('overflowing x0 + cw', (1, 2 ** 31 - 10, 20, 30, 40, 0, 0, 30, 40)),
])
def test_frame_plan_refuses_bad_crops(case, row):
    p9 = np.array([GOOD, row, GOOD], np.int32)
    rc, _ = plan(SIZES, p9)
    assert rc == capi.VP_ERR_INVALID, case
    assert capi.last_error()
    assert plan(SIZES, np.array([GOOD], np.int32))[0] == capi.VP_OK


def test_frame_plan_refuses_null_data_and_bad_frame_sizes_only_where_referenced():
    p9 = np.array([GOOD], np.int32)
    assert plan(SIZES, p9, null=(1,))[0] == capi.VP_ERR_INVALID
    assert plan(SIZES, p9, null=(0, 2, 3, 4))[0] == capi.VP_OK            # frames without crops are never touched
    bad = list(SIZES)
    bad[1] = (0, 1920)
    assert plan(bad, p9)[0] == capi.VP_ERR_INVALID
    bad[1], bad[3] = SIZES[1], (-5, 0)
    assert plan(bad, p9)[0] == capi.VP_OK


def test_frame_plan_refuses_crops_without_frames():
    lib = capi.load_library()
    p9 = np.array([GOOD], np.int32)
    assert plan(SIZES, p9, n_frames=0)[0] == capi.VP_ERR_INVALID
    assert plan(SIZES, p9, n_frames=-3)[0] == capi.VP_ERR_INVALID
    assert plan(SIZES, p9, n_frames=1)[0] == capi.VP_ERR_INVALID      # frame 1 of a one-frame table
    assert lib.vp_dbg_frame_plan(None, 5, p9.ctypes.data, 1, None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_frame_plan(frame_table(SIZES), 5, None, 1, None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_frame_plan(frame_table(SIZES), 5, p9.ctypes.data, -1, None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_frame_plan(frame_table(SIZES), 5, p9.ctypes.data, 1, None) == capi.VP_OK   # bands may be NULL


def test_infer_frames_null_handle_is_rejected_without_a_device():
    lib = capi.load_library()
    p9 = np.array([GOOD], np.int32)
    out = np.zeros((1, 17, 3), np.float32)
    assert lib.vp_infer_frames(None, frame_table(SIZES), len(SIZES), 0, p9.ctypes.data, 1, out.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_infer_frames(None, frame_table(SIZES), len(SIZES), 1, p9.ctypes.data, 1, out.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_infer_frames(None, None, 0, 0, None, 0, None) == capi.VP_ERR_INVALID


def test_frames_crop_params_is_per_frame_crop_params_with_the_frame_column():
    rng = np.random.default_rng(3)
    shapes = [(720, 1280, 3), (1080, 1920, 3), (481, 333, 3), (40, 30, 3)]
    boxes = []
    for f, (h, w, _) in enumerate(shapes):
        k = 0 if f == 2 else f + 1
        x1, y1 = rng.uniform(0, w * 0.8, k), rng.uniform(0, h * 0.8, k)
        boxes.append(np.stack([x1, y1, x1 + rng.uniform(2, w * 0.5, k), y1 + rng.uniform(2, h * 0.5, k), np.ones(k)], 1))
    p9 = frames_crop_params(boxes, shapes)
    assert p9.dtype == np.int32 and p9.shape == (sum(len(b) for b in boxes), 9)
    want = [np.concatenate([np.full((len(b), 1), f), crop_params(b, shapes[f][:2])], 1) for f, b in enumerate(boxes) if len(b)]
    assert np.array_equal(p9, np.concatenate(want))
    assert 2 not in p9[:, 0]
    assert frames_crop_params([np.zeros((0, 5))] * 3, shapes[:3]).shape == (0, 9)
    assert np.array_equal(frames_crop_params(boxes[1:2], shapes[1:2], pad_bbox=0)[:, 1:], crop_params(boxes[1], shapes[1][:2], 0))
    # and the plan accepts every table it builds, with the bands of those crops
    lib = capi.load_library()
    bands = np.zeros((len(shapes), 2), np.int32)
    assert lib.vp_dbg_frame_plan(frame_table([s[:2] for s in shapes]), len(shapes), p9.ctypes.data, len(p9), bands.ctypes.data) == capi.VP_OK
    assert bands[2].tolist() == [0, 0]
