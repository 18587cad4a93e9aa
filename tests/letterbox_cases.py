"""The named cases of the letterbox stage (csrc/lbgeom.h), shared by tests/test_letterbox_host.py (host tap against the numpy twin) and
tests/test_gpu_letterbox.py (device against the host tap): tiny inputs, chosen for where the code forks.  A case is (LetterboxCfg, [host Frame, ...])."""
from __future__ import annotations

import numpy as np

from easy_vitpose_amd.cropprep import Frame, rgb_to_nv12
from easy_vitpose_amd.devletterbox import LetterboxCfg

CANARY = 0xA5


def rgb_image(h, w, seed):
    """smooth content plus noise, so that a wrong tap or weight shows"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 7 + xx * 3) % 256, (yy * 2 + xx * 11 + 40) % 256, (yy * 5 + xx * 5 + 90) % 256], -1)
    return ((base + rng.integers(0, 64, (h, w, 3))) % 256).astype(np.uint8)


def pitched(a, extra, inner):
    """`a` [rows, ...] as a view with `extra` more bytes per row, cut out of a canary-filled parent with a canary margin on every side"""
    rows, row_bytes = a.shape[0], int(np.prod(a.shape[1:]))
    pitch = row_bytes + extra
    parent = np.full((rows + 2) * pitch + 16, CANARY, np.uint8)
    view = np.lib.stride_tricks.as_strided(parent[pitch + 5:], shape=a.shape, strides=(pitch,) + inner, writeable=True)
    view[...] = a
    return view


def rgb_frame(h, w, seed, extra=0):
    a = rgb_image(h, w, seed)
    return Frame.rgb(pitched(a, extra, (3, 1)) if extra else a)


def bgr_frame(h, w, seed, extra=0):
    a = np.ascontiguousarray(rgb_image(h, w, seed)[..., ::-1])
    return Frame.bgr(pitched(a, extra, (3, 1)) if extra else a)


def nv12_frame(h, w, seed, matrix='bt601', extra=0):
    y, uv = rgb_to_nv12(rgb_image(h, w, seed), matrix)
    rng = np.random.default_rng(seed + 1)   # full-range planes: the clips of the conversion are reached
    y = (y.astype(np.int32) + rng.integers(-40, 40, y.shape)).clip(0, 255).astype(np.uint8)
    uv = (uv.astype(np.int32) + rng.integers(-60, 60, uv.shape)).clip(0, 255).astype(np.uint8)
    if extra:
        return Frame.nv12(pitched(y, extra, (1,)), pitched(uv, extra + 2, (2, 1)), matrix)
    return Frame.nv12(y, uv, matrix)


def named_cases():
    c = {}
    S32 = LetterboxCfg((32, 32))
    # sizes and scale
    c['identity'] = (S32, [rgb_frame(32, 32, 1)])
    c['same_aspect_up'] = (S32, [rgb_frame(16, 16, 2)])
    c['same_aspect_down'] = (S32, [rgb_frame(48, 48, 3)])
    c['box_2x'] = (S32, [rgb_frame(64, 64, 4)])
    c['box_2x_nv12'] = (S32, [nv12_frame(64, 64, 5)])
    c['two_x_on_one_axis_and_half_up'] = (S32, [rgb_frame(64, 3, 6)])       # new_w = round(1.5) = 2: scale_y 2, scale_x 1.5, no box average
    c['half_to_even_down'] = (S32, [rgb_frame(64, 5, 7)])                   # new_w = round(2.5) = 2
    c['down_3x'] = (S32, [rgb_frame(96, 96, 8)])
    c['down_3x_nv12'] = (S32, [nv12_frame(96, 96, 9, 'bt709')])
    for h, w in ((1, 1), (2, 2), (1, 7), (7, 1)):
        c[f'frame_{h}x{w}'] = (LetterboxCfg((16, 16)), [rgb_frame(h, w, 10 + h + w), nv12_frame(h, w, 20 + h + w)])
    # placement
    c['wide'] = (S32, [rgb_frame(20, 50, 30)])
    c['tall'] = (S32, [rgb_frame(50, 20, 31)])
    c['wide_into_48x40'] = (LetterboxCfg((48, 40)), [nv12_frame(20, 50, 32)])
    c['tall_into_48x40'] = (LetterboxCfg((48, 40)), [bgr_frame(100, 20, 33)])
    c['odd_pad_5x7'] = (S32, [rgb_frame(5, 7, 34)])
    c['no_scaleup_small'] = (LetterboxCfg((32, 32), scaleup=False), [rgb_frame(10, 13, 35), nv12_frame(9, 11, 36)])
    c['no_scaleup_large'] = (LetterboxCfg((32, 32), scaleup=False), [rgb_frame(50, 70, 37)])
    # formats
    for m in ('bt601', 'bt709', 'bt601_full'):
        c[f'nv12_odd_{m}'] = (LetterboxCfg((48, 40)), [nv12_frame(33, 21, 40, m), nv12_frame(21, 33, 41, m)])
    c['bgr'] = (S32, [bgr_frame(20, 33, 42)])
    c['pitched'] = (S32, [rgb_frame(20, 33, 43, extra=7), bgr_frame(41, 17, 44, extra=1), nv12_frame(33, 21, 45, 'bt709', extra=9), nv12_frame(64, 64, 46, extra=3)])
    # output: the run is 8 (fp16), 4 (fp32) or 16 (u8) adjacent x.  in_w = 32: a multiple of every run (the 16-byte stores); 20: full runs and a tail for fp16 and
    # u8, a multiple for fp32, whose 16-byte stores it takes; 37: several full runs and a tail for every run (the element stores); 3: below one run
    for dtype in ('fp16', 'fp32', 'u8'):
        c[f'in_w_below_run_{dtype}'] = (LetterboxCfg((4, 3), dtype=dtype), [rgb_frame(9, 5, 50), nv12_frame(2, 7, 51)])
        c[f'in_w_16_{dtype}'] = (LetterboxCfg((16, 16), dtype=dtype), [nv12_frame(30, 41, 52)])
        for layout in ('nchw', 'nhwc'):
            for order in ('rgb', 'bgr'):
                for hw in ((32, 32), (33, 20), (9, 37)):
                    c[f'out_{dtype}_{layout}_{order}_{hw[0]}x{hw[1]}'] = (LetterboxCfg(hw, dtype, layout, order), [nv12_frame(21, 33, 53), bgr_frame(40, 17, 54)])
    for pad in (0, 114, 255):
        c[f'pad_value_{pad}'] = (LetterboxCfg((33, 20), pad_value=pad), [rgb_frame(9, 30, 55)])
    # batch
    c['mixed_batch'] = (LetterboxCfg((48, 40), dtype='fp32'), [nv12_frame(33, 21, 60, 'bt601_full'), bgr_frame(64, 64, 61), rgb_frame(96, 80, 62, extra=5), rgb_frame(48, 40, 63),
                                                                nv12_frame(1, 6, 64)])
    c['n_images_0'] = (S32, [])
    c['n_images_1'] = (S32, [nv12_frame(17, 23, 65)])
    c['n_images_2'] = (S32, [nv12_frame(17, 23, 66), rgb_frame(23, 17, 67)])
    c['n_images_64'] = (LetterboxCfg((16, 16)), [(rgb_frame, bgr_frame, nv12_frame)[i % 3](1 + (i * 5) % 23, 1 + (i * 11) % 19, 70 + i) for i in range(64)])
    return c


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
