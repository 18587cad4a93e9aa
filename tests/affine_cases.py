"""Seeded inputs of the affine-crop tests, shared by the golden generator (tests/golden/make_golden_affine.py) and the tests: regenerated from
seeds, only the reference's OUTPUTS live in tests/golden/affine.npz."""
from __future__ import annotations

import numpy as np

FRAME_A_HW = (240, 320)   # RGB
FRAME_B_HW = (96, 132)    # NV12 in the GPU tests (RGB content made into NV12 by cropprep.rgb_to_nv12)
DECODE_SEEDS = {17: 61, 133: 62}


def frame_rgb(hw, seed: int) -> np.ndarray:
    """A seeded uint8 RGB frame: noise under a few bright blobs"""
    rng = np.random.default_rng(seed)
    h, w = hw
    f = rng.integers(0, 256, size=(h, w, 3)).astype(np.float64) * 0.5
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(4):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.2) * h
        f += 120.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * r * r))[..., None] * rng.uniform(0.3, 1.0, size=3)
    return np.clip(f, 0, 255).astype(np.uint8)


def frames():
    return frame_rgb(FRAME_A_HW, 71), frame_rgb(FRAME_B_HW, 72)


def frame_b_nv12(matrix: str = 'bt601'):
    """frame B as the NV12 surface the GPU tests and the end-to-end golden use: (y, uv) made from its RGB content by cropprep.rgb_to_nv12 (a content maker,
    not an oracle: what the entries see of it is the integer conversion of csrc/pixfmt.h, restated by tests/affine_model.py)"""
    from easy_vitpose_amd.cropprep import rgb_to_nv12
    return rgb_to_nv12(frames()[1], matrix)


def geometry_boxes() -> np.ndarray:
    """float32 [40, 4] (x1, y1, x2, y2): the named cases first -- wider than 3:4, narrower, exactly 3:4, 2 x 3 px, 3000 x 3900 px on a 4K frame,
    four that reach outside a 320 x 240 frame -- then seeded ones with fractional corners."""
    named = [[30.0, 40.0, 230.0, 140.0],          # wider than 3:4
             [100.25, 10.5, 140.75, 200.125],     # narrower
             [60.0, 20.0, 150.0, 140.0],          # exactly 3:4 (90 x 120)
             [17.0, 33.0, 19.0, 36.0],            # 2 x 3 px
             [400.0, 100.0, 3400.0, 4000.0],      # 3000 x 3900 on a 4K (3840 x 2160) frame: below the frame's bottom too
             [-40.5, -20.25, 80.0, 130.0],        # over the top-left corner
             [250.0, 150.0, 400.0, 330.0],        # over the bottom-right corner
             [-500.0, -500.0, -400.0, -380.0],    # wholly outside
             [300.0, -10.0, 340.0, 250.0]]        # over the right edge, top and bottom
    rng = np.random.default_rng(73)
    x1, y1 = rng.uniform(-30, 300, size=31), rng.uniform(-30, 220, size=31)
    w, h = rng.uniform(3, 260, size=31), rng.uniform(3, 260, size=31)
    seeded = np.stack([x1, y1, x1 + w, y1 + h], 1)
    return np.concatenate([np.array(named), seeded]).astype(np.float32)


def e2e_boxes():
    """(boxes float32 [8, 4], frame index int32 [8]) of the end-to-end case: five on frame A (240 x 320), three on frame B (96 x 132); magnified, reduced,
    over a corner."""
    b = np.array([[40.0, 30.0, 160.0, 200.0], [100.5, 20.25, 300.0, 230.0], [-20.0, -15.0, 90.0, 120.0], [200.0, 100.0, 260.0, 180.0],
                  [10.0, 60.0, 70.0, 140.0], [20.0, 10.0, 100.0, 90.0], [60.0, 30.0, 140.0, 100.0], [5.5, 5.25, 60.0, 80.0]], dtype=np.float32)
    return b, np.array([0, 0, 0, 0, 0, 1, 1, 1], dtype=np.int32)
