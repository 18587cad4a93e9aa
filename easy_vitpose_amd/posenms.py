"""Person scores and OKS pose NMS (vp_pose_nms_stream; semantics in csrc/posenms.h): the parameters and their ctypes form.

The reference keeps them in ``data_cfg`` (``soft_nms``, ``oks_thr=0.9``, ``vis_thr=0.2``) and ships one sigma table, the 17-joint COCO one inside
``oks_iou``; every other joint layout needs its sigmas given.
"""
from __future__ import annotations

import dataclasses
import math
import numbers

import numpy as np

from . import _capi as capi

NMS_MAX_PER_FRAME = 1024
NMS_MAX_K = 256
COCO17_SIGMAS = (.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089)


@dataclasses.dataclass(frozen=True)
class PoseNms:
    """``oks_thr``: poses with OKS above it against a kept pose are duplicates (hard) / the width of the score decay (``soft``);
    ``vis_thr``: joints at or below this confidence do not count (None: every joint does); ``max_dets``: picks per frame under ``soft``;
    ``sigmas``: one per joint (None: the COCO-17 table, for that layout only)."""
    oks_thr: float = 0.9
    vis_thr: float | None = 0.2
    soft: bool = False
    max_dets: int = 20
    sigmas: tuple | None = None

    def __post_init__(self):
        def number(v):   # Python and numpy real scalars; a bool is not a threshold
            return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_))
        if not (number(self.oks_thr) and 0.0 < float(self.oks_thr) <= 1.0):
            raise ValueError(f'PoseNms: oks_thr in (0, 1] expected, got {self.oks_thr!r}')
        object.__setattr__(self, 'oks_thr', float(self.oks_thr))
        if self.vis_thr is not None:
            if not (number(self.vis_thr) and math.isfinite(self.vis_thr)):
                raise ValueError(f'PoseNms: vis_thr is a finite number or None, got {self.vis_thr!r}')
            object.__setattr__(self, 'vis_thr', float(self.vis_thr))
        if not (number(self.max_dets) and int(self.max_dets) == self.max_dets and self.max_dets >= 1):
            raise ValueError(f'PoseNms: max_dets >= 1 expected, got {self.max_dets!r}')
        object.__setattr__(self, 'max_dets', int(self.max_dets))
        object.__setattr__(self, 'soft', bool(self.soft))
        if self.sigmas is not None:
            s = tuple(float(v) for v in self.sigmas)
            if not s or len(s) > NMS_MAX_K or not all(math.isfinite(v) and v > 0.0 for v in s):
                raise ValueError(f'PoseNms: sigmas are 1..{NMS_MAX_K} finite values > 0')
            object.__setattr__(self, 'sigmas', s)


def resolve_sigmas(dataset, K: int, sigmas=None) -> np.ndarray:
    """The float32 sigma table of a `K`-joint model of `dataset`.  None stands for the COCO-17 table and is accepted for that layout only;
    any other dataset needs its sigmas given (the policy of configs.resolve_flip_pairs)."""
    if sigmas is None:
        if dataset != 'coco' or K != 17:
            raise ValueError(f'pose NMS: the built-in sigmas are those of the 17-joint COCO layout; dataset {dataset!r} with {K} joints needs '
                             'its own: PoseNms(sigmas=[...]), one per joint')
        sigmas = COCO17_SIGMAS
    a = np.ascontiguousarray(np.asarray(sigmas, dtype=np.float64).reshape(-1), dtype=np.float32)
    if a.size != K:
        raise ValueError(f'pose NMS: {a.size} sigmas for the {K} joints of dataset {dataset!r}')
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError('pose NMS: sigmas must be finite and > 0')
    return a


def c_config(cfg: PoseNms, sigmas: np.ndarray):
    """(vp_pose_nms_cfg, the array its pointer reads: keep it alive for the call)"""
    if not isinstance(cfg, PoseNms):
        raise TypeError(f'a PoseNms expected, got {type(cfg).__name__}')
    s = np.ascontiguousarray(sigmas, dtype=np.float32)
    c = capi.vp_pose_nms_cfg(float(cfg.oks_thr), float(cfg.vis_thr if cfg.vis_thr is not None else 0.0), int(cfg.vis_thr is not None),
                             int(bool(cfg.soft)), int(cfg.max_dets), int(s.size), s.ctypes.data)
    return c, s


def load_sigmas(path: str) -> tuple:
    """a JSON file holding one list of numbers (the CLI's --sigmas)"""
    import json
    with open(path) as f:
        v = json.load(f)
    if not isinstance(v, list) or not all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in v):
        raise ValueError(f'{path}: a JSON list of numbers expected')
    return tuple(float(x) for x in v)
