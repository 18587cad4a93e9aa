"""Keypoint smoothing on the device (vp_smooth_update_stream; semantics in csrc/eurogeom.h, numpy twin ``smooth.OneEuro``): configuration, the ctypes layer and
the host model over the tap.

A ``DeviceSmoother`` holds the One-Euro filter state of every live track of ``n_streams`` cameras in device memory, keyed by (stream, track id).  ``update`` is
stream-ordered on torch's current stream and never synchronises: it takes the keypoints of ``VitPoseHip.infer_boxes``, the ids and streams of
``DeviceTracker.update`` and the NMS's rank, and its output passes to ``draw_poses``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import numbers

import numpy as np

from . import _capi as capi
from ._stage import DeviceStage, check_tensor, handle_alias, ptr
from .devtracker import TRACK_MAX_STREAMS, mask_of
from .smooth import FLAG_BAD_ROW, FLAG_DUP, FLAG_FULL, MISSING, SLOTS   # noqa: F401  (re-exported)

MAX_JOINTS = 1024
MAX_ROWS = 65536


def state_dtype(n_joints: int) -> np.dtype:
    """one stream's blob as csrc/eurogeom.h lays it out; zeroed = new, last_seen == 0 = the slot is free, the pair of every joint = (y, x)"""
    K = int(n_joints)
    return np.dtype([('frame_count', np.int32), ('pad', np.int32, 3), ('id', np.int32, SLOTS), ('last_seen', np.int32, SLOTS),
                     ('x_prev', np.float64, (SLOTS, K, 2)), ('dx_prev', np.float64, (SLOTS, K, 2)), ('fresh', np.uint8, (SLOTS, K, 2))])


STATE_DTYPE = state_dtype(17)   # the COCO-17 layout; `state_dtype(K)` for any other joint count


@dataclasses.dataclass(frozen=True)
class SmoothCfg:
    """``min_cutoff``, ``beta``, ``d_cutoff``: the One-Euro parameters (the reference's defaults); ``fps=F`` sets ``d_cutoff = F``, the reference's video mode, in
    which ``t_e`` counts frames; ``max_age``: stepped calls a track's filter survives without a row; ``n_streams``: independent tables; ``missing``:
    'reference' (after a masked joint the filter blends away from -10, as the reference does) or 'restart' (the joint starts afresh from its next sample);
    ``max_rows``: the most rows one call may carry (default 128 per stream)."""
    min_cutoff: float = 1.7
    beta: float = 0.3
    d_cutoff: float = 30.0
    fps: "float | None" = None
    max_age: int = 1
    n_streams: int = 1
    missing: str = 'reference'
    max_rows: "int | None" = None

    def __post_init__(self):
        def integer(v):
            return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))

        def real(v):
            return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_)) and math.isfinite(v)
        if self.fps is not None:
            if not (real(self.fps) and self.fps > 0):
                raise ValueError(f'SmoothCfg: fps finite and > 0 expected, got {self.fps!r}')
            object.__setattr__(self, 'd_cutoff', float(self.fps))
            object.__setattr__(self, 'fps', float(self.fps))
        if not (real(self.min_cutoff) and self.min_cutoff > 0):
            raise ValueError(f'SmoothCfg: min_cutoff finite and > 0 expected, got {self.min_cutoff!r}')
        if not (real(self.d_cutoff) and self.d_cutoff > 0):
            raise ValueError(f'SmoothCfg: d_cutoff finite and > 0 expected, got {self.d_cutoff!r}')
        if not (real(self.beta) and self.beta >= 0):
            raise ValueError(f'SmoothCfg: beta finite and >= 0 expected, got {self.beta!r}')
        if not (integer(self.max_age) and self.max_age >= 0):
            raise ValueError(f'SmoothCfg: max_age >= 0 expected, got {self.max_age!r}')
        if not (integer(self.n_streams) and 1 <= self.n_streams <= TRACK_MAX_STREAMS):
            raise ValueError(f'SmoothCfg: n_streams in 1..{TRACK_MAX_STREAMS} expected, got {self.n_streams!r}')
        if self.missing not in MISSING:
            raise ValueError(f"SmoothCfg: missing 'reference' or 'restart' expected, got {self.missing!r}")
        if self.max_rows is None:
            object.__setattr__(self, 'max_rows', SLOTS * int(self.n_streams))
        if not (integer(self.max_rows) and 1 <= self.max_rows <= MAX_ROWS):
            raise ValueError(f'SmoothCfg: max_rows in 1..{MAX_ROWS} expected, got {self.max_rows!r}')
        for name in ('min_cutoff', 'beta', 'd_cutoff'):
            object.__setattr__(self, name, float(getattr(self, name)))
        for name in ('max_age', 'n_streams', 'max_rows'):
            object.__setattr__(self, name, int(getattr(self, name)))


def c_config(cfg: SmoothCfg, n_joints: int):
    if not isinstance(cfg, SmoothCfg):
        raise TypeError(f'a SmoothCfg expected, got {type(cfg).__name__}')
    if not (isinstance(n_joints, numbers.Integral) and 1 <= n_joints <= MAX_JOINTS):
        raise ValueError(f'n_joints in 1..{MAX_JOINTS} expected, got {n_joints!r}')
    return capi.vp_smooth_cfg(cfg.min_cutoff, cfg.beta, cfg.d_cutoff, cfg.max_age, cfg.n_streams, int(n_joints), cfg.max_rows, MISSING[cfg.missing])


def state_bytes(c_cfg) -> int:
    b = C.c_int64(0)
    capi.check(capi.load_library().vp_smoother_state_bytes(C.byref(c_cfg), C.byref(b)))
    assert b.value == state_dtype(c_cfg.n_joints).itemsize * c_cfg.n_streams
    return b.value


def _host_args(K, n_streams, kpts, ids, stream, rank, t_e):
    kpts = np.ascontiguousarray(kpts, dtype=np.float32).reshape(-1, K, 3)
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    n = len(ids)
    if len(kpts) != n:
        raise ValueError(f'kpts: {n} rows expected (one per id), got {len(kpts)}')
    opt = []
    for name, a in (('stream', stream), ('rank', rank)):
        a = None if a is None else np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        if a is not None and len(a) != n:
            raise ValueError(f'{name}: {n} entries expected, got {len(a)}')
        opt.append(a)
    return kpts, ids, opt[0], opt[1], _te(t_e, n_streams)


def _te(t_e, n_streams):
    """None, one number for every stream, or one per stream -> a float64 [n_streams] array or None"""
    if t_e is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(t_e, dtype=np.float64), (n_streams,)))


class HostSmoother:
    """csrc/eurogeom.h on a host state blob through the tap vp_dbg_smooth_host: the model the device is tested against, never a fallback."""

    def __init__(self, n_joints: int, cfg: SmoothCfg = SmoothCfg()):
        self.cfg, self.K, self._c = cfg, int(n_joints), c_config(cfg, n_joints)
        self.lib = capi.load_library()
        self.blob = np.zeros(cfg.n_streams, state_dtype(n_joints))
        assert state_bytes(self._c) == self.blob.nbytes

    def state(self) -> np.ndarray:
        return self.blob

    def reset(self, streams=None):
        for s in range(self.cfg.n_streams):
            if (mask_of(streams, self.cfg.n_streams) >> s) & 1:
                self.blob[s] = np.zeros((), self.blob.dtype)

    def update(self, kpts, ids, stream=None, rank=None, t_e=None, step_mask=None):
        kpts, ids, stream, rank, te = _host_args(self.K, self.cfg.n_streams, kpts, ids, stream, rank, t_e)
        out, flags = np.empty_like(kpts), np.empty(self.cfg.n_streams, np.int32)
        capi.check(self.lib.vp_dbg_smooth_host(self.blob.ctypes.data, C.byref(self._c), ptr(kpts), ptr(ids), ptr(stream), ptr(rank), len(ids),
                                               mask_of(step_mask, self.cfg.n_streams), ptr(te), ptr(out), flags.ctypes.data))
        return out, flags


class DeviceSmoother(DeviceStage):
    _destroy, _s = 'vp_smoother_destroy', handle_alias

    def __init__(self, engine, n_joints: "int | None" = None, cfg: SmoothCfg = SmoothCfg()):
        super().__init__(engine)
        self.K = int(engine.K if n_joints is None else n_joints)
        self.cfg, self._c = cfg, c_config(cfg, self.K)
        self._create(self.lib.vp_smoother_create, C.byref(self._c))

    def update(self, kpts, ids, stream=None, rank=None, t_e=None, step_mask=None, out=None):
        """One step of the streams in `step_mask` (None: all) on torch's current stream, no synchronisation.  `kpts`: float32 CUDA [n, K, 3] rows of
        (y, x, conf), contiguous; `ids`, `stream` (None: stream 0), `rank` (None: none): int32 CUDA [n]; `t_e`: None (1.0), a number or one per stream (host);
        `out`: None (a new tensor), or a tensor like `kpts` -- `kpts` itself filters in place.  Returns (out, flags int32 [n_streams]) device tensors."""
        import torch
        dev = self._dev
        check_tensor('kpts', kpts, torch.float32, ('n', self.K, 3), dev, True)
        n = kpts.shape[0]
        check_tensor('ids', ids, torch.int32, (n,), dev, True)
        check_tensor('stream', stream, torch.int32, (n,), dev)
        check_tensor('rank', rank, torch.int32, (n,), dev)
        if out is None:
            out = torch.empty_like(kpts)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == dev and out.shape == kpts.shape and out.is_contiguous()):
            raise ValueError(f'out: a contiguous float32 tensor like kpts on {dev} expected')
        te = _te(t_e, self.cfg.n_streams)
        flags = torch.empty((self.cfg.n_streams,), dtype=torch.int32, device=dev)
        self._check(self.lib.vp_smooth_update_stream(self._obj, ptr(kpts, n), ptr(ids, n), ptr(stream, n), ptr(rank, n), n, mask_of(step_mask, self.cfg.n_streams), ptr(te),
                                                     ptr(out, n), flags.data_ptr(), self._stream()))
        return out, flags

    def update_host(self, kpts, ids, stream=None, rank=None, t_e=None, step_mask=None):
        """`update` on numpy arrays (vp_smooth_update: upload, the same kernels, download, synchronous) -> (out, flags)"""
        kpts, ids, stream, rank, te = _host_args(self.K, self.cfg.n_streams, kpts, ids, stream, rank, t_e)
        out, flags = np.empty_like(kpts), np.empty(self.cfg.n_streams, np.int32)
        self._check(self.lib.vp_smooth_update(self._obj, ptr(kpts), ptr(ids), ptr(stream), ptr(rank), len(ids), mask_of(step_mask, self.cfg.n_streams), ptr(te),
                                              ptr(out), flags.ctypes.data))
        return out, flags

    def reset(self, streams=None):
        """zero the tables of `streams` (None: all) on torch's current stream"""
        self._check(self.lib.vp_smoother_reset_stream(self._obj, mask_of(streams, self.cfg.n_streams), self._stream()))

    def state(self) -> np.ndarray:
        """the device state as a state_dtype(K) array [n_streams] (synchronous; for tests)"""
        out = np.zeros(self.cfg.n_streams, state_dtype(self.K))
        self._check(self.lib.vp_smoother_download_state(self._obj, out.ctypes.data))
        return out
