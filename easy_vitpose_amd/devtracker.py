"""The box tracker on the device (vp_tracker_update_stream; semantics in csrc/sortgeom.h, Python twin ``tracker.Sort``): configuration, the ctypes layer, and
``DeviceSort``, the drop-in for ``VitInference(tracker=...)``.

A ``DeviceTracker`` holds ``n_streams`` independent SORT states in device memory (one per camera).  ``update`` is stream-ordered on torch's current stream and
never synchronises: the rows it returns pass in place to ``VitPoseHip.infer_boxes(rows, frame_index=stream)``, ``pose_nms(box_scores=rows[:, 4])`` and
``draw_poses(ids=ids)``.  Rows beyond the report are "absent" (box NaN, score 0, id -1, stream -1): the boxes entry gives them status 1 and zero keypoints, the
NMS rank -1.
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import math
import numbers

import numpy as np

from . import _capi as capi
from ._stage import DeviceStage, check_tensor, handle_alias

TRACK_MAX = 128
TRACK_MAX_STREAMS = 64
FLAG_DETS, FLAG_BIRTHS, FLAG_ROWS, FLAG_BAD_ROW = 1, 2, 4, 8

# csrc/sortgeom.h TrkStream
TRACK_DTYPE = np.dtype([('x', np.float64, 7), ('P', np.float64, (7, 7)), ('score', np.float64), ('id', np.int32), ('time_since_update', np.int32),
                        ('hit_streak', np.int32), ('hits', np.int32), ('age', np.int32), ('pad', np.int32)])
STATE_DTYPE = np.dtype([('n_tracks', np.int32), ('frame_count', np.int32), ('next_id', np.int32), ('n_rows', np.int32), ('flags', np.int32), ('pad', np.int32, 3),
                        ('tracks', TRACK_DTYPE, TRACK_MAX), ('rows', np.float64, (TRACK_MAX, 5)), ('row_ids', np.int32, TRACK_MAX)])


@dataclasses.dataclass(frozen=True)
class TrackCfg:
    """``max_age``: calls a track survives without a match; ``min_hits``: consecutive matches before a track is reported (once the stream is older than that);
    ``iou_threshold``: pairs below it are not matches (float32 on the device); ``n_streams``: independent SORT states."""
    max_age: int = 1
    min_hits: int = 3
    iou_threshold: float = 0.3
    n_streams: int = 1

    def __post_init__(self):
        def integer(v):
            return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))
        if not (integer(self.max_age) and self.max_age >= 0):
            raise ValueError(f'TrackCfg: max_age >= 0 expected, got {self.max_age!r}')
        if not (integer(self.min_hits) and self.min_hits >= 0):
            raise ValueError(f'TrackCfg: min_hits >= 0 expected, got {self.min_hits!r}')
        if not (integer(self.n_streams) and 1 <= self.n_streams <= TRACK_MAX_STREAMS):
            raise ValueError(f'TrackCfg: n_streams in 1..{TRACK_MAX_STREAMS} expected, got {self.n_streams!r}')
        t = self.iou_threshold
        if not (isinstance(t, numbers.Real) and not isinstance(t, (bool, np.bool_)) and math.isfinite(t) and 0.0 < float(np.float32(t)) < 1.0):
            raise ValueError(f'TrackCfg: iou_threshold in (0, 1) expected, got {t!r}')
        object.__setattr__(self, 'max_age', int(self.max_age))
        object.__setattr__(self, 'min_hits', int(self.min_hits))
        object.__setattr__(self, 'n_streams', int(self.n_streams))
        object.__setattr__(self, 'iou_threshold', float(np.float32(t)))   # the value the device compares with


def c_config(cfg: TrackCfg):
    if not isinstance(cfg, TrackCfg):
        raise TypeError(f'a TrackCfg expected, got {type(cfg).__name__}')
    return capi.vp_track_cfg(cfg.max_age, cfg.min_hits, cfg.iou_threshold, cfg.n_streams)


def state_bytes(n_streams: int) -> int:
    b = C.c_int64(0)
    capi.check(capi.load_library().vp_tracker_state_bytes(int(n_streams), C.byref(b)))
    assert b.value == STATE_DTYPE.itemsize * n_streams
    return b.value


def mask_of(step, n_streams: int) -> int:
    """a step / reset argument as the C mask: None = every stream, an int = the mask itself, else an iterable of stream indices"""
    if step is None:
        return (1 << n_streams) - 1
    if isinstance(step, numbers.Integral) and not isinstance(step, (bool, np.bool_)):
        m = int(step)
    else:
        m = 0
        for s in step:
            if not 0 <= int(s) < TRACK_MAX_STREAMS:
                raise ValueError(f'stream {s} outside 0..{TRACK_MAX_STREAMS - 1}')
            m |= 1 << int(s)
    if m < 0 or m >> n_streams:
        raise ValueError(f'a stream beyond n_streams = {n_streams} in {step!r}')
    return m


class RowBound:
    """The host-side bound on a call's report rows, kept without a synchronisation.  One stream: a call with detections reports only tracks matched or born in
    it, at most ``n_dets`` rows (rows the device skips as non-finite still count here; if ALL of a call's rows are skipped the call coasts and flag 4 tells);
    an empty call reports every listed track, those have ``time_since_update <= max_age + 1``, so each was matched or born in one of the last ``max_age + 2``
    calls (this one included): the sum of their ``n_dets``, capped at TRACK_MAX.  Several streams: the host does not know which stream a device row names, so a
    stream may coast in any call: the sum over that window whatever ``n_dets``, capped at TRACK_MAX per stepped stream -- and the cap alone as long as a call of the
    window stepped only some of the streams, or some of the streams were reset within it (a stream that is not stepped does not age, and the streams a partial
    reset leaves alone keep their tracks).  ``bound`` asks, ``push`` records a call, ``reset`` records a reset."""

    def __init__(self, max_age: int, n_streams: int = 1):
        self.n_streams = n_streams
        self._last = collections.deque(maxlen=max_age + 2)   # (n_dets, every stream stepped) per recorded call, a partial reset as (0, False)

    def bound(self, n_dets: int, stepped=None) -> int:
        """the bound for a call of `n_dets` rows that steps `stepped` streams (None: all), as if it came next; nothing is recorded"""
        stepped = self.n_streams if stepped is None else int(stepped)
        window = list(self._last)[-(self._last.maxlen - 1):]   # the last max_age + 1 records: with this call, max_age + 2
        window.append((int(n_dets), stepped == self.n_streams))
        cap = TRACK_MAX * stepped
        if not all(full for _, full in window):
            return cap
        if self.n_streams == 1 and n_dets > 0:
            return int(n_dets)
        return min(sum(n for n, _ in window), cap)

    def push(self, n_dets: int, stepped=None) -> int:
        b = self.bound(n_dets, stepped)
        self._last.append((int(n_dets), (self.n_streams if stepped is None else int(stepped)) == self.n_streams))
        return b

    def reset(self, n_reset=None):
        """every stream reset: nothing is listed any more; some: the others keep their tracks, so the cap holds until this leaves the window"""
        if n_reset is None or int(n_reset) >= self.n_streams:
            self._last.clear()
        elif int(n_reset) > 0:
            self._last.append((0, False))


class HostTracker:
    """csrc/sortgeom.h on a host state blob through the tap vp_dbg_track_host: the model the device is tested against, never a fallback."""

    def __init__(self, cfg: TrackCfg):
        self.cfg, self._c = cfg, c_config(cfg)
        self.lib = capi.load_library()
        self.blob = np.zeros(cfg.n_streams, STATE_DTYPE)
        assert state_bytes(cfg.n_streams) == self.blob.nbytes

    def state(self) -> np.ndarray:
        return self.blob

    def update(self, dets, frame_index=None, n_out=None, step=None):
        dets, fi = _host_args(dets, frame_index)
        n_out = TRACK_MAX * self.cfg.n_streams if n_out is None else int(n_out)
        out = _host_out(max(n_out, 0), self.cfg.n_streams)
        capi.check(self.lib.vp_dbg_track_host(self.blob.ctypes.data, C.byref(self._c), dets.ctypes.data if dets.size else None, dets.shape[1] if dets.ndim == 2 else 5,
                                              None if fi is None else fi.ctypes.data, len(dets), mask_of(step, self.cfg.n_streams), *[a.ctypes.data for a in out[:3]],
                                              n_out, out[3].ctypes.data, out[4].ctypes.data))
        return out


def _host_args(dets, frame_index):
    dets = np.ascontiguousarray(dets, dtype=np.float32)
    if dets.ndim != 2 or dets.shape[1] < 5:
        dets = dets.reshape(-1, 5)
    fi = None if frame_index is None else np.ascontiguousarray(frame_index, dtype=np.int32).reshape(-1)
    if fi is not None and len(fi) != len(dets):
        raise ValueError(f'frame_index: {len(dets)} entries expected, got {len(fi)}')
    return dets, fi


def _host_out(n_out: int, n_streams: int):
    return (np.empty((n_out, 6), np.float32), np.empty(n_out, np.int32), np.empty(n_out, np.int32), np.empty(n_streams + 1, np.int32), np.empty(n_streams, np.int32))


class DeviceTracker(DeviceStage):
    _destroy, _t = 'vp_tracker_destroy', handle_alias

    def __init__(self, engine, cfg: TrackCfg = TrackCfg()):
        super().__init__(engine)
        self.cfg, self._c = cfg, c_config(cfg)
        self._create(self.lib.vp_tracker_create, C.byref(self._c))
        self._bound = RowBound(cfg.max_age, cfg.n_streams)

    def row_bound(self, n_dets: int, step=None) -> int:
        """the bound on the report rows of the NEXT call, given its detection count and step argument: what `update` takes for `n_out` when none is given.  A
        query: it records nothing (`update` / `update_host` record every call themselves, whatever `n_out` they are given), so sizing a buffer with it first is safe.
        With one stream and detections the bound is `n_dets`; should EVERY row of such a call be non-finite, the device skips them all, the stream coasts and
        reports its listed tracks, and rows beyond `n_dets` are cut under flag 4."""
        return self._bound.bound(n_dets, bin(mask_of(step, self.cfg.n_streams)).count('1'))

    def update(self, dets, frame_index=None, n_out=None, step=None, n_dets=None):
        """One step of the streams in `step` (None: all) on torch's current stream, no synchronisation.  `dets`: float32 CUDA [n, >= 5] rows
        (x1, y1, x2, y2, score, ...), row-contiguous; `frame_index`: int32 CUDA [n] (None: stream 0).  Returns (rows float32 [n_out, 6], ids int32 [n_out],
        stream int32 [n_out], count int32 [n_streams + 1], flags int32 [n_streams]) device tensors; n_out defaults to `row_bound(n, step)` (see there for the one
        input it does not cover: a one-stream call whose rows are ALL non-finite).  Every call is recorded for the bound, with or without an `n_out`.
        `n_dets`: an int32 CUDA tensor of one element, the detection count decided on the device (vp_tracker_update_counted_stream): only the first
        min(n_dets, n) rows are read -- the detector stage's rows, image and count[-1:] pass in place; the bound is recorded with n."""
        import torch
        dev = self._dev
        if not (isinstance(dets, torch.Tensor) and dets.is_cuda and dets.dtype == torch.float32):
            raise TypeError('dets: a float32 torch CUDA tensor expected')
        if dets.device != dev or dets.ndim != 2 or dets.shape[1] < 5 or (dets.shape[0] > 0 and dets.stride(1) != 1):
            raise ValueError(f'dets: [n, >= 5] with contiguous rows on {dev} expected, got {tuple(dets.shape)} on {dets.device}')
        n = dets.shape[0]
        check_tensor('frame_index', frame_index, torch.int32, (n,), dev)
        mask = mask_of(step, self.cfg.n_streams)
        n_out = self.row_bound(n, mask) if n_out is None else int(n_out)
        if n_out < 0:
            raise ValueError('n_out < 0')
        ns = self.cfg.n_streams
        rows = torch.empty((n_out, 6), dtype=torch.float32, device=dev)
        ids = torch.empty((n_out,), dtype=torch.int32, device=dev)
        stream = torch.empty((n_out,), dtype=torch.int32, device=dev)
        count = torch.empty((ns + 1,), dtype=torch.int32, device=dev)
        flags = torch.empty((ns,), dtype=torch.int32, device=dev)
        io = (dets.data_ptr() if n else None, dets.stride(0) if n > 1 else max(dets.shape[1], 5), None if frame_index is None or n == 0 else frame_index.data_ptr(), n)
        out = (mask, rows.data_ptr(), ids.data_ptr(), stream.data_ptr(), n_out, count.data_ptr(), flags.data_ptr(), self._stream())
        if n_dets is None:
            self._check(self.lib.vp_tracker_update_stream(self._obj, *io, *out))
        else:
            if not (isinstance(n_dets, torch.Tensor) and n_dets.is_cuda and n_dets.dtype == torch.int32):
                raise TypeError('n_dets: an int32 torch CUDA tensor expected')
            if n_dets.device != dev or n_dets.numel() != 1:
                raise ValueError(f'n_dets: one element on {dev} expected')
            self._check(self.lib.vp_tracker_update_counted_stream(self._obj, *io, n_dets.data_ptr(), *out))
        self._bound.push(n, bin(mask).count('1'))
        return rows, ids, stream, count, flags

    def update_host(self, dets, frame_index=None, n_out=None, step=None):
        """`update` on numpy arrays (vp_tracker_update: upload, the same kernels, download, synchronous)."""
        dets, fi = _host_args(dets, frame_index)
        mask = mask_of(step, self.cfg.n_streams)
        n_out = self.row_bound(len(dets), mask) if n_out is None else int(n_out)
        out = _host_out(max(n_out, 0), self.cfg.n_streams)
        self._check(self.lib.vp_tracker_update(self._obj, dets.ctypes.data if dets.size else None, dets.shape[1], None if fi is None else fi.ctypes.data, len(dets),
                                               mask, *[a.ctypes.data for a in out[:3]], n_out, out[3].ctypes.data, out[4].ctypes.data))
        self._bound.push(len(dets), bin(mask).count('1'))
        return out

    def reset(self, streams=None):
        """zero the state of `streams` (None: all) on torch's current stream: their ids restart at 1"""
        mask = mask_of(streams, self.cfg.n_streams)
        self._check(self.lib.vp_tracker_reset_stream(self._obj, mask, self._stream()))
        self._bound.reset(bin(mask).count('1'))

    def state(self) -> np.ndarray:
        """the device state as a STATE_DTYPE array [n_streams] (synchronous; for tests)"""
        out = np.zeros(self.cfg.n_streams, STATE_DTYPE)
        self._check(self.lib.vp_tracker_download_state(self._obj, out.ctypes.data))
        return out


class DeviceSort:
    """``tracker.Sort``'s interface on the device tracker through the synchronous twin: ``update(dets[n, 5]) -> [m, 6]`` float64 (x1, y1, x2, y2, score, id).
    The boxes are the float32 rows of the device entry."""

    def __init__(self, engine, max_age: int = 1, min_hits: int = 3, iou_threshold: float = 0.3):
        self.max_age, self.min_hits, self.iou_threshold = max_age, min_hits, iou_threshold
        self.device_tracker = DeviceTracker(engine, TrackCfg(max_age, min_hits, iou_threshold, 1))

    def update(self, dets=np.empty((0, 5))) -> np.ndarray:
        dets = np.asarray(dets, dtype=np.float64).reshape(-1, 5)
        rows, _, _, count, _ = self.device_tracker.update_host(dets)
        return rows[:int(count[-1])].astype(np.float64)
