"""One-Euro keypoint smoothing keyed by (stream, track id): the numpy twin of csrc/eurogeom.h (vp_smooth_update_stream on the device, vp_dbg_smooth_host on the
host).  The filter is the reference's ``post_processing/one_euro_filter.py`` in its fixed-rate mode (``OneEuroFilter(x0, fps=F)``, called with ``t_e`` in
frames); every expression below performs the reference's operations in the reference's order on float64 arrays, so the twin, the tap and the reference agree
bit for bit.  The ``restart`` policy for missing joints has no reference: this file pins it.
"""
from __future__ import annotations

import numpy as np

SLOTS = 128
FLAG_DUP, FLAG_FULL, FLAG_BAD_ROW = 1, 2, 8
MISSING = {'reference': 0, 'restart': 1}
TWO_PI = 2 * np.pi


class _Track:
    __slots__ = ('x_prev', 'dx_prev', 'fresh', 'last_seen')

    def __init__(self, x0: np.ndarray, frame: int):
        self.x_prev = x0.astype(np.float64)            # [K, 2] (y, x)
        self.dx_prev = np.zeros(x0.shape, np.float64)
        self.fresh = np.ones(x0.shape, bool)
        self.last_seen = frame


def one_euro_step(x: np.ndarray, t_e: float, trk: _Track, min_cutoff: float, beta: float, d_cutoff: float, missing: int) -> np.ndarray:
    """one update of the [K, 2] coordinates `x` (float32) of a track; -> the float64 x_hat (the caller rounds it to float32 once)"""
    x = np.asarray(x, np.float32)
    t_e = np.float64(t_e)
    x64 = x.astype(np.float64)
    # the reference's first call subtracts two float32 arrays; every later one a float64 state from the float32 input
    d = np.where(trk.fresh, (x - trk.x_prev.astype(np.float32)).astype(np.float64), x64 - trk.x_prev)
    dx = d / t_e
    r = (TWO_PI * np.float64(d_cutoff)) * t_e
    a_d = r / (r + 1)
    dx_hat = a_d * dx + (1 - a_d) * trk.dx_prev
    cutoff = np.float64(min_cutoff) + np.float64(beta) * np.abs(dx_hat)
    r = (TWO_PI * cutoff) * t_e
    a = r / (r + 1)
    x_hat = a * x64 + (1 - a) * trk.x_prev
    x_hat = np.where(x <= 0, -10.0, x_hat)
    fresh = np.zeros(x.shape, bool)
    if missing == 1:
        restart = trk.x_prev <= 0
        x_hat = np.where(restart, np.where(x <= 0, -10.0, x64), x_hat)
        dx_hat = np.where(restart, 0.0, dx_hat)
        fresh = restart
    trk.x_prev, trk.dx_prev, trk.fresh = x_hat, dx_hat, fresh
    return x_hat


class OneEuro:
    """``update(kpts[n, K, 3], ids[n], stream=None, rank=None, t_e=None, step_mask=None) -> (out[n, K, 3] float32, flags[n_streams] int32)``: the lifecycle of
    include/vitpose_hip.h (vp_smooth_update_stream) on a dict of per-(stream, id) states.  `slots` maps a live (stream, id) to its table slot, so that `state()`
    of the device can be compared field by field."""

    def __init__(self, n_joints: int, min_cutoff: float = 1.7, beta: float = 0.3, d_cutoff: float = 30.0, max_age: int = 1, n_streams: int = 1,
                 missing='reference'):
        self.K, self.min_cutoff, self.beta, self.d_cutoff = int(n_joints), float(min_cutoff), float(beta), float(d_cutoff)
        self.max_age, self.n_streams = int(max_age), int(n_streams)
        self.missing = MISSING[missing] if isinstance(missing, str) else int(missing)
        self.reset()

    def reset(self, streams=None):
        if streams is None:
            self.tracks, self.slots, self.frame_count = {}, {}, [0] * self.n_streams
            return
        for s in streams:
            self.frame_count[s] = 0
            for key in [k for k in self.tracks if k[0] == s]:
                del self.tracks[key], self.slots[key]

    def update(self, kpts, ids, stream=None, rank=None, t_e=None, step_mask=None):
        kpts = np.asarray(kpts, np.float32).reshape(-1, self.K, 3)
        ids = np.asarray(ids, np.int32).reshape(-1)
        n = len(ids)
        stream = np.zeros(n, np.int32) if stream is None else np.asarray(stream, np.int32).reshape(-1)
        t_e = np.ones(self.n_streams) if t_e is None else np.broadcast_to(np.asarray(t_e, np.float64), (self.n_streams,))
        if step_mask is None:
            stepped = range(self.n_streams)
        elif isinstance(step_mask, (int, np.integer)):
            stepped = [s for s in range(self.n_streams) if (int(step_mask) >> s) & 1]
        else:
            stepped = sorted(int(s) for s in step_mask)
        out = kpts.copy()
        flags = np.zeros(self.n_streams, np.int32)
        outside = bool(((ids >= 0) & ((stream < 0) | (stream >= self.n_streams))).any())
        for s in stepped:
            self.frame_count[s] += 1
            fc = self.frame_count[s]
            if outside:
                flags[s] |= FLAG_BAD_ROW
            for key in [k for k, t in self.tracks.items() if k[0] == s and fc - t.last_seen > self.max_age + 1]:
                del self.tracks[key], self.slots[key]
            for i in range(n):
                if stream[i] != s or ids[i] < 0 or (rank is not None and rank[i] < 0):
                    continue
                if not np.isfinite(kpts[i, :, :2]).all():
                    flags[s] |= FLAG_BAD_ROW
                    continue
                key = (s, int(ids[i]))
                trk = self.tracks.get(key)
                if trk is not None:
                    if trk.last_seen == fc:
                        flags[s] |= FLAG_DUP
                        continue
                    gap = fc - trk.last_seen
                    trk.last_seen = fc
                    out[i, :, :2] = one_euro_step(kpts[i, :, :2], t_e[s] * np.float64(gap), trk, self.min_cutoff, self.beta, self.d_cutoff,
                                                  self.missing).astype(np.float32)
                    continue
                used = {v for k, v in self.slots.items() if k[0] == s}
                free = [t for t in range(SLOTS) if t not in used]
                if not free:
                    flags[s] |= FLAG_FULL
                    continue
                self.tracks[key] = _Track(kpts[i, :, :2], fc)
                self.slots[key] = free[0]
        return out, flags
