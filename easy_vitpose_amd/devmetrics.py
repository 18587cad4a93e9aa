"""Accuracy metrics against ground truth on the device (vp_metrics_*; semantics and summation order in csrc/metricsgeom.h): configuration, the state layout, the
numpy twin, the host tap, the device object and the finisher.

A ``DeviceMetrics`` is an accumulating stage with the life cycle of the tracker and the smoother: ``update`` adds the rows of one call -- predictions and ground
truth that already lie on the GPU -- to per-joint counts and sums on torch's current stream and never synchronises; ``result()`` reads the state once at the end
and ``finish`` turns it into the reference's figures (``vit_utils/top_down_eval.py`` keypoint_pck_accuracy / keypoint_auc / keypoint_epe / keypoint_nme on the
concatenated data set) from counts alone.  The OKS figures are the share of instances recovered at OKS t with one candidate per instance, not COCO AP.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import numbers

import numpy as np

from . import _capi as capi
from ._stage import DeviceStage, check_tensor, handle_alias, ptr
from .posenms import COCO17_SIGMAS, NMS_MAX_K

MAX_ROWS = 8192
BLOCK = 64
MAX_PCK, MAX_AUC, OKS_THRS = 8, 32, 10
F32, F64 = np.float32, np.float64


@dataclasses.dataclass(frozen=True)
class MetricsCfg:
    """``n_joints``; ``pck_thr``: up to 8 PCK thresholds on the normalised distance; ``auc_steps`` / ``auc_norm``: keypoint_auc's num_step (0: no AUC) and its
    scalar normaliser; ``vis_thr``: a ground-truth joint counts when its third column is above it; ``sigmas``: one per joint switches the OKS figures on ('coco'
    = the COCO-17 table, for 17 joints only)."""
    n_joints: int = 17
    pck_thr: tuple = (0.05, 0.1, 0.2)
    auc_steps: int = 20
    auc_norm: float = 30.0
    vis_thr: float = 0.0
    sigmas: "tuple | str | None" = None

    def __post_init__(self):
        def integer(v):
            return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))

        def real(v):
            return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_)) and math.isfinite(v)
        if not (integer(self.n_joints) and 1 <= self.n_joints <= NMS_MAX_K):
            raise ValueError(f'MetricsCfg: n_joints in 1..{NMS_MAX_K} expected, got {self.n_joints!r}')
        thr = tuple(self.pck_thr)
        if len(thr) > MAX_PCK or not all(real(t) for t in thr):
            raise ValueError(f'MetricsCfg: pck_thr holds up to {MAX_PCK} finite numbers, got {self.pck_thr!r}')
        if not (integer(self.auc_steps) and 0 <= self.auc_steps <= MAX_AUC):
            raise ValueError(f'MetricsCfg: auc_steps in 0..{MAX_AUC} expected, got {self.auc_steps!r}')
        if self.auc_steps > 0 and not (real(self.auc_norm) and self.auc_norm > 0):
            raise ValueError(f'MetricsCfg: auc_norm finite and > 0 expected, got {self.auc_norm!r}')
        if not real(self.vis_thr):
            raise ValueError(f'MetricsCfg: vis_thr is a finite number, got {self.vis_thr!r}')
        sig = self.sigmas
        if isinstance(sig, str):
            if sig != 'coco' or self.n_joints != 17:
                raise ValueError("MetricsCfg: sigmas='coco' names the COCO-17 table, for n_joints = 17 only")
            sig = COCO17_SIGMAS
        if sig is not None:
            sig = tuple(float(v) for v in sig)
            if len(sig) != self.n_joints or not all(math.isfinite(v) and v > 0.0 for v in sig):
                raise ValueError(f'MetricsCfg: sigmas are {self.n_joints} finite values > 0')
        object.__setattr__(self, 'n_joints', int(self.n_joints))
        object.__setattr__(self, 'pck_thr', tuple(float(t) for t in thr))
        object.__setattr__(self, 'auc_steps', int(self.auc_steps))
        object.__setattr__(self, 'auc_norm', float(self.auc_norm))
        object.__setattr__(self, 'vis_thr', float(self.vis_thr))
        object.__setattr__(self, 'sigmas', sig)

    @property
    def use_oks(self) -> bool:
        return self.sigmas is not None


def c_config(cfg: MetricsCfg):
    """(vp_metrics_cfg, the float32 sigma array or None: keep it alive for the call)"""
    if not isinstance(cfg, MetricsCfg):
        raise TypeError(f'a MetricsCfg expected, got {type(cfg).__name__}')
    thr = (C.c_float * 8)(*cfg.pck_thr)
    c = capi.vp_metrics_cfg(cfg.auc_norm, thr, cfg.vis_thr, cfg.n_joints, len(cfg.pck_thr), cfg.auc_steps, int(cfg.use_oks), 0)
    sig = np.ascontiguousarray(cfg.sigmas, dtype=F32) if cfg.use_oks else None
    return c, sig


def state_dtype(cfg: MetricsCfg) -> np.dtype:
    """the state blob as csrc/metricsgeom.h lays it out (8-byte words; zeroed = new)"""
    K, P, A = cfg.n_joints, len(cfg.pck_thr), cfg.auc_steps
    return np.dtype([('calls', np.int64), ('rows', np.int64), ('counted', np.int64), ('nonfinite', np.int64), ('oks_rows', np.int64), ('pad0', np.int64, 3),
                     ('oks_hits', np.int64, OKS_THRS), ('oks_sum', F64), ('pad1', np.int64, 5),
                     ('valid_norm', np.int64, K), ('valid_px', np.int64, K), ('sum_norm', F64, K), ('sum_px', F64, K),
                     ('pck_hits', np.int64, (P, K)), ('auc_hits', np.int64, (A, K))])


def new_state(cfg: MetricsCfg) -> np.ndarray:
    return np.zeros((), state_dtype(cfg))


def state_bytes(cfg: MetricsCfg) -> int:
    c, _ = c_config(cfg)
    b = C.c_int64(0)
    capi.check(capi.load_library().vp_metrics_state_bytes(C.byref(c), C.byref(b)))
    assert b.value == state_dtype(cfg).itemsize == 8 * (24 + cfg.n_joints * (4 + len(cfg.pck_thr) + cfg.auc_steps))
    return b.value


def norm_from_boxes(rows) -> np.ndarray:
    """(h, w) of tracker / detector rows (x1, y1, x2, y2, ...) as the float32 [n, 2] normaliser, in (y, x) order like the coordinates"""
    r = np.asarray(rows, dtype=F32).reshape(len(rows), -1)
    return np.ascontiguousarray(np.stack([r[:, 3] - r[:, 1], r[:, 2] - r[:, 0]], axis=1), dtype=F32)


def _host_args(K, pred, gt, norm, area, rank, set_):
    pred = np.ascontiguousarray(pred, dtype=F32).reshape(-1, K, 3)
    gt = np.ascontiguousarray(gt, dtype=F32).reshape(-1, K, 3)
    n = len(pred)
    if len(gt) != n:
        raise ValueError(f'gt: {n} rows expected (one per prediction), got {len(gt)}')
    out = []
    for name, a, dt, shape in (('norm', norm, F32, (n, 2)), ('area', area, F32, (n,)), ('rank', rank, np.int32, (n,)), ('set', set_, np.int32, (n,))):
        a = None if a is None else np.ascontiguousarray(a, dtype=dt)
        if a is not None and a.shape != shape:
            raise ValueError(f'{name}: shape {shape} expected, got {a.shape}')
        out.append(a)
    return (pred, gt, *out)


_exp = np.frompyfunc(math.exp, 1, 1)   # the C library's exp, element by element: what the host tap calls (numpy's own exp is another implementation)


def _tree64(leaves):
    """[blocks, 64, ...] -> [blocks, ...]: the balanced tree over the 64 rows of a block in row order (pairs at distance 1, then 2, ..., 32)"""
    a = leaves
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def _call_sum(leaves):
    """((0.0 + P(0)) + P(1)) + ... over the blocks in ascending order"""
    parts = _tree64(leaves)
    s = np.zeros(parts.shape[1:], F64)
    for b in range(len(parts)):
        s = s + parts[b]
    return s


def metrics_numpy(state: np.ndarray, cfg: MetricsCfg, pred, gt, norm=None, area=None, rank=None, set=None, set_value=0):
    """One update in numpy, the same bytes as the tap: adds the call to `state` (a state_dtype(cfg) scalar array, in place) and returns (dist [n, K], oks [n])."""
    K = cfg.n_joints
    pred, gt, norm, area, rank, set_ = _host_args(K, pred, gt, norm, area, rank, set)
    n = len(pred)
    nb = -(-n // BLOCK)
    counted = np.ones(n, bool)
    if rank is not None:
        counted &= rank >= 0
    if set_ is not None:
        counted &= set_ == np.int32(set_value)
    with np.errstate(all='ignore'):
        vis = counted[:, None] & (gt[:, :, 2] > F32(cfg.vis_thr))
        nrm = np.ones((n, 2), F32) if norm is None else norm.copy()
        on = ~(nrm == 0).any(axis=1)
        nrm[nrm <= 0] = F32(1e6)
        in_norm = vis & on[:, None]
        dy, dx = pred[:, :, 0] - gt[:, :, 0], pred[:, :, 1] - gt[:, :, 1]
        ry, rx = dy / nrm[:, 0:1], dx / nrm[:, 1:2]
        qn = np.sqrt(ry * ry + rx * rx)
        q1 = np.sqrt(dy * dy + dx * dx)
        assert qn.dtype == F32 and q1.dtype == F32
        st = state
        st['calls'] += 1
        st['rows'] += n
        st['counted'] += int(counted.sum())
        st['valid_norm'] += in_norm.sum(axis=0)
        st['valid_px'] += vis.sum(axis=0)
        for t, thr in enumerate(cfg.pck_thr):
            st['pck_hits'][t] += (in_norm & (qn < F32(thr))).sum(axis=0)
        if cfg.auc_steps > 0:
            A = F64(cfg.auc_norm)
            ay, ax = dy.astype(F64) / A, dx.astype(F64) / A
            qa = np.sqrt(ay * ay + ax * ax).astype(F32)
            for s in range(cfg.auc_steps):
                st['auc_hits'][s] += (vis & (qa < F32(s / cfg.auc_steps))).sum(axis=0)
        fn, f1 = in_norm & np.isfinite(qn), vis & np.isfinite(q1)
        nonfinite = int((in_norm & ~fn).sum()) + int((vis & ~f1).sum())
        leaves = np.zeros((nb * BLOCK, 2, K), F64)
        leaves[:n, 0] = np.where(fn, qn, F32(0)).astype(F64)
        leaves[:n, 1] = np.where(f1, q1, F32(0)).astype(F64)
        s = _call_sum(leaves.reshape(nb, BLOCK, 2, K))
        st['sum_norm'] = st['sum_norm'] + s[0]
        st['sum_px'] = st['sum_px'] + s[1]
        dist = np.where(in_norm, qn, F32(-1)).astype(F32)
        oks = np.full(n, -1, F32)
        if cfg.use_oks and area is not None:
            a = area.astype(F64)
            row = counted & np.isfinite(a) & (a > 0) & vis.any(axis=1)
            var = (2.0 * np.asarray(cfg.sigmas, F32).astype(F64)) ** 2
            denom = (a + a) / 2.0 + 2.220446049250313e-16
            d2 = (dx * dx + dy * dy).astype(F64)
            e = d2 / var[None, :] / denom[:, None] / 2.0
            use = vis & row[:, None]
            term = np.zeros((n, K), F64)
            term[use] = _exp(-e[use]).astype(F64)
            tot, cnt = np.zeros(n, F64), np.zeros(n, np.int64)
            for j in range(K):   # joint order
                tot = np.where(use[:, j], tot + term[:, j], tot)
                cnt += use[:, j]
            val = (tot / np.maximum(cnt, 1)).astype(F32)
            oks[row] = val[row]
            okf = row & np.isfinite(val)
            nonfinite += int((row & ~okf).sum())
            st['oks_rows'] += int(okf.sum())
            for t in range(OKS_THRS):
                st['oks_hits'][t] += int((okf & (val >= F32(0.5 + 0.05 * t))).sum())
            leaf = np.zeros(nb * BLOCK, F64)
            leaf[:n] = np.where(okf, val, F32(0)).astype(F64)
            st['oks_sum'] = st['oks_sum'] + _call_sum(leaf.reshape(nb, BLOCK))
        st['nonfinite'] += nonfinite
    return dist, oks


def metrics_tap(state: np.ndarray, cfg: MetricsCfg, pred, gt, norm=None, area=None, rank=None, set=None, set_value=0, dist=None, oks=None):
    """One update through the host tap vp_dbg_metrics_host: the model the device is tested against, never a fallback.  Adds the call to `state` in place and
    returns (dist [n, K], oks [n]) -- arrays the caller passed in, or new ones."""
    K = cfg.n_joints
    pred, gt, norm, area, rank, set_ = _host_args(K, pred, gt, norm, area, rank, set)
    n = len(pred)
    c, sig = c_config(cfg)
    assert state.dtype == state_dtype(cfg) and state.flags.c_contiguous
    dist = np.empty((n, K), F32) if dist is None else dist
    oks = np.empty(n, F32) if oks is None else oks
    capi.check(capi.load_library().vp_dbg_metrics_host(state.ctypes.data, C.byref(c), ptr(sig), ptr(pred), ptr(gt), ptr(norm), ptr(area), ptr(rank), ptr(set_),
                                                       int(set_value), n, ptr(dist), ptr(oks)))
    return dist, oks


@dataclasses.dataclass(frozen=True)
class MetricsResult:
    """The figures of a state.  ``pck(t)`` -> (acc [K] float64 with -1 where a joint has no valid sample, avg = the mean of the acc >= 0 or 0, cnt), as
    keypoint_pck_accuracy returns them on the concatenated data set; ``auc``; ``epe`` / ``nme`` (NaN when a non-finite distance was left out of the sum: the
    reference would report inf or NaN); ``oks_mean``, ``oks_recall`` [10] at 0.50:0.05:0.95 (NaN without an OKS row); the counters."""
    cfg: MetricsCfg
    state: np.ndarray
    auc: float
    epe: float
    nme: float
    oks_mean: float
    oks_recall: np.ndarray
    calls: int
    rows: int
    counted: int
    nonfinite: int
    oks_rows: int

    def pck(self, t: int):
        return _acc(self.state['pck_hits'][t], self.state['valid_norm'])


def _acc(hits, valid):
    acc = np.full(len(valid), -1.0, F64)
    ok = valid > 0
    acc[ok] = hits[ok] / valid[ok]          # int64 / int64 -> float64, as (d < thr).sum() / num_distance_valid
    sel = acc[acc >= 0]
    cnt = len(sel)
    return acc, (sel.mean() if cnt > 0 else 0), cnt


def finish(state: np.ndarray, cfg: MetricsCfg) -> MetricsResult:
    """restates the reference on the concatenated data set from counts alone"""
    st = state
    auc = 0
    for s in range(cfg.auc_steps):          # keypoint_auc: added sequentially in s
        auc += 1.0 / cfg.auc_steps * _acc(st['auc_hits'][s], st['valid_px'])[1]
    bad = int(st['nonfinite']) > 0
    epe = math.nan if bad else float(math.fsum(st['sum_px']) / max(1, int(st['valid_px'].sum())))
    nme = math.nan if bad else float(math.fsum(st['sum_norm']) / max(1, int(st['valid_norm'].sum())))
    rows = int(st['oks_rows'])
    return MetricsResult(cfg, st.copy(), float(auc), epe, nme, float(st['oks_sum'] / rows) if rows else math.nan,
                         st['oks_hits'] / rows if rows else np.full(OKS_THRS, np.nan), int(st['calls']), int(st['rows']), int(st['counted']),
                         int(st['nonfinite']), rows)


def parse_state(raw, cfg: MetricsCfg) -> np.ndarray:
    """the bytes of a snapshot (a numpy uint8 array) as a state_dtype(cfg) scalar array"""
    return np.frombuffer(np.ascontiguousarray(raw, dtype=np.uint8).tobytes(), dtype=state_dtype(cfg))[0].copy().reshape(())


class DeviceMetrics(DeviceStage):
    _destroy, _m = 'vp_metrics_destroy', handle_alias

    def __init__(self, engine, cfg: MetricsCfg):
        super().__init__(engine)
        self.cfg = cfg
        self._c, self._sig = c_config(cfg)
        self.nbytes = state_dtype(cfg).itemsize
        self._create(self.lib.vp_metrics_create, C.byref(self._c), ptr(self._sig))

    def update(self, pred, gt, norm=None, area=None, rank=None, set=None, set_value=0, dist=None, oks=None):
        """Adds one call on torch's current stream, no synchronisation.  `pred`, `gt`: float32 CUDA [n, K, 3], contiguous; `norm` float32 CUDA [n, 2], `area`
        float32 CUDA [n], `rank`, `set` int32 CUDA [n], each or None; `dist` float32 CUDA [n, K] and `oks` float32 CUDA [n]: optional outputs."""
        import torch
        dev, K = self._dev, self.cfg.n_joints
        if not (isinstance(pred, torch.Tensor) and pred.ndim == 3):
            raise TypeError('pred: a float32 torch CUDA tensor [n, K, 3] expected')
        n = pred.shape[0]
        check_tensor('pred', pred, torch.float32, (n, K, 3), dev, True)
        check_tensor('gt', gt, torch.float32, (n, K, 3), dev, True)
        check_tensor('norm', norm, torch.float32, (n, 2), dev)
        check_tensor('area', area, torch.float32, (n,), dev)
        check_tensor('rank', rank, torch.int32, (n,), dev)
        check_tensor('set', set, torch.int32, (n,), dev)
        check_tensor('dist', dist, torch.float32, (n, K), dev)
        check_tensor('oks', oks, torch.float32, (n,), dev)
        p = (lambda a: ptr(a, n))
        self._check(self.lib.vp_metrics_update_stream(self._obj, p(pred), p(gt), p(norm), p(area), p(rank), p(set), int(set_value), n, p(dist), p(oks), self._stream()))

    def update_host(self, pred, gt, norm=None, area=None, rank=None, set=None, set_value=0):
        """`update` on numpy arrays (vp_metrics_update: upload, the same kernels, download, synchronous) -> (dist, oks)"""
        pred, gt, norm, area, rank, set_ = _host_args(self.cfg.n_joints, pred, gt, norm, area, rank, set)
        n = len(pred)
        dist, oks = np.empty((n, self.cfg.n_joints), F32), np.empty(n, F32)
        self._check(self.lib.vp_metrics_update(self._obj, ptr(pred), ptr(gt), ptr(norm), ptr(area), ptr(rank), ptr(set_), int(set_value), n, ptr(dist), ptr(oks)))
        return dist, oks

    def reset(self):
        """zero the state on torch's current stream"""
        self._check(self.lib.vp_metrics_reset_stream(self._obj, self._stream()))

    def snapshot(self, out=None):
        """a stream-ordered device copy of the state on torch's current stream: a uint8 CUDA tensor of the state's size (`parse_state` reads it on the host)"""
        import torch
        dev = self._dev
        if out is None:
            out = torch.empty((self.nbytes,), dtype=torch.uint8, device=dev)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device == dev and out.numel() == self.nbytes and out.is_contiguous()):
            raise ValueError(f'out: a contiguous uint8 tensor of {self.nbytes} bytes on {dev} expected')
        self._check(self.lib.vp_metrics_snapshot_stream(self._obj, out.data_ptr(), self._stream()))
        return out

    def state(self) -> np.ndarray:
        """the device state as a state_dtype(cfg) scalar array (synchronous)"""
        out = new_state(self.cfg)
        self._check(self.lib.vp_metrics_download_state(self._obj, out.ctypes.data))
        return out

    def result(self) -> MetricsResult:
        return finish(self.state(), self.cfg)
