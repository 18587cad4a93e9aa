"""COCO keypoint AP / AR on the device (vp_cocoeval_*; the contract in csrc/cocogeom.h): configuration, the state layout, the numpy twin, the host taps, the device
object, the finisher and the two host helpers of a COCO validation run (annotation reader, results writer).

A ``DeviceCocoEval`` is an accumulating stage with the life cycle of ``DeviceMetrics``: ``update`` takes the detections and the ground truth of a batch of images
where they lie on the GPU and appends one 16-byte record per kept detection on torch's current stream, never synchronising; ``accumulate`` sorts the records and
fills the precision / recall tables on the device; ``result()`` downloads them once and ``finish`` gives the ten figures of COCOeval's ``summarize``.  The procedure
is COCOeval for ``iouType='keypoints'`` with one category and maxDets = 20.  UNPINNED: pycocotools is not available to this project's tests; the twin below is a
transcription of its loops, not a comparison against its binary.  Feed the images in ascending id order: the order of equal scores across images is then
COCOeval's stable ``argsort(-score)``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
import numbers

import numpy as np

from . import _capi as capi
from ._stage import DeviceStage, check_tensor, handle_alias, ptr
from .posenms import NMS_MAX_K

MAX_ROWS, MAX_GTS, MAX_FRAMES, MAX_RECORDS = 8192, 8192, 256, 1 << 20
MAX_DETS, IMG_GTS = 20, 128
HDR_WORDS = 16
F32, F64, I32 = np.float32, np.float64, np.int32
OKS_THRS = np.array([0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.8999999999999999, 0.95], F64)   # np.linspace(.5, .95, 10) as literals
REC_THRS = np.arange(101).astype(F64) * (1.0 / 100.0)                                                # np.linspace(0, 1, 101) bit for bit
AREA_RNG = ((0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))                                  # all, medium, large
EPS = 2.220446049250313e-16                                                                           # np.spacing(1)
RECORD = np.dtype([('score', F32), ('matched', np.uint32), ('ignored', np.uint32), ('image', np.uint32)])
STAT_NAMES = ('AP', 'AP50', 'AP75', 'APM', 'APL', 'AR', 'AR50', 'AR75', 'ARM', 'ARL')


def coco_sigmas(dataset: str = 'coco'):
    """the per-joint sigmas of COCOeval's Params.kpt_oks_sigmas as doubles (COCO-17 only; any other joint set must be given)"""
    if dataset != 'coco':
        raise ValueError(f"coco_sigmas: only 'coco' (17 joints) is known, got {dataset!r}: give the sigmas of any other joint set")
    return tuple(float(v) for v in np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0)


@dataclasses.dataclass(frozen=True)
class CocoEvalCfg:
    """``n_joints``; ``max_records``: the capacity of the record table (one record per kept detection, at most 20 per image); ``sigmas``: one double per joint
    ('coco' = the COCO-17 table, for 17 joints only)."""
    n_joints: int = 17
    max_records: int = 1 << 17
    sigmas: "tuple | str" = 'coco'

    def __post_init__(self):
        def integer(v):
            return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))
        if not (integer(self.n_joints) and 1 <= self.n_joints <= NMS_MAX_K):
            raise ValueError(f'CocoEvalCfg: n_joints in 1..{NMS_MAX_K} expected, got {self.n_joints!r}')
        if not (integer(self.max_records) and 1 <= self.max_records <= MAX_RECORDS):
            raise ValueError(f'CocoEvalCfg: max_records in 1..{MAX_RECORDS} expected, got {self.max_records!r}')
        sig = self.sigmas
        if isinstance(sig, str):
            if self.n_joints != 17:
                raise ValueError("CocoEvalCfg: sigmas='coco' names the COCO-17 table, for n_joints = 17 only")
            sig = coco_sigmas(sig)
        if sig is None:
            raise ValueError('CocoEvalCfg: sigmas are required')
        sig = tuple(float(v) for v in sig)
        if len(sig) != self.n_joints or not all(math.isfinite(v) and v > 0.0 for v in sig):
            raise ValueError(f'CocoEvalCfg: sigmas are {self.n_joints} finite values > 0')
        object.__setattr__(self, 'n_joints', int(self.n_joints))
        object.__setattr__(self, 'max_records', int(self.max_records))
        object.__setattr__(self, 'sigmas', sig)


def c_config(cfg: CocoEvalCfg):
    """(vp_cocoeval_cfg, the float64 sigma array: keep it alive for the call)"""
    if not isinstance(cfg, CocoEvalCfg):
        raise TypeError(f'a CocoEvalCfg expected, got {type(cfg).__name__}')
    return capi.vp_cocoeval_cfg(cfg.n_joints, cfg.max_records, (C.c_int32 * 2)(0, 0)), np.ascontiguousarray(cfg.sigmas, dtype=F64)


def state_dtype(cfg: CocoEvalCfg) -> np.dtype:
    """the state blob as csrc/cocogeom.h lays it out (zeroed = new)"""
    return np.dtype([('calls', np.int64), ('images', np.int64), ('rows', np.int64), ('kept', np.int64), ('records', np.int64), ('dropped', np.int64),
                     ('gts', np.int64), ('gt_overflow', np.int64), ('nonfinite', np.int64), ('npig', np.int64, 3), ('pad', np.int64, 4),
                     ('table', RECORD, cfg.max_records)])


RESULT = np.dtype([('calls', np.int64), ('images', np.int64), ('rows', np.int64), ('kept', np.int64), ('records', np.int64), ('dropped', np.int64),
                   ('gts', np.int64), ('gt_overflow', np.int64), ('nonfinite', np.int64), ('npig', np.int64, 3), ('pad', np.int64, 4),
                   ('precision', F64, (3, 10, 101)), ('recall', F64, (3, 10))])


def new_state(cfg: CocoEvalCfg) -> np.ndarray:
    return np.zeros((), state_dtype(cfg))


def state_bytes(cfg: CocoEvalCfg) -> int:
    c, _ = c_config(cfg)
    b, r = C.c_int64(0), C.c_int64(0)
    lib = capi.load_library()
    capi.check(lib.vp_cocoeval_state_bytes(C.byref(c), C.byref(b)))
    capi.check(lib.vp_cocoeval_result_bytes(C.byref(r)))
    assert b.value == state_dtype(cfg).itemsize == 8 * HDR_WORDS + 16 * cfg.max_records and r.value == RESULT.itemsize
    return b.value


def _host_args(K, kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame):
    kpts = np.ascontiguousarray(np.zeros((0, K, 3), F32) if kpts is None else kpts, dtype=F32).reshape(-1, K, 3)
    n = len(kpts)
    gt_kpts = np.ascontiguousarray(np.zeros((0, K, 3), F32) if gt_kpts is None else gt_kpts, dtype=F32).reshape(-1, K, 3)
    g = len(gt_kpts)
    out = []
    for name, a, dt, shape, needed in (('score', score, F32, (n,), n > 0), ('frame', frame, I32, (n,), False), ('rank', rank, I32, (n,), False),
                                       ('gt_box', gt_box, F32, (g, 4), g > 0), ('gt_area', gt_area, F32, (g,), g > 0), ('gt_flags', gt_flags, I32, (g,), False),
                                       ('gt_frame', gt_frame, I32, (g,), False)):
        if a is None and needed:
            raise ValueError(f'{name}: required')
        if a is None and name in ('score', 'gt_box', 'gt_area'):
            a = np.zeros(shape, dt)
        a = None if a is None else np.ascontiguousarray(a, dtype=dt)
        if a is not None and a.size == 0:
            a = a.reshape(shape)
        if a is not None and a.shape != shape:
            raise ValueError(f'{name}: shape {shape} expected, got {a.shape}')
        out.append(a)
    score, frame, rank, gt_box, gt_area, gt_flags, gt_frame = out
    return kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame


def _c_exp(v):
    try:
        return math.exp(v)
    except OverflowError:   # the C library returns +infinity where Python raises
        return math.inf


_exp = np.frompyfunc(_c_exp, 1, 1)   # the C library's exp, element by element: what the host tap calls (numpy's own exp is another implementation)


def _compute_oks(dts, gts, var):
    """COCOeval.computeOks for one image: dts [D, K, 3] in (y, x, .), gts = list of dict(kpts [K, 3] (y, x, v), box, area) -> ious [D, G].  One deviation: the sum of
    a pair's terms runs in joint order (np.cumsum), not pairwise."""
    ious = np.zeros((len(dts), len(gts)), F64)
    for j, gt in enumerate(gts):
        g = gt['kpts'].astype(F64)
        xg, yg, vg = g[:, 1], g[:, 0], g[:, 2]
        k1 = np.count_nonzero(vg > 0)
        bb = gt['box'].astype(F64)
        x0, x1 = bb[0] - bb[2], bb[0] + bb[2] * 2
        y0, y1 = bb[1] - bb[3], bb[1] + bb[3] * 2
        for i in range(len(dts)):
            d = dts[i].astype(F64)
            xd, yd = d[:, 1], d[:, 0]
            if k1 > 0:
                dx, dy = xd - xg, yd - yg
            else:
                z = np.zeros(len(g))
                dx = np.maximum(z, x0 - xd) + np.maximum(z, xd - x1)
                dy = np.maximum(z, y0 - yd) + np.maximum(z, yd - y1)
            e = (dx * dx + dy * dy) / var / (F64(gt['area']) + EPS) / 2
            if k1 > 0:
                e = e[vg > 0]
            ious[i, j] = np.cumsum(_exp(-e).astype(F64))[-1] / e.shape[0]
    return ious


def cocoeval_numpy_update(state: np.ndarray, cfg: CocoEvalCfg, kpts, score, frame=None, rank=None, gt_kpts=None, gt_box=None, gt_area=None, gt_flags=None,
                          gt_frame=None, n_frames: int = 1) -> np.ndarray:
    """One update in numpy, a transcription of COCOeval's computeOks / evaluateImg loops image by image, the same bytes as the tap: adds the call to `state` (a
    state_dtype(cfg) scalar array, in place) and returns match int32 [n, 10]."""
    K = cfg.n_joints
    kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame = _host_args(K, kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame)
    n, g = len(kpts), len(gt_kpts)
    var = (np.asarray(cfg.sigmas, F64) * 2) ** 2
    fr = np.zeros(n, I32) if frame is None else frame
    gfr = np.zeros(g, I32) if gt_frame is None else gt_frame
    counted = np.ones(n, bool) if rank is None else rank >= 0
    match = np.full((n, 10), -2, I32)
    st = state
    images0 = int(st['images'])
    with np.errstate(all='ignore'):
        for b in range(n_frames):
            rows = np.flatnonzero(counted & (fr == b))
            key = score[rows].astype(F64)
            key[np.isnan(key)] = -np.inf
            rows = rows[np.argsort(-key, kind='mergesort')][:MAX_DETS]
            grow = np.flatnonzero(gfr == b)
            st['gt_overflow'] += max(0, len(grow) - IMG_GTS)
            grow = grow[:IMG_GTS]
            gts = [dict(kpts=gt_kpts[j], box=gt_box[j], area=gt_area[j], iscrowd=bool(0 if gt_flags is None else gt_flags[j] & 1)) for j in grow]
            for gt in gts:
                gt['ignore0'] = gt['iscrowd'] or np.count_nonzero(gt['kpts'][:, 2] > 0) == 0
            dts = kpts[rows]
            x, y = dts[:, :, 1].astype(F64), dts[:, :, 0].astype(F64)
            d_area = (np.max(x, axis=1) - np.min(x, axis=1)) * (np.max(y, axis=1) - np.min(y, axis=1)) if len(rows) else np.zeros(0)
            ious = _compute_oks(dts, gts, var)
            bad = ~np.isfinite(ious)
            st['nonfinite'] += int(bad.sum())
            D, G = len(rows), len(gts)
            dtm = np.zeros((3, 10, D), bool)
            dt_ig = np.zeros((3, 10, D), bool)
            for a, (lo, hi) in enumerate(AREA_RNG):
                ignore = [gt['ignore0'] or bool(F64(gt['area']) < lo or F64(gt['area']) > hi) for gt in gts]
                gtind = np.argsort(np.array(ignore, bool), kind='mergesort') if G else np.zeros(0, np.int64)
                st['npig'][a] += G - int(sum(ignore))
                for tind, t in enumerate(OKS_THRS):
                    gtm = np.zeros(G, bool)
                    for dind in range(D):
                        iou = min([t, 1 - 1e-10])
                        m = -1
                        for gind in gtind:
                            if gtm[gind] and not gts[gind]['iscrowd']:
                                continue
                            if m > -1 and not ignore[m] and ignore[gind]:
                                break
                            if bad[dind, gind] or ious[dind, gind] < iou:   # DEVIATION: a non-finite OKS never matches
                                continue
                            iou = ious[dind, gind]
                            m = gind
                        if m == -1:
                            dt_ig[a, tind, dind] = bool(d_area[dind] < lo or d_area[dind] > hi)
                        else:
                            dt_ig[a, tind, dind] = ignore[m]
                            dtm[a, tind, dind] = True
                            gtm[m] = True
                        if a == 0:
                            match[rows[dind], tind] = -1 if m == -1 else grow[m]
            bits = (np.uint32(1) << np.arange(30, dtype=np.uint32)).reshape(3, 10, 1)
            matched = (dtm * bits).sum(axis=(0, 1)).astype(np.uint32)
            ignored = (dt_ig * bits).sum(axis=(0, 1)).astype(np.uint32)
            for dind in range(D):
                pos = int(st['records'])
                st['kept'] += 1
                if pos < cfg.max_records:
                    st['table'][pos] = (score[rows[dind]], matched[dind], ignored[dind], images0 + b)
                    st['records'] += 1
                else:
                    st['dropped'] += 1
            st['gts'] += G
    st['calls'] += 1
    st['images'] += n_frames
    st['rows'] += n
    return match


def cocoeval_numpy_oks(cfg: CocoEvalCfg, kpts, score, frame=None, rank=None, gt_kpts=None, gt_box=None, gt_area=None, gt_flags=None, gt_frame=None, n_frames: int = 1) -> list:
    """the OKS matrix [kept detections, used gts] of every image of a call, as the twin computes it (the tests' margin condition reads these)"""
    K = cfg.n_joints
    kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame = _host_args(K, kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame)
    var = (np.asarray(cfg.sigmas, F64) * 2) ** 2
    fr = np.zeros(len(kpts), I32) if frame is None else frame
    gfr = np.zeros(len(gt_kpts), I32) if gt_frame is None else gt_frame
    counted = np.ones(len(kpts), bool) if rank is None else rank >= 0
    out = []
    with np.errstate(all='ignore'):
        for b in range(n_frames):
            rows = np.flatnonzero(counted & (fr == b))
            key = score[rows].astype(F64)
            key[np.isnan(key)] = -np.inf
            rows = rows[np.argsort(-key, kind='mergesort')][:MAX_DETS]
            grow = np.flatnonzero(gfr == b)[:IMG_GTS]
            out.append(_compute_oks(kpts[rows], [dict(kpts=gt_kpts[j], box=gt_box[j], area=gt_area[j]) for j in grow], var))
    return out


def cocoeval_numpy_accumulate(state: np.ndarray) -> np.ndarray:
    """COCOeval.accumulate on a state -> a RESULT scalar array, the same bytes as the tap"""
    st = state
    res = np.zeros((), RESULT)
    for f in RESULT.names[:-2]:
        res[f] = st[f]
    R = int(st['records'])
    tab = st['table'][:R]
    key = tab['score'].astype(F64)
    key[np.isnan(key)] = -np.inf
    inds = np.argsort(-key, kind='mergesort')
    precision, recall = -np.ones((3, 10, 101)), -np.ones((3, 10))
    bit = np.uint32(1)
    for a in range(3):
        npig = int(st['npig'][a])
        if npig == 0:
            continue
        for t in range(10):
            dtm = ((tab['matched'][inds] >> np.uint32(10 * a + t)) & bit).astype(bool)
            dt_ig = ((tab['ignored'][inds] >> np.uint32(10 * a + t)) & bit).astype(bool)
            tp = np.cumsum(np.logical_and(dtm, np.logical_not(dt_ig))).astype(F64)
            fp = np.cumsum(np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))).astype(F64)
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            q = np.zeros(101)
            recall[a, t] = rc[-1] if nd else 0
            if nd:
                pr = np.maximum.accumulate(pr[::-1])[::-1]   # for i in range(nd - 1, 0, -1): if pr[i] > pr[i - 1]: pr[i - 1] = pr[i]
            ix = np.searchsorted(rc, REC_THRS, side='left')
            ok = ix < nd
            q[ok] = pr[ix[ok]]
            precision[a, t] = q
    res['precision'], res['recall'] = precision, recall
    return res


def cocoeval_tap(state: np.ndarray, cfg: CocoEvalCfg, kpts, score, frame=None, rank=None, gt_kpts=None, gt_box=None, gt_area=None, gt_flags=None, gt_frame=None,
                 n_frames: int = 1) -> np.ndarray:
    """One update through the host tap vp_dbg_cocoeval_update_host: the model the device is tested against, never a fallback.  Adds the call to `state` in place
    and returns match int32 [n, 10]."""
    K = cfg.n_joints
    kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame = _host_args(K, kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame)
    c, sig = c_config(cfg)
    assert state.dtype == state_dtype(cfg) and state.flags.c_contiguous
    match = np.empty((len(kpts), 10), I32)
    capi.check(capi.load_library().vp_dbg_cocoeval_update_host(state.ctypes.data, C.byref(c), sig.ctypes.data, ptr(kpts), ptr(score), ptr(frame), ptr(rank), len(kpts),
                                                               ptr(gt_kpts), ptr(gt_box), ptr(gt_area), ptr(gt_flags), ptr(gt_frame), len(gt_kpts), int(n_frames),
                                                               ptr(match)))
    return match


def cocoeval_tap_accumulate(state: np.ndarray, cfg: CocoEvalCfg) -> np.ndarray:
    """vp_dbg_cocoeval_accumulate_host on a state -> a RESULT scalar array"""
    c, _ = c_config(cfg)
    assert state.dtype == state_dtype(cfg) and state.flags.c_contiguous
    res = np.zeros((), RESULT)
    capi.check(capi.load_library().vp_dbg_cocoeval_accumulate_host(state.ctypes.data, C.byref(c), res.ctypes.data))
    return res


@dataclasses.dataclass(frozen=True)
class CocoResult:
    """``stats`` [10] in COCOeval's order (AP, AP50, AP75, APM, APL, AR, AR50, AR75, ARM, ARL; -1 where a range holds no gt), ``precision`` [3, 10, 101], ``recall``
    [3, 10] (ranges all / medium / large), the header counts."""
    stats: np.ndarray
    precision: np.ndarray
    recall: np.ndarray
    calls: int
    images: int
    rows: int
    kept: int
    records: int
    gts: int
    nonfinite: int
    npig: tuple

    def summary(self) -> str:
        """the ten lines of COCOeval.summarize for keypoints"""
        rows = (('Average Precision', '(AP)', '0.50:0.95', '   all'), ('Average Precision', '(AP)', '0.50', '   all'), ('Average Precision', '(AP)', '0.75', '   all'),
                ('Average Precision', '(AP)', '0.50:0.95', 'medium'), ('Average Precision', '(AP)', '0.50:0.95', ' large'),
                ('Average Recall', '(AR)', '0.50:0.95', '   all'), ('Average Recall', '(AR)', '0.50', '   all'), ('Average Recall', '(AR)', '0.75', '   all'),
                ('Average Recall', '(AR)', '0.50:0.95', 'medium'), ('Average Recall', '(AR)', '0.50:0.95', ' large'))
        return '\n'.join(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(t, ty, iou, ar, MAX_DETS, s) for (t, ty, iou, ar), s in zip(rows, self.stats))


def _mean(s):
    s = s[s > -1]
    return -1.0 if len(s) == 0 else float(np.mean(s))


def finish(result: np.ndarray) -> CocoResult:
    """COCOeval.summarize (keypoints) on a RESULT blob.  Raises when records were dropped or gts left out: the figures would not be the data set's."""
    r = result
    if int(r['dropped']) or int(r['gt_overflow']):
        raise RuntimeError(f"cocoeval: {int(r['dropped'])} records did not fit into max_records and {int(r['gt_overflow'])} gts exceeded {IMG_GTS} per image: "
                           'the figures would not describe the data set')
    p, rc = r['precision'], r['recall']
    t50, t75 = 0, 5
    stats = np.array([_mean(p[0]), _mean(p[0, t50]), _mean(p[0, t75]), _mean(p[1]), _mean(p[2]),
                      _mean(rc[0]), _mean(rc[0, t50:t50 + 1]), _mean(rc[0, t75:t75 + 1]), _mean(rc[1]), _mean(rc[2])], F64)
    return CocoResult(stats, p.copy(), rc.copy(), int(r['calls']), int(r['images']), int(r['rows']), int(r['kept']), int(r['records']), int(r['gts']),
                      int(r['nonfinite']), tuple(int(v) for v in r['npig']))


class DeviceCocoEval(DeviceStage):
    _destroy, _e = 'vp_cocoeval_destroy', handle_alias

    def __init__(self, engine, cfg: CocoEvalCfg):
        super().__init__(engine)
        self.cfg = cfg
        self._c, self._sig = c_config(cfg)
        self._create(self.lib.vp_cocoeval_create, C.byref(self._c), self._sig.ctypes.data)

    def update(self, kpts, score, frame=None, rank=None, gt_kpts=None, gt_box=None, gt_area=None, gt_flags=None, gt_frame=None, n_frames: int = 1, match=None):
        """Adds one call on torch's current stream, no synchronisation.  Contiguous CUDA tensors: `kpts` float32 [n, K, 3], `score` float32 [n], `frame`, `rank` int32
        [n] or None; `gt_kpts` float32 [g, K, 3], `gt_box` float32 [g, 4], `gt_area` float32 [g], `gt_flags`, `gt_frame` int32 [g] or None (all None: no gt);
        `match` int32 [n, 10]: optional output."""
        import torch
        dev, K = self._dev, self.cfg.n_joints
        if not (isinstance(kpts, torch.Tensor) and kpts.ndim == 3):
            raise TypeError('kpts: a float32 torch CUDA tensor [n, K, 3] expected')
        n = kpts.shape[0]
        g = 0 if gt_kpts is None else gt_kpts.shape[0]
        check_tensor('kpts', kpts, torch.float32, (n, K, 3), dev, True)
        check_tensor('score', score, torch.float32, (n,), dev, True)
        check_tensor('frame', frame, torch.int32, (n,), dev)
        check_tensor('rank', rank, torch.int32, (n,), dev)
        check_tensor('gt_kpts', gt_kpts, torch.float32, (g, K, 3), dev, g > 0)
        check_tensor('gt_box', gt_box, torch.float32, (g, 4), dev, g > 0)
        check_tensor('gt_area', gt_area, torch.float32, (g,), dev, g > 0)
        check_tensor('gt_flags', gt_flags, torch.int32, (g,), dev)
        check_tensor('gt_frame', gt_frame, torch.int32, (g,), dev)
        check_tensor('match', match, torch.int32, (n, 10), dev)
        p = ptr
        self._check(self.lib.vp_cocoeval_update_stream(self._obj, p(kpts, n), p(score, n), p(frame, n), p(rank, n), n, p(gt_kpts, g), p(gt_box, g), p(gt_area, g),
                                                       p(gt_flags, g), p(gt_frame, g), g, int(n_frames), p(match, n), self._stream()))

    def update_host(self, kpts, score, frame=None, rank=None, gt_kpts=None, gt_box=None, gt_area=None, gt_flags=None, gt_frame=None, n_frames: int = 1) -> np.ndarray:
        """`update` on numpy arrays (vp_cocoeval_update: upload, the same kernels, download, synchronous) -> match [n, 10]"""
        kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame = _host_args(self.cfg.n_joints, kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags,
                                                                                            gt_frame)
        match = np.empty((len(kpts), 10), I32)
        self._check(self.lib.vp_cocoeval_update(self._obj, ptr(kpts), ptr(score), ptr(frame), ptr(rank), len(kpts), ptr(gt_kpts), ptr(gt_box), ptr(gt_area),
                                                ptr(gt_flags), ptr(gt_frame), len(gt_kpts), int(n_frames), ptr(match)))
        return match

    def accumulate(self, out=None):
        """the precision / recall tables of the state so far, on torch's current stream: a uint8 CUDA tensor of RESULT.itemsize bytes (`parse_result` reads it)"""
        import torch
        dev = self._dev
        if out is None:
            out = torch.empty((RESULT.itemsize,), dtype=torch.uint8, device=dev)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device == dev and out.numel() == RESULT.itemsize and out.is_contiguous()):
            raise ValueError(f'out: a contiguous uint8 tensor of {RESULT.itemsize} bytes on {dev} expected')
        self._check(self.lib.vp_cocoeval_accumulate_stream(self._obj, out.data_ptr(), self._stream()))
        return out

    def accumulate_host(self) -> np.ndarray:
        """vp_cocoeval_accumulate: synchronous -> a RESULT scalar array"""
        res = np.zeros((), RESULT)
        self._check(self.lib.vp_cocoeval_accumulate(self._obj, res.ctypes.data))
        return res

    def reset(self):
        """zero the state on torch's current stream"""
        self._check(self.lib.vp_cocoeval_reset_stream(self._obj, self._stream()))

    def state(self) -> np.ndarray:
        """the device state as a state_dtype(cfg) scalar array (synchronous)"""
        out = new_state(self.cfg)
        self._check(self.lib.vp_cocoeval_download_state(self._obj, out.ctypes.data))
        return out

    def result(self) -> CocoResult:
        """accumulate, one small download, the ten figures"""
        return finish(self.accumulate_host())


def parse_result(raw) -> np.ndarray:
    """the bytes of an accumulate output (a numpy uint8 array) as a RESULT scalar array"""
    return np.frombuffer(np.ascontiguousarray(raw, dtype=np.uint8).tobytes(), dtype=RESULT)[0].copy().reshape(())


# ---------------------------------------------------------------- host helpers of a COCO validation run

@dataclasses.dataclass
class CocoAnnotations:
    """A COCO keypoint annotation file per image, image ids ascending, in the update entry's layout: ``gt_kpts[i]`` float32 [g_i, K, 3] rows of (y, x, v), ``gt_box[i]``
    float32 [g_i, 4] (x, y, w, h), ``gt_area[i]`` float32 [g_i], ``gt_flags[i]`` int32 [g_i] (bit 0 = iscrowd)."""
    image_ids: list
    file_names: list
    sizes: list            # (width, height)
    gt_kpts: list
    gt_box: list
    gt_area: list
    gt_flags: list
    n_joints: int

    def batch(self, indices):
        """the gts of images `indices` (positions in image_ids) as one update call: dict(gt_kpts, gt_box, gt_area, gt_flags, gt_frame, n_frames)"""
        idx = list(indices)
        K = self.n_joints
        cat = (lambda parts, shape, dt: np.concatenate([np.zeros(shape, dt)] + [p for p in parts], axis=0))
        return dict(gt_kpts=cat([self.gt_kpts[i] for i in idx], (0, K, 3), F32), gt_box=cat([self.gt_box[i] for i in idx], (0, 4), F32),
                    gt_area=cat([self.gt_area[i] for i in idx], (0,), F32), gt_flags=cat([self.gt_flags[i] for i in idx], (0,), I32),
                    gt_frame=cat([np.full(len(self.gt_area[i]), f, I32) for f, i in enumerate(idx)], (0,), I32), n_frames=len(idx))


def load_annotations(path, category_id: int = 1) -> CocoAnnotations:
    """reads a COCO keypoint annotation file (images, annotations of one category)"""
    with open(path) as f:
        data = json.load(f)
    images = sorted(data['images'], key=lambda im: im['id'])
    by_image = {im['id']: [] for im in images}
    K = None
    for ann in data.get('annotations', []):
        if ann.get('category_id', category_id) != category_id or ann['image_id'] not in by_image or 'keypoints' not in ann:
            continue
        if K is None:
            K = len(ann['keypoints']) // 3
        if len(ann['keypoints']) != 3 * K:
            raise ValueError(f"{path}: annotation {ann.get('id')} has {len(ann['keypoints'])} keypoint values, {3 * K} expected")
        by_image[ann['image_id']].append(ann)
    K = 17 if K is None else K
    out = CocoAnnotations([], [], [], [], [], [], [], K)
    for im in images:
        anns = by_image[im['id']]
        kp = np.array([a['keypoints'] for a in anns], F64).reshape(len(anns), K, 3)
        out.image_ids.append(int(im['id']))
        out.file_names.append(im.get('file_name', str(im['id']).zfill(12) + '.jpg'))
        out.sizes.append((int(im.get('width', 0)), int(im.get('height', 0))))
        out.gt_kpts.append(np.ascontiguousarray(kp[:, :, [1, 0, 2]], dtype=F32))
        out.gt_box.append(np.array([a['bbox'] for a in anns], F32).reshape(len(anns), 4))
        out.gt_area.append(np.array([a['area'] for a in anns], F32))
        out.gt_flags.append(np.array([int(a.get('iscrowd', 0)) & 1 for a in anns], I32))
    return out


def results_json(path, image_ids, kpts, scores, rounded: bool = True, category_id: int = 1) -> list:
    """The results list the reference's evaluation_on_coco.py writes: one element per detection with image_id, category_id, score, an empty bbox and keypoints as
    [x, y, 0] per joint -- `rounded` rounds the coordinates to whole pixels as that script does.  `kpts` [n, K, 3] in (y, x, .); writes `path` unless None."""
    kpts = np.asarray(kpts, F32)
    out = []
    for image_id, kp, s in zip(image_ids, kpts, scores):
        flat = []
        for k in kp:
            flat.append(float(round(float(k[1]), 0)) if rounded else float(k[1]))
            flat.append(float(round(float(k[0]), 0)) if rounded else float(k[0]))
            flat.append(0)
        out.append({'image_id': int(image_id), 'category_id': int(category_id), 'score': float(s), 'bbox': [], 'keypoints': flat})
    if path is not None:
        with open(path, 'w') as f:
            json.dump(out, f, indent=4)
    return out
