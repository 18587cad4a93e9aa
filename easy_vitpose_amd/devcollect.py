"""The collect stage (vp_collect_stream; contract in include/vitpose_hip.h and csrc/collectgeom.h): the persons a call keeps, packed into one dense record table
that one device-to-host copy brings down.  The numpy twin ``collect_numpy``, the parser ``parse_records``, the host tap and the layer behind
``VitPoseHip.collect`` / ``collect_host``.

The stage stands behind ``VitPoseHip.infer_boxes`` (its keypoints, crop params and status), the NMS (rank, score) and ``DeviceSmoother.update``; the ids and the
stream of every row are ``DeviceTracker.update``'s.  ``parse_records`` turns the table into the reference's ``{id: keypoints}`` per frame.
"""
from __future__ import annotations

import collections
import numbers

import numpy as np

from . import _capi as capi
from ._stage import check_tensor, ptr, stream_of

MAX_ROWS = 8192      # VP_COLLECT_MAX_ROWS
MAX_FRAMES = 64      # VP_COLLECT_MAX_FRAMES
MAX_JOINTS = 133
FIELDS = 8           # words in front of the keypoints: id, frame, row, score, box

Records = collections.namedtuple('Records', 'counts total ids frame row score box keypoints')


def header_words(n_frames: int) -> int:
    return (int(n_frames) + 1 + 3) // 4 * 4


def record_words(K: int) -> int:
    return (FIELDS + 3 * int(K) + 3) // 4 * 4


def collect_bytes(n_frames: int, K: int, max_records: int) -> int:
    """the size of a table (vp_collect_bytes' formula)"""
    _check_sizes(0, K, n_frames, max_records)
    return 4 * (header_words(n_frames) + int(max_records) * record_words(K))


def _integer(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))


def _check_sizes(n, K, n_frames, max_records):
    if not (_integer(n) and 0 <= n <= MAX_ROWS):
        raise ValueError(f'collect: n = {n} rows outside 0..{MAX_ROWS}')
    if not (_integer(n_frames) and 1 <= n_frames <= MAX_FRAMES):
        raise ValueError(f'collect: n_frames = {n_frames} outside 1..{MAX_FRAMES}')
    if not (_integer(K) and 1 <= K <= MAX_JOINTS):
        raise ValueError(f'collect: k = {K} joints outside 1..{MAX_JOINTS}')
    if not (_integer(max_records) and max_records >= 0):
        raise ValueError('collect: negative max_records')


def aligned_bytes(nbytes: int, fill: "int | None" = None) -> np.ndarray:
    """a uint8 array of `nbytes` whose first byte is 16-byte aligned (what the entries ask of a table), optionally filled"""
    raw = np.empty(int(nbytes) + 16, np.uint8)
    at = (-raw.ctypes.data) % 16
    out = raw[at:at + int(nbytes)]
    if fill is not None:
        out[:] = fill
    return out


def _host_rows(kpts, ids, frame, rank, status, score, crop_params):
    """numpy rows of a call, checked: kpts float32 [n, K, 3] contiguous, the int32 columns contiguous [n], score float32 [n] with its stride kept when it is a
    positive whole number of elements, crop_params int32 [n, 9]"""
    kpts = np.ascontiguousarray(kpts, dtype=np.float32)
    if kpts.ndim != 3 or kpts.shape[2] != 3:
        raise ValueError(f'kpts: [n, K, 3] expected, got {kpts.shape}')
    n = kpts.shape[0]
    cols = []
    for name, a in (('ids', ids), ('frame', frame), ('rank', rank), ('status', status)):
        a = None if a is None else np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        if a is not None and len(a) != n:
            raise ValueError(f'{name}: {n} entries expected, got {len(a)}')
        cols.append(a)
    if score is not None:
        score = np.asarray(score)
        if score.dtype != np.float32 or score.ndim != 1 or (n > 1 and (score.strides[0] <= 0 or score.strides[0] % 4)):
            score = np.ascontiguousarray(score, dtype=np.float32).reshape(-1)
        if len(score) != n:
            raise ValueError(f'score: {n} entries expected, got {len(score)}')
    if crop_params is not None:
        crop_params = np.ascontiguousarray(crop_params, dtype=np.int32)
        if crop_params.shape != (n, 9):
            raise ValueError(f'crop_params: [{n}, 9] expected, got {crop_params.shape}')
    return (kpts, *cols, score, crop_params)


def _table(out, nbytes):
    if out is None:
        return aligned_bytes(nbytes)
    if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.ndim == 1 and out.flags.c_contiguous and out.nbytes >= nbytes):
        raise ValueError(f'out: a contiguous uint8 array of at least {nbytes} bytes expected')
    return out


def collect_numpy(kpts, ids=None, frame=None, rank=None, status=None, score=None, crop_params=None, n_frames: int = 1, max_records: "int | None" = None,
                  out: "np.ndarray | None" = None) -> np.ndarray:
    """csrc/collectgeom.h in numpy: the bytes vp_collect_stream writes.  `max_records`: None = n.  `out`: a uint8 array to write into (the bytes behind the last
    written record stay as they are), None for a new one whose unwritten tail is zero."""
    kpts, ids, frame, rank, status, score, crop_params = _host_rows(kpts, ids, frame, rank, status, score, crop_params)
    n, K = kpts.shape[0], kpts.shape[1] if kpts.ndim == 3 else 0
    max_records = n if max_records is None else max_records
    _check_sizes(n, K, n_frames, max_records)
    hw, S = header_words(n_frames), record_words(K)
    nbytes = 4 * (hw + max_records * S)
    fresh = out is None
    out = _table(out, nbytes)
    if fresh:
        out[:] = 0
    fr = np.zeros(n, np.int32) if frame is None else frame
    valid = (fr >= 0) & (fr < n_frames)
    ordinal = np.zeros(n, np.int32)
    kept = valid.copy()
    if ids is not None:
        kept &= ids >= 0
    if rank is not None:
        kept &= rank >= 0
    if status is not None:
        kept &= status == 0
    counts = np.zeros(n_frames, np.int32)
    order = []
    for f in range(n_frames):
        rows = np.nonzero(valid & (fr == f))[0]
        ordinal[rows] = np.arange(len(rows), dtype=np.int32)
        rows = rows[kept[rows]]
        counts[f] = len(rows)
        order.append(rows)
    order = np.concatenate(order) if order else np.zeros(0, np.int64)
    header = np.zeros(hw, np.int32)
    header[:n_frames] = counts
    header[n_frames] = len(order)
    out[:4 * hw] = header.view(np.uint8)
    sel = order[:max_records]
    m = len(sel)
    rec = np.zeros((m, S), np.uint32)
    rec[:, 0] = (ordinal if ids is None else ids)[sel].view(np.uint32)
    rec[:, 1] = fr[sel].view(np.uint32)
    rec[:, 2] = sel.astype(np.uint32)
    if score is not None:
        rec[:, 3] = np.ascontiguousarray(score[sel]).view(np.uint32)
    if crop_params is not None:
        p = crop_params[sel].view(np.uint32)
        rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 7] = p[:, 1], p[:, 2], p[:, 1] + p[:, 3], p[:, 2] + p[:, 4]   # uint32 sums wrap, as the int32 ones do
    rec[:, FIELDS:FIELDS + 3 * K] = kpts.reshape(n, 3 * K).view(np.uint32)[sel]
    out[4 * hw:4 * (hw + m * S)] = rec.reshape(-1).view(np.uint8)
    return out[:nbytes]


def parse_records(buf, n_frames: int, K: int) -> Records:
    """A table as views: counts int32 [n_frames], the true total, and of the m = min(total, records the buffer holds) written records ids, frame, row int32 [m],
    score float32 [m], box int32 [m, 4] and keypoints float32 [m, K, 3]."""
    _check_sizes(0, K, n_frames, 0)
    buf = np.asarray(buf)
    if buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous:
        raise ValueError('parse_records: a contiguous uint8 array expected')
    hw, S = header_words(n_frames), record_words(K)
    if buf.nbytes < 4 * hw or buf.nbytes % 4:
        raise ValueError(f'parse_records: {buf.nbytes} bytes hold no header of {n_frames} frames')
    words = buf.view(np.int32)
    counts, total = words[:n_frames], int(words[n_frames])
    m = max(0, min(total, (len(words) - hw) // S))
    rec = words[hw:hw + m * S].reshape(m, S)
    return Records(counts, total, rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3].view(np.float32), rec[:, 4:8],
                   rec[:, FIELDS:FIELDS + 3 * K].view(np.float32).reshape(m, K, 3))


def frame_dicts(rec: Records, n_frames: int) -> "list[dict]":
    """the reference's result of a call: one `{id: keypoints [K, 3]}` per frame, in record order"""
    out = [dict() for _ in range(n_frames)]
    for i in range(len(rec.ids)):
        out[int(rec.frame[i])][int(rec.ids[i])] = rec.keypoints[i]
    return out


def _call_host(fn, handle, kpts, ids, frame, rank, status, score, crop_params, n_frames, max_records, out):
    kpts, ids, frame, rank, status, score, crop_params = _host_rows(kpts, ids, frame, rank, status, score, crop_params)
    n, K = kpts.shape[0], kpts.shape[1]
    max_records = n if max_records is None else max_records
    nbytes = None
    if _integer(max_records) and _integer(n_frames) and 1 <= n_frames <= MAX_FRAMES and 1 <= K <= MAX_JOINTS and max_records >= 0:
        nbytes = 4 * (header_words(n_frames) + max_records * record_words(K))
    fresh = out is None
    out = _table(out, nbytes if nbytes is not None else 16)   # (a call the library refuses writes nothing)
    if fresh:
        out[:] = 0
    stride = 1 if score is None or n < 2 else score.strides[0] // 4
    args = (ptr(kpts), n, K, ptr(ids), ptr(frame), ptr(rank), ptr(status), None if score is None or n == 0 else score.ctypes.data,
            stride, ptr(crop_params), int(n_frames), int(max_records), out.ctypes.data)
    capi.check(fn(*args) if handle is None else fn(handle, *args), handle)
    return out if nbytes is None else out[:nbytes]


def collect_tap(kpts, ids=None, frame=None, rank=None, status=None, score=None, crop_params=None, n_frames: int = 1, max_records: "int | None" = None,
                out: "np.ndarray | None" = None) -> np.ndarray:
    """vp_dbg_collect_host: csrc/collectgeom.h itself on host memory, no device needed (the model the device is tested against, never a fallback)"""
    return _call_host(capi.load_library().vp_dbg_collect_host, None, kpts, ids, frame, rank, status, score, crop_params, n_frames, max_records, out)


def collect_host(engine, kpts, ids=None, frame=None, rank=None, status=None, score=None, crop_params=None, n_frames: int = 1,
                 max_records: "int | None" = None, out: "np.ndarray | None" = None) -> np.ndarray:
    """`VitPoseHip.collect_host`: vp_collect on numpy arrays (upload, the same kernels, download, synchronous)"""
    return _call_host(engine.lib.vp_collect, engine._h, kpts, ids, frame, rank, status, score, crop_params, n_frames, max_records, out)


def collect_device(engine, kpts, ids=None, frame=None, rank=None, status=None, score=None, crop_params=None, n_frames: int = 1,
                   max_records: "int | None" = None, out=None):
    """`VitPoseHip.collect`: vp_collect_stream on torch CUDA tensors on torch's current stream, no synchronisation.  Returns the uint8 device table."""
    import torch
    dev = torch.device('cuda', engine.device_id)
    check_tensor('kpts', kpts, torch.float32, ('n', 'K', 3), dev, True)
    n, K = kpts.shape[0], kpts.shape[1]
    for t, name in ((ids, 'ids'), (frame, 'frame'), (rank, 'rank'), (status, 'status')):
        check_tensor(name, t, torch.int32, (n,), dev)
    check_tensor('score', score, torch.float32, (n,), dev, contiguous=False)
    check_tensor('crop_params', crop_params, torch.int32, (n, 9), dev)
    max_records = n if max_records is None else max_records
    _check_sizes(n, K, n_frames, max_records)
    nbytes = 4 * (header_words(n_frames) + max_records * record_words(K))
    if out is None:
        out = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    else:
        check_tensor('out', out, torch.uint8, ('bytes',), dev, True)
        if out.numel() < nbytes or out.data_ptr() % 16:
            raise ValueError(f'out: contiguous, 16-byte aligned, at least {nbytes} bytes on {dev} expected, got {tuple(out.shape)} on {out.device}')
    p = (lambda a: ptr(a, n))
    cs = stream_of(dev)
    capi.check(engine.lib.vp_collect_stream(engine._h, p(kpts), n, K, p(ids), p(frame), p(rank), p(status), p(score), 1 if score is None or n < 2 else score.stride(0),
                                            p(crop_params), int(n_frames), int(max_records), out.data_ptr(), cs), engine._h)
    return out
