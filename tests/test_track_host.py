"""CPU: the box tracker of csrc/sortgeom.h through the host taps vp_dbg_track_host / vp_dbg_lsap(-1) -- the same functions the kernels of
vp_tracker_update_stream run -- against the Python twin tracker.Sort, the twin against the reference's own Sort on crowded sequences that enter the
assignment branch (tests/golden/sort_crowd.npz), the assignment against scipy, every refusal of the C entries and of the Python layer, the flags and the
host-side row bound.  The device is compared with this host model in tests/test_gpu_track.py."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import os
import re
import warnings

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.devtracker import (FLAG_BAD_ROW, FLAG_BIRTHS, FLAG_DETS, FLAG_ROWS, STATE_DTYPE, TRACK_MAX, TRACK_MAX_STREAMS, HostTracker, RowBound, TrackCfg,
                                         c_config, mask_of, state_bytes)
from easy_vitpose_amd.tracker import Sort
from track_cases import CROWDS, IOU_THRESHOLD, all_sequences, associate_twin, crowd, far_people, lsap_cases, lsap_matrix, rows_with_state, run_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQUENCES = {tag: (frames, age, hits) for tag, frames, age, hits in all_sequences()}


@functools.lru_cache(maxsize=None)
def twin_rows(tag):
    frames, age, hits = SEQUENCES[tag]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return run_rows(Sort(age, hits, IOU_THRESHOLD).update, frames)


@functools.lru_cache(maxsize=None)
def twin_birth_frames(tag):
    """the frame every id (1-based) of the twin was born in"""
    frames, age, hits = SEQUENCES[tag]
    twin, born = Sort(age, hits, IOU_THRESHOLD), {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for f, d in enumerate(frames):
            first = twin._next_id
            twin.update(d.copy())
            born.update({k + 1: f for k in range(first, twin._next_id)})
    return born


def lsap_tap(device_id, iou, thr):
    iou = np.ascontiguousarray(iou, np.float64)
    out = np.full(iou.shape[0], -7, np.int32)
    capi.check(capi.load_library().vp_dbg_lsap(device_id, iou.ctypes.data, iou.shape[0], iou.shape[1], thr, out.ctypes.data))
    return out


def test_surface_symbols_macros_and_state_layout():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    for name in ('vp_tracker_create', 'vp_tracker_destroy', 'vp_tracker_reset_stream', 'vp_tracker_update_stream', 'vp_tracker_update', 'vp_tracker_state_bytes',
                 'vp_tracker_download_state', 'vp_dbg_track_host', 'vp_dbg_lsap'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r'VP_API\s+int\s+' + name + r'\s*\(', hdr), name
    assert re.search(r'#define\s+VP_HAS_TRACKER\s+1\b', hdr)
    assert re.search(r'#define\s+VP_TRACK_MAX\s+128\b', hdr) and TRACK_MAX == 128
    assert re.search(r'#define\s+VP_TRACK_MAX_STREAMS\s+64\b', hdr) and TRACK_MAX_STREAMS == 64
    assert re.search(r'#define\s+VP_ABI_VERSION\s+4\b', hdr) and lib.vp_abi_version() == 4
    assert C.sizeof(capi.vp_track_cfg) == 16
    assert state_bytes(1) == STATE_DTYPE.itemsize == 32 + 128 * (480 + 40 + 4) and state_bytes(64) == 64 * STATE_DTYPE.itemsize
    assert 'track.hip' in __import__('easy_vitpose_amd.build', fromlist=['SOURCES']).SOURCES


@pytest.mark.parametrize('tag', list(SEQUENCES))
def test_host_tap_against_the_twin(tag):
    """Row counts, frame and id columns equal; the fp64 boxes of the tap's state within 1e-9 of the twin's (the bound tests/test_host_logic.py grants the fp64
    tracker against the reference; measured: 1.1e-12 at most over the nine sequences -- the elimination order of sortgeom.h against LAPACK's inverse); the
    float32 rows are float32(fp64 box) exactly."""
    frames, age, hits = SEQUENCES[tag]
    want = twin_rows(tag)
    tap = HostTracker(TrackCfg(age, hits, IOU_THRESHOLD, 1))
    got, calls = rows_with_state(tap, frames)
    assert got.shape == want.shape
    assert np.array_equal(got[:, [0, 6]], want[:, [0, 6]])
    d = np.abs(got[:, 1:6] - want[:, 1:6])
    print(f'{tag}: {len(got)} rows, max |tap - twin| = {np.nanmax(d):.3e}')
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.nanmax(d) < 1e-9
    at = 0
    for rows, ids, stream, count, flags in calls:
        n = int(count[-1])
        assert count[0] == n and flags[0] == 0
        assert np.array_equal(rows[:n, :5], got[at:at + n, 1:6].astype(np.float32), equal_nan=True)
        assert np.array_equal(rows[:n, 5], got[at:at + n, 6].astype(np.float32)) and np.array_equal(ids[:n], got[at:at + n, 6].astype(np.int32))
        assert (stream[:n] == 0).all() and (stream[n:] == -1).all() and (ids[n:] == -1).all()
        assert np.isnan(rows[n:, :4]).all() and (rows[n:, 4] == 0).all() and (rows[n:, 5] == -1).all()
        at += n


@pytest.mark.parametrize('seed', [c[0] for c in CROWDS])
def test_twin_against_the_reference_on_crowds(golden_dir, seed):
    """The reference's Sort on sequences that enter the assignment branch.  Per frame the rows are equal as sets of (box, score); the ids agree up to ONE
    bijection over the sequence, and that bijection joins only tracks that are first reported in the same frame and were born in the same frame (births of one
    frame: the reference numbers them in an order that depends on a tie-break of its solver, the twin in detection-index order)."""
    want = np.load(os.path.join(golden_dir, 'sort_crowd.npz'))[f'crowd{seed}']
    got = twin_rows(f'crowd{seed}')
    assert got.shape == want.shape
    fwd, back, first_got, first_want, relabelled = {}, {}, {}, {}, 0
    for f in np.unique(want[:, 0]):
        a, b = got[got[:, 0] == f], want[want[:, 0] == f]
        assert a.shape == b.shape
        a, b = a[np.lexsort(a[:, 1:6].T[::-1])], b[np.lexsort(b[:, 1:6].T[::-1])]
        assert np.abs(a[:, 1:6] - b[:, 1:6]).max() < 1e-9
        for ia, ib in zip(a[:, 6].astype(int), b[:, 6].astype(int)):
            assert fwd.setdefault(ia, ib) == ib and back.setdefault(ib, ia) == ia, f'frame {int(f)}: id {ia} <-> {ib} breaks the bijection'
            first_got.setdefault(ia, f)
            first_want.setdefault(ib, f)
    born = twin_birth_frames(f'crowd{seed}')
    for ia, ib in fwd.items():
        relabelled += ia != ib
        assert first_got[ia] == first_want[ib]
        assert born[ia] == born[ib], f'id {ia} (born in frame {born[ia]}) is the reference\'s {ib}, an id the twin gave out in frame {born[ib]}'
    print(f'crowd {seed}: {len(fwd)} ids, {relabelled} relabelled')


@pytest.mark.parametrize('nd', (1, 2, 7, 63, 64, 65, 128))
def test_assignment_against_scipy(nd):
    from scipy.optimize import linear_sum_assignment
    for nd_, nt, dens in lsap_cases():
        if nd_ != nd:
            continue
        iou = lsap_matrix(nd, nt, dens)
        # the optimum: with a threshold below every non-zero entry the filter drops the zero pairs only
        tod = lsap_tap(-1, iou, 1e-30)
        assert len(set(tod[tod >= 0].tolist())) == (tod >= 0).sum(), 'a track paired twice'
        mine = sum(iou[d, t] for d, t in enumerate(tod) if t >= 0)
        r, c = linear_sum_assignment(-iou)
        best = iou[r, c].sum()
        assert abs(mine - best) <= 1e-12 * max(best, 1e-300), (nd, nt, dens, mine, best)
        assert np.array_equal(lsap_tap(-1, iou, IOU_THRESHOLD), associate_twin(iou, IOU_THRESHOLD)), (nd, nt, dens)


def test_the_shortcut_is_a_branch_of_its_own_and_degenerate_matrices():
    iou = np.array([[0.31, 0.29], [0.29, 0.0]])   # rows A, B; columns X, Y
    assert lsap_tap(-1, iou, IOU_THRESHOLD).tolist() == [0, -1], 'the shortcut pairs A-X'
    assert associate_twin(iou, IOU_THRESHOLD).tolist() == [0, -1]
    from scipy.optimize import linear_sum_assignment
    r, c = linear_sum_assignment(-iou)
    assert sorted(zip(r.tolist(), c.tolist())) == [(0, 1), (1, 0)], 'the optimum pairs A-Y and B-X, both under the threshold'
    assert lsap_tap(-1, iou.T.copy(), IOU_THRESHOLD).tolist() == [0, -1]
    assert lsap_tap(-1, np.zeros((5, 3)), IOU_THRESHOLD).tolist() == [-1] * 5
    two = np.array([[0.9, 0.8], [0.85, 0.1]])    # ambiguous: the assignment takes 0.8 + 0.85 over 0.9 + 0.1
    assert lsap_tap(-1, two, IOU_THRESHOLD).tolist() == [1, 0]
    nan = np.array([[np.nan, 0.8], [0.85, 0.9]])   # bounded on a NaN: ends, never pairs a NaN entry
    got = lsap_tap(-1, nan, IOU_THRESHOLD)
    assert got[0] in (-1, 1) and got[1] in (-1, 0, 1)
    lib = capi.load_library()
    out = np.zeros(2, np.int32)
    for thr in (0.0, 1.0, np.nan, -0.3):
        assert lib.vp_dbg_lsap(-1, two.ctypes.data, 2, 2, thr, out.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_lsap(-1, two.ctypes.data, 129, 2, 0.3, out.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_lsap(-1, None, 2, 2, 0.3, out.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_lsap(-1, two.ctypes.data, 2, 2, 0.3, None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_lsap(-1, None, 0, 0, 0.3, None) == capi.VP_OK


def _rc(cfg=(1, 3, 0.3, 2), n=2, stride=5, mask=1, n_out=4, null=None, state=True):
    lib = capi.load_library()
    c = capi.vp_track_cfg(*cfg) if cfg is not None else None
    blob = np.zeros(max(1, min(cfg[3], 64)) if cfg else 1, STATE_DTYPE)
    dets = np.array([[10, 10, 50, 90, 0.9], [100, 10, 150, 90, 0.8]], np.float32)
    out = dict(rows=np.zeros((8, 6), np.float32), ids=np.zeros(8, np.int32), stream=np.zeros(8, np.int32), count=np.zeros(65, np.int32), flags=np.zeros(64, np.int32))
    ptr = {k: v.ctypes.data for k, v in out.items()}
    ptr['dets'] = dets.ctypes.data
    if null:
        ptr[null] = None
    return lib.vp_dbg_track_host(blob.ctypes.data if state else None, None if c is None else C.byref(c), ptr['dets'], stride, None, n, mask, ptr['rows'], ptr['ids'],
                                 ptr['stream'], n_out, ptr['count'], ptr['flags'])


def test_every_refusal_of_the_c_entries():
    assert _rc() == capi.VP_OK
    assert _rc(null='flags') == capi.VP_OK
    for null in ('dets', 'rows', 'ids', 'stream', 'count'):
        assert _rc(null=null) == capi.VP_ERR_INVALID, null
    assert 'tracker' in capi.last_error(None)
    assert _rc(null='dets', n=0) == capi.VP_OK, 'the coasting call needs no detections'
    assert _rc(null='rows', n_out=0) == capi.VP_OK
    assert _rc(cfg=None) == capi.VP_ERR_INVALID and _rc(state=False) == capi.VP_ERR_INVALID
    assert _rc(stride=4) == capi.VP_ERR_INVALID and _rc(stride=6, n=1) == capi.VP_OK
    for ns in (0, -1, 65):
        assert _rc(cfg=(1, 3, 0.3, ns)) == capi.VP_ERR_INVALID, ns
    assert _rc(cfg=(1, 3, 0.3, 64), mask=1 << 63) == capi.VP_OK
    assert _rc(cfg=(-1, 3, 0.3, 1)) == capi.VP_ERR_INVALID and _rc(cfg=(1, -1, 0.3, 1)) == capi.VP_ERR_INVALID
    assert _rc(cfg=(0, 0, 0.3, 1)) == capi.VP_OK
    for thr in (0.0, 1.0, -0.1, 1.5, np.nan):
        assert _rc(cfg=(1, 3, thr, 1)) == capi.VP_ERR_INVALID, thr
    assert _rc(n_out=-1) == capi.VP_ERR_INVALID and _rc(n=-1) == capi.VP_ERR_INVALID
    assert _rc(mask=4) == capi.VP_ERR_INVALID and _rc(mask=3) == capi.VP_OK and _rc(mask=0) == capi.VP_OK
    lib = capi.load_library()   # the handle entries refuse a NULL handle / tracker before anything else
    h = C.c_void_p()
    good = capi.vp_track_cfg(1, 3, 0.3, 1)
    assert lib.vp_tracker_create(None, C.byref(good), C.byref(h)) == capi.VP_ERR_INVALID
    assert lib.vp_tracker_update_stream(None, None, 5, None, 0, 1, None, None, None, 0, None, None, None) == capi.VP_ERR_INVALID
    assert lib.vp_tracker_update(None, None, 5, None, 0, 1, None, None, None, 0, None, None) == capi.VP_ERR_INVALID
    assert lib.vp_tracker_reset_stream(None, 1, None) == capi.VP_ERR_INVALID and lib.vp_tracker_destroy(None) == capi.VP_ERR_INVALID
    assert lib.vp_tracker_download_state(None, None) == capi.VP_ERR_INVALID
    b = C.c_int64()
    assert lib.vp_tracker_state_bytes(0, C.byref(b)) == capi.VP_ERR_INVALID and lib.vp_tracker_state_bytes(65, C.byref(b)) == capi.VP_ERR_INVALID
    assert lib.vp_tracker_state_bytes(1, None) == capi.VP_ERR_INVALID


def test_trackcfg_and_python_refusals():
    assert TrackCfg() == TrackCfg(1, 3, float(np.float32(0.3)), 1) and hash(TrackCfg())
    with pytest.raises(dataclasses.FrozenInstanceError):
        TrackCfg().max_age = 2
    for kw in (dict(max_age=-1), dict(max_age=1.5), dict(max_age=True), dict(min_hits=-1), dict(min_hits='3'), dict(n_streams=0), dict(n_streams=65),
               dict(iou_threshold=0.0), dict(iou_threshold=1.0), dict(iou_threshold=float('nan')), dict(iou_threshold='0.3'), dict(iou_threshold=True)):
        with pytest.raises(ValueError):
            TrackCfg(**kw)
    got = TrackCfg(np.int64(2), np.int32(1), np.float32(0.5), np.int64(4))
    assert got == TrackCfg(2, 1, 0.5, 4) and type(got.max_age) is int and type(got.iou_threshold) is float
    with pytest.raises(TypeError):
        c_config({'max_age': 1})
    assert mask_of(None, 3) == 7 and mask_of([0, 2], 3) == 5 and mask_of(2, 3) == 2 and mask_of((), 3) == 0 and mask_of(None, 64) == 2 ** 64 - 1
    for bad in ([3], 8, -1, [64]):
        with pytest.raises(ValueError):
            mask_of(bad, 3)
    tap = HostTracker(TrackCfg(n_streams=2))
    with pytest.raises(ValueError, match='frame_index'):
        tap.update(np.zeros((2, 5), np.float32), frame_index=[0])
    with pytest.raises(capi.VpError):
        tap.update(np.zeros((1, 5), np.float32), n_out=-1)


def test_vitinference_and_cli_tracker_argument():
    """Raised from the arguments alone, before a device or a checkpoint is touched."""
    from easy_vitpose_amd import VitInference
    from easy_vitpose_amd.cli import build_parser
    from helpers import weights
    _, sd, _ = weights('s', 'coco')
    with pytest.raises(ValueError, match='tracker'):
        VitInference(sd, lambda img: np.empty((0, 5)), 's', dataset='coco', is_video=True, tracker='gpu')
    ap = build_parser()
    base = ['--input', 'clip.npy', '--synthetic', 's', '--boxes', 'b.json']
    assert ap.parse_args(base).tracker == 'host' and ap.parse_args(base + ['--tracker', 'device']).tracker == 'device'
    with pytest.raises(SystemExit):
        ap.parse_args(base + ['--tracker', 'gpu'])


def test_the_flags():
    cfg = TrackCfg(1, 3, 0.3, 1)
    for n in (128, 129):   # flag 1: detections beyond 128 are ignored, the first 128 kept
        tap = HostTracker(cfg)
        rows, ids, _, count, flags = tap.update(far_people(n, 1), n_out=200)
        assert flags[0] == (FLAG_DETS if n > 128 else 0) and count[-1] == 128 and ids[:128].tolist() == list(range(128, 0, -1))
        assert np.array_equal(tap.state()[0]['tracks']['x'][:128, 0], (far_people(n, 1)[:128, 0].astype(np.float64) + far_people(n, 1)[:128, 2]) / 2)
    tap = HostTracker(cfg)   # flag 2: births at 128 live tracks are dropped, the lowest detection indices kept
    tap.update(far_people(126, 2), n_out=200)
    d = np.concatenate([far_people(126, 2)[:120], far_people(5, 3, x0=20000.0)])   # 120 matches, 6 tracks coast, 5 births meet 126 live tracks
    rows, ids, _, count, flags = tap.update(d, n_out=200)
    S = tap.state()[0]
    assert flags[0] == FLAG_BIRTHS and S['n_tracks'] == 128 and S['next_id'] == 128 and count[-1] == 122
    assert sorted(ids[:122].tolist()) == list(range(1, 121)) + [127, 128]
    assert np.array_equal(S['tracks']['x'][126:128, 0], (d[120:122, 0].astype(np.float64) + d[120:122, 2]) / 2)
    rows, ids, _, count, flags = tap.update(d[:120], n_out=200)
    assert flags[0] == 0 and tap.state()[0]['n_tracks'] == 122, 'max_age 1: the six coasting tracks leave, the two unmatched births live on for a call'
    tap = HostTracker(cfg)   # flag 4: rows cut by n_out, the count keeps the true total
    full = HostTracker(cfg).update(far_people(7, 4), n_out=7)
    rows, ids, stream, count, flags = tap.update(far_people(7, 4), n_out=6)
    assert flags[0] == FLAG_ROWS and count.tolist() == [7, 7] and np.array_equal(rows, full[0][:6]) and full[4][0] == 0
    tap = HostTracker(TrackCfg(1, 3, 0.3, 2))   # flag 8: a non-finite row on its stream, a bad stream index on every stepped stream
    d = far_people(6, 5)
    d[1, 2] = np.nan
    d[4, 4] = np.inf
    rows, ids, stream, count, flags = tap.update(d, frame_index=[0, 0, 0, 1, 1, 1], n_out=8)
    assert flags.tolist() == [FLAG_BAD_ROW, FLAG_BAD_ROW] and count.tolist() == [2, 2, 4] and stream[:4].tolist() == [0, 0, 1, 1]
    clean = HostTracker(TrackCfg(1, 3, 0.3, 2)).update(d[[0, 2, 3, 5]], frame_index=[0, 0, 1, 1], n_out=8)
    assert np.array_equal(rows, clean[0], equal_nan=True) and clean[4].tolist() == [0, 0]
    tap = HostTracker(TrackCfg(1, 3, 0.3, 2))
    rows, ids, stream, count, flags = tap.update(far_people(3, 6), frame_index=[0, 2, -1], n_out=4, step=[0])
    assert flags.tolist() == [FLAG_BAD_ROW, 0] and count.tolist() == [1, 0, 1]
    tap = HostTracker(TrackCfg(1, 3, 0.3, 3))   # flag 4 names the streams whose rows were cut: not a stream without rows behind the cut
    rows, ids, stream, count, flags = tap.update(far_people(5, 8), frame_index=[0, 0, 0, 2, 2], n_out=2)
    assert flags.tolist() == [FLAG_ROWS, 0, FLAG_ROWS] and count.tolist() == [3, 0, 2, 5] and stream.tolist() == [0, 0]
    rows, ids, stream, count, flags = tap.update(far_people(5, 8), frame_index=[0, 0, 0, 2, 2], n_out=4)
    assert flags.tolist() == [0, 0, FLAG_ROWS] and stream.tolist() == [0, 0, 0, 2]
    # a stream outside the step mask is untouched, its rows are ignored; a stepped stream without rows coasts
    tap = HostTracker(TrackCfg(1, 1, 0.3, 2))
    tap.update(far_people(4, 7), frame_index=[0, 0, 1, 1], n_out=8)
    before = tap.state().copy()
    rows, ids, stream, count, flags = tap.update(far_people(4, 7), frame_index=[0, 0, 1, 1], n_out=8, step=[1])
    after = tap.state()
    assert after[0].tobytes() == before[0].tobytes() and after[1]['frame_count'] == 2 and count.tolist() == [0, 2, 2] and stream[:2].tolist() == [1, 1]
    rows, ids, stream, count, flags = tap.update(far_people(4, 7)[2:], frame_index=[1, 1], n_out=8)
    assert count.tolist() == [2, 2, 4] and ids[:4].tolist() == [2, 1, 2, 1], 'stream 0 coasts: its predicted boxes are reported'


def test_zero_area_boxes_and_ids_per_stream():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d = np.array([[5, 5, 5, 5, 0.5], [10, 10, 50, 90, 0.9], [60, 10, 60, 90, 0.7], [100, 40, 150, 40, 0.6]], np.float32)
        seq = [d, d, d[1:2], np.empty((0, 5), np.float32), d]
        twin, tap = Sort(2, 1, IOU_THRESHOLD), HostTracker(TrackCfg(2, 1, IOU_THRESHOLD, 1))
        want = run_rows(twin.update, [x.astype(np.float64) for x in seq])
    got, _ = rows_with_state(tap, seq)
    assert got.shape == want.shape and np.array_equal(got[:, [0, 6]], want[:, [0, 6]]) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) < 1e-9 and np.isnan(want).any(), 'a zero-area box is tracked for one call with a NaN box, as the twin does'


@pytest.mark.parametrize('max_age', [0, 1, 2, 3])
def test_row_bound_property(max_age):
    """The bound the Python layer sizes its buffers with, against the twin: seeded crowds with random empty calls."""
    rng = np.random.default_rng(40 + max_age)
    for trial in range(6):
        P, F = int(rng.integers(1, 30)), 40
        skip = tuple(int(f) for f in np.flatnonzero(rng.random(F) < 0.4))
        frames = crowd(100 * max_age + trial, P, F, miss=0.3, skip=skip)
        min_hits = int(rng.integers(0, 4))
        twin, bound = Sort(max_age, min_hits, IOU_THRESHOLD), RowBound(max_age)
        for d in frames:
            b = bound.push(len(d))
            assert len(twin.update(d.copy())) <= b <= TRACK_MAX
            assert b == len(d) or len(d) == 0
    many = RowBound(1, n_streams=4)   # several streams: the window sum whatever n_dets; a partial step falls back to the cap until it leaves the window
    assert [many.push(n) for n in (5, 0, 3, 0)] == [5, 5, 8, 3]
    assert many.push(2, stepped=1) == 128 and many.push(2) == 512 and many.push(1) == 512 and many.push(1) == 4


@pytest.mark.parametrize('max_age', [0, 1, 2, 3])
def test_row_bound_property_on_several_streams(max_age):
    """Several streams, one Sort twin per stream: rows attributed to random streams, random partial step masks, partial and full resets, calls without a
    row (every stepped stream coasts).  The rows the twins report in a call never exceed the bound that call gets; asking first changes nothing."""
    rng = np.random.default_rng(70 + max_age)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for trial in range(8):
            ns, F = int(rng.integers(2, 6)), 60
            min_hits = int(rng.integers(0, 4))
            per = [crowd(1000 * max_age + 10 * trial + s, int(rng.integers(1, 9)), F, miss=0.3) for s in range(ns)]
            twins, bound, partial_seen, coasted = [Sort(max_age, min_hits, IOU_THRESHOLD) for _ in range(ns)], RowBound(max_age, ns), 0, 0
            for f in range(F):
                r = rng.random()
                if r < 0.06:     # some streams restart: the others keep their tracks
                    which = [s for s in range(ns) if rng.random() < 0.5][:ns - 1] or [0]
                    for s in which:
                        twins[s] = Sort(max_age, min_hits, IOU_THRESHOLD)
                    bound.reset(len(which))
                    partial_seen += 1
                elif r < 0.09:   # all of them
                    twins = [Sort(max_age, min_hits, IOU_THRESHOLD) for _ in range(ns)]
                    bound.reset(ns)
                stepped = list(range(ns)) if rng.random() < 0.7 else [s for s in range(ns) if rng.random() < 0.5]
                empty = rng.random() < 0.35          # the detector did not run: no row at all
                silent = set() if empty else {s for s in stepped if rng.random() < 0.3}   # cameras without a row in a call that has rows
                dets = {s: (np.empty((0, 5)) if empty or s in silent else per[s][f]) for s in stepped}
                n_dets = sum(len(d) for d in dets.values())
                ask = bound.bound(n_dets, len(stepped))
                b = bound.push(n_dets, len(stepped))
                assert ask == b
                rows = sum(len(twins[s].update(dets[s].copy())) for s in stepped)
                coasted += int(rows > n_dets)
                assert rows <= b <= TRACK_MAX * max(len(stepped), 0), (trial, f, rows, b, n_dets, stepped)
            assert partial_seen > 0
        assert coasted > 0 or max_age == 0, 'the sequences do make streams coast beyond the rows of a call'


def test_row_bound_partial_reset_and_queries():
    b = RowBound(1, 3)
    assert [b.push(n) for n in (6, 6)] == [6, 12]
    b.reset(1)                                    # streams 0 and 2 keep their tracks: the window must not forget them
    assert b.bound(0) == b.bound(0) == 3 * 128 and b.push(0) == 3 * 128 and b.push(0) == 3 * 128
    assert b.push(0) == 0, 'three full calls later nothing can be listed'
    b.push(9)
    b.reset(3)
    assert b.bound(0) == 0 and b.bound(4) == 4
    b.reset(0)
    assert b.bound(0) == 0
    one = RowBound(2)
    for n in (3, 0, 2):
        assert one.bound(n) == one.bound(n)
        one.push(n)
    assert one.bound(0) == 5 and one.bound(7) == 7 and one.push(0) == 5
