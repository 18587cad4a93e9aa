"""CPU: the collect stage contract (csrc/collectgeom.h) through the host tap vp_dbg_collect_host -- the functions the kernels of vp_collect_stream run -- against
its numpy restatement (easy_vitpose_amd/devcollect.py), anchors written out as literals, a plain boolean mask, every refusal and the layout formula.  The device
is compared with this host model in tests/test_gpu_collect.py."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd import devcollect as dv
from easy_vitpose_amd.devcollect import collect_numpy, collect_tap, parse_records
import collect_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cc.host_cases()


def test_surface_symbols_macros_and_abi_version():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    for name in ('vp_collect_bytes', 'vp_collect_stream', 'vp_collect', 'vp_dbg_collect_host'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r'VP_API\s+\w+\s+' + name + r'\s*\(', hdr), name
    assert re.search(r'#define\s+VP_HAS_COLLECT\s+1\b', hdr)
    assert re.search(r'#define\s+VP_COLLECT_MAX_ROWS\s+8192\b', hdr) and dv.MAX_ROWS == 8192
    assert re.search(r'#define\s+VP_COLLECT_MAX_FRAMES\s+64\b', hdr) and dv.MAX_FRAMES == 64
    assert re.search(r'#define\s+VP_ABI_VERSION\s+4\b', hdr) and lib.vp_abi_version() == 4
    build = __import__('easy_vitpose_amd.build', fromlist=['SOURCES'])
    assert 'collect.hip' in build.SOURCES and 'collect.hip' not in build.SOURCE_FLAGS and 'collectgeom.h' in build.HEADERS


@pytest.mark.parametrize('name', sorted(CASES))
def test_tap_equals_the_numpy_twin_on_every_byte(name):
    got, want = collect_tap(**CASES[name]), collect_numpy(**CASES[name])
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), f'{name}: {int((got != want).sum())} bytes differ'


def test_every_combination_of_null_inputs():
    combos = cc.null_combos()
    assert len(combos) == 64
    tables = set()
    for name, cs in combos.items():
        got, want = collect_tap(**cs), collect_numpy(**cs)
        assert np.array_equal(got, want), name
        tables.add(got.tobytes())
    assert len(tables) == 64


def test_record_strides():
    assert [dv.record_words(k) for k in (1, 2, 17, 133)] == [12, 16, 60, 408]
    assert [dv.header_words(f) for f in (1, 3, 4, 63, 64)] == [4, 4, 8, 64, 68]


def test_anchor_three_rows():
    kp = np.arange(18, dtype=np.float32).reshape(3, 2, 3)
    cp = np.array([[1, 10, 20, 30, 40, 0, 0, 0, 0], [0, 11, 21, 31, 41, 0, 0, 0, 0], [1, 12, 22, 32, 42, 0, 0, 0, 0]], np.int32)
    kw = dict(kpts=kp, ids=np.array([5, 9, 6], np.int32), frame=np.array([1, 0, 1], np.int32), rank=np.array([0, 1, 2], np.int32), status=np.zeros(3, np.int32),
              score=np.array([0.5, 0.25, 2.0], np.float32), crop_params=cp, n_frames=2)
    f = lambda v: int(np.float32(v).view(np.int32))   # noqa: E731
    want = np.array([1, 2, 3, 0,                                                                                     # one row on frame 0, two on frame 1, three in all
                     9, 0, 1, f(0.25), 11, 21, 42, 62, f(6), f(7), f(8), f(9), f(10), f(11), 0, 0,                   # row 1 first: frame 0
                     5, 1, 0, f(0.5), 10, 20, 40, 60, f(0), f(1), f(2), f(3), f(4), f(5), 0, 0,
                     6, 1, 2, f(2.0), 12, 22, 44, 64, f(12), f(13), f(14), f(15), f(16), f(17), 0, 0], np.int32)
    for fn in (collect_tap, collect_numpy):
        assert fn(**kw).view(np.int32).tolist() == want.tolist(), fn.__name__


def test_anchor_ordinal_ids_count_dropped_rows():
    """without ids a row's id is its ordinal among the rows of its frame, dropped rows included: range(len(bboxes)) of the reference"""
    kp = np.zeros((6, 1, 3), np.float32)
    kw = dict(kpts=kp, frame=np.array([0, 1, 0, 7, 0, 1], np.int32), rank=np.array([0, -1, -1, 0, 0, 0], np.int32), n_frames=2)
    for fn in (collect_tap, collect_numpy):
        rec = parse_records(fn(**kw), 2, 1)
        assert rec.counts.tolist() == [2, 1] and rec.total == 3
        assert rec.row.tolist() == [0, 4, 5] and rec.frame.tolist() == [0, 0, 1]
        assert rec.ids.tolist() == [0, 2, 1], 'row 2 (dropped by its rank) and row 1 (dropped) take ordinals 1 and 0 of their frames; row 3 has no frame and none'
        assert rec.score.tolist() == [0.0] * 3 and not rec.box.any()


def test_anchor_max_records_cut_leaves_the_tail_and_keeps_the_true_totals():
    kp = np.arange(5 * 3, dtype=np.float32).reshape(5, 1, 3)
    kw = dict(kpts=kp, frame=np.array([1, 0, 1, 0, 1], np.int32), n_frames=2, max_records=2)
    nbytes = dv.collect_bytes(2, 1, 2)
    assert nbytes == 16 + 2 * 48
    for fn in (collect_tap, collect_numpy):
        buf = dv.aligned_bytes(nbytes + 48 + 5, fill=0xA5)
        out = fn(**kw, out=buf)
        assert out.nbytes == nbytes
        assert buf[:16].view(np.int32).tolist() == [2, 3, 5, 0], 'the header holds the true totals'
        rec = parse_records(out, 2, 1)
        assert rec.total == 5 and rec.row.tolist() == [1, 3] and rec.ids.tolist() == [0, 1]
        assert (buf[nbytes:] == 0xA5).all(), 'a byte behind the last written record was touched'
    # max_records beyond the total: the records that exist, and nothing behind them
    for fn in (collect_tap, collect_numpy):
        buf = dv.aligned_bytes(dv.collect_bytes(2, 1, 9), fill=0xA5)
        fn(**dict(kw, max_records=9), out=buf)
        assert parse_records(buf, 2, 1).row.tolist() == [1, 3, 0, 2, 4] and (buf[16 + 5 * 48:] == 0xA5).all()
    for fn in (collect_tap, collect_numpy):
        buf = dv.aligned_bytes(64, fill=0xA5)
        fn(**dict(kw, max_records=0), out=buf)
        assert buf[:16].view(np.int32).tolist() == [2, 3, 5, 0] and (buf[16:] == 0xA5).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_parse_records_returns_the_rows_of_a_boolean_mask(name):
    cs = CASES[name]
    order, ids, frame = cc.mask_rows(cs)
    n, K = cs['kpts'].shape[0], cs['kpts'].shape[1]
    rec = parse_records(collect_numpy(**cs), cs['n_frames'], K)
    assert rec.total == len(order) and rec.counts.tolist() == [int((frame[order] == f).sum()) for f in range(cs['n_frames'])]
    sel = order[:n if cs['max_records'] is None else cs['max_records']]
    assert rec.row.tolist() == sel.tolist() and rec.ids.tolist() == ids[sel].tolist() and rec.frame.tolist() == frame[sel].tolist()
    assert np.array_equal(rec.keypoints.view(np.uint32), cs['kpts'][sel].view(np.uint32)), 'keypoints bit for bit, NaN payloads included'
    if cs['score'] is not None:
        assert np.array_equal(rec.score.view(np.uint32), np.ascontiguousarray(cs['score'][sel]).view(np.uint32))
    if cs['crop_params'] is not None:
        p = cs['crop_params'][sel].astype(np.int64)
        wrap = lambda v: ((v + 2 ** 31) % 2 ** 32 - 2 ** 31)   # noqa: E731
        assert np.array_equal(rec.box, np.stack([p[:, 1], p[:, 2], wrap(p[:, 1] + p[:, 3]), wrap(p[:, 2] + p[:, 4])], -1))


def test_nan_payloads_survive():
    cs = CASES['nan_payload']
    w = cs['kpts'].view(np.uint32)
    assert ((w & 0x7f800000) == 0x7f800000).sum() > 20 and len(np.unique(w[np.isnan(cs['kpts'])])) > 20
    rec = parse_records(collect_tap(**cs), cs['n_frames'], 17)
    assert np.array_equal(rec.keypoints.view(np.uint32), cs['kpts'][rec.row].view(np.uint32))


def test_every_refusal_by_its_message():
    lib = capi.load_library()
    kp = np.zeros((2, 17, 3), np.float32)
    out = dv.aligned_bytes(1024)

    def call(kpts=kp.ctypes.data, n=2, k=17, stride=1, n_frames=1, max_records=2, out_=out.ctypes.data):
        rc = lib.vp_dbg_collect_host(kpts, n, k, None, None, None, None, None, stride, None, n_frames, max_records, out_)
        return rc, capi.last_error(None)
    assert call()[0] == capi.VP_OK
    for kw, msg in ((dict(n=-1), 'n = -1 rows outside 0..8192'), (dict(n=8193), 'n = 8193 rows outside 0..8192'),
                    (dict(n_frames=0), 'n_frames = 0 outside 1..64'), (dict(n_frames=65), 'n_frames = 65 outside 1..64'),
                    (dict(k=0), 'k = 0 joints outside 1..133'), (dict(k=134), 'k = 134 joints outside 1..133'),
                    (dict(max_records=-1), 'negative max_records'), (dict(kpts=None), 'null keypoints with n > 0'), (dict(out_=None), 'null output'),
                    (dict(stride=0), 'a score stride < 1'), (dict(out_=out.ctypes.data + 4), 'the output is not 16-byte aligned')):
        before = out.copy()
        rc, why = call(**kw)
        assert rc == capi.VP_ERR_INVALID and why == 'collect: ' + msg, (kw, why)
        assert np.array_equal(out, before), 'a refused call wrote'
    assert call(kpts=None, n=0)[0] == capi.VP_OK   # n = 0 needs no keypoints
    # the Python layer: the same limits, before the library is reached
    with pytest.raises(ValueError, match='8193 rows outside'):
        collect_numpy(np.zeros((8193, 1, 3), np.float32))
    with pytest.raises(capi.VpError, match='n = 8193 rows outside'):
        collect_tap(np.zeros((8193, 1, 3), np.float32))
    with pytest.raises(capi.VpError, match='n_frames = 65 outside'):
        collect_tap(kp, n_frames=65)
    with pytest.raises(ValueError, match='n_frames = 0 outside'):
        collect_numpy(kp, n_frames=0)
    with pytest.raises(capi.VpError, match='k = 134 joints'):
        collect_tap(np.zeros((1, 134, 3), np.float32))
    with pytest.raises(ValueError, match='negative max_records'):
        collect_numpy(kp, max_records=-1)
    with pytest.raises(ValueError, match='ids: 2 entries expected'):
        collect_numpy(kp, ids=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match=r'crop_params: \[2, 9\] expected'):
        collect_tap(kp, crop_params=np.zeros((2, 8), np.int32))
    with pytest.raises(ValueError, match='out: a contiguous uint8 array of at least'):
        collect_numpy(kp, out=np.zeros(8, np.uint8))


def test_collect_bytes_against_the_layout_formula():
    lib = capi.load_library()
    for n_frames in (1, 2, 3, 4, 5, 63, 64):
        for K in (1, 2, 3, 17, 133):
            for m in (0, 1, 7, 8192):
                want = 4 * ((n_frames + 1 + 3) // 4 * 4) + m * 16 * -(-(8 + 3 * K) // 4)
                assert lib.vp_collect_bytes(n_frames, K, m) == want == dv.collect_bytes(n_frames, K, m)
    assert lib.vp_collect_bytes(64, 133, 8192) == 272 + 8192 * 1632
    for bad in ((0, 17, 1), (65, 17, 1), (1, 0, 1), (1, 134, 1), (1, 17, -1)):
        assert lib.vp_collect_bytes(*bad) == -1


def test_n_zero_writes_a_zero_header_and_nothing_else():
    for fn in (collect_tap, collect_numpy):
        buf = dv.aligned_bytes(64, fill=0xA5)
        fn(np.zeros((0, 17, 3), np.float32), n_frames=5, max_records=0, out=buf)
        assert not buf[:32].any() and (buf[32:] == 0xA5).all()
