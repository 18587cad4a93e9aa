"""Flip-test as a handle mode (vp_set_flip_test, include/vitpose_hip.h): everything of it that runs without a GPU -- the exported surface, the
argument checks of the partner table (the function the setter itself calls, through its host-only tap), the index function of the interleaved
batch (the function the twin patch gather itself evaluates), and the Python / CLI front ends."""
from __future__ import annotations

import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import COCO17_FLIP_PAIRS, resolve_flip_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['vp_set_flip_test', 'vp_clear_flip_test', 'vp_flip_test_enabled', 'vp_group_set_flip_test', 'vp_group_clear_flip_test',
               'vp_dbg_flip_partner', 'vp_dbg_flip_layout', 'vp_dbg_decode_flip']


def _pairs(p):
    return np.ascontiguousarray(np.asarray(p, dtype=np.int32).reshape(-1, 2))


def test_library_exports_and_binds_the_mode():
    lib = capi.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f'{name} not exported'
        assert name in capi.SYMBOLS, f'{name} not bound by _capi'
        assert re.search(r'VP_API\s+int\s+' + name + r'\s*\(', hdr), f'{name} not declared in the header'
        assert getattr(lib, name).argtypes is not None, f'{name} has no ctypes signature'
    # the library and the header agree on the ABI version, and the header announces the mode to C users
    assert lib.vp_abi_version() == int(re.search(r'#define\s+VP_ABI_VERSION\s+(\d+)', hdr).group(1))
    assert re.search(r'#define\s+VP_HAS_FLIP_TEST_MODE\s+1', hdr)


def test_null_handles_are_refused_without_touching_a_device():
    lib = capi.load_library()
    p = _pairs(COCO17_FLIP_PAIRS)
    assert lib.vp_set_flip_test(None, p.ctypes.data, len(p), 0) == capi.VP_ERR_INVALID
    assert lib.vp_clear_flip_test(None) == capi.VP_ERR_INVALID
    assert lib.vp_flip_test_enabled(None) == 0
    assert lib.vp_group_set_flip_test(None, p.ctypes.data, len(p), 0) == capi.VP_ERR_INVALID
    assert lib.vp_group_clear_flip_test(None) == capi.VP_ERR_INVALID


def test_partner_table_and_its_refusals():
    """vp_dbg_flip_partner = the validation + table vp_set_flip_test runs against the active head's K."""
    lib = capi.load_library()
    out = np.full(17, -1, dtype=np.int32)
    p = _pairs(COCO17_FLIP_PAIRS)
    assert lib.vp_dbg_flip_partner(17, p.ctypes.data, len(p), out.ctypes.data) == capi.VP_OK
    assert out.tolist() == [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
    assert lib.vp_dbg_flip_partner(17, None, 0, out.ctypes.data) == capi.VP_OK        # no pairs: every joint is its own partner
    assert out.tolist() == list(range(17))
    assert lib.vp_dbg_flip_partner(17, p.ctypes.data, len(p), None) == capi.VP_OK     # validation only
    for bad in ([[0, 17]], [[-1, 3]], [[1, 2], [3, 133]]):
        b = _pairs(bad)
        assert lib.vp_dbg_flip_partner(17, b.ctypes.data, len(b), out.ctypes.data) == capi.VP_ERR_INVALID, bad
        assert 'outside' in capi.last_error()
    assert lib.vp_dbg_flip_partner(17, p.ctypes.data, -1, out.ctypes.data) == capi.VP_ERR_INVALID
    assert 'negative' in capi.last_error()
    assert lib.vp_dbg_flip_partner(17, None, 3, out.ctypes.data) == capi.VP_ERR_INVALID
    assert 'null' in capi.last_error()
    b = _pairs([[1, 2], [131, 132]])                                                    # valid for wholebody's 133 joints, not for 17
    assert lib.vp_dbg_flip_partner(133, b.ctypes.data, 2, None) == capi.VP_OK
    assert lib.vp_dbg_flip_partner(17, b.ctypes.data, 2, None) == capi.VP_ERR_INVALID


def test_interleaved_layout_over_every_batch():
    """Output row r of the forward batch reads crop src[r], mirrored or not: rows 2 i / 2 i + 1 are crop i and its mirror image, rows beyond 2 n
    (encoder padding, tile_rules.hip pick_run_batch: the next multiple of 4) repeat the last row.  Walked for every n a chunk can hold under
    every max_batch up to 128, with the row count the chunk plan really pads to (vp_dbg_run_batch)."""
    lib = capi.load_library()
    for max_batch in range(2, 129):
        for n in range(1, min(max_batch // 2, 64) + 1):
            for D in (384, 1280):
                rows = lib.vp_dbg_run_batch(2 * n, D, (max_batch + 3) // 4 * 4)
                assert 2 * n <= rows <= (max_batch + 3) // 4 * 4, (n, rows, max_batch)
                src = np.full(rows, -1, dtype=np.int32)
                mir = np.full(rows, -1, dtype=np.int32)
                assert lib.vp_dbg_flip_layout(n, rows, src.ctypes.data, mir.ctypes.data) == capi.VP_OK
                assert src[:2 * n].tolist() == [r // 2 for r in range(2 * n)]
                assert mir[:2 * n].tolist() == [r % 2 for r in range(2 * n)]
                assert (src[2 * n:] == n - 1).all() and (mir[2 * n:] == 1).all()
    one = np.zeros(4, dtype=np.int32)
    assert lib.vp_dbg_flip_layout(0, 4, one.ctypes.data, one.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_flip_layout(3, 5, one.ctypes.data, one.ctypes.data) == capi.VP_ERR_INVALID   # fewer rows than 2 n
    assert lib.vp_dbg_flip_layout(2, 4, None, one.ctypes.data) == capi.VP_ERR_INVALID


def test_flip_test_true_is_the_coco17_table_only():
    assert resolve_flip_pairs(None, 'coco', 17) is None and resolve_flip_pairs(False, 'wholebody', 133) is None
    assert resolve_flip_pairs(True, 'coco', 17) == [[a, a + 1] for a in range(1, 17, 2)]
    for dataset, k in (('wholebody', 133), ('coco_25', 25), ('mpii', 16), ('ap10k', 17), ('aic', 14)):
        with pytest.raises(ValueError, match='explicitly'):
            resolve_flip_pairs(True, dataset, k)
    assert resolve_flip_pairs([(0, 5), (2, 3)], 'mpii', 16) == [[0, 5], [2, 3]]
    with pytest.raises(ValueError, match='outside'):
        resolve_flip_pairs([[0, 16]], 'mpii', 16)


def test_vitinference_refuses_flip_test_true_for_another_dataset():
    """Raised from the arguments alone, before a device or a checkpoint is touched."""
    from easy_vitpose_amd import VitInference
    from helpers import weights
    _, sd, _ = weights('s', 'mpii')
    with pytest.raises(ValueError, match='COCO'):
        VitInference(sd, lambda img: np.empty((0, 5)), 's', dataset='mpii', flip_test=True)


def test_cli_arguments(tmp_path):
    from easy_vitpose_amd.cli import build_parser, flip_test_argument
    ap = build_parser()
    base = ['--input', 'clip.npy', '--synthetic', 's', '--boxes', 'b.json']
    a = ap.parse_args(base)
    assert not a.flip_test and a.flip_pairs is None and not a.shift_heatmap and flip_test_argument(a) is None
    a = ap.parse_args(base + ['--flip-test', '--shift-heatmap'])
    assert a.shift_heatmap and flip_test_argument(a) is True
    f = tmp_path / 'pairs.json'
    f.write_text(json.dumps([[0, 5], [1, 4]]))
    assert flip_test_argument(ap.parse_args(base + ['--flip-pairs', str(f)])) == [[0, 5], [1, 4]]
    f.write_text(json.dumps([[0, 5, 1]]))
    with pytest.raises(ValueError, match='pairs'):
        flip_test_argument(ap.parse_args(base + ['--flip-pairs', str(f)]))
