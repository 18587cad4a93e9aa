"""CPU: One-Euro keypoint smoothing of csrc/eurogeom.h through the host tap vp_dbg_smooth_host -- the same functions the kernels of vp_smooth_update_stream run --
against the reference's own OneEuroFilter (tests/golden/one_euro.npz) and against the numpy twin smooth.OneEuro, every refusal of the C entries and of the
Python layer, the flags and the gap rule.  Every comparison is an equality of bits.  The device is compared with this host model in tests/test_gpu_smooth.py."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.devsmooth import (FLAG_BAD_ROW, FLAG_DUP, FLAG_FULL, MAX_ROWS, SLOTS, STATE_DTYPE, HostSmoother, SmoothCfg, c_config, state_bytes, state_dtype)
from easy_vitpose_amd.smooth import OneEuro
from smooth_cases import SEQUENCES, interleaved_streams, run, same_bits, sequence, table_full, tag_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'one_euro.npz'))


def twin_of(K, cfg: SmoothCfg) -> OneEuro:
    return OneEuro(K, cfg.min_cutoff, cfg.beta, cfg.d_cutoff, cfg.max_age, cfg.n_streams, cfg.missing)


def assert_state_equals_twin(blob, twin: OneEuro):
    """every live track of the twin sits in the slot the rule gives it, with the twin's bits; every other slot is free"""
    assert blob['frame_count'].tolist() == twin.frame_count
    assert int((blob['last_seen'] > 0).sum()) == len(twin.tracks)
    for (s, tid), trk in twin.tracks.items():
        slot = twin.slots[(s, tid)]
        assert blob[s]['id'][slot] == tid and blob[s]['last_seen'][slot] == trk.last_seen, (s, tid, slot)
        assert same_bits(blob[s]['x_prev'][slot], trk.x_prev) and same_bits(blob[s]['dx_prev'][slot], trk.dx_prev), (s, tid)
        assert np.array_equal(blob[s]['fresh'][slot], trk.fresh.astype(np.uint8)), (s, tid)


def tap_against_twin(K, cfg_kw, calls):
    cfg = SmoothCfg(**cfg_kw)
    tap, twin = HostSmoother(K, cfg), twin_of(K, cfg)
    got, want = run(tap.update, tap.reset, calls), run(twin.update, twin.reset, calls)
    for i, ((go, gf), (wo, wf)) in enumerate(zip(got, want)):
        assert same_bits(go, wo), f'update {i}: keypoints'
        assert gf.tolist() == wf.tolist(), f'update {i}: flags'
    assert_state_equals_twin(tap.state(), twin)
    return got, tap


def test_surface_symbols_macros_and_state_layout():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    for name in ('vp_smoother_create', 'vp_smoother_destroy', 'vp_smoother_reset_stream', 'vp_smooth_update_stream', 'vp_smooth_update', 'vp_smoother_state_bytes',
                 'vp_smoother_download_state', 'vp_dbg_smooth_host'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and re.search(r'VP_API int %s\(' % name, hdr), name
    assert re.search(r'#define VP_HAS_SMOOTHER 1', hdr) and re.search(r'#define VP_SMOOTH_SLOTS %d\b' % SLOTS, hdr) and re.search(r'#define VP_SMOOTH_MAX_ROWS %d\b' % MAX_ROWS, hdr)
    for K, ns in ((1, 1), (17, 1), (133, 64), (1024, 2)):
        assert state_bytes(c_config(SmoothCfg(n_streams=ns), K)) == ns * (16 + 8 * SLOTS + SLOTS * K * 34) == ns * state_dtype(K).itemsize
    assert STATE_DTYPE == state_dtype(17) and STATE_DTYPE.fields['x_prev'][1] == 16 + 8 * SLOTS
    import easy_vitpose_amd.build as build
    assert 'smooth.hip' in build.SOURCES and build.SOURCE_FLAGS['smooth.hip'] == ['-ffp-contract=off'] and 'eurogeom.h' in build.HEADERS


@pytest.mark.parametrize('tag', GOLDEN['tags'].tolist())
def test_tap_equals_the_reference_bit_for_bit(tag):
    """one id on one stream: every output is float32(reference), the final x_prev / dx_prev are the reference's float64"""
    x, te, want = GOLDEN[tag + '_x'], GOLDEN[tag + '_te'], GOLDEN[tag + '_out']
    fps = float(GOLDEN['fps'][GOLDEN['tags'].tolist().index(tag)])
    K = x.shape[1]
    tap, twin = HostSmoother(K, SmoothCfg(fps=fps)), twin_of(K, SmoothCfg(fps=fps))
    conf = np.linspace(0, 1, K, dtype=np.float32)[:, None]
    for t in range(len(x)):
        row = np.concatenate([x[t], conf], axis=1)[None]
        for model in (tap, twin):
            out, flags = model.update(row, [3], t_e=te[t] if t else None)
            assert same_bits(out[0, :, :2], want[t]), f'frame {t}'
            assert same_bits(out[0, :, 2:], conf) and flags.tolist() == [0]
    st = tap.state()[0]
    assert st['id'][0] == 3 and st['last_seen'][0] == len(x) == st['frame_count'] and not st['fresh'][0].any()
    assert same_bits(st['x_prev'][0], GOLDEN[tag + '_xprev']) and same_bits(st['dx_prev'][0], GOLDEN[tag + '_dxprev'])
    assert (x[1:] <= 0).sum() > 0 and (want[1:][x[1:] <= 0] == -10).all(), 'the masked branch is entered'


def run_case(case):
    cfg_kw, calls = sequence(case)
    got, tap = tap_against_twin(case[1], cfg_kw, calls)
    flags = np.bitwise_or.reduce([f for _, f in got])
    changed = sum(not same_bits(o, c['kpts']) for (o, _), c in zip(got, [c for c in calls if 'reset' not in c]))
    assert changed >= 5, 'the sequences filter'
    return flags


@pytest.mark.parametrize('case', SEQUENCES, ids=tag_of)
def test_tap_equals_the_twin_on_the_sequences(case):
    run_case(case)


def test_the_sequences_reach_every_branch():
    seen = 0
    for case in SEQUENCES:
        seen |= int(np.bitwise_or.reduce(run_case(case)))
    assert seen & FLAG_DUP and seen & FLAG_BAD_ROW
    kinds = [c for case in SEQUENCES for c in sequence(case)[1]]
    assert any('reset' in c and c['reset'] is None for c in kinds) and any('reset' in c and c['reset'] == [0] for c in kinds)
    ups = [c for c in kinds if 'reset' not in c]
    assert any(len(c['ids']) == 0 for c in ups) and any(c['rank'] is not None and (c['rank'] < 0).any() for c in ups)
    assert any(c['step_mask'] is not None for c in ups) and any(c['stream'] is None for c in ups) and any((c['ids'] < 0).any() for c in ups)


def test_table_full_drops_the_129th_birth():
    cfg_kw, calls = table_full()
    got, tap = tap_against_twin(17, cfg_kw, calls)
    assert [f.tolist() for _, f in got] == [[FLAG_FULL], [FLAG_FULL]]
    assert same_bits(got[1][0][128], calls[1]['kpts'][128]) and not same_bits(got[1][0][127], calls[1]['kpts'][127])
    st = tap.state()[0]
    assert st['id'].tolist() == list(range(10, 138)) and (st['last_seen'] == 2).all()


def test_interleaved_streams_equal_the_twin():
    cfg_kw, calls = interleaved_streams()
    got, tap = tap_against_twin(17, cfg_kw, calls)
    assert all(f.tolist() == [0] * 64 for _, f in got) and (tap.state()['last_seen'][:, :2] == len(calls)).all()


@pytest.mark.parametrize('gap', [1, 2, 3])
def test_a_track_absent_for_g_frames_is_filtered_with_g_plus_1_times_t_e(gap):
    rng = np.random.default_rng(gap)
    K, te = 17, 0.5
    kp = rng.uniform(1, 300, (4, K, 3)).astype(np.float32)
    cfg = SmoothCfg(fps=25.0, max_age=3)
    a, b = HostSmoother(K, cfg), HostSmoother(K, cfg)
    for f in range(3):
        oa, _ = a.update(kp[f][None], [5], t_e=te)
        ob, _ = b.update(kp[f][None], [5], t_e=te)
    for _ in range(gap):   # a steps without the track (another id keeps the call non-empty), b does not step at all
        a.update(kp[0][None], [9], t_e=te)
    oa, _ = a.update(kp[3][None], [5], t_e=te)
    ob, _ = b.update(kp[3][None], [5], t_e=te * (gap + 1))
    assert same_bits(oa, ob) and not same_bits(oa, kp[3][None])
    assert same_bits(a.state()[0]['x_prev'][0], b.state()[0]['x_prev'][0]) and same_bits(a.state()[0]['dx_prev'][0], b.state()[0]['dx_prev'][0])
    # one frame more than max_age allows: the slot is freed and the row is a birth, returned unchanged
    c = HostSmoother(K, SmoothCfg(fps=25.0, max_age=gap - 1))
    c.update(kp[0][None], [5])
    for _ in range(gap):
        c.update(kp[0][:0], [])
    oc, _ = c.update(kp[3][None], [5])
    assert same_bits(oc, kp[3][None]) and c.state()[0]['fresh'][0].all() and c.state()[0]['last_seen'][0] == gap + 2
    d = HostSmoother(K, SmoothCfg(fps=25.0, max_age=gap))   # max_age stepped calls without a row are survived
    d.update(kp[0][None], [5])
    for _ in range(gap):
        d.update(kp[0][:0], [])
    od, _ = d.update(kp[3][None], [5])
    assert not same_bits(od, kp[3][None]) and not d.state()[0]['fresh'][0].any()


def test_restart_policy_and_in_place():
    K = 3
    cfgs = {m: SmoothCfg(fps=30.0, missing=m) for m in ('reference', 'restart')}
    rows = np.array([[[5, 7, .9], [0, 4, .8], [-2, 3, .7]], [[6, 8, .9], [2, 5, .8], [1, 4, .7]], [[7, 0, .9], [3, 6, .8], [2, 5, .7]], [[8, 9, .9], [4, 7, .8], [3, 6, .7]]],
                    np.float32)
    outs = {}
    for m, cfg in cfgs.items():
        tap = HostSmoother(K, cfg)
        outs[m] = [tap.update(r[None], [1])[0][0] for r in rows]
        assert same_bits(outs[m][0], rows[0]), 'a birth is returned unchanged, nothing masked'
    # born missing (0 and -2): the reference blends from them, restart takes the next sample as it is and is fresh again
    assert outs['restart'][1][1, 0] == 2 and outs['restart'][1][2, 0] == 1 and outs['reference'][1][1, 0] not in (2, -10)
    assert outs['reference'][2][0, 1] == -10 == outs['restart'][2][0, 1], 'masked this frame under both policies'
    assert outs['restart'][3][0, 1] == 9 and -10 < outs['reference'][3][0, 1] < 9
    # in place: out == kpts is legal through the tap
    lib, cfg = capi.load_library(), cfgs['reference']
    a, b = HostSmoother(K, cfg), HostSmoother(K, cfg)
    for r in rows:
        want, _ = a.update(r[None], [1])
        buf, ids, fl = r[None].copy(), np.array([1], np.int32), np.zeros(1, np.int32)
        capi.check(lib.vp_dbg_smooth_host(b.blob.ctypes.data, C.byref(b._c), buf.ctypes.data, ids.ctypes.data, None, None, 1, 1, None, buf.ctypes.data, fl.ctypes.data))
        assert same_bits(buf, want)
    assert a.state().tobytes() == b.state().tobytes()


def test_every_refusal_of_the_c_entries():
    lib = capi.load_library()
    K = 17
    good = dict(min_cutoff=1.7, beta=0.3, d_cutoff=30.0, max_age=1, n_streams=2, n_joints=K, max_rows=4, missing=0)
    blob = np.zeros(2, state_dtype(K))
    kp, ids, out, fl = np.ones((4, K, 3), np.float32), np.arange(4, dtype=np.int32), np.empty((4, K, 3), np.float32), np.zeros(2, np.int32)

    def call(cfg=None, kpts=kp.ctypes.data, idp=ids.ctypes.data, n=4, mask=3, te=None, outp=out.ctypes.data, null_cfg=False):
        c = capi.vp_smooth_cfg(**{**good, **(cfg or {})})
        tep = None if te is None else np.asarray(te, np.float64).ctypes.data
        rc = lib.vp_dbg_smooth_host(blob.ctypes.data, None if null_cfg else C.byref(c), kpts, idp, None, None, n, mask, tep, outp, fl.ctypes.data)
        return rc, capi.last_error()

    assert call()[0] == capi.VP_OK and call(n=0, kpts=None, idp=None, outp=None)[0] == capi.VP_OK, 'n = 0 with a mask is legal: it ages the streams'
    before = blob.tobytes()
    bad = [dict(null_cfg=True), dict(kpts=None), dict(idp=None), dict(outp=None), dict(n=-1), dict(n=5), dict(mask=4), dict(mask=1 << 63),
           dict(cfg=dict(n_streams=0)), dict(cfg=dict(n_streams=65)), dict(cfg=dict(n_joints=0)), dict(cfg=dict(n_joints=1025)), dict(cfg=dict(max_rows=0)),
           dict(cfg=dict(max_rows=MAX_ROWS + 1)), dict(cfg=dict(max_age=-1)), dict(cfg=dict(missing=2)), dict(cfg=dict(missing=-1)),
           dict(cfg=dict(min_cutoff=0.0)), dict(cfg=dict(min_cutoff=float('nan'))), dict(cfg=dict(min_cutoff=float('inf'))), dict(cfg=dict(d_cutoff=0.0)),
           dict(cfg=dict(d_cutoff=-1.0)), dict(cfg=dict(d_cutoff=float('inf'))), dict(cfg=dict(beta=-0.1)), dict(cfg=dict(beta=float('nan'))),
           dict(cfg=dict(beta=float('inf'))), dict(te=[1.0, 0.0]), dict(te=[float('nan'), 1.0]), dict(te=[1.0, float('inf')]), dict(te=[-1.0, 1.0])]
    for kw in bad:
        rc, why = call(**kw)
        assert rc == capi.VP_ERR_INVALID and why.startswith('smoother: '), (kw, rc, why)
    assert blob.tobytes() == before, 'a refused call touches nothing'
    assert call(cfg=dict(beta=0.0))[0] == capi.VP_OK
    b = C.c_int64(0)
    assert lib.vp_smoother_state_bytes(None, C.byref(b)) == capi.VP_ERR_INVALID
    assert lib.vp_smoother_state_bytes(C.byref(capi.vp_smooth_cfg(**good)), None) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_smooth_host(None, C.byref(capi.vp_smooth_cfg(**good)), kp.ctypes.data, ids.ctypes.data, None, None, 4, 3, None, out.ctypes.data, None) == capi.VP_ERR_INVALID
    for entry in (lib.vp_smoother_destroy,):
        assert entry(None) == capi.VP_ERR_INVALID
    assert lib.vp_smooth_update_stream(None, None, None, None, None, 0, 0, None, None, None, None) == capi.VP_ERR_INVALID
    assert lib.vp_smooth_update(None, None, None, None, None, 0, 0, None, None, None) == capi.VP_ERR_INVALID
    assert lib.vp_smoother_create(None, C.byref(capi.vp_smooth_cfg(**good)), C.byref(C.c_void_p())) == capi.VP_ERR_INVALID


def test_smoothcfg_validation_and_python_refusals():
    cfg = SmoothCfg()
    assert (cfg.min_cutoff, cfg.beta, cfg.d_cutoff, cfg.fps, cfg.max_age, cfg.n_streams, cfg.missing, cfg.max_rows) == (1.7, 0.3, 30.0, None, 1, 1, 'reference', 128)
    assert SmoothCfg(fps=25).d_cutoff == 25.0 and SmoothCfg(n_streams=3).max_rows == 384 and SmoothCfg(max_rows=5).max_rows == 5
    with pytest.raises(Exception):
        cfg.beta = 1.0   # frozen
    for kw in (dict(min_cutoff=0), dict(min_cutoff=float('nan')), dict(beta=-1), dict(beta=float('inf')), dict(d_cutoff=0), dict(fps=0), dict(fps=float('nan')),
               dict(max_age=-1), dict(max_age=1.5), dict(max_age=True), dict(n_streams=0), dict(n_streams=65), dict(missing='drop'), dict(missing=1),
               dict(max_rows=0), dict(max_rows=MAX_ROWS + 1), dict(min_cutoff='1')):
        with pytest.raises(ValueError):
            SmoothCfg(**kw)
    with pytest.raises(TypeError):
        c_config(dict(), 17)
    for K in (0, 1025):
        with pytest.raises(ValueError):
            c_config(cfg, K)
    tap = HostSmoother(17, cfg)
    with pytest.raises(ValueError):
        tap.update(np.zeros((2, 17, 3), np.float32), [1])
    with pytest.raises(ValueError):
        tap.update(np.zeros((1, 17, 3), np.float32), [1], stream=[0, 0])
    with pytest.raises(ValueError):
        tap.update(np.zeros((1, 17, 3), np.float32), [1], step_mask=[1])
    with pytest.raises(capi.VpError, match='max_rows'):
        tap.update(np.zeros((129, 17, 3), np.float32), np.arange(129))
    from easy_vitpose_amd import VitInference
    with pytest.raises((TypeError, ValueError), match='smooth'):
        VitInference({}, lambda img: np.empty((0, 5)), 's', dataset='coco', is_video=True, smooth='yes')
