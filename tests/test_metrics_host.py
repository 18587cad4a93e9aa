"""CPU: the metrics stage's contract (csrc/metricsgeom.h) through the host tap vp_dbg_metrics_host -- against the numpy twin on every byte, against the reference's
own outputs (tests/golden/metrics.npz, written by tests/golden/make_golden_metrics.py), and against anchors written as literals.  The device is tested against
this tap in tests/test_gpu_metrics.py."""
from __future__ import annotations

import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd import build
from easy_vitpose_amd import devmetrics as dm
from easy_vitpose_amd.devmetrics import MetricsCfg, finish, metrics_numpy, metrics_tap, new_state
import metrics_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['vp_metrics_create', 'vp_metrics_destroy', 'vp_metrics_reset_stream', 'vp_metrics_update_stream', 'vp_metrics_update', 'vp_metrics_snapshot_stream',
       'vp_metrics_state_bytes', 'vp_metrics_download_state', 'vp_dbg_metrics_host']
CASES = mc.host_cases()
F32 = np.float32


def test_surface():
    lib = capi.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes and re.search(r'VP_API int %s\(' % name, hdr), name
    assert re.search(r'#define\s+VP_HAS_METRICS\s+1\b', hdr) and re.search(r'#define\s+VP_METRICS_MAX_ROWS\s+8192\b', hdr) and dm.MAX_ROWS == 8192
    assert re.search(r'#define\s+VP_ABI_VERSION\s+4\b', hdr) and lib.vp_abi_version() == 4
    assert C.sizeof(capi.vp_metrics_cfg) == 64
    assert 'metrics.hip' in build.SOURCES and build.SOURCE_FLAGS['metrics.hip'] == ['-ffp-contract=off'] and 'metricsgeom.h' in build.HEADERS


def both(cs, states=None):
    """one update through the tap and through the twin -> ((state, dist, oks) of the tap, the same of the twin)"""
    a, b = states if states else (new_state(cs['cfg']), new_state(cs['cfg']))
    da, oa = metrics_tap(a, cs['cfg'], **mc.inputs(cs))
    db, ob = metrics_numpy(b, cs['cfg'], **mc.inputs(cs))
    return (a, da, oa), (b, db, ob)


def same_bytes(x, y):
    return x.tobytes() == y.tobytes()


@pytest.mark.parametrize('name', sorted(CASES))
def test_tap_equals_the_numpy_twin_on_every_byte(name):
    cs = CASES[name]
    (a, da, oa), (b, db, ob) = both(cs)
    (a, da2, oa2), (b, db2, ob2) = both(cs, (a, b))   # a second call on the same state: accumulation
    for f in a.dtype.names:
        assert same_bytes(a[f], b[f]), f'{name}: state field {f}'
    assert same_bytes(da, db) and same_bytes(oa, ob) and same_bytes(da, da2) and same_bytes(oa, oa2), name
    assert int(a['calls']) == 2 and int(a['rows']) == 2 * len(cs['pred'])
    if name.startswith('bad_values'):
        assert int(a['nonfinite']) > 0 and math.isnan(finish(a, cs['cfg']).epe)


def test_every_combination_of_null_inputs():
    for name, cs in mc.null_combos().items():
        (a, da, oa), (b, db, ob) = both(cs)
        assert same_bytes(a, b) and same_bytes(da, db) and same_bytes(oa, ob), name
        if cs['area'] is None:
            assert int(a['oks_rows']) == 0 and (oa == -1).all(), name
        if cs['rank'] is None and cs['set'] is None:
            assert int(a['counted']) == len(cs['pred']), name


def test_the_cap_of_a_call_at_133_joints():
    cs = mc.big_case()
    (a, da, oa), (b, db, ob) = both(cs)
    assert same_bytes(a, b) and same_bytes(da, db) and same_bytes(oa, ob)


# ---------------------------------------------------------------- against the reference
SPLITS = (1, 63, 64, 65, 129)


def feed(cfg, g, tag, update):
    """the data set in calls of 1, 63, 64, 65, 129 rows and the rest -> (dist, oks) concatenated"""
    pred, gt, norm, area = (g[f'{tag}_{k}'] for k in ('pred', 'gt', 'norm', 'area'))
    at, dist, oks = 0, [], []
    for size in SPLITS + (len(pred),):
        hi = min(len(pred), at + size)
        d, o = update(pred=pred[at:hi], gt=gt[at:hi], norm=norm[at:hi], area=area[at:hi])
        dist.append(d)
        oks.append(o)
        at = hi
    assert at == len(pred)
    return np.concatenate(dist), np.concatenate(oks)


def golden_cfg(g, K):
    return MetricsCfg(n_joints=K, pck_thr=tuple(g['pck_thrs']), auc_steps=int(g['auc_steps']), auc_norm=float(g['auc_norm']), sigmas=tuple(g[f'k{K}_sigmas']))


def check_against_reference(g, K, state, dist, oks, oks_ulp):
    """`state`, `dist`, `oks` of the data set fed in pieces, against the reference's stored outputs"""
    tag = f'k{K}'
    cfg = golden_cfg(g, K)
    assert same_bytes(dist, g[f'{tag}_dist'])                                    # _calc_distances bit for bit
    res = finish(state, cfg)
    for i in range(len(cfg.pck_thr)):
        acc, avg, cnt = res.pck(i)
        assert np.array_equal(acc, g[f'{tag}_pck{i}_acc']) and avg == g[f'{tag}_pck{i}_avg'] and cnt == g[f'{tag}_pck{i}_cnt'], i
    assert res.auc == g[f'{tag}_auc']
    assert res.nonfinite == 0
    # keypoint_epe's distances, by its own expression (_calc_distances with ones): float32 norm of the float32 difference, -1 where masked
    d = g[f'{tag}_pred'][:, :, :2] - g[f'{tag}_gt'][:, :, :2]
    dist_px = np.where(g[f'{tag}_gt'][:, :, 2] > 0, np.linalg.norm(d / np.ones((len(d), 1, 2), F32), axis=-1), F32(-1))
    assert dist_px.dtype == F32
    for name, got, ref32, arr in (('epe', res.epe, g[f'{tag}_epe'], dist_px), ('nme', res.nme, g[f'{tag}_nme'], g[f'{tag}_dist'])):
        valid = arr[arr != -1]
        terms = len(valid)
        exact = math.fsum(valid.astype(np.float64)) / max(1, terms)
        rel_exact, rel_ref = abs(got - exact) / exact, abs(got - float(ref32)) / float(ref32)
        print(f'K={K} {name}: {got!r}, fsum of the reference distances {exact!r} (rel {rel_exact:.2e}, bound {terms * 2.0 ** -53:.2e}), '
              f'the reference {float(ref32)!r} (rel {rel_ref:.2e}, bound {(21 + math.ceil(math.log2(terms))) * 2.0 ** -24:.2e})')
        assert rel_exact <= terms * 2.0 ** -53
        assert rel_ref <= (21 + math.ceil(math.log2(terms))) * 2.0 ** -24
    ref = g[f'{tag}_oks']
    assert np.array_equal(oks == -1, ref == -1)
    d = mc.ulp_diff(oks, ref)
    print(f'K={K}: {int((d > 0).sum())} of {d.size} OKS values differ from the reference, max {int(d.max())} float32 step(s)')
    assert d.max() <= oks_ulp
    have = ref[ref != -1]
    assert res.oks_rows == len(have)
    assert [int(h) for h in state['oks_hits']] == [int((have >= F32(0.5 + 0.05 * t)).sum()) for t in range(10)]


@pytest.mark.parametrize('K', [17, 133])
def test_against_the_reference(K):
    """OKS: the tap adds exp() terms in joint order, numpy's sum is pairwise from eight terms on and its exp is another implementation than the C library's: the
    fp64 means differ by a few 2^-52, which shows only across a float32 rounding boundary -- equal, or one float32 step apart (the bound of the NMS goldens)."""
    g = mc.golden()
    cfg = golden_cfg(g, K)
    state = new_state(cfg)
    dist, oks = feed(cfg, g, f'k{K}', lambda **kw: metrics_tap(state, cfg, **kw))
    assert int(state['calls']) == 6 and int(state['rows']) == int(state['counted']) == len(dist)
    check_against_reference(g, K, state, dist, oks, oks_ulp=1)


# ---------------------------------------------------------------- anchors as literals
def test_anchor_three_four_five():
    gt = np.zeros((3, 2, 3), F32)
    gt[:, :, 2] = 1
    gt[:, :, :2] = [[10, 20], [30, 40]]
    pred = gt.copy()
    pred[:, :, 0] += 3
    pred[:, :, 1] += 4
    norm = np.full((3, 2), 10, F32)
    cfg = MetricsCfg(n_joints=2, pck_thr=(0.5, 0.51), auc_steps=0)
    st = new_state(cfg)
    dist, oks = metrics_tap(st, cfg, pred, gt, norm=norm)
    assert (dist == F32(0.5)).all() and (oks == -1).all()
    assert st['pck_hits'].tolist() == [[0, 0], [3, 3]]           # strict: no hit at 0.5, a hit at 0.51
    assert st['valid_norm'].tolist() == [3, 3] and st['valid_px'].tolist() == [3, 3]
    assert st['sum_norm'].tolist() == [1.5, 1.5] and st['sum_px'].tolist() == [15.0, 15.0]
    r = finish(st, cfg)
    assert r.epe == 5.0 and r.nme == 0.5 and r.pck(0)[1] == 0 and r.pck(1)[1] == 1.0 and r.pck(1)[2] == 2


def order_anchor(n):
    """lane 0 of every block holds a pixel distance of 2^60, every other lane 128"""
    gt = np.zeros((n, 1, 3), F32)
    gt[:, 0, 2] = 1
    pred = gt.copy()
    pred[:, 0, 1] = 128
    pred[0::64, 0, 1] = 2.0 ** 60
    return pred, gt


def test_anchor_the_tree_keeps_what_a_sequential_sum_loses():
    cfg = MetricsCfg(n_joints=1, pck_thr=(), auc_steps=0)
    pred, gt = order_anchor(64)
    st = new_state(cfg)
    metrics_tap(st, cfg, pred, gt)
    seq = 2.0 ** 60
    for _ in range(63):
        seq += 128.0
    assert seq == 2.0 ** 60                                       # ulp(2^60) = 256: a sequential sum loses every 128
    # the tree: lane 0 + lane 1 = 2^60 + 128 ties to even = 2^60 (the one 128 it loses); the other 62 lanes arrive as partial sums of whole ulps
    assert st['sum_px'][0] == 2.0 ** 60 + 62 * 128 == 1152921504606854912.0
    tw = new_state(cfg)
    metrics_numpy(tw, cfg, pred, gt)
    assert same_bytes(st, tw)


def test_anchor_blocks_add_in_ascending_order():
    cfg = MetricsCfg(n_joints=1, pck_thr=(), auc_steps=0)
    # block 0 as above: P(0) = 2^60 + 7936; block 1 holds one distance of 96 (P(1) = 96), block 2 one row of 96 (P(2) = 96).  Ascending, each 96 = 0.375 ulp is
    # lost on its own: ((0 + P(0)) + P(1)) + P(2) = P(0).  Any order that adds P(1) and P(2) first keeps them: P(0) + 192 rounds up to P(0) + 256.
    pred, gt = order_anchor(64)
    gt = np.concatenate([gt, np.repeat(gt[:1], 65, axis=0)])
    tail = gt[64:].copy()
    tail[0, 0, 1] = tail[64, 0, 1] = 96
    pred = np.concatenate([pred, tail])
    st = new_state(cfg)
    metrics_tap(st, cfg, pred, gt)
    p0 = 2.0 ** 60 + 7936
    assert (p0 + 96.0) + 96.0 == p0 and p0 + (96.0 + 96.0) == p0 + 256
    assert st['sum_px'][0] == p0 and int(st['valid_px'][0]) == 129
    tw = new_state(cfg)
    metrics_numpy(tw, cfg, pred, gt)
    assert same_bytes(st, tw)


# ---------------------------------------------------------------- misc
def test_three_calls_equal_one_call_on_the_concatenation_for_every_integer_word():
    cs = mc.case(600, 64 + 128 + 70, 17)
    cfg = cs['cfg']
    one, three = new_state(cfg), new_state(cfg)
    metrics_tap(one, cfg, **mc.inputs(cs))
    for lo, hi in ((0, 64), (64, 192), (192, 262)):
        part = {k: (v[lo:hi] if isinstance(v, np.ndarray) else v) for k, v in mc.inputs(cs).items()}
        metrics_tap(three, cfg, **part)
    for f in one.dtype.names:
        if f in ('calls', 'sum_norm', 'sum_px', 'oks_sum'):
            continue
        assert np.array_equal(one[f], three[f]), f
    assert int(one['calls']) == 1 and int(three['calls']) == 3
    # the sums see another association (state + call_sum per call): equal to a few ulps only
    assert np.allclose(one['sum_norm'], three['sum_norm'], rtol=1e-13, atol=0) and np.allclose(one['sum_px'], three['sum_px'], rtol=1e-13, atol=0)
    three[...] = np.zeros((), three.dtype)                          # reset: zeroed = new
    metrics_tap(three, cfg, **mc.inputs(cs))
    assert same_bytes(one, three)


def test_state_bytes_formula():
    for K, P, A in ((1, 0, 0), (17, 3, 20), (133, 8, 32), (256, 4, 20)):
        cfg = MetricsCfg(n_joints=K, pck_thr=tuple([0.1] * P), auc_steps=A)
        assert dm.state_bytes(cfg) == 8 * (24 + K * (4 + P + A)) == new_state(cfg).nbytes


def test_norm_from_boxes():
    rows = np.array([[10, 20, 110, 220, 0.9, 0], [0, 0, 5, 7, 0.5, 1]], F32)
    assert dm.norm_from_boxes(rows).tolist() == [[200, 100], [7, 5]] and dm.norm_from_boxes(rows).dtype == F32


def test_every_refusal_by_message():
    lib = capi.load_library()
    kp = np.zeros((2, 17, 3), F32)
    sig = np.full(17, 0.05, F32)

    def call(n=2, pred=kp, gt=kp, sigmas=sig, state=True, null_cfg=False, **kw):
        f = dict(auc_norm=30.0, pck_thr=(0.05,), vis_thr=0.0, n_joints=17, n_pck=1, auc_steps=20, use_oks=1)
        f.update(kw)
        c = capi.vp_metrics_cfg(f['auc_norm'], (C.c_float * 8)(*f['pck_thr']), f['vis_thr'], f['n_joints'], f['n_pck'], f['auc_steps'], f['use_oks'], 0)
        st = np.full(8 * (24 + 256 * 44), 7, np.uint8)
        rc = lib.vp_dbg_metrics_host(st.ctypes.data if state else None, None if null_cfg else C.byref(c), None if sigmas is None else sigmas.ctypes.data,
                                     None if pred is None else pred.ctypes.data, None if gt is None else gt.ctypes.data, None, None, None, None, 0, n, None, None)
        assert rc != capi.VP_OK or state
        if rc != capi.VP_OK:
            assert (st == 7).all()                                  # a refusal writes nothing
        return rc, capi.last_error()
    bad_sig = sig.copy()
    bad_sig[5] = 0
    nan_sig = sig.copy()
    nan_sig[16] = np.nan
    for kw, msg in ((dict(null_cfg=True), 'null cfg'), (dict(pred=None), 'null pred or gt with n > 0'), (dict(gt=None), 'null pred or gt with n > 0'),
                    (dict(n=-1), 'n = -1 outside 0..8192'), (dict(n=8193), 'n = 8193 outside 0..8192'), (dict(n_joints=0), 'n_joints = 0 outside 1..256'),
                    (dict(n_joints=257), 'n_joints = 257 outside 1..256'), (dict(n_pck=9), 'n_pck = 9 outside 0..8'), (dict(n_pck=-1), 'n_pck = -1 outside 0..8'),
                    (dict(auc_steps=33), 'auc_steps = 33 outside 0..32'), (dict(auc_steps=-1), 'auc_steps = -1 outside 0..32'),
                    (dict(pck_thr=(math.inf,)), 'pck_thr[0] not finite'), (dict(pck_thr=(0.1, math.nan), n_pck=2), 'pck_thr[1] not finite'),
                    (dict(vis_thr=math.nan), 'vis_thr not finite'), (dict(auc_norm=0.0), 'auc_norm not finite or <= 0 with auc_steps > 0'),
                    (dict(auc_norm=math.inf), 'auc_norm not finite or <= 0 with auc_steps > 0'), (dict(auc_norm=-2.0), 'auc_norm not finite or <= 0 with auc_steps > 0'),
                    (dict(sigmas=None), 'use_oks without sigmas'), (dict(sigmas=bad_sig), 'sigma[5] not finite or <= 0'),
                    (dict(sigmas=nan_sig), 'sigma[16] not finite or <= 0'), (dict(state=False), 'null state')):
        rc, why = call(**kw)
        assert rc == capi.VP_ERR_INVALID and why == 'metrics: ' + msg, (kw, why)
    # what is NOT refused: a threshold beyond n_pck, auc_norm without AUC, no sigmas without OKS, n = 0 without rows
    assert call(pck_thr=(0.1, math.nan))[0] == capi.VP_OK and call(auc_norm=0.0, auc_steps=0)[0] == capi.VP_OK
    assert call(sigmas=None, use_oks=0)[0] == capi.VP_OK and call(n=0, pred=None, gt=None)[0] == capi.VP_OK
    b = C.c_int64(0)
    assert lib.vp_metrics_state_bytes(None, C.byref(b)) == capi.VP_ERR_INVALID and capi.last_error() == 'metrics: null cfg'
    with pytest.raises(ValueError, match='n_joints'):
        MetricsCfg(n_joints=300)
    with pytest.raises(ValueError, match='sigmas'):
        MetricsCfg(n_joints=17, sigmas=(0.1,) * 16)
    with pytest.raises(ValueError, match='norm'):
        metrics_tap(new_state(MetricsCfg()), MetricsCfg(), kp, kp, norm=np.ones((3, 2), F32))


def test_a_call_without_rows_counts_a_call():
    cfg = MetricsCfg()
    st = new_state(cfg)
    dist, oks = metrics_tap(st, cfg, np.zeros((0, 17, 3), F32), np.zeros((0, 17, 3), F32))
    assert int(st['calls']) == 1 and dist.shape == (0, 17) and oks.shape == (0,)
    st['calls'] = 0
    assert st.tobytes() == bytes(st.nbytes)
    r = finish(st, cfg)
    assert r.epe == 0 and r.nme == 0 and r.auc == 0 and r.pck(0)[1:] == (0, 0) and (r.pck(0)[0] == -1).all() and math.isnan(r.oks_mean)
