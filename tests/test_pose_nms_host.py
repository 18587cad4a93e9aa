"""CPU: person scores and OKS pose NMS (csrc/posenms.h) through the host taps vp_dbg_pose_nms_host / vp_dbg_pose_oks(-1) -- the same functions the
kernel of vp_pose_nms_stream runs -- against the reference's own nms.py results (tests/golden/pose_nms.npz), the edge cases by construction, every
refusal of the C entries and of the Python layer.  The device is compared with this host model in tests/test_gpu_pose_nms.py."""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import os
import re

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.posenms import COCO17_SIGMAS, NMS_MAX_K, NMS_MAX_PER_FRAME, PoseNms, c_config, load_sigmas, resolve_sigmas
from pose_nms_cases import edge_cases, golden_case, golden_cases, nms_host, oks_tap, people, sigmas17, soft_bound, ulp_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_symbols_macros_and_abi_version():
    hdr = open(os.path.join(ROOT, 'include', 'vitpose_hip.h')).read()
    lib = capi.load_library()
    for name in ('vp_pose_nms_stream', 'vp_pose_nms', 'vp_dbg_pose_nms_host', 'vp_dbg_pose_oks'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r'VP_API\s+int\s+' + name + r'\s*\(', hdr), name
    assert re.search(r'#define\s+VP_HAS_POSE_NMS\s+1\b', hdr)
    assert re.search(r'#define\s+VP_NMS_MAX_PER_FRAME\s+1024\b', hdr) and NMS_MAX_PER_FRAME == 1024
    assert re.search(r'#define\s+VP_NMS_MAX_K\s+256\b', hdr) and NMS_MAX_K == 256
    assert re.search(r'#define\s+VP_ABI_VERSION\s+4\b', hdr) and lib.vp_abi_version() == 4
    assert C.sizeof(capi.vp_pose_nms_cfg) == 32   # 2 floats, 4 int32, one pointer


@pytest.mark.parametrize('K,n,vi', sorted({(k, n, vi) for k, n, _, vi in golden_cases()}))
def test_pairwise_oks_against_the_reference(K, n, vi):
    """Equal, or one float32 step apart: the fp64 sum in joint order differs from numpy's pairwise sum by a few 2^-52, which shows only across a
    float32 rounding boundary."""
    g = golden_case(K, n, 0, vi)
    got = oks_tap(-1, g['kpts'], g['p9'], PoseNms(vis_thr=g['vis']), g['sigmas'])
    d = ulp_diff(got, g['oks'])
    print(f'K={K} n={n} vis={g["vis"]}: {int((d > 0).sum())} of {d.size} OKS values differ, max {int(d.max())} ulp')
    assert d.max() <= 1


@pytest.mark.parametrize('K,n,ti,vi', golden_cases())
def test_hard_and_soft_nms_against_the_reference(K, n, ti, vi):
    g = golden_case(K, n, ti, vi)
    cfg = PoseNms(oks_thr=g['thr'], vis_thr=g['vis'], max_dets=g['max_dets'])
    score, rank, count = nms_host(g['kpts'], g['box'], g['p9'], g['n_frames'], cfg, g['sigmas'])
    assert np.array_equal(rank, g['hard_rank'])                       # oks_nms's keep list, in its order
    assert np.array_equal(score.view(np.int32), g['score'].view(np.int32))
    assert count.tolist() == [int(((g['p9'][:, 0] == f) & (g['hard_rank'] >= 0)).sum()) for f in range(g['n_frames'])]
    score, rank, count = nms_host(g['kpts'], g['box'], g['p9'], g['n_frames'], dataclasses.replace(cfg, soft=True), g['sigmas'])
    assert np.array_equal(rank, g['soft_rank'])                       # soft_oks_nms's keep list, in its order
    picked = rank >= 0
    rel = np.abs(score[picked].astype(np.float64) - g['soft_score'][picked]) / g['soft_score'][picked]
    bound = soft_bound(rank[picked], g['thr'])
    print(f'K={K} n={n} thr={g["thr"]} vis={g["vis"]}: soft score max rel err {rel.max():.2e}, max err / bound {np.max(rel / np.maximum(bound, 1e-300)):.3f}')
    assert (rel <= bound).all()
    assert np.array_equal(score[~picked].view(np.int32), g['score'][~picked].view(np.int32))   # never picked: the instance score stays
    assert count.tolist() == [int(((g['p9'][:, 0] == f) & picked).sum()) for f in range(g['n_frames'])]


def test_empty_call_one_row_and_identical_rows():
    cfg, sig = PoseNms(), sigmas17()
    score, rank, count = nms_host(np.zeros((0, 17, 3), np.float32), np.zeros(0), np.zeros((0, 9)), 3, cfg, sig)
    assert count.tolist() == [0, 0, 0]
    lib = capi.load_library()
    c, keep = c_config(cfg, sig)
    assert lib.vp_dbg_pose_nms_host(None, 0, 17, None, 1, None, None, 0, C.byref(c), None, None, None) == capi.VP_OK   # n = 0: no pointer is needed
    cases = edge_cases()
    kp, bs, p9, nf, _ = cases['one_row']
    score, rank, count = nms_host(kp, bs, p9, nf, cfg, sig)
    assert rank.tolist() == [0] and count.tolist() == [1]
    vis = [float(c) for c in kp[0, :, 2] if c > np.float32(0.2)]
    assert score[0] == np.float32(sum(vis, 0.0) / len(vis) * float(bs[0]))   # fp64, joint order
    kp, bs, p9, nf, _ = cases['two_identical']
    for soft in (False, True):
        score, rank, count = nms_host(kp, bs, p9, nf, PoseNms(soft=soft), sig)
        assert score[0] == score[1] or soft
        assert rank[0] == 0, 'equal scores go to the lower row'
        assert rank[1] == (1 if soft else -1) and count.tolist() == [2 if soft else 1]
    assert oks_tap(-1, kp, p9, cfg, sig)[0, 1] == 1.0


def test_frames_interleaved_equal_the_frames_alone_and_empty_frames():
    sig = sigmas17()
    cases = edge_cases()
    kp, bs, p9, nf, _ = cases['three_frames_interleaved']
    for cfg in (PoseNms(oks_thr=0.5), PoseNms(oks_thr=0.5, soft=True, max_dets=3)):
        score, rank, count = nms_host(kp, bs, p9, nf, cfg, sig)
        assert (rank >= 0).sum() == count.sum() and (rank < 0).any()
        for f in range(nf):
            rows = np.flatnonzero(p9[:, 0] == f)
            assert len(rows) > 3
            q = p9[rows].copy()
            q[:, 0] = 0
            s1, r1, c1 = nms_host(kp[rows], bs[rows], q, 1, cfg, sig)
            assert np.array_equal(r1, rank[rows]) and np.array_equal(s1.view(np.int32), score[rows].view(np.int32)) and c1[0] == count[f]
            if cfg.soft:   # max_dets = 3: exactly three picks, ranks 0..2
                assert count[f] == 3 and sorted(rank[rows][rank[rows] >= 0].tolist()) == [0, 1, 2]
    kp, bs, p9, nf, _ = cases['frames_without_rows']
    score, rank, count = nms_host(kp, bs, p9, nf, PoseNms(), sig)
    assert count[[0, 1, 3]].tolist() == [0, 0, 0] and count[2] == (rank >= 0).sum() > 0


def test_bad_rows_strided_scores_and_invisible_people():
    sig = sigmas17()
    cases = edge_cases()
    kp, bs, p9, nf, st = cases['bad_status_and_frames']
    score, rank, count = nms_host(kp, bs, p9, nf, PoseNms(), sig, status=st)
    bad = [1, 6, 3, 8]
    assert (rank[bad] == -1).all()
    good = np.setdiff1d(np.arange(len(kp)), bad)
    s1, r1, c1 = nms_host(kp[good], bs[good], p9[good], nf, PoseNms(), sig)
    assert np.array_equal(r1, rank[good]) and np.array_equal(c1, count), 'bad rows take no part'
    # the detector's [n, 6] tensor in place: d_boxes + 4 with stride 6
    det = np.zeros((len(kp), 6), np.float32)
    det[:, 4] = bs
    s6, r6, _ = nms_host(kp, det.reshape(-1)[4:], p9, nf, PoseNms(), sig, status=st, score_stride=6)
    assert np.array_equal(s6.view(np.int32), score.view(np.int32)) and np.array_equal(r6, rank)
    kp, bs, p9, nf, _ = cases['no_visible_joint']
    score, rank, count = nms_host(kp, bs, p9, nf, PoseNms(), sig)
    assert score[2] == 0.0 and rank[2] >= 0
    oks = oks_tap(-1, kp, p9, PoseNms(), sig)
    assert (oks[:, 2] == 0.0).all(), 'the gate reads the CANDIDATE: a row without a visible joint has OKS 0 against every pick'
    assert oks[2, 2] == 0.0 and oks[2, 0] > 0.0
    s0, _, _ = nms_host(kp, bs, p9, nf, PoseNms(vis_thr=None), sig)
    assert abs(s0[2] - 0.1 * bs[2]) < 1e-6, 'vis_thr off: every joint counts'


def test_per_frame_cap():
    sig = sigmas17()
    rng = np.random.default_rng(9)
    for n0 in (NMS_MAX_PER_FRAME, NMS_MAX_PER_FRAME + 1):
        kp0, bs0, p0 = people(n0, seed=10, dup=0.0)
        kp1, bs1, p1 = people(5, seed=11)
        p1[:, 0] = 1
        order = rng.permutation(n0 + 5)
        kp, bs, p9 = np.concatenate([kp0, kp1])[order], np.concatenate([bs0, bs1])[order], np.concatenate([p0, p1])[order]
        score, rank, count = nms_host(kp, bs, p9, 2, PoseNms(), sig)
        on0 = p9[:, 0] == 0
        s1, r1, c1 = nms_host(kp[~on0], bs[~on0], p9[~on0], 2, PoseNms(), sig)
        assert np.array_equal(rank[~on0], r1) and count[1] == c1[1] > 0, 'the other frame of the call is still processed'
        if n0 > NMS_MAX_PER_FRAME:
            assert (rank[on0] == -2).all() and count[0] == 0
            sx, _, _ = nms_host(kp[on0][:7], bs[on0][:7], p9[on0][:7], 1, PoseNms(), sig)
            assert np.array_equal(score[on0][:7].view(np.int32), sx.view(np.int32)), 'its rows still get their instance score'
        else:
            assert (rank[on0] >= -1).all() and count[0] == (rank[on0] >= 0).sum() > 900
            kept = np.sort(rank[on0][rank[on0] >= 0])
            assert np.array_equal(kept, np.arange(count[0]))


def _rc(cfg_c, n=2, k=17, stride=1, n_frames=1, null=None):
    lib = capi.load_library()
    kp, bs, p9 = people(2, seed=3)
    score, rank, count = np.zeros(2, np.float32), np.zeros(2, np.int32), np.zeros(4, np.int32)
    ptr = {'kpts': kp.ctypes.data, 'box': bs.ctypes.data, 'p9': p9.ctypes.data, 'score': score.ctypes.data, 'rank': rank.ctypes.data}
    if null:
        ptr[null] = None
    return lib.vp_dbg_pose_nms_host(ptr['kpts'], n, k, ptr['box'], stride, ptr['p9'], None, n_frames, None if cfg_c is None else C.byref(cfg_c),
                                    ptr['score'], ptr['rank'], count.ctypes.data)


def test_every_refusal_of_the_c_entries():
    sig = sigmas17()
    good, keep = c_config(PoseNms(), sig)
    assert _rc(good) == capi.VP_OK
    for null in ('kpts', 'box', 'p9', 'score', 'rank'):
        assert _rc(good, null=null) == capi.VP_ERR_INVALID, null
    assert 'pose nms' in capi.last_error(None)
    assert _rc(None) == capi.VP_ERR_INVALID
    assert _rc(good, k=0) == capi.VP_ERR_INVALID and _rc(good, k=16) == capi.VP_ERR_INVALID   # n_sigmas != k
    big = np.full(257, 0.05, np.float32)
    c257 = capi.vp_pose_nms_cfg(0.9, 0.2, 1, 0, 20, 257, big.ctypes.data)
    assert _rc(c257, k=257) == capi.VP_ERR_INVALID
    for bad_sigma in (0.0, -0.1, np.nan, np.inf):
        s = sig.copy()
        s[5] = bad_sigma
        c = capi.vp_pose_nms_cfg(0.9, 0.2, 1, 0, 20, 17, s.ctypes.data)
        assert _rc(c) == capi.VP_ERR_INVALID, bad_sigma
    assert _rc(capi.vp_pose_nms_cfg(0.9, 0.2, 1, 0, 20, 17, None)) == capi.VP_ERR_INVALID
    for thr in (0.0, -0.5, 1.5, np.nan):
        assert _rc(capi.vp_pose_nms_cfg(thr, 0.2, 1, 0, 20, 17, sig.ctypes.data)) == capi.VP_ERR_INVALID, thr
    assert _rc(capi.vp_pose_nms_cfg(1.0, 0.2, 1, 0, 20, 17, sig.ctypes.data)) == capi.VP_OK
    assert _rc(capi.vp_pose_nms_cfg(0.9, 0.2, 1, 1, 0, 17, sig.ctypes.data)) == capi.VP_ERR_INVALID   # soft with max_dets < 1
    assert _rc(capi.vp_pose_nms_cfg(0.9, 0.2, 1, 0, 0, 17, sig.ctypes.data)) == capi.VP_OK            # hard: max_dets is not read
    assert _rc(good, n_frames=0) == capi.VP_ERR_INVALID
    assert _rc(good, stride=0) == capi.VP_ERR_INVALID
    assert _rc(good, n=-1) == capi.VP_ERR_INVALID
    # the pairwise tap and the handle entries refuse the same way (a NULL handle is refused before anything else)
    lib = capi.load_library()
    kp, bs, p9 = people(2, seed=3)
    out = np.zeros((2, 2), np.float32)
    assert lib.vp_dbg_pose_oks(-1, kp.ctypes.data, 2, 16, p9.ctypes.data, C.byref(good), out.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_pose_oks(-1, None, 2, 17, p9.ctypes.data, C.byref(good), out.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_pose_nms_stream(None, None, 0, 17, None, 1, None, None, 0, C.byref(good), None, None, None, None) == capi.VP_ERR_INVALID
    assert lib.vp_pose_nms(None, None, 0, 17, None, 1, None, None, 0, C.byref(good), None, None, None) == capi.VP_ERR_INVALID


def test_resolve_sigmas_and_posenms_refusals(tmp_path):
    assert np.array_equal(resolve_sigmas('coco', 17, None), np.asarray(COCO17_SIGMAS, np.float32))
    for dataset, k in (('wholebody', 133), ('coco_25', 25), ('mpii', 16), ('ap10k', 17), ('aic', 14), ('custom', 17)):
        with pytest.raises(ValueError, match=dataset):
            resolve_sigmas(dataset, k, None)
        assert resolve_sigmas(dataset, k, [0.05] * k).shape == (k,)
    with pytest.raises(ValueError, match='16 sigmas'):
        resolve_sigmas('coco', 17, [0.05] * 16)
    with pytest.raises(ValueError):
        resolve_sigmas('mpii', 16, [0.05] * 15 + [0.0])
    assert PoseNms() == PoseNms(0.9, 0.2, False, 20, None)
    with pytest.raises(dataclasses.FrozenInstanceError):
        PoseNms().oks_thr = 0.5
    for kw in (dict(oks_thr=0.0), dict(oks_thr=1.01), dict(oks_thr='0.9'), dict(vis_thr=float('nan')), dict(max_dets=0), dict(max_dets=2.5),
               dict(sigmas=[]), dict(sigmas=[0.1, -1.0]), dict(sigmas=[0.05] * 257)):
        with pytest.raises(ValueError):
            PoseNms(**kw)
    assert PoseNms(sigmas=[0.05, 0.1]).sigmas == (0.05, 0.1) and hash(PoseNms(sigmas=[0.05]))
    with pytest.raises(TypeError):
        c_config({'oks_thr': 0.9}, sigmas17())
    f = tmp_path / 's.json'
    f.write_text(json.dumps([0.05] * 16))
    assert load_sigmas(str(f)) == (0.05,) * 16
    for bad in ('x', {'sigmas': [0.1]}, [0.1, True]):
        f.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            load_sigmas(str(f))
    # numpy scalars are numbers, a bool is not
    got = PoseNms(oks_thr=np.float32(0.5), vis_thr=np.float32(0.25), max_dets=np.int64(7))
    assert got == PoseNms(0.5, 0.25, False, 7) and type(got.oks_thr) is float and type(got.max_dets) is int
    for kw in (dict(oks_thr=True), dict(vis_thr=False), dict(max_dets=True)):
        with pytest.raises(ValueError):
            PoseNms(**kw)


def test_vitinference_and_cli_argument_checks(tmp_path):
    """Raised from the arguments alone, before a device or a checkpoint is touched."""
    from easy_vitpose_amd import VitInference
    from easy_vitpose_amd.cli import build_parser, pose_nms_argument
    from helpers import weights
    det = lambda img: np.empty((0, 5))   # noqa: E731
    _, sd, _ = weights('s', 'mpii')
    with pytest.raises(ValueError, match='mpii'):
        VitInference(sd, det, 's', dataset='mpii', pose_nms=PoseNms())
    with pytest.raises(ValueError, match='15 sigmas'):
        VitInference(sd, det, 's', dataset='mpii', pose_nms=PoseNms(sigmas=[0.05] * 15))
    _, sd, _ = weights('s', 'coco')
    with pytest.raises(TypeError, match='PoseNms'):
        VitInference(sd, det, 's', dataset='coco', pose_nms=0.9)
    ap = build_parser()
    base = ['--input', 'clip.npy', '--synthetic', 's', '--boxes', 'b.json']
    assert pose_nms_argument(ap.parse_args(base)) is None
    assert pose_nms_argument(ap.parse_args(base + ['--pose-nms'])) == PoseNms()
    f = tmp_path / 's.json'
    f.write_text(json.dumps([0.05] * 17))
    got = pose_nms_argument(ap.parse_args(base + ['--pose-nms', '0.5', '--soft-nms', '--vis-thr', '0.3', '--sigmas', str(f)]))
    assert got == PoseNms(oks_thr=0.5, vis_thr=0.3, soft=True, sigmas=(0.05,) * 17)
    with pytest.raises(ValueError, match='--pose-nms'):
        pose_nms_argument(ap.parse_args(base + ['--soft-nms']))
