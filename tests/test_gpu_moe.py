"""ViTPose+ (expert) handles on the device: a mixed-expert batch against the split model's handles, bit for bit; against the
reference's keypoints; hipGraph replay across expert patterns; the existing entry points on an expert handle; errors."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.engine import VitPoseHip
from easy_vitpose_amd.moe import DATASETS, NUM_KEYPOINTS, split_vitpose_plus
from easy_vitpose_amd.synth import synthetic_crops, synthetic_moe_state_dict
from helpers import CONF_TOL, KP_TOL_PX

pytestmark = pytest.mark.gpu
P = 192


@functools.lru_cache(maxsize=2)
def moe_sd(variant: str, peaked: bool = True):
    return synthetic_moe_state_dict(model_shape(variant, 'coco'), P, seed=0, peaked=peaked)


@functools.lru_cache(maxsize=1)
def pool(n: int = 300):
    return np.concatenate([synthetic_crops(n // 2, 41, 'blobs'), synthetic_crops(n - n // 2, 42, 'noise')])


def expert_handle(variant, dtype='fp16', max_batch=64):
    return VitPoseHip(model_shape(variant, 'coco'), moe_sd(variant), dtype=dtype, max_batch=max_batch)


def split_handle(variant, dataset, dtype='fp16', max_batch=64):
    return VitPoseHip(model_shape(variant, dataset), split_vitpose_plus(moe_sd(variant), dataset), dtype=dtype, max_batch=max_batch)


def patterns(n):
    """(name, expert ids) of the expert patterns of a batch of n crops"""
    out = [('one', np.full(n, 3, np.int32)), ('interleaved', (np.arange(n) % 6).astype(np.int32))]
    if n >= 6:
        out.append(('blocks', np.repeat(np.arange(6), -(-n // 6))[:n][::-1].astype(np.int32).copy()))
        odd = np.zeros(n, np.int32)
        odd[n // 2] = 5
        out.append(('odd_wholebody', odd))
    if n % 24 == 0:   # segments of multiples of 4 crops: the 8-phase kernel keeps its 256-row tiles with experts
        out.append(('blocks4', np.repeat(np.arange(6), n // 6).astype(np.int32)))
    return out


def check_mixed(out, ks, ids, idx, ref):
    """out / ks = infer_mixed of crops pool[idx]; ref[e] = split handle e's keypoints of the whole pool"""
    for i, (e, j) in enumerate(zip(ids, idx)):
        K = NUM_KEYPOINTS[e]
        assert ks[i] == K
        assert np.array_equal(out[i, :K], ref[e][j]), f'crop {i} (expert {e}) differs from the split handle'
        assert not out[i, K:].any()


def _cases(sizes, n_pool):
    rng = np.random.default_rng(7)
    return [(n, name, ids, rng.choice(n_pool, size=n, replace=False)) for n in sizes for name, ids in patterns(n)]


@pytest.mark.parametrize('variant,sizes,max_batch', [
    ('s', (1, 3, 8, 13, 37, 64, 100), 64),
    ('b', (1, 3, 8, 13, 37, 64, 120, 256, 300), 256),
])
def test_mixed_batch_is_bit_identical_to_split_handles(one_launch_family, variant, sizes, max_batch):
    """fp16: crop i of a mixed batch == the same crop through the split model's handle (at whatever batch size: the one-launch family keeps the
    k order of every tile the rules pick, the crop-aligned fc2 fallback included) -- keypoints, bit for bit.  Sizes beyond max_batch are chunked;
    256 crops of ViTPose-B run mlp.fc2 on the 8-phase kernel (256-row tiles where the expert segments are multiples of 4 crops, else 192-row)."""
    crops = pool()
    cases = _cases(sizes, len(crops))
    eng = expert_handle(variant, 'fp16', max_batch)
    assert eng.experts == list(zip(DATASETS, NUM_KEYPOINTS)) and eng.part_features == P
    results = [eng.infer_mixed(crops[idx], ids) for _, _, ids, idx in cases]
    eng.close()
    ref = {}
    for e, ds in enumerate(DATASETS):
        h = split_handle(variant, ds, 'fp16', max_batch)
        ref[e] = h.infer(crops)
        h.close()
    for (n, name, ids, idx), (out, ks) in zip(cases, results):
        check_mixed(out, ks, ids, idx, ref)


@pytest.mark.parametrize('variant,sizes,max_batch', [('s', (1, 8, 13, 37, 100), 64), ('b', (1, 13, 64, 256), 256)])
def test_mixed_batch_bf16_against_split_handles(one_launch_family, variant, sizes, max_batch):
    """bf16: a plain handle is not bit-identical ACROSS batch sizes in bf16 (the cross-batch identity tests of the plain path are fp16), so the split
    handle runs the same n crops.  A single-expert batch is then the same computation: equal bits.  A mixed batch runs each expert's head on its segment
    (fewer crops than n), whose bf16 kernels round differently: within +-0.5 px and bf16's confidence bar (1.5e-2, tests/test_gpu_parity.py) of the
    split handle -- measured 0.02 px / 1.2e-3."""
    crops = pool()
    cases = _cases(sizes, len(crops))
    eng = expert_handle(variant, 'bf16', max_batch)
    results = [eng.infer_mixed(crops[idx], ids) for _, _, ids, idx in cases]
    eng.close()
    for e, ds in enumerate(DATASETS):
        h = split_handle(variant, ds, 'bf16', max_batch)
        for (n, name, ids, idx), (out, ks) in zip(cases, results):
            if not (ids == e).any():
                continue
            ref = h.infer(crops[idx])
            K = NUM_KEYPOINTS[e]
            got, want = out[ids == e, :K], ref[ids == e]
            assert not out[ids == e, K:].any() and (ks[ids == e] == K).all()
            if name == 'one':
                assert np.array_equal(got, want), (n, name, ds)
            else:
                assert np.abs(got[..., :2] - want[..., :2]).max() < KP_TOL_PX and np.abs(got[..., 2] - want[..., 2]).max() < 1.5e-2, (n, name, ds)
        h.close()


@pytest.mark.parametrize('variant,dtype', [('s', 'fp16'), ('b', 'bf16')])
def test_heatmaps_and_tokens_of_every_expert_equal_the_split_handle(one_launch_family, variant, dtype):
    crops = pool()[:5]
    eng = expert_handle(variant, dtype, 16)
    got = {}
    for e, ds in enumerate(DATASETS):
        eng.set_dataset(ds)
        assert eng.K == NUM_KEYPOINTS[e]
        got[e] = (eng.heatmaps(crops), eng.tokens(crops))
    eng.close()
    for e, ds in enumerate(DATASETS):
        h = split_handle(variant, ds, dtype, 16)
        hm, tok = h.heatmaps(crops), h.tokens(crops)
        h.close()
        assert got[e][0].shape == hm.shape and np.array_equal(got[e][0], hm), ds
        assert np.array_equal(got[e][1], tok), ds


def test_tokens_under_two_experts_differ_far_beyond_tolerance(one_launch_family):
    crops = pool()[:2]
    eng = expert_handle('s', 'fp16', 4)
    t0 = eng.tokens(crops)
    eng.set_dataset('wholebody')
    t5 = eng.tokens(crops)
    eng.close()
    D = t0.shape[-1]
    assert np.abs(t0 - t5).max() > 0.1                         # the expert channels [D - P, D) differ ...
    assert np.abs(t0[..., D - P:] - t5[..., D - P:]).mean() > 1e-2


@pytest.mark.parametrize('variant', ['s', 'b'])
@pytest.mark.parametrize('splitk', ['0', None])
def test_every_dataset_within_tolerance_of_the_reference(golden_dir, monkeypatch, variant, splitk):
    if splitk is not None:
        monkeypatch.setenv('VP_SPLITK', splitk)
    from cases import peaked_crops
    gold = {ds: np.load(os.path.join(golden_dir, f'moe_{variant}_{ds}.npz')) for ds in DATASETS}
    n = int(gold['coco']['n'])
    crops = peaked_crops(n)
    eng = expert_handle(variant, 'fp16', 64)
    out, ks = eng.infer_mixed(np.concatenate([crops] * 6), np.repeat(np.arange(6), n))   # one call, all six datasets
    single = []
    for ds in ('coco', 'wholebody'):   # and the single-expert path of small batches (split-K at its default)
        eng.set_dataset(ds)
        single.append((ds, eng.infer(crops[:1])))
    eng.close()
    for e, ds in enumerate(DATASETS):
        K = NUM_KEYPOINTS[e]
        kp, ref = out[e * n:(e + 1) * n, :K], gold[ds]['keypoints']
        dpx = np.abs(kp[..., :2] - ref[..., :2]).max()
        dcf = np.abs(kp[..., 2] - ref[..., 2]).max()
        print(f'[{variant}/{ds} splitk={splitk}] coordinate max err {dpx:.4f} px, confidence max err {dcf:.3e}')
        assert dpx < KP_TOL_PX and dcf < CONF_TOL, ds
    for ds, kp in single:
        ref = gold[ds]['keypoints'][:1]
        assert np.abs(kp[..., :2] - ref[..., :2]).max() < KP_TOL_PX and np.abs(kp[..., 2] - ref[..., 2]).max() < CONF_TOL


@pytest.mark.parametrize('n', [5, 8])
def test_graph_replay_never_crosses_expert_patterns(one_launch_family, n):
    crops = pool()[:n]
    A = np.zeros(n, np.int32)                                  # single expert (coco): captured and replayed
    C = np.full(n, 5, np.int32)                                # single expert (wholebody): same (n, buffers), another graph
    B = np.array([0, 5, 3, 5, 1, 2, 4, 0][:n], np.int32)       # mixed
    eng = expert_handle('s', 'fp16', 16)
    # B: eager, captured, replayed.  Its reverse holds the same counts in another permutation: B's graph with new tables, twice, then B's own again.
    # np.sort(B) holds them in expert order already: no gather, the crops staged where the forward reads them -- another source, another graph
    seq = [A, A, C, C, C, B, B, B, B[::-1].copy(), B[::-1].copy(), B, np.sort(B), np.sort(B), B, A, C, A]
    res = [eng.infer_mixed(crops, ids)[0] for ids in seq]
    eng.close()
    ref = {}
    for e, ds in enumerate(DATASETS):
        h = split_handle('s', ds, 'fp16', 16)
        ref[e] = h.infer(crops)
        h.close()
    for ids, out in zip(seq, res):
        check_mixed(out, [NUM_KEYPOINTS[e] for e in ids], ids, np.arange(n), ref)


@pytest.mark.parametrize('e', [0, 3, 5])
def test_existing_entry_points_on_an_expert_handle(one_launch_family, e):
    from easy_vitpose_amd.engine import PinnedArray
    crops = pool()[:6]
    frame = np.ascontiguousarray(np.tile(crops[0], (2, 3, 1)))
    params = np.array([[0, 0, 192, 256, 0, 0, 192, 256], [100, 40, 150, 200, 10, 20, 170, 240], [300, 200, 200, 300, 0, 0, 200, 300]], np.int32)
    pairs = [[1, 2], [3, 4]]
    ds = DATASETS[e]
    K = NUM_KEYPOINTS[e]

    def run(h):
        r = [h.infer(crops), h.infer_frame(frame, params), h.infer_flip(crops[:3], pairs)]
        pin = PinnedArray(crops.shape, np.uint8)
        pin.array[:] = crops
        out = np.zeros((len(crops), K, 3), np.float32)
        h.wait(h.submit(pin.array, out))
        r.append(out)
        pin.free()
        return r

    eng = expert_handle('s', 'fp16', 8)
    eng.set_dataset(ds)
    got = run(eng)
    eng.close()
    h = split_handle('s', ds, 'fp16', 8)
    want = run(h)
    h.close()
    for g, w in zip(got, want):
        assert g.shape[1] == K and np.array_equal(g, w)


def test_mixed_batch_is_run_to_run_identical_on_fresh_handles():
    crops = pool()[:29]
    ids = (np.arange(29) * 7 % 6).astype(np.int32)
    outs = []
    for _ in range(2):
        eng = expert_handle('s', 'bf16', 32)
        outs.append(eng.infer_mixed(crops, ids)[0])
        outs.append(eng.infer_mixed(crops, ids)[0])
        eng.close()
    assert all(np.array_equal(outs[0], o) for o in outs[1:])


def test_errors():
    crops = pool()[:2]
    eng = expert_handle('s', 'fp16', 4)
    lib, h = eng.lib, eng._h
    out = np.zeros((2, 133, 3), np.float32)
    bad = np.array([0, 6], np.int32)
    assert lib.vp_infer_experts(h, crops.ctypes.data, capi.VP_INPUT_U8_NHWC, 2, bad.ctypes.data, None, out.ctypes.data) == capi.VP_ERR_INVALID
    assert lib.vp_set_expert(h, 6) == capi.VP_ERR_INVALID and lib.vp_set_expert(h, -1) == capi.VP_ERR_INVALID
    with pytest.raises(ValueError):
        eng.set_dataset('coco_25')
    eng.close()
    plain = split_handle('s', 'coco', 'fp16', 4)
    ok = np.zeros(2, np.int32)
    assert plain.lib.vp_set_expert(plain._h, 0) == capi.VP_ERR_STATE
    assert plain.lib.vp_infer_experts(plain._h, crops.ctypes.data, capi.VP_INPUT_U8_NHWC, 2, ok.ctypes.data, None, out.ctypes.data) == capi.VP_ERR_STATE
    plain.close()
    with pytest.raises(capi.VpError) as ei:
        VitPoseHip(model_shape('b', 'coco'), moe_sd('b'), dtype='fp8', max_batch=4)
    assert ei.value.code == capi.VP_ERR_INVALID


def test_vit_inference_loads_an_unsplit_file(tmp_path, one_launch_family):
    """VitInference('vitpose+_s.pth', yolo, dataset='ap10k'): the unsplit file, the ap10k expert and head, det_class as for a split ap10k file."""
    import torch
    from easy_vitpose_amd.inference import VitInference
    path = tmp_path / 'vitpose+_s.pth'
    torch.save({'state_dict': {k: torch.from_numpy(np.array(v)) for k, v in moe_sd('s').items()}}, str(path))
    model = VitInference(str(path), lambda img: np.zeros((0, 5)), dataset='ap10k', max_batch=4)
    assert model.yolo_classes == [15, 16, 17, 18, 19, 20, 21, 22, 23] and model._vit_pose.K == 17 and model._vit_pose.dataset == 'ap10k'
    crops = pool()[:3]
    got = model._vit_pose.infer(crops)
    model._vit_pose.close()
    h = split_handle('s', 'ap10k', 'fp16', 4)
    want = h.infer(crops)
    h.close()
    assert np.array_equal(got, want)
