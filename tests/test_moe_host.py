"""ViTPose+ checkpoints on the host (no GPU): the split restated from model_split.py, detection, refusals, the C ABI surface
and the tile rule of a mixed-expert mlp.fc2."""
from __future__ import annotations

import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import ModelShape, model_shape
from easy_vitpose_amd.moe import DATASETS, NUM_KEYPOINTS, is_vitpose_plus, moe_info, split_vitpose_plus
from easy_vitpose_amd.synth import synthetic_moe_state_dict, synthetic_state_dict


def _digest(a) -> str:
    a = np.asarray(a)
    if a.dtype != np.int64:
        a = a.astype(np.float32)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope='module')
def tiny(golden_dir):
    z = np.load(os.path.join(golden_dir, 'moe_split_tiny.npz'))
    shp = ModelShape('tiny', int(z['D']), int(z['depth']), int(z['heads']), 17)
    return z, synthetic_moe_state_dict(shp, int(z['P']), n_experts=6, seed=int(z['seed']))


def test_tiny_input_is_the_one_the_reference_split(tiny):
    z, sd = tiny
    keys = sorted(sd)
    assert keys == list(z['input_keys'])
    assert [_digest(sd[k]) for k in keys] == list(z['input_digest'])


@pytest.mark.parametrize('dataset', DATASETS)
def test_split_equals_reference_model_split_bit_for_bit(tiny, dataset):
    z, sd = tiny
    out = split_vitpose_plus(sd, dataset)
    keys = sorted(out)
    assert keys == list(z[f'{dataset}/keys'])
    assert [','.join(str(d) for d in np.shape(out[k])) for k in keys] == list(z[f'{dataset}/shapes'])
    assert [_digest(out[k]) for k in keys] == list(z[f'{dataset}/digest'])


def test_split_accepts_a_wrapped_checkpoint_and_torch_tensors(tiny):
    import torch
    _, sd = tiny
    wrapped = {'state_dict': {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}}
    a = split_vitpose_plus(wrapped, 'wholebody')
    b = split_vitpose_plus(sd, 'wholebody')
    assert sorted(a) == sorted(b)
    assert all(np.array_equal(a[k].numpy(), b[k]) for k in a)


def test_detection_reads_e_p_and_k_per_expert():
    shp = model_shape('s', 'coco')
    sd = synthetic_moe_state_dict(shp, 192, seed=1)
    assert is_vitpose_plus(sd) and not is_vitpose_plus(synthetic_state_dict(shp, 1))
    info = moe_info(sd)
    assert (info.n_experts, info.part_features) == (6, 192)
    assert info.datasets == DATASETS and info.num_keypoints == (17, 14, 16, 17, 17, 133)
    four = {k: v for k, v in sd.items() if not any(f'experts.{e}.' in k for e in (4, 5))
            and not k.startswith(('associate_keypoint_heads.3.', 'associate_keypoint_heads.4.'))}
    assert moe_info(four)[:2] == (4, 192)
    sd128 = synthetic_moe_state_dict(shp, 128, n_experts=2, seed=1)
    assert moe_info(sd128)[:2] == (2, 128)


def test_synthetic_experts_are_distinct_and_heads_oversized():
    sd = synthetic_moe_state_dict(model_shape('s', 'coco'), 192, seed=2)
    w = [sd[f'backbone.blocks.0.mlp.experts.{e}.weight'] for e in range(6)]
    assert all(not np.array_equal(w[a], w[b]) for a in range(6) for b in range(a + 1, 6))
    rows = [sd[f'associate_keypoint_heads.{i}.final_layer.weight'].shape[0] for i in range(5)]
    assert any(r > k for r, k in zip(rows, NUM_KEYPOINTS[1:]))
    f0 = [sd[f'associate_keypoint_heads.{i}.final_layer.weight'][:14] for i in range(5)]
    assert all(not np.array_equal(f0[a], f0[b]) for a in range(5) for b in range(a + 1, 5))


@pytest.mark.parametrize('case', ['p_not_64', 'p_too_big', 'missing_expert', 'missing_head'])
def test_refusals(case):
    shp = model_shape('s', 'coco')
    if case == 'p_not_64':
        sd = synthetic_moe_state_dict(shp, 96, n_experts=2, seed=3)
        exc = RuntimeError
    elif case == 'p_too_big':
        sd = synthetic_moe_state_dict(shp, 192, n_experts=2, seed=3)
        for l in range(shp.depth):   # P = D: nothing shared
            sd[f'backbone.blocks.{l}.mlp.experts.0.weight'] = np.zeros((384, 1536), np.float32)
        exc = RuntimeError
    elif case == 'missing_expert':
        sd = synthetic_moe_state_dict(shp, 192, n_experts=3, seed=3)
        del sd['backbone.blocks.7.mlp.experts.2.weight']
        exc = KeyError
    else:
        sd = synthetic_moe_state_dict(shp, 192, n_experts=3, seed=3)
        for k in [k for k in sd if k.startswith('associate_keypoint_heads.1.')]:
            del sd[k]
        exc = KeyError
    with pytest.raises(exc):
        moe_info(sd)
    with pytest.raises(exc):
        split_vitpose_plus(sd, 'coco')


def test_split_refuses_an_unknown_dataset(tiny):
    with pytest.raises(ValueError):
        split_vitpose_plus(tiny[1], 'coco_25')


def test_expert_symbols_are_exported_and_bound():
    lib = capi.load_library()
    for name in ('vp_expert_info', 'vp_set_expert', 'vp_infer_experts', 'vp_dbg_expert_tile'):
        assert name in capi.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.vp_set_expert(None, 0) == capi.VP_ERR_INVALID
    assert lib.vp_expert_info(None, None, None, None) == capi.VP_ERR_INVALID
    assert lib.vp_infer_experts(None, None, 0, 0, None, None, None) == capi.VP_ERR_INVALID


def _expert_tile(variant, n_crops, bounds, N=768, gemm8_ok=1):
    lib = capi.load_library()
    b = (C.c_int32 * max(len(bounds), 1))(*bounds)
    return lib.vp_dbg_expert_tile(variant, n_crops * 192, N, gemm8_ok, b, len(bounds))


def test_expert_tile_rule_keeps_crop_aligned_tiles():
    # 32 / 64 / 96 / 192-row tiles divide a crop: kept whatever the expert pattern
    for v in (31, 9, 12, 30, 41, 8, 11, 20, 18):
        assert _expert_tile(v, 13, [1, 5, 6, 12]) == v
    # 128-row tiles: kept where every change is at an even crop, 256-row tiles where it is a multiple of 4
    assert _expert_tile(1, 16, [2, 8]) == 1 and _expert_tile(15, 16, [4]) == 15
    assert _expert_tile(1, 16, [3]) == 11
    assert _expert_tile(16, 256, [4, 40, 128]) == 16 and _expert_tile(17, 256, [8]) == 17
    assert _expert_tile(16, 256, [6]) == 18          # the 8-phase kernel's 192-row tile
    assert _expert_tile(17, 256, [1, 2, 3]) == 18
    assert _expert_tile(3, 100, [2]) == 11           # 2-phase 256 x 256 -> the residual default 192 x 128
    assert _expert_tile(16, 256, [6], gemm8_ok=0) == 11
    assert _expert_tile(16, 40, [6]) == 11           # too few 192 x 256 tiles for the 8-phase kernel
    assert _expert_tile(16, 256, []) == 16           # one expert: the rule's tile


def test_expert_tile_rule_never_spans_a_change():
    rng = np.random.default_rng(0)
    bm = {1: 128, 3: 256, 8: 192, 9: 64, 11: 192, 12: 64, 15: 128, 16: 256, 17: 256, 18: 192, 20: 192, 30: 64, 31: 32, 41: 96}
    for _ in range(300):
        n = int(rng.integers(2, 300))
        bounds = sorted(set(int(b) for b in rng.integers(1, n, size=int(rng.integers(1, 6)))))
        v = _expert_tile(int(rng.choice(list(bm))), n, bounds)
        assert all((b * 192) % bm[v] == 0 for b in bounds)


@pytest.mark.parametrize('name', ['vitpose+_b.pth', 'vitpose-b-coco.pth'])
def test_vit_inference_needs_a_dataset_for_an_unsplit_file(tmp_path, tiny, name):
    """The file name cannot tell which of the six heads is wanted: dataset=None is an error that lists them (before any device work)."""
    import torch
    from easy_vitpose_amd.inference import VitInference
    path = tmp_path / name
    torch.save({'state_dict': {k: torch.from_numpy(np.array(v)) for k, v in tiny[1].items()}}, str(path))
    with pytest.raises(ValueError) as ei:
        VitInference(str(path), lambda img: np.zeros((0, 5)))
    assert all(ds in str(ei.value) for ds in DATASETS)
    with pytest.raises(ValueError):
        VitInference(str(path), lambda img: np.zeros((0, 5)), dataset='coco_25')
