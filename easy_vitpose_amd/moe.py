"""ViTPose+ checkpoints: one backbone trained on six datasets ("mixture of experts").

The last ``P`` output features of every block's ``mlp.fc2`` come from a per-dataset expert
(``backbone.blocks.{l}.mlp.experts.{e}.{weight,bias}``) and every dataset has its own keypoint
head.  The reference handles such a file only offline: ``model_split.py`` cuts it into six
single-dataset state dicts.  :func:`split_vitpose_plus` restates that script for one dataset;
the C library loads the unsplit dict directly (``vp_load_weights``, ``vp_set_expert``,
``vp_infer_experts``) and gives bit for bit the split model's results.

Expert order follows ``model_split.py``: expert 0 = coco with ``keypoint_head``; expert ``i + 1``
= ``DATASETS[i + 1]`` with ``associate_keypoint_heads.{i}``, its final layer cut to the first
``K`` rows.  ``P`` is read from the checkpoint, never from a table.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

DATASETS = ('coco', 'aic', 'mpii', 'ap10k', 'apt36k', 'wholebody')
NUM_KEYPOINTS = (17, 14, 16, 17, 17, 133)

# the head tensors model_split.py moves from an associate head to keypoint_head (model_split.py weight_names)
_HEAD_TENSORS = ('deconv_layers.0.weight', 'deconv_layers.1.weight', 'deconv_layers.1.bias', 'deconv_layers.1.running_mean',
                 'deconv_layers.1.running_var', 'deconv_layers.1.num_batches_tracked', 'deconv_layers.3.weight',
                 'deconv_layers.4.weight', 'deconv_layers.4.bias', 'deconv_layers.4.running_mean', 'deconv_layers.4.running_var',
                 'deconv_layers.4.num_batches_tracked', 'final_layer.weight', 'final_layer.bias')


class MoeInfo(NamedTuple):
    n_experts: int           # E: experts present in block 0
    part_features: int       # P: output features of every expert (the last P of D)
    datasets: tuple          # dataset of expert e
    num_keypoints: tuple     # K of expert e


def _unwrap(sd):
    return sd['state_dict'] if 'state_dict' in sd else sd


def head_prefix(e: int) -> str:
    return 'keypoint_head' if e == 0 else f'associate_keypoint_heads.{e - 1}'


def is_vitpose_plus(sd) -> bool:
    return 'backbone.blocks.0.mlp.experts.0.weight' in _unwrap(sd)


def _shape(v):
    return tuple(v.shape)


def moe_info(sd) -> MoeInfo:
    """E, P and K per expert of a ViTPose+ state dict; the same refusals as the C loader: KeyError for a missing expert or
    head (load_state_dict's "Missing key(s)"), RuntimeError for a part size the kernels do not take ("size mismatch")."""
    sd = _unwrap(sd)
    if not is_vitpose_plus(sd):
        raise ValueError('not a ViTPose+ state dict (no backbone.blocks.0.mlp.experts.0.weight)')
    E = 0
    while f'backbone.blocks.0.mlp.experts.{E}.weight' in sd:
        E += 1
    if E > len(DATASETS):
        raise RuntimeError(f'ViTPose+ state dict with {E} experts: at most {len(DATASETS)} ({", ".join(DATASETS)})')
    D = int(_shape(sd['backbone.pos_embed'])[-1])
    P = int(_shape(sd['backbone.blocks.0.mlp.experts.0.weight'])[0])
    if P % 64 != 0 or P >= D:
        raise RuntimeError(f'ViTPose+ part_features {P} unsupported: must be a multiple of 64 and below embed_dim {D}')
    depth = 0
    while f'backbone.blocks.{depth}.mlp.fc2.weight' in sd:
        depth += 1
    for l in range(depth):
        for e in range(E):
            for t in ('weight', 'bias'):
                k = f'backbone.blocks.{l}.mlp.experts.{e}.{t}'
                if k not in sd:
                    raise KeyError(f'ViTPose+ state dict: expert {e} missing in block {l} (missing key {k})')
        if _shape(sd[f'backbone.blocks.{l}.mlp.fc2.weight'])[0] + P != D:
            raise RuntimeError(f'size mismatch for backbone.blocks.{l}.mlp.fc2.weight: {D - P} shared rows expected with P = {P}')
    for e in range(E):
        k = f'{head_prefix(e)}.final_layer.weight'
        if k not in sd:
            raise KeyError(f'ViTPose+ state dict: expert {e} ({DATASETS[e]}) has no head (missing key {k})')
    return MoeInfo(E, P, DATASETS[:E], NUM_KEYPOINTS[:E])


def _cat(a, b):
    if hasattr(a, 'detach'):
        import torch
        return torch.cat([a, b], dim=0)
    return np.concatenate([np.asarray(a), np.asarray(b)], axis=0)


def split_vitpose_plus(sd, dataset: str) -> dict:
    """The single-dataset state dict ``model_split.py`` writes for `dataset` (numpy or torch values, kept as given):
    every ``mlp.fc2`` = cat([shared, experts.{e}]) along the output features; for e > 0 the head tensors come from
    ``associate_keypoint_heads.{e - 1}`` with the final layer cut to K rows; every associate head and every expert tensor is dropped."""
    if dataset not in DATASETS:
        raise ValueError(f'unknown ViTPose+ dataset {dataset!r}: one of {", ".join(DATASETS)}')
    src = _unwrap(sd)
    info = moe_info(src)
    e = DATASETS.index(dataset)
    if e >= info.n_experts:
        raise KeyError(f'ViTPose+ state dict has {info.n_experts} experts: no expert {e} ({dataset})')
    out = dict(src)
    for key in src:
        if 'mlp.fc2' in key:
            out[key] = _cat(src[key], src[key.replace('fc2.', f'experts.{e}.')])
    if e > 0:
        for t in _HEAD_TENSORS:
            a = f'associate_keypoint_heads.{e - 1}.{t}'
            if a in src:
                out[f'keypoint_head.{t}'] = src[a]
        K = NUM_KEYPOINTS[e]
        for t in ('final_layer.weight', 'final_layer.bias'):
            out[f'keypoint_head.{t}'] = out[f'keypoint_head.{t}'][:K]
    for key in list(out):
        if key.startswith('associate_keypoint_heads.') or 'expert' in key:
            del out[key]
    return out
