"""Shape contract of the ViTPose hot path.

Mirrors (as a static table, not as importable python-dict configs) what the
reference spreads over ``easy_ViTPose/configs/ViTPose_common.py:65-195``
(``model_small/base/large/huge``: embed_dim / depth / num_heads),
``ViTPose_common.py:29-40`` (``data_cfg``: image 192x256, heatmap 48x64) and the
per-dataset ``out_channels`` (``configs/ViTPose_coco.py:4-18``,
``ViTPose_coco_25.py:4-20``, ``ViTPose_wholebody.py:4-20``, ``ViTPose_ap10k.py:4-22``,
``ViTPose_mpii.py``, ``ViTPose_aic.py``, ``ViTPose_apt36k.py``).

Name lookup follows ``vit_utils/util.py:20-41`` (``MODEL_ABBR_MAP``,
``infer_dataset_by_path``, ``dyn_model_import``).
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass

import numpy as np

# input crop (W, H) and heatmap (W, H): ViTPose_common.py:29-31
IMAGE_SIZE = (192, 256)
HEATMAP_SIZE = (48, 64)
IMG_H, IMG_W = 256, 192
HM_H, HM_W = 64, 48
PATCH = 16
TOKENS = 192  # 16 x 12 patches
GRID_H, GRID_W = 16, 12
DECONV_CH = 256  # num_deconv_filters=(256, 256): the classic decoder only (the simple decoder has no deconv layers)
HEADS = ('classic', 'simple')  # two deconvs + 1x1 conv | ReLU -> bilinear x 4 -> 3x3 conv (the model zoo's `-simple` files)

MODEL_ABBR_MAP = {'s': 'small', 'b': 'base', 'l': 'large', 'h': 'huge'}

# (embed_dim, depth, num_heads)   ViTPose_common.py:65-195
VARIANTS = {
    's': (384, 12, 12),
    'b': (768, 12, 12),
    'l': (1024, 24, 16),
    'h': (1280, 32, 16),
}

# dataset -> number of keypoints (head out_channels)
DATASET_KEYPOINTS = {
    'coco': 17,
    'coco_25': 25,
    'wholebody': 133,
    'mpii': 16,
    'aic': 14,
    'ap10k': 17,
    'apt36k': 17,
}


@dataclass(frozen=True)
class ModelShape:
    """Static shape of one (variant, dataset) model."""
    variant: str
    embed_dim: int
    depth: int
    num_heads: int
    num_keypoints: int
    head: str = 'classic'

    @property
    def head_dim(self) -> int:
        return self.embed_dim // self.num_heads

    @property
    def mlp_dim(self) -> int:
        return 4 * self.embed_dim

    def gflop_per_person(self) -> float:
        """Algorithmic FLOPs (2*M*N*K of every matmul/conv incl. attention core),
        the formula of SURVEY.md section 8(d)."""
        D, L, K = self.embed_dim, self.depth, self.num_keypoints
        encoder = L * (4608 * D * D + 147456 * D) + 294912 * D
        if self.head == 'simple':   # the commuted form: the 9-tap GEMM at 16 x 12 (2 * 192 * 9 K * D) + the 36-term stencil at 64 x 48
            return (encoder + 3456 * K * D + 221184 * K) / 1e9
        return (encoder + 1572864 * D + 1610612736 + 1572864 * K) / 1e9


def model_shape(variant: str, dataset: str | None = None, num_keypoints: int | None = None, head: str = 'classic') -> ModelShape:
    assert variant in VARIANTS, f'The model name {variant} is not valid'
    if num_keypoints is None:
        assert dataset in DATASET_KEYPOINTS, 'The specified dataset is not valid'
        num_keypoints = DATASET_KEYPOINTS[dataset]
    D, L, h = VARIANTS[variant]
    assert head in HEADS, f'unknown decoder {head!r}'
    return ModelShape(variant, D, L, h, int(num_keypoints), head)


def infer_dataset_by_path(model_path: str) -> str:
    """Same filename convention as ``vit_utils/util.py:28-34``:
    ``vitpose-b-coco_25.pth`` -> ``coco_25``. Raises ValueError like the reference."""
    model = os.path.basename(model_path)
    m = re.search(r'-([a-zA-Z0-9_]+)\.[pth, onnx, engine]', model)
    if not m:
        raise ValueError('Could not infer the dataset from ckpt name, specify it')
    return m.group(1)


def infer_variant_from_state_dict(sd) -> str:
    """The reference needs ``model_name`` for .pth files; the shapes also tell."""
    D = int(sd['backbone.pos_embed'].shape[-1])
    for v, (d, _, _) in VARIANTS.items():
        if d == D:
            return v
    raise ValueError(f'unknown embed_dim {D}')


def infer_head_from_state_dict(sd) -> str:
    """``'classic'`` (two deconvs + a 1x1 conv) or ``'simple'`` (ReLU -> bilinear x 4 -> 3x3 conv, the ``vitpose-*-simple`` files), by the
    rule the loader applies: simple when no ``keypoint_head.deconv_layers.*`` is present and ``final_layer.weight`` is ``[K, D, 3, 3]``.
    Raises ValueError for a dict that is neither (the loader refuses it too).

    Note: ``infer_dataset_by_path('vitpose-b-simple.pth')`` returns ``'simple'`` exactly as the reference's function does, so such a file
    needs ``dataset='coco'`` given or a name that ends in its dataset (``vitpose-b-simple-coco.pth``)."""
    w = sd['keypoint_head.final_layer.weight']
    shp = tuple(int(v) for v in w.shape)
    D = int(sd['backbone.pos_embed'].shape[-1])
    has_deconv = any(k.startswith('keypoint_head.deconv_layers.') for k in sd)
    three = len(shp) == 4 and shp[1:] == (D, 3, 3)
    if three and not has_deconv:
        return 'simple'
    if three:
        raise ValueError('keypoint_head.final_layer.weight is a 3x3 conv (simple decoder) but keypoint_head.deconv_layers.* are present')
    if int(np.prod(shp)) != shp[0] * DECONV_CH:
        raise ValueError(f'keypoint_head.final_layer.weight {shp}: neither [K, {DECONV_CH}, 1, 1] (classic decoder) nor [K, {D}, 3, 3] (simple decoder)')
    return 'classic'


# mirror joint pairs of the 17-joint COCO layout (left / right eye, ear, shoulder, elbow, wrist, hip, knee, ankle): the one flip-pair table the
# reference ships (datasets/COCO.py); every other dataset's pairs come from the user
COCO17_FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]


def resolve_flip_pairs(flip_test, dataset, num_keypoints):
    """`flip_test` of VitInference / the CLI -> the pair list to hand the handle, or None for "mode off".  True stands for the COCO-17
    table and is accepted for that layout only; any other dataset needs its pairs spelled out."""
    if flip_test is None or flip_test is False:
        return None
    if flip_test is True:
        if dataset != 'coco' or num_keypoints != 17:
            raise ValueError(f'flip_test=True stands for the mirror pairs of the 17-joint COCO layout; dataset {dataset!r} with {num_keypoints} '
                             'joints needs its pairs given explicitly: flip_test=[[left, right], ...]')
        return [list(p) for p in COCO17_FLIP_PAIRS]
    pairs = [[int(a), int(b)] for a, b in flip_test]
    for a, b in pairs:
        if not (0 <= a < num_keypoints and 0 <= b < num_keypoints):
            raise ValueError(f'flip pair ({a}, {b}) outside the {num_keypoints} joints of dataset {dataset!r}')
    return pairs
