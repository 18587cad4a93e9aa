#!/usr/bin/env python3
"""Generate tests/golden/affine.npz by running THE REFERENCE ITSELF (make_golden.py's stub recipe, imported, not edited): the training-side crop protocol.

    python tests/golden/make_golden_affine.py

Runs only where the reference checkout exists.  Nothing of the reference is copied: the file holds boxes, the reference's centres / scales / warp matrices /
keypoints and the numpy version it ran under (the float32 widths of `_xywh2cs` are numpy 2's promotion rules).  Frames, heatmaps and weights are regenerated
from seeds (tests/affine_cases.py, tests/golden/cases.py, easy_vitpose_amd/synth.py).

  center, scale200 [40, 2]   `TopDownCocoDataset._xywh2cs(x, y, w, h)` per box of affine_cases.geometry_boxes(), and scale * 200
  warp [40, 2, 3]            get_warp_matrix(0, center * 2, [191, 255], scale * 200)
  decode_k17 / decode_k133   keypoints_from_heatmaps(hm, center, scale * 200, unbiased=True, use_udp=True), one call per crop (N = 1), on
                             cases.peaked_heatmaps(40, K, seed) -> [40, K, 3] (y, x, conf)
  e2e_*                      the reference ViTPose (S / coco, the peaked synthetic checkpoint) on crops made by tests/affine_model.py (the independent scalar
                             model, not the product) from affine_cases.frames() -- frame A as RGB, frame B as the NV12 surface affine_cases.frame_b_nv12() -- decoded by keypoints_from_heatmaps with each box's centre and scale
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import make_golden as MG


def main():
    import affine_cases as AC
    import affine_model as AM
    from cases import peaked_heatmaps
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.synth import synthetic_state_dict

    VitInference, ViTPose, dyn_model_import = MG.import_reference()
    for name in ['json_tricks', 'pycocotools', 'pycocotools.coco', 'torchvision.transforms.functional', 'tqdm', 'PIL', 'PIL.Image', 'munkres']:
        if name not in sys.modules:   # what datasets/COCO.py imports for its file and image handling, none of it reached by _xywh2cs (make_golden.py's recipe)
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = MG._Stub(name)
    from easy_ViTPose.datasets.COCO import COCODataset
    from easy_ViTPose.vit_utils.post_processing.post_transforms import get_warp_matrix
    from easy_ViTPose.vit_utils.top_down_eval import keypoints_from_heatmaps

    ds = types.SimpleNamespace(aspect_ratio=192 * 1.0 / 256, pixel_std=200)   # what COCODataset.__init__ sets from image_size (192, 256)

    def xywh2cs(box):
        x1, y1, x2, y2 = (float(v) for v in box)
        return COCODataset._xywh2cs(ds, x1, y1, x2 - x1, y2 - y1)

    def cs_of(boxes):
        c, s = zip(*(xywh2cs(b) for b in boxes))
        c, s = np.stack(c), np.stack(s)
        assert c.dtype == np.float32 and s.dtype == np.float32, (c.dtype, s.dtype)
        s200 = s * 200
        assert s200.dtype == np.float32
        return c, s200

    boxes = AC.geometry_boxes()
    center, scale200 = cs_of(boxes)
    warp = np.stack([get_warp_matrix(0, c * 2.0, np.array([191, 255]), s) for c, s in zip(center, scale200)])
    out = dict(numpy_version=np.__version__, boxes=boxes, center=center, scale200=scale200, warp=warp.astype(np.float32))
    for K, seed in AC.DECODE_SEEDS.items():
        hm = peaked_heatmaps(len(boxes), K, seed)
        rows = []
        for i in range(len(boxes)):
            pts, prob = keypoints_from_heatmaps(heatmaps=hm[i:i + 1].copy(), center=center[i:i + 1], scale=scale200[i:i + 1], unbiased=True, use_udp=True)
            rows.append(np.concatenate([pts[:, :, ::-1], prob], axis=2))
        out[f'decode_k{K}'] = np.concatenate(rows).astype(np.float32)
        mine = AM.decode(hm, np.concatenate([center, scale200], 1))
        print(f'decode K = {K}: fp64 model vs reference max|d| = {np.abs(mine[..., :2] - out[f"decode_k{K}"][..., :2]).max():.3e} px, confidences equal: '
              f'{np.array_equal(mine[..., 2], out[f"decode_k{K}"][..., 2])}')

    # end to end: the reference model on the independent model's crops
    eb, ef = AC.e2e_boxes()
    ec, es = cs_of(eb)
    fa, fb = AC.frames()
    rows = [AM.frame_to_rgb_rows('rgb', (fa,)), AM.frame_to_rgb_rows('nv12', AC.frame_b_nv12(), 'bt601')]   # frame A is RGB, frame B an NV12 surface
    shp = model_shape('s', 'coco')
    V = MG.build_ref(VitInference, ViTPose, dyn_model_import, 'coco', 's', synthetic_state_dict(shp, seed=0, peaked=True))
    kps = []
    with torch.no_grad():
        for i in range(len(eb)):
            crop = AM.crop(rows[ef[i]], np.concatenate([ec[i], es[i]]))
            x, _, _ = V.pre_img(crop)                                   # 256 x 192 already: the resize is the identity
            hm = V._vit_pose(torch.from_numpy(x)).numpy()
            pts, prob = keypoints_from_heatmaps(heatmaps=hm, center=ec[i:i + 1], scale=es[i:i + 1], unbiased=True, use_udp=True)
            kps.append(np.concatenate([pts[:, :, ::-1], prob], axis=2))
    out.update(e2e_boxes=eb, e2e_frame=ef, e2e_center=ec, e2e_scale200=es, e2e_keypoints=np.concatenate(kps).astype(np.float32))
    print(f'e2e: {len(eb)} crops, confidences {out["e2e_keypoints"][..., 2].min():.3f} .. {out["e2e_keypoints"][..., 2].max():.3f}')
    np.savez_compressed(os.path.join(HERE, 'affine.npz'), **out)
    print('wrote affine.npz under numpy', np.__version__)


if __name__ == '__main__':
    main()
