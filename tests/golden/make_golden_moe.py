#!/usr/bin/env python3
"""Generate the ViTPose+ golden fixtures by running THE REFERENCE ITSELF in this container.

    python tests/golden/make_golden_moe.py            # writes tests/golden/moe_*.npz
    python tests/golden/make_golden_moe.py --only=split

Runs only where ``/root/reference`` exists (the build container); imported read-only like ``make_golden.py``, whose stubs and
model builder it reuses.  Nothing from the reference is copied: the fixtures hold seeds, shapes, key lists and the
reference's OUTPUTS.

* ``moe_split_tiny.npz`` (section ``split``): a tiny ViTPose+ state dict (D = 128, depth 2, 6 experts, P = 64; the aic / mpii heads'
  final layers carry 17 rows) from ``synthetic_moe_state_dict``, saved as a ``.pth`` and cut by the reference's own
  ``model_split.py`` in a subprocess.  Stored per dataset: the key list, every shape and a SHA-256 of every tensor's float32 bytes
  (the six split dicts themselves are ~8 MB each), plus the digest of the input dict.  Pins ``moe.split_vitpose_plus`` bit for bit.
* ``moe_<variant>_<dataset>.npz`` (section ``model``): ViTPose-B and -S with P = 192, peaked read-outs: the reference model's
  keypoints (``_inference_torch``) and the first crop's heatmap maxima on the split dict of every dataset, for 8 seeded crops
  (``cases.peaked_crops``).  The split dicts come from ``moe.split_vitpose_plus`` -- the function the tiny fixture pins to
  ``model_split.py`` (running the script on a ViTPose-B file would write six 350 MB checkpoints).  The oracle's deviation on the same
  inputs is printed, as ``make_golden.py`` does.
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

from make_golden import REF, build_ref, import_reference

ONLY = next((a.split('=', 1)[1].split(',') for a in sys.argv[1:] if a.startswith('--only=')), None)
TINY = dict(D=128, depth=2, heads=2, P=64, seed=5)
MODEL_PLAN = [('s', 192, 8), ('b', 192, 8)]   # (variant, P, crops)
MODEL_SEED = 0


def want(section: str) -> bool:
    return ONLY is None or section in ONLY


def digest(a) -> str:
    a = a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)
    if a.dtype != np.int64:
        a = a.astype(np.float32)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def tiny_state_dict():
    from easy_vitpose_amd.configs import ModelShape
    from easy_vitpose_amd.synth import synthetic_moe_state_dict
    shp = ModelShape('tiny', TINY['D'], TINY['depth'], TINY['heads'], 17)
    return synthetic_moe_state_dict(shp, TINY['P'], n_experts=6, seed=TINY['seed'])


def make_split():
    from easy_vitpose_amd.moe import DATASETS
    sd = tiny_state_dict()
    out = {'D': TINY['D'], 'depth': TINY['depth'], 'heads': TINY['heads'], 'P': TINY['P'], 'seed': TINY['seed'],
           'input_keys': np.array(sorted(sd)), 'input_digest': np.array([digest(sd[k]) for k in sorted(sd)])}
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'vitpose_plus_tiny.pth')
        torch.save({'state_dict': {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}}, src)
        subprocess.run([sys.executable, os.path.join(REF, 'model_split.py'), '--source', src, '--prefix', 'tiny_', '--target', td],
                       check=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
        for ds in DATASETS:
            s = torch.load(os.path.join(td, f'tiny_{ds}.pth'), map_location='cpu', weights_only=True)['state_dict']
            keys = sorted(s)
            out[f'{ds}/keys'] = np.array(keys)
            out[f'{ds}/shapes'] = np.array([','.join(str(d) for d in s[k].shape) for k in keys])
            out[f'{ds}/digest'] = np.array([digest(s[k]) for k in keys])
            print(f'split {ds}: {len(keys)} tensors, keypoint_head.final_layer.weight {tuple(s["keypoint_head.final_layer.weight"].shape)}')
    np.savez_compressed(os.path.join(HERE, 'moe_split_tiny.npz'), **out)


def make_model():
    from cases import peaked_crops
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.moe import DATASETS, split_vitpose_plus
    from easy_vitpose_amd.synth import synthetic_moe_state_dict
    from oracle import vitpose_cpu as O
    VitInference, ViTPose, dyn_model_import = import_reference()
    for variant, P, n in MODEL_PLAN:
        shp = model_shape(variant, 'coco')
        sd = synthetic_moe_state_dict(shp, P, seed=MODEL_SEED, peaked=True)
        crops = peaked_crops(n)
        for ds in DATASETS:
            split = split_vitpose_plus(sd, ds)
            # the reference's config modules exist per dataset; 'coco' serves every one (out_channels is set from the dict)
            V = build_ref(VitInference, ViTPose, dyn_model_import, 'coco', variant, split)
            with torch.no_grad():
                kps = np.concatenate([V._inference_torch(crops[i]) for i in range(n)], 0).astype(np.float32)
                hm0 = V._vit_pose(torch.from_numpy(V.pre_img(crops[0])[0])).numpy()
            sdt = O.to_torch_state_dict(split)
            mine = np.concatenate([O.inference_torch(sdt, shp.depth, shp.num_heads, crops[i]) for i in range(n)], 0)
            print(f'moe {variant}/{ds} (P = {P}): {n} crops x {kps.shape[1]} joints, confidences {kps[..., 2].min():.3f} .. {kps[..., 2].max():.3f}, '
                  f'oracle-vs-reference keypoints max|d| = {np.abs(mine - kps).max():.3e}')
            np.savez_compressed(os.path.join(HERE, f'moe_{variant}_{ds}.npz'), variant=variant, dataset=ds, P=P, seed=MODEL_SEED, n=n,
                                keypoints=kps, heatmap_max0=hm0[0].reshape(hm0.shape[1], -1).max(-1).astype(np.float32))


def main():
    if not os.path.isdir(REF):
        sys.exit(f'{REF} not found: the ViTPose+ goldens are generated where the reference is')
    if want('split'):
        make_split()
    if want('model'):
        make_model()


if __name__ == '__main__':
    main()
