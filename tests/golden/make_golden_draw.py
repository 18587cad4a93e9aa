"""Writes tests/golden/draw_tables.npz: the reference's drawing tables, as data.

    python tests/golden/make_golden_draw.py /path/to/easy_ViTPose

* every dataset's ``skeleton`` of ``vit_utils/visualization.py::joints_dict()`` as an int array (key = the dataset's name);
* ``limb_colors`` / ``point_colors``: the two palettes ``VitInference.draw`` asks for ('jet' sampled at 8, 'gist_rainbow' sampled at 10), computed with the
  reference's own expression (visualization.py:385-387, BGR) and flipped to RGB;
* ``matplotlib_version``: the version that produced them.

The module imports cv2, torchvision and ffmpeg at its top; none is needed by ``joints_dict``, so empty stand-in modules take those names for the import.
"""
import importlib.util
import os
import sys
import types

import numpy as np


def main(ref_root: str) -> None:
    for name in ('cv2', 'torchvision', 'ffmpeg'):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    import matplotlib
    import matplotlib.pyplot as plt
    path = os.path.join(ref_root, 'vit_utils', 'visualization.py')
    spec = importlib.util.spec_from_file_location('ref_visualization', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {name: np.asarray(d['skeleton'], dtype=np.int32).reshape(-1, 2) for name, d in mod.joints_dict().items()}

    def palette(color_palette, palette_samples):   # visualization.py:385-387, then BGR -> RGB
        bgr = np.round(np.array(plt.get_cmap(color_palette)(np.linspace(0, 1, palette_samples))) * 255).astype(np.uint8)[:, -2::-1]
        return np.ascontiguousarray(bgr[:, ::-1])
    out['limb_colors'] = palette('jet', 8)
    out['point_colors'] = palette('gist_rainbow', 10)
    out['matplotlib_version'] = np.array(matplotlib.__version__)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'draw_tables.npz')
    np.savez_compressed(dst, **out)
    print(dst, {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main(sys.argv[1])
