"""Export an ultralytics YOLOv8-detect checkpoint to the plain state dict the native detector network loads (easy_vitpose_amd.devyolo.load_yolo_state,
VitInference(yolo=FILE.npz), cli --yolo FILE.npz):

    python tools/export_yolo_state.py yolov8s.pt yolov8s.npz

It needs ultralytics, so it runs on a machine that has it; it cannot be run, and has not been run, where this project is developed and tested (ultralytics is
installed neither there nor on the GPU machines).  What it writes is `model.model.state_dict()` with the keys prefixed `model.`: every floating-point tensor as
float32.  Parity of the native network against the ultralytics binary on such a file is therefore UNPINNED."""
import sys

import numpy as np


def main(src, dst):
    from ultralytics import YOLO
    net = YOLO(src, task='detect').model
    sd = {k: v.detach().float().cpu().numpy() for k, v in net.state_dict().items() if v.is_floating_point()}
    np.savez(dst, **sd)
    print(f'{dst}: {len(sd)} tensors')


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
