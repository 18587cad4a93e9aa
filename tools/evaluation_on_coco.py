#!/usr/bin/env python3
"""COCO keypoint AP / AR of a checkpoint on an annotated image folder: the counterpart of the reference's evaluation_on_coco.py, with the evaluation on the device
(VitPoseHip.cocoeval, easy_vitpose_amd/devcoco.py) instead of a results file handed to pycocotools.

    python tools/evaluation_on_coco.py --model_path vitpose-b-coco.pth --model-name b --yolo_path yolov8s.pt --img_folder_path val2017 --annFile person_keypoints_val2017.json
    python tools/evaluation_on_coco.py --model_path vitpose-b-coco.pth --model-name b --gt-boxes --img_folder_path val2017 --annFile ... --crop affine --flip-test

The reference script's arguments, plus: --gt-boxes (the person boxes come from the annotations, score 1: no detector needed), the handle's --flip-test / --crop /
--pose-nms, --batch (frames per pose call: VitInference.inference_frames), --results FILE (the results list that script writes, its rounding of coordinates under
--round-results), --synthetic SIZE (a seeded peaked checkpoint instead of --model_path).  Images are read with Pillow in ascending image id order, so that equal
scores are ordered as COCOeval's stable sort orders them; the scores are VitInference's `_scores_bbox`.  Prints the ten figures in COCOeval.summarize's wording.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(description='COCO keypoint AP / AR, evaluated on the device')
    ap.add_argument('--model_path', type=str, default=None, help='Path to the ViT Pose model (.pth)')
    ap.add_argument('--model-name', type=str, choices=['s', 'b', 'l', 'h'], default=None, help='[s: ViT-S, b: ViT-B, l: ViT-L, h: ViT-H]')
    ap.add_argument('--yolo_path', type=str, default=None, help='Path to the YOLOv8 model')
    ap.add_argument('--img_folder_path', type=str, required=True, help='Path to the folder containing images')
    ap.add_argument('--annFile', type=str, required=True, help='Path to the COCO annotations file')
    ap.add_argument('--gt-boxes', action='store_true', help='take the person boxes from the annotations (score 1) instead of a detector')
    ap.add_argument('--synthetic', default=None, choices=['s', 'b', 'l', 'h'], help='seeded peaked synthetic checkpoint of this size instead of --model_path')
    ap.add_argument('--dataset', default=None, help='dataset of the checkpoint (default: from the file name; coco with --synthetic)')
    ap.add_argument('--flip-test', action='store_true', help='average each crop with its mirror image')
    ap.add_argument('--crop', default='pad', choices=['pad', 'affine'], help='how a box becomes the crop (affine: the training protocol)')
    ap.add_argument('--pose-nms', type=float, nargs='?', const=0.9, default=None, metavar='THR', help='person score = mean keypoint confidence x box score, OKS NMS')
    ap.add_argument('--batch', type=int, default=8, help='frames per pose call')
    ap.add_argument('--max-records', type=int, default=1 << 20)
    ap.add_argument('--results', default=None, metavar='FILE', help='write the results list of the reference script')
    ap.add_argument('--round-results', action='store_true', help='--results: round the coordinates to whole pixels as the reference script does')
    return ap.parse_args(argv)


def evaluation_on_coco(args):
    import torch
    from PIL import Image
    from easy_vitpose_amd import devcoco as dc
    from easy_vitpose_amd.inference import VitInference
    from easy_vitpose_amd.posenms import PoseNms
    assert (args.model_path is None) != (args.synthetic is None), 'give exactly one of --model_path / --synthetic'
    assert args.gt_boxes or args.yolo_path, 'give --yolo_path or --gt-boxes'
    ann = dc.load_annotations(args.annFile)
    queue = []   # --gt-boxes: the box rows of the frames of the batch in flight, in the order the detector is asked

    def gt_detector(img):
        return queue.pop(0)
    model, dataset = args.model_path, args.dataset
    if args.synthetic:
        from easy_vitpose_amd.configs import model_shape
        from easy_vitpose_amd.synth import synthetic_state_dict
        dataset = dataset or 'coco'
        model = synthetic_state_dict(model_shape(args.synthetic, dataset), 0, peaked=True)
    vit = VitInference(model, gt_detector if args.gt_boxes else args.yolo_path, args.model_name or args.synthetic, dataset=dataset, yolo_size=640, is_video=False,
                       flip_test=True if args.flip_test else None, crop=args.crop, pose_nms=None if args.pose_nms is None else PoseNms(oks_thr=args.pose_nms))
    K = ann.n_joints
    ev = vit._vit_pose.cocoeval(dc.CocoEvalCfg(K, args.max_records, 'coco' if K == 17 else None))
    all_ids, all_kp, all_sc = [], [], []
    for s in range(0, len(ann.image_ids), args.batch):
        idx = list(range(s, min(s + args.batch, len(ann.image_ids))))
        frames = [np.ascontiguousarray(Image.open(os.path.join(args.img_folder_path, ann.file_names[i])).convert('RGB')) for i in idx]
        if args.gt_boxes:
            for i in idx:
                b = ann.gt_box[i].astype(np.float64)
                queue.append(np.concatenate([b[:, :2], b[:, :2] + b[:, 2:], np.ones((len(b), 1))], axis=1))
        results = vit.inference_frames(frames)
        kp, sc, fr = [], [], []
        for f, (poses, scores) in enumerate(zip(results, vit._scores_frames)):
            for key in poses:
                kp.append(poses[key])
                sc.append(scores[key])
                fr.append(f)
                all_ids.append(ann.image_ids[idx[f]])
        kp = np.asarray(kp, np.float32).reshape(len(kp), K, 3)
        all_kp.append(kp)
        all_sc += sc
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        gt = ann.batch(idx)
        n_frames = gt.pop('n_frames')
        ev.update(dev(kp), dev(np.asarray(sc, np.float32)), frame=dev(np.asarray(fr, np.int32)), n_frames=n_frames, **{k: dev(v) for k, v in gt.items()})
    r = ev.result()
    ev.close()
    print(r.summary())
    if args.results:
        dc.results_json(args.results, all_ids, np.concatenate(all_kp + [np.zeros((0, K, 3), np.float32)]), all_sc, rounded=args.round_results)
    return r


if __name__ == '__main__':
    evaluation_on_coco(parse_arguments())
