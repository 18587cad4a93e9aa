#!/usr/bin/env python3
"""Command line driver over ``VitInference`` -- the frame loop of the reference's top-level ``inference.py:19-145`` (same option
names) for the HIP path: read an image or a frame stack, detect (ultralytics if it is installed, else boxes from a file), run the
pose path, track across frames (``is_video``), report FPS and write the ``--save-json`` file in the reference's wire format.

    python -m easy_vitpose_amd.cli --input frame.png --model vitpose-b-coco.pth --yolo yolov8s.pt --output-path out --save-json
    python -m easy_vitpose_amd.cli --input clip.npy --synthetic b --boxes boxes.json --output-path out --save-json
    python -m easy_vitpose_amd.cli --input clip.npy --synthetic b --boxes boxes.json --frame-batch 16   # 16 frames per pose call
    python -m easy_vitpose_amd.cli --input clip.npy --synthetic b --boxes boxes.json --flip-test        # flip-test (COCO-17 pairs; else --flip-pairs FILE.json)
    python -m easy_vitpose_amd.cli --input clip.npy --synthetic b --boxes boxes.json --pose-nms 0.9 --soft-nms   # person scores + OKS pose NMS per frame

    python -m easy_vitpose_amd.cli --input clip.npy --synthetic b --boxes boxes.json --output-path out --save-img        # the frames with the skeletons drawn on them, as PNG

    python -m easy_vitpose_amd.cli --input clip.npy --synthetic b --det-heads heads.npz --det-input 640 640                # the detector's raw heads: decode, filter and box NMS on the device

    python -m easy_vitpose_amd.cli --input clip.npy --synthetic b --det-engine mypkg.engine:make --det-input 640 640          # a detector engine on the same GPU

``--det-engine MODULE:FACTORY`` imports ``FACTORY`` from ``MODULE`` and calls it once: it returns the callable that takes the letterboxed device tensor
``[1, 3, H, W]`` (the letterbox stage, ``devletterbox``: ``--det-input``, fp16 unless ``--det-input-dtype`` says otherwise) and returns the raw head, a device
tensor or an ndarray.  The callable may carry ``nc`` (classes of its head, default 80) and ``head_dtype`` ('fp16' / 'fp32', default: fp32 for an fp32 input, else
fp16).  It is refused together with ``--yolo`` / ``--boxes`` / ``--det-heads``.
``--det-heads`` (an ``.npz`` with the raw YOLOv8 head ``[4 + nc, A]`` of every frame, as an engine on the same GPU leaves it) replaces ``--yolo`` / ``--boxes``:
the boxes then come from the detector stage (``devdetect``, ``VitInference(detect=)``); ``--det-input`` is the size the frames were letterboxed into.
``--save-img`` writes ``<stem>_<frame>.png`` per frame (``VitInference.draw``: skeletons drawn on the device, csrc/drawgeom.h) into the
``--save-json`` directory; a dataset other than COCO-17 needs ``--skeleton FILE.json``.  ``--labels`` adds the reference's ``#<id>: <score>`` tag at every
tracked box of a video (csrc/labelgeom.h, this project's own bitmap font), ``--label-scale S`` sets its size (pixels per font bit, 1..8; implies ``--labels``).
Not rebuilt (outside the hot path): preview windows (``--show``: OpenCV) and video
decoding -- a video is accepted as a ``.npy`` stack ``[frames, H, W, 3]`` uint8 RGB, or as a directory of image files.
``--rotate`` turns the input counter-clockwise as the reference's option does; ``--rotate-on device`` leaves the frames as read and turns them on the GPU
(``VitInference(rotate=)``, the orient stage of ``devorient``).  For a single image file (and a directory of images) the host route inherits the reference's
``Image.rotate(angle)``, which keeps the canvas and cuts the picture at 90 / 270; the device route is the true rotation the reference applies to video.
``--boxes`` (JSON: one ``[[x1, y1, x2, y2, conf], ...]`` list per frame, or a single list used for every frame) replaces the
detector when ultralytics is not installed (there is no network in the build image to fetch it or its weights).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np


def _read_frames(path: str, rotate: int):
    if os.path.isdir(path):
        from PIL import Image
        files = sorted(f for f in os.listdir(path) if f.lower().rsplit('.', 1)[-1] in ('png', 'jpg', 'jpeg', 'bmp'))
        return [np.array(Image.open(os.path.join(path, f)).convert('RGB').rotate(rotate)) for f in files], True
    ext = path[path.rfind('.') + 1:].lower()
    if ext == 'npy':
        arr = np.load(path)
        assert arr.dtype == np.uint8 and arr.ndim == 4 and arr.shape[3] == 3, 'frame stack must be uint8 [frames, H, W, 3] RGB'
        if rotate:
            arr = np.rot90(arr, k=(rotate // 90) % 4, axes=(1, 2))
        return list(np.ascontiguousarray(arr)), True
    assert ext not in ('avi', 'mp4', 'mov'), 'video decoding needs OpenCV: convert the clip to a .npy frame stack or a directory of images'
    from PIL import Image
    return [np.array(Image.open(path).convert('RGB').rotate(rotate))], False


def rotate_arguments(args):
    """--rotate / --rotate-on -> (the angle `_read_frames` turns the frames by on the host, VitInference's rotate=): one of the two is 0"""
    return (0, args.rotate) if args.rotate_on == 'device' else (args.rotate, 0)


def flip_test_argument(args):
    """--flip-test / --flip-pairs -> VitInference's flip_test=: None (off), True (the COCO-17 table) or the pair list of FILE.json."""
    if args.flip_pairs is not None:
        pairs = json.load(open(args.flip_pairs))
        if not (isinstance(pairs, list) and all(isinstance(p, list) and len(p) == 2 and all(isinstance(v, int) for v in p) for p in pairs)):
            raise ValueError(f'{args.flip_pairs}: a JSON list of [left, right] joint index pairs expected')
        return pairs
    return True if args.flip_test else None


def pose_nms_argument(args):
    """--pose-nms [THR] / --soft-nms / --vis-thr V / --sigmas FILE.json -> VitInference's pose_nms=: None (off) or a PoseNms."""
    if args.pose_nms is None:
        if args.soft_nms or args.vis_thr is not None or args.sigmas is not None:
            raise ValueError('--soft-nms, --vis-thr and --sigmas belong to --pose-nms')
        return None
    from easy_vitpose_amd.posenms import PoseNms, load_sigmas
    return PoseNms(oks_thr=args.pose_nms, vis_thr=0.2 if args.vis_thr is None else args.vis_thr, soft=args.soft_nms,
                   sigmas=None if args.sigmas is None else load_sigmas(args.sigmas))


def smooth_argument(args):
    """--smooth / --smooth-fps F / --min-cutoff / --beta / --smooth-missing -> VitInference's smooth=: None (off) or a SmoothCfg."""
    if not args.smooth and args.smooth_fps is None:
        if args.min_cutoff is not None or args.beta is not None or args.smooth_missing is not None:
            raise ValueError('--min-cutoff, --beta and --smooth-missing belong to --smooth')
        return None
    from easy_vitpose_amd.devsmooth import SmoothCfg
    kw = dict(fps=args.smooth_fps, missing=args.smooth_missing or 'reference')
    if args.min_cutoff is not None:
        kw['min_cutoff'] = args.min_cutoff
    if args.beta is not None:
        kw['beta'] = args.beta
    return SmoothCfg(**kw)


def detect_argument(args):
    """--det-heads FILE.npz / --det-input H W / --det-conf / --det-iou -> (the raw head of every frame, VitInference's detect=).  The file holds one array
    [frames, 4 + nc, A], or one [4 + nc, A] array per frame (taken in the order of their names), float16 or float32, YOLOv8's export layout."""
    from easy_vitpose_amd.devdetect import DetectCfg
    with np.load(args.det_heads) as z:
        arrays = [z[k] for k in sorted(z.files)]
    heads = list(arrays[0]) if len(arrays) == 1 and arrays[0].ndim == 3 else arrays
    if not heads or any(h.ndim != 2 or h.shape != heads[0].shape or h.dtype != heads[0].dtype for h in heads):
        raise ValueError(f'{args.det_heads}: one [frames, 4 + nc, A] array or one [4 + nc, A] array per frame expected')
    if heads[0].dtype not in (np.float16, np.float32) or heads[0].shape[0] < 5:
        raise ValueError(f'{args.det_heads}: float16 or float32 heads of at least 5 channels expected, got {heads[0].dtype} {heads[0].shape}')
    kw = {}
    if args.det_conf is not None:
        kw['conf_thr'] = args.det_conf
    if args.det_iou is not None:
        kw['iou_thr'] = args.det_iou
    dataset = args.dataset or 'coco'
    det_class = args.det_class or ('animals' if dataset in ('ap10k', 'apt36k') else 'human')
    cfg = DetectCfg(nc=heads[0].shape[0] - 4, dtype='fp16' if heads[0].dtype == np.float16 else 'fp32', classes=det_class if heads[0].shape[0] - 4 == 80 else None,
                    max_anchors=heads[0].shape[1], max_images=1, **kw)
    return heads, cfg


def det_engine_argument(args):
    """--det-engine MODULE:FACTORY / --det-input H W / --det-input-dtype / --det-conf / --det-iou -> (the engine callable, VitInference's detect=, its letterbox=)"""
    import importlib
    from easy_vitpose_amd.devdetect import DetectCfg
    from easy_vitpose_amd.devletterbox import LetterboxCfg
    if args.yolo is not None or args.boxes is not None or args.det_heads is not None:
        raise ValueError('--det-engine replaces --yolo / --boxes / --det-heads')
    module, sep, factory = args.det_engine.partition(':')
    if not (module and sep and factory):
        raise ValueError(f'--det-engine: MODULE:FACTORY expected, got {args.det_engine!r}')
    engine = getattr(importlib.import_module(module), factory)()
    if not callable(engine):
        raise TypeError(f'--det-engine: {args.det_engine} returned {type(engine).__name__}, not a callable')
    letterbox = LetterboxCfg(tuple(args.det_input), dtype=args.det_input_dtype or 'fp16')
    kw = {}
    if args.det_conf is not None:
        kw['conf_thr'] = args.det_conf
    if args.det_iou is not None:
        kw['iou_thr'] = args.det_iou
    nc = int(getattr(engine, 'nc', 80))
    dataset = args.dataset or 'coco'
    det_class = args.det_class or ('animals' if dataset in ('ap10k', 'apt36k') else 'human')
    detect = DetectCfg(nc=nc, dtype=getattr(engine, 'head_dtype', 'fp32' if letterbox.dtype == 'fp32' else 'fp16'), classes=det_class if nc == 80 else None, max_images=1, **kw)
    return engine, detect, letterbox


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--input', required=True, help='image file, .npy frame stack, or directory of images')
    ap.add_argument('--output-path', default='', help='output directory (required by --save-json)')
    ap.add_argument('--model', default=None, help='ViTPose checkpoint (.pth)')
    ap.add_argument('--synthetic', default=None, choices=['s', 'b', 'l', 'h'], help='seeded peaked synthetic checkpoint of this size instead of --model')
    ap.add_argument('--yolo', default=None, help='detector weights: a YOLOv8 state dict (.npz from tools/export_yolo_state.py, or a plain .pt) runs on the native '
                    'detector network at --det-input; an ultralytics checkpoint needs ultralytics')
    ap.add_argument('--boxes', default=None, help='JSON file with detector boxes (replaces --yolo)')
    ap.add_argument('--det-heads', default=None, metavar='FILE.npz', help='the detector\'s RAW head of every frame ([4 + nc, A], YOLOv8\'s export) instead of --yolo / '
                    '--boxes: best class, confidence threshold, class filter (--det-class; heads of 80 classes) and box NMS run on the device (devdetect)')
    ap.add_argument('--det-input', type=int, nargs=2, default=[640, 640], metavar=('H', 'W'), help='--det-heads: the detector input the frames were letterboxed into')
    ap.add_argument('--det-engine', default=None, metavar='MODULE:FACTORY', help='a detector engine on the same GPU instead of --yolo / --boxes / --det-heads: FACTORY() '
                    'returns the callable that takes the letterboxed device tensor [1, 3, H, W] (--det-input; the letterbox stage, devletterbox) and returns the raw head')
    ap.add_argument('--det-input-dtype', default=None, choices=['fp16', 'fp32', 'u8'], help='--det-engine: the dtype of the letterboxed tensor (default fp16)')
    ap.add_argument('--det-conf', type=float, default=None, help='--det-heads: confidence threshold (default 0.35, the reference\'s)')
    ap.add_argument('--det-iou', type=float, default=None, help='--det-heads: IoU threshold of the box NMS (default 0.7, ultralytics\')')
    ap.add_argument('--dataset', default=None, help='dataset of the checkpoint (default: from the --model file name); required for a ViTPose+ '
                    'checkpoint, whose six datasets are coco, aic, mpii, ap10k, apt36k, wholebody')
    ap.add_argument('--det-class', default=None)
    ap.add_argument('--model-name', default=None, choices=['s', 'b', 'l', 'h'])
    ap.add_argument('--yolo-size', type=int, default=320)
    ap.add_argument('--conf-threshold', type=float, default=0.5)
    ap.add_argument('--rotate', type=int, default=0, choices=[0, 90, 180, 270], help='turn the input by this many degrees counter-clockwise before anything else')
    ap.add_argument('--rotate-on', default='host', choices=['host', 'device'], help='--rotate: host (the default) turns the frames as they are read; device hands them '
                    'on as read and turns them on the GPU (the orient stage, devorient), one upload per frame.  For a single image FILE the host route inherits the '
                    'reference\'s Image.rotate(angle), which keeps the canvas and cuts the picture at 90 / 270; the device route is the true rotation the reference '
                    'applies to video')
    ap.add_argument('--yolo-step', type=int, default=1)
    ap.add_argument('--single-pose', action='store_true')
    ap.add_argument('--tracker', default='host', choices=['host', 'device'], help='video input: the SORT box tracker on the host (tracker.Sort, the default) or on '
                    'the device (devtracker.DeviceSort), with the reference\'s parameters either way')
    ap.add_argument('--save-json', action='store_true')
    ap.add_argument('--show', action='store_true')
    ap.add_argument('--save-img', action='store_true', help='write every frame with its skeletons drawn on it as <stem>_<frame>.png into the output directory')
    ap.add_argument('--skeleton', default=None, metavar='FILE.json', help='--save-img: the limb table [[a, b], ...] of the dataset (built in for COCO-17 only)')
    ap.add_argument('--labels', action='store_true', help='--save-img on video input: write the tag `#<id>: <score>` at the top-left corner of every tracked box')
    ap.add_argument('--label-scale', type=int, default=None, metavar='S', help='--labels: pixels per font bit, 1..8 (default: max(1, min(h, w) // 400) of the frame; '
                    'implies --labels)')
    ap.add_argument('--max-batch', type=int, default=64)
    ap.add_argument('--dtype', default='fp16', choices=['fp16', 'bf16'])
    ap.add_argument('--frame-batch', type=int, default=1, help='frames per pose call: the crops of N frames run as one batch (VitInference.inference_frames)')
    ap.add_argument('--flip-test', action='store_true', help='flip-test: average each crop with its mirror image (the accuracy mode of the reference\'s test '
                    'configs); on its own it stands for the COCO-17 mirror pairs, any other dataset needs --flip-pairs')
    ap.add_argument('--flip-pairs', default=None, metavar='FILE.json', help='mirror joint pairs [[left, right], ...] of the dataset (implies --flip-test)')
    ap.add_argument('--shift-heatmap', action='store_true', help='flip-test: shift the flipped-back heatmaps one pixel right (the reference\'s shift_heatmap)')
    ap.add_argument('--pose-nms', type=float, nargs='?', const=0.9, default=None, metavar='THR', help='person score = mean keypoint confidence x box score, and '
                    'OKS pose NMS per frame at this threshold (default 0.9, the reference\'s oks_thr): duplicate poses leave the output')
    ap.add_argument('--soft-nms', action='store_true', help='--pose-nms: soft OKS NMS (scores decay instead of a hard cut; the reference\'s soft_nms)')
    ap.add_argument('--vis-thr', type=float, default=None, metavar='V', help='--pose-nms: joints at or below this confidence do not count (default 0.2)')
    ap.add_argument('--sigmas', default=None, metavar='FILE.json', help='--pose-nms: per-joint OKS sigmas of the dataset (built in for COCO-17 only)')
    ap.add_argument('--crop', default='pad', choices=['pad', 'affine'], help='how a box becomes the 256 x 192 crop: pad (the default: +10 px, clipped, zero-padded to '
                    '3:4 and resized, as VitInference.inference does) or affine (the training / evaluation protocol: the box extended to 3:4 with image content, '
                    'scaled by --box-scale and warped; not together with --pose-nms)')
    ap.add_argument('--smooth', action='store_true', help='video input: One-Euro smoothing of every tracked person\'s keypoints on the device, keyed by the '
                    'tracker\'s ids (the reference\'s one_euro_filter.py with its defaults: min_cutoff 1.7, beta 0.3, d_cutoff 30)')
    ap.add_argument('--smooth-fps', type=float, default=None, metavar='F', help='--smooth with d_cutoff = F, the frame rate of the video (implies --smooth)')
    ap.add_argument('--min-cutoff', type=float, default=None, help='--smooth: the filter\'s min_cutoff (default 1.7)')
    ap.add_argument('--beta', type=float, default=None, help='--smooth: the filter\'s beta (default 0.3)')
    ap.add_argument('--smooth-missing', default=None, choices=['reference', 'restart'], help='--smooth: a joint at a coordinate <= 0 is reported at -10; afterwards '
                    'the filter blends away from -10 (reference, the default) or starts afresh from the next sample (restart)')
    ap.add_argument('--box-scale', type=float, default=1.25, metavar='S', help='--crop affine: the factor the box is scaled by (the reference\'s 1.25)')
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    assert not args.show, 'preview windows (OpenCV) are outside the HIP hot path: use --save-img or --save-json'
    assert not (args.save_json or args.save_img) or args.output_path, 'Specify an output path if using save-img or save-json flags'
    assert args.skeleton is None or args.save_img, '--skeleton belongs to --save-img'
    assert not (args.labels or args.label_scale is not None) or args.save_img, '--labels / --label-scale belong to --save-img'
    assert (args.model is None) != (args.synthetic is None), 'give exactly one of --model / --synthetic'
    assert args.frame_batch >= 1, '--frame-batch must be at least 1'
    # --det-engine: resolved (and refused together with the other detector options) before any file is read
    engine = det_engine_argument(args) if args.det_engine is not None else None
    assert engine is not None or args.det_input_dtype is None, '--det-input-dtype belongs to --det-engine'

    from easy_vitpose_amd import VitInference
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.jsonio import COCO17_JOINTS, save_json
    frames, is_video = _read_frames(args.input, rotate_arguments(args)[0])
    dataset = args.dataset or ('coco' if not args.model else None)   # --model: VitInference reads it from the file name (a ViTPose+ file needs --dataset)

    detector = args.yolo
    if args.boxes is not None:
        boxes = json.load(open(args.boxes))
        per_frame = bool(boxes) and isinstance(boxes[0], list) and bool(boxes[0]) and isinstance(boxes[0][0], list)
        state = {'i': 0}

        def detector(img):   # noqa: F811 -- one call per detector frame, in order
            b = boxes[min(state['i'], len(boxes) - 1)] if per_frame else boxes
            state['i'] += 1
            return np.asarray(b, dtype=np.float64).reshape(-1, 5)
    detect = None
    if args.det_heads is not None:
        assert args.yolo is None and args.boxes is None, '--det-heads replaces --yolo / --boxes'
        heads, detect = detect_argument(args)
        state = {'i': 0}

        def detector(img):   # noqa: F811 -- the raw head of every detector frame, in order (the last one again beyond the file)
            h = heads[min(state['i'], len(heads) - 1)]
            state['i'] += 1
            return h, tuple(args.det_input)
    letterbox = None
    if engine is not None:
        detector, detect, letterbox = engine
    elif args.yolo is not None and args.boxes is None and VitInference._native_yolo(args.yolo):
        # --yolo FILE.npz (or a plain state dict .pt): the native detector network (devyolo), letterbox -> DeviceYolo -> detect at --det-input
        from easy_vitpose_amd.devletterbox import LetterboxCfg
        letterbox = LetterboxCfg(tuple(args.det_input))
    assert detector is not None, 'give --yolo (ultralytics weights), --boxes, --det-heads or --det-engine'

    skeleton = None
    if args.skeleton is not None:
        from easy_vitpose_amd.draw import load_skeleton
        skeleton = load_skeleton(args.skeleton)
    labels = False
    if args.labels or args.label_scale is not None:
        from easy_vitpose_amd.draw import LabelStyle
        labels = LabelStyle(scale=0 if args.label_scale is None else args.label_scale)   # a scale outside 0..8 is refused here, before anything is loaded
    state_dict = None
    if args.synthetic:
        from easy_vitpose_amd.synth import synthetic_state_dict
        state_dict = synthetic_state_dict(model_shape(args.synthetic, dataset), 0, peaked=True)
    model = VitInference(state_dict if state_dict is not None else args.model, detector, args.model_name or args.synthetic,
                         args.det_class, dataset, args.yolo_size, is_video=is_video, single_pose=args.single_pose,
                         yolo_step=args.yolo_step, dtype=args.dtype, max_batch=args.max_batch,
                         flip_test=flip_test_argument(args), shift_heatmap=args.shift_heatmap, pose_nms=pose_nms_argument(args),
                         crop=args.crop, box_scale=args.box_scale, skeleton=skeleton, tracker='device' if args.tracker == 'device' else None,
                         smooth=smooth_argument(args), detect=detect, letterbox=letterbox, labels=labels, rotate=rotate_arguments(args)[1])
    print(f'>>> Model loaded: {args.model or "synthetic ViTPose-" + args.synthetic.upper()}')
    print(f'>>> Running inference on {args.input}')
    base = os.path.basename(args.input.rstrip('/'))
    stem = base[:base.rfind('.')] if '.' in base else base
    out_dir = os.path.join(args.output_path, base)
    if args.save_img:
        assert args.frame_batch == 1, '--save-img draws the state of the last frame of a pose call: use --frame-batch 1'
        from PIL import Image
        os.makedirs(out_dir, exist_ok=True)
    keypoints, dts = [], []
    for s in range(0, len(frames), args.frame_batch):
        batch = frames[s:s + args.frame_batch]
        t0 = time.time()
        keypoints.extend(model.inference_frames(batch))
        dts.extend([(time.time() - t0) / len(batch)] * len(batch))   # per frame: the batch's time over its frame count
        if args.save_img:   # outside the timed span, as the reference's drawing is
            Image.fromarray(model.draw(confidence_threshold=args.conf_threshold)).save(os.path.join(out_dir, f'{stem}_{s}.png'))
    if is_video:
        tot = sum(len(k) for k in keypoints)
        print(f'>>> Mean inference FPS: {1 / np.mean(dts):.2f}')
        print(f'>>> Total poses predicted: {tot} mean per frame: {tot / len(frames):.2f}')
        print(f'>>> Mean FPS per pose: {tot / max(sum(dts), 1e-9):.2f}')
    if args.save_json:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, stem + '_result.json')
        print('>>> Saving output json')
        save_json(path, keypoints, COCO17_JOINTS if model._vit_pose.K == 17 and model.dataset == 'coco' else None)
    return 0


if __name__ == '__main__':
    sys.exit(main())
