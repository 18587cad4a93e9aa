"""``VitInference`` -- the reference's public class (easy_ViTPose/inference.py:52-336)
with its backend slot filled by the MI355X-native HIP path.

Kept from the reference: constructor signature (:81-90), ``reset`` (:174-185),
``postprocess`` (:187-205), ``inference(img) -> {id: (K,3) (y,x,score)}`` (:221-281),
``pre_img`` (:314-318), the state attributes (:112-116, :274-279) and the exception
types.  Added: ``flip_test=`` (keyword): the reference's test-time flip averaging as a mode
of the engine handle (a pair list, or True for the COCO-17 table); ``pose_nms=`` (keyword, a ``PoseNms``): person scores
(keypoint confidence x box score, the reference's open note at :272) and per-frame OKS pose NMS after the pose call; ``smooth=`` (keyword, True or a
``SmoothCfg``): with ``is_video``, One-Euro smoothing of every tracked person's keypoints on the device (``devsmooth``; the reference's
``post_processing/one_euro_filter.py``), keyed by the tracker's ids, before the result dict and ``draw()``; ``rotate=`` (keyword, 0 / 90 / 180 / 270 degrees
counter-clockwise, the reference's ``--rotate``): the frames arrive as captured and are made upright on the device (``devorient``), results and ``draw()`` in
upright-frame pixels.  Changed on purpose: the per-box Python loop that ran the model once per
crop (:259-272) becomes ONE batched call into the C ABI (``_inference_batch``);
``_inference`` (single crop, :207-219) is still there and returns ``[1, K, 3]``.

Out of scope here: the YOLO detector is third-party;
``yolo`` may be a path (needs ``ultralytics``) or any callable
``img_rgb -> ndarray[n, 5] (x1, y1, x2, y2, conf)``.  With ``detect=`` (keyword, a ``devdetect.DetectCfg``) the
callable returns ``(raw head [4 + nc, A], (in_h, in_w))`` instead and the detector stage (vp_detect: best class, threshold,
class filter, box NMS, letterbox undone) makes the boxes on the device.  With ``letterbox=`` (a ``devletterbox.LetterboxCfg``)
on top of ``detect=`` the callable receives the letterboxed device tensor ``[1, 3, H, W]`` (vp_letterbox_stream) and returns the raw
head alone; the detector stage is fed the letterbox stage's own table.  The SORT tracker is ``tracker.Sort``
on the host by default, ``tracker='device'`` selects the device tracker
(``devtracker.DeviceSort``, vp_tracker_update), and a factory of any object with the
SORT ``update`` interface is taken as it is.
"""
from __future__ import annotations

import dataclasses
import os
import typing
from typing import Optional

import numpy as np

from .configs import IMG_H, IMG_W, infer_dataset_by_path, infer_head_from_state_dict, infer_variant_from_state_dict, model_shape, resolve_flip_pairs
from .cropprep import box_to_cs, frames_crop_params, resize_linear_u8
from .engine import VitPoseHip, decode_heatmaps
from .moe import DATASETS as MOE_DATASETS, is_vitpose_plus
from .draw import DrawStyle, LabelStyle, resolve_skeleton
from .posenms import PoseNms, resolve_sigmas

__all__ = ['VitInference']

MEAN = [0.485, 0.456, 0.406]  # inference.py:32
STD = [0.229, 0.224, 0.225]   # inference.py:33

DETC_TO_YOLO_YOLOC = {        # inference.py:36-48
    'human': [0], 'cat': [15], 'dog': [16], 'horse': [17], 'sheep': [18], 'cow': [19],
    'elephant': [20], 'bear': [21], 'zebra': [22], 'giraffe': [23],
    'animals': [15, 16, 17, 18, 19, 20, 21, 22, 23],
}


def pad_image(image: np.ndarray, aspect_ratio: float):
    """Zero-pad a crop to the given W/H aspect ratio; returns (padded, (left_pad, top_pad)).
    Same contract as ``vit_utils/inference.py:41-70``."""
    h, w = image.shape[:2]
    left = top = 0
    if w / h < aspect_ratio:
        tw = int(aspect_ratio * h)
        left = (tw - w) // 2
        out = np.zeros((h, tw) + image.shape[2:], dtype=image.dtype)
        out[:, left:left + w] = image
    else:
        th = int(w / aspect_ratio)
        top = (th - h) // 2
        out = np.zeros((th, w) + image.shape[2:], dtype=image.dtype)
        out[top:top + h] = image
    return out, (left, top)


class VitInference:
    """ViTPose inference with the MI355X HIP backend (see module docstring)."""

    def __init__(self, model,
                 yolo,
                 model_name: Optional[str] = None,
                 det_class: Optional[str] = None,
                 dataset: Optional[str] = None,
                 yolo_size: Optional[int] = 320,
                 device: Optional[str] = None,
                 is_video: Optional[bool] = False,
                 single_pose: Optional[bool] = False,
                 yolo_step: Optional[int] = 1,
                 *, dtype: str = 'fp16', max_batch: int = 64, tracker=None, flip_test=None, shift_heatmap: bool = False,
                 pose_nms: Optional[PoseNms] = None, crop: str = 'pad', box_scale: float = 1.25, skeleton=None, smooth=None, detect=None, letterbox=None, labels=False,
                 rotate: int = 0):
        # crop='affine': the training-protocol crop (cropprep.box_to_cs, VitPoseHip.infer_frames(crop='affine')) instead of the pad route; refused before anything is loaded
        if crop not in ('pad', 'affine'):
            raise ValueError(f"crop: 'pad' or 'affine' expected, got {crop!r}")
        if crop == 'affine' and pose_nms is not None:
            raise ValueError("pose_nms= does not run together with crop='affine' (the NMS area is defined on the pad route's crop)")
        # rotate: the frames arrive as captured and are turned by this many degrees counter-clockwise (the reference's --rotate) on the device (devorient); 0, 90, 180
        # or 270, refused before anything is loaded
        from .devorient import rotate_code
        self._rot_code, self._rot_k, self._orient = rotate_code(rotate), int(rotate) // 90, None
        if not (tracker is None or tracker == 'device' or callable(tracker)):
            raise ValueError(f"tracker: None (the host Sort), 'device' (devtracker.DeviceSort) or a factory expected, got {tracker!r}")
        # smooth: One-Euro keypoint smoothing per tracked person (devsmooth.SmoothCfg; True = the reference's defaults); refused before anything is loaded
        from .devsmooth import SmoothCfg
        if not (smooth is None or smooth is True or smooth is False or isinstance(smooth, SmoothCfg)):
            raise TypeError(f'smooth: None, True or a SmoothCfg expected, got {smooth!r}')
        self._smooth_cfg = SmoothCfg() if smooth is True else (smooth or None)
        self._smoother = None
        # detect: the detector stage (devdetect.DetectCfg): `yolo(img)` then returns (raw head, (in_h, in_w)) and the box rows come from vp_detect; refused before anything is loaded
        from .devdetect import DetectCfg
        if not (detect is None or isinstance(detect, DetectCfg)):
            raise TypeError(f'detect: None or a DetectCfg expected, got {detect!r}')
        self._detect_cfg, self._detector = detect, None
        # letterbox: the letterbox stage in front of the detector (devletterbox.LetterboxCfg, with detect=): `yolo(tensor)` then receives the letterboxed DEVICE tensor
        # [1, 3, H, W] and returns the raw head (a device tensor or an ndarray); the geometry is the stage's own
        from .devletterbox import LetterboxCfg
        if not (letterbox is None or isinstance(letterbox, LetterboxCfg)):
            raise TypeError(f'letterbox: None or a LetterboxCfg expected, got {letterbox!r}')
        if letterbox is not None and detect is None and not self._native_yolo(yolo):
            raise ValueError('letterbox= feeds the detector stage: give detect= (a DetectCfg) with it')
        self._letterbox_cfg, self._letterbox = letterbox, None
        if not (np.isfinite(box_scale) and box_scale > 0):
            raise ValueError(f'box_scale must be finite and > 0, got {box_scale!r}')
        self.crop, self.box_scale = crop, float(box_scale)
        # labels: draw() writes the `#<id>: <score>` tag of every tracked box (draw.LabelStyle; True = its defaults); off unless asked for
        if not (labels is None or labels is True or labels is False or isinstance(labels, LabelStyle)):
            raise TypeError(f'labels: False, True or a LabelStyle expected, got {labels!r}')
        self._labels = LabelStyle() if labels is True else (labels or None)
        self._skeleton, self._limbs = skeleton, None   # draw(): the limb table is resolved, or refused, when draw is first called (draw.resolve_skeleton)
        state_dict = None
        dataset_given = dataset is not None
        if isinstance(model, (str, os.PathLike)):
            assert os.path.isfile(model), f'The model file {model} does not exist'
            assert not str(model).endswith(('.onnx', '.engine')), \
                'the HIP backend loads .pth checkpoints only (no ONNX / TensorRT dispatch)'
            if dataset is None:
                try:
                    dataset = infer_dataset_by_path(str(model))
                except ValueError:
                    state_dict = self._load_pth(model)
                    if is_vitpose_plus(state_dict):
                        raise ValueError(self._moe_needs_dataset(model)) from None
                    raise
        else:  # an in-memory state dict (extension; used by tests / benchmarks)
            state_dict = model
            assert dataset is not None, 'dataset must be given with an in-memory state dict'
        self._yolo_state = None
        if callable(yolo):
            self.yolo = yolo
        elif self._native_yolo(yolo):
            # the native detector network (devyolo.DeviceYolo): built below, once the handle exists, and wired as letterbox -> DeviceYolo -> detect
            from .devyolo import load_yolo_state
            self._yolo_state = yolo if isinstance(yolo, dict) else load_yolo_state(yolo)
            self.yolo = None
        else:
            assert os.path.isfile(yolo), f'The YOLOv8 model {yolo} does not exist'
            try:
                from ultralytics import YOLO
            except ModuleNotFoundError as e:
                raise ModuleNotFoundError('ultralytics is not installed: pass a callable detector as `yolo`') from e
            self._yolo_model = YOLO(yolo, task='detect')
            self.yolo = self._call_ultralytics

        if device is None:
            device = 'cuda'
        assert str(device).startswith('cuda'), 'the HIP backend runs on an AMD GPU only (no CPU fallback)'
        self.device = device
        self.yolo_size = yolo_size
        self.yolo_step = yolo_step
        self.is_video = is_video
        self.single_pose = single_pose
        self._tracker_factory = tracker
        self.reset()

        self.save_state = True
        self._img = None
        self._yolo_res = None
        self._tracker_res = None
        self._keypoints = None
        self._scores_bbox = None

        assert dataset in ['mpii', 'coco', 'coco_25', 'wholebody', 'aic', 'ap10k', 'apt36k', 'custom'], \
            'The specified dataset is not valid'
        self.dataset = dataset
        if det_class is None:
            det_class = 'animals' if dataset in ['ap10k', 'apt36k'] else 'human'
        self.yolo_classes = DETC_TO_YOLO_YOLOC[det_class]
        assert model_name in [None, 's', 'b', 'l', 'h'], f'The model name {model_name} is not valid'

        if state_dict is None:
            state_dict = self._load_pth(model)
        plus = is_vitpose_plus(state_dict)
        if plus and not dataset_given:   # ViTPose+ (one file, six datasets): the filename cannot tell which head is wanted
            raise ValueError(self._moe_needs_dataset(model))
        if plus and dataset not in MOE_DATASETS:
            raise ValueError(f'dataset {dataset!r} is not one of the ViTPose+ datasets: {", ".join(MOE_DATASETS)}')
        if model_name is None:
            model_name = infer_variant_from_state_dict(state_dict)
        nk = None
        if dataset == 'custom':
            nk = int(np.asarray(state_dict['keypoint_head.final_layer.bias']).shape[0])
        self.target_size = [IMG_W, IMG_H]  # data_cfg['image_size'], ViTPose_common.py:30
        dev_id = int(str(device).split(':')[1]) if ':' in str(device) else 0
        # the decoder comes from the file too: a `vitpose-*-simple` checkpoint (no deconv layers, a 3x3 final conv) loads with no switch
        try:
            head = infer_head_from_state_dict(state_dict)
        except (KeyError, ValueError):   # a dict that is neither: the loader refuses it below, by tensor name, with the exception types it always raised
            head = 'classic'
        shape = model_shape(model_name, None if nk else dataset, nk, head=head)
        # flip_test (the reference's test configs: flip_test=True): a pair list, or True for the COCO-17 table; refused before anything is loaded
        flip_pairs = resolve_flip_pairs(flip_test, dataset, shape.num_keypoints)
        # pose_nms (data_cfg's oks_thr / vis_thr / soft_nms): off unless given; its sigma table is resolved, or refused, before anything is loaded
        if pose_nms is not None and not isinstance(pose_nms, PoseNms):
            raise TypeError(f'pose_nms: a PoseNms (or None) expected, got {type(pose_nms).__name__}')
        self._pose_nms = None
        if pose_nms is not None:
            sig = resolve_sigmas(dataset, shape.num_keypoints, pose_nms.sigmas)
            self._pose_nms = dataclasses.replace(pose_nms, sigmas=tuple(float(v) for v in sig))
        if self._yolo_state is not None:
            import torch   # the native detector runs on torch tensors: torch opens the device before the library does (the other order can leave torch without one)
            torch.cuda.init()
        self._vit_pose = VitPoseHip(shape, state_dict,
                                    dtype=dtype, device_id=dev_id, max_batch=max_batch, dataset=dataset if plus else None)
        if flip_pairs is not None:   # a mode of the handle: every call below (inference, inference_frames, the boxes route) inherits it
            self._vit_pose.set_flip_test(flip_pairs, shift_heatmap)
        if self._yolo_state is not None:
            lb = self._letterbox_cfg or LetterboxCfg(((int(yolo_size) + 31) // 32 * 32,) * 2)
            if lb.dtype != 'fp16' or lb.order != 'rgb':
                raise ValueError(f"yolo=: the native detector network reads the letterbox stage's fp16 RGB tensor, got dtype {lb.dtype!r}, order {lb.order!r}")
            dc = self._detect_cfg
            self.yolo = self._vit_pose.yolo(self._yolo_state, lb.input_hw, input_layout=lb.layout, head_dtype='fp32' if dc is None else dc.dtype,
                                            head_layout=0 if dc is None else dc.layout)
            if dc is None:
                cls = DETC_TO_YOLO_YOLOC[det_class]
                dc = DetectCfg(nc=self.yolo.nc, dtype='fp32', classes=det_class if max(cls) < self.yolo.nc else None)
            elif dc.nc != self.yolo.nc:
                raise ValueError(f'detect=: nc = {dc.nc}, the checkpoint has {self.yolo.nc} classes')
            self._letterbox_cfg, self._detect_cfg = lb, dc
        if self._detect_cfg is not None:
            self._detector = self._vit_pose.detector(dataclasses.replace(self._detect_cfg, max_images=1))
        if self._letterbox_cfg is not None:
            self._letterbox = self._vit_pose.letterbox(self._letterbox_cfg)
        if self._rot_k:
            self._orient = self._vit_pose.orient()
        if tracker == 'device' or self._smooth_cfg is not None:   # the device tracker and the smoother live on the engine's device: built now that there is one
            self.reset()
        self._inference = self._inference_hip

    @staticmethod
    def _native_yolo(yolo) -> bool:
        """yolo= names the native detector network: a state dict, an .npz, or any other file that IS a plain state dict (the file decides, not the packages
        installed).  A file that is not one -- an ultralytics pickle -- goes to ultralytics where that is installed and is otherwise refused with the exporter's
        name.  A callable goes where it always went."""
        if isinstance(yolo, dict):
            return True
        if callable(yolo) or not isinstance(yolo, (str, os.PathLike)):
            return False
        if str(yolo).endswith('.npz'):
            return True
        if not os.path.isfile(yolo):
            return False
        from .devyolo import load_yolo_state
        try:
            load_yolo_state(yolo)
            return True
        except ValueError:
            import importlib.util
            if importlib.util.find_spec('ultralytics') is None:
                raise
            return False

    @staticmethod
    def _load_pth(path):
        import torch
        ckpt = torch.load(path, map_location='cpu', weights_only=True)
        return ckpt['state_dict'] if 'state_dict' in ckpt else ckpt

    @staticmethod
    def _moe_needs_dataset(model) -> str:
        where = f' {model}' if isinstance(model, (str, os.PathLike)) else ''
        return (f'the ViTPose+ checkpoint{where} holds six datasets: pass dataset= one of {", ".join(MOE_DATASETS)}')

    # ----------------------------------------------------------------- glue
    def _call_ultralytics(self, img_rgb):
        results = self._yolo_model(img_rgb[..., ::-1], verbose=False, imgsz=self.yolo_size,
                                   device=self.device if self.device != 'cuda' else 0,   # inference.py:238
                                   classes=self.yolo_classes)[0]
        self._yolo_res = results
        return results.boxes.data.cpu().numpy()[:, :5]

    def reset(self):
        """Ready for a new video (inference.py:174-185)."""
        use_tracker = self.is_video and not self.single_pose
        self.tracker = None
        if use_tracker:
            # the reference's own parameters (inference.py:179-184): with detector-skipped frames (yolo_step > 1) a coasting track's hit streak restarts at
            # every re-match, so min_hits must be 1 there or no pose is reported on detector frames
            min_hits = 3 if self.yolo_step == 1 else 1
            if self._tracker_factory == 'device':   # ... on the device tracker (devtracker.DeviceSort: vp_tracker_update), once the engine exists
                if getattr(self, '_vit_pose', None) is not None:
                    from .devtracker import DeviceSort
                    self.tracker = DeviceSort(self._vit_pose, max_age=self.yolo_step, min_hits=min_hits, iou_threshold=0.3)
            elif self._tracker_factory is None:     # ... on the reference's own choice, the host Sort
                from .tracker import Sort
                self.tracker = Sort(max_age=self.yolo_step, min_hits=min_hits, iou_threshold=0.3)
            else:
                self.tracker = self._tracker_factory()
        # keypoint smoothing is keyed by the tracker's ids, so it runs only where a tracker does; a new video starts with empty filter tables
        if getattr(self, '_smoother', None) is not None:
            self._smoother.close()
        self._smoother = None
        if use_tracker and getattr(self, '_smooth_cfg', None) is not None and getattr(self, '_vit_pose', None) is not None:
            self._smoother = self._vit_pose.smoother(self._smooth_cfg)
        self.frame_counter = 0

    def _detect_rows(self, img, head, input_hw):
        """VitInference(detect=): the detector's raw head of one frame ([4 + nc, A], or [A, 4 + nc] under layout 1, with or without a leading 1) through the detector
        stage's synchronous twin (vp_detect): the [m, 5] rows (x1, y1, x2, y2, score) in frame pixels.  Every row is over DetectCfg.conf_thr already."""
        head = np.asarray(head)
        rows, _, _, count, _ = self._detector.detect_host(head.reshape((1,) + head.shape[-2:]), img.shape[:2], input_hw)
        return rows[:int(count[-1]), :5]

    def _letterbox_rows(self, img, upright=None):
        """VitInference(letterbox=, detect=): the frame goes to the device once, the letterbox stage writes the detector's input tensor there, `yolo(tensor)` returns
        the raw head, and the detector stage undoes the letterbox with the table the letterbox stage returned: the [m, 5] rows in frame pixels.  A head left on the
        device stays there (vp_detect_stream on torch's current stream); an ndarray head goes through the synchronous twin.  `upright` (rotate=): the frame is on
        the device already, made upright by the orient stage, and is read there."""
        tensor, table, _ = self._letterbox.letterbox([self._letterbox.upload(img) if upright is None else upright])
        head = self.yolo(tensor)
        if hasattr(head, 'data_ptr'):
            rows, _, _, count, _ = self._detector.detect(head.reshape((1,) + tuple(head.shape[-2:])), table)
            rows, count = rows.cpu().numpy(), count.cpu().numpy()
        else:
            head = np.asarray(head)
            rows, _, _, count, _ = self._detector.detect_host(head.reshape((1,) + head.shape[-2:]), table)
        return rows[:int(count[-1]), :5]

    def _smooth_results(self, results):
        """VitInference(smooth=): the keypoints of every person of every frame, in frame order, through the smoother's synchronous twin (vp_smooth_update), keyed by
        the tracker's ids on stream 0, before they enter the result dict and draw().  One call per frame (an empty frame ages the filters); a frame with more
        persons than the configuration's max_rows smooths the first max_rows of them."""
        if self._smoother is None:
            return
        K, cap = self._vit_pose.K, self._smoother.cfg.max_rows
        for frame_keypoints, _ in results:
            ids = list(frame_keypoints.keys())[:cap]
            kp = np.stack([frame_keypoints[i] for i in ids]).astype(np.float32) if ids else np.zeros((0, K, 3), np.float32)
            out, _ = self._smoother.update_host(kp, np.array(ids, dtype=np.int32).reshape(-1))
            for k, i in enumerate(ids):
                frame_keypoints[i] = out[k]

    @classmethod
    def postprocess(cls, heatmaps, org_w, org_h):
        """Heatmaps ``[N,K,64,48]`` -> ``[N,K,3]`` (y, x, conf); GPU decode kernel with the
        reference's arguments (inference.py:187-205)."""
        n = heatmaps.shape[0]
        wh = np.tile(np.array([[org_w, org_h]], dtype=np.int32), (n, 1))
        return decode_heatmaps(np.asarray(heatmaps, dtype=np.float32), wh)

    def pre_img(self, img):
        """inference.py:314-318 -- kept for API compatibility (host float path)."""
        org_h, org_w = img.shape[:2]
        img_input = resize_linear_u8(img, self.target_size) / 255
        img_input = ((img_input - MEAN) / STD).transpose(2, 0, 1)[None].astype(np.float32)
        return img_input, org_h, org_w

    def _inference_batch(self, crops: "list[np.ndarray]") -> np.ndarray:
        """N crops (uint8 RGB, any size, already padded to 3:4) -> ``[N, K, 3]``: OpenCV-style 8-bit bilinear
        resize on the host (cropprep.resize_linear_u8; identity for 256x192), then ONE call into the HIP
        library (normalisation is on device).  `inference(img)` does not use this: it hands the whole frame
        to the device crop kernel (`vp_infer_frame`)."""
        if len(crops) == 0:
            return np.empty((0, self._vit_pose.K, 3), dtype=np.float32)
        wh = np.array([[c.shape[1], c.shape[0]] for c in crops], dtype=np.int32)
        batch = np.stack([resize_linear_u8(np.ascontiguousarray(c), self.target_size) for c in crops])
        return self._vit_pose.infer(batch, wh)

    def _inference_hip(self, img: np.ndarray) -> np.ndarray:
        """Drop-in for ``_inference_torch`` (inference.py:320-328): one crop -> ``[1, K, 3]``."""
        return self._inference_batch([img])

    # ------------------------------------------------------------ inference
    def inference(self, img: np.ndarray) -> "dict[typing.Any, typing.Any]":
        """inference.py:221-281 with the crop loop batched: the one-frame case of `inference_frames`."""
        return self.inference_frames([img])[0]

    def inference_frames(self, imgs) -> "list[dict[typing.Any, typing.Any]]":
        """`[self.inference(img) for img in imgs]` with ONE pose call for the crops of all frames (`vp_infer_frames`): the detector
        runs on the same frames and the tracker is updated frame by frame, in order, as that loop would (neither depends on
        keypoints); then every crop of every frame is cropped, padded, resized and run on device from one upload per frame, and the
        offsets are added per crop.  `save_state` keeps the last frame's state."""
        pad_bbox = 10
        dets = []
        upright = None
        if getattr(self, '_orient', None) is not None and len(imgs):
            # rotate=: every frame goes to the device once, as captured, and the orient stage makes it upright there: what the letterbox stage and the pose call read.
            # Host-side consumers (a callable detector without letterbox=, draw()'s image) take np.rot90, by the stage's contract the same bytes
            upright = []
            for s in range(0, len(imgs), 64):
                upright += self._orient.orient([self._orient.upload(img) for img in imgs[s:s + 64]], self._rot_code)
            imgs = [np.ascontiguousarray(np.rot90(img, self._rot_k)) for img in imgs]
        for f, img in enumerate(imgs):
            res_pd = np.empty((0, 5))
            if (self.tracker is None or (self.frame_counter % self.yolo_step == 0 or self.frame_counter < 3)):
                if self._letterbox is not None:
                    det = self._letterbox_rows(img, None if upright is None else upright[f])
                else:
                    det = self.yolo(img) if self._detector is None else self._detect_rows(img, *self.yolo(img))
                det = np.asarray(det, dtype=np.float64).reshape((-1, 5))
                res_pd = det[det[:, 4] > 0.35].reshape((-1, 5))
            self.frame_counter += 1

            ids = None
            if self.tracker is not None:
                res_pd = self.tracker.update(res_pd)
                ids = res_pd[:, 5].astype(int).tolist()
            bboxes = res_pd[:, :4].round().astype(int)
            scores = res_pd[:, 4].tolist()
            if ids is None:
                ids = range(len(bboxes))
            dets.append((bboxes, ids, scores))

        # crop + zero-pad to 3:4 + resize + normalise all happen on device, each frame uploaded once
        frames = [np.ascontiguousarray(img) for img in imgs] if upright is None else upright
        if self.crop == 'affine':
            return self._affine_frames(imgs, frames, dets)
        p9 = frames_crop_params([d[0] for d in dets], [f.shape for f in frames], pad_bbox)
        kps = self._vit_pose.infer_frames(frames, p9)

        results, start = [], 0
        for bboxes, ids, scores in dets:
            params = p9[start:start + len(bboxes), 1:]
            kps_f = kps[start:start + len(bboxes)]
            start += len(bboxes)
            for i in range(len(bboxes)):                       # keep the reference's in-place box update (:261-262)
                bboxes[i] = (params[i, 0], params[i, 1], params[i, 0] + params[i, 2], params[i, 1] + params[i, 3])
            offsets = [np.array([p[1] - p[5], p[0] - p[4]]) for p in params]   # bbox[:2][::-1] - [top_pad, left_pad]
            frame_keypoints, scores_bbox = {}, {}
            for i, (id_, score) in enumerate(zip(ids, scores)):
                k = kps_f[i]
                k[:, :2] += offsets[i]
                frame_keypoints[id_] = k
                scores_bbox[id_] = score
            results.append((frame_keypoints, scores_bbox))
        if self._pose_nms is not None and len(kps):
            # kps holds frame pixels by now (the offsets above were added in place): one call for all frames, NMS per frame on the device
            box = np.array([s for d in dets for s in d[2]], dtype=np.float32)
            score, rank, _ = self._vit_pose.pose_nms_host(kps, box, p9, len(frames), self._pose_nms)
            start = 0
            for (bboxes, ids, scores), (frame_keypoints, scores_bbox) in zip(dets, results):
                for i, id_ in enumerate(ids):
                    if rank[start + i] < 0:   # a duplicate of a better pose of this frame (or beyond max_dets under soft NMS)
                        del frame_keypoints[id_], scores_bbox[id_]
                    else:
                        scores_bbox[id_] = float(score[start + i])
                start += len(bboxes)
        self._smooth_results(results)
        self._scores_frames = [r[1] for r in results]   # `_scores_bbox` of every frame of this call (tools/evaluation_on_coco.py reads a batch's scores here)
        if self.save_state and len(imgs):
            bboxes, ids, scores = dets[-1]
            self._img = imgs[-1]
            self._tracker_res = (bboxes, ids, scores)
            self._keypoints, self._scores_bbox = results[-1]
        return [r[0] for r in results]

    def _affine_frames(self, imgs, frames, dets):
        """the pose call of `inference_frames` under crop='affine': the tracker's boxes go through the affine route and the keypoints arrive in frame
        pixels, so no offset is added; the stored boxes stay the detector's"""
        fidx = np.concatenate([np.full(len(d[0]), f, dtype=np.float64) for f, d in enumerate(dets)] + [np.zeros(0)])
        boxes = np.concatenate([d[0].reshape(-1, 4) for d in dets] + [np.zeros((0, 4), dtype=int)]).astype(np.float32)
        cs = box_to_cs(boxes, self.box_scale) if len(boxes) else np.zeros((0, 4), dtype=np.float32)
        kps = self._vit_pose.infer_frames(frames, np.concatenate([fidx[:, None], cs.astype(np.float64)], axis=1), crop='affine')
        results, start = [], 0
        for bboxes, ids, scores in dets:
            kps_f = kps[start:start + len(bboxes)]
            start += len(bboxes)
            results.append(({id_: kps_f[i] for i, id_ in enumerate(ids)}, {id_: score for id_, score in zip(ids, scores)}))
        self._smooth_results(results)
        self._scores_frames = [r[1] for r in results]
        if self.save_state and len(imgs):
            self._img = imgs[-1]
            self._tracker_res = dets[-1]
            self._keypoints, self._scores_bbox = results[-1]
        return [r[0] for r in results]

    def draw(self, show_yolo=True, show_raw_yolo=False, confidence_threshold=0.5):
        """inference.py:283-312: an RGB copy of the last frame with every kept pose drawn on it -- limbs in the person's colour (the tracker's id, or the
        pose's ordinal in the frame, as the reference's person_index), joints in the joint's colour, joints at or below `confidence_threshold` left out --
        on the device through `VitPoseHip.draw_poses_host` (csrc/drawgeom.h: this project's own integer rasterisation, parity against OpenCV unpinned).
        `show_yolo` with a tracker on: the box outline of every kept pose, in the person's colour, each under its own skeleton; with `VitInference(labels=...)`
        also the reference's `#<id>: <score>` tag at the box's top-left corner, from the tracker's result, under the skeletons (csrc/labelgeom.h: this
        project's own bitmap font, parity against OpenCV's Hershey font unpinned).  NOT provided: `show_raw_yolo`'s detector plot -- the flag is accepted and ignored.  The skeleton is the COCO-17 one for that dataset; any other
        dataset needs `VitInference(skeleton=[[a, b], ...])`, refused here when it is missing."""
        if self._img is None or self._keypoints is None:
            raise RuntimeError('draw(): nothing to draw yet: call inference() first (with save_state on)')
        K = self._vit_pose.K
        if self._limbs is None:
            self._limbs = tuple(map(tuple, resolve_skeleton(self.dataset, K, self._skeleton).tolist()))
        img = np.array(self._img, dtype=np.uint8, order='C', copy=True)
        ids = list(self._keypoints.keys())
        kp = np.stack([self._keypoints[i] for i in ids]).astype(np.float32) if ids else np.zeros((0, K, 3), np.float32)
        boxes = labels = scores = None
        if show_yolo and self.tracker is not None:
            box_of = {i: b for b, i in zip(self._tracker_res[0], self._tracker_res[1])}
            boxes = np.array([box_of[i] for i in ids], dtype=np.float32).reshape(-1, 4)
            if getattr(self, '_labels', None) is not None:
                score_of = dict(zip(self._tracker_res[1], self._tracker_res[2]))
                labels, scores = self._labels, np.array([score_of[i] for i in ids], dtype=np.float32).reshape(-1)
        style = DrawStyle(conf_thr=confidence_threshold, skeleton=self._limbs)
        self._vit_pose.draw_poses_host([img], kp, np.zeros(len(ids), np.int32), style, ids=np.array(ids, dtype=np.int32).reshape(-1), boxes=boxes, labels=labels,
                                       scores=scores)
        return img
