"""Python host object over the C ABI: one ``VitPoseHip`` = one model on one GPU.

The C library owns the weights, workspaces and its HIP stream; numpy / torch are
only used to hand it pointers.  There is no CPU implementation behind this class.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import dataclasses

from . import _capi as capi
from . import moe
from .configs import HEADS, HM_H, HM_W, IMG_H, IMG_W, ModelShape
from ._stage import check_tensor, frame_on, stream_of
from .cropprep import PIX_FORMATS, YUV_MATRIX_IDS, Frame
from .posenms import PoseNms, resolve_sigmas
from .posenms import c_config as nms_c_config
from .draw import LABEL_MAX_ROWS, DrawStyle, LabelStyle, check_label_rows, check_records, check_rows, label_boxes, label_c_config, overlay_label_style, resolve_skeleton
from .draw import c_config as draw_c_config
from .draw import host_frame as host_draw_frame


def _as_f32_numpy(v) -> np.ndarray:
    if hasattr(v, 'detach'):  # torch tensor (bf16 / fp16 checkpoints have no numpy dtype: widen first)
        v = v.detach().float().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v), dtype=np.float32)


def _tensor_descs(state_dict):
    """state dict -> (ctypes array of vp_tensor_desc, list keeping the float32 arrays alive)"""
    sd = state_dict['state_dict'] if 'state_dict' in state_dict else state_dict  # inference.py:163-166
    keep, descs = [], []
    for name, v in sd.items():
        if name.endswith('num_batches_tracked'):
            continue
        a = _as_f32_numpy(v)
        keep.append(a)
        descs.append(capi.vp_tensor_desc(name.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), a.size))
    return (capi.vp_tensor_desc * len(descs))(*descs), keep


def _flip_pairs_array(pairs) -> np.ndarray:
    a = np.asarray(list(pairs) if pairs is not None else [], dtype=np.int64)
    if a.size and (a.ndim != 2 or a.shape[1] != 2):
        raise ValueError(f'flip pairs: [[left, right], ...] expected, got shape {a.shape}')
    return np.ascontiguousarray(a.reshape(-1, 2), dtype=np.int32)


class PinnedArray:
    """numpy view of page-locked host memory (vp_host_alloc): the buffers vp_infer_submit can copy from / to asynchronously."""

    def __init__(self, shape, dtype):
        self._lib = capi.load_library()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._ptr = self._lib.vp_host_alloc(max(n, 1))
        if not self._ptr:
            raise MemoryError(f'vp_host_alloc({n}) failed')
        buf = (C.c_char * max(n, 1)).from_address(self._ptr)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if getattr(self, '_ptr', None):
            self.array = None
            self._lib.vp_host_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _check_boxes(t, dev, n):
    """the box rows of the two draw entries: float32 CUDA [n, >= 4] on `dev`, unit column stride, any positive row stride (n = 'n': any count)"""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise TypeError('boxes: a float32 torch CUDA tensor expected')
    if (t.device != dev or t.ndim != 2 or n not in ('n', t.shape[0]) or t.shape[1] < 4 or (t.shape[0] > 0 and t.stride(1) != 1)
            or (t.shape[0] > 1 and t.stride(0) < 1)):
        raise ValueError(f'boxes: [{n}, >= 4] with unit column stride on {dev} expected, got {tuple(t.shape)} on {t.device}')


class VitPoseHip:
    """ViTPose (backbone + head + decode) on one MI355X through libvitpose_hip.so.

    A ViTPose+ state dict (easy_vitpose_amd/moe.py) loads as it is: ``.experts`` lists its ``(dataset, K)``, ``set_dataset``
    picks the expert every method runs (``dataset=`` at construction does the same; default coco), and ``infer_mixed`` runs
    a different dataset per crop in one call.  ``shape.num_keypoints`` is ignored for such a dict (its coco head has 17)."""

    def __init__(self, shape: ModelShape, state_dict, dtype: str = 'fp16', device_id: int = 0, max_batch: int = 64,
                 dataset: str | None = None):
        self.lib = capi.load_library()
        self.experts = []
        self._moe = moe.is_vitpose_plus(state_dict)
        if self._moe:
            moe.moe_info(state_dict)   # the loader's refusals, with the Python exception types
            shape = dataclasses.replace(shape, num_keypoints=moe.NUM_KEYPOINTS[0])
        elif dataset is not None:
            raise ValueError('dataset= selects an expert of a ViTPose+ state dict; this one is a plain checkpoint')
        self.shape = shape
        self.dtype = dtype
        self.device_id = int(device_id)
        self.max_batch = int(max_batch)
        self.K = shape.num_keypoints
        cfg = capi.vp_config(shape.embed_dim, shape.depth, shape.num_heads, shape.num_keypoints,
                             capi.DTYPES[dtype], self.device_id, self.max_batch)
        h = C.c_void_p()
        capi.check(self.lib.vp_create(C.byref(h), C.byref(cfg)))
        self._h = h
        try:
            self._load(state_dict)
            # the decoder the loader recognised in the state dict: 'classic' (two deconvs + 1x1 conv) or 'simple' (ReLU -> bilinear x 4 -> 3x3 conv)
            self.head = HEADS[int(self.lib.vp_head_kind(self._h))]
            if self.shape.head != self.head:
                self.shape = dataclasses.replace(self.shape, head=self.head)
            if self._moe:
                n, p, ks = C.c_int32(), C.c_int32(), (C.c_int32 * 8)()
                capi.check(self.lib.vp_expert_info(self._h, C.byref(n), C.byref(p), ks), self._h)
                self.part_features = p.value
                self.experts = [(moe.DATASETS[e], int(ks[e])) for e in range(n.value)]
                self.Kmax = max(k for _, k in self.experts)
                self.dataset = 'coco'
                if dataset is not None:
                    self.set_dataset(dataset)
        except Exception:
            self.close()
            raise

    # -------------------------------------------------------------- weights
    def _load(self, state_dict):
        arr, keep = _tensor_descs(state_dict)
        code = self.lib.vp_load_weights(self._h, arr, len(arr))
        if code == capi.VP_ERR_MISSING_TENSOR:
            raise KeyError(capi.last_error(self._h))      # load_state_dict's "Missing key(s)"
        if code == capi.VP_ERR_SHAPE:
            raise RuntimeError(capi.last_error(self._h))  # load_state_dict's "size mismatch"
        capi.check(code, self._h)

    # ------------------------------------------------------------ ViTPose+
    def set_dataset(self, name: str):
        """ViTPose+ handle: every method from now on runs this dataset's expert and head (vp_set_expert); K follows it."""
        names = [d for d, _ in self.experts]
        if not self._moe:
            raise capi.VpError(capi.VP_ERR_STATE, 'set_dataset: a plain checkpoint has one dataset')
        if name not in names:
            raise ValueError(f'unknown dataset {name!r} for this ViTPose+ checkpoint: one of {", ".join(names)}')
        e = names.index(name)
        drops_mode = self.flip_test and not self.flip_test_per_dataset and self.experts[e][1] != self.K   # another K: the switch takes place, the flip-test mode is cleared, VP_ERR_STATE says so
        code = self.lib.vp_set_expert(self._h, e)
        if code == capi.VP_OK or (drops_mode and code == capi.VP_ERR_STATE and not self.flip_test):
            self.dataset, self.K = name, self.experts[e][1]
        capi.check(code, self._h)

    def infer_mixed(self, crops: np.ndarray, datasets, org_wh=None):
        """One call, a dataset per crop (vp_infer_experts): returns ``(out, k)`` -- ``out`` float32 [N, Kmax, 3] where crop i fills
        its first ``k[i]`` joints (the rest are 0), ``k`` int32 [N].  `datasets`: names or expert indices."""
        crops = np.ascontiguousarray(crops)
        fmt = self._fmt(crops)
        n = crops.shape[0]
        datasets = list(datasets)
        assert len(datasets) == n, 'one dataset per crop'
        ids = self._dataset_ids(datasets, n)
        out = np.empty((n, self.Kmax, 3), dtype=np.float32)
        wh = None if org_wh is None else np.ascontiguousarray(org_wh, dtype=np.int32).reshape(n, 2)
        if n:
            capi.check(self.lib.vp_infer_experts(self._h, crops.ctypes.data, fmt, n, ids.ctypes.data,
                                                 None if wh is None else wh.ctypes.data, out.ctypes.data), self._h)
        ks = np.array([self.experts[i][1] if 0 <= i < len(self.experts) else 0 for i in ids], dtype=np.int32)
        return out, ks

    def _dataset_ids(self, datasets, n: int) -> np.ndarray:
        """`datasets` (names or expert indices, one per crop) -> int32 [n] expert ids (an unknown name becomes -1: the library refuses it, naming the crop)"""
        if not self._moe:
            raise capi.VpError(capi.VP_ERR_STATE, 'datasets=: the handle holds a plain (single-dataset) checkpoint, not a ViTPose+ one')
        names = [d for d, _ in self.experts]
        ids = np.ascontiguousarray([names.index(d) if isinstance(d, str) and d in names else (d if not isinstance(d, str) else -1)
                                    for d in datasets], dtype=np.int32)
        if len(ids) != n:   # the library reads n ids
            raise ValueError(f'datasets: one per crop expected ({n}), got {len(ids)}')
        return ids

    def dataset_k(self, datasets) -> np.ndarray:
        """int32 [n]: the joints each row of a per-crop dataset call fills (the rest of its Kmax joints are 0)"""
        datasets = list(datasets)
        return np.array([self.experts[i][1] for i in self._dataset_ids(datasets, len(datasets))], dtype=np.int32)

    def infer_mixed_device(self, d_crops, datasets, d_out, org_wh=None, stream=None):
        """`infer_mixed` on device-resident torch tensors, stream-ordered (vp_infer_experts_device_stream, contract in include/vitpose_hip.h):
        `d_crops` as in `infer_device`, `datasets` one name or expert index per crop (host), `d_out` float32 CUDA with n x Kmax x 3 elements --
        row i fills its first K of its dataset's joints (`dataset_k`), the rest are 0, rows in the caller's order, bit for bit `infer_mixed`'s.
        `org_wh`: int32 CUDA [n, 2] or None.  `stream`: a torch stream or a raw hipStream_t value (None: torch's current stream); ordering and host
        behaviour as `infer_device(ordered=True)` -- nothing blocks the host, consume `d_out` on that stream.  The active dataset is unchanged."""
        import torch
        assert d_crops.is_cuda and d_out.is_cuda and d_crops.is_contiguous() and d_out.is_contiguous()
        fmt = capi.VP_INPUT_U8_NHWC if d_crops.dtype == torch.uint8 else capi.VP_INPUT_F32_NCHW
        n = d_crops.shape[0]
        ids = self._dataset_ids(datasets, n)
        assert d_out.dtype == torch.float32 and d_out.numel() == n * self.Kmax * 3
        whp = None
        if org_wh is not None:
            assert org_wh.is_cuda and org_wh.dtype == torch.int32 and org_wh.numel() == 2 * n
            whp = org_wh.data_ptr()
        if stream is None:
            stream = torch.cuda.current_stream(d_crops.device)
        cs = stream.cuda_stream if hasattr(stream, 'cuda_stream') else int(stream)
        capi.check(self.lib.vp_infer_experts_device_stream(self._h, d_crops.data_ptr(), fmt, n, ids.ctypes.data, whp, d_out.data_ptr(), cs), self._h)
        return d_out

    # ------------------------------------------------------------ inference
    @staticmethod
    def _fmt(crops: np.ndarray):
        if crops.dtype == np.uint8:
            assert crops.ndim == 4 and crops.shape[1:] == (IMG_H, IMG_W, 3), \
                f'uint8 crops must be [N,{IMG_H},{IMG_W},3], got {crops.shape}'
            return capi.VP_INPUT_U8_NHWC
        assert crops.dtype == np.float32 and crops.ndim == 4 and crops.shape[1:] == (3, IMG_H, IMG_W), \
            f'float32 crops must be [N,3,{IMG_H},{IMG_W}], got {crops.dtype} {crops.shape}'
        return capi.VP_INPUT_F32_NCHW

    def infer(self, crops: np.ndarray, org_wh=None) -> np.ndarray:
        """crops (uint8 NHWC raw, or float32 NCHW normalised) -> float32 [N, K, 3] (y, x, conf)."""
        crops = np.ascontiguousarray(crops)
        fmt = self._fmt(crops)
        n = crops.shape[0]
        out = np.empty((n, self.K, 3), dtype=np.float32)
        if n == 0:
            return out
        wh = None if org_wh is None else np.ascontiguousarray(org_wh, dtype=np.int32).reshape(n, 2)
        capi.check(self.lib.vp_infer(self._h, crops.ctypes.data, fmt, n,
                                     None if wh is None else wh.ctypes.data, out.ctypes.data), self._h)
        return out

    def infer_device(self, d_crops, d_out, org_wh=None, sync: bool = True, ordered: bool = True):
        """Device-resident torch tensors in/out (no copies).  With `ordered` (default) the call goes through the stream-ordered entry
        (vp_infer_device_stream, contract in include/vitpose_hip.h): the library's kernels are ordered after everything already
        enqueued on torch's CURRENT stream (the producers of `d_crops`) and torch work enqueued afterwards waits for them -- `d_out`
        can be consumed by the next torch op without a host synchronisation.  WHERE the kernels run depends on the batch: up to 16
        crops (`VP_CALLER_STREAM`) they are launched on torch's current stream itself -- work the caller enqueues on that stream
        afterwards runs BEHIND them, not beside them, and the handle stays busy on that stream until the next call, `synchronize()` or
        `close()`; larger batches run on the library's own stream, fenced against the caller's with two events (work enqueued on the
        caller's stream afterwards waits for them too, other streams overlap freely).  `sync` additionally blocks the host until the
        result is complete.  `ordered=False`: the library's own stream with no ordering against torch's streams (vp_infer_device)."""
        import torch
        assert d_crops.is_cuda and d_out.is_cuda and d_crops.is_contiguous() and d_out.is_contiguous()
        fmt = capi.VP_INPUT_U8_NHWC if d_crops.dtype == torch.uint8 else capi.VP_INPUT_F32_NCHW
        n = d_crops.shape[0]
        assert d_out.dtype == torch.float32 and d_out.numel() == n * self.K * 3
        whp = None
        if org_wh is not None:
            assert org_wh.is_cuda and org_wh.dtype == torch.int32 and org_wh.numel() == 2 * n
            whp = org_wh.data_ptr()
        if ordered:
            cs = torch.cuda.current_stream(d_crops.device).cuda_stream
            capi.check(self.lib.vp_infer_device_stream(self._h, d_crops.data_ptr(), fmt, n, whp, d_out.data_ptr(), cs), self._h)
            if sync:
                self.synchronize()
        else:
            capi.check(self.lib.vp_infer_device(self._h, d_crops.data_ptr(), fmt, n, whp, d_out.data_ptr(), int(sync)), self._h)
        return d_out

    def submit(self, crops: np.ndarray, out: np.ndarray, org_wh=None) -> int:
        """Asynchronous host path (vp_infer_submit): enqueue one batch (<= max_batch crops) and return its slot; `crops`,
        `org_wh` and `out` must stay alive and untouched until `wait(slot)`.  Pinned buffers (PinnedArray) make the copies
        overlap the previous batch's compute; two batches may be in flight."""
        assert crops.flags['C_CONTIGUOUS'] and out.flags['C_CONTIGUOUS'] and out.dtype == np.float32
        n = crops.shape[0]
        assert out.size == n * self.K * 3
        wh = None if org_wh is None else np.ascontiguousarray(org_wh, dtype=np.int32).reshape(n, 2)
        self._inflight_wh = getattr(self, '_inflight_wh', {})
        slot = C.c_int32(-1)
        capi.check(self.lib.vp_infer_submit(self._h, crops.ctypes.data, self._fmt(crops), n, None if wh is None else wh.ctypes.data,
                                            out.ctypes.data, C.byref(slot)), self._h)
        self._inflight_wh[slot.value] = (crops, wh, out)
        return slot.value

    def wait(self, slot: int):
        capi.check(self.lib.vp_infer_wait(self._h, int(slot)), self._h)
        getattr(self, '_inflight_wh', {}).pop(int(slot), None)

    def infer_flip(self, crops: np.ndarray, flip_pairs, org_wh=None, shift_heatmap: bool = False, return_heatmaps: bool = False):
        """Flip-test inference (reference head `inference_model(x, flip_pairs)` + `flip_back`, topdown_heatmap_simple_head.py:
        195-218, post_transforms.py:110-147): average of the heatmaps of the crops and of their flipped-back mirror images,
        then the usual decode.  `flip_pairs`: the dataset's mirror joint pairs [[l, r], ...] (the reference ships none)."""
        crops = np.ascontiguousarray(crops)
        n = crops.shape[0]
        pairs = np.ascontiguousarray(np.asarray(flip_pairs, dtype=np.int32).reshape(-1, 2))
        wh = None if org_wh is None else np.ascontiguousarray(org_wh, dtype=np.int32).reshape(n, 2)
        out = np.empty((n, self.K, 3), dtype=np.float32)
        hm = np.empty((n, self.K, HM_H, HM_W), dtype=np.float32) if return_heatmaps else None
        if n:
            capi.check(self.lib.vp_infer_flip(self._h, crops.ctypes.data, self._fmt(crops), n,
                                              None if wh is None else wh.ctypes.data, pairs.ctypes.data if len(pairs) else None,
                                              len(pairs), int(bool(shift_heatmap)), out.ctypes.data,
                                              None if hm is None else hm.ctypes.data), self._h)
        return (out, hm) if return_heatmaps else out

    def set_flip_test(self, pairs, shift_heatmap: bool = False):
        """Flip-test as a mode of the handle (vp_set_flip_test, contract in include/vitpose_hip.h): from now on `infer`, `infer_device`,
        `submit` / `wait`, `infer_frame`, `infer_frames` and `infer_boxes` return the keypoints of the average of each crop's heatmaps and
        the flipped-back heatmaps of its mirror image, and `heatmaps` returns that average.  The mirror images ride in the same forward,
        so a chunk holds ``max_batch // 2`` crops (`submit` takes that many at most).  `pairs`: the dataset's mirror joint pairs
        [[l, r], ...], validated against the active head's K.  `tokens`, `infer_flip` are not affected; `infer_mixed` refuses while
        the mode is on (`set_flip_test_datasets` is the form it runs under).  A ViTPose+ handle: `set_dataset` to a head with another K clears the mode and raises."""
        pairs = _flip_pairs_array(pairs)
        capi.check(self.lib.vp_set_flip_test(self._h, pairs.ctypes.data if len(pairs) else None, len(pairs), int(bool(shift_heatmap))), self._h)

    def set_flip_test_datasets(self, pairs_by_dataset, shift_heatmap: bool = False):
        """The flip-test mode of a ViTPose+ handle with one pair table per dataset (vp_set_flip_test_experts, contract in include/vitpose_hip.h):
        `pairs_by_dataset` maps every dataset of the checkpoint -- by name or expert index -- to its mirror joint pairs [[l, r], ...], each validated
        against that dataset's K.  A dataset that is missing, named twice or unknown raises ValueError naming it before the library is called (it would
        silently mirror every joint onto itself).  While it is on, every method `set_flip_test` covers runs under the active dataset's table,
        `set_dataset` keeps the mode whatever the K, and `infer_mixed`, `infer_mixed_device`, `infer_frames(datasets=)` and `infer_boxes(datasets=)`
        return each crop's flip-test keypoints under its own dataset's table (a chunk holds ``max_batch // 2`` crops).  `clear_flip_test`
        switches it off, `set_flip_test` replaces it by the single-table mode."""
        if not self._moe:
            raise capi.VpError(capi.VP_ERR_STATE, 'set_flip_test_datasets: the handle holds a plain (single-dataset) checkpoint, not a ViTPose+ one')
        names = [d for d, _ in self.experts]
        by_expert = {}
        for key, pairs in dict(pairs_by_dataset).items():
            if isinstance(key, str):
                if key not in names:
                    raise ValueError(f'unknown dataset {key!r} for this ViTPose+ checkpoint: one of {", ".join(names)}')
                e = names.index(key)
            else:
                e = int(key)
                if not 0 <= e < len(names):
                    raise ValueError(f'unknown expert index {key!r} for this ViTPose+ checkpoint: 0 .. {len(names) - 1}')
            if e in by_expert:
                raise ValueError(f'dataset {names[e]!r} is given twice (by name and by expert index)')
            by_expert[e] = _flip_pairs_array(pairs)
        missing = [names[e] for e in range(len(names)) if e not in by_expert]
        if missing:
            raise ValueError(f'set_flip_test_datasets: no pairs for {", ".join(missing)} (give [] for a dataset without mirror pairs)')
        counts = np.ascontiguousarray([len(by_expert[e]) for e in range(len(names))], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([by_expert[e].reshape(-1, 2) for e in range(len(names))]), dtype=np.int32)
        capi.check(self.lib.vp_set_flip_test_experts(self._h, flat.ctypes.data if len(flat) else None, counts.ctypes.data, int(bool(shift_heatmap))), self._h)

    def clear_flip_test(self):
        """Back to the default mode (vp_clear_flip_test)."""
        capi.check(self.lib.vp_clear_flip_test(self._h), self._h)

    @property
    def flip_test(self) -> bool:
        return bool(self.lib.vp_flip_test_enabled(self._h))

    @property
    def flip_test_per_dataset(self) -> bool:
        """the mode is on with one pair table per dataset (`set_flip_test_datasets`)"""
        return self.lib.vp_flip_test_enabled(self._h) == 2

    def infer_frame(self, frame: np.ndarray, params: np.ndarray) -> np.ndarray:
        """Whole frame + crop geometry (cropprep.crop_params) -> [n, K, 3] in padded-crop pixels (vp_infer_frame)."""
        frame = np.ascontiguousarray(frame)
        assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
        params = np.ascontiguousarray(params, dtype=np.int32).reshape(-1, 8)
        n = params.shape[0]
        out = np.empty((n, self.K, 3), dtype=np.float32)
        if n == 0:
            return out
        capi.check(self.lib.vp_infer_frame(self._h, frame.ctypes.data, frame.shape[0], frame.shape[1],
                                           params.ctypes.data, n, out.ctypes.data), self._h)
        return out

    @staticmethod
    def _crop_mode(crop) -> bool:
        """True for crop='affine', False for crop='pad' (the default at every layer); anything else is refused"""
        if crop not in ('pad', 'affine'):
            raise ValueError(f"crop: 'pad' or 'affine' expected, got {crop!r}")
        return crop == 'affine'

    def infer_frames(self, frames, params: np.ndarray, datasets=None, crop: str = 'pad'):
        """The crops of several frames in one call (vp_infer_frames): params [n, 9] (cropprep.frames_crop_params) -> [n, K, 3] in
        padded-crop pixels.  `datasets` (a ViTPose+ handle: one name or expert index per crop, as in `infer_mixed`): a dataset per crop in the
        same call (vp_infer_frames_experts) -- returns ``(out, k)`` as `infer_mixed` does, ``out`` [n, Kmax, 3] with row i's first ``k[i]``
        joints filled, bit for bit `infer_mixed` on the host-prepared crops.  `frames`: numpy uint8 [H, W, 3] arrays (host path: one upload of the row band each frame's crops cover),
        or torch uint8 CUDA tensors [H, W, 3] on this handle's device (read in place, once torch's current stream on that
        device has been synchronised), or `Frame` objects (`Frame.rgb / bgr / nv12`: BGR, NV12 surfaces, pitched planes; vp_infer_images) -- formats may differ
        within a call, and the result has the bits of the call on `cropprep.to_rgb` of every frame.  A bare array or tensor is RGB; rows at a pitch (strides
        (pitch, 3, 1)) pass in place.  A list that mixes host and device frames raises TypeError.
        `crop='affine'` (vp_infer_images_affine): the training-protocol crop instead of the pad route.  `params` is then float [n, 5]
        (frame, cx, cy, S_w, S_h) -- the frame index and a `cropprep.box_to_cs` row -- and the result is [n, K, 3] in FRAME pixels, the bits of `infer` on
        `cropprep.affine_crops_host` followed by `cropprep.affine_back_map`.  Not together with `datasets`."""
        affine = self._crop_mode(crop)
        if affine and datasets is not None:
            raise ValueError("infer_frames: crop='affine' does not run together with datasets= (the affine route runs the handle's active dataset)")
        if affine:
            p5 = np.asarray(params, dtype=np.float64).reshape(-1, 5)
            fidx = p5[:, 0].astype(np.int32)
            if not (p5[:, 0] == fidx).all():
                raise ValueError("infer_frames: crop='affine' takes params [n, 5] = (frame, cx, cy, S_w, S_h) with a whole frame index")
            cs = np.ascontiguousarray(np.asarray(params).reshape(-1, 5)[:, 1:], dtype=np.float32)
            params = np.zeros((len(p5), 9), dtype=np.int32)
        params = np.ascontiguousarray(params, dtype=np.int32).reshape(-1, 9)
        n = params.shape[0]
        frames = [self._as_frame(f, i) for i, f in enumerate(frames)]
        on_dev = [f.on_device for f in frames]
        if any(on_dev) and not all(on_dev):
            raise TypeError('frames: all numpy arrays (host) or all torch CUDA tensors (device), not a mix')
        on_device = bool(frames) and all(on_dev)
        table = self._image_table(frames)
        ids = None if datasets is None else self._dataset_ids(datasets, n)
        out = np.empty((n, self.K if ids is None else self.Kmax, 3), dtype=np.float32)
        if n and on_device:
            import torch
            torch.cuda.current_stream(torch.device('cuda', self.device_id)).synchronize()   # the frames are complete before the library reads them
        if n and affine:
            capi.check(self.lib.vp_infer_images_affine(self._h, table, len(frames), int(on_device), fidx.ctypes.data, cs.ctypes.data, n, out.ctypes.data), self._h)
        elif n:
            capi.check(self.lib.vp_infer_images(self._h, table, len(frames), int(on_device), params.ctypes.data, n, None if ids is None else ids.ctypes.data,
                                                out.ctypes.data), self._h)
        return out if ids is None else (out, self.dataset_k(ids))

    @staticmethod
    def _as_frame(f, i: int) -> Frame:
        """entry i of a frame list as a `Frame`: a bare [H, W, 3] array or tensor means RGB.  Rows at a pitch (strides (pitch, 3, 1)) pass in place; any other
        host layout is copied, any other device layout refused."""
        if isinstance(f, Frame):
            return f
        try:
            if hasattr(f, 'data_ptr'):
                if not f.is_cuda:
                    raise TypeError('device frames must be torch uint8 CUDA tensors')
                return Frame.rgb(f)
            f = np.asarray(f)
            if f.dtype != np.uint8:
                raise TypeError(f'uint8 expected, got {f.dtype}')
            if f.ndim == 3 and f.shape[2] == 3:
                try:
                    return Frame.rgb(f)
                except ValueError:
                    return Frame.rgb(np.ascontiguousarray(f))   # reversed channels, a column step, ...: not a vp_image
            return Frame.rgb(f)
        except (TypeError, ValueError) as e:
            raise type(e)(f'frame {i}: {e}') from None

    def _image_table(self, frames, device_only: bool = False):
        """the vp_image table of `frames` (Frame objects; they keep the planes alive)"""
        table = (capi.vp_image * max(len(frames), 1))()
        for i, f in enumerate(frames):
            if device_only and not f.on_device:
                raise TypeError(f'frame {i}: torch uint8 CUDA tensors expected')
            if f.on_device:
                import torch
                frame_on(f, i, torch.device('cuda', self.device_id))
            p0, p1 = f.pointers()
            table[i] = capi.vp_image((C.c_void_p * 2)(p0, p1), (C.c_int64 * 2)(*f.pitch), f.h, f.w, PIX_FORMATS[f.format], YUV_MATRIX_IDS[f.matrix])
        return table

    def infer_boxes(self, frames, boxes, frame_index=None, pad: int = 10, out=None, crop_params: bool = False, status: bool = False, datasets=None,
                    nms: PoseNms | None = None, box_scores=None, crop: str = 'pad', box_scale: float = 1.25, cs: bool = False):
        """Detector boxes on device frames -> keypoints in FRAME pixels, all on the device (vp_infer_boxes_stream, contract in
        include/vitpose_hip.h).  `frames`: torch uint8 CUDA tensors [H, W, 3] on this handle's device (RGB; rows may be pitched: a view of a wider buffer),
        or `Frame` objects over device planes (`Frame.bgr`, `Frame.nv12`: vp_infer_boxes_images_stream), read in place; `boxes`: float32 CUDA
        [n, >= 4] (x1, y1, x2, y2, ...) with unit column stride, e.g. a detector's [n, 6] output as it is; `frame_index`: int32 CUDA [n]
        (None: every box on frame 0); `pad`: pixels added on every side before clipping.  Returns `out` float32 [n, K, 3] (allocated
        when not given), plus int32 [n, 9] crop params (cropprep.frames_crop_params rows) and int32 [n] status (0 ok, 1 bad frame index,
        2 non-finite box, 3 empty box; such rows are all zero) when asked for.  Everything is enqueued on torch's current stream without
        a host synchronisation, under the ordering notes of `infer_device`: consume the results with torch ops on that stream.
        `datasets` (a ViTPose+ handle: one name or expert index per box, on the host, as in `infer_mixed`): a dataset per box in the same call
        (vp_infer_boxes_experts_stream) -- `out` is then [n, Kmax, 3], row i's first `dataset_k(datasets)[i]` joints filled and the rest 0;
        crop params and status are the plain call's.
        `nms` (a PoseNms): person scores and per-frame OKS pose NMS run behind the boxes entry on the same stream (`pose_nms`); the call then returns
        (out, score, rank, count[, crop_params][, status]).  The box scores are `box_scores` (float32 CUDA [n]) or column 4 of `boxes`.  Not together with
        `datasets`: poses of different joint layouts are not comparable.
        `crop='affine'` (vp_infer_boxes_affine_stream): the training-protocol crop -- the box extended to 3:4 with image content and scaled by `box_scale`
        (the reference's 1.25), not clipped to the frame, `pad` unused.  Returns ``(out[, cs][, status])``: `cs=True` adds float32 [n, 4] (cx, cy, S_w, S_h)
        per box (`cropprep.box_to_cs`; a zero row where the status is not 0).  The keypoints have the bits of `infer_frames(crop='affine')` on those rows.
        Not together with `nms` (its area is the pad route's crop), `datasets` or `crop_params`."""
        import torch
        dev = torch.device('cuda', self.device_id)
        affine = self._crop_mode(crop)
        if affine:
            if nms is not None:
                raise ValueError("infer_boxes: nms= does not run together with crop='affine' (the NMS area is defined on the pad route's crop)")
            if datasets is not None:
                raise ValueError("infer_boxes: crop='affine' does not run together with datasets= (the affine route runs the handle's active dataset)")
            if crop_params:
                raise ValueError("infer_boxes: crop='affine' has no crop params: ask for cs=True")
            if not (np.isfinite(box_scale) and box_scale > 0):
                raise ValueError(f'infer_boxes: box_scale must be finite and > 0, got {box_scale!r}')
        elif cs:
            raise ValueError("infer_boxes: cs=True belongs to crop='affine' (the pad route returns crop_params)")
        if nms is not None:
            if datasets is not None:
                raise ValueError('infer_boxes: nms= does not run together with datasets= (poses of different joint layouts are not comparable)')
            if not isinstance(nms, PoseNms):
                raise TypeError(f'nms: a PoseNms expected, got {type(nms).__name__}')
            if box_scores is None and not (hasattr(boxes, 'ndim') and boxes.ndim == 2 and boxes.shape[1] >= 5):
                raise ValueError('infer_boxes: nms= needs the box scores: box_scores=, or boxes with a score in column 4')
        frames = [self._as_frame(f, i) for i, f in enumerate(frames)]
        table = self._image_table(frames, device_only=True)
        if not (isinstance(boxes, torch.Tensor) and boxes.is_cuda and boxes.dtype == torch.float32):
            raise TypeError('boxes: a float32 torch CUDA tensor expected')
        if boxes.device != dev:
            raise ValueError(f'boxes live on {boxes.device}, the handle on {dev}')
        if boxes.ndim != 2 or boxes.shape[1] < 4 or (boxes.shape[0] > 0 and boxes.stride(1) != 1):
            raise ValueError(f'boxes: [n, >= 4] with unit column stride expected, got {tuple(boxes.shape)} strides {boxes.stride()}')
        n = boxes.shape[0]
        row_stride = boxes.stride(0) if n > 1 else max(boxes.stride(0), 4)   # one row: its stride is never used
        fip = None
        if frame_index is not None:
            check_tensor('frame_index', frame_index, torch.int32, (n,), dev)
            fip = frame_index.data_ptr()
        ids = None if datasets is None else self._dataset_ids(datasets, n)
        K = self.K if ids is None else self.Kmax
        if out is None:
            out = torch.empty((n, K, 3), dtype=torch.float32, device=dev)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                  and out.device == dev and out.numel() == n * K * 3):
            raise ValueError(f'out: a contiguous float32 tensor of {n} x {K} x 3 on {dev} expected')
        cp = torch.empty((n, 9), dtype=torch.int32, device=dev) if crop_params or nms is not None else None
        st = torch.empty((n,), dtype=torch.int32, device=dev) if status or nms is not None else None
        bsc = None if nms is None else (box_scores if box_scores is not None else boxes[:, 4])
        want_cs, cs = cs, stream_of(dev)
        if affine:
            d_cs = torch.empty((n, 4), dtype=torch.float32, device=dev) if want_cs else None
            capi.check(self.lib.vp_infer_boxes_affine_stream(self._h, table, len(frames), boxes.data_ptr(), row_stride, fip, n, float(box_scale), out.data_ptr(),
                                                             None if d_cs is None else d_cs.data_ptr(), None if st is None else st.data_ptr(), cs), self._h)
            if d_cs is None and st is None:
                return out
            return (out,) + tuple(t for t in (d_cs, st) if t is not None)
        capi.check(self.lib.vp_infer_boxes_images_stream(self._h, table, len(frames), boxes.data_ptr(), row_stride, fip, n, int(pad),
                                                         None if ids is None else ids.ctypes.data, out.data_ptr(), None if cp is None else cp.data_ptr(),
                                                         None if st is None else st.data_ptr(), cs), self._h)
        if nms is not None:   # the same stream, directly behind the boxes entry
            score, rank, count = self.pose_nms(out, bsc, cp, len(frames), nms, status=st)
            return (out, score, rank, count) + ((cp,) if crop_params else ()) + ((st,) if status else ())
        if cp is None and st is None:
            return out
        return (out,) + tuple(t for t in (cp, st) if t is not None)

    # ------------------------------------------------------------ pose NMS
    def _nms_sigmas(self, cfg: PoseNms, K: int) -> np.ndarray:
        """the sigma table of a call.  The handle of a plain checkpoint does not know its dataset: its 17 joints are taken as COCO's when `cfg.sigmas` is None
        (VitInference, which knows the dataset, resolves them first)."""
        if not isinstance(cfg, PoseNms):
            raise TypeError(f'a PoseNms expected, got {type(cfg).__name__}')
        return resolve_sigmas(getattr(self, 'dataset', 'coco') if self._moe else 'coco', K, cfg.sigmas)

    def pose_nms(self, keypoints, box_scores, crop_params, n_frames: int, cfg: PoseNms, status=None):
        """Person scores and per-frame OKS pose NMS on the device (vp_pose_nms_stream, contract in include/vitpose_hip.h), stream-ordered on torch's current
        stream without a host synchronisation.  `keypoints`: float32 CUDA [n, K, 3] in frame pixels (`infer_boxes`' out); `box_scores`: float32 CUDA [n], any
        element stride (column 4 of a detector's [n, 6] tensor passes as the view it is); `crop_params`: int32 CUDA [n, 9]; `status`: int32 CUDA [n] or None.
        Returns (score float32 [n], rank int32 [n], count int32 [n_frames]): keep the rows with `rank >= 0`."""
        import torch
        dev = torch.device('cuda', self.device_id)
        check_tensor('keypoints', keypoints, torch.float32, ('n', 'K', 3), dev, True)
        n, K = keypoints.shape[0], keypoints.shape[1]
        check_tensor('box_scores', box_scores, torch.float32, (n,), dev, True, contiguous=False)
        check_tensor('crop_params', crop_params, torch.int32, (n, 9), dev, True)
        check_tensor('status', status, torch.int32, (n,), dev)
        c, keep = nms_c_config(cfg, self._nms_sigmas(cfg, K))
        score = torch.empty((n,), dtype=torch.float32, device=dev)
        rank = torch.empty((n,), dtype=torch.int32, device=dev)
        count = torch.empty((max(int(n_frames), 0),), dtype=torch.int32, device=dev)
        cs = stream_of(dev)
        capi.check(self.lib.vp_pose_nms_stream(self._h, keypoints.data_ptr(), n, K, box_scores.data_ptr(), box_scores.stride(0) if n > 1 else 1,
                                               crop_params.data_ptr(), None if status is None else status.data_ptr(), int(n_frames), C.byref(c),
                                               score.data_ptr(), rank.data_ptr(), count.data_ptr(), cs), self._h)
        return score, rank, count

    def pose_nms_host(self, keypoints, box_scores, crop_params, n_frames: int, cfg: PoseNms, status=None):
        """`pose_nms` on numpy arrays (vp_pose_nms: upload, the same kernel, download, synchronous)."""
        kp = np.ascontiguousarray(keypoints, dtype=np.float32)
        if kp.ndim != 3 or kp.shape[2] != 3:
            raise ValueError(f'keypoints: [n, K, 3] expected, got {kp.shape}')
        n, K = kp.shape[0], kp.shape[1]
        bs = np.ascontiguousarray(box_scores, dtype=np.float32)
        p9 = np.ascontiguousarray(crop_params, dtype=np.int32)
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        if bs.shape != (n,) or p9.shape != (n, 9) or (st is not None and st.shape != (n,)):
            raise ValueError(f'box_scores [{n}], crop_params [{n}, 9] and status [{n}] expected')
        c, keep = nms_c_config(cfg, self._nms_sigmas(cfg, K))
        score, rank, count = np.empty(n, np.float32), np.empty(n, np.int32), np.empty(max(int(n_frames), 0), np.int32)
        capi.check(self.lib.vp_pose_nms(self._h, kp.ctypes.data, n, K, bs.ctypes.data, 1, p9.ctypes.data, None if st is None else st.ctypes.data,
                                        int(n_frames), C.byref(c), score.ctypes.data, rank.ctypes.data, count.ctypes.data), self._h)
        return score, rank, count

    def tracker(self, cfg=None):
        """A box tracker on this handle's device (devtracker.DeviceTracker over vp_tracker_*): the stream-ordered stage in front of `infer_boxes`."""
        from .devtracker import DeviceTracker, TrackCfg
        return DeviceTracker(self, TrackCfg() if cfg is None else cfg)

    def detector(self, cfg=None):
        """A detector stage on this handle's device (devdetect.DeviceDetector over vp_detect_*): a detector's raw head to box rows, the stream-ordered stage in
        front of `tracker().update(rows, image, n_dets=count[-1:])`."""
        from .devdetect import DetectCfg, DeviceDetector
        return DeviceDetector(self, DetectCfg() if cfg is None else cfg)

    def letterbox(self, cfg=None):
        """A letterbox stage on this handle's device (devletterbox.DeviceLetterbox over vp_letterbox_*): device frames to the detector's input tensor, the
        stream-ordered stage in front of the detector network; its table goes to `detector().detect(pred, table)`."""
        from .devletterbox import DeviceLetterbox, LetterboxCfg
        return DeviceLetterbox(self, LetterboxCfg() if cfg is None else cfg)

    def yolo(self, state, in_hw=(640, 640), **kw):
        """The detector network on this handle's device (devyolo.DeviceYolo over vp_yolo_*): YOLOv8-detect from a state dict (or a path `load_yolo_state` reads),
        the stream-ordered stage between `letterbox()` and `detector()`.  `kw`: max_images, input_layout, head_dtype, head_layout."""
        from .devyolo import DeviceYolo
        return DeviceYolo(self, state, in_hw, **kw)

    def orient(self):
        """An orient stage on this handle's device (devorient.DeviceOrient over vp_orient_*): device frames as captured -- rotated, mirrored -- to upright device
        frames, the stream-ordered stage in front of `letterbox()` and of every entry that reads a frame."""
        from .devorient import DeviceOrient
        return DeviceOrient(self)

    def smoother(self, cfg=None):
        """A keypoint smoother for this handle's K joints on its device (devsmooth.DeviceSmoother over vp_smooth_*): the stream-ordered One-Euro stage behind
        `infer_boxes` (and its NMS), keyed by the tracker's (stream, id), in front of `draw_poses`."""
        from .devsmooth import DeviceSmoother, SmoothCfg
        return DeviceSmoother(self, self.K, SmoothCfg() if cfg is None else cfg)

    def metrics(self, cfg=None):
        """An accuracy evaluator on this handle's device (devmetrics.DeviceMetrics over vp_metrics_*): PCK / AUC / EPE / NME / OKS recall of predicted rows
        against ground-truth rows that lie on the GPU, accumulated stream-ordered without a host synchronisation and read once at the end (`result()`)."""
        from .devmetrics import DeviceMetrics, MetricsCfg
        return DeviceMetrics(self, MetricsCfg(n_joints=self.K) if cfg is None else cfg)

    def cocoeval(self, cfg=None):
        """A COCO keypoint AP / AR evaluator on this handle's device (devcoco.DeviceCocoEval over vp_cocoeval_*): `update` matches the detections of a batch of
        images against their ground truth where both lie on the GPU and appends one record per kept detection, `accumulate` sorts the records into the precision /
        recall tables, `result()` reads them once and gives the ten figures of COCOeval's summarize."""
        from .devcoco import CocoEvalCfg, DeviceCocoEval
        return DeviceCocoEval(self, CocoEvalCfg(n_joints=self.K) if cfg is None else cfg)

    # ------------------------------------------------------------ packed result
    def collect(self, kpts, ids=None, frame=None, rank=None, status=None, score=None, crop_params=None, n_frames: int = 1, max_records=None, out=None):
        """The kept persons of a call packed into one dense record table on the device (vp_collect_stream, contract in include/vitpose_hip.h and
        csrc/collectgeom.h), stream-ordered on torch's current stream without a host synchronisation: the stage behind `infer_boxes`, `pose_nms` and
        `smoother().update`.  `kpts`: float32 CUDA [n, K, 3]; `ids`, `frame`, `rank`, `status`: int32 CUDA [n] or None; `score`: float32 CUDA [n] with any
        positive element stride, such as the column view `rows[:, 4]`, or None; `crop_params`: int32 CUDA [n, 9] or None; `max_records`: None = n.  Returns the
        uint8 device table (`out`, or a new tensor): one copy to the host, then `devcollect.parse_records`."""
        from .devcollect import collect_device
        return collect_device(self, kpts, ids, frame, rank, status, score, crop_params, n_frames, max_records, out)

    def collect_host(self, kpts, ids=None, frame=None, rank=None, status=None, score=None, crop_params=None, n_frames: int = 1, max_records=None, out=None):
        """`collect` on numpy arrays (vp_collect: upload, the same kernels, download, synchronous).  Returns the uint8 table."""
        from .devcollect import collect_host
        return collect_host(self, kpts, ids, frame, rank, status, score, crop_params, n_frames, max_records, out)

    # ------------------------------------------------------------ skeleton overlay
    def _draw_skeleton(self, style: DrawStyle, K: int) -> np.ndarray:
        """the limb table of a call.  The handle of a plain checkpoint does not know its dataset: its 17 joints are taken as COCO's when `style.skeleton` is None
        (VitInference, which knows the dataset, resolves it first)."""
        if not isinstance(style, DrawStyle):
            raise TypeError(f'a DrawStyle expected, got {type(style).__name__}')
        return resolve_skeleton(getattr(self, 'dataset', 'coco') if self._moe else 'coco', K, style.skeleton)

    def draw_labels(self, frames, boxes, frame_index, style: LabelStyle = LabelStyle(), rank=None, ids=None, scores=None):
        """Track-id / score tags written onto device frames IN PLACE (vp_draw_labels_stream, contract in include/vitpose_hip.h and csrc/labelgeom.h), stream-ordered
        on torch's current stream without a host synchronisation: the stage in front of `draw_poses`.  `frames`: what `draw_poses` takes; `boxes`: float32 CUDA
        [n, >= 4] with unit column stride -- the tracker's rows pass as they are; `frame_index`: int32 CUDA [n] with any positive element stride; `rank` / `ids`:
        int32 CUDA [n] or None; `scores`: float32 CUDA [n] with any positive element stride, such as the column view `rows[:, 4]`, or None (the id alone).
        Returns the frames as `Frame` objects."""
        import torch
        dev = torch.device('cuda', self.device_id)
        if boxes is None:
            label_boxes(boxes)
        _check_boxes(boxes, dev, 'n')
        n = boxes.shape[0]
        if n > LABEL_MAX_ROWS:
            raise ValueError(f'labels: {n} rows exceed the {LABEL_MAX_ROWS} records of one call')
        check_tensor('frame_index', frame_index, torch.int32, (n,), dev, True, contiguous=False)
        check_tensor('rank', rank, torch.int32, (n,), dev)
        check_tensor('ids', ids, torch.int32, (n,), dev)
        check_tensor('scores', scores, torch.float32, (n,), dev, contiguous=False)
        c, keep = label_c_config(style)
        frames = [self._as_frame(f, i) for i, f in enumerate(frames)]
        table = self._image_table(frames, device_only=True)
        cs = stream_of(dev)
        capi.check(self.lib.vp_draw_labels_stream(self._h, table, len(frames), boxes.data_ptr(), 4 if n < 2 else boxes.stride(0), n, frame_index.data_ptr(),
                                                  frame_index.stride(0) if n > 1 else 1, None if rank is None else rank.data_ptr(),
                                                  None if ids is None else ids.data_ptr(), None if scores is None else scores.data_ptr(),
                                                  1 if scores is None or n < 2 else scores.stride(0), C.byref(c), cs), self._h)
        return frames

    def draw_labels_host(self, frames, boxes, frame_index, style: LabelStyle = LabelStyle(), rank=None, ids=None, scores=None):
        """`draw_labels` on numpy arrays and host frames, in place (vp_draw_labels: upload, the same kernels, download, synchronous).  Returns the frames as `Frame`s."""
        c, keep = label_c_config(style)
        frames = [host_draw_frame(f, i) for i, f in enumerate(frames)]
        bx, fi, rk, pid, sc = check_label_rows(boxes, frame_index, rank, ids, scores)
        capi.check(self.lib.vp_draw_labels(self._h, self._image_table(frames), len(frames), bx.ctypes.data, 4, bx.shape[0], fi.ctypes.data, 1,
                                           None if rk is None else rk.ctypes.data, None if pid is None else pid.ctypes.data,
                                           None if sc is None else sc.ctypes.data, 1, C.byref(c)), self._h)
        return frames

    def draw_poses(self, frames, keypoints, frame_index, style: DrawStyle = DrawStyle(), rank=None, ids=None, boxes=None, labels=None, scores=None):
        """Skeletons drawn onto device frames IN PLACE (vp_draw_poses_stream, contract in include/vitpose_hip.h), stream-ordered on torch's current stream without a
        host synchronisation: correct directly behind `infer_boxes` and `pose_nms`.  `frames`: what `infer_boxes` takes (uint8 CUDA tensors [H, W, 3] = RGB, or
        `Frame.rgb / bgr / nv12` over device planes, up to 8192 x 8192); `keypoints`: float32 CUDA [n, K, 3] in frame pixels; `frame_index`: int32 CUDA [n], or
        a column view such as `crop_params[:, 0]` (any positive element stride); `rank`: int32 CUDA [n] or None, rows with rank < 0 are not drawn; `ids`: int32
        CUDA [n] or None (the row index), the colour of a person's limbs; `boxes`: float32 CUDA [n, >= 4] with unit column stride or None, outlines drawn under the
        skeletons; `labels`: a `LabelStyle` enqueues `draw_labels` first (tags under the skeletons, in the limb palette of `style` unless it has colours of its
        own; needs `boxes`), `scores` its scores; None (the default) draws no tag.  Returns the frames as `Frame` objects."""
        import torch
        dev = torch.device('cuda', self.device_id)
        check_tensor('keypoints', keypoints, torch.float32, ('n', 'K', 3), dev, True)
        n, K = keypoints.shape[0], keypoints.shape[1]
        check_tensor('frame_index', frame_index, torch.int32, (n,), dev, True, contiguous=False)
        check_tensor('rank', rank, torch.int32, (n,), dev)
        check_tensor('ids', ids, torch.int32, (n,), dev)
        if boxes is not None:
            _check_boxes(boxes, dev, n)
        c, keep = draw_c_config(style, self._draw_skeleton(style, K))
        check_records(n, K, keep[0].shape[0], boxes is not None)
        frames = [self._as_frame(f, i) for i, f in enumerate(frames)]
        table = self._image_table(frames, device_only=True)
        if labels is not None:   # the tags first, the skeletons over them: the reference's order
            self.draw_labels(frames, label_boxes(boxes), frame_index, overlay_label_style(labels, style), rank=rank, ids=ids, scores=scores)
        cs = stream_of(dev)
        capi.check(self.lib.vp_draw_poses_stream(self._h, table, len(frames), keypoints.data_ptr(), n, K, frame_index.data_ptr(), frame_index.stride(0) if n > 1 else 1,
                                                 None if rank is None else rank.data_ptr(), None if ids is None else ids.data_ptr(),
                                                 None if boxes is None else boxes.data_ptr(), 4 if boxes is None or n < 2 else boxes.stride(0), C.byref(c), cs), self._h)
        return frames

    def draw_poses_host(self, frames, keypoints, frame_index, style: DrawStyle = DrawStyle(), rank=None, ids=None, boxes=None, labels=None, scores=None):
        """`draw_poses` on numpy arrays and host frames, in place (vp_draw_poses: upload, the same kernels, download, synchronous).  Returns the frames as `Frame`s.
        `labels`: a `LabelStyle` runs `draw_labels_host` first."""
        frames = [host_draw_frame(f, i) for i, f in enumerate(frames)]
        kp, fi, rk, pid, bx = check_rows(keypoints, frame_index, rank, ids, boxes)
        c, keep = draw_c_config(style, self._draw_skeleton(style, kp.shape[1]))
        check_records(kp.shape[0], kp.shape[1], keep[0].shape[0], bx is not None)
        if labels is not None:
            self.draw_labels_host(frames, label_boxes(bx), fi, overlay_label_style(labels, style), rank=rk, ids=pid, scores=scores)
        capi.check(self.lib.vp_draw_poses(self._h, self._image_table(frames), len(frames), kp.ctypes.data, kp.shape[0], kp.shape[1], fi.ctypes.data, 1,
                                          None if rk is None else rk.ctypes.data, None if pid is None else pid.ctypes.data,
                                          None if bx is None else bx.ctypes.data, 4, C.byref(c)), self._h)
        return frames

    def heatmaps(self, crops: np.ndarray) -> np.ndarray:
        crops = np.ascontiguousarray(crops)
        n = crops.shape[0]
        out = np.empty((n, self.K, HM_H, HM_W), dtype=np.float32)
        capi.check(self.lib.vp_infer_heatmaps(self._h, crops.ctypes.data, self._fmt(crops), n, out.ctypes.data), self._h)
        return out

    def tokens(self, crops: np.ndarray) -> np.ndarray:
        crops = np.ascontiguousarray(crops)
        n = crops.shape[0]
        out = np.empty((n, 192, self.shape.embed_dim), dtype=np.float32)
        capi.check(self.lib.vp_infer_tokens(self._h, crops.ctypes.data, self._fmt(crops), n, out.ctypes.data), self._h)
        return out

    # ------------------------------------------------------------ profiling
    def set_profiling(self, families=True):
        """True/False = all/none, or an iterable of family names from ``_capi.VP_PROF_NAMES``."""
        if families is True:
            mask = -1
        elif not families:
            mask = 0
        else:
            mask = 0
            for f in families:
                mask |= 1 << capi.VP_PROF_NAMES.index(f)
        capi.check(self.lib.vp_set_profiling(self._h, mask), self._h)

    def reset_profile(self):
        capi.check(self.lib.vp_reset_profile(self._h), self._h)

    def profile(self) -> dict:
        p = capi.vp_profile()
        capi.check(self.lib.vp_get_profile(self._h, C.byref(p)), self._h)
        return {name: dict(ms=p.ms[i], flops=p.flops[i], bytes=p.bytes[i], launches=p.launches[i])
                for i, name in enumerate(capi.VP_PROF_NAMES)}

    def profile_kernel(self, family: str) -> str:
        """Name of the kernel the last launch of `family` ran on, as the library's launch code recorded it (vp_profile_kernel)."""
        buf = C.create_string_buffer(256)
        capi.check(self.lib.vp_profile_kernel(self._h, capi.VP_PROF_NAMES.index(family), buf, len(buf)), self._h)
        return buf.value.decode('utf-8', 'replace')

    def synchronize(self):
        capi.check(self.lib.vp_synchronize(self._h), self._h)

    def close(self):
        if getattr(self, '_h', None):
            self.lib.vp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_heatmaps(heatmaps: np.ndarray, org_wh=None, device_id: int = 0) -> np.ndarray:
    """GPU decode of host heatmaps [N,K,64,48] -> [N,K,3] (y, x, conf) (vp_decode_only)."""
    lib = capi.load_library()
    hm = np.ascontiguousarray(heatmaps, dtype=np.float32)
    n, k, h, w = hm.shape
    assert (h, w) == (HM_H, HM_W)
    out = np.empty((n, k, 3), dtype=np.float32)
    wh = None if org_wh is None else np.ascontiguousarray(org_wh, dtype=np.int32).reshape(n, 2)
    capi.check(lib.vp_decode_only(device_id, hm.ctypes.data, n, k, None if wh is None else wh.ctypes.data, out.ctypes.data))
    return out


def decode_flip_heatmaps(heatmaps2: np.ndarray, pairs, shift_heatmap: bool = False, org_wh=None, device_id: int = 0) -> np.ndarray:
    """The flip-test mode's fused decode alone (vp_dbg_decode_flip): host heatmaps [2 N, K, 64, 48], crop i's maps at 2 i and its mirror
    image's at 2 i + 1 -> [N, K, 3] of their flip-test average, which is never formed."""
    lib = capi.load_library()
    hm = np.ascontiguousarray(heatmaps2, dtype=np.float32)
    n2, k, h, w = hm.shape
    assert (h, w) == (HM_H, HM_W) and n2 % 2 == 0
    pairs = _flip_pairs_array(pairs)
    out = np.empty((n2 // 2, k, 3), dtype=np.float32)
    wh = None if org_wh is None else np.ascontiguousarray(org_wh, dtype=np.int32).reshape(n2 // 2, 2)
    capi.check(lib.vp_dbg_decode_flip(device_id, hm.ctypes.data, n2 // 2, k, pairs.ctypes.data if len(pairs) else None, len(pairs),
                                      int(bool(shift_heatmap)), None if wh is None else wh.ctypes.data, out.ctypes.data))
    return out


def box_cs_host(boxes, frame_index=None, n_frames: int = 1, box_scale: float = 1.25):
    """What the box kernel of the affine boxes entry computes, on the host (vp_dbg_box_cs: csrc/affinegeom.h itself; no device needed): float32 boxes
    [n, >= 4] -> (cs float32 [n, 4], status int32 [n])."""
    lib = capi.load_library()
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    assert b.ndim == 2 and b.shape[1] >= 4
    fi = None if frame_index is None else np.ascontiguousarray(frame_index, dtype=np.int32)
    cs = np.empty((len(b), 4), dtype=np.float32)
    st = np.empty((len(b),), dtype=np.int32)
    capi.check(lib.vp_dbg_box_cs(b.ctypes.data, b.shape[1], None if fi is None else fi.ctypes.data, int(n_frames), len(b), float(box_scale),
                                 cs.ctypes.data, st.ctypes.data))
    return cs, st


def _host_image(frame: Frame):
    if frame.on_device:
        raise TypeError('a frame whose planes are on the host expected')
    p0, p1 = frame.pointers()
    return capi.vp_image((C.c_void_p * 2)(p0, p1), (C.c_int64 * 2)(*frame.pitch), frame.h, frame.w, PIX_FORMATS[frame.format], YUV_MATRIX_IDS[frame.matrix])


def affine_plan_host(frames, frame_index, cs) -> np.ndarray:
    """The plan of the host-frames affine route (vp_dbg_affine_plan; no device needed): int32 [n_frames, 2] = the frame rows [row0, row1) each
    frame's crops tap, {0, 0} for a frame without any.  Raises VpError for what vp_infer_images_affine refuses."""
    lib = capi.load_library()
    frames = [VitPoseHip._as_frame(f, i) for i, f in enumerate(frames)]
    table = (capi.vp_image * max(len(frames), 1))()
    for i, f in enumerate(frames):
        table[i] = _host_image(f)
    cs = np.ascontiguousarray(cs, dtype=np.float32).reshape(-1, 4)
    fi = None if frame_index is None else np.ascontiguousarray(frame_index, dtype=np.int32)
    bands = np.zeros((len(frames), 2), dtype=np.int32)
    capi.check(lib.vp_dbg_affine_plan(table, len(frames), None if fi is None else fi.ctypes.data, cs.ctypes.data, len(cs), bands.ctypes.data))
    return bands


def crop_affine_device(frame, cs, device_id: int = 0) -> np.ndarray:
    """The device affine crop kernel alone on one host frame of any layout (vp_dbg_crop_affine): uint8 RGB [n, 256, 192, 3]."""
    lib = capi.load_library()
    frame = VitPoseHip._as_frame(frame, 0)
    cs = np.ascontiguousarray(cs, dtype=np.float32).reshape(-1, 4)
    out = np.empty((len(cs), IMG_H, IMG_W, 3), dtype=np.uint8)
    im = _host_image(frame)
    capi.check(lib.vp_dbg_crop_affine(device_id, C.byref(im), cs.ctypes.data, len(cs), out.ctypes.data))
    return out


def decode_affine_heatmaps(heatmaps: np.ndarray, cs, device_id: int = 0, flip_pairs=None, shift_heatmap: bool = False) -> np.ndarray:
    """The affine decode alone (vp_dbg_decode_affine): host heatmaps [N, K, 64, 48] and cs [N, 4] -> [N, K, 3] (y, x, conf) in frame pixels.
    `flip_pairs` given: the flip-test mode's interleaved [2 N, K, 64, 48] (vp_dbg_decode_affine_flip)."""
    lib = capi.load_library()
    hm = np.ascontiguousarray(heatmaps, dtype=np.float32)
    n, k, h, w = hm.shape
    assert (h, w) == (HM_H, HM_W)
    if flip_pairs is not None:
        assert n % 2 == 0
        n //= 2
    cs = np.ascontiguousarray(cs, dtype=np.float32).reshape(n, 4)
    out = np.empty((n, k, 3), dtype=np.float32)
    if flip_pairs is None:
        capi.check(lib.vp_dbg_decode_affine(device_id, hm.ctypes.data, n, k, cs.ctypes.data, out.ctypes.data))
    else:
        pairs = _flip_pairs_array(flip_pairs)
        capi.check(lib.vp_dbg_decode_affine_flip(device_id, hm.ctypes.data, n, k, pairs.ctypes.data if len(pairs) else None, len(pairs), int(bool(shift_heatmap)),
                                                 cs.ctypes.data, out.ctypes.data))
    return out


def crop_prep_device(frame: np.ndarray, params: np.ndarray, device_id: int = 0) -> np.ndarray:
    """The device crop/pad/resize kernel alone (vp_dbg_crop_prep): uint8 [n, 256, 192, 3]."""
    lib = capi.load_library()
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    params = np.ascontiguousarray(params, dtype=np.int32).reshape(-1, 8)
    out = np.empty((len(params), IMG_H, IMG_W, 3), dtype=np.uint8)
    capi.check(lib.vp_dbg_crop_prep(device_id, frame.ctypes.data, frame.shape[0], frame.shape[1], params.ctypes.data,
                                    len(params), out.ctypes.data))
    return out


def crop_prep_image(frame: Frame, params: np.ndarray, device_id: int = 0) -> np.ndarray:
    """The device crop/pad/resize kernel alone on one host `Frame` of any layout (vp_dbg_crop_prep_image): uint8 RGB [n, 256, 192, 3]."""
    lib = capi.load_library()
    if frame.on_device:
        raise TypeError('crop_prep_image takes a frame whose planes are on the host')
    params = np.ascontiguousarray(params, dtype=np.int32).reshape(-1, 8)
    out = np.empty((len(params), IMG_H, IMG_W, 3), dtype=np.uint8)
    p0, p1 = frame.pointers()
    im = capi.vp_image((C.c_void_p * 2)(p0, p1), (C.c_int64 * 2)(*frame.pitch), frame.h, frame.w, PIX_FORMATS[frame.format], YUV_MATRIX_IDS[frame.matrix])
    capi.check(lib.vp_dbg_crop_prep_image(device_id, C.byref(im), params.ctypes.data, len(params), out.ctypes.data))
    return out


class VitPoseGroup:
    """One process, N GPUs (vp_group_*): weights replicated, crops of a call sharded contiguously, all devices concurrent."""

    def __init__(self, shape: ModelShape, state_dict, device_ids, dtype: str = 'fp16', max_batch: int = 64):
        self.lib = capi.load_library()
        self.shape, self.K = shape, shape.num_keypoints
        self.device_ids = [int(d) for d in device_ids]
        cfg = capi.vp_config(shape.embed_dim, shape.depth, shape.num_heads, shape.num_keypoints, capi.DTYPES[dtype], 0, int(max_batch))
        ids = (C.c_int32 * len(self.device_ids))(*self.device_ids)
        g = C.c_void_p()
        code = self.lib.vp_group_create(C.byref(g), C.byref(cfg), ids, len(self.device_ids))
        if code != capi.VP_OK:
            raise capi.VpError(code, (self.lib.vp_group_last_error(None) or b'').decode('utf-8', 'replace'))
        self._g = g
        arr, keep = _tensor_descs(state_dict)
        self._check(self.lib.vp_group_load_weights(self._g, arr, len(arr)))

    def _check(self, code):
        if code != capi.VP_OK:
            raise capi.VpError(code, (self.lib.vp_group_last_error(self._g) or b'').decode('utf-8', 'replace'))

    def infer(self, crops: np.ndarray, org_wh=None) -> np.ndarray:
        crops = np.ascontiguousarray(crops)
        n = crops.shape[0]
        out = np.empty((n, self.K, 3), dtype=np.float32)
        if n == 0:
            return out
        wh = None if org_wh is None else np.ascontiguousarray(org_wh, dtype=np.int32).reshape(n, 2)
        self._check(self.lib.vp_group_infer(self._g, crops.ctypes.data, VitPoseHip._fmt(crops), n,
                                            None if wh is None else wh.ctypes.data, out.ctypes.data))
        return out

    def set_flip_test(self, pairs, shift_heatmap: bool = False):
        """The flip-test mode on every member (vp_group_set_flip_test; VitPoseHip.set_flip_test): a round then takes max_batch // 2 crops per device."""
        pairs = _flip_pairs_array(pairs)
        self._check(self.lib.vp_group_set_flip_test(self._g, pairs.ctypes.data if len(pairs) else None, len(pairs), int(bool(shift_heatmap))))

    def clear_flip_test(self):
        self._check(self.lib.vp_group_clear_flip_test(self._g))

    def infer_allgather(self, crops: np.ndarray, d_all, org_wh=None):
        """`d_all`: one torch float32 tensor [n, K, 3] per device of the group; every one receives ALL keypoints (peer copies)."""
        crops = np.ascontiguousarray(crops)
        n = crops.shape[0]
        assert len(d_all) == len(self.device_ids) and all(t.is_cuda and t.is_contiguous() and t.numel() == n * self.K * 3 for t in d_all)
        ptrs = (C.c_void_p * len(d_all))(*[t.data_ptr() for t in d_all])
        out = np.empty((n, self.K, 3), dtype=np.float32)
        wh = None if org_wh is None else np.ascontiguousarray(org_wh, dtype=np.int32).reshape(n, 2)
        self._check(self.lib.vp_group_infer_allgather(self._g, crops.ctypes.data, VitPoseHip._fmt(crops), n,
                                                      None if wh is None else wh.ctypes.data, ptrs, out.ctypes.data))
        return out

    def close(self):
        if getattr(self, '_g', None):
            self.lib.vp_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
