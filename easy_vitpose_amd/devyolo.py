"""The detector network on the device (vp_yolo_*; the network, its plan, the load step and the decode in csrc/yologeom.h): YOLOv8-detect between the letterbox
stage and the detector stage, with nothing third-party.  ``load_yolo_state`` reads a checkpoint (an ``.npz`` written by tools/export_yolo_state.py, or a plain
state dict ``.pt`` / ``.pth``), ``synth_yolo`` makes a seeded one, ``yolo_plan`` / ``yolo_fold`` / ``yolo_decode_host`` are the host-only taps (no device) and
``DeviceYolo`` is the stage: callable on the letterboxed device tensor, it carries ``.nc`` and ``.head_dtype`` and so is an engine under the ``--det-engine``
contract of the CLI.

``DeviceYolo.__call__`` is stream-ordered on torch's current stream, never synchronises and never allocates: the head it returns is a view of a tensor the
object owns, overwritten by the next call.

Against the ultralytics binary and a real checkpoint PARITY UNPINNED: neither is installed here; the network is built from the published architecture.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _capi as capi
from ._stage import DeviceStage, handle_alias

MAX_IMAGES = 64
MAX_SIDE = 1280
HEAD_DTYPES = {'fp32': 0, 'fp16': 1}
NP_HEAD = {'fp32': np.float32, 'fp16': np.float16}
LAYOUTS = {'nchw': 0, 'nhwc': 1}
SCALES = {'n': (0.33, 0.25, 1024), 's': (0.33, 0.50, 1024), 'm': (0.67, 0.75, 768), 'l': (1.0, 1.0, 512), 'x': (1.0, 1.25, 512)}
KINDS = ('pack', 'conv', 'pool', 'up', 'decode')
EXPORTER = 'tools/export_yolo_state.py'


def load_yolo_state(path) -> dict:
    """A checkpoint as {name: float32 ndarray}: an ``.npz``, or a plain state dict ``.pt`` / ``.pth`` (``torch.load(weights_only=True)``).  An ultralytics pickle
    (a whole model object) is refused: tools/export_yolo_state.py, on a machine with ultralytics, writes its state dict to ``.npz``."""
    path = os.fspath(path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f'the YOLOv8 checkpoint {path} does not exist')
    if path.endswith('.npz'):
        with np.load(path) as z:
            return {k: np.require(z[k], np.float32, 'C') for k in z.files}
    import pickle
    import torch
    try:
        sd = torch.load(path, map_location='cpu', weights_only=True)
    except (pickle.UnpicklingError, RuntimeError, AttributeError, ModuleNotFoundError) as e:
        raise ValueError(f'{path} is not a plain state dict (an ultralytics checkpoint pickles the whole model object): export it with {EXPORTER} '
                         f'on a machine that has ultralytics, and pass the .npz') from e
    if isinstance(sd, dict) and 'state_dict' in sd and isinstance(sd['state_dict'], dict):
        sd = sd['state_dict']
    if not (isinstance(sd, dict) and sd and all(isinstance(k, str) and isinstance(v, torch.Tensor) for k, v in sd.items())):
        raise ValueError(f'{path} is not a plain state dict of tensors: export an ultralytics checkpoint with {EXPORTER} and pass the .npz')
    return {k: np.require(v.detach().to(torch.float32).numpy(), np.float32, 'C') for k, v in sd.items() if v.is_floating_point()}


def synth_yolo(scale: str = 'n', nc: int = 80, seed: int = 0) -> dict:
    """A seeded YOLOv8-detect state dict of `scale` (ultralytics' keys, unfused): He-scaled convolutions, BatchNorm statistics away from (0, 1) (a Bottleneck's second one at half gain), Detect's box
    biases at 1 and class biases at ultralytics' log(5 / nc / (640 / stride)^2), so that few anchors score high."""
    if scale not in SCALES:
        raise ValueError(f"synth_yolo: scale 'n', 's', 'm', 'l' or 'x' expected, got {scale!r}")
    if not 1 <= int(nc) <= 256:
        raise ValueError(f'synth_yolo: nc in 1..256 expected, got {nc!r}')
    depth, width, max_ch = SCALES[scale]
    rng = np.random.default_rng(seed)
    ch = lambda x: 8 * math.ceil(min(x, max_ch) * width / 8)   # noqa: E731
    d = lambda n: max(round(n * depth), 1)                      # noqa: E731
    sd = {}

    def conv(key, c1, c2, k, gain=1.0):
        sd[key + '.conv.weight'] = (rng.standard_normal((c2, c1, k, k)) * math.sqrt(2.0 / (c1 * k * k))).astype(np.float32)
        sd[key + '.bn.weight'] = (rng.uniform(0.7, 1.4, c2) * gain).astype(np.float32)
        sd[key + '.bn.bias'] = (rng.standard_normal(c2) * 0.2).astype(np.float32)
        sd[key + '.bn.running_mean'] = (rng.standard_normal(c2) * 0.3).astype(np.float32)
        sd[key + '.bn.running_var'] = rng.uniform(0.4, 1.8, c2).astype(np.float32)
        sd[key + '.bn.num_batches_tracked'] = np.asarray(1000.0, np.float32)

    def c2f(i, c1, c2, n):
        c = c2 // 2
        conv(f'model.{i}.cv1', c1, 2 * c, 1)
        for j in range(n):
            conv(f'model.{i}.m.{j}.cv1', c, c, 3)
            conv(f'model.{i}.m.{j}.cv2', c, c, 3, gain=0.5)   # the residual branch at half gain: activations do not grow shortcut by shortcut and the head does not saturate
        conv(f'model.{i}.cv2', (2 + n) * c, c2, 1)

    c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
    conv('model.0', 3, c64, 3)
    conv('model.1', c64, c128, 3)
    c2f(2, c128, c128, d(3))
    conv('model.3', c128, c256, 3)
    c2f(4, c256, c256, d(6))
    conv('model.5', c256, c512, 3)
    c2f(6, c512, c512, d(6))
    conv('model.7', c512, c1024, 3)
    c2f(8, c1024, c1024, d(3))
    conv('model.9.cv1', c1024, c1024 // 2, 1)
    conv('model.9.cv2', 2 * c1024, c1024, 1)
    c2f(12, c1024 + c512, c512, d(3))
    c2f(15, c512 + c256, c256, d(3))
    conv('model.16', c256, c256, 3)
    c2f(18, c256 + c512, c512, d(3))
    conv('model.19', c512, c512, 3)
    c2f(21, c512 + c1024, c1024, d(3))
    c2, c3 = max(16, c256 // 4, 64), max(c256, min(nc, 100))
    for lvl, (x, stride) in enumerate(((c256, 8), (c512, 16), (c1024, 32))):
        for br, cm, co in (('cv2', c2, 64), ('cv3', c3, nc)):
            conv(f'model.22.{br}.{lvl}.0', x, cm, 3)
            conv(f'model.22.{br}.{lvl}.1', cm, cm, 3)
            gain = 0.5 if br == 'cv2' else 1.0   # box logits of moderate spread: distances around the middle of the 16 bins
            sd[f'model.22.{br}.{lvl}.2.weight'] = (rng.standard_normal((co, cm, 1, 1)) * gain * math.sqrt(2.0 / cm)).astype(np.float32)
            bias = np.full(co, 1.0) if br == 'cv2' else np.full(co, math.log(5 / nc / (640 / stride) ** 2))
            sd[f'model.22.{br}.{lvl}.2.bias'] = bias.astype(np.float32)
    sd['model.22.dfl.conv.weight'] = np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)
    return sd


def _tensor_table(state: dict):
    """the vp_yolo_tensor table of a state dict (every `model.` entry as contiguous float32) and what keeps its memory alive"""
    if not isinstance(state, dict) or not state:
        raise TypeError('a state dict {name: array} expected')
    keep, rows = [], []
    for name, v in state.items():
        if not (isinstance(name, str) and name.startswith('model.')) or name.endswith('num_batches_tracked'):
            continue   # unknown keys outside `model.` and the BatchNorm counters are ignored
        if hasattr(v, 'detach'):
            v = v.detach().cpu().float().numpy()
        a = np.ascontiguousarray(v, dtype=np.float32)
        if a.ndim > 4:
            raise ValueError(f'{name}: a tensor of at most 4 dimensions expected, got shape {a.shape}')
        keep.append((name.encode(), a))
        rows.append(a)
    tab = (capi.vp_yolo_tensor * max(len(rows), 1))()
    for i, (nm, a) in enumerate(keep):
        shape = (C.c_int32 * 4)(*(list(a.shape) + [0] * (4 - a.ndim)))
        tab[i] = capi.vp_yolo_tensor(nm, a.ctypes.data_as(C.POINTER(C.c_float)), a.size, a.ndim, shape, 0)
    return tab, len(keep), keep


def _c_cfg(in_hw, max_images=1, input_layout='nchw', head_dtype='fp32', head_layout=0, keep_activations=False):
    if isinstance(in_hw, (int, np.integer)):
        in_hw = (in_hw, in_hw)
    h, w = (int(v) for v in in_hw)
    if input_layout not in LAYOUTS:
        raise ValueError(f"input_layout 'nchw' or 'nhwc' expected, got {input_layout!r}")
    if head_dtype not in HEAD_DTYPES:
        raise ValueError(f"head_dtype 'fp32' or 'fp16' expected, got {head_dtype!r}")
    return capi.vp_yolo_cfg(h, w, int(max_images), LAYOUTS[input_layout], HEAD_DTYPES[head_dtype], int(head_layout), (C.c_int32 * 2)(int(bool(keep_activations)), 0))


INFO_FIELDS = ('n_launches', 'n_buffers', 'n_convs', 'nc', 'A', 'scale', 'ch64', 'ch128', 'ch256', 'ch512', 'ch1024', 'd3', 'd6', 'det_c2', 'det_c3')


def yolo_plan(state: dict, in_hw, **cfg):
    """HOST ONLY (vp_dbg_yolo_plan): (info dict, launches as a list of dicts, buffers as a list of dicts) of the checkpoint at `in_hw`."""
    lib = capi.load_library()
    c = _c_cfg(in_hw, **cfg)
    tab, n, keep = _tensor_table(state)
    info = np.zeros(16, np.int32)
    capi.check(lib.vp_dbg_yolo_plan(C.byref(c), tab, n, None, 0, None, 0, info.ctypes.data))
    launches, bufs = (capi.vp_yolo_launch * int(info[0]))(), (capi.vp_yolo_buffer * int(info[1]))()
    capi.check(lib.vp_dbg_yolo_plan(C.byref(c), tab, n, launches, len(launches), bufs, len(bufs), info.ctypes.data))
    out = {k: int(v) for k, v in zip(INFO_FIELDS, info)}
    out['scale'] = chr(out['scale'])
    fields = [f for f, _ in capi.vp_yolo_launch._fields_ if f != 'reserved']
    ls = [{f: int(getattr(l, f)) for f in fields} for l in launches]
    for l in ls:
        l['kind'] = KINDS[l['kind']]
    return out, ls, [{'h': b.h, 'w': b.w, 'c': b.c, 'elem_bytes': b.elem_bytes} for b in bufs]


def yolo_fold(state: dict, in_hw, conv: int):
    """HOST ONLY (vp_dbg_yolo_fold): (w float16 [rows, cols] with cols = (ky, kx, channel padded to 8), b float32 [rows]) of convolution `conv` of the plan."""
    lib = capi.load_library()
    c = _c_cfg(in_hw)
    tab, n, keep = _tensor_table(state)
    dims = np.zeros(2, np.int32)
    capi.check(lib.vp_dbg_yolo_fold(C.byref(c), tab, n, int(conv), None, None, dims.ctypes.data))
    w, b = np.empty((int(dims[0]), int(dims[1])), np.uint16), np.empty(int(dims[0]), np.float32)
    capi.check(lib.vp_dbg_yolo_fold(C.byref(c), tab, n, int(conv), w.ctypes.data, b.ctypes.data, dims.ctypes.data))
    return w.view(np.float16), b


def yolo_decode_host(levels, nc: int, in_hw, head_dtype='fp32', head_layout=0):
    """HOST ONLY (vp_dbg_yolo_decode_host): `levels` = the three float32 [n, h_l, w_l, 64 + nc] Detect outputs (P3, P4, P5) to the head."""
    lib = capi.load_library()
    h, w = (int(v) for v in in_hw)
    levels = [np.ascontiguousarray(l, dtype=np.float32) for l in levels]
    n = int(levels[0].shape[0])
    for i, l in enumerate(levels):
        if l.shape != (n, h >> (3 + i), w >> (3 + i), 64 + nc):
            raise ValueError(f'level {i}: [{n}, {h >> (3 + i)}, {w >> (3 + i)}, {64 + nc}] expected, got {l.shape}')
    A = sum(l.shape[1] * l.shape[2] for l in levels)
    flat = np.concatenate([l.ravel() for l in levels])
    head = np.empty((n, 4 + nc, A) if head_layout == 0 else (n, A, 4 + nc), NP_HEAD[head_dtype])
    capi.check(lib.vp_dbg_yolo_decode_host(int(nc), h, w, n, flat.ctypes.data, HEAD_DTYPES[head_dtype], int(head_layout), head.ctypes.data))
    return head


class DeviceYolo(DeviceStage):
    """YOLOv8-detect on the engine's device.  ``state``: a state dict, or a path `load_yolo_state` reads.  ``in_hw``: the input size, multiples of 32.
    Callable on the letterboxed device tensor (fp16, [n, 3, H, W] under input_layout 'nchw', [n, H, W, 3] under 'nhwc', RGB, values / 255; n <= max_images):
    returns the head [n, 4 + nc, A] (head_layout 0) or [n, A, 4 + nc] of ``head_dtype``, a view of a device tensor this object owns.  ``keep_activations``
    (tests): every internal buffer in a region of its own, which `activation` needs; otherwise the regions are reused along the forward."""

    _destroy, _y = 'vp_yolo_destroy', handle_alias

    def __init__(self, engine, state, in_hw=(640, 640), max_images: int = 1, input_layout: str = 'nchw', head_dtype: str = 'fp32', head_layout: int = 0,
                 keep_activations: bool = False):
        import torch
        super().__init__(engine)
        if isinstance(state, (str, os.PathLike)):
            state = load_yolo_state(state)
        self._c = _c_cfg(in_hw, max_images, input_layout, head_dtype, head_layout, keep_activations)
        self.in_hw, self.max_images, self.input_layout, self.head_dtype, self.head_layout = (self._c.in_h, self._c.in_w), int(max_images), input_layout, head_dtype, int(head_layout)
        tab, n, keep = _tensor_table(state)
        self._create(self.lib.vp_yolo_create, C.byref(self._c), tab, n)
        nc, A, nl, nb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self.lib.vp_yolo_info(self._obj, C.byref(nc), C.byref(A), C.byref(nl), C.byref(nb)))
        self.nc, self.A, self.n_launches, self.device_bytes = nc.value, A.value, nl.value, nb.value
        shape = (self.max_images, 4 + self.nc, self.A) if self.head_layout == 0 else (self.max_images, self.A, 4 + self.nc)
        self._head = torch.zeros(shape, dtype=torch.float16 if head_dtype == 'fp16' else torch.float32, device=self._dev)

    def input_shape(self, n: int):
        h, w = self.in_hw
        return (n, 3, h, w) if self.input_layout == 'nchw' else (n, h, w, 3)

    def __call__(self, x):
        import torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float16):
            raise TypeError('DeviceYolo: an fp16 torch CUDA tensor expected (the letterbox stage\'s fp16 output)')
        if x.device != self._dev or not x.is_contiguous():
            raise ValueError(f'DeviceYolo: a contiguous tensor on {self._dev} expected')
        n = int(x.shape[0]) if x.dim() == 4 else -1
        if n < 0 or n > self.max_images or tuple(x.shape) != self.input_shape(n):
            raise ValueError(f'DeviceYolo: {self.input_shape("n")} with n <= {self.max_images} expected, got {tuple(x.shape)}')
        self._check(self.lib.vp_yolo_forward_stream(self._obj, x.data_ptr() if n else None, n, self._head.data_ptr() if n else None, self._stream()))
        return self._head[:n]

    def forward_host(self, x: np.ndarray) -> np.ndarray:
        """`__call__` on a numpy array (vp_yolo_forward: upload, the same kernels, download, synchronous)."""
        x = np.ascontiguousarray(x)
        n = int(x.shape[0])
        if x.dtype != np.float16 or tuple(x.shape) != self.input_shape(n):
            raise ValueError(f'DeviceYolo: float16 {self.input_shape("n")} expected, got {x.dtype} {x.shape}')
        shape = (n, 4 + self.nc, self.A) if self.head_layout == 0 else (n, self.A, 4 + self.nc)
        head = np.empty(shape, NP_HEAD[self.head_dtype])
        self._check(self.lib.vp_yolo_forward(self._obj, x.ctypes.data if n else None, n, head.ctypes.data if n else None))
        return head

    def activation(self, launch: int, n_images: int, buffer: dict) -> np.ndarray:
        """After a forward of n_images: the whole buffer launch `launch` of the plan wrote into ([n, h, w, c]; `buffer` = its row of `yolo_plan`)."""
        out = np.empty((n_images, buffer['h'], buffer['w'], buffer['c']), np.float16 if buffer['elem_bytes'] == 2 else np.float32)
        self._check(self.lib.vp_dbg_yolo_activation(self._obj, int(launch), int(n_images), out.ctypes.data))
        return out
