"""The oracle of the detector network (tests/test_yolo_host.py, tests/test_gpu_yolo.py): YOLOv8-detect, eval mode, restated with torch.nn.functional on the CPU in
float64 from the state dict alone, with its own BatchNorm fold.  It shares no code with the package: channel and repeat counts are read off the state dict's
shapes and keys, the layers are the published architecture.

Modes: 'exact' keeps every activation in float64; 'stored' rounds every Conv-module output (after SiLU and after a shortcut add: once, where the device stores)
to fp16, the six float32 Detect outputs to float32.  `perturb` (a seed) rounds each stored fp16 value up or down at random instead of to nearest: the
sensitivity of the head to the one thing the device may do differently, a float32 summation order that flips an fp16 rounding.  Weights are the folded fp16
ones and biases the folded float32 ones in every mode."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3


def fold(sd, key, module=True):
    """(w float64 [c2, c1, k, k] holding fp16 values, b float64 [c2] holding float32 values)"""
    if not module:
        w, b = np.asarray(sd[key + '.weight'], np.float64), np.asarray(sd[key + '.bias'], np.float32)
        return w.astype(np.float16).astype(np.float64), b.astype(np.float64)
    w = np.asarray(sd[key + '.conv.weight'], np.float64)
    if key + '.bn.weight' in sd:
        g, be = np.asarray(sd[key + '.bn.weight'], np.float64), np.asarray(sd[key + '.bn.bias'], np.float64)
        mu, var = np.asarray(sd[key + '.bn.running_mean'], np.float64), np.asarray(sd[key + '.bn.running_var'], np.float64)
        scale = g / np.sqrt(var + EPS)
        w = w * scale[:, None, None, None]
        b = be - mu * scale
    else:
        b = np.asarray(sd[key + '.conv.bias'], np.float64)
    return w.astype(np.float16).astype(np.float64), b.astype(np.float32).astype(np.float64)


def fold_image(sd, key, module, c_in_pad, rows):
    """the fold as the library lays it out: w float16 [rows, k k c_in_pad] in (ky, kx, channel) order, b float32 [rows]; zero beyond the checkpoint's channels"""
    w, b = fold(sd, key, module)
    c2, c1, k, _ = w.shape
    img = np.zeros((rows, k, k, c_in_pad), np.float16)
    img[:c2, :, :, :c1] = w.transpose(0, 2, 3, 1).astype(np.float16)
    bias = np.zeros(rows, np.float32)
    bias[:c2] = b
    return img.reshape(rows, -1), bias


def fuse(sd):
    """the same network as a fused checkpoint: conv.weight + conv.bias folded in float64 and stored as float32 (what a fused checkpoint holds), no bn.*"""
    out = {}
    for k, v in sd.items():
        if '.bn.' in k:
            continue
        if k.endswith('.conv.weight') and k[:-len('.conv.weight')] + '.bn.weight' in sd:
            key = k[:-len('.conv.weight')]
            g, be = np.asarray(sd[key + '.bn.weight'], np.float64), np.asarray(sd[key + '.bn.bias'], np.float64)
            mu, var = np.asarray(sd[key + '.bn.running_mean'], np.float64), np.asarray(sd[key + '.bn.running_var'], np.float64)
            scale = g / np.sqrt(var + EPS)
            out[k] = (np.asarray(v, np.float64) * scale[:, None, None, None]).astype(np.float32)
            out[key + '.conv.bias'] = (be - mu * scale).astype(np.float32)
        else:
            out[k] = v
    return out


class Net:
    def __init__(self, sd, mode='stored', perturb=None):
        assert mode in ('exact', 'stored')
        self.sd, self.mode = sd, mode
        self.rng = None if perturb is None else np.random.default_rng(perturb)
        self.convs = []   # (key, module) in the order they run

    def store(self, x):
        if self.mode == 'exact':
            return x
        v = x.numpy()
        r = v.astype(np.float16)
        if self.rng is not None:
            r64 = r.astype(np.float64)
            other = np.where(r64 > v, np.nextafter(r, np.float16(-np.inf)), np.where(r64 < v, np.nextafter(r, np.float16(np.inf)), r))
            r = np.where(self.rng.random(v.shape) < 0.5, r, other)
        return torch.from_numpy(r.astype(np.float64))

    def conv(self, x, key, k, s, res=None):
        self.convs.append((key, True))
        w, b = fold(self.sd, key)
        y = F.conv2d(x, torch.from_numpy(w), torch.from_numpy(b), stride=s, padding=k // 2)
        y = y * torch.sigmoid(y)
        if res is not None:
            y = y + res
        return self.store(y)

    def plain(self, x, key):
        self.convs.append((key, False))
        w, b = fold(self.sd, key, module=False)
        y = F.conv2d(x, torch.from_numpy(w), torch.from_numpy(b))
        return y if self.mode == 'exact' else y.to(torch.float32).to(torch.float64)

    def c2f(self, x, i, shortcut):
        key = f'model.{i}'
        y = list(self.conv(x, key + '.cv1', 1, 1).chunk(2, 1))
        j = 0
        while f'{key}.m.{j}.cv1.conv.weight' in self.sd:
            t = self.conv(y[-1], f'{key}.m.{j}.cv1', 3, 1)
            y.append(self.conv(t, f'{key}.m.{j}.cv2', 3, 1, res=y[-1] if shortcut else None))
            j += 1
        return self.conv(torch.cat(y, 1), key + '.cv2', 1, 1)

    def sppf(self, x, i):
        y = [self.conv(x, f'model.{i}.cv1', 1, 1)]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], 5, 1, 2))
        return self.conv(torch.cat(y, 1), f'model.{i}.cv2', 1, 1)

    def levels(self, x):
        """x float64 [n, 3, H, W] -> the three Detect outputs [n, 64 + nc, h, w]"""
        up = lambda t: F.interpolate(t, scale_factor=2, mode='nearest')   # noqa: E731
        x = self.conv(x, 'model.0', 3, 2)
        x = self.conv(x, 'model.1', 3, 2)
        x = self.c2f(x, 2, True)
        x = self.conv(x, 'model.3', 3, 2)
        x4 = self.c2f(x, 4, True)
        x = self.conv(x4, 'model.5', 3, 2)
        x6 = self.c2f(x, 6, True)
        x = self.conv(x6, 'model.7', 3, 2)
        x = self.c2f(x, 8, True)
        x9 = self.sppf(x, 9)
        x12 = self.c2f(torch.cat([up(x9), x6], 1), 12, False)
        x15 = self.c2f(torch.cat([up(x12), x4], 1), 15, False)
        x18 = self.c2f(torch.cat([self.conv(x15, 'model.16', 3, 2), x12], 1), 18, False)
        x21 = self.c2f(torch.cat([self.conv(x18, 'model.19', 3, 2), x9], 1), 21, False)
        out = []
        for l, f in enumerate((x15, x18, x21)):
            box = self.plain(self.conv(self.conv(f, f'model.22.cv2.{l}.0', 3, 1), f'model.22.cv2.{l}.1', 3, 1), f'model.22.cv2.{l}.2')
            cls = self.plain(self.conv(self.conv(f, f'model.22.cv3.{l}.0', 3, 1), f'model.22.cv3.{l}.1', 3, 1), f'model.22.cv3.{l}.2')
            out.append(torch.cat([box, cls], 1))
        return out


def decode(levels):
    """float64: the three [n, 64 + nc, h, w] Detect outputs -> the head [n, 4 + nc, A]"""
    heads = []
    for l, t in enumerate(levels):
        n, c, h, w = t.shape
        stride = 8 << l
        z = t[:, :64].reshape(n, 4, 16, h * w)
        d = (torch.softmax(z, 2) * torch.arange(16, dtype=torch.float64).view(1, 1, 16, 1)).sum(2)   # [n, 4, hw]
        gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
        ax, ay = gx.reshape(-1) + 0.5, gy.reshape(-1) + 0.5
        x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
        box = torch.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], 1) * stride
        heads.append(torch.cat([box, torch.sigmoid(t[:, 64:].reshape(n, c - 64, h * w))], 1))
    return torch.cat(heads, 2).numpy()


def forward(sd, x, mode='stored', perturb=None):
    """x: [n, 3, H, W] (fp16 values) -> the head float64 [n, 4 + nc, A]"""
    with torch.no_grad():
        return decode(Net(sd, mode, perturb).levels(torch.from_numpy(np.asarray(x, np.float64))))


def conv_order(sd):
    """(key, is a Conv module) of every convolution in the order the network runs them"""
    net = Net(sd, 'exact')
    with torch.no_grad():
        net.levels(torch.zeros(1, 3, 32, 32, dtype=torch.float64))
    return net.convs
