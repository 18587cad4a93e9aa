"""Seeded case families of the simple decoder's head on the fixed 16 x 12 token grid, shared by tests/test_simple_head_model.py (CPU) and
tests/test_gpu_simple_head.py.  A case = dict(x [B, 192, D] float32 values of the operand type, w [K, D, 3, 3], b [K]); numpy only.

    taps      per crop ONE token carries 2.0 in ONE channel; map k reads that channel through ONE tap (t = k % 9) with weight 2^-(1 + k % 3), bias k % 3 - 1: every product,
              every multiple of an interpolation weight (eighths) and every sum is exact in fp32, so the expected map is known bit for bit and a wrong tap, shift,
              ky / kx swap, border or neighbour is readable from the values.  The crops put the token in the four corners, on every edge and inside.
    edges     random content on the border tokens only (variant 'corners': the four corner tokens only): what crosses the 64 x 48 border must count as zero
    relu      negative inputs with large weights, -0.0, and (variant 'sub') nothing but the smallest subnormals of the operand type, both signs, under
              power-of-two weights that lift the positive ones into the normal fp32 range
    lo_plane  all-positive inputs under weights 2^-6 (1 + u / 2): hi = 2^-6, lo = u 2^-7 exactly, so dropping the lo rows moves every element by u / 2 of S --
              several times the bound
    seams     B = 3 crops of different content
    random    B = 2
"""
import numpy as np
import torch

F32 = np.float32
TOKENS, GRID_H, GRID_W = 192, 16, 12
TAP_TOKENS = ((0, 0), (0, 11), (15, 0), (15, 11), (0, 5), (15, 6), (7, 0), (8, 11), (7, 5))
SUB = {'fp16': 2.0 ** -24, 'bf16': 2.0 ** -133}          # the smallest subnormal of the operand type
SUB_WEIGHT = {'fp16': 2.0 ** 8, 'bf16': 2.0 ** 40}      # lifts it to 2^-16 / 2^-93: normal in fp32
U16 = {'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8}


def r16(x, dtype):
    x = np.ascontiguousarray(x, F32)
    if dtype == 'fp16':
        x = np.clip(x, -65504.0, 65504.0)
    return torch.from_numpy(x).to(torch.float16 if dtype == 'fp16' else torch.bfloat16).float().numpy()


def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def _seed(name, dtype, D, K):
    return _rng(sum(ord(ch) for ch in name), 0 if dtype == 'fp16' else 1, D, K)


def _weights(rng, K, D):
    return (rng.standard_normal((K, D, 3, 3)) * (0.3 / np.sqrt(9.0 * D))).astype(F32), (rng.standard_normal(K) * 0.02).astype(F32)


def taps(dtype, D, K, tokens=TAP_TOKENS):
    B = len(tokens)
    x = np.zeros((B, TOKENS, D), F32)
    w = np.zeros((K, D, 3, 3), F32)
    chan = [(37 * n + 5) % D for n in range(B)]
    for n, (i, j) in enumerate(tokens):
        x[n, i * GRID_W + j, chan[n]] = 2.0
    for k in range(K):
        t = k % 9
        for c in set(chan):
            w[k, c, t // 3, t % 3] = 2.0 ** -(1 + k % 3)
    b = np.array([k % 3 - 1 for k in range(K)], F32)
    return dict(x=x, w=w, b=b)


def edges(dtype, D, K, variant='border', B=2):
    rng = _seed('edges' + variant, dtype, D, K)
    x = r16(rng.standard_normal((B, GRID_H, GRID_W, D)), dtype)
    keep = np.zeros((GRID_H, GRID_W), bool)
    if variant == 'corners':
        keep[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    else:
        keep[[0, -1], :] = True
        keep[:, [0, -1]] = True
    x = (x * keep[None, :, :, None]).reshape(B, TOKENS, D).astype(F32)
    w, b = _weights(rng, K, D)
    return dict(x=x, w=w, b=b)


def relu(dtype, D, K, variant='neg', B=1):
    rng = _seed('relu' + variant, dtype, D, K)
    w, b = _weights(rng, K, D)
    if variant == 'sub':
        sign = np.where(rng.random((B, TOKENS, D)) < 0.5, -1.0, 1.0)
        x = (sign * SUB[dtype]).astype(F32)
        w = (np.where(rng.random(w.shape) < 0.5, -1.0, 1.0) * SUB_WEIGHT[dtype] * 2.0 ** -rng.integers(0, 3, w.shape)).astype(F32)
        return dict(x=x, w=w, b=np.zeros(K, F32))
    x = r16(rng.standard_normal((B, TOKENS, D)), dtype)
    x[..., 0:8] = -0.0                               # minus zero under large weights
    w[:, 0:8] = 100.0
    x[..., 8:16] = -r16(rng.uniform(500.0, 1000.0, (B, TOKENS, 8)), dtype)   # far negative under large weights: a missing relu moves every element by ~1e5
    w[:, 8:16] = 25.0
    x[..., 16:24] = -SUB[dtype]                      # the smallest negative subnormal
    w[:, 16:24] = SUB_WEIGHT[dtype]
    return dict(x=x.astype(F32), w=w.astype(F32), b=b)


def lo_plane(dtype, D, K, B=1):
    rng = _seed('lo', dtype, D, K)
    x = r16(rng.uniform(0.5, 1.5, (B, TOKENS, D)), dtype)
    w = np.full((K, D, 3, 3), 2.0 ** -6 * (1.0 + U16[dtype] / 2), F32)
    return dict(x=x, w=w, b=np.zeros(K, F32))


def random(dtype, D, K, B=2, name='random'):
    rng = _seed(name, dtype, D, K)
    x = r16(rng.standard_normal((B, TOKENS, D)), dtype)
    w, b = _weights(rng, K, D)
    return dict(x=x, w=w, b=b)


def seams(dtype, D, K):
    return random(dtype, D, K, B=3, name='seams')
