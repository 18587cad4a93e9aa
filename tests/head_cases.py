"""The seeded case families of the keypoint-head tests (tests/test_head_model.py on the CPU, tests/test_gpu_head.py on the device).  Every family takes
(dtype, B, Hin, Win, Cin) and returns the NHWC input x [B,Hin,Win,Cin] (float32 values of the operand type) and the raw tensors pack_deconv folds: w [Cin,256,4,4],
gamma, beta, mean, var [256]; final(dtype, Kp) returns the final 1x1 conv's w_fin [Kp,256] and b_fin [Kp].

    taps        exact.  BatchNorm is the identity (gamma 1, beta = mean = 0, var = float32(1 - 1e-5): scale == 1.0f, asserted).  Output channel o of 64-channel block
                o // 64 takes ONE tap (ti, tj) = divmod((o // 64 + rot) % 4, 2) of each output parity -- in the definition's terms ky in {2 ti, 2 ti + 1}, kx in
                {2 tj, 2 tj + 1} -- with weight 1.0 from source channel c(o) = (37 o + 11) mod Cin (one-to-one; every block of 64 output channels reaches every
                64-channel k-block); all other weights are 0.  x holds integer codes <= 64 (exact in bf16): channel c carries i + 1, j + 1, img + 1 or
                (c // 4) % 64 + 1 for c % 4 = 0, 1, 2, 3; channels no weight selects hold the poison 48.  The output is the source pixel's code, or exactly 0
                where the tap leaves the image: a wrong tap, parity, border, seam or channel is readable from the value.  rot = 0 and 1: every (parity, tap)
                pair on every n-range of a tile.
    onehot      the taps layout with full-mantissa weights of both signs and a real BatchNorm: ONE product per output, so one ulp of one folded weight is
                visible under the per-element bound -- the case that tells `fold, then round` from `round, then fold` at every shape and type (the Gaussian
                sum of the edges family hides it at fp16, Cin = 384)
    edges       Gaussian x and weights at the scales of test_deconv_bn_relu; every border row and column of every image x 32; one interior pixel per image 0 in
                all channels; gamma of both signs (o % 4 == 3 negative, channels 100 and 201 exactly 0); var cycles (0, 1e-6, 1, 30); |mean| up to 3
    relu_clamp  the edges data with beta chosen per channel group: NEG (0-7) -1e6: stored exactly 0; ZERO (8-23): the pre-activation at one output pixel per
                channel (PIX) within the bias's own float32 rounding of 0; BIG (24-27) +1e6: fp16 stores 65504, bf16 the rounded value; TINY (28-31): gamma 0
                and beta = k 1e-6: the pre-activation is beta everywhere, an fp16 subnormal
    final       w_fin = N(0, 0.02) with full float32 mantissas (lo carries bits), row 3 exactly 0 and the last row N(0, 8) (Kp >= 16); Kp in (1, 16, 17, 25, 133) =
                1, 1, 2, 2, 9 sixteen-joint groups, 16 with a full last group
Shapes: deconv1's geometry 16 x 12 with Cin = 384 (both types) and 1280 (fp16) at B = 1 (192 rows: less than one 256-row tile) and B = 3 (576 rows: on 128-row tiles the
seam at row 192 lies inside a tile and the one at 384 on a tile edge, the last 128- / 256-row tile is ragged, on 192-row tiles every seam is a tile edge); deconv2's
geometry 32 x 24 x 256 at B = 2 (the 24-pixel image rows straddle every tile height); the fused stage on deconv2's geometry at B = 1 and 2.
NaN and inf inputs are out of scope."""
import functools

import numpy as np

import head_model as HM

F32, F64 = np.float32, np.float64
DTYPES = ('fp16', 'bf16')
# the tiles the selection rule can put a deconv on (tile_rules.hip pick_gemm2_tile, epi 4): tests/test_head_model.py derives the set from the rule and asserts it
# equals this list; the fused stage's tile (EPI_DECONV_FINAL) runs stage 0 too -- the same gather on 256-row tiles -- though no rule picks it there
STAGE0_TILES = (31, 30, 12, 9, 1, 8)
FUSED_TILE = 3
DECONV1 = tuple((dt, B, 16, 12, Cin) for dt, Cin in (('fp16', 384), ('bf16', 384), ('fp16', 1280)) for B in (1, 3))
DECONV2 = tuple((dt, 2, 32, 24, 256) for dt in DTYPES)
FUSED = tuple((dt, B, 32, 24, 256) for dt in DTYPES for B in (1, 2))
KPS = (1, 16, 17, 25, 133)
POISON = 48.0
NEG, ZERO, BIG, TINY = slice(0, 8), slice(8, 24), slice(24, 28), slice(28, 32)


def _seed(*key):
    return [{'fp16': 1, 'bf16': 2}.get(k, k) for k in key]


def _tap_layout(Cin, rot):
    o = np.arange(256)
    ti, tj = np.divmod((o // 64 + rot) % 4, 2)
    c = (37 * o + 11) % Cin
    assert len(set(c)) == 256
    for b in range(4):                                   # every block of 64 output channels (one tap) reaches every 64-channel k-block
        assert set(c[b * 64:(b + 1) * 64] // 64) == set(range(Cin // 64))
    return o, ti, tj, c


def _codes(B, H, W, Cin, used):
    x = np.empty((B, H, W, Cin), F32)
    ch = np.arange(Cin)
    n, i, j = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing='ij')
    for r, v in enumerate((i + 1, j + 1, n + 1)):
        x[..., ch[ch % 4 == r]] = v[..., None]
    x[..., ch[ch % 4 == 3]] = ((ch[ch % 4 == 3] // 4) % 64 + 1).astype(F32)
    x[..., np.setdiff1d(ch, used)] = POISON
    assert x.max() <= 64 and x.min() >= 1
    return x


def _one_hot(Cin, rot, values):
    """w [Cin,256,4,4]: values[o, ky, kx] at source channel c(o) on the four (ky, kx) of channel o's tap, else 0"""
    o, ti, tj, c = _tap_layout(Cin, rot)
    w = np.zeros((Cin, 256, 4, 4), F32)
    for ky in range(4):
        for kx in range(4):
            m = (ky // 2 == ti) & (kx // 2 == tj)
            w[c[m], o[m], ky, kx] = values[m, ky, kx]
    return w, c


@functools.lru_cache(maxsize=None)
def taps(dtype, B, H, W, Cin, rot=0):
    w, c = _one_hot(Cin, rot, np.ones((256, 4, 4), F32))
    var = np.full(256, F32(1.0) - F32(1e-5), F32)
    assert ((var + HM.BN_EPS).astype(F32) == 1).all()    # the fold's scale is exactly 1.0f
    return dict(x=_codes(B, H, W, Cin, c), w=w, gamma=np.ones(256, F32), beta=np.zeros(256, F32), mean=np.zeros(256, F32), var=var, rot=rot)


def taps_expected(case):
    """the source pixel's code, or 0 where the tap leaves the image -- gathered directly, without the convolution"""
    x = case['x']
    B, H, W, Cin = x.shape
    o, ti, tj, c = _tap_layout(Cin, case['rot'])
    out = np.zeros((B, 2 * H, 2 * W, 256), F32)
    oy, ox = np.arange(2 * H), np.arange(2 * W)
    for t_i in range(2):
        for t_j in range(2):
            sel = (ti == t_i) & (tj == t_j)
            ky = 2 * t_i + (oy + 1) % 2                  # the ky of {2 ti, 2 ti + 1} with oy + 1 - ky even
            kx = 2 * t_j + (ox + 1) % 2
            iy, ix = (oy + 1 - ky) // 2, (ox + 1 - kx) // 2
            vy, vx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
            src = x[:, iy[vy][:, None], ix[vx][None, :]][..., c[sel]]
            out[:, oy[vy][:, None, None], ox[vx][None, :, None], np.flatnonzero(sel)[None, None, :]] = src
    return out


@functools.lru_cache(maxsize=None)
def onehot(dtype, B, H, W, Cin):
    rng = np.random.default_rng(_seed(dtype, 9, B, H, W, Cin))
    vals = (rng.uniform(0.5, 2.0, (256, 4, 4)) * np.where(rng.random((256, 4, 4)) < 0.5, -1.0, 1.0)).astype(F32)
    w, c = _one_hot(Cin, 0, vals)
    gamma = (1 + 0.1 * rng.standard_normal(256)).astype(F32)
    gamma[3::4] *= -1
    return dict(x=_codes(B, H, W, Cin, c), w=w, gamma=gamma, beta=(0.1 * rng.standard_normal(256)).astype(F32),
                mean=(0.5 * rng.standard_normal(256)).astype(F32), var=np.resize(np.array([0.3, 1.0, 2.5], F32), 256))


def _parts(case, dtype):
    """the folded operands of a case and the two float64 products every reference of it is built from (read-only: shared between tests)"""
    wf, bias = HM.fold(case['w'], case['gamma'], case['beta'], case['mean'], case['var'], dtype)
    z, A = HM.conv_parts(case['x'], wf)
    for a in (wf, bias, z, A):
        a.setflags(write=False)
    return dict(wf=wf, bias=bias, z=z, A=A)


@functools.lru_cache(maxsize=None)
def onehot_parts(dtype, B, H, W, Cin):
    return _parts(onehot(dtype, B, H, W, Cin), dtype)


@functools.lru_cache(maxsize=None)
def edges(dtype, B, H, W, Cin):
    rng = np.random.default_rng(_seed(dtype, B, H, W, Cin))
    x = rng.standard_normal((B, H, W, Cin), dtype=F32)
    border = np.zeros((H, W), bool)
    border[[0, -1], :] = True
    border[:, [0, -1]] = True
    x[:, border] *= 32
    for n in range(B):
        x[n, 1 + (5 * n + 3) % (H - 2), 1 + (7 * n + 2) % (W - 2)] = 0
    w = (rng.standard_normal((Cin, 256, 4, 4), dtype=F32) * (2.0 / (4 * Cin)) ** 0.5).astype(F32)
    gamma = np.abs(1 + 0.1 * rng.standard_normal(256)).astype(F32)
    gamma[3::4] *= -1
    gamma[[100, 201]] = 0
    return dict(x=HM.round16(x, dtype), w=w, gamma=gamma, beta=(0.1 * rng.standard_normal(256)).astype(F32),
                mean=rng.uniform(-3, 3, 256).astype(F32), var=np.resize(np.array([0, 1e-6, 1, 30], F32), 256))


@functools.lru_cache(maxsize=None)
def edges_parts(dtype, B, H, W, Cin):
    """... of the edges case (relu_clamp's are built from them)"""
    return _parts(edges(dtype, B, H, W, Cin), dtype)


def relu_pix(B, H, W):
    """PIX: the output pixel (img, oy, ox) of ZERO channel k at which its pre-activation is put at 0: corners, borders, the seam rows and interior pixels"""
    return [((3 * k) % B, (0, 2 * H - 1, 1, 2 * H - 2, 7, 2 * H // 2)[k % 6], (0, 2 * W - 1, 5, 2 * W - 2)[k % 4]) for k in range(ZERO.stop - ZERO.start)]


@functools.lru_cache(maxsize=None)
def relu_clamp(dtype, B, H, W, Cin):
    e, p = edges(dtype, B, H, W, Cin), edges_parts(dtype, B, H, W, Cin)
    gamma, beta = e['gamma'].copy(), e['beta'].copy()
    gamma[TINY] = 0
    beta[TINY] = F32(1e-6) * np.array([1, 2, 3, 0.5], F32)
    beta[NEG], beta[BIG] = -1e6, 1e6
    scale = (gamma / np.sqrt((e['var'] + HM.BN_EPS).astype(F32))).astype(F32)
    ms = (e['mean'] * scale).astype(F32)
    for k, (n, oy, ox) in enumerate(relu_pix(B, H, W)):
        o = ZERO.start + k
        beta[o] = F32(ms[o] - F32(p['z'][n, oy, ox, o]))             # bias = fl(beta - ms) is -z to a few float32 roundings of |ms| + |z|
    return dict(x=e['x'], w=e['w'], gamma=gamma, beta=beta, mean=e['mean'], var=e['var'])


@functools.lru_cache(maxsize=None)
def relu_parts(dtype, B, H, W, Cin):
    """edges_parts under relu_clamp's gamma and beta: the TINY channels' folded weights are 0 (tests/test_head_model.py checks this against a fresh fold)"""
    r, p = relu_clamp(dtype, B, H, W, Cin), edges_parts(dtype, B, H, W, Cin)
    wf, z, A = p['wf'].copy(), p['z'].copy(), p['A'].copy()
    wf[:, TINY], z[..., TINY], A[..., TINY] = 0, 0, 0
    _, bias = HM.fold(r['w'][:1], r['gamma'], r['beta'], r['mean'], r['var'], dtype)
    return dict(wf=wf, bias=bias, z=z, A=A)


@functools.lru_cache(maxsize=None)
def final(dtype, Kp):
    rng = np.random.default_rng(_seed(dtype, 77, Kp))
    w = (rng.standard_normal((Kp, 256)) * 0.02).astype(F32)
    if Kp >= 16:
        w[3] = 0
        w[Kp - 1] = (rng.standard_normal(256) * 8).astype(F32)
    return dict(w_fin=w, b_fin=(rng.standard_normal(Kp) * 0.1).astype(F32))
