"""A float64 model of one crop's heatmap decode (csrc/decode.hip decode_kernel), with a per-joint error bound and a conditioning class.

The model restates the KERNEL, statement by statement, in numpy float64 on the float32 input: the first-index arg-max and `maxval > 0` else (-1, -1); the seven
flat indices cx + 1 + (cy + 1)(W + 2) + k PADSZ + offs modulo K PADSZ; their split into (map, padded row, padded column); the edge clamp; the reflect-101
11 x 11 window; the float32 Gaussian weights of gauss11(); the clip to [0.001f, 50]; the log; the five differences; inv(H + eps I) with eps = 2^-23;
r = c - H^-1 g.  Everything after the float32 input is exact to float64 here, so what the device (or the float32 oracle) may differ by is the float32
arithmetic of the kernel, bounded term by term from the kernel's own operation counts (u = 2^-24, the unit roundoff of float32):

  blur      two passes of 11 products and 10 additions each (acc starts at 0, so the first addition is exact): every term of the window passes through at
            most 11 roundings per pass, |a_dev - a| <= ((1 + g11)^2 - 1) sum w_y w_x |v|, g11 = 11 u / (1 - 11 u) (a fused multiply-add only removes roundings).
            A window that holds -inf (and no NaN, no +inf) sums to -inf exactly: every weight is positive.
  clip+log  the clip is 1-Lipschitz and log' = 1 / a: |dl| <= da / max(a_clipped - da, 0.001).  A sample that is clipped with a margin larger than da on
            the device as well is the constant log(bound): no blur term.
  logf      LOGF_ULPS = 4 float32 ulps of the result: the device math library's figure is not documented in the toolchain's files, so this is the
            project's precedent for a device transcendental (tests/test_gpu_yolo.py, the SiLU).
  diffs     a float32 sum of n terms in any order is within (n - 1) u sum |terms| (first order): dx, dy 1 u (two terms, the 0.5 is exact), dxx, dyy 2 u
            (2 i_ is exact), dxy 7 u (eight terms).
  solve     (H + dH)(o + do) = g + dg  =>  |do| <= |H^-1| (|dg| + |dH| |o|) / (1 - rho), rho = || |H^-1| |dH| ||_inf, valid for rho < 1.  The float64
            evaluation of the 2 x 2 inverse adds 8 2^-53 (|a d| + b^2) / |det| relative to |o| (five float64 operations on a determinant with cancellation).
  store     rx, ry are stored as float32: u |r|.

Classes (decided here, never from the device's output):
  PLATEAU      all seven float64 samples are clipped to the same bound with a margin larger than da, or all seven windows hold identical values: the five
               differences are exactly 0 in float32 as well, H + eps I = eps I, the step is 0 and r = c on every bit.
  CONDITIONED  rho < RHO_MAX and max(bx, by) <= BOUND_MAX heatmap pixels: the coordinates must lie within the bound.
  ILL          everything else: only the arg-max is checked (a bit-equal confidence); where the bound is valid (rho < RHO_MAX) and places the device's
               coordinate within NEAR_PX of the arg-max (|o| + b <= NEAR_PX, maxval > 0), `near` is set and that is checked as well.
A joint whose own windows hold NaN (or both infinities) has class NAN: what it returns is outside the contract.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

H, W = 64, 48
PADSZ = (H + 2) * (W + 2)
OFFS = (0, 1, W + 2, W + 3, -W - 3, -1, -2 - W)   # i_, ix1, iy1, ix1y1, ix1_y1_, ix1_, iy1_ (decode.hip `offs`)
EPS = 2.0 ** -23
U = 2.0 ** -24
G11 = 11 * U / (1 - 11 * U)
BLUR_REL = (1 + G11) ** 2 - 1
LOGF_ULPS = 4
CLIP_LO, CLIP_HI = float(np.float32(0.001)), 50.0
PLATEAU, CONDITIONED, ILL, NAN = 0, 1, 2, 3
CLASS_NAMES = ('plateau', 'conditioned', 'ill-conditioned', 'nan')
RHO_MAX, BOUND_MAX, NEAR_PX = 0.5, 0.02, 1.5


def gauss11() -> np.ndarray:
    """decode.hip gauss11(): OpenCV getGaussianKernel(11, sigma <= 0), sigma = 2, float32 weights"""
    i = np.arange(11, dtype=np.float64)
    w = np.exp(-((i - 5.0) ** 2) / (2.0 * 2.0 * 2.0))
    return (w / w.sum()).astype(np.float32)


def reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def reflect_wrong(i, n):
    """BORDER_REFLECT (the edge pixel repeated) -- a wrong model"""
    i = np.where(i < 0, -i - 1, i)
    return np.where(i >= n, 2 * n - 1 - i, i)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# the wrong models of tests/test_decode_model.py: name -> what it changes
WRONG = ('reflect', 'last_tie', 'ge_zero', 'wrap_own_map', 'zero_pad', 'floor_1e-4', 'dy_sign', 'stride', 'eps0', 'wrap_kmax')


def decode_crop(maps: np.ndarray, K: int | None = None, wrong: str | None = None) -> dict:
    """maps: float32 [>= K, 64, 48], the crop's K maps first (what follows them in memory matters to the `wrap_kmax` wrong model only).
    Returns arrays over the K joints: rx, ry (float64, heatmap pixels, before the float32 store), cx, cy, idx, conf (float32), bx, by, rho, cls, near."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.shape[1:] == (H, W)
    K = len(maps) if K is None else K
    w = gauss11().astype(np.float64)
    reflect = reflect_wrong if wrong == 'reflect' else reflect101
    lo = 1e-4 if wrong == 'floor_1e-4' else CLIP_LO
    eps = 0.0 if wrong == 'eps0' else EPS
    offs = list(OFFS)
    if wrong == 'stride':
        offs[2] = W + 1
    out = {k: np.zeros(K) for k in ('rx', 'ry', 'cx', 'cy', 'bx', 'by', 'rho')}
    out['idx'] = np.zeros(K, np.int64)
    out['conf'] = np.zeros(K, np.float32)
    out['cls'] = np.zeros(K, np.int64)
    out['near'] = np.zeros(K, bool)
    total = (len(maps) if wrong == 'wrap_kmax' else K) * PADSZ
    for k in range(K):
        flat = maps[k].reshape(-1)
        has_nan = bool(np.isnan(flat).any())
        if has_nan:
            idx, maxval = 0, np.float32(np.nan)
        else:
            maxval = flat.max()
            hits = np.flatnonzero(flat == maxval)
            idx = int(hits[-1] if wrong == 'last_tie' else hits[0])
        positive = (maxval >= 0) if wrong == 'ge_zero' else (maxval > 0)
        cx, cy = (idx % W, idx // W) if positive else (-1, -1)
        a, da, wins = np.zeros(7), np.zeros(7), []
        zero_padded = np.zeros(7, bool)
        for s in range(7):
            f = cx + 1 + (cy + 1) * (W + 2) + k * PADSZ + offs[s]
            if wrong == 'wrap_own_map':
                f = k * PADSZ + (f - k * PADSZ) % PADSZ
            f %= total                                   # Python's % is the kernel's `f %= total; if (f < 0) f += total`
            kk, rem = divmod(f, PADSZ)
            py, px = rem // (W + 2) - 1, rem % (W + 2) - 1
            zero_padded[s] = wrong == 'zero_pad' and not (0 <= py < H and 0 <= px < W)
            py, px = min(max(py, 0), H - 1), min(max(px, 0), W - 1)
            rows, cols = reflect(py + np.arange(-5, 6), H), reflect(px + np.arange(-5, 6), W)
            win = maps[kk][np.ix_(rows, cols)].astype(np.float64)
            wins.append(win)
            if np.isnan(win).any() or (np.isposinf(win).any() and np.isneginf(win).any()):
                has_nan = True
            elif np.isinf(win).any():
                a[s], da[s] = (np.inf if np.isposinf(win).any() else -np.inf), 0.0
            else:
                a[s] = w @ win @ w
                da[s] = BLUR_REL * (w @ np.abs(win) @ w)
        out['idx'][k], out['conf'][k], out['cx'][k], out['cy'][k] = idx, maxval, cx, cy
        if has_nan:
            out['cls'][k] = NAN
            out['rx'][k] = out['ry'][k] = out['bx'][k] = out['by'][k] = np.nan
            continue
        ac = np.clip(a, lo, CLIP_HI)
        l = np.log(ac)
        sure_lo, sure_hi = a + da < lo, a - da > CLIP_HI
        with np.errstate(invalid='ignore'):
            dl = np.where(sure_lo | sure_hi, 0.0, da / np.maximum(ac - da, CLIP_LO)) + LOGF_ULPS * ulp32(l)
        if zero_padded.any():                            # wrong model: the log map padded with zeros
            l = np.where(zero_padded, 0.0, l)
        plateau = bool(sure_lo.all() or sure_hi.all() or all(np.array_equal(wins[0], x) for x in wins[1:])) and not zero_padded.any()
        i_, ix1, iy1, ix1y1, ix1_y1_, ix1_, iy1_ = l
        e_, ex1, ey1, ex1y1, ex1_y1_, ex1_, ey1_ = dl
        dx, dy = 0.5 * (ix1 - ix1_), 0.5 * (iy1 - iy1_)
        if wrong == 'dy_sign':
            dy = -dy
        dxx, dyy = ix1 - 2 * i_ + ix1_, iy1 - 2 * i_ + iy1_
        dxy = 0.5 * (ix1y1 - ix1 - iy1 + i_ + i_ - ix1_ - iy1_ + ix1_y1_)
        ddx = 0.5 * (ex1 + ex1_) + U * 0.5 * (abs(ix1) + abs(ix1_))
        ddy = 0.5 * (ey1 + ey1_) + U * 0.5 * (abs(iy1) + abs(iy1_))
        ddxx = ex1 + 2 * e_ + ex1_ + 2 * U * (abs(ix1) + 2 * abs(i_) + abs(ix1_))
        ddyy = ey1 + 2 * e_ + ey1_ + 2 * U * (abs(iy1) + 2 * abs(i_) + abs(iy1_))
        ddxy = 0.5 * (ex1y1 + ex1 + ey1 + 2 * e_ + ex1_ + ey1_ + ex1_y1_) \
            + 7 * U * 0.5 * (abs(ix1y1) + abs(ix1) + abs(iy1) + 2 * abs(i_) + abs(ix1_) + abs(iy1_) + abs(ix1_y1_))
        ha, hb, hd = dxx + eps, dxy, dyy + eps
        det = ha * hd - hb * hb
        with np.errstate(all='ignore'):
            ox, oy = np.float64(hd * dx - hb * dy) / det, np.float64(-hb * dx + ha * dy) / det
            hinv = np.abs(np.array([[hd, -hb], [-hb, ha]], dtype=np.float64) / det)
        rx, ry = cx - ox, cy - oy
        out['rx'][k], out['ry'][k] = rx, ry
        if plateau:                                      # bx = by = 0: the step is exactly 0 (a wrong model's own value is kept: eps = 0 gives 0 / 0)
            assert wrong is not None or (ox == 0 and oy == 0)
            out['cls'][k] = PLATEAU
            continue
        dH = np.array([[ddxx, ddxy], [ddxy, ddyy]])
        rho = float((hinv @ dH).sum(1).max()) if np.isfinite(hinv).all() else np.inf
        out['rho'][k] = rho
        if rho < 1:
            do = hinv @ (np.array([ddx, ddy]) + dH @ np.abs([ox, oy])) / (1 - rho)
            f64 = 8 * 2.0 ** -53 * (abs(ha * hd) + hb * hb) / abs(det)
            bx = do[0] + f64 * abs(ox) + U * abs(rx)
            by = do[1] + f64 * abs(oy) + U * abs(ry)
        else:
            bx = by = np.inf
        out['bx'][k], out['by'][k] = bx, by
        if rho < RHO_MAX and max(bx, by) <= BOUND_MAX:
            out['cls'][k] = CONDITIONED
        else:
            out['cls'][k] = ILL
            out['near'][k] = bool(rho < RHO_MAX and maxval > 0 and max(abs(ox) + bx, abs(oy) + by) <= NEAR_PX)
    return out


def decode_batch(hm: np.ndarray, wrong: str | None = None) -> dict:
    """[n, K, 64, 48] -> the fields of decode_crop as [n, K] arrays (every crop decoded on its own, as the kernel does)"""
    res = [decode_crop(np.ascontiguousarray(c, dtype=np.float32), wrong=wrong) for c in hm]
    return {k: np.stack([r[k] for r in res]) for k in res[0]}


def as_output(m: dict) -> np.ndarray:
    """a model's result as the kernel would store it in heatmap pixels: float32 [n, K, 3] = (ry, rx, conf)"""
    with np.errstate(all='ignore'):
        return np.stack([m['ry'].astype(np.float32), m['rx'].astype(np.float32), m['conf']], -1)


# ------------------------------------------------------------------------------------------------------------------ the frame mappings
def pad_frame(m: dict, org_wh, f32_steps: bool = False):
    """The pad route (decode.hip: fx = rx (ow / 47) + ow / 2 - ow 0.5 in float64, stored as float32; y with 63 and oh): the model's (y, x) in frame pixels
    [n, K, 2] and their bound.  The bound: the heatmap bound times the scale, plus the float32 store, u |f|, plus three float64 roundings of the larger
    operand (negligible, kept for the record).  f32_steps: the reference evaluates coords * scale + center - scale * 0.5 in float32, three roundings, of
    |r s|, |r s + c| and |f|.  org_wh = (94, 126): x = 2 rx + 47 - 47, exact."""
    wh = np.asarray(org_wh, dtype=np.int64).reshape(-1, 2)
    out, bound = [], []
    for axis, (r, b, span) in enumerate((('rx', 'bx', W - 1.0), ('ry', 'by', H - 1.0))):
        o = wh[:, axis].astype(np.float64)[:, None]
        s, c0, c1 = o / span, (wh[:, axis] // 2).astype(np.float64)[:, None], o * 0.5
        rr = m[r]                                                             # (the float32 store of rx, ry is inside the heatmap bound)
        f = rr * s + c0 - c1
        mag = np.maximum(np.abs(rr * s), np.maximum(np.abs(rr * s + c0), np.abs(f)))
        rnd = U * (np.abs(rr * s) + np.abs(rr * s + c0) + np.abs(f)) if f32_steps else U * np.abs(f)
        out.append(f)
        bound.append((m[b] * s + rnd + 3 * 2.0 ** -53 * mag) * (1 + 2.0 ** -20))   # (the roundings are relative to the device's own values)
    return np.stack(out[::-1], -1), np.stack(bound[::-1], -1)


def affine_frame(m: dict, cs):
    """The affine route (decode.hip AFF: x = (float)(rx (S_w / 47) + c_x - S_w 0.5), every float64 step unfused): (y, x) [n, K, 2] and the bound, the heatmap
    bound times the scale plus the float32 store and three float64 roundings."""
    cs = np.asarray(cs, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    out, bound = [], []
    for r, b, span, ci, si in (('rx', 'bx', W - 1.0, 0, 2), ('ry', 'by', H - 1.0, 1, 3)):
        s, c = (cs[:, si] / span)[:, None], cs[:, ci][:, None]
        half = cs[:, si][:, None] * 0.5
        rr = m[r]
        f = rr * s + c - half
        mag = np.maximum(np.abs(rr * s), np.maximum(np.abs(rr * s + c), np.abs(f)))
        out.append(f)
        bound.append((m[b] * s + U * np.abs(f) + 3 * 2.0 ** -53 * mag) * (1 + 2.0 ** -20))
    return np.stack(out[::-1], -1), np.stack(bound[::-1], -1)


def pad_plateau_bits(c: int, o: int, span: int) -> set:
    """The float32 values a plateau coordinate c may take on the pad route: c (o / span) + o / 2 - o 0.5 evaluated in float64 as written, or with the product
    and the first addition fused (the kernel's unit is compiled with contraction allowed) -- both are that line of decode.hip."""
    s = float(o) / float(span)
    c0, c1 = float(o // 2), float(o) * 0.5
    plain = np.float32(float(c) * s + c0 - c1)
    fused = np.float32(float(Fraction(float(c)) * Fraction(s) + Fraction(c0)) - c1)
    return {plain.view(np.uint32).item(), fused.view(np.uint32).item()}


# ------------------------------------------------------------------------------------------------------------------ the class rules
def check(m: dict, got: np.ndarray, route: str = 'pad', arg=None, f32_steps: bool = False, conf: bool = True):
    """`got` [n, K, 3] (y, x, conf) against the model `m` of the same maps under the class rules.  route 'hm': got is in heatmap pixels (x = rx);
    'pad': arg = org_wh [n, 2]; 'affine': arg = cs [n, 4].  Returns (worst err / bound over the conditioned joints, list of failure strings)."""
    got = np.asarray(got)
    n, K = m['cls'].shape
    if route == 'hm':
        want = np.stack([m['ry'], m['rx']], -1)
        bound = np.stack([m['by'], m['bx']], -1) + (U * np.abs(want) * 3 if f32_steps else 0)
        scale = np.ones((n, 2))
        centre = np.stack([m['cy'], m['cx']], -1)
    else:
        want, bound = pad_frame(m, arg, f32_steps) if route == 'pad' else affine_frame(m, arg)
        a = np.asarray(arg, dtype=np.float64).reshape(n, -1)
        scale = np.stack([a[:, -1] / (H - 1.0), a[:, -2] / (W - 1.0)], -1)
        cm = dict(m, rx=m['cx'], ry=m['cy'], bx=np.zeros((n, K)), by=np.zeros((n, K)))
        centre = (pad_frame(cm, arg) if route == 'pad' else affine_frame(cm, arg))[0]
    fails, worst = [], 0.0
    for i in range(n):
        for k in range(K):
            cls, g = m['cls'][i, k], got[i, k].astype(np.float64)
            where = f'crop {i} joint {k} ({CLASS_NAMES[cls]})'
            if cls == NAN:
                continue
            if conf and got[i, k, 2:].view(np.uint32)[0] != m['conf'][i, k:k + 1].view(np.uint32)[0]:
                fails.append(f'{where}: confidence {got[i, k, 2]!r} != {m["conf"][i, k]!r}')
            if cls == PLATEAU:
                ok = True
                for ax, (c, span) in enumerate(((m['cy'][i, k], H - 1), (m['cx'][i, k], W - 1))):
                    if route == 'pad' and not f32_steps:
                        ok &= got[i, k, ax:ax + 1].view(np.uint32)[0].item() in pad_plateau_bits(int(c), int(np.asarray(arg).reshape(n, 2)[i, 1 - ax]), span)
                    elif f32_steps:
                        ok &= abs(g[ax] - want[i, k, ax]) <= bound[i, k, ax]   # the float32 mapping's own roundings only (bx = by = 0)
                    else:
                        ok &= got[i, k, ax] == np.float32(want[i, k, ax])
                if not ok:
                    fails.append(f'{where}: ({g[0]!r}, {g[1]!r}) is not the arg-max ({want[i, k, 0]!r}, {want[i, k, 1]!r}) exactly')
            elif cls == CONDITIONED:
                ratio = float((np.abs(g[:2] - want[i, k]) / bound[i, k]).max()) if np.isfinite(g[:2]).all() else np.inf
                worst = max(worst, ratio)
                if not ratio <= 1:
                    fails.append(f'{where}: error / bound {ratio:.3g} (got {g[:2]}, model {want[i, k]}, bound {bound[i, k]})')
            elif m['near'][i, k]:
                d = np.abs(g[:2] - centre[i, k]) / scale[i]   # + the float32 roundings of the two mapped positions
                if not (d <= NEAR_PX + 4 * ulp32(np.maximum(np.abs(g[:2]), np.abs(centre[i, k]))) / scale[i]).all():
                    fails.append(f'{where}: {d} heatmap pixels from the arg-max')
    return worst, fails
