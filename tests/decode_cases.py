"""Seeded case families for the heatmap decode kernel (tests/test_decode_model.py on the CPU, tests/test_gpu_decode.py on the device).

A family is a list of batches, each float32 [n, K, 64, 48] with only the crops and maps the family needs.  The class every joint is expected to fall
into (tests/decode_model.py: plateau / conditioned / ill-conditioned) is stated in the table and in EXPECTED, and asserted against the model on the CPU.

  family      what it holds                                                                                         expected classes
  ties        one tied pair of maxima per map on a sigma-2 blob centred on the lower index (TIE_PAIRS)              conditioned
  extremes    the maximum at flat index 0, 3, 4, 1023, 1024, 2047, 2048, 3071                                       conditioned
  corners     the arg-max on the four corners, one pixel inside each, and mid-edge on the four sides                conditioned
  nonpos      maps that are nowhere positive (all < 0 / max exactly 0 / all -inf) at k = 0, at k > 0, with K = 1    conditioned beside a bright last row,
              and K = 2, beside a neighbour that is bright along its whole last row, a dark one, and one with a     plateau beside a dark neighbour or alone,
              blob at (46, 62) only                                                                                 ill-conditioned beside the (46, 62) blob (near: not checked, maxval <= 0)
  clip        spikes whose centre sample is above the floor (0.001) / the ceiling (50) and whose axis neighbours    conditioned, and plateau for the map above 50
              are below; a map above 50 everywhere; a flat positive map                                             everywhere and the flat map
  peaked      peaked_heatmaps(3, 17, 11) and peaked_heatmaps(2, 133, 12)                                             by the model (may hold ill-conditioned joints)
  record      the record route's crops (K_e = 1, 2, 17, a non-positive joint 0 each) between bright neighbours      as nonpos
"""
from __future__ import annotations

import functools

import numpy as np

from cases import peaked_heatmaps

H, W = 64, 48


def blob(rng, x, y, amp=0.6, sigma=2.0, noise=0.005):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    g = amp * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * sigma * sigma))
    return (g + rng.normal(0, noise, size=g.shape)).astype(np.float32)


def raised(m, *flat_indices, by=0.02):
    """the map with the given pixels raised to one common value above everything else"""
    m = m.copy()
    top = np.float32(m.max() + np.float32(by))
    for i in flat_indices:
        m.reshape(-1)[i] = top
    return m


def _tie_pairs():
    """(lower index, higher index, what): thread t owns 4 t .. 4 t + 3, 1024 + 4 t .. and 2048 + 4 t ..; lane = t % 64, wave = t // 64"""
    idx = lambda t, load=0, e=0: 1024 * load + 4 * t + e
    out = [(idx(300, 1, 0), idx(300, 1, 2), 'one f32x4'), (idx(77, 0, 1), idx(77, 1, 1), 'one thread, loads 0 and 1'),
           (idx(140, 0, 3), idx(140, 2, 3), 'one thread, loads 0 and 2')]
    for d in (1, 2, 4, 8, 16, 32):
        t = 64 * (d % 4) + 37          # a lane whose bit d is clear, a different wave per distance
        t &= ~d
        out.append((idx(t, 1, 1), idx(t ^ d, 1, 2), f'one wave, lanes {t % 64} and {(t ^ d) % 64} ({d} apart)'))
    for wa in range(4):
        for wb in range(wa + 1, 4):
            ta, tb = 64 * wa + 11 + wb, 64 * wb + 50 - wa
            out.append((idx(ta, 1, 0), idx(tb, 1, 3), f'waves {wa} and {wb}, the lower index in wave {wa}'))
            out.append((idx(tb, 0, 2), idx(ta, 2, 1), f'waves {wa} and {wb}, the lower index in wave {wb}'))
    out += [(1020, 1024, 'thread 255 (index 1020) before thread 0 (index 1024)'), (2044, 2048, 'thread 255 (index 2044) before thread 0 (index 2048)')]
    assert all(a < b for a, b, _ in out)
    return out


TIE_PAIRS = _tie_pairs()
EXTREME_INDICES = (0, 3, 4, 1023, 1024, 2047, 2048, 3071)
CORNER_XY = [(0, 0), (47, 0), (0, 63), (47, 63), (1, 1), (46, 1), (1, 62), (46, 62), (24, 0), (24, 63), (0, 32), (47, 32)]


def ties():
    rng = np.random.default_rng(301)
    return [np.stack([raised(blob(rng, lo % W, lo // W), lo, hi) for lo, hi, _ in TIE_PAIRS])[None]]


def extremes():
    rng = np.random.default_rng(302)
    return [np.stack([raised(blob(rng, i % W, i // W), i) for i in EXTREME_INDICES])[None]]


def corners():
    rng = np.random.default_rng(303)
    return [np.stack([raised(blob(rng, x, y), y * W + x) for x, y in CORNER_XY])[None]]


def nonpositive(rng, kind):
    m = -np.abs(blob(rng, 20, 30)) - np.float32(0.01)
    if kind == 'zero':
        m[10, 10] = 0.0
    elif kind == 'inf':
        m[...] = -np.inf
    return m


def bright_row(rng, x=17, y=25):
    """a blob, and the whole last row bright: the three wrapped samples of the following map's joint all differ from log 0.001"""
    m = blob(rng, x, y)
    m[H - 1] = np.float32(0.5) + rng.normal(0, 0.005, W).astype(np.float32)
    return m


NONPOS_KINDS = ('neg', 'zero', 'inf')


def nonpos():
    rng = np.random.default_rng(304)
    k4 = np.stack([np.stack([nonpositive(rng, kind), bright_row(rng), nonpositive(rng, kind), bright_row(rng, 30, 40)]) for kind in NONPOS_KINDS])
    k1 = np.stack([nonpositive(rng, kind)[None] for kind in NONPOS_KINDS])
    k2 = [np.stack([nonpositive(rng, kind), bright_row(rng)]) for kind in NONPOS_KINDS]               # k = 0 wraps into the last map
    k2 += [np.stack([bright_row(rng), nonpositive(rng, kind)]) for kind in NONPOS_KINDS]              # k = 1 wraps into map 0
    k2 += [np.stack([nonpositive(rng, 'neg'), blob(rng, 46, 62)])]                                    # the ill-conditioned one: the bottom-left pixel is dark
    k2 += [np.stack([nonpositive(rng, kind), blob(rng, 20, 20, noise=0.0)]) for kind in ('neg', 'inf')]   # a dark neighbour (no noise: below the floor by a margin): plateau
    return [k4, k1, np.stack(k2)]


FLOOR_A, CEIL_A = np.float32(0.027), np.float32(1300.0)


def spike(x, y, a, side=0.05):
    """an isolated single-pixel spike on a zero background (at least 6 pixels from every border: no reflected copy of it in any of the seven windows), and a
    much smaller one at (x - 3, y - 2) that makes the blurred neighbourhood asymmetric without lifting an axis neighbour over the bound"""
    m = np.zeros((H, W), np.float32)
    m[y, x] = a
    m[y - 2, x - 3] = np.float32(side) * a
    return m


def clip():
    rng = np.random.default_rng(305)
    above = (np.float32(2000.0) + rng.normal(0, 1.0, (H, W))).astype(np.float32)
    flat = np.full((H, W), 0.25, np.float32)
    return [np.stack([spike(20, 30, FLOOR_A), spike(6, 6, FLOOR_A), spike(40, 57, FLOOR_A, 0.03), spike(21, 33, CEIL_A), spike(41, 8, CEIL_A, 0.03), above, flat])[None]]


def peaked():
    return [peaked_heatmaps(3, 17, 11), peaked_heatmaps(2, 133, 12)]


RECORD_KMAX = 17


def record():
    """The record route: (maps float32 [n_maps, 64, 48], records int32 [n, 3] = (first, K_e, dst)).  Crops with K_e = 1, 2 and 17, each with a non-positive
    joint 0, between neighbour crops (K_e = 17) whose maps are all bright along the last row -- the first and the last in particular: a wrap that runs modulo
    Kmax, or that leaves the crop's own maps on either side, reads a bright row where the crop's own wrap reads its own maps."""
    rng = np.random.default_rng(306)
    bright = lambda: [bright_row(rng, int(rng.integers(5, 43)), int(rng.integers(5, 55))) for _ in range(RECORD_KMAX)]
    crops = [bright(), [nonpositive(rng, 'neg')], bright(), [nonpositive(rng, 'zero'), bright_row(rng)],
             [nonpositive(rng, 'neg')] + [blob(rng, int(rng.integers(3, 45)), int(rng.integers(3, 60))) for _ in range(RECORD_KMAX - 2)] + [bright_row(rng)], bright()]
    ks = [len(c) for c in crops]
    first = np.cumsum([0] + ks[:-1])
    dst = np.array([3, 0, 5, 1, 4, 2])
    return np.concatenate([np.stack(c) for c in crops]), np.stack([first, ks, dst], 1).astype(np.int32)


def record_family():
    """the record route's crops as plain batches (what every row must equal)"""
    maps, rec = record()
    return [maps[f:f + k][None] for f, k, _ in rec]


FAMILIES = {'ties': ties, 'extremes': extremes, 'corners': corners, 'nonpos': nonpos, 'clip': clip, 'peaked': peaked, 'record': record_family}
MAY_BE_ILL = ('nonpos', 'peaked')   # no other family may hold an ill-conditioned joint
ILL_SHARE_MAX = 0.05             # of the joints of all families together
P, C, I = 0, 1, 2                # decode_model.PLATEAU, CONDITIONED, ILL
# the class of every joint, per batch and crop (one entry for all joints of a crop, or one per joint); peaked: whatever the model says
EXPECTED = {'ties': [[C]], 'extremes': [[C]], 'corners': [[C]],
            'nonpos': [[C, C, C], [P, P, P], [C, C, C, C, C, C, [I, C], [P, C], [P, C]]],
            'clip': [[[C, C, C, C, C, P, P]]],
            'record': [[C], [P], [C], [C], [C], [C]]}


@functools.lru_cache(maxsize=None)
def family(name):
    out = FAMILIES[name]()
    for b in out:
        b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def models(name):
    """the float64 model of every batch of a family, computed once and shared"""
    import decode_model as M
    return [M.decode_batch(b) for b in family(name)]


def nan_crops():
    """[3, 4, 64, 48]: a crop with NaN scattered in two of its maps between two clean crops, and the same batch with that crop replaced by a clean one"""
    rng = np.random.default_rng(307)
    mk = lambda: np.stack([raised(blob(rng, x, y), y * W + x) for x, y in ((0, 0), (30, 20), (47, 63), (10, 50))])
    clean = np.stack([mk(), mk(), mk()])
    clean[0, 0], clean[2, 0] = nonpositive(rng, 'neg'), nonpositive(rng, 'zero')   # their samples wrap into their own crop's last map, never into the NaN crop
    dirty = clean.copy()
    for k in (0, 3):
        dirty[1, k].reshape(-1)[rng.choice(H * W, 40, replace=False)] = np.nan
    dirty[1, 3, 63, 47] = dirty[1, 0, 0, 0] = np.nan
    return dirty, clean


def sizes(n, seed=0):
    """odd (org_w, org_h) per crop, the generator of the reference goldens"""
    from cases import org_sizes
    return org_sizes(n + 1, 40 + seed)[1:]


def affine_cs(n, seed=0):
    """cs [n, 4] = (c_x, c_y, S_w, S_h) float32 with S_w from 20 to 2000 (3:4 boxes), both ends included"""
    rng = np.random.default_rng(500 + seed)
    sw = np.exp(rng.uniform(np.log(20.0), np.log(2000.0), n))
    sw[0] = 20.0
    if n > 1:
        sw[-1] = 2000.0
    return np.stack([rng.uniform(-100, 1500, n), rng.uniform(-100, 1000, n), sw, sw * 4.0 / 3.0], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ flip-test batches
def flip_pairs(K):
    """mirror pairs for a K-map family: the map the samples of joint 0 wrap into (K - 1) has a partner of its own"""
    return [] if K < 2 else [[0, 1]] if K == 2 else [[K - 1, 1]] if K == 3 else [[K - 1, 1], [0, 2]]


def quantised(hm):
    """the case on a 2^-12 grid (non-finite values kept; -0 becomes +0, which is what an average of two finite values gives)"""
    with np.errstate(invalid='ignore'):
        return np.where(np.isfinite(hm), np.round(hm.astype(np.float64) * 4096.0) / 4096.0 + 0.0, hm).astype(np.float32)


def flip_batch(q, pairs, shift, seed=0):
    """The interleaved [2 n, K, 64, 48] batch whose flip-test average is exactly q (q on the 2^-12 grid, |q| < 2^11): the crop is q + p and the flipped-back
    mirror q - p with p a seeded multiple of 2^-12 in every pixel (columns 0 and 47 included), all exactly representable, so 0.5 ((q + p) + (q - p)) = q on
    every bit.  With `shift` the mirror's column 47 is read for columns 0 and 1, so p is chosen there to make q - p equal in both."""
    rng = np.random.default_rng(700 + seed)
    n, K = q.shape[:2]
    fin = np.isfinite(q)
    qq = np.where(fin, q, 0).astype(np.float64)
    p = rng.integers(-8, 9, q.shape).astype(np.float64) / 4096.0
    if shift:
        p[..., 1] = qq[..., 1] - qq[..., 0] + p[..., 0]
        assert (fin[..., 0] == fin[..., 1]).all()
    p = np.where(fin, p, 0.0)
    crop, back = (q + p).astype(np.float32), (q - p).astype(np.float32)      # q + 0 keeps -inf
    assert np.array_equal(crop.astype(np.float64)[fin], (qq + p)[fin]) and np.array_equal(back.astype(np.float64)[fin], (qq - p)[fin])
    partner = np.arange(K)
    for a, b in pairs:
        partner[a], partner[b] = b, a
    fb = back.copy()                                                         # the flipped-back mirror before the shift: b'[x] = fb[x - 1], b'[0] = fb[0]
    if shift:
        fb[..., :-1] = back[..., 1:]
    mirror = fb[:, partner][..., ::-1]
    out = np.empty((2 * n,) + q.shape[1:], np.float32)
    out[0::2], out[1::2] = crop, mirror
    return out


def merged_on_host(hm2, pairs, shift):
    """0.5 (crop + shifted flip_back(mirror)) in float32: what the flip-test kernel forms in registers"""
    from oracle import vitpose_cpu as O
    a, b = hm2[0::2], O.flip_back(hm2[1::2], pairs).copy()
    if shift:
        b[..., 1:] = b.copy()[..., :-1]
    return np.float32(0.5) * (a + b)
