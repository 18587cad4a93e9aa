"""The seeded cases of the orient stage (csrc/orientgeom.h), shared by tests/test_orient_host.py (host tap against independent models) and
tests/test_gpu_orient.py (device against the host tap).  A case is a list of `Spec`s, the frames of ONE call (at most 64); `buffers` lays a case out in host memory:
every plane of either side a view into its own canary-filled parent, at the pitch and the base offset its spec names.  Tiny inputs, chosen for where the kernel
forks: T is its tile edge."""
from __future__ import annotations

import collections

import numpy as np

from easy_vitpose_amd.cropprep import Frame

T = 64          # csrc/orientgeom.h ORIENT_TILE
CANARY = 0xA5
LEAD = 64       # canary bytes in front of a plane's first byte and behind its last (plus the base offset)
PITCHES = ('tight', 'p1', 'p13', 'a256')   # row bytes, + 1, + 13, the next multiple of 256
OFFSETS = (0, 1, 5)                        # of a plane's first byte from a 16-byte boundary
EXTENTS = (1, 2, T - 1, T, T + 1, 2 * T + 1)

# pitch / offset: the source planes'; dpitch / doffset: the destination planes' (None: the source's)
Spec = collections.namedtuple('Spec', 'fmt h w code pitch offset dpitch doffset matrix seed')


def spec(fmt, h, w, code, pitch='tight', offset=0, dpitch=None, doffset=None, matrix='bt601', seed=0):
    return Spec(fmt, h, w, code, pitch, offset, pitch if dpitch is None else dpitch, offset if doffset is None else doffset, matrix, seed)


def admitted(s: Spec) -> bool:
    """an NV12 frame takes a code only where every axis the code reverses has even length (written out here, not imported)"""
    if s.fmt != 'nv12':
        return True
    rev_row, rev_col = s.code in (3, 4, 6, 7), s.code in (2, 3, 7, 8)
    return not ((rev_row and s.h % 2) or (rev_col and s.w % 2))


def out_hw(h, w, code):
    return (w, h) if code >= 5 else (h, w)


def plane_shapes(fmt, h, w):
    return ((h, w), ((h + 1) // 2, (w + 1) // 2, 2)) if fmt == 'nv12' else ((h, w, 3),)


def pitch_of(row_bytes: int, mode: str) -> int:
    return {'tight': row_bytes, 'p1': row_bytes + 1, 'p13': row_bytes + 13, 'a256': (row_bytes + 255) // 256 * 256}[mode]


def layout(shape, mode, offset):
    """(parent bytes, first byte of the view, strides) of a plane of `shape` inside a parent whose base is 64-byte aligned"""
    rows, row_bytes = shape[0], int(np.prod(shape[1:]))
    pitch = pitch_of(row_bytes, mode)
    start = LEAD + offset
    return start + (rows - 1) * pitch + row_bytes + LEAD, start, (pitch,) + ((shape[2], 1) if len(shape) == 3 else (1,))


def aligned_parent(size: int) -> np.ndarray:
    raw = np.full(size + 64, CANARY, np.uint8)
    shift = (-raw.ctypes.data) % 64
    return raw[shift:shift + size]


def host_plane(shape, mode, offset):
    size, start, strides = layout(shape, mode, offset)
    parent = aligned_parent(size)
    view = np.lib.stride_tricks.as_strided(parent[start:], shape=shape, strides=strides, writeable=True)
    assert view.ctypes.data % 16 == offset
    return parent, view


def content(s: Spec):
    """the planes of a spec's source frame, tight: every byte random, so that any misplaced byte shows"""
    rng = np.random.default_rng([s.seed, s.h, s.w, s.code, len(s.fmt)])
    return [rng.integers(0, 256, shp, dtype=np.uint8) for shp in plane_shapes(s.fmt, s.h, s.w)]


def make_frame(s: Spec, planes):
    return Frame(s.fmt, tuple(planes), s.matrix)


Buffers = collections.namedtuple('Buffers', 'src dst codes src_parents dst_parents tight')


def buffers(specs) -> Buffers:
    """the host layout of one call: source `Frame`s (filled), destination `Frame`s (canary), their parents, and the tight source frames"""
    src, dst, sp, dp, tight = [], [], [], [], []
    for s in specs:
        planes, views = content(s), []
        for a in planes:
            parent, view = host_plane(a.shape, s.pitch, s.offset)
            view[...] = a
            sp.append(parent)
            views.append(view)
        src.append(make_frame(s, views))
        tight.append(make_frame(s, planes))
        views = []
        for shp in plane_shapes(s.fmt, *out_hw(s.h, s.w, s.code)):
            parent, view = host_plane(shp, s.dpitch, s.doffset)
            dp.append(parent)
            views.append(view)
        dst.append(make_frame(s, views))
    return Buffers(src, dst, np.array([s.code for s in specs], np.int32), sp, dp, tight)


def expected_parents(specs, oriented):
    """the destination parents a correct call leaves: canaries everywhere but the row bytes of the rows, which hold `oriented` (tight Frames, one per spec)"""
    want = []
    for s, f in zip(specs, oriented):
        for a in f.planes:
            size, start, strides = layout(a.shape, s.dpitch, s.doffset)
            parent = np.full(size, CANARY, np.uint8)
            np.lib.stride_tricks.as_strided(parent[start:], shape=a.shape, strides=strides, writeable=True)[...] = a
            want.append(parent)
    return want


def _chunks(specs, name, cases):
    specs = [s for s in specs if admitted(s)]
    for k in range(0, len(specs), 64):
        cases[f'{name}_{k // 64}'] = specs[k:k + 64]


def named_cases():
    c = {}
    cyc = [(p, o) for p in PITCHES for o in OFFSETS]
    # every extent pair on every code: ragged tiles on each side and in the corner, 1 x 1, 1 x (T + 1), (T + 1) x 1; 3 w is a multiple of 4 and of 16 only at w = T.
    # Pitch and offset walk through their combinations
    k, rgb = 0, []
    for h in EXTENTS:
        for w in EXTENTS:
            for code in range(1, 9):
                rgb.append(spec('rgb', h, w, code, *cyc[k % 12], seed=k))
                k += 1
    _chunks(rgb, 'rgb_extents', c)
    bgr = []
    for h, w in ((1, 1), (1, T + 1), (T + 1, 1), (2, T - 1), (T - 1, T), (T, T + 1), (T + 1, 2 * T + 1), (2 * T + 1, T - 1), (5, 7)):
        for code in range(1, 9):
            bgr.append(spec('bgr', h, w, code, *cyc[(k + 5) % 12], seed=k))
            k += 1
    _chunks(bgr, 'bgr_extents', c)
    # NV12, even sizes on all codes: the UV plane of 2 e x 2 e has e pairs, so both planes get ragged and full tiles
    nv = []
    for h, w in ((2, 2), (2, 2 * T + 2), (2 * T + 2, 2), (T - 2, T + 2), (T, T), (T + 2, T - 2), (2 * T - 2, 2 * T + 2), (2 * T, 2 * T), (2 * T + 2, 2 * T - 2), (4 * T + 2, 2), (2, 4 * T + 2),
                 (2 * T + 2, 4 * T + 2)):
        for code in range(1, 9):
            nv.append(spec('nv12', h, w, code, *cyc[(k + 7) % 12], matrix=('bt601', 'bt709', 'bt601_full')[k % 3], seed=k))
            k += 1
    # ... odd sizes on the codes that take them (1 and 5 any; the others where the odd axis is not reversed)
    for h, w in ((1, 1), (1, T + 1), (T + 1, 1), (T - 1, T + 1), (T + 1, T - 1), (2 * T + 1, 3), (3, 2 * T + 1), (T - 1, T), (T, T - 1)):
        for code in range(1, 9):
            nv.append(spec('nv12', h, w, code, *cyc[(k + 1) % 12], seed=k))
            k += 1
    _chunks(nv, 'nv12_extents', c)
    # every pitch x every offset on every code of every format, at one size with a full and a ragged tile per axis; then aligned sources into unaligned
    # destinations and the reverse
    # (3 w is a multiple of 4 at w = T + 4 alone: the width at which reversed three-byte pixels move as whole words)
    for fmt, (h, w) in (('rgb', (T + 1, T + 2)), ('rgb', (T + 1, T + 4)), ('bgr', (T + 2, T + 1)), ('nv12', (T + 2, 2 * T + 2))):
        lay = []
        for code in range(1, 9):
            for p, o in cyc:
                lay.append(spec(fmt, h, w, code, p, o, seed=k))
                k += 1
            lay.append(spec(fmt, h, w, code, 'a256', 0, 'p1', 5, seed=k))
            lay.append(spec(fmt, h, w, code, 'p13', 1, 'a256', 0, seed=k + 1))
            lay.append(spec(fmt, h, w, code, 'tight', 0, 'tight', 5, seed=k + 2))
            k += 3
        _chunks(lay, f'{fmt}_{h}x{w}_layouts', c)
    # one mixed table of 64 small frames that differ in size, format and code; 33 frames: two launches; none
    mixed = []
    i = 0
    while len(mixed) < 64:
        fmt = ('rgb', 'nv12', 'bgr')[i % 3]
        s = spec(fmt, 2 * (1 + (i * 5) % 37) if fmt == 'nv12' else 1 + (i * 5) % 71, 2 * (1 + (i * 11) % 41) if fmt == 'nv12' else 1 + (i * 11) % 67, 1 + i % 8, *cyc[i % 12],
                 matrix=('bt601', 'bt709')[i % 2], seed=1000 + i)
        mixed.append(s)
        i += 1
    c['mixed_64'] = mixed
    c['frames_33'] = [spec(('nv12', 'rgb')[i % 2], 2 * (3 + i), 2 * (40 - i), 1 + (i * 3) % 8, *cyc[(i * 7) % 12], seed=2000 + i) for i in range(33)]
    c['n_0'] = []
    assert all(len(v) <= 64 and all(admitted(s) for s in v) for v in c.values())
    return c


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def frames_equal(a: Frame, b: Frame) -> bool:
    return (a.format, a.matrix, a.h, a.w) == (b.format, b.matrix, b.h, b.w) and all(same_bits(p, q) for p, q in zip(a.planes, b.planes))
