"""Host model of what csrc/gemm8f.hip (the 8-phase GEMM on MXFP8 operands) adds to the arithmetic of its 16-bit sibling: the tile walk that decides which
workgroup multiplies which tile after which, the E8M0 / e4m3 output quantiser of mlp.fc1's epilogue (csrc/mx8.h) and the two output layouts the kernel
addresses by hand.  A plain module: tests/test_fp8_gemm_model.py pins it on the CPU, tests/test_gpu_fp8_gemm.py compares the kernel with it.

The walk (gemm8_common.h).  A launch has G = min(tiles, 256) workgroups; workgroup b sits on XCD x = b & 7 as number j0 = b >> 3 of nloc = (G >> 3) +
(x < (G & 7)); XCD x owns the contiguous tiles [base, base + cnt) and the workgroup walks base + j0, base + j0 + nloc, ...  A tile number becomes (row
tile, column tile) through the grouped order of TileWalk::origin.  Below 256 tiles nobody has a second tile.

The quantiser (mx8.h).  A block of 32 consecutive columns of one row: E = exponent field of the float32 amax minus 7 (0 where the field is at most 7), every
element times 2^(127 - E) -- the amax lands in [128, 256) -- and rounded to the nearest e4m3 code, ties to even (v_cvt_pk_fp8_f32).  e4m3 here is e4m3fn:
codes 0x00 .. 0x7e are the values m 2^-9 (exponent field 0) and (8 + m) 2^(e - 10) (field e >= 1) up to 448, 0x7f is NaN, bit 7 the sign.

Acceptance of an output block against a float64 interval [lo, hi] per element that contains the device's float32 value (rounding is monotone):
    scale byte   byte(amax of the lower ends' magnitudes) <= E <= byte(amax of the upper ends'): one value wherever the amax interval stays in a binade;
    code         GIVEN the device's byte: code(lo 2^(127 - E)) <= got <= code(hi 2^(127 - E)) in value order, raw bytes compared through their rank;
                 both zeros have rank 0, and the byte 0x80 (-0) is admissible only where lo < 0."""
import numpy as np

F32, F64 = np.float32, np.float64


# ---- the tile walk ------------------------------------------------------------------------------------------------------------------------------------------

def xcd_range(ntiles, grid, wg):
    """gemm8_common.h::xcd_range for workgroup wg of a grid: (base, cnt, nloc, j0)"""
    xcd, j0 = wg & 7, wg >> 3
    nloc = (grid >> 3) + (1 if xcd < (grid & 7) else 0)
    q, r8 = ntiles >> 3, ntiles & 7
    base = xcd * (q + 1) if xcd < r8 else r8 * (q + 1) + (xcd - r8) * q
    return base, q + (1 if xcd < r8 else 0), nloc, j0


def origin(bid, tiles_m, tiles_n, group_m):
    """TileWalk::origin without `reverse`: tile number -> (row tile, column tile)"""
    if group_m > 1:
        per = group_m * tiles_n
        grp = bid // per
        first = grp * group_m
        gsz = min(tiles_m - first, group_m)
        r = bid - grp * per
        return first + r % gsz, r // gsz
    return bid // tiles_n, bid % tiles_n


def walk(M, N, bm, bn, group_m):
    """the tiles of every workgroup in the order it multiplies them: list (one entry per workgroup) of lists of (row tile, column tile)"""
    tm, tn = M // bm, N // bn
    tiles = tm * tn
    grid = min(tiles, 256)
    out = []
    for wg in range(grid):
        base, cnt, nloc, j0 = xcd_range(tiles, grid, wg)
        out.append([origin(base + t, tm, tn, group_m) for t in range(j0, cnt, nloc)])
    return out


def colour_row_tiles(w, n_row_tiles):
    """Colours 0, 1, 2 .. for the row tiles such that two tiles one workgroup multiplies one after the other never share a colour (greedy, in row order).
    Returns (colours, n_colours); raises where consecutive tiles of a workgroup lie in the SAME row tile (their operand scales are the same bytes)."""
    adj = [set() for _ in range(n_row_tiles)]
    for tiles in w:
        for (a, _), (b, _) in zip(tiles, tiles[1:]):
            if a == b:
                raise ValueError('consecutive tiles of a workgroup share a row tile')
            adj[a].add(b)
            adj[b].add(a)
    col = [-1] * n_row_tiles
    for r in range(n_row_tiles):
        used = {col[o] for o in adj[r]}
        col[r] = next(c for c in range(n_row_tiles + 1) if c not in used)
    return np.array(col), max(col) + 1


# ---- e4m3 and the block quantiser ---------------------------------------------------------------------------------------------------------------------------

def e4m3_values():
    """the float64 value of each of the 256 codes (0x7f / 0xff: NaN)"""
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.exp2(e.astype(F64) - 10.0))
    v = np.where((c & 0x7f) == 0x7f, np.nan, v)
    return np.where(c & 0x80, -v, v)


_POS = e4m3_values()[:0x7f]                                                  # 0 .. 448, increasing


def e4m3_rne(v):
    """float64 -> the nearest e4m3 code, ties to the even code, saturating at 448 (0x7e); the sign of v (of -0.0 too) goes to bit 7"""
    v = np.asarray(v, F64)
    a = np.abs(v)
    hi = np.clip(np.searchsorted(_POS, a, side='left'), 1, 0x7e)             # _POS[hi - 1] <= a <= _POS[hi] inside the range
    lo = hi - 1
    dl, dh = a - _POS[lo], _POS[hi] - a
    code = np.where((dh < dl) | ((dh == dl) & (hi % 2 == 0)), hi, lo)
    code = np.where(a >= 448.0, 0x7e, code)
    return (code | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


def e4m3_trunc(v):
    """the mutant: round toward zero"""
    v = np.asarray(v, F64)
    code = np.clip(np.searchsorted(_POS, np.abs(v), side='right') - 1, 0, 0x7e)
    return (code | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


def rank(codes):
    """the codes in value order: a signed integer, both zeros 0"""
    c = np.asarray(codes).astype(np.int64)
    return np.where(c & 0x80, -(c & 0x7f), c & 0x7f)


def scale_byte(amax):
    """mx_scale_byte of a float64 magnitude that stands for a float32: exponent field minus 7, 0 where the field is at most 7 (zero, float32 subnormals)"""
    amax = np.asarray(amax, F64)
    with np.errstate(divide='ignore'):
        field = np.where(amax > 0, np.floor(np.log2(np.where(amax > 0, amax, 1.0))) + 127, 0)
    field = np.clip(field, 0, 254).astype(np.int64)
    return np.where(field > 7, field - 7, 0)


def block_amax(a):
    return np.asarray(a).reshape(a.shape[0], a.shape[1] // 32, 32).max(-1)


def quantise(v, rne=e4m3_rne):
    """mx8.h on float32 values v [M, N]: (E [M, N / 32], codes [M, N])"""
    v = np.asarray(v, F32).astype(F64)
    E = scale_byte(block_amax(np.abs(v)))
    return E, rne(v * np.repeat(np.exp2(127.0 - E), 32, axis=1))


def dequantise(E, codes):
    return e4m3_values()[codes] * np.repeat(np.exp2(np.asarray(E, F64) - 127.0), 32, axis=1)


def accept(lo, hi, E_dev, codes_dev, rne=e4m3_rne):
    """The acceptance of the module docstring on [M, N] intervals -> dict: bad_scale [M, N / 32], bad_code [M, N], open_scale [M, N / 32] (two admissible bytes),
    open_code [M, N] (more than one admissible code under the device's byte), E_lo, E_hi"""
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    E_dev = np.asarray(E_dev).astype(np.int64)
    inside = (lo <= 0) & (hi >= 0)
    a_lo = np.where(inside, 0.0, np.minimum(np.abs(lo), np.abs(hi)))
    a_hi = np.maximum(np.abs(lo), np.abs(hi))
    E_lo, E_hi = scale_byte(block_amax(a_lo)), scale_byte(block_amax(a_hi))
    inv = np.repeat(np.exp2(127.0 - E_dev), 32, axis=1)
    c_lo, c_hi = rne(lo * inv), rne(hi * inv)
    got = rank(codes_dev)
    bad = (got < rank(c_lo)) | (got > rank(c_hi)) | ((np.asarray(codes_dev) == 0x80) & ~(lo < 0)) | ((np.asarray(codes_dev) & 0x7f) == 0x7f)
    return dict(bad_scale=(E_dev < E_lo) | (E_dev > E_hi), bad_code=bad, open_scale=E_lo != E_hi, open_code=rank(c_lo) != rank(c_hi), E_lo=E_lo, E_hi=E_hi)


# ---- the layouts the kernel addresses by hand ---------------------------------------------------------------------------------------------------------------

def deblock64(buf, M, N):
    """[M/64][N/64][64][64] (GemmArgs::out_blocked) -> [M, N]"""
    return np.asarray(buf).reshape(M // 64, N // 64, 64, 64).transpose(0, 2, 1, 3).reshape(M, N)


def swap_lane_pair(a):
    """the mutant of B3: the two lanes of a 32-column block exchange their 16 columns"""
    M, N = a.shape
    return a.reshape(M, N // 32, 2, 16)[:, :, ::-1, :].reshape(M, N)


# ---- section A: the fp64 product of the operands the kernel multiplied ---------------------------------------------------------------------------------------

def product(a_deq, w_deq, bias):
    """(ref, mag) in float64: a w^T + bias and sum |a| |w|"""
    a, w = np.asarray(a_deq, F64), np.asarray(w_deq, F64)
    return a @ w.T + np.asarray(bias, F64)[None, :], np.abs(a) @ np.abs(w).T


def rescale_blocks(a_deq, E_true, E_used):
    """a_deq as the MFMA would see it with the scale bytes E_used in place of E_true (both [rows, K / 32])"""
    return np.asarray(a_deq, F64) * np.repeat(np.exp2(np.asarray(E_used, F64) - np.asarray(E_true, F64)), 32, axis=1)
