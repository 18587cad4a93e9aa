"""The seeded problems of the MXFP8 GEMM's tests (tests/test_fp8_gemm_model.py on the CPU, tests/test_gpu_fp8_gemm.py on the device).  GEMM shapes are
(M, N, K) with K the reduction depth.

A. hand_over(name, K)   launches of MORE than 256 tiles, so that a workgroup multiplies a second (third) tile: HAND_OVER lists them.  The A operand is made
                        so that a scale dword from the wrong place is wrong by a power of two.  Gaussians, every 32-k block scaled to the amax
                        1.5 * 2^(rule + term + SHIFT):
                            rule(row tile, K-tile) = ORDER[K-tile] + 4 colour(row tile)   ORDER = 0 1 2 3 (nk = 4) / 0 1 4 5 2 3 (nk = 6): K-tiles 0, 1 and the
                                                     last two of a tile take 0 .. 3, every K-tile differs from the one and the two before it; colour() is
                                                     fp8_gemm_model.colour_row_tiles, so two tiles a workgroup multiplies one after the other are 4 apart;
                            term(row, block)       = (5 (row % 256) + 3 (block % 4)) % 7 - 3, within 2^-3 .. 2^3: a function of the place INSIDE the tile and
                                                     the K-tile alone, so at one lane's place the bytes of different (tile, K-tile) differ by the rule alone --
                                                     and rows 16, 64, 128 apart and the four blocks of a K-tile differ too.
                        The scale byte of a block is then 120 + rule + term + SHIFT exactly (checked on the bytes the device wrote).
B. fc1_exact()          M = 512, K = 512, N = 2048 (16 tiles).  Column n carries the pre-activation bias[n]: FAMILIES of 32-column blocks, listed below.  Rows
                        0, 100, 300, 511 have A = 0 and see bias[n] itself; row m elsewhere is one-hot, A[m, 32 (m // 256)] = s_m, and W[n, 0] = 448 2^j(n),
                        W[n, 32] = -+448 2^j(n) with 2^j(n) about |bias[n]| / 2^12: the accumulator is one exactly representable product, all rows differ; |s_m| <= 7.5 keeps the product
                        below |bias[n]|, so no row turns a whole block into GELU's far negative tail (all -0, where the model's slack for a denormal exp2 is all there is).
C. qkv_exact(mixed)     M = 512, N = 2304, K = 512, small integers: every partial sum is an integer far inside float32, the result far inside fp16's integers."""
import functools

import numpy as np

import fp8_gemm_model as FM
import ln_consumer_model as LM
import mlp_cases as MC
import mlp_model as MM

F32, F64 = np.float32, np.float64

# name -> (epi, M, N, tile width, tiles, group_m of the fp8 mode's rule for that GEMM, the depths K it runs at)
HAND_OVER = {
    'qkv': (0, 24576, 768, 256, 288, 4, (512, 768)),
    'qkv, three tiles': (0, 45056, 768, 256, 528, 4, (512,)),
    'fc1': (1, 24576, 768, 256, 288, 8, (512, 768)),
    'residual 256x192 (LDS-staged)': (6, 24576, 768, 192, 384, 2, (512, 768)),
    'residual 256x256 (register-direct)': (6, 18432, 1024, 256, 288, 2, (512, 768)),
}
HAND_OVER_CASES = [(name, K) for name, v in HAND_OVER.items() for K in v[6]]
ORDER = {4: (0, 1, 2, 3), 6: (0, 1, 4, 5, 2, 3)}
SHIFT = -11


def term(M, K):
    r = np.arange(M)[:, None] % 256
    b = np.arange(K // 32)[None, :] % 4
    return (5 * r + 3 * b) % 7 - 3


@functools.lru_cache(maxsize=None)
def rule(name, K):
    """([row tiles, K-tiles], the walk it was coloured for, the number of colours)"""
    epi, M, N, bn, tiles, gm, _ = HAND_OVER[name]
    w = FM.walk(M, N, 256, bn, gm)
    col, ncol = FM.colour_row_tiles(w, M // 256)
    nk = K // 128
    return np.asarray(ORDER[nk])[None, :] + 4 * col[:, None], w, ncol


def block_exponent(name, K):
    """[M, K / 32]: e of every block of A (amax = 1.5 2^e)"""
    M = HAND_OVER[name][1]
    r, _, _ = rule(name, K)
    return np.repeat(np.repeat(r, 256, axis=0), 4, axis=1) + term(M, K) + SHIFT


def expected_scale_bytes(name, K):
    return block_exponent(name, K) + 120


def hand_over(name, K):
    """dict A [M, K], W [N, K], bias [N], and for epi 6 the residual as fp16 plane bits r_hi, r_lo [M, N]"""
    epi, M, N, bn, tiles, gm, _ = HAND_OVER[name]
    rng = np.random.default_rng(9000 + M + N + K + epi)
    A = rng.standard_normal((M, K), dtype=F32)
    blk = A.reshape(M, K // 32, 32)
    blk *= (1.5 * np.exp2(block_exponent(name, K)) / np.abs(blk).max(-1)).astype(F32)[..., None]      # amax = 1.5 2^e: the code 192, the byte readable off a_deq
    W = (rng.standard_normal((N, K), dtype=F32) * F32(0.04))
    W[:, 1] += (0.1 * (np.arange(N) % 5)).astype(F32)
    bias = (rng.standard_normal(N) * 0.1).astype(F32)
    out = dict(A=A, W=W, bias=bias)
    if epi == 6:
        r = (rng.standard_normal((M, N), dtype=F32) * F32(2.0))
        hi = r.astype(np.float16)
        out['r_hi'] = hi.view(np.uint16)
        out['r_lo'] = (r - hi.astype(F32)).astype(np.float16).view(np.uint16)
    return out


def owners(name):
    """number of tiles per workgroup, from the walk"""
    epi, M, N, bn, tiles, gm, _ = HAND_OVER[name]
    return np.array([len(t) for t in FM.walk(M, N, 256, bn, gm)])


def sample_rows(name, per_tile=16):
    """rows for the fp64 check: per_tile rows of the first, second (and third) tile of the first and the last workgroup that has the most tiles -- at
    offsets that meet both X halves, all four 64-row wave groups and different fragment rows.  -> (rows, position in the walk of each row's tile)"""
    epi, M, N, bn, tiles, gm, _ = HAND_OVER[name]
    w = FM.walk(M, N, 256, bn, gm)
    most = max(len(t) for t in w)
    wgs = [i for i, t in enumerate(w) if len(t) == most]
    offs = (np.arange(per_tile) * 37 + 5) % 256
    rows, pos = [], []
    for wg in (wgs[0], wgs[-1]):
        for p, (rt, _) in enumerate(w[wg]):
            rows += list(rt * 256 + offs)
            pos += [p] * per_tile
    return np.array(rows), np.array(pos)


def chunks(name):
    """row ranges [(m0, m1)] that cover M in launches of at most 255 tiles each (whole row tiles, the full width)"""
    epi, M, N, bn, tiles, gm, _ = HAND_OVER[name]
    tn = N // bn
    rt = M // 256
    n = -(-rt * tn // 255)
    while -(-rt // n) * tn > 255:
        n += 1
    per = -(-rt // n)
    return [(i * per * 256, min((i + 1) * per, rt) * 256) for i in range(n) if i * per < rt]


# ---------------------------------------------------------------------------------------------------------------- B. the fc1 epilogue

B1_M, B1_N, B1_K = 512, 2048, 512
PURE_ROWS = (0, 100, 300, 511)
FAMILIES = ('sweep', 'zero', 'lone amax, columns 0-15', 'lone amax, columns 16-31', 'amax a power of two', 'amax one ulp below a power of two',
            'subnormal codes', 'ties', 'negative tail', 'large')
EXEMPT = ('ties', 'amax a power of two', 'amax one ulp below a power of two')      # built to sit on a decision: not counted in the undecided share


def _below(x):
    return np.nextafter(F32(x), F32(0))


@functools.lru_cache(maxsize=None)
def fc1_bias():
    """(bias [N] float32, family index per 32-column block [N / 32])"""
    rng = np.random.default_rng(4242)
    blocks, fam = [], []

    def add(name, v):
        v = np.asarray(v, F32)
        assert v.shape == (32,)
        blocks.append(v)
        fam.append(FAMILIES.index(name))

    z = np.zeros(32, F32)
    add('zero', z)
    for name, col in (('lone amax, columns 0-15', 5), ('lone amax, columns 16-31', 27)):
        for val in (1.75, -3.0):                                              # GELU(-3) = -4e-3: a lone negative amax
            v = z.copy()
            v[col] = val
            add(name, v)
    # amax exactly 2^k: x >= 16 is the `far` range of mlp_model (GELU(x) == x), x <= 2^-26 its `tiny` range (GELU(x) == x / 2); the rest of the block is ordinary
    for p, lone in ((16.0, 3), (1024.0, 20), (2.0 ** -27, 9), (2.0 ** -40, 30)):
        for name, top in (('amax a power of two', F32(p)), ('amax one ulp below a power of two', _below(p))):
            v = (rng.uniform(-0.9, 0.9, 32) * p).astype(F32)
            v[lone] = top
            add(name, v)
    # subnormal codes: the top binade is GELU(3) = 2.996 -> [2, 4); elements 2^-6 .. 2^-9 of it, and below 2^-10 of it (GELU(x) = x / 2 for small x)
    for sign in (1.0, -1.0):
        v = (sign * 4.0 * np.exp2(-rng.uniform(6.0, 9.0, 32))).astype(F32)
        v[24:] = (sign * 4.0 * np.exp2(-rng.uniform(10.0, 14.0, 8))).astype(F32)
        v[int(rng.integers(0, 24))] = 3.0
        add('subnormal codes', v)
    # ties.  Subnormal and first-binade codes: the amax element gives GELU in [2^-14, 2^-13) -> E = 106, code spacing 2^-30 below 2^-26; x = (2 i + 1) 2^-30 is in
    # the tiny range, GELU = (i + 1/2) 2^-30 exactly: ties above the codes i = 0 .. 13 (even and odd; 0 .. 7 subnormal, 8 .. 13 normal)
    v = z.copy()
    v[0] = 1.5 * 2.0 ** -13
    t = (2 * np.arange(14) + 1) * 2.0 ** -30
    v[1:15], v[16:30] = t, -t
    add('ties', v)
    # normal codes: x in [16, 32) is far, GELU == x; amax 31 -> scaled by 8, codes 16 apart in [128, 256): 17 + 2 i ties above the codes 8 i, even and odd
    v = np.concatenate([17.0 + 2.0 * np.arange(8), 16.0 + 2.0 * np.arange(8), 17.0 + 2.0 * np.arange(8), rng.uniform(16.0, 31.0, 8)]).astype(F32)
    add('ties', v)
    # the negative tail: beside ordinary values (codes of -0), and a block of its own (tiny negatives with codes of their own)
    v = rng.uniform(-2.0, 2.0, 32).astype(F32)
    v[[1, 4, 9, 17, 22, 31]] = [-8.5, -9.0, -11.0, -13.0, -40.0, -1e4]
    add('negative tail', v)
    add('negative tail', rng.uniform(-10.5, -8.2, 32).astype(F32))
    for top in (1e4, 3e3):
        v = rng.uniform(100.0, top, 32).astype(F32)
        v[int(rng.integers(0, 32))] = top
        v[::5] *= -1.0
        add('large', v)
    # the GELU sweep's own pre-activations (every bf16 pattern, scaled and biased), ordered by magnitude so that a block holds one size of them
    x = MC.gelu_sweep('bf16')['x']
    x = x[np.isfinite(x) & (np.abs(x) < 2.0 ** 100) & ((x == 0) | (np.abs(x) > 2.0 ** -100))]
    # between mlp_model's two exact ranges a value of few significant bits (s w with b = 0) puts GELU = x / 2 (1 + 0.8 |x|) within 1e-7 of a code boundary, and the
    # model leaves such elements open: there the sample keeps the values that the sweep's bias made generic (more than 12 significant bits)
    tiny, far = MM.ranges(x)
    x = x[tiny | far | ((x.view(np.uint32) & 0xfff) != 0)]
    n = B1_N - 32 * len(blocks)
    s = x[np.linspace(0, x.size - 1, n).astype(np.int64)]
    s = s[np.argsort(np.abs(s), kind='stable')]
    for i in range(n // 32):
        add('sweep', s[32 * i:32 * i + 32])
    order = rng.permutation(len(blocks))               # the families spread over the tiles and the waves
    return np.concatenate([blocks[i] for i in order]), np.array([fam[i] for i in order])


@functools.lru_cache(maxsize=None)
def fc1_exact():
    """dict A [M, K], W [N, K], bias [N], family [N / 32], pure (row mask), x [M, N] (the float32 pre-activation, bit for bit), s [M], ws [N]"""
    M, N, K = B1_M, B1_N, B1_K
    bias, fam = fc1_bias()
    m = np.arange(M) % 256
    s = ((8 + (m & 7)) / 8.0 * np.exp2(((m >> 3) & 15) - 13.0) * np.where(m & 128, -1.0, 1.0)).astype(F32)      # 256 different e4m3 values times a power of two
    s[list(PURE_ROWS)] = 0
    A = np.zeros((M, K), F32)
    A[np.arange(M), 32 * (np.arange(M) // 256)] = s
    ab = np.abs(bias.astype(F64))
    j = np.where(ab > 0, np.floor(np.log2(np.where(ab > 0, ab, 1.0))) - 12, -20.0)
    ws = np.exp2(j).astype(F32)                                             # the per-channel scale the packer derives: max |row| / 448
    W = np.zeros((N, K), F32)
    w1 = np.where(np.arange(N) % 3 == 0, F32(-448), F32(448))                # rows 256 .. 511 multiply this column: the same |product|, another sign pattern
    W[:, 0], W[:, 32] = F32(448) * ws, w1 * ws
    code = np.where(np.arange(M)[:, None] < 256, F32(448), w1[None, :])
    acc = (s[:, None] * code).astype(F32)                                   # an e4m3 value times a 4-bit integer: exact
    x = LM.fma32(acc, ws[None, :], bias[None, :])
    pure = np.zeros(M, bool)
    pure[list(PURE_ROWS)] = True
    return dict(A=A, W=W, bias=bias, family=fam, pure=pure, x=x, s=s, ws=ws)


def check_families(c):
    """the conditions the B1 problem promises, on the pure rows (x == bias): which family stands where, and that each is what its name says -> number of ties"""
    import mlp_model as MM
    bias, fam = c['bias'], c['family']
    assert np.array_equal(c['x'][list(PURE_ROWS)].view(np.uint32), np.broadcast_to(bias, (len(PURE_ROWS), bias.size)).view(np.uint32))
    assert set(fam) == set(range(len(FAMILIES))), 'a family is missing'
    g = MM.centre(bias, 'bf16').reshape(-1, 32)
    e = MM.e32(bias, 'bf16').reshape(-1, 32)
    b = bias.reshape(-1, 32)
    amax = np.abs(g).max(-1)
    is_ = lambda name: fam == FAMILIES.index(name)
    assert (amax[is_('zero')] == 0).all()
    for name, cols in (('lone amax, columns 0-15', slice(0, 16)), ('lone amax, columns 16-31', slice(16, 32))):
        blk = b[is_(name)]
        assert len(blk) and ((blk != 0).sum(-1) == 1).all() and ((blk[:, cols] != 0).sum(-1) == 1).all()
    for name in ('amax a power of two', 'amax one ulp below a power of two'):
        p2, pe = g[is_(name)], e[is_(name)]
        top = np.abs(p2).max(-1)
        assert len(p2) >= 3 and (pe[np.arange(len(p2)), np.abs(p2).argmax(-1)] == 0).all(), name      # the value is exact there
        assert (top.astype(F32) == top).all()
        if 'below' in name:
            top = np.nextafter(top.astype(F32), F32(np.inf)).astype(F64)
        assert (np.frexp(top)[0] == 0.5).all(), name
    sg = np.abs(g[is_('subnormal codes')])
    sub = sg / np.exp2(np.floor(np.log2(sg.max(-1))))[:, None]
    assert (((sub >= 2.0 ** -9) & (sub < 2.0 ** -6)).sum(-1) >= 16).all() and ((sub < 2.0 ** -10).sum(-1) >= 4).all()
    # ties: scaled by the block's own scale the exact value sits half-way between two codes, for even and for odd lower neighbours, subnormal and normal
    tg, te = g[is_('ties')], e[is_('ties')]
    E = FM.scale_byte(np.abs(tg).max(-1))
    sc = np.abs(tg) * np.exp2(127.0 - E)[:, None]
    vals = FM.e4m3_values()[:0x7f]
    lo = np.clip(np.searchsorted(vals, sc, side='right') - 1, 0, 0x7d)
    tie = (sc - vals[lo] == vals[lo + 1] - sc) & (te == 0)
    kinds = {(bool(l < 8), bool(l & 1)) for l in lo[tie]}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}, kinds
    assert tie.sum() >= 40
    nt = b[is_('negative tail')]
    assert (nt < -8).any(-1).all() and (nt < -8).all(-1).any() and (nt <= -13).any()
    assert np.abs(b[is_('large')]).max() == 1e4
    assert is_('sweep').sum() >= 16
    return int(tie.sum())


def fc1_interval(x):
    """[lo, hi] per element for the float32 value gelu_erf(x) (gelu_core with relu = max(x, 0): mlp_model's bf16 flavour)"""
    import mlp_model as MM
    c, e = MM.centre(x, 'bf16'), MM.e32(x, 'bf16')
    return c - e, c + e


def exempt_blocks(c):
    """[M, N / 32] mask: the blocks built to sit on a decision (pure rows of the tie and power-of-two families)"""
    ex = np.isin(c['family'], [FAMILIES.index(n) for n in EXEMPT])
    return c['pure'][:, None] & ex[None, :]


GELU_ARGMIN = -0.7517916                # GELU's one extremum: its minimum -0.16997


def gauss_interval(pre, b):
    """[lo, hi] for gelu_erf of a float32 pre-activation known as pre +- b (float64 arrays): the range of GELU over [pre - b, pre + b] -- its two ends, and the
    minimum where the range holds it -- widened by mlp_model's float32 evaluation error (taken at both ends, the larger one twice)"""
    import mlp_model as MM
    x0, x1 = pre - b, pre + b
    c0, c1 = MM.centre(x0, 'bf16'), MM.centre(x1, 'bf16')
    e = 2.0 * np.maximum(MM.e32(x0, 'bf16'), MM.e32(x1, 'bf16'))
    lo = np.where((x0 < GELU_ARGMIN) & (x1 > GELU_ARGMIN), float(MM.centre(np.array([GELU_ARGMIN]), 'bf16')[0]), np.minimum(c0, c1))
    return lo - e, np.maximum(c0, c1) + e


GAUSS_SHAPES = [(512, 3072, 768), (1280, 3072, 768), (256, 4096, 1024)]          # test_gpu_fp8.py's fc1 cases


def fc1_gauss(M, N, K):
    """B2's operands.  The pre-activation is known to b = 1e-4 sum |a| |w| (the accumulation term of test_gpu_fp8.py's qkv bound).  On zero-mean operands
    sum |a| |w| is about 0.64 sqrt(K) = 18 times the typical |pre|, and b alone then leaves HALF of all codes open (measured on the CPU: 52 % on that file's
    _operands) -- nothing would be decided.  So these Gaussians carry a mean: A = (g + 1.5) 2^k per block (k = -3 .. 3 as there), W[n] = (g + nu_n) s with
    nu_n = +-(0.5 .. 2), the sign alternating by column so that every block of 32 holds both, and s such that pre = +-(1.5 .. 6) (+ noise of 0.3): GELU's curved
    range on both sides, sum |a| |w| about 1.5 |pre|.  -> A, W, bias"""
    rng = np.random.default_rng(M * 3 + N + 1)
    A = ((rng.standard_normal((M, K)) + 1.5) * np.repeat(np.exp2(rng.integers(-3, 4, size=(M, K // 32))), 32, axis=1)).astype(F32)
    nu = np.where(np.arange(N) % 2 == 0, 1.0, -1.0) * rng.uniform(0.5, 2.0, N)
    W = ((rng.standard_normal((N, K)) + nu[:, None]) * (0.88 / K)).astype(F32)
    bias = (rng.standard_normal(N) * 0.1).astype(F32)
    return A, W, bias


# ---------------------------------------------------------------------------------------------------------------- C. the qkv epilogue

C_M, C_N, C_K = 512, 2304, 512


@functools.lru_cache(maxsize=None)
def qkv_exact(mixed):
    """small integers.  A in -3 .. 3 with every block's amax 3 or 2 (one binade: all scale bytes equal); mixed: every block times 1, 2 or 4 (three bytes).
    W in -3 .. 3 with one +-14 per row, so that the packer's scale is 14 / 448 = 2^-5 and every entry times 32 an e4m3 value; integer bias.
    The result is asserted below 2048, where fp16 holds every integer."""
    M, N, K = C_M, C_N, C_K
    rng = np.random.default_rng(77 + mixed)
    A = rng.integers(-3, 4, (M, K)).astype(F32)
    A[:, ::32] = np.where(rng.integers(0, 2, (M, K // 32)) == 1, 3.0, -2.0)
    if mixed:
        A *= np.repeat(np.exp2(rng.integers(0, 3, (M, K // 32))), 32, axis=1).astype(F32)
    W = rng.integers(-3, 4, (N, K)).astype(F32)
    W[np.arange(N), rng.integers(0, K, N)] = np.where(np.arange(N) % 2 == 0, 14.0, -14.0)
    bias = rng.integers(-20, 21, N).astype(F32)
    ref = A.astype(F64) @ W.astype(F64).T + bias
    assert np.abs(ref).max() < 2048 and (ref == np.rint(ref)).all()
    return dict(A=A, W=W, bias=bias, ref=ref.astype(F32))
