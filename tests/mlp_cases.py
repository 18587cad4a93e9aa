"""The seeded problems of the MLP pair's tests (tests/test_mlp_model.py on the CPU, tests/test_gpu_mlp.py on the device).

gelu_sweep(dtype)   M = N = 768, K = 256 (the smallest shape all 13 wide configurations accept: nine 256 x 256 / twelve 192 x 256 tiles of the 8-phase kernel,
                    K % 128 == 0, M % 192 == 0).  W[n, k] holds the 16-bit pattern (n % 256) * 256 + k (NaN and inf -> 0; bf16: below 2^-126 -> 0, the MFMA
                    flushes bf16 subnormals), A[m, :] is one-hot at k = m % 256 with the value s = 1, 2, 1.5 by row block: the accumulator is s w exactly in
                    any order and every 256 x 256 block of the output sees every pattern.  Bias by column block: 0 | seeded in (-2^-3, 2^-3) (x off the 16-bit
                    grid) | seeded in (-14, 14) (a dense float32 sample of the range where GELU is neither 0 nor x).  x = fl32(s w + b) in numpy float32 is the
                    device's pre-activation bit for bit, without the fold and with a neutral one (mean 0, rstd 1, ln_s 0).
SHAPES              fc1 [M, 4D, D] and fc2 [M, D, 4D] at M = 768 (4 crops) for D = 384, 768, 1024, 1280 (ViTPose-S, -B, -L, -H).
REFUSED             every (GEMM, D, variant) that the launchers refuse at these shapes, with the rule that refuses it; everything else must run.
transport(dtype)    M = N = K = 768, W = I: A = nine 256 x 256 blocks, each a seeded permutation of every admissible 16-bit pattern."""
import functools

import numpy as np

import ln_consumer_cases as LC
import ln_consumer_model as LM
import residual_row_model as RM

F32, F64 = np.float32, np.float64
DTYPES = LC.DTYPES
PERS, OUTB, AB, REV = 1, 2, 4, 8

# (label, variant, flags): tests/test_gpu_ln_consumer.py::CONFIGS / test_gpu_gemm_cfgs.py::test_wide_gemm_configurations
WIDE = [('cfg9', 9, 0), ('cfg1', 1, 0), ('cfg8', 8, 0), ('cfg8 persistent', 8, PERS), ('cfg11', 11, 0), ('gemm8 256x256', 16, 0), ('gemm8 192x256', 18, 0),
        ('cfg8 reversed', 8, REV), ('cfg12 4-stage ring', 12, 0), ('cfg30 two k-blocks per barrier', 30, 0), ('cfg31 32x64 tiles', 31, 0),
        ('cfg20 192x128, 3-stage ring', 20, 0), ('cfg3 256x256', 3, 0)]
# (label, variant): test_gpu_gemm_cfgs.py::_residual_gemm_configurations; group_m = 8 on the 8-phase tiles, 0 elsewhere
RESID = [('cfg11', 11), ('cfg8', 8), ('cfg9', 9), ('gemm8 256x192', 17), ('gemm8 256x256', 16), ('gemm8 192x256', 18), ('cfg12 4-stage ring', 12),
         ('cfg15 128x64 tiles', 15), ('cfg30 two k-blocks per barrier', 30), ('cfg31 32x64 tiles', 31), ('cfg41 96x64 tiles', 41),
         ('cfg20 192x128, 3-stage ring', 20), ('cfg3 256x256', 3)]
# (the four GELU sites among WIDE: the staged 2-phase epilogue of every gemm.hip tile, the persistent kernel, gemm8's register-direct epilogue on its two tiles)


def group_m(variant):
    return 8 if 16 <= variant <= 18 else 0


M = 768
SHAPES = {D: {'fc1': (M, 4 * D, D), 'fc2': (M, D, 4 * D)} for D in (384, 768, 1024, 1280)}
MODELS = {384: ('ViTPose-S', 1), 768: ('ViTPose-B', 256), 1024: ('ViTPose-L', 64), 1280: ('ViTPose-H', 128)}        # D -> (name, the batch of its BASELINE configuration)

# (GEMM, D, variant) -> the rule of gemm8.hip::gemm8_shape_ok that refuses it (gemm_launch hands the 8-phase ids to gemm8_launch).  fc1 (N = 4D: a multiple of
# 256 for every model, 18 tiles and more) is refused nowhere; fc2's N = D is what the 8-phase tiles do not always divide.
REFUSED = {
    ('fc2', 384, 17): 'M / 256 * N / 192 = 3 x 2 = 6 tiles < 8',
    ('fc2', 384, 16): 'N % 256 != 0',
    ('fc2', 384, 18): 'N % 256 != 0',
    ('fc2', 1024, 17): 'N % 192 != 0',
    ('fc2', 1280, 17): 'N % 192 != 0',
}


def r16(x, dtype):
    return RM.from_bits(RM.to_bits(np.asarray(x, F32), dtype), dtype)


# ---------------------------------------------------------------------------------------------------------------- A. the GELU sweep

def patterns(dtype):
    """the float32 value of each 16-bit pattern 0 .. 65535 as the sweep uses it: NaN, inf (and bf16 subnormals) -> 0"""
    v = RM.from_bits(np.arange(65536, dtype=np.uint32).astype(np.uint16), dtype)
    v = np.where(np.isfinite(v), v, F32(0))
    if dtype == 'bf16':
        v = np.where(np.abs(v) < F32(2.0 ** -126), F32(0), v)
    return v.astype(F32)


@functools.lru_cache(maxsize=None)
def gelu_sweep(dtype):
    """dict: A [768, 256], W [768, 256], bias [768], x [768, 768] (float32 pre-activations; inf where bf16's s w overflows), s [768], finite (mask),
    n_overflow (the count of non-finite x the construction gives, from the patterns' bits alone), neutral (rowstat, ln_s)"""
    Mm = N = 768
    K = 256
    pat = patterns(dtype)
    W = pat[(np.arange(N)[:, None] % 256) * 256 + np.arange(K)[None, :]]
    s = np.repeat(np.array([1.0, 2.0, 1.5], F32), 256)
    A = np.zeros((Mm, K), F32)
    A[np.arange(Mm), np.arange(Mm) % 256] = s
    rng = np.random.default_rng(2024 + (dtype == 'bf16'))
    bias = np.concatenate([np.zeros(256), rng.uniform(-2.0 ** -3, 2.0 ** -3, 256), rng.uniform(-14.0, 14.0, 256)]).astype(F32)
    w = W[:, np.arange(Mm) % 256].T                                        # w[m, n] = W[n, m % 256]
    with np.errstate(over='ignore'):
        x = ((s[:, None] * w).astype(F32) + bias[None, :]).astype(F32)     # s w is exact in float32 (at most 13 significant bits); ONE rounding in the add
    n_overflow = 0
    if dtype == 'bf16':
        # |w| = 2^127 (1 + f / 128): 2 w overflows for every f (2 x 128 patterns), 1.5 w where 1.5 (1 + f / 128) >= 2, f >= 43 (2 x 85); the bias (|b| < 14) is
        # far below half an ulp of 2^127 and moves nothing; each pattern stands once in every column block of a row block
        n_overflow = 3 * (2 * 128 + 2 * 85)
    return dict(A=A, W=W, bias=bias, x=x, s=s, finite=np.isfinite(x), n_overflow=n_overflow,
                neutral=(np.stack([np.zeros(Mm, F32), np.ones(Mm, F32)], 1), np.zeros(N, F32)))


def dense_grid(n=1 << 20):
    """a dense float32 grid of [-14, 14]"""
    return np.linspace(-14.0, 14.0, n).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- B. the model widths

def _cycle(idx, n):
    return np.resize(np.asarray(idx), n)


@functools.lru_cache(maxsize=None)
def fc1_rows(dtype, D):
    """(row index into LC.rows, family per row, A [M, D] = the hi plane, partials [M, D / 64, 2]): every case row in turn, the non-Gaussian ones on the first and
    last row of every 32-row block (as test_gpu_ln_consumer.py::_fold_problem places them), the zero row at 0, 191, 192 and M - 1"""
    R, P = LC.rows(dtype, D), LC.partials(dtype, D)
    idx = _cycle(np.arange(len(P)), M)
    edge = [i for i, f in enumerate(R['family']) if f != 'gauss']
    spots = [m for m in range(M) if m % 32 in (0, 31)]
    idx[spots] = _cycle(edge, len(spots))
    idx[[0, 191, 192, M - 1]] = LC.family_rows(dtype, D, ('const0',))[0]
    return idx, np.array(R['family'])[idx], RM.from_bits(R['hi'], dtype)[idx], P[idx]


@functools.lru_cache(maxsize=None)
def fc1_weights(dtype, D, scale=0.05):
    """W' [4D, D] with an asymmetric structure (row sums far from 0, of both signs), its float32 row sums ln_s, a bias"""
    N = 4 * D
    rng = np.random.default_rng(5000 + D + (dtype == 'bf16'))
    W = r16((rng.standard_normal((N, D)) * scale + 0.4 * scale * (np.arange(N)[:, None] % 5 - 1)).astype(F32), dtype)
    return W, W.astype(F64).sum(1).astype(F32), (rng.standard_normal(N) * 0.3).astype(F32)


@functools.lru_cache(maxsize=None)
def fc2_problem(dtype, D):
    """A [M, 4D] = round16(GELU(1.5 g)): hid's own distribution (skewed, a mass in [-0.17, 0], -0 entries from the far negative tail), W [D, 4D] = 0.03 g
    rounded, a bias, a residual 2 g (float32: the tap splits it into the two planes)"""
    K = 4 * D
    rng = np.random.default_rng(7000 + D + (dtype == 'bf16'))
    A = r16(LM.gelu64(1.5 * rng.standard_normal((M, K))).astype(F32), dtype)
    A[::7, ::5] = np.where(A[::7, ::5] <= 0, F32(-0.0), A[::7, ::5])       # GELU's tail rounds to -0: keep some in whatever the draw gave
    W = r16((rng.standard_normal((D, K)) * 0.03).astype(F32), dtype)
    bias = (rng.standard_normal(D) * 0.1).astype(F32)
    resid = (rng.standard_normal((M, D)) * 2.0).astype(F32)
    return A, W, bias, resid


# ---------------------------------------------------------------------------------------------------------------- C. transport

def transport_patterns(dtype):
    """the admissible patterns: every finite fp16 one; bf16: 0 and 2^-40 <= |v| <= 2^40 (the granule M2 stays finite, as residual_row_cases keeps it)"""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    with np.errstate(invalid='ignore'):                                    # the signalling NaNs among the patterns
        v = RM.from_bits(bits, dtype).astype(F64)
    ok = np.isfinite(v)
    if dtype == 'bf16':
        ok &= (v == 0) | ((np.abs(v) >= 2.0 ** -40) & (np.abs(v) <= 2.0 ** 40))
    return bits[ok]


@functools.lru_cache(maxsize=None)
def transport(dtype):
    """dict: bits [768, 768] uint16 (block (i, j) = a seeded permutation of the admissible patterns, cycled to 65536), A (their float32 values), W = I"""
    pats = transport_patterns(dtype)
    bits = np.empty((768, 768), np.uint16)
    for i in range(3):
        for j in range(3):
            rng = np.random.default_rng(31 + 3 * i + j + 100 * (dtype == 'bf16'))
            p = np.resize(pats, 65536)                                     # fp16: 63488 finite patterns, the first 2048 twice
            bits[256 * i:256 * i + 256, 256 * j:256 * j + 256] = rng.permutation(p).reshape(256, 256)
    return dict(bits=bits, A=RM.from_bits(bits, dtype), W=np.eye(768, dtype=F32))


def where_from(bits, got_bits, m, n):
    """for a message: the (block, row, column) places at which A holds the pattern found at (m, n)"""
    hits = np.argwhere(bits == got_bits[m, n])
    return [((int(a) // 256, int(b) // 256), int(a) % 256, int(b) % 256) for a, b in hits[:4]]


def misplaced(bits, got_bits, dtype):
    """None where got == A as values everywhere and as bits wherever the value is not zero (a zero may lose its sign to the +0 partial products); else the
    message: how many elements, the first (m, n), what was expected there, what was found and where A holds that pattern"""
    v, g = RM.from_bits(bits, dtype), RM.from_bits(got_bits, dtype)
    wrong = np.where(v == 0, g != 0, got_bits != bits)
    if not wrong.any():
        return None
    m, n = (int(i) for i in np.argwhere(wrong)[0])
    return (f'{int(wrong.sum())} elements are not where A holds them; first at (m, n) = ({m}, {n}) = block ({m // 256}, {n // 256}) row {m % 256} column {n % 256}: '
            f'expected pattern {int(bits[m, n]):#06x}, found {int(got_bits[m, n]):#06x}, which A holds at (block, row, column) {where_from(bits, got_bits, m, n)}')
