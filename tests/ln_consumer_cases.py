"""The seeded row families of the LayerNorm consumer tests (tests/test_ln_consumer_model.py on the CPU, tests/test_gpu_ln_consumer.py on the device): rows of
the two-plane residual stream, v = hi + lo with both planes in the operand type (split as the producers split, tests/residual_row_model.py), for
D = 384, 768, 1024, 1280 (6, 12, 16, 20 granules: the four ln_merge_row instantiations) and D = 256, 128 (the generic ln_merge loop).

Families (rows(dtype, D)['family'][i] names the family of row i):
    gauss            N(0, sigma), sigma = 1, 2, 1/2: the baseline
    offset8 / offset64 / offset1000     +-c + N(0, 1): rstd (acc - mean s) cancels log2(c) bits
    const0           the zero row: every formula is exact, rstd = rsqrt(eps) = 1e3, and the fold returns the bias
    const            one value on the whole row (1, -3.140625, 1000.5): variance 0; the between-granule term is only what mean's own rounding leaves
    sigma1e-4 / sigma1e-3               N(0, sigma): the variance is 1 % of eps / eps itself
    outlier          N(0, 1) and one 3000 (first granule, a middle one, the last column)
    granconst        constant within each granule, the granule means +-500 (unevenly): every M2_g is 0, only the between-granule term is not
    granconst_noise  the same + N(0, 0.1)
    limit            fp16: uniform over +-65504 and a row of +-65504 alone; bf16: 1e5 + N(0, 1) and -3e4 + N(0, 1) (the offsets of the producer test)
NaN and inf inputs are out of scope: every value here is finite, and so is every statistic."""
import functools

import numpy as np

import ln_consumer_model as LM
import residual_row_model as RM

F32 = np.float32
DS = (384, 768, 1024, 1280, 256, 128)
DTYPES = ('fp16', 'bf16')
FAMILIES = ('gauss', 'offset8', 'offset64', 'offset1000', 'const0', 'const', 'sigma1e-4', 'sigma1e-3', 'outlier', 'granconst', 'granconst_noise', 'limit')
NEUTRAL = ('gauss', 'const0', 'const', 'sigma1e-4', 'sigma1e-3')         # mean near 0 or variance 0: dropped where the statistics must be far from neutral


@functools.lru_cache(maxsize=None)
def rows(dtype, D):
    """dict: v [R, D] float32 (= hi + lo exactly), hi / lo bits [R, D], family (list of R names)"""
    rng = np.random.default_rng(D * 2 + (dtype == 'bf16'))
    T = D // 64
    out, fam = [], []

    def add(name, x):
        out.append(np.asarray(x, np.float64))
        fam.append(name)

    for s in (1.0, 2.0, 0.5):
        add('gauss', rng.standard_normal(D) * s)
    for c in (8.0, 64.0, 1000.0):
        for sign in (1.0, -1.0):
            add(f'offset{int(c)}', sign * c + rng.standard_normal(D))
    add('const0', np.zeros(D))
    for c in (1.0, -3.140625, 1000.5):
        add('const', np.full(D, c))
    add('sigma1e-4', rng.standard_normal(D) * 1e-4)
    add('sigma1e-3', rng.standard_normal(D) * 1e-3)
    for pos in (5, (T // 2) * 64 + 17, D - 1):
        x = rng.standard_normal(D)
        x[pos] = 3000.0
        add('outlier', x)
    for k in range(2):
        sg = np.where(rng.random(T) < 0.7, 1.0, -1.0)
        sg[k % T] = -1.0
        sg[(k + 1) % T] = 1.0                                  # both signs present, unevenly: the row mean is not 0
        gc = np.repeat(500.0 * sg, 64)
        add('granconst', gc)
        add('granconst_noise', gc + rng.standard_normal(D) * 0.1)
    if dtype == 'fp16':
        add('limit', rng.uniform(-65504.0, 65504.0, D))
        add('limit', np.where(rng.random(D) < 0.6, 65504.0, -65504.0))
    else:
        add('limit', 1e5 + rng.standard_normal(D))
        add('limit', -3e4 + rng.standard_normal(D))
    x = np.stack(out).astype(F32)
    _, hi, lo = RM.split(x, dtype)
    v = RM.decode(hi, lo, dtype)
    assert np.array_equal(v.astype(np.float64), RM.from_bits(hi, dtype).astype(np.float64) + RM.from_bits(lo, dtype).astype(np.float64))   # hi + lo is exact in float32
    return dict(v=v, hi=hi, lo=lo, family=fam)


def family_rows(dtype, D, names):
    return [i for i, f in enumerate(rows(dtype, D)['family']) if f in names]


@functools.lru_cache(maxsize=None)
def partials(dtype, D):
    """the float64 granule statistics of the stored rows, rounded to float32: [R, D / 64, 2]"""
    return LM.partials_fp64(rows(dtype, D)['v'])


def handmade_partials(T):
    """Partials no producer emits exactly but a merge must still handle, [R, T, 2] with their names: M2_g = 0 under unequal sums (a many-bit float32 each),
    one granule carrying all the variance, all zero."""
    rng = np.random.default_rng(900 + T)
    P, names = [], []
    for scale in (1.0, 3000.0):
        p = np.zeros((T, 2))
        p[:, 0] = rng.standard_normal(T) * 64.0 * scale + 17.0 * scale
        P.append(p)
        names.append('m2_zero_unequal_sums')
    for g in (0, T - 1):
        p = np.zeros((T, 2))
        p[:, 0] = 64.0 * 2.5
        p[g, 1] = 12345.678
        P.append(p)
        names.append('one_granule_variance')
    P.append(np.zeros((T, 2)))
    names.append('all_zero')
    return np.stack(P).astype(F32), names
