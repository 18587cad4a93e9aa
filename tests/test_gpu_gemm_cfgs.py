"""GPU: every PRODUCTION GEMM configuration launched directly (vp_dbg_gemm_case) at M = 192 x 64 token rows against an fp64
reference of the same rounded operands -- 192x128 tiles with 4 and 8 waves (Cfg8 / Cfg11), the persistent workgroups, the
8-phase kernels of gemm8.hip (256x256 / 256x192, end-of-tile and deferred epilogue), the LayerNorm-consumer fold, the
LayerNorm-producer epilogue with its row statistics, the 64x64-blocked `hid` layout on both sides, the reversed tile walk and
the hi+lo final 1x1 conv -- and bit identity between the configurations of one GEMM (same accumulation order by construction:
any difference is a schedule bug or a race).  VERDICT r1 item 6: these kernels used to be validated only transitively.
The dispatch of the tiles is generated from csrc/tiles.h, so every product tile (1, 3, 8, 9, 11, 12, 15, 20, 30, 31, 41) is launched once per epilogue
class here, and the two configuration matrices also run on bf16.
The data here are Gaussians and the residual taps return hi + lo summed: the edge values of the residual producer row (the fp16 clamp, fp16 subnormals and signed zeros in the
planes, rows with a large common offset, the association st + (hi + lo), the in-place update) and the planes and statistics bit for bit against a host model live in
tests/test_gpu_residual_row.py.  GELU over its whole domain (saturation, the negative tail, fp16-subnormal outputs, x off the 16-bit grid) at every site, fc1 and fc2
per element at every model's widths (D = 384 / 1024 / 1280 beside the 768 of this file) and the blocked hand-over by position live in tests/test_gpu_mlp.py."""
import ctypes as C

import numpy as np
import pytest

from easy_vitpose_amd import _capi as capi
from helpers import round_to

pytestmark = pytest.mark.gpu

M, D = 192 * 64, 768
PERS, OUTB, AB, REV = 1, 2, 4, 8


def _case(epi, variant, flags, A, W, bias, aux=None, rowstat=None, ln_s=None, group_m=8, want_stats=False, out_shape=None, dtype='fp16'):
    lib = capi.load_library()
    m, k = A.shape
    n = W.shape[0]
    out = np.empty(out_shape or (m, n), dtype=np.float32)
    stats = np.empty((m, n // 64, 2), dtype=np.float32) if want_stats else None
    p = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32).ctypes.data
    keep = [np.ascontiguousarray(a, dtype=np.float32) if a is not None else None for a in (A, W, bias, aux, rowstat, ln_s)]
    rc = lib.vp_dbg_gemm_case(0, capi.DTYPES[dtype], epi, variant, group_m, flags, m, n, k,
                              *[None if a is None else a.ctypes.data for a in keep], out.ctypes.data,
                              None if stats is None else stats.ctypes.data)
    assert rc == 0, capi.last_error()
    return (out, stats) if want_stats else out


def _gelu(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


@pytest.fixture(scope='module')
def operands():
    rng = np.random.default_rng(0)
    A = round_to(rng.standard_normal((M, D)).astype(np.float32), 'fp16')
    return rng, A


# the bf16 matrices run at 40 crops: still a multiple of 256 rows, more than 256 tiles of 256 x 256 (workgroups of the 8-phase kernel with one and with two tiles: 30 x 9)
# and more than the 512 resident workgroups of the persistent 192 x 128 kernel (40 x 18), and the 25-crop sub-case fits; each case stays at a few seconds
M_BF16 = 192 * 40


@pytest.fixture(scope='module')
def operands_bf16():
    rng = np.random.default_rng(1)
    A = round_to(rng.standard_normal((M_BF16, D)).astype(np.float32), 'bf16')
    return rng, A


ULP = {'fp16': 2.0 ** -10, 'bf16': 2.0 ** -7}


def _check16(got, ref, what, dtype='fp16'):
    err = np.abs(got - ref)
    tol = ULP[dtype] * np.abs(ref) + 2e-4            # one 16-bit rounding of the output + fp32 accumulation order
    assert (err <= tol).all(), f'{what}: max err {err.max():.3e} (worst ratio {(err / tol).max():.2f})'


WIDE = [('qkv', 3 * D, 0, 0), ('fc1', 4 * D, 1, OUTB)]


@pytest.mark.parametrize('name,N,epi,flags', WIDE)
def test_wide_gemm_configurations(operands, name, N, epi, flags):
    """LayerNorm-consumer fold + bias (+ GELU, + blocked output): fp64 reference, then bit identity of all configurations."""
    _wide_gemm_configurations(operands, name, N, epi, flags, 'fp16')


@pytest.mark.parametrize('name,N,epi,flags', WIDE)
def test_wide_gemm_configurations_bf16(operands_bf16, name, N, epi, flags):
    """The same matrix on bf16 operands (the BF16 instantiations of every configuration): fp64 reference at bf16's output rounding 2^-7, bit identity of all
    configurations, and every configuration run twice: equal bit for bit."""
    _wide_gemm_configurations(operands_bf16, name, N, epi, flags, 'bf16')


def _wide_gemm_configurations(operands, name, N, epi, flags, dtype):
    rng, A = operands
    M = A.shape[0]
    W = round_to((rng.standard_normal((N, D)) * 0.05).astype(np.float32), dtype)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    rowstat = np.stack([rng.standard_normal(M) * 0.2, 1.0 + 0.3 * rng.random(M)], 1).astype(np.float32)
    ln_s = W.astype(np.float64).sum(1).astype(np.float32)
    acc = A.astype(np.float64) @ W.astype(np.float64).T
    ref = (acc - rowstat[:, :1].astype(np.float64) * ln_s.astype(np.float64)) * rowstat[:, 1:].astype(np.float64) + bias
    if epi == 1:
        ref = _gelu(ref)
    outs = {}
    for label, variant, fl in [('cfg9', 9, 0), ('cfg1', 1, 0), ('cfg8', 8, 0), ('cfg8 persistent', 8, PERS), ('cfg11', 11, 0),
                               ('gemm8 256x256', 16, 0), ('gemm8 192x256', 18, 0), ('cfg8 reversed', 8, REV),
                               ('cfg12 4-stage ring', 12, 0), ('cfg30 two k-blocks per barrier', 30, 0), ('cfg31 32x64 tiles', 31, 0),
                               ('cfg20 192x128, 3-stage ring', 20, 0), ('cfg3 256x256', 3, 0)]:
        outs[label] = _case(epi, variant, flags | fl, A, W, bias, rowstat=rowstat, ln_s=ln_s, dtype=dtype)
        _check16(outs[label], ref, f'{name} {label}', dtype)
        if dtype == 'bf16':
            again = _case(epi, variant, flags | fl, A, W, bias, rowstat=rowstat, ln_s=ln_s, dtype=dtype)
            assert np.array_equal(again, outs[label]), f'{name}: {label} is not run-to-run identical ({(again != outs[label]).sum()} elements)'
    base = outs['cfg9']
    for label, o in outs.items():
        assert np.array_equal(o, base), f'{name}: {label} differs from cfg9 in {(o != base).sum()} elements'
    # without the fold (plain bias): the neutral-operand path of every kernel
    plain = A.astype(np.float64) @ W.astype(np.float64).T + bias
    if epi == 1:
        plain = _gelu(plain)
    for label, variant, fl in [('cfg8 persistent', 8, PERS), ('gemm8', 16, 0), ('gemm8 192x256', 18, 0)]:
        _check16(_case(epi, variant, flags | fl, A, W, bias, dtype=dtype), plain, f'{name} {label} (no fold)', dtype)
    # a row count only the 192-row tile divides (25 crops = 4800 rows: 25 x 9 / 25 x 12 tiles, workgroups with one and with two tiles; blocked output
    # rows that straddle 64-row blocks): bit for bit the 2-phase kernel
    r = 192 * 25
    a = _case(epi, 18, flags, A[:r], W, bias, rowstat=rowstat[:r], ln_s=ln_s, dtype=dtype)
    b = _case(epi, 9, flags, A[:r], W, bias, rowstat=rowstat[:r], ln_s=ln_s, dtype=dtype)
    assert np.array_equal(a, b), f'{name}: 192 x 256 tiles at {r} rows differ from cfg9 in {(a != b).sum()} elements'
    assert np.array_equal(a, base[:r])


RESID = [('proj', D, 0), ('fc2', 4 * D, AB | REV)]


@pytest.mark.parametrize('name,K,flags', RESID)
def test_residual_gemm_configurations(operands, name, K, flags):
    """bias + two-plane residual + LayerNorm row statistics (EPI_BIAS_RESID_LN): output planes and the per-granule
    (sum, centred M2) statistics against fp64; bit identity across tile configurations incl. the 8-phase kernels."""
    _residual_gemm_configurations(operands, name, K, flags, 'fp16')


@pytest.mark.parametrize('name,K,flags', RESID)
def test_residual_gemm_configurations_bf16(operands_bf16, name, K, flags):
    """The same matrix on bf16 operands and bf16 residual planes: the fp64 comparison keeps the fp16 bounds (the planes hold x to 2^-18 |x| = 3.8e-6 |x|, inside
    2e-5 max|ref|; a granule's 64 values sum to |x| of about 115, so the planes' rounding moves its sum by at most 115 x 2^-18 = 4.4e-4 < 2e-3 and its M2 by a
    few 1e-3 against a bound of 2e-3 x ~300), bit identity across configurations, every configuration run twice: equal bit for bit."""
    _residual_gemm_configurations(operands_bf16, name, K, flags, 'bf16')


def _residual_gemm_configurations(operands, name, K, flags, dtype):
    rng, A0 = operands
    M = A0.shape[0]
    A = round_to((rng.standard_normal((M, K)) * (1.0 if K == D else 0.5)).astype(np.float32), dtype)
    W = round_to((rng.standard_normal((D, K)) * 0.03).astype(np.float32), dtype)
    bias = (rng.standard_normal(D) * 0.1).astype(np.float32)
    resid = (rng.standard_normal((M, D)) * 2.0).astype(np.float32)
    hi = round_to(resid, dtype)
    x0 = hi.astype(np.float64) + round_to(resid - hi, dtype).astype(np.float64)          # what the two planes hold
    ref = A.astype(np.float64) @ W.astype(np.float64).T + bias + x0
    outs = {}
    for label, variant in [('cfg11', 11), ('cfg8', 8), ('cfg9', 9), ('gemm8 256x192', 17), ('gemm8 256x256', 16), ('gemm8 192x256', 18),
                           ('cfg12 4-stage ring', 12), ('cfg15 128x64 tiles', 15), ('cfg30 two k-blocks per barrier', 30), ('cfg31 32x64 tiles', 31),
                           ('cfg41 96x64 tiles', 41), ('cfg20 192x128, 3-stage ring', 20), ('cfg3 256x256', 3)]:
        gm = 8 if 16 <= variant <= 18 else 0
        o, st = _case(6, variant, flags, A, W, bias, aux=resid, want_stats=True, group_m=gm, dtype=dtype)
        outs[label] = (o, st)
        if dtype == 'bf16':
            o2, st2 = _case(6, variant, flags, A, W, bias, aux=resid, want_stats=True, group_m=gm, dtype=dtype)
            assert np.array_equal(o2, o) and np.array_equal(st2, st), f'{name}: {label} is not run-to-run identical'
        assert np.abs(o - ref).max() < 2e-5 * max(1.0, np.abs(ref).max()), f'{name} {label}: planes off by {np.abs(o - ref).max():.3e}'
        g = o.astype(np.float64).reshape(M, D // 64, 64)                                    # statistics of the STORED values
        assert np.abs(st[..., 0] - g.sum(-1)).max() < 2e-3, f'{name} {label}: granule sums'
        m2 = ((g - g.mean(-1, keepdims=True)) ** 2).sum(-1)
        assert np.abs(st[..., 1] - m2).max() < 2e-3 * max(1.0, m2.max()), f'{name} {label}: granule M2'
    bo, bs = outs['cfg11']
    for label, (o, st) in outs.items():
        assert np.array_equal(o, bo) and np.array_equal(st, bs), f'{name}: {label} differs from cfg11'
    if K == D:
        # the ragged last m-tile of the 256 x 256 tile at its smallest: 576 rows = 3 crops = two full tiles + 64 rows, N = K = 768; bit for bit cfg9 on the same rows
        r = 576
        o3, s3 = _case(6, 3, flags, A[:r], W, bias, aux=resid[:r], want_stats=True, group_m=0, dtype=dtype)
        o9, s9 = _case(6, 9, flags, A[:r], W, bias, aux=resid[:r], want_stats=True, group_m=0, dtype=dtype)
        assert np.array_equal(o3, o9) and np.array_equal(s3, s9), f'{name}: cfg3 at {r} rows differs from cfg9 in {(o3 != o9).sum()} elements'
        assert np.array_equal(o3, bo[:r]) and np.array_equal(s3, bs[:r])


@pytest.mark.parametrize('name,K,Dm,rows', [('fc2 ViTPose-L x 8', 4096, 1024, 192 * 8), ('fc2 ViTPose-B x 1', 3072, 768, 192), ('proj ViTPose-H x 4', 1280, 1280, 192 * 4),
                                            ('fc2 ViTPose-S x 3', 1536, 384, 192 * 3)])
def test_split_k_residual_gemm(name, K, Dm, rows):
    """Round 6, small batches: a residual GEMM as S partial products over k ranges (gemm.hip EPI_PARTIAL) + the fixed-order reduction kernel
    (elementwise.hip splitk_reduce_kernel).  Planes and granule statistics against fp64 at the tolerance of the one-launch epilogue; every (S, tile)
    combination run-to-run BIT-IDENTICAL (the reduction adds the partials in the order s = 0 .. S - 1: no atomics); all tiles of one S agree bit for bit
    (same k order inside a range, same reduction); against the unsplit kernel the planes differ only by the fp32 accumulation order."""
    rng = np.random.default_rng(K + rows)
    A = round_to((rng.standard_normal((rows, K)) * (1.0 if K == Dm else 0.5)).astype(np.float32), 'fp16')
    W = round_to((rng.standard_normal((Dm, K)) * 0.03).astype(np.float32), 'fp16')
    bias = (rng.standard_normal(Dm) * 0.1).astype(np.float32)
    resid = (rng.standard_normal((rows, Dm)) * 2.0).astype(np.float32)
    flags = 0 if K == Dm else AB
    hi = round_to(resid, 'fp16')
    x0 = hi.astype(np.float64) + round_to(resid - hi, 'fp16').astype(np.float64)
    ref = A.astype(np.float64) @ W.astype(np.float64).T + bias + x0
    base, _ = _case(6, 12, flags, A, W, bias, aux=resid, want_stats=True, group_m=0)
    for S in (2, 4, 8):
        if K % (S * 128):
            continue
        per_s = {}
        for variant in (12, 1, 11, 15, 20, 30, 31):
            o, st = _case(6, variant, flags | (S << 8), A, W, bias, aux=resid, want_stats=True, group_m=0)
            o2, st2 = _case(6, variant, flags | (S << 8), A, W, bias, aux=resid, want_stats=True, group_m=0)
            assert np.array_equal(o, o2) and np.array_equal(st, st2), f'{name}: split-K {S} on cfg{variant} is not run-to-run deterministic'
            assert np.abs(o - ref).max() < 2e-5 * max(1.0, np.abs(ref).max()), f'{name} S={S} cfg{variant}: planes off by {np.abs(o - ref).max():.3e}'
            g = o.astype(np.float64).reshape(rows, Dm // 64, 64)
            assert np.abs(st[..., 0] - g.sum(-1)).max() < 2e-3, f'{name} S={S} cfg{variant}: granule sums'
            m2 = ((g - g.mean(-1, keepdims=True)) ** 2).sum(-1)
            assert np.abs(st[..., 1] - m2).max() < 2e-3 * max(1.0, m2.max()), f'{name} S={S} cfg{variant}: granule M2'
            assert np.abs(o - base).max() < 4e-6 * max(1.0, np.abs(ref).max()), f'{name} S={S} cfg{variant}: further from the unsplit kernel than an accumulation order explains'
            per_s[variant] = (o, st)
        o0, s0 = per_s[12]
        for variant, (o, st) in per_s.items():
            assert np.array_equal(o, o0) and np.array_equal(st, s0), f'{name}: split-K {S} on cfg{variant} differs from cfg12'


@pytest.mark.parametrize('K,rows', [(768, 192 * 136), (3072, 192 * 136), (768, 192 * 7)])
def test_residual_gemm_192_row_tiles_across_tile_boundaries(K, rows):
    """The 8-phase kernel's 192 x 256 tile (X halves of 96 rows: uneven DMA piece counts per wave group, register-direct residual
    epilogue, the ring running on across tile boundaries) at a row count where workgroups own ONE OR TWO tiles (136 x 3 = 408 tiles on 256
    workgroups) and at a row count only this tile shape divides (1344 rows = 7 crops: not a multiple of 256): planes and statistics bit for
    bit those of the 2-phase kernel."""
    rng = np.random.default_rng(K + rows)
    A = round_to((rng.standard_normal((rows, K)) * (1.0 if K == D else 0.5)).astype(np.float32), 'fp16')
    W = round_to((rng.standard_normal((D, K)) * 0.03).astype(np.float32), 'fp16')
    bias = (rng.standard_normal(D) * 0.1).astype(np.float32)
    resid = (rng.standard_normal((rows, D)) * 2.0).astype(np.float32)
    flags = 0 if K == D else AB | REV                     # fc2 reads its activations in the 64 x 64-blocked layout fc1 writes
    o11, s11 = _case(6, 11, flags, A, W, bias, aux=resid, want_stats=True, group_m=0)
    for gm in (2, 8):
        o18, s18 = _case(6, 18, flags, A, W, bias, aux=resid, want_stats=True, group_m=gm)
        assert np.array_equal(o18, o11) and np.array_equal(s18, s11), f'192 x 256 tiles (group_m {gm}) differ from cfg11 in {(o18 != o11).sum()} elements'
    # (and the values themselves, on a sample of rows: the bit identity above carries it to all of them)
    idx = rng.choice(rows, 64, replace=False)
    hi = round_to(resid[idx], 'fp16')
    x0 = hi.astype(np.float64) + round_to(resid[idx] - hi, 'fp16').astype(np.float64)
    ref = A[idx].astype(np.float64) @ W.astype(np.float64).T + bias + x0
    assert np.abs(o11[idx] - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


def test_patch_embed_epilogue_with_statistics(operands):
    """EPI_POS_LN: + pos[m % 192], two-plane output, row statistics."""
    rng, A = operands
    W = round_to((rng.standard_normal((D, D)) * 0.02).astype(np.float32), 'fp16')
    pos = (rng.standard_normal((192, D)) * 0.5).astype(np.float32)
    bias = np.zeros(D, np.float32)
    ref = A.astype(np.float64) @ W.astype(np.float64).T + np.tile(pos.astype(np.float64), (M // 192, 1))
    first = None
    for variant in (8, 11, 9, 12, 30, 31):
        o, st = _case(7, variant, 0, A, W, bias, aux=pos, want_stats=True, group_m=0)
        assert np.abs(o - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
        g = o.astype(np.float64).reshape(M, D // 64, 64)
        assert np.abs(st[..., 0] - g.sum(-1)).max() < 2e-3
        if first is None:
            first = (o, st)
        assert np.array_equal(o, first[0]) and np.array_equal(st, first[1]), f'patch embed: cfg{variant} differs from cfg8'


@pytest.mark.parametrize('kp', [17, 133])
def test_final_conv_hi_lo_weights(kp):
    """EPI_HEATMAP: final 1x1 conv with hi+lo 16-bit weight pairs -> fp32 NCHW heatmaps; only the activations are rounded."""
    rng = np.random.default_rng(kp)
    B = 4
    A = round_to(np.maximum(rng.standard_normal((B * 3072, 256)), 0).astype(np.float32), 'fp16')
    W = (rng.standard_normal((kp, 256)) * 0.02).astype(np.float32)
    bias = (rng.standard_normal(kp) * 0.02).astype(np.float32)
    ref = (A.astype(np.float64) @ W.astype(np.float64).T + bias).reshape(B, 3072, kp).transpose(0, 2, 1)
    for variant in (8, 1, 9, 12, 30, 31):
        o = _case(5, variant, 0, A, W, bias, group_m=0, out_shape=(B, kp, 3072))
        assert np.abs(o - ref).max() < 3e-6 * max(1.0, np.abs(ref).max()), f'heatmap cfg{variant}: {np.abs(o - ref).max():.3e}'
