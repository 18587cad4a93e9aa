"""GPU: the consumer half of the fused LayerNorm -- ln_merge in ln_finalize_kernel / ln_finalize_kernel_t, in the 2-phase GEMM prologue (GemmArgs::ln_part) and in
ln_quant_kernel; ln_fold in the epilogues of gemm.hip, gemm8.hip and the two fused qkv + attention kernels -- each through a tap of its own, on the row families
of tests/ln_consumer_cases.py (common offsets, constant rows, a variance at eps, one outlier, rows where only the between-granule term is non-zero, the fp16 limit),
against the float32 model of tests/ln_consumer_model.py and against float64, with bounds per row and, for the fold, per element.  tests/test_ln_consumer_model.py
pins the model and the bounds on the CPU and shows the wrong formulas failing them.  NaN and inf inputs are out of scope."""
import functools

import numpy as np
import pytest

import ln_consumer_cases as LC
import ln_consumer_model as LM
import residual_row_model as RM
from easy_vitpose_amd import _capi as capi

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PERS, OUTB = 1, 2


def _c(a, dt=F32):
    return np.ascontiguousarray(a, dtype=dt)


def _bits(a):
    return _c(a).view(np.uint32)


def _finalize(p, D):
    p = _c(p)
    M, T = p.shape[:2]
    out = np.empty((M, 2), F32)
    capi.check(capi.load_library().vp_dbg_ln_finalize(0, M, T, D, p.ctypes.data, out.ctypes.data))
    return out


def _gemm(dtype, epi, variant, flags, A, W, bias, rowstat, ln_s):
    A, W, bias, rowstat, ln_s = (_c(a) for a in (A, W, bias, rowstat, ln_s))
    out = np.empty((A.shape[0], W.shape[0]), F32)
    capi.check(capi.load_library().vp_dbg_gemm_case(0, capi.DTYPES[dtype], epi, variant, 8, flags, A.shape[0], W.shape[0], A.shape[1], A.ctypes.data, W.ctypes.data,
                                                    bias.ctypes.data, None, rowstat.ctypes.data, ln_s.ctypes.data, out.ctypes.data, None))
    return out


def _gemm_lnpart(dtype, epi, variant, flags, A, W, bias, part, ln_s):
    """(return code, out); out keeps its fill where the tap refuses"""
    A, W, bias, part, ln_s = (_c(a) for a in (A, W, bias, part, ln_s))
    out = np.full((A.shape[0], W.shape[0]), 123.0, F32)
    rc = capi.load_library().vp_dbg_gemm_case_lnpart(0, capi.DTYPES[dtype], epi, variant, 8, flags, A.shape[0], W.shape[0], A.shape[1], A.ctypes.data, W.ctypes.data,
                                                     bias.ctypes.data, part.ctypes.data, part.shape[1], ln_s.ctypes.data, out.ctypes.data)
    return rc, out


def _cycle(idx, M):
    return np.resize(np.asarray(idx), M)


def _weights(dtype, N, K, seed, scale=0.05):
    """W' [N, K] with an asymmetric structure (row sums far from 0, of both signs), its float32 row sums, a bias"""
    rng = np.random.default_rng(seed)
    W = RM.from_bits(RM.to_bits((rng.standard_normal((N, K)) * scale + 0.4 * scale * (np.arange(N)[:, None] % 5 - 1)).astype(F32), dtype), dtype)
    return W, W.astype(F64).sum(1).astype(F32), (rng.standard_normal(N) * 0.3).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- a. the merge alone

def _merge_problem(T, M=300):
    D = 64 * T
    P = np.concatenate([LC.partials('fp16', D), LC.partials('bf16', D), LC.handmade_partials(T)[0]])
    V = np.concatenate([LC.rows('fp16', D)['v'], LC.rows('bf16', D)['v']])
    names = LC.rows('fp16', D)['family'] + LC.rows('bf16', D)['family'] + LC.handmade_partials(T)[1]
    idx = _cycle(np.arange(len(P)), M)
    return D, P[idx], V, idx, [names[i] for i in idx]


@pytest.mark.parametrize('T', (2, 4, 6, 12, 16, 20))
def test_merge_alone(T):
    """vp_dbg_ln_finalize on 300 rows (not a multiple of 64 or 256: the last workgroup of either kernel is ragged): the float64 partials of every case row rounded to
    float32, and hand-made partials (M2_g = 0 under unequal sums, one granule with all the variance, all zero).  mean == the model bit for bit; rstd within 2 float32
    ulps of the float64 1 / sqrt of the model's float32 variance (1 ulp for the device's rsqrtf + the final rounding); both inside the float64 bounds."""
    D, P, V, idx, names = _merge_problem(T)
    got = _finalize(P, D)
    mean, rstd, var = LM.merge(P, D)
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got[:, 0]), _bits(mean)), [names[i] for i in np.flatnonzero(_bits(got[:, 0]) != _bits(mean))[:5]]
    ref = 1.0 / np.sqrt(var.astype(F64))
    ulps = np.abs(got[:, 1].astype(F64) - ref) / np.spacing(ref.astype(F32)).astype(F64)
    mr, m2r, rr = LM.merge_fp64(P, D)
    Em, rel = LM.bounds(P, D, mr, m2r, rsqrt_rel=2.0 ** -22)
    r_mean = np.abs(got[:, 0] - mr) / np.where(Em > 0, Em, 1.0)
    r_rstd = np.abs(got[:, 1] - rr) / rr / rel
    rows = idx < len(V)                                                   # the case rows: also against the two-pass statistics of the stored row
    tm, tm2, tr = LM.two_pass_fp64(V[idx[rows]])
    Em2, rel2 = LM.bounds(P[rows], D, tm, tm2, partials_rounded=True, rsqrt_rel=2.0 ** -22)
    r2_mean = np.abs(got[rows, 0] - tm) / np.where(Em2 > 0, Em2, 1.0)
    r2_rstd = np.abs(got[rows, 1] - tr) / tr / rel2
    print(f'[ln consumer] merge T={T}: rstd worst {ulps.max():.2f} ulp of fp64 rsqrt(model var) ({names[int(ulps.argmax())]}); against the bounds: merge identity mean '
          f'{r_mean.max():.3f} rstd {r_rstd.max():.3f}, two-pass mean {r2_mean.max():.3f} rstd {r2_rstd.max():.3f}')
    assert ulps.max() <= 2.0
    assert r_mean.max() <= 1.0 and r_rstd.max() <= 1.0 and r2_mean.max() <= 1.0 and r2_rstd.max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------- b. the merge in the GEMM prologue

@pytest.mark.parametrize('dtype,D', [('fp16', 384), ('fp16', 768), ('fp16', 1024), ('fp16', 1280), ('fp16', 256), ('bf16', 768), ('bf16', 256)])
def test_merge_in_the_gemm_prologue(dtype, D):
    """GemmArgs::ln_part on the 2-phase tiles 9, 8, 11, 31, epi 0 and 1, M = 250 x N = 256 (a ragged last m-tile of every tile height: the prologue's m > M - 1 clamp
    runs): equal BIT FOR BIT to the same kernel fed the rowstat that ln_finalize wrote for the same partials -- common.h's `same ln_merge, same bits`, per kernel."""
    M, N = 250, 256
    R, P = LC.rows(dtype, D), LC.partials(dtype, D)
    idx = _cycle(np.arange(len(P)), M)
    A, part = RM.from_bits(R['hi'], dtype)[idx], P[idx]
    W, ln_s, bias = _weights(dtype, N, D, 40 + D)
    rowstat = _finalize(part, D)
    neutral = np.stack([np.zeros(M, F32), np.ones(M, F32)], 1)
    for epi in (0, 1):
        for variant in (9, 8, 11, 31):
            rc, fused = _gemm_lnpart(dtype, epi, variant, 0, A, W, bias, part, ln_s)
            assert rc == 0, capi.last_error()
            two = _gemm(dtype, epi, variant, 0, A, W, bias, rowstat, ln_s)
            assert np.isfinite(two).all()
            assert np.array_equal(_bits(fused), _bits(two)), f'cfg{variant} epi {epi}: {(_bits(fused) != _bits(two)).sum()} of {two.size} elements differ (rows {np.flatnonzero((_bits(fused) != _bits(two)).any(1))[:8]})'
        assert (two != _gemm(dtype, epi, 9, 0, A, W, bias, neutral, ln_s)).mean() > 0.5        # the statistics are not neutral: the comparison is of the fold


def test_prologue_refusals():
    """What gemm_launch cannot run with partial statistics comes back as an error and launches nothing (out keeps its fill): the 8-phase tiles (their epilogues read
    rowstat only -- at a shape they otherwise accept, and at the 250 rows of the test above), the persistent kernel (no statistics area behind its ring), an odd ln_tiles
    (a row of partials is fetched as 16-byte pieces)."""
    dtype = 'fp16'
    for variant, flags, M, K, T in ((16, 0, 2048, 384, 6), (16, 0, 250, 384, 6), (18, 0, 1536, 384, 6), (8, PERS, 384, 384, 6), (8, PERS, 250, 384, 6), (9, 0, 250, 320, 5)):
        rng = np.random.default_rng(M + K)
        A = RM.from_bits(RM.to_bits(rng.standard_normal((M, K)).astype(F32), dtype), dtype)
        part = np.abs(rng.standard_normal((M, T, 2))).astype(F32)
        W, ln_s, bias = _weights(dtype, 256, K, 7)
        for epi in (0, 1):
            rc, out = _gemm_lnpart(dtype, epi, variant, flags, A, W, bias, part, ln_s)
            assert rc != 0 and 'invalid' in capi.last_error().lower(), (variant, flags, M, K, T, rc, capi.last_error())
            assert (out == 123.0).all()
    # ... and the same shapes run where the launcher can: cfg8 without the persistent flag at 384 rows
    A = RM.from_bits(RM.to_bits(np.random.default_rng(3).standard_normal((384, 384)).astype(F32), dtype), dtype)
    W, ln_s, bias = _weights(dtype, 256, 384, 7)
    rc, out = _gemm_lnpart(dtype, 0, 8, 0, A, W, bias, LM.partials_fp64(A), ln_s)
    assert rc == 0 and np.isfinite(out).all() and (out != 123.0).any()


# ---------------------------------------------------------------------------------------------------------------- c, d. the fold at edge rows

CONFIGS = [('cfg9', 9, 0), ('cfg1', 1, 0), ('cfg8', 8, 0), ('cfg8 persistent', 8, PERS), ('cfg11', 11, 0), ('gemm8 256x256', 16, 0), ('gemm8 192x256', 18, 0),
           ('cfg8 reversed', 8, 8), ('cfg12 4-stage ring', 12, 0), ('cfg30 two k-blocks per barrier', 30, 0), ('cfg31 32x64 tiles', 31, 0),
           ('cfg20 192x128, 3-stage ring', 20, 0), ('cfg3 256x256', 3, 0)]            # the list of test_gpu_gemm_cfgs.py::test_wide_gemm_configurations


@functools.lru_cache(maxsize=None)
def _fold_problem(dtype, D, M=768):
    """A = the hi plane of the case rows: every row in turn, and the non-Gaussian ones again on the first and last row of every 32-row block -- the first and last row
    of every tile height (32 ... 256) and both sides of every crop boundary (rows 191 | 192, ...) hold an edge row; the zero row sits at 0, 191, 192 and 767."""
    R, P = LC.rows(dtype, D), LC.partials(dtype, D)
    idx = _cycle(np.arange(len(P)), M)
    edge = [i for i, f in enumerate(R['family']) if f != 'gauss']
    spots = [m for m in range(M) if m % 32 in (0, 31)]
    idx[spots] = _cycle(edge, len(spots))
    z = LC.family_rows(dtype, D, ('const0',))[0]
    idx[[0, 191, 192, M - 1]] = z
    fam = np.array(R['family'])[idx]
    rowstat = _finalize(P[idx], D)
    return idx, fam, RM.from_bits(R['hi'], dtype)[idx], R['v'][idx], rowstat


def _unit16(ref, dtype):
    """one rounding of a 16-bit output at the magnitude of its row: u16 max(|ref|, the row's rms)"""
    return LM.U16[dtype] * np.maximum(np.abs(ref), np.sqrt((ref ** 2).mean(1, keepdims=True)) + 1e-30)


@pytest.mark.parametrize('dtype', LC.DTYPES)
@pytest.mark.parametrize('D', (384, 1280))
@pytest.mark.parametrize('epi,flags', [(0, 0), (1, OUTB)])
def test_fold_at_edge_rows(dtype, D, epi, flags):
    """ln_fold in every epilogue that carries it, M = 768 x N = 768 (nine 256 x 256 and twelve 192 x 256 tiles: the fewest the 8-phase kernel accepts), K = D = 384 on
    every configuration and 1280 on cfg9 and the 8-phase tiles; statistics of the stored hi + lo from ln_finalize.  Per element against the float64
    rstd (sum hi W' - mean s) + b on the same float32 statistics, bound LM.fold_reference; zero rows return round16(bias) (epi 1: round16(GELU(bias)), as far as the
    fit's 1.2e-6 decides the rounding); all configurations equal bit for bit.  Then against the float64 LayerNorm(hi + lo) W' + b, bound + rstd u16 sum |v||W'|."""
    M = N = 768
    idx, fam, A, V, rowstat = _fold_problem(dtype, D)
    W, ln_s, bias = _weights(dtype, N, D, 70 + D + epi)
    ref, bound, _ = LM.fold_reference(A, W, ln_s, bias, rowstat[:, 0], rowstat[:, 1], epi, dtype)
    assert np.abs(ref).max() < 6e4                                        # nothing saturates the fp16 output
    configs = CONFIGS if D == 384 else [c for c in CONFIGS if c[1] in (9, 16, 18)]
    outs = {}
    for label, variant, fl in configs:
        o = _gemm(dtype, epi, variant, flags | fl, A, W, bias, rowstat, ln_s)
        assert np.isfinite(o).all(), label
        ratio = np.abs(o - ref) / bound
        print(f'[ln consumer] fold {dtype} D={D} epi {epi} {label}: worst |err| / bound {ratio.max():.3f} (row {int(ratio.max(1).argmax())}: {fam[int(ratio.max(1).argmax())]})')
        assert ratio.max() <= 1.0, label
        outs[label] = o
    base = outs['cfg9']
    for label, o in outs.items():
        assert np.array_equal(_bits(o), _bits(base)), f'{label} differs from cfg9 in {(_bits(o) != _bits(base)).sum()} elements (rows {np.flatnonzero((o != base).any(1))[:8]})'
    # the zero rows
    zr = np.flatnonzero(fam == 'const0')
    assert {0, 191, 192, M - 1} <= set(zr.tolist())
    r16 = lambda x: RM.from_bits(RM.to_bits(np.asarray(x, F32), dtype), dtype)
    if epi == 0:
        assert (base[zr] == r16(bias)[None, :]).all()
    else:
        g = LM.gelu64(bias.astype(F64))
        lo, hi = r16(g - LM.GELU_FIT - LM.U * np.abs(g)), r16(g + LM.GELU_FIT + LM.U * np.abs(g))
        undecided = (lo != hi).mean()                                      # rounding is monotone: whatever the fit returns within 1.2e-6 of GELU rounds into [lo, hi]
        print(f'[ln consumer] zero rows {dtype} D={D}: the fit decides the rounding of {100 * undecided:.1f} % of the {N} GELU(bias) values')
        assert ((base[zr] >= lo[None, :]) & (base[zr] <= hi[None, :])).all() and undecided < 0.5
        assert (base[zr] == base[zr[:1]]).all()
    # d. against the true LayerNorm of hi + lo
    ref_ln, bound_ln = LM.layernorm_reference(V, A, W, bias, epi, dtype, bound, rowstat[:, 1])
    err = np.abs(base - ref_ln)
    assert (err <= bound_ln).all(), f'worst {np.max(err / bound_ln):.3f}'
    units = err / _unit16(ref_ln, dtype)
    own = np.abs(base - ref) / _unit16(ref, dtype)
    for f in LC.FAMILIES:
        sel = fam == f
        print(f'[ln consumer] table {dtype} D={D} epi {epi} {f}: against LayerNorm(hi + lo), in 16-bit roundings of the output: median {np.median(units[sel]):.2f} max {units[sel].max():.1f}; '
              f'against the fold on hi: median {np.median(own[sel]):.2f} max {own[sel].max():.1f}; worst |err| / bound {np.max(err[sel] / bound_ln[sel]):.3f}')


# ---------------------------------------------------------------------------------------------------------------- e. fused qkv + attention

@pytest.mark.parametrize('dtype', LC.DTYPES)
@pytest.mark.parametrize('D,heads', [(768, 12), (1280, 16)])
def test_fused_qkv_attention_with_real_statistics(dtype, D, heads):
    """vp_dbg_qkvattn_ln -- qkvattn.hip (head dim 64, D = 768, one pair of crops: 12 tiles) and gemm8.hip's EPI_QKV_ATTN (head dim 80, D = 1280: 32 tiles) -- with the
    statistics of offset, outlier, granule-constant and limit rows: equal BIT FOR BIT to vp_dbg_gemm_case (epi 0, cfg9, the same rowstat and ln_s) followed by
    vp_dbg_attention.  With neutral statistics (all these kernels were run with so far) the fold is an exact no-op."""
    M = 384
    lib = capi.load_library()
    R, P = LC.rows(dtype, D), LC.partials(dtype, D)
    keep = [i for i, f in enumerate(R['family']) if f not in LC.NEUTRAL and not (dtype == 'bf16' and f == 'limit')]      # bf16's hi plane at 1e5 steps by 512: logits of 1e6
    assert {'offset8', 'offset64', 'offset1000', 'outlier'} <= {R['family'][i] for i in keep}
    idx = _cycle(keep, M)
    x = RM.from_bits(R['hi'], dtype)[idx]
    W, ln_s, bias = _weights(dtype, 3 * D, D, 90 + D, scale=1.5 / np.sqrt(D))
    rowstat = _finalize(P[idx], D)
    assert (np.abs(rowstat[:, 0]) > 1.0).mean() > 0.8                     # far from neutral
    fused = np.empty((M, D), F32)
    args = [_c(a) for a in (x, W, bias, rowstat, ln_s)]
    capi.check(lib.vp_dbg_qkvattn_ln(0, capi.DTYPES[dtype], 1, D, heads, *[a.ctypes.data for a in args], fused.ctypes.data))
    qkv = _gemm(dtype, 0, 9, 0, x, W, bias, rowstat, ln_s)
    assert np.isfinite(qkv).all()
    two = np.empty((M, D), F32)
    capi.check(lib.vp_dbg_attention(0, capi.DTYPES[dtype], M // 192, D, heads, qkv.ctypes.data, two.ctypes.data))
    assert np.isfinite(two).all()
    assert np.array_equal(_bits(fused), _bits(two)), f'{(_bits(fused) != _bits(two)).sum()} of {two.size} outputs differ from gemm + attention'
    plain = np.empty((M, D), F32)
    capi.check(lib.vp_dbg_qkvattn(0, capi.DTYPES[dtype], 1, D, heads, *[a.ctypes.data for a in args[:3]], plain.ctypes.data))
    assert (plain != fused).mean() > 0.5                                  # the statistics matter


# ---------------------------------------------------------------------------------------------------------------- f. ln_quant

@pytest.mark.parametrize('dtype', LC.DTYPES)
@pytest.mark.parametrize('M,Mp,D', [(192, 512, 768), (100, 128, 1024)])
def test_ln_quant(dtype, M, Mp, D):
    """vp_dbg_ln_quant (the fp8 mode's LayerNorm -> MXFP8 pass): with (mean, rstd) from ln_finalize on the same partials, the scale bytes equal the model's and the codes
    equal torch.float8_e4m3fn of the model's scaled values, bit for bit (the all-zero blocks of the zero row included); the padding rows M .. Mp - 1 -- whole 64-row groups
    at Mp = 512, the rest of a partly filled group at M = 100 -- come back as zero codes and zero scale bytes from buffers filled with 0xFF."""
    from test_gpu_ops import _mx_layout
    R, P = LC.rows(dtype, D), LC.partials(dtype, D)
    idx = _cycle(np.arange(len(P)), M)
    bits, part = _c(R['hi'][idx], np.uint16), _c(P[idx])
    codes, scales = np.empty(Mp * D, np.uint8), np.empty(Mp * D // 32, np.uint8)
    capi.check(capi.load_library().vp_dbg_ln_quant(0, capi.DTYPES[dtype], M, Mp, D, bits.ctypes.data, part.ctypes.data, codes.ctypes.data, scales.ctypes.data))
    code_off, scale_off = _mx_layout(Mp, D)
    c, s = codes[code_off], scales[scale_off]
    assert (c[M:] == 0).all() and (s[M:] == 0).all(), 'padding rows'
    rowstat = _finalize(part, D)
    E, ref_codes, _ = LM.mx_quantise(LM.quant_normalise(RM.from_bits(bits, dtype), rowstat[:, 0], rowstat[:, 1]))
    assert np.array_equal(s[:M], E), f'{(s[:M] != E).sum()} scale bytes differ (rows {np.flatnonzero((s[:M] != E).any(1))[:8]})'
    assert np.array_equal(c[:M], ref_codes), f'{(c[:M] != ref_codes).sum()} of {ref_codes.size} codes differ (rows {np.flatnonzero((c[:M] != ref_codes).any(1))[:8]})'
    z = np.flatnonzero(np.array(R['family'])[idx] == 'const0')
    assert len(z) and (s[z] == 0).all() and (c[z] == 0).all()
    assert (E > 0).mean() > 0.7 and len(np.unique(E)) > 4                 # the cases do exercise the scales
