"""GPU: the MLP pair -- fc1 with the GELU epilogue, the 64 x 64-blocked `hid` hand-over, fc2 reading it -- against the host model of tests/mlp_model.py on the
problems of tests/mlp_cases.py.  tests/test_mlp_model.py pins the model, its constants and the mutants on the CPU.

A. gelu_core / gelu_sat (csrc/common.h) over every 16-bit pattern times 1, 2 and 1.5, on and off the 16-bit grid, at all 13 wide configurations (the staged
   2-phase epilogue of every gemm.hip tile, the persistent kernel, gemm8's register-direct epilogue on 256 x 256 and 192 x 256 tiles), without the LayerNorm fold
   and with a neutral one: every output inside round16(centre -+ E32) (decided bits where the two ends agree; at most 1 % undecided), the negative tail in
   [-1e-14, 0], fp16 saturation == 65504, bf16 beyond 16 == round16(x), monotone on both sides of the minimum, all 26 launches equal bit for bit.
B. fc1 [768, 4D, D] and fc2 [768, D, 4D] at D = 384, 768, 1024, 1280, per element: fc1 on the LayerNorm-consumer edge rows against LM.fold_reference, blocked
   output and row-major; fc2 on hid-distributed activations against float64 with the accumulation + producer-row bound, blocked A (reversed walk) and row-major;
   every configuration runs or stands in MC.REFUSED (then: the invalid error, nothing written); the production picks run; equal bits across configurations
   (statistics included); bf16 twice.
C. W = I: every admissible 16-bit pattern, permuted per 256 x 256 block, through epi 0 (blocked output and not) and epi 6 (blocked A and not): positions exact.

NaN and inf pre-activations are out of scope, as in the LayerNorm-consumer tests."""
import functools

import numpy as np
import pytest

import ln_consumer_model as LM
import mlp_cases as MC
import mlp_model as MM
import residual_row_model as RM
from easy_vitpose_amd import _capi as capi
from helpers import round_to

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
OUTB, AB, REV = MC.OUTB, MC.AB, MC.REV
FILL = 123.0


def _c(a, dt=F32):
    return np.ascontiguousarray(a, dtype=dt)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _bits(a):
    return _c(a).view(np.uint32)


def _gemm(dtype, epi, variant, flags, A, W, bias, aux=None, rowstat=None, ln_s=None, group_m=8, want_stats=False):
    """(return code, out, stats); out and stats keep their fill where the tap refuses.  The operands must already be contiguous float32."""
    m, k = A.shape
    n = W.shape[0]
    out = np.full((m, n), FILL, F32)
    stats = np.full((m, n // 64, 2), FILL, F32) if want_stats else None
    rc = capi.load_library().vp_dbg_gemm_case(0, capi.DTYPES[dtype], epi, variant, group_m, flags, m, n, k, _ptr(A), _ptr(W), _ptr(bias), _ptr(aux), _ptr(rowstat),
                                              _ptr(ln_s), _ptr(out), _ptr(stats))
    return rc, out, stats


def _refused(rc, *outs):
    assert rc != 0 and 'invalid' in capi.last_error().lower(), (rc, capi.last_error())
    for o in outs:
        assert (o == FILL).all(), 'a refused launch wrote its output'


def _finalize(p, D):
    p = _c(p)
    out = np.empty((p.shape[0], 2), F32)
    capi.check(capi.load_library().vp_dbg_ln_finalize(0, p.shape[0], p.shape[1], D, p.ctypes.data, out.ctypes.data))
    return out


# ---------------------------------------------------------------------------------------------------------------- A. GELU over the domain

@pytest.mark.parametrize('dtype', MC.DTYPES)
def test_gelu_over_every_16_bit_input_at_every_site(dtype):
    """MC.gelu_sweep through epi 1 with the blocked output, 13 configurations x (no fold, neutral fold).  The model decides the bits of all but the undecided
    share; the sites must agree bit for bit, so the acceptance runs once on cfg9 and every other launch is compared with it."""
    p = MC.gelu_sweep(dtype)
    A, W, bias = _c(p['A']), _c(p['W']), _c(p['bias'])
    rowstat, ln_s = (_c(a) for a in p['neutral'])
    ok = p['finite']
    assert (~ok).sum() == p['n_overflow']
    x = p['x']
    base = None
    for label, variant, fl in MC.WIDE:
        for fold in (False, True):
            rc, o, _ = _gemm(dtype, 1, variant, OUTB | fl, A, W, bias, rowstat=rowstat if fold else None, ln_s=ln_s if fold else None)
            assert rc == 0, (label, capi.last_error())
            if base is None:
                base = o
            same = _bits(o)[ok] == _bits(base)[ok]
            # zeros of either sign are one value to the model, but the SITES must agree on the sign as well: they run one definition
            assert same.all(), f'{label}{" with the neutral fold" if fold else ""}: {(~same).sum()} outputs differ from cfg9, first at {np.argwhere(ok & (_bits(o) != _bits(base)))[0]}'
    got, xf = base[ok].astype(F64), x[ok]
    bad, undecided = MM.accept(xf, got, dtype)
    lo, hi = MM.interval(xf.astype(F64), dtype)
    two = (lo != hi) & (xf >= -8)
    implied = MM.implied_ratio(xf, got, dtype)
    emu = MM.to16(MM.emu32(xf, dtype), dtype).astype(F64)
    print(f'[mlp] GELU sweep {dtype}: {int((emu != got).sum())} outputs differ from the float32 emulation with an exact exp2 ({int(((emu != got) & (xf >= -8)).sum())} of them at x >= -8)')
    print(f'[mlp] GELU sweep {dtype}: {xf.size} finite pre-activations at 13 sites x 2, all equal bit for bit; undecided {100 * undecided:.3f} % of x >= -8 '
          f'({int(two.sum())} outputs, {int((got[two] == hi[two]).sum())} took the upper candidate); rejected {int(bad.sum())}; worst implied |r - centre| / E32 '
          f'{implied.max():.3f} at x = {xf[int(implied.argmax())]:.6g}')
    if bad.any():
        i = np.flatnonzero(bad)[:8]
        raise AssertionError(f'{int(bad.sum())} outputs outside the acceptance; first x {xf[i]}, got {got[i]}, lo {lo[i]}, hi {hi[i]}')
    assert undecided <= 0.01
    assert MM.monotone(xf, got) == 0
    if dtype == 'fp16':
        assert got.max() == 65504.0 and (got[xf > 65504.0] == 65504.0).all() and (xf > 65504.0).sum() > 1000
        sub = (np.abs(got) < 2.0 ** -14) & (got != 0)
        assert sub.sum() > 10000, 'fp16-subnormal outputs must survive'
    else:
        s2 = np.broadcast_to(p['s'][:, None] == 2.0, x.shape)[ok] & (xf > 16.0)
        assert s2.sum() > 10000 and np.isfinite(got[s2]).all() and (got[s2] == MM.round16(xf[s2].astype(F64), dtype)).all()


# ---------------------------------------------------------------------------------------------------------------- B. the model widths

@functools.lru_cache(maxsize=None)
def _fc1_reference(dtype, D):
    idx, fam, A, part = MC.fc1_rows(dtype, D)
    W, ln_s, bias = MC.fc1_weights(dtype, D)
    rowstat = _finalize(part, D)
    ref, bound, _ = LM.fold_reference(A, W, ln_s, bias, rowstat[:, 0], rowstat[:, 1], 1, dtype)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return fam, _c(A), _c(W), _c(ln_s), _c(bias), _c(rowstat), ref, bound


def _picks(kind, D):
    """the production picks of one GEMM of one model: (2-phase variant at 4 crops, 8-phase variant at the model's BASELINE batch or 0)"""
    lib = capi.load_library()
    name, batch = MC.MODELS[D]
    Mm, N, K = MC.SHAPES[D][kind]
    epi, wide = (1, 1) if kind == 'fc1' else (6, 0)
    v2 = lib.vp_dbg_gemm2_pick(epi, Mm, N, K, None)
    v8 = lib.vp_dbg_gemm8_pick(192 * batch, N, wide, 3, None)
    print(f'[mlp] {name} {kind}: 2-phase pick at 4 crops cfg{v2}; 8-phase pick at {batch} crops: {v8 or "none (2-phase kernels)"}')
    return v2, v8


@pytest.mark.parametrize('dtype', MC.DTYPES)
@pytest.mark.parametrize('D', sorted(MC.SHAPES))
def test_fc1_at_model_widths(dtype, D):
    """fc1 [768, 4D, D], epi 1, with the statistics ln_finalize wrote for the case rows: per element inside LM.fold_reference's bound, blocked and row-major output,
    13 configurations, equal bit for bit; bf16 twice."""
    fam, A, W, ln_s, bias, rowstat, ref, bound = _fc1_reference(dtype, D)
    ran, base = set(), None
    for label, variant, fl in MC.WIDE:
        assert ('fc1', D, variant) not in MC.REFUSED
        for flags in (OUTB, 0):
            rc, o, _ = _gemm(dtype, 1, variant, flags | fl, A, W, bias, rowstat=rowstat, ln_s=ln_s)
            assert rc == 0, (label, flags, capi.last_error())
            assert np.isfinite(o).all(), label
            if base is None:
                base = o
            if flags == OUTB:
                ratio = (np.abs(o - ref) / bound).max(1)
                r = int(ratio.argmax())
                print(f'[mlp] fc1 {dtype} D={D} {label}: worst |err| / bound {ratio.max():.3f} (row {r}: {fam[r]})')
                assert ratio.max() <= 1.0, label
            assert np.array_equal(_bits(o), _bits(base)), f'{label} flags {flags}: {(_bits(o) != _bits(base)).sum()} elements differ from cfg9 (rows {np.flatnonzero((o != base).any(1))[:8]})'
            if dtype == 'bf16':
                rc, again, _ = _gemm(dtype, 1, variant, flags | fl, A, W, bias, rowstat=rowstat, ln_s=ln_s)
                assert rc == 0 and np.array_equal(_bits(again), _bits(o)), f'{label} flags {flags}: not run-to-run identical'
        ran.add(variant)
    v2, v8 = _picks('fc1', D)
    assert v2 in ran and (v8 == 0 or v8 in ran), (v2, v8)


@functools.lru_cache(maxsize=None)
def _fc2_reference(dtype, D):
    A, W, bias, resid = MC.fc2_problem(dtype, D)
    ref, bound = MM.fc2_reference(A, W, bias, resid, dtype)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return _c(A), _c(W), _c(bias), _c(resid), ref, bound


@pytest.mark.parametrize('dtype', MC.DTYPES)
@pytest.mark.parametrize('D', sorted(MC.SHAPES))
def test_fc2_at_model_widths(dtype, D):
    """fc2 [768, D, 4D], epi 6, on hid-distributed activations: planes (hi + lo) per element inside MM.fc2_reference's bound, granule statistics against the stored
    values, blocked A with the reversed walk and row-major A, the 13 residual configurations: each runs or is in MC.REFUSED; equal bits, statistics included."""
    A, W, bias, resid, ref, bound = _fc2_reference(dtype, D)
    ran, base = set(), None
    for label, variant in MC.RESID:
        gm = MC.group_m(variant)
        for flags in (AB | REV, 0):
            rc, o, st = _gemm(dtype, 6, variant, flags, A, W, bias, aux=resid, group_m=gm, want_stats=True)
            if ('fc2', D, variant) in MC.REFUSED:
                _refused(rc, o, st)
                continue
            assert rc == 0, (label, flags, capi.last_error(), 'not in MC.REFUSED')
            assert np.isfinite(o).all() and np.isfinite(st).all(), label
            if base is None:
                base = (o, st)
            if flags == AB | REV:
                ratio = np.abs(o - ref) / bound
                print(f'[mlp] fc2 {dtype} D={D} {label}: worst |err| / bound {ratio.max():.4f}')
                assert ratio.max() <= 1.0, label
                g = o.astype(F64).reshape(MC.M, D // 64, 64)                  # statistics of the STORED values
                m2 = ((g - g.mean(-1, keepdims=True)) ** 2).sum(-1)
                assert np.abs(st[..., 0] - g.sum(-1)).max() < 2e-3 and np.abs(st[..., 1] - m2).max() < 2e-3 * max(1.0, m2.max()), f'{label}: granule statistics'
            assert np.array_equal(_bits(o), _bits(base[0])) and np.array_equal(_bits(st), _bits(base[1])), \
                f'{label} flags {flags}: {(_bits(o) != _bits(base[0])).sum()} elements, {(_bits(st) != _bits(base[1])).sum()} statistics differ from cfg11'
            if dtype == 'bf16':
                rc, o2, st2 = _gemm(dtype, 6, variant, flags, A, W, bias, aux=resid, group_m=gm, want_stats=True)
                assert rc == 0 and np.array_equal(_bits(o2), _bits(o)) and np.array_equal(_bits(st2), _bits(st)), f'{label} flags {flags}: not run-to-run identical'
            ran.add(variant)
    refused = {v for (k, d, v) in MC.REFUSED if k == 'fc2' and d == D}
    assert ran | refused == {v for _, v in MC.RESID} and not ran & refused
    print(f'[mlp] fc2 {dtype} D={D}: ran {sorted(ran)}, refused {sorted(refused)}')
    v2, v8 = _picks('fc2', D)
    assert v2 in ran and (v8 == 0 or v8 in ran), (v2, v8)


# ---------------------------------------------------------------------------------------------------------------- C. transport

def _same_place(what, bits, got_bits, dtype):
    msg = MC.misplaced(bits, got_bits, dtype)
    assert msg is None, f'{what}: {msg}'


@pytest.mark.parametrize('dtype', MC.DTYPES)
def test_transport_with_identity_weights(dtype):
    """W = I, bias 0, M = N = K = 768.  Epi 0 on the 13 wide configurations, blocked output and row-major: out == A.  Epi 6 on the 13 residual configurations
    (zero residual planes), blocked A and row-major: hi plane == A, lo plane all zero patterns, statistics those of A."""
    p = MC.transport(dtype)
    bits, A, W = p['bits'], _c(p['A']), _c(p['W'])
    bias = np.zeros(768, F32)
    if dtype == 'fp16':
        v = A.astype(F64)
        assert ((np.abs(v) < 2.0 ** -14) & (v != 0)).sum() > 9 * 2000 and (np.abs(v) == 65504.0).sum() >= 18
    for label, variant, fl in MC.WIDE:
        for flags in (OUTB, 0):
            rc, o, _ = _gemm(dtype, 0, variant, flags | fl, A, W, bias)
            assert rc == 0, (label, capi.last_error())
            _same_place(f'epi 0 {label} flags {flags}', bits, RM.to_bits(o, dtype), dtype)
            assert np.array_equal(np.where(o == 0, F32(0), o), np.where(A == 0, F32(0), A))
    # epi 6, plane bits on both sides
    zero = np.zeros((768, 768), np.uint16)
    s1_model = RM.granule_s1(A)
    m2, mean = RM.m2_fp64(A)
    m2_bound = RM.m2_bound(m2, mean)
    lib = capi.load_library()
    for label, variant in MC.RESID:
        for flags in (AB, 0):
            o_hi, o_lo = np.full((768, 768), 0xABCD, np.uint16), np.full((768, 768), 0xABCD, np.uint16)
            stats = np.full((768, 12, 2), FILL, F32)
            rc = lib.vp_dbg_gemm_case_planes(0, capi.DTYPES[dtype], 6, variant, MC.group_m(variant), flags, 768, 768, 768, _ptr(A), _ptr(W), _ptr(bias), _ptr(zero),
                                             _ptr(zero), None, 0, _ptr(o_hi), _ptr(o_lo), _ptr(stats))
            assert rc == 0, (label, capi.last_error())
            what = f'epi 6 {label} flags {flags}'
            _same_place(what, bits, o_hi, dtype)
            assert (o_lo == 0).all(), f'{what}: {(o_lo != 0).sum()} lo patterns are not +0, first at {np.argwhere(o_lo != 0)[0]}'
            assert np.isfinite(stats).all(), what
            s1, s2 = _c(stats[..., 0]), stats[..., 1].astype(F64)
            assert np.array_equal(_bits(np.where(s1 == 0, F32(0), s1)), _bits(np.where(s1_model == 0, F32(0), s1_model))), f'{what}: granule sums differ from the tree of the row model'
            with np.errstate(all='ignore'):
                r = np.where(m2_bound > 0, np.abs(s2 - m2) / m2_bound, np.where(s2 == m2, 0.0, np.inf))
            assert r.max() <= 1.0, f'{what}: granule M2 off by {r.max():.3f} of its bound'
    print(f'[mlp] transport {dtype}: {len(MC.transport_patterns(dtype))} patterns x 9 blocks, 26 + 26 launches, every element in place; worst |s2 - M2| / bound {r.max():.3f}')
    assert round_to(A, dtype).tobytes() == A.tobytes()                      # the operands were exact in the type: nothing above is a rounding question
