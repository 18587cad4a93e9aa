"""CPU: the host model of the MLP pair (tests/mlp_model.py) on the problems the device test runs (tests/mlp_cases.py), pinned before any GPU time is spent.

    * the float32 emulation of gelu_core (numpy float32 fmas, an exact exp2) stays within 0.5 E32 of the model's centre (fit64; x / 2 in the tiny range) on every
      sweep input of both types, and IS the exact value in the two ranges where E32 = 0: E32's constants come from the derivation in mlp_model.py, not from a
      device.  Worst ratio 0.495 (fp16, x = 4.014) / 0.474 (bf16, x = 4.012);
    * fit64 and the emulation against the true erf GELU: at most 1.2e-6, the figure of common.h's comment and of LM.GELU_FIT (1.059e-6 and 1.178e-6);
    * at most 1 % of the sweep inputs with x >= -8 leave the rounding of the output undecided (0.248 % fp16, 0.115 % bf16);
    * the acceptance has teeth: every mutant of mlp_model.mutants is rejected on the sweep.  One wrong kernel is NOT a mutant here, because the acceptance cannot
      see it: fma(-a, h, relu) rounded ONCE to 16 bits (v_fma_mix*).  Its result is round16 of a value inside fit64 +- E32, hence inside the interval, always --
      asserted below.  What catches it is the bit identity of the configurations (hipcc fused in SOME instantiations), which the device test asserts over all 13
      sites: the mutant does differ from the two-rounding form on the sweep, also asserted below."""
import numpy as np
import pytest

import ln_consumer_model as LM
import mlp_cases as MC
import mlp_model as MM
import residual_row_model as RM

F32, F64 = np.float32, np.float64


def _x(dtype):
    p = MC.gelu_sweep(dtype)
    return p['x'][p['finite']]


def test_round16_is_the_types_rounding():
    """round16 (float64 -> the type, one rounding) against torch's conversion on float32 inputs: every 16-bit pattern, midpoints, subnormals, the limits"""
    rng = np.random.default_rng(3)
    for dtype in MC.DTYPES:
        v = MC.patterns(dtype).astype(F64)
        mid = (np.sort(v)[1:] + np.sort(v)[:-1]) / 2.0                       # exact ties (24 bits suffice)
        x = np.concatenate([v, mid, mid * (1 + 2.0 ** -20), mid * (1 - 2.0 ** -20), rng.standard_normal(4096) * 1e-6, rng.standard_normal(4096) * 100]).astype(F32)
        x = x[np.abs(x) < (65520.0 if dtype == 'fp16' else 3.0e38)]
        assert np.array_equal(MM.round16(x.astype(F64), dtype), MC.r16(x, dtype).astype(F64))
    assert MM.round16(np.array([65519.9, 7e4, -1e9]), 'fp16').tolist() == [65504.0, 65504.0, -65504.0]


@pytest.mark.parametrize('dtype', MC.DTYPES)
def test_sweep_construction(dtype):
    """the sweep is what it says: every pattern in every 256 x 256 block, the overflow count from the bits, the saturation branch, subnormal outputs, x off the grid"""
    p = MC.gelu_sweep(dtype)
    A, W, x = p['A'], p['W'], p['x']
    assert np.array_equal(MC.r16(W, dtype), W) and (np.count_nonzero(A, axis=1) == 1).all()
    acc = A.astype(F64) @ W.astype(F64).T                                    # one product per element: exact
    with np.errstate(over='ignore'):
        assert np.array_equal((acc + p['bias'].astype(F64)[None, :]).astype(F32), x, equal_nan=True)
    assert (~p['finite']).sum() == p['n_overflow'] and not np.isnan(x).any()
    pat = MC.patterns(dtype)
    for i in range(3):
        for j in range(3):
            w = acc[256 * i:256 * i + 256, 256 * j:256 * j + 256] / float(p['s'][256 * i])
            assert np.array_equal(np.sort(w.ravel()), np.sort(pat.astype(F64)))
    xf = x[p['finite']]
    off_grid = MC.r16(xf, dtype) != xf
    assert off_grid.mean() > 0.3 and ((xf > -8) & (xf < 8) & off_grid).sum() > 100000
    if dtype == 'fp16':
        assert x[:, :256].max() == 131008.0 and (xf > 65504.0).sum() > 1000
        g = MM.fit64(xf.astype(F64), dtype)
        assert ((np.abs(g) < 2.0 ** -14) & (g != 0)).sum() > 10000           # fp16-subnormal outputs


@pytest.mark.parametrize('dtype', MC.DTYPES)
def test_emulation_within_half_e32(dtype):
    """|emu32 - centre| <= 0.5 E32 on every sweep input (centre = fit64 but in the tiny range, where it is x / 2); in the two exact ranges E32 = 0 and the
    emulation is the exact value bit for bit; fit64 itself is never further from centre than 2^-25 |centre|"""
    x = _x(dtype)
    x64 = x.astype(F64)
    err = np.abs(MM.emu32(x, dtype).astype(F64) - MM.centre(x64, dtype))
    E = MM.e32(x64, dtype)
    with np.errstate(all='ignore'):
        ratio = np.where(E > 0, err / E, np.where(err == 0, 0.0, np.inf))
    i = int(ratio.argmax())
    tiny, far = MM.ranges(x64)
    print(f'[mlp model] {dtype}: worst |emu32 - centre| / E32 = {ratio.max():.3f} at x = {x[i]:.6g}; exact ranges: tiny {int(tiny.sum())}, far {int(far.sum())} of {x.size} inputs')
    assert ratio.max() <= 0.5
    assert tiny.sum() > 1000 and (far & (x > 0)).sum() > 1000 and (err[tiny | (far & (x > 0))] == 0).all()
    assert (np.abs(MM.fit64(x64, dtype) - MM.centre(x64, dtype)) <= 2.0 ** -25 * np.abs(MM.centre(x64, dtype))).all()


def test_fit_against_erf_gelu():
    """common.h: |error| <= 1.2e-6 -- fit64 on the sweep inputs of both types, the float32 emulation on a dense grid of [-14, 14]"""
    for dtype in MC.DTYPES:
        x = _x(dtype).astype(F64)
        x = x[np.abs(x) < 1e6]                                               # beyond: GELU(x) = x, and |x - x| is no statement about the fit
        e = np.abs(MM.fit64(x, 'bf16') - LM.gelu64(x)).max()
        print(f'[mlp model] {dtype}: |fit64 - GELU| on the sweep inputs: {e:.3e}')
        assert e <= 1.2e-6
    g = MC.dense_grid()
    e = np.abs(MM.emu32(g, 'bf16').astype(F64) - LM.gelu64(g.astype(F64))).max()
    print(f'[mlp model] |emu32 - GELU| on {g.size} float32 points of [-14, 14]: {e:.3e}')
    assert e <= 1.2e-6 and LM.GELU_FIT == 1.2e-6


@pytest.mark.parametrize('dtype', MC.DTYPES)
def test_emulation_passes_and_undecided_share(dtype):
    """the emulation's own 16-bit outputs pass the whole acceptance (interval, tail, saturation, monotone); at most 1 % of the inputs x >= -8 are undecided"""
    x = _x(dtype)
    got = MM.to16(MM.emu32(x, dtype), dtype)
    bad, undecided = MM.accept(x, got, dtype)
    print(f'[mlp model] {dtype}: undecided share {100 * undecided:.3f} % of the inputs with x >= -8')
    assert not bad.any() and undecided <= 0.01
    assert MM.monotone(x, got) == 0
    if dtype == 'fp16':
        assert got.max() == 65504.0
    # what the 16-bit outputs still tell of the float32 value: never more than the float32 error itself; a neighbouring 16-bit value is far outside
    implied = MM.implied_ratio(x, got, dtype)
    print(f'[mlp model] {dtype}: worst implied |r - centre| / E32 of the emulation {implied.max():.3f}')
    assert implied.max() <= 0.5
    bits = RM.to_bits(got, dtype)
    pick = np.flatnonzero((x > -8) & (x < 16) & (np.abs(got) > 1e-3) & ((bits & 0x7fff) < 0x7bff))[::97]
    up = RM.from_bits((bits[pick] + 1).astype(np.uint16), dtype)
    assert (MM.implied_ratio(x[pick], up, dtype) > 1.0).mean() > 0.98 and MM.accept(x[pick], up, dtype)[0].mean() > 0.98


def test_misplaced_names_the_element():
    """MC.misplaced on the transport problem: the problem itself passes, a zero may lose its sign, a swapped pair / a flipped bit / a zero from nowhere are named"""
    for dtype in MC.DTYPES:
        bits = MC.transport(dtype)['bits']
        assert MC.misplaced(bits, bits.copy(), dtype) is None
        z = bits.copy()
        z[bits == 0x8000] = 0
        assert (bits == 0x8000).sum() >= 9 and MC.misplaced(bits, z, dtype) is None
        s = bits.copy()
        s[70, 65], s[70, 129] = bits[70, 129], bits[70, 65]                  # the same row of two neighbouring 64 x 64 blocks
        msg = MC.misplaced(bits, s, dtype)
        assert msg is not None and msg.startswith('2 elements') and '(70, 65)' in msg and '((0, 0), 70, 129)' in msg, msg
        f = bits.copy()
        f[300, 700] ^= 1
        assert '(300, 700)' in MC.misplaced(bits, f, dtype) and 'block (1, 2) row 44 column 188' in MC.misplaced(bits, f, dtype)
        n = bits.copy()
        n[5, 5] = 0 if RM.from_bits(bits[5:6, 5], dtype)[0] != 0 else 0x3c00
        assert MC.misplaced(bits, n, dtype) is not None


@pytest.mark.parametrize('dtype', MC.DTYPES)
def test_acceptance_rejects_every_mutant(dtype):
    x = _x(dtype)
    muts = MM.mutants(x, dtype)
    assert set(muts) >= {'tanh-approximate GELU', 'x sigmoid(1.702 x)', '0 for x < -3.5', 'truncating conversion', 'one fused rounding'}
    assert dtype == 'bf16' or {'max(x, 0) without the fp16 clamp', 'fp16 subnormals flushed'} <= set(muts)
    good = MM.to16(MM.emu32(x, dtype), dtype).astype(F64)
    for name, got in muts.items():
        bad, _ = MM.accept(x, got, dtype)
        print(f'[mlp model] {dtype} mutant {name}: {int(bad.sum())} of {x.size} outputs rejected; {int((got != good).sum())} differ from the emulation')
        if name == 'one fused rounding':
            # arithmetically indistinguishable by the interval (module docstring); the configurations' bit identity is its screen
            assert bad.sum() == 0 and (got != good).sum() > 0
        else:
            assert bad.sum() > 0, name


def test_fc2_bound_holds_for_a_float32_model():
    """fc2_reference's bound against a float32 evaluation in one fixed order (chunks of 64 accumulated in float32) through residual_row_model's row"""
    dtype, D = 'fp16', 384
    A, W, bias, resid = MC.fc2_problem(dtype, D)
    A, resid = A[:64], resid[:64]
    ref, bound = MM.fc2_reference(A, W, bias, resid, dtype)
    acc = np.zeros((64, D), F32)
    for k in range(0, 4 * D, 64):
        acc = (acc + (A[:, k:k + 64].astype(F64) @ W[:, k:k + 64].astype(F64).T).astype(F32)).astype(F32)
    _, hi, lo = RM.split(resid, dtype)
    _, ohi, olo = RM.row((acc + bias[None, :]).astype(F32), RM.decode(hi, lo, dtype), dtype)
    got = RM.from_bits(ohi, dtype).astype(F64) + RM.from_bits(olo, dtype).astype(F64)
    ratio = np.abs(got - ref) / bound
    print(f'[mlp model] fc2 bound, float32 model: worst ratio {ratio.max():.3f}')
    assert ratio.max() <= 1.0
    assert (np.signbit(A) & (A == 0)).sum() > 100 and ((A < 0) & (A > -0.17)).mean() > 0.2      # hid's distribution: -0 entries, the mass below 0
