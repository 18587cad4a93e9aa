"""CPU: the host model of the keypoint head (tests/head_model.py) on the case families the device test runs (tests/head_cases.py), pinned before any GPU time is spent.

    * the model's transposed convolution, BatchNorm(eval) + ReLU and final 1x1 conv against torch's float64 modules on unrounded operands, to 1e-12 of the magnitude sum;
    * the taps family: the model's output IS the gathered source code, bit for bit;
    * the bounds tests/test_gpu_head.py asserts (HM.bound0, HM.bound_final; derived in head_model's docstring) admit a float32 emulation of the kernel and the model
      itself against the un-folded module -- were that not so the derivation would be wrong, not the constant;
    * every wrong model of HM.WRONG_STAGE0 / HM.WRONG_FINAL fails those bounds on at least one case (the table is printed);
    * the set of tiles the selection rule can put a deconv on, swept over 1-400 crops of every model, equals HC.STAGE0_TILES: a rule change that makes another tile
      reachable fails here until tests/test_gpu_head.py runs it."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_cases as HC
import head_model as HM

F32, F64 = np.float32, np.float64
SMALL = (('fp16', 3, 16, 12, 384), ('bf16', 3, 16, 12, 384), ('fp16', 2, 32, 24, 256))     # the shapes the wrong models are shown on
PARTS = {'edges': (HC.edges, HC.edges_parts), 'relu_clamp': (HC.relu_clamp, HC.relu_parts), 'onehot': (HC.onehot, HC.onehot_parts)}


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, F64)).permute(0, 3, 1, 2)


def _case(family, shape):
    return PARTS[family][0](*shape), PARTS[family][1](*shape)


@pytest.mark.parametrize('B,H,W,Cin', [(2, 5, 3, 8), (3, 16, 12, 384)])
def test_model_against_torch_fp64(B, H, W, Cin):
    rng = np.random.default_rng(Cin + B)
    x = rng.standard_normal((B, H, W, Cin))
    w = rng.standard_normal((Cin, 256, 4, 4)) * (2.0 / (4 * Cin)) ** 0.5
    g, b, m = 1 + 0.3 * rng.standard_normal(256), 0.1 * rng.standard_normal(256), rng.standard_normal(256)
    g[::4] *= -1
    var = rng.uniform(0.0, 3.0, 256)
    z = HM.deconv(x, w)
    A = HM.deconv(np.abs(x), np.abs(w))
    tz = F.conv_transpose2d(_nchw(x), torch.from_numpy(w), None, stride=2, padding=1)
    assert (np.abs(z - tz.permute(0, 2, 3, 1).numpy()) <= 1e-12 * A).all()
    ty = F.relu(F.batch_norm(tz, torch.from_numpy(m), torch.from_numpy(var), torch.from_numpy(g), torch.from_numpy(b), training=False, eps=1e-5))
    y = HM.module(x, w, g, b, m, var, 'bf16')
    scale = np.abs(g) / np.sqrt(var + 1e-5)
    assert (np.abs(y - ty.permute(0, 2, 3, 1).numpy()) <= 1e-12 * (scale * (A + np.abs(m)) + np.abs(b))).all()
    # the final 1x1 conv: hi + lo stands for w to the operand type's 2u^2 (the model multiplies hi + lo, torch here w itself: compared on hi + lo)
    wf = (rng.standard_normal((25, 256)) * 0.02).astype(F32)
    bf = (rng.standard_normal(25) * 0.1).astype(F32)
    hi, lo = HM.split_final(wf, 'fp16')
    assert (np.abs(hi.astype(F64) + lo - wf) <= 2.0 ** -21 * np.abs(wf) + 2.0 ** -25).all() and (lo != 0).mean() > 0.9
    a = np.abs(rng.standard_normal((B, 2 * H, 2 * W, 256)))
    hm, S2 = HM.final(a, wf, bf, 'fp16')
    th = F.conv2d(_nchw(a), torch.from_numpy(hi.astype(F64) + lo)[:, :, None, None], torch.from_numpy(bf.astype(F64)))
    assert hm.shape == (B, 25, 2 * H, 2 * W) and (np.abs(hm - th.numpy()) <= 1e-12 * S2).all()


@pytest.mark.parametrize('shape', HC.DECONV1 + HC.DECONV2, ids=str)
@pytest.mark.parametrize('rot', (0, 1))
def test_taps_model_is_the_gathered_code(shape, rot):
    c = HC.taps(*shape, rot)
    wf, bias = HM.fold(c['w'], c['gamma'], c['beta'], c['mean'], c['var'], shape[0])
    assert np.array_equal(wf, c['w']) and not bias.any()                 # the identity BatchNorm folds to the weights themselves
    z, A = HM.conv_parts(c['x'], wf)
    v, stored, _ = HM.stage0(z, A, bias, shape[0])
    exp = HC.taps_expected(c)
    assert np.array_equal(stored, exp) and np.array_equal(v, exp)
    assert (exp == 0).any() and len(np.unique(exp)) > 40


@pytest.mark.parametrize('family', ('edges', 'relu_clamp', 'onehot'))
@pytest.mark.parametrize('shape', HC.DECONV1 + HC.DECONV2, ids=str)
def test_bounds_admit_a_float32_emulation(family, shape):
    """a float32 evaluation of the definition (one order a kernel may take) against the model, and both against the un-folded module, inside the bounds"""
    dtype, Cin = shape[0], shape[4]
    c, p = _case(family, shape)
    v, stored, S = HM.stage0(p['z'], p['A'], p['bias'], dtype)
    emu = HM.emulate_stage0(c['x'], p['wf'], p['bias'], dtype)
    mod = HM.module(c['x'], c['w'], c['gamma'], c['beta'], c['mean'], c['var'], dtype)
    r = HM.ratio(emu, v, HM.bound0(v, S, Cin, dtype)).max()
    r_mod = HM.ratio(emu, mod, HM.bound0(mod, S, Cin, dtype, unfolded=True)).max()
    r_ref = HM.ratio(stored, mod, HM.bound0(mod, S, Cin, dtype, unfolded=True)).max()
    print(f'[head model {family} {shape}] float32 emulation: worst err / bound {r:.3f} vs the model, {r_mod:.3f} vs the module; the model vs the module {r_ref:.3f}')
    assert r <= 1 and r_mod <= 1 and r_ref <= 1
    assert (v == 0).mean() > 0.2 and (v > 0).mean() > 0.2
    if family == 'relu_clamp':
        assert not stored[..., HC.NEG].any()
        big = stored[..., HC.BIG]
        assert (big == 65504).all() if dtype == 'fp16' else ((big > 9e5) & np.isfinite(big)).all()
        tiny = stored[..., HC.TINY]
        assert (tiny > 0).all() and (tiny < 2.0 ** -14).all()                                # fp16: subnormal
        for k, (n, oy, ox) in enumerate(HC.relu_pix(*shape[1:4])):                          # the pre-activation there: within one accumulation error of 0
            o = HC.ZERO.start + k
            assert abs(p['z'][n, oy, ox, o] + F64(p['bias'][o])) <= 4 * Cin * 2.0 ** -24 * S[n, oy, ox, o]


def test_relu_parts_are_a_fresh_fold():
    shape = ('fp16', 1, 16, 12, 384)
    r, p = HC.relu_clamp(*shape), HC.relu_parts(*shape)
    wf, bias = HM.fold(r['w'], r['gamma'], r['beta'], r['mean'], r['var'], 'fp16')
    z, A = HM.conv_parts(r['x'], wf)
    assert np.array_equal(wf, p['wf']) and np.array_equal(bias, p['bias']) and np.array_equal(z, p['z']) and np.array_equal(A, p['A'])


@pytest.mark.parametrize('dtype,B', [('fp16', 1), ('bf16', 2)])
def test_final_bound_admits_a_float32_emulation(dtype, B):
    p = HC.edges_parts(dtype, B, 32, 24, 256)
    a = HM.stage0(p['z'], p['A'], p['bias'], dtype)[1]
    for Kp in HC.KPS:
        f = HC.final(dtype, Kp)
        ref, S2 = HM.final(a, f['w_fin'], f['b_fin'], dtype)
        r = HM.ratio(HM.emulate_final(a, f['w_fin'], f['b_fin'], dtype), ref, HM.bound_final(S2)).max()
        bad = HM.ratio(HM.final(a, f['w_fin'], f['b_fin'], dtype, 'lo_dropped')[0], ref, HM.bound_final(S2))
        print(f'[head model final {dtype} B={B} Kp={Kp}] float32 emulation: worst err / bound {r:.3f}; lo plane dropped: {bad.max():.1f}, {(bad > 1).mean():.0%} of the elements fail')
        assert r <= 1
        assert bad.max() > 1
        if Kp >= 16:
            assert not bad[:, 3].any() and (bad[:, Kp - 1] > 1).any()       # the zero row has no lo plane; the large row's is large


def _wrong_ratio(wrong, family, shape):
    """worst err / bound of the wrong model's stored output, handed to the checker in place of the device's"""
    dtype, Cin = shape[0], shape[4]
    if family == 'taps':
        c = HC.taps(*shape, 0)
        wf, bias = HM.fold(c['w'], c['gamma'], c['beta'], c['mean'], c['var'], dtype, wrong)
        got = HM.stage0(HM.deconv(c['x'], wf, wrong), 0.0, bias, dtype, wrong)[1]
        return 0.0 if np.array_equal(got, HC.taps_expected(c)) else np.inf
    c, p = _case(family, shape)
    v, _, S = HM.stage0(p['z'], p['A'], p['bias'], dtype)
    if wrong in ('no_relu', 'no_clamp'):
        z, bias = p['z'], p['bias']
    else:
        wf, bias = HM.fold(c['w'], c['gamma'], c['beta'], c['mean'], c['var'], dtype, wrong)
        z = p['z'] if wrong == 'plus_mean' else HM.deconv(c['x'], wf, wrong)
    return HM.ratio(HM.stage0(z, 0.0, bias, dtype, wrong)[1], v, HM.bound0(v, S, Cin, dtype)).max()


def test_wrong_models_fail_the_bounds():
    table = {}
    for wrong in HM.WRONG_STAGE0:
        for family in ('taps', 'edges', 'relu_clamp', 'onehot'):
            table[wrong, family] = [_wrong_ratio(wrong, family, s) for s in SMALL]
    for k, v in table.items():
        print(f'[head model] {k[0]:18s} {k[1]:10s} worst err / bound per shape {SMALL}:', ' '.join(f'{r:.3g}' for r in v))
    fails = lambda wrong, family: all(r > 1 for r in table[wrong, family])
    for wrong in ('ky_swap', 'parity_transposed', 'border_clamp', 'seam'):       # the geometry: exact on the taps, and far outside the bounds on Gaussian data
        assert fails(wrong, 'taps') and fails(wrong, 'edges'), wrong
    assert fails('no_relu', 'edges') and fails('plus_mean', 'edges') and fails('no_relu', 'onehot')
    assert table['no_clamp', 'relu_clamp'][0] == np.inf and table['no_clamp', 'relu_clamp'][2] == np.inf      # fp16: inf in the BIG channels
    assert table['no_clamp', 'relu_clamp'][1] <= 1                                                             # bf16 has no clamp to lose
    assert fails('round_before_fold', 'onehot')
    assert not fails('round_before_fold', 'edges')          # ... which a Gaussian sum of 4 Cin products can hide (fp16, Cin = 384): why onehot exists
    for wrong in HM.WRONG_STAGE0:
        assert any(r > 1 for f in ('taps', 'edges', 'relu_clamp', 'onehot') for r in table[wrong, f]), wrong


def test_reachable_stage0_tiles():
    """every tile pick_gemm2_tile can return for deconv1 (K = 4 D) and deconv2 (K = 1024) of 1-400 crops is in the list the device test runs, and nothing else is"""
    from easy_vitpose_amd import _capi as capi
    lib = capi.load_library()
    seen = set()
    for n in range(1, 401):
        for D in (384, 768, 1024, 1280):
            seen.add(lib.vp_dbg_gemm2_pick(4, 192 * n, 256, 4 * D, None))
        seen.add(lib.vp_dbg_gemm2_pick(4, 768 * n, 256, 1024, None))
    assert seen == set(HC.STAGE0_TILES), seen
    assert HC.FUSED_TILE not in seen
    assert hasattr(lib, 'vp_dbg_head_case') and lib.vp_dbg_head_case.argtypes is not None
