"""CPU: the attention cases of tests/attention_cases.py keep their promises, a float32 model of the kernel's arithmetic stays inside the per-element bound,
and wrong kernels -- mutations of that model -- are caught by the checks tests/test_gpu_attention.py applies to the device's output.

The model is the arithmetic of the attention core (csrc/attn_core.h, the one definition every attention kernel runs): S in fp32, p = exp2(fma(s, c, -fl(max c))) with c = hd^-1/2 log2(e), l summed from the unrounded p, P rounded to the
16-bit type, PV in fp32, one rounding of o / l.  Its summation order is numpy's, not the MFMA's: the bound does not depend on the order.

One mutation the issue lists is NOT caught, and cannot be by a per-element bound of this form: l summed from the ROUNDED P.  With P~_k = p_k (1 + e_k),
|e_k| <= u, the mutant returns sum P~ v / sum P~, and  sum P~_k (v_k - ref) / sum P~  =  sum p_k e_k (v_k - ref) / sum P~  is at most u (mag + |ref|) / (1 - u):
the two u terms of the bound, which the correct kernel is entitled to.  (It is the better-conditioned quotient, if anything.)  The exact expectations do not
see it either: in ONEHOT / EDGE / FLAT every P is 0 or rounds to exactly 1.  test_l_from_rounded_p_is_inside_the_bound states that instead of asserting a catch."""
import numpy as np
import pytest

import attention_cases as AC
from easy_vitpose_amd import _capi as capi

F32 = np.float32
SHAPES = [(384, 12), (768, 12), (1280, 16)]
DROP, DOUBLE, SWAP = 77, 141, (9, 100)          # the keys the mutations touch (SWAP: two keys of different 32-key blocks)


def model_slab(dtype, q, k, v, mut=None):
    hd = q.shape[1]
    c = F32(F32(1.0 / np.sqrt(F32(hd))) * F32(AC.LOG2E))
    if mut == 'scale64':
        c = F32(F32(0.125) * F32(AC.LOG2E))
    s = q @ k.T                                                       # fp32
    mb = np.zeros((AC.T, 1), F32) if mut == 'no_max' else (s.max(1, keepdims=True) * c).astype(F32)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        arg = (s.astype(np.float64) * np.float64(c) - mb).astype(F32)     # the fma: one rounding (float64 holds the 48-bit product)
        p = np.exp2(arg.astype(np.float64)).astype(F32)
        pr = AC.round_to(p, dtype)
        l = (pr if mut == 'l_rounded' else p).sum(1, keepdims=True, dtype=F32)
        if mut == 'drop_key':
            pr[:, DROP] = 0
            l = l - p[:, DROP:DROP + 1]
        if mut == 'double_key':
            pr[:, DOUBLE] *= 2
            l = l + p[:, DOUBLE:DOUBLE + 1]
        vv = v
        if mut == 'swap_pv':
            vv = v.copy()
            vv[list(SWAP)] = v[list(SWAP[::-1])]
        o = pr @ vv
        return AC.round_to(o * (F32(1.0) / l), dtype)


def model(case, mut=None):
    out = np.empty(case.ref.shape, F32)
    for b in range(case.B):
        for h in range(case.heads):
            out[b * AC.T:(b + 1) * AC.T, h * case.hd:(h + 1) * case.hd] = model_slab(case.dtype, *case.slab(b, h), mut)
    return out


def failures(case, got):
    """the scenarios whose checks (those of the device test) reject `got`"""
    bad = set()
    ratio = AC.worst_ratio(case, got)
    bad.update(n for n, r in ratio.items() if not r <= 1.0)
    mask, exp = case.exact()
    wrong = mask & ~(got == exp)
    bad.update(AC.NAMES[s] for s in np.unique(case.scen_el[wrong]))
    return bad, ratio


@pytest.fixture(scope='module', params=[(dt, D, h) for dt in ('fp16', 'bf16') for D, h in SHAPES], ids=lambda p: f'{p[0]}-{p[1]}')
def case(request):
    return AC.case(request.param[0], 3, *request.param[1:])


def test_conditions(case):
    AC.check_conditions(case)


def test_every_scenario_sits_in_the_remapped_groups_and_their_tail():
    """head dim 32 / 80 walk (crop, head) ids in groups of 32 with a plain tail (36 = 32 + 4 slabs at 12 heads, 48 = 32 + 16 at 16): four tail slabs are four
    scenarios at 12 heads, so the tail is required to hold several scenarios and every scenario several slabs of the groups"""
    for heads in (12, 16):
        ids = np.arange(3 * heads)
        scen = ids % AC.N_SCEN
        body = ids < len(ids) // 32 * 32
        assert all((scen[body] == s).sum() >= 5 for s in range(AC.N_SCEN))
        assert len(set(scen[~body])) >= 4


def test_model_is_inside_the_bound(case):
    got = model(case)
    bad, ratio = failures(case, got)
    print(f'[attention model] {case.dtype} D={case.D}: worst err / bound ' + ', '.join(f'{n} {r:.2f}' for n, r in ratio.items()))
    assert np.isfinite(got).all()
    assert not bad, (bad, ratio)


CAUGHT_BY = {'no_max': {'onehot', 'hot'}, 'drop_key': {'flat', 'onehot'}, 'double_key': {'flat'}, 'swap_pv': {'onehot', 'edge'}, 'scale64': {'gauss', 'mixed'}}


@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_scale_of_head_dim_64_at_80_is_caught(dtype):
    bad, ratio = failures(AC.case(dtype, 3, 1280, 16), model(AC.case(dtype, 3, 1280, 16), 'scale64'))
    assert CAUGHT_BY['scale64'] <= bad, (bad, ratio)


@pytest.mark.parametrize('mut', ['no_max', 'drop_key', 'double_key', 'swap_pv'])
def test_mutation_is_caught(case, mut):
    bad, ratio = failures(case, model(case, mut))
    print(f'[attention model] {case.dtype} D={case.D} {mut}: caught by {sorted(bad)}')
    assert CAUGHT_BY[mut] <= bad, (mut, bad, ratio)


def test_l_from_rounded_p_is_inside_the_bound(case):
    """see the module docstring: no check of this form can tell this mutant from the kernel"""
    bad, ratio = failures(case, model(case, 'l_rounded'))
    assert not bad, (bad, ratio)


def test_fused_operands_meet_their_conditions_and_the_model_its_bound():
    """the smallest shape of the fused test (the others are checked on the device box before their launch).  These operands are what the eta sub term of the bound
    is for: the model stays inside the bound with it and leaves the relative terms alone behind (fp16 subnormal p against V of the order of 10^3)"""
    dtype, D, heads = 'fp16', 768, 12
    x, W, bias = AC.fused_operands(dtype, D, heads, 6)
    full, stored = AC.fused_qkv64(dtype, x, W, bias)
    AC.check_fused_conditions(dtype, D, heads, full, stored)
    worst = worst_rel = 0.0
    for b in range(0, stored.shape[0] // AC.T, 5):
        for h in range(heads):
            q, k, v = (stored[b * AC.T:(b + 1) * AC.T, i * D + h * 64:i * D + (h + 1) * 64] for i in range(3))
            ref, mag, lam, _, sub = AC.reference(q, k, v, dtype)
            err = np.abs(model_slab(dtype, q, k, v) - ref)
            worst = max(worst, (err / AC.bound(dtype, ref, mag, lam[:, None], sub)).max())
            worst_rel = max(worst_rel, (err / AC.bound(dtype, ref, mag, lam[:, None], 0.0)).max())
    print(f'[attention model] fused operands: worst err / bound {worst:.2f} (without the subnormal-p term {worst_rel:.2f})')
    assert worst <= 1.0 < worst_rel


@pytest.mark.parametrize('dtype,D,heads,flags,why', [
    ('fp16', 384, 12, 2, 'blocked qkv at head dim 32'), ('bf16', 1280, 16, 3, 'blocked qkv at head dim 80'), ('fp16', 384, 12, 4, 'MXFP8 at head dim 32'),
    ('fp16', 1280, 16, 4, 'MXFP8 at head dim 80'), ('bf16', 768, 12, 4, 'MXFP8 with bf16'), ('fp16', 768, 12, 5, 'MXFP8 with the query split'),
    ('fp16', 768, 12, 7, 'MXFP8 with the query split, blocked'), ('fp16', 768, 12, 8, 'an unknown flag'), ('fp16', 768, 16, 0, 'head dim 48')])
def test_tap_refuses_what_has_no_kernel(dtype, D, heads, flags, why):
    """vp_dbg_attention_case answers VP_ERR_INVALID before it touches a device (so this runs anywhere): the list of variants tests/test_gpu_attention.py cannot run"""
    qkv, out, sc = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.uint8)
    rc = capi.load_library().vp_dbg_attention_case(0, capi.DTYPES[dtype], 1, D, heads, flags, qkv.ctypes.data, out.ctypes.data, sc.ctypes.data)
    assert rc == capi.VP_ERR_INVALID, why
