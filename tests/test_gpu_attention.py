"""GPU: the attention core in every variant (csrc/attention.hip through vp_dbg_attention_case; the fused kernels of csrc/qkvattn.hip and csrc/gemm8.hip through
vp_dbg_qkvattn) on the adversarial cases of tests/attention_cases.py, against float64 with a bound PER ELEMENT and, where the output is known exactly, bit for bit.
tests/test_attention_cases_host.py shows on the CPU that these checks reject wrong kernels (no max-subtraction, a key dropped / doubled / swapped, a wrong scale).

Domain: base-2 logits within +-2^10 (asserted before every launch; see tests/attention_cases.py for what lies beyond).
Variants the launcher has no kernel for, which the tap refuses (tests/test_attention_cases_host.py::test_tap_refuses_what_has_no_kernel): the blocked qkv
layout and the MXFP8 output off head dim 64; MXFP8 with bf16; MXFP8 with the query split.  The tap's output buffer is filled with 0xFF bytes before the launch, so an
element no workgroup wrote arrives as NaN and fails the first assertion."""
import functools

import numpy as np
import pytest

import attention_cases as AC
from easy_vitpose_amd import _capi as capi

pytestmark = pytest.mark.gpu
B = 3
QSPLIT, BLOCKED, MX = 1, 2, 4


def _ptr(a):
    return None if a is None else a.ctypes.data


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(dtype, nb, D, heads, flags, qkv):
    """the tap: out [nb 192, D] (+ the E8M0 bytes [nb 192, D / 32] with MX)"""
    out = np.empty((nb * AC.T, D), np.float32)
    sc = np.empty((nb * AC.T, D // 32), np.uint8) if flags & MX else None
    capi.check(capi.load_library().vp_dbg_attention_case(0, capi.DTYPES[dtype], nb, D, heads, flags, _ptr(np.ascontiguousarray(qkv)), _ptr(out), _ptr(sc)))
    return (out, sc) if flags & MX else out


@functools.lru_cache(maxsize=None)
def plain(dtype, D, heads):
    """flags 0 on the shared case of a shape: run once, compared against by the other variants"""
    case = AC.case(dtype, B, D, heads)
    AC.check_conditions(case)
    out = run(dtype, B, D, heads, 0, case.qkv)
    out.setflags(write=False)
    return out


def check_against_fp64(case, got, tag):
    ratio = AC.worst_ratio(case, got)
    print(f'[attention] {tag}: worst err / bound ' + ', '.join(f'{n} {r:.3f}' for n, r in ratio.items()))
    assert np.isfinite(got).all(), f'{tag}: {(~np.isfinite(got)).sum()} outputs are not finite (0xFF fill = never written, or an overflow)'
    mask, exp = case.exact()
    wrong = mask & (got != exp)
    assert not wrong.any(), f'{tag}: {wrong.sum()} of {mask.sum()} exactly-known outputs differ; first at {np.argwhere(wrong)[0]}: got {got[wrong][0]}, expected {exp[wrong][0]}'
    assert all(r <= 1.0 for r in ratio.values()), f'{tag}: beyond the per-element bound: {ratio}'


@pytest.mark.parametrize('flags', [0, QSPLIT])
@pytest.mark.parametrize('D,heads', [(384, 12), (768, 12), (1280, 16)])
@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_attention_cases_against_fp64(dtype, D, heads, flags):
    """Every scenario on every head dim, plain and query-split: all outputs finite, |got - ref| within the derived bound on EVERY element (FLAT without the
    P-rounding term), ONEHOT / EDGE equal to the V row (or the mean of the tied pair) exactly.  The split kernel must also repeat the plain one bit for bit."""
    case = AC.case(dtype, B, D, heads)
    ref_run = plain(dtype, D, heads)
    got = ref_run if flags == 0 else run(dtype, B, D, heads, flags, case.qkv)
    check_against_fp64(case, got, f'{dtype} D={D} heads={heads} flags={flags}')
    assert np.array_equal(_bits(got), _bits(ref_run)), f'{(_bits(got) != _bits(ref_run)).sum()} outputs differ from the plain kernel'


@pytest.mark.parametrize('flags', [BLOCKED, BLOCKED | QSPLIT])
@pytest.mark.parametrize('D,heads', [(768, 12), (1024, 16)])
@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_blocked_qkv_layout_is_bit_identical(dtype, D, heads, flags):
    """qkv in the 64 x 64-blocked layout (the production default at head dim 64; the tap re-tiles from the layout's definition): the same operands, so the
    same bits as the row-major kernel.  3 crops = 9 blocks of 64 rows: a crop's 192 keys are three blocks, the crops' blocks differ."""
    case = AC.case(dtype, B, D, heads)
    ref_run = plain(dtype, D, heads)
    got = run(dtype, B, D, heads, flags, case.qkv)
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(ref_run)), f'{(_bits(got) != _bits(ref_run)).sum()} of {got.size} outputs differ from the row-major kernel'
    if D == 1024 and flags == BLOCKED:            # (1024, 16) is not among the fp64 shapes above: checked here, once
        check_against_fp64(case, got, f'{dtype} D={D} heads={heads} flags={flags}')


@pytest.mark.parametrize('flags', [MX, MX | BLOCKED])
def test_mxfp8_output(flags):
    """The fp8 mode's output stage (fp16, head dim 64): e4m3 codes + one E8M0 byte per 32 columns.  With b the bound of the 16-bit kernel and blk the block scale the
    reference's amax asks for:  |deq - ref| <= b + (|ref| + b) 2^-4 (e4m3: three mantissa bits) + 2 blk 2^-10 (its subnormal spacing 2^-9 blk, one binade of
    slack for a block whose amax sits at a power of two).  The scale byte itself is pinned wherever the reference amax is further than b from a power of two.
    ONEHOT / EDGE: the quantised expected rows, exactly -- up to the one thing that is not exact there: the row's common factor 1 / l = 1 -+ 2^-14.5 (the domain
    note of attention_cases.py), applied BEFORE the quantisation here.  An element whose code, or whose block's scale, changes between the factors 1 - 2^-13 and
    1 + 2^-13 may take either value."""
    from test_gpu_fp8 import _mx_qdq
    dtype, D, heads = 'fp16', 768, 12
    case = AC.case(dtype, B, D, heads)
    AC.check_conditions(case)
    deq, sc = run(dtype, B, D, heads, flags, case.qkv)
    assert np.isfinite(deq).all(), f'{(~np.isfinite(deq)).sum()} outputs are not finite (never written?)'
    b = case.bound()
    _, blk = _mx_qdq(case.ref.astype(np.float32))
    blk_el = np.repeat(blk, 32, axis=1)
    lim = b + (np.abs(case.ref) + b) * 2.0 ** -4 + 2 * blk_el * 2.0 ** -10
    ratio = np.abs(deq - case.ref) / lim
    print(f'[attention] MXFP8 flags={flags}: worst err / bound ' + ', '.join(f'{AC.NAMES[s]} {ratio[case.scen_el == s].max():.3f}' for s in range(AC.N_SCEN)))
    assert (ratio <= 1.0).all(), f'{(ratio > 1).sum()} outputs beyond the bound, worst {ratio.max():.3f}'
    # the scale bytes
    M = B * AC.T
    amax = np.abs(case.ref).reshape(M, D // 32, 32).max(-1)
    bb = b.reshape(M, D // 32, 32).max(-1)
    p2 = np.exp2(np.floor(np.log2(amax)))
    clear = (amax - bb > p2) & (amax + bb < 2 * p2)
    want = (np.log2(blk) + 127).astype(np.int64)
    assert clear.any()
    assert np.array_equal(sc[clear], want[clear]), f'{(sc[clear] != want[clear]).sum()} scale bytes differ where the reference amax is clear of a power of two'
    # the exactly-known rows
    mask, exp = case.exact()
    lo, _ = _mx_qdq(exp * np.float32(1 - 2.0 ** -13))
    mid, blk_mid = _mx_qdq(exp)
    hi, _ = _mx_qdq(exp * np.float32(1 + 2.0 ** -13))
    firm = (lo == mid) & (mid == hi)
    ok = np.where(firm, deq == mid, (deq == lo) | (deq == mid) | (deq == hi))
    assert firm[mask].any()
    assert ok[mask].all(), f'{(~ok & mask).sum()} of {mask.sum()} exactly-known outputs are not the quantised V row'
    firm_blk = firm.reshape(M, D // 32, 32).all(-1) & mask.reshape(M, D // 32, 32).all(-1)
    assert np.array_equal(sc[firm_blk], (np.log2(blk_mid) + 127).astype(np.int64)[firm_blk])
    if flags & BLOCKED:
        plain_mx, plain_sc = run(dtype, B, D, heads, MX, case.qkv)
        assert np.array_equal(_bits(deq), _bits(plain_mx)) and np.array_equal(sc, plain_sc), 'the blocked qkv layout changes the MXFP8 output'


@pytest.mark.parametrize('dtype,D,heads,npairs', [('fp16', 1280, 16, 8), ('bf16', 1280, 16, 9), ('fp16', 768, 12, 6)])
def test_fused_kernels_on_hot_operands(dtype, D, heads, npairs):
    """attn.qkv + attention in one kernel (head dim 80: gemm8.hip's EPI_QKV_ATTN tile, head dim 64: qkvattn.hip) on operands that reach what Gaussian ones do not:
    in fp16 the k and v the GEMM phase hands over leave +-65504 (the hand-over saturates, as the GEMM epilogue does), base-2 logits beyond 150, most rows one-hot.
    Equal to vp_dbg_gemm (epi 0) + the attention tap bit for bit, run to run, and inside the per-element bound of the float64 attention of the GEMM tap's qkv."""
    M, hd = npairs * 384, D // heads
    x, W, bias = AC.fused_operands(dtype, D, heads, npairs)
    full, stored = AC.fused_qkv64(dtype, x, W, bias)
    AC.check_fused_conditions(dtype, D, heads, full, stored)
    lib = capi.load_library()
    fused = np.empty((M, D), np.float32)
    capi.check(lib.vp_dbg_qkvattn(0, capi.DTYPES[dtype], npairs, D, heads, _ptr(x), _ptr(W), _ptr(bias), _ptr(fused)))
    qkv = np.empty((M, 3 * D), np.float32)
    capi.check(lib.vp_dbg_gemm(0, capi.DTYPES[dtype], 0, M, 3 * D, D, _ptr(x), _ptr(W), _ptr(bias), None, _ptr(qkv)))
    assert np.isfinite(qkv).all()
    if dtype == 'fp16':
        assert (np.abs(qkv[:, D:2 * D]) == 65504).any() and (np.abs(qkv[:, 2 * D:]) == 65504).any(), 'nothing saturated at the hand-over'
    two = run(dtype, M // AC.T, D, heads, 0, qkv)
    assert np.isfinite(fused).all(), f'{(~np.isfinite(fused)).sum()} outputs are not finite'
    assert np.array_equal(_bits(fused), _bits(two)), f'{(_bits(fused) != _bits(two)).sum()} of {fused.size} outputs differ from gemm + attention'
    again = np.empty_like(fused)
    capi.check(lib.vp_dbg_qkvattn(0, capi.DTYPES[dtype], npairs, D, heads, _ptr(x), _ptr(W), _ptr(bias), _ptr(again)))
    assert np.array_equal(_bits(fused), _bits(again)), 'run-to-run difference'
    worst = 0.0
    for b in range(M // AC.T):
        rows = slice(b * AC.T, (b + 1) * AC.T)
        for h in range(heads):
            q, k, v = (qkv[rows, i * D + h * hd:i * D + (h + 1) * hd] for i in range(3))
            ref, mag, lam, lg, sub = AC.reference(q, k, v, dtype)
            assert np.abs(lg).max() <= AC.LOGIT_MAX
            lim = AC.bound(dtype, ref, mag, lam[:, None], sub)
            worst = max(worst, (np.abs(fused[rows, h * hd:(h + 1) * hd] - ref) / lim).max())
    print(f'[attention] fused {dtype} D={D} npairs={npairs}: worst err / bound {worst:.3f}')
    assert worst <= 1.0
