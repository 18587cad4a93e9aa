"""GPU: the patch gather alone (vp_dbg_im2col: im2col_kernel plain and FLIP, im2col_twin_kernel; fp16 / bf16 x fp32-NCHW / u8-NHWC input = twelve instantiations)
against the host model (tests/patch_gather_model.py, pinned on the CPU by tests/test_patch_gather_host.py) BIT FOR BIT on the cases of tests/patch_gather_cases.py:
the conv's zero border, the column order, the mirror and the twin's backwards read, the source crop of padding rows and the twin's odd tail, the conversion's
rounding edges and fp16 clamp, every byte phase of the u8 unpack.  The device output is 0xFF-filled before the launch and followed by one output crop of guard
elements: no 0xFFFF code may be left (no case rounds to a NaN code), no guard byte touched.  Then the patch embed as a whole: the tap's output through the
EPI_POS_LN GEMM against the fp64 convolution of the rounded operands."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import patch_gather_cases as PC
import patch_gather_model as PM
from easy_vitpose_amd import _capi as capi

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
FMT = {'f32': 0, 'u8': 1}                                  # VP_INPUT_F32_NCHW / VP_INPUT_U8_NHWC
SHAPES = {0: ((1, 1), (3, 3), (4, 2)), 1: ((1, 1), (3, 3), (4, 2)), 2: ((2, 1), (5, 2), (6, 2))}
GUARD = 192 * 768


def _tap(dtype, fmt, mode, B, n_src, crops):
    """one vp_dbg_im2col call -> (rc, codes [B * 192, 768], guard bytes)"""
    crops = np.ascontiguousarray(crops[:max(n_src, 1)])
    out = np.zeros((B * 192, 768), np.uint16)
    guard = np.zeros(GUARD * 2, np.uint8)
    rc = capi.load_library().vp_dbg_im2col(0, capi.DTYPES[dtype], fmt, mode, B, n_src, crops.ctypes.data, out.ctypes.data, guard.ctypes.data)
    return rc, out, guard


def _ok(dtype, fmt, mode, B, n_src, crops):
    rc, out, guard = _tap(dtype, fmt, mode, B, n_src, crops)
    what = f'{dtype} fmt {fmt} mode {mode} B {B} n_src {n_src}'
    assert rc == 0, (what, capi.last_error())
    assert not (out == 0xFFFF).any(), f'{what}: {(out == 0xFFFF).sum()} codes unwritten'
    assert (guard == 0xFF).all(), f'{what}: {(guard != 0xFF).sum()} guard bytes overwritten'
    return out


def _inputs(dtype, fmt):
    """case name -> (what the tap is fed, the codes [3, 3, 256, 192] the model gathers)"""
    if fmt == 'f32':
        return {k: (v, PM.to16(v, dtype)) for k, v in PC.f32_cases(dtype).items()}
    return {k: (v, PM.to16(PM.nchw(PM.normalise_u8(v)), dtype)) for k, v in PC.u8_cases().items()}


def _first_diff(got, ref):
    m, k = np.argwhere(got != ref)[0]
    return (f'{(got != ref).sum()} of {ref.size} codes differ; first at crop {m // 192} patch ({m % 192 // 12}, {m % 12}) column c {k // 256} ky {k % 256 // 16} kx {k % 16}: '
            f'{got[m, k]:#06x} != {ref[m, k]:#06x}')


@pytest.mark.parametrize('mode', (0, 1, 2))
@pytest.mark.parametrize('fmt', ('f32', 'u8'))
@pytest.mark.parametrize('dtype', PC.DTYPES)
def test_gather_bit_for_bit(dtype, fmt, mode):
    for case, (x, bits) in _inputs(dtype, fmt).items():
        for B, n_src in SHAPES[mode]:
            got = _ok(dtype, FMT[fmt], mode, B, n_src, x)
            ref = PM.gather(bits, B, n_src, mode)
            assert np.array_equal(got, ref), f'{dtype} {fmt} mode {mode} {case} B {B} n_src {n_src}: {_first_diff(got, ref)}'
        assert np.array_equal(_ok(dtype, FMT[fmt], mode, B, n_src, x), got), f'{case}: run-to-run difference'


@pytest.mark.parametrize('fmt', ('f32', 'u8'))
@pytest.mark.parametrize('dtype', PC.DTYPES)
def test_twin_is_the_straight_and_the_mirrored_gather(dtype, fmt):
    """mode 2's even output crops equal mode 0's, its odd ones mode 1's: on the device's own outputs"""
    x = _inputs(dtype, fmt)['edges' if fmt == 'f32' else 'allbytes'][0]
    for B, n_src in SHAPES[2]:
        twin = _ok(dtype, FMT[fmt], 2, B, n_src, x).reshape(B, 192 * 768)
        straight = _ok(dtype, FMT[fmt], 0, n_src, n_src, x).reshape(n_src, -1)
        mirrored = _ok(dtype, FMT[fmt], 1, n_src, n_src, x).reshape(n_src, -1)
        for b in range(B):
            r = min(b, 2 * n_src - 1)
            assert np.array_equal(twin[b], (mirrored if r & 1 else straight)[r >> 1]), (B, n_src, b)


@pytest.mark.parametrize('mode', (0, 1, 2))
@pytest.mark.parametrize('dtype', PC.DTYPES)
def test_u8_input_is_the_fp32_input_of_its_normalisation(dtype, mode):
    B, n_src = SHAPES[mode][1]
    for case, u8 in PC.u8_cases().items():
        a = _ok(dtype, FMT['u8'], mode, B, n_src, u8)
        b = _ok(dtype, FMT['f32'], mode, B, n_src, PM.nchw(PM.normalise_u8(u8)))
        assert np.array_equal(a, b), f'{dtype} mode {mode} {case}: {_first_diff(a, b)}'


def test_refusals():
    x = PC.f32_cases('fp16')['gauss']
    for args in ((0, 2, 3, 2), (0, 2, 1, 1), (7, 0, 2, 2), (7, 2, 2, 1), (0, 3, 2, 2), (0, 0, 0, 1), (0, 0, 2, 0), (0, 0, 2, 3)):   # (fmt, mode, B, n_src)
        rc, out, guard = _tap('fp16', *args, x)
        assert rc != 0, args
        assert (out == 0).all() and (guard == 0).all()      # nothing came back


@pytest.mark.parametrize('dtype', PC.DTYPES)
def test_patch_embed_as_a_whole(dtype):
    """tap -> EPI_POS_LN GEMM (tiles 9 and 8) against the fp64 conv2d of the rounded operands + pos, at the tolerances of test_patch_embed_epilogue_with_statistics"""
    import residual_row_model as RM
    B, D = 2, 384
    rng = np.random.default_rng(D + (dtype == 'bf16'))
    x = PC.f32_cases(dtype)['gauss'][:B]
    A = RM.from_bits(_ok(dtype, 0, 0, B, B, x), dtype)                                     # [B * 192, 768], already of the operand type
    W = RM.from_bits(RM.to_bits((rng.standard_normal((D, 768)) * 0.02).astype(F32), dtype), dtype)
    pos = (rng.standard_normal((192, D)) * 0.5).astype(F32)
    bias = np.zeros(D, F32)
    x16 = RM.from_bits(PM.to16(x, dtype), dtype).astype(F64)
    conv = F.conv2d(torch.from_numpy(x16), torch.from_numpy(W.astype(F64).reshape(D, 3, 16, 16)), stride=16, padding=2).numpy()
    ref = conv.transpose(0, 2, 3, 1).reshape(B * 192, D) + np.tile(pos.astype(F64), (B, 1))
    first = None
    for variant in (9, 8):
        o, st = np.empty((B * 192, D), F32), np.empty((B * 192, D // 64, 2), F32)
        rc = capi.load_library().vp_dbg_gemm_case(0, capi.DTYPES[dtype], 7, variant, 0, 0, B * 192, D, 768, A.ctypes.data, W.ctypes.data, bias.ctypes.data, pos.ctypes.data,
                                                  None, None, o.ctypes.data, st.ctypes.data)
        assert rc == 0, capi.last_error()
        err = np.abs(o - ref).max()
        print(f'[patch embed {dtype} cfg{variant}] max |err| {err:.3e} (allowed {2e-5 * max(1.0, np.abs(ref).max()):.3e})')
        assert err < 2e-5 * max(1.0, np.abs(ref).max())
        g = o.astype(F64).reshape(B * 192, D // 64, 64)
        assert np.abs(st[..., 0] - g.sum(-1)).max() < 2e-3
        if first is None:
            first = (o, st)
        assert np.array_equal(o, first[0]) and np.array_equal(st, first[1]), f'patch embed: cfg{variant} differs from cfg9'
