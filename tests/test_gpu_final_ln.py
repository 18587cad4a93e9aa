"""GPU: the standalone LayerNorm pass as the default path launches it for last_norm (vp_dbg_layernorm_planes: layernorm_kernel<Ty, PLANES = true> on the two-plane
residual stream, plane = plane_rows * D of the PADDED batch, M <= plane_rows rows normalised) on every row family of tests/ln_consumer_cases.py, D = 384 / 768 /
1024 / 1280, fp16 and bf16, per element against the float64 LayerNorm of v = hi + lo within the bound of tests/final_ln_model.py (derived there from the kernel's
operations, pinned on the CPU by tests/test_final_ln_host.py).  Also: out16 == round16(out32) bit for bit; a row gives the same bits at every row position; rows
>= M stay unwritten and the 0xFFFF codes in the plane rows behind M influence nothing; and vp_dbg_layernorm (PLANES = false) on v -- hi + lo is exact in float32
on these rows -- gives the same bits, so the plain kernel runs the same families against the same bound."""
import numpy as np
import pytest

import final_ln_model as FM
import ln_consumer_cases as LC
import patch_gather_model as PM
import residual_row_model as RM
from easy_vitpose_amd import _capi as capi

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _planes(dtype, M, plane_rows, D, hi, lo, g, b):
    """one vp_dbg_layernorm_planes call on rows hi / lo [M, D]; plane rows M .. plane_rows - 1 hold 0xFFFF codes -> (out16, out32) [plane_rows, D]"""
    H, L = np.full((plane_rows, D), 0xFFFF, np.uint16), np.full((plane_rows, D), 0xFFFF, np.uint16)
    H[:M], L[:M] = hi, lo
    o16, o32 = np.zeros((plane_rows, D), F32), np.zeros((plane_rows, D), F32)
    rc = capi.load_library().vp_dbg_layernorm_planes(0, capi.DTYPES[dtype], M, plane_rows, D, H.ctypes.data, L.ctypes.data, g.ctypes.data, b.ctypes.data,
                                                     o16.ctypes.data, o32.ctypes.data)
    assert rc == 0, capi.last_error()
    return o16, o32


def _plain(dtype, v, g, b):
    v = np.ascontiguousarray(v, F32)
    o16, o32 = np.zeros_like(v), np.zeros_like(v)
    capi.check(capi.load_library().vp_dbg_layernorm(0, capi.DTYPES[dtype], v.shape[0], v.shape[1], v.ctypes.data, g.ctypes.data, b.ctypes.data, o16.ctypes.data, o32.ctypes.data))
    return o16, o32


def _positions(R):
    """row order of the launch: every case row at two positions (24 rows: the wave slots, position % 4, differ), to a count that is not a multiple of 4"""
    idx = np.concatenate([np.arange(R), np.roll(np.arange(R), 1), [0]])
    if len(idx) % 4 == 0:
        idx = np.concatenate([idx, [1]])
    return idx


@pytest.mark.parametrize('D', FM.DS)
@pytest.mark.parametrize('dtype', LC.DTYPES)
def test_final_layernorm(dtype, D):
    R = LC.rows(dtype, D)
    fam = np.array(R['family'])
    idx = _positions(len(fam))
    M = len(idx)
    assert M % 4 and set(idx) == set(range(len(fam)))
    hi, lo, v = R['hi'][idx], R['lo'][idx], R['v'][idx]
    for kind in FM.AFFINES:
        g, b = FM.affine(D, kind)
        ref, bnd = FM.reference(R['v'], g, b)[0], FM.bound(R['v'], g, b)
        o16, o32 = _planes(dtype, M, M, D, hi, lo, g, b)
        # per element inside the bound; the worst ratio per family
        r = FM.ratio(o32, ref[idx], bnd[idx]).max(-1)
        worst = {f: float(r[fam[idx] == f].max()) for f in LC.FAMILIES}
        print(f'[final ln {dtype} D={D} {kind}] worst |err| / bound per family (C = {FM.C_BOUND}):', {f: round(x, 3) for f, x in worst.items()})
        assert r.max() <= 1.0, (kind, fam[idx][int(r.argmax())], r.max())
        # the 16-bit output is the fp32 one rounded once
        assert np.array_equal(_bits(o16), _bits(RM.from_bits(PM.to16(o32, dtype), dtype))), 'out16 != round16(out32)'
        # the same row, the same bits, wherever it stands
        first = {int(i): p for p, i in reversed(list(enumerate(idx)))}
        for p, i in enumerate(idx):
            assert np.array_equal(_bits(o32[p]), _bits(o32[first[int(i)]])), f'row {i} ({fam[i]}) differs between positions {first[int(i)]} and {p}'
        # a padded plane: rows >= M unwritten, the 0xFFFF codes behind M without influence
        p16, p32 = _planes(dtype, M, M + 7, D, hi, lo, g, b)
        assert np.array_equal(_bits(p32[:M]), _bits(o32)) and np.array_equal(_bits(p16[:M]), _bits(o16)), 'plane_rows = M + 7 changes the result'
        assert (_bits(p32[M:]) == 0xFFFFFFFF).all() and np.isnan(p16[M:]).all(), 'a row >= M was written'
        # one row alone
        for i in (0, len(fam) - 1):
            for pr in (1, 8):
                s16, s32 = _planes(dtype, 1, pr, D, R['hi'][i:i + 1], R['lo'][i:i + 1], g, b)
                assert np.array_equal(_bits(s32[0]), _bits(o32[first[i]])) and np.array_equal(_bits(s16[0]), _bits(o16[first[i]])), (i, pr)
                assert (_bits(s32[1:]) == 0xFFFFFFFF).all()
        # the plain kernel on v = hi + lo: the same bits, hence the same families inside the same bound
        q16, q32 = _plain(dtype, v, g, b)
        assert np.array_equal(_bits(q32), _bits(o32)) and np.array_equal(_bits(q16), _bits(o16)), 'PLANES = false on hi + lo differs from the planes kernel'
        assert FM.ratio(q32, ref[idx], bnd[idx]).max() <= 1.0


def test_refusals():
    D = 384
    R = LC.rows('fp16', D)
    g, b = FM.affine(D, 'identity')
    lib = capi.load_library()
    o = np.zeros((4, D), F32)
    for M, pr, d in ((2, 1, D), (0, 4, D), (2, 4, 386), (2, 4, 1284)):
        assert lib.vp_dbg_layernorm_planes(0, capi.DTYPES['fp16'], M, pr, d, R['hi'].ctypes.data, R['lo'].ctypes.data, g.ctypes.data, b.ctypes.data, o.ctypes.data,
                                           o.ctypes.data) != 0, (M, pr, d)
