"""GPU: csrc/gemm8f.hip, the 8-phase GEMM on MXFP8 operands behind dtype='fp8', against exact host models (tests/fp8_gemm_model.py; the problems are
tests/fp8_gemm_cases.py, both pinned on the CPU by tests/test_fp8_gemm_model.py, where every assertion below is also shown to fail on a mutated model).
Shapes are (M, N, K) with K the reduction depth.

A. Tile hand-over.  launch8f starts min(tiles, 256) workgroups, so only a launch of more than 256 tiles gives a workgroup a second tile: ktile(swB = true),
   the scale dwords fetched ahead for the next tile, ring_start() behind the LDS-staged residual epilogue, the pinned scale registers.  All four kernel
   instances at 288 / 384 / 528 tiles, K = 512 (nk = 4: no steady-state iteration) and 768 (one), on operands whose every scale dword differs from the ones
   a lane could fetch instead by a power of two.  The large launch equals launches of at most 255 tiles of the same rows BIT FOR BIT (outputs, planes,
   granule statistics, codes, scale bytes), repeats itself bit for bit, and meets test_gpu_fp8.py's fp64 bounds on rows of a workgroup's first, second and
   third tile.  The tile is the one the mode's own rule picks (asserted), for the large launch and for every small one.
B. mlp.fc1's epilogue, per element on raw bytes: GELU, the amax over the lane pair, the E8M0 byte, the e4m3 codes, the two layouts.  B1 knows the float32
   pre-activation exactly (A = 0 or one exact product per row) and runs the families of fp8_gemm_cases.FAMILIES; B2 is a Gaussian product known to the
   accumulation bound.  B3: every byte written, every element where tests/test_gpu_ops.py::_mx_layout (not the header) says it is.
C. attn.qkv's store: small integers, exact on every bit, row-major and in the 64 x 64-blocked layout the mode's forward uses at head dim 64; the blocked
   store again on A's 288- and 528-tile launches."""
import numpy as np
import pytest

import fp8_gemm_cases as FC
import fp8_gemm_model as FM
from easy_vitpose_amd import _capi as capi
from test_gpu_ops import _mx_layout

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def _ptr(a):
    return None if a is None else a.ctypes.data


def _pick(epi, M, N):
    v = np.zeros(2, np.int32)
    assert capi.load_library().vp_dbg_gemm_fp8_pick(epi, M, N, v[:1].ctypes.data, v[1:].ctypes.data) == 0
    return int(v[0]), int(v[1])


def _raw(epi, A, W, bias, flags=0, deq=True, raw_out=False, a_scales=False):
    """one launch through vp_dbg_gemm_fp8_case_raw (epi 0 / 1) -> dict out [M, N] (epi 0 with flags = 1: device order), a_deq, w_deq, codes, scales, a_scales"""
    M, K = A.shape
    N = W.shape[0]
    r = dict(out=np.empty((M, N), F32))
    if deq:
        r['a_deq'], r['w_deq'] = np.empty((M, K), F32), np.empty((N, K), F32)
    if raw_out:
        r['codes'], r['scales'] = np.empty(M * N, np.uint8), np.empty(M * N // 32, np.uint8)
    if a_scales:
        r['a_scales'] = np.empty(M * K // 32, np.uint8)
    A, W, bias = (np.ascontiguousarray(a, F32) for a in (A, W, bias))
    rc = capi.load_library().vp_dbg_gemm_fp8_case_raw(0, epi, M, N, K, _ptr(A), _ptr(W), _ptr(bias), None, _ptr(r['out']), None, _ptr(r.get('a_deq')),
                                                      _ptr(r.get('w_deq')), flags, _ptr(r.get('codes')), _ptr(r.get('scales')), _ptr(r.get('a_scales')))
    assert rc == 0, capi.last_error()
    return r


def _planes(A, W, bias, r_hi, r_lo, deq=True):
    """epi 6 through vp_dbg_gemm_fp8_case_planes, in place as the forward launches it -> dict hi, lo (fp16 bits), stats, a_deq, w_deq"""
    M, K = A.shape
    N = W.shape[0]
    r = dict(hi=np.empty((M, N), np.uint16), lo=np.empty((M, N), np.uint16), stats=np.empty((M, N // 64, 2), F32))
    if deq:
        r['a_deq'], r['w_deq'] = np.empty((M, K), F32), np.empty((N, K), F32)
    A, W, bias, r_hi, r_lo = (np.ascontiguousarray(a) for a in (A, W, bias, r_hi, r_lo))
    rc = capi.load_library().vp_dbg_gemm_fp8_case_planes(0, M, N, K, _ptr(A), _ptr(W), _ptr(bias), _ptr(r_hi), _ptr(r_lo), 1, _ptr(r['hi']), _ptr(r['lo']),
                                                         _ptr(r['stats']), _ptr(r.get('a_deq')), _ptr(r.get('w_deq')))
    assert rc == 0, capi.last_error()
    return r


def _launch(epi, c, m0, m1, deq):
    """rows m0 .. m1 of problem c on the epilogue's tap; the arrays that must agree bit for bit come back under 'bits'"""
    A = c['A'][m0:m1]
    if epi == 6:
        r = _planes(A, c['W'], c['bias'], c['r_hi'][m0:m1], c['r_lo'][m0:m1], deq=deq)
        r['bits'] = dict(hi=r['hi'], lo=r['lo'], stats=r['stats'].view(np.uint32))
    else:
        r = _raw(epi, A, c['W'], c['bias'], deq=deq, raw_out=epi == 1, a_scales=deq)
        r['bits'] = dict(out=r['out'].view(np.uint32))
        if epi == 1:
            r['bits'].update(codes=r['codes'], scales=r['scales'])
    return r


def _f16(bits):
    return bits.view(np.float16).astype(F64)


# ---------------------------------------------------------------------------------------------------------------- A. tile hand-over

@pytest.mark.parametrize('name,K', FC.HAND_OVER_CASES)
def test_tile_hand_over(name, K):
    """Section A of the module docstring.  The fp64 bounds are test_gpu_fp8.py's own constants for each epilogue; the small launches are bit-identical
    to the large one, so a miss of these bounds would be the instruction on this data (blocks from 2^-14 to 2^8 in one row), not the walk."""
    from test_gpu_fp8 import _gelu, _mx_qdq
    epi, M, N, bn, tiles, gm, _ = FC.HAND_OVER[name]
    assert (M // 256) * (N // bn) == tiles and tiles > 256
    assert _pick(epi, M, N) == (17 if bn == 192 else 16, gm), 'the rule of the fp8 mode picks another tile for this shape'
    n_own = FC.owners(name)
    _, walk, _ = FC.rule(name, K)
    assert len(walk) == 256 and n_own.min() >= 1 and n_own.max() == -(-tiles // 256) and (n_own >= 2).sum() >= 16
    c = FC.hand_over(name, K)
    big = _launch(epi, c, 0, M, True)

    # the operands: every block's scale byte is the rule's, so what a lane could fetch instead differs from it
    a_deq = big['a_deq']
    want = FC.expected_scale_bytes(name, K)
    _, ex = np.frexp(FM.block_amax(np.abs(a_deq)))
    assert np.array_equal(ex - 1 + 120, want), 'scale bytes read off a_deq (every amax is 1.5 2^e: code 192)'
    if 'a_scales' in big:
        assert np.array_equal(big['a_scales'][_mx_layout(M, K)[1]], want), 'scale bytes as the device holds them'
    E = want.reshape(M // 256, 256, K // 128, 4)
    nk = K // 128
    for tl in walk:
        for (a, _), (b, _) in zip(tl, tl[1:]):
            six = [E[b, :, 0], E[b, :, 1], E[a, :, 0], E[a, :, 1], E[a, :, nk - 2], E[a, :, nk - 1]]
            assert all((six[i] != six[j]).all() for i in range(6) for j in range(i)), (a, b)

    # bit identity with launches in which nobody has a second tile
    for m0, m1 in FC.chunks(name):
        t = ((m1 - m0) // 256) * (N // bn)
        assert 8 <= t <= 255 and _pick(epi, m1 - m0, N) == (17 if bn == 192 else 16, gm)
        small = _launch(epi, c, m0, m1, False)
        for k, v in small['bits'].items():
            full = big['bits'][k]
            part = full.reshape(M, -1)[m0:m1].reshape(v.shape) if full.ndim > 1 else full[m0 * (full.size // M):m1 * (full.size // M)]
            diff = part != v
            assert not diff.any(), (f'{name} K={K}: {k} of rows {m0}..{m1} differ between the {tiles}-tile launch and a {t}-tile launch in {diff.sum()} places, '
                                    f'first at {np.argwhere(diff.reshape(m1 - m0, -1))[0] + [m0, 0]}')
    # repeatability
    again = _launch(epi, c, 0, M, False)
    for k, v in again['bits'].items():
        assert np.array_equal(v, big['bits'][k]), f'{name} K={K}: {k} differs between two runs of the large launch'
    del again

    # fp64 of the operands the kernel multiplied, on rows of a workgroup's first, second (and third) tile
    rows, pos = FC.sample_rows(name)
    assert len(rows) >= 64 and set(pos) == set(range(n_own.max()))
    ref, mag = FM.product(a_deq[rows], big['w_deq'], c['bias'])
    if epi == 0:
        err = np.abs(big['out'][rows] - ref)
        tol = 2.0 ** -10 * np.abs(ref) + 1e-4 * mag + 1e-4
    elif epi == 6:
        out = _f16(big['hi'][rows]) + _f16(big['lo'][rows])
        ref = ref + _f16(c['r_hi'][rows]) + _f16(c['r_lo'][rows])
        err = np.abs(out - ref)
        tol = 2e-5 * np.maximum(1.0, np.abs(ref)) + 3e-4 * mag
        g = out.reshape(len(rows), N // 64, 64)
        st = big['stats'][rows]
        assert np.abs(st[..., 0] - g.sum(-1)).max() < 2e-3 * max(1.0, np.abs(g.sum(-1)).max() / 64)
        m2 = ((g - g.mean(-1, keepdims=True)) ** 2).sum(-1)
        assert np.abs(st[..., 1] - m2).max() < 2e-3 * max(1.0, m2.max())
    else:
        ref = _gelu(ref)
        ref_q, blk = _mx_qdq(ref.astype(F32))
        step = np.repeat(blk, 32, axis=1) * 16.0
        out = big['out'][rows]
        err, tol = np.abs(out - ref_q), step * 1.001
        frac = (err > 0).mean()
        print(f'[fp8 gemm hand-over, {name} K={K}] {frac:.2e} of the sampled elements differ from quantise(fp64 reference)')
        assert frac < 5e-3
        assert np.abs(out - ref).max() <= (np.abs(ref) * 2.0 ** -4 + np.repeat(blk, 32, axis=1) * 2.0 ** -2).max() * 1.01
    worst = (err / tol).max(1)
    print(f'[fp8 gemm hand-over, {name} K={K}] {tiles} tiles, workgroups with 1/2/3 tiles: {[int((n_own == k).sum()) for k in (1, 2, 3)]}; worst err / bound on rows of '
          + ', '.join(f'tile {p + 1}: {worst[pos == p].max():.3f}' for p in sorted(set(pos))))
    assert (err <= tol).all(), f'{name} K={K}: worst ratio {worst.max():.2f} on row {rows[worst.argmax()]} (tile {pos[worst.argmax()] + 1} of its workgroup)'

    # C: the 64 x 64-blocked store of attn.qkv on the same launch
    if epi == 0:
        blocked = _raw(0, c['A'], c['W'], c['bias'], flags=1, deq=False)['out']
        assert np.array_equal(FM.deblock64(blocked.reshape(-1), M, N).view(np.uint32), big['out'].view(np.uint32)), 'the blocked qkv store differs from the row-major one'


# ---------------------------------------------------------------------------------------------------------------- B. the fc1 epilogue

def _deblock_mx(r, M, N):
    """(scale bytes [M, N / 32], codes [M, N]) through test_gpu_ops._mx_layout; B3: every byte of both buffers was written"""
    unwritten = int(((r['codes'] & 0x7f) == 0x7f).sum()), int((r['scales'] == 0xff).sum())
    assert unwritten == (0, 0), f'{unwritten[0]} code bytes are NaN codes (0xff: never written), {unwritten[1]} scale bytes still hold the 0xff fill'
    code_off, scale_off = _mx_layout(M, N)
    assert len(np.unique(code_off)) == M * N and len(np.unique(scale_off)) == M * N // 32
    E, codes = r['scales'][scale_off], r['codes'][code_off]
    assert np.array_equal(FM.dequantise(E, codes).astype(F32), r['out']), "the tap's own de-blocking (mx8.h) and _mx_layout disagree"
    return E, codes


def _where(bad, block):
    m, n = (int(i) for i in np.argwhere(bad)[0])
    return f'first at row {m}, ' + (f'block {n} (columns {32 * n}..)' if block else f'column {n} (block {n // 32}, lane half {n % 32 // 16})')


def test_fc1_epilogue_exact_preactivations():
    """B1 + B3.  x = fma(acc, w_scale, bias) is known bit for bit; GELU's float32 value lies in mlp_model's interval centre -+ e32; the scale byte and, given
    the device's byte, every code must come from that interval.  Rows and columns all differ, so a swapped lane pair or jj, or a scale dword from the odd lane,
    is a misplaced value (CPU test: those mutants fail here)."""
    c = FC.fc1_exact()
    M, N = c['x'].shape
    assert (M // 256) * (N // 256) >= 8 and _pick(1, M, N)[0] == 16
    r = _raw(1, c['A'], c['W'], c['bias'], raw_out=True)
    assert np.array_equal(r['a_deq'].view(np.uint32), c['A'].view(np.uint32)) and np.array_equal(r['w_deq'].view(np.uint32), c['W'].view(np.uint32)), 'operands not exact'
    E, codes = _deblock_mx(r, M, N)
    lo, hi = FC.fc1_interval(c['x'])
    a = FM.accept(lo, hi, E, codes)
    fam = lambda n: FC.FAMILIES[c['family'][n]]
    assert not a['bad_scale'].any(), (f"{a['bad_scale'].sum()} scale bytes outside the model's; {_where(a['bad_scale'], True)}: family "
                                      f"{fam(np.argwhere(a['bad_scale'])[0][1])}, got {E[a['bad_scale']][0]}, model {a['E_lo'][a['bad_scale']][0]}..{a['E_hi'][a['bad_scale']][0]}")
    assert not a['bad_code'].any(), (f"{a['bad_code'].sum()} codes outside the model's interval; {_where(a['bad_code'], False)}: family "
                                     f"{fam(np.argwhere(a['bad_code'])[0][1] // 32)}, got {codes[a['bad_code']][0]:#04x}")
    open_ = (a['open_code'] | np.repeat(a['open_scale'], 32, axis=1)) & ~np.repeat(FC.exempt_blocks(c), 32, axis=1)
    print(f'[fp8 gemm fc1 exact] {M}x{N}: every scale byte and code inside the model; undecided share {open_.mean():.2e}')
    assert open_.mean() <= 0.01


@pytest.mark.parametrize('M,N,K', FC.GAUSS_SHAPES)
def test_fc1_epilogue_gaussian_product(M, N, K):
    """B2.  The pre-activation is the fp64 product of the returned operands -+ b, b = 1e-4 sum |a| |w| (the accumulation term of test_gpu_fp8.py's qkv bound, the
    column's w_scale inside w_deq) + one float32 rounding of the fma; the interval acceptance of B1 on GELU's range over it.  (Why these operands carry a mean:
    fp8_gemm_cases.fc1_gauss.)"""
    A, W, bias = FC.fc1_gauss(M, N, K)
    r = _raw(1, A, W, bias, raw_out=True)
    E, codes = _deblock_mx(r, M, N)
    pre, mag = FM.product(r['a_deq'], r['w_deq'], bias)
    b = 1e-4 * mag + 2.0 ** -23 * np.abs(pre)
    lo, hi = FC.gauss_interval(pre, b)
    a = FM.accept(lo, hi, E, codes)
    share = (a['open_code'] | np.repeat(a['open_scale'], 32, axis=1)).mean()
    print(f"[fp8 gemm fc1 gauss {M}x{N}x{K}] bad scale bytes {a['bad_scale'].sum()}, bad codes {a['bad_code'].sum()}, undecided share {share:.2e}")
    assert share <= 0.02
    assert not a['bad_scale'].any(), f"{a['bad_scale'].sum()} scale bytes outside the reference's; {_where(a['bad_scale'], True)}"
    assert not a['bad_code'].any(), f"{a['bad_code'].sum()} codes outside the reference's interval; {_where(a['bad_code'], False)}"


# ---------------------------------------------------------------------------------------------------------------- C. the qkv epilogue

@pytest.mark.parametrize('mixed', [0, 1])
def test_qkv_epilogue_exact_integers(mixed):
    """A, W, w_scale and bias are small integers times powers of two, exactly representable: every partial sum is an integer far inside float32 and the fp16
    result is the integer product on every bit -- row-major and through the 64 x 64-blocked store (de-blocked here from the layout's definition)."""
    c = FC.qkv_exact(mixed)
    M, N = c['ref'].shape
    assert _pick(0, M, N)[0] == 16
    r = _raw(0, c['A'], c['W'], c['bias'], a_scales=True)
    assert np.array_equal(r['a_deq'], c['A']) and np.array_equal(r['w_deq'], c['W']), 'operands not exact'
    assert len(np.unique(r['a_scales'])) == (3 if mixed else 1)
    wrong = r['out'] != c['ref']
    assert not wrong.any(), f"{wrong.sum()} of {wrong.size} outputs are not the integer product; {_where(wrong, False)}: got {r['out'][wrong][0]}, expected {c['ref'][wrong][0]}"
    blocked = _raw(0, c['A'], c['W'], c['bias'], flags=1, deq=False)['out']
    assert np.array_equal(FM.deblock64(blocked.reshape(-1), M, N).view(np.uint32), r['out'].view(np.uint32)), 'the blocked qkv store differs from the row-major one'
