"""CPU: the host model and the case conditions of tests/test_gpu_fp8_gemm.py (fp8_gemm_model.py, fp8_gemm_cases.py), and that each of its assertions
bites: every check is run here on a mutation of the MODEL (a scale byte from the wrong K-tile or tile, a truncating quantiser, a swapped lane pair)."""
import numpy as np
import pytest
import torch

import fp8_gemm_cases as FC
import fp8_gemm_model as FM
import ln_consumer_model as LM
import mlp_model as MM
from easy_vitpose_amd import _capi as capi

F32, F64 = np.float32, np.float64
F8 = torch.float8_e4m3fn


def _host_e4m3(x):
    x = np.ascontiguousarray(x, F32)
    got = np.empty(x.size, np.uint8)
    assert capi.load_library().vp_dbg_host_e4m3(x.ctypes.data, got.ctypes.data, x.size) == 0
    return got.reshape(x.shape)


def _w_deq(W):
    """the weight packer on the host (weights.hip::upload_fp8_rows): per-row scale max |row| / 448, codes of row / scale"""
    sn = (np.abs(W).max(1) / F32(448.0)).astype(F32)
    sn = np.where(sn > 0, sn, F32(1))
    return FM.e4m3_values()[_host_e4m3((W / sn[:, None]).astype(F32))] * sn[:, None].astype(F64)


# ---------------------------------------------------------------------------------------------------------------- the e4m3 model

def test_e4m3_model_against_the_library_and_torch():
    vals = FM.e4m3_values()
    fin = np.isfinite(vals)
    assert np.array_equal(fin, (np.arange(256) & 0x7f) != 0x7f)
    t = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(F8).double().numpy()
    assert np.array_equal(vals[fin], t[fin])
    codes = np.arange(256, dtype=np.uint8)[fin]
    assert np.array_equal(FM.e4m3_rne(vals[fin]), codes) and np.array_equal(_host_e4m3(vals[fin]), codes)          # all 254 finite codes, -0 among them
    pos = vals[:0x7f]
    mid = (pos[:-1] + pos[1:]) / 2                                                                                   # every tie: exact in float32
    want = np.where(np.arange(0x7e) % 2 == 0, np.arange(0x7e), np.arange(0x7e) + 1).astype(np.uint8)
    for sign in (1.0, -1.0):
        w = want | (0x80 if sign < 0 else 0)
        assert np.array_equal(FM.e4m3_rne(sign * mid), w) and np.array_equal(_host_e4m3(sign * mid), w)
        for d in (-1, 1):                                                                                            # one float32 ulp to either side decides
            x = np.nextafter((sign * mid).astype(F32), F32(d * np.inf))
            assert np.array_equal(FM.e4m3_rne(x), _host_e4m3(x))
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-14, 9, 200000))).astype(F32)
    x = x[np.abs(x) < 448]
    assert np.array_equal(FM.e4m3_rne(x), _host_e4m3(x))
    assert np.array_equal(FM.e4m3_rne(np.array([448.0, 460.0, 1e6, -1e6])), np.array([0x7e, 0x7e, 0x7e, 0xfe], np.uint8))
    # the truncating mutant differs on every tie with an odd lower neighbour and nowhere on the codes themselves
    assert np.array_equal(FM.e4m3_trunc(vals[fin]), codes)
    assert np.array_equal(FM.e4m3_trunc(mid) != FM.e4m3_rne(mid), np.arange(0x7e) % 2 == 1)
    assert np.array_equal(FM.rank(codes), np.where(codes & 0x80, -1, 1) * (codes & 0x7f).astype(np.int64))


def test_block_quantiser_against_the_ln_consumer_restatement():
    rng = np.random.default_rng(4)
    y = (rng.standard_normal((64, 256)) * np.exp2(rng.integers(-30, 20, (64, 8))).repeat(32, axis=1)).astype(F32)
    y[3, 32:64] = 0
    y[5, 7] = 2.0 ** -140                                                   # a float32 subnormal amax: byte 0
    y[5, :7] = 0
    y[5, 8:32] = 0
    E, codes = FM.quantise(y)
    E2, codes2, _ = LM.mx_quantise(y)
    assert np.array_equal(E, E2) and E[3, 1] == 0 and E[5, 0] == 0
    same = (codes == codes2) | (((codes | codes2) & 0x7f) == 0)             # torch gives +0 for a negative value that rounds to zero
    assert same.all()
    deq = FM.dequantise(E, codes)
    assert (np.abs(deq - y) <= np.abs(y) * 2.0 ** -4 + np.repeat(np.exp2(E - 127.0), 32, axis=1) * 2.0 ** -10).all()


# ---------------------------------------------------------------------------------------------------------------- A. the walk and the scale rule

@pytest.mark.parametrize('name', list(FC.HAND_OVER))
def test_tile_ownership(name):
    epi, M, N, bn, tiles, gm, _ = FC.HAND_OVER[name]
    assert tiles == (M // 256) * (N // bn) and tiles > 256
    w = FM.walk(M, N, 256, bn, gm)
    assert len(w) == 256
    seen = sorted(t for wg in w for t in wg)
    assert seen == sorted((a, b) for a in range(M // 256) for b in range(N // bn)), 'every tile once'
    # xcd_range: XCD x owns tiles / 8 contiguous tiles, its 32 workgroups walk them 32 apart
    per_xcd = tiles // 8
    assert tiles % 8 == 0
    n = FC.owners(name)
    for wg in range(256):
        assert n[wg] == len(range(wg >> 3, per_xcd, 32))
    want = {288: {1: 224, 2: 32}, 384: {1: 128, 2: 128}, 528: {2: 240, 3: 16}}[tiles]
    assert {int(k): int((n == k).sum()) for k in np.unique(n)} == want
    rows, pos = FC.sample_rows(name)
    assert len(rows) >= 64 and len(set(rows)) == len(rows) and set(pos) == set(range(max(want)))
    # the comparison launches: whole row tiles, at most 255 tiles, nobody has a second one, every row covered once
    ch = FC.chunks(name)
    assert ch[0][0] == 0 and ch[-1][1] == M and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
    for m0, m1 in ch:
        sub = FM.walk(m1 - m0, N, 256, bn, gm)
        assert m0 % 256 == 0 and 8 <= len(sub) <= 255 and all(len(t) == 1 for t in sub)


def test_small_launches_have_one_tile_per_workgroup():
    for tiles_m, tiles_n in ((2, 9), (8, 15), (63, 4), (85, 3), (1, 255)):
        w = FM.walk(tiles_m * 256, tiles_n * 256, 256, 256, 4)
        assert len(w) == tiles_m * tiles_n and all(len(t) == 1 for t in w)
        assert len({t[0] for t in w}) == len(w)


@pytest.mark.parametrize('name,K', FC.HAND_OVER_CASES)
def test_scale_rule_all_differ(name, K):
    """what a lane could fetch instead of its scale dword differs from it: along every workgroup's walk, K-tiles 0 and 1 of the next tile, K-tiles 0, 1 and
    the last two of this one; inside a tile every K-tile from the one and the two before it"""
    r, w, ncol = FC.rule(name, K)
    nk = K // 128
    assert ncol <= 3
    assert all(len({r[0, k], r[0, k - 1]}) == 2 for k in range(1, nk)) and all(r[0, k] != r[0, k - 2] for k in range(2, nk))
    pairs = 0
    for tiles in w:
        for (a, _), (b, _) in zip(tiles, tiles[1:]):
            six = [r[b, 0], r[b, 1], r[a, 0], r[a, 1], r[a, nk - 2], r[a, nk - 1]]
            assert len(set(six)) == 6, (name, a, b, six)
            pairs += 1
    assert pairs == int((FC.owners(name) - 1).sum())
    t = FC.term(256, K)
    assert t.min() == -3 and t.max() == 3
    for d in (16, 64, 128):                                                  # the other rows of a lane's dword, the other wave group, the other X half
        assert (t[:256 - d] != t[d:]).all()
    assert all((t[:, i] != t[:, j]).all() for i in range(4) for j in range(i))
    e = FC.block_exponent(name, K)
    assert e.min() >= -14 and e.max() <= 8                                   # A stays below 2^9, the products far inside fp16


@pytest.mark.parametrize('name,K', [('qkv', 512), ('residual 256x192 (LDS-staged)', 768)])
def test_hand_over_operands_and_scale_mutations(name, K):
    """The host quantiser gives every block of A the byte the rule promises, and a K-tile multiplied with the scale dwords of the K-tile before it, or a tile's
    K-tile 0 with those of the previous tile's K-tile 0, moves the fp64 reference by far more than the bound of the GPU test -- on every sampled row."""
    epi, M, N, bn, tiles, gm, _ = FC.HAND_OVER[name]
    c = FC.hand_over(name, K)
    rows, pos = FC.sample_rows(name)
    want = FC.expected_scale_bytes(name, K)
    some = np.unique(np.concatenate([rows, np.arange(0, M, 97)]))
    E, codes, _ = LM.mx_quantise(c['A'][some])
    assert np.array_equal(E, want[some])
    E, codes = E[np.searchsorted(some, rows)], codes[np.searchsorted(some, rows)]
    a_deq = FM.dequantise(E, codes)
    w_deq = _w_deq(c['W'])
    ref, mag = FM.product(a_deq, w_deq, c['bias'])
    tol = 2.0 ** -10 * np.abs(ref) + 1e-4 * mag + 1e-4 if epi == 0 else 2e-5 * np.maximum(1.0, np.abs(ref)) + 3e-4 * mag       # test_gpu_fp8.py's constants
    # the host model of the kernel itself -- float32 accumulation in any order -- is far inside
    f32 = (a_deq.astype(F32) @ w_deq.astype(F32).T + c['bias']).astype(F64)
    assert (np.abs(f32 - ref) <= 0.1 * tol).all()
    # (a) every K-tile on the dwords of the K-tile before it (K-tile 0 keeps its own)
    prev_kt = np.concatenate([E[:, :4], E[:, :-4]], axis=1)
    # (b) K-tile 0 of a workgroup's second / third tile on the dwords of the tile before it, same place inside the tile
    _, w, _ = FC.rule(name, K)
    before = {}
    for tl in w:
        for (a, _), (b, _) in zip(tl, tl[1:]):
            before[b] = a
    prev_tile = E.copy()
    later = pos > 0
    src = np.array([before[r // 256] * 256 + r % 256 for r in rows[later]])
    prev_tile[later, :4] = want[src, :4]
    for what, E_used, sel in (('previous K-tile', prev_kt, np.ones(len(rows), bool)), ("previous tile's K-tile 0", prev_tile, later)):
        mut, _ = FM.product(FM.rescale_blocks(a_deq, E, E_used), w_deq, c['bias'])
        ratio = (np.abs(mut - ref) / tol).max(1)[sel]
        assert sel.sum() >= 32 and ratio.min() > 10, f'{name} K={K}, {what}: the reference moves by only {ratio.min():.1f} bounds on some sampled row'


# ---------------------------------------------------------------------------------------------------------------- B. the fc1 epilogue

def test_fc1_exact_families_and_undecided_share():
    c = FC.fc1_exact()
    n_ties = FC.check_families(c)
    M, N = c['x'].shape
    # the operands are exactly representable: MXFP8 of A and the packer's e4m3 of W give A and W back
    E, codes = FM.quantise(c['A'])
    assert np.array_equal(FM.dequantise(E, codes).astype(F32).view(np.uint32), c['A'].view(np.uint32))
    assert np.array_equal(_w_deq(c['W']).astype(F32).view(np.uint32), c['W'].view(np.uint32))
    assert len(np.unique(c['x'], axis=0)) == M - len(FC.PURE_ROWS) + 1 and len(np.unique(c['bias'])) > 0.75 * N      # (the sweep repeats values, two blocks are zeros)
    lo, hi = FC.fc1_interval(c['x'])
    # the float32 emulation of the kernel's own arithmetic, quantised by the model: accepted everywhere
    v = MM.emu32(c['x'], 'bf16')
    E, codes = FM.quantise(v)
    r = FM.accept(lo, hi, E, codes)
    assert not r['bad_scale'].any() and not r['bad_code'].any()
    exempt = FC.exempt_blocks(c)
    open_ = (r['open_code'] | np.repeat(r['open_scale'], 32, axis=1)) & ~np.repeat(exempt, 32, axis=1)
    share = open_.mean()
    print(f'[fc1 exact] {n_ties} ties; undecided share outside the tie and power-of-two families {share:.2e}')
    assert share <= 0.01
    pure = np.repeat(c['pure'][:, None], N, axis=1)
    ties = pure & np.repeat(c['family'] == FC.FAMILIES.index('ties'), 32)[None, :]
    assert not r['open_code'][ties].any(), 'the ties are decided: the model knows their value exactly'
    # mutants
    _, trunc = FM.quantise(v, rne=FM.e4m3_trunc)
    bad = FM.accept(lo, hi, E, trunc)['bad_code']
    assert bad[ties].sum() >= n_ties // 2 - 2 and bad.mean() > 0.3, 'a truncating conversion must fail the tie family (every tie above an odd code) and half of all elements'
    sw = FM.accept(lo, hi, E, FM.swap_lane_pair(codes))['bad_code']
    assert sw.mean() > 0.5, 'a swapped lane pair must misplace most values'
    rows16 = codes.reshape(M // 64, 4, 16, N)[:, ::-1].reshape(M, N)        # a swapped jj: the four 16-row fragments of a wave's 64 rows in the other order
    assert FM.accept(lo, hi, E, rows16)['bad_code'].mean() > 0.3
    odd = np.roll(E, 1, axis=1)                                             # the scale dword written by the other lane pair's owner: the neighbouring block's bytes
    assert FM.accept(lo, hi, odd, codes)['bad_scale'].mean() > 0.5
    assert FM.accept(lo, hi, np.where(E > 0, E + 1, E), codes)['bad_scale'].mean() > 0.9


def test_fc1_gaussian_undecided_share():
    """B2 on the smallest of its shapes, operands quantised on the host: the share of elements whose code or scale byte the reference and the accumulation
    bound leave open stays below the cap of the GPU test; the float32 model of the kernel is accepted everywhere."""
    M, N, K = FC.GAUSS_SHAPES[0]
    A, W, bias = FC.fc1_gauss(M, N, K)
    E, codes, _ = LM.mx_quantise(A)
    a_deq, w_deq = FM.dequantise(E, codes), _w_deq(W)
    pre, mag = FM.product(a_deq, w_deq, bias)
    b = 1e-4 * mag + 2.0 ** -23 * np.abs(pre)
    lo, hi = FC.gauss_interval(pre, b)
    x32 = (a_deq.astype(F32) @ w_deq.astype(F32).T + bias).astype(F32)
    assert (np.abs(x32 - pre) <= 0.2 * b).all()
    Eo, co = FM.quantise(MM.emu32(x32, 'bf16'))
    r = FM.accept(lo, hi, Eo, co)
    assert not r['bad_scale'].any() and not r['bad_code'].any()
    share = (r['open_code'] | np.repeat(r['open_scale'], 32, axis=1)).mean()
    print(f'[fc1 gauss {M}x{N}x{K}] pre-activations {np.percentile(pre, [1, 50, 99]).round(2)}, sum|a||w| / |pre| median {np.median(mag / np.abs(pre)):.2f}; undecided share {share:.3e}')
    assert share <= 0.02
    assert (pre < -1).mean() > 0.3 and (pre > 1).mean() > 0.3
    assert FM.accept(lo, hi, Eo, FM.swap_lane_pair(co))['bad_code'].mean() > 0.3


# ---------------------------------------------------------------------------------------------------------------- C. the qkv epilogue

@pytest.mark.parametrize('mixed', [0, 1])
def test_qkv_exact_operands(mixed):
    c = FC.qkv_exact(mixed)
    E, codes = FM.quantise(c['A'])
    assert len(np.unique(E)) == (3 if mixed else 1)
    assert np.array_equal(FM.dequantise(E, codes).astype(F32), c['A'])
    assert np.array_equal(_w_deq(c['W']).astype(F32), c['W'])
    assert np.array_equal(c['ref'].astype(np.float16).astype(F32), c['ref'])
    buf = np.arange(128 * 192).reshape(128, 192)
    blocked = buf.reshape(2, 64, 3, 64).transpose(0, 2, 1, 3).reshape(-1)                                            # [M/64][N/64][64][64]
    assert np.array_equal(FM.deblock64(blocked, 128, 192), buf)
