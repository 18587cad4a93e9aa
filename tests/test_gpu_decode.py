"""GPU: the six instantiations of csrc/decode.hip decode_kernel against the float64 model of tests/decode_model.py, per joint, on the case families of
tests/decode_cases.py (ties through every stage of the arg-max reduction, the extremes of the index range, corners and edges, non-positive maps and the
wrap of their samples, the clip bounds, peaked maps, the record route's crops).

The model decides each joint's class and bound; the device never does.  plateau: the coordinates are the arg-max mapped to the frame on every bit;
conditioned: within the derived bound; ill-conditioned: the arg-max only (a bit-equal confidence).  Confidences are bit equal everywhere.  The flip-test,
record and flip-test-record instantiations are held to the plain kernel's bits on batches whose average / whose crops are exactly the case."""
import numpy as np
import pytest

import decode_cases as DC
import decode_model as M
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd import decode_heatmaps
from easy_vitpose_amd.engine import decode_affine_heatmaps, decode_flip_heatmaps

pytestmark = pytest.mark.gpu

NAMES = list(DC.FAMILIES)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
twice = lambda n: np.tile(np.array([[94, 126]], np.int32), (n, 1))   # org_wh = (94, 126): the kernel writes exactly 2 x the heatmap position


@pytest.fixture(scope='module')
def quantised_models():
    """the model of every family's batches on the 2^-12 grid of the flip-test cases, computed once"""
    cache = {}

    def get(name, b):
        if (name, b) not in cache:
            q = DC.quantised(DC.family(name)[b])
            cache[name, b] = (q, M.decode_batch(q))
        return cache[name, b]
    return get


# ------------------------------------------------------------------------------------------------------------------ plain
@pytest.mark.parametrize('name', NAMES)
def test_plain_against_the_model(name):
    worst = {}
    for b, (hm, m) in enumerate(zip(DC.family(name), DC.models(name))):
        for tag, wh in (('(94, 126)', twice(len(hm))), ('odd sizes', DC.sizes(len(hm), b))):
            got = decode_heatmaps(np.array(hm), wh)
            w, fails = M.check(m, got, 'pad', wh)
            worst[tag] = max(worst.get(tag, 0.0), w)
            assert not fails, (name, b, tag, fails[:5])
    print(f'device, plain, {name}: worst err / bound ' + ', '.join(f'{t} {w:.3f}' for t, w in worst.items()))


@pytest.mark.parametrize('name', ['ties', 'nonpos'])
def test_batch_position(name):
    """a crop decodes to the same bits as crop 0, as crop 1 and as the last crop of a batch of 3, between crops that are bright where its samples would land
    if the wrap left the crop"""
    rng = np.random.default_rng(41)
    for b, hm in enumerate(DC.family(name)):
        K = hm.shape[1]
        other = lambda: np.stack([DC.bright_row(rng, int(rng.integers(5, 43)), int(rng.integers(5, 55))) for _ in range(K)])
        for i, case in enumerate(hm):
            alone = decode_heatmaps(case[None], DC.sizes(1, i))
            for pos in range(3):
                batch = np.stack([other(), other(), other()])
                batch[pos] = case
                wh = np.concatenate([DC.sizes(3, 9)[:pos], DC.sizes(1, i), DC.sizes(3, 9)[pos + 1:]])
                assert np.array_equal(bits(decode_heatmaps(batch, wh)[pos]), bits(alone[0])), (name, b, i, pos)


# ------------------------------------------------------------------------------------------------------------------ flip-test
@pytest.mark.parametrize('shift', [False, True])
@pytest.mark.parametrize('name', NAMES)
def test_flip_equals_plain_on_an_exact_average(name, shift):
    for b, hm in enumerate(DC.family(name)):
        q = DC.quantised(hm)
        pairs = DC.flip_pairs(q.shape[1])
        wh = DC.sizes(len(q), b)
        got = decode_flip_heatmaps(DC.flip_batch(q, pairs, shift, b), pairs, shift, wh)
        assert np.array_equal(bits(got), bits(decode_heatmaps(q, wh))), (name, b)


# ------------------------------------------------------------------------------------------------------------------ the record route
def test_record_route():
    """crops with K_e = 1, 2, 17 in one launch between bright neighbours: row dst_j is vp_decode_only of those K_e maps alone on every bit (and within the model's
    rules), joints beyond K_e are +0"""
    lib = capi.load_library()
    maps, rec = DC.record()
    n, kmax = len(rec), DC.RECORD_KMAX
    wh = DC.sizes(n, 3)
    out = np.full((n, kmax, 3), np.nan, np.float32)
    capi.check(lib.vp_dbg_decode_mix(0, maps.ctypes.data, len(maps), n, kmax, rec.ctypes.data, wh.ctypes.data, out.ctypes.data))
    for j, ((first, K, dst), m) in enumerate(zip(rec, DC.models('record'))):
        want = decode_heatmaps(maps[first:first + K][None], wh[dst][None])[0]
        assert np.array_equal(bits(out[dst, :K]), bits(want)), f'crop {j} (K {K})'
        assert not bits(out[dst, K:]).any(), f'crop {j}: joints beyond K'
        w, fails = M.check(m, out[dst:dst + 1, :K], 'pad', wh[dst][None])
        assert not fails, fails[:5]


@pytest.mark.parametrize('shift', [False, True])
def test_flip_record_route(shift):
    """the same crops under the per-expert flip-test mode: each crop's [2, K_e] pair averages to the quantised crop exactly; one partner row per K_e"""
    lib = capi.load_library()
    maps, rec = DC.record()
    n, kmax = len(rec), DC.RECORD_KMAX
    experts = {17: 0, 1: 1, 2: 2}
    tab = np.tile(np.arange(kmax, dtype=np.int32), (3, 1))
    for K, e in experts.items():
        for a, b in DC.flip_pairs(K):
            tab[e, a], tab[e, b] = b, a
    parts, rec4, first = [], [], 0
    for j, (f, K, dst) in enumerate(rec):
        q = DC.quantised(maps[f:f + K][None])
        parts.append((q, DC.flip_batch(q, DC.flip_pairs(int(K)), shift, j).reshape(2 * K, M.H, M.W)))
        rec4.append((first, K, dst, experts[int(K)]))
        first += 2 * K
    hm2 = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
    rec4 = np.ascontiguousarray(rec4, np.int32)
    wh = DC.sizes(n, 4)
    out = np.full((n, kmax, 3), np.nan, np.float32)
    capi.check(lib.vp_dbg_decode_flip_mix(0, hm2.ctypes.data, len(hm2), n, kmax, rec4.ctypes.data, tab.ctypes.data, 3, int(shift), wh.ctypes.data, out.ctypes.data))
    for j, ((q, _), (_, K, dst, _)) in enumerate(zip(parts, rec4)):
        assert np.array_equal(bits(out[dst, :K]), bits(decode_heatmaps(q, wh[dst][None])[0])), f'crop {j} (K {K})'
        assert not bits(out[dst, K:]).any(), f'crop {j}: joints beyond K'


# ------------------------------------------------------------------------------------------------------------------ affine
@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('name', NAMES)
def test_affine_against_the_model(name, flip, quantised_models):
    """the affine instantiations through the model's affine mapping, S_w from 20 to 2000, and a refused row (S_w = 0) that is all zero; with flip_pairs: the
    interleaved batch whose average is the quantised case, against the model of that case (shift 0 and 1)"""
    worst = 0.0
    for b, hm in enumerate(DC.family(name)):
        hm, m = quantised_models(name, b) if flip else (np.array(hm), DC.models(name)[b])
        n, K = hm.shape[:2]
        cs = np.concatenate([DC.affine_cs(n, b), np.array([[10.0, 20.0, 0.0, 0.0]], np.float32)])
        hm1 = np.concatenate([hm, hm[:1]])                                    # the refused row decodes a real crop
        if flip:
            pairs = DC.flip_pairs(K)
            outs = [decode_affine_heatmaps(DC.flip_batch(hm1, pairs, s, b), cs, flip_pairs=pairs, shift_heatmap=bool(s)) for s in (0, 1)]
            assert np.array_equal(bits(outs[0]), bits(outs[1])) and np.array_equal(bits(outs[0]), bits(decode_affine_heatmaps(hm1, cs)))
            got = outs[0]
        else:
            got = decode_affine_heatmaps(hm1, cs)
        assert not bits(got[n]).any(), 'the refused row'
        w, fails = M.check(m, got[:n], 'affine', cs[:n])
        worst = max(worst, w)
        assert not fails, (name, b, fails[:5])
    print(f"device, affine{' flip' if flip else ''}, {name}: worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ NaN isolation
def test_nan_crop_does_not_reach_its_neighbours():
    """what a joint with NaN in its own or its wrapped-into map returns is outside the contract; every other crop's rows are bit-identical to the
    run without the NaN crop"""
    dirty, clean = DC.nan_crops()
    wh = DC.sizes(3, 5)
    a, b = decode_heatmaps(dirty, wh), decode_heatmaps(clean, wh)
    assert np.array_equal(bits(a[[0, 2]]), bits(b[[0, 2]]))
    assert np.array_equal(bits(a[1, 1:3]), bits(b[1, 1:3]))                   # the NaN crop's own clean maps 1 and 2 wrap nowhere: theirs too
    m = M.decode_batch(clean)
    w, fails = M.check(m, b, 'pad', wh)
    assert not fails, fails[:5]
    pairs = DC.flip_pairs(4)
    q = DC.quantised(clean)
    qd = np.where(np.isnan(dirty), dirty, q)
    fa = decode_flip_heatmaps(DC.flip_batch(qd, pairs, False), pairs, False, wh)
    fb = decode_flip_heatmaps(DC.flip_batch(q, pairs, False), pairs, False, wh)
    assert np.array_equal(bits(fa[[0, 2]]), bits(fb[[0, 2]]))
