"""CPU: the float64 decode model of tests/decode_model.py and the case families of tests/decode_cases.py.

The families fall into the classes the case table states; the float32 oracle and the committed reference outputs lie within the model's class rules (so the
bound is one the reference itself meets); ten wrong models each fail the rules on the family named for them while the correct model passes; the flip-test
batches of the device test average to their case on every bit."""
import os

import numpy as np
import pytest

import decode_cases as DC
import decode_model as M
from cases import org_sizes, peaked_heatmaps
from oracle import vitpose_cpu as O

NAMES = list(DC.FAMILIES)


def test_weights_are_the_oracles():
    assert np.array_equal(M.gauss11().view(np.uint32), O.gaussian_kernel_1d(11).view(np.uint32))


def test_families_fall_into_the_stated_classes():
    """conditions, not measurements: every joint in its stated class, ill-conditioned joints only where allowed and at most 5 % of all"""
    total = ill = 0
    for name in NAMES:
        for b, m in enumerate(DC.models(name)):
            cls = m['cls']
            assert not (cls == M.NAN).any()
            total, ill = total + cls.size, ill + int((cls == M.ILL).sum())
            if name not in DC.MAY_BE_ILL:
                assert not (cls == M.ILL).any(), (name, b, np.argwhere(cls == M.ILL))
            if name in DC.EXPECTED:
                want = DC.EXPECTED[name][b]
                for i in range(len(cls)):
                    w = want[i if len(want) > 1 else 0]
                    assert cls[i].tolist() == (w if isinstance(w, list) else [w] * cls.shape[1]), (name, b, i, cls[i])
            cond = cls == M.CONDITIONED
            assert (m['rho'][cond] < M.RHO_MAX).all() and (np.maximum(m['bx'], m['by'])[cond] <= M.BOUND_MAX).all()
    print(f'ill-conditioned: {ill} of {total} joints')
    assert ill <= DC.ILL_SHARE_MAX * total
    assert (DC.models('nonpos')[2]['cls'][6, 0] == M.ILL) and not DC.models('nonpos')[2]['near'][6, 0]   # the known ill-conditioned case; maxval <= 0: no 1.5 px check


def test_tie_pairs_cover_the_reduction():
    """the pairs are what the case table says, in the kernel's thread layout: thread = (index % 1024) / 4, lane = thread % 64, wave = thread / 64"""
    th = lambda i: (i % 1024) // 4
    same_wave, waves = set(), set()
    for lo, hi, what in DC.TIE_PAIRS:
        a, b = th(lo), th(hi)
        if a // 64 == b // 64 and a != b:
            same_wave.add((a % 64) ^ (b % 64))
        elif a != b:
            waves.add((a // 64, b // 64))
    assert same_wave == {1, 2, 4, 8, 16, 32}
    assert waves >= {(x, y) for x in range(4) for y in range(4) if x != y}
    assert any(lo // 4 == hi // 4 for lo, hi, _ in DC.TIE_PAIRS) and any(hi - lo == 1024 for lo, hi, _ in DC.TIE_PAIRS) and any(hi - lo == 2048 for lo, hi, _ in DC.TIE_PAIRS)
    assert (1020, 1024) in {p[:2] for p in DC.TIE_PAIRS} and (2044, 2048) in {p[:2] for p in DC.TIE_PAIRS}
    m, hm = DC.models('ties')[0], DC.family('ties')[0]
    for k, (lo, hi, what) in enumerate(DC.TIE_PAIRS):
        flat = hm[0, k].reshape(-1)
        assert np.flatnonzero(flat == flat.max()).tolist() == [lo, hi] and m['idx'][0, k] == lo, what
    assert DC.models('extremes')[0]['idx'][0].tolist() == list(DC.EXTREME_INDICES)
    assert [(int(x), int(y)) for x, y in zip(DC.models('corners')[0]['cx'][0], DC.models('corners')[0]['cy'][0])] == DC.CORNER_XY


def test_clip_spikes_straddle_the_bounds():
    """the floor spikes: the centre sample above 0.001 and the four axis neighbours below it in the model's own blur; the ceiling spikes likewise around 50"""
    hm = DC.family('clip')[0][0]
    w = M.gauss11().astype(np.float64)
    for k, bound in ((0, M.CLIP_LO), (1, M.CLIP_LO), (2, M.CLIP_LO), (3, M.CLIP_HI), (4, M.CLIP_HI)):
        y, x = divmod(int(hm[k].argmax()), M.W)
        a = lambda yy, xx: w @ hm[k][np.ix_(M.reflect101(yy + np.arange(-5, 6), M.H), M.reflect101(xx + np.arange(-5, 6), M.W))].astype(np.float64) @ w
        assert a(y, x) > bound * 1.01, k
        below = [a(y, x + 1) < bound * 0.99, a(y, x - 1) < bound * 0.99, a(y + 1, x) < bound * 0.99, a(y - 1, x) < bound * 0.99]
        assert all(below), (k, below)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_within_the_class_rules(name):
    """O.decode_per_crop, whose blur, log and differences are float32 like the kernel's, through both pad mappings"""
    for b, (hm, m) in enumerate(zip(DC.family(name), DC.models(name))):
        for tag, wh in (('(94, 126)', np.tile(np.array([[94, 126]], np.int32), (len(hm), 1))), ('odd sizes', DC.sizes(len(hm), b))):
            worst, fails = M.check(m, O.decode_per_crop(np.array(hm), wh), 'pad', wh, f32_steps=True)
            print(f'oracle, {name} batch {b} {tag}: worst err / bound {worst:.3f}')
            assert not fails, fails[:5]


@pytest.mark.parametrize('tag', ['decode_k17', 'decode_k133'])
def test_reference_goldens_within_the_class_rules(golden_dir, tag):
    z = np.load(os.path.join(golden_dir, f'{tag}.npz'))
    n, k, seed = int(z['n']), int(z['k']), int(z['seed'])
    hm, wh = peaked_heatmaps(n, k, seed), org_sizes(n, seed)
    m = M.decode_batch(hm)
    worst, fails = M.check(m, z['expected'], 'pad', wh, f32_steps=True)
    cnt = np.bincount(m['cls'].ravel(), minlength=4)
    print(f'reference golden {tag}: worst err / bound {worst:.3f}; classes plateau / conditioned / ill {cnt[:3].tolist()}')
    assert not fails, fails[:5]
    assert cnt[M.CONDITIONED] >= 0.95 * m['cls'].size


def hm_fails(name, wrong):
    """failures of a (wrong) model's own output, as a device's, against the correct model's class rules, in heatmap pixels"""
    out = []
    for hm, m in zip(DC.family(name), DC.models(name)):
        out += M.check(m, M.as_output(M.decode_batch(hm, wrong=wrong)), 'hm')[1]
    return out


def record_fails(wrong):
    """the record route on the CPU: every crop's K_e maps decoded inside the launch's map array (what follows them is the next crop's maps)"""
    maps, rec = DC.record()
    out = []
    for (first, K, _), m in zip(rec, DC.models('record')):
        got = M.decode_crop(maps[first:first + DC.RECORD_KMAX], K=int(K), wrong=wrong)
        out += M.check(m, M.as_output({k: v[None] for k, v in got.items()}), 'hm')[1]
    return out


# wrong model -> the family that must catch it
CAUGHT_BY = {'reflect': 'corners', 'last_tie': 'ties', 'ge_zero': 'nonpos', 'wrap_own_map': 'nonpos', 'zero_pad': 'corners', 'floor_1e-4': 'clip',
             'dy_sign': 'corners', 'stride': 'ties', 'eps0': 'clip', 'wrap_kmax': 'record'}


def test_correct_model_passes_its_own_rules():
    for name in NAMES:
        assert not hm_fails(name, None), name
    assert not record_fails(None)


@pytest.mark.parametrize('wrong', M.WRONG)
def test_wrong_model_is_caught(wrong):
    assert set(CAUGHT_BY) == set(M.WRONG)
    fails = record_fails(wrong) if wrong == 'wrap_kmax' else hm_fails(CAUGHT_BY[wrong], wrong)
    print(f'{wrong}: {len(fails)} joints of {CAUGHT_BY[wrong]} fail, e.g. {fails[:1]}')
    assert fails
    if wrong == 'floor_1e-4':   # what no family caught before the clip family: the spikes themselves, not its plateaus
        assert any('joint 0 ' in f or 'joint 1 ' in f or 'joint 2 ' in f for f in fails)
    if wrong == 'last_tie':     # every tied pair, the crossing ones included
        assert len(fails) == len(DC.TIE_PAIRS)


@pytest.mark.parametrize('shift', [False, True])
def test_flip_batches_average_to_their_case_on_every_bit(shift):
    for name in NAMES:
        for b, hm in enumerate(DC.family(name)):
            q = DC.quantised(hm)
            pairs = DC.flip_pairs(q.shape[1])
            hm2 = DC.flip_batch(q, pairs, shift, b)
            assert np.array_equal(DC.merged_on_host(hm2, pairs, shift).view(np.uint32), q.view(np.uint32)), (name, b)
            assert not np.array_equal(hm2[0::2], q)                                       # and the crop alone is not the case
            d = (hm2[0::2] != q).reshape(-1, M.W) if np.isfinite(q).all() else None
            assert d is None or (d[:, 0].any() and d[:, 47].any())                        # perturbed in columns 0 and 47


def test_frame_mappings():
    m = DC.models('corners')[0]
    m = dict(m, rx=m['rx'].astype(np.float32).astype(np.float64), ry=m['ry'].astype(np.float32).astype(np.float64))   # positions the kernel can store
    wh = np.array([[94, 126]])
    f, b = M.pad_frame(m, wh)
    assert np.array_equal(f[..., 1], 2 * m['rx']) and np.array_equal(f[..., 0], 2 * m['ry'])
    assert (b[..., 1] >= 2 * m['bx']).all() and (b[..., 1] <= (2 * m['bx'] + 2.0 ** -24 * np.abs(f[..., 1])) * (1 + 2.0 ** -19) + 1e-12).all()
    cs = np.array([[47.0, 63.0, 94.0, 126.0]], np.float32)                               # the affine route on the same box: the same numbers
    fa, ba = M.affine_frame(m, cs)
    assert np.array_equal(fa, f) and np.array_equal(ba, b)
    for c, o, span in ((-1, 333, 47), (17, 899, 47), (63, 1199, 63), (0, 31, 47)):
        bits = M.pad_plateau_bits(c, o, span)
        exact = c * o / span + o // 2 - o / 2
        assert 1 <= len(bits) <= 2 and all(abs(float(np.array(v, np.uint32).view(np.float32)) - exact) <= 2.0 ** -24 * abs(exact) + 1e-12 for v in bits)


def test_near_rule_of_the_ill_conditioned_class():
    """no joint of the families sets `near` (their one ill-conditioned joint has maxval <= 0), so the rule itself is exercised here on a hand-made model row:
    an ill-conditioned joint with a valid bound is held to 1.5 heatmap pixels around its arg-max, in frame pixels of its own crop"""
    one = lambda v, dt=np.float64: np.array([[v]], dtype=dt)
    m = dict(cls=one(M.ILL, np.int64), near=one(True, bool), conf=one(0.5, np.float32), cx=one(10.0), cy=one(20.0), rx=one(10.4), ry=one(19.0), bx=one(0.3), by=one(0.3))
    wh = np.array([[470, 630]])                                                    # 10 frame pixels per heatmap pixel
    got = lambda y, x, c=0.5: np.array([[[y, x, c]]], np.float32)
    assert not M.check(m, got(200.0 + 14.0, 100.0 - 14.0), 'pad', wh)[1]
    assert M.check(m, got(200.0 + 16.0, 100.0), 'pad', wh)[1] and M.check(m, got(200.0, 100.0 - 16.0), 'pad', wh)[1]
    assert M.check(m, got(200.0, 100.0, 0.25), 'pad', wh)[1]                       # and the arg-max through the confidence
    m['near'] = one(False, bool)
    assert not M.check(m, got(900.0, -300.0), 'pad', wh)[1]
