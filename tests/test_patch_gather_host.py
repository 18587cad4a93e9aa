"""CPU: the host model of the patch gather (tests/patch_gather_model.py) pinned before any GPU time is spent.

(1) The model is the module's semantics: decode(gather(x16)) @ W.reshape(D, 768).T in float64 equals F.conv2d(x16, W, stride = 16, padding = 2) in float64 within
    float64 round-off -- mode 0, mode 1 (the conv of the mirrored crop), and the twin against both.
(2) normalise_u8 equals oracle.vitpose_cpu.pre_img bit for bit on all 256 x 3 values.
(3) The cases (tests/patch_gather_cases.py) can see the mistakes a gather kernel could make: each wrong variant differs from the model on them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import patch_gather_cases as PC
import patch_gather_model as PM
import residual_row_model as RM

F32, F64 = np.float32, np.float64


def _conv(x16, Wt):
    """fp64 conv of the decoded crops [n, 3, 256, 192] -> [n * 192, D]"""
    y = F.conv2d(torch.from_numpy(x16), torch.from_numpy(Wt), stride=16, padding=2).numpy()          # [n, D, 16, 12]
    return y.transpose(0, 2, 3, 1).reshape(-1, Wt.shape[0])


@pytest.mark.parametrize('dtype', PC.DTYPES)
@pytest.mark.parametrize('D', (8, 24))
def test_model_is_the_convolution(dtype, D):
    rng = np.random.default_rng(D)
    x = np.concatenate([PC.f32_cases(dtype)['gauss'][:2], PC.f32_cases(dtype)['position'][1:2]])
    bits = PM.to16(x, dtype)
    x16 = PM.decode(bits, dtype)
    Wt = rng.standard_normal((D, 3, 16, 16))
    Wt[:, :, :, 0] += 1.0                                 # asymmetric in kx, ky and c: a transposed or mirrored patch cannot cancel
    Wt[:, 1] *= 1.5
    Wt[:, :, 3] -= 0.5
    Wm = Wt.reshape(D, 768).T
    mag = np.abs(_conv(np.abs(x16), np.abs(Wt))).max()
    tol = 768 * 2.0 ** -52 * mag                          # 768 products summed in float64, in whatever order
    straight, mirrored = _conv(x16, Wt), _conv(np.ascontiguousarray(x16[..., ::-1]), Wt)
    for mode, ref in ((0, straight), (1, mirrored)):
        for B, n_src in ((3, 3), (4, 2)):
            got = PM.decode(PM.gather(bits, B, n_src, mode), dtype) @ Wm
            src = [min(b, n_src - 1) for b in range(B)]
            want = ref.reshape(3, 192, D)[src].reshape(B * 192, D)
            assert np.abs(got - want).max() <= tol, (mode, B, n_src, np.abs(got - want).max(), tol)
    for B, n_src in ((2, 1), (5, 2), (6, 2), (6, 3)):
        got = (PM.decode(PM.gather(bits, B, n_src, 2), dtype) @ Wm).reshape(B, 192, D)
        for b in range(B):
            r = min(b, 2 * n_src - 1)
            want = (mirrored if r & 1 else straight).reshape(3, 192, D)[r >> 1]
            assert np.abs(got[b] - want).max() <= tol, (B, n_src, b)
    assert np.abs(straight - mirrored).max() > 1e3 * tol  # the two references are told apart


def test_normalise_u8_is_pre_img():
    from oracle import vitpose_cpu as O
    img = np.zeros((256, 192, 3), np.uint8)
    img.reshape(-1, 3)[:256] = np.arange(256, dtype=np.uint8)[:, None]
    ref = O.pre_img(img)[0][0]                            # [3, 256, 192]
    got = PM.nchw(PM.normalise_u8(img)[None])[0]
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert len(np.unique(got.reshape(3, -1)[:, :256], axis=1).T) == 256


def test_u8_cases_hit_every_phase():
    cov = PC.phase_coverage(PC.u8_cases()['allbytes'][0])
    assert cov.all()                                      # every byte value at every (position in a 16-byte piece, channel)
    c = PC.u8_cases()['const']
    assert (c[0] == 0).all() and (c[1] == 255).all()


def test_f32_cases_cover_what_they_name():
    for dtype in PC.DTYPES:
        pos = PM.to16(PC.f32_cases(dtype)['position'][0], dtype)
        for c in range(3):
            assert len(np.unique(pos[c])) == 256 * 192    # every (y, x) its own code
        assert (pos[0] != pos[1]).all() and (pos[1] != pos[2]).all()
        e = PC.f32_cases(dtype)['edges']
        ev = PC.edge_values(dtype)
        for y, x in ((0, 0), (0, 191), (255, 0), (255, 191), (13, 14), (14, 13), (100, 189), (100, 190)):
            assert e[0, 0, y, x] in ev, (y, x)
        for k in range(3):
            assert set(np.unique(e[k].view(np.uint32))) >= set(ev.view(np.uint32))      # every edge value in every crop (the signed zeros by their bits)


# ---- the wrong variants -----------------------------------------------------------------------------------------------------------------------------------------

def _patches_order(order):
    def f(img):
        pad = np.zeros((3, 256 + 18, 192 + 18), np.uint16)
        pad[:, 2:258, 2:194] = img
        win = pad[:, :256, :192].reshape(3, 16, 16, 12, 16)                   # (c, py, ky, px, kx)
        return np.ascontiguousarray(win.transpose(*order)).reshape(192, 768)
    return f


def _wrong_side(img):
    """the mirrored crop with the zero border left where the STRAIGHT crop has it: the mirror's own left border reads past the row's end (here: the last pixel again)"""
    m = img[..., ::-1]
    pad = np.zeros((3, 258, 194), np.uint16)
    pad[:, 2:, 2:] = m
    pad[:, 2:, :2] = m[..., :1]
    win = pad[:, :256, :192].reshape(3, 16, 16, 12, 16)
    return np.ascontiguousarray(win.transpose(1, 3, 0, 2, 4)).reshape(192, 768)


def _patch_mirror(img):
    """mirror of every patch instead of the image: the patch grid of the straight crop, kx reversed"""
    return PM.patches(img).reshape(192, 3, 16, 16)[..., ::-1].reshape(192, 768)


WRONG_GATHER = {
    'border 0': dict(patches=lambda img: PM.patches(img, border=0)),
    'border 4': dict(patches=lambda img: PM.patches(img, border=4)),
    'kx / ky swapped': dict(patches=_patches_order((1, 3, 0, 4, 2))),
    'channel-minor columns': dict(patches=_patches_order((1, 3, 2, 4, 0))),
    'padding rows repeat crop 0': dict(source=lambda b, n, mode: ((b if b < n else 0), mode == 1) if mode != 2 else ((b >> 1, bool(b & 1)) if b < 2 * n else (0, False))),
    'twin parity swapped': dict(source=lambda b, n, mode: (PM.source(b, n, mode)[0], not PM.source(b, n, mode)[1]) if mode == 2 else PM.source(b, n, mode)),
}
WRONG_MIRROR = {'mirror of the patch': _patch_mirror, 'mirror: zero border on the wrong side': _wrong_side}
MIRROR_ONLY = ('twin parity swapped',) + tuple(WRONG_MIRROR)
PADDING_ONLY = ('padding rows repeat crop 0',)


def _gather_mirrored_by(fn, bits, B, n_src, mode):
    """gather whose mirrored output crops are fn(the straight crop)"""
    out = np.empty((B, 192, 768), np.uint16)
    for b in range(B):
        s, m = PM.source(b, n_src, mode)
        out[b] = fn(bits[s]) if m else PM.patches(bits[s])
    return out.reshape(B * 192, 768)


@pytest.mark.parametrize('dtype', PC.DTYPES)
def test_wrong_gathers_differ_on_the_cases(dtype):
    shapes = {0: ((1, 1), (3, 3), (4, 2)), 1: ((1, 1), (3, 3), (4, 2)), 2: ((2, 1), (5, 2), (6, 2))}
    seen = {}
    for case in ('position', 'edges'):
        bits = PM.to16(PC.f32_cases(dtype)[case], dtype)
        for mode, sh in shapes.items():
            for B, n_src in sh:
                ref = PM.gather(bits, B, n_src, mode)
                for name, kw in WRONG_GATHER.items():
                    d = bool((PM.gather(bits, B, n_src, mode, **kw) != ref).any())
                    seen.setdefault((name, case), {})[mode, B, n_src] = d
                for name, fn in WRONG_MIRROR.items():
                    seen.setdefault((name, case), {})[mode, B, n_src] = bool((_gather_mirrored_by(fn, bits, B, n_src, mode) != ref).any())
    for (name, case), hits in seen.items():
        for (mode, B, n_src), d in hits.items():
            padded = B > (2 * n_src if mode == 2 else n_src)
            applies = (mode != 0 if name in MIRROR_ONLY else True) and (padded if name in PADDING_ONLY else True)
            if name == 'twin parity swapped':
                applies = mode == 2
            assert d == applies, f'{name} on {case} (mode {mode}, B {B}, n_src {n_src}): differs = {d}'
    # the border variants on the position crop alone: one crop is enough
    one = PM.to16(PC.f32_cases(dtype)['position'][:1], dtype)
    for name in ('border 0', 'border 4'):
        assert (PM.gather(one, 1, 1, 1, **WRONG_GATHER[name]) != PM.gather(one, 1, 1, 1)).any(), name
    assert (_gather_mirrored_by(_wrong_side, one, 1, 1, 1) != PM.gather(one, 1, 1, 1)).any()


def _to16_truncate(x, dtype):
    """round toward zero instead of to nearest even (the fp16 clamp kept)"""
    bits = PM.to16(x, dtype)
    xc = np.clip(x, -PM.F16_MAX, PM.F16_MAX) if dtype == 'fp16' else x
    over = np.abs(RM.from_bits(bits, dtype).astype(F64)) > np.abs(np.asarray(xc, F64))
    return (bits - over.astype(np.uint16)).astype(np.uint16)          # sign-magnitude codes: one code towards zero


@pytest.mark.parametrize('dtype', PC.DTYPES)
def test_wrong_conversions_differ_on_the_cases(dtype):
    x = PC.f32_cases(dtype)['edges']
    ref = PM.to16(x, dtype)
    mask = PC.border_mask()
    trunc = _to16_truncate(x, dtype)
    assert (trunc[..., mask] != ref[..., mask]).any() and (np.abs(RM.from_bits(trunc, dtype)) <= np.abs(RM.from_bits(ref, dtype))).all()
    # ... and on the ties themselves: 1 + 3 * 2^-11 (fp16) / 1 + 3 * 2^-8 (bf16) round UP to even
    t = F32(1.0 + 3.0 * (2.0 ** -11 if dtype == 'fp16' else 2.0 ** -8))
    assert (x == t).any() and (trunc[x == t] != ref[x == t]).all()
    if dtype == 'fp16':
        noclamp = RM.to_bits(x, dtype)
        assert (noclamp != ref).any() and not np.isfinite(RM.from_bits(noclamp, dtype)).all() and np.isfinite(RM.from_bits(ref, dtype)).all()
    else:
        assert np.array_equal(RM.to_bits(x, dtype), ref)                # bf16 does not clamp
    # normalised uint8 values never sit on a tie, but truncation still shows on them
    u = PM.normalise_u8(PC.u8_cases()['allbytes'][:1])
    assert (_to16_truncate(u, dtype) != PM.to16(u, dtype)).any()


def test_symbols_exported():
    from easy_vitpose_amd import _capi as capi
    lib = capi.load_library()
    for name in ('vp_dbg_im2col', 'vp_dbg_layernorm_planes'):
        assert name in capi.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
