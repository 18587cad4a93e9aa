"""CPU: the float64 model of the simple decoder's head (tests/simple_head_model.py) against torch's float64 F.interpolate + F.conv2d, a float32 emulation of the
device's order inside the bound, every wrong model failing it on the case families (tests/simple_head_cases.py), the weight image through
vp_dbg_simple_head_pack (no device), infer_head_from_state_dict and the synthetic simple-decoder checkpoints."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import simple_head_cases as SC
import simple_head_model as SM
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import infer_head_from_state_dict, model_shape
from easy_vitpose_amd.synth import synthetic_state_dict

F32, F64 = np.float32, np.float64
SHAPES = [('fp16', 64, 17), ('bf16', 64, 5), ('fp16', 384, 17)]
FAMILIES = {'taps': SC.taps, 'edges': SC.edges, 'corners': lambda *a: SC.edges(*a, variant='corners'), 'relu': SC.relu,
            'relu_sub': lambda *a: SC.relu(*a, variant='sub'), 'lo_plane': SC.lo_plane, 'seams': SC.seams, 'random': SC.random}


def _torch_module(x, W, b):
    """F.interpolate(F.relu(x), scale_factor=4, mode='bilinear', align_corners=False) + F.conv2d(padding=1) in float64 on NCHW"""
    t = torch.from_numpy(np.asarray(x, F64).reshape(-1, 16, 12, x.shape[-1]).transpose(0, 3, 1, 2).copy())
    up = F.interpolate(F.relu(t), scale_factor=4, mode='bilinear', align_corners=False)
    return F.conv2d(up, torch.from_numpy(np.asarray(W, F64)), torch.from_numpy(np.asarray(b, F64)), padding=1).numpy()


@pytest.mark.parametrize('family', tuple(FAMILIES))
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_model_is_the_torch_module(family, shape):
    dtype, D, K = shape
    case = FAMILIES[family](dtype, D, K)
    hi, lo = SM.split(case['w'], dtype)
    v, S = SM.model(case['x'], case['w'], case['b'], dtype)
    ref = _torch_module(case['x'], hi.astype(F64) + lo.astype(F64), case['b'])
    assert v.shape == ref.shape == (case['x'].shape[0], K, 64, 48)
    assert np.abs(v - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), np.abs(v - ref).max()
    assert (S >= np.abs(v) * (1 - 1e-12)).all()


def test_sampling_rule_is_interpolate():
    for n in (16, 12):
        eye = torch.eye(n, dtype=torch.float64)[None, None]
        ref = F.interpolate(eye, scale_factor=(4, 1), mode='bilinear', align_corners=False)[0, 0].numpy()
        assert np.abs(SM.upsample_matrix(n) - ref).max() <= 1e-15
        assert set(np.unique(SM.upsample_matrix(n))) <= {0.0, 0.125, 0.375, 0.625, 0.875, 1.0}


@pytest.mark.parametrize('family', tuple(FAMILIES))
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_float32_emulation_stays_inside_the_bound(family, shape):
    dtype, D, K = shape
    case = FAMILIES[family](dtype, D, K)
    v, S = SM.model(case['x'], case['w'], case['b'], dtype)
    got = SM.emulate(case['x'], case['w'], case['b'], dtype)
    r = SM.ratio(got, v, SM.bound(S, D))
    print(f'[simple head emulation {family} {shape}] worst err / bound {r.max():.4f}')
    assert r.max() <= 1
    vu, Su = SM.model(case['x'], case['w'], case['b'], dtype, unsplit=True)
    assert SM.ratio(got, vu, SM.bound(Su, D, dtype, unsplit=True, x=case['x'])).max() <= 1


def test_taps_are_exact():
    """every value of the taps family is a float32 number and the float32 emulation returns exactly it: the GPU test may compare bit for bit"""
    for dtype, D, K in SHAPES + [('fp16', 64, 33)]:
        case = SC.taps(dtype, D, K)
        v, _ = SM.model(case['x'], case['w'], case['b'], dtype)
        assert np.array_equal(v, v.astype(F32).astype(F64))
        assert np.array_equal(SM.emulate(case['x'], case['w'], case['b'], dtype), v.astype(F32))
        assert len(np.unique(v)) > 20          # tent values, not a constant


# the family on which each wrong model is shown failing (others may fail too)
SHOWN = {'align_corners': ('random', 'taps'), 'relu_after_upsample': ('random', 'relu'), 'border_clamp': ('edges', 'corners', 'taps'),
         'kykx_transposed': ('random', 'taps'), 'bias_dropped': ('taps', 'random'), 'lo_dropped': ('lo_plane',)}


@pytest.mark.parametrize('wrong', SM.WRONG)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_wrong_models_fail_the_bound(wrong, shape):
    dtype, D, K = shape
    assert set(SHOWN) == set(SM.WRONG)
    for family in SHOWN[wrong]:
        case = FAMILIES[family](dtype, D, K)
        v, S = SM.model(case['x'], case['w'], case['b'], dtype)
        bad, _ = SM.model(case['x'], case['w'], case['b'], dtype, wrong=wrong)
        r = SM.ratio(bad.astype(F32), v, SM.bound(S, D))
        print(f'[simple head wrong model {wrong} on {family} {shape}] worst err / bound {r.max():.3g}, {np.mean(r > 1):.1%} of the elements outside')
        assert r.max() > 1, (wrong, family)


def test_border_clamp_shows_on_the_border_only():
    dtype, D, K = SHAPES[0]
    case = SC.edges(dtype, D, K)
    v, S = SM.model(case['x'], case['w'], case['b'], dtype)
    bad, _ = SM.model(case['x'], case['w'], case['b'], dtype, wrong='border_clamp')
    r = SM.ratio(bad, v, SM.bound(S, D))
    assert (r[:, :, 1:-1, 1:-1] <= 1).all() and (r[:, :, 0] > 1).any() and (r[:, :, -1] > 1).any() and (r[..., 0] > 1).any() and (r[..., -1] > 1).any()


# ---- the weight image, through the host-only tap

def _pack(dtype, w):
    K, D = w.shape[:2]
    lib = capi.load_library()
    rows = C.c_int32()
    w = np.ascontiguousarray(w, F32)
    assert lib.vp_dbg_simple_head_pack(capi.DTYPES[dtype], K, D, w.ctypes.data, None, C.byref(rows)) == 0, capi.last_error()
    img = np.full((9, rows.value, D), 0xABCD, np.uint16)
    assert lib.vp_dbg_simple_head_pack(capi.DTYPES[dtype], K, D, w.ctypes.data, img.ctypes.data, C.byref(rows)) == 0, capi.last_error()
    return img


def _vals(bits, dtype):
    t = torch.from_numpy(bits.view(np.int16).copy())
    return t.view(torch.float16 if dtype == 'fp16' else torch.bfloat16).float().numpy()


@pytest.mark.parametrize('dtype', ('fp16', 'bf16'))
@pytest.mark.parametrize('K', (1, 16, 17, 33))
def test_weight_image(dtype, K):
    D = 64
    rng = np.random.Generator(np.random.PCG64(K))
    w = (rng.standard_normal((K, D, 3, 3)) * 0.05).astype(F32)
    w[0, 0] = np.arange(1, 10, dtype=F32).reshape(3, 3)           # tap t carries t + 1: the layout is readable
    img = _pack(dtype, w)
    rows = 32 * ((K + 15) // 16)
    assert img.shape == (9, rows, D)
    val = _vals(img, dtype).reshape(9, rows // 32, 2, 16, D)      # [tap][slab][hi / lo][16 maps][D]
    hi, lo = val[:, :, 0].reshape(9, -1, D)[:, :K], val[:, :, 1].reshape(9, -1, D)[:, :K]
    assert np.array_equal(hi[:, 0, 0], np.arange(1, 10, dtype=F32))            # tap t = 3 ky + kx, tap-major
    mhi, mlo = SM.split(w, dtype)
    src = lambda a: a.transpose(2, 3, 0, 1).reshape(9, K, D)
    assert np.array_equal(hi, src(mhi)) and np.array_equal(lo, src(mlo))
    # hi + lo reproduces w to u^2 |w| (the rounding of lo, itself at most u |w|), or half the spacing of the fp16 subnormals where lo falls among them
    u = SM.U16[dtype]
    err = np.abs(hi.astype(F64) + lo.astype(F64) - src(w).astype(F64))
    assert (err <= u * u * np.abs(src(w)) + (2.0 ** -25 if dtype == 'fp16' else 0.0)).all()
    assert (np.abs(hi.astype(F64) - src(w)) > u * u * np.abs(src(w))).any()    # ... which hi alone does not
    pad = val.reshape(9, -1, 2, 16, D).transpose(0, 1, 3, 2, 4).reshape(9, -1, 2, D)[:, K:]
    assert not img.reshape(9, rows // 32, 2, 16, D).transpose(0, 1, 3, 2, 4).reshape(9, -1, 2, D)[:, K:].any() and not pad.any()   # padded rows: zero bits


def test_pack_refusals():
    lib = capi.load_library()
    rows = C.c_int32()
    w = np.zeros((1, 64, 3, 3), F32)
    assert lib.vp_dbg_simple_head_pack(7, 1, 64, w.ctypes.data, None, C.byref(rows)) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_simple_head_pack(0, 0, 64, w.ctypes.data, None, C.byref(rows)) == capi.VP_ERR_INVALID
    assert lib.vp_dbg_simple_head_pack(0, 1, 64, None, None, C.byref(rows)) == capi.VP_ERR_INVALID


# ---- the Python surface

def test_infer_head_from_state_dict_and_synth():
    shape = model_shape('s', 'coco')
    classic = synthetic_state_dict(shape, seed=3)
    simple = synthetic_state_dict(shape, seed=3, head='simple')
    assert infer_head_from_state_dict(classic) == 'classic' and infer_head_from_state_dict(simple) == 'simple'
    assert simple['keypoint_head.final_layer.weight'].shape == (17, 384, 3, 3) and simple['keypoint_head.final_layer.bias'].shape == (17,)
    assert not any(k.startswith('keypoint_head.deconv_layers') for k in simple)
    for k in classic:
        if k.startswith('backbone.'):
            assert np.array_equal(classic[k], simple[k]), k          # the backbone of a seed is one backbone
    both = dict(classic)
    both['keypoint_head.final_layer.weight'] = simple['keypoint_head.final_layer.weight']
    with pytest.raises(ValueError, match='deconv_layers'):
        infer_head_from_state_dict(both)
    odd = dict(simple)
    odd['keypoint_head.final_layer.weight'] = np.zeros((17, 100, 1, 1), F32)
    with pytest.raises(ValueError, match='final_layer.weight'):
        infer_head_from_state_dict(odd)
    assert model_shape('b', 'coco').head == 'classic' and model_shape('b', 'coco', head='simple').head == 'simple'
    lit = 2 * 3072 * 9 * 768 * 17 / 1e9
    assert model_shape('b', 'coco', head='simple').gflop_per_person() < model_shape('b', 'coco').gflop_per_person()
    head = model_shape('b', 'coco', head='simple').gflop_per_person() - (model_shape('b', 'coco').gflop_per_person() - (1572864 * 768 + 1610612736 + 1572864 * 17) / 1e9)
    assert abs(head - (2 * 192 * 9 * 17 * 768 + 72 * 17 * 3072) / 1e9) < 1e-9 and 14 < lit / head < 16      # the 9-tap GEMM is 16 x fewer than the literal form, the stencil adds 8 %


def test_peaked_simple_checkpoint_has_one_clear_maximum_per_joint():
    """the peaked simple-decoder checkpoint through the CPU oracle's backbone and this model: every joint's map has one dominant blob"""
    from oracle import vitpose_cpu as O
    from easy_vitpose_amd.synth import synthetic_crops
    shape = model_shape('s', 'coco')
    sd = synthetic_state_dict(shape, seed=11, peaked=True, head='simple')
    x = torch.from_numpy(O.pre_img(synthetic_crops(1, seed=5, kind='blobs')[0])[0])
    tok = O.backbone_forward(O.to_torch_state_dict(sd), x, shape.depth, shape.num_heads)
    tok = np.asarray(tok.detach().numpy(), F32).reshape(1, 192, shape.embed_dim)
    hm, _ = SM.model(tok, sd['keypoint_head.final_layer.weight'], sd['keypoint_head.final_layer.bias'], 'fp16', unsplit=True)
    hm = hm[0]
    peak = hm.reshape(17, -1).max(1)
    assert (peak > 0.2).all() and (peak < 1.6).all(), peak
    for k in range(17):
        y, xx = np.unravel_index(int(hm[k].argmax()), hm[k].shape)
        far = np.ones_like(hm[k], bool)
        far[max(y - 12, 0):y + 13, max(xx - 12, 0):xx + 13] = False
        assert hm[k][far].max() < 0.5 * peak[k], (k, peak[k], hm[k][far].max())
