"""GPU: simple-decoder checkpoints (ReLU -> bilinear x 4 -> 3x3 conv: csrc/simpleheadgeom.h) end to end, on ViTPose-S and once on ViTPose-B with the peaked synthetic
simple-decoder checkpoint at 3 crops:

    1  vp_infer_heatmaps against the float64 model (tests/simple_head_model.py) applied to the tokens vp_infer_tokens returned, inside the per-element bound
    2  vp_infer keypoints against the oracle's decode of the device's own heatmaps, at the decode tests' 2e-3
    3  the project's contract, +-0.5 px and 1e-3 confidence, against oracle backbone -> the model on float32 tokens and the un-split weights -> the oracle's decode
    4  the flip-test mode, 5 a replayed graph, 6 VitInference on a .pth, 7 the loader's refusals and a classic checkpoint on the same build
The reference cannot execute this decoder and no published `-simple` file is at hand: parity with upstream's binary is NOT pinned here; the float64 model is pinned
against torch's own F.interpolate + F.conv2d in tests/test_simple_head_model.py."""
import os

import numpy as np
import pytest
import torch

import simple_head_model as SM
from easy_vitpose_amd import VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.engine import decode_heatmaps
from easy_vitpose_amd.synth import synthetic_crops, synthetic_moe_state_dict, synthetic_state_dict
from helpers import CONF_TOL, KP_TOL_PX
from oracle import vitpose_cpu as O

pytestmark = pytest.mark.gpu

F32 = np.float32
COCO_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
DECODE_TOL = 2e-3              # tests/test_gpu_parity.py: the device decode against the oracle's on the same heatmaps
SAME_NET_TOL = 2e-3            # tests/test_gpu_flip_mode.py: the same network with other rounding points
N = 3
_cache = {}


def _crops():
    from cases import peaked_crops
    return peaked_crops(N)


def _run(variant):
    """the device's tokens, heatmaps and keypoints of the peaked simple-decoder checkpoint, computed once per variant"""
    if variant not in _cache:
        shp = model_shape(variant, 'coco', head='simple')
        sd = synthetic_state_dict(shp, 0, peaked=True, head='simple')
        eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)
        assert eng.head == 'simple' and eng.shape.head == 'simple' and eng.lib.vp_head_kind(eng._h) == 1
        crops = _crops()
        _cache[variant] = dict(shp=shp, sd=sd, crops=crops, tok=eng.tokens(crops), hm=eng.heatmaps(crops), kp=eng.infer(crops))
        eng.close()
    return _cache[variant]


VARIANTS = ('s', 'b')


@pytest.mark.parametrize('variant', VARIANTS)
def test_heatmaps_on_the_devices_own_tokens(variant):
    r = _run(variant)
    D = r['shp'].embed_dim
    x = SM.round16(r['tok'], 'fp16')                   # the head reads last_norm's output as 16-bit operands
    v, S = SM.model(x, r['sd']['keypoint_head.final_layer.weight'], r['sd']['keypoint_head.final_layer.bias'], 'fp16')
    q = SM.ratio(r['hm'], v, SM.bound(S, D))
    print(f'[simple decoder {variant}] heatmaps vs the model on the device\'s tokens: worst err / bound {q.max():.4f}, max |err| {np.abs(r["hm"] - v).max():.3e}, '
          f'heatmap max {v.max():.3f}')
    assert r['hm'].shape == (N, 17, 64, 48) and q.max() <= 1


@pytest.mark.parametrize('variant', VARIANTS)
def test_decode_on_the_devices_own_heatmaps(variant):
    r = _run(variant)
    d = np.abs(r['kp'] - O.decode_per_crop(r['hm']))
    print(f'[simple decoder {variant}] decode vs the oracle\'s on the device\'s heatmaps: max {d.max():.3e}')
    assert d.max() < DECODE_TOL


@pytest.mark.parametrize('variant', VARIANTS)
def test_contract_against_the_oracle_chain(variant):
    r = _run(variant)
    shp, sd = r['shp'], r['sd']
    x = torch.from_numpy(np.concatenate([O.pre_img(c)[0] for c in r['crops']]))
    tok = O.backbone_forward(O.to_torch_state_dict(sd), x, shp.depth, shp.num_heads).detach().numpy().astype(F32)
    ref_hm, _ = SM.model(tok, sd['keypoint_head.final_layer.weight'], sd['keypoint_head.final_layer.bias'], 'fp16', unsplit=True)
    ref_hm = ref_hm.astype(F32)
    ref = O.decode_per_crop(ref_hm)
    dpx = np.abs(r['kp'][..., :2] - ref[..., :2]).max(-1)
    dcf = np.abs(r['kp'][..., 2] - ref[..., 2])
    herr = np.abs(r['hm'] - ref_hm)
    print(f'[simple decoder {variant}] vs oracle backbone -> model -> oracle decode, {dpx.size} joints: coordinate max err {dpx.max():.4f} px (mean {dpx.mean():.4f}), '
          f'confidence max err {dcf.max():.3e} (rms {np.sqrt((dcf ** 2).mean()):.3e}), heatmap max err {herr.max():.3e}, peaks {ref[..., 2].min():.3f} .. {ref[..., 2].max():.3f}')
    assert dpx.max() < KP_TOL_PX and dcf.max() < CONF_TOL


def test_flip_test_mode():
    r = _run('s')
    eng = VitPoseHip(r['shp'], r['sd'], dtype='fp16', max_batch=8)
    mirrored = np.ascontiguousarray(r['crops'][:, :, ::-1])
    hm_m = eng.heatmaps(mirrored)
    eng.set_flip_test(COCO_PAIRS)
    kp, avg = eng.infer(r['crops']), eng.heatmaps(r['crops'])
    eng.close()
    assert np.array_equal(kp, decode_heatmaps(avg))                       # the mode's decode is the decode of the average it returns, bit for bit
    want = F32(0.5) * (r['hm'] + O.flip_back(hm_m, COCO_PAIRS))          # ... and that average is the crop's and its mirror's maps of two plain forwards
    d = np.abs(avg - want).max()
    cf = np.abs(kp[..., 2] - O.decode_per_crop(want)[..., 2]).max()
    print(f'[simple decoder flip mode] averaged maps vs two plain forwards: max |diff| {d:.3e}, confidence {cf:.3e}')
    assert d < SAME_NET_TOL and cf < CONF_TOL
    assert not np.array_equal(kp, r['kp'])


def test_graph_replay_gives_the_eager_bits(monkeypatch):
    r = _run('s')
    monkeypatch.setenv('VP_GRAPH', '0')
    eng = VitPoseHip(r['shp'], r['sd'], dtype='fp16', max_batch=4)
    ref = eng.infer(r['crops'])
    eng.close()
    monkeypatch.setenv('VP_GRAPH', '1')
    eng = VitPoseHip(r['shp'], r['sd'], dtype='fp16', max_batch=4)
    outs = [eng.infer(r['crops']) for _ in range(4)]                      # eager, capture + launch, replay, replay
    eng.close()
    assert np.array_equal(ref, r['kp'])
    for o in outs:
        assert np.array_equal(o, ref)


def test_vitinference_loads_a_simple_pth(tmp_path):
    from easy_vitpose_amd import VitInference
    r = _run('s')
    path = os.path.join(tmp_path, 'vitpose-s-simple-coco.pth')           # infer_dataset_by_path reads `coco`; `vitpose-s-simple.pth` would read `simple`
    torch.save({'state_dict': {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in r['sd'].items()}}, path)
    crops = synthetic_crops(2, 4, 'blobs')
    frame = np.zeros((480, 640, 3), np.uint8)
    frame[100:356, 50:242] = crops[0]
    frame[150:406, 400:592] = crops[1]
    boxes = np.array([[60, 110, 232, 346, 0.9], [410, 160, 582, 396, 0.8]], dtype=np.float64)   # + 10 px of padding: exactly the two crops, no resize
    model = VitInference(path, lambda img: boxes.copy(), max_batch=8)
    assert model._vit_pose.head == 'simple' and model.dataset == 'coco'
    res = model.inference(frame.copy())
    eng = VitPoseHip(r['shp'], r['sd'], dtype='fp16', max_batch=8)
    kp = eng.infer(crops)
    eng.close()
    assert sorted(res.keys()) == [0, 1]
    for i, (top, left) in enumerate(((100, 50), (150, 400))):
        assert np.array_equal(res[i][:, 2], kp[i, :, 2])
        assert np.abs(res[i][:, :2] - (kp[i, :, :2] + np.array([top, left], F32))).max() < 1e-4   # one float32 addition of the crop's corner
    with pytest.raises(AssertionError, match='dataset'):
        bad = os.path.join(tmp_path, 'vitpose-s-simple.pth')
        os.replace(path, bad)
        VitInference(bad, lambda img: boxes.copy(), max_batch=8)


def _load_error(shp, sd):
    with pytest.raises((KeyError, RuntimeError, capi.VpError)) as e:
        VitPoseHip(shp, sd, dtype='fp16', max_batch=2)
    return e.type, str(e.value)


def test_loader_refusals():
    """KeyError = VP_ERR_MISSING_TENSOR, RuntimeError = VP_ERR_SHAPE (engine._load), VpError carries its code"""
    shp = model_shape('s', 'coco')
    classic, simple = synthetic_state_dict(shp, 0), synthetic_state_dict(shp, 0, head='simple')
    fw, fb = 'keypoint_head.final_layer.weight', 'keypoint_head.final_layer.bias'
    both = dict(classic)
    both[fw] = simple[fw]
    t, msg = _load_error(shp, both)
    assert t is RuntimeError and fw in msg and 'keypoint_head.deconv_layers.' in msg
    odd = dict(simple)
    odd[fw] = np.zeros((17, 100, 1, 1), F32)
    t, msg = _load_error(shp, odd)
    assert t is RuntimeError and fw in msg and '1700' in msg
    nobias = {k: v for k, v in simple.items() if k != fb}
    t, msg = _load_error(shp, nobias)
    assert t is KeyError and fb in msg
    headless = {k: v for k, v in classic.items() if not k.startswith('keypoint_head.deconv_layers.')}
    t, msg = _load_error(shp, headless)                                   # a 1x1 final layer without its deconvs: the classic loader's own refusal
    assert t is KeyError and 'keypoint_head.deconv_layers.0.weight' in msg
    plus = synthetic_moe_state_dict(shp, 192)
    plus = {k: v for k, v in plus.items() if not k.startswith('keypoint_head.deconv_layers.')}
    plus[fw] = simple[fw]
    t, msg = _load_error(shp, plus)
    assert t is capi.VpError and f'status {capi.VP_ERR_INVALID}' in msg and fw in msg and 'no such checkpoints exist' in msg


def test_classic_checkpoint_on_the_same_build(golden_dir):
    """one existing golden, read only: the classic peaked ViTPose-S keypoints of the reference's own _inference_torch"""
    from cases import peaked_crops
    z = np.load(os.path.join(golden_dir, 'peaked_s_coco.npz'))
    n = int(z['n'])
    shp = model_shape('s', 'coco')
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=n)
    assert eng.head == 'classic' and eng.lib.vp_head_kind(eng._h) == 0
    kp = eng.infer(peaked_crops(n))
    eng.close()
    assert np.abs(kp[..., :2] - z['keypoints'][..., :2]).max() < KP_TOL_PX and np.abs(kp[..., 2] - z['keypoints'][..., 2]).max() < CONF_TOL
