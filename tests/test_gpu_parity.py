"""GPU: the HIP path (through the C ABI) against the CPU oracle and the committed
reference goldens, plus size-independent properties at the BASELINE batch size.

Tolerances (north_star): keypoint coordinates +-0.5 px, confidences 1e-3, against the
reference torch-CPU path.  Random-weight heatmaps are noise-like, so (SURVEY.md 7,
"parity is ill-conditioned on random weights") coordinate parity is asserted on joints
whose arg-max margin exceeds the heatmap error and whose DARK step is well-conditioned;
the fraction of joints that qualifies is asserted too, and heatmap-tensor error is
asserted on ALL joints.
"""
import os

import numpy as np
import pytest

from cases import org_sizes, peaked_heatmaps
from easy_vitpose_amd import VitInference, VitPoseHip, decode_heatmaps
from easy_vitpose_amd.synth import synthetic_crops
from helpers import (CONF_TOL, KP_TOL_PX, argmax_margin, dark_conditioned, dark_offset_px, oracle_heatmaps,
                     weights)
from oracle import vitpose_cpu as O

pytestmark = pytest.mark.gpu

# measured-error budgets per operand type (heatmap std of the synthetic checkpoints ~0.3)
HM_MAX_ERR = {'fp16': 4e-3, 'bf16': 3e-2}
HM_RMS_ERR = {'fp16': 6e-4, 'bf16': 5e-3}
CONF_ERR = {'fp16': CONF_TOL, 'bf16': 1.5e-2}   # bf16 operands do NOT meet the 1e-3 confidence bar


# ----------------------------------------------------------------------------- decode
@pytest.mark.parametrize('tag', ['decode_k17', 'decode_k133'])
def test_decode_matches_reference_golden(golden_dir, tag):
    """The reference's own outputs under one flat tolerance.  The per-joint check -- a float64 model of the kernel, a derived bound and a conditioning class per
    joint, ties, borders, the wrap and the clip bounds -- is tests/test_gpu_decode.py (tests/decode_model.py, tests/decode_cases.py)."""
    z = np.load(os.path.join(golden_dir, f'{tag}.npz'))
    n, k, seed = int(z['n']), int(z['k']), int(z['seed'])
    hm, wh = peaked_heatmaps(n, k, seed), org_sizes(n, seed)
    got = decode_heatmaps(hm, wh)
    exp = z['expected']
    assert np.array_equal(got[..., 2], exp[..., 2])              # confidences: bit exact
    d = np.abs(got[..., :2] - exp[..., :2])
    # flat map (crop 4, joint 5): Hessian is eps*I -> exact zero step in both
    assert d.max() < 2e-3, f'decode vs reference golden: {d.max():.3e} px'
    assert np.abs(got - O.decode_per_crop(hm, wh)).max() < 2e-3  # and vs the oracle


def test_decode_large_batch_properties():
    """BASELINE size (256 x 17 joints): batched decode == per-crop decode, permutation equivariant."""
    hm = peaked_heatmaps(256, 17, 99)
    full = decode_heatmaps(hm)
    perm = np.random.default_rng(0).permutation(256)
    assert np.array_equal(decode_heatmaps(hm[perm]), full[perm])
    idx = [0, 1, 2, 3, 4, 100, 255]
    single = np.concatenate([decode_heatmaps(hm[i:i + 1]) for i in idx])
    assert np.array_equal(single, full[idx])                     # no cross-crop coupling (the reference's N*K>5084 bug)
    ref = O.decode_per_crop(hm[:16])
    assert np.abs(full[:16] - ref).max() < 2e-3


# ------------------------------------------------------------------------------ model
def _engine(variant, dataset, dtype, max_batch=8):
    shp, sd, _ = weights(variant, dataset)
    return VitPoseHip(shp, sd, dtype=dtype, device_id=0, max_batch=max_batch)


@pytest.mark.parametrize('variant,dataset,n', [('l', 'coco_25', 2), ('h', 'wholebody', 2)])
def test_large_variants_parity_vs_oracle(variant, dataset, n):
    """ViTPose-L (D = 1024, 24 blocks, K = 25) and ViTPose-H (head dim 80, 32 blocks, K = 133 -> three n-tiles of hi+lo
    final-conv weights): heatmaps and confidences against the oracle on fresh crops (the goldens hold one crop each)."""
    crops = synthetic_crops(n, 17, 'blobs')
    ref_hm = oracle_heatmaps(variant, dataset, crops, chunk=1)
    eng = _engine(variant, dataset, 'fp16', max_batch=n)
    hm = eng.heatmaps(crops)
    err = np.abs(hm - ref_hm)
    print(f'[{variant}/fp16] heatmap std {ref_hm.std():.3f}  max|err| {err.max():.3e}  rms {np.sqrt((err ** 2).mean()):.3e}')
    assert err.max() < HM_MAX_ERR['fp16'] and np.sqrt((err ** 2).mean()) < HM_RMS_ERR['fp16']
    kp = eng.infer(crops)
    ref_kp = O.decode_per_crop(ref_hm)
    cerr = np.abs(kp[..., 2] - ref_kp[..., 2])
    print(f'[{variant}/fp16] confidence max err {cerr.max():.3e}, rms {np.sqrt((cerr ** 2).mean()):.3e}, {(cerr < CONF_TOL).mean():.4f} of {cerr.size} joints within 1e-3')
    # random-weight heatmaps are full-scale noise (std 0.3, maxima ~1): with 16-bit operands the error at the arg-max is
    # ~N(0, 3e-4) on the 32-block model, so 1e-3 is a 3-sigma event per joint.  North-star criterion on >= 95 % of the joints
    # here; on EVERY joint (1064 of them) with the peaked checkpoint, test_peaked_checkpoint_end_to_end_vs_reference_golden
    assert (cerr < CONF_TOL).mean() >= 0.95 and np.sqrt((cerr ** 2).mean()) < 0.5 * CONF_TOL
    eng.close()


@pytest.mark.parametrize('variant,dataset', [('s', 'coco'), ('b', 'coco'), ('l', 'coco_25'), ('h', 'wholebody')])
def test_peaked_checkpoint_end_to_end_vs_reference_golden(golden_dir, variant, dataset):
    """End-to-end north_star tolerances on EVERY joint: the peaked synthetic checkpoint gives one Gaussian-like blob per joint,
    the goldens are keypoints of the reference's own `_inference_torch` (136 / 136 / 100 / 1064 joints), and the device
    path must sit within +-0.5 px and 1e-3 of them -- no conditioning filter, no per-variant multiplier."""
    from cases import peaked_crops
    from easy_vitpose_amd.synth import synthetic_state_dict
    from easy_vitpose_amd.configs import model_shape
    z = np.load(os.path.join(golden_dir, f'peaked_{variant}_{dataset}.npz'))
    n = int(z['n'])
    shp = model_shape(variant, dataset)
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', device_id=0, max_batch=n)
    crops = peaked_crops(n)
    kp = eng.infer(crops)
    hm0 = eng.heatmaps(crops[:1])
    eng.close()
    ref = z['keypoints']
    dpx = np.abs(kp[..., :2] - ref[..., :2]).max(-1)
    dcf = np.abs(kp[..., 2] - ref[..., 2])
    herr = np.abs(hm0[:, :16] - z['heatmaps0'])
    print(f'[{variant}/peaked] {dpx.size} joints: coordinate max err {dpx.max():.4f} px (mean {dpx.mean():.4f}), confidence max err {dcf.max():.3e} '
          f'(rms {np.sqrt((dcf ** 2).mean()):.3e}), heatmap max err {herr.max():.3e}')
    ok = (dpx < KP_TOL_PX) & (dcf < CONF_TOL)
    assert ok.mean() >= 0.95, f'only {ok.mean():.3f} of the joints within +-0.5 px / 1e-3'
    assert dpx.max() < KP_TOL_PX and dcf.max() < CONF_TOL           # in fact all of them


@pytest.mark.parametrize('fuse_ln', ['1', '0'])
@pytest.mark.parametrize('variant,dataset', [('s', 'coco'), ('b', 'coco'), ('l', 'coco_25'), ('h', 'wholebody')])
def test_outlier_checkpoint_end_to_end_vs_reference_golden(golden_dir, variant, dataset, fuse_ln, monkeypatch):
    """Trained-ViT-like activation statistics: the peaked checkpoint with four residual channels at 100-1000 x
    the scale of the others from block 3 on (two constant +800 / -600, two token-dependent with |x| up to ~600) and an attention
    head whose logits reach ~45.  Goldens = the reference's own `_inference_torch` keypoints; +-0.5 px and 1e-3 on EVERY joint,
    through the fused-LayerNorm path (fp16 hi plane of the un-normalised rows as the GEMM operand, `rstd (acc - mean s)` fold,
    granule-merged row statistics) and through the standalone-LayerNorm path (VP_FUSE_LN=0)."""
    from cases import peaked_crops
    from easy_vitpose_amd.synth import synthetic_state_dict
    from easy_vitpose_amd.configs import model_shape
    monkeypatch.setenv('VP_FUSE_LN', fuse_ln)
    z = np.load(os.path.join(golden_dir, f'peaked_outlier_{variant}_{dataset}.npz'))
    n = int(z['n'])
    shp = model_shape(variant, dataset)
    eng = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True, outliers=True), dtype='fp16', device_id=0, max_batch=n)
    crops = peaked_crops(n)
    kp = eng.infer(crops)
    hm0 = eng.heatmaps(crops[:1])
    eng.close()
    ref = z['keypoints']
    assert np.isfinite(kp).all() and np.isfinite(hm0).all()
    dpx = np.abs(kp[..., :2] - ref[..., :2]).max(-1)
    dcf = np.abs(kp[..., 2] - ref[..., 2])
    herr = np.abs(hm0[:, :16] - z['heatmaps0'])
    print(f'[{variant}/outliers, fuse_ln={fuse_ln}] {dpx.size} joints: coordinate max err {dpx.max():.4f} px (mean {dpx.mean():.4f}), '
          f'confidence max err {dcf.max():.3e} (rms {np.sqrt((dcf ** 2).mean()):.3e}), heatmap max err {herr.max():.3e}')
    assert dpx.max() < KP_TOL_PX and dcf.max() < CONF_TOL


@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
@pytest.mark.parametrize('variant,dataset,n', [('s', 'coco', 16), ('b', 'coco', 8)])
def test_model_parity_vs_oracle(variant, dataset, n, dtype):
    crops = np.concatenate([synthetic_crops(n // 4, 7, 'blobs'), synthetic_crops(n - n // 4, 8, 'noise')])
    ref_hm = oracle_heatmaps(variant, dataset, crops)
    eng = _engine(variant, dataset, dtype, max_batch=16)
    hm = eng.heatmaps(crops)
    err = np.abs(hm - ref_hm)
    rms = float(np.sqrt((err ** 2).mean()))
    print(f'[{variant}/{dtype}] heatmap std {ref_hm.std():.3f}  max|err| {err.max():.3e}  rms {rms:.3e}')
    assert err.max() < HM_MAX_ERR[dtype] and rms < HM_RMS_ERR[dtype]
    kp = eng.infer(crops)
    ref_kp = O.decode_per_crop(ref_hm)
    # decode kernel on the device heatmaps == oracle decode of the same heatmaps (isolates decode from model error)
    assert np.array_equal(kp[..., 2], hm.reshape(n, -1, 3072).max(-1))
    cerr = np.abs(kp[..., 2] - ref_kp[..., 2])
    print(f'[{variant}/{dtype}] confidence max err {cerr.max():.3e} (tol {CONF_ERR[dtype]:.1e})')
    assert cerr.max() < CONF_ERR[dtype]
    # coordinates on these noise-like maps: only where the arg-max cannot flip under the measured error and the DARK step is
    # well-posed in the reference itself (a handful of joints); the real coordinate assertion -- EVERY joint -- is the peaked
    # checkpoint below and test_peaked_checkpoint_end_to_end_vs_reference_golden
    ok = (argmax_margin(ref_hm) > 4 * err.max()) & dark_conditioned(ref_hm) & (dark_offset_px(ref_kp, ref_hm) < 1.5)
    if ok.any():
        d = np.abs(kp[..., :2] - ref_kp[..., :2])[ok]
        print(f'[{variant}/{dtype}] noise maps: keypoint max err {d.max():.3f} px on the {ok.sum()} conditioned joints of {ok.size}')
        assert d.max() < KP_TOL_PX
    # the same crops through the PEAKED checkpoint of this variant, against the oracle computed here: all joints
    from easy_vitpose_amd.synth import synthetic_state_dict
    from easy_vitpose_amd.configs import model_shape
    shp = model_shape(variant, dataset)
    psd = synthetic_state_dict(shp, 0, peaked=True)
    peng = VitPoseHip(shp, psd, dtype=dtype, device_id=0, max_batch=16)
    pkp = peng.infer(crops)
    peng.close()
    psdt = O.to_torch_state_dict(psd)
    pref = np.concatenate([O.inference_torch(psdt, shp.depth, shp.num_heads, c) for c in crops])
    dpx, dcf = np.abs(pkp[..., :2] - pref[..., :2]).max(-1), np.abs(pkp[..., 2] - pref[..., 2])
    print(f'[{variant}/{dtype}] peaked checkpoint, {dpx.size} joints: coordinate max err {dpx.max():.4f} px, confidence max err {dcf.max():.3e}')
    if dtype == 'fp16':
        assert dpx.max() < KP_TOL_PX and dcf.max() < CONF_TOL
    else:   # bf16 operands: coordinates hold, confidences do not meet 1e-3
        assert dpx.max() < KP_TOL_PX and dcf.max() < CONF_ERR['bf16']
    # composition check on REALISTIC maps: add the measured device error tensor to peaked (trained-model-like)
    # heatmaps and decode both -- every joint must stay within the north_star tolerances
    pk = peaked_heatmaps(n, ref_hm.shape[1], 31)[:, :, :, :]
    valid = pk.reshape(n, -1, 3072).max(-1) > 0.05
    for i, j in [(1, 0), (2, 3), (3, 2), (4, 5)]:   # the deliberately degenerate joints (<=0, tie, flat) are not peaks
        valid[i, j] = False
    moved = decode_heatmaps(pk + (hm - ref_hm)) - decode_heatmaps(pk)
    print(f'[{variant}/{dtype}] peaked maps + device error: max coord shift {np.abs(moved[..., :2])[valid].max():.4f} px, '
          f'conf shift {np.abs(moved[..., 2])[valid].max():.2e}')
    if dtype == 'fp16':
        assert np.abs(moved[..., :2])[valid].max() < KP_TOL_PX and np.abs(moved[..., 2])[valid].max() < CONF_TOL
    eng.close()


@pytest.mark.parametrize('variant,dataset', [('s', 'coco'), ('b', 'coco'), ('l', 'coco_25'), ('h', 'wholebody')])
def test_model_matches_reference_golden(golden_dir, variant, dataset):
    """HIP heatmaps / confidences vs outputs of the reference itself (fixtures)."""
    z = np.load(os.path.join(golden_dir, f'model_{variant}_{dataset}.npz'))
    crops = synthetic_crops(int(z['n']), int(z['crop_seed']), str(z['kind']))
    eng = _engine(variant, dataset, 'fp16', max_batch=2)
    hm = eng.heatmaps(crops)
    exp = z['heatmaps']
    err = np.abs(hm[:, :exp.shape[1]] - exp)
    print(f'[{variant}] vs reference golden: max|err| {err.max():.3e} (hm std {exp.std():.3f})')
    assert err.max() < HM_MAX_ERR['fp16']
    kp = eng.infer(crops)
    cerr = np.abs(kp[..., 2] - z['keypoints'][..., 2])
    print(f'[{variant}] vs reference golden: confidence max err {cerr.max():.3e}, {(cerr < CONF_TOL).mean():.4f} of {cerr.size} joints within 1e-3')
    assert (cerr < CONF_TOL).mean() >= 0.95 and np.sqrt((cerr ** 2).mean()) < 0.5 * CONF_TOL   # noise-like maps: see above
    eng.close()


def test_tokens_tap_and_input_formats():
    """Backbone output after last_norm vs oracle; uint8 NHWC input == float32 NCHW input of pre_img."""
    shp, sd, sdt = weights('s', 'coco')
    crops = synthetic_crops(3, 5, 'noise')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)
    x = np.concatenate([O.pre_img(c)[0] for c in crops])
    import torch
    ref_tok = O.backbone_forward(sdt, torch.from_numpy(x), shp.depth, shp.num_heads).numpy()
    tok = eng.tokens(crops)
    assert np.abs(tok - ref_tok).max() < 2e-2 and np.sqrt(((tok - ref_tok) ** 2).mean()) < 2e-3
    assert np.array_equal(eng.heatmaps(crops), eng.heatmaps(x))   # device normalisation is bit-identical to pre_img
    eng.close()


@pytest.mark.usefixtures('one_launch_family')
def test_batching_edge_cases():
    """empty batch, batch 1, ragged chunking over max_batch, determinism, batch invariance."""
    shp, sd, _ = weights('s', 'coco')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)
    crops = synthetic_crops(11, 21, 'blobs')
    assert eng.infer(crops[:0]).shape == (0, 17, 3)
    full = eng.infer(crops)                                       # 4 + 4 + 3
    assert np.array_equal(full, eng.infer(crops))                 # deterministic
    assert np.array_equal(full[4:5], eng.infer(crops[4:5]))       # batch-size invariant, bit for bit
    assert np.array_equal(full[::-1], eng.infer(crops[::-1]))     # permutation equivariant
    wh = org_sizes(11, 5)
    scaled = eng.infer(crops, wh)
    assert np.array_equal(scaled[..., 2], full[..., 2])
    exp_x = (full[..., 1].astype(np.float64) / (192 / 47.0)) * (wh[:, None, 0] / 47.0) + (wh[:, None, 0] // 2 - wh[:, None, 0] * 0.5)
    assert np.abs(scaled[..., 1] - exp_x).max() < 1e-3 * max(1.0, float(np.abs(exp_x).max()) / 100)
    eng.close()


def test_state_dict_errors():
    shp, sd, _ = weights('s', 'coco')
    bad = dict(sd); del bad['backbone.blocks.3.mlp.fc1.weight']
    with pytest.raises(KeyError):
        VitPoseHip(shp, bad, max_batch=1)
    bad = dict(sd); bad['backbone.pos_embed'] = bad['backbone.pos_embed'][:, :100]
    with pytest.raises(RuntimeError):
        VitPoseHip(shp, bad, max_batch=1)


@pytest.mark.usefixtures('one_launch_family')
def test_baseline_batch_properties():
    """ViTPose-B, batch 256 (BASELINE config 2): crop i of the big batch == crop i alone;
    spot parity of 4 crops against the oracle."""
    shp, sd, _ = weights('b', 'coco')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=256)
    crops = synthetic_crops(256, 0, 'noise')
    crops[:8] = synthetic_crops(8, 1, 'blobs')
    out = eng.infer(crops)
    assert out.shape == (256, 17, 3) and np.isfinite(out).all()
    idx = [0, 3, 100, 255]
    assert np.array_equal(np.concatenate([eng.infer(crops[i:i + 1]) for i in idx]), out[idx])
    # ALL 256 crops against the small-batch path (64x64 / 128x128 tiles, one tile per workgroup, no 8-phase kernel): the
    # production kernels of the BASELINE batch must reproduce it bit for bit
    small = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
    assert np.array_equal(small.infer(crops), out)
    small.close()
    ref_hm = oracle_heatmaps('b', 'coco', crops[idx])
    ref = O.decode_per_crop(ref_hm)
    assert np.abs(out[idx][..., 2] - ref[..., 2]).max() < CONF_TOL
    eng.close()


@pytest.mark.usefixtures('one_launch_family')
def test_config5_ap10k_batch512_workload():
    """BASELINE configs[4]'s WORKLOAD -- ViTPose-B / AP-10K (17 animal joints, configs/ViTPose_ap10k.py:4-22), batch 512 on one
    GPU -- through the shipped fp16 path (its fp8 operands are tolerance-infeasible: DESIGN.md section 6, confirmed on the hardware by
    test_fp8_probe_confirms_the_emulation).  Full-batch properties: finite, crop i of 512 == crop i alone, all 512 == the
    small-batch path bit for bit; parity on 8 crops: heatmaps and confidences against the fp32 oracle on the bench's random
    checkpoint, +-0.5 px / 1e-3 on every joint with the peaked checkpoint."""
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.synth import synthetic_state_dict
    shp, sd, _ = weights('b', 'ap10k')
    assert (shp.embed_dim, shp.depth, shp.num_heads, shp.num_keypoints) == (768, 12, 12, 17)
    crops = synthetic_crops(512, 5, 'noise')
    crops[:16] = synthetic_crops(16, 6, 'blobs')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=512)
    out = eng.infer(crops)
    assert out.shape == (512, 17, 3) and np.isfinite(out).all()
    assert np.array_equal(eng.infer(crops), out)                                        # run-to-run
    idx = [0, 7, 255, 256, 300, 448, 510, 511]
    assert np.array_equal(np.concatenate([eng.infer(crops[i:i + 1]) for i in idx]), out[idx])
    hm = eng.heatmaps(crops[idx])
    eng.close()
    small = VitPoseHip(shp, sd, dtype='fp16', max_batch=16)
    assert np.array_equal(small.infer(crops), out)                                      # 32 chunks of 16 crops, other kernels
    small.close()
    ref_hm = oracle_heatmaps('b', 'ap10k', crops[idx])
    ref = O.decode_per_crop(ref_hm)
    err = np.abs(hm - ref_hm)
    cerr = np.abs(out[idx][..., 2] - ref[..., 2])
    print(f'[b/ap10k @512] heatmap max err {err.max():.3e} rms {np.sqrt((err ** 2).mean()):.3e}; confidence max err {cerr.max():.3e} over {cerr.size} joints')
    assert err.max() < HM_MAX_ERR['fp16'] and np.sqrt((err ** 2).mean()) < HM_RMS_ERR['fp16']
    assert (cerr < CONF_TOL).mean() >= 0.95 and np.sqrt((cerr ** 2).mean()) < 0.5 * CONF_TOL     # noise-like maps: see test_large_variants_parity_vs_oracle
    # coordinates on every joint: the peaked AP-10K checkpoint at the same batch size
    psd = synthetic_state_dict(model_shape('b', 'ap10k'), 0, peaked=True)
    peng = VitPoseHip(shp, psd, dtype='fp16', max_batch=512)
    pout = peng.infer(crops)
    peng.close()
    psdt = O.to_torch_state_dict(psd)
    pref = np.concatenate([O.inference_torch(psdt, shp.depth, shp.num_heads, crops[i]) for i in idx])
    dpx = np.abs(pout[idx][..., :2] - pref[..., :2]).max(-1)
    dcf = np.abs(pout[idx][..., 2] - pref[..., 2])
    print(f'[b/ap10k @512, peaked] {dpx.size} joints: coordinate max err {dpx.max():.4f} px, confidence max err {dcf.max():.3e}')
    assert dpx.max() < KP_TOL_PX and dcf.max() < CONF_TOL


def test_persistent_gemm_is_bit_identical(monkeypatch):
    """qkv / fc1 run as persistent workgroups (operand ring carried across tile boundaries) once a launch has >= 1024
    tiles; the arithmetic per tile is unchanged, so keypoints must be bit-identical to the one-tile-per-workgroup
    launch -- repeated, because a ring/barrier race would show up as run-to-run differences."""
    shp, sd, _ = weights('b', 'coco')
    crops = synthetic_crops(64, 21, 'noise')          # 64 x 18 = 1152 qkv tiles, 1536 fc1 tiles
    out = {}
    monkeypatch.setenv('VP_FUSE_QKV_ATTN', '0')       # attn.qkv as a GEMM of its own (otherwise the fused qkv + attention kernel takes it at this size)
    monkeypatch.setenv('VP_GEMM8', '0')               # and on the 2-phase kernels, where the persistent variant lives
    for flag in ('0', '1'):
        monkeypatch.setenv('VP_PERSIST', flag)
        eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=64)
        out[flag] = [eng.infer(crops) for _ in range(4)]
        eng.close()
    for o in out['0'][1:] + out['1']:
        assert np.array_equal(o, out['0'][0])


# ------------------------------------------------------------------- VitInference API
@pytest.mark.usefixtures('one_launch_family')
def test_vitinference_surface_with_fake_detector():
    shp, sd, sdt = weights('s', 'coco')
    frame = np.zeros((480, 640, 3), np.uint8)
    crops = synthetic_crops(2, 4, 'blobs')
    frame[100:356, 50:242] = crops[0]
    frame[150:406, 400:592] = crops[1]
    boxes = np.array([[60, 110, 232, 346, 0.9], [410, 160, 582, 396, 0.8], [0, 0, 50, 50, 0.2]], dtype=np.float64)
    model = VitInference(sd, lambda img: boxes.copy(), model_name='s', dataset='coco', max_batch=4)
    res = model.inference(frame)
    assert sorted(res.keys()) == [0, 1] and res[0].shape == (17, 3) and res[0].dtype == np.float32
    # the padded boxes are exactly the 192x256 pasted crops -> per-crop oracle on the same pixels
    for i, (x0, y0) in enumerate([(50, 100), (400, 150)]):
        crop = frame[y0:y0 + 256, x0:x0 + 192]
        ref = O.inference_torch(sdt, shp.depth, shp.num_heads, crop)[0]
        ref[:, :2] += [y0, x0]
        assert np.abs(res[i][:, 2] - ref[:, 2]).max() < CONF_TOL
        single = model._inference(crop)
        assert single.shape == (1, 17, 3)
        assert np.allclose(single[0][:, :2] + [y0, x0], res[i][:, :2], atol=1e-3)
    assert model._keypoints is res and model.frame_counter == 1
    hm = peaked_heatmaps(1, 17, 5)
    assert np.abs(VitInference.postprocess(hm, 192, 256) - O.postprocess(hm.copy(), 192, 256)).max() < 2e-3


def test_frame_inference_matches_reference_golden(golden_dir):
    """`VitInference.inference(frame)` against the output of the REFERENCE's own `VitInference.inference` on the
    same frame and detector output (tests/golden/frame_inference.npz: a fake ultralytics result object drove the
    reference's box loop, pad_image, per-box model call and offset arithmetic; cv2.resize = the repo's
    restatement, see make_golden.py).  Confidences within 1e-3; coordinates on the joints whose arg-max and DARK
    step are well-posed in the reference."""
    from cases import frame_case
    g = np.load(os.path.join(golden_dir, 'frame_inference.npz'))
    frame, boxes = frame_case()
    shp, sd, sdt = weights('s', 'coco')
    model = VitInference(sd, lambda img: boxes.copy(), model_name='s', dataset='coco', max_batch=4)
    res = model.inference(frame.copy())
    assert sorted(res.keys()) == g['ids'].tolist()
    tb, ids, scores = model._tracker_res
    assert np.array_equal(np.asarray(tb), g['padded_boxes']) and list(scores) == g['scores'].tolist()
    kp = np.stack([res[i] for i in g['ids']])
    ref = g['keypoints']
    cerr = np.abs(kp[..., 2] - ref[..., 2]).max()
    print(f'frame golden: confidence max err {cerr:.3e}')
    assert cerr < CONF_TOL
    # Coordinates: these noise-like maps have NO joint whose DARK step is well-conditioned in the reference itself
    # (helpers.dark_conditioned), so sub-pixel parity is asserted elsewhere (peaked maps, model parity tests).  What
    # this golden pins is the caller arithmetic -- box padding, pad_image offsets, crop -> frame transform: on joints
    # whose arg-max cannot flip and whose reference DARK step is moderate, the frame coordinates agree to the
    # north_star's 0.5 px of the model-input grid, scaled to frame pixels (measured: 0.015 px).
    from easy_vitpose_amd.cropprep import crop_params, prepare_crops_host
    det = boxes[boxes[:, 4] > 0.35]
    p = crop_params(det[:, :4].round().astype(int), frame.shape[:2], 10)
    ref_hm = oracle_heatmaps('s', 'coco', prepare_crops_host(frame, p))
    ok = (argmax_margin(ref_hm) > 5e-3) & (dark_offset_px(O.decode_per_crop(ref_hm, p[:, 6:8]), ref_hm, p[:, 6:8]) < 1.5)
    assert ok.sum() >= 10
    tol_y = (KP_TOL_PX * np.maximum(p[:, 7] / 256.0, 1.0))[:, None] * np.ones_like(ok, dtype=np.float64)
    tol_x = (KP_TOL_PX * np.maximum(p[:, 6] / 192.0, 1.0))[:, None] * np.ones_like(ok, dtype=np.float64)
    dy, dx = np.abs(kp[..., 0] - ref[..., 0]), np.abs(kp[..., 1] - ref[..., 1])
    print(f'frame golden: frame-coordinate max err y {dy[ok].max():.3f} x {dx[ok].max():.3f} px on {ok.sum()} of {ok.size} joints')
    assert (dy[ok] < tol_y[ok]).all() and (dx[ok] < tol_x[ok]).all()


def test_device_crop_prep_bit_exact_and_frame_entry():
    """crop + zero-pad + OpenCV-style resize on device == the host restatement, bit for bit;
    vp_infer_frame == vp_infer on the host-prepared crops."""
    from easy_vitpose_amd.cropprep import crop_params, prepare_crops_host
    from easy_vitpose_amd.engine import crop_prep_device
    rng = np.random.default_rng(17)
    frame = rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    boxes = np.array([[60, 110, 232, 346], [0, 0, 50, 300], [1200, 600, 1280, 720], [300, 100, 700, 650],
                      [500, 200, 874, 702], [10, 10, 1270, 700], [640, 300, 660, 340]], dtype=np.float64)
    boxes = np.concatenate([boxes, np.ones((len(boxes), 1))], 1)
    p = crop_params(boxes, frame.shape[:2])
    p[4] = (500, 200, 384, 512, 0, 0, 384, 512)           # exactly 2x -> box-average path
    host = prepare_crops_host(frame, p)
    dev = crop_prep_device(frame, p)
    assert np.array_equal(dev, host), f'{(dev != host).sum()} differing bytes'
    # and against the INDEPENDENT checker (oracle/resize_ref.c: scalar-C restatement of OpenCV's resize, not the product's numpy)
    from oracle.resize_ref import resize_linear_u8 as resize_ref
    for i, (x0, y0, cw, ch, left, top, pw, ph) in enumerate(p):
        canvas = np.zeros((ph, pw, 3), dtype=np.uint8)
        canvas[top:top + ch, left:left + cw] = frame[y0:y0 + ch, x0:x0 + cw]
        assert np.array_equal(dev[i], resize_ref(canvas, (192, 256))), f'crop {i} differs from the C oracle'
    shp, sd, _ = weights('s', 'coco')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)   # 7 crops -> chunks of 4 + 3
    a = eng.infer_frame(frame, p)
    b = eng.infer(host, p[:, 6:8])
    assert np.array_equal(a, b)
    eng.close()


def test_fused_layernorm_matches_standalone_layernorm(monkeypatch):
    """LayerNorm folded into the qkv / fc1 GEMMs (default) vs the standalone LayerNorm kernel: same network,
    different rounding points -- both must sit within the fp16 error budget of the oracle, and close to each other.
    Also exercises rows with a large common-mode offset (the fold rounds x BEFORE the mean is removed)."""
    shp, sd, sdt = weights('s', 'coco')
    crops = synthetic_crops(4, 9, 'noise')
    ref = oracle_heatmaps('s', 'coco', crops)
    out = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('VP_FUSE_LN', flag)
        eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)
        out[flag] = eng.heatmaps(crops)
        assert np.array_equal(out[flag], eng.heatmaps(crops))          # deterministic (no atomics in the statistics)
        eng.close()
    for flag, hm in out.items():
        e = np.abs(hm - ref)
        print(f'fuse_ln={flag}: max|err| {e.max():.3e} rms {np.sqrt((e ** 2).mean()):.3e}')
        assert e.max() < HM_MAX_ERR['fp16'] and np.sqrt((e ** 2).mean()) < HM_RMS_ERR['fp16']
    assert np.abs(out['1'] - out['0']).max() < 2e-3
    # common-mode stress: shift the positional embedding so every token row has mean ~ 3 x its std
    sd2 = dict(sd)
    sd2['backbone.pos_embed'] = sd['backbone.pos_embed'] + np.float32(2.0)
    import torch
    sdt2 = O.to_torch_state_dict(sd2)
    x = np.concatenate([O.pre_img(c)[0] for c in crops])
    ref2 = O.model_forward(sdt2, x, shp.depth, shp.num_heads)
    for flag in ('1', '0'):
        monkeypatch.setenv('VP_FUSE_LN', flag)
        eng = VitPoseHip(shp, sd2, dtype='fp16', max_batch=4)
        e = np.abs(eng.heatmaps(crops) - ref2)
        print(f'common-mode offset, fuse_ln={flag}: max|err| {e.max():.3e} rms {np.sqrt((e ** 2).mean()):.3e}')
        assert e.max() < 3 * HM_MAX_ERR['fp16']
        eng.close()


@pytest.mark.parametrize('shift', [False, True])
def test_flip_test_matches_oracle(shift):
    """Flip-test path (f-3): heatmaps of the crops and of their mirror images, flipped back (oracle pinned to the
    reference's flip_back golden), averaged, decoded -- against the oracle doing the same with the fp32 model."""
    from cases import coco_flip_pairs
    shp, sd, sdt = weights('s', 'coco')
    crops = synthetic_crops(3, 13, 'blobs')
    x = np.concatenate([O.pre_img(c)[0] for c in crops])
    ref_hm = O.flip_test_heatmaps(sdt, x, shp.depth, shp.num_heads, coco_flip_pairs(), shift_heatmap=shift)
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=2)            # 3 crops -> chunks of 2 + 1
    kp, hm = eng.infer_flip(crops, coco_flip_pairs(), shift_heatmap=shift, return_heatmaps=True)
    err = np.abs(hm - ref_hm)
    print(f'flip test (shift={shift}): heatmap max|err| {err.max():.3e} rms {np.sqrt((err ** 2).mean()):.3e}')
    assert err.max() < HM_MAX_ERR['fp16'] and np.sqrt((err ** 2).mean()) < HM_RMS_ERR['fp16']
    assert np.array_equal(kp, decode_heatmaps(hm))                   # the decode runs on the averaged maps
    assert np.abs(kp[..., 2] - O.decode_per_crop(ref_hm)[..., 2]).max() < CONF_TOL
    # a mirror-symmetric check that needs no oracle: flipping the input AND swapping the pairs reproduces the same average
    kp2, hm2 = eng.infer_flip(np.ascontiguousarray(crops[:, :, ::-1]), coco_flip_pairs(), return_heatmaps=True)
    if not shift:
        assert np.abs(O.flip_back(hm2, coco_flip_pairs()) - hm).max() < 2e-3
    eng.close()


def test_plain_c_caller_runs(tmp_path):
    """examples/c_api_demo.c (gcc, C99, nothing but the header) drives create / load_weights / infer / destroy."""
    import subprocess
    from test_host_logic import _build_c_demo
    exe = _build_c_demo(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = [l for l in res.stdout.splitlines() if l.startswith('crop 0 joint')]
    assert len(lines) == 3 and all('conf' in l for l in lines)
