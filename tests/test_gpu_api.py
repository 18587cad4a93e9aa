"""GPU: the host-facing entries added in round 2 -- stream-ordered device entry, asynchronous host path on pinned buffers,
hipGraph replay of small batches, the one-process multi-GPU group, ShardedPose over RCCL with the real engine."""
import os

import numpy as np
import pytest

from easy_vitpose_amd import PinnedArray, VitPoseGroup, VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd.synth import synthetic_crops
from helpers import weights

pytestmark = pytest.mark.gpu


def test_infer_device_is_ordered_after_torch_producers():
    """vp_infer_device ran on the library's stream with nothing ordering it after torch's stream.  The crops are
    produced by an asynchronous torch op chain (pinned H2D + arithmetic) right before the call; the result must equal the
    host-path result, and a torch consumer enqueued right after must see the finished keypoints -- no host synchronisation."""
    import torch
    shp, sd, _ = weights('s', 'coco')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
    crops = synthetic_crops(8, 3, 'blobs')
    ref = eng.infer(crops)
    dev = torch.device('cuda', 0)
    side = torch.cuda.Stream(device=dev)
    pinned = torch.from_numpy(crops).pin_memory()
    for _ in range(5):
        with torch.cuda.stream(side):
            junk = torch.empty(64 << 20, dtype=torch.uint8, device=dev).random_()      # keeps the side stream busy first
            d = pinned.to(dev, non_blocking=True)
            d = (d.to(torch.int16) + junk[:1].to(torch.int16) * 0).to(torch.uint8)     # produced late on the side stream
            out = torch.full((8, 17, 3), float('nan'), device=dev)
            eng.infer_device(d, out, sync=False)                                        # ordered after the producers ...
            summed = out.sum()                                                          # ... and before this consumer
        side.synchronize()
        assert torch.isfinite(summed).item()
        assert np.array_equal(out.cpu().numpy(), ref)
    eng.close()


def test_small_batch_ordered_entry_runs_on_the_callers_stream(monkeypatch):
    """Round 5: at <= 16 crops vp_infer_device_stream enqueues the chunk (eager launches on torch's legacy default stream, the hipGraph on any other stream) on the
    CALLER's stream instead of fencing its own stream against it with two events per call.  The handle's workspaces are then shared between streams over time: calls
    alternate between torch's default stream, a side stream, the handle's own stream (un-ordered device entry) and the host entry with nothing but the library's own
    ordering between them -- every result must be the host-path result, consumers enqueued right behind a call must see finished keypoints, and VP_CALLER_STREAM=0
    (the event-fenced path of rounds 2-4) must give the same bits."""
    import torch
    shp, sd, _ = weights('s', 'coco')
    crops = synthetic_crops(4, 5, 'blobs')
    dev = torch.device('cuda', 0)
    for mode in ('1', '0'):
        monkeypatch.setenv('VP_CALLER_STREAM', mode)
        eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
        ref = eng.infer(crops)
        side = torch.cuda.Stream(device=dev)
        d = torch.from_numpy(crops).to(dev)
        torch.cuda.synchronize()
        for it in range(4):
            o0 = torch.full((4, 17, 3), float('nan'), device=dev)
            eng.infer_device(d, o0, sync=False)                          # torch's default stream
            s0 = o0.sum()
            with torch.cuda.stream(side):
                side.wait_stream(torch.cuda.current_stream(dev))
                o1 = torch.full((4, 17, 3), float('nan'), device=dev)
                eng.infer_device(d, o1, sync=False)                      # a side stream: ordered behind the default-stream call by the library alone
                s1 = o1.sum()
            o2 = torch.full((4, 17, 3), float('nan'), device=dev)
            torch.cuda.current_stream(dev).synchronize()                 # o2's fill is done (the un-ordered entry's contract); the side stream's call may still be running
            eng.infer_device(d, o2, sync=True, ordered=False)            # the handle's own stream, right behind the side-stream call on the same workspaces
            host = eng.infer(crops)                                      # host entry
            side.synchronize()
            torch.cuda.synchronize()
            assert torch.isfinite(s0).item() and torch.isfinite(s1).item(), (mode, it)
            for name, o in (('default stream', o0), ('side stream', o1), ('own stream', o2)):
                assert np.array_equal(o.cpu().numpy(), ref), (mode, it, name)
            assert np.array_equal(host, ref), (mode, it)
        o3 = torch.full((4, 17, 3), float('nan'), device=dev)
        with torch.cuda.stream(side):
            eng.infer_device(d, o3, sync=False)
        eng.synchronize()                                                # vp_synchronize covers work left on a caller's stream
        assert np.array_equal(o3.cpu().numpy(), ref), mode
        eng.close()


def test_async_host_path_matches_sync_path():
    shp, sd, _ = weights('s', 'coco')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=16)
    batches = [synthetic_crops(16, 40 + i, 'noise') for i in range(5)]
    ref = [eng.infer(b) for b in batches]
    pin_in = [PinnedArray((16, 256, 192, 3), np.uint8) for _ in range(2)]
    pin_out = [PinnedArray((16, 17, 3), np.float32) for _ in range(2)]
    got, pending = [], []
    for i, b in enumerate(batches):                    # double-buffered: submit i+1 before waiting for i
        k = i & 1
        if len(pending) == 2:
            s, kk = pending.pop(0)
            eng.wait(s)
            got.append(pin_out[kk].array.copy())
        pin_in[k].array[...] = b
        pending.append((eng.submit(pin_in[k].array, pin_out[k].array), k))
    for s, kk in pending:
        eng.wait(s)
        got.append(pin_out[kk].array.copy())
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    with pytest.raises(Exception):                     # a third submission without a wait is refused, not queued silently
        s0 = eng.submit(pin_in[0].array, pin_out[0].array)
        s1 = eng.submit(pin_in[1].array, pin_out[1].array)
        try:
            eng.submit(pin_in[0].array, pin_out[0].array)
        finally:
            eng.wait(s0); eng.wait(s1)
    eng.close()


def test_small_batch_graph_replay_is_bit_identical(monkeypatch):
    """Batches of <= 16 crops are captured into a hipGraph on their second appearance and replayed afterwards."""
    shp, sd, _ = weights('s', 'coco')
    crops = synthetic_crops(8, 5, 'blobs')
    monkeypatch.setenv('VP_GRAPH', '0')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
    ref = eng.infer(crops)
    eng.close()
    monkeypatch.setenv('VP_GRAPH', '1')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
    outs = [eng.infer(crops) for _ in range(4)]        # eager, capture + launch, replay, replay
    other = synthetic_crops(8, 6, 'blobs')
    o2 = eng.infer(other)                              # same graph, new input bytes in the same staging buffer
    outs.append(eng.infer(crops))
    eng.close()
    for o in outs:
        assert np.array_equal(o, ref)
    assert not np.array_equal(o2, ref)


@pytest.mark.parametrize('variant,dataset,dtype,n', [('b', 'coco', 'bf16', 9), ('s', 'coco', 'bf16', 9), ('b', 'coco', 'fp16', 9), ('l', 'coco_25', 'fp16', 12), ('s', 'coco', 'bf16', 30), ('h', 'wholebody', 'fp16', 10)])
def test_small_batches_are_run_to_run_identical(variant, dataset, dtype, n):
    """A fresh handle, four forwards of the same crops: heatmaps bit for bit.  Round 6 (profiles/small_batch_r6.txt call 28): a gemm.hip whose epilogue had one more wave-uniform
    branch + barrier in front of the LDS staging lost this on the BF16 64 x 64 2-stage qkv kernel (ViTPose-B / -S at 9 crops) -- on the plain path, with several workgroups per
    CU -- while every fp16 build stayed stable; the layout test caught it by accident, this one is there on purpose (eager launches and hipGraph replay, both dtypes, the tile
    families of 9-30 crops)."""
    shp, sd, _ = weights(variant, dataset)
    crops = synthetic_crops(n, 19, 'blobs')
    crops[1::2] = synthetic_crops(len(crops[1::2]), 20, 'noise')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    hms = [eng.heatmaps(crops) for _ in range(4)]
    kps = [eng.infer(crops) for _ in range(4)]          # <= 16 crops: eager, capture, replay, replay
    eng.close()
    assert all(np.array_equal(hms[0], h) for h in hms[1:]), [int((hms[0] != h).sum()) for h in hms[1:]]
    assert all(np.array_equal(kps[0], k) for k in kps[1:])
    assert np.isfinite(hms[0]).all()


@pytest.mark.parametrize('variant,dataset,dtype,n', [('b', 'coco', 'fp16', 44), ('l', 'coco_25', 'fp16', 5), ('b', 'coco', 'bf16', 9)])
def test_blocked_qkv_layout_is_bit_identical(monkeypatch, variant, dataset, dtype, n):
    """Head dim 64: the qkv GEMM writes its output in the 64 x 64-blocked layout and the attention kernel reads a (crop, head)'s q / k / v as three
    contiguous 8 KiB blocks (VP_BLOCKED_QKV, default on).  Only addresses change: heatmaps and keypoints agree bit for bit with the row-major layout."""
    monkeypatch.setenv('VP_FUSE_QKV_ATTN', '0')   # the fused qkv + attention kernel never materialises qkv: this test is about the layout of that tensor
    shp, sd, _ = weights(variant, dataset)
    crops = synthetic_crops(n, 17, 'blobs')
    monkeypatch.setenv('VP_BLOCKED_QKV', '0')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    ref_kp, ref_hm = eng.infer(crops), eng.heatmaps(crops)
    eng.close()
    monkeypatch.delenv('VP_BLOCKED_QKV')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    kp, hm = eng.infer(crops), eng.heatmaps(crops)
    eng.close()
    assert np.array_equal(hm, ref_hm)
    assert np.array_equal(kp, ref_kp)
    assert np.isfinite(hm).all() and float(np.abs(hm).max()) > 0


@pytest.mark.parametrize('variant,dataset,dtype,n', [('s', 'coco', 'fp16', 8), ('b', 'coco', 'fp16', 16), ('l', 'coco_25', 'fp16', 3), ('b', 'coco', 'bf16', 1)])
def test_small_batch_statistics_fold_is_bit_identical(monkeypatch, variant, dataset, dtype, n):
    """Batches of <= 8 crops (default threshold; VP_FOLD_STATS=n moves it): qkv / fc1 merge the LayerNorm partial statistics of their
    tile rows themselves (gemm.hip prologue, GemmArgs::ln_part) instead of 2 x depth ln_finalize launches.  Same ln_merge, so heatmaps
    and keypoints agree bit for bit with the ln_finalize path (VP_FOLD_STATS=0), and the launches really disappear."""
    shp, sd, _ = weights(variant, dataset)
    crops = synthetic_crops(n, 33, 'blobs')
    monkeypatch.setenv('VP_GRAPH', '0')
    monkeypatch.setenv('VP_FOLD_STATS', '0')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    eng.set_profiling(True)
    ref_kp, ref_hm = eng.infer(crops), eng.heatmaps(crops)
    ref_launches = eng.profile()['layernorm']['launches']
    eng.close()
    if n <= 8:
        monkeypatch.delenv('VP_FOLD_STATS')          # the default threshold covers it
    else:
        monkeypatch.setenv('VP_FOLD_STATS', '64')    # measured slower than ln_finalize from 16 crops on: off by default, same bits
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    eng.set_profiling(True)
    kp, hm = eng.infer(crops), eng.heatmaps(crops)
    launches = eng.profile()['layernorm']['launches']
    eng.close()
    assert np.array_equal(hm, ref_hm)
    assert np.array_equal(kp, ref_kp)
    assert np.isfinite(hm).all() and float(np.abs(hm).max()) > 0
    assert ref_launches == 2 * (2 * shp.depth + 1) and launches == 2, (ref_launches, launches)   # only last_norm is left (two forward passes)


@pytest.mark.parametrize('variant,dataset,n,folded', [('s', 'coco', 12, 'both'), ('s', 'coco', 28, 'both'), ('b', 'coco', 12, 'both'), ('b', 'coco', 16, 'ln1'), ('l', 'coco_25', 12, 'ln1'),
                                                       ('h', 'wholebody', 10, 'ln1'), ('b', 'coco', 18, 'ln1'), ('l', 'coco_25', 14, 'ln1'), ('b', 'coco', 20, 'none')])
def test_statistics_fold_rule_beyond_8_crops(monkeypatch, variant, dataset, n, folded):
    """Round 6: beyond 8 crops the consumers' statistics merge is chosen PER CONSUMER (forward.hip forward_chunk): attn.qkv (LayerNorm-1) / mlp.fc1 (LayerNorm-2) fold where
    their GEMM runs on a 2-phase tile that keeps its occupancy with the (mean, rstd) area behind its ring -- not the 80 KiB ring of the default 192 x 128 tile (one workgroup
    per CU instead of two), not the 8-phase kernel, not a fused qkv + attention kernel.  Same ln_merge: heatmaps and keypoints equal the ln_finalize path (VP_FOLD_STATS=0)
    bit for bit, and exactly the expected ln_finalize launches disappear.  At 108-127 (pair, head) tiles (ViTPose-B 17-18 crops, -L 13-14) the two-launch qkv + attention path
    keeps attn.qkv because its tile folds; at 19-20 crops of ViTPose-B (default tile: no fold) the fused kernel takes it."""
    shp, sd, _ = weights(variant, dataset)
    crops = synthetic_crops(n, 35, 'blobs')
    crops[1::2] = synthetic_crops(len(crops[1::2]), 36, 'noise')
    monkeypatch.setenv('VP_GRAPH', '0')
    monkeypatch.setenv('VP_FOLD_STATS', '0')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
    eng.set_profiling(True)
    ref_kp, ref_hm = eng.infer(crops), eng.heatmaps(crops)
    ref_launches = eng.profile()['layernorm']['launches']
    eng.close()
    monkeypatch.delenv('VP_FOLD_STATS')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
    eng.set_profiling(True)
    kp, hm = eng.infer(crops), eng.heatmaps(crops)
    launches = eng.profile()['layernorm']['launches']
    kernels = {f: eng.profile_kernel(f) for f in ('gemm_qkv', 'gemm_fc1')}
    eng.close()
    L = shp.depth
    expect = {'both': 2, 'ln1': 2 * (L + 1), 'none': 2 * (2 * L + 1)}[folded]   # two forward passes; last_norm always launches
    print(f'[fold rule] {variant} x {n}: layernorm-family launches {ref_launches} -> {launches} ({folded}); {kernels}')
    assert ref_launches == 2 * (2 * L + 1) and launches == expect, (ref_launches, launches, kernels)
    assert ('qkvattn' in kernels['gemm_qkv']) == (folded == 'none'), kernels
    assert np.array_equal(hm, ref_hm) and np.array_equal(kp, ref_kp)


@pytest.mark.parametrize('variant,dataset,dtype,n', [('s', 'coco', 'fp16', 64), ('s', 'wholebody', 'fp16', 48), ('b', 'coco_25', 'bf16', 44)])
def test_fused_head_is_bit_identical(monkeypatch, variant, dataset, dtype, n):
    """Batches of >= 43 crops run deconv2 + final 1x1 conv as ONE kernel (gemm.hip EPI_DECONV_FINAL: the 256-channel activations
    stay in LDS).  Same arithmetic, same accumulation order as the two launches: heatmaps and keypoints must agree bit for bit
    (K = 17, 25 and 133: one, two and nine 16-joint weight groups; topdown_heatmap_simple_head.py:188-193)."""
    shp, sd, _ = weights(variant, dataset)
    crops = synthetic_crops(n, 21, 'blobs')
    monkeypatch.setenv('VP_FUSE_HEAD', '0')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    ref_kp, ref_hm = eng.infer(crops), eng.heatmaps(crops)
    eng.close()
    monkeypatch.setenv('VP_FUSE_HEAD', '1')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    eng.set_profiling(True)
    kp, hm = eng.infer(crops), eng.heatmaps(crops)
    prof = eng.profile()
    eng.close()
    assert prof['gemm_final']['launches'] == 0 and prof['gemm_deconv']['launches'] == 4, 'the fused kernel did not run'
    assert np.array_equal(hm, ref_hm)
    assert np.array_equal(kp, ref_kp)
    assert np.isfinite(hm).all() and float(np.abs(hm).max()) > 0


@pytest.mark.parametrize('n', [36, 96])
def test_mid_batch_gemm8_selection_is_bit_identical(monkeypatch, n):
    """Between ~32 and ~128 crops the 8-phase kernel takes a GEMM when its tiles fill the last round of 256 persistent workgroups
    (forward.hip gemm()): 36 crops -> qkv on 243 tiles over 240 workgroups (uneven XCD shares, some workgroups take two tiles),
    96 crops -> fc2 on 216 tiles of 256 x 256 with the residual epilogue.  Same arithmetic order as the 2-phase kernels: the whole
    path must not change by a bit against VP_GEMM8=0."""
    shp, sd, _ = weights('b', 'coco')
    crops = synthetic_crops(n, 41, 'blobs')
    fams = ('gemm_qkv', 'gemm_fc1', 'gemm_fc2')
    monkeypatch.setenv('VP_FUSE_QKV_ATTN', '0')   # keep attn.qkv a GEMM of its own here (the fused qkv + attention kernel has its own test)
    monkeypatch.setenv('VP_GEMM8', '0')           # a PRODUCT-side switch (vp_create): every GEMM on the 2-phase kernels
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
    ref_kp, ref_tok = eng.infer(crops), eng.tokens(crops)
    ref_kernels = {f: eng.profile_kernel(f) for f in fams}
    eng.close()
    monkeypatch.delenv('VP_GEMM8')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
    kp, tok = eng.infer(crops), eng.tokens(crops)
    kernels = {f: eng.profile_kernel(f) for f in fams}
    eng.close()
    # the two engines really ran different kernels (with the switch compiled out of the product build this test passed vacuously)
    assert all('gemm8_kernel' not in k and k for k in ref_kernels.values()), ref_kernels
    assert any('gemm8_kernel' in k for k in kernels.values()), kernels
    print(f'[{n} crops] VP_GEMM8=0: {ref_kernels}; default: {kernels}')
    assert np.array_equal(tok, ref_tok)
    assert np.array_equal(kp, ref_kp)


@pytest.mark.parametrize('variant,dataset,dtype,n', [('b', 'coco', 'fp16', 96), ('l', 'coco_25', 'fp16', 64), ('b', 'coco', 'bf16', 128), ('b', 'coco', 'fp16', 256),
                                                     ('l', 'coco_25', 'fp16', 16), ('b', 'coco', 'fp16', 23)])   # 16: replayed from a hipGraph; 23: odd, 144 tiles
def test_fused_qkv_attention_is_bit_identical(monkeypatch, variant, dataset, dtype, n):
    """attn.qkv + the attention core in one kernel per (pair of crops, head) (qkvattn.hip: 384 x 192 tiles on the 8-phase schedule, q / k / v handed
    to the attention core through LDS, the [M, 3D] tensor never in HBM) against the two-launch path (VP_FUSE_QKV_ATTN=0): same accumulation order,
    same LayerNorm fold, same roundings, same attention arithmetic -> backbone tokens and keypoints must not differ by a bit; repeated, because a
    ring / barrier race would show up as run-to-run differences."""
    shp, sd, _ = weights(variant, dataset)
    crops = synthetic_crops(n, 51, 'blobs')
    crops[n // 2:] = synthetic_crops(n - n // 2, 52, 'noise')
    monkeypatch.setenv('VP_FUSE_QKV_ATTN', '0')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    ref_kp, ref_tok = eng.infer(crops), eng.tokens(crops)
    ref_kernel = eng.profile_kernel('gemm_qkv')
    eng.close()
    monkeypatch.delenv('VP_FUSE_QKV_ATTN')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    runs = [(eng.infer(crops), eng.tokens(crops)) for _ in range(3)]
    kernel = eng.profile_kernel('gemm_qkv')
    odd = eng.infer(crops[:n - 1])                      # an odd batch: the last crop fills both halves of its pair
    odd_kernel = eng.profile_kernel('gemm_qkv')
    eng.close()
    assert 'qkvattn_kernel' in odd_kernel
    print(f'[{variant}/{dtype} @ {n}] qkv family: {ref_kernel!r} vs {kernel!r}')
    assert 'qkvattn_kernel' in kernel and 'qkvattn_kernel' not in ref_kernel
    for kp, tok in runs:
        assert np.array_equal(tok, ref_tok), f'{(tok != ref_tok).any(axis=(1, 2)).sum()} of {n} crops differ in the backbone output'
        assert np.array_equal(kp, ref_kp)
    assert np.array_equal(odd, ref_kp[:n - 1])


@pytest.mark.parametrize('dtype,n', [('fp16', 32), ('fp16', 17), ('fp16', 13), ('bf16', 16)])   # 13 crops: 208 tiles = 208 workgroups, a grid that is no multiple of 8
def test_fused_qkv_attention_head_dim_80_is_bit_identical(monkeypatch, dtype, n):
    """ViTPose-H (head dim 80, BASELINE configs[2]'s model): attn.qkv + the attention core as ONE kernel per (crop, head) -- gemm8.hip's 192 x 256 tile with
    EPI_QKV_ATTN: [q_h | k_h | v_h | 16 zero rows] head-major weights, q / k / v handed over through LDS, 12 query tiles on 8 waves -- against the two-launch
    path (VP_FUSE_QKV_ATTN=0): keypoints and backbone tokens bit for bit, three runs (a ring / barrier race would show as run-to-run differences); 17 crops =
    272 tiles = one round + 16."""
    shp, sd, _ = weights('h', 'wholebody')
    crops = synthetic_crops(n, 53, 'blobs')
    crops[n // 2:] = synthetic_crops(n - n // 2, 54, 'noise')
    monkeypatch.setenv('VP_FUSE_QKV_ATTN', '0')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    ref_kp, ref_tok = eng.infer(crops), eng.tokens(crops)
    ref_kernel = eng.profile_kernel('gemm_qkv')
    eng.close()
    monkeypatch.delenv('VP_FUSE_QKV_ATTN')
    eng = VitPoseHip(shp, sd, dtype=dtype, max_batch=n)
    runs = [(eng.infer(crops), eng.tokens(crops)) for _ in range(3)]
    kernel = eng.profile_kernel('gemm_qkv')
    eng.close()
    print(f'[h/{dtype} @ {n}] qkv family: {ref_kernel!r} vs {kernel!r}')
    assert ', 9, G8<256, 192>' in kernel and ', 9, ' not in ref_kernel
    for kp, tok in runs:
        assert np.array_equal(tok, ref_tok), f'{(tok != ref_tok).any(axis=(1, 2)).sum()} of {n} crops differ in the backbone output'
        assert np.array_equal(kp, ref_kp)


@pytest.mark.parametrize('variant,dataset,n,fc2', [('b', 'coco', 85, 'G8<256, 192>'), ('l', 'coco_25', 63, 'G8<256, 192>'), ('b', 'coco', 26, None),
                                                     ('b', 'coco', 88, 'G8<256, 256>')])
def test_192_row_tiles_and_odd_tile_counts_are_bit_identical(monkeypatch, variant, dataset, n, fc2):
    """Batches whose row count no 256-row tile divides (three of four batch sizes): fc1 / fc2 on the 8-phase kernel's 192 x 256 tile (VP_G8_BM192, a
    product-side switch) and launches of a tile count that is no multiple of 8 (one workgroup per tile: 255 / 252 fc2 tiles, 156 fused
    qkv + attention tiles at 26 crops; at 88 crops fc2 as ONE round of 198 tiles of 256 x 256, a pick of the round-4 selection rule, VP_G8_COST) against the
    kernels the round-3 rule picks: keypoints and backbone tokens bit for bit, three runs."""
    shp, sd, _ = weights(variant, dataset)
    crops = synthetic_crops(n, 61, 'blobs')
    crops[n // 2:] = synthetic_crops(n - n // 2, 62, 'noise')
    monkeypatch.setenv('VP_G8_BM192', '0')
    monkeypatch.setenv('VP_G8_COST', '0')
    monkeypatch.setenv('VP_FUSE_QKV_ATTN', '0')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
    ref_kp, ref_tok = eng.infer(crops), eng.tokens(crops)
    ref_k = {f: eng.profile_kernel(f) for f in ('gemm_qkv', 'gemm_fc1', 'gemm_fc2')}
    eng.close()
    monkeypatch.delenv('VP_G8_BM192')
    monkeypatch.delenv('VP_G8_COST')
    monkeypatch.delenv('VP_FUSE_QKV_ATTN')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
    runs = [(eng.infer(crops), eng.tokens(crops)) for _ in range(3)]
    k = {f: eng.profile_kernel(f) for f in ('gemm_qkv', 'gemm_fc1', 'gemm_fc2')}
    eng.close()
    print(f'[{variant} @ {n}] {ref_k} -> {k}')
    assert 'qkvattn_kernel' in k['gemm_qkv'] and 'qkvattn_kernel' not in ref_k['gemm_qkv']
    if fc2:
        assert fc2 in k['gemm_fc2'] and fc2 not in ref_k['gemm_fc2'], (k, ref_k)
    for kp, tok in runs:
        assert np.array_equal(tok, ref_tok), f'{(tok != ref_tok).any(axis=(1, 2)).sum()} of {n} crops differ in the backbone output'
        assert np.array_equal(kp, ref_kp)


def _tile_choice_batches(D, lo=17, hi=260):
    """One batch size per distinct (fc1 tile, fc2 tile, rounds class, tile count a multiple of 8 or not) signature of the selection rule."""
    import ctypes as C
    lib = capi.load_library()
    t = C.c_int32()
    seen, out = set(), []
    for n in range(lo, hi + 1):
        sig = []
        for N, wide in ((4 * D, 1), (D, 0)):
            v = lib.vp_dbg_gemm8_pick(192 * n, N, wide, 3, C.byref(t))
            sig.append((v, min(-(-t.value // 256), 3) if v else 0, (t.value % 8 != 0) if v else False))
        sig = tuple(sig)
        if sig not in seen:
            seen.add(sig)
            out.append(n)
    return out


def test_every_tile_choice_of_the_selection_rule_is_bit_identical():
    """The selection rule picks different kernels from batch size to batch size (2-phase, 256 x 256, 256 x 192, 192 x 256; one, two, many rounds; tile
    counts that are no multiple of 8).  One batch size per distinct signature of the rule (ViTPose-B, 17..260 crops): every crop of the batch must
    equal the max_batch = 8 path (64 x 64 / 128 x 128 tiles, consumer-merged statistics) bit for bit, and the kernels must be the ones the rule names."""
    shp, sd, _ = weights('b', 'coco')
    batches = _tile_choice_batches(shp.embed_dim)
    assert len(batches) >= 12, batches
    crops = synthetic_crops(max(batches), 71, 'blobs')
    crops[1::2] = synthetic_crops(len(crops[1::2]), 72, 'noise')
    small = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
    ref = small.infer(crops)
    small.close()
    names = {0: 'TileCfg', 16: 'G8<256, 256>', 17: 'G8<192, 256>', 18: 'G8<256, 192>'}
    import ctypes as C
    lib, t = capi.load_library(), C.c_int32()
    seen = set()
    for n in batches:
        eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
        out = eng.infer(crops[:n])
        k1, k2 = eng.profile_kernel('gemm_fc1'), eng.profile_kernel('gemm_fc2')
        eng.close()
        nr = lib.vp_dbg_run_batch(n, shp.embed_dim, (n + 3) // 4 * 4)   # round 6: the encoder may run the next multiple of 4 crops (tile_rules.hip pick_run_batch)
        v1 = lib.vp_dbg_gemm8_pick(192 * nr, 4 * shp.embed_dim, 1, 3, C.byref(t))
        v2 = lib.vp_dbg_gemm8_pick(192 * nr, shp.embed_dim, 0, 3, C.byref(t))
        assert names[v1] in k1 and names[v2] in k2, (n, v1, k1, v2, k2)
        seen.add((v1, v2))
        assert np.array_equal(out, ref[:n]), f'batch {n} ({k1} / {k2}): {(out != ref[:n]).any(axis=(1, 2)).sum()} crops differ from the max_batch = 8 path'
    print(f'[tile choices] batches {batches}: (fc1, fc2) variants seen {sorted(seen)}')
    assert {v for p in seen for v in p} >= {0, 16, 17, 18}


_C31, _C30, _C12, _C15 = '<32, 64, 64, 16, 32, 6, 6', '<64, 64, 64, 32, 32, 6, 6', '<64, 64, 64, 32, 32, 4, 0', '<128, 64, 64, 64, 32, 3, 0'
_C41, _C20, _C3, _C8 = '<96, 64, 64, 48, 32, 4, 0', '<192, 128, 64, 48, 64, 3, 1', '<256, 256, 64, 128, 64, 2, 1', '<192, 128, 64, 96, 64, 2, 1'


@pytest.mark.usefixtures('one_launch_family')
@pytest.mark.parametrize('variant,dataset,cases', [
    ('b', 'coco', [(1, _C31, _C31, None), (4, _C30, _C30, None), (12, _C12, _C12, None), (15, _C41, _C41, _C8), (16, _C41, _C41, None), (20, _C15, _C15, None),
                   (22, _C15, _C15, _C3), (32, _C20, _C20, None), (113, _C3, _C3, None)]),   # 113: no multiple of 4 the padding rule (pick_run_batch) rounds up
    ('l', 'coco_25', [(2, _C31, _C31, None), (12, _C41, _C41, None), (16, _C15, _C15, None), (17, _C15, _C15, _C3), (24, _C20, _C20, None)]),
    ('s', 'coco', [(3, _C31, _C31, None)]),
])
def test_small_batch_tile_rule_is_bit_identical(variant, dataset, cases):
    """Round 5: below the 8-phase regime the residual GEMMs run on 32 x 64 / 64 x 64 tiles with TWO k-blocks per barrier (<= 256 tiles), on the 4-stage 64 x 64 ring
    (<= 512 tiles) or on the 3-stage 128 x 64 tile -- tile_rules.hip pick_gemm2_tile.  Round 6: 96 x 64 tiles between the two (<= 448 tiles), one round of 8-wave
    192 x 128 tiles beyond 512 tiles of 128 x 64; mlp.fc1 -- and, at 113 crops of ViTPose-B, the residual GEMMs -- on one round of 256 x 256 tiles (ragged last m-tile) / on the
    default tile where the 128 x 128 tiles would overflow the resident slots.  Same k order: every crop must equal the max_batch = 8 path bit for bit (whose own GEMMs are 128 x 128 / 4-stage 64 x 64 tiles),
    and the kernels must be the ones the rule names."""
    shp, sd, _ = weights(variant, dataset)
    nmax = max(c[0] for c in cases)
    crops = synthetic_crops(nmax, 91, 'blobs')
    crops[1::2] = synthetic_crops(len(crops[1::2]), 92, 'noise')
    small = VitPoseHip(shp, sd, dtype='fp16', max_batch=8)
    ref = small.infer(crops) if nmax > 8 else small.infer(np.concatenate([crops, synthetic_crops(8 - nmax, 93, 'noise')]))[:nmax]
    small.close()
    for n, proj, fc2, fc1 in cases:
        eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
        out = eng.infer(crops[:n])
        out2 = eng.infer(crops[:n])                      # second sighting of the chunk: the hipGraph replay (<= 16 crops)
        kp, kf, k1 = eng.profile_kernel('gemm_proj'), eng.profile_kernel('gemm_fc2'), eng.profile_kernel('gemm_fc1')
        eng.close()
        assert proj in kp and fc2 in kf and (fc1 is None or fc1 in k1), (n, kp, kf, k1)
        assert np.array_equal(out, ref[:n]) and np.array_equal(out2, ref[:n]), f'{variant} batch {n} ({kp} / {kf}): {(out != ref[:n]).any(axis=(1, 2)).sum()} crops differ'


@pytest.mark.parametrize('variant,dataset,n,max_batch', [('b', 'coco', 43, 43), ('b', 'coco', 86, 86), ('l', 'coco_25', 65, 65), ('s', 'coco', 45, 48), ('b', 'coco', 90, 43)])
def test_padded_encoder_batch_is_bit_identical(variant, dataset, n, max_batch, monkeypatch):
    """Round 6: from 33 crops on the encoder runs the next multiple of 4 crops where that buys mlp.fc1 / mlp.fc2 an 8-phase tile (tile_rules.hip pick_run_batch; the padding
    rows repeat the last crop, the head and the decode run the real crops).  Keypoints AND heatmaps of the real crops must equal the unpadded run (VP_PAD_BATCH=0) bit for bit --
    also when the handle's max_batch is the odd size itself (workspaces rounded up in vp_create) and when a call is split into chunks (90 crops on max_batch 43: 43 + 43 + 4);
    and the padded run must really have taken the 8-phase kernel."""
    shp, sd, _ = weights(variant, dataset)
    crops = synthetic_crops(n, 83, 'blobs')
    crops[1::2] = synthetic_crops(len(crops[1::2]), 84, 'noise')
    monkeypatch.setenv('VP_PAD_BATCH', '0')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=max_batch)
    ref_kp = eng.infer(crops)
    ref_hm = eng.heatmaps(crops[:min(n, max_batch)])
    k_ref = eng.profile_kernel('gemm_fc1') + ' | ' + eng.profile_kernel('gemm_fc2')
    eng.close()
    monkeypatch.delenv('VP_PAD_BATCH')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=max_batch)
    kp = eng.infer(crops)
    kp2 = eng.infer(crops)                     # again: warm workspaces
    hm = eng.heatmaps(crops[:min(n, max_batch)])   # last forward = one full chunk: its kernels are the ones profile_kernel names
    k_pad = eng.profile_kernel('gemm_fc1') + ' | ' + eng.profile_kernel('gemm_fc2')
    eng.close()
    import ctypes as C
    run = capi.load_library().vp_dbg_run_batch(min(n, max_batch), shp.embed_dim, (max_batch + 3) // 4 * 4)
    print(f'[padded encoder batch] {variant} x {n} (max_batch {max_batch}): encoder runs {run} crops per full chunk; unpadded {k_ref}; padded {k_pad}')
    assert run > min(n, max_batch) and run % 4 == 0
    assert 'gemm8_kernel' in k_pad
    assert np.array_equal(kp, ref_kp) and np.array_equal(kp2, ref_kp), f'{(kp != ref_kp).any(axis=(1, 2)).sum()} crops differ'
    assert np.array_equal(hm, ref_hm)


def test_deconv_parity_order_is_bit_identical(monkeypatch):
    """VP_DECONV_PARITY_FAST (product-side switch): the four output parities of a deconv tile as consecutive logical blocks (same XCD: shared input
    rows) against parity-major launch order -- the same tiles, the same arithmetic: heatmaps bit for bit, fused and un-fused head."""
    shp, sd, _ = weights('b', 'coco')
    for n in (48, 16):                                  # 48: deconv2 + final conv fused; 16: three launches
        crops = synthetic_crops(n, 63, 'blobs')
        monkeypatch.setenv('VP_DECONV_PARITY_FAST', '0')
        eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
        ref_hm, ref_kp = eng.heatmaps(crops), eng.infer(crops)
        eng.close()
        monkeypatch.delenv('VP_DECONV_PARITY_FAST')
        eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=n)
        hm, kp = eng.heatmaps(crops), eng.infer(crops)
        eng.close()
        assert np.array_equal(hm, ref_hm) and np.array_equal(kp, ref_kp), f'n = {n}: {(hm != ref_hm).sum()} heatmap values differ'


def test_group_matches_single_handle():
    """vp_group_* with every visible device (1 on the test box): sharded result == unsharded result, bit for bit; the
    device-side all-gather leaves all keypoints on every member."""
    import torch
    ndev = torch.cuda.device_count()
    shp, sd, _ = weights('s', 'coco')
    crops = synthetic_crops(11, 9, 'blobs')
    one = VitPoseHip(shp, sd, dtype='fp16', max_batch=4)
    ref = one.infer(crops)
    one.close()
    grp = VitPoseGroup(shp, sd, list(range(ndev)), dtype='fp16', max_batch=4)     # 11 crops -> rounds of ndev x 4
    assert np.array_equal(grp.infer(crops), ref)
    d_all = [torch.zeros((11, 17, 3), device=f'cuda:{i}') for i in range(ndev)]
    out = grp.infer_allgather(crops, d_all)
    assert np.array_equal(out, ref)
    for t in d_all:
        assert np.array_equal(t.cpu().numpy(), ref)
    assert grp.infer(crops[:0]).shape == (0, 17, 3)
    grp.close()


def test_sharded_pose_over_rccl_with_the_real_engine():
    """ShardedPose (one process per GPU, all-gather over RCCL) with the real engine at the world size the box offers:
    the gathered result equals the unsharded one bit for bit (crops are independent)."""
    import torch
    import torch.distributed as dist
    from easy_vitpose_amd.parallel import ShardedPose
    shp, sd, _ = weights('s', 'coco')
    crops = synthetic_crops(10, 2, 'blobs')
    eng = VitPoseHip(shp, sd, dtype='fp16', max_batch=16)
    ref = eng.infer(crops)
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29533')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        sp = ShardedPose(eng.infer, shp.num_keypoints, device='cuda:0')
        got = sp.infer(crops).cpu().numpy()
        assert np.array_equal(got, ref)
        got = sp.infer(crops, pre_sharded=True, n_total=len(crops)).cpu().numpy()   # world 1: the shard is everything
        assert np.array_equal(got, ref)
    finally:
        dist.destroy_process_group()
        eng.close()


def test_video_mode_with_tracker_and_cli(tmp_path):
    """is_video=True: the built-in SORT tracker keeps ids across frames and predicts boxes on detector-skipped frames
    (yolo_step = 2), and the CLI writes the reference's --save-json wire format for a .npy frame stack."""
    import json
    from easy_vitpose_amd import VitInference, cli
    shp, sd, _ = weights('s', 'coco')
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, size=(6, 360, 480, 3), dtype=np.uint8)
    boxes = [[[40 + 5 * f, 60, 160 + 5 * f, 300, 0.9], [300 - 4 * f, 80, 400 - 4 * f, 320, 0.8]] for f in range(6)]
    calls = {'n': 0}

    def det(img):
        calls['n'] += 1
        return np.asarray(boxes[min(calls['n'] - 1, 5)], dtype=np.float64)

    model = VitInference(sd, det, model_name='s', dataset='coco', is_video=True, yolo_step=2, max_batch=4)
    seen = []
    for f in range(6):
        res = model.inference(frames[f])
        seen.append(sorted(res.keys()))
        assert all(v.shape == (17, 3) for v in res.values())
    # both people on EVERY frame with stable ids: on detector frames (matched tracks; min_hits = 1 for yolo_step > 1 as in the
    # reference, inference.py:179 -- with min_hits = 3 a re-matched coasting track would never be reported) and on skipped
    # frames (the tracker's predicted boxes)
    assert model.tracker.min_hits == 1 and model.tracker.max_age == 2
    assert all(s == [1, 2] for s in seen), seen
    assert calls['n'] < 6                                                # ... which it was (frame_counter % yolo_step)
    model.reset()
    assert model.frame_counter == 0 and model.tracker is not None
    np.save(tmp_path / 'clip.npy', frames)
    (tmp_path / 'boxes.json').write_text(json.dumps(boxes))
    rc = cli.main(['--input', str(tmp_path / 'clip.npy'), '--synthetic', 's', '--dataset', 'coco', '--boxes', str(tmp_path / 'boxes.json'),
                   '--output-path', str(tmp_path / 'out'), '--save-json', '--max-batch', '4'])
    assert rc == 0
    out = json.load(open(tmp_path / 'out' / 'clip.npy' / 'clip_result.json'))
    assert len(out['keypoints']) == 6 and out['skeleton']['0'] == 'nose'
    assert sorted(out['keypoints'][0].keys()) == ['1', '2'] and len(out['keypoints'][0]['1']) == 17 and len(out['keypoints'][0]['1'][0]) == 3

@pytest.mark.parametrize('variant,dataset', [('b', 'coco'), ('h', 'wholebody'), ('s', 'coco')])
def test_split_k_single_crop_calls_meet_the_tolerances_and_are_deterministic(golden_dir, variant, dataset, monkeypatch):
    """Round 6: calls of one or two crops (the reference's own per-person call, inference.py:259-272) run mlp.fc2 as four k ranges + the fixed-order reduction
    kernel (tile_rules.hip pick_splitk).  The accumulation order differs from the batched kernels, so these calls are no longer bit-identical to larger batches --
    what is asserted is what the north_star asks: every joint of the peaked golden within +-0.5 px / 1e-3 of the REFERENCE's keypoints, crop by crop and two at a
    time; run-to-run bit identity (no atomics anywhere); and the same against the one-launch path (VP_SPLITK=0), which must stay inside the same tolerances."""
    from cases import peaked_crops
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.synth import synthetic_state_dict
    z = np.load(os.path.join(golden_dir, f'peaked_{variant}_{dataset}.npz'))
    n = int(z['n'])
    shp = model_shape(variant, dataset)
    sd = synthetic_state_dict(shp, 0, peaked=True)
    crops, ref = peaked_crops(n), z['keypoints']
    got = {}
    for tag, env in (('split-K', None), ('one launch', '0')):
        if env is None:
            monkeypatch.delenv('VP_SPLITK', raising=False)
        else:
            monkeypatch.setenv('VP_SPLITK', env)
        eng = VitPoseHip(shp, sd, dtype='fp16', device_id=0, max_batch=2)
        one = np.concatenate([eng.infer(crops[i:i + 1]) for i in range(n)])
        one_again = np.concatenate([eng.infer(crops[i:i + 1]) for i in range(n)])
        kern = eng.profile_kernel('gemm_fc2')          # of the single-crop calls (ViTPose-S does not split two-crop calls)
        two = np.concatenate([eng.infer(crops[i:i + 2]) for i in range(0, n, 2)])
        eng.close()
        assert np.array_equal(one, one_again), f'{tag}: single-crop calls are not run-to-run deterministic'
        assert ('split-K' in kern) == (env is None), f'{tag}: mlp.fc2 ran on {kern}'
        for what, kp in (('1 crop per call', one), ('2 crops per call', two)):
            dpx = np.abs(kp[..., :2] - ref[..., :2]).max(-1)
            dcf = np.abs(kp[..., 2] - ref[..., 2])
            print(f'[{variant}/{dataset} {tag}, {what}] {dpx.size} joints: coordinate max err {dpx.max():.4f} px, confidence max err {dcf.max():.3e}; fc2 = {kern}')
            assert dpx.max() < 0.5 and dcf.max() < 1e-3, (tag, what)
        got[tag] = one
    d = np.abs(got['split-K'] - got['one launch'])      # (not a parity statement: a different fp32 accumulation order in mlp.fc2, through L blocks and the head)
    print(f'[{variant}/{dataset}] split-K against the one-launch path: coordinates differ by up to {d[..., :2].max():.4f} px, confidences by up to {d[..., 2].max():.3e}')
