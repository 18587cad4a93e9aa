/*
 * vitpose_hip.h -- C ABI of the MI355X-native ViTPose hot path (libvitpose_hip.so).
 *
 * Drop-in boundary: the reference's backend slot `VitInference._inference`
 * (easy_ViTPose/inference.py:207-219, assigned at :169-172, called at :268) whose
 * existing implementations are `_inference_torch` (:320-328) and `_inference_onnx`
 * (:330-337).  A backend takes one cropped+padded RGB crop, runs
 *     pre_img (:314-318) -> ViTPose.forward (vit_models/model.py:23-24)
 *             -> postprocess (:187-205)
 * and returns float32 [1, K, 3] = (y, x, conf) in crop pixels.  This library is
 * the batched form of exactly that call: N crops in, [N, K, 3] out.
 *
 * Plain C: opaque handle, plain pointers and sizes, int status codes.  No torch
 * types, no C++ types.  All entry points are thread-compatible, not thread-safe:
 * calls on one handle must be serialised by the caller (the reference's
 * VitInference is single-threaded and stateful too, inference.py:112-116).
 * Nothing here falls back to a CPU implementation: without a gfx950 device every
 * compute entry point returns VP_ERR_HIP.
 */
#ifndef VITPOSE_HIP_H
#define VITPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP_ABI_VERSION 4
#define VP_API __attribute__((visibility("default")))

/* status codes (0 = ok).  The Python host maps them onto the exception types the
 * reference raises at the same places (AssertionError / ValueError / KeyError,
 * easy_ViTPose/inference.py:91-92,127-128,138-144; vit_utils/util.py:33). */
enum {
    VP_OK = 0,
    VP_ERR_INVALID = 1,        /* bad argument / unsupported shape          */
    VP_ERR_HIP = 2,            /* HIP runtime error, no device, OOM         */
    VP_ERR_STATE = 3,          /* weights not loaded yet, handle destroyed  */
    VP_ERR_MISSING_TENSOR = 4, /* state-dict key absent (load_state_dict KeyError analogue) */
    VP_ERR_SHAPE = 5           /* state-dict tensor has the wrong size      */
};

/* arithmetic type of the GEMM/attention operands (accumulation is always fp32; LayerNorm / softmax statistics,
 * heatmaps and the decode are fp32; the residual stream is held as a hi + lo pair of 16-bit planes, >= 22 bits) */
enum {
    VP_DTYPE_F16 = 0,
    VP_DTYPE_BF16 = 1,
    /* OPT-IN, never a default: the encoder's qkv / fc1 / fc2 GEMMs on MXFP8 operands (OCP e4m3 + one power-of-two scale per 32 k,
     * csrc/mx8.h) through the block-scaled fp8 matrix instruction; residual stream, attention core, attn.proj, head and decode as in
     * VP_DTYPE_F16.  BASELINE configs[4].  Does NOT meet the north_star's 1e-3 on confidences (e4m3 carries 3 mantissa bits; measured
     * bounds in tests/test_gpu_fp8.py and DESIGN.md section 6); coordinates stay within +-0.5 px on peaked maps.  ViTPose-B / -L / -H only. */
    VP_DTYPE_FP8 = 2
};

/* layout of the crop batch handed to vp_infer* */
enum {
    VP_INPUT_F32_NCHW = 0, /* float32 [N,3,256,192], already normalised = output of pre_img (inference.py:314-318) */
    VP_INPUT_U8_NHWC = 1   /* uint8   [N,256,192,3] RGB crops; (x/255-mean)/std (inference.py:32-33,316-317) is applied on device */
};

typedef struct vp_ctx* vp_handle;
typedef struct vp_group* vp_group_handle; /* N handles in one process, one per device (vp_group_*) */

/* Model shape = one row of configs/ViTPose_common.py:65-195 + the dataset's
 * out_channels (configs/ViTPose_<dataset>.py).  Input is fixed at 256x192,
 * heatmaps at 64x48 (ViTPose_common.py:29-31). */
typedef struct vp_config {
    int32_t embed_dim;     /* 384 / 768 / 1024 / 1280 */
    int32_t depth;         /* 12 / 12 / 24 / 32       */
    int32_t num_heads;     /* 12 / 12 / 16 / 16  (head_dim must be 32, 64 or 80) */
    int32_t num_keypoints; /* 17 / 25 / 133 / ...      */
    int32_t dtype;         /* VP_DTYPE_*              */
    int32_t device_id;     /* HIP device ordinal      */
    int32_t max_batch;     /* workspace is sized for this many crops; larger N is processed in chunks */
} vp_config;

/* One tensor of the checkpoint, host float32, named exactly as in the reference's
 * state dict (`backbone.pos_embed`, `backbone.blocks.3.attn.qkv.weight`,
 * `keypoint_head.deconv_layers.1.running_var`, ... ; schema in SURVEY.md 8a,
 * loaded by the reference at easy_ViTPose/inference.py:162-166). */
typedef struct vp_tensor_desc {
    const char* name;
    const float* data;
    int64_t numel;
} vp_tensor_desc;

/* Per-kernel-family timing collected with HIP events on the handle's stream. */
#define VP_PROF_GEMM_PROJ 0  /* attn.proj GEMM (bias + residual planes + LayerNorm statistics), HBM-bound */
#define VP_PROF_GEMM_FC1 1   /* fc1 GEMM (bias + GELU)                     */
#define VP_PROF_GEMM_QKV 2   /* qkv GEMM (bias)                            */
#define VP_PROF_GEMM_PATCH 3 /* patch-embed GEMM (bias + pos)              */
#define VP_PROF_GEMM_DECONV 4
#define VP_PROF_GEMM_FINAL 5
#define VP_PROF_ATTN 6
#define VP_PROF_LAYERNORM 7
#define VP_PROF_IM2COL 8
#define VP_PROF_DECODE 9
#define VP_PROF_GEMM_FC2 10  /* mlp.fc2 GEMM (same epilogue as proj, K = 4 D) */
#define VP_PROF_COUNT 11

typedef struct vp_profile {
    double ms[VP_PROF_COUNT];      /* summed kernel time since the last reset  */
    double flops[VP_PROF_COUNT];   /* summed algorithmic FLOPs (2*M*N*K)       */
    double bytes[VP_PROF_COUNT];   /* summed algorithmic HBM bytes              */
    int64_t launches[VP_PROF_COUNT];
} vp_profile;

VP_API int vp_abi_version(void);

/* Create a context on cfg->device_id: stream, workspaces.  Replaces the model
 * construction `ViTPose(model_cfg)` + `.to(device)` (inference.py:156-167). */
VP_API int vp_create(vp_handle* out, const vp_config* cfg);

/* Upload a checkpoint: folds BatchNorm (eval, eps 1e-5) into the deconv weights,
 * pre-adds pos_embed[:,1:]+pos_embed[:,:1] (vit.py:382), re-tiles the transposed-conv
 * weights into 4 output-parity GEMM operands, converts matrices to cfg.dtype.
 * Replaces `load_state_dict` (inference.py:162-166).  Missing key ->
 * VP_ERR_MISSING_TENSOR, wrong numel -> VP_ERR_SHAPE. */
VP_API int vp_load_weights(vp_handle h, const vp_tensor_desc* tensors, int32_t n_tensors);

/* The hot path on host buffers: H2D crops, model, decode, D2H keypoints; returns
 * when `out` is complete.  Batched replacement of `_inference_torch`
 * (inference.py:320-328).  org_wh = N x (org_w, org_h) int32 of each crop before
 * pre_img's resize (NULL = 192x256 for all); out = float32 [N, K, 3] (y, x, conf).
 * Numerics contract: every call is run-to-run bit-identical (no atomics anywhere) and within the parity tolerances of the
 * reference (+-0.5 px, confidences 1e-3).  Equal BITS for a crop at every batch size hold inside the one-launch kernel family;
 * a chunk of one or two crops (ViTPose-H: also seven or eight) runs mlp.fc2 as four k ranges + a fixed-order reduction (a
 * different fp32 accumulation order), so such a call differs from the same crop inside a larger batch in the last bits.
 * VP_SPLITK=0 (read at vp_create) pins a handle to the one-launch family. */
VP_API int vp_infer(vp_handle h, const void* crops, int32_t input_format, int32_t n,
             const int32_t* org_wh, float* out);

/* Same with device-resident buffers (e.g. torch tensors' data_ptr()); enqueued on
 * the handle's stream, returns after the stream has been synchronised when
 * `sync` != 0.  d_org_wh may be NULL. */
VP_API int vp_infer_device(vp_handle h, const void* d_crops, int32_t input_format, int32_t n,
                    const int32_t* d_org_wh, float* d_out, int32_t sync);

/* vp_infer_device ordered against the CALLER's stream (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream; NULL =
 * the legacy default stream): the library's kernels start after everything enqueued on caller_stream so far (the producers
 * of d_crops / d_org_wh), and work enqueued on caller_stream afterwards (consumers of d_out) starts after them.  Returns
 * without synchronising.  This is the entry a framework should use; plain vp_infer_device leaves the ordering to the caller.
 * Batches of <= 16 crops (that fit max_batch; VP_CALLER_STREAM=0: never) are enqueued ON caller_stream itself -- same ordering guarantee, without the two cross-stream
 * events of the general path (~0.1 ms of a 0.6-2.4 ms call).  The handle orders its next call behind that work by itself, whatever entry or stream it comes through,
 * and vp_synchronize / vp_destroy wait for it; caller_stream is not touched again after the call returns (it may be destroyed once its work has completed). */
VP_API int vp_infer_device_stream(vp_handle h, const void* d_crops, int32_t input_format, int32_t n,
                                  const int32_t* d_org_wh, float* d_out, void* caller_stream);

/* Asynchronous host path: the H2D copy of call i+1 and the D2H copy of call i-1 run on a copy stream under the compute of
 * call i (two slots).  vp_infer_submit enqueues one batch (1 .. max_batch crops) and returns a slot id at once; `crops`,
 * `org_wh` must stay valid until the upload has happened and `out` until vp_infer_wait(slot) has returned.  For the copies
 * to be truly asynchronous the host buffers must be pinned: vp_host_alloc / vp_host_free (hipHostMalloc).  At most two
 * submissions may be in flight. */
VP_API void* vp_host_alloc(size_t bytes);
VP_API void vp_host_free(void* p);
VP_API int vp_infer_submit(vp_handle h, const void* crops, int32_t input_format, int32_t n, const int32_t* org_wh,
                           float* out, int32_t* slot);
VP_API int vp_infer_wait(vp_handle h, int32_t slot);

/* Multi-GPU in ONE process (the reference has no inference-side parallelism to mirror, inference.py:167,259-272
 * -- this is the build's own contract): one handle per device, weights replicated, the crops of a call sharded contiguously
 * (ceil(n / devices) each), every device running its shard concurrently (asynchronous submit on each handle).
 * vp_group_infer gathers the keypoints in the host buffer `out` [n, K, 3] (each device's D2H lands in its slice).
 * vp_group_infer_allgather additionally leaves ALL keypoints on EVERY device: d_all[i] = device buffer [n, K, 3] on device i;
 * each shard is copied peer to peer (hipMemcpyPeerAsync over the xGMI link of the pair) on its owner's stream -- the
 * all-gather of north_star without a collective library in the C ABI (the one-process-per-GPU Python host uses RCCL:
 * easy_vitpose_amd/parallel.py).  `out` may be NULL there.  cfg->device_id is ignored. */
/* Concurrency: a call enqueues upload + model + decode + download on EVERY member first and only then waits
 * for the members in turn and copies their slices into `out`.  Neither direction blocks the enqueue on a device: the download lands
 * in a pinned per-member staging buffer; the upload is asynchronous as it is when `crops` is page-locked memory the runtime knows
 * (vp_host_alloc / hipHostMalloc / hipHostRegister: checked with hipPointerGetAttributes) and otherwise goes through a pinned
 * per-member staging buffer in 4 MiB pieces (host memcpy of piece k + 1 under the DMA of piece k).  Pass pinned crops for full overlap:
 * with pageable memory the calling thread's memcpy (~10 GB/s: ~4 ms per 256 u8 crops, ~15 ms per 256 f32 crops) is what serialises the members.
 * Ordering of vp_group_infer_allgather: the peer copies into d_all[j] run on the OWNER's private stream; nothing orders them
 * against work the caller has in flight on device j, so d_all[*] must be idle (already synchronised) when the call starts;
 * the call returns after every copy has completed (host-synchronised), so consumers need no further ordering.  Pairs without
 * peer access are not an error (the runtime stages those copies through the host); vp_group_peer_access reports them. */
VP_API int vp_group_create(vp_group_handle* out, const vp_config* cfg, const int32_t* device_ids, int32_t n_devices);
/* number of ordered device pairs (i != j) of the group for which peer access could NOT be enabled (0 on an xGMI-connected node) */
VP_API int vp_group_peer_access_missing(vp_group_handle g);
VP_API int vp_group_size(vp_group_handle g);
VP_API vp_handle vp_group_member(vp_group_handle g, int32_t i);
VP_API int vp_group_load_weights(vp_group_handle g, const vp_tensor_desc* tensors, int32_t n_tensors);
VP_API int vp_group_infer(vp_group_handle g, const void* crops, int32_t input_format, int32_t n, const int32_t* org_wh, float* out);
VP_API int vp_group_infer_allgather(vp_group_handle g, const void* crops, int32_t input_format, int32_t n, const int32_t* org_wh,
                                    float* const* d_all, float* out);
VP_API int vp_group_destroy(vp_group_handle g);
VP_API const char* vp_group_last_error(vp_group_handle g);

/* Whole-frame entry: the crop loop of VitInference.inference (inference.py:259-266) on device.
 * frame = uint8 RGB [fh, fw, 3] on the host; crop_params = n x 8 int32 {x0, y0, cw, ch, left_pad, top_pad, pw, ph}:
 * the +10 px padded & clipped box (:261-262) and the zero-pad geometry of pad_image (vit_utils/inference.py:41-70).
 * One H2D of the frame; crop + zero-pad + OpenCV-style 8-bit bilinear resize (:316) + normalisation run on device.
 * out = float32 [n, K, 3] (y, x, conf) in padded-crop pixels; the caller adds (y0 - top_pad, x0 - left_pad) as :270 does. */
VP_API int vp_infer_frame(vp_handle h, const uint8_t* frame, int32_t fh, int32_t fw, const int32_t* crop_params,
                          int32_t n, float* out);

/* Many frames, one call: the crops of several frames (a video chunk, several cameras) in one batch.
 * frames[n_frames]: uint8 RGB [h, w, 3], C-contiguous.  crop_params = n x 9 int32 {frame, x0, y0, cw, ch, left_pad, top_pad, pw, ph}:
 * the frame index, then vp_infer_frame's eight values.  Crops come in any order, any crop may name any frame, a frame may have none.
 * The crops run in the caller's order in chunks of max_batch, exactly as vp_infer chunks them: the result has the bits of vp_infer on
 * the host-prepared crops in the same order.  out = float32 [n, K, 3] in padded-crop pixels, as vp_infer_frame.
 * frames_on_device = 0: every frame with at least one crop is uploaded as ONE copy of the row band its crops cover (rows [min y0,
 * max(y0 + ch)), full width) into a device staging arena of the handle (grown, never shrunk; freed by vp_destroy); frames without
 * crops are not copied.  frames_on_device = 1: the frames are device memory of the handle's device (checked with hipPointerGetAttributes
 * before anything is launched) and are read in place; the caller guarantees they are complete when the call starts.
 * Every crop is checked before any copy or launch (vp_dbg_frame_plan): VP_ERR_INVALID for a frame index outside [0, n_frames), a crop
 * outside its frame or its padded canvas, a non-positive size, a NULL data pointer on a referenced frame, n > 0 with n_frames <= 0.
 * n = 0: VP_OK, nothing is written.  A ViTPose+ handle runs its active expert (vp_set_expert). */
typedef struct vp_frame {
    const uint8_t* data;
    int32_t h;
    int32_t w;
} vp_frame;
VP_API int vp_infer_frames(vp_handle h, const vp_frame* frames, int32_t n_frames, int32_t frames_on_device,
                           const int32_t* crop_params, int32_t n, float* out);

/* Detector boxes to frame keypoints, all on the device, ordered on the CALLER's stream: the stream-ordered twin of vp_infer_frames.
 * frames[n_frames] (host table): uint8 RGB [h, w, 3] frames in device memory of the handle's device, every entry checked before anything is
 * enqueued (hipPointerGetAttributes + hipMemGetAddressRange: the whole frame inside one allocation); the caller's stream produces them.
 * d_xyxy: device float32 boxes, row i = (x1, y1, x2, y2) at d_xyxy + i * row_stride (row_stride >= 4: a detector's [n, 6] tensor passes in place
 * with 6).  d_frame_idx: device int32 [n], the frame of each box (NULL: frame 0).  pad: pixels added on every side before clipping (the
 * reference's 10).  Per box, a kernel computes cropprep.crop_params (the padded, clipped box; pad_image's canvas) in double precision, bit for
 * bit what the host computes on the float32 boxes widened to float64 (|coordinates| < 2^30; larger finite ones are clipped like any other).
 * d_out: device float32 [n, K, 3] (y, x, conf) in FRAME pixels: row i has the bits of vp_infer_frames on those crop rows (same max_batch
 * chunks, so the same plan, split-K included) followed by the offsets (y0 - top_pad, x0 - left_pad) added as VitInference.inference_frames
 * adds them.  d_crop_params (may be NULL): device int32 [n, 9], each box's frames_crop_params row {frame, x0, y0, cw, ch, left_pad, top_pad,
 * pw, ph}; (x0, y0, x0 + cw, y0 + ch) is the reference's in-place box update.  d_status (may be NULL): device int32 [n]: 0 ok, 1 frame index
 * outside [0, n_frames), 2 a coordinate is not finite, 3 the box is empty after padding and clipping (the host path's 'empty box' assertion),
 * checked in that order.  A row with a non-zero status reads no frame, gets all-zero keypoints and an all-zero d_crop_params row.
 * Ordering as vp_infer_device_stream: batches of <= 16 crops (that fit max_batch) run on caller_stream itself, larger ones on the handle's
 * stream fenced with two events; the next call on any stream, vp_synchronize and vp_destroy order themselves behind the work.  n > max_batch
 * runs in max_batch chunks.  Per chunk: the box kernel (launched once per 64 frames of the table, which travels by kernel argument) and the crop
 * kernel run eagerly, then the forward, decode and offset kernel (a replayed hipGraph for chunks of <= 16 crops).  The call never blocks the
 * host: no stream / device / event synchronisation and no copy from host memory; its device buffers are sized by max_batch and allocated on the
 * first call.  The one exception is vp_infer_device_stream's: when a fifth distinct small chunk (size, output pointer) evicts a cached graph,
 * the handle's current stream is synchronised once before that graph is destroyed.
 * VP_ERR_INVALID before anything is enqueued: a NULL pointer (frames, d_xyxy, d_out with n > 0), row_stride < 4, pad < 0, n > 0 with
 * n_frames <= 0, a frame side outside [1, 2^24], a frame that is not device memory of the handle's device.  n = 0: VP_OK, nothing is
 * written.  A ViTPose+ handle runs its active expert (vp_set_expert). */
VP_API int vp_infer_boxes_stream(vp_handle h, const vp_frame* frames, int32_t n_frames, const float* d_xyxy, int32_t row_stride,
                                 const int32_t* d_frame_idx, int32_t n, int32_t pad, float* d_out, int32_t* d_crop_params,
                                 int32_t* d_status, void* caller_stream);

/* Flip-test inference (the optional accuracy mode of the reference head, topdown_heatmap_simple_head.py:195-218 with
 * flip_back of vit_utils/post_processing/post_transforms.py:110-147; `flip_test=True, shift_heatmap=False` in
 * configs/ViTPose_common.py:91-93): the model runs on the crops and on their left-right mirror, the mirrored heatmaps are
 * flipped back (joint pairs swapped, x reversed, optionally shifted one pixel right) and averaged with the first ones, the
 * average is decoded.  flip_pairs = n_pairs x 2 joint indices (the dataset's mirror pairs; the reference ships none).
 * out [n,K,3] and / or heatmaps [n,K,64,48] (either may be NULL, not both). */
VP_API int vp_infer_flip(vp_handle h, const void* crops, int32_t input_format, int32_t n, const int32_t* org_wh,
                         const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap, float* out, float* heatmaps);

/* Flip-test as a MODE of the handle (how the reference's test configs quote accuracy: flip_test=True).  After vp_set_flip_test every entry that
 * decodes keypoints -- vp_infer, vp_infer_device, vp_infer_device_stream, vp_infer_submit / vp_infer_wait, vp_infer_frame, vp_infer_frames,
 * vp_infer_boxes_stream, vp_group_infer / vp_group_infer_allgather (set on every member: vp_group_set_flip_test) -- returns the keypoints of
 * 0.5 (heatmaps(crop) + flip_back(heatmaps(mirrored crop))), in that entry's own output layout and coordinate frame, and vp_infer_heatmaps returns
 * those averaged maps.  flip_pairs / shift_heatmap as in vp_infer_flip; the pairs are validated against the ACTIVE head's K and uploaded once.
 *   How it runs: the crops and their mirror images form ONE forward batch of twice the rows (crop, mirror, crop, mirror, ...), planned, padded and
 *   replayed from a hipGraph like any batch of that size, and the decode averages the two maps of a joint on the fly.  A chunk therefore holds
 *   max_batch / 2 of the caller's crops (vp_infer_submit: 1 .. max_batch / 2 per call), the small-batch thresholds (VP_GRAPH, VP_CALLER_STREAM)
 *   count the rows that run (2 n), and n crops under the mode are a 2 n batch: bit identity with another batch size or with vp_infer_flip (two
 *   passes of n) is NOT promised -- equal within the rounding of the 16-bit GEMMs, run-to-run identical.
 *   Not under the mode: vp_infer_tokens and vp_infer_flip (unchanged, whatever the mode); vp_infer_experts and its twins return VP_ERR_STATE while it is on
 *   (they run under the per-expert form below, vp_set_flip_test_experts).
 *   ViTPose+ handles: the mode belongs to the active expert's joints.  vp_set_expert to a head with the same K keeps it; to a head with another K the
 *   switch takes place, the mode is CLEARED and the call returns VP_ERR_STATE saying so (set it again with that dataset's pairs).
 *   fp8 handles: the mode sits above the encoder and runs as it does on fp16 (exactness of the fused decode and run-to-run identity are tested, parity figures are not).
 * VP_ERR_INVALID: n_pairs < 0, NULL pairs with n_pairs > 0, a joint index outside [0, K).  VP_ERR_STATE: weights not loaded, a vp_infer_submit in
 * flight, or max_batch == 1 (a crop and its mirror share the batch; there is no hidden two-pass fallback).  The set waits for the handle's
 * enqueued work (the table may still be read).  vp_clear_flip_test: back to the default; a handle whose mode was never set, or was cleared, runs exactly the launches it ran before.
 * vp_flip_test_enabled: 1 while the mode is on.  Library builds that carry the mode define VP_HAS_FLIP_TEST_MODE. */
#define VP_HAS_FLIP_TEST_MODE 1
VP_API int vp_set_flip_test(vp_handle h, const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap);
VP_API int vp_clear_flip_test(vp_handle h);
VP_API int vp_flip_test_enabled(vp_handle h);
/* the same on every member of a group (all or none: a member's refusal clears the mode on all of them).  vp_group_infer* return VP_ERR_STATE
 * when the members disagree on the mode (set through vp_group_member one by one). */
VP_API int vp_group_set_flip_test(vp_group_handle g, const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap);
VP_API int vp_group_clear_flip_test(vp_group_handle g);
/* The mode with ONE PARTNER TABLE PER EXPERT, for ViTPose+ handles: what lets the per-crop expert entries run under it.  n_pairs = host int32 [E] (E from
 * vp_expert_info), flip_pairs = expert 0's pairs, then expert 1's, ...: (sum of n_pairs) x 2 joint indices, each expert's validated against ITS K_e (a refusal
 * names the expert and the pair).  One device table [E, Kmax] is uploaded; the set waits for the handle's enqueued work as vp_set_flip_test does.  While this form is on:
 *   - every entry that honours the single-table mode honours this one with the ACTIVE expert's table, and vp_set_expert to any expert keeps the mode on and
 *     returns VP_OK (every expert has its own validated table: nothing is cleared);
 *   - vp_infer_experts, vp_infer_experts_device_stream, vp_infer_frames_experts and vp_infer_boxes_experts_stream run under it: row i = the flip-test keypoints of
 *     crop i under expert e_i's table, in the entry's own layout and coordinate frame, joints beyond K_{e_i} zero.  A chunk holds max_batch / 2 crops: they go into
 *     stable expert order, position j as forward rows 2 j (the crop) and 2 j + 1 (its mirror), so every expert's rows start at an even row; one encoder pass of
 *     2 nb rows, one head per expert present on its 2 cnt rows, ONE decode launch that averages each crop's two maps of a joint on the fly.  A chunk of one
 *     expert runs the launches of vp_set_expert + the mode.  The hipGraph pattern counts crops per expert; VP_GRAPH / VP_CALLER_STREAM count the 2 nb rows;
 *   - vp_flip_test_enabled returns 2 (1 for the single-table mode); vp_clear_flip_test switches it off; vp_set_flip_test replaces it by the single-table mode.
 * The single-table mode is unchanged: it refuses the per-crop entries and clears on a change of K.  No group, submit / wait or fp8 form (ViTPose+ refuses fp8).
 * VP_ERR_INVALID: NULL n_pairs, a negative count, NULL pairs with a positive total, an index outside [0, K_e).  VP_ERR_STATE: a plain (single-dataset) handle,
 * weights not loaded, a vp_infer_submit in flight, max_batch == 1.  A refused call leaves the handle as it was. */
#define VP_HAS_FLIP_TEST_EXPERTS 1
VP_API int vp_set_flip_test_experts(vp_handle h, const int32_t* flip_pairs, const int32_t* n_pairs, int32_t shift_heatmap);
/* HOST ONLY taps of the mode's pure functions: the partner table of k joints (partner may be NULL: validation only; the reason of a refusal is in
 * vp_last_error(NULL)), and the interleaved batch's index function -- src[r] / mirror[r] = the source crop of output row r in [0, rows) and whether
 * it is mirrored, for n crops in a forward of rows >= 2 n crops (rows beyond 2 n repeat the last one). */
VP_API int vp_dbg_flip_partner(int32_t k, const int32_t* flip_pairs, int32_t n_pairs, int32_t* partner);
VP_API int vp_dbg_flip_layout(int32_t n, int32_t rows, int32_t* src, int32_t* mirror);
/* The mode's decode kernel alone, on host data (as vp_decode_only): heatmaps2 = float32 [2 n, k, 64, 48], crop i's maps at 2 i and its mirror
 * image's at 2 i + 1 -> out [n, k, 3] = vp_decode_only of 0.5 (crop + flip_back(mirror)), bit for bit, without forming that tensor. */
VP_API int vp_dbg_decode_flip(int32_t device_id, const float* heatmaps2, int32_t n, int32_t k, const int32_t* flip_pairs, int32_t n_pairs,
                              int32_t shift_heatmap, const int32_t* org_wh, float* out);

/* Parity/debug taps.  Heatmaps = ViTPose.forward output, float32 [N, K, 64, 48] (under the flip-test mode: the averaged maps). */
VP_API int vp_infer_heatmaps(vp_handle h, const void* crops, int32_t input_format, int32_t n, float* heatmaps);
/* Backbone output after last_norm (vit.py:387), float32 [N, 192, D]. */
VP_API int vp_infer_tokens(vp_handle h, const void* crops, int32_t input_format, int32_t n, float* tokens);

/* ViTPose+ checkpoints (multi-dataset "mixture of experts", the reference's model_split.py without the split).  vp_load_weights recognises a
 * state dict with backbone.blocks.0.mlp.experts.0.weight: E experts (0 = coco with keypoint_head, e = 1..5 = aic / mpii / ap10k / apt36k /
 * wholebody with associate_keypoint_heads.{e-1}, final layer cut to K = 14 / 16 / 17 / 17 / 133 rows), each the last P output features of every
 * block's mlp.fc2.  The handle must have been created with num_keypoints = 17 and dtype fp16 / bf16 (fp8: VP_ERR_INVALID).
 * vp_expert_info: *n_experts = E (0 on a plain handle), *part_features = P, k_per_expert[e] = K_e (cap 8; any pointer may be NULL). */
VP_API int vp_expert_info(vp_handle h, int32_t* n_experts, int32_t* part_features, int32_t* k_per_expert);
/* Make expert e the active one (default 0 = coco): every other entry point (vp_infer*, submit / wait, vp_infer_frame, vp_infer_flip,
 * vp_infer_heatmaps, vp_infer_tokens) then runs expert e's mlp.fc2 and head, and K = K_e in every output shape -- bit for bit the handle of
 * model_split.py's file for that dataset.  VP_ERR_INVALID for e outside [0, E), VP_ERR_STATE on a plain handle or with a vp_infer_submit in flight. */
VP_API int vp_set_expert(vp_handle h, int32_t e);
/* One call, one encoder pass, a different expert per crop: expert_ids[i] in [0, E).  out = float32 [n, Kmax, 3] (Kmax = the largest K_e of the
 * checkpoint): crop i fills its first K_{e_i} joints, the rest are written as 0.  The crops are ordered by expert inside the call (mlp.fc2 of all
 * experts in one launch per layer, one head per expert present, ONE decode launch for the chunk; chunks of up to VP_GRAPH crops are replayed from a
 * hipGraph keyed on the count per expert, as for its twins below); crop i's result equals vp_set_expert(e_i) + vp_infer on that crop under
 * the one-launch family (VP_SPLITK=0).  VP_ERR_STATE on a plain handle. */
VP_API int vp_infer_experts(vp_handle h, const void* crops, int32_t input_format, int32_t n, const int32_t* expert_ids,
                            const int32_t* org_wh, float* out);

/* Per-crop experts on the production entries: the twins of vp_infer_device_stream, vp_infer_frames and vp_infer_boxes_stream that take expert_ids -- HOST
 * int32 [n], expert_ids[i] in [0, E) the dataset of crop / box i (the caller knows n, and which detector or class group produced which rows, on the host).
 * Everything else -- arguments, staging, chunks of max_batch, ordering, what blocks the host and what does not -- is the plain entry's; the outputs are
 * [n, Kmax, 3] rows in the CALLER's order with the joints beyond K_{e_i} written as 0, as vp_infer_experts returns them, on the device where the plain entry
 * writes to the device.  Row i has the bits of vp_infer_experts on the same crops, ids and max_batch.
 *   How a chunk runs: its crops in stable expert order (device crops: one gather; frames and boxes are cropped straight into that order), the encoder once
 *   with every expert's mlp.fc2 in one launch per layer, one head per expert present, ONE decode launch for the whole chunk that writes each crop's row in the
 *   caller's order, the boxes entry's offsets on those rows.  The chunk's tables (ids, order, decode records) reach the device as kernel arguments of a small
 *   kernel in front of the chunk: no copy from host memory, no synchronisation.  Chunks of <= 16 crops replay a hipGraph keyed on the count per expert: two
 *   calls with the same counts in another permutation replay the same graph.  A chunk whose crops share one expert runs the plain forward of that expert.
 * vp_infer_experts_device_stream: ordering and host behaviour of vp_infer_device_stream (<= 16 crops on caller_stream itself, larger batches on the handle's
 *   stream between two events; never blocks the host but for the graph eviction documented there).  d_org_wh: device int32 [n, 2] in the caller's order, or NULL.
 * vp_infer_frames_experts: vp_infer_frames' staging and host waits; out = host float32 [n, Kmax, 3] in padded-crop pixels.
 * vp_infer_boxes_experts_stream: vp_infer_boxes_stream plus expert_ids; d_out = device float32 [n, Kmax, 3] in frame pixels, d_crop_params and d_status in
 *   the caller's order with the plain entry's values; a row with a non-zero status reads no frame and is all zero.
 * Refusals, before anything is enqueued: the plain entry's own, then VP_ERR_STATE on a plain (single-dataset) handle, VP_ERR_INVALID for NULL expert_ids or an
 * id outside [0, E) (the message names the crop), VP_ERR_STATE while the flip-test mode is on (its partner table belongs to one head) or a vp_infer_submit is in
 * flight.  The active expert (vp_set_expert) is the same after the call as before.  Library builds that carry these entries define VP_HAS_EXPERT_ENTRIES. */
#define VP_HAS_EXPERT_ENTRIES 1
VP_API int vp_infer_experts_device_stream(vp_handle h, const void* d_crops, int32_t input_format, int32_t n, const int32_t* expert_ids,
                                          const int32_t* d_org_wh, float* d_out, void* caller_stream);
VP_API int vp_infer_frames_experts(vp_handle h, const vp_frame* frames, int32_t n_frames, int32_t frames_on_device, const int32_t* crop_params,
                                   int32_t n, const int32_t* expert_ids, float* out);
VP_API int vp_infer_boxes_experts_stream(vp_handle h, const vp_frame* frames, int32_t n_frames, const float* d_xyxy, int32_t row_stride,
                                         const int32_t* d_frame_idx, int32_t n, int32_t pad, const int32_t* expert_ids, float* d_out,
                                         int32_t* d_crop_params, int32_t* d_status, void* caller_stream);
/* Frames as a video pipeline holds them: NV12 decoder surfaces, BGR capture buffers, pitched views (an ROI, one frame of a batch buffer).  vp_image describes
 * one frame by plane pointers and row pitches, and the pixel fetch of the crop kernel converts each SOURCE pixel to RGB8 before any interpolation -- the
 * interpolation arithmetic is the RGB route's.  The result of either entry below is therefore, bit for bit, what vp_infer_frames / vp_infer_boxes_stream
 * return on the same frame converted on the host (easy_vitpose_amd/cropprep.py to_rgb), without the full-frame conversion pass: only the pixels under the
 * boxes are read.
 *   NV12 -> RGB (int32, arithmetic shifts; one definition in csrc/pixfmt.h):  y' = max(Y - yoff, 0), u' = U - 128, v' = V - 128,
 *     R = clip255((cy y' + crv v' + 2^19) >> 20),  G = clip255((cy y' + cgu u' + cgv v' + 2^19) >> 20),  B = clip255((cy y' + cbu u' + 2^19) >> 20)
 *     matrix            yoff  cy       crv      cgu      cgv      cbu
 *     VP_YUV_BT601      16    1220542  1673527  -409993  -852492  2116026    (OpenCV's COLOR_YUV2RGB_NV12 constants; parity against that binary is unpinned)
 *     VP_YUV_BT709      16    1220945  1879825  -223607  -558796  2215014
 *     VP_YUV_BT601_FULL 0     1048576  1470104  -360853  -748826  1858077
 *   Chroma is replicated, not interpolated: pixel (y, x) reads the UV pair (y >> 1, x >> 1).  Odd h or w is legal (the ceil sizes keep that index valid).
 *   The two planes are separate pointers: one allocation (a decoder surface, UV at base + pitch * aligned_h) or two.  Not supported: 10-bit P010 / P016,
 *   planar I420, RGBA, interpolated chroma.
 * vp_infer_images: the contract of vp_infer_frames (expert_ids == NULL: the handle's active expert) or of vp_infer_frames_experts (expert_ids != NULL) --
 *   chunks of max_batch, the staging (host frames: ONE upload per plane per frame of the row band its crops cover, Y rows [lo, hi) and UV rows
 *   [lo >> 1, (hi + 1) >> 1), (rows - 1) * pitch + row bytes each, never a byte past the last pixel), the host waits, the refusals.
 * vp_infer_boxes_images_stream: the contract of vp_infer_boxes_stream (expert_ids == NULL) or of vp_infer_boxes_experts_stream: no host synchronisation,
 *   the stream ordering, the status codes; the box kernel is launched once per 64 frames of the table.
 * Frames of one call may differ in format and matrix.  Device planes are checked one by one before anything is enqueued: (plane rows - 1) * pitch + row
 * bytes inside one allocation of the handle's device.  VP_ERR_INVALID on top of the plain entries' refusals (vp_dbg_image_plan; the message names the crop
 * or the frame): an unknown format or matrix, a negative pitch, pitch[0] below the row bytes, NV12 with a NULL plane[1] or pitch[1] < 2 ceil(w / 2).
 * vp_infer_frame, vp_infer_frames, vp_infer_frames_experts, vp_infer_boxes_stream and vp_infer_boxes_experts_stream are these entries on
 * vp_image{{data, NULL}, {3 w, 0}, h, w, VP_PIX_RGB24, 0}.  Library builds that carry them define VP_HAS_IMAGE_ENTRIES. */
#define VP_HAS_IMAGE_ENTRIES 1
#define VP_PIX_RGB24 0   /* plane[0]: R,G,B bytes, pitch[0] >= 3 w                      */
#define VP_PIX_BGR24 1   /* plane[0]: B,G,R bytes, pitch[0] >= 3 w                      */
#define VP_PIX_NV12  2   /* plane[0]: Y [h, w], pitch[0] >= w; plane[1]: U,V pairs
                            [ceil(h/2), ceil(w/2)], pitch[1] >= 2 ceil(w/2)            */
#define VP_YUV_BT601      0   /* limited range (Y 16..235) */
#define VP_YUV_BT709      1   /* limited range             */
#define VP_YUV_BT601_FULL 2   /* full range (JPEG / MJPEG) */
typedef struct vp_image {
    const uint8_t* plane[2];
    int64_t pitch[2];      /* bytes per row of each plane */
    int32_t h, w;
    int32_t format;        /* VP_PIX_*  */
    int32_t matrix;        /* VP_YUV_*, read for NV12 only */
} vp_image;   /* 48 bytes */
VP_API int vp_infer_images(vp_handle h, const vp_image* images, int32_t n_images, int32_t images_on_device, const int32_t* crop_params, int32_t n,
                           const int32_t* expert_ids, float* out);
VP_API int vp_infer_boxes_images_stream(vp_handle h, const vp_image* images, int32_t n_images, const float* d_xyxy, int32_t row_stride,
                                        const int32_t* d_frame_idx, int32_t n, int32_t pad, const int32_t* expert_ids, float* d_out,
                                        int32_t* d_crop_params, int32_t* d_status, void* caller_stream);
/* HOST ONLY, no device needed: vp_dbg_frame_plan over vp_image, the function vp_infer_images runs first (bands [n_images, 2] in frame rows, may be NULL).
 * VP_ERR_INVALID, the crop or frame named in vp_last_error(NULL), for everything vp_dbg_frame_plan refuses and for the image refusals listed above. */
VP_API int vp_dbg_image_plan(const vp_image* images, int32_t n_images, const int32_t* params9, int32_t n, int32_t* bands);
/* the device crop / zero-pad / resize kernel alone on ONE image whose planes are on the host (vp_dbg_crop_prep over vp_image): uint8 RGB crops [n, 256, 192, 3] */
VP_API int vp_dbg_crop_prep_image(int32_t device_id, const vp_image* image, const int32_t* crop_params, int32_t n, uint8_t* out);

/* The training-protocol crop: TopDownAffine(use_udp=True) on the box's own centre and scale, the crop ViTPose checkpoints were trained and evaluated on
 * (the reference's datasets/COCO.py _xywh2cs, post_transforms.py get_warp_matrix, and transform_preds(center, scale, use_udp=True) on the way back), as a second
 * crop route beside the pad route above; the pad route stays the default everywhere.  csrc/affinegeom.h states the arithmetic once:
 *   box -> (cx, cy, S_w, S_h): the box centre, the box EXTENDED to 3:4 with image content (not padded with black) and scaled by box_scale (the reference: 1.25),
 *     float32 at the reference's widths; the box is not clipped to the frame, pixels outside it read as 0; a side above 2^24 is clamped to 2^24.
 *   crop pixel (ox, oy) of the 192 x 256 crop samples the frame at  x = ox (S_w / 191) + (cx - S_w / 2),  y = oy (S_h / 255) + (cy - S_h / 2)  (fp64), bilinear
 *     in fixed point: 1/32-pixel positions Xq = floor(32 x + 0.5), 15-bit weights, (sum + 16384) >> 15 on source pixels converted to RGB8 as the pad route converts
 *     them.  Modelled on OpenCV's 8-bit warpAffine(INTER_LINEAR, BORDER_CONSTANT 0); parity against that binary is unpinned and not claimed.
 *   keypoints come back in FRAME pixels with one rounding: x = (float)(rx (S_w / 47) + cx - S_w / 2), y with 63 and S_h; no offsets follow.
 * vp_infer_images_affine: the frames entry.  frame_idx int32 [n] (NULL: frame 0) and cs float32 [n, 4] = (cx, cy, S_w, S_h) on the host (easy_vitpose_amd/cropprep.py
 *   box_to_cs), out [n, K, 3] (y, x, conf) in frame pixels.  Host frames are uploaded once: the row band their crops sample, computed from the map and clipped to
 *   the frame.  The chunks, the host waits and the frame refusals are vp_infer_images'; VP_ERR_INVALID too for a centre that is not finite or a scale that is not
 *   finite, not positive or above 2^24 (vp_dbg_affine_plan).
 * vp_infer_boxes_affine_stream: the boxes entry, under the ordering rules of vp_infer_boxes_images_stream word for word -- no synchronisation and no host copy,
 *   batches of up to 16 crops on the caller's stream.  d_cs float32 [n, 4] (may be NULL) receives every box's centre and scale, d_status (may be NULL) the status
 *   codes of vp_infer_boxes_stream (3: w <= 0 or h <= 0 of the box itself).  A row with a non-zero status reads no frame and gets zero keypoints and a zero d_cs row.
 *   VP_ERR_INVALID, before anything is enqueued, for everything vp_infer_boxes_images_stream refuses and for a box_scale that is not finite or <= 0.
 * Both run under the handle's flip-test mode, and a ViTPose+ handle runs its active expert.  Not part of this route: per-crop experts, pose NMS on its output (the
 * NMS area is the pad route's cw ch), the group, the submit / wait slots, rotation, and the non-UDP get_affine_transform.
 * Library builds that carry the route define VP_HAS_AFFINE_CROP. */
#define VP_HAS_AFFINE_CROP 1
VP_API int vp_infer_images_affine(vp_handle h, const vp_image* images, int32_t n_images, int32_t images_on_device, const int32_t* frame_idx, const float* cs,
                                  int32_t n, float* out);
VP_API int vp_infer_boxes_affine_stream(vp_handle h, const vp_image* images, int32_t n_images, const float* d_xyxy, int32_t row_stride,
                                        const int32_t* d_frame_idx, int32_t n, float box_scale, float* d_out, float* d_cs, int32_t* d_status,
                                        void* caller_stream);
/* HOST ONLY, no device needed.  vp_dbg_box_cs: what the box kernel of vp_infer_boxes_affine_stream computes, cs [n, 4] and status [n] (either may be NULL; a frame
 * index outside [0, n_frames) is status 1).  vp_dbg_affine_plan: the function vp_infer_images_affine runs first (bands [n_images, 2] in frame rows, may be NULL);
 * VP_ERR_INVALID with the crop named in vp_last_error(NULL). */
VP_API int vp_dbg_box_cs(const float* xyxy, int32_t row_stride, const int32_t* frame_idx, int32_t n_frames, int32_t n, float box_scale, float* cs, int32_t* status);
VP_API int vp_dbg_affine_plan(const vp_image* images, int32_t n_images, const int32_t* frame_idx, const float* cs, int32_t n, int32_t* bands);
/* One kernel on host data.  vp_dbg_crop_affine: the affine crop kernel alone on ONE image whose planes are on the host, behind the staging of vp_infer_images_affine:
 * uint8 RGB crops [n, 256, 192, 3].  vp_dbg_decode_affine: the affine decode on heatmaps [n, k, 64, 48] and cs [n, 4] -> [n, k, 3] in frame pixels;
 * vp_dbg_decode_affine_flip: on the flip-test mode's interleaved [2 n, k, 64, 48] (vp_dbg_decode_flip's arguments). */
VP_API int vp_dbg_crop_affine(int32_t device_id, const vp_image* image, const float* cs, int32_t n, uint8_t* out);
VP_API int vp_dbg_decode_affine(int32_t device_id, const float* heatmaps, int32_t n, int32_t k, const float* cs, float* out);
VP_API int vp_dbg_decode_affine_flip(int32_t device_id, const float* heatmaps2, int32_t n, int32_t k, const int32_t* flip_pairs, int32_t n_pairs,
                                     int32_t shift_heatmap, const float* cs, float* out);

/* Person scores and OKS pose NMS on the device, the stage behind the boxes entries (the reference's vit_utils/post_processing/nms.py oks_iou / oks_nms /
 * soft_oks_nms with data_cfg's oks_thr, vis_thr, soft_nms; csrc/posenms.h states the arithmetic once for the kernel and the host taps).
 * A row is one person: d_kpts float32 [n, k, 3] (y, x, conf) in frame pixels (the d_out of a boxes entry), a box score at d_box_score + i * score_stride
 * (a detector's [n, 6] tensor passes in place as d_boxes + 4 with stride 6), a d_crop_params row {frame, x0, y0, cw, ch, ...} and d_status (may be NULL:
 * every row good; then a bad box's all-zero d_crop_params row counts as a person of area 0 on frame 0).
 *   area  = (double)cw * (double)ch.
 *   score = (float)(mean of conf over the joints with conf > vis_thr, 0 if none; fp64 in joint order) * (double)box_score); use_vis_thr = 0: every joint.
 *   oks(d | g) as nms.py:51-86: float32 dx, dy, dx*dx + dy*dy, then fp64 e = that / (2 sigma_j)^2 / ((a_g + a_d) / 2 + 2^-52) / 2 over the joints whose
 *           CANDIDATE conf > vis_thr (the reference's `list(vg > t) and list(vd > t)` is the second list), oks = (float)(sum exp(-e) / count), 0 without joints.
 *   Per frame: the live row with the highest score is picked (equal scores: the lower row; the reference's tie order is an argsort artefact) and gets the next
 *   rank; hard: every live row with oks > oks_thr (float32 compare) is suppressed; soft != 0: every live row's fp64 score *= exp(-oks^2 / oks_thr), at most
 *   max_dets picks, and a picked row's d_score is the score it was picked with (every other row keeps its instance score).
 * d_score float32 [n]; d_rank int32 [n]: the pick order within the row's frame from 0, -1 suppressed / not reached within max_dets / status != 0 / frame
 * outside [0, n_frames), -2 for every row of a frame with more than VP_NMS_MAX_PER_FRAME good rows (that frame is not processed; its rows keep their instance
 * score); d_count (may be NULL) int32 [n_frames]: rows kept per frame.  Rows of a frame may lie anywhere in the call; a frame may have none.
 * vp_pose_nms_stream only enqueues on caller_stream (one kernel, one workgroup per frame; the (2 sigma)^2 table travels by kernel argument): no synchronisation,
 * no copy from host memory, no allocation, none of the handle's buffers -- correct directly behind a boxes entry on the same stream.  cfg and sigmas are HOST memory.
 * VP_ERR_INVALID before anything is enqueued: a NULL required pointer with n > 0, k outside 1..VP_NMS_MAX_K, n_sigmas != k, a sigma that is not finite or <= 0,
 * oks_thr outside (0, 1], soft with max_dets < 1, n > 0 with n_frames < 1, score_stride < 1.  n = 0: VP_OK, only d_count is written (zeros).
 * vp_pose_nms: the synchronous twin on host pointers (upload, the same kernel, download).  Library builds that carry the stage define VP_HAS_POSE_NMS. */
#define VP_HAS_POSE_NMS 1
#define VP_NMS_MAX_PER_FRAME 1024
#define VP_NMS_MAX_K 256
typedef struct vp_pose_nms_cfg {
    float oks_thr;
    float vis_thr;
    int32_t use_vis_thr;
    int32_t soft;
    int32_t max_dets;
    int32_t n_sigmas;
    const float* sigmas;   /* host [n_sigmas] */
} vp_pose_nms_cfg;
VP_API int vp_pose_nms_stream(vp_handle h, const float* d_kpts, int32_t n, int32_t k, const float* d_box_score, int32_t score_stride,
                              const int32_t* d_crop_params, const int32_t* d_status, int32_t n_frames, const vp_pose_nms_cfg* cfg, float* d_score,
                              int32_t* d_rank, int32_t* d_count, void* caller_stream);
VP_API int vp_pose_nms(vp_handle h, const float* kpts, int32_t n, int32_t k, const float* box_score, int32_t score_stride, const int32_t* crop_params,
                       const int32_t* status, int32_t n_frames, const vp_pose_nms_cfg* cfg, float* score, int32_t* rank, int32_t* count);
/* HOST ONLY, no device needed: csrc/posenms.h run row by row on the host, the model the device is tested against (a test tap, never a fallback); the
 * refusals of vp_pose_nms_stream, the reason in vp_last_error(NULL). */
VP_API int vp_dbg_pose_nms_host(const float* kpts, int32_t n, int32_t k, const float* box_score, int32_t score_stride, const int32_t* crop_params,
                                const int32_t* status, int32_t n_frames, const vp_pose_nms_cfg* cfg, float* score, int32_t* rank, int32_t* count);
/* The pairwise tap: oks [n, n] float32, entry (g, d) = candidate d against pick g over all n rows (host pointers; no status, no frames; n <= 32768);
 * device_id = -1: on the host (the serial sum of csrc/posenms.h), no device needed; a device runs the NMS kernel's evaluation -- the terms of an entry spread over
 * the L lanes a frame of n members gets, added in joint order -- so n chooses the L under test (64 up to 4 rows, 16 at 16, 2 at 128, 1 beyond). */
VP_API int vp_dbg_pose_oks(int32_t device_id, const float* kpts, int32_t n, int32_t k, const int32_t* crop_params, const vp_pose_nms_cfg* cfg, float* oks);

/* The skeleton overlay on device frames, the stage behind a boxes entry and vp_pose_nms_stream (modelled on the reference's draw_points_and_skeleton,
 * vit_utils/visualization.py:360-481: opaque colours, no anti-aliasing; csrc/drawgeom.h states the arithmetic once for the kernels and the host tap).  The
 * rasterisation is this library's own integer one: parity against OpenCV's circle / line / rectangle is unpinned and not claimed.
 * A row is one person: d_kpts float32 [n, k, 3] (y, x, conf) in frame pixels, a frame index at d_frame_idx + i * frame_stride (column 0 of a [n, 9] crop-params
 * tensor passes in place with stride 9; a row whose index is outside [0, n_images) is not drawn), d_rank (may be NULL) int32 [n]: a row with rank < 0 is not drawn
 * (the NMS output passes as it is), d_ids (may be NULL: the row's index) int32 [n]: the reference's person_index, d_boxes (may be NULL: no outlines) float32
 * (x1, y1, x2, y2) at d_boxes + i * box_stride.
 *   A float v is usable iff -16384 < v < 16384 (never for NaN / inf); its pixel is (int)v.  A joint is visible iff conf > conf_thr (float32) and x, y are usable.
 *   joint: the disk |p - c|^2 <= r^2.  limb (a, b), both joints visible, thickness t: with d = b - a, q = p - a the pixels with 0 <= q.d <= |d|^2 and
 *   (q x d)^2 <= floor(t^2 |d|^2 / 4), plus the caps 4 |p - a|^2 <= t^2 and 4 |p - b|^2 <= t^2.  box, four usable values: the outline of t pixels per side, the
 *   outermost t / 2 of them outside the box.  All in int64, exact for frames of up to 8192 x 8192.
 *   Order: rows ascending; within a row box, limbs in table order, joints in joint order; a pixel shows the LAST primitive that covers it, whatever the launch shape.
 *   Colours: limbs and box limb_colors[id mod n_limb_colors], joint j point_colors[j mod n_point_colors] (mathematical mod).  NV12 frames: each colour once through
 *   the forward matrix of the frame's `matrix` (round(x 2^8) integers, csrc/drawgeom.h); Y per covered pixel, a chroma sample takes the (U, V) of the last
 *   primitive that covers any of its up-to-four pixels.  No byte outside a covered pixel or chroma sample is written, pitch padding included.
 * vp_draw_poses_stream only enqueues on caller_stream (two kernels per 32 frames of the table; limb table, palettes and style travel by kernel argument): no
 * synchronisation, no copy from host memory, no allocation -- correct directly behind a boxes entry and vp_pose_nms_stream on the same stream.  The primitive
 * records live in a workspace of the handle (VP_DRAW_MAX_RECORDS, allocated by vp_create): calls on one handle from different streams are the caller's to order.
 * `images` are DEVICE frames; vp_image's plane pointers are const, and this entry WRITES through them.  cfg and its tables are HOST memory.
 * VP_ERR_INVALID before anything is enqueued: a NULL images / d_kpts / d_frame_idx or n_images < 1 with n > 0, k outside 1..256, n_limbs outside
 * 0..VP_DRAW_MAX_LIMBS or a limb index >= k, colour counts outside 1..VP_DRAW_MAX_COLORS, a NULL table, conf_thr not finite, radius outside 0..64, thickness outside
 * 1..16, frame_stride < 1 (box_stride < 1 with boxes), n * (box + n_limbs + k) above VP_DRAW_MAX_RECORDS, and for every image of the table: no data, h or w outside
 * 1..8192, the image refusals of vp_dbg_image_plan, a plane that is not device memory of the handle's device inside one allocation.  n = 0: VP_OK, nothing enqueued.
 * vp_draw_poses: the synchronous twin on host pointers and host planes (upload, the same kernels, download).
 * vp_dbg_draw_host: HOST ONLY, no device needed: csrc/drawgeom.h pixel by pixel on host planes, the model the device is tested against (a test tap, never a
 * fallback); the same refusals, the reason in vp_last_error(NULL).  Library builds that carry the stage define VP_HAS_DRAW. */
#define VP_HAS_DRAW 1
#define VP_DRAW_MAX_LIMBS  256
#define VP_DRAW_MAX_COLORS 32
#define VP_DRAW_MAX_RECORDS 65536   /* primitive slots of one call: n * ((d_boxes != NULL) + n_limbs + k) */
typedef struct vp_draw_cfg {
    float   conf_thr;                       /* joints at or below are not drawn; the reference's 0.5 */
    int32_t radius, thickness;              /* radius 0: max(1, min(h, w) / 150) per frame */
    int32_t n_limbs;  const uint8_t* limbs; /* host [n_limbs, 2] joint indices < k */
    int32_t n_point_colors; const uint8_t* point_colors;  /* host [n, 3] RGB */
    int32_t n_limb_colors;  const uint8_t* limb_colors;   /* host [n, 3] RGB */
} vp_draw_cfg;
VP_API int vp_draw_poses_stream(vp_handle h, const vp_image* images, int32_t n_images, const float* d_kpts, int32_t n, int32_t k, const int32_t* d_frame_idx,
                                int32_t frame_stride, const int32_t* d_rank, const int32_t* d_ids, const float* d_boxes, int32_t box_stride,
                                const vp_draw_cfg* cfg, void* caller_stream);
VP_API int vp_draw_poses(vp_handle h, const vp_image* images, int32_t n_images, const float* kpts, int32_t n, int32_t k, const int32_t* frame_idx,
                         int32_t frame_stride, const int32_t* rank, const int32_t* ids, const float* boxes, int32_t box_stride, const vp_draw_cfg* cfg);
VP_API int vp_dbg_draw_host(const vp_image* images, int32_t n_images, const float* kpts, int32_t n, int32_t k, const int32_t* frame_idx, int32_t frame_stride,
                            const int32_t* rank, const int32_t* ids, const float* boxes, int32_t box_stride, const vp_draw_cfg* cfg);

/* Track-id and score tags on device frames, the stage IN FRONT of vp_draw_poses_stream (modelled on the reference's draw_bboxes, vit_utils/inference.py:19-38:
 * `#<id>: <score>` on a filled tag at the top-left corner of every tracked box; csrc/labelgeom.h states the arithmetic once for the kernels and the host taps).
 * The font is this library's own 5 x 7 bitmap font over 16 symbols (# 0-9 : . - space and one spare): parity against OpenCV's Hershey font is unpinned and not
 * claimed.  Off unless called.
 * A row is one person: d_boxes (REQUIRED) float32 (x1, y1, x2, y2) at d_boxes + i * box_stride, a frame index at d_frame_idx + i * frame_stride (a row whose index
 * is outside [0, n_images) gets no tag), d_rank (may be NULL) int32 [n]: no tag for rank < 0, d_ids (may be NULL: the row's index) int32 [n], d_scores (may be NULL)
 * float32 at d_scores + i * score_stride -- the rows of vp_tracker_update_stream pass in place: d_boxes = rows, box_stride = 6, d_scores = rows + 4, score_stride = 6.
 *   Gates: the four box values usable (-16384 < v < 16384, never NaN: an absent tracker row draws nothing); corners truncated, then ordered.
 *   Text: `#<id>` (int32 in decimal), and `: <score>` iff d_scores, cfg->show_score and -1000 < s < 1000; the score text equals printf-style "%.2f" of the exact
 *   binary value, ties to even (0.125 -> 0.12, 0.375 -> 0.38), the sign from the sign bit (-0.0 -> -0.00); integer arithmetic only.  At most 22 characters.
 *   Geometry (int32): scale s = cfg->scale in 1..8, 0 for max(1, min(h, w) / 400) of the row's frame capped at 8; with L characters the tag is the block
 *   [x1, x1 + s (6 L + 1)) x [by, by + 9 s), by = y1 - 9 s when that is >= 0, else y1 (inside the box); glyph c at (x1 + s + 6 s c, by + s), every font bit an
 *   s x s square; clipped to the frame, never shifted.
 *   Colours: background colors[id mod n_colors] (mathematical mod); ink cfg->ink, or with auto_ink black when 77 R + 150 G + 29 B >= 32768 for the background and
 *   white otherwise.  NV12 as vp_draw_poses_stream.  Order index of a primitive 2 * row + (ink ? 1 : 0): a pixel shows the covering primitive with the highest
 *   one, a chroma sample the highest among its up-to-four pixels.  No byte outside a covered pixel or chroma sample is written; every written byte once per call.
 * vp_draw_labels_stream only enqueues on caller_stream (two kernels per 32 frames of the table; font, palette and frame table travel by kernel argument): no
 * synchronisation, no copy from host memory, no allocation.  The records live in a workspace of the handle (VP_LABEL_MAX_ROWS, allocated by vp_create): calls on one
 * handle from different streams are the caller's to order.  `images` are DEVICE frames and this entry WRITES through their plane pointers.  cfg is HOST memory.
 * VP_ERR_INVALID before anything is enqueued: NULL cfg; n < 0 or n > VP_LABEL_MAX_ROWS; a NULL images / d_boxes / d_frame_idx or n_images < 1 with n > 0; scale
 * outside 0..8; n_colors outside 1..VP_DRAW_MAX_COLORS or a NULL table; a stride < 1 (score_stride with scores only); the per-image refusals of
 * vp_draw_poses_stream; a plane that is not device memory of the handle's device inside one allocation.  n = 0: VP_OK, nothing enqueued.
 * vp_draw_labels: the synchronous twin on host pointers and host planes (upload, the same kernels, download).
 * vp_dbg_draw_labels_host: HOST ONLY, no device needed: csrc/labelgeom.h on host planes, rows in order (a test tap, never a fallback); the same refusals, the reason
 * in vp_last_error(NULL).  vp_dbg_label_text: HOST ONLY, the text of a tag as characters (the spare symbol as '?'), NUL-terminated, out holds 25 bytes.
 * vp_dbg_label_glyph: HOST ONLY, the 35 bits of glyph `code` (bit 5 * row + col; 0 for a code outside 0..15).  Library builds that carry the stage define
 * VP_HAS_DRAW_LABELS. */
#define VP_HAS_DRAW_LABELS 1
#define VP_LABEL_MAX_ROWS 8192
typedef struct vp_label_cfg {
    int32_t scale;                          /* 1..8; 0: max(1, min(h, w) / 400) per frame, at most 8 */
    int32_t n_colors; const uint8_t* colors; /* host [n, 3] RGB: the background of a tag is colors[id mod n] */
    int32_t auto_ink;                       /* non-zero: black or white ink by the background's luma; 0: `ink` */
    uint8_t ink[3];                         /* RGB */
    int32_t show_score;                     /* 0: the id alone even when scores are given */
} vp_label_cfg;
VP_API int vp_draw_labels_stream(vp_handle h, const vp_image* images, int32_t n_images, const float* d_boxes, int32_t box_stride, int32_t n,
                                 const int32_t* d_frame_idx, int32_t frame_stride, const int32_t* d_rank, const int32_t* d_ids, const float* d_scores,
                                 int32_t score_stride, const vp_label_cfg* cfg, void* caller_stream);
VP_API int vp_draw_labels(vp_handle h, const vp_image* images, int32_t n_images, const float* boxes, int32_t box_stride, int32_t n, const int32_t* frame_idx,
                          int32_t frame_stride, const int32_t* rank, const int32_t* ids, const float* scores, int32_t score_stride, const vp_label_cfg* cfg);
VP_API int vp_dbg_draw_labels_host(const vp_image* images, int32_t n_images, const float* boxes, int32_t box_stride, int32_t n, const int32_t* frame_idx,
                                   int32_t frame_stride, const int32_t* rank, const int32_t* ids, const float* scores, int32_t score_stride,
                                   const vp_label_cfg* cfg);
VP_API int vp_dbg_label_text(int32_t id, int32_t has_score, float score, char* out);
VP_API uint64_t vp_dbg_label_glyph(int32_t code);

/* The collect stage, BEHIND vp_infer_boxes_stream, its NMS and the smoother: the persons a call keeps packed into ONE dense record table, so that one device-to-host
 * copy yields what the reference's inference() returns, `{id: keypoints}` per frame (csrc/collectgeom.h states the contract once for the kernels and the host tap,
 * easy_vitpose_amd/devcollect.py restates it in numpy).  Off unless called.
 * n rows, 0 <= n <= VP_COLLECT_MAX_ROWS, on n_frames in 1..VP_COLLECT_MAX_FRAMES frames; d_kpts float32 [n, k, 3], 1 <= k <= 133 (REQUIRED with n > 0).  Every
 * other input may be NULL: d_ids int32 [n] (NULL: a row's id is its ordinal among the rows of its own frame in call order -- every row with a valid frame index
 * counts, kept or not: the reference's range(len(bboxes))), d_frame int32 [n] (NULL: frame 0), d_rank int32 [n] (the NMS's rank), d_status int32 [n] (the boxes
 * entry's status), d_score float32 at d_score + i * score_stride (the NMS's score, or column 4 of the tracker's rows in place; NULL: 0.0), d_crop_params int32
 * [n, 9] (the boxes entry's rows {frame, x0, y0, cw, ch, ...}; NULL: a box of four zeros).
 *   Kept: 0 <= frame < n_frames, id >= 0 when ids are given (an absent tracker row has id -1), rank >= 0 when ranks are given, status == 0 when a status is given.
 *   Output, vp_collect_bytes(n_frames, k, max_records) bytes: a header int32 [n_frames + 1] = the kept rows of every frame and the TRUE total last, whatever
 *   max_records is, zero-padded to a multiple of 16 bytes; then records of S = 4 ceil((8 + 3 k) / 4) 4-byte words: id, frame, the row's index in the call (int32),
 *   score (float32), box int32 (x0, y0, x0 + cw, y0 + ch) -- the padded and clipped box the reference writes back into bboxes --, the row's 3 k keypoint words bit
 *   for bit (a NaN keeps its payload), zeros.  Records by frame ascending, then in call order: the order of the reference's dict for one frame and of its list of
 *   dicts for several.  The first min(total, max_records) records are written; no byte behind the last written record is touched; every written byte is written
 *   once per call.  The order is decided without atomics: the table is a pure function of the inputs.
 * vp_collect_stream only enqueues on caller_stream (two kernels; every input travels by kernel argument): no synchronisation, no copy from host memory, no
 * allocation.  The record index and the id of every row live in a workspace of the handle (2 VP_COLLECT_MAX_ROWS + VP_COLLECT_MAX_FRAMES int32, allocated by
 * vp_create): calls on one handle from different streams share it and are the caller's to order.
 * VP_ERR_INVALID before anything is enqueued: n, n_frames or k outside their ranges; max_records < 0; NULL d_kpts with n > 0; NULL d_out; score_stride < 1; a
 * d_out that is not 16-byte aligned.  n = 0 writes a zero header and nothing else.
 * vp_collect_bytes: the size of the table, -1 for n_frames or k outside their ranges or max_records < 0.
 * vp_collect: the synchronous twin on host pointers (upload, the same kernels, download of the header and of the written records only).
 * vp_dbg_collect_host: HOST ONLY, no device needed: csrc/collectgeom.h on host memory, rows in order (a test tap, never a fallback); the same refusals, the reason in
 * vp_last_error(NULL).  Library builds that carry the stage define VP_HAS_COLLECT. */
#define VP_HAS_COLLECT 1
#define VP_COLLECT_MAX_ROWS 8192
#define VP_COLLECT_MAX_FRAMES 64
VP_API int64_t vp_collect_bytes(int32_t n_frames, int32_t k, int32_t max_records);
VP_API int vp_collect_stream(vp_handle h, const float* d_kpts, int32_t n, int32_t k, const int32_t* d_ids, const int32_t* d_frame, const int32_t* d_rank,
                             const int32_t* d_status, const float* d_score, int32_t score_stride, const int32_t* d_crop_params, int32_t n_frames,
                             int32_t max_records, void* d_out, void* caller_stream);
VP_API int vp_collect(vp_handle h, const float* kpts, int32_t n, int32_t k, const int32_t* ids, const int32_t* frame, const int32_t* rank, const int32_t* status,
                      const float* score, int32_t score_stride, const int32_t* crop_params, int32_t n_frames, int32_t max_records, void* out);
VP_API int vp_dbg_collect_host(const float* kpts, int32_t n, int32_t k, const int32_t* ids, const int32_t* frame, const int32_t* rank, const int32_t* status,
                               const float* score, int32_t score_stride, const int32_t* crop_params, int32_t n_frames, int32_t max_records, void* out);

/* The box tracker on the device, the stage IN FRONT of a boxes entry: SORT as the reference's video path runs it (sort.py Sort.update behind inference.py:247-249;
 * csrc/sortgeom.h states the arithmetic once for the kernels and the host taps, easy_vitpose_amd/tracker.py is the Python twin).  A tracker object holds n_streams
 * independent SORT states (one per camera: the multi-frame shape of vp_infer_frames and of the NMS) in device memory of the handle's device; a stream holds at most
 * VP_TRACK_MAX live tracks and takes at most VP_TRACK_MAX detections per call.
 *   d_dets float32 rows (x1, y1, x2, y2, score) at d_dets + i * row_stride (a detector's [n, 6] tensor passes in place with stride 6); d_frame_idx int32 [n_dets]: the
 *   stream of every row (NULL: all rows are stream 0).  Rows of a stream keep their call order.  step_mask: bit s = stream s advances one frame in this call; a stream
 *   in the mask without a detection row steps with empty input (the detector-skipped frame: every listed track's PREDICTED box is reported), a stream outside the
 *   mask is untouched and its rows are ignored.  n_dets = 0 is legal: the coasting call.
 *   Per stream (fp64, nothing contracted, correctly rounded sqrt and division): predict every track (area guard x[6] + x[2] <= 0 -> x[6] = 0); tracks whose predicted
 *   box is not finite leave the list; IoU against the detections (a zero-area pair: 0); association as tracker.associate: where every row and column of iou > thr
 *   holds at most one entry those entries are the pairs, otherwise the exact rectangular linear-sum assignment that maximises the total IoU (shortest augmenting
 *   paths, fp64 duals, every loop bounded by the matrix sides); pairs with iou < thr are dropped; matched tracks take the Kalman update in Joseph form; the
 *   unmatched detections become new tracks in DETECTION-INDEX order (the reference's order depends on a tie-break inside its assignment solver: tracker.py), ids from
 *   1 per stream; a track is reported when time_since_update < 1 and (hit_streak >= min_hits or frame_count <= min_hits); tracks leave when
 *   time_since_update > max_age.
 *   Output: d_rows float32 [n_out, 6] (x1, y1, x2, y2, score, id), the fp64 values rounded once; d_ids, d_stream int32 [n_out]; streams ascending, within a stream
 *   the reference's order (reversed track list).  Rows beyond the total are "absent": box NaN, score 0, id -1, stream -1 -- vp_infer_boxes_stream gives such a row
 *   status 1, reads no frame and returns zeros, the NMS gives it rank -1.  So d_rows passes in place to vp_infer_boxes_stream (row_stride 6, d_stream as d_frame_idx)
 *   and to the NMS as d_rows + 4.  d_count int32 [n_streams + 1]: rows per stream, last = the true total, whatever n_out.  d_flags (may be NULL) int32 [n_streams]:
 *   1 detections beyond VP_TRACK_MAX ignored (the first in call order kept); 2 births dropped at VP_TRACK_MAX live tracks (the lowest detection indices kept);
 *   4 rows of this stream cut by n_out (a stream without rows behind the cut is not flagged); 8 a detection row of this stream that is not finite was skipped, or a row of the call names a stream outside the table (that
 *   is raised on every stepped stream).
 * vp_tracker_update_stream only enqueues on caller_stream (two kernels: one workgroup per stepped stream, then one workgroup that packs the rows; the configuration
 * travels by kernel argument): no synchronisation, no copy from host memory, no allocation, none of the handle's workspaces.  Calls on one tracker from different
 * streams are the caller's to order.  vp_tracker_reset_stream zeroes the state of the streams in the mask on caller_stream (ids restart at 1).
 * VP_ERR_INVALID before anything is enqueued: a NULL cfg / d_count, NULL d_dets with n_dets > 0, NULL d_rows / d_ids / d_stream with n_out > 0, row_stride < 5,
 * n_streams outside 1..VP_TRACK_MAX_STREAMS, max_age < 0, min_hits < 0, iou_threshold not in (0, 1), n_dets < 0, n_out < 0, a mask bit beyond n_streams.
 * vp_tracker_update: the synchronous twin on host pointers (upload, the same kernels, download).  vp_tracker_create: on the device of h, state zeroed; the tracker
 * must be destroyed before h.  Library builds that carry the stage define VP_HAS_TRACKER. */
#define VP_HAS_TRACKER 1
#define VP_TRACK_MAX 128
#define VP_TRACK_MAX_STREAMS 64
typedef struct vp_track_cfg {
    int32_t max_age, min_hits;
    float   iou_threshold;
    int32_t n_streams;
} vp_track_cfg;
typedef struct vp_tracker* vp_tracker_handle;
VP_API int vp_tracker_create(vp_handle h, const vp_track_cfg* cfg, vp_tracker_handle* out);
VP_API int vp_tracker_destroy(vp_tracker_handle t);
VP_API int vp_tracker_reset_stream(vp_tracker_handle t, uint64_t stream_mask, void* caller_stream);
VP_API int vp_tracker_update_stream(vp_tracker_handle t, const float* d_dets, int32_t row_stride, const int32_t* d_frame_idx, int32_t n_dets, uint64_t step_mask,
                                    float* d_rows, int32_t* d_ids, int32_t* d_stream, int32_t n_out, int32_t* d_count, int32_t* d_flags, void* caller_stream);
VP_API int vp_tracker_update(vp_tracker_handle t, const float* dets, int32_t row_stride, const int32_t* frame_idx, int32_t n_dets, uint64_t step_mask, float* rows,
                             int32_t* ids, int32_t* stream, int32_t n_out, int32_t* count, int32_t* flags);
/* The state as csrc/sortgeom.h lays it out (TrkStream [n_streams]; easy_vitpose_amd/devtracker.py STATE_DTYPE), for tests: its size, and a synchronous download
 * (it waits for the device first). */
VP_API int vp_tracker_state_bytes(int32_t n_streams, int64_t* bytes);
VP_API int vp_tracker_download_state(vp_tracker_handle t, void* out);
/* HOST ONLY, no device needed: csrc/sortgeom.h run serially on a host state blob of vp_tracker_state_bytes (zeroed = a new tracker), the model the device is tested
 * against (a test tap, never a fallback); the refusals of vp_tracker_create and vp_tracker_update_stream, the reason in vp_last_error(NULL). */
VP_API int vp_dbg_track_host(void* state, const vp_track_cfg* cfg, const float* dets, int32_t row_stride, const int32_t* frame_idx, int32_t n_dets, uint64_t step_mask,
                             float* rows, int32_t* ids, int32_t* stream, int32_t n_out, int32_t* count, int32_t* flags);
/* The association alone on iou [nd, nt] fp64 (host pointers, nd, nt <= VP_TRACK_MAX): trk_of_det [nd] = the track paired with every detection or -1, shortcut,
 * assignment and threshold filter included.  device_id = -1: on the host, no device needed; a device runs the tracker kernel's association (one column per lane). */
VP_API int vp_dbg_lsap(int32_t device_id, const double* iou, int32_t nd, int32_t nt, float thr, int32_t* trk_of_det);
/* vp_tracker_update_stream with the detection count in device memory: the rows of the call are the first min(*d_n_dets, n_dets_cap) (a negative count: none); rows
 * from there on are never read, so they may hold anything (NaN, streams outside the table) and raise no flag.  The detector stage's d_rows, d_image and
 * d_count + n_images pass in place.  The same kernels: vp_tracker_update_stream is the d_n_dets == NULL case, bit for bit.  VP_ERR_INVALID for a NULL d_n_dets
 * and for everything vp_tracker_update_stream refuses (n_dets_cap in the place of n_dets). */
VP_API int vp_tracker_update_counted_stream(vp_tracker_handle t, const float* d_dets, int32_t row_stride, const int32_t* d_frame_idx, int32_t n_dets_cap,
                                            const int32_t* d_n_dets, uint64_t step_mask, float* d_rows, int32_t* d_ids, int32_t* d_stream, int32_t n_out,
                                            int32_t* d_count, int32_t* d_flags, void* caller_stream);

/* The detector stage, IN FRONT of the tracker: a detector's raw head tensor, left in device memory by an engine on the same GPU, to the [n, 6] box rows every entry
 * above takes in place -- best-class pick, confidence threshold, class filter, greedy box NMS, letterbox undone (the reference's YOLOv8 post-processing behind
 * inference.py:240-241; csrc/detgeom.h states the arithmetic once for the kernels and the host tap).  The detector network itself is not this library's; the letterboxing of the frame
 * into its input is the letterbox stage below, whose undo table this stage takes as `images`.  Up to VP_DET_MAX_IMAGES images per call; the image index is the
 * tracker's stream.  Everything is float32, nothing contracted, division correctly rounded.
 *   d_pred: the head, contiguous, float32 (VP_DET_F32) or float16 (VP_DET_F16, widened exactly); layout 0 = [n_images, 4 + nc, A] (YOLOv8's export), layout 1 =
 *   [n_images, A, 4 + nc].  Channels 0..3 = (cx, cy, w, h) in detector-input pixels, channels 4.. = class scores, already sigmoided.
 *   Per anchor: best = the first class of the strictly largest score (a NaN never wins; all NaN: no candidate).  The anchor is a CANDIDATE iff score > conf_thr,
 *   bit `best` of class_mask is set (the filter comes after the arg-max over ALL classes, as in ultralytics' non_max_suppression: a box that a masked class
 *   out-scores is no candidate) and cx, cy, w, h are finite; one that passes score and class with a box that is not finite is skipped and raises flag 8.
 *   Box: x1 = cx - w * 0.5f, x2 = cx + w * 0.5f, likewise y.  Order: score descending, equal scores by anchor ascending.
 *   Greedy NMS on those input-space boxes: side = (x2 - x1) + extent, area = side_x * side_y, iw = max(0, (min(x2a, x2b) - max(x1a, x1b)) + extent), likewise ih,
 *   iou = iw * ih / ((area_a + area_b) - iw * ih).  Walking the order, a live candidate is picked and suppresses every later live b with !(iou <= iou_thr) (the
 *   reference's keep rule `ovr <= thr`: a NaN suppresses); with agnostic = 0 only candidates of the same class suppress each other (no coordinate offset).  At most
 *   max_det picks.  extent = 0: the continuous convention (ultralytics, torchvision), 1: the pixel convention of the reference's post_processing/nms.py.
 *   The picks go to frame pixels: v = (v - pad) / gain, then min(max(v, 0), frame side), per image from the host table `images`.
 *   An image with more than VP_DET_MAX_CAND candidates is not processed: zero rows and flag 1 (so the result never depends on the order workgroups run in).
 *   Output: d_rows float32 [n_out, 6] = (x1, y1, x2, y2, score, class); d_image, d_anchor int32 [n_out]; images ascending, pick order within an image.  Rows beyond
 *   the total are "absent" as the tracker's: box NaN, score 0, class -1, image -1, anchor -1.  d_count int32 [n_images + 1]: rows per image, last = the true total
 *   whatever n_out.  d_flags (may be NULL) int32 [n_images]: 1 more than VP_DET_MAX_CAND candidates; 4 rows of this image cut by n_out; 8 a box that is not finite
 *   was skipped.
 * vp_detect_stream only enqueues on caller_stream (three kernels: the scan over anchor tiles x images, the NMS with one workgroup per image, a pack kernel with one thread per
 * output row; configuration and image table travel by kernel argument; the NMS kernel re-zeroes the counters, so back-to-back calls and captured graphs work): no
 * synchronisation, no copy from host memory, no allocation -- the detector object owns the candidate workspace.  Calls on one detector from different streams are the
 * caller's to order.  n_images = 0 is legal.
 * VP_ERR_INVALID before anything is enqueued: a NULL cfg / d_count, NULL d_pred / images with n_images > 0, NULL d_rows / d_image / d_anchor with n_out > 0, nc
 * outside 1..VP_DET_MAX_CLASSES, max_anchors outside 1..2^20, max_images outside 1..VP_DET_MAX_IMAGES, an unknown dtype or layout, conf_thr not finite or < 0,
 * iou_thr outside [0, 1], extent not finite or < 0, agnostic not 0 / 1, max_det outside 1..VP_DET_MAX_DET, a class_mask without a class below nc, A outside
 * 1..max_anchors, n_images outside 0..max_images, n_out < 0, d_pred not aligned to its element, an image whose gain is not finite and > 0, whose pad is not
 * finite or whose frame size is not finite and >= 0.
 * vp_detect: the synchronous twin on host pointers (upload, the same kernels, download).  vp_detector_create: on the device of h; the detector must be destroyed
 * before h.  Library builds that carry the stage define VP_HAS_DETECT. */
#define VP_HAS_DETECT 1
#define VP_DET_MAX_IMAGES 64
#define VP_DET_MAX_CLASSES 256
#define VP_DET_MAX_CAND 2048
#define VP_DET_MAX_DET 1024
#define VP_DET_F32 0
#define VP_DET_F16 1
typedef struct vp_det_cfg {
    int32_t  nc, max_anchors, max_images, dtype, layout;
    float    conf_thr, iou_thr, extent;
    int32_t  agnostic, max_det;
    uint32_t class_mask[8];   /* bit c of word c / 32: class c passes */
} vp_det_cfg;
typedef struct vp_det_image {
    float gain, pad_x, pad_y, frame_w, frame_h;
} vp_det_image;
typedef struct vp_detector* vp_detector_handle;
VP_API int vp_detector_create(vp_handle h, const vp_det_cfg* cfg, vp_detector_handle* out);
VP_API int vp_detector_destroy(vp_detector_handle d);
VP_API int vp_detect_stream(vp_detector_handle d, const void* d_pred, int32_t A, const vp_det_image* images, int32_t n_images, float* d_rows, int32_t* d_image,
                            int32_t* d_anchor, int32_t n_out, int32_t* d_count, int32_t* d_flags, void* caller_stream);
VP_API int vp_detect(vp_detector_handle d, const void* pred, int32_t A, const vp_det_image* images, int32_t n_images, float* rows, int32_t* image, int32_t* anchor,
                     int32_t n_out, int32_t* count, int32_t* flags);
/* HOST ONLY, no device needed: csrc/detgeom.h run serially, the model the device is tested against (a test tap, never a fallback); the refusals of
 * vp_detector_create and vp_detect_stream, the reason in vp_last_error(NULL). */
VP_API int vp_dbg_detect_host(const vp_det_cfg* cfg, const void* pred, int32_t A, const vp_det_image* images, int32_t n_images, float* rows, int32_t* image,
                              int32_t* anchor, int32_t n_out, int32_t* count, int32_t* flags);

/* The letterbox stage, IN FRONT of the detector network: frames in the layout their producer holds them (vp_image: NV12 decoder surfaces, BGR24 / RGB24 buffers,
 * pitched) to the detector's input tensor in device memory -- resize, pad, colour conversion, normalisation and transpose in one kernel -- together with the
 * vp_det_image table vp_detect_stream takes to undo it.  csrc/lbgeom.h states the arithmetic once for the kernel and the host tap; the detector network itself stays
 * third-party.  Up to VP_LB_MAX_IMAGES frames per call, which may differ in size, format and matrix; image i fills slice i of the tensor.
 *   Geometry (host, doubles; ultralytics' LetterBox(new_shape = (in_h, in_w), auto = False, scaleFill = False, center = True) on a frame of (h, w)):
 *   r = min(in_h / h, in_w / w), with scaleup = 0 r = min(r, 1.0); new_w = round(w r), new_h = round(h r) (round half to even on the double: nearbyint);
 *   left = round((in_w - new_w) / 2 - 0.1), top = round((in_h - new_h) / 2 - 0.1); the right and bottom pads are what remains.
 *   Pixels, in this order: every source pixel is converted to RGB8 (the image entries' definition above: NV12 with its matrix, chroma replicated; BGR swapped).  The
 *   h x w RGB8 image is resized to new_h x new_w as OpenCV's 8-bit cv2.resize(INTER_LINEAR) does (the crop kernel's restatement, easy_vitpose_amd/cropprep.py
 *   resize_linear_u8; parity against the OpenCV and ultralytics binaries is unpinned): scale = 1.0 / ((double)new / (double)src) per axis; for output index d
 *   f = (float)((d + 0.5) scale - 0.5) with product and difference in double, s = floor(f), f -= s, (f, s) = (0, 0) where s < 0 and (0, src - 1) where s >= src - 1,
 *   taps s and min(s + 1, src - 1) with weights a1 = rint(f 2048), a0 = rint((1 - f) 2048) in float32; r = p(s) a0 + p(s + 1) a1 along x in int32, then
 *   (((ay0 (r0 >> 4)) >> 16) + ((ay1 (r1 >> 4)) >> 16) + 2) >> 2 along y.  Where both scales are exactly 2.0 the result is the 2 x 2 box average (p00 + p01 + p10 +
 *   p11 + 2) >> 2; where new_h x new_w equals h x w the frame is copied.  The result lies at rows [top, top + new_h), columns [left, left + new_w); every other
 *   element is pad_value in all three channels.
 *   Output: order 0 = R, G, B channels (ultralytics' model input), 1 = B, G, R; layout 0 = [n, 3, in_h, in_w] (NCHW), 1 = [n, in_h, in_w, 3] (NHWC); dtype
 *   VP_LB_F32 = (float)v / 255.0f (division correctly rounded), VP_LB_F16 = that float rounded to nearest-even fp16 (what `im.half() / 255` gives), VP_LB_U8 = the
 *   byte v itself, for engines that normalise inside the model.
 *   det (host, may be NULL) [n_images]: the row of vp_detect_stream's `images` table per frame.  Where r was not clamped it is ultralytics' scale_boxes convention
 *   (easy_vitpose_amd/devdetect.py letterbox_params): gain = (float)min(in_h / h, in_w / w), pad_x = round((in_w - w gain) / 2 - 0.1), pad_y likewise -- from
 *   the UNROUNDED scaled size -- and frame_w = w, frame_h = h; where scaleup = 0 clamped r it is (1.0, left, top, w, h).  placement (host, may be NULL) int32
 *   [n_images, 4] = (left, top, new_w, new_h): where the pixels really lie.  The two are ultralytics' own conventions and differ by one pixel of pad for some sizes
 *   (5 x 7 into 640 x 640: top 91, pad_y 91; 1 x 6: top 266, pad_y 267): det is what undoes a detector's boxes the way ultralytics does, placement is the truth
 *   about the tensor.
 * vp_letterbox_stream only enqueues on caller_stream: one launch per 32 frames (the image records -- plane pointers, pitches, size, format, matrix, placement,
 *   scales -- travel by kernel argument), a workgroup per output row: adjacent lanes fetch adjacent pixels into LDS, then a lane stores a run of 16 output bytes per
 *   channel (8 fp16, 4 fp32, 16 u8 adjacent x); rows and pixels in the pad store the constant without a fetch; a d_out that is not 16-byte aligned or an in_w that is
 *   no multiple of the run takes element stores with the same values.  No synchronisation, no copy from host memory, no allocation, none of the handle's workspaces: it works under graph capture and back to back.  The
 *   planes are read in place; every plane is checked first to be device memory of the handle's device with (plane rows - 1) * pitch + row bytes inside one allocation.
 *   n_images = 0 is legal and enqueues nothing.  The handle needs no weights.
 * vp_letterbox: the synchronous twin, planes and tensor in host memory (upload at the caller's pitch, the same kernel, download).  vp_letterbox_plan: HOST ONLY, no
 *   device needed: det, placement and every refusal below that needs no device; it reads sizes and layout only (plane[0] may be NULL there).
 * VP_ERR_INVALID before anything is enqueued, the reason in vp_last_error (of the handle; vp_last_error(NULL) for the host-only entries): a NULL cfg, in_h / in_w
 *   outside 1..8192, an unknown dtype / layout / order, pad_value outside 0..255, scaleup not 0 / 1, n_images outside 0..VP_LB_MAX_IMAGES, NULL images or NULL
 *   output with n_images > 0, an output not aligned to its element, a frame with h or w < 1, the image refusals of vp_dbg_image_plan (an unknown format or matrix,
 *   a negative pitch, a pitch below the row bytes, NV12 with a NULL plane[1]), a NULL plane[0], a frame whose new_w or new_h comes out 0 (1280 x 1 into 640 x 640),
 *   a device plane that fails the allocation check.  A refused call leaves det and placement as they were.  Library builds that carry the stage define VP_HAS_LETTERBOX. */
#define VP_HAS_LETTERBOX 1
#define VP_LB_MAX_IMAGES 64
#define VP_LB_F32 0
#define VP_LB_F16 1
#define VP_LB_U8  2
typedef struct vp_letterbox_cfg {
    int32_t in_h, in_w;     /* the detector's input size, 1..8192 each */
    int32_t dtype;          /* VP_LB_* */
    int32_t layout;         /* 0 NCHW, 1 NHWC */
    int32_t order;          /* 0 RGB, 1 BGR */
    int32_t pad_value;      /* 0..255; ultralytics pads with 114 */
    int32_t scaleup;        /* 0: never enlarge a frame (r = min(r, 1)) */
} vp_letterbox_cfg;   /* 28 bytes */
VP_API int vp_letterbox_plan(const vp_letterbox_cfg* cfg, const vp_image* images, int32_t n_images, vp_det_image* det, int32_t* placement);
VP_API int vp_letterbox_stream(vp_handle h, const vp_letterbox_cfg* cfg, const vp_image* images, int32_t n_images, void* d_out, vp_det_image* det,
                               int32_t* placement, void* caller_stream);
VP_API int vp_letterbox(vp_handle h, const vp_letterbox_cfg* cfg, const vp_image* images, int32_t n_images, void* out, vp_det_image* det, int32_t* placement);
/* HOST ONLY, no device needed: csrc/lbgeom.h run serially on host planes, the model the device is tested against (a test tap, never a fallback); the refusals of
 * vp_letterbox, the reason in vp_last_error(NULL). */
VP_API int vp_dbg_letterbox_host(const vp_letterbox_cfg* cfg, const vp_image* images, int32_t n_images, void* out, vp_det_image* det, int32_t* placement);

/* The orient stage, IN FRONT of the letterbox stage: frames as a decoder or a capture device leaves them (a landscape surface plus a rotation tag, a mirrored
 * webcam, a ceiling camera) made upright on the device, so that every later stage -- letterbox, the frames and boxes entries, the overlays -- sees an upright
 * frame.  A pure permutation of bytes (csrc/orientgeom.h states it once for the kernel and the host tap): equal means equal bytes.  Up to VP_ORIENT_MAX_IMAGES
 * frames per call, which may differ in size, format, matrix and code.
 *   codes: HOST int32 [n], the EXIF orientation values: what the output is in terms of the source plane a of h x w elements
 *     VP_ORIENT_IDENTITY 1  a (a copy; compacts a pitched view)      h x w      VP_ORIENT_TRANSPOSE  5  a.T                              w x h
 *     VP_ORIENT_MIRROR   2  a[:, ::-1]                               h x w      VP_ORIENT_CW90       6  out[i, j] = a[h - 1 - j, i]      w x h  (90 degrees clockwise)
 *     VP_ORIENT_ROT180   3  a[::-1, ::-1]                            h x w      VP_ORIENT_TRANSVERSE 7  out[i, j] = a[h - 1 - j, w - 1 - i]  w x h
 *     VP_ORIENT_FLIP     4  a[::-1, :]                               h x w      VP_ORIENT_CCW90      8  out[i, j] = a[j, w - 1 - i]      w x h  (90 degrees counter-clockwise)
 *   An element is one byte of the Y plane, the two-byte U,V pair of the NV12 chroma plane (pair order kept), the three-byte pixel of RGB24 / BGR24 (channel order
 *   kept).  NV12: the Y plane is oriented with (h, w), the UV plane with the same code on (ceil(h / 2), ceil(w / 2)); that keeps the chroma rule (pixel (y, x)
 *   reads pair (y >> 1, x >> 1)) exactly when every reversed axis has even length, so an NV12 frame with an odd extent along an axis the code reverses is refused
 *   (codes 1 and 5 take any size).  Then to_rgb(orient(f)) == orient(to_rgb(f)), byte for byte.
 *   src, dst: HOST tables of n vp_image; dst[i] is the layout vp_orient_plan gives (h, w swapped by codes 5..8; format and matrix the source's; any pitch >= the row
 *   bytes, so a destination may be an ROI of a larger buffer).  vp_image's plane pointers are const, and the entries below WRITE through dst's.  No byte outside
 *   [row start, row start + row bytes) of a destination row is written or read-modify-written: the gap bytes of a pitched destination stay as they were.
 * vp_orient_plan: HOST ONLY, no device.  Fills dst[i].h, w, format, matrix; keeps a non-zero dst[i].pitch[p] after checking it, else writes the tight pitch (0 for
 *   an absent plane); leaves the plane pointers alone; plane_bytes [n, 2] (may be NULL) = (rows - 1) pitch + row bytes of each plane, 0 for an absent one.
 * vp_orient_stream only enqueues on caller_stream: one launch per 32 frames (the frame records travel by kernel argument), no atomics, no synchronisation, no host
 *   copy, no allocation, none of the handle's workspaces, so it runs under graph capture, back to back, and beside any other entry of the handle.  The handle needs
 *   no weights.  n = 0 is legal and enqueues nothing.
 * vp_orient: the synchronous twin, planes of both tables in host memory (upload at the caller's pitch, the same kernel, download of the row bytes of each
 *   destination row only).
 * VP_ERR_INVALID, before anything is enqueued and with the reason, naming the frame, in vp_last_error: NULL tables with n > 0, n outside 0..VP_ORIENT_MAX_IMAGES, a
 *   code outside 1..8, the image refusals of vp_dbg_image_plan, h or w < 1, a NULL plane, a dst entry whose h / w / format / matrix differ from the plan's, a dst pitch
 *   below its row bytes, the NV12 odd-axis case above, any overlap between a destination plane's byte range (first byte to last) and any source plane's or any other
 *   destination plane's of the call (there is no in-place orientation), a device plane, source or destination, that fails the handle's allocation check.  A refused
 *   call writes nothing.  Library builds that carry the stage define VP_HAS_ORIENT. */
#define VP_HAS_ORIENT 1
#define VP_ORIENT_MAX_IMAGES 64
#define VP_ORIENT_IDENTITY   1
#define VP_ORIENT_MIRROR     2
#define VP_ORIENT_ROT180     3
#define VP_ORIENT_FLIP       4
#define VP_ORIENT_TRANSPOSE  5
#define VP_ORIENT_CW90       6
#define VP_ORIENT_TRANSVERSE 7
#define VP_ORIENT_CCW90      8
VP_API int vp_orient_plan(const vp_image* src, const int32_t* codes, int32_t n, vp_image* dst, int64_t* plane_bytes);
VP_API int vp_orient_stream(vp_handle h, const vp_image* src, const int32_t* codes, const vp_image* dst, int32_t n, void* caller_stream);
VP_API int vp_orient(vp_handle h, const vp_image* src, const int32_t* codes, const vp_image* dst, int32_t n);
/* HOST ONLY, no device needed: csrc/orientgeom.h run serially on host planes, the model the device is tested against (a test tap, never a fallback); the refusals of
 * vp_orient, the reason in vp_last_error(NULL). */
VP_API int vp_dbg_orient_host(const vp_image* src, const int32_t* codes, const vp_image* dst, int32_t n);

/* Keypoint smoothing on the device, the stage BEHIND a boxes entry (and its NMS) and in front of vp_draw_poses_stream: the One-Euro filter of the reference's
 * post_processing/one_euro_filter.py in its fixed-rate mode, one filter per (stream, track id) (csrc/eurogeom.h states the arithmetic once for the kernels and the
 * host tap, easy_vitpose_amd/smooth.py is the numpy twin).  A smoother object holds n_streams tables of VP_SMOOTH_SLOTS slots for n_joints joints in device memory
 * of the handle's device: per slot an id, last_seen and 2 n_joints coordinate states (x_prev, dx_prev fp64, a fresh byte), per stream a frame_count.
 *   d_kpts float32 [n, n_joints, 3] rows of (y, x, conf); d_ids int32 [n] (the tracker's d_ids); d_stream int32 [n] (NULL: all rows are stream 0); d_rank int32 [n]
 *   (NULL: none; the NMS's rank); t_e HOST double [n_streams] (NULL: 1.0 each), copied into the kernel arguments; d_out float32 [n, n_joints, 3], may be d_kpts.
 *   Per stream s in step_mask, in this order: (1) frame_count += 1.  (2) slots with frame_count - last_seen > max_age + 1 become free (last_seen = the frame_count
 *   of the call that last updated the slot: a slot survives max_age stepped calls without a row).  (3) the rows of s in call order with id >= 0, rank >= 0 where
 *   a rank is given, and every y and x finite are ACTIVE.  Taken in call order: (4) an active row whose id owns a slot that no earlier row of this call touched is
 *   UPDATED with t_e[s] * (frame_count - last_seen) -- a track that skipped frames is filtered over the gap -- and last_seen = frame_count; (5) an active row whose
 *   id owns no slot is BORN into the lowest free slot (x_prev = x, dx_prev = 0, fresh; returned unchanged, nothing masked).  (6) every other row is copied through
 *   bit for bit and touches no state: id < 0 or a stream outside the table (the tracker's absent rows), rows of streams not in step_mask, rows that are not
 *   active, a row whose id an earlier row of this call already updated or bore (the first in call order wins), a birth that finds no free slot.
 *   The update of a coordinate (fp64, nothing contracted, division correctly rounded), x the float32 input, conf never touched:
 *     d = fresh ? (double)((float)x - (float)x_prev) : (double)x - x_prev;  dx = d / t_e;  r = (2 pi d_cutoff) t_e;  a_d = r / (r + 1);
 *     dx_hat = a_d dx + (1 - a_d) dx_prev;  cutoff = min_cutoff + beta |dx_hat|;  r = (2 pi cutoff) t_e;  a = r / (r + 1);  x_hat = a x + (1 - a) x_prev;
 *     x_hat = -10 where x <= 0;  x_prev = x_hat, dx_prev = dx_hat, fresh cleared;  the output is (float)x_hat.
 *   missing = 0: exactly that (the reference: after a masked sample the filter blends away from -10).  missing = 1 (restart): a coordinate whose x_prev <= 0 takes
 *   x_hat = x (-10 where x <= 0), dx_hat = 0 and is fresh again.
 *   d_flags (may be NULL) int32 [n_streams], 0 for a stream outside step_mask: 1 a row with an id already seen in this call was passed through; 2 a birth was
 *   dropped because the table is full; 8 an active-looking row of this stream (id >= 0, rank >= 0) that is not finite was skipped, or a row with id >= 0 names a
 *   stream outside the table (that is raised on every stepped stream).
 * vp_smooth_update_stream only enqueues on caller_stream (two kernels: one workgroup per stepped stream that ages, matches and bears, then one thread per row and
 * joint that filters; the configuration and t_e travel by kernel argument): no synchronisation, no copy from host memory, no allocation, none of the handle's
 * workspaces.  Calls on one smoother from different streams are the caller's to order.  vp_smoother_reset_stream zeroes the tables of the streams in the mask on
 * caller_stream.  n = 0 with a non-zero mask is legal: it ages the streams.
 * VP_ERR_INVALID before anything is enqueued: a NULL cfg, NULL d_kpts / d_ids / d_out with n > 0, n < 0 or n > max_rows, n_streams outside
 * 1..VP_TRACK_MAX_STREAMS, n_joints outside 1..1024, max_rows outside 1..VP_SMOOTH_MAX_ROWS, max_age < 0, min_cutoff / d_cutoff / any t_e not finite or <= 0, beta
 * not finite or < 0, missing not 0 or 1, a mask bit beyond n_streams.
 * vp_smooth_update: the synchronous twin on host pointers (upload, the same kernels, download).  vp_smoother_create: on the device of h, state zeroed (zeroed =
 * new); the smoother must be destroyed before h.  Library builds that carry the stage define VP_HAS_SMOOTHER. */
#define VP_HAS_SMOOTHER 1
#define VP_SMOOTH_SLOTS 128
#define VP_SMOOTH_MAX_ROWS 65536
typedef struct vp_smooth_cfg {
    double  min_cutoff, beta, d_cutoff;
    int32_t max_age, n_streams, n_joints, max_rows, missing;
} vp_smooth_cfg;
typedef struct vp_smoother* vp_smoother_handle;
VP_API int vp_smoother_create(vp_handle h, const vp_smooth_cfg* cfg, vp_smoother_handle* out);
VP_API int vp_smoother_destroy(vp_smoother_handle s);
VP_API int vp_smoother_reset_stream(vp_smoother_handle s, uint64_t stream_mask, void* caller_stream);
VP_API int vp_smooth_update_stream(vp_smoother_handle s, const float* d_kpts, const int32_t* d_ids, const int32_t* d_stream, const int32_t* d_rank, int32_t n,
                                   uint64_t step_mask, const double* t_e, float* d_out, int32_t* d_flags, void* caller_stream);
VP_API int vp_smooth_update(vp_smoother_handle s, const float* kpts, const int32_t* ids, const int32_t* stream, const int32_t* rank, int32_t n, uint64_t step_mask,
                            const double* t_e, float* out, int32_t* flags);
/* The state as csrc/eurogeom.h lays it out, for tests: n_streams blobs of  int32 frame_count, pad[3] | int32 id[128] | int32 last_seen[128] (0 = free) |
 * double x_prev[128][n_joints][2] | double dx_prev[128][n_joints][2] | uint8 fresh[128][n_joints][2]  (the pair = (y, x); easy_vitpose_amd/devsmooth.py
 * state_dtype); its size, and a synchronous download (it waits for the device first). */
VP_API int vp_smoother_state_bytes(const vp_smooth_cfg* cfg, int64_t* bytes);
VP_API int vp_smoother_download_state(vp_smoother_handle s, void* out);
/* HOST ONLY, no device needed: csrc/eurogeom.h run serially on a host state blob of vp_smoother_state_bytes (zeroed = a new smoother), the model the device is
 * tested against (a test tap, never a fallback); the refusals of vp_smoother_create and vp_smooth_update_stream, the reason in vp_last_error(NULL). */
VP_API int vp_dbg_smooth_host(void* state, const vp_smooth_cfg* cfg, const float* kpts, const int32_t* ids, const int32_t* stream, const int32_t* rank, int32_t n,
                              uint64_t step_mask, const double* t_e, float* out, int32_t* flags);

/* Accuracy metrics against ground truth on the device: an ACCUMULATING stage with the life cycle of the tracker and the smoother.  An evaluator object holds the
 * counts and sums of PCK (up to 8 thresholds), AUC, EPE, NME and OKS recall in device memory of the handle's device; every update adds the rows of one call to
 * them on the caller's stream and the state is read once at the end.  csrc/metricsgeom.h states the arithmetic (the reference's vit_utils/top_down_eval.py
 * _calc_distances / keypoint_pck_accuracy / keypoint_auc / keypoint_nme / keypoint_epe and post_processing/nms.py oks_iou as "ground truth against detected") and
 * the summation order once for the kernels and the host tap; easy_vitpose_amd/devmetrics.py holds the numpy twin and finish(), which turns a state into figures.
 *   d_pred float32 [n, n_joints, 3] rows of (y, x, conf); d_gt float32 [n, n_joints, 3] rows of (y, x, v); 0 <= n <= VP_METRICS_MAX_ROWS, n_joints in
 *   1..VP_NMS_MAX_K.  Optional, each may be NULL: d_norm float32 [n, 2] in (y, x) order (NULL: 1.0 both); d_area float32 [n] (NULL: no OKS for this call); d_rank
 *   int32 [n] (the row counts iff rank >= 0: the NMS's rank or the tracker's ids as they are); d_set int32 [n] with set_value (the row counts iff equal: the
 *   per-crop dataset index of a ViTPose+ call, one evaluator per dataset).  A COUNTED row passes both filters.
 *   Per joint of a counted row (float32, every operation rounded on its own): visible = v > vis_thr; dy = py - gy, dx = px - gx; the normalised distance
 *   qn = sqrtf((dy / n_y)^2 + (dx / n_x)^2) with a normaliser component <= 0 replaced by 1e6 and the whole row left out of this family when a component == 0; the
 *   pixel distance q1 = sqrtf(dy^2 + dx^2); the AUC distance qa = (float)sqrt(((double)dy / auc_norm)^2 + ((double)dx / auc_norm)^2).  valid_norm / valid_px
 *   count the visible joints (of rows not left out / of every counted row); pck_hits[t] += qn < pck_thr[t]; auc_hits[s] += qa < (float)((double)s / auc_steps)
 *   (strict); sum_norm += qn, sum_px += q1 in fp64.  DEVIATION from the reference: a non-finite distance is valid and never hits, but is left out of its sum and
 *   counted in `nonfinite`; the finisher then reports NaN for EPE / NME where the reference would report inf or NaN.
 *   OKS of a counted row (use_oks, d_area given, the area finite and > 0, at least one visible joint): csrc/posenms.h's terms over the visible joints in joint order
 *   with both areas = area; oks_rows += 1, oks_hits[t] += oks >= (float)(0.5 + 0.05 t) for t = 0..9, oks_sum += oks; a non-finite oks bumps `nonfinite` instead.
 *   It is the share of instances recovered at OKS t with one candidate per instance, NOT COCO AP.
 *   Summation order, part of the contract: rows form blocks of 64; a block's partial is the balanced binary tree over its 64 rows in row order (a row that does
 *   not contribute gives +0.0); a call's sum is ((0.0 + P(0)) + P(1)) + ... in ascending block order; the state takes state + call_sum.  The state is therefore a
 *   pure function of the inputs and the sequence of calls, bit for bit.
 *   State blob (vp_metrics_state_bytes = 8 (24 + n_joints (4 + n_pck + auc_steps)); zeroed = new), 8-byte words: int64 calls, rows, counted, nonfinite, oks_rows,
 *   0, 0, 0 | int64 oks_hits[10], double oks_sum, 0 x 5 | int64 valid_norm[K] | int64 valid_px[K] | double sum_norm[K] | double sum_px[K] | int64
 *   pck_hits[n_pck][K] | int64 auc_hits[auc_steps][K].
 *   Optional per-call outputs, every element written once per call: d_dist float32 [n, n_joints] = qn, or -1 where the joint is not in valid_norm; d_oks float32
 *   [n] = oks, or -1 where none.
 * vp_metrics_update_stream only enqueues on caller_stream (two kernels: one workgroup per 64 rows writes block partials into a workspace the evaluator owns, one
 * workgroup adds them into the state; n = 0 is legal and counts a call): no synchronisation, no host copy, no allocation, no atomics.  Calls on one evaluator from
 * different streams are the caller's to order.  vp_metrics_reset_stream zeroes the state on caller_stream; vp_metrics_snapshot_stream copies it to d_out (device,
 * vp_metrics_state_bytes) on caller_stream, so that a pipeline reads it without stopping.  vp_metrics_update: the synchronous twin on host pointers (upload, the same
 * kernels, download).  vp_metrics_create: on the device of h, state zeroed; sigmas = HOST float32 [n_joints] (required with use_oks, else may be NULL); the evaluator
 * must be destroyed before h.  vp_metrics_download_state waits for the device first.
 * VP_ERR_INVALID before anything is enqueued, the reason in vp_last_error: a NULL cfg, NULL d_pred / d_gt with n > 0, n outside 0..VP_METRICS_MAX_ROWS, n_joints
 * outside 1..VP_NMS_MAX_K, n_pck outside 0..8, auc_steps outside 0..32, a pck_thr in use or vis_thr not finite, auc_norm not finite or <= 0 with auc_steps > 0,
 * use_oks without sigmas or with a sigma not finite or <= 0, a NULL snapshot destination.  Library builds that carry the stage define VP_HAS_METRICS. */
#define VP_HAS_METRICS 1
#define VP_METRICS_MAX_ROWS 8192
typedef struct vp_metrics_cfg {
    double  auc_norm;
    float   pck_thr[8];
    float   vis_thr;
    int32_t n_joints, n_pck, auc_steps, use_oks;
    int32_t reserved;
} vp_metrics_cfg;
typedef struct vp_metrics* vp_metrics_handle;
VP_API int vp_metrics_create(vp_handle h, const vp_metrics_cfg* cfg, const float* sigmas, vp_metrics_handle* out);
VP_API int vp_metrics_destroy(vp_metrics_handle m);
VP_API int vp_metrics_reset_stream(vp_metrics_handle m, void* caller_stream);
VP_API int vp_metrics_update_stream(vp_metrics_handle m, const float* d_pred, const float* d_gt, const float* d_norm, const float* d_area, const int32_t* d_rank,
                                    const int32_t* d_set, int32_t set_value, int32_t n, float* d_dist, float* d_oks, void* caller_stream);
VP_API int vp_metrics_update(vp_metrics_handle m, const float* pred, const float* gt, const float* norm, const float* area, const int32_t* rank, const int32_t* set,
                             int32_t set_value, int32_t n, float* dist, float* oks);
VP_API int vp_metrics_snapshot_stream(vp_metrics_handle m, void* d_out, void* caller_stream);
VP_API int vp_metrics_state_bytes(const vp_metrics_cfg* cfg, int64_t* bytes);
VP_API int vp_metrics_download_state(vp_metrics_handle m, void* out);
/* HOST ONLY, no device needed: csrc/metricsgeom.h run serially on a host state blob of vp_metrics_state_bytes (zeroed = a new evaluator), honouring the summation
 * order: the model the device is tested against (a test tap, never a fallback); the refusals of vp_metrics_create and vp_metrics_update_stream, the reason in
 * vp_last_error(NULL). */
VP_API int vp_dbg_metrics_host(void* state, const vp_metrics_cfg* cfg, const float* sigmas, const float* pred, const float* gt, const float* norm, const float* area,
                               const int32_t* rank, const int32_t* set, int32_t set_value, int32_t n, float* dist, float* oks);

/* COCO keypoint AP / AR on the device: an ACCUMULATING evaluator with the life cycle of vp_metrics_*.  It is COCOeval for iouType = 'keypoints' (computeOks,
 * evaluateImg, accumulate) with fixed parameters -- one category, maxDets = 20, the area ranges all [0, 1e10], medium [32^2, 96^2], large [96^2, 1e10], the OKS
 * thresholds np.linspace(.5, .95, 10) and the recall thresholds np.linspace(0, 1, 101) -- restated operation by operation in csrc/cocogeom.h, once for the kernels
 * and the host taps; easy_vitpose_amd/devcoco.py holds the numpy twin and finish(), which gives the ten figures of summarize.  UNPINNED: the pycocotools binary is
 * not available to this project's tests, the contract is a restatement of its source.
 *   One update, coordinates in (y, x, .) order: d_kpts float32 [n, n_joints, 3], d_score float32 [n], d_frame int32 [n] (NULL: 0), d_rank int32 [n] (optional: the
 *   row counts iff rank >= 0); d_gt_kpts float32 [g, n_joints, 3] rows of (y, x, v), d_gt_box float32 [g, 4] rows of (x, y, w, h), d_gt_area float32 [g], d_gt_flags
 *   int32 [g] (bit 0 = iscrowd; NULL: 0), d_gt_frame int32 [g] (NULL: 0); n_frames.  0 <= n, g <= VP_COCOEVAL_MAX_ROWS, 1 <= n_frames <= VP_COCOEVAL_MAX_FRAMES.  A
 *   row or gt whose frame lies outside [0, n_frames) does not count; rows need not be grouped by frame.  At most 128 gts per image are used; later ones, in call
 *   order, are left out and counted in gt_overflow.
 *   Per image: the counted rows ordered by score descending, equal scores to the lower row, a NaN score as -infinity (the order of the pose NMS); the first 20 are
 *   kept.  area_d = (max x - min x) (max y - min y) over all joints in fp64.  Per gt: k1 = the count of v > 0, ignore0 = iscrowd || k1 == 0.  OKS in fp64 on the
 *   float32 inputs: e_j = (dx^2 + dy^2) / (2 sigma_j)^2 / (area_g + 2^-52) / 2, over the joints with v > 0 (dx = xd - xg), or with k1 == 0 the distance to the
 *   doubled box over all joints (x0 = bx - bw, x1 = bx + 2 bw, dx = max(0, x0 - xd) + max(0, xd - x1)); oks = sum of exp(-e_j) / count, the sum in joint order
 *   (DEVIATION: np.sum is pairwise, a few ulps).  DEVIATION: a non-finite oks never matches and is counted in `nonfinite`.  Matching per (range, threshold):
 *   ignore_g = ignore0 || area_g outside the range; the gts ordered stably, not-ignored first; the detections in order, each starting at best = min(thr, 1 - 1e-10)
 *   and walking the gts: skip a gt already matched unless it is a crowd, stop when the current match is not ignored and this gt is, skip when oks < best, else take
 *   it.  A matched detection inherits its gt's ignore flag, an unmatched one is ignored iff area_d lies outside the range; npig[range] += the not-ignored gts.
 *   Record, 16 bytes per kept detection: float32 score, uint32 matched (bit 10 range + threshold), uint32 ignored, uint32 image ordinal (state.images + frame),
 *   appended in image order, inside an image in kept order; one that does not fit into max_records is not written and counted in `dropped`.
 *   d_match int32 [n, 10], optional: the gt row matched under "all" at each threshold, -1 unmatched, -2 a row not among its image's kept 20 or not counted.
 *   State blob (vp_cocoeval_state_bytes = 128 + 16 max_records; zeroed = new): int64 calls, images, rows, kept, records, dropped, gts, gt_overflow, nonfinite,
 *   npig[3], 0 x 4 | the record table.  A pure function of the inputs and the sequence of calls, byte for byte.
 *   Accumulate: records ordered by score descending (NaN as -infinity), equal scores by table position (COCOeval's stable argsort(-score) when images are fed in
 *   ascending id order); per (range, threshold) integer cumulative tp / fp, rc = tp / npig, pr = tp / (fp + tp + 2^-52), the precision envelope from the back, the
 *   first position with rc >= each recall threshold.  Result blob (vp_cocoeval_result_bytes = 128 + 8 * 3060): the header | double precision [3][10][101] | double
 *   recall [3][10]; npig == 0 gives -1, no position gives precision 0, no record recall 0.
 * vp_cocoeval_update_stream and vp_cocoeval_accumulate_stream only enqueue on caller_stream, a fixed launch sequence per evaluator (capturable as one linear chain):
 * no synchronisation, no host copy, no allocation, no atomics.  d_out: device, 8-byte aligned.  vp_cocoeval_update / vp_cocoeval_accumulate: the synchronous twins on
 * host pointers.  vp_cocoeval_create: on the device of h, state zeroed, sigmas = HOST double [n_joints]; destroy the evaluator before h.
 * VP_ERR_INVALID before anything is enqueued, the reason in vp_last_error: a NULL cfg; NULL d_kpts / d_score with n > 0; NULL d_gt_kpts / d_gt_box / d_gt_area with
 * g > 0; n, g, n_frames, n_joints (1..VP_NMS_MAX_K) or max_records (1..VP_COCOEVAL_MAX_RECORDS) outside its range; NULL sigmas, or a sigma not finite or <= 0; a NULL
 * accumulate destination.  Library builds that carry the stage define VP_HAS_COCOEVAL. */
#define VP_HAS_COCOEVAL 1
#define VP_COCOEVAL_MAX_ROWS 8192
#define VP_COCOEVAL_MAX_FRAMES 256
#define VP_COCOEVAL_MAX_RECORDS (1 << 20)
typedef struct vp_cocoeval_cfg {
    int32_t n_joints, max_records;
    int32_t reserved[2];
} vp_cocoeval_cfg;
typedef struct vp_cocoeval* vp_cocoeval_handle;
VP_API int vp_cocoeval_create(vp_handle h, const vp_cocoeval_cfg* cfg, const double* sigmas, vp_cocoeval_handle* out);
VP_API int vp_cocoeval_destroy(vp_cocoeval_handle e);
VP_API int vp_cocoeval_reset_stream(vp_cocoeval_handle e, void* caller_stream);
VP_API int vp_cocoeval_update_stream(vp_cocoeval_handle e, const float* d_kpts, const float* d_score, const int32_t* d_frame, const int32_t* d_rank, int32_t n,
                                     const float* d_gt_kpts, const float* d_gt_box, const float* d_gt_area, const int32_t* d_gt_flags, const int32_t* d_gt_frame, int32_t g,
                                     int32_t n_frames, int32_t* d_match, void* caller_stream);
VP_API int vp_cocoeval_update(vp_cocoeval_handle e, const float* kpts, const float* score, const int32_t* frame, const int32_t* rank, int32_t n, const float* gt_kpts,
                              const float* gt_box, const float* gt_area, const int32_t* gt_flags, const int32_t* gt_frame, int32_t g, int32_t n_frames, int32_t* match);
VP_API int vp_cocoeval_accumulate_stream(vp_cocoeval_handle e, void* d_out, void* caller_stream);
VP_API int vp_cocoeval_accumulate(vp_cocoeval_handle e, void* out);
VP_API int vp_cocoeval_state_bytes(const vp_cocoeval_cfg* cfg, int64_t* bytes);
VP_API int vp_cocoeval_result_bytes(int64_t* bytes);
VP_API int vp_cocoeval_download_state(vp_cocoeval_handle e, void* out);
/* HOST ONLY, no device needed: csrc/cocogeom.h run serially on a host state blob of vp_cocoeval_state_bytes (zeroed = a new evaluator), and the accumulation of
 * such a blob into a result blob of vp_cocoeval_result_bytes: the model the device is tested against (test taps, never a fallback), with the refusals of
 * vp_cocoeval_create, vp_cocoeval_update_stream and vp_cocoeval_accumulate_stream, the reason in vp_last_error(NULL). */
VP_API int vp_dbg_cocoeval_update_host(void* state, const vp_cocoeval_cfg* cfg, const double* sigmas, const float* kpts, const float* score, const int32_t* frame,
                                       const int32_t* rank, int32_t n, const float* gt_kpts, const float* gt_box, const float* gt_area, const int32_t* gt_flags,
                                       const int32_t* gt_frame, int32_t g, int32_t n_frames, int32_t* match);
VP_API int vp_dbg_cocoeval_accumulate_host(const void* state, const vp_cocoeval_cfg* cfg, void* out);

/* HOST ONLY, no device needed: the plan those entries run for expert_ids [n] on a handle of n_experts experts and max_batch crops per chunk -- the pure function
 * ids -> order, segments that shapes their launches.  Per chunk c (crops [c max_batch, ...)), with B = max_batch rounded up to a multiple of 4:
 *   order [n]: position j of chunk c holds the chunk-local caller row order[c max_batch + j] (stable expert order)
 *   ids_padded [chunks, B]: the experts in that order; the rows beyond the chunk repeat the last id (the encoder's padding crops)
 *   counts [chunks, n_experts]: crops per expert = the run-length segments of the sorted ids
 *   records [n, 3]: the decode's record per position {first heatmap of the crop, K_e, destination row}, given k_per_expert [n_experts]
 *   pattern [chunks]: the expert pattern in the hipGraph key -- an exact code of `counts` (one byte per expert), 0 for a chunk of one expert, all ones where
 *   the counts do not fit (more than 8 experts or 254 crops of one: such a chunk runs eagerly)
 * Any output may be NULL.  Returns the number of chunks, or VP_ERR_INVALID (< 0) for an id outside [0, n_experts) (vp_last_error(NULL) names the crop). */
VP_API int vp_dbg_mix_plan(const int32_t* expert_ids, int32_t n, int32_t n_experts, int32_t max_batch, const int32_t* k_per_expert, int32_t* order,
                           int32_t* ids_padded, int32_t* counts, int32_t* records, uint64_t* pattern);
/* The record route of the decode kernel alone, on host data (as vp_decode_only): heatmaps = float32 [n_maps, 64, 48]; records [n, 3] as above, crop j's K_j
 * maps start at map first_j -> out [n, kmax, 3]: row dst_j = vp_decode_only of those K_j maps as one crop (org_wh [n, 2] by destination row, or NULL), bit for
 * bit, joints beyond K_j zero.  VP_ERR_INVALID for a record outside the maps or the output, or two records with one destination. */
VP_API int vp_dbg_decode_mix(int32_t device_id, const float* heatmaps, int32_t n_maps, int32_t n, int32_t kmax, const int32_t* records,
                             const int32_t* org_wh, float* out);
/* HOST ONLY: the plan of the same chunks under the per-expert flip-test mode (vp_set_flip_test_experts).  Arguments as vp_dbg_mix_plan; a chunk holds
 * max_batch / 2 crops and its forward 2 nb rows -- position j of the order is rows 2 j (the crop) and 2 j + 1 (its mirror):
 *   order [n], counts [chunks, n_experts], pattern [chunks]: per CROP, as vp_dbg_mix_plan gives them for chunks of max_batch / 2
 *   row_ids [chunks, B]: the expert of every forward row, ids[order[r >> 1]]; the rows beyond 2 nb repeat the last one
 *   records [n, 4]: {first, K_e, destination row, e} with first = 2 seg_start Kmax + 2 (j - seg_start) K_e; the mirror's K_e maps start at first + K_e
 * Returns the number of chunks, or VP_ERR_INVALID as vp_dbg_mix_plan does, and for max_batch < 2. */
VP_API int vp_dbg_mix_plan_flip(const int32_t* expert_ids, int32_t n, int32_t n_experts, int32_t max_batch, const int32_t* k_per_expert, int32_t* order,
                                int32_t* row_ids, int32_t* counts, int32_t* records, uint64_t* pattern);
/* That mode's decode kernel alone, on host data: heatmaps = float32 [n_maps, 64, 48]; records4 [n, 4] as above; partners = int32 [n_experts, kmax], row e the
 * mirror joint of every joint of expert e (vp_dbg_flip_partner, the identity beyond K_e) -> out [n, kmax, 3]: row dst_j = vp_dbg_decode_flip of the
 * [2, K_j, 64, 48] maps from first_j on under expert e_j's table, bit for bit, joints beyond K_j zero.  VP_ERR_INVALID for a record whose 2 K maps leave
 * [0, n_maps), a destination outside [0, n), two records with one destination, an expert outside [0, n_experts). */
VP_API int vp_dbg_decode_flip_mix(int32_t device_id, const float* heatmaps, int32_t n_maps, int32_t n, int32_t kmax, const int32_t* records4,
                                  const int32_t* partners, int32_t n_experts, int32_t shift_heatmap, const int32_t* org_wh, float* out);

/* Decode alone: keypoints_from_heatmaps(unbiased=True, use_udp=True) + postprocess
 * (vit_utils/top_down_eval.py:493-641, easy_ViTPose/inference.py:187-205), one crop
 * at a time semantics.  heatmaps float32 [N, K, 64, 48] on the host. */
VP_API int vp_decode_only(int32_t device_id, const float* heatmaps, int32_t n, int32_t k,
                   const int32_t* org_wh, float* out);

/* HIP stream of the handle (a hipStream_t), for callers that order their own work against it. */
VP_API void* vp_stream(vp_handle h);
VP_API int vp_synchronize(vp_handle h);

/* HIP-event timing per kernel family: family_mask bit f (1 << VP_PROF_*) turns timing of
 * family f on (two event records around each of its launches); -1 = all, 0 = off. */
VP_API int vp_set_profiling(vp_handle h, int32_t family_mask);
VP_API int vp_reset_profile(vp_handle h);
VP_API int vp_get_profile(vp_handle h, vp_profile* out);
/* Name of the kernel the LAST launch of family `family` (VP_PROF_*) ran on, as the profiler prints it minus the namespace
 * (e.g. "gemm8_kernel<F16, 1, G8<256>>", "gemm_kernel<F16, 6, 0, TileCfg<192, 128, 64, 48, 64, 2, 1>>"), written by the
 * launch code itself: bench.py reads `roofline.kernel` from here instead of restating the selection rule.  Empty string when
 * the family has not been launched yet.  Returns VP_ERR_INVALID for a bad family / NULL buffer. */
VP_API int vp_profile_kernel(vp_handle h, int32_t family, char* buf, int32_t cap);

VP_API int vp_destroy(vp_handle h);

/* Last error text of this handle (or of the failed vp_create when h == NULL).
 * The pointer stays valid until the next call on the same handle. */
VP_API const char* vp_last_error(vp_handle h);

/* ---- parity taps (used by tests/ only): run ONE kernel on host fp32 data; operands are
 * rounded to `dtype` exactly as the production packer / producing kernels round them. ---- */
/* out[M,N] = epilogue(A[M,K] . W[N,K]^T); epi: 0 = +bias (nn.Linear, vit.py:166), 1 = gelu(+bias)
 * (Mlp fc1+act, vit.py:137-138), 2 = +bias +aux[M,N] (residual add, vit.py:203-204),
 * 3 = +aux[m % 192] (patch embed + pos, vit.py:382).  K % 64 == 0. */
VP_API int vp_dbg_gemm(int32_t device_id, int32_t dtype, int32_t epi, int32_t M, int32_t N, int32_t K,
                       const float* A, const float* W, const float* bias, const float* aux, float* out);
/* qkv [B*192, 3*D] -> attention core output [B*192, D]  (vit.py:167-176) */
VP_API int vp_dbg_attention(int32_t device_id, int32_t dtype, int32_t B, int32_t D, int32_t heads,
                            const float* qkv, float* out);
/* the attention core in any variant of its launcher: flags 1 = query split, 2 = qkv passed to the kernel in the 64x64-blocked layout (re-tiled inside from the
 * row-major input), 4 = MXFP8 output (out = de-blocked, de-quantised values; out_scales [B*192, D/32] = the E8M0 bytes, NULL otherwise).  The device output is
 * filled with 0xFF bytes first, so an unwritten element returns as NaN.  VP_ERR_INVALID for what has no kernel: flags 2 / 4 off head dim 64, 4 with bf16 or
 * with flag 1. */
VP_API int vp_dbg_attention_case(int32_t device_id, int32_t dtype, int32_t B, int32_t D, int32_t heads, int32_t flags, const float* qkv, float* out,
                                 uint8_t* out_scales);
/* attn.qkv + attention core in ONE kernel (csrc/qkvattn.hip; head dim 64): x [2 npairs 192, D], Wqkv [3D, D], bias [3D] -> [M, D].  Neutral
 * LayerNorm statistics: the result must equal vp_dbg_gemm(epi 0) + vp_dbg_attention bit for bit.  npairs * heads >= 8. */
VP_API int vp_dbg_qkvattn(int32_t device_id, int32_t dtype, int32_t npairs, int32_t D, int32_t heads, const float* x, const float* W,
                          const float* bias, float* out);
/* LayerNorm(eps=1e-6) of x [M,D]: out16 = result rounded to dtype (returned as fp32), out32 = fp32 result */
VP_API int vp_dbg_layernorm(int32_t device_id, int32_t dtype, int32_t M, int32_t D, const float* x,
                            const float* gamma, const float* beta, float* out16, float* out32);
/* The last_norm launch of the default path (tests/test_gpu_final_ln.py): the same LayerNorm reading the two-plane residual stream.  hi_bits / lo_bits
 * [plane_rows, D] = the planes as 16-bit codes of `dtype`, uploaded as one buffer with plane = plane_rows * D (the stream is laid out for the encoder's padded
 * row count); the kernel is launched for M <= plane_rows rows.  out16 / out32 [plane_rows, D]: the stored codes as exact fp32 / the fp32 result; both device
 * outputs are filled with 0xFF bytes first, so an unwritten row returns as NaN and a written row >= M shows.  D % 4 == 0, D <= 1280. */
VP_API int vp_dbg_layernorm_planes(int32_t device_id, int32_t dtype, int32_t M, int32_t plane_rows, int32_t D, const uint16_t* hi_bits,
                                   const uint16_t* lo_bits, const float* gamma, const float* beta, float* out16, float* out32);
/* The patch gather alone (tests/test_gpu_patch_gather.py): crops -> the patch matrix [B * 192, 768] of PatchEmbed's conv (k 16, s 16, padding 2), row
 * b * 192 + py * 12 + px, column c * 256 + ky * 16 + kx.  mode 0 = the straight gather, 1 = the crops mirrored left-right, 2 = the flip-test twin gather (output
 * crop 2i = crop i, 2i + 1 = its mirror).  crops = host fp32 [n_src,3,256,192] (VP_INPUT_F32_NCHW) or uint8 [n_src,256,192,3] (VP_INPUT_U8_NHWC, normalised on
 * the device); modes 0 / 1: output crops n_src .. B - 1 repeat source crop n_src - 1; mode 2: output crops 2 n_src .. B - 1 repeat output crop 2 n_src - 1.
 * out_bits [B * 192 * 768] = the 16-bit codes as the kernel stored them.  The device output is filled with 0xFF bytes before the launch and followed by
 * 192 * 768 guard elements, returned as bytes in guard [2 * 192 * 768].  What the launchers refuse (mode 2 with 2 n_src > B, an unknown input_format) comes
 * back as an error, nothing is launched. */
VP_API int vp_dbg_im2col(int32_t device_id, int32_t dtype, int32_t input_format, int32_t mode, int32_t B, int32_t n_src, const void* crops,
                         uint16_t* out_bits, uint8_t* guard);
/* ConvTranspose2d(Cin,256,4,2,1)+BN(eval)+ReLU (topdown_heatmap_simple_head.py:303-319) on NHWC
 * x [B,Hin,Win,Cin] -> NHWC [B,2Hin,2Win,256]; tensors named keypoint_head.deconv_layers.{0,1}.* */
VP_API int vp_dbg_deconv(int32_t device_id, int32_t dtype, int32_t B, int32_t Hin, int32_t Win, int32_t Cin,
                         const float* x, const vp_tensor_desc* tensors, int32_t n_tensors, float* out);
/* ONE GEMM of the keypoint head on a chosen tile, launched with the arguments the forward builds for it (tests/test_gpu_head.py).  stage 0: deconv + BN + ReLU
 * (x [B,Hin,Win,Cin] NHWC -> out [B,2Hin,2Win,256], 16-bit returned as fp32); stage 1: the same with the final 1x1 conv fused behind it (out = fp32 heatmaps
 * [B,Kp,2Hin,2Win]); stage 2: the un-fused pair of launches on the same operands (mid = the 16-bit tensor, out = the heatmaps; 32 x 24 x 256 only).  variant = the
 * deconv's tile (gemm.hip Cfg id; -1 = the selection rule's pick), parity_fast = 1 the product's launch order / 0 that of VP_DECONV_PARITY_FAST=0.  tensors as for
 * vp_dbg_deconv; stages 1 / 2: w_fin [Kp,256], b_fin [Kp].  Every device output is filled with 0xFF bytes before the launch (an unwritten element returns as NaN)
 * and followed by 16 * (4 Hin Win) guard elements, returned as bytes in guard (of out: 2 bytes per element at stage 0, else 4) and mid_guard (of mid, 2 bytes per
 * element).  What the launcher refuses (a tile without a kernel for the epilogue, ...) comes back as an error, nothing is launched. */
VP_API int vp_dbg_head_case(int32_t device_id, int32_t dtype, int32_t stage, int32_t variant, int32_t parity_fast, int32_t B, int32_t Hin, int32_t Win,
                            int32_t Cin, const float* x, const vp_tensor_desc* tensors, int32_t n_tensors, int32_t Kp, const float* w_fin,
                            const float* b_fin, float* out, uint8_t* guard, float* mid, uint8_t* mid_guard);
/* the device crop / zero-pad / resize kernel alone: uint8 crops [n, 256, 192, 3] */
VP_API int vp_dbg_crop_prep(int32_t device_id, const uint8_t* frame, int32_t fh, int32_t fw, const int32_t* crop_params,
                            int32_t n, uint8_t* out);
/* one launch of a production GEMM configuration on HOST data (layouts built / undone inside): variant = tile configuration (gemm.hip Cfg id;
 * 16 / 17 / 18 = the 8-phase kernel of gemm8.hip with 256x256 / 256x192 / 192x256 tiles); flags: 1 persistent workgroups, 2 64x64-blocked output,
 * 4 64x64-blocked A operand, 8 reversed tile walk, 16 LayerNorm-consumer fold, bits 8-11 = S > 1: split-K (epi 6 only: S partial products over k ranges +
 * the fixed-order reduction kernel, the small-batch path of attn.proj / mlp.fc2); epi 0-3, 5 (final 1x1 conv with hi+lo
 * weights -> heatmaps [M/3072, N, 3072]), 6, 7; rowstat [M,2] + ln_s [N] = LayerNorm-consumer fold; stats [M, N/64, 2] (epi 6 / 7) */
VP_API int vp_dbg_gemm_case(int32_t device_id, int32_t dtype, int32_t epi, int32_t variant, int32_t group_m, int32_t flags,
                            int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias, const float* aux,
                            const float* rowstat, const float* ln_s, float* out, float* stats);
/* vp_dbg_gemm_case for the producers of the two-plane residual stream (epi 6 / 7), with the stream as plane BITS on both sides: epi 6 reads the residual
 * planes r_hi / r_lo [M, N] (16-bit codes of `dtype`), epi 7 the fp32 pos [192, N]; o_hi / o_lo [M, N] return the output planes, stats [M, N/64, 2] the
 * granule statistics.  in_place != 0 (epi 6): the kernel updates the residual planes themselves (out == aux, as the forward launches it); split-K
 * (flags bits 8-11) is in place either way. */
VP_API int vp_dbg_gemm_case_planes(int32_t device_id, int32_t dtype, int32_t epi, int32_t variant, int32_t group_m, int32_t flags, int32_t M, int32_t N,
                                   int32_t K, const float* A, const float* W, const float* bias, const uint16_t* r_hi, const uint16_t* r_lo,
                                   const float* pos, int32_t in_place, uint16_t* o_hi, uint16_t* o_lo, float* stats);
/* The consumer side of the fused LayerNorm, one kernel each on host data (tests/test_gpu_ln_consumer.py).
 * vp_dbg_ln_finalize: partials [M, tiles, 2] = (sum, M2 about the granule mean) per 64-column granule -> rowstat [M, 2] = (mean, rstd) of rows of D columns.
 * vp_dbg_gemm_case_lnpart: vp_dbg_gemm_case for epi 0 / 1 with the partials [M, ln_tiles, 2] in place of rowstat -- the consumer merges them in its prologue
 *   (ln_inv_d = 1 / K); an 8-phase tile, the persistent kernel and an odd ln_tiles are refused by the launcher and come back as an error, nothing is launched.
 * vp_dbg_qkvattn_ln: vp_dbg_qkvattn with the caller's rowstat [M, 2] and row sums ln_s [3D] (head dim 64 and 80, through the same head-major repack).
 * vp_dbg_ln_quant (fp8 mode): x_hi [M, D] = the hi plane as 16-bit codes, partials [M, D/64, 2] -> codes [Mp * D] and scales [Mp * D / 32] in the layouts of
 *   csrc/mx8.h, both filled with 0xFF bytes before the launch (the padding rows M .. Mp - 1 must come back zero).  Mp % 64 == 0, D % 128 == 0. */
VP_API int vp_dbg_ln_finalize(int32_t device_id, int32_t M, int32_t tiles, int32_t D, const float* partials, float* rowstat);
VP_API int vp_dbg_gemm_case_lnpart(int32_t device_id, int32_t dtype, int32_t epi, int32_t variant, int32_t group_m, int32_t flags, int32_t M, int32_t N,
                                   int32_t K, const float* A, const float* W, const float* bias, const float* partials, int32_t ln_tiles, const float* ln_s,
                                   float* out);
VP_API int vp_dbg_qkvattn_ln(int32_t device_id, int32_t dtype, int32_t npairs, int32_t D, int32_t heads, const float* x, const float* W, const float* bias,
                             const float* rowstat, const float* ln_s, float* out);
VP_API int vp_dbg_ln_quant(int32_t device_id, int32_t dtype, int32_t M, int32_t Mp, int32_t D, const uint16_t* x_hi, const float* partials, uint8_t* codes,
                           uint8_t* scales);
/* The sharding plan of vp_group_infer for n crops on w devices of max_batch maxb -- HOST ONLY, no device needed: the exact
 * function group_run executes.  Rounds of w * maxb crops; inside a round device i takes [off, off + cnt) with ceil(nr / w) crops
 * per device (trailing devices short or empty).  Entry e = round * w + device: offs[e], cnts[e].  Returns the number of
 * entries (rounds * w), also when it exceeds `cap` (nothing is written beyond cap); < 0 on bad arguments. */
VP_API int vp_dbg_group_plan(int32_t n, int32_t w, int32_t maxb, int32_t* offs, int32_t* cnts, int32_t cap);
/* The plan of vp_infer_frames -- HOST ONLY, no device needed, the function vp_infer_frames runs first: checks every crop of params9 [n, 9]
 * against frames[n_frames] (h, w and whether data is NULL; the pixels are never read) and writes bands [n_frames, 2] = the rows
 * [row0, row1) of each frame its crops cover ({0, 0} for a frame without crops; bands may be NULL).  VP_OK or VP_ERR_INVALID. */
VP_API int vp_dbg_frame_plan(const vp_frame* frames, int32_t n_frames, const int32_t* params9, int32_t n, int32_t* bands);
/* The box geometry of vp_infer_boxes_stream -- HOST ONLY, no device needed, the same function its kernel runs: host float32 boxes xyxy
 * (row i at xyxy + i * row_stride), frame_idx [n] (NULL: frame 0), frame_hw [n_frames, 2] = (h, w) -> out9 [n, 9] (the d_crop_params rows) and
 * status [n] (either may be NULL).  VP_ERR_INVALID for the host-argument refusals of vp_infer_boxes_stream (a NULL box / frame table,
 * row_stride < 4, pad < 0, n > 0 with n_frames <= 0, a frame side outside [1, 2^24]). */
VP_API int vp_dbg_box_geometry(const float* xyxy, int32_t row_stride, const int32_t* frame_idx, const int32_t* frame_hw, int32_t n_frames,
                               int32_t n, int32_t pad, int32_t* out9, int32_t* status);
/* HOST ONLY: which tile of the 8-phase GEMM kernel the selection rule picks for an [M, N] output -- 0 = none (2-phase kernels), 16 = 256 x 256,
 * 17 = 256 x 192, 18 = 192 x 256; wide != 0: 16-bit-output GEMMs (qkv, fc1), else the residual GEMMs; bm192_mask bits 1 / 2 as VP_G8_BM192, bit 4 = the
 * round-3 thresholds (as VP_G8_COST=0); *tiles (may be NULL) = its tile count */
VP_API int vp_dbg_gemm8_pick(int32_t M, int32_t N, int32_t wide, int32_t bm192_mask, int32_t* tiles);
/* HOST ONLY: which tile configuration of the 2-phase GEMM kernel (gemm.hip Cfg id: 8 / 11 = 192 x 128 with 4 / 8 waves, 1 = 128 x 128, 9 / 12 = 64 x 64 on a 2- / 4-stage
 * ring, 15 = 128 x 64 3-stage, 30 / 31 = 64 x 64 / 32 x 64 with two k-blocks per barrier) the selection rule picks for one GEMM of the path: epi = 0 bias (qkv), 1 bias + GELU
 * (fc1), 4 deconv, 5 final 1x1 conv, 6 residual + row statistics (attn.proj, mlp.fc2), 7 patch embed; [M, N] output, depth K; *group_m (may be NULL) = its tile-order group.
 * (Large batches: the 8-phase kernel takes the encoder GEMMs over where vp_dbg_gemm8_pick says so.) */
VP_API int vp_dbg_gemm2_pick(int32_t epi, int32_t M, int32_t N, int32_t K, int32_t* group_m);
/* HOST ONLY: the split-K rule of the residual GEMMs at small batches (attn.proj / mlp.fc2 of [M, N] x K): returns the number of k ranges S (1 = the one-launch
 * residual epilogue; S > 1 = S partial products + the fixed-order reduction kernel), *variant (may be NULL) = the gemm.hip Cfg id of the partial products */
VP_API int vp_dbg_splitk_pick(int32_t M, int32_t N, int32_t K, int32_t* variant);
/* HOST ONLY: the batch the ENCODER runs for a chunk of n crops of a model of embed dim D (>= n; limit = the largest batch the workspaces hold).  From 33 crops on a chunk
 * that is no multiple of 4 crops runs the next multiple of 4 where that moves mlp.fc1 / mlp.fc2 onto the 8-phase kernel's 256-row tiles (or saves a round of them): the padding
 * rows repeat the last crop, every kernel works row by row or crop by crop, so the real crops' keypoints are bit for bit those of the unpadded run; the head and the decode run
 * the real crops only.  VP_PAD_BATCH=0 switches the padding off. */
VP_API int vp_dbg_run_batch(int32_t n, int32_t D, int32_t limit);
/* HOST ONLY: the tile mlp.fc2 of a ViTPose+ batch that mixes experts runs -- `variant` = the tile the rules above picked for [M, N], gemm8_ok = the 8-phase
 * kernel may run the GEMM, bounds[0 .. n_bounds) = the crops (in expert order) at which the expert changes.  Returns `variant` where no tile spans a change
 * (32 / 64 / 96 / 192-row tiles always; 128 / 256-row tiles where every change is a multiple of 2 / 4 crops), else the crop-aligned fallback (18 = the 8-phase
 * 192 x 256 tile, 11 = the 2-phase 192 x 128 residual tile). */
VP_API int vp_dbg_expert_tile(int32_t variant, int32_t M, int32_t N, int32_t gemm8_ok, const int32_t* bounds, int32_t n_bounds);
/* HOST ONLY: the plan a handle of *cfg runs for a chunk of n crops (1 <= n <= max_batch; one expert), with the switches vp_create would read from the
 * environment now.  Writes min(cap, 55) ints to out and returns 55 (VP_ERR_INVALID on bad arguments):
 *   [0] crops the encoder runs (>= n: padding crops repeat the last one)   [1] / [2] attn.qkv / mlp.fc1 merge the LayerNorm statistics themselves
 *   [3] qkv path: 0 = attn.qkv GEMM + attention kernel, 1 = fused kernel (head dim 64), 2 = fused 8-phase tile (head dim 80)
 *   [4] attention on three workgroups per (crop, head)   [5] deconv2 + final conv fused   [6] fp8 mode: attn.proj on the MXFP8 kernel
 *   then 8 GEMMs -- patch embed, attn.qkv, attn.proj, mlp.fc1, mlp.fc2, deconv1, deconv2, final conv (unused when [5]) -- of 6 ints each:
 *   variant (gemm.hip Cfg id; 16 / 17 / 18 = the 8-phase 256 x 256 / 256 x 192 / 192 x 256 tile, on the MXFP8 kernel for the fp8 GEMMs), tile-order group,
 *   persistent workgroups, start stagger, split-K ranges S (1 = one launch), Cfg id of the partial products. */
VP_API int vp_dbg_chunk_plan(const vp_config* cfg, int32_t n, int32_t* out, int32_t cap);
/* The two-phase schedule of a group call -- HOST ONLY, stub members: the order in which group_run would submit to (+ (member + 1)) and
 * wait for (- (member + 1)) its members for n crops on w devices of max_batch maxb.  Within every round all submissions precede the
 * first wait: no member's enqueue waits for another member's compute.  Returns the trace length (also beyond `cap`); < 0 on bad arguments. */
VP_API int vp_dbg_group_trace(int32_t n, int32_t w, int32_t maxb, int32_t* trace, int32_t cap);
/* BASELINE config 5 probe (fp8 is documented tolerance-infeasible; this confirms the CPU emulation the
 * finding rests on, tests/fp8_budget.py, on the hardware): rows of A [M,K] and W [N,K] are quantised on device to OCP e4m3
 * (x / scale[row], v_cvt_pk_fp8_f32) and multiplied through v_mfma_f32_16x16x128_f8f6f4:
 * out[m][n] = a_scale[m] w_scale[n] sum_k a8 w8.  a_codes / w_codes (uint8 [M,K] / [N,K], may be NULL) return the codes.
 * M, N multiples of 16, K a multiple of 128. */
VP_API int vp_dbg_fp8_gemm(int32_t device_id, int32_t M, int32_t N, int32_t K, const float* A, const float* a_scale, const float* W,
                           const float* w_scale, float* out, uint8_t* a_codes, uint8_t* w_codes);
/* MX probe (the opt-in fp8 mode's operand format, csrc/mx8.h): rows of A [M,K] are quantised on device to MXFP8 -- OCP e4m3 codes with
 * one E8M0 power-of-two scale per block of 32 consecutive k -- W [N,K] to e4m3 with the given per-row scale, and multiplied through the
 * BLOCK-SCALED v_mfma_scale_f32_16x16x128_f8f6f4 with the operand roles and packed scale dwords of the production GEMM.  Returns the
 * product and (optionally) the codes / scale bytes in the library's layouts so that a test can restate the arithmetic exactly.
 * M % 64 == 0, N % 16 == 0, K % 128 == 0. */
VP_API int vp_dbg_mx_gemm(int32_t device_id, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* w_scale, float* out,
                          uint8_t* a_codes, uint8_t* a_scales, uint8_t* w_codes);
/* ONE launch of the fp8 mode's GEMM kernel (csrc/gemm8f.hip) on host fp32 data: A [M,K] is quantised to MXFP8 on device, W [N,K] on the host
 * as the weight packer does; a_deq [M,K] / w_deq [N,K] (may be NULL) return the values the codes and scales stand for.  epi 0: out = fp16(a.w^T
 * + bias); epi 1: out = gelu(a.w^T + bias) written as MXFP8 and returned de-quantised; epi 6: out = a.w^T + bias + aux as the two-plane residual
 * (hi + lo returned), stats [M, N/64, 2].  M % 256 == 0, K % 256 == 0, K >= 512, N % 256 == 0 (epi 6: N % 192 == 0 or N % 256 == 0). */
VP_API int vp_dbg_gemm_fp8_case(int32_t device_id, int32_t epi, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias,
                                const float* aux, float* out, float* stats, float* a_deq, float* w_deq);
/* vp_dbg_gemm_fp8_case with the buffers as the device holds them (tests/test_gpu_fp8_gemm.py).  flags: 1 = the 64 x 64-blocked output of attn.qkv (epi 0
 * only): out [M*N] then comes back in device order [M/64][N/64][64][64].  epi 1: o_codes [M*N] and o_scales [M*N/32] return the output's e4m3 codes and
 * E8M0 scale bytes in device order (csrc/mx8.h; both buffers are filled with 0xff before the launch); a_scales [M*K/32]: the scale bytes of the quantised
 * A operand in device order.  o_codes, o_scales, a_scales may be NULL. */
VP_API int vp_dbg_gemm_fp8_case_raw(int32_t device_id, int32_t epi, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias,
                                    const float* aux, float* out, float* stats, float* a_deq, float* w_deq, int32_t flags, uint8_t* o_codes,
                                    uint8_t* o_scales, uint8_t* a_scales);
/* HOST ONLY: the tile the vp_dbg_gemm_fp8_case* taps launch a case on, by the fp8 mode's own rule: variant 16 = 256 x 256, 17 = 256 x 192; group_m of the tile walk */
VP_API int vp_dbg_gemm_fp8_pick(int32_t epi, int32_t M, int32_t N, int32_t* variant, int32_t* group_m);
/* vp_dbg_gemm_fp8_case, epi 6, with the residual stream as plane bits (fp16 codes) on both sides, as vp_dbg_gemm_case_planes */
VP_API int vp_dbg_gemm_fp8_case_planes(int32_t device_id, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias,
                                       const uint16_t* r_hi, const uint16_t* r_lo, int32_t in_place, uint16_t* o_hi, uint16_t* o_lo, float* stats,
                                       float* a_deq, float* w_deq);
/* HOST ONLY: fp32 -> OCP e4m3 codes with the converter the fp8 weight packer uses (round to nearest even, saturating at 448) */
VP_API int vp_dbg_host_e4m3(const float* in, uint8_t* out, int64_t n);

/* ---- The detector network: YOLOv8-detect on the device ------------------------------------------------------------------------------------------------------
 * The stage between the letterbox stage and the detector stage: the tensor vp_letterbox_stream writes (fp16, [n, 3, H, W] or [n, H, W, 3], RGB, values / 255) to
 * the head vp_detect_stream takes ([n, 4 + nc, A], layout 0, or [n, A, 4 + nc], layout 1; float32 or float16).  csrc/yologeom.h states the network once: the layer
 * table and scaling rules of the scales n, s, m, l, x, the plan (every launch, every buffer), the load step and the Detect decode.  Eval mode, fp16 activations
 * (NHWC), fp16 weights with BatchNorm folded in double precision and rounded once, float32 biases, float32 accumulation, float32 Detect outputs and decode.
 *
 *   vp_yolo_create reads the scale (the rows of model.0.conv.weight), the repeat counts (the highest model.{i}.m.{j} present) and nc (the rows of
 *   model.22.cv3.0.2.weight) from the checkpoint's tensors (an ultralytics state dict of model.model: model.{i}.conv.weight, model.{i}.bn.*, ..., or a fused one
 *   with conv.weight + conv.bias), plans, folds, uploads and allocates every buffer for max_images images.  Nothing is allocated, copied or synchronised later.
 *   vp_yolo_forward_stream only enqueues on caller_stream: a pack pass, one implicit-GEMM MFMA kernel per convolution (bias, SiLU, the Bottleneck shortcut in its
 *   epilogue; split and cat are channel offsets), three max-pool launches, two upsample copies, one decode.  A linear chain, no atomics: run-to-run bit-identical
 *   and capturable in a graph.  d_input holds n_images images, d_head receives n_images heads; n_images 0 enqueues nothing.
 *   vp_yolo_forward: the synchronous twin on host pointers.  vp_yolo_info: nc, A, the number of launches and the bytes of device memory.
 *
 * Refusals (VP_ERR_INVALID, the reason in vp_last_error(h), before anything is enqueued): in_h / in_w not multiples of 32 in 32..1280, max_images outside 1..64,
 * an unknown input_layout, head_dtype or head_layout, nc outside 1..256, a missing tensor, a shape that contradicts the table, a repeat count of another scale,
 * a model.22.dfl.conv.weight that is not 0..15, n_images outside 0..max_images, a NULL or misaligned pointer.  Library builds that carry the stage define
 * VP_HAS_YOLO. */
#define VP_HAS_YOLO 1
typedef struct vp_yolo_cfg {
    int32_t in_h, in_w;      /* multiples of 32, 32..1280 */
    int32_t max_images;      /* 1..64 */
    int32_t input_layout;    /* 0 [n, 3, H, W], 1 [n, H, W, 3] */
    int32_t head_dtype;      /* VP_DET_F32 (0) or VP_DET_F16 */
    int32_t head_layout;     /* 0 [n, 4 + nc, A], 1 [n, A, 4 + nc] */
    int32_t reserved[2];     /* [0]: 1 keeps every internal buffer in a region of its own (vp_dbg_yolo_activation; more memory), 0 reuses regions; [1]: 0 */
} vp_yolo_cfg;
typedef struct vp_yolo_tensor {
    const char* name;
    const float* data;
    int64_t numel;
    int32_t ndim, shape[4];
    int32_t reserved;
} vp_yolo_tensor;
/* One launch of the plan.  kind: 0 pack (the caller's tensor to 8-channel NHWC), 1 convolution, 2 5x5 max-pool, 3 nearest x2 copy, 4 Detect decode.  A launch
 * reads channels [in_off, in_off + c_in) and writes channels [out_off, out_off + c_out) of every pixel of NHWC buffers with in_stride / out_stride channels per
 * pixel; res_buf >= 0: the shortcut added in the epilogue, read at the output pixel.  conv: the index vp_dbg_yolo_fold takes.  The decode reads the three
 * float32 level buffers in_buf, in_buf + 1, in_buf + 2 ([64 box logits | nc class logits] per anchor). */
typedef struct vp_yolo_launch {
    int32_t kind, layer, conv, k, s, act, f32_out;
    int32_t h_in, w_in, h_out, w_out, c_in, c_out;
    int32_t in_buf, in_off, in_stride, out_buf, out_off, out_stride, res_buf, res_off, res_stride;
    int32_t reserved[2];
} vp_yolo_launch;
/* One buffer of the plan: h x w pixels of c channels of elem_bytes each, per image.  Buffer 0 is the caller's input, the last one the caller's head. */
typedef struct vp_yolo_buffer { int32_t h, w, c, elem_bytes; } vp_yolo_buffer;
typedef struct vp_yolo* vp_yolo_handle;
VP_API int vp_yolo_create(vp_handle h, const vp_yolo_cfg* cfg, const vp_yolo_tensor* tensors, int32_t n_tensors, vp_yolo_handle* out);
VP_API int vp_yolo_destroy(vp_yolo_handle y);
VP_API int vp_yolo_info(vp_yolo_handle y, int32_t* nc, int32_t* A, int32_t* n_launches, int64_t* device_bytes);
VP_API int vp_yolo_forward_stream(vp_yolo_handle y, const void* d_input, int32_t n_images, void* d_head, void* caller_stream);
VP_API int vp_yolo_forward(vp_yolo_handle y, const void* input, int32_t n_images, void* head);
/* HOST ONLY (no device): the plan of a checkpoint at cfg.  launches [max_launches], buffers [max_buffers] (either may be NULL to ask for the counts only);
 * info int32 [16]: n_launches, n_buffers, n_convs, nc, A, the scale's letter, ch64, ch128, ch256, ch512, ch1024, d(3), d(6), Detect's c2, Detect's c3, 0.
 * The refusals of vp_yolo_create, the reason in vp_last_error(NULL). */
VP_API int vp_dbg_yolo_plan(const vp_yolo_cfg* cfg, const vp_yolo_tensor* tensors, int32_t n_tensors, vp_yolo_launch* launches, int32_t max_launches,
                            vp_yolo_buffer* buffers, int32_t max_buffers, int32_t* info);
/* HOST ONLY: the load step of convolution `conv` of the plan: w uint16 fp16 bits [rows][cols] with cols = k k c_in ((ky, kx, channel) order, channels padded to
 * 8), b float32 [rows]; dims int32 [2] = (rows, cols).  w / b may be NULL to ask for dims only. */
VP_API int vp_dbg_yolo_fold(const vp_yolo_cfg* cfg, const vp_yolo_tensor* tensors, int32_t n_tensors, int32_t conv, uint16_t* w, float* b, int32_t* dims);
/* HOST ONLY: yologeom.h's Detect decode run serially.  levels: float32, P3 then P4 then P5, each [n_images][h_l w_l][64 + nc] with h_l = in_h / (8, 16, 32);
 * head: [n_images, 4 + nc, A] (layout 0) or [n_images, A, 4 + nc] of head_dtype. */
VP_API int vp_dbg_yolo_decode_host(int32_t nc, int32_t in_h, int32_t in_w, int32_t n_images, const float* levels, int32_t head_dtype, int32_t head_layout, void* head);
/* After a forward of n_images: the whole buffer launch `launch` wrote into, [n_images][h][w][c] of its element type (the plan says which channels the launch
 * wrote).  Needs a stage created with cfg.reserved[0] = 1: its buffers are then never reused inside a forward and, filled with 0xFF bytes by vp_yolo_create,
 * show an element nothing wrote.  Synchronises. */
VP_API int vp_dbg_yolo_activation(vp_yolo_handle y, int32_t launch, int32_t n_images, void* out);
/* ONE launch of the convolution kernel on host data, on views the plan of a network never forms (a 1 x 1 reading at a channel offset): l gives k, s, act,
 * f32_out, the sizes and the three views (kind, layer, conv, the buffer ids are ignored); in fp16 bits [n][h_in][w_in][in_stride]; w fp16 bits [c_out][k k c_in] in
 * (ky, kx, channel) order; bias [c_out]; res (may be NULL) fp16 bits [n][h_out][w_out][res_stride]; out [n][h_out][w_out][out_stride] of the output's element
 * type, filled with 0xFF bytes before the launch so that an element the kernel did not write shows. */
VP_API int vp_dbg_yolo_conv_case(vp_handle h, const vp_yolo_launch* l, int32_t n_images, const uint16_t* in, const uint16_t* w, const float* bias, const uint16_t* res,
                                 void* out);

/* The simple decoder (upstream ViTPose's `vitpose-{s,b,l,h}-simple` files: TopdownHeatmapSimpleHead with num_deconv_layers = 0, upsample = 4 and
 * final_conv_kernel = 3, i.e. ReLU -> bilinear x 4 (align_corners = False) -> Conv2d(D, K, 3, padding = 1)).  vp_load_weights recognises it from the state dict --
 * vp_config is unchanged: the decoder is SIMPLE when no keypoint_head.deconv_layers.* tensor is present and keypoint_head.final_layer.weight holds K * D * 9
 * elements, classic (two deconvs + 1 x 1 conv) as ever otherwise.  Refused: a 3 x 3 final layer together with deconv_layers.* (VP_ERR_SHAPE), a final layer of
 * neither K * 256 nor K * D * 9 elements (VP_ERR_SHAPE), a ViTPose+ dict (mlp.experts.*) with a 3 x 3 final layer (VP_ERR_INVALID: no such checkpoints exist);
 * the message names the tensor.  On a simple-decoder handle the head of every entry (vp_infer*, submit / wait, frames, boxes, affine crops, the flip-test mode, graph
 * replay, groups, vp_infer_heatmaps) is one kernel in the commuted form of csrc/simpleheadgeom.h: fp32 from the tokens to the heatmaps, profiled under
 * VP_PROF_GEMM_FINAL.  Unpinned: parity with upstream ViTPose's own binary and with a published -simple checkpoint (the reference cannot execute this decoder).
 *   vp_head_kind: 0 = classic, 1 = simple; -1 without loaded weights.
 *   vp_dbg_simple_head_pack (HOST ONLY, no device): final_layer.weight w [K, D, 3, 3] -> the weight image the kernel reads, uint16 [9][rows][D] with
 *     rows = 32 ceil(K / 16): tap t = 3 ky + kx major, map k's hi row at (k / 16) 32 + k % 16 and its lo row 16 behind (hi = round16(w), lo = round16(w - hi)),
 *     rows of maps beyond K zero.  *rows is always written; image may be NULL to ask for it only.
 *   vp_dbg_simple_head_case: the launch the forward builds, on host data.  x = tokens float32 [B, 192, Cin] (rounded to dtype on upload: a no-op on values of that
 *     type), w [Kp, Cin, 3, 3], b [Kp] -> out float32 [B, Kp, 64, 48].  The device output is filled with 0xFF bytes first and followed by 16 planes of 64 x 48
 *     floats, which come back as bytes in guard [16 * 3072 * 4].  Cin a multiple of 32.  Library builds that carry the decoder define VP_HAS_SIMPLE_HEAD. */
#define VP_HAS_SIMPLE_HEAD 1
VP_API int vp_head_kind(vp_handle h);
VP_API int vp_dbg_simple_head_pack(int32_t dtype, int32_t K, int32_t D, const float* w, uint16_t* image, int32_t* rows);
VP_API int vp_dbg_simple_head_case(int32_t device_id, int32_t dtype, int32_t B, int32_t Cin, const float* x, const float* w, const float* b, int32_t Kp, float* out,
                                   uint8_t* guard);

#ifdef __cplusplus
}
#endif
#endif /* VITPOSE_HIP_H */
