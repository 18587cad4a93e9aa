// Internal launch interface between the C-ABI translation unit and the kernel
// translation units.  Everything here is host-side C++; kernels live in *.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Two builds of the same sources (easy_vitpose_amd/build.py): the PRODUCT library (libvitpose_hip.so) and, with -DVP_TOOLS, the
// measurement library tools/ loads (libvitpose_hip_tools.so): ablation flags and start stagger inside the GEMM loops, cycle
// stamps, the candidate rows of the tile table (tiles.h) and kernel variants, the development environment switches -- and two translation
// units of its own, probes.hip and tools_taps.hip.  In the product build GemmArgs::ablate / ::stagger read as the constant 0, so
// none of those branches exists in its kernels.
#ifdef VP_TOOLS
#define VP_ABLATE(g) ((g).ablate)
#define VP_STAGGER(g) ((g).stagger)
namespace vp {   // probes.hip: compiled into the measurement library only
// calibration micro-benchmarks (tools/): kind 0/1 = MFMA 16x16x32 / 32x32x16 f16 TFLOP/s, 2 = float4 copy TB/s
hipError_t peak_bench(int kind, double* result);
// tools/hwid_probe.py: every workgroup of a launch records (HW_REG_HW_ID, HW_REG_XCC_ID, start cycle lo, hi) -> d_out[blocks][4]
hipError_t hwid_probe_launch(uint32_t* d_out, int blocks, int threads, int lds_bytes, int spin, hipStream_t s);
}  // namespace vp
#else
#define VP_ABLATE(g) 0
#define VP_STAGGER(g) 0
#endif

namespace vp {

enum { DT_F16 = 0, DT_BF16 = 1 };

// More than 64 KiB of dynamic LDS is an opt-in, and a per-device function attribute: set once per (kernel instantiation, device).  `done` = the
// instantiation's own flags, a function-local static of its launcher; a device index outside the table sets the attribute at every launch.
inline hipError_t lds_opt_in(const void* kern, int bytes, bool (&done)[64]) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool known = dev >= 0 && dev < 64;
    if (known && done[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && known) done[dev] = true;
    return e;
}

// ----------------------------------------------------------------------- GEMM
// C[m][n] = sum_k A[m][k] * W[n][k]   (A activations, W = nn.Linear weight [out,in])
enum GemmEpi {
    EPI_BIAS = 0,        // + bias            -> 16-bit [M, ldo]           (qkv)
    EPI_BIAS_GELU = 1,   // gelu(+ bias)      -> 16-bit [M, ldo]           (fc1)
    EPI_BIAS_RESID = 2,  // + bias + aux[m]   -> fp32   [M, ldo] (aux may alias out: proj, fc2)
    EPI_POS = 3,         // + aux[m % 192]    -> fp32   [M, ldo]           (patch embed; bias folded into aux)
    EPI_DECONV = 4,      // relu(+ bias)      -> 16-bit NHWC, output-parity scatter (deconv + folded BN + ReLU)
    EPI_HEATMAP = 5,     // + bias            -> fp32 NCHW heatmaps [B, Kp, 64*48]  (final 1x1 conv)
    EPI_BIAS_RESID_LN = 6,  // EPI_BIAS_RESID on the two-plane residual stream + fused-LayerNorm row statistics
    EPI_POS_LN = 7,         // EPI_POS        writing the two-plane residual stream + row statistics
    EPI_DECONV_FINAL = 8,   // EPI_DECONV with the final 1x1 conv (EPI_HEATMAP) fused behind it: the 256-channel activations stay in LDS,
                            // fp32 NCHW heatmaps at out2 (256 x 256 tile only: N == 256, variant 3)
    EPI_QKV_ATTN = 9,       // gemm8.hip, 192 x 256 tiles only (round 5): attn.qkv of ONE crop x ONE head of head dim 80 (W = head-major [q | k | v | 16 zero rows],
                            // N = heads * 256) with the LayerNorm-consumer fold, q / k / v handed to the attention core through LDS; out = y [M, K] 16-bit
    EPI_PARTIAL = 10,       // split-K (round 6, small batches): workgroup (split s, tile) multiplies k in [s K / S, (s + 1) K / S) and writes its fp32 partial tile to
                            // out[s][M][ldo] -- no bias, no residual; splitk_reduce_launch adds the S partials in the fixed order s = 0 .. S - 1 (deterministic), then
                            // bias + residual planes, and writes planes + row statistics exactly like the EPI_BIAS_RESID_LN epilogue
};
enum GemmAMode { A_DENSE = 0, A_DECONV = 1 };

struct GemmArgs {
    const uint16_t* A;    // dense: [M, K] row-major.  deconv: NHWC source [B, Hin, Win, Cin]
    const uint16_t* W;    // [w_rows, K] row-major, zero padded rows (deconv: 4 parity slabs of [w_rows, K])
    const float* bias;    // [Npad]
    void* out;
    const float* aux;     // residual [M, ldo] / pos [192, ldo]
    int M, N, K, ldo;     // N = real columns (stores are masked to n < N)
    int Hin, Win, Cin;    // deconv geometry (K = 4 * Cin)
    const uint16_t* zero; // >= 128 B of zeros (deconv border taps)
    int Kp;               // heatmap: number of keypoints (== N)
    // EPI_DECONV_FINAL: final-layer weights as [16 hi][16 lo] row groups x 256 channels, bias [Kp], heatmaps fp32 [B, Kp, 2Hin, 2Win]
    const uint16_t* W2;
    const float* bias2;
    float* out2;
    int w_rows;           // rows W is padded to at upload (multiple of 256); deconv parity slab = w_rows * K
    int variant;          // tile configuration (an id of tiles.h)
    int group_m;          // grouped tile order: m-tiles per group (<= 1: plain n-fastest order)
    size_t w_parity_stride;  // filled by gemm_launch
    // ---- fused LayerNorm ----
    // producer side (EPI_BIAS_RESID_LN / EPI_POS_LN): the residual stream is two 16-bit planes, x = hi + lo,
    // hi = round16(x) at out / aux, lo = round16(x - hi) `plane` elements behind it; besides the rows the partial
    // row statistics (sum, M2 about the granule mean) of every 64-column granule go to stats_out[(m*(N/64) + n/64)*2]
    size_t plane;
    float* stats_out;
    // consumer side (EPI_BIAS / EPI_BIAS_GELU): A is the UN-normalised 16-bit residual stream, W has LayerNorm's
    // gamma folded in; the epilogue applies  v = rstd_m * (acc - mean_m * ln_s[n]) + bias[n]  with
    // rowstat[m] = (mean, rstd), ln_s[n] = sum_k W'[n][k], bias[n] = sum_k beta_k W[n][k] + b[n]
    const float* rowstat;
    const float* ln_s;
    // small batches: instead of rowstat, the producer's partial statistics [M][ln_tiles][2]; the consumer epilogue folds them itself
    // (common.h::ln_merge, the same code ln_finalize_kernel runs) and the 2 x depth ln_finalize launches disappear
    const float* ln_part;
    int ln_tiles;
    float ln_inv_d;       // 1 / D as the host computes it for ln_finalize_launch
    // 64x64-blocked activation layout [M/64][K/64][64][64]: every operand tile of the consuming GEMM is a run of
    // contiguous 8 KiB blocks (sequential DRAM bursts instead of 128-byte pieces at a row stride).  out_blocked: this
    // GEMM writes its 16-bit output that way (EPI_BIAS / EPI_BIAS_GELU, ldo == N); a_blocked: A is read that way.
    int a_blocked, out_blocked;
    // tile order last-to-first: a consumer of a tensor larger than the 256 MB Infinity Cache then starts with the
    // rows its producer wrote last (still cached) instead of the ones already evicted
    int reverse;
    // persistent workgroups whose operand ring runs on across tile boundaries (gemm.hip gemm_persist_kernel):
    // EPI_BIAS / EPI_BIAS_GELU on the default tile, K % 128 == 0
    int persist;
    // gemm8.hip: start of XCD x (= blockIdx & 7) delayed by x * stagger * 64 * 127 shader cycles, so that the eight XCDs reach
    // their tile boundaries -- the store bursts of the epilogue -- at different times instead of saturating HBM together
    int stagger;
    int ablate;           // VP_TOOLS builds only (tools/gemm_ablate.py): 1 = no operand loads after the prologue, 2 = every tile loads the A rows of m-tile 0 (A L2-resident), 8 = no epilogue stores
    char* desc;           // host side: when non-null the launch code writes the resolved kernel's name here (desc_cap bytes)
    int desc_cap;
    // ---- fp8 mode (gemm8f.hip; csrc/mx8.h): A = MXFP8 codes in 64 x 128 blocks (at `A`) + packed E8M0 block scales, W = e4m3 codes
    // row-major [w_rows, K] (at `W`) + one fp32 scale per output channel; EPI_BIAS_GELU writes its output as MXFP8 (codes at `out`, K of the
    // consumer = ldo, scales at out_scales)
    float attn_scale_log2e;   // EPI_QKV_ATTN: head_dim^-0.5 * log2(e)
    int splitk;        // EPI_PARTIAL: number of k ranges S (K % (S * BK) == 0; grid = tiles * S)
    int parity_fast;   // deconv: 1 = the four output parities of a tile are consecutive logical blocks (same XCD, shared input rows); 0 = parity on blockIdx.y
    union {
        const uint8_t* a_scales;   // fp8 mode (gemm8f.hip)
        // ViTPose+ mlp.fc2 of a batch that mixes experts (the residual epilogues' EXPERT instantiations of gemm.hip / gemm8.hip): the m-tile at row m0 belongs
        // to expert expert[m0 / 192] (one int32 per crop, device memory) and reads its weights expert * w_rows * K elements behind W, its bias
        // expert * w_rows floats behind bias.  The host never hands a tile that spans two experts (tile_rules.hip expert_tile_ok).
        const int32_t* expert;
    };
    const float* w_scale;
    uint8_t* out_scales;
};
hipError_t gemm_launch(int dtype, int epi, const GemmArgs& a, hipStream_t s);
// 8-phase persistent kernel (gemm8.hip): 256 x bn tiles (bn = 256 or 192), EPI_BIAS / EPI_BIAS_GELU / EPI_BIAS_RESID_LN.
// Selected through GemmArgs::variant 16 (bn 256) / 17 (bn 192) in gemm_launch.
bool gemm8_supported(int epi, const GemmArgs& a, int bn, int bm = 256);
// the part of gemm8_supported that depends on the shape alone (w_rows = the weight rows behind W): what the selection rule (tile_rules.hip) asks before it picks the kernel
bool gemm8_shape_ok(int epi, int M, int N, int K, int ldo, int w_rows, int bn, int bm);
hipError_t gemm8_launch(int dtype, int epi, const GemmArgs& a, int bn, hipStream_t s, int bm = 256);
// name of the kernel a launch resolves to, as the profiler prints it minus the namespace; written by the launch code when
// GemmArgs::desc != nullptr (vp_profile_kernel)

// 8-phase kernel on MXFP8 operands (gemm8f.hip): the encoder GEMMs of the opt-in fp8 mode.  K % 256 == 0, K >= 512, M % 256 == 0.
bool gemm8f_supported(int epi, const GemmArgs& a, int bn);
hipError_t gemm8f_launch(int epi, const GemmArgs& a, int bn, hipStream_t s);
// fp8 mode, between a residual GEMM and qkv / fc1 (quant8.hip): merges the producer's partial row statistics (ln_merge), normalises the
// hi plane of the residual stream and writes it as MXFP8 (codes [Mp/64][D/128][64][128], scales packed: mx8.h); rows >= M (padding up to
// the multiple of 256 the GEMM tiles need) are written as zeros.  LayerNorm's gamma / beta live in the consumer's weights / bias.
hipError_t ln_quant_launch(int dtype, const uint16_t* x_hi, const float* ln_part, int tiles, uint8_t* codes, uint8_t* scales, int M, int Mp, int D,
                           hipStream_t s);
// fp32 rows [M, K] -> MXFP8 in the same layouts (parity taps)
hipError_t mx_quantize_launch(const float* src, uint8_t* codes, uint8_t* scales, int M, int K, hipStream_t s);

// fill a 16-bit buffer with pseudo-random values in [-1, 1) (benchmark operands)
hipError_t fill_random16(int dtype, uint16_t* p, size_t n, uint32_t seed, hipStream_t s);

// partial row statistics [M][tiles][2] (sum, centred M2 per 64-column granule) -> rowstat [M][2] (mean, rstd), LayerNorm eps 1e-6
hipError_t ln_finalize_launch(const float* partials, float* rowstat, int M, int tiles, int D, hipStream_t s);
// split-K reduction of a residual GEMM (EPI_PARTIAL partials [S][M][N] fp32): x = ((p_0 + p_1) + ... + p_{S-1}) + bias + (x_hi + x_lo), written back as
// the two residual planes (in place: hi at x_hi, lo `plane` elements behind) + the partial row statistics [M][N/64][2] the LayerNorm consumers fold --
// the arithmetic of the EPI_BIAS_RESID_LN epilogue behind a fixed-order sum of the partials.  N % 64 == 0.
hipError_t splitk_reduce_launch(int dtype, const float* partials, int S, const float* bias, uint16_t* x_hi, size_t plane, float* stats_out, int M, int N,
                                hipStream_t s);

// fp8_probe.hip (parity tap of BASELINE config 5): rows of A [M,K] / W [N,K] -> e4m3 codes (x / scale[row]), out = scaled product
// through v_mfma_f32_16x16x128_f8f6f4
hipError_t fp8_probe_launch(const float* dA, const float* dW, const float* dAs, const float* dWs, uint8_t* dA8, uint8_t* dW8, float* dOut,
                            int M, int N, int K, hipStream_t s);

// MX probe: rows of A -> MXFP8 (e4m3 + one E8M0 scale per 32 k, layouts of mx8.h), W -> e4m3 per-row scale; product through the block-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4 with the operand roles and the packed scale dwords of the fp8 mode's GEMM.  M % 64 == 0, N % 16 == 0, K % 128 == 0
hipError_t mx_probe_launch(const float* dA, const float* dW, const float* dWs, uint8_t* dA8, uint8_t* dAs, uint8_t* dW8, float* dOut,
                           int M, int N, int K, hipStream_t s);

// ------------------------------------------------------------------ attention
// qkv [B*192, 3*D] 16-bit (columns = [q | k | v] x heads x head_dim, vit.py:166-167)
// out [B*192, D]   16-bit (columns = heads x head_dim, vit.py:176)
// qkv_blocked (head dim 64 only): qkv in the 64 x 64-blocked layout the GEMMs write with GemmArgs::out_blocked
// qsplit: three workgroups per (crop, head), one query tile per wave (small batches; the chunk plan decides, tile_rules.hip)
// mx_scales != nullptr (fp8 mode, head dim 64): the output is written as MXFP8 (codes at `out`, 64 x 128-blocked; E8M0 scales at mx_scales; no query split)
hipError_t attention_launch(int dtype, const uint16_t* qkv, uint16_t* out, int B, int D, int heads, hipStream_t s, bool qsplit, int qkv_blocked = 0,
                            uint8_t* mx_scales = nullptr);
// the softmax scale head_dim ** -0.5 (vit.py:156) folded into the base-2 exponent: what every attention kernel takes as scale_log2e.  ONE host
// definition: the fused and the unfused kernels must be handed the same float
inline float softmax_scale_log2e(int head_dim) { return (1.0f / sqrtf((float)head_dim)) * 1.4426950408889634f; }

// attn.qkv + attention core in one kernel (qkvattn.hip; head dim 64): tile = (pair of crops, head); the qkv tensor never reaches HBM.
// wh / bh / sh = head-major copies of the LayerNorm-folded qkv weights / bias / row sums (qkv_head_major_launch).  y bit-identical to
// gemm (EPI_BIAS, LayerNorm-consumer fold) + attention_launch.
struct QkvAttnArgs {
    const uint16_t* x_hi;     // hi plane of the residual stream [ncrops 192, D] (un-normalised 16-bit rows)
    const uint16_t* wh;       // [heads 192, D]
    const float* bh;          // [heads 192]
    const float* sh;          // [heads 192]
    const float* rowstat;     // (mean, rstd) per token row
    uint16_t* y;              // attention output [ncrops 192, D]
    int npairs, heads, D;
    int ncrops;               // 2 npairs, or 2 npairs - 1: the last pair of an odd batch runs its only crop in both halves (identical results stored twice)
    float scale_log2e;        // head_dim^-0.5 * log2(e)
    int ablate;               // VP_TOOLS builds only (tools/qkvattn_phases.py): 1 = no attention phase, 2 = no epilogue (LDS hand-over), 4 = no K-loop, 8 = no ring restart wait
};
bool qkvattn_supported(const QkvAttnArgs& a);
hipError_t qkvattn_launch(int dtype, const QkvAttnArgs& a, hipStream_t s, char* desc, int desc_cap);
hipError_t qkv_head_major_launch(const uint16_t* w, const float* b, const float* s, uint16_t* wh, float* bh, float* sh, int D, int K, hipStream_t st);
// head dim 80 (ViTPose-H; round 5): the fused kernel is gemm8.hip's 192 x 256 tile with EPI_QKV_ATTN -- one crop x one head per tile.  Head-major copy of the
// LayerNorm-folded qkv weights: rows h 256 + [0, 80) = q_h, [80, 160) = k_h, [160, 240) = v_h, [240, 256) = zeros; bias and row sums alike (heads * 256 entries)
hipError_t qkv_head_major80_launch(const uint16_t* w, const float* b, const float* s, uint16_t* wh, float* bh, float* sh, int D, int K, int heads, hipStream_t st);

// ---------------------------------------------------------------- elementwise
// fp32 [M, D] -> LayerNorm(eps 1e-6) -> 16-bit [M, D] (out16) and/or fp32 (out32), either may be null.
// plane != 0: x is the two-plane 16-bit residual stream (hi at x, lo `plane` elements behind) instead of fp32.
hipError_t layernorm_launch(int dtype, const float* x, const float* gamma, const float* beta,
                            uint16_t* out16, float* out32, int M, int D, hipStream_t s, size_t plane = 0);
// crops -> im2col patch matrix [B*192, 768] 16-bit (k = c*256 + ky*16 + kx, zero border of 2 px)
hipError_t im2col_launch(int dtype, const void* crops, int input_format, uint16_t* out, int B, hipStream_t s, bool flip = false, int n_src = 0);   // n_src < B: output crops n_src .. B - 1 repeat source crop n_src - 1
// ViTPose+ mixed batch: dst crop i = src crop idx[i] (idx: device int32 [n], each in [0, n_src)); crop_bytes % 16 == 0
hipError_t gather_crops_launch(const void* src, void* dst, const int32_t* idx, int n, size_t crop_bytes, hipStream_t s);
// flip-test: hm = 0.5 (hm + flip_back(hm_flipped)); partner[k] = mirror joint of k (k itself if unpaired)
hipError_t flip_merge_launch(float* hm, const float* hm_flipped, const int32_t* partner, int N, int K, int shift, hipStream_t s, int interleaved = 0);   // interleaved: crop n's maps lie 2 n K 3072 floats behind both pointers
// flip-test mode: B output crops = the n_src crops and their mirror images interleaved (2 i = crop i, 2 i + 1 = its mirror), rows beyond 2 n_src repeat the last one
hipError_t im2col_twin_launch(int dtype, const void* crops, int input_format, uint16_t* out, int B, int n_src, hipStream_t s);
void flip_twin_layout(int bo, int n_src, int* src, int* mirror);   // HOST: the source crop of output crop bo and whether it is mirrored (the kernel's own index function)

// one crop of a frame: src = plane 0 at the frame's pixel (y0, x0) (in a staged row band or in the caller's device frame), pitch = bytes per row of that plane;
// the crop is [ch, cw] pixels, placed at (top, left) of a zero [ph, pw] canvas (vp_infer_frames builds these on the host).  format / matrix (pixfmt.h) say how a
// source pixel becomes RGB8.  NV12: src1 = the UV pair of pixel (y0, x0), i.e. plane 1 at chroma (y0 >> 1, x0 >> 1), pitch1 its row bytes, and (oy, ox) = the
// parities of (y0, x0): crop pixel (yy, xx) reads the pair ((oy + yy) >> 1, (ox + xx) >> 1) behind src1 = the frame's ((y0 + yy) >> 1, (x0 + xx) >> 1)
struct CropRec {
    const uint8_t* src;
    int64_t pitch;
    int32_t cw, ch, left, top, pw, ph;
    const uint8_t* src1;
    int64_t pitch1;
    int32_t format, matrix, oy, ox;
};
// recs: device CropRec [n] -> crops u8 [n,256,192,3] RGB
hipError_t crop_resize_launch(const CropRec* recs, uint8_t* out, int n, hipStream_t s);

// vp_infer_boxes_stream (boxes.hip): frames [f0, f0 + count) of the call's table, passed by kernel argument (3 KiB: 64 entries of 48 bytes; 128 would pass the 4 KiB of a launch)
constexpr int BOX_FRAMES_PER_LAUNCH = 64;
struct BoxFrame {   // vp_image's fields
    const uint8_t* plane[2];
    int64_t pitch[2];
    int32_t h, w, format, matrix;
};
struct BoxFrames {
    BoxFrame fr[BOX_FRAMES_PER_LAUNCH];
    int32_t f0, count, n_frames;
};
// boxes xyxy (row i at xyxy + i * row_stride) + frame index [n] (NULL: frame 0) -> crop records, decode sizes wh [n, 2] = (pw, ph),
// aux [n, 4] = (y0 - top_pad, x0 - left_pad, status, 0); optional p9_out [n, 9] (frames_crop_params rows) and status_out [n].  slot (null: the identity):
// box i's crop record goes to recs[slot[i]] -- a ViTPose+ chunk with per-crop experts crops straight into its expert order; every other row stays at i
hipError_t box_geometry_launch(const BoxFrames& fr, const float* xyxy, int row_stride, const int32_t* frame_idx, int n, int pad, const uint8_t* zero_px,
                               CropRec* recs, int32_t* wh, int32_t* aux, int32_t* p9_out, int32_t* status_out, hipStream_t s, const int32_t* slot = nullptr);

// ---- the training-protocol affine crop (affinegeom.h): the second crop kernel, writing the same RGB8 crop buffer
// one crop: plane[p] = plane p of the frame at the first row the record may read (row y0 of plane 0, row y0 >> 1 of an NV12 frame's UV plane), in a staged row band
// or in the caller's device frame; rows [y0, y1) x columns [0, w) are the frame pixels that exist for this crop (a device frame: [0, h)), every other tap is 0.
// src(o) = o a + b per axis (affine_map).  A refused box is a record with y0 == y1: it reads nothing and gives a black crop
struct AffRec {
    const uint8_t* plane[2];
    int64_t pitch[2];
    double ax, bx, ay, by;
    int32_t w, y0, y1, format, matrix, pad_;
};
// recs: device AffRec [n] -> crops u8 [n,256,192,3] RGB
hipError_t crop_affine_launch(const AffRec* recs, uint8_t* out, int n, hipStream_t s);
// boxes xyxy (row i at xyxy + i * row_stride) + frame index [n] (NULL: frame 0) -> crop records, cs [n, 4] = (cx, cy, S_w, S_h) (what the affine decode reads;
// a box with a non-zero status: an all-zero row and a record that reads nothing); optional cs_out [n, 4] (the same rows) and status_out [n].  Frames by kernel
// argument and one writer per box, as box_geometry_launch
hipError_t box_cs_launch(const BoxFrames& fr, const float* xyxy, int row_stride, const int32_t* frame_idx, int n, float box_scale, AffRec* recs, float* cs,
                         float* cs_out, int32_t* status_out, hipStream_t s);

// --------------------------------------------------------------------- decode
// heatmaps fp32 [N, K, 64, 48] -> out fp32 [N, K, 3] (y, x, conf); org_wh int32 [N,2] or null
hipError_t decode_launch(const float* hm, const int32_t* org_wh, float* out, int N, int K, hipStream_t s);
// flip-test mode: hm = the interleaved batch [2 N, K, 64, 48] (crop, mirror, crop, mirror, ...); decodes 0.5 (crop + flip_back(mirror)) without materialising it,
// bit for bit flip_merge_launch + decode_launch
hipError_t decode_flip_launch(const float* hm, const int32_t* partner, int shift, const int32_t* org_wh, float* out, int N, int K, hipStream_t s);

// the affine route: cs float32 [N, 4] = (cx, cy, S_w, S_h) per crop instead of org_wh; out (y, x) in FRAME pixels with one rounding,
// x = (float)(rx (S_w / 47) + cx - S_w 0.5) in fp64 with unfused steps, y with 63; a row whose S_w is not > 0 (a refused box) is all zero
hipError_t decode_affine_launch(const float* hm, const float* cs, float* out, int N, int K, hipStream_t s);
hipError_t decode_affine_flip_launch(const float* hm, const int32_t* partner, int shift, const float* cs, float* out, int N, int K, hipStream_t s);

// ViTPose+ chunk with per-crop experts: the crop at position j of the chunk's expert order.  `first` = index of its first 64 x 48 map in the chunk's heatmap
// buffer, K = its expert's joint count, dst = its row in the caller's order (output row, and row of org_wh)
struct MixRec {
    int32_t first, K, dst;
};
// the record route of the decode: ONE launch for the whole chunk.  Block (j, k): k < recs[j].K decodes map recs[j].first + k as decode_launch does on a
// [1, K, 64, 48] crop (same arithmetic, same summation orders, same bits) into out[recs[j].dst][k]; k >= K writes zeros.  out fp32 [N, Kmax, 3], org_wh [N, 2] or null
hipError_t decode_mix_launch(const float* hm, const MixRec* recs, const int32_t* org_wh, float* out, int N, int Kmax, hipStream_t s);
// The same chunk under the per-expert flip-test mode (vp_set_flip_test_experts): the forward ran every crop and its mirror image as rows 2 j, 2 j + 1 of the expert
// order, so the crop's K maps start at `first` and its mirror's at first + K; e = its expert, the row of the [n_experts, Kmax] partner table its mirror is read by
struct MixRecFlip {
    int32_t first, K, dst, e;
};
// Block (j, k): k < recs[j].K decodes 0.5 (map first + k + flip_back(map first + K + partners[e][k])) as decode_flip_launch does on a [2, K, 64, 48] pair (same fp32
// add, exact multiply and summation orders: same bits) into out[recs[j].dst][k]; k >= K writes zeros.  partners: device int32 [n_experts, Kmax]
hipError_t decode_flip_mix_launch(const float* hm, const MixRecFlip* recs, const int32_t* partners, int shift, const int32_t* org_wh, float* out, int N, int Kmax,
                                  hipStream_t s);
// vp_infer_boxes_stream: decoded keypoints [n, K, 3] in padded-crop pixels -> frame pixels (aux as box_geometry_launch writes it; status != 0: all zero).  slot + recs
// (both or neither): rows of K = Kmax joints of a chunk with per-crop experts -- row i keeps the zeros behind its expert's recs[slot[i]].K joints
hipError_t box_offsets_launch(const int32_t* aux, float* out, int n, int K, hipStream_t s, const int32_t* slot = nullptr, const MixRec* recs = nullptr);

// The per-call tables of such a chunk travel by kernel argument (no copy from host memory): positions [base, base + count) of the expert order per launch --
// id = the expert, order = the caller row (gather_crops_launch's index, MixRec::dst), first / K as MixRec.  The launch with pad_to > 0 (the chunk's last)
// also writes ids[base + count .. pad_to) = its last id: the encoder's padding crops repeat the last crop.  slot[order[j]] = j: the caller row's position.
constexpr int MIX_CROPS_PER_LAUNCH = 128;
struct MixTable {
    int32_t id[MIX_CROPS_PER_LAUNCH], order[MIX_CROPS_PER_LAUNCH], first[MIX_CROPS_PER_LAUNCH], K[MIX_CROPS_PER_LAUNCH];
    int32_t base, count, pad_to;
};
hipError_t mix_tables_launch(const MixTable& t, int32_t* ids, int32_t* order, int32_t* slot, MixRec* recs, hipStream_t s);
// ... under the per-expert flip-test mode: position j of the expert order is forward rows 2 j and 2 j + 1, so ids[2 j] = ids[2 j + 1] = id (pad_to counts ROWS:
// ids[2 (base + count) .. pad_to) repeat the last id), order / slot stay per crop, and the decode's record is recs_flip[j] = {first, K, order, id}
// (recs[j] keeps {first, K, order} for box_offsets_launch, which reads K alone)
hipError_t mix_tables_flip_launch(const MixTable& t, int32_t* ids, int32_t* order, int32_t* slot, MixRec* recs, MixRecFlip* recs_flip, hipStream_t s);

// ---------------------------------------------------------------- simple decoder
// simplehead.hip: ReLU -> bilinear x 4 -> Conv2d(D, K, 3, padding = 1) in the commuted form of simpleheadgeom.h, one launch of (ceil(K / 16), n) workgroups.
// y = the last_norm tokens [n, 192, D] (16-bit), w = the tap-major hi / lo weight image (9 x rows x D, rows = sh_rows(K)), bias fp32 [K], hm fp32 [n, K, 64, 48].
// D a multiple of 32; y, w and hm 16-byte aligned.  hipErrorInvalidValue for anything else, nothing launched.
struct SimpleHeadArgs {
    const uint16_t* y;
    const uint16_t* w;
    const float* bias;
    float* hm;
    int n, K, D;
    size_t rows;
};
hipError_t simple_head_launch(int dtype, const SimpleHeadArgs& a, hipStream_t s);

}  // namespace vp
