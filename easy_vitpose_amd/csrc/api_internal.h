// Internal header shared by the translation units behind the C ABI (include/vitpose_hip.h):
//   handle.hip       -- the handle: vp_create / vp_destroy, the switches, the guards of every entry, its modes (expert, flip-test), profiling, vp_synchronize
//   forward.hip      -- the forward of a chunk: gemm / gemm_fp8, forward_chunk, head_chunk, decode_chunk, run_chunk and its hipGraph cache
//   infer.hip        -- the inference entries and their staging (vp_infer*: host / device crops, the two slots, frames, boxes, experts and their per-crop plan, flip), stream adoption
//   group.hip        -- the multi-device group (vp_group*)
//   weights.hip      -- the weight packer (vp_load_weights: BN / LayerNorm folding, 16-bit / e4m3 conversion, deconv re-tiling)
//   tile_rules.hip   -- which GEMM tile runs a shape (pure host functions + their host-only taps)
//   debug_taps.hip   -- vp_dbg_*: one kernel on host data (parity tests), and the measurement build's timing taps
//   metrics.hip      -- the accumulating accuracy-metrics stage (vp_metrics_*: an object of its own beside the handle, like the tracker and the smoother)
//   simplehead.hip   -- the simple decoder's head (one kernel, simpleheadgeom.h), vp_head_kind and its two taps
//   cocoeval.hip     -- the accumulating COCO keypoint AP / AR stage (vp_cocoeval_*: an object of its own beside the handle, like the metrics stage)
//   hoststage.h      -- what the synchronous twins of every stage share: the scratch-block layout and HostStage (includes this header in its hipcc part)
//   stageobj.h       -- what the six stage objects share: StageObj, stage_create / _destroy / _download / _reset, mask_check (includes this header in its hipcc part)
// Everything here is library-internal (hidden visibility); nothing of it appears in the public headers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vitpose_hip.h"
#ifdef VP_TOOLS
#include "../../include/vitpose_hip_tools.h"
#endif
#include "kernels.h"
#include "mx8.h"

namespace vpi {

struct Block {
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;          // standalone-LayerNorm path only
    uint16_t *w_qkv, *w_proj, *w_fc1, *w_fc2;      // fused path: w_qkv / w_fc1 carry LayerNorm's gamma
    float *b_qkv, *b_proj, *b_fc1, *b_fc2;         // fused path: b_qkv / b_fc1 = W.beta + b
    float *s_qkv, *s_fc1;                          // fused path: row sums of the (rounded) folded weights
    uint16_t* w_qkvh = nullptr;                    // head dim 64: head-major copies for the fused qkv + attention kernel (qkvattn.hip)
    float *b_qkvh = nullptr, *s_qkvh = nullptr;
    // fp8 mode: e4m3 codes [rows padded to 256][K] + one fp32 scale per output channel (LayerNorm's gamma folded into qkv / fc1 first)
    uint8_t *w_qkv8 = nullptr, *w_fc18 = nullptr, *w_fc28 = nullptr, *w_proj8 = nullptr;   // w_proj8: head dim 64 only (the attention kernel's MXFP8 output)
    float *ws_qkv = nullptr, *ws_fc1 = nullptr, *ws_fc2 = nullptr, *ws_proj = nullptr;
};

// Every selection switch of a handle: read ONCE, at vp_create, by read_switches from the environment.  The chunk plan
// (tile_rules.hip plan_chunk) and the orchestration read them here, never the environment.  The defaults are the shipped paths.
struct Switches {
    int g8_stagger = 0;               // gemm8: start delay per XCD in sleep quanta (VP_G8_STAGGER)
    int gemm8_mask = 0x7;             // GEMMs on the 8-phase kernel at large batch: 1 fc2, 2 fc1, 4 qkv, 8 proj (VP_GEMM8; proj measured slower)
    long g8_min_tiles = 448;          // the 8-phase tile qualifies from this many tiles (1.75 per CU; tools build: VP_G8_MIN_TILES)
    bool persist_gemm = true;         // qkv / fc1 as persistent workgroups at large batch (VP_PERSIST=0: one tile per workgroup)
    int order_mask = 8;               // tile walk last-to-first per GEMM: bit0 qkv, bit1 proj, bit2 fc1, bit3 fc2 (VP_ORDER)
    bool blocked_hid = true;          // mlp hidden activations in the 64x64-blocked layout (VP_BLOCKED_HID=0: row-major)
    bool blocked_qkv = true;          // qkv in the same blocked layout when the head dim is 64 (a (crop, head) slab = three contiguous 8 KiB blocks; VP_BLOCKED_QKV=0: row-major)
    bool fuse_ln = true;              // LayerNorm folded into the GEMMs on both sides of it (VP_FUSE_LN=0: standalone passes)
    bool fuse_qkv_attn = true;        // attn.qkv + attention core in one kernel where the chunk plan picks it (VP_FUSE_QKV_ATTN=0: two launches)
    bool qa_min_set = false;          // VP_QA_MIN_TILES is given: it alone decides the head-dim-64 fused kernel (plan_chunk)
    long qa_min_tiles = 108;          // head dim 64: the fused kernel from this many (pair, head) tiles (VP_QA_MIN_TILES)
    long qa80_min_tiles = 192;        // head dim 80: the fused tile from this many (crop, head) tiles (VP_QA80_MIN_TILES; wins from 12 crops x 16 heads on, profiles/qkvattn80_r5.txt)
    int qa80_group = 8;               // head dim 80 fused tile: crops per group of the tile order (VP_QA80_GROUP)
    int attn_qsplit = 128;            // attention: three workgroups per (crop, head) up to this many (crop, head) pairs (VP_ATTN_QSPLIT; 0: never): B x 1 0.521 -> 0.495 ms,
                                      // L x 1 1.215 -> 1.152, B x 8 0.949 -> 0.906; neutral at 128 pairs, slower from 192 on
    int g8_bm192 = 3;                 // the 8-phase kernel's 192 x 256 tile is a candidate for: 1 = the residual GEMMs, 2 = the wide GEMMs (VP_G8_BM192)
    bool pad_batch = true;            // the encoder runs the next multiple of 4 crops where that buys an 8-phase tile (tile_rules.hip pick_run_batch; VP_PAD_BATCH=0: never)
    bool g8_cost_model = true;        // tile selection with the round-4 extensions (VP_G8_COST=0: the round-3 thresholds + the 192-row fallback)
    bool deconv_parity_fast = true;   // head: the four output parities of a deconv tile run side by side on one XCD (VP_DECONV_PARITY_FAST=0: parity-major launch order)
    bool fuse_head = true;            // VP_FUSE_HEAD=0: deconv2 and the final 1x1 conv as two launches at every batch size
    bool fp8_proj16 = false;          // fp8 mode, head dim 64: attn.proj stays on the fp16 kernels (VP_FP8_PROJ16=1)
    int graph_max_n = 16;             // chunks of up to this many crops are captured into a hipGraph and replayed (VP_GRAPH; 0 = off)
    bool graph_null = true;           // ... on a caller's legacy default stream too (VP_GRAPH_NULL=0: plain launches there)
    int caller_stream_max_n = 16;     // vp_infer_device_stream: batches up to this many crops launch on the caller's stream (VP_CALLER_STREAM=0: off)
    bool fold_rule = true;            // beyond graph_max_n_stats crops: fold per consumer where its tile keeps its occupancy with the statistics area (plan_chunk; off when VP_FOLD_STATS is set)
    int graph_max_n_stats = 8;        // batches of <= this many crops: the consumer GEMMs (qkv, fc1) merge the LayerNorm partial statistics of their tile rows
                                      // themselves (once per row and tile, in the prologue: gemm.hip) and the 2 x depth ln_finalize launches disappear -- same
                                      // ln_merge, bit-identical.  Measured (profiles/fold_stats_r3.txt): -7...-12 % per step at 1-8 crops, +0...+20 % at
                                      // 16-48 (every column tile merges its rows again): threshold 8.  VP_FOLD_STATS=n moves it (0 = always ln_finalize).
                                      // Round 6 (merge on a register copy, profiles/small_batch_r6.txt call 11): -2.6 ... -6.5 % against ln_finalize at 1-8 crops.
                                      // Round 6, call 25: the '+0 ... +20 %' beyond 8 crops was the statistics area behind the default tile's 80 KiB ring (one workgroup per CU
                                      // instead of two), not the merge: beyond this threshold each consumer folds on its own where its tile keeps its occupancy (fold_rule).
                                      // Round 2 merged per LANE in the epilogue (16 x redundant): slower than ln_finalize even at 8 crops (3.89 vs 2.97 ms).
    // split-K for the residual GEMMs of small batches (round 6; tile_rules.hip pick_splitk, gemm.hip EPI_PARTIAL, elementwise.hip splitk_reduce_kernel).
    // VP_SPLITK=0 switches it off (the parity test flips it); VP_SPLITK="fc2:S:variant,proj:S:variant" overrides the rule.
    bool splitk_on = true;
    int splitk_force[2][2] = {{0, 0}, {0, 0}};   // [0 = proj, 1 = fc2][S, variant]; S = 0: the rule decides
    int gemm_variant[VP_PROF_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // tile cfg per GEMM family, -1 = the rules (tools build: VP_GEMM_TUNE)
    int gemm_group_m[VP_PROF_COUNT] = {0};
    int fam_ablate[VP_PROF_COUNT] = {0};   // VP_TOOLS: per-family ablation / experiment bits in the forward pass (VP_ABLATE_FAM="fam:bits,...")
};

}  // namespace vpi

namespace vpi {
// The plan of one chunk with per-crop experts (HOST ONLY, a pure function of the chunk's ids: mix_plan): the crops in stable expert order -- position j holds caller
// row order[j] (chunk-local) of expert ids[j] -- and the run-length segments of that order: segment s = expert seg_e[s] at positions [seg_s[s], seg_s[s + 1]).
// pattern = GraphKey::mix (mix_pattern): 0 for one segment.
struct MixPlan {
    int nb = 0;
    std::vector<int32_t> order, ids;
    std::vector<int> seg_e, seg_s;
    uint64_t pattern = 0;
};
}  // namespace vpi

struct vp_ctx {
    vp_config cfg;
    vpi::Switches sw;
    int D, L, heads, Kp, dtype, maxb;
    hipStream_t stream = nullptr;
    std::string err;
    bool loaded = false;
    std::vector<void*> allocs;
    // weights
    uint16_t* w_patch = nullptr;
    float* pos = nullptr;
    std::vector<vpi::Block> blocks;
    float *lnf_g = nullptr, *lnf_b = nullptr;
    uint16_t *w_d1 = nullptr, *w_d2 = nullptr, *w_fin = nullptr;
    size_t fin_rows = 0;   // physical (hi/lo interleaved) rows of w_fin
    int head_kind = 0;     // 0 = the classic decoder (two deconvs + 1x1 conv), 1 = the simple decoder (simpleheadgeom.h): w_fin = its 9-tap hi / lo weight image of
                           // fin_rows rows per tap, b_fin its bias, w_d1 .. b_d2 unused (the d1 / d2 workspaces stay allocated)
    float *b_d1 = nullptr, *b_d2 = nullptr, *b_fin = nullptr, *b_zero = nullptr;
    uint16_t* zero = nullptr;
    // workspaces
    void* in_stage = nullptr;
    int32_t* wh_stage = nullptr;
    float* x = nullptr;
    uint16_t *y = nullptr, *qkv = nullptr, *hid = nullptr, *d1 = nullptr, *d2 = nullptr;
    float *hm = nullptr, *kp = nullptr, *tok = nullptr;
    float* hm_keep = nullptr;         // vp_infer_flip only: heatmaps of the un-flipped crops while the flipped pass runs
    int32_t* partner = nullptr;       // vp_infer_flip only: mirror joint per joint, rewritten per call (the MODE below has its own flip_table)
    // flip-test MODE (vp_set_flip_test): every chunk of run_chunk / vp_infer_heatmaps runs its crops and their mirror images as one interleaved batch of twice
    // the rows (elementwise.hip im2col_twin_kernel) and decodes the average without materialising it (decode.hip decode_kernel<true>).  A chunk then holds
    // max_batch / 2 of the caller's crops (chunk_cap).  flip_gen = 0 while off, a fresh value per vp_set_flip_test: part of the hipGraph key, since the table
    // and the shift are baked into a captured decode launch.  flip_table = the mode's own partner table (vp_infer_flip rewrites `partner` per call).
    bool flip_on = false;
    int flip_shift = 0;
    uint32_t flip_gen = 0, flip_counter = 0;
    int32_t* flip_table = nullptr;    // device [Kmax]
    std::vector<int32_t> flip_pairs;  // the pairs as given (a group compares its members' modes)
    // ... with one table per expert (vp_set_flip_test_experts, a ViTPose+ handle): flip_ex on top of flip_on, flip_tables = device [n_experts, Kmax], row e validated
    // against expert e's K (identity beyond it).  Every entry of the single-table mode reads the active expert's row (flip_table_now), vp_set_expert keeps the mode,
    // and the per-crop expert entries run under it: mix_chunk_body doubles the rows of the chunk's plan, the decode reads row e of each crop's record
    bool flip_ex = false;
    int32_t* flip_tables = nullptr;
    float *ln_part = nullptr, *rowstat = nullptr;   // partial row statistics [M][D/64][2], (mean, rstd) [M][2]
    // fp8 mode (vp_config.dtype = VP_DTYPE_FP8; csrc/mx8.h, gemm8f.hip, quant8.hip): qkv / fc1 / fc2 on MXFP8 operands.  Token rows are
    // padded to Mp (a multiple of the 256-row GEMM tile, >= 512); x8 / xs8 = LayerNorm(x) as MXFP8 codes / scales, hs8 = block scales of
    // the MXFP8 `hid` (its codes live in c->hid)
    bool fp8 = false;
    size_t Mp = 0;
    uint8_t *x8 = nullptr, *xs8 = nullptr, *hs8 = nullptr;
    uint8_t *y8 = nullptr, *ys8 = nullptr;          // head dim 64: the attention output as MXFP8 (A operand of the fp8 attn.proj)
    // asynchronous host path (vp_infer_submit / vp_infer_wait): two slots, each with its own device staging, so that the
    // H2D of call i+1 and the D2H of call i-1 run on the copy stream under the compute of call i
    struct Slot {
        void* in = nullptr; int32_t* wh = nullptr; float* kp = nullptr; hipEvent_t h2d = nullptr, done = nullptr, out = nullptr; bool busy = false;
        // staged download (the group path): the D2H lands in this pinned buffer and vp_infer_wait copies it to the caller's `user_out`,
        // so the submission never blocks on the compute whatever kind of host memory the caller owns
        float* host_kp = nullptr; float* user_out = nullptr; size_t out_bytes = 0;
        // staged upload (the group path with PAGEABLE caller memory): an asynchronous H2D from pageable memory is host-synchronous (the
        // runtime stages it and waits), so the crops go through this pinned buffer in pieces -- host memcpy of piece k+1 under the DMA of piece k
        char* host_in = nullptr; size_t host_in_cap = 0;
    };
    Slot slots[2];
    hipStream_t copy_stream = nullptr;   // H2D of the asynchronous path
    hipStream_t d2h_stream = nullptr;    // D2H on its own stream: an in-order copy stream would hold the next upload behind `wait compute; download`
    int next_slot = 0;
    // small batches: the whole forward + decode of a chunk captured once per key into a hipGraph and replayed (170+ launches of a few microseconds
    // each are launch-bound below ~16 crops); VP_GRAPH=0 disables.  The key = everything baked into the captured launches: a new field is one edit here
    // (run_chunk builds the key once per call, compares it on lookup and stores it on first sighting)
    struct GraphKey {
        int n = 0, fmt = -1;
        const void* src = nullptr; const int32_t* wh = nullptr; float* out = nullptr;
        int expert = 0;                  // a ViTPose+ handle's active expert (fc2 weights, head, K)
        const int32_t* post = nullptr;   // vp_infer_boxes_stream: the frame-offset kernel after the decode (its aux buffer; null: none)
        uint32_t flip = 0;               // the flip-test mode's generation the launches were captured under (flip_gen; 0: mode off)
        const float* cs = nullptr;       // the affine crop route: the decode reads (cx, cy, S_w, S_h) per crop here and writes frame pixels (null: the pad route's decode)
        // the per-crop expert entries (vp_infer_experts_device_stream, ...).  mix = the chunk's expert pattern, the count per expert in an exact encoding
        // (mix_pattern): with the crops in stable expert order the counts determine every launch -- the gather, the encoder's tile bounds, each head's rows -- and
        // the permutation lives in table buffers the launches only point at.  0 for every chunk that runs one expert.  wide: the decode goes the record route
        // into rows of Kmax joints (a one-expert chunk of those entries: the plain forward under key.expert, then that decode).  Both 0 / false on every other entry.
        uint64_t mix = 0;
        bool wide = false;
        bool operator==(const GraphKey& o) const {
            return n == o.n && fmt == o.fmt && src == o.src && wh == o.wh && out == o.out && expert == o.expert && post == o.post && flip == o.flip &&
                   cs == o.cs && mix == o.mix && wide == o.wide;
        }
    };
    struct GraphEntry { GraphKey key; hipGraphExec_t exec = nullptr; bool no_graph = false; };   // no_graph: capture or launch failed once, the key stays eager
    GraphEntry graphs[4];
    int graph_victim = 0;
    // split-K workspace of the residual GEMMs of small batches: fp32 partial products [S][M][D] of up to splitk_rows token rows (none when Switches::splitk_on is off)
    float* splitk_ws = nullptr;
    size_t splitk_rows = 0;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;   // vp_infer_device_stream: ordering against the caller's stream
    // vp_infer_device_stream at small batches (round 5): the launches go onto the CALLER's stream (c->stream points at it for the duration of that call) instead of
    // being fenced against it with two cross-stream events per call (~0.1 ms at 1-16 crops).  The handle's workspaces are then used from more than one stream over
    // time: `adopt_stream` orders a call behind the previous one whenever the stream changes.
    hipStream_t own_stream = nullptr;       // the handle's compute stream (== stream outside that call)
    const void* last_stream_id = nullptr;   // identity of the caller's stream the workspaces were last used on (compared, never dereferenced: the caller may have destroyed it)
    bool foreign_pending = false;           // the last user was a caller's stream: ev_sw, recorded behind its launches, is what work on any other stream waits for
    hipEvent_t ev_sw = nullptr;
    uint8_t* frame_stage = nullptr;   // staging arena of vp_infer_frames / vp_infer_frame: the row band of every host frame of the current call
    size_t frame_cap = 0;
    vp::CropRec* crecs = nullptr;     // per-crop source + geometry of the current chunk [max_batch]
    vp::AffRec* arecs = nullptr;      // the affine crop route (vp_infer_images_affine, vp_infer_boxes_affine_stream): per-crop source + inverse map of the current chunk [max_batch]
    float* cs_stage = nullptr;        // ... and its (cx, cy, S_w, S_h) rows, what the affine decode reads [max_batch][4]
    void* draw_ws = nullptr;          // vp_draw_poses_stream: the primitive records of the current call, VP_DRAW_MAX_RECORDS keys then as many bodies (drawgeom.h), allocated by vp_create
    void* label_ws = nullptr;         // vp_draw_labels_stream: the tag records of the current call, VP_LABEL_MAX_ROWS of 40 bytes (labelgeom.h), allocated by vp_create
    void* collect_ws = nullptr;       // vp_collect_stream: record index and id of every row of the current call, kept rows per frame (collect.hip CollectWs), allocated by vp_create
    int32_t* box_aux = nullptr;      // vp_infer_boxes_stream: per box of the current chunk (y0 - top_pad, x0 - left_pad, status, 0) [max_batch][4]
    // ViTPose+ (multi-dataset "mixture of experts") handle, vp_load_weights on a state dict with backbone.blocks.*.mlp.experts.*: mlp.fc2 of block l is one full
    // [D, 4D] matrix + [D] bias per expert (the split model's: shared rows then the expert's P rows), blocks[l].w_fc2 / b_fc2 point at expert 0 and expert e lies
    // e * fc2_w_stride / fc2_b_stride elements behind; one keypoint head per expert.  `expert` = the active one (vp_set_expert): its fc2 slice, its head and its
    // K (= Kp) serve every existing entry point.  Kmax sizes every buffer indexed by keypoint (== Kp on a plain handle).
    struct Head { uint16_t *w_d1 = nullptr, *w_d2 = nullptr, *w_fin = nullptr; float *b_d1 = nullptr, *b_d2 = nullptr, *b_fin = nullptr; size_t fin_rows = 0; int K = 0; };
    int Kmax = 0;
    int n_experts = 0, part_features = 0, expert = 0;
    size_t fc2_w_stride = 0, fc2_b_stride = 0;
    std::vector<Head> ex_heads;
    // the per-crop expert entries (vp_infer_experts and its device, frames and boxes twins): the chunk's tables on the device, written by mix_tables_launch from kernel
    // arguments in front of the chunk -- expert_ids [0, B) the expert of every encoder crop in expert order (padding crops repeat the last one) and [B, 2 B) the caller row of
    // every position (gather_crops_launch), mix_slot = the position of every caller row, mix_recs = the decode's records.  mix = the host plan of the chunk run_chunk is
    // running (null on every other entry): it shapes the launches of chunk_body
    int32_t* expert_ids = nullptr;
    void* mix_stage = nullptr;        // vp_infer_experts: the chunk's crops in the caller's order, before the gather
    size_t mix_stage_cap = 0;
    const int32_t* mix_expert = nullptr;   // set by mix_chunk_body around a mixed chunk's encoder, null otherwise: mlp.fc2 runs all experts in one launch (GemmArgs::expert) ...
    std::vector<int> mix_bounds;           // ... on tiles that never span two experts: the crop index of every expert change
    int32_t* mix_slot = nullptr;
    vp::MixRec* mix_recs = nullptr;
    vp::MixRecFlip* mix_recs_flip = nullptr;   // the decode's records under the per-expert flip-test mode (allocated by vp_set_flip_test_experts)
    const vpi::MixPlan* mix = nullptr;
    vpi::MixPlan mix_host;                         // the plan of the current chunk and the scratch of its tables: host memory that lives with the handle
    std::vector<int32_t> mix_ks, mix_first, mix_k;
    // profiling
    uint32_t prof = 0;   // bit f = time kernel family f
    int gemm_ablate = 0;   // profiling only
    struct Ev { hipEvent_t a, b; int fam; double flops, bytes; };
    std::vector<Ev> evs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    vp_profile acc{};
    std::string kernel_desc[VP_PROF_COUNT];   // name of the kernel the last launch of each family resolved to (vp_profile_kernel)
};

namespace vpi {

// ---- handle.hip
extern thread_local std::string g_create_error;

int fail(vp_ctx* c, int code, const std::string& msg);
// the guards the entries share.  need_weights: VP_ERR_INVALID without a handle, VP_ERR_STATE before vp_load_weights.  slots_idle: VP_ERR_STATE
// "<who> with a vp_infer_submit in flight ..." while a slot is busy.  quiesce: wait for everything enqueued on the handle's buffers, on a caller's stream too
int need_weights(vp_ctx* c);
bool slots_busy(const vp_ctx* c);
int slots_idle(vp_ctx* c, const char* who);
int quiesce(vp_ctx* c);
inline size_t crop_bytes(int fmt) { return (size_t)3 * 256 * 192 * (fmt == VP_INPUT_F32_NCHW ? 4 : 1); }

#define HIPCHK(c, expr)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return fail((c), VP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));   \
    } while (0)

template <class T> int dalloc(vp_ctx* c, T** p, size_t count) {
    void* q = nullptr;
    HIPCHK(c, hipMalloc(&q, count * sizeof(T) + 256));
    c->allocs.push_back(q);
    *p = (T*)q;
    return VP_OK;
}

// ---- weights.hip
uint16_t host_to_bits(float v, int dtype);     // fp32 -> 16-bit storage on the host (round to nearest even), same as the device paths
float host_from_bits(uint16_t h, int dtype);
size_t pad128(size_t n);
int upload_f32(vp_ctx* c, float** dst, const float* src, size_t n, size_t npad = 0);
int upload_mat(vp_ctx* c, uint16_t** dst, const float* src, size_t rows, size_t cols, size_t rows_pad);
int upload_final(vp_ctx* c, uint16_t** dst, const float* src, size_t kp, size_t cols, size_t* rows_phys);
// the simple decoder's final_layer.weight [K, D, 3, 3] as simpleheadgeom.h's weight image (HOST ONLY: img = 9 x sh_rows(K) x D codes), and its upload
void pack_simple_final(const float* src, int K, int D, int dtype, std::vector<uint16_t>& img);
int upload_simple_final(vp_ctx* c, uint16_t** dst, const float* src, int K, int D, size_t* rows_phys);
int upload_ln_folded(vp_ctx* c, uint16_t** w_out, float** s_out, float** c_out, const float* W, const float* b,
                     const float* gamma, const float* beta, size_t N, size_t K);
int upload_fp8_rows(vp_ctx* c, uint8_t** w_out, float** ws_out, float** c_out, const float* W, const float* b, const float* gamma,
                    const float* beta, size_t N, size_t K);

struct Lookup {
    std::unordered_map<std::string, const vp_tensor_desc*> map;
    vp_ctx* c;
    int get(const std::string& name, int64_t numel, const float** out) {
        auto it = map.find(name);
        if (it == map.end()) return fail(c, VP_ERR_MISSING_TENSOR, "missing key in state dict: " + name);
        if (it->second->numel != numel || it->second->data == nullptr)
            return fail(c, VP_ERR_SHAPE, "size mismatch for " + name + ": expected " + std::to_string(numel) +
                                             " elements, got " + std::to_string(it->second->numel));
        *out = it->second->data;
        return VP_OK;
    }
    bool has(const std::string& name) const { return map.count(name) != 0; }
    int64_t numel(const std::string& name) const { auto it = map.find(name); return it == map.end() ? -1 : it->second->numel; }
};

size_t final_rows(size_t kp);   // physical (hi/lo interleaved) rows of the final conv's weights for kp keypoints
int pack_deconv(vp_ctx* c, Lookup& lk, int idx, int Cin, uint16_t** w_out, float** b_out, const std::string& head = "keypoint_head");
void use_expert(vp_ctx* c, int e);   // make expert e of a ViTPose+ handle the active one (head pointers, Kp)

// ---- handle.hip
// flip-test mode (HOST ONLY): partner[k] = the mirror joint of k among K joints (k itself when unpaired) from n_pairs x 2 indices; VP_OK or VP_ERR_INVALID with the reason in *why
int flip_partner_table(int K, const int32_t* pairs, int n_pairs, int32_t* partner, std::string* why);
// the partner table the flip-test mode reads now: the handle's one table, or the active expert's row of the per-expert tables
inline const int32_t* flip_table_now(const vp_ctx* c) { return c->flip_ex ? c->flip_tables + (size_t)c->expert * c->Kmax : c->flip_table; }
bool prof_begin(vp_ctx* c, int fam, double flops, double bytes);
void prof_end(vp_ctx* c, bool on);
void prof_collect(vp_ctx* c);
void read_switches(Switches& s);      // the environment's switches (vp_create, vp_dbg_chunk_plan)
void apply_gemm_tuning(Switches& s);  // its VP_GEMM_TUNE part (tools build only): what the parity taps' contexts take

// ---- infer.hip
// the layout of one frame (HOST ONLY): VP_ERR_INVALID with "frame f ..." in *why for an unknown format, an unknown matrix or a null UV plane of an NV12 frame, a negative
// pitch, a pitch below the plane's row bytes (csrc/pixfmt.h plane_row_bytes).  Sizes and plane[0] are the callers' checks
int image_check(const vp_image& im, int f, std::string* why);
// vp_infer_images' plan (HOST ONLY): checks every crop of p9 [n, 9] against its frame (and, at the first crop that names it, the frame's layout: image_check),
// bands [n_frames, 2] = frame rows [row0, row1) its crops cover ({0, 0}: no crop; may be NULL).  VP_OK or VP_ERR_INVALID with the reason in *why
int image_plan(const vp_image* frames, int n_frames, const int32_t* p9, int n, int32_t* bands, std::string* why);
// the crops of p9 from frames as crop-kernel records: host frames are uploaded band by band into c->frame_stage (one copy per plane of a frame with
// crops: Y / RGB rows [row0, row1), UV rows [row0 >> 1, (row1 + 1) >> 1), at the caller's pitch), device frames are read in place (every plane checked to be device
// memory of the handle's device first).  recs[n] (host), enqueued on c->stream
int stage_frames(vp_ctx* c, const vp_image* frames, int n_frames, bool on_device, const int32_t* p9, int n, const int32_t* bands,
                 std::vector<vp::CropRec>& recs);
// its first half, shared with the affine route: row0_ptr[2 f + p] = plane p of frame f at the first row of its band (null: no band), staged or in place
int stage_bands(vp_ctx* c, const vp_image* frames, int n_frames, bool on_device, const int32_t* bands, std::vector<const uint8_t*>& row0_ptr);
// vp_infer_images_affine's plan (HOST ONLY): checks every crop (frame index, finite centre, 0 < S <= BOX_MAX_SIDE) and, at the first crop that names it, its frame;
// bands [n_frames, 2] = frame rows [row0, row1) its crops tap (affinegeom.h affine_row_band; {0, 0}: none; may be NULL).  VP_OK or VP_ERR_INVALID with the reason in *why
int affine_plan(const vp_image* frames, int n_frames, const int32_t* frame_idx, const float* cs, int n, int32_t* bands, std::string* why);
// the crops of (frame_idx, cs) as affine crop records over the bands stage_bands placed
void affine_records(const vp_image* frames, const int32_t* frame_idx, const float* cs, int n, const int32_t* bands, const std::vector<const uint8_t*>& row0_ptr,
                    std::vector<vp::AffRec>& recs);
// vp_infer_boxes_stream / vp_dbg_box_geometry (HOST ONLY): the host arguments of a boxes call (sizes of every frame, row stride, pad, counts).
// VP_OK or VP_ERR_INVALID with the reason in *why
int box_args(int n_frames, const int32_t* frame_hw, int hw_stride, int row_stride, int n, int pad, std::string* why);
// the per-crop expert entries (HOST ONLY).  mix_check_ids: VP_ERR_INVALID with the reason in *why for null ids or an id outside [0, n_experts), naming the crop
// (every entry checks the whole call with it before anything is enqueued).  mix_plan: checked ids [nb] of one chunk -> p (reused from chunk to chunk).
// mix_pattern: the exact code of the counts per expert -- 8 bits each for up to 8 experts of up to 254 crops, 0 for a chunk of one expert, MIX_NO_GRAPH where the
// counts do not fit (such a chunk runs eagerly).  mix_records: MixRec's first / K of every position [nb] -- the head of segment s writes its maps [cnt, K_e, 64, 48]
// from map seg_s[s] * Kmax on (k_per_expert [n_experts])
constexpr uint64_t MIX_NO_GRAPH = ~(uint64_t)0;
int mix_check_ids(const int32_t* ids, int n, int n_experts, std::string* why);
void mix_plan(const int32_t* ids, int nb, int n_experts, MixPlan& p);
uint64_t mix_pattern(const std::vector<int>& seg_e, const std::vector<int>& seg_s, int n_experts);
void mix_records(const MixPlan& p, const int32_t* k_per_expert, int Kmax, int32_t* first, int32_t* K);
// ... under the per-expert flip-test mode: position j is forward rows 2 j (the crop) and 2 j + 1 (its mirror), the head of segment s writes [2 cnt, K_e, 64, 48] from map
// 2 seg_s[s] * Kmax on, so first = 2 seg_s[s] * Kmax + 2 (j - seg_s[s]) * K_e (the mirror's maps start K_e behind)
void mix_records_flip(const MixPlan& p, const int32_t* k_per_expert, int Kmax, int32_t* first, int32_t* K);
// vp_infer_submit; stage_out (the group path): the download lands in the slot's pinned buffer and vp_infer_wait copies it to `out`
int submit_impl(vp_ctx* c, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out, int32_t* slot_out, bool stage_out);

#define LAUNCH(c, fam, flops, bytes, expr)   \
    do {                                     \
        const bool on__ = prof_begin((c), (fam), (flops), (bytes)); \
        hipError_t e__ = (expr);             \
        prof_end((c), on__);                 \
        if (e__ != hipSuccess)               \
            return fail((c), VP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

struct LnFuse {
    bool a_blocked = false, out_blocked = false, reverse = false;   // 64x64-blocked activation layout on the A / output side (kernels.h)
    size_t plane = 0;                 // producer: elements between the hi and lo planes of the residual stream
    float* stats_out = nullptr;       // producer: partial row statistics
    const float* rowstat = nullptr;   // consumer: (mean, rstd) per row
    const float* ln_s = nullptr;      // consumer: row sums of the folded weights
    const float* ln_part = nullptr;   // consumer at small batch: the producer's partial statistics instead of rowstat
    int ln_tiles = 0;
    int* tiles_out = nullptr;         // producer: number of n-tiles written per row
};

// ---- tile_rules.hip: which kernel runs each GEMM of a chunk (pure host code)
constexpr int SPLITK_MAX_S = 8, SPLITK_MAX_CROPS = 32;
// the complete choice for one GEMM: gemm.hip Cfg id (16 / 17 / 18 = the 8-phase kernel's 256 x 256 / 256 x 192 / 192 x 256 tile; on an fp8 GEMM 16 / 17 = the MXFP8
// kernel's 256 x 256 / 256 x 192), tile-order group, persistent workgroups, start stagger; splitk > 1: that many partial products on Cfg splitk_variant + the reduction
struct GemmPick { int variant = -1, group_m = 0, persist = 0, stagger = 0, splitk = 1, splitk_variant = 0; };
// fam = VP_PROF_* family, epi = kernels.h GemmEpi, [M, N] x K with ldo = N; ln_part = a LayerNorm consumer that folds the partial statistics itself;
// splitk_rows = the rows the split-K workspace holds (0: none); mix_bounds = a ViTPose+ mixed batch's expert changes (nullptr: one expert)
GemmPick resolve_gemm(const Switches& s, int fam, int epi, int M, int N, int K, bool ln_part = false, size_t splitk_rows = 0,
                      const std::vector<int>* mix_bounds = nullptr);
GemmPick resolve_gemm_fp8(int fam, int epi, int Mp, int N);   // fp8 mode: qkv / fc1 / fc2 (and attn.proj at head dim 64) on the MXFP8 kernel
enum QkvPath { QKV_GEMM = 0, QKV_ATTN64 = 1, QKV_ATTN80 = 2 };   // attn.qkv GEMM + attention kernel; fused: qkvattn.hip (head dim 64) / gemm8.hip EPI_QKV_ATTN (head dim 80)
struct HeadPlan {
    int kind = 0;                     // vp_ctx::head_kind: 1 = the simple decoder's one launch (simplehead.hip), nothing below applies
    bool fused = false;               // deconv2 + the final 1x1 conv in one kernel (EPI_DECONV_FINAL)
    GemmPick deconv1, deconv2, final;  // final: unused when fused
};
struct ChunkPlan {
    int n = 0;                        // crops the encoder runs (>= the chunk's: padding crops repeat the last one)
    bool fold1 = false, fold2 = false;   // LayerNorm-1 / -2: attn.qkv / mlp.fc1 merge the partial statistics themselves (no ln_finalize launch)
    int qkv_path = QKV_GEMM;
    bool attn_qsplit = false;         // the attention kernel on three workgroups per (crop, head)
    bool proj_fp8 = false;            // fp8 mode: attn.proj on the MXFP8 kernel too (the attention kernel writes MXFP8)
    GemmPick gemm[VP_PROF_COUNT];     // the encoder GEMMs by family: PATCH, QKV, PROJ, FC1, FC2
    HeadPlan head;                    // the head of the chunk's crops
};
// fin_rows = physical rows of the final conv's weights (final_rows); mix_bounds as in resolve_gemm; head_kind = vp_ctx::head_kind
ChunkPlan plan_chunk(const Switches& s, int D, int heads, int max_batch, bool fp8, int n_in, size_t fin_rows, const std::vector<int>* mix_bounds = nullptr,
                     int head_kind = 0);
HeadPlan plan_head(const Switches& s, int D, int nh, size_t fin_rows, int head_kind = 0);

// ---- forward.hip: one GEMM of the path as `pk` resolved it (also what the vp_dbg_gemm* taps launch).  EPI_DECONV_FINAL: `out` = the fp32 heatmaps
int gemm(vp_ctx* c, int fam, int epi, const GemmPick& pk, const uint16_t* A, const uint16_t* W, const float* bias, void* out,
         const float* aux, int M, int N, int K, int ldo, int Hin = 0, int Win = 0, int Cin = 0, const LnFuse* ln = nullptr);
// ... and the arguments it launches with (vp_dbg_head_case launches the head's GEMMs from the same function)
vp::GemmArgs gemm_args(const vp_ctx* c, int fam, int epi, const GemmPick& pk, const uint16_t* A, const uint16_t* W, const float* bias, void* out,
                       const float* aux, int M, int N, int K, int ldo, int Hin = 0, int Win = 0, int Cin = 0, const LnFuse* ln = nullptr);
int gemm_fp8(vp_ctx* c, int fam, int epi, const GemmPick& pk, const uint8_t* A8, const uint8_t* a_scales, const uint8_t* W8, const float* w_scale, const float* bias,
             void* out, uint8_t* out_scales, const float* aux, int M, int N, int K, const LnFuse* ln);
// what a forward_chunk call asks for beyond the plain forward to heatmaps in c->hm
struct FwdOpts {
    bool tokens = false;   // also keep last_norm's fp32 tokens in c->tok (vp_infer_tokens)
    bool mirror = false;   // the crops are read mirrored left-right (vp_infer_flip's second pass)
    bool head = true;      // false: the encoder and last_norm only, tokens in c->y (mix_chunk_body runs the head per expert segment)
    int twin_src = 0;      // > 0 (flip-test mode): n_in = 2 * twin_src rows, the twin_src crops at d_crops interleaved with their mirror images (crop, mirror, crop, mirror, ...)
};
int forward_chunk(vp_ctx* c, const void* d_crops, int fmt, int n_in, const FwdOpts& o = FwdOpts());
int head_chunk(vp_ctx* c, const uint16_t* y, int nh, float* hm, const HeadPlan& hp);
int decode_chunk(vp_ctx* c, const int32_t* d_wh, float* d_out, int n, bool twin, const float* d_cs = nullptr);   // d_cs: the affine route's decode (d_wh unused)
int chunk_cap(const vp_ctx* c);
int chunk_rows(const vp_ctx* c, int nb);
int forward_mode_chunk(vp_ctx* c, const void* d_src, int fmt, int nb);
int run_chunk(vp_ctx* c, const void* d_src, int fmt, int nb, const int32_t* d_wh, float* d_out, const int32_t* post = nullptr, const float* d_cs = nullptr);

}  // namespace vpi
