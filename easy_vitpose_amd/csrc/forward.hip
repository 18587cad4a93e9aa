// The forward of one chunk behind the C ABI (include/vitpose_hip.h): the GEMM launchers, the encoder + head + decode of up to max_batch crops as the
// chunk's plan (tile_rules.hip plan_chunk) picked them, and the hipGraph cache that replays small chunks (run_chunk).
#include "api_internal.h"
#include "hoststage.h"
#include "simpleheadgeom.h"
#include "tiles.h"

using namespace vpi;

namespace vpi {

// the name of the kernel a launch of family fam resolved to, when the launch code gave one (vp_profile_kernel reports the LAST launch)
static void note_kernel(vp_ctx* c, int fam, const char* desc) {
    if (desc[0] && c->kernel_desc[fam] != desc) c->kernel_desc[fam] = desc;
}

// the launch arguments of one 2-phase / 8-phase GEMM of the path as `pk` resolved it: everything gemm() hands to vp::gemm_launch but the kernel-name buffer
// (also what vp_dbg_head_case launches, so that the tap cannot drift from the path)
vp::GemmArgs gemm_args(const vp_ctx* c, int fam, int epi, const GemmPick& pk, const uint16_t* A, const uint16_t* W, const float* bias, void* out,
                       const float* aux, int M, int N, int K, int ldo, int Hin, int Win, int Cin, const LnFuse* ln) {
    vp::GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.out = out; g.aux = aux;
    g.M = M; g.N = N; g.K = K; g.ldo = ldo;
    g.Hin = Hin; g.Win = Win; g.Cin = Cin; g.zero = c->zero; g.Kp = c->Kp;
    g.w_rows = (int)pad128((size_t)N);
    g.variant = pk.variant; g.group_m = pk.group_m; g.persist = pk.persist; g.stagger = pk.stagger;
    g.ablate = c->gemm_ablate | c->sw.fam_ablate[fam];
    g.parity_fast = c->sw.deconv_parity_fast;
    if (c->mix_expert && fam == VP_PROF_GEMM_FC2) g.expert = c->mix_expert;   // expert e's fc2 lies e * w_rows * K / e * w_rows behind (weights.hip upload_fc2_experts: w_rows = pad128(D))
    if (ln) {
        g.a_blocked = ln->a_blocked; g.out_blocked = ln->out_blocked; g.reverse = ln->reverse;
        g.plane = ln->plane; g.stats_out = ln->stats_out; g.rowstat = ln->rowstat; g.ln_s = ln->ln_s;
        g.ln_part = ln->ln_part; g.ln_tiles = ln->ln_tiles; g.ln_inv_d = 1.0f / (float)K;
    }
    if (epi == vp::EPI_DECONV_FINAL) { g.W2 = c->w_fin; g.bias2 = c->b_fin; g.out2 = (float*)out; g.out = nullptr; }   // deconv2 + final 1x1 conv in one kernel: `out` = the heatmaps, nothing else is written
    return g;
}

int gemm(vp_ctx* c, int fam, int epi, const GemmPick& pk, const uint16_t* A, const uint16_t* W, const float* bias, void* out,
         const float* aux, int M, int N, int K, int ldo, int Hin, int Win, int Cin, const LnFuse* ln) {
    vp::GemmArgs g = gemm_args(c, fam, epi, pk, A, W, bias, out, aux, M, N, K, ldo, Hin, Win, Cin, ln);
    if (ln && ln->tiles_out) *ln->tiles_out = N / 64;   // partial statistics are written per 64 columns, whatever the tile
    const bool deconv = epi == vp::EPI_DECONV || epi == vp::EPI_DECONV_FINAL;
    const double par = deconv ? 4.0 : 1.0;
    const double Nalg = (epi == vp::EPI_HEATMAP) ? (double)c->Kp : (double)N;   // heatmap: N counts the hi + lo weight rows
    double flops = 2.0 * M * Nalg * K * par;
    // algorithmic HBM bytes: each operand once, output once (+ residual read)
    const bool resid = epi == vp::EPI_BIAS_RESID || epi == vp::EPI_BIAS_RESID_LN;
    const bool f32out = resid || epi == vp::EPI_POS || epi == vp::EPI_POS_LN || epi == vp::EPI_HEATMAP;
    const double out_b = f32out ? 4.0 : 2.0;
    double bytes = 2.0 * M * (double)(deconv ? Cin : K) + 2.0 * N * (double)K * par + out_b * M * Nalg * par;
    if (epi == vp::EPI_DECONV_FINAL) {   // the 256-channel activations never reach HBM; the final conv's flops and the fp32 heatmaps count
        flops += 2.0 * M * par * (double)c->Kp * N;
        bytes += (4.0 * c->Kp - out_b * N) * M * par + 2.0 * c->fin_rows * N;
    }
    if (resid) bytes += 4.0 * M * (double)N;
    if (epi == vp::EPI_BIAS_RESID_LN || epi == vp::EPI_POS_LN) bytes += 8.0 * M * (double)(N / 64);   // partial row statistics
    char desc[192];
    desc[0] = 0;
    g.desc = desc; g.desc_cap = (int)sizeof(desc);   // the launch code names the kernel it resolved to (one snprintf per GEMM launch: vp_profile_kernel reports the LAST launch)
    // small batches: a residual GEMM as S partial products over k ranges + a fixed-order reduction (tile_rules.hip pick_splitk), x updated in place
    if (pk.splitk > 1) {
        if (out != (void*)aux || (size_t)M > c->splitk_rows || !c->splitk_ws) return fail(c, VP_ERR_INVALID, "split-K: a residual GEMM in place within the workspace only");
        vp::GemmArgs p = g;
        p.out = c->splitk_ws; p.aux = nullptr; p.bias = nullptr; p.stats_out = nullptr; p.plane = 0;
        p.variant = pk.splitk_variant; p.group_m = 0; p.splitk = pk.splitk; p.ldo = N; p.persist = 0;
        LAUNCH(c, fam, flops, bytes, vp::gemm_launch(c->dtype, vp::EPI_PARTIAL, p, c->stream));   // (flops / bytes stay the algorithmic figures of the GEMM; the partials' round trip is overhead)
        if (desc[0]) {
            char d2[224];
            snprintf(d2, sizeof(d2), "%s x split-K %d + splitk_reduce_kernel", desc, pk.splitk);
            note_kernel(c, fam, d2);
        }
        LAUNCH(c, fam, 0.0, 0.0, vp::splitk_reduce_launch(c->dtype, c->splitk_ws, pk.splitk, bias, (uint16_t*)out, g.plane, g.stats_out, M, N, c->stream));
        return VP_OK;
    }
    LAUNCH(c, fam, flops, bytes, vp::gemm_launch(c->dtype, epi, g, c->stream));
    note_kernel(c, fam, desc);
    return VP_OK;
}

// fp8 mode: one encoder GEMM on MXFP8 operands (gemm8f.hip).  epi: EPI_BIAS (qkv -> 16-bit), EPI_BIAS_GELU (fc1 -> MXFP8 codes at `out`,
// block scales at out_scales), EPI_BIAS_RESID_LN (fc2: two-plane residual + row statistics).  M = padded token rows (multiple of 256).
int gemm_fp8(vp_ctx* c, int fam, int epi, const GemmPick& pk, const uint8_t* A8, const uint8_t* a_scales, const uint8_t* W8, const float* w_scale, const float* bias,
             void* out, uint8_t* out_scales, const float* aux, int M, int N, int K, const LnFuse* ln) {
    vp::GemmArgs g{};
    g.A = (const uint16_t*)A8; g.W = (const uint16_t*)W8; g.bias = bias; g.out = out; g.aux = aux;
    g.M = M; g.N = N; g.K = K; g.ldo = N;
    g.a_scales = a_scales; g.w_scale = w_scale; g.out_scales = out_scales;
    g.w_rows = (int)pad128((size_t)N);
    if (ln) {
        g.out_blocked = ln->out_blocked; g.reverse = ln->reverse;
        g.plane = ln->plane; g.stats_out = ln->stats_out;
        if (ln->tiles_out) *ln->tiles_out = N / 64;
    }
    const int bn = vp::tile8_bn(pk.variant);   // tile_rules.hip resolve_gemm_fp8 (0 = not an 8-phase tile: refused below)
    g.group_m = pk.group_m;
    if (!vp::gemm8f_supported(epi, g, bn))
        return fail(c, VP_ERR_SHAPE, "fp8 mode: GEMM shape " + std::to_string(M) + " x " + std::to_string(N) + " x " + std::to_string(K) + " not supported by the MXFP8 kernel");
    const double flops = 2.0 * M * (double)N * K;
    double bytes = 1.0 * M * (double)K + M * (double)(K / 32) + 1.0 * N * (double)K;      // codes + block scales + weight codes
    bytes += epi == vp::EPI_BIAS ? 2.0 * M * (double)N : epi == vp::EPI_BIAS_GELU ? (1.0 + 1.0 / 32) * M * (double)N : 8.0 * M * (double)N + 8.0 * M * (double)(N / 64);
    char desc[192];
    desc[0] = 0;
    g.desc = desc; g.desc_cap = (int)sizeof(desc);
    LAUNCH(c, fam, flops, bytes, vp::gemm8f_launch(epi, g, bn, c->stream));
    note_kernel(c, fam, desc);
    return VP_OK;
}

// fc2 weights / bias of block b for the active expert (a ViTPose+ handle outside a mixed batch; expert 0 = the only one of a plain handle)
static const uint16_t* fc2_w(const vp_ctx* c, const vpi::Block& b) { return c->mix_expert ? b.w_fc2 : b.w_fc2 + (size_t)c->expert * c->fc2_w_stride; }
static const float* fc2_b(const vp_ctx* c, const vpi::Block& b) { return c->mix_expert ? b.b_fc2 : b.b_fc2 + (size_t)c->expert * c->fc2_b_stride; }

// forward of one chunk (n <= max_batch) with device-resident crops; heatmaps land in c->hm (FwdOpts, api_internal.h: what a call may ask for instead).
// Executes the chunk's plan (tile_rules.hip plan_chunk): which kernel runs each GEMM, the encoder batch, the LayerNorm folds, the qkv path.
// Under o.twin_src everything behind the patch gather is the plain forward of an n_in-crop batch.
int forward_chunk(vp_ctx* c, const void* d_crops, int fmt, int n_in, const FwdOpts& o) {
    const int D = c->D;
    const ChunkPlan pl = plan_chunk(c->sw, D, c->heads, c->maxb, c->fp8, n_in, c->fin_rows, c->mix_expert ? &c->mix_bounds : nullptr, c->head_kind);
    const GemmPick* pk = pl.gemm;
    const int n = pl.n;   // rows n_in .. n - 1 of a padded encoder batch repeat the last crop and are never read by the head
    const int M = n * 192;
    const double in_b = (fmt == VP_INPUT_F32_NCHW ? 4.0 : 1.0) * n_in * 3.0 * 256 * 192;
    if (o.twin_src) LAUNCH(c, VP_PROF_IM2COL, 0.0, 0.5 * in_b + 2.0 * M * 768, vp::im2col_twin_launch(c->dtype, d_crops, fmt, c->hid, n, o.twin_src, c->stream));
    else LAUNCH(c, VP_PROF_IM2COL, 0.0, in_b + 2.0 * M * 768, vp::im2col_launch(c->dtype, d_crops, fmt, c->hid, n, c->stream, o.mirror, n_in));
    int rc;
    size_t plane = 0;   // != 0: the residual stream c->x is held as two 16-bit planes (fused-LayerNorm path)
    const bool qkv_blocked = c->sw.blocked_qkv && D / c->heads == 64;
    auto attention = [&](uint16_t* out, double bytes, uint8_t* mx_scales) -> int {
        LAUNCH(c, VP_PROF_ATTN, 4.0 * 192 * 192 * (double)D * n, bytes,
               vp::attention_launch(c->dtype, c->qkv, out, n, D, c->heads, c->stream, pl.attn_qsplit, qkv_blocked ? 1 : 0, mx_scales));
        return VP_OK;
    };
    if (c->fp8) {
        // fp8 mode.  The residual stream, the attention core, attn.proj, the head and the decode are the fp16 path's; qkv / fc1 / fc2 run
        // on MXFP8 operands.  Token rows are padded to Mp (multiple of the 256-row tile, >= 512): padding rows carry zeros into the
        // GEMMs and are never read by a kernel that works per crop.
        const int Mp = (int)std::max<size_t>(up256((size_t)M), 512);
        plane = c->Mp * (size_t)D;                   // the planes are laid out for the handle's full padded row count
        uint16_t* xh = (uint16_t*)c->x;
        int tiles = 0;
        LnFuse prod; prod.plane = plane; prod.stats_out = c->ln_part; prod.tiles_out = &tiles;
        auto quant = [&]() -> int {                  // LayerNorm(x) -> MXFP8 (replaces ln_finalize; gamma / beta live in the consumer's weights / bias)
            LAUNCH(c, VP_PROF_LAYERNORM, 0.0, 8.0 * M * tiles + 2.0 * M * D + (1.0 + 1.0 / 32) * Mp * (double)D,
                   vp::ln_quant_launch(c->dtype, xh, c->ln_part, tiles, c->x8, c->xs8, M, Mp, D, c->stream));
            return VP_OK;
        };
        if ((rc = gemm(c, VP_PROF_GEMM_PATCH, vp::EPI_POS_LN, pk[VP_PROF_GEMM_PATCH], c->hid, c->w_patch, c->b_zero, c->x, c->pos, M, D, 768, D, 0, 0, 0, &prod))) return rc;
        for (int l = 0; l < c->L; ++l) {
            const Block& b = c->blocks[l];
            if ((rc = quant())) return rc;
            LnFuse cq; cq.out_blocked = qkv_blocked;
            if ((rc = gemm_fp8(c, VP_PROF_GEMM_QKV, vp::EPI_BIAS, pk[VP_PROF_GEMM_QKV], c->x8, c->xs8, b.w_qkv8, b.ws_qkv, b.b_qkv, c->qkv, nullptr, nullptr, Mp, 3 * D, D, &cq))) return rc;
            LnFuse pp = prod;
            if (pl.proj_fp8) {   // head dim 64: attention writes MXFP8, attn.proj runs on the fp8 kernel too
                if ((rc = attention((uint16_t*)c->y8, 7.0 * M * D, c->ys8))) return rc;
                if ((rc = gemm_fp8(c, VP_PROF_GEMM_PROJ, vp::EPI_BIAS_RESID_LN, pk[VP_PROF_GEMM_PROJ], c->y8, c->ys8, b.w_proj8, b.ws_proj, b.b_proj, c->x, nullptr, c->x, Mp, D, D, &pp))) return rc;
            } else {
                if ((rc = attention(c->y, 8.0 * M * D, nullptr))) return rc;
                if ((rc = gemm(c, VP_PROF_GEMM_PROJ, vp::EPI_BIAS_RESID_LN, pk[VP_PROF_GEMM_PROJ], c->y, b.w_proj, b.b_proj, c->x, c->x, M, D, D, D, 0, 0, 0, &pp))) return rc;
            }
            if ((rc = quant())) return rc;
            if ((rc = gemm_fp8(c, VP_PROF_GEMM_FC1, vp::EPI_BIAS_GELU, pk[VP_PROF_GEMM_FC1], c->x8, c->xs8, b.w_fc18, b.ws_fc1, b.b_fc1, c->hid, c->hs8, nullptr, Mp, 4 * D, D, nullptr))) return rc;
            LnFuse p2 = prod;
            if ((rc = gemm_fp8(c, VP_PROF_GEMM_FC2, vp::EPI_BIAS_RESID_LN, pk[VP_PROF_GEMM_FC2], (const uint8_t*)c->hid, c->hs8, b.w_fc28, b.ws_fc2, b.b_fc2, c->x, nullptr, c->x, Mp, D, 4 * D, &p2))) return rc;
        }
    } else if (c->sw.fuse_ln) {
        // LayerNorm folded into the GEMMs on both sides of it.  The residual stream is kept as two 16-bit planes
        // (x = hi + lo, same bytes as fp32, >= 22 significant bits): every producer (patch embed, attn.proj,
        // mlp.fc2) writes the planes + partial row statistics, a tiny kernel folds those into (mean, rstd), and
        // qkv / fc1 multiply the hi plane -- the UN-normalised rows -- by gamma-folded weights and normalise in
        // their epilogue.  Saves the 151 MB read + 75 MB write of 24 of the 25 LayerNorm passes.  Where the plan folds (fold1 / fold2), the consumer
        // merges the partial statistics itself and the ln_finalize launch disappears.
        plane = (size_t)M * D;
        uint16_t* xh = (uint16_t*)c->x;
        int tiles = 0;
        LnFuse prod; prod.plane = plane; prod.stats_out = c->ln_part; prod.tiles_out = &tiles;
        auto finalize = [&](bool folded) -> int {
            if (folded) return VP_OK;
            LAUNCH(c, VP_PROF_LAYERNORM, 0.0, 8.0 * M * tiles + 8.0 * M, vp::ln_finalize_launch(c->ln_part, c->rowstat, M, tiles, D, c->stream));
            return VP_OK;
        };
        const double qkv_attn_flops = 2.0 * M * 3.0 * D * D + 4.0 * 192 * 192 * (double)D * n, qkv_attn_bytes = 2.0 * M * D + 2.0 * 3 * D * (double)D + 2.0 * M * D;
        if ((rc = gemm(c, VP_PROF_GEMM_PATCH, vp::EPI_POS_LN, pk[VP_PROF_GEMM_PATCH], c->hid, c->w_patch, c->b_zero, c->x, c->pos, M, D, 768, D, 0, 0, 0, &prod))) return rc;
        if ((rc = finalize(pl.fold1))) return rc;
        for (int l = 0; l < c->L; ++l) {
            const Block& b = c->blocks[l];
            if (pl.qkv_path == QKV_ATTN80) {   // one crop x one head per 192 x 256 tile of the 8-phase kernel (gemm8.hip EPI_QKV_ATTN)
                vp::GemmArgs g80{};
                g80.A = xh; g80.W = b.w_qkvh; g80.bias = b.b_qkvh; g80.ln_s = b.s_qkvh; g80.rowstat = c->rowstat; g80.out = c->y;
                g80.M = M; g80.N = c->heads * 256; g80.K = D; g80.ldo = D; g80.w_rows = c->heads * 256; g80.variant = 18;
                // tile order: groups of 8 crops x all heads, crop fastest -- the 32 workgroups of an XCD then work on 8 crops x 4 heads at a time (12 operand K-slices
                // fetched per K-tile for 32 tiles instead of 18 with the head-fastest order: PMC traffic 800 -> ~450 MB per launch, profiles/qkvattn80_r5.txt)
                g80.group_m = c->sw.qa80_group;
                g80.attn_scale_log2e = vp::softmax_scale_log2e(80);
                g80.ablate = c->gemm_ablate | c->sw.fam_ablate[VP_PROF_GEMM_QKV];
                char desc[192];
                desc[0] = 0;
                g80.desc = desc; g80.desc_cap = (int)sizeof(desc);
                LAUNCH(c, VP_PROF_GEMM_QKV, qkv_attn_flops, qkv_attn_bytes, vp::gemm_launch(c->dtype, vp::EPI_QKV_ATTN, g80, c->stream));
                note_kernel(c, VP_PROF_GEMM_QKV, desc);
            } else if (pl.qkv_path == QKV_ATTN64) {   // one pair of crops x one head per tile (qkvattn.hip; an odd batch's last crop fills both halves of its pair)
                vp::QkvAttnArgs qa{};
                qa.x_hi = xh; qa.wh = b.w_qkvh; qa.bh = b.b_qkvh; qa.sh = b.s_qkvh; qa.rowstat = c->rowstat; qa.y = c->y;
                qa.npairs = (n + 1) / 2; qa.ncrops = n; qa.heads = c->heads; qa.D = D;
                qa.scale_log2e = vp::softmax_scale_log2e(64);
                char desc[96];
                desc[0] = 0;
                LAUNCH(c, VP_PROF_GEMM_QKV, qkv_attn_flops, qkv_attn_bytes, vp::qkvattn_launch(c->dtype, qa, c->stream, desc, (int)sizeof(desc)));
                note_kernel(c, VP_PROF_GEMM_QKV, desc);
            } else {
                LnFuse cq; cq.rowstat = c->rowstat; cq.ln_s = b.s_qkv; cq.reverse = (c->sw.order_mask & 1) != 0; cq.out_blocked = qkv_blocked;
                if (pl.fold1) { cq.rowstat = nullptr; cq.ln_part = c->ln_part; cq.ln_tiles = D / 64; }
                if ((rc = gemm(c, VP_PROF_GEMM_QKV, vp::EPI_BIAS, pk[VP_PROF_GEMM_QKV], xh, b.w_qkv, b.b_qkv, c->qkv, nullptr, M, 3 * D, D, 3 * D, 0, 0, 0, &cq))) return rc;
                if ((rc = attention(c->y, 8.0 * M * D, nullptr))) return rc;
            }
            LnFuse pp = prod; pp.reverse = (c->sw.order_mask & 2) != 0;
            if ((rc = gemm(c, VP_PROF_GEMM_PROJ, vp::EPI_BIAS_RESID_LN, pk[VP_PROF_GEMM_PROJ], c->y, b.w_proj, b.b_proj, c->x, c->x, M, D, D, D, 0, 0, 0, &pp))) return rc;
            if ((rc = finalize(pl.fold2))) return rc;
            LnFuse c1; c1.rowstat = c->rowstat; c1.ln_s = b.s_fc1; c1.out_blocked = c->sw.blocked_hid; c1.reverse = (c->sw.order_mask & 4) != 0;
            if (pl.fold2) { c1.rowstat = nullptr; c1.ln_part = c->ln_part; c1.ln_tiles = D / 64; }
            if ((rc = gemm(c, VP_PROF_GEMM_FC1, vp::EPI_BIAS_GELU, pk[VP_PROF_GEMM_FC1], xh, b.w_fc1, b.b_fc1, c->hid, nullptr, M, 4 * D, D, 4 * D, 0, 0, 0, &c1))) return rc;
            LnFuse p2 = prod; p2.a_blocked = c->sw.blocked_hid; p2.reverse = (c->sw.order_mask & 8) != 0;
            if ((rc = gemm(c, VP_PROF_GEMM_FC2, vp::EPI_BIAS_RESID_LN, pk[VP_PROF_GEMM_FC2], c->hid, fc2_w(c, b), fc2_b(c, b), c->x, c->x, M, D, 4 * D, D, 0, 0, 0, &p2))) return rc;
            if (l + 1 < c->L && (rc = finalize(pl.fold1))) return rc;   // last block: last_norm below is a standalone pass
        }
    } else {
    if ((rc = gemm(c, VP_PROF_GEMM_PATCH, vp::EPI_POS, pk[VP_PROF_GEMM_PATCH], c->hid, c->w_patch, c->b_zero, c->x, c->pos, M, D, 768, D))) return rc;
    for (int l = 0; l < c->L; ++l) {
        const Block& b = c->blocks[l];
        LAUNCH(c, VP_PROF_LAYERNORM, 0.0, 6.0 * M * D,
               vp::layernorm_launch(c->dtype, c->x, b.ln1_g, b.ln1_b, c->y, nullptr, M, D, c->stream));
        LnFuse q0; q0.out_blocked = qkv_blocked;
        if ((rc = gemm(c, VP_PROF_GEMM_QKV, vp::EPI_BIAS, pk[VP_PROF_GEMM_QKV], c->y, b.w_qkv, b.b_qkv, c->qkv, nullptr, M, 3 * D, D, 3 * D, 0, 0, 0, &q0))) return rc;
        if ((rc = attention(c->y, 8.0 * M * D, nullptr))) return rc;
        if ((rc = gemm(c, VP_PROF_GEMM_PROJ, vp::EPI_BIAS_RESID, pk[VP_PROF_GEMM_PROJ], c->y, b.w_proj, b.b_proj, c->x, c->x, M, D, D, D))) return rc;
        LAUNCH(c, VP_PROF_LAYERNORM, 0.0, 6.0 * M * D,
               vp::layernorm_launch(c->dtype, c->x, b.ln2_g, b.ln2_b, c->y, nullptr, M, D, c->stream));
        if ((rc = gemm(c, VP_PROF_GEMM_FC1, vp::EPI_BIAS_GELU, pk[VP_PROF_GEMM_FC1], c->y, b.w_fc1, b.b_fc1, c->hid, nullptr, M, 4 * D, D, 4 * D))) return rc;
        if ((rc = gemm(c, VP_PROF_GEMM_FC2, vp::EPI_BIAS_RESID, pk[VP_PROF_GEMM_FC2], c->hid, fc2_w(c, b), fc2_b(c, b), c->x, c->x, M, D, 4 * D, D))) return rc;
    }
    }
    // last_norm, head and decode: the caller's n_in crops (the planes are laid out for the encoder's row count)
    const int nh = n_in, Mh = nh * 192;
    LAUNCH(c, VP_PROF_LAYERNORM, 0.0, 6.0 * Mh * D,
           vp::layernorm_launch(c->dtype, c->x, c->lnf_g, c->lnf_b, c->y, o.tokens ? c->tok : nullptr, Mh, D, c->stream, plane));
    return o.head ? head_chunk(c, c->y, nh, c->hm, pl.head) : VP_OK;
}

// head of nh crops whose last_norm tokens start at y, with the active head weights (c->w_d1 .. c->w_fin, c->Kp) -> heatmaps [nh, Kp, 64, 48] at hm, as hp plans it
int head_chunk(vp_ctx* c, const uint16_t* y, int nh, float* hm, const HeadPlan& hp) {
    const int D = c->D;
    int rc;
    if (hp.kind == 1) {   // the simple decoder: relu -> bilinear x 4 -> 3x3 conv in one kernel, in the commuted form (simpleheadgeom.h)
        vp::SimpleHeadArgs a{y, c->w_fin, c->b_fin, hm, nh, c->Kp, D, c->fin_rows};
        LAUNCH(c, VP_PROF_GEMM_FINAL, vp::sh_flops(nh, c->Kp, D), vp::sh_bytes(nh, c->Kp, D), vp::simple_head_launch(c->dtype, a, c->stream));
        note_kernel(c, VP_PROF_GEMM_FINAL, c->dtype == vp::DT_F16 ? "simple_head_kernel<F16>" : "simple_head_kernel<BF16>");
        return VP_OK;
    }
    // head: tokens [n,16,12,D] (NHWC view of [n*192, D]) -> [n,32,24,256] -> [n,64,48,256] -> heatmaps [n,Kp,64,48]
    if ((rc = gemm(c, VP_PROF_GEMM_DECONV, vp::EPI_DECONV, hp.deconv1, y, c->w_d1, c->b_d1, c->d1, nullptr, nh * 192, 256, 4 * D, 256, 16, 12, D))) return rc;
    if (hp.fused) {   // the final 1x1 conv rides in deconv2's epilogue: the [n,64,48,256] tensor is never written
        return gemm(c, VP_PROF_GEMM_DECONV, vp::EPI_DECONV_FINAL, hp.deconv2, c->d1, c->w_d2, c->b_d2, hm, nullptr, nh * 768, 256, 1024, 256, 32, 24, 256);
    }
    if ((rc = gemm(c, VP_PROF_GEMM_DECONV, vp::EPI_DECONV, hp.deconv2, c->d1, c->w_d2, c->b_d2, c->d2, nullptr, nh * 768, 256, 1024, 256, 32, 24, 256))) return rc;
    if ((rc = gemm(c, VP_PROF_GEMM_FINAL, vp::EPI_HEATMAP, hp.final, c->d2, c->w_fin, c->b_fin, hm, nullptr, nh * 3072, (int)c->fin_rows, 256, 0))) return rc;
    return VP_OK;
}

// twin: c->hm holds the 2 n interleaved maps forward_mode_chunk leaves under the flip-test mode (never vp_infer_flip's own two passes, whatever the mode)
int decode_chunk(vp_ctx* c, const int32_t* d_wh, float* d_out, int n, bool twin, const float* d_cs) {
    if (d_cs && twin)
        LAUNCH(c, VP_PROF_DECODE, 0.0, 8.0 * n * c->Kp * 3072.0 + 12.0 * n * c->Kp,
               vp::decode_affine_flip_launch(c->hm, flip_table_now(c), c->flip_shift, d_cs, d_out, n, c->Kp, c->stream));
    else if (d_cs)
        LAUNCH(c, VP_PROF_DECODE, 0.0, 4.0 * n * c->Kp * 3072.0 + 12.0 * n * c->Kp, vp::decode_affine_launch(c->hm, d_cs, d_out, n, c->Kp, c->stream));
    else if (twin)
        LAUNCH(c, VP_PROF_DECODE, 0.0, 8.0 * n * c->Kp * 3072.0 + 12.0 * n * c->Kp,
               vp::decode_flip_launch(c->hm, flip_table_now(c), c->flip_shift, d_wh, d_out, n, c->Kp, c->stream));
    else
        LAUNCH(c, VP_PROF_DECODE, 0.0, 4.0 * n * c->Kp * 3072.0 + 12.0 * n * c->Kp,
               vp::decode_launch(c->hm, d_wh, d_out, n, c->Kp, c->stream));
    return VP_OK;
}

// crops of the caller a chunk holds: with the flip-test mode on, every crop brings its mirror image into the batch
int chunk_cap(const vp_ctx* c) { return c->flip_on ? c->maxb / 2 : c->maxb; }
// rows the forward of nb caller crops runs (before the plan's encoder padding): what the small-batch thresholds (hipGraph replay, caller's stream) are about
int chunk_rows(const vp_ctx* c, int nb) { return c->flip_on ? 2 * nb : nb; }

// the forward of a chunk of nb <= chunk_cap crops as the handle's mode asks: heatmaps [nb, Kp, 64, 48] in c->hm, or with the flip-test mode on the
// interleaved [2 nb, Kp, 64, 48] of the crops and their mirror images (decode_chunk averages them on the fly)
int forward_mode_chunk(vp_ctx* c, const void* d_src, int fmt, int nb) {
    FwdOpts o;
    if (c->flip_on) o.twin_src = nb;
    return forward_chunk(c, d_src, fmt, chunk_rows(c, nb), o);
}

using GraphKey = vp_ctx::GraphKey;
using GraphEntry = vp_ctx::GraphEntry;

// vp_infer_boxes_stream: keypoints in padded-crop pixels -> frame pixels, zero rows for invalid boxes (aux = c->box_aux)
static int offsets_chunk(vp_ctx* c, const int32_t* aux, float* d_out, int n) {
    LAUNCH(c, VP_PROF_DECODE, 0.0, 24.0 * n * c->Kp + 16.0 * n, vp::box_offsets_launch(aux, d_out, n, c->Kp, c->stream));
    return VP_OK;
}

// The chunk of a per-crop expert entry (k.wide; c->mix = its plan, the tables are on the device).  Mixed (k.mix != 0): the crops into expert order (crops in the
// caller's order: one gather; frames and boxes were cropped straight into it), the encoder once with every expert's mlp.fc2 in one launch per layer on tiles that never span two
// experts, one head per expert present on its segment's rows.  One expert: the plain forward under that expert.  Then ONE decode launch by records into rows of
// Kmax joints in the caller's order, and the frame offsets on those rows.  The only writer of c->mix_expert / c->mix_bounds.
// Under the per-expert flip-test mode (c->flip_ex; tw = 2): the twin patch gather on the ordered crops puts position j at rows 2 j (the crop) and 2 j + 1 (its mirror),
// so the encoder runs 2 n rows with doubled bounds -- every expert change at an even row -- each head its segment's 2 cnt rows, writing at 2 s0 * Kmax maps, and the
// decode averages a crop's two maps of a joint under its expert's table (mix_recs_flip).  One expert: that expert's plain forward under the mode.
static int mix_chunk_body(vp_ctx* c, const GraphKey& k) {
    const MixPlan& m = *c->mix;
    const int nseg = (int)m.seg_e.size(), D = c->D;
    const int tw = c->flip_ex ? 2 : 1;
    int rc;
    if (nseg == 1) {
        use_expert(c, m.seg_e[0]);
        if ((rc = forward_mode_chunk(c, k.src, k.fmt, k.n))) return rc;
    } else {
        const void* src = k.src;
        if (src != c->in_stage) {
            const size_t B = (size_t)((c->maxb + 3) / 4 * 4);
            HIPCHK(c, vp::gather_crops_launch(src, c->in_stage, c->expert_ids + B, k.n, crop_bytes(k.fmt), c->stream));
            src = c->in_stage;
        }
        FwdOpts encoder_only;
        encoder_only.head = false;
        if (tw == 2) encoder_only.twin_src = k.n;
        c->mix_expert = c->expert_ids;
        c->mix_bounds.clear();
        for (int s = 1; s < nseg; ++s) c->mix_bounds.push_back(tw * m.seg_s[s]);
        rc = forward_chunk(c, src, k.fmt, tw * k.n, encoder_only);
        c->mix_expert = nullptr;
        c->mix_bounds.clear();
        if (rc) return rc;
        for (int s = 0; s < nseg; ++s) {
            const int s0 = tw * m.seg_s[s], cnt = tw * (m.seg_s[s + 1] - m.seg_s[s]);
            use_expert(c, m.seg_e[s]);
            if ((rc = head_chunk(c, c->y + (size_t)s0 * 192 * D, cnt, c->hm + (size_t)s0 * c->Kmax * 3072, plan_head(c->sw, D, cnt, c->fin_rows)))) return rc;
        }
    }
    if (tw == 2)
        LAUNCH(c, VP_PROF_DECODE, 0.0, 8.0 * k.n * c->Kmax * 3072.0 + 12.0 * k.n * c->Kmax,
               vp::decode_flip_mix_launch(c->hm, c->mix_recs_flip, c->flip_tables, c->flip_shift, k.wh, k.out, k.n, c->Kmax, c->stream));
    else
        LAUNCH(c, VP_PROF_DECODE, 0.0, 4.0 * k.n * c->Kmax * 3072.0 + 12.0 * k.n * c->Kmax,
               vp::decode_mix_launch(c->hm, c->mix_recs, k.wh, k.out, k.n, c->Kmax, c->stream));
    if (k.post) LAUNCH(c, VP_PROF_DECODE, 0.0, 24.0 * k.n * c->Kmax + 16.0 * k.n, vp::box_offsets_launch(k.post, k.out, k.n, c->Kmax, c->stream, c->mix_slot, c->mix_recs));
    return VP_OK;
}

// forward + decode (+ frame offsets, key.post != null) of the chunk a key names, on c->stream: what the eager path launches and what a capture records
static int chunk_body(vp_ctx* c, const GraphKey& k) {
    int rc;
    if (k.wide) return mix_chunk_body(c, k);
    if ((rc = forward_mode_chunk(c, k.src, k.fmt, k.n))) return rc;
    if ((rc = decode_chunk(c, k.wh, k.out, k.n, c->flip_on, k.cs))) return rc;
    return k.post ? offsets_chunk(c, k.post, k.out, k.n) : VP_OK;
}

// the cache entry of a key, or nullptr: never seen (or evicted since)
static GraphEntry* graph_lookup(vp_ctx* c, const GraphKey& key) {
    for (auto& g : c->graphs)
        if (g.key == key) return &g;
    return nullptr;
}

// first sighting of a key: it takes the next of the four entries in turn.  VP_OK, or the error of the wait for the evicted graph
static int graph_remember(vp_ctx* c, const GraphKey& key) {
    GraphEntry& ge = c->graphs[c->graph_victim++ & 3];
    if (ge.exec) {   // eviction: the graph may still be executing on the stream (vp_infer_device with sync = 0)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        hipGraphExecDestroy(ge.exec);
    }
    ge = GraphEntry{};
    ge.key = key;
    return VP_OK;
}

// The chunk of `key` captured on the handle's OWN stream (nothing executes during a capture; the caller launches the result on c->stream) and instantiated.
// nullptr: the capture machinery failed, or a launch failed INSIDE the capture (e.g. a capture-illegal call) -- nothing has executed, the message
// of that launch is dropped: an error is reported only if the eager run fails too
static hipGraphExec_t graph_capture(vp_ctx* c, const GraphKey& key) {
    hipStream_t target = c->stream;
    c->stream = c->own_stream;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        const int rc = chunk_body(c, key);
        e = hipStreamEndCapture(c->stream, &graph);
        if (rc) c->err.clear();
        if (rc || (e == hipSuccess && !graph)) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (graph) hipGraphDestroy(graph);
    }
    c->stream = target;
    return e == hipSuccess ? exec : nullptr;
}

// give up on the graph for this key: the chunk runs eagerly now and from now on -- a handle never gets stuck retrying a capture
static int graph_give_up(vp_ctx* c, GraphEntry* ge) {
    (void)hipGetLastError();   // the sticky error of the call that failed
    if (ge->exec) hipGraphExecDestroy(ge->exec);
    ge->exec = nullptr;
    ge->no_graph = true;
    return chunk_body(c, ge->key);
}

// forward + decode of one chunk.  Small chunks (<= graph_max_n rows, profiling off) are launch-bound -- ~110-290 launches of a few
// microseconds each -- so the second time the same key (GraphKey, api_internal.h) is seen the chunk is captured into a hipGraph
// and from then on replayed with one hipGraphLaunch.
int run_chunk(vp_ctx* c, const void* d_src, int fmt, int nb, const int32_t* d_wh, float* d_out, const int32_t* post, const float* d_cs) {
    if (nb > chunk_cap(c)) return fail(c, VP_ERR_INVALID, "a chunk of " + std::to_string(nb) + " crops exceeds what the handle's workspaces hold in this mode");
    GraphKey key{nb, fmt, d_src, d_wh, d_out, c->expert, post, c->flip_gen, d_cs};
    if (c->mix && d_cs) return fail(c, VP_ERR_STATE, "the affine crop route does not run a chunk with per-crop experts");
    if (c->mix) {   // a per-crop expert entry: its chunk's pattern, or the one expert the whole chunk runs
        if ((c->flip_on && !c->flip_ex) || c->mix->nb != nb) return fail(c, VP_ERR_STATE, "a chunk with per-crop experts under the single-table flip-test mode, or a plan of another chunk");
        key.wide = true;
        key.mix = c->mix->pattern;
        key.expert = key.mix ? 0 : c->mix->seg_e[0];
        if (key.mix == MIX_NO_GRAPH) return chunk_body(c, key);   // a pattern the key cannot hold exactly
    }
    // a caller's legacy default stream (torch's usual current stream): VP_GRAPH_NULL=1 replays the graph there too (a caller that synchronises after
    // every call pays the 110-290 eager launches' host time); 0 = plain launches (equal when calls are enqueued back to back)
    if (chunk_rows(c, nb) > c->sw.graph_max_n || c->prof != 0 || (c->stream == nullptr && !c->sw.graph_null)) return chunk_body(c, key);
    GraphEntry* ge = graph_lookup(c, key);
    if (!ge) {   // first sighting: run eagerly (also performs every one-time function-attribute set-up outside a capture), remember the key
        const int rc = graph_remember(c, key);
        return rc ? rc : chunk_body(c, key);
    }
    if (ge->no_graph) return chunk_body(c, key);
    if (!ge->exec) {   // second sighting: capture, and launch on the stream of this call
        if (!(ge->exec = graph_capture(c, key))) return graph_give_up(c, ge);
        HIPCHK(c, hipGraphLaunch(ge->exec, c->stream));
        return VP_OK;
    }
    if (hipGraphLaunch(ge->exec, c->stream) == hipSuccess) return VP_OK;
    return graph_give_up(c, ge);   // a stream that does not take graph launches: nothing was enqueued
}

}  // namespace vpi
