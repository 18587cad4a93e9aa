// C ABI (include/vitpose_hip.h) of the MI355X-native ViTPose hot path:
// context + weight packer + forward orchestration.  No CPU fallback anywhere:
// every compute entry point needs a HIP device and fails with VP_ERR_HIP otherwise.
#include "api_internal.h"
#include "boxgeom.h"

using namespace vpi;

namespace vpi {

thread_local std::string g_create_error;

int fail(vp_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

bool prof_begin(vp_ctx* c, int fam, double flops, double bytes) {
    if (!((c->prof >> fam) & 1u)) return false;
    std::pair<hipEvent_t, hipEvent_t> p;
    if (!c->ev_pool.empty()) {
        p = c->ev_pool.back();
        c->ev_pool.pop_back();
    } else {
        hipEventCreate(&p.first);
        hipEventCreate(&p.second);
    }
    hipEventRecord(p.first, c->stream);
    c->evs.push_back({p.first, p.second, fam, flops, bytes});
    return true;
}
void prof_end(vp_ctx* c, bool on) {
    if (on) hipEventRecord(c->evs.back().b, c->stream);
}
void prof_collect(vp_ctx* c) {
    for (auto& e : c->evs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            c->acc.ms[e.fam] += ms;
            c->acc.flops[e.fam] += e.flops;
            c->acc.bytes[e.fam] += e.bytes;
            c->acc.launches[e.fam] += 1;
        }
        c->ev_pool.push_back({e.a, e.b});
    }
    c->evs.clear();
}

// Tile configuration per GEMM family.  Defaults = best measured on MI355X (profiles/);
// experiments override with VP_GEMM_TUNE="fam:variant:group_m,..." (fam = VP_PROF_* index).
void apply_gemm_tuning(Switches& s) {
#ifndef VP_TOOLS
    (void)s;
#else
    if (const char* t = getenv("VP_GEMM_TUNE")) {
        int f, v, gm, used = 0;
        while (sscanf(t, "%d:%d:%d%n", &f, &v, &gm, &used) == 3) {
            if (f >= 0 && f < VP_PROF_COUNT) { s.gemm_variant[f] = v; s.gemm_group_m[f] = gm; }
            t += used;
            if (*t == ',') ++t; else break;
        }
    }
#endif
}

// Every switch of a handle, read once (vp_create): switches between SHIPPED, tested code paths (each has a parity test that flips it) and the thresholds
// of the measured rules; the measurement build adds its development switches (tools/)
void read_switches(Switches& s) {
    auto on = [](const char* name, bool& dst) { if (const char* f = getenv(name)) dst = atoi(f) != 0; };
    auto num = [](const char* name, auto& dst) { if (const char* f = getenv(name)) dst = atol(f); };
    on("VP_FUSE_LN", s.fuse_ln);
    on("VP_PERSIST", s.persist_gemm);
    if (const char* f = getenv("VP_GRAPH")) s.graph_max_n = atoi(f) == 1 ? 16 : atoi(f);   // 0 = off, 1 = default, n > 1: capture chunks of up to n crops
    on("VP_GRAPH_NULL", s.graph_null);
    if (const char* f = getenv("VP_CALLER_STREAM")) s.caller_stream_max_n = atoi(f) == 1 ? 16 : atoi(f);   // 0 = always fence against the caller's stream with events
    on("VP_FUSE_HEAD", s.fuse_head);
    if (const char* f = getenv("VP_FOLD_STATS")) { s.graph_max_n_stats = atoi(f); s.fold_rule = false; }   // an explicit threshold: fold up to that many crops, nowhere else
    on("VP_BLOCKED_QKV", s.blocked_qkv);
    on("VP_FUSE_QKV_ATTN", s.fuse_qkv_attn);
    s.qa_min_set = getenv("VP_QA_MIN_TILES") != nullptr;
    num("VP_QA_MIN_TILES", s.qa_min_tiles);
    num("VP_QA80_MIN_TILES", s.qa80_min_tiles);
    num("VP_QA80_GROUP", s.qa80_group);
    num("VP_ATTN_QSPLIT", s.attn_qsplit);
    on("VP_DECONV_PARITY_FAST", s.deconv_parity_fast);
    on("VP_G8_COST", s.g8_cost_model);
    on("VP_PAD_BATCH", s.pad_batch);
    num("VP_G8_BM192", s.g8_bm192);   // mask: 1 = residual GEMMs, 2 = wide GEMMs may take the 192 x 256 tile of the 8-phase kernel (0: never)
    if (const char* f = getenv("VP_SPLITK")) {   // 0 = off; "fc2:S:variant,proj:S:variant" = override the rule (measurement sweeps)
        if (!strchr(f, ':')) s.splitk_on = atoi(f) != 0;
        else {
            const char* t = f;
            while (*t) {
                const int which = !strncmp(t, "fc2:", 4) ? 1 : !strncmp(t, "proj:", 5) ? 0 : -1;
                if (which < 0) break;
                t = strchr(t, ':') + 1;
                int S = 0, v = 0, used = 0;
                if (sscanf(t, "%d:%d%n", &S, &v, &used) != 2) break;
                s.splitk_force[which][0] = S; s.splitk_force[which][1] = v;
                t += used;
                if (*t == ',') ++t;
            }
        }
    }
    num("VP_GEMM8", s.gemm8_mask);   // which GEMMs may take the 8-phase kernel (1 fc2, 2 fc1, 4 qkv, 8 proj; 0 = the 2-phase kernels everywhere)
    s.fp8_proj16 = getenv("VP_FP8_PROJ16") != nullptr;
#ifdef VP_TOOLS   // development switches of the measurement build (tools/)
    num("VP_G8_MIN_TILES", s.g8_min_tiles);
    on("VP_BLOCKED_HID", s.blocked_hid);
    num("VP_ORDER", s.order_mask);
    num("VP_G8_STAGGER", s.g8_stagger);
    if (const char* t = getenv("VP_ABLATE_FAM")) {   // e.g. "2:64,1:64" = non-temporal stores in the qkv and fc1 epilogues
        int f, b, used = 0;
        while (sscanf(t, "%d:%d%n", &f, &b, &used) == 2) {
            if (f >= 0 && f < VP_PROF_COUNT) s.fam_ablate[f] = b;
            t += used;
            if (*t == ',') ++t; else break;
        }
    }
#endif
    apply_gemm_tuning(s);
}

int gemm(vp_ctx* c, int fam, int epi, const GemmPick& pk, const uint16_t* A, const uint16_t* W, const float* bias, void* out,
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
        if (ln->tiles_out) *ln->tiles_out = N / 64;   // partial statistics are written per 64 columns, whatever the tile
    }
    if (epi == vp::EPI_DECONV_FINAL) { g.W2 = c->w_fin; g.bias2 = c->b_fin; g.out2 = c->hm; }   // deconv2 + final 1x1 conv in one kernel
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
            if (c->kernel_desc[fam] != d2) c->kernel_desc[fam] = d2;
        }
        LAUNCH(c, fam, 0.0, 0.0, vp::splitk_reduce_launch(c->dtype, c->splitk_ws, pk.splitk, bias, (uint16_t*)out, g.plane, g.stats_out, M, N, c->stream));
        return VP_OK;
    }
    LAUNCH(c, fam, flops, bytes, vp::gemm_launch(c->dtype, epi, g, c->stream));
    if (desc[0] && c->kernel_desc[fam] != desc) c->kernel_desc[fam] = desc;
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
    const int bn = pk.variant == 17 ? 192 : 256;   // tile_rules.hip resolve_gemm_fp8
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
    if (desc[0] && c->kernel_desc[fam] != desc) c->kernel_desc[fam] = desc;
    return VP_OK;
}

}  // namespace vpi

namespace {

int head_chunk(vp_ctx* c, const uint16_t* y, int nh, float* hm, const HeadPlan& hp);

// fc2 weights / bias of block b for the active expert (a ViTPose+ handle outside a mixed batch; expert 0 = the only one of a plain handle)
const uint16_t* fc2_w(const vp_ctx* c, const vpi::Block& b) { return c->mix_expert ? b.w_fc2 : b.w_fc2 + (size_t)c->expert * c->fc2_w_stride; }
const float* fc2_b(const vp_ctx* c, const vpi::Block& b) { return c->mix_expert ? b.b_fc2 : b.b_fc2 + (size_t)c->expert * c->fc2_b_stride; }

// forward of one chunk (n <= max_batch) with device-resident crops; heatmaps land in c->hm (head = false: the encoder and last_norm only, tokens in c->y).
// Executes the chunk's plan (tile_rules.hip plan_chunk): which kernel runs each GEMM, the encoder batch, the LayerNorm folds, the qkv path.
// twin_src > 0 (flip-test mode): n_in = 2 * twin_src rows, the twin_src crops at d_crops interleaved with their mirror images (crop, mirror, crop, mirror, ...);
// everything behind the patch gather is the plain forward of an n_in-crop batch.
int forward_chunk(vp_ctx* c, const void* d_crops, int fmt, int n_in, bool want_tokens, bool flip = false, bool head = true, int twin_src = 0) {
    const int D = c->D;
    const ChunkPlan pl = plan_chunk(c->sw, D, c->heads, c->maxb, c->fp8, n_in, c->fin_rows, c->mix_expert ? &c->mix_bounds : nullptr);
    const GemmPick* pk = pl.gemm;
    const int n = pl.n;   // rows n_in .. n - 1 of a padded encoder batch repeat the last crop and are never read by the head
    const int M = n * 192;
    const double in_b = (fmt == VP_INPUT_F32_NCHW ? 4.0 : 1.0) * n_in * 3.0 * 256 * 192;
    if (twin_src) LAUNCH(c, VP_PROF_IM2COL, 0.0, 0.5 * in_b + 2.0 * M * 768, vp::im2col_twin_launch(c->dtype, d_crops, fmt, c->hid, n, twin_src, c->stream));
    else LAUNCH(c, VP_PROF_IM2COL, 0.0, in_b + 2.0 * M * 768, vp::im2col_launch(c->dtype, d_crops, fmt, c->hid, n, c->stream, flip, n_in));
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
        const int Mp = (int)std::max<size_t>((size_t)(M + 255) / 256 * 256, 512);
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
                g80.attn_scale_log2e = (1.0f / sqrtf(80.0f)) * 1.4426950408889634f;
                g80.ablate = c->gemm_ablate | c->sw.fam_ablate[VP_PROF_GEMM_QKV];
                char desc[192];
                desc[0] = 0;
                g80.desc = desc; g80.desc_cap = (int)sizeof(desc);
                LAUNCH(c, VP_PROF_GEMM_QKV, qkv_attn_flops, qkv_attn_bytes, vp::gemm_launch(c->dtype, vp::EPI_QKV_ATTN, g80, c->stream));
                if (desc[0] && c->kernel_desc[VP_PROF_GEMM_QKV] != desc) c->kernel_desc[VP_PROF_GEMM_QKV] = desc;
            } else if (pl.qkv_path == QKV_ATTN64) {   // one pair of crops x one head per tile (qkvattn.hip; an odd batch's last crop fills both halves of its pair)
                vp::QkvAttnArgs qa{};
                qa.x_hi = xh; qa.wh = b.w_qkvh; qa.bh = b.b_qkvh; qa.sh = b.s_qkvh; qa.rowstat = c->rowstat; qa.y = c->y;
                qa.npairs = (n + 1) / 2; qa.ncrops = n; qa.heads = c->heads; qa.D = D;
                qa.scale_log2e = (1.0f / sqrtf(64.0f)) * 1.4426950408889634f;
                char desc[96];
                desc[0] = 0;
                LAUNCH(c, VP_PROF_GEMM_QKV, qkv_attn_flops, qkv_attn_bytes, vp::qkvattn_launch(c->dtype, qa, c->stream, desc, (int)sizeof(desc)));
                if (desc[0] && c->kernel_desc[VP_PROF_GEMM_QKV] != desc) c->kernel_desc[VP_PROF_GEMM_QKV] = desc;
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
           vp::layernorm_launch(c->dtype, c->x, c->lnf_g, c->lnf_b, c->y, want_tokens ? c->tok : nullptr, Mh, D, c->stream, plane));
    return head ? head_chunk(c, c->y, nh, c->hm, pl.head) : VP_OK;
}

// head of nh crops whose last_norm tokens start at y, with the active head weights (c->w_d1 .. c->w_fin, c->Kp) -> heatmaps [nh, Kp, 64, 48] at hm, as hp plans it
int head_chunk(vp_ctx* c, const uint16_t* y, int nh, float* hm, const HeadPlan& hp) {
    const int D = c->D;
    int rc;
    // head: tokens [n,16,12,D] (NHWC view of [n*192, D]) -> [n,32,24,256] -> [n,64,48,256] -> heatmaps [n,Kp,64,48]
    if ((rc = gemm(c, VP_PROF_GEMM_DECONV, vp::EPI_DECONV, hp.deconv1, y, c->w_d1, c->b_d1, c->d1, nullptr, nh * 192, 256, 4 * D, 256, 16, 12, D))) return rc;
    if (hp.fused) {   // the final 1x1 conv rides in deconv2's epilogue: the [n,64,48,256] tensor is never written
        float* keep = c->hm;   // gemm() hands EPI_DECONV_FINAL c->hm as its heatmap output
        c->hm = hm;
        rc = gemm(c, VP_PROF_GEMM_DECONV, vp::EPI_DECONV_FINAL, hp.deconv2, c->d1, c->w_d2, c->b_d2, nullptr, nullptr, nh * 768, 256, 1024, 256, 32, 24, 256);
        c->hm = keep;
        return rc;
    }
    if ((rc = gemm(c, VP_PROF_GEMM_DECONV, vp::EPI_DECONV, hp.deconv2, c->d1, c->w_d2, c->b_d2, c->d2, nullptr, nh * 768, 256, 1024, 256, 32, 24, 256))) return rc;
    if ((rc = gemm(c, VP_PROF_GEMM_FINAL, vp::EPI_HEATMAP, hp.final, c->d2, c->w_fin, c->b_fin, hm, nullptr, nh * 3072, (int)c->fin_rows, 256, 0))) return rc;
    return VP_OK;
}

// twin: c->hm holds the 2 n interleaved maps forward_mode_chunk leaves under the flip-test mode (never vp_infer_flip's own two passes, whatever the mode)
int decode_chunk(vp_ctx* c, const int32_t* d_wh, float* d_out, int n, bool twin) {
    if (twin)
        LAUNCH(c, VP_PROF_DECODE, 0.0, 8.0 * n * c->Kp * 3072.0 + 12.0 * n * c->Kp,
               vp::decode_flip_launch(c->hm, c->flip_table, c->flip_shift, d_wh, d_out, n, c->Kp, c->stream));
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
    return c->flip_on ? forward_chunk(c, d_src, fmt, 2 * nb, false, false, true, nb) : forward_chunk(c, d_src, fmt, nb, false);
}

// vp_infer_boxes_stream: keypoints in padded-crop pixels -> frame pixels, zero rows for invalid boxes (aux = c->box_aux)
int offsets_chunk(vp_ctx* c, const int32_t* aux, float* d_out, int n) {
    LAUNCH(c, VP_PROF_DECODE, 0.0, 24.0 * n * c->Kp + 16.0 * n, vp::box_offsets_launch(aux, d_out, n, c->Kp, c->stream));
    return VP_OK;
}

// forward + decode of one chunk.  Small chunks (<= graph_max_n crops, profiling off) are launch-bound -- ~110-290 launches of a few
// microseconds each -- so the second time the same (n, format, buffers) combination is seen the chunk is captured into a hipGraph
// and from then on replayed with one hipGraphLaunch.  post != null: the frame-offset kernel of vp_infer_boxes_stream follows the decode
// (inside the graph; `post` is part of the key).
int run_chunk(vp_ctx* c, const void* d_src, int fmt, int nb, const int32_t* d_wh, float* d_out, const int32_t* post = nullptr) {
    int rc;
    if (nb > chunk_cap(c)) return fail(c, VP_ERR_INVALID, "a chunk of " + std::to_string(nb) + " crops exceeds what the handle's workspaces hold in this mode");
    auto eager = [&]() -> int {
        if ((rc = forward_mode_chunk(c, d_src, fmt, nb))) return rc;
        if ((rc = decode_chunk(c, d_wh, d_out, nb, c->flip_on))) return rc;
        return post ? offsets_chunk(c, post, d_out, nb) : VP_OK;
    };
    // a caller's legacy default stream (torch's usual current stream): VP_GRAPH_NULL=1 replays the graph there too (a caller that synchronises after
    // every call pays the 110-290 eager launches' host time); 0 = plain launches (equal when calls are enqueued back to back)
    if (chunk_rows(c, nb) > c->sw.graph_max_n || c->prof != 0 || (c->stream == nullptr && !c->sw.graph_null)) return eager();
    vp_ctx::GraphEntry* ge = nullptr;
    for (auto& g : c->graphs)
        if (g.n == nb && g.fmt == fmt && g.src == d_src && g.wh == d_wh && g.out == d_out && g.expert == c->expert && g.post == post && g.flip == c->flip_gen) { ge = &g; break; }
    if (ge && ge->exec) {
        const hipError_t el = hipGraphLaunch(ge->exec, c->stream);
        if (el == hipSuccess) return VP_OK;
        (void)hipGetLastError();   // a stream that does not take graph launches: nothing was enqueued -- this key runs eagerly from now on
        hipGraphExecDestroy(ge->exec);
        ge->exec = nullptr;
        ge->no_graph = true;
        return eager();
    }
    if (ge && ge->no_graph) return eager();   // capture or instantiation failed once for this key: it stays on the eager path
    if (!ge) {   // first sighting: run eagerly (also performs every one-time function-attribute set-up outside a capture), remember the key
        ge = &c->graphs[c->graph_victim++ & 3];
        if (ge->exec) {   // eviction: the graph may still be executing on the stream (vp_infer_device with sync = 0)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            hipGraphExecDestroy(ge->exec);
            ge->exec = nullptr;
        }
        ge->n = nb; ge->fmt = fmt; ge->src = d_src; ge->wh = d_wh; ge->out = d_out; ge->expert = c->expert; ge->post = post; ge->flip = c->flip_gen; ge->seen = 1; ge->no_graph = false;
        return eager();
    }
    // second sighting: capture.  Any failure of the capture machinery (not of the launches themselves) marks the key "do not
    // graph" and the chunk runs eagerly now and from now on -- a handle never gets stuck retrying a capture.
    hipGraph_t graph = nullptr;
    hipStream_t target = c->stream;   // the capture itself always runs on the handle's own stream (nothing executes during a capture); the graph is launched on `target`
    c->stream = c->own_stream;
    hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { c->stream = target; (void)hipGetLastError(); ge->no_graph = true; return eager(); }
    rc = forward_mode_chunk(c, d_src, fmt, nb);
    if (!rc) rc = decode_chunk(c, d_wh, d_out, nb, c->flip_on);
    if (!rc && post) rc = offsets_chunk(c, post, d_out, nb);
    e = hipStreamEndCapture(c->stream, &graph);
    c->stream = target;
    if (rc) {   // a launch failed INSIDE the capture (e.g. a capture-illegal call): nothing has executed -- drop the graph, clear the sticky
                // error and run the chunk eagerly, now and from now on; an error is reported only if the eager run fails too
        if (graph) hipGraphDestroy(graph);
        (void)hipGetLastError();
        ge->exec = nullptr;
        ge->no_graph = true;
        c->err.clear();
        return eager();
    }
    if (e == hipSuccess && graph) {
        e = hipGraphInstantiate(&ge->exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
    } else if (e == hipSuccess) {
        e = hipErrorUnknown;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ge->exec = nullptr;
        ge->no_graph = true;
        return eager();
    }
    HIPCHK(c, hipGraphLaunch(ge->exec, c->stream));
    return VP_OK;
}

size_t crop_bytes(int fmt) { return (size_t)3 * 256 * 192 * (fmt == VP_INPUT_F32_NCHW ? 4 : 1); }

// Work on the handle's buffers is about to be enqueued on stream s: order it behind whatever the previous call left on ANOTHER stream.
//   own -> own, caller A -> caller A: nothing (in-order streams);  own -> caller: record on own, caller waits;  caller -> own / another caller: wait for ev_sw,
//   which vp_infer_device_stream recorded on the caller's stream behind its launches (that stream itself is never touched again: it may be gone).
int adopt_stream(vp_ctx* c, hipStream_t s) {
    if (!c->foreign_pending && s == c->own_stream) return VP_OK;
    if (c->foreign_pending && (const void*)s == c->last_stream_id && s != c->own_stream) return VP_OK;
    if (!c->ev_sw) HIPCHK(c, hipEventCreateWithFlags(&c->ev_sw, hipEventDisableTiming));
    if (!c->foreign_pending) HIPCHK(c, hipEventRecord(c->ev_sw, c->own_stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_sw, 0));
    if (s == c->own_stream) c->foreign_pending = false;
    return VP_OK;
}

int check_ready(vp_ctx* c, int fmt, int n, const void* p0, const void* p1, bool adopt_own = true) {
    if (!c) return VP_ERR_INVALID;
    if (!c->loaded) return fail(c, VP_ERR_STATE, "weights not loaded: call vp_load_weights first");
    if (fmt != VP_INPUT_F32_NCHW && fmt != VP_INPUT_U8_NHWC) return fail(c, VP_ERR_INVALID, "unknown input_format");
    if (n < 0 || (n > 0 && (!p0 || !p1))) return fail(c, VP_ERR_INVALID, "null buffer or negative batch");
    hipError_t e = hipSetDevice(c->cfg.device_id);
    if (e != hipSuccess) return fail(c, VP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return adopt_own ? adopt_stream(c, c->own_stream) : VP_OK;   // every entry but the caller-stream path works on the handle's own stream
}

// The ordering of the caller-stream entries (vp_infer_device_stream, vp_infer_boxes_stream): `chunks` enqueues the call's work on c->stream.
// Batches of 1 .. caller_stream_max_n crops (<= max_batch) run ON the caller's stream -- in order with its producers and consumers by construction,
// no cross-stream dependency per call (two of them cost ~0.1 ms of a 0.6-2.4 ms step: profiles/small_batch_r5.txt); ev_sw, recorded behind the
// launches, is what the next call on any other stream (and vp_synchronize / vp_destroy) waits for.  Larger batches run on the handle's own
// stream, fenced against the caller's with ev_in / ev_out.
template <class Chunks> int caller_ordered(vp_ctx* c, hipStream_t cs, int n, Chunks chunks) {
    int rc;
    if (n > 0 && chunk_rows(c, n) <= c->sw.caller_stream_max_n && n <= chunk_cap(c) && cs != c->own_stream) {
        if ((rc = adopt_stream(c, cs))) return rc;
        c->stream = cs;
        rc = chunks();
        c->stream = c->own_stream;
        if (!c->ev_sw && hipEventCreateWithFlags(&c->ev_sw, hipEventDisableTiming) != hipSuccess) return fail(c, VP_ERR_HIP, "hipEventCreateWithFlags(ev_sw)");
        const hipError_t er = hipEventRecord(c->ev_sw, cs);   // also when rc != 0: part of the chunk may be enqueued
        c->foreign_pending = true;
        c->last_stream_id = (const void*)cs;
        if (rc) return rc;
        if (er != hipSuccess) return fail(c, VP_ERR_HIP, std::string("hipEventRecord(ev_sw): ") + hipGetErrorString(er));
        return VP_OK;
    }
    if ((rc = adopt_stream(c, c->own_stream))) return rc;
    if (!c->ev_in) HIPCHK(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
    if (!c->ev_out) HIPCHK(c, hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
    // everything the caller enqueued on its stream so far (the producers of the inputs) happens before the library's kernels ...
    HIPCHK(c, hipEventRecord(c->ev_in, cs));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_in, 0));
    if ((rc = chunks())) return rc;
    // ... and whatever the caller enqueues afterwards (consumers of the outputs) happens after them
    HIPCHK(c, hipEventRecord(c->ev_out, c->stream));
    HIPCHK(c, hipStreamWaitEvent(cs, c->ev_out, 0));
    return VP_OK;
}

}  // namespace

namespace vpi {   // shared with debug_taps.hip (vp_dbg_crop_prep)

int frame_plan(const vp_frame* frames, int n_frames, const int32_t* p9, int n, int32_t* bands, std::string* why) {
    auto bad = [&](const std::string& m) { if (why) *why = m; return VP_ERR_INVALID; };
    if (n < 0) return bad("negative crop count");
    if (n > 0 && n_frames <= 0) return bad("crops given but no frames");
    if (n > 0 && (!frames || !p9)) return bad("null frame or crop table");
    const int nf = n_frames > 0 ? n_frames : 0;
    std::vector<int64_t> lo(nf, INT64_MAX), hi(nf, -1);
    for (int i = 0; i < n; ++i) {
        const int32_t* p = p9 + 9 * (size_t)i;
        const int f = p[0];
        const std::string at = "crop " + std::to_string(i) + ": ";
        if (f < 0 || f >= n_frames) return bad(at + "frame index " + std::to_string(f) + " outside [0, " + std::to_string(n_frames) + ")");
        const vp_frame& fr = frames[f];
        if (!fr.data) return bad(at + "frame " + std::to_string(f) + " has no data");
        if (fr.h <= 0 || fr.w <= 0) return bad(at + "frame " + std::to_string(f) + " has a non-positive size");
        const int64_t x0 = p[1], y0 = p[2], cw = p[3], ch = p[4], left = p[5], top = p[6], pw = p[7], ph = p[8];
        if (cw <= 0 || ch <= 0 || pw <= 0 || ph <= 0) return bad(at + "non-positive crop or canvas size");
        if (x0 < 0 || y0 < 0 || x0 + cw > fr.w || y0 + ch > fr.h || left < 0 || top < 0 || left + cw > pw || top + ch > ph)
            return bad(at + "lies outside frame " + std::to_string(f) + " / its padded canvas");
        lo[f] = std::min(lo[f], y0);
        hi[f] = std::max(hi[f], y0 + ch);
    }
    if (bands)
        for (int f = 0; f < nf; ++f) {
            bands[2 * f] = hi[f] < 0 ? 0 : (int32_t)lo[f];
            bands[2 * f + 1] = hi[f] < 0 ? 0 : (int32_t)hi[f];
        }
    return VP_OK;
}

int stage_frames(vp_ctx* c, const vp_frame* frames, int n_frames, bool on_device, const int32_t* p9, int n, const int32_t* bands,
                 std::vector<vp::CropRec>& recs) {
    std::vector<const uint8_t*> row0_ptr(n_frames, nullptr);   // row bands[2 f] of frame f, where the kernel reads it
    if (on_device) {
        for (int f = 0; f < n_frames; ++f) {
            if (bands[2 * f] == bands[2 * f + 1]) continue;
            const vp_frame& fr = frames[f];
            const size_t fbytes = (size_t)fr.h * fr.w * 3;
            hipPointerAttribute_t a;
            std::memset(&a, 0, sizeof(a));
            void* base = nullptr;
            size_t size = 0;
            bool ok = hipPointerGetAttributes(&a, fr.data) == hipSuccess && a.type == hipMemoryTypeDevice && a.device == c->cfg.device_id;
            ok = ok && hipMemGetAddressRange(&base, &size, (void*)fr.data) == hipSuccess && fr.data + fbytes <= (const uint8_t*)base + size;
            if (!ok) {
                (void)hipGetLastError();
                return fail(c, VP_ERR_INVALID, "frame " + std::to_string(f) + " is not device memory of device " + std::to_string(c->cfg.device_id) +
                                                   " (or runs past the end of its allocation)");
            }
            row0_ptr[f] = fr.data + (size_t)bands[2 * f] * fr.w * 3;
        }
    } else {
        std::vector<size_t> off(n_frames, 0);
        size_t total = 0;
        for (int f = 0; f < n_frames; ++f) {
            if (bands[2 * f] == bands[2 * f + 1]) continue;
            off[f] = total;
            total += ((size_t)(bands[2 * f + 1] - bands[2 * f]) * frames[f].w * 3 + 255) & ~(size_t)255;
        }
        if (total > c->frame_cap) {   // grow the arena and release the smaller one (never shrunk): growing resolutions must not grow device memory
            void* q = nullptr;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (hipMalloc(&q, total + 256) != hipSuccess) {   // the old arena stays: the handle remains usable
                (void)hipGetLastError();
                return fail(c, VP_ERR_HIP, "cannot allocate a " + std::to_string(total) + "-byte frame staging arena");
            }
            if (c->frame_stage) {
                for (auto it = c->allocs.begin(); it != c->allocs.end(); ++it)
                    if (*it == (void*)c->frame_stage) { c->allocs.erase(it); break; }
                hipFree(c->frame_stage);
            }
            c->allocs.push_back(q);
            c->frame_stage = (uint8_t*)q;
            c->frame_cap = total;
        }
        for (int f = 0; f < n_frames; ++f) {   // ONE copy per frame with crops: its row band, full width
            if (bands[2 * f] == bands[2 * f + 1]) continue;
            const size_t pitch = (size_t)frames[f].w * 3;
            HIPCHK(c, hipMemcpyAsync(c->frame_stage + off[f], frames[f].data + (size_t)bands[2 * f] * pitch,
                                     (size_t)(bands[2 * f + 1] - bands[2 * f]) * pitch, hipMemcpyHostToDevice, c->stream));
            row0_ptr[f] = c->frame_stage + off[f];
        }
    }
    recs.resize(n);
    for (int i = 0; i < n; ++i) {
        const int32_t* p = p9 + 9 * (size_t)i;
        const int f = p[0];
        const int64_t pitch = (int64_t)frames[f].w * 3;
        vp::CropRec& r = recs[i];
        r.src = row0_ptr[f] + (size_t)(p[2] - bands[2 * f]) * pitch + (size_t)p[1] * 3;
        r.pitch = pitch;
        r.cw = p[3]; r.ch = p[4]; r.left = p[5]; r.top = p[6]; r.pw = p[7]; r.ph = p[8];
    }
    return VP_OK;
}

int box_args(int n_frames, const int32_t* frame_hw, int hw_stride, int row_stride, int n, int pad, std::string* why) {
    auto bad = [&](const std::string& m) { if (why) *why = m; return VP_ERR_INVALID; };
    if (n < 0) return bad("negative box count");
    if (row_stride < 4) return bad("row_stride " + std::to_string(row_stride) + " < 4 (x1, y1, x2, y2 per row)");
    if (pad < 0) return bad("negative pad");
    if (n > 0 && n_frames <= 0) return bad("boxes given but no frames");
    for (int f = 0; f < n_frames && n > 0; ++f) {   // every frame of the table: the frame indices live on the device
        const int32_t h = frame_hw[(size_t)f * hw_stride], w = frame_hw[(size_t)f * hw_stride + 1];
        if (h <= 0 || w <= 0 || h > vp::BOX_MAX_SIDE || w > vp::BOX_MAX_SIDE)
            return bad("frame " + std::to_string(f) + " has a size outside [1, 2^24]");
    }
    return VP_OK;
}

int flip_partner_table(int K, const int32_t* pairs, int n_pairs, int32_t* partner, std::string* why) {
    auto bad = [&](const std::string& m) { if (why) *why = m; return VP_ERR_INVALID; };
    if (K <= 0 || !partner) return bad("no joints");
    if (n_pairs < 0) return bad("negative n_pairs");
    if (n_pairs > 0 && !pairs) return bad("null flip_pairs with n_pairs > 0");
    for (int k = 0; k < K; ++k) partner[k] = k;
    for (int i = 0; i < n_pairs; ++i) {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || b < 0 || a >= K || b >= K)
            return bad("flip pair " + std::to_string(i) + " = (" + std::to_string(a) + ", " + std::to_string(b) + ") outside the head's " + std::to_string(K) + " joints");
        partner[a] = b;
        partner[b] = a;
    }
    return VP_OK;
}

}  // namespace vpi

extern "C" {

int vp_abi_version(void) { return VP_ABI_VERSION; }
int vp_group_destroy(vp_group_handle g);

int vp_create(vp_handle* out, const vp_config* cfg) {
    if (!out || !cfg) return fail(nullptr, VP_ERR_INVALID, "null argument");
    *out = nullptr;
    const int D = cfg->embed_dim, h = cfg->num_heads;
    if (D <= 0 || h <= 0 || D % h != 0 || D % 128 != 0 || D > 1280)
        return fail(nullptr, VP_ERR_INVALID, "embed_dim must be a multiple of 128 (<= 1280) and divisible by num_heads");
    const int hd = D / h;
    if (hd != 32 && hd != 64 && hd != 80) return fail(nullptr, VP_ERR_INVALID, "head_dim must be 32, 64 or 80");
    if (cfg->depth <= 0 || cfg->num_keypoints <= 0 || cfg->num_keypoints > 1024 || cfg->max_batch <= 0)
        return fail(nullptr, VP_ERR_INVALID, "depth, num_keypoints and max_batch must be positive");
    if (cfg->dtype != VP_DTYPE_F16 && cfg->dtype != VP_DTYPE_BF16 && cfg->dtype != VP_DTYPE_FP8) return fail(nullptr, VP_ERR_INVALID, "unknown dtype");
    // fp8 mode: the MXFP8 kernel has no small-tile fallback -- at the minimum padded row count (512) the narrowest GEMM (attn.proj / mlp.fc2,
    // N = D) must still have the 8 tiles gemm8f_supported asks for: 2 x D / 192 (or / 256) >= 8 -> D >= 768.  Rejected HERE, not at infer time.
    if (cfg->dtype == VP_DTYPE_FP8 && (D % 256 != 0 || D < 768))
        return fail(nullptr, VP_ERR_INVALID, "the fp8 mode needs embed_dim >= 768 and a multiple of 256 (K-tiles of 128, an even number of them; >= 8 tiles per GEMM at the smallest batch): ViTPose-B / -L / -H");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, VP_ERR_HIP, std::string("no HIP device available (this library has no CPU fallback): ") +
                                             (e != hipSuccess ? hipGetErrorString(e) : "device count 0"));
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, VP_ERR_INVALID, "device_id out of range");
    vp_ctx* c = new vp_ctx();
    c->cfg = *cfg;
    c->D = D; c->L = cfg->depth; c->heads = h; c->Kp = cfg->num_keypoints; c->Kmax = c->Kp;
    c->dtype = cfg->dtype == VP_DTYPE_BF16 ? vp::DT_BF16 : vp::DT_F16;   // fp8 mode: everything that is not one of the three MXFP8 GEMMs runs as fp16
    c->fp8 = cfg->dtype == VP_DTYPE_FP8;
    c->maxb = cfg->max_batch;
    read_switches(c->sw);
    auto bail = [&](int rc) { g_create_error = c->err; vp_destroy(c); return rc; };
    if ((e = hipSetDevice(cfg->device_id)) != hipSuccess) { c->err = hipGetErrorString(e); return bail(VP_ERR_HIP); }
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) { c->err = hipGetErrorString(e); return bail(VP_ERR_HIP); }
    c->own_stream = c->stream;
    const size_t B = (size_t)((c->maxb + 3) / 4 * 4);   // workspaces: the encoder may run the next multiple of 4 crops (forward_chunk)
    // fp8 mode: workspaces indexed by token row are sized for the padded row count the MXFP8 GEMM tiles need
    c->Mp = std::max<size_t>((B * 192 + 255) / 256 * 256, 512);
    const size_t M = c->fp8 ? c->Mp : B * 192;
    int rc = 0;
    void* stage = nullptr;
    if ((rc = dalloc(c, (char**)&stage, B * crop_bytes(VP_INPUT_F32_NCHW)))) return bail(rc);
    c->in_stage = stage;
    if ((rc = dalloc(c, &c->wh_stage, B * 2))) return bail(rc);
    if ((rc = dalloc(c, &c->x, M * D))) return bail(rc);
    if ((rc = dalloc(c, &c->y, M * D))) return bail(rc);
    if (c->fp8 && !c->sw.fuse_ln) { c->err = "the fp8 mode is built on the fused-LayerNorm path (unset VP_FUSE_LN)"; return bail(VP_ERR_INVALID); }
    if (c->sw.fuse_ln) {
        if ((rc = dalloc(c, &c->ln_part, M * (size_t)(D / 64) * 2))) return bail(rc);
        if ((rc = dalloc(c, &c->rowstat, M * 2))) return bail(rc);
    }
    if (c->fp8) {
        if ((rc = dalloc(c, &c->x8, M * D)) || (rc = dalloc(c, &c->xs8, M * (size_t)(D / 32))) || (rc = dalloc(c, &c->hs8, M * (size_t)(4 * D / 32)))) return bail(rc);
        if (hipMemset(c->x, 0, M * D * 4) != hipSuccess) { c->err = "hipMemset"; return bail(VP_ERR_HIP); }   // padding rows of the planes: read by fc2's residual epilogue
        if (hd == 64 && !c->sw.fp8_proj16) {   // VP_FP8_PROJ16=1: attn.proj stays on the fp16 kernels (parity test flips it; tile_rules.hip plan_chunk proj_fp8)
            if ((rc = dalloc(c, &c->y8, M * D)) || (rc = dalloc(c, &c->ys8, M * (size_t)(D / 32)))) return bail(rc);
            if (hipMemset(c->y8, 0, M * D) != hipSuccess || hipMemset(c->ys8, 0, M * (size_t)(D / 32)) != hipSuccess) { c->err = "hipMemset"; return bail(VP_ERR_HIP); }   // padding rows: zero codes
        }
    }
    if ((rc = dalloc(c, &c->qkv, M * 3 * D))) return bail(rc);
    if ((rc = dalloc(c, &c->hid, M * 4 * D))) return bail(rc);
    if ((rc = dalloc(c, &c->d1, B * 768 * 256))) return bail(rc);
    if ((rc = dalloc(c, &c->d2, B * 3072 * 256))) return bail(rc);
    if ((rc = dalloc(c, &c->hm, B * c->Kp * 3072))) return bail(rc);
    if ((rc = dalloc(c, &c->kp, B * c->Kp * 3))) return bail(rc);
    if (c->sw.fuse_ln && !c->fp8 && c->sw.splitk_on) {   // (the rows tile_rules.hip plan_chunk assumes)
        c->splitk_rows = (size_t)std::min<int>(c->maxb, SPLITK_MAX_CROPS) * 192;
        if ((rc = dalloc(c, &c->splitk_ws, (size_t)SPLITK_MAX_S * c->splitk_rows * D))) return bail(rc);
    }
    if ((rc = dalloc(c, &c->zero, (size_t)256))) return bail(rc);
    if (hipMemset(c->zero, 0, 512) != hipSuccess) { c->err = "hipMemset"; return bail(VP_ERR_HIP); }
    *out = c;
    return VP_OK;
}
int vp_infer_device(vp_handle c, const void* d_crops, int32_t fmt, int32_t n, const int32_t* d_org_wh, float* d_out, int32_t sync) {
    int rc = check_ready(c, fmt, n, d_crops, d_out);
    if (rc) return rc;
    const int cap = chunk_cap(c);
    for (int off = 0; off < n; off += cap) {
        const int nb = (n - off < cap) ? n - off : cap;
        const char* src = (const char*)d_crops + (size_t)off * crop_bytes(fmt);
        if ((rc = run_chunk(c, src, fmt, nb, d_org_wh ? d_org_wh + 2 * (size_t)off : nullptr, d_out + (size_t)off * c->Kp * 3))) return rc;
    }
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

int vp_infer_device_stream(vp_handle c, const void* d_crops, int32_t fmt, int32_t n, const int32_t* d_org_wh, float* d_out, void* caller_stream) {
    int rc = check_ready(c, fmt, n, d_crops, d_out, false);
    if (rc) return rc;
    const int cap = chunk_cap(c);
    return caller_ordered(c, (hipStream_t)caller_stream, n, [&]() -> int {
        for (int off = 0; off < n; off += cap) {   // vp_infer_device's chunks
            const int nb = (n - off < cap) ? n - off : cap;
            const char* src = (const char*)d_crops + (size_t)off * crop_bytes(fmt);
            if ((rc = run_chunk(c, src, fmt, nb, d_org_wh ? d_org_wh + 2 * (size_t)off : nullptr, d_out + (size_t)off * c->Kp * 3))) return rc;
        }
        return VP_OK;
    });
}

int vp_infer(vp_handle c, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out) {
    int rc = check_ready(c, fmt, n, crops, out);
    if (rc) return rc;
    const int cap = chunk_cap(c);
    if (n > cap && !c->slots[0].busy && !c->slots[1].busy) {
        // more than one chunk: through the two asynchronous slots, so that the upload of chunk i+1 and the download of chunk i-1
        // run under the compute of chunk i (fully overlapped when the caller's buffers are pinned; pageable buffers still work,
        // the runtime stages them synchronously)
        int pending[2], np = 0;
        for (int off = 0; off < n; off += cap) {
            const int nb = (n - off < cap) ? n - off : cap;
            int32_t slot = -1;
            rc = vp_infer_submit(c, (const char*)crops + (size_t)off * crop_bytes(fmt), fmt, nb, org_wh ? org_wh + 2 * (size_t)off : nullptr,
                                 out + (size_t)off * c->Kp * 3, &slot);
            if (rc) { for (int i = 0; i < np; ++i) vp_infer_wait(c, pending[i]); return rc; }
            pending[np++] = slot;
            if (np == 2) {
                if ((rc = vp_infer_wait(c, pending[0]))) { vp_infer_wait(c, pending[1]); return rc; }
                pending[0] = pending[1]; np = 1;
            }
        }
        for (int i = 0; i < np; ++i)
            if ((rc = vp_infer_wait(c, pending[i]))) return rc;
        return VP_OK;
    }
    for (int off = 0; off < n; off += cap) {
        const int nb = (n - off < cap) ? n - off : cap;
        const char* src = (const char*)crops + (size_t)off * crop_bytes(fmt);
        HIPCHK(c, hipMemcpyAsync(c->in_stage, src, (size_t)nb * crop_bytes(fmt), hipMemcpyHostToDevice, c->stream));
        if (org_wh) HIPCHK(c, hipMemcpyAsync(c->wh_stage, org_wh + 2 * (size_t)off, (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
        if ((rc = run_chunk(c, c->in_stage, fmt, nb, org_wh ? c->wh_stage : nullptr, c->kp))) return rc;
        HIPCHK(c, hipMemcpyAsync(out + (size_t)off * c->Kp * 3, c->kp, (size_t)nb * c->Kp * 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VP_OK;
}

// ---- asynchronous host path ----------------------------------------------------------------------------------------------
void* vp_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void vp_host_free(void* p) { if (p) hipHostFree(p); }

// stage_out: the D2H targets the slot's own pinned buffer and vp_infer_wait copies it to `out` (the group path: the caller's
// memory may be pageable, and an asynchronous copy to pageable memory is host-synchronous -- it would hold the submission until the
// compute is over and serialise the devices of a group)
// true when `p` is page-locked host memory the runtime knows (hipHostMalloc / vp_host_alloc / hipHostRegister): only such memory is
// copied asynchronously as it is
static bool host_ptr_is_pinned(const void* p) {
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // unknown to the runtime = pageable
    return a.type == hipMemoryTypeHost;
}

static int submit_impl(vp_handle c, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out, int32_t* slot_out, bool stage_out) {
    int rc = check_ready(c, fmt, n, crops, out);
    if (rc) return rc;
    if (!slot_out) return fail(c, VP_ERR_INVALID, "null slot pointer");
    if (n <= 0 || n > chunk_cap(c))
        return fail(c, VP_ERR_INVALID, c->flip_on ? "vp_infer_submit takes 1 .. max_batch / 2 crops per call while the flip-test mode is on" : "vp_infer_submit takes 1 .. max_batch crops per call");
    if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->d2h_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking));
    const int si = c->next_slot;
    vp_ctx::Slot& sl = c->slots[si];
    if (sl.busy) return fail(c, VP_ERR_STATE, "both slots in flight: call vp_infer_wait first");
    if (!sl.in) {
        char* q;
        if ((rc = dalloc(c, &q, (size_t)c->maxb * crop_bytes(VP_INPUT_F32_NCHW)))) return rc;
        sl.in = q;
    }
    if (!sl.wh && (rc = dalloc(c, &sl.wh, (size_t)c->maxb * 2))) return rc;
    if (!sl.kp && (rc = dalloc(c, &sl.kp, (size_t)c->maxb * c->Kmax * 3))) return rc;
    if (!sl.h2d) HIPCHK(c, hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming));
    if (!sl.done) HIPCHK(c, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    if (!sl.out) HIPCHK(c, hipEventCreateWithFlags(&sl.out, hipEventDisableTiming));
    // copy stream: H2D of this call (the slot's previous D2H finished: vp_infer_wait was called on it)
    const size_t in_bytes = (size_t)n * crop_bytes(fmt);
    if (stage_out && !host_ptr_is_pinned(crops)) {
        // the group path with pageable caller memory: staged through the slot's pinned buffer in 4 MiB pieces, so that this call never
        // waits for a device (hipMemcpyAsync from pageable memory held member i + 1's submission behind member i's staging)
        if (sl.host_in_cap < in_bytes) {
            if (sl.host_in) { HIPCHK(c, hipStreamSynchronize(c->copy_stream)); hipHostFree(sl.host_in); sl.host_in = nullptr; sl.host_in_cap = 0; }
            void* q = nullptr;
            HIPCHK(c, hipHostMalloc(&q, in_bytes, hipHostMallocDefault));
            sl.host_in = (char*)q; sl.host_in_cap = in_bytes;
        }
        const size_t piece = (size_t)4 << 20;
        for (size_t off = 0; off < in_bytes; off += piece) {
            const size_t len = in_bytes - off < piece ? in_bytes - off : piece;
            std::memcpy(sl.host_in + off, (const char*)crops + off, len);
            HIPCHK(c, hipMemcpyAsync((char*)sl.in + off, sl.host_in + off, len, hipMemcpyHostToDevice, c->copy_stream));
        }
    } else {
        HIPCHK(c, hipMemcpyAsync(sl.in, crops, in_bytes, hipMemcpyHostToDevice, c->copy_stream));
    }
    if (org_wh) HIPCHK(c, hipMemcpyAsync(sl.wh, org_wh, (size_t)n * 8, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(c, hipEventRecord(sl.h2d, c->copy_stream));
    // compute stream: after the upload
    HIPCHK(c, hipStreamWaitEvent(c->stream, sl.h2d, 0));
    if ((rc = run_chunk(c, sl.in, fmt, n, org_wh ? sl.wh : nullptr, sl.kp))) return rc;
    HIPCHK(c, hipEventRecord(sl.done, c->stream));
    // download stream: D2H of the keypoints after the compute
    HIPCHK(c, hipStreamWaitEvent(c->d2h_stream, sl.done, 0));
    float* dst = out;
    sl.user_out = nullptr;
    if (stage_out) {
        if (!sl.host_kp) {
            void* q = nullptr;
            HIPCHK(c, hipHostMalloc(&q, (size_t)c->maxb * c->Kmax * 12, hipHostMallocDefault));
            sl.host_kp = (float*)q;
        }
        dst = sl.host_kp;
        sl.user_out = out;
        sl.out_bytes = (size_t)n * c->Kp * 12;
    }
    HIPCHK(c, hipMemcpyAsync(dst, sl.kp, (size_t)n * c->Kp * 12, hipMemcpyDeviceToHost, c->d2h_stream));
    HIPCHK(c, hipEventRecord(sl.out, c->d2h_stream));
    sl.busy = true;
    *slot_out = si;
    c->next_slot = si ^ 1;
    return VP_OK;
}

int vp_infer_submit(vp_handle c, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out, int32_t* slot_out) {
    return submit_impl(c, crops, fmt, n, org_wh, out, slot_out, false);
}

int vp_infer_wait(vp_handle c, int32_t slot) {
    if (!c || slot < 0 || slot > 1) return VP_ERR_INVALID;
    vp_ctx::Slot& sl = c->slots[slot];
    if (!sl.busy) return fail(c, VP_ERR_STATE, "slot not in flight");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipEventSynchronize(sl.out));
    if (sl.user_out) { std::memcpy(sl.user_out, sl.host_kp, sl.out_bytes); sl.user_out = nullptr; }
    sl.busy = false;
    return VP_OK;
}

int vp_infer_flip(vp_handle c, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, const int32_t* flip_pairs,
                  int32_t n_pairs, int32_t shift_heatmap, float* out, float* heatmaps) {
    int rc = check_ready(c, fmt, n, crops, out ? (const void*)out : (const void*)heatmaps);
    if (rc) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && !flip_pairs)) return fail(c, VP_ERR_INVALID, "bad flip_pairs");
    if (n == 0) return VP_OK;   // nothing to do (and no async upload of the stack-lifetime partner table left in flight)
    std::vector<int32_t> partner(c->Kp);
    for (int k = 0; k < c->Kp; ++k) partner[k] = k;
    for (int i = 0; i < n_pairs; ++i) {
        const int a = flip_pairs[2 * i], b = flip_pairs[2 * i + 1];
        if (a < 0 || b < 0 || a >= c->Kp || b >= c->Kp) return fail(c, VP_ERR_INVALID, "flip pair index out of range");
        partner[a] = b;
        partner[b] = a;
    }
    const size_t hm_elems = (size_t)c->maxb * c->Kmax * 3072;
    if (!c->hm_keep && (rc = dalloc(c, &c->hm_keep, hm_elems))) return rc;
    if (!c->partner && (rc = dalloc(c, &c->partner, (size_t)c->Kmax))) return rc;
    HIPCHK(c, hipMemcpy(c->partner, partner.data(), (size_t)c->Kp * 4, hipMemcpyHostToDevice));   // synchronous: `partner` is a local
    for (int off = 0; off < n; off += c->maxb) {
        const int nb = (n - off < c->maxb) ? n - off : c->maxb;
        const char* src = (const char*)crops + (size_t)off * crop_bytes(fmt);
        HIPCHK(c, hipMemcpyAsync(c->in_stage, src, (size_t)nb * crop_bytes(fmt), hipMemcpyHostToDevice, c->stream));
        if (org_wh) HIPCHK(c, hipMemcpyAsync(c->wh_stage, org_wh + 2 * (size_t)off, (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
        if ((rc = forward_chunk(c, c->in_stage, fmt, nb, false, false))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->hm_keep, c->hm, (size_t)nb * c->Kp * 3072 * 4, hipMemcpyDeviceToDevice, c->stream));
        if ((rc = forward_chunk(c, c->in_stage, fmt, nb, false, true))) return rc;         // mirrored crops -> c->hm
        HIPCHK(c, vp::flip_merge_launch(c->hm_keep, c->hm, c->partner, nb, c->Kp, shift_heatmap ? 1 : 0, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->hm, c->hm_keep, (size_t)nb * c->Kp * 3072 * 4, hipMemcpyDeviceToDevice, c->stream));
        if (heatmaps) HIPCHK(c, hipMemcpyAsync(heatmaps + (size_t)off * c->Kp * 3072, c->hm, (size_t)nb * c->Kp * 3072 * 4, hipMemcpyDeviceToHost, c->stream));
        if (out) {
            if ((rc = decode_chunk(c, org_wh ? c->wh_stage : nullptr, c->kp, nb, false))) return rc;
            HIPCHK(c, hipMemcpyAsync(out + (size_t)off * c->Kp * 3, c->kp, (size_t)nb * c->Kp * 12, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VP_OK;
}

// ---- flip-test mode ------------------------------------------------------------------------------------------------------
int vp_set_flip_test(vp_handle c, const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap) {
    if (!c) return VP_ERR_INVALID;
    if (!c->loaded) return fail(c, VP_ERR_STATE, "weights not loaded: call vp_load_weights first");
    std::vector<int32_t> partner((size_t)c->Kmax);
    std::string why;
    if (flip_partner_table(c->Kp, flip_pairs, n_pairs, partner.data(), &why)) return fail(c, VP_ERR_INVALID, "vp_set_flip_test: " + why);
    for (int k = c->Kp; k < c->Kmax; ++k) partner[k] = k;
    if (c->maxb < 2)
        return fail(c, VP_ERR_STATE, "vp_set_flip_test: a crop and its mirror image share the forward batch, which needs max_batch >= 2 (this handle has 1)");
    if (c->slots[0].busy || c->slots[1].busy) return fail(c, VP_ERR_STATE, "vp_set_flip_test with a vp_infer_submit in flight: call vp_infer_wait first");
    int rc = vp_synchronize(c);   // a previous table may still be read by enqueued work (also on a caller's stream)
    if (rc) return rc;
    if (!c->flip_table && (rc = dalloc(c, &c->flip_table, (size_t)c->Kmax))) return rc;
    HIPCHK(c, hipMemcpy(c->flip_table, partner.data(), (size_t)c->Kmax * 4, hipMemcpyHostToDevice));   // synchronous: `partner` is a local
    c->flip_pairs.assign(flip_pairs, flip_pairs + 2 * (size_t)n_pairs);
    c->flip_shift = shift_heatmap ? 1 : 0;
    c->flip_on = true;
    c->flip_gen = ++c->flip_counter;   // never the value of an earlier set: a graph captured under another table or shift is not replayed
    return VP_OK;
}

int vp_clear_flip_test(vp_handle c) {
    if (!c) return VP_ERR_INVALID;
    if (c->slots[0].busy || c->slots[1].busy) return fail(c, VP_ERR_STATE, "vp_clear_flip_test with a vp_infer_submit in flight: call vp_infer_wait first");
    c->flip_on = false;
    c->flip_gen = 0;   // the graphs of the plain mode are valid again
    c->flip_pairs.clear();
    return VP_OK;
}

int vp_flip_test_enabled(vp_handle c) { return c && c->flip_on ? 1 : 0; }

int vp_dbg_flip_partner(int32_t k, const int32_t* flip_pairs, int32_t n_pairs, int32_t* partner) {
    std::string why;
    std::vector<int32_t> tmp((size_t)(k > 0 ? k : 0));
    const int rc = flip_partner_table(k, flip_pairs, n_pairs, partner ? partner : tmp.data(), &why);
    if (rc) g_create_error = why;
    return rc;
}

int vp_dbg_flip_layout(int32_t n, int32_t rows, int32_t* src, int32_t* mirror) {
    if (n <= 0 || rows < 2 * n || !src || !mirror) return VP_ERR_INVALID;
    for (int bo = 0; bo < rows; ++bo) {
        int s_, m_;
        vp::flip_twin_layout(bo, n, &s_, &m_);
        src[bo] = s_; mirror[bo] = m_;
    }
    return VP_OK;
}

int vp_infer_heatmaps(vp_handle c, const void* crops, int32_t fmt, int32_t n, float* heatmaps) {
    int rc = check_ready(c, fmt, n, crops, heatmaps);
    if (rc) return rc;
    const int cap = chunk_cap(c);
    const size_t map_bytes = (size_t)c->Kp * 3072 * 4;
    for (int off = 0; off < n; off += cap) {
        const int nb = (n - off < cap) ? n - off : cap;
        HIPCHK(c, hipMemcpyAsync(c->in_stage, (const char*)crops + (size_t)off * crop_bytes(fmt), (size_t)nb * crop_bytes(fmt), hipMemcpyHostToDevice, c->stream));
        if ((rc = forward_mode_chunk(c, c->in_stage, fmt, nb))) return rc;
        if (c->flip_on) {   // the averaged maps, materialised in the straight crops' slots (every second one of the interleaved batch)
            HIPCHK(c, vp::flip_merge_launch(c->hm, c->hm + (size_t)c->Kp * 3072, c->flip_table, nb, c->Kp, c->flip_shift, c->stream, 1));
            HIPCHK(c, hipMemcpy2DAsync(heatmaps + (size_t)off * c->Kp * 3072, map_bytes, c->hm, 2 * map_bytes, map_bytes, (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        } else {
            HIPCHK(c, hipMemcpyAsync(heatmaps + (size_t)off * c->Kp * 3072, c->hm, (size_t)nb * map_bytes, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VP_OK;
}

int vp_infer_tokens(vp_handle c, const void* crops, int32_t fmt, int32_t n, float* tokens) {
    int rc = check_ready(c, fmt, n, crops, tokens);
    if (rc) return rc;
    if (!c->tok && (rc = dalloc(c, &c->tok, (size_t)c->maxb * 192 * c->D))) return rc;
    for (int off = 0; off < n; off += c->maxb) {
        const int nb = (n - off < c->maxb) ? n - off : c->maxb;
        HIPCHK(c, hipMemcpyAsync(c->in_stage, (const char*)crops + (size_t)off * crop_bytes(fmt), (size_t)nb * crop_bytes(fmt), hipMemcpyHostToDevice, c->stream));
        if ((rc = forward_chunk(c, c->in_stage, fmt, nb, true))) return rc;
        HIPCHK(c, hipMemcpyAsync(tokens + (size_t)off * 192 * c->D, c->tok, (size_t)nb * 192 * c->D * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VP_OK;
}

// ---- ViTPose+ (expert) handles --------------------------------------------------------------------------------------------
int vp_expert_info(vp_handle c, int32_t* n_experts, int32_t* part_features, int32_t* k_per_expert) {
    if (!c) return VP_ERR_INVALID;
    if (!c->loaded) return fail(c, VP_ERR_STATE, "weights not loaded: call vp_load_weights first");
    if (n_experts) *n_experts = c->n_experts;
    if (part_features) *part_features = c->part_features;
    if (k_per_expert)
        for (int e = 0; e < c->n_experts && e < 8; ++e) k_per_expert[e] = c->ex_heads[e].K;
    return VP_OK;
}

int vp_set_expert(vp_handle c, int32_t e) {
    if (!c) return VP_ERR_INVALID;
    if (!c->loaded) return fail(c, VP_ERR_STATE, "weights not loaded: call vp_load_weights first");
    if (!c->n_experts) return fail(c, VP_ERR_STATE, "vp_set_expert: the handle holds a plain (single-dataset) checkpoint, not a ViTPose+ one");
    if (e < 0 || e >= c->n_experts) return fail(c, VP_ERR_INVALID, "expert id " + std::to_string(e) + " outside [0, " + std::to_string(c->n_experts) + ")");
    if (c->slots[0].busy || c->slots[1].busy) return fail(c, VP_ERR_STATE, "vp_set_expert with a vp_infer_submit in flight: call vp_infer_wait first");
    const int k_before = c->Kp;
    use_expert(c, e);
    if (c->flip_on && c->Kp != k_before) {   // the pairs were validated against the previous head's joints and say nothing about this one's
        vp_clear_flip_test(c);
        return fail(c, VP_ERR_STATE, "vp_set_expert: expert " + std::to_string(e) + " is active, but its head has " + std::to_string(c->Kp) + " joints, not " +
                                         std::to_string(k_before) + ": the flip-test mode was cleared -- call vp_set_flip_test with this dataset's pairs");
    }
    return VP_OK;
}

int vp_infer_experts(vp_handle c, const void* crops, int32_t fmt, int32_t n, const int32_t* expert_ids, const int32_t* org_wh, float* out) {
    int rc = check_ready(c, fmt, n, crops, out);
    if (rc) return rc;
    if (!c->n_experts) return fail(c, VP_ERR_STATE, "vp_infer_experts: the handle holds a plain (single-dataset) checkpoint, not a ViTPose+ one");
    if (n > 0 && !expert_ids) return fail(c, VP_ERR_INVALID, "null expert_ids");
    for (int i = 0; i < n; ++i)
        if (expert_ids[i] < 0 || expert_ids[i] >= c->n_experts)
            return fail(c, VP_ERR_INVALID, "expert id " + std::to_string(expert_ids[i]) + " of crop " + std::to_string(i) + " outside [0, " + std::to_string(c->n_experts) + ")");
    if (c->slots[0].busy || c->slots[1].busy) return fail(c, VP_ERR_STATE, "vp_infer_experts with a vp_infer_submit in flight: call vp_infer_wait first");
    if (c->flip_on) return fail(c, VP_ERR_STATE, "vp_infer_experts does not run under the flip-test mode (one partner table per handle, not per crop): call vp_clear_flip_test first");
    // per chunk, the crops in expert order (stable): each expert is one contiguous segment, so that mlp.fc2's m-tiles see one expert and the head runs once per expert
    const int saved = c->expert, D = c->D;
    const size_t cb = crop_bytes(fmt), B = (size_t)((c->maxb + 3) / 4 * 4);
    std::vector<int32_t> ids(2 * B), wh(2 * (size_t)c->maxb);
    std::vector<int> order(c->maxb);
    std::vector<float> kp((size_t)c->maxb * c->Kmax * 3);
    auto run = [&]() -> int {
        for (int off = 0; off < n; off += c->maxb) {
            const int nb = (n - off < c->maxb) ? n - off : c->maxb;
            for (int j = 0; j < nb; ++j) order[j] = off + j;
            std::stable_sort(order.begin(), order.begin() + nb, [&](int a, int b) { return expert_ids[a] < expert_ids[b]; });
            bool identity = true;
            for (int j = 0; j < nb; ++j) identity = identity && order[j] == off + j;
            if (identity) {
                HIPCHK(c, hipMemcpyAsync(c->in_stage, (const char*)crops + (size_t)off * cb, (size_t)nb * cb, hipMemcpyHostToDevice, c->stream));
            } else {   // one upload in the caller's order, then a device gather into expert order
                if (c->mix_stage_cap < B * cb) {
                    if (c->mix_stage) {
                        HIPCHK(c, hipStreamSynchronize(c->stream));
                        for (auto it = c->allocs.begin(); it != c->allocs.end(); ++it)
                            if (*it == c->mix_stage) { c->allocs.erase(it); break; }
                        HIPCHK(c, hipFree(c->mix_stage));
                        c->mix_stage = nullptr; c->mix_stage_cap = 0;
                    }
                    char* q = nullptr;
                    int arc = dalloc(c, &q, B * cb);
                    if (arc) return arc;
                    c->mix_stage = q; c->mix_stage_cap = B * cb;
                }
                HIPCHK(c, hipMemcpyAsync(c->mix_stage, (const char*)crops + (size_t)off * cb, (size_t)nb * cb, hipMemcpyHostToDevice, c->stream));
            }
            if (org_wh) {
                for (int j = 0; j < nb; ++j) { wh[2 * j] = org_wh[2 * (size_t)order[j]]; wh[2 * j + 1] = org_wh[2 * (size_t)order[j] + 1]; }
                HIPCHK(c, hipMemcpyAsync(c->wh_stage, wh.data(), (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
            }
            const int32_t* d_wh = org_wh ? c->wh_stage : nullptr;
            // segments of the chunk: (expert, first crop, count); ids[B + j] = the gather order
            std::vector<int> seg_e, seg_s;
            for (int j = 0; j < nb; ++j) {
                ids[j] = expert_ids[order[j]];
                ids[B + j] = order[j] - off;
                if (j == 0 || ids[j] != ids[j - 1]) { seg_e.push_back(ids[j]); seg_s.push_back(j); }
            }
            seg_s.push_back(nb);
            for (size_t j = nb; j < B; ++j) ids[j] = ids[nb - 1];   // encoder padding crops repeat the last crop (pick_run_batch)
            if (!identity) {
                HIPCHK(c, hipMemcpyAsync(c->expert_ids, ids.data(), 2 * B * 4, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, vp::gather_crops_launch(c->mix_stage, c->in_stage, c->expert_ids + B, nb, cb, c->stream));
            }
            if (seg_e.size() == 1) {   // one expert: the single-dataset path as it is (tile rules, split-K, hipGraph replay keyed on the expert)
                use_expert(c, seg_e[0]);
                if ((rc = run_chunk(c, c->in_stage, fmt, nb, d_wh, c->kp))) return rc;
            } else {
                // mixed: the encoder once (mlp.fc2 of every expert in one launch per layer: GemmArgs::expert), then head + decode per expert segment.
                // Eager: the expert pattern shapes the head launches, so a captured graph would have to be keyed on it (the single-expert path above replays)
                if (identity) HIPCHK(c, hipMemcpyAsync(c->expert_ids, ids.data(), B * 4, hipMemcpyHostToDevice, c->stream));
                c->mix_expert = c->expert_ids;
                c->mix_bounds.assign(seg_s.begin() + 1, seg_s.end() - 1);
                rc = forward_chunk(c, c->in_stage, fmt, nb, false, false, false);
                c->mix_expert = nullptr;
                c->mix_bounds.clear();
                if (rc) return rc;
                for (size_t s = 0; s < seg_e.size(); ++s) {
                    const int s0 = seg_s[s], cnt = seg_s[s + 1] - s0;
                    use_expert(c, seg_e[s]);
                    float* hm = c->hm + (size_t)s0 * c->Kmax * 3072;
                    if ((rc = head_chunk(c, c->y + (size_t)s0 * 192 * D, cnt, hm, plan_head(c->sw, D, cnt, c->fin_rows)))) return rc;
                    LAUNCH(c, VP_PROF_DECODE, 0.0, 4.0 * cnt * c->Kp * 3072.0 + 12.0 * cnt * c->Kp,
                           vp::decode_launch(hm, d_wh ? d_wh + 2 * (size_t)s0 : nullptr, c->kp + (size_t)s0 * c->Kmax * 3, cnt, c->Kp, c->stream));
                }
            }
            HIPCHK(c, hipMemcpyAsync(kp.data(), c->kp, (size_t)nb * c->Kmax * 12, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));   // also keeps ids / wh (host vectors) alive until their uploads are done
            // segment s's crops lie at [s0 Kmax + (j - s0) K_e] x 3 floats: back to the caller's order, joints beyond K_e = 0
            for (size_t s = 0; s < seg_e.size(); ++s) {
                const int K = c->ex_heads[seg_e[s]].K;
                for (int j = seg_s[s]; j < seg_s[s + 1]; ++j) {
                    float* dst = out + (size_t)order[j] * c->Kmax * 3;
                    std::memcpy(dst, &kp[((size_t)seg_s[s] * c->Kmax + (size_t)(j - seg_s[s]) * K) * 3], (size_t)K * 12);
                    std::memset(dst + (size_t)K * 3, 0, (size_t)(c->Kmax - K) * 12);
                }
            }
        }
        return VP_OK;
    };
    rc = run();
    use_expert(c, saved);
    return rc;
}

int vp_infer_frames(vp_handle c, const vp_frame* frames, int32_t n_frames, int32_t on_device, const int32_t* p9, int32_t n, float* out) {
    if (!c) return VP_ERR_INVALID;
    std::vector<int32_t> bands((size_t)(n_frames > 0 ? n_frames : 0) * 2);
    std::string why;
    if (frame_plan(frames, n_frames, p9, n, bands.data(), &why)) return fail(c, VP_ERR_INVALID, why);   // before any copy or launch
    int rc = check_ready(c, VP_INPUT_U8_NHWC, n, p9, out);
    if (rc || n == 0) return rc;
    std::vector<vp::CropRec> recs;
    if ((rc = stage_frames(c, frames, n_frames, on_device != 0, p9, n, bands.data(), recs))) return rc;
    if (!c->crecs && (rc = dalloc(c, &c->crecs, (size_t)c->maxb))) return rc;
    std::vector<int32_t> wh((size_t)c->maxb * 2);
    const int cap = chunk_cap(c);
    for (int off = 0; off < n; off += cap) {   // vp_infer's chunks: the same crops per chunk, so the same bits
        const int nb = (n - off < cap) ? n - off : cap;
        HIPCHK(c, hipMemcpyAsync(c->crecs, recs.data() + off, (size_t)nb * sizeof(vp::CropRec), hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, VP_PROF_IM2COL, 0.0, (double)nb * 256 * 192 * 3 * 5, vp::crop_resize_launch(c->crecs, (uint8_t*)c->in_stage, nb, c->stream));
        // decode scales by the padded-canvas size (pw, ph) of each crop = the image pre_img receives
        for (int i = 0; i < nb; ++i) { wh[2 * i] = p9[9 * (size_t)(off + i) + 7]; wh[2 * i + 1] = p9[9 * (size_t)(off + i) + 8]; }
        HIPCHK(c, hipMemcpyAsync(c->wh_stage, wh.data(), (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // recs / wh are rewritten for the next chunk
        if ((rc = run_chunk(c, c->in_stage, VP_INPUT_U8_NHWC, nb, c->wh_stage, c->kp))) return rc;
        HIPCHK(c, hipMemcpyAsync(out + (size_t)off * c->Kp * 3, c->kp, (size_t)nb * c->Kp * 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VP_OK;
}

// the one-frame case of vp_infer_frames
int vp_infer_frame(vp_handle c, const uint8_t* frame, int32_t fh, int32_t fw, const int32_t* crop_params, int32_t n, float* out) {
    int rc = check_ready(c, VP_INPUT_U8_NHWC, n, frame, out);
    if (rc) return rc;
    if (fh <= 0 || fw <= 0 || (n > 0 && !crop_params)) return fail(c, VP_ERR_INVALID, "bad frame geometry");
    const vp_frame fr{frame, fh, fw};
    std::vector<int32_t> p9((size_t)n * 9);
    for (int i = 0; i < n; ++i) {
        p9[9 * (size_t)i] = 0;
        std::memcpy(&p9[9 * (size_t)i + 1], crop_params + 8 * (size_t)i, 32);
    }
    return vp_infer_frames(c, &fr, 1, 0, p9.data(), n, out);
}

int vp_dbg_frame_plan(const vp_frame* frames, int32_t n_frames, const int32_t* params9, int32_t n, int32_t* bands) {
    std::string why;
    const int rc = frame_plan(frames, n_frames, params9, n, bands, &why);
    if (rc) g_create_error = why;
    return rc;
}

int vp_infer_boxes_stream(vp_handle c, const vp_frame* frames, int32_t n_frames, const float* d_xyxy, int32_t row_stride, const int32_t* d_frame_idx,
                          int32_t n, int32_t pad, float* d_out, int32_t* d_crop_params, int32_t* d_status, void* caller_stream) {
    if (!c) return VP_ERR_INVALID;
    // every host argument is checked before anything is enqueued
    if (n > 0 && (!frames || !d_xyxy || !d_out)) return fail(c, VP_ERR_INVALID, "null frame table, box or output pointer");
    std::vector<int32_t> hw((size_t)std::max(n > 0 ? n_frames : 0, 0) * 2);
    for (size_t f = 0; f < hw.size() / 2; ++f) { hw[2 * f] = frames[f].h; hw[2 * f + 1] = frames[f].w; }
    std::string why;
    if (box_args(n_frames, hw.data(), 2, row_stride, n, pad, &why)) return fail(c, VP_ERR_INVALID, why);
    int rc = check_ready(c, VP_INPUT_U8_NHWC, n, d_xyxy, d_out, false);
    if (rc || n == 0) return rc;
    for (int f = 0; f < n_frames; ++f) {   // device memory of the handle's device, the whole frame inside one allocation (as stage_frames checks)
        const vp_frame& fr = frames[f];
        hipPointerAttribute_t a;
        std::memset(&a, 0, sizeof(a));
        void* base = nullptr;
        size_t size = 0;
        bool ok = fr.data && hipPointerGetAttributes(&a, fr.data) == hipSuccess && a.type == hipMemoryTypeDevice && a.device == c->cfg.device_id;
        ok = ok && hipMemGetAddressRange(&base, &size, (void*)fr.data) == hipSuccess && fr.data + (size_t)fr.h * fr.w * 3 <= (const uint8_t*)base + size;
        if (!ok) {
            (void)hipGetLastError();
            return fail(c, VP_ERR_INVALID, "frame " + std::to_string(f) + " is not device memory of device " + std::to_string(c->cfg.device_id) +
                                               " (or runs past the end of its allocation)");
        }
    }
    // the chunk's crop records / decode sizes / offsets live in handle buffers sized by max_batch, allocated on the first call
    if (!c->crecs && (rc = dalloc(c, &c->crecs, (size_t)c->maxb))) return rc;
    if (!c->box_aux && (rc = dalloc(c, &c->box_aux, (size_t)c->maxb * 4))) return rc;
    const int cap = chunk_cap(c);
    return caller_ordered(c, (hipStream_t)caller_stream, n, [&]() -> int {
        for (int off = 0; off < n; off += cap) {   // vp_infer_frames' chunks: the same crops per chunk, so the same plan and bits
            const int nb = (n - off < cap) ? n - off : cap;
            // geometry + crop run eagerly in front of the chunk's graph: the frame pointers change from call to call, the graph's buffers do not
            for (int f0 = 0; f0 < n_frames; f0 += vp::BOX_FRAMES_PER_LAUNCH) {
                vp::BoxFrames bf;
                std::memset(&bf, 0, sizeof(bf));
                bf.f0 = f0; bf.count = std::min(n_frames - f0, vp::BOX_FRAMES_PER_LAUNCH); bf.n_frames = n_frames;
                for (int j = 0; j < bf.count; ++j) { bf.data[j] = frames[f0 + j].data; bf.h[j] = frames[f0 + j].h; bf.w[j] = frames[f0 + j].w; }
                LAUNCH(c, VP_PROF_IM2COL, 0.0, 64.0 * nb,
                       vp::box_geometry_launch(bf, d_xyxy + (size_t)off * row_stride, row_stride, d_frame_idx ? d_frame_idx + off : nullptr, nb, pad,
                                               (const uint8_t*)c->zero, c->crecs, c->wh_stage, c->box_aux,
                                               d_crop_params ? d_crop_params + (size_t)off * 9 : nullptr, d_status ? d_status + off : nullptr, c->stream));
            }
            LAUNCH(c, VP_PROF_IM2COL, 0.0, (double)nb * 256 * 192 * 3 * 5, vp::crop_resize_launch(c->crecs, (uint8_t*)c->in_stage, nb, c->stream));
            if ((rc = run_chunk(c, c->in_stage, VP_INPUT_U8_NHWC, nb, c->wh_stage, d_out + (size_t)off * c->Kp * 3, c->box_aux))) return rc;
        }
        return VP_OK;
    });
}

int vp_dbg_box_geometry(const float* xyxy, int32_t row_stride, const int32_t* frame_idx, const int32_t* frame_hw, int32_t n_frames, int32_t n, int32_t pad,
                        int32_t* out9, int32_t* status) {
    std::string why;
    if (n > 0 && (!xyxy || (n_frames > 0 && !frame_hw))) why = "null box or frame table";
    const int rc = why.empty() ? box_args(n_frames, frame_hw, 2, row_stride, n, pad, &why) : (int)VP_ERR_INVALID;
    if (rc) { g_create_error = why; return rc; }
    for (int i = 0; i < n; ++i) {   // what box_geometry_kernel computes for box i
        const int32_t f = frame_idx ? frame_idx[i] : 0;
        int32_t p8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int st = vp::BOX_BAD_FRAME;
        if (f >= 0 && f < n_frames) {
            const float* b = xyxy + (size_t)i * row_stride;
            st = vp::box_geometry(b[0], b[1], b[2], b[3], frame_hw[2 * (size_t)f], frame_hw[2 * (size_t)f + 1], pad, p8);
            if (st != vp::BOX_OK) std::memset(p8, 0, sizeof(p8));
        }
        if (out9) {
            out9[9 * (size_t)i] = st == vp::BOX_OK ? f : 0;
            std::memcpy(out9 + 9 * (size_t)i + 1, p8, sizeof(p8));
        }
        if (status) status[i] = st;
    }
    return VP_OK;
}

// decode of host heatmaps on device `device_id`: partner == null: [n, k, 64, 48] as they are; else the interleaved [2 n, k, 64, 48] of the flip-test mode
static int decode_host(int32_t device_id, const float* heatmaps, int32_t n, int32_t k, const int32_t* partner, int32_t shift, const int32_t* org_wh, float* out) {
    if (!heatmaps || !out || n <= 0 || k <= 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, VP_ERR_HIP, "no HIP device available (no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, VP_ERR_INVALID, "device_id out of range");
    vp_ctx* c = nullptr;   // errors below are reported through the create-error slot
    HIPCHK(c, hipSetDevice(device_id));
    float *d_hm = nullptr, *d_out = nullptr;
    int32_t *d_wh = nullptr, *d_partner = nullptr;
    const size_t hb = (size_t)n * k * 3072 * 4 * (partner ? 2 : 1), ob = (size_t)n * k * 12;
    int rc = VP_OK;
    hipError_t e = hipMalloc((void**)&d_hm, hb);
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, ob);
    if (e == hipSuccess) e = hipMemcpy(d_hm, heatmaps, hb, hipMemcpyHostToDevice);
    if (e == hipSuccess && org_wh) {
        e = hipMalloc((void**)&d_wh, (size_t)n * 8);
        if (e == hipSuccess) e = hipMemcpy(d_wh, org_wh, (size_t)n * 8, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && partner) {
        e = hipMalloc((void**)&d_partner, (size_t)k * 4);
        if (e == hipSuccess) e = hipMemcpy(d_partner, partner, (size_t)k * 4, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = partner ? vp::decode_flip_launch(d_hm, d_partner, shift ? 1 : 0, d_wh, d_out, n, k, nullptr) : vp::decode_launch(d_hm, d_wh, d_out, n, k, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(nullptr, VP_ERR_HIP, std::string(partner ? "vp_dbg_decode_flip: " : "vp_decode_only: ") + hipGetErrorString(e));
    if (d_hm) hipFree(d_hm);
    if (d_out) hipFree(d_out);
    if (d_wh) hipFree(d_wh);
    if (d_partner) hipFree(d_partner);
    return rc;
}

int vp_decode_only(int32_t device_id, const float* heatmaps, int32_t n, int32_t k, const int32_t* org_wh, float* out) {
    return decode_host(device_id, heatmaps, n, k, nullptr, 0, org_wh, out);
}

int vp_dbg_decode_flip(int32_t device_id, const float* heatmaps2, int32_t n, int32_t k, const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap,
                       const int32_t* org_wh, float* out) {
    if (k <= 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    std::vector<int32_t> partner((size_t)k);
    std::string why;
    if (flip_partner_table(k, flip_pairs, n_pairs, partner.data(), &why)) return fail(nullptr, VP_ERR_INVALID, why);
    return decode_host(device_id, heatmaps2, n, k, partner.data(), shift_heatmap, org_wh, out);
}

// ---- multi-GPU group (one process, N devices): crops sharded contiguously, weights replicated ------------------------------
struct vp_group {
    std::vector<vp_ctx*> h;
    int peer_missing = 0;        // ordered device pairs without peer access (their all-gather copies are staged through the host)
    std::vector<float*> d_all;   // per device: [max_total, K, 3] keypoints of EVERY shard (vp_group_infer_allgather)
    size_t all_cap = 0;
    std::string err;
};
namespace { thread_local std::string g_group_error; }

int vp_group_create(vp_group_handle* out, const vp_config* cfg, const int32_t* device_ids, int32_t n_devices) {
    if (!out || !cfg || !device_ids || n_devices <= 0) { g_group_error = "null argument"; return VP_ERR_INVALID; }
    *out = nullptr;
    vp_group* g = new vp_group();
    for (int i = 0; i < n_devices; ++i) {
        vp_config c = *cfg;
        c.device_id = device_ids[i];
        vp_handle h = nullptr;
        int rc = vp_create(&h, &c);
        if (rc) { g_group_error = std::string("device ") + std::to_string(device_ids[i]) + ": " + vp_last_error(nullptr); vp_group_destroy(g); return rc; }
        g->h.push_back(h);
    }
    // peer access for the device-side all-gather (xGMI links are point to point: one copy per pair)
    for (int i = 0; i < n_devices; ++i)
        for (int j = 0; j < n_devices; ++j)
            if (i != j) {
                hipSetDevice(device_ids[i]);
                int can = 0;
                bool ok = false;
                if (hipDeviceCanAccessPeer(&can, device_ids[i], device_ids[j]) == hipSuccess && can) {
                    hipError_t e = hipDeviceEnablePeerAccess(device_ids[j], 0);
                    ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
                }
                if (!ok) { (void)hipGetLastError(); ++g->peer_missing; }   // not fatal: hipMemcpyPeerAsync stages such a pair through the host
            }
    *out = g;
    return VP_OK;
}

int vp_group_size(vp_group_handle g) { return g ? (int)g->h.size() : 0; }
int vp_group_peer_access_missing(vp_group_handle g) { return g ? g->peer_missing : -1; }

int vp_group_load_weights(vp_group_handle g, const vp_tensor_desc* tensors, int32_t n_tensors) {
    if (!g) return VP_ERR_INVALID;
    for (auto* h : g->h) {
        int rc = vp_load_weights(h, tensors, n_tensors);
        if (rc) { g->err = h->err; return rc; }
    }
    return VP_OK;
}

// shard i of n crops over w devices: [off, off + cnt), contiguous, ceil(n / w) per device (the last ones may be short or empty)
static void group_shard(int n, int w, int i, int& off, int& cnt) {
    const int per = (n + w - 1) / w;
    off = per * i < n ? per * i : n;
    cnt = n - off < per ? n - off : per;
}

// the whole plan of a call: rounds of (devices x max_batch) crops, entry e = round * w + device -> [offs[e], offs[e] + cnts[e])
static int group_plan(int n, int w, int maxb, std::vector<int>& offs, std::vector<int>& cnts) {
    offs.clear(); cnts.clear();
    if (n < 0 || w <= 0 || maxb <= 0) return -1;
    const long per_round = (long)w * maxb;
    for (long r0 = 0; r0 < n; r0 += per_round) {
        const int nr = (int)(n - r0 < per_round ? n - r0 : per_round);
        for (int i = 0; i < w; ++i) {
            int off, cnt;
            group_shard(nr, w, i, off, cnt);
            offs.push_back((int)r0 + off);
            cnts.push_back(cnt);
        }
    }
    return (int)offs.size();
}

int vp_dbg_group_plan(int32_t n, int32_t w, int32_t maxb, int32_t* offs, int32_t* cnts, int32_t cap) {
    std::vector<int> o, k;
    const int e = group_plan(n, w, maxb, o, k);
    if (e < 0 || cap < 0 || (cap > 0 && (!offs || !cnts))) return -1;
    for (int i = 0; i < e && i < cap; ++i) { offs[i] = o[i]; cnts[i] = k[i]; }
    return e;
}

// The two-phase schedule of a group call, as ONE function for the real path (group_run) and for the host-only trace
// (vp_dbg_group_trace): per round of `w` plan entries, phase 1 calls submit(member, off, cnt) for EVERY member with work before phase 2
// calls wait(member) for any of them.  submit returns 0 or an error code; on an error every member already submitted in this round
// is waited for (drained) before the error is returned, so no slot of any member stays in flight.
extern "C++" {
template <class Submit, class Wait>
static int group_rounds(const std::vector<int>& offs, const std::vector<int>& cnts, int w, Submit submit, Wait wait) {
    const int entries = (int)offs.size();
    for (int e0 = 0; e0 < entries; e0 += w) {
        std::vector<char> inflight(w, 0);
        auto drain = [&](int from) { for (int i = from; i < w; ++i) if (inflight[i]) { wait(i); inflight[i] = 0; } };
        for (int i = 0; i < w; ++i) {                    // phase 1 -- enqueue on every member; nothing here waits for a device
            if (cnts[e0 + i] <= 0) continue;
            const int rc = submit(i, offs[e0 + i], cnts[e0 + i]);
            if (rc) { drain(0); return rc; }
            inflight[i] = 1;
        }
        for (int i = 0; i < w; ++i)                      // phase 2 -- collect
            if (inflight[i]) {
                inflight[i] = 0;
                const int rc = wait(i);
                if (rc) { drain(i + 1); return rc; }
            }
    }
    return VP_OK;
}
}   // extern "C++"

// host-only: the order in which a call of n crops on w members of max_batch maxb submits (+ (member + 1)) and waits (- (member + 1)),
// with stub members (tests/test_host_logic.py: every submission of a round precedes its first wait)
int vp_dbg_group_trace(int32_t n, int32_t w, int32_t maxb, int32_t* trace, int32_t cap) {
    std::vector<int> offs, cnts;
    if (group_plan(n, w, maxb, offs, cnts) < 0 || cap < 0 || (cap > 0 && !trace)) return -1;
    int len = 0;
    auto put = [&](int v) { if (len < cap) trace[len] = v; ++len; };
    group_rounds(offs, cnts, w, [&](int i, int, int) { put(i + 1); return 0; }, [&](int i) { put(-(i + 1)); return 0; });
    return len;
}

static int group_run(vp_group* g, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out, float* const* d_all) {
    if (!g || n < 0 || (n > 0 && (!crops || (!out && !d_all)))) return VP_ERR_INVALID;
    const int w = (int)g->h.size();
    const int K = g->h[0]->Kp;
    std::vector<float> scratch;
    if (!out) { scratch.resize((size_t)n * K * 3); out = scratch.data(); }
    std::vector<int> offs, cnts;
    for (int i = 1; i < w; ++i)   // one plan for all members: they must agree on the flip-test mode (vp_group_set_flip_test sets them alike)
        if (g->h[i]->flip_on != g->h[0]->flip_on || (g->h[0]->flip_on && (g->h[i]->flip_shift != g->h[0]->flip_shift || g->h[i]->flip_pairs != g->h[0]->flip_pairs))) {
            g->err = "the members of the group disagree on the flip-test mode (member " + std::to_string(i) + " against member 0): set it with vp_group_set_flip_test";
            return VP_ERR_STATE;
        }
    if (group_plan(n, w, chunk_cap(g->h[0]), offs, cnts) < 0) return VP_ERR_INVALID;
    std::vector<int> slot(w, -1);
    // phase 1 per member: upload (pinned caller memory as it is, pageable memory through the member's pinned staging buffer), model,
    // decode, download into the member's pinned staging buffer, and the peer copies of the device-side all-gather -- all enqueued, none
    // waited for, so the members compute concurrently.  phase 2: wait for the member's download, copy its slice to the caller's buffer.
    auto submit = [&](int i, int off, int cnt) -> int {
        vp_ctx* c = g->h[i];
        int rc = submit_impl(c, (const char*)crops + (size_t)off * crop_bytes(fmt), fmt, cnt, org_wh ? org_wh + 2 * (size_t)off : nullptr,
                             out + (size_t)off * K * 3, &slot[i], true);
        if (rc) { g->err = c->err; slot[i] = -1; return rc; }
        if (d_all) {   // all-gather on the device side: this shard's keypoints to every device's copy, peer to peer, on the owner's stream
            for (int j = 0; j < w; ++j) {
                hipError_t e = hipMemcpyPeerAsync(d_all[j] + (size_t)off * K * 3, g->h[j]->cfg.device_id, c->slots[slot[i]].kp,
                                                  c->cfg.device_id, (size_t)cnt * K * 12, c->stream);
                if (e != hipSuccess) {
                    g->err = std::string("hipMemcpyPeerAsync: ") + hipGetErrorString(e);
                    vp_infer_wait(c, slot[i]); slot[i] = -1;   // this member is not marked in flight yet: collect it here
                    return VP_ERR_HIP;
                }
            }
        }
        return VP_OK;
    };
    auto wait = [&](int i) -> int {
        int rc = vp_infer_wait(g->h[i], slot[i]);
        slot[i] = -1;
        if (!rc && d_all) rc = vp_synchronize(g->h[i]);
        if (rc) g->err = g->h[i]->err;
        return rc;
    };
    return group_rounds(offs, cnts, w, submit, wait);
}

int vp_group_infer(vp_group_handle g, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out) {
    if (!out && n > 0) return VP_ERR_INVALID;
    return group_run(g, crops, fmt, n, org_wh, out, nullptr);
}

int vp_group_infer_allgather(vp_group_handle g, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* const* d_all, float* out) {
    if (!g || !d_all) return VP_ERR_INVALID;
    return group_run(g, crops, fmt, n, org_wh, out, d_all);
}

vp_handle vp_group_member(vp_group_handle g, int32_t i) { return (g && i >= 0 && i < (int)g->h.size()) ? g->h[i] : nullptr; }

int vp_group_set_flip_test(vp_group_handle g, const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap) {
    if (!g) return VP_ERR_INVALID;
    for (auto* h : g->h) {
        const int rc = vp_set_flip_test(h, flip_pairs, n_pairs, shift_heatmap);
        if (rc) { g->err = h->err; for (auto* q : g->h) vp_clear_flip_test(q); return rc; }   // all or none
    }
    return VP_OK;
}

int vp_group_clear_flip_test(vp_group_handle g) {
    if (!g) return VP_ERR_INVALID;
    for (auto* h : g->h) {
        const int rc = vp_clear_flip_test(h);
        if (rc) { g->err = h->err; return rc; }
    }
    return VP_OK;
}

int vp_group_destroy(vp_group_handle g) {
    if (!g) return VP_OK;
    for (auto* h : g->h) vp_destroy(h);
    delete g;
    return VP_OK;
}

const char* vp_group_last_error(vp_group_handle g) { return g ? g->err.c_str() : g_group_error.c_str(); }

void* vp_stream(vp_handle c) { return c ? (void*)c->stream : nullptr; }

int vp_synchronize(vp_handle c) {
    if (!c) return VP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if (c->foreign_pending && c->ev_sw) HIPCHK(c, hipEventSynchronize(c->ev_sw));   // the last call ran on a caller's stream
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

int vp_set_profiling(vp_handle c, int32_t enable) {
    if (!c) return VP_ERR_INVALID;
    c->prof = (uint32_t)enable;   // bitmask over VP_PROF_* families (-1 = all)
    return VP_OK;
}

int vp_reset_profile(vp_handle c) {
    if (!c) return VP_ERR_INVALID;
    if (c->foreign_pending && c->ev_sw) hipEventSynchronize(c->ev_sw);   // a small stream-ordered call recorded its timing events on the CALLER's stream
    hipStreamSynchronize(c->stream);
    prof_collect(c);
    std::memset(&c->acc, 0, sizeof(c->acc));
    return VP_OK;
}

int vp_get_profile(vp_handle c, vp_profile* out) {
    if (!c || !out) return VP_ERR_INVALID;
    if (c->foreign_pending && c->ev_sw) HIPCHK(c, hipEventSynchronize(c->ev_sw));   // as vp_synchronize: the last call may have run (and been timed) on a caller's stream
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    *out = c->acc;
    return VP_OK;
}

int vp_profile_kernel(vp_handle c, int32_t family, char* buf, int32_t cap) {
    if (!c || family < 0 || family >= VP_PROF_COUNT || !buf || cap <= 0) return VP_ERR_INVALID;
    snprintf(buf, (size_t)cap, "%s", c->kernel_desc[family].c_str());
    return VP_OK;
}

int vp_destroy(vp_handle c) {
    if (!c) return VP_OK;
    hipSetDevice(c->cfg.device_id);
    if (c->foreign_pending && c->ev_sw) hipEventSynchronize(c->ev_sw);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto& e : c->evs) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    for (auto& p : c->ev_pool) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    for (auto& sl : c->slots) { if (sl.h2d) hipEventDestroy(sl.h2d); if (sl.done) hipEventDestroy(sl.done); if (sl.out) hipEventDestroy(sl.out); if (sl.host_kp) hipHostFree(sl.host_kp); if (sl.host_in) hipHostFree(sl.host_in); }
    if (c->ev_in) hipEventDestroy(c->ev_in);
    if (c->ev_out) hipEventDestroy(c->ev_out);
    if (c->ev_sw) hipEventDestroy(c->ev_sw);
    for (auto& ge : c->graphs) if (ge.exec) hipGraphExecDestroy(ge.exec);
    for (void* p : c->allocs) hipFree(p);
    if (c->copy_stream) { hipStreamSynchronize(c->copy_stream); hipStreamDestroy(c->copy_stream); }
    if (c->d2h_stream) { hipStreamSynchronize(c->d2h_stream); hipStreamDestroy(c->d2h_stream); }
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return VP_OK;
}

const char* vp_last_error(vp_handle c) { return c ? c->err.c_str() : g_create_error.c_str(); }

}  // extern "C"
