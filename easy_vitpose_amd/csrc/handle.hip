// The handle behind the C ABI (include/vitpose_hip.h): creation and destruction, the environment's switches, the guards every entry shares,
// the handle's modes (active expert, flip-test), profiling and synchronisation.  No CPU fallback anywhere: every compute entry point needs a
// HIP device and fails with VP_ERR_HIP otherwise.
#include "api_internal.h"
#include "hoststage.h"

using namespace vpi;

namespace vpi {

thread_local std::string g_create_error;

int fail(vp_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

int need_weights(vp_ctx* c) {
    if (!c) return VP_ERR_INVALID;
    return c->loaded ? (int)VP_OK : fail(c, VP_ERR_STATE, "weights not loaded: call vp_load_weights first");
}

bool slots_busy(const vp_ctx* c) { return c->slots[0].busy || c->slots[1].busy; }

int slots_idle(vp_ctx* c, const char* who) {
    return slots_busy(c) ? fail(c, VP_ERR_STATE, std::string(who) + " with a vp_infer_submit in flight: call vp_infer_wait first") : (int)VP_OK;
}

// the last call may have run (and been timed) on a caller's stream: ev_sw, recorded behind its launches, then the handle's own stream
int quiesce(vp_ctx* c) {
    if (c->foreign_pending && c->ev_sw) HIPCHK(c, hipEventSynchronize(c->ev_sw));
    if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP_OK;
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
    if (const char* t = getenv("VP_ABLATE_FAM")) {   // e.g. "2:8,1:8" = no output stores in the qkv and fc1 epilogues
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
    c->Mp = std::max<size_t>(up256(B * 192), 512);
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
    if ((rc = dalloc(c, (char**)&c->draw_ws, (size_t)VP_DRAW_MAX_RECORDS * 48))) return bail(rc);   // 16-byte keys + 32-byte bodies: the stream entry allocates nothing
    if ((rc = dalloc(c, (char**)&c->label_ws, (size_t)VP_LABEL_MAX_ROWS * 40))) return bail(rc);   // 40-byte tag records: vp_draw_labels_stream allocates nothing
    if ((rc = dalloc(c, (char**)&c->collect_ws, (size_t)(2 * VP_COLLECT_MAX_ROWS + VP_COLLECT_MAX_FRAMES) * 4))) return bail(rc);   // vp_collect_stream allocates nothing
    if (hipMemset(c->zero, 0, 512) != hipSuccess) { c->err = "hipMemset"; return bail(VP_ERR_HIP); }
    *out = c;
    return VP_OK;
}

// ---- pinned host memory for the asynchronous host path (vp_infer_submit) -------------------------------------------------------
void* vp_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void vp_host_free(void* p) { if (p) hipHostFree(p); }

// ---- flip-test mode ------------------------------------------------------------------------------------------------------
int vp_set_flip_test(vp_handle c, const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap) {
    int rc = need_weights(c);
    if (rc) return rc;
    std::vector<int32_t> partner((size_t)c->Kmax);
    std::string why;
    if (flip_partner_table(c->Kp, flip_pairs, n_pairs, partner.data(), &why)) return fail(c, VP_ERR_INVALID, "vp_set_flip_test: " + why);
    for (int k = c->Kp; k < c->Kmax; ++k) partner[k] = k;
    if (c->maxb < 2)
        return fail(c, VP_ERR_STATE, "vp_set_flip_test: a crop and its mirror image share the forward batch, which needs max_batch >= 2 (this handle has 1)");
    if ((rc = slots_idle(c, "vp_set_flip_test"))) return rc;
    if ((rc = vp_synchronize(c))) return rc;   // a previous table may still be read by enqueued work (also on a caller's stream)
    if (!c->flip_table && (rc = dalloc(c, &c->flip_table, (size_t)c->Kmax))) return rc;
    HIPCHK(c, hipMemcpy(c->flip_table, partner.data(), (size_t)c->Kmax * 4, hipMemcpyHostToDevice));   // synchronous: `partner` is a local
    c->flip_pairs.assign(flip_pairs, flip_pairs + 2 * (size_t)n_pairs);
    c->flip_shift = shift_heatmap ? 1 : 0;
    c->flip_on = true;
    c->flip_ex = false;                // (replaces the per-expert form)
    c->flip_gen = ++c->flip_counter;   // never the value of an earlier set: a graph captured under another table or shift is not replayed
    return VP_OK;
}

// one table per expert: everything is validated and every refusal returned before the handle changes
int vp_set_flip_test_experts(vp_handle c, const int32_t* flip_pairs, const int32_t* n_pairs, int32_t shift_heatmap) {
    int rc = need_weights(c);
    if (rc) return rc;
    if (!c->n_experts) return fail(c, VP_ERR_STATE, "vp_set_flip_test_experts: the handle holds a plain (single-dataset) checkpoint, not a ViTPose+ one (vp_set_flip_test is its mode)");
    if (!n_pairs) return fail(c, VP_ERR_INVALID, "vp_set_flip_test_experts: null n_pairs");
    const int E = c->n_experts;
    size_t total = 0;
    for (int e = 0; e < E; ++e) {
        if (n_pairs[e] < 0) return fail(c, VP_ERR_INVALID, "vp_set_flip_test_experts: expert " + std::to_string(e) + ": negative n_pairs");
        total += (size_t)n_pairs[e];
    }
    if (total > 0 && !flip_pairs) return fail(c, VP_ERR_INVALID, "vp_set_flip_test_experts: null flip_pairs with a positive pair count");
    std::vector<int32_t> tables((size_t)E * c->Kmax);
    size_t at = 0;
    for (int e = 0; e < E; ++e) {
        int32_t* row = tables.data() + (size_t)e * c->Kmax;
        std::string why;
        if (flip_partner_table(c->ex_heads[e].K, n_pairs[e] ? flip_pairs + 2 * at : nullptr, n_pairs[e], row, &why))
            return fail(c, VP_ERR_INVALID, "vp_set_flip_test_experts: expert " + std::to_string(e) + ": " + why);
        for (int k = c->ex_heads[e].K; k < c->Kmax; ++k) row[k] = k;
        at += (size_t)n_pairs[e];
    }
    if (c->maxb < 2)
        return fail(c, VP_ERR_STATE, "vp_set_flip_test_experts: a crop and its mirror image share the forward batch, which needs max_batch >= 2 (this handle has 1)");
    if ((rc = slots_idle(c, "vp_set_flip_test_experts"))) return rc;
    if ((rc = vp_synchronize(c))) return rc;   // a previous table may still be read by enqueued work (also on a caller's stream)
    if (!c->flip_tables && (rc = dalloc(c, &c->flip_tables, tables.size()))) return rc;
    if (!c->mix_recs_flip && (rc = dalloc(c, &c->mix_recs_flip, (size_t)((c->maxb + 3) / 4 * 4)))) return rc;
    HIPCHK(c, hipMemcpy(c->flip_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice));   // synchronous: `tables` is a local
    c->flip_pairs.assign(flip_pairs, flip_pairs + 2 * total);
    c->flip_pairs.insert(c->flip_pairs.end(), n_pairs, n_pairs + E);   // (the counts too: two handles' modes compare equal only with the same split)
    c->flip_shift = shift_heatmap ? 1 : 0;
    c->flip_on = true;
    c->flip_ex = true;
    c->flip_gen = ++c->flip_counter;
    return VP_OK;
}

int vp_clear_flip_test(vp_handle c) {
    if (!c) return VP_ERR_INVALID;
    if (int rc = slots_idle(c, "vp_clear_flip_test")) return rc;
    c->flip_on = false;
    c->flip_ex = false;
    c->flip_gen = 0;   // the graphs of the plain mode are valid again
    c->flip_pairs.clear();
    return VP_OK;
}

int vp_flip_test_enabled(vp_handle c) { return c && c->flip_on ? (c->flip_ex ? 2 : 1) : 0; }   // 2: one table per expert (vp_set_flip_test_experts)

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

// ---- ViTPose+ (expert) handles --------------------------------------------------------------------------------------------
int vp_expert_info(vp_handle c, int32_t* n_experts, int32_t* part_features, int32_t* k_per_expert) {
    if (int rc = need_weights(c)) return rc;
    if (n_experts) *n_experts = c->n_experts;
    if (part_features) *part_features = c->part_features;
    if (k_per_expert)
        for (int e = 0; e < c->n_experts && e < 8; ++e) k_per_expert[e] = c->ex_heads[e].K;
    return VP_OK;
}

int vp_set_expert(vp_handle c, int32_t e) {
    if (int rc = need_weights(c)) return rc;
    if (!c->n_experts) return fail(c, VP_ERR_STATE, "vp_set_expert: the handle holds a plain (single-dataset) checkpoint, not a ViTPose+ one");
    if (e < 0 || e >= c->n_experts) return fail(c, VP_ERR_INVALID, "expert id " + std::to_string(e) + " outside [0, " + std::to_string(c->n_experts) + ")");
    if (int rc = slots_idle(c, "vp_set_expert")) return rc;
    const int k_before = c->Kp;
    use_expert(c, e);
    if (c->flip_on && !c->flip_ex && c->Kp != k_before) {   // the pairs were validated against the previous head's joints and say nothing about this one's
        vp_clear_flip_test(c);
        return fail(c, VP_ERR_STATE, "vp_set_expert: expert " + std::to_string(e) + " is active, but its head has " + std::to_string(c->Kp) + " joints, not " +
                                         std::to_string(k_before) + ": the flip-test mode was cleared -- call vp_set_flip_test with this dataset's pairs");
    }
    return VP_OK;
}

void* vp_stream(vp_handle c) { return c ? (void*)c->stream : nullptr; }

int vp_synchronize(vp_handle c) {
    if (!c) return VP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    return quiesce(c);
}

int vp_set_profiling(vp_handle c, int32_t enable) {
    if (!c) return VP_ERR_INVALID;
    c->prof = (uint32_t)enable;   // bitmask over VP_PROF_* families (-1 = all)
    return VP_OK;
}

int vp_reset_profile(vp_handle c) {
    if (!c) return VP_ERR_INVALID;
    quiesce(c);   // a small stream-ordered call recorded its timing events on the CALLER's stream
    prof_collect(c);
    std::memset(&c->acc, 0, sizeof(c->acc));
    return VP_OK;
}

int vp_get_profile(vp_handle c, vp_profile* out) {
    if (!c || !out) return VP_ERR_INVALID;
    if (int rc = quiesce(c)) return rc;
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
    quiesce(c);
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
