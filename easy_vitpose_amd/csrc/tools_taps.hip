// vp_dbg_*: the timing taps and probes of the measurement library (libvitpose_hip_tools.so, include/vitpose_hip_tools.h); tools/ load them.
// Compiled into the tools library only (easy_vitpose_amd/build.py TOOLS_SOURCES); the parity taps the tests use are debug_taps.hip.
#include "dbg_util.h"

using namespace vpi;

namespace {
// a GEMM launch on RANDOM device operands in any production configuration: epi = kernels.h GemmEpi 0, 1 (optionally with the
// LayerNorm-consumer fold), 2, 3, 6; flags: 1 persist, 2 out_blocked, 4 a_blocked, 8 reverse, 16 LayerNorm-consumer fold
struct RandCase {
    vp::GemmArgs g{};
    size_t out_bytes = 0, stats_floats = 0;
    void* out[2] = {nullptr, nullptr};
    float* stats[2] = {nullptr, nullptr};
};
int make_rand_case(vp_ctx* c, RandCase& rc, int epi, int flags, int M, int N, int K, int nout) {
    uint16_t *dA, *dW, *dAux16 = nullptr;
    float *dB, *dAux32 = nullptr, *dRow = nullptr, *dS = nullptr;
    int r;
    const size_t MN = (size_t)M * N, wrows = pad128(N);
    if ((r = dalloc(c, &dA, (size_t)M * K)) || (r = dalloc(c, &dW, wrows * K)) || (r = dalloc(c, &c->zero, (size_t)256))) return r;
    vp::fill_random16(c->dtype, dA, (size_t)M * K, 1u, nullptr);
    vp::fill_random16(c->dtype, dW, wrows * K, 2u, nullptr);
    // flags 64 / 128 (tools/clock_power_probe.py, VP_PROBE_SET=operand_bits): the SAME instruction stream on all-zero operands / on operands that are all the
    // constant 0x3c00 (1.0 in fp16) -- how much of a launch's time is the board power limit (the chip clocks by the energy its operand bits toggle)
    if (flags & 64) { HIPCHK(c, hipMemset(dA, 0, (size_t)M * K * 2)); HIPCHK(c, hipMemset(dW, 0, wrows * K * 2)); }
    if (flags & 128) { HIPCHK(c, hipMemsetD16(dA, 0x3c00, (size_t)M * K)); HIPCHK(c, hipMemsetD16(dW, 0x3c00, wrows * K)); }
    std::vector<float> hb(wrows), hs(wrows), hr((size_t)M * 2);
    uint32_t lcg = 12345u;
    auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)((lcg >> 8) & 0xffff) / 65536.f - 0.5f; };
    for (auto& v : hb) v = rnd();
    for (auto& v : hs) v = 4.f * rnd();
    for (size_t i = 0; i < (size_t)M; ++i) { hr[2 * i] = 0.2f * rnd(); hr[2 * i + 1] = 1.f + 0.4f * rnd(); }
    if ((r = upload_f32(c, &dB, hb.data(), wrows))) return r;
    vp::GemmArgs& g = rc.g;
    g.A = dA; g.W = dW; g.bias = dB; g.M = M; g.N = N; g.K = K; g.ldo = N; g.zero = c->zero; g.Kp = c->Kp;
    g.w_rows = (int)wrows;
    g.persist = (flags & 1) != 0; g.out_blocked = (flags & 2) != 0; g.a_blocked = (flags & 4) != 0; g.reverse = (flags & 8) != 0;
    if (flags & 16) {
        if ((r = upload_f32(c, &dRow, hr.data(), (size_t)M * 2)) || (r = upload_f32(c, &dS, hs.data(), wrows))) return r;
        g.rowstat = dRow; g.ln_s = dS;
    }
    if (epi == vp::EPI_BIAS || epi == vp::EPI_BIAS_GELU) {
        rc.out_bytes = MN * 2;
    } else if (epi == vp::EPI_BIAS_RESID || epi == vp::EPI_POS) {
        rc.out_bytes = MN * 4;
        const size_t na = epi == vp::EPI_BIAS_RESID ? MN : (size_t)192 * N;
        if ((r = dalloc(c, &dAux32, na))) return r;
        std::vector<float> ha(na);
        for (auto& v : ha) v = 2.f * rnd();
        HIPCHK(c, hipMemcpy(dAux32, ha.data(), na * 4, hipMemcpyHostToDevice));
        g.aux = dAux32;
    } else if (epi == vp::EPI_BIAS_RESID_LN) {
        rc.out_bytes = MN * 4;   // hi plane + lo plane
        rc.stats_floats = (size_t)M * (N / 64) * 2;
        if ((r = dalloc(c, &dAux16, 2 * MN))) return r;
        vp::fill_random16(c->dtype, dAux16, MN, 3u, nullptr);
        vp::fill_random16(c->dtype, dAux16 + MN, MN, 4u, nullptr);
        g.aux = (const float*)dAux16;
        g.plane = MN;
    } else {
        return fail(c, VP_ERR_INVALID, "unsupported epilogue for the random GEMM case");
    }
    for (int i = 0; i < nout; ++i) {
        char* o;
        if ((r = dalloc(c, &o, rc.out_bytes))) return r;
        HIPCHK(c, hipMemset(o, 0xff, rc.out_bytes));
        rc.out[i] = o;
        if (rc.stats_floats) {
            if ((r = dalloc(c, &rc.stats[i], rc.stats_floats))) return r;
            HIPCHK(c, hipMemset(rc.stats[i], 0xff, rc.stats_floats * 4));
        }
    }
    HIPCHK(c, hipDeviceSynchronize());
    return VP_OK;
}
}  // namespace

extern "C" {

// tools/qkvattn_phases.py: average milliseconds of the fused qkv + attention kernel on random operands, optionally with phases compiled out
VP_API int vp_dbg_qkvattn_bench(int32_t device, int32_t npairs, int32_t D, int32_t heads, int32_t iters, int32_t ablate, float* ms_out) {
    vp_ctx* c = dbg_ctx(device, VP_DTYPE_F16);
    if (!c) return VP_ERR_HIP;
    const size_t M = (size_t)npairs * 384;
    uint16_t *dx, *dwh, *dy;
    float *dbh, *dsh, *drow;
    int rc;
    if ((rc = dalloc(c, &dx, M * D)) || (rc = dalloc(c, &dwh, 3 * (size_t)D * D)) || (rc = dalloc(c, &dy, M * D)) || (rc = dalloc(c, &dbh, 3 * (size_t)D)) ||
        (rc = dalloc(c, &dsh, 3 * (size_t)D)) || (rc = dalloc(c, &drow, 2 * M)))
        return dbg_finish(c, rc);
    vp::fill_random16(c->dtype, dx, M * D, 1u, nullptr);
    vp::fill_random16(c->dtype, dwh, 3 * (size_t)D * D, 2u, nullptr);
    hipMemset(dbh, 0, 3 * (size_t)D * 4); hipMemset(dsh, 0, 3 * (size_t)D * 4); hipMemset(drow, 0, 2 * M * 4);
    vp::QkvAttnArgs qa{};
    qa.x_hi = dx; qa.wh = dwh; qa.bh = dbh; qa.sh = dsh; qa.rowstat = drow; qa.y = dy; qa.npairs = npairs; qa.ncrops = 2 * npairs; qa.heads = heads; qa.D = D; qa.ablate = ablate;
    qa.scale_log2e = vp::softmax_scale_log2e(64);
    vp::GemmArgs g80{};   // head dim 80: gemm8.hip EPI_QKV_ATTN (heads * 256 head-major rows: the 3 D^2 buffer is larger than heads * 256 * D)
    const bool h80 = heads * 80 == D;
    g80.A = dx; g80.W = dwh; g80.bias = dbh; g80.ln_s = dsh; g80.rowstat = drow; g80.out = dy;
    g80.M = (int)M; g80.N = heads * 256; g80.K = D; g80.ldo = D; g80.w_rows = heads * 256; g80.variant = 18; g80.ablate = ablate;
    g80.attn_scale_log2e = vp::softmax_scale_log2e(80);
    auto launch = [&]() { return h80 ? vp::gemm_launch(c->dtype, vp::EPI_QKV_ATTN, g80, nullptr) : vp::qkvattn_launch(c->dtype, qa, nullptr, nullptr, 0); };
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = launch();
    hipDeviceSynchronize();
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch();
    hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("qkvattn bench: ") + hipGetErrorString(e)));
    return dbg_finish(c, VP_OK);
}

// tools/gemm_timeline.py: one persistent launch of the qkv / fc1 shape with per-tile phase stamps (shader cycles) of wave 0 of
// every workgroup: stamps[wg][tile][8] = (main loop start, main loop end, epilogue end, 5 stamps inside k-step 5: top, after the
// barrier, after the global_load_lds issues, after the first MFMA block, end), up to 32 tiles per workgroup.
VP_API int vp_dbg_gemm_timeline(int32_t device, int32_t dtype, int32_t epi, int32_t M, int32_t N, int32_t K, uint64_t* stamps,
                                int32_t max_wg) {
    if ((epi != 0 && epi != 1) || !stamps) return fail(nullptr, VP_ERR_INVALID, "bad timeline request");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    uint16_t *dA, *dW, *dO;
    float* dB;
    unsigned long long* dS;
    int rc;
    const size_t wrows = pad128(N), nst = (size_t)max_wg * 32 * 8;
    if ((rc = dalloc(c, &dA, (size_t)M * K)) || (rc = dalloc(c, &dW, wrows * K)) || (rc = dalloc(c, &dB, wrows)) ||
        (rc = dalloc(c, &dO, (size_t)M * N)) || (rc = dalloc(c, &dS, nst)) || (rc = dalloc(c, &c->zero, (size_t)256)))
        return dbg_finish(c, rc);
    vp::fill_random16(c->dtype, dA, (size_t)M * K, 1u, nullptr);
    vp::fill_random16(c->dtype, dW, wrows * K, 2u, nullptr);
    hipMemset(dB, 0, wrows * 4);
    hipMemset(dS, 0, nst * 8);
    vp::GemmArgs g{};
    g.A = dA; g.W = dW; g.bias = dB; g.out = dO; g.M = M; g.N = N; g.K = K; g.ldo = N; g.zero = c->zero;
    g.w_rows = (int)wrows; g.variant = 8; g.group_m = 8; g.persist = 1;
    hipError_t e = vp::gemm_launch(c->dtype, epi, g, nullptr);          // warm
    g.ablate = 32 | (getenv("VP_TL_ABL") ? atoi(getenv("VP_TL_ABL")) : 0); g.stats_out = (float*)dS;
    if (e == hipSuccess) e = vp::gemm_launch(c->dtype, epi, g, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(stamps, dS, nst * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("timeline: ") + hipGetErrorString(e)));
    return dbg_finish(c, VP_OK);
}

// Time `iters` launches of one GEMM configuration on random device operands (HIP events).
// epi as in vp_dbg_gemm (0..3); returns average milliseconds per launch in *ms_out.
VP_API int vp_dbg_gemm_bench(int32_t device, int32_t dtype, int32_t epi, int32_t variant, int32_t group_m, int32_t M,
                             int32_t N, int32_t K, int32_t iters, float* ms_out) {
    if (epi < 0 || epi > 3 || M <= 0 || N <= 0 || K <= 0 || K % 64 || iters <= 0 || !ms_out)
        return fail(nullptr, VP_ERR_INVALID, "bad gemm bench shape");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    uint16_t *dA, *dW, *dO16 = nullptr;
    float *dB, *dAux = nullptr, *dO32 = nullptr;
    int rc;
    const size_t MN = (size_t)M * N, wrows = pad128(N);
    if ((rc = dalloc(c, &dA, (size_t)M * K)) || (rc = dalloc(c, &dW, wrows * K)) || (rc = dalloc(c, &dB, wrows)) ||
        (rc = dalloc(c, &c->zero, (size_t)256)))
        return dbg_finish(c, rc);
    if (epi >= 2) { if ((rc = dalloc(c, &dO32, MN)) || (rc = dalloc(c, &dAux, (size_t)192 * N))) return dbg_finish(c, rc); }
    else if ((rc = dalloc(c, &dO16, MN))) return dbg_finish(c, rc);
    vp::fill_random16(c->dtype, dA, (size_t)M * K, 1u, nullptr);
    vp::fill_random16(c->dtype, dW, wrows * K, 2u, nullptr);
    hipMemset(dB, 0, wrows * 4);
    if (dO32) hipMemset(dO32, 0, MN * 4);
    if (dAux) hipMemset(dAux, 0, (size_t)192 * N * 4);
    c->sw.gemm_variant[0] = variant & 0xff;
    c->sw.gemm_group_m[0] = group_m;
    c->gemm_ablate = variant >> 8;   // tools only: ablation flags in the high bits
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    void* outp = epi >= 2 ? (void*)dO32 : (void*)dO16;
    const float* aux = epi == 2 ? dO32 : dAux;
    const GemmPick pk = resolve_gemm(c->sw, 0, epi, M, N, K);
    for (int i = 0; i < 2 && !rc; ++i) rc = gemm(c, 0, epi, pk, dA, dW, dB, outp, aux, M, N, K, N);
    hipDeviceSynchronize();
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters && !rc; ++i) rc = gemm(c, 0, epi, pk, dA, dW, dB, outp, aux, M, N, K, N);
    hipEventRecord(e1, nullptr);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(c, VP_ERR_HIP, "gemm bench kernel failed");
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return dbg_finish(c, rc);
}

// average milliseconds per launch of one production GEMM configuration on random operands
VP_API int vp_dbg_gemm_bench2(int32_t device, int32_t dtype, int32_t epi, int32_t variant, int32_t group_m, int32_t flags, int32_t M,
                              int32_t N, int32_t K, int32_t iters, float* ms_out) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 64 || iters <= 0 || !ms_out) return fail(nullptr, VP_ERR_INVALID, "bad gemm bench shape");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    RandCase rc;
    int r = make_rand_case(c, rc, epi, flags, M, N, K, 1);
    if (r) return dbg_finish(c, r);
    vp::GemmArgs g = rc.g;
    g.variant = variant & 0xff; g.group_m = group_m; g.ablate = variant >> 8;
    g.out = rc.out[0]; g.stats_out = rc.stats[0];
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = vp::gemm_launch(c->dtype, epi, g, nullptr);
    hipDeviceSynchronize();
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = vp::gemm_launch(c->dtype, epi, g, nullptr);
    hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("gemm bench2: ") + hipGetErrorString(e)));
    return dbg_finish(c, VP_OK);
}

// tools/gemm8_timeline.py: one gemm8 launch (variant 16 / 17, epi 0 / 1) with cycle stamps of waves 0 and 4 of every workgroup:
// stamps[wg][group][tile < 16][8] = (main loop begin, main loop end, epilogue end, P4 wait of K-tile 0 begin / end, of K-tile 1 begin / end, 0)
VP_API int vp_dbg_gemm8_timeline(int32_t device, int32_t dtype, int32_t epi, int32_t variant, int32_t flags, int32_t ablate, int32_t M,
                                 int32_t N, int32_t K, uint64_t* stamps, int32_t max_wg) {
    if ((epi != 0 && epi != 1 && epi != vp::EPI_BIAS_RESID_LN) || !stamps || max_wg < 256) return fail(nullptr, VP_ERR_INVALID, "bad timeline request");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    RandCase rc;
    int r = make_rand_case(c, rc, epi, flags, M, N, K, 1);
    if (r) return dbg_finish(c, r);
    unsigned long long* dS;
    const size_t nst = (size_t)max_wg * 2 * 16 * 8;
    if ((r = dalloc(c, &dS, nst))) return dbg_finish(c, r);
    hipMemset(dS, 0, nst * 8);
    vp::GemmArgs g = rc.g;
    g.variant = variant; g.group_m = 8; g.out = rc.out[0];
    if (epi == vp::EPI_BIAS_RESID_LN) g.stats_out = rc.stats[0];
    hipError_t e = vp::gemm_launch(c->dtype, epi, g, nullptr);   // warm
    g.ablate = 32 | ablate;
    if (epi == vp::EPI_BIAS_RESID_LN) { g.stats_out = rc.stats[0]; g.ln_part = (const float*)dS; }   // the residual GEMM writes real statistics: stamps go to the unused ln_part
    else g.stats_out = (float*)dS;
    if (e == hipSuccess) e = vp::gemm_launch(c->dtype, epi, g, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(stamps, dS, nst * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("gemm8 timeline: ") + hipGetErrorString(e)));
    return dbg_finish(c, VP_OK);
}

// run two configurations of the same GEMM on the same random operands `reps` times each and compare every output byte
// (and the row statistics): the race / schedule screen for kernels whose arithmetic order is identical by construction
VP_API int vp_dbg_gemm_compare(int32_t device, int32_t dtype, int32_t epi, int32_t variant_a, int32_t group_a, int32_t flags_a,
                               int32_t variant_b, int32_t group_b, int32_t flags_b, int32_t M, int32_t N, int32_t K, int32_t reps,
                               uint64_t* n_mismatch, double* max_abs_diff) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 64 || reps <= 0 || !n_mismatch || !max_abs_diff) return fail(nullptr, VP_ERR_INVALID, "bad gemm compare shape");
    if ((flags_a & (2 | 4 | 16)) != (flags_b & (2 | 4 | 16))) return fail(nullptr, VP_ERR_INVALID, "layout / fold flags must agree");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    RandCase rc;
    int r = make_rand_case(c, rc, epi, flags_a, M, N, K, 2);
    if (r) return dbg_finish(c, r);
    *n_mismatch = 0; *max_abs_diff = 0.0;
    std::vector<uint16_t> ha(rc.out_bytes / 2), hb2(rc.out_bytes / 2);
    std::vector<float> sa(rc.stats_floats), sb(rc.stats_floats);
    for (int rep = 0; rep < reps; ++rep) {
        for (int w = 0; w < 2; ++w) {
            vp::GemmArgs g = rc.g;
            const int fl = w ? flags_b : flags_a;
            g.variant = w ? variant_b : variant_a; g.group_m = w ? group_b : group_a;
            g.persist = (fl & 1) != 0; g.reverse = (fl & 8) != 0;
            g.out = rc.out[w]; g.stats_out = rc.stats[w];
            hipMemsetAsync(rc.out[w], 0xff, rc.out_bytes, nullptr);
            hipError_t e = vp::gemm_launch(c->dtype, epi, g, nullptr);
            if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("gemm compare launch ") + (w ? "B: " : "A: ") + hipGetErrorString(e)));
        }
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(ha.data(), rc.out[0], rc.out_bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(hb2.data(), rc.out[1], rc.out_bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess && rc.stats_floats) e = hipMemcpy(sa.data(), rc.stats[0], rc.stats_floats * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && rc.stats_floats) e = hipMemcpy(sb.data(), rc.stats[1], rc.stats_floats * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("gemm compare: ") + hipGetErrorString(e)));
        const bool f32out = (epi == vp::EPI_BIAS_RESID || epi == vp::EPI_POS);
        if (f32out) {
            const float* fa = (const float*)ha.data(); const float* fb = (const float*)hb2.data();
            for (size_t i = 0; i < rc.out_bytes / 4; ++i)
                if (std::memcmp(&fa[i], &fb[i], 4)) { ++*n_mismatch; const double d = std::fabs((double)fa[i] - (double)fb[i]); if (!(d <= *max_abs_diff)) *max_abs_diff = d; }
        } else {
            for (size_t i = 0; i < ha.size(); ++i)
                if (ha[i] != hb2[i]) {
                    ++*n_mismatch;
                    const double d = std::fabs((double)host_from_bits(ha[i], c->dtype) - (double)host_from_bits(hb2[i], c->dtype));
                    if (!(d <= *max_abs_diff)) *max_abs_diff = d;
                }
        }
        for (size_t i = 0; i < sa.size(); ++i)
            if (std::memcmp(&sa[i], &sb[i], 4)) { ++*n_mismatch; const double d = std::fabs((double)sa[i] - (double)sb[i]); if (!(d <= *max_abs_diff)) *max_abs_diff = d; }
    }
    return dbg_finish(c, VP_OK);
}

VP_API int vp_dbg_hwid_probe(int32_t device, int32_t blocks, int32_t threads, int32_t lds_bytes, int32_t spin, uint32_t* out) {
    if (!out || blocks <= 0 || blocks > 65536 || threads <= 0 || threads > 1024 || lds_bytes < 16 || lds_bytes > 160 * 1024 || spin < 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, VP_ERR_HIP, "no HIP device");
    uint32_t* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)blocks * 16) != hipSuccess) return fail(nullptr, VP_ERR_HIP, "hipMalloc");
    hipError_t e = vp::hwid_probe_launch(d, blocks, threads, lds_bytes, spin, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d, (size_t)blocks * 16, hipMemcpyDeviceToHost);
    hipFree(d);
    return e == hipSuccess ? VP_OK : fail(nullptr, VP_ERR_HIP, hipGetErrorString(e));
}

// Calibration: kind 0/1 = MFMA-only loop (16x16x32 / 32x32x16 f16) in TFLOP/s, 2 = float4 copy in TB/s (read+write); the other kinds: probes.hip peak_bench.
VP_API int vp_dbg_peak(int32_t device, int32_t kind, double* result) {
    const bool known = (kind >= 0 && kind <= 12) || (kind >= 100 && kind < 164) || (kind >= 170 && kind < 178) || (kind >= 200 && kind < 248) ||
                       (kind >= 300 && kind < 492) || (kind >= 500 && kind < 504);
    if (!result || !known) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, VP_ERR_HIP, "no HIP device");
    hipError_t e = vp::peak_bench(kind, result);
    return e == hipSuccess ? VP_OK : fail(nullptr, VP_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
