// vp_dbg_*: parity taps (ONE kernel on host fp32 data, used by tests/).  The timing taps tools/ load live in tools_taps.hip (tools library only).
#include "dbg_util.h"

using namespace vpi;

// ---------------------------------------------------------------------------
// Debug / parity taps: run ONE kernel on host fp32 data (operands are rounded to
// `dtype` exactly as the production packer / producers do).  Used by tests/ only.
// ---------------------------------------------------------------------------

// the two-plane residual stream of a producer-row case, up: plane bits as given, or fp32 values split on the host as the producers split them
static int upload_planes(vp_ctx* c, uint16_t** dst, const float* aux, const uint16_t* r_hi, const uint16_t* r_lo, size_t MN) {
    if (!(r_hi && r_lo) && !aux) return fail(c, VP_ERR_INVALID, "aux required");
    std::vector<uint16_t> hp(2 * MN);
    if (r_hi && r_lo) {
        std::memcpy(hp.data(), r_hi, MN * 2);
        std::memcpy(hp.data() + MN, r_lo, MN * 2);
    } else
        for (size_t i = 0; i < MN; ++i) {
            const uint16_t hi = host_to_bits(aux[i], c->dtype);
            hp[i] = hi;
            hp[MN + i] = host_to_bits(aux[i] - host_from_bits(hi, c->dtype), c->dtype);
        }
    int r;
    if ((r = dalloc(c, dst, 2 * MN))) return r;
    if (hipMemcpy(*dst, hp.data(), hp.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return fail(c, VP_ERR_HIP, "H2D");
    return VP_OK;
}
// ... and down: the plane bits themselves (o_hi / o_lo), or hi + lo summed (out)
static int download_planes(vp_ctx* c, const uint16_t* planes, float* out, uint16_t* o_hi, uint16_t* o_lo, size_t MN) {
    if (o_hi && o_lo) {
        if (hipMemcpy(o_hi, planes, MN * 2, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(o_lo, planes + MN, MN * 2, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, VP_ERR_HIP, "D2H");
        return VP_OK;
    }
    std::vector<float> hi(MN), lo(MN);
    int r;
    if ((r = download16(c, planes, hi.data(), MN)) || (r = download16(c, planes + MN, lo.data(), MN))) return r;
    for (size_t i = 0; i < MN; ++i) out[i] = hi[i] + lo[i];
    return VP_OK;
}

// The residual stream of a producer-row case as plane BITS (vp_dbg_gemm_case_planes) instead of fp32 values split / summed here (vp_dbg_gemm_case)
struct PlaneIO {
    const uint16_t *r_hi, *r_lo;   // epi 6: the residual planes [M,N]
    uint16_t *o_hi, *o_lo;         // the output planes [M,N]
    bool in_place;                 // epi 6: out == aux, the kernel updates the residual planes themselves
};

extern "C" {

// out = epilogue(A[M,K] . W[N,K]^T): epi 0 bias->16bit, 1 bias+gelu->16bit, 2 bias+aux[M,N]->fp32, 3 aux[m%192]->fp32
VP_API int vp_dbg_gemm(int32_t device, int32_t dtype, int32_t epi, int32_t M, int32_t N, int32_t K, const float* A,
                       const float* W, const float* bias, const float* aux, float* out) {
    if (epi < 0 || epi > 3 || M <= 0 || N <= 0 || K <= 0 || K % 64) return fail(nullptr, VP_ERR_INVALID, "bad gemm test shape");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    uint16_t *dA, *dW, *dO16 = nullptr;
    float *dB, *dAux = nullptr, *dO32 = nullptr;
    int rc;
    const size_t MN = (size_t)M * N;
    if ((rc = upload_mat(c, &dA, A, M, K, M))) return dbg_finish(c, rc);
    if ((rc = upload_mat(c, &dW, W, N, K, pad128(N)))) return dbg_finish(c, rc);
    if ((rc = upload_f32(c, &dB, bias, N, pad128(N)))) return dbg_finish(c, rc);
    if (epi >= 2) {
        if ((rc = upload_f32(c, &dAux, aux, epi == 2 ? MN : (size_t)192 * N))) return dbg_finish(c, rc);
        if ((rc = dalloc(c, &dO32, MN))) return dbg_finish(c, rc);
    } else if ((rc = dalloc(c, &dO16, MN))) return dbg_finish(c, rc);
    if ((rc = dalloc(c, &c->zero, (size_t)256))) return dbg_finish(c, rc);
    rc = gemm(c, 0, epi, resolve_gemm(c->sw, 0, epi, M, N, K), dA, dW, dB, epi >= 2 ? (void*)dO32 : (void*)dO16, dAux, M, N, K, N);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(c, VP_ERR_HIP, "gemm kernel failed");
    if (!rc) {
        if (epi >= 2) { if (hipMemcpy(out, dO32, MN * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(c, VP_ERR_HIP, "D2H"); }
        else rc = download16(c, dO16, out, MN);
    }
    return dbg_finish(c, rc);
}

// qkv [B*192, 3*D] fp32 -> out [B*192, D] fp32 (attention core, vit.py:167-176)
VP_API int vp_dbg_attention(int32_t device, int32_t dtype, int32_t B, int32_t D, int32_t heads, const float* qkv, float* out) {
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    uint16_t *dq, *dout;
    int rc;
    const size_t M = (size_t)B * 192;
    if ((rc = upload_mat(c, &dq, qkv, M, 3 * (size_t)D, M))) return dbg_finish(c, rc);
    if ((rc = dalloc(c, &dout, M * D))) return dbg_finish(c, rc);
    const char* qs = getenv("VP_ATTN_QSPLIT");   // read per call (a parity test flips it inside one process); handles read it once, at vp_create
    hipError_t e = vp::attention_launch(c->dtype, dq, dout, B, D, heads, nullptr, (long)B * heads <= (qs ? atol(qs) : Switches{}.attn_qsplit));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("attention: ") + hipGetErrorString(e)));
    return dbg_finish(c, download16(c, dout, out, M * D));
}

// The attention core in every variant the launcher has (tests/test_gpu_attention.py): qkv [B*192, 3*D] fp32 (row-major, rounded to dtype) -> out [B*192, D] fp32.
// flags: 1 = query split (three workgroups per (crop, head)), 2 = qkv handed over in the 64 x 64-blocked layout [M/64][3D/64][64][64] (kernels.h GemmArgs::out_blocked:
// element (m, n) lives in block (m / 64, n / 64) at row m % 64, column n % 64), 4 = MXFP8 output: out = the de-blocked, de-quantised values, out_scales [M, D/32] =
// the E8M0 bytes.  The device output is filled with 0xFF bytes before the launch (NaN in fp16 / bf16 and in e4m3): an unwritten element shows.  Combinations
// attention_launch has no kernel for are VP_ERR_INVALID: blocked or MX off head dim 64, MX with bf16, MX with the query split.
VP_API int vp_dbg_attention_case(int32_t device, int32_t dtype, int32_t B, int32_t D, int32_t heads, int32_t flags, const float* qkv, float* out, uint8_t* out_scales) {
    if (B <= 0 || D <= 0 || heads <= 0 || D % heads || (flags & ~7) || !qkv || !out) return fail(nullptr, VP_ERR_INVALID, "bad attention case");
    if (dtype != VP_DTYPE_F16 && dtype != VP_DTYPE_BF16) return fail(nullptr, VP_ERR_INVALID, "attention case: dtype");
    const int hd = D / heads;
    const bool qsplit = flags & 1, blocked = flags & 2, mx = flags & 4;
    if (hd != 32 && hd != 64 && hd != 80) return fail(nullptr, VP_ERR_INVALID, "attention case: head dim");
    if ((blocked || mx) && hd != 64) return fail(nullptr, VP_ERR_INVALID, "attention case: blocked qkv and MXFP8 output are head dim 64 only");
    if (mx && (dtype != VP_DTYPE_F16 || qsplit || D % 128 || !out_scales)) return fail(nullptr, VP_ERR_INVALID, "attention case: MXFP8 output is fp16, unsplit");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    const size_t M = (size_t)B * 192, N3 = 3 * (size_t)D, MD = M * D;
    std::vector<uint16_t> hq(M * N3);
    for (size_t m = 0; m < M; ++m)
        for (size_t n = 0; n < N3; ++n) {
            const size_t dst = blocked ? ((m / 64) * (N3 / 64) + n / 64) * 4096 + (m % 64) * 64 + n % 64 : m * N3 + n;
            hq[dst] = host_to_bits(qkv[m * N3 + n], c->dtype);
        }
    uint16_t* dq;
    char* dout;
    uint8_t* dsc = nullptr;
    int rc;
    const size_t out_bytes = mx ? MD : MD * 2;
    if ((rc = dalloc(c, &dq, M * N3)) || (rc = dalloc(c, &dout, out_bytes)) || (mx && (rc = dalloc(c, &dsc, MD / 32)))) return dbg_finish(c, rc);
    hipError_t e = hipMemcpy(dq, hq.data(), hq.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xff, out_bytes);
    if (e == hipSuccess && mx) e = hipMemset(dsc, 0xff, MD / 32);
    if (e == hipSuccess) e = vp::attention_launch(c->dtype, dq, (uint16_t*)dout, B, D, heads, nullptr, qsplit, blocked, dsc);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("attention case: ") + hipGetErrorString(e)));
    if (!mx) return dbg_finish(c, download16(c, (const uint16_t*)dout, out, MD));
    std::vector<uint8_t> co(MD), so(MD / 32);
    if (hipMemcpy(co.data(), dout, MD, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(so.data(), dsc, MD / 32, hipMemcpyDeviceToHost) != hipSuccess)
        return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
    for (size_t m = 0; m < M; ++m)
        for (size_t n = 0; n < (size_t)D; ++n) {
            const uint8_t sb = so[vp::mx_scale_off(m, n >> 5, D)];
            out[m * D + n] = vp_host_e4m3_to_float(co[vp::mx_code_off(m, n, D)]) * std::ldexp(1.0f, (int)sb - 127);
            if (!(n & 31)) out_scales[m * (D / 32) + (n >> 5)] = sb;
        }
    return dbg_finish(c, VP_OK);
}

}  // extern "C"

// attn.qkv + attention core in one kernel (qkvattn.hip): x [2 npairs 192, D] (rounded to dtype), Wqkv [3D, D], bias [3D] -> out [M, D] (as fp32).
// Run with neutral LayerNorm statistics (mean 0, rstd 1, row sums 0: ln_fold(acc, 0, 0, 1, b) == acc + b exactly), so the result must equal
// vp_dbg_gemm(epi 0) followed by vp_dbg_attention bit for bit.
// the body of vp_dbg_qkvattn (rowstat == ln_s == NULL: the neutral statistics) and vp_dbg_qkvattn_ln (the caller's rowstat [M,2] and row sums ln_s [3D], through the same
// head-major repack as the bias)
static int qkvattn_case(int32_t device, int32_t dtype, int32_t npairs, int32_t D, int32_t heads, const float* x, const float* W, const float* bias, const float* rowstat,
                        const float* ln_s, float* out) {
    if (npairs <= 0 || D <= 0 || heads <= 0 || !x || !W || !bias || !out || !rowstat != !ln_s) return fail(nullptr, VP_ERR_INVALID, "bad qkvattn test shape");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    const size_t M = (size_t)npairs * 384;
    uint16_t *dx, *dw, *dwh, *dy;
    float *db, *dbh, *ds, *dsh, *drow;
    int rc;
    std::vector<float> zeros(3 * (size_t)D, 0.f), row(2 * M);
    for (size_t m = 0; m < M; ++m) { row[2 * m] = 0.f; row[2 * m + 1] = 1.f; }
    if ((rc = upload_mat(c, &dx, x, M, D, M)) || (rc = upload_mat(c, &dw, W, 3 * (size_t)D, D, pad128(3 * (size_t)D))) || (rc = upload_f32(c, &db, bias, 3 * (size_t)D)) ||
        (rc = upload_f32(c, &ds, ln_s ? ln_s : zeros.data(), 3 * (size_t)D)) || (rc = upload_f32(c, &drow, rowstat ? rowstat : row.data(), 2 * M)) || (rc = dalloc(c, &dwh, 3 * (size_t)D * D)) ||
        (rc = dalloc(c, &dbh, 3 * (size_t)D)) || (rc = dalloc(c, &dsh, 3 * (size_t)D)) || (rc = dalloc(c, &dy, M * D)))
        return dbg_finish(c, rc);
    if (heads * 80 == D) {   // head dim 80: gemm8.hip EPI_QKV_ATTN on the 192 x 256 tile (one crop x one head), head-major weights of heads * 256 rows
        uint16_t* dwh80; float *dbh80, *dsh80;
        const size_t rows = (size_t)heads * 256;
        if ((rc = dalloc(c, &dwh80, rows * D)) || (rc = dalloc(c, &dbh80, rows)) || (rc = dalloc(c, &dsh80, rows))) return dbg_finish(c, rc);
        hipError_t e8 = vp::qkv_head_major80_launch(dw, db, ds, dwh80, dbh80, dsh80, D, D, heads, nullptr);
        vp::GemmArgs g80{};
        g80.A = dx; g80.W = dwh80; g80.bias = dbh80; g80.ln_s = dsh80; g80.rowstat = drow; g80.out = dy;
        g80.M = (int)M; g80.N = heads * 256; g80.K = D; g80.ldo = D; g80.w_rows = heads * 256; g80.variant = 18;
        g80.attn_scale_log2e = vp::softmax_scale_log2e(80);
        if (e8 == hipSuccess && !vp::gemm8_supported(vp::EPI_QKV_ATTN, g80, 256, 192)) return dbg_finish(c, fail(c, VP_ERR_INVALID, "shape not supported by the fused qkv + attention tile (head dim 80)"));
        if (e8 == hipSuccess) e8 = vp::gemm_launch(c->dtype, vp::EPI_QKV_ATTN, g80, nullptr);
        if (e8 == hipSuccess) e8 = hipDeviceSynchronize();
        if (e8 != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("qkvattn (head dim 80): ") + hipGetErrorString(e8)));
        return dbg_finish(c, download16(c, dy, out, M * D));
    }
    hipError_t e = vp::qkv_head_major_launch(dw, db, ds, dwh, dbh, dsh, D, D, nullptr);
    vp::QkvAttnArgs qa{};
    qa.x_hi = dx; qa.wh = dwh; qa.bh = dbh; qa.sh = dsh; qa.rowstat = drow; qa.y = dy; qa.npairs = npairs; qa.ncrops = 2 * npairs; qa.heads = heads; qa.D = D;
    qa.scale_log2e = vp::softmax_scale_log2e(64);
    if (e == hipSuccess && !vp::qkvattn_supported(qa)) return dbg_finish(c, fail(c, VP_ERR_INVALID, "shape not supported by the fused qkv + attention kernel"));
    if (e == hipSuccess) e = vp::qkvattn_launch(c->dtype, qa, nullptr, nullptr, 0);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("qkvattn: ") + hipGetErrorString(e)));
    return dbg_finish(c, download16(c, dy, out, M * D));
}

extern "C" {

VP_API int vp_dbg_qkvattn(int32_t device, int32_t dtype, int32_t npairs, int32_t D, int32_t heads, const float* x, const float* W, const float* bias, float* out) {
    return qkvattn_case(device, dtype, npairs, D, heads, x, W, bias, nullptr, nullptr, out);
}

// vp_dbg_qkvattn with the caller's LayerNorm statistics (tests/test_gpu_ln_consumer.py): rowstat [M,2] = (mean, rstd) per row, ln_s [3D] = the row sums of W.  Must equal
// vp_dbg_gemm_case (epi 0, the same rowstat and ln_s) followed by vp_dbg_attention bit for bit.
VP_API int vp_dbg_qkvattn_ln(int32_t device, int32_t dtype, int32_t npairs, int32_t D, int32_t heads, const float* x, const float* W, const float* bias,
                             const float* rowstat, const float* ln_s, float* out) {
    if (!rowstat || !ln_s) return fail(nullptr, VP_ERR_INVALID, "bad qkvattn test shape");
    return qkvattn_case(device, dtype, npairs, D, heads, x, W, bias, rowstat, ln_s, out);
}

// ln_finalize_launch alone: partials [M, tiles, 2] = (sum, M2 about the granule mean) per 64-column granule -> rowstat [M, 2] = (mean, rstd) of rows of D columns
// (tiles = 6 / 12 / 16 / 20: ln_finalize_kernel_t; anything else: the generic ln_finalize_kernel)
VP_API int vp_dbg_ln_finalize(int32_t device, int32_t M, int32_t tiles, int32_t D, const float* partials, float* rowstat) {
    if (M <= 0 || tiles <= 0 || D <= 0 || !partials || !rowstat) return fail(nullptr, VP_ERR_INVALID, "bad ln_finalize case");
    vp_ctx* c = dbg_ctx(device, VP_DTYPE_F16);
    if (!c) return VP_ERR_HIP;
    float *dP, *dR;
    int rc;
    if ((rc = upload_f32(c, &dP, partials, (size_t)M * tiles * 2)) || (rc = dalloc(c, &dR, (size_t)M * 2))) return dbg_finish(c, rc);
    hipError_t e = hipMemset(dR, 0xff, (size_t)M * 8);
    if (e == hipSuccess) e = vp::ln_finalize_launch(dP, dR, M, tiles, D, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(rowstat, dR, (size_t)M * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, VP_ERR_HIP, std::string("ln_finalize: ") + hipGetErrorString(e));
    return dbg_finish(c, rc);
}

// ln_quant_launch alone (fp8 mode): x_hi [M, D] = the hi plane as 16-bit codes of `dtype`, partials [M, D / 64, 2] -> codes [Mp * D] (the blocked layout of csrc/mx8.h) and
// scales [Mp * D / 32] (the packed dwords).  Both outputs are filled with 0xFF bytes before the launch: the padding rows M .. Mp - 1 must come back written (zero).
VP_API int vp_dbg_ln_quant(int32_t device, int32_t dtype, int32_t M, int32_t Mp, int32_t D, const uint16_t* x_hi, const float* partials, uint8_t* codes, uint8_t* scales) {
    if (M <= 0 || Mp < M || Mp % 64 || D <= 0 || D % 128 || !x_hi || !partials || !codes || !scales || (dtype != VP_DTYPE_F16 && dtype != VP_DTYPE_BF16))
        return fail(nullptr, VP_ERR_INVALID, "bad ln_quant case");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    const size_t MD = (size_t)M * D, PD = (size_t)Mp * D;
    uint16_t* dX;
    float* dP;
    uint8_t *dC, *dS;
    int rc;
    if ((rc = dalloc(c, &dX, MD)) || (rc = upload_f32(c, &dP, partials, (size_t)M * (D / 64) * 2)) || (rc = dalloc(c, &dC, PD)) || (rc = dalloc(c, &dS, PD / 32)))
        return dbg_finish(c, rc);
    hipError_t e = hipMemcpy(dX, x_hi, MD * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dC, 0xff, PD);
    if (e == hipSuccess) e = hipMemset(dS, 0xff, PD / 32);
    if (e == hipSuccess) e = vp::ln_quant_launch(c->dtype, dX, dP, D / 64, dC, dS, M, Mp, D, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(codes, dC, PD, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(scales, dS, PD / 32, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, VP_ERR_HIP, std::string("ln_quant: ") + hipGetErrorString(e));
    return dbg_finish(c, rc);
}

// LayerNorm(eps 1e-6): x [M,D] fp32 -> out16 (as fp32) [M,D] and out32 [M,D]
VP_API int vp_dbg_layernorm(int32_t device, int32_t dtype, int32_t M, int32_t D, const float* x, const float* gamma,
                            const float* beta, float* out16, float* out32) {
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    float *dx, *dg, *db, *d32;
    uint16_t* d16;
    int rc;
    const size_t MD = (size_t)M * D;
    if ((rc = upload_f32(c, &dx, x, MD)) || (rc = upload_f32(c, &dg, gamma, D)) || (rc = upload_f32(c, &db, beta, D)) ||
        (rc = dalloc(c, &d32, MD)) || (rc = dalloc(c, &d16, MD))) return dbg_finish(c, rc);
    hipError_t e = vp::layernorm_launch(c->dtype, dx, dg, db, d16, d32, M, D, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out32, d32, MD * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("layernorm: ") + hipGetErrorString(e)));
    return dbg_finish(c, download16(c, d16, out16, MD));
}

// The last_norm launch of the default path (tests/test_gpu_final_ln.py): layernorm_kernel<Ty, PLANES = true> on the two-plane residual stream.  hi_bits / lo_bits
// [plane_rows, D] = the planes as 16-bit codes of `dtype`, uploaded as ONE buffer with plane = plane_rows * D between them (forward.hip lays the stream out for the
// encoder's padded row count and normalises the caller's M <= plane_rows rows).  out16 [plane_rows, D] = the stored codes as exact fp32, out32 [plane_rows, D] = the
// fp32 result; both device outputs are filled with 0xFF bytes before the launch: an unwritten row returns as NaN, a written row >= M shows.
VP_API int vp_dbg_layernorm_planes(int32_t device, int32_t dtype, int32_t M, int32_t plane_rows, int32_t D, const uint16_t* hi_bits, const uint16_t* lo_bits,
                                   const float* gamma, const float* beta, float* out16, float* out32) {
    if (M <= 0 || plane_rows < M || plane_rows > (1 << 20) || D <= 0 || (D & 3) || D > 1280 || !hi_bits || !lo_bits || !gamma || !beta || !out16 || !out32 ||
        (dtype != VP_DTYPE_F16 && dtype != VP_DTYPE_BF16))
        return fail(nullptr, VP_ERR_INVALID, "bad layernorm planes case");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    const size_t PD = (size_t)plane_rows * D;
    uint16_t *dx, *d16;
    float *dg, *db, *d32;
    int rc;
    if ((rc = upload_planes(c, &dx, nullptr, hi_bits, lo_bits, PD)) || (rc = upload_f32(c, &dg, gamma, D)) || (rc = upload_f32(c, &db, beta, D)) ||
        (rc = dalloc(c, &d32, PD)) || (rc = dalloc(c, &d16, PD)))
        return dbg_finish(c, rc);
    hipError_t e = hipMemset(d32, 0xff, PD * 4);
    if (e == hipSuccess) e = hipMemset(d16, 0xff, PD * 2);
    if (e == hipSuccess) e = vp::layernorm_launch(c->dtype, (const float*)dx, dg, db, d16, d32, M, D, nullptr, PD);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out32, d32, PD * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("layernorm planes: ") + hipGetErrorString(e)));
    return dbg_finish(c, download16(c, d16, out16, PD));
}

// The patch gather alone (tests/test_gpu_patch_gather.py): mode 0 = im2col_launch(flip = false), 1 = im2col_launch(flip = true), 2 = im2col_twin_launch.  crops = host
// fp32 [n_src,3,256,192] (VP_INPUT_F32_NCHW) or uint8 [n_src,256,192,3] (VP_INPUT_U8_NHWC); modes 0 / 1: B output crops from n_src <= B source crops (the last one
// repeated), mode 2: 2 n_src interleaved output crops (crop, mirror) + padding.  out_bits [B * 192 * 768] = the 16-bit codes exactly as the kernel stored them.  The device
// output is filled with 0xFF bytes before the launch and followed by 192 * 768 guard elements (one output crop), which come back as bytes in guard [2 * 192 * 768].
// What the launchers refuse (twin with 2 n_src > B, an unknown input format) comes back as an error, nothing is launched.
VP_API int vp_dbg_im2col(int32_t device, int32_t dtype, int32_t input_format, int32_t mode, int32_t B, int32_t n_src, const void* crops, uint16_t* out_bits,
                         uint8_t* guard) {
    if (mode < 0 || mode > 2 || B <= 0 || B > 4096 || n_src <= 0 || n_src > B || !crops || !out_bits || !guard || (dtype != VP_DTYPE_F16 && dtype != VP_DTYPE_BF16))
        return fail(nullptr, VP_ERR_INVALID, "bad im2col case");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    const size_t crop_bytes = input_format == VP_INPUT_F32_NCHW ? (size_t)3 * 256 * 192 * 4 : input_format == VP_INPUT_U8_NHWC ? (size_t)256 * 192 * 3 : 0;
    const size_t out_n = (size_t)B * 192 * 768, G = (size_t)192 * 768;
    char* din;
    uint16_t* dout;
    int rc;
    if ((rc = dalloc(c, &din, crop_bytes ? crop_bytes * n_src : (size_t)256)) || (rc = dalloc(c, &dout, out_n + G))) return dbg_finish(c, rc);
    hipError_t e = crop_bytes ? hipMemcpy(din, crops, crop_bytes * n_src, hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess) e = hipMemset(dout, 0xff, (out_n + G) * 2);
    if (e == hipSuccess)
        e = mode == 2 ? vp::im2col_twin_launch(c->dtype, din, input_format, dout, B, n_src, nullptr)
                      : vp::im2col_launch(c->dtype, din, input_format, dout, B, nullptr, mode == 1, n_src);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out_bits, dout, out_n * 2, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(guard, dout + out_n, G * 2, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, VP_ERR_HIP, std::string("im2col: ") + hipGetErrorString(e));
    return dbg_finish(c, rc);
}

// ConvTranspose2d(Cin,256,4,2,1,bias=False)+BN(eval)+ReLU on NHWC x [B,Hin,Win,Cin] fp32 -> NHWC [B,2Hin,2Win,256] fp32.
// tensors = {"keypoint_head.deconv_layers.0.weight", ".1.weight", ".1.bias", ".1.running_mean", ".1.running_var"}
VP_API int vp_dbg_deconv(int32_t device, int32_t dtype, int32_t B, int32_t Hin, int32_t Win, int32_t Cin, const float* x,
                         const vp_tensor_desc* tensors, int32_t n_tensors, float* out) {
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    Lookup lk;
    lk.c = c;
    for (int i = 0; i < n_tensors; ++i) lk.map[tensors[i].name] = &tensors[i];
    uint16_t *dx, *dw, *dout;
    float* db;
    int rc;
    const size_t Min = (size_t)B * Hin * Win;
    if ((rc = pack_deconv(c, lk, 0, Cin, &dw, &db))) return dbg_finish(c, rc);
    if ((rc = upload_mat(c, &dx, x, Min, Cin, Min))) return dbg_finish(c, rc);
    if ((rc = dalloc(c, &dout, Min * 4 * 256))) return dbg_finish(c, rc);
    if ((rc = dalloc(c, &c->zero, (size_t)256))) return dbg_finish(c, rc);
    if (hipMemset(c->zero, 0, 512) != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "memset"));
    rc = gemm(c, 0, vp::EPI_DECONV, resolve_gemm(c->sw, 0, vp::EPI_DECONV, (int)Min, 256, 4 * Cin), dx, dw, db, dout, nullptr, (int)Min, 256, 4 * Cin, 256, Hin, Win, Cin);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(c, VP_ERR_HIP, "deconv kernel failed");
    if (!rc) rc = download16(c, dout, out, Min * 4 * 256);
    return dbg_finish(c, rc);
}

// ONE GEMM of the keypoint head on a chosen tile (tests/test_gpu_head.py), launched through vp::gemm_launch with the arguments forward.hip's own gemm_args builds for it.
//   stage 0: EPI_DECONV                       x [B,Hin,Win,Cin] NHWC -> out = the 16-bit NHWC tensor [B,2Hin,2Win,256] (as fp32)
//   stage 1: EPI_DECONV_FINAL                 ... -> out = the fp32 heatmaps [B,Kp,2Hin,2Win] (deconv + folded BN + ReLU + the final 1x1 conv in one kernel)
//   stage 2: EPI_DECONV, then EPI_HEATMAP     the un-fused head on the same operands: mid = the 16-bit tensor, out = the heatmaps (EPI_HEATMAP's images are 64 x 48:
//                                             Hin x Win = 32 x 24, Cin = 256 only; its launch runs on the rule's tile)
// variant = the deconv's tile (a gemm.hip Cfg id), -1 = what resolve_gemm picks for the shape; parity_fast = Switches::deconv_parity_fast for this call.  tensors = the raw
// deconv + BN tensors as for vp_dbg_deconv (packed by pack_deconv); stages 1 / 2: w_fin [Kp,256], b_fin [Kp] (upload_final: hi + lo planes).  x is rounded to dtype on
// upload (a no-op on values that are already of that type).  Every device output is filled with 0xFF bytes first and has 16 * (4 Hin Win) more elements behind it, which come
// back as bytes in guard / mid_guard: an unwritten element returns as NaN, a write past the end shows in the guard.  What gemm_launch refuses comes back as its error.
VP_API int vp_dbg_head_case(int32_t device, int32_t dtype, int32_t stage, int32_t variant, int32_t parity_fast, int32_t B, int32_t Hin, int32_t Win, int32_t Cin,
                            const float* x, const vp_tensor_desc* tensors, int32_t n_tensors, int32_t Kp, const float* w_fin, const float* b_fin, float* out,
                            uint8_t* guard, float* mid, uint8_t* mid_guard) {
    if (stage < 0 || stage > 2 || (parity_fast & ~1) || B <= 0 || Hin <= 0 || Win <= 0 || Cin <= 0 || Cin % 64 || !x || !tensors || n_tensors <= 0 || !out || !guard ||
        (dtype != VP_DTYPE_F16 && dtype != VP_DTYPE_BF16) || (size_t)B * Hin * Win > ((size_t)1 << 20))
        return fail(nullptr, VP_ERR_INVALID, "bad head case");
    if (stage >= 1 && (Kp <= 0 || Kp > 4096 || !w_fin || !b_fin)) return fail(nullptr, VP_ERR_INVALID, "head case: the final conv's Kp, w_fin and b_fin required");
    if (stage == 2 && (Hin != 32 || Win != 24 || Cin != 256 || !mid || !mid_guard))
        return fail(nullptr, VP_ERR_INVALID, "head case: the un-fused head is deconv2's geometry (32 x 24 x 256) and returns the 16-bit tensor too");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    Lookup lk;
    lk.c = c;
    for (int i = 0; i < n_tensors; ++i) lk.map[tensors[i].name] = &tensors[i];
    const size_t Min = (size_t)B * Hin * Win, opix = (size_t)4 * Hin * Win, G = 16 * opix;
    const size_t act_n = Min * 4 * 256, hm_n = (size_t)B * (stage ? Kp : 0) * opix;
    uint16_t *dx, *dw;
    float* db;
    char *d_act = nullptr, *d_hm = nullptr;
    int rc;
    if ((rc = pack_deconv(c, lk, 0, Cin, &dw, &db)) || (rc = upload_mat(c, &dx, x, Min, Cin, Min)) || (rc = dalloc(c, &c->zero, (size_t)256))) return dbg_finish(c, rc);
    if (hipMemset(c->zero, 0, 512) != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "memset"));
    if (stage != 1 && ((rc = dalloc(c, &d_act, (act_n + G) * 2)) || hipMemset(d_act, 0xff, (act_n + G) * 2) != hipSuccess)) return dbg_finish(c, rc ? rc : fail(c, VP_ERR_HIP, "memset"));
    if (stage >= 1) {
        c->Kp = Kp;
        if ((rc = upload_final(c, &c->w_fin, w_fin, Kp, 256, &c->fin_rows)) || (rc = upload_f32(c, &c->b_fin, b_fin, Kp, pad128(Kp))) || (rc = dalloc(c, &d_hm, (hm_n + G) * 4)))
            return dbg_finish(c, rc);
        if (hipMemset(d_hm, 0xff, (hm_n + G) * 4) != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "memset"));
    }
    c->sw.deconv_parity_fast = parity_fast != 0;
    const int epi = stage == 1 ? vp::EPI_DECONV_FINAL : vp::EPI_DECONV;
    GemmPick pk = resolve_gemm(c->sw, VP_PROF_GEMM_DECONV, epi, (int)Min, 256, 4 * Cin);
    if (variant >= 0) { pk = GemmPick{}; pk.variant = variant; }
    const vp::GemmArgs g = gemm_args(c, VP_PROF_GEMM_DECONV, epi, pk, dx, dw, db, stage == 1 ? (void*)d_hm : (void*)d_act, nullptr, (int)Min, 256, 4 * Cin, 256, Hin, Win, Cin);
    hipError_t e = vp::gemm_launch(c->dtype, epi, g, nullptr);
    if (e == hipSuccess && stage == 2) {
        const int M2 = B * 3072, N2 = (int)c->fin_rows;
        const vp::GemmArgs h = gemm_args(c, VP_PROF_GEMM_FINAL, vp::EPI_HEATMAP, resolve_gemm(c->sw, VP_PROF_GEMM_FINAL, vp::EPI_HEATMAP, M2, N2, 256), (const uint16_t*)d_act,
                                         c->w_fin, c->b_fin, d_hm, nullptr, M2, N2, 256, 0);
        e = vp::gemm_launch(c->dtype, vp::EPI_HEATMAP, h, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("head case: ") + hipGetErrorString(e)));
    if (d_act) {
        if ((rc = download16(c, (const uint16_t*)d_act, stage == 0 ? out : mid, act_n))) return dbg_finish(c, rc);
        if (hipMemcpy(stage == 0 ? guard : mid_guard, d_act + act_n * 2, G * 2, hipMemcpyDeviceToHost) != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
    }
    if (d_hm && (hipMemcpy(out, d_hm, hm_n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(guard, d_hm + hm_n * 4, G * 4, hipMemcpyDeviceToHost) != hipSuccess))
        return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
    return dbg_finish(c, VP_OK);
}

// ---- production-configuration GEMM tap (tests/test_gpu_gemm_cfgs.py, tools/gemm8_check.py) ----

// ONE launch of any production GEMM configuration on HOST fp32 data (tests/test_gpu_gemm_cfgs.py): operands are rounded to
// `dtype` exactly as the packer / producing kernels round them, layouts (64x64-blocked A / output, two-plane residual stream,
// hi+lo final-conv weights) are built and undone here.
//   epi 0 / 1: out[M,N] 16-bit (returned as fp32); rowstat [M,2] + ln_s [N] non-NULL = LayerNorm-consumer fold
//   epi 2 / 3: out[M,N] fp32, aux = residual [M,N] / pos [192,N]
//   epi 6 / 7: aux = fp32 residual [M,N] (split into hi + lo planes on upload) / pos [192,N]; out = hi + lo planes summed;
//              stats [M, N/64, 2] = (sum, centred M2) per 64-column granule
//   epi 5:     W = final 1x1 conv weight [N = Kp, K = 256], A = [M = B 3072, 256]; out = heatmaps [B, Kp, 3072] fp32
// flags: 1 persistent, 2 out_blocked, 4 a_blocked, 8 reverse
// the body of vp_dbg_gemm_case and vp_dbg_gemm_case_planes (io != NULL: epi 6 / 7 on plane bits; aux = pos for epi 7)
static int gemm_case(int32_t device, int32_t dtype, int32_t epi, int32_t variant, int32_t group_m, int32_t flags, int32_t M, int32_t N, int32_t K, const float* A,
                     const float* W, const float* bias, const float* aux, const float* rowstat, const float* ln_s, float* out, float* stats, const PlaneIO* io,
                     const float* ln_part = nullptr, int ln_tiles = 0) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 64 || !A || !W || !bias) return fail(nullptr, VP_ERR_INVALID, "bad gemm case");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    c->Kp = N;
    int r;
    const size_t MN = (size_t)M * N, wrows = pad128(N);
    const bool ablk = (flags & 4) != 0, oblk = (flags & 2) != 0;
    uint16_t *dA, *dW;
    float *dB, *dAux32 = nullptr, *dRow = nullptr, *dS = nullptr, *dStats = nullptr;
    uint16_t* dAux16 = nullptr;
    void* dOut = nullptr;
    // A (optionally in the 64x64-blocked layout [M/64][K/64][64][64])
    {
        std::vector<uint16_t> ha((size_t)M * K);
        for (size_t m = 0; m < (size_t)M; ++m)
            for (size_t k = 0; k < (size_t)K; ++k) {
                const size_t dst = ablk ? ((((m >> 6) * (K >> 6) + (k >> 6)) << 12) + ((m & 63) << 6) + (k & 63)) : m * K + k;
                ha[dst] = host_to_bits(A[m * K + k], c->dtype);
            }
        if ((r = dalloc(c, &dA, (size_t)M * K))) return dbg_finish(c, r);
        if (hipMemcpy(dA, ha.data(), ha.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "H2D"));
    }
    size_t fin_rows = 0;
    if (epi == vp::EPI_HEATMAP) { if ((r = upload_final(c, &dW, W, N, K, &fin_rows))) return dbg_finish(c, r); }
    else if ((r = upload_mat(c, &dW, W, N, K, wrows))) return dbg_finish(c, r);
    if ((r = upload_f32(c, &dB, bias, N, wrows)) || (r = dalloc(c, &c->zero, (size_t)256))) return dbg_finish(c, r);
    vp::GemmArgs g{};
    g.A = dA; g.W = dW; g.bias = dB; g.M = M; g.N = N; g.K = K; g.ldo = N; g.zero = c->zero; g.Kp = N;
    g.w_rows = (int)wrows; g.variant = variant; g.group_m = group_m;
    g.persist = (flags & 1) != 0; g.out_blocked = oblk; g.a_blocked = ablk; g.reverse = (flags & 8) != 0;
    if (rowstat && ln_s) {
        if ((r = upload_f32(c, &dRow, rowstat, (size_t)M * 2)) || (r = upload_f32(c, &dS, ln_s, N, wrows))) return dbg_finish(c, r);
        g.rowstat = dRow; g.ln_s = dS;
    }
    if (ln_part) {   // the consumer merges the producer's partial statistics itself: set as forward.hip sets them
        float* dPart;
        if ((r = upload_f32(c, &dPart, ln_part, (size_t)M * ln_tiles * 2)) || (r = upload_f32(c, &dS, ln_s, N, wrows))) return dbg_finish(c, r);
        g.ln_part = dPart; g.ln_tiles = ln_tiles; g.ln_inv_d = 1.0f / (float)K; g.ln_s = dS;
    }
    size_t out_bytes = 0;
    const bool prod = epi == vp::EPI_BIAS_RESID_LN || epi == vp::EPI_POS_LN;
    if (epi == vp::EPI_BIAS || epi == vp::EPI_BIAS_GELU) out_bytes = MN * 2;
    else if (epi == vp::EPI_BIAS_RESID || epi == vp::EPI_POS || prod) out_bytes = MN * 4;
    else if (epi == vp::EPI_HEATMAP) { out_bytes = MN * 4; g.N = (int)fin_rows; g.ldo = 0; g.w_rows = (int)pad128(fin_rows); }
    else return dbg_finish(c, fail(c, VP_ERR_INVALID, "unsupported epilogue"));
    if (epi == vp::EPI_BIAS_RESID || epi == vp::EPI_POS || epi == vp::EPI_POS_LN) {
        if (!aux) return dbg_finish(c, fail(c, VP_ERR_INVALID, "aux required"));
        if ((r = upload_f32(c, &dAux32, aux, epi == vp::EPI_BIAS_RESID ? MN : (size_t)192 * N))) return dbg_finish(c, r);
        g.aux = dAux32;
    }
    if (epi == vp::EPI_BIAS_RESID_LN) {
        if ((r = upload_planes(c, &dAux16, aux, io ? io->r_hi : nullptr, io ? io->r_lo : nullptr, MN))) return dbg_finish(c, r);
        g.aux = (const float*)dAux16;
    }
    if (prod) {
        g.plane = MN;
        if ((r = dalloc(c, &dStats, (size_t)M * (N / 64) * 2))) return dbg_finish(c, r);
        g.stats_out = dStats;
    }
    if (io && io->in_place) dOut = dAux16;   // as forward.hip launches the residual GEMMs: out == aux
    else {
        char* o;
        if ((r = dalloc(c, &o, out_bytes))) return dbg_finish(c, r);
        dOut = o;
        hipMemset(dOut, 0xff, out_bytes);
    }
    g.out = dOut;
    const int splitk = (flags >> 8) & 15;   // epi 6 only: S partial products (EPI_PARTIAL) + splitk_reduce_kernel instead of the one-launch residual epilogue
    hipError_t e;
    if (splitk > 1) {
        if (epi != vp::EPI_BIAS_RESID_LN) return dbg_finish(c, fail(c, VP_ERR_INVALID, "split-K is a residual-GEMM path (epi 6)"));
        float* ws = nullptr;
        if ((r = dalloc(c, &ws, (size_t)splitk * MN))) return dbg_finish(c, r);
        hipMemset(ws, 0xff, (size_t)splitk * MN * 4);
        vp::GemmArgs p = g;
        p.out = ws; p.aux = nullptr; p.bias = nullptr; p.stats_out = nullptr; p.plane = 0; p.splitk = splitk; p.persist = 0;
        e = vp::gemm_launch(c->dtype, vp::EPI_PARTIAL, p, nullptr);
        if (e == hipSuccess) e = vp::splitk_reduce_launch(c->dtype, ws, splitk, dB, dAux16, MN, dStats, M, N, nullptr);
        dOut = dAux16;   // the reduction updates the residual planes in place
    } else {
        e = vp::gemm_launch(c->dtype, epi, g, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, std::string("gemm case: ") + hipGetErrorString(e)));
    if (epi == vp::EPI_BIAS || epi == vp::EPI_BIAS_GELU) {
        std::vector<float> t(MN);
        if ((r = download16(c, (const uint16_t*)dOut, t.data(), MN))) return dbg_finish(c, r);
        for (size_t m = 0; m < (size_t)M; ++m)
            for (size_t n = 0; n < (size_t)N; ++n) {
                const size_t src = oblk ? ((((m >> 6) * ((size_t)N >> 6) + (n >> 6)) << 12) + ((m & 63) << 6) + (n & 63)) : m * N + n;
                out[m * N + n] = t[src];
            }
    } else if (prod) {
        if ((r = download_planes(c, (const uint16_t*)dOut, out, io ? io->o_hi : nullptr, io ? io->o_lo : nullptr, MN))) return dbg_finish(c, r);
        if (stats && hipMemcpy(stats, dStats, (size_t)M * (N / 64) * 8, hipMemcpyDeviceToHost) != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
    } else {
        if (hipMemcpy(out, dOut, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
    }
    return dbg_finish(c, VP_OK);
}

VP_API int vp_dbg_gemm_case(int32_t device, int32_t dtype, int32_t epi, int32_t variant, int32_t group_m, int32_t flags, int32_t M,
                            int32_t N, int32_t K, const float* A, const float* W, const float* bias, const float* aux, const float* rowstat,
                            const float* ln_s, float* out, float* stats) {
    if (!out) return fail(nullptr, VP_ERR_INVALID, "bad gemm case");
    return gemm_case(device, dtype, epi, variant, group_m, flags, M, N, K, A, W, bias, aux, rowstat, ln_s, out, stats, nullptr);
}

// vp_dbg_gemm_case for a LayerNorm consumer that merges the partial statistics in its prologue (GemmArgs::ln_part, epi 0 / 1): partials [M, ln_tiles, 2] instead of
// rowstat, ln_inv_d = 1 / K as forward.hip sets it.  What gemm_launch refuses (an 8-phase tile, the persistent kernel, an odd ln_tiles) comes back as the error it is.
VP_API int vp_dbg_gemm_case_lnpart(int32_t device, int32_t dtype, int32_t epi, int32_t variant, int32_t group_m, int32_t flags, int32_t M, int32_t N, int32_t K,
                                   const float* A, const float* W, const float* bias, const float* partials, int32_t ln_tiles, const float* ln_s, float* out) {
    if ((epi != vp::EPI_BIAS && epi != vp::EPI_BIAS_GELU) || !partials || ln_tiles <= 0 || !ln_s || !out) return fail(nullptr, VP_ERR_INVALID, "bad gemm ln_part case");
    return gemm_case(device, dtype, epi, variant, group_m, flags, M, N, K, A, W, bias, nullptr, nullptr, ln_s, out, nullptr, nullptr, partials, ln_tiles);
}

// The producer row's own tap (tests/test_gpu_residual_row.py): vp_dbg_gemm_case for epi 6 / 7 with the residual stream as plane BITS on both sides, so that a test
// sees hi and lo themselves (signs of zeros, subnormals, the saturated codes) and chooses residual planes no fp32 value splits into.  epi 6: r_hi / r_lo [M,N] =
// the residual planes; epi 7: pos [192,N] fp32 (r_hi / r_lo unused).  o_hi / o_lo [M,N] = the output planes, stats [M, N/64, 2].  in_place (epi 6): the kernel
// updates the residual planes themselves (out == aux, as forward.hip launches it); split-K (flags >> 8) is in place either way.
VP_API int vp_dbg_gemm_case_planes(int32_t device, int32_t dtype, int32_t epi, int32_t variant, int32_t group_m, int32_t flags, int32_t M, int32_t N, int32_t K,
                                   const float* A, const float* W, const float* bias, const uint16_t* r_hi, const uint16_t* r_lo, const float* pos,
                                   int32_t in_place, uint16_t* o_hi, uint16_t* o_lo, float* stats) {
    if ((epi != vp::EPI_BIAS_RESID_LN && epi != vp::EPI_POS_LN) || !o_hi || !o_lo || !stats || (epi == vp::EPI_BIAS_RESID_LN ? !r_hi || !r_lo : !pos || in_place))
        return fail(nullptr, VP_ERR_INVALID, "bad gemm planes case");
    const PlaneIO io{r_hi, r_lo, o_hi, o_lo, in_place != 0};
    return gemm_case(device, dtype, epi, variant, group_m, flags, M, N, K, A, W, bias, pos, nullptr, nullptr, nullptr, stats, &io);
}

// image + crop geometry -> the uint8 [n,256,192,3] RGB crops the model is fed (the device crop/pad/resize kernel alone, behind the staging of
// vp_infer_images: the one-frame case)
VP_API int vp_dbg_crop_prep_image(int32_t device, const vp_image* image, const int32_t* crop_params, int32_t n, uint8_t* out) {
    if (!image || !crop_params || !out || n <= 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    std::vector<int32_t> p9((size_t)n * 9, 0);
    for (int i = 0; i < n; ++i) std::memcpy(&p9[9 * (size_t)i + 1], crop_params + 8 * (size_t)i, 32);
    int32_t band[2];
    std::string why;
    if (image_plan(image, 1, p9.data(), n, band, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    vp_ctx* c = dbg_ctx(device, VP_DTYPE_F16);
    if (!c) return VP_ERR_HIP;
    std::vector<vp::CropRec> recs;
    uint8_t* dout;
    vp::CropRec* drec;
    int rc;
    const size_t ob = (size_t)n * 256 * 192 * 3;
    if ((rc = stage_frames(c, image, 1, false, p9.data(), n, band, recs)) || (rc = dalloc(c, &dout, ob)) || (rc = dalloc(c, &drec, (size_t)n)))
        return dbg_finish(c, rc);
    hipError_t e = hipMemcpy(drec, recs.data(), (size_t)n * sizeof(vp::CropRec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = vp::crop_resize_launch(drec, dout, n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, VP_ERR_HIP, std::string("crop_prep: ") + hipGetErrorString(e));
    return dbg_finish(c, rc);
}

// image + centres and scales -> the uint8 [n,256,192,3] RGB crops of the affine route (crop_affine_kernel alone, behind the staging of vp_infer_images_affine:
// the one-frame case)
VP_API int vp_dbg_crop_affine(int32_t device, const vp_image* image, const float* cs, int32_t n, uint8_t* out) {
    if (!image || !cs || !out || n <= 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    int32_t band[2];
    std::string why;
    if (affine_plan(image, 1, nullptr, cs, n, band, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    vp_ctx* c = dbg_ctx(device, VP_DTYPE_F16);
    if (!c) return VP_ERR_HIP;
    std::vector<const uint8_t*> row0_ptr;
    std::vector<vp::AffRec> recs;
    uint8_t* dout;
    vp::AffRec* drec;
    int rc;
    const size_t ob = (size_t)n * 256 * 192 * 3;
    if ((rc = stage_bands(c, image, 1, false, band, row0_ptr)) || (rc = dalloc(c, &dout, ob)) || (rc = dalloc(c, &drec, (size_t)n))) return dbg_finish(c, rc);
    affine_records(image, nullptr, cs, n, band, row0_ptr, recs);
    hipError_t e = hipMemcpy(drec, recs.data(), (size_t)n * sizeof(vp::AffRec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = vp::crop_affine_launch(drec, dout, n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, VP_ERR_HIP, std::string("crop_affine: ") + hipGetErrorString(e));
    return dbg_finish(c, rc);
}

// ... on a packed RGB frame
VP_API int vp_dbg_crop_prep(int32_t device, const uint8_t* frame, int32_t fh, int32_t fw, const int32_t* crop_params, int32_t n, uint8_t* out) {
    if (!frame || fh <= 0 || fw <= 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    const vp_image im{{frame, nullptr}, {(int64_t)fw * 3, 0}, fh, fw, VP_PIX_RGB24, 0};
    return vp_dbg_crop_prep_image(device, &im, crop_params, n, out);
}

// BASELINE config 5 probe: rows quantised to OCP e4m3 on device + one GEMM through v_mfma_f32_16x16x128_f8f6f4 (fp8_probe.hip)
VP_API int vp_dbg_fp8_gemm(int32_t device, int32_t M, int32_t N, int32_t K, const float* A, const float* a_scale, const float* W,
                           const float* w_scale, float* out, uint8_t* a_codes, uint8_t* w_codes) {
    if (M <= 0 || N <= 0 || K <= 0 || M % 16 || N % 16 || K % 128 || !A || !W || !a_scale || !w_scale || !out)
        return fail(nullptr, VP_ERR_INVALID, "bad fp8 probe shape");
    vp_ctx* c = dbg_ctx(device, VP_DTYPE_F16);
    if (!c) return VP_ERR_HIP;
    float *dA, *dW, *dAs, *dWs, *dO;
    uint8_t *dA8, *dW8;
    int rc;
    if ((rc = upload_f32(c, &dA, A, (size_t)M * K)) || (rc = upload_f32(c, &dW, W, (size_t)N * K)) || (rc = upload_f32(c, &dAs, a_scale, M)) ||
        (rc = upload_f32(c, &dWs, w_scale, N)) || (rc = dalloc(c, &dO, (size_t)M * N)) || (rc = dalloc(c, &dA8, (size_t)M * K)) ||
        (rc = dalloc(c, &dW8, (size_t)N * K)))
        return dbg_finish(c, rc);
    hipError_t e = vp::fp8_probe_launch(dA, dW, dAs, dWs, dA8, dW8, dO, M, N, K, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dO, (size_t)M * N * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && a_codes) e = hipMemcpy(a_codes, dA8, (size_t)M * K, hipMemcpyDeviceToHost);
    if (e == hipSuccess && w_codes) e = hipMemcpy(w_codes, dW8, (size_t)N * K, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, VP_ERR_HIP, std::string("fp8 probe: ") + hipGetErrorString(e));
    return dbg_finish(c, rc);
}

// MX probe (round 4): A -> MXFP8 on device (mx8.h layouts), W -> e4m3 with the per-row scale given; out = block-scaled MFMA product.
// a_codes [M*K] (blocked layout), a_scales [M*K/32] (packed dword layout), w_codes [N*K] may be NULL.
VP_API int vp_dbg_mx_gemm(int32_t device, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* w_scale, float* out,
                          uint8_t* a_codes, uint8_t* a_scales, uint8_t* w_codes) {
    if (M <= 0 || N <= 0 || K <= 0 || M % 64 || N % 16 || K % 128 || !A || !W || !w_scale || !out) return fail(nullptr, VP_ERR_INVALID, "bad mx probe shape");
    vp_ctx* c = dbg_ctx(device, VP_DTYPE_F16);
    if (!c) return VP_ERR_HIP;
    float *dA, *dW, *dWs, *dO;
    uint8_t *dA8, *dAs, *dW8;
    int rc;
    if ((rc = upload_f32(c, &dA, A, (size_t)M * K)) || (rc = upload_f32(c, &dW, W, (size_t)N * K)) || (rc = upload_f32(c, &dWs, w_scale, N)) ||
        (rc = dalloc(c, &dO, (size_t)M * N)) || (rc = dalloc(c, &dA8, (size_t)M * K)) || (rc = dalloc(c, &dAs, (size_t)M * K / 32)) ||
        (rc = dalloc(c, &dW8, (size_t)N * K)))
        return dbg_finish(c, rc);
    hipError_t e = vp::mx_probe_launch(dA, dW, dWs, dA8, dAs, dW8, dO, M, N, K, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dO, (size_t)M * N * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && a_codes) e = hipMemcpy(a_codes, dA8, (size_t)M * K, hipMemcpyDeviceToHost);
    if (e == hipSuccess && a_scales) e = hipMemcpy(a_scales, dAs, (size_t)M * K / 32, hipMemcpyDeviceToHost);
    if (e == hipSuccess && w_codes) e = hipMemcpy(w_codes, dW8, (size_t)N * K, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(c, VP_ERR_HIP, std::string("mx probe: ") + hipGetErrorString(e));
    return dbg_finish(c, rc);
}

// ONE launch of the MXFP8 GEMM kernel (gemm8f.hip) on host fp32 data (tests/test_gpu_fp8.py).  A [M,K] is quantised to MXFP8 on device
// (mx_quantize_launch: the layouts of csrc/mx8.h), W [N,K] on the host exactly as the weight packer does (per-output-channel scale);
// a_deq / w_deq return what the codes and scales stand for, so that the test can restate the product exactly.
//   epi 0: out = a.w^T * w_scale + bias, rounded to fp16        epi 1: out = gelu(...) as MXFP8 (returned de-quantised)
//   epi 6: out = ... + aux (two-plane residual, returned as hi + lo), stats [M, N/64, 2]
// the tile of one case: the project's own rule, as forward.hip asks it (no way to force a tile)
static GemmPick fp8_case_pick(int32_t epi, int32_t M, int32_t N) {
    const int fam = epi == 0 ? VP_PROF_GEMM_QKV : epi == 1 ? VP_PROF_GEMM_FC1 : VP_PROF_GEMM_FC2;
    return resolve_gemm_fp8(fam, epi, M, N);
}
// what vp_dbg_gemm_fp8_case_raw adds (tests/test_gpu_fp8_gemm.py): the buffers as the device holds them
struct Fp8Raw {
    bool out_blocked;                       // epi 0: LnFuse::out_blocked; `out` comes back in device order [M/64][N/64][64][64]
    uint8_t *o_codes, *o_scales, *a_scales; // epi 1: output codes [M*N] / scale bytes [M*N/32]; any epi: operand scale bytes [M*K/32]; device order, may be NULL
};
// the body of vp_dbg_gemm_fp8_case, vp_dbg_gemm_fp8_case_raw and vp_dbg_gemm_fp8_case_planes (io != NULL: epi 6 on plane bits)
static int gemm_fp8_case(int32_t device, int32_t epi, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias, const float* aux, float* out,
                         float* stats, float* a_deq, float* w_deq, const PlaneIO* io, const Fp8Raw* raw = nullptr) {
    if (M <= 0 || N <= 0 || K <= 0 || M % 256 || K % 256 || N % 64 || !A || !W || !bias || (epi != 0 && epi != 1 && epi != 6) || (raw && raw->out_blocked && epi != 0))
        return fail(nullptr, VP_ERR_INVALID, "bad fp8 gemm case");
    vp_ctx* c = dbg_ctx(device, VP_DTYPE_F16);
    if (!c) return VP_ERR_HIP;
    int r;
    const size_t MN = (size_t)M * N, MK = (size_t)M * K;
    float *dA, *dB, *dWs, *dStats = nullptr;
    uint8_t *dA8, *dAs, *dW8, *dOs = nullptr;
    uint16_t* dAux16 = nullptr;
    char* dOut;
    if ((r = upload_f32(c, &dA, A, MK)) || (r = dalloc(c, &dA8, MK)) || (r = dalloc(c, &dAs, MK / 32)) ||
        (r = upload_fp8_rows(c, &dW8, &dWs, nullptr, W, nullptr, nullptr, nullptr, N, K)) || (r = upload_f32(c, &dB, bias, N, pad128(N))))
        return dbg_finish(c, r);
    hipError_t e = vp::mx_quantize_launch(dA, dA8, dAs, M, K, nullptr);
    if (e != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "mx quantize"));
    const size_t out_bytes = epi == 0 ? MN * 2 : epi == 1 ? MN : MN * 4;
    LnFuse ln;
    if (epi == 1) {
        if ((r = dalloc(c, &dOs, MN / 32))) return dbg_finish(c, r);
        hipMemset(dOs, 0xff, MN / 32);   // as the codes below: an unwritten scale dword shows
    }
    if (raw) ln.out_blocked = raw->out_blocked;
    if (epi == 6) {
        if ((r = upload_planes(c, &dAux16, aux, io ? io->r_hi : nullptr, io ? io->r_lo : nullptr, MN)) || (r = dalloc(c, &dStats, (size_t)M * (N / 64) * 2)))
            return dbg_finish(c, r);
        ln.plane = MN; ln.stats_out = dStats;
    }
    if (io && io->in_place) dOut = (char*)dAux16;   // as forward.hip launches mlp.fc2: out == aux
    else {
        if ((r = dalloc(c, &dOut, out_bytes))) return dbg_finish(c, r);
        hipMemset(dOut, 0xff, out_bytes);
    }
    const int fam = epi == 0 ? VP_PROF_GEMM_QKV : epi == 1 ? VP_PROF_GEMM_FC1 : VP_PROF_GEMM_FC2;
    r = gemm_fp8(c, fam, epi, fp8_case_pick(epi, M, N), dA8, dAs, dW8, dWs, dB, dOut, dOs, (const float*)dAux16, M, N, K, &ln);
    if (!r && hipDeviceSynchronize() != hipSuccess) r = fail(c, VP_ERR_HIP, "fp8 gemm kernel failed");
    if (r) return dbg_finish(c, r);
    // what the operands stand for
    {
        std::vector<uint8_t> ca(MK), sa(MK / 32);
        if (hipMemcpy(ca.data(), dA8, MK, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(sa.data(), dAs, MK / 32, hipMemcpyDeviceToHost) != hipSuccess)
            return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
        if (raw && raw->a_scales) memcpy(raw->a_scales, sa.data(), sa.size());
        if (a_deq)
            for (size_t m = 0; m < (size_t)M; ++m)
                for (size_t k = 0; k < (size_t)K; ++k)
                    a_deq[m * K + k] = vp_host_e4m3_to_float(ca[vp::mx_code_off(m, k, K)]) * std::ldexp(1.0f, (int)sa[vp::mx_scale_off(m, k >> 5, K)] - 127);
        if (w_deq) {
            std::vector<uint8_t> cw((size_t)N * K);
            std::vector<float> sw(N);
            if (hipMemcpy(cw.data(), dW8, cw.size(), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(sw.data(), dWs, (size_t)N * 4, hipMemcpyDeviceToHost) != hipSuccess)
                return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
            for (size_t n = 0; n < (size_t)N; ++n)
                for (size_t k = 0; k < (size_t)K; ++k) w_deq[n * K + k] = vp_host_e4m3_to_float(cw[n * K + k]) * sw[n];
        }
    }
    if (epi == 0) {
        r = download16(c, (const uint16_t*)dOut, out, MN);
    } else if (epi == 1) {
        std::vector<uint8_t> co(MN), so(MN / 32);
        if (hipMemcpy(co.data(), dOut, MN, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(so.data(), dOs, MN / 32, hipMemcpyDeviceToHost) != hipSuccess)
            return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
        if (raw && raw->o_codes) memcpy(raw->o_codes, co.data(), co.size());
        if (raw && raw->o_scales) memcpy(raw->o_scales, so.data(), so.size());
        for (size_t m = 0; m < (size_t)M; ++m)
            for (size_t n = 0; n < (size_t)N; ++n)
                out[m * N + n] = vp_host_e4m3_to_float(co[vp::mx_code_off(m, n, N)]) * std::ldexp(1.0f, (int)so[vp::mx_scale_off(m, n >> 5, N)] - 127);
    } else {
        if ((r = download_planes(c, (const uint16_t*)dOut, out, io ? io->o_hi : nullptr, io ? io->o_lo : nullptr, MN))) return dbg_finish(c, r);
        if (stats && hipMemcpy(stats, dStats, (size_t)M * (N / 64) * 8, hipMemcpyDeviceToHost) != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
    }
    return dbg_finish(c, r);
}

VP_API int vp_dbg_gemm_fp8_case(int32_t device, int32_t epi, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias,
                                const float* aux, float* out, float* stats, float* a_deq, float* w_deq) {
    if (!out) return fail(nullptr, VP_ERR_INVALID, "bad fp8 gemm case");
    return gemm_fp8_case(device, epi, M, N, K, A, W, bias, aux, out, stats, a_deq, w_deq, nullptr);
}

// ... with the buffers as the device holds them (tests/test_gpu_fp8_gemm.py).  flags: 1 = LnFuse::out_blocked (epi 0 only).  o_codes / o_scales (epi 1) and
// a_scales may be NULL; the test de-blocks them itself
VP_API int vp_dbg_gemm_fp8_case_raw(int32_t device, int32_t epi, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias, const float* aux,
                                    float* out, float* stats, float* a_deq, float* w_deq, int32_t flags, uint8_t* o_codes, uint8_t* o_scales, uint8_t* a_scales) {
    if (!out || (flags & ~1)) return fail(nullptr, VP_ERR_INVALID, "bad fp8 gemm case");
    const Fp8Raw raw{(flags & 1) != 0, o_codes, o_scales, a_scales};
    return gemm_fp8_case(device, epi, M, N, K, A, W, bias, aux, out, stats, a_deq, w_deq, nullptr, &raw);
}

// host only: the tile the taps above launch a case on -- resolve_gemm_fp8's variant (16 = 256 x 256, 17 = 256 x 192) and its group_m
VP_API int vp_dbg_gemm_fp8_pick(int32_t epi, int32_t M, int32_t N, int32_t* variant, int32_t* group_m) {
    if (M <= 0 || N <= 0 || (epi != 0 && epi != 1 && epi != 6) || !variant || !group_m) return VP_ERR_INVALID;
    const GemmPick p = fp8_case_pick(epi, M, N);
    *variant = p.variant; *group_m = p.group_m;
    return VP_OK;
}

// ... and its producer-row sibling (epi 6), as vp_dbg_gemm_case_planes: residual and output as plane bits, in_place = out == aux; a_deq / w_deq as above
VP_API int vp_dbg_gemm_fp8_case_planes(int32_t device, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias, const uint16_t* r_hi,
                                       const uint16_t* r_lo, int32_t in_place, uint16_t* o_hi, uint16_t* o_lo, float* stats, float* a_deq, float* w_deq) {
    if (!r_hi || !r_lo || !o_hi || !o_lo || !stats) return fail(nullptr, VP_ERR_INVALID, "bad fp8 gemm planes case");
    const PlaneIO io{r_hi, r_lo, o_hi, o_lo, in_place != 0};
    return gemm_fp8_case(device, 6, M, N, K, A, W, bias, nullptr, nullptr, stats, a_deq, w_deq, &io);
}

// host-only: fp32 -> OCP e4m3 codes with the library's own converter (the one the weight packer of the fp8 mode uses)
VP_API int vp_dbg_host_e4m3(const float* in, uint8_t* out, int64_t n) {
    if (!in || !out || n < 0) return VP_ERR_INVALID;
    for (int64_t i = 0; i < n; ++i) out[i] = vp_host_e4m3(in[i]);
    return VP_OK;
}

}  // extern "C"
