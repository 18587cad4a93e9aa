// The simple decoder's head (csrc/simpleheadgeom.h): ReLU -> bilinear x 4 -> Conv2d(D, K, 3, padding = 1) as ONE kernel in the commuted form, plus its public
// symbols: vp_head_kind, vp_dbg_simple_head_case (the launch head_chunk builds, on host data) and vp_dbg_simple_head_pack (HOST ONLY: the weight image).
//
// One workgroup of 4 waves per (crop, slab of 16 output maps):
//   MFMA phase     P[9 taps][16 maps][192 tokens] = relu(tokens) . W_t^T on mfma_f32_16x16x32, operands straight from global memory (a wave owns 48 tokens = 3 row
//                  tiles and all 9 taps: 27 accumulator tiles), ReLU on the token bits as they are loaded, the hi and the lo weight rows into the same accumulators.
//                  The fp32 result goes to LDS: rows of 196 floats (192 + 4, so that the 16 maps a store instruction touches fall on different banks), 112 896 B,
//                  one workgroup per CU.
//   stencil phase  a thread takes (map, token cell): the 4 x 4 output pixels of the cell need the 3 x 3 neighbouring cells of each tap (81 LDS reads for 16 outputs),
//                  consecutive lanes read consecutive tokens; it writes four 16-byte pieces of the [n, K, 64, 48] heatmaps.
// No atomics, no intermediate in HBM, no 16-bit rounding behind the tokens; a crop's maps depend on that crop's tokens only and the order of every sum is fixed.
#include "api_internal.h"
#include "common.h"
#include "dbg_util.h"
#include "simpleheadgeom.h"

using namespace vpi;

namespace vp {

constexpr int SH_THREADS = 256, SH_WAVES = 4, SH_WAVE_TILES = SH_TOKENS / 16 / SH_WAVES;   // 3 token tiles per wave
constexpr int SH_LDS_ROW = SH_TOKENS + 4;                                                  // floats per (tap, map) row of P
constexpr int SH_LDS_BYTES = SH_TAPS * SH_SLAB * SH_LDS_ROW * 4;
static_assert(SH_WAVE_TILES * SH_WAVES * 16 == SH_TOKENS, "the waves split the token tiles evenly");
static_assert(SH_SLAB * SH_TOKENS % SH_THREADS == 0, "the threads split the (map, cell) items evenly");
static_assert(SH_LDS_BYTES <= 160 * 1024, "P fits the LDS of a CU");

// sign set -> +0 on both halves of a 32-bit pair: -0.0 and every negative (NaN with the sign set included) contribute nothing
__device__ __forceinline__ uint32_t relu_bits2(uint32_t x) { return x & ~(((x >> 15) & 0x00010001u) * 0xffffu); }

template <class T>
__global__ __launch_bounds__(SH_THREADS) void simple_head_kernel(SimpleHeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float P[];
    const int slab = blockIdx.x, crop = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int D = a.D;
    {
        const uint16_t* arow[SH_WAVE_TILES];
#pragma unroll
        for (int m = 0; m < SH_WAVE_TILES; ++m) arow[m] = a.y + ((size_t)crop * SH_TOKENS + (wave * SH_WAVE_TILES + m) * 16 + r) * D + g * 8;
        const uint16_t* wrow = a.w + ((size_t)slab * 2 * SH_SLAB + r) * D + g * 8;   // rows < a.rows, columns < D: inside the image
        const size_t tap_stride = a.rows * (size_t)D, lo_off = (size_t)SH_SLAB * D;
        f32x4 acc[SH_WAVE_TILES][SH_TAPS];
#pragma unroll
        for (int m = 0; m < SH_WAVE_TILES; ++m)
#pragma unroll
            for (int t = 0; t < SH_TAPS; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < D; k0 += 32) {
            u32x4 af[SH_WAVE_TILES];
#pragma unroll
            for (int m = 0; m < SH_WAVE_TILES; ++m) {
                af[m] = *reinterpret_cast<const u32x4*>(arow[m] + k0);
#pragma unroll
                for (int e = 0; e < 4; ++e) af[m][e] = relu_bits2(af[m][e]);
            }
#pragma unroll
            for (int t = 0; t < SH_TAPS; ++t) {
                const u32x4 bh = *reinterpret_cast<const u32x4*>(wrow + t * tap_stride + k0);
                const u32x4 bl = *reinterpret_cast<const u32x4*>(wrow + t * tap_stride + lo_off + k0);
#pragma unroll
                for (int m = 0; m < SH_WAVE_TILES; ++m) acc[m][t] = mfma16<T>(af[m], bh, acc[m][t]);
#pragma unroll
                for (int m = 0; m < SH_WAVE_TILES; ++m) acc[m][t] = mfma16<T>(af[m], bl, acc[m][t]);
            }
        }
        // C lane l holds rows (tokens) 4 g .. 4 g + 3 of column (map) r: one 16-byte store per tile
#pragma unroll
        for (int m = 0; m < SH_WAVE_TILES; ++m)
#pragma unroll
            for (int t = 0; t < SH_TAPS; ++t)
                *reinterpret_cast<f32x4*>(&P[(t * SH_SLAB + r) * SH_LDS_ROW + (wave * SH_WAVE_TILES + m) * 16 + g * 4]) = acc[m][t];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < SH_SLAB * SH_TOKENS; q += SH_THREADS) {
        const int map = q / SH_TOKENS, cell = q - map * SH_TOKENS, k = slab * SH_SLAB + map;
        if (k >= a.K) break;   // maps ascend with q: the rest of a ragged slab is padding
        const int i = cell / SH_GRID_W, j = cell - i * SH_GRID_W;
        // positions a = 0 .. 5 of the 6 x 6 window of samples the cell's 4 x 4 outputs reach through the 3 x 3 taps: yy = 4 i - 1 + a.  sh_sample's i0 is row i - 1 for
        // a < 3 and row i beyond; where it clamps instead (i0 == i1, or l == 0 at the top rows) the clamped window row holds the same value and sh_lerp returns it exactly
        float ly[6], lx[6];
        bool vy[6], vx[6];
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            int i0, i1;
            const int yy = SH_UP * i - 1 + s, xx = SH_UP * j - 1 + s;
            vy[s] = (unsigned)yy < (unsigned)SH_HM_H;
            vx[s] = (unsigned)xx < (unsigned)SH_HM_W;
            sh_sample(yy, SH_GRID_H, &i0, &i1, &ly[s]);
            sh_sample(xx, SH_GRID_W, &i0, &i1, &lx[s]);
        }
        const int wr[3] = {(i > 0 ? i - 1 : 0) * SH_GRID_W, i * SH_GRID_W, (i < SH_GRID_H - 1 ? i + 1 : i) * SH_GRID_W};
        const int wc[3] = {j > 0 ? j - 1 : 0, j, j < SH_GRID_W - 1 ? j + 1 : j};
        const float bias = a.bias[k];
        float acc[4][4];
#pragma unroll
        for (int by = 0; by < 4; ++by)
#pragma unroll
            for (int bx = 0; bx < 4; ++bx) acc[by][bx] = bias;
#pragma unroll
        for (int t = 0; t < SH_TAPS; ++t) {
            const int ky = t / 3, kx = t - 3 * ky;
            const float* p = &P[(t * SH_SLAB + map) * SH_LDS_ROW];
            float w[3][3];
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int e = 0; e < 3; ++e) w[d][e] = p[wr[d] + wc[e]];
#pragma unroll
            for (int by = 0; by < 4; ++by) {
                const int s = by + ky, d0 = s < 3 ? 0 : 1;
                float v[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) v[e] = vy[s] ? sh_lerp(w[d0][e], w[d0 + 1][e], ly[s]) : 0.f;
#pragma unroll
                for (int bx = 0; bx < 4; ++bx) {
                    const int s2 = bx + kx, e0 = s2 < 3 ? 0 : 1;
                    const float u = vx[s2] ? sh_lerp(v[e0], v[e0 + 1], lx[s2]) : 0.f;
                    acc[by][bx] = acc[by][bx] + u;
                }
            }
        }
        float* o = a.hm + ((size_t)crop * a.K + k) * (SH_HM_H * SH_HM_W) + (size_t)(SH_UP * i) * SH_HM_W + SH_UP * j;
#pragma unroll
        for (int by = 0; by < 4; ++by) *reinterpret_cast<f32x4*>(o + by * SH_HM_W) = f32x4{acc[by][0], acc[by][1], acc[by][2], acc[by][3]};
    }
}

hipError_t simple_head_launch(int dtype, const SimpleHeadArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.n > 65535 || a.K <= 0 || a.D <= 0 || a.D % 32 || a.rows != sh_rows((size_t)a.K) || !a.y || !a.w || !a.bias || !a.hm ||
        ((uintptr_t)a.hm & 15) || ((uintptr_t)a.y & 15) || ((uintptr_t)a.w & 15))
        return hipErrorInvalidValue;
    static bool attr_done[2][64] = {};
    auto kern = dtype == DT_F16 ? simple_head_kernel<F16> : simple_head_kernel<BF16>;
    if (hipError_t e = lds_opt_in((const void*)kern, SH_LDS_BYTES, attr_done[dtype == DT_F16 ? 0 : 1]); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((a.K + SH_SLAB - 1) / SH_SLAB, a.n), dim3(SH_THREADS), SH_LDS_BYTES, s, a);
    return hipGetLastError();
}

}  // namespace vp

extern "C" {

int vp_head_kind(vp_handle c) {
    if (need_weights(c)) return -1;
    return c->head_kind;
}

int vp_dbg_simple_head_pack(int32_t dtype, int32_t K, int32_t D, const float* w, uint16_t* image, int32_t* rows) {
    if ((dtype != VP_DTYPE_F16 && dtype != VP_DTYPE_BF16) || K <= 0 || K > 4096 || D <= 0 || D > 8192 || !w || !rows)
        return fail(nullptr, VP_ERR_INVALID, "bad simple head pack");
    *rows = (int32_t)vp::sh_rows((size_t)K);
    if (!image) return VP_OK;
    std::vector<uint16_t> img;
    pack_simple_final(w, K, D, dtype == VP_DTYPE_F16 ? vp::DT_F16 : vp::DT_BF16, img);
    std::memcpy(image, img.data(), img.size() * 2);
    return VP_OK;
}

int vp_dbg_simple_head_case(int32_t device, int32_t dtype, int32_t B, int32_t Cin, const float* x, const float* w, const float* b, int32_t Kp, float* out,
                            uint8_t* guard) {
    if (B <= 0 || B > 4096 || Cin <= 0 || Cin % 32 || Cin > 8192 || Kp <= 0 || Kp > 4096 || !x || !w || !b || !out || !guard ||
        (dtype != VP_DTYPE_F16 && dtype != VP_DTYPE_BF16))
        return fail(nullptr, VP_ERR_INVALID, "bad simple head case");
    vp_ctx* c = dbg_ctx(device, dtype);
    if (!c) return VP_ERR_HIP;
    c->D = Cin; c->Kp = Kp; c->head_kind = 1;
    const size_t M = (size_t)B * vp::SH_TOKENS, hm_n = (size_t)B * Kp * 3072, G = (size_t)16 * 3072;
    uint16_t* dx;
    float* d_hm;
    int rc;
    if ((rc = upload_mat(c, &dx, x, M, Cin, M)) || (rc = upload_simple_final(c, &c->w_fin, w, Kp, Cin, &c->fin_rows)) ||
        (rc = upload_f32(c, &c->b_fin, b, Kp, pad128(Kp))) || (rc = dalloc(c, &d_hm, hm_n + G)))
        return dbg_finish(c, rc);
    if (hipMemset(d_hm, 0xff, (hm_n + G) * 4) != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "memset"));
    HeadPlan hp = plan_head(c->sw, Cin, B, c->fin_rows, 1);
    if ((rc = head_chunk(c, dx, B, d_hm, hp))) return dbg_finish(c, rc);
    if (hipDeviceSynchronize() != hipSuccess) return dbg_finish(c, fail(c, VP_ERR_HIP, "simple head kernel failed"));
    if (hipMemcpy(out, d_hm, hm_n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(guard, d_hm + hm_n, G * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return dbg_finish(c, fail(c, VP_ERR_HIP, "D2H"));
    return dbg_finish(c, VP_OK);
}

}  // extern "C"
