// Epilogues of the 8-phase GEMM kernels, written once for gemm8.hip (16-bit operands) and gemm8f.hip (MXFP8 operands).
//
// Both kernels leave a tile in the same accumulator layout (gemm8.hip's header: lane (fg, frow) of wave (wr, wc) holds, for fragment f and row
// group J, four values of tile row  wr XR/2 + rowJ(J) + frow), and differ only in how a lane's value is formed from it: acc + bias there,
// fma(acc, w_scale, bias) here.  So an epilogue below takes the VALUE as a callback  val(f, J) -> f32x4  and owns the rest:
//   * G8ResidLds<C>     geometry of the LDS-staged residual epilogue (256 x 192 tiles): the kernels' pass loops and the launchers' LDS size
//   * g8_resid_regs     register-direct residual epilogue (256-wide tiles): residual loads, planes_decode8 / planes_split8, stores, granule_stats16
// The operand ring, its waits and barriers, and the bias / scale loads stay in the kernels.
#pragma once
#include "gemm8_common.h"

namespace vp {
namespace {

// tile row of m-fragment J of a wave (+ wr XR/2 + lane row)
template <class C> __device__ __forceinline__ constexpr int g8_rowJ(int J) { return (J / C::MJ) * C::XR + (J % C::MJ) * 16; }

// LDS-staged residual epilogue: the tile passes through LDS in NPASS passes of CR rows (fp32, rows padded by 16 bytes), is walked in 8-column
// chunks (NCH per thread and pass) as in gemm.hip's fused-LayerNorm producer, and the granule statistics of the whole tile collect behind the rows.
template <class C> struct G8ResidLds {
    static constexpr int ROWBYTES = C::BN * 4 + 16;
    static constexpr int JPP = (C::BN == 256) ? 2 : 4;  // m-fragments (per wave and X half) staged per pass
    static constexpr int CR = 32 * JPP;                 // rows per pass
    static constexpr int NPASS = 256 / CR;
    static constexpr int CPR = C::BN / 8;               // 8-element chunks per row
    static constexpr int NCH = CR * CPR / C::NT;        // chunks per thread per pass
    static constexpr int GR = C::BN / 64;               // statistics granules per row
    static constexpr int BYTES = CR * ROWBYTES + C::BM * GR * 8;   // staged rows + statistics of the tile
    static constexpr int LDS = BYTES > C::RING ? BYTES : C::RING;  // dynamic LDS of a kernel with this epilogue
    static_assert(NCH * C::NT == CR * CPR, "chunks must split evenly over threads");
    static_assert(BYTES <= 160 * 1024, "LDS");
    // staged row lr of pass p  <->  tile row (p / (4/JPP)) 128 + (lr / (16 JPP)) 64 + ((p % (4/JPP)) JPP + (lr / 16) % JPP) 16 + lr % 16
    static __device__ __forceinline__ int tile_row(int p, int lr) {
        return (p / (4 / JPP)) * 128 + (lr / (16 * JPP)) * 64 + ((p % (4 / JPP)) * JPP + (lr / 16) % JPP) * 16 + (lr & 15);
    }
};

// Residual epilogue straight from registers (EPI_BIAS_RESID_LN on 256-wide tiles).  Lane (fg_e, frow_e): rows mrow + rowJ(J), columns nb .. nb + 15
// (W rows are permuted on their way into LDS); the statistics granule is the four lanes fg_e = 0..3 of a row (common.h, granule_stats16).  No LDS,
// no barrier: the operand ring runs on across the tile boundary.  The residual of row group J (hi cols 0-7, hi 8-15, lo 0-7, lo 8-15) is fetched RD
// row groups ahead (0: load, then use).
template <class T, class C, int RD, class Val>
__device__ __forceinline__ void g8_resid_regs(const GemmArgs& g, int mrow, int nb, int fg_e, Val val) {
    uint16_t* out_hi = (uint16_t*)g.out;
    uint16_t* out_lo = out_hi + g.plane;
    const uint16_t* aux_hi = (const uint16_t*)g.aux;
    const uint16_t* aux_lo = aux_hi + g.plane;
    const bool store = !(VP_ABLATE(g) & 8);
    const int gran = g.N >> 6;
    u32x4 res[RD + 1][4];
    auto load_res = [&](int J, u32x4(&r)[4]) {
        const size_t o = (size_t)(mrow + g8_rowJ<C>(J)) * g.ldo + nb;
        r[0] = *(const u32x4*)(aux_hi + o);
        r[1] = *(const u32x4*)(aux_hi + o + 8);
        r[2] = *(const u32x4*)(aux_lo + o);
        r[3] = *(const u32x4*)(aux_lo + o + 8);
    };
#pragma unroll
    for (int J = 0; J < RD; ++J) load_res(J, res[J]);
#pragma unroll
    for (int J = 0; J < C::TJ; ++J) {
        if (J + RD < C::TJ) load_res(J + RD, res[(J + RD) % (RD + 1)]);
        const u32x4(&r)[4] = res[J % (RD + 1)];
        const int m = mrow + g8_rowJ<C>(J);
        const size_t o = (size_t)m * g.ldo + nb;
        float v[16];   // column nb + c
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const f32x4 st = val(f, J);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[f * 4 + e] = st[e] + planes_decode8<T>(r[f >> 1], r[2 + (f >> 1)], (f & 1) * 4 + e);
        }
        u32x4 oh[2], ol[2];
        planes_split8<T>(v, oh[0], ol[0]);
        planes_split8<T>(v + 8, oh[1], ol[1]);
        if (store) {
            *(u32x4*)(out_hi + o) = oh[0];
            *(u32x4*)(out_hi + o + 8) = oh[1];
            *(u32x4*)(out_lo + o) = ol[0];
            *(u32x4*)(out_lo + o + 8) = ol[1];
        }
        const float2 gs = granule_stats16(v);
        if (fg_e == 0 && store) *(float2*)(g.stats_out + ((size_t)m * gran + (nb >> 6)) * 2) = gs;
    }
}

}  // namespace
}  // namespace vp
