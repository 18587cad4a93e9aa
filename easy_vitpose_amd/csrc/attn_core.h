// The attention core of the fixed 192-token ViTPose sequence (vit.py:164-176), ONE definition for the three kernels that run it:
// attention_kernel (attention.hip: head dim 32 / 64 / 80), qkvattn_kernel (qkvattn.hip: head dim 64 behind the qkv GEMM) and the EPI_QKV_ATTN
// tile of gemm8.hip (head dim 80 behind the qkv GEMM).  The fused kernels must give the unfused path's bits (tests/test_gpu_api.py flips the
// fused path, tests/test_gpu_attention.py compares them on hot operands): everything that agreement rests on is here.
//
//  S^T = K Q^T   (MFMA A = K rows from LDS, B = Q rows)
//  softmax over keys in fp32 registers (scale folded into the exponent)
//  O^T = V^T P^T (MFMA A = V^T via the gfx950 LDS transpose read, B = P^T = the S^T accumulators re-packed)
//
// Computing the TRANSPOSED products makes every lane own one query column (q = lane & 15): row max / row sum need only two cross-lane steps
// (xor 16, 32), and the S^T accumulator registers of two 16-key tiles are directly the 8-element B fragment of the PV MFMA (the MFMA k index is
// a permutation-invariant sum: k slot (g, e) = key 32 kb + 4 g + e for e < 4, 32 kb + 16 + 4 g + e - 4 otherwise).
//
// V stays ROW-MAJOR in LDS, cut into [192 keys][16 d] sub-tiles (32-byte rows, so the 8 rows a 32-lane half touches are one 256-byte bank row:
// conflict-free without padding); `ds_read_b64_tr_b16` hands lane i of a 16-lane group column i of a [4 keys][16 d] block, i.e. the V^T
// fragment, with no transposed staging pass.  When the head dim is a multiple of 32 the d columns of sub-tile pairs are interleaved (column c of
// sub-tile dt = d 32(dt/2) + 8(c/4) + 4(dt&1) + c%4) so that a lane's two O^T accumulators are 8 consecutive head-dim values of one query = one
// 16-byte store (attn_out_pair); head dim 80 has five plain sub-tiles and 8-byte stores (attn_out_single).
//
// What a site keeps: its LDS layouts and hand-overs, where Q comes from, its tile loops and what runs between the steps -- and the S^T = K Q^T
// loop itself.  The three differ in the K row stride (128 bytes with the GEMM's XOR swizzle, HDP * 2 + 16, 160), in how the d >= 80 lanes of the
// third k-step are zeroed and in Q coming from HBM or from LDS; one form for all of them would have to change a site's address arithmetic, so
// each keeps its own.  Its contract with the rest: s[kt] = keys 16 kt .. + 15 (rows, MFMA A) x the tile's 16 queries (columns), k ascending in
// steps of 32.  The kb loop of O^T = V^T P^T stays at the sites too, around attn_vt_frag: as one helper over QT tiles x G sub-tiles it cost
// attention_kernel<32> 13 VGPRs (91 -> 104: four blocks per CU instead of five).
#pragma once
#include "common.h"

namespace vp {

// ds_read_b64_tr_b16: column i of a [4 keys][16 d] block to lane i of a 16-lane group
__device__ __forceinline__ u32x2 lds_read_tr16(const char* p) {
    typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 h4;
    typedef __attribute__((address_space(3))) h4* lds_h4;
    const h4 v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4)(p));
    return __builtin_bit_cast(u32x2, v);
}

// Softmax of one query tile over its 12 score accumulators (destroyed: they hold the unrounded p afterwards); P re-packed as the six PV
// B-fragments, returns 1 / l.  Max and sum run kt-major inside the lane, then xor 16, xor 32; l is summed from the UNROUNDED p.  P is in [0, 1]
// and O a convex combination of 16-bit V values: neither can overflow the 16-bit range, so no saturating conversion here or in attn_out_*.
template <class T> __device__ __forceinline__ float attn_softmax(f32x4 (&s)[12], float scale_log2e, u32x4 (&pf)[6]) {
    float mx = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < 12; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float l = 0.f;
    const float mb = mx * scale_log2e;
#pragma unroll
    for (int kt = 0; kt < 12; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = softmax_p(s[kt][r], scale_log2e, mb);
            s[kt][r] = p;
            l += p;
        }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
#pragma unroll
    for (int kb = 0; kb < 6; ++kb) {
        pf[kb][0] = pack2_nosat<T>(s[2 * kb][0], s[2 * kb][1]);
        pf[kb][1] = pack2_nosat<T>(s[2 * kb][2], s[2 * kb][3]);
        pf[kb][2] = pack2_nosat<T>(s[2 * kb + 1][0], s[2 * kb + 1][1]);
        pf[kb][3] = pack2_nosat<T>(s[2 * kb + 1][2], s[2 * kb + 1][3]);
    }
    return 1.0f / l;
}

// per-lane base of the V transpose reads (Vs = the V image, fr = lane & 15, fg = lane >> 4): lane (4 j + m) of a 16-lane group supplies the
// address of (key 4 fg + j, column chunk m) and receives column fr of keys 4 fg .. 4 fg + 3.  attention.hip and gemm8.hip write this one line
// out: behind a call hipcc no longer shares its terms with their K / Q addresses and forms it with one or two more VALU instructions
__device__ __forceinline__ const char* attn_vfrag(const char* Vs, int fr, int fg) { return Vs + (fg * 4 + (fr >> 2)) * 32 + (fr & 3) * 8; }

// V^T A-fragment of (sub-tile dt, key block kb); vfrag = attn_vfrag of the V image, VSUB = bytes per sub-tile
template <int VSUB> __device__ __forceinline__ u32x4 attn_vt_frag(const char* vfrag, int dt, int kb) {
    const char* p = vfrag + dt * VSUB + kb * 1024;
    const u32x2 lo = lds_read_tr16(p);          // keys 32 kb + 4 g + 0..3
    const u32x2 hi = lds_read_tr16(p + 512);    // keys 32 kb + 16 + 4 g + 0..3
    return u32x4{lo[0], lo[1], hi[0], hi[1]};
}

// output conversion: o * 1/l, then 16 bit.  attn_out_scale is the multiply alone (the MXFP8 output stage of attention.hip quantises its values)
__device__ __forceinline__ f32x4 attn_out_scale(f32x4 o, float inv_l) { return f32x4{o[0] * inv_l, o[1] * inv_l, o[2] * inv_l, o[3] * inv_l}; }
// one accumulator = rows d 16 dt + 4 fg + {0..3} of a plain sub-tile: 8 bytes
template <class T> __device__ __forceinline__ u32x2 attn_out_single(f32x4 o, float inv_l) {
    const f32x4 v = attn_out_scale(o, inv_l);
    return u32x2{pack2_nosat<T>(v[0], v[1]), pack2_nosat<T>(v[2], v[3])};
}
// the accumulators of an interleaved sub-tile pair = d 16 dp + 8 fg + {0..3} and + {4..7}: 16 bytes
template <class T> __device__ __forceinline__ u32x4 attn_out_pair(f32x4 o0, f32x4 o1, float inv_l) {
    const u32x2 a = attn_out_single<T>(o0, inv_l), b = attn_out_single<T>(o1, inv_l);
    return u32x4{a[0], a[1], b[0], b[1]};
}

}  // namespace vp
