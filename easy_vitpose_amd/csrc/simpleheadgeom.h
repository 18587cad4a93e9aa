// The ViTPose *simple* decoder (upstream ViTPose's TopdownHeatmapSimpleHead with num_deconv_layers = 0, upsample = 4, final_conv_kernel = 3):
//     hm = Conv2d(D, K, 3, padding = 1)( bilinear x 4, align_corners = False ( relu(tokens [n, 16, 12, D]) ) )
// stated once for the kernel of simplehead.hip, the weight packer and the host taps.  Nothing else in the library states the sampling rule, the zero rule of the
// 64 x 48 border, the weight layout or the summation order.
//
// The literal form.  r = relu(tokens):
//     hm[k, y, x] = b[k] + sum over (ky, kx, c) of w[k, c, ky, kx] U(r)[c, y + ky - 1, x + kx - 1]
// U = the x 4 upsample to 64 x 48 (sh_sample below, rows and columns alike), and U(r) is ZERO outside 64 x 48 (the convolution's padding).
//
// The form that runs.  ReLU comes first and everything behind it is linear, so the upsample and the channel sum commute:
//     P_t[k] = r . W_t^T at 16 x 12 for each of the 9 taps t = 3 ky + kx         one GEMM: M = 192 n, N = 9 K, K = D
//     hm[k, y, x] = b[k] + sum over t of U(P_t[k])[y + ky - 1, x + kx - 1]       with the same zero outside 64 x 48
// 16 x fewer multiply-adds than the literal form, and the 64 x 48 x D tensor never exists.
//
// The summation order of one output element (fixed: run to run and batch position to batch position the bits are the same):
//     acc = b[k];  for t = 0 .. 8 in this order:  acc = acc + u_t
//     u_t = 0 where (y + ky - 1, x + kx - 1) lies outside 64 x 48, else with (i0, i1, ly) = sh_sample(y + ky - 1, 16) and (j0, j1, lx) = sh_sample(x + kx - 1, 12):
//         c0 = sh_lerp(P_t[i0][j0], P_t[i1][j0], ly)     c1 = sh_lerp(P_t[i0][j1], P_t[i1][j1], ly)     u_t = sh_lerp(c0, c1, lx)
//     sh_lerp(a, b, l) = fma(l, b - a, a): where the rule clamps (i1 == i0, or l == 0) it returns a exactly.
// P_t[k] itself is an fp32 MFMA accumulation over D of the 16-bit tokens (ReLU applied on the bits: sign set -> +0) with the hi rows, then the lo rows, of the
// weight image into the same accumulator, 32 channels per instruction in ascending channel order.  Nothing is rounded to 16 bits between the tokens and the heatmap.
//
// The weight image.  final_layer.weight [K, D, 3, 3] -> per tap t a [rows][D] matrix in the operand type, rows = 32 ceil(K / 16) in upload_final's interleave:
// map k's hi row at (k / 16) 32 + k % 16, its lo row 16 behind (hi = round16(w), lo = round16(w - hi)); rows of maps beyond K are zero.  Tap t starts at
// t rows D (sh_weight_index).  The bias stays float32.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SH_HD __host__ __device__ inline
#else
#define SH_HD inline
#endif

namespace vp {

constexpr int SH_GRID_H = 16, SH_GRID_W = 12, SH_TOKENS = SH_GRID_H * SH_GRID_W;   // the token grid
constexpr int SH_UP = 4, SH_HM_H = SH_UP * SH_GRID_H, SH_HM_W = SH_UP * SH_GRID_W;   // 64 x 48 heatmaps
constexpr int SH_TAPS = 9, SH_SLAB = 16;                                            // 3 x 3 taps; output maps per workgroup (one MFMA tile of columns)

// PyTorch's align_corners = False source index of output row / column u over n source rows / columns at scale 4:
//   s = max((u + 0.5) / 4 - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, n - 1), l = s - i0 in {0, .125, .375, .625, .875}: exact in binary
SH_HD void sh_sample(int u, int n, int* i0, int* i1, float* l) {
    float s = ((float)u + 0.5f) * 0.25f - 0.5f;   // every operand and result a multiple of 1 / 8 below 2^7: exact
    s = s < 0.f ? 0.f : s;
    const int f = (int)s;
    *i0 = f;
    *i1 = f + 1 < n ? f + 1 : n - 1;
    *l = s - (float)f;
}

// the zero rule: a tap's sample position (yy, xx) = (y + ky - 1, x + kx - 1) contributes only inside the 64 x 48 map
SH_HD bool sh_inside(int yy, int xx) { return (unsigned)yy < (unsigned)SH_HM_H && (unsigned)xx < (unsigned)SH_HM_W; }

SH_HD float sh_lerp(float a, float b, float l) { return __builtin_fmaf(l, b - a, a); }

// rows of one tap's weight matrix for K maps (== weights.hip final_rows), and element (tap t, map k, lo plane?, channel d) of the image
SH_HD size_t sh_rows(size_t K) { return (K + SH_SLAB - 1) / SH_SLAB * 2 * SH_SLAB; }
SH_HD size_t sh_weight_index(int t, int k, int lo, int d, size_t rows, int D) {
    return ((size_t)t * rows + (size_t)(k / SH_SLAB) * 2 * SH_SLAB + (size_t)(k % SH_SLAB) + (lo ? SH_SLAB : 0)) * (size_t)D + (size_t)d;
}
// final_layer.weight [K, D, 3, 3] element (k, d, ky, kx)
SH_HD size_t sh_source_index(int k, int d, int ky, int kx, int D) { return (((size_t)k * D + d) * 3 + ky) * 3 + kx; }

// algorithmic work of the commuted form for n crops: the tap GEMM and the 36-term stencil; bytes = tokens + weight image + bias + heatmaps
SH_HD double sh_flops(int n, int K, int D) { return 2.0 * SH_TOKENS * n * (double)SH_TAPS * K * D + 2.0 * 36.0 * n * (double)K * SH_HM_H * SH_HM_W; }
SH_HD double sh_bytes(int n, int K, int D) {
    return 2.0 * SH_TOKENS * n * (double)D + 2.0 * SH_TAPS * (double)sh_rows(K) * D + 4.0 * K + 4.0 * n * (double)K * SH_HM_H * SH_HM_W;
}

}  // namespace vp
