// HBM-bound helpers of the ViTPose path: patch gather (im2col) and LayerNorm.
#include "common.h"
#include "kernels.h"
#include "pixfmt.h"
#include "../../include/vitpose_hip.h"

namespace vp {

// ------------------------------------------------------------------ im2col
// PatchEmbed = Conv2d(3, D, k=16, s=16, padding=2) (vit.py:222): patch (py,px) covers
// rows 16py-2 .. 16py+13, cols 16px-2 .. 16px+13 of the 256x192 crop, zero outside.
// Row m = b*192 + py*12 + px of the patch matrix, column k = c*256 + ky*16 + kx
// (the flattening of the conv weight [D,3,16,16]).
// One block = one patch row (b, py): its input is 3 x 16 whole image rows (read as contiguous
// 16-byte pieces), its output 12 consecutive rows of the patch matrix (18 KiB contiguous); the
// transposition in between goes through LDS, so that both HBM sides are fully coalesced (the
// thread-per-output-chunk version fetched 2.1x the algorithmic bytes: 64-byte pieces of 128-byte lines).
// FLIP: the crop is mirrored left-right on the fly (flip-test, topdown_heatmap_simple_head.py:195-218).
template <class Ty, int FMT, bool FLIP>
__global__ __launch_bounds__(256) void im2col_kernel(const void* __restrict__ in, uint16_t* __restrict__ out, int B, int n_src) {
    constexpr int XS = 208;                                  // LDS row: x = -2 .. 205 (index x + 2)
    __shared__ __attribute__((aligned(16))) uint16_t tile[3 * 16 * XS];
    const int tid = threadIdx.x;
    const int bo = blockIdx.x >> 4, py = blockIdx.x & 15;    // output crop bo reads source crop min(bo, n_src - 1): the rows of a padded encoder batch (forward.hip forward_chunk) repeat the last crop
    const int b = min(bo, n_src - 1);
    const int ytop = 16 * py - 2;
    if (FMT == VP_INPUT_F32_NCHW) {
        // 3 channels x 16 rows x 48 float4
        for (int id = tid; id < 3 * 16 * 48; id += 256) {
            const int x4 = id % 48, ky = (id / 48) & 15, c = id / (48 * 16);
            const int y = ytop + ky;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if ((unsigned)y < 256u) v = *(const f32x4*)((const float*)in + (((size_t)b * 3 + c) * 256 + y) * 192 + x4 * 4);
            if (FLIP) {   // pixel x of the source row lands at x' = 191 - x
                uint32_t* dst = (uint32_t*)(tile + (c * 16 + ky) * XS + (188 - x4 * 4) + 2);
                dst[0] = pack2<Ty>(v[3], v[2]);
                dst[1] = pack2<Ty>(v[1], v[0]);
            } else {
                uint32_t* dst = (uint32_t*)(tile + (c * 16 + ky) * XS + x4 * 4 + 2);
                dst[0] = pack2<Ty>(v[0], v[1]);
                dst[1] = pack2<Ty>(v[2], v[3]);
            }
        }
    } else {
        // 16 rows x 576 bytes (192 px x RGB) as 36 16-byte pieces per row
        for (int id = tid; id < 16 * 36; id += 256) {
            const int q = id % 36, ky = id / 36;
            const int y = ytop + ky;
            u32x4 raw = u32x4{0, 0, 0, 0};
            const bool inside = (unsigned)y < 256u;
            if (inside) raw = *(const u32x4*)((const uint8_t*)in + ((size_t)b * 256 + y) * 576 + q * 16);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int off = q * 16 + e, x = off / 3, c = off - x * 3;
                // pre_img (easy_ViTPose/inference.py:316-317): float64 x/255, (x-MEAN)/STD, cast to fp32
                const double mean = c == 0 ? 0.485 : (c == 1 ? 0.456 : 0.406);
                const double stdv = c == 0 ? 0.229 : (c == 1 ? 0.224 : 0.225);
                const uint8_t u = (uint8_t)(raw[e >> 2] >> ((e & 3) * 8));
                const float f = inside ? (float)(((double)u / 255.0 - mean) / stdv) : 0.f;
                tile[(c * 16 + ky) * XS + (FLIP ? 191 - x : x) + 2] = to_bits<Ty>(f);
            }
        }
    }
    if (tid < 96) {   // left zero border (x = -2, -1) of every (c, ky) row
        tile[(tid >> 1) * XS + (tid & 1)] = 0;
    }
    __syncthreads();
    uint16_t* orow = out + ((size_t)bo * 192 + py * 12) * 768;
    for (int id = tid; id < 12 * 96; id += 256) {
        const int px = id / 96, kc = id - px * 96;
        const int c = kc >> 5, ky = (kc & 31) >> 1, kx0 = (kc & 1) * 8;
        *(u32x4*)(orow + (size_t)id * 8) = *(const u32x4*)(tile + (c * 16 + ky) * XS + 16 * px + kx0);
    }
}

hipError_t im2col_launch(int dtype, const void* crops, int fmt, uint16_t* out, int B, hipStream_t s, bool flip, int n_src) {
    if (B <= 0) return hipSuccess;
    if (n_src <= 0 || n_src > B) n_src = B;   // B output crops from n_src source crops (the last one repeated)
    const int grid = B * 16;   // one block per patch row
#define VP_I2C(TY, F)                                                                                              \
    do {                                                                                                           \
        if (flip) hipLaunchKernelGGL((im2col_kernel<TY, F, true>), dim3(grid), dim3(256), 0, s, crops, out, B, n_src);    \
        else hipLaunchKernelGGL((im2col_kernel<TY, F, false>), dim3(grid), dim3(256), 0, s, crops, out, B, n_src);        \
    } while (0)
    if (fmt == VP_INPUT_F32_NCHW) {
        if (dtype == DT_F16) VP_I2C(F16, VP_INPUT_F32_NCHW); else VP_I2C(BF16, VP_INPUT_F32_NCHW);
    } else if (fmt == VP_INPUT_U8_NHWC) {
        if (dtype == DT_F16) VP_I2C(F16, VP_INPUT_U8_NHWC); else VP_I2C(BF16, VP_INPUT_U8_NHWC);
    } else {
        return hipErrorInvalidValue;
    }
#undef VP_I2C
    return hipGetLastError();
}

// ------------------------------------------------------- flip-test twin gather
// Flip-test mode (vp_set_flip_test): the patch rows of n crops AND of their mirror images in one launch, interleaved -- output crop 2i is
// crop i, output crop 2i + 1 its mirror (bit for bit the FLIP path above).  One block = one patch row (py) of one PAIR: the 3 x 16 source
// rows are read from HBM once, converted once and laid into LDS the straight way; the straight output reads them as im2col_kernel does,
// the mirrored output reads the same tile backwards (output column xo = source column 191 - xo; the conv's zero border of the mirror
// image lies at source columns 192, 193).  Output rows beyond 2 n_src (a padded encoder batch) repeat the last one, 2 n_src - 1.
__host__ __device__ inline void flip_twin_source(int bo, int n_src, int* src, int* mirror) {   // output crop bo of the interleaved batch
    const int r = bo < 2 * n_src - 1 ? bo : 2 * n_src - 1;
    *src = r >> 1;
    *mirror = r & 1;
}

template <class Ty, int FMT>
__global__ __launch_bounds__(256) void im2col_twin_kernel(const void* __restrict__ in, uint16_t* __restrict__ out, int B, int n_src) {
    constexpr int XS = 208;                                  // LDS row: x = -2 .. 205 (index x + 2)
    __shared__ __attribute__((aligned(16))) uint16_t tile[3 * 16 * XS];
    const int tid = threadIdx.x;
    const int pair = blockIdx.x >> 4, py = blockIdx.x & 15;
    int b, m0, b1, m1;
    flip_twin_source(2 * pair, n_src, &b, &m0);              // both output crops of a pair read the same source crop
    flip_twin_source(2 * pair + 1, n_src, &b1, &m1);
    const int ytop = 16 * py - 2;
    if (FMT == VP_INPUT_F32_NCHW) {
        for (int id = tid; id < 3 * 16 * 48; id += 256) {
            const int x4 = id % 48, ky = (id / 48) & 15, c = id / (48 * 16);
            const int y = ytop + ky;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if ((unsigned)y < 256u) v = *(const f32x4*)((const float*)in + (((size_t)b * 3 + c) * 256 + y) * 192 + x4 * 4);
            uint32_t* dst = (uint32_t*)(tile + (c * 16 + ky) * XS + x4 * 4 + 2);
            dst[0] = pack2<Ty>(v[0], v[1]);
            dst[1] = pack2<Ty>(v[2], v[3]);
        }
    } else {
        for (int id = tid; id < 16 * 36; id += 256) {
            const int q = id % 36, ky = id / 36;
            const int y = ytop + ky;
            u32x4 raw = u32x4{0, 0, 0, 0};
            const bool inside = (unsigned)y < 256u;
            if (inside) raw = *(const u32x4*)((const uint8_t*)in + ((size_t)b * 256 + y) * 576 + q * 16);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int off = q * 16 + e, x = off / 3, c = off - x * 3;
                const double mean = c == 0 ? 0.485 : (c == 1 ? 0.456 : 0.406);   // pre_img, as im2col_kernel
                const double stdv = c == 0 ? 0.229 : (c == 1 ? 0.224 : 0.225);
                const uint8_t u = (uint8_t)(raw[e >> 2] >> ((e & 3) * 8));
                const float f = inside ? (float)(((double)u / 255.0 - mean) / stdv) : 0.f;
                tile[(c * 16 + ky) * XS + x + 2] = to_bits<Ty>(f);
            }
        }
    }
    if (tid < 192) {   // zero border of every (c, ky) row: x = -2, -1 (the straight crop's left) and x = 192, 193 (the mirror's left)
        const int r = tid >> 2, j = tid & 3;
        tile[r * XS + (j < 2 ? j : 192 + j)] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int bo = 2 * pair + half;
        if (bo >= B) break;
        const bool mirror = half ? m1 != 0 : m0 != 0;
        uint16_t* orow = out + ((size_t)bo * 192 + py * 12) * 768;
        for (int id = tid; id < 12 * 96; id += 256) {
            const int px = id / 96, kc = id - px * 96;
            const int c = kc >> 5, ky = (kc & 31) >> 1, kx0 = (kc & 1) * 8;
            const uint16_t* row = tile + (c * 16 + ky) * XS;
            u32x4 v;
            if (!mirror) {
                v = *(const u32x4*)(row + 16 * px + kx0);
            } else {   // output columns xo .. xo + 7 = LDS elements 195 - xo' .. 188 - xo' (xo' = 16 px + kx0), an 8-byte aligned run read upwards and reversed
                const uint32_t* q = (const uint32_t*)(row + 188 - 16 * px - kx0);
                const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
                v = u32x4{(w3 >> 16) | (w3 << 16), (w2 >> 16) | (w2 << 16), (w1 >> 16) | (w1 << 16), (w0 >> 16) | (w0 << 16)};
            }
            *(u32x4*)(orow + (size_t)id * 8) = v;
        }
    }
}

hipError_t im2col_twin_launch(int dtype, const void* crops, int fmt, uint16_t* out, int B, int n_src, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (n_src <= 0 || 2 * n_src > B) return hipErrorInvalidValue;   // B output crops: 2 n_src interleaved + padding
    const int grid = (B + 1) / 2 * 16;   // one block per patch row of a pair
#define VP_I2T(TY, F) hipLaunchKernelGGL((im2col_twin_kernel<TY, F>), dim3(grid), dim3(256), 0, s, crops, out, B, n_src)
    if (fmt == VP_INPUT_F32_NCHW) {
        if (dtype == DT_F16) VP_I2T(F16, VP_INPUT_F32_NCHW); else VP_I2T(BF16, VP_INPUT_F32_NCHW);
    } else if (fmt == VP_INPUT_U8_NHWC) {
        if (dtype == DT_F16) VP_I2T(F16, VP_INPUT_U8_NHWC); else VP_I2T(BF16, VP_INPUT_U8_NHWC);
    } else {
        return hipErrorInvalidValue;
    }
#undef VP_I2T
    return hipGetLastError();
}

void flip_twin_layout(int bo, int n_src, int* src, int* mirror) { flip_twin_source(bo, n_src, src, mirror); }

// ------------------------------------------------------------- flip-test merge
// hm[n][k][y][x] = 0.5 (hm[n][k][y][x] + back[n][k][y][x]),  back = flip_back(hm_flipped) (post_transforms.py:110-147:
// channels swapped by the mirror pairs, then reversed in x), optionally shifted right by one pixel
// (topdown_heatmap_simple_head.py:213-215, `shift_heatmap`); the average is what the flip-test consumer takes.
// crop n's maps start n * a_stride / n * b_stride floats behind hm / hm_flipped: K * 3072 for two tensors of their own (vp_infer_flip), 2 K * 3072 for the
// interleaved batch of the flip-test mode (hm_flipped = hm + K * 3072: the merged maps land in the straight crop's slot)
__global__ __launch_bounds__(256) void flip_merge_kernel(float* __restrict__ hm, const float* __restrict__ hm_flipped,
                                                         const int32_t* __restrict__ partner, int K, int shift, size_t total,
                                                         size_t a_stride, size_t b_stride) {
    for (size_t id = (size_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (size_t)gridDim.x * 256) {
        const int x = (int)(id % 48);
        const size_t row = id / 48;                    // (n*K + k)*64 + y
        const int y = (int)(row & 63);
        const size_t nk = row >> 6;
        const int k = (int)(nk % K);
        const size_t n = nk / K;
        int xs = x;                                    // column of the flipped-back map before the shift
        if (shift && x > 0) xs = x - 1;
        const float b = hm_flipped[n * b_stride + ((size_t)partner[k] * 64 + y) * 48 + (47 - xs)];
        float* a = hm + n * a_stride + ((size_t)k * 64 + y) * 48 + x;
        *a = 0.5f * (*a + b);
    }
}

hipError_t flip_merge_launch(float* hm, const float* hm_flipped, const int32_t* partner, int N, int K, int shift, hipStream_t s, int interleaved) {
    const size_t total = (size_t)N * K * 3072, stride = (size_t)K * 3072 * (interleaved ? 2 : 1);
    int grid = (int)((total + 255) / 256);
    if (grid > 16384) grid = 16384;
    if (total) hipLaunchKernelGGL(flip_merge_kernel, dim3(grid), dim3(256), 0, s, hm, hm_flipped, partner, K, shift, total, stride, stride);
    return hipGetLastError();
}

// ViTPose+ mixed batch: dst crop i = src crop idx[i] (crops in expert order).  16-byte pieces; blockIdx.y = destination crop
__global__ void gather_crops_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const int32_t* __restrict__ idx, size_t pieces) {
    const uint4* s = src + (size_t)idx[blockIdx.y] * pieces;
    uint4* d = dst + (size_t)blockIdx.y * pieces;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < pieces; j += (size_t)gridDim.x * blockDim.x) d[j] = s[j];
}

hipError_t gather_crops_launch(const void* src, void* dst, const int32_t* idx, int n, size_t crop_bytes, hipStream_t s) {
    if (crop_bytes % 16 || n < 0 || n > 65535) return hipErrorInvalidValue;
    if (n) hipLaunchKernelGGL(gather_crops_kernel, dim3(36, n), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, idx, crop_bytes / 16);
    return hipGetLastError();
}

// ViTPose+ chunk with per-crop experts: the call's tables from the kernel argument into the handle's device buffers (kernels.h MixTable).  One thread owns
// every value it writes; the launches of a chunk write disjoint positions, so the order among them does not matter.
// TWIN (the per-expert flip-test mode, mix_tables_flip_launch): position j is forward rows 2 j and 2 j + 1 -- the ids are written per ROW (pad_to counts rows), the
// decode's four-field record goes to recs_flip, everything else stays per crop.
template <bool TWIN>
__global__ __launch_bounds__(MIX_CROPS_PER_LAUNCH) void mix_tables_kernel(MixTable t, int32_t* __restrict__ ids, int32_t* __restrict__ order,
                                                                        int32_t* __restrict__ slot, MixRec* __restrict__ recs, MixRecFlip* __restrict__ recs_flip) {
    const int i = threadIdx.x;
    if (i < t.count) {
        const int j = t.base + i;
        if (TWIN) { ids[2 * j] = t.id[i]; ids[2 * j + 1] = t.id[i]; }
        else ids[j] = t.id[i];
        order[j] = t.order[i];
        slot[t.order[i]] = j;
        MixRec r;
        r.first = t.first[i]; r.K = t.K[i]; r.dst = t.order[i];
        recs[j] = r;
        if (TWIN) {
            MixRecFlip f;
            f.first = t.first[i]; f.K = t.K[i]; f.dst = t.order[i]; f.e = t.id[i];
            recs_flip[j] = f;
        }
    }
    if (t.count > 0)
        for (int j = (TWIN ? 2 : 1) * (t.base + t.count) + i; j < t.pad_to; j += MIX_CROPS_PER_LAUNCH) ids[j] = t.id[t.count - 1];
}

hipError_t mix_tables_launch(const MixTable& t, int32_t* ids, int32_t* order, int32_t* slot, MixRec* recs, hipStream_t s) {
    if (t.count < 0 || t.count > MIX_CROPS_PER_LAUNCH || t.base < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mix_tables_kernel<false>, dim3(1), dim3(MIX_CROPS_PER_LAUNCH), 0, s, t, ids, order, slot, recs, (MixRecFlip*)nullptr);
    return hipGetLastError();
}

hipError_t mix_tables_flip_launch(const MixTable& t, int32_t* ids, int32_t* order, int32_t* slot, MixRec* recs, MixRecFlip* recs_flip, hipStream_t s) {
    if (t.count < 0 || t.count > MIX_CROPS_PER_LAUNCH || t.base < 0 || !recs_flip) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mix_tables_kernel<true>, dim3(1), dim3(MIX_CROPS_PER_LAUNCH), 0, s, t, ids, order, slot, recs, recs_flip);
    return hipGetLastError();
}

// --------------------------------------------------------------- LayerNorm
// nn.LayerNorm(eps=1e-6) (vit.py:274) over the fp32 residual stream, one wave per
// token row, row held in registers (D <= 1280 -> <= 5 float4 per lane), two-pass
// mean / variance in fp32, output rounded once to the GEMM operand type.
// PLANES: x is the two-plane 16-bit residual stream of the fused-LayerNorm path (x = hi + lo, gemm.hip).
template <class Ty, bool PLANES>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, uint16_t* __restrict__ out16,
                                                        float* __restrict__ out32, int M, int D, size_t plane) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nv = D >> 2;
    const f32x4* xr = (const f32x4*)(x + (size_t)row * D);
    f32x4 v[5];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int idx = lane + 64 * i;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (idx < nv) {
            if constexpr (PLANES) {
                const uint16_t* xh = (const uint16_t*)x + (size_t)row * D;
                const u32x2 h = ((const u32x2*)xh)[idx], l = ((const u32x2*)(xh + plane))[idx];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int sh = (e & 1) * 16;
                    v[i][e] = from_bits<Ty>((uint16_t)(h[e >> 1] >> sh)) + from_bits<Ty>((uint16_t)(l[e >> 1] >> sh));
                }
            } else {
                v[i] = xr[idx];
            }
            sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    const float mean = wave_sum(sum) / (float)D;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int idx = lane + 64 * i;
        if (idx < nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[i][e] - mean;
                sq += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)D + 1e-6f);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int idx = lane + 64 * i;
        if (idx < nv) {
            const f32x4 g = ((const f32x4*)gamma)[idx];
            const f32x4 b = ((const f32x4*)beta)[idx];
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * rstd * g[e] + b[e];
            if (out16) {
                u32x2 o;
                o[0] = pack2<Ty>(y[0], y[1]);
                o[1] = pack2<Ty>(y[2], y[3]);
                ((u32x2*)(out16 + (size_t)row * D))[idx] = o;
            }
            if (out32) ((f32x4*)(out32 + (size_t)row * D))[idx] = y;
        }
    }
}

hipError_t layernorm_launch(int dtype, const float* x, const float* gamma, const float* beta, uint16_t* out16,
                            float* out32, int M, int D, hipStream_t s, size_t plane) {
    if ((D & 3) || D > 1280) return hipErrorInvalidValue;
    const int grid = (M + 3) / 4;
#define VP_LN(TY, PL) hipLaunchKernelGGL((layernorm_kernel<TY, PL>), dim3(grid), dim3(256), 0, s, x, gamma, beta, out16, out32, M, D, plane)
    if (dtype == DT_F16) { if (plane) VP_LN(F16, true); else VP_LN(F16, false); }
    else { if (plane) VP_LN(BF16, true); else VP_LN(BF16, false); }
#undef VP_LN
    return hipGetLastError();
}

// Fused-LayerNorm helper: the residual GEMMs leave, per token row and 64-column granule, (sum, M2 about the
// granule mean).  Fold them in a FIXED order (deterministic, unlike atomics) into (mean, rstd) per row with the
// pairwise-merge identity  M2 = sum_g [M2_g + 64 (mean_g - mean)^2]  -- no E[x^2] - mean^2 cancellation.
__global__ __launch_bounds__(256) void ln_finalize_kernel(const float* __restrict__ partials, float* __restrict__ rowstat,
                                                          int M, int tiles, float inv_d) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float mean, rstd;
    ln_merge(partials + (size_t)m * tiles * 2, tiles, inv_d, mean, rstd);
    rowstat[2 * (size_t)m] = mean;
    rowstat[2 * (size_t)m + 1] = rstd;
}

// Round 5: the same merge with a row's partials fetched UP FRONT as 16-byte loads (one memory latency instead of 2 x tiles dependent 4-byte loads 8 bytes
// apart) and 64-thread workgroups (768 instead of 192 at 256 crops: every CU takes part).  ln_merge runs on the register copy: the same operations in the same
// order, hence the same bits (the kernel sits between every residual GEMM and its consumer: 24 launches per ViTPose-B forward, 64 per ViTPose-H).
template <int TILES>
__global__ __launch_bounds__(64) void ln_finalize_kernel_t(const float* __restrict__ partials, float* __restrict__ rowstat, int M, float inv_d) {
    static_assert(TILES % 2 == 0, "a row of partials is a whole number of 16-byte pieces");
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= M) return;
    const f32x4* src = (const f32x4*)(partials + (size_t)m * TILES * 2);
    float v[2 * TILES];
#pragma unroll
    for (int i = 0; i < TILES / 2; ++i) {
        const f32x4 q = src[i];
        v[4 * i] = q[0]; v[4 * i + 1] = q[1]; v[4 * i + 2] = q[2]; v[4 * i + 3] = q[3];
    }
    float mean, rstd;
    ln_merge(v, TILES, inv_d, mean, rstd);
    *(float2*)(rowstat + 2 * (size_t)m) = float2{mean, rstd};
}

// Split-K reduction of a residual GEMM (round 6, small batches; gemm.hip EPI_PARTIAL): the S fp32 partial products of every output element are added in the
// FIXED order s = 0 .. S - 1 (run-to-run deterministic; no atomics); st = sum + bias then goes through the producer row of common.h (planes_decode8,
// planes_split8, granule_stats8) like the EPI_BIAS_RESID_LN epilogue's.  One 8-column chunk per thread; every load of a thread is issued before the first add.
template <class T, int SMAX>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int S, const float* __restrict__ bias, uint16_t* __restrict__ x_hi,
                                                            size_t plane, float* __restrict__ stats_out, int M, int N) {
    const int cpr = N >> 3;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = c < (size_t)M * cpr;
    const int m = ok ? (int)(c / cpr) : 0, ch = ok ? (int)(c - (size_t)m * cpr) : 0;
    const size_t off = (size_t)m * N + ch * 8, slab = (size_t)M * N;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (ok) {
        f32x4 p0[SMAX], p1[SMAX];
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
            if (s < S) {
                p0[s] = *(const f32x4*)(part + s * slab + off);
                p1[s] = *(const f32x4*)(part + s * slab + off + 4);
            }
        const u32x4 ra = *(const u32x4*)(x_hi + off), rb = *(const u32x4*)(x_hi + plane + off);
        const f32x4 b0 = *(const f32x4*)(bias + ch * 8), b1 = *(const f32x4*)(bias + ch * 8 + 4);
        f32x4 a0 = p0[0], a1 = p1[0];
#pragma unroll
        for (int s = 1; s < SMAX; ++s)
            if (s < S) { a0 += p0[s]; a1 += p1[s]; }
        a0 += b0; a1 += b1;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (e < 4 ? a0[e] : a1[e - 4]) + planes_decode8<T>(ra, rb, e);
        u32x4 oh, ol;
        planes_split8<T>(v, oh, ol);
        *(u32x4*)(x_hi + off) = oh;
        *(u32x4*)(x_hi + plane + off) = ol;
    }
    const float2 gs = granule_stats8(v);
    if (ok && (ch & 7) == 0) *(float2*)(stats_out + ((size_t)m * (N >> 6) + (ch >> 3)) * 2) = gs;
}

hipError_t splitk_reduce_launch(int dtype, const float* partials, int S, const float* bias, uint16_t* x_hi, size_t plane, float* stats_out, int M, int N,
                                hipStream_t s) {
    if (S < 1 || S > 8 || N % 64 != 0 || M <= 0) return hipErrorInvalidValue;
    const size_t chunks = (size_t)M * (N / 8);
    const dim3 grid((unsigned)((chunks + 255) / 256)), block(256);
    if (dtype == DT_F16) {
        if (S <= 4) hipLaunchKernelGGL((splitk_reduce_kernel<F16, 4>), grid, block, 0, s, partials, S, bias, x_hi, plane, stats_out, M, N);
        else hipLaunchKernelGGL((splitk_reduce_kernel<F16, 8>), grid, block, 0, s, partials, S, bias, x_hi, plane, stats_out, M, N);
    } else {
        if (S <= 4) hipLaunchKernelGGL((splitk_reduce_kernel<BF16, 4>), grid, block, 0, s, partials, S, bias, x_hi, plane, stats_out, M, N);
        else hipLaunchKernelGGL((splitk_reduce_kernel<BF16, 8>), grid, block, 0, s, partials, S, bias, x_hi, plane, stats_out, M, N);
    }
    return hipGetLastError();
}

hipError_t ln_finalize_launch(const float* partials, float* rowstat, int M, int tiles, int D, hipStream_t s) {
    const float inv_d = 1.0f / (float)D;
    const dim3 grid((M + 63) / 64), block(64);
    switch (tiles) {   // D / 64 of ViTPose-S / -B / -L / -H; anything else: the generic kernel
        case 6: hipLaunchKernelGGL(ln_finalize_kernel_t<6>, grid, block, 0, s, partials, rowstat, M, inv_d); break;
        case 12: hipLaunchKernelGGL(ln_finalize_kernel_t<12>, grid, block, 0, s, partials, rowstat, M, inv_d); break;
        case 16: hipLaunchKernelGGL(ln_finalize_kernel_t<16>, grid, block, 0, s, partials, rowstat, M, inv_d); break;
        case 20: hipLaunchKernelGGL(ln_finalize_kernel_t<20>, grid, block, 0, s, partials, rowstat, M, inv_d); break;
        default: hipLaunchKernelGGL(ln_finalize_kernel, dim3((M + 255) / 256), dim3(256), 0, s, partials, rowstat, M, tiles, inv_d);
    }
    return hipGetLastError();
}

template <class Ty>
__global__ void fill_random16_kernel(uint16_t* p, size_t n, uint32_t seed) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        uint32_t h = (uint32_t)i * 2654435761u ^ seed;
        h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
        p[i] = to_bits<Ty>((float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f);
    }
}

hipError_t fill_random16(int dtype, uint16_t* p, size_t n, uint32_t seed, hipStream_t s) {
    if (dtype == DT_F16) hipLaunchKernelGGL(fill_random16_kernel<F16>, dim3(2048), dim3(256), 0, s, p, n, seed);
    else hipLaunchKernelGGL(fill_random16_kernel<BF16>, dim3(2048), dim3(256), 0, s, p, n, seed);
    return hipGetLastError();
}

}  // namespace vp

// ---------------------------------------------------------------------------
// Crop preparation on device: for every detected box, crop the frame, zero-pad to 3:4
// (pad_image, vit_utils/inference.py:41-70) and resize to 256x192 exactly as OpenCV's 8-bit INTER_LINEAR
// does (easy_ViTPose/inference.py:316): half-pixel centres, 11-bit fixed-point coefficients, int32
// horizontal pass, (((b0*(S0>>4))>>16)+((b1*(S1>>4))>>16)+2)>>2 vertical pass, 2x2 box average at exactly
// 2x.  Integer arithmetic -> bit-identical to easy_vitpose_amd/cropprep.py.  One block = one output row.
namespace vp {

struct AxisCoef { int s0, s1, a0, a1; };

__device__ __forceinline__ AxisCoef axis_coef(int d, int dsize, int ssize) {
    const double inv = (double)dsize / (double)ssize;
    const double scale = 1.0 / inv;
    float f = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
    int s = (int)floorf(f);
    f = __fsub_rn(f, (float)s);
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    AxisCoef c;
    c.s0 = s;
    c.s1 = min(s + 1, ssize - 1);
    c.a1 = (int)rintf(__fmul_rn(f, 2048.f));
    c.a0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
    return c;
}

// One output pixel of crop record r whose frame is in format FMT.  fetch = the RGB8 value of a padded-canvas pixel: the SOURCE pixel converted once
// (pixfmt.h), zero outside the crop; both interpolation branches then run on RGB exactly as they did when RGB24 was the only format.
template <int FMT> __device__ __forceinline__ void crop_pixel(const CropRec& r, int oy, int ox, uint8_t* __restrict__ dst) {
    const uint8_t* __restrict__ src = r.src;
    const uint8_t* __restrict__ src1 = r.src1;
    const int cw = r.cw, ch = r.ch, left = r.left, top = r.top, pw = r.pw, ph = r.ph;
    const YuvCoef k = yuv_coef(FMT == PIX_NV12 ? r.matrix : 0);
    auto fetch = [&](int Y, int X, int* rgb) {   // padded-canvas pixel
        const int yy = Y - top, xx = X - left;
        if ((unsigned)yy >= (unsigned)ch || (unsigned)xx >= (unsigned)cw) { rgb[0] = rgb[1] = rgb[2] = 0; return; }
        if (FMT == PIX_NV12) {
            const uint8_t* uv = src1 + (size_t)((r.oy + yy) >> 1) * r.pitch1 + (size_t)((r.ox + xx) >> 1) * 2;
            yuv_to_rgb(k, src[(size_t)yy * r.pitch + (size_t)xx], uv[0], uv[1], rgb);
            return;
        }
        const uint8_t* p = src + (size_t)yy * r.pitch + (size_t)xx * 3;
        rgb[0] = p[FMT == PIX_BGR24 ? 2 : 0]; rgb[1] = p[1]; rgb[2] = p[FMT == PIX_BGR24 ? 0 : 2];
    };
    int p00[3], p01[3], p10[3], p11[3];
    if (pw == 384 && ph == 512) {                 // exactly 2x: OpenCV's INTER_LINEAR == fast INTER_AREA
        fetch(2 * oy, 2 * ox, p00); fetch(2 * oy, 2 * ox + 1, p01); fetch(2 * oy + 1, 2 * ox, p10); fetch(2 * oy + 1, 2 * ox + 1, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)((p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2);
        return;
    }
    const AxisCoef cx = axis_coef(ox, 192, pw), cy = axis_coef(oy, 256, ph);
    fetch(cy.s0, cx.s0, p00); fetch(cy.s0, cx.s1, p01); fetch(cy.s1, cx.s0, p10); fetch(cy.s1, cx.s1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int r0 = p00[c] * cx.a0 + p01[c] * cx.a1;
        const int r1 = p10[c] * cx.a0 + p11[c] * cx.a1;
        dst[c] = (uint8_t)((((cy.a0 * (r0 >> 4)) >> 16) + ((cy.a1 * (r1 >> 4)) >> 16) + 2) >> 2);
    }
}

__global__ __launch_bounds__(192) void crop_resize_kernel(const CropRec* __restrict__ recs, uint8_t* __restrict__ out) {
    const int crop = blockIdx.x >> 8, oy = blockIdx.x & 255, ox = threadIdx.x;
    const CropRec r = recs[crop];   // each crop its own source (band or device frame), pitch and format: one kernel for one or many frames
    uint8_t* dst = out + (((size_t)crop * 256 + oy) * 192 + ox) * 3;
    if (r.format == PIX_RGB24) crop_pixel<PIX_RGB24>(r, oy, ox, dst);   // block-uniform: a launch may hold records of several formats
    else if (r.format == PIX_NV12) crop_pixel<PIX_NV12>(r, oy, ox, dst);
    else crop_pixel<PIX_BGR24>(r, oy, ox, dst);
}

hipError_t crop_resize_launch(const CropRec* recs, uint8_t* out, int n, hipStream_t s) {
    hipLaunchKernelGGL(crop_resize_kernel, dim3(n * 256), dim3(192), 0, s, recs, out);
    return hipGetLastError();
}

}  // namespace vp
