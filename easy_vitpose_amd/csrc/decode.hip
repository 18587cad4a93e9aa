// Heatmap decode: keypoints_from_heatmaps(unbiased=True, use_udp=True) + postprocess
// (vit_utils/top_down_eval.py:493-641, easy_ViTPose/inference.py:187-205), with the
// reference's one-crop-at-a-time semantics (VitInference calls it with N == 1).
//
// HBM-bound: the only full read is one coalesced float4 sweep of each 64x48 map for
// the arg-max (first index wins ties, top_down_eval.py:106).  The DARK refinement
// (post_dark_udp, :354-415) needs the 11x11 Gaussian-blurred, clipped, log'ed map at
// only 7 positions around the arg-max, so instead of blurring 3072 pixels per joint
// (what the reference's N*K cv2.GaussianBlur calls do) the block evaluates those 7
// samples directly from the raw map (the re-read hits L2): 7 x 11 row sums
// (horizontal pass, fp32 like OpenCV's intermediate), then 7 column sums.
// The sample positions follow the reference's flat index arithmetic into the
// edge-padded map exactly -- including the wrap-around of negative indices that
// numpy fancy indexing performs when coords are -1 (max <= 0).
#include "common.h"
#include "kernels.h"

namespace vp {

static constexpr int HH = 64, WW = 48, HW = HH * WW;
static constexpr int PADSZ = (HH + 2) * (WW + 2);   // 3300

__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

struct GaussK { float w[11]; };

// FLIP (flip-test mode, vp_set_flip_test): hm is the interleaved batch [2 N, K, 64, 48] -- crop n at 2 n, its mirror image at 2 n + 1 -- and the map the block
// decodes is 0.5 (crop's map k + flip_back(mirror's map partner[k])), formed in registers wherever the plain kernel loads a value: the same fp32 add and exact
// multiply as flip_merge_kernel and the same summation orders below, so the result equals flip_merge + decode bit for bit while the merged tensor is never
// written.  flip_back = x reversed (column x reads 47 - x; with `shift`, column x > 0 reads 48 - x and column 0 keeps 47): a reversed 192-byte row is the same
// one or two cache lines, read as one aligned 16-byte load (+ one scalar under `shift`) and swizzled in registers.
//
// MIX (a ViTPose+ chunk with per-crop experts, decode_mix_launch): the grid is [N, Kmax] and the crop at position n of the chunk's expert order brings its own
// record -- where its maps start, how many joints its expert has, which row of the caller's order it is.  Blocks k < K_e run the code below on exactly the values the
// plain kernel sees for that crop as a [1, K_e, 64, 48] batch (the record only replaces the three index expressions n K + k, n and blockIdx.x), so the bits are the plain
// kernel's; blocks k >= K_e write the zeros of the padded row.  FLIP and MIX are compile-time: decode_kernel<false, false> keeps the instruction stream it had.
//
// FLIP and MIX (the per-expert flip-test mode, decode_flip_mix_launch): `recs` holds MixRecFlip records, `partner` the [n_experts, Kmax] table.  The crop's K_e maps
// start at `first`, its mirror's at first + K_e (a [2, K_e, 64, 48] pair), and the mirror is read through row e of the table: the FLIP body on the values it sees
// for that pair under expert e's table, so the bits are decode_kernel<true, false>'s.  The three other instantiations keep their instruction streams.
//
// AFF (the affine crop route, decode_affine_launch / decode_affine_flip_launch; never with MIX): `org_wh` carries float32 cs[row] = (cx, cy, S_w, S_h) instead of integer
// sizes, and the last thread writes FRAME pixels with one rounding, transform_preds(center, scale, use_udp=True) on the box's own centre and scale:
// x = (float)(rx (S_w / 47) + cx - S_w 0.5) in fp64, every step unfused (so a host restatement in numpy has the same bits), y with 63 and S_h.  A row whose
// S_w is not > 0 is a refused box: all zero.  AFF is compile-time too: the four instantiations without it keep their instruction streams.
template <bool FLIP, bool MIX, bool AFF = false>
__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ hm, const int32_t* __restrict__ org_wh,
                                                     float* __restrict__ out, int K, GaussK gk, const int32_t* __restrict__ partner, int shift,
                                                     const MixRec* __restrict__ recs) {
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    __shared__ float s_part[7][11];
    __shared__ float s_samp[7];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x / K, k = blockIdx.x % K;
    int first = 0, row = n;   // MIX: the crop's first map, and its row in org_wh / out
    if (MIX && FLIP) {
        const MixRecFlip r = ((const MixRecFlip*)recs)[n];
        row = r.dst;
        if (k >= r.K) {
            if (tid < 3) out[((size_t)row * K + k) * 3 + tid] = 0.f;
            return;
        }
        out += ((size_t)row * K + k) * 3;
        partner += (size_t)r.e * K;   // the expert's row of the [n_experts, Kmax] table
        first = r.first;
        K = r.K;
    } else if (MIX) {
        const MixRec r = recs[n];
        row = r.dst;
        if (k >= r.K) {   // a joint this crop's expert does not have (the whole block leaves: no barrier was reached yet)
            if (tid < 3) out[((size_t)row * K + k) * 3 + tid] = 0.f;
            return;
        }
        out += ((size_t)row * K + k) * 3;   // K is still Kmax here: the output rows' stride
        first = r.first;
        K = r.K;
    }
    const float* map = hm + (MIX ? (size_t)first + k : FLIP ? (size_t)2 * n * K + k : (size_t)blockIdx.x) * HW;
    const float* mir = FLIP ? hm + (MIX ? (size_t)first + K + partner[k] : (size_t)(2 * n + 1) * K + partner[k]) * HW : nullptr;

    // ---- arg-max / max over 3072 values, first index on ties (_get_max_preds, :82-114)
    float best = -INFINITY;
    int bidx = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int v4 = tid + 256 * i;
        f32x4 v = ((const f32x4*)map)[v4];
        if (FLIP) {   // columns x0 .. x0 + 3 of row y average with the mirror's columns 47 - x0 .. 44 - x0 (shift: 48 - x0 .. 45 - x0, column 0 with 47)
            const int y = v4 / 12, x0 = (v4 - y * 12) * 4;
            const float* mrow = mir + y * WW;
            const f32x4 r = *(const f32x4*)(mrow + 44 - x0);
            f32x4 b = f32x4{r[3], r[2], r[1], r[0]};
            if (shift) b = f32x4{x0 ? mrow[48 - x0] : r[3], r[3], r[2], r[1]};
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = 0.5f * (v[e] + b[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v[e] > best || bidx == 0x7fffffff) { best = v[e]; bidx = v4 * 4 + e; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
    }
    if (lane == 0) { s_val[wave] = best; s_idx[wave] = bidx; }
    __syncthreads();
    best = s_val[0]; bidx = s_idx[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float ov = s_val[w];
        const int oi = s_idx[w];
        if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
    }
    const float maxval = best;
    const float cx = maxval > 0.f ? (float)(bidx % WW) : -1.f;
    const float cy = maxval > 0.f ? (float)(bidx / WW) : -1.f;

    // ---- 7 samples of log(clip(blur(map))) at the reference's flat padded indices (:389-402)
    // order: i_, ix1, iy1, ix1y1, ix1_y1_, ix1_, iy1_
    if (tid < 77) {
        const int s = tid / 11, ty = tid % 11;
        const int offs[7] = {0, 1, WW + 2, WW + 3, -WW - 3, -1, -2 - WW};
        const int total = K * PADSZ;
        int f = (int)cx + 1 + ((int)cy + 1) * (WW + 2) + k * PADSZ + offs[s];
        f %= total;
        if (f < 0) f += total;                        // numpy negative-index wrap (per-crop array)
        const int kk = f / PADSZ, rem = f % PADSZ;
        int py = rem / (WW + 2) - 1, px = rem % (WW + 2) - 1;
        py = min(max(py, 0), HH - 1);                 // np.pad(mode='edge')
        px = min(max(px, 0), WW - 1);
        const int ry = reflect101(py + ty - 5, HH) * WW;
        const float* src = hm + (MIX ? (size_t)first + kk : (size_t)(FLIP ? 2 * n : n) * K + kk) * HW + ry;
        const float* msrc = FLIP ? hm + (MIX ? (size_t)first + K + partner[kk] : (size_t)(2 * n + 1) * K + partner[kk]) * HW + ry : nullptr;   // the neighbour map the samples wrap into, and ITS partner
        float acc = 0.f;
#pragma unroll
        for (int tx = 0; tx < 11; ++tx) {
            const int x = reflect101(px + tx - 5, WW);
            float v = src[x];
            if (FLIP) v = 0.5f * (v + msrc[47 - ((shift && x > 0) ? x - 1 : x)]);
            acc += gk.w[tx] * v;
        }
        s_part[s][ty] = acc;
    }
    __syncthreads();
    if (tid < 7) {
        float acc = 0.f;
#pragma unroll
        for (int ty = 0; ty < 11; ++ty) acc += gk.w[ty] * s_part[tid][ty];
        acc = fminf(fmaxf(acc, 0.001f), 50.f);       // np.clip(.., 0.001, 50)  :386
        s_samp[tid] = logf(acc);                     // np.log                  :387
    }
    __syncthreads();
    if (tid == 0) {
        const float i_ = s_samp[0], ix1 = s_samp[1], iy1 = s_samp[2], ix1y1 = s_samp[3];
        const float ix1_y1_ = s_samp[4], ix1_ = s_samp[5], iy1_ = s_samp[6];
        const float dx = 0.5f * (ix1 - ix1_);
        const float dy = 0.5f * (iy1 - iy1_);
        const float dxx = ix1 - 2.f * i_ + ix1_;
        const float dyy = iy1 - 2.f * i_ + iy1_;
        const float dxy = 0.5f * (ix1y1 - ix1 - iy1 + i_ + i_ - ix1_ - iy1_ + ix1_y1_);
        // inv(H + eps_f32 * I) in float64 (:411-413)
        const double eps = 1.1920928955078125e-07;
        const double a = (double)dxx + eps, b = (double)dxy, d = (double)dyy + eps;
        const double det = a * d - b * b;
        const double ox = (d * (double)dx - b * (double)dy) / det;
        const double oy = (-b * (double)dx + a * (double)dy) / det;
        const float rx = (float)((double)cx - ox);   // coords -= H^-1 d, stored back as float32 (:414)
        const float ry = (float)((double)cy - oy);
        // transform_preds(use_udp=True) with center = (w//2, h//2), scale = (w, h)
        // (post_transforms.py:183-192, inference.py:200-204), float64 then float32
        if (AFF) {
            const float* q = (const float*)org_wh + 4 * (size_t)n;
            const double sw = (double)q[2], sh = (double)q[3];
            float* o = out + (size_t)blockIdx.x * 3;
            if (!(q[2] > 0.f)) { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; return; }
            const double fx = __dsub_rn(__dadd_rn(__dmul_rn((double)rx, __ddiv_rn(sw, WW - 1.0)), (double)q[0]), __dmul_rn(sw, 0.5));
            const double fy = __dsub_rn(__dadd_rn(__dmul_rn((double)ry, __ddiv_rn(sh, HH - 1.0)), (double)q[1]), __dmul_rn(sh, 0.5));
            o[0] = (float)fy;
            o[1] = (float)fx;
            o[2] = maxval;
            return;
        }
        int ow = 192, oh = 256;
        if (org_wh) { ow = org_wh[2 * (MIX ? row : n)]; oh = org_wh[2 * (MIX ? row : n) + 1]; }
        const double fx = (double)rx * ((double)ow / (WW - 1.0)) + (double)(ow / 2) - (double)ow * 0.5;
        const double fy = (double)ry * ((double)oh / (HH - 1.0)) + (double)(oh / 2) - (double)oh * 0.5;
        float* o = MIX ? out : out + (size_t)blockIdx.x * 3;   // [n, K, 3] of the caller's crops in every mode
        o[0] = (float)fy;                            // (y, x, conf)  inference.py:205
        o[1] = (float)fx;
        o[2] = maxval;
    }
}

static GaussK gauss11() {
    // OpenCV getGaussianKernel(11, sigma<=0): sigma = 0.3*((11-1)*0.5-1)+0.8 = 2.0, float32 weights, sum 1
    GaussK gk;
    double w[11], sum = 0.0;
    for (int i = 0; i < 11; ++i) { w[i] = exp(-((i - 5.0) * (i - 5.0)) / (2.0 * 2.0 * 2.0)); sum += w[i]; }
    for (int i = 0; i < 11; ++i) gk.w[i] = (float)(w[i] / sum);
    return gk;
}

hipError_t decode_launch(const float* hm, const int32_t* org_wh, float* out, int N, int K, hipStream_t s) {
    hipLaunchKernelGGL((decode_kernel<false, false>), dim3(N * K), dim3(256), 0, s, hm, org_wh, out, K, gauss11(), (const int32_t*)nullptr, 0, (const MixRec*)nullptr);
    return hipGetLastError();
}

hipError_t decode_flip_launch(const float* hm, const int32_t* partner, int shift, const int32_t* org_wh, float* out, int N, int K, hipStream_t s) {
    if (!partner) return hipErrorInvalidValue;
    hipLaunchKernelGGL((decode_kernel<true, false>), dim3(N * K), dim3(256), 0, s, hm, org_wh, out, K, gauss11(), partner, shift, (const MixRec*)nullptr);
    return hipGetLastError();
}

hipError_t decode_mix_launch(const float* hm, const MixRec* recs, const int32_t* org_wh, float* out, int N, int Kmax, hipStream_t s) {
    if (!recs) return hipErrorInvalidValue;
    hipLaunchKernelGGL((decode_kernel<false, true>), dim3(N * Kmax), dim3(256), 0, s, hm, org_wh, out, Kmax, gauss11(), (const int32_t*)nullptr, 0, recs);
    return hipGetLastError();
}

hipError_t decode_flip_mix_launch(const float* hm, const MixRecFlip* recs, const int32_t* partners, int shift, const int32_t* org_wh, float* out, int N, int Kmax,
                                  hipStream_t s) {
    if (!recs || !partners) return hipErrorInvalidValue;
    hipLaunchKernelGGL((decode_kernel<true, true>), dim3(N * Kmax), dim3(256), 0, s, hm, org_wh, out, Kmax, gauss11(), partners, shift, (const MixRec*)recs);
    return hipGetLastError();
}

hipError_t decode_affine_launch(const float* hm, const float* cs, float* out, int N, int K, hipStream_t s) {
    if (!cs) return hipErrorInvalidValue;
    hipLaunchKernelGGL((decode_kernel<false, false, true>), dim3(N * K), dim3(256), 0, s, hm, (const int32_t*)cs, out, K, gauss11(), (const int32_t*)nullptr, 0, (const MixRec*)nullptr);
    return hipGetLastError();
}

hipError_t decode_affine_flip_launch(const float* hm, const int32_t* partner, int shift, const float* cs, float* out, int N, int K, hipStream_t s) {
    if (!cs || !partner) return hipErrorInvalidValue;
    hipLaunchKernelGGL((decode_kernel<true, false, true>), dim3(N * K), dim3(256), 0, s, hm, (const int32_t*)cs, out, K, gauss11(), partner, shift, (const MixRec*)nullptr);
    return hipGetLastError();
}

}  // namespace vp
