// vp_yolo_*: YOLOv8-detect as a stream-ordered device stage (the network, the plan, the load step and the decode: yologeom.h), its synchronous host twin, the
// host-only taps (plan, fold, decode) and the activation tap.  Five kernels: yolo_pack_kernel (the caller's 3-channel tensor to 8-channel NHWC), yolo_conv_kernel
// (every convolution: implicit GEMM on mfma_f32_16x16x32_f16, operands straight from global memory, no LDS), yolo_pool_kernel, yolo_up_kernel, yolo_decode_kernel.
// A forward is the plan's launches in order on the caller's stream: no atomics, no allocation, no copy, no synchronisation.
#include "api_internal.h"
#include "hoststage.h"
#include "stageobj.h"
#include "common.h"
#include "yologeom.h"

using namespace vpi;

struct vp_yolo : StageObj {
    vp_yolo_cfg cfg{};
    vp::YoloPlan plan;
    char* arena = nullptr;               // every internal buffer for max_images images, 256-byte aligned parts
    std::vector<size_t> buf_off;         // byte offset of buffer b in the arena (the two external buffers: unused)
    _Float16* w = nullptr;               // the weight images
    float* b = nullptr;                  // the biases
    size_t device_bytes = 0;
};

namespace vp {

constexpr int CONV_THREADS = 256, CONV_WAVES = 4, CONV_PIX = 32, CONV_CH = YOLO_TILE_N;   // a wave: 32 pixels x 32 output channels = 2 x 2 MFMA tiles
constexpr int EW_THREADS = 256;

struct ConvArgs {
    const _Float16* in;
    const _Float16* w;      // [rows_pad][cols_pad]
    const float* bias;      // [rows_pad]
    void* out;
    const _Float16* res;    // nullptr: none
    int M, H, W, Ho, Wo;    // M = images x Ho x Wo
    int cpt;                // 8-channel groups per tap = c_in / 8
    int steps;              // cols_pad / 32
    int cols_pad;
    int c_out, s, act;
    int in_off, in_stride, out_off, out_stride, res_off, res_stride;
};

// Implicit GEMM, roles swapped so that a lane ends with four consecutive CHANNELS of one pixel: the MFMA's A operand is the weight image (row = output channel
// lane & 15, k = 8 (lane >> 4) .. + 7), its B operand the gathered activations (col = pixel lane & 15, the same k), D[row = channel 4 (lane >> 4) + r][col = pixel].
// k runs (ky, kx, channel): with c_in a multiple of 8 the 8 consecutive k of a lane are 8 consecutive channels of one tap -- one 16-byte load from NHWC, one from
// the weight image.  The weight image is zero beyond the real rows and columns, so only the activation side is predicated: a tap outside the image, a pixel beyond
// M or a k group beyond the last tap contributes zero, and its address is never formed.
template <int KS, bool F32>
__global__ __launch_bounds__(CONV_THREADS) void yolo_conv_kernel(ConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * CONV_WAVES + wave) * CONV_PIX, n0 = blockIdx.y * CONV_CH;
    if (m0 >= a.M) return;   // wave-uniform; the kernel has no barrier
    constexpr int PAD = KS / 2;
    bool vm[2];
    int iy0[2], ix0[2];
    size_t img[2];
    const int hw = a.Ho * a.Wo;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int m = m0 + t * 16 + r;
        vm[t] = m < a.M;
        const int mm = vm[t] ? m : 0;
        const int bi = mm / hw, rem = mm - bi * hw, oy = rem / a.Wo, ox = rem - oy * a.Wo;
        iy0[t] = oy * a.s - PAD;
        ix0[t] = ox * a.s - PAD;
        img[t] = (size_t)bi * a.H * a.W;
    }
    const _Float16* wrow[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) wrow[u] = a.w + (size_t)(n0 + u * 16 + r) * a.cols_pad + g * 8;   // rows < rows_pad, columns < cols_pad: always inside the image
    f32x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    int c8 = g, tap = 0;
    while (c8 >= a.cpt) { c8 -= a.cpt; ++tap; }
    for (int step = 0; step < a.steps; ++step) {
        f16x8 wf[2], xf[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) wf[u] = *reinterpret_cast<const f16x8*>(wrow[u] + (size_t)step * 32);
        const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int iy = iy0[t] + ky, ix = ix0[t] + kx;
            xf[t] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (tap < KS * KS && vm[t] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                xf[t] = *reinterpret_cast<const f16x8*>(a.in + yolo_at(img[t] + (size_t)iy * a.W + ix, a.in_stride, a.in_off, c8 * 8));
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u], xf[t], acc[u][t], 0, 0, 0);
        c8 += 4;
        while (c8 >= a.cpt) { c8 -= a.cpt; ++tap; }
    }
    // epilogue: bias, SiLU, shortcut, one rounding
    const bool vec = ((a.out_off | a.out_stride) & 3) == 0 && (!a.res || ((a.res_off | a.res_stride) & 3) == 0);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (!vm[t]) continue;
        const size_t pix = (size_t)(m0 + t * 16 + r);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ch0 = n0 + u * 16 + g * 4;
            if (ch0 >= a.c_out) continue;
            const float4 bv = *reinterpret_cast<const float4*>(a.bias + ch0);   // the bias is padded to rows_pad
            float v[4] = {acc[u][t][0] + bv.x, acc[u][t][1] + bv.y, acc[u][t][2] + bv.z, acc[u][t][3] + bv.w};
            if (a.act) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = yolo_silu(v[i]);
            }
            const bool full = vec && ch0 + 4 <= a.c_out;
            if (a.res) {
                const _Float16* rp = a.res + yolo_at(pix, a.res_stride, a.res_off, ch0);
                if (full) {
                    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
                    const h4 q = *reinterpret_cast<const h4*>(rp);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] += (float)q[i];
                } else {
                    for (int i = 0; i < 4 && ch0 + i < a.c_out; ++i) v[i] += (float)rp[i];
                }
            }
            if constexpr (F32) {
                float* op = (float*)a.out + yolo_at(pix, a.out_stride, a.out_off, ch0);
                if (full) *reinterpret_cast<float4*>(op) = float4{v[0], v[1], v[2], v[3]};
                else
                    for (int i = 0; i < 4 && ch0 + i < a.c_out; ++i) op[i] = v[i];
            } else {
                _Float16* op = (_Float16*)a.out + yolo_at(pix, a.out_stride, a.out_off, ch0);
                if (full) {
                    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
                    *reinterpret_cast<h4*>(op) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
                } else {
                    for (int i = 0; i < 4 && ch0 + i < a.c_out; ++i) op[i] = (_Float16)v[i];
                }
            }
        }
    }
}

// the caller's [n, 3, H, W] (layout 0) or [n, H, W, 3] (layout 1) to [n, H, W, 8], channels 3..7 zero; one pixel per thread
__global__ __launch_bounds__(EW_THREADS) void yolo_pack_kernel(const _Float16* __restrict__ in, _Float16* __restrict__ out, int layout, int hw, size_t total) {
    const size_t p = (size_t)blockIdx.x * EW_THREADS + threadIdx.x;
    if (p >= total) return;
    f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (layout == 0) {
        const size_t bi = p / (size_t)hw, px = p - bi * (size_t)hw;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = in[(bi * 3 + ch) * (size_t)hw + px];
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = in[p * 3 + ch];
    }
    *reinterpret_cast<f16x8*>(out + yolo_at(p, 8, 0, 0)) = v;
}

// 5 x 5 max-pool, stride 1, pad 2 (padding never wins: taps outside the image are skipped); one (pixel, 8-channel group) per thread, in and out slices of one buffer
__global__ __launch_bounds__(EW_THREADS) void yolo_pool_kernel(const _Float16* __restrict__ buf, _Float16* __restrict__ outb, int H, int W, int groups, int stride, int in_off,
                                                               int out_off, size_t total) {
    const size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const int gq = (int)(i % (size_t)groups);
    const size_t p = i / (size_t)groups;
    const size_t hw = (size_t)H * W, bi = p / hw, rem = p - bi * hw;
    const int y = (int)(rem / (size_t)W), x = (int)(rem - (size_t)y * W);
    const int y_lo = y - 2 < 0 ? 0 : y - 2, y_hi = y + 2 > H - 1 ? H - 1 : y + 2, x_lo = x - 2 < 0 ? 0 : x - 2, x_hi = x + 2 > W - 1 ? W - 1 : x + 2;
    f16x8 m = *reinterpret_cast<const f16x8*>(buf + yolo_at(p, stride, in_off, gq * 8));
    for (int yy = y_lo; yy <= y_hi; ++yy)
        for (int xx = x_lo; xx <= x_hi; ++xx) {
            const f16x8 q = *reinterpret_cast<const f16x8*>(buf + yolo_at(bi * hw + (size_t)yy * W + xx, stride, in_off, gq * 8));
#pragma unroll
            for (int k = 0; k < 8; ++k) m[k] = q[k] > m[k] ? q[k] : m[k];
        }
    *reinterpret_cast<f16x8*>(outb + yolo_at(p, stride, out_off, gq * 8)) = m;
}

// nearest x 2: out (2h x 2w) pixel (y, x) = in pixel (y / 2, x / 2); one (output pixel, 8-channel group) per thread
__global__ __launch_bounds__(EW_THREADS) void yolo_up_kernel(const _Float16* __restrict__ in, _Float16* __restrict__ out, int h, int w, int groups, int in_stride, int in_off,
                                                             int out_stride, int out_off, size_t total) {
    const size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const int gq = (int)(i % (size_t)groups);
    const size_t p = i / (size_t)groups;
    const size_t ohw = (size_t)4 * h * w, bi = p / ohw, rem = p - bi * ohw;
    const int y = (int)(rem / (size_t)(2 * w)), x = (int)(rem - (size_t)y * (2 * w));
    const size_t src = bi * (size_t)h * w + (size_t)(y >> 1) * w + (x >> 1);
    *reinterpret_cast<f16x8*>(out + yolo_at(p, out_stride, out_off, gq * 8)) = *reinterpret_cast<const f16x8*>(in + yolo_at(src, in_stride, in_off, gq * 8));
}

template <typename T> __global__ __launch_bounds__(EW_THREADS) void yolo_decode_kernel(DecodeArgs d, T* __restrict__ head) {
    const size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x;
    const size_t per_img = (size_t)d.A * d.units;
    if (i >= per_img * (size_t)d.n_images) return;
    const size_t img = i / per_img, rem = i - img * per_img;
    // anchors run along the lanes (layout 0 stores coalesce), units outer
    const int unit = (int)(rem / (size_t)d.A), a = (int)(rem - (size_t)unit * d.A);
    yolo_decode_unit<T>(d, head, img, a, unit);
}

}  // namespace vp

namespace {

using vp::YoloPlan;

int cfg_check(const vp_yolo_cfg* cfg, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "yolo: " + m; return (int)VP_ERR_INVALID; };
    if (!cfg) return bad("null cfg");
    if (cfg->in_h < 32 || cfg->in_h > vp::YOLO_MAX_SIDE || cfg->in_h % 32 || cfg->in_w < 32 || cfg->in_w > vp::YOLO_MAX_SIDE || cfg->in_w % 32)
        return bad("input size " + std::to_string(cfg->in_h) + " x " + std::to_string(cfg->in_w) + ": multiples of 32 in 32.." + std::to_string(vp::YOLO_MAX_SIDE) + " expected");
    if (cfg->max_images < 1 || cfg->max_images > vp::YOLO_MAX_IMAGES) return bad("max_images = " + std::to_string(cfg->max_images) + " outside 1.." + std::to_string(vp::YOLO_MAX_IMAGES));
    if (cfg->input_layout != 0 && cfg->input_layout != 1) return bad("input_layout = " + std::to_string(cfg->input_layout) + " is neither 0 nor 1");
    if (cfg->head_dtype != VP_DET_F32 && cfg->head_dtype != VP_DET_F16) return bad("head_dtype = " + std::to_string(cfg->head_dtype) + " is neither VP_DET_F32 nor VP_DET_F16");
    if (cfg->head_layout != 0 && cfg->head_layout != 1) return bad("head_layout = " + std::to_string(cfg->head_layout) + " is neither 0 nor 1");
    return VP_OK;
}

// cfg + checkpoint -> plan (HOST ONLY); every refusal of the checkpoint's structure except the per-tensor shapes, which the fold reports
int make_plan(const vp_yolo_cfg* cfg, const vp_yolo_tensor* tensors, int n_tensors, vp::YoloTensors* tab, YoloPlan* plan, std::string* why) {
    if (int rc = cfg_check(cfg, why)) return rc;
    vp::YoloDims d;
    const std::string r = vp::yolo_read_dims(tensors, n_tensors, tab, &d);
    if (!r.empty()) { *why = "yolo: " + r; return VP_ERR_INVALID; }
    vp::yolo_plan(d, cfg->in_h, cfg->in_w, cfg->head_dtype, plan);
    return VP_OK;
}

// the weight images and biases of every convolution as the device holds them (HOST ONLY)
int fold_all(const vp::YoloTensors& tab, const YoloPlan& plan, std::vector<uint16_t>* w, std::vector<float>* b, std::string* why) {
    w->assign(plan.w_elems, 0);
    b->assign(plan.b_elems, 0.f);
    for (const vp::YoloConv& cv : plan.convs) {
        const std::string r = vp::yolo_fold(tab, cv, w->data() + cv.w_off, (size_t)cv.cols_pad, b->data() + cv.b_off);
        if (!r.empty()) { *why = "yolo: " + r; return VP_ERR_INVALID; }
    }
    return VP_OK;
}

void* buf_ptr(const vp_yolo* y, int b, const void* d_input, void* d_head) {
    if (b == 0) return const_cast<void*>(d_input);
    if (b == (int)y->plan.bufs.size() - 1) return d_head;
    return y->arena + y->buf_off[(size_t)b];
}

template <int KS> void conv_launch(const vp::ConvArgs& a, bool f32, dim3 grid, hipStream_t s) {
    if (f32) hipLaunchKernelGGL((vp::yolo_conv_kernel<KS, true>), grid, dim3(vp::CONV_THREADS), 0, s, a);
    else hipLaunchKernelGGL((vp::yolo_conv_kernel<KS, false>), grid, dim3(vp::CONV_THREADS), 0, s, a);
}

// Where every internal buffer lies in the arena (HOST ONLY); returns the arena's bytes.  keep: one region per buffer, so that every launch's output is still there
// after a forward (the activation tap).  Otherwise a buffer's region is free again after the last launch that touches it: a buffer is placed, in the order of the
// first launch that writes it, at the lowest offset that overlaps no buffer still alive -- alive through the launch of its last use, so a launch never reads one
// buffer and writes another in the same bytes.
size_t place_buffers(const YoloPlan& p, int max_images, bool keep, std::vector<size_t>* off) {
    const int nb = (int)p.bufs.size(), nl = (int)p.launches.size();
    std::vector<size_t> bytes((size_t)nb, 0);
    std::vector<int> first((size_t)nb, nl), last((size_t)nb, -1);
    for (int b = 1; b + 1 < nb; ++b) bytes[(size_t)b] = up256((size_t)max_images * p.bufs[b].h * p.bufs[b].w * p.bufs[b].c * p.bufs[b].elem_bytes);
    auto touch = [&](int b, int i) { if (b > 0 && b + 1 < nb) { first[(size_t)b] = std::min(first[(size_t)b], i); last[(size_t)b] = std::max(last[(size_t)b], i); } };
    for (int i = 0; i < nl; ++i) {
        const vp_yolo_launch& l = p.launches[(size_t)i];
        touch(l.in_buf, i); touch(l.out_buf, i); touch(l.res_buf, i);
        if (l.kind == vp::YK_DECODE) { touch(l.in_buf + 1, i); touch(l.in_buf + 2, i); }
    }
    off->assign((size_t)nb, 0);
    size_t total = 0;
    std::vector<int> order;
    for (int b = 1; b + 1 < nb; ++b) order.push_back(b);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first[(size_t)a] < first[(size_t)b]; });
    std::vector<int> placed;
    for (int b : order) {
        size_t at = keep ? total : 0;
        for (bool moved = !keep; moved;) {
            moved = false;
            for (int q : placed)
                if (last[(size_t)q] >= first[(size_t)b] && at < (*off)[(size_t)q] + bytes[(size_t)q] && (*off)[(size_t)q] < at + bytes[(size_t)b]) {
                    at = (*off)[(size_t)q] + bytes[(size_t)q];
                    moved = true;
                }
        }
        (*off)[(size_t)b] = at;
        placed.push_back(b);
        total = std::max(total, at + bytes[(size_t)b]);
    }
    return total;
}

// one convolution launch: the grid every caller uses
void conv_run(const vp::ConvArgs& a, int k, bool f32, int rows_pad, hipStream_t s) {
    const dim3 grid((unsigned)((a.M + vp::CONV_WAVES * vp::CONV_PIX - 1) / (vp::CONV_WAVES * vp::CONV_PIX)), (unsigned)(rows_pad / vp::CONV_CH));
    if (k == 3) conv_launch<3>(a, f32, grid, s);
    else conv_launch<1>(a, f32, grid, s);
}

vp::DecodeArgs decode_args(const YoloPlan& p, const float* const lvl[3], int layout, int n_images) {
    vp::DecodeArgs d;
    for (int i = 0; i < 3; ++i) { d.lvl[i] = lvl[i]; d.h[i] = p.level_h[i]; d.w[i] = p.level_w[i]; d.a0[i] = p.level_a0[i]; }
    d.A = p.A; d.nc = p.d.nc; d.units = 2 + (p.d.nc + vp::DEC_CLS - 1) / vp::DEC_CLS;
    d.layout = layout; d.n_images = n_images;
    return d;
}

// the plan's launches in order on stream s
int forward_enqueue(vp_yolo* y, const void* d_input, int n, void* d_head, hipStream_t s) {
    using namespace vp;
    vp_ctx* c = y->c;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if (n == 0) return VP_OK;
    const YoloPlan& p = y->plan;
    auto blocks = [](size_t total) { return dim3((unsigned)((total + EW_THREADS - 1) / EW_THREADS)); };
    for (const vp_yolo_launch& l : p.launches) {
        void* in = buf_ptr(y, l.in_buf, d_input, d_head);
        void* out = buf_ptr(y, l.out_buf, d_input, d_head);
        switch (l.kind) {
            case YK_PACK: {
                const size_t total = (size_t)n * l.h_in * l.w_in;
                hipLaunchKernelGGL(yolo_pack_kernel, blocks(total), dim3(EW_THREADS), 0, s, (const _Float16*)in, (_Float16*)out, y->cfg.input_layout, l.h_in * l.w_in, total);
                break;
            }
            case YK_CONV: {
                const YoloConv& cv = p.convs[(size_t)l.conv];
                ConvArgs a;
                a.in = (const _Float16*)in; a.w = y->w + cv.w_off; a.bias = y->b + cv.b_off; a.out = out;
                a.res = l.res_buf >= 0 ? (const _Float16*)buf_ptr(y, l.res_buf, d_input, d_head) : nullptr;
                a.M = n * l.h_out * l.w_out; a.H = l.h_in; a.W = l.w_in; a.Ho = l.h_out; a.Wo = l.w_out;
                a.cpt = l.c_in / 8; a.steps = cv.cols_pad / YOLO_TILE_K; a.cols_pad = cv.cols_pad;
                a.c_out = l.c_out; a.s = l.s; a.act = l.act;
                a.in_off = l.in_off; a.in_stride = l.in_stride; a.out_off = l.out_off; a.out_stride = l.out_stride; a.res_off = l.res_off; a.res_stride = l.res_stride;
                conv_run(a, l.k, l.f32_out != 0, cv.rows_pad, s);
                break;
            }
            case YK_POOL: {
                const int groups = l.c_in / 8;
                const size_t total = (size_t)n * l.h_in * l.w_in * groups;
                hipLaunchKernelGGL(yolo_pool_kernel, blocks(total), dim3(EW_THREADS), 0, s, (const _Float16*)in, (_Float16*)out, l.h_in, l.w_in, groups, l.in_stride, l.in_off,
                                   l.out_off, total);
                break;
            }
            case YK_UP: {
                const int groups = l.c_in / 8;
                const size_t total = (size_t)n * l.h_out * l.w_out * groups;
                hipLaunchKernelGGL(yolo_up_kernel, blocks(total), dim3(EW_THREADS), 0, s, (const _Float16*)in, (_Float16*)out, l.h_in, l.w_in, groups, l.in_stride, l.in_off,
                                   l.out_stride, l.out_off, total);
                break;
            }
            default: {
                const float* lvl[3];
                for (int i = 0; i < 3; ++i) lvl[i] = (const float*)buf_ptr(y, l.in_buf + i, d_input, d_head);
                const DecodeArgs d = decode_args(p, lvl, y->cfg.head_layout, n);
                const size_t total = (size_t)n * d.A * d.units;
                if (y->cfg.head_dtype == VP_DET_F16) hipLaunchKernelGGL((yolo_decode_kernel<_Float16>), blocks(total), dim3(EW_THREADS), 0, s, d, (_Float16*)out);
                else hipLaunchKernelGGL((yolo_decode_kernel<float>), blocks(total), dim3(EW_THREADS), 0, s, d, (float*)out);
                break;
            }
        }
        HIPCHK(c, hipGetLastError());
    }
    return VP_OK;
}

int call_args(const vp_yolo* y, const void* input, int n_images, const void* head, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "yolo: " + m; return (int)VP_ERR_INVALID; };
    if (n_images < 0 || n_images > y->cfg.max_images) return bad("n_images = " + std::to_string(n_images) + " outside 0.." + std::to_string(y->cfg.max_images));
    if (n_images > 0 && !(input && head)) return bad("null input or head with n_images > 0");
    if ((uintptr_t)input % 2) return bad("input is not aligned to its element size");
    if ((uintptr_t)head % (y->cfg.head_dtype == VP_DET_F16 ? 2 : 4)) return bad("head is not aligned to its element size");
    return VP_OK;
}

size_t head_bytes(const vp_yolo* y, int n) { return (size_t)n * (4 + y->plan.d.nc) * (size_t)y->plan.A * (y->cfg.head_dtype == VP_DET_F16 ? 2 : 4); }

}  // namespace

extern "C" {

int vp_yolo_create(vp_handle c, const vp_yolo_cfg* cfg, const vp_yolo_tensor* tensors, int32_t n_tensors, vp_yolo_handle* out) {
    std::vector<uint16_t> w;
    std::vector<float> b;
    return stage_create(c, out,
                        [&](vp_yolo* y, std::string* why) {   // a bad plan or a failed fold: its own code and text
                            vp::YoloTensors tab;
                            int rc = make_plan(cfg, tensors, n_tensors, &tab, &y->plan, why);
                            if (!rc) rc = fold_all(tab, y->plan, &w, &b, why);
                            return rc;
                        },
                        [&](vp_yolo* y) {
                            y->cfg = *cfg;
                            const size_t total = place_buffers(y->plan, cfg->max_images, cfg->reserved[0] != 0, &y->buf_off);
                            y->arena = y->alloc(total, 0xFF);
                            y->w = y->alloc<_Float16>(w.size() * 2);
                            y->b = y->alloc<float>(b.size() * 4);
                            y->up(y->w, w.data(), w.size() * 2);
                            y->up(y->b, b.data(), b.size() * 4);
                            if (y->err == hipSuccess) y->err = hipDeviceSynchronize();
                            y->device_bytes = total + w.size() * 2 + b.size() * 4;
                            return std::string("yolo: device memory (") + std::to_string(total) + " bytes of activations): ";
                        });
}

int vp_yolo_destroy(vp_yolo_handle y) { return stage_destroy(y); }

int vp_yolo_info(vp_yolo_handle y, int32_t* nc, int32_t* A, int32_t* n_launches, int64_t* device_bytes) {
    if (!y) return VP_ERR_INVALID;
    if (nc) *nc = y->plan.d.nc;
    if (A) *A = y->plan.A;
    if (n_launches) *n_launches = (int32_t)y->plan.launches.size();
    if (device_bytes) *device_bytes = (int64_t)y->device_bytes;
    return VP_OK;
}

int vp_yolo_forward_stream(vp_yolo_handle y, const void* d_input, int32_t n_images, void* d_head, void* caller_stream) {
    if (!y) return VP_ERR_INVALID;
    std::string why;
    if (call_args(y, d_input, n_images, d_head, &why)) return fail(y->c, VP_ERR_INVALID, why);
    return forward_enqueue(y, d_input, n_images, d_head, (hipStream_t)caller_stream);
}

int vp_yolo_forward(vp_yolo_handle y, const void* input, int32_t n_images, void* head) {
    if (!y) return VP_ERR_INVALID;
    vp_ctx* c = y->c;
    std::string why;
    if (call_args(y, input, n_images, head, &why)) return fail(c, VP_ERR_INVALID, why);
    if (n_images == 0) return VP_OK;
    HostStage st(c);   // one scratch block: input | head
    const size_t in_bytes = (size_t)n_images * 3 * y->cfg.in_h * y->cfg.in_w * 2, hb = head_bytes(y, n_images);
    const size_t o_in = st.part(in_bytes), o_head = st.part(hb);
    if (st.alloc()) return st.rc;
    st.up(st.at(o_in), input, in_bytes, "upload input");
    if (!st.rc) st.rc = forward_enqueue(y, st.at(o_in), n_images, st.at(o_head), st.s);
    if (!st.rc) st.down(head, st.at(o_head), hb, "download head");
    st.sync();
    return st.rc;
}

int vp_dbg_yolo_plan(const vp_yolo_cfg* cfg, const vp_yolo_tensor* tensors, int32_t n_tensors, vp_yolo_launch* launches, int32_t max_launches, vp_yolo_buffer* buffers,
                     int32_t max_buffers, int32_t* info) {
    std::string why;
    vp::YoloTensors tab;
    YoloPlan p;
    if (int rc = make_plan(cfg, tensors, n_tensors, &tab, &p, &why)) return fail(nullptr, rc, why);
    std::vector<uint16_t> w;
    std::vector<float> b;
    if (int rc = fold_all(tab, p, &w, &b, &why)) return fail(nullptr, rc, why);   // the per-tensor refusals
    if (!info) return fail(nullptr, VP_ERR_INVALID, "yolo: null info");
    if ((launches && max_launches < (int)p.launches.size()) || (buffers && max_buffers < (int)p.bufs.size()))
        return fail(nullptr, VP_ERR_INVALID, "yolo: the plan has " + std::to_string(p.launches.size()) + " launches and " + std::to_string(p.bufs.size()) + " buffers");
    if (launches) std::memcpy(launches, p.launches.data(), sizeof(vp_yolo_launch) * p.launches.size());
    if (buffers) std::memcpy(buffers, p.bufs.data(), sizeof(vp_yolo_buffer) * p.bufs.size());
    const int32_t v[16] = {(int32_t)p.launches.size(), (int32_t)p.bufs.size(), (int32_t)p.convs.size(), p.d.nc, p.A, (int32_t)p.d.scale, p.d.ch64, p.d.ch128, p.d.ch256,
                           p.d.ch512, p.d.ch1024, p.d.d3, p.d.d6, p.d.c2d, p.d.c3d, 0};
    std::memcpy(info, v, sizeof(v));
    return VP_OK;
}

int vp_dbg_yolo_fold(const vp_yolo_cfg* cfg, const vp_yolo_tensor* tensors, int32_t n_tensors, int32_t conv, uint16_t* w, float* b, int32_t* dims) {
    std::string why;
    vp::YoloTensors tab;
    YoloPlan p;
    if (int rc = make_plan(cfg, tensors, n_tensors, &tab, &p, &why)) return fail(nullptr, rc, why);
    if (conv < 0 || conv >= (int)p.convs.size()) return fail(nullptr, VP_ERR_INVALID, "yolo: conv = " + std::to_string(conv) + " outside 0.." + std::to_string(p.convs.size() - 1));
    const vp::YoloConv& cv = p.convs[(size_t)conv];
    if (dims) { dims[0] = cv.c2w; dims[1] = cv.cols; }
    if (!w && !b) return VP_OK;
    if (!w || !b) return fail(nullptr, VP_ERR_INVALID, "yolo: w and b come together");
    const std::string r = vp::yolo_fold(tab, cv, w, (size_t)cv.cols, b);
    if (!r.empty()) return fail(nullptr, VP_ERR_INVALID, "yolo: " + r);
    return VP_OK;
}

int vp_dbg_yolo_decode_host(int32_t nc, int32_t in_h, int32_t in_w, int32_t n_images, const float* levels, int32_t head_dtype, int32_t head_layout, void* head) {
    vp_yolo_cfg cfg{};
    cfg.in_h = in_h; cfg.in_w = in_w; cfg.max_images = vp::YOLO_MAX_IMAGES; cfg.head_dtype = head_dtype; cfg.head_layout = head_layout;
    std::string why;
    if (int rc = cfg_check(&cfg, &why)) return fail(nullptr, rc, why);
    if (nc < 1 || nc > vp::YOLO_MAX_NC) return fail(nullptr, VP_ERR_INVALID, "yolo: nc = " + std::to_string(nc) + " outside 1.." + std::to_string(vp::YOLO_MAX_NC));
    if (n_images < 0 || n_images > vp::YOLO_MAX_IMAGES) return fail(nullptr, VP_ERR_INVALID, "yolo: n_images = " + std::to_string(n_images) + " outside 0.." + std::to_string(vp::YOLO_MAX_IMAGES));
    if (n_images > 0 && !(levels && head)) return fail(nullptr, VP_ERR_INVALID, "yolo: null levels or head");
    YoloPlan p;
    p.d.nc = nc;
    const float* lvl[3];
    const float* at = levels;
    int a0 = 0;
    for (int i = 0; i < 3; ++i) {
        p.level_h[i] = in_h >> (3 + i); p.level_w[i] = in_w >> (3 + i); p.level_a0[i] = a0;
        a0 += p.level_h[i] * p.level_w[i];
        lvl[i] = at;
        at += (size_t)n_images * p.level_h[i] * p.level_w[i] * (vp::YOLO_BOX_CH + nc);
    }
    p.A = a0;
    const vp::DecodeArgs d = decode_args(p, lvl, head_layout, n_images);
    for (int img = 0; img < n_images; ++img)
        for (int a = 0; a < d.A; ++a)
            for (int u = 0; u < d.units; ++u) {
                if (head_dtype == VP_DET_F16) vp::yolo_decode_unit<_Float16>(d, (_Float16*)head, (size_t)img, a, u);
                else vp::yolo_decode_unit<float>(d, (float*)head, (size_t)img, a, u);
            }
    return VP_OK;
}

int vp_dbg_yolo_activation(vp_yolo_handle y, int32_t launch, int32_t n_images, void* out) {
    if (!y) return VP_ERR_INVALID;
    vp_ctx* c = y->c;
    const YoloPlan& p = y->plan;
    if (launch < 0 || launch >= (int)p.launches.size()) return fail(c, VP_ERR_INVALID, "yolo: launch = " + std::to_string(launch) + " outside 0.." + std::to_string(p.launches.size() - 1));
    const int b = p.launches[(size_t)launch].out_buf;
    if (b == (int)p.bufs.size() - 1) return fail(c, VP_ERR_INVALID, "yolo: the decode writes the caller's head, not a buffer of the stage");
    if (!y->cfg.reserved[0]) return fail(c, VP_ERR_STATE, "yolo: the activation tap needs a stage created with cfg.reserved[0] = 1 (every buffer kept)");
    if (n_images < 1 || n_images > y->cfg.max_images || !out) return fail(c, VP_ERR_INVALID, "yolo: n_images outside 1..max_images or null out");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, y->arena + y->buf_off[(size_t)b], (size_t)n_images * p.bufs[b].h * p.bufs[b].w * p.bufs[b].c * p.bufs[b].elem_bytes, hipMemcpyDeviceToHost));
    return VP_OK;
}

int vp_dbg_yolo_conv_case(vp_handle c, const vp_yolo_launch* l, int32_t n_images, const uint16_t* in, const uint16_t* w, const float* bias, const uint16_t* res, void* out) {
    using namespace vp;
    if (!c) return VP_ERR_INVALID;
    auto bad = [&](const std::string& m) { return fail(c, VP_ERR_INVALID, "yolo conv case: " + m); };
    if (!l || !in || !w || !bias || !out) return bad("null argument");
    const int pad = l->k / 2;
    if ((l->k != 1 && l->k != 3) || (l->s != 1 && l->s != 2)) return bad("k in {1, 3} and s in {1, 2} expected");
    if (n_images < 1 || n_images > YOLO_MAX_IMAGES || l->h_in < 1 || l->w_in < 1 || l->h_in > YOLO_MAX_SIDE || l->w_in > YOLO_MAX_SIDE) return bad("sizes outside the stage's");
    if (l->h_out != (l->h_in + 2 * pad - l->k) / l->s + 1 || l->w_out != (l->w_in + 2 * pad - l->k) / l->s + 1) return bad("h_out / w_out are not the convolution's");
    if (l->c_in < 8 || l->c_in % 8 || l->in_off < 0 || l->in_off % 8 || l->in_stride % 8 || l->in_off + l->c_in > l->in_stride || l->in_stride > 8192)
        return bad("input view: channels, offset and stride in multiples of 8, offset + channels <= stride expected");
    if (l->c_out < 1 || l->out_off < 0 || l->out_off + l->c_out > l->out_stride || l->out_stride > 8192) return bad("output view: offset + channels <= stride expected");
    if (res && (l->res_off < 0 || l->res_off + l->c_out > l->res_stride || l->res_stride > 8192)) return bad("shortcut view: offset + channels <= stride expected");
    if (res && l->f32_out) return bad("a shortcut goes with an fp16 output");
    const int cols = l->k * l->k * l->c_in, cols_pad = yolo_pad_to(cols, YOLO_TILE_K), rows_pad = yolo_pad_to(l->c_out, YOLO_TILE_N);
    std::vector<uint16_t> wi((size_t)rows_pad * cols_pad, 0);
    std::vector<float> bi((size_t)rows_pad, 0.f);
    for (int o = 0; o < l->c_out; ++o) {
        std::memcpy(&wi[(size_t)o * cols_pad], w + (size_t)o * cols, sizeof(uint16_t) * (size_t)cols);
        bi[(size_t)o] = bias[o];
    }
    const size_t pin = (size_t)n_images * l->h_in * l->w_in, pout = (size_t)n_images * l->h_out * l->w_out;
    HostStage st(c);   // one scratch block: in | out | res | w | bias
    const size_t in_bytes = pin * l->in_stride * 2, out_bytes = pout * l->out_stride * (l->f32_out ? 4 : 2), res_bytes = pout * l->res_stride * 2;
    const size_t o_in = st.part(in_bytes), o_out = st.part(out_bytes), o_res = res ? st.part(res_bytes) : 0, o_w = st.part(wi.size() * 2), o_b = st.part(bi.size() * 4);
    if (st.alloc()) return st.rc;
    char *d_in = st.at(o_in), *d_out = st.at(o_out), *d_res = st.at(o_res), *d_w = st.at(o_w), *d_b = st.at(o_b);
    hipStream_t s = st.s;
    st.up(d_in, in, in_bytes, "upload in");
    st.up(d_w, wi.data(), wi.size() * 2, "upload w");
    st.up(d_b, bi.data(), bi.size() * 4, "upload bias");
    if (res) st.up(d_res, res, res_bytes, "upload res");
    st.chk(hipMemsetAsync(d_out, 0xFF, up256(out_bytes), s), "fill out");   // the part's whole room: what the kernel must not write stays 0xFF
    if (!st.rc) {
        ConvArgs a;
        a.in = (const _Float16*)d_in; a.w = (const _Float16*)d_w; a.bias = (const float*)d_b; a.out = d_out; a.res = res ? (const _Float16*)d_res : nullptr;
        a.M = (int)pout; a.H = l->h_in; a.W = l->w_in; a.Ho = l->h_out; a.Wo = l->w_out;
        a.cpt = l->c_in / 8; a.steps = cols_pad / YOLO_TILE_K; a.cols_pad = cols_pad;
        a.c_out = l->c_out; a.s = l->s; a.act = l->act;
        a.in_off = l->in_off; a.in_stride = l->in_stride; a.out_off = l->out_off; a.out_stride = l->out_stride; a.res_off = l->res_off; a.res_stride = l->res_stride;
        conv_run(a, l->k, l->f32_out != 0, rows_pad, s);
        st.chk(hipGetLastError(), "launch");
        st.down(out, d_out, out_bytes, "download out");
    }
    st.sync();
    return st.rc;
}

}  // extern "C"
