// The letterbox stage's arithmetic (include/vitpose_hip.h, "The letterbox stage"), stated once for the kernel of letterbox.hip and the host tap
// vp_dbg_letterbox_host: the geometry of ultralytics' LetterBox(new_shape, auto=False, scaleFill=False, center=True) over doubles (host only), the axis
// coefficients and the two passes of OpenCV's 8-bit INTER_LINEAR as easy_vitpose_amd/cropprep.py resize_linear_u8 restates them, and the output values.
// Every source pixel is converted to RGB8 first (pixfmt.h), the resize runs on RGB8.  letterbox.hip is compiled with -ffp-contract=off: the fp64 product and
// difference of a coefficient stay two operations, as numpy computes them, and float32 division is correctly rounded.
#pragma once
#include <cmath>
#include <cstdint>

#include "pixfmt.h"

#if defined(__HIPCC__)
#define VP_LB_HD __host__ __device__ inline
#else
#define VP_LB_HD inline
#endif

namespace vp {

constexpr int LB_MAX_IMAGES = 64, LB_MAX_SIDE = 8192;
constexpr int LB_F32 = 0, LB_F16 = 1, LB_U8 = 2;              // == VP_LB_*
constexpr int LB_RESIZE = 0, LB_IDENTITY = 1, LB_BOX2 = 2;    // LbRec::mode

// one image of a call as the kernel and the host tap read it
struct LbRec {
    const uint8_t* plane[2];
    int64_t pitch[2];
    int32_t h, w, format, matrix;
    int32_t left, top, new_w, new_h;   // the resized frame lies at rows [top, top + new_h), columns [left, left + new_w) of the output
    int32_t mode, pad_;
    double scale_x, scale_y;           // 1.0 / ((double)new / (double)src): OpenCV's scale_x = 1. / inv_scale_x
};

struct LbParams { int32_t in_h, in_w, dtype, layout, order, pad_value; };

struct LbAxis { int s0, s1, a0, a1; };

// output index d of an axis of ssize source pixels: taps s0, s1 and their 11-bit weights (cropprep._axis_coeffs)
VP_LB_HD LbAxis lb_axis(int d, double scale, int ssize) {
    const double pos = ((double)d + 0.5) * scale;
    float f = (float)(pos - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    LbAxis c;
    c.s0 = s;
    c.s1 = s + 1 < ssize - 1 ? s + 1 : ssize - 1;
    c.a1 = (int)rintf(f * 2048.f);
    c.a0 = (int)rintf((1.f - f) * 2048.f);
    return c;
}

// source pixel (y, x) of a frame in format FMT as RGB8
template <int FMT> VP_LB_HD void lb_fetch(const LbRec& r, const YuvCoef& k, int y, int x, int* rgb) {
    if (FMT == PIX_NV12) {
        const uint8_t* uv = r.plane[1] + (int64_t)(y >> 1) * r.pitch[1] + (int64_t)(x >> 1) * 2;
        yuv_to_rgb(k, r.plane[0][(int64_t)y * r.pitch[0] + x], uv[0], uv[1], rgb);
        return;
    }
    const uint8_t* p = r.plane[0] + (int64_t)y * r.pitch[0] + (int64_t)x * 3;
    rgb[0] = p[FMT == PIX_BGR24 ? 2 : 0]; rgb[1] = p[1]; rgb[2] = p[FMT == PIX_BGR24 ? 0 : 2];
}

// pixel (y, x) of the resized frame (0 <= y < new_h, 0 <= x < new_w); cy = lb_axis(y, scale_y, h), read in mode LB_RESIZE only
template <int FMT> VP_LB_HD void lb_pixel(const LbRec& r, const YuvCoef& k, const LbAxis& cy, int y, int x, int* rgb) {
    if (r.mode == LB_IDENTITY) { lb_fetch<FMT>(r, k, y, x, rgb); return; }
    int p00[3], p01[3], p10[3], p11[3];
    if (r.mode == LB_BOX2) {   // both scales exactly 2: INTER_LINEAR is the 2 x 2 box average there
        lb_fetch<FMT>(r, k, 2 * y, 2 * x, p00); lb_fetch<FMT>(r, k, 2 * y, 2 * x + 1, p01);
        lb_fetch<FMT>(r, k, 2 * y + 1, 2 * x, p10); lb_fetch<FMT>(r, k, 2 * y + 1, 2 * x + 1, p11);
        for (int c = 0; c < 3; ++c) rgb[c] = (p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2;
        return;
    }
    const LbAxis cx = lb_axis(x, r.scale_x, r.w);
    lb_fetch<FMT>(r, k, cy.s0, cx.s0, p00); lb_fetch<FMT>(r, k, cy.s0, cx.s1, p01);
    lb_fetch<FMT>(r, k, cy.s1, cx.s0, p10); lb_fetch<FMT>(r, k, cy.s1, cx.s1, p11);
    for (int c = 0; c < 3; ++c) {
        const int r0 = p00[c] * cx.a0 + p01[c] * cx.a1;
        const int r1 = p10[c] * cx.a0 + p11[c] * cx.a1;
        rgb[c] = (uint8_t)((((cy.a0 * (r0 >> 4)) >> 16) + ((cy.a1 * (r1 >> 4)) >> 16) + 2) >> 2);
    }
}

// the output value of byte v: what `im.float() / 255` and `im.half() / 255` give
VP_LB_HD float lb_f32(int v) { return (float)v / 255.0f; }
VP_LB_HD _Float16 lb_f16(int v) { return (_Float16)lb_f32(v); }

VP_LB_HD int lb_elem_bytes(int dtype) { return dtype == LB_F32 ? 4 : (dtype == LB_F16 ? 2 : 1); }

// element index of (image n, channel c, row y, column x) in the output tensor
VP_LB_HD int64_t lb_index(const LbParams& p, int64_t n, int c, int y, int x) {
    return p.layout == 0 ? ((n * 3 + c) * p.in_h + y) * p.in_w + x : ((n * p.in_h + y) * p.in_w + x) * 3 + c;
}

// ---- the geometry (HOST ONLY, doubles).  false: new_w or new_h comes out 0
struct LbPlace { int32_t left, top, new_w, new_h; };
struct LbUndo { float gain, pad_x, pad_y; };   // what vp_detect_stream divides and subtracts by (ultralytics' scale_boxes)

inline bool lb_geometry(int h, int w, int in_h, int in_w, int scaleup, LbPlace* pl, LbUndo* un) {
    const double gain = std::fmin((double)in_h / (double)h, (double)in_w / (double)w);
    const bool clamped = !scaleup && gain > 1.0;
    const double r = clamped ? 1.0 : gain;
    const double nw = std::nearbyint((double)w * r), nh = std::nearbyint((double)h * r);   // round half to even
    if (nw < 1.0 || nh < 1.0) return false;
    pl->new_w = (int32_t)nw;
    pl->new_h = (int32_t)nh;
    pl->left = (int32_t)std::nearbyint((double)(in_w - pl->new_w) / 2.0 - 0.1);
    pl->top = (int32_t)std::nearbyint((double)(in_h - pl->new_h) / 2.0 - 0.1);
    if (clamped) {
        un->gain = 1.0f; un->pad_x = (float)pl->left; un->pad_y = (float)pl->top;
    } else {   // devdetect.letterbox_params: the pads from the UNROUNDED scaled size
        un->gain = (float)gain;
        un->pad_x = (float)(std::nearbyint(((double)in_w - (double)w * gain) / 2.0 - 0.1) + 0.0);   // + 0.0: round(-0.1) is 0, not -0
        un->pad_y = (float)(std::nearbyint(((double)in_h - (double)h * gain) / 2.0 - 0.1) + 0.0);
    }
    return true;
}

// mode and scales of a placed frame
inline void lb_resize_mode(int h, int w, const LbPlace& pl, LbRec* r) {
    r->scale_x = 1.0 / ((double)pl.new_w / (double)w);
    r->scale_y = 1.0 / ((double)pl.new_h / (double)h);
    r->mode = (pl.new_w == w && pl.new_h == h) ? LB_IDENTITY : (r->scale_x == 2.0 && r->scale_y == 2.0 ? LB_BOX2 : LB_RESIZE);
}

}  // namespace vp
