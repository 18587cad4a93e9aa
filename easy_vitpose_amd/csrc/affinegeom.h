// The training-protocol crop of ViTPose (TopDownAffine(use_udp=True)) for ONE box, written once: box -> centre and scale, the inverse map of the
// warp, and the fixed-point sampling position of an output pixel.  Shared by the device kernels (affine.hip box_cs_kernel and
// crop_affine_kernel), the host plan of vp_infer_images_affine (infer.hip) and the host-only tap vp_dbg_box_cs, so that the CPU tests of the tap pin the
// arithmetic the device runs.  easy_vitpose_amd/cropprep.py (box_to_cs, affine_crops_host) restates it in numpy.
//
// Box to centre and scale: _xywh2cs (easy_ViTPose/datasets/COCO.py:322-337) with its widths, on a float32 box (x1, y1, x2, y2) widened to double:
//   w = x2 - x1, h = y2 - y1;  cx = (float)(x1 + w 0.5), cy = (float)(y1 + h 0.5)
//   w > 0.75 h: h = w / 0.75;  w < 0.75 h: w = h 0.75        (the box is EXTENDED to 3:4 with image content, not padded with black)
//   s = (float)(w / 200);  s = (float)(s box_scale);  S_w = (float)(s 200)        (numpy 2 keeps the float32 scale array float32 under both multiplications)
// and likewise S_h.  The reference's 1.25 is the default box_scale; its `center[0] != -1` test (a dataset sentinel for 'no box') is not reproduced: a
// box whose centre is x = -1 is scaled like every other.  The box is NOT clipped to the frame: pixels outside it read as 0.
// Status values and their order are box_geometry's: 2 a coordinate is not finite, 3 w <= 0 or h <= 0 (1, a bad frame index, is the caller's).
// Every finite input has a defined result: a side above BOX_MAX_SIDE (or one that overflowed float32) is CLAMPED to BOX_MAX_SIDE, each side on its own,
// and a side that underflowed to 0 is an empty box (status 3) -- a valid (cx, cy, S_w, S_h) always has S_w > 0 and S_h > 0, which is what lets an all-zero
// row stand for a refused box behind the decode.
//
// Inverse map (the device never inverts a matrix): output pixel (ox, oy) of the 192 x 256 crop samples the frame at
//   src_x(ox) = ox (S_w / 191) + (cx - S_w / 2),   src_y(oy) = oy (S_h / 255) + (cy - S_h / 2)
// in fp64 with the product and the sum kept unfused (the library builds with -ffp-contract=fast): the inverse of get_warp_matrix(0, c 2, [191, 255], S)
// (vit_utils/post_processing/post_transforms.py:312-340).  Rotation is not supported.
//
// Sampling: the project's own fixed-point contract, MODELLED ON OpenCV's 8-bit warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) -- 1/32-pixel source coordinates,
// 15-bit weights -- and PARITY UNPINNED against that binary (cv2 is not installed where this was written; equality is not claimed):
//   Xq = floor(src_x 32 + 0.5) as int64 (src_x 32 + 0.5 clamped to +-2^40 first: any such position is far outside a frame of at most BOX_MAX_SIDE pixels),
//   sx = Xq >> 5, ax = Xq & 31;  the same for y
//   weights (32 - ax)(32 - ay) 32, ax (32 - ay) 32, (32 - ax) ay 32, ax ay 32  (sum 32768) on taps (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1)
//   per channel out = (sum w p + 16384) >> 15, the taps being source pixels converted to RGB8 (pixfmt.h), a tap outside the frame 0.
// Integer from Xq on, so host and device agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "boxgeom.h"

namespace vp {

// box -> cs4 = {cx, cy, S_w, S_h}; returns BOX_OK, BOX_NOT_FINITE or BOX_EMPTY (cs4 untouched unless BOX_OK)
__host__ __device__ inline int box_cs(float bx1, float by1, float bx2, float by2, float box_scale, float* cs4) {
    const double x1 = bx1, y1 = by1, x2 = bx2, y2 = by2;
    if (!isfinite(x1) || !isfinite(y1) || !isfinite(x2) || !isfinite(y2)) return BOX_NOT_FINITE;
    double w = x2 - x1, h = y2 - y1;
    if (!(w > 0.0) || !(h > 0.0)) return BOX_EMPTY;
    const float cx = (float)(x1 + w * 0.5), cy = (float)(y1 + h * 0.5);   // (w 0.5 is exact: fused or not, one rounding)
    const double t = 0.75 * h;
    if (w > t) h = w / 0.75;
    else if (w < t) w = h * 0.75;
    float sw = (float)(w / 200.0), sh = (float)(h / 200.0);
    sw = (float)((double)sw * (double)box_scale); sh = (float)((double)sh * (double)box_scale);   // the float32 product: exact in double, rounded once
    sw = (float)((double)sw * 200.0); sh = (float)((double)sh * 200.0);
    sw = fminf(sw, (float)BOX_MAX_SIDE); sh = fminf(sh, (float)BOX_MAX_SIDE);
    if (!(sw > 0.f) || !(sh > 0.f)) return BOX_EMPTY;
    cs4[0] = cx; cs4[1] = cy; cs4[2] = sw; cs4[3] = sh;
    return BOX_OK;
}

// a caller's (cx, cy, S_w, S_h): finite, 0 < S <= BOX_MAX_SIDE
__host__ __device__ inline bool cs_valid(const float* cs4) {
    return isfinite((double)cs4[0]) && isfinite((double)cs4[1]) && cs4[2] > 0.f && cs4[3] > 0.f && cs4[2] <= (float)BOX_MAX_SIDE && cs4[3] <= (float)BOX_MAX_SIDE;
}

// src(o) = o A + B per axis
struct AffineMap { double ax, bx, ay, by; };

__host__ __device__ inline AffineMap affine_map(const float* cs4) {
    const double cx = cs4[0], cy = cs4[1], sw = cs4[2], sh = cs4[3];
    return AffineMap{sw / 191.0, cx - sw * 0.5, sh / 255.0, cy - sh * 0.5};   // (S 0.5 is exact)
}

// output index o of an axis -> the integer source position s and its 1/32 fraction a
__host__ __device__ inline void affine_axis(int o, double A, double B, int64_t* s, int* a) {
#ifdef __HIP_DEVICE_COMPILE__
    const double src = __dadd_rn(__dmul_rn((double)o, A), B);
#else
    volatile double prod = (double)o * A;   // kept apart from the sum whatever the host compiler is allowed to contract
    const double src = prod + B;
#endif
    const double lim = 1099511627776.0;   // 2^40
    const double q = fmin(fmax(src * 32.0 + 0.5, -lim), lim);   // (src 32 is exact: one rounding, fused or not)
    const int64_t X = (int64_t)floor(q);
    *s = X >> 5;
    *a = (int)(X & 31);
}

// one channel of one output pixel from its four taps
__host__ __device__ inline int affine_blend(int p00, int p01, int p10, int p11, int ax, int ay) {
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    return (w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 16384) >> 15;
}

// frame rows [*lo, *hi) the crop of cs4 taps on a frame of fh rows (lo == hi: none): src_y grows with oy, so rows sy(0) .. sy(255) + 1, clipped
__host__ __device__ inline void affine_row_band(const float* cs4, int32_t fh, int32_t* lo, int32_t* hi) {
    const AffineMap m = affine_map(cs4);
    int64_t s0, s1;
    int a;
    affine_axis(0, m.ay, m.by, &s0, &a);
    affine_axis(255, m.ay, m.by, &s1, &a);
    const int64_t l = s0 < 0 ? 0 : (s0 > fh ? fh : s0), h = s1 + 2 < 0 ? 0 : (s1 + 2 > fh ? fh : s1 + 2);
    *lo = (int32_t)l;
    *hi = (int32_t)(h < l ? l : h);
}

}  // namespace vp
