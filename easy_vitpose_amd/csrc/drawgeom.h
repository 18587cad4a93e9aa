// The skeleton overlay of vp_draw_poses_stream (include/vitpose_hip.h), for ONE value each: the gates of a row and a joint, the integer coverage test of a
// disk, a limb and a rectangle outline, the draw order, the colours and the forward RGB -> YUV conversion.  Shared by the device kernels (draw.hip) and the
// host-only tap vp_dbg_draw_host, so that the CPU tests of the tap pin the arithmetic the device runs, as posenms.h, boxgeom.h and affinegeom.h do for theirs.
// easy_vitpose_amd/draw.py restates it in numpy, tests/draw_model.py in plain scalar loops.
//
// Modelled on the reference's draw_points_and_skeleton (vit_utils/visualization.py:360-481): opaque colours, no anti-aliasing.  The rasterisation is this
// project's own integer one: parity against OpenCV's circle / line / rectangle is UNPINNED and not claimed.
//
// A row is one person: keypoints [K, 3] (y, x, conf) float32 in frame pixels, a frame index, optionally a rank (rank < 0: the row is not drawn), an id (absent:
// the row's index in the call) and a box (x1, y1, x2, y2) float32.
//   coordinate  a float v is usable iff -16384 < v < 16384 (false for NaN and +-inf); its pixel is (int)v, truncation toward zero, so |pixel| <= DRAW_COORD_MAX.
//   joint       visible iff conf > conf_thr (float32 compare, false for a NaN confidence) and x and y are usable; pixel ((int)x, (int)y).
//   limb (a, b) drawn iff both of its joints are visible (visualization.py:436).
//   box         drawn iff its four values are usable; the corners are ordered after truncation (x1 <= x2, y1 <= y2).
// Coverage of pixel p = (px, py), all in int64:
//   disk at c, radius r:          |p - c|^2 <= r^2
//   limb a -> b, thickness t:     d = b - a, L2 = |d|^2, q = p - a;
//                                 (L2 > 0 and 0 <= q.d <= L2 and (q x d)^2 <= floor(t^2 L2 / 4))  or  4 |p - a|^2 <= t^2  or  4 |p - b|^2 <= t^2
//                                 (the last two are the round caps; a == b leaves the caps only)
//   outline of thickness t:       o = t / 2 (integer division);  x1 - o <= px <= x2 + o and y1 - o <= py <= y2 + o, and NOT
//                                 (x1 - o + t <= px <= x2 + o - t and y1 - o + t <= py <= y2 + o - t): t pixels on every side, the outermost o of them outside the box
// Bounds: frames have h, w <= DRAW_MAX_DIM = 8192, so 0 <= p <= 8191 and |a|, |b|, |c| <= 16383: |q| <= 24574 and |d| <= 32766 per axis,
//   |q.d| and |q x d| <= 2 * 24574 * 32766 < 1.62e9, (q x d)^2 < 2.6e18 < 2^63; L2 <= 2 * 32766^2 < 2.15e9 and t <= 16: t^2 L2 < 5.5e11.  Every test is exact.
// Draw order (the reference's): rows in ascending row index; within a row its box, then its limbs in table order, then its joints in joint order.  A pixel shows
//   the LAST primitive in this order that covers it: record index = row * (has_box + n_limbs + K) + slot is the order.
// Colours: limb and box colour = limb_colors[id mod n_limb_colors], joint colour = point_colors[j mod n_point_colors], the mathematical mod (negative ids).
//   Radius 0 stands for max(1, min(h, w) / 150) of the row's frame (visualization.py:389).
// Writing: RGB24 / BGR24 three bytes per covered pixel.  NV12: every colour is converted once, (Y, U, V) below; Y per covered pixel, and a chroma sample takes
//   the (U, V) of the last primitive in draw order that covers any of its up-to-four pixels.
// RGB -> YUV, the forward matrices of pixfmt.h's table as round(x 2^8) integers of the standard matrices (Kr, Kb = 0.299, 0.114 / 0.2126, 0.0722; limited range:
//   luma scaled by 219/255, chroma by 224/255), int32 with an arithmetic right shift:
//     Y = clip255(yoff + ((yr R + yg G + yb B + 128) >> 8)),  U = clip255(128 + ((ur R + ug G + ub B + 128) >> 8)),  V likewise
//     matrix      yoff  yr  yg   yb   ur   ug   ub   vr   vg    vb
//     BT601       16    66  129  25   -38  -74  112  112  -94   -18
//     BT709       16    47  157  16   -26  -87  112  112  -102  -10
//     BT601_FULL  0     77  150  29   -43  -85  128  128  -107  -21
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pixfmt.h"

namespace vp {

constexpr int DRAW_MAX_LIMBS = 256;     // VP_DRAW_MAX_LIMBS
constexpr int DRAW_MAX_COLORS = 32;     // VP_DRAW_MAX_COLORS
constexpr int DRAW_MAX_K = 256;
constexpr int DRAW_MAX_DIM = 8192;
constexpr int DRAW_COORD_MAX = 16383;
constexpr int DRAW_MAX_RADIUS = 64, DRAW_MAX_THICKNESS = 16;

enum DrawType { DRAW_EMPTY = 0, DRAW_BOX = 1, DRAW_LIMB = 2, DRAW_DISK = 3 };

// the style of a call, by kernel argument (no host-to-device copy): 4 + 3 * 4 + 512 + 2 * 96 + 2 * 4 bytes
struct DrawStyle {
    float conf_thr;
    int32_t radius, thickness, n_limbs;
    uint8_t limbs[DRAW_MAX_LIMBS * 2];
    int32_t n_point_colors, n_limb_colors;
    uint8_t point_colors[DRAW_MAX_COLORS * 3], limb_colors[DRAW_MAX_COLORS * 3];   // RGB
};

// One primitive slot as the raster pass reads it.  The key is what the tile test needs (16 bytes); x0 > x1 marks an empty slot.
struct DrawKey { int16_t x0, y0, x1, y1; int32_t frame, type; };   // inclusive bounding box, clipped to the frame
struct DrawBody { int32_t type, frame, ax, ay, bx, by, t, color; };   // t: radius or thickness; color: the three bytes as the plane holds them (or Y, U, V), byte 0 lowest

struct RgbYuvCoef { int32_t yoff, y[3], u[3], v[3]; };

__host__ __device__ inline RgbYuvCoef rgb_yuv_coef(int matrix) {
    if (matrix == YUV_BT709) return RgbYuvCoef{16, {47, 157, 16}, {-26, -87, 112}, {112, -102, -10}};
    if (matrix == YUV_BT601_FULL) return RgbYuvCoef{0, {77, 150, 29}, {-43, -85, 128}, {128, -107, -21}};
    return RgbYuvCoef{16, {66, 129, 25}, {-38, -74, 112}, {112, -94, -18}};
}

// one (R, G, B) colour -> yuv[3]
__host__ __device__ inline void rgb_to_yuv(const RgbYuvCoef& k, int R, int G, int B, int* yuv) {
    yuv[0] = clip255(k.yoff + ((k.y[0] * R + k.y[1] * G + k.y[2] * B + 128) >> 8));
    yuv[1] = clip255(128 + ((k.u[0] * R + k.u[1] * G + k.u[2] * B + 128) >> 8));
    yuv[2] = clip255(128 + ((k.v[0] * R + k.v[1] * G + k.v[2] * B + 128) >> 8));
}

// the three bytes of an RGB colour as a frame of (format, matrix) holds them, byte 0 lowest
__host__ __device__ inline int32_t draw_pack_color(const uint8_t* rgb, int format, int matrix) {
    int c[3] = {rgb[0], rgb[1], rgb[2]};
    if (format == PIX_BGR24) { c[0] = rgb[2]; c[2] = rgb[0]; }
    if (format == PIX_NV12) rgb_to_yuv(rgb_yuv_coef(matrix), rgb[0], rgb[1], rgb[2], c);
    return c[0] | (c[1] << 8) | (c[2] << 16);
}

__host__ __device__ inline bool draw_usable(float v) { return v > -16384.f && v < 16384.f; }
__host__ __device__ inline bool draw_visible(const float* kp, int j, float conf_thr) {
    return kp[3 * j + 2] > conf_thr && draw_usable(kp[3 * j]) && draw_usable(kp[3 * j + 1]);
}
__host__ __device__ inline int draw_mod(int32_t a, int32_t n) { const int m = a % n; return m < 0 ? m + n : m; }
__host__ __device__ inline int draw_radius(int radius, int h, int w) {
    if (radius > 0) return radius;
    const int r = (h < w ? h : w) / 150;
    return r > 1 ? r : 1;
}

__host__ __device__ inline bool draw_covers_disk(int64_t px, int64_t py, int64_t cx, int64_t cy, int64_t r) {
    const int64_t dx = px - cx, dy = py - cy;
    return dx * dx + dy * dy <= r * r;
}
__host__ __device__ inline bool draw_covers_limb(int64_t px, int64_t py, int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t t) {
    const int64_t dx = bx - ax, dy = by - ay, L2 = dx * dx + dy * dy, qx = px - ax, qy = py - ay, rx = px - bx, ry = py - by;
    if (4 * (qx * qx + qy * qy) <= t * t || 4 * (rx * rx + ry * ry) <= t * t) return true;
    if (L2 == 0) return false;
    const int64_t dot = qx * dx + qy * dy, cross = qx * dy - qy * dx;
    return dot >= 0 && dot <= L2 && cross * cross <= (t * t * L2) / 4;
}
__host__ __device__ inline bool draw_covers_box(int64_t px, int64_t py, int64_t x1, int64_t y1, int64_t x2, int64_t y2, int64_t t) {
    const int64_t o = t / 2;
    if (px < x1 - o || px > x2 + o || py < y1 - o || py > y2 + o) return false;
    return !(px >= x1 - o + t && px <= x2 + o - t && py >= y1 - o + t && py <= y2 + o - t);
}
__host__ __device__ inline bool draw_covers(const DrawBody& b, int px, int py) {
    if (b.type == DRAW_DISK) return draw_covers_disk(px, py, b.ax, b.ay, b.t);
    if (b.type == DRAW_LIMB) return draw_covers_limb(px, py, b.ax, b.ay, b.bx, b.by, b.t);
    if (b.type == DRAW_BOX) return draw_covers_box(px, py, b.ax, b.ay, b.bx, b.by, b.t);
    return false;
}

// What one row needs from the call, and the primitive of slot s of the row (s in [0, has_box + n_limbs + K): box, limbs, joints).  The gates live here: a slot
// that is not drawn comes back with key.x0 > key.x1 and type DRAW_EMPTY.  h, w, format, matrix: the row's frame (the caller has checked the frame index).
struct DrawRow {
    const float* kp;        // [K, 3]
    const float* box;       // 4 values or null
    int32_t id, frame, h, w, format, matrix;
};

__host__ __device__ inline void draw_primitive(const DrawRow& r, int K, const DrawStyle& st, int s, DrawKey* key, DrawBody* body) {
    *key = DrawKey{1, 1, 0, 0, r.frame, DRAW_EMPTY};
    *body = DrawBody{DRAW_EMPTY, r.frame, 0, 0, 0, 0, 0, 0};
    const int has_box = r.box ? 1 : 0;
    int64_t x0, y0, x1, y1;
    if (s < has_box) {
        for (int q = 0; q < 4; ++q)
            if (!draw_usable(r.box[q])) return;
        const int xa = (int)r.box[0], ya = (int)r.box[1], xb = (int)r.box[2], yb = (int)r.box[3];
        body->type = DRAW_BOX;
        body->ax = xa < xb ? xa : xb; body->ay = ya < yb ? ya : yb; body->bx = xa < xb ? xb : xa; body->by = ya < yb ? yb : ya;
        body->t = st.thickness;
        body->color = draw_pack_color(st.limb_colors + 3 * draw_mod(r.id, st.n_limb_colors), r.format, r.matrix);
        const int o = st.thickness / 2;
        x0 = body->ax - o; y0 = body->ay - o; x1 = body->bx + o; y1 = body->by + o;
    } else if (s < has_box + st.n_limbs) {
        const int l = s - has_box, a = st.limbs[2 * l], b = st.limbs[2 * l + 1];
        if (!draw_visible(r.kp, a, st.conf_thr) || !draw_visible(r.kp, b, st.conf_thr)) return;
        body->type = DRAW_LIMB;
        body->ax = (int)r.kp[3 * a + 1]; body->ay = (int)r.kp[3 * a]; body->bx = (int)r.kp[3 * b + 1]; body->by = (int)r.kp[3 * b];
        body->t = st.thickness;
        body->color = draw_pack_color(st.limb_colors + 3 * draw_mod(r.id, st.n_limb_colors), r.format, r.matrix);
        const int o = (st.thickness + 1) / 2;   // everything covered lies within t / 2 of the segment
        x0 = (body->ax < body->bx ? body->ax : body->bx) - o; x1 = (body->ax < body->bx ? body->bx : body->ax) + o;
        y0 = (body->ay < body->by ? body->ay : body->by) - o; y1 = (body->ay < body->by ? body->by : body->ay) + o;
    } else {
        const int j = s - has_box - st.n_limbs;
        if (!draw_visible(r.kp, j, st.conf_thr)) return;
        body->type = DRAW_DISK;
        body->ax = body->bx = (int)r.kp[3 * j + 1]; body->ay = body->by = (int)r.kp[3 * j];
        body->t = draw_radius(st.radius, r.h, r.w);
        body->color = draw_pack_color(st.point_colors + 3 * draw_mod(j, st.n_point_colors), r.format, r.matrix);
        x0 = body->ax - body->t; x1 = body->ax + body->t; y0 = body->ay - body->t; y1 = body->ay + body->t;
    }
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > r.w - 1) x1 = r.w - 1;
    if (y1 > r.h - 1) y1 = r.h - 1;
    if (x0 > x1 || y0 > y1) { body->type = DRAW_EMPTY; return; }   // nothing of it on the frame
    *key = DrawKey{(int16_t)x0, (int16_t)y0, (int16_t)x1, (int16_t)y1, r.frame, body->type};
}

}  // namespace vp
