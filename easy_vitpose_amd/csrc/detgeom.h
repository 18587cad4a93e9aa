// The detector stage's arithmetic (include/vitpose_hip.h, "The detector stage"), stated once for the kernels of detect.hip and the host tap vp_dbg_detect_host:
// best-class pick, candidate test, box corners, the 64-bit sort key, the IoU of the greedy NMS and the map back to frame pixels.  Everything is float32, every
// operation is written out one at a time (detect.hip is compiled with -ffp-contract=off, division is correctly rounded), so device and host agree bit for bit.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define VP_DET_HD __host__ __device__ inline
#else
#define VP_DET_HD inline
#endif

namespace vp {

constexpr int DET_MAX_IMAGES = 64, DET_MAX_CLASSES = 256, DET_MAX_CAND = 2048, DET_MAX_DET = 1024, DET_MAX_ANCHORS = 1 << 20;
constexpr int DET_FLAG_CAND = 1, DET_FLAG_ROWS = 4, DET_FLAG_BAD_BOX = 8;

struct DetParams {
    int32_t nc, layout, dtype, agnostic, max_det;
    float conf_thr, iou_thr, extent;
    uint32_t class_mask[8];
};

struct DetImage { float gain, pad_x, pad_y, frame_w, frame_h; };   // == vp_det_image
struct DetImages { DetImage im[DET_MAX_IMAGES]; };                  // the table of a call, a kernel argument

// one candidate as the scan leaves it and the NMS reads it
struct DetCand { float cx, cy, w, h, score; int32_t cls, anchor, pad; };

VP_DET_HD uint32_t det_bits(float v) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(v);
#else
    std::memcpy(&u, &v, 4);
#endif
    return u;
}

VP_DET_HD bool det_finite(float v) { return (det_bits(v) & 0x7f800000u) != 0x7f800000u; }

// the running best of an anchor: class c with score s replaces (best, cls) iff s is no NaN and strictly larger (the first class of the largest score wins)
VP_DET_HD void det_pick(float s, int c, float& best, int& cls) {
    if (s == s && (cls < 0 || s > best)) { best = s; cls = c; }
}

// 0: no candidate, 1: candidate, 2: passes score and class but its box is not finite (skipped, flag 8)
VP_DET_HD int det_candidate(const DetParams& p, float best, int cls, float cx, float cy, float w, float h) {
    if (cls < 0 || !(best > p.conf_thr) || !((p.class_mask[cls >> 5] >> (cls & 31)) & 1u)) return 0;
    return det_finite(cx) && det_finite(cy) && det_finite(w) && det_finite(h) ? 1 : 2;
}

// (x1, y1, x2, y2) in detector-input pixels
VP_DET_HD void det_box(float cx, float cy, float w, float h, float* b) {
    const float hw = w * 0.5f, hh = h * 0.5f;
    b[0] = cx - hw; b[1] = cy - hh; b[2] = cx + hw; b[3] = cy + hh;
}

// ascending key order = score descending, then anchor ascending (candidate scores are > conf_thr >= 0, so equal floats have equal bits)
VP_DET_HD uint64_t det_key(float score, int32_t anchor) {
    const uint32_t u = det_bits(score), asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)(~asc) << 32) | (uint32_t)anchor;
}

// the score a key was made from (a candidate's score is positive)
VP_DET_HD float det_key_score(uint64_t key) {
    const uint32_t u = ~(uint32_t)(key >> 32) ^ 0x80000000u;
    float v;
#if defined(__HIP_DEVICE_COMPILE__)
    v = __uint_as_float(u);
#else
    std::memcpy(&v, &u, 4);
#endif
    return v;
}

VP_DET_HD float det_area(const float* b, float extent) {
    const float sx = (b[2] - b[0]) + extent, sy = (b[3] - b[1]) + extent;
    return sx * sy;
}

// b is suppressed by a iff !(det_iou(a, b) <= iou_thr): a NaN suppresses
VP_DET_HD float det_iou(const float* a, const float* b, float extent) {
    const float lx = a[0] < b[0] ? b[0] : a[0], ly = a[1] < b[1] ? b[1] : a[1];
    const float hx = a[2] < b[2] ? a[2] : b[2], hy = a[3] < b[3] ? a[3] : b[3];
    float iw = (hx - lx) + extent, ih = (hy - ly) + extent;
    iw = iw < 0.f ? 0.f : iw;
    ih = ih < 0.f ? 0.f : ih;
    const float inter = iw * ih;
    return inter / ((det_area(a, extent) + det_area(b, extent)) - inter);
}

VP_DET_HD float det_unpad(float v, float pad, float gain, float side) {
    v = (v - pad) / gain;
    v = v < 0.f ? 0.f : v;
    return v < side ? v : side;
}

// a picked box to frame pixels
VP_DET_HD void det_to_frame(const DetImage& im, const float* b, float* out) {
    out[0] = det_unpad(b[0], im.pad_x, im.gain, im.frame_w);
    out[1] = det_unpad(b[1], im.pad_y, im.gain, im.frame_h);
    out[2] = det_unpad(b[2], im.pad_x, im.gain, im.frame_w);
    out[3] = det_unpad(b[3], im.pad_y, im.gain, im.frame_h);
}

}  // namespace vp
