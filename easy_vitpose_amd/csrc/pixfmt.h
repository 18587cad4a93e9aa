// Pixel formats of the frames and boxes entries (include/vitpose_hip.h vp_image) and the ONE definition of their conversion to RGB8, shared by
// the crop kernel's pixel fetch (elementwise.hip crop_resize_kernel) and the host (frame_plan's checks, the byte counts of the staging).
// easy_vitpose_amd/cropprep.py::nv12_to_rgb restates it in numpy; tests/test_pixfmt_host.py pins that restatement against plain integers.
//
// NV12 -> RGB, int32 with arithmetic right shifts (floor), per SOURCE pixel, before any interpolation:
//   y' = max(Y - yoff, 0), u' = U - 128, v' = V - 128
//   R = clip255((cy y' + crv v'          + 2^19) >> 20)
//   G = clip255((cy y' + cgu u' + cgv v' + 2^19) >> 20)
//   B = clip255((cy y' + cbu u'          + 2^19) >> 20)
// BT601 (limited range) carries the integers of 1.164 / 1.596 / 0.391 / 0.813 / 2.018 at shift 20, the constants of OpenCV's
// cvtColor(COLOR_YUV2RGB_NV12); BT709 (limited) and BT601_FULL are round(x 2^20) of the standard matrices.  Over all 2^24 (Y, U, V) the largest
// intermediate magnitude is 5.7e8: int32 holds it.  Chroma is replicated: pixel (y, x) reads the UV pair (y >> 1, x >> 1).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PF_HD __host__ __device__ inline
#else   // a plain host compiler (the layout part of hoststage.h in a stand-alone program): the same functions, host only
#define PF_HD inline
#endif

namespace vp {

enum PixFormat { PIX_RGB24 = 0, PIX_BGR24 = 1, PIX_NV12 = 2, PIX_FORMATS = 3 };   // == VP_PIX_*
enum YuvMatrix { YUV_BT601 = 0, YUV_BT709 = 1, YUV_BT601_FULL = 2, YUV_MATRICES = 3 };   // == VP_YUV_*

struct YuvCoef { int32_t yoff, cy, crv, cgu, cgv, cbu; };

PF_HD YuvCoef yuv_coef(int matrix) {
    if (matrix == YUV_BT709) return YuvCoef{16, 1220945, 1879825, -223607, -558796, 2215014};
    if (matrix == YUV_BT601_FULL) return YuvCoef{0, 1048576, 1470104, -360853, -748826, 1858077};
    return YuvCoef{16, 1220542, 1673527, -409993, -852492, 2116026};
}

PF_HD int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one (Y, U, V) sample -> rgb[3]
PF_HD void yuv_to_rgb(const YuvCoef& k, int Y, int U, int V, int* rgb) {
    const int32_t yy = Y - k.yoff, y = (yy < 0 ? 0 : yy) * k.cy + (1 << 19), u = U - 128, v = V - 128;
    rgb[0] = clip255((y + k.crv * v) >> 20);
    rgb[1] = clip255((y + k.cgu * u + k.cgv * v) >> 20);
    rgb[2] = clip255((y + k.cbu * u) >> 20);
}

// bytes of one row of plane p (0 / 1) of a w-pixel-wide frame, and that plane's row count for h frame rows
PF_HD int64_t plane_row_bytes(int format, int plane, int64_t w) {
    if (format == PIX_NV12) return plane == 0 ? w : 2 * ((w + 1) / 2);
    return plane == 0 ? 3 * w : 0;
}
PF_HD int64_t plane_rows(int format, int plane, int64_t h) {
    if (plane == 0) return h;
    return format == PIX_NV12 ? (h + 1) / 2 : 0;
}

}  // namespace vp
