// Box -> crop geometry of VitInference.inference (easy_ViTPose/inference.py:261-262 and pad_image, vit_utils/inference.py:41-70) as
// easy_vitpose_amd/cropprep.py::crop_params computes it, for ONE box.  Shared by the device kernel of vp_infer_boxes_stream (boxes.hip)
// and the host-only tap vp_dbg_box_geometry, so that the CPU test of the tap pins the arithmetic the device runs.
//
// crop_params on float64 boxes:  b = box.round().astype(int)  (numpy round = round half to even = rint)
//   x0, x1 = clip([b0 - pad, b2 + pad], 0, W);  y0, y1 = clip([b1 - pad, b3 + pad], 0, H);  cw, ch = x1 - x0, y1 - y0  ('empty box' unless > 0)
//   cw / ch < 0.75:  pw = int(0.75 * ch), left = (pw - cw) // 2     else:  ph = int(cw / 0.75), top = (ph - ch) // 2
// Here everything up to the clip stays in double and the clip comes BEFORE the conversion to int, so that every finite input has a defined
// result (a box from -1e30 to 1e30 is a full-width crop); it equals the numpy result wherever numpy's astype(int) is itself defined
// (|coordinate| < 2^30 is what the tests sweep).  Both floor divisions have a non-negative dividend (the branch condition makes pw >= cw and
// ph >= ch), so C's truncating division is Python's //.  Frame sides are at most BOX_MAX_SIDE (checked on the host), so pw, ph fit int32.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace vp {

enum BoxStatus { BOX_OK = 0, BOX_BAD_FRAME = 1, BOX_NOT_FINITE = 2, BOX_EMPTY = 3 };
constexpr int32_t BOX_MAX_SIDE = 1 << 24;

// box (x1, y1, x2, y2) on a frame of fh x fw pixels -> p8 = {x0, y0, cw, ch, left, top, pw, ph}; returns a BoxStatus (p8 untouched unless BOX_OK)
__host__ __device__ inline int box_geometry(float bx1, float by1, float bx2, float by2, int32_t fh, int32_t fw, int32_t pad, int32_t* p8) {
    const double x1 = bx1, y1 = by1, x2 = bx2, y2 = by2;
    if (!isfinite(x1) || !isfinite(y1) || !isfinite(x2) || !isfinite(y2)) return BOX_NOT_FINITE;
    const double W = fw, H = fh;
    const double cx0 = fmin(fmax(rint(x1) - pad, 0.0), W), cx1 = fmin(fmax(rint(x2) + pad, 0.0), W);
    const double cy0 = fmin(fmax(rint(y1) - pad, 0.0), H), cy1 = fmin(fmax(rint(y2) + pad, 0.0), H);
    const int32_t x0 = (int32_t)cx0, y0 = (int32_t)cy0, cw = (int32_t)cx1 - x0, ch = (int32_t)cy1 - y0;
    if (cw <= 0 || ch <= 0) return BOX_EMPTY;
    int32_t left = 0, top = 0, pw = cw, ph = ch;
    if ((double)cw / (double)ch < 0.75) {
        pw = (int32_t)(0.75 * (double)ch);
        left = (pw - cw) / 2;
    } else {
        ph = (int32_t)((double)cw / 0.75);
        top = (ph - ch) / 2;
    }
    p8[0] = x0; p8[1] = y0; p8[2] = cw; p8[3] = ch; p8[4] = left; p8[5] = top; p8[6] = pw; p8[7] = ph;
    return BOX_OK;
}

}  // namespace vp
