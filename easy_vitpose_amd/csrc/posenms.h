// Person scores and OKS pose NMS of the reference (vit_utils/post_processing/nms.py oks_iou / oks_nms / soft_oks_nms, parameters of
// configs/ViTPose_common.py data_cfg: oks_thr, vis_thr, soft_nms), for ONE value each.  Shared by the device kernels of vp_pose_nms_stream
// (posenms.hip) and the host-only taps vp_dbg_pose_nms_host / vp_dbg_pose_oks(-1), so that the CPU tests of the taps pin the arithmetic the device
// runs, as boxgeom.h does for the box geometry.
//
// A row is one person: keypoints [K, 3] (y, x, conf) float32 in frame pixels, a box score, a frames_crop_params row {frame, x0, y0, cw, ch, ...}.
//   area    = (double)cw * (double)ch                      (the padded, clipped box)
//   score   = (float)(mean of conf over the joints with conf > vis_thr (0 if none), fp64 in joint order, times (double)box_score)
//   oks(d | g), candidate d against pick g, nms.py:51-86 with its arithmetic widths: dx = xd - xg, dy = yd - yg and dx*dx + dy*dy are float32
//             roundings each (numpy on float32 arrays; the pragma below keeps -ffp-contract=fast from fusing them), then in fp64
//             e_j = that / (2 sigma_j)^2 / ((a_g + a_d) / 2 + 2^-52) / 2,  oks = (float)(sum_j exp(-e_j) / count), sum in joint order, 0 with no joint.
//             The visibility gate keeps joint j when the CANDIDATE's conf_j > vis_thr: the reference writes `list(vg > t) and list(vd > t)`, and
//             Python's `and` of two non-empty lists IS the second list, so the pick's confidences never enter.  That is kept.
//   order   = the live row with the highest score is picked; equal scores go to the LOWER row.  (Deviation: the reference's order on ties is
//             whatever argsort()[::-1] leaves, an artefact of numpy's sort.)  A NaN score orders as -infinity.
//   hard    = every live row with oks > (float)oks_thr dies, compared in float32 as numpy does.
//   soft    = every live row's score (fp64) *= exp(-(double)oks * (double)oks / (double)(float)oks_thr)   (nms.py:150, 'gaussian')
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace vp {

constexpr int NMS_MAX_PER_FRAME = 1024;   // VP_NMS_MAX_PER_FRAME
constexpr int NMS_MAX_K = 256;            // VP_NMS_MAX_K

struct NmsParams {
    float oks_thr, vis_thr;
    int32_t use_vis_thr, soft, max_dets;
};
struct NmsVars { double v[NMS_MAX_K]; };   // (2 sigma_j)^2, by kernel argument (2 KiB)

__host__ __device__ inline double nms_var(float sigma) { const double s2 = 2.0 * (double)sigma; return s2 * s2; }

// a member of frame p9[0]'s NMS: a good row on a frame of the table
__host__ __device__ inline bool nms_member(int32_t status, int32_t frame, int32_t n_frames) { return status == 0 && frame >= 0 && frame < n_frames; }

__host__ __device__ inline double nms_area(const int32_t* p9) { return (double)p9[3] * (double)p9[4]; }

__host__ __device__ inline float nms_instance_score(const float* kp, int K, float box_score, const NmsParams& p) {
    double sum = 0.0;
    int cnt = 0;
    for (int j = 0; j < K; ++j) {
        const float c = kp[3 * j + 2];
        if (!p.use_vis_thr || c > p.vis_thr) { sum += (double)c; ++cnt; }
    }
    const double kpt = cnt ? sum / (double)cnt : 0.0;
    return (float)(kpt * (double)box_score);
}

// oks in three steps, so that the kernel can spread the terms of a candidate over lanes and still add them in joint order:
//   denom = (a_g + a_d) / 2 + np.spacing(1);  term_j = exp(-e_j) for a joint that passes the gate;  oks = (float)(sum of the terms in joint order / their count)
__host__ __device__ inline double nms_oks_denom(double a_g, double a_d) { return (a_g + a_d) / 2.0 + 2.220446049250313e-16; }   // np.spacing(1) = 2^-52
__host__ __device__ inline bool nms_oks_gate(const float* d, int j, const NmsParams& p) { return !p.use_vis_thr || d[3 * j + 2] > p.vis_thr; }
__host__ __device__ inline double nms_oks_term(const float* g, const float* d, int j, double var, double denom) {
#pragma clang fp contract(off)
    const float dy = d[3 * j] - g[3 * j], dx = d[3 * j + 1] - g[3 * j + 1];
    const float xx = dx * dx, yy = dy * dy;
    const float d2 = xx + yy;
    const double e = (double)d2 / var / denom / 2.0;
    return exp(-e);
}
__host__ __device__ inline float nms_oks_mean(double sum, int cnt) { return cnt ? (float)(sum / (double)cnt) : 0.f; }

__host__ __device__ inline float nms_oks(const float* g, const float* d, int K, double a_g, double a_d, const double* vars, const NmsParams& p) {
    const double denom = nms_oks_denom(a_g, a_d);
    double sum = 0.0;
    int cnt = 0;
    for (int j = 0; j < K; ++j) {
        if (!nms_oks_gate(d, j, p)) continue;
        sum += nms_oks_term(g, d, j, vars[j], denom);
        ++cnt;
    }
    return nms_oks_mean(sum, cnt);
}

__host__ __device__ inline double nms_soft_factor(float oks, float oks_thr) { return exp(-((double)oks * (double)oks) / (double)oks_thr); }

// the pick's order: (score, member) a before b.  Members are in ascending row order, so the lower member is the lower row.  NaN -> -infinity makes
// the order total, hence the workgroup reduction's result independent of its shape.  m = INT32_MAX with key -infinity is "no live member".
__host__ __device__ inline double nms_key(double score) { return score != score ? -INFINITY : score; }
__host__ __device__ inline bool nms_before(double ka, int32_t ma, double kb, int32_t mb) { return ka > kb || (ka == kb && ma < mb); }

}  // namespace vp
