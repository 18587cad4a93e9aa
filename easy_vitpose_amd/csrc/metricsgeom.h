// Accuracy metrics against ground truth as an accumulating device stage (vp_metrics_*): the reference's vit_utils/top_down_eval.py _calc_distances / _distance_acc /
// keypoint_pck_accuracy / keypoint_auc / keypoint_nme / keypoint_epe and post_processing/nms.py oks_iou read as "ground truth against detected", for ONE row and
// joint each, plus the summation order of a call.  Shared by the kernels (metrics.hip) and the host tap vp_dbg_metrics_host, as collectgeom.h and eurogeom.h are;
// easy_vitpose_amd/devmetrics.py metrics_numpy is the numpy twin.  The unit is compiled with -ffp-contract=off: every float32 / fp64 operation below is rounded on
// its own, division and square root are correctly rounded.
//
//   pred float32 [n, K, 3] rows of (y, x, conf); gt float32 [n, K, 3] rows of (y, x, v); 0 <= n <= METRICS_MAX_ROWS, 1 <= K <= NMS_MAX_K.  Optional, each may be
//   NULL: norm float32 [n, 2] in (y, x) order (NULL: 1.0 both); area float32 [n] (NULL: no OKS for this call); rank int32 [n] (the row counts iff rank >= 0);
//   set int32 [n] with the scalar set_value (the row counts iff equal).  A COUNTED row passes both filters.
//   Per joint j of a counted row:
//     visible   v > vis_thr in float32 (a NaN v is not visible);  dy = py - gy, dx = px - gx (float32)
//     qn        the normalised distance (PCK, NME; _calc_distances): the row is OFF for this family when a component of its norm == 0; otherwise a component <= 0
//               becomes 1e6f; qn = sqrtf((dy / n_y) (dy / n_y) + (dx / n_x) (dx / n_x)).  valid_norm[j] counts the visible joints of rows that are not off.
//     q1        the pixel distance (EPE; the reference calls _calc_distances with ones, so no row is off): sqrtf(dy dy + dx dx).  valid_px[j] counts visible joints.
//     qa        the AUC distance: keypoint_auc tiles a Python scalar into a float64 array, so the division and the norm are fp64 and the store into the float32
//               distance array rounds once: qa = (float)sqrt(((double)dy / A)^2 + ((double)dx / A)^2), A = auc_norm.  It counts against valid_px[j].
//     hits      pck_hits[t][j] += qn < pck_thr[t];  auc_hits[s][j] += qa < (float)((double)s / auc_steps): strict float32 comparisons (numpy compares the float32
//               array with a weak Python float).
//     sums      sum_norm[j] += (double)qn;  sum_px[j] += (double)q1, in the order below.
//     DEVIATION a non-finite distance is valid and never hits (what inf < thr and nan < thr give), but it is LEFT OUT of its sum and bumps `nonfinite` instead (once
//               for qn where the joint is in valid_norm, once for q1); finish() then reports NaN for the NME / EPE where the reference would report inf or NaN.
//   OKS of a counted row, with use_oks, area given, a = (double)area[i] finite and > 0 and at least one visible joint: over the visible joints in joint order
//     nms_oks_term(gt_row, pred_row, j, (2 sigma_j)^2, nms_oks_denom(a, a)) and nms_oks_mean of posenms.h; oks_rows += 1; oks_hits[t] += oks >= (float)(0.5 + 0.05 t),
//     t = 0..9; oks_sum += (double)oks; a non-finite oks bumps `nonfinite` instead of the three.  This is the share of instances recovered at OKS t with one
//     candidate per instance, NOT COCO AP.
//   Summation order (part of the contract: the state is a pure function of the inputs).  Rows form blocks of 64: b = i / 64, l = i % 64.  A row that does not
//     contribute gives +0.0.  A block's partial P(b) is the balanced binary tree over its 64 leaves in lane order -- pairs at distance 1, then 2, 4, ..., 32
//     (metrics_tree64; an xor butterfly gives the same value).  A call's sum is ((0.0 + P(0)) + P(1)) + ... in ascending block order, and the state takes
//     state + call_sum.  Per joint for sum_norm and sum_px, over rows for oks_sum.
//   State blob, 8-byte words (zeroed = new):  header 8: int64 calls, rows (sum of n), counted, nonfinite, oks_rows, 0, 0, 0 | OKS 16: int64 oks_hits[10], double
//     oks_sum, 0 x 5 | int64 valid_norm[K] | int64 valid_px[K] | double sum_norm[K] | double sum_px[K] | int64 pck_hits[n_pck][K] | int64 auc_hits[auc_steps][K].
//   Optional per-call outputs, every element written once per call: dist float32 [n, K] = qn, or -1 where the joint is not in valid_norm (the reference's
//     _calc_distances(...).T); oks float32 [n] = oks, or -1 where none.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "posenms.h"

namespace vp {

constexpr int METRICS_MAX_ROWS = 8192;                                  // VP_METRICS_MAX_ROWS
constexpr int METRICS_BLOCK = 64;                                       // rows per block of the summation order
constexpr int METRICS_MAX_BLOCKS = METRICS_MAX_ROWS / METRICS_BLOCK;    // 128
constexpr int METRICS_MAX_PCK = 8, METRICS_MAX_AUC = 32, METRICS_OKS_THRS = 10;
constexpr int METRICS_HDR_WORDS = 8, METRICS_OKS_WORDS = 16;
// header words
constexpr int METRICS_W_CALLS = 0, METRICS_W_ROWS = 1, METRICS_W_COUNTED = 2, METRICS_W_NONFINITE = 3, METRICS_W_OKS_ROWS = 4;
constexpr int METRICS_W_OKS_HITS = METRICS_HDR_WORDS, METRICS_W_OKS_SUM = METRICS_HDR_WORDS + METRICS_OKS_THRS;

struct MetricsParams {
    double auc_norm;
    float pck_thr[METRICS_MAX_PCK];
    float auc_thr[METRICS_MAX_AUC];   // (float)((double)s / auc_steps)
    float vis_thr;
    int32_t n_joints, n_pck, auc_steps, use_oks;
};

// word offsets of the per-joint parts
__host__ __device__ inline size_t metrics_w_valid_norm() { return METRICS_HDR_WORDS + METRICS_OKS_WORDS; }
__host__ __device__ inline size_t metrics_w_valid_px(int K) { return metrics_w_valid_norm() + (size_t)K; }
__host__ __device__ inline size_t metrics_w_sum_norm(int K) { return metrics_w_valid_norm() + 2 * (size_t)K; }
__host__ __device__ inline size_t metrics_w_sum_px(int K) { return metrics_w_valid_norm() + 3 * (size_t)K; }
__host__ __device__ inline size_t metrics_w_pck(int K) { return metrics_w_valid_norm() + 4 * (size_t)K; }
__host__ __device__ inline size_t metrics_w_auc(int K, int n_pck) { return metrics_w_pck(K) + (size_t)n_pck * K; }
__host__ __device__ inline size_t metrics_state_words(int K, int n_pck, int auc_steps) { return metrics_w_auc(K, n_pck) + (size_t)auc_steps * K; }
// the count kinds of a joint in the order the state holds them: 0 valid_norm, 1 valid_px, 2 + t pck_hits[t], 2 + n_pck + s auc_hits[s]
__host__ __device__ inline int metrics_count_kinds(const MetricsParams& p) { return 2 + p.n_pck + p.auc_steps; }
__host__ __device__ inline size_t metrics_w_count(int K, int kind) { return metrics_w_valid_norm() + (size_t)(kind < 2 ? kind : kind + 2) * K; }

__host__ __device__ inline bool metrics_finite(float v) { return v - v == 0.0f; }
__host__ __device__ inline bool metrics_finite(double v) { return v - v == 0.0; }

__host__ __device__ inline bool metrics_counted(const int32_t* rank, const int32_t* set, int32_t set_value, int i) {
    return (!rank || rank[i] >= 0) && (!set || set[i] == set_value);
}

// the normalisers of row i: false when the row is off for the normalised family
__host__ __device__ inline bool metrics_row_norm(const float* norm, int i, float& ny, float& nx) {
    ny = norm ? norm[2 * (size_t)i] : 1.0f;
    nx = norm ? norm[2 * (size_t)i + 1] : 1.0f;
    const bool on = !(ny == 0.0f || nx == 0.0f);
    if (ny <= 0.0f) ny = 1e6f;
    if (nx <= 0.0f) nx = 1e6f;
    return on;
}

struct MetricsJoint {
    bool vis;            // counts in valid_px
    bool in_norm;        // counts in valid_norm
    float qn, q1, qa;    // meaningful where the flag above says so (qa: where vis and auc_steps > 0)
};

// joint j of a counted row: p = the predicted row, g = the ground-truth row (K x 3 floats each)
__host__ __device__ inline MetricsJoint metrics_joint(const float* p, const float* g, int j, float ny, float nx, bool norm_on, const MetricsParams& m) {
    MetricsJoint r;
    r.vis = g[3 * j + 2] > m.vis_thr;
    r.in_norm = r.vis && norm_on;
    const float dy = p[3 * j] - g[3 * j], dx = p[3 * j + 1] - g[3 * j + 1];
    const float ry = dy / ny, rx = dx / nx;
    const float ryy = ry * ry, rxx = rx * rx;
    r.qn = sqrtf(ryy + rxx);
    const float yy = dy * dy, xx = dx * dx;
    r.q1 = sqrtf(yy + xx);
    r.qa = 0.0f;
    if (m.auc_steps > 0) {
        const double ay = (double)dy / m.auc_norm, ax = (double)dx / m.auc_norm;
        const double ayy = ay * ay, axx = ax * ax;
        r.qa = (float)sqrt(ayy + axx);
    }
    return r;
}

__host__ __device__ inline float metrics_oks_thr(int t) { const double s = 0.05 * (double)t; return (float)(0.5 + s); }
// OKS of this row is defined: the area as the OKS reads it
__host__ __device__ inline bool metrics_oks_area(const MetricsParams& m, const float* area, int i, double& a) {
    if (!m.use_oks || !area) return false;
    a = (double)area[i];
    return metrics_finite(a) && a > 0.0;
}

// HOST and twin side of the summation order: the balanced tree over 64 leaves in lane order, in place
inline double metrics_tree64(double* v) {
    for (int d = 1; d < METRICS_BLOCK; d *= 2)
        for (int i = 0; i < METRICS_BLOCK; i += 2 * d) v[i] = v[i] + v[i + d];
    return v[0];
}

}  // namespace vp
