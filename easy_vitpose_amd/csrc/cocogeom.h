// COCO keypoint AP / AR as an accumulating device stage (vp_cocoeval_*): COCOeval for iouType = 'keypoints' (computeOks, evaluateImg, accumulate) restated operation
// by operation with fixed parameters -- one category, maxDets = 20, the area ranges all / medium / large, the ten OKS thresholds and the 101 recall thresholds.
// Shared by the kernels (cocoeval.hip) and the host taps vp_dbg_cocoeval_update_host / vp_dbg_cocoeval_accumulate_host; easy_vitpose_amd/devcoco.py holds the numpy
// twin and finish(), which turns the result blob into the ten figures of summarize.  The unit is compiled with -ffp-contract=off: every fp64 operation below is
// rounded on its own.  UNPINNED: the pycocotools binary is not available to the tests, this is a restatement of its source.
//
//   Inputs of one update, coordinates in this project's (y, x, .) order: kpts float32 [n, K, 3], score float32 [n], frame int32 [n] (NULL: 0), rank int32 [n]
//   (optional: the row counts iff rank >= 0); gt_kpts float32 [g, K, 3] rows of (y, x, v), gt_box float32 [g, 4] rows of (x, y, w, h), gt_area float32 [g], gt_flags
//   int32 [g] (bit 0 = iscrowd; NULL: 0), gt_frame int32 [g] (NULL: 0); n_frames.  0 <= n, g <= 8192, 1 <= n_frames <= 256, 1 <= K <= NMS_MAX_K.  A row or gt whose
//   frame lies outside [0, n_frames) does not count; rows need not be grouped by frame.  At most 128 gts per image are used: later ones, in call order, are left out
//   and counted in gt_overflow.
//   Per image:
//     detections  the counted rows of the image ordered by score descending, equal scores to the lower row, a NaN score as -infinity (posenms.h nms_key /
//                 nms_before); the first 20 are KEPT.  area_d = (max x - min x) (max y - min y) over all K joints in fp64 (what loadRes computes); a NaN
//                 coordinate makes it NaN, as np.min / np.max do.
//     gts         k1 = the count of v > 0; ignore0 = iscrowd || k1 == 0.
//     oks(d, g)   fp64 on the float32 inputs converted exactly: vars_j = (2 sigma_j)^2 from HOST doubles; e_j = (dx^2 + dy^2) / vars_j / (area_g + 2^-52) / 2.
//                 k1 > 0: dx = xd - xg, dy = yd - yg over the joints with v > 0.  k1 == 0: the distance to the doubled box over all joints, x0 = bx - bw,
//                 x1 = bx + bw 2, dx = max(0, x0 - xd) + max(0, xd - x1), likewise y (max propagates a NaN as np.max does).  oks = sum of exp(-e_j) / count.
//                 DEVIATION: the sum runs in joint order, numpy's np.sum is pairwise: a few fp64 ulps.  DEVIATION: a non-finite oks never matches and bumps
//                 `nonfinite` (COCOeval would match a NaN).
//     matching    for each range a (all [0, 1e10], medium [32^2, 96^2], large [96^2, 1e10]) and threshold t (np.linspace(.5, .95, 10) as a literal table):
//                 ignore_g = ignore0 || area_g < lo || area_g > hi; the gts ordered stably, not-ignored first.  Walk the kept detections in order; start with best =
//                 min(thr, 1 - 1e-10); walk the gts in that order: skip a gt already matched at (a, t) unless it is a crowd; stop when the current match is a
//                 not-ignored gt and this gt is ignored; skip when oks < best; otherwise take this gt and set best = oks.  A matched detection inherits its gt's
//                 ignore flag; an unmatched one is ignored iff area_d < lo || area_d > hi.  npig[a] += the not-ignored gts.
//   Record, 16 bytes, one per kept detection: float32 score, uint32 matched (bit 10 a + t), uint32 ignored (same bits), uint32 image ordinal (state.images + frame);
//     appended in image order, inside an image in the kept order.  A record that does not fit into max_records is not written and counted in `dropped`.
//   d_match int32 [n, 10], optional: the gt row matched under range "all" at each threshold; -1 unmatched; -2 a row that is not among its image's kept 20 or does
//     not count.
//   State blob (zeroed = new): 16 int64 words calls, images, rows (sum of n), kept, records, dropped, gts (used), gt_overflow, nonfinite, npig[3], 0 x 4, then the
//     record table [max_records].  A pure function of the inputs and the sequence of calls, byte for byte.
//   Accumulate: the records ordered by score descending (NaN as -infinity, -0 == +0), equal scores by table position -- a unique key, so the result does not depend
//     on the sorting method; it is COCOeval's stable argsort(-score) when the images are fed in ascending id order.  Per (a, t) in that order: integer cumulative
//     tp (matched, not ignored) and fp (unmatched, not ignored); rc = tp / npig, pr = tp / (fp + tp + 2^-52) in fp64; the precision envelope from the back; for each
//     recall threshold (double)k (1.0 / 100.0), k = 0..100 (== np.linspace(0, 1, 101) bit for bit), the first position with rc >= thr gives precision[a][t][k], 0 when
//     there is none; recall[a][t] = the last rc, 0 without records; npig[a] == 0 gives -1 everywhere.
//   Result blob: the 16 header words | double precision [3][10][101] | double recall [3][10].
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "posenms.h"

namespace vp {

constexpr int COCO_MAX_ROWS = 8192, COCO_MAX_GTS = 8192, COCO_MAX_FRAMES = 256;   // VP_COCOEVAL_MAX_*
constexpr int COCO_MAX_DETS = 20, COCO_IMG_GTS = 128;
constexpr int COCO_AREAS = 3, COCO_THRS = 10, COCO_AT = COCO_AREAS * COCO_THRS, COCO_RECS = 101;
constexpr int COCO_MAX_RECORDS = 1 << 20;
constexpr int COCO_HDR_WORDS = 16;
constexpr int COCO_W_CALLS = 0, COCO_W_IMAGES = 1, COCO_W_ROWS = 2, COCO_W_KEPT = 3, COCO_W_RECORDS = 4, COCO_W_DROPPED = 5, COCO_W_GTS = 6, COCO_W_GT_OVERFLOW = 7,
              COCO_W_NONFINITE = 8, COCO_W_NPIG = 9;
constexpr int COCO_RESULT_DOUBLES = COCO_AT * COCO_RECS + COCO_AT;
constexpr double COCO_EPS = 2.220446049250313e-16;   // np.spacing(1) = 2^-52

struct CocoRecord {
    float score;
    uint32_t matched, ignored, image;
};

__host__ __device__ inline size_t coco_state_bytes(int max_records) { return (size_t)COCO_HDR_WORDS * 8 + (size_t)max_records * sizeof(CocoRecord); }
__host__ __device__ inline size_t coco_result_bytes() { return (size_t)COCO_HDR_WORDS * 8 + (size_t)COCO_RESULT_DOUBLES * 8; }

// np.linspace(.5, .95, 10), the doubles numpy produces: not 0.5 + 0.05 t (entry 8)
__host__ __device__ inline double coco_oks_thr(int t) {
    switch (t) {
        case 0: return 0.5;
        case 1: return 0.55;
        case 2: return 0.6;
        case 3: return 0.65;
        case 4: return 0.7;
        case 5: return 0.75;
        case 6: return 0.8;
        case 7: return 0.85;
        case 8: return 0.8999999999999999;
        default: return 0.95;
    }
}
// np.linspace(0, 1, 101) bit for bit (k / 100.0 is not)
__host__ __device__ inline double coco_rec_thr(int k) { return (double)k * (1.0 / 100.0); }
__host__ __device__ inline double coco_area_lo(int a) { return a == 0 ? 0.0 : (a == 1 ? 1024.0 : 9216.0); }
__host__ __device__ inline double coco_area_hi(int a) { return a == 1 ? 9216.0 : 1e10; }
__host__ __device__ inline bool coco_outside(double area, int a) { return area < coco_area_lo(a) || area > coco_area_hi(a); }

__host__ __device__ inline bool coco_finite(double v) { return v - v == 0.0; }
__host__ __device__ inline bool coco_counted(const int32_t* rank, const int32_t* frame, int i, int n_frames, int& f) {
    f = frame ? frame[i] : 0;
    return (!rank || rank[i] >= 0) && f >= 0 && f < n_frames;
}
__host__ __device__ inline int coco_gt_frame(const int32_t* gt_frame, int j) { return gt_frame ? gt_frame[j] : 0; }

// np.min / np.max steps: a NaN sticks
__host__ __device__ inline double coco_min(double m, double v) { return (v < m || v != v) ? v : m; }
__host__ __device__ inline double coco_max(double m, double v) { return (v > m || v != v) ? v : m; }
__host__ __device__ inline double coco_max0(double v) { return coco_max(0.0, v); }

// the detection's area as loadRes computes it: d = the row, K x 3 floats of (y, x, .)
__host__ __device__ inline double coco_det_area(const float* d, int K) {
    double y0 = (double)d[0], y1 = y0, x0 = (double)d[1], x1 = x0;
    for (int j = 1; j < K; ++j) {
        const double y = (double)d[3 * j], x = (double)d[3 * j + 1];
        y0 = coco_min(y0, y); y1 = coco_max(y1, y);
        x0 = coco_min(x0, x); x1 = coco_max(x1, x);
    }
    const double w = x1 - x0, h = y1 - y0;
    return w * h;
}

__host__ __device__ inline int coco_k1(const float* g, int K) {
    int k1 = 0;
    for (int j = 0; j < K; ++j) k1 += g[3 * j + 2] > 0.0f;
    return k1;
}

// computeOks for one pair: d, g = the rows, box = (x, y, w, h) of the gt, area = the gt's, k1 = coco_k1(g)
__host__ __device__ inline double coco_oks(const float* d, const float* g, const float* box, double area, int k1, int K, const double* vars) {
    const double aeps = area + COCO_EPS;
    double sum = 0.0;
    if (k1 > 0) {
        for (int j = 0; j < K; ++j) {
            if (!(g[3 * j + 2] > 0.0f)) continue;
            const double dy = (double)d[3 * j] - (double)g[3 * j], dx = (double)d[3 * j + 1] - (double)g[3 * j + 1];
            const double xx = dx * dx, yy = dy * dy;
            const double e = (xx + yy) / vars[j] / aeps / 2.0;
            sum = sum + exp(-e);
        }
        return sum / (double)k1;
    }
    const double bx = (double)box[0], by = (double)box[1], bw = (double)box[2], bh = (double)box[3];
    const double x0 = bx - bw, x1 = bx + bw * 2.0, y0 = by - bh, y1 = by + bh * 2.0;
    for (int j = 0; j < K; ++j) {
        const double yd = (double)d[3 * j], xd = (double)d[3 * j + 1];
        const double dx = coco_max0(x0 - xd) + coco_max0(xd - x1), dy = coco_max0(y0 - yd) + coco_max0(yd - y1);
        const double xx = dx * dx, yy = dy * dy;
        const double e = (xx + yy) / vars[j] / aeps / 2.0;
        sum = sum + exp(-e);
    }
    return sum / (double)K;
}

// evaluateImg's walk for one (range, threshold) over D kept detections and G gts.  oks [D][ld]: a non-finite value stored as -1 never matches; order [G] = the gts,
// not-ignored first; ign [G], crowd [G] by gt.  Calls out(d, m) with m = the matched gt or -1, in detection order.
template <class OksAt, class U8, class Out>
__host__ __device__ inline void coco_walk(int D, int G, double thr, OksAt oks, const U8* order, const U8* ign, const U8* crowd, Out out) {
    uint64_t m0 = 0, m1 = 0;   // the gts matched at this (range, threshold): 128 bits
    const double start = thr < 1.0 - 1e-10 ? thr : 1.0 - 1e-10;
    for (int d = 0; d < D; ++d) {
        double best = start;
        int m = -1;
        for (int q = 0; q < G; ++q) {
            const int j = order[q];
            const bool taken = ((j < 64 ? m0 >> j : m1 >> (j - 64)) & 1) != 0;
            if (taken && !crowd[j]) continue;
            if (m > -1 && !ign[m] && ign[j]) break;
            const double o = oks(d, j);
            if (o < best) continue;
            best = o;
            m = j;
        }
        if (m > -1) {
            if (m < 64) m0 |= 1ull << m;
            else m1 |= 1ull << (m - 64);
        }
        out(d, m);
    }
}

// the sort key of a record: ascending key == score descending (NaN as -infinity, -0 == +0), then table position
__host__ __device__ inline uint64_t coco_sort_key(float score, uint32_t pos) {
    float s = score != score ? -INFINITY : score;
    if (s == 0.0f) s = 0.0f;
    union { float f; uint32_t u; } c;
    c.f = s;
    const uint32_t up = (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);   // ascending in the float's order
    return ((uint64_t)(~up) << 32) | pos;
}

__host__ __device__ inline double coco_recall(int64_t tp, int64_t npig) { return (double)tp / (double)npig; }
__host__ __device__ inline double coco_precision(int64_t tp, int64_t fp) { return (double)tp / (((double)fp + (double)tp) + COCO_EPS); }
// the first k with coco_rec_thr(k) > rc (101 when none), rc in [0, 1]
__host__ __device__ inline int coco_first_thr_above(double rc) {
    int k = (int)(rc * 100.0);
    k = k < 0 ? 0 : (k > COCO_RECS ? COCO_RECS : k);
    while (k < COCO_RECS && coco_rec_thr(k) <= rc) ++k;
    while (k > 0 && coco_rec_thr(k - 1) > rc) --k;
    return k;
}

}  // namespace vp
