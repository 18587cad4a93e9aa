// The box tracker of VitInference(is_video=True) -- SORT: a constant-velocity Kalman filter per track on (centre x, centre y, area, aspect ratio) and an
// assignment on the IoU between detections and predicted boxes -- for ONE track, ONE pair, ONE column each.  Shared by the device kernels of
// vp_tracker_update_stream (track.hip) and the host-only taps vp_dbg_track_host / vp_dbg_lsap(-1), so that the CPU tests of the taps pin the arithmetic the
// device runs, as posenms.h does for the pose NMS.  A restatement of easy_vitpose_amd/tracker.py, which stays the Python twin.
//
// All arithmetic is fp64 and nothing is contracted: the pragma below holds to the end of the translation unit that includes this header (track.hip holds the
// tracker and nothing else), and because the backend fuses regardless of the pragma under -ffp-contract=fast, build.py compiles track.hip with
// -ffp-contract=off (SOURCE_FLAGS).  fp64 square roots and divisions are correctly rounded on the host and on gfx950.  So the device and the host tap agree
// bit for bit.  They do not agree bit for bit with numpy / LAPACK: see trk_update.
//
//   state    x[7] = (cx, cy, area, ratio, vcx, vcy, varea), P[7][7], score, id (0-based; reported + 1), time_since_update, hit_streak, hits, age
//   predict  x[6] = 0 if x[6] + x[2] <= 0;  x = F x;  P = F P F^T + Q  with F = I + (position += velocity): every sum has two non-zero terms, so this IS
//            numpy's result;  age += 1;  hit_streak = 0 if time_since_update > 0;  time_since_update += 1;  the predicted box = x_to_box(x)
//   update   y = z - x[:4];  S = P[:4,:4] + R;  S^-1 by Gauss-Jordan without pivoting (S is symmetric positive definite), columns 0..3 in order: the pivot row
//            is DIVIDED by the pivot, then taken times the column entry from every other row;  K = P[:, :4] S^-1;  x += K y;  Joseph form
//            P = (I - K H) P (I - K H)^T + K R K^T with I - K H applied as the rank-4 correction it is: A = P - K P[:4, :], P = A - A[:, :4] K^T + K R K^T,
//            every sum in index order.  R = diag(1, 1, 10, 10), Q = diag(1, 1, 1, 1, .01, .01, 1e-4), P0 = diag(10 x 4, 1e4 x 3)
//   box_to_z (x1 + w / 2, y1 + h / 2, w h, w / h);  x_to_box: w = sqrt(x2 x3), h = x2 / w, (cx -+ w / 2, cy -+ h / 2)
//   iou      inter / union, 0 where the union is not > 0 (a zero-area pair)
//   associate (tracker.associate) over iou [nd, nt]:  if every row and every column of iou > thr holds at most one entry, those entries are the pairs (the
//            unambiguous shortcut: NOT the optimum in general);  otherwise the exact rectangular linear-sum assignment that maximises the total IoU: shortest
//            augmenting paths with fp64 duals over cost = -iou, rows = the smaller side.  One augmentation per row, at most max(nd, nt) column scans each; a
//            scan settles the open column that is first in (reduced path cost, unassigned before assigned, lower column): lsap_before.  Pairs with
//            iou < thr are dropped.  Births = the unmatched detections in detection-index order.
//   report   time_since_update < 1 and (hit_streak >= min_hits or frame_count <= min_hits);  a call without detections reports every listed track's predicted
//            box;  rows in reversed track-list order;  then tracks with time_since_update > max_age leave the list.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace vp {

constexpr int TRK_MAX = 128;           // VP_TRACK_MAX: live tracks per stream, detections per stream and call
constexpr int TRK_MAX_STREAMS = 64;    // VP_TRACK_MAX_STREAMS
constexpr int TRK_LD = TRK_MAX + 1;    // row pitch of the assignment matrix in doubles: a column walk by consecutive lanes touches consecutive LDS banks

constexpr int TRK_FLAG_DETS = 1, TRK_FLAG_BIRTHS = 2, TRK_FLAG_ROWS = 4, TRK_FLAG_BAD_ROW = 8;

struct TrkParams {
    int32_t max_age, min_hits;
    float iou_thr;
    int32_t n_streams;
};

// The state as vp_tracker_download_state returns it: TrkStream [n_streams].  rep / rep_id = the report rows of the stream's last step in fp64, rows [0, n_rows).
struct TrkTrack {
    double x[7], P[49], score;
    int32_t id, tsu, streak, hits, age, pad;
};
struct TrkStream {
    int32_t n_tracks, frame_count, next_id, n_rows, flags, pad[3];
    TrkTrack trk[TRK_MAX];
    double rep[TRK_MAX][5];   // x1 y1 x2 y2 score
    int32_t rep_id[TRK_MAX];  // id + 1
};
static_assert(sizeof(TrkTrack) == 480 && sizeof(TrkStream) == 32 + 480 * TRK_MAX + 40 * TRK_MAX + 4 * TRK_MAX, "the state layout is part of the test surface");

__host__ __device__ inline bool trk_finite(double v) { return v - v == 0.0; }
// Which NaN an invalid operation returns (sign, payload) differs between the host and the device: every NaN that can reach the state or a report row -- the
// ratio of a zero-area detection and the box of such a track -- is stored as the one quiet NaN of the NAN macro, so that state and rows stay comparable byte by byte.
__host__ __device__ inline double trk_canon(double v) { return v != v ? (double)NAN : v; }

__host__ __device__ inline double trk_iou(const double* d, const double* t) {
    double w = fmin(d[2], t[2]) - fmax(d[0], t[0]), h = fmin(d[3], t[3]) - fmax(d[1], t[1]);
    w = w > 0.0 ? w : 0.0;
    h = h > 0.0 ? h : 0.0;
    const double inter = w * h;
    const double uni = (d[2] - d[0]) * (d[3] - d[1]) + (t[2] - t[0]) * (t[3] - t[1]) - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

__host__ __device__ inline void trk_box_to_z(const double* b, double* z) {
    const double w = b[2] - b[0], h = b[3] - b[1];
    z[0] = b[0] + w / 2.0;
    z[1] = b[1] + h / 2.0;
    z[2] = w * h;
    z[3] = trk_canon(w / h);
}

__host__ __device__ inline void trk_x_to_box(const double* x, double* b) {
    const double w = sqrt(x[2] * x[3]);
    const double h = x[2] / w;
    b[0] = trk_canon(x[0] - w / 2.0);
    b[1] = trk_canon(x[1] - h / 2.0);
    b[2] = trk_canon(x[0] + w / 2.0);
    b[3] = trk_canon(x[1] + h / 2.0);
}

__host__ __device__ inline bool trk_box_finite(const double* b) { return trk_finite(b[0]) && trk_finite(b[1]) && trk_finite(b[2]) && trk_finite(b[3]); }

__host__ __device__ inline double trk_q(int i) { return i < 4 ? 1.0 : (i < 6 ? 0.01 : 1e-4); }
__host__ __device__ inline double trk_r(int i) { return i < 2 ? 1.0 : 10.0; }

__host__ __device__ inline void trk_init(TrkTrack& t, const double* det, int32_t id) {
    trk_box_to_z(det, t.x);
    t.x[4] = t.x[5] = t.x[6] = 0.0;
#pragma unroll
    for (int i = 0; i < 49; ++i) t.P[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) t.P[i * 7 + i] = i < 4 ? 10.0 : 1e4;
    t.score = det[4];
    t.id = id;
    t.tsu = t.streak = t.hits = t.age = t.pad = 0;
}

__host__ __device__ inline void trk_predict(TrkTrack& t, double* box) {
    if (t.x[6] + t.x[2] <= 0.0) t.x[6] = 0.0;   // the area must not go negative
#pragma unroll
    for (int i = 0; i < 3; ++i) t.x[i] = t.x[i] + t.x[i + 4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) t.P[i * 7 + j] = t.P[i * 7 + j] + t.P[(i + 4) * 7 + j];   // F P
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) t.P[i * 7 + j] = t.P[i * 7 + j] + t.P[i * 7 + j + 4];     // (F P) F^T
#pragma unroll
    for (int i = 0; i < 7; ++i) t.P[i * 7 + i] = t.P[i * 7 + i] + trk_q(i);
    t.age += 1;
    if (t.tsu > 0) t.streak = 0;
    t.tsu += 1;
    trk_x_to_box(t.x, box);
}

__host__ __device__ inline void trk_update(TrkTrack& t, const double* det) {
    t.tsu = 0;
    t.hits += 1;
    t.streak += 1;
    double z[4], y[4], G[4][8];
    trk_box_to_z(det, z);
#pragma unroll
    for (int a = 0; a < 4; ++a) y[a] = z[a] - t.x[a];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            G[a][b] = a == b ? t.P[a * 7 + b] + trk_r(a) : t.P[a * 7 + b];
            G[a][b + 4] = a == b ? 1.0 : 0.0;
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // [S | I] -> [I | S^-1]
        const double piv = G[k][k];
#pragma unroll
        for (int c = 0; c < 8; ++c) G[k][c] = G[k][c] / piv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == k) continue;
            const double f = G[r][k];
#pragma unroll
            for (int c = 0; c < 8; ++c) G[r][c] = G[r][c] - f * G[k][c];
        }
    }
    double K[7][4];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) s = s + t.P[i * 7 + a] * G[a][b + 4];
            K[i][b] = s;
        }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) s = s + K[i][b] * y[b];
        t.x[i] = t.x[i] + s;
    }
    double A[49];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s = s + K[i][k] * t.P[k * 7 + j];
            A[i * 7 + j] = t.P[i * 7 + j] - s;
        }
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            double s = 0.0, q = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s = s + A[i * 7 + k] * K[j][k];
                q = q + K[i][k] * trk_r(k) * K[j][k];
            }
            t.P[i * 7 + j] = A[i * 7 + j] - s + q;
        }
    t.score = det[4];
}

__host__ __device__ inline bool trk_reported(const TrkTrack& t, int frame_count, int min_hits) { return t.tsu < 1 && (t.streak >= min_hits || frame_count <= min_hits); }

// the assignment's column scan: the reduced cost of reaching column j through row i, and the order in which an open column is settled
// (f = 1: the column is assigned to a row; j = INT32_MAX with key +infinity is "no open column")
__host__ __device__ inline double lsap_reduced(double min_val, double iou, double u, double v) { return min_val + (-iou) - u - v; }
__host__ __device__ inline bool lsap_before(double ka, int32_t fa, int32_t ja, double kb, int32_t fb, int32_t jb) {
    return ka < kb || (ka == kb && (fa < fb || (fa == fb && ja < jb)));
}

}  // namespace vp
