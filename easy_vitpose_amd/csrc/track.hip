// vp_tracker_*: the box tracker (SORT) as a stream-ordered device stage in front of the boxes entry (semantics: sortgeom.h), its synchronous host twin
// vp_tracker_update and the two taps vp_dbg_track_host / vp_dbg_lsap.  Two launches per call: track_update_kernel, one workgroup per stepped stream, and
// track_gather_kernel, one workgroup.  vp_tracker_update_counted_stream is the same call with the detection count read from device memory.  No atomics, no flags between workgroups, every reduction in a fixed order: a call is bit-identical from run to run.
#include "api_internal.h"
#include "hoststage.h"
#include "stageobj.h"
#include "sortgeom.h"

using namespace vpi;

struct vp_tracker : StageObj {
    vp::TrkParams p{};
    vp::TrkStream* state = nullptr;   // device [n_streams]
};

namespace vp {

constexpr int TRK_THREADS = TRK_MAX, TRK_WAVES = TRK_THREADS / 64, GATHER_THREADS = 256;

// The LDS of one stream's step (about 146 KiB of the 160 KiB a workgroup may declare).  M = the assignment matrix, rows = the smaller of (detections, tracks):
// M[r * TRK_LD + c] = iou of (detection r, track c), or of (detection c, track r) when there are more detections than tracks.
struct TrkLds {
    double M[TRK_MAX * TRK_LD];
    double det[TRK_MAX][5], tbox[TRK_MAX][4];
    double u[TRK_MAX];
    double wkey[2][TRK_WAVES];
    int32_t wf[2][TRK_WAVES], wj[2][TRK_WAVES];
    int32_t r4c[TRK_MAX], c4r[TRK_MAX], path[TRK_MAX], tod[TRK_MAX], dot[TRK_MAX], birth[TRK_MAX];
    int32_t wcnt[TRK_WAVES];
};

// exclusive prefix of `flag` over the workgroup in thread order, and the total (two barriers; every thread calls it)
__device__ inline int wg_prefix(TrkLds& L, bool flag, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) L.wcnt[wave] = __popcll(b);
    __syncthreads();
    int off = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
    for (int w = 0; w < TRK_WAVES; ++w) {
        if (w < wave) off += L.wcnt[w];
        all += L.wcnt[w];
    }
    __syncthreads();
    total = all;
    return off;
}

// tracker.associate on L.M [nr, nc] (nr <= nc <= TRK_MAX): L.c4r[r] = the column paired with row r, or -1.  Every thread of the workgroup calls it; thread j
// owns column j.  Every loop is bounded by construction: nr augmentations of at most nc scans, an augmenting path of at most nr + 1 columns.
__device__ inline void associate_lanes(TrkLds& L, int nr, int nc, double thr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the shortcut: every row and every column of M > thr holds at most one entry
    int cc = 0, rc = 0, only = -1;
    if (tid < nc)
        for (int r = 0; r < nr; ++r) cc += L.M[r * TRK_LD + tid] > thr;
    if (tid < nr)
        for (int c = 0; c < nc; ++c)
            if (L.M[tid * TRK_LD + c] > thr) { ++rc; only = c; }
    const int ambiguous = __syncthreads_or(cc > 1 || rc > 1);
    if (!ambiguous) {
        if (tid < nr) L.c4r[tid] = only;
    } else {
        double v = 0.0;
        if (tid < nr) { L.u[tid] = 0.0; L.c4r[tid] = -1; }
        if (tid < nc) L.r4c[tid] = -1;
        __syncthreads();
        for (int cur = 0; cur < nr; ++cur) {
            double spc = INFINITY, min_val = 0.0;
            bool sc = false;
            int32_t path = -1, i = cur, sink = -1;
            for (int step = 0; step < nc; ++step) {
                const double ui = L.u[i];
                double bk = INFINITY;
                int32_t bf = 1, bj = INT32_MAX;
                if (tid < nc && !sc) {
                    const double r = lsap_reduced(min_val, L.M[i * TRK_LD + tid], ui, v);
                    if (r < spc) { spc = r; path = i; }
                    if (spc < INFINITY) { bk = spc; bf = L.r4c[tid] != -1; bj = tid; }
                }
                for (int d = 32; d > 0; d >>= 1) {
                    const double ok = __shfl_xor(bk, d);
                    const int32_t of = __shfl_xor(bf, d), oj = __shfl_xor(bj, d);
                    if (lsap_before(ok, of, oj, bk, bf, bj)) { bk = ok; bf = of; bj = oj; }
                }
                const int buf = step & 1;   // two buffers: the next scan's writes never meet this scan's reads, one barrier per scan
                if (lane == 0) { L.wkey[buf][wave] = bk; L.wf[buf][wave] = bf; L.wj[buf][wave] = bj; }
                __syncthreads();
                bk = L.wkey[buf][0]; bf = L.wf[buf][0]; bj = L.wj[buf][0];
                for (int w = 1; w < TRK_WAVES; ++w)
                    if (lsap_before(L.wkey[buf][w], L.wf[buf][w], L.wj[buf][w], bk, bf, bj)) { bk = L.wkey[buf][w]; bf = L.wf[buf][w]; bj = L.wj[buf][w]; }
                if (bj == INT32_MAX) break;   // no finite path (a NaN in the matrix): this row stays unpaired
                min_val = bk;
                if (tid == bj) sc = true;
                if (bf == 0) { sink = bj; break; }
                i = L.r4c[bj];
            }
            if (sink >= 0) {
                if (tid < nc && sc) {   // the duals: the scanned columns and the rows they are assigned to (one row per column: no two threads meet)
                    const double d = min_val - spc;
                    if (tid != sink) L.u[L.r4c[tid]] = L.u[L.r4c[tid]] + d;
                    v = v - d;
                }
                if (tid == 0) L.u[cur] = L.u[cur] + min_val;
                if (tid < nc) L.path[tid] = path;
            }
            __syncthreads();
            if (sink >= 0 && tid == 0) {
                int32_t j = sink;
                for (int k = 0; k <= nr; ++k) {
                    const int32_t r = L.path[j];
                    L.r4c[j] = r;
                    const int32_t next = L.c4r[r];
                    L.c4r[r] = j;
                    j = next;
                    if (r == cur || j < 0) break;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < nr) {
        const int32_t c = L.c4r[tid];
        if (c >= 0 && !(L.M[tid * TRK_LD + c] >= thr)) L.c4r[tid] = -1;
    }
    __syncthreads();
}

__global__ __launch_bounds__(TRK_THREADS) void track_update_kernel(TrkStream* __restrict__ state, TrkParams p, const float* __restrict__ dets, int row_stride,
                                                                   const int32_t* __restrict__ fidx, int n_dets, const int32_t* __restrict__ d_n_dets,
                                                                   unsigned long long step_mask) {
    __shared__ TrkLds L;
    const int tid = threadIdx.x;
    if (d_n_dets) {   // the counted entry: the rows of this call are the first min(*d_n_dets, n_dets); the others are never read
        const int m = *d_n_dets;
        n_dets = m < 0 ? 0 : (m < n_dets ? m : n_dets);
    }
    int s = -1;   // the blockIdx.x-th stream of the mask
    for (int b = 0, k = -1; b < TRK_MAX_STREAMS; ++b)
        if ((step_mask >> b) & 1ull) {
            if (++k == (int)blockIdx.x) { s = b; break; }
        }
    if (s < 0 || s >= p.n_streams) return;
    TrkStream& S = state[s];
    const double thr = (double)p.iou_thr;

    // 1. this stream's detection rows in call order
    int total = 0, bad_row = 0;
    for (int base = 0; base < n_dets; base += TRK_THREADS) {
        const int i = base + tid;
        const bool in = i < n_dets;
        const int32_t f = in ? (fidx ? fidx[i] : 0) : s;
        bool take = in && f == s;
        float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (take) {
            bool fin = true;
#pragma unroll
            for (int q = 0; q < 5; ++q) { v[q] = dets[(size_t)i * row_stride + q]; fin = fin && trk_finite((double)v[q]); }
            if (!fin) { take = false; bad_row = 1; }
        }
        if (f < 0 || f >= p.n_streams) bad_row = 1;
        int all;
        const int off = total + wg_prefix(L, take, all);
        if (take && off < TRK_MAX) {
#pragma unroll
            for (int q = 0; q < 5; ++q) L.det[off][q] = (double)v[q];
        }
        total += all;
    }
    int flags = __syncthreads_or(bad_row) ? TRK_FLAG_BAD_ROW : 0;
    if (total > TRK_MAX) flags |= TRK_FLAG_DETS;
    const int nd = total < TRK_MAX ? total : TRK_MAX;

    // 2. predict, one lane per track; tracks whose predicted box is not finite leave the list
    int nt = S.n_tracks;
    const int frame = S.frame_count + 1, next_id = S.next_id;
    TrkTrack T;
    double box[4] = {0.0, 0.0, 0.0, 0.0};
    bool have = tid < nt, good = false;
    if (have) {
        T = S.trk[tid];
        trk_predict(T, box);
        good = trk_box_finite(box);
    }
    {
        int n_good;
        const int k = wg_prefix(L, good, n_good);
        if (n_good != nt) {   // rare: compact through the state (every lane holds its track in registers by now)
            if (good) S.trk[k] = T;
            if (good) {
#pragma unroll
                for (int q = 0; q < 4; ++q) L.tbox[k][q] = box[q];
            }
            __syncthreads();
            nt = n_good;
            have = tid < nt;
            if (have) T = S.trk[tid];
        } else if (have) {
#pragma unroll
            for (int q = 0; q < 4; ++q) L.tbox[tid][q] = box[q];
        }
    }
    if (tid < TRK_MAX) { L.tod[tid] = -1; L.dot[tid] = -1; }
    __syncthreads();

    // 3. + 4. the IoU matrix and the association
    if (nd > 0 && nt > 0) {
        const bool tr = nd > nt;
        const int nr = tr ? nt : nd, nc = tr ? nd : nt;
        for (int idx = tid; idx < nd * nt; idx += TRK_THREADS) {
            const int d = idx / nt, t = idx - d * nt;
            L.M[(tr ? t : d) * TRK_LD + (tr ? d : t)] = trk_iou(L.det[d], L.tbox[t]);
        }
        __syncthreads();
        associate_lanes(L, nr, nc, thr);
        if (tid < nr && L.c4r[tid] >= 0) {
            const int d = tr ? L.c4r[tid] : tid, t = tr ? tid : L.c4r[tid];
            L.tod[d] = t;
            L.dot[t] = d;
        }
        __syncthreads();
    }

    // 5. update the matched tracks, create the births (the unmatched detections in detection-index order)
    if (have && L.dot[tid] >= 0) trk_update(T, L.det[L.dot[tid]]);
    int nb;
    {
        const bool unmatched = tid < nd && L.tod[tid] < 0;
        const int b = wg_prefix(L, unmatched, nb);
        if (unmatched && nt + b < TRK_MAX) L.birth[nt + b] = tid;
    }
    if (nt + nb > TRK_MAX) { flags |= TRK_FLAG_BIRTHS; nb = TRK_MAX - nt; }
    __syncthreads();
    if (tid >= nt && tid < nt + nb) {
        trk_init(T, L.det[L.birth[tid]], next_id + (tid - nt));
        have = true;
    }

    // 6. the report rows, in reversed list order
    bool rep = false;
    if (have) {
        trk_x_to_box(T.x, box);
        rep = nd == 0 || trk_reported(T, frame, p.min_hits);
    }
    int n_rep;
    {
        const int q = wg_prefix(L, rep, n_rep);
        if (rep) {
            const int row = n_rep - 1 - q;
#pragma unroll
            for (int k = 0; k < 4; ++k) S.rep[row][k] = box[k];
            S.rep[row][4] = T.score;
            S.rep_id[row] = T.id + 1;
        }
    }

    // 7. the surviving tracks, compacted (every lane read its track long before the first barrier above)
    int n_keep;
    {
        const bool keep = have && T.tsu <= p.max_age;
        const int k = wg_prefix(L, keep, n_keep);
        if (keep) S.trk[k] = T;
    }
    if (tid == 0) {
        S.n_tracks = n_keep;
        S.frame_count = frame;
        S.next_id = next_id + nb;
        S.n_rows = n_rep;
        S.flags = flags;
    }
}

// The stepped streams' report rows packed into the caller's buffers: stream ascending, the state's order within a stream; rows up to n_out are "absent".
__global__ __launch_bounds__(GATHER_THREADS) void track_gather_kernel(const TrkStream* __restrict__ state, int n_streams, unsigned long long step_mask,
                                                                      float* __restrict__ rows, int32_t* __restrict__ ids, int32_t* __restrict__ stream, int n_out,
                                                                      int32_t* __restrict__ count, int32_t* __restrict__ flags_out) {
    __shared__ int32_t s_cnt[TRK_MAX_STREAMS], s_off[TRK_MAX_STREAMS + 1];
    const int tid = threadIdx.x;
    if (tid < n_streams) s_cnt[tid] = ((step_mask >> tid) & 1ull) ? state[tid].n_rows : 0;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int s = 0; s < n_streams; ++s) { s_off[s] = acc; acc += s_cnt[s]; }
        s_off[n_streams] = acc;
    }
    __syncthreads();
    const int total = s_off[n_streams];
    if (tid < n_streams) {
        count[tid] = s_cnt[tid];
        if (flags_out) {
            int f = ((step_mask >> tid) & 1ull) ? state[tid].flags : 0;
            if (s_cnt[tid] > 0 && s_off[tid] + s_cnt[tid] > n_out) f |= TRK_FLAG_ROWS;   // rows of THIS stream were cut
            flags_out[tid] = f;
        }
    }
    if (tid == 0) count[n_streams] = total;
    for (int i = tid; i < n_out; i += GATHER_THREADS) {
        if (i < total) {
            int s = 0;
            while (s + 1 < n_streams && s_off[s + 1] <= i) ++s;   // at most n_streams - 1 steps
            const int r = i - s_off[s];
            const TrkStream& S = state[s];
#pragma unroll
            for (int k = 0; k < 5; ++k) rows[(size_t)i * 6 + k] = (float)S.rep[r][k];
            rows[(size_t)i * 6 + 5] = (float)S.rep_id[r];
            ids[i] = S.rep_id[r];
            stream[i] = s;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) rows[(size_t)i * 6 + k] = NAN;
            rows[(size_t)i * 6 + 4] = 0.f;
            rows[(size_t)i * 6 + 5] = -1.f;
            ids[i] = -1;
            stream[i] = -1;
        }
    }
}

// vp_dbg_lsap on a device: the association of track_update_kernel alone on a matrix from the host
__global__ __launch_bounds__(TRK_THREADS) void track_lsap_kernel(const double* __restrict__ iou, int nd, int nt, float thr, int32_t* __restrict__ trk_of_det) {
    __shared__ TrkLds L;
    const int tid = threadIdx.x;
    const bool tr = nd > nt;
    const int nr = tr ? nt : nd, nc = tr ? nd : nt;
    for (int idx = tid; idx < nd * nt; idx += TRK_THREADS) {
        const int d = idx / nt, t = idx - d * nt;
        L.M[(tr ? t : d) * TRK_LD + (tr ? d : t)] = iou[idx];
    }
    if (tid < nd) L.tod[tid] = -1;
    __syncthreads();
    associate_lanes(L, nr, nc, (double)thr);
    if (tid < nr && L.c4r[tid] >= 0) L.tod[tr ? L.c4r[tid] : tid] = tr ? tid : L.c4r[tid];
    __syncthreads();
    if (tid < nd) trk_of_det[tid] = L.tod[tid];
}

}  // namespace vp

namespace {

// ---- the host model: sortgeom.h run serially, in the kernels' order (HOST ONLY)

// tracker.associate on M [nr, nc] with row pitch ld: c4r [nr]
void associate_host(const double* M, int ld, int nr, int nc, double thr, int32_t* c4r) {
    bool ambiguous = false;
    std::vector<int> cc((size_t)nc, 0);
    for (int r = 0; r < nr; ++r) {
        int rc = 0;
        c4r[r] = -1;
        for (int c = 0; c < nc; ++c)
            if (M[(size_t)r * ld + c] > thr) { ++rc; ++cc[c]; c4r[r] = c; }
        if (rc > 1) ambiguous = true;
    }
    for (int c = 0; c < nc; ++c)
        if (cc[c] > 1) ambiguous = true;
    if (ambiguous) {
        std::vector<double> u((size_t)nr, 0.0), v((size_t)nc, 0.0), spc((size_t)nc);
        std::vector<int32_t> r4c((size_t)nc, -1), path((size_t)nc);
        std::vector<char> sc((size_t)nc);
        for (int r = 0; r < nr; ++r) c4r[r] = -1;
        for (int cur = 0; cur < nr; ++cur) {
            std::fill(spc.begin(), spc.end(), (double)INFINITY);
            std::fill(path.begin(), path.end(), -1);
            std::fill(sc.begin(), sc.end(), 0);
            double min_val = 0.0;
            int32_t i = cur, sink = -1;
            for (int step = 0; step < nc; ++step) {
                double bk = INFINITY;
                int32_t bf = 1, bj = INT32_MAX;
                for (int j = 0; j < nc; ++j) {
                    if (sc[j]) continue;
                    const double r = vp::lsap_reduced(min_val, M[(size_t)i * ld + j], u[i], v[j]);
                    if (r < spc[j]) { spc[j] = r; path[j] = i; }
                    if (spc[j] < INFINITY && vp::lsap_before(spc[j], r4c[j] != -1, j, bk, bf, bj)) { bk = spc[j]; bf = r4c[j] != -1; bj = j; }
                }
                if (bj == INT32_MAX) break;
                min_val = bk;
                sc[bj] = 1;
                if (bf == 0) { sink = bj; break; }
                i = r4c[bj];
            }
            if (sink < 0) continue;
            for (int j = 0; j < nc; ++j)
                if (sc[j]) {
                    const double d = min_val - spc[j];
                    if (j != sink) u[r4c[j]] = u[r4c[j]] + d;
                    v[j] = v[j] - d;
                }
            u[cur] = u[cur] + min_val;
            int32_t j = sink;
            for (int k = 0; k <= nr; ++k) {
                const int32_t r = path[j];
                r4c[j] = r;
                const int32_t next = c4r[r];
                c4r[r] = j;
                j = next;
                if (r == cur || j < 0) break;
            }
        }
    }
    for (int r = 0; r < nr; ++r)
        if (c4r[r] >= 0 && !(M[(size_t)r * ld + c4r[r]] >= thr)) c4r[r] = -1;
}

// track_update_kernel for stream s
void step_host(vp::TrkStream& S, int s, const vp::TrkParams& p, const float* dets, int row_stride, const int32_t* fidx, int n_dets) {
    using namespace vp;
    const double thr = (double)p.iou_thr;
    std::vector<double> det, tbox((size_t)TRK_MAX * 4), M;
    int total = 0, flags = 0;
    for (int i = 0; i < n_dets; ++i) {
        const int32_t f = fidx ? fidx[i] : 0;
        if (f < 0 || f >= p.n_streams) { flags |= TRK_FLAG_BAD_ROW; continue; }
        if (f != s) continue;
        bool fin = true;
        for (int q = 0; q < 5; ++q) fin = fin && trk_finite((double)dets[(size_t)i * row_stride + q]);
        if (!fin) { flags |= TRK_FLAG_BAD_ROW; continue; }
        if (total < TRK_MAX)
            for (int q = 0; q < 5; ++q) det.push_back((double)dets[(size_t)i * row_stride + q]);
        ++total;
    }
    if (total > TRK_MAX) flags |= TRK_FLAG_DETS;
    const int nd = total < TRK_MAX ? total : TRK_MAX;

    int nt = S.n_tracks;
    const int frame = S.frame_count + 1, next_id = S.next_id;
    std::vector<TrkTrack> T((size_t)TRK_MAX);
    std::vector<char> good((size_t)TRK_MAX, 0);
    std::vector<double> boxes((size_t)TRK_MAX * 4);
    int n_good = 0;
    for (int t = 0; t < nt; ++t) {
        T[t] = S.trk[t];
        trk_predict(T[t], &boxes[(size_t)t * 4]);
        good[t] = trk_box_finite(&boxes[(size_t)t * 4]);
        n_good += good[t];
    }
    if (n_good != nt) {
        int k = 0;
        for (int t = 0; t < nt; ++t)
            if (good[t]) {
                S.trk[k] = T[t];
                for (int q = 0; q < 4; ++q) tbox[(size_t)k * 4 + q] = boxes[(size_t)t * 4 + q];
                ++k;
            }
        nt = n_good;
        for (int t = 0; t < nt; ++t) T[t] = S.trk[t];
    } else {
        tbox = boxes;
    }
    std::vector<int32_t> tod((size_t)TRK_MAX, -1), dot((size_t)TRK_MAX, -1), c4r((size_t)TRK_MAX, -1);
    if (nd > 0 && nt > 0) {
        const bool tr = nd > nt;
        const int nr = tr ? nt : nd, nc = tr ? nd : nt;
        M.assign((size_t)nr * nc, 0.0);
        for (int d = 0; d < nd; ++d)
            for (int t = 0; t < nt; ++t) M[(size_t)(tr ? t : d) * nc + (tr ? d : t)] = trk_iou(&det[(size_t)d * 5], &tbox[(size_t)t * 4]);
        associate_host(M.data(), nc, nr, nc, thr, c4r.data());
        for (int r = 0; r < nr; ++r)
            if (c4r[r] >= 0) {
                const int d = tr ? c4r[r] : r, t = tr ? r : c4r[r];
                tod[d] = t;
                dot[t] = d;
            }
    }
    for (int t = 0; t < nt; ++t)
        if (dot[t] >= 0) trk_update(T[t], &det[(size_t)dot[t] * 5]);
    int nb = 0;
    for (int d = 0; d < nd; ++d)
        if (tod[d] < 0) {
            if (nt + nb < TRK_MAX) trk_init(T[nt + nb], &det[(size_t)d * 5], next_id + nb);
            ++nb;
        }
    if (nt + nb > TRK_MAX) { flags |= TRK_FLAG_BIRTHS; nb = TRK_MAX - nt; }
    const int n_list = nt + nb;
    int n_rep = 0;
    for (int t = 0; t < n_list; ++t) n_rep += nd == 0 || trk_reported(T[t], frame, p.min_hits);
    for (int t = 0, q = 0; t < n_list; ++t)
        if (nd == 0 || trk_reported(T[t], frame, p.min_hits)) {
            const int row = n_rep - 1 - q++;
            trk_x_to_box(T[t].x, S.rep[row]);
            S.rep[row][4] = T[t].score;
            S.rep_id[row] = T[t].id + 1;
        }
    int n_keep = 0;
    for (int t = 0; t < n_list; ++t)
        if (T[t].tsu <= p.max_age) S.trk[n_keep++] = T[t];
    S.n_tracks = n_keep;
    S.frame_count = frame;
    S.next_id = next_id + nb;
    S.n_rows = n_rep;
    S.flags = flags;
}

// track_gather_kernel
void gather_host(const vp::TrkStream* state, int n_streams, uint64_t step_mask, float* rows, int32_t* ids, int32_t* stream, int n_out, int32_t* count, int32_t* flags_out) {
    int total = 0;
    for (int s = 0; s < n_streams; ++s) {
        const bool stepped = (step_mask >> s) & 1ull;
        const int cnt = stepped ? state[s].n_rows : 0;
        for (int r = 0; r < cnt; ++r) {
            const int i = total + r;
            if (i >= n_out) break;
            for (int k = 0; k < 5; ++k) rows[(size_t)i * 6 + k] = (float)state[s].rep[r][k];
            rows[(size_t)i * 6 + 5] = (float)state[s].rep_id[r];
            ids[i] = state[s].rep_id[r];
            stream[i] = s;
        }
        count[s] = cnt;
        if (flags_out) flags_out[s] = (stepped ? state[s].flags : 0) | (cnt > 0 && total + cnt > n_out ? vp::TRK_FLAG_ROWS : 0);
        total += cnt;
    }
    count[n_streams] = total;
    for (int i = total; i < n_out; ++i) {
        for (int k = 0; k < 4; ++k) rows[(size_t)i * 6 + k] = NAN;
        rows[(size_t)i * 6 + 4] = 0.f;
        rows[(size_t)i * 6 + 5] = -1.f;
        ids[i] = -1;
        stream[i] = -1;
    }
}

// every refusal (HOST ONLY), before anything is enqueued
int cfg_check(const vp_track_cfg* cfg, vp::TrkParams& p, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "tracker: " + m; return (int)VP_ERR_INVALID; };
    if (!cfg) return bad("null cfg");
    if (cfg->n_streams < 1 || cfg->n_streams > VP_TRACK_MAX_STREAMS) return bad("n_streams = " + std::to_string(cfg->n_streams) + " outside 1.." + std::to_string(VP_TRACK_MAX_STREAMS));
    if (cfg->max_age < 0) return bad("max_age < 0");
    if (cfg->min_hits < 0) return bad("min_hits < 0");
    if (!(cfg->iou_threshold > 0.f && cfg->iou_threshold < 1.f)) return bad("iou_threshold outside (0, 1)");
    p.max_age = cfg->max_age; p.min_hits = cfg->min_hits; p.iou_thr = cfg->iou_threshold; p.n_streams = cfg->n_streams;
    return VP_OK;
}

int update_args(const vp::TrkParams& p, const void* dets, int row_stride, int n_dets, uint64_t step_mask, const void* rows, const void* ids, const void* stream, int n_out,
                const void* count, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "tracker: " + m; return (int)VP_ERR_INVALID; };
    if (n_dets < 0) return bad("negative n_dets");
    if (n_out < 0) return bad("negative n_out");
    if (row_stride < 5) return bad("row_stride = " + std::to_string(row_stride) + " < 5");
    if (n_dets > 0 && !dets) return bad("null detections with n_dets > 0");
    if (!count) return bad("null count");
    if (n_out > 0 && !(rows && ids && stream)) return bad("null rows, ids or stream with n_out > 0");
    return mask_check(step_mask, p.n_streams, "tracker: ", why);
}

// the checked call on stream s: two launches
int update_enqueue(vp_tracker* t, const float* d_dets, int row_stride, const int32_t* d_fidx, int n_dets, const int32_t* d_n_dets, uint64_t step_mask, float* d_rows,
                   int32_t* d_ids, int32_t* d_stream, int n_out, int32_t* d_count, int32_t* d_flags, hipStream_t s) {
    vp_ctx* c = t->c;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int blocks = popcount64(step_mask);
    if (blocks > 0) {
        hipLaunchKernelGGL(vp::track_update_kernel, dim3(blocks), dim3(vp::TRK_THREADS), 0, s, t->state, t->p, d_dets, row_stride, d_fidx, n_dets,
                           d_n_dets, (unsigned long long)step_mask);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(vp::track_gather_kernel, dim3(1), dim3(vp::GATHER_THREADS), 0, s, t->state, t->p.n_streams, (unsigned long long)step_mask, d_rows, d_ids, d_stream,
                       n_out, d_count, d_flags);
    HIPCHK(c, hipGetLastError());
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_tracker_create(vp_handle c, const vp_track_cfg* cfg, vp_tracker_handle* out) {
    return stage_create(c, out, [&](vp_tracker* t, std::string* why) { return cfg_check(cfg, t->p, why); },
                        [](vp_tracker* t) {
                            t->state = t->alloc<vp::TrkStream>(sizeof(vp::TrkStream) * (size_t)t->p.n_streams, 0);
                            return "tracker state: ";
                        });
}

int vp_tracker_destroy(vp_tracker_handle t) { return stage_destroy(t); }

int vp_tracker_reset_stream(vp_tracker_handle t, uint64_t stream_mask, void* caller_stream) {
    if (!t) return VP_ERR_INVALID;
    return stage_reset_masked(t, t->state, sizeof(vp::TrkStream), t->p.n_streams, stream_mask, "tracker: ", caller_stream);
}

int vp_tracker_update_stream(vp_tracker_handle t, const float* d_dets, int32_t row_stride, const int32_t* d_frame_idx, int32_t n_dets, uint64_t step_mask, float* d_rows,
                             int32_t* d_ids, int32_t* d_stream, int32_t n_out, int32_t* d_count, int32_t* d_flags, void* caller_stream) {
    if (!t) return VP_ERR_INVALID;
    std::string why;
    if (update_args(t->p, d_dets, row_stride, n_dets, step_mask, d_rows, d_ids, d_stream, n_out, d_count, &why)) return fail(t->c, VP_ERR_INVALID, why);
    return update_enqueue(t, d_dets, row_stride, d_frame_idx, n_dets, nullptr, step_mask, d_rows, d_ids, d_stream, n_out, d_count, d_flags, (hipStream_t)caller_stream);
}

int vp_tracker_update_counted_stream(vp_tracker_handle t, const float* d_dets, int32_t row_stride, const int32_t* d_frame_idx, int32_t n_dets_cap, const int32_t* d_n_dets,
                                     uint64_t step_mask, float* d_rows, int32_t* d_ids, int32_t* d_stream, int32_t n_out, int32_t* d_count, int32_t* d_flags,
                                     void* caller_stream) {
    if (!t) return VP_ERR_INVALID;
    std::string why;
    if (!d_n_dets) return fail(t->c, VP_ERR_INVALID, "tracker: null d_n_dets");
    if (update_args(t->p, d_dets, row_stride, n_dets_cap, step_mask, d_rows, d_ids, d_stream, n_out, d_count, &why)) return fail(t->c, VP_ERR_INVALID, why);
    return update_enqueue(t, d_dets, row_stride, d_frame_idx, n_dets_cap, d_n_dets, step_mask, d_rows, d_ids, d_stream, n_out, d_count, d_flags, (hipStream_t)caller_stream);
}

int vp_tracker_update(vp_tracker_handle t, const float* dets, int32_t row_stride, const int32_t* frame_idx, int32_t n_dets, uint64_t step_mask, float* rows, int32_t* ids,
                      int32_t* stream, int32_t n_out, int32_t* count, int32_t* flags) {
    if (!t) return VP_ERR_INVALID;
    vp_ctx* c = t->c;
    std::string why;
    if (update_args(t->p, dets, row_stride, n_dets, step_mask, rows, ids, stream, n_out, count, &why)) return fail(c, VP_ERR_INVALID, why);
    // one scratch block: dets | frame index | rows | ids | stream | count | flags
    HostStage st(c);
    const int ns = t->p.n_streams;
    const size_t det_bytes = n_dets ? ((size_t)(n_dets - 1) * row_stride + 5) * 4 : 0, ob = (size_t)n_out * 4, sb = (size_t)(ns + 1) * 4;
    const size_t o_det = st.part(det_bytes), o_fi = st.part((size_t)n_dets * 4), o_rows = st.part((size_t)n_out * 24), o_ids = st.part(ob), o_st = st.part(ob), o_ct = st.part(sb),
                 o_fl = st.part(sb);
    if (st.alloc()) return st.rc;
    float *d_det = st.at<float>(o_det), *d_rows = st.at<float>(o_rows);
    int32_t *d_fi = st.at<int32_t>(o_fi), *d_ids = st.at<int32_t>(o_ids), *d_st = st.at<int32_t>(o_st), *d_ct = st.at<int32_t>(o_ct), *d_fl = st.at<int32_t>(o_fl);
    if (n_dets) st.up(d_det, dets, det_bytes, "upload detections");
    if (n_dets && frame_idx) st.up(d_fi, frame_idx, (size_t)n_dets * 4, "upload frame index");
    if (!st.rc)
        st.rc = update_enqueue(t, n_dets ? d_det : nullptr, row_stride, n_dets && frame_idx ? d_fi : nullptr, n_dets, nullptr, step_mask, d_rows, d_ids, d_st, n_out, d_ct, d_fl, st.s);
    if (!st.rc) {
        if (n_out) {
            st.down(rows, d_rows, (size_t)n_out * 24, "download rows");
            st.down(ids, d_ids, ob, "download ids");
            st.down(stream, d_st, ob, "download stream");
        }
        st.down(count, d_ct, sb, "download count");
        if (flags) st.down(flags, d_fl, (size_t)ns * 4, "download flags");
    }
    st.sync();
    return st.rc;
}

int vp_tracker_state_bytes(int32_t n_streams, int64_t* bytes) {
    if (!bytes || n_streams < 1 || n_streams > VP_TRACK_MAX_STREAMS) return fail(nullptr, VP_ERR_INVALID, "tracker: n_streams outside 1.." + std::to_string(VP_TRACK_MAX_STREAMS) + " or null bytes");
    *bytes = (int64_t)(sizeof(vp::TrkStream) * (size_t)n_streams);
    return VP_OK;
}

int vp_tracker_download_state(vp_tracker_handle t, void* out) {
    if (!t || !out) return VP_ERR_INVALID;
    return stage_download(t, out, t->state, sizeof(vp::TrkStream) * (size_t)t->p.n_streams);
}

int vp_dbg_track_host(void* state, const vp_track_cfg* cfg, const float* dets, int32_t row_stride, const int32_t* frame_idx, int32_t n_dets, uint64_t step_mask,
                      float* rows, int32_t* ids, int32_t* stream, int32_t n_out, int32_t* count, int32_t* flags) {
    vp::TrkParams p;
    std::string why;
    if (cfg_check(cfg, p, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    if (!state) return fail(nullptr, VP_ERR_INVALID, "tracker: null state");
    if (update_args(p, dets, row_stride, n_dets, step_mask, rows, ids, stream, n_out, count, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    vp::TrkStream* S = (vp::TrkStream*)state;
    for (int s = 0; s < p.n_streams; ++s)
        if ((step_mask >> s) & 1ull) step_host(S[s], s, p, dets, row_stride, frame_idx, n_dets);
    gather_host(S, p.n_streams, step_mask, rows, ids, stream, n_out, count, flags);
    return VP_OK;
}

int vp_dbg_lsap(int32_t device_id, const double* iou, int32_t nd, int32_t nt, float thr, int32_t* trk_of_det) {
    auto bad = [&](const std::string& m) { return fail(nullptr, VP_ERR_INVALID, "tracker: vp_dbg_lsap: " + m); };
    if (nd < 0 || nt < 0 || nd > VP_TRACK_MAX || nt > VP_TRACK_MAX) return bad("nd or nt outside 0.." + std::to_string(VP_TRACK_MAX));
    if (!(thr > 0.f && thr < 1.f)) return bad("thr outside (0, 1)");
    if (nd > 0 && !trk_of_det) return bad("null trk_of_det");
    if (nd > 0 && nt > 0 && !iou) return bad("null iou");
    for (int d = 0; d < nd; ++d) trk_of_det[d] = -1;
    if (nd == 0 || nt == 0) return VP_OK;
    if (device_id < 0) {
        const bool tr = nd > nt;
        const int nr = tr ? nt : nd, nc = tr ? nd : nt;
        std::vector<double> M((size_t)nr * nc);
        for (int d = 0; d < nd; ++d)
            for (int t = 0; t < nt; ++t) M[(size_t)(tr ? t : d) * nc + (tr ? d : t)] = iou[(size_t)d * nt + t];
        std::vector<int32_t> c4r((size_t)nr, -1);
        associate_host(M.data(), nc, nr, nc, (double)thr, c4r.data());
        for (int r = 0; r < nr; ++r)
            if (c4r[r] >= 0) trk_of_det[tr ? c4r[r] : r] = tr ? r : c4r[r];
        return VP_OK;
    }
    vp_ctx* c = nullptr;   // errors are reported through the create-error slot
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(c, VP_ERR_HIP, "no HIP device available (no CPU fallback)");
    if (device_id >= ndev) return fail(c, VP_ERR_INVALID, "device_id out of range");
    HIPCHK(c, hipSetDevice(device_id));
    HostStage st(c);   // iou | pairs; blocking copies around a launch on the default stream
    const size_t o_iou = st.part((size_t)nd * nt * 8), o_out = st.part((size_t)nd * 4);
    if (st.alloc()) return st.rc;
    double* d_iou = st.at<double>(o_iou);
    int32_t* d_out = st.at<int32_t>(o_out);
    st.chk(hipMemcpy(d_iou, iou, (size_t)nd * nt * 8, hipMemcpyHostToDevice), "upload iou");
    if (!st.rc) {
        hipLaunchKernelGGL(vp::track_lsap_kernel, dim3(1), dim3(vp::TRK_THREADS), 0, 0, d_iou, nd, nt, thr, d_out);
        st.chk(hipGetLastError(), "track_lsap_kernel");
        st.chk(hipMemcpy(trk_of_det, d_out, (size_t)nd * 4, hipMemcpyDeviceToHost), "download pairs");
    }
    return st.rc;
}

}  // extern "C"
