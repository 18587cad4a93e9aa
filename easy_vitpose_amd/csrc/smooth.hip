// vp_smoother_* / vp_smooth_*: One-Euro keypoint smoothing keyed by (stream, track id) as a stream-ordered device stage behind the boxes entry and its NMS
// (semantics: eurogeom.h), its synchronous host twin vp_smooth_update and the tap vp_dbg_smooth_host.  Two launches per call: smooth_assign_kernel, one workgroup
// per stepped stream (ageing, id matching, births), and smooth_filter_kernel, one thread per (row, joint).  No atomics, no flags between workgroups: every row maps
// to at most one slot and every slot to at most one row of a call, so a call is bit-identical from run to run.
#include "api_internal.h"
#include "hoststage.h"
#include "stageobj.h"
#include "eurogeom.h"

using namespace vpi;

struct vp_smoother : StageObj {
    vp::EuroParams p{};
    char* state = nullptr;           // device: n_streams blobs (eurogeom.h) | slot_of_row int32 [max_rows] | gap_of_row int32 [max_rows]
    int32_t* slot_of_row = nullptr;
    int32_t* gap_of_row = nullptr;
    size_t state_bytes = 0;
};

namespace vp {

constexpr int EURO_THREADS = EURO_SLOTS, EURO_WAVES = EURO_THREADS / 64, FILTER_THREADS = 256;
// the codes of a chunk row while it is being placed (never stored)
constexpr int32_t EURO_UNKNOWN = INT32_MIN, EURO_DUP = INT32_MIN + 1, EURO_DROP = INT32_MIN + 2;

struct EuroLds {
    int32_t sid[EURO_SLOTS], sseen[EURO_SLOTS];                    // the table
    int32_t rrow[EURO_THREADS], rid[EURO_THREADS], fin[EURO_THREADS];   // the candidate rows of a chunk: caller row, id, every coordinate finite
    int32_t code[EURO_THREADS], gap[EURO_THREADS], born[EURO_THREADS];
    int32_t freeslot[EURO_SLOTS];
    int32_t wcnt[EURO_WAVES];
};

// exclusive prefix of `flag` over the workgroup in thread order, and the total (two barriers; every thread calls it): the tracker's ballot prefix
__device__ inline int euro_prefix(EuroLds& L, bool flag, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) L.wcnt[wave] = __popcll(b);
    __syncthreads();
    int off = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
    for (int w = 0; w < EURO_WAVES; ++w) {
        if (w < wave) off += L.wcnt[w];
        all += L.wcnt[w];
    }
    __syncthreads();
    total = all;
    return off;
}

// One workgroup per stepped stream; thread t is slot t of the table and row t of a chunk of at most EURO_THREADS candidate rows.  The rows are placed chunk by
// chunk in call order, which equals placing them one by one (eurogeom.h / the host model below): within a chunk the matches against the table come first -- a slot
// takes the first row of its id and calls every later one a duplicate -- then the rows of unknown ids: the first row of each id takes the next free slot in row
// order, a repeat is a duplicate if that first row was born and dropped with it otherwise.
__global__ __launch_bounds__(EURO_THREADS) void smooth_assign_kernel(char* __restrict__ state, EuroParams p, const float* __restrict__ kpts, const int32_t* __restrict__ ids,
                                                                     const int32_t* __restrict__ stream, const int32_t* __restrict__ rank, int n,
                                                                     unsigned long long step_mask, int32_t* __restrict__ slot_of_row, int32_t* __restrict__ gap_of_row,
                                                                     int32_t* __restrict__ flags_out) {
    __shared__ EuroLds L;
    const int tid = threadIdx.x;
    int s = -1;   // the blockIdx.x-th stream of the mask
    for (int b = 0, k = -1; b < EURO_MAX_STREAMS; ++b)
        if ((step_mask >> b) & 1ull) {
            if (++k == (int)blockIdx.x) { s = b; break; }
        }
    if (s < 0 || s >= p.n_streams) return;
    const int K = p.n_joints, row_floats = 3 * K;
    char* B = state + (size_t)s * euro_stream_bytes(K);
    int32_t* hdr = (int32_t*)B;
    int32_t* g_id = (int32_t*)(B + euro_off_id());
    int32_t* g_seen = (int32_t*)(B + euro_off_seen());
    const int fc = hdr[0] + 1;
    {
        int32_t id = g_id[tid], seen = g_seen[tid];
        if (seen > 0 && fc - seen - 1 > p.max_age) { id = 0; seen = 0; }   // ageing
        L.sid[tid] = id;
        L.sseen[tid] = seen;
    }
    int flags = 0;
    __syncthreads();

    for (int base = 0; base < n; base += EURO_THREADS) {
        const int i = base + tid;
        const bool in = i < n;
        const int32_t f = in ? (stream ? stream[i] : 0) : s;
        const int32_t id = in ? ids[i] : -1;
        if (id >= 0 && (f < 0 || f >= p.n_streams)) flags |= EURO_FLAG_BAD_ROW;
        const bool mine = in && f == s;
        const bool cand = mine && id >= 0 && (!rank || rank[i] >= 0);
        if (mine && !cand) slot_of_row[i] = EURO_PASS;
        int m;
        const int off = euro_prefix(L, cand, m);
        if (cand) { L.rrow[off] = i; L.rid[off] = id; L.fin[off] = 1; }
        __syncthreads();
        // every y and x of a candidate row finite: the chunk's rows flattened over the workgroup, consecutive lanes on consecutive floats of a row, no load
        // depending on another
        const int chunk_floats = m * row_floats;
#pragma unroll 8
        for (int e = tid; e < chunk_floats; e += EURO_THREADS) {
            const int c = e / row_floats, q = e - c * row_floats;
            const float v = kpts[(size_t)L.rrow[c] * row_floats + q];
            if (q % 3 != 2 && !euro_finite(v)) L.fin[c] = 0;   // every writer stores the same value
        }
        __syncthreads();
        if (tid < m) {
            L.code[tid] = L.fin[tid] ? EURO_UNKNOWN : EURO_PASS;
            L.gap[tid] = 0;
            if (!L.fin[tid]) flags |= EURO_FLAG_BAD_ROW;
        }
        __syncthreads();
        // the ids the table knows: the slot scans the chunk (each row matches at most one slot: the ids of the occupied slots are distinct)
        if (L.sseen[tid] > 0) {
            const int32_t my = L.sid[tid];
            int32_t seen = L.sseen[tid];
            for (int c = 0; c < m; ++c)
                if (L.fin[c] && L.rid[c] == my) {
                    if (seen != fc) { L.code[c] = tid; L.gap[c] = fc - seen; seen = fc; }
                    else L.code[c] = EURO_DUP;
                }
            L.sseen[tid] = seen;
        }
        __syncthreads();
        // the unknown ids: the first row of each takes a free slot in row order
        const bool unknown = tid < m && L.code[tid] == EURO_UNKNOWN;
        int first = tid;
        if (unknown)
            for (int c = 0; c < tid; ++c)
                if (L.code[c] == EURO_UNKNOWN && L.rid[c] == L.rid[tid]) { first = c; break; }
        const bool is_first = unknown && first == tid, is_free = L.sseen[tid] == 0;
        int n_first, n_free;
        const int b = euro_prefix(L, is_first, n_first);
        const int fr = euro_prefix(L, is_free, n_free);
        if (is_free) L.freeslot[fr] = tid;
        L.born[tid] = is_first && b < n_free;
        __syncthreads();
        int32_t code = tid < m ? L.code[tid] : EURO_PASS;
        if (unknown) {
            if (is_first) code = b < n_free ? euro_birth_code(L.freeslot[b]) : EURO_DROP;
            else code = L.born[first] ? EURO_DUP : EURO_DROP;
        }
        __syncthreads();   // every read of code[] and sseen[] above is done
        if (unknown && is_first && b < n_free) {
            const int slot = L.freeslot[b];
            L.sid[slot] = L.rid[tid];
            L.sseen[slot] = fc;
        }
        if (tid < m) {
            if (code == EURO_DUP) { flags |= EURO_FLAG_DUP; code = EURO_PASS; }
            if (code == EURO_DROP) { flags |= EURO_FLAG_FULL; code = EURO_PASS; }
            slot_of_row[L.rrow[tid]] = code;
            gap_of_row[L.rrow[tid]] = L.gap[tid];
        }
        __syncthreads();
    }
    g_id[tid] = L.sid[tid];
    g_seen[tid] = L.sseen[tid];
    int all = 0;
    if (__syncthreads_or(flags & EURO_FLAG_DUP)) all |= EURO_FLAG_DUP;
    if (__syncthreads_or(flags & EURO_FLAG_FULL)) all |= EURO_FLAG_FULL;
    if (__syncthreads_or(flags & EURO_FLAG_BAD_ROW)) all |= EURO_FLAG_BAD_ROW;
    if (tid == 0) {
        hdr[0] = fc;
        if (flags_out) flags_out[s] = all;
    }
}

// One thread per (row, joint): consecutive lanes walk consecutive joints, so the 12 bytes of a keypoint and the 16 + 16 + 2 bytes of its state are contiguous
// across the lanes.  Every thread reads its keypoint before it writes it: d_out == d_kpts is legal.  The rows of a stream outside the mask never look at
// slot_of_row (it holds an earlier call's codes there).
__global__ __launch_bounds__(FILTER_THREADS) void smooth_filter_kernel(char* __restrict__ state, EuroParams p, EuroTe te, const float* kpts, const int32_t* __restrict__ stream,
                                                                       const int32_t* __restrict__ slot_of_row, const int32_t* __restrict__ gap_of_row, int n,
                                                                       unsigned long long step_mask, float* out, int32_t* __restrict__ flags_out) {
    const int K = p.n_joints;
    if (flags_out && blockIdx.x == 0 && (int)threadIdx.x < p.n_streams && !((step_mask >> threadIdx.x) & 1ull)) flags_out[threadIdx.x] = 0;
    const size_t gid = (size_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
    if (gid >= (size_t)n * K) return;
    const int row = (int)(gid / K), j = (int)(gid - (size_t)row * K);
    const int32_t f = stream ? stream[row] : 0;
    const bool stepped = f >= 0 && f < p.n_streams && ((step_mask >> f) & 1ull);
    const int32_t code = stepped ? slot_of_row[row] : EURO_PASS;
    float y = kpts[gid * 3], x = kpts[gid * 3 + 1];
    const float conf = kpts[gid * 3 + 2];
    const int slot = code >= 0 ? code : euro_birth_slot(code);
    if (code != EURO_PASS && slot >= 0 && slot < EURO_SLOTS) {
        char* B = state + (size_t)f * euro_stream_bytes(K);
        const size_t e = ((size_t)slot * K + j) * 2;
        double* xp = (double*)(B + euro_off_x(K)) + e;
        double* dxp = (double*)(B + euro_off_dx(K)) + e;
        uint8_t* fp = (uint8_t*)(B + euro_off_fresh(K)) + e;
        double x0, x1, d0, d1;
        uint8_t f0, f1;
        if (code < 0) {
            euro_birth(y, x0, d0, f0);
            euro_birth(x, x1, d1, f1);
        } else {
            x0 = xp[0]; x1 = xp[1]; d0 = dxp[0]; d1 = dxp[1]; f0 = fp[0]; f1 = fp[1];
            const double t_e = te.v[f] * (double)gap_of_row[row];
            y = euro_update(y, t_e, p, x0, d0, f0);
            x = euro_update(x, t_e, p, x1, d1, f1);
        }
        xp[0] = x0; xp[1] = x1; dxp[0] = d0; dxp[1] = d1; fp[0] = f0; fp[1] = f1;
    }
    out[gid * 3] = y;
    out[gid * 3 + 1] = x;
    out[gid * 3 + 2] = conf;
}

}  // namespace vp

namespace {

// ---- the host model: eurogeom.h run serially, row by row in call order (HOST ONLY)
void smooth_host(char* state, const vp::EuroParams& p, const vp::EuroTe& te, const float* kpts, const int32_t* ids, const int32_t* stream, const int32_t* rank, int n,
                 uint64_t step_mask, float* out, int32_t* flags_out) {
    using namespace vp;
    const int K = p.n_joints;
    if (out != kpts && n > 0) memcpy(out, kpts, (size_t)n * K * 3 * sizeof(float));
    bool outside = false;
    for (int i = 0; i < n; ++i) {
        const int32_t f = stream ? stream[i] : 0;
        if (ids[i] >= 0 && (f < 0 || f >= p.n_streams)) outside = true;
    }
    for (int s = 0; s < p.n_streams; ++s) {
        if (!((step_mask >> s) & 1ull)) {
            if (flags_out) flags_out[s] = 0;
            continue;
        }
        char* B = state + (size_t)s * euro_stream_bytes(K);
        int32_t* hdr = (int32_t*)B;
        int32_t* sid = (int32_t*)(B + euro_off_id());
        int32_t* seen = (int32_t*)(B + euro_off_seen());
        double* xp = (double*)(B + euro_off_x(K));
        double* dxp = (double*)(B + euro_off_dx(K));
        uint8_t* fp = (uint8_t*)(B + euro_off_fresh(K));
        const int fc = ++hdr[0];
        int flags = outside ? EURO_FLAG_BAD_ROW : 0;
        for (int t = 0; t < EURO_SLOTS; ++t)
            if (seen[t] > 0 && fc - seen[t] - 1 > p.max_age) { sid[t] = 0; seen[t] = 0; }
        for (int i = 0; i < n; ++i) {
            if ((stream ? stream[i] : 0) != s || ids[i] < 0 || (rank && rank[i] < 0)) continue;
            const float* r = kpts + (size_t)i * K * 3;
            float* o = out + (size_t)i * K * 3;
            bool fin = true;
            for (int j = 0; j < K; ++j) fin = fin && euro_finite(r[3 * j]) && euro_finite(r[3 * j + 1]);
            if (!fin) { flags |= EURO_FLAG_BAD_ROW; continue; }
            int slot = -1, free_slot = -1;
            for (int t = 0; t < EURO_SLOTS; ++t) {
                if (seen[t] > 0 && sid[t] == ids[i]) slot = t;
                if (seen[t] == 0 && free_slot < 0) free_slot = t;
            }
            if (slot >= 0) {
                if (seen[slot] == fc) { flags |= EURO_FLAG_DUP; continue; }
                const double t_e = te.v[s] * (double)(fc - seen[slot]);
                seen[slot] = fc;
                for (int q = 0; q < 2 * K; ++q) {
                    const size_t e = (size_t)slot * K * 2 + q;
                    const int at = 3 * (q / 2) + (q & 1);
                    o[at] = euro_update(r[at], t_e, p, xp[e], dxp[e], fp[e]);
                }
            } else if (free_slot >= 0) {
                sid[free_slot] = ids[i];
                seen[free_slot] = fc;
                for (int q = 0; q < 2 * K; ++q) {
                    const size_t e = (size_t)free_slot * K * 2 + q;
                    euro_birth(r[3 * (q / 2) + (q & 1)], xp[e], dxp[e], fp[e]);
                }
            } else {
                flags |= EURO_FLAG_FULL;
            }
        }
        if (flags_out) flags_out[s] = flags;
    }
}

// every refusal (HOST ONLY), before anything is enqueued
int cfg_check(const vp_smooth_cfg* cfg, vp::EuroParams& p, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "smoother: " + m; return (int)VP_ERR_INVALID; };
    auto finite = [](double v) { return v - v == 0.0; };
    if (!cfg) return bad("null cfg");
    if (cfg->n_streams < 1 || cfg->n_streams > VP_TRACK_MAX_STREAMS) return bad("n_streams = " + std::to_string(cfg->n_streams) + " outside 1.." + std::to_string(VP_TRACK_MAX_STREAMS));
    if (cfg->n_joints < 1 || cfg->n_joints > vp::EURO_MAX_JOINTS) return bad("n_joints = " + std::to_string(cfg->n_joints) + " outside 1.." + std::to_string(vp::EURO_MAX_JOINTS));
    if (cfg->max_rows < 1 || cfg->max_rows > VP_SMOOTH_MAX_ROWS) return bad("max_rows = " + std::to_string(cfg->max_rows) + " outside 1.." + std::to_string(VP_SMOOTH_MAX_ROWS));
    if (cfg->max_age < 0) return bad("max_age < 0");
    if (!(finite(cfg->min_cutoff) && cfg->min_cutoff > 0.0)) return bad("min_cutoff not finite or <= 0");
    if (!(finite(cfg->d_cutoff) && cfg->d_cutoff > 0.0)) return bad("d_cutoff not finite or <= 0");
    if (!(finite(cfg->beta) && cfg->beta >= 0.0)) return bad("beta not finite or < 0");
    if (cfg->missing != 0 && cfg->missing != 1) return bad("missing = " + std::to_string(cfg->missing) + " is neither 0 (reference) nor 1 (restart)");
    p.min_cutoff = cfg->min_cutoff; p.beta = cfg->beta; p.d_cutoff = cfg->d_cutoff;
    p.max_age = cfg->max_age; p.n_streams = cfg->n_streams; p.n_joints = cfg->n_joints; p.max_rows = cfg->max_rows; p.missing = cfg->missing;
    return VP_OK;
}

int update_args(const vp::EuroParams& p, const void* kpts, const void* ids, int n, uint64_t step_mask, const double* t_e, const void* out, vp::EuroTe& te, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "smoother: " + m; return (int)VP_ERR_INVALID; };
    if (n < 0) return bad("negative n");
    if (n > p.max_rows) return bad("n = " + std::to_string(n) + " > max_rows = " + std::to_string(p.max_rows));
    if (n > 0 && !(kpts && ids && out)) return bad("null keypoints, ids or out with n > 0");
    for (int s = 0; s < vp::EURO_MAX_STREAMS; ++s) te.v[s] = 1.0;
    if (t_e)
        for (int s = 0; s < p.n_streams; ++s) {
            if (!(t_e[s] - t_e[s] == 0.0 && t_e[s] > 0.0)) return bad("t_e[" + std::to_string(s) + "] not finite or <= 0");
            te.v[s] = t_e[s];
        }
    return mask_check(step_mask, p.n_streams, "smoother: ", why);
}

// the checked call on stream q: two launches
int update_enqueue(vp_smoother* s, const vp::EuroTe& te, const float* d_kpts, const int32_t* d_ids, const int32_t* d_stream, const int32_t* d_rank, int n, uint64_t step_mask,
                   float* d_out, int32_t* d_flags, hipStream_t q) {
    vp_ctx* c = s->c;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int blocks = popcount64(step_mask);
    if (blocks > 0) {
        hipLaunchKernelGGL(vp::smooth_assign_kernel, dim3(blocks), dim3(vp::EURO_THREADS), 0, q, s->state, s->p, d_kpts, d_ids, d_stream, d_rank, n,
                           (unsigned long long)step_mask, s->slot_of_row, s->gap_of_row, d_flags);
        HIPCHK(c, hipGetLastError());
    }
    const size_t work = (size_t)n * s->p.n_joints;
    const unsigned grid = (unsigned)((work + vp::FILTER_THREADS - 1) / vp::FILTER_THREADS);
    hipLaunchKernelGGL(vp::smooth_filter_kernel, dim3(grid ? grid : 1), dim3(vp::FILTER_THREADS), 0, q, s->state, s->p, te, d_kpts, d_stream, s->slot_of_row, s->gap_of_row, n,
                       (unsigned long long)step_mask, d_out, d_flags);
    HIPCHK(c, hipGetLastError());
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_smoother_create(vp_handle c, const vp_smooth_cfg* cfg, vp_smoother_handle* out) {
    return stage_create(c, out, [&](vp_smoother* s, std::string* why) { return cfg_check(cfg, s->p, why); },
                        [](vp_smoother* s) {
                            s->state_bytes = vp::euro_stream_bytes(s->p.n_joints) * (size_t)s->p.n_streams;   // a multiple of 16
                            s->state = s->alloc(s->state_bytes + 2 * (size_t)s->p.max_rows * sizeof(int32_t), 0);
                            s->slot_of_row = (int32_t*)(s->state + s->state_bytes);
                            s->gap_of_row = s->slot_of_row + s->p.max_rows;
                            return "smoother state: ";
                        });
}

int vp_smoother_destroy(vp_smoother_handle s) { return stage_destroy(s); }

int vp_smoother_reset_stream(vp_smoother_handle s, uint64_t stream_mask, void* caller_stream) {
    if (!s) return VP_ERR_INVALID;
    return stage_reset_masked(s, s->state, vp::euro_stream_bytes(s->p.n_joints), s->p.n_streams, stream_mask, "smoother: ", caller_stream);
}

int vp_smooth_update_stream(vp_smoother_handle s, const float* d_kpts, const int32_t* d_ids, const int32_t* d_stream, const int32_t* d_rank, int32_t n, uint64_t step_mask,
                            const double* t_e, float* d_out, int32_t* d_flags, void* caller_stream) {
    if (!s) return VP_ERR_INVALID;
    std::string why;
    vp::EuroTe te;
    if (update_args(s->p, d_kpts, d_ids, n, step_mask, t_e, d_out, te, &why)) return fail(s->c, VP_ERR_INVALID, why);
    return update_enqueue(s, te, d_kpts, d_ids, d_stream, d_rank, n, step_mask, d_out, d_flags, (hipStream_t)caller_stream);
}

int vp_smooth_update(vp_smoother_handle s, const float* kpts, const int32_t* ids, const int32_t* stream, const int32_t* rank, int32_t n, uint64_t step_mask,
                     const double* t_e, float* out, int32_t* flags) {
    if (!s) return VP_ERR_INVALID;
    vp_ctx* c = s->c;
    std::string why;
    vp::EuroTe te;
    if (update_args(s->p, kpts, ids, n, step_mask, t_e, out, te, &why)) return fail(c, VP_ERR_INVALID, why);
    // one scratch block: keypoints | ids | stream | rank | flags; the filter runs in place on the keypoints
    HostStage st(c);
    const int ns = s->p.n_streams;
    const size_t kp_bytes = (size_t)n * s->p.n_joints * 3 * sizeof(float), nb = (size_t)n * 4;
    const size_t o_kp = st.part(kp_bytes), o_ids = st.part(nb), o_st = st.part(nb), o_rk = st.part(nb), o_fl = st.part((size_t)ns * 4);
    if (st.alloc()) return st.rc;
    float* d_kp = st.at<float>(o_kp);
    int32_t *d_ids = st.at<int32_t>(o_ids), *d_st = st.at<int32_t>(o_st), *d_rk = st.at<int32_t>(o_rk), *d_fl = st.at<int32_t>(o_fl);
    if (n) {
        st.up(d_kp, kpts, kp_bytes, "upload keypoints");
        st.up(d_ids, ids, nb, "upload ids");
        if (stream) st.up(d_st, stream, nb, "upload stream");
        if (rank) st.up(d_rk, rank, nb, "upload rank");
    }
    if (!st.rc) st.rc = update_enqueue(s, te, d_kp, d_ids, n && stream ? d_st : nullptr, n && rank ? d_rk : nullptr, n, step_mask, d_kp, d_fl, st.s);
    if (!st.rc) {
        if (n) st.down(out, d_kp, kp_bytes, "download keypoints");
        if (flags) st.down(flags, d_fl, (size_t)ns * 4, "download flags");
    }
    st.sync();
    return st.rc;
}

int vp_smoother_state_bytes(const vp_smooth_cfg* cfg, int64_t* bytes) {
    vp::EuroParams p;
    std::string why;
    if (cfg_check(cfg, p, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    if (!bytes) return fail(nullptr, VP_ERR_INVALID, "smoother: null bytes");
    *bytes = (int64_t)(vp::euro_stream_bytes(p.n_joints) * (size_t)p.n_streams);
    return VP_OK;
}

int vp_smoother_download_state(vp_smoother_handle s, void* out) {
    if (!s || !out) return VP_ERR_INVALID;
    return stage_download(s, out, s->state, s->state_bytes);
}

int vp_dbg_smooth_host(void* state, const vp_smooth_cfg* cfg, const float* kpts, const int32_t* ids, const int32_t* stream, const int32_t* rank, int32_t n,
                       uint64_t step_mask, const double* t_e, float* out, int32_t* flags) {
    vp::EuroParams p;
    std::string why;
    vp::EuroTe te;
    if (cfg_check(cfg, p, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    if (!state) return fail(nullptr, VP_ERR_INVALID, "smoother: null state");
    if (update_args(p, kpts, ids, n, step_mask, t_e, out, te, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    smooth_host((char*)state, p, te, kpts, ids, stream, rank, n, step_mask, out, flags);
    return VP_OK;
}

}  // extern "C"
