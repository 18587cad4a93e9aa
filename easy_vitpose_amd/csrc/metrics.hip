// vp_metrics_*: accuracy metrics against ground truth (PCK, AUC, EPE, NME, OKS recall) as an accumulating, stream-ordered device stage (semantics and summation
// order: metricsgeom.h), its synchronous host twin vp_metrics_update and the tap vp_dbg_metrics_host.  Two launches per update: metrics_rows_kernel, one workgroup
// per block of 64 rows (the lane is the row, the joints go round the four waves) that writes per-(block, joint) counts and tree sums into a workspace of the
// evaluator, and metrics_finish_kernel, one workgroup that adds the block partials in ascending block order into the state.  No atomics, no flags between
// workgroups: the state is a pure function of the inputs, bit for bit.
#include "api_internal.h"
#include "hoststage.h"
#include "stageobj.h"
#include "metricsgeom.h"

using namespace vpi;

namespace vp {

constexpr int MET_THREADS = 256, MET_WAVES = MET_THREADS / 64, MET_FIN_THREADS = 1024, MET_FIN_GROUPS = MET_FIN_THREADS / NMS_MAX_K;
constexpr int MET_HDR_WORDS = 15;   // what one thread each of the finish kernel adds: calls + rows, counted, nonfinite, oks_rows, oks_hits[10], oks_sum

// the per-block words that are not per joint (64 bytes)
struct MetricsBlockHdr {
    int32_t counted, nonfinite, oks_rows, oks_hits[METRICS_OKS_THRS], pad;
    double oks_sum;
};

// the workspace of one call: sums [blocks][2][K] (sum_norm, sum_px), cnt [blocks][kinds][K] (metrics_count_kinds order), hdr [blocks]
struct MetricsWs {
    double* sums;
    int32_t* cnt;
    MetricsBlockHdr* hdr;
};

// the balanced tree over the 64 lanes in lane order (pairs at distance 1, 2, ..., 32): every lane ends with the root's value, a + b == b + a bit for bit
__device__ inline double met_tree64(double v) {
#pragma unroll
    for (int d = 1; d < 64; d *= 2) v = v + __shfl_xor(v, d, 64);
    return v;
}

// One workgroup per block of 64 rows; lane = row, wave w takes joints w, w + 4, ...  The 12-byte records of a lane lie 12 K bytes apart: the four waves and the
// following iterations walk the same cache lines.  The OKS terms of a joint round pass through LDS so that every wave adds them in joint order (two buffers, one
// barrier per round).
__global__ __launch_bounds__(MET_THREADS) void metrics_rows_kernel(MetricsParams m, const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ norm,
                                                                   const float* __restrict__ area, const int32_t* __restrict__ rank, const int32_t* __restrict__ set,
                                                                   int32_t set_value, int n, const double* __restrict__ vars, MetricsWs ws, float* __restrict__ d_dist,
                                                                   float* __restrict__ d_oks) {
    __shared__ double terms[2][MET_WAVES][64];
    __shared__ int32_t wave_nonfinite[MET_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
    const int K = m.n_joints, C = metrics_count_kinds(m);
    const int i = b * METRICS_BLOCK + lane;
    const bool in = i < n;
    const bool counted = in && metrics_counted(rank, set, set_value, i);
    float ny = 1.0f, nx = 1.0f;
    const bool norm_on = counted && metrics_row_norm(norm, i, ny, nx);
    const bool oks_call = m.use_oks && area != nullptr;   // the same for every thread
    double a = 1.0;
    const bool oks_row = counted && metrics_oks_area(m, area, i, a);
    const double denom = nms_oks_denom(a, a);
    const float* p = pred + (size_t)(in ? i : 0) * 3 * K;
    const float* g = gt + (size_t)(in ? i : 0) * 3 * K;
    int nonfin = 0, oks_cnt = 0;
    double oks_sum = 0.0;
    const int rounds = (K + MET_WAVES - 1) / MET_WAVES;
    for (int c = 0; c < rounds; ++c) {
        const int j = c * MET_WAVES + wave;   // the same for every lane of a wave
        MetricsJoint r;
        r.vis = r.in_norm = false;
        r.qn = r.q1 = r.qa = 0.0f;
        if (j < K && counted) r = metrics_joint(p, g, j, ny, nx, norm_on, m);
        if (j < K) {
            const bool fn = r.in_norm && metrics_finite(r.qn), f1 = r.vis && metrics_finite(r.q1);
            int mine = 0;
            {
                const int c0 = __popcll(__ballot(r.in_norm)), c1 = __popcll(__ballot(r.vis));
                if (lane == 0) mine = c0;
                if (lane == 1) mine = c1;
            }
            for (int t = 0; t < m.n_pck; ++t) {
                const int h = __popcll(__ballot(r.in_norm && r.qn < m.pck_thr[t]));
                if (lane == 2 + t) mine = h;
            }
            for (int s = 0; s < m.auc_steps; ++s) {
                const int h = __popcll(__ballot(r.vis && r.qa < m.auc_thr[s]));
                if (lane == 2 + m.n_pck + s) mine = h;
            }
            nonfin += __popcll(__ballot(r.in_norm && !fn)) + __popcll(__ballot(r.vis && !f1));
            const double sn = met_tree64(fn ? (double)r.qn : 0.0), s1 = met_tree64(f1 ? (double)r.q1 : 0.0);
            if (lane < C) ws.cnt[((size_t)b * C + lane) * K + j] = mine;
            if (lane == 0) {
                ws.sums[((size_t)b * 2) * K + j] = sn;
                ws.sums[((size_t)b * 2 + 1) * K + j] = s1;
            }
            if (d_dist && in) d_dist[(size_t)i * K + j] = r.in_norm ? r.qn : -1.0f;
        }
        if (oks_call) {
            double t = -1.0;   // no term: exp() is never negative
            if (j < K && oks_row && r.vis) t = nms_oks_term(g, p, j, vars[j], denom);
            terms[c & 1][wave][lane] = t;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < MET_WAVES; ++w) {
                const double v = terms[c & 1][w][lane];
                if (v != -1.0) { oks_sum = oks_sum + v; ++oks_cnt; }
            }
        }
    }
    if (lane == 0) wave_nonfinite[wave] = nonfin;
    __syncthreads();
    if (wave != 0) return;
    const bool has = oks_row && oks_cnt > 0;
    const float oks = has ? nms_oks_mean(oks_sum, oks_cnt) : -1.0f;
    const bool okf = has && metrics_finite(oks);
    if (d_oks && in) d_oks[i] = oks;
    MetricsBlockHdr h;
    h.counted = __popcll(__ballot(counted));
    h.oks_rows = __popcll(__ballot(okf));
    h.nonfinite = __popcll(__ballot(has && !okf));
#pragma unroll
    for (int t = 0; t < METRICS_OKS_THRS; ++t) h.oks_hits[t] = __popcll(__ballot(okf && oks >= metrics_oks_thr(t)));
    h.pad = 0;
    h.oks_sum = met_tree64(okf ? (double)oks : 0.0);
    if (lane == 0) {
        for (int w = 0; w < MET_WAVES; ++w) h.nonfinite += wave_nonfinite[w];
        ws.hdr[b] = h;
    }
}

// One workgroup.  Thread (group q, joint j) adds the block partials of joint j in ascending block order into the state: the count kinds q, q + 4, ... and, in
// groups 2 and 3, sum_norm and sum_px.  Threads 0..14 then add one header / OKS word each.
__global__ __launch_bounds__(MET_FIN_THREADS) void metrics_finish_kernel(MetricsParams m, int n, int nblocks, MetricsWs ws, char* __restrict__ state) {
    int64_t* W = (int64_t*)state;
    double* D = (double*)state;
    const int t = threadIdx.x, q = t / NMS_MAX_K, j = t % NMS_MAX_K;
    const int K = m.n_joints, C = metrics_count_kinds(m);
    if (j < K) {
        for (int kind = q; kind < C; kind += MET_FIN_GROUPS) {
            int64_t s = 0;
            for (int b = 0; b < nblocks; ++b) s += ws.cnt[((size_t)b * C + kind) * K + j];
            W[metrics_w_count(K, kind) + j] += s;
        }
        if (q >= 2) {
            const int which = q - 2;   // 0 sum_norm, 1 sum_px
            double s = 0.0;
            for (int b = 0; b < nblocks; ++b) s = s + ws.sums[((size_t)b * 2 + which) * K + j];
            const size_t at = (which ? metrics_w_sum_px(K) : metrics_w_sum_norm(K)) + j;
            D[at] = D[at] + s;
        }
    }
    if (t >= MET_HDR_WORDS) return;
    if (t == 0) {
        W[METRICS_W_CALLS] += 1;
        W[METRICS_W_ROWS] += n;
    } else if (t == 14) {
        double s = 0.0;
        for (int b = 0; b < nblocks; ++b) s = s + ws.hdr[b].oks_sum;
        D[METRICS_W_OKS_SUM] = D[METRICS_W_OKS_SUM] + s;
    } else {
        // 1 counted, 2 nonfinite, 3 oks_rows, 4..13 oks_hits: MetricsBlockHdr's int32 words in their order
        int64_t s = 0;
        for (int b = 0; b < nblocks; ++b) s += ((const int32_t*)&ws.hdr[b])[t - 1];
        const int at = t == 1 ? METRICS_W_COUNTED : t == 2 ? METRICS_W_NONFINITE : t == 3 ? METRICS_W_OKS_ROWS : METRICS_W_OKS_HITS + (t - 4);
        W[at] += s;
    }
}

}  // namespace vp

struct vp_metrics : StageObj {
    vp::MetricsParams p{};
    char* state = nullptr;     // device, one allocation: state | vars double [K] | the workspace of a call (MetricsWs) for METRICS_MAX_BLOCKS blocks
    double* vars = nullptr;
    vp::MetricsWs ws{};
    size_t state_bytes = 0;
};

namespace {

// ---- the host model: metricsgeom.h run serially, block by block in the contract's summation order (HOST ONLY)
void metrics_host(char* state, const vp::MetricsParams& m, const double* vars, const float* pred, const float* gt, const float* norm, const float* area, const int32_t* rank,
                  const int32_t* set, int32_t set_value, int n, float* dist, float* oks_out) {
    using namespace vp;
    const int K = m.n_joints, C = metrics_count_kinds(m);
    const int nblocks = (n + METRICS_BLOCK - 1) / METRICS_BLOCK;
    std::vector<int64_t> cnt((size_t)C * K, 0);
    std::vector<double> call_sum((size_t)2 * K, 0.0), leaf((size_t)2 * K * METRICS_BLOCK);
    int64_t counted_rows = 0, nonfinite = 0, oks_rows = 0, oks_hits[METRICS_OKS_THRS] = {0};
    double oks_sum = 0.0, oks_leaf[METRICS_BLOCK];
    for (int b = 0; b < nblocks; ++b) {
        std::fill(leaf.begin(), leaf.end(), 0.0);
        for (int l = 0; l < METRICS_BLOCK; ++l) {
            oks_leaf[l] = 0.0;
            const int i = b * METRICS_BLOCK + l;
            if (i >= n) continue;
            if (dist)
                for (int j = 0; j < K; ++j) dist[(size_t)i * K + j] = -1.0f;
            if (oks_out) oks_out[i] = -1.0f;
            if (!metrics_counted(rank, set, set_value, i)) continue;
            ++counted_rows;
            float ny, nx;
            const bool norm_on = metrics_row_norm(norm, i, ny, nx);
            double a = 1.0;
            const bool oks_row = metrics_oks_area(m, area, i, a);
            const double denom = nms_oks_denom(a, a);
            const float* p = pred + (size_t)i * 3 * K;
            const float* g = gt + (size_t)i * 3 * K;
            double osum = 0.0;
            int ocnt = 0;
            for (int j = 0; j < K; ++j) {
                const MetricsJoint r = metrics_joint(p, g, j, ny, nx, norm_on, m);
                if (r.in_norm) {
                    ++cnt[(size_t)0 * K + j];
                    if (dist) dist[(size_t)i * K + j] = r.qn;
                    if (metrics_finite(r.qn)) leaf[((size_t)j * 2) * METRICS_BLOCK + l] = (double)r.qn;
                    else ++nonfinite;
                    for (int t = 0; t < m.n_pck; ++t) cnt[(size_t)(2 + t) * K + j] += r.qn < m.pck_thr[t];
                }
                if (r.vis) {
                    ++cnt[(size_t)1 * K + j];
                    if (metrics_finite(r.q1)) leaf[((size_t)j * 2 + 1) * METRICS_BLOCK + l] = (double)r.q1;
                    else ++nonfinite;
                    for (int s = 0; s < m.auc_steps; ++s) cnt[(size_t)(2 + m.n_pck + s) * K + j] += r.qa < m.auc_thr[s];
                    if (oks_row) { osum = osum + nms_oks_term(g, p, j, vars[j], denom); ++ocnt; }
                }
            }
            if (oks_row && ocnt > 0) {
                const float oks = nms_oks_mean(osum, ocnt);
                if (oks_out) oks_out[i] = oks;
                if (metrics_finite(oks)) {
                    ++oks_rows;
                    for (int t = 0; t < METRICS_OKS_THRS; ++t) oks_hits[t] += oks >= metrics_oks_thr(t);
                    oks_leaf[l] = (double)oks;
                } else {
                    ++nonfinite;
                }
            }
        }
        for (int e = 0; e < 2 * K; ++e) {   // e = 2 j + which
            const size_t at = (size_t)(e & 1) * K + (e >> 1);
            call_sum[at] = call_sum[at] + metrics_tree64(&leaf[(size_t)e * METRICS_BLOCK]);
        }
        oks_sum = oks_sum + metrics_tree64(oks_leaf);
    }
    int64_t* W = (int64_t*)state;
    double* D = (double*)state;
    W[METRICS_W_CALLS] += 1;
    W[METRICS_W_ROWS] += n;
    W[METRICS_W_COUNTED] += counted_rows;
    W[METRICS_W_NONFINITE] += nonfinite;
    W[METRICS_W_OKS_ROWS] += oks_rows;
    for (int t = 0; t < METRICS_OKS_THRS; ++t) W[METRICS_W_OKS_HITS + t] += oks_hits[t];
    D[METRICS_W_OKS_SUM] = D[METRICS_W_OKS_SUM] + oks_sum;
    for (int kind = 0; kind < C; ++kind)
        for (int j = 0; j < K; ++j) W[metrics_w_count(K, kind) + j] += cnt[(size_t)kind * K + j];
    for (int j = 0; j < K; ++j) {
        D[metrics_w_sum_norm(K) + j] = D[metrics_w_sum_norm(K) + j] + call_sum[j];
        D[metrics_w_sum_px(K) + j] = D[metrics_w_sum_px(K) + j] + call_sum[(size_t)K + j];
    }
}

// every refusal of the configuration (HOST ONLY), before anything is enqueued or allocated
int cfg_check(const vp_metrics_cfg* cfg, const float* sigmas, vp::MetricsParams& p, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "metrics: " + m; return (int)VP_ERR_INVALID; };
    if (!cfg) return bad("null cfg");
    if (cfg->n_joints < 1 || cfg->n_joints > vp::NMS_MAX_K) return bad("n_joints = " + std::to_string(cfg->n_joints) + " outside 1.." + std::to_string(vp::NMS_MAX_K));
    if (cfg->n_pck < 0 || cfg->n_pck > vp::METRICS_MAX_PCK) return bad("n_pck = " + std::to_string(cfg->n_pck) + " outside 0.." + std::to_string(vp::METRICS_MAX_PCK));
    if (cfg->auc_steps < 0 || cfg->auc_steps > vp::METRICS_MAX_AUC)
        return bad("auc_steps = " + std::to_string(cfg->auc_steps) + " outside 0.." + std::to_string(vp::METRICS_MAX_AUC));
    for (int t = 0; t < cfg->n_pck; ++t)
        if (!vp::metrics_finite(cfg->pck_thr[t])) return bad("pck_thr[" + std::to_string(t) + "] not finite");
    if (!vp::metrics_finite(cfg->vis_thr)) return bad("vis_thr not finite");
    if (cfg->auc_steps > 0 && !(vp::metrics_finite(cfg->auc_norm) && cfg->auc_norm > 0.0)) return bad("auc_norm not finite or <= 0 with auc_steps > 0");
    if (cfg->use_oks) {
        if (!sigmas) return bad("use_oks without sigmas");
        for (int j = 0; j < cfg->n_joints; ++j)
            if (!(vp::metrics_finite(sigmas[j]) && sigmas[j] > 0.0f)) return bad("sigma[" + std::to_string(j) + "] not finite or <= 0");
    }
    p = vp::MetricsParams{};
    p.auc_norm = cfg->auc_steps > 0 ? cfg->auc_norm : 1.0;
    for (int t = 0; t < cfg->n_pck; ++t) p.pck_thr[t] = cfg->pck_thr[t];
    for (int s = 0; s < cfg->auc_steps; ++s) p.auc_thr[s] = (float)((double)s / (double)cfg->auc_steps);
    p.vis_thr = cfg->vis_thr;
    p.n_joints = cfg->n_joints; p.n_pck = cfg->n_pck; p.auc_steps = cfg->auc_steps; p.use_oks = cfg->use_oks ? 1 : 0;
    return VP_OK;
}

int update_args(const void* pred, const void* gt, int n, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "metrics: " + m; return (int)VP_ERR_INVALID; };
    if (n < 0 || n > vp::METRICS_MAX_ROWS) return bad("n = " + std::to_string(n) + " outside 0.." + std::to_string(vp::METRICS_MAX_ROWS));
    if (n > 0 && !(pred && gt)) return bad("null pred or gt with n > 0");
    return VP_OK;
}

// the checked call on stream q: the rows kernel (n > 0), then the finish kernel
int update_enqueue(vp_metrics* e, const float* d_pred, const float* d_gt, const float* d_norm, const float* d_area, const int32_t* d_rank, const int32_t* d_set, int32_t set_value,
                   int n, float* d_dist, float* d_oks, hipStream_t q) {
    vp_ctx* c = e->c;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int nblocks = (n + vp::METRICS_BLOCK - 1) / vp::METRICS_BLOCK;
    if (nblocks > 0) {
        hipLaunchKernelGGL(vp::metrics_rows_kernel, dim3(nblocks), dim3(vp::MET_THREADS), 0, q, e->p, d_pred, d_gt, d_norm, d_area, d_rank, d_set, set_value, n,
                           (const double*)e->vars, e->ws, d_dist, d_oks);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(vp::metrics_finish_kernel, dim3(1), dim3(vp::MET_FIN_THREADS), 0, q, e->p, n, nblocks, e->ws, e->state);
    HIPCHK(c, hipGetLastError());
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_metrics_create(vp_handle c, const vp_metrics_cfg* cfg, const float* sigmas, vp_metrics_handle* out) {
    return stage_create(c, out, [&](vp_metrics* e, std::string* why) { return cfg_check(cfg, sigmas, e->p, why); },
                        [&](vp_metrics* e) {
                            const vp::MetricsParams& p = e->p;
                            const int K = p.n_joints, C = vp::metrics_count_kinds(p), B = vp::METRICS_MAX_BLOCKS;
                            e->state_bytes = vp::metrics_state_words(K, p.n_pck, p.auc_steps) * 8;
                            StageLayout lay;   // state | vars | sums | counts | block headers
                            const size_t o_state = lay.part(e->state_bytes), o_vars = lay.part((size_t)K * 8), o_sums = lay.part((size_t)B * 2 * K * 8),
                                         o_cnt = lay.part((size_t)B * C * K * 4), o_hdr = lay.part((size_t)B * sizeof(vp::MetricsBlockHdr));
                            std::vector<double> vars((size_t)K, 1.0);
                            if (p.use_oks)
                                for (int j = 0; j < K; ++j) vars[j] = vp::nms_var(sigmas[j]);
                            char* mem = e->alloc(lay.end, 0);
                            e->up(mem + o_vars, vars.data(), (size_t)K * 8);
                            e->state = mem + o_state;
                            e->vars = (double*)(mem + o_vars);
                            e->ws.sums = (double*)(mem + o_sums);
                            e->ws.cnt = (int32_t*)(mem + o_cnt);
                            e->ws.hdr = (vp::MetricsBlockHdr*)(mem + o_hdr);
                            return "metrics state: ";
                        });
}

int vp_metrics_destroy(vp_metrics_handle e) { return stage_destroy(e); }

int vp_metrics_reset_stream(vp_metrics_handle e, void* caller_stream) {
    if (!e) return VP_ERR_INVALID;
    return stage_reset(e, e->state, e->state_bytes, caller_stream);
}

int vp_metrics_update_stream(vp_metrics_handle e, const float* d_pred, const float* d_gt, const float* d_norm, const float* d_area, const int32_t* d_rank, const int32_t* d_set,
                             int32_t set_value, int32_t n, float* d_dist, float* d_oks, void* caller_stream) {
    if (!e) return VP_ERR_INVALID;
    std::string why;
    if (update_args(d_pred, d_gt, n, &why)) return fail(e->c, VP_ERR_INVALID, why);
    return update_enqueue(e, d_pred, d_gt, d_norm, d_area, d_rank, d_set, set_value, n, d_dist, d_oks, (hipStream_t)caller_stream);
}

int vp_metrics_update(vp_metrics_handle e, const float* pred, const float* gt, const float* norm, const float* area, const int32_t* rank, const int32_t* set, int32_t set_value,
                      int32_t n, float* dist, float* oks) {
    if (!e) return VP_ERR_INVALID;
    vp_ctx* c = e->c;
    std::string why;
    if (update_args(pred, gt, n, &why)) return fail(c, VP_ERR_INVALID, why);
    // one scratch block: pred | gt | norm | area | rank | set | oks | dist
    HostStage st(c);
    const int K = e->p.n_joints;
    const size_t kp_bytes = (size_t)n * K * 3 * sizeof(float), nb = (size_t)n * 4, dist_bytes = (size_t)n * K * 4;
    const size_t o_pred = st.part(kp_bytes), o_gt = st.part(kp_bytes), o_norm = st.part((size_t)n * 8), o_area = st.part(nb), o_rank = st.part(nb), o_set = st.part(nb), o_oks = st.part(nb),
                 o_dist = st.part(dist_bytes);
    if (st.alloc()) return st.rc;
    float *d_pred = st.at<float>(o_pred), *d_gt = st.at<float>(o_gt), *d_norm = st.at<float>(o_norm), *d_area = st.at<float>(o_area), *d_oks = st.at<float>(o_oks),
          *d_dist = st.at<float>(o_dist);
    int32_t *d_rank = st.at<int32_t>(o_rank), *d_set = st.at<int32_t>(o_set);
    if (n) {
        st.up(d_pred, pred, kp_bytes, "upload pred");
        st.up(d_gt, gt, kp_bytes, "upload gt");
        if (norm) st.up(d_norm, norm, (size_t)n * 8, "upload norm");
        if (area) st.up(d_area, area, nb, "upload area");
        if (rank) st.up(d_rank, rank, nb, "upload rank");
        if (set) st.up(d_set, set, nb, "upload set");
    }
    if (!st.rc)
        st.rc = update_enqueue(e, d_pred, d_gt, n && norm ? d_norm : nullptr, n && area ? d_area : nullptr, n && rank ? d_rank : nullptr, n && set ? d_set : nullptr, set_value, n,
                               n && dist ? d_dist : nullptr, n && oks ? d_oks : nullptr, st.s);
    if (!st.rc && n) {
        if (dist) st.down(dist, d_dist, dist_bytes, "download dist");
        if (oks) st.down(oks, d_oks, nb, "download oks");
    }
    st.sync();
    return st.rc;
}

int vp_metrics_snapshot_stream(vp_metrics_handle e, void* d_out, void* caller_stream) {
    if (!e) return VP_ERR_INVALID;
    vp_ctx* c = e->c;
    if (!d_out) return fail(c, VP_ERR_INVALID, "metrics: null snapshot destination");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpyAsync(d_out, e->state, e->state_bytes, hipMemcpyDeviceToDevice, (hipStream_t)caller_stream));
    return VP_OK;
}

int vp_metrics_state_bytes(const vp_metrics_cfg* cfg, int64_t* bytes) {
    if (!cfg) return fail(nullptr, VP_ERR_INVALID, "metrics: null cfg");
    if (!bytes) return fail(nullptr, VP_ERR_INVALID, "metrics: null bytes");
    if (cfg->n_joints < 1 || cfg->n_joints > vp::NMS_MAX_K || cfg->n_pck < 0 || cfg->n_pck > vp::METRICS_MAX_PCK || cfg->auc_steps < 0 || cfg->auc_steps > vp::METRICS_MAX_AUC)
        return fail(nullptr, VP_ERR_INVALID, "metrics: n_joints, n_pck or auc_steps out of range");
    *bytes = (int64_t)(vp::metrics_state_words(cfg->n_joints, cfg->n_pck, cfg->auc_steps) * 8);
    return VP_OK;
}

int vp_metrics_download_state(vp_metrics_handle e, void* out) {
    if (!e || !out) return VP_ERR_INVALID;
    return stage_download(e, out, e->state, e->state_bytes);
}

int vp_dbg_metrics_host(void* state, const vp_metrics_cfg* cfg, const float* sigmas, const float* pred, const float* gt, const float* norm, const float* area, const int32_t* rank,
                        const int32_t* set, int32_t set_value, int32_t n, float* dist, float* oks) {
    vp::MetricsParams p;
    std::string why;
    if (cfg_check(cfg, sigmas, p, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    if (!state) return fail(nullptr, VP_ERR_INVALID, "metrics: null state");
    if (update_args(pred, gt, n, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    std::vector<double> vars((size_t)p.n_joints, 1.0);
    if (p.use_oks)
        for (int j = 0; j < p.n_joints; ++j) vars[j] = vp::nms_var(sigmas[j]);
    metrics_host((char*)state, p, vars.data(), pred, gt, norm, area, rank, set, set_value, n, dist, oks);
    return VP_OK;
}

}  // extern "C"
