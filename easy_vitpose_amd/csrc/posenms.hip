// vp_pose_nms_stream: person scores and per-frame OKS pose NMS on the device (semantics: posenms.h), its synchronous host twin vp_pose_nms and
// the two taps vp_dbg_pose_nms_host / vp_dbg_pose_oks.  No atomics and every sum in joint order: a call is bit-identical from run to run and
// independent of the launch shape.
#include "api_internal.h"
#include "hoststage.h"
#include "posenms.h"

using namespace vpi;

namespace vp {

constexpr int NMS_THREADS = 256, NMS_WAVES = NMS_THREADS / 64;

// One workgroup per frame.  Pass 1 walks all n rows in tiles of 256 and gathers the frame's members in ascending row order (ballot prefix per wave,
// wave counts through LDS); on the way every row gets its instance score and rank -1 from exactly one thread of the grid: a member's from its frame's
// workgroup, any other row i from workgroup i % n_frames.  Then, per pick: a workgroup arg-max over the live members (two barriers per pick), the
// pick's keypoints staged in LDS, then the candidates: L lanes per member, L the largest power of two with members * L <= 256 (1 from 129 members on, 64 for
// up to 4).  Lane l of a member's group computes the terms exp(-e_j) of joints j = l, l + L, ... from the member's keypoints in global memory (L2; 12 bytes per
// lane, contiguous); after each round of L joints the group adds the L terms in joint order, every lane the same chain of shuffles and fp64 adds -- the sum
// of nms_oks whatever L is (a gated-out joint contributes +0.0, which leaves a sum of non-negative terms, or a NaN, as it is; the joints are counted apart).
// A thread per member with its K exps in a row leaves most lanes idle below 256 members, and staging the terms through LDS for a thread per member to add puts the
// summing threads and two barriers per pass on the critical path: both were tried and dropped.  LDS arrays indexed by member are read
// with member = thread + 256 t or member = group + (256 / L) t: consecutive lanes or lane groups, consecutive 4- / 8-byte elements, no bank conflict.
// More than NMS_MAX_PER_FRAME members: rank -2.
__host__ __device__ inline int nms_lanes(int members) {   // lanes per member of the candidate pass
    int L = 1;
    while (L < 64 && members * (L * 2) <= NMS_THREADS) L *= 2;
    return L;
}

// OKS of candidate d against pick g on a group of L lanes (a power of two <= 64, the group aligned to L, all of its lanes here together), l = this lane's place
// in the group: nms_oks with the terms spread over the lanes and added in joint order.  Every lane of the group returns the same value.
__device__ inline float oks_lanes(const float* g, const float* d, int K, double a_g, double a_d, const double* vars, const NmsParams& p, int L, int l) {
    const double denom = nms_oks_denom(a_g, a_d);
    double sum = 0.0;
    int cnt = 0;
    for (int j0 = 0; j0 < K; j0 += L) {
        const int j = j0 + l;
        double term = 0.0;
        if (j < K && nms_oks_gate(d, j, p)) { term = nms_oks_term(g, d, j, vars[j], denom); ++cnt; }
        for (int q = 0; q < L; ++q) sum += __shfl(term, q, L);   // joints j0 .. j0 + L - 1 in order
    }
    for (int q = L >> 1; q > 0; q >>= 1) cnt += __shfl_xor(cnt, q, L);
    return nms_oks_mean(sum, cnt);
}

__global__ __launch_bounds__(NMS_THREADS) void pose_nms_kernel(const float* __restrict__ kpts, int n, int K, const float* __restrict__ box_score, int score_stride,
                                                                const int32_t* __restrict__ p9, const int32_t* __restrict__ status, int n_frames, NmsParams p,
                                                                NmsVars vars, float* __restrict__ score_out, int32_t* __restrict__ rank_out,
                                                                int32_t* __restrict__ count_out) {
    __shared__ double s_score[NMS_MAX_PER_FRAME], s_area[NMS_MAX_PER_FRAME];
    __shared__ int32_t s_idx[NMS_MAX_PER_FRAME], s_live[NMS_MAX_PER_FRAME], s_rank[NMS_MAX_PER_FRAME];
    __shared__ float s_pick[NMS_MAX_K * 3];
    __shared__ double s_wkey[NMS_WAVES];
    __shared__ int32_t s_wm[NMS_WAVES], s_wcnt[NMS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
    const size_t row = (size_t)K * 3;

    int total = 0;
    for (int base = 0; base < n; base += NMS_THREADS) {
        const int i = base + tid;
        const bool in = i < n;
        const int32_t fi = in ? p9[(size_t)i * 9] : -1;
        const bool member = in && nms_member(status ? status[i] : 0, fi, n_frames);
        const bool mine = member && fi == f;
        float sc = 0.f;
        if (in && (member ? mine : i % n_frames == f)) {
            sc = nms_instance_score(kpts + (size_t)i * row, K, box_score[(size_t)i * score_stride], p);
            score_out[i] = sc;
            rank_out[i] = -1;
        }
        const unsigned long long b = __ballot(mine);
        if (lane == 0) s_wcnt[wave] = __popcll(b);
        __syncthreads();
        int off = total + __popcll(b & ((1ull << lane) - 1ull)), all = 0;
        for (int w = 0; w < NMS_WAVES; ++w) {
            if (w < wave) off += s_wcnt[w];
            all += s_wcnt[w];
        }
        if (mine && off < NMS_MAX_PER_FRAME) {
            s_idx[off] = i;
            s_score[off] = (double)sc;
            s_area[off] = nms_area(p9 + (size_t)i * 9);
            s_live[off] = 1;
            s_rank[off] = -1;
        }
        total += all;
        __syncthreads();
    }
    if (total > NMS_MAX_PER_FRAME) {   // the frame is not processed: -2 on every member (written by the thread that wrote its -1)
        for (int base = 0; base < n; base += NMS_THREADS) {
            const int i = base + tid;
            if (i < n && nms_member(status ? status[i] : 0, p9[(size_t)i * 9], n_frames) && p9[(size_t)i * 9] == f) rank_out[i] = -2;
        }
        if (count_out && tid == 0) count_out[f] = 0;
        return;
    }

    const int L = nms_lanes(total);
    int picks = 0;
    while (true) {
        double bk = -INFINITY;
        int32_t bm = INT32_MAX;
        for (int m = tid; m < total; m += NMS_THREADS)
            if (s_live[m]) {
                const double k = nms_key(s_score[m]);
                if (nms_before(k, m, bk, bm)) { bk = k; bm = m; }
            }
        for (int d = 32; d > 0; d >>= 1) {
            const double ok = __shfl_xor(bk, d);
            const int32_t om = __shfl_xor(bm, d);
            if (nms_before(ok, om, bk, bm)) { bk = ok; bm = om; }
        }
        if (lane == 0) { s_wkey[wave] = bk; s_wm[wave] = bm; }
        __syncthreads();
        bk = s_wkey[0]; bm = s_wm[0];
        for (int w = 1; w < NMS_WAVES; ++w)
            if (nms_before(s_wkey[w], s_wm[w], bk, bm)) { bk = s_wkey[w]; bm = s_wm[w]; }
        if (bm == INT32_MAX) break;   // nothing live (uniform: every thread reads the same four entries)
        const int g = s_idx[bm];
        if (tid == 0) { s_live[bm] = 0; s_rank[bm] = picks; }
        ++picks;
        if (p.soft && picks >= p.max_dets) break;   // nms.py:189: what the last pick would rescore is never picked
        for (int t = tid; t < K * 3; t += NMS_THREADS) s_pick[t] = kpts[(size_t)g * row + t];
        __syncthreads();
        const double a_g = s_area[bm];
        for (int m = tid / L; m < total; m += NMS_THREADS / L) {   // a group's lanes share m: they branch together, and the shuffles stay inside the group
            if (!s_live[m]) continue;
            const int l = tid & (L - 1);
            const float oks = oks_lanes(s_pick, kpts + (size_t)s_idx[m] * row, K, a_g, s_area[m], vars.v, p, L, l);
            if (l == 0) {
                if (p.soft) s_score[m] *= nms_soft_factor(oks, p.oks_thr);
                else if (oks > p.oks_thr) s_live[m] = 0;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    for (int m = tid; m < total; m += NMS_THREADS) {
        const int32_t r = s_rank[m];
        rank_out[s_idx[m]] = r;
        if (p.soft && r >= 0) score_out[s_idx[m]] = (float)s_score[m];   // the score it had when it was picked
    }
    if (count_out && tid == 0) count_out[f] = picks;
}

// oks [n, n]: entry (g, d) = candidate d against pick g, every row taken as it is (no status, no frames).  It runs the product's oks_lanes with the L a frame of n
// members gets (nms_lanes), one group of L lanes per entry, so the tap pins the lane-split sum for that L against the serial nms_oks of the host tap.
__global__ __launch_bounds__(NMS_THREADS) void pose_oks_kernel(const float* __restrict__ kpts, int n, int K, const int32_t* __restrict__ p9, NmsParams p, NmsVars vars,
                                                                int L, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * NMS_THREADS + threadIdx.x, j = t / L;
    if (j >= (size_t)n * n) return;   // a whole group at a time: L divides the block
    const size_t g = j / n, d = j % n, row = (size_t)K * 3;
    const int l = (int)(t & (size_t)(L - 1));
    const float oks = oks_lanes(kpts + g * row, kpts + d * row, K, nms_area(p9 + g * 9), nms_area(p9 + d * 9), vars.v, p, L, l);
    if (l == 0) out[j] = oks;
}

}  // namespace vp

namespace {

// every refusal of the four entries (HOST ONLY), before anything is enqueued; fills the kernel's parameters
int nms_args(bool need_ptrs, int n, int k, int score_stride, int n_frames, const vp_pose_nms_cfg* cfg, vp::NmsParams& p, vp::NmsVars& vars, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "pose nms: " + m; return (int)VP_ERR_INVALID; };
    if (!cfg) return bad("null cfg");
    if (n < 0) return bad("negative n");
    if (n > 0 && !need_ptrs) return bad("null keypoint, box score, crop params, score or rank pointer");
    if (k < 1 || k > VP_NMS_MAX_K) return bad("k = " + std::to_string(k) + " outside 1.." + std::to_string(VP_NMS_MAX_K));
    if (cfg->n_sigmas != k || !cfg->sigmas) return bad("n_sigmas = " + std::to_string(cfg->n_sigmas) + " for k = " + std::to_string(k) + " joints (or a null table)");
    for (int j = 0; j < k; ++j)
        if (!std::isfinite(cfg->sigmas[j]) || !(cfg->sigmas[j] > 0.f)) return bad("sigma " + std::to_string(j) + " is not a finite value > 0");
    if (!(cfg->oks_thr > 0.f && cfg->oks_thr <= 1.f)) return bad("oks_thr outside (0, 1]");
    if (cfg->soft && cfg->max_dets < 1) return bad("soft with max_dets < 1");
    if (n > 0 && n_frames < 1) return bad("n > 0 with n_frames < 1");
    if (n_frames < 0) return bad("negative n_frames");
    if (score_stride < 1) return bad("score_stride < 1");
    p.oks_thr = cfg->oks_thr; p.vis_thr = cfg->vis_thr; p.use_vis_thr = cfg->use_vis_thr != 0; p.soft = cfg->soft != 0; p.max_dets = cfg->max_dets;
    std::memset(&vars, 0, sizeof(vars));
    for (int j = 0; j < k; ++j) vars.v[j] = vp::nms_var(cfg->sigmas[j]);
    return VP_OK;
}

// the checked call on stream s: launches only
int nms_enqueue(vp_ctx* c, const float* d_kpts, int n, int k, const float* d_box_score, int score_stride, const int32_t* d_p9, const int32_t* d_status, int n_frames,
                const vp::NmsParams& p, const vp::NmsVars& vars, float* d_score, int32_t* d_rank, int32_t* d_count, hipStream_t s) {
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if (n == 0) {
        if (d_count && n_frames > 0) HIPCHK(c, hipMemsetAsync(d_count, 0, (size_t)n_frames * 4, s));
        return VP_OK;
    }
    hipLaunchKernelGGL(vp::pose_nms_kernel, dim3(n_frames), dim3(vp::NMS_THREADS), 0, s, d_kpts, n, k, d_box_score, score_stride, d_p9, d_status, n_frames, p, vars,
                       d_score, d_rank, d_count);
    HIPCHK(c, hipGetLastError());
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_pose_nms_stream(vp_handle c, const float* d_kpts, int32_t n, int32_t k, const float* d_box_score, int32_t score_stride, const int32_t* d_crop_params,
                       const int32_t* d_status, int32_t n_frames, const vp_pose_nms_cfg* cfg, float* d_score, int32_t* d_rank, int32_t* d_count, void* caller_stream) {
    if (!c) return VP_ERR_INVALID;
    vp::NmsParams p;
    vp::NmsVars vars;
    std::string why;
    if (nms_args(d_kpts && d_box_score && d_crop_params && d_score && d_rank, n, k, score_stride, n_frames, cfg, p, vars, &why)) return fail(c, VP_ERR_INVALID, why);
    return nms_enqueue(c, d_kpts, n, k, d_box_score, score_stride, d_crop_params, d_status, n_frames, p, vars, d_score, d_rank, d_count, (hipStream_t)caller_stream);
}

int vp_pose_nms(vp_handle c, const float* kpts, int32_t n, int32_t k, const float* box_score, int32_t score_stride, const int32_t* crop_params, const int32_t* status,
                int32_t n_frames, const vp_pose_nms_cfg* cfg, float* score, int32_t* rank, int32_t* count) {
    if (!c) return VP_ERR_INVALID;
    vp::NmsParams p;
    vp::NmsVars vars;
    std::string why;
    if (nms_args(kpts && box_score && crop_params && score && rank, n, k, score_stride, n_frames, cfg, p, vars, &why)) return fail(c, VP_ERR_INVALID, why);
    if (n == 0) {
        if (count && n_frames > 0) std::memset(count, 0, (size_t)n_frames * 4);
        return VP_OK;
    }
    // one scratch block: kpts | box scores | crop params | status | score | rank | count
    HostStage st(c);
    const size_t kp_bytes = (size_t)n * k * 12, bs_bytes = ((size_t)(n - 1) * score_stride + 1) * 4, nb = (size_t)n * 4;
    const size_t o_kp = st.part(kp_bytes), o_bs = st.part(bs_bytes), o_p9 = st.part((size_t)n * 36), o_st = st.part(nb), o_sc = st.part(nb), o_rk = st.part(nb),
                 o_ct = st.part((size_t)n_frames * 4);
    if (st.alloc()) return st.rc;
    float *d_kp = st.at<float>(o_kp), *d_bs = st.at<float>(o_bs), *d_sc = st.at<float>(o_sc);
    int32_t *d_p9 = st.at<int32_t>(o_p9), *d_st = st.at<int32_t>(o_st), *d_rk = st.at<int32_t>(o_rk), *d_ct = st.at<int32_t>(o_ct);
    st.up(d_kp, kpts, kp_bytes, "upload keypoints");
    st.up(d_bs, box_score, bs_bytes, "upload box scores");
    st.up(d_p9, crop_params, (size_t)n * 36, "upload crop params");
    if (status) st.up(d_st, status, nb, "upload status");
    if (!st.rc) st.rc = nms_enqueue(c, d_kp, n, k, d_bs, score_stride, d_p9, status ? d_st : nullptr, n_frames, p, vars, d_sc, d_rk, d_ct, st.s);
    if (!st.rc) {
        st.down(score, d_sc, nb, "download score");
        st.down(rank, d_rk, nb, "download rank");
        if (count) st.down(count, d_ct, (size_t)n_frames * 4, "download count");
    }
    st.sync();
    return st.rc;
}

// the semantics of posenms.h run row by row on the host: what pose_nms_kernel computes, in the same order
int vp_dbg_pose_nms_host(const float* kpts, int32_t n, int32_t k, const float* box_score, int32_t score_stride, const int32_t* crop_params, const int32_t* status,
                         int32_t n_frames, const vp_pose_nms_cfg* cfg, float* score, int32_t* rank, int32_t* count) {
    vp::NmsParams p;
    vp::NmsVars vars;
    std::string why;
    if (nms_args(kpts && box_score && crop_params && score && rank, n, k, score_stride, n_frames, cfg, p, vars, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    if (count && n_frames > 0) std::memset(count, 0, (size_t)n_frames * 4);
    if (n == 0) return VP_OK;
    const size_t row = (size_t)k * 3;
    std::vector<std::vector<int32_t>> members((size_t)n_frames);
    for (int i = 0; i < n; ++i) {
        score[i] = vp::nms_instance_score(kpts + i * row, k, box_score[(size_t)i * score_stride], p);
        rank[i] = -1;
        const int32_t f = crop_params[(size_t)i * 9];
        if (vp::nms_member(status ? status[i] : 0, f, n_frames)) members[f].push_back(i);
    }
    std::vector<double> sc, area;
    std::vector<char> live;
    for (int f = 0; f < n_frames; ++f) {
        const std::vector<int32_t>& idx = members[f];
        const int total = (int)idx.size();
        if (total > vp::NMS_MAX_PER_FRAME) {
            for (int32_t i : idx) rank[i] = -2;
            continue;
        }
        sc.resize(total); area.resize(total); live.assign(total, 1);
        for (int m = 0; m < total; ++m) { sc[m] = (double)score[idx[m]]; area[m] = vp::nms_area(crop_params + (size_t)idx[m] * 9); }
        int picks = 0;
        while (true) {
            double bk = -INFINITY;
            int32_t bm = INT32_MAX;
            for (int m = 0; m < total; ++m)
                if (live[m] && vp::nms_before(vp::nms_key(sc[m]), m, bk, bm)) { bk = vp::nms_key(sc[m]); bm = m; }
            if (bm == INT32_MAX) break;
            live[bm] = 0;
            rank[idx[bm]] = picks++;
            if (p.soft) score[idx[bm]] = (float)sc[bm];
            if (p.soft && picks >= p.max_dets) break;
            const float* g = kpts + idx[bm] * row;
            for (int m = 0; m < total; ++m)
                if (live[m]) {
                    const float oks = vp::nms_oks(g, kpts + idx[m] * row, k, area[bm], area[m], vars.v, p);
                    if (p.soft) sc[m] *= vp::nms_soft_factor(oks, p.oks_thr);
                    else if (oks > p.oks_thr) live[m] = 0;
                }
        }
        if (count) count[f] = picks;
    }
    return VP_OK;
}

int vp_dbg_pose_oks(int32_t device_id, const float* kpts, int32_t n, int32_t k, const int32_t* crop_params, const vp_pose_nms_cfg* cfg, float* oks) {
    vp::NmsParams p;
    vp::NmsVars vars;
    std::string why;
    if (nms_args(kpts && crop_params && oks, n, k, 1, 1, cfg, p, vars, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    if (n > 32768) return fail(nullptr, VP_ERR_INVALID, "pose nms: vp_dbg_pose_oks takes at most 32768 rows");
    if (n == 0) return VP_OK;
    const size_t row = (size_t)k * 3;
    if (device_id < 0) {
        for (int g = 0; g < n; ++g)
            for (int d = 0; d < n; ++d)
                oks[(size_t)g * n + d] = vp::nms_oks(kpts + g * row, kpts + d * row, k, vp::nms_area(crop_params + (size_t)g * 9), vp::nms_area(crop_params + (size_t)d * 9), vars.v, p);
        return VP_OK;
    }
    vp_ctx* c = nullptr;   // errors are reported through the create-error slot
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(c, VP_ERR_HIP, "no HIP device available (no CPU fallback)");
    if (device_id >= ndev) return fail(c, VP_ERR_INVALID, "device_id out of range");
    HIPCHK(c, hipSetDevice(device_id));
    HostStage st(c);   // kpts | crop params | oks; blocking copies around a launch on the default stream
    const size_t o_kp = st.part((size_t)n * row * 4), o_p9 = st.part((size_t)n * 36), o_out = st.part((size_t)n * n * 4);
    if (st.alloc()) return st.rc;
    float *d_kp = st.at<float>(o_kp), *d_out = st.at<float>(o_out);
    int32_t* d_p9 = st.at<int32_t>(o_p9);
    st.chk(hipMemcpy(d_kp, kpts, (size_t)n * row * 4, hipMemcpyHostToDevice), "upload keypoints");
    st.chk(hipMemcpy(d_p9, crop_params, (size_t)n * 36, hipMemcpyHostToDevice), "upload crop params");
    if (!st.rc) {
        const int L = vp::nms_lanes(n);
        hipLaunchKernelGGL(vp::pose_oks_kernel, dim3((unsigned)(((size_t)n * n * L + vp::NMS_THREADS - 1) / vp::NMS_THREADS)), dim3(vp::NMS_THREADS), 0, 0, d_kp, n, k, d_p9,
                           p, vars, L, d_out);
        st.chk(hipGetLastError(), "pose_oks_kernel");
        st.chk(hipMemcpy(oks, d_out, (size_t)n * n * 4, hipMemcpyDeviceToHost), "download oks");
    }
    return st.rc;
}

}  // extern "C"
