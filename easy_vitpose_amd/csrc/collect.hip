// vp_collect_stream: the kept persons of a call packed into one dense record table, the stage BEHIND vp_infer_boxes_stream, its NMS and the smoother (semantics:
// collectgeom.h), its synchronous host twin vp_collect and the host-only tap vp_dbg_collect_host.  Two kernels: a plan that gives every row its record index from
// ballots and a prefix over waves, then a copy with one wave per row.  No atomics: the table is a pure function of the inputs whatever the launch shape.
#include "api_internal.h"
#include "hoststage.h"
#include "collectgeom.h"

using namespace vpi;

namespace vp {

constexpr int COLLECT_PLAN_THREADS = 1024, COLLECT_PLAN_WAVES = COLLECT_PLAN_THREADS / 64;
constexpr int COLLECT_COPY_THREADS = 256, COLLECT_COPY_ROWS = COLLECT_COPY_THREADS / 64;   // one wave per row

// the handle's workspace (int32): the record index of every row inside its frame (-1: not kept) | the id of every row | the kept rows of every frame
struct CollectWs {
    int32_t *dst, *id, *count;
};
constexpr size_t COLLECT_WS_WORDS = 2 * (size_t)COLLECT_MAX_ROWS + COLLECT_MAX_FRAMES;

// One workgroup per frame f, 16 waves, each on a contiguous segment of the rows (a multiple of 64).  Pass 1: a wave counts the rows of frame f in its segment and the
// kept ones among them (ballots).  The counts of the waves in front, through LDS, are where its segment starts.  Pass 2: the same ballots again, and every row of
// frame f gets its ordinal (the id of a call without ids) and, when kept, its index among the frame's kept rows.  A row of no frame of the table is written by no
// workgroup; the copy kernel tests the frame itself.  One writer per word.
__global__ __launch_bounds__(COLLECT_PLAN_THREADS) void collect_plan_kernel(CollectIn in, CollectWs ws) {
    __shared__ int32_t s_mine[COLLECT_PLAN_WAVES], s_kept[COLLECT_PLAN_WAVES];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = (in.n + COLLECT_PLAN_THREADS - 1) / COLLECT_PLAN_THREADS * 64;
    const int lo = wave * seg, hi = lo + seg < in.n ? lo + seg : in.n;   // uniform per wave
    int cm = 0, ck = 0;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const bool mine = i < hi && collect_frame(in, i) == f, kept = mine && collect_gates(in, i);
        cm += __popcll(__ballot(mine));
        ck += __popcll(__ballot(kept));
    }
    if (lane == 0) { s_mine[wave] = cm; s_kept[wave] = ck; }
    __syncthreads();
    int om = 0, ok = 0, total = 0;
    for (int q = 0; q < COLLECT_PLAN_WAVES; ++q) {
        if (q < wave) { om += s_mine[q]; ok += s_kept[q]; }
        total += s_kept[q];
    }
    const unsigned long long before = (1ull << lane) - 1;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const bool mine = i < hi && collect_frame(in, i) == f, kept = mine && collect_gates(in, i);
        const unsigned long long bm = __ballot(mine), bk = __ballot(kept);
        if (mine) {
            ws.id[i] = in.ids ? in.ids[i] : om + __popcll(bm & before);
            ws.dst[i] = kept ? ok + __popcll(bk & before) : -1;
        }
        om += __popcll(bm);
        ok += __popcll(bk);
    }
    if (tid == 0) ws.count[f] = total;
}

// One wave per row, four rows per workgroup; the LAST workgroup writes the header instead.  A kept row's record index is its index inside its frame plus the kept rows
// of the frames in front (a wave sum over at most 63 counts); a record behind max_records is not written.  Lane l writes the 16-byte granules l, l + 64, ... of
// the record with one store each (header and record stride are multiples of 16 bytes, d_out is 16-byte aligned); the keypoint words are read dword by dword, a
// wave's reads covering one contiguous span of the row.
__global__ __launch_bounds__(COLLECT_COPY_THREADS) void collect_copy_kernel(CollectIn in, CollectWs ws, uint32_t* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int hw = collect_header_words(in.n_frames);
    if (blockIdx.x == gridDim.x - 1) {   // uniform
        if (tid < hw) {
            int32_t v = 0;
            if (tid < in.n_frames) v = ws.count[tid];
            else if (tid == in.n_frames)
                for (int q = 0; q < in.n_frames; ++q) v += ws.count[q];
            out[tid] = (uint32_t)v;
        }
        return;
    }
    const int i = blockIdx.x * COLLECT_COPY_ROWS + (tid >> 6);
    if (i >= in.n) return;   // uniform per wave, as every exit below
    const int32_t f = collect_frame(in, i);
    if (!collect_valid(in, f)) return;
    int32_t dst = ws.dst[i];
    if (dst < 0) return;
    int32_t c = lane < f ? ws.count[lane] : 0;
    for (int m = 32; m; m >>= 1) c += __shfl_xor(c, m);
    dst += c;
    if (dst >= in.max_records) return;
    const int32_t id = ws.id[i];
    const int S = collect_record_words(in.K);
    uint4* rec = (uint4*)(out + hw + (size_t)dst * S);
    for (int g = lane; 4 * g < S; g += 64)
        rec[g] = make_uint4(collect_word(in, i, id, f, 4 * g), collect_word(in, i, id, f, 4 * g + 1), collect_word(in, i, id, f, 4 * g + 2),
                            collect_word(in, i, id, f, 4 * g + 3));
}

}  // namespace vp

namespace {

// every refusal of the three entries (HOST ONLY), before anything is enqueued
int collect_args(const void* kpts, int n, int K, int score_stride, int n_frames, int max_records, const void* out, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "collect: " + m; return (int)VP_ERR_INVALID; };
    if (n < 0 || n > VP_COLLECT_MAX_ROWS) return bad("n = " + std::to_string(n) + " rows outside 0.." + std::to_string(VP_COLLECT_MAX_ROWS));
    if (n_frames < 1 || n_frames > VP_COLLECT_MAX_FRAMES) return bad("n_frames = " + std::to_string(n_frames) + " outside 1.." + std::to_string(VP_COLLECT_MAX_FRAMES));
    if (K < 1 || K > vp::COLLECT_MAX_K) return bad("k = " + std::to_string(K) + " joints outside 1.." + std::to_string(vp::COLLECT_MAX_K));
    if (max_records < 0) return bad("negative max_records");
    if (n > 0 && !kpts) return bad("null keypoints with n > 0");
    if (!out) return bad("null output");
    if (score_stride < 1) return bad("a score stride < 1");
    if ((uintptr_t)out % 16) return bad("the output is not 16-byte aligned");
    return VP_OK;
}

vp::CollectIn collect_in(const float* kpts, int n, int K, const int32_t* ids, const int32_t* frame, const int32_t* rank, const int32_t* status, const float* score,
                         int score_stride, const int32_t* crop_params, int n_frames, int max_records) {
    return vp::CollectIn{(const uint32_t*)kpts, ids, frame, rank, status, (const uint32_t*)score, crop_params, n, K, n_frames, max_records, (int64_t)score_stride};
}

// the checked call on stream s, launches only
int collect_enqueue(vp_ctx* c, const vp::CollectIn& in, void* d_out, hipStream_t s) {
    int32_t* w = (int32_t*)c->collect_ws;
    const vp::CollectWs ws{w, w + vp::COLLECT_MAX_ROWS, w + 2 * vp::COLLECT_MAX_ROWS};
    hipLaunchKernelGGL(vp::collect_plan_kernel, dim3(in.n_frames), dim3(vp::COLLECT_PLAN_THREADS), 0, s, in, ws);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(vp::collect_copy_kernel, dim3((in.n + vp::COLLECT_COPY_ROWS - 1) / vp::COLLECT_COPY_ROWS + 1), dim3(vp::COLLECT_COPY_THREADS), 0, s, in, ws,
                       (uint32_t*)d_out);
    HIPCHK(c, hipGetLastError());
    return VP_OK;
}

// collectgeom.h on host memory, rows in order
void collect_host(const vp::CollectIn& in, uint32_t* out) {
    const int hw = vp::collect_header_words(in.n_frames), S = vp::collect_record_words(in.K);
    std::vector<int32_t> count((size_t)in.n_frames, 0), seen((size_t)in.n_frames, 0), at((size_t)in.n_frames, 0);
    for (int i = 0; i < in.n; ++i) {
        const int32_t f = vp::collect_frame(in, i);
        if (vp::collect_valid(in, f) && vp::collect_gates(in, i)) ++count[f];
    }
    int32_t total = 0;
    for (int f = 0; f < in.n_frames; ++f) { at[f] = total; total += count[f]; }
    for (int q = 0; q < hw; ++q) out[q] = q < in.n_frames ? (uint32_t)count[q] : (q == in.n_frames ? (uint32_t)total : 0u);
    for (int i = 0; i < in.n; ++i) {
        const int32_t f = vp::collect_frame(in, i);
        if (!vp::collect_valid(in, f)) continue;
        const int32_t id = in.ids ? in.ids[i] : seen[f];
        ++seen[f];
        if (!vp::collect_gates(in, i)) continue;
        const int32_t dst = at[f]++;
        if (dst >= in.max_records) continue;
        uint32_t* rec = out + hw + (size_t)dst * S;
        for (int w = 0; w < S; ++w) rec[w] = vp::collect_word(in, i, id, f, w);
    }
}

}  // namespace

extern "C" {

int64_t vp_collect_bytes(int32_t n_frames, int32_t k, int32_t max_records) {
    if (n_frames < 1 || n_frames > VP_COLLECT_MAX_FRAMES || k < 1 || k > vp::COLLECT_MAX_K || max_records < 0) return -1;
    return vp::collect_bytes(n_frames, k, max_records);
}

int vp_collect_stream(vp_handle c, const float* d_kpts, int32_t n, int32_t k, const int32_t* d_ids, const int32_t* d_frame, const int32_t* d_rank,
                      const int32_t* d_status, const float* d_score, int32_t score_stride, const int32_t* d_crop_params, int32_t n_frames, int32_t max_records,
                      void* d_out, void* caller_stream) {
    if (!c) return VP_ERR_INVALID;
    std::string why;
    if (collect_args(d_kpts, n, k, score_stride, n_frames, max_records, d_out, &why)) return fail(c, VP_ERR_INVALID, why);
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    return collect_enqueue(c, collect_in(d_kpts, n, k, d_ids, d_frame, d_rank, d_status, d_score, score_stride, d_crop_params, n_frames, max_records), d_out,
                           (hipStream_t)caller_stream);
}

int vp_collect(vp_handle c, const float* kpts, int32_t n, int32_t k, const int32_t* ids, const int32_t* frame, const int32_t* rank, const int32_t* status,
               const float* score, int32_t score_stride, const int32_t* crop_params, int32_t n_frames, int32_t max_records, void* out) {
    if (!c) return VP_ERR_INVALID;
    std::string why;
    if (collect_args(kpts, n, k, score_stride, n_frames, max_records, out, &why)) return fail(c, VP_ERR_INVALID, why);
    // one scratch block: the table | keypoints | ids | frame | rank | status | score | crop params
    HostStage st(c);
    const size_t nb = (size_t)n * 4, sc_bytes = score && n > 0 ? ((size_t)(n - 1) * score_stride + 1) * 4 : 0;
    const size_t o_out = st.part((size_t)vp::collect_bytes(n_frames, k, max_records));
    const void* src[7] = {kpts, ids, frame, rank, status, score, crop_params};
    const size_t bytes[7] = {(size_t)n * 3 * k * 4, nb, nb, nb, nb, sc_bytes, (size_t)n * 9 * 4};
    const char* what[7] = {"upload keypoints", "upload ids", "upload frame", "upload rank", "upload status", "upload score", "upload crop params"};
    size_t off[7];
    for (int i = 0; i < 7; ++i) off[i] = st.part(bytes[i]);
    if (st.alloc()) return st.rc;
    const void* dev[7];   // an absent input stays null; an empty one has an address and no copy
    for (int i = 0; i < 7; ++i) {
        dev[i] = src[i] ? st.at(off[i]) : nullptr;
        if (src[i] && bytes[i]) st.up(st.at(off[i]), src[i], bytes[i], what[i]);
    }
    char* d = st.at(o_out);
    if (!st.rc)
        st.rc = collect_enqueue(c, collect_in((const float*)dev[0], n, k, (const int32_t*)dev[1], (const int32_t*)dev[2], (const int32_t*)dev[3], (const int32_t*)dev[4],
                                              (const float*)dev[5], score_stride, (const int32_t*)dev[6], n_frames, max_records), d, st.s);
    // the header first: its total says how many records were written, and no byte behind them is touched on the host either
    const size_t hb = (size_t)vp::collect_header_words(n_frames) * 4;
    if (!st.rc) st.down(out, d, hb, "download header");
    st.sync();
    if (!st.rc) {
        const int32_t total = ((const int32_t*)out)[n_frames], m = total < max_records ? total : max_records;
        if (m > 0) {
            st.down((char*)out + hb, d + hb, (size_t)m * vp::collect_record_words(k) * 4, "download records");
            st.sync();
        }
    }
    return st.rc;
}

int vp_dbg_collect_host(const float* kpts, int32_t n, int32_t k, const int32_t* ids, const int32_t* frame, const int32_t* rank, const int32_t* status,
                        const float* score, int32_t score_stride, const int32_t* crop_params, int32_t n_frames, int32_t max_records, void* out) {
    std::string why;
    if (collect_args(kpts, n, k, score_stride, n_frames, max_records, out, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    collect_host(collect_in(kpts, n, k, ids, frame, rank, status, score, score_stride, crop_params, n_frames, max_records), (uint32_t*)out);
    return VP_OK;
}

}  // extern "C"
