// vp_cocoeval_*: COCO keypoint AP / AR as an accumulating, stream-ordered device stage (contract: cocogeom.h), its synchronous host-pointer twins and the host-only
// taps vp_dbg_cocoeval_update_host / vp_dbg_cocoeval_accumulate_host.
//   update:     coco_prep_kernel (per image: the kept count; fills d_match with -2), coco_update_kernel (one workgroup per image: top 20, the OKS matrix in LDS,
//               one lane per (range, threshold) for the greedy walk, records at records + the prefix of the kept counts) and coco_header_kernel (the header words).
//   accumulate: 64-bit keys (score descending, table position), a bitonic network over the live records padded to a power of two (2048 keys per workgroup in LDS,
//               the wider strides in global memory), the sorted flag words, per-chunk tp / fp counts, their prefix, one workgroup per (chunk of 1024, range x
//               threshold) for precision, its envelope inside the chunk and the recall crossings, and one workgroup per (range, threshold) for the 101 values.
// No atomics, no flags between workgroups, no synchronisation, no allocation in a call; the launch sequence depends on the configuration only, so a call captures
// as one linear chain.
#include "api_internal.h"
#include "hoststage.h"
#include "stageobj.h"
#include "cocogeom.h"

using namespace vpi;

namespace vp {

constexpr int CE_THREADS = 256, CE_WAVES = CE_THREADS / 64, CE_ROW_SLOTS = COCO_MAX_ROWS / CE_THREADS;   // 32 rows per thread at most
constexpr int CE_SORT_LOCAL = 2048;                       // keys one workgroup sorts in LDS
constexpr int CE_CHUNK = 1024, CE_PER_THREAD = CE_CHUNK / CE_THREADS;   // positions per chunk of the scans
static_assert(COCO_MAX_FRAMES <= CE_THREADS && COCO_IMG_GTS + COCO_MAX_DETS <= CE_THREADS && COCO_AT <= 64, "one thread per frame / gt + detection / (range, threshold)");

// what one image adds to the header (32 bytes)
struct CocoImg {
    int32_t kept, gts, gt_overflow, nonfinite, npig[COCO_AREAS], pad;
};

struct CocoWs {
    int32_t* kept;       // [COCO_MAX_FRAMES] of a call
    CocoImg* img;        // [COCO_MAX_FRAMES]
    uint64_t* keys;      // [pcap]
    uint2* flags;        // [max_records] (matched, ignored) in sorted order
    int32_t* partial;    // [chunks][COCO_AT][2] tp, fp of a chunk, then their exclusive prefix
    double* chunkmax;    // [COCO_AT][chunks]
    int32_t* idx;        // [COCO_AT][COCO_RECS] the first position with rc >= thr, -1 none
    double* pin;         // [COCO_AT][COCO_RECS] the envelope at that position inside its chunk
    double* lastrc;      // [COCO_AT]
    int32_t chunks, pcap;
};

__device__ inline int ce_block_sum(int v, int* s4) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

// One workgroup per image b: kept[b] = min(20, the counted rows of the image); the workgroups share the -2 fill of d_match.
__global__ __launch_bounds__(CE_THREADS) void coco_prep_kernel(int n, int n_frames, const int32_t* __restrict__ frame, const int32_t* __restrict__ rank, CocoWs ws,
                                                                int32_t* __restrict__ d_match) {
    __shared__ int s4[CE_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    int cnt = 0;
    for (int i = tid; i < n; i += CE_THREADS) {
        int f;
        cnt += coco_counted(rank, frame, i, n_frames, f) && f == b;
    }
    cnt = ce_block_sum(cnt, s4);
    if (tid == 0) ws.kept[b] = cnt < COCO_MAX_DETS ? cnt : COCO_MAX_DETS;
    if (d_match) {
        const int total = n * COCO_THRS, per = (total + n_frames - 1) / n_frames;
        const int lo = b * per, hi = lo + per < total ? lo + per : total;
        for (int i = lo + tid; i < hi; i += CE_THREADS) d_match[i] = -2;
    }
}

__global__ __launch_bounds__(CE_THREADS) void coco_update_kernel(int K, int n, int g, int n_frames, const float* __restrict__ kpts, const float* __restrict__ score,
                                                                  const int32_t* __restrict__ frame, const int32_t* __restrict__ rank, const float* __restrict__ gt_kpts,
                                                                  const float* __restrict__ gt_box, const float* __restrict__ gt_area, const int32_t* __restrict__ gt_flags,
                                                                  const int32_t* __restrict__ gt_frame, const double* __restrict__ vars, CocoWs ws, char* __restrict__ state,
                                                                  int max_records, int32_t* __restrict__ d_match) {
    __shared__ double s_oks[COCO_MAX_DETS][COCO_IMG_GTS];
    __shared__ double s_garea[COCO_IMG_GTS], s_darea[COCO_MAX_DETS];
    __shared__ int s_grow[COCO_IMG_GTS], s_gk1[COCO_IMG_GTS], s_drow[COCO_MAX_DETS];
    __shared__ uint8_t s_crowd[COCO_IMG_GTS], s_ign[COCO_AREAS][COCO_IMG_GTS], s_order[COCO_AREAS][COCO_IMG_GTS];
    __shared__ float s_wkey[CE_WAVES];
    __shared__ int s_wrow[CE_WAVES], s4[CE_WAVES], s_G, s_gtotal, s_npig[COCO_AREAS];
    __shared__ uint32_t s_lane_m[COCO_AT], s_lane_i[COCO_AT];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- stage 1: the first 20 of the image's rows in (key descending, row ascending) order.  Thread tid holds rows tid, tid + 256, ... in registers.
    float key[CE_ROW_SLOTS];
    uint32_t valid = 0;
#pragma unroll
    for (int c = 0; c < CE_ROW_SLOTS; ++c) {
        const int i = c * CE_THREADS + tid;
        int f = 0;
        const bool ok = i < n && coco_counted(rank, frame, i, n_frames, f) && f == b;
        const float s = ok ? score[i] : 0.0f;
        key[c] = s != s ? -INFINITY : s;
        if (ok) valid |= 1u << c;
    }
    int D = 0;
    for (int r = 0; r < COCO_MAX_DETS; ++r) {
        float bk = -INFINITY;
        int br = INT32_MAX;
#pragma unroll
        for (int c = 0; c < CE_ROW_SLOTS; ++c)
            if (((valid >> c) & 1) && (br == INT32_MAX || key[c] > bk)) { bk = key[c]; br = c * CE_THREADS + tid; }   // rows ascend with c: a tie stays with the lower
#pragma unroll
        for (int d = 1; d < 64; d *= 2) {
            const float ok_ = __shfl_xor(bk, d, 64);
            const int or_ = __shfl_xor(br, d, 64);
            if (nms_before((double)ok_, or_, (double)bk, br)) { bk = ok_; br = or_; }
        }
        if (lane == 0) { s_wkey[wave] = bk; s_wrow[wave] = br; }
        __syncthreads();
        bk = s_wkey[0]; br = s_wrow[0];
#pragma unroll
        for (int w = 1; w < CE_WAVES; ++w)
            if (nms_before((double)s_wkey[w], s_wrow[w], (double)bk, br)) { bk = s_wkey[w]; br = s_wrow[w]; }
        __syncthreads();
        if (br == INT32_MAX) break;   // the same for every thread
        if (tid == 0) s_drow[r] = br;
        if ((br & (CE_THREADS - 1)) == tid) valid &= ~(1u << (br / CE_THREADS));
        D = r + 1;
    }

    // ---- the image's gts in call order (wave 0), the first 128 used
    if (wave == 0) {
        int cnt = 0;
        for (int base = 0; base < g; base += 64) {
            const int j = base + lane;
            const bool ok = j < g && coco_gt_frame(gt_frame, j) == b;
            const uint64_t mask = __ballot(ok);
            const int pos = cnt + __popcll(mask & ((1ull << lane) - 1));
            if (ok && pos < COCO_IMG_GTS) s_grow[pos] = j;
            cnt += __popcll(mask);
        }
        if (lane == 0) { s_G = cnt < COCO_IMG_GTS ? cnt : COCO_IMG_GTS; s_gtotal = cnt; }
    }
    __syncthreads();
    const int G = s_G;
    if (tid < G) {
        const int j = s_grow[tid];
        const int k1 = coco_k1(gt_kpts + (size_t)j * 3 * K, K);
        const double area = (double)gt_area[j];
        const bool crowd = gt_flags ? (gt_flags[j] & 1) != 0 : false;
        s_gk1[tid] = k1;
        s_garea[tid] = area;
        s_crowd[tid] = crowd;
#pragma unroll
        for (int a = 0; a < COCO_AREAS; ++a) s_ign[a][tid] = crowd || k1 == 0 || coco_outside(area, a);
    } else if (tid >= COCO_IMG_GTS && tid - COCO_IMG_GTS < D) {
        s_darea[tid - COCO_IMG_GTS] = coco_det_area(kpts + (size_t)s_drow[tid - COCO_IMG_GTS] * 3 * K, K);
    }
    __syncthreads();
    if (tid < COCO_AREAS) {   // the stable order, not-ignored first
        int p = 0;
        for (int q = 0; q < G; ++q)
            if (!s_ign[tid][q]) s_order[tid][p++] = (uint8_t)q;
        s_npig[tid] = p;
        for (int q = 0; q < G; ++q)
            if (s_ign[tid][q]) s_order[tid][p++] = (uint8_t)q;
    }

    // ---- stage 2: the OKS matrix, one pair per thread and round, the joint terms in joint order
    int nonfin = 0;
    for (int p = tid; p < D * G; p += CE_THREADS) {
        const int d = p / G, q = p - d * G, j = s_grow[q];
        double o = coco_oks(kpts + (size_t)s_drow[d] * 3 * K, gt_kpts + (size_t)j * 3 * K, gt_box + (size_t)j * 4, s_garea[q], s_gk1[q], K, vars);
        if (!coco_finite(o)) { ++nonfin; o = -1.0; }
        s_oks[d][q] = o;
    }
    nonfin = ce_block_sum(nonfin, s4);   // its barriers publish s_oks and s_order

    // ---- stage 3: one lane per (range, threshold)
    if (tid < COCO_AT) {
        const int a = tid / COCO_THRS, t = tid - a * COCO_THRS;
        uint32_t mbits = 0, ibits = 0;
        coco_walk(D, G, coco_oks_thr(t), [&](int d, int j) { return s_oks[d][j]; }, s_order[a], s_ign[a], s_crowd, [&](int d, int m) {
            if (m > -1) mbits |= 1u << d;
            if (m > -1 ? s_ign[a][m] != 0 : coco_outside(s_darea[d], a)) ibits |= 1u << d;
            if (a == 0 && d_match) d_match[(size_t)s_drow[d] * COCO_THRS + t] = m > -1 ? s_grow[m] : -1;
        });
        s_lane_m[tid] = mbits;
        s_lane_i[tid] = ibits;
    }

    // ---- stage 4: the records, at records + the kept counts of the images before this one
    const int before = ce_block_sum(tid < b ? ws.kept[tid] : 0, s4);   // its barriers publish s_lane_*
    const int64_t* W = (const int64_t*)state;
    if (tid < D) {
        uint32_t m = 0, ig = 0;
#pragma unroll
        for (int l = 0; l < COCO_AT; ++l) {
            m |= ((s_lane_m[l] >> tid) & 1u) << l;
            ig |= ((s_lane_i[l] >> tid) & 1u) << l;
        }
        const int64_t pos = W[COCO_W_RECORDS] + before + tid;
        if (pos < max_records) {
            CocoRecord r;
            r.score = score[s_drow[tid]];
            r.matched = m;
            r.ignored = ig;
            r.image = (uint32_t)(W[COCO_W_IMAGES] + b);
            ((CocoRecord*)(state + COCO_HDR_WORDS * 8))[pos] = r;
        }
    }
    if (tid == 0) {
        CocoImg im;
        im.kept = D;
        im.gts = G;
        im.gt_overflow = s_gtotal - G;
        im.nonfinite = nonfin;
        for (int a = 0; a < COCO_AREAS; ++a) im.npig[a] = s_npig[a];
        im.pad = 0;
        ws.img[b] = im;
    }
}

// One workgroup: thread f adds word f of the images' partials in image order into the header.
__global__ __launch_bounds__(64) void coco_header_kernel(int n, int n_frames, int max_records, CocoWs ws, char* __restrict__ state) {
    int64_t* W = (int64_t*)state;
    const int f = threadIdx.x;
    if (f >= 7) return;
    int64_t s = 0;
    for (int b = 0; b < n_frames; ++b) s += ((const int32_t*)&ws.img[b])[f];
    if (f == 0) {
        const int64_t room = (int64_t)max_records - W[COCO_W_RECORDS], w = s < room ? s : room;
        W[COCO_W_CALLS] += 1;
        W[COCO_W_IMAGES] += n_frames;
        W[COCO_W_ROWS] += n;
        W[COCO_W_KEPT] += s;
        W[COCO_W_RECORDS] += w;
        W[COCO_W_DROPPED] += s - w;
    } else if (f == 1) {
        W[COCO_W_GTS] += s;
    } else if (f == 2) {
        W[COCO_W_GT_OVERFLOW] += s;
    } else if (f == 3) {
        W[COCO_W_NONFINITE] += s;
    } else {
        W[COCO_W_NPIG + (f - 4)] += s;
    }
}

// ---------------------------------------------------------------- accumulate

__device__ inline int ce_live(const char* state) { return (int)((const int64_t*)state)[COCO_W_RECORDS]; }
// the size of the sort network: the power of two >= the live records, at least one workgroup's keys
__device__ inline int ce_pow2(int R) {
    int P = CE_SORT_LOCAL;
    while (P < R) P <<= 1;
    return P;
}

__global__ __launch_bounds__(CE_THREADS) void coco_keys_kernel(const char* __restrict__ state, CocoWs ws) {
    const int R = ce_live(state), P = ce_pow2(R);
    const int i = blockIdx.x * CE_THREADS + threadIdx.x;
    if (i >= P || i >= ws.pcap) return;
    const CocoRecord* rec = (const CocoRecord*)(state + COCO_HDR_WORDS * 8);
    ws.keys[i] = i < R ? coco_sort_key(rec[i].score, (uint32_t)i) : ~0ull;
    if (blockIdx.x == 0)
        for (int q = threadIdx.x; q < COCO_AT * COCO_RECS; q += CE_THREADS) ws.idx[q] = -1;
}

// compare-exchange steps j = j_hi .. 1 of merge size k on the 2048 keys of this workgroup in LDS; gbase = the global index of its first key
__device__ inline void ce_lds_steps(uint64_t* s, int k, int j_hi, int gbase) {
    for (int j = j_hi; j > 0; j >>= 1) {
#pragma unroll
        for (int q = 0; q < CE_SORT_LOCAL / 2 / CE_THREADS; ++q) {
            const int p = q * CE_THREADS + threadIdx.x;
            const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), o = i | j;
            const bool up = ((gbase + i) & k) == 0;
            const uint64_t x = s[i], y = s[o];
            if ((x > y) == up) { s[i] = y; s[o] = x; }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(CE_THREADS) void coco_sort_local_kernel(const char* __restrict__ state, CocoWs ws) {
    __shared__ uint64_t s[CE_SORT_LOCAL];
    const int P = ce_pow2(ce_live(state)), gbase = blockIdx.x * CE_SORT_LOCAL;
    if (gbase >= P) return;
    for (int q = threadIdx.x; q < CE_SORT_LOCAL; q += CE_THREADS) s[q] = ws.keys[gbase + q];
    __syncthreads();
    for (int k = 2; k <= CE_SORT_LOCAL; k <<= 1) ce_lds_steps(s, k, k >> 1, gbase);
    for (int q = threadIdx.x; q < CE_SORT_LOCAL; q += CE_THREADS) ws.keys[gbase + q] = s[q];
}

__global__ __launch_bounds__(CE_THREADS) void coco_sort_global_kernel(const char* __restrict__ state, CocoWs ws, int k, int j) {
    const int P = ce_pow2(ce_live(state));
    const int p = blockIdx.x * CE_THREADS + threadIdx.x;
    if (k > P || p >= P / 2) return;
    const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), o = i | j;
    const bool up = (i & k) == 0;
    const uint64_t x = ws.keys[i], y = ws.keys[o];
    if ((x > y) == up) { ws.keys[i] = y; ws.keys[o] = x; }
}

__global__ __launch_bounds__(CE_THREADS) void coco_sort_merge_kernel(const char* __restrict__ state, CocoWs ws, int k) {
    __shared__ uint64_t s[CE_SORT_LOCAL];
    const int P = ce_pow2(ce_live(state)), gbase = blockIdx.x * CE_SORT_LOCAL;
    if (k > P || gbase >= P) return;
    for (int q = threadIdx.x; q < CE_SORT_LOCAL; q += CE_THREADS) s[q] = ws.keys[gbase + q];
    __syncthreads();
    ce_lds_steps(s, k, CE_SORT_LOCAL >> 1, gbase);
    for (int q = threadIdx.x; q < CE_SORT_LOCAL; q += CE_THREADS) ws.keys[gbase + q] = s[q];
}

__global__ __launch_bounds__(CE_THREADS) void coco_gather_kernel(const char* __restrict__ state, CocoWs ws) {
    const int R = ce_live(state), i = blockIdx.x * CE_THREADS + threadIdx.x;
    if (i >= R) return;
    const CocoRecord* rec = (const CocoRecord*)(state + COCO_HDR_WORDS * 8);
    const uint32_t pos = (uint32_t)ws.keys[i];
    ws.flags[i] = make_uint2(rec[pos].matched, rec[pos].ignored);
}

// the tp / fp bits of sorted position i
__device__ inline void ce_bits(const CocoWs& ws, int i, int R, uint32_t& tp, uint32_t& fp) {
    tp = fp = 0;
    if (i < R) {
        const uint2 f = ws.flags[i];
        tp = f.x & ~f.y;
        fp = ~f.x & ~f.y & ((1u << COCO_AT) - 1);
    }
}

// One workgroup per chunk of 1024 sorted positions: the tp and fp counts of the chunk for each (range, threshold).
__global__ __launch_bounds__(CE_THREADS) void coco_chunk_counts_kernel(const char* __restrict__ state, CocoWs ws) {
    __shared__ int s_cnt[CE_WAVES][2 * COCO_AT];
    const int R = ce_live(state), c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (c * CE_CHUNK >= R) return;
    int mine = 0;   // lane x of a wave keeps count x: 2 (10 a + t) + (0 tp, 1 fp)
    for (int q = 0; q < CE_PER_THREAD; ++q) {
        uint32_t tp, fp;
        ce_bits(ws, c * CE_CHUNK + q * CE_THREADS + tid, R, tp, fp);
#pragma unroll
        for (int bit = 0; bit < COCO_AT; ++bit) {
            const int ct = __popcll(__ballot((tp >> bit) & 1)), cf = __popcll(__ballot((fp >> bit) & 1));
            if (lane == 2 * bit) mine += ct;
            if (lane == 2 * bit + 1) mine += cf;
        }
    }
    if (lane < 2 * COCO_AT) s_cnt[wave][lane] = mine;
    __syncthreads();
    if (tid < 2 * COCO_AT) ws.partial[(size_t)c * 2 * COCO_AT + tid] = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
}

// One workgroup: thread x turns count x of the chunks into its exclusive prefix over the chunks.
__global__ __launch_bounds__(64) void coco_chunk_prefix_kernel(const char* __restrict__ state, CocoWs ws) {
    const int R = ce_live(state), C = (R + CE_CHUNK - 1) / CE_CHUNK, x = threadIdx.x;
    if (x >= 2 * COCO_AT) return;
    int run = 0;
    for (int c = 0; c < C; ++c) {
        const int v = ws.partial[(size_t)c * 2 * COCO_AT + x];
        ws.partial[(size_t)c * 2 * COCO_AT + x] = run;
        run += v;
    }
}

// One workgroup per (chunk, range x threshold); thread tid holds positions 4 tid .. 4 tid + 3 of the chunk.  Cumulative tp / fp, the precision, its envelope inside
// the chunk, and at every position where the recall steps over recall thresholds: idx and the envelope there.  Each (range, threshold, k) has one writer.
__global__ __launch_bounds__(CE_THREADS) void coco_scan_kernel(const char* __restrict__ state, CocoWs ws) {
    __shared__ int s_w[CE_WAVES];
    __shared__ double s_max[CE_THREADS];
    const int R = ce_live(state), c = blockIdx.x, at = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t npig = ((const int64_t*)state)[COCO_W_NPIG + at / COCO_THRS];
    if (c * CE_CHUNK >= R || npig == 0) return;
    const int i0 = c * CE_CHUNK + tid * CE_PER_THREAD;
    int tb[CE_PER_THREAD], fb[CE_PER_THREAD], st = 0, sf = 0;
#pragma unroll
    for (int q = 0; q < CE_PER_THREAD; ++q) {
        uint32_t tp, fp;
        ce_bits(ws, i0 + q, R, tp, fp);
        tb[q] = (tp >> at) & 1;
        fb[q] = (fp >> at) & 1;
        st += tb[q];
        sf += fb[q];
    }
    // exclusive prefix over the threads of (tp, fp) packed as tp | fp << 16 (each at most 1024)
    const int mine = st | (sf << 16);
    int inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int ex = inc - mine;
    for (int w = 0; w < wave; ++w) ex += s_w[w];
    int64_t tp = ws.partial[(size_t)c * 2 * COCO_AT + 2 * at] + (ex & 0xffff), fp = ws.partial[(size_t)c * 2 * COCO_AT + 2 * at + 1] + (ex >> 16);
    double pr[CE_PER_THREAD], rc[CE_PER_THREAD];
#pragma unroll
    for (int q = 0; q < CE_PER_THREAD; ++q) {
        tp += tb[q];
        fp += fb[q];
        const bool in = i0 + q < R;
        pr[q] = in ? coco_precision(tp, fp) : -1.0;   // below every precision
        rc[q] = coco_recall(tp, npig);
    }
    // the envelope from the back, inside the chunk
#pragma unroll
    for (int q = CE_PER_THREAD - 2; q >= 0; --q) pr[q] = pr[q] > pr[q + 1] ? pr[q] : pr[q + 1];
    s_max[tid] = pr[0];
    __syncthreads();
    for (int off = 1; off < CE_THREADS; off <<= 1) {
        const double o = tid + off < CE_THREADS ? s_max[tid + off] : -1.0;
        __syncthreads();
        if (o > s_max[tid]) s_max[tid] = o;
        __syncthreads();
    }
    const double after = tid + 1 < CE_THREADS ? s_max[tid + 1] : -1.0;
    if (tid == 0) ws.chunkmax[(size_t)at * ws.chunks + c] = s_max[0];
    tp -= st;   // back to the count before this thread's first position
#pragma unroll
    for (int q = 0; q < CE_PER_THREAD; ++q) {
        const int i = i0 + q;
        tp += tb[q];
        if (i >= R) break;
        if (i == 0 || tb[q]) {
            const int k_lo = i == 0 ? 0 : coco_first_thr_above(coco_recall(tp - 1, npig));
            const double env = pr[q] > after ? pr[q] : after;
            for (int k = k_lo; k < COCO_RECS && coco_rec_thr(k) <= rc[q]; ++k) {
                ws.idx[at * COCO_RECS + k] = i;
                ws.pin[at * COCO_RECS + k] = env;
            }
        }
        if (i == R - 1) ws.lastrc[at] = rc[q];
    }
}

// One workgroup per (range, threshold): the envelope over the chunks behind a crossing's chunk, and the 101 precisions and the recall; workgroup 0 copies the header.
__global__ __launch_bounds__(CE_THREADS) void coco_final_kernel(const char* __restrict__ state, CocoWs ws, char* __restrict__ out) {
    __shared__ double s_cm[COCO_MAX_RECORDS / CE_CHUNK];
    const int R = ce_live(state), C = (R + CE_CHUNK - 1) / CE_CHUNK, at = blockIdx.x, tid = threadIdx.x;
    const int64_t* W = (const int64_t*)state;
    const int64_t npig = W[COCO_W_NPIG + at / COCO_THRS];
    double* res = (double*)(out + COCO_HDR_WORDS * 8);
    if (at == 0 && tid < COCO_HDR_WORDS) ((int64_t*)out)[tid] = W[tid];
    if (npig == 0 || R == 0) {   // the same for every thread
        const double v = npig == 0 ? -1.0 : 0.0;
        if (tid < COCO_RECS) res[at * COCO_RECS + tid] = v;
        if (tid == COCO_RECS) res[COCO_AT * COCO_RECS + at] = v;
        return;
    }
    for (int c = tid; c < C; c += CE_THREADS) s_cm[c] = ws.chunkmax[(size_t)at * ws.chunks + c];
    __syncthreads();
    if (tid == 0)
        for (int c = C - 2; c >= 0; --c) s_cm[c] = s_cm[c] > s_cm[c + 1] ? s_cm[c] : s_cm[c + 1];
    __syncthreads();
    if (tid < COCO_RECS) {
        const int ix = ws.idx[at * COCO_RECS + tid];
        double v = 0.0;
        if (ix >= 0) {
            v = ws.pin[at * COCO_RECS + tid];
            const int c = ix / CE_CHUNK;
            if (c + 1 < C && s_cm[c + 1] > v) v = s_cm[c + 1];
        }
        res[at * COCO_RECS + tid] = v;
    }
    if (tid == COCO_RECS) res[COCO_AT * COCO_RECS + at] = ws.lastrc[at];
}

}  // namespace vp

struct vp_cocoeval : StageObj {
    int K = 0, max_records = 0;
    char* state = nullptr;   // device, one allocation: state | vars double [K] | the workspace (CocoWs)
    double* vars = nullptr;
    vp::CocoWs ws{};
    size_t state_bytes = 0;
};

namespace {

struct UpdateArgs {
    const float *kpts, *score;
    const int32_t *frame, *rank;
    int n;
    const float *gt_kpts, *gt_box, *gt_area;
    const int32_t *gt_flags, *gt_frame;
    int g, n_frames;
    int32_t* match;
};

// ---- the host model of an update: cocogeom.h run serially, image by image (HOST ONLY)
void update_host(char* state, int K, int max_records, const double* vars, const UpdateArgs& u) {
    using namespace vp;
    int64_t* W = (int64_t*)state;
    CocoRecord* table = (CocoRecord*)(state + COCO_HDR_WORDS * 8);
    if (u.match)
        for (size_t i = 0; i < (size_t)u.n * COCO_THRS; ++i) u.match[i] = -2;
    const int64_t images0 = W[COCO_W_IMAGES];
    int64_t kept = 0, written = 0, gts = 0, overflow = 0, nonfinite = 0, npig[COCO_AREAS] = {0, 0, 0};
    std::vector<int> rows, grow;
    std::vector<double> oks((size_t)COCO_MAX_DETS * COCO_IMG_GTS), garea(COCO_IMG_GTS);
    std::vector<uint8_t> crowd(COCO_IMG_GTS), ign((size_t)COCO_AREAS * COCO_IMG_GTS), order((size_t)COCO_AREAS * COCO_IMG_GTS);
    std::vector<int> gk1(COCO_IMG_GTS);
    for (int b = 0; b < u.n_frames; ++b) {
        rows.clear();
        grow.clear();
        for (int i = 0; i < u.n; ++i) {
            int f;
            if (coco_counted(u.rank, u.frame, i, u.n_frames, f) && f == b) rows.push_back(i);
        }
        std::stable_sort(rows.begin(), rows.end(), [&](int x, int y) { return nms_before(nms_key((double)u.score[x]), x, nms_key((double)u.score[y]), y); });
        const int D = (int)std::min<size_t>(rows.size(), COCO_MAX_DETS);
        int total = 0;
        for (int j = 0; j < u.g; ++j)
            if (coco_gt_frame(u.gt_frame, j) == b) {
                if (total < COCO_IMG_GTS) grow.push_back(j);
                ++total;
            }
        const int G = (int)grow.size();
        for (int q = 0; q < G; ++q) {
            const int j = grow[q];
            gk1[q] = coco_k1(u.gt_kpts + (size_t)j * 3 * K, K);
            garea[q] = (double)u.gt_area[j];
            crowd[q] = u.gt_flags ? (u.gt_flags[j] & 1) != 0 : 0;
            for (int a = 0; a < COCO_AREAS; ++a) ign[(size_t)a * COCO_IMG_GTS + q] = crowd[q] || gk1[q] == 0 || coco_outside(garea[q], a);
        }
        for (int a = 0; a < COCO_AREAS; ++a) {
            uint8_t* o = &order[(size_t)a * COCO_IMG_GTS];
            const uint8_t* ig = &ign[(size_t)a * COCO_IMG_GTS];
            int p = 0;
            for (int q = 0; q < G; ++q)
                if (!ig[q]) o[p++] = (uint8_t)q;
            npig[a] += p;
            for (int q = 0; q < G; ++q)
                if (ig[q]) o[p++] = (uint8_t)q;
        }
        for (int d = 0; d < D; ++d)
            for (int q = 0; q < G; ++q) {
                const int j = grow[q];
                double o = coco_oks(u.kpts + (size_t)rows[d] * 3 * K, u.gt_kpts + (size_t)j * 3 * K, u.gt_box + (size_t)j * 4, garea[q], gk1[q], K, vars);
                if (!coco_finite(o)) { ++nonfinite; o = -1.0; }
                oks[(size_t)d * COCO_IMG_GTS + q] = o;
            }
        uint32_t matched[COCO_MAX_DETS] = {0}, ignored[COCO_MAX_DETS] = {0};
        for (int a = 0; a < COCO_AREAS; ++a)
            for (int t = 0; t < COCO_THRS; ++t) {
                const uint8_t* ig = &ign[(size_t)a * COCO_IMG_GTS];
                coco_walk(D, G, coco_oks_thr(t), [&](int d, int j) { return oks[(size_t)d * COCO_IMG_GTS + j]; }, &order[(size_t)a * COCO_IMG_GTS], ig, crowd.data(),
                          [&](int d, int m) {
                              const uint32_t bit = 1u << (COCO_THRS * a + t);
                              if (m > -1) matched[d] |= bit;
                              if (m > -1 ? ig[m] != 0 : coco_outside(coco_det_area(u.kpts + (size_t)rows[d] * 3 * K, K), a)) ignored[d] |= bit;
                              if (a == 0 && u.match) u.match[(size_t)rows[d] * COCO_THRS + t] = m > -1 ? grow[m] : -1;
                          });
            }
        for (int d = 0; d < D; ++d) {
            const int64_t pos = W[COCO_W_RECORDS] + kept + d;
            if (pos < max_records) {
                CocoRecord r;
                r.score = u.score[rows[d]];
                r.matched = matched[d];
                r.ignored = ignored[d];
                r.image = (uint32_t)(images0 + b);
                table[pos] = r;
                ++written;
            }
        }
        kept += D;
        gts += G;
        overflow += total - G;
    }
    W[COCO_W_CALLS] += 1;
    W[COCO_W_IMAGES] += u.n_frames;
    W[COCO_W_ROWS] += u.n;
    W[COCO_W_KEPT] += kept;
    W[COCO_W_RECORDS] += written;
    W[COCO_W_DROPPED] += kept - written;
    W[COCO_W_GTS] += gts;
    W[COCO_W_GT_OVERFLOW] += overflow;
    W[COCO_W_NONFINITE] += nonfinite;
    for (int a = 0; a < COCO_AREAS; ++a) W[COCO_W_NPIG + a] += npig[a];
}

// ---- the host model of accumulate (HOST ONLY)
void accumulate_host(const char* state, char* out) {
    using namespace vp;
    const int64_t* W = (const int64_t*)state;
    const CocoRecord* table = (const CocoRecord*)(state + COCO_HDR_WORDS * 8);
    memcpy(out, state, COCO_HDR_WORDS * 8);
    double* res = (double*)(out + COCO_HDR_WORDS * 8);
    const int R = (int)W[COCO_W_RECORDS];
    std::vector<uint64_t> keys((size_t)R);
    for (int i = 0; i < R; ++i) keys[i] = coco_sort_key(table[i].score, (uint32_t)i);
    std::sort(keys.begin(), keys.end());
    std::vector<double> pr((size_t)R), rc((size_t)R);
    for (int at = 0; at < COCO_AT; ++at) {
        const int64_t npig = W[COCO_W_NPIG + at / COCO_THRS];
        double* prec = res + (size_t)at * COCO_RECS;
        double& recall = res[COCO_AT * COCO_RECS + at];
        if (npig == 0 || R == 0) {
            const double v = npig == 0 ? -1.0 : 0.0;
            for (int k = 0; k < COCO_RECS; ++k) prec[k] = v;
            recall = v;
            continue;
        }
        int64_t tp = 0, fp = 0;
        for (int i = 0; i < R; ++i) {
            const CocoRecord& r = table[(uint32_t)keys[i]];
            const bool m = (r.matched >> at) & 1, ig = (r.ignored >> at) & 1;
            tp += m && !ig;
            fp += !m && !ig;
            rc[i] = coco_recall(tp, npig);
            pr[i] = coco_precision(tp, fp);
        }
        recall = rc[R - 1];
        for (int i = R - 1; i > 0; --i)
            if (pr[i] > pr[i - 1]) pr[i - 1] = pr[i];
        int i = 0;
        for (int k = 0; k < COCO_RECS; ++k) {
            while (i < R && rc[i] < coco_rec_thr(k)) ++i;
            prec[k] = i < R ? pr[i] : 0.0;
        }
    }
}

int cfg_check(const vp_cocoeval_cfg* cfg, const double* sigmas, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "cocoeval: " + m; return (int)VP_ERR_INVALID; };
    if (!cfg) return bad("null cfg");
    if (cfg->n_joints < 1 || cfg->n_joints > vp::NMS_MAX_K) return bad("n_joints = " + std::to_string(cfg->n_joints) + " outside 1.." + std::to_string(vp::NMS_MAX_K));
    if (cfg->max_records < 1 || cfg->max_records > vp::COCO_MAX_RECORDS)
        return bad("max_records = " + std::to_string(cfg->max_records) + " outside 1.." + std::to_string(vp::COCO_MAX_RECORDS));
    if (!sigmas) return bad("null sigmas");
    for (int j = 0; j < cfg->n_joints; ++j)
        if (!(vp::coco_finite(sigmas[j]) && sigmas[j] > 0.0)) return bad("sigma[" + std::to_string(j) + "] not finite or <= 0");
    return VP_OK;
}

int update_check(const UpdateArgs& u, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "cocoeval: " + m; return (int)VP_ERR_INVALID; };
    if (u.n < 0 || u.n > vp::COCO_MAX_ROWS) return bad("n = " + std::to_string(u.n) + " outside 0.." + std::to_string(vp::COCO_MAX_ROWS));
    if (u.g < 0 || u.g > vp::COCO_MAX_GTS) return bad("g = " + std::to_string(u.g) + " outside 0.." + std::to_string(vp::COCO_MAX_GTS));
    if (u.n_frames < 1 || u.n_frames > vp::COCO_MAX_FRAMES) return bad("n_frames = " + std::to_string(u.n_frames) + " outside 1.." + std::to_string(vp::COCO_MAX_FRAMES));
    if (u.n > 0 && !(u.kpts && u.score)) return bad("null kpts or score with n > 0");
    if (u.g > 0 && !(u.gt_kpts && u.gt_box && u.gt_area)) return bad("null gt_kpts, gt_box or gt_area with g > 0");
    return VP_OK;
}

void host_vars(const double* sigmas, int K, std::vector<double>& vars) {
    vars.resize((size_t)K);
    for (int j = 0; j < K; ++j) { const double s2 = 2.0 * sigmas[j]; vars[j] = s2 * s2; }
}

int update_enqueue(vp_cocoeval* e, const UpdateArgs& u, hipStream_t q) {
    vp_ctx* c = e->c;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    hipLaunchKernelGGL(vp::coco_prep_kernel, dim3(u.n_frames), dim3(vp::CE_THREADS), 0, q, u.n, u.n_frames, u.frame, u.rank, e->ws, u.match);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(vp::coco_update_kernel, dim3(u.n_frames), dim3(vp::CE_THREADS), 0, q, e->K, u.n, u.g, u.n_frames, u.kpts, u.score, u.frame, u.rank, u.gt_kpts, u.gt_box,
                       u.gt_area, u.gt_flags, u.gt_frame, (const double*)e->vars, e->ws, e->state, e->max_records, u.match);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(vp::coco_header_kernel, dim3(1), dim3(64), 0, q, u.n, u.n_frames, e->max_records, e->ws, e->state);
    HIPCHK(c, hipGetLastError());
    return VP_OK;
}

int accumulate_enqueue(vp_cocoeval* e, char* d_out, hipStream_t q) {
    using namespace vp;
    vp_ctx* c = e->c;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const CocoWs& ws = e->ws;
    const char* st = e->state;
    const int T = CE_THREADS;
    hipLaunchKernelGGL(coco_keys_kernel, dim3(ws.pcap / T), dim3(T), 0, q, st, ws);
    hipLaunchKernelGGL(coco_sort_local_kernel, dim3(ws.pcap / CE_SORT_LOCAL), dim3(T), 0, q, st, ws);
    for (int k = 2 * CE_SORT_LOCAL; k <= ws.pcap; k <<= 1) {
        for (int j = k >> 1; j >= CE_SORT_LOCAL; j >>= 1) hipLaunchKernelGGL(coco_sort_global_kernel, dim3(ws.pcap / 2 / T), dim3(T), 0, q, st, ws, k, j);
        hipLaunchKernelGGL(coco_sort_merge_kernel, dim3(ws.pcap / CE_SORT_LOCAL), dim3(T), 0, q, st, ws, k);
    }
    hipLaunchKernelGGL(coco_gather_kernel, dim3((e->max_records + T - 1) / T), dim3(T), 0, q, st, ws);
    hipLaunchKernelGGL(coco_chunk_counts_kernel, dim3(ws.chunks), dim3(T), 0, q, st, ws);
    hipLaunchKernelGGL(coco_chunk_prefix_kernel, dim3(1), dim3(64), 0, q, st, ws);
    hipLaunchKernelGGL(coco_scan_kernel, dim3(ws.chunks, COCO_AT), dim3(T), 0, q, st, ws);
    hipLaunchKernelGGL(coco_final_kernel, dim3(COCO_AT), dim3(T), 0, q, st, ws, d_out);
    HIPCHK(c, hipGetLastError());
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_cocoeval_create(vp_handle c, const vp_cocoeval_cfg* cfg, const double* sigmas, vp_cocoeval_handle* out) {
    return stage_create(c, out, [&](vp_cocoeval*, std::string* why) { return cfg_check(cfg, sigmas, why); },
                        [&](vp_cocoeval* e) {
                            const int K = e->K = cfg->n_joints, M = e->max_records = cfg->max_records;
                            e->state_bytes = vp::coco_state_bytes(M);
                            int pcap = vp::CE_SORT_LOCAL;
                            while (pcap < M) pcap <<= 1;
                            const int chunks = (M + vp::CE_CHUNK - 1) / vp::CE_CHUNK;
                            const size_t AT = vp::COCO_AT, RK = AT * vp::COCO_RECS;
                            const size_t sizes[] = {e->state_bytes, (size_t)K * 8, vp::COCO_MAX_FRAMES * 4, vp::COCO_MAX_FRAMES * sizeof(vp::CocoImg), (size_t)pcap * 8,
                                                    (size_t)M * 8, (size_t)chunks * 2 * AT * 4, AT * chunks * 8, RK * 4, RK * 8, AT * 8};
                            StageLayout lay;
                            size_t off[11];
                            for (int i = 0; i < 11; ++i) off[i] = lay.part(sizes[i]);
                            std::vector<double> vars;
                            host_vars(sigmas, K, vars);
                            char* mem = e->alloc(lay.end, 0);
                            e->up(mem + off[1], vars.data(), (size_t)K * 8);
                            e->state = mem;
                            e->vars = (double*)(mem + off[1]);
                            e->ws.kept = (int32_t*)(mem + off[2]);
                            e->ws.img = (vp::CocoImg*)(mem + off[3]);
                            e->ws.keys = (uint64_t*)(mem + off[4]);
                            e->ws.flags = (uint2*)(mem + off[5]);
                            e->ws.partial = (int32_t*)(mem + off[6]);
                            e->ws.chunkmax = (double*)(mem + off[7]);
                            e->ws.idx = (int32_t*)(mem + off[8]);
                            e->ws.pin = (double*)(mem + off[9]);
                            e->ws.lastrc = (double*)(mem + off[10]);
                            e->ws.chunks = chunks;
                            e->ws.pcap = pcap;
                            return "cocoeval state: ";
                        });
}

int vp_cocoeval_destroy(vp_cocoeval_handle e) { return stage_destroy(e); }

int vp_cocoeval_reset_stream(vp_cocoeval_handle e, void* caller_stream) {
    if (!e) return VP_ERR_INVALID;
    return stage_reset(e, e->state, e->state_bytes, caller_stream);
}

int vp_cocoeval_update_stream(vp_cocoeval_handle e, const float* d_kpts, const float* d_score, const int32_t* d_frame, const int32_t* d_rank, int32_t n, const float* d_gt_kpts,
                              const float* d_gt_box, const float* d_gt_area, const int32_t* d_gt_flags, const int32_t* d_gt_frame, int32_t g, int32_t n_frames, int32_t* d_match,
                              void* caller_stream) {
    if (!e) return VP_ERR_INVALID;
    const UpdateArgs u{d_kpts, d_score, d_frame, d_rank, n, d_gt_kpts, d_gt_box, d_gt_area, d_gt_flags, d_gt_frame, g, n_frames, d_match};
    std::string why;
    if (update_check(u, &why)) return fail(e->c, VP_ERR_INVALID, why);
    return update_enqueue(e, u, (hipStream_t)caller_stream);
}

int vp_cocoeval_update(vp_cocoeval_handle e, const float* kpts, const float* score, const int32_t* frame, const int32_t* rank, int32_t n, const float* gt_kpts, const float* gt_box,
                       const float* gt_area, const int32_t* gt_flags, const int32_t* gt_frame, int32_t g, int32_t n_frames, int32_t* match) {
    if (!e) return VP_ERR_INVALID;
    vp_ctx* c = e->c;
    const UpdateArgs h{kpts, score, frame, rank, n, gt_kpts, gt_box, gt_area, gt_flags, gt_frame, g, n_frames, match};
    std::string why;
    if (update_check(h, &why)) return fail(c, VP_ERR_INVALID, why);
    // one scratch block: kpts | score | frame | rank | gt_kpts | gt_box | gt_area | gt_flags | gt_frame | match
    HostStage st(c);
    const int K = e->K;
    const size_t raw[] = {(size_t)n * K * 12, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)g * K * 12, (size_t)g * 16, (size_t)g * 4, (size_t)g * 4, (size_t)g * 4, (size_t)n * 40};
    const void* src[] = {kpts, score, frame, rank, gt_kpts, gt_box, gt_area, gt_flags, gt_frame, nullptr};
    size_t off[10];
    for (int i = 0; i < 10; ++i) off[i] = st.part(raw[i]);
    if (st.alloc()) return st.rc;
    void* dev[10];
    for (int i = 0; i < 10; ++i) {
        const bool given = raw[i] > 0 && (i == 9 ? match != nullptr : src[i] != nullptr);
        dev[i] = given ? st.at(off[i]) : nullptr;
        if (given && i < 9) st.up(dev[i], src[i], raw[i], "cocoeval upload");
    }
    if (!st.rc) {
        const UpdateArgs u{(const float*)dev[0], (const float*)dev[1], (const int32_t*)dev[2], (const int32_t*)dev[3], n, (const float*)dev[4], (const float*)dev[5],
                           (const float*)dev[6], (const int32_t*)dev[7], (const int32_t*)dev[8], g, n_frames, (int32_t*)dev[9]};
        st.rc = update_enqueue(e, u, st.s);
    }
    if (!st.rc && dev[9]) st.down(match, dev[9], raw[9], "cocoeval download match");
    st.sync();
    return st.rc;
}

int vp_cocoeval_accumulate_stream(vp_cocoeval_handle e, void* d_out, void* caller_stream) {
    if (!e) return VP_ERR_INVALID;
    if (!d_out) return fail(e->c, VP_ERR_INVALID, "cocoeval: null accumulate destination");
    return accumulate_enqueue(e, (char*)d_out, (hipStream_t)caller_stream);
}

int vp_cocoeval_accumulate(vp_cocoeval_handle e, void* out) {
    if (!e) return VP_ERR_INVALID;
    vp_ctx* c = e->c;
    if (!out) return fail(c, VP_ERR_INVALID, "cocoeval: null accumulate destination");
    HostStage st(c);   // the result; a blocking copy behind the synchronisation
    st.chk(hipDeviceSynchronize(), "hipDeviceSynchronize()");
    const size_t o_res = st.part(vp::coco_result_bytes());
    if (st.alloc()) return st.rc;
    st.rc = accumulate_enqueue(e, st.at(o_res), st.s);
    st.sync();
    st.chk(hipMemcpy(out, st.at(o_res), vp::coco_result_bytes(), hipMemcpyDeviceToHost), "cocoeval download result");
    return st.rc;
}

int vp_cocoeval_state_bytes(const vp_cocoeval_cfg* cfg, int64_t* bytes) {
    if (!cfg) return fail(nullptr, VP_ERR_INVALID, "cocoeval: null cfg");
    if (!bytes) return fail(nullptr, VP_ERR_INVALID, "cocoeval: null bytes");
    if (cfg->max_records < 1 || cfg->max_records > vp::COCO_MAX_RECORDS) return fail(nullptr, VP_ERR_INVALID, "cocoeval: max_records out of range");
    *bytes = (int64_t)vp::coco_state_bytes(cfg->max_records);
    return VP_OK;
}

int vp_cocoeval_result_bytes(int64_t* bytes) {
    if (!bytes) return fail(nullptr, VP_ERR_INVALID, "cocoeval: null bytes");
    *bytes = (int64_t)vp::coco_result_bytes();
    return VP_OK;
}

int vp_cocoeval_download_state(vp_cocoeval_handle e, void* out) {
    if (!e || !out) return VP_ERR_INVALID;
    return stage_download(e, out, e->state, e->state_bytes);
}

int vp_dbg_cocoeval_update_host(void* state, const vp_cocoeval_cfg* cfg, const double* sigmas, const float* kpts, const float* score, const int32_t* frame, const int32_t* rank,
                                int32_t n, const float* gt_kpts, const float* gt_box, const float* gt_area, const int32_t* gt_flags, const int32_t* gt_frame, int32_t g,
                                int32_t n_frames, int32_t* match) {
    std::string why;
    if (cfg_check(cfg, sigmas, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    if (!state) return fail(nullptr, VP_ERR_INVALID, "cocoeval: null state");
    const UpdateArgs u{kpts, score, frame, rank, n, gt_kpts, gt_box, gt_area, gt_flags, gt_frame, g, n_frames, match};
    if (update_check(u, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    std::vector<double> vars;
    host_vars(sigmas, cfg->n_joints, vars);
    update_host((char*)state, cfg->n_joints, cfg->max_records, vars.data(), u);
    return VP_OK;
}

int vp_dbg_cocoeval_accumulate_host(const void* state, const vp_cocoeval_cfg* cfg, void* out) {
    if (!cfg) return fail(nullptr, VP_ERR_INVALID, "cocoeval: null cfg");
    if (cfg->max_records < 1 || cfg->max_records > vp::COCO_MAX_RECORDS) return fail(nullptr, VP_ERR_INVALID, "cocoeval: max_records out of range");
    if (!state) return fail(nullptr, VP_ERR_INVALID, "cocoeval: null state");
    if (!out) return fail(nullptr, VP_ERR_INVALID, "cocoeval: null accumulate destination");
    const int64_t R = ((const int64_t*)state)[vp::COCO_W_RECORDS];
    if (R < 0 || R > cfg->max_records) return fail(nullptr, VP_ERR_INVALID, "cocoeval: the state's records word lies outside 0..max_records");
    accumulate_host((const char*)state, (char*)out);
    return VP_OK;
}

}  // extern "C"
