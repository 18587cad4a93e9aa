// vp_detector_* / vp_detect*: a detector's raw head to tracker-ready box rows as a stream-ordered device stage (semantics: detgeom.h), its synchronous host twin
// vp_detect and the host tap vp_dbg_detect_host.  Three launches per call: det_scan_kernel over (anchor tiles x images) finds the candidates (one global atomic per
// workgroup reserves their slots, in arbitrary order), det_nms_kernel, one workgroup per image, ranks them on the 64-bit key -- which restores a fixed order -- runs
// the greedy NMS and re-zeroes the image's counters, det_pack_kernel, one thread per output row, packs the images' rows.  Every output is a pure function of the inputs.
#include "api_internal.h"
#include "hoststage.h"
#include "stageobj.h"
#include "detgeom.h"

using namespace vpi;

struct vp_detector : StageObj {
    vp::DetParams p{};
    int max_anchors = 0, max_images = 0;
    vp::DetCand* cand = nullptr;    // device [max_images][DET_MAX_CAND]
    int32_t* counters = nullptr;    // device [max_images][2]: candidates found, scan flags; zero between calls
    float* st_rows = nullptr;       // device [max_images][max_det][6]: the picks of an image
    int32_t* st_anchor = nullptr;   // device [max_images][max_det]
    int32_t* st_n = nullptr;        // device [max_images][2]: picks, flags
};

namespace vp {

constexpr int SCAN_THREADS = 128, SCAN_WAVES = SCAN_THREADS / 64, NMS_THREADS = 512, NMS_PER_THREAD = DET_MAX_CAND / NMS_THREADS, PACK_THREADS = 256;

typedef _Float16 det_half8 __attribute__((ext_vector_type(8)));

// APT consecutive elements from p as float32 (fp16 widened exactly); APT > 1: one 16-byte load, p is 16-byte aligned
template <typename T, int APT> __device__ inline void det_load(const T* __restrict__ p, float* v) {
    if constexpr (APT == 1) {
        v[0] = (float)p[0];
    } else if constexpr (sizeof(T) == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        const det_half8 q = *reinterpret_cast<const det_half8*>(p);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (float)q[k];
    }
}

// Kernel A.  LAYOUT 0 ([C, A] per image): lanes run along A, a lane owns APT consecutive anchors (APT > 1 only where every class row is 16-byte aligned: the host
// checks the base pointer and A).  LAYOUT 1 ([A, C]): a lane owns one anchor and walks its row.
template <typename T, int APT, int LAYOUT>
__global__ __launch_bounds__(SCAN_THREADS) void det_scan_kernel(const T* __restrict__ pred, int A, DetParams p, DetCand* __restrict__ cand, int32_t* __restrict__ counters) {
    __shared__ int32_t s_wave[SCAN_WAVES], s_base;
    const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = 4 + p.nc;
    const T* base = pred + (size_t)img * C * A;
    const int a0 = (blockIdx.x * SCAN_THREADS + tid) * APT;   // < 2^20 + SCAN_THREADS * APT
    const bool in = a0 < A;                                   // APT > 1: A is a multiple of APT, so a lane's anchors are all inside or all outside
    float best[APT], box[4][APT];
    int cls[APT];
#pragma unroll
    for (int k = 0; k < APT; ++k) { best[k] = 0.f; cls[k] = -1; box[0][k] = box[1][k] = box[2][k] = box[3][k] = 0.f; }
    if (in) {
        if constexpr (LAYOUT == 0) {
            const T* col = base + a0;
#pragma unroll 4   // measured at 64 images of 84 x 8400: unroll 8 is slower (fp16 41.7 against 29.5 us, fp32 31.0 against 30.1 us)
            for (int c = 0; c < p.nc; ++c) {
                float s[APT];
                det_load<T, APT>(col + (size_t)(4 + c) * A, s);
#pragma unroll
                for (int k = 0; k < APT; ++k) det_pick(s[k], c, best[k], cls[k]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) det_load<T, APT>(col + (size_t)q * A, box[q]);
        } else {
            const T* row = base + (size_t)a0 * C;
#pragma unroll 4
            for (int c = 0; c < p.nc; ++c) det_pick((float)row[4 + c], c, best[0], cls[0]);
#pragma unroll
            for (int q = 0; q < 4; ++q) box[q][0] = (float)row[q];
        }
    }
    int kind[APT], mine = 0, bad = 0;
#pragma unroll
    for (int k = 0; k < APT; ++k) {
        kind[k] = in ? det_candidate(p, best[k], cls[k], box[0][k], box[1][k], box[2][k], box[3][k]) : 0;
        mine += kind[k] == 1;
        bad |= kind[k] == 2;
    }
    // exclusive prefix of `mine` over the workgroup, one reservation for all of it
    int inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    const int any_bad = __syncthreads_or(bad);
    int off = inc - mine, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) {
        if (w < wave) off += s_wave[w];
        total += s_wave[w];
    }
    if (tid == 0) {
        s_base = total > 0 ? atomicAdd(&counters[img * 2], total) : 0;
        if (any_bad) atomicOr(&counters[img * 2 + 1], DET_FLAG_BAD_BOX);
    }
    __syncthreads();
    int slot = s_base + off;
#pragma unroll
    for (int k = 0; k < APT; ++k)
        if (kind[k] == 1) {
            if (slot < DET_MAX_CAND) {   // an image beyond the cap is not processed: its surplus candidates are only counted
                DetCand cd;
                cd.cx = box[0][k]; cd.cy = box[1][k]; cd.w = box[2][k]; cd.h = box[3][k]; cd.score = best[k]; cd.cls = cls[k]; cd.anchor = a0 + k; cd.pad = 0;
                cand[(size_t)img * DET_MAX_CAND + slot] = cd;
            }
            ++slot;
        }
}

struct NmsLds {
    uint64_t key[DET_MAX_CAND];
    float box[DET_MAX_CAND][4];
    uint8_t cls[DET_MAX_CAND], live[DET_MAX_CAND];
    uint16_t picks[DET_MAX_DET];
};
static_assert(sizeof(NmsLds) <= 64 * 1024, "the NMS kernel's static LDS");

// Kernel B: one workgroup per image
__global__ __launch_bounds__(NMS_THREADS) void det_nms_kernel(const DetCand* __restrict__ cand, int32_t* __restrict__ counters, DetParams p, DetImages images, int max_det_stride,
                                                              float* __restrict__ st_rows, int32_t* __restrict__ st_anchor, int32_t* __restrict__ st_n) {
    __shared__ NmsLds L;
    const int img = blockIdx.x, tid = threadIdx.x;
    const int found = counters[img * 2];
    int flags = counters[img * 2 + 1];
    if (found > DET_MAX_CAND) flags |= DET_FLAG_CAND;
    const int n = found > DET_MAX_CAND ? 0 : found;
    const DetCand* mine = cand + (size_t)img * DET_MAX_CAND;

    // rank every candidate on its key: the keys are pairwise distinct (the anchor is part of them), so the ranks are a permutation
    uint64_t k[NMS_PER_THREAD];
    int rank[NMS_PER_THREAD];
#pragma unroll
    for (int q = 0; q < NMS_PER_THREAD; ++q) {
        const int i = tid + q * NMS_THREADS;
        k[q] = i < n ? det_key(mine[i].score, mine[i].anchor) : ~(uint64_t)0;
        rank[q] = 0;
        L.key[i] = k[q];
        L.live[i] = i < n;
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const uint64_t o = L.key[j];
#pragma unroll
        for (int q = 0; q < NMS_PER_THREAD; ++q) rank[q] += o < k[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NMS_PER_THREAD; ++q) {
        const int i = tid + q * NMS_THREADS;
        if (i < n) {
            const DetCand cd = mine[i];
            const int r = rank[q];   // < n
            L.key[r] = k[q];
            det_box(cd.cx, cd.cy, cd.w, cd.h, L.box[r]);
            L.cls[r] = (uint8_t)cd.cls;
        }
    }
    __syncthreads();

    // the greedy walk: picks are serial, the sweep of a pick runs over the lanes
    int n_pick = 0;
    for (int i = 0; i < n && n_pick < p.max_det;) {
        // the next live candidate from i on, eight flags per read (live[] is DET_MAX_CAND long and zero from n on)
        const uint64_t w = *reinterpret_cast<const uint64_t*>(&L.live[i & ~7]) >> ((i & 7) * 8);
        if (w == 0) { i = (i & ~7) + 8; continue; }
        i += (__ffsll((unsigned long long)w) - 1) >> 3;
        if (i >= n) break;
        if (tid == 0) L.picks[n_pick] = (uint16_t)i;
        ++n_pick;
        const float a[4] = {L.box[i][0], L.box[i][1], L.box[i][2], L.box[i][3]};
        const int ca = L.cls[i];
        for (int j = i + 1 + tid; j < n; j += NMS_THREADS)
            if (L.live[j] && (p.agnostic || L.cls[j] == ca) && !(det_iou(a, L.box[j], p.extent) <= p.iou_thr)) L.live[j] = 0;
        ++i;
        __syncthreads();
    }
    __syncthreads();   // picks[] of the last pick (a walk without a pick has no barrier of its own)

    const DetImage im = images.im[img];
    for (int r = tid; r < n_pick; r += NMS_THREADS) {
        const int i = L.picks[r];
        float out[4];
        det_to_frame(im, L.box[i], out);
        float* row = st_rows + ((size_t)img * max_det_stride + r) * 6;
        row[0] = out[0]; row[1] = out[1]; row[2] = out[2]; row[3] = out[3];
        row[4] = det_key_score(L.key[i]);
        row[5] = (float)L.cls[i];
        st_anchor[(size_t)img * max_det_stride + r] = (int32_t)(uint32_t)L.key[i];
    }
    if (tid == 0) {
        st_n[img * 2] = n_pick;
        st_n[img * 2 + 1] = flags;
        counters[img * 2] = 0;       // the next call (or the next replay of a captured one) starts from zero
        counters[img * 2 + 1] = 0;
    }
}

// Kernel C: the images' rows packed into the caller's buffers, images ascending; rows up to n_out are "absent".  One row per thread; every workgroup repeats the
// prefix over the (at most 64) image counts, the first one also writes counts and flags.  (As ONE workgroup it took 78 us for the 19200 rows of 64 images, more
// than the scan and the NMS together: profiles/detect_device.txt.)
__global__ __launch_bounds__(PACK_THREADS) void det_pack_kernel(const float* __restrict__ st_rows, const int32_t* __restrict__ st_anchor, const int32_t* __restrict__ st_n,
                                                                int n_images, int max_det_stride, float* __restrict__ rows, int32_t* __restrict__ image,
                                                                int32_t* __restrict__ anchor, int n_out, int32_t* __restrict__ count, int32_t* __restrict__ flags_out) {
    __shared__ int32_t s_cnt[DET_MAX_IMAGES], s_off[DET_MAX_IMAGES + 1];
    const int tid = threadIdx.x;
    if (tid < n_images) s_cnt[tid] = st_n[tid * 2];
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int s = 0; s < n_images; ++s) { s_off[s] = acc; acc += s_cnt[s]; }
        s_off[n_images] = acc;
    }
    __syncthreads();
    const int total = s_off[n_images];
    if (blockIdx.x == 0 && tid < n_images) {
        count[tid] = s_cnt[tid];
        if (flags_out) {
            int f = st_n[tid * 2 + 1];
            if (s_cnt[tid] > 0 && s_off[tid] + s_cnt[tid] > n_out) f |= DET_FLAG_ROWS;   // rows of THIS image were cut
            flags_out[tid] = f;
        }
    }
    if (blockIdx.x == 0 && tid == 0) count[n_images] = total;
    const int i = blockIdx.x * PACK_THREADS + tid;
    if (i < n_out) {
        if (i < total) {
            int s = 0;
            while (s + 1 < n_images && s_off[s + 1] <= i) ++s;   // at most n_images - 1 steps
            const size_t src = (size_t)s * max_det_stride + (i - s_off[s]);
#pragma unroll
            for (int q = 0; q < 6; ++q) rows[(size_t)i * 6 + q] = st_rows[src * 6 + q];
            image[i] = s;
            anchor[i] = st_anchor[src];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) rows[(size_t)i * 6 + q] = NAN;
            rows[(size_t)i * 6 + 4] = 0.f;
            rows[(size_t)i * 6 + 5] = -1.f;
            image[i] = -1;
            anchor[i] = -1;
        }
    }
}

}  // namespace vp

namespace {

float widen(const void* pred, int dtype, size_t idx) {
    return dtype == VP_DET_F16 ? (float)((const _Float16*)pred)[idx] : ((const float*)pred)[idx];
}

// ---- the host model: detgeom.h run serially (HOST ONLY)
void detect_host(const vp::DetParams& p, const void* pred, int A, const vp_det_image* images, int n_images, float* rows, int32_t* image, int32_t* anchor, int n_out,
                 int32_t* count, int32_t* flags_out) {
    using namespace vp;
    const int C = 4 + p.nc;
    int total = 0;
    std::vector<DetCand> cand;
    std::vector<std::pair<uint64_t, int>> order;
    std::vector<float> box;
    std::vector<char> live;
    for (int img = 0; img < n_images; ++img) {
        const size_t base = (size_t)img * C * A;
        auto at = [&](int ch, int a) { return widen(pred, p.dtype, p.layout == 0 ? base + (size_t)ch * A + a : base + (size_t)a * C + ch); };
        cand.clear();
        int flags = 0, found = 0;
        for (int a = 0; a < A; ++a) {
            float best = 0.f;
            int cls = -1;
            for (int c = 0; c < p.nc; ++c) det_pick(at(4 + c, a), c, best, cls);
            const float cx = at(0, a), cy = at(1, a), w = at(2, a), h = at(3, a);
            const int kind = det_candidate(p, best, cls, cx, cy, w, h);
            if (kind == 2) flags |= DET_FLAG_BAD_BOX;
            if (kind != 1) continue;
            if (found < DET_MAX_CAND) cand.push_back(DetCand{cx, cy, w, h, best, cls, a, 0});
            ++found;
        }
        if (found > DET_MAX_CAND) { flags |= DET_FLAG_CAND; cand.clear(); }
        const int n = (int)cand.size();
        order.resize((size_t)n);
        for (int i = 0; i < n; ++i) order[i] = {det_key(cand[i].score, cand[i].anchor), i};
        std::sort(order.begin(), order.end());
        box.resize((size_t)n * 4);
        live.assign((size_t)n, 1);
        for (int r = 0; r < n; ++r) {
            const DetCand& cd = cand[order[r].second];
            det_box(cd.cx, cd.cy, cd.w, cd.h, &box[(size_t)r * 4]);
        }
        int n_pick = 0;
        DetImage im;
        std::memcpy(&im, &images[img], sizeof(im));
        for (int i = 0; i < n && n_pick < p.max_det; ++i) {
            if (!live[i]) continue;
            const DetCand& ci = cand[order[i].second];
            for (int j = i + 1; j < n; ++j)
                if (live[j] && (p.agnostic || cand[order[j].second].cls == ci.cls) && !(det_iou(&box[(size_t)i * 4], &box[(size_t)j * 4], p.extent) <= p.iou_thr)) live[j] = 0;
            const int o = total + n_pick;
            if (o < n_out) {
                det_to_frame(im, &box[(size_t)i * 4], rows + (size_t)o * 6);
                rows[(size_t)o * 6 + 4] = det_key_score(order[i].first);
                rows[(size_t)o * 6 + 5] = (float)ci.cls;
                image[o] = img;
                anchor[o] = ci.anchor;
            }
            ++n_pick;
        }
        count[img] = n_pick;
        if (flags_out) flags_out[img] = flags | (n_pick > 0 && total + n_pick > n_out ? DET_FLAG_ROWS : 0);
        total += n_pick;
    }
    count[n_images] = total;
    for (int i = total; i < n_out; ++i) {
        for (int q = 0; q < 4; ++q) rows[(size_t)i * 6 + q] = NAN;
        rows[(size_t)i * 6 + 4] = 0.f;
        rows[(size_t)i * 6 + 5] = -1.f;
        image[i] = -1;
        anchor[i] = -1;
    }
}

bool finite_f(float v) { return vp::det_finite(v); }

// every refusal (HOST ONLY), before anything is enqueued
int cfg_check(const vp_det_cfg* cfg, vp::DetParams& p, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "detector: " + m; return (int)VP_ERR_INVALID; };
    if (!cfg) return bad("null cfg");
    if (cfg->nc < 1 || cfg->nc > VP_DET_MAX_CLASSES) return bad("nc = " + std::to_string(cfg->nc) + " outside 1.." + std::to_string(VP_DET_MAX_CLASSES));
    if (cfg->max_anchors < 1 || cfg->max_anchors > vp::DET_MAX_ANCHORS) return bad("max_anchors = " + std::to_string(cfg->max_anchors) + " outside 1.." + std::to_string(vp::DET_MAX_ANCHORS));
    if (cfg->max_images < 1 || cfg->max_images > VP_DET_MAX_IMAGES) return bad("max_images = " + std::to_string(cfg->max_images) + " outside 1.." + std::to_string(VP_DET_MAX_IMAGES));
    if (cfg->dtype != VP_DET_F32 && cfg->dtype != VP_DET_F16) return bad("dtype = " + std::to_string(cfg->dtype) + " is neither VP_DET_F32 nor VP_DET_F16");
    if (cfg->layout != 0 && cfg->layout != 1) return bad("layout = " + std::to_string(cfg->layout) + " is neither 0 nor 1");
    if (!(finite_f(cfg->conf_thr) && cfg->conf_thr >= 0.f)) return bad("conf_thr not finite or < 0");
    if (!(cfg->iou_thr >= 0.f && cfg->iou_thr <= 1.f)) return bad("iou_thr outside [0, 1]");
    if (!(finite_f(cfg->extent) && cfg->extent >= 0.f)) return bad("extent not finite or < 0");
    if (cfg->agnostic != 0 && cfg->agnostic != 1) return bad("agnostic = " + std::to_string(cfg->agnostic) + " is neither 0 nor 1");
    if (cfg->max_det < 1 || cfg->max_det > VP_DET_MAX_DET) return bad("max_det = " + std::to_string(cfg->max_det) + " outside 1.." + std::to_string(VP_DET_MAX_DET));
    bool any = false;
    for (int c = 0; c < cfg->nc; ++c) any = any || ((cfg->class_mask[c >> 5] >> (c & 31)) & 1u);
    if (!any) return bad("class_mask selects no class below nc = " + std::to_string(cfg->nc));
    p.nc = cfg->nc; p.layout = cfg->layout; p.dtype = cfg->dtype; p.agnostic = cfg->agnostic; p.max_det = cfg->max_det;
    p.conf_thr = cfg->conf_thr; p.iou_thr = cfg->iou_thr; p.extent = cfg->extent;
    for (int q = 0; q < 8; ++q) p.class_mask[q] = cfg->class_mask[q];
    return VP_OK;
}

int call_args(const vp::DetParams& p, int max_anchors, int max_images, const void* pred, int A, const vp_det_image* images, int n_images, const void* rows, const void* image,
              const void* anchor, int n_out, const void* count, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "detector: " + m; return (int)VP_ERR_INVALID; };
    if (n_images < 0 || n_images > max_images) return bad("n_images = " + std::to_string(n_images) + " outside 0.." + std::to_string(max_images));
    if (n_out < 0) return bad("negative n_out");
    if (A < 1 || A > max_anchors) return bad("A = " + std::to_string(A) + " outside 1.." + std::to_string(max_anchors));
    if (!count) return bad("null count");
    if (n_out > 0 && !(rows && image && anchor)) return bad("null rows, image or anchor with n_out > 0");
    if (n_images > 0 && !pred) return bad("null pred with n_images > 0");
    if (n_images > 0 && !images) return bad("null images with n_images > 0");
    if ((uintptr_t)pred % (p.dtype == VP_DET_F16 ? 2 : 4)) return bad("pred is not aligned to its element size");
    for (int i = 0; i < n_images; ++i) {
        const vp_det_image& m = images[i];
        if (!(finite_f(m.gain) && m.gain > 0.f)) return bad("image " + std::to_string(i) + ": gain not finite or <= 0");
        if (!(finite_f(m.pad_x) && finite_f(m.pad_y))) return bad("image " + std::to_string(i) + ": pad not finite");
        if (!(finite_f(m.frame_w) && finite_f(m.frame_h) && m.frame_w >= 0.f && m.frame_h >= 0.f)) return bad("image " + std::to_string(i) + ": frame size not finite or < 0");
    }
    return VP_OK;
}

template <typename T> void scan_launch(const vp_detector* d, const void* d_pred, int A, int n_images, hipStream_t s) {
    using namespace vp;
    constexpr int V = 16 / (int)sizeof(T);
    const T* pred = (const T*)d_pred;
    if (d->p.layout == 1) {
        hipLaunchKernelGGL((det_scan_kernel<T, 1, 1>), dim3((A + SCAN_THREADS - 1) / SCAN_THREADS, n_images), dim3(SCAN_THREADS), 0, s, pred, A, d->p, d->cand, d->counters);
    } else if ((uintptr_t)d_pred % 16 == 0 && A % V == 0) {   // every class row of every image starts 16-byte aligned
        hipLaunchKernelGGL((det_scan_kernel<T, V, 0>), dim3((A + SCAN_THREADS * V - 1) / (SCAN_THREADS * V), n_images), dim3(SCAN_THREADS), 0, s, pred, A, d->p, d->cand,
                           d->counters);
    } else {
        hipLaunchKernelGGL((det_scan_kernel<T, 1, 0>), dim3((A + SCAN_THREADS - 1) / SCAN_THREADS, n_images), dim3(SCAN_THREADS), 0, s, pred, A, d->p, d->cand, d->counters);
    }
}

// the checked call on stream s: three launches
int detect_enqueue(vp_detector* d, const void* d_pred, int A, const vp_det_image* images, int n_images, float* d_rows, int32_t* d_image, int32_t* d_anchor, int n_out,
                   int32_t* d_count, int32_t* d_flags, hipStream_t s) {
    vp_ctx* c = d->c;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if (n_images > 0) {
        if (d->p.dtype == VP_DET_F16) scan_launch<_Float16>(d, d_pred, A, n_images, s);
        else scan_launch<float>(d, d_pred, A, n_images, s);
        HIPCHK(c, hipGetLastError());
        vp::DetImages tab;
        std::memset(&tab, 0, sizeof(tab));
        static_assert(sizeof(vp::DetImage) == sizeof(vp_det_image), "vp_det_image and DetImage");
        std::memcpy(tab.im, images, sizeof(vp_det_image) * (size_t)n_images);
        hipLaunchKernelGGL(vp::det_nms_kernel, dim3(n_images), dim3(vp::NMS_THREADS), 0, s, d->cand, d->counters, d->p, tab, d->p.max_det, d->st_rows, d->st_anchor, d->st_n);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(vp::det_pack_kernel, dim3(std::max(1, (n_out + vp::PACK_THREADS - 1) / vp::PACK_THREADS)), dim3(vp::PACK_THREADS), 0, s, d->st_rows, d->st_anchor, d->st_n, n_images, d->p.max_det, d_rows, d_image, d_anchor, n_out,
                       d_count, d_flags);
    HIPCHK(c, hipGetLastError());
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_detector_create(vp_handle c, const vp_det_cfg* cfg, vp_detector_handle* out) {
    return stage_create(c, out, [&](vp_detector* d, std::string* why) { return cfg_check(cfg, d->p, why); },
                        [&](vp_detector* d) {
                            d->max_anchors = cfg->max_anchors;
                            d->max_images = cfg->max_images;
                            const size_t ni = (size_t)cfg->max_images, nd = (size_t)d->p.max_det;
                            d->cand = d->alloc<vp::DetCand>(sizeof(vp::DetCand) * ni * vp::DET_MAX_CAND);
                            d->counters = d->alloc<int32_t>(ni * 8, 0);
                            d->st_rows = d->alloc<float>(ni * nd * 24);
                            d->st_anchor = d->alloc<int32_t>(ni * nd * 4);
                            d->st_n = d->alloc<int32_t>(ni * 8);
                            return "detector workspace: ";
                        });
}

int vp_detector_destroy(vp_detector_handle d) { return stage_destroy(d); }

int vp_detect_stream(vp_detector_handle d, const void* d_pred, int32_t A, const vp_det_image* images, int32_t n_images, float* d_rows, int32_t* d_image, int32_t* d_anchor,
                     int32_t n_out, int32_t* d_count, int32_t* d_flags, void* caller_stream) {
    if (!d) return VP_ERR_INVALID;
    std::string why;
    if (call_args(d->p, d->max_anchors, d->max_images, d_pred, A, images, n_images, d_rows, d_image, d_anchor, n_out, d_count, &why)) return fail(d->c, VP_ERR_INVALID, why);
    return detect_enqueue(d, d_pred, A, images, n_images, d_rows, d_image, d_anchor, n_out, d_count, d_flags, (hipStream_t)caller_stream);
}

int vp_detect(vp_detector_handle d, const void* pred, int32_t A, const vp_det_image* images, int32_t n_images, float* rows, int32_t* image, int32_t* anchor, int32_t n_out,
              int32_t* count, int32_t* flags) {
    if (!d) return VP_ERR_INVALID;
    vp_ctx* c = d->c;
    std::string why;
    if (call_args(d->p, d->max_anchors, d->max_images, pred, A, images, n_images, rows, image, anchor, n_out, count, &why)) return fail(c, VP_ERR_INVALID, why);
    // one scratch block: pred | rows | image | anchor | count | flags
    HostStage st(c);
    const size_t es = d->p.dtype == VP_DET_F16 ? 2 : 4;
    const size_t pred_bytes = (size_t)n_images * (4 + d->p.nc) * (size_t)A * es, ob = (size_t)n_out * 4, sb = (size_t)(n_images + 1) * 4;
    const size_t o_pred = st.part(pred_bytes), o_rows = st.part((size_t)n_out * 24), o_im = st.part(ob), o_an = st.part(ob), o_ct = st.part(sb), o_fl = st.part(sb);
    if (st.alloc()) return st.rc;
    char* d_pred = st.at(o_pred);
    float* d_rows = st.at<float>(o_rows);
    int32_t *d_im = st.at<int32_t>(o_im), *d_an = st.at<int32_t>(o_an), *d_ct = st.at<int32_t>(o_ct), *d_fl = st.at<int32_t>(o_fl);
    if (pred_bytes) st.up(d_pred, pred, pred_bytes, "upload pred");
    if (!st.rc) st.rc = detect_enqueue(d, d_pred, A, images, n_images, d_rows, d_im, d_an, n_out, d_ct, d_fl, st.s);
    if (!st.rc) {
        if (n_out) {
            st.down(rows, d_rows, (size_t)n_out * 24, "download rows");
            st.down(image, d_im, ob, "download image");
            st.down(anchor, d_an, ob, "download anchor");
        }
        st.down(count, d_ct, sb, "download count");
        if (flags && n_images) st.down(flags, d_fl, (size_t)n_images * 4, "download flags");
    }
    st.sync();
    return st.rc;
}

int vp_dbg_detect_host(const vp_det_cfg* cfg, const void* pred, int32_t A, const vp_det_image* images, int32_t n_images, float* rows, int32_t* image, int32_t* anchor,
                       int32_t n_out, int32_t* count, int32_t* flags) {
    vp::DetParams p;
    std::string why;
    if (cfg_check(cfg, p, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    if (call_args(p, cfg->max_anchors, cfg->max_images, pred, A, images, n_images, rows, image, anchor, n_out, count, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    detect_host(p, pred, A, images, n_images, rows, image, anchor, n_out, count, flags);
    return VP_OK;
}

}  // extern "C"
