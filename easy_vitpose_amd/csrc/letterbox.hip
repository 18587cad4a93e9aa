// vp_letterbox*: frames (vp_image: NV12 / BGR24 / RGB24, pitched) to a detector's input tensor as a stream-ordered device stage (semantics: lbgeom.h), its
// synchronous host twin vp_letterbox, the host-only plan vp_letterbox_plan and the host tap vp_dbg_letterbox_host.  One kernel, a workgroup per output row: adjacent lanes fetch
// adjacent pixels into LDS, then a lane stores a run of adjacent x -- 16 bytes per channel plane -- so the stores are dwordx4 whatever the dtype; the image records travel by kernel argument, LB_PER_LAUNCH per launch.
#include "api_internal.h"
#include "hoststage.h"
#include "detgeom.h"
#include "lbgeom.h"

using namespace vpi;

namespace vp {

constexpr int LB_THREADS = 128, LB_PER_LAUNCH = 32;
struct LbRecs { LbRec r[LB_PER_LAUNCH]; };   // a kernel argument
static_assert(sizeof(LbRec) == 88 && sizeof(LbRecs) + sizeof(LbParams) + 16 <= 4096, "the image records of a launch fit the kernel argument segment");

template <int DTYPE> struct LbElem;
template <> struct LbElem<LB_F32> { typedef float T; };
template <> struct LbElem<LB_F16> { typedef _Float16 T; };
template <> struct LbElem<LB_U8> { typedef uint8_t T; };

__host__ __device__ inline int lb_plane_stride(int in_w) { return (in_w + 15) & ~15; }   // bytes of one channel plane of the row in LDS
template <int DTYPE> __host__ __device__ inline int lb_lds_bytes(int in_w) { return 256 * (int)sizeof(typename LbElem<DTYPE>::T) + 3 * lb_plane_stride(in_w); }

// pass 1 of a row inside the placed frame: adjacent lanes take adjacent output pixels (their taps are neighbours in the source: coalesced loads) and leave the RGB8
// values, already in the output's channel order, in the three channel planes of the row in LDS
template <int FMT> __device__ __forceinline__ void lb_row(const LbRec& r, const LbParams& p, int y, uint8_t* __restrict__ s_row, int stride) {
    const YuvCoef k = yuv_coef(FMT == PIX_NV12 ? r.matrix : 0);
    LbAxis cy{0, 0, 0, 0};
    if (r.mode == LB_RESIZE) cy = lb_axis(y, r.scale_y, r.h);   // once per row
    for (int ox = threadIdx.x; ox < p.in_w; ox += LB_THREADS) {
        int rgb[3] = {p.pad_value, p.pad_value, p.pad_value};
        const int x = ox - r.left;
        if ((unsigned)x < (unsigned)r.new_w) lb_pixel<FMT>(r, k, cy, y, x, rgb);   // a pixel of the pad fetches nothing
        s_row[ox] = (uint8_t)(p.order ? rgb[2] : rgb[0]);
        s_row[stride + ox] = (uint8_t)rgb[1];
        s_row[2 * stride + ox] = (uint8_t)(p.order ? rgb[0] : rgb[2]);
    }
}

// One workgroup per output row: grid (in_h, images of this launch), dynamic LDS lb_lds_bytes (the table of the 256 output values, then the row's three planes).
// Pass 2: a lane takes a run of R adjacent x -- 16 output bytes per channel plane.  VEC: the output base is 16-byte aligned and in_w is a multiple of R, so every
// run of every plane is one aligned 16-byte store; otherwise element stores with the row end checked.  Both write the same values.  A row wholly in the pad skips
// pass 1 and stores the constant.
template <int DTYPE, bool VEC>
__global__ __launch_bounds__(LB_THREADS) void letterbox_kernel(LbRecs recs, LbParams p, int first_image, void* __restrict__ out_) {
    typedef typename LbElem<DTYPE>::T T;
    constexpr int R = 16 / (int)sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(R)));
    typedef uint8_t RunT __attribute__((ext_vector_type(R)));
    extern __shared__ __attribute__((aligned(16))) uint8_t s_lds[];
    T* s_tab = reinterpret_cast<T*>(s_lds);   // the 256 output values, two correctly rounded divisions per thread
    uint8_t* s_row = s_lds + 256 * sizeof(T);
    const int stride = lb_plane_stride(p.in_w);
    for (int v = threadIdx.x; v < 256; v += LB_THREADS) {
        if constexpr (DTYPE == LB_F32) s_tab[v] = lb_f32(v);
        else if constexpr (DTYPE == LB_F16) s_tab[v] = lb_f16(v);
        else s_tab[v] = (uint8_t)v;
    }
    const int oy = blockIdx.x;
    const LbRec& r = recs.r[blockIdx.y];
    const int y = oy - r.top;
    const bool row_in = (unsigned)y < (unsigned)r.new_h;   // the same for the whole workgroup
    if (row_in) {
        if (r.format == PIX_NV12) lb_row<PIX_NV12>(r, p, y, s_row, stride);
        else if (r.format == PIX_RGB24) lb_row<PIX_RGB24>(r, p, y, s_row, stride);
        else lb_row<PIX_BGR24>(r, p, y, s_row, stride);
    }
    __syncthreads();
    T* out = (T*)out_;
    const int64_t n = first_image + blockIdx.y;
    const int runs = (p.in_w + R - 1) / R;
    for (int run = threadIdx.x; run < runs; run += LB_THREADS) {
        const int x0 = run * R;
        RunT v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (row_in) v[c] = *reinterpret_cast<const RunT*>(s_row + c * stride + x0);   // (bytes behind in_w in the last run are read, never stored)
            else v[c] = (RunT)(uint8_t)p.pad_value;
        }
        if (p.layout == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                T* dst = out + lb_index(p, n, c, oy, x0);
                if constexpr (VEC) {
                    VecT q;
#pragma unroll
                    for (int j = 0; j < R; ++j) q[j] = s_tab[v[c][j]];
                    *reinterpret_cast<VecT*>(dst) = q;
                } else {
#pragma unroll
                    for (int j = 0; j < R; ++j)
                        if (x0 + j < p.in_w) dst[j] = s_tab[v[c][j]];
                }
            }
        } else {
            T* dst = out + lb_index(p, n, 0, oy, x0);   // 3 R contiguous elements
            if constexpr (VEC) {
                T e[3 * R];
#pragma unroll
                for (int j = 0; j < R; ++j) { e[3 * j] = s_tab[v[0][j]]; e[3 * j + 1] = s_tab[v[1][j]]; e[3 * j + 2] = s_tab[v[2][j]]; }
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    VecT q;
#pragma unroll
                    for (int j = 0; j < R; ++j) q[j] = e[g * R + j];
                    reinterpret_cast<VecT*>(dst)[g] = q;
                }
            } else {
#pragma unroll
                for (int j = 0; j < R; ++j)
                    if (x0 + j < p.in_w) { dst[3 * j] = s_tab[v[0][j]]; dst[3 * j + 1] = s_tab[v[1][j]]; dst[3 * j + 2] = s_tab[v[2][j]]; }
            }
        }
    }
}

}  // namespace vp

namespace {

using vp::LbParams;
using vp::LbRec;

// every refusal of the configuration (HOST ONLY)
int cfg_check(const vp_letterbox_cfg* cfg, LbParams& p, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "letterbox: " + m; return (int)VP_ERR_INVALID; };
    if (!cfg) return bad("null cfg");
    if (cfg->in_h < 1 || cfg->in_h > vp::LB_MAX_SIDE || cfg->in_w < 1 || cfg->in_w > vp::LB_MAX_SIDE)
        return bad("input " + std::to_string(cfg->in_h) + " x " + std::to_string(cfg->in_w) + " outside 1.." + std::to_string(vp::LB_MAX_SIDE));
    if (cfg->dtype != VP_LB_F32 && cfg->dtype != VP_LB_F16 && cfg->dtype != VP_LB_U8) return bad("dtype = " + std::to_string(cfg->dtype) + " is none of VP_LB_F32, VP_LB_F16, VP_LB_U8");
    if (cfg->layout != 0 && cfg->layout != 1) return bad("layout = " + std::to_string(cfg->layout) + " is neither 0 (NCHW) nor 1 (NHWC)");
    if (cfg->order != 0 && cfg->order != 1) return bad("order = " + std::to_string(cfg->order) + " is neither 0 (RGB) nor 1 (BGR)");
    if (cfg->pad_value < 0 || cfg->pad_value > 255) return bad("pad_value = " + std::to_string(cfg->pad_value) + " outside 0..255");
    if (cfg->scaleup != 0 && cfg->scaleup != 1) return bad("scaleup = " + std::to_string(cfg->scaleup) + " is neither 0 nor 1");
    p = LbParams{cfg->in_h, cfg->in_w, cfg->dtype, cfg->layout, cfg->order, cfg->pad_value};
    return VP_OK;
}

// the two host tables of a call, kept aside until every refusal has passed: a refused call leaves the caller's arrays as they were
struct Tables {
    std::vector<vp_det_image> det;
    std::vector<int32_t> placement;
    void publish(vp_det_image* d, int32_t* pl) const {   // either may be null
        if (d && !det.empty()) std::memcpy(d, det.data(), sizeof(vp_det_image) * det.size());
        if (pl && !placement.empty()) std::memcpy(pl, placement.data(), sizeof(int32_t) * placement.size());
    }
};

// the plan of a call (HOST ONLY): every refusal that needs no device, the records, the undo table and the placement
int plan(const vp_letterbox_cfg* cfg, const vp_image* images, int n_images, LbParams& p, std::vector<LbRec>& recs, Tables& t, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "letterbox: " + m; return (int)VP_ERR_INVALID; };
    if (cfg_check(cfg, p, why)) return VP_ERR_INVALID;
    if (n_images < 0 || n_images > VP_LB_MAX_IMAGES) return bad("n_images = " + std::to_string(n_images) + " outside 0.." + std::to_string(VP_LB_MAX_IMAGES));
    if (n_images > 0 && !images) return bad("null images with n_images > 0");
    recs.resize((size_t)n_images);
    t.det.resize((size_t)n_images);
    t.placement.resize((size_t)n_images * 4);
    for (int f = 0; f < n_images; ++f) {
        const vp_image& im = images[f];
        if (im.h < 1 || im.w < 1) return bad("frame " + std::to_string(f) + " has a non-positive size " + std::to_string(im.h) + " x " + std::to_string(im.w));
        std::string w;
        if (image_check(im, f, &w)) return bad(w);
        vp::LbPlace pl;
        vp::LbUndo un;
        if (!vp::lb_geometry(im.h, im.w, p.in_h, p.in_w, cfg->scaleup, &pl, &un))
            return bad("frame " + std::to_string(f) + " of " + std::to_string(im.h) + " x " + std::to_string(im.w) + " scales to an empty image in " + std::to_string(p.in_h) + " x " +
                       std::to_string(p.in_w));
        LbRec& r = recs[f];
        r.plane[0] = im.plane[0]; r.plane[1] = im.plane[1];
        r.pitch[0] = im.pitch[0]; r.pitch[1] = im.pitch[1];
        r.h = im.h; r.w = im.w; r.format = im.format; r.matrix = im.format == vp::PIX_NV12 ? im.matrix : 0;
        r.left = pl.left; r.top = pl.top; r.new_w = pl.new_w; r.new_h = pl.new_h;
        r.pad_ = 0;
        vp::lb_resize_mode(im.h, im.w, pl, &r);
        t.det[f] = vp_det_image{un.gain, un.pad_x, un.pad_y, (float)im.w, (float)im.h};
        t.placement[4 * f] = pl.left; t.placement[4 * f + 1] = pl.top; t.placement[4 * f + 2] = pl.new_w; t.placement[4 * f + 3] = pl.new_h;
    }
    return VP_OK;
}

// what the entries that read pixels refuse on top of the plan
int out_check(const LbParams& p, const vp_image* images, int n_images, const void* out, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "letterbox: " + m; return (int)VP_ERR_INVALID; };
    for (int f = 0; f < n_images; ++f)
        if (!images[f].plane[0]) return bad("frame " + std::to_string(f) + " has no data (plane[0] is null)");
    if (n_images > 0 && !out) return bad("null output with n_images > 0");
    if ((uintptr_t)out % (uintptr_t)vp::lb_elem_bytes(p.dtype)) return bad("the output is not aligned to its element size");
    return VP_OK;
}

// frame f is read in place: every plane device memory of the handle's device, inside one allocation (the check of the image entries)
int check_device_image(vp_ctx* c, const vp_image& im, int f) {
    bool ok = true;
    for (int pl = 0; pl < plane_count(im) && ok; ++pl) ok = device_range_ok(c, im.plane[pl], plane_bytes(im, pl));
    if (ok) return VP_OK;
    (void)hipGetLastError();
    return fail(c, VP_ERR_INVALID, "letterbox: frame " + std::to_string(f) + " is not device memory of device " + std::to_string(c->cfg.device_id) +
                                       " (or runs past the end of its allocation)");
}

template <int DTYPE> void launch(const vp::LbRecs& tab, const LbParams& p, int first, int count, void* d_out, hipStream_t s) {
    constexpr int R = 16 / (int)sizeof(typename vp::LbElem<DTYPE>::T);
    const dim3 grid((unsigned)p.in_h, (unsigned)count);
    const size_t lds = (size_t)vp::lb_lds_bytes<DTYPE>(p.in_w);   // <= 1 KiB + 3 * 8192
    if ((uintptr_t)d_out % 16 == 0 && p.in_w % R == 0) hipLaunchKernelGGL((vp::letterbox_kernel<DTYPE, true>), grid, dim3(vp::LB_THREADS), lds, s, tab, p, first, d_out);
    else hipLaunchKernelGGL((vp::letterbox_kernel<DTYPE, false>), grid, dim3(vp::LB_THREADS), lds, s, tab, p, first, d_out);
}

// the checked call on stream s (the handle's device is current): one launch per LB_PER_LAUNCH images
int enqueue(vp_ctx* c, const LbParams& p, const std::vector<LbRec>& recs, void* d_out, hipStream_t s) {
    const int n = (int)recs.size();
    for (int first = 0; first < n; first += vp::LB_PER_LAUNCH) {
        const int count = std::min(vp::LB_PER_LAUNCH, n - first);
        vp::LbRecs tab;
        std::memset(&tab, 0, sizeof(tab));
        std::memcpy(tab.r, recs.data() + first, sizeof(LbRec) * (size_t)count);
        if (p.dtype == VP_LB_F32) launch<vp::LB_F32>(tab, p, first, count, d_out, s);
        else if (p.dtype == VP_LB_F16) launch<vp::LB_F16>(tab, p, first, count, d_out, s);
        else launch<vp::LB_U8>(tab, p, first, count, d_out, s);
        HIPCHK(c, hipGetLastError());
    }
    return VP_OK;
}

// ---- the host model: lbgeom.h run serially (HOST ONLY)
template <int FMT> void host_image(const LbParams& p, const LbRec& r, int64_t n, void* out) {
    const vp::YuvCoef k = vp::yuv_coef(FMT == vp::PIX_NV12 ? r.matrix : 0);
    for (int oy = 0; oy < p.in_h; ++oy) {
        const int y = oy - r.top;
        const bool row_in = (unsigned)y < (unsigned)r.new_h;
        vp::LbAxis cy{0, 0, 0, 0};
        if (row_in && r.mode == vp::LB_RESIZE) cy = vp::lb_axis(y, r.scale_y, r.h);
        for (int ox = 0; ox < p.in_w; ++ox) {
            int rgb[3] = {p.pad_value, p.pad_value, p.pad_value};
            const int x = ox - r.left;
            if (row_in && (unsigned)x < (unsigned)r.new_w) vp::lb_pixel<FMT>(r, k, cy, y, x, rgb);
            for (int c = 0; c < 3; ++c) {
                const int v = rgb[p.order ? 2 - c : c] & 255;
                const int64_t i = vp::lb_index(p, n, c, oy, ox);
                if (p.dtype == VP_LB_F32) ((float*)out)[i] = vp::lb_f32(v);
                else if (p.dtype == VP_LB_F16) ((_Float16*)out)[i] = vp::lb_f16(v);
                else ((uint8_t*)out)[i] = (uint8_t)v;
            }
        }
    }
}

}  // namespace

extern "C" {

int vp_letterbox_plan(const vp_letterbox_cfg* cfg, const vp_image* images, int32_t n_images, vp_det_image* det, int32_t* placement) {
    LbParams p;
    std::vector<LbRec> recs;
    Tables t;
    std::string why;
    if (plan(cfg, images, n_images, p, recs, t, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    t.publish(det, placement);
    return VP_OK;
}

int vp_letterbox_stream(vp_handle c, const vp_letterbox_cfg* cfg, const vp_image* images, int32_t n_images, void* d_out, vp_det_image* det, int32_t* placement,
                        void* caller_stream) {
    if (!c) return VP_ERR_INVALID;
    LbParams p;
    std::vector<LbRec> recs;
    Tables t;
    std::string why;
    if (plan(cfg, images, n_images, p, recs, t, &why) || out_check(p, images, n_images, d_out, &why)) return fail(c, VP_ERR_INVALID, why);
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    for (int f = 0; f < n_images; ++f)
        if (check_device_image(c, images[f], f)) return VP_ERR_INVALID;
    t.publish(det, placement);
    return enqueue(c, p, recs, d_out, (hipStream_t)caller_stream);
}

int vp_letterbox(vp_handle c, const vp_letterbox_cfg* cfg, const vp_image* images, int32_t n_images, void* out, vp_det_image* det, int32_t* placement) {
    if (!c) return VP_ERR_INVALID;
    LbParams p;
    std::vector<LbRec> recs;
    Tables t;
    std::string why;
    if (plan(cfg, images, n_images, p, recs, t, &why) || out_check(p, images, n_images, out, &why)) return fail(c, VP_ERR_INVALID, why);
    t.publish(det, placement);
    if (n_images == 0) return VP_OK;
    // one scratch block: the tensor, then every plane at the caller's pitch
    HostStage st(c);
    const size_t out_bytes = (size_t)n_images * 3 * (size_t)p.in_h * (size_t)p.in_w * (size_t)vp::lb_elem_bytes(p.dtype);
    const size_t o_out = st.part(out_bytes);
    std::vector<size_t> off((size_t)n_images * 2, 0);
    for (int f = 0; f < n_images; ++f)
        for (int pl = 0; pl < plane_count(images[f]); ++pl) off[2 * f + pl] = st.part(plane_bytes(images[f], pl));
    if (st.alloc()) return st.rc;
    for (int f = 0; f < n_images && !st.rc; ++f)
        for (int pl = 0; pl < plane_count(images[f]); ++pl) {
            st.up(st.at(off[2 * f + pl]), images[f].plane[pl], plane_bytes(images[f], pl), "upload plane");
            recs[f].plane[pl] = st.at<const uint8_t>(off[2 * f + pl]);
        }
    if (!st.rc) st.rc = enqueue(c, p, recs, st.at(o_out), st.s);
    if (!st.rc) st.down(out, st.at(o_out), out_bytes, "download tensor");
    st.sync();
    return st.rc;
}

int vp_dbg_letterbox_host(const vp_letterbox_cfg* cfg, const vp_image* images, int32_t n_images, void* out, vp_det_image* det, int32_t* placement) {
    LbParams p;
    std::vector<LbRec> recs;
    Tables t;
    std::string why;
    if (plan(cfg, images, n_images, p, recs, t, &why) || out_check(p, images, n_images, out, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    t.publish(det, placement);
    for (int f = 0; f < n_images; ++f) {
        if (recs[f].format == vp::PIX_NV12) host_image<vp::PIX_NV12>(p, recs[f], f, out);
        else if (recs[f].format == vp::PIX_RGB24) host_image<vp::PIX_RGB24>(p, recs[f], f, out);
        else host_image<vp::PIX_BGR24>(p, recs[f], f, out);
    }
    return VP_OK;
}

}  // extern "C"
