// vp_draw_poses_stream: the skeleton overlay on device frames (semantics: drawgeom.h), its synchronous host twin vp_draw_poses and the host-only tap
// vp_dbg_draw_host.  A gather: every pixel looks up the last primitive in draw order that covers it.  No atomics and no scatter, so the picture is a pure function
// of the inputs whatever the launch shape.
#include "api_internal.h"
#include "hoststage.h"
#include "drawgeom.h"

using namespace vpi;

namespace vp {

constexpr int DRAW_THREADS = 256, DRAW_WAVES = DRAW_THREADS / 64;
constexpr int DRAW_TILE_W = 32, DRAW_TILE_H = 8;   // both even: a chroma sample never straddles two workgroups
constexpr int DRAW_LIST = 256;                     // hits a workgroup holds in LDS before it resolves them (>= DRAW_THREADS: a chunk's hits always fit an empty list)
constexpr int DRAW_FRAMES_PER_LAUNCH = 32;

struct DrawFrame {   // vp_image's fields, the planes writable
    uint8_t* plane[2];
    int64_t pitch[2];
    int32_t h, w, format, matrix;
};
struct DrawFrames {   // frames [f0, f0 + count) of the table, by kernel argument; tile0[g] = the first workgroup of frame f0 + g
    DrawFrame fr[DRAW_FRAMES_PER_LAUNCH];
    int32_t tile0[DRAW_FRAMES_PER_LAUNCH + 1];
    int32_t f0, count;
};

// One thread per primitive slot of the call (row-major: row, then box / limbs / joints): the gates and the record, one writer per record.  A row of a frame outside
// [f0, f0 + count) -- another launch's, or no frame of the table -- leaves empty records.
__global__ __launch_bounds__(DRAW_THREADS) void draw_prims_kernel(const float* __restrict__ kpts, int n, int K, const int32_t* __restrict__ frame_idx, int frame_stride,
                                                                  const int32_t* __restrict__ rank, const int32_t* __restrict__ ids, const float* __restrict__ boxes,
                                                                  int box_stride, DrawFrames fr, DrawStyle st, DrawKey* __restrict__ keys, DrawBody* __restrict__ bodies) {
    const int S = (boxes ? 1 : 0) + st.n_limbs + K;
    const int t = blockIdx.x * DRAW_THREADS + threadIdx.x;
    if (t >= n * S) return;
    const int i = t / S, s = t - i * S;
    const int32_t f = frame_idx[(size_t)i * frame_stride];
    DrawKey key{1, 1, 0, 0, f, DRAW_EMPTY};
    DrawBody body{DRAW_EMPTY, f, 0, 0, 0, 0, 0, 0};
    if (f >= fr.f0 && f < fr.f0 + fr.count && !(rank && rank[i] < 0)) {
        const DrawFrame& F = fr.fr[f - fr.f0];
        const DrawRow row{kpts + (size_t)i * K * 3, boxes ? boxes + (size_t)i * box_stride : nullptr, ids ? ids[i] : i, f, F.h, F.w, F.format, F.matrix};
        draw_primitive(row, K, st, s, &key, &body);
    }
    keys[t] = key;
    bodies[t] = body;
}

// One workgroup per 32 x 8 tile of a frame, one thread per pixel.  The workgroup walks the call's records in order in chunks of 256: a thread tests one record's frame
// and bounding box against the tile, the hits are compacted into the LDS list in record order (ballot prefix per wave, wave counts through LDS); when the next chunk's
// hits would not fit, the list is resolved first -- every thread walks it from the back and keeps the first record that covers its pixel, a later list overrides an
// earlier one -- so the picture does not depend on the list's capacity.  NV12: Y per pixel, then the tile's 16 x 4 chroma samples take the colour of the highest
// record among their pixels.  A tile without a hit writes nothing.
__global__ __launch_bounds__(DRAW_THREADS) void draw_raster_kernel(DrawFrames fr, const DrawKey* __restrict__ keys, const DrawBody* __restrict__ bodies, int n_rec) {
    __shared__ DrawBody s_body[DRAW_LIST];
    __shared__ int32_t s_idx[DRAW_LIST];
    __shared__ int32_t s_wcnt[DRAW_WAVES];
    __shared__ int32_t s_win[DRAW_THREADS], s_col[DRAW_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int g = 0;
    for (int q = 1; q < fr.count; ++q)
        if ((int)blockIdx.x >= fr.tile0[q]) g = q;
    const int h = fr.fr[g].h, w = fr.fr[g].w, format = fr.fr[g].format, f = fr.f0 + g;
    const int tiles_x = (w + DRAW_TILE_W - 1) / DRAW_TILE_W, lt = (int)blockIdx.x - fr.tile0[g];
    const int tx0 = (lt % tiles_x) * DRAW_TILE_W, ty0 = (lt / tiles_x) * DRAW_TILE_H;
    const int px = tx0 + (tid & (DRAW_TILE_W - 1)), py = ty0 + tid / DRAW_TILE_W;
    const bool inside = px < w && py < h;

    int32_t win = -1, col = 0;
    auto resolve = [&](int cnt) {
        if (!inside) return;
        for (int m = cnt - 1; m >= 0; --m)
            if (draw_covers(s_body[m], px, py)) { win = s_idx[m]; col = s_body[m].color; break; }
    };
    int cnt = 0;   // uniform over the workgroup
    for (int base = 0; base < n_rec; base += DRAW_THREADS) {
        const int i = base + tid;
        bool hit = false;
        if (i < n_rec) {
            const DrawKey k = keys[i];
            hit = k.frame == f && k.x0 <= k.x1 && k.x0 < tx0 + DRAW_TILE_W && k.x1 >= tx0 && k.y0 < ty0 + DRAW_TILE_H && k.y1 >= ty0;
        }
        const unsigned long long b = __ballot(hit);
        if (lane == 0) s_wcnt[wave] = __popcll(b);
        __syncthreads();
        int off = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
        for (int q = 0; q < DRAW_WAVES; ++q) {
            if (q < wave) off += s_wcnt[q];
            all += s_wcnt[q];
        }
        if (cnt + all > DRAW_LIST) {   // uniform
            resolve(cnt);
            cnt = 0;
            __syncthreads();
        }
        if (hit) {
            s_body[cnt + off] = bodies[i];
            s_idx[cnt + off] = i;
        }
        cnt += all;
        __syncthreads();
    }
    resolve(cnt);

    const DrawFrame& F = fr.fr[g];
    if (format != PIX_NV12) {
        if (win >= 0) {
            uint8_t* p = F.plane[0] + (int64_t)py * F.pitch[0] + 3 * px;
            p[0] = (uint8_t)col; p[1] = (uint8_t)(col >> 8); p[2] = (uint8_t)(col >> 16);
        }
        return;
    }
    if (win >= 0) F.plane[0][(int64_t)py * F.pitch[0] + px] = (uint8_t)col;
    s_win[tid] = win;
    s_col[tid] = col;
    __syncthreads();
    if (tid < (DRAW_TILE_W / 2) * (DRAW_TILE_H / 2)) {
        const int cx = tid % (DRAW_TILE_W / 2), cy = tid / (DRAW_TILE_W / 2);
        int32_t bw = -1, bc = 0;
        for (int q = 0; q < 4; ++q) {
            const int m = (2 * cy + (q >> 1)) * DRAW_TILE_W + 2 * cx + (q & 1);
            if (s_win[m] > bw) { bw = s_win[m]; bc = s_col[m]; }
        }
        if (bw >= 0) {   // one of its pixels lies on the frame, so the sample does
            uint8_t* p = F.plane[1] + (int64_t)(ty0 / 2 + cy) * F.pitch[1] + 2 * (tx0 / 2 + cx);
            p[0] = (uint8_t)(bc >> 8); p[1] = (uint8_t)(bc >> 16);
        }
    }
}

}  // namespace vp

namespace {

struct DrawCall {   // the checked arguments of a call
    vp::DrawStyle st;
    int slots = 0;   // per row
};

// every refusal of the three entries (HOST ONLY), before anything is enqueued; fills the style the kernels take
int draw_args(bool need_ptrs, const vp_image* images, int n_images, int n, int k, int frame_stride, bool has_box, int box_stride, const vp_draw_cfg* cfg, DrawCall& dc,
              std::string* why) {
    auto bad = [&](const std::string& m) { *why = "draw: " + m; return (int)VP_ERR_INVALID; };
    if (!cfg) return bad("null cfg");
    if (n < 0) return bad("negative n");
    if (n_images < 0) return bad("negative n_images");
    if (n > 0 && !need_ptrs) return bad("null image table, keypoint or frame index pointer");
    if (k < 1 || k > vp::DRAW_MAX_K) return bad("k = " + std::to_string(k) + " outside 1.." + std::to_string(vp::DRAW_MAX_K));
    if (cfg->n_limbs < 0 || cfg->n_limbs > VP_DRAW_MAX_LIMBS) return bad("n_limbs = " + std::to_string(cfg->n_limbs) + " outside 0.." + std::to_string(VP_DRAW_MAX_LIMBS));
    if (cfg->n_limbs > 0 && !cfg->limbs) return bad("null limb table");
    for (int l = 0; l < 2 * cfg->n_limbs; ++l)
        if (cfg->limbs[l] >= k) return bad("limb " + std::to_string(l / 2) + " names joint " + std::to_string(cfg->limbs[l]) + " of " + std::to_string(k));
    if (cfg->n_point_colors < 1 || cfg->n_point_colors > VP_DRAW_MAX_COLORS || cfg->n_limb_colors < 1 || cfg->n_limb_colors > VP_DRAW_MAX_COLORS)
        return bad("colour counts outside 1.." + std::to_string(VP_DRAW_MAX_COLORS));
    if (!cfg->point_colors || !cfg->limb_colors) return bad("null colour table");
    if (!std::isfinite(cfg->conf_thr)) return bad("conf_thr is not finite");
    if (cfg->radius < 0 || cfg->radius > vp::DRAW_MAX_RADIUS) return bad("radius = " + std::to_string(cfg->radius) + " outside 0.." + std::to_string(vp::DRAW_MAX_RADIUS));
    if (cfg->thickness < 1 || cfg->thickness > vp::DRAW_MAX_THICKNESS)
        return bad("thickness = " + std::to_string(cfg->thickness) + " outside 1.." + std::to_string(vp::DRAW_MAX_THICKNESS));
    if (frame_stride < 1 || (has_box && box_stride < 1)) return bad("a stride < 1");
    dc.slots = (has_box ? 1 : 0) + cfg->n_limbs + k;
    if ((int64_t)n * dc.slots > VP_DRAW_MAX_RECORDS)
        return bad("n = " + std::to_string(n) + " rows of " + std::to_string(dc.slots) + " primitives exceed the " + std::to_string(VP_DRAW_MAX_RECORDS) + " records of the workspace");
    if (n > 0 && n_images < 1) return bad("n > 0 with n_images < 1");
    for (int f = 0; f < n_images && n > 0; ++f) {
        const vp_image& im = images[f];
        const std::string at = "frame " + std::to_string(f);
        if (!im.plane[0]) return bad(at + " has no data");
        if (im.h <= 0 || im.w <= 0) return bad(at + " has a non-positive size");
        if (im.h > vp::DRAW_MAX_DIM || im.w > vp::DRAW_MAX_DIM) return bad(at + " is larger than " + std::to_string(vp::DRAW_MAX_DIM) + " in h or w");
        std::string w;
        if (image_check(im, f, &w)) return bad(w);
    }
    vp::DrawStyle& st = dc.st;
    std::memset(&st, 0, sizeof(st));
    st.conf_thr = cfg->conf_thr; st.radius = cfg->radius; st.thickness = cfg->thickness; st.n_limbs = cfg->n_limbs;
    st.n_point_colors = cfg->n_point_colors; st.n_limb_colors = cfg->n_limb_colors;
    if (cfg->n_limbs) std::memcpy(st.limbs, cfg->limbs, (size_t)cfg->n_limbs * 2);
    std::memcpy(st.point_colors, cfg->point_colors, (size_t)cfg->n_point_colors * 3);
    std::memcpy(st.limb_colors, cfg->limb_colors, (size_t)cfg->n_limb_colors * 3);
    return VP_OK;
}

// frame f read and written in place: every plane device memory of the handle's device, inside one allocation (the check of the boxes entries)
int check_device_image(vp_ctx* c, const vp_image& im, int f) {
    bool ok = true;
    for (int p = 0; p < plane_count(im) && ok; ++p) ok = device_range_ok(c, im.plane[p], plane_bytes(im, p));
    if (ok) return VP_OK;
    (void)hipGetLastError();
    return fail(c, VP_ERR_INVALID, "draw: frame " + std::to_string(f) + " is not device memory of device " + std::to_string(c->cfg.device_id) +
                                       " (or runs past the end of its allocation)");
}

// the checked call on stream s, launches only: per 32 frames of the table the records of their rows, then their tiles
int draw_enqueue(vp_ctx* c, const vp_image* d_images, int n_images, const float* d_kpts, int n, int k, const int32_t* d_frame_idx, int frame_stride, const int32_t* d_rank,
                 const int32_t* d_ids, const float* d_boxes, int box_stride, const DrawCall& dc, hipStream_t s) {
    const int n_rec = n * dc.slots;
    vp::DrawKey* keys = (vp::DrawKey*)c->draw_ws;
    vp::DrawBody* bodies = (vp::DrawBody*)((char*)c->draw_ws + (size_t)VP_DRAW_MAX_RECORDS * sizeof(vp::DrawKey));
    for (int f0 = 0; f0 < n_images; f0 += vp::DRAW_FRAMES_PER_LAUNCH) {
        vp::DrawFrames fr;
        std::memset(&fr, 0, sizeof(fr));
        fr.f0 = f0; fr.count = std::min(n_images - f0, vp::DRAW_FRAMES_PER_LAUNCH);
        for (int g = 0; g < fr.count; ++g) {
            const vp_image& im = d_images[f0 + g];
            fr.fr[g] = vp::DrawFrame{{const_cast<uint8_t*>(im.plane[0]), const_cast<uint8_t*>(im.plane[1])}, {im.pitch[0], im.pitch[1]}, im.h, im.w, im.format, im.matrix};
            fr.tile0[g + 1] = fr.tile0[g] + ((im.w + vp::DRAW_TILE_W - 1) / vp::DRAW_TILE_W) * ((im.h + vp::DRAW_TILE_H - 1) / vp::DRAW_TILE_H);
        }
        hipLaunchKernelGGL(vp::draw_prims_kernel, dim3((n_rec + vp::DRAW_THREADS - 1) / vp::DRAW_THREADS), dim3(vp::DRAW_THREADS), 0, s, d_kpts, n, k, d_frame_idx,
                           frame_stride, d_rank, d_ids, d_boxes, box_stride, fr, dc.st, keys, bodies);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(vp::draw_raster_kernel, dim3(fr.tile0[fr.count]), dim3(vp::DRAW_THREADS), 0, s, fr, keys, bodies, n_rec);
        HIPCHK(c, hipGetLastError());
    }
    return VP_OK;
}

// drawgeom.h on host planes, record by record in draw order (a later record overwrites an earlier one: the last one that covers a pixel or a chroma sample stays)
void draw_host(const vp_image* images, int n_images, const float* kpts, int n, int k, const int32_t* frame_idx, int frame_stride, const int32_t* rank, const int32_t* ids,
               const float* boxes, int box_stride, const DrawCall& dc) {
    for (int i = 0; i < n; ++i) {
        const int32_t f = frame_idx[(size_t)i * frame_stride];
        if (f < 0 || f >= n_images || (rank && rank[i] < 0)) continue;
        const vp_image& im = images[f];
        const vp::DrawRow row{kpts + (size_t)i * k * 3, boxes ? boxes + (size_t)i * box_stride : nullptr, ids ? ids[i] : i, f, im.h, im.w, im.format, im.matrix};
        for (int s = 0; s < dc.slots; ++s) {
            vp::DrawKey key;
            vp::DrawBody b;
            vp::draw_primitive(row, k, dc.st, s, &key, &b);
            for (int py = key.y0; py <= key.y1; ++py)
                for (int px = key.x0; px <= key.x1; ++px) {   // (an empty slot: y0 > y1)
                    if (!vp::draw_covers(b, px, py)) continue;
                    if (im.format == vp::PIX_NV12) {
                        const_cast<uint8_t*>(im.plane[0])[(int64_t)py * im.pitch[0] + px] = (uint8_t)b.color;
                        uint8_t* q = const_cast<uint8_t*>(im.plane[1]) + (int64_t)(py >> 1) * im.pitch[1] + 2 * (px >> 1);
                        q[0] = (uint8_t)(b.color >> 8); q[1] = (uint8_t)(b.color >> 16);
                    } else {
                        uint8_t* q = const_cast<uint8_t*>(im.plane[0]) + (int64_t)py * im.pitch[0] + 3 * px;
                        q[0] = (uint8_t)b.color; q[1] = (uint8_t)(b.color >> 8); q[2] = (uint8_t)(b.color >> 16);
                    }
                }
        }
    }
}

}  // namespace

extern "C" {

int vp_draw_poses_stream(vp_handle c, const vp_image* images, int32_t n_images, const float* d_kpts, int32_t n, int32_t k, const int32_t* d_frame_idx, int32_t frame_stride,
                         const int32_t* d_rank, const int32_t* d_ids, const float* d_boxes, int32_t box_stride, const vp_draw_cfg* cfg, void* caller_stream) {
    if (!c) return VP_ERR_INVALID;
    DrawCall dc;
    std::string why;
    if (draw_args(images && d_kpts && d_frame_idx, images, n_images, n, k, frame_stride, d_boxes != nullptr, box_stride, cfg, dc, &why)) return fail(c, VP_ERR_INVALID, why);
    if (n == 0) return VP_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    for (int f = 0; f < n_images; ++f)
        if (const int rc = check_device_image(c, images[f], f)) return rc;
    return draw_enqueue(c, images, n_images, d_kpts, n, k, d_frame_idx, frame_stride, d_rank, d_ids, d_boxes, box_stride, dc, (hipStream_t)caller_stream);
}

int vp_draw_poses(vp_handle c, const vp_image* images, int32_t n_images, const float* kpts, int32_t n, int32_t k, const int32_t* frame_idx, int32_t frame_stride,
                  const int32_t* rank, const int32_t* ids, const float* boxes, int32_t box_stride, const vp_draw_cfg* cfg) {
    if (!c) return VP_ERR_INVALID;
    DrawCall dc;
    std::string why;
    if (draw_args(images && kpts && frame_idx, images, n_images, n, k, frame_stride, boxes != nullptr, box_stride, cfg, dc, &why)) return fail(c, VP_ERR_INVALID, why);
    if (n == 0) return VP_OK;
    // one scratch block: the planes of every frame | keypoints | frame index | rank | ids | boxes
    HostStage st(c);
    const size_t kp_bytes = (size_t)n * k * 12, fi_bytes = ((size_t)(n - 1) * frame_stride + 1) * 4, nb = (size_t)n * 4, bx_bytes = ((size_t)(n - 1) * box_stride + 4) * 4;
    std::vector<size_t> o_pl;
    for (int f = 0; f < n_images; ++f)
        for (int p = 0; p < plane_count(images[f]); ++p) o_pl.push_back(st.part(plane_bytes(images[f], p)));
    const size_t o_kp = st.part(kp_bytes), o_fi = st.part(fi_bytes), o_rk = st.part(nb), o_id = st.part(nb), o_bx = boxes ? st.part(bx_bytes) : 0;
    if (st.alloc()) return st.rc;
    std::vector<vp_image> dev(images, images + n_images);
    for (int f = 0, i = 0; f < n_images; ++f)
        for (int p = 0; p < plane_count(images[f]); ++p, ++i) {
            dev[f].plane[p] = st.at<uint8_t>(o_pl[i]);
            if (images[f].plane[p]) st.up(st.at(o_pl[i]), images[f].plane[p], plane_bytes(images[f], p), "upload frame");
        }
    const float *d_kp = st.at<float>(o_kp), *d_bx = boxes ? st.at<float>(o_bx) : nullptr;
    const int32_t *d_fi = st.at<int32_t>(o_fi), *d_rk = st.at<int32_t>(o_rk), *d_id = st.at<int32_t>(o_id);
    st.up(st.at(o_kp), kpts, kp_bytes, "upload keypoints");
    st.up(st.at(o_fi), frame_idx, fi_bytes, "upload frame index");
    if (rank) st.up(st.at(o_rk), rank, nb, "upload rank");
    if (ids) st.up(st.at(o_id), ids, nb, "upload ids");
    if (boxes) st.up(st.at(o_bx), boxes, bx_bytes, "upload boxes");
    if (!st.rc) st.rc = draw_enqueue(c, dev.data(), n_images, d_kp, n, k, d_fi, frame_stride, rank ? d_rk : nullptr, ids ? d_id : nullptr, d_bx, box_stride, dc, st.s);
    for (int f = 0; f < n_images && !st.rc; ++f)   // the frames are written back in place
        for (int p = 0; p < plane_count(images[f]); ++p)
            st.down(const_cast<uint8_t*>(images[f].plane[p]), dev[f].plane[p], plane_bytes(images[f], p), "download frame");
    st.sync();
    return st.rc;
}

int vp_dbg_draw_host(const vp_image* images, int32_t n_images, const float* kpts, int32_t n, int32_t k, const int32_t* frame_idx, int32_t frame_stride, const int32_t* rank,
                     const int32_t* ids, const float* boxes, int32_t box_stride, const vp_draw_cfg* cfg) {
    DrawCall dc;
    std::string why;
    if (draw_args(images && kpts && frame_idx, images, n_images, n, k, frame_stride, boxes != nullptr, box_stride, cfg, dc, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    draw_host(images, n_images, kpts, n, k, frame_idx, frame_stride, rank, ids, boxes, box_stride, dc);
    return VP_OK;
}

}  // extern "C"
