// vp_draw_labels_stream: the track-id / score tags on device frames, the stage in front of the skeleton overlay (semantics: labelgeom.h), its synchronous host twin
// vp_draw_labels and the host-only taps vp_dbg_draw_labels_host, vp_dbg_label_text and vp_dbg_label_glyph.  A gather: a pixel is written by the one workgroup whose
// row is the last that covers it.  No atomics and no scatter, so the picture is a pure function of the inputs whatever the launch shape.
#include "api_internal.h"
#include "hoststage.h"
#include "labelgeom.h"

using namespace vpi;

namespace vp {

constexpr int LABEL_THREADS = 256, LABEL_WAVES = LABEL_THREADS / 64;
constexpr int LABEL_TILE_W = 32, LABEL_TILE_H = 8;   // both even and frame-aligned: a chroma sample never straddles two tiles
constexpr int LABEL_FRAMES_PER_LAUNCH = 32;

struct LabelFrame {   // vp_image's fields, the planes writable
    uint8_t* plane[2];
    int64_t pitch[2];
    int32_t h, w, format, matrix;
};
struct LabelFrames {   // frames [f0, f0 + count) of the table, by kernel argument
    LabelFrame fr[LABEL_FRAMES_PER_LAUNCH];
    int32_t f0, count;
};

// the frame-aligned tiles a span [lo, hi] of pixels touches
__host__ __device__ inline int label_tiles(int lo, int hi, int tile) { return hi / tile - lo / tile + 1; }

// One thread per row of the call: the gates, the text and the record, one writer per record.  A row of a frame outside [f0, f0 + count) -- another launch's, or no
// frame of the table -- leaves an empty record.
__global__ __launch_bounds__(LABEL_THREADS) void label_rows_kernel(const float* __restrict__ boxes, int box_stride, int n, const int32_t* __restrict__ frame_idx,
                                                                   int frame_stride, const int32_t* __restrict__ rank, const int32_t* __restrict__ ids,
                                                                   const float* __restrict__ scores, int score_stride, LabelFrames fr, LabelStyle st,
                                                                   LabelRec* __restrict__ recs) {
    const int i = blockIdx.x * LABEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t f = frame_idx[(size_t)i * frame_stride];
    LabelRec rec;
    if (f >= fr.f0 && f < fr.f0 + fr.count && !(rank && rank[i] < 0)) {
        const LabelFrame& F = fr.fr[f - fr.f0];
        const LabelRow row{boxes + (size_t)i * box_stride, ids ? ids[i] : i, scores ? 1 : 0, scores ? scores[(size_t)i * score_stride] : 0.f, f, F.h, F.w, F.format, F.matrix};
        label_record(row, st, &rec);
    } else {
        rec = LabelRec{};
        rec.x0 = rec.y0 = 1;
        rec.frame = f;
    }
    recs[i] = rec;
}

// One workgroup per (row, frame-aligned 32 x 8 tile of the row's clipped block), one thread per pixel: blockIdx.y is the row, blockIdx.x the tile of its block in
// row-major order (the grid holds the most tiles a block of this launch can touch; a workgroup beyond its row's count returns).  A thread finds what its row puts on
// its pixel (nothing, background, ink), then the workgroup walks the LATER records in chunks of 256: a thread tests one record's frame and bounding box against
// the tile, the waves' ballots go through LDS, and every thread tests its pixel against the records that hit -- few, and the same for every lane.  A thread writes
// its pixel only if no later record covers it.  NV12: a chroma sample is written by this workgroup iff no later record covers any of its
// pixels and this row covers one of them: it then owns the sample's highest order index, and the sample is ink iff one of those pixels is.  One writer per byte.
__global__ __launch_bounds__(LABEL_THREADS) void label_raster_kernel(LabelFrames fr, LabelStyle st, const LabelRec* __restrict__ recs, int n) {
    __shared__ int8_t s_mine[LABEL_THREADS], s_later[LABEL_THREADS];
    __shared__ unsigned long long s_mask[LABEL_WAVES];
    const int tid = threadIdx.x, row = blockIdx.y;
    const LabelRec rec = recs[row];
    if (rec.x0 > rec.x1 || rec.frame < fr.f0 || rec.frame >= fr.f0 + fr.count) return;   // uniform
    const int tiles_x = label_tiles(rec.x0, rec.x1, LABEL_TILE_W), tiles_y = label_tiles(rec.y0, rec.y1, LABEL_TILE_H);
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;   // uniform
    const LabelFrame& F = fr.fr[rec.frame - fr.f0];
    const int tx0 = (rec.x0 / LABEL_TILE_W + (int)blockIdx.x % tiles_x) * LABEL_TILE_W, ty0 = (rec.y0 / LABEL_TILE_H + (int)blockIdx.x / tiles_x) * LABEL_TILE_H;
    const int px = tx0 + (tid & (LABEL_TILE_W - 1)), py = ty0 + tid / LABEL_TILE_W;
    const int mine = label_cover(rec, st.font, px, py);   // 0 outside the block, so outside the frame too
    bool later = false;
    for (int base = row + 1; base < n; base += LABEL_THREADS) {   // uniform bounds: every thread of the workgroup reaches both barriers
        const int j = base + tid;
        bool hit = false;
        if (j < n) {
            const LabelRec& o = recs[j];
            hit = o.frame == rec.frame && o.x0 <= o.x1 && o.x0 < tx0 + LABEL_TILE_W && o.x1 >= tx0 && o.y0 < ty0 + LABEL_TILE_H && o.y1 >= ty0;
        }
        const unsigned long long b = __ballot(hit);
        if ((tid & 63) == 0) s_mask[tid >> 6] = b;
        __syncthreads();
        for (int q = 0; q < LABEL_WAVES; ++q) {
            const unsigned long long v = s_mask[q];
            unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
            while (m) {   // the records of this chunk that touch the tile: few, and the same for every lane
                const LabelRec& o = recs[base + 64 * q + __builtin_ctzll(m)];
                m &= m - 1;
                later = later || (px >= o.x0 && px <= o.x1 && py >= o.y0 && py <= o.y1);
            }
        }
        __syncthreads();   // s_mask is rewritten by the next chunk
    }
    const int32_t col = mine == 2 ? rec.ink : rec.bg;
    if (F.format != PIX_NV12) {
        if (mine && !later) {
            uint8_t* p = F.plane[0] + (int64_t)py * F.pitch[0] + 3 * px;
            p[0] = (uint8_t)col; p[1] = (uint8_t)(col >> 8); p[2] = (uint8_t)(col >> 16);
        }
        return;
    }
    if (mine && !later) F.plane[0][(int64_t)py * F.pitch[0] + px] = (uint8_t)col;
    s_mine[tid] = (int8_t)mine;
    s_later[tid] = later ? 1 : 0;
    __syncthreads();
    if (tid < (LABEL_TILE_W / 2) * (LABEL_TILE_H / 2)) {
        const int cx = tid % (LABEL_TILE_W / 2), cy = tid / (LABEL_TILE_W / 2);
        int best = 0, lat = 0;
        for (int q = 0; q < 4; ++q) {
            const int m = (2 * cy + (q >> 1)) * LABEL_TILE_W + 2 * cx + (q & 1);
            best = s_mine[m] > best ? s_mine[m] : best;
            lat |= s_later[m];
        }
        if (best && !lat) {   // one of its pixels lies in the clipped block, so the sample lies on the frame
            const int32_t cc = best == 2 ? rec.ink : rec.bg;
            uint8_t* p = F.plane[1] + (int64_t)(ty0 / 2 + cy) * F.pitch[1] + 2 * (tx0 / 2 + cx);
            p[0] = (uint8_t)(cc >> 8); p[1] = (uint8_t)(cc >> 16);
        }
    }
}

}  // namespace vp

namespace {

// every refusal of the three entries (HOST ONLY), before anything is enqueued; fills the style the kernels take
int label_args(bool need_ptrs, const vp_image* images, int n_images, int n, int box_stride, int frame_stride, bool has_scores, int score_stride, const vp_label_cfg* cfg,
               vp::LabelStyle& st, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "labels: " + m; return (int)VP_ERR_INVALID; };
    if (!cfg) return bad("null cfg");
    if (n < 0) return bad("negative n");
    if (n > VP_LABEL_MAX_ROWS) return bad("n = " + std::to_string(n) + " rows exceed the " + std::to_string(VP_LABEL_MAX_ROWS) + " records of the workspace");
    if (n_images < 0) return bad("negative n_images");
    if (n > 0 && !need_ptrs) return bad("null image table, box or frame index pointer (labels need boxes)");
    if (cfg->scale < 0 || cfg->scale > vp::LABEL_MAX_SCALE) return bad("scale = " + std::to_string(cfg->scale) + " outside 0.." + std::to_string(vp::LABEL_MAX_SCALE));
    if (cfg->n_colors < 1 || cfg->n_colors > VP_DRAW_MAX_COLORS) return bad("colour count outside 1.." + std::to_string(VP_DRAW_MAX_COLORS));
    if (!cfg->colors) return bad("null colour table");
    if (box_stride < 1 || frame_stride < 1 || (has_scores && score_stride < 1)) return bad("a stride < 1");
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
    std::memset(&st, 0, sizeof(st));
    st.scale = cfg->scale; st.n_colors = cfg->n_colors; st.auto_ink = cfg->auto_ink ? 1 : 0; st.show_score = cfg->show_score ? 1 : 0;
    std::memcpy(st.colors, cfg->colors, (size_t)cfg->n_colors * 3);
    std::memcpy(st.ink, cfg->ink, 3);
    for (int g = 0; g < vp::LABEL_GLYPHS; ++g) st.font[g] = vp::label_glyph(g);
    return VP_OK;
}

// frame f read and written in place: every plane device memory of the handle's device, inside one allocation (the check of vp_draw_poses_stream)
int check_device_image(vp_ctx* c, const vp_image& im, int f) {
    bool ok = true;
    for (int p = 0; p < plane_count(im) && ok; ++p) ok = device_range_ok(c, im.plane[p], plane_bytes(im, p));
    if (ok) return VP_OK;
    (void)hipGetLastError();
    return fail(c, VP_ERR_INVALID, "labels: frame " + std::to_string(f) + " is not device memory of device " + std::to_string(c->cfg.device_id) +
                                       " (or runs past the end of its allocation)");
}

// the checked call on stream s, launches only: per 32 frames of the table the records of their rows, then the tiles of their blocks
int label_enqueue(vp_ctx* c, const vp_image* d_images, int n_images, const float* d_boxes, int box_stride, int n, const int32_t* d_frame_idx, int frame_stride,
                  const int32_t* d_rank, const int32_t* d_ids, const float* d_scores, int score_stride, const vp::LabelStyle& st, hipStream_t s) {
    vp::LabelRec* recs = (vp::LabelRec*)c->label_ws;
    for (int f0 = 0; f0 < n_images; f0 += vp::LABEL_FRAMES_PER_LAUNCH) {
        vp::LabelFrames fr;
        std::memset(&fr, 0, sizeof(fr));
        fr.f0 = f0; fr.count = std::min(n_images - f0, vp::LABEL_FRAMES_PER_LAUNCH);
        int tiles = 1;   // the most tiles the block of a row of these frames can touch: the widest text at the frame's scale, at the worst alignment, clipped to the frame
        for (int g = 0; g < fr.count; ++g) {
            const vp_image& im = d_images[f0 + g];
            fr.fr[g] = vp::LabelFrame{{const_cast<uint8_t*>(im.plane[0]), const_cast<uint8_t*>(im.plane[1])}, {im.pitch[0], im.pitch[1]}, im.h, im.w, im.format, im.matrix};
            const int sc = vp::label_scale(st.scale, im.h, im.w), bw = sc * (6 * vp::LABEL_MAX_TEXT + 1), bh = 9 * sc;
            const int tx = std::min((bw - 2) / vp::LABEL_TILE_W + 2, (im.w + vp::LABEL_TILE_W - 1) / vp::LABEL_TILE_W);
            const int ty = std::min((bh - 2) / vp::LABEL_TILE_H + 2, (im.h + vp::LABEL_TILE_H - 1) / vp::LABEL_TILE_H);
            tiles = std::max(tiles, tx * ty);
        }
        hipLaunchKernelGGL(vp::label_rows_kernel, dim3((n + vp::LABEL_THREADS - 1) / vp::LABEL_THREADS), dim3(vp::LABEL_THREADS), 0, s, d_boxes, box_stride, n, d_frame_idx,
                           frame_stride, d_rank, d_ids, d_scores, score_stride, fr, st, recs);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(vp::label_raster_kernel, dim3(tiles, n), dim3(vp::LABEL_THREADS), 0, s, fr, st, recs, n);
        HIPCHK(c, hipGetLastError());
    }
    return VP_OK;
}

// labelgeom.h on host planes, row by row in order, the background of a row before its ink (a later primitive overwrites an earlier one: the one with the highest
// order index that covers a pixel or a chroma sample stays)
void label_host(const vp_image* images, int n_images, const float* boxes, int box_stride, int n, const int32_t* frame_idx, int frame_stride, const int32_t* rank,
                const int32_t* ids, const float* scores, int score_stride, const vp::LabelStyle& st) {
    for (int i = 0; i < n; ++i) {
        const int32_t f = frame_idx[(size_t)i * frame_stride];
        if (f < 0 || f >= n_images || (rank && rank[i] < 0)) continue;
        const vp_image& im = images[f];
        const vp::LabelRow row{boxes + (size_t)i * box_stride, ids ? ids[i] : i, scores ? 1 : 0, scores ? scores[(size_t)i * score_stride] : 0.f, f, im.h, im.w, im.format, im.matrix};
        vp::LabelRec rec;
        vp::label_record(row, st, &rec);
        for (int pass = 1; pass <= 2; ++pass)
            for (int py = rec.y0; py <= rec.y1; ++py)
                for (int px = rec.x0; px <= rec.x1; ++px) {   // (an empty record: y0 > y1)
                    if (vp::label_cover(rec, st.font, px, py) < pass) continue;   // pass 1: the whole block in the background colour; pass 2: the ink
                    const int32_t col = pass == 2 ? rec.ink : rec.bg;
                    if (im.format == vp::PIX_NV12) {
                        const_cast<uint8_t*>(im.plane[0])[(int64_t)py * im.pitch[0] + px] = (uint8_t)col;
                        uint8_t* q = const_cast<uint8_t*>(im.plane[1]) + (int64_t)(py >> 1) * im.pitch[1] + 2 * (px >> 1);
                        q[0] = (uint8_t)(col >> 8); q[1] = (uint8_t)(col >> 16);
                    } else {
                        uint8_t* q = const_cast<uint8_t*>(im.plane[0]) + (int64_t)py * im.pitch[0] + 3 * px;
                        q[0] = (uint8_t)col; q[1] = (uint8_t)(col >> 8); q[2] = (uint8_t)(col >> 16);
                    }
                }
    }
}

const char LABEL_CHARS[17] = "#0123456789:.- ?";

}  // namespace

extern "C" {

int vp_draw_labels_stream(vp_handle c, const vp_image* images, int32_t n_images, const float* d_boxes, int32_t box_stride, int32_t n, const int32_t* d_frame_idx,
                          int32_t frame_stride, const int32_t* d_rank, const int32_t* d_ids, const float* d_scores, int32_t score_stride, const vp_label_cfg* cfg,
                          void* caller_stream) {
    if (!c) return VP_ERR_INVALID;
    vp::LabelStyle st;
    std::string why;
    if (label_args(images && d_boxes && d_frame_idx, images, n_images, n, box_stride, frame_stride, d_scores != nullptr, score_stride, cfg, st, &why))
        return fail(c, VP_ERR_INVALID, why);
    if (n == 0) return VP_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    for (int f = 0; f < n_images; ++f)
        if (const int rc = check_device_image(c, images[f], f)) return rc;
    return label_enqueue(c, images, n_images, d_boxes, box_stride, n, d_frame_idx, frame_stride, d_rank, d_ids, d_scores, score_stride, st, (hipStream_t)caller_stream);
}

int vp_draw_labels(vp_handle c, const vp_image* images, int32_t n_images, const float* boxes, int32_t box_stride, int32_t n, const int32_t* frame_idx, int32_t frame_stride,
                   const int32_t* rank, const int32_t* ids, const float* scores, int32_t score_stride, const vp_label_cfg* cfg) {
    if (!c) return VP_ERR_INVALID;
    vp::LabelStyle st;
    std::string why;
    if (label_args(images && boxes && frame_idx, images, n_images, n, box_stride, frame_stride, scores != nullptr, score_stride, cfg, st, &why))
        return fail(c, VP_ERR_INVALID, why);
    if (n == 0) return VP_OK;
    // one scratch block: the planes of every frame | boxes | frame index | rank | ids | scores
    HostStage hs(c);
    const size_t bx_bytes = ((size_t)(n - 1) * box_stride + 4) * 4, fi_bytes = ((size_t)(n - 1) * frame_stride + 1) * 4, nb = (size_t)n * 4, sc_bytes = ((size_t)(n - 1) * score_stride + 1) * 4;
    std::vector<size_t> o_pl;
    for (int f = 0; f < n_images; ++f)
        for (int p = 0; p < plane_count(images[f]); ++p) o_pl.push_back(hs.part(plane_bytes(images[f], p)));
    const size_t o_bx = hs.part(bx_bytes), o_fi = hs.part(fi_bytes), o_rk = hs.part(nb), o_id = hs.part(nb), o_sc = scores ? hs.part(sc_bytes) : 0;
    if (hs.alloc()) return hs.rc;
    std::vector<vp_image> dev(images, images + n_images);
    for (int f = 0, i = 0; f < n_images; ++f)
        for (int p = 0; p < plane_count(images[f]); ++p, ++i) {
            dev[f].plane[p] = hs.at<uint8_t>(o_pl[i]);
            if (images[f].plane[p]) hs.up(hs.at(o_pl[i]), images[f].plane[p], plane_bytes(images[f], p), "upload frame");
        }
    const float *d_bx = hs.at<float>(o_bx), *d_sc = scores ? hs.at<float>(o_sc) : nullptr;
    const int32_t *d_fi = hs.at<int32_t>(o_fi), *d_rk = hs.at<int32_t>(o_rk), *d_id = hs.at<int32_t>(o_id);
    hs.up(hs.at(o_bx), boxes, bx_bytes, "upload boxes");
    hs.up(hs.at(o_fi), frame_idx, fi_bytes, "upload frame index");
    if (rank) hs.up(hs.at(o_rk), rank, nb, "upload rank");
    if (ids) hs.up(hs.at(o_id), ids, nb, "upload ids");
    if (scores) hs.up(hs.at(o_sc), scores, sc_bytes, "upload scores");
    if (!hs.rc) hs.rc = label_enqueue(c, dev.data(), n_images, d_bx, box_stride, n, d_fi, frame_stride, rank ? d_rk : nullptr, ids ? d_id : nullptr, d_sc, score_stride, st, hs.s);
    for (int f = 0; f < n_images && !hs.rc; ++f)   // the frames are written back in place
        for (int p = 0; p < plane_count(images[f]); ++p)
            hs.down(const_cast<uint8_t*>(images[f].plane[p]), dev[f].plane[p], plane_bytes(images[f], p), "download frame");
    hs.sync();
    return hs.rc;
}

int vp_dbg_draw_labels_host(const vp_image* images, int32_t n_images, const float* boxes, int32_t box_stride, int32_t n, const int32_t* frame_idx, int32_t frame_stride,
                            const int32_t* rank, const int32_t* ids, const float* scores, int32_t score_stride, const vp_label_cfg* cfg) {
    vp::LabelStyle st;
    std::string why;
    if (label_args(images && boxes && frame_idx, images, n_images, n, box_stride, frame_stride, scores != nullptr, score_stride, cfg, st, &why))
        return fail(nullptr, VP_ERR_INVALID, why);
    label_host(images, n_images, boxes, box_stride, n, frame_idx, frame_stride, rank, ids, scores, score_stride, st);
    return VP_OK;
}

int vp_dbg_label_text(int32_t id, int32_t has_score, float score, char* out) {
    if (!out) return fail(nullptr, VP_ERR_INVALID, "labels: null text buffer");
    uint8_t codes[24];
    const int L = vp::label_format(id, has_score != 0, score, codes);
    for (int c = 0; c < L; ++c) out[c] = LABEL_CHARS[codes[c]];
    out[L] = 0;
    return VP_OK;
}

uint64_t vp_dbg_label_glyph(int32_t code) { return code >= 0 && code < vp::LABEL_GLYPHS ? vp::label_glyph(code) : 0; }

}  // extern "C"
