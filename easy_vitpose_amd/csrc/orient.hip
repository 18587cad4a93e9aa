// vp_orient*: frames (vp_image: NV12 / BGR24 / RGB24, pitched) made upright on the device -- the eight EXIF orientations as a pure permutation of elements
// (semantics: orientgeom.h) -- as a stream-ordered stage in front of the letterbox, its synchronous host twin vp_orient, the host-only plan vp_orient_plan and
// the host tap vp_dbg_orient_host.  One kernel, a workgroup per 64 x 64-element tile of a DESTINATION plane, a flat grid over the tiles of every plane of the
// launch's frames; the frame records and the tile prefix travel by kernel argument, ORIENT_PER_LAUNCH frames per launch.  Both global sides are touched in
// contiguous runs: a transposing code reads its tile along source rows into a padded LDS tile and stores it along destination rows; the others go from
// registers.  Four-byte accesses where base and pitch allow (sixteen for a run that keeps its byte order), element accesses otherwise, the same values either way.  No byte outside the row bytes of a
// destination row is written or read-modify-written: a row end takes byte stores.
#include "api_internal.h"
#include "hoststage.h"
#include "orientgeom.h"
#include "pixfmt.h"

using namespace vpi;

namespace vp {

constexpr int ORIENT_THREADS = 256, ORIENT_PER_LAUNCH = 32, ORIENT_SLOTS = 2 * ORIENT_PER_LAUNCH;
struct OrientRec {   // one frame: 80 bytes
    const uint8_t* src[2];
    uint8_t* dst[2];
    int64_t spitch[2], dpitch[2];
    int32_t h, w, format, code;   // the SOURCE frame in pixels
};
// a kernel argument.  first[2 f + p] = the first tile of plane p of the launch's frame f, first[2 count] = the launch's tiles (an absent plane has none)
struct OrientTab { OrientRec r[ORIENT_PER_LAUNCH]; int32_t first[ORIENT_SLOTS + 1]; int32_t pad_; };
static_assert(sizeof(OrientRec) == 80 && sizeof(OrientTab) + 16 <= 4096, "the frame records of a launch fit the kernel argument segment");

__host__ __device__ inline int orient_elem_bytes(int format, int plane) { return format == PIX_NV12 ? (plane ? 2 : 1) : 3; }
__host__ __device__ inline int orient_plane_h(int format, int plane, int h) { return plane ? (format == PIX_NV12 ? (h + 1) / 2 : 0) : h; }
__host__ __device__ inline int orient_plane_w(int format, int plane, int w) { return plane ? (format == PIX_NV12 ? (w + 1) / 2 : 0) : w; }
__host__ __device__ inline int64_t orient_tiles(int oh, int ow) {
    return (int64_t)((oh + ORIENT_TILE - 1) / ORIENT_TILE) * (int64_t)((ow + ORIENT_TILE - 1) / ORIENT_TILE);
}

// nb <= 4 bytes of v to p: one aligned word where the caller says so, bytes otherwise (a row end, an unaligned base or pitch)
__device__ __forceinline__ void orient_store(uint8_t* p, uint32_t v, int nb, bool word) {
    if (word && nb == 4) {
        *reinterpret_cast<uint32_t*>(p) = v;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < nb) p[q] = (uint8_t)(v >> (8 * q));
    }
}

// One destination tile of a plane of ES-byte elements: destination rows [i0, i0 + nrd), columns [j0, j0 + ncd) of the oh x ow output; ph x pw = the source plane.
// A lane makes four adjacent destination bytes of one row at a time (the run of a tile row starts at byte ES j0, a multiple of 4).
template <int ES>
__device__ __forceinline__ void orient_tile(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t sp, int64_t dp, int ph, int pw, OrientOps o, int i0, int j0,
                                            int nrd, int ncd, uint32_t* s_words) {
    constexpr int WPR = 16 * ES;              // words of a full tile row
    constexpr int LP = ES * ORIENT_TILE + 4;  // bytes of a tile row in LDS: one word of padding, an odd count of words
    const bool src_al = (((uintptr_t)src | (uintptr_t)sp) & 3) == 0, dst_al = (((uintptr_t)dst | (uintptr_t)dp) & 3) == 0;
    const int x0 = ES * j0, lb = ES * ncd;    // the destination run of a tile row: bytes [x0, x0 + lb) of the row
    if (!o.transpose) {
        // the source run of destination bytes [x0 + x, x0 + x + 4): the same bytes, or with the columns reversed one word whose elements swap places (ES 1, 2)
        const bool fwd_word = !o.rev_col && src_al;
        const bool rev_word = o.rev_col && ES < 3 && src_al && ((ES * pw) & 3) == 0;
        int x_lo = 0;   // the word loop takes bytes [x_lo, lb) of the run
        if (!o.rev_col && (((uintptr_t)src | (uintptr_t)sp | (uintptr_t)dst | (uintptr_t)dp) & 15) == 0) {
            // the same bytes, both sides 16-byte aligned: whole 16-byte pieces of the run as one load and one store, the rest of the run below
            constexpr int CPR = 4 * ES;
            for (int idx = threadIdx.x; idx < nrd * CPR; idx += ORIENT_THREADS) {
                const int i = i0 + idx / CPR, x = 16 * (idx % CPR);
                if (x + 16 > lb) continue;
                const uint8_t* srow = src + (int64_t)(o.rev_row ? ph - 1 - i : i) * sp;
                *reinterpret_cast<uint4*>(dst + (int64_t)i * dp + x0 + x) = *reinterpret_cast<const uint4*>(srow + x0 + x);
            }
            x_lo = lb & ~15;
        } else if (ES == 3 && o.rev_col && src_al && dst_al && ((3 * pw) & 3) == 0) {
            // three-byte pixels with the columns reversed: four pixels are three aligned words on either side, b0 .. b11 -> b9 b10 b11 b6 b7 b8 b3 b4 b5 b0 b1 b2
            for (int idx = threadIdx.x; idx < nrd * 16; idx += ORIENT_THREADS) {
                const int i = i0 + idx / 16, x = 12 * (idx % 16);
                if (x + 12 > lb) continue;
                const uint32_t* s = reinterpret_cast<const uint32_t*>(src + (int64_t)(o.rev_row ? ph - 1 - i : i) * sp + (3 * pw - 12 - x0 - x));
                const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
                uint32_t* d = reinterpret_cast<uint32_t*>(dst + (int64_t)i * dp + x0 + x);
                d[0] = (w2 >> 8) | ((w1 & 0x00ff0000u) << 8);
                d[1] = (w1 >> 24) | ((w2 & 0xffu) << 8) | ((w0 >> 24) << 16) | (w1 << 24);
                d[2] = ((w1 >> 8) & 0xffu) | (w0 << 8);
            }
            x_lo = lb - lb % 12;
        }
        for (int idx = threadIdx.x; idx < nrd * WPR && x_lo < lb; idx += ORIENT_THREADS) {
            const int ii = idx / WPR, x = 4 * (idx % WPR);
            if (x < x_lo || x >= lb) continue;
            const int nb = lb - x < 4 ? lb - x : 4;
            const int i = i0 + ii;
            const uint8_t* srow = src + (int64_t)(o.rev_row ? ph - 1 - i : i) * sp;
            uint32_t v = 0;
            if (nb == 4 && fwd_word) {
                v = *reinterpret_cast<const uint32_t*>(srow + x0 + x);
            } else if (nb == 4 && rev_word) {
                const uint32_t u = *reinterpret_cast<const uint32_t*>(srow + (ES * pw - 4 - x0 - x));
                v = ES == 1 ? __builtin_bswap32(u) : (u >> 16) | (u << 16);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q >= nb) break;
                    const int e = (x + q) / ES, k = (x + q) % ES;
                    const int c = o.rev_col ? pw - 1 - (j0 + e) : j0 + e;
                    v |= (uint32_t)srow[c * ES + k] << (8 * q);
                }
            }
            orient_store(dst + (int64_t)i * dp + x0 + x, v, nb, dst_al);
        }
        return;
    }
    // transposing: destination column j0 + jj is source row sr(jj), destination row i0 + ii is source column sc(ii).  LDS row jj holds the bytes of source
    // row sr(jj) over the nrd source columns from c_first on, in source order
    uint8_t* s_bytes = reinterpret_cast<uint8_t*>(s_words);
    const int c_first = o.rev_col ? pw - i0 - nrd : i0;
    const int rb = ES * nrd;
    const bool in_word = src_al && ((ES * c_first) & 3) == 0;
    for (int idx = threadIdx.x; idx < ncd * WPR; idx += ORIENT_THREADS) {
        const int jj = idx / WPR, wd = idx % WPR, x = 4 * wd;
        if (x >= rb) continue;
        const int j = j0 + jj;
        const uint8_t* run = src + (int64_t)(o.rev_row ? ph - 1 - j : j) * sp + (int64_t)ES * c_first;
        if (rb - x >= 4 && in_word) {
            s_words[jj * (LP / 4) + wd] = *reinterpret_cast<const uint32_t*>(run + x);
        } else {
            const int nb = rb - x < 4 ? rb - x : 4;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nb) s_bytes[jj * LP + x + q] = run[x + q];
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nrd * WPR; idx += ORIENT_THREADS) {
        const int ii = idx / WPR, x = 4 * (idx % WPR);
        if (x >= lb) continue;
        const int nb = lb - x < 4 ? lb - x : 4;
        const int lc = (o.rev_col ? nrd - 1 - ii : ii) * ES;
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q >= nb) break;
            const int e = (x + q) / ES, k = (x + q) % ES;
            v |= (uint32_t)s_bytes[e * LP + lc + k] << (8 * q);
        }
        orient_store(dst + (int64_t)(i0 + ii) * dp + x0 + x, v, nb, dst_al);
    }
}

// grid = the launch's tiles, flat; n_slots = 2 x its frames.  Everything up to the tile body is the same for the whole workgroup.
__global__ __launch_bounds__(ORIENT_THREADS) void orient_kernel(OrientTab tab, int n_slots) {
    __shared__ __attribute__((aligned(16))) uint32_t s_words[ORIENT_TILE * (3 * ORIENT_TILE + 4) / 4];
    const int tile = blockIdx.x;
    int lo = 0, hi = n_slots;   // first[lo] <= tile < first[hi]: the slot found holds at least one tile
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.first[mid] <= tile) lo = mid; else hi = mid;
    }
    const OrientRec& r = tab.r[lo >> 1];
    const int p = lo & 1;
    const int es = orient_elem_bytes(r.format, p), ph = orient_plane_h(r.format, p, r.h), pw = orient_plane_w(r.format, p, r.w);
    const OrientOps o = orient_ops(r.code);
    const int oh = o.transpose ? pw : ph, ow = o.transpose ? ph : pw;
    const int tiles_x = (ow + ORIENT_TILE - 1) / ORIENT_TILE, t = tile - tab.first[lo];
    const int i0 = (t / tiles_x) * ORIENT_TILE, j0 = (t % tiles_x) * ORIENT_TILE;
    const int nrd = oh - i0 < ORIENT_TILE ? oh - i0 : ORIENT_TILE, ncd = ow - j0 < ORIENT_TILE ? ow - j0 : ORIENT_TILE;
    if (es == 1) orient_tile<1>(r.src[p], r.dst[p], r.spitch[p], r.dpitch[p], ph, pw, o, i0, j0, nrd, ncd, s_words);
    else if (es == 2) orient_tile<2>(r.src[p], r.dst[p], r.spitch[p], r.dpitch[p], ph, pw, o, i0, j0, nrd, ncd, s_words);
    else orient_tile<3>(r.src[p], r.dst[p], r.spitch[p], r.dpitch[p], ph, pw, o, i0, j0, nrd, ncd, s_words);
}

}  // namespace vp

namespace {

using vp::OrientRec;

// the plan of a call (HOST ONLY): every refusal that reads no pixel and no pointer, and the destination layouts.  dst_in: the caller's table, whose non-zero
// pitches are kept after the check (the plan entry) -- or, with strict, whose every field must be the plan's (the entries that move pixels)
int plan(const vp_image* src, const int32_t* codes, int n, const vp_image* dst_in, bool strict, std::vector<vp_image>& out, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "orient: " + m; return (int)VP_ERR_INVALID; };
    if (n < 0 || n > VP_ORIENT_MAX_IMAGES) return bad("n = " + std::to_string(n) + " outside 0.." + std::to_string(VP_ORIENT_MAX_IMAGES));
    if (n > 0 && (!src || !codes || !dst_in)) return bad("null src, codes or dst with n > 0");
    out.resize((size_t)n);
    for (int f = 0; f < n; ++f) {
        const std::string fr = "frame " + std::to_string(f);
        const vp_image& im = src[f];
        const int code = codes[f];
        if (code < vp::ORIENT_FIRST || code > vp::ORIENT_LAST) return bad(fr + " has orientation code " + std::to_string(code) + " outside 1..8");
        if (im.h < 1 || im.w < 1) return bad(fr + " has a non-positive size " + std::to_string(im.h) + " x " + std::to_string(im.w));
        vp_image layout = im;   // the plan reads no pointer: a null plane is the refusal of the entries that move pixels
        layout.plane[1] = layout.plane[0] = reinterpret_cast<const uint8_t*>(&layout);
        std::string w;
        if (image_check(layout, f, &w)) return bad(w);
        const bool nv12 = im.format == vp::PIX_NV12;
        if (nv12 && !vp::orient_nv12_ok(code, im.h, im.w))
            return bad(fr + " is NV12 of " + std::to_string(im.h) + " x " + std::to_string(im.w) + ": code " + std::to_string(code) + " reverses an axis of odd length");
        vp_image& d = out[f];
        d = dst_in[f];
        const int oh = vp::orient_out_h(code, im.h, im.w), ow = vp::orient_out_w(code, im.h, im.w);
        if (strict && (d.h != oh || d.w != ow || d.format != im.format || d.matrix != im.matrix))
            return bad(fr + ": dst is " + std::to_string(d.h) + " x " + std::to_string(d.w) + " format " + std::to_string(d.format) + " matrix " + std::to_string(d.matrix) +
                       ", the plan says " + std::to_string(oh) + " x " + std::to_string(ow) + " format " + std::to_string(im.format) + " matrix " + std::to_string(im.matrix));
        d.h = oh; d.w = ow; d.format = im.format; d.matrix = im.matrix;
        for (int pl = 0; pl < 2; ++pl) {
            const int64_t row = vp::plane_row_bytes(d.format, pl, ow);
            if (pl >= plane_count(d)) { if (!strict) d.pitch[pl] = 0; continue; }
            if (d.pitch[pl] == 0 && !strict) d.pitch[pl] = row;
            if (d.pitch[pl] < row)
                return bad(fr + ": dst pitch[" + std::to_string(pl) + "] " + std::to_string(d.pitch[pl]) + " is below its " + std::to_string(row) + " row bytes");
        }
    }
    return VP_OK;
}

struct Range { const uint8_t* lo; const uint8_t* hi; int frame; bool is_dst; };

// what the entries that move pixels refuse on top of the plan: a null plane, and a destination plane whose bytes (first to last) meet a source plane's or
// another destination plane's
int planes_check(const vp_image* src, const std::vector<vp_image>& dst, int n, std::string* why) {
    auto bad = [&](const std::string& m) { *why = "orient: " + m; return (int)VP_ERR_INVALID; };
    std::vector<Range> rs;
    for (int f = 0; f < n; ++f)
        for (int pl = 0; pl < plane_count(src[f]); ++pl) {
            if (!src[f].plane[pl]) return bad("frame " + std::to_string(f) + " has no data (src plane[" + std::to_string(pl) + "] is null)");
            if (!dst[f].plane[pl]) return bad("frame " + std::to_string(f) + " has nowhere to go (dst plane[" + std::to_string(pl) + "] is null)");
            rs.push_back(Range{src[f].plane[pl], src[f].plane[pl] + plane_bytes(src[f], pl), f, false});
            rs.push_back(Range{dst[f].plane[pl], dst[f].plane[pl] + plane_bytes(dst[f], pl), f, true});
        }
    for (size_t a = 0; a < rs.size(); ++a)
        for (size_t b = a + 1; b < rs.size(); ++b) {
            if (!rs[a].is_dst && !rs[b].is_dst) continue;   // two sources may be one frame
            if (rs[a].lo < rs[b].hi && rs[b].lo < rs[a].hi) {
                const Range& d = rs[a].is_dst ? rs[a] : rs[b];
                const Range& o = rs[a].is_dst ? rs[b] : rs[a];
                return bad("a dst plane of frame " + std::to_string(d.frame) + " overlaps a " + (o.is_dst ? "dst" : "src") + " plane of frame " + std::to_string(o.frame) +
                           " (there is no in-place orientation)");
            }
        }
    return VP_OK;
}

// the records of a checked call, and its refusal where the tiles of one launch do not fit the grid
int records(const vp_image* src, const int32_t* codes, const std::vector<vp_image>& dst, int n, std::vector<OrientRec>& recs, std::string* why) {
    recs.resize((size_t)n);
    for (int first = 0; first < n; first += vp::ORIENT_PER_LAUNCH) {
        int64_t tiles = 0;
        for (int f = first; f < std::min(n, first + vp::ORIENT_PER_LAUNCH); ++f) {
            OrientRec& r = recs[f];
            for (int pl = 0; pl < 2; ++pl) {
                r.src[pl] = src[f].plane[pl]; r.dst[pl] = const_cast<uint8_t*>(dst[f].plane[pl]);
                r.spitch[pl] = src[f].pitch[pl]; r.dpitch[pl] = dst[f].pitch[pl];
            }
            r.h = src[f].h; r.w = src[f].w; r.format = src[f].format; r.code = codes[f];
            for (int pl = 0; pl < plane_count(src[f]); ++pl) tiles += vp::orient_tiles(vp::plane_rows(dst[f].format, pl, dst[f].h), vp::orient_plane_w(dst[f].format, pl, dst[f].w));
        }
        if (tiles > INT32_MAX) { *why = "orient: frames " + std::to_string(first) + ".. hold more tiles than one launch takes"; return VP_ERR_INVALID; }
    }
    return VP_OK;
}

// plane pl of frame f, bytes [q, q + bytes): device memory of the handle's device, inside one allocation (the check of the image entries)
int check_device_plane(vp_ctx* c, const uint8_t* q, size_t bytes, int f, const char* side) {
    if (device_range_ok(c, q, bytes)) return VP_OK;
    (void)hipGetLastError();
    return fail(c, VP_ERR_INVALID, std::string("orient: ") + side + " frame " + std::to_string(f) + " is not device memory of device " + std::to_string(c->cfg.device_id) +
                                       " (or runs past the end of its allocation)");
}

// the checked call on stream s (the handle's device is current): one launch per ORIENT_PER_LAUNCH frames
int enqueue(vp_ctx* c, const std::vector<OrientRec>& recs, hipStream_t s) {
    const int n = (int)recs.size();
    for (int first = 0; first < n; first += vp::ORIENT_PER_LAUNCH) {
        const int count = std::min(vp::ORIENT_PER_LAUNCH, n - first);
        vp::OrientTab tab;
        std::memset(&tab, 0, sizeof(tab));
        std::memcpy(tab.r, recs.data() + first, sizeof(OrientRec) * (size_t)count);
        int64_t tiles = 0;
        for (int k = 0; k < count; ++k)
            for (int pl = 0; pl < 2; ++pl) {
                const OrientRec& r = tab.r[k];
                tab.first[2 * k + pl] = (int32_t)tiles;
                const int ph = vp::orient_plane_h(r.format, pl, r.h), pw = vp::orient_plane_w(r.format, pl, r.w);
                if (ph > 0 && pw > 0) tiles += vp::orient_tiles(vp::orient_out_h(r.code, ph, pw), vp::orient_out_w(r.code, ph, pw));
            }
        tab.first[2 * count] = (int32_t)tiles;
        if (tiles == 0) continue;
        hipLaunchKernelGGL(vp::orient_kernel, dim3((unsigned)tiles), dim3(vp::ORIENT_THREADS), 0, s, tab, 2 * count);
        HIPCHK(c, hipGetLastError());
    }
    return VP_OK;
}

// every host-side check of the entries that move pixels; dst_full = the checked destination table
int checked(const vp_image* src, const int32_t* codes, const vp_image* dst, int n, std::vector<vp_image>& dst_full, std::vector<OrientRec>& recs, std::string* why) {
    if (plan(src, codes, n, dst, true, dst_full, why) || planes_check(src, dst_full, n, why)) return VP_ERR_INVALID;
    return records(src, codes, dst_full, n, recs, why);
}

}  // namespace

extern "C" {

int vp_orient_plan(const vp_image* src, const int32_t* codes, int32_t n, vp_image* dst, int64_t* plane_bytes_out) {
    std::vector<vp_image> out;
    std::string why;
    if (plan(src, codes, n, dst, false, out, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    for (int f = 0; f < n; ++f) {
        dst[f].h = out[f].h; dst[f].w = out[f].w; dst[f].format = out[f].format; dst[f].matrix = out[f].matrix;
        dst[f].pitch[0] = out[f].pitch[0]; dst[f].pitch[1] = out[f].pitch[1];
        if (plane_bytes_out)
            for (int pl = 0; pl < 2; ++pl) plane_bytes_out[2 * f + pl] = pl < plane_count(out[f]) ? (int64_t)plane_bytes(out[f], pl) : 0;
    }
    return VP_OK;
}

int vp_orient_stream(vp_handle c, const vp_image* src, const int32_t* codes, const vp_image* dst, int32_t n, void* caller_stream) {
    if (!c) return VP_ERR_INVALID;
    std::vector<vp_image> full;
    std::vector<OrientRec> recs;
    std::string why;
    if (checked(src, codes, dst, n, full, recs, &why)) return fail(c, VP_ERR_INVALID, why);
    if (n == 0) return VP_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    for (int f = 0; f < n; ++f)
        for (int pl = 0; pl < plane_count(src[f]); ++pl)
            if (check_device_plane(c, src[f].plane[pl], plane_bytes(src[f], pl), f, "src") || check_device_plane(c, full[f].plane[pl], plane_bytes(full[f], pl), f, "dst"))
                return VP_ERR_INVALID;
    return enqueue(c, recs, (hipStream_t)caller_stream);
}

int vp_orient(vp_handle c, const vp_image* src, const int32_t* codes, const vp_image* dst, int32_t n) {
    if (!c) return VP_ERR_INVALID;
    std::vector<vp_image> full;
    std::vector<OrientRec> recs;
    std::string why;
    if (checked(src, codes, dst, n, full, recs, &why)) return fail(c, VP_ERR_INVALID, why);
    if (n == 0) return VP_OK;
    // one scratch block: every plane of either side at the caller's pitch, each part at its caller's address modulo 256 (the kernel then takes the access
    // widths it would take on the caller's own layout)
    HostStage st(c);
    std::vector<size_t> off((size_t)n * 4, 0);
    for (int f = 0; f < n; ++f)
        for (int pl = 0; pl < plane_count(src[f]); ++pl) {
            off[4 * f + pl] = st.part(plane_bytes(src[f], pl), (size_t)((uintptr_t)src[f].plane[pl] % 256));
            off[4 * f + 2 + pl] = st.part(plane_bytes(full[f], pl), (size_t)((uintptr_t)full[f].plane[pl] % 256));
        }
    if (st.alloc()) return st.rc;
    for (int f = 0; f < n && !st.rc; ++f)
        for (int pl = 0; pl < plane_count(src[f]); ++pl) {
            st.up(st.at(off[4 * f + pl]), src[f].plane[pl], plane_bytes(src[f], pl), "upload plane");
            recs[f].src[pl] = st.at<uint8_t>(off[4 * f + pl]);
            recs[f].dst[pl] = st.at<uint8_t>(off[4 * f + 2 + pl]);
        }
    if (!st.rc) st.rc = enqueue(c, recs, st.s);
    for (int f = 0; f < n && !st.rc; ++f)   // the row bytes of every destination row, never the gap between two rows
        for (int pl = 0; pl < plane_count(src[f]); ++pl)
            st.chk(hipMemcpy2DAsync(const_cast<uint8_t*>(full[f].plane[pl]), (size_t)full[f].pitch[pl], st.at(off[4 * f + 2 + pl]), (size_t)full[f].pitch[pl],
                                    (size_t)vp::plane_row_bytes(full[f].format, pl, full[f].w), (size_t)vp::plane_rows(full[f].format, pl, full[f].h), hipMemcpyDeviceToHost, st.s),
                   "download plane");
    st.sync();
    return st.rc;
}

int vp_dbg_orient_host(const vp_image* src, const int32_t* codes, const vp_image* dst, int32_t n) {
    std::vector<vp_image> full;
    std::vector<OrientRec> recs;
    std::string why;
    if (checked(src, codes, dst, n, full, recs, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    for (int f = 0; f < n; ++f) {
        const OrientRec& r = recs[f];
        const vp::OrientOps o = vp::orient_ops(r.code);
        for (int pl = 0; pl < plane_count(src[f]); ++pl) {
            const int es = vp::orient_elem_bytes(r.format, pl), ph = vp::orient_plane_h(r.format, pl, r.h), pw = vp::orient_plane_w(r.format, pl, r.w);
            const int oh = vp::orient_out_h(r.code, ph, pw), ow = vp::orient_out_w(r.code, ph, pw);
            for (int i = 0; i < oh; ++i)
                for (int j = 0; j < ow; ++j) {
                    int sr, sc;
                    vp::orient_source(o, ph, pw, i, j, &sr, &sc);
                    std::memcpy(r.dst[pl] + (int64_t)i * r.dpitch[pl] + (int64_t)j * es, r.src[pl] + (int64_t)sr * r.spitch[pl] + (int64_t)sc * es, (size_t)es);
                }
        }
    }
    return VP_OK;
}

}  // extern "C"
