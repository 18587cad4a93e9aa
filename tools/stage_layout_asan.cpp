// Address / undefined-behaviour check of the layout part of csrc/hoststage.h (up256, StageLayout, plane_count, plane_bytes): a stand-alone program, HOST ONLY, no
// device is touched and nothing of it is loaded into Python.  The layout part is header-only, so this file is the whole program:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/stage_layout_asan.cpp -o stage_layout_asan && ./stage_layout_asan
//
// For the part list of each of the sixteen sites that stage host arrays (the synchronous twins and the two handle-less taps) it lays the block out at zero counts,
// with every optional part absent, at one row, at counts around 256 bytes of a part, on pitched NV12 / RGB planes and, for orient, at every caller address modulo
// 256, and asserts: every offset = skew (mod 256); parts in order, disjoint, each with room for up256(bytes); total >= the end of the last part + 256.  The block is
// a heap block of exactly total() bytes and the room of every part is written and read back, so a part past the block or over another part is a heap overflow or a
// wrong byte.  A plane is a heap block of exactly plane_bytes() and every row of it is written.  At the largest counts the entries accept the arithmetic is compared
// with 128-bit integers (nothing is allocated).  Then the mask part of csrc/stageobj.h (popcount64, mask_check) on the masks at the edges of n_streams = 1 and 64.
// Exit status 0, "stage layout ok" and no sanitizer report is the pass (tests/test_stage_layout_host.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../easy_vitpose_amd/csrc/hoststage.h"
#include "../easy_vitpose_amd/csrc/stageobj.h"

using vpi::plane_bytes;
using vpi::plane_count;
using vpi::up256;

struct Part { size_t bytes, skew; };
typedef std::vector<Part> Parts;
static long n_layouts = 0;

#define REQUIRE(cond)                                                                          \
    do {                                                                                       \
        if (!(cond)) { std::printf("%s: %s fails (line %d)\n", site, #cond, __LINE__); std::exit(1); } \
    } while (0)

static void check(const char* site, const Parts& parts) {
    vpi::StageLayout lay;
    std::vector<size_t> off;
    unsigned __int128 wide = 0;   // the same rule in integers that cannot wrap
    for (const Part& p : parts) {
        off.push_back(lay.part(p.bytes, p.skew));
        REQUIRE(off.back() % 256 == p.skew);
        REQUIRE((unsigned __int128)off.back() == wide + p.skew);
        wide = (wide + p.skew + ((unsigned __int128)p.bytes + 255) / 256 * 256 + 255) / 256 * 256;
        REQUIRE(wide + 256 <= (unsigned __int128)SIZE_MAX && (unsigned __int128)lay.total() == wide + 256);
    }
    for (size_t i = 0; i < parts.size(); ++i) {
        const size_t next = i + 1 < parts.size() ? off[i + 1] : lay.total() - 256;
        REQUIRE(off[i] + up256(parts[i].bytes) <= next);   // in order, disjoint, room for up256(bytes); behind the last part 256 bytes of slack
    }
    REQUIRE(lay.end % 256 == 0 && lay.total() == lay.end + 256);
    ++n_layouts;
    if (lay.total() > ((size_t)64 << 20)) return;   // the arithmetic only
    std::unique_ptr<uint8_t[]> block(new uint8_t[lay.total()]);   // exactly total() bytes
    for (size_t i = 0; i < parts.size(); ++i) std::memset(block.get() + off[i], (int)(i + 1), up256(parts[i].bytes));
    for (size_t i = 0; i < parts.size(); ++i)
        for (size_t b = 0; b < up256(parts[i].bytes); b += 255) REQUIRE(block[off[i] + b] == (uint8_t)(i + 1));
    std::memset(block.get() + lay.end, 0xEE, 256);   // the slack
}

// a frame on exact heap planes: every row of every plane written, first byte to last
struct Frame {
    vp_image im{};
    std::unique_ptr<uint8_t[]> mem[2];
    Frame(int format, int h, int w, int64_t extra_pitch) {
        im.format = format; im.h = h; im.w = w; im.matrix = 0;
        for (int p = 0; p < plane_count(im); ++p) {
            im.pitch[p] = vp::plane_row_bytes(format, p, w) + extra_pitch;
            mem[p].reset(new uint8_t[plane_bytes(im, p)]);
            im.plane[p] = mem[p].get();
            for (int64_t r = 0; r < vp::plane_rows(format, p, h); ++r) std::memset(mem[p].get() + r * im.pitch[p], 0x5A, (size_t)vp::plane_row_bytes(format, p, w));
        }
    }
};

static void add_planes(Parts& parts, const std::vector<Frame>& frames, bool skewed = false) {
    for (const Frame& f : frames)
        for (int p = 0; p < plane_count(f.im); ++p) parts.push_back(Part{plane_bytes(f.im, p), skewed ? (size_t)((uintptr_t)f.im.plane[p] % 256) : 0});
}

// ---- the part lists of the sixteen sites, as their entries state them (o: bit i set = optional input i given)
static Parts pose_nms(size_t n, size_t k, size_t ss, size_t nf) { return {{n * k * 12, 0}, {((n - 1) * ss + 1) * 4, 0}, {n * 36, 0}, {n * 4, 0}, {n * 4, 0}, {n * 4, 0}, {nf * 4, 0}}; }
static Parts draw(const std::vector<Frame>& fr, size_t n, size_t k, size_t fs, bool boxes, size_t bs) {
    Parts p;
    add_planes(p, fr);
    p.insert(p.end(), {{n * k * 12, 0}, {((n - 1) * fs + 1) * 4, 0}, {n * 4, 0}, {n * 4, 0}});
    if (boxes) p.push_back({((n - 1) * bs + 4) * 4, 0});
    return p;
}
static Parts labels(const std::vector<Frame>& fr, size_t n, size_t bs, size_t fs, bool scores, size_t ss) {
    Parts p;
    add_planes(p, fr);
    p.insert(p.end(), {{((n - 1) * bs + 4) * 4, 0}, {((n - 1) * fs + 1) * 4, 0}, {n * 4, 0}, {n * 4, 0}});
    if (scores) p.push_back({((n - 1) * ss + 1) * 4, 0});
    return p;
}
static Parts collect(size_t table, size_t n, size_t k, bool score, size_t ss) {
    return {{table, 0}, {n * 3 * k * 4, 0}, {n * 4, 0}, {n * 4, 0}, {n * 4, 0}, {n * 4, 0}, {score && n ? ((n - 1) * ss + 1) * 4 : 0, 0}, {n * 36, 0}};
}
static Parts tracker(size_t nd, size_t rs, size_t n_out, size_t ns) {
    return {{nd ? ((nd - 1) * rs + 5) * 4 : 0, 0}, {nd * 4, 0}, {n_out * 24, 0}, {n_out * 4, 0}, {n_out * 4, 0}, {(ns + 1) * 4, 0}, {(ns + 1) * 4, 0}};
}
static Parts smoother(size_t n, size_t k, size_t ns) { return {{n * k * 12, 0}, {n * 4, 0}, {n * 4, 0}, {n * 4, 0}, {ns * 4, 0}}; }
static Parts detect(size_t ni, size_t nc, size_t A, size_t es, size_t n_out) {
    return {{ni * (4 + nc) * A * es, 0}, {n_out * 24, 0}, {n_out * 4, 0}, {n_out * 4, 0}, {(ni + 1) * 4, 0}, {(ni + 1) * 4, 0}};
}
static Parts letterbox(const std::vector<Frame>& fr, size_t in_h, size_t in_w, size_t es) {
    Parts p{{fr.size() * 3 * in_h * in_w * es, 0}};
    add_planes(p, fr);
    return p;
}
static Parts orient(const std::vector<Frame>& src, const std::vector<Frame>& dst) {   // src and dst plane by plane, each at its caller's address modulo 256
    Parts p;
    for (size_t f = 0; f < src.size(); ++f)
        for (int pl = 0; pl < plane_count(src[f].im); ++pl) {
            p.push_back({plane_bytes(src[f].im, pl), (size_t)((uintptr_t)src[f].im.plane[pl] % 256)});
            p.push_back({plane_bytes(dst[f].im, pl), (size_t)((uintptr_t)dst[f].im.plane[pl] % 256)});
        }
    return p;
}
static Parts metrics(size_t n, size_t k) { return {{n * k * 12, 0}, {n * k * 12, 0}, {n * 8, 0}, {n * 4, 0}, {n * 4, 0}, {n * 4, 0}, {n * 4, 0}, {n * k * 4, 0}}; }
static Parts coco_update(size_t n, size_t g, size_t k) {
    return {{n * k * 12, 0}, {n * 4, 0}, {n * 4, 0}, {n * 4, 0}, {g * k * 12, 0}, {g * 16, 0}, {g * 4, 0}, {g * 4, 0}, {g * 4, 0}, {n * 40, 0}};
}
static Parts coco_accumulate(size_t result) { return {{result, 0}}; }
static Parts yolo_forward(size_t ni, size_t h, size_t w, size_t nc, size_t A, size_t es) { return {{ni * 3 * h * w * 2, 0}, {ni * (4 + nc) * A * es, 0}}; }
static Parts yolo_conv(size_t pin, size_t in_stride, size_t pout, size_t out_stride, size_t oes, bool res, size_t res_stride, size_t w_elems, size_t b_elems) {
    Parts p{{pin * in_stride * 2, 0}, {pout * out_stride * oes, 0}};
    if (res) p.push_back({pout * res_stride * 2, 0});
    p.insert(p.end(), {{w_elems * 2, 0}, {b_elems * 4, 0}});
    return p;
}
static Parts pose_oks(size_t n, size_t k) { return {{n * k * 12, 0}, {n * 36, 0}, {n * n * 4, 0}}; }
static Parts lsap(size_t nd, size_t nt) { return {{nd * nt * 8, 0}, {nd * 4, 0}}; }

int main() {
    const char* site = "up256";
    REQUIRE(up256(0) == 0 && up256(1) == 256 && up256(255) == 256 && up256(256) == 256 && up256(257) == 512);

    // frames: NV12 and RGB / BGR, odd sizes, rows of 255 / 256 / 257 bytes, with and without a pitch larger than the row
    std::vector<std::vector<Frame>> sets;
    for (int64_t extra : {0, 1, 13, 64}) {
        std::vector<Frame> s;
        for (int w : {1, 255, 256, 257}) { s.emplace_back(VP_PIX_NV12, 1, w, extra); s.emplace_back(VP_PIX_NV12, 33, w, extra); }
        for (int w : {1, 85, 86, 48}) { s.emplace_back(VP_PIX_RGB24, 1, w, extra); s.emplace_back(VP_PIX_BGR24, 32, w, extra); }
        sets.push_back(std::move(s));
    }
    site = "plane_bytes";
    {
        const Frame nv(VP_PIX_NV12, 5, 7, 9), rgb(VP_PIX_RGB24, 4, 3, 2);
        REQUIRE(plane_count(nv.im) == 2 && plane_count(rgb.im) == 1);
        REQUIRE(plane_bytes(nv.im, 0) == 4 * 16 + 7 && plane_bytes(nv.im, 1) == 2 * 17 + 8 && plane_bytes(rgb.im, 0) == 3 * 11 + 9);
    }

    const size_t counts[] = {1, 2, 8, 63, 64, 65, 257};   // one row; parts of n * 4 bytes at 252, 256 and 260 bytes (a row count never gives 255 or 257: the byte planes do)
    for (size_t n : counts)
        for (size_t k : {1, 17, 133}) {
            for (size_t stride : {1, 5, 6})
                for (size_t nf : {0, 1, 64}) check(site = "vp_pose_nms", pose_nms(n, k, stride, nf));
            check(site = "vp_dbg_pose_oks", pose_oks(n, k));
            for (size_t ns : {1, 63, 64}) check(site = "vp_smooth_update", smoother(n, k, ns));
            check(site = "vp_metrics_update", metrics(n, k));
            for (size_t g : {0, 1, 64, 65}) check(site = "vp_cocoeval_update", coco_update(n, g, k));
            for (int o = 0; o < 2; ++o)
                for (size_t table : {255, 256, 257, 4096 + 36}) check(site = "vp_collect", collect(table, n, k, o != 0, 6));
            for (const std::vector<Frame>& fr : sets)
                for (int o = 0; o < 2; ++o) {
                    check(site = "vp_draw_poses", draw(fr, n, k, 9, o != 0, 6));
                    check(site = "vp_draw_labels", labels(fr, n, 6, 9, o != 0, 6));
                }
        }
    // zero counts where the entry accepts them
    for (size_t k : {1, 17}) {
        check(site = "vp_smooth_update", smoother(0, k, 1));
        check(site = "vp_metrics_update", metrics(0, k));
        check(site = "vp_cocoeval_update", coco_update(0, 0, k));
        check(site = "vp_cocoeval_update", coco_update(0, 3, k));
        check(site = "vp_collect", collect(4 * 2, 0, k, false, 1));
        check(site = "vp_collect", collect(4 * 2, 0, k, true, 1));
    }
    for (size_t nd : {0, 1, 63, 64, 65, 128})
        for (size_t n_out : {0, 1, 64, 65})
            for (size_t ns : {1, 64}) check(site = "vp_tracker_update", tracker(nd, 6, n_out, ns));
    for (size_t nd : {1, 31, 32, 33, 128})
        for (size_t nt : {1, 32, 128}) check(site = "vp_dbg_lsap", lsap(nd, nt));
    for (size_t ni : {0, 1, 2, 64})
        for (size_t A : {1, 51, 64, 8400})
            for (size_t es : {2, 4})
                for (size_t n_out : {0, 1, 64, 300}) check(site = "vp_detect", detect(ni, 1, A, es, n_out));
    for (const std::vector<Frame>& fr : sets)
        for (size_t es : {1, 2, 4}) check(site = "vp_letterbox", letterbox(fr, 32, 32, es));
    check(site = "vp_cocoeval_accumulate", coco_accumulate(1));
    check(site = "vp_cocoeval_accumulate", coco_accumulate(255));
    check(site = "vp_cocoeval_accumulate", coco_accumulate(10 * 1024 + 8));
    for (size_t ni : {1, 2})
        for (size_t es : {2, 4}) check(site = "vp_yolo_forward", yolo_forward(ni, 32, 64, 80, 42, es));
    for (int o = 0; o < 2; ++o)
        for (size_t pix : {1, 15, 16, 17})
            for (size_t oes : {2, 4}) check(site = "vp_dbg_yolo_conv_case", yolo_conv(4 * pix, 8, pix, 17, oes, o != 0, 24, 32 * 96, 32));

    // orient: the caller's planes at every residue modulo 256 (the multiples of 1, so those of 2, 4 and 16 too): frames carved from one arena at arena + r
    site = "vp_orient";
    {
        std::unique_ptr<uint8_t[]> arena(new uint8_t[1 << 16]);
        for (int r = 0; r < 256; ++r)
            for (int format : {VP_PIX_NV12, VP_PIX_RGB24}) {
                vp_image s{}, d{};
                s.format = d.format = format; s.h = d.w = 5; s.w = d.h = 7;   // a transposing code swaps h and w
                uint8_t* q = arena.get() + r;
                for (vp_image* im : {&s, &d})
                    for (int p = 0; p < plane_count(*im); ++p) {
                        im->pitch[p] = vp::plane_row_bytes(format, p, im->w) + 3;
                        im->plane[p] = q;
                        q += plane_bytes(*im, p) + (size_t)(r * 5 + p);   // the next plane at another residue
                    }
                Parts parts;
                for (int p = 0; p < plane_count(s); ++p) {
                    parts.push_back({plane_bytes(s, p), (size_t)((uintptr_t)s.plane[p] % 256)});
                    parts.push_back({plane_bytes(d, p), (size_t)((uintptr_t)d.plane[p] % 256)});
                }
                check(site, parts);
            }
        for (const std::vector<Frame>& fr : sets) check(site, orient(fr, fr));
    }

    // the largest counts the entries accept: the sums stay below 2^64 (check() compares every step with 128-bit integers)
    check(site = "vp_smooth_update", smoother(VP_SMOOTH_MAX_ROWS, 1024, 64));
    check(site = "vp_detect", detect(64, 256, (size_t)1 << 20, 4, (size_t)1 << 20));
    check(site = "vp_yolo_forward", yolo_forward(64, 1280, 1280, 256, (size_t)1 << 20, 4));
    check(site = "vp_dbg_pose_oks", pose_oks(32768, 1024));

    // the mask part of csrc/stageobj.h: no mask, the last stream, the first bit beyond it, all 64 bits, at n_streams 1 and 64 (a shift by 64 would be undefined)
    site = "mask_check";
    int n_masks = 0;
    for (int ns : {1, 64}) {
        const uint64_t last = 1ull << (ns - 1), all = ~0ull;
        std::string why;
        REQUIRE(vpi::mask_check(0, ns, "tracker: ", &why) == VP_OK && vpi::mask_check(last, ns, "tracker: ", &why) == VP_OK && why.empty());
        REQUIRE(vpi::popcount64(0) == 0 && vpi::popcount64(last) == 1 && vpi::popcount64(all) == 64);
        n_masks += 2;
        if (ns < 64) {   // bit n_streams exists
            REQUIRE(vpi::mask_check(1ull << ns, ns, "tracker: ", &why) == VP_ERR_INVALID && why == "tracker: a mask bit beyond n_streams = 1");
            REQUIRE(vpi::mask_check(all, ns, "smoother: ", &why) == VP_ERR_INVALID && why == "smoother: a mask bit beyond n_streams = 1");
            REQUIRE(vpi::popcount64(1ull << ns) == 1);
            n_masks += 2;
        } else {
            REQUIRE(vpi::mask_check(all, ns, "smoother: ", &why) == VP_OK && why.empty());
            ++n_masks;
        }
    }

    std::printf("stage layout ok (%ld layouts, %d masks)\n", n_layouts, n_masks);
    return 0;
}
