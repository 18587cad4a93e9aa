// Address / undefined-behaviour check of the host side of the detector network (csrc/yologeom.h: the plan, the load step, the Detect decode): a stand-alone
// program, HOST ONLY, no device is touched and nothing of it is loaded into Python.  yologeom.h is header-only on the host, so this file is the whole program:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/yolo_host_asan.cpp -o yolo_host_asan && ./yolo_host_asan
//
// Every checkpoint tensor, every folded weight image and bias, every Detect level and every head is a heap block of exactly its documented size, so a byte read
// or written past one is a heap overflow the sanitizer reports.  It plans every scale at several sizes and walks every launch's extents, folds every convolution
// of scale n and m (nc = 91: the padded class branch) from an unfused and a fused checkpoint, and decodes both head layouts.  Exit status 0, "yolo host ok" and
// no sanitizer report is the pass (tests/test_yolo_host.py builds and runs it).
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../easy_vitpose_amd/csrc/yologeom.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffffff) / 16777216.f; }

struct Checkpoint {
    std::vector<std::string> names;
    std::vector<std::unique_ptr<float[]>> data;
    std::vector<vp_yolo_tensor> tab;
    void add(const std::string& name, std::initializer_list<int> shape, float lo, float hi) {
        int64_t n = 1;
        for (int s : shape) n *= s;
        std::unique_ptr<float[]> p(new float[(size_t)n]);   // exactly numel floats
        for (int64_t i = 0; i < n; ++i) p[i] = uniform(lo, hi);
        vp_yolo_tensor t{};
        t.numel = n; t.ndim = (int32_t)shape.size();
        int i = 0;
        for (int s : shape) t.shape[i++] = s;
        t.data = p.get();
        names.push_back(name);
        data.push_back(std::move(p));
        tab.push_back(t);
    }
    void finish() { for (size_t i = 0; i < tab.size(); ++i) tab[i].name = names[i].c_str(); }
};

// the checkpoint of a plan's convolutions, unfused or fused
static void fill(const vp::YoloPlan& p, bool fused, Checkpoint* ck) {
    for (const vp::YoloConv& cv : p.convs) {
        if (!cv.module) {
            ck->add(cv.key + ".weight", {cv.c2, cv.c1, cv.k, cv.k}, -1.f, 1.f);
            ck->add(cv.key + ".bias", {cv.c2}, -1.f, 1.f);
            continue;
        }
        ck->add(cv.key + ".conv.weight", {cv.c2, cv.c1, cv.k, cv.k}, -1.f, 1.f);
        if (fused) { ck->add(cv.key + ".conv.bias", {cv.c2}, -1.f, 1.f); continue; }
        ck->add(cv.key + ".bn.weight", {cv.c2}, 0.5f, 1.5f);
        ck->add(cv.key + ".bn.bias", {cv.c2}, -1.f, 1.f);
        ck->add(cv.key + ".bn.running_mean", {cv.c2}, -1.f, 1.f);
        ck->add(cv.key + ".bn.running_var", {cv.c2}, 0.f, 2.f);
    }
    ck->add("model.22.dfl.conv.weight", {1, 16, 1, 1}, 0.f, 0.f);
    for (int j = 0; j < 16; ++j) ck->data.back()[j] = (float)j;
    ck->finish();
}

static int fail(const char* what, const std::string& why) { std::printf("FAILED %s: %s\n", what, why.c_str()); return 1; }

int main() {
    uint64_t sum = 0;
    const int sizes[][2] = {{32, 32}, {64, 96}, {640, 640}, {1280, 1280}};
    for (char scale : {'n', 's', 'm', 'l', 'x'})
        for (const auto& hw : sizes) {
            vp::YoloDims d;
            if (!vp::yolo_dims(scale, 80, &d)) return fail("dims", std::string(1, scale));
            vp::YoloPlan p;
            vp::yolo_plan(d, hw[0], hw[1], VP_DET_F32, &p);
            for (const vp_yolo_launch& l : p.launches) {
                const vp_yolo_buffer &bi = p.bufs[(size_t)l.in_buf], &bo = p.bufs[(size_t)l.out_buf];
                const size_t pin = (size_t)64 * bi.h * bi.w, pout = (size_t)64 * bo.h * bo.w;
                if (l.kind != vp::YK_DECODE && vp::yolo_at(pin - 1, l.in_stride, l.in_off, l.c_in - 1) >= pin * (size_t)bi.c) return fail("extent", "input");
                if (l.kind != vp::YK_DECODE && vp::yolo_at(pout - 1, l.out_stride, l.out_off, l.c_out - 1) >= pout * (size_t)bo.c) return fail("extent", "output");
                sum += (uint64_t)l.c_in * 31 + (uint64_t)l.c_out;
            }
        }
    for (int round = 0; round < 4; ++round) {
        const bool fused = round & 1;
        vp::YoloDims d;
        vp::yolo_dims(round < 2 ? 'n' : 'm', round < 2 ? 80 : 91, &d);
        vp::YoloPlan p;
        vp::yolo_plan(d, 32, 64, VP_DET_F32, &p);
        Checkpoint ck;
        fill(p, fused, &ck);
        vp::YoloTensors tab;
        vp::YoloDims back;
        const std::string why = vp::yolo_read_dims(ck.tab.data(), (int)ck.tab.size(), &tab, &back);
        if (!why.empty()) return fail("read_dims", why);
        if (back.scale != d.scale || back.nc != d.nc || back.c3d != d.c3d) return fail("read_dims", "other dims than the plan's");
        for (const vp::YoloConv& cv : p.convs) {
            std::unique_ptr<uint16_t[]> w(new uint16_t[(size_t)cv.c2w * cv.cols]);   // exactly rows x cols
            std::unique_ptr<float[]> b(new float[(size_t)cv.c2w]);
            const std::string r = vp::yolo_fold(tab, cv, w.get(), (size_t)cv.cols, b.get());
            if (!r.empty()) return fail("fold", r);
            for (size_t i = 0; i < (size_t)cv.c2w * cv.cols; ++i) sum += w[i];
        }
        // the decode on levels and heads of exact size
        const int n = 2, nc = d.nc, cs = vp::YOLO_BOX_CH + nc;
        std::unique_ptr<float[]> lvl[3];
        const float* ptr[3];
        vp::DecodeArgs da;
        for (int i = 0; i < 3; ++i) {
            const size_t count = (size_t)n * p.level_h[i] * p.level_w[i] * cs;
            lvl[i].reset(new float[count]);
            for (size_t q = 0; q < count; ++q) lvl[i][q] = uniform(-20.f, 20.f);
            ptr[i] = lvl[i].get();
            da.lvl[i] = ptr[i]; da.h[i] = p.level_h[i]; da.w[i] = p.level_w[i]; da.a0[i] = p.level_a0[i];
        }
        da.A = p.A; da.nc = nc; da.units = 2 + (nc + vp::DEC_CLS - 1) / vp::DEC_CLS; da.n_images = n;
        for (int layout = 0; layout < 2; ++layout) {
            da.layout = layout;
            const size_t count = (size_t)n * (4 + nc) * p.A;
            std::unique_ptr<float[]> head(new float[count]);
            for (int img = 0; img < n; ++img)
                for (int a = 0; a < p.A; ++a)
                    for (int u = 0; u < da.units; ++u) vp::yolo_decode_unit<float>(da, head.get(), (size_t)img, a, u);
            for (size_t q = 0; q < count; ++q) {
                if (!(head[q] == head[q])) return fail("decode", "a NaN in the head");
                sum += (uint64_t)(head[q] * 16.f);
            }
        }
    }
    // fp64 -> fp16 bits: the ends of the range
    const double edge[] = {0.0, -0.0, 5.9604644775390625e-8, 2.98023223876953125e-8, 2.9802322387695316e-8, 65504.0, 65519.9, 65520.0, 1e30, -1e30, 6.103515625e-5, 6.0975551605224609e-5};
    const uint16_t want[] = {0x0000, 0x8000, 0x0001, 0x0000, 0x0001, 0x7bff, 0x7bff, 0x7c00, 0x7c00, 0xfc00, 0x0400, 0x03ff};
    for (size_t i = 0; i < sizeof(edge) / sizeof(edge[0]); ++i)
        if (vp::yolo_f16_bits(edge[i]) != want[i]) return fail("f16_bits", std::to_string(edge[i]));
    std::printf("yolo host ok, checksum %llu\n", (unsigned long long)sum);
    return 0;
}
