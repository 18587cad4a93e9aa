// Address / undefined-behaviour check of the host path of the label stage (csrc/labelgeom.h through vp_dbg_draw_labels_host and vp_dbg_label_text): a stand-alone
// program, HOST ONLY, no device is touched.  Every plane is a heap block of exactly (rows - 1) * pitch + row bytes, so a byte written past a plane's extent is a
// heap overflow the sanitizer reports.  Crowds at the row cap (VP_LABEL_MAX_ROWS), tags at every edge of the frame and wholly off it, coordinates at the usable
// limit and the non-finite values, the largest scale, and the maximal text (#-2147483648: -1000.00) into a buffer of exactly 25 bytes.
//
//   for f in <build.py SOURCES>; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=fast -Xarch_host -fsanitize=address,undefined \
//       -c easy_vitpose_amd/csrc/$f -o $OUT/${f%.hip}.o; done                         # the sanitizer instruments the host side only; the device code is the product's
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/label_host_asan.cpp -o $OUT/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $OUT/*.o -o $OUT/label_host_asan && $OUT/label_host_asan
//
// Prints the number of calls and a checksum of the planes; exit status 0 and no sanitizer report is the pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/vitpose_hip.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffffff) / 16777216.f; }

static float coordinate(int extent) {
    switch (rnd() % 14) {
        case 0: return NAN;
        case 1: return INFINITY;
        case 2: return -INFINITY;
        case 3: return 16383.99f;
        case 4: return -16383.99f;
        case 5: return 16384.f;
        case 6: return -16384.f;
        case 7: return uniform(-16383.f, 16383.f);
        case 8: return rnd() & 1 ? -0.9f : (float)extent - 0.01f;
        case 9: return (float)extent - (float)(rnd() % 80);    // a tag across the far edge
        case 10: return -(float)(rnd() % 1100);                // ... across the near edge, or wholly before it
        default: return uniform(-10.f, (float)extent + 10.f);
    }
}

static float score_value() {
    switch (rnd() % 10) {
        case 0: return NAN;
        case 1: return INFINITY;
        case 2: return -0.f;
        case 3: return -999.99994f;
        case 4: return 999.99994f;
        case 5: return 1000.f;
        case 6: return 1e-45f;
        case 7: return uniform(-1000.f, 1000.f);
        default: return uniform(0.f, 1.f);
    }
}

static int32_t id_value() {
    switch (rnd() % 6) {
        case 0: return INT32_MIN;
        case 1: return INT32_MAX;
        case 2: return -1;
        default: return (int32_t)rnd() - (int32_t)(rnd() & 0xffff);
    }
}

int main() {
    uint8_t colors[3 * 7];
    for (auto& v : colors) v = (uint8_t)rnd();
    uint64_t sum = 0;
    int calls = 0;
    // the text taps first: the longest text fills its 25 bytes exactly
    {
        char* out = (char*)malloc(25);
        const float scores[] = {-999.99994f, 999.99994f, -0.f, 0.125f, NAN, 1e-45f, 1000.f};
        const int32_t ids[] = {INT32_MIN, INT32_MAX, 0, -1, 7};
        for (float s : scores)
            for (int32_t id : ids)
                for (int has = 0; has < 2; ++has) {
                    if (vp_dbg_label_text(id, has, s, out) != VP_OK) { fprintf(stderr, "text refused\n"); return 1; }
                    sum = sum * 1099511628211ull + strlen(out);
                }
        vp_dbg_label_text(INT32_MIN, 1, -999.99994f, out);
        if (strcmp(out, "#-2147483648: -1000.00") != 0) { fprintf(stderr, "maximal text: %s\n", out); return 1; }
        free(out);
        for (int code = -2; code < 18; ++code) sum = sum * 1099511628211ull + vp_dbg_label_glyph(code);
    }
    const int sizes[][2] = {{97, 131}, {64, 96}, {1, 1}, {2, 3}, {9, 33}, {240, 7}, {72, 1064}};
    for (int it = 0; it < 300; ++it) {
        const int n = it % 50 == 49 ? VP_LABEL_MAX_ROWS : 1 + (int)(rnd() % 12);
        vp_image images[2];
        std::vector<uint8_t*> blocks;
        std::vector<size_t> bytes;
        for (int f = 0; f < 2; ++f) {
            const int* hw = sizes[rnd() % 7];
            vp_image& im = images[f];
            im.h = hw[0]; im.w = hw[1]; im.format = (int32_t)(rnd() % 3); im.matrix = (int32_t)(rnd() % 3);
            const int pad = (int)(rnd() % 3) * 5;
            const int planes = im.format == VP_PIX_NV12 ? 2 : 1;
            im.plane[1] = nullptr; im.pitch[1] = 0;
            for (int p = 0; p < planes; ++p) {
                const int64_t row = im.format == VP_PIX_NV12 ? (p ? 2 * ((im.w + 1) / 2) : im.w) : 3 * im.w, rows = p ? (im.h + 1) / 2 : im.h;
                im.pitch[p] = row + pad;
                const size_t b = (size_t)((rows - 1) * im.pitch[p] + row);
                uint8_t* q = (uint8_t*)malloc(b);
                for (size_t i = 0; i < b; ++i) q[i] = (uint8_t)rnd();
                im.plane[p] = q;
                blocks.push_back(q); bytes.push_back(b);
            }
        }
        // rows of exactly the strides the call names: boxes [n, 6] (the tracker's rows, the score in column 4), frame index at stride 3
        std::vector<float> rows((size_t)(n - 1) * 6 + 5);
        std::vector<int32_t> fi((size_t)(n - 1) * 3 + 1), rank(n), ids(n);
        for (int i = 0; i < n; ++i) {
            fi[(size_t)i * 3] = (int32_t)(rnd() % 4) - 1;   // -1 and 2 name no frame
            rank[i] = (int32_t)(rnd() % 4) - 1;
            ids[i] = id_value();
            const vp_image& im = images[fi[(size_t)i * 3] == 1 ? 1 : 0];
            for (int q = 0; q < 4; ++q) rows[(size_t)i * 6 + q] = coordinate(q & 1 ? im.h : im.w);
            rows[(size_t)i * 6 + 4] = score_value();
        }
        vp_label_cfg cfg;
        cfg.scale = (int32_t)(rnd() % 9); cfg.n_colors = 7; cfg.colors = colors; cfg.auto_ink = (int32_t)(rnd() & 1);
        cfg.ink[0] = (uint8_t)rnd(); cfg.ink[1] = (uint8_t)rnd(); cfg.ink[2] = (uint8_t)rnd(); cfg.show_score = (int32_t)(rnd() % 4 != 0);
        const int rc = vp_dbg_draw_labels_host(images, 2, rows.data(), 6, n, fi.data(), 3, rnd() & 1 ? rank.data() : nullptr, rnd() & 1 ? ids.data() : nullptr,
                                               rnd() % 4 ? rows.data() + 4 : nullptr, 6, &cfg);
        if (rc != VP_OK) { fprintf(stderr, "call %d refused: %s\n", it, vp_last_error(nullptr)); return 1; }
        ++calls;
        for (size_t b = 0; b < blocks.size(); ++b) {
            for (size_t i = 0; i < bytes[b]; ++i) sum = sum * 1099511628211ull + blocks[b][i];
            free(blocks[b]);
        }
    }
    printf("label_host_asan: %d calls, checksum %016llx\n", calls, (unsigned long long)sum);
    return 0;
}
