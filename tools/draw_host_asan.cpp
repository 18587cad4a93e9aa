// Address / undefined-behaviour check of the host path of the skeleton overlay (csrc/drawgeom.h through vp_dbg_draw_host): a stand-alone program, HOST ONLY, no
// device is touched.  Every plane is a heap block of exactly (rows - 1) * pitch + row bytes, so a byte written past a plane's extent is a heap overflow the
// sanitizer reports; coordinates are drawn from far outside the frame, the usable limit and the non-finite values.
//
//   for f in <build.py SOURCES>; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=fast -Xarch_host -fsanitize=address,undefined \
//       -c easy_vitpose_amd/csrc/$f -o $OUT/${f%.hip}.o; done                         # the sanitizer instruments the host side only; the device code is the product's
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/draw_host_asan.cpp -o $OUT/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $OUT/*.o -o $OUT/draw_host_asan && $OUT/draw_host_asan
//
// Prints the number of calls and a checksum of the planes; exit status 0 and no sanitizer report is the pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/vitpose_hip.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffffff) / 16777216.f; }

static float coordinate(int extent) {
    switch (rnd() % 12) {
        case 0: return NAN;
        case 1: return INFINITY;
        case 2: return -INFINITY;
        case 3: return 16383.99f;
        case 4: return -16383.99f;
        case 5: return 16384.f;
        case 6: return -16384.f;
        case 7: return uniform(-16383.f, 16383.f);
        case 8: return rnd() & 1 ? -0.9f : (float)extent - 0.01f;
        default: return uniform(-10.f, (float)extent + 10.f);
    }
}

int main() {
    const int K = 17, n = 6;
    std::vector<uint8_t> limbs;
    for (int l = 0; l < 40; ++l) { limbs.push_back((uint8_t)(rnd() % K)); limbs.push_back((uint8_t)(rnd() % K)); }
    uint8_t pc[3 * 5], lc[3 * 3];
    for (auto& v : pc) v = (uint8_t)rnd();
    for (auto& v : lc) v = (uint8_t)rnd();
    uint64_t sum = 0;
    int calls = 0;
    const int sizes[][2] = {{97, 131}, {64, 96}, {1, 1}, {2, 3}, {9, 33}, {240, 7}};
    for (int it = 0; it < 400; ++it) {
        vp_image images[2];
        std::vector<uint8_t*> blocks;
        std::vector<size_t> bytes;
        for (int f = 0; f < 2; ++f) {
            const int* hw = sizes[rnd() % 6];
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
        std::vector<float> kp((size_t)n * K * 3), boxes((size_t)n * 4);
        std::vector<int32_t> fi(n), rank(n), ids(n);
        for (int i = 0; i < n; ++i) {
            fi[i] = (int32_t)(rnd() % 4) - 1;   // -1 and 2 name no frame
            rank[i] = (int32_t)(rnd() % 4) - 1;
            ids[i] = (int32_t)rnd();
            const vp_image& im = images[fi[i] == 1 ? 1 : 0];
            for (int j = 0; j < K; ++j) {
                kp[((size_t)i * K + j) * 3] = coordinate(im.h);
                kp[((size_t)i * K + j) * 3 + 1] = coordinate(im.w);
                kp[((size_t)i * K + j) * 3 + 2] = rnd() % 8 ? uniform(0.f, 1.f) : NAN;
            }
            for (int q = 0; q < 4; ++q) boxes[(size_t)i * 4 + q] = coordinate(q & 1 ? im.h : im.w);
        }
        vp_draw_cfg cfg{uniform(0.f, 0.6f), (int32_t)(rnd() % 65), 1 + (int32_t)(rnd() % 16), 40, limbs.data(), 5, pc, 3, lc};
        const int rc = vp_dbg_draw_host(images, 2, kp.data(), n, K, fi.data(), 1, rnd() & 1 ? rank.data() : nullptr, rnd() & 1 ? ids.data() : nullptr,
                                        rnd() & 1 ? boxes.data() : nullptr, 4, &cfg);
        if (rc != VP_OK) { fprintf(stderr, "call %d refused: %s\n", it, vp_last_error(nullptr)); return 1; }
        ++calls;
        for (size_t b = 0; b < blocks.size(); ++b) {
            for (size_t i = 0; i < bytes[b]; ++i) sum = sum * 1099511628211ull + blocks[b][i];
            free(blocks[b]);
        }
    }
    printf("draw_host_asan: %d calls, checksum %016llx\n", calls, (unsigned long long)sum);
    return 0;
}
