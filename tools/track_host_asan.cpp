// Address / undefined-behaviour check of the host path of the box tracker (csrc/sortgeom.h through vp_dbg_track_host and vp_dbg_lsap(-1)): a stand-alone program,
// HOST ONLY, no device is touched.  The state blob, the detection rows and every output are heap blocks of exactly the documented size, so a byte read or written
// past one is a heap overflow the sanitizer reports; the calls run crowded streams to the capacity (more than VP_TRACK_MAX detections, births at VP_TRACK_MAX
// live tracks), non-finite rows, stream indices outside the table, zero-area boxes, partial step masks, n_out from 0 on, and assignment matrices with NaN entries.
//
//   for f in <build.py SOURCES>; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=fast -Xarch_host -fsanitize=address,undefined \
//       $([ $f = track.hip ] && echo -ffp-contract=off) -c easy_vitpose_amd/csrc/$f -o $OUT/${f%.hip}.o; done                         # the sanitizer instruments the host side only; the device code is the product's
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/track_host_asan.cpp -o $OUT/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $OUT/*.o -o $OUT/track_host_asan && $OUT/track_host_asan
//
// Prints the number of calls and a checksum of the outputs; exit status 0 and no sanitizer report is the pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../include/vitpose_hip.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffffff) / 16777216.f; }

int main() {
    uint64_t sum = 0;
    int calls = 0;
    const int stream_counts[] = {1, 2, 5, 64};
    for (int round = 0; round < 12; ++round) {
        const int ns = stream_counts[round % 4];
        vp_track_cfg cfg{(int32_t)(rnd() % 4), (int32_t)(rnd() % 4), round & 1 ? 0.3f : 0.05f, ns};
        int64_t bytes = 0;
        if (vp_tracker_state_bytes(ns, &bytes) != VP_OK) return 1;
        void* state = calloc(1, (size_t)bytes);
        const int crowd = round % 3 == 0 ? 140 : (round % 3 == 1 ? 60 : 9);   // persons per stream
        float* base = (float*)malloc((size_t)ns * crowd * 4 * sizeof(float));
        for (int i = 0; i < ns * crowd; ++i) {
            const float x = uniform(0.f, 600.f), y = uniform(0.f, 300.f);
            base[4 * i] = x; base[4 * i + 1] = y; base[4 * i + 2] = x + uniform(20.f, 90.f); base[4 * i + 3] = y + uniform(40.f, 200.f);
        }
        for (int frame = 0; frame < 10; ++frame) {
            const int stride = 5 + (int)(rnd() % 3);
            int n = 0;
            const int cap = ns * crowd;
            float* dets = (float*)malloc(((size_t)(cap > 0 ? cap - 1 : 0) * stride + 5) * sizeof(float));
            int32_t* fi = (int32_t*)malloc((size_t)cap * sizeof(int32_t));
            const bool empty = rnd() % 5 == 0;
            for (int i = 0; i < cap && !empty; ++i) {
                if (rnd() % 8 == 0) continue;   // a miss
                float* d = dets + (size_t)n * stride;
                for (int q = 0; q < 4; ++q) d[q] = base[4 * i + q] + uniform(-3.f, 3.f) + 2.f * (float)frame;
                d[4] = uniform(0.3f, 0.95f);
                switch (rnd() % 40) {
                    case 0: d[rnd() % 5] = NAN; break;
                    case 1: d[rnd() % 5] = INFINITY; break;
                    case 2: d[2] = d[0]; break;                 // zero width
                    case 3: d[3] = d[1]; d[2] = d[0]; break;    // a point
                    default: break;
                }
                fi[n] = i / crowd;
                if (rnd() % 50 == 0) fi[n] = rnd() & 1 ? -1 : ns + (int32_t)(rnd() % 3);
                ++n;
            }
            uint64_t mask = ns == 64 ? ~0ull : (1ull << ns) - 1ull;
            if (rnd() % 3 == 0) mask &= ((uint64_t)rnd() << 32) | rnd();
            const int n_out = (int)(rnd() % 4) == 0 ? (int)(rnd() % 8) : ns * 128;
            float* rows = (float*)malloc((size_t)n_out * 6 * sizeof(float) + 1);
            int32_t* ids = (int32_t*)malloc((size_t)n_out * 4 + 1);
            int32_t* st = (int32_t*)malloc((size_t)n_out * 4 + 1);
            int32_t* count = (int32_t*)malloc((size_t)(ns + 1) * 4);
            int32_t* flags = (int32_t*)malloc((size_t)ns * 4);
            const int rc = vp_dbg_track_host(state, &cfg, n ? dets : nullptr, stride, ns == 1 && (rnd() & 1) ? nullptr : fi, n, mask, rows, ids, st, n_out, count,
                                             rnd() % 4 ? flags : nullptr);
            if (rc != VP_OK) { fprintf(stderr, "call %d refused: %s\n", calls, vp_last_error(nullptr)); return 1; }
            ++calls;
            for (int i = 0; i < n_out; ++i) sum = sum * 1099511628211ull + (uint64_t)(uint32_t)ids[i] + (uint64_t)(uint32_t)st[i];
            for (int s = 0; s <= ns; ++s) sum = sum * 1099511628211ull + (uint64_t)(uint32_t)count[s];
            free(dets); free(fi); free(rows); free(ids); free(st); free(count); free(flags);
        }
        for (int64_t i = 0; i < bytes; ++i) sum = sum * 1099511628211ull + ((const uint8_t*)state)[i];
        free(state); free(base);
    }
    const int sizes[] = {1, 2, 7, 64, 65, 128};
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b)
            for (int kind = 0; kind < 3; ++kind) {
                const int nd = sizes[a], nt = sizes[b];
                double* iou = (double*)malloc((size_t)nd * nt * sizeof(double));
                for (int i = 0; i < nd * nt; ++i) {
                    iou[i] = rnd() % 3 == 0 || kind == 1 ? (double)uniform(0.f, 1.f) : 0.0;
                    if (kind == 2 && rnd() % 16 == 0) iou[i] = NAN;
                }
                int32_t* out = (int32_t*)malloc((size_t)nd * 4);
                if (vp_dbg_lsap(-1, iou, nd, nt, 0.3f, out) != VP_OK) { fprintf(stderr, "lsap %d x %d refused: %s\n", nd, nt, vp_last_error(nullptr)); return 1; }
                ++calls;
                for (int d = 0; d < nd; ++d) {
                    if (out[d] < -1 || out[d] >= nt) { fprintf(stderr, "lsap %d x %d: pair out of range\n", nd, nt); return 1; }
                    sum = sum * 1099511628211ull + (uint64_t)(uint32_t)out[d];
                }
                free(iou); free(out);
            }
    printf("track_host_asan: %d calls, checksum %016llx\n", calls, (unsigned long long)sum);
    return 0;
}
