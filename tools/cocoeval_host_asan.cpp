// Address / undefined-behaviour check of the host path of the COCO keypoint evaluator (csrc/cocogeom.h through vp_dbg_cocoeval_update_host,
// vp_dbg_cocoeval_accumulate_host, vp_cocoeval_state_bytes and vp_cocoeval_result_bytes): a stand-alone program, HOST ONLY, no device is touched.  Every input, the
// state, `match` and the result are heap blocks of exactly the size the contract names, so a byte read or written past one is a heap overflow the sanitizer
// reports.  Every optional pointer NULL in turn, all at once and in random combinations; n = 0, g = 0 and both at the cap; n_frames 1 and 256; K = 1, 17, 133 and
// 256; max_records 1 and one short of the total; more than 128 gts in an image; frames out of range; NaN / inf / zero / negative inputs.
//
// Built as tools/metrics_host_asan.cpp says in its header, with cocoeval.hip one more unit without contraction:
//
//   for f in <build.py SOURCES>; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=fast -Xarch_host -fsanitize=address,undefined \
//       $(<f in build.py SOURCE_FLAGS> && echo -ffp-contract=off) -c easy_vitpose_amd/csrc/$f -o $OUT/${f%.hip}.o; done
//                                                                                      # the sanitizer instruments the host side only; the device code is the product's
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/cocoeval_host_asan.cpp -o $OUT/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $OUT/*.o -o $OUT/cocoeval_host_asan && $OUT/cocoeval_host_asan
//
// Prints the number of calls and a checksum of the states and results; exit status 0 and no sanitizer report is the pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../include/vitpose_hip.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static float unit() { return (float)(rnd() & 0xffffff) / 16777216.f; }

template <class T> static T* block(size_t count) { return (T*)malloc(count ? count * sizeof(T) : 1); }

int main() {
    uint64_t sum = 0;
    int calls = 0, refused = 0;
    const int ks[] = {1, 17, 133, 256};
    int64_t result_bytes = 0;
    if (vp_cocoeval_result_bytes(&result_bytes) != VP_OK || result_bytes != 128 + 8 * 3060) { fprintf(stderr, "vp_cocoeval_result_bytes: %lld\n", (long long)result_bytes); return 1; }
    for (int it = 0; it < 200; ++it) {
        const int K = ks[it % 4];
        const bool cap = it % 50 == 49;   // both at the cap
        const int n = cap ? VP_COCOEVAL_MAX_ROWS : (it % 13 == 12 ? 0 : 1 + (int)(rnd() % 300));
        const int g = cap ? VP_COCOEVAL_MAX_ROWS : (it % 11 == 10 ? 0 : 1 + (int)(rnd() % 300));
        const int n_frames = it % 3 == 0 ? 1 : (it % 3 == 1 ? VP_COCOEVAL_MAX_FRAMES : 1 + (int)(rnd() % 40));
        // which optional pointers are given (frame, rank, gt_flags, gt_frame, match): every single NULL, all NULL and all given come round, the rest are random
        const uint32_t given = it < 5 ? ~(1u << it) : (it == 5 ? 0u : (it == 6 ? ~0u : rnd()));
        vp_cocoeval_cfg cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.n_joints = K;
        cfg.max_records = it % 7 == 0 ? 1 : (it % 7 == 1 ? 39 : 2 * 20 * VP_COCOEVAL_MAX_FRAMES);   // 1, one short of two calls of two full images, room for all
        int64_t bytes = -1;
        if (vp_cocoeval_state_bytes(&cfg, &bytes) != VP_OK || bytes != 128 + 16 * (int64_t)cfg.max_records) { fprintf(stderr, "vp_cocoeval_state_bytes: %lld\n", (long long)bytes); return 1; }
        char* state = block<char>((size_t)bytes);   // exactly `bytes`
        memset(state, 0, (size_t)bytes);
        char* result = block<char>((size_t)result_bytes);
        float *kp = block<float>((size_t)n * K * 3), *score = block<float>(n), *gk = block<float>((size_t)g * K * 3), *gb = block<float>((size_t)g * 4), *ga = block<float>(g);
        int32_t *frame = block<int32_t>(n), *rank = block<int32_t>(n), *gflags = block<int32_t>(g), *gframe = block<int32_t>(g), *match = block<int32_t>((size_t)n * 10);
        double* sig = block<double>(K);
        for (int j = 0; j < K; ++j) sig[j] = 0.025 + 0.1 * unit();
        for (int i = 0; i < g; ++i) {
            for (int q = 0; q < 3 * K; ++q) gk[(size_t)i * 3 * K + q] = q % 3 == 2 ? (float)(rnd() % 3) : 300.f * unit();
            if (rnd() % 10 == 0)
                for (int j = 0; j < K; ++j) gk[(size_t)i * 3 * K + 3 * j + 2] = 0.f;   // no labelled joint: the box branch
            if (rnd() % 200 == 0) gk[(size_t)i * 3 * K + rnd() % (3 * K)] = NAN;
            for (int q = 0; q < 4; ++q) gb[4 * i + q] = 200.f * unit();
            ga[i] = rnd() % 15 == 0 ? (rnd() % 3 == 0 ? 0.f : (rnd() % 2 ? NAN : -5.f)) : 500.f + 30000.f * unit();
            gflags[i] = (int32_t)(rnd() % 8 == 0);
            gframe[i] = it % 5 == 4 ? 0 : (int32_t)(rnd() % (n_frames + 2)) - 1;   // every fifth: all in image 0 (more than 128), else some out of range
        }
        for (int i = 0; i < n; ++i) {
            const size_t src = g ? (size_t)(rnd() % g) : 0;
            for (int q = 0; q < 3 * K; ++q) kp[(size_t)i * 3 * K + q] = (g ? gk[src * 3 * K + q] : 300.f * unit()) + 30.f * (unit() - 0.5f) * (float)(rnd() % 3);
            if (rnd() % 100 == 0) kp[(size_t)i * 3 * K + rnd() % (3 * K)] = rnd() % 2 ? NAN : INFINITY;
            score[i] = rnd() % 50 == 0 ? NAN : (float)(rnd() % 32) / 32.f;
            frame[i] = it % 5 == 4 ? 0 : (int32_t)(rnd() % (n_frames + 2)) - 1;
            rank[i] = (int32_t)(rnd() % 6) - 1;
        }
        for (int rep = 0; rep < 2; ++rep) {   // the second call accumulates
            const int rc = vp_dbg_cocoeval_update_host(state, &cfg, sig, kp, score, given & 1 ? frame : nullptr, given & 2 ? rank : nullptr, n, gk, gb, ga, given & 4 ? gflags : nullptr,
                                                       given & 8 ? gframe : nullptr, g, n_frames, given & 16 ? match : nullptr);
            if (rc != VP_OK) { fprintf(stderr, "call %d refused: %s\n", it, vp_last_error(nullptr)); return 1; }
            ++calls;
            if (vp_dbg_cocoeval_accumulate_host(state, &cfg, result) != VP_OK) { fprintf(stderr, "accumulate %d refused: %s\n", it, vp_last_error(nullptr)); return 1; }
            ++calls;
        }
        const int64_t* W = (const int64_t*)state;
        if (W[0] != 2 || W[1] != 2 * (int64_t)n_frames || W[2] != 2 * (int64_t)n || W[3] != W[4] + W[5] || W[4] > cfg.max_records || memcmp(state, result, 128)) {
            fprintf(stderr, "call %d: header %lld %lld %lld %lld %lld %lld\n", it, (long long)W[0], (long long)W[1], (long long)W[2], (long long)W[3], (long long)W[4], (long long)W[5]);
            return 1;
        }
        for (int64_t i = 0; i < bytes; ++i) sum = sum * 1099511628211ull + (uint8_t)state[i];
        for (int64_t i = 0; i < result_bytes; ++i) sum = sum * 1099511628211ull + (uint8_t)result[i];
        if (given & 16)
            for (size_t i = 0; i < (size_t)n * 10; ++i) sum = sum * 1099511628211ull + (uint32_t)match[i];
        free(state); free(result); free(kp); free(score); free(gk); free(gb); free(ga); free(frame); free(rank); free(gflags); free(gframe); free(match); free(sig);
    }
    // the refusals write nothing and read nothing
    {
        vp_cocoeval_cfg cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.n_joints = 1;
        cfg.max_records = 4;
        float kp[3] = {0, 0, 0}, sc[1] = {0}, box[4] = {0, 0, 1, 1}, area[1] = {1};
        double sigma = 0.05, zero = 0.0, nan = NAN;
        char* state = block<char>(128 + 64);
        memset(state, 0, 128 + 64);
        char* result = block<char>((size_t)result_bytes);
        auto call = [&](const vp_cocoeval_cfg* c, const double* s, const float* k, const float* sco, int n, const float* gk, const float* gb, const float* ga, int g, int nf, void* st) {
            return vp_dbg_cocoeval_update_host(st, c, s, k, sco, nullptr, nullptr, n, gk, gb, ga, nullptr, nullptr, g, nf, nullptr) == VP_ERR_INVALID;
        };
        refused += call(nullptr, &sigma, kp, sc, 1, kp, box, area, 1, 1, state);
        refused += call(&cfg, nullptr, kp, sc, 1, kp, box, area, 1, 1, state);
        refused += call(&cfg, &zero, kp, sc, 1, kp, box, area, 1, 1, state);
        refused += call(&cfg, &nan, kp, sc, 1, kp, box, area, 1, 1, state);
        refused += call(&cfg, &sigma, nullptr, sc, 1, kp, box, area, 1, 1, state);
        refused += call(&cfg, &sigma, kp, nullptr, 1, kp, box, area, 1, 1, state);
        refused += call(&cfg, &sigma, kp, sc, 1, nullptr, box, area, 1, 1, state);
        refused += call(&cfg, &sigma, kp, sc, 1, kp, nullptr, area, 1, 1, state);
        refused += call(&cfg, &sigma, kp, sc, 1, kp, box, nullptr, 1, 1, state);
        refused += call(&cfg, &sigma, kp, sc, -1, kp, box, area, 1, 1, state);
        refused += call(&cfg, &sigma, kp, sc, VP_COCOEVAL_MAX_ROWS + 1, kp, box, area, 1, 1, state);
        refused += call(&cfg, &sigma, kp, sc, 1, kp, box, area, -1, 1, state);
        refused += call(&cfg, &sigma, kp, sc, 1, kp, box, area, VP_COCOEVAL_MAX_ROWS + 1, 1, state);
        refused += call(&cfg, &sigma, kp, sc, 1, kp, box, area, 1, 0, state);
        refused += call(&cfg, &sigma, kp, sc, 1, kp, box, area, 1, VP_COCOEVAL_MAX_FRAMES + 1, state);
        refused += call(&cfg, &sigma, kp, sc, 1, kp, box, area, 1, 1, nullptr);
        vp_cocoeval_cfg bad = cfg;
        bad.n_joints = 0; refused += call(&bad, &sigma, kp, sc, 1, kp, box, area, 1, 1, state);
        bad.n_joints = 257; refused += call(&bad, &sigma, kp, sc, 1, kp, box, area, 1, 1, state);
        bad = cfg; bad.max_records = 0; refused += call(&bad, &sigma, kp, sc, 1, kp, box, area, 1, 1, state);
        bad.max_records = VP_COCOEVAL_MAX_RECORDS + 1; refused += call(&bad, &sigma, kp, sc, 1, kp, box, area, 1, 1, state);
        refused += vp_dbg_cocoeval_accumulate_host(state, &cfg, nullptr) == VP_ERR_INVALID;
        refused += vp_dbg_cocoeval_accumulate_host(nullptr, &cfg, result) == VP_ERR_INVALID;
        refused += vp_dbg_cocoeval_accumulate_host(state, nullptr, result) == VP_ERR_INVALID;
        int64_t b = 0;
        refused += vp_cocoeval_state_bytes(nullptr, &b) == VP_ERR_INVALID;
        refused += vp_cocoeval_state_bytes(&cfg, nullptr) == VP_ERR_INVALID;
        refused += vp_cocoeval_result_bytes(nullptr) == VP_ERR_INVALID;
        for (int i = 0; i < 128 + 64; ++i)
            if (state[i]) { fprintf(stderr, "a refusal wrote the state\n"); return 1; }
        ((int64_t*)state)[4] = 5;   // a records word beyond max_records is refused, not followed
        refused += vp_dbg_cocoeval_accumulate_host(state, &cfg, result) == VP_ERR_INVALID;
        free(state); free(result);
        if (refused != 27) { fprintf(stderr, "%d of 27 refusals\n", refused); return 1; }
    }
    printf("cocoeval_host_asan: %d calls, %d refusals, checksum %016llx\n", calls, refused, (unsigned long long)sum);
    return 0;
}
