// Address / undefined-behaviour check of the host path of the metrics stage (csrc/metricsgeom.h through vp_dbg_metrics_host and vp_metrics_state_bytes): a
// stand-alone program, HOST ONLY, no device is touched.  Every input, the state and both outputs are heap blocks of exactly the size the contract names (the state
// is vp_metrics_state_bytes long), so a byte read or written past one is a heap overflow the sanitizer reports.  Every optional pointer NULL in turn, all at once
// and in random combinations, n = 0 and n at the cap, K = 1, 17, 133 and 256, n_pck 0..8, auc_steps 0..32, NaN / inf / zero / negative inputs.
//
// Built as tools/collect_host_asan.cpp says in its header, with metrics.hip one more unit without contraction:
//
//   for f in <build.py SOURCES>; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=fast -Xarch_host -fsanitize=address,undefined \
//       $(<f in build.py SOURCE_FLAGS> && echo -ffp-contract=off) -c easy_vitpose_amd/csrc/$f -o $OUT/${f%.hip}.o; done
//                                                                                      # the sanitizer instruments the host side only; the device code is the product's
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/metrics_host_asan.cpp -o $OUT/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $OUT/*.o -o $OUT/metrics_host_asan && $OUT/metrics_host_asan
//
// Prints the number of calls and a checksum of the states; exit status 0 and no sanitizer report is the pass.
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
    for (int it = 0; it < 240; ++it) {
        const int K = ks[it % 4];
        const int n = it % 60 == 59 ? VP_METRICS_MAX_ROWS : (it % 13 == 12 ? 0 : 1 + (int)(rnd() % 200));
        // which optional pointers are given (norm, area, rank, set, dist, oks): every single NULL, all NULL and all given come round, the rest are random
        const uint32_t given = it < 6 ? ~(1u << it) : (it == 6 ? 0u : (it == 7 ? ~0u : rnd()));
        vp_metrics_cfg cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.n_joints = K;
        cfg.n_pck = it % 5 == 0 ? 8 : (int)(rnd() % 9);
        cfg.auc_steps = it % 7 == 0 ? 32 : (int)(rnd() % 33);
        cfg.auc_norm = 30.0;
        cfg.vis_thr = it % 3 ? 0.f : 0.3f;
        cfg.use_oks = it % 4 != 3;
        for (int t = 0; t < 8; ++t) cfg.pck_thr[t] = 0.05f * (float)(t + 1);
        int64_t bytes = -1;
        if (vp_metrics_state_bytes(&cfg, &bytes) != VP_OK || bytes != 8 * (24 + (int64_t)K * (4 + cfg.n_pck + cfg.auc_steps))) {
            fprintf(stderr, "vp_metrics_state_bytes: %lld for K %d n_pck %d auc_steps %d\n", (long long)bytes, K, cfg.n_pck, cfg.auc_steps);
            return 1;
        }
        char* state = block<char>((size_t)bytes);   // exactly `bytes`
        memset(state, 0, (size_t)bytes);
        float *pred = block<float>((size_t)n * K * 3), *gt = block<float>((size_t)n * K * 3), *norm = block<float>((size_t)n * 2), *area = block<float>(n);
        float *sig = block<float>(K), *dist = block<float>((size_t)n * K), *oks = block<float>(n);
        int32_t *rank = block<int32_t>(n), *set = block<int32_t>(n);
        for (int j = 0; j < K; ++j) sig[j] = 0.025f + 0.1f * unit();
        for (int i = 0; i < n; ++i) {
            for (int q = 0; q < 3 * K; ++q) {
                const size_t at = (size_t)i * 3 * K + q;
                gt[at] = q % 3 == 2 ? (float)(rnd() % 3) : 300.f * unit();
                pred[at] = gt[at] + 20.f * (unit() - 0.5f);
                if (rnd() % 500 == 0) pred[at] = rnd() % 2 ? NAN : INFINITY;
                if (rnd() % 900 == 0) gt[at] = NAN;
            }
            norm[2 * i] = rnd() % 20 == 0 ? 0.f : (rnd() % 20 == 0 ? -3.f : 50.f + 300.f * unit());
            norm[2 * i + 1] = rnd() % 20 == 0 ? 0.f : 40.f + 200.f * unit();
            area[i] = rnd() % 15 == 0 ? (rnd() % 2 ? 0.f : NAN) : 2000.f + 60000.f * unit();
            rank[i] = (int32_t)(rnd() % 6) - 1;
            set[i] = (int32_t)(rnd() % 3);
        }
        for (int rep = 0; rep < 2; ++rep) {   // the second call accumulates
            const int rc = vp_dbg_metrics_host(state, &cfg, cfg.use_oks ? sig : nullptr, pred, gt, given & 1 ? norm : nullptr, given & 2 ? area : nullptr,
                                               given & 4 ? rank : nullptr, given & 8 ? set : nullptr, 1, n, given & 16 ? dist : nullptr, given & 32 ? oks : nullptr);
            if (rc != VP_OK) { fprintf(stderr, "call %d refused: %s\n", it, vp_last_error(nullptr)); return 1; }
            ++calls;
        }
        const int64_t* W = (const int64_t*)state;
        if (W[0] != 2 || W[1] != 2 * (int64_t)n || W[2] > W[1]) { fprintf(stderr, "call %d: header %lld %lld %lld\n", it, (long long)W[0], (long long)W[1], (long long)W[2]); return 1; }
        for (int64_t i = 0; i < bytes; ++i) sum = sum * 1099511628211ull + (uint8_t)state[i];
        if (given & 16)
            for (size_t i = 0; i < (size_t)n * K; ++i) { uint32_t w; memcpy(&w, dist + i, 4); sum = sum * 1099511628211ull + w; }
        if (given & 32)
            for (int i = 0; i < n; ++i) { uint32_t w; memcpy(&w, oks + i, 4); sum = sum * 1099511628211ull + w; }
        free(state); free(pred); free(gt); free(norm); free(area); free(sig); free(dist); free(oks); free(rank); free(set);
    }
    // the refusals write nothing and read nothing
    {
        vp_metrics_cfg cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.n_joints = 1;
        float kp[3] = {0, 0, 0};
        char* state = block<char>(8 * 28);
        memset(state, 0, 8 * 28);
        auto call = [&](const vp_metrics_cfg* c, const float* sigmas, const float* p, const float* g, int n, void* st) {
            return vp_dbg_metrics_host(st, c, sigmas, p, g, nullptr, nullptr, nullptr, nullptr, 0, n, nullptr, nullptr) == VP_ERR_INVALID;
        };
        refused += call(nullptr, nullptr, kp, kp, 1, state);
        refused += call(&cfg, nullptr, nullptr, kp, 1, state);
        refused += call(&cfg, nullptr, kp, nullptr, 1, state);
        refused += call(&cfg, nullptr, kp, kp, -1, state);
        refused += call(&cfg, nullptr, kp, kp, VP_METRICS_MAX_ROWS + 1, state);
        refused += call(&cfg, nullptr, kp, kp, 1, nullptr);
        vp_metrics_cfg bad = cfg;
        bad.n_joints = 0; refused += call(&bad, nullptr, kp, kp, 1, state);
        bad.n_joints = 257; refused += call(&bad, nullptr, kp, kp, 1, state);
        bad = cfg; bad.n_pck = 9; refused += call(&bad, nullptr, kp, kp, 1, state);
        bad = cfg; bad.auc_steps = 33; refused += call(&bad, nullptr, kp, kp, 1, state);
        bad = cfg; bad.auc_steps = 1; bad.auc_norm = 0.0; refused += call(&bad, nullptr, kp, kp, 1, state);
        bad = cfg; bad.n_pck = 1; bad.pck_thr[0] = NAN; refused += call(&bad, nullptr, kp, kp, 1, state);
        bad = cfg; bad.vis_thr = INFINITY; refused += call(&bad, nullptr, kp, kp, 1, state);
        bad = cfg; bad.use_oks = 1; refused += call(&bad, nullptr, kp, kp, 1, state);
        float zero_sigma = 0.f;
        refused += call(&bad, &zero_sigma, kp, kp, 1, state);
        int64_t b = 0;
        refused += vp_metrics_state_bytes(nullptr, &b) == VP_ERR_INVALID;
        refused += vp_metrics_state_bytes(&cfg, nullptr) == VP_ERR_INVALID;
        for (int i = 0; i < 8 * 28; ++i)
            if (state[i]) { fprintf(stderr, "a refusal wrote the state\n"); return 1; }
        free(state);
        if (refused != 17) { fprintf(stderr, "%d of 17 refusals\n", refused); return 1; }
    }
    printf("metrics_host_asan: %d calls, %d refusals, checksum %016llx\n", calls, refused, (unsigned long long)sum);
    return 0;
}
