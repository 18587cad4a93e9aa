// Address / undefined-behaviour check of the host path of the keypoint smoother (csrc/eurogeom.h through vp_dbg_smooth_host): a stand-alone program, HOST ONLY,
// no device is touched.  The state blob, the keypoint rows, the id / stream / rank arrays and every output are heap blocks of exactly the documented size, so a
// byte read or written past one is a heap overflow the sanitizer reports; the calls run tables to the capacity (129 ids on a stream), duplicate ids, non-finite
// rows, absent rows, stream indices outside the table, partial step masks, rank masks, n = 0 ageing calls, in-place calls, both missing policies, K from 1 to 1024
// and every refusal.
//
//   for f in <build.py SOURCES>; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=fast -Xarch_host -fsanitize=address,undefined \
//       $([ $f = track.hip -o $f = smooth.hip ] && echo -ffp-contract=off) -c easy_vitpose_amd/csrc/$f -o $OUT/${f%.hip}.o; done     # the sanitizer instruments the host side only; the device code is the product's
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/smooth_host_asan.cpp -o $OUT/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $OUT/*.o -o $OUT/smooth_host_asan && $OUT/smooth_host_asan
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
    int calls = 0, refused = 0;
    const int stream_counts[] = {1, 2, 5, 64};
    const int joints[] = {1, 17, 133, 1024};
    for (int round = 0; round < 16; ++round) {
        const int ns = stream_counts[round % 4], K = joints[(round / 4) % 4];
        const int crowd = K == 1024 ? 3 : (round % 3 == 0 ? 129 : (round % 3 == 1 ? 40 : 6));   // persons per stream
        const int cap = ns * crowd + 4;
        vp_smooth_cfg cfg{1.7, round & 1 ? 0.3 : 0.0, round & 2 ? 30.0 : 59.94, (int32_t)(rnd() % 4), ns, K, cap, round & 1};
        int64_t bytes = 0;
        if (vp_smoother_state_bytes(&cfg, &bytes) != VP_OK) return 1;
        void* state = calloc(1, (size_t)bytes);
        for (int frame = 0; frame < 8; ++frame) {
            int n = 0;
            const bool empty = rnd() % 5 == 0;
            int want = 0;
            for (int i = 0; i < cap && !empty; ++i) want += rnd() % 8 != 0;
            float* kp = (float*)malloc((size_t)want * K * 3 * sizeof(float) + (want ? 0 : 1));
            int32_t* ids = (int32_t*)malloc((size_t)want * 4 + (want ? 0 : 1));
            int32_t* st = (int32_t*)malloc((size_t)want * 4 + (want ? 0 : 1));
            int32_t* rk = (int32_t*)malloc((size_t)want * 4 + (want ? 0 : 1));
            for (n = 0; n < want; ++n) {
                const int person = (int)(rnd() % (uint32_t)(ns * crowd));
                float* r = kp + (size_t)n * K * 3;
                for (int q = 0; q < 3 * K; ++q) r[q] = rnd() % 30 == 0 ? 0.f : uniform(-5.f, 600.f);
                ids[n] = person / ns;   // repeats within a call are the duplicates
                st[n] = person % ns;
                rk[n] = rnd() % 6 == 0 ? -1 : (int32_t)(rnd() % 4);
                switch (rnd() % 40) {
                    case 0: r[3 * (rnd() % K) + rnd() % 2] = NAN; break;
                    case 1: r[3 * (rnd() % K) + rnd() % 2] = INFINITY; break;
                    case 2: r[3 * (rnd() % K) + 2] = NAN; break;          // a confidence: no reason to skip
                    case 3: ids[n] = -1; st[n] = -1; break;               // an absent row
                    case 4: st[n] = rnd() & 1 ? -3 : ns + (int32_t)(rnd() % 3); break;
                    default: break;
                }
            }
            uint64_t mask = ns == 64 ? ~0ull : (1ull << ns) - 1ull;
            if (rnd() % 3 == 0) mask &= ((uint64_t)rnd() << 32) | rnd();
            double* te = (double*)malloc((size_t)ns * sizeof(double));
            for (int s = 0; s < ns; ++s) te[s] = 0.5 * (double)(1 + rnd() % 6);
            const bool in_place = rnd() % 3 == 0;
            float* out = in_place ? kp : (float*)malloc((size_t)n * K * 3 * sizeof(float) + (n ? 0 : 1));
            int32_t* flags = (int32_t*)malloc((size_t)ns * 4);
            const int rc = vp_dbg_smooth_host(state, &cfg, n ? kp : nullptr, n ? ids : nullptr, ns == 1 && (rnd() & 1) ? nullptr : st, rnd() & 1 ? rk : nullptr, n, mask,
                                              rnd() % 4 ? te : nullptr, n ? out : nullptr, rnd() % 4 ? flags : nullptr);
            if (rc != VP_OK) { fprintf(stderr, "call %d refused: %s\n", calls, vp_last_error(nullptr)); return 1; }
            ++calls;
            for (size_t i = 0; i < (size_t)n * K * 3; ++i) {
                uint32_t u;
                memcpy(&u, out + i, 4);
                sum = sum * 1099511628211ull + u;
            }
            if (!in_place) free(out);
            free(kp); free(ids); free(st); free(rk); free(te); free(flags);
        }
        for (int64_t i = 0; i < bytes; ++i) sum = sum * 1099511628211ull + ((const uint8_t*)state)[i];
        // the refusals on the same exact-size blocks: nothing may be read or written
        {
            float* kp = (float*)malloc((size_t)K * 3 * sizeof(float));
            int32_t id = 1;
            double bad_te[64];
            for (int s = 0; s < 64; ++s) bad_te[s] = s == ns - 1 ? 0.0 : 1.0;
            vp_smooth_cfg c2 = cfg;
            c2.missing = 2;
            refused += vp_dbg_smooth_host(state, &c2, kp, &id, nullptr, nullptr, 1, 1, nullptr, kp, nullptr) == VP_ERR_INVALID;
            refused += vp_dbg_smooth_host(state, nullptr, kp, &id, nullptr, nullptr, 1, 1, nullptr, kp, nullptr) == VP_ERR_INVALID;
            refused += vp_dbg_smooth_host(state, &cfg, nullptr, &id, nullptr, nullptr, 1, 1, nullptr, kp, nullptr) == VP_ERR_INVALID;
            refused += vp_dbg_smooth_host(state, &cfg, kp, &id, nullptr, nullptr, cap + 1, 1, nullptr, kp, nullptr) == VP_ERR_INVALID;
            refused += vp_dbg_smooth_host(state, &cfg, kp, &id, nullptr, nullptr, -1, 1, nullptr, kp, nullptr) == VP_ERR_INVALID;
            refused += vp_dbg_smooth_host(state, &cfg, kp, &id, nullptr, nullptr, 1, 1, bad_te, kp, nullptr) == VP_ERR_INVALID;
            if (ns < 64) refused += vp_dbg_smooth_host(state, &cfg, kp, &id, nullptr, nullptr, 1, 1ull << ns, nullptr, kp, nullptr) == VP_ERR_INVALID;
            else ++refused;
            free(kp);
        }
        for (int64_t i = 0; i < bytes; ++i) sum = sum * 1099511628211ull + ((const uint8_t*)state)[i];
        free(state);
    }
    if (refused != 16 * 7) { fprintf(stderr, "%d of %d refusals\n", refused, 16 * 7); return 1; }
    printf("smooth_host_asan: %d calls, %d refusals, checksum %016llx\n", calls, refused, (unsigned long long)sum);
    return 0;
}
