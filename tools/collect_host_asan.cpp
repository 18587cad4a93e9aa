// Address / undefined-behaviour check of the host path of the collect stage (csrc/collectgeom.h through vp_dbg_collect_host and vp_collect_bytes): a stand-alone
// program, HOST ONLY, no device is touched.  Every input and the table are heap blocks of exactly the size the contract names (the score block ends with the last
// strided element, the table is vp_collect_bytes long), so a byte read or written past one is a heap overflow the sanitizer reports.  max_records from 0 to beyond
// the total, every optional pointer NULL in turn and all at once, K = 1, 17 and 133, frames outside the table, n at the cap on 64 frames, n = 0.
//
//   for f in <build.py SOURCES>; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=fast -Xarch_host -fsanitize=address,undefined \
//       $([ $f = track.hip -o $f = smooth.hip -o $f = detect.hip -o $f = letterbox.hip ] && echo -ffp-contract=off) -c easy_vitpose_amd/csrc/$f -o $OUT/${f%.hip}.o; done
//                                                                                      # the sanitizer instruments the host side only; the device code is the product's
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/collect_host_asan.cpp -o $OUT/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $OUT/*.o -o $OUT/collect_host_asan && $OUT/collect_host_asan
//
// Prints the number of calls and a checksum of the tables; exit status 0 and no sanitizer report is the pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../include/vitpose_hip.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

template <class T> static T* block(size_t count) { return (T*)malloc(count ? count * sizeof(T) : 1); }

int main() {
    uint64_t sum = 0;
    int calls = 0, refused = 0;
    const int ks[] = {1, 17, 133, 2};
    for (int it = 0; it < 400; ++it) {
        const int K = ks[it % 4], n_frames = it % 7 == 6 ? 64 : 1 + (int)(rnd() % 5);
        const int n = it % 100 == 99 ? VP_COLLECT_MAX_ROWS : (it % 31 == 30 ? 0 : 1 + (int)(rnd() % 90));
        const int stride = 1 + (int)(rnd() % 6);
        // which optional inputs are given: every single NULL, all NULL and all given come round, the rest are random
        const uint32_t given = it < 6 ? ~(1u << it) : (it == 6 ? 0u : (it == 7 ? ~0u : rnd()));
        float* kp = block<float>((size_t)n * K * 3);
        int32_t *ids = block<int32_t>(n), *frame = block<int32_t>(n), *rank = block<int32_t>(n), *status = block<int32_t>(n), *cp = block<int32_t>((size_t)n * 9);
        float* score = block<float>(n ? (size_t)(n - 1) * stride + 1 : 0);
        int total = 0;
        for (int i = 0; i < n; ++i) {
            for (int q = 0; q < 3 * K; ++q) { const uint32_t w = rnd() % 9 ? rnd() : 0x7fc00000u | rnd(); memcpy(kp + (size_t)i * 3 * K + q, &w, 4); }
            ids[i] = (int32_t)(rnd() % 40) - 1;
            frame[i] = (int32_t)(rnd() % (uint32_t)(n_frames + 2)) - 1;
            rank[i] = (int32_t)(rnd() % 5) - 1;
            status[i] = rnd() % 6 ? 0 : 1 + (int32_t)(rnd() % 3);
            score[(size_t)i * stride] = (float)(rnd() & 0xffff) / 65536.f;
            for (int q = 0; q < 9; ++q) cp[(size_t)i * 9 + q] = q >= 1 && q <= 4 && rnd() % 16 == 0 ? INT32_MAX - (int32_t)(rnd() % 100) : (int32_t)(rnd() % 4000) - 50;
            const int f = given & 2 ? frame[i] : 0;
            total += f >= 0 && f < n_frames && !((given & 1) && ids[i] < 0) && !((given & 4) && rank[i] < 0) && !((given & 8) && status[i] != 0);
        }
        // max_records: 0, below, at and beyond the total
        const int picks[] = {0, total / 2, total > 0 ? total - 1 : 0, total, total + 1, total + 7};
        const int max_records = picks[rnd() % 6];
        const int64_t bytes = vp_collect_bytes(n_frames, K, max_records);
        if (bytes < 0) { fprintf(stderr, "vp_collect_bytes refused %d %d %d\n", n_frames, K, max_records); return 1; }
        void* out = nullptr;
        if (posix_memalign(&out, 16, (size_t)bytes)) return 1;   // exactly `bytes`, 16-byte aligned
        memset(out, 0xA5, (size_t)bytes);
        const int rc = vp_dbg_collect_host(kp, n, K, given & 1 ? ids : nullptr, given & 2 ? frame : nullptr, given & 4 ? rank : nullptr, given & 8 ? status : nullptr,
                                           given & 16 ? score : nullptr, stride, given & 32 ? cp : nullptr, n_frames, max_records, out);
        if (rc != VP_OK) { fprintf(stderr, "call %d refused: %s\n", it, vp_last_error(nullptr)); return 1; }
        const int32_t* hdr = (const int32_t*)out;
        if (hdr[n_frames] != total) { fprintf(stderr, "call %d: total %d, expected %d\n", it, hdr[n_frames], total); return 1; }
        ++calls;
        for (int64_t i = 0; i < bytes; ++i) sum = sum * 1099511628211ull + ((const uint8_t*)out)[i];
        free(out); free(kp); free(ids); free(frame); free(rank); free(status); free(cp); free(score);
    }
    // the refusals write nothing and read nothing
    {
        float kp[3] = {0, 0, 0};
        void* out = nullptr;
        if (posix_memalign(&out, 16, 64)) return 1;
        const int bad[][5] = {{-1, 1, 1, 1, 1}, {VP_COLLECT_MAX_ROWS + 1, 1, 1, 1, 1}, {1, 0, 1, 1, 1}, {1, 134, 1, 1, 1}, {1, 1, 0, 1, 1}, {1, 1, 1, 0, 1},
                              {1, 1, 1, VP_COLLECT_MAX_FRAMES + 1, 1}, {1, 1, 1, 1, -1}};   // n, k, score_stride, n_frames, max_records
        for (const auto& b : bad) refused += vp_dbg_collect_host(kp, b[0], b[1], nullptr, nullptr, nullptr, nullptr, nullptr, b[2], nullptr, b[3], b[4], out) == VP_ERR_INVALID;
        refused += vp_dbg_collect_host(nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, 1, 1, out) == VP_ERR_INVALID;
        refused += vp_dbg_collect_host(kp, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, 1, 1, nullptr) == VP_ERR_INVALID;
        refused += vp_dbg_collect_host(kp, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, 1, 1, (char*)out + 4) == VP_ERR_INVALID;
        free(out);
        if (refused != 11) { fprintf(stderr, "%d of 11 refusals\n", refused); return 1; }
    }
    printf("collect_host_asan: %d calls, %d refusals, checksum %016llx\n", calls, refused, (unsigned long long)sum);
    return 0;
}
