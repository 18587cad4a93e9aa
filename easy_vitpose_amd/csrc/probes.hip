// Measurement code of the tools library (libvitpose_hip_tools.so) only: calibration micro-benchmarks and issue / store / placement probes.
// No plan can launch any of these kernels, so the product library does not carry them (easy_vitpose_amd/build.py TOOLS_SOURCES).
#include "common.h"
#include "kernels.h"

// ---------------------------------------------------------------------------
// Calibration micro-benchmarks (tools/ only): what this box's matrix pipe and HBM
// deliver, measured with the same compiler and launch path as the product kernels.
namespace vp {

template <int SHAPE>
__global__ __launch_bounds__(256, 2) void peak_mfma_kernel(float* out, int iters) {
    u32x4 a = {0x3c003c00u + threadIdx.x, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u};
    u32x4 b = {0x38003800u, 0x38003800u + threadIdx.x, 0x38003800u, 0x38003800u};
    if (SHAPE == 16) {
        f32x4 acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = mfma16<F16>(a, b, acc[i]);
        }
        f32x4 s = acc[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) s += acc[i];
        if (s[0] == 12345.f) out[threadIdx.x] = s[1];
    } else {
        typedef __attribute__((ext_vector_type(16))) float f32x16;
        f32x16 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc[i], 0, 0, 0);
        }
        if (acc[0][0] + acc[1][1] + acc[2][2] + acc[3][3] == 12345.f) out[threadIdx.x] = acc[0][1];
    }
}

__global__ __launch_bounds__(256) void peak_copy_kernel(const f32x4* __restrict__ in, f32x4* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = in[i];
}

// HBM ceiling, calibrated properly (peak_copy_kernel above keeps ONE 16-byte load in flight per lane and reads 4.6 TB/s,
// the guide's float4 copy 6.29).  A persistent grid walks chunks of 256 lanes x U x 16 bytes; the U loads of a chunk are issued back to
// back (U x 16 bytes in flight per lane, each wave instruction = 1 KiB contiguous), then the U stores.  MODE 0 = copy (n float4 in, n out),
// 1 = read only (the sum of the data is kept alive by a never-true store), 2 = write only.  NT = non-temporal loads / stores.
template <int MODE, int U, bool NT>
__global__ __launch_bounds__(256) void peak_stream_kernel(const u32x4* __restrict__ in, u32x4* __restrict__ out, size_t n, uint32_t* sink) {
    const size_t chunk = (size_t)256 * U;
    const size_t nchunks = n / chunk;
    u32x4 keep = {0u, 0u, 0u, 0u};
    u32x4 fill = {threadIdx.x, 1u, 2u, 3u};
    for (size_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const size_t base = c * chunk + threadIdx.x;
        u32x4 v[U];
        if (MODE != 2) {
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = NT ? __builtin_nontemporal_load(in + base + (size_t)u * 256) : in[base + (size_t)u * 256];
        }
        if (MODE == 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) keep ^= v[u];
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const u32x4 w = MODE == 2 ? fill : v[u];
                if (NT) __builtin_nontemporal_store(w, out + base + (size_t)u * 256);
                else out[base + (size_t)u * 256] = w;
            }
        }
    }
    if (MODE == 1 && (keep[0] ^ keep[1] ^ keep[2] ^ keep[3]) == 0x12345677u) sink[threadIdx.x] = keep[0];
}

// VALU issue-rate probe: per round 16 independent fp32 multiply-adds per lane as 16 v_fma_f32 (PK = 0) or as 8
// v_pk_fma_f32 on register pairs (PK = 1); NW waves per workgroup, one workgroup per CU; nothing else in the loop.  Is the packed form a
// throughput gain on this chip where no MFMA issues beside it (a GEMM epilogue)?
template <int NW, int PK>
__global__ __launch_bounds__(NW * 64, 1) void valu_probe_kernel(int iters, float* sink) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    f32x2 a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = f32x2{1.0f + 0.001f * (float)(threadIdx.x + i), 0.5f + 0.002f * (float)(threadIdx.x + i)};
    const f32x2 m = {1.0001f, 0.9999f}, c = {0.25f, -0.25f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (PK) {
                    asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(m), "v"(c));
                } else {
                    asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i][0]) : "v"(m[0]), "v"(c[0]));
                    asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i][1]) : "v"(m[1]), "v"(c[1]));
                }
            }
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += a[i][0] + a[i][1];
    if (s == 12345.f) sink[threadIdx.x] = s;
}

// Where do the workgroups of a launch land?  Every workgroup records HW_REG_HW_ID, HW_REG_XCC_ID and the time it started (tools/hwid_probe.py):
// which wave slots / CU / XCD two co-resident 512-thread workgroups of a 2-per-CU launch get.
__global__ void hwid_probe_kernel(uint32_t* out, int spin) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (threadIdx.x == 0) {
        const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);     // HW_REG_HW_ID, 32 bits
        const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 20);   // HW_REG_XCC_ID
        const unsigned long long t = __builtin_readcyclecounter();
        out[4 * blockIdx.x + 0] = hw;
        out[4 * blockIdx.x + 1] = xcc;
        out[4 * blockIdx.x + 2] = (uint32_t)t;
        out[4 * blockIdx.x + 3] = (uint32_t)(t >> 32);
        ((volatile char*)smem)[0] = 1;
    }
    for (int i = 0; i < spin; ++i) __builtin_amdgcn_s_sleep(64);   // stay resident so that the first round of workgroups fills the chip
}

hipError_t hwid_probe_launch(uint32_t* d_out, int blocks, int threads, int lds_bytes, int spin, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void*)hwid_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hwid_probe_kernel, dim3(blocks), dim3(threads), lds_bytes, s, d_out, spin);
    return hipGetLastError();
}

// LDS-DMA ceiling: every wave streams 1 KiB pieces global -> LDS (global_load_lds_dwordx4) from an L2-resident
// source, DEPTH pieces in flight, nothing else.  blocks_per_cu x 256 threads, 64 KiB LDS ring per block.
template <int DEPTH>
__global__ __launch_bounds__(256) void peak_glds_kernel(const char* __restrict__ src, size_t src_bytes, int iters, float* sink) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t stride = (size_t)gridDim.x * 4 * 1024;
    size_t off = ((size_t)blockIdx.x * 4 + wave) * 1024;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            glds16(src + (off & (src_bytes - 1)) + lane * 16, smem + ((wave * DEPTH + d) & 63) * 1024);   // src_bytes is a power of two
            off += stride;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (iters < 0) sink[threadIdx.x] = ((float*)smem)[threadIdx.x];
}

// Issue-interplay probe (tools/issue_probe.py): every wave runs `iters` rounds of 16 independent MFMAs (256 matrix-pipe cycles)
// and, per round, optionally (mode bit 0) ONE 16-byte-per-lane global store to a streaming address, (bit 1) ONE 1 KiB LDS-DMA
// load with 8 kept in flight, (bit 2) 48 independent VALU FMAs, (bit 3) 4 stores instead of 1.  NW waves per workgroup, one
// workgroup per CU: NW = 4 -> one wave per SIMD, NW = 8 -> two.  What a store / DMA / VALU block costs a wave whose matrix
// pipe is otherwise saturated is the difference to mode 0.
template <int NW, int mode>
__global__ __launch_bounds__(NW * 64, 1) void issue_probe_kernel(int iters, char* __restrict__ dst, const char* __restrict__ src,
                                                                 size_t mask, float* sink) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32x4 a = {0x3c003c00u + threadIdx.x, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u};
    u32x4 b = {0x38003800u, 0x38003800u + threadIdx.x, 0x38003800u, 0x38003800u};
    f32x4 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = 1.0f + 0.001f * (float)(lane + i);
    size_t off = ((size_t)(blockIdx.x * NW + wave) * 1024 * 64) & mask;
    u32x4 data = {(uint32_t)lane, 1u, 2u, 3u};
    if (mode & 2) {
#pragma unroll
        for (int d = 0; d < 8; ++d) glds16(src + ((off + d * 1024) & mask) + lane * 16, smem + ((wave * 8 + d) & 127) * 1024);
    }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            acc[i] = mfma16<F16>(a, b, acc[i]);
            if (mode & 4) {
#pragma unroll
                for (int q = 0; q < 3; ++q) f[(i * 3 + q) & 7] = fmaf(f[(i * 3 + q) & 7], 1.0001f, 0.5f);
            }
            if (i == 3 && (mode & 1)) {
                *(u32x4*)(dst + off + lane * 16) = data;
                if (mode & 8) {
                    *(u32x4*)(dst + ((off + 1024) & mask) + lane * 16) = data;
                    *(u32x4*)(dst + ((off + 2048) & mask) + lane * 16) = data;
                    *(u32x4*)(dst + ((off + 3072) & mask) + lane * 16) = data;
                }
            }
            if (i == 9 && (mode & 2)) {
                glds16(src + off + lane * 16, smem + ((wave * 8 + (it & 7)) & 127) * 1024);
                asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
            }
        }
        off = (off + 4096) & mask;
        data[1] += 1u;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    f32x4 s4 = acc[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) s4 += acc[i];
    float fs = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) fs += f[i];
    if (s4[0] + fs == 12345.f) sink[threadIdx.x] = s4[1] + ((float*)smem)[threadIdx.x];
}

// the same MFMA work per round as issue_probe_kernel mode 0 in the 32x32x16 shape (8 MFMAs of 32 matrix-pipe cycles), DEP = number
// of independent accumulators (8: no dependent pair closer than 8 MFMAs; 4 / 2: dependent issue distance 4 / 2)
template <int NW, int DEP>
__global__ __launch_bounds__(NW * 64, 1) void issue_probe32_kernel(int iters, float* sink) {
    typedef __attribute__((ext_vector_type(16))) float f32x16;
    u32x4 a = {0x3c003c00u + threadIdx.x, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u};
    u32x4 b = {0x38003800u, 0x38003800u + threadIdx.x, 0x38003800u, 0x38003800u};
    f32x16 acc[DEP];
#pragma unroll
    for (int i = 0; i < DEP; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            acc[i % DEP] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc[i % DEP], 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < DEP; ++i) s += acc[i][0] + acc[i][5];
    if (s == 12345.f) sink[threadIdx.x] = s;
}

// kind 0: MFMA 16x16x32 f16, 1: MFMA 32x32x16 f16 (returns TFLOP/s); 2: float4 copy (returns TB/s read+write);
// 170 + (0 | 1 | 2: 8 / 4 / 2 independent accumulators) (+ 4: two waves per SIMD): the 32x32x16 probe, nanoseconds per round
// 100 + mode (+ 32: two waves per SIMD; mode bit 4: 1 MiB = L2-resident buffers): issue probe, returns nanoseconds per round
// 3 / 4 / 5 / 6: LDS-DMA stream from a 32 MiB / 1 GiB / 2 MiB / 256 KiB source, 2 blocks per CU (TB/s into LDS)
// Store-path probe (tools/store_probe.py): every wave issues ROUNDS x 16 stores of 16 bytes per lane, the way a gemm8 epilogue does (one 128 x 64
// block of 16-bit values per wave and "tile" = 16 KiB), into its own region of a buffer that is either small (stays in L2) or 1 GiB.
// PAT 0: a store instruction = 1 KiB contiguous; 1: 16 rows x 64 contiguous bytes at a row stride (4 lanes of a row adjacent);
// 2: 16 rows x four 16-byte pieces 32 bytes apart (the round-2/3 epilogue: a lane's 32 bytes of a row leave as two stores).
template <int PAT>
__global__ void store_probe_kernel(char* __restrict__ dst, size_t wave_bytes, size_t mask, int rounds, int row_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    const size_t base = ((size_t)blockIdx.x * nw + wave) * wave_bytes;
    const int frow = lane & 15, fg = lane >> 4;
    u32x4 v = {(uint32_t)lane, 1u, 2u, 3u};
    for (int r = 0; r < rounds; ++r) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {   // i = (row group J, half h)
            const int J = i >> 1, h = i & 1;
            size_t off;
            if (PAT == 0) off = (size_t)i * 1024 + lane * 16;
            else if (PAT == 1) off = (size_t)(J * 16 + frow) * row_stride + h * 64 + fg * 16;
            else off = (size_t)(J * 16 + frow) * row_stride + fg * 32 + h * 16;
            off = (base + (size_t)r * 16384 + off) & mask;
            *(u32x4*)(dst + off) = v;
            v[1] += 1;
        }
    }
}

hipError_t peak_bench(int kind, double* result) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    float ms = 0.f;
    if (kind >= 200 && kind < 248) {
        // 200 + 16 * waves code (0: 4, 1: 8, 2: 16 waves per CU) + 4 * pattern + 2 * (1 GiB instead of L2-resident) + (row stride 6144 instead of 128):
        // returns shader-clock-independent NANOSECONDS per store instruction and CU
        const int k = kind - 200, wc = k >> 4, pat = (k >> 2) & 3, big = (k >> 1) & 1, strided = k & 1;
        const int nw = wc == 0 ? 4 : wc == 1 ? 8 : 16;
        const size_t bytes = big ? ((size_t)1 << 30) : ((size_t)16 << 20);
        char* dst;
        hipMalloc((void**)&dst, bytes + (1 << 20));
        const int rounds = 64;
        const size_t wave_bytes = big ? bytes / (256 * nw) : (size_t)16384 * 4;   // small: every wave rewrites its own 64 KiB (chip total <= 16 MiB: L2 + MALL)
        const int row_stride = strided ? 6144 : 128;
        auto launch = [&]() {
            if (pat == 0) hipLaunchKernelGGL(store_probe_kernel<0>, dim3(256), dim3(nw * 64), 0, nullptr, dst, wave_bytes, bytes - 1, rounds, row_stride);
            else if (pat == 1) hipLaunchKernelGGL(store_probe_kernel<1>, dim3(256), dim3(nw * 64), 0, nullptr, dst, wave_bytes, bytes - 1, rounds, row_stride);
            else hipLaunchKernelGGL(store_probe_kernel<2>, dim3(256), dim3(nw * 64), 0, nullptr, dst, wave_bytes, bytes - 1, rounds, row_stride);
        };
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(e0, nullptr);
            launch();
            hipEventRecord(e1, nullptr);
            hipDeviceSynchronize();
        }
        hipEventElapsedTime(&ms, e0, e1);
        *result = (double)ms * 1e6 / ((double)rounds * 16 * nw);   // ns per store instruction and CU
        hipFree(dst);
    } else if (kind == 0 || kind == 1) {
        float* d;
        hipMalloc(&d, 4096);
        const int iters = 20000, blocks = 256 * 2;
        for (int rep = 0; rep < 2; ++rep) {
            hipEventRecord(e0, nullptr);
            if (kind == 0) hipLaunchKernelGGL(peak_mfma_kernel<16>, dim3(blocks), dim3(256), 0, nullptr, d, iters);
            else hipLaunchKernelGGL(peak_mfma_kernel<32>, dim3(blocks), dim3(256), 0, nullptr, d, iters);
            hipEventRecord(e1, nullptr);
            hipDeviceSynchronize();
        }
        hipEventElapsedTime(&ms, e0, e1);
        const double flops = (double)blocks * 4 * iters * (kind == 0 ? 16.0 * 16384 : 4.0 * 32768);
        *result = flops / (ms * 1e-3) / 1e12;
        hipFree(d);
    } else if (kind >= 170 && kind < 178) {
        const int dep = (kind - 170) & 3, two = (kind - 170) & 4;
        float* d;
        hipMalloc(&d, 4096);
        const int iters = 8000;
        for (int rep = 0; rep < 2; ++rep) {
            hipEventRecord(e0, nullptr);
#define VP_P32(NW, D) hipLaunchKernelGGL((issue_probe32_kernel<NW, D>), dim3(256), dim3(NW * 64), 0, nullptr, iters, d)
            if (!two) { if (dep == 0) VP_P32(4, 8); else if (dep == 1) VP_P32(4, 4); else VP_P32(4, 2); }
            else { if (dep == 0) VP_P32(8, 8); else if (dep == 1) VP_P32(8, 4); else VP_P32(8, 2); }
#undef VP_P32
            hipEventRecord(e1, nullptr);
            hipDeviceSynchronize();
        }
        hipEventElapsedTime(&ms, e0, e1);
        *result = (double)ms * 1e6 / iters;
        hipFree(d);
    } else if (kind >= 100 && kind < 164) {
        const int mode = (kind - 100) & 31, nw = (kind - 100) & 32 ? 8 : 4;
        const size_t bytes = (mode & 16) ? ((size_t)1 << 20) : ((size_t)256 << 20);   // bit 4: all traffic inside 1 MiB (L2-resident)
        char *dst, *src; float* d;
        hipMalloc(&dst, bytes + 8192); hipMalloc(&src, bytes + 8192); hipMalloc(&d, 4096);
        hipMemset(src, 1, bytes + 8192);
        const int iters = 8000;
        hipError_t (*run)(int, int, char*, const char*, size_t, float*) = nullptr;
        switch (mode & 15) {
#define VP_PROBE(M) case M: run = [](int nw_, int it_, char* d_, const char* s_, size_t m_, float* k_) -> hipError_t { \
                if (nw_ == 4) { auto k = issue_probe_kernel<4, M>; hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 131072); \
                    hipLaunchKernelGGL(k, dim3(256), dim3(256), 131072, nullptr, it_, d_, s_, m_, k_); } \
                else { auto k = issue_probe_kernel<8, M>; hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 131072); \
                    hipLaunchKernelGGL(k, dim3(256), dim3(512), 131072, nullptr, it_, d_, s_, m_, k_); } \
                return hipGetLastError(); }; break;
            VP_PROBE(0) VP_PROBE(1) VP_PROBE(2) VP_PROBE(3) VP_PROBE(4) VP_PROBE(5) VP_PROBE(6) VP_PROBE(7)
            VP_PROBE(9) VP_PROBE(11) VP_PROBE(13) VP_PROBE(15)
#undef VP_PROBE
        }
        if (!run) { hipFree(dst); hipFree(src); hipFree(d); hipEventDestroy(e0); hipEventDestroy(e1); return hipErrorInvalidValue; }
        for (int rep = 0; rep < 2; ++rep) {
            hipEventRecord(e0, nullptr);
            run(nw, iters, dst, src, bytes - 1, d);
            hipEventRecord(e1, nullptr);
            hipDeviceSynchronize();
        }
        hipEventElapsedTime(&ms, e0, e1);
        *result = (double)ms * 1e6 / iters;
        hipFree(dst); hipFree(src); hipFree(d);
    } else if (kind >= 300 && kind < 492) {
        // 300 + 64 * mode (0 copy, 1 read, 2 write) + 32 * nt + 8 * ucode (U = 1, 2, 4, 8) + gridcode (workgroups = 256 x {2, 4, 8, 16, 32, 64}; 6: one per chunk; 7: 256 x 3):
        // TB/s of algorithmic traffic (copy: bytes read + bytes written) over 1 GiB per direction
        const int k = kind - 300, mode = k >> 6, nt = (k >> 5) & 1, uc = (k >> 3) & 3, gc = k & 7;
        const int U = 1 << uc;
        const size_t n = (size_t)1 << 26;   // 64 Mi x 16 bytes = 1 GiB
        u32x4 *a = nullptr, *b = nullptr; uint32_t* d = nullptr;
        if (mode != 2) { hipMalloc((void**)&a, n * 16); hipMemset(a, 1, n * 16); }
        if (mode != 1) { hipMalloc((void**)&b, n * 16); hipMemset(b, 2, n * 16); }
        hipMalloc((void**)&d, 4096);
        const size_t nchunks = n / ((size_t)256 * U);
        static const int gmul[8] = {2, 4, 8, 16, 32, 64, 0, 3};
        const unsigned grid = gc == 6 ? (unsigned)nchunks : 256u * gmul[gc];
#define VP_STREAM(M, UU, N) hipLaunchKernelGGL((peak_stream_kernel<M, UU, N>), dim3(grid), dim3(256), 0, nullptr, a, b, n, d)
#define VP_STREAM_U(M, N) do { if (U == 1) VP_STREAM(M, 1, N); else if (U == 2) VP_STREAM(M, 2, N); else if (U == 4) VP_STREAM(M, 4, N); else VP_STREAM(M, 8, N); } while (0)
#define VP_STREAM_N(M) do { if (nt) VP_STREAM_U(M, true); else VP_STREAM_U(M, false); } while (0)
        float best = 1e30f;
        for (int rep = 0; rep < 5; ++rep) {
            hipEventRecord(e0, nullptr);
            if (mode == 0) VP_STREAM_N(0); else if (mode == 1) VP_STREAM_N(1); else VP_STREAM_N(2);
            hipEventRecord(e1, nullptr);
            hipDeviceSynchronize();
            hipEventElapsedTime(&ms, e0, e1);
            if (rep > 0 && ms < best) best = ms;
        }
#undef VP_STREAM_N
#undef VP_STREAM_U
#undef VP_STREAM
        *result = (mode == 0 ? 2.0 : 1.0) * n * 16 / (best * 1e-3) / 1e12;
        if (a) hipFree(a);
        if (b) hipFree(b);
        hipFree(d);
    } else if (kind >= 500 && kind < 504) {   // 500 + 2 * (two waves per SIMD) + packed: VALU probe, nanoseconds per round of 64 multiply-adds per lane
        const int pk = (kind - 500) & 1, two = (kind - 500) >> 1;
        float* d;
        hipMalloc(&d, 4096);
        const int iters = 20000;
        for (int rep = 0; rep < 2; ++rep) {
            hipEventRecord(e0, nullptr);
            if (!two) { if (pk) hipLaunchKernelGGL((valu_probe_kernel<4, 1>), dim3(256), dim3(256), 0, nullptr, iters, d); else hipLaunchKernelGGL((valu_probe_kernel<4, 0>), dim3(256), dim3(256), 0, nullptr, iters, d); }
            else { if (pk) hipLaunchKernelGGL((valu_probe_kernel<8, 1>), dim3(256), dim3(512), 0, nullptr, iters, d); else hipLaunchKernelGGL((valu_probe_kernel<8, 0>), dim3(256), dim3(512), 0, nullptr, iters, d); }
            hipEventRecord(e1, nullptr);
            hipDeviceSynchronize();
        }
        hipEventElapsedTime(&ms, e0, e1);
        *result = (double)ms * 1e6 / iters;
        hipFree(d);
    } else if (kind >= 3 && kind <= 12) {   // 7 .. 12: 64 / 96 / 128 / 192 / 256 / 384 MiB sources: is the 256 MB memory-side cache faster than HBM?
        static const size_t mib[] = {32, 1024, 2, 0, 64, 96, 128, 192, 256, 384};
        const size_t bytes = kind == 6 ? ((size_t)256 << 10) : (mib[kind - 3] << 20);
        char* a; float* d;
        hipMalloc(&a, bytes); hipMalloc(&d, 4096);
        hipMemset(a, 1, bytes);
        const int iters = 2000, blocks = 512, depth = 10;
        hipFuncSetAttribute((const void*)peak_glds_kernel<10>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        for (int rep = 0; rep < 2; ++rep) {
            hipEventRecord(e0, nullptr);
            hipLaunchKernelGGL(peak_glds_kernel<10>, dim3(blocks), dim3(256), 65536, nullptr, a, bytes, iters, d);
            hipEventRecord(e1, nullptr);
            hipDeviceSynchronize();
        }
        hipEventElapsedTime(&ms, e0, e1);
        *result = (double)blocks * 4 * depth * 1024.0 * iters / (ms * 1e-3) / 1e12;
        hipFree(a); hipFree(d);
    } else {
        const size_t n = (size_t)1 << 26;   // 64 Mi float4 = 1 GiB
        f32x4 *a, *b;
        hipMalloc(&a, n * 16); hipMalloc(&b, n * 16);
        hipMemset(a, 1, n * 16);
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(e0, nullptr);
            hipLaunchKernelGGL(peak_copy_kernel, dim3(256 * 16), dim3(256), 0, nullptr, a, b, n);
            hipEventRecord(e1, nullptr);
            hipDeviceSynchronize();
        }
        hipEventElapsedTime(&ms, e0, e1);
        *result = 2.0 * n * 16 / (ms * 1e-3) / 1e12;
        hipFree(a); hipFree(b);
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    return hipGetLastError();
}

}  // namespace vp
