// Helpers of the vp_dbg_* taps, shared by the parity taps (debug_taps.hip, product) and the timing taps (tools_taps.hip, tools library only).
#pragma once
#include "api_internal.h"

namespace vpi {

inline vp_ctx* dbg_ctx(int device, int dtype) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        g_create_error = "no HIP device available (no CPU fallback)";
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    vp_ctx* c = new vp_ctx();
    c->cfg.device_id = device;
    c->dtype = dtype == VP_DTYPE_F16 ? vp::DT_F16 : vp::DT_BF16;
    apply_gemm_tuning(c->sw);
    return c;
}
inline int dbg_finish(vp_ctx* c, int rc) {
    if (rc) g_create_error = c->err;
    vp_destroy(c);
    return rc;
}
// device 16-bit -> host fp32
inline int download16(vp_ctx* c, const uint16_t* d, float* out, size_t n) {
    std::vector<uint16_t> t(n);
    HIPCHK(c, hipMemcpy(t.data(), d, n * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        if (c->dtype == vp::DT_BF16) {
            uint32_t u = (uint32_t)t[i] << 16;
            std::memcpy(&out[i], &u, 4);
        } else {
            const uint32_t h = t[i], sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ff;
            uint32_t u;
            if (e == 0) {
                if (m == 0) u = sign;
                else { int sh = 0; uint32_t mm = m; while (!(mm & 0x400)) { mm <<= 1; ++sh; }
                       u = sign | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ff) << 13); }
            } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
            else u = sign | ((e + 112) << 23) | (m << 13);
            std::memcpy(&out[i], &u, 4);
        }
    }
    return VP_OK;
}

}  // namespace vpi
