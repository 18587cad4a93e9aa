// The lifetime of a stage object (DESIGN.md "Stage objects").  The tracker, the smoother, the metrics and COCO evaluators, the detector stage and the YOLO network
// each keep an object of their own beside the handle; this header is what the six share, in two parts like hoststage.h.
//
//   * The mask part (HOST ONLY, plain C++, no HIP header: tools/stage_layout_asan.cpp includes it alone): popcount64 and mask_check of a stream mask.
//   * The device part (hipcc only): StageObj, the base that owns the object's device allocations and keeps the first failure of its create, and the bodies of
//     vp_*_create / _destroy / _download_state / _reset_stream.  Every entry keeps its own null check of the handle and its own argument checks.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/vitpose_hip.h"

namespace vpi {

inline int popcount64(uint64_t m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }

// a step / reset mask names no stream beyond n_streams; who = the stage's prefix ("tracker: ")
inline int mask_check(uint64_t mask, int n_streams, const char* who, std::string* why) {
    if (n_streams < 64 && (mask >> n_streams)) { *why = std::string(who) + "a mask bit beyond n_streams = " + std::to_string(n_streams); return VP_ERR_INVALID; }
    return VP_OK;
}

}  // namespace vpi

#if defined(__HIPCC__)
#include <memory>

#include "api_internal.h"

namespace vpi {

// The base of vp_tracker, vp_smoother, vp_metrics, vp_cocoeval, vp_detector and vp_yolo.  alloc() and up() are for the create: err keeps the FIRST failure, and
// after one nothing more is allocated, copied or recorded.  The destructor frees what was recorded, so `delete` is the whole clean-up on every path.
struct StageObj {
    vp_ctx* c = nullptr;
    std::vector<void*> mem;   // device allocations, in the order of the create
    hipError_t err = hipSuccess;
    StageObj() = default;
    StageObj(const StageObj&) = delete;
    StageObj& operator=(const StageObj&) = delete;
    ~StageObj() { for (void* p : mem) (void)hipFree(p); }
    // hipMalloc of bytes, filled with the byte `fill` (< 0: left as it is)
    template <class T = char> T* alloc(size_t bytes, int fill = -1) {
        void* p = nullptr;
        if (err == hipSuccess && (err = hipMalloc(&p, bytes)) == hipSuccess) {
            mem.push_back(p);
            if (fill >= 0) err = hipMemset(p, fill, bytes);
        }
        return (T*)p;
    }
    void up(void* dst, const void* src, size_t bytes) { if (err == hipSuccess) err = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
};

// vp_*_create.  check(obj, &why) is the stage's host-only part: every refusal of the configuration, with its code, and the fields that follow from it; nothing
// has touched the device when it refuses.  body(obj) allocates through obj->alloc / up and returns the prefix of the stage's failure message.
template <class T, class Check, class Body> int stage_create(vp_ctx* c, T** out, Check check, Body body) {
    if (!c || !out) return VP_ERR_INVALID;
    *out = nullptr;
    std::unique_ptr<T> o(new T);
    o->c = c;
    std::string why;
    if (const int rc = check(o.get(), &why)) return fail(c, rc, why);
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const std::string what = body(o.get());
    if (o->err != hipSuccess) return fail(c, VP_ERR_HIP, what + hipGetErrorString(o->err));
    *out = o.release();
    return VP_OK;
}

// vp_*_destroy: waits for the device, frees; the errors of these calls are ignored
template <class T> int stage_destroy(T* o) {
    if (!o) return VP_ERR_INVALID;
    (void)hipSetDevice(o->c->cfg.device_id);
    (void)hipDeviceSynchronize();
    delete o;
    return VP_OK;
}

// vp_*_download_state behind the entry's null checks: a blocking copy behind a device synchronisation
inline int stage_download(StageObj* o, void* out, const void* src, size_t bytes) {
    vp_ctx* c = o->c;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return VP_OK;
}

// vp_*_reset_stream of the streams in mask: one memset of `stride` bytes per selected stream, in stream order, on the caller's stream
inline int stage_reset_masked(StageObj* o, void* base, size_t stride, int n_streams, uint64_t mask, const char* who, void* caller_stream) {
    vp_ctx* c = o->c;
    std::string why;
    if (mask_check(mask, n_streams, who, &why)) return fail(c, VP_ERR_INVALID, why);
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    for (int k = 0; k < n_streams; ++k)
        if ((mask >> k) & 1ull) HIPCHK(c, hipMemsetAsync((char*)base + (size_t)k * stride, 0, stride, (hipStream_t)caller_stream));
    return VP_OK;
}

// ... of a stage with one state: the whole of it
inline int stage_reset(StageObj* o, void* state, size_t bytes, void* caller_stream) { return stage_reset_masked(o, state, bytes, 1, 1ull, "", caller_stream); }

}  // namespace vpi
#endif
