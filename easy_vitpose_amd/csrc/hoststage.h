// Host staging of the synchronous entries (DESIGN.md "Host staging").  Every stage has a stream-ordered entry on device pointers and a synchronous twin on host
// arrays; the twin is: lay out, upload, the stage's enqueue, download.  This header is what the twins share, in two parts.
//
//   * The layout part (HOST ONLY, plain C++, no HIP header: tools/stage_layout_asan.cpp includes it alone): up256, the StageLayout accumulator that places the
//     parts of one scratch block, and the byte extent of a vp_image's planes.
//   * The device part (hipcc only): HostStage, one scratch block of a call with the first-failure bookkeeping of its copies, and device_range_ok, the ONE check
//     "these bytes are device memory of the handle's device inside one allocation" behind check_device_frame / _image / _plane.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/vitpose_hip.h"
#include "pixfmt.h"

namespace vpi {

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

inline int plane_count(const vp_image& im) { return im.format == vp::PIX_NV12 ? 2 : 1; }
inline size_t plane_bytes(const vp_image& im, int p) {   // of plane p, first byte to last: pitch padding between the rows, none behind the last
    return (size_t)(vp::plane_rows(im.format, p, im.h) - 1) * (size_t)im.pitch[p] + (size_t)vp::plane_row_bytes(im.format, p, im.w);
}

// The parts of one block, in order.  part() returns the part's offset: a multiple of 256 plus skew (skew < 256: vp_orient places a plane at its caller's address
// modulo 256), with room for up256(bytes) before the next part.  end = the sum of the rooms (what the state arenas of the creates allocate), total() = end plus
// 256 bytes of slack (what a scratch block allocates: a kernel that reads a full vector at a part's last element stays inside the block).
struct StageLayout {
    size_t end = 0;   // a multiple of 256
    size_t part(size_t bytes, size_t skew = 0) {
        const size_t at = end + skew;
        end = up256(at + up256(bytes));
        return at;
    }
    size_t total() const { return end + 256; }
};

}  // namespace vpi

#if defined(__HIPCC__)
#include "api_internal.h"

namespace vpi {

// [ptr, ptr + bytes) is device memory of the handle's device and lies inside one allocation.  A refusal leaves the runtime's error for the caller to clear
inline bool device_range_ok(const vp_ctx* c, const void* ptr, size_t bytes) {
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof(a));
    void* base = nullptr;
    size_t size = 0;
    const uint8_t* q = (const uint8_t*)ptr;
    return q && hipPointerGetAttributes(&a, q) == hipSuccess && a.type == hipMemoryTypeDevice && a.device == c->cfg.device_id &&
           hipMemGetAddressRange(&base, &size, (void*)q) == hipSuccess && q + bytes <= (const uint8_t*)base + size;
}

// The scratch block of one synchronous call: part() ... alloc() ... up() ... the stage's enqueue on s ... down() ... sync(); the destructor frees the block on every
// return path.  rc keeps the FIRST failure (later calls still run, as the copies of a call always did); the site skips its enqueue and its downloads on rc.
// c = nullptr (the handle-less taps): the caller has set the device, failures go to the create-error slot, s is the default stream.
class HostStage : public StageLayout {
public:
    int rc = VP_OK;
    hipStream_t s;
    explicit HostStage(vp_ctx* c) : s(c ? c->own_stream : nullptr), c_(c) {
        if (c) chk(hipSetDevice(c->cfg.device_id), "hipSetDevice(c->cfg.device_id)");
    }
    ~HostStage() { if (m_) (void)hipFree(m_); }
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;
    void chk(hipError_t e, const char* what) { if (e != hipSuccess && !rc) rc = fail(c_, VP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
    int alloc() {   // the one hipMalloc of the call, total() bytes
        if (!rc) chk(hipMalloc((void**)&m_, total()), "scratch block of a synchronous entry");
        return rc;
    }
    template <class T = char> T* at(size_t off) const { return (T*)(m_ + off); }
    void up(void* dst, const void* src, size_t bytes, const char* what) { chk(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s), what); }
    void down(void* dst, const void* src, size_t bytes, const char* what) { chk(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s), what); }
    void sync() { chk(hipStreamSynchronize(s), "hipStreamSynchronize"); }

private:
    vp_ctx* c_;
    char* m_ = nullptr;
};

}  // namespace vpi
#endif
