// Keypoint smoothing of the video path -- the One-Euro filter of the reference's post_processing/one_euro_filter.py in its fixed-rate mode (fps given, so
// d_cutoff = fps and t_e counts frames) -- for ONE coordinate of ONE joint.  Shared by the device kernels of vp_smooth_update_stream (smooth.hip) and the host-only
// tap vp_dbg_smooth_host, so that the CPU tests of the tap pin the arithmetic the device runs, as sortgeom.h does for the tracker.  easy_vitpose_amd/smooth.py is
// the numpy twin.
//
// All arithmetic is fp64 and nothing is contracted: the pragma below holds to the end of the translation unit that includes this header (smooth.hip holds the
// smoother and nothing else) and build.py compiles smooth.hip with -ffp-contract=off (SOURCE_FLAGS), for the reason given there for track.hip.  fp64 division is
// correctly rounded on the host and on gfx950.  Every operation below is one the reference's numpy expression performs, in its order, so the host tap, the device
// and the reference agree bit for bit.
//
//   state   per coordinate (the y and the x column of a (y, x, conf) row; conf is never touched): x_prev, dx_prev (fp64) and a FRESH byte, set at birth
//   birth   x_prev = x, dx_prev = 0, fresh = 1; the row is returned unchanged (the reference's constructor: no masking)
//   update  with the float32 input x and the effective t_e:
//             d      = fresh ? (double)((float)x - (float)x_prev) : (double)x - x_prev      (the reference's first call subtracts two float32 arrays)
//             dx     = d / t_e
//             r      = (2 pi * d_cutoff) * t_e;   a_d = r / (r + 1);   dx_hat = a_d * dx + (1 - a_d) * dx_prev
//             cutoff = min_cutoff + beta * |dx_hat|
//             r      = (2 pi * cutoff) * t_e;     a = r / (r + 1);     x_hat = a * (double)x + (1 - a) * x_prev
//             x_hat  = -10 where x <= 0                                                       (the reference's mask, per coordinate)
//             x_prev = x_hat, dx_prev = dx_hat, fresh = 0;  the output is (float)x_hat, rounded once
//   missing = 1 (restart; no reference, pinned by the numpy twin): a coordinate whose x_prev <= 0 (born missing, or masked last time) does not blend away from
//           -10 as the reference does: x_hat = x (-10 where x <= 0), dx_hat = 0, fresh = 1.
//
// The table (one per stream): EURO_SLOTS slots of (id, last_seen, 2K coordinate states) and a frame_count; which track sits in which slot is fixed by the rule in
// include/vitpose_hip.h so that the state can be compared byte for byte.  The blob of one stream, every part a multiple of 16 bytes:
//   int32 frame_count, pad[3] | int32 id[128] | int32 last_seen[128] (0 = the slot is free) | double x_prev[128][K][2] | double dx_prev[128][K][2] |
//   uint8 fresh[128][K][2]                                                                              (the pair = (y, x))
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace vp {

constexpr int EURO_SLOTS = 128;           // VP_SMOOTH_SLOTS: smoothed tracks per stream
constexpr int EURO_MAX_STREAMS = 64;      // VP_TRACK_MAX_STREAMS
constexpr int EURO_MAX_JOINTS = 1024;
constexpr int EURO_FLAG_DUP = 1, EURO_FLAG_FULL = 2, EURO_FLAG_BAD_ROW = 8;
constexpr double EURO_TWO_PI = 6.283185307179586;   // 2 * np.pi

struct EuroParams {
    double min_cutoff, beta, d_cutoff;
    int32_t max_age, n_streams, n_joints, max_rows, missing;
};
struct EuroTe {
    double v[EURO_MAX_STREAMS];   // t_e per stream, by kernel argument
};

// offsets into one stream's blob
__host__ __device__ inline size_t euro_off_id() { return 16; }
__host__ __device__ inline size_t euro_off_seen() { return 16 + 4 * (size_t)EURO_SLOTS; }
__host__ __device__ inline size_t euro_off_x(int) { return 16 + 8 * (size_t)EURO_SLOTS; }
__host__ __device__ inline size_t euro_off_dx(int K) { return euro_off_x(K) + (size_t)EURO_SLOTS * K * 16; }
__host__ __device__ inline size_t euro_off_fresh(int K) { return euro_off_dx(K) + (size_t)EURO_SLOTS * K * 16; }
__host__ __device__ inline size_t euro_stream_bytes(int K) { return euro_off_fresh(K) + (size_t)EURO_SLOTS * K * 2; }

__host__ __device__ inline bool euro_finite(float v) { return v - v == 0.f; }

// slot_of_row codes: >= 0 update that slot, EURO_PASS copy the row through, <= EURO_BIRTH0 - slot a birth into that slot
constexpr int32_t EURO_PASS = -1, EURO_BIRTH0 = -2;
__host__ __device__ inline int32_t euro_birth_code(int slot) { return EURO_BIRTH0 - slot; }
__host__ __device__ inline int euro_birth_slot(int32_t code) { return EURO_BIRTH0 - code; }

__host__ __device__ inline void euro_birth(float x, double& x_prev, double& dx_prev, uint8_t& fresh) {
    x_prev = (double)x;
    dx_prev = 0.0;
    fresh = 1;
}

// one update of one coordinate; -> the output
__host__ __device__ inline float euro_update(float x, double t_e, const EuroParams& p, double& x_prev, double& dx_prev, uint8_t& fresh) {
    double x_hat, dx_hat;
    if (p.missing == 1 && x_prev <= 0.0) {
        x_hat = x <= 0.f ? -10.0 : (double)x;
        dx_hat = 0.0;
        fresh = 1;
    } else {
        const double d = fresh ? (double)(x - (float)x_prev) : (double)x - x_prev;
        const double dx = d / t_e;
        double r = (EURO_TWO_PI * p.d_cutoff) * t_e;
        const double a_d = r / (r + 1.0);
        dx_hat = a_d * dx + (1.0 - a_d) * dx_prev;
        const double cutoff = p.min_cutoff + p.beta * fabs(dx_hat);
        r = (EURO_TWO_PI * cutoff) * t_e;
        const double a = r / (r + 1.0);
        x_hat = a * (double)x + (1.0 - a) * x_prev;
        if (x <= 0.f) x_hat = -10.0;
        fresh = 0;
    }
    x_prev = x_hat;
    dx_prev = dx_hat;
    return (float)x_hat;
}

}  // namespace vp
