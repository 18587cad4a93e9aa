// The orient stage's arithmetic, stated once (include/vitpose_hip.h vp_orient*): the eight EXIF orientations of a plane of h x w ELEMENTS as a pure permutation.
// An element is one byte of a Y plane, the two-byte U,V pair of an NV12 chroma plane (pair order kept) or the three-byte pixel of RGB24 / BGR24 (channel
// order kept).  The kernel (orient.hip) and the host model (vp_dbg_orient_host) both map an output element to its source element with orient_source;
// easy_vitpose_amd/devorient.py::orient_host_numpy restates the table by slicing, independent of this header.
//
//   code  output                                   size   (transpose, reverse source row, reverse source column)
//   1     a                                        h x w  (0, 0, 0)
//   2     a[:, ::-1]                               h x w  (0, 0, 1)
//   3     a[::-1, ::-1]                            h x w  (0, 1, 1)
//   4     a[::-1, :]                               h x w  (0, 1, 0)
//   5     a.T                                      w x h  (1, 0, 0)
//   6     out[i, j] = a[h - 1 - j, i]              w x h  (1, 1, 0)   90 degrees clockwise
//   7     out[i, j] = a[h - 1 - j, w - 1 - i]      w x h  (1, 1, 1)
//   8     out[i, j] = a[j, w - 1 - i]              w x h  (1, 0, 1)   90 degrees counter-clockwise
//
// NV12: the Y plane is oriented with (h, w), the UV plane with the same code on (ceil(h / 2), ceil(w / 2)) pairs.  That reproduces the chroma rule of pixfmt.h
// (pixel (y, x) reads pair (y >> 1, x >> 1)) exactly when every REVERSED axis has even length: pixel y' = h - 1 - y then reads pair (h - 1 - y) >> 1 =
// h / 2 - 1 - (y >> 1), the reversed pair row.  An NV12 frame with an odd extent along an axis the code reverses is refused (orient_nv12_ok).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vp {

constexpr int ORIENT_FIRST = 1, ORIENT_LAST = 8;   // == VP_ORIENT_*
constexpr int ORIENT_TILE = 64;                    // the kernel's tile edge in elements (tests/orient_cases.py names it T)

struct OrientOps { int transpose, rev_row, rev_col; };   // reverse the SOURCE row / column index

__host__ __device__ inline OrientOps orient_ops(int code) {
    switch (code) {
        case 2: return OrientOps{0, 0, 1};
        case 3: return OrientOps{0, 1, 1};
        case 4: return OrientOps{0, 1, 0};
        case 5: return OrientOps{1, 0, 0};
        case 6: return OrientOps{1, 1, 0};
        case 7: return OrientOps{1, 1, 1};
        case 8: return OrientOps{1, 0, 1};
        default: return OrientOps{0, 0, 0};
    }
}

// the output plane of a source plane of h x w elements
__host__ __device__ inline int orient_out_h(int code, int h, int w) { return orient_ops(code).transpose ? w : h; }
__host__ __device__ inline int orient_out_w(int code, int h, int w) { return orient_ops(code).transpose ? h : w; }

// output element (i, j) of the oriented plane = source element (*r, *c) of the h x w source plane
__host__ __device__ inline void orient_source(const OrientOps& o, int h, int w, int i, int j, int* r, int* c) {
    const int r0 = o.transpose ? j : i, c0 = o.transpose ? i : j;
    *r = o.rev_row ? h - 1 - r0 : r0;
    *c = o.rev_col ? w - 1 - c0 : c0;
}

// NV12 under `code`: every axis the code reverses has even length (codes 1 and 5 reverse none)
__host__ __device__ inline bool orient_nv12_ok(int code, int h, int w) {
    const OrientOps o = orient_ops(code);
    return !((o.rev_row && (h & 1)) || (o.rev_col && (w & 1)));
}

}  // namespace vp
