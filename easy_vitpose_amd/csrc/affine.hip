// The two kernels of the training-protocol affine crop route (affinegeom.h: the contract; include/vitpose_hip.h vp_infer_images_affine,
// vp_infer_boxes_affine_stream): boxes -> centre and scale and crop records on the device, and the crop kernel that writes the RGB8 crop buffer
// crop_resize_kernel writes -- so im2col, the twin of the flip-test mode and the forward are the pad route's.  They are the counterparts of boxes.hip's
// box_geometry_kernel and elementwise.hip's crop_resize_kernel and live in a translation unit of their own so that those files, and the device code
// compiled from them, stay byte for byte what they were.  Neither uses atomics (one thread owns every value it writes): a call is bit-identical from run to run.
#include "affinegeom.h"
#include "kernels.h"
#include "pixfmt.h"

namespace vp {

// vp_infer_boxes_affine_stream: one thread per box of the chunk, frames and windows as box_geometry_kernel.  A box -> (cx, cy, S_w, S_h) (affinegeom.h box_cs), its
// crop record over the whole device frame, and its row of `cs` for the decode; a box with a non-zero status gets a record that reads nothing (y0 == y1: a black
// crop) and an all-zero cs row, which the affine decode turns into all-zero keypoints.  No offsets kernel follows this route.
__global__ __launch_bounds__(64) void box_cs_kernel(BoxFrames fr, const float* __restrict__ xyxy, int row_stride, const int32_t* __restrict__ frame_idx, int n,
                                                    float box_scale, AffRec* __restrict__ recs, float* __restrict__ cs, float* __restrict__ cs_out,
                                                    int32_t* __restrict__ status_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int32_t f = frame_idx ? frame_idx[i] : 0;
    const bool in_window = f >= fr.f0 && f < fr.f0 + fr.count;
    const bool last_window = fr.f0 + fr.count == fr.n_frames;
    if (!in_window && !(last_window && (f < 0 || f >= fr.n_frames))) return;
    float q[4] = {0.f, 0.f, 0.f, 0.f};
    int st = BOX_BAD_FRAME;
    if (in_window) {
        const float* b = xyxy + (size_t)i * row_stride;
        st = box_cs(b[0], b[1], b[2], b[3], box_scale, q);
        if (st != BOX_OK) q[0] = q[1] = q[2] = q[3] = 0.f;
    }
    AffRec r;
    if (st == BOX_OK) {
        const BoxFrame& im = fr.fr[f - fr.f0];
        const AffineMap m = affine_map(q);
        r.plane[0] = im.plane[0]; r.plane[1] = im.format == PIX_NV12 ? im.plane[1] : nullptr;
        r.pitch[0] = im.pitch[0]; r.pitch[1] = im.format == PIX_NV12 ? im.pitch[1] : 0;
        r.ax = m.ax; r.bx = m.bx; r.ay = m.ay; r.by = m.by;
        r.w = im.w; r.y0 = 0; r.y1 = im.h; r.format = im.format; r.matrix = im.matrix; r.pad_ = 0;
    } else {
        r.plane[0] = r.plane[1] = nullptr; r.pitch[0] = r.pitch[1] = 0;
        r.ax = r.bx = r.ay = r.by = 0.0;
        r.w = 0; r.y0 = r.y1 = 0; r.format = PIX_RGB24; r.matrix = 0; r.pad_ = 0;
    }
    recs[i] = r;
    for (int j = 0; j < 4; ++j) cs[4 * i + j] = q[j];
    if (cs_out)
        for (int j = 0; j < 4; ++j) cs_out[(size_t)4 * i + j] = q[j];
    if (status_out) status_out[i] = st;
}

hipError_t box_cs_launch(const BoxFrames& fr, const float* xyxy, int row_stride, const int32_t* frame_idx, int n, float box_scale, AffRec* recs, float* cs,
                         float* cs_out, int32_t* status_out, hipStream_t s) {
    hipLaunchKernelGGL(box_cs_kernel, dim3((n + 63) / 64), dim3(64), 0, s, fr, xyxy, row_stride, frame_idx, n, box_scale, recs, cs, cs_out, status_out);
    return hipGetLastError();
}

// The training-protocol affine crop (affinegeom.h: the contract, PARITY UNPINNED against OpenCV's warpAffine): one block = one output row, one thread = one
// output pixel; the row's source row and fraction depend on the block alone (uniform values: computed once per block, not per pixel).  fetch = the RGB8 value of
// a frame pixel exactly as crop_pixel's fetch converts it (pixfmt.h), 0 outside the rows and columns the record names -- no read ever leaves them.
template <int FMT> __device__ __forceinline__ void affine_pixel(const AffRec& r, int64_t sy, int ay, int ox, uint8_t* __restrict__ dst) {
    const YuvCoef k = yuv_coef(FMT == PIX_NV12 ? r.matrix : 0);
    auto fetch = [&](int64_t Y, int64_t X, int* rgb) {   // frame pixel
        if (Y < r.y0 || Y >= r.y1 || X < 0 || X >= r.w) { rgb[0] = rgb[1] = rgb[2] = 0; return; }
        const size_t yy = (size_t)(Y - r.y0), xx = (size_t)X;
        if (FMT == PIX_NV12) {
            const uint8_t* uv = r.plane[1] + (size_t)((Y >> 1) - (r.y0 >> 1)) * r.pitch[1] + (xx >> 1) * 2;
            yuv_to_rgb(k, r.plane[0][yy * r.pitch[0] + xx], uv[0], uv[1], rgb);
            return;
        }
        const uint8_t* p = r.plane[0] + yy * r.pitch[0] + xx * 3;
        rgb[0] = p[FMT == PIX_BGR24 ? 2 : 0]; rgb[1] = p[1]; rgb[2] = p[FMT == PIX_BGR24 ? 0 : 2];
    };
    int64_t sx;
    int ax;
    affine_axis(ox, r.ax, r.bx, &sx, &ax);
    int p00[3], p01[3], p10[3], p11[3];
    fetch(sy, sx, p00); fetch(sy, sx + 1, p01); fetch(sy + 1, sx, p10); fetch(sy + 1, sx + 1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)affine_blend(p00[c], p01[c], p10[c], p11[c], ax, ay);
}

__global__ __launch_bounds__(192) void crop_affine_kernel(const AffRec* __restrict__ recs, uint8_t* __restrict__ out) {
    const int crop = blockIdx.x >> 8, oy = blockIdx.x & 255, ox = threadIdx.x;
    const AffRec r = recs[crop];
    uint8_t* dst = out + (((size_t)crop * 256 + oy) * 192 + ox) * 3;
    int64_t sy;
    int ay;
    affine_axis(oy, r.ay, r.by, &sy, &ay);
    if (sy + 1 < r.y0 || sy >= r.y1) { dst[0] = dst[1] = dst[2] = 0; return; }   // the whole row lies outside (block-uniform; every row of a refused box)
    if (r.format == PIX_RGB24) affine_pixel<PIX_RGB24>(r, sy, ay, ox, dst);   // block-uniform: a launch may hold records of several formats
    else if (r.format == PIX_NV12) affine_pixel<PIX_NV12>(r, sy, ay, ox, dst);
    else affine_pixel<PIX_BGR24>(r, sy, ay, ox, dst);
}

hipError_t crop_affine_launch(const AffRec* recs, uint8_t* out, int n, hipStream_t s) {
    hipLaunchKernelGGL(crop_affine_kernel, dim3(n * 256), dim3(192), 0, s, recs, out);
    return hipGetLastError();
}

}  // namespace vp
