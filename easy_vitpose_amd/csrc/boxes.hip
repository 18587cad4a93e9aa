// vp_infer_boxes_stream's two small kernels: detector boxes -> crop records on the device, and the frame offsets after the decode.
// Neither uses atomics (one thread owns every value it writes), so a call is bit-identical from run to run.
#include "boxgeom.h"
#include "kernels.h"
#include "pixfmt.h"

namespace vp {

// One thread per box of the chunk.  A launch sees frames [f0, f0 + count) of the call's table (kernel argument); a box whose frame lies
// elsewhere is left to the launch that holds its frame, and a frame index outside [0, n_frames) is settled by the launch holding the last
// frame, so every box is written by exactly one launch.  A box with a non-zero status gets a harmless record (a 1 x 1 crop of `zero_px`,
// decoded as a 1 x 1 canvas) and aux status != 0, which box_offsets_kernel turns into all-zero keypoints.
__global__ __launch_bounds__(64) void box_geometry_kernel(BoxFrames fr, const float* __restrict__ xyxy, int row_stride, const int32_t* __restrict__ frame_idx,
                                                          int n, int pad, const uint8_t* __restrict__ zero_px, CropRec* __restrict__ recs,
                                                          int32_t* __restrict__ wh, int32_t* __restrict__ aux, int32_t* __restrict__ p9_out,
                                                          int32_t* __restrict__ status_out, const int32_t* __restrict__ slot) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int32_t f = frame_idx ? frame_idx[i] : 0;
    const bool in_window = f >= fr.f0 && f < fr.f0 + fr.count;
    const bool last_window = fr.f0 + fr.count == fr.n_frames;
    if (!in_window && !(last_window && (f < 0 || f >= fr.n_frames))) return;
    int32_t p8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int st = BOX_BAD_FRAME;
    if (in_window) {
        const float* b = xyxy + (size_t)i * row_stride;
        st = box_geometry(b[0], b[1], b[2], b[3], fr.fr[f - fr.f0].h, fr.fr[f - fr.f0].w, pad, p8);
        if (st != BOX_OK)
            for (int j = 0; j < 8; ++j) p8[j] = 0;
    }
    CropRec r;
    if (st == BOX_OK) {
        const BoxFrame& im = fr.fr[f - fr.f0];
        const bool nv12 = im.format == PIX_NV12;
        r.src = im.plane[0] + (size_t)p8[1] * im.pitch[0] + (size_t)p8[0] * (nv12 ? 1 : 3);
        r.pitch = im.pitch[0];
        r.cw = p8[2]; r.ch = p8[3]; r.left = p8[4]; r.top = p8[5]; r.pw = p8[6]; r.ph = p8[7];
        r.src1 = nv12 ? im.plane[1] + (size_t)(p8[1] >> 1) * im.pitch[1] + (size_t)(p8[0] >> 1) * 2 : nullptr;
        r.pitch1 = nv12 ? im.pitch[1] : 0;
        r.format = im.format; r.matrix = im.matrix; r.oy = p8[1] & 1; r.ox = p8[0] & 1;
    } else {
        r.src = zero_px; r.pitch = 3;
        r.cw = r.ch = r.pw = r.ph = 1; r.left = r.top = 0;
        r.src1 = nullptr; r.pitch1 = 0;
        r.format = PIX_RGB24; r.matrix = 0; r.oy = r.ox = 0;
    }
    recs[slot ? slot[i] : i] = r;   // a chunk with per-crop experts: straight into its place in the expert order
    wh[2 * i] = r.pw;   // decode scales by the padded canvas, as vp_infer_frames passes it
    wh[2 * i + 1] = r.ph;
    aux[4 * i] = p8[1] - p8[5];       // y0 - top_pad
    aux[4 * i + 1] = p8[0] - p8[4];   // x0 - left_pad
    aux[4 * i + 2] = st;
    aux[4 * i + 3] = 0;
    if (p9_out) {
        int32_t* o = p9_out + (size_t)i * 9;
        o[0] = st == BOX_OK ? f : 0;
        for (int j = 0; j < 8; ++j) o[1 + j] = p8[j];
    }
    if (status_out) status_out[i] = st;
}

hipError_t box_geometry_launch(const BoxFrames& fr, const float* xyxy, int row_stride, const int32_t* frame_idx, int n, int pad, const uint8_t* zero_px,
                               CropRec* recs, int32_t* wh, int32_t* aux, int32_t* p9_out, int32_t* status_out, hipStream_t s, const int32_t* slot) {
    hipLaunchKernelGGL(box_geometry_kernel, dim3((n + 63) / 64), dim3(64), 0, s, fr, xyxy, row_stride, frame_idx, n, pad, zero_px, recs, wh, aux, p9_out,
                       status_out, slot);
    return hipGetLastError();
}

// out [n, K, 3] (y, x, conf) in padded-crop pixels -> frame pixels: + (y0 - top_pad, x0 - left_pad) in float32, as VitInference.inference_frames
// adds them (numpy's float64 add of an integer below 2^24 followed by the float32 store rounds the exact sum once, as this add does);
// rows with a non-zero status become all zero.  slot / recs (null: every row has K joints): a ViTPose+ chunk with per-crop experts, rows of K = Kmax joints --
// row i's expert has recs[slot[i]].K of them, the zeros the decode wrote behind those stay zeros.
__global__ __launch_bounds__(256) void box_offsets_kernel(const int32_t* __restrict__ aux, float* __restrict__ out, int n, int K, const int32_t* __restrict__ slot,
                                                          const MixRec* __restrict__ recs) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n * K) return;
    const int i = j / K;
    float* o = out + (size_t)j * 3;
    if (aux[4 * i + 2] != BOX_OK) {
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
        return;
    }
    if (slot && j - i * K >= recs[slot[i]].K) return;
    o[0] = o[0] + (float)aux[4 * i];
    o[1] = o[1] + (float)aux[4 * i + 1];
}

hipError_t box_offsets_launch(const int32_t* aux, float* out, int n, int K, hipStream_t s, const int32_t* slot, const MixRec* recs) {
    if ((slot != nullptr) != (recs != nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(box_offsets_kernel, dim3((n * K + 255) / 256), dim3(256), 0, s, aux, out, n, K, slot, recs);
    return hipGetLastError();
}

}  // namespace vp
