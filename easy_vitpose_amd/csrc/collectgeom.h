// The collect stage of vp_collect_stream (include/vitpose_hip.h), for ONE value each: the gates of a row, the id of a row, the layout of the packed table and the
// words of a record.  Shared by the device kernels (collect.hip) and the host-only tap vp_dbg_collect_host, so that the CPU tests of the tap pin the arithmetic the
// device runs, as labelgeom.h does for the tags.  easy_vitpose_amd/devcollect.py restates it in numpy (collect_numpy).
//
// Modelled on what the reference's inference() returns (inference.py: `{id: keypoints}` over `zip(ids, bboxes, ...)`, ids = the tracker's or range(len(bboxes))):
// the persons a call keeps, in one dense table that one device-to-host copy brings down.
//
// A row is one person of the call: keypoints float32 [K, 3], optionally an id, a frame index, the NMS's rank, the boxes entry's status, a score and a crop-params row.
//   frame     d_frame[i], 0 without d_frame; VALID iff 0 <= frame < n_frames.
//   id        d_ids[i]; without d_ids the row's ORDINAL: the count of earlier VALID rows of the same frame in call order, kept or not (range(len(bboxes))).
//   kept      valid, id >= 0 when ids are given (an absent tracker row has id -1), rank >= 0 when ranks are given, status == 0 when a status is given.
//   order     records by frame ascending, then by call order: record index = (kept rows of the frames before) + (kept rows of the same frame before the row).
//   layout    header int32 [n_frames + 1] = kept rows per frame, the TRUE total last (whatever max_records), zero-padded to a multiple of 4 words; then records of
//             S = 4 ceil((8 + 3 K) / 4) words: id, frame, row index in the call, score (float32; 0.0 without d_score), box int32 (x0, y0, x0 + cw, y0 + ch) of the
//             crop-params row {frame, x0, y0, cw, ch, ...} with wrapping int32 sums (four zeros without d_crop_params), the 3 K keypoint words bit for bit, zeros.
//   writing   the header and the first min(total, max_records) records; no byte behind the last written record; every written byte once per call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vp {

constexpr int COLLECT_MAX_ROWS = 8192;     // VP_COLLECT_MAX_ROWS
constexpr int COLLECT_MAX_FRAMES = 64;     // VP_COLLECT_MAX_FRAMES
constexpr int COLLECT_MAX_K = 133;
constexpr int COLLECT_FIELDS = 8;          // words in front of the keypoints

__host__ __device__ inline int collect_header_words(int n_frames) { return (n_frames + 1 + 3) / 4 * 4; }
__host__ __device__ inline int collect_record_words(int K) { return (COLLECT_FIELDS + 3 * K + 3) / 4 * 4; }
__host__ __device__ inline int64_t collect_bytes(int n_frames, int K, int max_records) {
    return 4 * ((int64_t)collect_header_words(n_frames) + (int64_t)max_records * collect_record_words(K));
}

// the inputs of a call (device pointers in the kernels, host pointers in the tap); by kernel argument
struct CollectIn {
    const uint32_t* kpts;         // [n, K, 3] as words: copied, never interpreted
    const int32_t* ids;           // or null
    const int32_t* frame;         // or null
    const int32_t* rank;          // or null
    const int32_t* status;        // or null
    const uint32_t* score;        // or null; float32 as words at score_stride
    const int32_t* crop_params;   // [n, 9] or null
    int32_t n, K, n_frames, max_records;
    int64_t score_stride;
};

__host__ __device__ inline int32_t collect_frame(const CollectIn& in, int i) { return in.frame ? in.frame[i] : 0; }
__host__ __device__ inline bool collect_valid(const CollectIn& in, int32_t f) { return f >= 0 && f < in.n_frames; }
// the gates behind the frame's: i is a row with a valid frame
__host__ __device__ inline bool collect_gates(const CollectIn& in, int i) {
    return !(in.ids && in.ids[i] < 0) && !(in.rank && in.rank[i] < 0) && !(in.status && in.status[i] != 0);
}

// word w of the record of row i (w < collect_record_words(K)); id = the row's id, given or ordinal
__host__ __device__ inline uint32_t collect_word(const CollectIn& in, int i, int32_t id, int32_t f, int w) {
    if (w >= COLLECT_FIELDS) return w < COLLECT_FIELDS + 3 * in.K ? in.kpts[(size_t)i * 3 * in.K + (w - COLLECT_FIELDS)] : 0u;
    if (w == 0) return (uint32_t)id;
    if (w == 1) return (uint32_t)f;
    if (w == 2) return (uint32_t)i;
    if (w == 3) return in.score ? in.score[(size_t)i * (size_t)in.score_stride] : 0u;
    if (!in.crop_params) return 0u;
    const int32_t* p = in.crop_params + (size_t)i * 9;
    const uint32_t x0 = (uint32_t)p[1], y0 = (uint32_t)p[2];
    return w == 4 ? x0 : (w == 5 ? y0 : (w == 6 ? x0 + (uint32_t)p[3] : y0 + (uint32_t)p[4]));
}

}  // namespace vp
