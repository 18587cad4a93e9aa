// The inference entries of the C ABI (include/vitpose_hip.h) and their staging: host crops, device crops on the handle's or a caller's stream,
// the two asynchronous slots, frames, device boxes, ViTPose+ mixed batches (vp_infer_experts; per-crop experts on the device, frames and boxes entries with
// their host-side plan, mix_plan, and its doubled form under the per-expert flip-test mode, mix_records_flip), vp_infer_flip.  Each walks its crops in chunks (for_chunks) and hands a chunk to forward.hip.
#include "affinegeom.h"
#include "api_internal.h"
#include "hoststage.h"
#include "boxgeom.h"
#include "pixfmt.h"

using namespace vpi;

namespace {

// The one walk over n crops in chunks of at most cap: body(off, nb) for crops [off, off + nb), stopping at the first error
template <class Body> int for_chunks(int n, int cap, Body body) {
    for (int off = 0; off < n; off += cap)
        if (const int rc = body(off, std::min(n - off, cap))) return rc;
    return VP_OK;
}

// The host-staged chunk: crops [off, off + nb) of a host batch into in_stage (or dst) and, where given, their sizes into wh_stage, on c->stream ...
int stage_in(vp_ctx* c, const void* crops, int fmt, const int32_t* org_wh, int off, int nb, void* dst = nullptr) {
    HIPCHK(c, hipMemcpyAsync(dst ? dst : c->in_stage, (const char*)crops + (size_t)off * crop_bytes(fmt), (size_t)nb * crop_bytes(fmt), hipMemcpyHostToDevice, c->stream));
    if (org_wh) HIPCHK(c, hipMemcpyAsync(c->wh_stage, org_wh + 2 * (size_t)off, (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
    return VP_OK;
}
// ... and nb results of `elem` floats each from d_res back to rows [off, off + nb) of the caller's `out`; copy_out_sync also waits for the chunk:
// the staging buffers are rewritten by the next one
int copy_out(vp_ctx* c, float* out, const float* d_res, size_t elem, int off, int nb) {
    HIPCHK(c, hipMemcpyAsync(out + (size_t)off * elem, d_res, (size_t)nb * elem * 4, hipMemcpyDeviceToHost, c->stream));
    return VP_OK;
}
int copy_out_sync(vp_ctx* c, float* out, const float* d_res, size_t elem, int off, int nb) {
    if (const int rc = copy_out(c, out, d_res, elem, off, nb)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

// vp_infer_device / vp_infer_device_stream: n device-resident crops through run_chunk on c->stream (the entries differ in the ordering around this)
int device_chunks(vp_ctx* c, const void* d_crops, int fmt, int n, const int32_t* d_wh, float* d_out) {
    return for_chunks(n, chunk_cap(c), [&](int off, int nb) {
        return run_chunk(c, (const char*)d_crops + (size_t)off * crop_bytes(fmt), fmt, nb, d_wh ? d_wh + 2 * (size_t)off : nullptr, d_out + (size_t)off * c->Kp * 3);
    });
}

// frame f of a call that reads its frames in place: every plane device memory of the handle's device, (plane rows - 1) * pitch + row bytes of it inside one
// allocation (the planes may share one or not).  A null plane fails here too: vp_infer_boxes_stream relies on it (vp_infer_frames has refused one in
// image_plan, with the crop that names it).  The format and the pitches have passed image_check
int check_device_frame(vp_ctx* c, const vp_image& im, int f) {
    bool ok = true;
    for (int p = 0; p < plane_count(im) && ok; ++p) ok = device_range_ok(c, im.plane[p], plane_bytes(im, p));
    if (ok) return VP_OK;
    (void)hipGetLastError();
    return fail(c, VP_ERR_INVALID, "frame " + std::to_string(f) + " is not device memory of device " + std::to_string(c->cfg.device_id) +
                                       " (or runs past the end of its allocation)");
}

// the RGB24 frames of the entries that came before vp_image: {{data, NULL}, {3 w, 0}, h, w, RGB24, 0}
std::vector<vp_image> rgb_images(const vp_frame* frames, int n_frames) {
    std::vector<vp_image> v(frames && n_frames > 0 ? (size_t)n_frames : 0);
    for (size_t f = 0; f < v.size(); ++f) v[f] = vp_image{{frames[f].data, nullptr}, {(int64_t)frames[f].w * 3, 0}, frames[f].h, frames[f].w, VP_PIX_RGB24, 0};
    return v;
}
const vp_image* table_ptr(const std::vector<vp_image>& v) { return v.empty() ? nullptr : v.data(); }   // (a temporary lives to the end of the call it is passed to)

// A grow-only device buffer of the handle (*buf, *cap bytes) holds at least `bytes`: the larger one is allocated first, then the smaller one is
// released (never shrunk: growing inputs must not grow device memory without bound), so a failed allocation leaves the handle usable
template <class T> int grow_buffer(vp_ctx* c, T** buf, size_t* cap, size_t bytes, const char* what) {
    if (bytes <= *cap) return VP_OK;
    void* q = nullptr;
    if (*buf) HIPCHK(c, hipStreamSynchronize(c->stream));   // enqueued work may still read the old one
    if (hipMalloc(&q, bytes + 256) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, VP_ERR_HIP, "cannot allocate a " + std::to_string(bytes) + "-byte " + what);
    }
    if (*buf) {
        const auto it = std::find(c->allocs.begin(), c->allocs.end(), (void*)*buf);
        if (it != c->allocs.end()) c->allocs.erase(it);
        hipFree(*buf);
    }
    c->allocs.push_back(q);
    *buf = (T*)q;
    *cap = bytes;
    return VP_OK;
}

// Work on the handle's buffers is about to be enqueued on stream s: order it behind whatever the previous call left on ANOTHER stream.
//   own -> own, caller A -> caller A: nothing (in-order streams);  own -> caller: record on own, caller waits;  caller -> own / another caller: wait for ev_sw,
//   which vp_infer_device_stream recorded on the caller's stream behind its launches (that stream itself is never touched again: it may be gone).
int adopt_stream(vp_ctx* c, hipStream_t s) {
    if (!c->foreign_pending && s == c->own_stream) return VP_OK;
    if (c->foreign_pending && (const void*)s == c->last_stream_id && s != c->own_stream) return VP_OK;
    if (!c->ev_sw) HIPCHK(c, hipEventCreateWithFlags(&c->ev_sw, hipEventDisableTiming));
    if (!c->foreign_pending) HIPCHK(c, hipEventRecord(c->ev_sw, c->own_stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_sw, 0));
    if (s == c->own_stream) c->foreign_pending = false;
    return VP_OK;
}

int check_ready(vp_ctx* c, int fmt, int n, const void* p0, const void* p1, bool adopt_own = true) {
    if (const int rc = need_weights(c)) return rc;
    if (fmt != VP_INPUT_F32_NCHW && fmt != VP_INPUT_U8_NHWC) return fail(c, VP_ERR_INVALID, "unknown input_format");
    if (n < 0 || (n > 0 && (!p0 || !p1))) return fail(c, VP_ERR_INVALID, "null buffer or negative batch");
    hipError_t e = hipSetDevice(c->cfg.device_id);
    if (e != hipSuccess) return fail(c, VP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return adopt_own ? adopt_stream(c, c->own_stream) : VP_OK;   // every entry but the caller-stream path works on the handle's own stream
}

// The ordering of the caller-stream entries (vp_infer_device_stream, vp_infer_boxes_stream): `chunks` enqueues the call's work on c->stream.
// Batches of 1 .. caller_stream_max_n crops (<= max_batch) run ON the caller's stream -- in order with its producers and consumers by construction,
// no cross-stream dependency per call (two of them cost ~0.1 ms of a 0.6-2.4 ms step: profiles/small_batch_r5.txt); ev_sw, recorded behind the
// launches, is what the next call on any other stream (and vp_synchronize / vp_destroy) waits for.  Larger batches run on the handle's own
// stream, fenced against the caller's with ev_in / ev_out.
template <class Chunks> int caller_ordered(vp_ctx* c, hipStream_t cs, int n, Chunks chunks) {
    int rc;
    if (n > 0 && chunk_rows(c, n) <= c->sw.caller_stream_max_n && n <= chunk_cap(c) && cs != c->own_stream) {
        if ((rc = adopt_stream(c, cs))) return rc;
        c->stream = cs;
        rc = chunks();
        c->stream = c->own_stream;
        if (!c->ev_sw && hipEventCreateWithFlags(&c->ev_sw, hipEventDisableTiming) != hipSuccess) return fail(c, VP_ERR_HIP, "hipEventCreateWithFlags(ev_sw)");
        const hipError_t er = hipEventRecord(c->ev_sw, cs);   // also when rc != 0: part of the chunk may be enqueued
        c->foreign_pending = true;
        c->last_stream_id = (const void*)cs;
        if (rc) return rc;
        if (er != hipSuccess) return fail(c, VP_ERR_HIP, std::string("hipEventRecord(ev_sw): ") + hipGetErrorString(er));
        return VP_OK;
    }
    if ((rc = adopt_stream(c, c->own_stream))) return rc;
    if (!c->ev_in) HIPCHK(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
    if (!c->ev_out) HIPCHK(c, hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
    // everything the caller enqueued on its stream so far (the producers of the inputs) happens before the library's kernels ...
    HIPCHK(c, hipEventRecord(c->ev_in, cs));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_in, 0));
    if ((rc = chunks())) return rc;
    // ... and whatever the caller enqueues afterwards (consumers of the outputs) happens after them
    HIPCHK(c, hipEventRecord(c->ev_out, c->stream));
    HIPCHK(c, hipStreamWaitEvent(cs, c->ev_out, 0));
    return VP_OK;
}

// ---- per-crop expert entries: what vp_infer_experts_device_stream, vp_infer_frames_experts and vp_infer_boxes_experts_stream share
// every refusal of such a call, before anything is enqueued (the entry's own argument checks and check_ready come first)
int mix_ready(vp_ctx* c, const char* who, int n, const int32_t* expert_ids) {
    if (!c->n_experts) return fail(c, VP_ERR_STATE, std::string(who) + ": the handle holds a plain (single-dataset) checkpoint, not a ViTPose+ one");
    std::string why;
    if (mix_check_ids(expert_ids, n, c->n_experts, &why)) return fail(c, VP_ERR_INVALID, why);
    if (c->flip_on && !c->flip_ex)
        return fail(c, VP_ERR_STATE, std::string(who) + " does not run under the flip-test mode (one partner table per handle, not per crop): call vp_clear_flip_test first");
    return slots_idle(c, who);
}

// the plan of chunk [off, off + nb) and its tables onto the device: kernel arguments only, MIX_CROPS_PER_LAUNCH positions per launch, on c->stream
// (the ids were checked for the whole call by mix_ready; the plan and its scratch live in the handle: no allocation per chunk once they have grown)
int mix_chunk_tables(vp_ctx* c, const int32_t* expert_ids, int off, int nb, MixPlan& p) {
    mix_plan(expert_ids + off, nb, c->n_experts, p);
    const int B = (c->maxb + 3) / 4 * 4;
    std::vector<int32_t>&ks = c->mix_ks, &first = c->mix_first, &K = c->mix_k;
    ks.resize(c->n_experts); first.resize(nb); K.resize(nb);
    for (int e = 0; e < c->n_experts; ++e) ks[e] = c->ex_heads[e].K;
    if (c->flip_ex) mix_records_flip(p, ks.data(), c->Kmax, first.data(), K.data());   // the per-expert flip-test mode: nb <= max_batch / 2 crops, two forward rows each
    else mix_records(p, ks.data(), c->Kmax, first.data(), K.data());
    for (int base = 0; base < nb; base += vp::MIX_CROPS_PER_LAUNCH) {
        vp::MixTable t;
        std::memset(&t, 0, sizeof(t));
        t.base = base; t.count = std::min(nb - base, vp::MIX_CROPS_PER_LAUNCH);
        t.pad_to = base + t.count == nb ? B : 0;   // encoder padding crops repeat the last crop (pick_run_batch)
        for (int i = 0; i < t.count; ++i) { t.id[i] = p.ids[base + i]; t.order[i] = p.order[base + i]; t.first[i] = first[base + i]; t.K[i] = K[base + i]; }
        if (c->flip_ex)
            LAUNCH(c, VP_PROF_IM2COL, 0.0, 48.0 * t.count, vp::mix_tables_flip_launch(t, c->expert_ids, c->expert_ids + B, c->mix_slot, c->mix_recs, c->mix_recs_flip, c->stream));
        else
            LAUNCH(c, VP_PROF_IM2COL, 0.0, 28.0 * t.count, vp::mix_tables_launch(t, c->expert_ids, c->expert_ids + B, c->mix_slot, c->mix_recs, c->stream));
    }
    return VP_OK;
}

// run_chunk under plan p; whatever it returns, the handle's own expert is the active one again (an eager chunk leaves its last segment's)
int run_mix_chunk(vp_ctx* c, const MixPlan& p, const void* d_src, int fmt, int nb, const int32_t* d_wh, float* d_out, const int32_t* post = nullptr) {
    const int own = c->expert;
    c->mix = &p;
    const int rc = run_chunk(c, d_src, fmt, nb, d_wh, d_out, post);
    c->mix = nullptr;
    use_expert(c, own);
    return rc;
}

}  // namespace

namespace vpi {   // shared with debug_taps.hip (vp_dbg_crop_prep) and group.hip (submit_impl)

int image_check(const vp_image& im, int f, std::string* why) {
    auto bad = [&](const std::string& m) { if (why) *why = "frame " + std::to_string(f) + " " + m; return VP_ERR_INVALID; };
    if (im.format < 0 || im.format >= vp::PIX_FORMATS) return bad("has an unknown pixel format " + std::to_string(im.format));
    const bool nv12 = im.format == vp::PIX_NV12;
    if (nv12 && (im.matrix < 0 || im.matrix >= vp::YUV_MATRICES)) return bad("has an unknown YUV matrix " + std::to_string(im.matrix));
    if (im.pitch[0] < 0 || (nv12 && im.pitch[1] < 0)) return bad("has a negative pitch");
    if (im.w > 0 && im.pitch[0] < vp::plane_row_bytes(im.format, 0, im.w))
        return bad("has pitch[0] " + std::to_string(im.pitch[0]) + " below its " + std::to_string(vp::plane_row_bytes(im.format, 0, im.w)) + " row bytes");
    if (nv12 && !im.plane[1]) return bad("is NV12 without a UV plane (plane[1] is null)");
    if (nv12 && im.w > 0 && im.pitch[1] < vp::plane_row_bytes(im.format, 1, im.w))
        return bad("has pitch[1] " + std::to_string(im.pitch[1]) + " below the " + std::to_string(vp::plane_row_bytes(im.format, 1, im.w)) + " bytes of a UV row (2 ceil(w / 2))");
    return VP_OK;
}

int image_plan(const vp_image* frames, int n_frames, const int32_t* p9, int n, int32_t* bands, std::string* why) {
    auto bad = [&](const std::string& m) { if (why) *why = m; return VP_ERR_INVALID; };
    if (n < 0) return bad("negative crop count");
    if (n > 0 && n_frames <= 0) return bad("crops given but no frames");
    if (n > 0 && (!frames || !p9)) return bad("null frame or crop table");
    const int nf = n_frames > 0 ? n_frames : 0;
    std::vector<int64_t> lo(nf, INT64_MAX), hi(nf, -1);
    for (int i = 0; i < n; ++i) {
        const int32_t* p = p9 + 9 * (size_t)i;
        const int f = p[0];
        const std::string at = "crop " + std::to_string(i) + ": ";
        if (f < 0 || f >= n_frames) return bad(at + "frame index " + std::to_string(f) + " outside [0, " + std::to_string(n_frames) + ")");
        const vp_image& fr = frames[f];
        if (!fr.plane[0]) return bad(at + "frame " + std::to_string(f) + " has no data");
        if (fr.h <= 0 || fr.w <= 0) return bad(at + "frame " + std::to_string(f) + " has a non-positive size");
        if (hi[f] < 0) {   // the first crop that names the frame: its layout
            std::string w;
            if (image_check(fr, f, &w)) return bad(at + w);
        }
        const int64_t x0 = p[1], y0 = p[2], cw = p[3], ch = p[4], left = p[5], top = p[6], pw = p[7], ph = p[8];
        if (cw <= 0 || ch <= 0 || pw <= 0 || ph <= 0) return bad(at + "non-positive crop or canvas size");
        if (x0 < 0 || y0 < 0 || x0 + cw > fr.w || y0 + ch > fr.h || left < 0 || top < 0 || left + cw > pw || top + ch > ph)
            return bad(at + "lies outside frame " + std::to_string(f) + " / its padded canvas");
        lo[f] = std::min(lo[f], y0);
        hi[f] = std::max(hi[f], y0 + ch);
    }
    if (bands)
        for (int f = 0; f < nf; ++f) {
            bands[2 * f] = hi[f] < 0 ? 0 : (int32_t)lo[f];
            bands[2 * f + 1] = hi[f] < 0 ? 0 : (int32_t)hi[f];
        }
    return VP_OK;
}

int stage_bands(vp_ctx* c, const vp_image* frames, int n_frames, bool on_device, const int32_t* bands, std::vector<const uint8_t*>& row0_ptr) {
    // plane p of frame f at the first row of its band, where the kernel reads it: Y / RGB row bands[2 f], UV row bands[2 f] >> 1
    row0_ptr.assign((size_t)n_frames * 2, nullptr);
    auto band_rows = [&](int f, int p, int64_t* r0, int64_t* r1) {   // rows [*r0, *r1) of plane p the band covers
        *r0 = p ? bands[2 * f] >> 1 : bands[2 * f];
        *r1 = p ? ((int64_t)bands[2 * f + 1] + 1) >> 1 : bands[2 * f + 1];
    };
    auto planes = [&](int f) { return plane_count(frames[f]); };
    if (on_device) {
        for (int f = 0; f < n_frames; ++f) {
            if (bands[2 * f] == bands[2 * f + 1]) continue;
            if (const int rc = check_device_frame(c, frames[f], f)) return rc;
            for (int p = 0; p < planes(f); ++p) {
                int64_t r0, r1;
                band_rows(f, p, &r0, &r1);
                row0_ptr[2 * f + p] = frames[f].plane[p] + (size_t)r0 * frames[f].pitch[p];
            }
        }
    } else {
        // the band of a plane keeps the caller's pitch: (rows - 1) * pitch + row bytes, never a byte past the last pixel
        auto band_bytes = [&](int f, int p) {
            int64_t r0, r1;
            band_rows(f, p, &r0, &r1);
            return (size_t)(r1 - r0 - 1) * (size_t)frames[f].pitch[p] + (size_t)vp::plane_row_bytes(frames[f].format, p, frames[f].w);
        };
        std::vector<size_t> off((size_t)n_frames * 2, 0);
        size_t total = 0;
        for (int f = 0; f < n_frames; ++f) {
            if (bands[2 * f] == bands[2 * f + 1]) continue;
            for (int p = 0; p < planes(f); ++p) {
                off[2 * f + p] = total;
                total += (band_bytes(f, p) + 255) & ~(size_t)255;
            }
        }
        if (const int rc = grow_buffer(c, &c->frame_stage, &c->frame_cap, total, "frame staging arena")) return rc;
        for (int f = 0; f < n_frames; ++f) {   // ONE copy per plane of a frame with crops: its row band, full width
            if (bands[2 * f] == bands[2 * f + 1]) continue;
            for (int p = 0; p < planes(f); ++p) {
                int64_t r0, r1;
                band_rows(f, p, &r0, &r1);
                HIPCHK(c, hipMemcpyAsync(c->frame_stage + off[2 * f + p], frames[f].plane[p] + (size_t)r0 * frames[f].pitch[p], band_bytes(f, p), hipMemcpyHostToDevice,
                                         c->stream));
                row0_ptr[2 * f + p] = c->frame_stage + off[2 * f + p];
            }
        }
    }
    return VP_OK;
}

int stage_frames(vp_ctx* c, const vp_image* frames, int n_frames, bool on_device, const int32_t* p9, int n, const int32_t* bands,
                 std::vector<vp::CropRec>& recs) {
    std::vector<const uint8_t*> row0_ptr;
    if (const int rc = stage_bands(c, frames, n_frames, on_device, bands, row0_ptr)) return rc;
    recs.resize(n);
    for (int i = 0; i < n; ++i) {
        const int32_t* p = p9 + 9 * (size_t)i;
        const int f = p[0];
        const vp_image& im = frames[f];
        const bool nv12 = im.format == vp::PIX_NV12;
        vp::CropRec& r = recs[i];
        r.src = row0_ptr[2 * f] + (size_t)(p[2] - bands[2 * f]) * im.pitch[0] + (size_t)p[1] * (nv12 ? 1 : 3);
        r.pitch = im.pitch[0];
        r.cw = p[3]; r.ch = p[4]; r.left = p[5]; r.top = p[6]; r.pw = p[7]; r.ph = p[8];
        r.src1 = nv12 ? row0_ptr[2 * f + 1] + (size_t)((p[2] >> 1) - (bands[2 * f] >> 1)) * im.pitch[1] + (size_t)(p[1] >> 1) * 2 : nullptr;
        r.pitch1 = nv12 ? im.pitch[1] : 0;
        r.format = im.format; r.matrix = im.matrix; r.oy = p[2] & 1; r.ox = p[1] & 1;
    }
    return VP_OK;
}

int affine_plan(const vp_image* frames, int n_frames, const int32_t* frame_idx, const float* cs, int n, int32_t* bands, std::string* why) {
    auto bad = [&](const std::string& m) { if (why) *why = m; return VP_ERR_INVALID; };
    if (n < 0) return bad("negative crop count");
    if (n > 0 && n_frames <= 0) return bad("crops given but no frames");
    if (n > 0 && (!frames || !cs)) return bad("null frame table or centre / scale table");
    const int nf = n_frames > 0 ? n_frames : 0;
    std::vector<int32_t> lo(nf, INT32_MAX), hi(nf, -1);
    std::vector<uint8_t> seen(nf, 0);
    for (int i = 0; i < n; ++i) {
        const int f = frame_idx ? frame_idx[i] : 0;
        const float* q = cs + 4 * (size_t)i;
        const std::string at = "crop " + std::to_string(i) + ": ";
        if (f < 0 || f >= n_frames) return bad(at + "frame index " + std::to_string(f) + " outside [0, " + std::to_string(n_frames) + ")");
        const vp_image& fr = frames[f];
        if (!fr.plane[0]) return bad(at + "frame " + std::to_string(f) + " has no data");
        if (fr.h <= 0 || fr.w <= 0 || fr.h > vp::BOX_MAX_SIDE || fr.w > vp::BOX_MAX_SIDE) return bad(at + "frame " + std::to_string(f) + " has a size outside [1, 2^24]");
        if (!seen[f]) {   // the first crop that names the frame: its layout
            std::string w;
            if (image_check(fr, f, &w)) return bad(at + w);
            seen[f] = 1;
        }
        if (!vp::cs_valid(q)) return bad(at + "centre not finite, or a scale that is not finite, not positive or above 2^24");
        int32_t l, h;
        vp::affine_row_band(q, fr.h, &l, &h);
        if (l < h) { lo[f] = std::min(lo[f], l); hi[f] = std::max(hi[f], h); }
    }
    if (bands)
        for (int f = 0; f < nf; ++f) {
            bands[2 * f] = hi[f] < 0 ? 0 : lo[f];
            bands[2 * f + 1] = hi[f] < 0 ? 0 : hi[f];
        }
    return VP_OK;
}

void affine_records(const vp_image* frames, const int32_t* frame_idx, const float* cs, int n, const int32_t* bands, const std::vector<const uint8_t*>& row0_ptr,
                    std::vector<vp::AffRec>& recs) {
    recs.resize(n);
    for (int i = 0; i < n; ++i) {
        const int f = frame_idx ? frame_idx[i] : 0;
        const vp_image& im = frames[f];
        const bool nv12 = im.format == vp::PIX_NV12;
        const vp::AffineMap m = vp::affine_map(cs + 4 * (size_t)i);
        vp::AffRec& r = recs[i];
        r.plane[0] = row0_ptr[2 * f]; r.plane[1] = nv12 ? row0_ptr[2 * f + 1] : nullptr;
        r.pitch[0] = im.pitch[0]; r.pitch[1] = nv12 ? im.pitch[1] : 0;
        r.ax = m.ax; r.bx = m.bx; r.ay = m.ay; r.by = m.by;
        r.w = im.w; r.y0 = bands[2 * f]; r.y1 = bands[2 * f + 1];   // (a frame without a band: y0 == y1, no read)
        r.format = im.format; r.matrix = im.matrix; r.pad_ = 0;
    }
}

int box_args(int n_frames, const int32_t* frame_hw, int hw_stride, int row_stride, int n, int pad, std::string* why) {
    auto bad = [&](const std::string& m) { if (why) *why = m; return VP_ERR_INVALID; };
    if (n < 0) return bad("negative box count");
    if (row_stride < 4) return bad("row_stride " + std::to_string(row_stride) + " < 4 (x1, y1, x2, y2 per row)");
    if (pad < 0) return bad("negative pad");
    if (n > 0 && n_frames <= 0) return bad("boxes given but no frames");
    for (int f = 0; f < n_frames && n > 0; ++f) {   // every frame of the table: the frame indices live on the device
        const int32_t h = frame_hw[(size_t)f * hw_stride], w = frame_hw[(size_t)f * hw_stride + 1];
        if (h <= 0 || w <= 0 || h > vp::BOX_MAX_SIDE || w > vp::BOX_MAX_SIDE)
            return bad("frame " + std::to_string(f) + " has a size outside [1, 2^24]");
    }
    return VP_OK;
}

// ---- per-crop experts: the plan of a chunk (HOST ONLY) ------------------------------------------------------------------------
int mix_check_ids(const int32_t* ids, int n, int n_experts, std::string* why) {
    auto bad = [&](const std::string& m) { if (why) *why = m; return VP_ERR_INVALID; };
    if (n > 0 && !ids) return bad("null expert_ids");
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= n_experts)
            return bad("expert id " + std::to_string(ids[i]) + " of crop " + std::to_string(i) + " outside [0, " + std::to_string(n_experts) + ")");
    return VP_OK;
}

void mix_plan(const int32_t* ids, int nb, int n_experts, MixPlan& p) {
    p.nb = nb;
    p.order.resize(nb > 0 ? nb : 0);   // (p is reused from chunk to chunk: its vectors keep their capacity)
    p.ids.resize(nb > 0 ? nb : 0);
    p.seg_e.clear();
    p.seg_s.clear();
    for (int i = 0; i < nb; ++i) p.order[i] = i;
    std::stable_sort(p.order.begin(), p.order.end(), [&](int32_t a, int32_t b) { return ids[a] < ids[b]; });
    for (int j = 0; j < nb; ++j) {
        p.ids[j] = ids[p.order[j]];
        if (j == 0 || p.ids[j] != p.ids[j - 1]) { p.seg_e.push_back(p.ids[j]); p.seg_s.push_back(j); }
    }
    p.seg_s.push_back(nb);
    p.pattern = mix_pattern(p.seg_e, p.seg_s, n_experts);
}

uint64_t mix_pattern(const std::vector<int>& seg_e, const std::vector<int>& seg_s, int n_experts) {
    if (seg_e.size() <= 1) return 0;
    if (n_experts > 8) return MIX_NO_GRAPH;
    uint64_t code = 0;
    for (size_t s = 0; s < seg_e.size(); ++s) {
        const int cnt = seg_s[s + 1] - seg_s[s];
        if (cnt > 254) return MIX_NO_GRAPH;
        code |= (uint64_t)cnt << (8 * seg_e[s]);   // one byte per expert: two count vectors share a code only if they are equal
    }
    return code;
}

void mix_records(const MixPlan& p, const int32_t* k_per_expert, int Kmax, int32_t* first, int32_t* K) {
    for (size_t s = 0; s < p.seg_e.size(); ++s)
        for (int j = p.seg_s[s]; j < p.seg_s[s + 1]; ++j) {
            K[j] = k_per_expert[p.seg_e[s]];
            first[j] = p.seg_s[s] * Kmax + (j - p.seg_s[s]) * K[j];
        }
}

void mix_records_flip(const MixPlan& p, const int32_t* k_per_expert, int Kmax, int32_t* first, int32_t* K) {
    for (size_t s = 0; s < p.seg_e.size(); ++s)
        for (int j = p.seg_s[s]; j < p.seg_s[s + 1]; ++j) {
            K[j] = k_per_expert[p.seg_e[s]];
            first[j] = 2 * p.seg_s[s] * Kmax + 2 * (j - p.seg_s[s]) * K[j];
        }
}

// ---- asynchronous host path ----------------------------------------------------------------------------------------------
// true when `p` is page-locked host memory the runtime knows (hipHostMalloc / vp_host_alloc / hipHostRegister): only such memory is
// copied asynchronously as it is
static bool host_ptr_is_pinned(const void* p) {
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // unknown to the runtime = pageable
    return a.type == hipMemoryTypeHost;
}

// stage_out: the D2H targets the slot's own pinned buffer and vp_infer_wait copies it to `out` (the group path: the caller's
// memory may be pageable, and an asynchronous copy to pageable memory is host-synchronous -- it would hold the submission until the
// compute is over and serialise the devices of a group)
int submit_impl(vp_ctx* c, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out, int32_t* slot_out, bool stage_out) {
    int rc = check_ready(c, fmt, n, crops, out);
    if (rc) return rc;
    if (!slot_out) return fail(c, VP_ERR_INVALID, "null slot pointer");
    if (n <= 0 || n > chunk_cap(c))
        return fail(c, VP_ERR_INVALID, c->flip_on ? "vp_infer_submit takes 1 .. max_batch / 2 crops per call while the flip-test mode is on" : "vp_infer_submit takes 1 .. max_batch crops per call");
    if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->d2h_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking));
    const int si = c->next_slot;
    vp_ctx::Slot& sl = c->slots[si];
    if (sl.busy) return fail(c, VP_ERR_STATE, "both slots in flight: call vp_infer_wait first");
    if (!sl.in) {
        char* q;
        if ((rc = dalloc(c, &q, (size_t)c->maxb * crop_bytes(VP_INPUT_F32_NCHW)))) return rc;
        sl.in = q;
    }
    if (!sl.wh && (rc = dalloc(c, &sl.wh, (size_t)c->maxb * 2))) return rc;
    if (!sl.kp && (rc = dalloc(c, &sl.kp, (size_t)c->maxb * c->Kmax * 3))) return rc;
    if (!sl.h2d) HIPCHK(c, hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming));
    if (!sl.done) HIPCHK(c, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    if (!sl.out) HIPCHK(c, hipEventCreateWithFlags(&sl.out, hipEventDisableTiming));
    // copy stream: H2D of this call (the slot's previous D2H finished: vp_infer_wait was called on it)
    const size_t in_bytes = (size_t)n * crop_bytes(fmt);
    if (stage_out && !host_ptr_is_pinned(crops)) {
        // the group path with pageable caller memory: staged through the slot's pinned buffer in 4 MiB pieces, so that this call never
        // waits for a device (hipMemcpyAsync from pageable memory held member i + 1's submission behind member i's staging)
        if (sl.host_in_cap < in_bytes) {
            if (sl.host_in) { HIPCHK(c, hipStreamSynchronize(c->copy_stream)); hipHostFree(sl.host_in); sl.host_in = nullptr; sl.host_in_cap = 0; }
            void* q = nullptr;
            HIPCHK(c, hipHostMalloc(&q, in_bytes, hipHostMallocDefault));
            sl.host_in = (char*)q; sl.host_in_cap = in_bytes;
        }
        const size_t piece = (size_t)4 << 20;
        for (size_t off = 0; off < in_bytes; off += piece) {
            const size_t len = in_bytes - off < piece ? in_bytes - off : piece;
            std::memcpy(sl.host_in + off, (const char*)crops + off, len);
            HIPCHK(c, hipMemcpyAsync((char*)sl.in + off, sl.host_in + off, len, hipMemcpyHostToDevice, c->copy_stream));
        }
    } else {
        HIPCHK(c, hipMemcpyAsync(sl.in, crops, in_bytes, hipMemcpyHostToDevice, c->copy_stream));
    }
    if (org_wh) HIPCHK(c, hipMemcpyAsync(sl.wh, org_wh, (size_t)n * 8, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(c, hipEventRecord(sl.h2d, c->copy_stream));
    // compute stream: after the upload
    HIPCHK(c, hipStreamWaitEvent(c->stream, sl.h2d, 0));
    if ((rc = run_chunk(c, sl.in, fmt, n, org_wh ? sl.wh : nullptr, sl.kp))) return rc;
    HIPCHK(c, hipEventRecord(sl.done, c->stream));
    // download stream: D2H of the keypoints after the compute
    HIPCHK(c, hipStreamWaitEvent(c->d2h_stream, sl.done, 0));
    float* dst = out;
    sl.user_out = nullptr;
    if (stage_out) {
        if (!sl.host_kp) {
            void* q = nullptr;
            HIPCHK(c, hipHostMalloc(&q, (size_t)c->maxb * c->Kmax * 12, hipHostMallocDefault));
            sl.host_kp = (float*)q;
        }
        dst = sl.host_kp;
        sl.user_out = out;
        sl.out_bytes = (size_t)n * c->Kp * 12;
    }
    HIPCHK(c, hipMemcpyAsync(dst, sl.kp, (size_t)n * c->Kp * 12, hipMemcpyDeviceToHost, c->d2h_stream));
    HIPCHK(c, hipEventRecord(sl.out, c->d2h_stream));
    sl.busy = true;
    *slot_out = si;
    c->next_slot = si ^ 1;
    return VP_OK;
}

}  // namespace vpi

extern "C" {

int vp_infer_device(vp_handle c, const void* d_crops, int32_t fmt, int32_t n, const int32_t* d_org_wh, float* d_out, int32_t sync) {
    int rc = check_ready(c, fmt, n, d_crops, d_out);
    if (rc || (rc = device_chunks(c, d_crops, fmt, n, d_org_wh, d_out))) return rc;
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

int vp_infer_device_stream(vp_handle c, const void* d_crops, int32_t fmt, int32_t n, const int32_t* d_org_wh, float* d_out, void* caller_stream) {
    const int rc = check_ready(c, fmt, n, d_crops, d_out, false);
    if (rc) return rc;
    return caller_ordered(c, (hipStream_t)caller_stream, n, [&]() { return device_chunks(c, d_crops, fmt, n, d_org_wh, d_out); });
}

int vp_infer(vp_handle c, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out) {
    int rc = check_ready(c, fmt, n, crops, out);
    if (rc) return rc;
    const int cap = chunk_cap(c);
    if (n > cap && !slots_busy(c)) {
        // more than one chunk: through the two asynchronous slots, so that the upload of chunk i+1 and the download of chunk i-1
        // run under the compute of chunk i (fully overlapped when the caller's buffers are pinned; pageable buffers still work,
        // the runtime stages them synchronously)
        int pending[2], np = 0;
        rc = for_chunks(n, cap, [&](int off, int nb) -> int {
            int32_t slot = -1;
            int r = vp_infer_submit(c, (const char*)crops + (size_t)off * crop_bytes(fmt), fmt, nb, org_wh ? org_wh + 2 * (size_t)off : nullptr,
                                    out + (size_t)off * c->Kp * 3, &slot);
            if (r) return r;
            pending[np++] = slot;
            if (np < 2) return VP_OK;
            r = vp_infer_wait(c, pending[0]);
            pending[0] = pending[1]; np = 1;
            return r;
        });
        for (int i = 0; i < np; ++i) {   // whatever is still in flight, after an error too; the first error is the call's
            const int r = vp_infer_wait(c, pending[i]);
            if (!rc) rc = r;
        }
        return rc;
    }
    return for_chunks(n, cap, [&](int off, int nb) -> int {
        int r = stage_in(c, crops, fmt, org_wh, off, nb);
        if (r || (r = run_chunk(c, c->in_stage, fmt, nb, org_wh ? c->wh_stage : nullptr, c->kp))) return r;
        return copy_out_sync(c, out, c->kp, (size_t)c->Kp * 3, off, nb);
    });
}

int vp_infer_submit(vp_handle c, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out, int32_t* slot_out) {
    return submit_impl(c, crops, fmt, n, org_wh, out, slot_out, false);
}

int vp_infer_wait(vp_handle c, int32_t slot) {
    if (!c || slot < 0 || slot > 1) return VP_ERR_INVALID;
    vp_ctx::Slot& sl = c->slots[slot];
    if (!sl.busy) return fail(c, VP_ERR_STATE, "slot not in flight");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipEventSynchronize(sl.out));
    if (sl.user_out) { std::memcpy(sl.user_out, sl.host_kp, sl.out_bytes); sl.user_out = nullptr; }
    sl.busy = false;
    return VP_OK;
}

int vp_infer_flip(vp_handle c, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, const int32_t* flip_pairs,
                  int32_t n_pairs, int32_t shift_heatmap, float* out, float* heatmaps) {
    int rc = check_ready(c, fmt, n, crops, out ? (const void*)out : (const void*)heatmaps);
    if (rc) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && !flip_pairs)) return fail(c, VP_ERR_INVALID, "bad flip_pairs");
    if (n == 0) return VP_OK;   // nothing to do (and no async upload of the stack-lifetime partner table left in flight)
    std::vector<int32_t> partner(c->Kp);
    std::string why;
    if (flip_partner_table(c->Kp, flip_pairs, n_pairs, partner.data(), &why)) return fail(c, VP_ERR_INVALID, "vp_infer_flip: " + why);
    const size_t hm_elems = (size_t)c->maxb * c->Kmax * 3072;
    if (!c->hm_keep && (rc = dalloc(c, &c->hm_keep, hm_elems))) return rc;
    if (!c->partner && (rc = dalloc(c, &c->partner, (size_t)c->Kmax))) return rc;
    HIPCHK(c, hipMemcpy(c->partner, partner.data(), (size_t)c->Kp * 4, hipMemcpyHostToDevice));   // synchronous: `partner` is a local
    FwdOpts mirrored;
    mirrored.mirror = true;
    return for_chunks(n, c->maxb, [&](int off, int nb) -> int {   // its own two passes of up to max_batch crops, whatever the handle's mode
        int rc = stage_in(c, crops, fmt, org_wh, off, nb);
        if (rc || (rc = forward_chunk(c, c->in_stage, fmt, nb))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->hm_keep, c->hm, (size_t)nb * c->Kp * 3072 * 4, hipMemcpyDeviceToDevice, c->stream));
        if ((rc = forward_chunk(c, c->in_stage, fmt, nb, mirrored))) return rc;   // mirrored crops -> c->hm
        HIPCHK(c, vp::flip_merge_launch(c->hm_keep, c->hm, c->partner, nb, c->Kp, shift_heatmap ? 1 : 0, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->hm, c->hm_keep, (size_t)nb * c->Kp * 3072 * 4, hipMemcpyDeviceToDevice, c->stream));
        if (heatmaps && (rc = copy_out(c, heatmaps, c->hm, (size_t)c->Kp * 3072, off, nb))) return rc;
        if (out && ((rc = decode_chunk(c, org_wh ? c->wh_stage : nullptr, c->kp, nb, false)) || (rc = copy_out(c, out, c->kp, (size_t)c->Kp * 3, off, nb)))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return VP_OK;
    });
}

int vp_infer_heatmaps(vp_handle c, const void* crops, int32_t fmt, int32_t n, float* heatmaps) {
    int rc = check_ready(c, fmt, n, crops, heatmaps);
    if (rc) return rc;
    const size_t map_elems = (size_t)c->Kp * 3072, map_bytes = map_elems * 4;
    return for_chunks(n, chunk_cap(c), [&](int off, int nb) -> int {
        int rc = stage_in(c, crops, fmt, nullptr, off, nb);
        if (rc || (rc = forward_mode_chunk(c, c->in_stage, fmt, nb))) return rc;
        if (!c->flip_on) return copy_out_sync(c, heatmaps, c->hm, map_elems, off, nb);
        // the averaged maps, materialised in the straight crops' slots (every second one of the interleaved batch)
        HIPCHK(c, vp::flip_merge_launch(c->hm, c->hm + map_elems, flip_table_now(c), nb, c->Kp, c->flip_shift, c->stream, 1));
        HIPCHK(c, hipMemcpy2DAsync(heatmaps + (size_t)off * map_elems, map_bytes, c->hm, 2 * map_bytes, map_bytes, (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return VP_OK;
    });
}

int vp_infer_tokens(vp_handle c, const void* crops, int32_t fmt, int32_t n, float* tokens) {
    int rc = check_ready(c, fmt, n, crops, tokens);
    if (rc) return rc;
    if (!c->tok && (rc = dalloc(c, &c->tok, (size_t)c->maxb * 192 * c->D))) return rc;
    FwdOpts with_tokens;
    with_tokens.tokens = true;
    return for_chunks(n, c->maxb, [&](int off, int nb) -> int {
        int rc = stage_in(c, crops, fmt, nullptr, off, nb);
        if (rc || (rc = forward_chunk(c, c->in_stage, fmt, nb, with_tokens))) return rc;
        return copy_out_sync(c, tokens, c->tok, (size_t)192 * c->D, off, nb);
    });
}

int vp_infer_experts(vp_handle c, const void* crops, int32_t fmt, int32_t n, const int32_t* expert_ids, const int32_t* org_wh, float* out) {
    int rc = check_ready(c, fmt, n, crops, out);
    if (rc || (rc = mix_ready(c, "vp_infer_experts", n, expert_ids))) return rc;
    return for_chunks(n, chunk_cap(c), [&](int off, int nb) -> int {   // the host-staged caller of the per-crop chunk: its twins' plan, tables, body and replay
        MixPlan& p = c->mix_host;
        int rc = mix_chunk_tables(c, expert_ids, off, nb, p);
        if (rc) return rc;
        // The crops go up in the caller's order.  Ids that never decrease (one expert among them) are the expert order already: straight into in_stage.
        // Any other chunk goes into mix_stage, and the chunk body gathers: it does so exactly when its source is not in_stage
        void* src = c->in_stage;
        if (!std::is_sorted(expert_ids + off, expert_ids + off + nb)) {
            if ((rc = grow_buffer(c, &c->mix_stage, &c->mix_stage_cap, (size_t)((c->maxb + 3) / 4 * 4) * crop_bytes(fmt), "mixed-batch staging buffer"))) return rc;
            src = c->mix_stage;
        }
        // the sizes stay in the caller's order too: the record route reads the row it writes
        if ((rc = stage_in(c, crops, fmt, org_wh, off, nb, src)) || (rc = run_mix_chunk(c, p, src, fmt, nb, org_wh ? c->wh_stage : nullptr, c->kp))) return rc;
        return copy_out_sync(c, out, c->kp, (size_t)c->Kmax * 3, off, nb);
    });
}

int vp_infer_experts_device_stream(vp_handle c, const void* d_crops, int32_t fmt, int32_t n, const int32_t* expert_ids, const int32_t* d_org_wh, float* d_out,
                                   void* caller_stream) {
    int rc = check_ready(c, fmt, n, d_crops, d_out, false);
    if (rc || (rc = mix_ready(c, "vp_infer_experts_device_stream", n, expert_ids))) return rc;
    return caller_ordered(c, (hipStream_t)caller_stream, n, [&]() {
        return for_chunks(n, chunk_cap(c), [&](int off, int nb) -> int {   // vp_infer_experts' chunks: the same crops per chunk, so the same plan and bits
            MixPlan& p = c->mix_host;
            if (const int rc = mix_chunk_tables(c, expert_ids, off, nb, p)) return rc;
            return run_mix_chunk(c, p, (const char*)d_crops + (size_t)off * crop_bytes(fmt), fmt, nb, d_org_wh ? d_org_wh + 2 * (size_t)off : nullptr,
                                 d_out + (size_t)off * c->Kmax * 3);
        });
    });
}

// vp_infer_frames (mixed == false) and vp_infer_frames_experts (a flag, not a null test: null ids are an error of the latter)
static int frames_impl(vp_ctx* c, const char* who, const vp_image* frames, int32_t n_frames, int32_t on_device, const int32_t* p9, int32_t n, const int32_t* expert_ids,
                       bool mixed, float* out) {
    if (!c) return VP_ERR_INVALID;
    std::vector<int32_t> bands((size_t)(n_frames > 0 ? n_frames : 0) * 2);
    std::string why;
    if (image_plan(frames, n_frames, p9, n, bands.data(), &why)) return fail(c, VP_ERR_INVALID, why);   // before any copy or launch
    int rc = check_ready(c, VP_INPUT_U8_NHWC, n, p9, out);
    if (rc || (mixed && (rc = mix_ready(c, who, n, expert_ids))) || n == 0) return rc;
    std::vector<vp::CropRec> recs;
    if ((rc = stage_frames(c, frames, n_frames, on_device != 0, p9, n, bands.data(), recs))) return rc;
    if (!c->crecs && (rc = dalloc(c, &c->crecs, (size_t)c->maxb))) return rc;
    std::vector<int32_t> wh((size_t)c->maxb * 2);
    std::vector<vp::CropRec> sorted(mixed ? (size_t)c->maxb : 0);
    return for_chunks(n, chunk_cap(c), [&](int off, int nb) -> int {   // vp_infer's chunks: the same crops per chunk, so the same (plan and) bits
        MixPlan& p = c->mix_host;
        const vp::CropRec* src = recs.data() + off;
        if (mixed) {   // the tables first; the records go to their place in the expert order
            if (const int rc = mix_chunk_tables(c, expert_ids, off, nb, p)) return rc;
            for (int j = 0; j < nb; ++j) sorted[j] = recs[(size_t)off + p.order[j]];
            src = sorted.data();
        }
        HIPCHK(c, hipMemcpyAsync(c->crecs, src, (size_t)nb * sizeof(vp::CropRec), hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, VP_PROF_IM2COL, 0.0, (double)nb * 256 * 192 * 3 * 5, vp::crop_resize_launch(c->crecs, (uint8_t*)c->in_stage, nb, c->stream));
        // decode scales by the padded-canvas size (pw, ph) of each crop = the image pre_img receives; in the caller's order (the record route reads the row it writes)
        for (int i = 0; i < nb; ++i) { wh[2 * i] = p9[9 * (size_t)(off + i) + 7]; wh[2 * i + 1] = p9[9 * (size_t)(off + i) + 8]; }
        HIPCHK(c, hipMemcpyAsync(c->wh_stage, wh.data(), (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // recs / sorted / wh are rewritten for the next chunk
        if (const int rc = mixed ? run_mix_chunk(c, p, c->in_stage, VP_INPUT_U8_NHWC, nb, c->wh_stage, c->kp) : run_chunk(c, c->in_stage, VP_INPUT_U8_NHWC, nb, c->wh_stage, c->kp))
            return rc;
        return copy_out_sync(c, out, c->kp, (size_t)(mixed ? c->Kmax : c->Kp) * 3, off, nb);
    });
}

int vp_infer_frames_experts(vp_handle c, const vp_frame* frames, int32_t n_frames, int32_t on_device, const int32_t* p9, int32_t n, const int32_t* expert_ids,
                            float* out) {
    return frames_impl(c, "vp_infer_frames_experts", table_ptr(rgb_images(frames, n_frames)), n_frames, on_device, p9, n, expert_ids, true, out);
}

int vp_infer_frames(vp_handle c, const vp_frame* frames, int32_t n_frames, int32_t on_device, const int32_t* p9, int32_t n, float* out) {
    return frames_impl(c, "vp_infer_frames", table_ptr(rgb_images(frames, n_frames)), n_frames, on_device, p9, n, nullptr, false, out);
}

int vp_infer_images(vp_handle c, const vp_image* images, int32_t n_images, int32_t on_device, const int32_t* p9, int32_t n, const int32_t* expert_ids, float* out) {
    return frames_impl(c, "vp_infer_images", images, n_images, on_device, p9, n, expert_ids, expert_ids != nullptr, out);
}

// the one-frame case of vp_infer_frames
int vp_infer_frame(vp_handle c, const uint8_t* frame, int32_t fh, int32_t fw, const int32_t* crop_params, int32_t n, float* out) {
    int rc = check_ready(c, VP_INPUT_U8_NHWC, n, frame, out);
    if (rc) return rc;
    if (fh <= 0 || fw <= 0 || (n > 0 && !crop_params)) return fail(c, VP_ERR_INVALID, "bad frame geometry");
    const vp_frame fr{frame, fh, fw};
    std::vector<int32_t> p9((size_t)n * 9);
    for (int i = 0; i < n; ++i) {
        p9[9 * (size_t)i] = 0;
        std::memcpy(&p9[9 * (size_t)i + 1], crop_params + 8 * (size_t)i, 32);
    }
    return vp_infer_frames(c, &fr, 1, 0, p9.data(), n, out);
}

int vp_dbg_frame_plan(const vp_frame* frames, int32_t n_frames, const int32_t* params9, int32_t n, int32_t* bands) {
    std::string why;
    const int rc = image_plan(table_ptr(rgb_images(frames, n_frames)), n_frames, params9, n, bands, &why);
    if (rc) g_create_error = why;
    return rc;
}

int vp_dbg_image_plan(const vp_image* images, int32_t n_images, const int32_t* params9, int32_t n, int32_t* bands) {
    std::string why;
    const int rc = image_plan(images, n_images, params9, n, bands, &why);
    if (rc) g_create_error = why;
    return rc;
}

// vp_infer_boxes_stream (expert_ids == null) and vp_infer_boxes_experts_stream
static int boxes_impl(vp_ctx* c, const char* who, const vp_image* frames, int32_t n_frames, const float* d_xyxy, int32_t row_stride, const int32_t* d_frame_idx,
                      int32_t n, int32_t pad, const int32_t* expert_ids, bool mixed, float* d_out, int32_t* d_crop_params, int32_t* d_status, void* caller_stream) {
    if (!c) return VP_ERR_INVALID;
    // every host argument is checked before anything is enqueued
    if (n > 0 && (!frames || !d_xyxy || !d_out)) return fail(c, VP_ERR_INVALID, "null frame table, box or output pointer");
    std::vector<int32_t> hw((size_t)std::max(n > 0 ? n_frames : 0, 0) * 2);
    for (size_t f = 0; f < hw.size() / 2; ++f) { hw[2 * f] = frames[f].h; hw[2 * f + 1] = frames[f].w; }
    std::string why;
    if (box_args(n_frames, hw.data(), 2, row_stride, n, pad, &why)) return fail(c, VP_ERR_INVALID, why);
    for (int f = 0; f < n_frames && n > 0; ++f)   // the layout of every frame of the table
        if (image_check(frames[f], f, &why)) return fail(c, VP_ERR_INVALID, why);
    int rc = check_ready(c, VP_INPUT_U8_NHWC, n, d_xyxy, d_out, false);
    if (rc || (mixed && (rc = mix_ready(c, who, n, expert_ids))) || n == 0) return rc;
    for (int f = 0; f < n_frames; ++f)   // every frame of the table: which ones the boxes name is on the device
        if ((rc = check_device_frame(c, frames[f], f))) return rc;
    // the chunk's crop records / decode sizes / offsets live in handle buffers sized by max_batch, allocated on the first call
    if (!c->crecs && (rc = dalloc(c, &c->crecs, (size_t)c->maxb))) return rc;
    if (!c->box_aux && (rc = dalloc(c, &c->box_aux, (size_t)c->maxb * 4))) return rc;
    return caller_ordered(c, (hipStream_t)caller_stream, n, [&]() {
        return for_chunks(n, chunk_cap(c), [&](int off, int nb) -> int {   // vp_infer_frames' chunks: the same crops per chunk, so the same plan and bits
            MixPlan& p = c->mix_host;
            if (mixed)   // the tables first: the box kernel writes each crop record to its place in the expert order (sizes, offsets, params and status stay in the caller's)
                if (const int rc = mix_chunk_tables(c, expert_ids, off, nb, p)) return rc;
            // geometry + crop run eagerly in front of the chunk's graph: the frame pointers change from call to call, the graph's buffers do not
            for (int f0 = 0; f0 < n_frames; f0 += vp::BOX_FRAMES_PER_LAUNCH) {
                vp::BoxFrames bf;
                std::memset(&bf, 0, sizeof(bf));
                bf.f0 = f0; bf.count = std::min(n_frames - f0, vp::BOX_FRAMES_PER_LAUNCH); bf.n_frames = n_frames;
                for (int j = 0; j < bf.count; ++j) {
                    const vp_image& im = frames[f0 + j];
                    bf.fr[j] = vp::BoxFrame{{im.plane[0], im.plane[1]}, {im.pitch[0], im.pitch[1]}, im.h, im.w, im.format, im.matrix};
                }
                LAUNCH(c, VP_PROF_IM2COL, 0.0, 64.0 * nb,
                       vp::box_geometry_launch(bf, d_xyxy + (size_t)off * row_stride, row_stride, d_frame_idx ? d_frame_idx + off : nullptr, nb, pad,
                                               (const uint8_t*)c->zero, c->crecs, c->wh_stage, c->box_aux,
                                               d_crop_params ? d_crop_params + (size_t)off * 9 : nullptr, d_status ? d_status + off : nullptr, c->stream,
                                               mixed ? c->mix_slot : nullptr));
            }
            LAUNCH(c, VP_PROF_IM2COL, 0.0, (double)nb * 256 * 192 * 3 * 5, vp::crop_resize_launch(c->crecs, (uint8_t*)c->in_stage, nb, c->stream));
            if (mixed) return run_mix_chunk(c, p, c->in_stage, VP_INPUT_U8_NHWC, nb, c->wh_stage, d_out + (size_t)off * c->Kmax * 3, c->box_aux);
            return run_chunk(c, c->in_stage, VP_INPUT_U8_NHWC, nb, c->wh_stage, d_out + (size_t)off * c->Kp * 3, c->box_aux);
        });
    });
}

int vp_infer_boxes_stream(vp_handle c, const vp_frame* frames, int32_t n_frames, const float* d_xyxy, int32_t row_stride, const int32_t* d_frame_idx,
                          int32_t n, int32_t pad, float* d_out, int32_t* d_crop_params, int32_t* d_status, void* caller_stream) {
    return boxes_impl(c, "vp_infer_boxes_stream", table_ptr(rgb_images(frames, n_frames)), n_frames, d_xyxy, row_stride, d_frame_idx, n, pad, nullptr, false, d_out, d_crop_params, d_status, caller_stream);
}

int vp_infer_boxes_experts_stream(vp_handle c, const vp_frame* frames, int32_t n_frames, const float* d_xyxy, int32_t row_stride, const int32_t* d_frame_idx,
                                  int32_t n, int32_t pad, const int32_t* expert_ids, float* d_out, int32_t* d_crop_params, int32_t* d_status, void* caller_stream) {
    return boxes_impl(c, "vp_infer_boxes_experts_stream", table_ptr(rgb_images(frames, n_frames)), n_frames, d_xyxy, row_stride, d_frame_idx, n, pad, expert_ids, true, d_out,
                      d_crop_params, d_status, caller_stream);
}

int vp_infer_boxes_images_stream(vp_handle c, const vp_image* images, int32_t n_images, const float* d_xyxy, int32_t row_stride, const int32_t* d_frame_idx, int32_t n,
                                 int32_t pad, const int32_t* expert_ids, float* d_out, int32_t* d_crop_params, int32_t* d_status, void* caller_stream) {
    return boxes_impl(c, "vp_infer_boxes_images_stream", images, n_images, d_xyxy, row_stride, d_frame_idx, n, pad, expert_ids, expert_ids != nullptr, d_out, d_crop_params,
                      d_status, caller_stream);
}

// ---- the affine crop route (affinegeom.h): the frames entry on host centres and scales, the boxes entry on device boxes
int vp_infer_images_affine(vp_handle c, const vp_image* images, int32_t n_images, int32_t on_device, const int32_t* frame_idx, const float* cs, int32_t n, float* out) {
    if (!c) return VP_ERR_INVALID;
    std::vector<int32_t> bands((size_t)(n_images > 0 ? n_images : 0) * 2);
    std::string why;
    if (affine_plan(images, n_images, frame_idx, cs, n, bands.data(), &why)) return fail(c, VP_ERR_INVALID, "vp_infer_images_affine: " + why);   // before any copy or launch
    int rc = check_ready(c, VP_INPUT_U8_NHWC, n, cs, out);
    if (rc || n == 0) return rc;
    std::vector<const uint8_t*> row0_ptr;
    std::vector<vp::AffRec> recs;
    if ((rc = stage_bands(c, images, n_images, on_device != 0, bands.data(), row0_ptr))) return rc;
    affine_records(images, frame_idx, cs, n, bands.data(), row0_ptr, recs);
    if (!c->arecs && (rc = dalloc(c, &c->arecs, (size_t)c->maxb))) return rc;
    if (!c->cs_stage && (rc = dalloc(c, &c->cs_stage, (size_t)c->maxb * 4))) return rc;
    return for_chunks(n, chunk_cap(c), [&](int off, int nb) -> int {   // vp_infer_images' chunks
        HIPCHK(c, hipMemcpyAsync(c->arecs, recs.data() + off, (size_t)nb * sizeof(vp::AffRec), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->cs_stage, cs + 4 * (size_t)off, (size_t)nb * 16, hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, VP_PROF_IM2COL, 0.0, (double)nb * 256 * 192 * 3 * 5, vp::crop_affine_launch(c->arecs, (uint8_t*)c->in_stage, nb, c->stream));
        if (const int rc = run_chunk(c, c->in_stage, VP_INPUT_U8_NHWC, nb, nullptr, c->kp, nullptr, c->cs_stage)) return rc;
        return copy_out_sync(c, out, c->kp, (size_t)c->Kp * 3, off, nb);   // (also: the caller's cs and recs are read before the call returns)
    });
}

int vp_infer_boxes_affine_stream(vp_handle c, const vp_image* images, int32_t n_images, const float* d_xyxy, int32_t row_stride, const int32_t* d_frame_idx, int32_t n,
                                 float box_scale, float* d_out, float* d_cs, int32_t* d_status, void* caller_stream) {
    if (!c) return VP_ERR_INVALID;
    // every host argument is checked before anything is enqueued
    if (n > 0 && (!images || !d_xyxy || !d_out)) return fail(c, VP_ERR_INVALID, "null frame table, box or output pointer");
    if (!std::isfinite(box_scale) || !(box_scale > 0.f)) return fail(c, VP_ERR_INVALID, "vp_infer_boxes_affine_stream: box_scale must be finite and > 0");
    std::vector<int32_t> hw((size_t)std::max(n > 0 ? n_images : 0, 0) * 2);
    for (size_t f = 0; f < hw.size() / 2; ++f) { hw[2 * f] = images[f].h; hw[2 * f + 1] = images[f].w; }
    std::string why;
    if (box_args(n_images, hw.data(), 2, row_stride, n, 0, &why)) return fail(c, VP_ERR_INVALID, why);
    for (int f = 0; f < n_images && n > 0; ++f)   // the layout of every frame of the table
        if (image_check(images[f], f, &why)) return fail(c, VP_ERR_INVALID, why);
    int rc = check_ready(c, VP_INPUT_U8_NHWC, n, d_xyxy, d_out, false);
    if (rc || n == 0) return rc;
    for (int f = 0; f < n_images; ++f)   // every frame of the table: which ones the boxes name is on the device
        if ((rc = check_device_frame(c, images[f], f))) return rc;
    if (!c->arecs && (rc = dalloc(c, &c->arecs, (size_t)c->maxb))) return rc;
    if (!c->cs_stage && (rc = dalloc(c, &c->cs_stage, (size_t)c->maxb * 4))) return rc;
    return caller_ordered(c, (hipStream_t)caller_stream, n, [&]() {
        return for_chunks(n, chunk_cap(c), [&](int off, int nb) -> int {   // vp_infer_images_affine's chunks: the same crops per chunk, so the same bits
            // geometry + crop run eagerly in front of the chunk's graph: the frame pointers change from call to call, the graph's buffers do not
            for (int f0 = 0; f0 < n_images; f0 += vp::BOX_FRAMES_PER_LAUNCH) {
                vp::BoxFrames bf;
                std::memset(&bf, 0, sizeof(bf));
                bf.f0 = f0; bf.count = std::min(n_images - f0, vp::BOX_FRAMES_PER_LAUNCH); bf.n_frames = n_images;
                for (int j = 0; j < bf.count; ++j) {
                    const vp_image& im = images[f0 + j];
                    bf.fr[j] = vp::BoxFrame{{im.plane[0], im.plane[1]}, {im.pitch[0], im.pitch[1]}, im.h, im.w, im.format, im.matrix};
                }
                LAUNCH(c, VP_PROF_IM2COL, 0.0, 64.0 * nb,
                       vp::box_cs_launch(bf, d_xyxy + (size_t)off * row_stride, row_stride, d_frame_idx ? d_frame_idx + off : nullptr, nb, box_scale, c->arecs, c->cs_stage,
                                         d_cs ? d_cs + (size_t)off * 4 : nullptr, d_status ? d_status + off : nullptr, c->stream));
            }
            LAUNCH(c, VP_PROF_IM2COL, 0.0, (double)nb * 256 * 192 * 3 * 5, vp::crop_affine_launch(c->arecs, (uint8_t*)c->in_stage, nb, c->stream));
            return run_chunk(c, c->in_stage, VP_INPUT_U8_NHWC, nb, nullptr, d_out + (size_t)off * c->Kp * 3, nullptr, c->cs_stage);
        });
    });
}

int vp_dbg_box_cs(const float* xyxy, int32_t row_stride, const int32_t* frame_idx, int32_t n_frames, int32_t n, float box_scale, float* cs, int32_t* status) {
    std::string why;
    if (n < 0) why = "negative box count";
    else if (n > 0 && !xyxy) why = "null box table";
    else if (row_stride < 4) why = "row_stride " + std::to_string(row_stride) + " < 4 (x1, y1, x2, y2 per row)";
    else if (!std::isfinite(box_scale) || !(box_scale > 0.f)) why = "box_scale must be finite and > 0";
    if (!why.empty()) { g_create_error = why; return VP_ERR_INVALID; }
    for (int i = 0; i < n; ++i) {   // what box_cs_kernel computes for box i
        const int32_t f = frame_idx ? frame_idx[i] : 0;
        float q[4] = {0.f, 0.f, 0.f, 0.f};
        int st = vp::BOX_BAD_FRAME;
        if (f >= 0 && f < n_frames) {
            const float* b = xyxy + (size_t)i * row_stride;
            st = vp::box_cs(b[0], b[1], b[2], b[3], box_scale, q);
            if (st != vp::BOX_OK) q[0] = q[1] = q[2] = q[3] = 0.f;
        }
        if (cs) std::memcpy(cs + 4 * (size_t)i, q, sizeof(q));
        if (status) status[i] = st;
    }
    return VP_OK;
}

int vp_dbg_affine_plan(const vp_image* images, int32_t n_images, const int32_t* frame_idx, const float* cs, int32_t n, int32_t* bands) {
    std::string why;
    const int rc = affine_plan(images, n_images, frame_idx, cs, n, bands, &why);
    if (rc) g_create_error = why;
    return rc;
}

int vp_dbg_box_geometry(const float* xyxy, int32_t row_stride, const int32_t* frame_idx, const int32_t* frame_hw, int32_t n_frames, int32_t n, int32_t pad,
                        int32_t* out9, int32_t* status) {
    std::string why;
    if (n > 0 && (!xyxy || (n_frames > 0 && !frame_hw))) why = "null box or frame table";
    const int rc = why.empty() ? box_args(n_frames, frame_hw, 2, row_stride, n, pad, &why) : (int)VP_ERR_INVALID;
    if (rc) { g_create_error = why; return rc; }
    for (int i = 0; i < n; ++i) {   // what box_geometry_kernel computes for box i
        const int32_t f = frame_idx ? frame_idx[i] : 0;
        int32_t p8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int st = vp::BOX_BAD_FRAME;
        if (f >= 0 && f < n_frames) {
            const float* b = xyxy + (size_t)i * row_stride;
            st = vp::box_geometry(b[0], b[1], b[2], b[3], frame_hw[2 * (size_t)f], frame_hw[2 * (size_t)f + 1], pad, p8);
            if (st != vp::BOX_OK) std::memset(p8, 0, sizeof(p8));
        }
        if (out9) {
            out9[9 * (size_t)i] = st == vp::BOX_OK ? f : 0;
            std::memcpy(out9 + 9 * (size_t)i + 1, p8, sizeof(p8));
        }
        if (status) status[i] = st;
    }
    return VP_OK;
}

// One decode launch on host data, on device `device_id`: the scratch, the uploads, the launch, the download (into NaN: every value must be written), the frees.
// records != null: n_maps maps by records into [n, k] rows;  partner != null: the interleaved [n_maps = 2 n, k, 64, 48] of the flip-test mode;  neither: [n, k, 64, 48];
// both (n_tables > 0): four-field records and a [n_tables, k] partner table, the per-expert flip-test mode
static int decode_host(const char* who, int32_t device_id, const float* heatmaps, size_t n_maps, int32_t n, int32_t k, const int32_t* partner, int32_t shift,
                       const int32_t* records, const int32_t* org_wh, float* out, int32_t n_tables = 0, const float* cs = nullptr) {
    if (!heatmaps || !out || n <= 0 || k <= 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, VP_ERR_HIP, "no HIP device available (no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, VP_ERR_INVALID, "device_id out of range");
    vp_ctx* c = nullptr;   // errors below are reported through the create-error slot
    HIPCHK(c, hipSetDevice(device_id));
    void* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // the maps, the sizes (the affine route: cs [n, 4]), the partner table, the records (each where given), the output
    const void* h[4] = {heatmaps, cs ? (const void*)cs : (const void*)org_wh, partner, records};
    const size_t bytes[5] = {n_maps * 3072 * 4, (size_t)n * (cs ? 16 : 8), (size_t)k * 4 * (n_tables ? n_tables : 1), (size_t)n * (n_tables ? sizeof(vp::MixRecFlip) : sizeof(vp::MixRec)),
                             (size_t)n * k * 12};
    hipError_t e = hipMalloc(&d[4], bytes[4]);
    if (e == hipSuccess) e = hipMemset(d[4], 0xff, bytes[4]);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) {
        if (!h[i]) continue;
        e = hipMalloc(&d[i], bytes[i]);
        if (e == hipSuccess) e = hipMemcpy(d[i], h[i], bytes[i], hipMemcpyHostToDevice);
    }
    const float* d_hm = (const float*)d[0];
    const int32_t* d_wh = (const int32_t*)d[1];
    if (e == hipSuccess)
        e = cs        ? (partner ? vp::decode_affine_flip_launch(d_hm, (const int32_t*)d[2], shift ? 1 : 0, (const float*)d[1], (float*)d[4], n, k, nullptr)
                                 : vp::decode_affine_launch(d_hm, (const float*)d[1], (float*)d[4], n, k, nullptr))
            : n_tables ? vp::decode_flip_mix_launch(d_hm, (const vp::MixRecFlip*)d[3], (const int32_t*)d[2], shift ? 1 : 0, d_wh, (float*)d[4], n, k, nullptr)
            : records ? vp::decode_mix_launch(d_hm, (const vp::MixRec*)d[3], d_wh, (float*)d[4], n, k, nullptr)
            : partner   ? vp::decode_flip_launch(d_hm, (const int32_t*)d[2], shift ? 1 : 0, d_wh, (float*)d[4], n, k, nullptr)
                        : vp::decode_launch(d_hm, d_wh, (float*)d[4], n, k, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d[4], bytes[4], hipMemcpyDeviceToHost);
    const int rc = e == hipSuccess ? (int)VP_OK : fail(nullptr, VP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    for (void* q : d)
        if (q) hipFree(q);
    return rc;
}

int vp_decode_only(int32_t device_id, const float* heatmaps, int32_t n, int32_t k, const int32_t* org_wh, float* out) {
    return decode_host("vp_decode_only", device_id, heatmaps, (size_t)n * k, n, k, nullptr, 0, nullptr, org_wh, out);
}

int vp_dbg_decode_affine(int32_t device_id, const float* heatmaps, int32_t n, int32_t k, const float* cs, float* out) {
    if (!cs) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    return decode_host("vp_dbg_decode_affine", device_id, heatmaps, (size_t)n * k, n, k, nullptr, 0, nullptr, nullptr, out, 0, cs);
}

// ... under the flip-test mode: the interleaved [2 n, k, 64, 48] batch
int vp_dbg_decode_affine_flip(int32_t device_id, const float* heatmaps2, int32_t n, int32_t k, const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap,
                              const float* cs, float* out) {
    if (k <= 0 || !cs) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    std::vector<int32_t> partner((size_t)k);
    std::string why;
    if (flip_partner_table(k, flip_pairs, n_pairs, partner.data(), &why)) return fail(nullptr, VP_ERR_INVALID, why);
    return decode_host("vp_dbg_decode_affine_flip", device_id, heatmaps2, (size_t)n * k * 2, n, k, partner.data(), shift_heatmap, nullptr, nullptr, out, 0, cs);
}

int vp_dbg_decode_flip(int32_t device_id, const float* heatmaps2, int32_t n, int32_t k, const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap,
                       const int32_t* org_wh, float* out) {
    if (k <= 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    std::vector<int32_t> partner((size_t)k);
    std::string why;
    if (flip_partner_table(k, flip_pairs, n_pairs, partner.data(), &why)) return fail(nullptr, VP_ERR_INVALID, why);
    return decode_host("vp_dbg_decode_flip", device_id, heatmaps2, (size_t)n * k * 2, n, k, partner.data(), shift_heatmap, nullptr, org_wh, out);
}

int vp_dbg_mix_plan(const int32_t* expert_ids, int32_t n, int32_t n_experts, int32_t max_batch, const int32_t* k_per_expert, int32_t* order, int32_t* ids_padded,
                    int32_t* counts, int32_t* records, uint64_t* pattern) {
    if (n < 0 || n_experts <= 0 || max_batch <= 0 || (n > 0 && !expert_ids)) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    std::string why;
    if (mix_check_ids(expert_ids, n, n_experts, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    const int B = (max_batch + 3) / 4 * 4;
    int kmax = 0;
    for (int e = 0; e < n_experts && k_per_expert; ++e) kmax = std::max(kmax, k_per_expert[e]);
    int ci = 0;
    const int rc = for_chunks(n, max_batch, [&](int off, int nb) -> int {   // the entries' own walk
        MixPlan p;
        mix_plan(expert_ids + off, nb, n_experts, p);
        if (order) std::memcpy(order + off, p.order.data(), (size_t)nb * 4);
        if (ids_padded)   // what mix_tables_kernel leaves in the handle's id buffer
            for (int j = 0; j < B; ++j) ids_padded[(size_t)ci * B + j] = p.ids[std::min(j, nb - 1)];
        if (counts) {
            std::memset(counts + (size_t)ci * n_experts, 0, (size_t)n_experts * 4);
            for (size_t s = 0; s < p.seg_e.size(); ++s) counts[(size_t)ci * n_experts + p.seg_e[s]] = p.seg_s[s + 1] - p.seg_s[s];
        }
        if (records && k_per_expert) {
            std::vector<int32_t> first(nb), K(nb);
            mix_records(p, k_per_expert, kmax, first.data(), K.data());
            for (int j = 0; j < nb; ++j) { int32_t* r = records + 3 * (size_t)(off + j); r[0] = first[j]; r[1] = K[j]; r[2] = p.order[j]; }
        }
        if (pattern) pattern[ci] = p.pattern;
        ++ci;
        return VP_OK;
    });
    return rc ? rc : ci;
}

int vp_dbg_decode_mix(int32_t device_id, const float* heatmaps, int32_t n_maps, int32_t n, int32_t kmax, const int32_t* records, const int32_t* org_wh, float* out) {
    if (!heatmaps || !out || !records || n <= 0 || kmax <= 0 || n_maps <= 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int j = 0; j < n; ++j) {   // every record inside the maps and the output, every output row written once
        const int32_t* r = records + 3 * (size_t)j;
        if (r[0] < 0 || r[1] <= 0 || r[1] > kmax || (int64_t)r[0] + r[1] > n_maps || r[2] < 0 || r[2] >= n || seen[r[2]]++)
            return fail(nullptr, VP_ERR_INVALID, "record " + std::to_string(j) + " lies outside the maps or the output, or repeats a row");
    }
    return decode_host("vp_dbg_decode_mix", device_id, heatmaps, (size_t)n_maps, n, kmax, nullptr, 0, records, org_wh, out);
}

int vp_dbg_mix_plan_flip(const int32_t* expert_ids, int32_t n, int32_t n_experts, int32_t max_batch, const int32_t* k_per_expert, int32_t* order, int32_t* row_ids,
                         int32_t* counts, int32_t* records, uint64_t* pattern) {
    if (n < 0 || n_experts <= 0 || max_batch <= 0 || (n > 0 && !expert_ids)) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    if (max_batch < 2) return fail(nullptr, VP_ERR_INVALID, "max_batch < 2: a crop and its mirror image share the forward batch");
    std::string why;
    if (mix_check_ids(expert_ids, n, n_experts, &why)) return fail(nullptr, VP_ERR_INVALID, why);
    const int B = (max_batch + 3) / 4 * 4;
    int kmax = 0;
    for (int e = 0; e < n_experts && k_per_expert; ++e) kmax = std::max(kmax, k_per_expert[e]);
    int ci = 0;
    const int rc = for_chunks(n, max_batch / 2, [&](int off, int nb) -> int {   // the entries' own walk under the mode (chunk_cap)
        MixPlan p;
        mix_plan(expert_ids + off, nb, n_experts, p);
        if (order) std::memcpy(order + off, p.order.data(), (size_t)nb * 4);
        if (row_ids)   // what mix_tables_kernel<true> leaves in the handle's id buffer
            for (int r = 0; r < B; ++r) row_ids[(size_t)ci * B + r] = p.ids[std::min(r >> 1, nb - 1)];
        if (counts) {
            std::memset(counts + (size_t)ci * n_experts, 0, (size_t)n_experts * 4);
            for (size_t s = 0; s < p.seg_e.size(); ++s) counts[(size_t)ci * n_experts + p.seg_e[s]] = p.seg_s[s + 1] - p.seg_s[s];
        }
        if (records && k_per_expert) {
            std::vector<int32_t> first(nb), K(nb);
            mix_records_flip(p, k_per_expert, kmax, first.data(), K.data());
            for (int j = 0; j < nb; ++j) { int32_t* r = records + 4 * (size_t)(off + j); r[0] = first[j]; r[1] = K[j]; r[2] = p.order[j]; r[3] = p.ids[j]; }
        }
        if (pattern) pattern[ci] = p.pattern;
        ++ci;
        return VP_OK;
    });
    return rc ? rc : ci;
}

int vp_dbg_decode_flip_mix(int32_t device_id, const float* heatmaps, int32_t n_maps, int32_t n, int32_t kmax, const int32_t* records4, const int32_t* partners,
                           int32_t n_experts, int32_t shift_heatmap, const int32_t* org_wh, float* out) {
    if (!heatmaps || !out || !records4 || !partners || n <= 0 || kmax <= 0 || n_maps <= 0 || n_experts <= 0) return fail(nullptr, VP_ERR_INVALID, "bad argument");
    for (int i = 0; i < n_experts * kmax; ++i)   // the kernel indexes maps with it
        if (partners[i] < 0 || partners[i] >= kmax) return fail(nullptr, VP_ERR_INVALID, "partner table entry " + std::to_string(i) + " outside [0, kmax)");
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int j = 0; j < n; ++j) {   // every record's 2 K maps inside the maps, its row inside the output and written once, its expert inside the table
        const int32_t* r = records4 + 4 * (size_t)j;
        if (r[0] < 0 || r[1] <= 0 || r[1] > kmax || (int64_t)r[0] + 2 * (int64_t)r[1] > n_maps || r[2] < 0 || r[2] >= n || seen[r[2]]++ || r[3] < 0 || r[3] >= n_experts)
            return fail(nullptr, VP_ERR_INVALID, "record " + std::to_string(j) + " lies outside the maps, the output or the partner table, or repeats a row");
        for (int k = 0; k < r[1]; ++k)   // a mirror joint of this crop must be one of ITS K maps
            if (partners[(size_t)r[3] * kmax + k] >= r[1])
                return fail(nullptr, VP_ERR_INVALID, "record " + std::to_string(j) + ": expert " + std::to_string(r[3]) + "'s partner of joint " + std::to_string(k) + " is outside its " + std::to_string(r[1]) + " joints");
    }
    return decode_host("vp_dbg_decode_flip_mix", device_id, heatmaps, (size_t)n_maps, n, kmax, partners, shift_heatmap, records4, org_wh, out, n_experts);
}

}  // extern "C"
