// The multi-device group of the C ABI (include/vitpose_hip.h, vp_group_*): one process, N devices, one handle per device; crops sharded
// contiguously, weights replicated.
#include "api_internal.h"

using namespace vpi;

extern "C" {

struct vp_group {
    std::vector<vp_ctx*> h;
    int peer_missing = 0;        // ordered device pairs without peer access (their all-gather copies are staged through the host)
    std::vector<float*> d_all;   // per device: [max_total, K, 3] keypoints of EVERY shard (vp_group_infer_allgather)
    size_t all_cap = 0;
    std::string err;
};
namespace { thread_local std::string g_group_error; }

int vp_group_create(vp_group_handle* out, const vp_config* cfg, const int32_t* device_ids, int32_t n_devices) {
    if (!out || !cfg || !device_ids || n_devices <= 0) { g_group_error = "null argument"; return VP_ERR_INVALID; }
    *out = nullptr;
    vp_group* g = new vp_group();
    for (int i = 0; i < n_devices; ++i) {
        vp_config c = *cfg;
        c.device_id = device_ids[i];
        vp_handle h = nullptr;
        int rc = vp_create(&h, &c);
        if (rc) { g_group_error = std::string("device ") + std::to_string(device_ids[i]) + ": " + vp_last_error(nullptr); vp_group_destroy(g); return rc; }
        g->h.push_back(h);
    }
    // peer access for the device-side all-gather (xGMI links are point to point: one copy per pair)
    for (int i = 0; i < n_devices; ++i)
        for (int j = 0; j < n_devices; ++j)
            if (i != j) {
                hipSetDevice(device_ids[i]);
                int can = 0;
                bool ok = false;
                if (hipDeviceCanAccessPeer(&can, device_ids[i], device_ids[j]) == hipSuccess && can) {
                    hipError_t e = hipDeviceEnablePeerAccess(device_ids[j], 0);
                    ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
                }
                if (!ok) { (void)hipGetLastError(); ++g->peer_missing; }   // not fatal: hipMemcpyPeerAsync stages such a pair through the host
            }
    *out = g;
    return VP_OK;
}

int vp_group_size(vp_group_handle g) { return g ? (int)g->h.size() : 0; }
int vp_group_peer_access_missing(vp_group_handle g) { return g ? g->peer_missing : -1; }

int vp_group_load_weights(vp_group_handle g, const vp_tensor_desc* tensors, int32_t n_tensors) {
    if (!g) return VP_ERR_INVALID;
    for (auto* h : g->h) {
        int rc = vp_load_weights(h, tensors, n_tensors);
        if (rc) { g->err = h->err; return rc; }
    }
    return VP_OK;
}

// shard i of n crops over w devices: [off, off + cnt), contiguous, ceil(n / w) per device (the last ones may be short or empty)
static void group_shard(int n, int w, int i, int& off, int& cnt) {
    const int per = (n + w - 1) / w;
    off = per * i < n ? per * i : n;
    cnt = n - off < per ? n - off : per;
}

// the whole plan of a call: rounds of (devices x max_batch) crops, entry e = round * w + device -> [offs[e], offs[e] + cnts[e])
static int group_plan(int n, int w, int maxb, std::vector<int>& offs, std::vector<int>& cnts) {
    offs.clear(); cnts.clear();
    if (n < 0 || w <= 0 || maxb <= 0) return -1;
    const long per_round = (long)w * maxb;
    for (long r0 = 0; r0 < n; r0 += per_round) {
        const int nr = (int)(n - r0 < per_round ? n - r0 : per_round);
        for (int i = 0; i < w; ++i) {
            int off, cnt;
            group_shard(nr, w, i, off, cnt);
            offs.push_back((int)r0 + off);
            cnts.push_back(cnt);
        }
    }
    return (int)offs.size();
}

int vp_dbg_group_plan(int32_t n, int32_t w, int32_t maxb, int32_t* offs, int32_t* cnts, int32_t cap) {
    std::vector<int> o, k;
    const int e = group_plan(n, w, maxb, o, k);
    if (e < 0 || cap < 0 || (cap > 0 && (!offs || !cnts))) return -1;
    for (int i = 0; i < e && i < cap; ++i) { offs[i] = o[i]; cnts[i] = k[i]; }
    return e;
}

// The two-phase schedule of a group call, as ONE function for the real path (group_run) and for the host-only trace
// (vp_dbg_group_trace): per round of `w` plan entries, phase 1 calls submit(member, off, cnt) for EVERY member with work before phase 2
// calls wait(member) for any of them.  submit returns 0 or an error code; on an error every member already submitted in this round
// is waited for (drained) before the error is returned, so no slot of any member stays in flight.
extern "C++" {
template <class Submit, class Wait>
static int group_rounds(const std::vector<int>& offs, const std::vector<int>& cnts, int w, Submit submit, Wait wait) {
    const int entries = (int)offs.size();
    for (int e0 = 0; e0 < entries; e0 += w) {
        std::vector<char> inflight(w, 0);
        auto drain = [&](int from) { for (int i = from; i < w; ++i) if (inflight[i]) { wait(i); inflight[i] = 0; } };
        for (int i = 0; i < w; ++i) {                    // phase 1 -- enqueue on every member; nothing here waits for a device
            if (cnts[e0 + i] <= 0) continue;
            const int rc = submit(i, offs[e0 + i], cnts[e0 + i]);
            if (rc) { drain(0); return rc; }
            inflight[i] = 1;
        }
        for (int i = 0; i < w; ++i)                      // phase 2 -- collect
            if (inflight[i]) {
                inflight[i] = 0;
                const int rc = wait(i);
                if (rc) { drain(i + 1); return rc; }
            }
    }
    return VP_OK;
}
}   // extern "C++"

// host-only: the order in which a call of n crops on w members of max_batch maxb submits (+ (member + 1)) and waits (- (member + 1)),
// with stub members (tests/test_host_logic.py: every submission of a round precedes its first wait)
int vp_dbg_group_trace(int32_t n, int32_t w, int32_t maxb, int32_t* trace, int32_t cap) {
    std::vector<int> offs, cnts;
    if (group_plan(n, w, maxb, offs, cnts) < 0 || cap < 0 || (cap > 0 && !trace)) return -1;
    int len = 0;
    auto put = [&](int v) { if (len < cap) trace[len] = v; ++len; };
    group_rounds(offs, cnts, w, [&](int i, int, int) { put(i + 1); return 0; }, [&](int i) { put(-(i + 1)); return 0; });
    return len;
}

static int group_run(vp_group* g, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out, float* const* d_all) {
    if (!g || n < 0 || (n > 0 && (!crops || (!out && !d_all)))) return VP_ERR_INVALID;
    const int w = (int)g->h.size();
    const int K = g->h[0]->Kp;
    std::vector<float> scratch;
    if (!out) { scratch.resize((size_t)n * K * 3); out = scratch.data(); }
    std::vector<int> offs, cnts;
    for (int i = 1; i < w; ++i)   // one plan for all members: they must agree on the flip-test mode (vp_group_set_flip_test sets them alike)
        if (g->h[i]->flip_on != g->h[0]->flip_on || g->h[i]->flip_ex != g->h[0]->flip_ex || (g->h[0]->flip_on && (g->h[i]->flip_shift != g->h[0]->flip_shift || g->h[i]->flip_pairs != g->h[0]->flip_pairs))) {
            g->err = "the members of the group disagree on the flip-test mode (member " + std::to_string(i) + " against member 0): set it with vp_group_set_flip_test";
            return VP_ERR_STATE;
        }
    if (group_plan(n, w, chunk_cap(g->h[0]), offs, cnts) < 0) return VP_ERR_INVALID;
    std::vector<int> slot(w, -1);
    // phase 1 per member: upload (pinned caller memory as it is, pageable memory through the member's pinned staging buffer), model,
    // decode, download into the member's pinned staging buffer, and the peer copies of the device-side all-gather -- all enqueued, none
    // waited for, so the members compute concurrently.  phase 2: wait for the member's download, copy its slice to the caller's buffer.
    auto submit = [&](int i, int off, int cnt) -> int {
        vp_ctx* c = g->h[i];
        int rc = submit_impl(c, (const char*)crops + (size_t)off * crop_bytes(fmt), fmt, cnt, org_wh ? org_wh + 2 * (size_t)off : nullptr,
                             out + (size_t)off * K * 3, &slot[i], true);
        if (rc) { g->err = c->err; slot[i] = -1; return rc; }
        if (d_all) {   // all-gather on the device side: this shard's keypoints to every device's copy, peer to peer, on the owner's stream
            for (int j = 0; j < w; ++j) {
                hipError_t e = hipMemcpyPeerAsync(d_all[j] + (size_t)off * K * 3, g->h[j]->cfg.device_id, c->slots[slot[i]].kp,
                                                  c->cfg.device_id, (size_t)cnt * K * 12, c->stream);
                if (e != hipSuccess) {
                    g->err = std::string("hipMemcpyPeerAsync: ") + hipGetErrorString(e);
                    vp_infer_wait(c, slot[i]); slot[i] = -1;   // this member is not marked in flight yet: collect it here
                    return VP_ERR_HIP;
                }
            }
        }
        return VP_OK;
    };
    auto wait = [&](int i) -> int {
        int rc = vp_infer_wait(g->h[i], slot[i]);
        slot[i] = -1;
        if (!rc && d_all) rc = vp_synchronize(g->h[i]);
        if (rc) g->err = g->h[i]->err;
        return rc;
    };
    return group_rounds(offs, cnts, w, submit, wait);
}

int vp_group_infer(vp_group_handle g, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* out) {
    if (!out && n > 0) return VP_ERR_INVALID;
    return group_run(g, crops, fmt, n, org_wh, out, nullptr);
}

int vp_group_infer_allgather(vp_group_handle g, const void* crops, int32_t fmt, int32_t n, const int32_t* org_wh, float* const* d_all, float* out) {
    if (!g || !d_all) return VP_ERR_INVALID;
    return group_run(g, crops, fmt, n, org_wh, out, d_all);
}

vp_handle vp_group_member(vp_group_handle g, int32_t i) { return (g && i >= 0 && i < (int)g->h.size()) ? g->h[i] : nullptr; }

int vp_group_set_flip_test(vp_group_handle g, const int32_t* flip_pairs, int32_t n_pairs, int32_t shift_heatmap) {
    if (!g) return VP_ERR_INVALID;
    for (auto* h : g->h) {
        const int rc = vp_set_flip_test(h, flip_pairs, n_pairs, shift_heatmap);
        if (rc) { g->err = h->err; for (auto* q : g->h) vp_clear_flip_test(q); return rc; }   // all or none
    }
    return VP_OK;
}

int vp_group_clear_flip_test(vp_group_handle g) {
    if (!g) return VP_ERR_INVALID;
    for (auto* h : g->h) {
        const int rc = vp_clear_flip_test(h);
        if (rc) { g->err = h->err; return rc; }
    }
    return VP_OK;
}

int vp_group_destroy(vp_group_handle g) {
    if (!g) return VP_OK;
    for (auto* h : g->h) vp_destroy(h);
    delete g;
    return VP_OK;
}

const char* vp_group_last_error(vp_group_handle g) { return g ? g->err.c_str() : g_group_error.c_str(); }

}  // extern "C"
