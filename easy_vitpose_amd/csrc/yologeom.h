// The YOLOv8-detect network as the library runs it (vp_yolo_*, include/vitpose_hip.h "The detector network"), stated once for the kernels of yolo.hip, the
// host taps and the plan the CPU tests walk.
//
//   * the scaling rules and the layer table (yolo_dims): channel and repeat counts of the scales n, s, m, l, x;
//   * the plan (yolo_plan): every launch of a forward with its shapes, channel offsets / strides and buffer ids, and every buffer's extent.  A tensor is a VIEW
//     (buffer, channel offset, channels) of an NHWC buffer whose channel stride is the buffer's channel count: the halves of a C2f's cv1, the Bottleneck outputs,
//     SPPF's pools, the upsampled maps and the layer outputs a later `cat` reads are written straight into the concatenation's buffer, so `cat` and `split` never run;
//   * the address rule (yolo_at) every kernel forms its addresses with;
//   * the load step (yolo_fold): BatchNorm folded in double precision, one rounding to fp16, the [C_out][ky][kx][C_in padded to 8] weight image;
//   * the Detect decode (yolo_dfl, yolo_box, yolo_sigmoid): float32, operation by operation.
//
// Stem: the convolution kernel reads 8-channel groups only, so layer 0 is fed by a small pack pass (YK_PACK) that writes an 8-channel NHWC copy of the caller's
// 3-channel tensor, channels 3..7 zero; model.0's weights get five zero input channels.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vitpose_hip.h"

#if defined(__HIPCC__)
#define YG_HD __host__ __device__ inline
#else
#define YG_HD inline
#endif

namespace vp {

constexpr int YK_PACK = 0, YK_CONV = 1, YK_POOL = 2, YK_UP = 3, YK_DECODE = 4;
constexpr int YOLO_REG = 16;                 // DFL bins per box side
constexpr int YOLO_BOX_CH = 4 * YOLO_REG;    // 64 box logits per anchor
constexpr int YOLO_MAX_SIDE = 1280, YOLO_MAX_IMAGES = 64, YOLO_MAX_NC = 256;
constexpr int YOLO_TILE_N = 32, YOLO_TILE_K = 32;   // the convolution kernel's weight image: rows padded to TILE_N, columns to TILE_K, both with zeros

// ---- the address rule: element (pixel, channel c of the view) of an NHWC buffer with `stride` channels per pixel, the view starting at channel `off`
YG_HD size_t yolo_at(size_t pixel, int stride, int off, int c) { return pixel * (size_t)stride + (size_t)off + (size_t)c; }

// ---- the Detect decode, float32
// the expectation of a 16-bin softmax: m = max z, e_j = expf(z_j - m), sum_j j e_j / sum_j e_j
YG_HD float yolo_dfl(const float* z) {
    float m = z[0];
    for (int j = 1; j < YOLO_REG; ++j) m = z[j] > m ? z[j] : m;
    float num = 0.f, den = 0.f;
    for (int j = 0; j < YOLO_REG; ++j) {
        const float e = expf(z[j] - m);
        den = den + e;
        num = num + (float)j * e;
    }
    return num / den;
}
// one axis of a head row from the two distances of that axis: (centre, size) * stride; a = the anchor coordinate (g + 0.5)
YG_HD void yolo_box_axis(float a, float d_lo, float d_hi, float stride, float* centre, float* size) {
    const float lo = a - d_lo, hi = a + d_hi;
    *centre = (lo + hi) / 2.f * stride;
    *size = (hi - lo) * stride;
}
YG_HD float yolo_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }
YG_HD float yolo_silu(float v) { return v / (1.f + expf(-v)); }

// ---- the decode of one anchor, the same code in the kernel (one thread per unit) and in the host tap
struct DecodeArgs {
    const float* lvl[3];    // [n][h w][64 + nc]
    int h[3], w[3], a0[3];
    int A, nc, units;       // units per anchor: 0 the x axis (left, right -> cx, w), 1 the y axis (top, bottom -> cy, h), 2.. class blocks of DEC_CLS classes
    int layout, n_images;
};
constexpr int DEC_CLS = 32;

template <typename T> YG_HD void yolo_head_put(T* head, int layout, int nc, int A, size_t img, int a, int ch, float v) {
    const size_t C = (size_t)(4 + nc);
    head[layout == 0 ? (img * C + (size_t)ch) * (size_t)A + (size_t)a : (img * (size_t)A + (size_t)a) * C + (size_t)ch] = (T)v;
}

// one unit of one anchor: the same code on the device (one thread per unit) and in the host tap
template <typename T> YG_HD void yolo_decode_unit(const DecodeArgs& d, T* head, size_t img, int a, int unit) {
    const int l = a >= d.a0[2] ? 2 : a >= d.a0[1] ? 1 : 0;
    const int ai = a - d.a0[l], gy = ai / d.w[l], gx = ai - gy * d.w[l];
    const int cs = YOLO_BOX_CH + d.nc;
    const float* z = d.lvl[l] + yolo_at(img * (size_t)(d.h[l] * d.w[l]) + (size_t)ai, cs, 0, 0);
    if (unit < 2) {
        const float stride = (float)(8 << l);
        const float anchor = (float)(unit == 0 ? gx : gy) + 0.5f;
        float lo[YOLO_REG], hi[YOLO_REG];
        for (int j = 0; j < YOLO_REG; ++j) { lo[j] = z[YOLO_REG * unit + j]; hi[j] = z[YOLO_REG * (unit + 2) + j]; }
        float centre, size;
        yolo_box_axis(anchor, yolo_dfl(lo), yolo_dfl(hi), stride, &centre, &size);
        yolo_head_put(head, d.layout, d.nc, d.A, img, a, unit, centre);
        yolo_head_put(head, d.layout, d.nc, d.A, img, a, 2 + unit, size);
    } else {
        const int c0 = (unit - 2) * DEC_CLS, c1 = c0 + DEC_CLS < d.nc ? c0 + DEC_CLS : d.nc;
        for (int c = c0; c < c1; ++c) yolo_head_put(head, d.layout, d.nc, d.A, img, a, 4 + c, yolo_sigmoid(z[YOLO_BOX_CH + c]));
    }
}

// ---- everything below is the host's: the plan and the load step

inline int yolo_pad8(int c) { return (c + 7) & ~7; }
inline int yolo_pad_to(int v, int m) { return (v + m - 1) / m * m; }

struct YoloDims {
    char scale = '?';
    int ch64 = 0, ch128 = 0, ch256 = 0, ch512 = 0, ch1024 = 0;
    int d3 = 0, d6 = 0;        // d(3), d(6)
    int nc = 0, c2d = 0, c3d = 0;   // Detect's branch widths
};

// chX = 8 ceil(min(X, max_ch) width / 8), d(n) = max(round(n depth), 1)
inline bool yolo_dims(char scale, int nc, YoloDims* out) {
    double depth, width;
    int max_ch;
    switch (scale) {
        case 'n': depth = 0.33; width = 0.25; max_ch = 1024; break;
        case 's': depth = 0.33; width = 0.50; max_ch = 1024; break;
        case 'm': depth = 0.67; width = 0.75; max_ch = 768; break;
        case 'l': depth = 1.0; width = 1.0; max_ch = 512; break;
        case 'x': depth = 1.0; width = 1.25; max_ch = 512; break;
        default: return false;
    }
    auto ch = [&](int x) { return 8 * (int)std::ceil((x < max_ch ? x : max_ch) * width / 8.0); };
    auto d = [&](int n) { const int r = (int)std::nearbyint(n * depth); return r > 1 ? r : 1; };
    YoloDims o;
    o.scale = scale;
    o.ch64 = ch(64); o.ch128 = ch(128); o.ch256 = ch(256); o.ch512 = ch(512); o.ch1024 = ch(1024);
    o.d3 = d(3); o.d6 = d(6);
    o.nc = nc;
    o.c2d = std::max(16, std::max(o.ch256 / 4, YOLO_BOX_CH));
    o.c3d = std::max(o.ch256, std::min(nc, 100));
    *out = o;
    return true;
}

// one convolution of the network: where its tensors are in the checkpoint and in the weight arena
struct YoloConv {
    std::string key;      // "model.0", "model.2.m.0.cv1", "model.22.cv2.0.2" ...
    bool module = true;   // Conv module (conv + BatchNorm + SiLU; or fused conv.weight + conv.bias) against a plain Conv2d with bias
    int c1 = 0, c2 = 0, k = 1, s = 1;   // the checkpoint's shape [c2, c1, k, k]
    int c1p = 0, c2w = 0;               // input channels read (c1 padded to 8), output channels written (c2 padded to 8 for fp16 outputs, c2 for float32 ones)
    int cols = 0, cols_pad = 0, rows_pad = 0;   // cols = k k c1p; the device image is [rows_pad][cols_pad]
    size_t w_off = 0, b_off = 0;        // element offsets into the fp16 weight arena and the float32 bias arena
};

struct YoloView { int buf = -1, off = 0, c = 0, h = 0, w = 0; };

struct YoloPlan {
    YoloDims d;
    int in_h = 0, in_w = 0, A = 0;
    int level_h[3] = {0, 0, 0}, level_w[3] = {0, 0, 0}, level_a0[3] = {0, 0, 0};
    std::vector<YoloConv> convs;
    std::vector<vp_yolo_launch> launches;
    std::vector<vp_yolo_buffer> bufs;   // 0 = the caller's input, the last one = the caller's head
    size_t w_elems = 0, b_elems = 0;

    int buf(int h, int w, int c, int eb) {
        bufs.push_back(vp_yolo_buffer{h, w, c, eb});
        return (int)bufs.size() - 1;
    }
    YoloView whole(int b) const { return YoloView{b, 0, bufs[b].c, bufs[b].h, bufs[b].w}; }
    YoloView slice(int b, int off, int c) const { return YoloView{b, off, c, bufs[b].h, bufs[b].w}; }
    YoloView fresh(int h, int w, int c) { return whole(buf(h, w, c, 2)); }

    vp_yolo_launch blank(int kind, int layer) const {
        vp_yolo_launch l;
        std::memset(&l, 0, sizeof(l));
        l.kind = kind; l.layer = layer; l.conv = -1; l.res_buf = -1; l.k = 1; l.s = 1;
        return l;
    }
    void io(vp_yolo_launch& l, const YoloView& in, const YoloView& out) const {
        l.h_in = in.h; l.w_in = in.w; l.h_out = out.h; l.w_out = out.w;
        l.in_buf = in.buf; l.in_off = in.off; l.in_stride = bufs[in.buf].c;
        l.out_buf = out.buf; l.out_off = out.off; l.out_stride = bufs[out.buf].c;
    }
    // c1 / c2: the checkpoint's channel counts; in.c = c1 padded to 8; out.c = the channels written
    void conv(int layer, const std::string& key, bool module, int c1, int c2, int k, int s, const YoloView& in, const YoloView& out, const YoloView* res = nullptr) {
        YoloConv cv;
        cv.key = key; cv.module = module; cv.c1 = c1; cv.c2 = c2; cv.k = k; cv.s = s;
        cv.c1p = in.c; cv.c2w = out.c;
        cv.cols = k * k * cv.c1p;
        cv.cols_pad = yolo_pad_to(cv.cols, YOLO_TILE_K);
        cv.rows_pad = yolo_pad_to(cv.c2w, YOLO_TILE_N);
        cv.w_off = w_elems; cv.b_off = b_elems;
        w_elems += (size_t)cv.rows_pad * cv.cols_pad;
        b_elems += (size_t)cv.rows_pad;
        vp_yolo_launch l = blank(YK_CONV, layer);
        l.conv = (int)convs.size();
        l.k = k; l.s = s; l.act = module ? 1 : 0; l.f32_out = bufs[out.buf].elem_bytes == 4;
        l.c_in = cv.c1p; l.c_out = cv.c2w;
        io(l, in, out);
        if (res) { l.res_buf = res->buf; l.res_off = res->off; l.res_stride = bufs[res->buf].c; }
        convs.push_back(cv);
        launches.push_back(l);
    }
    void c2f(int layer, const YoloView& in, int c2, int n, bool shortcut, const YoloView& out) {
        const std::string key = "model." + std::to_string(layer);
        const int c = c2 / 2;
        const int cat = buf(in.h, in.w, (2 + n) * c, 2);
        conv(layer, key + ".cv1", true, in.c, 2 * c, 1, 1, in, slice(cat, 0, 2 * c));
        for (int j = 0; j < n; ++j) {
            const YoloView y = slice(cat, (1 + j) * c, c), z = slice(cat, (2 + j) * c, c);
            const std::string m = key + ".m." + std::to_string(j);
            const int tmp = buf(in.h, in.w, c, 2);   // one per Bottleneck: no buffer is written twice in a forward, so the activation tap sees every launch
            conv(layer, m + ".cv1", true, c, c, 3, 1, y, whole(tmp));
            conv(layer, m + ".cv2", true, c, c, 3, 1, whole(tmp), z, shortcut ? &y : nullptr);
        }
        conv(layer, key + ".cv2", true, (2 + n) * c, c2, 1, 1, whole(cat), out);
    }
    void pool(int layer, const YoloView& in, const YoloView& out) {
        vp_yolo_launch l = blank(YK_POOL, layer);
        l.k = 5; l.c_in = in.c; l.c_out = out.c;
        io(l, in, out);
        launches.push_back(l);
    }
    void up(int layer, const YoloView& in, const YoloView& out) {
        vp_yolo_launch l = blank(YK_UP, layer);
        l.c_in = in.c; l.c_out = out.c;
        io(l, in, out);
        launches.push_back(l);
    }
};

// The plan of a network of dims d at in_h x in_w.  input_layout / head_dtype / head_layout only shape the two external buffers.
inline void yolo_plan(const YoloDims& d, int in_h, int in_w, int head_dtype, YoloPlan* out) {
    YoloPlan p;
    p.d = d; p.in_h = in_h; p.in_w = in_w;
    const int H = in_h, W = in_w;
    const int in = p.buf(H, W, 3, 2);
    const YoloView pk = p.fresh(H, W, 8);
    {
        vp_yolo_launch l = p.blank(YK_PACK, -1);
        l.c_in = 3; l.c_out = 8;
        p.io(l, p.whole(in), pk);
        p.launches.push_back(l);
    }
    // the concatenations 11, 14, 17, 20 and the three Detect inputs' float32 outputs exist before their producers
    const int cat11 = p.buf(H / 16, W / 16, d.ch1024 + d.ch512, 2), cat14 = p.buf(H / 8, W / 8, d.ch512 + d.ch256, 2);
    const int cat17 = p.buf(H / 16, W / 16, d.ch256 + d.ch512, 2), cat20 = p.buf(H / 32, W / 32, d.ch512 + d.ch1024, 2);
    int lvl[3];
    for (int i = 0; i < 3; ++i) lvl[i] = p.buf(H >> (3 + i), W >> (3 + i), YOLO_BOX_CH + d.nc, 4);
    const YoloView t0 = p.fresh(H / 2, W / 2, d.ch64);
    p.conv(0, "model.0", true, 3, d.ch64, 3, 2, pk, t0);
    const YoloView t1 = p.fresh(H / 4, W / 4, d.ch128);
    p.conv(1, "model.1", true, d.ch64, d.ch128, 3, 2, t0, t1);
    const YoloView t2 = p.fresh(H / 4, W / 4, d.ch128);
    p.c2f(2, t1, d.ch128, d.d3, true, t2);
    const YoloView t3 = p.fresh(H / 8, W / 8, d.ch256);
    p.conv(3, "model.3", true, d.ch128, d.ch256, 3, 2, t2, t3);
    const YoloView t4 = p.slice(cat14, d.ch512, d.ch256);
    p.c2f(4, t3, d.ch256, d.d6, true, t4);
    const YoloView t5 = p.fresh(H / 16, W / 16, d.ch512);
    p.conv(5, "model.5", true, d.ch256, d.ch512, 3, 2, t4, t5);
    const YoloView t6 = p.slice(cat11, d.ch1024, d.ch512);
    p.c2f(6, t5, d.ch512, d.d6, true, t6);
    const YoloView t7 = p.fresh(H / 32, W / 32, d.ch1024);
    p.conv(7, "model.7", true, d.ch512, d.ch1024, 3, 2, t6, t7);
    const YoloView t8 = p.fresh(H / 32, W / 32, d.ch1024);
    p.c2f(8, t7, d.ch1024, d.d3, true, t8);
    const YoloView t9 = p.slice(cat20, d.ch512, d.ch1024);
    {
        const int c_ = d.ch1024 / 2;
        const int cat = p.buf(H / 32, W / 32, 4 * c_, 2);
        p.conv(9, "model.9.cv1", true, d.ch1024, c_, 1, 1, t8, p.slice(cat, 0, c_));
        for (int j = 0; j < 3; ++j) p.pool(9, p.slice(cat, j * c_, c_), p.slice(cat, (j + 1) * c_, c_));
        p.conv(9, "model.9.cv2", true, 4 * c_, d.ch1024, 1, 1, p.whole(cat), t9);
    }
    p.up(10, t9, p.slice(cat11, 0, d.ch1024));
    const YoloView t12 = p.slice(cat17, d.ch256, d.ch512);
    p.c2f(12, p.whole(cat11), d.ch512, d.d3, false, t12);
    p.up(13, t12, p.slice(cat14, 0, d.ch512));
    const YoloView t15 = p.fresh(H / 8, W / 8, d.ch256);
    p.c2f(15, p.whole(cat14), d.ch256, d.d3, false, t15);
    p.conv(16, "model.16", true, d.ch256, d.ch256, 3, 2, t15, p.slice(cat17, 0, d.ch256));
    const YoloView t18 = p.fresh(H / 16, W / 16, d.ch512);
    p.c2f(18, p.whole(cat17), d.ch512, d.d3, false, t18);
    p.conv(19, "model.19", true, d.ch512, d.ch512, 3, 2, t18, p.slice(cat20, 0, d.ch512));
    const YoloView t21 = p.fresh(H / 32, W / 32, d.ch1024);
    p.c2f(21, p.whole(cat20), d.ch1024, d.d3, false, t21);
    const YoloView x[3] = {t15, t18, t21};
    const int c3p = yolo_pad8(d.c3d);
    int a0 = 0;
    for (int i = 0; i < 3; ++i) {
        const std::string li = std::to_string(i);
        const YoloView b1 = p.fresh(x[i].h, x[i].w, d.c2d), b2 = p.fresh(x[i].h, x[i].w, d.c2d);
        p.conv(22, "model.22.cv2." + li + ".0", true, x[i].c, d.c2d, 3, 1, x[i], b1);
        p.conv(22, "model.22.cv2." + li + ".1", true, d.c2d, d.c2d, 3, 1, b1, b2);
        p.conv(22, "model.22.cv2." + li + ".2", false, d.c2d, YOLO_BOX_CH, 1, 1, b2, p.slice(lvl[i], 0, YOLO_BOX_CH));
        const YoloView s1 = p.fresh(x[i].h, x[i].w, c3p), s2 = p.fresh(x[i].h, x[i].w, c3p);
        p.conv(22, "model.22.cv3." + li + ".0", true, x[i].c, d.c3d, 3, 1, x[i], s1);
        p.conv(22, "model.22.cv3." + li + ".1", true, d.c3d, d.c3d, 3, 1, s1, s2);
        p.conv(22, "model.22.cv3." + li + ".2", false, d.c3d, d.nc, 1, 1, s2, p.slice(lvl[i], YOLO_BOX_CH, d.nc));
        p.level_h[i] = x[i].h; p.level_w[i] = x[i].w; p.level_a0[i] = a0;
        a0 += x[i].h * x[i].w;
    }
    p.A = a0;
    const int head = p.buf(1, p.A, 4 + d.nc, head_dtype == VP_DET_F16 ? 2 : 4);
    {
        vp_yolo_launch l = p.blank(YK_DECODE, 22);
        l.c_in = YOLO_BOX_CH + d.nc; l.c_out = 4 + d.nc;
        l.h_in = p.level_h[0]; l.w_in = p.level_w[0]; l.h_out = 1; l.w_out = p.A;
        l.in_buf = lvl[0]; l.in_off = 0; l.in_stride = YOLO_BOX_CH + d.nc;   // the three level buffers are lvl[0], lvl[0] + 1, lvl[0] + 2
        l.out_buf = head; l.out_off = 0; l.out_stride = 4 + d.nc;
        l.f32_out = head_dtype != VP_DET_F16;
        p.launches.push_back(l);
    }
    *out = std::move(p);
}

// ---- the checkpoint
struct YoloTensors {
    std::unordered_map<std::string, const vp_yolo_tensor*> map;
    const vp_yolo_tensor* find(const std::string& name) const {
        auto it = map.find(name);
        return it == map.end() ? nullptr : it->second;
    }
};

inline bool yolo_shape_is(const vp_yolo_tensor* t, int n0, int n1 = -1, int n2 = -1, int n3 = -1) {
    const int want[4] = {n0, n1, n2, n3};
    int nd = 0;
    int64_t numel = 1;
    while (nd < 4 && want[nd] >= 0) { numel *= want[nd]; ++nd; }
    if (t->ndim != nd || t->numel != numel || !t->data) return false;
    for (int i = 0; i < nd; ++i)
        if (t->shape[i] != want[i]) return false;
    return true;
}

inline std::string yolo_shape_str(const vp_yolo_tensor* t) {
    std::string s = "[";
    for (int i = 0; i < t->ndim && i < 4; ++i) s += (i ? ", " : "") + std::to_string(t->shape[i]);
    return s + "]";
}

// Scale, repeat counts and nc read from the checkpoint, checked against the table.  Returns "" or the reason of the refusal.
inline std::string yolo_read_dims(const vp_yolo_tensor* tensors, int n_tensors, YoloTensors* tab, YoloDims* d) {
    if (!tensors || n_tensors < 1) return "no tensors";
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name) return "tensor " + std::to_string(i) + " has no name";
        if (tensors[i].ndim < 0 || tensors[i].ndim > 4) return std::string("tensor ") + tensors[i].name + ": ndim outside 0..4";
        tab->map[tensors[i].name] = &tensors[i];
    }
    const vp_yolo_tensor* w0 = tab->find("model.0.conv.weight");
    if (!w0) return "missing tensor model.0.conv.weight";
    if (w0->ndim != 4 || w0->shape[1] != 3 || w0->shape[2] != 3 || w0->shape[3] != 3) return "model.0.conv.weight: shape " + yolo_shape_str(w0) + " is not [ch64, 3, 3, 3]";
    char scale = '?';
    for (char s : {'n', 's', 'm', 'l', 'x'}) {
        YoloDims t;
        yolo_dims(s, 1, &t);
        if (t.ch64 == w0->shape[0]) scale = s;
    }
    if (scale == '?') return "model.0.conv.weight: " + std::to_string(w0->shape[0]) + " rows are the width of no YOLOv8 scale (16 n, 32 s, 48 m, 64 l, 80 x)";
    const vp_yolo_tensor* wc = tab->find("model.22.cv3.0.2.weight");
    if (!wc) return "missing tensor model.22.cv3.0.2.weight";
    if (wc->ndim < 1) return "model.22.cv3.0.2.weight: shape " + yolo_shape_str(wc) + " has no rows";
    const int nc = wc->shape[0];
    if (nc < 1 || nc > YOLO_MAX_NC) return "nc = " + std::to_string(nc) + " outside 1.." + std::to_string(YOLO_MAX_NC);
    yolo_dims(scale, nc, d);
    // each repeat count from the highest model.{i}.m.{j} present
    const int layers[8] = {2, 4, 6, 8, 12, 15, 18, 21};
    const int want[8] = {d->d3, d->d6, d->d6, d->d3, d->d3, d->d3, d->d3, d->d3};
    for (int q = 0; q < 8; ++q) {
        int n = 0;
        const std::string pre = "model." + std::to_string(layers[q]) + ".m.";
        while (n < 64 && tab->find(pre + std::to_string(n) + ".cv1.conv.weight")) ++n;
        if (n != want[q])
            return "model." + std::to_string(layers[q]) + ": " + std::to_string(n) + " Bottlenecks in the checkpoint, scale " + std::string(1, scale) + " has " + std::to_string(want[q]);
    }
    const vp_yolo_tensor* dfl = tab->find("model.22.dfl.conv.weight");
    if (dfl) {
        bool ok = dfl->numel == YOLO_REG && dfl->data;
        for (int j = 0; ok && j < YOLO_REG; ++j) ok = dfl->data[j] == (float)j;
        if (!ok) return "model.22.dfl.conv.weight is not 0..15";
    }
    return "";
}

// fp64 -> binary16 bits, one rounding to nearest even
inline uint16_t yolo_f16_bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    const uint16_t sign = (uint16_t)((u >> 48) & 0x8000u);
    const double a = std::fabs(v);
    if (!(a == a)) return (uint16_t)(sign | 0x7e00u);
    if (a >= 65520.0) return (uint16_t)(sign | 0x7c00u);
    if (a == 0.0) return sign;
    int e;
    (void)std::frexp(a, &e);
    int E = e - 1;
    if (E < -14) E = -14;
    double r = std::nearbyint(std::ldexp(a, 10 - E));   // a / 2^(E - 10): exact, then to nearest even
    if (E == -14 && r < 1024.0) return (uint16_t)(sign | (uint16_t)r);
    if (r == 2048.0) { r = 1024.0; ++E; }
    return (uint16_t)(sign | ((uint32_t)(E + 15) << 10) | ((uint32_t)r - 1024u));
}

// The load step of one convolution: w [c2w][ky][kx][c1p] fp16 bits (row stride `ld`), b [c2w] float32; rows and input channels beyond the checkpoint's are zero.
// scale = gamma / sqrt(var + 1e-3), w' = w scale, b' = beta - mean scale, all in double.  Returns "" or the reason of the refusal.
inline std::string yolo_fold(const YoloTensors& tab, const YoloConv& cv, uint16_t* w, size_t ld, float* b) {
    const std::string wk = cv.key + (cv.module ? ".conv.weight" : ".weight");
    const vp_yolo_tensor* tw = tab.find(wk);
    if (!tw) return "missing tensor " + wk;
    if (!yolo_shape_is(tw, cv.c2, cv.c1, cv.k, cv.k))
        return wk + ": shape " + yolo_shape_str(tw) + " contradicts [" + std::to_string(cv.c2) + ", " + std::to_string(cv.c1) + ", " + std::to_string(cv.k) + ", " + std::to_string(cv.k) + "]";
    const vp_yolo_tensor *g = nullptr, *be = nullptr, *mu = nullptr, *var = nullptr, *bias = nullptr;
    auto vec = [&](const std::string& name, const vp_yolo_tensor** t) -> std::string {
        *t = tab.find(name);
        if (!*t) return "missing tensor " + name;
        if (!yolo_shape_is(*t, cv.c2)) return name + ": shape " + yolo_shape_str(*t) + " contradicts [" + std::to_string(cv.c2) + "]";
        return "";
    };
    std::string why;
    if (!cv.module) {
        if (!(why = vec(cv.key + ".bias", &bias)).empty()) return why;
    } else if (tab.find(cv.key + ".bn.weight") || !tab.find(cv.key + ".conv.bias")) {
        if (!(why = vec(cv.key + ".bn.weight", &g)).empty()) return why;
        if (!(why = vec(cv.key + ".bn.bias", &be)).empty()) return why;
        if (!(why = vec(cv.key + ".bn.running_mean", &mu)).empty()) return why;
        if (!(why = vec(cv.key + ".bn.running_var", &var)).empty()) return why;
    } else {
        if (!(why = vec(cv.key + ".conv.bias", &bias)).empty()) return why;
    }
    for (int o = 0; o < cv.c2w; ++o) {
        uint16_t* row = w + (size_t)o * ld;
        std::memset(row, 0, sizeof(uint16_t) * (size_t)cv.cols);
        if (o >= cv.c2) { b[o] = 0.f; continue; }
        double scale = 1.0;
        if (g) {
            scale = (double)g->data[o] / std::sqrt((double)var->data[o] + 1e-3);
            b[o] = (float)((double)be->data[o] - (double)mu->data[o] * scale);
        } else {
            b[o] = bias->data[o];
        }
        for (int c = 0; c < cv.c1; ++c)
            for (int ky = 0; ky < cv.k; ++ky)
                for (int kx = 0; kx < cv.k; ++kx) {
                    const double v = (double)tw->data[(((size_t)o * cv.c1 + c) * cv.k + ky) * cv.k + kx] * scale;
                    row[((size_t)ky * cv.k + kx) * cv.c1p + c] = yolo_f16_bits(v);
                }
    }
    return "";
}

}  // namespace vp
