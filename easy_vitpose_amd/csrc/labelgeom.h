// The label stage of vp_draw_labels_stream (include/vitpose_hip.h), for ONE value each: the gates of a row, the text of a tag, the font, the integer geometry of a
// tag, the draw order and the colours.  Shared by the device kernels (label.hip) and the host-only taps vp_dbg_draw_labels_host / vp_dbg_label_text /
// vp_dbg_label_glyph, so that the CPU tests of the taps pin the arithmetic the device runs, as drawgeom.h does for the skeleton overlay (whose helpers this header
// reuses: draw_usable, draw_mod, draw_pack_color).  easy_vitpose_amd/draw.py restates it in numpy, tests/label_model.py in plain scalar loops.
//
// Modelled on the reference's draw_bboxes (vit_utils/inference.py:19-38): `#<id>: <score>` on a filled tag at the top-left corner of every tracked box, opaque
// colours, no anti-aliasing.  The font is this project's own 5 x 7 bitmap font: parity against OpenCV's Hershey font (FONT_HERSHEY_SIMPLEX) is UNPINNED and not
// claimed, neither for the glyphs nor for the size of a tag.
//
// A row is one person: a box (x1, y1, x2, y2) float32 in frame pixels, a frame index, optionally a rank (rank < 0: no tag), an id (absent: the row's index in the
// call) and a score.
//   gates     the frame index lies in the table, rank >= 0 when given, the four box values pass draw_usable (-16384 < v < 16384, false for NaN: an absent tracker
//             row -- NaN box, id -1 -- draws nothing); the corners are truncated toward zero and then ordered, as draw_primitive does: (x1, y1) = the smaller ones.
//   text      `#<id>` or `#<id>: <score>` over the 16 symbols below (4-bit codes).  The id is the int32 in decimal, '-' for negative values.  The score is printed
//             iff scores are given, show_score is set and -1000 < s < 1000 (false for NaN); its text equals Python's format(float(s), '.2f') for every such
//             float32: the sign is the sign bit (-0.0 prints -0.00), and |s| = M 2^-sh exactly (M the 24-bit significand, sh >= 14) is rounded to q hundredths
//             half-to-even in integers: v = 100 M < 2^31, q = v >> sh, r = v - (q << sh), q += (r > 2^(sh-1)) or (r == 2^(sh-1) and q odd); sh > 32 gives q = 0.
//             q <= 100000 (the largest float below 1000 prints 1000.00).  At most 22 characters: #-2147483648: -1000.00.
//   font      glyph g, bit 5 * row + col (row 0 the top one, col 0 the left one) set = ink; 5 x 7 ink in a cell of advance 6.
//   geometry  all int32.  Scale s = cfg scale in 1..8, 0 for max(1, min(h, w) / 400) of the row's frame capped at 8.  With L characters the tag is the block
//             [x1, x1 + s (6 L + 1)) x [by, by + 9 s), by = y1 - 9 s when that is >= 0, else by = y1 (the tag inside the box; the reference's `y1 > 20` rule).
//             Glyph c has its origin at (gx, gy) = (x1 + s + 6 s c, by + s); a pixel is INK iff it lies in a glyph's 5 s x 7 s cell and the glyph's bit at
//             ((py - gy) / s, (px - gx) / s) is set, otherwise inside the block it is BACKGROUND.  The block is clipped to the frame; it is never shifted.
//             |x1|, |y1| <= 16383 and s (6 L + 1) <= 8 * 133 = 1064: every value stays below 2^15 in magnitude before the clip.
//   colours   background = colors[id mod n_colors] (draw_mod, the mathematical mod); ink = an explicit RGB colour, or automatic: black when
//             77 R + 150 G + 29 B >= 32768 for the background, white otherwise.  Both packed once per row by draw_pack_color (BGR order, or Y, U, V).
//   order     the order index of a pixel's covering primitive is 2 * row + (ink ? 1 : 0); a pixel shows the covering primitive with the HIGHEST order index, whatever
//             the launch shape.  NV12: Y per covered pixel; a chroma sample takes the (U, V) of the highest order index among its up-to-four pixels.
//   writing   no byte outside a covered pixel or chroma sample is written, pitch padding included; every written byte is written once per call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drawgeom.h"

namespace vp {

constexpr int LABEL_MAX_ROWS = 8192;    // VP_LABEL_MAX_ROWS
constexpr int LABEL_MAX_SCALE = 8;
constexpr int LABEL_MAX_TEXT = 22;      // characters of a tag; a record holds 24
constexpr int LABEL_CODES = 12;         // bytes of 4-bit codes in a record
constexpr int LABEL_GLYPHS = 16;

// the alphabet: '#', '0'..'9', ':', '.', '-', ' ' and one spare (a hollow box, never produced by label_format)
enum LabelCode { LBL_HASH = 0, LBL_0 = 1, LBL_COLON = 11, LBL_DOT = 12, LBL_MINUS = 13, LBL_SPACE = 14, LBL_SPARE = 15 };

// the font, bit 5 * row + col per glyph; a function (not a table) so that host and device read the same literals.  The kernels take the 16 words by argument.
__host__ __device__ inline uint64_t label_glyph(int code) {
    switch (code) {
        case 0: return 0x295f57d4aull;    // #
        case 1: return 0x3a33ae62eull;    // 0
        case 2: return 0x3884210c4ull;    // 1
        case 3: return 0x7c444422eull;    // 2
        case 4: return 0x3a304111full;    // 3
        case 5: return 0x211f4a988ull;    // 4
        case 6: return 0x3a3083c3full;    // 5
        case 7: return 0x3a317844cull;    // 6
        case 8: return 0x08422221full;    // 7
        case 9: return 0x3a317462eull;    // 8
        case 10: return 0x1910f462eull;   // 9
        case 11: return 0x008401080ull;   // :
        case 12: return 0x18c000000ull;   // .
        case 13: return 0x0000f8000ull;   // -
        case 14: return 0x000000000ull;   // space
        case 15: return 0x7e318c63full;   // spare
    }
    return 0;
}

// the style of a call, by kernel argument (no host-to-device copy): 4 * 4 + 96 + 4 + 4 + 128 bytes
struct LabelStyle {
    int32_t scale, n_colors, auto_ink, show_score;
    uint8_t colors[DRAW_MAX_COLORS * 3];   // RGB
    uint8_t ink[4];                        // RGB, one byte of padding
    int32_t pad;
    uint64_t font[LABEL_GLYPHS];
};

// One tag as the raster pass reads it (40 bytes).  x0 > x1 marks an empty record.
struct LabelRec {
    int16_t x0, y0, x1, y1;        // inclusive bounding box of the block, clipped to the frame
    int32_t frame;
    int16_t ox, oy;                // the block's origin (x1, by), unclipped
    uint8_t scale, len;
    uint16_t pad;
    uint32_t c0, c1, c2;           // LABEL_CODES bytes of 4-bit codes, character c in word c / 8 at bit 4 * (c % 8): named words, so that a lane's c indexes no array
    int32_t bg, ink;               // the three bytes as the plane holds them (or Y, U, V), byte 0 lowest
};

__host__ __device__ inline int label_scale(int scale, int h, int w) {
    if (scale > 0) return scale;
    int s = (h < w ? h : w) / 400;
    if (s < 1) s = 1;
    return s > LABEL_MAX_SCALE ? LABEL_MAX_SCALE : s;
}

// hundredths of |s| rounded half-to-even on the exact binary value, for a float32 with |s| < 1000 given by its bits (integers only)
__host__ __device__ inline int32_t label_hundredths(uint32_t bits) {
    const int e = (int)((bits >> 23) & 0xff);
    const int64_t M = e ? (int64_t)((bits & 0x7fffffu) | 0x800000u) : (int64_t)(bits & 0x7fffffu);
    const int sh = e ? 150 - e : 149;   // |s| = M 2^-sh; |s| < 1000 < 2^10: e <= 136, sh >= 14
    const int64_t v = 100 * M;          // < 2^31
    if (sh > 32) return 0;              // v < 2^31 <= 2^(sh - 1) / 2: below the half
    const int64_t q = v >> sh, r = v - (q << sh), half = (int64_t)1 << (sh - 1);
    return (int32_t)(q + ((r > half || (r == half && (q & 1))) ? 1 : 0));
}

// the text of a tag as symbol codes, one per byte of out[24]; returns its length L <= 22
__host__ __device__ inline int label_format(int32_t id, bool has_score, float score, uint8_t* out) {
    int L = 0;
    out[L++] = LBL_HASH;
    int64_t a = id;
    if (a < 0) { out[L++] = LBL_MINUS; a = -a; }
    uint8_t d[10];
    int nd = 0;
    do { d[nd++] = (uint8_t)(a % 10); a /= 10; } while (a);
    while (nd) out[L++] = (uint8_t)(LBL_0 + d[--nd]);
    if (!has_score || !(score > -1000.f && score < 1000.f)) return L;
    uint32_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
    bits = __float_as_uint(score);
#else
    { union { float f; uint32_t u; } pun; pun.f = score; bits = pun.u; }
#endif
    int32_t q = label_hundredths(bits);
    out[L++] = LBL_COLON;
    out[L++] = LBL_SPACE;
    if (bits >> 31) out[L++] = LBL_MINUS;
    int32_t ip = q / 100;
    const int32_t fp = q - 100 * ip;
    do { d[nd++] = (uint8_t)(ip % 10); ip /= 10; } while (ip);
    while (nd) out[L++] = (uint8_t)(LBL_0 + d[--nd]);
    out[L++] = LBL_DOT;
    out[L++] = (uint8_t)(LBL_0 + fp / 10);
    out[L++] = (uint8_t)(LBL_0 + fp % 10);
    return L;
}

// What one row needs from the call.  h, w, format, matrix: the row's frame (the caller has checked the frame index and the rank).
struct LabelRow {
    const float* box;       // 4 values
    int32_t id, has_score;
    float score;
    int32_t frame, h, w, format, matrix;
};

// the record of a row; the box gate lives here: a row that is not drawn comes back with x0 > x1
__host__ __device__ inline void label_record(const LabelRow& r, const LabelStyle& st, LabelRec* rec) {
    *rec = LabelRec{1, 1, 0, 0, r.frame, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = 0; q < 4; ++q)
        if (!draw_usable(r.box[q])) return;
    const int xa = (int)r.box[0], ya = (int)r.box[1], xb = (int)r.box[2], yb = (int)r.box[3];
    const int x1 = xa < xb ? xa : xb, y1 = ya < yb ? ya : yb;
    uint8_t text[24];
    const int L = label_format(r.id, r.has_score && st.show_score, r.score, text);
    const int s = label_scale(st.scale, r.h, r.w);
    const int by = y1 - 9 * s >= 0 ? y1 - 9 * s : y1;
    int x0 = x1, y0 = by, xe = x1 + s * (6 * L + 1) - 1, ye = by + 9 * s - 1;
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (xe > r.w - 1) xe = r.w - 1;
    if (ye > r.h - 1) ye = r.h - 1;
    if (x0 > xe || y0 > ye) return;   // nothing of it on the frame
    rec->x0 = (int16_t)x0; rec->y0 = (int16_t)y0; rec->x1 = (int16_t)xe; rec->y1 = (int16_t)ye;
    rec->ox = (int16_t)x1; rec->oy = (int16_t)by;
    rec->scale = (uint8_t)s; rec->len = (uint8_t)L;
    for (int c = 0; c < L; ++c) {
        const uint32_t bits = (uint32_t)text[c] << (4 * (c & 7));
        if (c < 8) rec->c0 |= bits; else if (c < 16) rec->c1 |= bits; else rec->c2 |= bits;
    }
    const uint8_t* bg = st.colors + 3 * draw_mod(r.id, st.n_colors);
    uint8_t ink[3] = {st.ink[0], st.ink[1], st.ink[2]};
    if (st.auto_ink) ink[0] = ink[1] = ink[2] = (77 * bg[0] + 150 * bg[1] + 29 * bg[2] >= 32768) ? 0 : 255;
    rec->bg = draw_pack_color(bg, r.format, r.matrix);
    rec->ink = draw_pack_color(ink, r.format, r.matrix);
}

__host__ __device__ inline bool label_in_block(const LabelRec& r, int px, int py) { return px >= r.x0 && px <= r.x1 && py >= r.y0 && py <= r.y1; }

// 0: the pixel is outside the record's block; 1: background; 2: ink.  font: the 16 glyph words
__host__ __device__ inline int label_cover(const LabelRec& r, const uint64_t* font, int px, int py) {
    if (!label_in_block(r, px, py)) return 0;
    const int s = r.scale, gx = px - r.ox - s, gy = py - r.oy - s;
    if (gx < 0 || gy < 0 || gy >= 7 * s) return 1;
    const int c = gx / (6 * s);
    if (c >= r.len) return 1;
    const int col = (gx - 6 * s * c) / s;
    if (col >= 5) return 1;
    const int code = ((c < 8 ? r.c0 : (c < 16 ? r.c1 : r.c2)) >> (4 * (c & 7))) & 15;
    return (font[code] >> (5 * (gy / s) + col)) & 1 ? 2 : 1;
}

}  // namespace vp
