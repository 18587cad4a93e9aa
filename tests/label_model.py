"""The label stage contract (csrc/labelgeom.h) restated in plain scalar Python, as a GATHER: every tag of the call gives two primitives, its background block and
its ink, with the order index 2 * row + (ink ? 1 : 0); every pixel takes the covering primitive with the highest order index, every chroma sample the highest one
among its up-to-four pixels.  The host tap and the numpy twin are painters (a later row overwrites an earlier one); this file is the other formulation.

Independent of the header where it can be: the text comes from Python's own formatter, the font is written out as pictures, the glyph lookup uses floor
divisions from the block's corner, not the header's glyph origin; plain Python integers (unbounded), float32 compares through numpy scalars.
"""
import numpy as np

from draw_model import rgb_to_yuv, usable

FONT = {   # 5 x 7, '#' = ink
    '#': ('.#.#.', '.#.#.', '#####', '.#.#.', '#####', '.#.#.', '.#.#.'),
    '0': ('.###.', '#...#', '#..##', '#.#.#', '##..#', '#...#', '.###.'),
    '1': ('..#..', '.##..', '..#..', '..#..', '..#..', '..#..', '.###.'),
    '2': ('.###.', '#...#', '....#', '...#.', '..#..', '.#...', '#####'),
    '3': ('#####', '...#.', '..#..', '...#.', '....#', '#...#', '.###.'),
    '4': ('...#.', '..##.', '.#.#.', '#..#.', '#####', '...#.', '...#.'),
    '5': ('#####', '#....', '####.', '....#', '....#', '#...#', '.###.'),
    '6': ('..##.', '.#...', '#....', '####.', '#...#', '#...#', '.###.'),
    '7': ('#####', '....#', '...#.', '..#..', '.#...', '.#...', '.#...'),
    '8': ('.###.', '#...#', '#...#', '.###.', '#...#', '#...#', '.###.'),
    '9': ('.###.', '#...#', '#...#', '.####', '....#', '...#.', '.##..'),
    ':': ('.....', '..#..', '..#..', '.....', '..#..', '..#..', '.....'),
    '.': ('.....', '.....', '.....', '.....', '.....', '.##..', '.##..'),
    '-': ('.....', '.....', '.....', '#####', '.....', '.....', '.....'),
    ' ': ('.....', '.....', '.....', '.....', '.....', '.....', '.....'),
    '?': ('#####', '#...#', '#...#', '#...#', '#...#', '#...#', '#####'),   # the spare symbol
}


def text_of(pid, score, show_score):
    if score is None or not show_score:
        return f'#{pid}'
    s = float(np.float32(score))
    return f'#{pid}: {s:.2f}' if -1000.0 < s < 1000.0 else f'#{pid}'


def tags(boxes, frame_index, n_frames, hw, colors, scale, ink, show_score, rank=None, ids=None, scores=None):
    """[(row, frame, x1, by, s, text, background RGB, ink RGB)] of the rows that pass the gates"""
    out = []
    for i in range(len(boxes)):
        f = int(frame_index[i])
        if f < 0 or f >= n_frames or (rank is not None and int(rank[i]) < 0) or not all(usable(v) for v in boxes[i]):
            continue
        xa, ya, xb, yb = (int(float(v)) for v in boxes[i])
        x1, y1 = min(xa, xb), min(ya, yb)
        pid = int(ids[i]) if ids is not None else i
        h, w = hw[f]
        s = scale if scale > 0 else min(8, max(1, min(h, w) // 400))
        by = y1 - 9 * s if y1 - 9 * s >= 0 else y1
        bg = tuple(int(c) for c in colors[pid % len(colors)])
        if ink is None:
            fg = (0, 0, 0) if 77 * bg[0] + 150 * bg[1] + 29 * bg[2] >= 32768 else (255, 255, 255)
        else:
            fg = tuple(int(c) for c in ink)
        out.append((i, f, x1, by, s, text_of(pid, None if scores is None else scores[i], show_score), bg, fg))
    return out


def cover(tag, px, py):
    """None: the pixel is outside the tag's block; else 0 (background) or 1 (ink)"""
    _, _, x1, by, s, text, _, _ = tag
    if not (x1 <= px < x1 + s * (6 * len(text) + 1) and by <= py < by + 9 * s):
        return None
    u, v = (px - x1) // s - 1, (py - by) // s - 1   # font bits from the inside of the one-bit margin
    if u < 0 or not 0 <= v < 7 or u % 6 >= 5 or u // 6 >= len(text):
        return 0
    return 1 if FONT[text[u // 6]][v][u % 6] == '#' else 0


def label_model(frames, boxes, frame_index, colors, scale, ink, show_score, rank=None, ids=None, scores=None):
    """Writes in place on `frames` (cropprep.Frame over numpy planes) byte by byte.  Returns per frame the list of (plane, row, byte column) it wrote."""
    all_tags = tags(boxes, frame_index, len(frames), [(fr.h, fr.w) for fr in frames], colors, scale, ink, show_score, rank, ids, scores)
    written = []
    for f, fr in enumerate(frames):
        h, w = fr.h, fr.w
        win = [[-1] * w for _ in range(h)]   # the highest order index that covers the pixel
        color = {}
        for tag in all_tags:
            if tag[1] != f:
                continue
            row, _, x1, by, s, text, bg, fg = tag
            color[2 * row], color[2 * row + 1] = bg, fg
            for py in range(max(by, 0), min(by + 9 * s, h)):
                for px in range(max(x1, 0), min(x1 + s * (6 * len(text) + 1), w)):
                    c = cover(tag, px, py)
                    if c is not None and 2 * row + c > win[py][px]:
                        win[py][px] = 2 * row + c
        wr = []
        if fr.format != 'nv12':
            for py in range(h):
                for px in range(w):
                    if win[py][px] >= 0:
                        rgb = color[win[py][px]]
                        for c in range(3):
                            fr.planes[0][py, px, c] = rgb[2 - c] if fr.format == 'bgr' else rgb[c]
                            wr.append((0, py, 3 * px + c))
        else:
            for py in range(h):
                for px in range(w):
                    if win[py][px] >= 0:
                        fr.planes[0][py, px] = rgb_to_yuv(color[win[py][px]], fr.matrix)[0]
                        wr.append((0, py, px))
            for cy in range((h + 1) // 2):
                for cx in range((w + 1) // 2):
                    best = max(win[py][px] for py in (2 * cy, 2 * cy + 1) if py < h for px in (2 * cx, 2 * cx + 1) if px < w)
                    if best >= 0:
                        _, u, v = rgb_to_yuv(color[best], fr.matrix)
                        fr.planes[1][cy, cx, 0], fr.planes[1][cy, cx, 1] = u, v
                        wr += [(1, cy, 2 * cx), (1, cy, 2 * cx + 1)]
        written.append(wr)
    return written
