"""Seeded cases of the label stage (csrc/labelgeom.h) and the runners that write one case through each statement of the contract: the host tap
vp_dbg_draw_labels_host, the numpy twin, the scalar model of tests/label_model.py, and the device (vp_draw_labels).  Shared by tests/test_label_host.py and
tests/test_gpu_label.py; a case is data only and is never modified: every runner writes on fresh frames built from the case's seed (draw_cases.build_frames:
frames inside larger seeded buffers, so the pitch padding is a sentinel, and a runner returns the WHOLE buffers).
"""
import numpy as np

from easy_vitpose_amd.draw import LIMB_COLORS, LabelStyle, draw_labels_model_host, draw_labels_numpy
from draw_cases import EVEN, ODD, build_frames, same  # noqa: F401 -- `same` is re-exported

LIGHT_DARK = ((250, 240, 200), (10, 20, 60), (128, 128, 128), (0, 110, 0))   # luma 77 R + 150 G + 29 B: 61050, 5510, 32768 (the threshold itself), 16500


def case(specs, boxes, fi, style=LabelStyle(), rank=None, ids=None, scores=None, seed=0):
    return dict(specs=specs, boxes=np.asarray(boxes, np.float32).reshape(-1, 4), fi=np.asarray(fi, np.int32), style=style,
                rank=None if rank is None else np.asarray(rank, np.int32), ids=None if ids is None else np.asarray(ids, np.int32),
                scores=None if scores is None else np.asarray(scores, np.float32), seed=seed)


def crowd(rng, n, h, w):
    """n boxes with top-left corners all over an h x w frame (some tags clipped by its edges)"""
    x1, y1 = rng.uniform(-8, w - 4, n), rng.uniform(-4, h + 4, n)
    return np.stack([x1, y1, x1 + rng.uniform(5, 60, n), y1 + rng.uniform(5, 60, n)], -1).astype(np.float32)


def host_cases():
    """name -> case: the CPU set (also the device's)"""
    out = {}
    rng = np.random.default_rng(23)
    scales = (1, 2, 3, 0)
    for k, (fmt, matrix) in enumerate((f, m) for f in ('rgb', 'bgr', 'nv12') for m in ('bt601', 'bt709', 'bt601_full')):
        h, w = ODD if k % 2 == 0 else EVEN
        out[f'{fmt}_{matrix}_{h}x{w}_s{scales[k % 4]}'] = case([(h, w, fmt, matrix, 0)], crowd(rng, 5, h, w), np.zeros(5), LabelStyle(scale=scales[k % 4]),
                                                          ids=[3, -1, -9, 12, 2147483647], scores=rng.uniform(0, 1, 5), seed=len(out))
    for fmt in ('rgb', 'nv12'):
        out[f'{fmt}_pitched'] = case([(97, 131, fmt, 'bt709', 37)], crowd(rng, 4, *ODD), np.zeros(4), LabelStyle(scale=1), scores=rng.uniform(-3, 3, 4), seed=40)
    # every edge of a 97 x 131 frame, and tags that lie wholly off it (the last four rows): left, right, top (y1 < 0: the tag hangs from y1), bottom (y1 beyond
    # the last row: the tag above it crosses the edge); off-frame: right of it, above it, far left, below it
    edges = [[-5, 40, 30, 80], [120, 40, 130, 80], [40, -4, 90, 30], [60, 100, 90, 120], [140, 40, 150, 60], [20, -50, 60, -30], [-2000, 30, -1900, 60], [10, 200, 40, 230]]
    for fmt in ('rgb', 'nv12'):
        out[f'edges_{fmt}'] = case([(97, 131, fmt, 'bt601', 3)], edges, np.zeros(8), LabelStyle(scale=1), ids=np.arange(8) * 11, scores=np.linspace(0.1, 0.9, 8), seed=41)
    out['bottom_inside_s8'] = case([(64, 96, 'nv12', 'bt601', 0)], [[3, 10, 90, 60]], [0], LabelStyle(scale=8), ids=[4], seed=42)   # 9 s = 72 > y1: hangs from y1 = 10 to row 81
    # y1 - 9 s = -1, 0, 1 at s = 2: inside the box, then above it from row 0 and from row 1
    out['above_or_inside'] = case([(97, 131, 'nv12', 'bt709', 0)], [[2, 17, 40, 60], [45, 18, 80, 60], [88, 19, 120, 60]], np.zeros(3), LabelStyle(scale=2), ids=[1, 2, 3], seed=43)
    # overlapping tags at odd offsets: the later row wins, and chroma samples straddle two tags
    out['overlap2'] = case([(97, 131, 'nv12', 'bt601', 0)], [[10, 30, 60, 80], [23, 35, 70, 90]], np.zeros(2), LabelStyle(scale=1), ids=[5, 6], scores=[0.5, 0.25], seed=44)
    out['overlap3'] = case([(64, 96, 'nv12', 'bt601_full', 5)], [[5, 30, 60, 60], [12, 37, 70, 62], [9, 41, 50, 63]], np.zeros(3), LabelStyle(scale=2), ids=[7, 1, 4],
                           scores=[0.875, 0.125, 0.375], seed=45)
    out['overlap3_rgb'] = case([(64, 96, 'rgb', 'bt601', 0)], [[5, 30, 60, 60], [12, 37, 70, 62], [9, 41, 50, 63]], np.zeros(3), LabelStyle(scale=2), ids=[7, 1, 4], seed=46)
    nan = np.nan
    gates = [[10, 20, 50, 60], [40, 40, 80, 80], [nan, nan, nan, nan], [nan, 30, 60, 70], [16384, 30, 60, 70], [30, -16384, 60, 70], [16383.5, 50, 20.5, 70.9],
             [70, 60, -16383.9, 30], [60, 80, 90, 95]]
    out['gates'] = case([(97, 131, 'bgr', 'bt601', 0)], gates, np.zeros(9), LabelStyle(scale=1), rank=[0, -1, 0, 1, 2, 3, 4, 5, -3], ids=[1, 2, -1, 4, 5, 6, 7, 8, 9],
                        scores=[0.9] * 9, seed=47)
    bx = crowd(rng, 4, *EVEN)
    out['no_scores'] = case([(64, 96, 'rgb', 'bt601', 0)], bx, np.zeros(4), LabelStyle(scale=1), ids=[10, 20, 30, 40], seed=48)
    out['show_score_off'] = case([(64, 96, 'rgb', 'bt601', 0)], bx, np.zeros(4), LabelStyle(scale=1, show_score=False), ids=[10, 20, 30, 40], scores=[0.1, 0.2, 0.3, 0.4], seed=48)
    out['odd_scores'] = case([(97, 131, 'nv12', 'bt601', 0)], [[5, 12, 9, 20], [5, 30, 9, 40], [5, 48, 9, 50], [5, 66, 9, 70], [5, 84, 9, 90]], np.zeros(5), LabelStyle(scale=1),
                             ids=[0, 7, -1, 2147483647, -2147483648], scores=[nan, -0.0, np.inf, 999.99994, -999.99994], seed=49)
    spots = [[4, 12, 9, 20], [50, 12, 60, 20], [4, 40, 9, 50], [50, 40, 60, 50]]
    out['auto_ink'] = case([(64, 96, 'nv12', 'bt601', 0)], spots, np.zeros(4), LabelStyle(scale=1, colors=LIGHT_DARK), ids=[0, 1, 2, 3], scores=[0.5] * 4, seed=50)
    out['explicit_ink'] = case([(64, 96, 'rgb', 'bt601', 0)], spots, np.zeros(4), LabelStyle(scale=1, colors=LIGHT_DARK, ink=(255, 0, 128)), ids=[0, 1, 2, 3], scores=[0.5] * 4, seed=51)
    bx = np.concatenate([crowd(rng, 3, *ODD), crowd(rng, 3, *EVEN)])[[0, 3, 1, 4, 2, 5]]
    out['two_frames'] = case([(97, 131, 'rgb', 'bt601', 0), (64, 96, 'nv12', 'bt709', 3)], bx, [0, 1, 0, 1, 0, 1], LabelStyle(scale=1), scores=rng.uniform(0, 1, 6), seed=52)
    out['no_row_frame'] = case([(97, 131, 'rgb', 'bt601', 0), (64, 96, 'nv12', 'bt601', 0), (64, 96, 'bgr', 'bt601', 0)], crowd(rng, 4, 60, 90), [0, -1, 3, 2], LabelStyle(scale=1), seed=53)
    return out


def crowd_case(fmt):
    """600 overlapping tags on a 64 x 96 frame: the raster pass walks the later rows in chunks of 256, so a row has up to three chunks of them, most of which hit
    its tiles"""
    rng = np.random.default_rng(31)
    return case([(64, 96, fmt, 'bt601', 7)], crowd(rng, 600, *EVEN), np.zeros(600), LabelStyle(scale=1), ids=rng.integers(-99, 999, 600), scores=rng.uniform(0, 1, 600),
                rank=np.where(rng.random(600) < 0.1, -1, 0), seed=60)


def run_tap(cs):
    frames, buffers = build_frames(cs['specs'], cs['seed'])
    draw_labels_model_host(frames, cs['boxes'], cs['fi'], cs['style'], rank=cs['rank'], ids=cs['ids'], scores=cs['scores'])
    return buffers


def run_numpy(cs):
    frames, buffers = build_frames(cs['specs'], cs['seed'])
    draw_labels_numpy(frames, cs['boxes'], cs['fi'], cs['style'], rank=cs['rank'], ids=cs['ids'], scores=cs['scores'])
    return buffers


def run_model(cs):
    """(buffers, written): the scalar model's picture and, per frame, the bytes it wrote"""
    from label_model import label_model
    frames, buffers = build_frames(cs['specs'], cs['seed'])
    st = cs['style']
    written = label_model(frames, cs['boxes'], cs['fi'], st.colors if st.colors is not None else LIMB_COLORS, st.scale, st.ink, st.show_score, rank=cs['rank'],
                          ids=cs['ids'], scores=cs['scores'])
    return buffers, written


def run_device(cs, engine):
    frames, buffers = build_frames(cs['specs'], cs['seed'])
    engine.draw_labels_host(frames, cs['boxes'], cs['fi'], cs['style'], rank=cs['rank'], ids=cs['ids'], scores=cs['scores'])
    return buffers
