"""Per-layer share of a forward of the detector network from a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/yolo_bench.py --trace SCALE BATCH
    python tools/yolo_trace_share.py DIR SCALE BATCH [--size 640]

Reads every *kernel_trace.csv under DIR, keeps the dispatches of the stage's kernels (yolo_*) in start order, folds them onto the plan's launches (the trace holds
a whole number of forwards) and prints, per model.{i} layer, the median time of a forward spent there and its share.  Needs no GPU."""
from __future__ import annotations

import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from easy_vitpose_amd.devyolo import synth_yolo, yolo_plan
    d, scale, batch = sys.argv[1], sys.argv[2], int(sys.argv[3])
    size = int(sys.argv[sys.argv.index('--size') + 1]) if '--size' in sys.argv else 640
    rows = []
    for path in glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True):
        with open(path, newline='') as f:
            for r in csv.DictReader(f):
                if 'yolo_' in r['Kernel_Name']:
                    rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp']), r['Kernel_Name']))
    rows.sort()
    _, launches, _ = yolo_plan(synth_yolo(scale, 80, 0), (size, size), max_images=batch)
    nl = len(launches)
    assert rows and len(rows) % nl == 0, f'{len(rows)} dispatches of the stage, the plan has {nl} launches'
    per = np.asarray([r[1] for r in rows], np.float64).reshape(-1, nl) / 1e3   # us, [forward, launch]
    med = np.median(per, axis=0)
    total = float(med.sum())
    print(f'## per-layer share, scale {scale}, batch {batch}, {size} x {size}: kernel time from a kernel trace of its own, median of {per.shape[0]} forwards; '
          f'sum of kernels {total / 1e3:.3f} ms')
    by = {}
    for l, t in zip(launches, med):
        key = 'pack' if l['layer'] < 0 else ('model.22 decode' if l['kind'] == 'decode' else f"model.{l['layer']}")
        by.setdefault(key, [0.0, 0])
        by[key][0] += float(t)
        by[key][1] += 1
    for key, (t, n) in by.items():
        print(f'{key:<16} {n:>3} launches {t:>9.1f} us {t / total:>6.1%}')
    kinds = {}
    for l, t in zip(launches, med):
        name = l['kind'] + (f" {l['k']}x{l['k']} s{l['s']}" if l['kind'] == 'conv' else '')
        kinds[name] = kinds.get(name, 0.0) + float(t)
    print('by kind: ' + ', '.join(f'{k} {v / total:.1%}' for k, v in sorted(kinds.items(), key=lambda kv: -kv[1])))


if __name__ == '__main__':
    main()
