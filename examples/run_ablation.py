#!/usr/bin/env python3
"""Ablating a rotor while the recorders watch: the four-variable atrial model's S1-S2 spiral with a tip recorder and a wave
recorder attached throughout; some hundred milliseconds after the S2 the host reads where a tip is and draws a line of block —
a catheter dragged, one disc lesion per dwell time, from the tip's neighbourhood to the nearest border (fib_tf_amd/lesions.py:
the lesions are burnt on the device, right after their ticks, and neither recorder is detached).  Printed: the tip and wavelet
counts across the intervention.  Written: the last frame times the final phase field, with the counts drawn underneath.

    python examples/run_ablation.py [--size N] [--ms T] [--s2-ms T] [--ablate-ms T] [--dwell-ms T] [--radius R] [--every K] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd import lesions
from fib_tf_amd.fenton import Fenton4v


def path_to_border(row, col, n, step):
    """points from (row, col) straight to the nearest border of the n x n sheet, `step` cells apart"""
    dist = {'top': row, 'bottom': n - 1 - row, 'left': col, 'right': n - 1 - col}
    side = min(dist, key=dist.get)
    dr, dc = {'top': (-1, 0), 'bottom': (1, 0), 'left': (0, -1), 'right': (0, 1)}[side]
    count = int(dist[side] // step) + 2
    return [(float(np.clip(row + dr * step * i, 0, n - 1)), float(np.clip(col + dc * step * i, 0, n - 1))) for i in range(count)]


def strip(values, width, rows=48):
    """a series drawn as a bar strip of `width` columns: one grey bar per sample"""
    out = np.zeros((rows, width), np.float32)
    if len(values):
        top = max(1, int(np.max(values)))
        for x in range(width):
            v = values[min(len(values) - 1, x * len(values) // width)]
            out[rows - int(round((rows - 1) * v / top)) - 1:, x] = 0.8
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ms', type=float, default=900.0)
    ap.add_argument('--s2-ms', type=float, default=210.0)
    ap.add_argument('--ablate-ms', type=float, default=500.0)
    ap.add_argument('--dwell-ms', type=float, default=4.0)
    ap.add_argument('--radius', type=float, default=3.0)
    ap.add_argument('--every', type=int, default=5)
    ap.add_argument('--out', default='ablation.png')
    ap.add_argument('--no-plot', action='store_true')
    args = ap.parse_args(argv)
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': args.ms, 'dt_per_plot': 10})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 1.0)
    s2, ablate = sheet.millisecond_to_step(args.s2_ms), sheet.millisecond_to_step(args.ablate_ms)
    tips = sheet.record_tips(every=args.every)
    waves = sheet.record_waves(every=args.every)
    prog, path = None, []
    for tick in sheet.run():
        if tick == s2:
            sheet.fire_op('s2')
        if tick == ablate:
            # the host-side part of the loop: where is a tip now?  (no tip: the sheet's centre, next to the obstacle)
            latest = [t for t in tips.tips() if len(t)]
            row, col = (float(latest[-1]['y'][0]), float(latest[-1]['x'][0])) if latest else (n / 2.0, n / 2.0)
            path = path_to_border(row, col, n, max(1.0, args.radius))
            prog = sheet.program_lesions(lesions.drag(path, start_ms=0.0, dwell_ms=args.dwell_ms, radius=args.radius))
            print('tick %d: a line of %d lesions from (%.1f, %.1f) to (%.1f, %.1f)' % ((tick, len(path), row, col) + path[-1]))
    applied = prog.applied() if prog else 0
    if prog:
        prog.end()                                        # sheet.phase is the field as it now is
    tip_counts, wave_counts = tips.counts(), waves.counts()
    n_tips = tip_counts[:, 0] + tip_counts[:, 1]
    print('%d lesions applied; %d samples' % (applied, len(n_tips)))
    cut = (ablate + 1) // args.every
    for name, series in (('tips', n_tips), ('wavelets', wave_counts[:, 0])):
        before, after = series[:cut], series[cut:]
        print('  %-8s before: mean %.2f, max %d   after: mean %.2f, max %d, last %d'
              % (name, before.mean() if len(before) else 0, before.max() if len(before) else 0, after.mean() if len(after) else 0,
                 after.max() if len(after) else 0, series[-1] if len(series) else 0))
    frame = np.clip(sheet.image() * sheet.phase, 0.0, 1.0)
    tips.close()
    waves.close()
    if not args.no_plot:
        from fib_tf_amd.screen import Screen
        picture = np.vstack([frame, strip(n_tips, n), strip(wave_counts[:, 0], n)])
        screen = Screen(picture.shape[0], picture.shape[1], 'ablation')
        screen.imshow(picture)
        screen.save(args.out)
        print('the last frame times the final phase field, the tip counts and the wavelet counts written to %s' % args.out)
    return {'applied': applied, 'path': path, 'tip_counts': n_tips, 'wave_counts': wave_counts[:, 0], 'phase': sheet.phase, 'frame': frame}


if __name__ == '__main__':
    main()
