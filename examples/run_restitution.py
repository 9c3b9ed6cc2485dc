#!/usr/bin/env python3
"""A dynamic restitution protocol run entirely on the device: a Fenton 4v sheet paced from its left edge by a train whose
cycle length shortens step by step (a stimulus program, fib_tf_amd/stimulus.py: one `s1_train` per cycle length), while the
beat recorder (fib_tf_amd/beats.py) keeps the last beats of every cell.  At the end of every step the ring of the centre column
is read, and each beat's action-potential duration is drawn against the diastolic interval in front of it: the APD restitution
curve, written as a PNG through the headless Screen (DI to the right, APD upwards).  Nothing is read back while a step runs.

    python examples/run_restitution.py [--size N] [--from-ms T] [--to-ms T] [--step-ms T] [--beats K] [--every K] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.screen import Screen
from fib_tf_amd.stimulus import s1_train


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--from-ms', type=float, default=400.0, help='the first cycle length')
    ap.add_argument('--to-ms', type=float, default=200.0, help='the last cycle length')
    ap.add_argument('--step-ms', type=float, default=25.0)
    ap.add_argument('--beats', type=int, default=6, help='stimuli per cycle length')
    ap.add_argument('--every', type=int, default=5)
    ap.add_argument('--out', default='restitution.png')
    args = ap.parse_args(argv)
    n = args.size
    cycles = np.arange(args.from_ms, args.to_ms - 1e-9, -args.step_ms)
    total_ms = float(sum(c * args.beats for c in cycles)) + 50.0
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': total_ms, 'dt_per_plot': 10})
    sheet.define(s1=False)                       # no wave from define(): the program's first stimulus follows tick 0
    protocol, start = [], 0.0
    for c in cycles:                             # one train per cycle length, back to back
        protocol += s1_train('left', 1.0, period_ms=float(c), n=args.beats, start_ms=start)
        start += c * args.beats
    column = np.zeros((n, n), bool)
    column[:, n // 2] = True
    points = []
    with sheet.program_stimuli(protocol) as prog, sheet.record_beats(every=args.every, depth=min(16, args.beats + 1)) as rec:
        ticks = iter(sheet.run())
        for c in cycles:
            for _ in range(sheet.millisecond_to_step(c * args.beats)):
                next(ticks, None)
            di, apd = rec.restitution(mask=column)                   # the beats of this step (and the last of the one before)
            s = rec.summary(last=min(4, rec.depth))
            alt = np.nanmax(np.abs(s['apd_alt'])) if np.isfinite(s['apd_alt']).any() else float('nan')
            print('CL %5.0f ms: %5d (DI, APD) pairs in the centre column, mean APD %6.1f ms, beats per cell %d .. %d, largest |alternans| %.1f ms'
                  % (c, len(di), np.nanmean(s['apd_mean']), rec.beats()['count'].min(), rec.beats()['count'].max(), alt))
            points.append(np.stack([di, apd], axis=1))
        for _ in ticks:
            pass
        print('%d stimuli applied' % prog.applied())
    pts = np.concatenate(points) if points else np.zeros((0, 2))
    pts = np.unique(np.round(pts, 3), axis=0)                        # (a ring read twice gives its beats twice)
    if not len(pts):
        sys.exit('no beat with a diastolic interval in front of it: pace longer or slower')
    size = 256
    image = np.zeros((size, size), np.float32)
    hi = float(max(pts.max(), 1.0)) * 1.05
    x = np.clip((pts[:, 0] / hi * (size - 1)).astype(int), 0, size - 1)
    y = np.clip((pts[:, 1] / hi * (size - 1)).astype(int), 0, size - 1)
    image[size - 1 - y, x] = 1.0
    screen = Screen(size, size, 'restitution')
    screen.imshow(image)
    screen.save(args.out)
    print('APD against DI, both 0 .. %.0f ms, %d points, written to %s' % (hi, len(pts), args.out))
    return pts


if __name__ == '__main__':
    main()
