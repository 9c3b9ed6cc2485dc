#!/usr/bin/env python3
"""The two halves of the restitution pair from one run on the device: the pacing staircase of examples/run_restitution.py — a
Fenton 4v sheet paced from its left edge by a train whose cycle length shortens step by step — with the beat recorder keeping the
last beats of every cell.  At the end of every step the conduction velocity of every beat of the ring is fitted on the device
(fib_tf_amd/velocity.py: BeatRecorder.cv_restitution) and paired with the diastolic interval in front of it, beside the APD
pairs of restitution().  Two panels are written as one PNG through the headless Screen: APD against DI on the left, CV against DI
on the right (DI to the right, the quantity upwards); and the speed map of the last beat as a second PNG.

    python examples/run_cv_restitution.py [--size N] [--from-ms T] [--to-ms T] [--step-ms T] [--beats K] [--every K] [--radius R]
                                          [--out FILE] [--speed-out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.screen import Screen
from fib_tf_amd.stimulus import s1_train


def panel(x, y, x_hi, y_hi, size=256):
    """the points as a size x size picture: x to the right over 0 .. x_hi, y upwards over 0 .. y_hi"""
    image = np.zeros((size, size), np.float32)
    if len(x):
        c = np.clip((x / x_hi * (size - 1)).astype(int), 0, size - 1)
        r = np.clip((y / y_hi * (size - 1)).astype(int), 0, size - 1)
        image[size - 1 - r, c] = 1.0
    return image


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--from-ms', type=float, default=400.0, help='the first cycle length')
    ap.add_argument('--to-ms', type=float, default=200.0, help='the last cycle length')
    ap.add_argument('--step-ms', type=float, default=25.0)
    ap.add_argument('--beats', type=int, default=6, help='stimuli per cycle length')
    ap.add_argument('--every', type=int, default=2, help='ticks per sample: the time resolution of the upstrokes')
    ap.add_argument('--radius', type=int, default=3)
    ap.add_argument('--out', default='cv_restitution.png')
    ap.add_argument('--speed-out', default='cv_speed.png')
    args = ap.parse_args(argv)
    n = args.size
    cycles = np.arange(args.from_ms, args.to_ms - 1e-9, -args.step_ms)
    total_ms = float(sum(c * args.beats for c in cycles)) + 50.0
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': total_ms, 'dt_per_plot': 10})
    sheet.define(s1=False)
    protocol, start = [], 0.0
    for c in cycles:
        protocol += s1_train('left', 1.0, period_ms=float(c), n=args.beats, start_ms=start)
        start += c * args.beats
    # away from the paced edge (where the front is still forming) and from the far one (where it runs out)
    middle = np.zeros((n, n), bool)
    middle[:, n // 4:3 * n // 4] = True
    max_dt = 0.4 * float(cycles.min())                       # below half the shortest cycle length
    apd_pts, cv_pts, speed = [], [], None
    with sheet.program_stimuli(protocol) as prog, sheet.record_beats(every=args.every, depth=min(16, args.beats + 1)) as rec:
        ticks = iter(sheet.run())
        for c in cycles:
            for _ in range(sheet.millisecond_to_step(c * args.beats)):
                next(ticks, None)
            di_a, apd = rec.restitution(mask=middle)
            di_c, cv = rec.cv_restitution(mask=middle, max_rms=1.0, radius=args.radius, max_dt=max_dt)
            print('CL %5.0f ms: %6d (DI, APD) and %6d (DI, CV) pairs; median APD %6.1f ms, median CV %.3f cells/ms'
                  % (c, len(di_a), len(di_c), np.median(apd) if len(apd) else np.nan, np.median(cv) if len(cv) else np.nan))
            apd_pts.append(np.stack([di_a, apd], axis=1))
            cv_pts.append(np.stack([di_c, cv], axis=1))
        speed = rec.speed(last=1, radius=args.radius, max_dt=max_dt)[-1]
        for _ in ticks:
            pass
        print('%d stimuli applied' % prog.applied())
    a = np.unique(np.round(np.concatenate(apd_pts), 3), axis=0)      # (a ring read twice gives its beats twice)
    v = np.unique(np.round(np.concatenate(cv_pts), 4), axis=0)
    if not len(a) or not len(v):
        sys.exit('no beat with a diastolic interval in front of it and a fit: pace longer or slower')
    di_hi = float(max(a[:, 0].max(), v[:, 0].max(), 1.0)) * 1.05
    apd_hi, cv_hi = float(a[:, 1].max()) * 1.05, 2.0 * float(np.median(v[:, 1]))          # (a stray fit on times that hardly differ is clipped)
    size = 256
    both = np.concatenate([panel(a[:, 0], a[:, 1], di_hi, apd_hi, size), np.full((size, 4), 0.5, np.float32),
                           panel(v[:, 0], v[:, 1], di_hi, cv_hi, size)], axis=1)
    screen = Screen(both.shape[0], both.shape[1], 'cv restitution')
    screen.imshow(both)
    screen.save(args.out)
    print('APD (0 .. %.0f ms) and CV (0 .. %.2f cells/ms) against DI (0 .. %.0f ms), %d and %d points, written to %s'
          % (apd_hi, cv_hi, di_hi, len(a), len(v), args.out))
    fin = np.isfinite(speed)
    top = 2.0 * float(np.median(speed[fin])) if fin.any() else 1.0      # (under the paced columns all cells fire at once: clipped to white)
    screen = Screen(n, n, 'speed')
    screen.imshow(np.where(fin, np.clip(speed / top, 0, 1), 0.0).astype(np.float32))       # black: no fit
    screen.save(args.speed_out)
    print('speed of the last beat, 0 .. %.2f cells/ms (black: no fit at %d of %d cells), written to %s'
          % (top, int((~fin).sum()), fin.size, args.speed_out))
    return a, v


if __name__ == '__main__':
    main()
