#!/usr/bin/env python3
"""Rotor trajectories of the four-variable atrial model's S1-S2 spiral: a planar wave from the left edge (S1), a second
stimulus in the upper-left quadrant 210 ms later, and the broken end curling around the obstacle.  The spiral tips are found
on the device every `--every` ticks (fib_tf_amd/tips.py: nothing is read back between the samples), linked into
trajectories on the host, and drawn over the last frame into a greyscale PNG through the headless Screen: +1 rotors
white, -1 rotors black.

    python examples/run_tips.py [--size N] [--ms T] [--every K] [--max-jump PX] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd import tips
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.screen import Screen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ms', type=float, default=1000.0)
    ap.add_argument('--every', type=int, default=2)
    ap.add_argument('--max-jump', type=float, default=6.0)
    ap.add_argument('--out', default='tips.png')
    args = ap.parse_args()
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': args.ms, 'dt_per_plot': 10})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 1.0)
    second_stimulus = sheet.millisecond_to_step(210)
    with sheet.record_tips(every=args.every) as rec:         # U against the v gate, under the mask phase > 0.5
        for tick in sheet.run():
            if tick == second_stimulus:
                sheet.fire_op('s2')
        per_sample = rec.tips()
        counts = rec.counts()
        cut = rec.truncated()
    paths = tips.link(per_sample, args.max_jump)
    print('%d samples, at most %d tips in one, %d trajectories (%d samples had more tips than the lists hold)'
          % (len(per_sample), int(counts[:, 2].max()) if len(counts) else 0, len(paths), len(cut)))
    for p in sorted(paths, key=lambda p: -len(p.points))[:10]:
        print('  charge %+d: %4d samples, %7.1f .. %7.1f ms, from (%.1f, %.1f) to (%.1f, %.1f)'
              % (p.charge, len(p.points), p.points['t_ms'][0], p.points['t_ms'][-1], p.points['y'][0], p.points['x'][0],
                 p.points['y'][-1], p.points['x'][-1]))
    frame = 0.25 + 0.5 * np.clip(sheet.image() * sheet.phase, 0.0, 1.0)          # the last frame in mid-greys
    for p in paths:
        rows = np.clip(p.points['y'].astype(int), 0, n - 1)
        cols = np.clip(p.points['x'].astype(int), 0, n - 1)
        frame[rows, cols] = 1.0 if p.charge > 0 else 0.0
    screen = Screen(n, n, 'rotor trajectories')
    screen.imshow(frame)
    screen.save(args.out)
    print('trajectories over the last frame written to %s' % args.out)


if __name__ == '__main__':
    main()
