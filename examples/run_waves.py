#!/usr/bin/env python3
"""Wavelets and tips of a spiral wave: the Fenton 4-variable sheet with a circular obstacle, S1 from the left edge, S2 in the
upper-left quadrant.  Every `--every` ticks the device labels the excited domains (fib_tf_amd/waves.py) and finds the phase
singularities (fib_tf_amd/tips.py); nothing is read back between the samples.  The PNG shows, through the headless Screen, the
wavelet count (bright) beside the tip count (dim) over time on top, and below them the label plane of the last sample, every
wave in a grey of its own.

    python examples/run_waves.py [--size N] [--ms T] [--every K] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.screen import Screen


def steps(panel, values, top, grey):
    """draws the integer series `values` left to right into the [h, w] panel, `top` at its upper edge"""
    h, w = panel.shape
    if len(values) == 0:
        return
    cols = np.linspace(0, w - 1, len(values)).astype(int)
    rows = (h - 1) * (1.0 - np.minimum(np.asarray(values, np.float64), top) / top)
    panel[rows.astype(int), cols] = grey


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--ms', type=float, default=600.0)
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--out', default='waves.png')
    args = ap.parse_args(argv)
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': args.ms})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 1.0)
    second_stimulus = sheet.millisecond_to_step(210)
    with sheet.record_waves(every=args.every) as waves, sheet.record_tips(every=args.every) as tips:
        for tick in sheet.run():
            if tick == second_stimulus:
                sheet.fire_op('s2')
        counts = waves.counts()
        if len(counts) == 0:
            print('no sample was taken (--ms shorter than --every ticks)')
            return None
        per_sample = waves.waves()
        labels = waves.labels()
        tip_counts = tips.counts()
        t = waves.times_ms()
    n_waves, n_tips = counts[:, 0], tip_counts[:, 0] + tip_counts[:, 1]
    last = per_sample[-1]
    print('%d samples up to %.1f ms; up to %d waves and %d tips at a time; the last sample has %d waves, the largest of %d cells'
          % (len(t), t[-1], n_waves.max(), n_tips.max(), len(last), last['area'].max() if len(last) else 0))
    h = 64
    frame = np.full((h + 1 + n, max(n, 256)), 0.1, np.float32)
    top = max(int(n_waves.max()), int(n_tips.max()), 1)
    steps(frame[:h], n_tips, top, 0.5)
    steps(frame[:h], n_waves, top, 1.0)
    frame[h] = 0.0
    seeds = np.unique(labels[labels >= 0])
    grey = np.zeros(labels.shape, np.float32)
    for k, seed in enumerate(seeds):
        grey[labels == seed] = 0.35 + 0.65 * (k + 1) / len(seeds)
    frame[h + 1:, :n] = grey
    screen = Screen(frame.shape[0], frame.shape[1], 'waves (bright) and tips (dim) over time; the waves of the last sample')
    screen.imshow(frame)
    screen.save(args.out)
    print('written to %s' % args.out)
    return n_waves, n_tips, labels


if __name__ == '__main__':
    main()
