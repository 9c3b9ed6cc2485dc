#!/usr/bin/env python3
"""Unipolar and bipolar electrograms of a spiral wave: the Fenton 4-variable sheet with a circular obstacle, S1 from the left
edge, S2 in the upper-left quadrant, and four point electrodes two cells above the sheet on a line through the middle.  Every
`--every` ticks the device forms the membrane current div(phi grad V) and sums it through the four lead fields
(fib_tf_amd/leads.py: nothing is read back between the samples).  The four unipolar traces and the three bipolar traces of
neighbouring electrodes are drawn, one above the other, into a greyscale PNG through the headless Screen.

    python examples/run_unipolar.py [--size N] [--ms T] [--every K] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd import leads
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.screen import Screen


def curve(panel, values):
    """draws `values` left to right into the [h, w] panel, scaled symmetrically about zero to its height"""
    h, w = panel.shape
    if len(values) == 0:
        return
    top = max(float(np.abs(values).max()), 1e-30)
    cols = np.linspace(0, w - 1, len(values)).astype(int)
    rows = (h - 1) * (0.5 - 0.5 * np.asarray(values) / top)
    panel[h // 2] = 0.4
    panel[rows.astype(int), cols] = 1.0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--ms', type=float, default=600.0)
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--out', default='unipolar.png')
    args = ap.parse_args(argv)
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': args.ms})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 1.0)
    second_stimulus = sheet.millisecond_to_step(210)
    row, first, gap = n // 2, 5 * n // 8, max(2, 5 * n // 512)
    electrodes = [(row, first + k * gap) for k in range(4)]
    table = leads.point_table(n, n, z=2.0)
    with sheet.record_leads(electrodes, tables=table, every=args.every) as rec:      # weighted by the phase field
        for tick in sheet.run():
            if tick == second_stimulus:
                sheet.fire_op('s2')
        uni = rec.traces()
        bip = rec.bipolar([(0, 1), (1, 2), (2, 3)])
        t = rec.times_ms()
    if len(t) == 0:
        print('no sample was taken (--ms shorter than --every ticks)')
        return None
    print('%d samples up to %.1f ms; unipolar |phi| up to %.4g, bipolar up to %.4g' % (len(t), t[-1], np.abs(uni).max(), np.abs(bip).max()))
    h, w = 64, max(256, min(len(t), 1024))
    traces = [uni[:, e] for e in range(4)] + [bip[:, k] for k in range(3)]
    frame = np.full((len(traces) * (h + 1) - 1, w), 0.25, np.float32)
    for k, v in enumerate(traces):
        if k:
            frame[k * (h + 1) - 1] = 0.0
        curve(frame[k * (h + 1):k * (h + 1) + h], v)
    screen = Screen(frame.shape[0], frame.shape[1], 'unipolar 0-3 (top), bipolar 0-1, 1-2, 2-3 (bottom)')
    screen.imshow(frame)
    screen.save(args.out)
    print('traces written to %s' % args.out)
    return uni, bip


if __name__ == '__main__':
    main()
