#!/usr/bin/env python3
"""Excited fraction and mean intracellular sodium of the Courtemanche atrial model over an S1-S2 run: a planar wave from the left
edge (S1), a second stimulus in the upper-left quadrant 300 ms later.  Both curves are whole-tissue statistics taken on the
device every `--every` ticks (fib_tf_amd/stats.py: nothing is read back between the samples) and drawn, one above the
other, into a greyscale PNG through the headless Screen.

    python examples/run_stats.py [--size N] [--ms T] [--every K] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.court import Courtemanche
from fib_tf_amd.screen import Screen


def curve(panel, values, lo, hi):
    """draws `values` left to right into the [h, w] panel, scaled from [lo, hi] to its height"""
    h, w = panel.shape
    if len(values) == 0:
        return
    cols = np.linspace(0, w - 1, len(values)).astype(int)
    rows = (h - 1) - np.clip((np.asarray(values) - lo) / max(hi - lo, 1e-30), 0.0, 1.0) * (h - 1)
    panel[rows.astype(int), cols] = 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--ms', type=float, default=600.0)
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--out', default='stats.png')
    args = ap.parse_args()
    n = args.size
    sheet = Courtemanche({'width': n, 'height': n, 'dt': 0.1, 'diff': 0.809, 'duration': args.ms, 'dt_per_plot': 10})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 10.0)
    second_stimulus = sheet.millisecond_to_step(300)
    columns = [('V', 'frac_above', -55.0), ('_Na_i_', 'mean'), ('V', 'min'), ('V', 'max'), ('V', 'nonfinite')]
    with sheet.record_stats(columns, every=args.every) as rec:       # means weighted by the phase field, the rest under phase > 0.5
        for tick in sheet.run():
            if tick % 10 == 0:
                sheet.fire_op('slow')
            if tick == second_stimulus:
                sheet.fire_op('s2')
        rec.check_finite()
        t = rec.table()
    print('%d samples; excited fraction %.3f .. %.3f, mean Na_i %.5f .. %.5f mM, V in [%.1f, %.1f] mV'
          % (len(t), t['V_frac_above'].min(), t['V_frac_above'].max(), t['_Na_i__mean'].min(), t['_Na_i__mean'].max(),
             t['V_min'].min(), t['V_max'].max()))
    h, w = 128, max(256, min(len(t), 1024))
    frame = np.full((2 * h + 1, w), 0.25, np.float32)
    frame[h] = 0.0
    curve(frame[:h], t['V_frac_above'], 0.0, 1.0)
    curve(frame[h + 1:], t['_Na_i__mean'], t['_Na_i__mean'].min(), t['_Na_i__mean'].max())
    screen = Screen(frame.shape[0], frame.shape[1], 'excited fraction (top), mean Na_i (bottom)')
    screen.imshow(frame)
    screen.save(args.out)
    print('curves written to %s' % args.out)


if __name__ == '__main__':
    main()
