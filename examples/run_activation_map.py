#!/usr/bin/env python3
"""Activation maps of spiral-wave re-entry in the four-variable atrial model: the S1-S2 protocol of run_fenton.py (512 x 512
sheet, circular obstacle, S1 from the left edge, S2 in the upper-left quadrant at 210 ms) with an activation recorder
attached, so that every cell's upstroke times and action-potential duration are kept on the device — nothing is read back
until the end.  Writes

    isochrones.png     the last activation time of every cell, grey = time within the last `--band` ms, with black
                       isochrone lines every `--step` ms
    cycle_length.png   last_up - prev_up, scaled to [--cl-min, --cl-max] ms

and prints the cycle length at the pixel run() watches ([20, W//2]) and the median APD90.

    python examples/run_activation_map.py [--size N] [--ms T] [--out DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.screen import write_png_grey


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ms', type=float, default=1000.0)
    ap.add_argument('--out', default='.')
    ap.add_argument('--band', type=float, default=200.0, help='ms of activation history the grey scale spans')
    ap.add_argument('--step', type=float, default=10.0, help='ms between isochrone lines')
    ap.add_argument('--cl-min', type=float, default=60.0)
    ap.add_argument('--cl-max', type=float, default=300.0)
    args = ap.parse_args()
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': args.ms, 'dt_per_plot': 10})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 1.0)
    second_stimulus = sheet.millisecond_to_step(210)

    with sheet.record_activation() as rec:
        for tick in sheet.run():
            if tick == second_stimulus:
                sheet.fire_op('s2')
        maps = rec.maps()

    last, prev, apd = maps['last_up'], maps['prev_up'], maps['apd']
    tissue = sheet.phase > 0.5
    t_end = float(np.nanmax(last))
    grey = np.clip((last - (t_end - args.band)) / args.band, 0.0, 1.0)
    lines = np.zeros_like(tissue)
    band = np.floor(np.nan_to_num(last, nan=-1.0) / args.step)
    lines[:, 1:] |= band[:, 1:] != band[:, :-1]
    lines[1:, :] |= band[1:, :] != band[:-1, :]
    img = np.where(np.isnan(last) | ~tissue, 0.0, np.where(lines, 0.0, 0.25 + 0.75 * grey))
    os.makedirs(args.out, exist_ok=True)
    write_png_grey(os.path.join(args.out, 'isochrones.png'), img)
    cl = last - prev
    write_png_grey(os.path.join(args.out, 'cycle_length.png'),
                   np.where(np.isnan(cl) | ~tissue, 0.0, (cl - args.cl_min) / (args.cl_max - args.cl_min)))
    print('upstrokes at the watched pixel [20, %d]: %d, last cycle length %.2f ms' % (n // 2, maps['count'][20, n // 2],
                                                                                        cl[20, n // 2]))
    print('median APD90 over the tissue: %.1f ms; cells activated: %d of %d' % (
        np.nanmedian(np.where(tissue, apd, np.nan)), int((maps['count'] > 0).sum()), n * n))


if __name__ == '__main__':
    main()
