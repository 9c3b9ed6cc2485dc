#!/usr/bin/env python3
"""Anisotropic conduction in the four-variable atrial model: a sheet whose fibres rotate across it — along the columns at the
left edge, along the rows at the right edge — with an anisotropy ratio of `--ratio` (set_fibres; fib_tf_amd/tensor.py).  Two runs:

    fibres_isochrones.png   a point stimulus in the middle: the first activation time of every cell, grey = time, with black
                            isochrone lines every `--step` ms — ellipses whose long axis follows the local fibre
    fibres_spiral.png       S1 from the left edge, S2 in the upper-left quadrant at `--s2` ms: the potential at the end of the run,
                            a spiral on the anisotropic sheet

and prints the front's speed along and across the fibres near the stimulus, from the activation recorder's velocity fit.

    python examples/run_fibres.py [--size N] [--ratio R] [--ms T] [--s2 T2] [--out DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.screen import write_png_grey
from fib_tf_amd.stimulus import Stimulus
from fib_tf_amd.velocity import speed_of


def fibre_angle(n):
    """radians from the +column axis towards the +row axis: a quarter turn from the left edge to the right edge"""
    return np.broadcast_to(np.linspace(0.0, np.pi / 2, n)[None, :], (n, n))


def sheet(n, ratio, ms):
    m = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': ms, 'dt_per_plot': 10})
    m.set_fibres(fibre_angle(n), ratio)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ratio', type=float, default=3.0, help='longitudinal over transverse diffusion (up to 3 every weight is non-negative)')
    ap.add_argument('--ms', type=float, default=600.0, help='length of the S1-S2 run')
    ap.add_argument('--s2', type=float, default=210.0)
    ap.add_argument('--step', type=float, default=10.0, help='ms between isochrone lines')
    ap.add_argument('--out', default='.')
    args = ap.parse_args()
    n = args.size
    if n < 64 or args.ratio < 1.0:
        ap.error('size >= 64 and ratio >= 1')
    os.makedirs(args.out, exist_ok=True)

    # ---- a point stimulus: isochrones ----
    m = sheet(n, args.ratio, n / 2.0)
    m.define(s1=False)
    c = n // 2
    with m.program_stimuli([Stimulus(('disc', c, c, 3), 1.0, at_tick=0)]), m.record_activation() as rec:
        for _ in m.run():
            pass
        first = rec.maps()['first_up']
        fit = rec.velocity('first_up')
    t_end = float(np.nanmax(first))
    band = np.floor(np.nan_to_num(first, nan=-1.0) / args.step)
    lines = np.zeros(first.shape, bool)
    lines[:, 1:] |= band[:, 1:] != band[:, :-1]
    lines[1:, :] |= band[1:, :] != band[:-1, :]
    write_png_grey(os.path.join(args.out, 'fibres_isochrones.png'),
                   np.where(np.isnan(first), 0.0, np.where(lines, 0.0, 1.0 - 0.75 * first / max(t_end, 1e-6))))
    speed = speed_of(fit)
    th = float(fibre_angle(n)[c, c])                                      # the fibre through the stimulus site
    d = max(8, n // 16)
    along = (c + int(round(d * np.sin(th))), c + int(round(d * np.cos(th))))
    across = (c + int(round(d * np.cos(th))), c - int(round(d * np.sin(th))))
    print('front speed %d cells from the stimulus: %.3f cells per ms along the fibre, %.3f across it (ratio %.3f; sqrt(%g) = %.3f)'
          % (d, speed[along], speed[across], speed[along] / speed[across], args.ratio, args.ratio ** 0.5))

    # ---- S1-S2: a spiral ----
    m = sheet(n, args.ratio, args.ms)
    m.define()
    m.add_pace_op('s2', 'luq', 1.0)
    s2 = m.millisecond_to_step(args.s2)
    for tick in m.run():
        if tick == s2:
            m.fire_op('s2')
    write_png_grey(os.path.join(args.out, 'fibres_spiral.png'), np.clip(m.image(), 0.0, 1.0))
    print('wrote fibres_isochrones.png and fibres_spiral.png to %s' % os.path.abspath(args.out))


if __name__ == '__main__':
    main()
