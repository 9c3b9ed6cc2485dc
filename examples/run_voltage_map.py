#!/usr/bin/env python3
"""A voltage map before and after an ablation: the four-variable atrial model paced from the left edge with a potential-map
recorder attached — the unipolar electrogram at every site of a lattice, formed on the device (fib_tf_amd/potential.py) — and an
activation recorder beside it.  After the first beat a vertical line is burnt into the sheet (`ablate`), the sheet is paced again
and mapped again.  Printed: the peak-to-peak amplitude of the electrograms before and after, on the line and off it, and how far
the electrogram's activation time (steepest negative slope) lies from the membrane's (`first_up`).  Written: the two voltage
maps and the map of electrogram LAT minus first_up, side by side.

    python examples/run_voltage_map.py [--size N] [--ms T] [--every K] [--radius R] [--step S] [--height Z] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd import potential
from fib_tf_amd.fenton import Fenton4v


def beat(sheet, ticks, table, every, step):
    """`ticks` ticks with the two recorders attached -> (voltage map, electrogram LAT in ms, first_up in ms at the sites)"""
    st = sheet._stepper
    with sheet.record_potential_map(table, every=every, step=(step, step), max_samples=ticks // every + 1) as rec, \
            sheet.record_activation() as act:
        st.step(ticks)
        volt, lat = rec.voltage(), rec.lat_ms()
        rows, cols = rec.sites()
        first_up = act.maps()['first_up'][np.ix_(rows, cols)].astype(np.float64)
    return volt, lat, first_up


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ms', type=float, default=1600.0, help='both beats together')
    ap.add_argument('--every', type=int, default=2)
    ap.add_argument('--radius', type=int, default=16)
    ap.add_argument('--step', type=int, default=4)
    ap.add_argument('--height', type=float, default=2.0, help='of the electrode above the sheet, in cells')
    ap.add_argument('--out', default='voltage_map.png')
    ap.add_argument('--no-plot', action='store_true')
    args = ap.parse_args(argv)
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': args.ms, 'dt_per_plot': 10})
    sheet.add_hole_to_phase_field(3 * n // 4, n // 4, 12 * n / 512.0)
    sheet.define()                                            # (the S1 wave starts at the left edge)
    sheet.add_pace_op('again', 'left', 1.0)
    table = potential.truncated_table(args.radius, args.height)
    ticks = sheet.millisecond_to_step(args.ms) // 2
    before, lat, first_up = beat(sheet, ticks, table, args.every, args.step)
    col = n // 2
    sheet.ablate(('line', n // 8, col, 7 * n // 8, col, max(1.5, 3 * n / 512.0)))
    sheet.fire_op('again')
    after, _, _ = beat(sheet, ticks, table, args.every, args.step)
    dlat = lat - first_up
    on_line = np.zeros(before.shape, bool)
    on_line[(n // 8) // args.step + 1:(7 * n // 8) // args.step, col // args.step] = True
    print('%d x %d sites, radius %d, a sample every %d ticks' % (before.shape + (args.radius, args.every)))
    for name, v in (('before', before), ('after', after)):
        print('  voltage %-6s on the line: median %.4g   off it: median %.4g' % (name, np.median(v[on_line]), np.median(v[~on_line])))
    seen = np.isfinite(dlat)
    print('  electrogram LAT minus first_up: median %.2f ms, 5th .. 95th percentile %.2f .. %.2f ms over %d sites'
          % ((np.median(dlat[seen]),) + tuple(np.percentile(dlat[seen], (5, 95))) + (int(seen.sum()),)) if seen.any() else '  no site was activated')
    if not args.no_plot:
        from fib_tf_amd.screen import Screen
        top = max(float(before.max()), float(after.max()), 1e-30)
        span = max(float(np.abs(dlat[seen]).max()), 1e-30) if seen.any() else 1.0
        picture = np.hstack([before / top, after / top, np.where(seen, 0.5 + 0.5 * dlat / span, 0.0)]).astype(np.float32)
        screen = Screen(picture.shape[0], picture.shape[1], 'voltage map')
        screen.imshow(picture)
        screen.save(args.out)
        print('the voltage map before, after, and LAT minus first_up written to %s' % args.out)
    return before, after, dlat


if __name__ == '__main__':
    main()
