#!/usr/bin/env python3
"""Two-electrode electrogram of the Beeler-Reuter sheet with the electrodes on the device: 512 x 512, circular obstacle, S1
from the left edge, S2 in the upper-left quadrant at 300 ms, two Gaussian electrodes of radius 5 thirty pixels apart on the
middle row, one sample per millisecond.  The weighted sums are taken on the device behind the tick that ends each
millisecond and stay there until the run is over — no frame is read back.  Writes `test.dat` (one row per millisecond, one
column per electrode: the mean of image() * mask) and prints the activation delay between the electrodes.

    python examples/run_egm.py [--size N] [--ms T] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd import egm
from fib_tf_amd.br import BeelerReuter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ms', type=float, default=3000.0)
    ap.add_argument('--out', default='test.dat')
    args = ap.parse_args()
    n = args.size
    sheet = BeelerReuter({'width': n, 'height': n, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.0, 'duration': args.ms,
                          'skip': False, 'cheby': True})
    sheet.add_hole_to_phase_field(150 * n // 512, n // 2, 50 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 10.0)
    s2 = sheet.millisecond_to_step(300)
    x = 300 * n // 512
    m1, m2 = egm.create_mask(sheet, x + 15, n // 2, 5), egm.create_mask(sheet, x - 15, n // 2, 5)
    out = egm.record_on_device(sheet, m1, m2, on_tick=lambda i: sheet.fire_op('s2') if i == s2 else None)
    np.savetxt(args.out, out)
    print('%d samples of 2 electrodes written to %s' % (len(out), args.out))
    try:
        print('activation delay between the electrodes: %.2f ms' % egm.delay_ms(out))
    except ValueError as e:
        print('no delay: %s' % e)


if __name__ == '__main__':
    main()
