#!/usr/bin/env python3
"""The movie, the electrogram and the rotors of one run, all recorded on the device: the four-variable atrial model's S1-S2
spiral of examples/run_tips.py (a planar wave from the left edge, a second stimulus in the upper-left quadrant 210 ms later,
the broken end curling around the obstacle) with three recorders attached to the same handle —

  * frames of image() * phase every `--every` ticks at run(im)'s own cadence (fib_tf_amd/frames.py), as 8-bit grey under a
    2 x 2 mean unless --full,
  * two Gaussian electrodes once per millisecond (fib_tf_amd/egm.py),
  * the spiral tips every second tick (fib_tf_amd/tips.py).

Nothing is read back while the model runs; between two samples of any of the three the handle keeps its multi-tick launches.
`cube.npy` is written once at the end (replay it with `python -m fib_tf_amd.playcube cube.npy`).

    python examples/run_movie.py [--size N] [--ms T] [--every K] [--full] [--out cube]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd import egm, tips
from fib_tf_amd.fenton import Fenton4v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ms', type=float, default=1000.0)
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--full', action='store_true', help='float32 frames at full resolution (what the reference drivers keep)')
    ap.add_argument('--out', default='cube')
    args = ap.parse_args()
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': args.ms, 'dt_per_plot': 10})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 1.0)
    second_stimulus = sheet.millisecond_to_step(210)
    shape = dict(block=(1, 1), fmt='float32') if args.full else dict(block=(2, 2), fmt='uint8')
    masks = [egm.create_mask(sheet, n * 0.6 + 15, n // 2, 5), egm.create_mask(sheet, n * 0.6 - 15, n // 2, 5)]
    with sheet.record_frames(every=args.every, first=1, **shape) as movie, \
            sheet.record_electrodes(masks, every=1) as electrodes, \
            sheet.record_tips(every=2) as rotors:
        for tick in sheet.run():
            if tick == second_stimulus:
                sheet.fire_op('s2')
        movie.save(args.out)
        frames, shape_px = movie.count(), movie.shape
        traces = electrodes.traces()
        paths = tips.link(rotors.tips(), 6.0)
        stats = sheet._stepper.launch_stats()
    print('%d frames of %d x %d %s written to %s.npy' % (frames, shape_px[0], shape_px[1], movie.dtype, args.out))
    print('%d electrogram samples, swing %.3f / %.3f' % (len(traces), float(np.ptp(traces[:, 0])), float(np.ptp(traces[:, 1]))))
    print('%d rotor trajectories, the longest %d samples' % (len(paths), max([len(p.points) for p in paths], default=0)))
    print('%d ticks in %d launches (%d of them multi-tick launches of %d ticks in all)'
          % (stats['ticks'], stats['launches'], stats['mt_launches'], stats['mt_ticks']))


if __name__ == '__main__':
    main()
