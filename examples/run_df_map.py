#!/usr/bin/env python3
"""Dominant-frequency and regularity maps of the four-variable atrial model's S1-S2 spiral: a planar wave from the left edge
(S1), a second stimulus in the upper-left quadrant 210 ms later, and the broken end curling around the obstacle.  Every
`--every` ticks the potential is folded on the device into a per-cell Welch periodogram (fib_tf_amd/spectrum.py: no frame is
kept, nothing is read back while the run goes on); at the end the two maps come back and are written as greyscale PNGs through
the headless Screen: the dominant frequency scaled to [0, --fmax], and the regularity index (the share of the band's power
within one bin of the peak).

    python examples/run_df_map.py [--size N] [--ms T] [--every K] [--nfft N] [--fmin HZ] [--fmax HZ] [--out PREFIX]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.screen import Screen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ms', type=float, default=3000.0)
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--nfft', type=int, default=128)
    ap.add_argument('--fmin', type=float, default=2.0)
    ap.add_argument('--fmax', type=float, default=20.0)
    ap.add_argument('--out', default='df')
    args = ap.parse_args()
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': args.ms, 'dt_per_plot': 10})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define()
    sheet.add_pace_op('s2', 'luq', 1.0)
    second_stimulus = sheet.millisecond_to_step(210)
    with sheet.record_spectrum(every=args.every, nfft=args.nfft, fmin=args.fmin, fmax=args.fmax) as rec:
        for tick in sheet.run():
            if tick == second_stimulus:
                sheet.fire_op('s2')
        segments = rec.segments()
        if segments == 0:
            sys.exit('no segment of %d samples has ended after %g ms: run longer, or shorten --nfft or --every'
                     % (args.nfft, args.ms))
        df, regularity = rec.dominant_frequency(refine=True)
        freqs = rec.freqs()
    tissue = sheet.phase > 0.5
    print('%d segments of %d samples, %d bins from %.2f to %.2f Hz' % (segments, args.nfft, len(freqs), freqs[0], freqs[-1]))
    print('dominant frequency over the tissue: median %.2f Hz, 5 %% .. 95 %%: %.2f .. %.2f Hz; regularity: median %.2f'
          % (np.median(df[tissue]), np.percentile(df[tissue], 5), np.percentile(df[tissue], 95), np.median(regularity[tissue])))
    for name, image in (('dominant_frequency', df / args.fmax), ('regularity', regularity)):
        screen = Screen(n, n, name)
        screen.imshow(np.where(tissue, np.clip(np.nan_to_num(image), 0.0, 1.0), 0.0).astype(np.float32))
        path = '%s_%s.png' % (args.out, name)
        screen.save(path)
        print('%s written to %s' % (name.replace('_', ' '), path))


if __name__ == '__main__':
    main()
