#!/usr/bin/env python3
"""Cross-field spiral induction with the S2 timed from the waveback, on the device: define() starts a planar S1 wave from the
left edge; a probe in the middle of the sheet watches it pass, and when the wave's back has left the probe — the cells there
fall back below the level — the library fires ONE S2 over the upper left quadrant `--delay-ms` later.  No tick is tuned by
hand and the host reads nothing back while it runs: the same script works for Fenton 4v and Beeler-Reuter, for any `diff` and
any grid (fib_tf_amd/triggers.py; the tips are recorded on the device beside it, fib_tf_amd/tips.py).

    python examples/run_closed_loop.py [--model fenton|br] [--size N] [--delay-ms T] [--ms T] [--every K]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.triggers import s2_on_waveback


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', choices=('fenton', 'br'), default='fenton')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--delay-ms', type=float, default=10.0, help='S2 this long after the waveback has passed the probe')
    ap.add_argument('--ms', type=float, default=800.0)
    ap.add_argument('--every', type=int, default=10)
    args = ap.parse_args(argv)
    n = args.size
    cfg = {'width': n, 'height': n, 'dt': 0.1, 'duration': args.ms, 'dt_per_plot': 10}
    if args.model == 'br':
        from fib_tf_amd.br import BeelerReuter
        sheet, v = BeelerReuter(dict(cfg, diff=0.809, cheby=True, skip=False)), 10.0
    else:
        from fib_tf_amd.fenton import Fenton4v
        sheet, v = Fenton4v(dict(cfg, diff=1.5)), 1.0
    sheet.define()                               # the S1 wave from the left edge
    # the level: a quarter of the way from rest to the stimulus value — above it a cell is excited, whatever the model's units
    level = float(sheet.min_v) + 0.25 * (v - float(sheet.min_v))
    probe = (n // 2 - 4, n // 2 + 4, n // 2 - 4, n // 2 + 4)
    rules = s2_on_waveback(probe, 'luq', v, level=level, delay_ms=args.delay_ms, floor=None)
    with sheet.trigger_stimuli(rules, every=args.every) as prog, sheet.record_tips(every=args.every) as tips:
        for tick in sheet.run():
            pass
        fired, counts = prog.fired(), tips.counts()
    if not fired:
        print('the waveback never passed the probe within %g ms: no S2' % args.ms)
        return fired, counts
    s2_tick = fired[0][0]
    after = counts[(s2_tick + 1) // args.every:]
    print('S2 after tick %d (%.1f ms), %g ms behind the waveback at the probe; tips after it: %s'
          % (s2_tick, (s2_tick + 1) * prog.tick_ms, args.delay_ms,
             'none' if not len(after) or not after[:, 2].any() else 'up to %d at once, %d at the end' % (after[:, 2].max(), after[-1, 2])))
    return fired, counts


if __name__ == '__main__':
    main()
