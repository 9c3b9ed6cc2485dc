#!/usr/bin/env python3
"""An S1-S2 protocol run entirely on the device: a train of planar S1 waves from the left edge of a Fenton 4v sheet with a
hole, then ONE premature S2 from a disc beside the hole, timed into the tail of the last S1 wave.  The loop body fires nothing:
the whole protocol is a stimulus program (fib_tf_amd/stimulus.py) the library applies tick by tick, and the spiral tips and the
excited fraction of the tissue are recorded on the device beside it (fib_tf_amd/tips.py, fib_tf_amd/stats.py).

    python examples/run_s1s2.py [--size N] [--s1-ms T] [--n-s1 K] [--s2-ms T] [--ms T]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fib_tf_amd.fenton import Fenton4v
from fib_tf_amd.stimulus import s1s2


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--s1-ms', type=float, default=300.0, help='S1 cycle length')
    ap.add_argument('--n-s1', type=int, default=3)
    ap.add_argument('--s2-ms', type=float, default=210.0, help='coupling interval: S2 this long after the last S1')
    ap.add_argument('--ms', type=float, default=1500.0)
    ap.add_argument('--every', type=int, default=10)
    args = ap.parse_args(argv)
    n = args.size
    sheet = Fenton4v({'width': n, 'height': n, 'dt': 0.1, 'diff': 1.5, 'duration': args.ms, 'dt_per_plot': 10})
    sheet.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    sheet.define(s1=False)                       # no wave from define(): the program's first S1 follows tick 0
    # S1 as fire_op would fire it (the whole sheet floored at min_v); S2 from a disc next to the hole, the rest untouched
    disc = ('disc', n // 2, n // 2 - 45 * n / 512.0 - n / 16.0, n / 16.0)
    s1, _ = s1s2('left', 1.0, s1_ms=args.s1_ms, n_s1=args.n_s1, s2_ms=args.s2_ms)
    _, s2 = s1s2('left', 1.0, s1_ms=args.s1_ms, n_s1=args.n_s1, s2_ms=args.s2_ms, s2_site=disc, floor=None)
    protocol = [s1, s2]
    with sheet.program_stimuli(protocol) as prog, sheet.record_tips(every=args.every) as tips, \
            sheet.record_stats([('U', 'frac_above', 0.5), ('U', 'nonfinite')], every=args.every) as stats:
        for tick in sheet.run():
            pass
        stats.check_finite()
        counts = tips.counts()
        t = stats.table()
        s2_tick = prog.entries[1]['first']
        print('%d stimuli applied (%d S1 + the S2 after tick %d)' % (prog.applied(), args.n_s1, s2_tick))
    after = counts[(s2_tick + 1) // args.every:]          # the samples taken after the S2
    print('excited fraction %.3f .. %.3f; tips after the S2: %s' % (t['U_frac_above'].min(), t['U_frac_above'].max(),
                                                                    'none' if not len(after) or not after[:, 2].any()
                                                                    else 'up to %d at once, %d at the end' % (after[:, 2].max(), after[-1, 2])))
    return prog.entries, t, counts


if __name__ == '__main__':
    main()
