"""cost of the trigger program (fib_tf_amd/triggers.py; csrc/record_kernels.inc sense_kernel, trigger_kernel, stim_gated_kernel)
against the polling loop it replaces:

    python tools/bench_triggers.py [--ticks K] [--configs fenton512,court1024] [--out FILE]

A configuration is a model and the side of its square grid: fenton512, court1024, fenton96, ...

For each configuration one JSON line.  Every figure is host wall time per tick over K ticks stepped ONE CALL PER TICK, as a
driver loop steps, ended by a sync(); best of 3:
  none_us / none_again_us   no program: before and after the other columns (their difference is the spread of the run)
  idle_us[every]            a program whose rule never detects, every = 1 and every = 10: sense and decide alone
  waveback_us               s2_on_waveback on a probe in the middle of the sheet, every = 10
  polling_us                the loop it replaces: image() read back every 10th tick, the same decision on the host, fire_op
  electrode_us              an electrode recorder over the probe at every = 10: the yardstick, the launch cutting is the same
One process; stops at the first failure.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fib_tf_amd.triggers import Sensor, Trigger, s2_on_waveback  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_electrodes import wall  # noqa: E402
from bench_stimulus import make, parse_config  # noqa: E402


def one(name, ticks):
    model, n = parse_config(name)
    m, v = make(model, n)
    st = m._stepper
    m.add_pace_op('s2', 'luq', v)
    slow = (lambda i: m.fire_op('slow') if i % 10 == 0 else None) if model == 'court' else (lambda i: None)
    st.step(50)
    st.sync()
    rest = float(m.min_v)
    level = rest + 0.25 * (v - rest)
    probe = (n // 2 - 4, n // 2 + 4, n // 8, n // 8 + 8)
    mask = np.zeros((n, n), bool)
    mask[probe[0]:probe[1], probe[2]:probe[3]] = True

    def none(_=None):
        for i in range(ticks):
            slow(i)
            st.step(1)
        st.sync()

    def polling():
        lo, span = m._frame_levels()
        was, fired = None, False
        for i in range(ticks):
            slow(i)
            st.step(1)
            if i % 10 == 9 and not fired:
                now = bool((m.image()[mask] > (level - lo) / span).any())
                if was and not now:
                    m.fire_op('s2')
                    fired = True
                was = now
        st.sync()

    idle = [Trigger(Sensor(probe, v + 10.0 * abs(v - rest)), site='luq', v=v)]
    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'none_us': wall(none, ticks), 'idle_us': {}}
    for every in (1, 10):
        out['idle_us'][str(every)] = wall(none, ticks, after=lambda p: p.close(),
                                          before=lambda e=every: m.trigger_stimuli(idle, every=e, capacity=ticks // e + 1))
    out['waveback_us'] = wall(none, ticks, after=lambda p: p.close(),
                              before=lambda: m.trigger_stimuli(s2_on_waveback(probe, 'luq', v, level=level), every=10, capacity=ticks // 10 + 1))
    out['polling_us'] = wall(polling, ticks)
    out['electrode_us'] = wall(none, ticks, after=lambda r: r.close(),
                               before=lambda: m.record_electrodes([mask.astype(np.float32)], every=10, capacity=ticks // 10 + 1))
    out['none_again_us'] = wall(none, ticks)
    st.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=600)
    ap.add_argument('--configs', default='fenton512,court1024')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    for name in args.configs.split(','):
        parse_config(name)
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')
    return lines


if __name__ == '__main__':
    main()
