"""cost of the stimulus program (fib_tf_amd/stimulus.py, csrc/record_kernels.inc stim_kernel) against fire_op in the loop body:

    python tools/bench_stimulus.py [--ticks K] [--configs fenton512,court1024] [--periods 300,10] [--out FILE]

A configuration is a model and the side of its square grid: fenton512, court1024, fenton96, ...

For each configuration one JSON line.  The protocols are an S1 train from 'left' every 300 ticks and a burst every 10 ticks.
Every figure is host wall time per tick over K ticks stepped ONE CALL PER TICK, as a driver loop steps, ended by a sync();
best of 3:
  none_us / none_again_us   no stimulus: before and after the other columns (their difference is the spread of the run)
  program_us[period]        the stimuli from a program on the device (attached before the clock starts)
  fire_op_us[period]        the same stimuli fired from the loop body: `if i % period == period - 1: model.fire_op('s1')`
  stim_kernel_us            the kernel alone, median of its HIP-event-bracketed launches (the 'left' rectangle with the whole
                            grid floored at min_v, fire_op's operation: every cell of the potential read and written once)
  pace_kernel_us            fire_op's kernel alone, the same way
One process; stops at the first failure.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fib_tf_amd.stimulus import s1_train  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_electrodes import wall  # noqa: E402

def parse_config(name):
    """'fenton512' -> ('fenton', 512)"""
    m = re.fullmatch(r'(fenton|court)(\d+)', name)
    if not m or int(m.group(2)) < 16:
        raise ValueError('a configuration is fenton<N> or court<N>, N >= 16 (got %r)' % name)
    return m.group(1), int(m.group(2))


def make(model, n):
    cfg = {'height': n, 'width': n, 'dt': 0.1, 'dt_per_plot': 10, 'duration': 1000}
    if model == 'court':
        from fib_tf_amd.court import Courtemanche
        m, v = Courtemanche(dict(cfg, diff=0.809)), 20.0
    else:
        from fib_tf_amd.fenton import Fenton4v
        m, v = Fenton4v(dict(cfg, diff=1.5)), 1.0
    m.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    m.define()
    m.add_pace_op('s1', 'left', v)
    return m, v


def one(name, ticks, periods):
    model, n = parse_config(name)
    m, v = make(model, n)
    st = m._stepper
    slow = (lambda i: m.fire_op('slow') if i % 10 == 0 else None) if model == 'court' else (lambda i: None)
    st.step(50)
    st.sync()

    def none(_=None):
        for i in range(ticks):
            slow(i)
            st.step(1)
        st.sync()

    def fired(period):
        def run():
            for i in range(ticks):
                slow(i)
                st.step(1)
                if i % period == period - 1:
                    m.fire_op('s1')
            st.sync()
        return run

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'none_us': wall(none, ticks), 'program_us': {}, 'fire_op_us': {}}
    for p in periods:
        out['program_us'][str(p)] = wall(none, ticks, after=lambda prog: prog.close(),
                                         before=lambda p=p: m.program_stimuli(s1_train('left', v, period=p, n=0, start_tick=p - 1)))
        out['fire_op_us'][str(p)] = wall(fired(p), ticks)
    out['none_again_us'] = wall(none, ticks)
    with m.program_stimuli(s1_train('left', v, period=1, n=0)):
        st.step(1)
        st.trace_begin()
        st.step(50)
        ev = st.trace_end()
    out['stim_kernel_us'] = round(float(np.median([e['dur'] for e in ev if e['name'] == 'stim_kernel'])), 2)
    st.trace_begin()
    for _ in range(50):
        m.fire_op('s1')
    ev = st.trace_end()
    out['pace_kernel_us'] = round(float(np.median([e['dur'] for e in ev if e['name'] == 'pace_kernel'])), 2)
    st.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=600)
    ap.add_argument('--configs', default='fenton512,court1024')
    ap.add_argument('--periods', default='300,10')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    periods = [int(s) for s in args.periods.split(',')]
    for name in args.configs.split(','):
        parse_config(name)
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks, periods)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')
    return lines


if __name__ == '__main__':
    main()
