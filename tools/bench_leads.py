"""cost of the lead recorder (fib_tf_amd/leads.py, csrc/record_kernels.inc lead_kernel, lead_combine_kernel):

    python tools/bench_leads.py [--ticks K] [--configs fenton512] [--leads 1,16,64] [--every 10] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it), one JSON line.
Everything is timed with HIP events on the handle's stream:
  sample_us[E]            one sample of E leads on a line through the middle, a point electrode's table, the phase field as the
                          weight: the median over 50 samples of lead_kernel and lead_combine_kernel, each bracketed by two
                          events (fibhip_trace_begin / _end), and their sum
  none_us_per_tick        K ticks in ONE call with no recorder (fibhip_time_steps), best of 3
  every_us_per_tick[E]    the same K ticks with the recorder attached at --every, best of 3
  loss_percent[E]         what the run with the recorder loses against the run without
One process; stops at the first failure.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fib_tf_amd import leads  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_activation import CONFIGS, make  # noqa: E402

KERNELS = ('lead_kernel', 'lead_combine_kernel')


def line_of(n, count):
    """`count` electrodes on the middle row, evenly spread over the middle half of the columns"""
    return [(n // 2, int(c)) for c in np.linspace(n // 4, 3 * n // 4, count).astype(int)]


def one(name, ticks, counts, every):
    model, n = CONFIGS[name]
    m = make(model, n)
    st = m._stepper
    s2 = m.millisecond_to_step(210)
    st.step(s2)
    m.fire_op('s2')
    st.step(20)
    st.sync()
    tab = leads.point_table(n, n, 2.0)

    def per_tick():
        return round(min(st.time_steps(ticks)[0] for _ in range(3)) / ticks * 1e3, 3)

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'every': every, 'sample_us': {}, 'every_us_per_tick': {}, 'loss_percent': {}}
    out['none_us_per_tick'] = per_tick()
    for e in counts:
        cells = line_of(n, e)
        with m.record_leads(cells, tables=tab, every=1, capacity=52):
            st.step(1)
            st.trace_begin()
            st.step(50)
            ev = st.trace_end()
        k = {nm: round(float(np.median([x['dur'] for x in ev if x['name'] == nm])), 2) for nm in KERNELS}
        k['sum'] = round(k['lead_kernel'] + k['lead_combine_kernel'], 2)
        out['sample_us'][str(e)] = k
        with m.record_leads(cells, tables=tab, every=every, capacity=3 * (ticks // every) + 3) as rec:
            out['every_us_per_tick'][str(e)] = per_tick()
            assert np.all(np.isfinite(rec.raw()))
        out['loss_percent'][str(e)] = round(100.0 * (out['every_us_per_tick'][str(e)] / out['none_us_per_tick'] - 1.0), 2)
    out['none_again_us_per_tick'] = per_tick()
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=400)
    ap.add_argument('--configs', default='fenton512')
    ap.add_argument('--leads', default='1,16,64')
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks, [int(x) for x in args.leads.split(',')], args.every)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
