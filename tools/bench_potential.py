"""cost of the potential-map recorder (fib_tf_amd/potential.py, csrc/record_kernels.inc pmap_source_kernel, pmap_conv_kernel,
pmap_summary_kernel):

    python tools/bench_potential.py [--ticks K] [--configs fenton512] [--radii 4,16,32] [--steps 1,4] [--every 10] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it), one JSON line.
Everything is timed with HIP events on the handle's stream:
  sample_us[R/step]       one sample of the full window at radius R and step (step, step), a point electrode's table, the phase
                          field as the weight: the median over 20 samples of pmap_source_kernel and pmap_conv_kernel, each
                          bracketed by two events (fibhip_trace_begin / _end), and their sum; `summary` is pmap_summary_kernel
                          over those 20 samples
  leads64_sample_us       the lead recorder's two kernels for 64 leads on the same state, for comparison
  none_us_per_tick        K ticks in ONE call with no recorder (fibhip_time_steps), best of 3
  every_us_per_tick[..]   the same K ticks with the recorder attached at --every, best of 3
  loss_percent[..]        what the run with the recorder loses against the run without
One process; stops at the first failure.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fib_tf_amd import leads, potential  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_activation import CONFIGS, make  # noqa: E402
from bench_leads import line_of  # noqa: E402

KERNELS = ('pmap_source_kernel', 'pmap_conv_kernel')
SAMPLES = 20


def median_us(events, name):
    return round(float(np.median([x['dur'] for x in events if x['name'].split('<')[0] == name])), 2)


def one(name, ticks, radii, steps, every):
    model, n = CONFIGS[name]
    m = make(model, n)
    st = m._stepper
    s2 = m.millisecond_to_step(210)
    st.step(s2)
    m.fire_op('s2')
    st.step(20)
    st.sync()

    def per_tick():
        return round(min(st.time_steps(ticks)[0] for _ in range(3)) / ticks * 1e3, 3)

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'every': every, 'sample_us': {}, 'every_us_per_tick': {}, 'loss_percent': {}}
    out['none_us_per_tick'] = per_tick()
    with m.record_leads(line_of(n, 64), tables=leads.point_table(n, n, 2.0), every=1, capacity=SAMPLES + 2):
        st.step(1)
        st.trace_begin()
        st.step(SAMPLES)
        ev = st.trace_end()
    out['leads64_sample_us'] = round(median_us(ev, 'lead_kernel') + median_us(ev, 'lead_combine_kernel'), 2)
    for R in radii:
        tab = potential.truncated_table(R, 2.0)
        for s in steps:
            key = 'R%d/step%d' % (R, s)
            with m.record_potential_map(tab, every=1, step=(s, s), max_samples=SAMPLES + 2) as rec:
                st.step(1)
                st.trace_begin()
                st.step(SAMPLES)
                ev = st.trace_end()
                st.trace_begin()
                rec.summary(1, SAMPLES)
                sv = st.trace_end()
                sites = rec.shape
            k = {nm: median_us(ev, nm) for nm in KERNELS}
            k['sum'] = round(sum(k.values()), 2)
            k['summary'] = median_us(sv, 'pmap_summary_kernel')
            k['sites'] = list(sites)
            k['gfma_per_s'] = round(sites[0] * sites[1] * (2 * R + 1) ** 2 / k['pmap_conv_kernel'] * 1e-3, 1)
            out['sample_us'][key] = k
            with m.record_potential_map(tab, every=every, step=(s, s), max_samples=3 * (ticks // every) + 3) as rec:
                out['every_us_per_tick'][key] = per_tick()
                assert np.all(np.isfinite(rec.raw(0, 2)))
            out['loss_percent'][key] = round(100.0 * (out['every_us_per_tick'][key] / out['none_us_per_tick'] - 1.0), 2)
    out['none_again_us_per_tick'] = per_tick()
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=400)
    ap.add_argument('--configs', default='fenton512')
    ap.add_argument('--radii', default='4,16,32')
    ap.add_argument('--steps', default='1,4')
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks, [int(x) for x in args.radii.split(',')], [int(x) for x in args.steps.split(',')], args.every)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
