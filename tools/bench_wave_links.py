"""cost of the wave recorder's links (fib_tf_amd/waves.py links=True, csrc/record_kernels.inc wave_link_kernel and
wave_link_pack_kernel), on the model of tools/bench_waves.py — the same grids, protocol and conventions:

    python tools/bench_wave_links.py [--ticks K] [--configs fenton512] [--every 10] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it: a spiral), one JSON
line.  The device side is timed with HIP events on the handle's stream:
  sample_us[conn]         one sample with links under conn = 4 and 8: the median over 50 samples of each of the six kernels, each
                          bracketed by two events (fibhip_trace_begin / _end) — the four existing ones and the two new ones of
                          the SAME run —, their sum and the two new ones' share; beside it the sample's wave and link counts
  none_us_per_tick        K ticks in ONE call with no recorder (fibhip_time_steps), best of 3
  off_us_per_tick         the same K ticks with the recorder attached at --every, links off, best of 3
  links_us_per_tick       ... and with links on
  loss_percent            what the run with links loses against the run without a recorder / against the run with links off
  polling_us_per_tick     the alternative a host has without links: K ticks in series of --every, behind each a read of the label
                          plane (`labels()`, a synchronising H x W read-back) and the overlap count in NumPy (wall clock, best of 3)
One process; stops at the first failure.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_activation import CONFIGS, make  # noqa: E402

KERNELS = ('wave_label_kernel', 'wave_merge_kernel', 'wave_root_kernel', 'wave_reduce_kernel', 'wave_link_kernel', 'wave_link_pack_kernel')


def polling(m, st, ticks, every):
    """what a host does without links: the label plane after every sample, the pairs of consecutive planes counted in NumPy"""
    best = None
    for _ in range(3):
        with m.record_waves(every=every, capacity=ticks // every + 1) as rec:
            st.sync()
            before = None
            t0 = time.perf_counter()
            for _ in range(ticks // every):
                st.step(every)
                now = rec.labels()
                if before is not None:
                    both = (before >= 0) & (now >= 0)
                    np.unique(before[both].astype(np.int64) << 32 | now[both], return_counts=True)
                before = now
            st.sync()
            dt = (time.perf_counter() - t0) / (ticks // every * every) * 1e6
        best = dt if best is None else min(best, dt)
    return round(best, 3)


def one(name, ticks, every):
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

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'every': every, 'sample_us': {}, 'counts': {}, 'link_counts': {}}
    out['none_us_per_tick'] = per_tick()
    for conn in (4, 8):
        with m.record_waves(every=1, conn=conn, capacity=52, links=True) as rec:
            st.step(1)
            st.trace_begin()
            st.step(50)
            ev = st.trace_end()
            out['counts'][str(conn)] = rec.counts()[-1].tolist()
            out['link_counts'][str(conn)] = rec.link_counts()[-1].tolist()
        k = {nm: round(float(np.median([x['dur'] for x in ev if x['name'] == nm])), 2) for nm in KERNELS}
        k['sum'] = round(sum(k[nm] for nm in KERNELS), 2)
        k['links'] = round(k['wave_link_kernel'] + k['wave_link_pack_kernel'], 2)
        out['sample_us'][str(conn)] = k
    with m.record_waves(every=every, capacity=3 * (ticks // every) + 3) as rec:
        out['off_us_per_tick'] = per_tick()
    with m.record_waves(every=every, capacity=3 * (ticks // every) + 3, links=True) as rec:
        out['links_us_per_tick'] = per_tick()
        assert len(rec.links_truncated()) == 0
        out['links_per_sample_max'] = int(rec.link_counts()[:, 0].max())
    out['loss_percent'] = {'against_none': round(100.0 * (out['links_us_per_tick'] / out['none_us_per_tick'] - 1.0), 2),
                           'against_links_off': round(100.0 * (out['links_us_per_tick'] / out['off_us_per_tick'] - 1.0), 2)}
    out['none_again_us_per_tick'] = per_tick()
    out['polling_us_per_tick'] = polling(m, st, ticks, every)
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=400)
    ap.add_argument('--configs', default='fenton512')
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks, args.every)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
