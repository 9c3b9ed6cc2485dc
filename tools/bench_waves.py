"""cost of the wave recorder (fib_tf_amd/waves.py, csrc/record_kernels.inc wave_label_kernel, wave_merge_kernel, wave_root_kernel,
wave_reduce_kernel):

    python tools/bench_waves.py [--ticks K] [--configs fenton512] [--every 10] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it: a spiral), one JSON
line.  The device side is timed with HIP events on the handle's stream:
  sample_us[conn]         one sample under conn = 4 and 8: the median over 50 samples of each of the four kernels, each bracketed
                          by two events (fibhip_trace_begin / _end), and their sum; beside it the sample's counts
  none_us_per_tick        K ticks in ONE call with no recorder (fibhip_time_steps), best of 3
  every_us_per_tick       the same K ticks with the recorder attached at --every, best of 3
  loss_percent            what the run with the recorder loses against the run without
  polling_us_per_tick     the alternative: K ticks in series of --every, behind each a get_state and scipy.ndimage.label on the
                          host (wall clock, best of 3; null without scipy)
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

KERNELS = ('wave_label_kernel', 'wave_merge_kernel', 'wave_root_kernel', 'wave_reduce_kernel')


def polling(m, st, ticks, every, level, mask):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    best = None
    for _ in range(3):
        st.sync()
        t0 = time.perf_counter()
        for _ in range(ticks // every):
            st.step(every)
            plane = (st.get_state(0) > level) & mask
            _, n = ndimage.label(plane)
        st.sync()
        dt = (time.perf_counter() - t0) / (ticks // every * every) * 1e6
        best = dt if best is None else min(best, dt)
    return round(best, 3)


def one(name, ticks, every):
    from fib_tf_amd import waves
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

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'every': every, 'sample_us': {}, 'counts': {}}
    out['none_us_per_tick'] = per_tick()
    for conn in (4, 8):
        with m.record_waves(every=1, conn=conn, capacity=52) as rec:
            st.step(1)
            st.trace_begin()
            st.step(50)
            ev = st.trace_end()
            out['counts'][str(conn)] = rec.counts()[-1].tolist()
        k = {nm: round(float(np.median([x['dur'] for x in ev if x['name'] == nm])), 2) for nm in KERNELS}
        k['sum'] = round(sum(k[nm] for nm in KERNELS), 2)
        out['sample_us'][str(conn)] = k
    with m.record_waves(every=every, capacity=3 * (ticks // every) + 3) as rec:
        out['every_us_per_tick'] = per_tick()
        level, mask = rec.level, rec.mask != 0
        assert rec.counts()[:, 0].min() >= 0
    out['loss_percent'] = round(100.0 * (out['every_us_per_tick'] / out['none_us_per_tick'] - 1.0), 2)
    out['none_again_us_per_tick'] = per_tick()
    out['polling_us_per_tick'] = polling(m, st, ticks, every, np.float32(level), mask)
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
