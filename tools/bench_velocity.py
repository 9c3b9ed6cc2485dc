"""cost of the velocity fit (fib_tf_amd/velocity.py, csrc/record_kernels.inc velocity_fit_kernel) against what it replaces:

    python tools/bench_velocity.py [--sizes 512,2048] [--depth 8] [--radii 2,4] [--host-sizes 512] [--out FILE]

For each size n a Fenton sheet of n x n cells is paced from the left every 300 ticks until every ring of `depth` beats is full
(a sample every 10 ticks, full resolution); then, one JSON line per size:
  device_us[R]     BeatRecorder's device call for one beat — fibhip_beats_velocity: the launch and its four read-backs —, wall,
                   best of 3
  kernel_us[R]     velocity_fit_kernel alone, its HIP-event-bracketed launch (fibhip_trace_begin/_end), best of 3
  ring_mib,        the alternative's first step: the ring read back (fibhip_beats_read: three planes of `depth` slots, the
  readback_us      counts and the live peak), wall, best of 3
  host_us[R]       the alternative's second step: the NumPy restatement of the definition (tests/velocity_ref.py) on the ring
                   read back, once; null for the sizes that are not in --host-sizes (minutes at 2048 x 2048)
  fitted[R]        (structural) the pixels with a fit, of n * n
Nothing is asserted on the times.  One process; stops at the first failure.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from fib_tf_amd import velocity as vel  # noqa: E402
from fib_tf_amd.fenton import Fenton4v  # noqa: E402
from fib_tf_amd.stimulus import Stimulus  # noqa: E402

PERIOD, EVERY, MAX_DT = 300, 10, 20.0


def best_of(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return round(best * 1e6, 1), out


def one(n, depth, radii, host):
    import velocity_ref
    ticks = PERIOD * depth + n // 3 + 60                      # the last wave has crossed the sheet (it runs about 3.3 cells per ms)
    m = Fenton4v({'height': n, 'width': n, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': ticks})
    m.define(s1=False)
    st = m._stepper
    out = {'size': n, 'depth': depth, 'ticks': ticks, 'device_us': {}, 'kernel_us': {}, 'host_us': {}, 'fitted': {}}
    with m.program_stimuli([Stimulus((0, n, 0, 6), 1.0, at_tick=0, period=PERIOD, count=0, floor=0.0)]):
        with m.record_beats(every=EVERY, depth=depth) as rec:
            st.step(ticks)
            st.sync()
            out['readback_us'], raw = best_of(rec.raw)
            out['ring_mib'] = round(sum(a.nbytes for a in raw) / 2.0 ** 20, 1)
            t_up, count = raw[0], raw[3]
            out['beats_per_pixel'] = [int(count.min()), int(count.max())]
            for R in radii:
                mc = vel.default_min_cells(R)
                out['device_us'][str(R)], maps = best_of(lambda: st.beats_velocity(0, R, MAX_DT, mc))
                out['fitted'][str(R)] = int(np.isfinite(maps[1]).sum())
                durs = []
                for _ in range(3):
                    st.trace_begin()
                    st.beats_velocity(0, R, MAX_DT, mc)
                    durs += [e['dur'] for e in st.trace_end() if e['name'] == 'velocity_fit_kernel']
                out['kernel_us'][str(R)] = round(float(min(durs)), 2)
                if host:
                    t0 = time.perf_counter()
                    want = velocity_ref.fit(t_up, count, back=0, radius=R, max_dt=MAX_DT, min_cells=mc)
                    out['host_us'][str(R)] = round((time.perf_counter() - t0) * 1e6, 1)
                    assert all(velocity_ref.same(g, w) for g, w in zip(maps, want)), 'the device differs from the restatement'
                else:
                    out['host_us'][str(R)] = None
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='512,2048')
    ap.add_argument('--depth', type=int, default=8)
    ap.add_argument('--radii', default='2,4')
    ap.add_argument('--host-sizes', default='512')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    radii = [int(r) for r in args.radii.split(',')]
    host = {int(s) for s in args.host_sizes.split(',') if s}
    lines = []
    for n in (int(s) for s in args.sizes.split(',')):
        r = one(n, args.depth, radii, n in host)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
