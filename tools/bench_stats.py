"""cost of the statistics recorder (fib_tf_amd/stats.py, csrc/record_kernels.inc stats_kernel) against polling:

    python tools/bench_stats.py [--ticks K] [--configs court1024,fenton512] [--strides 1,10,100] [--out FILE]

For each configuration one JSON line.  The columns are the reference observer's (court_ultra.py:465-486, 504-509): the
phase-weighted means of two state arrays, the share of the tissue below a level, a finite check.  Every figure is host wall
time per tick over K ticks stepped ONE CALL PER TICK, as a driver loop steps, ended by the call that makes the result
visible; best of 3:
  none_us / none_again_us   no recorder, a sync() at the end: before and after the other columns
  device_us[stride]         StatsRecorder at that stride (attached before the clock starts), raw() at the end
  polled_us[stride]         what court_ultra.cl_observer and run_small do at that stride: the arrays read back whole,
                            np.average(..., weights=phase) of each and the share below the level
  stats_kernel_us, stats_combine_kernel_us   the kernels alone, median of their HIP-event-bracketed launches
  read_GBps                 the bytes stats_kernel must read (each array named once, the weight plane and the mask once per
                            array that needs them) over stats_kernel_us;  copy_GBps: fibhip_copy_bandwidth in the same run
One process; stops at the first failure.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fib_tf_amd import _lib  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_electrodes import wall  # noqa: E402

CONFIGS = {'court1024': ('court', 1024), 'court512': ('court', 512), 'fenton512': ('fenton', 512), 'fenton1024': ('fenton', 1024)}


def make(model, n):
    cfg = {'height': n, 'width': n, 'dt': 0.1, 'dt_per_plot': 10, 'duration': 1000}
    if model == 'court':
        from fib_tf_amd.court import Courtemanche
        m = Courtemanche(dict(cfg, diff=0.809))
        names, level = ('_Na_i_', '_f_Ca_'), -55.0
    else:
        from fib_tf_amd.fenton import Fenton4v
        m = Fenton4v(dict(cfg, diff=1.5))
        names, level = ('V', 'W'), 0.3
    m.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    m.define()
    pot = type(m).VAR_NAMES[0]
    columns = [(names[0], 'mean'), (names[1], 'mean'), (pot, 'frac_below', level), (pot, 'nonfinite')]
    return m, columns, names, level


def one(name, ticks, strides):
    model, n = CONFIGS[name]
    m, columns, names, level = make(model, n)
    st = m._stepper
    slow = (lambda i: m.fire_op('slow') if i % 10 == 0 else None) if model == 'court' else (lambda i: None)
    st.step(50)
    st.sync()
    phase = m.phase
    inside = phase > 1e-3
    lvl = np.float32(level)

    def none():
        for i in range(ticks):
            slow(i)
            st.step(1)
        st.sync()

    def device(rec):
        for i in range(ticks):
            slow(i)
            st.step(1)
        assert rec.raw().shape[1] == len(columns)

    def polled(stride):
        def run():
            rows = []
            for i in range(ticks):
                slow(i)
                st.step(1)
                if (i + 1) % stride == 0:
                    a = np.average(m._State[names[0]].eval(), weights=phase)
                    b = np.average(m._State[names[1]].eval(), weights=phase)
                    v = m._State[type(m).VAR_NAMES[0]].eval()
                    rows.append([a, b, np.sum(v[inside] < lvl) / np.sum(inside), np.count_nonzero(~np.isfinite(v))])
            st.sync()
        return run

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'none_us': wall(none, ticks), 'device_us': {}, 'polled_us': {}}
    for s in strides:
        out['device_us'][str(s)] = wall(device, ticks, after=lambda rec: rec.close(),
                                        before=lambda s=s: m.record_stats(columns, every=s, mask=inside, capacity=max(1, ticks // s)))
        out['polled_us'][str(s)] = wall(polled(s), ticks)
    out['none_again_us'] = wall(none, ticks)
    with m.record_stats(columns, every=1, mask=inside, capacity=64):
        st.step(1)
        st.trace_begin()
        st.step(50)
        ev = st.trace_end()
    for nm in ('stats_kernel', 'stats_combine_kernel'):
        out[nm + '_us'] = round(float(np.median([e['dur'] for e in ev if e['name'] == nm])), 2)
    # three distinct arrays: two read with the weight plane (4 + 4 bytes a cell), one with the mask (4 + 1)
    nbytes = n * n * (2 * 8 + 5)
    out['read_bytes'] = nbytes
    out['read_GBps'] = round(nbytes / out['stats_kernel_us'] / 1e3, 1)
    out['copy_GBps'] = round(_lib.copy_bandwidth(device=m.device, library=st._L), 1)
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=400)
    ap.add_argument('--configs', default='court1024,fenton512')
    ap.add_argument('--strides', default='1,10,100')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    strides = [int(s) for s in args.strides.split(',')]
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks, strides)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
