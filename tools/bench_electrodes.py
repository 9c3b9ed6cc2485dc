"""cost of the electrode recorder (fib_tf_amd/egm.py, csrc/record_kernels.inc electrode_kernel) against polling:

    python tools/bench_electrodes.py [--ticks K] [--configs fenton512,br512,fenton4096] [--strides 1,2,10] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it; the reference's
two Gaussian electrodes of radius 5, 30 px apart), one JSON line.  Every figure is host wall time per tick over K ticks
stepped ONE CALL PER TICK, as a driver loop steps, ended by the call that makes the result visible; best of 3:
  none_us                 no recorder, a sync() at the end
  device_us[stride]       ElectrodeRecorder at that stride (attached before the clock starts), traces() at the end
  polled_us[stride]       what egm.record() does at that stride: image() and two np.mean(frame * mask) at every sample
  electrode_kernel_us     the kernel alone, median of its HIP-event-bracketed launches (fibhip_trace_begin/_end)
  combine_us              (with --whole-grid) the same for a whole-grid electrode: electrode_kernel over 256 chunks and
                          electrode_combine_kernel behind it
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
from fib_tf_amd import egm  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_activation import CONFIGS, make  # noqa: E402


def wall(fn, ticks, before=None, after=None):
    """best of 3 of fn(); `before` / `after` (attaching and detaching a recorder) stay outside the clock"""
    best = None
    for _ in range(3):
        arg = before() if before else None
        t0 = time.perf_counter()
        fn(arg) if before else fn()
        dt = time.perf_counter() - t0
        if after:
            after(arg)
        best = dt if best is None else min(best, dt)
    return round(best / ticks * 1e6, 2)


def one(name, ticks, strides, whole_grid):
    model, n = CONFIGS[name]
    m = make(model, n)
    st = m._stepper
    s2 = m.millisecond_to_step(210)
    st.step(s2)
    m.fire_op('s2')
    st.step(20)
    st.sync()
    c = n // 2
    masks = [egm.create_mask(m, c + 15 * n // 512, c, 5), egm.create_mask(m, c - 15 * n // 512, c, 5)]

    def none():
        for _ in range(ticks):
            st.step(1)
        st.sync()

    def device(rec):
        for _ in range(ticks):
            st.step(1)
        assert rec.traces().shape[1] == 2

    def polled(stride):
        def run():
            rows = []
            for i in range(ticks):
                st.step(1)
                if i % stride == 0:
                    frame = m.image()
                    rows.append([np.mean(frame * masks[0]), np.mean(frame * masks[1])])
            st.sync()
        return run

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'none_us': wall(none, ticks), 'device_us': {}, 'polled_us': {}}
    for s in strides:
        out['device_us'][str(s)] = wall(device, ticks, before=lambda s=s: m.record_electrodes(masks, every=s, capacity=ticks // s),
                                        after=lambda rec: rec.close())
        out['polled_us'][str(s)] = wall(polled(s), ticks)
    out['none_again_us'] = wall(none, ticks)

    def kernel_times(mask_list, k):
        with m.record_electrodes(mask_list, every=1, capacity=k + 1):
            st.step(1)
            st.trace_begin()
            st.step(k)
            ev = st.trace_end()
        return {nm: round(float(np.median([e['dur'] for e in ev if e['name'] == nm])), 2)
                for nm in ('electrode_kernel', 'electrode_combine_kernel') if any(e['name'] == nm for e in ev)}
    out['electrode_kernel_us'] = kernel_times(masks, 50)['electrode_kernel']
    if whole_grid:
        phi = np.random.default_rng(0).uniform(0.5, 1.0, (n, n)).astype(np.float32)
        out['whole_grid_us'] = kernel_times([phi], 20)
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=400)
    ap.add_argument('--configs', default='fenton512,br512,fenton4096')
    ap.add_argument('--strides', default='1,2,10')
    ap.add_argument('--whole-grid', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    strides = [int(s) for s in args.strides.split(',')]
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks, strides, args.whole_grid)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
