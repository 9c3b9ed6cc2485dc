"""cost of the tip recorder (fib_tf_amd/tips.py, csrc/record_kernels.inc tip_kernel) against polling:

    python tools/bench_tips.py [--ticks K] [--configs fenton512,fenton4096] [--strides 1,10] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it), one JSON
line.  Every figure is host wall time per tick over K ticks stepped ONE CALL PER TICK, as a driver loop steps, ended by
the call that makes the result visible; best of 3:
  none_us            no recorder, a sync() at the end
  device_us[stride]  TipRecorder at that stride (attached before the clock starts), counts() at the end
  polled_us[stride]  polling: both watched arrays read back and searched with the NumPy restatement (tests/tip_ref.py) at
                     every sample
  tip_kernel_us      the kernel alone, median of its HIP-event-bracketed launches (fibhip_trace_begin/_end)
  copy_us            copy_kernel moving the bytes tip_kernel reads once (two arrays: read + written = that many bytes), from
                     the rate fibhip_copy_bandwidth measures in this run at that size
  launch_stats       (structural) multi-tick launches and ticks of the stride-10 run: ten-tick launches survive
Under `rocprofv3 --kernel-trace --stats -- python tools/bench_tips.py ...` the profiler's own tip_kernel time is the figure
DESIGN.md section 12 quotes.  One process; stops at the first failure.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fib_tf_amd import _lib  # noqa: E402
import tip_ref  # noqa: E402
from bench_activation import CONFIGS, make  # noqa: E402
from bench_electrodes import wall  # noqa: E402


def one(name, ticks, strides):
    model, n = CONFIGS[name]
    m = make(model, n)
    st = m._stepper
    s2 = m.millisecond_to_step(210)
    st.step(s2)
    m.fire_op('s2')
    st.step(20)
    st.sync()
    var, var2, a0, b0 = m.tip_signals
    mask = None if m.phase is None else np.asarray(m.phase) > 0.5

    def none():
        for _ in range(ticks):
            st.step(1)
        st.sync()

    def device(rec):
        for _ in range(ticks):
            st.step(1)
        assert rec.counts().shape[1] == 3

    def polled(stride):
        def run():
            rows = []
            for i in range(ticks):
                st.step(1)
                if (i + 1) % stride == 0:
                    rows.append(tip_ref.tips(st.get_state(var), st.get_state(var2), a0, b0, mask)[1])
            st.sync()
        return run

    out = {'config': name, 'cells': n * n, 'ticks': ticks, 'none_us': wall(none, ticks), 'device_us': {}, 'polled_us': {}}
    for s in strides:
        stats = {}

        def attach(s=s):
            stats['before'] = st.launch_stats()
            return m.record_tips(every=s, capacity=ticks // s)

        def detach(rec):
            stats['after'] = st.launch_stats()
            stats['tips'] = rec.counts()[:, 2].tolist()
            rec.close()
        out['device_us'][str(s)] = wall(device, ticks, before=attach, after=detach)
        if s == 10:
            out['launch_stats'] = {k: stats['after'][k] - stats['before'][k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
        out.setdefault('tips_per_sample_max', {})[str(s)] = int(max(stats['tips'])) if stats['tips'] else 0
        out['polled_us'][str(s)] = wall(polled(s), ticks)
    out['none_again_us'] = wall(none, ticks)
    with m.record_tips(every=1, capacity=52):
        st.step(1)
        st.trace_begin()
        st.step(50)
        ev = st.trace_end()
    out['tip_kernel_us'] = round(float(np.median([e['dur'] for e in ev if e['name'] == 'tip_kernel'])), 2)
    moved = 2 * n * n * 4                                     # what tip_kernel reads once: the two watched arrays
    gbs = _lib.copy_bandwidth(nbytes=moved // 2, reps=20, device=0)    # a copy of one array: the same bytes, read + written
    out['copy_gbs'] = round(float(gbs), 1)
    out['copy_us'] = round(moved / (gbs * 1e9) * 1e6, 2)
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=400)
    ap.add_argument('--configs', default='fenton512,fenton4096')
    ap.add_argument('--strides', default='1,10')
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
