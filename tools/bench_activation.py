"""cost of the activation recorder (fib_tf_amd/activation.py, csrc/record_kernels.inc observe_kernel):

    python tools/bench_activation.py [--ticks K] [--configs fenton512,br512,fenton4096] [--out FILE]

For each configuration (BASELINE's grids: obstacle, S1 wave, S2 in the upper-left quadrant, warmed past it), one JSON line:
  unobserved / observed Mcell-steps/s and us per tick  fibhip_time_steps over K ticks, best of 3 (the observed handle runs one
                                                       launch per tick followed by the recorder's kernel)
  observe_us                                           the recorder's kernel alone, median of its HIP-event-bracketed launches
                                                       (fibhip_trace_begin/_end) over K ticks
  observe_gbs, copy_gbs, observe_vs_copy               its 12 bytes per cell at that time, against the streaming-copy yardstick
                                                       (fibhip_copy_bandwidth) — 1.0 means copy speed
  plain_us                                             observed tick minus the recorder: what one launch per tick costs the
                                                       handle against its usual plan (unobserved_us)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fib_tf_amd import _lib  # noqa: E402

CONFIGS = {
    'fenton512': ('fenton', 512), 'br512': ('br', 512), 'fenton4096': ('fenton', 4096),
}


def make(model, n):
    cfg = {'height': n, 'width': n, 'dt': 0.1, 'dt_per_plot': 10, 'duration': 1000}
    if model == 'fenton':
        from fib_tf_amd.fenton import Fenton4v
        m = Fenton4v(dict(cfg, diff=1.5))
        m.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
        amp = 1.0
    else:
        from fib_tf_amd.br import BeelerReuter
        m = BeelerReuter(dict(cfg, diff=0.809, cheby=True, skip=False))
        m.add_hole_to_phase_field(150 * n // 512, 200 * n // 512, 40 * n / 512.0)
        amp = 10.0
    m.define()
    m.add_pace_op('s2', 'luq', amp)
    return m


def rate(st, cells, ticks):
    best = min(st.time_steps(ticks)[0] for _ in range(3))
    return cells * st.steps_per_tick * ticks / (best * 1e-3) / 1e6, best / ticks * 1e3


def one(name, ticks):
    model, n = CONFIGS[name]
    m = make(model, n)
    st = m._stepper
    cells = n * n
    s2 = m.millisecond_to_step(210)
    st.step(s2)
    m.fire_op('s2')
    st.step(20)
    st.sync()
    unobs_rate, unobs_us = rate(st, cells, ticks)
    rec = m.record_activation()
    st.step(5)
    st.sync()
    obs_rate, obs_us = rate(st, cells, ticks)
    st.trace_begin()
    st.step(ticks)
    ev = st.trace_end()
    rec.close()
    obs_k = [e['dur'] for e in ev if e['name'] == 'observe_kernel']
    assert len(obs_k) == ticks, (len(obs_k), ticks)
    observe_us = float(np.median(obs_k))
    copy_gbs = _lib.copy_bandwidth(nbytes=max(cells * 4, 1 << 20), reps=10, library=st._L)
    observe_gbs = 12.0 * cells / (observe_us * 1e-6) / 1e9
    st.close()
    return {'config': name, 'cells': cells, 'ticks': ticks, 'unobserved_mcells': round(unobs_rate, 1),
            'observed_mcells': round(obs_rate, 1), 'unobserved_us': round(unobs_us, 2), 'observed_us': round(obs_us, 2),
            'observe_us': round(observe_us, 2), 'observe_gbs': round(observe_gbs, 1), 'copy_gbs': round(copy_gbs, 1),
            'observe_vs_copy': round(observe_gbs / copy_gbs, 3), 'plain_us': round(obs_us - observe_us, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=200)
    ap.add_argument('--configs', default='fenton512,br512,fenton4096')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []
    for name in args.configs.split(','):
        r = one(name, args.ticks)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
