"""cost of a diffusion tensor (fibhip_set_tensor; csrc/tick_kernel.inc behind TensorOf):

    python tools/bench_tensor.py [--size N] [--ticks K] [--repeats R] [--out FILE]

Microseconds per tick of a Fenton and a Beeler-Reuter (direct gates) sheet of N x N cells with a hole, fast policy,
  (a) tensor_us      on a handle with a rotating fibre field (ratio 2), whose plan is the flat row the tensor table lists first for
                     the grid (Fenton: 10 sub-steps in 32 x 32 tiles of 1024 threads; Beeler-Reuter: 5 in 32 x 32 of 512), and
  (b) same_row_us    on the same handle with the tensor removed and FIBHIP_VARIANT naming that very row of the isotropic table: the
                     same kernel family, the same fusion depth and tile on the same device in the same run — what the five weight
                     planes, their loads and the four extra multiplications per cell cost;
  (c) default_us     beside them, the handle as it runs by default (strips, several ticks per launch): what a tensor handle gives up
                     by running flat tiles, one launch per tick or part of it.
HIP events on the handle's stream around K ticks that end in a synchronise (fibhip_time_steps); one untimed run of each arm first,
then `repeats` rounds that alternate the arms, medians and the spread (max - min) of each.  Reported, not gated.
The last line written to FILE is the JSON record; the lines above it say how the figures were taken."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = {'fenton': '10,32,32,1024', 'br': '5,32,32,512'}


def fibres(n):
    """fibres that rotate by a quarter turn across the sheet, anisotropy ratio 2"""
    from fib_tf_amd.tensor import fibre_tensor
    angle = np.broadcast_to(np.linspace(0.0, np.pi / 2, n)[None, :], (n, n))
    return fibre_tensor(angle, 2.0)


def make(kind, n):
    from fib_tf_amd.br import BeelerReuter
    from fib_tf_amd.fenton import Fenton4v
    # (Beeler-Reuter with its direct gates: the Chebyshev path runs a build with the table baked in, which keeps the default rows of
    # the isotropic table only — no flat row of 5 sub-steps to put beside the tensor's)
    cfg = {'height': n, 'width': n, 'dt': 0.1, 'dt_per_plot': 10, 'duration': 1000, 'diff': 1.5 if kind == 'fenton' else 0.809, 'cheby': False,
           'skip': False}
    m = (Fenton4v if kind == 'fenton' else BeelerReuter)(cfg)
    m.add_hole_to_phase_field(n // 2, n // 2, 30 * n / 512.0)
    m.define()
    return m


def arm(st, state, ticks):
    st.set_state(-1, state)
    ms, _ = st.time_steps(ticks)
    return ms * 1e3 / ticks


def measure(kind, n, ticks, repeats):
    m = make(kind, n)
    st = m._stepper
    state = st.get_state(-1)
    D = fibres(n)
    arms = {'tensor_us': (D, None), 'same_row_us': (None, ROWS[kind]), 'default_us': (None, None)}
    got = {k: [] for k in arms}
    plans = {}
    for rnd in range(repeats + 1):                                        # round 0: untimed (code objects, the plan's own timing)
        for name, (tensor, row) in arms.items():
            os.environ.pop('FIBHIP_VARIANT', None)
            if row:
                os.environ['FIBHIP_VARIANT'] = row
            if tensor is None:
                st.set_tensor(None)
                st.set_phase(m.phase)                                     # (chooses the plan again, under this arm's environment)
            else:
                st.set_tensor(*tensor)
            st.set_state(-1, state)
            st.step(1)                                                    # the first tick of a plan may time candidate shapes
            st.sync()
            plans[name] = (st.launch_plan(), st.plan_tile(), st.ticks_per_launch())
            if name != 'default_us':                                      # both arms on the row this tool names, or no figure at all
                K, TX, TY, NT = (int(x) for x in ROWS[kind].split(','))
                if plans[name][0][0] != K or tuple(plans[name][1]) != (TX, TY, -NT):
                    sys.exit('bench_tensor: %s %s runs %r, not the row %s' % (kind, name, plans[name], ROWS[kind]))
            us = arm(st, state, ticks)
            if rnd:
                got[name].append(us)
    os.environ.pop('FIBHIP_VARIANT', None)
    out = {'model': kind, 'size': n, 'ticks': ticks, 'repeats': repeats}
    for name in arms:
        out[name] = round(statistics.median(got[name]), 3)
        out[name.replace('_us', '_spread_us')] = round(max(got[name]) - min(got[name]), 3)
        out[name.replace('_us', '_plan')] = plans[name]
    out['tensor_over_same_row'] = round(out['tensor_us'] / out['same_row_us'], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ticks', type=int, default=2000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tensor_cost.txt'))
    a = ap.parse_args()
    if a.size < 16 or a.ticks < 1 or a.repeats < 1:
        ap.error('size >= 16, ticks >= 1, repeats >= 1')
    from fib_tf_amd import _lib
    if _lib.lib().fibhip_device_count() < 1:
        sys.exit('bench_tensor: no HIP device (this measurement has no CPU path)')
    rec = [measure(kind, a.size, a.ticks, a.repeats) for kind in ('fenton', 'br')]
    lines = ['tools/bench_tensor.py --size %d --ticks %d --repeats %d' % (a.size, a.ticks, a.repeats),
             'us per tick by HIP events around %d ticks ending in a synchronise; fast policy, hole of radius %g; medians of %d alternating rounds'
             % (a.ticks, 30 * a.size / 512.0, a.repeats)]
    for r in rec:
        lines.append('%-6s %d^2: tensor %.2f us (spread %.2f) | same flat row without a tensor (FIBHIP_VARIANT=%s) %.2f us (spread %.2f) | '
                     'ratio %.3f | default plan without a tensor %.2f us (spread %.2f)'
                     % (r['model'], r['size'], r['tensor_us'], r['tensor_spread_us'], ROWS[r['model']], r['same_row_us'], r['same_row_spread_us'],
                        r['tensor_over_same_row'], r['default_us'], r['default_spread_us']))
    lines.append(json.dumps(rec))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
