#!/usr/bin/env python3
"""tensor_accuracy — every model's step with a diffusion tensor, measured against the oracle with the tensor.

Runs comparisons (a) - (c) of tests/test_gpu_tensor_models.py (cases, bounds and comparisons of tests/tensor_cases.py) on the
device and prints the worst error AS A FRACTION OF ITS BOUND per model, mode, policy and array: (a) one tick on the K = 1 row over
the three grids, without and with a hole; (b) one sub-step taken apart; (c) 20 ticks on oblique, heterogeneous fibres, both
snapshots.  The tests keep the bounds; the measured values live in profiles/tensor_accuracy.txt:

    python tools/tensor_accuracy.py > profiles/tensor_accuracy.txt
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import tensor_cases as tcs  # noqa: E402
from test_gpu_variant_table import EXTRA_ENV  # noqa: E402

POLICIES = ['exact', 'fast']


class Env:
    """monkeypatch's two methods on os.environ, for tensor_cases.device_tick outside pytest"""

    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def row(section, what, value, bound):
    print('%-12s %-104s %9.3f' % (section, what, value / bound if bound else value))
    return (value / bound if bound else value) > (1.0 if bound else 0.0)


def main():
    import oracle as orc
    from test_gpu_frames import PLAN_ENV
    orc.build()
    orc.lib()
    env = Env()
    over = 0
    print('# tools/tensor_accuracy.py: worst error / bound of a tensor handle against the oracle under oracle.tensor (tests/tensor_cases.py)')
    print('# (a) tick: Fenton 20 sub-steps 3e-6 (fast 6e-4); Beeler-Reuter one tick 1e-5 direct, 5e-5 Chebyshev (fast 1.5e-4) of 120 mV,')
    print('#     1e-5 and 1; Courtemanche one tick 6e-6 (fast 3e-5) of its scale; grids %s, without and with a hole' % ', '.join('%dx%d' % g for g in tcs.GRIDS))
    print('# (b) sub-step: "cells with V1 != RN(T + a)" is a count (bound 0); the rest as tests/tensor_cases.py substep_figures derives')
    print('# (c) trajectory: 2e-5 of range after ticks 10 and 20 (fast policy with Chebyshev gates 4e-5; its H at tick 10: the named exception of')
    print('#     tests/tensor_cases.py traj_figures, the distance from the oracle\'s own envelope over 3 x its width + 4e-5), 64 x 64')
    print('%-12s %-104s %9s' % ('', 'model, policy, array', 'of bound'))
    for name in tcs.ALL_CASES:
        for policy in POLICIES:
            fast = policy == 'fast'
            worst = tcs.Worst()
            for hole in (False, True):
                for H, W in tcs.GRIDS:
                    got, _ = tcs.device_tick(name, H, W, fast, hole, env)
                    tcs.compare_tick(orc, worst, name, fast, H, W, hole, got)
            lines = {}
            for key, (err, tol, scale, _, _) in worst.rows.items():
                k = re.sub(r' hole=\d', '', key)
                lines[k] = max(lines.get(k, 0.0), err / (tol * scale))
            for k in sorted(lines):
                over += row('(a) tick', k, lines[k], 1.0)
        sys.stdout.flush()
    for k in PLAN_ENV + EXTRA_ENV:
        os.environ.pop(k, None)
    H, W = 70, 75
    phi, D = tcs.hole_field(H, W), tcs.spd_field(H, W, 23)
    for name in tcs.ALL_CASES:
        for policy in POLICIES:
            fast = policy == 'fast'
            if fast:
                os.environ['FIBHIP_COURT_AGG'] = '0'
            a, b = tcs.handle(name, H, W, fast, phi, spt=1, diff=0.0), tcs.handle(name, H, W, fast, phi, D, spt=1)
            os.environ.pop('FIBHIP_COURT_AGG', None)
            try:
                s0 = b.get_state(-1)
                a.step(1)
                b.step(1)
                T, got = a.get_state(-1), b.get_state(-1)
            finally:
                a.close()
                b.close()
            others, figs = tcs.substep_figures(name, fast, s0, T, got, D, phi)
            over += row('(b) sub-step', '%s %s arrays other than the potential that differ' % (name, policy), float(len(others)), 0.0)
            for what, value, bound in figs:
                over += row('(b) sub-step', what, value, bound)
    sys.stdout.flush()
    for name in tcs.TRAJ_CASES:
        ref = tcs.oracle_traj(orc, name)
        for policy in POLICIES:
            figs = tcs.traj_figures(orc, name, policy == 'fast', tcs.device_traj(name, policy == 'fast'), ref)
            lines = {}
            for what, err, bound in figs:
                k = re.sub(r' t\d+\b', '', what)
                lines[k] = max(lines.get(k, 0.0), err / bound)
            for k in lines:
                over += row('(c) 20 ticks', '%s %s: %s' % (name, policy, k), lines[k], 1.0)
        sys.stdout.flush()
    print('# figures above their bound: %d' % over)


if __name__ == '__main__':
    main()
