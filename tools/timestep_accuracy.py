#!/usr/bin/env python3
"""timestep_accuracy — the models at time steps and diffusion coefficients other than 0.1 ms, measured against the reference.

Runs the comparisons of tests/test_gpu_timestep.py (fixtures tests/golden/ts_*.npz, cases and bounds of
tests/timestep_cases.py) and prints, per model, (dt, diff) and variable, the worst error AS A FRACTION OF ITS BOUND — for one
sub-step and for the 20-tick trajectories; columns: the CPU oracle against the reference (under the rounding-faithful
policy's bounds), the device under the fast and under the rounding-faithful policy.  A figure is the worst over the cases
that share the line (Beeler-Reuter: n = 1, 5, 0 and skip on and off; Courtemanche: chronic and not; both snapshots).
The tests keep the bounds; the measured values live in profiles/timestep_accuracy.txt:

    python tools/timestep_accuracy.py > profiles/timestep_accuracy.txt        (--cpu: the oracle's column only, no GPU)
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import timestep_cases as tc  # noqa: E402


def golden(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))


def device_figures(orc, policy):
    names = list(orc.COURT_VARS)
    out = {}
    for p in range(tc.NPAIRS):
        c = tc.fenton_step_case(golden, p)
        out['step fenton ' + tc.pair_id('fenton', p)] = tc.fenton_step_figures(tc.device_fenton_step(c, policy), c, policy)
        c = tc.br_step_case(golden, p)
        out['step br ' + tc.pair_id('br', p)] = [f for tag in ('direct', 'cheby') for n in (1, 5, 0)
                                                 for f in tc.br_step_figures(tc.device_br_step(c, tag, n, policy), c, tag, n, policy)]
        c = tc.court_step_case(golden, p, names)
        out['step court ' + tc.pair_id('court', p)] = [
            f for chronic in (True, False)
            for f in tc.court_step_figures(tc.device_court_step(c, chronic, policy), c, chronic, policy, orc, names, device=True)]
        f = golden('ts_fenton_traj_p%d' % p)
        out['traj fenton ' + tc.pair_id('fenton', p)] = tc.fenton_traj_figures(tc.device_fenton_traj(f, policy), f)
        f = golden('ts_br_traj_p%d' % p)
        out['traj br ' + tc.pair_id('br', p)] = [x for tag in tc.BR_TAGS
                                                 for x in tc.br_traj_figures(tc.device_br_traj(f, tag, policy), f, tag, policy)]
        f = golden('ts_court_traj_p%d' % p)
        snaps, trend = tc.device_court_traj(f, policy)
        out['traj court ' + tc.pair_id('court', p)] = tc.court_traj_figures(snaps, trend, f, names)
        f = golden('ts_court_ultra_traj_p%d' % p)
        out['traj court_ultra ' + tc.pair_id('court', p)] = tc.court_traj_figures(
            tc.device_court_ultra_traj(f, policy), None, f, names, tc.COURT_ULTRA_SCALES, 'court_ultra')
    return out


def line_of(what):
    """the cases that share a line of the table"""
    what = re.sub(r' n=\d| t\d+$|_skip', '', what)
    return re.sub(r'^court (chronic|acute) ', 'court ', what)


def worst(figs):
    out = {}
    for what, err, bound in figs:
        k = line_of(what)
        out[k] = max(out.get(k, 0.0), err / bound)
    return out


def main():
    import oracle as orc
    orc.build()
    cpu_only = '--cpu' in sys.argv[1:]
    orc.lib()
    orc.set_threads(min(orc.num_threads(), 2))
    cols = [('oracle', worst_of(tc.oracle_figures(orc, golden)))]
    if not cpu_only:
        for policy in tc.POLICIES:
            cols.append((policy, worst_of(device_figures(orc, policy))))
    print('# tools/timestep_accuracy.py: worst error / bound against the reference\'s own solve() and define() (tests/golden/ts_*.npz)')
    print('# bounds: one sub-step STEP_TOL[policy] * max(1, dt / 0.1) of range (exact 4e-6, fast 3e-5); 20 ticks 2e-5 of range (fast')
    print('# policy with Chebyshev gates 4e-5); oracle: the exact policy\'s bounds.  Named exception, fast policy with Chebyshev gates:')
    print('# H in one sub-step 1e-4 * max(dt / 0.1, 0.1 / dt), M and H over 20 ticks 4e-5 * max(dt / 0.1, 0.1 / dt) (timestep_cases.fit_room)')
    print('# "near a singularity": distance from the oracle\'s sensitivity envelope over its margin (tests/timestep_cases.py)')
    print('%-18s %-20s %-44s' % ('', '(dt, diff)', 'variable') + ''.join('%9s' % name for name, _ in cols))
    over = 0
    for section in cols[0][1]:
        kind, model, pair = section.split(' ')
        for k in cols[0][1][section]:
            vals = [c[section][k] for _, c in cols]
            over += sum(v > 1.0 for v in vals)
            print('%-18s %-20s %-44s' % (kind + ' ' + model, pair, k) + ''.join('%9.3f' % v for v in vals))
        sys.stdout.flush()
    print('# figures above 1.000: %d' % over)
    if not cpu_only:
        from test_gpu_timestep import applied_diffusion_error
        print('# relative error of the diffusion constant the device applies, as test_applied_diffusion_constant estimates it, over')
        print('# its bound 2^-25 (a constant rounded wrongly is off by 2^-24 .. 2^-23 of itself: 2.0 .. 4.0 here)')
        for model in ('fenton', 'br', 'court'):
            for p in (0, 1, 2):
                vals = [applied_diffusion_error(orc, model, p, policy)[0] / 2.0 ** -25 for policy in tc.POLICIES]
                print('%-18s %-20s %-44s' % ('diffusion ' + model, tc.pair_id(model, p), 'float(diff * dt)') + '%9s' % ''
                      + ''.join('%9.3f' % v for v in vals))


def worst_of(sections):
    return {s: worst(figs) for s, figs in sections.items()}


if __name__ == '__main__':
    main()
