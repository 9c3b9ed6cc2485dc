"""not-gpu: pins the ORACLE (oracle/fib_oracle.c) to the golden vectors that the reference's own
functions produced (tests/golden/make_golden.py), and to the reference's own native cross-check
(generate_table.cpp output committed as tests/golden/court_calc_inter_m50.txt).

  * arithmetic-only paths: bit-exact
  * one solve(): <= 4e-6 of the variable's range (libm vs NumPy transcendental kernels, few ulp)
  * trajectories (200-1000 sub-steps): <= 2e-5 .. 1e-3 of range, growing with the horizon
"""
import os

import numpy as np
import pytest


def close(got, want, tol, scale, what):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    assert err <= tol * scale, '%s: max|d| %.3e > %.1e*%g' % (what, err, tol, scale)


def test_unit_ops_bit_exact(orc, golden):
    u = golden('unit_ops')
    assert np.array_equal(orc.enforce_boundary(u['X']), u['enforce_boundary'])
    assert np.array_equal(orc.laplace(u['X']), u['laplace_nophase'])
    assert np.array_equal(orc.laplace(u['X'], u['phi']), u['laplace_phase'])
    assert np.array_equal(orc.phase_field(u['X'], u['phi']), u['phase_field'])


def test_rush_larsen(orc, golden):
    u = golden('unit_ops')
    for dt in (0.1, 0.5, 1.0):
        close(orc.rush_larsen(u['rl_g'], u['rl_inf'], u['rl_tau'], dt), u['rush_larsen_dt%g' % dt], 3e-7, 1.0,
              'rush_larsen %g' % dt)


@pytest.mark.parametrize('variant', ['phase', 'nophase'])
def test_fenton_step(orc, golden, variant):
    f = golden('fenton_step_' + variant)
    slab = np.stack([f[k] for k in 'UVWS'])
    out = orc.fenton_step(slab, float(f['dt']), float(f['diff']), f['phase'])
    for i, k in enumerate('UVWS'):
        close(out[i], f[k + '1'], 2e-7, 1.0, 'fenton ' + k)
    assert np.array_equal(out[1], f['V1']) and np.array_equal(out[2], f['W1'])
    d = orc.fenton_diff(*[f[k] for k in 'UVWS'])
    for i, k in enumerate('UVWS'):
        close(d[i], f['d' + k], 4e-7, 1.0, 'fenton d' + k)


@pytest.mark.parametrize('mode', ['direct', 'cheby'])
@pytest.mark.parametrize('n', [1, 5, 0])
def test_br_step(orc, golden, mode, n):
    f = golden('br_step')
    tbl = golden('br_cheby_table')['d'].astype(np.float32) if mode == 'cheby' else None
    slab = np.stack([f[k] for k in orc.BR_VARS])
    out = orc.br_step(slab, 0.1, 0.809, f['phase'], tbl, n)
    for i, k in enumerate(orc.BR_VARS):
        close(out[i], f['%s1_%s_n%d' % (k, mode, n)], 2e-6, {'V': 120.0, 'C': 1e-5}.get(k, 1.0), 'br ' + k)


SINGULAR = [-10.0001, -10.0, 7.9, -47.13, -14.1, 3.3328, 19.9]


def court_envelope_samples(orc, slab, phase, chronic, dt=0.1, diff=0.809):
    """one Courtemanche step under every combination of exp() moved by -1/0/+1 ulp and all potentials moved by -2 .. +2
    float32 neighbours: what ANY float32 evaluation of the reference's formulas may legitimately return"""
    samples = []
    try:
        for ulps in (-1, 0, 1):
            orc.set_exp_ulps(ulps)
            for shift in (-2, -1, 0, 1, 2):
                s2 = slab.copy()
                for _ in range(abs(shift)):
                    s2[0] = np.nextafter(s2[0], np.float32(np.inf if shift > 0 else -np.inf))
                samples.append(orc.court_step(s2, dt, diff, phase, chronic).astype(np.float64))
    finally:
        orc.set_exp_ulps(0)
    return np.stack(samples)


@pytest.mark.parametrize('tag', ['chronic', 'acute'])
def test_court_step(orc, golden, tag):
    f = golden('court_step')
    slab = np.stack([f[k] for k in orc.COURT_VARS])
    out = orc.court_step(slab, 0.1, 0.809, f['phase'], tag == 'chronic')
    V = orc.enforce_boundary(f['V'])
    near = np.zeros(V.shape, bool)
    exact = np.zeros(V.shape, bool)
    for s in SINGULAR:
        near |= np.abs(V - np.float32(s)) < 0.06
        exact |= V == np.float32(s)
    ok = ~near | exact
    # near a singularity: the golden value must lie inside the oracle's own sensitivity envelope there (the step
    # re-evaluated with exp() anywhere within one ulp and every potential within two float32 neighbours), see test_gpu_parity.test_court_single_step
    samples = court_envelope_samples(orc, slab, f['phase'], tag == 'chronic')
    scales = {'V': 150.0, '_Na_i_': 3.0, '_K_i_': 15.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5, '_Ca_up_': 1.0}
    for i, k in enumerate(orc.COURT_VARS):
        want = f['%s_1_%s' % (k, tag)].astype(np.float64)
        tol = 4e-6 * scales.get(k, 1.0)
        d = np.abs(out[i].astype(np.float64) - want)
        assert d[ok].max() <= tol, (k, d[ok].max())
        lo, hi = samples[:, i].min(axis=0), samples[:, i].max(axis=0)
        margin = 3.0 * (hi - lo) + tol
        outside = np.maximum(lo - margin - want, want - hi - margin)
        assert outside[near].max() <= 0.0, (k, outside[near].max())


def test_court_calc_inter_vs_reference_binary(orc):
    want = np.loadtxt(os.path.join(os.path.dirname(__file__), 'golden', 'court_calc_inter_m50.txt'))
    got = orc.court_calc_inter(-50.0)
    for i, (g, w) in enumerate(zip(got, want)):
        tol = 5e-6 if i == 3 else 2e-6      # tau_d: court.py:304 uses V+10.0001, courtemanche.h:178 V+10
        assert abs(g - w) <= tol * max(abs(w), 1.0) + 6e-7, (i, g, w)


def test_reference_binary_is_reproducible():
    """when the reference tree is present (build container), oracle/_ref rebuilt from it must print
    exactly the committed fixture"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle', '_ref', 'generate_table')
    if not os.path.exists(exe):
        pytest.skip('oracle/_ref not built (no reference tree on this machine)')
    out = subprocess.check_output([exe]).decode()
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'court_calc_inter_m50.txt')) as f:
        assert out == f.read()


@pytest.mark.parametrize('name', ['fenton_traj64', 'fenton_traj_ragged'])
def test_fenton_trajectory(orc, golden, name):
    f = golden(name)
    slab = np.stack([f['init_' + k] for k in 'UVWS']).copy()
    t0 = 0
    for t in [int(x) for x in f['snap_ticks']]:
        orc.fenton_run(slab, 0.1, float(f['diff']), f['phase'], 10 * (t - t0))
        t0 = t
        for i, k in enumerate('UVWS'):
            close(slab[i], f['%s_t%d' % (k, t)], 2e-6, 1.0, '%s %s t%d' % (name, k, t))


def test_fenton_driver(orc, golden):
    from fib_tf_amd.ionic import IonicModel
    f = golden('fenton_driver96')
    g = IonicModel({'height': 96, 'width': 96})
    slab = np.stack([f['init_' + k] for k in 'UVWS']).copy()
    cube = []
    for i in range(60):
        orc.fenton_run(slab, 0.1, 1.5, f['phase'], 10)
        if i == int(f['s2'][0]):
            slab[0] = orc.pace(slab[0], *g.pace_rect('luq'), float(f['s2'][1]), 0.0)
        if i % 10 == 0:
            cube.append(slab[0] * f['phase'])
    close(np.array(cube), f['cube'], 5e-6, 1.0, 'cube')
    for i, k in enumerate('UVWS'):
        close(slab[i], f['%s_t60' % k], 5e-6, 1.0, 'final ' + k)


@pytest.mark.parametrize('name', ['br_traj64_direct', 'br_traj64_cheby', 'br_traj64_skip', 'br_traj64_cheby_skip'])
def test_br_trajectory(orc, golden, name):
    from fib_tf_amd.ionic import IonicModel
    f = golden(name)
    tbl = golden('br_cheby_table')['d'].astype(np.float32) if bool(f['cheby']) else None
    slab = np.stack([f['init_' + k] for k in orc.BR_VARS]).copy()
    g = IonicModel({'height': 64, 'width': 64})
    t0 = 0
    for t in [int(x) for x in f['snap_ticks']]:
        for i in range(t0, t):
            orc.br_run(slab, 0.1, float(f['diff']), f['phase'], tbl, bool(f['skip']), 1)
            if name.endswith('cheby_skip') and i == 10:
                slab[0] = orc.pace(slab[0], *g.pace_rect('luq'), 10.0, -90.0)
        t0 = t
        for i, k in enumerate(orc.BR_VARS):
            want = f['%s_t%d' % (k, t)]
            sc = {'V': 120.0, 'C': max(float(want.max() - want.min()), 1e-7)}.get(k, 1.0)
            close(slab[i], want, 1e-5, sc, '%s %s t%d' % (name, k, t))


def test_court_trajectory(orc, golden):
    f = golden('court_traj64')
    slab = np.stack([f['init_' + k] for k in orc.COURT_VARS]).copy()
    calcium = ('_Ca_i_', '_Ca_rel_', '_Ca_up_', '_u_', '_v_', '_w_', '_f_Ca_')
    scales = {'V': 150.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5}
    t0 = 0
    for t in [int(x) for x in f['snap_ticks']]:
        orc.court_run(slab, 0.1, float(f['diff']), f['phase'], True, t0, t - t0)
        t0 = t
        for i, k in enumerate(orc.COURT_VARS):
            tol = 1e-5 if t <= 100 else (5e-3 if k in calcium else 2e-4)
            close(slab[i], f['%s_t%d' % (k, t)], tol, scales.get(k, 1.0), 'court %s t%d' % (k, t))


def test_golden_probe_values(golden):
    """the anchors SURVEY.md 8c quotes from an independent probe of the reference"""
    f = golden('fenton_traj64')
    assert abs(float(f['U_t20'].astype(np.float64).sum()) - 3586.757049) < 1e-3
    assert abs(float(f['U_t20'].max()) - 1.013836) < 1e-6
    b = golden('br_traj64_cheby')['V_t40']
    assert abs(float(b.mean()) - (-48.70845)) < 1e-4 and abs(float(b.max()) - 0.63488) < 1e-4
    c = golden('court_traj64')
    assert abs(float(c['V_t300'].mean()) - (-11.68459)) < 1e-4


def test_court_ultra_trajectory(orc, golden):
    """single-rate court_ultra.py schedule (all 21 variables every tick, dt)"""
    from fib_tf_amd.ionic import IonicModel
    f = golden('court_ultra_traj')
    H, W = f['phase'].shape
    rect = IonicModel({'height': H, 'width': W}).pace_rect('luq')
    slab = np.stack([f['init_' + k] for k in orc.COURT_VARS]).copy()
    t0 = 0
    for t in [int(x) for x in f['snap_ticks']]:
        for i in range(t0, t):
            orc.court_ultra_run(slab, 0.1, float(f['diff']), f['phase'], True, 1)
            if i == 50:
                slab[0] = orc.pace(slab[0], *rect, 10.0, -100.0)
        t0 = t
        for i, k in enumerate(orc.COURT_VARS):
            close(slab[i], f['%s_t%d' % (k, t)], 1e-5, {'V': 150.0, '_Ca_i_': 1e-3}.get(k, 1.0), 'ultra %s t%d' % (k, t))


def test_court_ultra_us_trajectory(orc, golden):
    """court_ultra.py with config['ultra_slow']=True: 22 arrays, `_us_` scales i_Na"""
    from fib_tf_amd.ionic import IonicModel
    f = golden('court_ultra_us_traj')
    H, W = f['phase'].shape
    names = [str(x) for x in f['names']]
    assert names == list(orc.COURT_VARS) + ['_us_']
    rect = IonicModel({'height': H, 'width': W}).pace_rect('luq')
    slab = np.stack([f['init_' + k] for k in names]).copy()
    t0 = 0
    for t in [int(x) for x in f['snap_ticks']]:
        for i in range(t0, t):
            orc.court_ultra_us_run(slab, 0.1, float(f['diff']), f['phase'], True, 1)
            if i == 50:
                slab[0] = orc.pace(slab[0], *rect, 10.0, -100.0)
        t0 = t
        for i, k in enumerate(names):
            # _u_/_v_: the SR-release sigmoids (width 1.367e-15 in Fn) amplify libm-vs-stand-in ulps of the currents
            close(slab[i], f['%s_t%d' % (k, t)], 1e-5, {'V': 150.0, '_Ca_i_': 1e-3, '_u_': 5.0, '_v_': 5.0}.get(k, 1.0),
                  'ultra_us %s t%d' % (k, t))
    # the gate itself: per-step increments are ~1e-7, so it is pinned to a few ulp of 0.72
    assert np.max(np.abs(slab[21] - f['_us__t120'])) <= 2e-7
    a, b = orc.court_us_inter(f['us_sweep_V'])
    # 1 - tanh(x) cancels for V >> -83 mV: one ulp of tanh is an absolute 6e-8 in alpha_us/3e-5
    assert np.allclose(a, f['us_sweep_us_infinity'], rtol=3e-6, atol=3e-7)
    assert np.allclose(b, f['us_sweep_tau_us'], rtol=3e-6, atol=0)


@pytest.fixture(scope='module')
def timestep_figures(orc, golden):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import timestep_cases as tc
    n = orc.num_threads()
    orc.set_threads(min(n, 2))                          # planes of 960 and 2688 cells: a wide team only waits for itself
    try:
        return tc, tc.oracle_figures(orc, golden)
    finally:
        orc.set_threads(n)


@pytest.mark.parametrize('kind,model', [('step', 'fenton'), ('step', 'br'), ('step', 'court'), ('traj', 'fenton'), ('traj', 'br'),
                                        ('traj', 'court'), ('traj', 'court_ultra')])     # (court_ultra.py's solve is court.py's)
@pytest.mark.parametrize('p', range(4))
def test_oracle_at_other_time_steps(timestep_figures, kind, model, p):
    """the oracle against the reference's own solve() and define() at (dt, diff) other than (0.1, .): tests/golden/ts_*.npz,
    under the bounds the device's rounding-faithful policy gets in tests/test_gpu_timestep.py (one sub-step:
    4e-6 * max(1, dt / 0.1) of range; 20 ticks: 2e-5 of range) — measured here against the reference, so the device's
    oracle comparisons at these time steps do not rest on the oracle alone"""
    tc, figs = timestep_figures
    tc.check(figs['%s %s %s' % (kind, model, tc.pair_id(model.split('_')[0], p))])


def test_timestep_fixtures_exact_parts(orc, golden):
    """arithmetic-only parts of the new fixtures, bit for bit in the oracle at every dt: Fenton's V1 and W1 (no
    transcendental function on their path), Beeler-Reuter's slow gates under solve(state, 0)"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import timestep_cases as tc
    for p in range(tc.NPAIRS):
        c = tc.fenton_step_case(golden, p)
        out = orc.fenton_step(np.stack([c[k] for k in 'UVWS']), c['dt'], c['diff'], c['phase'])
        assert np.array_equal(out[1], c['V1']) and np.array_equal(out[2], c['W1']), p
        c = tc.br_step_case(golden, p)
        out = orc.br_step(np.stack([c[k] for k in tc.BR_VARS]), c['dt'], c['diff'], c['phase'], None, 0)
        for i, k in enumerate(tc.BR_VARS):
            if k in tc.BR_SLOW:
                assert np.array_equal(out[i], c[k]), (p, k)


def test_fenton_simple_trajectory(orc, golden):
    """fenton_simple.py: zero-padded convolution Laplacian, its own S2 op on [:H//2, :W//2]"""
    f = golden('fenton_simple_traj')
    s = np.stack([f['init_' + k] for k in 'UVWS']).copy()
    H, W = s[0].shape
    t0 = 0
    for t in [int(x) for x in f['snap_steps']]:
        for i in range(t0, t):
            orc.fenton_simple_run(s, 0.1, float(f['diff']), 1)
            if i == int(f['s2_step']):
                s2 = np.zeros_like(s[0])
                s2[:H // 2, :W // 2] = 1.0
                s[0] = np.maximum(s[0], s2)
        t0 = t
        for k, n in enumerate('UVWS'):
            close(s[k], f['%s_t%d' % (n, t)], 1e-6, 1.0, 'fenton_simple %s t%d' % (n, t))
    # the outermost ring is where the variant differs from fenton.py: check that the fixture really exercises it
    assert abs(float(f['U_t10'][0, 2]) - float(f['U_t10'][1, 2])) > 0.05
