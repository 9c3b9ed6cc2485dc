"""Shared by tests/test_oracle_golden.py, tests/test_gpu_timestep.py and tools/timestep_accuracy.py: the fixtures
tests/golden/ts_*.npz (the reference's own solve() and define() at time steps and diffusion coefficients other than
0.1 ms, tests/golden/make_golden.py section 4), the bounds, and the comparisons as lists of figures
`(what, error, bound)` — the tests assert error <= bound for each, the tool prints error / bound.

Bounds.  One sub-step: STEP_TOL[policy] * max(1, dt / 0.1) of the variable's range.  The difference between two float32
evaluations of one step is a rate error times dt (the transcendental functions differ by a few ulp in the rates, the
update multiplies by dt), so a step above 0.1 ms gets proportionally more room; a step below 0.1 gets none.
Trajectories: the bounds of tests/test_gpu_parity.py unchanged (2e-5 of range at <= 200 sub-steps).
"""
import numpy as np

PAIRS = {'fenton': [(0.02, 1.5), (0.05, 3.0), (0.2, 0.7), (0.03, 0.0)],
         'br': [(0.02, 0.809), (0.05, 1.6), (0.2, 0.4), (0.03, 0.0)],
         'court': [(0.02, 0.809), (0.05, 1.6), (0.2, 0.4), (0.03, 0.0)]}
NPAIRS = 4
POLICIES = ['fast', 'exact']
STEP_TOL = {'exact': 4e-6, 'fast': 3e-5}
TRAJ_TOL = 2e-5
BR_VARS = ('V', 'C', 'M', 'H', 'J', 'D', 'F', 'XI')
BR_SLOW = ('J', 'D', 'F', 'XI')
BR_TAGS = ('direct', 'cheby', 'direct_skip', 'cheby_skip')
COURT_STEP_SCALES = {'V': 150.0, '_Na_i_': 3.0, '_K_i_': 15.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5, '_Ca_up_': 1.0}
COURT_TRAJ_SCALES = {'V': 150.0, '_Na_i_': 1.0, '_K_i_': 1.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5, '_Ca_up_': 1.0}
COURT_ULTRA_SCALES = {'V': 150.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5}
SINGULAR = [-10.0001, -10.0, 7.9, -47.13, -14.1, 3.3328, 19.9]
S2_TICK = 12                # Courtemanche trajectories: S2 in the left upper quadrant after this tick


def room(dt):
    return max(1.0, dt / 0.1)


def pair_id(model, p):
    return 'dt%g-diff%g' % PAIRS[model][p]


def maxerr(got, want):
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float('inf')
    return float(np.abs(got - np.asarray(want, np.float64)).max())


def check(figures):
    bad = ['%s: %.3e > %.3e' % f for f in figures if not f[1] <= f[2]]
    assert not bad, '; '.join(bad)


# ------------------------------------------------------------------------------------------------
# loaders: the layout of make_golden.timestep_steps() back into the keys of the 0.1 ms fixtures
# ------------------------------------------------------------------------------------------------
def _head(f, p, model):
    dt, diff = float(f['dt'][p]), float(f['diff'][p])
    assert (dt, diff) == PAIRS[model][p]
    return {'dt': dt, 'diff': diff, 'phase': f['phase']}


def fenton_step_case(golden, p):
    f = golden('ts_fenton_step')
    c = _head(f, p, 'fenton')
    for k in 'UVWS':
        c[k], c[k + '1'] = f[k], f['%s1_p%d' % (k, p)]
    return c


def br_step_case(golden, p):
    f = golden('ts_br_step')
    c = _head(f, p, 'br')
    for k in BR_VARS:
        c[k] = f[k]
        for tag in ('direct', 'cheby'):
            for n in (1, 5, 0):
                if k not in BR_SLOW:                    # V, C, M, H do not depend on n
                    c['%s1_%s_n%d' % (k, tag, n)] = f['%s1_%s_p%d' % (k, tag, p)]
                elif n == 0:                            # solve(state, 0) returns the slow gates it was given
                    c['%s1_%s_n0' % (k, tag)] = f[k]
                else:
                    c['%s1_%s_n%d' % (k, tag, n)] = f['%s1_%s_n%d_p%d' % (k, tag, n, p)]
    return c


def court_step_case(golden, p, names):
    f = golden('ts_court_step')
    c = _head(f, p, 'court')
    for k in names:
        c[k] = f[k]
        c[k + '_1_chronic'] = f['%s_1_chronic_p%d' % (k, p)]
        key = '%s_1_acute_p%d' % (k, p)                 # stored only where `chronic` changes the variable
        c[k + '_1_acute'] = f[key] if key in f.files else c[k + '_1_chronic']
    return c


def cheby_table(golden):
    return golden('br_cheby_table')['d'].astype(np.float32)


# ------------------------------------------------------------------------------------------------
# figures: one sub-step
# ------------------------------------------------------------------------------------------------
def fenton_step_figures(out, c, policy):
    tol = STEP_TOL[policy] * room(c['dt'])
    return [('fenton %s1' % k, maxerr(o, c[k + '1']), tol) for k, o in zip('UVWS', out)]


def br_step_figures(out, c, tag, n, policy):
    figs = []
    for k, o in zip(BR_VARS, out):
        tol = STEP_TOL[policy] * room(c['dt'])
        if tag == 'cheby' and policy == 'fast' and k == 'H':
            tol = 1e-4 * fit_room(c['dt'])      # the exception of test_gpu_parity.test_br_single_step, see fit_room
        scale = {'V': 120.0, 'C': 1e-5}.get(k, 1.0)
        figs.append(('br %s %s n=%d' % (tag, k, n), maxerr(o, c['%s1_%s_n%d' % (k, tag, n)]), tol * scale))
    return figs


def fit_room(dt):
    """NAMED EXCEPTION — fast policy, Chebyshev gates: how the allowance for the fused multiply-adds in the degree-8 sums
    scales with dt.  Above 0.1 ms like every other bound, dt / 0.1.  Below, 0.1 / dt instead of 1:

    The fast policy's sums round at other points than the reference's, so the fitted time constant differs by an ABSOLUTE
    delta (nine terms, 2^-24 of their magnitudes each: for tau_h the magnitudes add up to 600 - 1000 between -90 and -84 mV
    and above 25 mV, delta ~ 1e-4).  The reference's fit of tau_h is no time constant there: it
    runs through zero at -88.1 and -83.9 mV (0.034 at -88.12, -0.65 at rest).  The update g + (g - g_inf) expm1(-dt / tau)
    turns delta into |g - g_inf| delta (dt / tau^2) exp(-dt / tau), which over tau peaks at tau = dt / 2 with
    |g - g_inf| delta 4 e^-2 / dt: where the fit passes through zero some cell sits near that peak, and the error grows
    as 1 / dt.  At 0.1 ms the cell at -88.12 mV is past the peak (dt / tau = 3, measured 6.9e-5 there); at 0.02 - 0.05 it is
    on it.  Measured, one sub-step, h, one cell (V = -88.12, tau fit 0.034, |h - h_inf| = 0.80): 1.27e-4 at dt 0.02
    (bound 5e-4), 1.42e-4 at 0.03 (3.3e-4), 1.31e-4 at 0.05 (2e-4), 3.9e-5 at 0.2 (2e-4); at most one other cell above 3e-5,
    and the rounding-faithful policy 6e-8 everywhere.  Nothing of this comes from a constant of fibhip_create."""
    return max(dt / 0.1, 0.1 / dt)


def court_masks(V0):
    """cells within 0.06 mV of a removable singularity of calc_inter (court.py:303-410), and those exactly on one"""
    near = np.zeros(V0.shape, bool)
    exact = np.zeros(V0.shape, bool)
    for s in SINGULAR:
        near |= np.abs(V0 - np.float32(s)) < 0.06
        exact |= V0 == np.float32(s)
    return near, exact


def court_step_figures(out, c, chronic, policy, orc, names, device):
    """away from the singularities: the plain bound.  Near one: inside the oracle's own sensitivity envelope there (the
    step re-evaluated with exp() within one ulp and every potential within two float32 neighbours), widened by three times
    its width plus the plain bound — tests/test_gpu_parity.test_court_single_step; the figure is the distance from the
    envelope over that margin.  device=False checks the reference's values against the envelope (test_oracle_golden)."""
    from test_oracle_golden import court_envelope_samples
    tagc = 'chronic' if chronic else 'acute'
    slab = np.stack([c[k] for k in names])
    near, exact = court_masks(orc.enforce_boundary(c['V']))
    ok = ~near | exact
    samples = court_envelope_samples(orc, slab, c['phase'], chronic, c['dt'], c['diff'])
    figs = []
    for i, k in enumerate(names):
        want = c['%s_1_%s' % (k, tagc)].astype(np.float64)
        tol = STEP_TOL[policy] * room(c['dt']) * COURT_STEP_SCALES.get(k, 1.0)
        got = np.asarray(out[i], np.float64)
        fin = np.isfinite(got).all()
        figs.append(('court %s %s' % (tagc, k), float(np.abs(got - want)[ok].max()) if fin else float('inf'), tol))
        lo, hi = samples[:, i].min(axis=0), samples[:, i].max(axis=0)
        if device:
            lo, hi, x = np.minimum(lo, want), np.maximum(hi, want), got
        else:
            x = want
        margin = 3.0 * (hi - lo) + tol
        dist = np.maximum(np.maximum(lo - x, x - hi), 0.0) / margin
        figs.append(('court %s %s near a singularity' % (tagc, k), float(dist[near].max()) if fin else float('inf'), 1.0))
    return figs


# ------------------------------------------------------------------------------------------------
# figures: trajectories (snapshots: dict tick -> [nvar, H, W])
# ------------------------------------------------------------------------------------------------
def span(a):
    return max(float(np.max(a) - np.min(a)), 1e-30)


def fenton_traj_figures(snaps, f):
    return [('fenton %s t%d' % (k, t), maxerr(s[i], f['%s_t%d' % (k, t)]), TRAJ_TOL)
            for t, s in snaps.items() for i, k in enumerate('UVWS')]


def br_traj_figures(snaps, f, tag, policy):
    """test_br_trajectory_64's bounds: 2e-5 of range, twice that under the fast policy with Chebyshev gates.
    NAMED EXCEPTION — fast policy, Chebyshev gates, M and H: that 4e-5 times fit_room(dt).  H: the foot of every wave takes
    cells through -83.9 mV, where the fitted tau_h passes through zero and the 1 / dt law of fit_room holds (96 cells of two
    columns at dt 0.02).  M: it follows the cell's own potential with the slope of m_inf, 0.011 per mV at -27 mV, and the
    potential's bound is 120 mV * 4e-5 = 4.8e-3 mV: 4.48e-5 measured beside a potential 2.8e-3 mV off.
    Measured (bound): H 1.00e-4 (2e-4) at (0.02, 0.809) skip; M 4.48e-5, H 4.05e-5 (8e-5) at (0.05, 1.6) skip;
    H 4.34e-5 (8e-5) at (0.2, 0.4); every other figure of the fast policy <= 2.7e-5 / 4e-5, of the rounding-faithful one
    <= 6.8e-6 / 2e-5."""
    cheby_fast = policy == 'fast' and tag.startswith('cheby')
    figs = []
    for t, s in snaps.items():
        for i, k in enumerate(BR_VARS):
            want = f['%s_%s_t%d' % (tag, k, t)]
            scale = {'V': 120.0, 'C': max(span(want), float(np.abs(want).max()))}.get(k, 1.0)
            rel = TRAJ_TOL * (2 if cheby_fast else 1) * (fit_room(float(f['dt'])) if cheby_fast and k in 'MH' else 1)
            figs.append(('br %s %s t%d' % (tag, k, t), maxerr(s[i], want), rel * scale))
    return figs


def court_traj_figures(snaps, trend, f, names, scales=COURT_TRAJ_SCALES, what='court'):
    """test_court_trajectory's scales and 2e-5.  The snapshots of the multirate model are taken right behind a 'slow', which
    evaluated calc_inter on the very potentials of the snapshot: a cell that 'slow' met within 0.06 mV of a removable
    singularity (court.py:303-410) got slow variables that are noise in the reference itself, and is left out for the 17
    variables 'slow' assigns, as test_gpu_parity.test_court_single_step leaves such cells out.  One cell of the fixtures is
    one: (15, 27) of (0.2, 0.4) at tick 21, V = 3.3327 beside tau_xr's 0/0 at 3.3328 — _xr_ 2.8e-5 under the fast policy."""
    figs = []
    for t, s in snaps.items():
        near, exact = court_masks(f['V_t%d' % t])
        near = near & ~exact if what == 'court' else np.zeros(near.shape, bool)
        for i, k in enumerate(names):
            keep = ~near if i >= 4 else np.ones(near.shape, bool)
            figs.append(('%s %s t%d' % (what, k, t), maxerr(s[i][keep], f['%s_t%d' % (k, t)][keep]), TRAJ_TOL * scales.get(k, 1.0)))
    if trend is not None:
        trend = np.asarray(trend)
        assert trend.shape == f['trend'].shape
        figs.append(('court trend V', maxerr(trend[:, 0], f['trend'][:, 0]), 2e-4 * 150.0))
        figs.append(('court trend Na_i', maxerr(trend[:, 1], f['trend'][:, 1]), 2e-4))
    return figs


# ------------------------------------------------------------------------------------------------
# the oracle's side of every comparison
# ------------------------------------------------------------------------------------------------
def oracle_fenton_traj(orc, f):
    slab = np.stack([f['init_' + k] for k in 'UVWS']).copy()
    snaps, t0 = {}, 0
    for t in [int(x) for x in f['snap_ticks']]:
        orc.fenton_run(slab, float(f['dt']), float(f['diff']), f['phase'], 10 * (t - t0))
        snaps[t], t0 = slab.copy(), t
    return snaps


def oracle_br_traj(orc, f, tag, tbl):
    slab = np.stack([f['init_' + k] for k in BR_VARS]).copy()
    snaps, t0 = {}, 0
    for t in [int(x) for x in f['snap_ticks']]:
        orc.br_run(slab, float(f['dt']), float(f['diff']), f['phase'], tbl if tag.startswith('cheby') else None,
                   tag.endswith('skip'), t - t0)
        snaps[t], t0 = slab.copy(), t
    return snaps


def luq(H, W):
    return 1, H // 2, 1, W // 2                        # IonicModel.pace_rect('luq')


def oracle_court_traj(orc, f, names):
    slab = np.stack([f['init_' + k] for k in names]).copy()
    H, W = slab.shape[1:]
    snaps, trend = {}, []
    want = [int(x) for x in f['snap_ticks']]
    for i in range(max(want)):
        orc.court_run(slab, float(f['dt']), float(f['diff']), f['phase'], True, i, 1)
        if i % 10 == 0:
            trend.append([slab[0][W // 2, 20], slab[1][W // 2, 20]])
        if i == S2_TICK:
            slab[0] = orc.pace(slab[0], *luq(H, W), 10.0, -100.0)
        if i + 1 in want:
            snaps[i + 1] = slab.copy()
    return snaps, np.array(trend, np.float32)


def oracle_court_ultra_traj(orc, f, names):
    slab = np.stack([f['init_' + k] for k in names]).copy()
    snaps, t0 = {}, 0
    for t in [int(x) for x in f['snap_ticks']]:
        orc.court_ultra_run(slab, float(f['dt']), float(f['diff']), f['phase'], True, t - t0)
        snaps[t], t0 = slab.copy(), t
    return snaps


# ------------------------------------------------------------------------------------------------
# the device's side: through the model classes, as tests/test_gpu_parity.py goes
# ------------------------------------------------------------------------------------------------
def device_cfg(h, w, dt, diff, policy, **kw):
    c = {'dt': dt, 'dt_per_plot': 10, 'duration': 1000, 'timeline': False, 'timeline_name': 'unused.json', 'save_graph': False,
         'skip': False, 'cheby': False, 'height': h, 'width': w, 'diff': diff, 'fast_math': policy == 'fast'}
    c.update(kw)
    return c


def run_to(model, ticks, hook=None):
    model.duration = ticks * model.dt_per_step * model.dt + 1e-9
    for i in model.run():
        if hook:
            hook(i)


def device_fenton_step(c, policy):
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v(device_cfg(*c['U'].shape, c['dt'], c['diff'], policy))
    m.phase = c['phase']
    return m.solve(tuple(c[k] for k in 'UVWS'))


def device_br_step(c, tag, n, policy):
    from fib_tf_amd.br import BeelerReuter
    m = BeelerReuter(device_cfg(*c['V'].shape, c['dt'], c['diff'], policy, cheby=(tag == 'cheby')))
    m.phase = c['phase']
    return m.solve(tuple(c[k] for k in BR_VARS), n)


def device_court_step(c, chronic, policy):
    from fib_tf_amd.court import Courtemanche
    m = Courtemanche(device_cfg(*c['V'].shape, c['dt'], c['diff'], policy))
    m.chronic = chronic
    m.phase = c['phase']
    out = m.solve({k: c[k] for k in m.VAR_NAMES})
    return [out[k] for k in m.VAR_NAMES]


def _play(m, f, hook=None):
    """define()'s initial state bit for bit, then the fixture's snapshots"""
    for k in m.VAR_NAMES:
        assert np.array_equal(m._State[k].eval(), f['init_' + k]), 'initial %s' % k
    snaps, t0 = {}, 0
    for t in [int(x) for x in f['snap_ticks']]:
        run_to(m, t - t0, (lambda i, t0=t0: hook(i + t0)) if hook else None)
        snaps[t], t0 = np.stack([m._State[k].eval() for k in m.VAR_NAMES]), t
    return snaps


def device_fenton_traj(f, policy):
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v(device_cfg(*f['phase'].shape, float(f['dt']), float(f['diff']), policy))
    m.add_hole_to_phase_field(*[float(x) for x in f['hole']])
    assert np.array_equal(m.phase, f['phase'])
    m.define()
    return _play(m, f)


def device_br_traj(f, tag, policy):
    from fib_tf_amd.br import BeelerReuter
    m = BeelerReuter(device_cfg(*f['phase'].shape, float(f['dt']), float(f['diff']), policy, cheby=tag.startswith('cheby'),
                                skip=tag.endswith('skip')))
    m.add_hole_to_phase_field(*[float(x) for x in f['hole']])
    assert np.array_equal(m.phase, f['phase'])
    m.define()
    return _play(m, f)


def device_court_traj(f, policy):
    """fast tick every iteration, 'slow' + 'trend' every 10th (court.py:615-621), S2 after tick S2_TICK"""
    from fib_tf_amd.court import Courtemanche
    m = Courtemanche(device_cfg(*f['phase'].shape, float(f['dt']), float(f['diff']), policy))
    m.phase = f['phase']
    m.define()
    m.add_pace_op('s2', 'luq', 10.0)
    trend = []

    def hook(g):
        if g % 10 == 0:
            m.fire_op('slow')
            m.fire_op('trend')
            trend.append(m._Trend.eval())
        if g == S2_TICK:
            m.fire_op('s2')

    return _play(m, f, hook), np.array(trend)


def device_court_ultra_traj(f, policy):
    from fib_tf_amd import court_ultra
    m = court_ultra.Courtemanche(device_cfg(*f['phase'].shape, float(f['dt']), float(f['diff']), policy, ultra_slow=False))
    m.phase = f['phase']
    m.define()
    return _play(m, f)


def oracle_figures(orc, golden):
    """every new fixture against the oracle under the exact policy's bounds: {section: figures}"""
    names = list(orc.COURT_VARS)
    tbl = cheby_table(golden)
    out = {}
    for p in range(NPAIRS):
        c = fenton_step_case(golden, p)
        got = orc.fenton_step(np.stack([c[k] for k in 'UVWS']), c['dt'], c['diff'], c['phase'])
        out['step fenton ' + pair_id('fenton', p)] = fenton_step_figures(got, c, 'exact')
        c = br_step_case(golden, p)
        figs = []
        for tag in ('direct', 'cheby'):
            for n in (1, 5, 0):
                got = orc.br_step(np.stack([c[k] for k in BR_VARS]), c['dt'], c['diff'], c['phase'],
                                  tbl if tag == 'cheby' else None, n)
                figs += br_step_figures(got, c, tag, n, 'exact')
        out['step br ' + pair_id('br', p)] = figs
        c = court_step_case(golden, p, names)
        figs = []
        for chronic in (True, False):
            got = orc.court_step(np.stack([c[k] for k in names]), c['dt'], c['diff'], c['phase'], chronic)
            figs += court_step_figures(got, c, chronic, 'exact', orc, names, device=False)
        out['step court ' + pair_id('court', p)] = figs
        f = golden('ts_fenton_traj_p%d' % p)
        out['traj fenton ' + pair_id('fenton', p)] = fenton_traj_figures(oracle_fenton_traj(orc, f), f)
        f = golden('ts_br_traj_p%d' % p)
        figs = []
        for tag in BR_TAGS:
            figs += br_traj_figures(oracle_br_traj(orc, f, tag, tbl), f, tag, 'exact')
        out['traj br ' + pair_id('br', p)] = figs
        f = golden('ts_court_traj_p%d' % p)
        snaps, trend = oracle_court_traj(orc, f, names)
        out['traj court ' + pair_id('court', p)] = court_traj_figures(snaps, trend, f, names)
        f = golden('ts_court_ultra_traj_p%d' % p)
        out['traj court_ultra ' + pair_id('court', p)] = court_traj_figures(
            oracle_court_ultra_traj(orc, f, names), None, f, names, COURT_ULTRA_SCALES, 'court_ultra')
    return out
