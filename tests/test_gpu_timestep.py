"""-m gpu: the hand-written models at time steps and diffusion coefficients other than 0.1 ms.

`dt` is folded into more host-side constants than any other value (fibhip_create, csrc/fibhip.hip: Fenton's 1 - dt/tau
factors, Beeler-Reuter's -dt and -(5 dt), Courtemanche's 10 dt, its two expm1 constants and the aggregates' -dt log2 e, and
float(diff * dt) for all three; the traced generator folds them a second time in Python).  Every other parity test runs at
dt = 0.1, where a constant formed for 0.1, from the wrong step or rounded twice is invisible.

(dt, diff) pairs per model: two steps below 0.1, one above, one without diffusion (tests/timestep_cases.py PAIRS);
fixtures tests/golden/ts_*.npz from the reference's own solve() and define() (tests/golden/make_golden.py section 4).

Tolerances (tests/test_gpu_parity.py has the rule):
  * one sub-step: STEP_TOL[policy] * max(1, dt / 0.1) of range; steps below 0.1 get no extra room
  * trajectories of 20 ticks: 2e-5 of range, as at 0.1
  * one named exception to both, the fast policy with Chebyshev gates (timestep_cases.fit_room has the arithmetic and the
    measured values): H in one sub-step, M and H along a trajectory scale with max(dt / 0.1, 0.1 / dt)
  * one tick of a seeded 70 x 130 state against the oracle at the same dt: TICK_TOL below
  * kernel forms against each other, the traced twin of Fenton, diff = 0 under a permutation of the cells: bit for bit
  * the diffusion constant the device applies, measured by regression: within 2^-25 of float(diff * dt)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timestep_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

POLICIES = tc.POLICIES
PAIR_IDS = {m: [tc.pair_id(m, p) for p in range(tc.NPAIRS)] for m in tc.PAIRS}
ENV = ('FIBHIP_MT', 'FIBHIP_MT_MAX', 'FIBHIP_VARIANT', 'FIBHIP_AHEAD', 'FIBHIP_AUTOTUNE', 'FIBHIP_NO_MULTI', 'FIBHIP_NO_LAZY',
       'FIBHIP_COURT_AGG')


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def flags(policy):
    from fib_tf_amd import _lib
    return _lib.FAST if policy == 'fast' else 0


# --------------------------------------------------------------------------------------------
# one sub-step against the reference
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['fenton'])
def test_fenton_single_step(gpu_lib, golden, p, policy):
    c = tc.fenton_step_case(golden, p)
    out = tc.device_fenton_step(c, policy)
    tc.check(tc.fenton_step_figures(out, c, policy))
    if policy == 'exact':       # V and W never pass through a transcendental: bit for bit at every dt
        assert np.array_equal(out[1], c['V1'])
        assert np.array_equal(out[2], c['W1'])


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('tag', ['direct', 'cheby'])
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['br'])
def test_br_single_step(gpu_lib, golden, p, tag, policy):
    """n = 1, 5 (the slow gates advance 5 dt: the first sub-step of a skip tick) and 0 (they are carried over)"""
    c = tc.br_step_case(golden, p)
    for n in (1, 5, 0):
        out = tc.device_br_step(c, tag, n, policy)
        tc.check(tc.br_step_figures(out, c, tag, n, policy))
        if n == 0:
            for k, o in zip(tc.BR_VARS, out):
                if k in tc.BR_SLOW:
                    assert np.array_equal(o, c[k]), k


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('chronic', [True, False], ids=['chronic', 'acute'])
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['court'])
def test_court_single_step(gpu_lib, golden, orc, p, chronic, policy):
    """all 21 outputs: the fast set advanced by dt, the slow set by 10 dt"""
    c = tc.court_step_case(golden, p, orc.COURT_VARS)
    out = tc.device_court_step(c, chronic, policy)
    tc.check(tc.court_step_figures(out, c, chronic, policy, orc, list(orc.COURT_VARS), device=True))


# --------------------------------------------------------------------------------------------
# 20 ticks through define() / run() against the reference
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['fenton'])
def test_fenton_trajectory(gpu_lib, golden, p, policy):
    f = golden('ts_fenton_traj_p%d' % p)
    tc.check(tc.fenton_traj_figures(tc.device_fenton_traj(f, policy), f))


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('tag', tc.BR_TAGS)
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['br'])
def test_br_trajectory(gpu_lib, golden, p, tag, policy):
    f = golden('ts_br_traj_p%d' % p)
    tc.check(tc.br_traj_figures(tc.device_br_traj(f, tag, policy), f, tag, policy))


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['court'])
def test_court_trajectory(gpu_lib, golden, orc, p, policy):
    """21 ticks: 'slow' and the 'trend' probe at ticks 0, 10 and 20, S2 after tick 12"""
    f = golden('ts_court_traj_p%d' % p)
    snaps, trend = tc.device_court_traj(f, policy)
    tc.check(tc.court_traj_figures(snaps, trend, f, list(orc.COURT_VARS)))


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['court'])
def test_court_ultra_trajectory(gpu_lib, golden, orc, p, policy):
    """single rate: every tick assigns all 21 variables with dt (the expm1 constants are formed from dt, not 10 dt)"""
    f = golden('ts_court_ultra_traj_p%d' % p)
    tc.check(tc.court_traj_figures(tc.device_court_ultra_traj(f, policy), None, f, list(orc.COURT_VARS), tc.COURT_ULTRA_SCALES,
                                   'court_ultra'))


# --------------------------------------------------------------------------------------------
# one tick of a seeded state on 70 x 130 against the oracle at the same dt
# --------------------------------------------------------------------------------------------
# test_gpu_parity.test_br_vs_oracle_random_state allows the rounding-faithful policy 1e-5 of range for a tick (5e-5 with the
# Chebyshev gates).  The fast policy is given the same multiple of its one-step bound: 1e-5 * 3e-5 / 4e-6.
TICK_TOL = {'exact': 1e-5, 'fast': 1e-5 * tc.STEP_TOL['fast'] / tc.STEP_TOL['exact']}
BIG = (70, 130)


def clear_of_br_singular(V):
    """0.5 mV clearance from the 0/0 voltages of alpha_m and alpha_x1, which are not this file's subject: one ulp of exp there
    is a relative rate error of 6e-7 / distance (tests/golden/make_golden.py timestep_steps)"""
    for s in (-47.0, -23.0):
        close_by = np.abs(V - np.float32(s)) < 0.5
        V[close_by] = np.where(V[close_by] < s, np.float32(s - 0.5), np.float32(s + 0.5))
    return V


@pytest.fixture(scope='module')
def big_states():
    return make_big_states()


def make_big_states():
    H, W = BIG
    rng = np.random.default_rng(77)
    fe = np.stack([rng.uniform(-0.05, 1.05, (H, W)), rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W)),
                   rng.uniform(0, 1, (H, W))]).astype(np.float32)
    br = np.empty((8, H, W), np.float32)
    br[0] = clear_of_br_singular(rng.uniform(-85, 25, (H, W)).astype(np.float32))
    br[1] = np.exp(rng.uniform(np.log(1e-7), np.log(1e-5), (H, W)))
    br[2:] = rng.uniform(1e-5, 0.99999, (6, H, W))
    co = rng.uniform(1e-5, 0.99999, (21, H, W)).astype(np.float32)
    co[0] = rng.uniform(-100.0, 50.0, (H, W))
    co[1] = rng.uniform(10.0, 13.0, (H, W))
    co[5] = rng.uniform(130.0, 145.0, (H, W))
    co[12] = np.exp(rng.uniform(np.log(5e-5), np.log(1e-3), (H, W)))
    co[16] = rng.uniform(0.5, 2.0, (H, W))
    co[20] = rng.uniform(1.0, 2.0, (H, W))
    phi = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
    for a in (fe, br, co, phi):
        a.setflags(write=False)
    return {'fenton': fe, 'br': br, 'court': co, 'phi': phi}


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['fenton'])
def test_fenton_vs_oracle_random_state(gpu_lib, orc, big_states, p, policy):
    from fib_tf_amd import _lib
    dt, diff = tc.PAIRS['fenton'][p]
    st = _lib.Stepper(_lib.FENTON4V, *BIG, dt, diff, flags=flags(policy))
    st.set_phase(big_states['phi'])
    st.set_state(-1, big_states['fenton'])
    st.step(1)
    got = st.get_state(-1)
    st.close()
    ref = big_states['fenton'].copy()
    orc.fenton_run(ref, dt, diff, big_states['phi'], 10)
    tol = TICK_TOL[policy] * tc.room(dt)
    tc.check([('fenton %s' % k, tc.maxerr(got[i], ref[i]), tol) for i, k in enumerate('UVWS')])


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['br'])
def test_br_vs_oracle_random_state(gpu_lib, orc, big_states, p, policy):
    """both gate paths, both multirate modes.  With the direct gates, a cell whose potential stands within 0.1 mV of a 0/0
    voltage of the rate formulas (-47 mV alpha_m, -23 mV alpha_x1) at the start of one of the five sub-steps is left out: one
    ulp of exp is a relative rate error of 6e-7 / distance there, in the oracle as on the device.  The potentials of a
    seeded state move by several mV per sub-step, so the initial clearance does not last: (0.02, 0.809) has a cell at
    -46.995 mV before the fifth sub-step (m 1.4e-5 off), (0.03, 0) with skip one at -46.999 (5.8e-5); no other cell is
    above 1e-5."""
    from fib_tf_amd.br import BeelerReuter
    dt, diff = tc.PAIRS['br'][p]
    figs = []
    for cheby in (False, True):
        for skip in (False, True):
            m = BeelerReuter(tc.device_cfg(*BIG, dt, diff, policy, cheby=cheby, skip=skip))
            m.phase = big_states['phi']
            m.define()
            m._stepper.set_state(-1, big_states['br'])
            tc.run_to(m, 1)
            got = m._stepper.get_state()
            tbl = m.chebyshev_table().astype(np.float32) if cheby else None
            ref = big_states['br'].copy()
            keep = np.ones(BIG, bool)
            for n in range(5):                              # the oracle's tick, sub-step by sub-step (br.py:98-107)
                V0 = orc.enforce_boundary(ref[0])
                if not cheby:
                    keep &= (np.abs(V0 + 47.0) >= 0.1) & (np.abs(V0 + 23.0) >= 0.1)
                ref = orc.br_step(ref, dt, diff, big_states['phi'], tbl, ((5 if n == 0 else 0) if skip else 1))
            whole = big_states['br'].copy()
            orc.br_run(whole, dt, diff, big_states['phi'], tbl, skip, 1)
            assert np.array_equal(whole, ref) and keep.mean() > 0.95
            tol = TICK_TOL[policy] * (5 if cheby else 1) * tc.room(dt)
            what = 'br cheby=%s skip=%s ' % (cheby, skip)
            figs += [(what + 'V', tc.maxerr(got[0][keep], ref[0][keep]), tol * 120.0),
                     (what + 'C', tc.maxerr(got[1][keep], ref[1][keep]), tol * 1e-5),
                     (what + 'gates', tc.maxerr(got[2:][:, keep], ref[2:][:, keep]), tol)]
    tc.check(figs)


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('slow', [True, False], ids=['with-slow', 'fast-only'])
@pytest.mark.parametrize('p', range(4), ids=PAIR_IDS['court'])
def test_court_vs_oracle_random_state(gpu_lib, orc, big_states, p, slow, policy):
    """a tick with 'slow' behind it (tick 0) and one without; cells within 0.06 mV of a removable singularity of calc_inter —
    before the tick or, for 'slow', after it — are left out (tests/test_gpu_parity.test_court_single_step has their story)"""
    from fib_tf_amd import _lib
    dt, diff = tc.PAIRS['court'][p]
    st = _lib.Stepper(_lib.COURT, *BIG, dt, diff, flags=flags(policy) | _lib.CHRONIC)
    st.set_phase(big_states['phi'])
    st.set_state(-1, big_states['court'])
    st.step(1)
    if slow:
        st.step_slow()
    got = st.get_state(-1)
    st.close()
    ref = big_states['court'].copy()
    orc.court_run(ref, dt, diff, big_states['phi'], True, 0 if slow else 1, 1)
    near = tc.court_masks(orc.enforce_boundary(big_states['court'][0]))[0] | tc.court_masks(orc.enforce_boundary(ref[0]))[0]
    assert near.sum() < 0.02 * near.size
    assert np.isfinite(got).all()
    tol = TICK_TOL[policy] * tc.room(dt)
    tc.check([('court %s' % k, tc.maxerr(got[i][~near], ref[i][~near]), tol * tc.COURT_STEP_SCALES.get(k, 1.0))
              for i, k in enumerate(orc.COURT_VARS)])
    if not slow:
        assert np.array_equal(got[4:], big_states['court'][4:])      # the slow set waits for 'slow'


# --------------------------------------------------------------------------------------------
# the diffusion constant the kernels apply is float(diff * dt)
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('model,p', [(m, p) for m in ('fenton', 'br', 'court') for p in (0, 1, 2)])
def test_applied_diffusion_constant(gpu_lib, orc, model, p, policy):
    """A diffusion constant that is off by one float32 neighbour — diff and dt rounded before they are multiplied, say —
    changes a potential by 1e-7 of ddt * laplace(V): two orders below any tolerance here, and below one ulp of the potential.
    It is systematic, though, so 37 500 cells show it: the slope of (device - oracle) against ddt * N, with N the neighbours'
    share of the Laplacian (the Laplacian without its centre weight — a sum over other cells, so independent of everything
    the cell's own kinetics see), estimates the relative error of the constant.  A wrong rounding moves float(diff * dt) by
    at least 2^-24 of itself; the rounding of the new potentials (ulp <= 4.8e-7 for |V| < 8) leaves the estimate a noise of
    sqrt(ulp * 2^-24 / (cells * rms(ddt N))) <= 5e-9.  Bound: 2^-25 = 3e-8, six such deviations from both.
    One sub-step; potentials seeded in a narrow band around zero, every other variable at rest."""
    dt, diff = tc.PAIRS[model][p]
    eps, worst = applied_diffusion_error(orc, model, p, policy)
    assert worst <= tc.STEP_TOL[policy] * tc.room(dt) * {'fenton': 1.0, 'br': 120.0, 'court': 150.0}[model]
    assert abs(eps) <= 2.0 ** -25, 'the diffusion constant applied is off by %.3g of float(diff * dt) = %.9g' % (
        eps, float(np.float32(diff * dt)))


def applied_diffusion_error(orc, model, p, policy):
    """(relative error of the applied diffusion constant as the regression estimates it, max |device - oracle|)"""
    from fib_tf_amd import _lib
    from fib_tf_amd.court import INITIAL
    H, W = 150, 250
    dt, diff = tc.PAIRS[model][p]
    rng = np.random.default_rng(1000 + p)
    if model == 'fenton':
        mid, nvar, rest = _lib.FENTON4V, 4, [0.0, 1.0, 1.0, 0.0]
        v = rng.uniform(0.0, 1.0, (H, W))
    elif model == 'br':
        mid, nvar, rest = _lib.BR, 8, [-84.624, 1e-4, 0.01, 0.988, 0.975, 0.003, 0.994, 0.0001]
        v = rng.uniform(-8.0, 8.0, (H, W))
    else:
        mid, nvar, rest = _lib.COURT, 21, [x for _, x in INITIAL]
        v = rng.uniform(-8.0, 8.0, (H, W))
    state = np.empty((nvar, H, W), np.float32)
    for i, x in enumerate(rest):
        state[i] = x
    state[0] = v
    st = _lib.Stepper(mid, H, W, dt, diff, flags=flags(policy) | (_lib.CHRONIC if model == 'court' else 0), steps_per_tick=1)
    st.set_state(-1, state)
    st.step(1)
    got = st.get_state(0).astype(np.float64)
    st.close()
    if model == 'fenton':
        ref = orc.fenton_step(state, dt, diff)[0]
    elif model == 'br':
        ref = orc.br_step(state, dt, diff, None, None, 1)[0]
    else:
        ref = orc.court_step(state, dt, diff, None, True)[0]
    V0 = orc.enforce_boundary(state[0])
    delta = np.zeros((5, 5), np.float32)
    delta[2, 2] = 1.0
    centre = float(orc.laplace(delta)[2, 2])                          # the stencil's weight of the cell itself
    N = orc.laplace(V0).astype(np.float64) - centre * V0.astype(np.float64)
    ddt = float(np.float32(diff * dt))
    inner = (slice(2, -2), slice(2, -2))
    x = (ddt * N)[inner]
    x = x - x.mean()
    d = (got - ref.astype(np.float64))[inner]
    return float((x * d).sum() / (x * x).sum()), float(np.abs(d).max())


# --------------------------------------------------------------------------------------------
# kernel forms agree bit for bit at a time step other than 0.1
# --------------------------------------------------------------------------------------------
FORM_PAIRS = [0, 2]                                       # (0.02, .) and (0.2, .)
FORM_SHAPES = [(45, 70), (70, 130)]
TICKS = 12


def _same(results, base):
    for name, r in results.items():
        assert np.isfinite(r).all(), name
        assert np.array_equal(r, results[base]), '%s differs from %s (max |d| %.3g)' % (name, base,
                                                                                       float(np.abs(r - results[base]).max()))


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('H,W', FORM_SHAPES)
@pytest.mark.parametrize('p', FORM_PAIRS, ids=[PAIR_IDS['fenton'][p] for p in FORM_PAIRS])
def test_fenton_kernel_forms_bit_identical(gpu_lib, monkeypatch, p, H, W, policy):
    """one launch per tick (FIBHIP_MT=0), the default plan, a K=10 strip row and the K=1 row of the variant table, and a
    declared series: 12 ticks of a seeded state with a phase field, a pace after the fifth"""
    from fib_tf_amd import _lib
    dt, diff = tc.PAIRS['fenton'][p]
    rng = np.random.default_rng(7 * H + W)
    init = np.stack([rng.uniform(-0.02, 1.0, (H, W)), rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W)),
                     rng.uniform(0, 1, (H, W))]).astype(np.float32)
    phi = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
    results = {}
    for name, env, declare in (('one launch per tick', {'FIBHIP_MT': '0'}, False), ('default plan', {}, False),
                               ('K=10 strip', {'FIBHIP_VARIANT': '10,44,25,-3'}, False),
                               ('K=1', {'FIBHIP_VARIANT': '1,64,4,256'}, False), ('declared series', {}, True)):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            st = _lib.Stepper(_lib.FENTON4V, H, W, dt, diff, flags=flags(policy))
            st.set_phase(phi)
            st.set_state(-1, init)
            st.step(5)
            st.pace(H // 4, H // 4 + 5, W // 3, W // 3 + 6, 1.0, 0.0)
            if declare:
                st.expect(TICKS - 5)
            for _ in range(TICKS - 5):
                st.step(1)
            results[name] = st.get_state(-1)
            st.close()
    _same(results, 'one launch per tick')


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('cheby,skip', [(True, True), (False, False)], ids=['cheby-skip', 'direct'])
@pytest.mark.parametrize('H,W', FORM_SHAPES)
@pytest.mark.parametrize('p', FORM_PAIRS, ids=[PAIR_IDS['br'][p] for p in FORM_PAIRS])
def test_br_kernel_forms_bit_identical(gpu_lib, monkeypatch, big_states, p, H, W, cheby, skip, policy):
    """the same forms as for Fenton, and with the Chebyshev gates the build with the table compiled in against the stock one"""
    from fib_tf_amd.br import BeelerReuter
    dt, diff = tc.PAIRS['br'][p]
    init = np.ascontiguousarray(big_states['br'][:, :H, :W])
    phi = np.ascontiguousarray(big_states['phi'][:H, :W])
    forms = [('one launch per tick', {'FIBHIP_MT': '0'}, False, False), ('default plan', {}, False, False),
             ('K=5 strip', {'FIBHIP_VARIANT': '5,54,21,-2'}, False, False), ('K=1', {'FIBHIP_VARIANT': '1,64,4,256'}, False, False),
             ('declared series', {}, True, False)]
    if cheby:
        forms.append(('table compiled in', {}, False, True))
    results = {}
    for name, env, declare, spec in forms:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m = BeelerReuter(tc.device_cfg(H, W, dt, diff, policy, cheby=cheby, skip=skip, specialise=spec))
            m.phase = phi
            m.define()
            assert (m._library is not None) == spec
            st = m._stepper
            st.set_state(-1, init)
            st.step(5)
            st.pace(0, H // 2, 0, W // 2, 10.0, -100.0)
            if declare:
                st.expect(TICKS - 5)
            for _ in range(TICKS - 5):
                st.step(1)
            results[name] = st.get_state(-1)
            st.close()
    _same(results, 'one launch per tick')


def _court_play(H, W, dt, diff, policy, ticks=TICKS):
    """`ticks` fast ticks, 'slow' after every 10th, one pace: tests/test_gpu_parity._court_run at another time step"""
    from fib_tf_amd import _lib
    from fib_tf_amd.court import INITIAL
    rng = np.random.default_rng(11)
    init = np.empty((21, H, W), np.float32)
    for i, (_, v) in enumerate(INITIAL):
        init[i] = v
    init[0] += rng.uniform(-5, 60, (H, W)).astype(np.float32)
    phi = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
    st = _lib.Stepper(_lib.COURT, H, W, dt, diff, flags=flags(policy))
    st.set_phase(phi)
    st.set_state(-1, init)
    snaps = []
    for i in range(ticks):
        st.step(1)
        if i % 10 == 0:
            st.step_slow()
        if i == 4:
            st.pace(0, max(1, H // 2), 0, max(1, W // 2), 10.0, -100.0)
        if i in (0, 6, 10, ticks - 1):
            snaps.append(st.get_state(-1))
    st.close()
    return snaps


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('H,W', FORM_SHAPES)
@pytest.mark.parametrize('p', FORM_PAIRS, ids=[PAIR_IDS['court'][p] for p in FORM_PAIRS])
def test_court_launch_forms_bit_identical(gpu_lib, monkeypatch, p, H, W, policy):
    """two- and three-tick launches and the tick fused with 'slow' against one launch per tick and op
    (FIBHIP_NO_MULTI=1, FIBHIP_NO_LAZY=1)"""
    dt, diff = tc.PAIRS['court'][p]
    a = _court_play(H, W, dt, diff, policy)
    monkeypatch.setenv('FIBHIP_NO_MULTI', '1')
    monkeypatch.setenv('FIBHIP_NO_LAZY', '1')
    b = _court_play(H, W, dt, diff, policy)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.isfinite(x).all()
        assert np.array_equal(x, y), 'observation %d differs (max |d| %.3g)' % (i, float(np.abs(x - y).max()))


COURT_SCALES = [150.0, 1.0] + [1.0] * 3 + [1.0] + [1.0] * 6 + [1e-3] + [1.0] * 3 + [1.5] + [1.0] * 3 + [1.0]
COURT_CALCIUM = (12, 15, 16, 17, 18, 19, 20)


@pytest.mark.parametrize('H,W', FORM_SHAPES)
@pytest.mark.parametrize('p', FORM_PAIRS, ids=[PAIR_IDS['court'][p] for p in FORM_PAIRS])
def test_court_aggregated_fast_tick(gpu_lib, monkeypatch, p, H, W):
    """the aggregates fold -dt log2 e: against the plain kernels (FIBHIP_COURT_AGG=0) within the bound of
    tests/test_gpu_parity.test_court_aggregated_fast_tick"""
    dt, diff = tc.PAIRS['court'][p]
    a = _court_play(H, W, dt, diff, 'fast')
    monkeypatch.setenv('FIBHIP_COURT_AGG', '0')
    b = _court_play(H, W, dt, diff, 'fast')
    figs = []
    for i, (sa, sb) in enumerate(zip(a, b)):
        for v in range(21):
            rel = 1e-3 if v in COURT_CALCIUM else (2e-5 if v in (0, 1, 5) else 2e-4)
            figs.append(('observation %d var %d' % (i, v), tc.maxerr(sa[v], sb[v]), rel * COURT_SCALES[v]))
    tc.check(figs)


# --------------------------------------------------------------------------------------------
# the traced twins: the generator folds the same constants a second time, in Python
# --------------------------------------------------------------------------------------------
@pytest.fixture
def _restore_modules():
    saved = {k: sys.modules.get(k) for k in ('tensorflow', 'ionic', 'screen')}
    yield
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


@pytest.mark.parametrize('p', FORM_PAIRS, ids=[PAIR_IDS['fenton'][p] for p in FORM_PAIRS])
def test_generated_four_variable_equals_handwritten(gpu_lib, golden, _restore_modules, p):
    """tests/models/four_variable.py -> tracer -> generated kernel at (0.02, 1.5) and (0.2, 0.7): the reference's trajectory
    within its bound and, under the rounding-faithful policy, the hand-written Fenton kernel bit for bit, as at 0.1"""
    from traced_cases import TIMESTEP_TWINS, make_model
    from fib_tf_amd import _lib
    f = golden('ts_fenton_traj_p%d' % p)
    dt, diff = float(f['dt']), float(f['diff'])
    assert ('fv', dt, diff) in TIMESTEP_TWINS
    init = np.stack([f['init_' + k] for k in 'UVWS'])
    _, H, W = init.shape
    for fast in (False, True):
        m = make_model('fv', H, W, fast_math=fast, dt=dt, diff=diff)
        m.phase = f['phase']
        m.define()
        m._ensure_compiled()
        assert m._stepper.launch_plan() == (10, 1)
        m._stepper.set_state(-1, init)
        nat = _lib.Stepper(_lib.FENTON4V, H, W, dt, diff, flags=_lib.FAST if fast else 0)
        nat.set_phase(f['phase'])
        nat.set_state(-1, init)
        t0 = 0
        for t in [int(x) for x in f['snap_ticks']]:
            m._stepper.step(t - t0)
            nat.step(t - t0)
            t0 = t
            got = m._stepper.get_state(-1)
            tc.check([('fv %s t%d' % (k, t), tc.maxerr(got[i], f['%s_t%d' % (k, t)]), 2e-4 if fast else tc.TRAJ_TOL)
                      for i, k in enumerate('UVWS')])
            if not fast:
                assert np.array_equal(got, nat.get_state(-1)), 'generated vs hand-written kernel differ at tick %d' % t
        nat.close()


@pytest.mark.parametrize('p', FORM_PAIRS, ids=[PAIR_IDS['br'][p] for p in FORM_PAIRS])
def test_generated_eight_variable_vs_handwritten(gpu_lib, golden, _restore_modules, p):
    """tests/models/eight_variable.py at (0.02, 0.809) and (0.2, 0.4) against the reference's br.py (direct gates) and the
    hand-written kernel, within test_gpu_traced.test_generated_eight_variable_vs_handwritten's bound"""
    from traced_cases import TIMESTEP_TWINS, make_model
    from fib_tf_amd import _lib
    f = golden('ts_br_traj_p%d' % p)
    dt, diff = float(f['dt']), float(f['diff'])
    assert ('ev', dt, diff) in TIMESTEP_TWINS
    init = np.stack([f['init_' + k] for k in tc.BR_VARS])
    _, H, W = init.shape
    m = make_model('ev', H, W, fast_math=False, dt=dt, diff=diff)
    m.phase = f['phase']
    m.define()
    m._ensure_compiled()
    assert m._stepper.launch_plan() == (5, 1)
    m._stepper.set_state(-1, init)
    nat = _lib.Stepper(_lib.BR, H, W, dt, diff)
    nat.set_phase(f['phase'])
    nat.set_state(-1, init)
    scales = {'V': 120.0, 'C': 1e-4}
    t0 = 0
    for t in [int(x) for x in f['snap_ticks']]:
        m._stepper.step(t - t0)
        nat.step(t - t0)
        t0 = t
        got, hand = m._stepper.get_state(-1), nat.get_state(-1)
        figs = []
        for i, k in enumerate(tc.BR_VARS):
            s = scales.get(k, 1.0)
            figs.append(('ev %s t%d' % (k, t), tc.maxerr(got[i], f['direct_%s_t%d' % (k, t)]), 3e-5 * s))
            figs.append(('ev vs hand-written %s t%d' % (k, t), tc.maxerr(got[i], hand[i]), 3e-5 * s))
        tc.check(figs)
    nat.close()


# --------------------------------------------------------------------------------------------
# diff = 0: a cell's new state does not depend on its neighbours
# --------------------------------------------------------------------------------------------
def _permuted(arrs, perm):
    """the interior cells of every plane moved by `perm`; the outermost ring stays (enforce_boundary overwrites it with its
    inner neighbours, whatever the diffusion coefficient)"""
    out = []
    for a in arrs:
        b = np.array(a, np.float32)
        inner = b[1:-1, 1:-1]
        b[1:-1, 1:-1] = inner.ravel()[perm].reshape(inner.shape)
        out.append(b)
    return out


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('model', ['fenton', 'br-direct', 'br-cheby', 'court'])
def test_no_diffusion_no_neighbours(gpu_lib, golden, orc, model, policy):
    """(0.03, 0): permuting the interior cells of the input planes permutes the interior of the output, bit for bit —
    float(diff * dt) is zero, and a zero times the Laplacian changes no potential"""
    if model == 'fenton':
        c, names = tc.fenton_step_case(golden, 3), 'UVWS'
        solve = lambda arrs: tc.device_fenton_step(dict(c, **dict(zip(names, arrs))), policy)
    elif model.startswith('br'):
        c, names = tc.br_step_case(golden, 3), tc.BR_VARS
        solve = lambda arrs: tc.device_br_step(dict(c, **dict(zip(names, arrs))), model[3:], 1, policy)
    else:
        names = list(orc.COURT_VARS)
        c = tc.court_step_case(golden, 3, names)
        solve = lambda arrs: tc.device_court_step(dict(c, **dict(zip(names, arrs))), True, policy)
    assert c['diff'] == 0.0
    H, W = c[names[0]].shape
    perm = np.random.default_rng(5).permutation((H - 2) * (W - 2))
    assert (perm != np.arange(perm.size)).mean() > 0.9
    arrs = [c[k] for k in names]
    plain = solve(arrs)
    moved = solve(_permuted(arrs, perm))
    for k, a, b in zip(names, _permuted(plain, perm), moved):
        assert np.array_equal(a[1:-1, 1:-1], b[1:-1, 1:-1], equal_nan=True), k
