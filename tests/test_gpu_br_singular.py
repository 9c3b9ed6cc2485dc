"""-m gpu: Beeler-Reuter with cells EXACTLY on its two 0/0 voltages (V == -47.0f: alpha_m; V == -23.0f: the second quotient of
i_K1), where the kernels define the quotients as their limits 10 and 25 (csrc/models.hpp BeelerReuter::ab, csrc/br_step.inc;
DESIGN.md 9, "op contract").  The reference's float32 formulas give NaN there, which its clips turn into M = 1e-5 and
V = -85 mV: there is no reference value to be faithful to, so the yardstick is the float64 restatement tests/br_ref64.py
(validated against the oracle on control cells by tests/test_br_singular_cpu.py).

  * control and exact cells: STEP_TOL[policy] of the array's scale for one sub-step, TICK_TOL[policy] for a tick — the
    bounds of tests/test_gpu_parity.py and tests/test_gpu_timestep.py, with their one named exception (H under the fast
    policy with Chebyshev gates, 1e-4);
  * the +-1, +-2, +-4 float32 neighbours of the two voltages, ill-conditioned in the reference's own formulas: inside the
    oracle's sensitivity envelope widened by three times its width plus the bound (test_gpu_variant_table.oracle_error_bar);
    the planted neighbours are the only cells treated so (br_singular_cases.N_NEIGHBOUR_CELLS, a count);
  * kernel forms: bit for bit within a policy."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import br_ref64  # noqa: E402
import br_singular_cases as sc  # noqa: E402
import timestep_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

POLICIES = tc.POLICIES
DT = 0.1
ENV = ('FIBHIP_MT', 'FIBHIP_MT_MAX', 'FIBHIP_VARIANT', 'FIBHIP_AHEAD', 'FIBHIP_AUTOTUNE', 'FIBHIP_K', 'FIBHIP_PERIOD_ROW')


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def check(figs):
    """figures (what, error, bound): each printed for the record, then asserted"""
    for f in figs:
        print('%-58s %.3e  bound %.3e' % f)
    tc.check(figs)


def err(got, want, mask):
    got = np.asarray(got, np.float64)[..., mask]
    if not np.isfinite(got).all():
        return float('inf')
    return float(np.abs(got - np.asarray(want, np.float64)[..., mask]).max(initial=0.0))


# --------------------------------------------------------------------------------------------
# one sub-step through BeelerReuter.solve
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def planted():
    st, _ = sc.plane()
    st.setflags(write=False)
    exact, neigh = sc.classify(st[0])
    phi = sc.phase(*sc.SHAPE)
    ref = {n: br_ref64.substep(st, DT, sc.DIFF, phi, n) for n in (0, 1, 5)}
    return {'state': st, 'exact': exact, 'neigh': neigh, 'phi': phi, 'ref64': ref, 'envelope': {}}


def step_tol(policy, cheby, k):
    # the one named exception of test_br_single_step: the degree-8 sums under fused multiply-adds, visible in H only
    return 1e-4 if cheby and policy == 'fast' and k == 'H' else tc.STEP_TOL[policy]


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('cheby', [False, True], ids=['direct', 'cheby'])
@pytest.mark.parametrize('n', [0, 1, 5])
def test_br_exact_singular_single_step(gpu_lib, orc, planted, n, cheby, policy):
    """solve(state, n) on the planted 37 x 53 plane, phase hole (25, 17, 7), diff 0.809 (the br_step fixture's setting).
    Direct gates: every array of the control and exact cells against br_ref64, the neighbours inside the oracle's envelope.
    Chebyshev gates (no 0/0 in the fits, but the currents are shared): the gates of every cell against the oracle with the
    same table; V and C — which read the OLD gates only — as under the direct gates.
    Measured on an MI355X with the two selects taken out of the kernels, exact cells: M 0.56 off under both policies (the
    clip floor 1e-5); V 68.4 mV off under the rounding-faithful policy (0/0 = NaN through the clip: -85 mV) and 0.175 mV
    under the fast one — its denominator fma(1 / e, -1 / E23, 1) is a stray tiny number there, not 0, so the quotient is 0
    instead of 25 and i_K1 is short of 0.35 * 0.2 * 25.  With them: <= 7.3e-8 (gates) and 3.4e-6 mV."""
    from fib_tf_amd.br import BeelerReuter
    from test_gpu_variant_table import oracle_error_bar
    st, exact, neigh, phi = planted['state'], planted['exact'], planted['neigh'], planted['phi']
    m = BeelerReuter(tc.device_cfg(*sc.SHAPE, DT, sc.DIFF, policy, cheby=cheby))
    m.phase = phi
    got = np.stack(m.solve(tuple(st[i] for i in range(8)), n))
    assert np.isfinite(got).all()
    # the envelope of the DIRECT gates' step: V and C read the old gates only, so they are the same values under either gate
    # form, and the Chebyshev fits have no 0/0 (their gates are held to the plain bound at EVERY cell, neighbours included;
    # the degree-8 sums are too sensitive to an ulp of V for an envelope at this bound to mean anything)
    if n not in planted['envelope']:
        planted['envelope'][n] = oracle_error_bar(orc, lambda s: orc.br_step(s, DT, sc.DIFF, phi, None, n), st,
                                                  sc.step_bounds(tc.STEP_TOL['exact']))
    oref, ill, lo, hi = planted['envelope'][n]
    if cheby:
        oref = orc.br_step(st, DT, sc.DIFF, phi, m.chebyshev_table().astype(np.float32), n)
    held = ~neigh
    assert not (ill & held & ~exact).any(), 'control cells ill-conditioned in the oracle itself'
    assert int((ill & ~exact).sum()) <= sc.N_NEIGHBOUR_CELLS == int(neigh.sum()) and int(exact.sum()) == sc.N_EXACT_CELLS
    ref64 = planted['ref64'][n]
    tag = 'cheby' if cheby else 'direct'
    figs = []
    for i, (k, scale) in enumerate(zip(tc.BR_VARS, sc.BR_SCALES)):
        tol = step_tol(policy, cheby, k) * scale
        if cheby and i >= 2:
            figs.append(('%s %s n=%d %s every cell, against the oracle' % (tag, policy, n, k), err(got[i], oref[i], held | neigh), tol))
            figs.append(('%s %s n=%d %s exact cells, against the oracle' % (tag, policy, n, k), err(got[i], oref[i], exact), tol))
            continue
        for name, mask in (('control', held & ~exact), ('exact', exact)):
            figs.append(('%s %s n=%d %s %s cells' % (tag, policy, n, k, name), err(got[i], ref64[i], mask), tol))
        # the neighbours: distance from the oracle's envelope over its margin
        margin = 3.0 * (hi[i] - lo[i]) + tol
        dist = np.maximum(np.maximum(lo[i] - got[i], got[i] - hi[i]), 0.0) / margin
        figs.append(('%s %s n=%d %s neighbours / envelope' % (tag, policy, n, k), float(dist[neigh].max()), 1.0))
    check(figs)
    # no exact cell on a clip bound that the float64 value is not on (gates under Chebyshev: that the oracle's is not on)
    want = ref64.astype(np.float32)
    if cheby:
        want[2:] = oref[2:]
    stray = sc.on_bound(got) & ~sc.on_bound(want) & exact
    assert not stray.any(), 'exact cells on a clip bound: arrays %s' % sorted({tc.BR_VARS[v] for v in np.argwhere(stray)[:, 0]})
    if n == 0:
        assert np.array_equal(got[4:], st[4:])             # solve(state, 0) carries the slow gates over, bit for bit


# --------------------------------------------------------------------------------------------
# kernel forms on a 70 x 130 state, exact cells on every lane role and on the tile seams
# --------------------------------------------------------------------------------------------
BIG = (70, 130)
# (name, environment, tile the plan must run, multi-tick launches: True = must be taken, False = must not, None = the plan's
# own business — the default plan is chosen by measurement on the first tick, and only a single-launch plan runs multi-tick)
FORMS = [('K=1', {'FIBHIP_VARIANT': '1,64,4,256', 'FIBHIP_MT': '0'}, (64, 4, -256), False),
         ('K=5 strip 54x21, multi-tick', {'FIBHIP_VARIANT': '5,54,21,-2'}, (54, 21, 2), True),
         ('K=5 strip 54x21, one launch per tick', {'FIBHIP_VARIANT': '5,54,21,-2', 'FIBHIP_MT': '0'}, (54, 21, 2), False),
         ('K=5 strip 54x27, multi-tick', {'FIBHIP_VARIANT': '5,54,27,-3'}, (54, 27, 3), True),
         ('K=5 strip 54x27, one launch per tick', {'FIBHIP_VARIANT': '5,54,27,-3', 'FIBHIP_MT': '0'}, (54, 27, 3), False),
         ('default plan', {}, None, None),
         ('default plan, one launch per tick', {'FIBHIP_MT': '0'}, None, False),
         ('declared series', {}, None, None)]


@pytest.fixture(scope='module')
def forms_case():
    from test_gpu_timestep import make_big_states
    big = make_big_states()
    st = sc.kernel_forms_state(big['br'])
    st.setflags(write=False)
    return {'state': st, 'phi': big['phi'], 'ref64': {}}


def ref_tick(state, phi, skip):
    """(five chained br_ref64 sub-steps, the cells to compare).  As test_br_vs_oracle_random_state does, a cell that stands
    within 0.1 mV of a 0/0 voltage WITHOUT standing on it at the start of one of the five sub-steps is left out: there one
    ulp of exp is a relative rate error of 6e-7 / distance in any float32 evaluation of the reference's formulas.  A cell
    that stands ON one is kept: that is what this file is about."""
    s = np.asarray(state, np.float64)
    keep = np.ones(s.shape[1:], bool)
    for i in range(5):
        V0 = br_ref64.enforce_boundary(s[0])
        for x in (47.0, 23.0):
            d = np.abs(V0 + x)
            keep &= (d >= 0.1) | (d == 0.0)
        s = br_ref64.substep(s, DT, sc.DIFF, phi, ((5 if i == 0 else 0) if skip else 1))
    return s, keep


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('cheby,skip', [(False, False), (False, True), (True, False), (True, True)],
                         ids=['direct', 'direct-skip', 'cheby', 'cheby-skip'])
def test_br_exact_singular_kernel_forms(gpu_lib, monkeypatch, forms_case, cheby, skip, policy):
    """one tick and three ticks in every kernel form: bit for bit within the policy; the K = 1 kernel's tick against five
    chained br_ref64 sub-steps (direct gates: br_ref64 has no others) within TICK_TOL[policy]"""
    from fib_tf_amd.br import BeelerReuter
    from test_gpu_timestep import TICK_TOL
    init, phi = forms_case['state'], forms_case['phi']
    forms = [f + (False,) for f in FORMS] + ([('table compiled in', {}, None, None, True)] if cheby else [])
    results = {}
    for name, env, tile, mt, spec in forms:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m = BeelerReuter(tc.device_cfg(*BIG, DT, sc.DIFF, policy, cheby=cheby, skip=skip, specialise=spec))
            m.phase = phi
            m.define()
            assert (m._library is not None) == spec
            s = m._stepper
            assert tile is None or s.plan_tile() == tile, '%s: the plan runs tile %s' % (name, s.plan_tile())
            s.set_state(-1, init)
            s.step(1)
            one = s.get_state(-1)
            s.set_state(-1, init)
            if name == 'declared series':
                s.expect(3)
                for _ in range(3):
                    s.step(1)
            else:
                s.step(3)
            three = s.get_state(-1)
            if mt is not None:
                assert (s.launch_stats()['mt_ticks'] > 0) == mt, '%s: %d ticks ran in multi-tick launches' % (name, s.launch_stats()['mt_ticks'])
            s.close()
            results[name] = (one, three)
    for name, (one, three) in results.items():
        assert np.isfinite(one).all() and np.isfinite(three).all(), name
        for what, a, b in (('one tick', one, results['K=1'][0]), ('three ticks', three, results['K=1'][1])):
            assert np.array_equal(a, b), '%s, %s: differs from K=1 in %d cells (max |d| %.3g)' % (
                name, what, int((a != b).any(axis=0).sum()), float(np.abs(a - b).max()))
    exact, _ = sc.classify(init[0])
    hit = sc.on_bound(results['K=1'][0])
    if not cheby:
        if skip not in forms_case['ref64']:
            forms_case['ref64'][skip] = ref_tick(init, phi, skip)
        ref, keep = forms_case['ref64'][skip]
        # (an exact cell may come within 0.1 mV of a voltage AGAIN in a later sub-step, and is then left out like any other)
        assert keep[exact].mean() > 0.9 and keep.mean() > 0.95
        exact = exact & keep
        one = results['K=1'][0]
        tol = TICK_TOL[policy]
        check([('direct skip=%s %s V' % (skip, policy), err(one[0], ref[0], keep), tol * 120.0),
               ('direct skip=%s %s C' % (skip, policy), err(one[1], ref[1], keep), tol * 1e-5),
               ('direct skip=%s %s gates' % (skip, policy), err(one[2:], ref[2:], keep), tol),
               ('direct skip=%s %s V exact cells' % (skip, policy), err(one[0], ref[0], exact), tol * 120.0),
               ('direct skip=%s %s gates exact cells' % (skip, policy), err(one[2:], ref[2:], exact), tol)])
        hit &= ~sc.on_bound(ref.astype(np.float32))
        assert not hit[:, exact].any(), 'exact cells on a clip bound after a tick'


# --------------------------------------------------------------------------------------------
# a repolarising sheet: a plateau whose potentials cross both voltages
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sheet_case():
    st, snapped = sc.sheet()
    st.setflags(write=False)
    return {'state': st, 'snapped': snapped, 'ref64': br_ref64.tick(st, DT, sc.DIFF, None, False)}


@pytest.mark.parametrize('policy', POLICIES)
def test_br_repolarising_sheet_has_no_spike(gpu_lib, sheet_case, policy):
    """64 x 96, V a ramp from -22 to -24 mV (rows 0-31) and from -46 to -48 mV (rows 32-63) across the columns, one cell in
    eight snapped to exactly -23.0f / -47.0f, plateau gates (M 0.9, H and J 1e-5, D 0.3, F 0.7, XI 0.2, C 2e-7): one tick,
    EVERY cell against five chained br_ref64 sub-steps within TICK_TOL[policy]; no cell on -85 or 25 mV; no gate of a
    snapped cell on a clip bound that br_ref64's is not on (H and J start ON their floor 1e-5 and, with h_inf and j_inf
    below it at these potentials, stay there in float64 too: M, D, F and XI are the gates that must not be).
    Under the reference's own formulas each snapped cell of the upper band ends the first sub-step at -85 mV and each of
    the lower band with M = 1e-5 (measured with the selects taken out: V 21.8 mV and M 0.48 off after the tick under the
    rounding-faithful policy, 0.06 mV and 7.2e-4 under the fast one).
    Measured with them (bound): rounding-faithful V 9.1e-6 mV at the snapped cells, M 2.8e-6 at the snapped cells and
    9.69e-6 (1e-5) over every cell; fast policy M 9.63e-6 (7.5e-5).  The largest M error is NOT at a snapped cell: the
    ramp's step is 0.021 mV, so some unsnapped column always stands within 0.0105 mV of -47 before the last sub-step, where
    half an ulp of exp(-0.1 x) is a relative error of 3e-8 / (0.1 x) in alpha_m in ANY float32 evaluation of the reference's
    formula (the CPU oracle: 9.69e-6 at the same cell, 0.0086 mV away).  That ill-conditioning is the reference's own and is
    not changed here; this sheet's worst cell happens to stay inside the bound."""
    from fib_tf_amd import _lib
    from test_gpu_timestep import TICK_TOL
    init, snapped, ref = sheet_case['state'], sheet_case['snapped'], sheet_case['ref64']
    st = _lib.Stepper(_lib.BR, *init.shape[1:], DT, sc.DIFF, flags=_lib.FAST if policy == 'fast' else 0)
    st.set_state(-1, init)
    st.step(1)
    got = st.get_state(-1)
    st.close()
    assert np.isfinite(got).all()
    tol = TICK_TOL[policy]
    every = np.ones(snapped.shape, bool)
    figs = []
    for i, (k, scale) in enumerate(zip(tc.BR_VARS, sc.BR_SCALES)):
        figs.append(('sheet %s %s every cell' % (policy, k), err(got[i], ref[i], every), tol * scale))
        figs.append(('sheet %s %s snapped cells' % (policy, k), err(got[i], ref[i], snapped), tol * scale))
    check(figs)
    assert not sc.on_bound(got)[0].any(), 'cells on -85 or 25 mV'
    stray = sc.on_bound(got) & ~sc.on_bound(ref.astype(np.float32))
    assert not stray[:, snapped].any(), 'snapped cells with a gate on a clip bound'
    assert not sc.on_bound(got)[[2, 5, 6, 7]][:, snapped].any()
