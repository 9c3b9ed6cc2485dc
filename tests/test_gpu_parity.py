"""-m gpu: parity of the HIP path (through the ctypes C ABI and the Python API) against
(a) the committed golden vectors produced by the reference's own functions and (b) the oracle on
the same seeded inputs.

Two arithmetic policies are shipped and BOTH are tested here (config['fast_math']):
  fast  (default)  hardware exp/log/rcp/sqrt, reciprocal-multiply for division by model constants
  exact            one float32 rounding per reference op (IEEE-equivalent division, ocml functions)

Tolerances (float32):
  * pure arithmetic (boundary, Laplacian incl. phase-field term): BIT-EXACT under both policies.
  * one sub-step through tanh/exp/expm1/log: |d| <= 4e-6 * range (exact), 3e-5 * range (fast).
    At a time step other than 0.1 ms (tests/test_gpu_timestep.py) these are multiplied by max(1, dt / 0.1): the difference
    between two float32 evaluations of a step is a rate error times dt; a step below 0.1 ms gets no extra room.
  * trajectories, both policies: |d| <= 2e-5 * range at <= 200 sub-steps, 1e-3 * range at 1000
    sub-steps (round-off grows along the upstroke; beyond wave break the dynamics are chaotic).
`range` is max_v - min_v of the model (1 for Fenton, 120 mV for BR, 150 mV for Courtemanche);
gates and concentrations use their own span.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = {'dt': 0.1, 'dt_per_plot': 10, 'duration': 1000, 'timeline': False, 'timeline_name': 'unused.json',
       'save_graph': False, 'skip': False, 'cheby': False}


def cfg(h, w, diff, policy='exact', **kw):
    c = dict(CFG, height=h, width=w, diff=diff, fast_math=(policy == 'fast'))
    c.update(kw)
    return c


POLICIES = ['fast', 'exact']
STEP_TOL = {'exact': 4e-6, 'fast': 3e-5}


def span(a):
    return max(float(np.max(a) - np.min(a)), 1e-30)


def assert_close(got, want, rel, what, scale=None):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert np.isfinite(got).all(), '%s: non-finite values' % what
    s = scale if scale is not None else max(span(want), float(np.abs(want).max()) * 1e-3, 1e-30)
    err = float(np.abs(got - want).max())
    assert err <= rel * s, '%s: max|d| = %.3e > %.1e * %.3g' % (what, err, rel, s)


# --------------------------------------------------------------------------------------------
# unit ops (ionic.py:44-123)
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
def test_unit_ops_bit_exact(gpu_lib, golden, policy):
    from fib_tf_amd.ionic import IonicModel
    u = golden('unit_ops')
    m = IonicModel(cfg(37, 53, 1.0, policy))
    assert np.array_equal(m.enforce_boundary(u['X']), u['enforce_boundary'])
    assert np.array_equal(m.laplace(u['X']), u['laplace_nophase'])
    m.phase = u['phi']
    assert np.array_equal(m.laplace(u['X']), u['laplace_phase'])
    assert np.array_equal(m.phase_field(np.pad(u['X'], 1, mode='reflect')), u['phase_field'])


@pytest.mark.parametrize('policy', POLICIES)
def test_rush_larsen(gpu_lib, golden, policy):
    from fib_tf_amd.ionic import IonicModel
    u = golden('unit_ops')
    m = IonicModel(cfg(37, 53, 1.0, policy))
    for dt in (0.1, 0.5, 1.0):
        got = m.rush_larsen(u['rl_g'], u['rl_inf'], u['rl_tau'], dt)
        assert_close(got, u['rush_larsen_dt%g' % dt], 4e-7 if policy == 'exact' else 2e-6, 'rush_larsen dt=%g' % dt,
                     scale=1.0)
    assert m.rush_larsen(np.float32(0.5), 0.2, 3.0, 0.1).shape == ()


def test_phase_field_construction(golden):
    # host-side geometry, no GPU needed but kept next to its consumer
    from fib_tf_amd.ionic import IonicModel
    u = golden('unit_ops')
    m = IonicModel(cfg(37, 53, 1.0))
    m.add_hole_to_phase_field(20, 15, 6)
    assert np.array_equal(m.phase, u['hole_a'])
    m.add_hole_to_phase_field(26, 18, 30, neg=True)
    assert np.array_equal(m.phase, u['hole_ab'])


# --------------------------------------------------------------------------------------------
# single sub-step vs golden (branch-covering random states)
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('variant', ['phase', 'nophase'])
def test_fenton_single_step(gpu_lib, golden, variant, policy):
    from fib_tf_amd.fenton import Fenton4v
    f = golden('fenton_step_' + variant)
    m = Fenton4v(cfg(37, 53, float(f['diff']), policy))
    if f['phase'].size:
        m.phase = f['phase']
    out = m.solve(tuple(f[k] for k in 'UVWS'))
    for k, o in zip('UVWS', out):
        assert_close(o, f[k + '1'], STEP_TOL[policy], 'fenton %s1' % k, scale=1.0)
    if policy == 'exact':       # V and W never pass through a transcendental: bit-exact
        assert np.array_equal(out[1], f['V1'])
        assert np.array_equal(out[2], f['W1'])


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('cheby', [False, True])
@pytest.mark.parametrize('n', [0, 1, 5])
def test_br_single_step(gpu_lib, golden, cheby, n, policy):
    from fib_tf_amd.br import BeelerReuter
    f = golden('br_step')
    m = BeelerReuter(cfg(37, 53, 0.809, policy, cheby=cheby))
    m.phase = f['phase']
    names = m.VAR_NAMES
    out = m.solve(tuple(f[k] for k in names), n)
    tag = 'cheby' if cheby else 'direct'
    for k, o in zip(names, out):
        want = f['%s1_%s_n%d' % (k, tag, n)]
        scale = {'V': 120.0, 'C': 1e-5}.get(k, 1.0)
        tol = STEP_TOL[policy]
        if cheby and policy == 'fast' and k == 'H':
            # the fast policy evaluates the degree-8 sums with fused multiply-adds: other rounding points than the
            # reference's, amplified ~1e2 by the sums; only the h gate's fit is conditioned badly enough to show
            # (br.py:289-301; measured 6.9e-5, every other variable <= 1.3e-5: tools/br_step_error.py)
            tol = 1e-4
        assert_close(o, want, tol, 'br %s %s n=%d [%s]' % (tag, k, n, policy), scale=scale)
        if n == 0 and k in ('J', 'D', 'F', 'XI'):      # solve(state, 0) carries the slow gates over: bit for bit
            assert np.array_equal(o, f[k])


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('skip', [False, True])
def test_br_specialised_build_is_bit_identical(gpu_lib, policy, skip):
    """BeelerReuter(cheby=True) runs a build of the library with its Chebyshev table compiled in as literals
    (fib_tf_amd/br.py specialised_library); the stock library takes the table as a kernel argument.  Same
    arithmetic: the states must agree bit for bit, whatever the fusion depth."""
    from fib_tf_amd.br import BeelerReuter
    res = []
    for spec in (True, False):
        m = BeelerReuter(cfg(96, 80, 0.809, policy, cheby=True, skip=skip, specialise=spec, duration=4.0))
        m.add_hole_to_phase_field(30, 40, 8)
        m.define()
        assert (m._library is not None) == spec
        for _ in m.run():
            pass
        res.append(np.stack([m._State[k].eval() for k in m.VAR_NAMES]))
        if spec:
            fused, launches = m._stepper.launch_plan()        # (chosen by measurement: any split of the 5 sub-steps)
            assert '_spec' in m._library._name and fused * launches == 5
    assert np.array_equal(res[0], res[1])


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('H,W', [(70, 66), (65, 64), (64, 65), (80, 130)])
def test_court_fused_slow_tick_is_bit_identical(gpu_lib, policy, H, W, monkeypatch):
    """the reference driver fires 'slow' right after every 10th tick (court.py:612-617); the library launches that
    tick and the slow op as ONE kernel (Courtemanche::MODE_FASTSLOW) when the grid allows it ((H-1) % 4 and
    (W-1) % 64 nonzero) — the same arithmetic on the same inputs, so the state must not change by a bit; the
    (65, .) and (., 65) grids take the two-launch path by construction"""
    from fib_tf_amd.court import Courtemanche
    res = []
    for lazy in (True, False):
        if lazy:
            monkeypatch.delenv('FIBHIP_NO_LAZY', raising=False)
        else:
            monkeypatch.setenv('FIBHIP_NO_LAZY', '1')
        m = Courtemanche(cfg(H, W, 0.809, policy, duration=4.3))
        m.add_hole_to_phase_field(W // 2, H // 2, 6)
        m.define()
        m.add_pace_op('s2', 'luq', 10.0)
        trend = []
        for i in m.run():
            if i % 10 == 0:
                m.fire_op('slow')
                m.fire_op('trend')
                trend.append(m._Trend.eval())
            if i == 21:
                m.fire_op('s2')
            if i == 33:
                m._State['_Ca_i_'].eval()                    # a read between a tick and nothing: flushes the pending tick
        res.append((np.stack([m._State[k].eval() for k in m.VAR_NAMES]), np.array(trend)))
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])


def _court_run(monkeypatch, agg, H, W, poke=None, ticks=57):
    """raw C ABI: `ticks` fast ticks, 'slow' after every 10th, one S2-style pace, optionally a host write in between"""
    from fib_tf_amd import _lib
    from fib_tf_amd.court import INITIAL
    if agg:
        monkeypatch.delenv('FIBHIP_COURT_AGG', raising=False)
    else:
        monkeypatch.setenv('FIBHIP_COURT_AGG', '0')
    rng = np.random.default_rng(11)
    init = np.empty((21, H, W), np.float32)
    for i, (_, v) in enumerate(INITIAL):
        init[i] = v
    init[0] += rng.uniform(-5, 60, (H, W)).astype(np.float32)
    phi = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
    st = _lib.Stepper(_lib.COURT, H, W, 0.1, 0.809, flags=_lib.FAST)
    st.set_phase(phi)
    st.set_state(-1, init)
    snaps = []
    for i in range(ticks):
        st.step(1)
        if i % 10 == 0:
            st.step_slow()
        if i == 12:
            st.pace(0, max(1, H // 2), 0, max(1, W // 2), 10.0, -100.0)
        if poke and i == poke[0]:
            st.set_state(poke[1], poke[2])
        if i in (0, 9, 10, 11, 30, ticks - 1):
            snaps.append(st.get_state(-1))
    st.close()
    return snaps


COURT_SCALES = [150.0, 1.0] + [1.0] * 3 + [1.0] + [1.0] * 6 + [1e-3] + [1.0] * 3 + [1.5] + [1.0] * 3 + [1.0]
# the SR-release subsystem switches through a sigmoid one ulp of Fn wide (see test_court_trajectory): looser there
COURT_CALCIUM = (12, 15, 16, 17, 18, 19, 20)


def court_rel(v):
    # V itself: 2e-5 * 150 mV = 3e-3 mV; a gate follows V with a slope of up to 0.05 per mV (oi_inf, court.py:371)
    return 1e-3 if v in COURT_CALCIUM else (2e-5 if v in (0, 1, 5) else 2e-4)


@pytest.mark.parametrize('H,W', [(70, 66), (65, 64), (40, 131)])
def test_court_aggregated_fast_tick(gpu_lib, monkeypatch, H, W):
    """Courtemanche, fast policy, one device: the tick kernels read five per-cell aggregates of the slow variables
    (CourtAgg, models.hpp) that 'slow' maintains, instead of the 12 variables they are made of.  Against the plain
    kernels (FIBHIP_COURT_AGG=0) on the same inputs the trajectories agree to the fast policy's own tolerance —
    the sums are re-associated, nothing else changes — across 'slow' ops (fused and, on the 65-row grid, separate)"""
    a = _court_run(monkeypatch, True, H, W)
    b = _court_run(monkeypatch, False, H, W)
    for sa, sb in zip(a, b):
        for v in range(21):
            assert_close(sa[v], sb[v], court_rel(v), 'var %d' % v, scale=COURT_SCALES[v])


@pytest.mark.parametrize('H,W', [(70, 66), (65, 64), (33, 200), (3, 5)])
def test_court_multi_tick_launches_bit_identical(gpu_lib, monkeypatch, H, W):
    """fibhip_step defers Courtemanche ticks so that up to three consecutive fast ticks run as ONE temporally blocked
    launch (and the last one still rides on 'slow'): the same arithmetic per cell, so not a bit may differ from one
    launch per tick (FIBHIP_NO_MULTI=1) — with a pace, a host write and read-backs falling between the ticks"""
    xs = np.full((H, W), 0.6, np.float32)
    monkeypatch.delenv('FIBHIP_NO_MULTI', raising=False)
    a = _court_run(monkeypatch, True, H, W, poke=(26, 11, xs))
    monkeypatch.setenv('FIBHIP_NO_MULTI', '1')
    b = _court_run(monkeypatch, True, H, W, poke=(26, 11, xs))
    for sa, sb in zip(a, b):
        assert np.array_equal(sa, sb)


def test_court_multi_tick_launch_count(gpu_lib, monkeypatch):
    """ten ticks and a 'slow': three 3-tick launches and the fused tick+slow launch"""
    from fib_tf_amd import _lib
    from fib_tf_amd.court import INITIAL
    monkeypatch.delenv('FIBHIP_NO_MULTI', raising=False)
    monkeypatch.delenv('FIBHIP_COURT_AGG', raising=False)
    H, W = 70, 66
    init = np.empty((21, H, W), np.float32)
    for i, (_, v) in enumerate(INITIAL):
        init[i] = v
    st = _lib.Stepper(_lib.COURT, H, W, 0.1, 0.809, flags=_lib.FAST)
    st.set_state(-1, init)
    st.step(1)
    st.step_slow()                       # (first tick: aggregates formed, then tick + slow)
    st.sync()
    st.time_begin()
    for i in range(10):
        st.step(1)
    st.step_slow()
    ms, launches = st.time_end()
    assert launches == 4, launches
    st.close()


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_court_deferred_ticks_random_call_sequences(gpu_lib, monkeypatch, seed):
    """fibhip_step is an enqueue (ticks wait until a launch is full, the last one for a 'slow' that may follow): whatever
    the caller does in between — steps of any count, 'slow' at any time, pacing, probes, single-array and whole-state
    reads and writes, timing brackets, sync — must see and leave exactly what one launch per tick leaves.  Random call
    sequences, compared call by call with the undeferred library (FIBHIP_NO_MULTI + FIBHIP_NO_LAZY)."""
    from fib_tf_amd import _lib
    from fib_tf_amd.court import INITIAL
    H, W = 41, 70
    rng0 = np.random.default_rng(100 + seed)
    init = np.empty((21, H, W), np.float32)
    for i, (_, v) in enumerate(INITIAL):
        init[i] = v
    init[0] += rng0.uniform(-5, 40, (H, W)).astype(np.float32)
    phi = rng0.uniform(0.3, 1.0, (H, W)).astype(np.float32)

    def play(deferred):
        for k in ('FIBHIP_NO_MULTI', 'FIBHIP_NO_LAZY'):
            if deferred:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, '1')
        rng = np.random.default_rng(seed)                 # the same sequence both times
        st = _lib.Stepper(_lib.COURT, H, W, 0.1, 0.809, flags=_lib.FAST)
        st.set_phase(phi)
        st.set_state(-1, init)
        seen = []
        for _ in range(120):
            op = rng.choice(['step1', 'step1', 'step1', 'stepn', 'slow', 'pace', 'probe', 'get1', 'getall', 'set1', 'sync',
                             'timed'])
            if op == 'step1':
                st.step(1)
            elif op == 'stepn':
                st.step(int(rng.integers(0, 9)))
            elif op == 'slow':
                st.step_slow()
            elif op == 'pace':
                r0, c0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 4))
                st.pace(r0, r0 + 4, c0, c0 + 4, 5.0, -100.0)
            elif op == 'probe':
                seen.append(np.float32(st.probe(int(rng.integers(0, 21)), int(rng.integers(0, H)), int(rng.integers(0, W)))))
            elif op == 'get1':
                seen.append(st.get_state(int(rng.integers(0, 21))).copy())
            elif op == 'getall':
                seen.append(st.get_state(-1))
            elif op == 'set1':
                v = int(rng.integers(1, 21))
                st.set_state(v, (st.get_state(v) * np.float32(0.999)).astype(np.float32))
            elif op == 'sync':
                st.sync()
            else:
                st.time_begin()
                st.step(int(rng.integers(1, 6)))
                st.time_end()
        seen.append(st.get_state(-1))
        st.close()
        return seen

    a, b = play(True), play(False)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), 'observation %d differs' % i


def test_court_aggregates_follow_host_writes(gpu_lib, monkeypatch):
    """set_state of a slow variable between two ticks: the aggregates are recomputed before the next tick (a stale
    aggregate would keep the old conductance: compare with the plain kernels after the write)"""
    H, W = 48, 70
    xs = np.full((H, W), 0.6, np.float32)                  # _xs_ (index 11): i_Ks = Cm g_Ks xs^2 (V - E_K)
    d = np.full((H, W), 0.4, np.float32)                   # _d_ (index 13): i_Ca_L
    for poke in ((15, 11, xs), (23, 13, d)):
        a = _court_run(monkeypatch, True, H, W, poke=poke, ticks=31)
        b = _court_run(monkeypatch, False, H, W, poke=poke, ticks=31)
        assert float(np.abs(a[-1][0] - _court_run(monkeypatch, True, H, W, ticks=31)[-1][0]).max()) > 1e-3   # the write matters
        for v in range(21):
            assert_close(a[-1][v], b[-1][v], court_rel(v), 'var %d after a host write' % v, scale=COURT_SCALES[v])


def test_court_aggregates_off_after_state_ptr(gpu_lib, monkeypatch):
    """a raw device pointer handed out (fibhip_state_ptr) means the state can change behind the library's back: the
    handle returns to the plain kernels and keeps producing the plain kernels' bits"""
    from fib_tf_amd import _lib
    from fib_tf_amd.court import INITIAL
    monkeypatch.delenv('FIBHIP_COURT_AGG', raising=False)
    H, W = 40, 70
    init = np.empty((21, H, W), np.float32)
    for i, (_, v) in enumerate(INITIAL):
        init[i] = v
    out = []
    for ptr in (True, False):
        if not ptr:
            monkeypatch.setenv('FIBHIP_COURT_AGG', '0')
        st = _lib.Stepper(_lib.COURT, H, W, 0.1, 0.809, flags=_lib.FAST)
        st.set_state(-1, init)
        if ptr:
            st.state_buf(5)
        st.step(12)
        st.step_slow()
        st.step(3)
        out.append(st.get_state(-1))
        st.close()
    assert np.array_equal(out[0], out[1])


SINGULAR = [-10.0001, -10.0, 7.9, -47.13, -14.1, 3.3328, 19.9]


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('chronic', [True, False])
def test_court_single_step(gpu_lib, golden, orc, chronic, policy):
    """all 21 outputs of one solve; cells within 0.06 mV of a removable singularity of calc_inter
    (court.py:303-410) are compared loosely: there the reference's own formula amplifies one ulp
    of exp() by 1e4-1e6 (0/0 form), so even NumPy vs libm differ at the 1e-2 level."""
    from fib_tf_amd.court import Courtemanche
    f = golden('court_step')
    m = Courtemanche(cfg(37, 53, 0.809, policy))
    m.chronic = chronic
    m.phase = f['phase']
    out = m.solve({k: f[k] for k in m.VAR_NAMES})
    V = orc.enforce_boundary(f['V'])
    near = np.zeros(V.shape, bool)
    exact = np.zeros(V.shape, bool)
    for s in SINGULAR:
        near |= np.abs(V - np.float32(s)) < 0.06
        exact |= V == np.float32(s)
    tag = 'chronic' if chronic else 'acute'
    # Near a removable singularity the comparison is against the ORACLE'S OWN SENSITIVITY there: the same step
    # evaluated with exp() moved by -1/0/+1 ulp and every potential by -2 .. +2 float32 neighbours.  What the reference
    # formula does to one ulp of exp and of its input is the honest error bar of ANY float32 evaluation of it; the
    # device value must lie inside the envelope of those fifteen answers (and the golden one), widened by three times its own width plus the ordinary
    # tolerance.  (Width for the 62 near cells of the fixture: median 0 .. 1e-5 of the variable's range, 0.85 for the
    # one cell a few ulp from V = -14.1, where the reference's own xr rate is noise; the old blanket bound was 0.2.)
    slab = np.stack([f[k] for k in orc.COURT_VARS])
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_oracle_golden import court_envelope_samples
    samples = court_envelope_samples(orc, slab, f['phase'], chronic)
    scales = {'V': 150.0, '_Na_i_': 3.0, '_K_i_': 15.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5, '_Ca_up_': 1.0}
    for i, k in enumerate(m.VAR_NAMES):
        assert orc.COURT_VARS[i] == k
        want = f['%s_1_%s' % (k, tag)]
        sc = scales.get(k, 1.0)
        got = out[k].astype(np.float64)
        d = np.abs(got - want)
        assert np.isfinite(out[k]).all(), k
        ok = ~near | exact
        tol = (6e-6 if policy == 'exact' else 4e-5) * sc
        assert d[ok].max() <= tol, '%s: %.3e' % (k, d[ok].max())
        lo = np.minimum(samples[:, i].min(axis=0), want)
        hi = np.maximum(samples[:, i].max(axis=0), want)
        margin = 3.0 * (hi - lo) + tol
        outside = np.maximum(lo - margin - got, got - hi - margin)
        assert outside[near].max() <= 0.0, '%s near a singularity: %.3e outside the oracle\'s sensitivity envelope (width %.3e)' % (
            k, outside[near].max(), (hi - lo)[near].max())


def test_court_calc_inter_reference_binary(orc):
    """the oracle's calc_inter against the numbers the reference's own generate_table.cpp prints
    (compiled from /root/reference into oracle/_ref; output committed as a fixture)"""
    path = os.path.join(os.path.dirname(__file__), 'golden', 'court_calc_inter_m50.txt')
    want = np.loadtxt(path)
    got = orc.court_calc_inter(-50.0)
    # tau_d (index 3): court.py uses V+10.0001 where courtemanche.h:178-182 uses V+10.0
    for i, (g, w) in enumerate(zip(got, want)):
        tol = 5e-6 if i == 3 else 2e-6
        assert abs(g - w) <= tol * max(abs(w), 1.0) + 6e-7, (i, g, w)


# --------------------------------------------------------------------------------------------
# trajectories through the public API (define / run / fire_op / image) vs golden
# --------------------------------------------------------------------------------------------
def run_to(model, ticks, hook=None):
    """advance `ticks` ticks through model.run()"""
    model.duration = ticks * model.dt_per_step * model.dt + 1e-9
    for i in model.run():
        if hook:
            hook(i)


# (NT < -32: rows_kernel, potential in registers + DPP taps, with R = -NT - 32 rows per wave)
FENTON_VARIANTS = ['', '10,44,25,-35', '5,54,21,-35', '10,44,28,-3', '10,44,25,-3', '10,44,27,-3', '10,44,30,-3', '5,54,25,-3',
                   '5,54,28,-3', '5,54,31,-3', '5,54,34,-3', '10,44,32,-4', '10,44,36,-4', '10,44,40,-4',
                   '10,44,44,-4', '5,54,21,-3', '5,54,23,-3', '5,54,22,-4', '5,54,27,-3', '5,54,32,-4', '5,54,40,-3', '5,54,44,-4',
                   '5,54,56,-4', '2,60,18,-4', '10,32,32,512', '10,32,32,1024', '10,32,32,256', '5,32,32,256', '5,32,32,512',
                   '5,32,16,256', '2,64,16,256', '2,32,32,256', '1,64,16,256', '1,64,4,256']


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('variant', FENTON_VARIANTS)
def test_fenton_trajectory_64(gpu_lib, golden, variant, monkeypatch, policy):
    """64x64 with a hole, ICs from define(); every fusion depth / tile shape must give the SAME
    answer as the one-step-per-launch kernel (bit-exact) and match the golden trajectory"""
    from fib_tf_amd.fenton import Fenton4v
    if variant:
        monkeypatch.setenv('FIBHIP_VARIANT', variant)
    f = golden('fenton_traj64')
    m = Fenton4v(cfg(64, 64, float(f['diff']), policy))
    m.add_hole_to_phase_field(*[float(x) for x in f['hole']])
    assert np.array_equal(m.phase, f['phase'])
    m.define()
    for k in 'UVWS':
        assert np.array_equal(m._State[k].eval(), f['init_' + k])
    t0 = 0
    for t in [int(x) for x in f['snap_ticks']]:
        m.duration = (t - t0) * m.dt_per_step * m.dt + 1e-9
        for _ in m.run():
            pass
        t0 = t
        rel = 2e-5 if t <= 20 else 1e-3
        for k in 'UVWS':
            assert_close(m._State[k].eval(), f['%s_t%d' % (k, t)], rel, 'fenton %s tick %d [%s]' % (k, t, variant),
                         scale=1.0)


@pytest.mark.parametrize('policy', POLICIES)
def test_fenton_fusion_depths_bit_identical(gpu_lib, monkeypatch, policy):
    """temporal blocking must not change a single bit: K=10/5/2 vs K=1 on a ragged grid with
    a hole, after 30 sub-steps"""
    from fib_tf_amd.fenton import Fenton4v
    res = {}
    for variant in ('1,64,4,256', '10,32,32,512', '5,32,32,256', '2,64,16,256', '10,32,32,1024', '10,44,25,-35', '5,54,21,-35',
                    '10,44,25,-3', '10,44,28,-3', '10,44,32,-4', '10,44,44,-4', '5,54,21,-3', '5,54,22,-4', '5,54,27,-3',
                    '5,54,32,-4', '5,54,40,-3', '5,54,56,-4', '2,60,18,-4'):
        monkeypatch.setenv('FIBHIP_VARIANT', variant)
        m = Fenton4v(cfg(45, 70, 1.1, policy))
        m.add_hole_to_phase_field(30, 20, 7)
        m.define()
        run_to(m, 3)
        res[variant] = np.stack([m._State[k].eval() for k in 'UVWS'])
    base = res['1,64,4,256']
    for k, v in res.items():
        assert np.array_equal(v, base), 'variant %s differs from one-step-per-launch' % k



# --------------------------------------------------------------------------------------------
# several ticks per launch (strip_mt_kernel): a grid whose tiles are all resident at once runs consecutive Fenton
# ticks as ONE launch whose tiles hand the rim of their compute box to each other between two ticks
# --------------------------------------------------------------------------------------------
def _fenton_state(H, W, seed):
    rng = np.random.default_rng(seed)
    init = np.empty((4, H, W), np.float32)
    init[0] = rng.uniform(-0.02, 1.0, (H, W))
    init[1] = rng.uniform(0, 1, (H, W))
    init[2] = rng.uniform(0, 1, (H, W))
    init[3] = rng.uniform(0, 1, (H, W))
    phi = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
    return init, phi


def _fenton_play(monkeypatch, mt, H, W, policy, phase, steps, variant=None):
    from fib_tf_amd import _lib
    if mt:
        monkeypatch.delenv('FIBHIP_MT', raising=False)
    else:
        monkeypatch.setenv('FIBHIP_MT', '0')
    if variant:
        monkeypatch.setenv('FIBHIP_VARIANT', variant)
    else:
        monkeypatch.delenv('FIBHIP_VARIANT', raising=False)
    init, phi = _fenton_state(H, W, 7 * H + W)
    st = _lib.Stepper(_lib.FENTON4V, H, W, 0.1, 1.3, flags=_lib.FAST if policy == 'fast' else 0)
    if phase:
        st.set_phase(phi)
    st.set_state(-1, init)
    out = []
    for n in steps:
        if n == 'pace':
            st.pace(H // 4, H // 4 + 5, W // 3, W // 3 + 6, 1.0, 0.0)
        elif n == 'get':
            out.append(st.get_state(0).copy())
        elif isinstance(n, tuple):                            # n single-tick calls, as run() issues them
            for _ in range(n[0]):
                st.step(1)
        else:
            st.step(n)
    out.append(st.get_state(-1))
    tpl, launches = st.ticks_per_launch(), None
    st.close()
    return out, tpl


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('phase', [True, False])
@pytest.mark.parametrize('H,W,variant', [(45, 70, '10,44,25,-3'), (64, 64, '10,44,28,-3'), (200, 300, '10,44,25,-3'), (130, 89, '10,44,32,-4'),
                                         (512, 512, None), (3, 5, '10,44,25,-3'), (26, 45, '10,44,25,-3')])
def test_fenton_multi_tick_launches_bit_identical(gpu_lib, monkeypatch, policy, phase, H, W, variant):
    """T ticks in one launch (tiles exchanging their rims through the 16-byte-cell buffer, neighbour-only waits) against
    one launch per tick (FIBHIP_MT=0): the same arithmetic per cell, so not a bit may differ — with calls of many ticks
    (several full launches + a remainder), single-tick calls (launches of 1, 2, 4, ... ticks), a pace and a read-back in
    between.  512x512 is the benchmark's own tiling: 252 workgroups, one per compute unit."""
    steps = [1, 3, 'pace', 37, 'get', (21,), 'pace', 2, (5,), 'get', 70]
    a, tpl = _fenton_play(monkeypatch, True, H, W, policy, phase, steps, variant)
    b, _ = _fenton_play(monkeypatch, False, H, W, policy, phase, steps, variant)
    if variant or policy == 'fast':      # (the rounding-faithful policy runs 512x512 as two launches of 5 sub-steps: one per tick)
        assert tpl > 1, 'the multi-tick path was not taken'
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.isfinite(x).all()
        assert np.array_equal(x, y), 'observation %d differs (max |d| %.3g)' % (i, float(np.abs(x - y).max()))


def test_fenton_multi_tick_launch_count(gpu_lib, monkeypatch):
    """twenty single-tick calls and a sync: launches of 1, 2, 4, 8 ticks and the remaining 5; one call of 70 ticks: 32 + 32
    + 6 (the last one at the sync)"""
    from fib_tf_amd import _lib
    monkeypatch.delenv('FIBHIP_MT', raising=False)
    monkeypatch.delenv('FIBHIP_MT_MAX', raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', '10,44,25,-3')
    init, phi = _fenton_state(96, 100, 5)
    st = _lib.Stepper(_lib.FENTON4V, 96, 100, 0.1, 1.3, flags=_lib.FAST)
    st.set_state(-1, init)
    st.step(1)
    st.sync()
    st.time_begin()
    for _ in range(20):
        st.step(1)
    ms, launches = st.time_end()
    assert launches == 5, launches
    st.time_begin()
    st.step(70)
    ms, launches = st.time_end()
    assert launches == 3, launches
    # series of equal length (run() with an image() every 10 ticks): a series is ONE launch, issued at its first tick (the
    # last series had that length) or by the read-back before it (the last two had)
    for _ in range(2):
        for _ in range(10):
            st.step(1)
        st.get_state(0)
    st.time_begin()
    for _ in range(10):
        st.step(1)
    ms, launches = st.time_end()
    assert launches == 1, launches
    stats = st.launch_stats()
    assert stats['ticks'] == 1 + 20 + 70 + 30 and stats['mt_ticks'] <= stats['ticks'] and stats['mt_launches'] >= 6, stats
    st.close()


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_fenton_deferred_ticks_random_call_sequences(gpu_lib, monkeypatch, seed):
    """fibhip_step is an enqueue here too: whatever the caller does between ticks must see and leave exactly what one
    launch per tick leaves (random call sequences, compared observation by observation with FIBHIP_MT=0)"""
    from fib_tf_amd import _lib
    H, W = 83, 120
    init, phi = _fenton_state(H, W, 100 + seed)

    def play(mt):
        if mt:
            monkeypatch.delenv('FIBHIP_MT', raising=False)
        else:
            monkeypatch.setenv('FIBHIP_MT', '0')
        rng = np.random.default_rng(seed)
        st = _lib.Stepper(_lib.FENTON4V, H, W, 0.1, 1.3, flags=_lib.FAST)
        st.set_phase(phi)
        st.set_state(-1, init)
        seen = []
        for _ in range(150):
            op = rng.choice(['step1', 'step1', 'step1', 'step1', 'stepn', 'pace', 'probe', 'get1', 'getall', 'set1', 'sync', 'timed',
                             'phase'])
            if op == 'step1':
                st.step(1)
            elif op == 'stepn':
                st.step(int(rng.integers(0, 45)))
            elif op == 'pace':
                r0, c0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 4))
                st.pace(r0, r0 + 4, c0, c0 + 4, 1.0, 0.0)
            elif op == 'probe':
                seen.append(np.float32(st.probe(int(rng.integers(0, 4)), int(rng.integers(0, H)), int(rng.integers(0, W)))))
            elif op == 'get1':
                seen.append(st.get_state(int(rng.integers(0, 4))).copy())
            elif op == 'getall':
                seen.append(st.get_state(-1))
            elif op == 'set1':
                v = int(rng.integers(1, 4))
                st.set_state(v, (st.get_state(v) * np.float32(0.999)).astype(np.float32))
            elif op == 'sync':
                st.sync()
            elif op == 'phase':
                st.set_phase(phi if rng.integers(0, 2) else None)
            else:
                st.time_begin()
                st.step(int(rng.integers(1, 6)))
                st.time_end()
        seen.append(st.get_state(-1))
        st.close()
        return seen

    a, b = play(True), play(False)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), 'observation %d differs' % i


def test_two_handles_multi_tick_side_by_side(gpu_lib, monkeypatch):
    """two handles on their own streams, each wanting every compute unit for its resident tiles: the library orders their
    multi-tick launches one behind the other (two half-resident grids would wait for each other)"""
    from fib_tf_amd import _lib
    monkeypatch.delenv('FIBHIP_MT', raising=False)
    monkeypatch.delenv('FIBHIP_VARIANT', raising=False)
    H = W = 512
    init, phi = _fenton_state(H, W, 3)
    hs = [_lib.Stepper(_lib.FENTON4V, H, W, 0.1, 1.3, flags=_lib.FAST) for _ in range(2)]
    for st in hs:
        st.set_phase(phi)
        st.set_state(-1, init)
    for _ in range(6):
        for st in hs:
            st.step(40)
    a, b = [st.get_state(-1) for st in hs]
    for st in hs:
        st.close()
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('cheby,skip', [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize('H,W,variant', [(70, 130, '5,54,21,-2'), (45, 70, '5,54,27,-3'), (512, 512, None)])
def test_br_multi_tick_launches_bit_identical(gpu_lib, monkeypatch, policy, cheby, skip, H, W, variant):
    """Beeler-Reuter ticks (5 sub-steps, eight arrays = two 16-byte cells per grid cell) several per launch against one
    launch per tick: bit-identical, for both gate forms, with the `skip` multirate schedule (the sub-step index restarts
    with every tick inside the launch), on the stock library (forced tile shape) and on the specialised build (512x512)"""
    from fib_tf_amd.br import BeelerReuter
    if H == 512 and (skip or not cheby):
        pytest.skip('the full-size case runs once per policy')

    def play(mt):
        if mt:
            monkeypatch.delenv('FIBHIP_MT', raising=False)
        else:
            monkeypatch.setenv('FIBHIP_MT', '0')
        if variant:
            monkeypatch.setenv('FIBHIP_VARIANT', variant)
        else:
            monkeypatch.delenv('FIBHIP_VARIANT', raising=False)
        m = BeelerReuter(cfg(H, W, 0.809, policy, cheby=cheby, skip=skip))
        m.add_hole_to_phase_field(H * 0.3, W * 0.4, min(H, W) * 0.12)
        m.define()
        st = m._stepper
        out = []
        for n in (1, 2, 7, 'pace', 40, 'get', 3, 33):
            if n == 'pace':
                st.pace(0, H // 2, 0, W // 2, 10.0, -100.0)
            elif n == 'get':
                out.append(st.get_state(0).copy())
            else:
                st.step(n)
        out.append(st.get_state(-1))
        tpl = st.ticks_per_launch()
        st.close()
        return out, tpl

    (a, tpl), (b, _) = play(True), play(False)
    if variant:
        assert tpl > 1, 'the multi-tick path was not taken'
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.isfinite(x).all()
        assert np.array_equal(x, y), 'observation %d differs (max |d| %.3g)' % (i, float(np.abs(x - y).max()))


@pytest.mark.parametrize('policy', POLICIES)
def test_fenton_run_ahead_matches_one_launch_per_tick(gpu_lib, monkeypatch, policy):
    """run-ahead: after two equally long series of ticks that each end in ONE read-back, the read-back launches the next
    series before it waits for its copy, and fibhip_step hands those ticks out.  Whatever the caller does instead of
    stepping on — a pace, a host write, a probe, an early or a late read-back, a sync — must see exactly what one launch
    per tick (FIBHIP_MT=0) leaves: the ticks handed out so far are recomputed from the untouched state, the rest is
    cancelled.  Also: in the steady pattern a series costs ONE launch."""
    from fib_tf_amd import _lib
    H, W = 130, 150
    init, phi = _fenton_state(H, W, 31)
    script = ([('steps', 10), ('get',)] * 4 +                                  # steady: run-ahead from the third read-back on
              [('steps', 4), ('pace',), ('steps', 6), ('get',)] +              # a pace in the middle of a run-ahead series
              [('steps', 10), ('get',), ('steps', 10), ('get',)] +
              [('steps', 3), ('get',)] +                                       # an early read-back
              [('steps', 10), ('get',), ('steps', 10), ('get',), ('get',)] +   # two read-backs in a row
              [('steps', 15), ('get',)] +                                      # a longer series than predicted
              [('steps', 10), ('get',), ('steps', 10), ('get',)] +
              [('steps', 5), ('sync',), ('steps', 5), ('get',)] +
              [('steps', 10), ('get',), ('steps', 10), ('get',)] +
              [('steps', 2), ('set',), ('steps', 8), ('get',)] +
              [('steps', 10), ('get',), ('steps', 10), ('get',)] +
              [('steps', 7), ('probe',), ('steps', 3), ('get',), ('steps', 10), ('getall',)])

    def play(mt):
        if mt:
            monkeypatch.delenv('FIBHIP_MT', raising=False)
        else:
            monkeypatch.setenv('FIBHIP_MT', '0')
        monkeypatch.setenv('FIBHIP_VARIANT', '10,44,25,-3')
        st = _lib.Stepper(_lib.FENTON4V, H, W, 0.1, 1.3, flags=_lib.FAST if policy == 'fast' else 0)
        st.set_phase(phi)
        st.set_state(-1, init)
        seen, steady = [], None
        for k, op in enumerate(script):
            if op[0] == 'steps':
                for _ in range(op[1]):
                    st.step(1)
            elif op[0] == 'get':
                seen.append(st.get_state(0).copy())
            elif op[0] == 'getall':
                seen.append(st.get_state(-1))
            elif op[0] == 'pace':
                st.pace(10, 40, 20, 60, 1.0, 0.0)
            elif op[0] == 'sync':
                st.sync()
            elif op[0] == 'set':
                st.set_state(2, (st.get_state(2) * np.float32(0.97)).astype(np.float32))
            elif op[0] == 'probe':
                seen.append(np.float32(st.probe(0, 64, 75)))
            if k == 5:
                steady = st.launch_stats()['launches']
            if k == 7:
                steady = st.launch_stats()['launches'] - steady        # launches of the fourth steady series
        stats = st.launch_stats()
        st.close()
        return seen, steady, stats

    a, steady, sa = play(True)
    b, _, sb = play(False)
    assert sa['ticks'] == sb['ticks'] == sum(op[1] for op in script if op[0] == 'steps')
    assert steady == 1, 'a steady series should be one launch (the run-ahead), got %r' % steady
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), 'observation %d differs' % i


@pytest.mark.parametrize('model', ['fenton', 'br'])
def test_series_launched_whole_and_cut_short(gpu_lib, monkeypatch, model):
    """fibhip_step launches a whole series at its first tick when the caller's last series had that length (a benchmark
    region, run() with a sync or probe every n ticks).  A caller that stops earlier than predicted gets the launch STOPPED at
    the tick it has reached (the host's word, read by every tile at every tick boundary) — or, when a tile was past that tick
    already, the ticks recomputed from the untouched state.  Either way every observation equals one launch per tick."""
    import time
    from fib_tf_amd import _lib
    H, W = 130, 150
    script = ([('steps', 12), ('sync',)] * 3 +                                  # the 2nd and 3rd series: one launch each
              [('steps', 5), ('sync',), ('get',)] +                             # cut short: stopped at tick 5 (or recomputed)
              [('steps', 5), ('sync',), ('steps', 5), ('probe',)] +
              [('steps', 12), ('sync',), ('steps', 12), ('sync',)] +
              [('steps', 4), ('sleep',), ('sync',), ('get',)] +                 # the launch of 12 has finished: too late to stop
              [('steps', 9), ('pace',), ('steps', 9), ('sync',), ('steps', 20), ('getall',)])

    def play(mt):
        if mt:
            monkeypatch.delenv('FIBHIP_MT', raising=False)
        else:
            monkeypatch.setenv('FIBHIP_MT', '0')
        if model == 'fenton':
            monkeypatch.setenv('FIBHIP_VARIANT', '10,44,25,-3')
            init, phi = _fenton_state(H, W, 41)
            st = _lib.Stepper(_lib.FENTON4V, H, W, 0.1, 1.3, flags=_lib.FAST)
            st.set_phase(phi)
            st.set_state(-1, init)
            keep = None
        else:
            from fib_tf_amd.br import BeelerReuter
            monkeypatch.setenv('FIBHIP_VARIANT', '5,54,21,-2')
            keep = BeelerReuter(cfg(H, W, 0.809, 'fast', cheby=True, skip=False))
            keep.add_hole_to_phase_field(40, 60, 15)
            keep.define()
            st = keep._stepper
            st.pace(0, H // 2, 0, W // 2, 10.0, -100.0)
        seen, per_series = [], []
        for op in script:
            l0 = st.launch_stats()['launches']
            if op[0] == 'steps':
                for _ in range(op[1]):
                    st.step(1)
                per_series.append(st.launch_stats()['launches'] - l0)
            elif op[0] == 'sync':
                st.sync()
            elif op[0] == 'sleep':
                time.sleep(0.05)
            elif op[0] == 'get':
                seen.append(st.get_state(0).copy())
            elif op[0] == 'getall':
                seen.append(st.get_state(-1))
            elif op[0] == 'pace':
                st.pace(10, 40, 20, 60, 1.0 if model == 'fenton' else 10.0, 0.0 if model == 'fenton' else -100.0)
            elif op[0] == 'probe':
                seen.append(np.float32(st.probe(0, 64, 75)))
        stats = st.launch_stats()
        st.close()
        return seen, per_series, stats

    a, series, sa = play(True)
    b, _, sb = play(False)
    assert sa['ticks'] == sb['ticks'] == sum(op[1] for op in script if op[0] == 'steps')
    assert series[1] == 1 and series[2] == 1, 'a series of the predicted length should be one launch: %r' % (series,)
    assert sa['ahead_stopped_in_time'] + sa['ahead_recomputed'] >= 2, sa
    assert sa['ahead_recomputed'] >= 1, sa                     # (the series the caller slept on)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.isfinite(x).all()
        assert np.array_equal(x, y), 'observation %d differs' % i


def test_periodic_series_are_predicted(gpu_lib, monkeypatch):
    """series lengths that repeat with a period — 6 ticks + read-back, 10 + read-back, 4 + sync: run() with an image() every 10
    ticks inside 20-tick benchmark regions — are launched whole from their second period on (one launch per series, the
    read-backs' frames inside the launches of the series that follow them); every observation equals one launch per tick"""
    from fib_tf_amd import _lib
    H, W = 130, 150
    init, phi = _fenton_state(H, W, 53)

    def play(mt):
        if mt:
            monkeypatch.delenv('FIBHIP_MT', raising=False)
        else:
            monkeypatch.setenv('FIBHIP_MT', '0')
        monkeypatch.setenv('FIBHIP_VARIANT', '10,44,25,-3')
        st = _lib.Stepper(_lib.FENTON4V, H, W, 0.1, 1.3, flags=_lib.FAST)
        st.set_phase(phi)
        st.set_state(-1, init)
        seen, per_period = [], []
        for period in range(5):
            l0 = st.launch_stats()['launches']
            for n, op in ((6, 'get'), (10, 'get'), (4, 'sync')):
                for _ in range(n):
                    st.step(1)
                if op == 'get':
                    seen.append(st.get_state(0).copy())
                else:
                    st.sync()
            per_period.append(st.launch_stats()['launches'] - l0)
        seen.append(st.get_state(-1))
        st.close()
        return seen, per_period

    a, per = play(True)
    b, _ = play(False)
    assert per[-1] == 3 and per[-2] == 3, 'a predicted period of three series should be three launches: %r' % (per,)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), 'observation %d differs' % i


@pytest.mark.parametrize('ids', [None, '16'])
def test_run_ahead_stress_in_lockstep(gpu_lib, monkeypatch, ids):
    """(ids = 16: launch ids cycle through 1 .. 16 instead of 1 .. 65535, so that the id the host's word still names comes
    round again at once — it must not be given to another launch while the word stands there; a build without that rule fails
    this case within 22 series)
    tools/dbg/stress_ahead.py for a few seconds: a multi-tick handle and a one-launch-per-tick handle driven in lockstep with
    random series lengths, observations, host writes and pauses — the host's word arrives early, just in time and too late —
    every observation bit-identical (a minute of it at 512x512: 70 000 series, 35 000 observations)"""
    import subprocess
    import sys
    for k in ('FIBHIP_MT', 'FIBHIP_VARIANT', 'FIBHIP_AHEAD', 'FIBHIP_MT_IDS'):
        monkeypatch.delenv(k, raising=False)
    if ids:
        monkeypatch.setenv('FIBHIP_MT_IDS', ids)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'dbg', 'stress_ahead.py'), '6', '256'], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'stress ok' in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


def test_run_ahead_off_switch(gpu_lib, monkeypatch):
    from fib_tf_amd import _lib
    monkeypatch.setenv('FIBHIP_AHEAD', '0')
    monkeypatch.setenv('FIBHIP_VARIANT', '10,44,25,-3')
    init, phi = _fenton_state(64, 64, 2)
    st = _lib.Stepper(_lib.FENTON4V, 64, 64, 0.1, 1.3, flags=_lib.FAST)
    st.set_state(-1, init)
    for _ in range(4):
        for _ in range(10):
            st.step(1)
        st.get_state(0)
    l0 = st.launch_stats()['launches']
    for _ in range(10):
        st.step(1)
    st.get_state(0)
    assert st.launch_stats()['launches'] - l0 == 2          # the first tick at once, the other nine together; nothing ahead
    st.close()


@pytest.mark.parametrize('H,W,period', [(512, 512, 2), (200, 300, 3), (512, 512, 10)])
def test_read_back_inside_the_launch_delivers_every_frame(gpu_lib, monkeypatch, H, W, period):
    """the run-ahead launch writes the frame into the caller's page-locked array itself and raises one word per tile in host
    memory; the host returns when every word has arrived.  A word that overtook its tile's cells would hand out a frame
    with cells of the PREVIOUS read-back (the pinned arrays are reused): 400 frames, short series (the frame then changes
    from read-back to read-back while the stores are still on their way), each compared with the plain path."""
    from fib_tf_amd import _lib
    monkeypatch.delenv('FIBHIP_MT', raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', '10,44,25,-3')
    init, phi = _fenton_state(H, W, 77)
    frames = {}
    for ahead in ('1', '0'):
        monkeypatch.setenv('FIBHIP_AHEAD', ahead)
        st = _lib.Stepper(_lib.FENTON4V, H, W, 0.1, 1.3, flags=_lib.FAST)
        st.set_phase(phi)
        st.set_state(-1, init)
        out = []
        for k in range(400):
            st.step(period)
            out.append(st.get_state(k % 2 * 3).sum(dtype=np.float64))       # U and S alternately; the array is reused at once
            if k % 97 == 0:
                out.append(st.get_state(0).copy())
        out.append(st.get_state(-1))
        frames[ahead] = out
        st.close()
    for i, (x, y) in enumerate(zip(frames['1'], frames['0'])):
        assert np.array_equal(x, y), 'read-back %d differs' % i

@pytest.mark.parametrize('policy', POLICIES)
def test_fenton_ragged_nophase(gpu_lib, golden, policy):
    from fib_tf_amd.fenton import Fenton4v
    f = golden('fenton_traj_ragged')
    m = Fenton4v(cfg(45, 70, float(f['diff']), policy))
    m.define()
    t0 = 0
    for t in [int(x) for x in f['snap_ticks']]:
        run_to(m, t - t0)
        t0 = t
        for k in 'UVWS':
            assert_close(m._State[k].eval(), f['%s_t%d' % (k, t)], 2e-5, 'ragged %s t%d' % (k, t), scale=1.0)


@pytest.mark.parametrize('policy', POLICIES)
def test_fenton_driver_semantics(gpu_lib, golden, policy):
    """fenton.py __main__ at 96x96: S2 in the left upper quadrant fired at tick 30, image()*phase
    cube every 10 ticks — pins tick indexing, pacing rectangle and image()"""
    from fib_tf_amd.fenton import Fenton4v
    f = golden('fenton_driver96')
    m = Fenton4v(cfg(96, 96, 1.5, policy, duration=60))
    m.add_hole_to_phase_field(48, 48, 8)
    m.define()
    m.add_pace_op('s2', 'luq', 1.0)
    s2 = int(f['s2'][0])
    cube = []
    for i in m.run():
        if i == s2:
            m.fire_op('s2')
        if i % 10 == 0:
            cube.append(m.image() * m.phase)
    assert m.samples == 60 and m.dt_per_step == 10 and m.millisecond_to_step(210) == 210
    want = f['cube']
    assert len(cube) == want.shape[0]
    for j, (g, w) in enumerate(zip(cube, want)):
        assert_close(g, w, 1e-4 if j < 4 else 1e-3, 'cube frame %d' % j, scale=1.0)
    for k in 'UVWS':
        assert_close(m._State[k].eval(), f['%s_t60' % k], 1e-3, 'driver final ' + k, scale=1.0)


@pytest.mark.parametrize('name', ['br_traj64_direct', 'br_traj64_cheby', 'br_traj64_skip', 'br_traj64_cheby_skip'])
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('variant', ['', '1,64,4,256', '5,32,32,512', '5,54,21,-3', '5,54,21,-2', '3,58,19,-2', '5,54,28,-3',
                                     '5,54,16,-2'])
def test_br_trajectory_64(gpu_lib, golden, name, variant, monkeypatch, policy):
    from fib_tf_amd.br import BeelerReuter
    if variant:
        monkeypatch.setenv('FIBHIP_VARIANT', variant)
    f = golden(name)
    m = BeelerReuter(cfg(64, 64, float(f['diff']), policy, cheby=bool(f['cheby']), skip=bool(f['skip'])))
    m.add_hole_to_phase_field(*[float(x) for x in f['hole']])
    m.define()
    m.add_pace_op('s2', 'luq', 10.0)
    for k in m.VAR_NAMES:
        assert np.array_equal(m._State[k].eval(), f['init_' + k])
    fire = (lambda i: m.fire_op('s2') if i == 10 else None) if name.endswith('cheby_skip') else None
    t0 = 0
    for t in [int(x) for x in f['snap_ticks']]:
        # run() restarts its tick counter: shift the S2 tick accordingly
        hook = (lambda i, t0=t0: fire(i + t0)) if fire else None
        run_to(m, t - t0, hook)
        t0 = t
        rel = 2e-5 if t <= 20 else 2e-4
        if policy == 'fast' and bool(f['cheby']):
            rel *= 2                                        # fused multiply-adds in the Chebyshev sums (see above)
        for k in m.VAR_NAMES:
            want = f['%s_t%d' % (k, t)]
            scale = {'V': 120.0, 'C': max(span(want), float(np.abs(want).max()))}.get(k, 1.0)   # >= 1 ulp of C
            assert_close(m._State[k].eval(), want, rel, '%s %s t%d [%s]' % (name, k, t, variant), scale=scale)


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('name', ['court_traj64', 'court_traj_ragged'])
def test_court_trajectory(gpu_lib, golden, name, policy):
    """fast tick every iteration, 'slow' + 'trend' every 10th (court.py:615-621)"""
    from fib_tf_amd.court import Courtemanche
    f = golden(name)
    H, W = f['phase'].shape
    m = Courtemanche(cfg(H, W, float(f['diff']), policy))
    m.phase = f['phase']
    m.define()
    m.add_pace_op('s2', 'luq', 10.0)
    s2 = 30 if name.endswith('ragged') else -1
    for k in m.VAR_NAMES:
        assert np.array_equal(m._State[k].eval(), f['init_' + k])
    trend = []
    t0 = 0

    def hook(i):
        g = i + t0
        if g % 10 == 0:
            m.fire_op('slow')
            m.fire_op('trend')
            trend.append(m._Trend.eval())
        if g == s2:
            m.fire_op('s2')

    scales = {'V': 150.0, '_Na_i_': 1.0, '_K_i_': 1.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5, '_Ca_up_': 1.0}
    # the SR-release gates switch through exp((Fn - 3.4175e-13)/1.367e-15) (court.py:242,246): a
    # sigmoid so steep that one ulp of Fn moves the release onset; past ~100 ticks the calcium
    # subsystem of ANY two float32 implementations (NumPy vs libm vs ocml) differs at the 1e-3 level
    calcium = ('_Ca_i_', '_Ca_rel_', '_Ca_up_', '_u_', '_v_', '_w_', '_f_Ca_')
    for t in [int(x) for x in f['snap_ticks']]:
        run_to(m, t - t0, hook)
        t0 = t
        for k in m.VAR_NAMES:
            rel = 2e-5 if t <= 100 else (5e-3 if k in calcium else 2e-4)
            assert_close(m._State[k].eval(), f['%s_t%d' % (k, t)], rel, '%s %s t%d' % (name, k, t),
                         scale=scales.get(k, 1.0))
    want = f['trend']
    got = np.array(trend)
    assert got.shape == want.shape
    assert_close(got[:, 0], want[:, 0], 2e-4, 'trend V', scale=150.0)
    assert_close(got[:, 1], want[:, 1], 2e-4, 'trend Na_i', scale=1.0)


def test_court_keep_state_and_resume(gpu_lib):
    """run(keep_state=True) -> model.state -> define(state=...) (court.py:615,623-626)"""
    from fib_tf_amd.court import Courtemanche
    m1 = Courtemanche(cfg(40, 48, 0.809, duration=2))
    m1.define()
    for i in m1.run(keep_state=True):
        if i % 10 == 0:
            m1.fire_op('slow')
    assert set(m1.state) == set(m1.VAR_NAMES)
    m2 = Courtemanche(cfg(40, 48, 0.809, duration=1))
    m2.define(state=m1.state)
    for k in m1.VAR_NAMES:
        assert np.array_equal(m2._State[k].eval(), m1.state[k])


@pytest.mark.parametrize('model', ['fenton', 'br'])
def test_keep_state_and_resume_every_model(gpu_lib, model):
    """run(keep_state=True) -> model.state -> define(state=...) for the models whose reference `define` cannot resume
    (fenton.py:110, br.py:64 take s1 only; SURVEY 5 asks for it for all): a run cut in two at a tick boundary and resumed from
    the kept state ends in the bits of the uncut run"""
    from fib_tf_amd.fenton import Fenton4v
    from fib_tf_amd.br import BeelerReuter
    cls, diff = (Fenton4v, 1.1) if model == 'fenton' else (BeelerReuter, 0.809)
    spt = 10 if model == 'fenton' else 5

    def make(ticks):
        m = cls(dict(cfg(45, 70, diff), duration=ticks * spt * 0.1 + 1e-9))
        m.add_hole_to_phase_field(30, 20, 7)
        return m
    whole = make(14)
    whole.define()
    for _ in whole.run(keep_state=True):
        pass
    first = make(6)
    first.define()
    for _ in first.run(keep_state=True):
        pass
    assert set(first.state) == set(first.VAR_NAMES)
    second = make(8)
    second.define(state=first.state)
    for k in first.VAR_NAMES:
        assert np.array_equal(second._State[k].eval(), first.state[k])
    for _ in second.run(keep_state=True):
        pass
    for k in whole.VAR_NAMES:
        assert np.array_equal(second.state[k], whole.state[k]), k
    with pytest.raises(KeyError):
        make(1).define(state={'V': first.state[first.VAR_NAMES[0]]})
    with pytest.raises(ValueError):
        make(1).define(state={k: v[:-1] for k, v in first.state.items()})


# --------------------------------------------------------------------------------------------
# oracle comparisons on seeded inputs at sizes the oracle finishes in seconds
# --------------------------------------------------------------------------------------------
def test_fenton_vs_oracle_256(gpu_lib, orc):
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v(cfg(256, 200, 1.5))
    m.add_hole_to_phase_field(100, 128, 20)
    m.define()
    m.add_pace_op('s2', 'luq', 1.0)
    ref = np.stack([m._State[k].eval() for k in 'UVWS'])
    run_to(m, 20)
    orc.fenton_run(ref, 0.1, 1.5, m.phase, 200)
    got = np.stack([m._State[k].eval() for k in 'UVWS'])
    assert_close(got, ref, 2e-5, 'fenton 256x200, 200 steps', scale=1.0)
    m.fire_op('s2')
    r0, r1, c0, c1 = m.pace_rect('luq')
    ref[0] = orc.pace(ref[0], r0, r1, c0, c1, 1.0, 0.0)
    assert_close(m._State['U'].eval(), ref[0], 2e-5, 'after S2', scale=1.0)


def test_br_vs_oracle_random_state(gpu_lib, orc):
    """seeded random state, one full tick (5 sub-steps) — both gate paths, both multirate modes"""
    from fib_tf_amd.br import BeelerReuter
    rng = np.random.default_rng(7)
    H, W = 70, 130
    st = np.empty((8, H, W), np.float32)
    st[0] = rng.uniform(-85, 25, (H, W))
    st[1] = np.exp(rng.uniform(np.log(1e-7), np.log(1e-5), (H, W)))
    st[2:] = rng.uniform(1e-5, 0.99999, (6, H, W))
    for cheby in (False, True):
        for skip in (False, True):
            m = BeelerReuter(cfg(H, W, 0.809, cheby=cheby, skip=skip))
            m.add_hole_to_phase_field(60, 30, 11)
            m.define()
            m._stepper.set_state(-1, st)
            run_to(m, 1)
            ref = st.copy()
            tbl = m.chebyshev_table().astype(np.float32) if cheby else None
            orc.br_run(ref, 0.1, 0.809, m.phase, tbl, skip, 1)
            got = m._stepper.get_state()
            # the degree-8 fits in the scaled-monomial basis cancel ~2 digits (coefficients up to 27,
            # br.py:289-301): the Chebyshev path is allowed 5x the direct path's tolerance
            rel = 5e-5 if cheby else 1e-5
            assert_close(got[0], ref[0], rel, 'br V cheby=%s skip=%s' % (cheby, skip), scale=120.0)
            assert_close(got[2:], ref[2:], rel, 'br gates', scale=1.0)
            assert_close(got[1], ref[1], rel, 'br C', scale=1e-5)


def test_pace_locations(gpu_lib, orc):
    from fib_tf_amd.fenton import Fenton4v
    for loc in ('left', 'right', 'top', 'bottom', 'luq', 'llq', 'ruq', 'rlq', 'nowhere'):
        m = Fenton4v(cfg(23, 31, 1.0))
        m.define(s1=False)
        rng = np.random.default_rng(3)
        u = rng.uniform(-0.2, 0.9, (23, 31)).astype(np.float32)
        m._stepper.set_state(0, u)
        m.add_pace_op('p', loc, 0.7)
        m.fire_op('p')
        s = np.full((23, 31), m.min_v, np.float32)
        H, W = 23, 31
        sl = {'left': (slice(None), slice(None, 5)), 'right': (slice(None), slice(-5, None)),
              'top': (slice(None, 5), slice(None)), 'bottom': (slice(-5, None), slice(None)),
              'luq': (slice(1, H // 2), slice(1, W // 2)), 'llq': (slice(H // 2, -1), slice(1, W // 2)),
              'ruq': (slice(1, H // 2), slice(W // 2, -1)), 'rlq': (slice(H // 2, -1), slice(W // 2, -1))}
        if loc in sl:
            s[sl[loc]] = 0.7
        assert np.array_equal(m._State['U'].eval(), np.maximum(u, s)), loc


def test_api_guards():
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v(cfg(16, 16, 1.0))
    with pytest.raises(AssertionError):
        m.add_pace_op('s2', 'luq', 1.0)          # before define, ionic.py:141-142
    m.defined = True
    with pytest.raises(AssertionError):
        m.add_hole_to_phase_field(8, 8, 2)       # after define, ionic.py:92-93


# --------------------------------------------------------------------------------------------
# court_ultra.py semantics: single rate, all variables every tick, checkpoint files
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
def test_court_ultra_trajectory(gpu_lib, golden, policy, tmp_path):
    from fib_tf_amd import court_ultra
    f = golden('court_ultra_traj')
    H, W = f['phase'].shape
    m = court_ultra.Courtemanche(cfg(H, W, float(f['diff']), policy, ultra_slow=False))
    m.phase = f['phase']
    m.define()
    m.add_pace_op('s2', 'luq', 10.0)
    for k in m.VAR_NAMES:
        assert np.array_equal(m._State[k].eval(), f['init_' + k])
    t0 = 0

    def hook(i):
        g = i + t0
        if g % 10 == 0:
            m.fire_op('slow')                      # an empty op in court_ultra.py: must change nothing
        if g == 50:
            m.fire_op('s2')

    scales = {'V': 150.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5}
    for t in [int(x) for x in f['snap_ticks']]:
        run_to(m, t - t0, hook)
        t0 = t
        for k in m.VAR_NAMES:
            assert_close(m._State[k].eval(), f['%s_t%d' % (k, t)], 2e-5, 'court_ultra %s t%d' % (k, t),
                         scale=scales.get(k, 1.0))
    # checkpoint round trip in the reference's file format, then resume
    m.duration = 1 * m.dt + 1e-9
    for _ in m.run(keep_state=True):
        pass
    court_ultra.save_state(tmp_path / 'state_small', m.state)
    st = court_ultra.load_state(tmp_path / 'state_small')
    assert set(st) == set(m.VAR_NAMES)
    m2 = court_ultra.Courtemanche(cfg(H, W, float(f['diff']), policy, ultra_slow=False))
    m2.phase = f['phase']
    m2.define(state=st)
    for k in m.VAR_NAMES:
        assert np.array_equal(m2._State[k].eval(), m.state[k])


@pytest.mark.parametrize('policy', POLICIES)
def test_court_ultra_slow_gate(gpu_lib, golden, orc, policy, capsys):
    """config['ultra_slow']=True: the 22-array model with the `_us_` gate (court_ultra.py:81-82,198-199,221-222,
    445-450), its two extra intermediates and the ϕ-weighted observer (court_ultra.py:465-486)"""
    from fib_tf_amd import court_ultra
    f = golden('court_ultra_us_traj')
    H, W = f['phase'].shape
    m = court_ultra.Courtemanche(cfg(H, W, float(f['diff']), policy, ultra_slow=True))
    m.phase = f['phase']
    m.define()
    m.add_pace_op('s2', 'luq', 10.0)
    assert m.VAR_NAMES[-1] == '_us_' and len(m.VAR_NAMES) == 22
    for k in m.VAR_NAMES:
        assert np.array_equal(m._State[k].eval(), f['init_' + k])
    t0 = 0

    def hook(i):
        if i + t0 == 50:
            m.fire_op('s2')

    # _u_/_v_: the SR-release sigmoids (width 1.367e-15 in Fn) amplify ulps of the currents; the oracle shows
    # 1.1e-5 against the same fixture (tests/test_oracle_golden.py)
    sr = 5.0 if policy == 'exact' else 15.0
    scales = {'V': 150.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5, '_u_': sr, '_v_': sr}
    for t in [int(x) for x in f['snap_ticks']]:
        run_to(m, t - t0, hook)
        t0 = t
        for k in m.VAR_NAMES:
            assert_close(m._State[k].eval(), f['%s_t%d' % (k, t)], 2e-5, 'court_ultra_us %s t%d' % (k, t),
                         scale=scales.get(k, 1.0))
    # the gate moves ~1e-7 per step: compare the accumulated change itself, not just the value
    us, ref = m._State['_us_'].eval(), f['_us__t120']
    assert np.max(np.abs(us - ref)) <= (2e-7 if policy == 'exact' else 2e-6)
    # calc_inter on the device vs the reference's sweep and the oracle
    inter = m.calc_inter(f['us_sweep_V'])
    tol = 2e-6 if policy == 'exact' else 2e-4
    # 1 - tanh(x) cancels for V >> -83 mV: an absolute ulp(1) of tanh is all that can be asked of us_infinity
    assert np.allclose(inter['us_infinity'], f['us_sweep_us_infinity'], rtol=tol, atol=3e-7 if policy == 'exact' else 3e-6)
    assert np.allclose(inter['tau_us'], f['us_sweep_tau_us'], rtol=tol, atol=0)
    # observer: 7 columns with ultra_slow (court_ultra.py:482)
    rows = []
    court_ultra.cl_observer(m, rows, 1000, 5, 77)
    assert len(rows) == 1 and len(rows[0]) == 7 and rows[0][:2] == [1005, 77]
    assert abs(rows[0][4] - np.average(us, weights=m.phase)) < 1e-6
    assert abs(rows[0][5] - np.average(m._Inter['us_infinity'].eval(), weights=m.phase)) < 1e-6
    assert '1005:' in capsys.readouterr().out


@pytest.mark.parametrize('policy', POLICIES)
def test_court_calc_inter_device(gpu_lib, golden, orc, policy):
    """Courtemanche.calc_inter evaluated by the device code: against the oracle on a voltage sweep that
    includes the neighbourhoods of every removable singularity, and against generate_table's values at -50 mV"""
    from fib_tf_amd import _lib
    vs = np.concatenate([np.linspace(-100, 50, 601), [-10.0001, 7.9, -47.13, -40.0, -14.1, 3.3328, 19.9, -50.0]]).astype(np.float32)
    got = _lib.court_inter(vs, fast=(policy == 'fast'))
    order = ('d_infinity', 'f_infinity', 'tau_w', 'tau_d', 'tau_f', 'w_infinity', 'm_inf', 'h_inf', 'j_inf', 'tau_oa',
             'tau_oi', 'tau_ua', 'tau_ui', 'tau_xr', 'tau_xs', 'tau_m', 'tau_h', 'tau_j', 'oa_infinity', 'oi_infinity',
             'ua_infinity', 'ui_infinity', 'xr_infinity', 'xs_infinity', 'g_Kur', 'f_NaK', 'i_NaCaa', 'i_NaCab', 'i_K1a',
             'i_Kra')                                          # courtemanche.h:105-134 order = orc_court_calc_inter
    want = np.stack([orc.court_calc_inter(float(v)) for v in vs], axis=1)          # [30, n]
    tol = 3e-6 if policy == 'exact' else 3e-4
    for k, name in enumerate(order):
        w, g = want[k], got[name]
        ok = np.abs(g - w) <= tol * np.maximum(np.abs(w), 1e-30)
        assert ok.all(), (name, vs[~ok][:5], g[~ok][:5], w[~ok][:5])


def test_run_with_screen_and_cycle_length_observer(gpu_lib, tmp_path):
    """run(im): a frame every dt_per_plot sub-steps and the cycle-length detector at pixel
    [20, width//2] (ionic.py:206-224), through the headless Screen"""
    from fib_tf_amd.fenton import Fenton4v
    from fib_tf_amd.screen import Screen
    m = Fenton4v(cfg(64, 96, 1.5, 'fast', duration=120, dt_per_plot=20))
    m.add_hole_to_phase_field(70, 40, 6)
    m.define()
    seen = []
    m.cl_observer = lambda i, cl: seen.append((i, cl))
    im = Screen(64, 96, 'test', keep=3)
    ticks = [i for i in m.run(im, block=True)]
    assert ticks == list(range(120))
    assert im.count == 60                                           # every int(20/10) = 2 ticks
    assert len(im.frames) == 3 and im.last.shape == (64, 96)
    assert len(seen) == 1 and 10 < seen[0][0] < 100                 # the S1 front passes column 48 once
    im.save(str(tmp_path / 'last.png'))
    assert open(tmp_path / 'last.png', 'rb').read(8) == b'\x89PNG\r\n\x1a\n'
    expect = m.image() * m.phase
    assert np.abs(im.last - expect).max() < 0.2                     # last frame was taken 1 tick earlier


# --------------------------------------------------------------------------------------------
# edge cases: tiny / skinny grids, every kernel family, odd fusion plans
# --------------------------------------------------------------------------------------------
TINY = [(3, 3), (3, 9), (4, 7), (5, 5), (9, 3), (2050, 6), (6, 1300), (64, 63), (65, 129)]


@pytest.mark.parametrize('shape', TINY, ids=['%dx%d' % s for s in TINY])
def test_fenton_tiny_and_skinny_grids(gpu_lib, orc, shape, monkeypatch):
    """3x3 is the smallest grid the reference's pads accept (interior of one cell: every tap clamps to it)"""
    from fib_tf_amd.fenton import Fenton4v
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    st = np.stack([rng.uniform(-0.05, 1.05, (H, W)), rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W)),
                   rng.uniform(0, 1, (H, W))]).astype(np.float32)
    phi = rng.uniform(0.2, 1.0, (H, W)).astype(np.float32)
    ref = st.copy()
    orc.fenton_run(ref, 0.1, 1.2, phi, 20)
    for variant in ('', '1,64,4,256', '5,32,32,256', '10,32,32,512', '5,54,21,-3', '2,60,18,-4', '10,44,25,-35',
                    '5,54,21,-35', '10,44,25,-3', '10,44,44,-4', '5,54,56,-4'):
        if variant:
            monkeypatch.setenv('FIBHIP_VARIANT', variant)
        else:
            monkeypatch.delenv('FIBHIP_VARIANT', raising=False)
        m = Fenton4v(cfg(H, W, 1.2, 'exact'))
        m.phase = phi
        m.define(s1=False)
        m._stepper.set_state(-1, st)
        run_to(m, 2)
        got = m._stepper.get_state()
        assert_close(got, ref, 3e-6, 'fenton %dx%d [%s]' % (H, W, variant), scale=1.0)


@pytest.mark.parametrize('spt', [1, 3, 7, 12])
def test_custom_steps_per_tick(gpu_lib, orc, spt):
    """steps_per_tick other than the reference's unroll factor: the launch plan mixes fusion depths
    (e.g. 7 = 5 + 2) and must still equal `spt` plain sub-steps"""
    from fib_tf_amd import _lib
    H, W = 70, 90
    rng = np.random.default_rng(spt)
    st = np.stack([rng.uniform(-0.05, 1.05, (H, W)), rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W)),
                   rng.uniform(0, 1, (H, W))]).astype(np.float32)
    phi = rng.uniform(0.2, 1.0, (H, W)).astype(np.float32)
    s = _lib.Stepper(_lib.FENTON4V, H, W, 0.1, 0.9, steps_per_tick=spt)
    s.set_state(-1, st)
    s.set_phase(phi)
    s.step(3)
    got = s.get_state()
    fused, launches = s.launch_plan()
    assert fused <= max(spt, 1) and launches >= 1
    ref = st.copy()
    orc.fenton_run(ref, 0.1, 0.9, phi, 3 * spt)
    assert_close(got, ref, 3e-6, 'spt=%d' % spt, scale=1.0)
    s.close()


def test_c_abi_argument_checks(gpu_lib):
    from fib_tf_amd import _lib
    with pytest.raises(_lib.FibhipError, match='at least 3x3'):
        _lib.Stepper(_lib.FENTON4V, 2, 8, 0.1, 1.0)
    with pytest.raises(_lib.FibhipError, match='unknown model'):
        _lib.Stepper(9, 8, 8, 0.1, 1.0)
    with pytest.raises(_lib.FibhipError, match='dt must be positive'):
        _lib.Stepper(_lib.FENTON4V, 8, 8, 0.0, 1.0)
    with pytest.raises(_lib.FibhipError, match='ghost'):
        _lib.Stepper(_lib.FENTON4V, 30, 8, 0.1, 1.0, global_height=60, row_offset=10, ghost_top=4, ghost_bottom=4)
    s = _lib.Stepper(_lib.BR, 8, 8, 0.1, 1.0, flags=_lib.CHEBY)
    with pytest.raises(_lib.FibhipError, match='Chebyshev table not set'):
        s.step(1)
    with pytest.raises(_lib.FibhipError, match='108'):
        s.set_consts(np.zeros(5, np.float32))
    s.close()
    c = _lib.Stepper(_lib.FENTON4V, 8, 8, 0.1, 1.0)
    with pytest.raises(_lib.FibhipError, match='Courtemanche only'):
        c.step_slow()
    with pytest.raises(_lib.FibhipError, match='out of range'):
        c.probe(0, 8, 0)
    c.close()


def test_timeline_and_save_graph_keys(gpu_lib, tmp_path, monkeypatch):
    """config['timeline'] / ['timeline_name'] / ['save_graph'] of the reference (ionic.py:190-191,231-241):
    timeline writes a Chrome-trace JSON for one extra tick; save_graph is accepted and ignored"""
    import json
    from fib_tf_amd.fenton import Fenton4v
    name = str(tmp_path / 'timeline_4v.json')
    m = Fenton4v(cfg(64, 64, 1.5, 'fast', duration=5, timeline=True, timeline_name=name, save_graph=True))
    m.define()
    before = None
    for i in m.run():
        before = i
    assert before == 4
    tr = json.load(open(name))
    fused, per_tick = m._stepper.launch_plan()
    assert len(tr['traceEvents']) == per_tick                       # one event per launch of the traced tick
    t_end = 0.0
    for ev in tr['traceEvents']:
        assert ev['ph'] == 'X' and ev['dur'] > 0 and ev['ts'] >= t_end - 1e-3 and 'kernel<K=%d' % fused in ev['name']
        assert ev['args']['sub_steps_fused'] == fused and ev['args']['tile'].count('x') == 1
        t_end = ev['ts'] + ev['dur']
    # a plan of several launches per tick: one event each, in order
    monkeypatch.setenv('FIBHIP_VARIANT', '2,60,18,-4')
    m = Fenton4v(cfg(64, 64, 1.5, 'fast', duration=2, timeline=True, timeline_name=name))
    m.define()
    for _ in m.run():
        pass
    tr = json.load(open(name))
    assert len(tr['traceEvents']) == 5 and all('strip_kernel<K=2, tile 60x18' in e['name'] for e in tr['traceEvents'])
    # Courtemanche: the tick and the pending machinery do not hide launches from the trace
    monkeypatch.delenv('FIBHIP_VARIANT')
    from fib_tf_amd.court import Courtemanche
    c = Courtemanche(cfg(64, 64, 0.809, 'fast', duration=1.05, timeline=True, timeline_name=name))
    c.define()
    for i in c.run():
        if i % 10 == 0:
            c.fire_op('slow')
    tr = json.load(open(name))
    assert len(tr['traceEvents']) >= 1 and tr['traceEvents'][0]['args']['ticks'] == 1


# --------------------------------------------------------------------------------------------
# fenton_simple.py / fenton_jit.py: the stand-alone scripts with the zero-padded convolution Laplacian
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
def test_fenton_simple_trajectory(gpu_lib, golden, policy, tmp_path, capsys):
    from fib_tf_amd.fenton_simple import Fenton4vSimple
    f = golden('fenton_simple_traj')
    H, W = f['init_U'].shape
    cfg_s = {'width': W, 'height': H, 'dt': 0.1, 'dt_per_plot': 10, 'diff': float(f['diff']), 'samples': 300,
             's2_time': int(f['s2_step']) * 0.1, 'fast_math': policy == 'fast',
             'timeline_name': str(tmp_path / 'timeline_simple.json')}
    got = {}
    for samples in (10, 100, 200, 300):                     # run() from the initial state to each snapshot
        m = Fenton4vSimple(dict(cfg_s, samples=samples))
        m.define()
        assert np.array_equal(m.state(), np.stack([f['init_' + k] for k in 'UVWS']))
        m.run(None)
        got[samples] = m.state()
        for k, n in enumerate('UVWS'):
            assert_close(got[samples][k], f['%s_t%d' % (n, samples)], 2e-5 if samples <= 100 else 1e-4,
                         'fenton_simple %s t%d' % (n, samples), scale=1.0)
    assert 'elapsed' in capsys.readouterr().out and (tmp_path / 'timeline_simple.json').exists()
    # fused (10 steps per launch when S2 and the end fall on multiples of 10) and one step per launch: bit-identical
    res = []
    for force1 in (False, True):
        m = Fenton4vSimple(dict(cfg_s, samples=300, s2_time=14.9))
        m.define()
        assert m._s2_step == 149 and m._spt == 10
        if force1:
            m._chunk = lambda with_frames: 1
        m.run(None)
        assert m._stepper.launch_plan() == ((1, 1) if force1 else (10, 1))
        res.append(m.state())
    assert np.array_equal(res[0], res[1])


def test_fenton_jit_with_screen(gpu_lib, tmp_path):
    """run(im): a frame of the RAW potential after every dt_per_plot-th step (fenton_simple.py:195-197); the class
    of fenton_jit.py is the same model"""
    from fib_tf_amd.fenton_simple import Fenton4vJIT
    from fib_tf_amd.screen import Screen
    m = Fenton4vJIT({'width': 64, 'height': 48, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'samples': 100,
                     's2_time': 5.0, 'timeline_name': str(tmp_path / 't.json')})
    m.define()
    im = Screen(48, 64, 'jit', keep=100)
    m.run(im)
    assert im.count == 10 and m._spt == 1                  # frames after steps 0, 10, ..., 90: no fusion possible
    assert np.array_equal(im.frames[-1].shape, (48, 64))
    ref = Fenton4vJIT({'width': 64, 'height': 48, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'samples': 100,
                       's2_time': 5.0, 'timeline_name': str(tmp_path / 't2.json')})
    ref.define()
    ref.run(None)
    assert np.array_equal(ref.state(), m.state())


def test_create_rejects_what_the_kernels_cannot_index(gpu_lib):
    """32-bit index arithmetic inside the kernels: a grid whose array view reaches 2^31 floats is refused at create
    time (before any allocation), as are the other malformed descriptions"""
    from fib_tf_amd import _lib
    with pytest.raises(_lib.FibhipError, match='32-bit'):
        _lib.Stepper(_lib.FENTON4V, 65536, 32768, 0.1, 1.0)
    with pytest.raises(_lib.FibhipError, match='at least 3x3'):
        _lib.Stepper(_lib.FENTON4V, 2, 100, 0.1, 1.0)
    with pytest.raises(_lib.FibhipError, match='dt must be positive'):
        _lib.Stepper(_lib.FENTON4V, 32, 32, 0.0, 1.0)
    with pytest.raises(_lib.FibhipError, match='Fenton 4v model only'):
        _lib.Stepper(_lib.BR, 32, 32, 0.1, 1.0, flags=_lib.ZEROPAD)
    with pytest.raises(_lib.FibhipError, match='unknown model'):
        _lib.Stepper(17, 32, 32, 0.1, 1.0)


def test_court_fused_slow_tick_small_shapes(gpu_lib, monkeypatch):
    """the one-launch tick + slow on awkward grids (3 rows, 3 columns, sizes around the 64x4 tile edges): same bits as
    the two-launch path; raw C ABI so that many shapes stay cheap"""
    from fib_tf_amd import _lib
    from fib_tf_amd.court import INITIAL
    rng = np.random.default_rng(7)
    shapes = [(3, 3), (3, 70), (70, 3), (4, 64), (5, 65), (6, 7), (8, 128), (9, 129), (13, 66), (66, 130), (7, 191)]
    for H, W in shapes:
        init = np.empty((21, H, W), np.float32)
        for i, (_, v) in enumerate(INITIAL):
            init[i] = v
        init[0] += rng.uniform(-5, 30, (H, W)).astype(np.float32)
        phi = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
        out = []
        for lazy in (True, False):
            if lazy:
                monkeypatch.delenv('FIBHIP_NO_LAZY', raising=False)
            else:
                monkeypatch.setenv('FIBHIP_NO_LAZY', '1')
            st = _lib.Stepper(_lib.COURT, H, W, 0.1, 0.809, flags=_lib.FAST | _lib.CHRONIC)
            st.set_phase(phi)
            st.set_state(-1, init)
            for i in range(23):
                st.step(1)
                if i % 10 == 0:
                    st.step_slow()
                if i == 12:
                    st.pace(0, max(1, H // 2), 0, max(1, W // 2), 10.0, -100.0)
            out.append(st.get_state(-1))
            st.close()
        assert np.array_equal(out[0], out[1]), (H, W)


def test_readback_into_page_locked_arrays(gpu_lib):
    """single-array read-backs (eval(), image()) land in page-locked buffers of a small pool, written by the device
    directly (fibhip_get_state_direct); the whole-state read-back takes the staged path: same bytes either way, a
    buffer is reused only after its array is gone, and beyond _lib.PINNED_MAX live arrays the binding falls back to
    pageable memory"""
    import gc
    from fib_tf_amd import _lib
    gc.collect()                       # page-locked arrays of earlier tests that only the collector can free leave the pool first
    rng = np.random.default_rng(3)
    H, W = 37, 53
    init = rng.uniform(0, 1, (4, H, W)).astype(np.float32)
    st = _lib.Stepper(_lib.FENTON4V, H, W, 0.1, 1.5, flags=_lib.FAST)
    st.set_state(-1, init)
    whole = st.get_state(-1)
    assert np.array_equal(whole, init)
    held = [st.get_state(v % 4) for v in range(_lib.PINNED_MAX + 3)]          # more live arrays than the pool has buffers
    for v, a in enumerate(held):
        assert np.array_equal(a, init[v % 4])
    addrs = {a.ctypes.data for a in held}
    assert len(addrs) == len(held)                                             # no two live arrays share memory
    first = held[0].ctypes.data
    keep = held[1].copy()
    del held[0]
    gc.collect()
    again = st.get_state(2)                                                    # takes the buffer that was just released
    assert again.ctypes.data == first and np.array_equal(again, init[2])
    assert np.array_equal(held[0], keep)                                       # the other arrays are untouched
    st.step(3)
    assert not np.array_equal(st.get_state(0), init[0])
    st.close()


def test_stock_library_kernel_after_specialised_library_kernel(gpu_lib, monkeypatch):
    """two builds of the library in one process: a Beeler-Reuter handle runs kernels from the specialised build (table as
    literals), then the first kernel launched from the STOCK library is the copy yardstick.  Under rocprofv3 this sequence
    died in round 2 (kernels of the same name in two fat binaries); every non-stock build now carries a build tag in its
    kernel symbols (csrc/models.hpp FIB_BUILD_TAG).  tools/prof_stock_after_spec.sh runs this test under the profiler."""
    import subprocess
    from fib_tf_amd import _lib
    from fib_tf_amd.br import BeelerReuter
    monkeypatch.delenv('FIBHIP_VARIANT', raising=False)
    m = BeelerReuter(cfg(96, 128, 0.809, 'fast', cheby=True))
    m.define()
    spec = m._library
    if spec is None:
        pytest.skip('no specialised build here (no compiler, none cached)')
    assert spec._name != _lib.SO
    m._stepper.step(7)
    m._stepper.sync()
    # no kernel symbol of the specialised build has a namesake in the stock library
    def kernel_syms(path):
        out = subprocess.check_output(['nm', '-D', '--defined-only', path]).decode()
        return {l.split()[-1] for l in out.splitlines() if '_kernel' in l}
    assert kernel_syms(spec._name) and not (kernel_syms(spec._name) & kernel_syms(_lib.SO))
    assert _lib.copy_bandwidth(1 << 26, 2) > 100.0          # stock library, first launch from it
    m._stepper.step(3)
    m._stepper.sync()
    assert np.isfinite(m._State['V'].eval()).all()


def test_copy_bandwidth_yardstick(gpu_lib):
    """fibhip_copy_bandwidth: the plain streaming copy bench.py reports next to the roofline peak"""
    from fib_tf_amd import _lib
    gbs = _lib.copy_bandwidth(1 << 28, 3)
    assert 500.0 < gbs < 8000.0, gbs                       # an MI355X does several TB/s; 8 TB/s is the HBM3E peak
    with pytest.raises(_lib.FibhipError):
        _lib.copy_bandwidth(1024, 1)
