"""Shared by tests/test_gpu_tensor.py, tests/test_gpu_tensor_models.py, tests/test_tensor_oracle_cpu.py and
tools/tensor_accuracy.py: the fibre fields, states, handles, mutants of the operator and the comparisons of a tensor handle of
every model with the oracle stepping under `oracle.tensor` (oracle/fib_oracle.c orc_set_tensor: tests/tensor_ref.py laplace32 in
laplace's place).  The bounds, plays, scales and masks are imported from where the stock handles' tests keep them
(tests/test_gpu_variant_table.py, tests/timestep_cases.py); nothing here is fitted to what the device gives.

    (a) one tick against the oracle          device_tick / compare_tick / oracle_tick_V
    (b) one sub-step taken apart             substep_figures (the derivations stand beside the forms)
    (c) trajectories on oblique fibres       traj_setup / oracle_traj / device_traj / traj_figures
    mutants(params)                          the tensors a subtly wrong kernel would effectively apply"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tensor_ref  # noqa: E402
import timestep_cases as tc  # noqa: E402
from test_gpu_variant_table import (BR_DIFF, COURT_DIFF, COURT_PLAY, COURT_PLAY_ALL, COURT_STEP_SCALES, FAST_STEP_TOL, FENTON_DIFF,  # noqa: E402,F401
                                    NEAR_CAP, Worst, br_reference, br_state, br_table, clear_env, court_near_singular, court_oracle,
                                    court_state, fenton_state, oracle_error_bar)

FENTON, BR, COURT, COURT_US = 0, 1, 2, 3
U24 = 2.0 ** -24
# rounded operations on the longest path of the Fast form, prepared planes included: derived beside the form itself
# (csrc/stencil.hpp lap9_tensor) — 5 for the second-order part, 3 for its weights, 2 for the first-order term's two FMAs
N_FAST = 10
DIFF = {FENTON: 1.2, BR: 0.809, COURT: 0.809, COURT_US: 0.809}
DT = 0.1
GRIDS = [(70, 75), (9, 129), (65, 33)]       # no multiple of the 64 x 4 or 32 x 32 tiles; on 9 x 129 a tick and 'slow' cannot fuse
ANCHOR_ENV = {'FIBHIP_VARIANT': '1,64,4,256', 'FIBHIP_NO_LAZY': '1'}     # the K = 1 row, as test_every_row forces it


# ---- fields ---------------------------------------------------------------------------------------------------------------------
def spd_params(H, W, seed):
    """(angle, ratio, scale) of spd_field"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-np.pi, np.pi, (H, W)), rng.uniform(1.0, 3.0, (H, W)), rng.uniform(0.3, 1.0, (H, W))


def spd_field(H, W, seed):
    """a random fibre field: angle, ratio <= 3 and scale all varying from cell to cell"""
    return tensor_ref.fibre_planes(*spd_params(H, W, seed))


def hole_field(H, W):
    """add_hole_to_phase_field's plane for a hole in the middle, radius a sixth of the shorter side"""
    return disc_hole(H, W, H // 2, W // 2, min(H, W) / 6.0)


def disc_hole(H, W, row, col, radius):
    rows, cols = np.arange(H)[:, None] - row, np.arange(W)[None, :] - col
    mask = np.array(0.5 * (np.tanh(np.hypot(cols, rows) - radius) + 1.0), dtype=np.float32)
    return np.maximum(mask, np.float32(1e-5))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def unit_values(H, W):
    rng = np.random.default_rng(H * 100 + W)
    X = rng.standard_normal((H, W)).astype(np.float32)
    flat = X.reshape(-1)
    n = flat.size
    flat[rng.choice(n, max(2, n // 10), replace=False)] = 0.0            # exact zeros
    flat[1], flat[n // 2] = np.float32(1e-20), np.float32(-1e20)          # edge magnitudes, far from the denormals
    flat[n // 3] = np.inf
    return X


def mutants(params):
    """name -> (dyy, dxx, dxy): what a subtly wrong kernel would effectively apply in place of fibre_planes(*params) — the
    weight planes of the two axes swapped, the sign of dxy, no tensor at all, no heterogeneity (so no div D part), and an
    anisotropy ratio or an angle that is a little off"""
    angle, ratio, scale = (np.asarray(p, np.float64) for p in params)
    dyy, dxx, dxy = tensor_ref.fibre_planes(angle, ratio, scale)
    one = np.ones_like(dyy)
    return {'dxx for dyy': (dxx, dyy, dxy),
            '-dxy': (dyy, dxx, -dxy),
            'identity': (one, one, 0 * one),
            'mean tensor': tuple(np.full_like(p, p.mean(dtype=np.float64)) for p in (dyy, dxx, dxy)),
            'ratio 2.9 for 3': tensor_ref.fibre_planes(angle, ratio * (2.9 / 3.0), scale, shape=dyy.shape),
            'angle + 0.01': tensor_ref.fibre_planes(angle + 0.01, ratio, scale, shape=dyy.shape)}


def first_order_without_div(dyy, dxx, dxy, phi, dtype=np.float32):
    """tensor_ref.first_order with the div D part dropped: Fenton's one more mutant, patched into the NumPy sub-step"""
    t = dtype
    dyy, dxx, dxy = (np.asarray(p, t) for p in (dyy, dxx, dxy))
    phi = np.ones_like(dyy) if phi is None else np.asarray(phi, t)
    dpy, dpx = tensor_ref._dy(phi), tensor_ref._dx(phi)
    return dyy * dpy + dxy * dpx, dxy * dpy + dxx * dpx, t(4.0) * phi


# ---- handles --------------------------------------------------------------------------------------------------------------------
CASES = {   # name -> (model, flags without the policy, state maker)
    'fenton': (FENTON, 0, fenton_state),
    'br-direct': (BR, 0, br_state),
    'br-cheby': (BR, 1, br_state),                                       # FIBHIP_CHEBY
    'court': (COURT, 4, court_state),                                     # FIBHIP_CHRONIC; the fast / slow mix
    'court-all': (COURT, 4 | 16, court_state),                            # FIBHIP_ALLVARS
    'court-us': (COURT_US, 4, lambda H, W: court_state(H, W, us=True)),
}
MORE_CASES = {  # the multirate schedule of Beeler-Reuter (FIBHIP_SKIP) and acute Courtemanche: tests/test_gpu_tensor_models.py
    'br-direct-skip': (BR, 2, br_state),
    'br-cheby-skip': (BR, 1 | 2, br_state),
    'court-acute': (COURT, 0, court_state),
    'court-all-acute': (COURT, 16, court_state),
    'court-us-acute': (COURT_US, 0, lambda H, W: court_state(H, W, us=True)),
}
ALL_CASES = dict(CASES, **MORE_CASES)


def handle(name, H, W, fast, phi=None, tensor=None, spt=0, diff=None, state=None):
    from fib_tf_amd import _lib
    model, flags, make = ALL_CASES[name]
    st = _lib.Stepper(model, H, W, DT, DIFF[model] if diff is None else diff, flags=flags | (_lib.FAST if fast else 0), steps_per_tick=spt)
    if flags & 1:
        st.set_consts(br_table())
    if phi is not None:
        st.set_phase(phi)
    if tensor is not None:
        st.set_tensor(*tensor)
    st.set_state(-1, make(H, W)[0] if state is None else state)
    return st


def run_ticks(st, name, n):
    """n ticks; Courtemanche's two-rate handle fires 'slow' once, right behind a tick, as the reference's driver does"""
    if name == 'court':
        st.step(n - 2)
        st.step(1)
        st.step_slow()
        st.step(1)
    else:
        st.step(n)
    return st.get_state(-1)


def kind_of(name):
    model, flags, _ = ALL_CASES[name]
    return {'model': model, 'cheby': model == BR and bool(flags & 1), 'skip': model == BR and bool(flags & 2), 'chronic': bool(flags & 4),
            'allv': bool(flags & 16), 'us': model == COURT_US, 'two_rate': model == COURT and not flags & 16}


def court_names(orc, name):
    return list(orc.COURT_VARS) + (['_us_'] if kind_of(name)['us'] else [])


# ---- (a) one tick against the oracle --------------------------------------------------------------------------------------------
def tick_fields(name, H, W, hole):
    """(state, phase or None, tensor planes, their parameters) of comparison (a)"""
    params = spd_params(H, W, 17 + H)
    return ALL_CASES[name][2](H, W)[0], (hole_field(H, W) if hole else None), tensor_ref.fibre_planes(*params), params


def tick_script(name):
    k = kind_of(name)
    return [2] if k['model'] == FENTON else [1] if k['model'] == BR else COURT_PLAY if k['two_rate'] else COURT_PLAY_ALL


def device_tick(name, H, W, fast, hole, monkeypatch):
    """the play of (a) on the K = 1 row: the state compared with the oracle (Fenton: after 20 sub-steps; Beeler-Reuter and
    Courtemanche: after the first tick, as test_br_rows and test_court_rows compare), and the launches the timed part took"""
    clear_env(monkeypatch, **ANCHOR_ENV)
    state, phi, D, _ = tick_fields(name, H, W, hole)
    st = handle(name, H, W, fast, phi, D)
    try:
        assert st.plan_tile() == (64, 4, -256) and st.launch_plan()[0] == 1, 'the forced row is not the plan'
        obs, launches = [], None
        for op in tick_script(name):
            if op == 'all':
                obs.append(st.get_state(-1))
            elif op == 'slow':
                st.step_slow()
            elif op == 'tb':
                st.time_begin()
            elif op == 'te':
                launches = st.time_end()[1]
            else:
                st.step(op)
        obs.append(st.get_state(-1))
    finally:
        st.close()
    for x in obs:
        assert np.isfinite(x).all(), 'non-finite values'
    return obs[0], launches


def _court_run(orc, name):
    k = kind_of(name)
    if k['us']:
        return lambda ref, phi: orc.court_ultra_us_run(ref, DT, COURT_DIFF, phi, k['chronic'], 1)
    if k['allv']:
        return lambda ref, phi: orc.court_ultra_run(ref, DT, COURT_DIFF, phi, k['chronic'], 1)
    return lambda ref, phi: orc.court_run(ref, DT, COURT_DIFF, phi, k['chronic'], 1, 1)


def tick_tol(name, fast):
    """the bound of (a) and the potential's scale: test_fenton_rows', test_br_rows' and test_court_rows'"""
    k = kind_of(name)
    if k['model'] == FENTON:
        return (20 * FAST_STEP_TOL if fast else 3e-6), 1.0
    if k['model'] == BR:
        return (5 * FAST_STEP_TOL if fast else (5e-5 if k['cheby'] else 1e-5)), 120.0
    return (FAST_STEP_TOL if fast else 6e-6), COURT_STEP_SCALES['V']


def compare_tick(orc, worst, name, fast, H, W, hole, got):
    """device state `got` of device_tick against the oracle with the tensor, into `worst` — the comparisons of
    test_fenton_rows ('oracle'), test_br_rows (build 'oracle') and test_court_rows, with their bounds"""
    state, phi, D, _ = tick_fields(name, H, W, hole)
    k = kind_of(name)
    tol, _ = tick_tol(name, fast)
    key = '%s %s hole=%d' % (name, 'fast' if fast else 'exact', hole)
    where = '%dx%d' % (H, W)
    with orc.tensor(*D):
        if k['model'] == FENTON:
            ref = state.copy()
            orc.fenton_run(ref, DT, FENTON_DIFF, phi, 20)
            worst.add(key, got, ref, tol, 1.0, where)
        elif k['model'] == BR:
            ref, ill, lo, hi = br_reference(orc, state, phi, br_table() if k['cheby'] else None, k['skip'], 5e-5 if k['cheby'] else 1e-5)
            g = got.astype(np.float64)
            excess = np.maximum(lo - g, g - hi) - 3.0 * (hi - lo)
            for what, sl, scale in ((' V', slice(0, 1), 120.0), (' gates', slice(2, 8), 1.0), (' C', slice(1, 2), 1e-5)):
                worst.add(key + what, g[sl], ref[sl], tol, scale, where, mask=ill)
                worst.add_ill(key + what, excess[sl], tol, scale, where, ill)
        else:
            court_oracle(orc, worst, key, court_names(orc, name), state, phi, got, _court_run(orc, name), tol)


def oracle_tick_V(orc, name, H, W, hole, D):
    """the potential of (a)'s play from the oracle alone, under tensor D"""
    state, phi, _, _ = tick_fields(name, H, W, hole)
    k = kind_of(name)
    ref = state.copy()
    with orc.tensor(*D):
        if k['model'] == FENTON:
            orc.fenton_run(ref, DT, FENTON_DIFF, phi, 20)
        elif k['model'] == BR:
            orc.br_run(ref, DT, BR_DIFF, phi, br_table() if k['cheby'] else None, k['skip'], 1)
        else:
            _court_run(orc, name)(ref, phi)
    return ref[0]


# ---- (b) one sub-step taken apart -----------------------------------------------------------------------------------------------
BR_CLIP = (np.float32(-85.0), np.float32(25.0))


def substep_figures(name, fast, s0, T, got, D, phi):
    """`got` = the state one sub-step after `s0` on a handle with tensor D and the model's diff; `T` = the same on a handle
    without a tensor and diff = 0.  Returns (arrays other than the potential that differ from T's, figures); a figure is
    (what, value, bound) and the test asserts value <= bound.

    V0 = enforce_boundary(s0[0]); ddt = float32(diff * dt); the sub-step's potential is T + ddt * L(V0) up to its roundings.

    Exact policy, a = RN(ddt * laplace32(V0)):
      Fenton, Courtemanche (FAST, ALL, US): the kernels form o = DV + ddt * lap with DV == T, so V1 == RN(T + a): the figure is
        the number of cells where it is not, bound 0.
      Beeler-Reuter: V1 = clip(RN(RN(V0 + a) - x)) and T = clip(RN(V0 - x)), x = dt * I_sum.  Off the clip
        V1 - T - a = (RN(V0 + a) - (V0 + a)) + (V1 - (RN(V0 + a) - x)) - (T - (V0 - x)): three roundings of at most half an ulp,
        |.| <= 2^-24 (|V0 + a| + |V1| + |T|).  Cells where V1 or T sits on the clip are left out (their share is a figure, bound
        NEAR_CAP).
    Fast policy, a = ddt * laplace64(V0) in float64: the same three roundings at most (a fused multiply-add only removes one),
      and the operator itself within the unit op's bound N_FAST 2^-24 terms64 (test_unit_op), times ddt:
        |V1 - T - a| <= 2^-24 (|V0 + a| + |V1| + |T|) + ddt N_FAST 2^-24 terms64(V0)."""
    k = kind_of(name)
    model = k['model']
    others = [v for v in range(1, T.shape[0]) if not same(got[v], T[v])]
    V0 = np.pad(s0[0][1:-1, 1:-1], 1, mode='edge')
    ddt = np.float32(DIFF[model] * DT)
    V1, T0 = got[0].astype(np.float64), T[0].astype(np.float64)
    tag = '%s %s' % (name, 'fast' if fast else 'exact')
    keep = np.ones(V0.shape, bool)
    figs = []
    if model == BR:
        keep = ~(np.isin(got[0], BR_CLIP) | np.isin(T[0], BR_CLIP))
        figs.append((tag + ' share of cells on the clip', float(1.0 - keep.mean()), NEAR_CAP))
    if not fast:
        a = ddt * tensor_ref.laplace32(V0, *D, phi)
        assert a.dtype == np.float32
        if model != BR:
            figs.append((tag + ' cells with V1 != RN(T + a)', float((got[0] != T[0] + a).sum()), 0.0))
            return others, figs
        a = a.astype(np.float64)
        bound = U24 * (np.abs(V0 + a) + np.abs(V1) + np.abs(T0))
    else:
        a = float(ddt) * tensor_ref.laplace64(V0, *D, phi)
        bound = U24 * (np.abs(V0 + a) + np.abs(V1) + np.abs(T0)) + float(ddt) * N_FAST * U24 * tensor_ref.terms64(V0, *D, phi)
    ratio = np.abs(V1 - T0 - a)[keep] / bound[keep]
    figs.append((tag + ' worst |V1 - T - a| / bound', float(ratio.max()), 1.0))
    return others, figs


# ---- (c) trajectories on oblique, heterogeneous fibres --------------------------------------------------------------------------
TRAJ_N, TRAJ_SNAPS = 64, (10, 20)
TRAJ_CASES = ['fenton', 'br-direct', 'br-cheby', 'br-direct-skip', 'br-cheby-skip', 'court', 'court-us']


def traj_params():
    """fibres turning from pi / 8 to 3 pi / 8 across the columns at ratio 3, the conductivity falling from 1 to 0.6 up the
    rows (div D != 0)"""
    n = TRAJ_N
    angle = np.broadcast_to(np.linspace(np.pi / 8, 3 * np.pi / 8, n)[None, :], (n, n))
    scale = np.broadcast_to(np.linspace(0.6, 1.0, n)[:, None], (n, n))
    return angle, np.full((n, n), 3.0), scale


def traj_setup(name):
    """(initial state, phase, tensor planes): the model's resting state with a disc of radius 6 around (20, 20) raised — where
    dxy is largest, so the wave runs obliquely to the fibres — and a hole of radius 8 at the centre"""
    from fib_tf_amd.court import INITIAL
    n = TRAJ_N
    k = kind_of(name)
    rest, up = {FENTON: ((0.0, 1.0, 1.0, 0.0), 1.0), BR: ((-84.624, 1e-4, 0.01, 0.988, 0.975, 0.003, 0.994, 0.0001), 10.0),
                COURT: (tuple(v for _, v in INITIAL), 20.0), COURT_US: (tuple(v for _, v in INITIAL) + (0.72,), 20.0)}[k['model']]
    state = np.empty((len(rest), n, n), np.float32)
    for i, v in enumerate(rest):
        state[i] = v
    rows, cols = np.arange(n)[:, None] - 20, np.arange(n)[None, :] - 20
    state[0][np.hypot(rows, cols) <= 6.0] = up
    return state, disc_hole(n, n, n // 2, n // 2, 8.0), tensor_ref.fibre_planes(*traj_params())


def oracle_traj(orc, name, D=None, state=None):
    """{tick: state} from the oracle under tensor D (default: the field of traj_setup), from `state` (default: traj_setup's)"""
    state0, phi, D0 = traj_setup(name)
    state = state0 if state is None else state
    k = kind_of(name)
    slab, snaps, t0 = state.copy(), {}, 0
    with orc.tensor(*(D0 if D is None else D)):
        for t in TRAJ_SNAPS:
            if k['model'] == FENTON:
                orc.fenton_run(slab, DT, FENTON_DIFF, phi, 10 * (t - t0))
            elif k['model'] == BR:
                orc.br_run(slab, DT, BR_DIFF, phi, br_table() if k['cheby'] else None, k['skip'], t - t0)
            elif k['us']:
                orc.court_ultra_us_run(slab, DT, COURT_DIFF, phi, k['chronic'], t - t0)
            else:
                orc.court_run(slab, DT, COURT_DIFF, phi, k['chronic'], t0 + 1, t - t0)     # 'slow' behind ticks 10 and 20
            snaps[t], t0 = slab.copy(), t
    return snaps


def device_traj(name, fast):
    state, phi, D = traj_setup(name)
    st = handle(name, TRAJ_N, TRAJ_N, fast, phi, D, state=state)
    snaps, t0 = {}, 0
    try:
        for t in TRAJ_SNAPS:
            st.step(t - t0)
            if kind_of(name)['two_rate']:
                st.step_slow()
            snaps[t], t0 = st.get_state(-1), t
    finally:
        st.close()
    return snaps


_ENVELOPE = {}
EXCEPTION_TICK = 10        # traj_figures' named exception: H at this snapshot, fast policy, Chebyshev gates


def br_traj_envelope(orc, name):
    """(cells where the oracle's own H spreads by more than 2 TRAJ_TOL at tick EXCEPTION_TICK, lower envelope, upper envelope; the
    envelopes as [tick][array]) of oracle_error_bar: the trajectory again with exp() moved by -1 / +1 ulp and with the initial
    potential moved by -2 .. +2 float32 neighbours.  oracle_error_bar asserts that at most NEAR_CAP of the cells are such."""
    if name not in _ENVELOPE:
        state, _, _ = traj_setup(name)
        bounds = np.full(8 * len(TRAJ_SNAPS), np.inf)
        bounds[8 * TRAJ_SNAPS.index(EXCEPTION_TICK) + tc.BR_VARS.index('H')] = 2 * tc.TRAJ_TOL

        def run(st):
            snaps = oracle_traj(orc, name, state=st)
            return np.concatenate([snaps[t] for t in TRAJ_SNAPS])

        _, ill, lo, hi = oracle_error_bar(orc, run, state, bounds)
        _ENVELOPE[name] = (ill, {t: lo[8 * j:8 * j + 8] for j, t in enumerate(TRAJ_SNAPS)}, {t: hi[8 * j:8 * j + 8] for j, t in enumerate(TRAJ_SNAPS)})
    return _ENVELOPE[name]


def traj_figures(orc, name, fast, snaps, ref):
    """the figures of the stock trajectory tests at this horizon (<= 20 ticks: TRAJ_TOL of range under both policies, the named
    exceptions of br_traj_figures included), with the oracle's snapshots `ref` where those read a fixture.

    NAMED EXCEPTION — fast policy, Chebyshev gates, H at tick 10 on this field, and nothing else (M, and H at tick 20, keep
    br_traj_figures' own bound): the figure is the distance from the oracle's own envelope over the margin 3 x the envelope's
    width + the ordinary bound (2 TRAJ_TOL = 4e-5), at every cell, bound 1 — the form timestep_cases.court_step_figures and
    Worst.add_ill apply where the oracle itself is ill-conditioned.  Where the oracle is well-conditioned the width is nothing
    and this is the ordinary bound; the envelope is wider than the bound on about 1 % of the cells (tests/
    test_tensor_oracle_cpu.py holds that share under NEAR_CAP).  The price: where the envelope is 5.1e-5 wide, as at cell
    (16, 10), the margin is 3 x 5.1e-5 + 4e-5 = 1.9e-4 beyond the envelope, up to 2.4e-4 from the oracle's own value — six times
    the stock bound there, for a miss of 6 %; at the widest cell (1.0e-4, skip) 3.4e-4 beyond the envelope.
    Why: the disc's wave is curved and oblique to the fibres, so at tick 10 a ring of cells stands on the upstroke
    (-60 .. -30 mV), where h falls from 1 at the rate (alpha_h + beta_h)(V) whose slope is 0.02 per ms per mV: a potential
    1e-3 mV off for the 2 - 3 ms of the foot — a fifth of the potential's own bound of 4.8e-3 mV — moves h by 4e-5.  The
    reference's float32 arithmetic does not pin the potential that well: the oracle with exp() one ulp up moves H by 3.76e-5 at
    cell (16, 10) (V = -41.9 mV, H = 0.855) beside 8.5e-4 mV in V; with every coefficient of the Chebyshev table one float32
    neighbour up, by 4.71e-5 at (29, 29).  The fast policy, whose degree-8 sums round at other points (fused multiply-adds),
    measured H 4.250e-5 at that cell (16, 10) (envelope 5.1e-5 wide there) and, with skip, 4.047e-5 at (21, 10) (2.2e-5 wide),
    both at tick 10, beside potentials 4.2e-4 and 5.3e-5 mV off; H at tick 20 2.2e-5, M at most 2.0e-5, every other figure of the
    fast policy <= 0.61 of its bound, H under the exact policy 8.2e-6 of 2e-5."""
    k = kind_of(name)
    policy = 'fast' if fast else 'exact'
    if k['model'] == FENTON:
        return tc.fenton_traj_figures(snaps, {'%s_t%d' % (v, t): ref[t][i] for t in ref for i, v in enumerate('UVWS')})
    if k['model'] == BR:
        tag = ('cheby' if k['cheby'] else 'direct') + ('_skip' if k['skip'] else '')
        f = {'%s_%s_t%d' % (tag, v, t): ref[t][i] for t in ref for i, v in enumerate(tc.BR_VARS)}
        f['dt'] = DT
        figs = tc.br_traj_figures(snaps, f, tag, policy)
        if not (fast and k['cheby']):
            return figs
        _, lo, hi = br_traj_envelope(orc, name)
        out = []
        for what, err, bound in figs:
            if what != 'br %s H t%d' % (tag, EXCEPTION_TICK):
                out.append((what, err, bound))
                continue
            t, i = EXCEPTION_TICK, tc.BR_VARS.index('H')
            got = snaps[t][i].astype(np.float64)
            margin = 3.0 * (hi[t][i] - lo[t][i]) + bound
            dist = np.maximum(np.maximum(lo[t][i] - got, got - hi[t][i]), 0.0) / margin
            out.append((what + ' outside the oracle\'s envelope, over 3 x its width + %.0e' % bound,
                        float(dist.max()) if np.isfinite(got).all() else float('inf'), 1.0))
        return out
    names = court_names(orc, name)
    f = {'%s_t%d' % (v, t): ref[t][i] for t in ref for i, v in enumerate(names)}
    if k['us']:
        return tc.court_traj_figures(snaps, None, f, names, tc.COURT_ULTRA_SCALES, 'court_ultra')
    return tc.court_traj_figures(snaps, None, f, names)


def traj_tol_V(name):
    """the potential's bound in traj_figures under the exact policy"""
    return tc.TRAJ_TOL * {FENTON: 1.0, BR: 120.0, COURT: 150.0, COURT_US: 150.0}[kind_of(name)['model']]


def moved(V, V_mutant, bound):
    """(largest move of the potential over the bound, share of the cells moved by more than the bound)"""
    d = np.abs(np.asarray(V, np.float64) - np.asarray(V_mutant, np.float64))
    return float(d.max() / bound), float((d > bound).mean())
