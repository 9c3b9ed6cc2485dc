"""-m gpu: fibre fields on the device (include/fibhip.h fibhip_set_tensor) against tests/tensor_ref.py, the
restatement of the operator in NumPy: the unit op, the identity tensor against the stock handle, every row of the second variant
table, one sub-step taken apart, plane-wave speeds along and across the fibres, the recorders beside a tensor, and the refusals
through the C ABI.  Bit comparisons use np.array_equal (a zero may change sign)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tensor_ref  # noqa: E402
from tensor_cases import (BR, CASES, COURT, COURT_US, DIFF, FENTON, N_FAST, U24, handle, hole_field, run_ticks, same,  # noqa: E402
                          spd_field, unit_values)
from test_gpu_variant_table import clear_env, fenton_state  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- 4. the unit op -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hole', [False, True], ids=['plain', 'hole'])
@pytest.mark.parametrize('shape', [(5, 4), (13, 17), (70, 75)], ids=lambda s: '%dx%d' % s)
def test_unit_op(shape, hole):
    from fib_tf_amd import _lib
    H, W = shape
    X, (dyy, dxx, dxy) = unit_values(H, W), spd_field(H, W, 3 + H)
    phi = hole_field(H, W) if hole else None
    exact = _lib.unit_laplace_tensor(X, dyy, dxx, dxy, phi=phi, fast=False)
    want = tensor_ref.laplace32(X, dyy, dxx, dxy, phi)
    assert np.isfinite(want).sum() > want.size // 2
    assert same(exact, want), 'exact policy: %d cells differ from the float32 restatement' % int((exact != want).sum())
    fast = _lib.unit_laplace_tensor(X, dyy, dxx, dxy, phi=phi, fast=True)
    ref, bound = tensor_ref.laplace64(X, dyy, dxx, dxy, phi), N_FAST * U24 * tensor_ref.terms64(X, dyy, dxx, dxy, phi)
    fin = np.isfinite(bound)
    err = np.abs(fast[fin].astype(np.float64) - ref[fin])
    print('fast policy: worst error / bound = %.3f over %d cells' % (float((err / np.maximum(bound[fin], 1e-300)).max()), int(fin.sum())))
    assert np.all(err <= bound[fin])
    assert not np.isfinite(fast[~fin]).any()                              # (the inf's neighbours: non-finite on both sides)


def test_model_laplace_uses_the_tensor():
    from fib_tf_amd.fenton import Fenton4v
    H, W = 13, 17
    m = Fenton4v({'width': W, 'height': H, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.2, 'duration': 1, 'fast_math': False})
    m.add_hole_to_phase_field(8, 6, 3)
    dyy, dxx, dxy = spd_field(H, W, 9)
    m.set_tensor(dyy, dxx, dxy)
    X = np.random.default_rng(2).standard_normal((H, W)).astype(np.float32)
    assert same(m.laplace(X), tensor_ref.laplace32(X, dyy, dxx, dxy, m.phase))


# ---- handles ---------------------------------------------------------------------------------------------------------------------
# (CASES, handle and run_ticks: tests/tensor_cases.py)


# ---- 5. the identity tensor is no tensor -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('hole', [False, True], ids=['plain', 'hole'])
@pytest.mark.parametrize('name', list(CASES))
def test_identity_tensor_exact(name, hole, monkeypatch):
    clear_env(monkeypatch)
    H, W = 70, 75
    phi = hole_field(H, W) if hole else None
    one, zero = np.ones((H, W), np.float32), np.zeros((H, W), np.float32)
    a, b = handle(name, H, W, False, phi), handle(name, H, W, False, phi, (one, one, zero))
    try:
        want, got = run_ticks(a, name, 12), run_ticks(b, name, 12)
        assert b.plan_tile()[2] < 0 and b.ticks_per_launch() == 1        # flat tiles, one launch per tick or part of it
    finally:
        a.close()
        b.close()
    assert np.isfinite(want).all()
    for v in range(want.shape[0]):
        assert same(got[v], want[v]), 'array %d: %d cells differ' % (v, int((got[v] != want[v]).sum()))


@pytest.mark.parametrize('hole', [False, True], ids=['plain', 'hole'])
@pytest.mark.parametrize('name', list(CASES))
def test_identity_tensor_fast_one_substep(name, hole, monkeypatch):
    """Fast policy, one sub-step: the two forms of the Laplacian re-associate differently, so the potential may differ — by at
    most float(diff * dt) times the unit op's bound (for the states drawn here that covers the last rounding of the potential
    as well: its ulp is far below diff * dt * 10 * 2^-24 * sum |term|) — and nothing else does.  FIBHIP_COURT_AGG=0: the stock
    handle on the plain kernels too, which a tensor handle always runs."""
    clear_env(monkeypatch, FIBHIP_COURT_AGG='0')
    H, W = 70, 75
    phi = hole_field(H, W) if hole else None
    one, zero = np.ones((H, W), np.float32), np.zeros((H, W), np.float32)
    model = CASES[name][0]
    a, b = handle(name, H, W, True, phi, spt=1), handle(name, H, W, True, phi, (one, one, zero), spt=1)
    try:
        s0 = a.get_state(-1)
        a.step(1)
        b.step(1)
        want, got = a.get_state(-1), b.get_state(-1)
    finally:
        a.close()
        b.close()
    for v in range(1, want.shape[0]):
        assert same(got[v], want[v]), 'array %d: %d cells differ' % (v, int((got[v] != want[v]).sum()))
    V0 = np.pad(s0[0][1:-1, 1:-1], 1, mode='edge')                        # enforce_boundary
    bound = float(np.float32(DIFF[model] * 0.1)) * N_FAST * U24 * tensor_ref.terms64(V0, one, one, zero, phi)
    err = np.abs(got[0].astype(np.float64) - want[0])
    print('%s: worst |dV| / bound = %.3f' % (name, float((err / bound).max())))
    assert np.all(err <= bound)


@pytest.mark.parametrize('name', ['fenton', 'court'])
def test_set_phase_and_removal_on_a_tensor_handle(name, monkeypatch):
    """fibhip_set_phase on a tensor handle prepares the tensor's planes again: field first or tensor first, the same run; and a
    handle whose tensor was removed is the stock handle again (Courtemanche, fast policy: back on its aggregates)"""
    clear_env(monkeypatch)
    H, W = 70, 75
    phi, D = hole_field(H, W), spd_field(H, W, 41)
    a, b = handle(name, H, W, True, phi, D), handle(name, H, W, True, None, D)
    c, d, e = handle(name, H, W, True, phi), handle(name, H, W, True, phi, D), handle(name, H, W, True, None, D)
    try:
        b.set_phase(phi)
        first = run_ticks(a, name, 4)
        assert same(run_ticks(b, name, 4), first)
        assert not same(run_ticks(e, name, 4), first)                     # (the field is seen)
        d.set_tensor(None)
        assert d.ticks_per_launch() == c.ticks_per_launch() and d.plan_tile() == c.plan_tile()
        assert same(run_ticks(d, name, 4), run_ticks(c, name, 4))
    finally:
        for st in (a, b, c, d, e):
            st.close()


# ---- 6. every row of the second table --------------------------------------------------------------------------------------------
def _tensor_rows():
    from fib_tf_amd import _lib
    try:
        return _lib.tensor_variants()
    except Exception:                                                    # (collection without a built library: the CPU suite says so)
        return []


ROWS = _tensor_rows()
_ANCHOR = {}
NAME_OF = {(FENTON, 0): 'fenton', (BR, 0): 'br-direct', (BR, 1): 'br-cheby', (COURT, 0): 'court', (COURT, 3): 'court', (COURT, 2): 'court-all',
           (COURT_US, 2): 'court-us'}


def play_row(name, H, W, fast, env, monkeypatch):
    clear_env(monkeypatch, **env)
    st = handle(name, H, W, fast, hole_field(H, W), spd_field(H, W, 17))
    try:
        tile, K = st.plan_tile(), st.launch_plan()[0]
        l0 = st.launch_stats()['launches']
        out = run_ticks(st, name, 3)
        return out, tile, K, st.launch_stats()['launches'] - l0
    finally:
        st.close()


@pytest.mark.parametrize('grid', [(70, 75), (5, 4)], ids=lambda g: '%dx%d' % g)
@pytest.mark.parametrize('i', range(len(ROWS)), ids=lambda i: '%d-%d-%s-K%d-%dx%d-%d' % tuple(ROWS[i][k] for k in ('model', 'mode', 'fast', 'K', 'TX', 'TY', 'NT')))
def test_every_row(i, grid, monkeypatch):
    r = ROWS[i]
    H, W = grid
    name, fast = NAME_OF[(r['model'], r['mode'])], bool(r['fast'])
    key = (name, fast, grid)
    if key not in _ANCHOR:                                               # the K = 1 row, 'slow' a launch of its own
        _ANCHOR[key] = play_row(name, H, W, fast, {'FIBHIP_VARIANT': '1,64,4,256', 'FIBHIP_NO_LAZY': '1'}, monkeypatch)
    want, tile1, K1, launches1 = _ANCHOR[key]
    assert tile1 == (64, 4, -256) and K1 == 1
    fused = r['model'] == COURT and r['mode'] == 3                        # MODE_FASTSLOW: the tick and 'slow' behind it as one launch
    env = {'FIBHIP_VARIANT': '%d,%d,%d,%d' % (r['K'], r['TX'], r['TY'], r['NT'])}
    if r['model'] == COURT and not fused:
        env['FIBHIP_NO_LAZY'] = '1'
    got, tile, K, launches = play_row(name, H, W, fast, env, monkeypatch)
    assert tile == (r['TX'], r['TY'], -r['NT']) and K == r['K'], 'the forced row is not the plan: %r %r' % (tile, K)
    if fused and (H - 1) % r['TY'] and (W - 1) % r['TX']:                 # (plan.inc: a border cell's inward neighbour in its own tile)
        assert launches == launches1 - 1, 'tick + slow did not run as one launch'
    assert np.isfinite(want).all()
    for v in range(want.shape[0]):
        assert same(got[v], want[v]), 'array %d: %d cells differ from the K = 1 row' % (v, int((got[v] != want[v]).sum()))


def test_every_listed_row_is_covered():
    assert len(ROWS) == 24 and {(r['model'], r['mode']) for r in ROWS} == set(NAME_OF)


# ---- 7. the sub-step uses that operator ---------------------------------------------------------------------------------------------
def test_substep_taken_apart(monkeypatch):
    clear_env(monkeypatch)
    H, W = 70, 75
    phi, D = hole_field(H, W), spd_field(H, W, 23)
    diff = 1.2
    a, b = handle('fenton', H, W, False, phi, spt=1, diff=0.0), handle('fenton', H, W, False, phi, D, spt=1, diff=diff)
    try:
        s0 = b.get_state(-1)
        a.step(1)
        b.step(1)
        T, got = a.get_state(-1), b.get_state(-1)
    finally:
        a.close()
        b.close()
    U0 = np.pad(s0[0][1:-1, 1:-1], 1, mode='edge')                        # enforce_boundary
    lap = tensor_ref.laplace32(U0, *D, phi)
    want = lap * np.float32(diff * 0.1) + T[0]                            # RN(RN(lap * ddt) + T), T = RN(RN(dU dt) + U0)
    assert want.dtype == np.float32 and same(got[0], want), '%d cells differ' % int((got[0] != want).sum())
    assert np.abs(lap).max() > 0.1 and not same(got[0], T[0])
    for v in (1, 2, 3):
        assert same(got[v], T[v])


# ---- 8. plane waves along and across the fibres -------------------------------------------------------------------------------------
def _crossing(prev, now, k, up):
    return None if not (prev < up <= now) else (k - 1 + float(up - prev) / float(now - prev))


def cpu_wave(H, W, edge, probes, dt, diff, D, max_ticks=200):
    """activation times (in ticks, interpolated inside the tick as the recorder does) at the probes, on the CPU"""
    s = np.stack([np.zeros((H, W)), np.ones((H, W)), np.ones((H, W)), np.zeros((H, W))]).astype(np.float32)
    s[0][edge] = 1.0
    prev, t = [s[0][p] for p in probes], [None] * len(probes)
    for k in range(1, max_ticks + 1):
        for _ in range(10):
            s = tensor_ref.fenton_substep(s, dt, diff, *D)
        for j, p in enumerate(probes):
            if t[j] is None:
                t[j] = _crossing(prev[j], s[0][p], k, np.float32(0.5))
            prev[j] = s[0][p]
        if all(x is not None for x in t):
            return t
    raise AssertionError('the wave did not reach the probes')


_SPEED = {}


@pytest.mark.parametrize('along', [True, False], ids=['along', 'across'])
def test_plane_wave_speed(along, monkeypatch):
    from fib_tf_amd.fenton import Fenton4v
    clear_env(monkeypatch)
    H, W = (16, 200) if along else (200, 16)
    probes = [(8, 50), (8, 150)] if along else [(50, 8), (150, 8)]
    edge = (slice(None), slice(0, 5)) if along else (slice(0, 5), slice(None))
    m = Fenton4v({'width': W, 'height': H, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 100, 'fast_math': False})
    m.set_fibres(0.0, 2.0)                                                # along the columns, everywhere
    m.define(s1=False)
    t_ref = cpu_wave(H, W, edge, probes, 0.1, 1.5, m.tensor)
    m.add_pace_op('s1', 'left' if along else 'top', 1.0)
    with m.record_activation() as rec:
        m.fire_op('s1')
        m._stepper.step(int(t_ref[1]) + 3)
        first = rec.maps()['first_up']
    t = [float(first[p]) for p in probes]                                 # ms; one tick is 1 ms
    assert np.isfinite(t).all(), t
    cv, cv_ref = 100.0 / (t[1] - t[0]), 100.0 / (t_ref[1] - t_ref[0])
    _SPEED[along] = cv
    print('%s the fibres: %.4f cells per ms on the device, %.4f on the CPU' % ('along' if along else 'across', cv, cv_ref))
    if len(_SPEED) == 2:
        print('speed along / across = %.4f beside sqrt(2) = %.4f' % (_SPEED[True] / _SPEED[False], 2 ** 0.5))
    assert abs(cv / cv_ref - 1.0) <= 2.0 / (t_ref[1] - t_ref[0])          # one tick either way at each probe


# ---- 9. beside the rest ----------------------------------------------------------------------------------------------------------------
def _recorded_run():
    from fib_tf_amd.fenton import Fenton4v
    from fib_tf_amd.stimulus import Stimulus
    m = Fenton4v({'width': 64, 'height': 64, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 40, 'fast_math': False})
    m.set_fibres(np.pi / 4, 2.0)                                          # the diagonal towards growing rows and columns
    m.define(s1=False)
    out = {}
    with m.record_activation() as act, m.record_beats(every=2) as beats, m.record_tips(every=5) as tips, m.record_frames(every=10) as fr, \
            m.record_stats([('U', 'mean'), ('U', 'max'), ('V', 'min')], every=3) as stats, \
            m.program_stimuli([Stimulus((30, 34, 30, 34), 1.0, at_tick=0), Stimulus((30, 34, 30, 34), 1.0, at_tick=30)]) as prog:
        for _ in m.run():
            pass
        out['first_up'] = act.maps()['first_up']
        for k, v in act.velocity('first_up').items():
            out['act_' + k] = v
        for k, v in beats.velocity().items():
            out['beat_' + k] = np.asarray(v)
        out['tips'] = np.asarray(tips.counts())
        out['frames'] = np.asarray(fr.frames())
        out['stats'] = np.asarray(stats.raw())
        out['applied'] = np.asarray(prog.applied())
    out['U'] = m.image()
    return out


def test_recorders_beside_a_tensor(monkeypatch):
    clear_env(monkeypatch)
    a, b = _recorded_run(), _recorded_run()
    assert set(a) == set(b)
    for k in a:
        assert same(a[k], b[k]), k
    assert int(a['applied']) == 2 and a['frames'].shape[0] == 4 and a['stats'].shape[0] == 13 and np.isfinite(a['U']).all()
    # consistency, not accuracy: the wave of the point stimulus arrives sooner along the fibres than across them, and on the long
    # axis of its ellipse the fitted gradient of activation time points along the fibre, to within the fit's own residual
    t = a['first_up']
    assert np.isfinite(t[48, 48]) and t[48, 48] < t[48, 16] and t[16, 16] < t[16, 48]
    gy, gx, rms = (float(a['act_' + k][48, 48]) for k in ('gy', 'gx', 'rms'))
    fibre = np.array([np.sin(np.pi / 4), np.cos(np.pi / 4)])              # (row, column) components
    g = np.array([gy, gx])
    across = g - (g @ fibre) * fibre
    print('gradient (%.5f, %.5f) ms per cell, across the fibre %.2e, rms %.2e' % (gy, gx, float(np.hypot(*across)), rms))
    assert g @ fibre > 0 and np.hypot(*across) <= rms


# ---- 10. refusals through the C ABI ------------------------------------------------------------------------------------------------------
def _refused(st, twin, call, words):
    """`call` is refused in `words`; the handle then still steps, and still equals its twin"""
    from fib_tf_amd import _lib
    with pytest.raises(_lib.FibhipError, match=words):
        call()
    st.step(1)
    twin.step(1)
    assert same(st.get_state(-1), twin.get_state(-1))


def test_refusals_on_a_tensor_handle(monkeypatch):
    clear_env(monkeypatch)
    H, W = 20, 24
    phi, D = hole_field(H, W), spd_field(H, W, 31)
    st, twin = handle('fenton', H, W, False, phi, D), handle('fenton', H, W, False, phi, D)
    try:
        tables = np.ones((1, H, W), np.float32)
        words = 'not on a handle with a diffusion tensor'
        _refused(st, twin, lambda: st.leads_begin([(5, 5, 0)], tables), 'leads_begin: ' + words)
        _refused(st, twin, lambda: st.pmap_begin(np.ones((3, 3), np.float32)), 'pmap_begin: ' + words)
        patch = np.full((2, 2), 0.5, np.float32)
        _refused(st, twin, lambda: st.lesion_begin([(0, (4, 6, 4, 6), patch)]), 'lesion_begin: ' + words)
        _refused(st, twin, lambda: st.lesion_apply((4, 6, 4, 6), patch), 'lesion_apply: ' + words)
        # planes the library does not take: the tensor that stands stays
        one, zero = np.ones((H, W), np.float32), np.zeros((H, W), np.float32)
        nan = one.copy()
        nan[3, 3] = np.nan
        _refused(st, twin, lambda: st.set_tensor(one, one, one), 'not positive definite everywhere')
        _refused(st, twin, lambda: st.set_tensor(nan, one, zero), 'not finite everywhere')
        _refused(st, twin, lambda: st.set_tensor(one, np.float32(1.01) * one, zero), 'largest eigenvalue is above 1')
        # ... and not while a lead recorder is attached to a handle that has no tensor yet
        st.set_tensor(None)
        twin.set_tensor(None)
        st.leads_begin([(5, 5, 0)], tables)
        twin.leads_begin([(5, 5, 0)], tables)
        _refused(st, twin, lambda: st.set_tensor(*D), 'not while a lead recorder')
    finally:
        st.close()
        twin.close()


def test_set_tensor_refused_by_handle_kind(monkeypatch):
    from fib_tf_amd import _lib
    from traced_cases import MODELS, make_model
    clear_env(monkeypatch)

    def pair(make):
        return make(), make()

    def check(st, twin, state, words):
        try:
            st.set_state(-1, state)
            twin.set_state(-1, state)
            D = spd_field(st.height, st.width, 5)
            _refused(st, twin, lambda: st.set_tensor(*D), words)
        finally:
            st.close()
            twin.close()

    st, twin = pair(lambda: _lib.Stepper(FENTON, 20, 24, 0.1, 1.2, flags=_lib.ZEROPAD))
    check(st, twin, fenton_state(20, 24)[0], 'set_tensor: not on a model with the zero-padded Laplacian')
    st, twin = pair(lambda: _lib.Stepper(FENTON, 40, 24, 0.1, 1.2, global_height=80, row_offset=20, ghost_top=10, ghost_bottom=10))
    check(st, twin, fenton_state(40, 24)[0], 'set_tensor: not on a row block')
    name = next(iter(MODELS))
    models = []
    for _ in range(2):
        m = make_model(name, 32, 32)
        m.define()
        m._ensure_compiled()
        models.append(m)
    a, b = (m._stepper for m in models)
    D = spd_field(32, 32, 5)
    _refused(a, b, lambda: a.set_tensor(*D), 'set_tensor: not on a traced model')
