"""-m gpu: every model's step with a real diffusion tensor against something outside the kernels (DESIGN.md 25 "What the tests
hold").  The reference has no tensors; the independent side is tests/tensor_ref.py (the operator from its definition) and the
oracle's reaction terms, joined by the oracle's tensor switch (oracle.tensor; tests/test_tensor_oracle_cpu.py holds that join).
Cases, bounds and comparisons: tests/tensor_cases.py — the bounds are the stock handles' own, or derived there.

  (a) one tick on the K = 1 row against the oracle, every model and mode, both policies (test_every_row carries the K = 1 row to
      the other 23 kernels);  (b) one sub-step taken apart;  (c) 20 ticks on oblique, heterogeneous fibres;  (d) plans no forced
  row reaches;  (e) the handle's life: a tensor replaced, a state kept and resumed;  (f) set_fibres / config['fibre_angle'] on the
  models other than Fenton;  (g) a stimulus program and a frame recorder beside a tensor."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tensor_cases as tcs  # noqa: E402
import timestep_cases as tc  # noqa: E402
from tensor_cases import ALL_CASES, ANCHOR_ENV, CASES, GRIDS, handle, hole_field, run_ticks, same, spd_field  # noqa: E402
from test_gpu_variant_table import Worst, clear_env, fuses_slow  # noqa: E402

pytestmark = pytest.mark.gpu

POLICIES = ['exact', 'fast']


def bits(got, want, what):
    assert np.isfinite(want).all(), what
    for v in range(want.shape[0]):
        assert same(got[v], want[v]), '%s: array %d: %d cells differ' % (what, v, int((got[v] != want[v]).sum()))


# ---- (a) one tick against the oracle with the tensor ------------------------------------------------------------------------------
@pytest.mark.parametrize('hole', [False, True], ids=['plain', 'hole'])
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('name', list(ALL_CASES))
def test_tick_against_the_oracle(gpu_lib, orc, monkeypatch, name, policy, hole):
    """on the K = 1 row under FIBHIP_NO_LAZY, as test_every_row's anchor runs: a tick and the 'slow' behind it are two launches
    on every grid here.  The launch that carries both (70 x 75 can have it, 9 x 129 cannot) never runs in this test: it is
    compared bit for bit with this row by test_default_plan below and by test_gpu_tensor.test_every_row."""
    fast = policy == 'fast'
    worst = Worst()
    for H, W in GRIDS:
        got, launches = tcs.device_tick(name, H, W, fast, hole, monkeypatch)
        if launches is not None:
            assert launches == 2, 'FIBHIP_NO_LAZY: a tick and its \'slow\' are two launches'
        tcs.compare_tick(orc, worst, name, fast, H, W, hole, got)
    bad = worst.check()
    assert not bad, '\n'.join(bad)


# ---- (b) one sub-step taken apart -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('name', list(ALL_CASES))
def test_substep_taken_apart_every_model(gpu_lib, monkeypatch, name, policy):
    """twin handles of one sub-step per tick: the tensor and diff on one, no tensor and diff = 0 on the other (T).  The stock twin
    of the fast policy stays on the plain kernels (FIBHIP_COURT_AGG=0), which a tensor handle always runs."""
    fast = policy == 'fast'
    clear_env(monkeypatch, **({'FIBHIP_COURT_AGG': '0'} if fast else {}))
    H, W = 70, 75
    phi, D = hole_field(H, W), spd_field(H, W, 23)
    a, b = handle(name, H, W, fast, phi, spt=1, diff=0.0), handle(name, H, W, fast, phi, D, spt=1)
    try:
        s0 = b.get_state(-1)
        a.step(1)
        b.step(1)
        T, got = a.get_state(-1), b.get_state(-1)
    finally:
        a.close()
        b.close()
    assert np.isfinite(got).all() and not same(got[0], T[0])
    others, figs = tcs.substep_figures(name, fast, s0, T, got, D, phi)
    for f in figs:
        print('%s: %.4g (bound %.3g)' % f)
    assert not others, 'arrays %s differ from the twin without diffusion' % others
    tc.check(figs)


# ---- (c) trajectories on oblique, heterogeneous fibres ----------------------------------------------------------------------------
_TRAJ = {}


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('name', tcs.TRAJ_CASES)
def test_trajectory_on_oblique_fibres(gpu_lib, orc, monkeypatch, name, policy):
    clear_env(monkeypatch)
    if name not in _TRAJ:
        _TRAJ[name] = tcs.oracle_traj(orc, name)
    ref = _TRAJ[name]
    snaps = tcs.device_traj(name, policy == 'fast')
    figs = tcs.traj_figures(orc, name, policy == 'fast', snaps, ref)
    what, err, bound = max(figs, key=lambda f: f[1] / f[2])
    print('%s %s: worst figure %s, %.3e of %.3e (%.3f)' % (name, policy, what, err, bound, err / bound))
    tc.check(figs)


# ---- (d) plans that no forced row reaches -----------------------------------------------------------------------------------------
def anchored(name, H, W, fast, phi, D, monkeypatch, play, **kw):
    """(the play on the K = 1 row, launches it took)"""
    clear_env(monkeypatch, **ANCHOR_ENV)
    st = handle(name, H, W, fast, phi, D, **kw)
    try:
        assert st.plan_tile() == (64, 4, -256) and st.launch_plan()[0] == 1
        l0 = st.launch_stats()['launches']
        return play(st), st.launch_stats()['launches'] - l0
    finally:
        st.close()


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('name,grid', [(n, GRIDS[0]) for n in CASES] + [('court', GRIDS[1])], ids=lambda x: x if isinstance(x, str) else '%dx%d' % x)
def test_default_plan(gpu_lib, monkeypatch, name, grid, policy):
    fast = policy == 'fast'
    H, W = grid
    phi, D = hole_field(H, W), spd_field(H, W, 29)
    want, launches1 = anchored(name, H, W, fast, phi, D, monkeypatch, lambda st: run_ticks(st, name, 3))
    clear_env(monkeypatch)
    st = handle(name, H, W, fast, phi, D)
    try:
        l0 = st.launch_stats()['launches']
        got = run_ticks(st, name, 3)
        launches = st.launch_stats()['launches'] - l0
        print('%s %s %dx%d: plan K = %d in tile %s, %d launches (K = 1 row: %d)' % (name, policy, H, W, st.launch_plan()[0], st.plan_tile(), launches, launches1))
        assert st.ticks_per_launch() == 1
    finally:
        st.close()
    if name == 'court':                                                   # the tick and 'slow' as one launch where the rule allows it
        assert launches == launches1 - (1 if fuses_slow(H, W) else 0)
        assert fuses_slow(H, W) == (grid == GRIDS[0])
    bits(got, want, name)


@pytest.mark.parametrize('policy', POLICIES)
def test_large_grid_plan(gpu_lib, monkeypatch, policy):
    """740 x 740: more than 512 tiles of 32 x 32, so a tick is two launches of five sub-steps (csrc/plan.inc)"""
    fast = policy == 'fast'
    H = W = 740
    phi, D = hole_field(H, W), spd_field(H, W, 31)
    want, launches1 = anchored('fenton', H, W, fast, phi, D, monkeypatch, lambda st: run_ticks(st, 'fenton', 1))
    assert launches1 == 10
    clear_env(monkeypatch)
    st = handle('fenton', H, W, fast, phi, D)
    try:
        assert st.launch_plan()[0] == 5 and st.plan_tile() == (32, 32, -512), (st.launch_plan(), st.plan_tile())
        l0 = st.launch_stats()['launches']
        got = run_ticks(st, 'fenton', 1)
        assert st.launch_stats()['launches'] - l0 == 2
    finally:
        st.close()
    bits(got, want, 'fenton 740 x 740')


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('name,spt', [('fenton', 3), ('fenton', 7), ('fenton', 12), ('br-direct', 3), ('br-direct', 7), ('br-cheby', 3), ('br-cheby', 7)])
def test_ticks_of_other_lengths(gpu_lib, monkeypatch, name, spt, policy):
    """a tick of `spt` sub-steps (Fenton: K descends through the second table, 12 = 10 + 2, 7 = 5 + 2, 3 = 2 + 1) equals `spt`
    ticks of one sub-step"""
    fast = policy == 'fast'
    H, W = GRIDS[0]
    phi, D = hole_field(H, W), spd_field(H, W, 37)
    clear_env(monkeypatch)
    a, b = handle(name, H, W, fast, phi, D, spt=1), handle(name, H, W, fast, phi, D, spt=spt)
    try:
        if name == 'fenton':
            assert b.launch_plan()[0] == {3: 2, 7: 5, 12: 10}[spt], b.launch_plan()
        assert a.launch_plan()[0] == 1
        a.step(spt)
        b.step(1)
        want, got = a.get_state(-1), b.get_state(-1)
    finally:
        a.close()
        b.close()
    bits(got, want, '%s, %d sub-steps per tick' % (name, spt))


# ---- (e) the handle's life --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('between', [False, True], ids=['straight', 'set_state-between'])
@pytest.mark.parametrize('name,policy', [('fenton', 'exact'), ('court', 'fast')])
def test_tensor_replaced(gpu_lib, monkeypatch, name, policy, between):
    clear_env(monkeypatch)
    fast = policy == 'fast'
    H, W = GRIDS[0]
    phi, D1, D2 = hole_field(H, W), spd_field(H, W, 43), spd_field(H, W, 47)
    a, b, c = handle(name, H, W, fast, phi, D1), None, handle(name, H, W, fast, phi, D1)
    try:
        mid = run_ticks(a, name, 3)
        a.set_tensor(*D2)
        if between:
            mid = ALL_CASES[name][2](H + 1, W)[0][:, :H]                  # another seeded state
            a.set_state(-1, mid)
        b = handle(name, H, W, fast, phi, D2, state=mid)
        got, want = run_ticks(a, name, 3), run_ticks(b, name, 3)
        run_ticks(c, name, 3)
        if between:
            c.set_state(-1, mid)
        assert not same(run_ticks(c, name, 3)[0], want[0])                # (the second tensor is seen)
    finally:
        for st in (a, b, c):
            if st is not None:
                st.close()
    bits(got, want, name)


@pytest.mark.parametrize('name', list(CASES))
def test_keep_state_and_resume_on_tensor_handles(gpu_lib, monkeypatch, name):
    """test_keep_state_and_resume_every_model's statement: a run cut at a tick boundary and resumed on a new handle from the state
    read back ends in the bits of the uncut run"""
    clear_env(monkeypatch)
    H, W = GRIDS[0]
    phi, D = hole_field(H, W), spd_field(H, W, 53)
    a, b, c = handle(name, H, W, False, phi, D), handle(name, H, W, False, phi, D), None
    try:
        run_ticks(a, name, 3)
        want = run_ticks(a, name, 4)
        kept = run_ticks(b, name, 3)
        c = handle(name, H, W, False, phi, D, state=kept)
        assert same(c.get_state(-1), kept)
        got = run_ticks(c, name, 4)
    finally:
        for st in (a, b, c):
            if st is not None:
                st.close()
    bits(got, want, name)


# ---- (f) the Python path for the other models -------------------------------------------------------------------------------------
def _model(kind, H, W, **kw):
    from fib_tf_amd import court_ultra
    from fib_tf_amd.br import BeelerReuter
    from fib_tf_amd.court import Courtemanche
    cls = {'br': BeelerReuter, 'court': Courtemanche, 'court_ultra': court_ultra.Courtemanche}[kind]
    return cls(tc.device_cfg(H, W, 0.1, 0.809, 'exact', **kw))


@pytest.mark.parametrize('how', ['set_fibres', 'config'])
@pytest.mark.parametrize('kind', ['br', 'court', 'court_ultra'])
def test_python_fibres_other_models(gpu_lib, monkeypatch, kind, how):
    from fib_tf_amd import _lib
    clear_env(monkeypatch)
    H, W = 40, 52
    if how == 'config':
        angle, ratio, scale = 0.6, 2.5, 1.0
        m = _model(kind, H, W, fibre_angle=angle, anisotropy=ratio)
    else:
        rng = np.random.default_rng(61)
        angle, ratio, scale = rng.uniform(-np.pi, np.pi, (H, W)), rng.uniform(1.0, 3.0, (H, W)), rng.uniform(0.3, 1.0, (H, W))
        m = _model(kind, H, W)
        m.set_fibres(angle, ratio, scale)
    m.add_hole_to_phase_field(20, 18, 5)
    m.define()
    D = tcs.tensor_ref.fibre_planes(angle, ratio, scale, shape=(H, W))
    for p, q in zip(m.tensor, D):
        assert same(p, q)
    st = m._stepper
    s0 = st.get_state(-1)
    ref = _lib.Stepper(m.MODEL_ID, H, W, 0.1, 0.809, flags=m._flags())
    try:
        ref.set_phase(m.phase)
        ref.set_tensor(*D)
        ref.set_state(-1, s0)
        for h in (st, ref):
            h.step(5)
            if kind == 'court':
                h.step_slow()
                h.step(1)
        got, want = st.get_state(-1), ref.get_state(-1)
        plain = _lib.Stepper(m.MODEL_ID, H, W, 0.1, 0.809, flags=m._flags())
        try:
            plain.set_phase(m.phase)
            plain.set_state(-1, s0)
            plain.step(5)
            assert not same(plain.get_state(0), got[0])                   # (the fibres are seen)
        finally:
            plain.close()
    finally:
        ref.close()
    assert not same(got[0], s0[0])
    bits(got, want, kind)


# ---- (g) beside the rest ----------------------------------------------------------------------------------------------------------
def _fenton_model():
    from fib_tf_amd.fenton import Fenton4v
    H, W = 48, 56
    m = Fenton4v(tc.device_cfg(H, W, 0.1, 1.2, 'exact', duration=40))
    m.add_hole_to_phase_field(30, 24, 6)
    m.set_tensor(*spd_field(H, W, 67))
    m.define()
    return m


def test_stimulus_program_beside_a_tensor(gpu_lib, monkeypatch):
    from fib_tf_amd.stimulus import Stimulus
    clear_env(monkeypatch)
    a, b = _fenton_model(), _fenton_model()
    site = (8, 20, 30, 44)
    with a.program_stimuli([Stimulus(site, 1.0, at_tick=2, mode='max', floor='min_v')]) as prog:
        a._stepper.step(6)
        assert int(prog.applied()) == 1
        got = a._stepper.get_state(-1)
    b._stepper.step(3)
    before = b._stepper.get_state(0).copy()
    b._stepper.pace(*site, 1.0, float(b.min_v))
    assert not same(b._stepper.get_state(0), before)
    b._stepper.step(3)
    bits(got, b._stepper.get_state(-1), 'stimulus program')


def test_frame_recorder_beside_a_tensor(gpu_lib, monkeypatch):
    clear_env(monkeypatch)
    a, b = _fenton_model(), _fenton_model()
    with a.record_frames(every=1, fmt='float32') as rec:
        a._stepper.step(5)
        frames = np.asarray(rec.frames())
    assert frames.shape == (5, 48, 56) and frames.dtype == np.float32
    for t in range(5):
        b._stepper.step(1)
        assert same(frames[t], b._stepper.get_state(0) * np.asarray(b.phase, np.float32)), 'frame %d' % t
    assert not same(frames[4], frames[0])
