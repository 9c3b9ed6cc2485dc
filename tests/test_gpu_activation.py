"""-m gpu: the activation recorder (include/fibhip.h fibhip_observe_*, fib_tf_amd/activation.py) on the device.

The maps it records are checked bit for bit against the NumPy restatement (tests/activation_ref.py) applied to the
watched array read back after every tick of a plain run of the same protocol; the state it observes must stay bitwise
what an unobserved handle computes; and the physics it measures must agree with probe timing and the reference's
conduction-velocity table.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from activation_ref import ActivationRef, bit_equal  # noqa: E402

pytestmark = pytest.mark.gpu


def fenton(n=96, fast=True, hole=True, duration=400):
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': n, 'width': n, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': duration,
                  'fast_math': fast})
    if hole:
        m.add_hole_to_phase_field(n // 2, n // 2, 9)
    m.define()
    m.add_pace_op('s2', 'luq', 1.0)
    return m


def br(skip, duration=350):
    from fib_tf_amd.br import BeelerReuter
    m = BeelerReuter({'height': 64, 'width': 64, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 0.809, 'duration': duration,
                      'cheby': True, 'skip': skip})
    m.add_hole_to_phase_field(30, 36, 7)
    m.define()
    m.add_pace_op('s2', 'luq', 10.0)
    return m


def court(duration=40):
    from fib_tf_amd.court import Courtemanche
    m = Courtemanche({'height': 64, 'width': 64, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 0.809, 'duration': duration})
    m.add_hole_to_phase_field(30, 36, 7)
    m.define()
    m.add_pace_op('s2', 'luq', 20.0)
    return m


def traced(duration=40):
    from traced_cases import make_model
    m = make_model('ap', 64, 64, (30, 30, 7))
    m.duration = duration
    m.define()
    m.add_pace_op('s2', 'luq', 1.0)
    m._ensure_compiled()                                      # (a traced model builds its handle on first use)
    return m


def protocol(m, i, s2, slow):
    if slow and i % 10 == 0:
        m.fire_op('slow')
    if i == s2:
        m.fire_op('s2')


def plain_maps(make, s2, slow=False, up=None, down=None):
    """the restatement fed with pot().eval() after every tick of an unobserved run (read before that tick's stimuli)"""
    from fib_tf_amd.activation import default_thresholds
    m = make()
    d_up, d_down = default_thresholds(float(m.min_v), float(m.max_v))
    ref = ActivationRef(m.pot().eval(), d_up if up is None else up, d_down if down is None else down, m.dt,
                        m._stepper.steps_per_tick)
    for i in m.run():
        ref.step(m.pot().eval())
        protocol(m, i, s2, slow)
    state = m._stepper.get_state(-1)
    m._stepper.close()
    return ref, state


def observed_maps(make, s2, slow=False, **kw):
    """the same protocol under IonicModel.run() with a recorder attached after define()"""
    m = make()
    st = m._stepper
    with m.record_activation(**kw) as rec:
        ticks0 = st.launch_stats()['ticks']
        for i in m.run():
            protocol(m, i, s2, slow)
        maps, k = rec.maps(), rec.ticks()
        stats = st.launch_stats()
    state = st.get_state(-1)
    assert k == m.samples and stats['ticks'] - ticks0 == m.samples, (k, stats, m.samples)
    assert stats['mt_launches'] == 0                       # every tick a plain launch while attached
    st.close()
    return maps, state


def assert_maps_equal(maps, ref, need_beats=1):
    want = ref.maps()
    for name in want:
        assert bit_equal(maps[name], want[name]), '%s: %d cells differ' % (
            name, int((maps[name].view(np.int32) != want[name].view(np.int32)).sum()))
    assert want['count'].max() >= need_beats                  # (the protocol produced events at all)


@pytest.mark.parametrize('fast', [True, False], ids=['fast', 'exact'])
def test_fenton_maps_bit_exact(gpu_lib, fast):
    """Fenton 4v 96^2, obstacle, S1 + an S2 in the upper-left quadrant at 190 ms that breaks into a second front"""
    make = lambda: fenton(96, fast)                           # noqa: E731
    ref, state_plain = plain_maps(make, 190)
    maps, state_obs = observed_maps(make, 190)
    assert_maps_equal(maps, ref, need_beats=2)
    assert np.isfinite(ref.apd).sum() > 1000
    assert bit_equal(state_obs, state_plain)


@pytest.mark.parametrize('skip', [False, True], ids=['every-step', 'skip'])
def test_br_maps_bit_exact(gpu_lib, skip):
    make = lambda: br(skip)                                   # noqa: E731
    ref, state_plain = plain_maps(make, 500)
    maps, state_obs = observed_maps(make, 500)
    assert_maps_equal(maps, ref)
    assert np.isfinite(ref.apd).sum() > 100
    assert bit_equal(state_obs, state_plain)


def test_court_maps_bit_exact_with_slow_ticks(gpu_lib):
    make = lambda: court()                                    # noqa: E731
    ref, state_plain = plain_maps(make, 150, slow=True)
    maps, state_obs = observed_maps(make, 150, slow=True)
    assert_maps_equal(maps, ref)
    assert bit_equal(state_obs, state_plain)


def test_traced_model_maps_bit_exact(gpu_lib):
    make = lambda: traced()                                   # noqa: E731
    ref, state_plain = plain_maps(make, 200)
    maps, state_obs = observed_maps(make, 200)
    assert_maps_equal(maps, ref)
    assert bit_equal(state_obs, state_plain)


def test_custom_thresholds_and_other_var(gpu_lib):
    """var 1 of Fenton (V, a gate that recovers towards 1 at rest and falls on excitation), started just below `up`, with
    explicit thresholds: rested cells cross up, the S1 wave then takes them down — still the restatement"""
    from fib_tf_amd.fenton import Fenton4v
    cfg = {'height': 64, 'width': 80, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.0, 'duration': 120}
    a, b = Fenton4v(dict(cfg)), Fenton4v(dict(cfg))
    for m in (a, b):
        m.define()
        m._stepper.set_state(1, np.full((64, 80), 0.899, np.float32))
    ref = ActivationRef(a._State['V'].eval(), 0.9, 0.5, 0.1, 10)
    rec = b.record_activation(up=0.9, down=0.5, var=1)
    for _ in a.run():
        ref.step(a._State['V'].eval())
    for _ in b.run():
        pass
    assert_maps_equal(rec.maps(), ref)
    assert np.isfinite(ref.apd).any()
    rec.close()


def test_state_untouched_and_reattach(gpu_lib):
    """N observed ticks leave every state array bitwise where an unobserved handle has it; attach / detach in mid-run and
    attach again: the maps and the tick count start from scratch"""
    a, b = fenton(128, hole=True), fenton(128, hole=True)
    sa, sb = a._stepper, b._stepper
    rec = b.record_activation()
    assert sb.ticks_per_launch() == 1
    for st in (sa, sb):
        st.step(4)
    assert rec.ticks() == 4
    st_b = sb.get_state(-1)
    assert bit_equal(st_b, sa.get_state(-1))
    rec.close()
    for st in (sa, sb):
        st.step(2)
        st.pace(1, 64, 1, 64, 1.0, 0.0)
        st.step(3)
    rec = b.record_activation()
    assert rec.ticks() == 0
    m0 = rec.maps()
    assert (m0['count'] == 0).all() and np.isnan(m0['first_up']).all() and np.isnan(m0['apd']).all()
    ref = ActivationRef(sb.get_state(0), rec.up, rec.down, 0.1, 10)
    for t in range(60):
        for st in (sa, sb):
            st.step(1)
        ref.step(sa.get_state(0))
        if t == 30:                                           # (a stimulus between two ticks belongs to the next one)
            for st in (sa, sb):
                st.pace(64, 127, 64, 127, 1.0, 0.0)
    assert rec.ticks() == 60
    assert_maps_equal(rec.maps(), ref)
    b.record_activation()                                     # attaching again while attached clears as well
    assert b._stepper.observe_ticks() == 0
    assert (b._stepper.observe_get('count') == 0).all()
    assert bit_equal(sb.get_state(-1), sa.get_state(-1))
    sb.observe_end()


def test_trace_shows_the_observer(gpu_lib):
    m = fenton(96, hole=False)
    st = m._stepper
    st.step(2)
    st.sync()
    n0 = st.launch_stats()['launches']
    plain = st.trace_tick()
    with m.record_activation():
        ev = st.trace_tick()
        assert [e['name'] for e in ev] == [e['name'] for e in plain] + ['observe_kernel']
        assert ev[-1]['ts'] >= ev[-2]['ts']
    stats = st.launch_stats()
    assert stats['ticks'] == 4 and stats['launches'] - n0 == len(plain) + len(ev)


def _probe_crossings(st, row, cols, thresh, i, prev, out):
    """upstroke times of probed pixels in ms-since-start ticks, interpolated as tests/test_gpu_physics.py::velocity does"""
    cur = [float(st.probe(0, row, c)) for c in cols]
    if prev is not None:
        for j, (pa, a) in enumerate(zip(prev, cur)):
            if pa < thresh <= a:
                out[j].append(i + (thresh - pa) / (a - pa))    # observed tick i starts at i ticks after attach
    return cur


def test_strip_last_up_agrees_with_probe_timing(gpu_lib):
    """the 48 x 420 strip of test_gpu_physics.py: last_up at the two probe columns vs probe timing, within 1e-3 ms"""
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': 48, 'width': 420, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.0, 'duration': 700})
    m.define()
    st = m._stepper
    rec = m.record_activation()
    cols, ups, prev = (150, 300), ([], []), None
    for i in m.run():
        prev = _probe_crossings(st, 24, cols, 0.5, i, prev, ups)
    last = rec.maps()['last_up']
    tick = m.dt_per_step * m.dt
    for j, c in enumerate(cols):
        assert len(ups[j]) == 1
        assert abs(float(last[24, c]) - ups[j][0] * tick) < 1e-3, (c, float(last[24, c]), ups[j][0] * tick)
    rec.close()


@pytest.mark.parametrize('policy', ['fast', 'exact'])
def test_map_conduction_velocity_ratios(gpu_lib, policy):
    """CV(d) / CV(1.0) from the last_up map along the strip's middle row vs the reference's diff_conduction_velcoty.dat"""
    from test_gpu_physics import FENTON_CV
    from fib_tf_amd.activation import conduction_velocity
    from fib_tf_amd.fenton import Fenton4v
    cv = {}
    for d in (0.5, 1.0, 1.5):
        m = Fenton4v({'height': 48, 'width': 420, 'dt': 0.1, 'dt_per_plot': 10, 'diff': d, 'duration': 900,
                      'fast_math': policy == 'fast'})
        m.define()
        with m.record_activation() as rec:
            for _ in m.run():
                pass
            t = rec.maps()['last_up']
        assert np.isfinite(t[24, 150:300]).all()
        cv[d] = conduction_velocity(t, 24, 150, 300)
    for d in cv:
        got, want = cv[d] / cv[1.0], FENTON_CV[d] / FENTON_CV[1.0]
        assert abs(got / want - 1.0) < 0.05, 'diff %.2f: CV ratio %.3f vs reference %.3f' % (d, got, want)


def test_anchored_reentry_cycle_length(gpu_lib):
    """the 512^2 anchored-reentry protocol of test_gpu_physics.py: last_up - prev_up at the watched pixel [20, W//2]
    is the last cycle length probing measures there"""
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': 512, 'width': 512, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 1000})
    m.add_hole_to_phase_field(256, 256, 512 // 17)
    m.define()
    m.add_pace_op('s2', 'luq', 1.0)
    s2 = m.millisecond_to_step(210)
    st = m._stepper
    rec = m.record_activation()
    ups, prev = ([],), None
    for i in m.run():
        if i == s2:
            m.fire_op('s2')
        prev = _probe_crossings(st, 20, (256,), 0.5, i, prev, ups)
    ups = ups[0]
    maps = rec.maps()
    assert len(ups) >= 4 and maps['count'][20, 256] == len(ups)
    tick = m.dt_per_step * m.dt
    cl_probe = (ups[-1] - ups[-2]) * tick
    cl_map = float(maps['last_up'][20, 256] - maps['prev_up'][20, 256])
    assert abs(cl_map - cl_probe) < 1e-3, (cl_map, cl_probe)
    assert 60 < cl_map < 400
    rec.close()


def test_argument_checks(gpu_lib):
    from fib_tf_amd import _lib
    L = _lib.lib()
    st = _lib.Stepper(_lib.FENTON4V, 32, 40, 0.1, 1.0)
    st.set_state(-1, np.zeros((4, 32, 40), np.float32))
    h = st._h
    nan = float('nan')
    for var, up, down in ((-1, 0.5, 0.1), (4, 0.5, 0.1), (0, 0.1, 0.5), (0, nan, 0.1), (0, 0.5, nan)):
        assert L.fibhip_observe_begin(h, var, up, down) == -1, (var, up, down)             # FIBHIP_EINVAL
    buf = np.empty((32, 40), np.float32)
    k = C.c_longlong()
    assert L.fibhip_observe_get(h, 0, buf.ctypes.data_as(C.c_void_p)) == -1        # nothing attached
    assert L.fibhip_observe_ticks(h, C.byref(k)) == -1
    assert L.fibhip_observe_begin(h, 0, 0.5, 0.5) == 0                                  # down == up is allowed
    assert L.fibhip_observe_get(h, 5, buf.ctypes.data_as(C.c_void_p)) == -1
    assert L.fibhip_observe_get(h, -1, buf.ctypes.data_as(C.c_void_p)) == -1
    assert L.fibhip_observe_get(h, 0, None) == -1
    assert L.fibhip_observe_ticks(h, None) == -1
    assert L.fibhip_observe_ticks(h, C.byref(k)) == 0 and k.value == 0
    assert L.fibhip_observe_end(h) == 0 and L.fibhip_observe_end(h) == 0
    assert L.fibhip_observe_begin(None, 0, 0.5, 0.1) == -1
    st.close()
    # a handle with ghost rows (a row block) is refused
    blk = _lib.Stepper(_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    assert L.fibhip_observe_begin(blk._h, 0, 0.5, 0.1) == -1
    assert b'row block' in L.fibhip_last_error()
    blk.close()
