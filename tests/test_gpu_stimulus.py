"""-m gpu: the stimulus program (include/fibhip.h fibhip_stim_*, fib_tf_amd/stimulus.py) on the device.

No tolerance anywhere in this file: a program must leave the BYTES that the same stimuli leave when the caller's loop body
fires them (fire_op / Stepper.pace), and the bytes of the NumPy restatement (tests/stim_ref.py) applied to the state read back
at the event ticks.  The grids are the smallest that reach each path of stim_kernel: 37 x 53 and 20 x 130 (scalar: odd widths,
rows not 16-byte aligned), 64 x 64 (16-byte loads and stores, a box that starts at an odd column) and 96 x 100 (several tiles,
multi-tick launches)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stim_ref as ref  # noqa: E402
from test_gpu_frames import PACE_V, PLAN_ENV, VARIANT_96x100, wave  # noqa: E402
from test_gpu_stats import model_columns, planes as stat_planes  # noqa: E402
from test_gpu_tips import MAKERS, court, fenton  # noqa: E402

pytestmark = pytest.mark.gpu

S1_TICKS, S2_TICK, CHECKPOINTS = (0, 7, 14, 21, 28), 23, (24, 40, 60)


def set_env(monkeypatch, env):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def protocol(v):
    from fib_tf_amd.stimulus import Stimulus, s1_train
    return s1_train('left', v, period=7, n=5) + [Stimulus('luq', v, at_tick=S2_TICK)]


def play(kind, programmed, ticks=60, checkpoints=CHECKPOINTS):
    """60 single-tick calls with the S1 train and the S2 — from a program, or fired from the loop body — and, for Courtemanche,
    the driver's 'slow' every 10th tick.  -> ([state bytes at the checkpoints], applied, launch stats since attach, before's)"""
    m = MAKERS[kind](96, 100)
    st = m._stepper
    wave(m, kind)
    v = PACE_V[kind]
    s0 = st.launch_stats()
    prog = m.program_stimuli(protocol(v)) if programmed else None
    left, luq = m.pace_rect('left'), m.pace_rect('luq')
    states = []
    for i in range(ticks):
        st.step(1)
        if not programmed:
            if i in S1_TICKS:
                st.pace(*left, v, float(m.min_v))
            if i == S2_TICK:
                m.fire_op('s2')
        if kind == 'court' and i % 10 == 0:
            m.fire_op('slow')
        if i + 1 in checkpoints:
            states.append(st.get_state(-1).tobytes())
    applied = prog.applied() if programmed else None
    s1 = st.launch_stats()
    if prog:
        assert prog.events(ticks) == [(t, 0) for t in S1_TICKS if t < S2_TICK] + [(S2_TICK, 1)] + [(t, 0) for t in S1_TICKS if t > S2_TICK]
        prog.close()
    return states, applied, {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}, st


@pytest.mark.parametrize('mt', ['mt', 'mt0'])
@pytest.mark.parametrize('kind,plan', [('fenton', 'forced'), ('fenton', 'default'), ('br', 'default'), ('court', 'default'),
                                       ('traced', 'default')])
def test_program_equals_fire_op(gpu_lib, monkeypatch, kind, plan, mt):
    """The forced 12-tile shape (VARIANT_96x100) is a Fenton shape — ten sub-steps per launch — so it is run for Fenton only, beside
    the plan Fenton chooses itself; Beeler-Reuter, Courtemanche (on aggregates: no multi-tick launches) and the traced model run
    under the plan they choose.  Every case runs with multi-tick launches allowed and with FIBHIP_MT=0."""
    env = {'FIBHIP_VARIANT': VARIANT_96x100} if plan == 'forced' else {}
    if mt == 'mt0':
        env['FIBHIP_MT'] = '0'
    set_env(monkeypatch, env)
    want, _, _, st_a = play(kind, False)
    st_a.close()
    got, applied, stats, st_b = play(kind, True)
    st_b.close()
    assert len(want) == 3 and len(set(want)) == 3                 # (the state moves)
    for tick, g, w in zip(CHECKPOINTS, got, want):
        assert g == w, '%s %s %s: the state after %d ticks differs from the run that fires from the loop body' % (kind, plan, mt, tick)
    assert applied == 6 and stats['ticks'] == 60, (applied, stats)
    if mt == 'mt0':
        assert stats['mt_ticks'] == 0
    elif kind == 'fenton' and plan == 'forced':
        assert stats['mt_ticks'] > 0                              # (the program ran beside multi-tick launches)


def test_program_changes_the_state(gpu_lib, monkeypatch):
    """(the yardstick of the test above is not blind: without the stimuli the state is another one)"""
    set_env(monkeypatch, {'FIBHIP_VARIANT': VARIANT_96x100})
    with_stim, _, _, a = play('fenton', True, checkpoints=(60,))
    m = fenton(96, 100)
    wave(m, 'fenton')
    m._stepper.step(60)
    assert m._stepper.get_state(-1).tobytes() != with_stim[0]
    a.close()
    m._stepper.close()


def random_program(H, W, rng, nvar, var2):
    """a MAX plane and an ADD plane due after the same ticks on array 0 (their order matters), the same pair on array `var2`,
    an entry held for three ticks, a rectangle whose outside is untouched and a rectangle that floors the whole array.  One
    plane's box starts at an odd column and ends at an odd column."""
    def boxed(fill, r0, r1, c0, c1, lo, hi):
        p = np.full((H, W), fill, np.float32)
        p[r0:r1, c0:c1] = rng.uniform(lo, hi, (r1 - r0, c1 - c0)).astype(np.float32)
        return p
    planes = [boxed(-np.inf, 3, H - 5, 5, W - 7, 0.0, 1.0), boxed(0.0, 1, H // 2, 2, W // 2 + 1, -0.25, 0.25),
              rng.uniform(0.0, 1.0, (H, W)).astype(np.float32), boxed(0.0, H // 2, H, 0, 4, -0.1, 0.1)]
    planes[2][rng.uniform(size=(H, W)) < 0.5] = -np.inf           # a scattered site: half the cells untouched
    assert planes[0][3, 5] != -np.inf and ref.box(planes[0], 'max')[2] % 2 == 1
    entries = [
        {'var': 0, 'mode': 'max', 'shape': 'plane', 'plane': 0, 'first': 1, 'period': 4, 'count': 3, 'hold': 1},
        {'var': 0, 'mode': 'add', 'shape': 'plane', 'plane': 1, 'first': 1, 'period': 4, 'count': 3, 'hold': 1},
        {'var': var2, 'mode': 'add', 'shape': 'plane', 'plane': 3, 'first': 1, 'period': 4, 'count': 0, 'hold': 1},
        {'var': var2, 'mode': 'max', 'shape': 'plane', 'plane': 2, 'first': 1, 'period': 0, 'count': 1, 'hold': 1},
        {'var': 0, 'mode': 'add', 'shape': 'plane', 'plane': 3, 'first': 4, 'period': 5, 'count': 2, 'hold': 3},
        {'var': nvar - 1, 'mode': 'max', 'shape': 'rect', 'r0': 2, 'r1': 9, 'c0': 3, 'c1': W - 1, 'v': 0.75, 'floor': -np.inf, 'first': 2,
         'period': 0, 'count': 1, 'hold': 2},
        {'var': 1, 'mode': 'add', 'shape': 'rect', 'r0': H - 3, 'r1': H, 'c0': 0, 'c1': W, 'v': 0.5, 'floor': -0.125, 'first': 6, 'period': 0,
         'count': 1, 'hold': 1}]
    return entries, planes


def crowd(H, W, nvar):
    """ten entries due after the same tick: more than one launch takes (eight), arrays mixed, both modes"""
    return [{'var': i % nvar, 'mode': 'add' if i % 3 else 'max', 'shape': 'rect', 'r0': i, 'r1': H - i, 'c0': 2 * i + 1, 'c1': W - i,
             'v': 0.05 * (i + 1), 'floor': 0.0 if i % 3 else (-np.inf if i % 2 else 0.1), 'first': 2, 'period': 3, 'count': 2, 'hold': 1}
            for i in range(10)]


def against_the_restatement(gpu_lib, make, entries, planes, ticks, what):
    """the program on one handle, fibhip_step in calls of several ticks; a twin stepped tick by tick with
    get_state -> stim_ref -> set_state at the event ticks"""
    a, b = make(), make()
    a.stim_begin(entries, planes)
    events = ref.events(entries, ticks)
    left = ticks
    for n in (1, 3, 2, 5, ticks):
        n = min(n, left)
        a.step(n)
        left -= n
    for k in range(ticks):
        b.step(1)
        if any(t == k for t, _ in events):
            b.set_state(-1, ref.apply_tick(b.get_state(-1), entries, planes, k))
    assert a.stim_count() == len(events), what
    got, want = a.get_state(-1), b.get_state(-1)
    for v in range(got.shape[0]):
        assert got[v].tobytes() == want[v].tobytes(), '%s: array %d differs in %d cells' % (what, v, int((got[v] != want[v]).sum()))
    assert np.isfinite(got).all()
    a.stim_end()
    a.close()
    b.close()
    return len(events)


@pytest.mark.parametrize('shape,layout', [((37, 53), 'planar'), ((20, 130), 'planar'), ((64, 64), 'planar'), ((37, 53), 'interleaved'),
                                          ((64, 64), 'interleaved')], ids=lambda a: a if isinstance(a, str) else '%dx%d' % a)
def test_planes_and_add_equal_the_restatement(gpu_lib, shape, layout):
    """(the row-interleaved slab — pitch = nvar * W, the layout of a row block, here without ghost rows — takes the scalar path
    at every width)"""
    H, W = shape
    rng = np.random.default_rng(1000 * H + W)
    init = rng.uniform(0, 1, (4, H, W)).astype(np.float32)
    flags = gpu_lib.FAST | (gpu_lib.ROW_INTERLEAVED if layout == 'interleaved' else 0)

    def make():
        st = gpu_lib.Stepper(gpu_lib.FENTON4V, H, W, 0.1, 1.3, flags=flags)
        st.set_state(-1, init)
        return st
    entries, planes = random_program(H, W, rng, 4, 2)
    n = against_the_restatement(gpu_lib, make, entries, planes, 14, '%dx%d %s' % (H, W, layout))
    n2 = against_the_restatement(gpu_lib, make, crowd(H, W, 4), None, 7, '%dx%d %s, ten entries at once' % (H, W, layout))
    assert n == 3 + 3 + 4 + 1 + 6 + 2 + 1 and n2 == 20


def test_the_restatement_on_a_model_with_multi_tick_launches(gpu_lib, monkeypatch):
    """96 x 100 at the forced shape: the same comparison where the ticks between two events are one launch"""
    set_env(monkeypatch, {'FIBHIP_VARIANT': VARIANT_96x100})
    rng = np.random.default_rng(96100)
    init = None

    def make():
        nonlocal init
        m = fenton(96, 100)
        wave(m, 'fenton')
        st = m._stepper
        if init is None:
            init = st.get_state(-1).copy()
        st.set_state(-1, init)
        return st
    entries, planes = random_program(96, 100, rng, 4, 2)
    against_the_restatement(gpu_lib, make, entries, planes, 14, '96x100')


def launch_rule(gpu_lib, monkeypatch, entries):
    set_env(monkeypatch, {'FIBHIP_VARIANT': VARIANT_96x100})
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    st.stim_begin(entries)
    s0 = st.launch_stats()
    for _ in range(64):
        st.step(1)
    st.sync()
    s1 = st.launch_stats()
    n = st.stim_count()
    st.close()
    return {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}, n


def test_sixty_four_single_tick_calls_are_eight_launches(gpu_lib, monkeypatch):
    """an event every 8 ticks: between two events the ticks are ONE launch, and the stimulus is one more"""
    rect = dict(var=0, mode='max', shape='rect', r0=0, r1=96, c0=0, c1=5, v=1.0, floor=0.0)
    one = [dict(rect, first=7, period=8, count=0)]
    stats, n = launch_rule(gpu_lib, monkeypatch, one)
    assert stats['mt_launches'] == 8 and stats['mt_ticks'] == 64 and stats['launches'] == 16 and n == 8, (stats, n)
    two = one + [dict(rect, mode='add', var=2, r0=10, r1=20, c0=3, c1=50, v=0.01, first=7, period=8, count=8)]
    stats, n = launch_rule(gpu_lib, monkeypatch, two)
    assert stats['mt_launches'] == 8 and stats['mt_ticks'] == 64 and stats['launches'] == 16 and n == 16, (stats, n)


def test_a_handle_without_a_program_launches_as_before(gpu_lib, monkeypatch):
    """... and one whose program has no event left goes back to the launches it had"""
    set_env(monkeypatch, {'FIBHIP_VARIANT': VARIANT_96x100})
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    st.stim_begin([dict(var=0, mode='max', shape='rect', r0=0, r1=96, c0=0, c1=5, v=1.0, floor=0.0, first=2)])
    s0 = st.launch_stats()
    st.step(3)
    st.step(40)
    st.sync()
    s1 = st.launch_stats()
    assert s1['mt_ticks'] - s0['mt_ticks'] == 43 and s1['mt_launches'] - s0['mt_launches'] == 3, (s0, s1)       # 3, then 32 + 8
    assert s1['launches'] - s0['launches'] == 4 and st.stim_count() == 1
    st.close()


def test_plain_ticks_on_a_handle_that_has_made_multi_tick_launches(gpu_lib, monkeypatch):
    """The stimulus behind a PLAIN tick looks at no give-up word: the device's word belongs to the multi-tick launches (an autotune
    candidate that gave up leaves it raised until the next such launch zeroes it), and a plain tick stands behind a confirmed
    stream anyway.  Here the handle has made multi-tick launches (its epoch words exist) and then steps one call per tick with
    an event after EVERY tick — first = 0, period 1 — and a stimulus held for three ticks: every tick is a plain launch, every
    stimulus is written.  Then the same after a recovered give-up, where every tick is plain for good.  The yardstick fires from
    the loop body; an ADD entry on array 2 beside it shows a dropped event (MAX of the same value twice would hide one)."""
    def run(programmed, env):
        set_env(monkeypatch, dict({'FIBHIP_VARIANT': VARIANT_96x100}, **env))
        m = fenton(96, 100)
        st = m._stepper
        wave(m, 'fenton')
        st.step(12)                                               # multi-tick launches: the epoch words are allocated
        st.sync()
        made = st.launch_stats()['mt_launches']
        plane = np.zeros((96, 100), np.float32)
        plane[20:40, 11:50] = 0.004
        entries = [dict(var=0, mode='max', shape='rect', r0=0, r1=96, c0=0, c1=5, v=1.0, floor=0.0, first=0, period=1, count=6),
                   dict(var=0, mode='max', shape='rect', r0=1, r1=48, c0=1, c1=50, v=0.9, floor=0.0, first=7, period=0, count=1, hold=3),
                   dict(var=2, mode='add', shape='plane', plane=0, first=0, period=1, count=10)]
        if programmed:
            st.stim_begin(entries, [plane])
        s0 = st.launch_stats()
        with warnings.catch_warnings(record=True):
            warnings.simplefilter('always')
            for i in range(10):
                st.step(1)
                if not programmed:
                    x = st.get_state(-1)
                    st.set_state(-1, ref.apply_tick(x, entries, [plane], i))
            state = st.get_state(-1).tobytes()
        s1 = st.launch_stats()
        n = st.stim_count() if programmed else None
        fb = st.fallbacks()
        st.close()
        return state, n, {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}, made, fb
    want, _, _, made, _ = run(False, {})
    got, n, stats, made, fb = run(True, {})
    assert made > 0 and fb == (0, 0)
    assert stats['ticks'] == 10 and stats['mt_ticks'] == 0 and stats['launches'] == 20, stats     # ten plain ticks, ten stimuli
    assert n == 6 + 3 + 10 and got == want
    got, n, stats, made, fb = run(True, {'FIBHIP_MT_FAKE_GIVEUP': '1'})     # the first multi-tick launch of the handle gives up
    assert fb[0] == 1 and stats['mt_ticks'] == 0 and n == 19 and got == want, (fb, stats, n)


def beside(gpu_lib, programmed, activation):
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    weight, mask = stat_planes(96, 100, 4)
    rec = m.record_activation() if activation else None
    st.stats_begin(model_columns('fenton', m), weight, mask, 5, 12)
    left = m.pace_rect('left')
    prog = None
    if programmed:
        from fib_tf_amd.stimulus import Stimulus
        prog = m.program_stimuli([Stimulus('left', 1.0, at_tick=6, period=7, count=0)])
    for i in range(60):
        st.step(1)
        if not programmed and i % 7 == 6:
            st.pace(*left, 1.0, float(m.min_v))
    table = st.stats_read().tobytes()
    maps = [rec.maps()[k].tobytes() for k in gpu_lib.OBS_MAPS] if activation else None
    state = st.get_state(-1).tobytes()
    if prog:
        assert prog.applied() == 8
    st.close()
    return table, maps, state


@pytest.mark.parametrize('activation', [False, True], ids=['stats', 'stats+activation'])
def test_beside_the_recorders(gpu_lib, monkeypatch, activation):
    """a sample every 5 ticks, a stimulus every 7: the samples come first (tick 34 has both), the table and the maps are those
    of the run that polls nothing but fires from its loop body"""
    set_env(monkeypatch, {'FIBHIP_VARIANT': VARIANT_96x100})
    want = beside(gpu_lib, False, activation)
    got = beside(gpu_lib, True, activation)
    assert got[0] == want[0] and got[2] == want[2]
    if activation:
        assert got[1] == want[1] and len(set(got[1])) > 1


def test_court_event_tick_is_not_fused_with_slow(gpu_lib):
    """a stimulus due after the tick 'slow' would ride on: the order is tick, stimulus, slow — whatever array the entry names"""
    from fib_tf_amd.court import Courtemanche
    from fib_tf_amd.stimulus import Stimulus
    slow_var = Courtemanche.tip_signals[1]
    for var, v, mode in ((0, 20.0, 'max'), (slow_var, 0.01, 'add')):
        twin = court(64, 80)
        wave(twin, 'court')
        ts = twin._stepper
        ts.step(5)
        x = ts.get_state(-1)
        s = ref.rect_plane(64, 80, *twin.pace_rect('luq'), v, float(twin.min_v) if mode == 'max' else 0.0)
        ts.set_state(var, ref.apply(x[var], s, mode))
        twin.fire_op('slow')
        ts.step(3)
        want = ts.get_state(-1).tobytes()
        fused = court(64, 80)                                     # (the yardstick is not blind: slow before the stimulus differs)
        wave(fused, 'court')
        fused._stepper.step(5)
        fused.fire_op('slow')
        y = fused._stepper.get_state(-1)
        fused._stepper.set_state(var, ref.apply(y[var], s, mode))
        fused._stepper.step(3)
        assert fused._stepper.get_state(-1).tobytes() != want
        m = court(64, 80)
        wave(m, 'court')
        st = m._stepper
        with m.program_stimuli([Stimulus('luq', v, at_tick=4, mode=mode, var=var)]) as prog:
            st.step(5)                                            # (the last tick may be held back for 'slow' to ride on)
            m.fire_op('slow')
            st.step(3)
            assert st.get_state(-1).tobytes() == want, (var, mode)
            assert prog.applied() == 1
        for s_ in (ts, fused._stepper, st):
            s_.close()


def test_refusals(gpu_lib):
    import ctypes as C
    m = fenton(64, 80)
    st = m._stepper
    L, h = st._L, st._h
    good = dict(var=0, mode=0, shape=0, r0=0, r1=8, c0=0, c1=8, v=1.0, floor=0.0, plane=0, first=0, period=0, count=1, hold=1)
    plane = np.zeros((64, 80), np.float32)

    def begin(n=None, nplanes=0, planes=None, handle=h, entries=None, **kw):
        entries = [dict(good, **kw)] if entries is None else entries
        arr = (gpu_lib.StimEntry * max(len(entries), 1))()
        for i, e in enumerate(entries):
            for k, val in e.items():
                setattr(arr[i], k, val)
        pp = planes.ctypes.data_as(C.POINTER(C.c_float)) if planes is not None else None
        return L.fibhip_stim_begin(handle, len(entries) if n is None else n, arr, nplanes, pp)
    bad = [(dict(var=-1), b'entry 0: bad var -1'), (dict(var=4), b'entry 0: bad var 4'), (dict(mode=2), b'entry 0: unknown mode 2'),
           (dict(mode=-1), b'entry 0: unknown mode -1'), (dict(shape=2), b'entry 0: unknown shape 2'),
           (dict(shape=1, plane=0), b'entry 0: plane 0 of 0'), (dict(shape=1, plane=1, nplanes=1, planes=plane), b'entry 0: plane 1 of 1'),
           (dict(shape=1, plane=-1, nplanes=1, planes=plane), b'entry 0: plane -1 of 1'),
           (dict(r0=8, r1=8), b'entry 0: rows [8, 8) x columns [0, 8) is empty or outside the 64 x 80 grid'),
           (dict(r1=65), b'is empty or outside'), (dict(c0=-1), b'is empty or outside'), (dict(c1=81), b'is empty or outside'),
           (dict(c0=9, c1=3), b'is empty or outside'), (dict(hold=3, period=2, count=2), b'entry 0: hold 3 > period 2'),
           (dict(hold=0), b'entry 0: hold must be >= 1'), (dict(first=-1), b'entry 0: first must be >= 0'),
           (dict(count=2), b'entry 0: period 0 means one event'), (dict(count=0), b'entry 0: period 0 means one event'),
           (dict(period=-1), b'must be >= 0'), (dict(period=3, count=-1), b'must be >= 0'),
           (dict(v=float('inf')), b'entry 0: v must be finite'), (dict(v=float('nan')), b'entry 0: v must be finite'),
           (dict(floor=float('nan')), b'entry 0: floor must be finite'), (dict(floor=float('inf')), b'entry 0: floor must be finite'),
           (dict(mode=1, floor=float('-inf')), b'entry 0: floor must be finite'),
           (dict(n=0), b'1 .. 64 entries'), (dict(n=65), b'1 .. 64 entries'), (dict(nplanes=9, planes=plane), b'0 .. 8 planes'),
           (dict(nplanes=-1), b'0 .. 8 planes'), (dict(nplanes=1), b'0 .. 8 planes')]
    for kw, msg in bad:
        assert begin(**kw) == -1, kw
        err = L.fibhip_last_error()
        assert b'stim_begin' in err and msg in err, (kw, err)
    assert begin(entries=[good, good, dict(good, var=7)]) == -1 and b'entry 2: bad var 7' in L.fibhip_last_error()
    k = C.c_longlong()
    assert L.fibhip_stim_count(h, C.byref(k)) != 0 and b'no program' in L.fibhip_last_error()           # nothing was attached
    assert L.fibhip_stim_end(h) == 0                                                                    # (nothing attached: nothing)
    assert begin(floor=float('-inf')) == 0                                                              # MAX: the outside untouched
    assert begin() == -1 and b'attached already' in L.fibhip_last_error()                               # a second program
    assert L.fibhip_stim_count(h, C.byref(k)) == 0 and k.value == 0 and L.fibhip_stim_count(h, None) != 0
    assert L.fibhip_stim_end(h) == 0 and L.fibhip_stim_end(h) == 0
    st.step_edges()
    assert begin() == -1 and b'open tick' in L.fibhip_last_error()
    st.step_interior()
    st.step_commit()
    assert begin(handle=None) != 0 and L.fibhip_stim_begin(h, 1, None, 0, None) != 0
    assert begin(entries=[dict(good, first=i) for i in range(64)]) == 0                                 # 64 entries fit
    st.step(70)
    assert st.stim_count() == 64
    with pytest.raises(ValueError, match='a plane of shape'):
        st.stim_begin([good], [np.zeros((3, 3), np.float32)])
    with pytest.raises(ValueError, match='unknown field'):
        st.stim_begin([dict(good, every=3)])
    st.close()                                                    # destroyed with a program attached
    with pytest.raises(gpu_lib.FibhipError, match='null handle'):
        st.stim_begin([good])                                     # a program on a destroyed handle
    # the recorder object on a closed program
    from fib_tf_amd.stimulus import Stimulus
    m2 = fenton(64, 80)
    prog = m2.program_stimuli([Stimulus('left', 1.0, at_tick=0)])
    with pytest.raises(gpu_lib.FibhipError, match='attached already'):
        m2.program_stimuli([Stimulus('left', 1.0, at_tick=0)])
    prog.close()
    prog.close()
    with pytest.raises(AssertionError, match='closed'):
        prog.applied()
    m2._stepper.close()


def test_row_block_refused(gpu_lib):
    blk = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    arr = (gpu_lib.StimEntry * 1)()
    arr[0].r1 = arr[0].c1 = 4
    arr[0].count = arr[0].hold = 1
    rc = blk._L.fibhip_stim_begin(blk._h, 1, arr, 0, None)
    assert rc == -1 and b'row block' in blk._L.fibhip_last_error()
    blk.close()


def test_timeline_lists_the_stimulus(gpu_lib):
    m = fenton(96, 130)
    st = m._stepper
    st.step(1)
    st.stats_begin(model_columns('fenton', m), None, None, 1, 8)
    st.stim_begin([dict(var=0, mode='max', shape='rect', r0=0, r1=96, c0=0, c1=5, v=1.0, floor=0.0, first=1)])
    names = [e['name'] for e in st.trace_tick()] + ['|'] + [e['name'] for e in st.trace_tick()]
    assert names.count('stim_kernel') == 1, names
    assert names.index('|') < max(i for i, n in enumerate(names) if n == 'stats_combine_kernel') < names.index('stim_kernel'), names
    st.close()


def test_example_and_bench_tool_run(gpu_lib, tmp_path, capsys):
    """examples/run_s1s2.py and tools/bench_stimulus.py end to end at a tiny size (in this process: what is checked is that they
    run and that what they print rests on what happened)"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    ex = load('examples/run_s1s2.py', 'run_s1s2_under_test')
    entries, table, counts = ex.main(['--size', '96', '--s1-ms', '20', '--n-s1', '2', '--s2-ms', '12', '--ms', '60', '--every', '5'])
    out = capsys.readouterr().out
    assert '3 stimuli applied (2 S1 + the S2 after tick 32)' in out and 'excited fraction' in out, out
    assert [(e['first'], e['period'], e['count']) for e in entries] == [(0, 20, 2), (32, 0, 1)]
    assert entries[0]['shape'] == 'rect' and entries[0]['floor'] == 0.0 and entries[1]['shape'] == 'plane'
    assert len(table) == 12 and len(counts) == 12 and 0 < table['U_frac_above'].max() <= 1
    bench = load('tools/bench_stimulus.py', 'bench_stimulus_under_test')
    path = tmp_path / 'bench.txt'
    lines = bench.main(['--ticks', '40', '--configs', 'fenton96', '--periods', '10', '--out', str(path)])
    import json
    assert [json.loads(x) for x in path.read_text().splitlines()] == lines and len(lines) == 1
    r = lines[0]
    assert r['config'] == 'fenton96' and r['cells'] == 96 * 96 and set(r['program_us']) == set(r['fire_op_us']) == {'10'}
    for k in ('none_us', 'none_again_us', 'stim_kernel_us', 'pace_kernel_us'):
        assert r[k] > 0, (k, r)
