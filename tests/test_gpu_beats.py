"""-m gpu: the beat recorder (include/fibhip.h fibhip_beats_*, fib_tf_amd/beats.py) on the device.

The ring planes, the counts, the live peak and the summary maps must EQUAL the NumPy restatement (tests/beat_ref.py) fed with the
state read back after every sample tick: every bit of every number, NaN for NaN (beat_ref.same) — no tolerance anywhere in this
file.  The grids are the smallest that reach each path: 37 x 53 (one pixel per thread, odd everything), 64 x 64 (16-byte loads
and stores), 20 x 130 (rows not 16-byte aligned), 96 x 100 (several tiles, multi-tick launches) and one 512 x 512 case (many
workgroups)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beat_ref as ref  # noqa: E402
import spectrum_ref  # noqa: E402
from test_gpu_tips import MAKERS, fenton, court  # noqa: E402

from fib_tf_amd import beats as bt  # noqa: E402

pytestmark = pytest.mark.gpu

PLAN_ENV = ('FIBHIP_MT', 'FIBHIP_AHEAD', 'FIBHIP_MT_FAKE_GIVEUP', 'FIBHIP_VARIANT', 'FIBHIP_MT_MAX', 'FIBHIP_MT_IDS', 'FIBHIP_AUTOTUNE')
VARIANT_96x100 = '10,44,25,-3'                              # the forced small shape of tests/test_gpu_recovery.py: 12 tiles
PACE_V = {'fenton': 1.0, 'br': 10.0, 'court': 20.0, 'traced': 1.0}
# pacing period, run length and stride in ticks, so that at least three whole beats pass every cell.  A Fenton beat lasts about
# 200 ticks, one of the Aliev-Panfilov model about 30.  The Courtemanche sheet at these settings stays above -60 mV for some 2100
# ticks and is back at rest after 3000 (found on the CPU oracle); its default levels — 50 % and 10 % of [-100, 50] mV — put
# `down` below the resting potential, so it is watched at -40 / -60 mV
PERIOD = {'fenton': 300, 'br': 800, 'court': 3000, 'traced': 100}
TICKS = {'fenton': 1000, 'br': 2700, 'court': 11500, 'traced': 340}
STRIDE = {'fenton': 5, 'br': 5, 'court': 25, 'traced': 5}
LEVELS = {'court': (np.float32(-40.0), np.float32(-60.0))}
MAPS = ('t_up', 't_down', 'peak', 'count', 'pk')
SUMMARY = ('nused', 'apd_mean', 'cl_mean', 'apd_alt')


def same_all(got, want, names, what):
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert ref.same(g, w), '%s %s: %d of %d values differ' % (what, name, int((~((g == w) | ((g != g) & (w != w)))).sum()), g.size)


def levels(m):
    return bt.default_levels(float(m.min_v), float(m.max_v))


def paced(kind, H, W):
    """a model of `kind` from rest under a stimulus program: the left columns every PERIOD ticks, from tick 0 on"""
    m = MAKERS[kind](H, W)
    st = m._stepper
    st.stim_begin([dict(var=0, mode='max', shape='rect', r0=0, r1=H, c0=0, c1=5, v=PACE_V[kind], floor=-np.inf, first=0,
                        period=PERIOD[kind], count=0)])
    return m, st


def advance(m, st, kind, done, n):
    """n ticks in as few calls as the model allows: Courtemanche's 'slow' rides on every tenth tick"""
    if kind != 'court':
        st.step(n)
        return
    while n > 0:
        if done % 10 == 0:
            m.fire_op('slow')
        k = min(n, 10 - done % 10)
        st.step(k)
        done, n = done + k, n - k


def follow(m, st, kind, ticks, every, depth, region=None, block=(1, 1), reduce='mean', weight=None, lasts=None, what='', lv=None,
           pace=None):
    """attaches the recorder and the restatement to the state as it stands, runs `ticks` ticks, feeds the restatement from the
    state read back after every sample tick, and compares everything that can be read; returns the restatement.  `pace` =
    (first, period, rectangle, v): fibhip_pace from the host right after those ticks — sample ticks, so the state read back is
    the state the sample saw, and the stimulus belongs to the next sample"""
    up, down = lv or levels(m)
    st.beats_begin(0, region, block, reduce, weight, every, up, down, depth)
    r = ref.Beats(ref.pixel(st.get_state(0), region, block, reduce, weight), up, down, depth, every, m.dt, m.dt_per_step)
    assert st.beats_shape() == r.xp.shape + (depth,)
    for s in range(ticks // every):
        advance(m, st, kind, s * every, every)
        r.sample(ref.pixel(st.get_state(0), region, block, reduce, weight))
        t = (s + 1) * every
        if pace and t >= pace[0] and (t - pace[0]) % pace[1] == 0:
            st.pace(*pace[2], pace[3], float(m.min_v))
    assert st.beats_count() == ticks // every, what
    same_all(st.beats_read(), r.read(), MAPS, what)
    for last in lasts or sorted({1, min(4, depth), depth}):
        same_all(st.beats_summary(last), r.summary(last), SUMMARY, '%s summary(%d)' % (what, last))
    st.beats_end()
    return r


@pytest.mark.parametrize('shape', [(37, 53), (64, 64), (20, 130)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_ring_equals_the_restatement(gpu_lib, kind, shape):
    H, W = shape
    m, st = paced(kind, H, W)
    # (64 x 64: a ring shorter than the beat count)
    depth = 2 if shape == (64, 64) else 8
    r = follow(m, st, kind, TICKS[kind], STRIDE[kind], depth, what='%s %dx%d' % (kind, H, W), lv=LEVELS.get(kind))
    done = r.t_down == r.t_down
    print('%s %dx%d: %d .. %d upstrokes per cell, %d finished beats in the ring' % (kind, H, W, r.n.min(), r.n.max(), int(done.sum())))
    assert r.n.min() >= 3 and done.any(axis=0).all()          # at least three beats passed every cell, and the ring holds a finished one
    if depth == 2:
        assert r.n.min() > depth
    st.close()


def wave(m, kind='fenton'):
    """an S1 wave on its way (define()'s own columns) and a second one from a stimulus in the middle, a few ticks old"""
    st = m._stepper
    H, W = m.height, m.width
    st.pace(H // 3, H // 3 + 7, W // 3, W // 3 + 9, PACE_V[kind], float(m.min_v))
    st.step(4)
    st.sync()


def test_multi_tick_launches(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    m = fenton(96, 100)
    wave(m)
    st = m._stepper
    st.stim_begin([dict(var=0, mode='max', shape='rect', r0=0, r1=96, c0=0, c1=5, v=1.0, floor=-np.inf, first=100, period=150, count=0)])
    plane = np.random.default_rng(96).uniform(0.8, 1.0, (96, 100)).astype(np.float32)
    r = follow(m, st, 'fenton', 400, 4, 4, what='96x100 full')
    assert r.n.max() >= 2 and st.launch_stats()['mt_launches'] > 0
    r = follow(m, st, 'fenton', 300, 6, 3, (1, 96, 5, 98), (2, 3), 'mean', plane, what='96x100 block mean')
    assert r.n.max() >= 1
    st.close()


def test_many_workgroups(gpu_lib):
    """512 x 512 under a 4 x 4 mean, a sample every 10 ticks, 400 ticks: the S1 wave and a stimulus in the middle pass"""
    m = fenton(512, 512)
    wave(m)
    r = follow(m, m._stepper, 'fenton', 400, 10, 4, None, (4, 4), 'mean', None, what='512x512')
    assert r.xp.shape == (128, 128) and r.n.max() >= 1 and (r.t_down == r.t_down).any() and len(np.unique(r.t_up)) > 100
    m._stepper.close()


def variants(H, W):
    """(region, block, reduce, weighted): each of region, block, point / mean and weight on and off"""
    return [(None, (1, 1), 'mean', False), ((1, H, 5, W - 2), (2, 3), 'mean', True), ((0, H, 4, W), (4, 4), 'point', True),
            ((0, H, 0, W), (1, 1), 'point', True), ((2, H - 1, 8, W - 4), (1, 1), 'mean', False), (None, (3, 2), 'point', False)]


@pytest.mark.parametrize('every', [1, 3, 10])
def test_strides_and_pixel_variants(gpu_lib, every):
    """Fenton 64 x 64 from the same state for every variant: the S1 wave on its way, a stimulus in the middle, and the left edge
    paced from the host every 120 ticks, right after a sample tick of every stride (the second pace falls into the tail of the
    first beat: some cells follow, some do not)"""
    H, W = 64, 64
    m = fenton(H, W)
    wave(m)
    st = m._stepper
    state0 = st.get_state(-1).copy()
    plane = np.random.default_rng(every).uniform(0.05, 1.0, (H, W)).astype(np.float32)
    events = 0
    for region, block, reduce, weighted in variants(H, W):
        st.set_state(-1, state0)
        r = follow(m, st, 'fenton', 360, every, 3, region, block, reduce, plane if weighted else None,
                   what='every %d region %s block %s %s weight %s' % (every, region, block, reduce, weighted), pace=(60, 120, (0, H, 0, 5), 1.0))
        events += int(r.n.sum())
    assert events > 1000
    st.close()


def test_vector_and_scalar_path(gpu_lib):
    """full resolution on aligned rows, with and without a weight plane: four pixels per thread (the timeline event's K says
    so); a window that starts at an odd column, one whose width is no multiple of four, a block: one pixel per thread; all equal
    the restatement"""
    m = fenton(64, 64)
    wave(m)
    st = m._stepper
    up, down = levels(m)
    plane = np.random.default_rng(7).uniform(0.9, 1.0, (64, 64)).astype(np.float32)
    state0 = st.get_state(-1).copy()                          # (the wave crosses the sheet in some fifteen ticks: every window sees it)
    for region, block, weight, per_thread in ((None, (1, 1), None, 4), ((3, 60, 4, 64), (1, 1), plane, 4), ((0, 64, 1, 61), (1, 1), None, 1),
                                              ((0, 64, 0, 62), (1, 1), plane, 1), (None, (1, 2), None, 1)):
        st.set_state(-1, state0)
        st.beats_begin(0, region, block, 'mean', weight, 1, up, down, 2)
        r = ref.Beats(ref.pixel(st.get_state(0), region, block, 'mean', weight), up, down, 2, 1, m.dt, m.dt_per_step)
        ev = [e for e in st.trace_tick() if e['name'] == 'beat_kernel']
        assert len(ev) == 1 and ev[0]['K'] == per_thread, (region, ev)
        r.sample(ref.pixel(st.get_state(0), region, block, 'mean', weight))
        for _ in range(12):
            st.step(1)
            r.sample(ref.pixel(st.get_state(0), region, block, 'mean', weight))
        same_all(st.beats_read(), r.read(), MAPS, 'window %s block %s' % (region, block))
        assert r.n.sum() > 0
        st.beats_end()
    st.close()


def _plan_run(gpu_lib, monkeypatch, env, record, every=10, ticks=80):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(96, 100)
    st = m._stepper
    wave(m)                                                   # (plan selection happens at the first tick)
    up, down = levels(m)
    out = None
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        if record:
            st.beats_begin(0, None, (1, 1), 'mean', None, every, up, down, 4)
        s0 = st.launch_stats()                                # (behind the attach: beats_begin is a launch of its own)
        st.step(ticks)
        if record:
            assert st.beats_count() == ticks // every
        s1 = st.launch_stats()                                # (before the reads: beats_summary is a launch of its own)
        if record:
            out = st.beats_read() + st.beats_summary(4)
        state = st.get_state(-1)
        fb = st.fallbacks()
    st.close()
    return out, state, fb, {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}


def test_launch_count_and_plan_independence(gpu_lib, monkeypatch):
    out, state, fb, stats = _plan_run(gpu_lib, monkeypatch, {}, True)
    assert fb[0] == 0
    # between two samples the handle runs the fewest launches `every` allows: eight ten-tick launches and eight samples
    assert stats['ticks'] == 80 and stats['mt_ticks'] == 80 and stats['mt_launches'] == 8, stats
    assert stats['launches'] == 8 + 8, stats
    assert out[3].sum() > 1000 and len(np.unique(out[0])) > 100
    for env in ({'FIBHIP_MT': '0'}, {'FIBHIP_AHEAD': '0'}, {'FIBHIP_MT_FAKE_GIVEUP': '2'}):
        out2, st2, fb2, stats2 = _plan_run(gpu_lib, monkeypatch, env, True)
        same_all(out2, out, MAPS + SUMMARY, str(env))
        assert st2.tobytes() == state.tobytes(), env
        assert stats2['ticks'] == 80, (env, stats2)
        if 'FIBHIP_MT_FAKE_GIVEUP' in env:
            assert fb2[0] == 1 and fb2[1] > 0, fb2            # one launch gave up and was recovered
        if 'FIBHIP_MT' in env:
            assert stats2['mt_ticks'] == 0
    _, plain, _, pstats = _plan_run(gpu_lib, monkeypatch, {}, False)
    assert plain.tobytes() == state.tobytes()                 # the recorder changes nothing of the state
    assert pstats['ticks'] == 80 and pstats['mt_ticks'] > 0


def _all(gpu_lib, which, ticks=60):
    """a spectrum every 2 ticks, the activation maps, frames every 5 ticks, beats every 4 and a trigger program (those named in
    `which`; the trigger program always: it changes the state every recorder sees) on one Fenton handle, one call"""
    m = fenton(96, 100)
    st = m._stepper
    wave(m)
    up, down = levels(m)
    # sensed every 4 ticks — the beat recorder's sample ticks: the sample comes before the stimulus the rule fires
    st.trig_begin([dict(site='rect', var=0, level=0.5, need=1, r0=40, r1=56, c0=80, c1=90)],
                  [dict(sensor=0, edge='rise', blank=1, mode='max', shape='rect', var=0, r0=70, r1=80, c0=10, c1=30, v=1.0, floor=-np.inf)],
                  every=4, capacity=ticks // 4)
    if 'sp' in which:
        st.spectrum_begin(0, None, (2, 2), 'mean', None, 2, 10, spectrum_ref.hann(10), spectrum_ref.twiddles(10), [1, 2, 3], 5)
    if 'obs' in which:
        st.observe_begin(0, up, down)
    if 'fr' in which:
        st.frames_begin(0, (0, 96, 0, 100), (2, 2), 'mean', 0.0, 1.0, None, 'uint8', 5, 5, ticks // 5)
    if 'bt' in which:
        st.beats_begin(0, None, (2, 2), 'mean', None, 4, up, down, 4)
    st.step(ticks)
    out = {}
    if 'sp' in which:
        out['sp'] = st.spectrum_read()[0].tobytes()
    if 'obs' in which:
        out['obs'] = [st.observe_get(k).tobytes() for k in ('first_up', 'last_up', 'prev_up', 'apd', 'count')]
    if 'fr' in which:
        out['fr'] = st.frames_read().tobytes()
    if 'bt' in which:
        got = st.beats_read()
        assert got[3].sum() > 100 and st.beats_count() == ticks // 4
        out['bt'] = [g.tobytes() for g in got + st.beats_summary(4)]
    out['trig'] = st.trig_read().tobytes()
    out['state'] = st.get_state(-1).tobytes()
    st.close()
    return out


def test_beside_the_other_recorders_and_a_trigger_program(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    everything = _all(gpu_lib, ('sp', 'obs', 'fr', 'bt'))
    for which in ('sp', 'obs', 'fr', 'bt'):
        alone = _all(gpu_lib, (which,))
        assert alone[which] == everything[which], which       # each records what it records alone
        assert alone['state'] == everything['state'] and alone['trig'] == everything['trig'], which


def test_literal_planes_under_a_slow_courtemanche_array(gpu_lib):
    """the ticks leave an array 'slow' assigns untouched between two 'slow' ops, so set_state puts literal planes — NaN, +-inf,
    exactly `up`, exactly `down` — under the recorder on the device; the array read back after the tick is what was written"""
    from fib_tf_amd.court import Courtemanche
    slow_var = Courtemanche.tip_signals[1]                    # a gate 'slow' assigns
    H, W = 64, 80
    m = court(H, W)
    st = m._stepper
    UP, DOWN = np.float32(0.5), np.float32(0.125)
    nan, inf = np.nan, np.inf
    values = np.array([0.0, 0.125, 0.25, 0.5, 0.75, 1.0, nan, inf, -inf, 0.1, 0.6], np.float32)
    rng = np.random.default_rng(80)
    planes = [rng.choice(values, (H, W)) for _ in range(14)]
    st.set_state(slow_var, planes[0])
    for region, block in ((None, (1, 1)), ((1, H, 3, W), (2, 2))):
        st.beats_begin(slow_var, region, block, 'mean', None, 1, UP, DOWN, 3)
        r = ref.Beats(ref.pixel(planes[0], region, block), UP, DOWN, 3, 1, m.dt, m.dt_per_step)
        for p in planes[1:] + planes[:1]:
            st.set_state(slow_var, p)
            st.step(1)
            assert st.get_state(slow_var).tobytes() == p.tobytes()        # the tick left the array as it was written
            r.sample(ref.pixel(p, region, block))
        same_all(st.beats_read(), r.read(), MAPS, 'literal planes %s' % (block,))
        for last in (1, 2, 3):
            same_all(st.beats_summary(last), r.summary(last), SUMMARY, 'literal planes %s summary(%d)' % (block, last))
        if block == (1, 1):
            assert r.n.max() > 3 and np.isinf(r.peak).any()       # (the ring wrapped somewhere; a beat peaked at +inf)
        st.beats_end()
    st.close()


def test_court_sample_of_a_slow_array_is_taken_before_slow(gpu_lib):
    """a sample of a slow array due at the tick 'slow' would ride on: the two are not fused, the sample holds the array as the
    tick left it"""
    from fib_tf_amd.court import Courtemanche
    slow_var = Courtemanche.tip_signals[1]
    twin = court(64, 80)
    wave(twin, 'court')
    states = []
    for s in range(4):
        twin._stepper.step(5)
        states.append(twin._stepper.get_state(slow_var).copy())
        twin.fire_op('slow')
    assert states[0].tobytes() != twin._stepper.get_state(slow_var).tobytes()
    x0 = None
    twin._stepper.close()
    m = court(64, 80)
    wave(m, 'court')
    st = m._stepper
    x0 = st.get_state(slow_var).copy()
    level = np.float32(np.median(states[-1]))                 # a level the gate crosses somewhere
    st.beats_begin(slow_var, None, (1, 1), 'mean', None, 5, level, level, 2)
    r = ref.Beats(ref.pixel(x0), level, level, 2, 5, m.dt, m.dt_per_step)
    for s in range(4):
        st.step(5)                                            # (the last tick may be held back for 'slow' to ride on)
        m.fire_op('slow')
        r.sample(ref.pixel(states[s]))
    same_all(st.beats_read(), r.read(), MAPS, 'slow array')
    assert (r.xp != x0).any()
    st.close()


def test_refusals(gpu_lib):
    import ctypes as C
    from fib_tf_amd._lib import _ip
    m = fenton(64, 80)
    st = m._stepper
    L, h = st._L, st._h

    def begin(handle=h, var=0, window=(0, 64, 0, 80), by=1, bx=1, reduce=1, every=1, up=0.5, down=0.1, depth=4):
        w = np.ascontiguousarray(window, np.intc)
        return L.fibhip_beats_begin(handle, var, w.ctypes.data_as(_ip), by, bx, reduce, None, every, up, down, depth)
    for kw in (dict(var=-1), dict(var=st.nvar), dict(window=(0, 65, 0, 80)), dict(window=(4, 4, 0, 80)), dict(by=0), dict(bx=17),
               dict(reduce=2), dict(every=0), dict(depth=0), dict(depth=17), dict(down=0.6), dict(up=float('nan'))):
        assert begin(**kw) != 0, kw
        assert b'beats_begin' in L.fibhip_last_error(), kw
    k = C.c_longlong()
    assert L.fibhip_beats_count(h, C.byref(k)) != 0 and b'no recorder' in L.fibhip_last_error()
    assert L.fibhip_beats_read(h, None, None, None, None, None) != 0 and b'no recorder' in L.fibhip_last_error()
    assert begin() == 0
    assert begin() != 0 and b'attached already' in L.fibhip_last_error()         # a second recorder
    assert st.beats_count() == 0                              # the refused calls left the recorder attached
    for last in (0, 5, -1):
        assert L.fibhip_beats_summary(h, last, None, None, None, None) != 0 and b'beats_summary' in L.fibhip_last_error()
    assert L.fibhip_beats_summary(h, 4, None, None, None, None) == 0
    assert begin(down=0.5) != 0 and L.fibhip_beats_end(h) == 0 and begin(down=0.5) == 0       # down == up is allowed
    assert L.fibhip_beats_end(h) == 0 and L.fibhip_beats_end(h) == 0            # end without begin: nothing
    st.step_edges()
    assert begin() != 0 and b'open tick' in L.fibhip_last_error()
    st.step_interior()
    st.step_commit()
    assert begin(handle=None) != 0
    with pytest.raises(ValueError):
        m.record_beats(depth=17)
    with pytest.raises(ValueError):
        m.record_beats(up=0.1, down=0.5)
    with m.record_beats(every=2, depth=3, region=(0, 64, 0, 80), block=(2, 2)) as rec:
        assert rec.shape == (32, 40) and rec.samples() == 0 and (rec.up, rec.down) == bt.default_levels(0.0, 1.0)
        with pytest.raises(ValueError):
            rec.summary(last=4)
    st.close()
    blk = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 80, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    assert begin(handle=blk._h, window=(0, 42, 0, 80)) == -1 and b'row block' in L.fibhip_last_error()
    blk.close()
    inter = gpu_lib.Stepper(gpu_lib.FENTON4V, 64, 80, 0.1, 1.3, flags=gpu_lib.FAST | gpu_lib.ROW_INTERLEAVED)
    assert begin(handle=inter._h) == -1 and b'row-interleaved' in L.fibhip_last_error()
    inter.close()


def test_timeline_lists_the_sample(gpu_lib):
    m = fenton(96, 130)
    st = m._stepper
    st.step(1)
    up, down = levels(m)
    st.beats_begin(0, None, (1, 1), 'mean', None, 2, up, down, 2)
    names = [e['name'] for _ in range(4) for e in st.trace_tick()]
    assert names.count('beat_kernel') == 2, names
    assert st.beats_count() == 2
    st.close()


def test_python_layer_on_a_paced_sheet(gpu_lib):
    """the CPU suite's physics check on the device, through the public interface: Fenton 64 x 64 from rest, columns 0-5 paced
    every 300 ticks by a stimulus program; every cell beats once per pace, within the sampling bound of 2 * every ticks"""
    from fib_tf_amd.fenton import Fenton4v
    from fib_tf_amd.stimulus import Stimulus
    m = Fenton4v({'height': 64, 'width': 64, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 1200})
    m.define(s1=False)
    with m.program_stimuli([Stimulus((0, 64, 0, 6), 1.0, at_tick=0, period=300, count=0, floor=0.0)]):
        with m.record_beats(every=10, depth=4) as rec:
            m._stepper.step(1200)
            assert rec.samples() == 120
            b = rec.beats()
            assert (b['count'] == 4).all() and np.isfinite(b['t_up']).all() and b['t_up'].dtype == np.float32
            cl = rec.cl()
            assert cl.shape == (4, 64, 64) and np.isnan(cl[0]).all() and (np.abs(cl[1:] - 300) <= 20).all()
            di, apd = rec.restitution()
            assert len(di) == len(apd) == 3 * 64 * 64 and (di > 0).all() and (apd > 50).all()
            s = rec.summary(last=4)
            assert (s['nused'] == 4).all() and (np.abs(s['cl_mean'] - 300) <= 20).all() and (np.abs(s['apd_alt']) <= 20).all()
            assert (s['apd_mean'] >= rec.apd().min(axis=0)).all() and (s['apd_mean'] <= rec.apd().max(axis=0)).all()
    m._stepper.close()
