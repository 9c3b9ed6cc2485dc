"""-m gpu: a series of ticks the caller has DECLARED (fibhip_expect, as IonicModel.run() does) goes out in launches of up to
MT_MAX_TICKS_DECLARED ticks (csrc/ctx.hpp: 256) instead of 32 when it holds MT_DECLARED_MIN_TICKS (128) ticks or more — and stays
as cheap to break, to sample inside of and to recover from as the short launches were.

The yardstick is the library's own one-launch-per-tick mode (FIBHIP_MT=0): every state array, and every recorded trace, must
match it bit for bit.  Grids of 96 x 96: with Fenton's 44 x 25 tiles that is 3 x 4 tiles — interior, edge and corner tiles; both
arithmetic policies."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = ('FIBHIP_MT', 'FIBHIP_MT_MAX', 'FIBHIP_MT_FAKE_GIVEUP', 'FIBHIP_AHEAD', 'FIBHIP_MT_WAIT_MS', 'FIBHIP_MT_IDS', 'FIBHIP_VARIANT',
       'FIBHIP_AUTOTUNE')
N = 96
VARIANT = {'fenton': '10,44,25,-3', 'br': '5,54,21,-2'}         # the forced small shapes of tests/test_gpu_recovery.py
CAP, CAP_UNDECLARED, LONG = 256, 32, 128                        # MT_MAX_TICKS_DECLARED, MT_MAX_TICKS, MT_DECLARED_MIN_TICKS
KINDS = [pytest.param(k, p, id='%s-%s' % (k, p)) for k in ('fenton', 'br') for p in ('fast', 'exact')]
POLICIES = ['fast', 'exact']


def _model(monkeypatch, kind, policy, env):
    """the model at 96 x 96 with a hole in its phase field, its S1 wave under way, 's2' registered, one tick done (the plan is
    chosen on the first tick) and the stream idle"""
    from fib_tf_amd.br import BeelerReuter
    from fib_tf_amd.fenton import Fenton4v
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT[kind])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = {'width': N, 'height': N, 'dt': 0.1, 'dt_per_plot': 10, 'duration': 1000, 'skip': False, 'cheby': True,
           'fast_math': policy == 'fast', 'diff': 1.5 if kind == 'fenton' else 0.809}
    m = (Fenton4v if kind == 'fenton' else BeelerReuter)(cfg)
    m.add_hole_to_phase_field(40, 48, 9)
    m.define()
    m.add_pace_op('s2', 'luq', 1.0 if kind == 'fenton' else 10.0)
    st = m._stepper
    st.step(1)
    st.sync()
    return m, st


def _series(monkeypatch, kind, policy, env, ticks, declare=True, broken_at=None):
    """one tick, then `ticks` ticks one call each, declared as one series; broken_at: image() and fire_op('s2') after that
    many of them.  Returns (state, launch_stats, ticks_per_launch while the series runs)"""
    m, st = _model(monkeypatch, kind, policy, env)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)      # (the one warning of a launch that gave up)
        if declare:
            st.expect(ticks)
        tpl = st.ticks_per_launch()
        for t in range(ticks):
            if t == broken_at:
                m.image()
                m.fire_op('s2')
            st.step(1)
        state = st.get_state(-1)
        stats = st.launch_stats()
    stats['tpl_after'] = st.ticks_per_launch()
    st.close()
    return state, stats, tpl


_reference = {}


def _one_launch_per_tick(monkeypatch, kind, policy, ticks, broken_at=None):
    """the same calls with FIBHIP_MT=0, computed once per case and shared"""
    key = (kind, policy, ticks, broken_at)
    if key not in _reference:
        state, stats, tpl = _series(monkeypatch, kind, policy, {'FIBHIP_MT': '0'}, ticks, broken_at=broken_at)
        assert tpl == 1 and stats['mt_launches'] == 0 and stats['ticks'] == 1 + ticks, stats
        state.setflags(write=False)
        _reference[key] = state
    return _reference[key]


def _same(got, want, what):
    assert np.isfinite(got).all(), what
    for v in range(len(want)):
        assert np.array_equal(got[v], want[v]), '%s: array %d differs (max |d| %.3g)' % (what, v, float(np.abs(got[v] - want[v]).max()))


@pytest.mark.parametrize('kind,policy', KINDS)
def test_declared_series_is_bit_identical_in_long_launches(gpu_lib, monkeypatch, kind, policy):
    """300 declared ticks under the default cap, under FIBHIP_MT_MAX=32 and one launch per tick: the same bits in every array.
    The launches are counted: 10 of up to 32 ticks, and ceil(300 / 256) = 2 under the default cap of 256 — the cap the
    measurement chose is below 300, so the series is two launches (256 + 44) rather than the one a cap above 300 would
    make; a series of exactly the cap is checked to be ONE launch right behind it, on the same handle."""
    want = _one_launch_per_tick(monkeypatch, kind, policy, 300)
    short, s32, tpl32 = _series(monkeypatch, kind, policy, {'FIBHIP_MT_MAX': '32'}, 300)
    assert tpl32 == 32 and s32['mt_launches'] == 10 and s32['mt_ticks'] == 300 and s32['ticks'] == 301, s32
    _same(short, want, 'FIBHIP_MT_MAX=32')

    m, st = _model(monkeypatch, kind, policy, {})
    st.expect(300)
    assert st.ticks_per_launch() == CAP
    for _ in range(300):
        st.step(1)
    got = st.get_state(-1)
    s = st.launch_stats()
    assert st.ticks_per_launch() == CAP_UNDECLARED           # (no declared series is running any more)
    assert s['mt_launches'] == -(-300 // CAP) and s['mt_ticks'] == 300 and s['ticks'] == 301, s
    assert s['gave_up_recovered'] == 0 and s['ahead_recomputed'] == 0, s
    _same(got, want, 'default cap')
    st.expect(CAP)                                            # a series that fits the cap: one launch
    for _ in range(CAP):
        st.step(1)
    st.sync()
    s2 = st.launch_stats()
    assert s2['mt_launches'] == s['mt_launches'] + 1 and s2['mt_ticks'] == 300 + CAP and s2['ticks'] == 301 + CAP, s2
    st.close()


@pytest.mark.parametrize('kind,policy', KINDS)
def test_declared_series_broken_in_the_middle(gpu_lib, monkeypatch, kind, policy):
    """300 ticks declared; after 137 of them the caller reads a frame (image()) and fires 's2', then goes on to 300.  The launch
    that ran ahead is stopped at the tick the caller reached, or recomputed — which of the two is the device's business; the
    state is that of the one-launch-per-tick run and no tick is counted twice or lost."""
    want = _one_launch_per_tick(monkeypatch, kind, policy, 300, broken_at=137)
    got, s, tpl = _series(monkeypatch, kind, policy, {}, 300, broken_at=137)
    assert tpl == CAP
    _same(got, want, 'series broken after 137 of 300 ticks')
    assert s['ticks'] == 301, s
    assert s['ahead_stopped_in_time'] + s['ahead_recomputed'] == 1, s
    assert s['gave_up_recovered'] == 0, s


@pytest.mark.parametrize('policy', POLICIES)
def test_no_declared_launch_spans_a_sample_tick(gpu_lib, monkeypatch, policy):
    """an electrode recorder that samples every 7th tick bounds every launch of a declared series of 300: 42 samples, at least
    ceil(300 / 7) launches, and the trace of the one-launch-per-tick run"""
    rects = [(10, 30, 20, 50), (0, 64, 0, 90)]
    rng = np.random.default_rng(7)
    patches = [rng.uniform(0, 1, (r1 - r0, c1 - c0)).astype(np.float32) for r0, r1, c0, c1 in rects]

    def run(env):
        m, st = _model(monkeypatch, 'fenton', policy, env)
        st.electrode_begin(0, rects, patches, every=7, capacity=64)
        before = st.launch_stats()
        st.expect(300)
        for _ in range(300):
            st.step(1)
        trace = st.electrode_read()
        after = st.launch_stats()
        state = st.get_state(-1)
        st.close()
        return trace, state, {k: after[k] - before[k] for k in ('mt_launches', 'mt_ticks', 'ticks')}

    want, want_state, d0 = run({'FIBHIP_MT': '0'})
    got, got_state, d = run({})
    assert want.shape == (42, 2) and got.shape == (42, 2) and np.isfinite(got).all()
    assert np.array_equal(got, want), 'max |d| %.3g' % float(np.abs(got - want).max())
    _same(got_state, want_state, 'state behind the sampled series')
    assert d0['ticks'] == 300 and d['ticks'] == 300 and d['mt_ticks'] == 300, (d0, d)
    assert d['mt_launches'] >= -(-300 // 7), d             # (fewer: some launch held more than 7 ticks, so spanned a sample)


@pytest.mark.parametrize('policy', POLICIES)
def test_long_declared_launch_that_gives_up_is_recovered(gpu_lib, monkeypatch, policy):
    """FIBHIP_MT_FAKE_GIVEUP=1: the first multi-tick launch — the 200 declared ticks in one — finds the give-up word raised
    in its name.  The host recomputes its ticks one launch per tick from the state it started from: the same bits, and every
    counter exact."""
    want = _one_launch_per_tick(monkeypatch, 'fenton', policy, 200)
    got, s, tpl = _series(monkeypatch, 'fenton', policy, {'FIBHIP_MT_FAKE_GIVEUP': '1'}, 200)
    assert tpl == CAP
    _same(got, want, 'after the recovery')
    assert s['ticks'] == 201 and s['mt_ticks'] == 0 and s['mt_launches'] == 0, s
    assert s['gave_up_recovered'] == 1 and s['ticks_recomputed_after_give_up'] == 200, s
    assert s['tpl_after'] == 1, s                             # one launch per tick from here on


def test_undeclared_caller_keeps_the_short_cap(gpu_lib, monkeypatch):
    """100 single-tick calls and no declaration: the launches grow 2, 4, ... 32 and no further"""
    m, st = _model(monkeypatch, 'fenton', 'fast', {})
    assert st.ticks_per_launch() == CAP_UNDECLARED
    seen = []
    last = st.launch_stats()
    for _ in range(100):
        st.step(1)
        s = st.launch_stats()
        dl, dt = s['mt_launches'] - last['mt_launches'], s['mt_ticks'] - last['mt_ticks']
        if dl:
            assert dl == 1 and dt <= CAP_UNDECLARED, (dl, dt, seen)
            seen.append(dt)
        last = s
    st.sync()
    s = st.launch_stats()
    dl, dt = s['mt_launches'] - last['mt_launches'], s['mt_ticks'] - last['mt_ticks']
    assert dt <= CAP_UNDECLARED * max(dl, 1), (dl, dt)
    assert s['ticks'] == 101 and max(seen) == CAP_UNDECLARED, (s, seen)
    st.close()


@pytest.mark.parametrize('ticks,launches', [(70, 3), (LONG - 1, 4), (LONG, 1)])
def test_short_declared_series_keeps_its_launches(gpu_lib, monkeypatch, ticks, launches):
    """a declaration below MT_DECLARED_MIN_TICKS goes out 32 ticks at a time as it always did (70 = 32 + 32 + 6); from that
    length on it is one launch.  The same bits either way."""
    want = _one_launch_per_tick(monkeypatch, 'fenton', 'fast', ticks)
    got, s, tpl = _series(monkeypatch, 'fenton', 'fast', {}, ticks)
    assert tpl == (CAP if ticks >= LONG else CAP_UNDECLARED)
    assert s['mt_launches'] == launches and s['mt_ticks'] == ticks and s['ticks'] == 1 + ticks, s
    _same(got, want, '%d declared ticks' % ticks)
