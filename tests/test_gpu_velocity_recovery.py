"""-m gpu: the velocity fit behind a multi-tick launch that gave up (csrc/sched.inc recover()): fibhip_beats_velocity reads the
ring through read_confirmed like fibhip_beats_summary — if the wait behind its launch finds a give-up, the state is recovered, the
lost samples are taken again and the fit is launched once more on the planes as they then stand.

The method and the helpers are those of tests/test_gpu_beats_recovery.py: the yardstick is the library's own one-launch-per-tick
mode (FIBHIP_MT=0), every bit of every number (NaN for NaN); the give-up is the test switch FIBHIP_MT_FAKE_GIVEUP=n — nothing is
provoked, nothing waits out a bound; the fallback count is proved 0 immediately in front of the call under test ('mark:before');
n runs over the launches that stand unconfirmed there.

The activation recorder sees every tick, so while it is attached no launch fuses ticks and fibhip_observe_velocity never has an
unconfirmed multi-tick launch directly in front of it: the launch that gives up stands in front of fibhip_observe_begin, which
recovers before it attaches, and the call under test is the pair — attach, run, fit."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import velocity_ref as ref  # noqa: E402
from test_gpu_beats_recovery import BLOCK, DOWN, UP, WINDOW  # noqa: E402
from test_gpu_recovery_entry_points import AHEAD, ENV, SHAPES, _Run, _counters, _snapshot, _thin  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402

pytestmark = pytest.mark.gpu

FIT = (2, 20.0, 13)                                          # radius, max_dt, min_cells


def _play(lib, monkeypatch, script, env):
    """test_gpu_beats_recovery._play's sheet (Fenton 96 x 100 at the forced small shape, the S1 wave and a stimulus in the middle
    on their way).  ints: step(n); ('x', n): n single-tick calls; ('bt_begin', every, depth), 'bt_read', 'bt_count', 'bt_velocity'
    (the newest beat); 'obs_begin', 'obs_maps', 'obs_velocity' (last_up); 'get'; 'mark:<name>'"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', SHAPES['fenton'][2])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(SHAPES['fenton'][0], SHAPES['fenton'][1])
    st = m._stepper
    st.pace(32, 39, 33, 42, 1.0, 0.0)
    plane = np.random.default_rng(8).uniform(0.9, 1.0, (m.height, m.width)).astype(np.float32)
    out = _Run()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for op in script:
            name = op if isinstance(op, str) else (None if isinstance(op, int) else op[0])
            if isinstance(op, int):
                st.step(op)
            elif name == 'x':
                for _ in range(op[1]):
                    st.step(1)
            elif name == 'bt_begin':
                st.beats_begin(0, WINDOW, BLOCK, 'mean', plane, op[1], UP, DOWN, op[2])
            elif name == 'bt_read':
                out.obs += list(st.beats_read())
            elif name == 'bt_velocity':
                out.obs += list(st.beats_velocity(0, *FIT))
            elif name == 'bt_count':
                out.obs.append(np.array([st.beats_count()], np.int64))
            elif name == 'obs_begin':
                st.observe_begin(0, 0.5, 0.1)
            elif name == 'obs_maps':
                out.obs += [st.observe_get(which) for which in lib.OBS_MAPS]
            elif name == 'obs_velocity':
                out.obs += list(st.observe_velocity('last_up', *FIT))
            elif name == 'get':
                out.obs.append(st.get_state(0).copy())
            elif name.startswith('mark:'):
                out.marks[name[5:]] = _snapshot(st)
            else:
                raise AssertionError('unknown op %r' % (op,))
        out.obs.append(st.get_state(-1))
    out.stats, out.fb, out.tpl, out.plan = st.launch_stats(), st.fallbacks(), st.ticks_per_launch(), st.launch_plan()
    out.warned = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    st.close()
    return out


def _same(got, want, what):
    assert len(got.obs) == len(want.obs)
    for i, (x, y) in enumerate(zip(got.obs, want.obs)):
        assert ref.same(x, y), '%s: observation %d differs from the one-launch-per-tick run' % (what, i)


def _behind_a_give_up(lib, monkeypatch, script, ahead):
    """test_gpu_beats_recovery._behind_a_give_up over this file's _play"""
    base = {} if ahead else {'FIBHIP_AHEAD': '0'}
    want = _play(lib, monkeypatch, script, dict(base, FIBHIP_MT='0'))
    free = _play(lib, monkeypatch, script, base)
    assert want.fb == (0, 0) and not want.warned and want.stats['mt_launches'] == 0
    assert free.fb == (0, 0) and not free.warned and free.stats['mt_launches'] >= 1, free.stats
    _same(free, want, 'untouched')
    _counters(free, want, 'untouched')
    hi = free.marks['after']['mt_launches']
    assert hi >= 1, 'no multi-tick launch stands in front of the call under test: %r' % (free.marks,)
    for nth in _thin(list(range(1, hi + 1)), most=6):
        what = 'launch %d of %d gave up' % (nth, hi)
        got = _play(lib, monkeypatch, script, dict(base, FIBHIP_MT_FAKE_GIVEUP=str(nth)))
        assert got.marks['before']['fb'] == (0, 0), (what, 'found before the call under test', got.marks)
        assert got.fb[0] == 1, (what, got.fb)
        _same(got, want, what)
        _counters(got, want, what)
    return want, free


@pytest.mark.parametrize('ahead', AHEAD)
def test_beats_velocity_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, ahead):
    """the recorder attached from the start (a sample every 10 ticks), 50 ticks one call each and nothing that synchronises before
    the fit: five ten-tick launches, each with a sample behind it; whatever n, fibhip_beats_velocity is the first to find the
    give-up, and its maps are those of the one-launch-per-tick run"""
    script = [('bt_begin', 10, 4), ('x', 50), 'mark:before', 'bt_velocity', 'mark:after', ('x', 30), 'get', 'bt_read', 'bt_velocity', 'bt_count']
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] == 5 and free.marks['before']['ticks'] == 50, free.marks
    nfit, gy = want.obs[0], want.obs[1]
    assert nfit.shape == (46, 32) and nfit.dtype == np.int32 and np.isfinite(gy).sum() > 100      # the fit had something to fit
    t_up, count = want.obs[5], want.obs[8]
    assert all(ref.same(g, w) for g, w in zip(want.obs[10:14], ref.fit(t_up, count, 0, *FIT)))   # and the yardstick is the restatement's


@pytest.mark.parametrize('ahead', AHEAD)
def test_observe_velocity_on_a_recorder_attached_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, ahead):
    """ten ticks in multi-tick launches, none confirmed (the S1 wave is a third of the way across); then the activation recorder
    is attached — it recovers before it copies the potential it compares the first tick with —, 23 ticks are observed one launch
    each, and the fit on last_up equals the one-launch-per-tick run's"""
    script = [10, 'mark:before', 'obs_begin', ('x', 14), 9, 'obs_velocity', 'mark:after', 'obs_maps', 'get']
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] >= 1 and free.marks['after']['mt_launches'] == free.marks['before']['mt_launches'], free.marks
    nfit, gy = want.obs[0], want.obs[1]
    assert nfit.shape == (96, 100) and np.isfinite(gy).sum() > 100
    last_up, count = want.obs[5], want.obs[8]
    assert all(ref.same(g, w) for g, w in zip(want.obs[:4], ref.fit(last_up[None], count, 0, *FIT)))
