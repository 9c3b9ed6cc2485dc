"""-m gpu: the frame recorder behind a multi-tick launch that gave up (csrc/sched.inc recover(): the recorder's tick counter
goes back with the state, the replay fills the same slots of the cube again).

The method is that of tests/test_gpu_recovery_entry_points.py, whose handle, snapshots and comparisons are used here: the
yardstick is the library's own one-launch-per-tick mode (FIBHIP_MT=0), bit for bit; the give-up is the test switch
FIBHIP_MT_FAKE_GIVEUP=n — nothing is provoked, nothing waits out a bound; the fallback count is proved 0 immediately in front
of the call under test ('mark:before'); n runs over the launches that stand unconfirmed there."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_recovery_entry_points import AHEAD, ENV, SHAPES, _Handle, _Run, _counters, _same, _snapshot, _thin  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW, BLOCK = (2, 94, 4, 100), (2, 3)


def _play(lib, monkeypatch, script, env):
    """runs `script` on a fresh Fenton handle (96 x 100, the forced small shape) under `env`.  ints: step(n); ('x', n): n
    single-tick calls; ('fr_begin', every, first, fmt); 'fr_read', 'fr_count', 'fr_end'; 'get'; 'mark:<name>'"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', SHAPES['fenton'][2])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = _Handle(lib, 'fenton', False)
    st = h.st
    plane = np.random.default_rng(8).uniform(0.1, 1.0, (h.H, h.W)).astype(np.float32)
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
            elif name == 'fr_begin':
                st.frames_begin(0, WINDOW, BLOCK, 'mean', -0.02, 1.02, plane, op[3], op[1], op[2], 64)
            elif name == 'fr_read':
                out.obs.append(st.frames_read())
            elif name == 'fr_count':
                out.obs.append(np.int64(st.frames_count()))
            elif name == 'fr_end':
                st.frames_end()
            elif name == 'get':
                out.obs.append(st.get_state(0).copy())
            elif name.startswith('mark:'):
                out.marks[name[5:]] = _snapshot(st)
            else:
                raise AssertionError('unknown op %r' % (op,))
        out.obs.append(st.get_state(-1))
    out.stats, out.fb, out.tpl, out.plan = st.launch_stats(), st.fallbacks(), st.ticks_per_launch(), st.launch_plan()
    out.warned = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    h.close()
    return out


def _behind_a_give_up(lib, monkeypatch, script, ahead):
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
        _same(got, want, what)                              # every frame equals the FIBHIP_MT=0 run's
        _counters(got, want, what)                          # `ticks` is unchanged across the recovery
    return want, free


@pytest.mark.parametrize('ahead', AHEAD)
def test_frames_begin_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, ahead):
    """frames_begin defines tick 0 of the cube: it synchronises (and so recovers) before it attaches"""
    script = [40, 'mark:before', ('fr_begin', 3, 1, 'float32'), 'mark:after', ('x', 14), 9, 'fr_count', 'fr_read', 'get']
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] == 2, free.marks            # 32 + 8 ticks
    assert int(want.obs[0]) == 8 and want.obs[1].shape == (8, 46, 32)


@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('call', ['fr_read', 'fr_count', 'fr_end'])
def test_entry_points_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, call, ahead):
    """the recorder attached from the start, 30 ticks one call each and nothing that synchronises before the call under test: a
    ten-tick launch with a sample behind it, three times over — the give-up stands in front of a sample inside the series
    (n = 1, 2) or in front of the call itself (n = 3)"""
    tail = ['fr_read'] if call != 'fr_end' else []
    script = [('fr_begin', 10, 10, 'uint8'), ('x', 30), 'mark:before', call, 'mark:after', ('x', 20), 'get'] + tail
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] == 3 and free.marks['before']['ticks'] == 30, free.marks
    if call == 'fr_read':
        assert want.obs[0].shape == (3, 46, 32) and want.obs[0].dtype == np.uint8 and want.obs[2].shape == (5, 46, 32)
        assert len(np.unique(want.obs[0])) > 10


@pytest.mark.parametrize('ahead', AHEAD)
def test_a_sample_inside_a_series_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, ahead):
    """one call of 47 ticks with first = 4, every = 10: launches of 4, 10, 10, 10, 10 and 3 ticks, a sample behind each of the
    first five; the last three ticks wait for the read, which launches them, and nothing is confirmed before it"""
    script = [('fr_begin', 10, 4, 'float32'), 47, 'mark:before', 'fr_read', 'mark:after', 13, 'fr_read', 'get']
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] == 5 and free.marks['before']['ticks'] == 44, free.marks
    assert free.marks['after']['mt_launches'] == 6 and free.marks['after']['ticks'] == 47, free.marks
    assert want.obs[0].shape == (5, 46, 32) and want.obs[1].shape == (6, 46, 32)
