"""-m gpu: the beat recorder behind a multi-tick launch that gave up (csrc/sched.inc recover(): the recorder's tick counter goes
back with the state; the samples queued behind the lost launch wrote nothing, and the replay takes the lost samples again, in
order — no upstroke is counted twice, none is lost, and every time is the one the sample index gives).

The method is that of tests/test_gpu_spectrum_recovery.py: the yardstick is the library's own one-launch-per-tick mode
(FIBHIP_MT=0), every bit of every number (NaN for NaN); the give-up is the test switch FIBHIP_MT_FAKE_GIVEUP=n — nothing is
provoked, nothing waits out a bound; the fallback count is proved 0 immediately in front of the call under test
('mark:before'); n runs over the launches that stand unconfirmed there."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beat_ref as ref  # noqa: E402
from test_gpu_recovery_entry_points import AHEAD, ENV, SHAPES, _Run, _counters, _snapshot, _thin  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW, BLOCK = (2, 94, 4, 100), (2, 3)
UP, DOWN = np.float32(0.5), np.float32(0.1)


def _play(lib, monkeypatch, script, env):
    """runs `script` on a fresh Fenton model (96 x 100, the forced small shape; the S1 wave and a stimulus in the middle on
    their way) under `env`.  ints: step(n); ('x', n): n single-tick calls; ('bt_begin', every, depth); 'bt_read', 'bt_summary',
    'bt_count', 'bt_end'; 'get'; 'mark:<name>'"""
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
                _, every, depth = op
                st.beats_begin(0, WINDOW, BLOCK, 'mean', plane, every, UP, DOWN, depth)
            elif name == 'bt_read':
                out.obs += list(st.beats_read())
            elif name == 'bt_summary':
                out.obs += list(st.beats_summary(1))
            elif name == 'bt_count':
                out.obs.append(np.array([st.beats_count()], np.int64))
            elif name == 'bt_end':
                st.beats_end()
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


def _behind_a_give_up(lib, monkeypatch, script, ahead, nths=None):
    base = {} if ahead else {'FIBHIP_AHEAD': '0'}
    want = _play(lib, monkeypatch, script, dict(base, FIBHIP_MT='0'))
    free = _play(lib, monkeypatch, script, base)
    assert want.fb == (0, 0) and not want.warned and want.stats['mt_launches'] == 0
    assert free.fb == (0, 0) and not free.warned and free.stats['mt_launches'] >= 1, free.stats
    _same(free, want, 'untouched')
    _counters(free, want, 'untouched')
    hi = free.marks['after']['mt_launches']
    assert hi >= 1, 'no multi-tick launch stands in front of the call under test: %r' % (free.marks,)
    for nth in (nths if nths is not None else _thin(list(range(1, hi + 1)), most=6)):
        assert 1 <= nth <= hi
        what = 'launch %d of %d gave up' % (nth, hi)
        got = _play(lib, monkeypatch, script, dict(base, FIBHIP_MT_FAKE_GIVEUP=str(nth)))
        assert got.marks['before']['fb'] == (0, 0), (what, 'found before the call under test', got.marks)
        assert got.fb[0] == 1, (what, got.fb)
        _same(got, want, what)                              # every plane and map equals the FIBHIP_MT=0 run's
        _counters(got, want, what)                          # `ticks` is unchanged across the recovery
    return want, free


EVERY, SAMPLES, DEPTH = 20, 20, 2


def _what_each_sample_records(lib, monkeypatch):
    """a run of its own, one launch per tick, read after every sample: per sample, how many upstrokes and downstrokes it recorded"""
    script = [('bt_begin', EVERY, DEPTH)]
    for _ in range(SAMPLES):
        script += [EVERY, 'bt_read']
    obs = _play(lib, monkeypatch, script, {'FIBHIP_MT': '0'}).obs
    ups, downs = [], []
    n0, down0 = 0, 0
    for s in range(SAMPLES):
        t_up, t_down, peak, n, pk = obs[5 * s:5 * s + 5]
        closed = int(n.sum()) - int((pk == pk).sum())        # every beat is open or was closed (by a downstroke or by the next upstroke)
        ups.append(int(n.sum()) - n0)
        downs.append(closed - down0)
        n0, down0 = int(n.sum()), closed
    return ups, downs


@pytest.mark.parametrize('ahead', AHEAD)
def test_the_launch_in_front_of_each_kind_of_sample_gives_up(gpu_lib, monkeypatch, ahead):
    """four hundred single-tick calls: twenty launches of twenty ticks with a sample behind each, a ring of two beats, and nothing
    that synchronises before the read: the give-up stands in front of a sample that records nothing, of one that records
    upstrokes, of one that records downstrokes, and in the very first launch — nineteen launches, far more than the ring is
    deep, stand unconfirmed behind it, their samples void"""
    ups, downs = _what_each_sample_records(gpu_lib, monkeypatch)
    nothing = [s for s in range(SAMPLES) if ups[s] == 0 and downs[s] == 0]
    rising = [s for s in range(1, SAMPLES) if ups[s] > 0]
    falling = [s for s in range(SAMPLES) if downs[s] > 0 and ups[s] == 0]
    print('upstrokes per sample', ups, 'downstrokes', downs)
    assert nothing and rising and falling, (ups, downs)
    script = [('bt_begin', EVERY, DEPTH), ('x', EVERY * SAMPLES), 'mark:before', 'bt_read', 'mark:after', 'bt_summary', ('x', 2 * EVERY),
              'bt_read', 'bt_count', 'get']
    nths = sorted({1, nothing[0] + 1, rising[0] + 1, falling[0] + 1})         # launch s + 1 stands in front of sample s
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead, nths)
    assert free.marks['before']['mt_launches'] == SAMPLES and free.marks['before']['ticks'] == EVERY * SAMPLES, free.marks
    assert SAMPLES - 1 > DEPTH and want.obs[3].sum() == sum(ups) and want.obs[14].tolist() == [SAMPLES + 2]


@pytest.mark.parametrize('ahead', AHEAD)
def test_beats_begin_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, ahead):
    """beats_begin defines tick 0 and the first xp: it synchronises (and so recovers) before it attaches"""
    script = [10, 'mark:before', ('bt_begin', 3, 2), 'mark:after', ('x', 14), 13, 'bt_count', 'bt_read', 'bt_summary', 'get']
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] >= 1, free.marks
    assert want.obs[0].tolist() == [9] and want.obs[1].shape == (2, 46, 32) and want.obs[4].sum() > 0


@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('call', ['bt_read', 'bt_summary', 'bt_count', 'bt_end'])
def test_entry_points_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, call, ahead):
    """the recorder attached from the start (a sample every 10 ticks), 50 ticks one call each and nothing that synchronises
    before the call under test: five ten-tick launches, each with a sample behind it; whatever n, the call under test is the
    first to find the give-up"""
    tail = ['bt_read', 'bt_summary', 'bt_count'] if call != 'bt_end' else []
    script = [('bt_begin', 10, 4), ('x', 50), 'mark:before', call, 'mark:after', ('x', 30), 'get'] + tail
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] == 5 and free.marks['before']['ticks'] == 50, free.marks
    if call == 'bt_read':
        assert want.obs[0].shape == (4, 46, 32) and want.obs[3].sum() > 100 and len(np.unique(want.obs[0])) > 100
    if call == 'bt_count':
        assert want.obs[0].tolist() == [5] and want.obs[-2].tolist() == [8]
