"""-m gpu: the spectrum recorder behind a multi-tick launch that gave up (csrc/sched.inc recover(): the recorder's tick counter
goes back with the state; the samples and the folds queued behind the lost launch wrote nothing, and the replay takes the lost
samples and issues the lost folds again, in order — no sample is folded twice, none is lost).

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
import spectrum_ref as ref  # noqa: E402
from test_gpu_recovery_entry_points import AHEAD, ENV, SHAPES, _Handle, _Run, _counters, _same, _snapshot, _thin  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW, BLOCK, BINS = (2, 94, 4, 100), (2, 3), [0, 1, 2]


def _play(lib, monkeypatch, script, env):
    """runs `script` on a fresh Fenton handle (96 x 100, the forced small shape) under `env`.  ints: step(n); ('x', n): n
    single-tick calls; ('sp_begin', every, nfft, chunk); 'sp_read', 'sp_peak', 'sp_count', 'sp_end'; 'get'; 'mark:<name>'"""
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
            elif name == 'sp_begin':
                _, every, nfft, chunk = op
                st.spectrum_begin(0, WINDOW, BLOCK, 'mean', plane, every, nfft, ref.hann(nfft), ref.twiddles(nfft), BINS, chunk)
            elif name == 'sp_read':
                P, seg = st.spectrum_read()
                out.obs += [P, np.int64(seg)]
            elif name == 'sp_peak':
                out.obs += list(st.spectrum_peak(0, len(BINS) - 1, 1))
            elif name == 'sp_count':
                out.obs.append(np.array(st.spectrum_count(), np.int64))
            elif name == 'sp_end':
                st.spectrum_end()
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
        _same(got, want, what)                              # every plane and map equals the FIBHIP_MT=0 run's
        _counters(got, want, what)                          # `ticks` is unchanged across the recovery
    return want, free


@pytest.mark.parametrize('ahead', AHEAD)
def test_spectrum_begin_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, ahead):
    """spectrum_begin defines tick 0 of the first segment: it synchronises (and so recovers) before it attaches"""
    script = [40, 'mark:before', ('sp_begin', 3, 4, 2), 'mark:after', ('x', 14), 13, 'sp_count', 'sp_read', 'sp_peak', 'get']
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] == 2, free.marks            # 32 + 8 ticks
    assert want.obs[0].tolist() == [9, 2] and want.obs[1].shape == (3, 46, 32) and int(want.obs[2]) == 2
    assert len(np.unique(want.obs[1])) > 100


@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('call', ['sp_read', 'sp_peak', 'sp_count', 'sp_end'])
def test_entry_points_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, call, ahead):
    """the recorder attached from the start (a sample every 10 ticks, segments of 4 samples, folds of 2), 50 ticks one call each
    and nothing that synchronises before the call under test: five ten-tick launches, each with a sample behind it — the
    give-up stands in front of a mid-chunk sample (n = 1, 3, 5), in front of the sample whose fold ends no segment (n = 2), in
    front of the sample whose fold ends a segment (n = 4); whatever n, the call under test is the first to find it"""
    tail = ['sp_read', 'sp_peak', 'sp_count'] if call != 'sp_end' else []
    script = [('sp_begin', 10, 4, 2), ('x', 50), 'mark:before', call, 'mark:after', ('x', 30), 'get'] + tail
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] == 5 and free.marks['before']['ticks'] == 50, free.marks
    if call == 'sp_read':
        assert want.obs[0].shape == (3, 46, 32) and int(want.obs[1]) == 1 and int(want.obs[4]) == 2
        assert len(np.unique(want.obs[0])) > 100 and want.obs[0].tobytes() != want.obs[3].tobytes()
    if call == 'sp_count':
        assert want.obs[0].tolist() == [5, 1] and want.obs[-2].tolist() == [8, 2]


@pytest.mark.parametrize('ahead', AHEAD)
def test_samples_inside_a_series_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, ahead):
    """one call of 47 ticks, a sample every 5 ticks, segments of 4, folds of 4: nine launches of five ticks, a sample behind
    each, a fold that ends a segment behind the fourth and the eighth; the ring of four planes is shorter than what is queued
    behind an unconfirmed launch, so a sample behind a launch that gave up must not overwrite a slot that is still to be folded;
    the last two ticks wait for the read, which launches them, and nothing is confirmed before it"""
    script = [('sp_begin', 5, 4, 4), 47, 'mark:before', 'sp_read', 'mark:after', 'sp_peak', 13, 'sp_read', 'sp_count', 'get']
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, script, ahead)
    assert free.marks['before']['mt_launches'] == 9 and free.marks['before']['ticks'] == 45, free.marks
    assert free.marks['after']['mt_launches'] == 10 and free.marks['after']['ticks'] == 47, free.marks
    assert int(want.obs[1]) == 2 and int(want.obs[7]) == 3 and want.obs[8].tolist() == [12, 3]
