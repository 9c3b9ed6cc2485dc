"""-m gpu: the trigger program behind multi-tick launches that give up (csrc/sched.inc recover(), the rule above confirm()).
The automaton's state IS the log on the device: row s follows from row s - 1 and the state.  Sense, decide and the gated apply
are queued behind their launch without confirming it; the gated apply writes nothing once a launch in front of it gave up, and
the replay rewrites the rows of the lost samples in order — no detection lost, none doubled, a pending delay and a half-delivered
train come out as in the untouched run.  The give-up is the test switch FIBHIP_MT_FAKE_GIVEUP=n (the n-th multi-tick launch
finds the give-up word raised and leaves at its first boundary): nothing waits out a bound, nothing is provoked.  The yardsticks
are the untouched run and the FIBHIP_MT=0 run, byte for byte.  The train is ADD: a pulse applied twice or not at all shows."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_frames import PLAN_ENV, VARIANT_96x100, wave  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402

pytestmark = pytest.mark.gpu

EVERY = 5
SITE = dict(r0=84, r1=91, c0=85, c1=93)


def program():
    """every = 5, six launches of five ticks.  Rule 0 paces the site at rest when nothing arrived for two samples (detected at
    sample 1, in the 2nd launch); rule 1 sees the rise at sample 2 (3rd launch) and answers one sample later with a train of
    three ADD pulses at the samples 3, 4, 5: a detection, a delay and a train that straddle whichever launch gives up"""
    sensor = dict(var=0, level=0.5, need=1, site='rect', **SITE)
    stim = dict(var=0, shape='rect', **SITE)
    return [sensor], [dict(stim, sensor=0, edge='rise', escape=2, blank=30, mode='max', v=1.0, floor=0.0),
                      dict(stim, sensor=0, edge='rise', blank=8, delay=1, count=3, period=1, mode='add', v=-0.0625, floor=0.0)]


def _run(monkeypatch, env, script):
    """`script`: ints = step(n); ('x', n) = n single-tick calls; 'begin' / 'read' / 'end' / 'mark' on a Fenton handle at the forced
    12-tile shape.  Returns (logs read, final state, fallbacks, launch stats since the wave, marks)"""
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    sensors, rules = program()
    logs, marks = [], []
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        s0 = st.launch_stats()
        for op in script:
            if isinstance(op, int):
                st.step(op)
            elif isinstance(op, tuple):
                for _ in range(op[1]):
                    st.step(1)
            elif op == 'begin':
                st.trig_begin(sensors, rules, every=EVERY, capacity=16)
            elif op == 'read':
                logs.append(st.trig_read().tobytes())
            elif op == 'end':
                st.trig_end()
            elif op == 'mark':
                marks.append((st.fallbacks(), st.launch_stats()['mt_launches'] - s0['mt_launches']))
        state = st.get_state(-1).tobytes()
        fb, s1 = st.fallbacks(), st.launch_stats()
    st.close()
    stats = {k_: s1[k_] - s0[k_] for k_ in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
    stats['before'] = s0['mt_launches']                       # (the multi-tick launches of wave(): FIBHIP_MT_FAKE_GIVEUP counts them)
    return logs, state, fb, stats, marks


def rows_of(log):
    return np.frombuffer(log, np.int32).reshape(-1, 2, 6)


@pytest.mark.parametrize('nth', [1, 3, 4, 6])
def test_give_up_with_samples_queued_behind_it(gpu_lib, monkeypatch, nth):
    """30 ticks one call each: six five-tick launches, each with a sample (and from the 2nd on a stimulus) queued behind it, nothing
    synchronises before the state is read.  The first, a middle (the one that holds the rise detection; the one inside the
    train) and the last launch give up: log, state and detection count are those of the untouched run."""
    script = ['begin', ('x', 30), 'mark']
    logs, state, fb0, s0, marks0 = _run(monkeypatch, {}, script + ['read'])
    assert fb0 == (0, 0) and marks0[0][1] == 6 and s0['ticks'] == 30 and s0['mt_ticks'] == 30, (fb0, marks0, s0)
    assert s0['launches'] == 6 + 3 * 6, s0
    rows = rows_of(logs[0])
    assert rows[:, 0, 4].tolist() == [0, 2, 0, 0, 0, 0] and rows[:, 1, 4].tolist() == [0, 0, 1, 0, 0, 0], rows    # escape, then the rise
    assert rows[:, 0, 5].tolist() == [0, 1, 0, 0, 0, 0] and rows[:, 1, 5].tolist() == [0, 0, 0, 1, 1, 1], rows    # the pace, the train
    plogs, pstate, pfb, ps, _ = _run(monkeypatch, {'FIBHIP_MT': '0'}, script + ['read'])
    assert pstate == state and plogs == logs and pfb == (0, 0) and ps['mt_ticks'] == 0 and ps['ticks'] == 30
    # (the log is read AFTER the state here: reading it flushes and would find the give-up first)
    _, gstate, fb, s, marks = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script)
    assert marks[0][0] == (0, 0)                              # (not found before the read: the samples were queued behind it)
    assert fb[0] == 1 and fb[1] > 0, (nth, fb)                # one launch gave up and was recovered
    assert gstate == state, nth
    assert s['ticks'] == 30 and s['mt_ticks'] + fb[1] <= 30, (s, fb)
    glogs, cstate, cfb, _, _ = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script + ['read'])
    assert glogs == logs and cstate == state and cfb[0] == 1, (nth, rows_of(glogs[0]), rows)
    assert rows_of(glogs[0])[-1, :, 3].tolist() == [1, 1]    # one detection per rule: none lost, none doubled


@pytest.mark.parametrize('entry', ['begin', 'read', 'end'])
def test_give_up_in_front_of_begin_read_and_end(gpu_lib, monkeypatch, entry):
    """trig_begin, trig_read and trig_end directly behind multi-tick launches nobody has confirmed, the last of which gave up"""
    script = {'begin': [20, 'mark', 'begin', ('x', 30), 'read'],
              'read': ['begin', ('x', 20), 'mark', 'read', ('x', 10), 'read'],
              'end': ['begin', ('x', 20), 'mark', 'end', 7, 'begin', ('x', 10), 'read']}[entry]
    want, state, fb0, s0, marks0 = _run(monkeypatch, {}, script)
    assert fb0 == (0, 0) and marks0[0][1] >= 1, marks0
    for nth in sorted({1, marks0[0][1]}):
        got, gstate, fb, s, marks = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script)
        assert marks[0][0] == (0, 0) and fb[0] == 1, (entry, nth, marks, fb)
        assert got == want and gstate == state, (entry, nth)
        assert s['ticks'] == s0['ticks'], (s, s0)
