"""-m gpu: the stimulus program behind multi-tick launches that give up (csrc/sched.inc recover(), the rule above confirm()).
The stimulus is queued behind its launch without confirming it; stim_kernel writes nothing once a launch in front of it gave up,
and the replay applies the events of the replayed ticks again — and no others.  The give-up is the test switch
FIBHIP_MT_FAKE_GIVEUP=n (the n-th multi-tick launch finds the give-up word raised and leaves at its first boundary): nothing
waits out a bound, nothing hangs.  The yardsticks are the untouched run, the FIBHIP_MT=0 run and the run that fires from its loop
body, byte for byte.  The ADD entry is what shows an event applied twice or not at all: MAX alone is idempotent."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_frames import PLAN_ENV, VARIANT_96x100, wave  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402

pytestmark = pytest.mark.gpu

LEFT = dict(var=0, mode='max', shape='rect', r0=0, r1=96, c0=0, c1=5, v=1.0, floor=0.0, first=4, period=5, count=0)


def program(with_add):
    """S1 from 'left' after ticks 4, 9, 14, ... (floor = Fenton's min_v = 0: fire_op's operation); with_add: a plane added to
    array 2 at the same ticks, behind it in the program"""
    if not with_add:
        return [LEFT], None
    rng = np.random.default_rng(7)
    plane = np.zeros((96, 100), np.float32)
    plane[11:70, 3:90] = rng.uniform(-0.01, 0.01, (59, 87)).astype(np.float32)
    return [LEFT, dict(var=2, mode='add', shape='plane', plane=0, first=4, period=5, count=0)], [plane]


def _run(monkeypatch, env, script, with_add=False, fire=False):
    """`script`: ints = step(n); ('x', n) = n single-tick calls; 'begin' / 'count' / 'end' / 'mark' on a Fenton handle at the
    forced 12-tile shape.  fire: no program — the loop body fires 'left' after the ticks the program would (single-tick calls
    only).  Returns (counts read, final state, fallbacks, launch stats since the wave, marks)"""
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(96, 100)
    assert float(m.min_v) == LEFT['floor'] and m.pace_rect('left') == (0, 96, 0, 5)
    st = m._stepper
    wave(m, 'fenton')
    entries, planes = program(with_add)
    counts, marks = [], []
    attached, k = False, 0
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        s0 = st.launch_stats()
        for op in script:
            if isinstance(op, int):
                assert not fire
                st.step(op)
            elif isinstance(op, tuple):
                for _ in range(op[1]):
                    st.step(1)
                    if fire and attached and k % 5 == 4:
                        st.pace(0, 96, 0, 5, 1.0, 0.0)
                    k += 1
            elif op == 'begin':
                attached, k = True, 0
                if not fire:
                    st.stim_begin(entries, planes)
            elif op == 'count' and not fire:
                counts.append(st.stim_count())
            elif op == 'end':
                attached = False
                if not fire:
                    st.stim_end()
            elif op == 'mark':
                marks.append((st.fallbacks(), st.launch_stats()['mt_launches'] - s0['mt_launches']))
        state = st.get_state(-1).tobytes()
        fb, s1 = st.fallbacks(), st.launch_stats()
    st.close()
    stats = {k_: s1[k_] - s0[k_] for k_ in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
    stats['before'] = s0['mt_launches']                       # (the multi-tick launches of wave(): FIBHIP_MT_FAKE_GIVEUP counts them)
    return counts, state, fb, stats, marks


@pytest.mark.parametrize('nth', [1, 2, 4, 6])
def test_give_up_with_stimuli_queued_behind_it(gpu_lib, monkeypatch, nth):
    """30 ticks one call each, an event every 5: six five-tick launches, each with a stimulus queued behind it, nothing
    synchronises before the state is read.  Whichever launch gives up, the state and the count are those of the untouched run;
    one launch gave up, every tick is counted once."""
    script = ['begin', ('x', 30), 'mark']
    fired = _run(monkeypatch, {}, script, fire=True)[1]
    for with_add in (False, True):
        _, state, fb0, s0, marks0 = _run(monkeypatch, {}, script + ['count'], with_add)
        assert fb0 == (0, 0) and marks0[0][1] == 6 and s0['ticks'] == 30 and s0['mt_ticks'] == 30, (fb0, marks0, s0)
        assert s0['launches'] == 12, s0
        pcount, pstate, pfb, ps, _ = _run(monkeypatch, {'FIBHIP_MT': '0'}, script + ['count'], with_add)
        assert pstate == state and pfb == (0, 0) and ps['mt_ticks'] == 0 and ps['ticks'] == 30
        assert (state == fired) == (not with_add)             # MAX alone: the run that fires from its loop body; the ADD entry moves it
        # (the count is read AFTER the state here: reading it flushes and would find the give-up first)
        gcount, gstate, fb, s, marks = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script, with_add)
        assert marks[0][0] == (0, 0)                          # (not found before the read: the stimuli were queued behind it)
        assert fb[0] == 1 and fb[1] > 0, (nth, fb)            # (1, ...): one launch gave up and was recovered
        assert gstate == state, (nth, with_add)
        assert s['ticks'] == 30 and s['mt_ticks'] + fb[1] <= 30, (s, fb)       # every tick counted once
        count, cstate, cfb, _, _ = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script + ['count'], with_add)
        assert count == pcount == [6 * (2 if with_add else 1)] and cstate == state and cfb[0] == 1, (count, pcount, cfb)


@pytest.mark.parametrize('entry', ['begin', 'end'])
def test_give_up_in_front_of_begin_and_end(gpu_lib, monkeypatch, entry):
    """stim_begin and stim_end directly behind multi-tick launches nobody has confirmed, the last of which gave up: begin defines
    tick 0 on the recovered state, end leaves no replay that wants the program"""
    script = {'begin': [20, 'mark', 'begin', ('x', 10), 'count'],
              'end': ['begin', ('x', 10), 'mark', 'end', 7, 'begin', ('x', 5), 'count']}[entry]
    for with_add in (False, True):
        want, state, fb0, s0, marks0 = _run(monkeypatch, {}, script, with_add)
        assert fb0 == (0, 0) and marks0[0][1] >= 1, marks0
        for nth in sorted({1, marks0[0][1]}):
            got, gstate, fb, s, marks = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script, with_add)
            assert marks[0][0] == (0, 0) and fb[0] == 1, (entry, nth, marks, fb)
            assert got == want and gstate == state, (entry, nth, with_add)
            assert s['ticks'] == s0['ticks'], (s, s0)
