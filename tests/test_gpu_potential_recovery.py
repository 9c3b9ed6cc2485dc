"""-m gpu: the potential-map recorder behind multi-tick launches that give up (csrc/sched.inc recover(), the rule above confirm()).
The give-up is the test switch FIBHIP_MT_FAKE_GIVEUP=n — the n-th multi-tick launch finds the give-up word raised and leaves at
its first boundary: nothing waits out a bound, nothing hangs.  The yardstick is the untouched run, byte for byte."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_frames import PLAN_ENV, VARIANT_96x100, wave  # noqa: E402
from test_potential_cpu import table_for  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW, STEP = (3, 90, 2, 100), (2, 3)                      # 44 x 33 sites
NPIX = 44 * 33


def _run(gpu_lib, monkeypatch, env, script):
    """`script`: ints = step(n); ('x', n) = n single-tick calls; 'begin' / 'read' / 'summary' / 'count' / 'end' / 'mark' on a Fenton
    handle at the forced 12-tile shape.  Returns (cubes and summaries read, final state, fallbacks, launch stats since the wave,
    marks)"""
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    weight = np.random.default_rng(4).uniform(0.1, 1, (96, 100)).astype(np.float32)
    table = table_for(5)
    out, marks = [], []
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
                st.pmap_begin(table, weight, WINDOW, STEP, 0, 5, 64)
            elif op == 'read':
                out.append(st.pmap_read().tobytes())
            elif op == 'summary':
                out.append(b''.join(a.tobytes() for a in st.pmap_summary()))
            elif op == 'count':
                out.append(st.pmap_count())
            elif op == 'end':
                st.pmap_end()
            elif op == 'mark':
                marks.append((st.fallbacks(), st.launch_stats()['mt_launches'] - s0['mt_launches']))
        state = st.get_state(-1).tobytes()
        fb, s1 = st.fallbacks(), st.launch_stats()
    st.close()
    stats = {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
    stats.update({k: s1[k] for k in ('ticks_recomputed_after_give_up', 'gave_up_recovered')})
    stats['before'] = s0['mt_launches']                       # (the multi-tick launches of wave(): FIBHIP_MT_FAKE_GIVEUP counts them)
    return out, state, fb, stats, marks


@pytest.mark.parametrize('nth', [1, 2, 4, 6])
def test_give_up_with_samples_queued_behind_it(gpu_lib, monkeypatch, nth):
    """30 ticks one call each, a sample every 5: six five-tick launches, each with a sample queued behind it, nothing synchronises
    before the cube is read.  Whichever launch gives up, the cube, the summary and the state are those of the untouched run and
    every tick is counted once, the replayed ones as plain ticks"""
    script = ['begin', ('x', 30), 'mark', 'read', 'summary', ('x', 10), 'read', 'summary']
    want, state, fb0, s0, marks0 = _run(gpu_lib, monkeypatch, {}, script)
    assert fb0 == (0, 0) and marks0[0][1] == 6 and s0['ticks'] == 40 and s0['mt_ticks'] == 40, (fb0, marks0, s0)
    first = np.frombuffer(want[0], np.float64).reshape(6, NPIX)
    assert all(np.any(first[s] != first[s + 1]) for s in range(5))           # (a wave is under way: the map moves)
    plain, pstate, pfb, ps, _ = _run(gpu_lib, monkeypatch, {'FIBHIP_MT': '0'}, script)
    assert plain == want and pstate == state and pfb == (0, 0) and ps['mt_ticks'] == 0 and ps['ticks'] == 40
    got, gstate, fb, s, marks = _run(gpu_lib, monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script)
    assert marks[0][0] == (0, 0)                              # (not found before the read: the samples were queued behind it)
    assert fb[0] == 1 and fb[1] > 0, fb
    assert got == want and gstate == state, nth
    assert s['ticks'] == 40 and s['mt_ticks'] + fb[1] <= s['ticks'], (s, fb)
    assert s['ticks_recomputed_after_give_up'] == fb[1] and s['gave_up_recovered'] == 1, (s, fb)
    assert len(np.frombuffer(got[2], np.float64)) == 8 * NPIX


@pytest.mark.parametrize('entry', ['begin', 'read', 'summary', 'count', 'end'])
def test_entry_points_behind_an_unconfirmed_launch(gpu_lib, monkeypatch, entry):
    """each entry point directly behind multi-tick launches nobody has confirmed, the last of which gave up: begin defines
    tick 0 on the recovered state, read, summary and count hand out recovered samples, end leaves no replay that wants the
    recorder"""
    script = {'begin': [20, 'mark', 'begin', ('x', 10), 'read', 'summary'],
              'read': ['begin', ('x', 10), 'mark', 'read', ('x', 5), 'read'],
              'summary': ['begin', ('x', 10), 'mark', 'summary', 'read', ('x', 5), 'read', 'summary'],
              'count': ['begin', ('x', 10), 'mark', 'count', 'read', ('x', 5), 'read', 'summary'],
              'end': ['begin', ('x', 10), 'mark', 'end', 7, 'begin', 10, 'read', 'summary']}[entry]
    want, state, fb0, s0, marks0 = _run(gpu_lib, monkeypatch, {}, script)
    assert fb0 == (0, 0) and marks0[0][1] >= 1, marks0
    for nth in sorted({1, marks0[0][1]}):
        got, gstate, fb, s, marks = _run(gpu_lib, monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script)
        assert marks[0][0] == (0, 0) and fb[0] == 1, (entry, nth, marks, fb)
        assert got == want and gstate == state, (entry, nth)
        assert s['ticks'] == s0['ticks'], (s, s0)
