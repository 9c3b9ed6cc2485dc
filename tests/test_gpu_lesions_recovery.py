"""-m gpu: the lesion program behind multi-tick launches that give up (csrc/sched.inc recover(), the rule above confirm()).
A lesion is queued behind its launch without confirming it; lesion_apply_kernel writes nothing once a launch in front of it gave
up, an older lesion stands, and the replay applies the events of the replayed ticks again — and no others.  The give-up is the
test switch FIBHIP_MT_FAKE_GIVEUP=n (the n-th multi-tick launch finds the give-up word raised and leaves at its first boundary):
nothing waits out a bound, nothing hangs.  The yardstick is the untouched run, byte for byte.  Every patch holds factors strictly
between the floor and 1, so a lesion applied twice — or not at all — leaves other bytes in the field."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_frames import PLAN_ENV, VARIANT_96x100  # noqa: E402
from test_gpu_lesions import make  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 96, 100
BOXES = [(10, 40, 3, 30), (20, 60, 10, 50), (0, 12, 0, 9), (50, 96, 60, 100), (30, 31, 40, 41), (5, 90, 2, 20)]


def lesions(first=4, period=5):
    """six lesions, one after every fifth tick; overlapping boxes, factors in [0.5, 0.95]"""
    rng = np.random.default_rng(5)
    return [(first + period * i, b, rng.uniform(0.5, 0.95, (b[1] - b[0], b[3] - b[2])).astype(np.float32)) for i, b in enumerate(BOXES)]


def _run(monkeypatch, env, script):
    """`script`: ints = step(n); ('x', n) = n single-tick calls; 'begin' / 'count' / 'end' / 'apply' / 'phase' / 'mark' on a Fenton
    handle at the forced 12-tile shape.  -> (what 'count' and 'phase' read, final state, final field, fallbacks, stats, marks)"""
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = make('fenton', shape=(H, W))
    st = m._stepper
    st.step(4)
    st.sync()
    read, marks = [], []
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
                st.lesion_begin(lesions())
            elif op == 'count':
                read.append(st.lesion_count())
            elif op == 'end':
                st.lesion_end()
            elif op == 'apply':
                st.lesion_apply((40, 60, 45, 70), np.full((20, 25), 0.75, np.float32))
            elif op == 'phase':
                read.append(st.get_phase().tobytes())
            elif op == 'mark':
                marks.append((st.fallbacks(), st.launch_stats()['mt_launches'] - s0['mt_launches']))
        state = st.get_state(-1).tobytes()
        field = st.get_phase().tobytes()
        fb, s1 = st.fallbacks(), st.launch_stats()
    st.close()
    stats = {k_: s1[k_] - s0[k_] for k_ in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
    stats['before'] = s0['mt_launches']                       # (the multi-tick launches so far: FIBHIP_MT_FAKE_GIVEUP counts them)
    return read, state, field, fb, stats, marks


@pytest.mark.parametrize('nth', [1, 2, 4, 6])
def test_give_up_with_lesions_queued_behind_it(gpu_lib, monkeypatch, nth):
    """30 ticks one call each, a lesion after every fifth: six five-tick launches, each with a lesion queued behind it, nothing
    synchronises before the state is read.  nth = 1: the launch in front of the first lesion; 2, 4, 6: a launch BEHIND lesions
    that stand.  Whichever gives up, the state, the field and the count are those of the untouched run; one launch gave up,
    every tick is counted once, no lesion was applied twice"""
    script = ['begin', ('x', 30), 'mark']
    _, state, field, fb0, s0, marks0 = _run(monkeypatch, {}, script)
    assert fb0 == (0, 0) and marks0[0][1] == 6 and s0['ticks'] == 30 and s0['mt_ticks'] == 30, (fb0, marks0, s0)
    assert s0['launches'] == 6 + 2 * 6, s0
    pread, pstate, pfield, pfb, ps, _ = _run(monkeypatch, {'FIBHIP_MT': '0'}, script + ['count'])
    assert pstate == state and pfield == field and pfb == (0, 0) and ps['mt_ticks'] == 0 and pread == [6]
    _, gstate, gfield, fb, s, marks = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script)
    assert marks[0][0] == (0, 0)                              # (not found before the read: the lesions were queued behind it)
    assert fb[0] == 1 and fb[1] > 0, (nth, fb)                # (1, ...): one launch gave up and was recovered
    assert gfield == field, nth                               # no lesion lost, none applied twice
    assert gstate == state, nth
    assert s['ticks'] == 30 and s['mt_ticks'] + fb[1] <= 30, (s, fb)
    read, cstate, cfield, cfb, _, _ = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script + ['count'])
    assert read == [6] and cstate == state and cfield == field and cfb[0] == 1, (read, cfb)


@pytest.mark.parametrize('entry', ['begin', 'end', 'apply', 'phase'])
def test_give_up_in_front_of_an_entry_point(gpu_lib, monkeypatch, entry):
    """lesion_begin, lesion_end, lesion_apply and get_phase directly behind multi-tick launches nobody has confirmed, the last of
    which gave up: begin defines tick 0 on the recovered state, end leaves no replay that wants the program, apply writes behind
    a confirmed stream, get_phase hands out the field of the replayed run"""
    script = {'begin': [20, 'mark', 'begin', ('x', 10), 'count'],
              'end': ['begin', ('x', 10), 'mark', 'end', 7, 'begin', ('x', 5), 'count'],
              'apply': ['begin', ('x', 12), 'mark', 'apply', ('x', 8), 'count'],
              'phase': ['begin', ('x', 12), 'mark', 'phase', ('x', 8), 'count']}[entry]
    want, state, field, fb0, s0, marks0 = _run(monkeypatch, {}, script)
    assert fb0 == (0, 0) and marks0[0][1] >= 1, marks0
    for nth in sorted({1, marks0[0][1]}):
        got, gstate, gfield, fb, s, marks = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script)
        assert marks[0][0] == (0, 0) and fb[0] == 1, (entry, nth, marks, fb)
        assert got == want and gstate == state and gfield == field, (entry, nth)
        assert s['ticks'] == s0['ticks'], (s, s0)
