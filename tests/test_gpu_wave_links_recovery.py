"""-m gpu: the wave recorder's links behind multi-tick launches that give up (csrc/sched.inc recover(), the rule above confirm()).
The give-up is the test switch FIBHIP_MT_FAKE_GIVEUP=n, as in tests/test_gpu_waves_recovery.py.  What is new here: `prev`, the
label plane of the sample before, is carried from sample to sample, and SEVERAL samples can stand unconfirmed behind a launch
that gave up — the two link kernels read the give-up word and leave prev, the table and the slot alone, so the replay takes the
lost samples again, in order, from the plane of the last good one.  The yardstick is the untouched run, byte for byte."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_link_ref as lref  # noqa: E402
import wave_ref as ref  # noqa: E402
from test_gpu_frames import PLAN_ENV, VARIANT_96x100, wave  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_WAVES = 32
MAX_LINKS = 48


def _link_bytes(st):
    lcounts, lrecords = st.waves_links_read()
    return lcounts.tobytes() + b''.join(lref.sorted_links(lrecords[s], lcounts[s, 1]).tobytes() for s in range(len(lcounts)))


def _sample_bytes(st):
    """wave counts and records (sorted by seed), link counts and records (sorted by (prev, seed)) and the label plane"""
    counts, records = st.waves_read()
    recs = b''.join(ref.sorted_records(records[s], counts[s, 1]).tobytes() for s in range(len(counts)))
    return counts.tobytes() + recs + _link_bytes(st) + (st.waves_labels().tobytes() if len(counts) else b'')


def _run(gpu_lib, monkeypatch, env, script):
    """`script`: ints = step(n); ('x', n) = n single-tick calls; 'begin' (waves_begin and waves_links_begin) / 'read' /
    'links_read' / 'labels' / 'count' / 'end' / 'mark' on a Fenton handle at the forced 12-tile shape.  Returns (what was read,
    final state, fallbacks, launch stats since the wave, marks, the link counts of the first read)"""
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    mask = np.random.default_rng(4).uniform(size=(96, 100)) < 0.97
    out, marks, first = [], [], []
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
                st.waves_begin(0, 0, 0.3, 1, 1, 0.9, 8, mask.astype(np.uint8), MAX_WAVES, 5, 64)
                st.waves_links_begin(MAX_LINKS)
            elif op == 'read':
                out.append(_sample_bytes(st))
                if not first:
                    first.append(st.waves_links_read()[0])
            elif op == 'links_read':
                out.append(_link_bytes(st))
            elif op == 'labels':
                out.append(st.waves_labels().tobytes())
            elif op == 'count':
                out.append(st.waves_count())
            elif op == 'end':
                st.waves_end()
            elif op == 'mark':
                marks.append((st.fallbacks(), st.launch_stats()['mt_launches'] - s0['mt_launches']))
        state = st.get_state(-1).tobytes()
        fb, s1 = st.fallbacks(), st.launch_stats()
    st.close()
    stats = {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
    stats.update({k: s1[k] for k in ('ticks_recomputed_after_give_up', 'gave_up_recovered')})
    stats['before'] = s0['mt_launches']                       # (the multi-tick launches of wave(): FIBHIP_MT_FAKE_GIVEUP counts them)
    return out, state, fb, stats, marks, first


@pytest.mark.parametrize('nth', [1, 2, 4, 6])
def test_give_up_with_samples_queued_behind_it(gpu_lib, monkeypatch, nth):
    """30 ticks one call each, a sample every 5 with links: six five-tick launches, each with a sample queued behind it, nothing
    synchronises before the lists are read.  nth = 1 leaves five void samples queued behind the launch that gave up — what a
    double buffer of label planes would get wrong.  Whichever launch gives up, link counts and records, wave samples, label
    plane, state and tick counts are those of the untouched run and of the run without multi-tick launches"""
    script = ['begin', ('x', 30), 'mark', 'read', ('x', 10), 'read']
    want, state, fb0, s0, marks0, first = _run(gpu_lib, monkeypatch, {}, script)
    assert fb0 == (0, 0) and marks0[0][1] == 6 and s0['ticks'] == 40 and s0['mt_ticks'] == 40, (fb0, marks0, s0)
    lcounts = first[0]
    print('link counts of the untouched run: %s' % lcounts.tolist())
    # the untouched run has links, and they differ from sample to sample: waves are under way
    assert lcounts.shape == (6, 4) and lcounts[0].tolist() == [0, 0, 0, 0] and np.all(lcounts[1:, 0] >= 1) and np.all(lcounts[:, 3] == 0)
    assert len(np.unique(lcounts[1:, 2])) >= 3
    plain, pstate, pfb, ps, _, _ = _run(gpu_lib, monkeypatch, {'FIBHIP_MT': '0'}, script)
    assert plain == want and pstate == state and pfb == (0, 0) and ps['mt_ticks'] == 0 and ps['ticks'] == 40
    got, gstate, fb, s, marks, _ = _run(gpu_lib, monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script)
    assert marks[0][0] == (0, 0)                              # (not found before the read: the samples were queued behind it)
    assert fb[0] == 1 and fb[1] > 0, fb
    assert got == want and gstate == state, nth
    assert s['ticks'] == 40 and s['mt_ticks'] + fb[1] <= s['ticks'], (s, fb)
    assert s['ticks_recomputed_after_give_up'] == fb[1] and s['gave_up_recovered'] == 1, (s, fb)


@pytest.mark.parametrize('entry', ['links_begin', 'links_read', 'read', 'labels', 'count', 'end'])
def test_entry_points_behind_an_unconfirmed_launch(gpu_lib, monkeypatch, entry):
    """each entry point directly behind multi-tick launches nobody has confirmed, the last of which gave up.  links_begin needs
    an attached recorder that has seen no tick, so it stands behind waves_begin, which confirms: the pair is what follows the
    launch that gave up, and defines sample 0 (no links) on the recovered state"""
    script = {'links_begin': [20, 'mark', 'begin', ('x', 10), 'read'],
              'links_read': ['begin', ('x', 10), 'mark', 'links_read', 'read', ('x', 5), 'read'],
              'read': ['begin', ('x', 10), 'mark', 'read', ('x', 5), 'read'],
              'labels': ['begin', ('x', 10), 'mark', 'labels', 'read', ('x', 5), 'read'],
              'count': ['begin', ('x', 10), 'mark', 'count', 'read', ('x', 5), 'read'],
              'end': ['begin', ('x', 10), 'mark', 'end', 7, 'begin', 5, 'read']}[entry]
    want, state, fb0, s0, marks0, _ = _run(gpu_lib, monkeypatch, {}, script)
    assert fb0 == (0, 0) and marks0[0][1] >= 1, marks0
    for nth in sorted({1, marks0[0][1]}):
        got, gstate, fb, s, marks, _ = _run(gpu_lib, monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(s0['before'] + nth)}, script)
        assert marks[0][0] == (0, 0) and fb[0] == 1, (entry, nth, marks, fb)
        assert got == want and gstate == state, (entry, nth)
        assert s['ticks'] == s0['ticks'], (s, s0)
