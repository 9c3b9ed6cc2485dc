"""-m gpu: every recorder attached at once — electrode, tip, frame, statistics, spectrum and beat recorders, a stimulus program and
a trigger program, with strides that are no multiples of one another — on the smallest Fenton grid that gets multi-tick launches
(the forced 12-tile shape of tests/test_gpu_recovery.py).  The same calls run three ways: as they come, with the second multi-tick
launch giving up (the test switch FIBHIP_MT_FAKE_GIVEUP: nothing is provoked, nothing waits out a bound) and one launch per tick
(FIBHIP_MT=0).  Every read-back and the final state are the same bytes in all three, and on the one tick all eight hooks share
the timeline shows their kernels in hook order: electrode, tip, frame, statistics, spectrum, beat, stimulus, trigger."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref  # noqa: E402
from test_gpu_frames import PLAN_ENV, VARIANT_96x100, wave  # noqa: E402
from test_gpu_stats import model_columns, planes  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402
from test_gpu_triggers_recovery import program  # noqa: E402

pytestmark = pytest.mark.gpu

# strides in ticks; the stimulus program has an event after every 10th tick.  420 is the first tick all of them share
EVERY = dict(el=2, tip=3, fr=4, st=5, sp=6, bt=7, trig=3, stim=10)
SHARED = 420
TICKS = SHARED + 5
EL_RECTS = [(10, 30, 20, 50), (0, 64, 0, 90)]
WINDOW, BLOCK = (2, 94, 4, 100), (2, 3)
NFFT, CHUNK, BINS = 12, 2, [0, 1, 2, 3, 5, 6]
HOOK_ORDER = ['electrode_kernel', 'tip_kernel', 'frame_kernel', 'stats_kernel', 'stats_combine_kernel', 'spectrum_sample_kernel',
              'spectrum_fold_kernel', 'beat_kernel', 'stim_kernel', 'sense_kernel', 'trigger_kernel', 'stim_gated_kernel']


def _tips_bytes(counts, recs):
    """the counters, and of every sample its valid records (in no fixed order on the device: sorted here)"""
    out = [counts.tobytes()]
    for s in range(len(counts)):
        valid = recs[s, :min(int(counts[s, 2]), recs.shape[1])]
        out.append(valid[np.lexsort(valid.T[::-1])].tobytes())
    return b''.join(out)


def _run(monkeypatch, env):
    """-> (read-backs by name, the kernel names of tick SHARED, fallbacks, multi-tick launches before the attach / during the run)"""
    assert all(SHARED % e == 0 for e in EVERY.values()) and SHARED // EVERY['sp'] % CHUNK == 0
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    H, W = m.height, m.width
    rng = np.random.default_rng(11)
    patches = [rng.uniform(-1, 1, (r1 - r0, c1 - c0)).astype(np.float32) for r0, r1, c0, c1 in EL_RECTS]
    plane = rng.uniform(0.9, 1.0, (H, W)).astype(np.float32)
    weight, mask = planes(H, W, 4)
    sensors, rules = program()
    got = {}
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        before = st.launch_stats()['mt_launches']
        st.electrode_begin(0, EL_RECTS, patches, EVERY['el'], TICKS // EVERY['el'] + 1)
        st.tips_begin(0, 1, 0.5, 0.5, mask, EVERY['tip'], 64, TICKS // EVERY['tip'] + 1)
        st.frames_begin(0, WINDOW, BLOCK, 'mean', -0.02, 1.02, plane, 'uint8', EVERY['fr'], None, TICKS // EVERY['fr'] + 1)
        st.stats_begin(model_columns('fenton', m), weight, mask, EVERY['st'], TICKS // EVERY['st'] + 1)
        st.spectrum_begin(0, WINDOW, BLOCK, 'mean', plane, EVERY['sp'], NFFT, spectrum_ref.hann(NFFT), spectrum_ref.twiddles(NFFT), BINS, CHUNK)
        st.beats_begin(0, WINDOW, BLOCK, 'mean', plane, EVERY['bt'], 0.5, 0.1, 2)
        st.stim_begin([dict(var=0, mode='add', shape='rect', r0=40, r1=47, c0=3, c1=12, first=EVERY['stim'] - 1, period=EVERY['stim'], count=0,
                            hold=1, v=0.03125, floor=0.0)])
        st.trig_begin(sensors, rules, every=EVERY['trig'], capacity=TICKS // EVERY['trig'] + 1)
        for _ in range(SHARED - 1):
            st.step(1)
        during = st.launch_stats()['mt_launches'] - before
        st.trace_begin()
        st.step(1)
        names = [e['name'].split('<')[0] for e in st.trace_end()]
        for _ in range(TICKS - SHARED):
            st.step(1)
        got['electrodes'] = st.electrode_read().tobytes()
        got['tips'] = _tips_bytes(*st.tips_read())
        got['frames'] = st.frames_read().tobytes()
        got['statistics'] = st.stats_read().tobytes()
        P, segments = st.spectrum_read()
        got['spectrum'] = P.tobytes() + bytes([segments]) + b''.join(x.tobytes() for x in st.spectrum_peak(0, len(BINS) - 1))
        got['beats'] = b''.join(x.tobytes() for x in st.beats_read() + st.beats_summary(2))
        got['stimuli'] = st.stim_count()
        got['triggers'] = st.trig_read().tobytes()
        got['counts'] = (st.electrode_count(), st.tips_count(), st.frames_count(), st.stats_count(), st.spectrum_count(), st.beats_count(),
                         st.trig_count())
        got['state'] = st.get_state(-1).tobytes()
        fb = st.fallbacks()
    st.close()
    return got, names, fb, before, during


def test_all_recorders_at_once_three_ways(gpu_lib, monkeypatch):
    free, names, fb, before, during = _run(monkeypatch, {})
    assert fb == (0, 0) and during >= 2, (fb, during)
    assert free['counts'] == tuple(TICKS // EVERY[k] if k != 'sp' else (TICKS // EVERY[k], TICKS // EVERY[k] // NFFT)
                                   for k in ('el', 'tip', 'fr', 'st', 'sp', 'bt', 'trig')), free['counts']
    assert free['stimuli'] == TICKS // EVERY['stim']
    # the shared tick: the hooks' kernels in hook order, behind the tick's own launches
    hooks = [n for n in names[names.index('electrode_kernel'):] if n != 'electrode_combine_kernel']
    print('tick %d:' % SHARED, names)
    assert hooks == HOOK_ORDER, names
    plain, _, pfb, _, pduring = _run(monkeypatch, {'FIBHIP_MT': '0'})
    assert pfb == (0, 0) and pduring == 0
    gave_up, gnames, gfb, gbefore, _ = _run(monkeypatch, {'FIBHIP_MT_FAKE_GIVEUP': str(before + 2)})
    assert gbefore == before and gfb[0] == 1 and gfb[1] > 0, (gfb, before, gbefore)
    assert gnames == names
    for what, run in (('one launch per tick', plain), ('the second multi-tick launch gave up', gave_up)):
        for key, want in free.items():
            assert run[key] == want, '%s: %s differs from the run as it comes' % (what, key)
