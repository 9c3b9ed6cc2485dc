"""-m gpu: the lead recorder beside everything else — the electrode, tip, frame, statistics, spectrum and beat recorders, a
stimulus program and a trigger program, all on one 64 x 64 Fenton handle, each with a stride of its own.  What every recorder
reads back must be what it reads back when it is the only recorder on the handle (the two programs write the state, so they are
attached in every run): the hooks share a tick without seeing one another."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref  # noqa: E402
from test_gpu_frames import PLAN_ENV, wave  # noqa: E402
from test_gpu_leads import positions, tables_for  # noqa: E402
from test_gpu_stats import model_columns, planes  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402

pytestmark = pytest.mark.gpu

H = W = 64
# strides in ticks; the stimulus program has an event after every 10th tick.  The lead recorder's 9 is nobody else's
EVERY = dict(el=2, tip=3, fr=4, st=5, sp=6, bt=7, ld=9, trig=3, stim=10)
TICKS = 95
EL_RECTS = [(10, 30, 20, 50), (0, 64, 0, 60)]
WINDOW, BLOCK = (2, 62, 4, 64), (2, 3)
NFFT, CHUNK, BINS = 12, 2, [0, 1, 2, 3, 5, 6]
SITE = dict(r0=50, r1=57, c0=48, c1=56)
RECORDERS = ('el', 'tip', 'fr', 'st', 'ld', 'sp', 'bt')


def program():
    sensor = dict(var=0, level=0.5, need=1, site='rect', **SITE)
    stim = dict(var=0, shape='rect', **SITE)
    return [sensor], [dict(stim, sensor=0, edge='rise', escape=2, blank=30, mode='max', v=1.0, floor=0.0),
                      dict(stim, sensor=0, edge='rise', blank=8, delay=1, count=3, period=1, mode='add', v=-0.0625, floor=0.0)]


def _tips_bytes(counts, recs):
    out = [counts.tobytes()]
    for s in range(len(counts)):
        valid = recs[s, :min(int(counts[s, 2]), recs.shape[1])]
        out.append(valid[np.lexsort(valid.T[::-1])].tobytes())
    return b''.join(out)


def _run(monkeypatch, which):
    """the recorders named in `which` and both programs on a fresh handle -> the read-backs by name"""
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    m = fenton(H, W)
    st = m._stepper
    wave(m, 'fenton')
    rng = np.random.default_rng(11)
    patches = [rng.uniform(-1, 1, (r1 - r0, c1 - c0)).astype(np.float32) for r0, r1, c0, c1 in EL_RECTS]
    plane = rng.uniform(0.9, 1.0, (H, W)).astype(np.float32)
    weight, mask = planes(H, W, 4)
    sensors, rules = program()
    got = {}
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        if 'el' in which:
            st.electrode_begin(0, EL_RECTS, patches, EVERY['el'], TICKS // EVERY['el'] + 1)
        if 'tip' in which:
            st.tips_begin(0, 1, 0.5, 0.5, mask, EVERY['tip'], 64, TICKS // EVERY['tip'] + 1)
        if 'fr' in which:
            st.frames_begin(0, WINDOW, BLOCK, 'mean', -0.02, 1.02, plane, 'uint8', EVERY['fr'], None, TICKS // EVERY['fr'] + 1)
        if 'st' in which:
            st.stats_begin(model_columns('fenton', m), weight, mask, EVERY['st'], TICKS // EVERY['st'] + 1)
        if 'ld' in which:
            st.leads_begin(positions(H, W, 64, 4), tables_for(H, W), weight, 0, EVERY['ld'], TICKS // EVERY['ld'] + 1)
        if 'sp' in which:
            st.spectrum_begin(0, WINDOW, BLOCK, 'mean', plane, EVERY['sp'], NFFT, spectrum_ref.hann(NFFT), spectrum_ref.twiddles(NFFT), BINS, CHUNK)
        if 'bt' in which:
            st.beats_begin(0, WINDOW, BLOCK, 'mean', plane, EVERY['bt'], 0.5, 0.1, 2)
        st.stim_begin([dict(var=0, mode='add', shape='rect', r0=40, r1=47, c0=3, c1=12, first=EVERY['stim'] - 1, period=EVERY['stim'], count=0,
                            hold=1, v=0.03125, floor=0.0)])
        st.trig_begin(sensors, rules, every=EVERY['trig'], capacity=TICKS // EVERY['trig'] + 1)
        for _ in range(TICKS):
            st.step(1)
        if 'el' in which:
            got['el'] = (st.electrode_count(), st.electrode_read().tobytes())
        if 'tip' in which:
            got['tip'] = (st.tips_count(), _tips_bytes(*st.tips_read()))
        if 'fr' in which:
            got['fr'] = (st.frames_count(), st.frames_read().tobytes())
        if 'st' in which:
            got['st'] = (st.stats_count(), st.stats_read().tobytes())
        if 'ld' in which:
            got['ld'] = (st.leads_count(), st.leads_read().tobytes())
        if 'sp' in which:
            P, segments = st.spectrum_read()
            got['sp'] = (st.spectrum_count(), P.tobytes() + bytes([segments]) + b''.join(x.tobytes() for x in st.spectrum_peak(0, len(BINS) - 1)))
        if 'bt' in which:
            got['bt'] = (st.beats_count(), b''.join(x.tobytes() for x in st.beats_read() + st.beats_summary(2)))
        got['stim'] = st.stim_count()
        got['trig'] = (st.trig_count(), st.trig_read().tobytes())
        got['state'] = st.get_state(-1).tobytes()
        assert st.fallbacks() == (0, 0)
    st.close()
    return got


def test_every_output_equals_its_solo_run(gpu_lib, monkeypatch):
    together = _run(monkeypatch, RECORDERS)
    assert together['ld'][0] == TICKS // EVERY['ld'] and together['stim'] == TICKS // EVERY['stim']
    assert together['trig'][0] == TICKS // EVERY['trig']
    rows = np.frombuffer(together['ld'][1], np.float64).reshape(TICKS // EVERY['ld'], 64)
    assert np.all(np.isfinite(rows)) and all(len(np.unique(rows[:, e])) > 1 for e in range(64))
    for name in RECORDERS:
        solo = _run(monkeypatch, (name,))
        assert solo[name] == together[name], '%s: its output beside the others differs from its solo run' % name
        for key in ('stim', 'trig', 'state'):
            assert solo[key] == together[key], '%s solo: %s differs' % (name, key)
