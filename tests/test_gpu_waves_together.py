"""-m gpu: the wave recorder beside everything else — the electrode, tip, frame, statistics, lead, spectrum and beat recorders, a
stimulus program and a trigger program, all on one 64 x 64 Fenton handle, each with a stride of its own.  What every recorder
reads back must be what it reads back when it is the only recorder on the handle (the two programs write the state, so they are
attached in every run), and what the wave recorder reads back must be the NumPy restatement of the states at its sample ticks."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref  # noqa: E402
import wave_ref as ref  # noqa: E402
from test_gpu_frames import PLAN_ENV, wave  # noqa: E402
from test_gpu_leads import positions, tables_for  # noqa: E402
from test_gpu_leads_together import BINS, BLOCK, CHUNK, EL_RECTS, NFFT, WINDOW, _tips_bytes, program  # noqa: E402
from test_gpu_stats import model_columns, planes  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402

pytestmark = pytest.mark.gpu

H = W = 64
# strides in ticks; the stimulus program has an event after every 10th tick.  The wave recorder's 11 is nobody else's
EVERY = dict(el=2, tip=3, fr=4, st=5, sp=6, bt=7, ld=9, wv=11, trig=3, stim=10)
TICKS = 95
RECORDERS = ('el', 'tip', 'fr', 'st', 'ld', 'wv', 'sp', 'bt')
WAVE = dict(level=0.4, level2=0.3, conn=8, max_waves=64)


def _waves_bytes(counts, records, labels):
    return counts.tobytes() + b''.join(ref.sorted_records(records[s], counts[s, 1]).tobytes() for s in range(len(counts))) + labels.tobytes()


def _run(monkeypatch, which, poll=False):
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
    got = {'polled': []}
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
        if 'wv' in which:
            st.waves_begin(0, 0, WAVE['level'], 1, 1, WAVE['level2'], WAVE['conn'], mask, WAVE['max_waves'], EVERY['wv'], TICKS // EVERY['wv'] + 1)
        if 'sp' in which:
            st.spectrum_begin(0, WINDOW, BLOCK, 'mean', plane, EVERY['sp'], NFFT, spectrum_ref.hann(NFFT), spectrum_ref.twiddles(NFFT), BINS, CHUNK)
        if 'bt' in which:
            st.beats_begin(0, WINDOW, BLOCK, 'mean', plane, EVERY['bt'], 0.5, 0.1, 2)
        st.stim_begin([dict(var=0, mode='add', shape='rect', r0=40, r1=47, c0=3, c1=12, first=EVERY['stim'] - 1, period=EVERY['stim'], count=0,
                            hold=1, v=0.03125, floor=0.0)])
        st.trig_begin(sensors, rules, every=EVERY['trig'], capacity=TICKS // EVERY['trig'] + 1)
        for i in range(TICKS):
            st.step(1)
            if poll and (i + 1) % EVERY['wv'] == 0:
                got['polled'].append(st.get_state(-1).copy())
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
        if 'wv' in which:
            counts, records = st.waves_read()
            got['wv'] = (st.waves_count(), _waves_bytes(counts, records, st.waves_labels()))
            got['wv-raw'] = (counts, records, st.waves_labels())
        if 'sp' in which:
            P, segments = st.spectrum_read()
            got['sp'] = (st.spectrum_count(), P.tobytes() + bytes([segments]) + b''.join(x.tobytes() for x in st.spectrum_peak(0, len(BINS) - 1)))
        if 'bt' in which:
            got['bt'] = (st.beats_count(), b''.join(x.tobytes() for x in st.beats_read() + st.beats_summary(2)))
        got['stim'] = st.stim_count()
        got['trig'] = (st.trig_count(), st.trig_read().tobytes())
        got['state'] = st.get_state(-1).tobytes()
        got['mask'] = mask
        assert st.fallbacks() == (0, 0)
    st.close()
    return got


def test_every_output_equals_its_solo_run(gpu_lib, monkeypatch):
    together = _run(monkeypatch, RECORDERS)
    assert together['wv'][0] == TICKS // EVERY['wv'] and together['stim'] == TICKS // EVERY['stim']
    assert together['trig'][0] == TICKS // EVERY['trig'] and together['ld'][0] == TICKS // EVERY['ld']
    for name in RECORDERS:
        solo = _run(monkeypatch, (name,))
        assert solo[name] == together[name], '%s: its output beside the others differs from its solo run' % name
        for key in ('stim', 'trig', 'state'):
            assert solo[key] == together[key], '%s solo: %s differs' % (name, key)
    # the wave recorder's output is the restatement of the states at its sample ticks (a run that reads them back in between)
    polled = _run(monkeypatch, ('wv',), poll=True)
    assert polled['wv'] == together['wv'] and polled['state'] == together['state'] and len(polled['polled']) == TICKS // EVERY['wv']
    counts, records, labels = together['wv-raw']
    cells = []
    for s, X in enumerate(polled['polled']):
        plane = ref.set_plane(X[0], WAVE['level'], 'above', together['mask'], (X[1], 'below', WAVE['level2']))
        want_counts, want_rec, want_lab = ref.sample(plane, WAVE['conn'], WAVE['max_waves'])
        assert counts[s].tolist() == want_counts.tolist() and want_counts[0] <= WAVE['max_waves'], (s, counts[s], want_counts)
        assert ref.sorted_records(records[s], counts[s, 1]).tobytes() == want_rec.tobytes(), s
        if s == len(counts) - 1:
            assert np.array_equal(labels, want_lab)
        cells.append(int(want_counts[2]))
    assert min(cells) > 0 and len(set(cells)) > 1, cells     # (waves are under way)
