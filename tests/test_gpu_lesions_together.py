"""-m gpu: the lesion program beside everything else — the electrode, tip, frame, statistics, lead, wave, spectrum and beat
recorders, a stimulus program and a trigger program, all on one 64 x 64 Fenton handle, each with a stride of its own.  The final
state and field must be those of the run with the programs alone (no recorder's hook disturbs the lesions), and the lead
recorder — the one whose kernel reads the handle's phase planes — pins the hook order: its sample ON the event tick sees the old
field, the next one the new field."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lead_ref  # noqa: E402
import lesion_ref as ref  # noqa: E402
import spectrum_ref  # noqa: E402
from test_gpu_frames import PLAN_ENV, wave  # noqa: E402
from test_gpu_leads import compare, positions, tables_for  # noqa: E402
from test_gpu_leads_together import BINS, BLOCK, CHUNK, EL_RECTS, EVERY, NFFT, WINDOW, program  # noqa: E402
from test_gpu_stats import model_columns, planes  # noqa: E402

pytestmark = pytest.mark.gpu

H = W = 64
TICKS = 60
LESIONS = [(('disc', 20, 12, 3), 9), (('disc', 30, 30, 4), 17), (('line', 40, 5, 50, 40, 1.5), 17), (('disc', 55, 55, 2), 35)]


def fenton_with_hole():
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': H, 'width': W, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 1000})
    m.add_hole_to_phase_field(45, 20, 5)
    m.define()
    return m


def entries(m):
    from fib_tf_amd import lesions
    return lesions.compile_program(m, [lesions.Lesion(s, at_tick=t) for s, t in LESIONS])


def _run(monkeypatch, recorders):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    m = fenton_with_hole()
    st = m._stepper
    wave(m, 'fenton')
    rng = np.random.default_rng(11)
    patches = [rng.uniform(-1, 1, (r1 - r0, c1 - c0)).astype(np.float32) for r0, r1, c0, c1 in EL_RECTS]
    plane = rng.uniform(0.9, 1.0, (H, W)).astype(np.float32)
    weight, mask = planes(H, W, 4)
    sensors, rules = program()
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        if recorders:
            st.electrode_begin(0, EL_RECTS, patches, EVERY['el'], TICKS // EVERY['el'] + 1)
            st.tips_begin(0, 1, 0.5, 0.5, mask, EVERY['tip'], 64, TICKS // EVERY['tip'] + 1)
            st.frames_begin(0, WINDOW, BLOCK, 'mean', -0.02, 1.02, plane, 'uint8', EVERY['fr'], None, TICKS // EVERY['fr'] + 1)
            st.stats_begin(model_columns('fenton', m), weight, mask, EVERY['st'], TICKS // EVERY['st'] + 1)
            st.leads_begin(positions(H, W, 16, 4), tables_for(H, W), weight, 0, EVERY['ld'], TICKS // EVERY['ld'] + 1)
            st.spectrum_begin(0, WINDOW, BLOCK, 'mean', plane, EVERY['sp'], NFFT, spectrum_ref.hann(NFFT), spectrum_ref.twiddles(NFFT), BINS, CHUNK)
            st.beats_begin(0, WINDOW, BLOCK, 'mean', plane, EVERY['bt'], 0.5, 0.1, 2)
            waves = m.record_waves(every=8)
        st.stim_begin([dict(var=0, mode='add', shape='rect', r0=40, r1=47, c0=3, c1=12, first=EVERY['stim'] - 1, period=EVERY['stim'], count=0,
                            hold=1, v=0.03125, floor=0.0)])
        st.trig_begin(sensors, rules, every=EVERY['trig'], capacity=TICKS // EVERY['trig'] + 1)
        st.lesion_begin(entries(m))
        for _ in range(TICKS):
            st.step(1)
        out = dict(state=st.get_state(-1).tobytes(), field=st.get_phase().tobytes(), applied=st.lesion_count(), stim=st.stim_count(),
                   trig=st.trig_read().tobytes())
        if recorders:
            out['samples'] = (st.electrode_count(), st.tips_count(), st.frames_count(), st.stats_count(), st.leads_count(), st.spectrum_count()[0],
                              st.beats_count(), len(waves.counts()))
        assert st.fallbacks() == (0, 0)
    st.close()
    return out


def test_state_and_field_equal_the_run_with_the_programs_alone(gpu_lib, monkeypatch):
    together = _run(monkeypatch, True)
    alone = _run(monkeypatch, False)
    assert together['samples'] == tuple(TICKS // EVERY[k] for k in ('el', 'tip', 'fr', 'st', 'ld', 'sp', 'bt')) + (TICKS // 8,)
    assert together['applied'] == alone['applied'] == len(LESIONS) and together['stim'] == alone['stim'] == TICKS // EVERY['stim']
    for key in ('field', 'state', 'trig'):
        assert together[key] == alone[key], key
    m = fenton_with_hole()
    want = ref.apply_sites(m.phase, H, W, [s for s, _ in LESIONS])
    m._stepper.close()
    assert together['field'] == want.tobytes() and np.isfinite(np.frombuffer(together['state'], np.float32)).all()


def test_lead_sample_on_the_event_tick_sees_the_old_field(gpu_lib, monkeypatch):
    """a lead sample every 4 ticks, a lesion after tick 7 — the tick of sample 1: that sample equals the restatement
    (tests/lead_ref.py, within its own float64 summation bound) evaluated with the OLD field, the next one with the NEW field,
    and neither equals the other field's.  This pins the lesion row behind the lead row"""
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    m = fenton_with_hole()
    st = m._stepper
    wave(m, 'fenton')
    old = m.phase.copy()
    site = ('disc', 32, 30, 6)
    new = ref.apply_sites(old, H, W, [site])
    pos, tables = positions(H, W, 8, 4), tables_for(H, W)
    st.leads_begin(pos, tables, None, 0, 4, 4)
    from fib_tf_amd import lesions
    st.lesion_begin(lesions.compile_program(m, [lesions.Lesion(site, at_tick=7)]))
    states = {}
    for i in range(12):
        st.step(1)
        if i in (7, 11):
            states[i] = st.get_state(0)
    rows = st.leads_read()
    assert rows.shape == (3, 8) and st.get_phase().tobytes() == new.tobytes()
    compare(rows[1], states[7], old, None, pos, tables, 'event tick, old field')
    compare(rows[2], states[11], new, None, pos, tables, 'next sample, new field')
    for row, X, phase in ((rows[1], states[7], new), (rows[2], states[11], old)):
        T = lead_ref.terms(X, phase, None, pos, tables)
        other = lead_ref.traces(X, phase, None, pos, tables)
        assert any(abs(row[e] - other[e]) > lead_ref.bound(T[e]) for e in range(len(pos)))      # (the test can tell the fields apart)
    st.close()
