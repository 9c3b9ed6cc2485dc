"""-m gpu: the potential-map recorder beside everything else — the electrode, tip, frame, statistics, lead, wave, spectrum and
beat recorders, a stimulus program, a trigger program and a lesion program, all on one 64 x 64 Fenton handle with an obstacle
field, each with a stride of its own.  What every recorder reads back must be what it reads back when it is the only recorder on
the handle (the three programs write the state or the field, so they are attached in every run): the hooks share a tick without
seeing one another.  And the launch order on a shared tick: with the map recorder absent it is what it was, with it attached its
two kernels stand directly behind the lead recorder's."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref  # noqa: E402
from test_gpu_frames import PLAN_ENV, wave  # noqa: E402
from test_gpu_leads import positions, tables_for  # noqa: E402
from test_gpu_leads_together import BINS, BLOCK, CHUNK, EL_RECTS, NFFT, WINDOW, _tips_bytes, program  # noqa: E402
from test_gpu_stats import model_columns, planes  # noqa: E402
from test_potential_cpu import table_for  # noqa: E402

pytestmark = pytest.mark.gpu

H = W = 64
# strides in ticks; the stimulus program has an event after every 10th tick.  The map recorder's 11 is nobody else's
EVERY = dict(el=2, tip=3, fr=4, st=5, sp=6, bt=7, wv=8, ld=9, pm=11, trig=3, stim=10)
TICKS = 95
LESIONS = [(('disc', 20, 12, 3), 9), (('line', 40, 5, 50, 40, 1.5), 43), (('disc', 30, 30, 4), 54)]     # 43 and 54: behind samples of the map
PM_LATTICE = ((1, 64, 0, 63), (3, 2))
RECORDERS = ('el', 'tip', 'fr', 'st', 'ld', 'pm', 'wv', 'sp', 'bt')


def model():
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': H, 'width': W, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 1000})
    m.add_hole_to_phase_field(45, 20, 5)
    m.define()
    return m


def attach(st, m, which, every, ticks):
    """the recorders named in `which`, in an order that is not the hook order, and the three programs"""
    from fib_tf_amd import lesions
    rng = np.random.default_rng(11)
    patches = [rng.uniform(-1, 1, (r1 - r0, c1 - c0)).astype(np.float32) for r0, r1, c0, c1 in EL_RECTS]
    plane = rng.uniform(0.9, 1.0, (H, W)).astype(np.float32)
    weight, mask = planes(H, W, 4)
    sensors, rules = program()
    cap = lambda k: ticks // every[k] + 1  # noqa: E731
    if 'pm' in which:
        st.pmap_begin(table_for(6), weight, PM_LATTICE[0], PM_LATTICE[1], 0, every['pm'], cap('pm'))
    if 'el' in which:
        st.electrode_begin(0, EL_RECTS, patches, every['el'], cap('el'))
    if 'tip' in which:
        st.tips_begin(0, 1, 0.5, 0.5, mask, every['tip'], 64, cap('tip'))
    if 'fr' in which:
        st.frames_begin(0, WINDOW, BLOCK, 'mean', -0.02, 1.02, plane, 'uint8', every['fr'], None, cap('fr'))
    if 'st' in which:
        st.stats_begin(model_columns('fenton', m), weight, mask, every['st'], cap('st'))
    if 'ld' in which:
        st.leads_begin(positions(H, W, 16, 4), tables_for(H, W), weight, 0, every['ld'], cap('ld'))
    if 'wv' in which:
        st.waves_begin(0, 0, 0.5, -1, 0, 0.0, 4, mask, 64, every['wv'], cap('wv'))
    if 'sp' in which:
        st.spectrum_begin(0, WINDOW, BLOCK, 'mean', plane, every['sp'], NFFT, spectrum_ref.hann(NFFT), spectrum_ref.twiddles(NFFT), BINS, CHUNK)
    if 'bt' in which:
        st.beats_begin(0, WINDOW, BLOCK, 'mean', plane, every['bt'], 0.5, 0.1, 2)
    st.stim_begin([dict(var=0, mode='add', shape='rect', r0=40, r1=47, c0=3, c1=12, first=every['stim'] - 1, period=every['stim'], count=0,
                        hold=1, v=0.03125, floor=0.0)])
    st.trig_begin(sensors, rules, every=every['trig'], capacity=cap('trig'))
    st.lesion_begin(lesions.compile_program(m, [lesions.Lesion(s, at_tick=t) for s, t in LESIONS if t < ticks]))


def _waves_bytes(counts, recs):
    out = [counts.tobytes()]
    for s in range(len(counts)):
        valid = recs[s, :min(int(counts[s, 1]), recs.shape[1])]
        out.append(np.sort(valid, order='seed').tobytes())
    return b''.join(out)


def _run(monkeypatch, which):
    """the recorders named in `which` and the three programs on a fresh handle -> the read-backs by name"""
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    m = model()
    st = m._stepper
    wave(m, 'fenton')
    got = {}
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        attach(st, m, which, EVERY, TICKS)
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
        if 'pm' in which:
            got['pm'] = (st.pmap_count(), st.pmap_read().tobytes(), b''.join(a.tobytes() for a in st.pmap_summary()))
        if 'wv' in which:
            got['wv'] = (st.waves_count(), _waves_bytes(*st.waves_read()))
        if 'sp' in which:
            P, segments = st.spectrum_read()
            got['sp'] = (st.spectrum_count(), P.tobytes() + bytes([segments]) + b''.join(x.tobytes() for x in st.spectrum_peak(0, len(BINS) - 1)))
        if 'bt' in which:
            got['bt'] = (st.beats_count(), b''.join(x.tobytes() for x in st.beats_read() + st.beats_summary(2)))
        got['stim'] = st.stim_count()
        got['trig'] = (st.trig_count(), st.trig_read().tobytes())
        got['lesion'] = (st.lesion_count(), st.get_phase().tobytes())
        got['state'] = st.get_state(-1).tobytes()
        assert st.fallbacks() == (0, 0)
    st.close()
    return got


def test_every_output_equals_its_solo_run(gpu_lib, monkeypatch):
    together = _run(monkeypatch, RECORDERS)
    assert together['pm'][0] == TICKS // EVERY['pm'] and together['stim'] == TICKS // EVERY['stim']
    assert together['trig'][0] == TICKS // EVERY['trig'] and together['lesion'][0] == len(LESIONS)
    cube = np.frombuffer(together['pm'][1], np.float64).reshape(TICKS // EVERY['pm'], 21, 32)
    assert np.all(np.isfinite(cube)) and all(np.any(cube[s] != cube[s + 1]) for s in range(len(cube) - 1))
    for name in RECORDERS:
        solo = _run(monkeypatch, (name,))
        assert solo[name] == together[name], '%s: its output beside the others differs from its solo run' % name
        for key in ('stim', 'trig', 'lesion', 'state'):
            assert solo[key] == together[key], '%s solo: %s differs' % (name, key)


def _shared_tick(monkeypatch, which):
    """every stride 1, a lesion behind the second tick: the kernels of that tick, in launch order"""
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    m = model()
    st = m._stepper
    wave(m, 'fenton')
    every = dict.fromkeys(EVERY, 1)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        attach(st, m, which, every, 12)
        st.step(9)
        st.trace_begin()
        st.step(1)                                            # tick 9: the first lesion's
        names = [e['name'].split('<')[0] for e in st.trace_end()]
    st.close()
    return names


# the hooks' kernels in RECORDERS order, as they stood before the map recorder had a row
HOOK_ORDER = ['electrode_kernel', 'electrode_combine_kernel', 'tip_kernel', 'frame_kernel', 'stats_kernel', 'stats_combine_kernel', 'lead_kernel',
              'lead_combine_kernel', 'wave_label_kernel', 'wave_merge_kernel', 'wave_root_kernel', 'wave_reduce_kernel', 'spectrum_sample_kernel',
              'spectrum_fold_kernel', 'beat_kernel', 'stim_kernel', 'trigger_kernel', 'lesion_apply_kernel', 'lesion_prep_kernel']


def test_launch_order_on_a_shared_tick(gpu_lib, monkeypatch):
    without = _shared_tick(monkeypatch, tuple(r for r in RECORDERS if r != 'pm'))
    hooks = [n for n in without if n in HOOK_ORDER]
    assert [n for n in HOOK_ORDER if n in hooks] == hooks and {'lead_combine_kernel', 'wave_label_kernel', 'lesion_apply_kernel'} <= set(hooks), without
    assert not any('pmap' in n for n in without)
    beside = _shared_tick(monkeypatch, RECORDERS)
    i = beside.index('lead_combine_kernel')
    assert beside[i + 1:i + 3] == ['pmap_source_kernel', 'pmap_conv_kernel'], beside
    assert beside[:i + 1] + beside[i + 3:] == without
