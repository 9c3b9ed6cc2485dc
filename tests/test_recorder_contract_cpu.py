"""not-gpu: what the twelve recorder and program classes have in common, class by class — the two refusals that come before
anything else in every constructor (no handle yet; a model that runs as row blocks), the `every` check, the default capacity
of a whole run, the closed-recorder message of every reader, close() twice, `with`, and the sample times.  The stepper is a
stand-in that records the calls; no library is loaded."""
from collections import namedtuple

import numpy as np
import pytest

from fib_tf_amd import activation, beats, egm, frames, leads, lesions, spectrum, stats, stimulus, tips, triggers, waves
from fib_tf_amd.sharded import ShardedStepper

H, W = 6, 8
CANNED = {'frames_shape': (3, 4, np.dtype(np.float32)), 'spectrum_shape': (3, 4, 2), 'beats_shape': (3, 4, 5),
          'trig_read': np.zeros((3, 1, 6), np.int32), 'get_phase': np.full((H, W), 0.5, np.float32)}


class StubStepper:
    """records (name, args, kwargs) of every call"""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)

        def call(*a, **kw):
            self.log.append((name, a, kw))
            return CANNED.get(name)
        return call

    def called(self, name):
        return sum(1 for c in self.log if c[0] == name)


class Model:
    VAR_NAMES = ('V', 'g')
    height, width = H, W
    min_v, max_v = 0.0, 1.0
    duration, dt, dt_per_step, diff = 100, 0.1, 10, 1.0
    phase = None

    def __init__(self, stepper):
        self._stepper = stepper

    def millisecond_to_step(self, t):
        return int(t / (self.dt_per_step * self.dt))

    def _frame_levels(self):
        return 0.0, 1.0

    def _image_affine(self):
        return 1.0, 0.0


RECT = (1, 3, 2, 6)
Case = namedtuple('Case', 'cls who clause noun end args kw every readers times')


def case(cls, who, clause, noun, end, args=(), kw=None, every=None, readers=(), times=None):
    return Case(cls, who, clause, noun, end, args, kw or {}, every, readers, times)


def _args(c):
    """the required arguments, made anew (a Trigger keeps its Sensor by identity)"""
    return tuple(a() if callable(a) else a for a in c.args)


EVERY = '%s: every must be >= 1'
CASES = [
    case(activation.ActivationRecorder, 'record_activation', 'activation maps are recorded', 'activation recorder', 'observe_end',
         readers=('ticks', 'maps')),
    case(egm.ElectrodeRecorder, 'record_electrodes', 'electrode traces are recorded', 'electrode recorder', 'electrode_end',
         args=([np.eye(H, W)],), kw={'check_affine': False}, every=EVERY, readers=('count', 'traces')),
    case(tips.TipRecorder, 'record_tips', 'spiral tips are recorded', 'tip recorder', 'tips_end', kw={'var2': 1, 'levels': (0.5, 0.5)},
         every=EVERY, readers=('count', 'counts', 'truncated', 'tips')),
    case(frames.FrameRecorder, 'record_frames', 'frames are recorded', 'frame recorder', 'frames_end', kw={'var': 1}, every=EVERY,
         readers=('count', 'frames', 'times'), times='times'),
    case(stats.StatsRecorder, 'record_stats', 'tissue statistics are recorded', 'statistics recorder', 'stats_end', args=([('V', 'mean')],),
         every=EVERY, readers=('count', 'raw', 'values', 'times', 'table', 'check_finite'), times='times'),
    case(leads.LeadRecorder, 'record_leads', 'electrograms are recorded', 'lead recorder', 'leads_end', args=([(2, 3)], np.ones((H, W))),
         every=EVERY, readers=('count', 'raw', 'traces', ('bipolar', [(0, 0)]), 'times_ms'), times='times_ms'),
    case(waves.WaveRecorder, 'record_waves', 'waves are labelled', 'wave recorder', 'waves_end', kw={'links': True}, every=EVERY,
         readers=('count', 'counts', 'raw', 'truncated', 'waves', 'labels', 'times_ms', 'link_counts', 'links_raw', 'links_truncated',
                  'links', 'events', 'tracks'), times='times_ms'),
    case(spectrum.SpectrumRecorder, 'record_spectrum', 'spectra are recorded', 'spectrum recorder', 'spectrum_end', kw={'nfft': 8},
         every=EVERY, readers=('samples', 'segments', 'raw', 'power', 'peak_maps', 'dominant_frequency')),
    case(beats.BeatRecorder, 'record_beats', 'beats are recorded', 'beat recorder', 'beats_end', every=EVERY,
         readers=('samples', 'raw', 'beats', 'apd', 'di', 'cl', 'restitution', 'summary')),
    case(stimulus.StimulusProgram, 'program_stimuli', 'a stimulus program runs', 'stimulus program', 'stim_end',
         args=(lambda: [stimulus.Stimulus(RECT, 1.0, at_tick=2)],), readers=('applied',)),
    case(triggers.TriggerProgram, 'trigger_stimuli', 'a trigger program runs', 'trigger program', 'trig_end',
         args=(lambda: [triggers.Trigger(triggers.Sensor(RECT, 0.5), site=RECT, v=1.0)],), every='%s: every must be >= 1 (got 0)'),
    case(lesions.LesionProgram, 'program_lesions', 'the geometry changes', 'lesion program', 'lesion_end',
         args=(lambda: [lesions.Lesion(('disc', 3, 4, 1.5), at_tick=2)],), readers=('applied', 'phase')),
]
IDS = [c.cls.__name__ for c in CASES]
WITH_CAPACITY = ('ElectrodeRecorder', 'TipRecorder', 'FrameRecorder', 'StatsRecorder', 'LeadRecorder', 'WaveRecorder', 'TriggerProgram')


def attach(c, **kw):
    st = StubStepper()
    return c.cls(Model(st), *_args(c), **dict(c.kw, **kw)), st


def test_the_table_names_the_twelve_classes():
    assert len(CASES) == len(set(IDS)) == 12


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_refusals_come_first(c):
    """before define() and on row blocks: refused before any argument is looked at (the required ones are None here)"""
    dummies = (None,) * len(c.args)
    with pytest.raises(AssertionError) as e:
        c.cls(Model(None), *dummies)
    assert str(e.value) == '%s should be called after calling define' % c.who
    sharded = ShardedStepper.__new__(ShardedStepper)
    sharded.world = 2
    with pytest.raises(NotImplementedError) as e:
        c.cls(Model(sharded), *dummies)
    assert str(e.value) == '%s: %s on a single device only; this model runs as row blocks over 2 ranks' % (c.who, c.clause)


def test_ablate_refusals():
    with pytest.raises(AssertionError) as e:
        lesions.ablate(Model(None), None)
    assert str(e.value) == 'ablate should be called after calling define'
    sharded = ShardedStepper.__new__(ShardedStepper)
    sharded.world = 2
    with pytest.raises(NotImplementedError) as e:
        lesions.ablate(Model(sharded), None)
    assert str(e.value) == 'ablate: the geometry changes on a single device only; this model runs as row blocks over 2 ranks'
    st = StubStepper()
    m = Model(st)
    assert lesions.ablate(m, ('disc', 3, 4, 1.5)) == st.log[0][1][0] and [c[0] for c in st.log] == ['lesion_apply', 'get_phase']
    assert m.phase is CANNED['get_phase']


@pytest.mark.parametrize('c', [c for c in CASES if c.every], ids=[i for i, c in zip(IDS, CASES) if c.every])
def test_every_must_be_at_least_one(c):
    with pytest.raises(ValueError) as e:
        attach(c, every=0)
    assert str(e.value) == c.every % c.who


@pytest.mark.parametrize('c', [c for c in CASES if c.cls.__name__ in WITH_CAPACITY], ids=WITH_CAPACITY)
def test_default_capacity_is_a_whole_run(c):
    """duration 100 ms in ticks of 1 ms, a sample every 3 ticks: 33 samples; the stepper is handed that number"""
    rec, st = attach(c, every=3)
    begin = st.log[0]
    assert rec.capacity == 33 and type(rec.capacity) is int
    assert begin[0].endswith('_begin') and (begin[2]['capacity'] if 'capacity' in begin[2] else begin[1][-1]) == 33
    rec, st = attach(c, every=300)
    assert rec.capacity == 1                                                  # at least one
    rec, st = attach(c, every=3, capacity=np.int64(5))
    assert rec.capacity == 5 and type(rec.capacity) is int


def test_default_capacity_of_the_frame_recorder_counts_from_first():
    c = CASES[IDS.index('FrameRecorder')]
    for every, first, want in ((3, None, 33), (3, 1, 34), (3, 2, 33), (10, 1, 10), (10, 10, 10), (200, 100, 1), (200, 101, 1)):
        rec, st = attach(c, every=every, first=first)
        assert rec.capacity == want and st.log[0][1][-1] == want, (every, first)
        assert rec.first == (every if first is None else first)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_close_twice_ends_once_and_with_closes(c):
    rec, st = attach(c)
    assert rec.open and st.called(c.end) == 0
    rec.close()
    rec.close()
    assert not rec.open and st.called(c.end) == 1
    rec, st = attach(c)
    with rec as inside:
        assert inside is rec and rec.open
    assert not rec.open and st.called(c.end) == 1
    assert rec.__exit__(None, None, None) is False and st.called(c.end) == 1
    rec, st = attach(c)
    with pytest.raises(KeyError):                                             # (an exception inside the block passes through, after the close)
        with rec:
            raise KeyError('x')
    assert not rec.open and st.called(c.end) == 1


@pytest.mark.parametrize('c', [c for c in CASES if c.readers], ids=[i for i, c in zip(IDS, CASES) if c.readers])
def test_every_reader_of_a_closed_recorder_says_so(c):
    rec, st = attach(c)
    rec.close()
    n = len(st.log)
    for r in c.readers:
        name, a = (r, ()) if isinstance(r, str) else (r[0], r[1:])
        with pytest.raises(AssertionError) as e:
            getattr(rec, name)(*a)
        assert str(e.value) == 'the %s has been closed' % c.noun, name
    assert len(st.log) == n                                                   # nothing reached the stepper


def test_a_closed_trigger_program_keeps_its_log():
    """the one class whose readers go on after close(): the log is read once more before the program is detached"""
    c = CASES[IDS.index('TriggerProgram')]
    rec, st = attach(c)
    rec.close()
    assert [x[0] for x in st.log] == ['trig_begin', 'trig_read', 'trig_end']
    assert rec.samples() == 3 and rec.rows() is not None and rec.rows(1, 1).shape == (1, 1, 6) and len(st.log) == 3
    rec.open, rec._kept = False, None
    with pytest.raises(AssertionError) as e:
        rec.samples()
    assert str(e.value) == 'the trigger program has been closed'


def test_ending_a_lesion_program_updates_the_model():
    c = CASES[IDS.index('LesionProgram')]
    rec, st = attach(c)
    assert lesions.LesionProgram.close is lesions.LesionProgram.end
    rec.end()
    assert [x[0] for x in st.log] == ['lesion_begin', 'lesion_end', 'get_phase'] and rec._model.phase is CANNED['get_phase']


@pytest.mark.parametrize('c', [c for c in CASES if c.times], ids=[i for i, c in zip(IDS, CASES) if c.times])
def test_sample_times(c):
    """sample s of a recorder follows tick (s + 1) * every - 1; frame s of the frame recorder follows tick first + s * every"""
    rec, st = attach(c, every=3)
    n = len(st.log)
    got = getattr(rec, c.times)(2, 3)
    assert rec.tick_ms == float(10 * 0.1) and len(st.log) == n                # (a count that is given asks the stepper nothing)
    want = (3 + (2 + np.arange(3)) * 3) * rec.tick_ms if c.cls is frames.FrameRecorder else (2 + 1 + np.arange(3)) * 3 * rec.tick_ms
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    if c.cls is frames.FrameRecorder:
        rec, st = attach(c, every=3, first=1)
        assert getattr(rec, c.times)(2, 3).tolist() == [7.0, 10.0, 13.0]
    else:
        assert got.tolist() == [9.0, 12.0, 15.0]
    assert getattr(rec, c.times)(2, -1).shape == (0,)
