"""the trigger program without a device: header and binding agree, the automaton's restatement (tests/trigger_ref.py) on
hand-written sequences with the expected rows written out, the count, and the Python layer (sites, ms -> samples, refusals,
as_program, the protocol helpers)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trigger_ref as ref  # noqa: E402

from fib_tf_amd import _lib, triggers  # noqa: E402
from fib_tf_amd.stimulus import Stimulus  # noqa: E402
from fib_tf_amd.triggers import Sensor, Trigger, burst_on_arrival, compile_program, demand_pacer, s2_on_waveback  # noqa: E402

HEADER = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'fibhip.h')).read()


def rows(rule, activity):
    """(t, n, cause, fired) per sample"""
    return [(r['t'], r['n'], r['cause'], r['fired']) for r in ref.run_rule(rule, activity)]


def test_header_and_binding_agree():
    for name in ('fibhip_trig_begin', 'fibhip_trig_count', 'fibhip_trig_read', 'fibhip_trig_end'):
        assert re.search(r'\bint %s\(' % name, HEADER)
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is C.c_int
    assert len(_lib.SYMBOLS['fibhip_trig_begin'][0]) == 10 and _lib.SYMBOLS['fibhip_trig_begin'][0][9] is C.c_longlong
    for macro, val in (('FIBHIP_MAX_TRIG_SENSORS', _lib.MAX_TRIG_SENSORS), ('FIBHIP_MAX_TRIG_RULES', _lib.MAX_TRIG_RULES),
                       ('FIBHIP_TRIG_ROW', len(_lib.TRIG_FIELDS))):
        assert int(re.search(r'#define %s (\d+)' % macro, HEADER).group(1)) == val
    assert re.search(r'#define FIBHIP_TRIG_MAX_TIME \(1 << 24\)', HEADER) and _lib.TRIG_MAX_TIME == 1 << 24
    assert re.search(r'#define FIBHIP_ABI_VERSION 1\b', HEADER)
    for enum, names in (('fibhip_trig_edge', _lib.TRIG_EDGES), ('fibhip_trig_site', _lib.TRIG_SITES), ('fibhip_trig_field', _lib.TRIG_FIELDS)):
        body = re.search(r'enum %s \{([^}]*)\}' % enum, HEADER).group(1)
        got = [(n.strip().split('=')[0].strip(), int(n.split('=')[1])) for n in body.split(',')]
        assert [n.rsplit('_', 1)[1].lower() for n, _ in got] == list(names) and [v for _, v in got] == list(range(len(names)))

    def fields(struct):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), HEADER, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        out = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                typ, names = decl.split(None, 1)
                out += [(n.strip(), C.c_int if typ == 'int' else C.c_float) for n in names.split(',')]
        return out
    assert fields('fibhip_trig_sensor') == list(_lib.TrigSensor._fields_)
    assert fields('fibhip_trig_rule') == list(_lib.TrigRule._fields_)
    assert ref.FIELDS == _lib.TRIG_FIELDS


def test_a_rise():
    assert rows({'edge': 'rise', 'blank': 1}, [0, 0, 1, 1, 0, 1]) == [
        (-1, 0, 0, 0), (-1, 0, 0, 0), (0, 1, 1, 1), (1, 1, 0, 0), (2, 1, 0, 0), (0, 2, 1, 1)]


def test_a_fall():
    assert rows({'edge': 'fall', 'blank': 1}, [1, 1, 0, 0, 1, 0]) == [
        (-1, 0, 0, 0), (-1, 0, 0, 0), (0, 1, 1, 1), (1, 1, 0, 0), (2, 1, 0, 0), (0, 2, 1, 1)]


def test_an_unknown_first_sample_is_not_an_edge():
    """the virtual row has a = -1: active at the first sample is not a rise, inactive is not a fall"""
    assert rows({'edge': 'rise', 'blank': 1}, [1, 1, 0, 1]) == [(-1, 0, 0, 0), (-1, 0, 0, 0), (-1, 0, 0, 0), (0, 1, 1, 1)]
    assert rows({'edge': 'fall', 'blank': 1}, [0, 0, 1, 0]) == [(-1, 0, 0, 0), (-1, 0, 0, 0), (-1, 0, 0, 0), (0, 1, 1, 1)]


def test_an_edge_inside_blank_is_ignored():
    assert rows({'edge': 'rise', 'blank': 4}, [0, 1, 0, 1, 0, 1, 0, 1]) == [
        (-1, 0, 0, 0), (0, 1, 1, 1), (1, 1, 0, 0), (2, 1, 0, 0), (3, 1, 0, 0), (0, 2, 1, 1), (1, 2, 0, 0), (2, 2, 0, 0)]
    # (the rise at sample 3 has p.t + 1 = 3 < 4: ignored; the one at sample 5 has p.t + 1 = 4: heard)


def test_an_escape_detection_counts_from_arm_and_from_the_last_detection():
    assert rows({'edge': 'rise', 'arm': 2, 'escape': 3, 'blank': 1}, [0] * 9) == [
        (-1, 0, 0, 0), (-1, 0, 0, 0), (-1, 0, 0, 0), (-1, 0, 0, 0), (0, 1, 2, 1), (1, 1, 0, 0), (2, 1, 0, 0), (0, 2, 2, 1), (1, 2, 0, 0)]
    # (armed at sample 2: (s - arm) + 1 >= 3 first at s = 4; then p.t + 1 >= 3 at s = 7).  An edge restarts the interval:
    assert rows({'edge': 'rise', 'escape': 3, 'blank': 1}, [0, 1, 0, 0, 0, 0]) == [
        (-1, 0, 0, 0), (0, 1, 1, 1), (1, 1, 0, 0), (2, 1, 0, 0), (0, 2, 2, 1), (1, 2, 0, 0)]
    # nothing is heard before `arm`, an edge neither:
    assert rows({'edge': 'rise', 'arm': 3, 'blank': 1}, [0, 1, 0, 1]) == [(-1, 0, 0, 0), (-1, 0, 0, 0), (-1, 0, 0, 0), (0, 1, 1, 1)]


def test_max_det_exhausted():
    assert rows({'edge': 'rise', 'blank': 1, 'max_det': 2, 'escape': 2}, [0, 1, 0, 1, 0, 1, 0, 0]) == [
        (-1, 0, 0, 0), (0, 1, 1, 1), (1, 1, 0, 0), (0, 2, 1, 1), (1, 2, 0, 0), (2, 2, 0, 0), (3, 2, 0, 0), (4, 2, 0, 0)]


def test_a_delay_and_a_train():
    """delay 2, count 3, period 4, hold 2: pulses at t = 2, 3, 6, 7, 10, 11"""
    rule = {'edge': 'rise', 'blank': 12, 'delay': 2, 'count': 3, 'period': 4, 'hold': 2}
    got = rows(rule, [0, 1] + [0, 1] * 8)
    assert [r[0] for r in got] == [-1] + list(range(12)) + [0, 1, 2, 3, 4]
    assert [r[3] for r in got] == [0] + [0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1] + [0, 0, 1, 1, 0]
    assert [r[2] for r in got] == [0, 1] + [0] * 11 + [1] + [0] * 4 and got[-1][1] == 2
    # period 0: one pulse of `hold` samples
    assert [r[3] for r in rows({'edge': 'rise', 'blank': 4, 'delay': 1, 'hold': 3}, [0, 1, 1, 1, 1, 1, 1])] == [0, 0, 1, 1, 1, 0, 0]


def test_the_count_is_strict_ignores_nan_and_need_decides():
    x = np.array([[0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nan, 0.75], [1.0, 0.25, np.inf, -np.inf]], np.float32)
    site = np.ones((2, 4), bool)
    assert ref.count(x, site, 0.5) == 4                       # (0.5 itself and the NaN do not count; +inf does)
    site[1, 0] = False
    assert ref.count(x, site, 0.5) == 3 and ref.count(x, site, np.inf) == 0
    sensors = [dict(var=0, level=0.5, need=3, site='mask', mask=site), dict(var=0, level=0.5, need=4, site='rect', r0=0, r1=2, c0=0, c1=4),
               dict(var=0, level=0.5, need=5, site='rect', r0=0, r1=2, c0=0, c1=4)]
    rules = [dict(sensor=i, edge='rise', blank=1, var=0, mode='add', shape='rect', r0=0, r1=1, c0=0, c1=1, v=1.0, floor=0.0) for i in range(3)]
    p = ref.Program(sensors, rules, None, 2, 4)
    p.sample(x[np.newaxis])
    assert p.log()[0, :, :2].tolist() == [[3, 1], [4, 1], [4, 0]]


class Model:
    """what the Python layer asks of a model"""
    height, width, dt, dt_per_step, min_v, duration = 40, 60, 0.1, 10, -84.0, 100.0
    VAR_NAMES = ('V', 'm', 'h')

    def pace_rect(self, name):
        return {'left': (0, 40, 0, 5), 'luq': (0, 20, 0, 30)}.get(name)

    def millisecond_to_step(self, t):
        return int(t / (self.dt_per_step * self.dt))


def test_sites_go_through_the_stimulus_parser():
    m = Model()
    assert Sensor('left', -40.0).compile(m) == dict(var=0, level=-40.0, site='rect', r0=0, r1=40, c0=0, c1=5, need=1)
    assert Sensor((1, 5, 2, 9), 0.5, frac=0.5, var='h').compile(m) == dict(var=2, level=0.5, site='rect', r0=1, r1=5, c0=2, c1=9, need=14)
    d = Sensor(('disc', 10, 10, 2), 0.0, frac=1.0).compile(m)
    assert d['site'] == 'mask' and d['mask'].sum() == 13 == d['need'] and d['mask'][10, 12] and not d['mask'][11, 12]
    mask = np.zeros((40, 60), bool)
    mask[3, 4:7] = True
    assert Sensor(mask, 0.0, need=2).compile(m)['mask'].tolist() == mask.tolist()
    for bad, word in ((lambda: Sensor('nowhere', 0.0).compile(m), 'unknown pacing site'), (lambda: Sensor((0, 41, 0, 5), 0.0).compile(m), 'outside'),
                      (lambda: Sensor(np.zeros((40, 60), bool), 0.0).compile(m), 'no cell'), (lambda: Sensor(np.zeros((40, 60), np.float32), 0.0).compile(m), 'boolean'),
                      (lambda: Sensor('left', 0.0, need=201).compile(m), 'need'), (lambda: Sensor('left', 0.0, need=0).compile(m), 'need'),
                      (lambda: Sensor('left', 0.0, need=1, frac=0.5), 'not both'), (lambda: Sensor('left', 0.0, frac=0.0), 'frac'),
                      (lambda: Sensor('left', float('nan')), 'number'), (lambda: Sensor('left', 0.0, var='x').compile(m), 'unknown array')):
        with pytest.raises(ValueError, match=word):
            bad()


def test_milliseconds_become_samples_and_refusals():
    m = Model()
    a = Sensor('left', -40.0)
    t = Trigger(a, on='fall', delay_ms=20, blank_ms=100, arm_ms=10, escape_ms=50, site='luq', v=10.0, count=3, period_ms=10, hold=10)
    sensors, rules, planes = compile_program(m, [t, Trigger(a, site=('disc', 5, 5, 2), v=1.0, floor=None)], 10)
    assert len(sensors) == 1 and planes[0].shape == (40, 60) and rules[1]['shape'] == 'plane' and rules[1]['plane'] == 0
    assert rules[0] == dict(sensor=0, edge='fall', arm=1, blank=10, escape=5, max_det=0, delay=2, count=3, period=1, hold=1, var=0, mode='max',
                            shape='rect', r0=0, r1=20, c0=0, c1=30, v=10.0, floor=-84.0)
    assert rules[1]['blank'] == 1 and rules[1]['hold'] == 1 and rules[1]['delay'] == 0     # (blank defaults to the train's length)
    ok = dict(site='luq', v=1.0)
    for bad, word in ((lambda: compile_program(m, [Trigger(a, delay_ms=15, **ok)], 10), 'not a multiple'),
                      (lambda: compile_program(m, [Trigger(a, delay=7, **ok)], 2), 'not a multiple'),
                      (lambda: compile_program(m, [Trigger(a, delay=4, blank=2, **ok)], 1), 'blank'),
                      (lambda: compile_program(m, [Trigger(a, count=3, period=2, blank=4, **ok)], 1), 'blank'),
                      (lambda: compile_program(m, [Trigger(a, count=2, **ok)], 1), 'count must be 1'),
                      (lambda: compile_program(m, [Trigger(a, count=2, period=2, hold=3, **ok)], 1), 'hold'),
                      (lambda: compile_program(m, [Trigger(a, count=0, period=2, **ok)], 1), 'count'),
                      (lambda: compile_program(m, [Trigger(a, max_detections=-1, **ok)], 1), 'max_detections'),
                      (lambda: compile_program(m, [Trigger(a, **ok)] * 9, 1), 'rules'), (lambda: compile_program(m, [], 1), 'rules'),
                      (lambda: compile_program(m, [Trigger(Sensor('left', 0.0), **ok) for _ in range(8)] + [], 0), 'every'),
                      (lambda: compile_program(m, [Stimulus('luq', 1.0, at_tick=0)], 1), 'not a Trigger'),
                      (lambda: Trigger(a, on='up', **ok), 'on is one of'), (lambda: Trigger('left', **ok), 'Sensor'),
                      (lambda: Trigger(a, delay=1, delay_ms=1.0, **ok), 'not both'), (lambda: Trigger(a, wait=3, **ok), 'unknown argument'),
                      (lambda: compile_program(m, [Trigger(a, site='luq')], 1), 'finite')):
        with pytest.raises(ValueError, match=word):
            bad()


class FakeStepper:
    def __init__(self, rows):
        self.rows, self.began = np.asarray(rows, np.int32), None

    def trig_begin(self, sensors, rules, planes, every, capacity):
        self.began = (sensors, rules, planes, every, capacity)

    def trig_count(self):
        return len(self.rows)

    def trig_read(self, first=0, count=None):
        return self.rows[first:None if count is None else first + count]

    def trig_end(self):
        self.began = None


def test_log_detections_fired_and_as_program():
    m = Model()
    rule = {'edge': 'fall', 'blank': 6, 'delay': 1, 'count': 2, 'period': 2, 'escape': 9}
    log = ref.as_array([[r] for r in ref.run_rule(rule, [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])])
    m._stepper = FakeStepper(log)
    t = Trigger(Sensor('left', -40.0), on='fall', blank=12, delay=2, count=2, period=4, escape=18, site='luq', v=10.0)
    prog = triggers.TriggerProgram(m, [t], every=2)
    assert m._stepper.began[3:] == (2, 50) and prog.samples() == 13
    assert prog.detections() == [(5, 0, 'edge'), (23, 0, 'escape')]
    assert prog.fired() == [(7, 0, 'edge'), (11, 0, 'edge'), (25, 0, 'escape')]
    table = prog.log()
    assert table.shape == (13, 1) and table['tick'][2, 0] == 5 and table['t_ms'][2, 0] == 6.0 and table['cause'][2, 0] == 1
    replay = prog.as_program()
    assert [(s.at_tick, s.site, s.v, s.mode, s.floor) for s in replay] == [(7, 'luq', 10.0, 'max', 'min_v'), (11, 'luq', 10.0, 'max', 'min_v'),
                                                                           (25, 'luq', 10.0, 'max', 'min_v')]
    prog.close()
    assert prog.fired()[0] == (7, 0, 'edge')                  # (the log read at close stays readable)


def test_the_protocol_helpers():
    m = Model()
    (s2,) = s2_on_waveback((10, 14, 30, 34), 'luq', 10.0, level=-60.0, delay_ms=20, frac=0.5)
    r = compile_program(m, [s2], 10)[1][0]
    assert (r['edge'], r['delay'], r['max_det'], r['blank'], r['escape']) == ('fall', 2, 1, 3, 0) and s2.sensor.frac == 0.5
    (dp,) = demand_pacer('left', 10.0, level=-40.0, escape_ms=300)
    r = compile_program(m, [dp], 10)[1][0]
    assert (r['edge'], r['escape'], r['max_det'], r['blank'], r['count']) == ('rise', 30, 0, 1, 1)
    assert dp.sensor.site == dp.stimulus.site == 'left'            # (it watches the site it paces)
    # nothing arrives: paced every escape interval.  An arrival is a detection too: the pulse goes into the site the wave has
    # just excited (triggered pacing, as the docstring says) and the interval starts again
    quiet = [x['fired'] for x in ref.run_rule(r, [0] * 70)]
    assert np.flatnonzero(quiet).tolist() == [29, 59]
    heard = [x['fired'] for x in ref.run_rule(r, [0] * 10 + [1] * 5 + [0] * 45)]
    assert np.flatnonzero(heard).tolist() == [10, 40]
    (b,) = burst_on_arrival((10, 14, 30, 34), 'left', 10.0, level=-40.0, n=8, cycle_ms=50, delay_ms=10)
    r = compile_program(m, [b], 10)[1][0]
    assert (r['edge'], r['count'], r['period'], r['delay'], r['blank'], r['max_det']) == ('rise', 8, 5, 1, 1 + 7 * 5 + 1, 1)
