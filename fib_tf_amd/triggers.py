"""triggers — triggered stimulation: sense a site, decide, fire a stimulus, all on the device.

A `StimulusProgram` (stimulus.py) applies every entry at a tick fixed before the run.  The usual protocols are not like that: an
S2 belongs a fixed delay after the S1 waveback has passed a site, a demand pacer fires when nothing arrived within an escape
interval, an anti-tachycardia burst follows the detection of an arrival.  A `TriggerProgram` closes that loop on the device: a
`Sensor` counts the cells of a site above a level (`sense_kernel`), a `Trigger` is a small automaton that decides from the
sensor's edges (`trigger_kernel`) and its stimulus is applied by a gated variant of `stim_kernel` — every `every` ticks, queued
behind the launch that ends there; between two samples the handle keeps its multi-tick launches.  The
definition is exact integer arithmetic (include/fibhip.h, fibhip_trig_*; restated in NumPy in tests/trigger_ref.py)."""
import numpy as np

from ._lib import MAX_TRIG_RULES, MAX_TRIG_SENSORS, TRIG_EDGES, TRIG_FIELDS, TRIG_MAX_TIME
from ._recorder import DeviceRecorder, attach, run_capacity, tick_ms
from .stimulus import _DEFAULT, Stimulus, check_timing

CAUSES = (None, 'edge', 'escape')


class Sensor:
    """a site watched on the device: the count of its cells with X > level (strict; a NaN does not count), active when the
    count reaches `need`.

    site     what a Stimulus takes: one of pace_rect's names, (r0, r1, c0, c1), ('disc', y, x, r) or a boolean [height, width] array
    level    the level of the comparison, in the array's own units
    need= | frac=      cells above the level that make the sensor active: a number (default 1), or a share of the site's cells
    var      the state array, an index or a name of VAR_NAMES; 0 is the potential"""

    def __init__(self, site, level, need=None, frac=None, var=0):
        if need is not None and frac is not None:
            raise ValueError('Sensor: give need or frac, not both')
        if frac is not None and not 0.0 < float(frac) <= 1.0:
            raise ValueError('Sensor: frac is a share of the site, 0 < frac <= 1 (got %r)' % (frac,))
        if not float(level) == float(level):
            raise ValueError('Sensor: the level must be a number')
        self.site, self.level, self.need, self.frac, self.var = site, float(level), need, frac, var

    def compile(self, model):
        """the dict Stepper.trig_begin takes.  The site goes through Stimulus.shape: one parser for both."""
        if isinstance(self.site, np.ndarray) and self.site.dtype != np.bool_:
            raise ValueError('Sensor: a site is a name, a rectangle, a disc or a boolean array (got an array of %s)' % self.site.dtype)
        probe = Stimulus(self.site, 1.0, at_tick=0, mode='max', floor=None, var=self.var)
        shape = probe.shape(model)
        d = {'var': probe.var_index(model), 'level': self.level}
        if shape[0] == 'rect':
            r0, r1, c0, c1 = shape[1]
            d.update(site='rect', r0=r0, r1=r1, c0=c0, c1=c1)
            cells = (r1 - r0) * (c1 - c0)
        else:
            mask = shape[1] != np.float32(-np.inf)
            cells = int(mask.sum())
            if cells == 0:
                raise ValueError('Sensor: the site holds no cell')
            d.update(site='mask', mask=mask)
        need = 1 if self.need is None else int(self.need)
        if self.frac is not None:
            need = max(1, int(np.ceil(float(self.frac) * cells)))
        if not 1 <= need <= cells:
            raise ValueError('Sensor: need must be 1 .. %d, the cells of the site (got %d)' % (cells, need))
        d['need'] = need
        return d


class Trigger:
    """one rule: a sensor, an edge, its timing and the stimulus it fires.

    sensor                      a Sensor (rules may share one)
    on                          'rise' (the sensor becomes active: an arrival) or 'fall' (it stops being active: the waveback)
    delay_ms= | delay=          from the detection to the first pulse
    blank_ms= | blank=          after a detection further edges are ignored for this long; default: the length of the train
    arm_ms= | arm=              nothing is detected before this time
    escape_ms= | escape=        a detection is forced when none happened for this long (counted from `arm`, then from the last
                                detection); 0: never
    max_detections              0: without limit
    stimulus                    a Stimulus-like site and value: Trigger(..., site=, v=, mode=, floor=, var=) are handed to
                                `Stimulus`; count, period(_ms), hold(_ms) shape the train fired per detection
    Times given in ms go through millisecond_to_step; all times are counted in SAMPLES (`every` ticks), and a time that is not a
    multiple of `every` ticks is a ValueError, not a rounding."""

    TIMES = ('delay', 'blank', 'arm', 'escape', 'period', 'hold')

    def __init__(self, sensor, on='rise', site=None, v=None, mode='max', floor=_DEFAULT, var=0, count=1,
                 max_detections=0, **times):
        if not isinstance(sensor, Sensor):
            raise ValueError('Trigger: sensor must be a Sensor (got %r)' % (sensor,))
        if on not in TRIG_EDGES:
            raise ValueError('Trigger: on is one of %s (got %r)' % (', '.join(TRIG_EDGES), on))
        self.sensor, self.on, self.count, self.max_detections = sensor, on, int(count), int(max_detections)
        self.times = {}
        for name in self.TIMES:
            ms, ticks = times.pop(name + '_ms', None), times.pop(name, None)
            if ms is not None and ticks is not None:
                raise ValueError('Trigger: give %s_ms or %s, not both' % (name, name))
            self.times[name] = ('ms', ms) if ms is not None else ('ticks', ticks)
        if times:
            raise ValueError('Trigger: unknown argument %s' % ', '.join(sorted(times)))
        # (the Stimulus carries the site, v, mode, floor and var — and parses them; its own timing is not used)
        self.stimulus = Stimulus(site, v, at_tick=0, mode=mode, floor=floor, var=var)

    def samples(self, model, name, every):
        """the time `name` in samples"""
        unit, val = self.times[name]
        if val is None:
            return None
        ticks = model.millisecond_to_step(val) if unit == 'ms' else int(val)
        if ticks % every:
            raise ValueError('Trigger: %s = %s %s is %d ticks, not a multiple of every = %d ticks' % (name, val, unit, ticks, every))
        return ticks // every

    def compile(self, model, sensor_index, every, planes, keys):
        t = {name: self.samples(model, name, every) for name in self.TIMES}
        period, hold = t['period'] or 0, 1 if t['hold'] is None else t['hold']
        delay, arm, escape = t['delay'] or 0, t['arm'] or 0, t['escape'] or 0
        check_timing(0, period, self.count, hold)
        if self.count < 1:
            raise ValueError('Trigger: count must be >= 1 (got %d)' % self.count)
        train = delay + (self.count - 1) * period + hold
        blank = train if t['blank'] is None else t['blank']
        if blank < train:
            raise ValueError('Trigger: blank %d is shorter than the train it fires (delay + (count - 1) * period + hold = %d samples): '
                             'a train must not be cut by a new detection' % (blank, train))
        if self.max_detections < 0:
            raise ValueError('Trigger: max_detections must be >= 0')
        for name, val in (('delay', delay), ('blank', blank), ('arm', arm), ('escape', escape), ('period', period), ('hold', hold)):
            if not 0 <= val <= TRIG_MAX_TIME:
                raise ValueError('Trigger: %s = %d samples is outside 0 .. %d' % (name, val, TRIG_MAX_TIME))
        s = self.stimulus
        r = {'sensor': sensor_index, 'edge': self.on, 'arm': arm, 'blank': blank, 'escape': escape, 'max_det': self.max_detections,
             'delay': delay, 'count': self.count, 'period': period, 'hold': hold, 'var': s.var_index(model), 'mode': s.mode}
        shape = s.shape(model)
        if shape[0] == 'rect':
            (r0, r1, c0, c1), v, floor = shape[1:]
            r.update(shape='rect', r0=r0, r1=r1, c0=c0, c1=c1, v=v, floor=floor)
        else:
            key = shape[1].tobytes()
            if key not in keys:
                keys[key] = len(planes)
                planes.append(shape[1])
            r.update(shape='plane', plane=keys[key])
        return r


def compile_program(model, rules, every):
    """[Trigger] -> (sensors, rules, planes): what Stepper.trig_begin takes (rules that name the same Sensor share it)"""
    rules = list(rules)
    if not 1 <= len(rules) <= MAX_TRIG_RULES:
        raise ValueError('trigger_stimuli: 1 .. %d rules (got %d)' % (MAX_TRIG_RULES, len(rules)))
    if int(every) < 1:
        raise ValueError('trigger_stimuli: every must be >= 1 (got %r)' % (every,))
    sensors, index, out, planes, keys = [], {}, [], [], {}
    for i, t in enumerate(rules):
        if not isinstance(t, Trigger):
            raise ValueError('trigger_stimuli: rule %d is not a Trigger (got %r)' % (i, t))
        if id(t.sensor) not in index:
            if len(sensors) == MAX_TRIG_SENSORS:
                raise ValueError('trigger_stimuli: more than %d sensors' % MAX_TRIG_SENSORS)
            index[id(t.sensor)] = len(sensors)
            sensors.append(t.sensor.compile(model))
        out.append(t.compile(model, index[id(t.sensor)], int(every), planes, keys))
    return sensors, out, planes


class TriggerProgram(DeviceRecorder):
    """a trigger program attached to a model's handle; see `IonicModel.trigger_stimuli`.

        with model.trigger_stimuli(s2_on_waveback(probe, 'luq', 1.0, level=0.2, delay_ms=20), every=10) as prog:
            for i in model.run():
                pass                     # nothing to poll: the S2 follows the waveback at the probe
            print(prog.fired())

    Sample s follows tick (s + 1) * every - 1; tick 0 is the first tick after the program was attached."""
    NOUN, END = 'trigger program', 'trig_end'

    def __init__(self, model, rules, every=1, capacity=None):
        self._st = st = attach(model, 'trigger_stimuli', 'a trigger program runs')
        self.triggers, self.every = list(rules), int(every)
        self.sensors, self.rules, self.planes = compile_program(model, self.triggers, self.every)
        self.capacity = int(run_capacity(model, self.every) if capacity is None else capacity)
        self.tick_ms = tick_ms(model)
        st.trig_begin(self.sensors, self.rules, self.planes, every=self.every, capacity=self.capacity)
        self.open = True
        self._kept = None

    def _check(self):
        if self._kept is None:                   # (closed with its log kept: the readers go on)
            super()._check()

    def samples(self):
        """samples taken so far"""
        self._check()
        return self._st.trig_count() if self.open else len(self._kept)

    def rows(self, first=0, count=None):
        """int32 [count, nrules, 6]: c, a, t, n, cause, fired per sample and rule"""
        self._check()
        if not self.open:
            return self._kept[first:None if count is None else first + count]
        return self._st.trig_read(first, count)

    def tick_of(self, s):
        """the loop tick sample s follows"""
        return (int(s) + 1) * self.every - 1

    def log(self):
        """the structured rows: one record per (sample, rule) with the sample, its tick and t_ms, the rule and the row's fields"""
        rows = self.rows()
        dt = np.dtype([('sample', np.int64), ('tick', np.int64), ('t_ms', np.float64), ('rule', np.int32)] + [(f, np.int32) for f in TRIG_FIELDS])
        out = np.zeros(rows.shape[:2], dt)
        s = np.arange(rows.shape[0])[:, np.newaxis]
        out['sample'], out['rule'] = s, np.arange(rows.shape[1])[np.newaxis, :]
        out['tick'] = (s + 1) * self.every - 1
        out['t_ms'] = (out['tick'] + 1) * self.tick_ms
        for i, f in enumerate(TRIG_FIELDS):
            out[f] = rows[:, :, i]
        return out

    def _where(self, field):
        rows = self.rows()
        found = []
        for s, r in zip(*np.nonzero(rows[:, :, TRIG_FIELDS.index(field)])):
            # (a pulse belongs to the last detection: its cause is the cause at the sample where t was 0)
            cause = rows[s - rows[s, r, 2], r, 4] if rows[s, r, 2] >= 0 else 0
            found.append((self.tick_of(s), int(r), CAUSES[int(cause)]))
        return found

    def detections(self):
        """[(tick, rule, cause)]: the detections so far, cause 'edge' or 'escape'"""
        return self._where('cause')

    def fired(self):
        """[(tick, rule, cause)]: every application of a rule's stimulus so far (a held pulse counts once per tick), with the
        cause of the detection it belongs to"""
        return self._where('fired')

    def as_program(self):
        """the `Stimulus` list that replays what fired, open loop: handed to `program_stimuli` on a fresh model (attached at the
        same tick) it leaves the same bytes"""
        out = []
        for tick, r, _ in self.fired():
            s = self.triggers[r].stimulus
            out.append(Stimulus(s.site, s.v, at_tick=tick, mode=s.mode, floor=s.floor, var=s.var))
        return out

    def close(self):
        """detaches the program (the log read so far stays readable)"""
        if self.open:
            self._kept = self._st.trig_read()
            super().close()


# ---- protocols ------------------------------------------------------------------------------------------------------
def s2_on_waveback(probe, s2_site, v, level, delay_ms=0.0, need=None, frac=None, arm_ms=0.0, var=0, **kw):
    """ONE S2 from `s2_site`, `delay_ms` after the waveback passes `probe` (the probe's cells fall back below `level`): the
    cross-field protocol that makes spirals, timed from the wave instead of from a tick found by hand"""
    return [Trigger(Sensor(probe, level, need=need, frac=frac, var=var), on='fall', delay_ms=delay_ms, arm_ms=arm_ms, max_detections=1,
                    site=s2_site, v=v, **kw)]


def demand_pacer(site, v, level, escape_ms, need=None, frac=None, blank_ms=None, var=0, **kw):
    """triggered-plus-escape pacing of `site` (a pacemaker's triggered mode, VVT / AAT): the rule watches the site itself, and a
    detection is either an arrival there (a rise) or the end of `escape_ms` without one, counted from the last detection.  The
    pulse follows EVERY detection — a rule's automaton does not fire by cause.  After an escape it paces tissue nothing reached;
    after an arrival it is delivered into the site the wave has just excited (MAX with `v`: cells of the site still below `v`
    are raised to it), which starts no second wave, and the interval starts again.  So the site is never left longer than
    `escape_ms` without an activation, and no pulse falls into the middle of a sensed cycle.  It is NOT an inhibited pacer: a
    rule that hears an arrival and stays silent is not something one rule can say."""
    sensor = Sensor(site, level, need=need, frac=frac, var=var)
    return [Trigger(sensor, on='rise', escape_ms=escape_ms, blank_ms=blank_ms, site=site, v=v, **kw)]


def burst_on_arrival(probe, site, v, level, n, cycle_ms, delay_ms=0.0, need=None, frac=None, max_detections=1, var=0, **kw):
    """a burst of `n` pulses `cycle_ms` apart from `site`, `delay_ms` after an arrival at `probe`: anti-tachycardia pacing"""
    return [Trigger(Sensor(probe, level, need=need, frac=frac, var=var), on='rise', delay_ms=delay_ms, count=n,
                    period_ms=cycle_ms if n > 1 else None, max_detections=max_detections, site=site, v=v, **kw)]
