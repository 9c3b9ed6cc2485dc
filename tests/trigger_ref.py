"""NumPy restatement of the trigger program (include/fibhip.h fibhip_trig_*): a sensor's count, one step of a rule's automaton,
and a whole program run on a state at one sample (the stimuli go through tests/stim_ref.py).  Everything is integer arithmetic
on strict float32 comparisons: the device must equal this bit for bit.

    c = #{cells of the site with X > level}      a = (c >= need)
    row s of a rule = {c, a, t, n, cause, fired} from row s - 1 (the virtual row -1: a = -1, t = -1, n = 0)"""
import numpy as np

import stim_ref

FIELDS = ('c', 'a', 't', 'n', 'cause', 'fired')
VIRTUAL = {'c': 0, 'a': -1, 't': -1, 'n': 0, 'cause': 0, 'fired': 0}
RISE, FALL = 'rise', 'fall'


def site_mask(sensor, H, W):
    """the boolean [H, W] site of a sensor dict (site 'rect' with r0, r1, c0, c1, or 'mask' with `mask`)"""
    if sensor.get('site', 'rect') in ('rect', 0):
        m = np.zeros((H, W), bool)
        m[sensor['r0']:sensor['r1'], sensor['c0']:sensor['c1']] = True
        return m
    return np.asarray(sensor['mask']) != 0


def count(x, site, level):
    """cells of the boolean site with x > level: strict, float32, a NaN does not count"""
    with np.errstate(invalid='ignore'):
        return int(np.count_nonzero((np.asarray(x, np.float32) > np.float32(level)) & site))


def step(rule, prev, s, c, a):
    """one rule, one sample: (rule dict, previous row dict, sample index, count, activity) -> row dict"""
    edge = rule.get('edge', RISE)
    edge = (RISE, FALL)[edge] if isinstance(edge, int) else edge
    arm, blank, escape, max_det = (int(rule.get(k, 0)) for k in ('arm', 'blank', 'escape', 'max_det'))
    delay, period = int(rule.get('delay', 0)), int(rule.get('period', 0))
    cnt, hold = int(rule.get('count', 1)), int(rule.get('hold', 1))
    pa, pt, pn = prev['a'], prev['t'], prev['n']
    e = pa >= 0 and ((pa == 0 and a == 1) if edge == RISE else (pa == 1 and a == 0))
    listen = s >= arm and (max_det == 0 or pn < max_det) and (pt < 0 or pt + 1 >= blank)
    quiet = escape > 0 and listen and ((s - arm if pt < 0 else pt) + 1 >= escape)
    det = listen and (e or quiet)
    cause = (1 if e else 2) if det else 0
    t = 0 if det else (-1 if pt < 0 else pt + 1)
    n = pn + int(det)
    u = t - delay
    fired = t >= 0 and u >= 0 and (u < hold if period == 0 else (u // period < cnt and u % period < hold))
    return {'c': int(c), 'a': int(a), 't': t, 'n': n, 'cause': cause, 'fired': int(fired)}


def run_rule(rule, activity, counts=None):
    """the rows of one rule over a sequence of sensor activities (0 / 1): the automaton on its own"""
    rows, prev = [], VIRTUAL
    for s, a in enumerate(activity):
        prev = step(rule, prev, s, a if counts is None else counts[s], a)
        rows.append(prev)
    return rows


def as_array(rows):
    """[[row dict per rule] per sample] -> int32 [samples, rules, 6]"""
    return np.array([[[r[f] for f in FIELDS] for r in sample] for sample in rows], np.int32).reshape(len(rows), -1, len(FIELDS))


class Program:
    """sensors and rules as the dicts Stepper.trig_begin takes; sample(state) -> the new state, the rows appended to .rows"""

    def __init__(self, sensors, rules, planes, H, W):
        self.sensors, self.rules, self.planes, self.H, self.W = sensors, rules, planes, H, W
        self.sites = [site_mask(q, H, W) for q in sensors]
        self.prev = [VIRTUAL for _ in rules]
        self.rows = []

    def sample(self, state):
        s = len(self.rows)
        cs = [count(state[int(q.get('var', 0))], site, q['level']) for q, site in zip(self.sensors, self.sites)]
        acts = [int(c >= int(q.get('need', 1))) for c, q in zip(cs, self.sensors)]
        row = [step(r, p, s, cs[r['sensor']], acts[r['sensor']]) for r, p in zip(self.rules, self.prev)]
        self.prev = row
        self.rows.append(row)
        state = np.array(state, np.float32, copy=True)
        for r, out in zip(self.rules, row):
            if out['fired']:
                mode = r.get('mode', 'max')
                mode = stim_ref.MODES[mode] if isinstance(mode, int) else mode
                var = int(r.get('var', 0))
                state[var] = stim_ref.apply(state[var], stim_ref.plane_of(r, self.planes, self.H, self.W), mode)
        return state

    def log(self):
        return as_array(self.rows)
