"""tips — spiral-wave tips (phase singularities, rotors) recorded on the device while a model runs, and linked into
trajectories on the host.

A tip is a plaquette of four neighbouring cells around which the state-space phase atan2(B - b0, A - a0) of two state
arrays A = X[var], B = X[var2] winds once; its charge (+1 / -1) is the sense of rotation.  The definition is exact
(include/fibhip.h, fibhip_tips_*; restated in NumPy in tests/tip_ref.py).  `TipRecorder` has the library take the tips
every `every` ticks (`tip_kernel`) and keeps the lists on the device until they are read; `link()` joins the tips of
consecutive samples into trajectories.  No reference counterpart: the reference's drivers look at image() by eye."""
from collections import namedtuple

import numpy as np

from ._recorder import SampledRecorder, attach, check_every, mask_plane, run_capacity, tick_ms

TIP_DTYPE = np.dtype([('t_ms', np.float64), ('y', np.float32), ('x', np.float32), ('charge', np.int32)])
POINT_DTYPE = np.dtype([('t_ms', np.float64), ('y', np.float32), ('x', np.float32)])

Trajectory = namedtuple('Trajectory', ['charge', 'points'])     # points: structured (t_ms, y, x), one per sample it lived


class TipRecorder(SampledRecorder):
    """spiral tips recorded on the device; see `IonicModel.record_tips`.

        with model.record_tips(every=10) as rec:
            for i in model.run():
                ...
            per_sample = rec.tips()              # one structured array (t_ms, y, x, charge) per sample, after ticks 9, 19, ...
            paths = tips.link(per_sample, max_jump=3.0)

    `t_ms` is the model time since the recorder was attached at which the sample was taken: (s + 1) * every ticks of
    `dt_per_step * dt` ms.  `y`, `x` are plaquette centres (row + 0.5, column + 0.5).  At most `max_tips` tips are kept per
    sample (`truncated()` names the samples that had more); `counts()` is exact regardless.  Between two samples the handle
    keeps its multi-tick launches."""
    NOUN, END, COUNT = 'tip recorder', 'tips_end', 'tips_count'

    def __init__(self, model, var2=None, levels=None, every=1, max_tips=256, capacity=None, var=0, mask=None):
        self._st = st = attach(model, 'record_tips', 'spiral tips are recorded')
        signals = getattr(model, 'tip_signals', None)
        if var2 is None or levels is None:
            if signals is None:
                raise ValueError('record_tips: %s has no tip_signals; pass var2 and levels=(a0, b0)' % type(model).__name__)
            if var != signals[0] and levels is None:
                raise ValueError('record_tips: tip_signals gives the level of array %d, not of var=%d; pass levels' % (signals[0], var))
            if var2 is None:
                var2 = signals[1]
            if levels is None:
                if var2 != signals[1]:
                    raise ValueError('record_tips: tip_signals gives the level of array %d, not of var2=%d; pass levels' % (signals[1], var2))
                levels = (signals[2], signals[3])
        self.var, self.var2 = int(var), int(var2)
        self.levels = (float(levels[0]), float(levels[1]))
        self.every = check_every('record_tips', every)
        self.max_tips = int(max_tips)
        self.tick_ms = tick_ms(model)
        self.capacity = int(run_capacity(model, self.every) if capacity is None else capacity)
        self.mask = mask = mask_plane(model, mask, 'record_tips')
        st.tips_begin(self.var, self.var2, self.levels[0], self.levels[1], mask, self.every, self.max_tips, self.capacity)
        self.open = True

    def counts(self, first=0, count=None):
        """int32 [samples, 3]: n_pos, n_neg, stored of every sample taken so far (exact even where the list was cut)"""
        self._check()
        return self._st.tips_read(first, count, records=False)[0]

    def truncated(self):
        """indices of the samples that had more tips than `max_tips`: their lists are cut, their counts are not"""
        return np.flatnonzero(self.counts()[:, 2] > self.max_tips)

    def tips(self, first=0, count=None):
        """a list with one structured array (t_ms, y, x, charge) per sample, sorted by (row, column)"""
        self._check()
        counts, records = self._st.tips_read(first, count)
        out = []
        for s in range(len(counts)):
            r = records[s, :min(int(counts[s, 2]), self.max_tips)]
            r = r[np.lexsort((r[:, 1], r[:, 0]))]
            a = np.empty(len(r), TIP_DTYPE)
            a['t_ms'] = (int(first) + s + 1) * self.every * self.tick_ms
            a['y'] = r[:, 0] + 0.5
            a['x'] = r[:, 1] + 0.5
            a['charge'] = r[:, 2]
            out.append(a)
        return out


def link(tips_per_sample, max_jump):
    """joins the tips of consecutive samples into trajectories: greedy nearest-neighbour matching of tips of EQUAL charge
    within `max_jump` pixels — of all (trajectory alive in the previous sample, tip of this sample) pairs the closest is
    linked first, ties broken by order.  A tip no trajectory reaches starts a new one; a trajectory no tip continues ends.
    `tips_per_sample`: what `TipRecorder.tips()` returns.  Returns a list of `Trajectory(charge, points)` in order of first
    appearance, `points` a structured array (t_ms, y, x)."""
    done, alive = [], []                                      # a trajectory in the making: [serial, charge, [points]]
    serial = 0
    for tips in tips_per_sample:
        tips = np.asarray(tips)
        pairs = []
        for ti, tr in enumerate(alive):
            _, y, x = tr[2][-1]
            for k in np.flatnonzero(tips['charge'] == tr[1]):
                d = float(np.hypot(float(tips['y'][k]) - y, float(tips['x'][k]) - x))
                if d <= max_jump:
                    pairs.append((d, ti, int(k)))
        pairs.sort()
        used_tr, used_tip, nxt = set(), set(), []
        for d, ti, k in pairs:
            if ti in used_tr or k in used_tip:
                continue
            used_tr.add(ti)
            used_tip.add(k)
            alive[ti][2].append((float(tips['t_ms'][k]), float(tips['y'][k]), float(tips['x'][k])))
            nxt.append(alive[ti])
        done += [tr for ti, tr in enumerate(alive) if ti not in used_tr]
        for k in range(len(tips)):
            if k not in used_tip:
                nxt.append([serial, int(tips['charge'][k]), [(float(tips['t_ms'][k]), float(tips['y'][k]), float(tips['x'][k]))]])
                serial += 1
        alive = nxt
    return [Trajectory(tr[1], np.array(tr[2], POINT_DTYPE)) for tr in sorted(done + alive, key=lambda tr: tr[0])]
