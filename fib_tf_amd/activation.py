"""Activation maps recorded on the device: per-cell local activation time, cycle length and action-potential duration
(include/fibhip.h, fibhip_observe_*).

    model.define()
    with model.record_activation() as rec:       # up = 50 %, down = 10 % of [min_v, max_v] (APD90)
        for i in model.run():
            ...
        maps = rec.maps()                        # first_up, last_up, prev_up, apd (ms since attach), count
    cl = maps['last_up'] - maps['prev_up']       # the last cycle length of every cell

After every tick the library compares the watched array before and after the tick and updates the maps where a threshold
was crossed (linear interpolation inside the tick); nothing is copied to the host until `maps()`.  While a recorder is
attached every tick is its own launch (no multi-tick launches, no run-ahead): DESIGN.md §9 gives the cost.
"""
import numpy as np

from ._recorder import DeviceRecorder, attach

MAPS = ('first_up', 'last_up', 'prev_up', 'apd', 'count')


def default_thresholds(min_v, max_v):
    """(up, down): the 0.5 level of [min_v, max_v] that IonicModel._paint detects wavefronts at, and the 0.1 level (APD90),
    as float32"""
    span = max_v - min_v
    return np.float32(min_v + 0.5 * span), np.float32(min_v + 0.1 * span)


class ActivationRecorder(DeviceRecorder):
    """the recorder attached to one model's handle; see `IonicModel.record_activation`.  close() detaches it (the handle goes
    back to its usual launch plan)"""
    NOUN, END = 'activation recorder', 'observe_end'

    def __init__(self, model, up=None, down=None, var=0):
        self._st = st = attach(model, 'record_activation', 'activation maps are recorded')
        d_up, d_down = default_thresholds(float(model.min_v), float(model.max_v))
        self.up = np.float32(d_up if up is None else up)
        self.down = np.float32(d_down if down is None else down)
        self.var = int(var)
        st.observe_begin(self.var, self.up, self.down)
        self.open = True

    def ticks(self):
        """ticks observed since the recorder was attached"""
        self._check()
        return self._st.observe_ticks()

    def maps(self):
        """{'first_up', 'last_up', 'prev_up', 'apd': [H, W] float32 in ms since attach (NaN: no such event yet),
        'count': [H, W] int32 upstrokes}"""
        self._check()
        return {k: self._st.observe_get(k) for k in MAPS}

    def velocity(self, which='last_up', radius=2, max_dt=20.0, min_cells=None, mask=None):
        """{'nfit': int32, 'gy', 'gx', 'rms': float32}, each [H, W]: the plane fit of fib_tf_amd/velocity.py on the time map
        `which` ('first_up', 'last_up' or 'prev_up'), made on the device — the gradient of activation time in ms per cell, its
        residual and the cells that took part; velocity.speed_of and direction_of turn it into speed and direction.  `mask`:
        [H, W], non-zero where a cell counts"""
        from . import velocity as vel
        self._check()
        if which not in MAPS[:3]:
            raise ValueError("velocity: which is 'first_up', 'last_up' or 'prev_up' (got %r)" % (which,))
        radius, max_dt, min_cells = vel.check_args(radius, max_dt, min_cells, who='velocity')
        return dict(zip(vel.MAPS, self._st.observe_velocity(which, radius, max_dt, min_cells, mask)))


def conduction_velocity(t_map, row, c0, c1):
    """speed of a front crossing columns [c0, c1) of `row`, in pixels per ms: the least-squares slope of column against
    activation time there (`t_map`, e.g. maps()['last_up']), unsigned.  NaN cells are left out; NaN when fewer than two
    remain or the times do not change."""
    t = np.asarray(t_map, np.float64)[row, c0:c1]
    x = np.arange(c0, c1, dtype=np.float64)
    ok = np.isfinite(t)
    if ok.sum() < 2:
        return float('nan')
    t, x = t[ok], x[ok]
    tc = t - t.mean()
    den = float((tc * tc).sum())
    if den == 0.0:
        return float('nan')
    slope = float((tc * (x - x.mean())).sum()) / den      # dx/dt: columns as a function of time
    return abs(slope)
