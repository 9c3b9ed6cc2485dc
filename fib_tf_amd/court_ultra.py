"""court_ultra — the single-rate research variant of the Courtemanche model
(siravan/fib_tf `court_ultra.py:32-559`): every tick assigns ALL state variables with dt
(`court_ultra.py:107-111,127-128`) instead of court.py's fast/slow split, `fire_op('slow')` is an empty
op there (`court_ultra.py:110`), and run states are checkpointed with `np.save(name, m.state)` /
`np.load(name).item(0)` (`court_ultra.py:511,518`).

Device side: the same kernel as court.py instantiated with `MODE_ALL` (flag FIBHIP_ALLVARS).
`config['ultra_slow'] = True` adds the 22nd array `_us_`, an ultra-slow gate that scales i_Na
(`court_ultra.py:81-82,198-199,221-222,445-450`): device model `CourtemancheUS` (FIBHIP_COURT_US)."""
from functools import partial

import numpy as np

from . import _lib
from .court import INITIAL, Courtemanche as _Courtemanche


class _InterVar:
    """`m._Inter[key].eval()` (court_ultra.py:113,475-479): the intermediate evaluated on the current V"""

    def __init__(self, model, key):
        self._model, self._key = model, key

    def eval(self):
        return self._model.calc_inter(self._model._V.eval())[self._key]


class Courtemanche(_Courtemanche):
    # record_tips() defaults (var, var2, a0, b0), as in court.py: V against _j_ (normalised loop area 0.79; _xr_ 0.57).  From
    # the parity oracle on the CPU, this variant's golden protocol (tests/golden/court_ultra_traj: 48 x 56, diff 1.5, holes
    # (28, 24, 5) and (28, 24, 22, neg), single rate, S1 only), cell (row 24, column 12) over 5000 ticks: V in
    # [-80.0922318, 39.8651848] mV, _j_ in [9.99999975e-06, 0.969333589]; each level is the midpoint.
    tip_signals = (0, 4, -20.1135235, 0.484671795)

    def __init__(self, props):
        super().__init__(props)
        self.ultra_slow = bool(getattr(self, 'ultra_slow', False))
        if self.ultra_slow:                                    # instance-level: the 22-array model
            self.MODEL_ID = _lib.COURT_US
            self.VAR_NAMES = tuple(n for n, _ in INITIAL) + ('_us_',)

    def _flags(self):
        return super()._flags() | _lib.ALLVARS

    def define(self, s1=True, state=None):
        if state is None and self.ultra_slow:
            state = {}
            for name, value in INITIAL:
                self.init_state_variable(state, name, value)
            self.init_state_variable(state, '_us_', 0.72)      # steady state at 500 ms, court_ultra.py:81-82
            if s1:
                state['V'][:, :25] = 20.0
        super().define(s1=s1, state=state)
        self._ops['slow'] = ('call', lambda: None)             # tf.group() of nothing, court_ultra.py:110
        self._Inter = {k: _InterVar(self, k) for k in _lib.COURT_INTER_KEYS}

    def _fire_trend(self):
        # only V, at [width//2, height//8] (court_ultra.py:112-116)
        v = self._stepper.probe(0, self.width // 2, self.height // 8)
        self._Trend.value = np.array([v, 0.0], dtype=np.float32)

    def solve(self, State):
        """one single-rate evaluation of all variables on host arrays (court_ultra.py:134-262)"""
        arrs = np.stack([np.asarray(State[n], np.float32) for n in self.VAR_NAMES])
        st = self._new_stepper(steps_per_tick=1, shard=False)
        try:
            st.set_state(-1, arrs)
            st.step(1)
            res = st.get_state(-1)
        finally:
            st.close()
        return {n: res[i] for i, n in enumerate(self.VAR_NAMES)}


def save_state(path, state):
    """`np.save('state_small', m.state)` of the reference (court_ultra.py:511): a pickled dict name -> array"""
    np.save(path, state, allow_pickle=True)


def load_state(path):
    """`np.load('state_small.npy').item(0)` of the reference (court_ultra.py:518)"""
    if not str(path).endswith('.npy'):
        path = str(path) + '.npy'
    return np.load(path, allow_pickle=True).item(0)


def cl_observer(m, cyclelengths, i0, i, cl):
    """the ϕ-weighted cycle-length observer of court_ultra.py:465-486 (bind with functools.partial)"""
    mean_na = np.average(m._State['_Na_i_'].eval(), weights=m.phase)
    mean_ca = np.average(m._State['_f_Ca_'].eval(), weights=m.phase)
    if m.ultra_slow:
        mean_us = np.average(m._State['_us_'].eval(), weights=m.phase)
        inter = m.calc_inter(m._V.eval())
        mean_us_infinity = np.average(inter['us_infinity'], weights=m.phase)
        mean_tau_us = np.average(inter['tau_us'], weights=m.phase)
        cyclelengths.append([i0 + i, cl, mean_na, mean_ca, mean_us, mean_us_infinity, mean_tau_us])
        print('%d:\t%d\t%.3f\t%.3f\t%.5f\t%.5f\t%.0f' % (i + i0, cl, mean_na, mean_ca, mean_us, mean_us_infinity,
                                                       mean_tau_us))
    else:
        cyclelengths.append([i0 + i, cl, mean_na, mean_ca])
        print('%d:\t%d\t%.3f\t%.3f' % (i + i0, cl, mean_na, mean_ca))


def image_level(m, cutoff):
    """the float32 level L with  image() < cutoff  <=>  V < L  for every float32 V (NaN is in neither): image() is
    (V - lo) / span in float32 (`_frame_levels`), which never decreases with V, so the cells below the cutoff are the cells
    below the smallest V that reaches it.  Found by walking float32 neighbours from lo + cutoff * span."""
    lo, span = (np.float32(v) for v in m._frame_levels())
    cut = np.float32(cutoff)

    def below(v):
        return (np.float32(v) - lo) / span < cut
    L = np.float32(float(lo) + float(cutoff) * float(span))
    while not below(L):
        L = np.nextafter(L, np.float32(-np.inf))
    while below(L):
        L = np.nextafter(L, np.float32(np.inf))
    return float(L)


def record_observables(m, every=1, capacity=None):
    """the reference observer's whole-tissue numbers, recorded on the device every `every` ticks (fib_tf_amd/stats.py) instead
    of polled: the ϕ-weighted means of `_Na_i_` and `_f_Ca_` — and of `_us_` with `ultra_slow` — that `cl_observer`
    (court_ultra.py:465-486) takes from whole arrays read back, ρ (court_ultra.py:504-509: the share of the tissue, phase >
    1e-3, whose image() is below 0.2, -55 mV) as the column 'V_frac_below', and a count of cells that are not finite.
    The observer's two means of FUNCTIONS of V (us_infinity, tau_us) are not recorded: a mean of f(V) is not f of a mean, and
    the recorder takes statistics of state arrays only.  Returns the StatsRecorder (a context manager)."""
    if m.phase is None:
        raise AssertionError('record_observables: the observer weighs with the phase field; this model has none')
    cols = [('_Na_i_', 'mean'), ('_f_Ca_', 'mean')]
    if m.ultra_slow:
        cols.append(('_us_', 'mean'))
    cols += [('V', 'frac_below', image_level(m, 0.2)), ('V', 'nonfinite')]
    return m.record_stats(cols, every=every, weight='phase', mask=np.asarray(m.phase) > 1e-3, capacity=capacity)


def run_small(config, im, cyclelengths, radius=50, i0=0, state_file='state_small'):
    """the two-stage protocol's first stage (court_ultra.py:489-512): annular domain, S1-S2, checkpoint"""
    m = Courtemanche(config)
    m.add_hole_to_phase_field(m.width // 2, m.height // 2, radius)
    m.add_hole_to_phase_field(m.width // 2, m.height // 2, m.width // 2 - 6, neg=True)
    m.define()
    m.add_pace_op('s2', 'luq', 10.0)
    m.cl_observer = partial(cl_observer, m, cyclelengths, i0)
    s2 = m.millisecond_to_step(300)
    for i in m.run(im, keep_state=True, block=False):
        if i % 10 == 0:
            m.fire_op('slow')
        if i == s2:
            m.fire_op('s2')
        if i % 5000 == 0:
            image, phase = m.image(), m.phase
            rho = np.sum(image[phase > 1e-3] < 0.2) / np.sum(phase > 1e-3)     # cutoff -55 mV
            print('ρ = %.4f' % rho)
    save_state(state_file, m.state)
    return m.state


def run_large(config, im, cyclelengths, radius, i0=0, state_file='state_small', out_file='state_large'):
    """second stage (court_ultra.py:514-528): resume the checkpoint around a different obstacle"""
    m = Courtemanche(config)
    m.add_hole_to_phase_field(m.width // 2, m.height // 2, radius)
    m.define(state=load_state(state_file))
    m.cl_observer = partial(cl_observer, m, cyclelengths, i0)
    for i in m.run(im, keep_state=True, block=False):
        if i % 10 == 0:
            m.fire_op('slow')
    save_state(out_file, m.state)
    return m.state
