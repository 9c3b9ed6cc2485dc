"""stimulus — pacing protocols run on the device: stimuli at programmed ticks, from sites of any shape.

The reference's only stimulus is add_pace_op / fire_op (ionic.py:125-169): one of eight named rectangles, `pot = max(pot, s)`,
fired when the caller's loop body says so — `if i == s2: model.fire_op('s2')`, one host round trip per stimulus.  A
`StimulusProgram` hands the whole protocol to the library at once: S1 trains, S1-S2 scans, bursts, a point stimulus next to a
hole, a stimulus held for a few milliseconds.  The library applies each entry right after its tick (`stim_kernel`), queued on the
stream behind the launch that ends there; between two stimuli the handle keeps its multi-tick launches.
The definition is exact (include/fibhip.h, fibhip_stim_*; restated in NumPy in tests/stim_ref.py).  add_pace_op and fire_op
stay as they are."""
import math

import numpy as np

from ._lib import MAX_STIM_ENTRIES, MAX_STIM_PLANES, STIM_MODES
from ._recorder import DeviceRecorder, array_index, attach, tick_ms

_DEFAULT = object()


def untouched(mode):
    """the value of S that leaves a cell as it is: -inf under 'max', 0 under 'add'"""
    return -math.inf if mode == 'max' else 0.0


class Stimulus:
    """one entry of a program.

    site     one of pace_rect's names ('left', 'luq', ...), a tuple (r0, r1, c0, c1), a disc ('disc', y, x, r) — the cells
             within r of row y, column x —, a boolean [height, width] array, or a float [height, width] array that IS the
             plane S (v is then not given)
    v        the stimulus value on the site
    at_ms= | at_tick=          the first event follows tick at_tick of the loop (`for i in model.run()`: i == at_tick)
    period_ms= | period=       the train's cycle length; None or 0: one event
    count    events of the train (0 with a period: without end)
    hold_ms= | hold=           ticks in a row the stimulus is applied at each event (>= 1, <= period)
    mode     'max': X = max(X, S), fire_op's operation; 'add': X = X + S
    floor    the value of S off the site: 'min_v' (the model's: what fire_op does — the whole grid is floored), a number, or
             None: off the site nothing is touched.  Default: 'min_v' under 'max', None under 'add'.
    var      the state array, an index or a name of VAR_NAMES; 0 is the potential"""

    def __init__(self, site, v=None, at_ms=None, at_tick=None, period_ms=None, period=None, count=1, hold_ms=None, hold=1, mode='max',
                 floor=_DEFAULT, var=0):
        if (at_ms is None) == (at_tick is None):
            raise ValueError('Stimulus: give at_ms or at_tick (one of them)')
        if period_ms is not None and period is not None:
            raise ValueError('Stimulus: give period_ms or period, not both')
        if hold_ms is not None and hold != 1:
            raise ValueError('Stimulus: give hold_ms or hold, not both')
        if mode not in STIM_MODES:
            raise ValueError('Stimulus: mode is one of %s (got %r)' % (', '.join(STIM_MODES), mode))
        self.site, self.v, self.mode, self.var = site, v, mode, var
        self.at_ms, self.at_tick, self.period_ms, self.period = at_ms, at_tick, period_ms, period
        self.count, self.hold_ms, self.hold = count, hold_ms, hold
        self.floor = ('min_v' if mode == 'max' else None) if floor is _DEFAULT else floor

    # ---- timing ---------------------------------------------------------------------------------------------------
    def timing(self, model):
        """(first, period, count, hold) in ticks: milliseconds go through millisecond_to_step (the model's dt_per_step)"""
        first = int(self.at_tick) if self.at_tick is not None else model.millisecond_to_step(self.at_ms)
        if self.period_ms is not None:
            period = model.millisecond_to_step(self.period_ms)
            if period < 1:
                raise ValueError('Stimulus: a period of %g ms is less than one tick' % self.period_ms)
        else:
            period = int(self.period or 0)
        hold = max(1, model.millisecond_to_step(self.hold_ms)) if self.hold_ms is not None else int(self.hold)
        return check_timing(first, period, int(self.count), hold)

    # ---- site -----------------------------------------------------------------------------------------------------
    def shape(self, model):
        """('rect', (r0, r1, c0, c1), v, floor) or ('plane', S): the site on the model's grid"""
        H, W = model.height, model.width
        mode, site = self.mode, self.site
        floor = self.floor
        if isinstance(floor, str):
            if floor != 'min_v':
                raise ValueError("Stimulus: floor is 'min_v', a number or None (got %r)" % floor)
            floor = float(model.min_v)
        elif floor is None:
            floor = untouched(mode)
        else:
            floor = float(floor)
        rect = None
        if isinstance(site, str):
            rect = model.pace_rect(site)
            if rect is None:
                raise ValueError('Stimulus: unknown pacing site %r' % site)
        elif isinstance(site, (tuple, list)) and len(site) == 4 and site[0] == 'disc':
            _, y, x, r = site
            rows = np.arange(H)[:, np.newaxis] - float(y)
            cols = np.arange(W)[np.newaxis, :] - float(x)
            site = np.hypot(rows, cols) <= float(r)
            if not site.any():
                raise ValueError('Stimulus: the disc %r holds no cell of the %d x %d grid' % (self.site, H, W))
        elif isinstance(site, (tuple, list)) and len(site) == 4:
            rect = tuple(int(a) for a in site)
        if rect is not None:
            r0, r1, c0, c1 = rect
            if r0 < 0 or r1 > H or c0 < 0 or c1 > W or r0 >= r1 or c0 >= c1:
                raise ValueError('Stimulus: rows [%d, %d) x columns [%d, %d) is empty or outside the %d x %d grid' % (r0, r1, c0, c1, H, W))
            if self.v is None or not math.isfinite(float(self.v)):
                raise ValueError('Stimulus: v must be a finite number (got %r)' % (self.v,))
            return ('rect', rect, float(self.v), floor)
        a = np.asarray(site)
        if a.shape != (H, W):
            raise ValueError('Stimulus: a site of shape %s on a %d x %d grid' % (a.shape, H, W))
        if a.dtype == np.bool_:
            if self.v is None or not math.isfinite(float(self.v)):
                raise ValueError('Stimulus: v must be a finite number (got %r)' % (self.v,))
            return ('plane', np.where(a, np.float32(self.v), np.float32(floor)).astype(np.float32))
        if self.v is not None:
            raise ValueError('Stimulus: a float array IS the plane S: v must not be given')
        return ('plane', np.ascontiguousarray(a, np.float32))

    def var_index(self, model):
        return array_index(model.VAR_NAMES, self.var, 'Stimulus')


def check_timing(first, period, count, hold):
    if first < 0:
        raise ValueError('Stimulus: the first event follows tick %d: must be >= 0 (a stimulus before any tick is fire_op\'s job)' % first)
    if hold < 1:
        raise ValueError('Stimulus: hold must be >= 1 (got %d)' % hold)
    if period < 0 or count < 0:
        raise ValueError('Stimulus: period and count must be >= 0 (got %d, %d)' % (period, count))
    if period == 0 and count != 1:
        raise ValueError('Stimulus: without a period there is one event: count must be 1 (got %d)' % count)
    if period > 0 and hold > period:
        raise ValueError('Stimulus: hold %d > period %d' % (hold, period))
    return first, period, count, hold


def plane_box(plane, mode):
    """(r0, r1, c0, c1) of the cells of `plane` that are not "untouched" — the box the library visits — or (0, 0, 0, 0)"""
    hit = ~(np.asarray(plane, np.float32) == np.float32(untouched(mode)))
    if not hit.any():
        return (0, 0, 0, 0)
    rows, cols = np.flatnonzero(hit.any(axis=1)), np.flatnonzero(hit.any(axis=0))
    return (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1)


def compile_program(model, stimuli):
    """[Stimulus] -> (entries, planes): the dicts Stepper.stim_begin takes and the planes they index (equal planes are shared)"""
    stimuli = list(stimuli)
    if not 1 <= len(stimuli) <= MAX_STIM_ENTRIES:
        raise ValueError('program_stimuli: 1 .. %d entries (got %d)' % (MAX_STIM_ENTRIES, len(stimuli)))
    entries, planes, keys = [], [], {}
    for i, s in enumerate(stimuli):
        if not isinstance(s, Stimulus):
            raise ValueError('program_stimuli: entry %d is not a Stimulus (got %r)' % (i, s))
        first, period, count, hold = s.timing(model)
        e = {'var': s.var_index(model), 'mode': s.mode, 'first': first, 'period': period, 'count': count, 'hold': hold}
        shape = s.shape(model)
        if shape[0] == 'rect':
            (r0, r1, c0, c1), v, floor = shape[1:]
            e.update(shape='rect', r0=r0, r1=r1, c0=c0, c1=c1, v=v, floor=floor)
        else:
            key = shape[1].tobytes()
            if key not in keys:
                if len(planes) == MAX_STIM_PLANES:
                    raise ValueError('program_stimuli: entry %d: more than %d different planes' % (i, MAX_STIM_PLANES))
                keys[key] = len(planes)
                planes.append(shape[1])
            e.update(shape='plane', plane=keys[key])
        entries.append(e)
    return entries, planes


def entry_due(e, k):
    """is entry `e` (a dict of compile_program) applied right after tick k?"""
    m = k - e['first']
    if m < 0:
        return False
    if e['period'] == 0:
        return m < e['hold']
    return m % e['period'] < e['hold'] and (e['count'] == 0 or m // e['period'] < e['count'])


def expand(entries, n_ticks):
    """[(tick, entry index)] of the first n_ticks ticks: by tick, entries due after the same tick in program order"""
    return [(k, i) for k in range(int(n_ticks)) for i, e in enumerate(entries) if entry_due(e, k)]


class StimulusProgram(DeviceRecorder):
    """a stimulus program attached to a model's handle; see `IonicModel.program_stimuli`.

        with model.program_stimuli(s1s2('left', 1.0, s1_ms=300, n_s1=5, s2_ms=190, s2_site=('disc', 90, 100, 12))) as prog:
            for i in model.run():
                pass                     # nothing to fire: the library applies each stimulus right after its tick
            print(prog.applied())

    Tick 0 is the first tick after the program was attached.  `events(n)` is the host-side expansion of the program."""
    NOUN, END = 'stimulus program', 'stim_end'

    def __init__(self, model, stimuli):
        self._st = st = attach(model, 'program_stimuli', 'a stimulus program runs')
        self.stimuli = list(stimuli)
        self.entries, self.planes = compile_program(model, self.stimuli)
        self.tick_ms = tick_ms(model)
        st.stim_begin(self.entries, self.planes)
        self.open = True

    def events(self, n_ticks):
        """[(tick, entry index)] the program applies during the first n_ticks ticks (pure Python: no device)"""
        return expand(self.entries, n_ticks)

    def applied(self):
        """events applied since the program was attached"""
        self._check()
        return self._st.stim_count()


# ---- protocols ------------------------------------------------------------------------------------------------------
def s1_train(site, v, period_ms=None, n=1, start_ms=None, period=None, start_tick=None, **kw):
    """n stimuli from `site`, one per cycle length: a basic S1 drive.  Times in ms (period_ms, start_ms) or in ticks (period,
    start_tick); the first one follows tick 0 unless told otherwise"""
    if start_ms is None and start_tick is None:
        start_tick = 0
    return [Stimulus(site, v, at_ms=start_ms, at_tick=start_tick, period_ms=period_ms, period=period, count=n, **kw)]


def s1s2(site, v, s1_ms, n_s1, s2_ms, s2_site=None, s2_v=None, start_ms=0.0, **kw):
    """n_s1 S1 stimuli `s1_ms` apart, then one S2 (from `s2_site`, default the S1 site) `s2_ms` after the LAST S1: one point of a
    scan of the vulnerable window"""
    last = start_ms + (n_s1 - 1) * s1_ms
    return [Stimulus(site, v, at_ms=start_ms, period_ms=s1_ms if n_s1 > 1 else None, count=n_s1, **kw),
            Stimulus(site if s2_site is None else s2_site, v if s2_v is None else s2_v, at_ms=last + s2_ms, **kw)]


def burst(site, v, start_ms, cycle_ms, n, **kw):
    """n stimuli `cycle_ms` apart from `start_ms` on: burst pacing, the way fibrillation is induced"""
    return [Stimulus(site, v, at_ms=start_ms, period_ms=cycle_ms if n > 1 else None, count=n, **kw)]
