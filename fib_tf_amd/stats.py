"""stats — whole-tissue statistics recorded on the device while a model runs.

The numbers one plots first for a fibrillation run or a slow ionic drift: weighted means of several state arrays at once,
extremes, the excited or repolarised fraction of the tissue, and a finite check.  The reference's drivers poll them
(court_ultra.py:465-486 reads whole arrays back and takes np.average(..., weights=phase); :504-509 computes the share of the
tissue below -55 mV from one more read-back; ionic.py:208-212 has a NaN detector commented out).  `StatsRecorder` has the
library take them every `every` ticks (`stats_kernel`, `stats_combine_kernel`) into a table of float64 rows kept on the
device until it is read: no read-back and no synchronisation per sample, and between two samples the handle keeps its
multi-tick launches.  The definition is exact (include/fibhip.h, fibhip_stats_*; restated in NumPy
in tests/stats_ref.py)."""
import math
from collections import namedtuple

import numpy as np

from ._lib import MAX_STAT_COLS, MAX_STAT_COLS_PER_ARRAY
from ._recorder import SampledRecorder, array_index, attach, check_every, mask_plane, run_capacity, sample_times, tick_ms, weight_plane

# Python kind -> (device kind, what the host divides the device's value by: None, the sum of the weights, the masked cells)
KINDS = {'sum': ('sum', None), 'min': ('min', None), 'max': ('max', None), 'below': ('below', None), 'above': ('above', None),
         'nonfinite': ('nonfinite', None), 'mean': ('sum', 'weight'), 'frac_below': ('below', 'cells'),
         'frac_above': ('above', 'cells')}
NEED_LEVEL = ('below', 'above', 'frac_below', 'frac_above')

Column = namedtuple('Column', ['var', 'name', 'kind', 'level', 'field'])


def parse_columns(columns, var_names):
    """[(array, kind) or (array, kind, level), ...] -> [Column]: `array` a name of `var_names` or an index into it, `kind` one
    of KINDS, `level` for the kinds that compare.  The field name of a column in `table()` is '<array>_<kind>'; a repeated
    name gets '_2', '_3', ... appended."""
    var_names = tuple(var_names)
    cols = list(columns)
    if not 1 <= len(cols) <= MAX_STAT_COLS:
        raise ValueError('record_stats: 1 .. %d columns (got %d)' % (MAX_STAT_COLS, len(cols)))
    out, per_array, seen = [], {}, {}
    for c in cols:
        if isinstance(c, (str, int)) or not 2 <= len(c) <= 3:
            raise ValueError('record_stats: a column is (array, kind) or (array, kind, level), got %r' % (c,))
        arr, kind = c[0], c[1]
        var = array_index(var_names, arr, 'record_stats')
        if kind not in KINDS:
            raise ValueError('record_stats: unknown kind %r (one of %s)' % (kind, ', '.join(sorted(KINDS))))
        if kind in NEED_LEVEL:
            if len(c) != 3 or c[2] is None or math.isnan(float(c[2])):
                raise ValueError('record_stats: %r needs a level: (%r, %r, level)' % (kind, arr, kind))
            level = float(c[2])
        else:
            if len(c) == 3 and c[2] is not None:
                raise ValueError('record_stats: %r takes no level (got %r)' % (kind, c[2]))
            level = 0.0
        per_array[var] = per_array.get(var, 0) + 1
        if per_array[var] > MAX_STAT_COLS_PER_ARRAY:
            raise ValueError('record_stats: more than %d columns on array %r' % (MAX_STAT_COLS_PER_ARRAY, var_names[var]))
        field = '%s_%s' % (var_names[var], kind)
        seen[field] = seen.get(field, 0) + 1
        if seen[field] > 1:
            field = '%s_%d' % (field, seen[field])
        out.append(Column(var, var_names[var], kind, level, field))
    return out


def device_columns(cols):
    """what Stepper.stats_begin takes: (var, device kind, level) per column"""
    return [(c.var, KINDS[c.kind][0], c.level) for c in cols]


def weight_sum(weight, cells):
    """the divisor of a 'mean': the sum of (double)w over the cells with w != 0, exactly (math.fsum); `cells` without a plane"""
    if weight is None:
        return float(cells)
    w = np.asarray(weight, np.float32).astype(np.float64).ravel()
    return math.fsum(w[w != 0].tolist())


def finish(raw, cols, wsum, cells):
    """the device's rows -> the columns' values: float64 [samples, ncols], 'mean' divided by `wsum`, the fractions by `cells`"""
    out = np.array(raw, np.float64, copy=True).reshape(-1, len(cols))
    with np.errstate(all='ignore'):
        for j, c in enumerate(cols):
            div = KINDS[c.kind][1]
            if div == 'weight':
                out[:, j] = out[:, j] / np.float64(wsum)
            elif div == 'cells':
                out[:, j] = out[:, j] / np.float64(cells)
    return out


def table_dtype(cols):
    return np.dtype([('t_ms', np.float64)] + [(c.field, np.float64) for c in cols])


def make_table(raw, cols, wsum, cells, every, tick_ms, first=0):
    """structured array: t_ms (model time since attach of sample first, first + 1, ...) + one float64 field per column"""
    vals = finish(raw, cols, wsum, cells)
    t = np.empty(len(vals), table_dtype(cols))
    t['t_ms'] = sample_times(first, len(vals), int(every), float(tick_ms))
    for j, c in enumerate(cols):
        t[c.field] = vals[:, j]
    return t


def first_nonfinite(raw, cols, cells):
    """(sample, column) of the first value of `raw` that says the state is not finite, or None: a 'nonfinite' count above
    zero, a sum or mean that is NaN or Inf, a min or max that is infinite although cells were looked at"""
    raw = np.asarray(raw, np.float64).reshape(-1, len(cols))
    for s in range(len(raw)):
        for j, c in enumerate(cols):
            v = raw[s, j]
            dev = KINDS[c.kind][0]
            if (dev == 'nonfinite' and v > 0) or (dev == 'sum' and not np.isfinite(v)) or \
                    (dev in ('min', 'max') and not np.isfinite(v) and cells > 0) or np.isnan(v):
                return s, j
    return None


def check_finite(raw, cols, cells, every, tick_ms, first=0):
    """raises FloatingPointError naming the first sample (and the tick it was taken after) whose row shows a value of the state
    that is not finite"""
    hit = first_nonfinite(raw, cols, cells)
    if hit is not None:
        s, j = hit
        sample = int(first) + s
        tick = (sample + 1) * int(every) - 1
        raise FloatingPointError('the state is not finite: sample %d (after tick %d, t = %g ms since attach), column %s = %r'
                                 % (sample, tick, (tick + 1) * float(tick_ms), cols[j].field, float(np.asarray(raw).reshape(-1, len(cols))[s, j])))


class StatsRecorder(SampledRecorder):
    """tissue statistics recorded on the device; see `IonicModel.record_stats`.

        with model.record_stats([('V', 'mean'), ('_Na_i_', 'mean'), ('V', 'frac_below', -55.0), ('V', 'nonfinite')], every=10) as rec:
            for i in model.run():
                ...
            t = rec.table()          # structured: t_ms, V_mean, _Na_i__mean, V_frac_below, V_nonfinite
            rec.check_finite()

    `t_ms` is the model time since the recorder was attached at which the sample was taken: (s + 1) * every ticks of
    `dt_per_step * dt` ms.  'sum' and 'mean' weigh with `weight`; every other kind looks at the cells of `mask`."""
    NOUN, END, COUNT = 'statistics recorder', 'stats_end', 'stats_count'

    def __init__(self, model, columns, every=1, weight='phase', mask=None, capacity=None):
        self._st = st = attach(model, 'record_stats', 'tissue statistics are recorded')
        self.columns = parse_columns(columns, model.VAR_NAMES)
        self.every = check_every('record_stats', every)
        cells = model.height * model.width
        self.weight = weight = weight_plane(model, weight, 'record_stats')
        self.mask = mask = mask_plane(model, mask, 'record_stats')
        self.weight_sum = weight_sum(weight, cells)
        self.cells = int(np.count_nonzero(mask)) if mask is not None else cells
        self.tick_ms = tick_ms(model)
        self.capacity = int(run_capacity(model, self.every) if capacity is None else capacity)
        st.stats_begin(device_columns(self.columns), weight, mask, self.every, self.capacity)
        self.open = True

    def raw(self, first=0, count=None):
        """float64 [samples, ncols] exactly as the device wrote it: sums for 'mean', counts for the fractions"""
        self._check()
        return self._st.stats_read(first, count)

    def values(self, first=0, count=None):
        """float64 [samples, ncols]: the columns' values ('mean' and the fractions divided on the host, in float64)"""
        return finish(self.raw(first, count), self.columns, self.weight_sum, self.cells)

    def times(self, first=0, count=None):
        return sample_times(first, self._span(first, count), self.every, self.tick_ms)

    def table(self, first=0, count=None):
        """structured array: t_ms + one float64 field per column, named '<array>_<kind>'"""
        return make_table(self.raw(first, count), self.columns, self.weight_sum, self.cells, self.every, self.tick_ms, first)

    def check_finite(self):
        """raises FloatingPointError naming the first sample / tick whose row shows a value that is not finite"""
        check_finite(self.raw(), self.columns, self.cells, self.every, self.tick_ms)
