"""waves — the excited domains of the sheet, labelled and measured on the device while a model runs.

How many separate waves are on the sheet, how large are they and where: the wavelet count and the size distribution of the
excited domains are the standard complexity measures of fibrillation, and a wave that ends on a boundary, on a hole or on itself
has no tip for the tip recorder to find.  `WaveRecorder` has the library label the connected components of the cells that meet a
condition every `every` ticks (`wave_label_kernel`, `wave_merge_kernel`, `wave_root_kernel`, `wave_reduce_kernel`) and keeps
their counts and records on the device until they are read: no read-back and no synchronisation per sample (DESIGN.md section
21).  The definition is exact (include/fibhip.h, fibhip_waves_*; restated in NumPy in tests/wave_ref.py).  With
`kind='below'` the same machinery gives the domains of the excitable gap."""
import numpy as np

from ._lib import MAX_WAVES, WAVE_KINDS

WAVE_DTYPE = np.dtype([('t_ms', np.float64), ('seed', np.int32), ('area', np.int32), ('cy', np.float64), ('cx', np.float64),
                       ('r0', np.int32), ('r1', np.int32), ('c0', np.int32), ('c1', np.int32)])


def _array_index(model, var, what):
    if isinstance(var, str):
        if var not in model.VAR_NAMES:
            raise ValueError('record_waves: unknown array %r for %s (the model has %s)' % (var, what, ', '.join(model.VAR_NAMES)))
        return model.VAR_NAMES.index(var)
    var = int(var)
    if not 0 <= var < len(model.VAR_NAMES):
        raise ValueError('record_waves: %s names array %d of %d' % (what, var, len(model.VAR_NAMES)))
    return var


def _kind_index(kind, what):
    if kind not in WAVE_KINDS:
        raise ValueError("record_waves: %s is 'above' or 'below' (got %r)" % (what, kind))
    return WAVE_KINDS.index(kind)


def _level(level, what):
    with np.errstate(over='ignore'):
        level = float(np.float32(level))
    if not np.isfinite(level):
        raise ValueError('record_waves: %s must be finite (got %r)' % (what, level))
    return level


def default_mask(model):
    """phase > 0.5 where the model has a phase field, with the outer ring of the grid — the ghost copies — cleared"""
    phase = getattr(model, 'phase', None)
    mask = np.ones((model.height, model.width), bool) if phase is None else np.asarray(phase) > 0.5
    mask = mask.copy()
    mask[0, :] = mask[-1, :] = False
    mask[:, 0] = mask[:, -1] = False
    return mask


class WaveRecorder:
    """excited domains recorded on the device; see `IonicModel.record_waves`.

        with model.record_waves(every=10) as rec:
            for i in model.run():
                ...
            n = rec.counts()[:, 0]               # the wavelet count over time
            per_sample = rec.waves()             # one structured array (t_ms, seed, area, cy, cx, r0, r1, c0, c1) per sample
            plane = rec.labels()                 # the label plane of the last sample

    `t_ms` is the model time since the recorder was attached at which the sample was taken: (s + 1) * every ticks of
    `dt_per_step * dt` ms.  At most `max_waves` waves are kept per sample (`truncated()` names the samples that had more);
    `counts()` is exact regardless."""

    def __init__(self, model, level=None, kind='above', every=1, conn=4, mask=None, max_waves=256, capacity=None, var=0, also=None):
        from .activation import default_thresholds
        from .sharded import ShardedStepper
        st = model._stepper
        if st is None:
            raise AssertionError('record_waves should be called after calling define')
        if isinstance(st, ShardedStepper):
            raise NotImplementedError('record_waves: waves are labelled on a single device only; this model runs as row '
                                      'blocks over %d ranks' % st.world)
        self.var = _array_index(model, var, 'var')
        self.kind = _kind_index(kind, 'kind')
        if level is None:
            level = default_thresholds(float(model.min_v), float(model.max_v))[0]
        self.level = _level(level, 'level')
        self.var2, self.kind2, self.level2 = -1, 0, 0.0
        if also is not None:
            if len(also) != 3:
                raise ValueError('record_waves: also is (array, kind, level)')
            self.var2 = _array_index(model, also[0], 'also')
            self.kind2 = _kind_index(also[1], "also's kind")
            self.level2 = _level(also[2], "also's level")
        self.conn = int(conn)
        if self.conn not in (4, 8):
            raise ValueError('record_waves: conn is 4 or 8 (got %r)' % (conn,))
        self.every = int(every)
        if self.every < 1:
            raise ValueError('record_waves: every must be >= 1')
        self.max_waves = int(max_waves)
        if not 1 <= self.max_waves <= MAX_WAVES:
            raise ValueError('record_waves: max_waves is 1 .. %d (got %d)' % (MAX_WAVES, self.max_waves))
        self.tick_ms = float(model.dt_per_step * model.dt)
        if capacity is None:                     # the samples of a whole run of model.duration (whatever has run already), at least 1
            ticks = int(model.duration / (model.dt_per_step * model.dt))
            capacity = max(1, ticks // self.every)
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError('record_waves: capacity must be >= 1')
        if mask is None:
            mask = default_mask(model)
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        if mask.shape != (model.height, model.width):
            raise ValueError('record_waves: a mask of shape %s on a %d x %d grid' % (mask.shape, model.height, model.width))
        self.mask = mask
        self._st = st
        st.waves_begin(self.var, self.kind, self.level, self.var2, self.kind2, self.level2, self.conn, mask, self.max_waves, self.every,
                       self.capacity)
        self.open = True

    def _check(self):
        if not self.open:
            raise AssertionError('the wave recorder has been closed')

    def count(self):
        """samples taken since the recorder was attached"""
        self._check()
        return self._st.waves_count()

    def counts(self, first=0, count=None):
        """int32 [samples, 3]: n (waves), stored (records kept), cells (set cells) of every sample; exact even where the list was cut"""
        self._check()
        return self._st.waves_read(first, count, records=False)[0]

    def raw(self, first=0, count=None):
        """(counts, records) exactly as the device wrote them: records [samples, max_waves] of struct fibhip_wave_record, the
        first `stored` of a sample valid, in the order of arrival"""
        self._check()
        return self._st.waves_read(first, count)

    def truncated(self):
        """indices of the samples that had more waves than `max_waves`: their lists are cut, their counts are not"""
        return np.flatnonzero(self.counts()[:, 0] > self.max_waves)

    def waves(self, first=0, count=None):
        """a list with one structured array (t_ms, seed, area, cy, cx, r0, r1, c0, c1) per sample, sorted by seed; the centroid
        (cy, cx) is the float64 quotient of the integer sums by the area"""
        counts, records = self.raw(first, count)
        out = []
        for s in range(len(counts)):
            r = records[s, :int(counts[s, 1])]
            r = r[np.argsort(r['seed'], kind='stable')]
            a = np.empty(len(r), WAVE_DTYPE)
            a['t_ms'] = (int(first) + s + 1) * self.every * self.tick_ms
            for f in ('seed', 'area', 'r0', 'r1', 'c0', 'c1'):
                a[f] = r[f]
            a['cy'] = r['sum_r'].astype(np.float64) / r['area']
            a['cx'] = r['sum_c'].astype(np.float64) / r['area']
            out.append(a)
        return out

    def labels(self):
        """the label plane of the latest sample: int32 [height, width], the seed of the cell's wave, -1 where the cell is not set"""
        self._check()
        return self._st.waves_labels()

    def times_ms(self, first=0, count=None):
        n = self.count() - int(first) if count is None else int(count)
        return (int(first) + 1 + np.arange(max(n, 0))) * self.every * self.tick_ms

    def close(self):
        """detaches the recorder and frees the lists"""
        if self.open:
            self.open = False
            self._st.waves_end()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
