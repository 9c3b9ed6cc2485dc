"""beats — a per-cell history of the last beats kept on the device while a model runs: APD restitution, alternans maps and
beat counts without the movie cube.

The activation recorder keeps one upstroke, one APD and one count per cell; a second beat overwrites the first, and every tick
is a launch of its own.  `BeatRecorder` has the library compare a pixel plane every `every` ticks with the plane of the
previous sample and keep, per pixel, a ring of the last `depth` beats: the interpolated time of the upstroke through `up`, of the
downstroke through `down`, and the peak in between.  Between two samples the handle keeps its multi-tick launches; nothing
leaves the device until it is asked for.  The definition is exact (include/fibhip.h, fibhip_beats_*;
restated in NumPy in tests/beat_ref.py).

    with model.record_beats(every=10, depth=8) as rec:
        for i in model.run():
            ...
        di, apd = rec.restitution()              # every (DI, APD) pair of every cell
        maps = rec.summary(last=4)               # nused, apd_mean, cl_mean, apd_alt

All times are milliseconds since the recorder was attached."""
import numpy as np

from . import velocity as _velocity
from ._recorder import DeviceRecorder, attach, check_every, tick_ms, weight_plane

MAX_DEPTH = 16                                   # include/fibhip.h FIBHIP_BEATS_MAX_DEPTH
SUMMARY_MAPS = ('nused', 'apd_mean', 'cl_mean', 'apd_alt')


def default_levels(min_v, max_v):
    """(up, down): the 50 % and the 10 % level of [min_v, max_v] as float32 — the activation recorder's defaults"""
    from .activation import default_thresholds
    return default_thresholds(min_v, max_v)


def check_args(every, depth, up, down, block, reduce):
    """the refusals that need no device: raises ValueError"""
    check_every('record_beats', every)
    if not 1 <= int(depth) <= MAX_DEPTH:
        raise ValueError('record_beats: depth must be 1 .. %d (got %d)' % (MAX_DEPTH, depth))
    if not np.float32(down) <= np.float32(up):
        raise ValueError('record_beats: the levels must be numbers with down <= up (got down %r, up %r)' % (down, up))
    if reduce not in ('point', 'mean'):
        raise ValueError("record_beats: reduce is 'point' or 'mean'")
    if len(block) != 2 or not all(1 <= int(b) <= 16 for b in block):
        raise ValueError('record_beats: a block is 1 .. 16 cells each way')


def order_ring(t_up, t_down, peak, count, pk=None):
    """the ring planes [depth, ...] in slot order (beat b in slot b % depth) -> the same planes in beat order: index -1 is
    the newest beat of every pixel, index -1 - j the one j beats before it, NaN in front where a pixel has fewer than `depth`
    beats.  With `pk` (the live peak, NaN outside a beat) the peak of a beat still open is filled in.  Returns a dict with
    't_up', 't_down', 'peak' (float32) and 'count' (int32)"""
    t_up, t_down, peak = (np.asarray(a, np.float32) for a in (t_up, t_down, peak))
    count = np.asarray(count, np.int32)
    depth = t_up.shape[0]
    assert t_up.shape == t_down.shape == peak.shape == (depth,) + count.shape
    b = count.astype(np.int64)[None] - depth + np.arange(depth).reshape((depth,) + (1,) * count.ndim)     # the beat number at index j
    have = b >= 0
    slot = np.where(have, b % depth, 0)
    out = {}
    for name, plane in (('t_up', t_up), ('t_down', t_down), ('peak', peak)):
        out[name] = np.where(have, np.take_along_axis(plane, slot, axis=0), np.float32(np.nan)).astype(np.float32)
    if pk is not None:
        pk = np.asarray(pk, np.float32)
        is_open = (pk == pk) & (count > 0)
        out['peak'][-1] = np.where(is_open, pk, out['peak'][-1])
    out['count'] = count.copy()
    return out


def apd_of(beats):
    """float64 [depth, ...]: t_down - t_up of every beat (NaN: no such beat, or it never finished)"""
    return beats['t_down'].astype(np.float64) - beats['t_up'].astype(np.float64)


def cl_of(beats):
    """float64 [depth, ...]: cl[b] = t_up[b] - t_up[b - 1]; index 0 has no predecessor in the ring and is NaN"""
    t = beats['t_up'].astype(np.float64)
    out = np.full(t.shape, np.nan)
    out[1:] = t[1:] - t[:-1]
    return out


def di_of(beats):
    """float64 [depth, ...]: the diastolic interval in front of every beat, di[b] = t_up[b] - t_down[b - 1]; index 0 is NaN"""
    tu, td = beats['t_up'].astype(np.float64), beats['t_down'].astype(np.float64)
    out = np.full(tu.shape, np.nan)
    out[1:] = tu[1:] - td[:-1]
    return out


def restitution_of(beats, mask=None):
    """(di, apd): two flat float64 arrays, the pairs of every pixel (those of `mask`, a boolean map) and beat that has both"""
    di, apd = di_of(beats), apd_of(beats)
    ok = np.isfinite(di) & np.isfinite(apd)
    if mask is not None:
        mask = np.asarray(mask, bool)
        if mask.shape != di.shape[1:]:
            raise ValueError('restitution: a mask of shape %s on a map of shape %s' % (mask.shape, di.shape[1:]))
        ok &= mask[None]
    return di[ok], apd[ok]


class BeatRecorder(DeviceRecorder):
    """the last `depth` beats of every pixel, kept on the device; see `IonicModel.record_beats`"""
    NOUN, END = 'beat recorder', 'beats_end'

    def __init__(self, model, every=10, depth=8, up=None, down=None, var=0, region=None, block=(1, 1), reduce='mean', weight=None):
        self._st = st = attach(model, 'record_beats', 'beats are recorded')
        self.every, self.depth, self.var = int(every), int(depth), int(var)
        self.tick_ms = tick_ms(model)
        if (up is None or down is None) and self.var != 0:
            raise ValueError('record_beats: the default levels are those of array 0; pass up and down for var = %d' % self.var)
        d_up, d_down = default_levels(float(model.min_v), float(model.max_v))
        self.up = np.float32(d_up if up is None else up)
        self.down = np.float32(d_down if down is None else down)
        self.block = tuple(int(b) for b in block)
        self.reduce = reduce
        check_args(self.every, self.depth, self.up, self.down, self.block, reduce)
        self.window = (0, model.height, 0, model.width) if region is None else tuple(int(v) for v in region)
        self.weight = weight = weight_plane(model, weight, 'record_beats')
        st.beats_begin(self.var, self.window, self.block, self.reduce, weight, self.every, self.up, self.down, self.depth)
        oh, ow, _ = st.beats_shape()
        self.shape = (oh, ow)
        self.open = True

    def samples(self):
        """samples taken since the recorder was attached"""
        self._check()
        return self._st.beats_count()

    def raw(self):
        """(t_up, t_down, peak [depth, oh, ow] float32 in slot order, count [oh, ow] int32, pk [oh, ow] float32): the
        recorder's planes as they stand on the device"""
        self._check()
        return self._st.beats_read()

    def beats(self):
        """{'t_up', 't_down', 'peak': float32 [depth, oh, ow], 'count': int32 [oh, ow]}: index -1 is the newest beat of every
        pixel, NaN in front where a pixel has fewer beats; the peak of a beat still open is the running one"""
        return order_ring(*self.raw())

    def apd(self):
        """float64 [depth, oh, ow]: t_down - t_up"""
        return apd_of(self.beats())

    def di(self):
        """float64 [depth, oh, ow]: di[b] = t_up[b] - t_down[b - 1]"""
        return di_of(self.beats())

    def cl(self):
        """float64 [depth, oh, ow]: cl[b] = t_up[b] - t_up[b - 1]"""
        return cl_of(self.beats())

    def restitution(self, mask=None):
        """(di, apd): the flat pairs of every pixel (of `mask`) and beat that has both — the restitution curve's points"""
        return restitution_of(self.beats(), mask)

    def summary(self, last=4):
        """{'nused': int32, 'apd_mean', 'cl_mean', 'apd_alt': float32}, each [oh, ow], made on the device over the newest
        `last` (1 .. depth) beats: the beats with an APD, their mean APD, the mean cycle length, and the signed alternans
        amplitude (its sign changes across the sheet where the alternans is discordant)"""
        self._check()
        if not 1 <= int(last) <= self.depth:
            raise ValueError('summary: last must be 1 .. depth = %d (got %d)' % (self.depth, last))
        return dict(zip(SUMMARY_MAPS, self._st.beats_summary(int(last))))

    def velocity(self, last=1, radius=2, max_dt=20.0, min_cells=None, mask=None):
        """{'gy', 'gx', 'rms': float32 [last, oh, ow], 'nfit': int32 [last, oh, ow]}: the gradient of activation time (ms per
        pixel along rows and columns), the residual of the fit and the cells that took part, for the newest `last` (1 .. depth)
        beats of every pixel in beats()'s order, index -1 the newest — a plane fitted on the device to the upstroke times of the
        (2 * radius + 1)^2 pixels around each that lie within `max_dt` ms of its own (fib_tf_amd/velocity.py).  NaN where fewer
        than `min_cells` (default: a majority of the window) match or they lie on one line.  One device call per beat: memory
        stays at four maps.  `max_dt`: below half the shortest cycle length, so that two beats of a neighbour are never
        confused, and above the time a front needs to cross `radius` pixels.  `mask`: [oh, ow], non-zero where a pixel counts"""
        self._check()
        radius, max_dt, min_cells = _velocity.check_args(radius, max_dt, min_cells, self.depth, last, 'velocity')
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
            if mask.shape != self.shape:
                raise ValueError('velocity: a mask of shape %s on a map of shape %s' % (mask.shape, self.shape))
        out = {k: np.empty((int(last),) + self.shape, np.int32 if k == 'nfit' else np.float32) for k in _velocity.MAPS}
        for back in range(int(last)):
            for k, m in zip(_velocity.MAPS, self._st.beats_velocity(back, radius, max_dt, min_cells, mask)):
                out[k][int(last) - 1 - back] = m
        return out

    def speed(self, last=1, **kw):
        """float64 [last, oh, ow]: the conduction velocity in CELLS per ms (the block is taken out), NaN where there is no fit;
        the keywords are velocity()'s"""
        return _velocity.speed_of(self.velocity(last, **kw), self.block)

    def cv_restitution(self, last=None, mask=None, max_rms=None, **kw):
        """(di, cv): the flat pairs of every pixel (of `mask`) and beat of the newest `last` (None: depth) that has a diastolic
        interval in front of it and a fit, with a residual of at most `max_rms` ms if given — CV restitution, the other half of
        restitution()'s pair.  The other keywords are velocity()'s"""
        last = self.depth if last is None else int(last)
        vel = self.velocity(last, mask=mask, **kw)
        return _velocity.cv_restitution_of(self.beats(), vel, self.block, mask, max_rms)
