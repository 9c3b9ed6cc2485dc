"""potential — the unipolar electrogram at every site of a lattice, recorded on the device while a model runs.

What an electro-anatomical mapping system shows is not the membrane potential but the extracellular potential at many sites at
once.  `PotentialMapRecorder` has the library form the lead recorder's source every `every` ticks — the membrane current
w * laplace(X), the `laplace()` of this code base in the exact form — and convolve it, in float64, with ONE lead-field table
truncated at a radius R <= 32 (`pmap_source_kernel`, `pmap_conv_kernel`): one float64 per sample and site, kept on the device in
a cube until it is read.  From the cube the device makes, at read time, the per-site summary
(`pmap_summary_kernel`): the extremes — the voltage map is their difference — and the steepest negative slope, the
electrogram's activation time.  The definition is exact (include/fibhip.h, fibhip_pmap_*; restated in NumPy in
tests/potential_ref.py)."""
import numpy as np

from ._lib import PMAP_MAX_RADIUS, PMAP_MAX_STEP
from ._recorder import SampledRecorder, array_index, attach, check_every, run_capacity, sample_times, tick_ms, weight_plane
from .leads import _zero_padded, point_table
from .tensor import refuse as refuse_tensor

WHO = 'record_potential_map'


def truncated_table(R, z, dx=1.0):
    """the lead field of a point electrode `z` > 0 cells above the sheet, truncated at `R` cells each way: float32 [R + 1, R + 1]
    (`leads.point_table`)"""
    return point_table(int(R) + 1, int(R) + 1, z, dx)


def parse_table(table, radius):
    """(table, radius) as `record_potential_map` takes them -> (float32 [R + 1, R + 1], R)"""
    table = np.asarray(table, np.float32)
    if table.ndim != 2 or table.shape[0] != table.shape[1]:
        raise ValueError('%s: the table is [R + 1, R + 1] (got an array of shape %s)' % (WHO, table.shape))
    R = table.shape[0] - 1 if radius is None else int(radius)
    if not 1 <= R <= PMAP_MAX_RADIUS:
        raise ValueError('%s: radius must be 1 .. %d (got %d)' % (WHO, PMAP_MAX_RADIUS, R))
    if table.shape != (R + 1, R + 1):
        raise ValueError('%s: a table of shape %s for radius %d: it must be [%d, %d]' % (WHO, table.shape, R, R + 1, R + 1))
    if not np.all(np.isfinite(table)):
        raise ValueError('%s: the table has a value that is not finite' % WHO)
    return np.ascontiguousarray(table), R


def parse_lattice(window, step, h, w):
    """(window, step) -> ((r0, r1, c0, c1), (sy, sx), (oh, ow)); window None: the whole grid"""
    win = (0, h, 0, w) if window is None else tuple(int(a) for a in window)
    if len(win) != 4:
        raise ValueError('%s: a window is (r0, r1, c0, c1)' % WHO)
    r0, r1, c0, c1 = win
    if not (0 <= r0 < r1 <= h and 0 <= c0 < c1 <= w):
        raise ValueError('%s: the window rows [%d, %d) x columns [%d, %d) is empty or outside the %d x %d grid' % (WHO, r0, r1, c0, c1, h, w))
    try:
        sy, sx = (int(a) for a in step)
    except (TypeError, ValueError):
        raise ValueError('%s: a step is (sy, sx)' % WHO)
    if not (1 <= sy <= PMAP_MAX_STEP and 1 <= sx <= PMAP_MAX_STEP):
        raise ValueError('%s: a step is 1 .. %d cells each way (got %d x %d)' % (WHO, PMAP_MAX_STEP, sy, sx))
    return win, (sy, sx), (-(-(r1 - r0) // sy), -(-(c1 - c0) // sx))


class PotentialMapRecorder(SampledRecorder):
    """unipolar electrograms at every site of a lattice, recorded on the device; see `IonicModel.record_potential_map`.

        tab = potential.truncated_table(16, z=2.0)
        with m.record_potential_map(tab, every=10, step=(4, 4)) as rec:
            for i in m.run():
                ...
            volt = rec.voltage()            # float64 [oh, ow]: peak-to-peak amplitude
            lat = rec.lat_ms()              # float64 [oh, ow]: the time of the steepest negative slope
            phi = rec.maps()                # float64 [samples, oh, ow]

    `times_ms()` is the model time since the recorder was attached at which a sample was taken: (s + 1) * every ticks of
    `dt_per_step * dt` ms."""
    NOUN, END, COUNT = 'potential-map recorder', 'pmap_end', 'pmap_count'

    def __init__(self, model, table, radius=None, every=10, window=None, step=(1, 1), var=0, weight='phase', max_samples=None):
        self._st = st = attach(model, WHO, 'potential maps are recorded')
        if _zero_padded(model):
            raise ValueError('%s: not on a model with the zero-padded Laplacian (ZEROPAD): its diffusion term is not this source' % WHO)
        refuse_tensor(model, WHO, 'its diffusion term is not this source')
        self.table, self.radius = parse_table(table, radius)
        self.window, self.step, self.shape = parse_lattice(window, step, model.height, model.width)
        self.every = check_every(WHO, every)
        self.var = array_index(model.VAR_NAMES, var, WHO, check_range=False)              # (an index is the library's to refuse)
        self.weight = weight = weight_plane(model, weight, WHO, finite=True)
        self.scale = float(getattr(model, 'diff', 1.0))
        self.tick_ms = tick_ms(model)
        self.capacity = int(run_capacity(model, self.every) if max_samples is None else max_samples)
        if self.capacity < 1:
            raise ValueError('%s: max_samples must be >= 1' % WHO)
        st.pmap_begin(self.table, weight, self.window, self.step, self.var, self.every, self.capacity)
        self.open = True

    def sites(self):
        """(rows int [oh], cols int [ow]): site (i, j) sits at the cell (rows[i], cols[j])"""
        r0, r1, c0, c1 = self.window
        return np.arange(r0, r1, self.step[0]), np.arange(c0, c1, self.step[1])

    def raw(self, first=0, count=None):
        """float64 [samples, oh, ow] exactly as the device wrote it"""
        self._check()
        return self._st.pmap_read(first, count)

    def maps(self, first=0, count=None, scale=None):
        """the electrograms: raw * scale, float64 [samples, oh, ow].  `scale` defaults to the model's `diff`, as for
        `LeadRecorder.traces`; the 1 / (4 pi sigma) of a medium is the caller's"""
        s = self.scale if scale is None else float(scale)
        return self.raw(first, count) * np.float64(s)

    def times_ms(self, first=0, count=None):
        return sample_times(first, self._span(first, count), self.every, self.tick_ms)

    def summary(self, first=0, count=None):
        """made on the device over the samples [first, first + count) (at least 2; count=None: all so far), per site and
        unscaled: a dict of vmin, vmax (float64) with their sample indices kmin, kmax (int32), and dmin, the most negative
        phi[s] - phi[s - 1], with its index kd = s"""
        self._check()
        return dict(zip(('vmin', 'vmax', 'dmin', 'kmin', 'kmax', 'kd'), self._st.pmap_summary(first, count)))

    def voltage(self, first=0, count=None, scale=None):
        """the voltage map: peak-to-peak amplitude (vmax - vmin) * |scale| per site, float64 [oh, ow]"""
        s = self.summary(first, count)
        return (s['vmax'] - s['vmin']) * np.float64(abs(self.scale if scale is None else float(scale)))

    def lat_ms(self, first=0, count=None):
        """the electrogram's local activation time: the midpoint, in ms since attach, of the two samples between which the
        potential fell most steeply; float64 [oh, ow] (for a negative `scale` the steepest fall is a rise: this map is of the
        raw values)"""
        kd = self.summary(first, count)['kd'].astype(np.float64)
        return (kd + 0.5) * self.every * self.tick_ms

    def bipolar(self, axis=1, first=0, count=None, scale=None):
        """bipolar electrograms, on the host: differences of neighbouring sites along `axis` of the lattice (0: rows, 1:
        columns), site k + 1 minus site k; float64 [samples, oh - 1, ow] or [samples, oh, ow - 1]"""
        if axis not in (0, 1):
            raise ValueError('bipolar: axis is 0 (rows) or 1 (columns)')
        return np.diff(self.maps(first, count, scale), axis=axis + 1)
