"""leads — unipolar electrograms recorded on the device while a model runs.

An extracellular electrode does not see the potential under it: it sees the transmembrane current of every cell of the sheet,
weighted by the inverse distance.  `LeadRecorder` has the library form that current every `every` ticks — the Laplacian of the
potential with the phase-field term, the `laplace()` of this code base, times a weight plane (the phase field: the conservative
div(phi grad V), silent outside the tissue) — and sum it, in float64, through up to 64 lead fields at once (`lead_kernel`,
`lead_combine_kernel`): one float64 per sample and lead, kept on the device until it is read, no read-back and no synchronisation
per sample.  The definition is exact (include/fibhip.h, fibhip_leads_*; restated in NumPy in
tests/lead_ref.py).

A lead field is a table T[|dr|][|dc|] of the size of the grid: `point_table` makes the one of a point electrode at a height z
above the sheet; a finite-size electrode or a far-field ECG lead is any other finite table."""
import numpy as np

from ._lib import MAX_LEAD_TABLES, MAX_LEADS
from ._recorder import SampledRecorder, array_index, attach, check_every, run_capacity, sample_times, tick_ms, weight_plane
from .tensor import refuse as refuse_tensor


def point_table(h, w, z, dx=1.0):
    """the lead field of a point electrode `z` > 0 cells above the sheet, as a table over the row and column distances i, j in
    cells: float32(1 / sqrt((i * dx)**2 + (j * dx)**2 + z**2)), evaluated in float64 and rounded once; float32 [h, w]"""
    h, w = int(h), int(w)
    z, dx = float(z), float(dx)
    if h < 1 or w < 1:
        raise ValueError('point_table: a table of %d x %d' % (h, w))
    if not (z > 0 and np.isfinite(z)) or not (dx > 0 and np.isfinite(dx)):
        raise ValueError('point_table: z and dx must be finite and > 0 (got z = %r, dx = %r)' % (z, dx))
    i = np.arange(h, dtype=np.float64)[:, np.newaxis] * dx
    j = np.arange(w, dtype=np.float64)[np.newaxis, :] * dx
    return (1.0 / np.sqrt(i * i + j * j + z * z)).astype(np.float32)


def parse_leads(positions, tables, table_of, h, w):
    """(positions, tables, table_of) as `record_leads` takes them -> (int32 [n, 3] = row, col, table; float32 [ntables, h, w])"""
    pos = np.asarray(positions)
    if pos.ndim != 2 or pos.shape[1] != 2 or not 1 <= len(pos) <= MAX_LEADS:
        raise ValueError('record_leads: 1 .. %d electrodes, each a (row, col) (got an array of shape %s)' % (MAX_LEADS, pos.shape))
    if not np.issubdtype(pos.dtype, np.integer):
        if not np.all(pos == np.floor(pos)):
            raise ValueError('record_leads: an electrode sits at an integer cell (row, col)')
        pos = pos.astype(np.int64)
    tables = np.asarray(tables, np.float32)
    if tables.ndim == 2:
        tables = tables[np.newaxis]
    if tables.ndim != 3 or not 1 <= len(tables) <= MAX_LEAD_TABLES:
        raise ValueError('record_leads: 1 .. %d lead-field tables [height, width] (got an array of shape %s)' % (MAX_LEAD_TABLES, tables.shape))
    if tables.shape[1:] != (h, w):
        raise ValueError('record_leads: a table of shape %s on a %d x %d grid' % (tables.shape[1:], h, w))
    if not np.all(np.isfinite(tables)):
        raise ValueError('record_leads: a lead-field table has a value that is not finite')
    for e, (r, c) in enumerate(pos):
        if not (0 <= r < h and 0 <= c < w):
            raise ValueError('record_leads: electrode %d at (%d, %d) is outside the %d x %d grid' % (e, r, c, h, w))
    if table_of is None:
        if len(tables) != 1:
            raise ValueError('record_leads: %d tables: table_of must name one for every electrode' % len(tables))
        table_of = np.zeros(len(pos), np.int64)
    table_of = np.asarray(table_of)
    if table_of.shape != (len(pos),) or not np.issubdtype(table_of.dtype, np.integer):
        raise ValueError('record_leads: table_of is one table index per electrode (%d of them)' % len(pos))
    for e, t in enumerate(table_of):
        if not 0 <= t < len(tables):
            raise ValueError('record_leads: electrode %d names table %d of %d' % (e, t, len(tables)))
    out = np.empty((len(pos), 3), np.int32)
    out[:, :2] = pos
    out[:, 2] = table_of
    return out, np.ascontiguousarray(tables)


def _zero_padded(model):
    """a traced model whose Laplacian is the zero-padded 3x3 convolution (traced.py generates ZEROPAD into its header)"""
    c = getattr(model, '_compiled', None)
    return isinstance(c, dict) and 'ZEROPAD = true' in c.get('source', '')


class LeadRecorder(SampledRecorder):
    """unipolar electrograms recorded on the device; see `IonicModel.record_leads`.

        tab = leads.point_table(m.height, m.width, z=2.0)
        with m.record_leads([(256, 300), (256, 305)], tables=tab, every=10) as rec:
            for i in m.run():
                ...
            phi = rec.traces()              # float64 [samples, 2]
            bip = rec.bipolar([(0, 1)])     # float64 [samples, 1]

    `times_ms()` is the model time since the recorder was attached at which a sample was taken: (s + 1) * every ticks of
    `dt_per_step * dt` ms."""
    NOUN, END, COUNT = 'lead recorder', 'leads_end', 'leads_count'

    def __init__(self, model, positions, tables, table_of=None, every=1, weight='phase', var=0, capacity=None):
        self._st = st = attach(model, 'record_leads', 'electrograms are recorded')
        if _zero_padded(model):
            raise ValueError('record_leads: not on a model with the zero-padded Laplacian (ZEROPAD): its diffusion term is not this source')
        refuse_tensor(model, 'record_leads', 'its diffusion term is not this source')
        self.pos, self.tables = parse_leads(positions, tables, table_of, model.height, model.width)
        self.every = check_every('record_leads', every)
        self.var = array_index(model.VAR_NAMES, var, 'record_leads', check_range=False)      # (an index is the library's to refuse)
        self.weight = weight = weight_plane(model, weight, 'record_leads', finite=True)
        self.scale = float(getattr(model, 'diff', 1.0))
        self.tick_ms = tick_ms(model)
        self.capacity = int(run_capacity(model, self.every) if capacity is None else capacity)
        if self.capacity < 1:
            raise ValueError('record_leads: capacity must be >= 1')
        st.leads_begin(self.pos, self.tables, weight, self.var, self.every, self.capacity)
        self.open = True

    def raw(self, first=0, count=None):
        """float64 [samples, electrodes] exactly as the device wrote it"""
        self._check()
        return self._st.leads_read(first, count)

    def traces(self, scale=None, first=0, count=None):
        """the unipolar electrograms: raw * scale, float64 [samples, electrodes].  `scale` defaults to the model's `diff`, which
        makes the source diff * div(w grad X), the diffusion term of the model; the 1 / (4 pi sigma) of a medium is the
        caller's"""
        s = self.scale if scale is None else float(scale)
        return self.raw(first, count) * np.float64(s)

    def bipolar(self, pairs, scale=None, first=0, count=None):
        """differences of pairs of electrodes: column k is trace[a_k] - trace[b_k] for pairs[k] = (a_k, b_k)"""
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        n = len(self.pos)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= n):
            raise ValueError('bipolar: a pair names an electrode outside 0 .. %d' % (n - 1))
        t = self.traces(scale, first, count)
        return t[:, pairs[:, 0]] - t[:, pairs[:, 1]]

    def times_ms(self, first=0, count=None):
        return sample_times(first, self._span(first, count), self.every, self.tick_ms)
