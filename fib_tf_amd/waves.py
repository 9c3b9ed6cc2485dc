"""waves — the excited domains of the sheet, labelled and measured on the device while a model runs.

How many separate waves are on the sheet, how large are they and where: the wavelet count and the size distribution of the
excited domains are the standard complexity measures of fibrillation, and a wave that ends on a boundary, on a hole or on itself
has no tip for the tip recorder to find.  `WaveRecorder` has the library label the connected components of the cells that meet a
condition every `every` ticks (`wave_label_kernel`, `wave_merge_kernel`, `wave_root_kernel`, `wave_reduce_kernel`) and keeps
their counts and records on the device until they are read: no read-back and no synchronisation per sample (DESIGN.md section
21).  The definition is exact (include/fibhip.h, fibhip_waves_*; restated in NumPy in tests/wave_ref.py).  With
`kind='below'` the same machinery gives the domains of the excitable gap.

With `links=True` two more kernels (`wave_link_kernel`, `wave_link_pack_kernel`) keep, per sample, the pairs (wave of the sample
before, wave of this sample) that share cells and how many cells they share: what tells a wave that split from one that died
while another was born beside it.  `events` and `track` below turn those lists into wavebreak, coalescence, birth and death
counts and into a genealogy of the waves — plain NumPy on the lists, nothing of the device."""
import numpy as np

from ._lib import MAX_WAVE_LINKS, MAX_WAVES, WAVE_KINDS
from ._recorder import SampledRecorder, attach, check_every, mask_plane, run_capacity, sample_times, tick_ms

WAVE_DTYPE = np.dtype([('t_ms', np.float64), ('seed', np.int32), ('area', np.int32), ('cy', np.float64), ('cx', np.float64),
                       ('r0', np.int32), ('r1', np.int32), ('c0', np.int32), ('c1', np.int32)])


LINK_DTYPE = np.dtype([('t_ms', np.float64), ('prev', np.int32), ('seed', np.int32), ('overlap', np.int32)])
EVENT_DTYPE = np.dtype([('t_ms', np.float64), ('waves', np.int32), ('births', np.int32), ('deaths', np.int32), ('splits', np.int32),
                        ('merges', np.int32), ('continued', np.int32)])
POINT_DTYPE = np.dtype([('t_ms', np.float64), ('seed', np.int32), ('area', np.int32), ('cy', np.float64), ('cx', np.float64)])


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


class WaveRecorder(SampledRecorder):
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
    NOUN, END, COUNT = 'wave recorder', 'waves_end', 'waves_count'

    def __init__(self, model, level=None, kind='above', every=1, conn=4, mask=None, max_waves=256, capacity=None, var=0, also=None,
                 links=False, max_links=None):
        from .activation import default_thresholds
        self._st = st = attach(model, 'record_waves', 'waves are labelled')
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
        self.every = check_every('record_waves', every)
        self.max_waves = int(max_waves)
        if not 1 <= self.max_waves <= MAX_WAVES:
            raise ValueError('record_waves: max_waves is 1 .. %d (got %d)' % (MAX_WAVES, self.max_waves))
        self.max_links = 0
        if links:
            self.max_links = min(2 * self.max_waves, MAX_WAVE_LINKS) if max_links is None else int(max_links)
            if not 1 <= self.max_links <= MAX_WAVE_LINKS:
                raise ValueError('record_waves: max_links is 1 .. %d (got %d)' % (MAX_WAVE_LINKS, self.max_links))
        self.tick_ms = tick_ms(model)
        self.capacity = int(run_capacity(model, self.every) if capacity is None else capacity)
        if self.capacity < 1:
            raise ValueError('record_waves: capacity must be >= 1')
        self.mask = mask = mask_plane(model, default_mask(model) if mask is None else mask, 'record_waves')
        st.waves_begin(self.var, self.kind, self.level, self.var2, self.kind2, self.level2, self.conn, mask, self.max_waves, self.every,
                       self.capacity)
        self.open = True
        if self.max_links:
            try:
                st.waves_links_begin(self.max_links)
            except Exception:
                self.close()
                raise

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

    # ---- links -------------------------------------------------------------------------------------------------------------
    def _check_links(self):
        self._check()
        if not self.max_links:
            raise ValueError('this wave recorder keeps no links: attach it with record_waves(links=True)')

    def link_counts(self, first=0, count=None):
        """int32 [samples, 4]: links (distinct pairs that found a place in the table), stored (records kept), cells (cells set in
        this sample and in the one before: exact), lost (cells whose pair found no place; while 0, `links` is exact)"""
        self._check_links()
        return self._st.waves_links_read(first, count, records=False)[0]

    def links_raw(self, first=0, count=None):
        """(counts, records) exactly as the device wrote them: records [samples, max_links] of struct fibhip_wave_link, the first
        `stored` of a sample valid, in the order of arrival"""
        self._check_links()
        return self._st.waves_links_read(first, count)

    def links_truncated(self):
        """indices of the samples whose link list is not complete: more links than `max_links`, or cells lost"""
        c = self.link_counts()
        return np.flatnonzero((c[:, 0] > self.max_links) | (c[:, 3] > 0))

    def links(self, first=0, count=None):
        """a list with one structured array (t_ms, prev, seed, overlap) per sample, sorted by (prev, seed): `prev` is a seed of the
        sample before, `seed` one of this sample, `overlap` the cells the two waves share.  Sample 0 has none"""
        counts, records = self.links_raw(first, count)
        out = []
        for s in range(len(counts)):
            r = records[s, :int(counts[s, 1])]
            r = r[np.lexsort((r['seed'], r['prev']))]
            a = np.empty(len(r), LINK_DTYPE)
            a['t_ms'] = (int(first) + s + 1) * self.every * self.tick_ms
            for f in ('prev', 'seed', 'overlap'):
                a[f] = r[f]
            out.append(a)
        return out

    def events(self, min_overlap=1):
        """`events` of every sample taken so far; a cut wave list or link list is refused (ValueError naming the sample)"""
        self._check_links()
        return events(self.waves(), self.links(), min_overlap, wave_counts=self.counts(), link_counts=self.link_counts(),
                      times_ms=self.times_ms())

    def tracks(self, min_overlap=1):
        """`track` of every sample taken so far; a cut wave list or link list is refused (ValueError naming the sample)"""
        self._check_links()
        return track(self.waves(), self.links(), min_overlap, wave_counts=self.counts(), link_counts=self.link_counts(),
                     times_ms=self.times_ms())

    def labels(self):
        """the label plane of the latest sample: int32 [height, width], the seed of the cell's wave, -1 where the cell is not set"""
        self._check()
        return self._st.waves_labels()

    def times_ms(self, first=0, count=None):
        return sample_times(first, self._span(first, count), self.every, self.tick_ms)


# ---- what the links say: events and tracks (host code on the lists) --------------------------------------------------------------
class Track:
    """one wave followed along `continued` links: `id`; `born` 'start' (there at sample 0), 'birth' (no wave before it overlaps it),
    'split' (its one predecessor went on into several) or 'merge' (several predecessors); `ended` 'death' (nothing overlaps it
    in the next sample), 'split', 'merge' or 'end' (alive at the last sample); `parents` and `children` are track ids; `points`
    is structured (t_ms, seed, area, cy, cx), one row per sample it lived through"""
    __slots__ = ('id', 'born', 'ended', 'parents', 'children', 'points')

    def __init__(self, id, born):
        self.id, self.born, self.ended, self.parents, self.children, self.points = id, born, 'end', [], [], []

    @property
    def lifetime_ms(self):
        return float(self.points['t_ms'][-1] - self.points['t_ms'][0])

    def __repr__(self):
        return 'Track(id=%d, born=%r, ended=%r, parents=%r, children=%r, points=%d)' % (self.id, self.born, self.ended, self.parents,
                                                                                       self.children, len(self.points))


def _checked(waves_per_sample, links_per_sample, wave_counts, link_counts):
    n = len(waves_per_sample)
    if len(links_per_sample) != n:
        raise ValueError('%d wave lists but %d link lists' % (n, len(links_per_sample)))
    if wave_counts is not None:
        wave_counts = np.asarray(wave_counts)
        for s in range(n):
            if not (wave_counts[s, 0] == wave_counts[s, 1] == len(waves_per_sample[s])):
                raise ValueError('sample %d: the wave list was cut (%d waves, %d given): raise max_waves'
                                 % (s, wave_counts[s, 0], len(waves_per_sample[s])))
    if link_counts is not None:
        link_counts = np.asarray(link_counts)
        for s in range(n):
            if not (link_counts[s, 0] == link_counts[s, 1] == len(links_per_sample[s])) or link_counts[s, 3] != 0:
                raise ValueError('sample %d: the link list was cut (%d links, %d given, %d cells lost): raise max_links'
                                 % (s, link_counts[s, 0], len(links_per_sample[s]), link_counts[s, 3]))
    if n and len(links_per_sample[0]):
        raise ValueError('sample 0: the first sample has no links')


def _graph(s, waves_per_sample, links_per_sample, min_overlap):
    """the overlap graph between the samples s - 1 and s: (seeds before, seeds now, links kept, out-degrees, in-degrees)"""
    P = [int(x) for x in waves_per_sample[s - 1]['seed']]
    Q = [int(x) for x in waves_per_sample[s]['seed']]
    L = links_per_sample[s]
    kept = [(int(p), int(q)) for p, q, o in zip(L['prev'], L['seed'], L['overlap']) if o >= min_overlap]
    out, into = dict.fromkeys(P, 0), dict.fromkeys(Q, 0)
    for p, q in kept:
        if p not in out or q not in into:
            raise ValueError('sample %d: the link (%d, %d) names a wave that is not in the wave lists (a cut list?)' % (s, p, q))
        out[p] += 1
        into[q] += 1
    return P, Q, kept, out, into


def _time_of(s, waves_per_sample, links_per_sample, times_ms):
    if times_ms is not None:
        return float(times_ms[s])
    for a in (waves_per_sample[s], links_per_sample[s]):
        if len(a) and 't_ms' in (a.dtype.names or ()):
            return float(a['t_ms'][0])
    return float('nan')


def events(waves_per_sample, links_per_sample, min_overlap=1, wave_counts=None, link_counts=None, times_ms=None):
    """what happened between consecutive samples, from `WaveRecorder.waves()` and `.links()` (or lists like them): a structured
    array with one row per sample, (t_ms, waves, births, deaths, splits, merges, continued).  With d+(p) and d-(q) the out- and
    in-degrees of the overlap graph between the samples s - 1 and s over the links of overlap >= `min_overlap`: a birth is a
    wave q of s with d- = 0, a death a wave p of s - 1 with d+ = 0, a split a p with d+ >= 2, a merge a q with d- >= 2, and
    `continued` counts the links whose two ends both have degree 1.  Row 0 has its waves and zeros.  The lists must be whole:
    with `wave_counts` / `link_counts` (the recorder's `counts()` / `link_counts()`) a cut list is refused by sample; a link
    that names a wave that is in no list is refused either way.  `times_ms`: the sample times where a sample may be empty."""
    _checked(waves_per_sample, links_per_sample, wave_counts, link_counts)
    out = np.zeros(len(waves_per_sample), EVENT_DTYPE)
    for s in range(len(out)):
        out['t_ms'][s] = _time_of(s, waves_per_sample, links_per_sample, times_ms)
        out['waves'][s] = len(waves_per_sample[s])
        if s == 0:
            continue
        P, Q, kept, dout, din = _graph(s, waves_per_sample, links_per_sample, min_overlap)
        out['births'][s] = sum(1 for q in Q if din[q] == 0)
        out['deaths'][s] = sum(1 for p in P if dout[p] == 0)
        out['splits'][s] = sum(1 for p in P if dout[p] >= 2)
        out['merges'][s] = sum(1 for q in Q if din[q] >= 2)
        out['continued'][s] = sum(1 for p, q in kept if dout[p] == 1 and din[q] == 1)
    return out


def track(waves_per_sample, links_per_sample, min_overlap=1, wave_counts=None, link_counts=None, times_ms=None):
    """the waves followed from sample to sample: a list of `Track`, ids in the order of first appearance (by sample, then by
    seed).  A track runs along `continued` links only (both ends of degree 1); every other link ends a track and starts
    another, and is kept as parent -> child.  A wave with several predecessors is born by 'merge' (whatever else its parents
    did), one whose single predecessor went on into several by 'split'.  The same lists and checks as `events`."""
    _checked(waves_per_sample, links_per_sample, wave_counts, link_counts)
    tracks, alive = [], {}                               # alive: seed in the latest sample -> track

    def point(s, rec):
        t = _time_of(s, waves_per_sample, links_per_sample, times_ms)
        names = rec.dtype.names
        if 'cy' in names:
            cy, cx = float(rec['cy']), float(rec['cx'])
        else:
            cy, cx = float(rec['sum_r']) / float(rec['area']), float(rec['sum_c']) / float(rec['area'])
        return (t, int(rec['seed']), int(rec['area']), cy, cx)

    for s in range(len(waves_per_sample)):
        W = waves_per_sample[s]
        now = {}
        if s == 0:
            for rec in W:
                t = Track(len(tracks), 'start')
                tracks.append(t)
                t.points.append(point(s, rec))
                now[int(rec['seed'])] = t
        else:
            P, Q, kept, dout, din = _graph(s, waves_per_sample, links_per_sample, min_overlap)
            before = {q: [] for q in Q}
            for p, q in kept:
                before[q].append(p)
            for rec in W:
                q = int(rec['seed'])
                ps = sorted(before[q])
                if len(ps) == 1 and dout[ps[0]] == 1:
                    t = alive[ps[0]]
                else:
                    t = Track(len(tracks), 'birth' if not ps else 'merge' if len(ps) >= 2 else 'split')
                    tracks.append(t)
                    for p in ps:
                        parent = alive[p]
                        t.parents.append(parent.id)
                        parent.children.append(t.id)
                        parent.ended = 'split' if dout[p] >= 2 else 'merge'
                t.points.append(point(s, rec))
                now[q] = t
            for p in P:
                if dout[p] == 0:
                    alive[p].ended = 'death'
        alive = now
    for t in tracks:
        t.parents.sort()
        t.children.sort()
        t.points = np.array(t.points, POINT_DTYPE)
    return tracks
