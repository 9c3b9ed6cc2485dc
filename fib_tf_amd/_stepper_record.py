"""the recorder and program bindings of `_lib.Stepper` (include/fibhip.h fibhip_observe_* ... fibhip_trig_*), as a mixin: what
the bindings repeat — an optional [height, width] plane, a window, a counter, a read of samples [first, first + count), a shape
query, a list of dicts turned into structs, a stack of planes — is written once at the top.  A pointer made by
ndarray.ctypes.data_as keeps its array alive, so the helpers hand back pointers."""
import ctypes as C

import numpy as np

from ._lib import (FRAME_FORMAT, FRAME_REDUCE, MAX_TRIG_RULES, MAX_TRIG_SENSORS, OBS_MAPS, STAT_KINDS, STIM_MODES, STIM_SHAPES, TRIG_EDGES,
                   TRIG_FIELDS, TRIG_SITES, WAVE_LINK_DTYPE, WAVE_RECORD_DTYPE, LesionEntry, StatCol, StimEntry, TrigRule, TrigSensor, _fp,
                   _ip)

_ubp = C.POINTER(C.c_ubyte)
_dp = C.POINTER(C.c_double)
_STIMULUS = (('mode', STIM_MODES), ('shape', STIM_SHAPES))             # the named fields of a stimulus and their enums


class RecorderBindings:
    """needs `_h`, `_L`, `_ck`, `_fallback_warning`, `height` and `width` of the class it is mixed into"""

    # ---- the repeated pieces ----------------------------------------------------------------------------------------
    def _plane(self, who, what, a, dtype):
        """the pointer to an optional [height, width] plane (`what`: 'weight plane', float32, or 'mask', uint8), or None"""
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        if a.shape != (self.height, self.width):
            raise ValueError('%s: a %s of shape %s on a %d x %d grid' % (who, what, a.shape, self.height, self.width))
        return a.ctypes.data_as(_ubp if dtype is np.uint8 else _fp)

    def _window(self, window):
        """the pointer to (r0, r1, c0, c1) as int[4]; None: the whole grid"""
        return np.ascontiguousarray((0, self.height, 0, self.width) if window is None else window, np.intc).reshape(4).ctypes.data_as(_ip)

    def _count(self, fn):
        k = C.c_longlong()
        self._ck(fn(self._h, C.byref(k)))
        return int(k.value)

    def _shape3(self, fn):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._ck(fn(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def _span(self, count_fn, first, count):
        """(first, count, rows to allocate) of a read; count=None: all taken so far"""
        if count is None:
            count = self._count(count_fn) - int(first)
        return int(first), int(count), max(int(count), 0)

    def _rows(self, count_fn, read_fn, first, count, tail_shape, dtype, ptr):
        """samples [first, first + count) of a recorder that keeps one row of `tail_shape` per sample"""
        first, count, n = self._span(count_fn, first, count)
        out = np.empty((n,) + tuple(tail_shape), dtype)
        self._ck(read_fn(self._h, first, count, out.ctypes.data_as(ptr)))
        return out

    def _lists(self, count_fn, read_fn, first, count, ncounts, tail_shape, dtype, ptr, records):
        """samples [first, first + count) of a recorder that keeps `ncounts` counters and a list of records per sample"""
        first, count, n = self._span(count_fn, first, count)
        counts = np.zeros((n, ncounts), np.int32)
        recs = np.zeros((n,) + tuple(tail_shape), dtype) if records else None
        self._ck(read_fn(self._h, first, count, counts.ctypes.data_as(_ip), recs.ctypes.data_as(ptr) if records else None))
        return counts, recs

    def _entries(self, arr, items, who, noun, names, ints):
        """fills the struct array `arr` from a list of dicts of stimulus-like entries: the fields of `names` = ((field, enum), ...)
        are names or numbers, hold and count default to 1, v and floor are floats, the fields of `ints` integers, fields left
        out 0; any other field is refused"""
        for i, e in enumerate(items):
            d = dict(e)
            for field, enum in names:
                val = d.pop(field, 0)
                setattr(arr[i], field, enum.index(val) if isinstance(val, str) else int(val))
            arr[i].hold, arr[i].count = int(d.pop('hold', 1)), int(d.pop('count', 1))
            arr[i].v, arr[i].floor = float(d.pop('v', 0.0)), float(d.pop('floor', 0.0))
            for k, val in d.items():
                if k not in ints:
                    raise ValueError('%s: %s %d: unknown field %r' % (who, noun, i, k))
                setattr(arr[i], k, int(val))
        return arr

    def _plane_stack(self, who, planes):
        """(how many, the pointer to them as one float32 [n, height, width] array) of a list of planes; (0, None) without one"""
        if planes is None or not len(planes):
            return 0, None
        for p in planes:
            if np.shape(p) != (self.height, self.width):
                raise ValueError('%s: a plane of shape %s on a %d x %d grid' % (who, np.shape(p), self.height, self.width))
        stack = np.ascontiguousarray(np.stack([np.asarray(p, np.float32) for p in planes]), np.float32)
        return len(stack), stack.ctypes.data_as(_fp)

    def _fit_maps(self, fn, first, shape, radius, max_dt, min_cells, mp):
        """the four maps of a velocity fit: `first` is the call's own leading argument (back, or which plane)"""
        nf = np.empty(shape, np.int32)
        gy, gx, rms = (np.empty(shape, np.float32) for _ in range(3))
        self._ck(fn(self._h, int(first), int(radius), float(np.float32(max_dt)), int(min_cells), mp, nf.ctypes.data_as(_ip),
                    gy.ctypes.data_as(_fp), gx.ctypes.data_as(_fp), rms.ctypes.data_as(_fp)))
        return nf, gy, gx, rms

    # ---- activation recorder (include/fibhip.h fibhip_observe_*) --------------------------------------------------
    def observe_begin(self, var, up, down):
        """attaches (or re-attaches, clearing the maps) the per-cell activation recorder on array `var`"""
        self._ck(self._L.fibhip_observe_begin(self._h, int(var), float(up), float(down)))

    def observe_get(self, which):
        """one map as a [height, width] array: 'first_up', 'last_up', 'prev_up', 'apd' (float32) or 'count' (int32)"""
        k = OBS_MAPS.index(which)
        out = np.empty((self.height, self.width), np.int32 if which == 'count' else np.float32)
        self._ck(self._L.fibhip_observe_get(self._h, k, out.ctypes.data_as(C.c_void_p)))
        return out

    def observe_ticks(self):
        """ticks observed since observe_begin"""
        return self._count(self._L.fibhip_observe_ticks)

    def observe_velocity(self, which, radius, max_dt, min_cells, mask=None):
        """(nfit int32, gy, gx, rms float32), each [height, width]: the velocity fit on the time plane `which` ('first_up',
        'last_up' or 'prev_up'); `mask`: [height, width], non-zero where a cell counts, or None"""
        mp = self._plane('observe_velocity', 'mask', mask, np.uint8)
        return self._fit_maps(self._L.fibhip_observe_velocity, OBS_MAPS.index(which), (self.height, self.width), radius, max_dt, min_cells, mp)

    def observe_end(self):
        self._ck(self._L.fibhip_observe_end(self._h))

    # ---- electrode recorder (include/fibhip.h fibhip_electrode_*) -------------------------------------------------
    def electrode_begin(self, var, rects, patches, every=1, capacity=1):
        """attaches (or re-attaches, with an empty trace) the electrode recorder on array `var`: `rects` is a list of
        (r0, r1, c0, c1), `patches` the float32 weight arrays of those shapes; one sample every `every` ticks, `capacity`
        samples at the most"""
        rects = np.ascontiguousarray(rects, np.intc).reshape(-1, 4)
        if len(patches) != len(rects):
            raise ValueError('electrode_begin: %d rectangles but %d weight patches' % (len(rects), len(patches)))
        flat = []
        for (r0, r1, c0, c1), w in zip(rects, patches):
            w = np.asarray(w, np.float32)
            if w.shape != (r1 - r0, c1 - c0):
                raise ValueError('electrode_begin: a patch of shape %s for rows [%d, %d) x columns [%d, %d)' % (w.shape, r0, r1, c0, c1))
            flat.append(w.ravel())
        weights = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(1), np.float32)
        self._ck(self._L.fibhip_electrode_begin(self._h, int(var), len(rects), rects.ctypes.data_as(_ip), weights.ctypes.data_as(_fp),
                                                int(every), int(capacity)))
        self._el_n = len(rects)

    def electrode_count(self):
        """samples taken since electrode_begin (ticks accepted but not launched yet included)"""
        return self._count(self._L.fibhip_electrode_count)

    def electrode_read(self, first=0, count=None):
        """samples [first, first + count) as a float32 [count, n] array (count=None: all taken so far); blocks like
        get_state, detaches nothing"""
        return self._rows(self._L.fibhip_electrode_count, self._L.fibhip_electrode_read, first, count, (getattr(self, '_el_n', 0),),
                          np.float32, _fp)

    def electrode_end(self):
        self._ck(self._L.fibhip_electrode_end(self._h))

    # ---- tip recorder (include/fibhip.h fibhip_tips_*) ------------------------------------------------------------
    def tips_begin(self, var, var2, a0, b0, mask=None, every=1, max_tips=256, capacity=1):
        """attaches (or re-attaches, with empty lists) the tip recorder on arrays `var`, `var2` with the levels `a0`, `b0`;
        `mask`: [height, width], non-zero where a cell counts, or None; one sample every `every` ticks, `capacity` samples of
        up to `max_tips` tips at the most"""
        mp = self._plane('tips_begin', 'mask', mask, np.uint8)
        self._ck(self._L.fibhip_tips_begin(self._h, int(var), int(var2), float(a0), float(b0), mp, int(every), int(max_tips),
                                           int(capacity)))
        self._tip_max = int(max_tips)

    def tips_count(self):
        """samples taken since tips_begin (ticks accepted but not launched yet included)"""
        return self._count(self._L.fibhip_tips_count)

    def tips_read(self, first=0, count=None, records=True):
        """samples [first, first + count) (count=None: all taken so far) as (counts, records): counts int32 [count, 3] =
        n_pos, n_neg, stored; records int32 [count, max_tips, 4] = row, column, charge, 0, of which the first
        min(stored, max_tips) of each sample are valid, in no fixed order (records=False: None).  Blocks like get_state,
        detaches nothing"""
        return self._lists(self._L.fibhip_tips_count, self._L.fibhip_tips_read, first, count, 3, (getattr(self, '_tip_max', 0), 4),
                           np.int32, _ip, records)

    def tips_end(self):
        self._ck(self._L.fibhip_tips_end(self._h))

    # ---- frame recorder (include/fibhip.h fibhip_frames_*) --------------------------------------------------------
    def frames_begin(self, var=0, window=None, block=(1, 1), reduce='mean', lo=0.0, span=1.0, weight=None, fmt='float32', every=1,
                     first=None, capacity=1):
        """attaches (or re-attaches, with an empty cube) the frame recorder on array `var`: `window` = (r0, r1, c0, c1) (None:
        the whole grid), `block` = (by, bx), `reduce` 'point' / 'mean', the levels of y = (X - lo) / span, `weight` an
        [height, width] float32 plane or None, `fmt` 'float32' / 'uint8'; a frame after ticks first, first + every, ...
        (first=None: every), `capacity` frames at the most"""
        win = self._window(window)
        wp = self._plane('frames_begin', 'weight plane', weight, np.float32)
        self._ck(self._L.fibhip_frames_begin(self._h, int(var), win, int(block[0]), int(block[1]),
                                             FRAME_REDUCE.index(reduce), float(lo), float(span), wp, FRAME_FORMAT.index(fmt),
                                             int(every), int(every if first is None else first), int(capacity)))

    def frames_count(self):
        """frames taken since frames_begin (ticks accepted but not launched yet included)"""
        return self._count(self._L.fibhip_frames_count)

    def frames_shape(self):
        """(oh, ow, dtype) of the attached recorder's frames"""
        oh, ow, bpp = self._shape3(self._L.fibhip_frames_shape)
        return oh, ow, np.dtype(np.uint8 if bpp == 1 else np.float32)

    def frames_read(self, first=0, count=None):
        """frames [first, first + count) as a [count, oh, ow] array of float32 or uint8 (count=None: all taken so far); blocks
        like get_state, detaches nothing"""
        first, count, _ = self._span(self._L.fibhip_frames_count, first, count)
        oh, ow, dtype = self.frames_shape()
        return self._rows(None, self._L.fibhip_frames_read, first, count, (oh, ow), dtype, C.c_void_p)

    def frames_end(self):
        self._ck(self._L.fibhip_frames_end(self._h))

    # ---- spectrum recorder (include/fibhip.h fibhip_spectrum_*) ----------------------------------------------------
    def spectrum_begin(self, var=0, window=None, block=(1, 1), reduce='mean', weight=None, every=1, nfft=128, win=None, tw=None,
                       bins=(2,), chunk=1):
        """attaches the spectrum recorder on array `var`: the frame recorder's `window`, `block`, `reduce` and `weight` (levels
        0 and 1), a sample every `every` ticks, segments of `nfft` samples weighted by `win` [nfft] float32, the twiddle table
        `tw` [nfft, 2] float32 (cos, -sin of 2 pi m / nfft), the strictly ascending frequency indices `bins` (at most 128, each
        in [0, nfft / 2]) and `chunk` (1 .. 32, a divisor of nfft): the samples folded by one launch"""
        wnd = self._window(window)
        wp = self._plane('spectrum_begin', 'weight plane', weight, np.float32)
        win = np.ascontiguousarray(win, np.float32)
        tw = np.ascontiguousarray(tw, np.float32)
        if win.shape != (int(nfft),) or tw.shape != (int(nfft), 2):
            raise ValueError('spectrum_begin: win must be [nfft] and tw [nfft, 2] (got %s and %s for nfft = %d)' % (win.shape, tw.shape, nfft))
        b = np.ascontiguousarray(bins, np.intc).reshape(-1)
        self._ck(self._L.fibhip_spectrum_begin(self._h, int(var), wnd, int(block[0]), int(block[1]),
                                               FRAME_REDUCE.index(reduce), wp, int(every), int(nfft), win.ctypes.data_as(_fp),
                                               tw.ctypes.data_as(_fp), int(b.size), b.ctypes.data_as(_ip), int(chunk)))

    def spectrum_count(self):
        """(samples taken, segments finished) since spectrum_begin (ticks accepted but not launched yet included)"""
        s, g = C.c_longlong(), C.c_longlong()
        self._ck(self._L.fibhip_spectrum_count(self._h, C.byref(s), C.byref(g)))
        return int(s.value), int(g.value)

    def spectrum_shape(self):
        """(oh, ow, nb) of the attached recorder"""
        return self._shape3(self._L.fibhip_spectrum_shape)

    def spectrum_read(self):
        """(P [nb, oh, ow] float32, segments): the power summed over the finished segments; blocks like get_state"""
        oh, ow, nb = self.spectrum_shape()
        out = np.empty((nb, oh, ow), np.float32)
        seg = C.c_longlong()
        self._ck(self._L.fibhip_spectrum_read(self._h, out.ctypes.data_as(_fp), C.byref(seg)))
        return out, int(seg.value)

    def spectrum_peak(self, a, b, halfwidth=1):
        """(kpeak int32, ppeak, pband, pnear float32), each [oh, ow], over the bin positions a <= i <= b"""
        oh, ow, _ = self.spectrum_shape()
        kp = np.empty((oh, ow), np.int32)
        pp, pb, pn = (np.empty((oh, ow), np.float32) for _ in range(3))
        self._ck(self._L.fibhip_spectrum_peak(self._h, int(a), int(b), int(halfwidth), kp.ctypes.data_as(_ip), pp.ctypes.data_as(_fp),
                                              pb.ctypes.data_as(_fp), pn.ctypes.data_as(_fp)))
        return kp, pp, pb, pn

    def spectrum_end(self):
        self._ck(self._L.fibhip_spectrum_end(self._h))

    # ---- beat recorder (include/fibhip.h fibhip_beats_*) -----------------------------------------------------------
    def beats_begin(self, var=0, window=None, block=(1, 1), reduce='mean', weight=None, every=1, up=0.5, down=0.1, depth=8):
        """attaches the beat recorder on array `var`: the frame recorder's `window`, `block`, `reduce` and `weight` (levels 0
        and 1), a sample every `every` ticks, the levels `down` <= `up` and a ring of `depth` (1 .. 16) beats per pixel"""
        wnd = self._window(window)
        wp = self._plane('beats_begin', 'weight plane', weight, np.float32)
        self._ck(self._L.fibhip_beats_begin(self._h, int(var), wnd, int(block[0]), int(block[1]),
                                            FRAME_REDUCE.index(reduce), wp, int(every), float(np.float32(up)), float(np.float32(down)),
                                            int(depth)))

    def beats_count(self):
        """samples taken since beats_begin (ticks accepted but not launched yet included)"""
        return self._count(self._L.fibhip_beats_count)

    def beats_shape(self):
        """(oh, ow, depth) of the attached recorder"""
        return self._shape3(self._L.fibhip_beats_shape)

    def beats_read(self):
        """(t_up, t_down, peak float32 [depth, oh, ow] in SLOT order — beat b in slot b % depth —, count int32 [oh, ow], pk
        float32 [oh, ow]); blocks like get_state"""
        oh, ow, d = self.beats_shape()
        tu, td, pe = (np.empty((d, oh, ow), np.float32) for _ in range(3))
        n = np.empty((oh, ow), np.int32)
        pk = np.empty((oh, ow), np.float32)
        self._ck(self._L.fibhip_beats_read(self._h, tu.ctypes.data_as(_fp), td.ctypes.data_as(_fp), pe.ctypes.data_as(_fp),
                                           n.ctypes.data_as(_ip), pk.ctypes.data_as(_fp)))
        return tu, td, pe, n, pk

    def beats_summary(self, last):
        """(nused int32, apd_mean, cl_mean, apd_alt float32), each [oh, ow], over the newest `last` beats"""
        oh, ow, _ = self.beats_shape()
        nu = np.empty((oh, ow), np.int32)
        am, cm, al = (np.empty((oh, ow), np.float32) for _ in range(3))
        self._ck(self._L.fibhip_beats_summary(self._h, int(last), nu.ctypes.data_as(_ip), am.ctypes.data_as(_fp), cm.ctypes.data_as(_fp),
                                              al.ctypes.data_as(_fp)))
        return nu, am, cm, al

    def beats_velocity(self, back, radius, max_dt, min_cells, mask=None):
        """(nfit int32, gy, gx, rms float32), each [oh, ow]: the velocity fit on the beat `back` beats before every pixel's
        newest; `mask`: [oh, ow] of the pixel plane, non-zero where a pixel counts, or None"""
        oh, ow, _ = self.beats_shape()
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.shape != (oh, ow):
                raise ValueError('beats_velocity: a mask of shape %s on a pixel plane of %d x %d' % (mask.shape, oh, ow))
            mp = mask.ctypes.data_as(_ubp)
        return self._fit_maps(self._L.fibhip_beats_velocity, back, (oh, ow), radius, max_dt, min_cells, mp)

    def beats_end(self):
        self._ck(self._L.fibhip_beats_end(self._h))

    # ---- statistics recorder (include/fibhip.h fibhip_stats_*) ----------------------------------------------------
    def stats_begin(self, cols, weight=None, mask=None, every=1, capacity=1):
        """attaches the statistics recorder: `cols` is a list of (var, kind, level) with kind one of STAT_KINDS (or its
        number), `weight` an [height, width] float32 plane or None (what SUM columns weigh with), `mask` an [height, width]
        array, non-zero where a cell counts for the other kinds, or None; one row of float64 every `every` ticks, `capacity`
        rows at the most"""
        arr = (StatCol * max(len(cols), 1))()
        for i, (var, kind, level) in enumerate(cols):
            arr[i].var, arr[i].kind = int(var), STAT_KINDS.index(kind) if isinstance(kind, str) else int(kind)
            arr[i].level = float(level)
        wp = self._plane('stats_begin', 'weight plane', weight, np.float32)
        mp = self._plane('stats_begin', 'mask', mask, np.uint8)
        self._ck(self._L.fibhip_stats_begin(self._h, len(cols), arr, wp, mp, int(every), int(capacity)))
        self._st_n = len(cols)

    def stats_count(self):
        """samples taken since stats_begin (ticks accepted but not launched yet included)"""
        return self._count(self._L.fibhip_stats_count)

    def stats_read(self, first=0, count=None):
        """samples [first, first + count) as a float64 [count, ncols] array (count=None: all taken so far); blocks like
        get_state, detaches nothing"""
        return self._rows(self._L.fibhip_stats_count, self._L.fibhip_stats_read, first, count, (getattr(self, '_st_n', 0),), np.float64, _dp)

    def stats_end(self):
        self._ck(self._L.fibhip_stats_end(self._h))

    # ---- lead recorder (include/fibhip.h fibhip_leads_*) ----------------------------------------------------------
    def leads_begin(self, pos, tables, weight=None, var=0, every=1, capacity=1):
        """attaches the lead recorder: `pos` is a list of (row, col, table), `tables` a float32 [ntables, height, width] array
        of lead-field tables, `weight` an [height, width] float32 plane or None (weight 1); one row of float64, one value per
        lead, every `every` ticks, `capacity` rows at the most"""
        pos = np.ascontiguousarray(pos, np.int32).reshape(-1, 3)
        tables = np.ascontiguousarray(tables, np.float32)
        if tables.ndim != 3 or tables.shape[1:] != (self.height, self.width):
            raise ValueError('leads_begin: tables of shape %s on a %d x %d grid' % (tables.shape, self.height, self.width))
        wp = self._plane('leads_begin', 'weight plane', weight, np.float32)
        self._ck(self._L.fibhip_leads_begin(self._h, int(var), len(pos), pos.ctypes.data_as(_ip), len(tables), tables.ctypes.data_as(_fp), wp,
                                            int(every), int(capacity)))
        self._ld_n = len(pos)

    def leads_count(self):
        """samples taken since leads_begin (ticks accepted but not launched yet included)"""
        return self._count(self._L.fibhip_leads_count)

    def leads_read(self, first=0, count=None):
        """samples [first, first + count) as a float64 [count, nleads] array (count=None: all taken so far); blocks like
        get_state, detaches nothing"""
        return self._rows(self._L.fibhip_leads_count, self._L.fibhip_leads_read, first, count, (getattr(self, '_ld_n', 0),), np.float64, _dp)

    def leads_end(self):
        self._ck(self._L.fibhip_leads_end(self._h))

    # ---- potential-map recorder (include/fibhip.h fibhip_pmap_*) ---------------------------------------------------
    def pmap_begin(self, table, weight=None, window=None, step=(1, 1), var=0, every=1, capacity=1):
        """attaches the potential-map recorder: `table` is the float32 [R + 1, R + 1] lead-field table (its shape gives the
        radius R), `weight` an [height, width] float32 plane or None (weight 1), `window` = (r0, r1, c0, c1) (None: the whole
        grid) and `step` = (sy, sx) the lattice of sites; one float64 [oh, ow] plane every `every` ticks, `capacity` planes at
        the most"""
        table = np.ascontiguousarray(table, np.float32)
        if table.ndim != 2 or table.shape[0] != table.shape[1] or table.shape[0] < 2:
            raise ValueError('pmap_begin: a table of shape %s is not [R + 1, R + 1]' % (table.shape,))
        win = np.ascontiguousarray((0, self.height, 0, self.width) if window is None else window, np.intc).reshape(4)
        sy, sx = int(step[0]), int(step[1])
        wp = self._plane('pmap_begin', 'weight plane', weight, np.float32)
        self._ck(self._L.fibhip_pmap_begin(self._h, int(var), table.shape[0] - 1, table.ctypes.data_as(_fp), wp, win.ctypes.data_as(_ip), sy, sx,
                                           int(every), int(capacity)))
        self._pm_shape = (-(-int(win[1] - win[0]) // sy), -(-int(win[3] - win[2]) // sx))

    def pmap_count(self):
        """samples taken since pmap_begin (ticks accepted but not launched yet included)"""
        return self._count(self._L.fibhip_pmap_count)

    def pmap_read(self, first=0, count=None):
        """samples [first, first + count) as a float64 [count, oh, ow] array (count=None: all taken so far); blocks like
        get_state, detaches nothing"""
        return self._rows(self._L.fibhip_pmap_count, self._L.fibhip_pmap_read, first, count, getattr(self, '_pm_shape', (0, 0)), np.float64, _dp)

    def pmap_summary(self, first=0, count=None):
        """(vmin, vmax, dmin float64, kmin, kmax, kd int32), each [oh, ow], over the samples [first, first + count) (count=None:
        all taken so far; at least 2)"""
        first, count, _ = self._span(self._L.fibhip_pmap_count, first, count)
        shape = getattr(self, '_pm_shape', (0, 0))
        f = [np.empty(shape, np.float64) for _ in range(3)]
        k = [np.empty(shape, np.int32) for _ in range(3)]
        self._ck(self._L.fibhip_pmap_summary(self._h, first, count, *([a.ctypes.data_as(_dp) for a in f] + [a.ctypes.data_as(_ip) for a in k])))
        return tuple(f + k)

    def pmap_end(self):
        self._ck(self._L.fibhip_pmap_end(self._h))

    # ---- wave recorder (include/fibhip.h fibhip_waves_*) ----------------------------------------------------------
    def waves_begin(self, var=0, kind=0, level=0.0, var2=-1, kind2=0, level2=0.0, conn=4, mask=None, max_waves=256, every=1, capacity=1):
        """attaches (or re-attaches, with empty lists) the wave recorder: a cell is set where `mask` ([height, width], or None:
        everywhere) is non-zero and array `var` is above (`kind` 0) or below (1) `level`, and array `var2` (-1: none) meets
        (`kind2`, `level2`) too; the connected components under `conn` = 4 or 8 are the waves; one sample every `every` ticks,
        `capacity` samples of up to `max_waves` records at the most"""
        mp = self._plane('waves_begin', 'mask', mask, np.uint8)
        self._ck(self._L.fibhip_waves_begin(self._h, int(var), int(kind), float(level), int(var2), int(kind2), float(level2), int(conn), mp,
                                            int(max_waves), int(every), int(capacity)))
        self._wave_max = int(max_waves)
        self._wave_link_max = 0

    def waves_links_begin(self, max_links=512):
        """turns links on for the wave recorder just attached (before its first tick): per sample, which waves of the sample
        before share cells with which waves of this one, up to `max_links` records (prev, seed, overlap)"""
        self._ck(self._L.fibhip_waves_links_begin(self._h, int(max_links)))
        self._wave_link_max = int(max_links)

    def waves_links_read(self, first=0, count=None, records=True):
        """samples [first, first + count) (count=None: all taken so far) as (counts, links): counts int32 [count, 4] = links,
        stored, cells, lost; links WAVE_LINK_DTYPE [count, max_links], of which the first `stored` of each sample are valid, in
        no fixed order (records=False: None).  Blocks like waves_read; refused while links are off"""
        return self._lists(self._L.fibhip_waves_count, self._L.fibhip_waves_links_read, first, count, 4, (getattr(self, '_wave_link_max', 0),),
                           WAVE_LINK_DTYPE, C.c_void_p, records)

    def waves_count(self):
        """samples taken since waves_begin (ticks accepted but not launched yet included)"""
        return self._count(self._L.fibhip_waves_count)

    def waves_read(self, first=0, count=None, records=True):
        """samples [first, first + count) (count=None: all taken so far) as (counts, records): counts int32 [count, 3] = n,
        stored, cells; records WAVE_RECORD_DTYPE [count, max_waves], of which the first `stored` of each sample are valid, in
        no fixed order (records=False: None).  Blocks like get_state, detaches nothing"""
        return self._lists(self._L.fibhip_waves_count, self._L.fibhip_waves_read, first, count, 3, (getattr(self, '_wave_max', 0),),
                           WAVE_RECORD_DTYPE, C.c_void_p, records)

    def waves_labels(self):
        """the label plane of the latest sample: int32 [height, width], the seed of the cell's wave or -1"""
        out = np.empty((self.height, self.width), np.int32)
        self._ck(self._L.fibhip_waves_labels(self._h, out.ctypes.data_as(_ip)))
        return out

    def waves_end(self):
        self._ck(self._L.fibhip_waves_end(self._h))
        self._wave_link_max = 0

    # ---- stimulus program (include/fibhip.h fibhip_stim_*) --------------------------------------------------------
    def stim_begin(self, entries, planes=None):
        """attaches a stimulus program: `entries` is a list of dicts with the fields of fibhip_stim_entry (`mode` 'max' / 'add'
        or its number, `shape` 'rect' / 'plane' or its number; fields left out are 0, hold and count 1), `planes` a list of
        [height, width] float32 arrays the 'plane' entries index"""
        arr = self._entries((StimEntry * max(len(entries), 1))(), entries, 'stim_begin', 'entry', _STIMULUS,
                            ('var', 'r0', 'r1', 'c0', 'c1', 'plane', 'first', 'period'))
        nplanes, pp = self._plane_stack('stim_begin', planes)
        self._ck(self._L.fibhip_stim_begin(self._h, len(entries), arr, nplanes, pp))

    def stim_count(self):
        """events applied since stim_begin (flushes: the ticks accepted so far are launched first)"""
        return self._count(self._L.fibhip_stim_count)

    def stim_end(self):
        self._ck(self._L.fibhip_stim_end(self._h))

    # ---- lesion program (include/fibhip.h fibhip_lesion_*) --------------------------------------------------------
    def lesion_begin(self, lesions):
        """attaches a lesion program: `lesions` is a list of (tick, (r0, r1, c0, c1), patch) — the patch a float32
        [r1 - r0, c1 - c0] array of factors in [0, 1] — applied to the phase field right after tick `tick`, in list order"""
        arr = (LesionEntry * max(len(lesions), 1))()
        flat, off = [], 0
        for i, (tick, box, patch) in enumerate(lesions):
            r0, r1, c0, c1 = (int(a) for a in box)
            p = np.ascontiguousarray(patch, np.float32)
            if p.shape != (r1 - r0, c1 - c0):
                raise ValueError('lesion_begin: entry %d: a patch of shape %s on the box rows [%d, %d) x columns [%d, %d)' % (i, p.shape, r0, r1, c0, c1))
            arr[i].offset, arr[i].tick = off, int(tick)
            arr[i].r0, arr[i].r1, arr[i].c0, arr[i].c1 = r0, r1, c0, c1
            flat.append(p.ravel())
            off += p.size
        packed = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(1), np.float32)
        self._ck(self._L.fibhip_lesion_begin(self._h, len(lesions), arr, off, packed.ctypes.data_as(_fp)))

    def lesion_count(self):
        """entries applied since lesion_begin (ticks accepted but not launched yet count)"""
        return self._count(self._L.fibhip_lesion_count)

    def lesion_end(self):
        self._ck(self._L.fibhip_lesion_end(self._h))

    def lesion_apply(self, box, patch):
        """one lesion now: phi = max(phi * patch, 1e-5) on the box (r0, r1, c0, c1), the derived planes recomputed around it"""
        b = np.asarray([int(a) for a in box], np.int32)
        p = np.ascontiguousarray(patch, np.float32)
        if b.shape != (4,) or p.shape != (int(b[1] - b[0]), int(b[3] - b[2])):
            raise ValueError('lesion_apply: a patch of shape %s on the box %s' % (p.shape, tuple(int(a) for a in b)))
        self._ck(self._L.fibhip_lesion_apply(self._h, b.ctypes.data_as(_ip), p.ctypes.data_as(_fp)))
        self._fallback_warning()

    def get_phase(self):
        """the handle's current phase field, float32 [height, width]"""
        out = np.empty((self.height, self.width), np.float32)
        self._ck(self._L.fibhip_get_phase(self._h, out.ctypes.data_as(_fp)))
        self._fallback_warning()
        return out

    # ---- trigger program (include/fibhip.h fibhip_trig_*) ---------------------------------------------------------
    def trig_begin(self, sensors, rules, planes=None, every=1, capacity=4096):
        """attaches a trigger program: `sensors` is a list of dicts with the fields of fibhip_trig_sensor (`site` 'rect' with r0,
        r1, c0, c1, or 'mask' with `mask`, a [height, width] array whose non-zero cells are the site), `rules` a list of dicts
        with the fields of fibhip_trig_rule (`edge` 'rise' / 'fall', `mode` 'max' / 'add', `shape` 'rect' / 'plane', or their
        numbers; fields left out are 0, count and hold 1), `planes` the [height, width] float32 arrays the 'plane' stimuli index"""
        sa = (TrigSensor * max(len(sensors), 1))()
        masks = []
        for i, q in enumerate(sensors[:MAX_TRIG_SENSORS]):
            d = dict(q)
            site = d.pop('site', 0)
            sa[i].site = TRIG_SITES.index(site) if isinstance(site, str) else int(site)
            sa[i].level, sa[i].need = float(d.pop('level', 0.0)), int(d.pop('need', 1))
            mask = d.pop('mask', None)
            if sa[i].site == 1:
                if mask is None or np.shape(mask) != (self.height, self.width):
                    raise ValueError('trig_begin: sensor %d: a mask of shape %s on a %d x %d grid' % (i, np.shape(mask), self.height, self.width))
                masks.append((np.asarray(mask) != 0).astype(np.uint8))
            for k, val in d.items():
                if k not in ('var', 'r0', 'r1', 'c0', 'c1'):
                    raise ValueError('trig_begin: sensor %d: unknown field %r' % (i, k))
                setattr(sa[i], k, int(val))
        ra = self._entries((TrigRule * max(len(rules), 1))(), rules[:MAX_TRIG_RULES], 'trig_begin', 'rule', (('edge', TRIG_EDGES),) + _STIMULUS,
                           ('sensor', 'arm', 'blank', 'escape', 'max_det', 'delay', 'period', 'var', 'r0', 'r1', 'c0', 'c1', 'plane'))
        mp = np.ascontiguousarray(np.stack(masks), np.uint8).ctypes.data_as(_ubp) if masks else None
        nplanes, pp = self._plane_stack('trig_begin', planes)
        self._ck(self._L.fibhip_trig_begin(self._h, len(sensors), sa, mp, len(rules), ra, nplanes, pp, int(every), int(capacity)))
        self._trig_n = len(rules)

    def trig_count(self):
        """samples taken since trig_begin (ticks accepted but not launched yet included)"""
        return self._count(self._L.fibhip_trig_count)

    def trig_read(self, first=0, count=None):
        """rows [first, first + count) of the log as an int32 [count, nrules, 6] array — c, a, t, n, cause, fired — (count=None:
        all taken so far); blocks like get_state, detaches nothing"""
        return self._rows(self._L.fibhip_trig_count, self._L.fibhip_trig_read, first, count, (getattr(self, '_trig_n', 0), len(TRIG_FIELDS)),
                          np.int32, _ip)

    def trig_end(self):
        self._ck(self._L.fibhip_trig_end(self._h))
