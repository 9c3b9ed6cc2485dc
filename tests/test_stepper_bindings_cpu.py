"""not-gpu: what every recorder binding of `_lib.Stepper` hands to the C functions, and what it hands back.

A `Stepper` made without a device (`Stepper.__new__`) is given a recording stand-in for the loaded library: a plain Python
object whose `fibhip_*` attributes decode their arguments DURING the call — scalars as they come, pointers through
np.ctypeslib.as_array, struct arrays by indexing —, fill the out-parameters with a known byte pattern and return 0.  Every
test calls a recorder's bindings with arguments that are not the defaults, on a grid that is not square, and compares the log:
the scalars in order (the enum numbers the names become included), the dtype, shape and bytes of every array and struct field,
None where an optional plane is absent, and the dtype, shape and bytes of every array that comes back.  The host-side
refusals are pinned with their full messages."""
import ctypes as C

import numpy as np
import pytest

from fib_tf_amd import _lib

H, W = 6, 8                     # not square: a transposed shape cannot pass
HANDLE = 0x5eed
SAMPLES = 3                     # what every *_count reports
OH, OW = 3, 4                   # what every *_shape reports
FP, IP, UBP, DP, VP = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_ubyte), C.POINTER(C.c_double), C.c_void_p


def f32(x):
    return float(np.float32(x))


def pattern(seed, dtype, shape):
    """the bytes the stand-in writes into an out-array"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return ((seed * 37 + np.arange(n)) % 251).astype(np.uint8).view(dtype).reshape(shape)


def view(p, ctype, dtype, shape):
    """the memory behind a pointer argument as an array; the pointer's ctypes type is part of what is pinned"""
    assert isinstance(p, ctype), (type(p), ctype)
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    if n == 0:
        return np.empty(shape, dtype)
    keep = getattr(p, '_arr', None)                     # (ndarray.ctypes.data_as keeps its array: never look past its end)
    assert keep is None or keep.nbytes >= n, (keep.nbytes, n)
    return np.ctypeslib.as_array(C.cast(p, UBP), shape=(n,)).view(dtype).reshape(shape)


def read(p, ctype, dtype, shape):
    return None if p is None else view(p, ctype, dtype, shape).copy()


def fill(p, ctype, dtype, shape, seed):
    if p is None:
        return None
    view(p, ctype, dtype, shape)[...] = pattern(seed, dtype, shape)
    return 'out %s %s' % (np.dtype(dtype).name if np.dtype(dtype).names is None else 'struct', tuple(shape))


def put(ref, ctype, value):
    """fills a ctypes.byref out-parameter"""
    assert isinstance(ref._obj, ctype), type(ref._obj)
    ref._obj.value = value
    return 'ref'


def structs(arr, ctype, n):
    """the first n elements of a ctypes struct array as dicts"""
    assert arr._type_ is ctype and len(arr) == max(n, 1)
    return [{f: getattr(arr[i], f) for f, _ in ctype._fields_} for i in range(n)]


class FakeLibrary:
    """stands where the loaded library stands; `log` is [(name, decoded arguments after the handle)]"""

    def __init__(self):
        self.log = []
        self.bpp = 4
        self.tail = {'electrode': (2,), 'tips': (5, 4), 'stats': (3,), 'leads': (2,), 'waves': (7,), 'links': (9,), 'trig': (2, 6)}

    def __getattr__(self, name):
        if not name.startswith('fibhip_'):
            raise AttributeError(name)

        def call(h, *args):
            assert isinstance(h, C.c_void_p) and h.value == HANDLE
            fn = getattr(self, '_' + name[len('fibhip_'):], None)
            if fn is None and name.endswith('_count'):
                fn = self._count
            self.log.append((name, tuple(args) if fn is None else tuple(fn(*args))))
            return 0
        return call

    def rows(self, count, key):
        return (max(count, 0),) + self.tail[key]

    # ---- shared shapes ---------------------------------------------------------------------------------------------
    def _count(self, ref):
        return (put(ref, C.c_longlong, SAMPLES),)

    def _shape3(self, third, a, b, c):
        return put(a, C.c_int, OH), put(b, C.c_int, OW), put(c, C.c_int, third)

    # ---- activation ------------------------------------------------------------------------------------------------
    def _observe_get(self, k, out):
        return k, fill(out, VP, np.int32 if k == 4 else np.float32, (H, W), k)

    def _observe_ticks(self, ref):
        return (put(ref, C.c_longlong, 7),)

    # ---- electrodes ------------------------------------------------------------------------------------------------
    def _electrode_begin(self, var, n, rects, weights, every, capacity):
        r = read(rects, IP, np.intc, (n, 4))
        return var, n, r, read(weights, FP, np.float32, (max(sum((a[1] - a[0]) * (a[3] - a[2]) for a in r), 1),)), every, capacity

    def _electrode_read(self, first, count, out):
        return first, count, fill(out, FP, np.float32, self.rows(count, 'electrode'), 1)

    # ---- tips ------------------------------------------------------------------------------------------------------
    def _tips_begin(self, var, var2, a0, b0, mask, every, max_tips, capacity):
        return var, var2, a0, b0, read(mask, UBP, np.uint8, (H, W)), every, max_tips, capacity

    def _tips_read(self, first, count, counts, recs):
        return first, count, fill(counts, IP, np.int32, (max(count, 0), 3), 2), fill(recs, IP, np.int32, self.rows(count, 'tips'), 3)

    # ---- frames ----------------------------------------------------------------------------------------------------
    def _frames_begin(self, var, win, by, bx, reduce, lo, span, weight, fmt, every, first, capacity):
        return var, read(win, IP, np.intc, (4,)), by, bx, reduce, lo, span, read(weight, FP, np.float32, (H, W)), fmt, every, first, capacity

    def _frames_shape(self, a, b, c):
        return self._shape3(self.bpp, a, b, c)

    def _frames_read(self, first, count, out):
        return first, count, fill(out, VP, np.uint8 if self.bpp == 1 else np.float32, (max(count, 0), OH, OW), 4)

    # ---- spectrum --------------------------------------------------------------------------------------------------
    def _spectrum_begin(self, var, wnd, by, bx, reduce, weight, every, nfft, win, tw, nb, bins, chunk):
        return (var, read(wnd, IP, np.intc, (4,)), by, bx, reduce, read(weight, FP, np.float32, (H, W)), every, nfft,
                read(win, FP, np.float32, (nfft,)), read(tw, FP, np.float32, (nfft, 2)), nb, read(bins, IP, np.intc, (nb,)), chunk)

    def _spectrum_count(self, s, g):
        return put(s, C.c_longlong, 5), put(g, C.c_longlong, 2)

    def _spectrum_shape(self, a, b, c):
        return self._shape3(2, a, b, c)

    def _spectrum_read(self, out, seg):
        return fill(out, FP, np.float32, (2, OH, OW), 5), put(seg, C.c_longlong, 2)

    def _spectrum_peak(self, a, b, hw, kp, pp, pb, pn):
        return (a, b, hw, fill(kp, IP, np.int32, (OH, OW), 6)) + tuple(fill(p, FP, np.float32, (OH, OW), 7 + i) for i, p in enumerate((pp, pb, pn)))

    # ---- beats -----------------------------------------------------------------------------------------------------
    def _beats_begin(self, var, wnd, by, bx, reduce, weight, every, up, down, depth):
        return var, read(wnd, IP, np.intc, (4,)), by, bx, reduce, read(weight, FP, np.float32, (H, W)), every, up, down, depth

    def _beats_shape(self, a, b, c):
        return self._shape3(5, a, b, c)

    def _beats_read(self, tu, td, pe, n, pk):
        return tuple(fill(p, FP, np.float32, (5, OH, OW), 10 + i) for i, p in enumerate((tu, td, pe))) + (
            fill(n, IP, np.int32, (OH, OW), 13), fill(pk, FP, np.float32, (OH, OW), 14))

    def _beats_summary(self, last, nu, am, cm, al):
        return (last, fill(nu, IP, np.int32, (OH, OW), 15)) + tuple(fill(p, FP, np.float32, (OH, OW), 16 + i) for i, p in enumerate((am, cm, al)))

    # ---- statistics, leads -----------------------------------------------------------------------------------------
    def _stats_begin(self, n, cols, weight, mask, every, capacity):
        return n, structs(cols, _lib.StatCol, n), read(weight, FP, np.float32, (H, W)), read(mask, UBP, np.uint8, (H, W)), every, capacity

    def _stats_read(self, first, count, out):
        return first, count, fill(out, DP, np.float64, self.rows(count, 'stats'), 20)

    def _leads_begin(self, var, n, pos, ntab, tables, weight, every, capacity):
        return var, n, read(pos, IP, np.int32, (n, 3)), ntab, read(tables, FP, np.float32, (ntab, H, W)), read(weight, FP, np.float32, (H, W)), every, capacity

    def _leads_read(self, first, count, out):
        return first, count, fill(out, DP, np.float64, self.rows(count, 'leads'), 21)

    # ---- waves -----------------------------------------------------------------------------------------------------
    def _waves_begin(self, var, kind, level, var2, kind2, level2, conn, mask, max_waves, every, capacity):
        return var, kind, level, var2, kind2, level2, conn, read(mask, UBP, np.uint8, (H, W)), max_waves, every, capacity

    def _waves_read(self, first, count, counts, recs):
        return first, count, fill(counts, IP, np.int32, (max(count, 0), 3), 22), fill(recs, VP, _lib.WAVE_RECORD_DTYPE, self.rows(count, 'waves'), 23)

    def _waves_links_read(self, first, count, counts, recs):
        return first, count, fill(counts, IP, np.int32, (max(count, 0), 4), 24), fill(recs, VP, _lib.WAVE_LINK_DTYPE, self.rows(count, 'links'), 25)

    def _waves_labels(self, out):
        return (fill(out, IP, np.int32, (H, W), 26),)

    # ---- programs --------------------------------------------------------------------------------------------------
    def _stim_begin(self, n, entries, nplanes, planes):
        return n, structs(entries, _lib.StimEntry, n), nplanes, read(planes, FP, np.float32, (nplanes, H, W))

    def _lesion_begin(self, n, entries, floats, packed):
        return n, structs(entries, _lib.LesionEntry, n), floats, read(packed, FP, np.float32, (max(floats, 1),))

    def _lesion_apply(self, box, p):
        b = read(box, IP, np.int32, (4,))
        return b, read(p, FP, np.float32, (b[1] - b[0], b[3] - b[2]))

    def _get_phase(self, out):
        return (fill(out, FP, np.float32, (H, W), 27),)

    def _trig_begin(self, ns, sensors, masks, nr, rules, nplanes, planes, every, capacity):
        s = structs(sensors, _lib.TrigSensor, ns)
        return (ns, s, read(masks, UBP, np.uint8, (sum(q['site'] == 1 for q in s), H, W)), nr, structs(rules, _lib.TrigRule, nr), nplanes,
                read(planes, FP, np.float32, (nplanes, H, W)), every, capacity)

    def _trig_read(self, first, count, out):
        return first, count, fill(out, IP, np.int32, self.rows(count, 'trig'), 28)


def make():
    L = FakeLibrary()
    st = _lib.Stepper.__new__(_lib.Stepper)
    st._h, st._L, st.height, st.width, st.nvar, st._warned = C.c_void_p(HANDLE), L, H, W, 4, True
    return st, L


def same(got, want):
    if isinstance(want, np.ndarray):
        return isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    if isinstance(want, (list, tuple)):
        return type(got) is type(want) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if isinstance(want, dict):
        return isinstance(got, dict) and sorted(got) == sorted(want) and all(same(got[k], want[k]) for k in want)
    return type(got) is type(want) and got == want


def calls(L, *want):
    """the log is exactly `want`, [(name without the prefix, arguments)], and is emptied"""
    got, L.log = L.log, []
    assert [g[0] for g in got] == ['fibhip_' + w[0] for w in want]
    for g, w in zip(got, want):
        assert same(g[1], tuple(w[1:])), (g, w)


def back(got, seed, dtype, shape):
    """an array that came back is the stand-in's pattern, with the dtype and shape the binding promises"""
    assert same(got, pattern(seed, dtype, shape)), (got.dtype, got.shape)


def refused(message, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert str(e.value) == message


def plane(seed=0, dtype=np.float64):
    return (np.arange(H * W).reshape(H, W) * 0.25 + seed).astype(dtype)


WINDOW = (1, 5, 2, 8)
ENDS = ('observe', 'electrode', 'tips', 'frames', 'spectrum', 'beats', 'stats', 'leads', 'waves', 'stim', 'lesion', 'trig')
COUNTS = ('electrode', 'tips', 'frames', 'beats', 'stats', 'leads', 'waves', 'stim', 'lesion', 'trig')


@pytest.mark.parametrize('name', ENDS)
def test_end(name):
    st, L = make()
    assert getattr(st, name + '_end')() is None
    calls(L, (name + '_end',))


@pytest.mark.parametrize('name', COUNTS)
def test_count(name):
    st, L = make()
    got = getattr(st, name + '_count')()
    assert type(got) is int and got == SAMPLES
    calls(L, (name + '_count', 'ref'))


def test_activation():
    st, L = make()
    st.observe_begin(np.int64(2), np.float32(0.3), 0.125)
    calls(L, ('observe_begin', 2, f32(0.3), 0.125))
    for k, which in enumerate(_lib.OBS_MAPS):
        dtype = np.int32 if which == 'count' else np.float32
        back(st.observe_get(which), k, dtype, (H, W))
        calls(L, ('observe_get', k, 'out %s %s' % (np.dtype(dtype).name, (H, W))))
    got = st.observe_ticks()
    assert type(got) is int and got == 7
    calls(L, ('observe_ticks', 'ref'))


def test_electrodes():
    st, L = make()
    L.tail['electrode'] = (0,)
    back(st.electrode_read(0, 2), 1, np.float32, (2, 0))                     # before any electrode_begin: no electrode, and the call is made
    calls(L, ('electrode_read', 0, 2, 'out float32 (2, 0)'))
    L.tail['electrode'] = (2,)
    p0, p1 = np.arange(6.0).reshape(2, 3), np.arange(4, dtype=np.int64).reshape(4, 1) + 0.5
    st.electrode_begin(3, [(1, 3, 2, 5), (0, 4, 7, 8)], [p0, p1], every=5, capacity=11)
    calls(L, ('electrode_begin', 3, 2, np.array([[1, 3, 2, 5], [0, 4, 7, 8]], np.intc),
              np.concatenate([p0.ravel(), p1.ravel()]).astype(np.float32), 5, 11))
    back(st.electrode_read(1, 2), 1, np.float32, (2, 2))
    calls(L, ('electrode_read', 1, 2, 'out float32 (2, 2)'))
    back(st.electrode_read(1), 1, np.float32, (SAMPLES - 1, 2))              # count=None: all taken so far
    calls(L, ('electrode_count', 'ref'), ('electrode_read', 1, SAMPLES - 1, 'out float32 (2, 2)'))
    back(st.electrode_read(5), 1, np.float32, (0, 2))                        # past the end: the count goes through as it is
    calls(L, ('electrode_count', 'ref'), ('electrode_read', 5, SAMPLES - 5, 'out float32 (0, 2)'))
    st.electrode_begin(0, [], [])
    calls(L, ('electrode_begin', 0, 0, np.zeros((0, 4), np.intc), np.zeros(1, np.float32), 1, 1))
    refused('electrode_begin: 2 rectangles but 1 weight patches', st.electrode_begin, 0, [(0, 1, 0, 1), (0, 1, 0, 1)], [np.ones((1, 1))])
    refused('electrode_begin: a patch of shape (3, 2) for rows [1, 3) x columns [2, 5)', st.electrode_begin, 0, [(1, 3, 2, 5)], [p0.T])
    calls(L)


def test_tips():
    st, L = make()
    mask = (np.arange(H * W).reshape(H, W) % 3).astype(np.int64)           # 0, 1, 2: converted to uint8, not to 0 / 1
    st.tips_begin(0, 2, 0.3, np.float32(0.7), mask=mask, every=4, max_tips=5, capacity=9)
    calls(L, ('tips_begin', 0, 2, 0.3, f32(0.7), mask.astype(np.uint8), 4, 5, 9))
    st.tips_begin(1, 3, 0.5, 0.25)
    calls(L, ('tips_begin', 1, 3, 0.5, 0.25, None, 1, 256, 1))
    L.tail['tips'] = (256, 4)
    counts, recs = st.tips_read(1, 2)
    back(counts, 2, np.int32, (2, 3))
    back(recs, 3, np.int32, (2, 256, 4))
    calls(L, ('tips_read', 1, 2, 'out int32 (2, 3)', 'out int32 (2, 256, 4)'))
    counts, recs = st.tips_read(records=False)
    back(counts, 2, np.int32, (SAMPLES, 3))
    assert recs is None
    calls(L, ('tips_count', 'ref'), ('tips_read', 0, SAMPLES, 'out int32 (3, 3)', None))
    refused('tips_begin: a mask of shape (8, 6) on a 6 x 8 grid', st.tips_begin, 0, 1, 0.0, 0.0, mask=mask.T)
    calls(L)


@pytest.mark.parametrize('bpp', [4, 1])
def test_frames(bpp):
    st, L = make()
    L.bpp = bpp
    st.frames_begin(2, window=WINDOW, block=(2, 3), reduce='mean', lo=0.1, span=2.5, weight=plane(1), fmt='uint8', every=6, first=4,
                    capacity=12)
    calls(L, ('frames_begin', 2, np.array(WINDOW, np.intc), 2, 3, 1, 0.1, 2.5, plane(1, np.float32), 1, 6, 4, 12))
    st.frames_begin(reduce='point')
    calls(L, ('frames_begin', 0, np.array((0, H, 0, W), np.intc), 1, 1, 0, 0.0, 1.0, None, 0, 1, 1, 1))
    st.frames_begin(every=7)                                                  # first=None: every
    calls(L, ('frames_begin', 0, np.array((0, H, 0, W), np.intc), 1, 1, 1, 0.0, 1.0, None, 0, 7, 7, 1))
    dtype = np.dtype(np.uint8 if bpp == 1 else np.float32)
    assert st.frames_shape() == (OH, OW, dtype) and [type(v) for v in st.frames_shape()[:2]] == [int, int]
    calls(L, ('frames_shape', 'ref', 'ref', 'ref'), ('frames_shape', 'ref', 'ref', 'ref'))
    back(st.frames_read(1, 2), 4, dtype, (2, OH, OW))
    calls(L, ('frames_shape', 'ref', 'ref', 'ref'), ('frames_read', 1, 2, 'out %s (2, 3, 4)' % dtype.name))
    back(st.frames_read(1), 4, dtype, (SAMPLES - 1, OH, OW))
    calls(L, ('frames_count', 'ref'), ('frames_shape', 'ref', 'ref', 'ref'), ('frames_read', 1, SAMPLES - 1, 'out %s (2, 3, 4)' % dtype.name))
    refused('frames_begin: a weight plane of shape (8, 6) on a 6 x 8 grid', st.frames_begin, weight=plane().T)
    calls(L)


def test_spectrum():
    st, L = make()
    win, tw = np.arange(8) / 8.0, np.arange(16).reshape(8, 2) / 16.0
    st.spectrum_begin(1, window=WINDOW, block=(2, 1), reduce='point', weight=plane(2), every=3, nfft=8, win=win, tw=tw, bins=(2, 3, 4), chunk=4)
    calls(L, ('spectrum_begin', 1, np.array(WINDOW, np.intc), 2, 1, 0, plane(2, np.float32), 3, 8, win.astype(np.float32), tw.astype(np.float32),
              3, np.array((2, 3, 4), np.intc), 4))
    st.spectrum_begin(nfft=8, win=win, tw=tw)
    calls(L, ('spectrum_begin', 0, np.array((0, H, 0, W), np.intc), 1, 1, 1, None, 1, 8, win.astype(np.float32), tw.astype(np.float32), 1,
              np.array((2,), np.intc), 1))
    got = st.spectrum_count()
    assert got == (5, 2) and [type(v) for v in got] == [int, int]
    calls(L, ('spectrum_count', 'ref', 'ref'))
    got = st.spectrum_shape()
    assert got == (OH, OW, 2) and [type(v) for v in got] == [int, int, int]
    calls(L, ('spectrum_shape', 'ref', 'ref', 'ref'))
    P, seg = st.spectrum_read()
    back(P, 5, np.float32, (2, OH, OW))
    assert type(seg) is int and seg == 2
    calls(L, ('spectrum_shape', 'ref', 'ref', 'ref'), ('spectrum_read', 'out float32 (2, 3, 4)', 'ref'))
    kp, pp, pb, pn = st.spectrum_peak(1, np.int64(2), halfwidth=3)
    back(kp, 6, np.int32, (OH, OW))
    for i, a in enumerate((pp, pb, pn)):
        back(a, 7 + i, np.float32, (OH, OW))
    calls(L, ('spectrum_shape', 'ref', 'ref', 'ref'), ('spectrum_peak', 1, 2, 3, 'out int32 (3, 4)') + ('out float32 (3, 4)',) * 3)
    refused('spectrum_begin: a weight plane of shape (8, 6) on a 6 x 8 grid', st.spectrum_begin, weight=plane().T, nfft=8, win=win, tw=tw)
    refused('spectrum_begin: win must be [nfft] and tw [nfft, 2] (got (8,) and (2, 8) for nfft = 8)', st.spectrum_begin, nfft=8, win=win, tw=tw.T)
    refused('spectrum_begin: win must be [nfft] and tw [nfft, 2] (got (8,) and (8, 2) for nfft = 4)', st.spectrum_begin, nfft=4, win=win, tw=tw)
    calls(L)


def test_beats():
    st, L = make()
    st.beats_begin(1, window=WINDOW, block=(3, 2), reduce='point', weight=plane(3), every=4, up=0.3, down=0.1, depth=5)
    calls(L, ('beats_begin', 1, np.array(WINDOW, np.intc), 3, 2, 0, plane(3, np.float32), 4, f32(0.3), f32(0.1), 5))
    st.beats_begin()
    calls(L, ('beats_begin', 0, np.array((0, H, 0, W), np.intc), 1, 1, 1, None, 1, 0.5, f32(0.1), 8))
    got = st.beats_shape()
    assert got == (OH, OW, 5) and [type(v) for v in got] == [int, int, int]
    calls(L, ('beats_shape', 'ref', 'ref', 'ref'))
    tu, td, pe, n, pk = st.beats_read()
    for i, a in enumerate((tu, td, pe)):
        back(a, 10 + i, np.float32, (5, OH, OW))
    back(n, 13, np.int32, (OH, OW))
    back(pk, 14, np.float32, (OH, OW))
    calls(L, ('beats_shape', 'ref', 'ref', 'ref'), ('beats_read',) + ('out float32 (5, 3, 4)',) * 3 + ('out int32 (3, 4)', 'out float32 (3, 4)'))
    nu, am, cm, al = st.beats_summary(np.int64(4))
    back(nu, 15, np.int32, (OH, OW))
    for i, a in enumerate((am, cm, al)):
        back(a, 16 + i, np.float32, (OH, OW))
    calls(L, ('beats_shape', 'ref', 'ref', 'ref'), ('beats_summary', 4, 'out int32 (3, 4)') + ('out float32 (3, 4)',) * 3)
    refused('beats_begin: a weight plane of shape (8, 6) on a 6 x 8 grid', st.beats_begin, weight=plane().T)
    calls(L)


def test_stats():
    st, L = make()
    mask = np.arange(H * W).reshape(H, W) % 3
    st.stats_begin([(0, 'sum', 0.0), (2, 'above', 0.3), (1, 5, -1)], weight=plane(4), mask=mask, every=7, capacity=13)
    calls(L, ('stats_begin', 3, [{'var': 0, 'kind': 0, 'level': 0.0}, {'var': 2, 'kind': 4, 'level': f32(0.3)},
                                 {'var': 1, 'kind': 5, 'level': -1.0}], plane(4, np.float32), mask.astype(np.uint8), 7, 13))
    back(st.stats_read(1, 2), 20, np.float64, (2, 3))
    calls(L, ('stats_read', 1, 2, 'out float64 (2, 3)'))
    back(st.stats_read(), 20, np.float64, (SAMPLES, 3))
    calls(L, ('stats_count', 'ref'), ('stats_read', 0, SAMPLES, 'out float64 (3, 3)'))
    st.stats_begin([(1, 'min', 0.0)])
    calls(L, ('stats_begin', 1, [{'var': 1, 'kind': 1, 'level': 0.0}], None, None, 1, 1))
    refused('stats_begin: a weight plane of shape (8, 6) on a 6 x 8 grid', st.stats_begin, [(0, 'sum', 0.0)], weight=plane().T)
    refused('stats_begin: a mask of shape (8, 6) on a 6 x 8 grid', st.stats_begin, [(0, 'sum', 0.0)], mask=mask.T)
    calls(L)


def test_leads():
    st, L = make()
    tables = np.stack([plane(5), plane(6)])
    st.leads_begin([(1, 2, 0), (3, 4, 1)], tables, weight=plane(7), var=2, every=3, capacity=8)
    calls(L, ('leads_begin', 2, 2, np.array([(1, 2, 0), (3, 4, 1)], np.int32), 2, tables.astype(np.float32), plane(7, np.float32), 3, 8))
    st.leads_begin([(0, 0, 0)], tables[:1])
    calls(L, ('leads_begin', 0, 1, np.array([(0, 0, 0)], np.int32), 1, tables[:1].astype(np.float32), None, 1, 1))
    L.tail['leads'] = (1,)
    back(st.leads_read(1, 2), 21, np.float64, (2, 1))
    calls(L, ('leads_read', 1, 2, 'out float64 (2, 1)'))
    back(st.leads_read(2), 21, np.float64, (SAMPLES - 2, 1))
    calls(L, ('leads_count', 'ref'), ('leads_read', 2, SAMPLES - 2, 'out float64 (1, 1)'))
    refused('leads_begin: tables of shape (2, 8, 6) on a 6 x 8 grid', st.leads_begin, [(0, 0, 0)], tables.transpose(0, 2, 1))
    refused('leads_begin: tables of shape (6, 8) on a 6 x 8 grid', st.leads_begin, [(0, 0, 0)], tables[0])
    refused('leads_begin: a weight plane of shape (8, 6) on a 6 x 8 grid', st.leads_begin, [(0, 0, 0)], tables, weight=plane().T)
    calls(L)


def test_waves_and_links():
    st, L = make()
    mask = np.arange(H * W).reshape(H, W) % 3
    st.waves_begin(1, 1, 0.3, 2, 0, np.float32(0.7), conn=8, mask=mask, max_waves=7, every=5, capacity=6)
    calls(L, ('waves_begin', 1, 1, 0.3, 2, 0, f32(0.7), 8, mask.astype(np.uint8), 7, 5, 6))
    L.tail['links'] = (0,)
    counts, recs = st.waves_links_read(0, 2)                                 # links are off: no room for a record
    back(recs, 25, _lib.WAVE_LINK_DTYPE, (2, 0))
    calls(L, ('waves_links_read', 0, 2, 'out int32 (2, 4)', 'out struct (2, 0)'))
    L.tail['links'] = (9,)
    st.waves_links_begin(np.int64(9))
    calls(L, ('waves_links_begin', 9))
    counts, recs = st.waves_read(1, 2)
    back(counts, 22, np.int32, (2, 3))
    back(recs, 23, _lib.WAVE_RECORD_DTYPE, (2, 7))
    calls(L, ('waves_read', 1, 2, 'out int32 (2, 3)', 'out struct (2, 7)'))
    counts, recs = st.waves_read(records=False)
    back(counts, 22, np.int32, (SAMPLES, 3))
    assert recs is None
    calls(L, ('waves_count', 'ref'), ('waves_read', 0, SAMPLES, 'out int32 (3, 3)', None))
    counts, recs = st.waves_links_read(1)
    back(counts, 24, np.int32, (SAMPLES - 1, 4))
    back(recs, 25, _lib.WAVE_LINK_DTYPE, (SAMPLES - 1, 9))
    calls(L, ('waves_count', 'ref'), ('waves_links_read', 1, SAMPLES - 1, 'out int32 (2, 4)', 'out struct (2, 9)'))
    counts, recs = st.waves_links_read(0, 1, records=False)
    assert recs is None
    calls(L, ('waves_links_read', 0, 1, 'out int32 (1, 4)', None))
    back(st.waves_labels(), 26, np.int32, (H, W))
    calls(L, ('waves_labels', 'out int32 (6, 8)'))
    st.waves_end()
    assert st._wave_link_max == 0 and st._wave_max == 7                       # (the end of a recorder turns its links off)
    st.waves_links_begin()
    st.waves_begin()                                                          # (and so does attaching the next one)
    assert st._wave_link_max == 0 and st._wave_max == 256
    calls(L, ('waves_end',), ('waves_links_begin', 512), ('waves_begin', 0, 0, 0.0, -1, 0, 0.0, 4, None, 256, 1, 1))
    refused('waves_begin: a mask of shape (8, 6) on a 6 x 8 grid', st.waves_begin, mask=mask.T)
    calls(L)


STIM_ZERO = {f: 0.0 if f in ('v', 'floor') else 0 for f, _ in _lib.StimEntry._fields_}
RULE_ZERO = {f: 0.0 if f in ('v', 'floor') else 0 for f, _ in _lib.TrigRule._fields_}
SENSOR_ZERO = {f: 0.0 if f == 'level' else 0 for f, _ in _lib.TrigSensor._fields_}


def test_stimulus_program():
    st, L = make()
    e0 = {'var': 1, 'mode': 'add', 'shape': 'plane', 'plane': 1, 'first': 3, 'period': 10, 'count': 4, 'hold': 2}
    e1 = {'mode': 0, 'shape': 'rect', 'r0': 1, 'r1': 3, 'c0': 2, 'c1': np.int64(6), 'v': 0.3, 'floor': -np.inf}
    st.stim_begin([e0, e1, {}], planes=[plane(8), plane(9, np.float32)])
    calls(L, ('stim_begin', 3, [dict(STIM_ZERO, var=1, mode=1, shape=1, plane=1, first=3, period=10, count=4, hold=2),
                                dict(STIM_ZERO, r0=1, r1=3, c0=2, c1=6, v=f32(0.3), floor=-np.inf, count=1, hold=1),
                                dict(STIM_ZERO, count=1, hold=1)], 2, np.stack([plane(8, np.float32), plane(9, np.float32)])))
    assert e0['mode'] == 'add' and 'shape' in e1                              # (the caller's dicts are left as they were)
    for planes in (None, []):
        st.stim_begin([], planes)
        calls(L, ('stim_begin', 0, [], 0, None))
    refused("stim_begin: entry 1: unknown field 'sensor'", st.stim_begin, [{}, {'sensor': 1}])
    refused('stim_begin: a plane of shape (8, 6) on a 6 x 8 grid', st.stim_begin, [{}], planes=[plane(), plane().T])
    calls(L)


def test_lesion_program():
    st, L = make()
    p0, p1 = np.arange(6.0).reshape(2, 3) / 8, np.arange(4.0).reshape(4, 1) / 4
    st.lesion_begin([(5, (1, 3, 2, 5), p0), (np.int64(2), (0, 4, 7, 8), p1)])
    calls(L, ('lesion_begin', 2, [{'offset': 0, 'tick': 5, 'r0': 1, 'r1': 3, 'c0': 2, 'c1': 5, 'reserved': 0},
                                  {'offset': 6, 'tick': 2, 'r0': 0, 'r1': 4, 'c0': 7, 'c1': 8, 'reserved': 0}], 10,
              np.concatenate([p0.ravel(), p1.ravel()]).astype(np.float32)))
    st.lesion_begin([])
    calls(L, ('lesion_begin', 0, [], 0, np.zeros(1, np.float32)))
    st.lesion_apply((1, 3, 2, 5), p0)
    calls(L, ('lesion_apply', np.array((1, 3, 2, 5), np.int32), p0.astype(np.float32)))
    back(st.get_phase(), 27, np.float32, (H, W))
    calls(L, ('get_phase', 'out float32 (6, 8)'))
    refused('lesion_begin: entry 1: a patch of shape (3, 2) on the box rows [1, 3) x columns [2, 5)', st.lesion_begin,
            [(0, (0, 4, 7, 8), p1), (0, (1, 3, 2, 5), p0.T)])
    refused('lesion_apply: a patch of shape (3, 2) on the box (1, 3, 2, 5)', st.lesion_apply, (1, 3, 2, 5), p0.T)
    refused('lesion_apply: a patch of shape (2, 3) on the box (1, 3, 2)', st.lesion_apply, (1, 3, 2), p0)
    calls(L)


def test_trigger_program():
    st, L = make()
    m0, m1 = np.arange(H * W).reshape(H, W) % 3, np.arange(H * W).reshape(H, W) % 2 == 0
    sensors = [{'site': 'mask', 'mask': m0, 'var': 1, 'level': 0.3, 'need': 4},
               {'site': 'rect', 'r0': 1, 'r1': 3, 'c0': 2, 'c1': 6}, {'site': 1, 'mask': m1, 'level': -1}]
    r0 = {'sensor': 2, 'edge': 'fall', 'arm': 1, 'blank': 9, 'escape': 30, 'max_det': 2, 'delay': 3, 'count': 2, 'period': 4, 'hold': 2,
          'var': 1, 'mode': 'add', 'shape': 'plane', 'plane': 1}
    r1 = {'edge': 0, 'mode': 'max', 'shape': 0, 'r0': 1, 'r1': 3, 'c0': 2, 'c1': 6, 'v': 0.3, 'floor': -np.inf}
    st.trig_begin(sensors, [r0, r1], planes=[plane(8), plane(9)], every=5, capacity=17)
    calls(L, ('trig_begin', 3, [dict(SENSOR_ZERO, site=1, var=1, level=f32(0.3), need=4), dict(SENSOR_ZERO, r0=1, r1=3, c0=2, c1=6, need=1),
                                dict(SENSOR_ZERO, site=1, level=-1.0, need=1)], np.stack([m0 != 0, m1]).astype(np.uint8), 2,
              [dict(RULE_ZERO, sensor=2, edge=1, arm=1, blank=9, escape=30, max_det=2, delay=3, count=2, period=4, hold=2, var=1, mode=1,
                    shape=1, plane=1), dict(RULE_ZERO, r0=1, r1=3, c0=2, c1=6, v=f32(0.3), floor=-np.inf, count=1, hold=1)],
              2, np.stack([plane(8, np.float32), plane(9, np.float32)]), 5, 17))
    assert sensors[0]['site'] == 'mask' and r0['edge'] == 'fall'
    back(st.trig_read(1, 2), 28, np.int32, (2, 2, 6))
    calls(L, ('trig_read', 1, 2, 'out int32 (2, 2, 6)'))
    back(st.trig_read(), 28, np.int32, (SAMPLES, 2, 6))
    calls(L, ('trig_count', 'ref'), ('trig_read', 0, SAMPLES, 'out int32 (3, 2, 6)'))
    st.trig_begin([{}], [{}])
    calls(L, ('trig_begin', 1, [dict(SENSOR_ZERO, need=1)], None, 1, [dict(RULE_ZERO, count=1, hold=1)], 0, None, 1, 4096))
    refused('trig_begin: sensor 1: a mask of shape (8, 6) on a 6 x 8 grid', st.trig_begin, [{}, {'site': 'mask', 'mask': m0.T}], [{}])
    refused('trig_begin: sensor 0: a mask of shape () on a 6 x 8 grid', st.trig_begin, [{'site': 'mask'}], [{}])
    refused("trig_begin: sensor 0: unknown field 'plane'", st.trig_begin, [{'plane': 1}], [{}])
    refused("trig_begin: rule 1: unknown field 'first'", st.trig_begin, [{}], [{}, {'first': 1}])
    refused('trig_begin: a plane of shape (8, 6) on a 6 x 8 grid', st.trig_begin, [{}], [{}], planes=[plane().T])
    calls(L)
