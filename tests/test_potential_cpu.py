"""not-gpu: the potential-map recorder's host side — the NumPy restatement (tests/potential_ref.py) against math.fsum and against
the lead recorder's restatement, the condition the bit tests rest on (another order of summation changes bits on these planes),
the restated summary on hand-made cubes, PotentialMapRecorder (fib_tf_amd/potential.py) over a stub stepper, its argument
checks, and what the bindings hand to the C functions.  Nothing here needs a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lead_ref  # noqa: E402
import potential_ref as ref  # noqa: E402
from test_leads_cpu import front, hole  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {'fibhip_pmap_begin': 10, 'fibhip_pmap_count': 2, 'fibhip_pmap_read': 4, 'fibhip_pmap_summary': 9, 'fibhip_pmap_end': 1}
SEED = 5                        # of the test planes: test_another_order_changes_bits holds for it


def plane_for(H, W, with_phase, seed=SEED):
    """(X, phase, q): a front on the grid, the phase field with a hole or none, the source plane with the phase field as weight"""
    X = front(H, W, seed + H * W)
    phase = hole(H, W) if with_phase else None
    return X, phase, ref.source_plane(X, phase, phase)


def table_for(R, seed=0):
    from fib_tf_amd import potential
    return potential.truncated_table(R, 1.5 + 0.25 * seed, 0.7)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_phase', [False, True], ids=['nophase', 'hole'])
@pytest.mark.parametrize('shape', [(5, 3), (4, 64), (37, 53)], ids=lambda s: '%dx%d' % s)
def test_restatement_against_fsum(shape, with_phase):
    """every site of the full lattice within n u / (1 - n u) * sum |terms| of the correctly rounded exact sum"""
    H, W = shape
    X, phase, q = plane_for(H, W, with_phase)
    assert q.dtype == np.float32 and np.array_equal(q[1:-1, 1:-1], lead_ref.weighted(X, phase, phase))
    assert not np.any(q[0]) and not np.any(q[-1]) and not np.any(q[:, 0]) and not np.any(q[:, -1]) and np.any(q != 0)
    for R in (1, 3, 6):
        T = table_for(R)
        phi = ref.maps(q, T)
        assert phi.shape == (H, W) and phi.dtype == np.float64 and np.any(phi != 0)
        worst = 0.0
        for r in range(H):
            for c in range(W):
                t = ref.terms(q, T, r, c)
                assert t.shape == ((2 * R + 1) ** 2,)
                b = ref.bound(t, R)
                err = abs(phi[r, c] - ref.exact(q, T, r, c))
                assert err <= b, (shape, R, r, c, phi[r, c], err, b)
                worst = max(worst, err / b if b > 0 else 0.0)
        print('%dx%d phase %s R %d: largest |sum - exact| / bound %.3g' % (H, W, with_phase, R, worst))


def test_restatement_against_the_lead_restatement():
    """R = 32 on a 33 x 30 grid: the window of every site covers every cell, so a site's non-zero terms are the lead recorder's
    terms for a lead at the same cell with the same table, as a multiset; the two sums differ by their orders only"""
    from fib_tf_amd import potential
    H, W, R = 33, 30, 32
    X, phase, q = plane_for(H, W, True)
    T = potential.truncated_table(R, 2.0)
    phi = ref.maps(q, T)
    for r, c in ((0, 0), (16, 15), (32, 29), (5, 22), (32, 0)):
        mine = ref.terms(q, T, r, c)
        lead = lead_ref.terms(X, phase, phase, [(r, c, 0)], T[:, :W])[0]
        assert len(lead) == (H - 2) * (W - 2) and np.count_nonzero(lead) > len(lead) // 2
        assert sorted(mine[mine != 0].tolist()) == sorted(lead[lead != 0].tolist())
        want = lead_ref.traces(X, phase, phase, [(r, c, 0)], T[:, :W])[0]
        b = ref.bound(mine, R)
        assert b >= lead_ref.bound(lead) and abs(phi[r, c] - want) <= 2 * b, (r, c, phi[r, c], want, b)


@pytest.mark.parametrize('shape,R', [((5, 3), 1), ((4, 64), 2), ((37, 53), 1), ((37, 53), 5), ((70, 130), 3), ((33, 30), 32)],
                         ids=lambda v: str(v).replace(' ', ''))
def test_another_order_changes_bits(shape, R):
    """columns before rows is another order of the same terms: on the planes the device tests use it changes at least one bit
    of at least one site, so a device that summed in another order could not pass them.  A condition on the inputs (SEED).
    (5 x 3 has ONE interior column: every row sum has one term that is not zero and both orders add the same three numbers in
    the same order — no seed can make that plane see the order, and the test says so)"""
    H, W = shape
    _, _, q = plane_for(H, W, True)
    T = table_for(R)
    a, b = ref.maps(q, T), ref.maps(q, T, order='cols')
    if shape == (5, 3):
        assert a.tobytes() == b.tobytes() and np.any(a != 0)
        return
    assert a.tobytes() != b.tobytes()
    assert np.allclose(a, b, rtol=1e-9, atol=1e-12)


def test_sub_lattice_and_sites():
    H, W = 37, 53
    _, _, q = plane_for(H, W, True)
    T = table_for(4)
    full = ref.maps(q, T)
    rows, cols = ref.lattice(H, W, (3, 30, 5, 50), (7, 9))
    assert rows.tolist() == [3, 10, 17, 24] and cols.tolist() == [5, 14, 23, 32, 41]
    sub = ref.maps(q, T, (3, 30, 5, 50), (7, 9))
    assert sub.shape == (4, 5) and sub.tobytes() == np.ascontiguousarray(full[np.ix_(rows, cols)]).tobytes()


# ---- the summary -------------------------------------------------------------------------------------------------------------
def test_summary_on_hand_made_cubes():
    nan = float('nan')
    cube = np.array([[1.0, 3.0, nan, 2.0, 5.0],
                     [0.0, 3.0, 1.0, nan, 5.0],
                     [0.0, 1.0, 0.0, 1.0, 5.0],
                     [2.0, 3.0, 4.0, 0.0, 5.0],
                     [1.0, 1.0, 9.0, 0.0, 5.0]]).reshape(5, 1, 5)
    vmin, vmax, dmin, kmin, kmax, kd = ref.summary(cube)
    assert all(a.shape == (1, 5) for a in (vmin, vmax, dmin, kmin, kmax, kd))
    assert vmin.dtype == vmax.dtype == dmin.dtype == np.float64 and kmin.dtype == kmax.dtype == kd.dtype == np.int32
    # site 0: the minimum 0.0 twice (first wins: 1), the steepest fall -1.0 twice (1 -> 0 at s = 1, 2 -> 1 at s = 4: first wins)
    assert (vmin[0, 0], kmin[0, 0], vmax[0, 0], kmax[0, 0], dmin[0, 0], kd[0, 0]) == (0.0, 1, 2.0, 3, -1.0, 1)
    # site 1: the maximum 3.0 three times (first wins: 0), the minimum 1.0 twice (2), falls of -2.0 at s = 2 and s = 4 (2)
    assert (vmin[0, 1], kmin[0, 1], vmax[0, 1], kmax[0, 1], dmin[0, 1], kd[0, 1]) == (1.0, 2, 3.0, 0, -2.0, 2)
    # site 2: a NaN first stays in vmin and vmax, and in dmin, whose first element it makes NaN
    assert np.isnan(vmin[0, 2]) and np.isnan(vmax[0, 2]) and np.isnan(dmin[0, 2]) and (kmin[0, 2], kmax[0, 2], kd[0, 2]) == (0, 0, 1)
    # site 3: a NaN later replaces nothing: min 0.0 first at 3, max 2.0 at 0; d = NaN, NaN, -1, 0: dmin starts as NaN and stays
    assert (vmin[0, 3], kmin[0, 3], vmax[0, 3], kmax[0, 3]) == (0.0, 3, 2.0, 0) and np.isnan(dmin[0, 3]) and kd[0, 3] == 1
    # site 4: constant: everything is the first element, d = +0.0
    assert (vmin[0, 4], kmin[0, 4], vmax[0, 4], kmax[0, 4], dmin[0, 4], kd[0, 4]) == (5.0, 0, 5.0, 0, 0.0, 1)
    # a window: indices count from the recorder's first sample
    vmin, vmax, dmin, kmin, kmax, kd = ref.summary(cube, 2, 3)
    assert (vmin[0, 0], kmin[0, 0], vmax[0, 0], kmax[0, 0], dmin[0, 0], kd[0, 0]) == (0.0, 2, 2.0, 3, -1.0, 4)
    assert (vmin[0, 3], kmin[0, 3], dmin[0, 3], kd[0, 3]) == (0.0, 3, -1.0, 3)
    with pytest.raises(AssertionError):
        ref.summary(cube, 4, 1)


# ---- the Python class on a stub stepper ----------------------------------------------------------------------------------------
H, W = 6, 8


class StubStepper:
    """records (name, args, kwargs) of every call"""

    def __init__(self, canned=None):
        self.log, self.canned = [], canned or {}

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)

        def call(*a, **kw):
            self.log.append((name, a, kw))
            return self.canned.get(name)
        return call

    def called(self, name):
        return sum(1 for c in self.log if c[0] == name)


class Model:
    VAR_NAMES = ('V', 'g')
    height, width = H, W
    duration, dt, dt_per_step, diff = 100, 0.1, 10, 2.0
    phase = None

    def __init__(self, stepper):
        self._stepper = stepper


def attach(table=None, canned=None, **kw):
    from fib_tf_amd import potential
    st = StubStepper(canned)
    return potential.PotentialMapRecorder(Model(st), potential.truncated_table(2, 1.0) if table is None else table, **kw), st


def test_refusals_come_first():
    from fib_tf_amd import potential
    from fib_tf_amd.sharded import ShardedStepper
    with pytest.raises(AssertionError) as e:
        potential.PotentialMapRecorder(Model(None), None)
    assert str(e.value) == 'record_potential_map should be called after calling define'
    sharded = ShardedStepper.__new__(ShardedStepper)
    sharded.world = 2
    with pytest.raises(NotImplementedError) as e:
        potential.PotentialMapRecorder(Model(sharded), None)
    assert str(e.value) == 'record_potential_map: potential maps are recorded on a single device only; this model runs as row blocks over 2 ranks'
    m = Model(object())
    m._compiled = {'source': 'struct Custom {\n    static constexpr bool ZEROPAD = true;\n'}
    with pytest.raises(ValueError, match='zero-padded Laplacian'):
        potential.PotentialMapRecorder(m, potential.truncated_table(2, 1.0))


def test_every_capacity_and_what_begin_is_handed():
    with pytest.raises(ValueError) as e:
        attach(every=0)
    assert str(e.value) == 'record_potential_map: every must be >= 1'
    rec, st = attach(every=3)                                  # duration 100 ms in ticks of 1 ms, a sample every 3 ticks
    assert rec.capacity == 33 and type(rec.capacity) is int and rec.every == 3
    name, a, kw = st.log[0]
    assert name == 'pmap_begin' and not kw and a[-1] == 33 and a[-2] == 3 and a[-3] == 0
    assert a[0].shape == (3, 3) and a[0].dtype == np.float32 and a[1] is None and a[2] == (0, H, 0, W) and a[3] == (1, 1)
    assert attach(every=300)[0].capacity == 1                  # at least one
    rec, st = attach(every=3, max_samples=np.int64(5))
    assert rec.capacity == 5 and type(rec.capacity) is int
    assert attach()[0].every == 10 and attach()[0].capacity == 10          # the default stride
    with pytest.raises(ValueError, match='max_samples must be >= 1'):
        attach(max_samples=0)
    rec, st = attach(var='g', window=(1, 6, 2, 7), step=(2, 3))
    assert rec.var == 1 and rec.shape == (3, 2) and st.log[0][1][2:5] == ((1, 6, 2, 7), (2, 3), 1)
    rows, cols = rec.sites()
    assert rows.tolist() == [1, 3, 5] and cols.tolist() == [2, 5]
    m = Model(StubStepper())
    m.phase = np.full((H, W), 0.5, np.float32)
    from fib_tf_amd import potential
    rec = potential.PotentialMapRecorder(m, potential.truncated_table(1, 1.0))
    assert np.array_equal(rec.weight, m.phase) and rec.scale == 2.0 and m._stepper.log[0][1][1] is rec.weight
    assert potential.PotentialMapRecorder(m, potential.truncated_table(1, 1.0), weight=None).weight is None


def test_close_twice_readers_after_close_and_sample_times():
    rec, st = attach()
    assert rec.open and st.called('pmap_end') == 0
    rec.close()
    rec.close()
    assert not rec.open and st.called('pmap_end') == 1
    n = len(st.log)
    for name, a in (('count', ()), ('raw', ()), ('maps', ()), ('summary', ()), ('voltage', ()), ('lat_ms', ()), ('bipolar', (0,)), ('times_ms', ())):
        with pytest.raises(AssertionError) as e:
            getattr(rec, name)(*a)
        assert str(e.value) == 'the potential-map recorder has been closed', name
    assert len(st.log) == n                                    # nothing reached the stepper
    rec, st = attach()
    with rec as inside:
        assert inside is rec
    assert not rec.open and st.called('pmap_end') == 1
    rec, st = attach(every=3)
    n = len(st.log)
    got = rec.times_ms(2, 3)
    assert rec.tick_ms == 1.0 and len(st.log) == n and got.dtype == np.float64 and got.tolist() == [9.0, 12.0, 15.0]
    assert rec.times_ms(2, -1).shape == (0,)


def test_derived_maps():
    """voltage, lat_ms, maps and bipolar from what the stepper hands back"""
    f = np.arange(6, dtype=np.float64).reshape(2, 3)
    k = np.arange(6, dtype=np.int32).reshape(2, 3)
    cube = np.arange(24, dtype=np.float64).reshape(4, 2, 3) ** 2
    rec, st = attach(every=3, window=(0, 2, 0, 3), canned={'pmap_summary': (f, f + 2.5, -f, k, k + 1, k + 2), 'pmap_read': cube})
    s = rec.summary(1, 3)
    assert st.log[-1] == ('pmap_summary', (1, 3), {}) and sorted(s) == ['dmin', 'kd', 'kmax', 'kmin', 'vmax', 'vmin']
    assert np.array_equal(rec.voltage(), np.full((2, 3), 2.5 * 2.0)) and np.array_equal(rec.voltage(scale=-1.0), np.full((2, 3), 2.5))
    assert np.array_equal(rec.lat_ms(), (k + 2 + 0.5) * 3 * 1.0)              # the midpoint of samples kd - 1 and kd
    assert np.array_equal(rec.maps(), cube * 2.0) and np.array_equal(rec.raw(1, 2), cube) and st.log[-1] == ('pmap_read', (1, 2), {})
    assert np.array_equal(rec.bipolar(0), 2.0 * (cube[:, 1:] - cube[:, :-1])) and rec.bipolar(0).shape == (4, 1, 3)
    assert np.array_equal(rec.bipolar(1, scale=1.0), cube[:, :, 1:] - cube[:, :, :-1]) and rec.bipolar(1).shape == (4, 2, 2)
    with pytest.raises(ValueError, match='axis is 0'):
        rec.bipolar(2)


def test_argument_checks():
    from fib_tf_amd import leads, potential
    T = potential.truncated_table(4, 2.0, 0.5)
    assert T.shape == (5, 5) and T.dtype == np.float32 and np.array_equal(T, leads.point_table(5, 5, 2.0, 0.5))
    assert potential.parse_table(T, None)[1] == 4 and potential.parse_table(T, 4)[1] == 4
    with pytest.raises(ValueError, match=r'a table of shape \(5, 5\) for radius 3: it must be \[4, 4\]'):
        attach(T, radius=3)
    with pytest.raises(ValueError, match=r'the table is \[R \+ 1, R \+ 1\] \(got an array of shape \(5, 4\)\)'):
        attach(T[:, :4])
    with pytest.raises(ValueError, match=r'the table is \[R \+ 1, R \+ 1\]'):
        attach(T[0])
    with pytest.raises(ValueError, match=r'radius must be 1 \.\. 32 \(got 0\)'):
        attach(np.ones((1, 1), np.float32))
    with pytest.raises(ValueError, match=r'radius must be 1 \.\. 32 \(got 33\)'):
        attach(np.ones((34, 34), np.float32))
    assert attach(np.ones((33, 33), np.float32))[0].radius == 32
    for bad in (np.nan, np.inf, -np.inf):
        t = T.copy()
        t[2, 3] = bad
        with pytest.raises(ValueError, match='the table has a value that is not finite'):
            attach(t)
    for step in ((0, 1), (1, 0), (17, 1), (1, 17), (-1, 1)):
        with pytest.raises(ValueError, match=r'a step is 1 \.\. 16 cells each way'):
            attach(step=step)
    with pytest.raises(ValueError, match=r'a step is \(sy, sx\)'):
        attach(step=3)
    assert attach(step=(16, 16))[0].shape == (1, 1)
    for win in ((2, 2, 0, W), (0, H, 5, 5), (3, 2, 0, W), (-1, H, 0, W), (0, H + 1, 0, W), (0, H, 0, W + 1)):
        with pytest.raises(ValueError, match='is empty or outside the 6 x 8 grid'):
            attach(window=win)
    w = np.ones((H, W), np.float32)
    w[1, 2] = np.nan
    with pytest.raises(ValueError, match='the weight plane has a value that is not finite'):
        attach(weight=w)
    with pytest.raises(ValueError, match=r'a weight plane of shape \(8, 6\)'):
        attach(weight=np.ones((W, H), np.float32))
    with pytest.raises(ValueError, match="weight is 'phase', None or"):
        attach(weight='phi')
    with pytest.raises(ValueError, match='unknown array'):
        attach(var='w')


# ---- the C ABI and the bindings ----------------------------------------------------------------------------------------------
def test_declarations_and_arity():
    from fib_tf_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    for name, nargs in ENTRY_POINTS.items():
        assert 'int %s(' % name in src
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is C.c_int and len(_lib.SYMBOLS[name][0]) == nargs, name
    assert _lib.SYMBOLS['fibhip_pmap_begin'][0][9] is C.c_longlong
    assert '#define FIBHIP_PMAP_MAX_RADIUS %d' % _lib.PMAP_MAX_RADIUS in src and _lib.PMAP_MAX_RADIUS == 32
    assert '#define FIBHIP_PMAP_MAX_STEP %d' % _lib.PMAP_MAX_STEP in src and _lib.PMAP_MAX_STEP == 16


def test_library_exports_the_entry_points():
    from fib_tf_amd import _lib
    L = C.CDLL(_lib.SO)
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None, name


FP, IP, DP = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)
HANDLE = 0x5eed


def arr(p, ctype, dtype, shape):
    assert isinstance(p, ctype), (type(p), ctype)
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_ubyte)), shape=(n,)).view(dtype).reshape(shape)


class FakeLibrary:
    """stands where the loaded library stands: decodes and logs the arguments, fills the out-arrays"""

    def __init__(self):
        self.log = []

    def fibhip_pmap_begin(self, h, var, R, table, weight, window, sy, sx, every, capacity):
        assert h.value == HANDLE
        self.log.append(('begin', var, R, arr(table, FP, np.float32, (R + 1, R + 1)).copy(),
                         None if weight is None else arr(weight, FP, np.float32, (H, W)).copy(), arr(window, IP, np.intc, (4,)).tolist(), sy, sx,
                         every, capacity))
        return 0

    def fibhip_pmap_count(self, h, ref):
        assert isinstance(ref._obj, C.c_longlong)
        ref._obj.value = 3
        self.log.append(('count',))
        return 0

    def fibhip_pmap_read(self, h, first, count, out):
        arr(out, DP, np.float64, (max(count, 0), 2, 3))[...] = 7.0
        self.log.append(('read', first, count))
        return 0

    def fibhip_pmap_summary(self, h, first, count, *out):
        assert len(out) == 6
        for i, p in enumerate(out):
            arr(p, DP if i < 3 else IP, np.float64 if i < 3 else np.int32, (2, 3))[...] = i + 1
        self.log.append(('summary', first, count))
        return 0

    def fibhip_pmap_end(self, h):
        self.log.append(('end',))
        return 0

    def fibhip_destroy(self, h):                               # (Stepper.close, when the stand-in's stepper is collected)
        return 0


def test_bindings():
    from fib_tf_amd import _lib
    L = FakeLibrary()
    st = _lib.Stepper.__new__(_lib.Stepper)
    st._h, st._L, st.height, st.width, st.nvar, st._warned = C.c_void_p(HANDLE), L, H, W, 4, True
    T = np.arange(9, dtype=np.float64).reshape(3, 3)
    wgt = np.arange(H * W, dtype=np.float64).reshape(H, W)
    st.pmap_begin(T, wgt, (1, 6, 2, 8), (2, 3), 1, 5, 9)
    got = L.log.pop()
    assert got[:3] == ('begin', 1, 2) and np.array_equal(got[3], T.astype(np.float32)) and np.array_equal(got[4], wgt.astype(np.float32))
    assert got[5:] == ([1, 6, 2, 8], 2, 3, 5, 9)
    st.pmap_begin(T)                                           # the defaults: the whole grid, step 1, no plane
    got = L.log.pop()
    assert got[4] is None and got[5:] == ([0, H, 0, W], 1, 1, 1, 1)
    with pytest.raises(ValueError, match=r'a table of shape \(3, 2\) is not \[R \+ 1, R \+ 1\]'):
        st.pmap_begin(T[:, :2])
    with pytest.raises(ValueError, match=r'a weight plane of shape \(8, 6\)'):
        st.pmap_begin(T, wgt.T)
    st.pmap_begin(T, None, (1, 6, 2, 8), (3, 2))                # 5 rows by 3: two site rows; 6 columns by 2: three
    L.log.clear()
    assert st.pmap_count() == 3 and L.log == [('count',)]
    out = st.pmap_read(1, 2)
    assert out.shape == (2, 2, 3) and out.dtype == np.float64 and np.all(out == 7.0) and L.log[-1] == ('read', 1, 2)
    out = st.pmap_read()                                       # count=None: all taken so far
    assert out.shape == (3, 2, 3) and L.log[-2:] == [('count',), ('read', 0, 3)]
    s = st.pmap_summary(1)
    assert L.log[-2:] == [('count',), ('summary', 1, 2)] and len(s) == 6
    assert [a.dtype for a in s] == [np.float64] * 3 + [np.int32] * 3 and [float(a[0, 0]) for a in s] == [1, 2, 3, 4, 5, 6]
    assert all(a.shape == (2, 3) for a in s)
    st.pmap_end()
    assert L.log[-1] == ('end',)
