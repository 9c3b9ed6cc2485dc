"""not-gpu: the lead recorder's host side — the NumPy restatement (tests/lead_ref.py) against the reference-generated Laplacian
and phase-term vectors, the properties the definition implies (the clamped stencil conserves, a trace is linear in its table,
mirrored electrodes over a symmetric state agree), `point_table`, LeadRecorder's argument checks (fib_tf_amd/leads.py) and the C
ABI, none of which needs a device."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lead_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('fibhip_leads_begin', 'fibhip_leads_count', 'fibhip_leads_read', 'fibhip_leads_end')


def front(H, W, seed=0):
    """a state with a wavefront on the grid: a plateau behind a smooth front that runs obliquely, plus a little noise"""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:H, 0:W]
    x = 1.0 / (1.0 + np.exp((c + 0.4 * r - 0.55 * (W + 0.4 * H)) / 1.5))
    return (x + rng.normal(scale=1e-3, size=(H, W))).astype(np.float32)


def hole(H, W):
    r, c = np.mgrid[0:H, 0:W]
    d = np.hypot(r - 0.4 * H, c - 0.6 * W)
    return np.maximum(0.5 * (np.tanh(d - 0.2 * min(H, W)) + 1.0), 1e-5).astype(np.float32)


def test_declarations_and_binding():
    from fib_tf_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    for name in ENTRY_POINTS:
        assert 'int %s(' % name in src
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is _lib.C.c_int
    assert len(_lib.SYMBOLS['fibhip_leads_begin'][0]) == 9
    assert '#define FIBHIP_MAX_LEADS %d' % _lib.MAX_LEADS in src and _lib.MAX_LEADS == 64
    assert '#define FIBHIP_MAX_LEAD_TABLES %d' % _lib.MAX_LEAD_TABLES in src and _lib.MAX_LEAD_TABLES == 4
    assert '#define FIBHIP_ABI_VERSION 1' in src


def test_library_exports_the_entry_points():
    """the built library (dlopen needs no device) exports the four entry points by name"""
    from fib_tf_amd import _lib
    L = _lib.C.CDLL(_lib.SO)
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None, name


def test_source_equals_the_reference_vectors(golden):
    """where every tap lies inside [1, H - 2] x [1, W - 2] the boundary clamp reads what the reference's REFLECT pad reads: there
    the source is the reference's laplace(), bit for bit, with and without a phase field, and so is the phase term"""
    u = golden('unit_ops')
    X, phi = u['X'], u['phi']
    inner = (slice(1, -1), slice(1, -1))                      # of the interior plane: the cells 2 .. H - 3, 2 .. W - 3
    whole = (slice(2, -2), slice(2, -2))
    assert np.array_equal(ref.stencil(X)[inner], u['laplace_nophase'][whole])
    assert np.array_equal(ref.source(X)[inner], u['laplace_nophase'][whole])
    assert np.array_equal(ref.phase_term(X, phi)[inner], u['phase_field'][whole])
    assert np.array_equal(ref.source(X, phi)[inner], u['laplace_phase'][whole])
    # ... and on the whole interior it is the reference's laplace() of the boundary-enforced array
    assert np.array_equal(ref.clamped(X), u['enforce_boundary'])
    assert ref.source(X, phi).shape == (X.shape[0] - 2, X.shape[1] - 2) and ref.source(X, phi).dtype == np.float32


@pytest.mark.parametrize('shape', [(3, 3), (5, 3), (4, 64), (37, 53), (64, 64)], ids=lambda s: '%dx%d' % s)
def test_clamped_stencil_conserves(shape):
    """no phase field, a table of ones: the stencil's weights sum to zero and the clamp hands every flux that leaves the interior
    back, so the exact sum of the sources is zero.  On a state of few bits (multiples of 2^-10 in [0, 1]) the float32 stencil is
    exact, the terms are the exact sources and the trace is 0 within the summation bound; on a general state what is left is the
    rounding of the stencil's ten float32 operations"""
    H, W = shape
    ones = np.ones((H, W), np.float32)
    pos = [(H // 2, W // 2, 0)]
    X = (np.round(front(H, W, 3) * 1024) / 1024).astype(np.float32)
    t = ref.terms(X, None, None, pos, ones)[0]
    assert t.shape == ((H - 2) * (W - 2),)
    assert H * W < 16 or np.any(t != 0)
    assert abs(ref.traces(X, None, None, pos, ones)[0]) <= ref.bound(t)
    X = front(H, W, 3)
    t = ref.terms(X, None, None, pos, ones)[0]
    slack = len(t) * 10 * 2.0 ** -24 * 12.0 * float(np.abs(X).max())
    assert abs(ref.traces(X, None, None, pos, ones)[0]) <= slack + ref.bound(t)


def test_linearity_in_the_table():
    """tables of few bits (multiples of 2^-8): their float32 sum is exact, and so is the float64 sum of two terms — the terms of
    A + B are the terms of A plus the terms of B, bit for bit; a scaling by a power of two scales the trace"""
    H, W = 37, 53
    X, phi = front(H, W, 1), hole(H, W)
    rng = np.random.default_rng(5)
    A = (np.round(rng.uniform(-1, 1, (H, W)) * 256) / 256).astype(np.float32)
    B = (np.round(rng.uniform(-1, 1, (H, W)) * 256) / 256).astype(np.float32)
    pos = [(10, 20, 0)]
    ta, tb = ref.terms(X, phi, phi, pos, A)[0], ref.terms(X, phi, phi, pos, B)[0]
    assert np.any(ta != 0) and np.any(tb != 0)
    assert np.array_equal(ref.terms(X, phi, phi, pos, A + B)[0], ta + tb)
    assert np.array_equal(ref.terms(X, phi, phi, pos, 4 * A)[0], 4 * ta)
    assert ref.traces(X, phi, phi, pos, 4 * A)[0] == 4 * ref.traces(X, phi, phi, pos, A)[0]
    total = ref.traces(X, phi, phi, pos, A + B)[0]
    assert abs(total - (math.fsum(ta.tolist()) + math.fsum(tb.tolist()))) <= 2.0 ** -52 * abs(total)
    # several tables on one recorder: lead e uses the table it names
    both = ref.traces(X, phi, phi, [(10, 20, 0), (10, 20, 1)], np.stack([A, B]))
    assert both[0] == math.fsum(ta.tolist()) and both[1] == math.fsum(tb.tolist())


def test_reciprocity_of_mirrored_electrodes():
    from fib_tf_amd import leads
    """(on a state of few bits, multiples of 2^-10: the float32 stencil adds its taps in a fixed order, which a mirror changes —
    exact sums do not care; the phase term's products and quotient mirror exactly on any state)"""
    H, W = 37, 53
    X = (np.round(front(H, W, 2) * 1024) / 1024).astype(np.float32)
    X = (X + X[:, ::-1]).astype(np.float32)                   # symmetric about the vertical axis
    tab = leads.point_table(H, W, 1.5)
    a, b = ref.traces(X, None, None, [(12, 9, 0), (12, W - 1 - 9, 0)], tab)
    assert a != 0 and a == b
    X = (X + X[::-1]).astype(np.float32)
    phi = hole(H, W)
    phi = (phi * phi[::-1] * phi[:, ::-1] * phi[::-1, ::-1]).astype(np.float32)
    phi = np.maximum((phi + phi[::-1]) * np.float32(0.5), 1e-5).astype(np.float32)
    phi = np.maximum((phi + phi[:, ::-1]) * np.float32(0.5), 1e-5).astype(np.float32)
    assert np.array_equal(phi, phi[::-1]) and np.array_equal(phi, phi[:, ::-1])
    t = ref.terms(X, phi, phi, [(5, 9, 0), (H - 1 - 5, 9, 0), (5, W - 1 - 9, 0), (H - 1 - 5, W - 1 - 9, 0)], tab)
    # the vertical mirror flips the sign of S - N and of dpy together, the horizontal one E - W and dpx: the same terms, mirrored
    assert np.array_equal(t[0].reshape(H - 2, W - 2), t[1].reshape(H - 2, W - 2)[::-1])
    assert np.array_equal(t[0].reshape(H - 2, W - 2), t[2].reshape(H - 2, W - 2)[:, ::-1])
    v = ref.traces(X, phi, phi, [(5, 9, 0), (H - 1 - 5, 9, 0), (5, W - 1 - 9, 0), (H - 1 - 5, W - 1 - 9, 0)], tab)
    assert v[0] != 0 and v[0] == v[1] == v[2] == v[3]


@pytest.mark.parametrize('z,dx', [(2.0, 1.0), (0.5, 0.25), (7.3, 1.7)])
def test_point_table(z, dx):
    from fib_tf_amd import leads
    H, W = 19, 23
    T = leads.point_table(H, W, z, dx)
    assert T.shape == (H, W) and T.dtype == np.float32
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    exact = 1.0 / np.sqrt((i * dx) ** 2 + (j * dx) ** 2 + z * z)
    # half an ulp of the float32 result (plus the float64 evaluation's own error, 2^-29 of that)
    ulp = np.spacing(T).astype(np.float64)
    assert np.all(np.abs(T.astype(np.float64) - exact) <= 0.5 * ulp * (1 + 2.0 ** -28))
    assert T[0, 0] == np.float32(1.0 / z) and np.all(np.diff(T, axis=0) < 0) and np.all(np.diff(T, axis=1) < 0)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='z and dx'):
            leads.point_table(H, W, bad)
    with pytest.raises(ValueError, match='z and dx'):
        leads.point_table(H, W, 1.0, 0.0)


def test_argument_checks():
    from fib_tf_amd import leads
    H, W = 8, 9
    tab = leads.point_table(H, W, 2.0)
    pos, T = leads.parse_leads([(1, 2), (7, 8)], tab, None, H, W)
    assert pos.tolist() == [[1, 2, 0], [7, 8, 0]] and pos.dtype == np.int32 and T.shape == (1, H, W) and T.dtype == np.float32
    pos, T = leads.parse_leads([(1, 2), (3, 4)], np.stack([tab, 2 * tab]), [1, 0], H, W)
    assert pos.tolist() == [[1, 2, 1], [3, 4, 0]] and T.shape == (2, H, W)
    with pytest.raises(ValueError, match='1 .. 64 electrodes'):
        leads.parse_leads(np.zeros((0, 2), int), tab, None, H, W)
    with pytest.raises(ValueError, match='1 .. 64 electrodes'):
        leads.parse_leads([(1, 1)] * 65, tab, None, H, W)
    with pytest.raises(ValueError, match='1 .. 64 electrodes'):
        leads.parse_leads([(1, 1, 0)], tab, None, H, W)
    with pytest.raises(ValueError, match='integer cell'):
        leads.parse_leads([(1.5, 1)], tab, None, H, W)
    with pytest.raises(ValueError, match=r'electrode 1 at \(8, 0\) is outside the 8 x 9 grid'):
        leads.parse_leads([(0, 0), (8, 0)], tab, None, H, W)
    with pytest.raises(ValueError, match='outside'):
        leads.parse_leads([(0, -1)], tab, None, H, W)
    with pytest.raises(ValueError, match='1 .. 4 lead-field tables'):
        leads.parse_leads([(0, 0)], np.stack([tab] * 5), [0], H, W)
    with pytest.raises(ValueError, match=r'a table of shape \(9, 8\)'):
        leads.parse_leads([(0, 0)], tab.T, None, H, W)
    bad = tab.copy()
    bad[3, 3] = np.inf
    with pytest.raises(ValueError, match='not finite'):
        leads.parse_leads([(0, 0)], bad, None, H, W)
    with pytest.raises(ValueError, match='table_of must name one'):
        leads.parse_leads([(0, 0)], np.stack([tab, tab]), None, H, W)
    with pytest.raises(ValueError, match='one table index per electrode'):
        leads.parse_leads([(0, 0), (1, 1)], np.stack([tab, tab]), [0], H, W)
    with pytest.raises(ValueError, match='electrode 0 names table 2 of 2'):
        leads.parse_leads([(0, 0)], np.stack([tab, tab]), [2], H, W)


def test_sample_tick_rule():
    assert ref.sample_ticks(10, 1) == list(range(10))
    assert ref.sample_ticks(30, 10) == [9, 19, 29] and ref.sample_ticks(9, 10) == []


def test_sharded_undefined_and_zero_padded_models_are_refused():
    """the Python guards: nothing reaches the library"""
    from fib_tf_amd import leads
    from fib_tf_amd.sharded import ShardedStepper

    class M:
        VAR_NAMES = ('V',)
        height, width = 8, 9
        _stepper = ShardedStepper.__new__(ShardedStepper)
    M._stepper.world = 2
    tab = leads.point_table(8, 9, 1.0)
    with pytest.raises(NotImplementedError, match='single device'):
        leads.LeadRecorder(M(), [(1, 1)], tab)
    M._stepper = None
    with pytest.raises(AssertionError, match='after calling define'):
        leads.LeadRecorder(M(), [(1, 1)], tab)
    M._stepper = object()
    M._compiled = {'source': 'struct Custom {\n    static constexpr bool ZEROPAD = true;\n'}
    with pytest.raises(ValueError, match='zero-padded Laplacian'):
        leads.LeadRecorder(M(), [(1, 1)], tab)


def test_wavefront_input_gives_a_signal():
    """the input the device tests use has a front on the grid: the reference trace is far from zero against its own bound.  (3 x 3
    has ONE interior cell, every tap of which clamps onto it: its source is zero whatever the state)"""
    from fib_tf_amd import leads
    X = front(3, 3, 9)
    assert np.all(ref.terms(X, None, None, [(1, 1, 0)], leads.point_table(3, 3, 2.0)) == 0)
    for H, W in ((4, 64), (5, 3), (37, 53), (64, 64), (130, 67)):
        X = front(H, W, H * W)
        tab = leads.point_table(H, W, 2.0)
        pos = [(H // 2, W // 2, 0)]
        t = ref.terms(X, None, None, pos, tab)[0]
        v = ref.traces(X, None, None, pos, tab)[0]
        assert abs(v) > 100 * ref.bound(t) and v != 0, (H, W, v, ref.bound(t))
