"""the wave recorder without a device: the NumPy restatement of its definition (tests/wave_ref.py) against scipy.ndimage.label and
a direct per-component computation, the crafted planes the device tests use, the declarations, the bindings and the Python guards."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('fibhip_waves_begin', 'fibhip_waves_count', 'fibhip_waves_read', 'fibhip_waves_labels', 'fibhip_waves_end')
TILE = (16, 64)                                               # wave_label_kernel's tile: rows x columns
PERCOLATION = 0.5927                                          # site percolation threshold of the square lattice: large ragged clusters


# ---- the crafted planes (shared with tests/test_gpu_waves.py) ------------------------------------------------------------
def cells_plane(H, W, cells):
    """only `cells` set; None where one of them is outside the grid"""
    s = np.zeros((H, W), bool)
    for r, c in cells:
        if not (0 <= r < H and 0 <= c < W):
            return None
        s[r, c] = True
    return s


def serpentine(H, W):
    """one cell wide, through every tile: the even rows whole, joined at alternating ends — ONE wave, the longest path there is"""
    s = np.zeros((H, W), bool)
    s[0::2] = True
    for r in range(1, H, 2):
        s[r, W - 1 if (r // 2) % 2 == 0 else 0] = True
    return s


def spiral(H, W):
    r, c = np.mgrid[0:H, 0:W]
    y, x = r - 0.5 * H, c - 0.5 * W
    rho, theta = np.hypot(y, x), np.arctan2(y, x)
    pitch = max(4.0, min(H, W) / 3.0)
    return ((rho / pitch - theta / (2 * np.pi)) % 1.0 < 0.4) & (rho > 1.0)


def ring(H, W):
    r, c = np.mgrid[0:H, 0:W]
    d = np.hypot(r - 0.5 * (H - 1), c - 0.5 * (W - 1))
    return (d <= 0.45 * min(H, W)) & (d >= 0.25 * min(H, W))


def checkerboard(H, W):
    r, c = np.mgrid[0:H, 0:W]
    return (r + c) % 2 == 0


def random_plane(H, W, seed, density=PERCOLATION):
    return np.random.default_rng(1000 * seed + 31 * H + W).uniform(size=(H, W)) < density


def crafted(H, W):
    """name -> plane, every crafted geometry that fits the grid"""
    ty, tx = TILE
    out = {'empty': np.zeros((H, W), bool), 'full': np.ones((H, W), bool), 'single': cells_plane(H, W, [(H // 2, W // 2)]),
           'corner-diagonal': cells_plane(H, W, [(ty - 1, tx - 1), (ty, tx)]),
           'corner-antidiagonal': cells_plane(H, W, [(ty - 1, tx), (ty, tx - 1)]),
           'across-a-tile-row': cells_plane(H, W, [(ty - 1, 5), (ty, 5), (2 * ty - 1, W - 1), (2 * ty, W - 1)]),
           'across-a-tile-column': cells_plane(H, W, [(0, tx - 1), (0, tx), (H - 1, tx - 1), (H - 1, tx)]),
           'serpentine': serpentine(H, W), 'spiral': spiral(H, W), 'ring': ring(H, W), 'checkerboard': checkerboard(H, W)}
    for seed in (1, 2, 3):
        out['random-%d' % seed] = random_plane(H, W, seed)
    return {k: v for k, v in out.items() if v is not None}


# ---- the restatement -----------------------------------------------------------------------------------------------------
def direct_records(labels):
    """per component, straight from the definition"""
    H, W = labels.shape
    out = []
    for seed in np.unique(labels[labels >= 0]):
        r, c = np.nonzero(labels == seed)
        out.append((seed, len(r), int(r.sum()), int(c.sum()), r.min(), r.max(), c.min(), c.max()))
    return np.array(out, ref.RECORD_DTYPE) if out else np.zeros(0, ref.RECORD_DTYPE)


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('shape', [(5, 3), (37, 53), (130, 67)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('density', [0.3, 0.5, 0.7])
def test_label_equals_scipy(shape, density, conn):
    ndimage = pytest.importorskip('scipy.ndimage')
    H, W = shape
    s = random_plane(H, W, int(density * 10), density)
    structure = np.ones((3, 3), int) if conn == 8 else None
    theirs, n = ndimage.label(s, structure=structure)
    # scipy's labels mapped to the smallest linear index of each component: partition and seeds must be identical
    flat = theirs.ravel()
    first = np.full(n + 1, H * W, np.int64)
    np.minimum.at(first, flat, np.arange(H * W))
    want = np.where(flat > 0, first[flat], -1).reshape(H, W).astype(np.int32)
    got = ref.label(s, conn)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    counts, rec, lab = ref.sample(s, conn)
    assert counts.tolist() == [n, n, int(s.sum())] and np.array_equal(lab, got)
    direct = direct_records(got)
    assert len(rec) == n and all(np.array_equal(rec[f], direct[f]) for f in ref.FIELDS)
    assert np.all(np.diff(rec['seed']) > 0) and int(rec['area'].sum()) == int(s.sum())


def test_crafted_planes_are_what_they_claim():
    H, W = 130, 67
    planes = crafted(H, W)
    assert len(planes) == 14
    n = {(k, conn): ref.sample(v, conn)[0][0] for k, v in planes.items() for conn in (4, 8)}
    assert n['empty', 4] == 0 and n['full', 4] == 1 and n['single', 8] == 1
    assert (n['corner-diagonal', 4], n['corner-diagonal', 8]) == (2, 1)
    assert (n['corner-antidiagonal', 4], n['corner-antidiagonal', 8]) == (2, 1)
    assert n['across-a-tile-row', 4] == 2 and n['across-a-tile-column', 4] == 2
    assert n['serpentine', 4] == 1 and n['ring', 4] == 1 and n['spiral', 4] >= 1
    assert n['checkerboard', 4] == (H * W + 1) // 2 and n['checkerboard', 8] == 1
    counts, rec, lab = ref.sample(planes['ring'], 4)
    assert lab[H // 2, W // 2] == -1 and rec['area'][0] > TILE[0] * TILE[1]
    # the serpentine visits every tile
    s = planes['serpentine']
    for y0 in range(0, H, TILE[0]):
        for x0 in range(0, W, TILE[1]):
            assert s[y0:y0 + TILE[0], x0:x0 + TILE[1]].any()
    # a small grid keeps what fits
    assert 'corner-diagonal' not in crafted(37, 53) and 'across-a-tile-row' in crafted(37, 53)


def test_set_plane_compares_strictly_and_never_sets_a_nan():
    X = np.array([[0.5, 0.25, np.nan], [np.inf, -np.inf, 0.75]], np.float32)
    assert ref.set_plane(X, 0.5, 'above').tolist() == [[False, False, False], [True, False, True]]
    assert ref.set_plane(X, 0.5, 'below').tolist() == [[False, True, False], [False, True, False]]
    G = np.array([[1, 1, 1], [0, 1, 1]], np.float32)
    assert ref.set_plane(X, 0.1, 'above', mask=[[1, 1, 1], [1, 1, 0]], also=(G, 'above', 0.5)).tolist() == [[True, True, False], [False, False, False]]
    with pytest.raises(ValueError):
        ref.set_plane(X, 0.5, 'beside')
    with pytest.raises(ValueError):
        ref.label(X > 0, 6)


# ---- declarations, bindings, guards ----------------------------------------------------------------------------------------
def test_declarations_and_binding():
    from fib_tf_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    assert '#define FIBHIP_ABI_VERSION 1\n' in src
    for name in ENTRY_POINTS:
        assert 'int %s(' % name in src
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is _lib.C.c_int
    assert len(_lib.SYMBOLS['fibhip_waves_begin'][0]) == 12
    assert '#define FIBHIP_MAX_WAVES %d\n' % _lib.MAX_WAVES in src
    assert _lib.WAVE_RECORD_DTYPE.itemsize == 40 and _lib.WAVE_RECORD_DTYPE == ref.RECORD_DTYPE
    for s in ('waves_begin', 'waves_count', 'waves_read', 'waves_labels', 'waves_end'):
        assert callable(getattr(_lib.Stepper, s))


def test_library_exports_the_entry_points():
    """the built library (dlopen needs no device) exports the five entry points by name"""
    from fib_tf_amd import _lib
    L = _lib.C.CDLL(_lib.SO)
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None, name


class _NoLibrary:
    def waves_begin(self, *a):
        raise AssertionError('the guard let the call through to the library')


class _Model:
    VAR_NAMES = ('V', 'g')
    height, width = 8, 9
    min_v, max_v = 0.0, 1.0
    dt, dt_per_step, duration = 0.1, 10, 100
    phase = None
    _stepper = _NoLibrary()


def test_python_guards():
    """nothing reaches the library"""
    from fib_tf_amd import waves
    from fib_tf_amd.sharded import ShardedStepper

    class Sharded(_Model):
        _stepper = ShardedStepper.__new__(ShardedStepper)
    Sharded._stepper.world = 2
    with pytest.raises(NotImplementedError, match='single device'):
        waves.WaveRecorder(Sharded)
    with pytest.raises(ValueError, match='conn is 4 or 8'):
        waves.WaveRecorder(_Model, conn=6)
    with pytest.raises(ValueError, match="'above' or 'below'"):
        waves.WaveRecorder(_Model, kind='beside')
    with pytest.raises(ValueError, match="'above' or 'below'"):
        waves.WaveRecorder(_Model, also=('g', 'over', 0.5))
    for bad in (0, 65537):
        with pytest.raises(ValueError, match='max_waves is 1 .. 65536'):
            waves.WaveRecorder(_Model, max_waves=bad)
    for bad in (np.nan, np.inf, 1e39):
        with pytest.raises(ValueError, match='level must be finite'):
            waves.WaveRecorder(_Model, level=bad)
    with pytest.raises(ValueError, match="also's level must be finite"):
        waves.WaveRecorder(_Model, also=('g', 'above', -np.inf))
    with pytest.raises(ValueError, match='unknown array'):
        waves.WaveRecorder(_Model, var='h')
    with pytest.raises(ValueError, match='every must be >= 1'):
        waves.WaveRecorder(_Model, every=0)
    with pytest.raises(ValueError, match='a mask of shape'):
        waves.WaveRecorder(_Model, mask=np.ones((3, 3)))
    with pytest.raises(AssertionError, match='let the call through'):       # (the stand-in does refuse what the guards pass)
        waves.WaveRecorder(_Model)


def test_default_mask_and_level():
    from fib_tf_amd import waves
    from fib_tf_amd.activation import default_thresholds

    class M(_Model):
        phase = np.ones((8, 9), np.float32)
    M.phase[3, 4] = 0.2
    mask = waves.default_mask(M)
    assert mask.dtype == bool and not mask[0].any() and not mask[-1].any() and not mask[:, 0].any() and not mask[:, -1].any()
    assert not mask[3, 4] and mask[1:-1, 1:-1].sum() == 6 * 7 - 1
    assert waves.default_mask(_Model)[1:-1, 1:-1].all()
    assert default_thresholds(0.0, 1.0)[0] == np.float32(0.5)
