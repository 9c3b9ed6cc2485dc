"""not-gpu: fibre fields (fib_tf_amd/tensor.py, include/fibhip.h fibhip_set_tensor) — the operator's restatement
(tests/tensor_ref.py) against the continuous operator and against the oracle at D = I, the host-side checks and guards, and the
second variant table of the built library."""
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import tensor_ref  # noqa: E402

FENTON, BR, COURT, COURT_US = 0, 1, 2, 3
PARENT_VARIANT_COUNT = 326       # fibhip_variant_count of the library before the second table existed
# csrc/launch.hpp g_tensor_variants: (model, mode) -> [(K, TX, TY, NT)], each under both policies
TENSOR_ROWS = {
    (FENTON, 0): [(10, 32, 32, 1024), (5, 32, 32, 512), (2, 64, 16, 256), (1, 64, 4, 256)],
    (BR, 0): [(5, 32, 32, 512), (1, 64, 4, 256)],
    (BR, 1): [(5, 32, 32, 512), (1, 64, 4, 256)],
    (COURT, 0): [(1, 64, 4, 256)],           # MODE_FAST
    (COURT, 2): [(1, 64, 4, 256)],           # MODE_ALL
    (COURT, 3): [(1, 64, 4, 256)],           # MODE_FASTSLOW
    (COURT_US, 2): [(1, 64, 4, 256)],
}


def _smooth_case(n):
    """a smooth fibre field (angle, ratio 3, scale all varying) and a smooth V on [0, 1]^2 with n points a side; float64"""
    h = 1.0 / (n - 1)
    y, x = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing='ij')
    th = 0.7 * np.sin(2 * x + y)
    s = (1 + 0.3 * np.cos(3 * y)) / 1.3
    r = 1.0 / 3.0
    c, sn = np.cos(th), np.sin(th)
    dxx, dyy, dxy = s * (c * c + r * sn * sn), s * (sn * sn + r * c * c), s * (1 - r) * c * sn
    V = np.sin(3 * x) * np.cos(2 * y) + x * y
    # div(D grad V), analytically differentiated where it is cheap: V's derivatives in closed form, D's by the product rule on
    # fourth-order differences of the smooth planes (their error, h^4, is far below the operator's h^2)
    Vx, Vy = 3 * np.cos(3 * x) * np.cos(2 * y) + y, -2 * np.sin(3 * x) * np.sin(2 * y) + x
    Vxx, Vyy, Vxy = -9 * np.sin(3 * x) * np.cos(2 * y), -4 * np.sin(3 * x) * np.cos(2 * y), -6 * np.cos(3 * x) * np.sin(2 * y) + 1

    def d4(A, axis):
        r1 = np.roll(A, -1, axis) - np.roll(A, 1, axis)
        r2 = np.roll(A, -2, axis) - np.roll(A, 2, axis)
        return (8 * r1 - r2) / (12 * h)
    exact = dyy * Vyy + 2 * dxy * Vxy + dxx * Vxx + (d4(dyy, 0) + d4(dxy, 1)) * Vy + (d4(dxy, 0) + d4(dxx, 1)) * Vx
    return h, V, dyy, dxx, dxy, exact


def test_operator_converges_at_second_order():
    err = []
    for n in (33, 65, 129):
        h, V, dyy, dxx, dxy, exact = _smooth_case(n)
        got = tensor_ref.laplace64(V, dyy, dxx, dxy) / (2 * h * h)          # the stencil's scale is 2 h^2
        m = (slice(3, -3), slice(3, -3))                                    # (away from the pad and the rolled differences)
        err.append(np.abs(got - exact)[m].max())
    print('errors', err, 'ratios', err[0] / err[1], err[1] / err[2])
    assert 3.5 < err[0] / err[1] < 4.5 and 3.5 < err[1] / err[2] < 4.5, err


@pytest.mark.parametrize('hole', [False, True], ids=['plain', 'hole'])
def test_identity_tensor_is_the_reference_stencil(hole):
    import oracle
    H, W = 9, 11
    rng = np.random.default_rng(5)
    X = rng.standard_normal((H, W)).astype(np.float32)
    phi = None
    if hole:
        rows, cols = np.arange(H)[:, None] - 4, np.arange(W)[None, :] - 5
        phi = np.maximum(np.array(0.5 * (np.tanh(np.hypot(cols, rows) - 2.0) + 1.0), np.float32), np.float32(1e-5))
    one, zero = np.ones((H, W), np.float32), np.zeros((H, W), np.float32)
    Xb = oracle.enforce_boundary(X)
    want = oracle.laplace(Xb, phi)
    got = tensor_ref.laplace32(Xb, one, one, zero, phi)
    assert np.array_equal(got, want)
    assert abs(tensor_ref.laplace64(Xb, one, one, zero, phi) - want.astype(np.float64)).max() < 1e-4


def test_fibre_tensor_planes_and_weights():
    from fib_tf_amd import tensor
    rng = np.random.default_rng(1)
    ang, ratio, scale = rng.uniform(-3, 3, (6, 7)), rng.uniform(1, 3, (6, 7)), rng.uniform(0.2, 1, (6, 7))
    got, want = tensor.fibre_tensor(ang, ratio, scale), tensor_ref.fibre_planes(ang, ratio, scale)
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == (6, 7) and np.array_equal(g, w)
    for g, w in zip(tensor.weights(*got), tensor_ref.weights(*want)):
        assert g.dtype == np.float32 and np.array_equal(g, w)
    tensor.check_tensor(*got)
    # fibres along the columns: the column direction conducts `ratio` times better
    dyy, dxx, dxy = tensor.fibre_tensor(0.0, 2.0, shape=(3, 4))
    assert np.all(dxx == 1) and np.all(dyy == 0.5) and np.all(dxy == 0)
    # the eigenvalues are scale and scale / ratio, the eigenvector of the larger one is the fibre direction
    dyy, dxx, dxy = (float(p[0, 0]) for p in tensor.fibre_tensor(0.6, 2.5, 0.8, shape=(3, 3)))
    lam, vec = np.linalg.eigh(np.array([[dyy, dxy], [dxy, dxx]]))
    assert np.allclose(lam, [0.8 / 2.5, 0.8], rtol=1e-6)
    assert abs(abs(vec[:, 1] @ np.array([np.sin(0.6), np.cos(0.6)])) - 1) < 1e-6
    with pytest.raises(ValueError, match=r'\[H, W\]'):
        tensor.fibre_tensor(0.0, 2.0)
    with pytest.raises(ValueError, match='>= 1'):
        tensor.fibre_tensor(0.0, 0.5, shape=(3, 3))
    with pytest.raises(ValueError, match=r'scale must be in \(0, 1\]'):
        tensor.fibre_tensor(0.0, 2.0, 1.5, shape=(3, 3))


def test_monotone_up_to_ratio_three():
    from fib_tf_amd import tensor
    assert tensor.is_monotone(*tensor.fibre_tensor(np.pi / 4, 3.0, shape=(4, 4)))
    assert not tensor.is_monotone(*tensor.fibre_tensor(np.pi / 4, 3.01, shape=(4, 4)))
    th = np.linspace(0, np.pi, 721)[None, :]
    assert tensor.is_monotone(*tensor.fibre_tensor(th, 2.999))
    # (along an axis the bound is the same: the weight of the taps across the fibres, 1.5 / ratio - 0.5, changes sign at 3)
    assert tensor.is_monotone(*tensor.fibre_tensor(0.0, 3.0, shape=(3, 3))) and not tensor.is_monotone(*tensor.fibre_tensor(0.0, 3.01, shape=(3, 3)))


def test_check_tensor_refusals():
    from fib_tf_amd import tensor
    one, zero = np.ones((4, 5), np.float32), np.zeros((4, 5), np.float32)
    bad = one.copy()
    bad[2, 3] = np.nan
    for planes in ((bad, one, zero), (one, bad, zero), (one, one, bad * 0)):
        with pytest.raises(ValueError, match='not finite everywhere'):
            tensor.check_tensor(*planes)
    with pytest.raises(ValueError, match='not finite everywhere'):
        tensor.check_tensor(one, one * np.inf, zero)
    for planes in ((0.5 * one, 0.5 * one, 0.5 * one), (zero, one, zero), (-one, one, zero), (0.5 * one, 0.5 * one, -0.6 * one)):
        with pytest.raises(ValueError, match='not positive definite everywhere'):
            tensor.check_tensor(*planes)
    with pytest.raises(ValueError, match='largest eigenvalue is above 1.*raise diff instead'):
        tensor.check_tensor(1.001 * one, one, zero)
    with pytest.raises(ValueError, match='largest eigenvalue is above 1'):
        tensor.check_tensor(0.9 * one, 0.9 * one, 0.2 * one)
    tensor.check_tensor(one, one, zero)                                   # the identity is the largest tensor there is
    tensor.check_tensor(*tensor.fibre_tensor(0.3, 2.0, 1.0, shape=(4, 5)))  # ... and rounding does not push a unit tensor over
    with pytest.raises(ValueError, match='the grid is'):
        tensor.check_tensor(one, one, zero, shape=(5, 4))
    with pytest.raises(ValueError, match='one shape'):
        tensor.check_tensor(one, one[:3], zero)
    # the library's words (csrc/fibhip.hip tensor_check) are these
    src = open(os.path.join(ROOT, 'fib_tf_amd', 'csrc', 'fibhip.hip')).read()
    for msg in (tensor.NOT_FINITE, tensor.NOT_SPD, tensor.OVER_UNIT):
        assert '"%s"' % msg in src, msg


def _model(**extra):
    from fib_tf_amd.fenton import Fenton4v
    cfg = {'width': 12, 'height': 10, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 1}
    cfg.update(extra)
    return Fenton4v(cfg)


def test_model_api_and_guards():
    from fib_tf_amd import tensor
    m = _model()
    assert m.tensor is None
    m.set_fibres(0.4, 2.0)
    want = tensor.fibre_tensor(0.4, 2.0, shape=(10, 12))
    assert all(np.array_equal(a, b) for a, b in zip(m.tensor, want))
    m.set_tensor(None, None, None)
    assert m.tensor is None
    with pytest.raises(ValueError, match='not positive definite'):
        m.set_tensor(np.ones((10, 12)), np.ones((10, 12)), np.ones((10, 12)))
    with pytest.raises(ValueError, match='the grid is'):
        m.set_tensor(*tensor.fibre_tensor(0.0, 2.0, shape=(12, 10)))
    # the configuration keys of the uniform case
    c = _model(fibre_angle=0.25, anisotropy=3.0)
    assert all(np.array_equal(a, b) for a, b in zip(c.tensor, tensor.fibre_tensor(0.25, 3.0, shape=(10, 12))))
    assert _model(anisotropy=2.0).tensor[1][0, 0] == 1.0 and _model(anisotropy=2.0).tensor[0][0, 0] == 0.5
    # above ratio 3 at an oblique angle: one warning per process
    tensor._warned[0] = False
    with pytest.warns(RuntimeWarning, match='negative weight'):
        _model().set_fibres(0.7, 4.0)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        _model().set_fibres(0.7, 5.0)
    # before define() only
    m.set_fibres(0.4, 2.0)
    m.defined = True
    with pytest.raises(AssertionError, match='before calling define'):
        m.set_fibres(0.4, 2.0)
    with pytest.raises(AssertionError, match='before calling define'):
        m.set_tensor(*want)
    # what reads the isotropic operator or recomputes the phase planes raises before anything reaches the library
    m._stepper = object()
    table = np.ones((10, 12), np.float32)
    for call, who in ((lambda: m.record_leads([(3, 3)], table), 'record_leads'),
                      (lambda: m.record_potential_map(np.ones((3, 3), np.float32)), 'record_potential_map'),
                      (lambda: m.program_lesions([]), 'program_lesions'),
                      (lambda: m.ablate(('disc', 4, 4, 2)), 'ablate')):
        with pytest.raises(ValueError, match=who + ': not on a model with a diffusion tensor'):
            call()
    m._stepper = None


def test_row_blocks_and_traced_models_are_refused():
    from fib_tf_amd import sharded, traced
    from fib_tf_amd.sharded import ShardedStepper
    st = ShardedStepper.__new__(ShardedStepper)
    st.world = 2
    with pytest.raises(NotImplementedError, match='set_tensor: .* on a single device only; this model runs as row blocks over 2 ranks'):
        st.set_tensor(None)
    m = _model()
    m.set_fibres(0.0, 2.0)
    saved = sharded.dist_world
    sharded.dist_world = lambda: (0, 2)
    try:
        with pytest.raises(NotImplementedError, match='single device only; this model runs as row blocks over 2 ranks'):
            m._new_stepper()
    finally:
        sharded.dist_world = saved
    t = traced.IonicModel({'width': 12, 'height': 10, 'dt': 0.1, 'diff': 1.0})
    with pytest.raises(NotImplementedError, match='set_tensor: .* this model is traced'):
        t.set_fibres(0.0, 2.0)
    with pytest.raises(NotImplementedError, match='this model is traced'):
        traced.IonicModel({'width': 12, 'height': 10, 'dt': 0.1, 'diff': 1.0, 'anisotropy': 2.0})


def test_new_symbols_are_bound_and_declared():
    from fib_tf_amd import _lib
    hdr = open(_lib.HDR).read()
    L = _lib.lib()
    for name in ('fibhip_set_tensor', 'fibhip_tensor_variant_count', 'fibhip_tensor_variant_info', 'fibhip_unit_laplace_tensor'):
        assert name in _lib.SYMBOLS and re.search(r'\bint %s\(' % name, hdr), name
        assert getattr(L, name).argtypes is not None
    assert L.fibhip_abi_version() == 1


def test_tensor_variant_table():
    from fib_tf_amd import _lib
    L = _lib.lib()
    rows = _lib.tensor_variants()
    assert len(rows) == L.fibhip_tensor_variant_count()
    want = {(model, mode, fast, 1) + shape for (model, mode), shapes in TENSOR_ROWS.items() for shape in shapes for fast in (0, 1)}
    got = [tuple(r[k] for k in ('model', 'mode', 'fast', 'phase', 'K', 'TX', 'TY', 'NT')) for r in rows]
    assert len(got) == len(set(got)) and set(got) == want
    assert len(got) == 2 * sum(len(s) for s in TENSOR_ROWS.values())
    for r in rows:
        assert r['kind'] == _lib.MK_TICK and r['has_mt'] == 0 and r['phase'] == 1, r
        assert r['NT'] % 64 == 0 and 64 <= r['NT'] <= 1024, r
    for (model, mode) in TENSOR_ROWS:
        for fast in (0, 1):
            assert any(r['model'] == model and r['mode'] == mode and r['fast'] == fast and r['K'] == 1 for r in rows), (model, mode, fast)
    out = (_lib.C.c_int * 10)()
    for i in (-1, len(rows)):
        assert L.fibhip_tensor_variant_info(i, out) < 0 and b'tensor_variant_info' in L.fibhip_last_error()
    # the first table is what it was: the second one is no part of it
    assert L.fibhip_variant_count() == PARENT_VARIANT_COUNT
    assert {r['model'] for r in _lib.variants()} == {0, 1, 2, 3, 100, 101}
