"""not-gpu: the statistics recorder's host side — the NumPy restatement (tests/stats_ref.py) against the expressions it stands
for (np.average with weights, the ρ of court_ultra.run_small), its edge cases, the sample-tick rule, and StatsRecorder's column
parsing, table and finite check (fib_tf_amd/stats.py), which need no device."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stats_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('V', '_Na_i_', '_f_Ca_', '_j_')


def test_declarations_and_binding():
    from fib_tf_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    for name in ('fibhip_stats_begin', 'fibhip_stats_count', 'fibhip_stats_read', 'fibhip_stats_end'):
        assert 'int %s(' % name in src
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is _lib.C.c_int
    assert len(_lib.SYMBOLS['fibhip_stats_begin'][0]) == 7
    assert [f[0] for f in _lib.StatCol._fields_] == ['var', 'kind', 'level'] and _lib.C.sizeof(_lib.StatCol) == 12
    order = [k.lower() for k in __import__('re').findall(r'FIBHIP_STAT_([A-Z]+) = \d', src)]
    assert tuple(order) == _lib.STAT_KINDS == ref.KINDS
    assert '#define FIBHIP_MAX_STAT_COLS %d' % _lib.MAX_STAT_COLS in src
    assert '#define FIBHIP_MAX_STAT_COLS_PER_ARRAY %d' % _lib.MAX_STAT_COLS_PER_ARRAY in src
    assert '#define FIBHIP_ABI_VERSION 1' in src


@pytest.mark.parametrize('seed', range(4))
def test_mean_is_np_average(seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(37, 53)) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
    w = rng.uniform(0, 1, (37, 53)).astype(np.float32)
    w[rng.uniform(size=w.shape) < 0.2] = 0
    wsum = math.fsum(w.astype(np.float64).ravel().tolist())
    mean = ref.value(x, 'sum', weight=w) / wsum
    want = np.average(x.astype(np.float64), weights=w.astype(np.float64))
    n = int(np.count_nonzero(w))
    bound = n * 2.0 ** -53 * float(np.sum(np.abs(w.astype(np.float64) * x.astype(np.float64)))) / wsum
    assert abs(mean - want) <= bound, (mean, want, bound)
    # without a plane: the plain sum
    assert ref.value(x, 'sum') == math.fsum(x.astype(np.float64).ravel().tolist())


@pytest.mark.parametrize('seed', range(4))
def test_rho_is_run_smalls_expression(seed):
    rng = np.random.default_rng(10 + seed)
    lo, span = np.float32(-100.0), np.float32(150.0)
    V = rng.uniform(-90, 30, (40, 44)).astype(np.float32)
    from fib_tf_amd import court_ultra

    class M:
        def _frame_levels(self):
            return float(lo), float(span)
    L = court_ultra.image_level(M(), 0.2)
    L32 = np.float32(L)
    for v in (L32, np.nextafter(L32, np.float32(-np.inf)), np.nextafter(L32, np.float32(np.inf))):       # exactly at the level
        V[rng.integers(0, 40), rng.integers(0, 44)] = v
    V[3, 3] = np.nan
    phase = rng.uniform(0, 1, (40, 44)).astype(np.float32)
    phase[rng.uniform(size=phase.shape) < 0.3] = 1e-5
    image = (V - lo) / span
    with np.errstate(invalid='ignore'):
        rho = np.sum(image[phase > 1e-3] < 0.2) / np.sum(phase > 1e-3)
    mask = phase > 1e-3
    got = ref.value(V, 'below', L, mask=mask) / np.count_nonzero(mask)
    assert got == rho
    assert (L32 - lo) / span >= np.float32(0.2) and (np.nextafter(L32, np.float32(-np.inf)) - lo) / span < np.float32(0.2)


def test_edge_cases():
    x = np.array([[1.0, -2.0, np.nan], [np.inf, -np.inf, 0.0]], np.float32)
    none = np.zeros((2, 3), np.uint8)
    assert ref.value(x, 'min', mask=none) == np.inf and ref.value(x, 'max', mask=none) == -np.inf       # an empty mask
    assert ref.value(x, 'below', 5.0, mask=none) == 0 and ref.value(x, 'nonfinite', mask=none) == 0
    nan = np.full((2, 3), np.nan, np.float32)
    assert ref.value(nan, 'min') == np.inf and ref.value(nan, 'max') == -np.inf                          # NaN only
    assert ref.value(nan, 'below', 0.0) == 0 and ref.value(nan, 'above', 0.0) == 0 and ref.value(nan, 'nonfinite') == 6
    assert ref.value(x, 'min') == -np.inf and ref.value(x, 'max') == np.inf                             # +-Inf take part
    assert ref.value(x, 'nonfinite') == 3
    assert ref.value(x, 'below', 0.0) == 2 and ref.value(x, 'above', 0.0) == 2                           # NaN in neither
    fin = np.array([[1, 1, 0], [0, 0, 1]], np.uint8)
    assert ref.value(x, 'min', mask=fin) == -2.0 and ref.value(x, 'max', mask=fin) == 1.0
    z = np.array([[0.0, -0.0]], np.float32)
    assert ref.value(z, 'min') == 0.0 and ref.value(z, 'max') == 0.0                                     # -0 == +0
    assert ref.value(z, 'below', 0.0) == 0 and ref.value(z, 'above', -0.0) == 0
    w = np.array([[1, 1, 0], [0, 0, 2]], np.float32)
    assert ref.value(x, 'sum', weight=w) == -1.0                                                         # NaN, Inf under zero weights
    assert math.isnan(ref.value(x, 'sum', weight=np.ones((2, 3), np.float32)))
    w[0, 2] = 1
    assert math.isnan(ref.value(x, 'sum', weight=w))
    w[0, 2], w[1, 0] = 0, 1
    assert ref.value(x, 'sum', weight=w) == np.inf


def test_sample_tick_rule():
    assert ref.sample_ticks(10, 1) == list(range(10))
    assert ref.sample_ticks(10, 3) == [2, 5, 8]
    assert ref.sample_ticks(9, 10) == [] and ref.sample_ticks(10, 10) == [9]
    from fib_tf_amd import stats
    cols = stats.parse_columns([('V', 'min')], NAMES)
    t = stats.make_table(np.zeros((3, 1)), cols, 1.0, 1, 3, 0.5)
    assert t['t_ms'].tolist() == [(k + 1) * 0.5 for k in ref.sample_ticks(10, 3)]


def test_column_parsing_and_errors():
    from fib_tf_amd import stats
    cols = stats.parse_columns([('V', 'mean'), ('_Na_i_', 'mean'), (2, 'mean'), ('V', 'below', -55.0), ('V', 'min'), ('V', 'max'),
                                ('V', 'nonfinite'), ('V', 'frac_above', -20), ('V', 'below', -70.0)], NAMES)
    assert [c.field for c in cols] == ['V_mean', '_Na_i__mean', '_f_Ca__mean', 'V_below', 'V_min', 'V_max', 'V_nonfinite',
                                       'V_frac_above', 'V_below_2']
    assert stats.device_columns(cols) == [(0, 'sum', 0.0), (1, 'sum', 0.0), (2, 'sum', 0.0), (0, 'below', -55.0), (0, 'min', 0.0),
                                          (0, 'max', 0.0), (0, 'nonfinite', 0.0), (0, 'above', -20.0), (0, 'below', -70.0)]
    assert stats.table_dtype(cols).names == ('t_ms',) + tuple(c.field for c in cols)
    with pytest.raises(ValueError, match="unknown array 'Vm'"):
        stats.parse_columns([('Vm', 'mean')], NAMES)
    with pytest.raises(ValueError, match='array index 4'):
        stats.parse_columns([(4, 'mean')], NAMES)
    with pytest.raises(ValueError, match="unknown kind 'median'"):
        stats.parse_columns([('V', 'median')], NAMES)
    with pytest.raises(ValueError, match="more than 8 columns on array 'V'"):
        stats.parse_columns([('V', 'below', float(i)) for i in range(9)], NAMES)
    assert len(stats.parse_columns([('V', 'below', float(i)) for i in range(8)] + [('_j_', 'min')], NAMES)) == 9
    with pytest.raises(ValueError, match='needs a level'):
        stats.parse_columns([('V', 'below')], NAMES)
    with pytest.raises(ValueError, match='needs a level'):
        stats.parse_columns([('V', 'frac_below', float('nan'))], NAMES)
    with pytest.raises(ValueError, match='takes no level'):
        stats.parse_columns([('V', 'max', 1.0)], NAMES)
    with pytest.raises(ValueError, match='1 .. 64 columns'):
        stats.parse_columns([], NAMES)
    with pytest.raises(ValueError, match='1 .. 64 columns'):
        stats.parse_columns([(i % 4, 'min') for i in range(65)], NAMES)
    with pytest.raises(ValueError, match='a column is'):
        stats.parse_columns(['V'], NAMES)


def test_table_and_finite_check():
    from fib_tf_amd import stats
    cols = stats.parse_columns([('V', 'mean'), ('V', 'frac_below', -55.0), ('V', 'nonfinite'), ('V', 'min'), ('_j_', 'sum')], NAMES)
    raw = np.array([[10.0, 5.0, 0.0, -80.0, 3.0], [20.0, 10.0, 0.0, -81.0, 4.0], [np.nan, 9.0, 2.0, -82.0, 5.0],
                    [30.0, 20.0, 0.0, -83.0, 6.0]])
    t = stats.make_table(raw, cols, 4.0, 20, 10, 0.1)
    assert t.dtype.names == ('t_ms', 'V_mean', 'V_frac_below', 'V_nonfinite', 'V_min', '_j__sum')
    assert np.allclose(t['t_ms'], [1.0, 2.0, 3.0, 4.0])
    assert t['V_mean'][:2].tolist() == [2.5, 5.0] and t['V_frac_below'].tolist() == [0.25, 0.5, 0.45, 1.0]
    assert t['V_min'].tolist() == [-80.0, -81.0, -82.0, -83.0] and t['_j__sum'].tolist() == [3.0, 4.0, 5.0, 6.0]
    stats.check_finite(raw[:2], cols, 20, 10, 0.1)
    assert stats.first_nonfinite(raw, cols, 20) == (2, 0)
    with pytest.raises(FloatingPointError, match=r'sample 2 \(after tick 29'):
        stats.check_finite(raw, cols, 20, 10, 0.1)
    only_count = raw.copy()
    only_count[2, 0] = 25.0
    assert stats.first_nonfinite(only_count, cols, 20) == (2, 2)
    with pytest.raises(FloatingPointError, match='V_nonfinite'):
        stats.check_finite(only_count, cols, 20, 10, 0.1)
    inf_min = raw[:2].copy()
    inf_min[1, 3] = -np.inf
    assert stats.first_nonfinite(inf_min, cols, 20) == (1, 3)
    assert stats.first_nonfinite(np.array([[1.0, 1.0, 0.0, np.inf, 1.0]]), cols, 0) is None      # an empty mask: MIN is +inf
    assert stats.weight_sum(None, 12) == 12.0
    w = np.array([[0.5, 0.0], [0.25, 1e-8]], np.float32)
    assert stats.weight_sum(w, 4) == math.fsum([0.5, 0.25, float(np.float32(1e-8))])


def test_sharded_model_is_refused():
    """the Python guard: a model whose stepper is a ShardedStepper raises NotImplementedError before anything reaches the library"""
    from fib_tf_amd import stats
    from fib_tf_amd.sharded import ShardedStepper

    class M:
        VAR_NAMES = NAMES
        _stepper = ShardedStepper.__new__(ShardedStepper)
    M._stepper.world = 2
    with pytest.raises(NotImplementedError, match='single device'):
        stats.StatsRecorder(M(), [('V', 'mean')])
    M._stepper = None
    with pytest.raises(AssertionError, match='after calling define'):
        stats.StatsRecorder(M(), [('V', 'mean')])
