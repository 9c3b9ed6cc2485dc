"""-m gpu: the lead recorder (include/fibhip.h fibhip_leads_*, fib_tf_amd/leads.py) on the device.

Every sample is compared with the NumPy restatement (tests/lead_ref.py) on the state read back at the sample's tick.  The terms
(double)K * (double)q are exact, so all the device may differ by is the order of its float64 summation:
|device - fsum(terms)| <= n u / (1 - n u) * sum |terms|, n the interior cells, u = 2^-53 — the standard bound for a float64 sum of
n terms in ANY order, derived and not measured (one float32 rounding anywhere in the source misses it by nine orders of
magnitude).  The grids are the smallest that reach every path of lead_kernel: 3 x 3 (one interior cell), 5 x 3 and 4 x 64 (less
than a tile either way, W a multiple of 4 and not), 37 x 53 (odd everything, three tile rows), 64 x 64 (tiles exactly full) and
130 x 67 (more than one tile both ways, a last tile of two rows and of three columns)."""
import contextlib
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lead_ref as ref  # noqa: E402
from test_gpu_frames import PLAN_ENV, VARIANT_96x100, wave  # noqa: E402
from test_gpu_tips import fenton  # noqa: E402
from test_leads_cpu import front, hole  # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = [(3, 3), (4, 64), (5, 3), (37, 53), (64, 64), (130, 67)]
TILE = (16, 64)                                               # lead_kernel's tile: rows x columns


def tables_for(H, W, n=4):
    from fib_tf_amd import leads
    rng = np.random.default_rng(H * 1000 + W)
    out = [leads.point_table(H, W, 2.0), leads.point_table(H, W, 0.5, 0.3), rng.uniform(-1, 1, (H, W)).astype(np.float32),
           (rng.normal(size=(H, W)) * 10.0 ** rng.uniform(-3, 3, (H, W))).astype(np.float32)]
    return np.stack(out[:n])


def positions(H, W, n, ntables):
    """the four corners, both sides of a tile seam (the grid's far corner where it has none), the centre; then random cells"""
    rng = np.random.default_rng(H + 7 * W)
    fixed = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (min(TILE[0] - 1, H - 1), min(TILE[1] - 1, W - 1)),
             (min(TILE[0], H - 1), min(TILE[1], W - 1)), (H // 2, W // 2)]
    cells = fixed + [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(max(0, n - len(fixed)))]
    return [(r, c, e % ntables) for e, (r, c) in enumerate(cells[:n])]


def compare(row, X, phase, weight, pos, tables, what):
    """one sample against the restatement; -> (largest |device - exact| / bound, largest |exact|)"""
    assert row.shape == (len(pos),) and row.dtype == np.float64, (what, row.shape, row.dtype)
    T = ref.terms(X, phase, weight, pos, tables)
    want = ref.traces(X, phase, weight, pos, tables)
    worst = 0.0
    for e in range(len(pos)):
        b = ref.bound(T[e])
        err = abs(row[e] - want[e])
        print('%s lead %d at %s: device %r exact %r |diff| %.3g bound %.3g' % (what, e, tuple(pos[e]), row[e], want[e], err, b))
        assert np.isfinite(row[e]) and err <= b, '%s lead %d at %s: device %r exact %r bound %g' % (what, e, tuple(pos[e]), row[e], want[e], b)
        if b > 0:
            worst = max(worst, err / b)
    return worst, float(np.abs(want).max())


def raw_stepper(gpu_lib, H, W, phase=None, flags=None, dt=0.1, seed=0):
    """a Fenton handle with a wavefront on the grid in V and the gates anywhere in (0, 1)"""
    st = gpu_lib.Stepper(gpu_lib.FENTON4V, H, W, dt, 1.3, flags=gpu_lib.FAST if flags is None else flags)
    if phase is not None:
        st.set_phase(phase)
    rng = np.random.default_rng(seed)
    state = rng.uniform(0.1, 0.9, (4, H, W)).astype(np.float32)
    state[0] = front(H, W, seed) * np.float32(0.8) + np.float32(0.1)
    st.set_state(-1, state)
    return st


def one_sample(st, pos, tables, weight, var=0):
    st.leads_begin(pos, tables, weight, var, 1, 1)
    st.step(1)
    assert st.leads_count() == 1
    row = st.leads_read()[0]
    X = st.get_state(var).copy()
    st.leads_end()
    return row, X


@pytest.mark.parametrize('with_phase', [False, True], ids=['nophase', 'hole'])
@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: '%dx%d' % s)
def test_terms_equal_the_restatement(gpu_lib, shape, with_phase):
    """E = 1 and E = 64 over 4 tables; the weight plane absent, the phase field, and an explicit plane"""
    H, W = shape
    phase = hole(H, W) if with_phase else None
    st = raw_stepper(gpu_lib, H, W, phase, seed=H * W)
    tabs = tables_for(H, W)
    explicit = np.random.default_rng(3).uniform(-1, 1, (H, W)).astype(np.float32)
    explicit[np.random.default_rng(4).uniform(size=(H, W)) < 0.2] = 0
    worst = signal = 0.0
    for n, nt in ((1, 1), (64, 4)):
        pos = positions(H, W, n, nt)
        if n == 1:
            pos = [(H // 2, W // 2, 0)]
        for wname, weight in (('none', None), ('phase', phase), ('explicit', explicit)):
            if wname == 'phase' and phase is None:
                continue
            row, X = one_sample(st, pos, tabs[:nt], weight)
            w, s = compare(row, X, phase, weight, pos, tabs[:nt], '%dx%d E=%d weight %s' % (H, W, n, wname))
            worst, signal = max(worst, w), max(signal, s)
    # a front is on the grid: the reference trace is not identically zero (3 x 3 has one interior cell, every tap of which clamps
    # onto it: there the source is zero whatever the state, and the device must say exactly that)
    assert signal > 0 or shape == (3, 3)
    print('%dx%d phase %s: largest |device - exact| / bound %.3g, largest |trace| %.3g' % (H, W, with_phase, worst, signal))
    st.close()


def test_refusals(gpu_lib):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W)
    tabs = tables_for(H, W)
    ok = [(1, 1, 0)]
    with pytest.raises(gpu_lib.FibhipError, match=r'1 \.\. 64 leads \(got 65\)'):
        st.leads_begin([(1, 1, 0)] * 65, tabs, None, 0, 1, 1)
    with pytest.raises(gpu_lib.FibhipError, match=r'1 \.\. 4 lead-field tables \(got 5\)'):
        st.leads_begin(ok, np.concatenate([tabs, tabs[:1]]), None, 0, 1, 1)
    with pytest.raises(gpu_lib.FibhipError, match=r'lead 1: cell \(37, 0\) is outside the 37 x 53 grid'):
        st.leads_begin([(0, 0, 0), (37, 0, 0)], tabs, None, 0, 1, 1)
    with pytest.raises(gpu_lib.FibhipError, match='lead 0: table 2 of 2'):
        st.leads_begin([(0, 0, 2)], tabs[:2], None, 0, 1, 1)
    bad = tabs.copy()
    bad[1, 5, 6] = np.nan
    with pytest.raises(gpu_lib.FibhipError, match=r'table 1 has a value that is not finite \(row 5, column 6\)'):
        st.leads_begin(ok, bad, None, 0, 1, 1)
    w = np.ones((H, W), np.float32)
    w[7, 8] = np.inf
    with pytest.raises(gpu_lib.FibhipError, match=r'weight plane has a value that is not finite \(row 7, column 8\)'):
        st.leads_begin(ok, tabs, w, 0, 1, 1)
    with pytest.raises(gpu_lib.FibhipError, match='bad var 4'):
        st.leads_begin(ok, tabs, None, 4, 1, 1)
    with pytest.raises(gpu_lib.FibhipError, match='every must be >= 1'):
        st.leads_begin(ok, tabs, None, 0, 0, 1)
    with pytest.raises(gpu_lib.FibhipError, match='bad capacity 0'):
        st.leads_begin(ok, tabs, None, 0, 1, 0)
    with pytest.raises(gpu_lib.FibhipError, match='no recorder attached'):
        st.leads_count()
    with pytest.raises(gpu_lib.FibhipError, match='no recorder attached'):
        st.leads_read(0, 0)
    st.leads_end()                                            # (no recorder attached: nothing)
    st.step_edges()
    with pytest.raises(gpu_lib.FibhipError, match='leads_begin inside an open tick'):
        st.leads_begin(ok, tabs, None, 0, 1, 1)
    st.step_interior()
    st.step_commit()
    st.close()
    zp = gpu_lib.Stepper(gpu_lib.FENTON4V, H, W, 0.1, 1.3, flags=gpu_lib.FAST | gpu_lib.ZEROPAD)
    with pytest.raises(gpu_lib.FibhipError, match='zero-padded Laplacian'):
        zp.leads_begin(ok, tabs, None, 0, 1, 1)
    zp.close()
    shard = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    with pytest.raises(gpu_lib.FibhipError, match='not on a row block'):
        shard.leads_begin(ok, tables_for(42, 40), None, 0, 1, 1)
    shard.close()


def test_nan_in_one_cell_makes_every_lead_nan(gpu_lib):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W, hole(H, W))
    tabs = tables_for(H, W)
    pos = positions(H, W, 64, 4)
    clean = st.get_state(-1).copy()
    x = clean.copy()
    x[0, 20, 30] = np.nan
    st.set_state(-1, x)
    row, X = one_sample(st, pos, tabs, hole(H, W))
    assert np.isnan(X[20, 30]) and np.all(np.isnan(row)), row
    st.set_state(-1, clean)                                   # nothing else is harmed: the next recorder, on a clean state
    row, X = one_sample(st, pos, tabs, hole(H, W))
    compare(row, X, hole(H, W), hole(H, W), pos, tabs, 'after the NaN')
    st.close()


def test_source_does_not_depend_on_the_policy(gpu_lib):
    """the same state under the exact and the fast policy gives the same bytes: the source is always the exact form.  A tick of
    1e-30 ms moves no cell of a state that stays clear of zero, so both handles hold the state set_state gave them, boundary
    enforced, when the sample is taken"""
    H, W = 37, 53
    phase = hole(H, W)
    tabs = tables_for(H, W)
    pos = positions(H, W, 64, 4)
    rows, states = [], []
    for flags in (0, gpu_lib.FAST):
        st = raw_stepper(gpu_lib, H, W, phase, flags=flags, dt=1e-30, seed=9)
        row, X = one_sample(st, pos, tabs, phase)
        compare(row, X, phase, phase, pos, tabs, 'policy flags %d' % flags)
        rows.append(row)
        states.append(X)
        st.close()
    assert states[0].tobytes() == states[1].tobytes() and len(np.unique(states[0])) > 100
    assert rows[0].tobytes() == rows[1].tobytes()


# ---- invariance: the same run under other launch plans, strides and lead lists -----------------------------------------------
@contextlib.contextmanager
def plan_env(env):
    saved = {k: os.environ.get(k) for k in PLAN_ENV}
    try:
        for k in PLAN_ENV:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


PLAN_TICKS = 70
PLAN_POS = positions(96, 100, 64, 4)


def plan_run(env, every=1, pos=None):
    """Fenton 96 x 100, a wave under way, PLAN_TICKS single-tick calls -> (the trace, the final state, multi-tick ticks)"""
    pos = PLAN_POS if pos is None else pos
    with plan_env(env), warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        m = fenton(96, 100)
        st = m._stepper
        wave(m, 'fenton')
        weight = np.random.default_rng(4).uniform(0.1, 1, (96, 100)).astype(np.float32)
        s0 = st.launch_stats()
        st.leads_begin(pos, tables_for(96, 100), weight, 0, every, PLAN_TICKS // every)
        for _ in range(PLAN_TICKS):
            st.step(1)
        assert st.leads_count() == PLAN_TICKS // every
        rows = st.leads_read()
        state = st.get_state(-1).tobytes()
        assert st.fallbacks() == (0, 0)
        mt = st.launch_stats()['mt_ticks'] - s0['mt_ticks']
        st.close()
    return rows, state, mt


@pytest.fixture(scope='module')
def base_run(gpu_lib):
    rows, state, mt = plan_run({'FIBHIP_VARIANT': VARIANT_96x100}, 10)
    assert mt == PLAN_TICKS                                   # (between two samples the handle keeps its multi-tick launches)
    assert rows.shape == (7, 64) and all(len(np.unique(rows[:, e])) == 7 for e in range(64))
    return rows, state


@pytest.mark.parametrize('env', [{'FIBHIP_VARIANT': VARIANT_96x100, 'FIBHIP_MT': '0'}, {}, {'FIBHIP_VARIANT': '1,64,4,256'}],
                         ids=['one-launch-per-tick', 'unforced', 'flat-tiles'])
def test_trace_does_not_depend_on_the_launch_plan(gpu_lib, base_run, env):
    rows, state, mt = plan_run(env, 10)
    assert state == base_run[1]
    assert rows.tobytes() == base_run[0].tobytes(), env
    if env.get('FIBHIP_MT') == '0':
        assert mt == 0


@pytest.mark.parametrize('every', [1, 7])
def test_trace_does_not_depend_on_the_stride(gpu_lib, base_run, every):
    """every in {1, 7, 10}: the samples the strides share are the same bytes"""
    rows, state, _ = plan_run({'FIBHIP_VARIANT': VARIANT_96x100}, every)
    assert state == base_run[1] and rows.shape == (PLAN_TICKS // every, 64)
    ticks = ref.sample_ticks(PLAN_TICKS, every)
    shared = [k for k in ref.sample_ticks(PLAN_TICKS, 10) if k in ticks]
    assert shared == ([9, 19, 29, 39, 49, 59, 69] if every == 1 else [69])
    for k in shared:
        assert rows[ticks.index(k)].tobytes() == base_run[0][ref.sample_ticks(PLAN_TICKS, 10).index(k)].tobytes(), (every, k)


def test_trace_does_not_depend_on_the_lead_list(gpu_lib, base_run):
    """the list permuted: the columns permuted.  One lead alone: its column among the 64"""
    perm = np.random.default_rng(8).permutation(64)
    rows, _, _ = plan_run({'FIBHIP_VARIANT': VARIANT_96x100}, 10, [PLAN_POS[i] for i in perm])
    for j, i in enumerate(perm):
        assert rows[:, j].tobytes() == base_run[0][:, i].tobytes(), (j, i)
    for i in (0, 37, 63):
        rows, _, _ = plan_run({'FIBHIP_VARIANT': VARIANT_96x100}, 10, [PLAN_POS[i]])
        assert rows.shape == (7, 1) and rows[:, 0].tobytes() == base_run[0][:, i].tobytes(), i


# ---- the models ------------------------------------------------------------------------------------------------------------
def hole_model(kind, H, W):
    cfg = {'height': H, 'width': W, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 0.809, 'duration': 1000}
    if kind.startswith('fenton'):
        from fib_tf_amd.fenton import Fenton4v
        m = Fenton4v(dict(cfg, diff=1.5, fast_math=kind == 'fenton-fast'))
    elif kind == 'br':
        from fib_tf_amd.br import BeelerReuter
        m = BeelerReuter(dict(cfg, cheby=True, skip=False))
    elif kind == 'court':
        from fib_tf_amd.court import Courtemanche
        m = Courtemanche(cfg)
    else:
        from traced_cases import make_model
        m = make_model('ap', H, W)
        m.duration = 1000
    m.add_hole_to_phase_field(W // 2 + 3, H // 2 - 2, 6)
    m.define()
    if kind == 'traced':
        m._ensure_compiled()
    return m


@pytest.mark.parametrize('kind', ['fenton-fast', 'fenton-exact', 'br', 'court', 'traced'])
def test_models_through_record_leads(gpu_lib, kind):
    """IonicModel.record_leads on every model, a phase field with a hole as the default weight: raw() against the restatement on
    the state polled at every sample tick; Courtemanche with a 'slow' between two samples; traces, bipolar and times_ms"""
    from fib_tf_amd import leads
    H, W = 37, 53
    m = hole_model(kind, H, W)
    wave(m, kind.split('-')[0])
    st = m._stepper
    tab = leads.point_table(H, W, 2.0)
    cells = [(H // 2, 10), (H // 2, 14), (0, 0), (H - 1, W - 1)]
    pos = [(r, c, 0) for r, c in cells]
    with m.record_leads(cells, tables=tab, every=3, capacity=4) as rec:
        assert rec.capacity == 4 and np.array_equal(rec.weight, m.phase) and rec.scale == float(m.diff)
        states = []
        for i in range(12):
            if kind == 'court' and i == 4:
                m.fire_op('slow')
            st.step(1)
            if (i + 1) % 3 == 0:
                states.append(st.get_state(0).copy())
        assert rec.count() == 4
        raw = rec.raw()
        assert raw.shape == (4, 4) and raw.dtype == np.float64
        signal = 0.0
        for s, X in enumerate(states):
            signal = max(signal, compare(raw[s], X, m.phase, m.phase, pos, tab, '%s sample %d' % (kind, s))[1])
        assert signal > 0 and len(np.unique(raw[:, 0])) > 1
        assert np.array_equal(rec.traces(), raw * np.float64(m.diff)) and np.array_equal(rec.traces(scale=1.0), raw)
        bip = rec.bipolar([(0, 1), (3, 2)])
        assert np.array_equal(bip, np.stack([rec.traces()[:, 0] - rec.traces()[:, 1], rec.traces()[:, 3] - rec.traces()[:, 2]], 1))
        assert np.allclose(rec.times_ms(), (1 + np.arange(4)) * 3 * m.dt_per_step * m.dt)
        with pytest.raises(ValueError, match='outside 0 .. 3'):
            rec.bipolar([(0, 4)])
    # weight=None: the plain Laplacian with the phase term; an explicit plane
    plane = np.random.default_rng(2).uniform(0, 1, (H, W)).astype(np.float32)
    for weight in (None, plane):
        with m.record_leads(cells, tables=tab, weight=weight, capacity=1) as rec:
            st.step(1)
            compare(rec.raw()[0], st.get_state(0), m.phase, weight, pos, tab, '%s weight %s' % (kind, 'None' if weight is None else 'plane'))
    with pytest.raises(AssertionError, match='has been closed'):
        rec.raw()
    st.close()


def test_court_slow_array_is_sampled_before_slow(gpu_lib):
    """a lead on an array Courtemanche's 'slow' assigns, 'slow' fired right behind a sample tick: the sample sees the array as the
    tick left it (the recorder's before_slow)"""
    from fib_tf_amd import leads
    H, W = 37, 53
    m = hole_model('court', H, W)
    wave(m, 'court')
    st = m._stepper
    slow = type(m).tip_signals[1]
    tab = leads.point_table(H, W, 1.0)
    cells = [(H // 2, W // 2), (3, 4)]
    with m.record_leads(cells, tables=tab, every=2, var=slow, capacity=3) as rec:
        polled = []
        for i in range(6):
            st.step(1)
            if i % 2 == 1:
                polled.append(st.get_state(slow).copy())
                m.fire_op('slow')                              # belongs to the next tick
        raw = rec.raw()
    for s, X in enumerate(polled):
        compare(raw[s], X, m.phase, m.phase, [(r, c, 0) for r, c in cells], tab, 'slow array sample %d' % s)
    st.close()


# ---- capacity, read ranges, attach and detach --------------------------------------------------------------------------------
def test_capacity_count_and_read_ranges(gpu_lib):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W)
    tabs = tables_for(H, W)
    pos = positions(H, W, 5, 4)
    st.leads_begin(pos, tabs, None, 0, 2, 3)
    assert st.leads_count() == 0 and st.leads_read().shape == (0, 5)
    states = []
    for i in range(6):
        st.step(1)
        if i % 2 == 1:
            states.append(st.get_state(0).copy())
    assert st.leads_count() == 3
    full = st.leads_read()
    for s in range(3):
        compare(full[s], states[s], None, None, pos, tabs, 'sample %d' % s)
    assert st.leads_read(1, 2).tobytes() == full[1:].tobytes() and st.leads_read(2, 1).tobytes() == full[2:].tobytes()
    assert st.leads_read(3, 0).shape == (0, 5)
    with pytest.raises(gpu_lib.FibhipError, match=r'samples \[2, 4\) of 3 taken'):
        st.leads_read(2, 2)
    with pytest.raises(gpu_lib.FibhipError, match='of 3 taken'):
        st.leads_read(-1, 1)
    st.step(1)                                                # tick 7: no sample
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(1)                                            # tick 8 would take sample number 3
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(5)
    assert st.leads_count() == 3 and st.leads_read().tobytes() == full.tobytes()
    st.leads_end()
    st.step(3)                                                # detached: nothing holds the handle back
    st.close()


def test_detach_reattach_and_beside_another_recorder(gpu_lib):
    H, W = 64, 64
    st = raw_stepper(gpu_lib, H, W, hole(H, W))
    tabs = tables_for(H, W)
    pos = positions(H, W, 9, 4)
    weight, mask = hole(H, W), (hole(H, W) > 0.5).astype(np.uint8)
    st.stats_begin([(0, 'sum', 0.0), (0, 'max', 0.0)], weight, mask, 3, 8)       # another recorder is on already
    st.step(2)
    st.leads_begin(pos, tabs, weight, 0, 2, 4)                # tick 0 of the lead recorder is the handle's third
    states = []
    for i in range(4):
        st.step(1)
        if i % 2 == 1:
            states.append(st.get_state(0).copy())
    first = st.leads_read()
    for s in range(2):
        compare(first[s], states[s], weight, weight, pos, tabs, 'beside the statistics recorder, sample %d' % s)
    assert st.stats_count() == 2
    st.leads_end()
    st.leads_end()                                            # (twice: nothing)
    st.step(1)
    st.leads_begin(pos[:3], tabs, None, 0, 1, 2)              # re-attach: other leads, a stride of its own
    assert st.leads_count() == 0
    st.step(1)
    X = st.get_state(0).copy()
    again = st.leads_read()
    assert again.shape == (1, 3)
    compare(again[0], X, weight, None, pos[:3], tabs, 're-attached')
    st.leads_begin(pos, tabs, weight, 0, 1, 1)                # begin over an attached recorder: the old one goes
    st.step(1)
    compare(st.leads_read()[0], st.get_state(0), weight, weight, pos, tabs, 'begun over')
    assert st.stats_count() == 3
    st.close()                                                # (destroy frees an attached recorder)


def test_timeline_lists_the_sample(gpu_lib):
    H, W = 130, 67
    st = raw_stepper(gpu_lib, H, W)
    st.leads_begin(positions(H, W, 3, 1), tables_for(H, W, 1), None, 0, 2, 4)
    st.step(1)
    st.trace_begin()
    st.step(1)
    names = [e['name'].split('<')[0] for e in st.trace_end()]
    assert names[-2:] == ['lead_kernel', 'lead_combine_kernel'], names
    st.trace_begin()
    st.step(1)
    assert not any('lead' in e['name'] for e in st.trace_end())
    st.close()


def test_example_runs_headless(gpu_lib, tmp_path):
    """examples/run_unipolar.py end to end at a tiny size, in this process: four unipolar and three bipolar traces, a PNG"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('run_unipolar_under_test', os.path.join(root, 'examples', 'run_unipolar.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = tmp_path / 'unipolar.png'
    uni, bip = ex.main(['--size', '64', '--ms', '30', '--every', '5', '--out', str(out)])
    assert uni.shape == (6, 4) and bip.shape == (6, 3) and np.all(np.isfinite(uni)) and np.any(uni != 0)
    assert np.array_equal(bip[:, 1], uni[:, 1] - uni[:, 2])
    assert out.read_bytes()[:8] == b'\x89PNG\r\n\x1a\n'
