"""-m gpu: the potential-map recorder (include/fibhip.h fibhip_pmap_*, fib_tf_amd/potential.py) on the device.

Every sample is compared with the NumPy restatement (tests/potential_ref.py) on the state read back at the sample's tick, BIT FOR
BIT: the order of summation is part of the definition (a function of the radius alone), the products are exact and the device's
fused multiply-add rounds what multiply-then-add rounds.  tests/test_potential_cpu.py shows that these planes can see the order.
The grids are the smallest that reach every path of pmap_conv_kernel: 5 x 3 and 4 x 64 (less than a tile either way), 37 x 53
(odd everything, three tile rows of sites) and 70 x 130 (more than one 64 x 16 tile of sites both ways; at R = 32 with the step
(7, 9) the span of a tile is staged in several slabs and the rows are de-interleaved by the column step)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lead_ref  # noqa: E402
import potential_ref as ref  # noqa: E402
from test_gpu_frames import VARIANT_96x100, wave  # noqa: E402
from test_gpu_leads import hole_model, plan_env, raw_stepper  # noqa: E402
from test_gpu_tips import br, fenton  # noqa: E402
from test_leads_cpu import hole  # noqa: E402
from test_potential_cpu import table_for  # noqa: E402

pytestmark = pytest.mark.gpu

# (grid, radius, window, step)
CASES = [((5, 3), 1, None, (1, 1)), ((4, 64), 2, None, (1, 1)), ((37, 53), 1, None, (1, 1)), ((37, 53), 2, None, (1, 1)),
         ((37, 53), 5, None, (1, 1)), ((70, 130), 32, (2, 69, 1, 128), (7, 9)), ((70, 130), 3, None, (1, 1))]
CASE_IDS = ['%dx%d-R%d-step%dx%d' % (g + (r,) + s) for g, r, _, s in CASES]


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = got.view(np.uint64) != want.view(np.uint64) if got.dtype == np.float64 else got != want
    assert got.tobytes() == want.tobytes(), '%s: %d of %d values differ, first at %s' % (what, int(diff.sum()), got.size, np.argwhere(diff)[:1].tolist())


def check(st, phase, table, weight, window, step, var=0, ticks=4, what=''):
    """a sample behind every one of `ticks` ticks: the cube against the restatement on the state polled at each tick, the
    summary of all samples and of a window of them against the restated summary of the device's cube"""
    H, W = st.height, st.width
    st.pmap_begin(table, weight, window, step, var, 1, ticks)
    states = []
    for _ in range(ticks):
        st.step(1)
        states.append(st.get_state(var).copy())
    assert st.pmap_count() == ticks
    cube = st.pmap_read()
    rows, cols = ref.lattice(H, W, window, step)
    assert cube.shape == (ticks, len(rows), len(cols)) and cube.dtype == np.float64
    for s, X in enumerate(states):
        same(cube[s], ref.maps(ref.source_plane(X, phase, weight), table, window, step), '%s sample %d' % (what, s))
    for first, count in ((0, ticks), (1, 2)):
        got = st.pmap_summary(first, count)
        for name, g, w in zip(('vmin', 'vmax', 'dmin', 'kmin', 'kmax', 'kd'), got, ref.summary(cube, first, count)):
            same(g, w, '%s summary [%d, %d) %s' % (what, first, first + count, name))
    st.pmap_end()
    return cube


@pytest.mark.parametrize('grid,R,window,step', CASES, ids=CASE_IDS)
def test_fenton_with_the_obstacle_field(gpu_lib, grid, R, window, step):
    """Fenton, a phase field with a hole: the field as the weight (record_potential_map's default), no weight, a random plane"""
    H, W = grid
    phase = hole(H, W)
    st = raw_stepper(gpu_lib, H, W, phase, seed=H * W)
    plane = np.random.default_rng(3).uniform(-1, 1, (H, W)).astype(np.float32)
    signal = 0.0
    for wname, weight in (('phase', phase), ('none', None), ('plane', plane)):
        cube = check(st, phase, table_for(R), weight, window, step, what='%s weight %s' % (CASE_IDS[CASES.index((grid, R, window, step))], wname))
        assert np.all(np.isfinite(cube))
        signal = max(signal, float(np.abs(cube).max()))
    assert signal > 0
    st.close()


@pytest.mark.parametrize('grid,R,window,step', CASES[2:], ids=CASE_IDS[2:])
def test_beeler_reuter_without_a_field(gpu_lib, grid, R, window, step):
    H, W = grid
    m = br(H, W)
    wave(m, 'br')
    st = m._stepper
    assert getattr(m, 'phase', None) is None
    plane = np.random.default_rng(5).uniform(-1, 1, (H, W)).astype(np.float32)
    for weight in (None, plane):
        cube = check(st, None, table_for(R, 2), weight, window, step, ticks=3, what='br')
        assert np.all(np.isfinite(cube)) and np.any(cube != 0)
    st.close()


# ---- the same state gives the same bytes ---------------------------------------------------------------------------------------
PLAN_TICKS = 70
PLAN_LATTICE = ((3, 90, 2, 100), (2, 3))


def plan_run(env, every=10):
    """Fenton 96 x 100, a wave under way, PLAN_TICKS single-tick calls -> (cube, summary bytes, final state, multi-tick ticks)"""
    with plan_env(env), warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        m = fenton(96, 100)
        st = m._stepper
        wave(m, 'fenton')
        weight = np.random.default_rng(4).uniform(0.1, 1, (96, 100)).astype(np.float32)
        s0 = st.launch_stats()
        st.pmap_begin(table_for(5), weight, PLAN_LATTICE[0], PLAN_LATTICE[1], 0, every, PLAN_TICKS // every)
        for _ in range(PLAN_TICKS):
            st.step(1)
        assert st.pmap_count() == PLAN_TICKS // every
        cube = st.pmap_read()
        summary = b''.join(a.tobytes() for a in st.pmap_summary())
        state = st.get_state(-1).tobytes()
        assert st.fallbacks() == (0, 0)
        mt = st.launch_stats()['mt_ticks'] - s0['mt_ticks']
        st.close()
    return cube, summary, state, mt


@pytest.fixture(scope='module')
def base_run(gpu_lib):
    cube, summary, state, mt = plan_run({'FIBHIP_VARIANT': VARIANT_96x100}, 10)
    assert mt == PLAN_TICKS                                   # (between two samples the handle keeps its multi-tick launches)
    assert cube.shape == (7, 44, 33) and all(np.any(cube[s] != cube[s + 1]) for s in range(6))
    return cube, summary, state


@pytest.mark.parametrize('env', [{'FIBHIP_VARIANT': VARIANT_96x100, 'FIBHIP_MT': '0'}, {}, {'FIBHIP_VARIANT': '1,64,4,256'}],
                         ids=['one-launch-per-tick', 'unforced', 'flat-tiles'])
def test_cube_does_not_depend_on_the_launch_plan(gpu_lib, base_run, env):
    cube, summary, state, mt = plan_run(env, 10)
    assert state == base_run[2]
    assert cube.tobytes() == base_run[0].tobytes() and summary == base_run[1], env
    if env.get('FIBHIP_MT') == '0':
        assert mt == 0


@pytest.mark.parametrize('every', [1, 7])
def test_cube_does_not_depend_on_the_stride(gpu_lib, base_run, every):
    """every in {1, 7, 10}: the samples the strides share are the same bytes"""
    cube, _, state, _ = plan_run({'FIBHIP_VARIANT': VARIANT_96x100}, every)
    assert state == base_run[2] and cube.shape == (PLAN_TICKS // every, 44, 33)
    ticks = lead_ref.sample_ticks(PLAN_TICKS, every)
    shared = [k for k in lead_ref.sample_ticks(PLAN_TICKS, 10) if k in ticks]
    assert shared == ([9, 19, 29, 39, 49, 59, 69] if every == 1 else [69])
    for k in shared:
        assert cube[ticks.index(k)].tobytes() == base_run[0][lead_ref.sample_ticks(PLAN_TICKS, 10).index(k)].tobytes(), (every, k)


def one_sample(st, table, weight, window=None, step=(1, 1), var=0):
    st.pmap_begin(table, weight, window, step, var, 1, 1)
    st.step(1)
    assert st.pmap_count() == 1
    plane = st.pmap_read()[0]
    X = st.get_state(var).copy()
    st.pmap_end()
    return plane, X


def test_source_does_not_depend_on_the_policy(gpu_lib):
    """the same state under the exact and the fast policy gives the same bytes: the source is always the exact form.  A tick of
    1e-30 ms moves no cell of a state that stays clear of zero (tests/test_gpu_leads.py)"""
    H, W = 37, 53
    phase = hole(H, W)
    planes, states = [], []
    for flags in (0, gpu_lib.FAST):
        st = raw_stepper(gpu_lib, H, W, phase, flags=flags, dt=1e-30, seed=9)
        plane, X = one_sample(st, table_for(5), phase)
        same(plane, ref.maps(ref.source_plane(X, phase, phase), table_for(5)), 'policy flags %d' % flags)
        planes.append(plane)
        states.append(X)
        st.close()
    assert states[0].tobytes() == states[1].tobytes() and len(np.unique(states[0])) > 100
    assert planes[0].tobytes() == planes[1].tobytes()


def test_sub_lattice_equals_the_sites_of_the_full_lattice(gpu_lib):
    H, W = 70, 130
    phase = hole(H, W)
    st = raw_stepper(gpu_lib, H, W, phase, seed=2)
    start = st.get_state(-1).copy()
    T = table_for(6)
    full, X = one_sample(st, T, phase)
    for window, step in (((2, 69, 1, 128), (7, 9)), ((0, 70, 0, 130), (16, 16)), ((5, 6, 7, 130), (1, 2)), ((60, 70, 120, 130), (3, 1))):
        st.set_state(-1, start)
        sub, X2 = one_sample(st, T, phase, window, step)
        assert X2.tobytes() == X.tobytes()
        rows, cols = ref.lattice(H, W, window, step)
        same(sub, np.ascontiguousarray(full[np.ix_(rows, cols)]), 'window %s step %s' % (window, step))
    st.close()


def test_one_nan_cell_reaches_the_sites_within_r_plus_one_and_no_others(gpu_lib):
    """a NaN planted in one cell spreads through the tick's own sub-steps; of the cells that are NaN when the sample is taken,
    each one makes exactly the sites within Chebyshev distance R + 1 of it NaN — R of the table, one of the stencil — and no
    others: the sites that are NaN are the union of those squares, and nothing else of the map is touched"""
    H, W, R = 37, 53, 2
    st = raw_stepper(gpu_lib, H, W, seed=4)
    clean = st.get_state(-1).copy()
    T = table_for(R)
    good, _ = one_sample(st, T, None)
    x = clean.copy()
    x[0, 18, 26] = np.nan
    st.set_state(-1, x)
    plane, X = one_sample(st, T, None)
    bad = np.isnan(X)
    rr, cc = np.nonzero(bad)
    assert bad[18, 26] and 1 <= len(rr) < H * W // 4
    assert rr.min() > R + 2 and rr.max() < H - R - 3 and cc.min() > R + 2 and cc.max() < W - R - 3      # (clear of the boundary clamp)
    want = np.zeros((H, W), bool)
    for r, c in zip(rr, cc):
        want[r - R - 1:r + R + 2, c - R - 1:c + R + 2] = True
    assert np.array_equal(np.isnan(plane), want) and not want.all()
    same(plane, ref.maps(ref.source_plane(X, None, None), T), 'with the NaN')
    assert np.all(np.isfinite(good))
    st.close()


def test_against_the_lead_recorder(gpu_lib):
    """33 x 30, R = 32 and the full point table: every site's window covers every cell, so a site and a lead at the same cell sum
    the same terms in two orders; both recorders attached to one handle, a 3 x 3 lattice, each site within twice the derived
    bound of its lead"""
    from fib_tf_amd import leads, potential
    H, W, R = 33, 30, 32
    phase = hole(H, W)
    st = raw_stepper(gpu_lib, H, W, phase, seed=6)
    T = potential.truncated_table(R, 2.0)
    window, step = (2, 33, 1, 30), (12, 12)
    rows, cols = ref.lattice(H, W, window, step)
    assert len(rows) == len(cols) == 3
    pos = [(int(r), int(c), 0) for r in rows for c in cols]
    st.leads_begin(pos, leads.point_table(H, W, 2.0)[np.newaxis], phase, 0, 1, 2)
    st.pmap_begin(T, phase, window, step, 0, 1, 2)
    st.step(1)
    st.step(1)
    X = st.get_state(0).copy()
    lead, site = st.leads_read()[1], st.pmap_read()[1]
    q = ref.source_plane(X, phase, phase)
    same(site, ref.maps(q, T, window, step), 'beside the lead recorder')
    for e, (r, c, _) in enumerate(pos):
        b = ref.bound(ref.terms(q, T, r, c), R)
        assert lead[e] != 0 and abs(site[e // 3, e % 3] - lead[e]) <= 2 * b, (r, c, site[e // 3, e % 3], lead[e], b)
    st.close()


# ---- through the model: lesions, Courtemanche's slow arrays, the derived maps ---------------------------------------------------
def test_with_a_lesion_program(gpu_lib):
    """a sample every 4 ticks, a lesion after tick 7 — the tick of sample 1: that sample sees the OLD field (the lesion row
    stands behind every sampler), the next one the NEW field; the weight plane handed over at attach stays what it was"""
    import lesion_ref
    from fib_tf_amd import lesions
    H, W = 37, 53
    m = hole_model('fenton-fast', H, W)
    wave(m, 'fenton')
    st = m._stepper
    old = m.phase.copy()
    site = ('disc', 20, 12, 4)
    new = lesion_ref.apply_sites(old, H, W, [site])
    T = table_for(4)
    with m.record_potential_map(T, every=4, step=(2, 2), max_samples=3) as rec:
        st.lesion_begin(lesions.compile_program(m, [lesions.Lesion(site, at_tick=7)]))
        states = []
        for i in range(12):
            st.step(1)
            if i % 4 == 3:
                states.append(st.get_state(0).copy())
        assert st.get_phase().tobytes() == new.tobytes() and new.tobytes() != old.tobytes()
        raw = rec.raw()
        for s, field in enumerate((old, old, new)):
            same(raw[s], ref.maps(ref.source_plane(states[s], field, old), T, None, (2, 2)), 'sample %d' % s)
        other = ref.maps(ref.source_plane(states[2], old, old), T, None, (2, 2))
        assert other.tobytes() != raw[2].tobytes()            # (the test can tell the fields apart)
        # the derived maps
        s = rec.summary()
        for name, w in zip(('vmin', 'vmax', 'dmin', 'kmin', 'kmax', 'kd'), ref.summary(raw)):
            same(s[name], w, name)
        assert np.array_equal(rec.voltage(), (s['vmax'] - s['vmin']) * m.diff) and np.array_equal(rec.maps(), raw * np.float64(m.diff))
        assert np.array_equal(rec.lat_ms(), (s['kd'] + 0.5) * 4 * m.dt_per_step * m.dt)
        assert np.array_equal(rec.bipolar(1, scale=1.0), raw[:, :, 1:] - raw[:, :, :-1])
        assert np.allclose(rec.times_ms(), (1 + np.arange(3)) * 4 * m.dt_per_step * m.dt)
        rows, cols = rec.sites()
        assert rows.tolist() == list(range(0, H, 2)) and cols.tolist() == list(range(0, W, 2)) and raw.shape == (3, len(rows), len(cols))
        assert np.array_equal(rec.weight, old) and rec.radius == 4
    with pytest.raises(AssertionError, match='has been closed'):
        rec.raw()
    st.close()


def test_court_slow_array_is_sampled_before_slow(gpu_lib):
    """a map of an array Courtemanche's 'slow' assigns, 'slow' fired right behind a sample tick: the sample sees the array as the
    tick left it (the recorder's before_slow)"""
    H, W = 20, 24
    from fib_tf_amd.court import Courtemanche
    m = Courtemanche({'height': H, 'width': W, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 0.809, 'duration': 1000})
    m.add_hole_to_phase_field(W // 2 + 3, H // 2 - 2, 4)
    m.define()
    wave(m, 'court')
    st = m._stepper
    slow = type(m).tip_signals[1]
    T = table_for(3)
    with m.record_potential_map(T, every=2, var=slow, max_samples=3) as rec:
        polled = []
        for i in range(6):
            st.step(1)
            if i % 2 == 1:
                polled.append(st.get_state(slow).copy())
                m.fire_op('slow')                              # belongs to the next tick
        raw = rec.raw()
    assert polled[0].tobytes() != polled[1].tobytes()
    for s, X in enumerate(polled):
        same(raw[s], ref.maps(ref.source_plane(X, m.phase, m.phase), T), 'slow array sample %d' % s)
    st.close()


# ---- capacity, read ranges, refusals ---------------------------------------------------------------------------------------------
def test_capacity_count_read_ranges_and_timeline(gpu_lib):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W)
    T = table_for(2)
    st.pmap_begin(T, None, (1, 30, 2, 50), (3, 5), 0, 2, 3)
    assert st.pmap_count() == 0 and st.pmap_read().shape == (0, 10, 10)
    st.step(1)
    st.trace_begin()
    st.step(1)
    names = [e['name'].split('<')[0] for e in st.trace_end()]
    assert names[-2:] == ['pmap_source_kernel', 'pmap_conv_kernel'], names
    st.trace_begin()
    st.step(1)
    assert not any('pmap' in e['name'] for e in st.trace_end())
    st.step(3)
    assert st.pmap_count() == 3
    full = st.pmap_read()
    assert st.pmap_read(1, 2).tobytes() == full[1:].tobytes() and st.pmap_read(3, 0).shape == (0, 10, 10)
    with pytest.raises(gpu_lib.FibhipError, match=r'samples \[2, 4\) of 3 taken'):
        st.pmap_read(2, 2)
    with pytest.raises(gpu_lib.FibhipError, match=r'pmap_summary: samples \[2, 4\) of 3 taken'):
        st.pmap_summary(2, 2)
    with pytest.raises(gpu_lib.FibhipError, match=r'at least 2 samples \(got 1\)'):
        st.pmap_summary(2, 1)
    st.step(1)                                                # tick 7: no sample
    with pytest.raises(gpu_lib.FibhipError, match='trace full .*potential map recorder holds 3 samples'):
        st.step(1)                                            # tick 8 would take sample number 3
    assert st.pmap_count() == 3 and st.pmap_read().tobytes() == full.tobytes()
    st.pmap_end()
    st.pmap_end()                                             # (twice: nothing)
    st.step(3)                                                # detached: nothing holds the handle back
    st.close()


def test_refusals(gpu_lib):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W)
    T = table_for(3)
    with pytest.raises(gpu_lib.FibhipError, match=r'radius must be 1 \.\. 32 \(got 33\)'):
        st.pmap_begin(np.ones((34, 34), np.float32))
    for step in ((0, 1), (1, 17)):
        with pytest.raises(gpu_lib.FibhipError, match=r'a step is 1 \.\. 16 cells each way \(got %d x %d\)' % step):
            st.pmap_begin(T, step=step)
    for window in ((5, 5, 0, W), (0, H + 1, 0, W), (0, H, 10, 9), (-1, H, 0, W)):
        with pytest.raises(gpu_lib.FibhipError, match='pmap_begin: the window rows .* is empty or outside the 37 x 53 grid'):
            st.pmap_begin(T, window=window)
    bad = T.copy()
    bad[1, 2] = np.nan
    with pytest.raises(gpu_lib.FibhipError, match=r'the table has a value that is not finite \(row 1, column 2\)'):
        st.pmap_begin(bad)
    w = np.ones((H, W), np.float32)
    w[7, 8] = np.inf
    with pytest.raises(gpu_lib.FibhipError, match=r'weight plane has a value that is not finite \(row 7, column 8\)'):
        st.pmap_begin(T, w)
    with pytest.raises(gpu_lib.FibhipError, match='bad var 4'):
        st.pmap_begin(T, var=4)
    with pytest.raises(gpu_lib.FibhipError, match='every must be >= 1'):
        st.pmap_begin(T, every=0)
    with pytest.raises(gpu_lib.FibhipError, match='bad capacity 0'):
        st.pmap_begin(T, capacity=0)
    with pytest.raises(gpu_lib.FibhipError, match='bad capacity'):
        st.pmap_begin(T, capacity=2 ** 62)                    # (more bytes than a size_t counts: refused before any allocation)
    for fn in (st.pmap_count, lambda: st.pmap_read(0, 0), lambda: st.pmap_summary(0, 2)):
        with pytest.raises(gpu_lib.FibhipError, match='no recorder attached'):
            fn()
    st.pmap_end()                                             # (no recorder attached: nothing)
    st.step_edges()
    with pytest.raises(gpu_lib.FibhipError, match='pmap_begin inside an open tick'):
        st.pmap_begin(T)
    st.step_interior()
    st.step_commit()
    st.close()
    zp = gpu_lib.Stepper(gpu_lib.FENTON4V, H, W, 0.1, 1.3, flags=gpu_lib.FAST | gpu_lib.ZEROPAD)
    with pytest.raises(gpu_lib.FibhipError, match='zero-padded Laplacian'):
        zp.pmap_begin(T)
    zp.close()
    shard = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    with pytest.raises(gpu_lib.FibhipError, match='not on a row block'):
        shard.pmap_begin(T)
    shard.close()


def test_example_runs_headless(gpu_lib, tmp_path):
    """examples/run_voltage_map.py end to end at a tiny size, in this process: the voltage maps before and after the lesion and
    the map of electrogram LAT minus first_up"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('run_voltage_map_under_test', os.path.join(root, 'examples', 'run_voltage_map.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = tmp_path / 'voltage_map.png'
    before, after, dlat = ex.main(['--size', '64', '--ms', '60', '--every', '5', '--radius', '6', '--step', '4', '--out', str(out)])
    assert before.shape == after.shape == dlat.shape == (16, 16) and np.all(np.isfinite(before)) and np.all(before >= 0) and np.any(before > 0)
    assert np.any(after != before)
    assert out.read_bytes()[:8] == b'\x89PNG\r\n\x1a\n'
