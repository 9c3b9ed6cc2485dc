"""-m gpu: the wave recorder (include/fibhip.h fibhip_waves_*, fib_tf_amd/waves.py) on the device.

Its definition is integer arithmetic on strict float32 compares, so counts, records (sorted by seed) and the whole label plane
must EQUAL the NumPy restatement (tests/wave_ref.py).  Crafted geometries go in through the mask with kind 'above' and level
-3e38: every finite cell passes the compare, the set plane is the mask whatever the dynamics do.  The grids are the smallest
that reach every path of the kernels: 3 x 3, 5 x 3 and 4 x 64 (one tile, no merge launch), 37 x 53 (three tile rows, ragged),
64 x 64 (tiles exactly full) and 130 x 67 (more than one tile both ways: tile corners, a last tile of two rows and three
columns).  On the dynamics the reference is computed from the state read back at every sample."""
import contextlib
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_ref as ref  # noqa: E402
from test_gpu_frames import PLAN_ENV, wave  # noqa: E402
from test_leads_cpu import front  # noqa: E402
from test_waves_cpu import TILE, checkerboard, crafted, random_plane  # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = [(3, 3), (4, 64), (5, 3), (37, 53), (64, 64), (130, 67)]
EVERYTHING = -3e38                                            # every finite float32 is above it
ROOMY = 8192                                                  # more records than any plane here has waves


def raw_stepper(gpu_lib, H, W, dt=0.1, seed=0, flags=None):
    """a Fenton handle with a wavefront on the grid in V and the gates anywhere in (0, 1)"""
    st = gpu_lib.Stepper(gpu_lib.FENTON4V, H, W, dt, 1.3, flags=gpu_lib.FAST if flags is None else flags)
    rng = np.random.default_rng(seed)
    state = rng.uniform(0.1, 0.9, (4, H, W)).astype(np.float32)
    state[0] = front(H, W, seed) * np.float32(0.8) + np.float32(0.1)
    st.set_state(-1, state)
    return st


def same_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in ref.FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, got[f][:8], want[f][:8])


def check_sample(counts, records, labels, s, conn, max_waves, what):
    """one device sample against the restatement of the set plane `s`; -> the reference's (counts, records)"""
    want_counts, want_rec, want_lab = ref.sample(s, conn, max_waves)
    print('%s: device counts %s reference %s' % (what, counts.tolist(), want_counts.tolist()))
    assert counts.dtype == np.int32 and counts.tolist() == want_counts.tolist(), (what, counts, want_counts)
    if labels is not None:
        assert labels.dtype == np.int32 and np.array_equal(labels, want_lab), (what, np.argwhere(labels != want_lab)[:8])
    got = ref.sorted_records(records, counts[1])
    if want_counts[0] <= max_waves:
        same_records(got, want_rec, what)
    else:
        # cut: WHICH waves are stored is unspecified — every stored one is whole and exact, none appears twice
        assert len(got) == max_waves and len(np.unique(got['seed'])) == max_waves, (what, got['seed'])
        at = np.searchsorted(want_rec['seed'], got['seed'])
        assert np.all(at < len(want_rec)) and np.array_equal(want_rec['seed'][at], got['seed']), (what, got['seed'])
        same_records(got, want_rec[at], what)
    return want_counts, want_rec


def crafted_sample(st, plane, conn, max_waves, what):
    st.waves_begin(0, 0, EVERYTHING, -1, 0, 0.0, conn, plane.astype(np.uint8), max_waves, 1, 1)
    st.step(1)
    assert st.waves_count() == 1
    counts, records = st.waves_read()
    labels = st.waves_labels()
    assert np.all(np.isfinite(st.get_state(0)))               # (so the set plane IS the mask)
    st.waves_end()
    return check_sample(counts[0], records[0], labels, plane, conn, max_waves, what)


@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: '%dx%d' % s)
def test_crafted_planes_equal_the_restatement(gpu_lib, shape):
    H, W = shape
    st = raw_stepper(gpu_lib, H, W, seed=H * W)
    planes = crafted(H, W)
    assert {'empty', 'full', 'single', 'serpentine', 'spiral', 'ring', 'checkerboard', 'random-1', 'random-2', 'random-3'} <= set(planes)
    if shape == (130, 67):
        assert len(planes) == 14                              # the tile-corner pairs and both straddling pairs fit
    for name, plane in planes.items():
        for conn in (4, 8):
            crafted_sample(st, plane, conn, ROOMY, '%dx%d %s conn %d' % (H, W, name, conn))
    st.close()


def test_tile_corner_pairs(gpu_lib):
    """only (15, 63) and (16, 64), the corner of four tiles: one wave under conn = 8, two under conn = 4; the anti-diagonal too"""
    H, W = 130, 67
    st = raw_stepper(gpu_lib, H, W)
    ty, tx = TILE
    for cells in ([(ty - 1, tx - 1), (ty, tx)], [(ty - 1, tx), (ty, tx - 1)]):
        plane = np.zeros((H, W), bool)
        for r, c in cells:
            plane[r, c] = True
        c4, r4 = crafted_sample(st, plane, 4, ROOMY, 'corner %s conn 4' % cells)
        c8, r8 = crafted_sample(st, plane, 8, ROOMY, 'corner %s conn 8' % cells)
        assert c4.tolist() == [2, 2, 2] and c8.tolist() == [1, 1, 2]
        assert r8['seed'][0] == min(r * W + c for r, c in cells) and r8['area'][0] == 2
    st.close()


@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: '%dx%d' % s)
def test_checkerboard_is_cut_at_max_waves(gpu_lib, shape):
    """conn = 4: every cell its own wave, far more than max_waves = 16 — n and cells exact, 16 whole records of distinct seeds, the
    label plane complete.  conn = 8: one wave through nothing but diagonals, across every tile corner"""
    H, W = shape
    st = raw_stepper(gpu_lib, H, W, seed=3)
    plane = checkerboard(H, W)
    counts, _ = crafted_sample(st, plane, 4, 16, '%dx%d checkerboard cut' % shape)
    n = (H * W + 1) // 2
    assert counts.tolist() == [n, min(n, 16), n]
    counts, rec = crafted_sample(st, plane, 8, 16, '%dx%d checkerboard conn 8' % shape)
    assert counts.tolist() == [1, 1, n] and rec['area'][0] == n
    st.close()


# ---- dynamics ------------------------------------------------------------------------------------------------------------
def fenton_hole(H, W, fast=True):
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': H, 'width': W, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 1000, 'fast_math': fast})
    m.add_hole_to_phase_field(W - 14, H - 14, 5)
    m.define()
    return m


def blobs(H, W, state):
    """`state` with the potential of three separated blobs — a block larger than a tile, a disc, and a disc that touches the hole —
    and the gates closed between them, so that the three waves stay apart for a while (on the CPU oracle: several waves in 11
    and 18 of the 70 samples on the two grids, one wave over the whole sheet in between, the first gaps opening at the end)"""
    r, c = np.mgrid[0:H, 0:W]
    discs = [(H - 8, 7), (H - 14, W - 22)]
    v = np.zeros((H, W), np.float32)
    v[2:int(0.5 * H), 2:int(0.6 * W)] = 1.0
    quiet = np.ones((H, W), bool)
    quiet[:int(0.5 * H) + 2] = False
    for y, x in discs:
        v[np.hypot(r - y, c - x) <= 3.5] = 1.0
        quiet[np.hypot(r - y, c - x) <= 6] = False
    out = state.copy()
    out[0] = v
    out[1][quiet] = 0.0
    out[2][quiet] = 0.0
    return out


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


DYN_TICKS = 70
DYN_GRIDS = [(64, 64), (130, 67)]
FORCED = '10,44,25,-3'


def dyn_run(shape, env, every=10, poll=False, fast=True, **kw):
    """Fenton with a hole, three blobs, DYN_TICKS single-tick calls -> (counts, records, labels, final state, the states polled at
    the sample ticks, the recorder's mask and level)"""
    H, W = shape
    with plan_env(env), warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        m = fenton_hole(H, W, fast)
        st = m._stepper
        st.set_state(-1, blobs(H, W, st.get_state(-1)))
        polled = []
        with m.record_waves(every=every, capacity=DYN_TICKS // every, **kw) as rec:
            for i in range(DYN_TICKS):
                st.step(1)
                if poll and (i + 1) % every == 0:
                    polled.append(st.get_state(-1).copy())
            assert rec.count() == DYN_TICKS // every
            counts, records = rec.raw()
            labels = rec.labels()
            mask, level = rec.mask, rec.level
        state = st.get_state(-1).tobytes()
        assert st.fallbacks() == (0, 0)
        st.close()
    return counts, records, labels, state, polled, mask, level


def same_run(a, b, what):
    """two runs' samples, byte for byte where the bytes are specified: counts, records sorted by seed, the label plane, the state"""
    assert a[0].tobytes() == b[0].tobytes(), what
    for s in range(len(a[0])):
        ra, rb = ref.sorted_records(a[1][s], a[0][s, 1]), ref.sorted_records(b[1][s], b[0][s, 1])
        assert ra.tobytes() == rb.tobytes(), (what, s)
    assert a[2].tobytes() == b[2].tobytes() and a[3] == b[3], what


@pytest.fixture(scope='module', params=DYN_GRIDS, ids=lambda s: '%dx%d' % s)
def polled_run(request, gpu_lib):
    """every = 1, the state read back behind every tick: each sample equals the reference taken from that state"""
    shape = request.param
    run = dyn_run(shape, {'FIBHIP_VARIANT': FORCED}, every=1, poll=True)
    counts, records, labels, _, polled, mask, level = run
    assert level == 0.5 and not mask[0].any() and not mask[:, 0].any() and not mask[shape[0] - 14, shape[1] - 14]
    several = big = 0
    for s, X in enumerate(polled):
        plane = ref.set_plane(X[0], level, 'above', mask)
        want, rec = check_sample(counts[s], records[s], labels if s == len(polled) - 1 else None, plane, 4, 256, '%dx%d tick %d' % (shape + (s,)))
        several += want[0] >= 2
        big += len(rec) > 0 and rec['area'].max() > TILE[0] * TILE[1]
    # the reference's own output: the planes are not empty — several waves in three samples or more, one larger than a tile
    assert several >= 3 and big >= 1, (several, big)
    return shape, run


def test_dynamics_equal_the_restatement(polled_run):
    shape, run = polled_run
    assert run[0].shape == (DYN_TICKS, 3)


def same_samples(run, base, every, what):
    """the samples of `run` (a stride of `every`, no read-back in between) are the polled run's at the same ticks, byte for byte"""
    assert run[3] == base[3], what
    ticks = list(range(every - 1, DYN_TICKS, every))
    assert len(ticks) == len(run[0]), what
    for s, k in enumerate(ticks):
        assert run[0][s].tobytes() == base[0][k].tobytes(), (what, k)
        assert ref.sorted_records(run[1][s], run[0][s, 1]).tobytes() == ref.sorted_records(base[1][k], base[0][k, 1]).tobytes(), (what, k)
    if ticks[-1] == DYN_TICKS - 1:
        assert run[2].tobytes() == base[2].tobytes(), what


@pytest.mark.parametrize('env', [{'FIBHIP_VARIANT': FORCED, 'FIBHIP_MT': '0'}, {}, {'FIBHIP_VARIANT': '1,64,4,256'}, {'FIBHIP_VARIANT': FORCED}],
                         ids=['one-launch-per-tick', 'unforced', 'flat-tiles', 'forced-small'])
def test_samples_do_not_depend_on_the_launch_plan(gpu_lib, polled_run, env):
    shape, base = polled_run
    same_samples(dyn_run(shape, env, every=10), base, 10, env)


@pytest.mark.parametrize('every', [1, 7])
def test_samples_do_not_depend_on_the_stride(gpu_lib, polled_run, every):
    shape, base = polled_run
    same_samples(dyn_run(shape, {'FIBHIP_VARIANT': FORCED}, every=every), base, every, every)


@pytest.mark.parametrize('shape', DYN_GRIDS, ids=lambda s: '%dx%d' % s)
def test_below_and_a_gate(gpu_lib, shape):
    """kind 'below' (the excitable gap), conn = 8, and `also=` a gate, each against the reference on the polled states"""
    H, W = shape
    for kw, conn in (({'kind': 'below'}, 4), ({'kind': 'below', 'conn': 8, 'level': 0.3}, 8), ({'also': ('V', 'above', 0.5)}, 4),
                     ({'also': (2, 'below', 0.9), 'conn': 8, 'max_waves': 3}, 8)):
        counts, records, labels, _, polled, mask, level = dyn_run(shape, {}, every=10, poll=True, **kw)
        seen = 0
        for s, X in enumerate(polled):
            also = None
            if 'also' in kw:
                a = kw['also']
                also = (X[1 if a[0] == 'V' else a[0]], a[1], a[2])
            plane = ref.set_plane(X[0], level, kw.get('kind', 'above'), mask, also)
            want, _ = check_sample(counts[s], records[s], labels if s == len(polled) - 1 else None, plane, conn, kw.get('max_waves', 256),
                                   '%dx%d %s sample %d' % (H, W, kw, s))
            seen += want[2]
        assert seen > 0, kw


def test_policy_does_not_matter(gpu_lib):
    """the exact and the fast policy on a state set identically: a tick of 1e-30 ms moves no cell of a state that stays clear of
    zero, both handles hold what set_state gave them, and the samples are the same bytes"""
    H, W = 37, 53
    out = []
    for flags in (0, gpu_lib.FAST):
        st = raw_stepper(gpu_lib, H, W, dt=1e-30, seed=9, flags=flags)
        st.waves_begin(0, 0, 0.5, 1, 1, 0.6, 8, random_plane(H, W, 5, 0.9).astype(np.uint8), 256, 1, 1)
        st.step(1)
        counts, records = st.waves_read()
        X = st.get_state(-1).copy()
        plane = ref.set_plane(X[0], 0.5, 'above', random_plane(H, W, 5, 0.9), (X[1], 'below', 0.6))
        want, _ = check_sample(counts[0], records[0], st.waves_labels(), plane, 8, 256, 'policy flags %d' % flags)
        assert want[0] >= 2
        out.append((X.tobytes(), counts.tobytes(), ref.sorted_records(records[0], counts[0, 1]).tobytes(), st.waves_labels().tobytes()))
        st.close()
    assert out[0] == out[1]


@pytest.mark.parametrize('kind', [0, 1], ids=['above', 'below'])
def test_nan_is_never_set(gpu_lib, kind):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W, seed=2)
    x = st.get_state(-1).copy()
    x[0, 20, 30] = np.nan
    st.set_state(-1, x)
    st.waves_begin(0, kind, 0.5, -1, 0, 0.0, 4, None, 256, 1, 1)
    st.step(1)
    counts, records = st.waves_read()
    labels = st.waves_labels()
    X = st.get_state(0).copy()
    assert np.isnan(X[20, 30]) and labels[20, 30] == -1
    nan = np.isnan(X)
    assert np.all(labels[nan] == -1)
    plane = ref.set_plane(X, 0.5, 'below' if kind else 'above')
    want, _ = check_sample(counts[0], records[0], labels, plane, 4, 256, 'NaN kind %d' % kind)
    assert want[2] > 0
    st.close()


# ---- other models and API edges --------------------------------------------------------------------------------------------
def test_beeler_reuter(gpu_lib):
    from test_gpu_leads import hole_model
    H, W = 37, 53
    m = hole_model('br', H, W)
    wave(m, 'br')
    st = m._stepper
    with m.record_waves(level=-40, capacity=1) as rec:
        st.step(1)
        X = st.get_state(0).copy()
        counts, records = rec.raw()
        plane = ref.set_plane(X, -40, 'above', rec.mask)
        want, _ = check_sample(counts[0], records[0], rec.labels(), plane, 4, 256, 'Beeler-Reuter')
        assert want[0] >= 1
        w, first = rec.waves()[0], ref.sorted_records(records[0], counts[0, 1])
        assert w['t_ms'][0] == m.dt_per_step * m.dt and np.array_equal(w['seed'], first['seed'])
        assert np.array_equal(w['cy'], first['sum_r'] / first['area']) and np.array_equal(w['cx'], first['sum_c'] / first['area'])
        assert np.array_equal(rec.counts(), counts) and len(rec.truncated()) == 0 and rec.times_ms().tolist() == [m.dt_per_step * m.dt]
    st.close()


def test_courtemanche_on_a_slow_array(gpu_lib):
    """`also=` on an array 'slow' assigns, 'slow' fired right behind the sample tick: the sample sees the array as the tick left it"""
    from test_gpu_leads import hole_model
    H, W = 37, 53
    m = hole_model('court', H, W)
    wave(m, 'court')
    st = m._stepper
    slow = type(m).tip_signals[1]
    X0 = st.get_state(slow)[1:-1, 1:-1]
    assert X0.min() < X0.max()                                # (the stimulus of wave() has moved the array where it fired)
    mid = float(0.5 * (np.float64(X0.min()) + np.float64(X0.max())))
    with m.record_waves(level=-200, also=(slow, 'above', mid), capacity=1) as rec:
        st.step(1)
        X = st.get_state(-1).copy()
        m.fire_op('slow')                                     # belongs to the next tick
        counts, records = rec.raw()
        plane = ref.set_plane(X[0], -200, 'above', rec.mask, (X[slow], 'above', np.float32(mid)))
        want, _ = check_sample(counts[0], records[0], rec.labels(), plane, 4, 256, 'Courtemanche, slow array')
        assert 0 < want[2] < rec.mask.sum()
    st.close()


def test_refusals(gpu_lib):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W)
    ok = dict(var=0, kind=0, level=0.5, var2=-1, kind2=0, level2=0.0, conn=4, mask=None, max_waves=16, every=1, capacity=1)
    for change, msg in (({'conn': 6}, r'conn is 4 or 8 \(got 6\)'), ({'var': 4}, 'bad var 4'), ({'var': -1}, 'bad var -1'),
                        ({'var2': 4}, 'bad var2 4'), ({'var2': -2}, 'bad var2 -2'), ({'max_waves': 0}, r'1 \.\. 65536 waves per sample \(got 0\)'),
                        ({'max_waves': 65537}, r'got 65537'), ({'level': np.nan}, 'level must be finite'), ({'level': np.inf}, 'level must be finite'),
                        ({'var2': 1, 'level2': -np.inf}, 'level2 must be finite'), ({'kind': 2}, 'bad kind 2'), ({'var2': 1, 'kind2': -1}, 'bad kind2 -1'),
                        ({'every': 0}, 'every must be >= 1'), ({'capacity': 0}, 'bad capacity 0')):
        with pytest.raises(gpu_lib.FibhipError, match=msg):
            st.waves_begin(**dict(ok, **change))
    for call in (st.waves_count, st.waves_labels, lambda: st.waves_read(0, 0)):
        with pytest.raises(gpu_lib.FibhipError, match='no recorder attached'):
            call()
    st.waves_end()                                            # (no recorder attached: nothing)
    st.waves_begin(**dict(ok, every=2))
    with pytest.raises(gpu_lib.FibhipError, match='no sample has been taken yet'):
        st.waves_labels()
    st.step(1)
    with pytest.raises(gpu_lib.FibhipError, match='no sample has been taken yet'):
        st.waves_labels()
    st.step(1)
    assert st.waves_labels().shape == (H, W)
    st.waves_end()
    st.step_edges()
    with pytest.raises(gpu_lib.FibhipError, match='waves_begin inside an open tick'):
        st.waves_begin(**ok)
    st.step_interior()
    st.step_commit()
    st.close()
    shard = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    with pytest.raises(gpu_lib.FibhipError, match='not on a row block'):
        shard.waves_begin(**ok)
    shard.close()


def test_capacity_count_and_read_ranges(gpu_lib):
    H, W = 37, 53
    st = raw_stepper(gpu_lib, H, W)
    st.waves_begin(0, 0, 0.5, -1, 0, 0.0, 4, None, 64, 2, 3)
    assert st.waves_count() == 0 and st.waves_read()[0].shape == (0, 3)
    states = []
    for i in range(6):
        st.step(1)
        if i % 2 == 1:
            states.append(st.get_state(0).copy())
    assert st.waves_count() == 3
    counts, records = st.waves_read()
    for s in range(3):
        check_sample(counts[s], records[s], st.waves_labels() if s == 2 else None, ref.set_plane(states[s], 0.5), 4, 64, 'sample %d' % s)
    c12, r12 = st.waves_read(1, 2)
    assert c12.tobytes() == counts[1:].tobytes() and r12.tobytes() == records[1:].tobytes()
    assert st.waves_read(3, 0)[0].shape == (0, 3)
    with pytest.raises(gpu_lib.FibhipError, match=r'samples \[2, 4\) of 3 taken'):
        st.waves_read(2, 2)
    st.step(1)                                                # tick 7: no sample
    launches = st.launch_stats()['launches']
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(1)                                            # tick 8 would take sample number 3
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(5)
    assert st.launch_stats()['launches'] == launches          # refused before anything was enqueued
    again = st.waves_read()
    assert st.waves_count() == 3 and again[0].tobytes() == counts.tobytes() and again[1].tobytes() == records.tobytes()
    st.waves_end()
    st.step(3)                                                # detached: nothing holds the handle back
    st.close()


def test_timeline_lists_the_sample(gpu_lib):
    st = raw_stepper(gpu_lib, 130, 67)
    st.waves_begin(0, 0, 0.5, -1, 0, 0.0, 4, None, 64, 2, 4)
    st.step(1)
    st.trace_begin()
    st.step(1)
    names = [e['name'].split('<')[0] for e in st.trace_end()]
    assert names[-4:] == ['wave_label_kernel', 'wave_merge_kernel', 'wave_root_kernel', 'wave_reduce_kernel'], names
    st.close()
    st = raw_stepper(gpu_lib, 4, 64)                          # one tile: nothing to merge
    st.waves_begin(0, 0, 0.5, -1, 0, 0.0, 4, None, 64, 1, 4)
    st.trace_begin()
    st.step(1)
    names = [e['name'].split('<')[0] for e in st.trace_end()]
    assert names[-3:] == ['wave_label_kernel', 'wave_root_kernel', 'wave_reduce_kernel'] and 'wave_merge_kernel' not in names, names
    st.close()


def test_example_runs_headless(gpu_lib, tmp_path):
    """examples/run_waves.py end to end at a tiny size, in this process: the two counts over time, the label plane, a PNG"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('run_waves_under_test', os.path.join(root, 'examples', 'run_waves.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = tmp_path / 'waves.png'
    n_waves, n_tips, labels = ex.main(['--size', '64', '--ms', '30', '--every', '5', '--out', str(out)])
    assert n_waves.shape == (6,) and n_tips.shape == (6,) and n_waves.max() >= 1
    assert labels.shape == (64, 64) and labels.max() >= 0 and out.exists()
