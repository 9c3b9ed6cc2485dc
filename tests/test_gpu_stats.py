"""-m gpu: the statistics recorder (include/fibhip.h fibhip_stats_*, fib_tf_amd/stats.py) on the device.

Every sample is compared with the NumPy restatement (tests/stats_ref.py) on the state read back at the sample's tick.  MIN,
MAX, BELOW, ABOVE and NONFINITE must be EQUAL.  SUM is held to |device - exact| <= n * 2^-53 * sum |w * X|, n the cells with
w != 0: the standard bound for a float64 sum of n terms in ANY order, so it rests on no property of the kernel's tree (a
float32 accumulation misses it by about eight orders of magnitude).  The grids are the smallest that reach each path of
stats_kernel: 37 x 53 (scalar, odd everything, two chunks), 64 x 64 (16-byte loads), 20 x 130 (rows not 16-byte aligned),
96 x 100 (several tiles, multi-tick launches) and one 512 x 512 case (256 chunks: the chunk table and the combine tree full)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stats_ref as ref  # noqa: E402
import tip_ref  # noqa: E402
from test_gpu_frames import PLAN_ENV, VARIANT_96x100, wave  # noqa: E402
from test_gpu_tips import MAKERS, court, fenton  # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = [(37, 53), (64, 64), (20, 130), (96, 100)]
LEVELS = {'fenton': (0.5, 0.1), 'br': (-30.0, -80.0), 'court': (-25.0, -75.0), 'traced': (0.5, 0.1)}


def chunk_cells(H, W):
    """stats_begin's chunk table on a planar slab: at most 256 equal chunks of at least 1024 cells, whole 16-byte groups where
    the vector path may run"""
    cs = max(1024, -(-H * W // 256))
    return -(-cs // 4) * 4 if W % 4 == 0 else cs


def model_columns(kind, m):
    """eight columns on array 0, two more arrays, and for Courtemanche a slow array (slow_sample_due)"""
    nvar = m._stepper.nvar
    a, b = LEVELS[kind]
    cols = [(0, 'sum', 0.0), (0, 'min', 0.0), (0, 'max', 0.0), (0, 'below', a), (0, 'above', a), (0, 'nonfinite', 0.0), (0, 'below', b),
            (0, 'above', b), (1, 'sum', 0.0), (1, 'max', 0.0), (nvar - 1, 'min', 0.0), (nvar - 1, 'sum', 0.0)]
    if kind == 'court':
        slow = type(m).tip_signals[1]
        assert type(m).VAR_NAMES[slow] not in ('V', '_Na_i_', '_m_', '_h_')
        cols += [(slow, 'sum', 0.0), (slow, 'below', 0.5), (slow, 'max', 0.0)]
    return cols


def compare(raw, states, cols, weight, mask, what):
    """-> the largest |device - exact| / bound over the SUM columns"""
    assert raw.shape == (len(states), len(cols)) and raw.dtype == np.float64, (what, raw.shape)
    worst = 0.0
    for s, x in enumerate(states):
        want = ref.sample(x, cols, weight, mask)
        for j, (var, kind, level) in enumerate(cols):
            if kind == 'sum' and not np.isfinite(want[j]):        # a NaN or Inf under a non-zero weight propagates
                assert np.isnan(raw[s, j]) if np.isnan(want[j]) else raw[s, j] == want[j], '%s sample %d column %d: device %r exact %r' % (
                    what, s, j, raw[s, j], want[j])
            elif kind == 'sum':
                bound = ref.sum_bound(x[var], weight)
                err = abs(raw[s, j] - want[j])
                assert np.isfinite(raw[s, j]) and err <= bound, '%s sample %d column %d (%s of array %d): device %r exact %r bound %g' % (
                    what, s, j, kind, var, raw[s, j], want[j], bound)
                if bound > 0:
                    worst = max(worst, err / bound)
            else:
                assert raw[s, j] == want[j], '%s sample %d column %d (%s of array %d): device %r reference %r' % (
                    what, s, j, kind, var, raw[s, j], want[j])
    return worst


def planes(H, W, seed):
    rng = np.random.default_rng(seed)
    weight = rng.uniform(0.05, 1.0, (H, W)).astype(np.float32)
    weight[rng.uniform(size=(H, W)) < 0.2] = 0
    mask = (rng.uniform(size=(H, W)) < 0.7).astype(np.uint8)
    return weight, mask


@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_samples_equal_the_restatement(gpu_lib, kind, shape):
    H, W = shape
    m = MAKERS[kind](H, W)
    wave(m, kind)
    st = m._stepper
    cols = model_columns(kind, m)
    weight, mask = planes(H, W, 1000 * H + W)
    worst, varied, n = 0.0, 0, 0
    for every in (1, 3):
        for wt, mk in ((weight, mask), (None, mask), (weight, None), (None, None)):
            st.stats_begin(cols, wt, mk, every, 6 // every)
            states = []
            for i in range(6):
                if kind == 'court' and i == 3:
                    m.fire_op('slow')
                st.step(1)
                if (i + 1) % every == 0:
                    states.append(st.get_state(-1).copy())
            assert st.stats_count() == 6 // every
            raw = st.stats_read()
            what = '%s %dx%d every %d weight %s mask %s' % (kind, H, W, every, wt is not None, mk is not None)
            worst = max(worst, compare(raw, states, cols, wt, mk, what))
            varied += len(np.unique(raw[:, 0])) > 1
            n += 1
            st.stats_end()
    assert varied > 0                                         # (a wave is under way: the sums move)
    print('%s %dx%d: %d configurations, largest |device - exact| / bound over the SUM columns: %.3g' % (kind, H, W, n, worst))
    st.close()


def test_full_chunk_table(gpu_lib):
    """512 x 512: 256 chunks of 1024 cells, every lane of the combine tree holds four partials"""
    assert chunk_cells(512, 512) == 1024 and 512 * 512 // 1024 == 256
    m = fenton(512, 512)
    wave(m, 'fenton')
    st = m._stepper
    cols = model_columns('fenton', m)
    weight, mask = planes(512, 512, 7)
    st.stats_begin(cols, weight, mask, 2, 2)
    states = []
    for i in range(4):
        st.step(1)
        if i % 2 == 1:
            states.append(st.get_state(-1).copy())
    worst = compare(st.stats_read(), states, cols, weight, mask, '512x512')
    print('512x512: largest |device - exact| / bound over the SUM columns: %.3g' % worst)
    st.close()


@pytest.mark.parametrize('shape', [(37, 53), (64, 64)], ids=lambda s: '%dx%d' % s)
def test_row_interleaved_slab(gpu_lib, shape):
    """a handle whose slab is row-interleaved (pitch = nvar * W: the layout of a row block, here without ghost rows): the scalar
    path's row * pitch + column addressing with pitch != W, under a weight plane and a mask"""
    H, W = shape
    st = gpu_lib.Stepper(gpu_lib.FENTON4V, H, W, 0.1, 1.3, flags=gpu_lib.FAST | gpu_lib.ROW_INTERLEAVED)
    rng = np.random.default_rng(H + W)
    st.set_state(-1, rng.uniform(0, 1, (4, H, W)).astype(np.float32))
    weight, mask = planes(H, W, H * W + 1)
    cols = [(v, k, 0.5) for v in range(4) for k in ('sum', 'min', 'max', 'below', 'above', 'nonfinite')]
    st.stats_begin(cols, weight, mask, 2, 2)
    states = []
    for i in range(4):
        st.step(1)
        if i % 2 == 1:
            states.append(st.get_state(-1).copy())
    worst = compare(st.stats_read(), states, cols, weight, mask, 'row-interleaved %dx%d' % (H, W))
    assert len({s[v].tobytes() for s in states for v in range(4)}) == 8      # (eight different arrays: none was taken for another)
    print('row-interleaved %dx%d: largest |device - exact| / bound over the SUM columns: %.3g' % (H, W, worst))
    st.close()


PLANT_COLS = [(2, 'max', 0.0), (2, 'min', 0.0), (2, 'nonfinite', 0.0), (2, 'below', 2.0), (2, 'above', 0.7), (2, 'below', 0.3),
              (2, 'sum', 0.0), (3, 'sum', 0.0)]


def plant_cells(H, W):
    cs = chunk_cells(H, W)
    n = H * W
    rng = np.random.default_rng(H * W)
    cells = [0, W - 1, (H - 1) * W, n - 1, (H - 1) * W + W // 2, (H // 2) * W + W - 1, ((n - 1) // cs) * cs,
             int(rng.integers(1, H - 1)) * W + int(rng.integers(1, W - 1))]
    assert ((n - 1) // cs) * cs > 0                           # (every grid here has more than one chunk)
    return cells


@pytest.mark.parametrize('shape', GRIDS + [(512, 512)], ids=lambda s: '%dx%d' % s)
def test_no_cell_is_missed_or_taken_twice(gpu_lib, shape):
    """a constant gate array (Fenton's array 2: pointwise, no stencil) with ONE planted cell, one tick, one sample: the spike is
    the maximum and the only cell above 0.7, the dip the minimum and the only cell below 0.3, the NaN and the Inf are each
    counted once — at the four corners, in the last row, in the last column, at the first cell of the last chunk and at a
    seeded interior cell.  What the tick made of the planted value is read back; that the cell is seen exactly once is not
    left to the restatement alone: the counts are asserted to be 1."""
    H, W = shape
    n = H * W
    st = gpu_lib.Stepper(gpu_lib.FENTON4V, H, W, 0.1, 1.3, flags=gpu_lib.FAST)
    base = np.full((4, H, W), 0.5, np.float32)
    st.set_state(-1, base)
    cells = plant_cells(H, W)
    st.stats_begin(PLANT_COLS, None, None, 1, 4 * len(cells))
    states, planted = [], []
    for cell in cells:
        for value in (0.9, 0.1, np.nan, np.inf):
            x = base[2].copy()
            x.ravel()[cell] = value
            st.set_state(2, x)
            st.step(1)
            states.append(st.get_state(-1).copy())
            st.set_state(-1, base)                            # (whatever the planted value did to the other arrays is undone)
            planted.append((cell, value))
    raw = st.stats_read()
    compare(raw, states, PLANT_COLS, None, None, '%dx%d planted' % (H, W))
    for s, (cell, value) in enumerate(planted):
        x = states[s][2].ravel()
        row = dict(zip(('max', 'min', 'nonfinite', 'all', 'above', 'below'), raw[s]))
        what = '%dx%d cell %d (row %d, column %d) value %r: %r' % (H, W, cell, cell // W, cell % W, value, row)
        if value == 0.9:
            assert row['above'] == 1 and row['max'] == x[cell] and np.nanargmax(x) == cell and row['nonfinite'] == 0, what
            assert row['below'] == 0 and row['all'] == n, what
        elif value == 0.1:
            assert row['below'] == 1 and row['min'] == x[cell] and np.nanargmin(x) == cell and row['nonfinite'] == 0, what
            assert row['above'] == 0 and row['all'] == n, what
        else:
            assert not np.isfinite(x[cell]) and row['nonfinite'] == 1, what
            assert row['all'] + row['above'] >= n - 1, what
    st.stats_end()
    # under a mask and a weight plane: BELOW with a level above every value is the mask's cell count; a NaN under a zero weight
    # leaves SUM finite, the same NaN under a non-zero weight makes it NaN
    weight, mask = planes(H, W, n)
    cell = cells[-1]
    x = base[2].copy()
    x.ravel()[cell] = np.nan
    for wv in (0.0, 0.75):
        weight.ravel()[cell] = wv
        mask.ravel()[cell] = 1
        st.set_state(-1, base)
        st.stats_begin(PLANT_COLS, weight, mask, 1, 2)
        st.step(1)
        clean = st.get_state(-1).copy()
        st.set_state(2, x)
        st.step(1)
        dirty = st.get_state(-1).copy()
        raw = st.stats_read()
        assert raw[0, 3] == np.count_nonzero(mask) and raw[1, 3] == np.count_nonzero(mask) - 1 and raw[1, 2] == 1, raw
        assert np.isnan(dirty[2].ravel()[cell])
        compare(raw[:1], [clean], PLANT_COLS, weight, mask, '%dx%d masked' % (H, W))
        if wv == 0.0:
            compare(raw[1:], [dirty], PLANT_COLS, weight, mask, '%dx%d NaN under a zero weight' % (H, W))
            assert np.isfinite(raw[1, 6])
        else:
            assert np.isnan(raw[1, 6]), raw[1]
            compare(raw[1:], [dirty], PLANT_COLS, weight, mask, '%dx%d NaN under a weight' % (H, W))
        st.stats_end()
    st.close()


def _plan_run(gpu_lib, monkeypatch, env, record, calls=40, every=10):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')                                         # (plan selection happens at the first tick)
    weight, mask = planes(96, 100, 4)
    cols = model_columns('fenton', m)
    out = None
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        s0 = st.launch_stats()
        if record:
            st.stats_begin(cols, weight, mask, every, calls // every)
        for i in range(calls):
            st.step(1)
        if record:
            assert st.stats_count() == calls // every
            out = st.stats_read()
        state = st.get_state(-1)
        fb, s1 = st.fallbacks(), st.launch_stats()
    st.close()
    return out, state, fb, {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}


def test_table_does_not_depend_on_the_launch_plan(gpu_lib, monkeypatch):
    forced = {'FIBHIP_VARIANT': VARIANT_96x100}
    raw, state, fb, stats = _plan_run(gpu_lib, monkeypatch, forced, True)
    assert fb[0] == 0
    # between two samples the handle runs the fewest launches `every` allows: four ten-tick launches, two launches per sample
    assert stats['ticks'] == 40 and stats['mt_ticks'] == 40 and stats['mt_launches'] == 4, stats
    assert stats['launches'] == stats['mt_launches'] + 2 * 4, stats
    assert raw.shape == (4, 12) and any(raw[s].tobytes() != raw[0].tobytes() for s in range(1, 4))
    for env in ({}, {'FIBHIP_MT': '0'}, {'FIBHIP_AHEAD': '0'}, dict(forced, FIBHIP_MT='0'), dict(forced, FIBHIP_AHEAD='0'),
                dict(forced, FIBHIP_MT_FAKE_GIVEUP='2')):
        r2, st2, fb2, stats2 = _plan_run(gpu_lib, monkeypatch, env, True)
        assert r2.tobytes() == raw.tobytes(), (env, r2, raw)
        assert st2.tobytes() == state.tobytes(), env
        assert stats2['ticks'] == 40, (env, stats2)
        if 'FIBHIP_MT_FAKE_GIVEUP' in env:
            assert fb2[0] == 1 and fb2[1] > 0, fb2            # one launch gave up and was recovered
        elif 'FIBHIP_MT' in env:
            assert stats2['mt_ticks'] == 0
        elif 'FIBHIP_VARIANT' in env:
            assert stats2['mt_ticks'] == 40 and stats2['mt_launches'] == 4, (env, stats2)
        else:                                                 # the plan the handle chooses itself: multi-tick launches ran there too
            print('plan %r: %r' % (env, stats2))
            assert fb2[0] == 0 and stats2['mt_ticks'] > 0, (env, stats2)
    _, plain, _, pstats = _plan_run(gpu_lib, monkeypatch, forced, False)
    assert plain.tobytes() == state.tobytes()                 # the recorder changes nothing of the state
    assert pstats['ticks'] == 40 and pstats['mt_ticks'] > 0
    assert pstats['launches'] == pstats['mt_launches'] + (pstats['ticks'] - pstats['mt_ticks']), pstats


def test_sixty_four_single_tick_calls_are_eight_launches(gpu_lib, monkeypatch):
    raw, _, fb, stats = _plan_run(gpu_lib, monkeypatch, {'FIBHIP_VARIANT': VARIANT_96x100}, True, calls=64, every=8)
    assert fb[0] == 0 and raw.shape[0] == 8
    assert stats['mt_ticks'] == 64 and stats['mt_launches'] == 8 and stats['launches'] == 8 + 2 * 8, stats


def _four(gpu_lib, which, ticks=60):
    """electrodes every 3, tips every 4, frames every 5 and statistics every 7 ticks (those named in `which`) on one handle"""
    from fib_tf_amd import egm
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    _, var2, a0, b0 = m.tip_signals
    rect, patch = egm.crop_mask(egm.create_mask(m, 60, 40, 5))
    weight, mask = planes(96, 100, 4)
    s0 = st.launch_stats()
    if 'el' in which:
        st.electrode_begin(0, [rect], [patch], 3, ticks // 3)
    if 'tip' in which:
        st.tips_begin(0, var2, a0, b0, None, 4, 256, ticks // 4)
    if 'fr' in which:
        st.frames_begin(0, (0, 96, 0, 100), (2, 2), 'mean', 0.0, 1.0, None, 'uint8', 5, 5, ticks // 5)
    if 'st' in which:
        st.stats_begin(model_columns('fenton', m), weight, mask, 7, ticks // 7)
    st.step(ticks)
    out = {}
    if 'el' in which:
        out['el'] = st.electrode_read().tobytes()
    if 'tip' in which:
        c, r = st.tips_read()
        out['tip'] = (c.tobytes(), [tip_ref.sorted_records(r[s], c[s, 2], 256).tobytes() for s in range(len(c))])
    if 'fr' in which:
        out['fr'] = st.frames_read().tobytes()
    if 'st' in which:
        assert st.stats_count() == ticks // 7
        out['st'] = st.stats_read().tobytes()
    s1 = st.launch_stats()
    st.close()
    return out, {k: s1[k] - s0[k] for k in s0 if k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}


def test_four_samplers_on_one_handle(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    all4, stats = _four(gpu_lib, ('el', 'tip', 'fr', 'st'))
    cuts = [t for t in range(1, 61) if t % 3 == 0 or t % 4 == 0 or t % 5 == 0 or t % 7 == 0]
    lengths = np.diff([0] + cuts)
    samples = 60 // 3 + 60 // 4 + 60 // 5 + 2 * (60 // 7)      # (the statistics recorder: two launches per sample)
    assert stats['ticks'] == 60, stats
    assert stats['mt_launches'] == int((lengths >= 2).sum()) and stats['mt_ticks'] == int(lengths[lengths >= 2].sum()), (stats, lengths)
    assert stats['launches'] == len(cuts) + samples, (stats, len(cuts), samples)
    for which in ('el', 'tip', 'fr', 'st'):
        alone, _ = _four(gpu_lib, (which,))
        assert alone[which] == all4[which], which             # each records what it records alone


def test_with_the_activation_recorder_every_tick_is_one_launch(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    tables = []
    for activation in (False, True):
        m = fenton(96, 100)
        st = m._stepper
        wave(m, 'fenton')
        rec = m.record_activation() if activation else None
        st.stats_begin(model_columns('fenton', m), None, None, 5, 4)
        s0 = st.launch_stats()
        st.step(20)
        tables.append(st.stats_read())
        s1 = st.launch_stats()
        assert s1['ticks'] - s0['ticks'] == 20
        if activation:
            assert s1['mt_ticks'] == s0['mt_ticks']
            assert s1['launches'] - s0['launches'] == 20 + 20 + 2 * 4
            rec.close()
        else:
            assert s1['mt_launches'] - s0['mt_launches'] == 4 and s1['launches'] - s0['launches'] == 4 + 2 * 4
        st.close()
    assert tables[0].tobytes() == tables[1].tobytes()


def test_court_sample_of_a_slow_array_is_taken_before_slow(gpu_lib):
    """a sample due at the tick 'slow' would ride on, one of its columns on a slow array: the two are not fused, the row holds
    the array as the tick left it"""
    from fib_tf_amd.court import Courtemanche
    slow_var = Courtemanche.tip_signals[1]
    twin = court(64, 80)
    wave(twin, 'court')
    twin._stepper.step(5)
    before = twin._stepper.get_state(-1).copy()
    twin.fire_op('slow')
    after = twin._stepper.get_state(slow_var).copy()
    twin._stepper.close()
    assert before[slow_var].tobytes() != after.tobytes()
    m = court(64, 80)
    wave(m, 'court')
    st = m._stepper
    cols = [(0, 'min', 0.0), (slow_var, 'sum', 0.0), (slow_var, 'max', 0.0), (slow_var, 'below', 0.5)]
    st.stats_begin(cols, None, None, 5, 2)
    st.step(5)                                                # (the last tick may be held back for 'slow' to ride on)
    m.fire_op('slow')
    assert st.stats_count() == 1
    raw = st.stats_read()
    compare(raw, [before], cols, None, None, 'slow array')
    assert raw[0, 2] != float(after.max()) or raw[0, 3] != np.count_nonzero(after < 0.5)       # (not the array behind 'slow')
    assert st.get_state(slow_var).tobytes() == after.tobytes()
    st.close()


def test_capacity_and_reading(gpu_lib):
    m = fenton(37, 53)
    wave(m, 'fenton')
    st = m._stepper
    cols = model_columns('fenton', m)
    st.stats_begin(cols, None, None, 2, 3)
    st.step(5)
    assert st.stats_count() == 2                              # (ticks accepted but not launched yet count)
    st.sync()
    ticks = st.launch_stats()['ticks']
    two = st.stats_read()
    state = st.get_state(-1)
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(3)                                            # would take sample number 3
    st.sync()
    assert st.launch_stats()['ticks'] == ticks                # nothing of the refused call ran
    assert st.get_state(-1).tobytes() == state.tobytes() and st.stats_read().tobytes() == two.tobytes()
    st.step(1)                                                # sample number 2 still fits: the table is full now
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(2)
    st.sync()
    assert st.launch_stats()['ticks'] == ticks + 1
    raw = st.stats_read()
    assert raw.shape == (3, len(cols)) and raw[:2].tobytes() == two.tobytes()
    compare(raw[2:], [st.get_state(-1)], cols, None, None, 'last sample')
    assert st.stats_read(1, 2).tobytes() == raw[1:].tobytes() and st.stats_read(3, 0).shape == (0, len(cols))
    for first, count in ((0, 4), (2, 2), (-1, 1), (4, 0), (0, -1)):
        with pytest.raises(gpu_lib.FibhipError, match='stats_read'):
            st.stats_read(first, count)
    st.stats_end()
    st.stats_end()                                            # (nothing attached: nothing to do)
    with pytest.raises(gpu_lib.FibhipError, match='no recorder'):
        st.stats_read(0, 0)
    with pytest.raises(gpu_lib.FibhipError, match='no recorder'):
        st.stats_count()
    st.step(30)                                               # the handle runs on without a recorder
    st.stats_begin(cols, None, None, 1, 2)
    st.step(1)
    st.close()                                                # destroyed with a recorder attached


def test_refusals(gpu_lib):
    import ctypes as C
    m = fenton(64, 80)
    st = m._stepper
    L, h = st._L, st._h
    plane = np.ones((64, 80), np.float32)

    def begin(cols=((0, 0, 0.0),), weight=None, every=1, cap=4, handle=h, ncols=None):
        arr = (gpu_lib.StatCol * max(len(cols), 1))()
        for i, (v, k, lv) in enumerate(cols):
            arr[i].var, arr[i].kind, arr[i].level = v, k, lv
        wp = weight.ctypes.data_as(C.POINTER(C.c_float)) if weight is not None else None
        return L.fibhip_stats_begin(handle, len(cols) if ncols is None else ncols, arr, wp, None, every, cap)
    bad_w = plane.copy()
    bad_w[5, 7] = np.inf
    nan_w = plane.copy()
    nan_w[63, 79] = np.nan
    bad = [(dict(cols=((-1, 0, 0.0),)), b'bad var -1'), (dict(cols=((0, 1, 0.0), (st.nvar, 0, 0.0))), b'column 1: bad var'),
           (dict(cols=((0, 6, 0.0),)), b'unknown kind 6'), (dict(cols=((0, -1, 0.0),)), b'unknown kind -1'),
           (dict(cols=((0, 3, float('nan')),)), b'level must be a number'), (dict(cols=((0, 4, float('nan')),)), b'level must be a number'),
           (dict(weight=bad_w), b'not finite (row 5, column 7)'), (dict(weight=nan_w), b'not finite (row 63, column 79)'),
           (dict(cols=tuple((1, 1, 0.0) for _ in range(9))), b'more than 8 columns on array 1'), (dict(every=0), b'every must be >= 1'),
           (dict(every=-2), b'every must be >= 1'), (dict(cap=0), b'bad capacity 0'), (dict(cap=-1), b'bad capacity'),
           (dict(cap=2 ** 62), b'bad capacity'), (dict(ncols=0), b'1 .. 64 columns'), (dict(ncols=65), b'1 .. 64 columns')]
    for kw, msg in bad:
        assert begin(**kw) == -1, kw
        err = L.fibhip_last_error()
        assert b'stats_begin' in err and msg in err, (kw, err)
    k = C.c_longlong()
    assert L.fibhip_stats_count(h, C.byref(k)) != 0 and b'no recorder' in L.fibhip_last_error()        # nothing was attached
    assert begin(cols=((0, 1, float('nan')), (0, 0, float('nan')), (0, 5, float('nan')))) == 0          # a level nobody reads
    assert begin() == -1 and b'attached already' in L.fibhip_last_error()                             # a second begin without an end
    k.value = -1
    assert L.fibhip_stats_count(h, C.byref(k)) == 0 and k.value == 0
    assert L.fibhip_stats_end(h) == 0
    st.step_edges()
    assert begin() == -1 and b'open tick' in L.fibhip_last_error()
    st.step_interior()
    st.step_commit()
    st.stats_begin([(v, 1 + i % 2, 0.0) for v in range(4) for i in range(8)])       # 32 columns, 8 on each array (through the binding,
                                                                                    # which sizes the rows stats_read hands to the library)
    st.step(1)
    raw = st.stats_read()
    x = st.get_state(-1)
    assert raw.shape == (1, 32) and raw[0, 8] == x[1].min() and raw[0, 31] == x[3].max()
    assert begin(handle=None) != 0
    assert L.fibhip_stats_count(h, None) != 0
    assert L.fibhip_stats_read(h, 0, 1, None) != 0 and b'null destination' in L.fibhip_last_error()
    assert L.fibhip_stats_end(h) == 0 and L.fibhip_stats_end(h) == 0
    with pytest.raises(ValueError, match='weight plane'):
        st.stats_begin([(0, 'sum', 0.0)], weight=np.ones((3, 3), np.float32))
    with pytest.raises(ValueError, match='a mask of shape'):
        st.stats_begin([(0, 'min', 0.0)], mask=np.ones((3, 3), np.uint8))
    st.close()


def test_row_block_refused_by_the_library(gpu_lib):
    blk = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    arr = (gpu_lib.StatCol * 1)()
    rc = blk._L.fibhip_stats_begin(blk._h, 1, arr, None, None, 1, 4)
    assert rc == -1 and b'row block' in blk._L.fibhip_last_error()
    blk.close()


@pytest.mark.parametrize('kind', ['fenton', 'court'])
def test_timeline_lists_the_sample(gpu_lib, kind):
    m = MAKERS[kind](96, 130)
    st = m._stepper
    st.step(1)
    st.stats_begin(model_columns(kind, m), None, None, 2, 8)
    names = [e['name'] for e in st.trace_tick()] + ['|'] + [e['name'] for e in st.trace_tick()]
    assert names.count('stats_kernel') == 1 and names.count('stats_combine_kernel') == 1, names
    assert names.index('|') < names.index('stats_kernel') < names.index('stats_combine_kernel'), names
    st.close()


def test_recorder_object(gpu_lib):
    """StatsRecorder end to end on a model with a hole: names, the default weight and mask, mean and fractions, the finite check"""
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': 96, 'width': 100, 'dt': 0.1, 'dt_per_plot': 100, 'diff': 1.5, 'duration': 1000})
    m.add_hole_to_phase_field(50, 48, 9)
    m.define()
    m.duration = 12.5 * m.dt_per_step * m.dt                  # twelve ticks
    st = m._stepper
    names = type(m).VAR_NAMES
    columns = [(names[0], 'mean'), (1, 'mean'), (names[0], 'frac_above', 0.5), (names[0], 'min'), (names[0], 'max'),
               (names[0], 'nonfinite'), (names[0], 'sum')]
    with m.record_stats(columns, every=4) as rec:
        assert rec.capacity == 3 and np.array_equal(rec.weight, m.phase) and np.array_equal(rec.mask != 0, m.phase > 0.5)
        assert not rec.mask.all() and rec.cells == np.count_nonzero(m.phase > 0.5)
        states = []
        for i in m.run():
            if (i + 1) % 4 == 0:
                states.append(st.get_state(-1).copy())
        assert rec.count() == 3
        raw, t = rec.raw(), rec.table()
        dev = [(c.var, k, c.level) for c, k in zip(rec.columns, ('sum', 'sum', 'above', 'min', 'max', 'nonfinite', 'sum'))]
        compare(raw, states, dev, m.phase, rec.mask, 'recorder object')
        assert t.dtype.names == ('t_ms', '%s_mean' % names[0], '%s_mean' % names[1], '%s_frac_above' % names[0], '%s_min' % names[0],
                                 '%s_max' % names[0], '%s_nonfinite' % names[0], '%s_sum' % names[0])
        assert np.allclose(t['t_ms'], [4 * rec.tick_ms, 8 * rec.tick_ms, 12 * rec.tick_ms])
        for s, x in enumerate(states):
            want = np.average(x[0].astype(np.float64), weights=m.phase.astype(np.float64))
            wx = np.abs(m.phase.astype(np.float64) * x[0].astype(np.float64)).sum() / m.phase.astype(np.float64).sum()
            assert abs(t[s][1] - want) <= np.count_nonzero(m.phase) * 2.0 ** -53 * wx, (s, t[s][1], want)
            assert t[s][3] == np.count_nonzero(x[0][m.phase > 0.5] > np.float32(0.5)) / rec.cells
            assert t[s][7] == raw[s, 6]
        rec.check_finite()
        x = st.get_state(0).copy()
        x[40, 10] = np.nan
        st.set_state(0, x)
        with pytest.raises(gpu_lib.FibhipError, match='trace full'):
            st.step(4)
    with m.record_stats([(names[0], 'nonfinite'), (names[0], 'mean')], every=2, capacity=2) as rec:
        st.step(4)
        with pytest.raises(FloatingPointError, match=r'sample 0 \(after tick 1'):
            rec.check_finite()
    with pytest.raises(AssertionError, match='closed'):
        rec.count()
    with pytest.raises(ValueError, match='unknown array'):
        m.record_stats([('nope', 'mean')])
    st.close()


def test_court_ultra_observables(gpu_lib):
    """record_observables against cl_observer's own expressions (np.average of the float32 arrays read back, weights = phase)
    and run_small's ρ, evaluated on the arrays read back at the same ticks.  np.average works in float32 here (both inputs are
    float32).  The bound: n * 2^-24 * sum |w * x| / sum w, n the cells — every product is rounded once and no term passes through
    more than n - 1 float32 additions, so the weighted sum is within n u sum |w * x| of the exact one in ANY order, u = 2^-24
    (NumPy's pairwise order stays near log2(n) u, which also leaves room for the rounding of sum w and of the quotient).  The
    device's own error, n * 2^-53 of the same sum, vanishes beside it.  ρ is met exactly."""
    from fib_tf_amd import court_ultra
    for ultra_slow in (False, True):
        m = court_ultra.Courtemanche({'height': 64, 'width': 80, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 0.809, 'duration': 1000,
                                      'ultra_slow': ultra_slow})
        m.add_hole_to_phase_field(40, 32, 8)
        m.add_hole_to_phase_field(40, 32, 30, neg=True)
        m.define()
        st = m._stepper
        st.pace(20, 27, 26, 35, 20.0, float(m.min_v))
        with court_ultra.record_observables(m, every=3, capacity=4) as rec:
            polled = []
            for i in range(12):
                st.step(1)
                if (i + 1) % 3 == 0:
                    row = [m._State['_Na_i_'].eval().copy(), m._State['_f_Ca_'].eval().copy()]
                    if ultra_slow:
                        row.append(m._State['_us_'].eval().copy())
                    polled.append((row, m.image()))
            t = rec.table()
            fields = ['_Na_i__mean', '_f_Ca__mean'] + (['_us__mean'] if ultra_slow else []) + ['V_frac_below', 'V_nonfinite']
            assert t.dtype.names == tuple(['t_ms'] + fields) and len(t) == 4
            phase = m.phase
            n = phase.size
            for s, (arrays, image) in enumerate(polled):
                for f, x in zip(fields, arrays):
                    want = np.average(x, weights=phase)
                    bound = n * 2.0 ** -24 * float(np.sum(np.abs(phase.astype(np.float64) * x.astype(np.float64)))) / float(
                        np.sum(phase.astype(np.float64)))
                    assert abs(t[f][s] - float(want)) <= bound, (ultra_slow, s, f, t[f][s], want, bound)
                rho = np.sum(image[phase > 1e-3] < 0.2) / np.sum(phase > 1e-3)
                assert t['V_frac_below'][s] == rho, (s, t['V_frac_below'][s], rho)
                assert t['V_nonfinite'][s] == 0
            assert 0 < t['V_frac_below'][-1] < 1
            rec.check_finite()
        st.close()
