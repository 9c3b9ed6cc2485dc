"""-m gpu: Fenton's exchange-period rows (csrc/launch.hpp S4P: K = 6 in 52 x 21 tiles of two-row strips; K = 8 in 48 x 23 and
K = 7 in 50 x 23 passed these tests too, lost at 512 x 512 and left the table with their cases) as the multi-tick launches they are
for — the tiles of one launch hand their rims over every K sub-steps, K below the tick's 10, and only
the launch's last period is short (csrc/strip_kernel.inc PERIODS, csrc/sched.inc mt_launch).

Every comparison is bit for bit, within a policy, with the one-sub-step-per-launch kernel (FIBHIP_VARIANT=1,64,4,256,
FIBHIP_MT=0) on the same inputs and calls, as tests/test_gpu_variant_table.py compares its rows.  The row is forced with
FIBHIP_VARIANT and confirmed to have run: launch_plan() names the period, plan_tile() the row's tile, and the ticks are counted
as multi-tick ticks.

Inputs: a hole in the phase field, the S1 column under way, a 'luq' pace fired mid-run.  Grids: 56 x 112 — a
3 x 3 tile grid with one tile that has all eight neighbours and short tiles at two edges — and 96 x 200, where two interior
tiles are adjacent."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = ('FIBHIP_MT', 'FIBHIP_MT_MAX', 'FIBHIP_MT_FAKE_GIVEUP', 'FIBHIP_AHEAD', 'FIBHIP_MT_WAIT_MS', 'FIBHIP_MT_IDS', 'FIBHIP_VARIANT',
       'FIBHIP_AUTOTUNE', 'FIBHIP_K', 'FIBHIP_ZEROPAD', 'FIBHIP_PERIOD_ROW')
ANCHOR = {'FIBHIP_VARIANT': '1,64,4,256', 'FIBHIP_MT': '0'}
ROWS = [(6, 52, 21, 2)]                                        # K, TX, TY, rows per wave
GRIDS = [(56, 112), (96, 200)]
POLICIES = ['fast', 'exact']
SPT = 10
ROW_IDS = ['K%d' % r[0] for r in ROWS]
GRID_IDS = ['%dx%d' % g for g in GRIDS]


def _env_of(row):
    return {'FIBHIP_VARIANT': '%d,%d,%d,%d' % (row[0], row[1], row[2], -row[3])}


def _model(monkeypatch, policy, H, W, env):
    """Fenton 4v at H x W with a hole in its phase field, its S1 column set, 's2' registered at 'luq'; nothing has run"""
    from fib_tf_amd.fenton import Fenton4v
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = {'width': W, 'height': H, 'dt': 0.1, 'dt_per_plot': SPT, 'duration': 1000, 'skip': False, 'fast_math': policy == 'fast',
           'diff': 1.5}
    m = Fenton4v(cfg)
    m.add_hole_to_phase_field(W // 2 + 3, H // 2 - 2, 9)
    m.define()
    m.add_pace_op('s2', 'luq', 1.0)
    return m, m._stepper


def _ran_as_periods(st, row, stats):
    """None, or why the forced row is not what ran the multi-tick launches"""
    K, TX, TY, R = row
    if st.launch_plan() != (K, 1) or st.plan_tile() != (TX, TY, R):
        return 'row not taken: the plan is %s in tile %s, not (%d, 1) in %s' % (st.launch_plan(), st.plan_tile(), K, (TX, TY, R))
    if not stats['mt_ticks'] > 0:
        return 'no tick ran in a multi-tick launch: %s' % stats
    return None


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (x, y) in enumerate(zip(got, want)):
        assert np.isfinite(x).all(), '%s: observation %d is not finite' % (what, i)
        assert x.shape == y.shape and np.array_equal(x, y), '%s: observation %d differs in %d cells (max |d| %.3g)' % (
            what, i, int((x != y).sum()), float(np.abs(x.astype(np.float64) - y).max()))


_reference = {}


def _shared(key, make):
    """the anchor's answer to one case: computed once, shared, left unchanged"""
    if key not in _reference:
        out = make()
        for x in out[0]:
            x.setflags(write=False)
        _reference[key] = out
    return _reference[key]


# ---- launches of 1, 2, 3, 4, 5, 9 and 33 ticks ---------------------------------------------------------------------------------
# at K = 6 their last periods hold 4, 2, 0 (3 ticks: an exact multiple), 4, 2, 0 and 0 sub-steps: every length a launch of whole
# ticks of 10 sub-steps can end on.  One tick is a plain launch plan (K sub-steps and the shallower launches that complete the tick).
LAUNCHES = [1, 2, 3, 4, 5, 9, 33]


def _launches(monkeypatch, policy, H, W, env, row=None):
    """every count of LAUNCHES as one call — one launch — with the potential read back behind each, the pace behind the fourth"""
    m, st = _model(monkeypatch, policy, H, W, dict(env, FIBHIP_MT_MAX='64', FIBHIP_AHEAD='0'))
    out = []
    for i, n in enumerate(LAUNCHES):
        st.step(n)
        out.append(st.get_state(0).copy())
        if i == 3:
            m.fire_op('s2')
    out.append(st.get_state(-1))
    stats = st.launch_stats()
    why = _ran_as_periods(st, row, stats) if row else None
    st.close()
    return out, stats, why


@pytest.mark.parametrize('H,W', GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_launches_of_every_last_period(gpu_lib, monkeypatch, row, policy, H, W):
    assert [(n * SPT) % row[0] for n in LAUNCHES] == {6: [4, 2, 0, 4, 2, 0, 0]}[row[0]]
    want, s0, _ = _shared(('launches', policy, H, W), lambda: _launches(monkeypatch, policy, H, W, ANCHOR))
    assert s0['mt_ticks'] == 0 and s0['ticks'] == sum(LAUNCHES)
    got, stats, why = _launches(monkeypatch, policy, H, W, _env_of(row), row)
    assert not why, why
    _same(got, want, 'K = %d, %s, %d x %d' % (row[0], policy, H, W))
    # every call of two ticks or more was ONE multi-tick launch
    assert stats['ticks'] == sum(LAUNCHES) and stats['mt_ticks'] == sum(LAUNCHES) - 1 and stats['mt_launches'] == len(LAUNCHES) - 1, stats
    assert stats['gave_up_recovered'] == 0 and stats['ahead_recomputed'] == 0, stats


# ---- a declared series broken by fire_op ---------------------------------------------------------------------------------------
def _declared(monkeypatch, policy, H, W, env, at, row=None):
    """one tick; 40 ticks declared and asked for one call each, 's2' fired behind `at` of them"""
    m, st = _model(monkeypatch, policy, H, W, env)
    st.step(1)
    st.sync()
    st.expect(40)
    for t in range(40):
        if t == at:
            m.fire_op('s2')
        st.step(1)
    out = [st.get_state(-1)]
    stats = st.launch_stats()
    why = _ran_as_periods(st, row, stats) if row else None
    st.close()
    return out, stats, why


@pytest.mark.parametrize('H,W', GRIDS[:1], ids=GRID_IDS[:1])
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('where', ['boundary', 'between'])
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_declared_series_broken_at_and_between_period_boundaries(gpu_lib, monkeypatch, row, where, policy, H, W):
    """the launch that ran ahead holds the state after n ticks only where n ticks end on a period boundary (3 ticks at
    K = 6): there it is stopped, or recomputed if the word came too late — the device's business; after 5 ticks no
    boundary falls on the tick's end, so the launch is cancelled and the ticks recomputed, always"""
    K = row[0]
    at = {6: 3}[K] if where == 'boundary' else 5
    assert ((at * SPT) % K == 0) == (where == 'boundary')
    want, s0, _ = _shared(('declared', policy, H, W, at), lambda: _declared(monkeypatch, policy, H, W, ANCHOR, at))
    got, s, why = _declared(monkeypatch, policy, H, W, _env_of(row), at, row)
    assert not why, why
    _same(got, want, 'K = %d, %s, pace behind %d of 40 declared ticks' % (K, policy, at))
    assert s['ticks'] == s0['ticks'] == 41, (s, s0)
    assert s['ahead_stopped_in_time'] + s['ahead_recomputed'] == 1 and s['gave_up_recovered'] == 0, s
    if where == 'between':
        assert s['ahead_recomputed'] == 1, s


# ---- a read-back inside a running launch ---------------------------------------------------------------------------------------
def _image_into_own_pinned_buffer(st, H, W):
    """the potential read back as image() reads it (fibhip_get_state_direct) into a page-locked buffer of this test's own: the
    binding's pool of such buffers (fib_tf_amd/_lib.py PINNED_MAX) may be held by arrays other tests of the process keep alive,
    and a pageable destination is a plain copy that starts no launch"""
    import ctypes as C
    L, p, n = st._L, C.c_void_p(), H * W
    assert L.fibhip_host_alloc(4 * n, C.byref(p)) == 0 and p.value
    try:
        st._ck(L.fibhip_get_state_direct(st._h, 0, C.cast(p, C.POINTER(C.c_float))))
        return np.array(np.ctypeslib.as_array((C.c_float * n).from_address(p.value)).reshape(H, W))
    finally:
        L.fibhip_host_free(p)


def _read_back(monkeypatch, policy, H, W, env, row=None):
    """12 ticks; 20 ticks declared, image() in front of the first of them — the frame travels inside the launch that runs ahead —
    then the 20 ticks one call each"""
    m, st = _model(monkeypatch, policy, H, W, env)
    st.step(12)
    st.sync()
    st.expect(20)
    before = st.launch_stats()['launches']
    frame = _image_into_own_pinned_buffer(st, H, W)
    started = st.launch_stats()['launches'] - before
    for _ in range(20):
        st.step(1)
    out = [frame, st.get_state(-1)]
    stats = st.launch_stats()
    why = _ran_as_periods(st, row, stats) if row else None
    st.close()
    return out, stats, (why, started)


@pytest.mark.parametrize('H,W', GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_read_back_inside_a_launch(gpu_lib, monkeypatch, row, policy, H, W):
    want, s0, _ = _shared(('read-back', policy, H, W), lambda: _read_back(monkeypatch, policy, H, W, ANCHOR))
    got, s, (why, started) = _read_back(monkeypatch, policy, H, W, _env_of(row), row)
    assert not why, why
    assert started == 1, 'the read-back in front of a declared series started %d launches' % started
    _same(got, want, 'K = %d, %s, %d x %d' % (row[0], policy, H, W))
    assert s['ticks'] == s0['ticks'] == 32 and s['mt_ticks'] == 32, (s, s0)
    assert s['gave_up_recovered'] == 0 and s['ahead_recomputed'] == 0, s


# ---- a launch that gives up ----------------------------------------------------------------------------------------------------
SCRIPT = [1, 9, 'get', ('x', 10), 'get', 33, 'sync', ('x', 7)]


def _script(monkeypatch, policy, H, W, env):
    m, st = _model(monkeypatch, policy, H, W, dict(env, FIBHIP_MT_MAX='64'))
    out = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for op in SCRIPT:
            if isinstance(op, int):
                st.step(op)
            elif op == 'get':
                out.append(st.get_state(0).copy())
            elif op == 'sync':
                st.sync()
            else:
                for _ in range(op[1]):
                    st.step(1)
        out.append(st.get_state(-1))
    stats, tpl, plan = st.launch_stats(), st.ticks_per_launch(), (st.launch_plan(), st.plan_tile())
    st.close()
    return out, stats, (tpl, plan, [w for w in caught if issubclass(w.category, RuntimeWarning)])


@pytest.mark.parametrize('nth', [1, 2, 3])
@pytest.mark.parametrize('policy', POLICIES[:1])
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_period_launch_that_gives_up_is_recovered(gpu_lib, monkeypatch, row, policy, nth):
    """FIBHIP_MT_FAKE_GIVEUP=n: the n-th multi-tick launch finds the give-up word raised in its name and leaves at its first
    period boundary.  The state it started from is restored and its ticks are recomputed as plain ticks: the same bits, every tick
    counted once (the counters of test_counters_across_a_recovery)."""
    H, W = GRIDS[0]
    ticks = sum(op if isinstance(op, int) else op[1] for op in SCRIPT if isinstance(op, int) or op[0] == 'x')
    want, s0, _ = _shared(('script', policy, H, W), lambda: _script(monkeypatch, policy, H, W, ANCHOR))
    free, s1, (tpl1, plan1, w1) = _script(monkeypatch, policy, H, W, _env_of(row))
    assert plan1 == ((row[0], 1), (row[1], row[2], row[3])) and tpl1 > 1 and not w1, (plan1, tpl1)
    _same(free, want, 'K = %d, no give-up' % row[0])
    got, s, (tpl, plan, warned) = _script(monkeypatch, policy, H, W, dict(_env_of(row), FIBHIP_MT_FAKE_GIVEUP=str(nth)))
    _same(got, want, 'K = %d, launch %d gave up' % (row[0], nth))
    fb = (s['gave_up_recovered'], s['ticks_recomputed_after_give_up'])
    assert fb[0] == 1 and tpl == 1, (fb, tpl)
    assert len(warned) == 1 and 'gave up' in str(warned[0].message)
    assert s0['ticks'] == s1['ticks'] == s['ticks'] == ticks, (s0, s1, s)
    assert s0['mt_ticks'] == 0 and 0 < s1['mt_ticks'] <= s1['ticks'] and 0 <= s['mt_ticks'] <= s['ticks'], (s1, s)
    assert s['mt_ticks'] + fb[1] <= s['ticks'] and s['mt_launches'] <= s1['mt_launches'], (s, s1)
    assert s1['gave_up_recovered'] == 0 and s1['ticks_recomputed_after_give_up'] == 0, s1


# ---- the row beside a K = 10 plan: the launches of long declared series only ------------------------------------------------
def _mixed(monkeypatch, policy, H, W, env):
    """what a handle does whose first tick's measurement chose the row (here named by FIBHIP_PERIOD_ROW beside a forced K = 10
    plan, so that small grids take the path): a long declared series (K = 6 launches), a read-back, a short declared series
    whose launch carries a frame (K = 10), a pace, undeclared ticks (K = 10), and a long declared series broken between two
    period boundaries — both tilings alternate on one handle and one array of epoch words"""
    m, st = _model(monkeypatch, policy, H, W, env)
    st.step(1)
    st.sync()
    out = []
    st.expect(130)
    for _ in range(130):
        st.step(1)
    out.append(st.get_state(0).copy())
    st.expect(20)
    before = st.launch_stats()['launches']
    out.append(_image_into_own_pinned_buffer(st, H, W))
    started = st.launch_stats()['launches'] - before
    for _ in range(20):
        st.step(1)
    m.fire_op('s2')
    st.step(9)
    out.append(st.get_state(0).copy())
    st.expect(140)
    for t in range(140):
        if t == 50:
            m.fire_op('s2')
        st.step(1)
    out.append(st.get_state(-1))
    facts = (st.launch_stats(), st.launch_plan(), st.plan_tile(), started)
    st.close()
    return out, facts


@pytest.mark.parametrize('H,W', GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_row_beside_the_plan_runs_long_declared_series_only(gpu_lib, monkeypatch, row, policy, H, W):
    want, (s0, _, _, _) = _shared(('mixed', policy, H, W), lambda: _mixed(monkeypatch, policy, H, W, ANCHOR))
    plain, (s10, plan10, tile10, started10) = _mixed(monkeypatch, policy, H, W, {'FIBHIP_VARIANT': '10,44,25,-3'})
    env = {'FIBHIP_VARIANT': '10,44,25,-3', 'FIBHIP_PERIOD_ROW': _env_of(row)['FIBHIP_VARIANT']}
    got, (s, plan, tile, started) = _mixed(monkeypatch, policy, H, W, env)
    _same(plain, want, 'K = 10 alone, %s, %d x %d' % (policy, H, W))
    _same(got, want, 'K = %d beside K = 10, %s, %d x %d' % (row[0], policy, H, W))
    # both introspection calls name the shape of the long declared launches; without the row, the plan's
    assert (plan10, tile10) == ((10, 1), (44, 25, 3)) and (plan, tile) == ((row[0], 1), (row[1], row[2], row[3])), (plan10, tile10, plan, tile)
    assert started10 == 1 and started == 1
    assert s['ticks'] == s10['ticks'] == s0['ticks'] == 300 and s['mt_ticks'] > 0 and s0['mt_ticks'] == 0, (s, s10, s0)
    assert s['gave_up_recovered'] == 0 and s10['gave_up_recovered'] == 0, (s, s10)
    # the series broken after 50 of 140 ticks: 500 sub-steps are no multiple of 6, so the period launch is cancelled and its
    # ticks recomputed — always; the K = 10 launch of the same calls may be stopped in time
    assert s['ahead_recomputed'] >= 1, s


# ---- the row is never the answer of a rule --------------------------------------------------------------------------------------
@pytest.mark.parametrize('spt,env', [(8, {}), (7, {}), (9, {}), (10, {'FIBHIP_K': '7'}), (10, {'FIBHIP_K': '9'}), (10, {'FIBHIP_VARIANT': '6,99,99,-3'})])
def test_only_its_own_name_takes_the_row(gpu_lib, monkeypatch, spt, env):
    """a tick of 7, 8 or 9 sub-steps, FIBHIP_K above the row's K, or a shape that names no row: build_plan's descent to a
    shallower K passes the row by — the plan starts with the K = 5 strips as it always did, and no launch covers several ticks"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('FIBHIP_AUTOTUNE', '0')
    st = gpu_lib.Stepper(gpu_lib.FENTON4V, 96, 200, 0.1, 1.5, flags=gpu_lib.FAST, steps_per_tick=spt)
    try:
        K, launches = st.launch_plan()
        assert K != 6 and st.plan_tile()[:2] != (52, 21), (st.launch_plan(), st.plan_tile())
        if 'FIBHIP_VARIANT' not in env:
            assert K == 5, (K, launches)
        st.step(3)
        st.sync()
        assert st.launch_stats()['mt_ticks'] == 0 and st.ticks_per_launch() == 1
    finally:
        st.close()
