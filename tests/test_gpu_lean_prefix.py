"""-m gpu: the whole PREFIX of the exchange-period kernel's rim strips (csrc/strip_kernel.inc LEAN_PREFIX).  A strip of the K = 6
row that is fully live for the first n of a period's 6 sub-steps runs those n sub-steps without the row bookkeeping and the rest
with it; a strip that is whole for all 6 takes the lean loop as before, and a launch's short last period takes the bookkeeping
throughout.  None of that may change a bit.

Every case names the row with FIBHIP_PERIOD_ROW beside a forced K = 10 plan (so that grids this small run several ticks per
launch at all), plays three declared series on one handle — 3 ticks, 128 ticks, 1 tick, one call per tick — and compares every
state array behind each series bitwise with the same calls under FIBHIP_MT=0.  Beside a plan, the row runs the launches of
declarations of 128 ticks or more only (csrc/sched.inc mt_variant): the 128 ticks are ONE launch of 213 whole periods and a short
last period of 2 sub-steps; the 3 ticks are a K = 10 launch and the single tick a plain one, as on every handle whose measurement
chose the row.  test_forced_row_launches_of_whole_and_short_periods therefore forces the row (FIBHIP_VARIANT), which then runs
EVERY multi-tick launch: 3 ticks are five whole periods, 4 ticks six periods and a short last one of 4 sub-steps, 2 ticks three
periods and a short last one of 2.

Grids (width x height, tiles of 52 x 21): 104 x 42 — 2 x 2 tiles, every strip class with the box open above and below;
104 x 30 — a second tile row of 9 rows, strips whose rows end inside them (prefix 0); 52 x 21 — one tile, nothing open, every
strip whole; 156 x 63 — a middle tile whose eight neighbours all exist."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = ('FIBHIP_MT', 'FIBHIP_MT_MAX', 'FIBHIP_MT_FAKE_GIVEUP', 'FIBHIP_AHEAD', 'FIBHIP_MT_WAIT_MS', 'FIBHIP_MT_IDS', 'FIBHIP_VARIANT',
       'FIBHIP_AUTOTUNE', 'FIBHIP_K', 'FIBHIP_ZEROPAD', 'FIBHIP_PERIOD_ROW')
ROWS = ['6,52,21,-2']
GRIDS = [(104, 42), (104, 30), (52, 21), (156, 63)]            # width, height
SERIES = [3, 128, 1]                                            # declared ticks (one tick is 10 sub-steps)
SPT = 10
PLAN = '10,44,25,-3'


def _model(monkeypatch, policy, hole, W, H, env):
    from fib_tf_amd.fenton import Fenton4v
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = {'width': W, 'height': H, 'dt': 0.1, 'dt_per_plot': SPT, 'duration': 1000, 'skip': False, 'fast_math': policy == 'fast',
           'diff': 1.5}
    m = Fenton4v(cfg)
    if hole:
        m.add_hole_to_phase_field(W // 2 + 3, H // 2 - 2, 5)
    m.define()
    return m, m._stepper


def _play(monkeypatch, policy, hole, W, H, env, series, declared=True):
    """the series one after the other on one handle, one call per tick; every state array behind each of them"""
    m, st = _model(monkeypatch, policy, hole, W, H, env)
    st.step(1)
    st.sync()
    out = []
    for n in series:
        if declared:
            st.expect(n)
            for _ in range(n):
                st.step(1)
        else:
            st.step(n)
        out.append(st.get_state(-1))
    facts = (st.launch_stats(), st.launch_plan(), st.plan_tile())
    st.close()
    return out, facts


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (x, y) in enumerate(zip(got, want)):
        assert np.isfinite(x).all(), '%s: series %d is not finite' % (what, i)
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), '%s: series %d differs in %d cells (max |d| %.3g)' % (
            what, i, int((x != y).sum()), float(np.abs(x.astype(np.float64) - y).max()))
        assert float(x[0].max()) > 0.1,'%s: series %d holds no excited cell' % (what, i)


_reference = {}


def _anchor(monkeypatch, key, policy, hole, W, H, series, declared):
    """the same calls with FIBHIP_MT=0: computed once per case, shared, left unchanged"""
    if key not in _reference:
        out, (stats, _, _) = _play(monkeypatch, policy, hole, W, H, {'FIBHIP_VARIANT': PLAN, 'FIBHIP_MT': '0'}, series, declared)
        assert stats['mt_ticks'] == 0 and stats['ticks'] == 1 + sum(series), stats
        for x in out:
            x.setflags(write=False)
        _reference[key] = out
    return _reference[key]


@pytest.mark.parametrize('W,H', GRIDS, ids=['%dx%d' % g for g in GRIDS])
@pytest.mark.parametrize('hole', [True, False], ids=['hole', 'plain'])
@pytest.mark.parametrize('policy', ['fast', 'exact'])
@pytest.mark.parametrize('row', ROWS)
def test_declared_series_beside_the_plan(gpu_lib, monkeypatch, row, policy, hole, W, H):
    want = _anchor(monkeypatch, ('beside', policy, hole, W, H), policy, hole, W, H, SERIES, True)
    got, (stats, plan, tile) = _play(monkeypatch, policy, hole, W, H, {'FIBHIP_VARIANT': PLAN, 'FIBHIP_PERIOD_ROW': row}, SERIES)
    K, TX, TY, NT = (int(x) for x in row.split(','))
    assert plan == (K, 1) and tile == (TX, TY, -NT), 'row %s did not run the long declared series: plan %s, tile %s' % (row, plan, tile)
    _same(got, want, 'row %s, %s, %s, %d x %d' % (row, policy, 'hole' if hole else 'no hole', W, H))
    assert stats['ticks'] == 1 + sum(SERIES), stats
    assert stats['gave_up_recovered'] == 0 and stats['mt_ticks'] > 0, stats
    assert stats['mt_ticks'] >= 128, 'the 128 declared ticks did not run in multi-tick launches: %s' % stats


FORCED = [3, 4, 2]                                              # ticks per call: last periods of 0, 4 and 2 sub-steps at K = 6


@pytest.mark.parametrize('W,H', GRIDS[:2], ids=['%dx%d' % g for g in GRIDS[:2]])
@pytest.mark.parametrize('policy', ['fast', 'exact'])
@pytest.mark.parametrize('row', ROWS)
def test_forced_row_launches_of_whole_and_short_periods(gpu_lib, monkeypatch, row, policy, W, H):
    assert [(n * SPT) % int(row.split(',')[0]) for n in FORCED] == [0, 4, 2]
    want = _anchor(monkeypatch, ('forced', policy, W, H), policy, True, W, H, FORCED, False)
    got, (stats, plan, tile) = _play(monkeypatch, policy, True, W, H, {'FIBHIP_VARIANT': row, 'FIBHIP_AHEAD': '0'}, FORCED, declared=False)
    K, TX, TY, NT = (int(x) for x in row.split(','))
    assert plan == (K, 1) and tile == (TX, TY, -NT), (plan, tile)
    _same(got, want, 'row %s forced, %s, %d x %d' % (row, policy, W, H))
    # every call was ONE multi-tick launch of the row
    assert stats['mt_ticks'] == sum(FORCED) and stats['mt_launches'] == len(FORCED), stats
    assert stats['gave_up_recovered'] == 0 and stats['ahead_recomputed'] == 0, stats
