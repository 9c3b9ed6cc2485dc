"""-m gpu: EVERY row of the kernel variant table (csrc/launch.hpp g_variants), enumerated from the built library at run
time (fib_tf_amd._lib.variants), forced, confirmed to have run, and compared

  (a) bit for bit with the one-sub-step-per-launch kernel (FIBHIP_VARIANT=1,64,4,256, FIBHIP_MT=0; Courtemanche on
      aggregates: FIBHIP_NO_MULTI=1 FIBHIP_NO_LAZY=1) on the same state and call sequence — the contract the plan
      selection by measurement (csrc/plan.inc autotune / autotune_multi) rests on, and
  (b) that anchor with the CPU oracle, once per (model, mode, policy, phase, grid), at the tolerances the tests of
      tests/test_gpu_parity.py already use (named where they are applied).

Grids are built from each row's own tile TX x TY: G1 = (2 TY + 1) x (2 TX + 1) — 3 x 3 tiles, the last row and column of
tiles one cell thick, so a border cell's inward neighbours lie in another tile — and G2 = (3 TY) x (3 TX), an exact fit
with an interior tile that has all eight neighbours.  States are seeded and differ in every cell.  No list of shapes is
kept here: a row added to the table is tested without anyone touching this file, and a forcing string that names no row
makes the row fail with "shape not taken" (build_plan would otherwise fall back to another row of that K in silence).

tests/test_variant_table_cpu.py checks the table itself, the share of cells left out near Courtemanche's singular
potentials, and that comparison (b) would see a tile-seam error (a mutation of the oracle's own step)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FENTON, BR, COURT, COURT_US, FENTON_ZP, COURT_AGG = 0, 1, 2, 3, 100, 101
POLICIES = ['fast', 'exact']
ANCHOR = '1,64,4,256'
# every variable that moves the plan: PLAN_ENV of tests/test_gpu_frames.py and the ones below
EXTRA_ENV = ('FIBHIP_K', 'FIBHIP_COURT_AGG', 'FIBHIP_NO_MULTI', 'FIBHIP_NO_LAZY', 'FIBHIP_COURT_MULTI2', 'FIBHIP_COURT_MULTI3')

FENTON_DT, FENTON_DIFF = 0.1, 1.2
BR_DIFF = COURT_DIFF = 0.809
# tests/test_gpu_parity.py STEP_TOL: the per-sub-step bounds of the two policies.  The fast policy's oracle bound here is
# n_substeps * FAST_STEP_TOL, summed linearly: a ceiling, deliberately loose — sharpness comes from (a) and the exact policy
FAST_STEP_TOL = 3e-5
# test_court_single_step: cells within 0.06 mV of a removable singularity of calc_inter are left out of the ORACLE
# comparison (never out of the bit comparison); at most NEAR_CAP of a grid's cells may be
SINGULAR = [-10.0001, -10.0, 7.9, -47.13, -14.1, 3.3328, 19.9]
NEAR_CAP = 0.03
COURT_STEP_SCALES = {'V': 150.0, '_Na_i_': 3.0, '_K_i_': 15.0, '_Ca_i_': 1e-3, '_Ca_rel_': 1.5, '_Ca_up_': 1.0}   # test_court_single_step


def grids_of(r):
    TX, TY = r['TX'], r['TY']
    return [(2 * TY + 1, 2 * TX + 1), (3 * TY, 3 * TX)]


def shape_of(r):
    return (r['K'], r['TX'], r['TY'], r['NT'])


def variant_env(r):
    """FIBHIP_VARIANT of a row: the ONE place a forcing string is made"""
    return '%d,%d,%d,%d' % shape_of(r)


def multi_env(r):
    """FIBHIP_COURT_MULTI2 / FIBHIP_COURT_MULTI3 of a row"""
    return '%d,%d,%d' % (r['TX'], r['TY'], r['NT'])


def clear_env(monkeypatch, **env):
    from test_gpu_frames import PLAN_ENV
    for k in PLAN_ENV + EXTRA_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- states ----------------------------------------------------------------------------------------------------------
def fenton_state(H, W):
    """drawn as test_fenton_tiny_and_skinny_grids draws it (phase field: uniform(0.3, 1.0))"""
    rng = np.random.default_rng(H * 1000 + W)
    st = np.stack([rng.uniform(-0.05, 1.05, (H, W)), rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W)),
                   rng.uniform(0, 1, (H, W))]).astype(np.float32)
    return st, rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)


def br_state(H, W):
    """drawn as test_br_vs_oracle_random_state draws it"""
    rng = np.random.default_rng(7 + H * 1000 + W)
    st = np.empty((8, H, W), np.float32)
    st[0] = rng.uniform(-85, 25, (H, W))
    st[1] = np.exp(rng.uniform(np.log(1e-7), np.log(1e-5), (H, W)))
    st[2:] = rng.uniform(1e-5, 0.99999, (6, H, W))
    return st, rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)


def court_state(H, W, us=False):
    """drawn as _court_run draws it: the resting state with the potential spread over 65 mV"""
    from fib_tf_amd.court import INITIAL
    rng = np.random.default_rng(11 + H * 1000 + W)
    init = np.empty((21 + (1 if us else 0), H, W), np.float32)
    for i, (_, v) in enumerate(INITIAL):
        init[i] = v
    if us:
        init[21] = 0.72                                       # court_ultra.py: the `_us_` gate's steady state
    init[0] += rng.uniform(-5, 60, (H, W)).astype(np.float32)
    return init, rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)


def court_near_singular(V):
    """cells whose potential, as the step sees it (border cells take their inward neighbour's: enforce_boundary), lies
    within 0.06 mV of a singular potential"""
    V = np.asarray(V, np.float32)
    Vb = np.pad(V[1:-1, 1:-1], 1, mode='edge')
    near = np.zeros(V.shape, bool)
    for s in SINGULAR:
        near |= np.abs(Vb - np.float32(s)) < 0.06
        near |= np.abs(V - np.float32(s)) < 0.06
    return near


_BR_TABLE = []


def br_table():
    if not _BR_TABLE:
        from fib_tf_amd.br import BeelerReuter
        _BR_TABLE.append(BeelerReuter({'height': 8, 'width': 8, 'cheby': True})._table32())
    return _BR_TABLE[0]


# ---- one play on one handle -------------------------------------------------------------------------------------------
def play(lib, model, flags, H, W, diff, state, phi, script, consts=None, library=None):
    """the calls of `script` on a fresh handle: an int = step(n), 'all' = whole-state read-back, 'get' = read-back of array
    0, 'pace', 'slow', 'sync', 'tb' / 'te' = time_begin / time_end (the launch count goes to facts['launches']).
    Returns (observations + final state, facts about what ran)"""
    st = lib.Stepper(model, H, W, 0.1, diff, flags=flags, library=library)
    try:
        if consts is not None:
            st.set_consts(consts)
        if phi is not None:
            st.set_phase(phi)
        st.set_state(-1, state)
        facts = {'tile': st.plan_tile(), 'launches': []}
        if model in (FENTON, BR):
            facts['K'] = st.launch_plan()[0]                  # (sub-steps of the plan's first launch)
        out = []
        for op in script:
            if op == 'all':
                out.append(st.get_state(-1))
            elif op == 'get':
                out.append(st.get_state(0).copy())
            elif op == 'pace':
                if model == FENTON:
                    st.pace(H // 4, H // 4 + 5, W // 3, W // 3 + 6, 1.0, 0.0)
                else:
                    st.pace(0, max(1, H // 2), 0, max(1, W // 2), 10.0, -100.0)
            elif op == 'slow':
                st.step_slow()
            elif op == 'sync':
                st.sync()
            elif op == 'tb':
                st.time_begin()
            elif op == 'te':
                facts['launches'].append(st.time_end()[1])
            else:
                st.step(op)
        out.append(st.get_state(-1))
        facts['tpl'] = st.ticks_per_launch()
        facts['stats'] = st.launch_stats()
        facts['tile_end'] = st.plan_tile()
    finally:
        st.close()
    for x in out:
        assert np.isfinite(x).all(), 'non-finite values'
    return out, facts


def plan_only(lib, model, flags, H, W, diff, phi):
    """(tile of the plan, ticks per launch) of a handle that launches nothing"""
    st = lib.Stepper(model, H, W, 0.1, diff, flags=flags)
    try:
        if phi is not None:
            st.set_phase(phi)
        return st.plan_tile(), st.ticks_per_launch()
    finally:
        st.close()


def same_bits(got, want):
    """None, or where two lists of observations differ"""
    for i, (x, y) in enumerate(zip(got, want)):
        if not np.array_equal(x, y):
            d = np.abs(x.astype(np.float64) - y) if x.shape == y.shape else None
            if d is None:
                return 'observation %d: shapes %s and %s' % (i, x.shape, y.shape)
            cell = np.unravel_index(int(np.argmax(d)), d.shape)
            return 'observation %d differs from the anchor in %d cells, max |d| %.3g at %s' % (i, int((x != y).sum()), float(d.max()), cell)
    return None


def took(facts, r):
    """None, or why the forced row is not what the plan launches first"""
    want = (r['TX'], r['TY'], -r['NT'])
    if facts['tile'] != want or facts['tile_end'] != want or facts.get('K', r['K']) != r['K']:
        return 'shape not taken: the plan runs K = %s in tile %s, not K = %d in %s' % (facts.get('K', '?'), facts['tile'], r['K'], want)
    return None


class Worst:
    """largest oracle error per key, as a fraction of its bound, with the cell: printed for the record, asserted by check()"""

    def __init__(self):
        self.rows = {}

    def add(self, key, got, want, tol, scale, where, mask=None):
        d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
        if mask is not None:
            d = np.where(mask, 0.0, d)                        # (broadcasts over a stack of arrays)
        err = float(d.max())
        cell = tuple(int(i) for i in np.unravel_index(int(np.argmax(d)), d.shape))
        cur = self.rows.get(key)
        if cur is None or err / (tol * scale) > cur[0] / (cur[1] * cur[2]):
            self.rows[key] = (err, tol, scale, where, cell)

    def add_ill(self, key, excess, tol, scale, where, mask):
        """the cells add() left out (`mask`): `excess` = how far the value lies outside the oracle's own envelope there,
        less three times the envelope's width — test_court_single_step's margin — which the ordinary bound must cover"""
        if mask.any():
            d = np.where(mask, np.asarray(excess, np.float64), -np.inf)
            cell = tuple(int(i) for i in np.unravel_index(int(np.argmax(d)), d.shape))
            err = max(float(d.max()), 0.0)
            key += ' [ill-conditioned cells, beyond 3 x the oracle\'s own width]'
            cur = self.rows.get(key)
            if cur is None or err / (tol * scale) > cur[0] / (cur[1] * cur[2]):
                self.rows[key] = (err, tol, scale, where, cell)

    def check(self):
        bad = []
        for key, (err, tol, scale, where, cell) in sorted(self.rows.items()):
            print('oracle %-44s max |d| %.3e  bound %.1e * %g  (%s, cell %s)' % (key, err, tol, scale, where, cell))
            if not err <= tol * scale:
                bad.append('%s: anchor against the oracle: %.3e > %.1e * %g (%s, cell %s)' % (key, err, tol, scale, where, cell))
        return bad


def report(ran, rows, failures, n_mt=None):
    """`ran` = the rows whose forced plays all completed (None: a case that forces no row, anchors only)"""
    want = {shape_of(r) + (r['mode'],) for r in rows}
    if ran is not None:
        print('rows enumerated %d, run %d%s' % (len(want), len(ran), '' if n_mt is None else ', as multi-tick launches %d' % n_mt))
    assert not failures, '%d failure(s):\n%s' % (len(failures), '\n'.join(failures))
    assert ran is None or ran == want, 'rows enumerated but not run: %s' % sorted(want ^ ran)


# ---------------------------------------------------------------------------------------------------------------------
# Fenton 4v and its zero-padded-Laplacian form; Beeler-Reuter on the stock and on the specialised library
# ---------------------------------------------------------------------------------------------------------------------
SINGLE = [1, 'all', 1]                          # two ticks, one launch plan each: sub0 > 0 in the later launches, buffers flip
MULTI = [1, 5, 'pace', 3, 'get', 4]             # has_mt rows: launches of several ticks, a pace and a read-back between them


def run_tile_rows(lib, monkeypatch, rows, model, flags, diff, state_of, phase, consts, library, anchors, oracle, tag):  # noqa: C901
    """every row of `rows` on its two grids, single-tick and (has_mt) multi-tick, against the anchor of the same grid;
    `anchors`: cache {(H, W): (single, multi)}.  With `oracle(H, W, state, phi, single_obs)` given, the anchor of every
    grid is compared with the oracle through it INSTEAD (comparison (b), a test of its own).
    Returns (rows run, rows run as multi-tick launches, failures)"""
    ran, n_mt, failures, seen = set(), 0, [], set()
    for r in rows:
        label = '%s %s' % (tag, variant_env(r))
        try:
            for H, W in grids_of(r):
                state, phi = state_of(H, W)
                phi = phi if phase else None
                if (H, W) not in anchors:
                    clear_env(monkeypatch, FIBHIP_VARIANT=ANCHOR, FIBHIP_MT='0')
                    a1, f1 = play(lib, model, flags, H, W, diff, state, phi, SINGLE, consts)
                    a2, f2 = play(lib, model, flags, H, W, diff, state, phi, MULTI, consts)
                    assert f1['tile'] == (64, 4, -256) and f2['stats']['mt_ticks'] == 0, 'the anchor is not the K = 1 kernel'
                    anchors[(H, W)] = (a1, a2)
                a1, a2 = anchors[(H, W)]
                if oracle is not None:                            # the anchor against the oracle: nothing else runs
                    if (H, W) not in seen:
                        seen.add((H, W))
                        oracle(H, W, state, phi, a1)
                    continue
                clear_env(monkeypatch, FIBHIP_VARIANT=variant_env(r), FIBHIP_MT='0')
                got, facts = play(lib, model, flags, H, W, diff, state, phi, SINGLE, consts, library)
                why = took(facts, r) or same_bits(got, a1)
                if not why and facts['stats']['mt_ticks']:
                    why = 'FIBHIP_MT=0 but %d ticks ran in multi-tick launches' % facts['stats']['mt_ticks']
                if why:
                    failures.append('%s on %dx%d, one launch plan per tick: %s' % (label, H, W, why))
                if r['has_mt']:
                    clear_env(monkeypatch, FIBHIP_VARIANT=variant_env(r))
                    got, facts = play(lib, model, flags, H, W, diff, state, phi, MULTI, consts, library)
                    why = took(facts, r) or same_bits(got, a2)
                    if not why and not (facts['tpl'] > 1 and facts['stats']['mt_ticks'] > 0):
                        why = 'the multi-tick path was not taken (ticks per launch %d, %d ticks in multi-tick launches)' % (
                            facts['tpl'], facts['stats']['mt_ticks'])
                    if why:
                        failures.append('%s on %dx%d, several ticks per launch: %s' % (label, H, W, why))
            n_mt += 1 if r['has_mt'] else 0
            ran.add(shape_of(r) + (r['mode'],))                   # (its forced plays have all completed)
        except Exception as e:                                    # (every failing row is reported, not the first one)
            failures.append('%s: %s: %s' % (label, type(e).__name__, e))
    return (ran if oracle is None else None), n_mt, failures


# (fenton_simple.py has no phase field, so the oracle has none for the zero-padded form: no 'oracle' case for its phase = 1 rows)
FENTON_CASES = [(m, pol, ph, what) for m in (FENTON, FENTON_ZP) for pol in POLICIES for ph in (1, 0) for what in ('bits', 'oracle')
                if not (m == FENTON_ZP and ph and what == 'oracle')]


@pytest.mark.parametrize('model,policy,phase,what', FENTON_CASES,
                         ids=['%s-%s-%d-%s' % ('fenton_zeropad' if c[0] == FENTON_ZP else 'fenton', c[1], c[2], c[3]) for c in FENTON_CASES])
def test_fenton_rows(gpu_lib, orc, monkeypatch, model, policy, phase, what):
    """what = 'bits': every row against the anchor (a); 'oracle': the anchor of every grid against the oracle (b).
    fenton_simple.py has no phase field, so the oracle has none for the zero-padded form: its phase = 1 rows have the
    bit comparison only, and no 'oracle' case."""
    fast = 1 if policy == 'fast' else 0
    rows = [r for r in gpu_lib.variants() if (r['model'], r['fast'], r['phase']) == (model, fast, phase)]
    assert rows and all(r['mode'] == 0 for r in rows)
    flags = (gpu_lib.FAST if fast else 0) | (gpu_lib.ZEROPAD if model == FENTON_ZP else 0)
    worst = Worst()
    # test_fenton_tiny_and_skinny_grids: 3e-6 at 20 sub-steps under the rounding-faithful policy
    tol = 20 * FAST_STEP_TOL if fast else 3e-6

    def oracle(H, W, state, phi, obs):
        ref = state.copy()
        if model == FENTON:
            orc.fenton_run(ref, FENTON_DT, FENTON_DIFF, phi, 20)
        else:
            assert phi is None
            orc.fenton_simple_run(ref, FENTON_DT, FENTON_DIFF, 20)
        worst.add('fenton%s %s phase=%d' % ('_zeropad' if model == FENTON_ZP else '', policy, phase), obs[-1], ref, tol, 1.0, '%dx%d' % (H, W))

    ran, n_mt, failures = run_tile_rows(gpu_lib, monkeypatch, rows, FENTON, flags, FENTON_DIFF, fenton_state, phase, None, None,
                                        _FENTON_ANCHORS.setdefault((model, fast, phase), {}), oracle if what == 'oracle' else None,
                                        'fenton%s %s phase=%d' % ('_zeropad' if model == FENTON_ZP else '', policy, phase))
    report(ran, rows, failures + worst.check(), n_mt)


_FENTON_ANCHORS = {}


@pytest.mark.parametrize('phase', [1, 0])
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('build', ['stock', 'specialised', 'oracle'])
def test_br_rows(gpu_lib, orc, monkeypatch, build, policy, phase):
    """both gate forms (mode 0 direct, 1 Chebyshev) x the `skip` multirate schedule: the sub-step index restarts with every
    tick, in plans that mix rows as 2+2+1 and 3+2 too.  The specialised build (the Chebyshev table compiled in) runs the
    rows of ITS table against the stock library's anchor.  build = 'oracle': the stock library's anchors against the oracle
    and nothing else (comparison (b)).
    Cells where the oracle itself is ill-conditioned are bounded by its own envelope instead (oracle_error_bar)."""
    from fib_tf_amd import br
    fast = 1 if policy == 'fast' else 0
    library = br.specialised_library(br_table()) if build == 'specialised' else None
    assert (library is not None) == (build == 'specialised')
    against_oracle = build == 'oracle'              # comparison (b): the stock library's anchors against the oracle
    table = [r for r in gpu_lib.variants(library) if (r['model'], r['fast'], r['phase']) == (BR, fast, phase)]
    assert {r['mode'] for r in table} == {0, 1}
    worst = Worst()
    ran, n_mt, failures = set(), 0, []
    for mode in (0, 1):
        rows = [r for r in table if r['mode'] == mode]
        consts = br_table() if mode == 1 else None
        # test_br_vs_oracle_random_state: one tick, 1e-5 direct, 5e-5 Chebyshev, on V / 120 mV, gates / 1, C / 1e-5
        tol = 5 * FAST_STEP_TOL if fast else (5e-5 if mode == 1 else 1e-5)
        for skip in (False, True):
            flags = (gpu_lib.FAST if fast else 0) | (gpu_lib.CHEBY if mode == 1 else 0) | (gpu_lib.SKIP if skip else 0)
            key = 'br %s %s skip=%d phase=%d' % ('cheby' if mode else 'direct', policy, skip, phase)

            def oracle(H, W, state, phi, obs):
                ref, ill, lo, hi = br_reference(orc, state, phi, consts, skip, 5e-5 if mode == 1 else 1e-5)
                got = obs[0].astype(np.float64)
                excess = np.maximum(lo - got, got - hi) - 3.0 * (hi - lo)
                for name, sl, scale in ((' V', slice(0, 1), 120.0), (' gates', slice(2, 8), 1.0), (' C', slice(1, 2), 1e-5)):
                    worst.add(key + name, got[sl], ref[sl], tol, scale, '%dx%d' % (H, W), mask=ill)
                    worst.add_ill(key + name, excess[sl], tol, scale, '%dx%d' % (H, W), ill)

            a, b, c = run_tile_rows(gpu_lib, monkeypatch, rows, BR, flags, BR_DIFF, br_state, phase, consts, library,
                                    _BR_ANCHORS.setdefault((fast, phase, mode, skip), {}), oracle if against_oracle else None,
                                    '%s [%s]' % (key, build))
            ran = None if a is None else ran | a
            n_mt += b
            failures += c
    report(ran, table, failures + worst.check(), n_mt)


def oracle_error_bar(orc, run, state, bounds):
    """(the oracle's answer, the cells where the oracle ITSELF has no answer to within the bounds, the lower and the upper
    envelope of its answers).  `run(state)` is the oracle's restatement of the play; `bounds[v]` the absolute bound of
    array v.  The reference's float32 formulas are 0/0 forms at some potentials (Beeler-Reuter: -47 mV alpha_m, -23 i_K1,
    -77 i_x1; its Chebyshev fits of the time constants pass close to zero near -84 mV, where 1/tau turns one ulp of V into
    1 % of a gate; Courtemanche: SINGULAR), and a state as rough as the seeded ones carries cells through them inside a
    tick's sub-steps or along the ticks of a play.  As test_court_single_step does (court_envelope_samples), the oracle's
    own error bar is taken from the oracle: the same play with exp() moved by -1 / +1 ulp and with every potential moved
    by -2 .. +2 float32 neighbours.  A cell where those seven answers spread by more than the bound in any array is not
    compared with the one answer but, as that test does, with their envelope: the device value must lie inside it widened by
    three times its own width plus the ordinary bound (Worst.add_ill).  No cell goes unchecked; at most NEAR_CAP of a
    grid's cells may be treated so."""
    runs = [run(state.copy())]
    for k in (-2, -1, 1, 2):
        moved = state.copy()
        for _ in range(abs(k)):
            moved[0] = np.nextafter(moved[0], np.float32(np.inf if k > 0 else -np.inf))
        runs.append(run(moved))
    try:
        for u in (-1, 1):
            orc.set_exp_ulps(u)
            runs.append(run(state.copy()))
    finally:
        orc.set_exp_ulps(0)
    r = np.stack(runs).astype(np.float64)
    lo, hi = r.min(axis=0), r.max(axis=0)
    ill = (hi - lo > np.asarray(bounds, np.float64)[:, None, None]).any(axis=0)
    assert ill.mean() <= NEAR_CAP, '%.2f %% of the cells are ill-conditioned in the oracle itself' % (100 * ill.mean())
    return runs[0], ill, lo, hi


def br_reference(orc, state, phi, consts, skip, rel):
    """oracle_error_bar of one tick, at the rounding-faithful policy's bound `rel` (the set of cells does not depend on the
    policy under test)"""
    return oracle_error_bar(orc, lambda st: orc.br_run(st, 0.1, BR_DIFF, phi, consts, skip, 1), state,
                            [rel * 120.0, rel * 1e-5] + [rel] * 6)


_BR_ANCHORS = {}                # the stock library's anchors, shared by the two builds: {(fast, phase, mode, skip): {(H, W): ...}}


# ---------------------------------------------------------------------------------------------------------------------
# Courtemanche: the plain kernels (both policies; FIBHIP_COURT_AGG=0 keeps the fast policy on them), court_ultra's
# 22-variable model, and the kernels on aggregates with their launches of two and three ticks
# ---------------------------------------------------------------------------------------------------------------------
MODE_FAST, MODE_ALL, MODE_FASTSLOW = 0, 2, 3                         # csrc/models.hpp CourtT
COURT_PLAY = [1, 'all', 'tb', 1, 'slow', 'te', 1]                    # a tick; a tick with 'slow' right behind it; a tick
COURT_PLAY_ALL = [1, 'all', 1]                                       # (FIBHIP_ALLVARS handles have no 'slow')
AGG_PLAY = [1, 'slow', 'sync', 'tb', 5, 'sync', 4, 'slow', 3, 'te']  # launches of 3 and of 2 ticks, a tick fused with 'slow'


def agg_play_oracle(orc, st, phi):
    """AGG_PLAY on the oracle: 13 ticks, 'slow' behind the first and the tenth"""
    for tick0, n in ((0, 1), (1, 8), (10, 1), (1, 3)):          # (court_run fires 'slow' behind a tick whose index is 0 mod 10)
        orc.court_run(st, 0.1, COURT_DIFF, phi, False, tick0, n)
    return st


def fuses_slow(H, W):
    """build_plan's rule for the launch that carries a tick AND the 'slow' behind it (64 x 4 tiles: every border cell's
    inward neighbour inside the border cell's own tile)"""
    return (H - 1) % 4 != 0 and (W - 1) % 64 != 0


def court_oracle(orc, worst, key, names, state, phi, got, run, tol):
    ref = state.copy()
    run(ref, phi)
    near = court_near_singular(state[0])
    assert near.mean() <= NEAR_CAP, '%.2f %% of the cells lie near a singular potential' % (100 * near.mean())
    for i, k in enumerate(names):
        worst.add('%s %s' % (key, k), got[i], ref[i], tol, COURT_STEP_SCALES.get(k, 1.0), '%dx%d' % state.shape[1:], mask=near)


@pytest.mark.parametrize('phase', [1, 0])
@pytest.mark.parametrize('policy', POLICIES)
def test_court_rows(gpu_lib, orc, monkeypatch, policy, phase):
    fast = 1 if policy == 'fast' else 0
    rows = [r for r in gpu_lib.variants() if r['model'] in (COURT, COURT_US) and (r['fast'], r['phase']) == (fast, phase)]
    assert {(r['model'], r['mode']) for r in rows} == {(COURT, MODE_FAST), (COURT, MODE_ALL), (COURT, MODE_FASTSLOW), (COURT_US, MODE_ALL)}
    assert all(r['K'] == 1 and r['kind'] == gpu_lib.MK_TICK for r in rows)
    worst = Worst()
    # test_court_single_step: one tick, 6e-6 * scale under the rounding-faithful policy
    tol = FAST_STEP_TOL if fast else 6e-6
    anchors, failures, ran = {}, [], set()
    for r in rows:
        label = 'court model %d mode %d %s phase=%d %s' % (r['model'], r['mode'], policy, phase, variant_env(r))
        us = r['model'] == COURT_US
        allv = r['mode'] == MODE_ALL
        flags = (gpu_lib.FAST if fast else 0) | (gpu_lib.ALLVARS if allv and not us else 0)
        script = COURT_PLAY_ALL if allv else COURT_PLAY
        try:
            for H, W in grids_of(r):
                state, phi = court_state(H, W, us)
                phi = phi if phase else None
                akey = (r['model'], allv, H, W)
                if akey not in anchors:
                    clear_env(monkeypatch, FIBHIP_VARIANT=ANCHOR, FIBHIP_MT='0', FIBHIP_COURT_AGG='0', FIBHIP_NO_LAZY='1')
                    a, f = play(gpu_lib, r['model'], flags, H, W, COURT_DIFF, state, phi, script)
                    assert f['tile'] == (64, 4, -256) and f['launches'] in ([], [2]), 'the anchor is not one launch per operation'
                    anchors[akey] = a
                    names = list(orc.COURT_VARS) + (['_us_'] if us else [])
                    if us:
                        run = lambda ref, phi: orc.court_ultra_us_run(ref, 0.1, COURT_DIFF, phi, False, 1)
                    elif allv:
                        run = lambda ref, phi: orc.court_ultra_run(ref, 0.1, COURT_DIFF, phi, False, 1)
                    else:
                        run = lambda ref, phi: orc.court_run(ref, 0.1, COURT_DIFF, phi, False, 1, 1)
                    court_oracle(orc, worst, 'court%s %s phase=%d' % ('_us' if us else '_all' if allv else '', policy, phase), names, state, phi,
                                 a[0], run, tol)
                env = dict(FIBHIP_VARIANT=variant_env(r), FIBHIP_MT='0', FIBHIP_COURT_AGG='0')
                if r['mode'] != MODE_FASTSLOW:
                    env['FIBHIP_NO_LAZY'] = '1'
                clear_env(monkeypatch, **env)
                got, facts = play(gpu_lib, r['model'], flags, H, W, COURT_DIFF, state, phi, script)
                why = took(facts, r) or same_bits(got, anchors[akey])
                if not why and not allv:
                    # the launch count says which kernels ran: the fused tick + 'slow' where the rule allows it (G2), else two
                    want = 1 if r['mode'] == MODE_FASTSLOW and fuses_slow(H, W) else 2
                    if facts['launches'] != [want]:
                        why = 'a tick and its \'slow\' took %s launches, not %d' % (facts['launches'], want)
                if why:
                    failures.append('%s on %dx%d: %s' % (label, H, W, why))
            if r['mode'] == MODE_FASTSLOW:
                assert [fuses_slow(H, W) for H, W in grids_of(r)] == [False, True]
            ran.add(shape_of(r) + (r['mode'],) + (r['model'],))   # (its forced plays have all completed)
        except Exception as e:
            failures.append('%s: %s: %s' % (label, type(e).__name__, e))
    want = {shape_of(r) + (r['mode'],) + (r['model'],) for r in rows}
    print('rows enumerated %d, run %d' % (len(want), len(ran)))
    failures += worst.check()
    assert not failures, '%d failure(s):\n%s' % (len(failures), '\n'.join(failures))
    assert ran == want, 'rows enumerated but not run: %s' % sorted(want ^ ran)


@pytest.mark.parametrize('what', ['bits', 'plain1', 'plain2', 'plain3'])
@pytest.mark.parametrize('phase', [1, 0])
def test_court_aggregate_rows(gpu_lib, orc, monkeypatch, phase, what):
    """Courtemanche on aggregates (fast policy): its K = 1 rows, the fused tick + 'slow', and every shape of the launches
    of three and of two ticks.  A trace forces one tick per launch (csrc/sched.inc), so what ran is confirmed through
    plan_tile() — the shape of the deepest multi-tick plan — ticks_per_launch() and the launch count of the play: with
    FIBHIP_COURT_MULTI3 forced the plan of three ticks is the row and the launches of two take the table's first K = 2
    row; with FIBHIP_COURT_MULTI2 forced the three-tick launches take the table's first K = 3 row, and the same string
    on a handle without three-tick launches (FIBHIP_COURT_MULTI3=0,0,0) shows the row as its plan.  The shape of the
    two-tick launches INSIDE the mixed play is therefore not observed directly, in either case: it is inferred from
    build_plan reading the same variable the same way on both handles, from ticks_per_launch() == 3 (a string that names
    no row ends the multi-tick plans at that depth) and from the launch count.  FIBHIP_AUTOTUNE=0 throughout: the plan is
    the forced one, not the fastest of the day.
    what = 'bits': every row against the anchor; 'plain1' / 'plain2' / 'plain3': the anchor of every grid of the K = 1 / 2 / 3
    rows against the plain kernels (FIBHIP_COURT_AGG=0) at the bounds of test_court_aggregated_fast_tick, and nothing else."""
    from test_gpu_parity import COURT_SCALES, court_rel
    rows = [r for r in gpu_lib.variants() if r['model'] == COURT_AGG and r['phase'] == phase]
    assert rows and all(r['fast'] == 1 for r in rows)
    first = {K: next(r for r in rows if r['K'] == K and r['mode'] == MODE_FAST) for K in (2, 3)}
    flags = gpu_lib.FAST
    worst = Worst()
    anchors, failures, ran, n_multi, seen = _AGG_ANCHORS.setdefault(phase, {}), [], set(), 0, set()
    for r in rows:
        label = 'court on aggregates mode %d phase=%d K=%d %s' % (r['mode'], phase, r['K'], multi_env(r))
        try:
            assert r['mode'] in (MODE_FAST, MODE_FASTSLOW) and (r['K'] == 1 or r['mode'] == MODE_FAST)
            for H, W in grids_of(r):
                state, phi = court_state(H, W)
                phi = phi if phase else None
                if (H, W) not in anchors:
                    clear_env(monkeypatch, FIBHIP_VARIANT=ANCHOR, FIBHIP_NO_MULTI='1', FIBHIP_NO_LAZY='1', FIBHIP_AUTOTUNE='0')
                    a, f = play(gpu_lib, COURT, flags, H, W, COURT_DIFF, state, phi, AGG_PLAY)
                    assert f['tile'] == (64, 4, -256) and f['tpl'] == 1 and f['launches'] == [13], 'the anchor is not one launch per operation'
                    anchors[(H, W)] = a
                if what != 'bits':
                    if (H, W) in seen or what != 'plain%d' % r['K']:
                        continue
                    seen.add((H, W))
                    a = anchors[(H, W)]
                    # test_court_aggregated_fast_tick: against the plain kernels the sums are re-associated, nothing else
                    clear_env(monkeypatch, FIBHIP_VARIANT=ANCHOR, FIBHIP_COURT_AGG='0', FIBHIP_NO_LAZY='1', FIBHIP_AUTOTUNE='0')
                    p, _ = play(gpu_lib, COURT, flags, H, W, COURT_DIFF, state, phi, AGG_PLAY)
                    # where the play itself is ill-conditioned (the oracle's own answers along it spread by more than the bound)
                    # two float32 evaluations may differ by that much: there the difference must stay within three times the
                    # oracle's own width plus the bound; everywhere else within the bound
                    _, ill, lo, hi = oracle_error_bar(orc, lambda st: agg_play_oracle(orc, st, phi), state,
                                                      [court_rel(v) * COURT_SCALES[v] for v in range(21)])
                    for v in range(21):
                        key = 'aggregates against plain kernels phase=%d var %d' % (phase, v)
                        worst.add(key, a[-1][v], p[-1][v], court_rel(v), COURT_SCALES[v], '%dx%d' % (H, W), mask=ill)
                        worst.add_ill(key, np.abs(a[-1][v].astype(np.float64) - p[-1][v]) - 3.0 * (hi[v] - lo[v]), court_rel(v),
                                      COURT_SCALES[v], '%dx%d' % (H, W), ill)
                    continue
                env, want_tile, want_tpl = dict(FIBHIP_AUTOTUNE='0'), (r['TX'], r['TY'], -r['NT']), 3
                fused = fuses_slow(H, W)
                if r['K'] == 1:
                    env.update(FIBHIP_VARIANT=variant_env(r), FIBHIP_NO_MULTI='1')
                    if r['mode'] == MODE_FAST:
                        env['FIBHIP_NO_LAZY'] = '1'
                    want_tpl = 1
                    want_launches = 12 if r['mode'] == MODE_FASTSLOW and fused else 13
                else:
                    env['FIBHIP_COURT_MULTI%d' % r['K']] = multi_env(r)
                    if r['K'] == 2:
                        want_tile = (first[3]['TX'], first[3]['TY'], -first[3]['NT'])
                        clear_env(monkeypatch, FIBHIP_COURT_MULTI3='0,0,0', **env)
                        tile, tpl = plan_only(gpu_lib, COURT, flags, H, W, COURT_DIFF, phi)
                        if (tile, tpl) != ((r['TX'], r['TY'], -r['NT']), 2):
                            failures.append('%s on %dx%d: shape not taken: launches of two ticks run tile %s (%d ticks per launch)' % (
                                label, H, W, tile, tpl))
                    # 5 ticks = 3 + 2, 4 ticks + 'slow' = 3 + the fused launch (or a tick and 'slow'), 3 ticks = 3
                    want_launches = 5 if fused else 6
                clear_env(monkeypatch, **env)
                got, facts = play(gpu_lib, COURT, flags, H, W, COURT_DIFF, state, phi, AGG_PLAY)
                why = None
                if facts['tile'] != want_tile or facts['tile_end'] != want_tile or facts['tpl'] != want_tpl:
                    why = 'shape not taken: the deepest plan runs tile %s, %d ticks per launch, not %s, %d' % (
                        facts['tile'], facts['tpl'], want_tile, want_tpl)
                why = why or same_bits(got, anchors[(H, W)])
                if not why and facts['launches'] != [want_launches]:
                    why = 'the play took %s launches, not %d' % (facts['launches'], want_launches)
                if why:
                    failures.append('%s on %dx%d: %s' % (label, H, W, why))
            n_multi += 1 if r['K'] > 1 else 0
            ran.add(shape_of(r) + (r['mode'],))                   # (its forced plays have all completed)
        except Exception as e:
            failures.append('%s: %s: %s' % (label, type(e).__name__, e))
    report(ran if what == 'bits' else None, rows, failures + worst.check(), n_multi)


_AGG_ANCHORS = {}
