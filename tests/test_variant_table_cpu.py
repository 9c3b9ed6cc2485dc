"""not-gpu: the kernel variant table of the built library (csrc/launch.hpp g_variants), read through
fibhip_variant_count / fibhip_variant_info, checked for what build_plan / autotune / find_variant (csrc/plan.inc) take
for granted — and a mutation check of the oracle comparison tests/test_gpu_variant_table.py makes.

The GPU file takes its rows from the same enumeration, so what is checked here is what runs there."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FENTON, BR, COURT, COURT_US, FENTON_ZP, COURT_AGG = 0, 1, 2, 3, 100, 101
SHAPE = ('model', 'mode', 'fast', 'phase', 'K', 'TX', 'TY', 'NT')
# sub-steps per tick of the model a table id runs (fibhip_default_steps_per_tick; the two ids that are no fibhip_model
# run Fenton's and Courtemanche's tick)
SPT_OF = {FENTON: 10, FENTON_ZP: 10, BR: 5, COURT: 1, COURT_US: 1, COURT_AGG: 1}


def threads_of(kind, K, TY, NT):
    """csrc/launch.hpp threads_of: the threads of a flat tile are listed; a strip (NT = -R) and a rows kernel
    (NT = -(32 + R)) run one wave per R rows of the tile grown by the rim of the K - 1 sub-steps still to come"""
    from fib_tf_amd import _lib
    if kind == _lib.MK_TICK:
        return NT
    R = -NT - (32 if kind == _lib.MK_ROWS else 0)
    return 64 * ((TY + 2 * (K - 1) + R - 1) // R)


def tables():
    """(name, rows) of the stock library and of the specialised Beeler-Reuter build __graft_entry__.build() leaves"""
    from fib_tf_amd import _lib, br
    out = [('stock', _lib.variants())]
    spec = br.specialised_library(br.BeelerReuter({'height': 8, 'width': 8, 'cheby': True})._table32())
    assert spec is not None, 'run __graft_entry__.build() first'
    out.append(('specialised Beeler-Reuter', _lib.variants(spec)))
    return out


def test_enumeration_answers_for_its_own_library():
    from fib_tf_amd import _lib
    (_, stock), (_, spec) = tables()
    L = _lib.lib()
    assert len(stock) == L.fibhip_variant_count() > 300
    assert [L.fibhip_default_steps_per_tick(m) for m in (FENTON, BR, COURT, COURT_US)] == [SPT_OF[m] for m in (FENTON, BR, COURT, COURT_US)]
    out = (_lib.C.c_int * 10)()
    for i in (-1, len(stock)):
        assert L.fibhip_variant_info(i, out) < 0 and b'variant_info' in L.fibhip_last_error()
    assert {r['model'] for r in stock} == {FENTON, BR, COURT, COURT_US, FENTON_ZP, COURT_AGG}
    # the specialised build carries Beeler-Reuter's defaults only: a strict part of the stock library's rows
    key = lambda r: tuple(r[k] for k in _lib.VARIANT_FIELDS)
    assert {r['model'] for r in spec} == {BR}
    assert 0 < len(spec) < len([r for r in stock if r['model'] == BR])
    assert {key(r) for r in spec} < {key(r) for r in stock}
    # kind follows from how the table lists NT (V4 / S4 / W4 of csrc/launch.hpp)
    for r in stock:
        assert r['kind'] == (_lib.MK_TICK if r['NT'] > 0 else _lib.MK_STRIP if r['NT'] > -32 else _lib.MK_ROWS), r


@pytest.mark.parametrize('which', [0, 1], ids=['stock', 'specialised'])
def test_table_invariants(which):
    from fib_tf_amd import _lib
    name, rows = tables()[which]
    bad = []
    seen = set()
    for r in rows:
        k = tuple(r[f] for f in SHAPE)
        if k in seen:
            bad.append('%s: listed twice (find_variant shadows the second): %r' % (name, k))
        seen.add(k)
        n = threads_of(r['kind'], r['K'], r['TY'], r['NT'])
        if not 64 <= n <= 1024 or n % 64:
            bad.append('%s: %r runs %d threads per workgroup' % (name, k, n))
        if r['model'] not in SPT_OF:
            bad.append('%s: %r: a model tests/test_gpu_variant_table.py does not know' % (name, k))
        elif r['has_mt'] and not (r['kind'] == _lib.MK_STRIP and r['K'] == SPT_OF[r['model']] and r['model'] in (FENTON, BR)):
            bad.append('%s: %r is listed as a multi-tick launch' % (name, k))
        # (K counts sub-steps of one tick; Courtemanche on aggregates fuses up to three whole ticks: csrc/plan.inc multi_max)
        if not 1 <= r['K'] <= (3 if r['model'] == COURT_AGG else SPT_OF.get(r['model'], 1)):
            bad.append('%s: %r: K outside what a launch can cover' % (name, k))
    groups = {}
    for r in rows:
        groups.setdefault((r['model'], r['mode'], r['fast']), {}).setdefault(r['phase'], set()).add((r['K'], r['TX'], r['TY'], r['NT']))
    for g, by_phase in groups.items():
        if set(by_phase) != {0, 1}:
            bad.append('%s: (model, mode, fast) = %r has phase values %r only' % (name, g, sorted(by_phase)))
        elif by_phase[0] != by_phase[1]:
            bad.append('%s: %r: the two phase values list different shapes: %r' % (name, g, sorted(by_phase[0] ^ by_phase[1])))
        for ph, shapes in by_phase.items():
            if not any(s[0] == 1 for s in shapes):
                bad.append('%s: %r phase %d has no K = 1 row for the remainder of a tick' % (name, g, ph))
    assert not bad, '\n'.join(bad)


def test_grids_of_the_gpu_test_stay_small():
    """the two grids per row of tests/test_gpu_variant_table.py: nine tiles each — every one resident, so every has_mt row
    runs as a multi-tick launch — and none larger than 168 x 162"""
    from test_gpu_variant_table import grids_of
    for _, rows in tables():
        for r in rows:
            for H, W in grids_of(r):
                assert -(-H // r['TY']) * -(-W // r['TX']) == 9
                assert 3 <= H <= 168 and 3 <= W <= 3 * 64
    assert max(H for _, rows in tables() for r in rows for H, _ in grids_of(r)) == 168
    assert max(W for _, rows in tables() for r in rows for H, W in grids_of(r) if H == 168) == 162


# --------------------------------------------------------------------------------------------------------------------
# the share of Courtemanche cells the GPU test leaves out of its oracle comparison
# --------------------------------------------------------------------------------------------------------------------
def test_court_states_keep_clear_of_the_singular_potentials():
    from test_gpu_variant_table import court_state, court_near_singular, NEAR_CAP, grids_of
    from fib_tf_amd import _lib
    worst = 0.0
    for H, W in sorted({g for r in _lib.variants() if r['model'] in (COURT, COURT_AGG) for g in grids_of(r)}):
        init, _ = court_state(H, W)
        share = float(court_near_singular(init[0]).mean())
        worst = max(worst, share)
        assert share <= NEAR_CAP, '%dx%d: %.2f %% of the cells within 0.06 mV of a singular potential' % (H, W, 100 * share)
    print('largest share left out: %.2f %%' % (100 * worst))


def test_br_states_leave_few_cells_to_the_oracles_own_error_bar(orc):
    """the cells tests/test_gpu_variant_table.py leaves out of its Beeler-Reuter oracle comparison — where the oracle's own
    answer moves by more than the bound under one ulp of exp() or two of V — are a small share of every grid"""
    from test_gpu_variant_table import br_state, br_reference, br_table, NEAR_CAP, grids_of
    from fib_tf_amd import _lib
    worst = 0.0
    for H, W in sorted({g for r in _lib.variants() if r['model'] == BR for g in grids_of(r)}):
        st, phi = br_state(H, W)
        for tbl, rel in ((None, 1e-5), (br_table(), 5e-5)):
            for skip in (False, True):
                for p in (phi, None):
                    worst = max(worst, float(br_reference(orc, st, p, tbl, skip, rel)[1].mean()))      # (asserts the cap itself)
    print('largest share left out: %.2f %%' % (100 * worst))
    assert worst <= NEAR_CAP


# --------------------------------------------------------------------------------------------------------------------
# mutation check: would the oracle comparison of the GPU test see a kernel that reads one tile-seam column wrongly?
# --------------------------------------------------------------------------------------------------------------------
def _fenton_steps(orc, st, phi, dt, diff, nsteps, seam=None):
    """orc_fenton_step restated on the oracle's own operations; with `seam` = c the Laplacian's input has column c taken
    from column c - 1: what a tile that reads its left halo one cell off would compute"""
    st = st.copy()
    dtf, ddt = np.float32(dt), np.float32(diff * dt)
    for _ in range(nsteps):
        U0 = orc.enforce_boundary(st[0])
        X = U0
        if seam is not None:
            X = U0.copy()
            X[:, seam] = U0[:, seam - 1]
        lap = orc.laplace(X, phi)
        d = orc.fenton_diff(st[0], st[1], st[2], st[3])
        st = np.stack([(U0 + dtf * d[0]) + ddt * lap, st[1] + dtf * d[1], st[2] + dtf * d[2], st[3] + dtf * d[3]]).astype(np.float32)
    return st


def test_oracle_comparison_sees_a_seam_error(orc):
    from test_gpu_variant_table import fenton_state, grids_of, FAST_STEP_TOL, FENTON_DT, FENTON_DIFF
    TX, TY = 44, 25
    (H, W), _ = grids_of({'TX': TX, 'TY': TY})
    assert (H, W) == (51, 89)
    st, phi = fenton_state(H, W)
    nsteps = 20
    true = orc.fenton_run(st.copy(), FENTON_DT, FENTON_DIFF, phi, nsteps)
    same = _fenton_steps(orc, st, phi, FENTON_DT, FENTON_DIFF, nsteps)
    assert np.array_equal(same, true), 'the restated step is not the oracle\'s'
    wrong = _fenton_steps(orc, st, phi, FENTON_DT, FENTON_DIFF, nsteps, seam=TX)
    ceiling = nsteps * FAST_STEP_TOL                              # the loosest bound the GPU test applies (fast policy)
    err = float(np.abs(wrong - true).max())
    print('seam error after %d sub-steps: %.3e = %.0f x the fast ceiling %.1e' % (nsteps, err, err / ceiling, ceiling))
    assert err > 100 * ceiling
