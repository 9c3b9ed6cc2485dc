"""Beeler-Reuter at its 0/0 voltages, CPU side: the float64 restatement (tests/br_ref64.py) against the oracle on control
cells, and the oracle AT the two voltages (V == -47.0f: alpha_m defined as 10; V == -23.0f: i_K1's second quotient defined as
25; DESIGN.md 9, "op contract") against the float64 restatement.

Bounds: STEP_TOL['exact'] (4e-6) of the array's scale per sub-step, the scales of test_br_single_step (V / 120 mV,
C / 1e-5, gates / 1): what the suite allows two float32 evaluations of one sub-step.  The +-1, +-2, +-4 float32 neighbours of
the two voltages are ill-conditioned in the reference's own float32 formulas (one ulp of exp is a relative rate error of
6e-8 / (c |x|)) and are held to the oracle's own sensitivity envelope instead (test_gpu_variant_table.oracle_error_bar);
they are the ONLY cells that may be: N_NEIGHBOUR_CELLS, a count."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import br_ref64  # noqa: E402
import br_singular_cases as sc  # noqa: E402
from timestep_cases import BR_VARS, STEP_TOL  # noqa: E402

TOL = STEP_TOL['exact']
CASES = [(dt, n) for dt in (0.1, 0.02) for n in (1, 5)]


@pytest.fixture(scope='module')
def planes():
    st, control = sc.plane()
    exact, neigh = sc.classify(st[0])
    for a in (st, control):
        a.setflags(write=False)
    return {'state': st, 'control': control, 'exact': exact, 'neigh': neigh, 'phi': sc.phase(*sc.SHAPE)}


def figures(got, want, mask, what):
    return ['%s %s: %.3e > %.1e * %g at %s' % (what, k, err, TOL, s, cell)
            for k, s, err, cell in ((k, s, *worst(got[i], want[i], mask)) for i, (k, s) in enumerate(zip(BR_VARS, sc.BR_SCALES)))
            if not err <= TOL * s]


def worst(got, want, mask):
    d = np.where(mask, np.abs(np.asarray(got, np.float64) - want), 0.0)
    if not np.isfinite(np.asarray(got)[mask]).all():
        return float('inf'), None
    return float(d.max()), tuple(int(i) for i in np.unravel_index(int(np.argmax(d)), d.shape))


@pytest.mark.parametrize('dt,n', CASES)
def test_ref64_matches_oracle_on_control_cells(orc, planes, dt, n):
    """validates the restatement against the code path the goldens pin: every cell of the planted plane that is neither
    exact nor a neighbour, and every cell of the plane without planted cells"""
    for name, st, mask in (('planted plane', planes['state'], ~(planes['exact'] | planes['neigh'])),
                           ('control plane', planes['control'], np.ones(sc.SHAPE, bool))):
        got = orc.br_step(st, dt, sc.DIFF, planes['phi'], None, n)
        want = br_ref64.substep(st, dt, sc.DIFF, planes['phi'], n)
        assert mask.sum() > 0.9 * mask.size
        bad = figures(got, want, mask, name)
        assert not bad, '; '.join(bad)


@pytest.mark.parametrize('dt,n', CASES)
def test_ref64_inputs_from_the_oracle(orc, planes, dt, n):
    """step() fed the oracle's own float32 boundary-enforced potential and Laplacian (bit-exact paths of the goldens) gives
    what it gives from its float64 ones: the two ways the GPU tests may form its inputs"""
    st = planes['state']
    V0 = orc.enforce_boundary(st[0])
    assert np.array_equal(V0, sc.seen(st[0]))
    a = br_ref64.step(st, dt, orc.laplace(V0, planes['phi']).astype(np.float64) * sc.DIFF, V0, n)
    b = br_ref64.substep(st, dt, sc.DIFF, planes['phi'], n)
    for i, s in enumerate(sc.BR_SCALES):
        assert np.abs(a[i] - b[i]).max() <= 0.1 * TOL * s, BR_VARS[i]


@pytest.mark.parametrize('dt,n', CASES)
def test_oracle_at_exact_cells(orc, planes, dt, n):
    """the oracle AT the two voltages: finite, within the one-sub-step bound of the float64 restatement, and on a clip
    bound only where the restatement is.  (The reference's formulas give NaN there, which the clips turn into V = -85 and
    M = 1e-5: this test fails with the oracle's two definitions taken out.)"""
    st, exact = planes['state'], planes['exact']
    got = orc.br_step(st, dt, sc.DIFF, planes['phi'], None, n)
    assert np.isfinite(got).all()
    want = br_ref64.substep(st, dt, sc.DIFF, planes['phi'], n)
    assert exact.sum() == sc.N_EXACT_CELLS
    bad = figures(got, want, exact, 'exact cells')
    assert not bad, '; '.join(bad)
    stray = sc.on_bound(got) & ~sc.on_bound(want.astype(np.float32)) & exact
    assert not stray.any(), 'exact cells on a clip bound the float64 restatement is not on: %s' % (np.argwhere(stray)[:8].tolist(),)


@pytest.mark.parametrize('dt,n', CASES)
def test_oracle_neighbours_inside_envelope(orc, planes, dt, n):
    """the +-k-ulp neighbours: the float64 value lies inside the oracle's own sensitivity envelope (exp within one ulp, V
    within two float32 neighbours) widened by three times its width plus the bound.  No control cell is ill-conditioned,
    and at most the planted neighbours are treated this way."""
    from test_gpu_variant_table import oracle_error_bar
    st, exact, neigh = planes['state'], planes['exact'], planes['neigh']
    bounds = sc.step_bounds(TOL)
    ref, ill, lo, hi = oracle_error_bar(orc, lambda s: orc.br_step(s, dt, sc.DIFF, planes['phi'], None, n), st, bounds)
    assert not (ill & ~(exact | neigh)).any(), 'control cells ill-conditioned in the oracle: %s' % (np.argwhere(ill & ~(exact | neigh))[:8].tolist(),)
    by_envelope = ill & ~exact
    assert int(by_envelope.sum()) <= sc.N_NEIGHBOUR_CELLS
    want = br_ref64.substep(st, dt, sc.DIFF, planes['phi'], n)
    assert np.isfinite(ref).all()
    for i, (k, b) in enumerate(zip(BR_VARS, bounds)):
        # neighbours the envelope does not cover are well-conditioned: the plain bound
        plain = neigh & ~ill
        assert np.abs(ref[i].astype(np.float64) - want[i])[plain].max(initial=0.0) <= b, k
        margin = 3.0 * (hi[i] - lo[i]) + b
        out = np.maximum(lo[i] - want[i], want[i] - hi[i])
        assert (out <= margin)[by_envelope].all(), '%s: %.3e beyond the envelope' % (k, float((out - margin)[by_envelope].max()))


def test_plane_has_what_it_says(planes):
    st, exact, neigh = planes['state'], planes['exact'], planes['neigh']
    V = st[0]
    H, W = sc.SHAPE
    ring = np.ones(sc.SHAPE, bool)
    ring[1:-1, 1:-1] = False
    beside = ~ring
    beside[2:-2, 2:-2] = False                                          # the cells next to the ring
    for s in (sc.S47, sc.S23):
        at = sc.seen(V) == s
        assert at[2:-2, 2:-2].any() and (at & ring).any() and (at & beside).any()
        assert (V[0] == s).any() and (V[:, 0] == s).any()              # planted on the ring itself, where nobody reads it
    assert all(exact[r, c] for r in (0, H - 1) for c in (0, W - 1))      # the four corners, clamped along both axes
    assert int(neigh.sum()) == sc.N_NEIGHBOUR_CELLS
    assert set(sc.seen(V)[neigh].tolist()) == set(sc.NEIGHBOURS.tolist())
    clear = ~(exact | neigh)
    assert (np.minimum(np.abs(sc.seen(V) + 47.0), np.abs(sc.seen(V) + 23.0))[clear] >= 0.5 - 1e-6).all()


def test_sheet_and_forms_states():
    from test_gpu_timestep import make_big_states
    st = sc.kernel_forms_state(make_big_states()['br'])
    exact, _ = sc.classify(st[0])
    assert exact.sum() == 18 + 19 + 19
    cols = {r: set(np.flatnonzero(exact[r]).tolist()) for r in (20, 21, 27)}
    assert 54 in cols[20] and {64, 127} <= cols[21] and 108 in cols[27]
    assert (st[0] == sc.S47).sum() == 28 and (st[0] == sc.S23).sum() == 28
    # (21, 1) lies next to the ring: the ring cell (21, 0) reads it; (27, 129) lies ON the ring, where nobody reads it
    assert exact[21, 0] and st[0][27, 129] == sc.S23 and not exact[27, 129]
    sh, snapped = sc.sheet()
    assert snapped.mean() == 0.125 and (sh[0][:32][snapped[:32]] == sc.S23).all() and (sh[0][32:][snapped[32:]] == sc.S47).all()
    unsnapped = np.minimum(np.abs(sh[0] + 47.0), np.abs(sh[0] + 23.0))[~snapped]
    assert unsnapped.min() > 1e-3 and unsnapped.max() < 1.01
