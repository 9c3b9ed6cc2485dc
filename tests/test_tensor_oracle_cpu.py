"""The oracle's tensor switch (oracle/fib_oracle.c orc_laplace_tensor, orc_set_tensor; oracle.tensor) and what
tests/test_gpu_tensor_models.py rests on, with the oracle alone — no device:

  the C operator equals tests/tensor_ref.py laplace32 bit for bit; at D = I the three sub-steps are the stock ones; the Fenton
  sub-step under the switch is tensor_ref.fenton_substep, also chained 200 times; the switch checks its planes and clears itself;
  the caps of comparisons (a) and (b) — how many cells the oracle itself leaves to its envelope, or to Beeler-Reuter's clip —
  hold on the grids used; and every mutant of the operator (tensor_cases.mutants) moves the potential by at least 100 times the
  bound it is compared under, and by more than the bound on at least 5 % of the cells: the comparisons would see it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tensor_cases as tcs  # noqa: E402
import tensor_ref  # noqa: E402
from tensor_cases import BR, COURT, DIFF, DT, FENTON, GRIDS, NEAR_CAP, same  # noqa: E402
from test_gpu_variant_table import br_reference, br_state, br_table, court_near_singular, court_state, fenton_state  # noqa: E402


@pytest.mark.parametrize('hole', [False, True], ids=['plain', 'hole'])
@pytest.mark.parametrize('shape', [(5, 4), (13, 17), (70, 75)], ids=lambda s: '%dx%d' % s)
def test_operator_is_laplace32(orc, shape, hole):
    """the six planes of test_gpu_tensor.test_unit_op (exact zeros, 1e-20, -1e20 and an infinity among them)"""
    H, W = shape
    X, D = tcs.unit_values(H, W), tcs.spd_field(H, W, 3 + H)
    phi = tcs.hole_field(H, W) if hole else None
    want = tensor_ref.laplace32(X, *D, phi)
    assert np.isfinite(want).sum() > want.size // 2
    assert same(orc.laplace_tensor(X, *D, phi), want)


def _substeps(orc, H, W, phi):
    """name -> the oracle's sub-step of a seeded state, as a function of nothing"""
    f, b, c = fenton_state(H, W)[0], br_state(H, W)[0], court_state(H, W)[0]
    return {'fenton': lambda: orc.fenton_step(f, DT, DIFF[FENTON], phi),
            'br direct': lambda: orc.br_step(b, DT, DIFF[BR], phi),
            'br cheby n=5': lambda: orc.br_step(b, DT, DIFF[BR], phi, br_table(), 5),
            'court chronic': lambda: orc.court_step(c, DT, DIFF[COURT], phi, True),
            'court acute': lambda: orc.court_step(c, DT, DIFF[COURT], phi, False)}


@pytest.mark.parametrize('hole', [False, True], ids=['plain', 'hole'])
def test_identity_tensor_leaves_every_substep(orc, hole):
    H, W = 70, 75
    phi = tcs.hole_field(H, W) if hole else None
    one, zero = np.ones((H, W), np.float32), np.zeros((H, W), np.float32)
    steps = _substeps(orc, H, W, phi)
    stock = {k: f() for k, f in steps.items()}
    with orc.tensor(one, one, zero):
        ident = {k: f() for k, f in steps.items()}
    with orc.tensor(*tcs.spd_field(H, W, 5)):
        real = {k: f() for k, f in steps.items()}
    for k in steps:
        assert np.isfinite(stock[k]).all()
        assert same(ident[k], stock[k]), k
        assert not same(real[k][0], stock[k][0]), '%s: the switch is not read' % k
        assert same(real[k][1:], stock[k][1:]), '%s: only the potential may see the tensor' % k


def test_fenton_substep_is_tensor_refs(orc):
    H, W = 70, 75
    phi, D = tcs.hole_field(H, W), tcs.spd_field(H, W, 23)
    s = fenton_state(H, W)[0]
    with orc.tensor(*D):
        assert same(orc.fenton_step(s, DT, 1.2, phi), tensor_ref.fenton_substep(s, DT, 1.2, *D, phi))
        chained = orc.fenton_run(s.copy(), DT, 1.2, phi, 200)
    want = s
    for _ in range(200):
        want = tensor_ref.fenton_substep(want, DT, 1.2, *D, phi)
    assert np.isfinite(want).all() and same(chained, want)


def test_switch_checks_and_clears(orc):
    H, W = 13, 17
    s, D = fenton_state(H, W)[0], tcs.spd_field(H, W, 1)
    stock = orc.fenton_step(s, DT, 1.2)
    with pytest.raises(ValueError, match='planes are'):
        with orc.tensor(*tcs.spd_field(H, W + 1, 1)):
            orc.fenton_step(s, DT, 1.2)
    assert same(orc.fenton_step(s, DT, 1.2), stock)                       # cleared behind the exception
    with orc.tensor(*D) as planes:
        assert all(p.dtype == np.float32 and p.flags.c_contiguous for p in planes)
        assert not same(orc.fenton_step(s, DT, 1.2), stock)
        with pytest.raises(AssertionError):
            with orc.tensor(*D):
                pass
    assert same(orc.fenton_step(s, DT, 1.2), stock)


# ---- the caps of (a) and (b) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hole', [False, True], ids=['plain', 'hole'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: '%dx%d' % g)
def test_caps_of_the_tick_comparison(orc, grid, hole):
    """Beeler-Reuter: the cells the oracle with the tensor leaves to its own envelope (oracle_error_bar asserts NEAR_CAP);
    Courtemanche: the cells near a singular potential"""
    H, W = grid
    for name in ('br-direct', 'br-cheby', 'br-direct-skip', 'br-cheby-skip'):
        state, phi, D, _ = tcs.tick_fields(name, H, W, hole)
        k = tcs.kind_of(name)
        with orc.tensor(*D):
            _, ill, _, _ = br_reference(orc, state, phi, br_table() if k['cheby'] else None, k['skip'], 5e-5 if k['cheby'] else 1e-5)
        print('%s %dx%d: %.2f %% of the cells ill-conditioned in the oracle' % (name, H, W, 100 * ill.mean()))
        assert ill.mean() <= NEAR_CAP
    near = court_near_singular(court_state(H, W)[0][0]).mean()
    print('court %dx%d: %.2f %% of the cells near a singular potential' % (H, W, 100 * near))
    assert near <= NEAR_CAP


@pytest.mark.parametrize('name', ['br-direct', 'br-cheby'])
def test_caps_of_the_substep_comparison(orc, name):
    """(b) with the oracle's own form standing in for the device: the clipped share and the three-rounding bound"""
    H, W = 70, 75
    phi, D = tcs.hole_field(H, W), tcs.spd_field(H, W, 23)
    s0 = br_state(H, W)[0]
    tbl = br_table() if tcs.kind_of(name)['cheby'] else None
    T = orc.br_step(s0, DT, 0.0, phi, tbl)
    with orc.tensor(*D):
        got = orc.br_step(s0, DT, DIFF[BR], phi, tbl)
    others, figs = tcs.substep_figures(name, False, s0, T, got, D, phi)
    for f in figs:
        print('%s: %.4g (bound %.3g)' % f)
    assert not others
    assert len(figs) == 2 and all(v <= b for _, v, b in figs)
    assert figs[1][1] > 0.25                                              # (the bound is no wider than the roundings it counts)


# ---- the mutants: what the comparisons see ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['fenton', 'br-direct', 'br-cheby', 'br-cheby-skip', 'court', 'court-all-acute', 'court-us'])
def test_tick_comparison_sees_every_mutant(orc, name):
    """the random field of (a), with a hole, 70 x 75; on it the ratio varies from cell to cell, so 'ratio 2.9 for 3' is every
    cell's ratio times 2.9 / 3.  Every mutant: at least 100 times the bound somewhere, more than the bound on at least 5 % of the
    cells.

    NAMED EXCEPTION — 'angle + 0.01' with Beeler-Reuter's Chebyshev gates: 100 times the DIRECT gates' bound (1e-5 of 120 mV), not
    Chebyshev's (5e-5); the share of cells is asserted at Chebyshev's own bound as for every other case.  What a mutant of the
    operator does to the potential in one tick does not depend on the gate form: diff * dt * (L_mutant - L) V summed over five
    sub-steps, 0.42 - 0.43 mV at most for this mutant with either form (353 times the direct bound on br-direct; 354 and 358 times
    it, 70.7 and 71.6 times their own bound, on the two Chebyshev cases).  Chebyshev's bound is five times wider for a reason that has nothing to do with the operator —
    the fits of the rate functions are not the functions — so the same move counts five times less against it; 87 % of the cells are
    beyond Chebyshev's bound all the same."""
    H, W = GRIDS[0]
    _, _, D, params = tcs.tick_fields(name, H, W, True)
    tol, scale = tcs.tick_tol(name, False)
    V = tcs.oracle_tick_V(orc, name, H, W, True, D)
    for what, Dm in tcs.mutants(params).items():
        Vm = tcs.oracle_tick_V(orc, name, H, W, True, Dm)
        worst, share = tcs.moved(V, Vm, tol * scale)
        print('%s, %s: %.3g times the bound, %.1f %% of the cells beyond it' % (name, what, worst, 100 * share))
        if tcs.kind_of(name)['cheby'] and what == 'angle + 0.01':
            worst = tcs.moved(V, Vm, tcs.tick_tol('br-direct', False)[0] * scale)[0]
        assert worst >= 100.0 and share >= 0.05, what


@pytest.mark.parametrize('name', ['fenton', 'br-direct', 'br-cheby-skip', 'court', 'court-us'])
def test_trajectory_comparison_sees_every_mutant(orc, name):
    ref = tcs.oracle_traj(orc, name)
    bound = tcs.traj_tol_V(name)
    for what, Dm in tcs.mutants(tcs.traj_params()).items():
        got = tcs.oracle_traj(orc, name, Dm)
        worst, share = max(tcs.moved(ref[t][0], got[t][0], bound) for t in tcs.TRAJ_SNAPS)
        print('%s, %s: %.3g times the bound, %.1f %% of the cells beyond it' % (name, what, worst, 100 * share))
        assert worst >= 100.0 and share >= 0.05, what


def test_trajectory_comparison_sees_a_dropped_divergence(orc, monkeypatch):
    """Fenton's one more mutant: the div D part of the first-order term dropped, in the NumPy sub-step"""
    state, phi, D = tcs.traj_setup('fenton')
    ref = tcs.oracle_traj(orc, 'fenton')[20][0]
    monkeypatch.setattr(tensor_ref, 'first_order', tcs.first_order_without_div)
    s = state
    for _ in range(200):
        s = tensor_ref.fenton_substep(s, DT, DIFF[FENTON], *D, phi)
    worst, share = tcs.moved(ref, s[0], tcs.traj_tol_V('fenton'))
    print('fenton, no div D: %.3g times the bound, %.1f %% of the cells beyond it' % (worst, 100 * share))
    assert worst >= 100.0 and share >= 0.05


@pytest.mark.parametrize('name', ['br-cheby', 'br-cheby-skip'])
def test_cap_of_the_trajectory_exception(orc, name):
    """the named exception of tensor_cases.traj_figures (H at tick 10): the cells where the oracle's own H spreads by more than the
    ordinary bound — where the exception asks less than that bound — are few (oracle_error_bar asserts NEAR_CAP), the envelope
    holds the oracle's own snapshots, and M, and H at tick 20, keep the stock bound"""
    ill, lo, hi = tcs.br_traj_envelope(orc, name)
    print('%s: %.2f %% of the cells ill-conditioned in the oracle itself, H at tick 10' % (name, 100 * ill.mean()))
    assert 0 < ill.mean() <= NEAR_CAP
    ref = tcs.oracle_traj(orc, name)
    assert all((lo[t] <= ref[t]).all() and (ref[t] <= hi[t]).all() for t in tcs.TRAJ_SNAPS)
    figs = tcs.traj_figures(orc, name, True, ref, ref)
    assert len(figs) == 16 and all(e == 0.0 for _, e, _ in figs)
    # and a snapshot one ordinary bound off in H, where the oracle is well-conditioned, is outside the exception's margin too
    off = {t: ref[t].copy() for t in ref}
    cell = np.unravel_index(int(np.argmin(hi[10][3] - lo[10][3])), ill.shape)
    off[10][3][cell] += np.float32(4.2e-5)
    worst = max(tcs.traj_figures(orc, name, True, off, ref), key=lambda f: f[1] / f[2])
    print('%s: H one bound off at %s: %s %.3f' % (name, cell, worst[0], worst[1]))
    assert worst[1] > 1.0
    for t, v in ((10, 2), (20, 2), (20, 3)):                              # the stock bound everywhere else: 4.2e-5 off is outside
        off = {s: ref[s].copy() for s in ref}
        off[t][v][np.unravel_index(int(np.argmax(hi[t][v] - lo[t][v])), ill.shape)] += np.float32(4.2e-5)
        assert max(e / b for _, e, b in tcs.traj_figures(orc, name, True, off, ref)) > 1.0, (t, v)
