"""One Beeler-Reuter sub-step (br.py:125-205, direct gates) restated in plain NumPy float64.  TEST INFRASTRUCTURE.

No oracle and no device code: the formulas are written down a second time, from the reference's text, in double precision
and in their numerically stable spellings, so that the float32 implementations (oracle/fib_oracle.c, csrc/br_step.inc) can
be held to something that has an answer at EVERY float32 potential:

  * e^y - 1 is expm1(y);
  * the two 0/0 forms are x / -expm1(-c x) with the value 1/c at x == 0:
        alpha_m = -(V+47) / (exp(-0.1 (V+47)) - 1)      -> 10 at V = -47
        (V+23) / (1 - exp(-0.04 (V+23)))   (in i_K1)     -> 25 at V = -23
    which the float32 formulas turn into 0/0 at exactly V == -47.0f and V == -23.0f ("op contract").

The constants are the float32 values the reference's graph holds (its ab_coef table is float32, a Python float becomes
float32 where it meets a tensor), widened to double: the model restated is the reference's, not a neighbouring one.

step() takes what the sub-step reads: the state, dt, the diffusion term laplace(V0) * diff already formed, and the
boundary-enforced potential V0 (a cell of the outer ring is evaluated at its inner neighbour's potential,
ionic.py:107-113).  enforce_boundary() and laplace() form those in float64, for callers that have nothing else."""
import numpy as np


def _f(x):
    return float(np.float32(x))


# ab_coef, br.py:49-62 (float32; the d and f rows pre-multiplied by 2 in double first)
AB = np.array([[0.0005, 0.083, 50., 0.0, 0.0, 0.057, 1.0],        # ca_x1
               [0.0013, -0.06, 20., 0.0, 0.0, -0.04, 1.0],        # cb_x1
               [0.0000, 0.0, 47., -1.0, 47., -0.1, -1.0],         # ca_m
               [40., -0.056, 72., 0.0, 0.0, 0.0, 0.0],            # cb_m
               [0.126, -.25, 77., 0.0, 0.0, 0.0, 0.0],            # ca_h
               [1.7, 0.0, 22.5, 0.0, 0.0, -0.082, 1.0],           # cb_h
               [0.055, -.25, 78.0, 0.0, 0.0, -0.2, 1.0],          # ca_j
               [0.3, 0.0, 32., 0.0, 0.0, -0.1, 1.0],              # cb_j
               [2 * 0.095, -0.01, -5., 0.0, 0.0, -0.072, 1.0],    # ca_d
               [2 * 0.07, -0.017, 44., 0.0, 0.0, 0.05, 1.0],      # cb_d
               [2 * 0.012, -0.008, 28., 0.0, 0.0, 0.15, 1.0],     # ca_f
               [2 * 0.0065, -0.02, 30., 0.0, 0.0, -0.2, 1.0]],    # cb_f
              dtype=np.float32).astype(np.float64)
GATE_LO, GATE_HI = _f(0.00001), _f(0.99999)                       # rush_larsen's clip, ionic.py:115-123
V_LO, V_HI = -85.0, 25.0                                          # br.py:167-168


def removable(x, c):
    """x / (1 - exp(-c x)), continued by its limit 1/c at x == 0"""
    x = np.asarray(x, np.float64)
    zero = x == 0.0
    xs = np.where(zero, 1.0, x)
    return np.where(zero, 1.0 / c, xs / -np.expm1(-c * xs))


def rate(v, c):
    """calc_alpha_bata_tf, br.py:255-264"""
    if c[3] == 0.0:
        return c[0] * np.exp(c[1] * (v + c[2])) / (np.exp(c[5] * (v + c[2])) + c[6])
    # the one row with a linear term, alpha_m: c0 = 0, c2 == c4, c6 = -1: c3 (v + c4) / expm1(c5 (v + c4))
    assert c[0] == 0.0 and c[2] == c[4] and c[6] == -1.0
    return -c[3] * removable(v + c[4], -c[5])


def rates(v):
    """the twelve rates, in the table's row order"""
    return [rate(v, c) for c in AB]


def inf_tau(a, b):
    """calc_inf_tau, br.py:266-273"""
    return a / (a + b), 1.0 / (a + b)


def rush_larsen(g, ginf, tau, dt):
    """ionic.py:115-123"""
    return np.clip(g + (g - ginf) * np.expm1(-dt / tau), GATE_LO, GATE_HI)


def currents(V0, C, M, H, J, D, F, XI):
    """(i_K1, i_x1, i_Na, i_Ca), br.py:150-163"""
    k04, k08 = _f(0.04), _f(0.08)
    iK1 = _f(0.35) * (4.0 * np.expm1(k04 * (V0 + 85.0)) / (np.exp(k08 * (V0 + 53.0)) + np.exp(k04 * (V0 + 53.0)))
                      + _f(0.2) * removable(V0 + 23.0, k04))
    ix1 = XI * _f(0.8) * np.expm1(k04 * (V0 + 77.0)) / np.exp(k04 * (V0 + 35.0))
    iNa = (4.0 * M * M * M * H * J + _f(0.005)) * (V0 - 50.0)
    ECa = _f(0.0 - 82.3) - _f(13.0278) * np.log(C)
    iCa = _f(1.0 * 0.09) * D * F * (V0 - ECa)
    return iK1, ix1, iNa, iCa


def step(state, dt, lapdiff, V0, n=1):
    """solve(state, n): `state` [8, H, W] = V C M H J D F XI (float32 or float64), `lapdiff` = laplace(V0) * diff, `V0` the
    boundary-enforced potential; n = how many dt the slow gates advance (0: carried over).  Returns float64 [8, H, W]."""
    s = np.asarray(state, np.float64)
    V0 = np.asarray(V0, np.float64)
    _, C, M, H, J, D, F, XI = s
    dt = _f(dt)
    r = rates(V0)
    out = np.empty_like(s)
    out[2] = rush_larsen(M, *inf_tau(r[2], r[3]), dt)
    out[3] = rush_larsen(H, *inf_tau(r[4], r[5]), dt)
    if n > 0:
        dtn = _f(dt * n)
        out[7] = rush_larsen(XI, *inf_tau(r[0], r[1]), dtn)
        out[4] = rush_larsen(J, *inf_tau(r[6], r[7]), dtn)
        out[5] = rush_larsen(D, *inf_tau(r[8], r[9]), dtn)
        out[6] = rush_larsen(F, *inf_tau(r[10], r[11]), dtn)
    else:
        out[4], out[5], out[6], out[7] = J, D, F, XI
    iK1, ix1, iNa, iCa = currents(V0, C, M, H, J, D, F, XI)
    out[0] = np.clip(V0 + dt * np.asarray(lapdiff, np.float64) - dt * (iK1 + ix1 + iNa + iCa), V_LO, V_HI)
    out[1] = C + dt * (_f(-1.0e-7) * iCa + _f(0.07) * (_f(1.0e-7) - C))
    return out


def enforce_boundary(V):
    """ionic.py:107-113: the interior re-padded by its own edge"""
    return np.pad(np.asarray(V, np.float64)[1:-1, 1:-1], 1, mode='edge')


def laplace(V0, phi=None):
    """ionic.py:44-60 and :70-81 on the REFLECT-padded array: the nine-point stencil, plus the phase-field term"""
    X = np.pad(np.asarray(V0, np.float64), 1, mode='reflect')
    c = X[1:-1, 1:-1]
    n, s, w, e = X[:-2, 1:-1], X[2:, 1:-1], X[1:-1, :-2], X[1:-1, 2:]
    lap = n + s + w + e + 0.5 * (X[:-2, :-2] + X[2:, :-2] + X[:-2, 2:] + X[2:, 2:]) - 6.0 * c
    if phi is not None:
        P = np.pad(np.asarray(phi, np.float64), 1, mode='reflect')
        lap = lap + ((s - n) * (P[2:, 1:-1] - P[:-2, 1:-1]) + (e - w) * (P[1:-1, 2:] - P[1:-1, :-2])) / (4.0 * P[1:-1, 1:-1])
    return lap


def substep(state, dt, diff, phi=None, n=1):
    """step() with both of its derived inputs formed here, in float64"""
    V0 = enforce_boundary(np.asarray(state)[0])
    return step(state, dt, laplace(V0, phi) * diff, V0, n)


def tick(state, dt, diff, phi=None, skip=False):
    """five chained sub-steps (br.py:98-107), float64 throughout; with `skip` the slow gates advance 5 dt on the first"""
    s = np.asarray(state, np.float64)
    for i in range(5):
        s = substep(s, dt, diff, phi, ((5 if i == 0 else 0) if skip else 1))
    return s
