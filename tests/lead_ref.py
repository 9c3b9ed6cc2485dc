"""The lead recorder's definition (include/fibhip.h, fibhip_leads_*) restated in NumPy.

float32 arithmetic, one rounding per operation, in the reference's order (ionic.py:44-81): the source plane on the interior cells
through the boundary clamp, the weighted plane, and the float64 terms (double)K * (double)q, which are exact.  `traces` sums the
terms with math.fsum — the correctly rounded exact sum, the yardstick of the device's float64 summation, whose order it does not
share."""
import math

import numpy as np

U = 2.0 ** -53
f32 = np.float32


def clamped(X):
    """enforce_boundary: every cell reads X[clamp(r, 1, H - 2)][clamp(c, 1, W - 2)]"""
    X = np.asarray(X, f32)
    H, W = X.shape
    r = np.clip(np.arange(H), 1, H - 2)
    c = np.clip(np.arange(W), 1, W - 2)
    return X[np.ix_(r, c)]


def _taps(X):
    """the nine taps of every interior cell, each [H - 2, W - 2], read through the clamp"""
    B = np.pad(clamped(X)[1:-1, 1:-1], 1, mode='edge')          # interior + a ring of clamped taps
    n, m = B.shape
    at = lambda dr, dc: B[1 + dr:n - 1 + dr, 1 + dc:m - 1 + dc]  # noqa: E731
    return {k: at(*d) for k, d in dict(N=(-1, 0), S=(1, 0), W=(0, -1), E=(0, 1), NW=(-1, -1), SW=(1, -1), NE=(-1, 1), SE=(1, 1),
                                       C=(0, 0)).items()}


def stencil(X):
    """stencil9 in the reference's order (ionic.py:51-53) on the interior cells: float32 [H - 2, W - 2]"""
    t = _taps(X)
    with np.errstate(all='ignore'):
        l = (((t['N'] + t['S']) + t['W']) + t['E']) + f32(0.5) * (((t['NW'] + t['SW']) + t['NE']) + t['SE'])
        return (l - f32(6.0) * t['C']).astype(f32)


def phase_term(X, phase):
    """the phase-field term (ionic.py:78-80) on the interior cells: ((S - N) * dpy + (E - W) * dpx) / (4 phi), the differences of
    phi REFLECT-padded, the quotient correctly rounded"""
    t = _taps(X)
    P = np.pad(np.asarray(phase, f32), 1, mode='reflect')
    dpy = (P[2:, 1:-1] - P[:-2, 1:-1])[1:-1, 1:-1]
    dpx = (P[1:-1, 2:] - P[1:-1, :-2])[1:-1, 1:-1]
    q4 = (f32(4.0) * np.asarray(phase, f32))[1:-1, 1:-1]
    with np.errstate(all='ignore'):
        return (((t['S'] - t['N']) * dpy + (t['E'] - t['W']) * dpx) / q4).astype(f32)


def source(X, phase=None):
    """the source plane on the interior cells, float32 [H - 2, W - 2]: laplace(enforce_boundary(X))[1:-1, 1:-1] in the exact form"""
    s = stencil(X)
    if phase is not None:
        with np.errstate(all='ignore'):
            s = (s + phase_term(X, phase)).astype(f32)
    return s


def weighted(X, phase=None, weight=None):
    """q = w * S, one float32 product; weight None: q = S"""
    s = source(X, phase)
    if weight is None:
        return s
    with np.errstate(all='ignore'):
        return (np.asarray(weight, f32)[1:-1, 1:-1] * s).astype(f32)


def kernel_of(pos, tables, H, W):
    """K_e on the interior cells: T[t_e][|r - r_e|][|c - c_e|], float32 [H - 2, W - 2]"""
    r, c, t = (int(x) for x in pos)
    T = np.asarray(tables, f32)
    if T.ndim == 2:
        T = T[np.newaxis]
    dr = np.abs(np.arange(1, H - 1) - r)
    dc = np.abs(np.arange(1, W - 1) - c)
    return T[t][np.ix_(dr, dc)]


def terms(X, phase, weight, pos, tables):
    """float64 [E, (H - 2) * (W - 2)]: the exact products (double)K_e * (double)q of every lead over the interior cells"""
    X = np.asarray(X, f32)
    H, W = X.shape
    q = weighted(X, phase, weight).astype(np.float64)
    with np.errstate(all='ignore'):
        return np.stack([(kernel_of(p, tables, H, W).astype(np.float64) * q).ravel() for p in np.asarray(pos).reshape(-1, 3)])


def traces(X, phase, weight, pos, tables):
    """float64 [E]: math.fsum of every lead's terms (NaN where a term is NaN)"""
    out = []
    for t in terms(X, phase, weight, pos, tables):
        out.append(math.fsum(t.tolist()) if np.all(np.isfinite(t)) else float(np.sum(t)))
    return np.array(out, np.float64)


def bound(t):
    """what any order of float64 summation of the n terms `t` may differ from their exact sum by: n u / (1 - n u) * sum |t|"""
    t = np.asarray(t, np.float64).ravel()
    n = len(t)
    return n * U / (1.0 - n * U) * math.fsum(np.abs(t).tolist())


def sample_ticks(nticks, every):
    """the ticks (0-based) behind which a sample is taken: every - 1, 2 * every - 1, ..."""
    return [k for k in range(nticks) if (k + 1) % every == 0]
