"""The potential-map recorder's definition (include/fibhip.h, fibhip_pmap_*) restated in NumPy.

The source plane is the lead recorder's (tests/lead_ref.py `weighted`), +0.0 on the outer ring and off the grid.  `maps` follows
the definition's order of summation — rows dr = -R .. R, within a row dc = -R .. R, every float64 addition rounded on its own;
the products of two float32 values are exact in float64, so multiply-then-add here is the device's fused multiply-add bit for
bit — and `exact` sums the same terms with math.fsum, the yardstick whose order nobody shares.  `summary` restates the per-site
summary of a cube."""
import math

import numpy as np

import lead_ref

U = lead_ref.U
f32 = np.float32


def source_plane(X, phase=None, weight=None):
    """q on the whole grid, float32 [H, W]: lead_ref.weighted on the interior cells, +0.0 on the outer ring"""
    X = np.asarray(X, f32)
    q = np.zeros(X.shape, f32)
    q[1:-1, 1:-1] = lead_ref.weighted(X, phase, weight)
    return q


def lattice(H, W, window=None, step=(1, 1)):
    """(rows, cols): site (i, j) sits at the cell (rows[i], cols[j])"""
    r0, r1, c0, c1 = (0, H, 0, W) if window is None else window
    return np.arange(r0, r1, step[0]), np.arange(c0, c1, step[1])


def padded(q, R):
    return np.pad(np.asarray(q, f32), R).astype(np.float64)          # (zeros: +0.0)


def maps(q, table, window=None, step=(1, 1), order='rows'):
    """float64 [oh, ow]: the definition's sum at every site of the lattice.  order='cols' sums columns before rows — NOT the
    definition; the order-sensitivity test uses it"""
    T = np.asarray(table, f32).astype(np.float64)
    R = T.shape[0] - 1
    assert T.shape == (R + 1, R + 1)
    H, W = np.shape(q)
    rows, cols = lattice(H, W, window, step)
    P = padded(q, R)
    phi = np.zeros((len(rows), len(cols)), np.float64)
    with np.errstate(all='ignore'):
        for a in range(-R, R + 1):
            p = np.zeros_like(phi)
            for b in range(-R, R + 1):
                dr, dc = (a, b) if order == 'rows' else (b, a)
                p = p + T[abs(dr), abs(dc)] * P[np.ix_(rows + R + dr, cols + R + dc)]
            phi = phi + p
    return phi


def terms(q, table, r, c):
    """float64 [(2R + 1)^2]: the exact products of the site at the cell (r, c), in the definition's order"""
    T = np.asarray(table, f32).astype(np.float64)
    R = T.shape[0] - 1
    P = padded(q, R)
    d = np.abs(np.arange(-R, R + 1))
    with np.errstate(all='ignore'):
        return (T[np.ix_(d, d)] * P[r:r + 2 * R + 1, c:c + 2 * R + 1]).ravel()


def exact(q, table, r, c):
    t = terms(q, table, r, c)
    return math.fsum(t.tolist()) if np.all(np.isfinite(t)) else float(np.sum(t))


def bound(t, R):
    """what the definition's sum may differ from the exact sum of the terms `t` by: n u / (1 - n u) * sum |t| with
    n = (2R + 1)^2 + 2R + 1 — the additions of the row sums and those of the rows"""
    n = (2 * R + 1) ** 2 + 2 * R + 1
    return n * U / (1.0 - n * U) * math.fsum(np.abs(np.asarray(t, np.float64)).tolist())


def summary(cube, first=0, count=None):
    """the per-site summary of the samples [first, first + count) of a cube [samples, oh, ow], plain loops: (vmin, vmax, dmin
    float64, kmin, kmax, kd int32).  Strict compares, the first occurrence wins, every value starts from the first element"""
    cube = np.asarray(cube, np.float64)
    count = len(cube) - first if count is None else count
    assert count >= 2
    c = cube[first:first + count]
    vmin, vmax = c[0].copy(), c[0].copy()
    kmin = np.full(c[0].shape, first, np.int32)
    kmax = kmin.copy()
    with np.errstate(all='ignore'):
        dmin = c[1] - c[0]
        kd = np.full(c[0].shape, first + 1, np.int32)
        for s in range(1, count):
            lo, hi = c[s] < vmin, c[s] > vmax
            vmin[lo], kmin[lo] = c[s][lo], first + s
            vmax[hi], kmax[hi] = c[s][hi], first + s
            if s > 1:
                d = c[s] - c[s - 1]
                m = d < dmin
                dmin[m], kd[m] = d[m], first + s
    return vmin, vmax, dmin, kmin, kmax, kd
