"""The tensor operator of DESIGN.md 25, restated in NumPy — what tests/test_tensor_cpu.py and tests/test_gpu_tensor.py compare
the device with.  Written from the definition, not from the kernels:

    weights(dyy, dxx, dxy)                      the five float32 planes, one rounded operation per line
    laplace32(X, dyy, dxx, dxy, phi=None)       the Exact policy's operator in float32, every product and sum rounded once, in order
    laplace64(X, dyy, dxx, dxy, phi=None)       the same operator in float64 (weights formed in float64 too)
    terms64(X, dyy, dxx, dxy, phi=None)         per cell, the sum of the magnitudes of the elementary terms of laplace64
    fibre_planes(angle, ratio, scale)           fibre_tensor's planes
    fenton_substep(slab, dt, diff, ...)         one Fenton sub-step on the CPU: oracle.fenton_diff plus laplace32

X is read through the REFLECT pad, as the reference's laplace reads it (ionic.py:49-50); the caller applies enforce_boundary.
Tap names: N = row - 1, S = row + 1, W = column - 1, E = column + 1."""
import numpy as np

F = np.float32


def weights(dyy, dxx, dxy, dtype=np.float32):
    t = dtype
    dyy, dxx, dxy = (np.asarray(p, t) for p in (dyy, dxx, dxy))
    wd = t(0.25) * (dyy + dxx)
    wy = t(1.5) * dyy - t(0.5) * dxx
    wx = t(1.5) * dxx - t(0.5) * dyy
    wa = wd + dxy
    wb = wd - dxy
    wc = t(12.0) * wd
    return wy, wx, wa, wb, wc


def _taps(X):
    P = np.pad(X, 1, mode='reflect')
    c = slice(1, -1)
    return dict(N=P[:-2, c], S=P[2:, c], W=P[c, :-2], E=P[c, 2:], NW=P[:-2, :-2], SW=P[2:, :-2], NE=P[:-2, 2:], SE=P[2:, 2:], C=P[c, c])


def _dy(A):
    """central difference along the rows without the 1/2, REFLECT-padded"""
    P = np.pad(A, 1, mode='reflect')
    return P[2:, 1:-1] - P[:-2, 1:-1]


def _dx(A):
    P = np.pad(A, 1, mode='reflect')
    return P[1:-1, 2:] - P[1:-1, :-2]


def first_order(dyy, dxx, dxy, phi, dtype=np.float32):
    """(gy, gx, q4): the first-order coefficients and 4 phi"""
    t = dtype
    dyy, dxx, dxy = (np.asarray(p, t) for p in (dyy, dxx, dxy))
    phi = np.ones_like(dyy) if phi is None else np.asarray(phi, t)
    dpy, dpx = _dy(phi), _dx(phi)
    p2 = t(2.0) * phi
    gy = (dyy * dpy + dxy * dpx) + p2 * (_dy(dyy) + _dx(dxy))
    gx = (dxy * dpy + dxx * dpx) + p2 * (_dy(dxy) + _dx(dxx))
    return gy, gx, t(4.0) * phi


def _fma32(a, b, c):
    """RN32(a * b + c) for float32 arrays: the product is exact in float64"""
    with np.errstate(all='ignore'):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _divc32(a, c):
    """a / c as the kernels divide by 4 phi (csrc/models.hpp Exact::divc): q = RN(a * rc), r = fma(-q, c, a), fma(r, rc, q) with
    rc = RN(1 / c) — RN(a / c) for every finite a in range, NaN for an infinite one"""
    with np.errstate(all='ignore'):
        rc = F(1.0) / c
        q = a * rc
        r = _fma32(-q, c, a)
        return _fma32(r, rc, q)


def laplace32(X, dyy, dxx, dxy, phi=None):
    X = np.asarray(X, F)
    wy, wx, wa, wb, wc = weights(dyy, dxx, dxy)
    t = _taps(X)
    with np.errstate(all='ignore'):
        l = ((((wy * t['N'] + wy * t['S']) + wx * t['W']) + wx * t['E']) + (((wa * t['NW'] + wb * t['SW']) + wb * t['NE']) + wa * t['SE'])) - wc * t['C']
        gy, gx, q4 = first_order(dyy, dxx, dxy, phi)
        num = (t['S'] - t['N']) * gy + (t['E'] - t['W']) * gx
        return l + _divc32(num, q4)


def laplace64(X, dyy, dxx, dxy, phi=None):
    D = np.float64
    X = np.asarray(X, D)
    wy, wx, wa, wb, wc = weights(dyy, dxx, dxy, D)
    t = _taps(X)
    with np.errstate(all='ignore'):
        l = wy * (t['N'] + t['S']) + wx * (t['W'] + t['E']) + wa * (t['NW'] + t['SE']) + wb * (t['NE'] + t['SW']) - wc * t['C']
        gy, gx, q4 = first_order(dyy, dxx, dxy, phi, D)
        return l + ((t['S'] - t['N']) * gy + (t['E'] - t['W']) * gx) / q4


def terms64(X, dyy, dxx, dxy, phi=None):
    """sum over the elementary terms of laplace64 of their magnitudes: every product coefficient * tensor entry * tap of the
    second-order part (wy N = 1.5 dyy N - 0.5 dxx N: two terms), and every product of the first-order part"""
    D = np.float64
    X = np.asarray(X, D)
    dyy, dxx, dxy = (np.abs(np.asarray(p, D)) for p in (dyy, dxx, dxy))
    t = {k: np.abs(v) for k, v in _taps(X).items()}
    with np.errstate(all='ignore'):
        s = (1.5 * dyy + 0.5 * dxx) * (t['N'] + t['S']) + (1.5 * dxx + 0.5 * dyy) * (t['W'] + t['E'])
        s = s + (0.25 * (dyy + dxx) + dxy) * (t['NW'] + t['SE'] + t['NE'] + t['SW']) + 3.0 * (dyy + dxx) * t['C']
        phi = np.ones_like(dyy) if phi is None else np.asarray(phi, D)
        ap = lambda A: np.abs(np.pad(A, 1, mode='reflect'))
        ady = lambda A: ap(A)[2:, 1:-1] + ap(A)[:-2, 1:-1]
        adx = lambda A: ap(A)[1:-1, 2:] + ap(A)[1:-1, :-2]
        sdyy, sdxx, sdxy = (np.asarray(p, D) for p in (dyy, dxx, dxy))
        gy = dyy * ady(phi) + dxy * adx(phi) + 2.0 * phi * (ady(sdyy) + adx(sdxy))
        gx = dxy * ady(phi) + dxx * adx(phi) + 2.0 * phi * (ady(sdxy) + adx(sdxx))
        return s + ((t['S'] + t['N']) * gy + (t['E'] + t['W']) * gx) / (4.0 * phi)


def fibre_planes(angle, ratio, scale=1.0, shape=None):
    """(dyy, dxx, dxy) float32: longitudinal `scale`, transverse `scale / ratio`, fibres at `angle` from the +column axis towards
    the +row axis; formed in float64 and rounded once"""
    angle, ratio, scale = (np.asarray(a, np.float64) for a in (angle, ratio, scale))
    shp = np.broadcast_shapes(angle.shape, ratio.shape, scale.shape, tuple(shape) if shape is not None else ())
    lon, tra = scale, scale / ratio
    c, s = np.cos(angle), np.sin(angle)
    planes = (lon * (s * s) + tra * (c * c), lon * (c * c) + tra * (s * s), (lon - tra) * (c * s))
    return tuple(np.ascontiguousarray(np.broadcast_to(p, shp), dtype=np.float32) for p in planes)


def fenton_substep(slab, dt, diff, dyy, dxx, dxy, phi=None):
    """one Fenton sub-step (fenton.py:101-106) with the tensor operator in laplace's place: [4, H, W] float32 -> the same"""
    import oracle
    U, V, W, S = (np.asarray(a, F) for a in slab)
    dU, dV, dW, dS = (np.asarray(d, F).reshape(U.shape) for d in oracle.fenton_diff(U, V, W, S))
    U0 = oracle.enforce_boundary(U)
    lap = laplace32(U0, dyy, dxx, dxy, phi)
    dtf, ddt = F(dt), F(float(diff) * float(dt))
    return np.stack([(U0 + dtf * dU) + ddt * lap, V + dtf * dV, W + dtf * dW, S + dtf * dS])
