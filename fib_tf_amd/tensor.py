"""Fibre fields: per-cell diffusion tensors D = [[dyy, dxy], [dxy, dxx]] (rows are y, columns are x), dimensionless and relative
to the model's `diff` — anisotropic and heterogeneous conduction (include/fibhip.h fibhip_set_tensor).

    dyy, dxx, dxy = fibre_tensor(angle, ratio, scale)       # angle, ratio, scale: scalars or [H, W] arrays
    model.set_tensor(dyy, dxx, dxy)                          # or model.set_fibres(angle, ratio, scale); before define()

Host side only: the planes, their checks (the library's own, in the same words) and the five weight planes as the device forms
them.  The operator itself runs on the device (csrc/stencil.hpp lap9_tensor, csrc/pointwise.inc tensor_prep_cell)."""
import warnings

import numpy as np

MONOTONE_RATIO = 3.0        # up to this anisotropy ratio every weight of the 9-point form is non-negative, at every angle
EIG_SLACK = 1e-6            # the library's: the planes are float32 roundings of a tensor whose largest eigenvalue is at most 1

NOT_FINITE = 'set_tensor: the tensor planes are not finite everywhere'
NOT_SPD = 'set_tensor: the tensor is not positive definite everywhere'
OVER_UNIT = 'set_tensor: the largest eigenvalue is above 1: the tensor is relative to diff (raise diff instead)'


def fibre_tensor(angle, ratio, scale=1.0, shape=None):
    """(dyy, dxx, dxy) as float32 planes for fibres at `angle` (radians from the +column axis towards the +row axis), with
    longitudinal over transverse diffusion `ratio` >= 1 and longitudinal diffusion `scale` in (0, 1] (transverse: scale / ratio).
    Each argument is a scalar or an [H, W] array; `shape` = (H, W) when all three are scalars.  Formed in float64, rounded once."""
    angle, ratio, scale = (np.asarray(a, np.float64) for a in (angle, ratio, scale))
    shp = np.broadcast_shapes(angle.shape, ratio.shape, scale.shape, tuple(shape) if shape is not None else ())
    if len(shp) != 2:
        raise ValueError('fibre_tensor: the planes are [H, W]: pass arrays of that shape, or shape=(H, W) (got %s)' % (shp,))
    if not (np.all(np.isfinite(angle)) and np.all(np.isfinite(ratio)) and np.all(np.isfinite(scale))):
        raise ValueError('fibre_tensor: angle, ratio and scale must be finite')
    if np.any(ratio < 1.0):
        raise ValueError('fibre_tensor: ratio is longitudinal over transverse diffusion, >= 1 (got %g)' % ratio.min())
    if np.any(scale <= 0.0) or np.any(scale > 1.0):
        raise ValueError('fibre_tensor: scale must be in (0, 1]: the tensor is relative to diff (raise diff instead)')
    lon, tra = scale, scale / ratio
    c, s = np.cos(angle), np.sin(angle)
    dxx = lon * (c * c) + tra * (s * s)
    dyy = lon * (s * s) + tra * (c * c)
    dxy = (lon - tra) * (c * s)
    return tuple(np.ascontiguousarray(np.broadcast_to(p, shp), dtype=np.float32) for p in (dyy, dxx, dxy))


def _planes(dyy, dxx, dxy, shape=None):
    planes = [np.asarray(p, np.float32) for p in (dyy, dxx, dxy)]
    if not (planes[0].ndim == 2 and planes[0].shape == planes[1].shape == planes[2].shape):
        raise ValueError('set_tensor: three [H, W] planes of one shape (got %s)' % ([p.shape for p in planes],))
    if shape is not None and planes[0].shape != tuple(shape):
        raise ValueError('set_tensor: the planes have shape %s, the grid is %s' % (planes[0].shape, tuple(shape)))
    return planes


def check_tensor(dyy, dxx, dxy, shape=None):
    """raises ValueError for planes the library refuses, in its words: not finite, not positive definite, or with a largest
    eigenvalue above 1 by more than rounding.  Returns the three planes as float32 arrays."""
    planes = _planes(dyy, dxx, dxy, shape)
    a, b, c = (p.astype(np.float64) for p in planes)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(c))):
        raise ValueError(NOT_FINITE)
    if not np.all((a > 0.0) & (b > 0.0) & (a * b - c * c > 0.0)):
        raise ValueError(NOT_SPD)
    if np.any(0.5 * (a + b) + np.sqrt(0.25 * (a - b) * (a - b) + c * c) > 1.0 + EIG_SLACK):
        raise ValueError(OVER_UNIT)
    return planes


def weights(dyy, dxx, dxy):
    """the five float32 weight planes (wy, wx, wa, wb, wc) exactly as the device forms them: one rounded operation per line,
    no contraction (csrc/stencil.hpp tensor_weights)"""
    dyy, dxx, dxy = _planes(dyy, dxx, dxy)
    f = np.float32
    wd = f(0.25) * (dyy + dxx)
    wy = f(1.5) * dyy - f(0.5) * dxx        # N, S
    wx = f(1.5) * dxx - f(0.5) * dyy        # W, E
    wa = wd + dxy                           # NW, SE
    wb = wd - dxy                           # NE, SW
    wc = f(12.0) * wd                       # centre
    return wy, wx, wa, wb, wc


def is_monotone(dyy, dxx, dxy):
    """are all weights non-negative (a monotone scheme: no over- or undershoot)?  True at every angle while the anisotropy
    ratio is at most 3; beyond that the operator is still consistent"""
    wy, wx, wa, wb, _ = weights(dyy, dxx, dxy)
    return bool(min(wy.min(), wx.min(), wa.min(), wb.min()) >= 0.0)


_warned = [False]


def warn_if_not_monotone(dyy, dxx, dxy):
    """once per process: a tensor with a negative weight (anisotropy ratio above 3 at an oblique angle)"""
    if not _warned[0] and not is_monotone(dyy, dxx, dxy):
        _warned[0] = True
        warnings.warn('fib_tf_amd: this diffusion tensor gives the 9-point operator a negative weight (an anisotropy ratio above %g at an '
                      'oblique angle): still a consistent discretisation, but no longer a monotone one — steep fronts may over- or '
                      'undershoot a little' % MONOTONE_RATIO, RuntimeWarning, stacklevel=3)


def refuse(model, who, why):
    """`who` does not go with a diffusion tensor: raises before anything reaches the library"""
    if getattr(model, 'tensor', None) is not None:
        raise ValueError('%s: not on a model with a diffusion tensor (set_tensor / set_fibres): %s' % (who, why))
