"""TEST INFRASTRUCTURE: the NumPy restatement of the statistics recorder's definition (include/fibhip.h, fibhip_stats_*).

`sample(states, cols, weight, mask)` is one row in float64.  SUM is the EXACT sum (math.fsum over the float64 products, each
of which is exact: two float32 factors); the device's float64 tree is held to the order-free bound `sum_bound`.  Everything
else is plain NumPy and must be met exactly."""
import math

import numpy as np

KINDS = ('sum', 'min', 'max', 'below', 'above', 'nonfinite')


def _kind(k):
    return k if isinstance(k, str) else KINDS[int(k)]


def terms(x, weight):
    """the float64 products w * x of the cells with w != 0 (w = 1 without a plane), row-major"""
    x = np.asarray(x, np.float32).astype(np.float64).ravel()
    if weight is None:
        return x
    w = np.asarray(weight, np.float32).astype(np.float64).ravel()
    keep = w != 0
    with np.errstate(all='ignore'):
        return w[keep] * x[keep]


def exact_sum(x, weight):
    t = terms(x, weight)
    if not np.all(np.isfinite(t)):                           # a NaN or Inf under a non-zero weight propagates
        with np.errstate(all='ignore'):
            return float(np.sum(t))
    return math.fsum(t.tolist())


def sum_bound(x, weight):
    """|any float64 summation of the n terms - their exact sum| <= n * 2^-53 * sum |term| (to first order; n * u << 1 here)"""
    t = terms(x, weight)
    return len(t) * 2.0 ** -53 * math.fsum(np.abs(t).tolist())


def value(x, kind, level=0.0, weight=None, mask=None):
    kind = _kind(kind)
    x = np.asarray(x, np.float32)
    if kind == 'sum':
        return exact_sum(x, weight)
    sel = x.ravel() if mask is None else x.ravel()[np.asarray(mask).ravel() != 0]
    if kind in ('min', 'max'):
        sel = sel[~np.isnan(sel)]
        if sel.size == 0:                                    # no cell qualifies (an empty mask, or NaN only)
            return float('inf') if kind == 'min' else float('-inf')
        return float(sel.min() if kind == 'min' else sel.max())
    with np.errstate(invalid='ignore'):
        if kind == 'below':
            return float(np.count_nonzero(sel < np.float32(level)))
        if kind == 'above':
            return float(np.count_nonzero(sel > np.float32(level)))
    return float(np.count_nonzero(~np.isfinite(sel)))


def sample(states, cols, weight=None, mask=None):
    """states: [nvar, H, W] float32 (or anything indexable by var); cols: [(var, kind, level)] -> float64 [ncols]"""
    return np.array([value(states[var], kind, level, weight, mask) for var, kind, level in cols], np.float64)


def sample_ticks(nticks, every):
    """the ticks k (counted from 0 at attach) after which a sample is taken: (k + 1) % every == 0"""
    return [k for k in range(nticks) if (k + 1) % every == 0]
