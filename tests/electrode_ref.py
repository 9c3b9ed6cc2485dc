"""NumPy reference for the electrode recorder (include/fibhip.h fibhip_electrode_*): the exact (float64) weighted sums and
the error bound the header derives from the summation depth."""
import math

import numpy as np

U = 2.0 ** -24           # unit roundoff of float32


def depth(m):
    """D(m): the most float32 additions a term of an m-cell patch may pass through"""
    return math.ceil(m / 256) + 16


def gamma(d):
    """gamma_(d+1): d additions and one product rounding"""
    return (d + 1) * U / (1.0 - (d + 1) * U)


def weighted_sum(x, rect, patch):
    """(S, A): the float64 sum of patch * x over rect = (r0, r1, c0, c1), and the sum of |patch * x|"""
    r0, r1, c0, c1 = rect
    p = np.asarray(patch, np.float32).astype(np.float64) * np.asarray(x, np.float32)[r0:r1, c0:c1].astype(np.float64)
    return float(p.sum()), float(np.abs(p).sum())


def bound(x, rect, patch):
    """|trace - S| may not exceed this"""
    r0, r1, c0, c1 = rect
    return gamma(depth((r1 - r0) * (c1 - c0))) * weighted_sum(x, rect, patch)[1]


def pairwise_mean_bound(frame, mask):
    """the same kind of bound for np.mean(frame * mask) in float32 (NumPy's pairwise summation: D = ceil(log2(H * W)) + 8),
    before the division by H * W"""
    p = np.asarray(frame, np.float64) * np.asarray(mask, np.float64)
    return gamma(math.ceil(math.log2(p.size)) + 8) * float(np.abs(p).sum())
