"""TEST INFRASTRUCTURE: the NumPy restatement of the tip recorder's definition (include/fibhip.h, fibhip_tips_*).

Exact integer arithmetic on float32 inputs: float32 subtractions of the levels, float64 cross products of float32 numbers
(both products exact, so the sign of the rounded difference is the exact sign), comparisons.  The device equals it bit for
bit, so no test that uses it needs a tolerance."""
import numpy as np


def charges(A, B, a0, b0, mask=None):
    """int32 [H-1, W-1]: the charge of every plaquette, upper-left cell (i, j); corners in the order
    (i,j) -> (i,j+1) -> (i+1,j+1) -> (i+1,j)"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        a = (A - np.float32(a0)).astype(np.float32)
        b = (B - np.float32(b0)).astype(np.float32)
        ca = [a[:-1, :-1], a[:-1, 1:], a[1:, 1:], a[1:, :-1]]
        cb = [b[:-1, :-1], b[:-1, 1:], b[1:, 1:], b[1:, :-1]]
        w = np.zeros(ca[0].shape, np.int32)
        for e in range(4):
            a1, b1 = ca[e].astype(np.float64), cb[e].astype(np.float64)
            a2, b2 = ca[(e + 1) % 4].astype(np.float64), cb[(e + 1) % 4].astype(np.float64)
            cross = a1 * b2 - a2 * b1
            w += ((b1 < 0) & (b2 >= 0) & (cross > 0)).astype(np.int32)
            w -= ((b2 < 0) & (b1 >= 0) & (cross < 0)).astype(np.int32)
    if mask is not None:
        m = np.asarray(mask) != 0
        w[~(m[:-1, :-1] & m[:-1, 1:] & m[1:, 1:] & m[1:, :-1])] = 0     # all four corners inside, or the plaquette does not count
    return w


def tips(A, B, a0, b0, mask=None):
    """(records, (n_pos, n_neg)): records int32 [n, 3] = row, column, charge of every tip, sorted by (row, column)"""
    w = charges(A, B, a0, b0, mask)
    rc = np.argwhere(w != 0)                                   # (row-major: sorted by row, then column)
    rec = np.concatenate([rc, w[w != 0][:, None]], axis=1).astype(np.int32).reshape(-1, 3)
    return rec, (int((w > 0).sum()), int((w < 0).sum()))


def sorted_records(records, stored, max_tips):
    """the valid records of one device sample ([max_tips, 4] in arrival order) as int32 [n, 3] sorted by (row, column)"""
    r = np.asarray(records)[:min(int(stored), int(max_tips))]
    assert np.all(r[:, 3] == 0)
    r = r[np.lexsort((r[:, 1], r[:, 0]))]
    return np.ascontiguousarray(r[:, :3], np.int32)
