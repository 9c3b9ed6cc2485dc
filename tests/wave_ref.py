"""wave_ref — the wave recorder's definition (include/fibhip.h, fibhip_waves_*) restated in NumPy and plain Python, for the tests.

A cell is SET when the mask is non-zero there and the strict float32 compare(s) hold; set cells that touch under conn = 4 or 8
form a wave; its seed is the smallest linear index r * W + c among its cells.  Everything here is integer arithmetic on the
outcome of the compares, so the device has to agree bit for bit.  `label` is a union-find in plain Python that shares nothing
with the device's kernels (and is itself checked against scipy.ndimage.label in test_waves_cpu.py)."""
import numpy as np

RECORD_DTYPE = np.dtype([('seed', np.int32), ('area', np.int32), ('sum_r', np.int64), ('sum_c', np.int64),
                         ('r0', np.int32), ('r1', np.int32), ('c0', np.int32), ('c1', np.int32)])
FIELDS = RECORD_DTYPE.names


def _cond(X, kind, level):
    X = np.asarray(X, np.float32)
    level = np.float32(level)
    if kind not in ('above', 'below'):
        raise ValueError('kind is above or below')
    with np.errstate(invalid='ignore'):
        return X > level if kind == 'above' else X < level          # (a NaN compares false either way)


def set_plane(X, level, kind='above', mask=None, also=None):
    """the boolean plane of the set cells: `also` = (X2, kind2, level2) or None; `mask` non-zero where a cell counts, or None"""
    s = _cond(X, kind, level)
    if also is not None:
        s = s & _cond(also[0], also[1], also[2])
    if mask is not None:
        s = s & (np.asarray(mask) != 0)
    return s


def label(s, conn=4):
    """int32 [H, W]: the seed of the cell's wave, -1 where `s` is false"""
    if conn not in (4, 8):
        raise ValueError('conn is 4 or 8')
    s = np.asarray(s, bool)
    H, W = s.shape
    parent = list(range(H * W))

    def find(i):
        root = i
        while parent[root] != root:
            root = parent[root]
        while parent[i] != root:
            parent[i], i = root, parent[i]
        return root

    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if conn == 8 else [])
    cells = np.argwhere(s)
    for r, c in cells.tolist():
        i = r * W + c
        for dr, dc in back:
            rr, cc = r + dr, c + dc
            if 0 <= rr < H and 0 <= cc < W and s[rr, cc]:
                a, b = find(i), find(rr * W + cc)
                if a != b:
                    parent[max(a, b)] = min(a, b)                    # the smaller index stays the root: the seed
    out = np.full(H * W, -1, np.int32)
    for r, c in cells.tolist():
        out[r * W + c] = find(r * W + c)
    return out.reshape(H, W)


def measure(labels):
    """the records of a label plane, sorted by seed"""
    labels = np.asarray(labels)
    H, W = labels.shape
    flat = labels.ravel()
    idx = np.flatnonzero(flat >= 0)
    seeds, inv, area = np.unique(flat[idx], return_inverse=True, return_counts=True)
    out = np.zeros(len(seeds), RECORD_DTYPE)
    out['seed'] = seeds
    out['area'] = area
    r, c = (idx // W).astype(np.int64), (idx % W).astype(np.int64)
    np.add.at(out['sum_r'], inv, r)
    np.add.at(out['sum_c'], inv, c)
    out['r0'] = H
    out['c0'] = W
    out['r1'] = -1
    out['c1'] = -1
    np.minimum.at(out['r0'], inv, r.astype(np.int32))
    np.maximum.at(out['r1'], inv, r.astype(np.int32))
    np.minimum.at(out['c0'], inv, c.astype(np.int32))
    np.maximum.at(out['c1'], inv, c.astype(np.int32))
    return out


def sample(s, conn=4, max_waves=None):
    """(counts int32 [3] = n, stored, cells; records sorted by seed — ALL of them; labels) of one set plane"""
    lab = label(s, conn)
    rec = measure(lab)
    n = len(rec)
    stored = n if max_waves is None else min(n, int(max_waves))
    return np.array([n, stored, int(np.count_nonzero(s))], np.int32), rec, lab


def sorted_records(records, stored):
    """the first `stored` device records, sorted by seed"""
    r = np.asarray(records)[:int(stored)]
    return r[np.argsort(r['seed'], kind='stable')]
