"""NumPy restatement of the stimulus program (include/fibhip.h fibhip_stim_*): what one entry does to one array, when an entry
is due, and a whole program applied to a state at one tick.  The device must equal this bit for bit.

    MAX   X = np.fmax(X, S)                         ADD   X = X + S   (float32, one rounding)
A cell whose S is the mode's "untouched" value (-inf for MAX, +0 or -0 for ADD) keeps its bits, whatever they are."""
import numpy as np

MODES = ('max', 'add')


def untouched(mode):
    return np.float32(-np.inf) if mode == 'max' else np.float32(0.0)


def rect_plane(H, W, r0, r1, c0, c1, v, floor):
    """S of a rectangle: v inside rows [r0, r1) x columns [c0, c1), `floor` outside"""
    s = np.full((H, W), floor, np.float32)
    s[r0:r1, c0:c1] = np.float32(v)
    return s


def apply(x, s, mode):
    """one entry on one array: x, s float32 [H, W] -> the new array"""
    x = np.asarray(x, np.float32)
    s = np.asarray(s, np.float32)
    assert mode in MODES and x.shape == s.shape
    with np.errstate(all='ignore'):
        new = np.fmax(x, s) if mode == 'max' else (x + s).astype(np.float32)
    keep = s == untouched(mode)                                 # (+0 == -0; a NaN in S is not "untouched")
    return np.where(keep, x, new).astype(np.float32)


def box(s, mode):
    """(r0, r1, c0, c1) of the cells of plane `s` that are not "untouched", or (0, 0, 0, 0): what the host cuts at attach"""
    hit = ~(np.asarray(s, np.float32) == untouched(mode))
    if not hit.any():
        return (0, 0, 0, 0)
    rows, cols = np.flatnonzero(hit.any(axis=1)), np.flatnonzero(hit.any(axis=0))
    return (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1)


def due(entry, k):
    """is the entry applied right after tick k (k = 0 is the first tick after attach)?  entry: dict with first, period, count,
    hold"""
    first, period, count, hold = (int(entry.get(n, d)) for n, d in (('first', 0), ('period', 0), ('count', 1), ('hold', 1)))
    m = k - first
    if m < 0:
        return False
    if period == 0:
        return m < hold
    return m % period < hold and (count == 0 or m // period < count)


def events(entries, n_ticks):
    """[(tick, entry index)] of the first n_ticks ticks, by tick, ties in program order"""
    return [(k, i) for k in range(n_ticks) for i, e in enumerate(entries) if due(e, k)]


def plane_of(entry, planes, H, W):
    if entry.get('shape', 'rect') in ('rect', 0):
        return rect_plane(H, W, entry['r0'], entry['r1'], entry['c0'], entry['c1'], entry['v'], entry['floor'])
    return np.asarray(planes[entry['plane']], np.float32)


def apply_tick(state, entries, planes, k):
    """the entries due after tick k, in program order, on a state [nvar, H, W] (a copy is returned)"""
    state = np.array(state, np.float32, copy=True)
    _, H, W = state.shape
    for e in entries:
        if due(e, k):
            mode = e.get('mode', 'max')
            mode = MODES[mode] if isinstance(mode, int) else mode
            var = int(e.get('var', 0))
            state[var] = apply(state[var], plane_of(e, planes, H, W), mode)
    return state
