"""The lesion program restated in NumPy (include/fibhip.h, fibhip_lesion_*): site -> box and patch, the update of the phase field,
and the event list.  Written from the definition, not from fib_tf_amd/lesions.py, which the tests compare against it.

    phi[r, c] = max(phi[r, c] * m[r - r0, c - c0], float32(1e-5))      for the cells of the box, in float32

An entry with tick t is applied right after tick t of the loop (tick 0 is the first tick after attach); entries due after the
same tick are applied in program order."""
import numpy as np

FLOOR = np.float32(1e-5)
# two overlapping discs (row, col, radius) whose order matters on a 70 x 130 grid with hole_field(): their outer tails overlap
# each other and the outer tail of the hole, where phi is just below 1, so (phi * a) * b and (phi * b) * a round differently in
# some cells (on a field of ones the two products commute).  All three factors are close to 1 there, so the field stays as
# gentle as one hole's edge (|dphi| / 4 phi <= 1.81): discs pushed INTO the hole's rim multiply steep tails into a slope no
# explicit step survives — true of two overlapping holes of the reference as well — and a test on a blown-up state shows
# nothing.  Asserted in tests/test_lesions_cpu.py; the GPU tests apply them on one tick in this order
ORDER_PAIR = (('disc', 40, 72, 3), ('disc', 46, 74, 3))


def hole_field(H=70, W=130, x=90, y=40, radius=9):
    """the field of a model with one hole, add_hole_to_phase_field's expression (ionic.py:83-105)"""
    return np.maximum(np.ones((H, W), np.float32) * disc_plane(H, W, y, x, radius), 1e-5)


def disc_plane(H, W, row, col, radius):
    """the mask add_hole_to_phase_field(x=col, y=row, radius) multiplies in: float64 0.5 * (tanh(dist - radius) + 1) as float32"""
    cols = np.arange(W)[np.newaxis, :] - col
    rows = np.arange(H)[:, np.newaxis] - row
    return np.array(0.5 * (np.tanh(np.hypot(cols, rows) - radius) + 1.0), dtype=np.float32)


def line_plane(H, W, r0, c0, r1, c1, halfwidth):
    """the same edge profile on the distance to the segment (r0, c0) - (r1, c1), cell by cell"""
    out = np.empty((H, W), np.float64)
    a, d = np.array([r0, c0], np.float64), np.array([r1 - r0, c1 - c0], np.float64)
    for r in range(H):
        for c in range(W):
            p = np.array([r, c], np.float64) - a
            t = min(1.0, max(0.0, float(p @ d) / float(d @ d))) if float(d @ d) > 0 else 0.0
            q = p - t * d
            out[r, c] = np.hypot(q[1], q[0])
    return np.array(0.5 * (np.tanh(out - halfwidth) + 1.0), dtype=np.float32)


def plane_of(H, W, site):
    if isinstance(site, tuple) and site[0] == 'disc':
        return disc_plane(H, W, *site[1:])
    if isinstance(site, tuple) and site[0] == 'line':
        return line_plane(H, W, *site[1:])
    return np.asarray(site, np.float32)


def crop(plane):
    """(box, patch): the bounding box (r0, r1, c0, c1) of the factors that are not exactly 1.0f; None when there is none"""
    rr, cc = np.nonzero(plane != np.float32(1.0))
    if rr.size == 0:
        return None
    box = (int(rr.min()), int(rr.max()) + 1, int(cc.min()), int(cc.max()) + 1)
    return box, plane[box[0]:box[1], box[2]:box[3]].copy()


def patch(H, W, site):
    return crop(plane_of(H, W, site))


def apply_host(phase, box, m):
    r0, r1, c0, c1 = box
    out = np.array(phase, np.float32)
    for r in range(r0, r1):
        for c in range(c0, c1):
            out[r, c] = max(np.float32(out[r, c] * np.float32(m[r - r0, c - c0])), FLOOR)
    return out


def apply_sites(phase, H, W, sites):
    """the sites applied in order, each with its own floor"""
    for s in sites:
        phase = apply_host(phase, *patch(H, W, s))
    return phase


def events(ticks, n_ticks):
    """[(tick, entry index)] of the first n_ticks ticks, from a tick-by-tick walk: program order within a tick"""
    return [(k, i) for k in range(int(n_ticks)) for i, t in enumerate(ticks) if t == k]
