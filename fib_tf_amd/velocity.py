"""velocity — conduction-velocity maps and CV restitution from the activation times the recorders keep on the device.

A plane is fitted to the activation times of a space-time window around every pixel (Bayly et al. 1998): the (2R + 1)^2
neighbours, each with the beat of its ring that lies closest in time to the centre's, and of those the ones within `max_dt`.
The fit runs on the device where the ring lies (include/fibhip.h, fibhip_beats_velocity / fibhip_observe_velocity; DESIGN.md
section 23); what comes back are four maps: `gy`, `gx` — the gradient of activation time in ms per pixel along rows and columns
—, `rms`, the residual of the fit in ms, and `nfit`, the cells that took part.  Where the fit breaks down (a collision, a line
of block, the tip of a spiral) fewer cells match in time and the residual grows: `nfit` and `rms` say where.  The definition is
exact and restated in NumPy in tests/velocity_ref.py.

    with model.record_beats(every=5, depth=8) as rec:
        for i in model.run():
            ...
        v = rec.velocity(last=2)                 # gy, gx, rms [2, oh, ow], nfit; index -1 the newest beat
        cv = rec.speed(last=1)[-1]               # cells per ms
        di, cv = rec.cv_restitution()            # every (DI, CV) pair of every pixel: the other half of the restitution pair

The functions here are the host's share: speed and direction from the gradient, and the pairing with the diastolic intervals."""
import numpy as np

MAX_RADIUS = 4                                   # include/fibhip.h FIBHIP_VEL_MAX_RADIUS
MAPS = ('nfit', 'gy', 'gx', 'rms')


def default_min_cells(radius):
    """a majority of the window: (2R + 1)^2 // 2 + 1"""
    return (2 * int(radius) + 1) ** 2 // 2 + 1


def check_args(radius, max_dt, min_cells=None, depth=None, last=None, who='velocity'):
    """the refusals that need no device: raises ValueError; returns (radius, max_dt as float32, min_cells)"""
    radius = int(radius)
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError('%s: radius must be 1 .. %d (got %d)' % (who, MAX_RADIUS, radius))
    with np.errstate(over='ignore'):
        max_dt = np.float32(max_dt)
    if not (np.isfinite(max_dt) and max_dt > 0):
        raise ValueError('%s: max_dt must be finite and > 0 (got %r)' % (who, float(max_dt)))
    min_cells = default_min_cells(radius) if min_cells is None else int(min_cells)
    if not 3 <= min_cells <= (2 * radius + 1) ** 2:
        raise ValueError('%s: min_cells must be 3 .. (2 * radius + 1)^2 = %d (got %d)' % (who, (2 * radius + 1) ** 2, min_cells))
    if last is not None and not 1 <= int(last) <= int(depth):
        raise ValueError('%s: last must be 1 .. depth = %d (got %d)' % (who, depth, last))
    return radius, max_dt, min_cells


def _gradient(v, block):
    by, bx = (float(b) for b in block)
    return np.asarray(v['gy'], np.float64) / by, np.asarray(v['gx'], np.float64) / bx      # ms per cell


def speed_of(v, block=(1, 1)):
    """float64, shaped like the maps: 1 / hypot(gy / by, gx / bx) in cells per ms, for maps of pixels of by x bx cells (NaN
    where there is no fit; inf where the times of the window do not change)"""
    gy, gx = _gradient(v, block)
    with np.errstate(divide='ignore'):
        return 1.0 / np.hypot(gy, gx)


def direction_of(v, block=(1, 1)):
    """float64: the direction the front travels in, atan2(rows, columns) of the gradient per cell — 0 along a row towards higher
    columns, pi / 2 down the columns towards higher rows"""
    gy, gx = _gradient(v, block)
    return np.arctan2(gy, gx)


def cv_restitution_of(beats, vel, block=(1, 1), mask=None, max_rms=None):
    """(di, cv): two flat float64 arrays, the pairs of every pixel (those of `mask`, a boolean map) and beat that has both a
    diastolic interval in front of it and a fit (with a residual of at most `max_rms` ms, if given).  `beats` is
    BeatRecorder.beats(), `vel` BeatRecorder.velocity(last) — its index -1 - j is the beats' index -1 - j"""
    from .beats import di_of
    cv = speed_of(vel, block)
    last = cv.shape[0]
    di = di_of(beats)[-last:]
    if di.shape != cv.shape:
        raise ValueError('cv_restitution: velocity maps of shape %s beside beats of shape %s' % (cv.shape, di_of(beats).shape))
    ok = np.isfinite(di) & np.isfinite(cv)
    if max_rms is not None:
        with np.errstate(invalid='ignore'):
            ok &= np.asarray(vel['rms'], np.float64) <= float(max_rms)
    if mask is not None:
        mask = np.asarray(mask, bool)
        if mask.shape != di.shape[1:]:
            raise ValueError('cv_restitution: a mask of shape %s on a map of shape %s' % (mask.shape, di.shape[1:]))
        ok &= mask[None]
    return di[ok], cv[ok]
