"""NumPy restatement of the velocity fit's definition (include/fibhip.h, fibhip_beats_velocity / fibhip_observe_velocity /
fibhip_velocity_fit).  The device must equal it bit for bit: loops over the window's offsets and the ring's entries in the order
the header states, vectorised over the pixels; d is ONE float32 subtraction, the sums are float64 and every product and every
addition is an operation of its own (NumPy fuses nothing).  `same()` is beat_ref's: every bit of every number, any NaN for any
NaN.

`fit(..., trace=True)` also says which branches of the definition the input took, for the test that proves that the crafted
inputs of the GPU test take them all."""
import numpy as np

from beat_ref import same  # noqa: F401

F32 = np.float32
MAX_RADIUS = 4


def default_min_cells(radius):
    return (2 * int(radius) + 1) ** 2 // 2 + 1


def fit(t, count, back=0, radius=2, max_dt=20.0, min_cells=None, mask=None, trace=False):
    """t float32 [depth, oh, ow] in slot order, count int32 [oh, ow] -> (nfit int32, gy, gx, rms float32), each [oh, ow]"""
    t = np.asarray(t, F32)
    count = np.asarray(count, np.int32)
    depth, oh, ow = t.shape
    R = int(radius)
    max_dt = F32(max_dt)
    if min_cells is None:
        min_cells = default_min_cells(R)
    assert count.shape == (oh, ow) and 1 <= depth <= 16 and 0 <= back < depth and 1 <= R <= MAX_RADIUS
    assert np.isfinite(max_dt) and max_dt > 0 and 3 <= min_cells <= (2 * R + 1) ** 2
    n = count.astype(np.int64)
    if mask is not None:
        n = np.where(np.asarray(mask) != 0, n, 0)               # a pixel outside the mask holds nothing and takes no part
    held = np.clip(np.minimum(n, depth), 0, None)               # the beats n - held .. n - 1
    # the centre
    has = back < held
    b = np.where(has, n - 1 - back, 0)
    tc = np.where(has, np.take_along_axis(t, (b % depth)[None], axis=0)[0], F32(np.nan)).astype(F32)
    centre = tc == tc
    # the neighbours: outside the plane there is a pixel that holds nothing
    npad = np.pad(n, R, constant_values=0)
    hpad = np.pad(held, R, constant_values=0)
    tpad = np.pad(t, ((0, 0), (R, R), (R, R)), constant_values=np.nan)
    N, Sy, Sx, Syy, Sxx, Sxy = (np.zeros((oh, ow), np.int64) for _ in range(6))
    St, Syt, Sxt, Stt = (np.zeros((oh, ow), np.float64) for _ in range(4))
    ties = 0
    with np.errstate(invalid='ignore', over='ignore'):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                win = (slice(R + dy, R + dy + oh), slice(R + dx, R + dx + ow))
                nq, hq, tq = npad[win], hpad[win], tpad[(slice(None),) + win]
                best = np.full((oh, ow), np.inf, F32)
                bd = np.zeros((oh, ow), F32)
                for j in range(depth):                          # ascending beat number
                    walk = j < hq
                    slot = np.where(walk, (nq - hq + j) % depth, 0)
                    d = (np.take_along_axis(tq, slot[None], axis=0)[0] - tc).astype(F32)
                    ad = np.abs(d)
                    ties += int((walk & centre & (ad == best) & (ad <= max_dt)).sum())
                    keep = walk & (ad < best)                   # strict: a tie keeps the older beat; NaN compares false
                    best = np.where(keep, ad, best)
                    bd = np.where(keep, d, bd)
                used = centre & (best <= max_dt)
                dd = np.where(used, bd, F32(0)).astype(np.float64)
                u = used.astype(np.int64)
                N += u
                Sy += u * dy
                Sx += u * dx
                Syy += u * dy * dy
                Sxx += u * dx * dx
                Sxy += u * dy * dx
                # (a sum is never -0.0, so adding the +0.0 of a cell that is not used changes no bit)
                St = St + dd
                Syt = Syt + np.float64(dy) * dd
                Sxt = Sxt + np.float64(dx) * dd
                Stt = Stt + dd * dd
        cyy = N * Syy - Sy * Sy
        cxx = N * Sxx - Sx * Sx
        cxy = N * Sxy - Sy * Sx
        det = cyy * cxx - cxy * cxy
        ok = (N >= min_cells) & (det != 0)
        f = np.float64
        Nf = N.astype(f)
        cyt = Nf * Syt - Sy.astype(f) * St
        cxt = Nf * Sxt - Sx.astype(f) * St
        safe = np.where(ok, det, 1).astype(f)
        safe_n = np.where(ok, N, 1).astype(f)
        gy = (cxx.astype(f) * cyt - cxy.astype(f) * cxt) / safe
        gx = (cyy.astype(f) * cxt - cxy.astype(f) * cyt) / safe
        a = (St - (gy * Sy.astype(f) + gx * Sx.astype(f))) / safe_n
        sse = Stt - ((a * St + gy * Syt) + gx * Sxt)
        rms = np.sqrt(np.where(sse > 0.0, sse, 0.0) / safe_n)
        nan = F32(np.nan)
        out = (N.astype(np.int32), np.where(ok, gy.astype(F32), nan).astype(F32), np.where(ok, gx.astype(F32), nan).astype(F32),
               np.where(ok, rms.astype(F32), nan).astype(F32))
    if trace:
        return out, {'centre_missing': int((~centre).sum()), 'refused_for_n': int((centre & (N < min_cells)).sum()),
                     'refused_for_det': int((centre & (N >= min_cells) & (det == 0)).sum()), 'fitted': int(ok.sum()), 'ties': ties}
    return out


# ---- crafted rings: what no run would produce -------------------------------------------------------------------------------
# Times from a small set, so that exact ties (10 and 18 around 14), exact max_dt distances (8 ms: 10 .. 18, 18 .. 26) and
# windows on one line happen all the time; NaN and +-inf among them; counts of 0, below the depth and far above it.
CRAFTED_MAX_DT = 8.0
CRAFTED_TIMES = np.array([10, 12, 14, 14, 16, 18, 18, 26, 34, 50, np.nan, np.inf, -np.inf], F32)
CRAFTED_SHAPES = [(1, 1), (1, 7), (5, 3), (19, 70), (33, 129)]
CRAFTED_DEPTHS = (1, 3, 16)


def crafted(shape, depth, seed):
    """(t float32 [depth, oh, ow], count int32 [oh, ow], mask uint8 [oh, ow])"""
    rng = np.random.default_rng(1000 * seed + 16 * shape[0] + depth)
    t = rng.choice(CRAFTED_TIMES, (depth,) + tuple(shape)).astype(F32)
    # a smooth part, so that whole windows fit too: a front at 2 ms per column and 1 per row under the newest beats
    y, x = np.mgrid[:shape[0], :shape[1]]
    smooth = rng.random(shape) < 0.5
    t = np.where(smooth[None], (10 + (2 * x + y) % 8 + 32 * np.arange(depth).reshape(-1, 1, 1)).astype(F32), t)
    kind = rng.integers(0, 4, shape)
    count = np.select([kind == 0, kind == 1, kind == 2], [0, rng.integers(0, depth + 1, shape), depth + rng.integers(0, 4, shape)],
                      1000000007 + rng.integers(0, 64, shape)).astype(np.int32)
    count = np.where(rng.random(shape) < 0.7, np.maximum(count, 1), count).astype(np.int32)
    mask = (rng.random(shape) < 0.8).astype(np.uint8)
    return t, count, mask


def crafted_cases(shape):
    """the cases of one shape: depth 1, 3 and 16, R = 1 .. 4, back 0 and depth - 1, with and without a mask; min_cells the default
    without a mask and 3, the smallest, with it"""
    for depth in CRAFTED_DEPTHS:
        t, count, mask = crafted(shape, depth, 7)
        for radius in (1, 2, 3, 4):
            for back in sorted({0, depth - 1}):
                for m in (None, mask):
                    yield dict(t=t, count=count, back=back, radius=radius, max_dt=CRAFTED_MAX_DT,
                               min_cells=default_min_cells(radius) if m is None else 3, mask=m)


def fit_beats(t_up, count, last, **kw):
    """the maps of the newest `last` beats stacked in beats()'s order (index -1 the newest): what BeatRecorder.velocity returns"""
    maps = [fit(t_up, count, back=back, **kw) for back in range(int(last) - 1, -1, -1)]
    return {k: np.stack([m[i] for m in maps]) for i, k in enumerate(('nfit', 'gy', 'gx', 'rms'))}
