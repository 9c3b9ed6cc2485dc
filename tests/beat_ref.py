"""NumPy restatement of the beat recorder's definition (include/fibhip.h, fibhip_beats_*).  The device must equal it bit for
bit.  Every operation is a float32 operation rounded on its own, in the order the header states; vectorised over the pixels,
sequential over the samples.

One remark on "bit for bit": a NaN the arithmetic makes (inf / inf under a sample of +-inf) carries the sign the machine gives
it — x86 and the GPU differ —, and IEEE 754 leaves it open.  `same()` compares every bit of every number, the sign of zero
included, and takes any NaN for any NaN."""
import numpy as np

import frame_ref

F32 = np.float32
NAN = F32(np.nan)


def pixel(X, window=None, block=(1, 1), reduce='mean', weight=None):
    """the sampled plane [oh, ow]: the frame recorder's pixel at lo = 0, span = 1"""
    return frame_ref.frame(X, window, block, reduce, 0.0, 1.0, weight)


def same(got, want):
    """same shape, same type, the same bits in every number; NaN equals NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != 'f':
        return got.tobytes() == want.tobytes()
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn)) and np.where(gn, 0, got).tobytes() == np.where(wn, 0, want).tobytes()


class Beats:
    """the recorder's state: made from the pixel plane at attach, fed the pixel plane of every sample, in order"""

    def __init__(self, pix0, up, down, depth, every, dt, steps_per_tick):
        self.xp = np.array(pix0, F32)
        self.up, self.down = F32(up), F32(down)
        assert self.down <= self.up
        self.depth, self.every = int(depth), int(every)
        assert 1 <= self.depth <= 16 and self.every >= 1
        self.dt, self.spt = float(dt), int(steps_per_tick)
        self.step = F32(float(self.every) * self.dt * self.spt)              # (float)((double)every * dt * spt)
        shape = self.xp.shape
        self.pk = np.full(shape, np.nan, F32)
        self.n = np.zeros(shape, np.int32)
        self.t_up = np.full((self.depth,) + shape, np.nan, F32)              # slot order: beat b in slot b % depth
        self.t_down = np.full((self.depth,) + shape, np.nan, F32)
        self.peak = np.full((self.depth,) + shape, np.nan, F32)
        self.s = 0

    def _put(self, plane, slot, where, value):
        """plane[slot[p], p] = value[p] at the pixels p of `where`"""
        idx = np.nonzero(where)
        plane[(slot[idx],) + idx] = np.broadcast_to(value, where.shape)[idx]

    def sample(self, pix):
        xc = np.asarray(pix, F32)
        assert xc.shape == self.xp.shape
        xp, up, down, pk, n, D = self.xp, self.up, self.down, self.pk, self.n, self.depth
        t0 = F32(float(self.s * self.every) * self.dt * self.spt)            # (float)((double)(s * every) * dt * spt)
        with np.errstate(all='ignore'):
            is_open = pk == pk
            rise = (xp < up) & (xc >= up)
            fall = (xp >= down) & (xc < down) & is_open & ~rise
            t_rise = t0 + ((up - xp) / (xc - xp)) * self.step
            t_fall = t0 + ((xp - down) / (xp - xc)) * self.step
            grown = np.where(xc > pk, xc, pk)
        assert t_rise.dtype == F32 and t_fall.dtype == F32
        prev_slot, slot = (n - 1) % D, n % D
        # 1. upstroke: a beat still open leaves its peak and no t_down; the new beat takes slot n mod depth
        self._put(self.peak, prev_slot, rise & is_open, pk)
        self._put(self.t_up, slot, rise, t_rise)
        self._put(self.t_down, slot, rise, NAN)
        self._put(self.peak, slot, rise, NAN)
        # 2. downstroke of an open beat
        self._put(self.t_down, prev_slot, fall, t_fall)
        self._put(self.peak, prev_slot, fall, pk)
        # 3. otherwise the running peak; then pk and n of the events
        new_pk = np.where(rise, xc, np.where(fall, NAN, np.where(is_open, grown, pk)))
        self.pk = new_pk.astype(F32)
        self.n = (n + rise).astype(np.int32)
        self.xp = xc.copy()
        self.s += 1

    def read(self):
        """(t_up, t_down, peak [depth, ...] in slot order, n, pk)"""
        return self.t_up.copy(), self.t_down.copy(), self.peak.copy(), self.n.copy(), self.pk.copy()

    def summary(self, last):
        return summary(self.t_up, self.t_down, self.n, last)


def summary(t_up, t_down, n, last):
    """(nused int32, apd_mean, cl_mean, apd_alt float32) over the newest `last` beats of ring planes in slot order"""
    t_up, t_down, n = np.asarray(t_up, F32), np.asarray(t_down, F32), np.asarray(n, np.int32)
    D = t_up.shape[0]
    assert 1 <= last <= D
    shape = n.shape
    cnt = n.astype(np.int64)
    b0 = np.maximum(0, np.maximum(cnt - np.minimum(cnt, D), cnt - last))

    def at(plane, b):
        return np.take_along_axis(plane, (b % D)[None], axis=0)[0]

    used, pairs, ncl = (np.zeros(shape, np.int32) for _ in range(3))
    tot, alt, cls = (np.zeros(shape, F32) for _ in range(3))
    before = np.full(shape, np.nan, F32)                     # the APD of beat b - 1 (NaN: none in the walk)
    with np.errstate(all='ignore'):
        for j in range(D):                                   # the walk's j-th beat, b = b0 + j, of every pixel that has one
            b = b0 + j
            valid = b < cnt
            apd = at(t_down, b) - at(t_up, b)
            num = valid & (apd == apd)
            tot = np.where(num, np.where(used == 0, apd, tot + apd), tot)
            pair = num & (before == before)
            d = apd - before
            term = np.where(b % 2 == 1, d, -d)
            alt = np.where(pair, np.where(pairs == 0, term, alt + term), alt)
            used = used + num
            pairs = pairs + pair
            before = np.where(valid, apd, before)
            if j >= 1:
                cl = at(t_up, b) - at(t_up, b - 1)
                cnum = valid & (cl == cl)
                cls = np.where(cnum, np.where(ncl == 0, cl, cls + cl), cls)
                ncl = ncl + cnum
        assert tot.dtype == F32 and alt.dtype == F32 and cls.dtype == F32
        apd_mean = np.where(used > 0, tot / used.astype(F32), NAN)
        cl_mean = np.where(ncl > 0, cls / ncl.astype(F32), NAN)
        apd_alt = np.where(pairs > 0, alt / pairs.astype(F32), NAN)
    assert apd_mean.dtype == F32 and cl_mean.dtype == F32 and apd_alt.dtype == F32
    return used.astype(np.int32), apd_mean, cl_mean, apd_alt


def sample_ticks(every, ticks):
    """the tick numbers (counted from 1 at attach) a sample follows, among the first `ticks` ticks"""
    return list(range(every, ticks + 1, every))
