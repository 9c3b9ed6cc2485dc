"""NumPy restatement of the spectrum recorder's definition (include/fibhip.h, fibhip_spectrum_*).  The device must equal it
bit for bit.  Every operation is a float32 operation rounded on its own, in the order the header states; vectorised over the
pixels (and the bins), sequential over the samples."""
import numpy as np

import frame_ref

F32 = np.float32


def hann(N):
    """the periodic Hann window: 0.5 - 0.5 cos(2 pi n / N) in float64, rounded to float32"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(F32)


def rect(N):
    return np.ones(N, F32)


def twiddles(N):
    """tw[m] = (cos(2 pi m / N), -sin(2 pi m / N)), computed in float64 and then rounded to float32"""
    a = 2.0 * np.pi * np.arange(N) / N
    return np.stack([np.cos(a), -np.sin(a)], axis=1).astype(F32)


def pixel(X, window=None, block=(1, 1), reduce='mean', weight=None):
    """the sampled plane [oh, ow]: the frame recorder's pixel at lo = 0, span = 1"""
    return frame_ref.frame(X, window, block, reduce, 0.0, 1.0, weight)


class Spectrum:
    """the recorder's state: feed it the pixel plane of every sample, in order"""

    def __init__(self, shape, nfft, bins, win=None, tw=None, chunk=1):
        self.N = int(nfft)
        self.bins = [int(k) for k in bins]
        assert all(0 <= k <= self.N // 2 for k in self.bins) and all(a < b for a, b in zip(self.bins, self.bins[1:]))
        self.win = hann(self.N) if win is None else np.asarray(win, F32)
        self.tw = twiddles(self.N) if tw is None else np.asarray(tw, F32)
        assert self.win.shape == (self.N,) and self.tw.shape == (self.N, 2)
        self.chunk = int(chunk)
        assert 1 <= self.chunk <= 32 and self.N % self.chunk == 0
        nb = len(self.bins)
        self.re = np.zeros((nb,) + tuple(shape), F32)
        self.im = np.zeros_like(self.re)
        self.P = np.zeros_like(self.re)
        self.samples = 0
        self.segments = 0
        self.ring = []

    def sample(self, pix):
        pix = np.asarray(pix, F32)
        assert pix.shape == self.re.shape[1:]
        self.ring.append(pix.copy())
        self.samples += 1
        if self.samples % self.chunk == 0:
            self._fold()

    def _fold(self):
        s0 = self.samples - self.chunk
        k = np.array(self.bins, np.int64)
        with np.errstate(all='ignore'):
            for c, x in enumerate(self.ring):
                j = (s0 + c) % self.N
                y = x * self.win[j]
                m = (k * j) % self.N                               # integer arithmetic, 64 bits wide here
                cr = self.tw[m, 0][:, None, None]
                ci = self.tw[m, 1][:, None, None]
                self.re = self.re + y[None] * cr
                self.im = self.im + y[None] * ci
                assert y.dtype == F32 and self.re.dtype == F32 and self.im.dtype == F32
                if j == self.N - 1:
                    self.P = self.P + ((self.re * self.re) + (self.im * self.im))
                    self.re = np.zeros_like(self.re)
                    self.im = np.zeros_like(self.im)
                    self.segments += 1
        assert self.P.dtype == F32
        self.ring = []

    def read(self):
        """(P [nb, oh, ow] float32, segments): the samples of an unfinished segment are in neither"""
        return self.P.copy(), self.segments

    def count(self):
        return self.samples, self.samples // self.N

    def peak(self, a, b, halfwidth):
        return peak(self.P, self.segments, a, b, halfwidth)


def peak(P, segments, a, b, halfwidth):
    """(kpeak int32, ppeak, pband, pnear float32), each [oh, ow], over the bin positions a <= i <= b"""
    P = np.asarray(P, F32)
    assert 0 <= a <= b < P.shape[0] and halfwidth >= 0
    shape = P.shape[1:]
    kp = np.full(shape, -1, np.int32)
    best = np.full(shape, np.nan, F32)
    with np.errstate(all='ignore'):
        if segments > 0:
            for i in range(a, b + 1):
                p = P[i]
                take = np.where(kp < 0, p == p, p > best)          # the first P that is a number, then strictly greater ones
                best = np.where(take, p, best)
                kp = np.where(take, np.int32(i), kp)
        pband = P[a].copy()
        for i in range(a + 1, b + 1):
            pband = pband + P[i]
        lo = np.maximum(a, kp - halfwidth)
        hi = np.minimum(b, kp + halfwidth)
        pnear = np.full(shape, np.nan, F32)
        for i in range(a, b + 1):
            inside = (kp >= 0) & (i >= lo) & (i <= hi)
            pnear = np.where(inside & (i == lo), P[i], np.where(inside, pnear + P[i], pnear))
    assert best.dtype == F32 and pband.dtype == F32 and pnear.dtype == F32
    return kp, best, pband, pnear


def sample_ticks(every, ticks):
    """the tick numbers (counted from 1 at attach) a sample follows, among the first `ticks` ticks"""
    return list(range(every, ticks + 1, every))
