"""spectrum — per-cell power spectra and dominant-frequency maps folded on the device while a model runs.

The dominant-frequency (DF) map and its regularity index answer at what rate each cell is being driven.  Computed from the
movie cube they need every frame kept (1 MiB per sample at 512 x 512); `SpectrumRecorder` has the library fold a per-cell Welch
periodogram on the device instead: every `every` ticks one pixel plane is sampled, every `chunk` samples `spectrum_fold_kernel`
adds them to the running DFT sums of the recorded bins, every `nfft` samples a segment ends and its power is added to P.  Only
the maps come back.  The definition is exact (include/fibhip.h, fibhip_spectrum_*; restated in NumPy in
tests/spectrum_ref.py): segments of `nfft` samples without overlap and without detrending, a window the caller supplies."""
import numpy as np

from ._recorder import DeviceRecorder, attach, check_every, tick_ms, weight_plane

MAX_BINS, MAX_CHUNK, MIN_NFFT, MAX_NFFT = 128, 32, 4, 65536      # include/fibhip.h FIBHIP_SPECTRUM_*


def hann(N):
    """the periodic Hann window, float32: with it a constant leaks into bins 0 and +-1 only"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(N)) / int(N))).astype(np.float32)


def window_table(window, N):
    """`window` ('hann': periodic Hann; 'rect'; or an array of N numbers) as the float32 table the library takes"""
    if isinstance(window, str):
        if window == 'hann':
            return hann(N)
        if window == 'rect':
            return np.ones(int(N), np.float32)
        raise ValueError("record_spectrum: window is 'hann', 'rect' or an array of nfft = %d numbers" % N)
    w = np.ascontiguousarray(window, np.float32)
    if w.shape != (int(N),):
        raise ValueError('record_spectrum: a window of shape %s for nfft = %d' % (w.shape, N))
    return w


def twiddle_table(N):
    """[N, 2] float32: cos(2 pi m / N) and -sin(2 pi m / N), computed in float64 and then rounded"""
    a = 2.0 * np.pi * np.arange(int(N)) / int(N)
    return np.ascontiguousarray(np.stack([np.cos(a), -np.sin(a)], axis=1).astype(np.float32))


def bin_hz(nfft, every, tick_ms):
    """the spacing of the frequency indices in Hz: 1 / (N * every * tick_ms * 1e-3)"""
    return 1.0 / (int(nfft) * int(every) * float(tick_ms) * 1e-3)


def freqs_of(bins, nfft, every, tick_ms):
    """Hz per recorded bin: k / (N * every * tick_ms * 1e-3)"""
    return np.asarray(bins, np.float64) * bin_hz(nfft, every, tick_ms)


def default_chunk(nfft):
    """the largest divisor of nfft that is at most 16"""
    return max(c for c in range(1, 17) if int(nfft) % c == 0)


def bins_from_band(fmin, fmax, nfft, every, tick_ms):
    """the frequency indices k with fmin <= f_k <= fmax (Hz); without fmin the band starts at k = 2, above the leakage of a
    constant under the periodic Hann window; without fmax it ends at N / 2"""
    df = bin_hz(nfft, every, tick_ms)
    k0 = 2 if fmin is None else max(0, int(np.ceil(float(fmin) / df - 1e-9)))
    k1 = int(nfft) // 2 if fmax is None else min(int(nfft) // 2, int(np.floor(float(fmax) / df + 1e-9)))
    if k1 < k0:
        raise ValueError('record_spectrum: no frequency index between %r and %r Hz (the indices are %g Hz apart, up to %g Hz)'
                         % (fmin, fmax, df, df * (int(nfft) // 2)))
    if k1 - k0 + 1 > MAX_BINS:
        raise ValueError('record_spectrum: %d frequency indices between %r and %r Hz, at most %d are recorded: narrow the band '
                         'or pass bins' % (k1 - k0 + 1, fmin, fmax, MAX_BINS))
    return list(range(k0, k1 + 1))


def check_args(every, nfft, bins, chunk, block, reduce):
    """the refusals that need no device: raises ValueError"""
    check_every('record_spectrum', every)
    if not MIN_NFFT <= int(nfft) <= MAX_NFFT:
        raise ValueError('record_spectrum: nfft must be %d .. %d (got %d)' % (MIN_NFFT, MAX_NFFT, nfft))
    if not 1 <= int(chunk) <= MAX_CHUNK or int(nfft) % int(chunk):
        raise ValueError('record_spectrum: chunk must be 1 .. %d and divide nfft = %d (got %d)' % (MAX_CHUNK, nfft, chunk))
    bins = [int(k) for k in bins]
    if not 1 <= len(bins) <= MAX_BINS:
        raise ValueError('record_spectrum: 1 .. %d bins (got %d)' % (MAX_BINS, len(bins)))
    if any(k < 0 or k > int(nfft) // 2 for k in bins):
        raise ValueError('record_spectrum: a bin is a frequency index in [0, nfft / 2 = %d]' % (int(nfft) // 2))
    if any(a >= b for a, b in zip(bins, bins[1:])):
        raise ValueError('record_spectrum: the bins must be strictly ascending')
    if reduce not in ('point', 'mean'):
        raise ValueError("record_spectrum: reduce is 'point' or 'mean'")
    if len(block) != 2 or not all(1 <= int(b) <= 16 for b in block):
        raise ValueError('record_spectrum: a block is 1 .. 16 cells each way')
    return bins


def band_positions(freqs, fmin=None, fmax=None, bins=None):
    """(a, b): the first and last recorded position whose frequency lies in [fmin, fmax] Hz.  Without fmin the band starts at
    the first recorded bin with frequency index >= 2 (`bins`: the indices; a constant leaks into 0 and 1 under the Hann window)"""
    freqs = np.asarray(freqs, np.float64)
    ok = np.ones(len(freqs), bool)
    if fmin is not None:
        ok &= freqs >= float(fmin) * (1 - 1e-12)
    elif bins is not None:
        ok &= np.asarray(bins) >= 2
    if fmax is not None:
        ok &= freqs <= float(fmax) * (1 + 1e-12)
    at = np.flatnonzero(ok)
    if len(at) == 0:
        raise ValueError('no recorded bin between %r and %r Hz' % (fmin, fmax))
    return int(at[0]), int(at[-1])


def dominant_from_maps(kpeak, pband, pnear, freqs, power=None, refine=False):
    """(df_hz, regularity) float64 from the peak maps: the frequency of the recorded bin at position kpeak and pnear / pband,
    NaN where kpeak = -1.  `refine` (needs `power` [nb, oh, ow]): parabolic interpolation through the peak and its two
    neighbouring positions where both are recorded and one frequency index away"""
    kpeak = np.asarray(kpeak)
    freqs = np.asarray(freqs, np.float64)
    ok = kpeak >= 0
    at = np.where(ok, kpeak, 0)
    df = np.where(ok, freqs[at], np.nan)
    with np.errstate(all='ignore'):
        reg = np.where(ok, np.asarray(pnear, np.float64) / np.asarray(pband, np.float64), np.nan)
        if refine:
            if power is None:
                raise ValueError('refine=True needs the power')
            P = np.asarray(power, np.float64)
            nb = P.shape[0]
            if nb >= 3:
                inner = ok & (at >= 1) & (at <= nb - 2)
                i0 = np.clip(at, 1, nb - 2)
                even = inner & np.isclose(freqs[i0] - freqs[i0 - 1], freqs[i0 + 1] - freqs[i0])
                yy, xx = np.indices(kpeak.shape)
                l, c, r = P[i0 - 1, yy, xx], P[i0, yy, xx], P[i0 + 1, yy, xx]
                den = l - 2.0 * c + r
                delta = np.where(even & (den < 0), 0.5 * (l - r) / den, 0.0)
                step = freqs[i0 + 1] - freqs[i0]
                df = np.where(even, df + np.clip(delta, -0.5, 0.5) * step, df)
    return df, reg


class SpectrumRecorder(DeviceRecorder):
    """per-cell power spectra folded on the device; see `IonicModel.record_spectrum`.

        with model.record_spectrum(every=10, nfft=128, fmin=2, fmax=30) as rec:
            for i in model.run():
                ...
            df_hz, regularity = rec.dominant_frequency()

    `power()` returns float64 [nb, oh, ow], the mean periodogram over the finished segments; `freqs()` the Hz of each recorded
    bin.  There is no detrending: with the periodic Hann window a constant leaks into bins 0 and +-1 only, so the band defaults
    to the frequency indices >= 2."""
    NOUN, END = 'spectrum recorder', 'spectrum_end'

    def __init__(self, model, every=10, nfft=128, fmin=None, fmax=None, bins=None, window='hann', chunk=None, var=0, block=(1, 1),
                 reduce='mean', region=None, weight=None):
        self._st = st = attach(model, 'record_spectrum', 'spectra are recorded')
        self.every, self.nfft, self.var = int(every), int(nfft), int(var)
        self.tick_ms = tick_ms(model)
        self.chunk = default_chunk(self.nfft) if chunk is None else int(chunk)
        self.block = tuple(int(b) for b in block)
        self.reduce = reduce
        if bins is None:
            check_args(self.every, self.nfft, [0], self.chunk, self.block, reduce)
            bins = bins_from_band(fmin, fmax, self.nfft, self.every, self.tick_ms)
        self.bins = check_args(self.every, self.nfft, bins, self.chunk, self.block, reduce)
        self.window = (0, model.height, 0, model.width) if region is None else tuple(int(v) for v in region)
        self.win = window_table(window, self.nfft)
        self.tw = twiddle_table(self.nfft)
        self.weight = weight = weight_plane(model, weight, 'record_spectrum')
        st.spectrum_begin(self.var, self.window, self.block, self.reduce, weight, self.every, self.nfft, self.win, self.tw, self.bins,
                          self.chunk)
        oh, ow, _ = st.spectrum_shape()
        self.shape = (oh, ow)
        self.open = True

    def freqs(self):
        """float64 [nb]: Hz per recorded bin, k / (nfft * every * tick_ms * 1e-3)"""
        return freqs_of(self.bins, self.nfft, self.every, self.tick_ms)

    def samples(self):
        """samples taken since the recorder was attached"""
        self._check()
        return self._st.spectrum_count()[0]

    def segments(self):
        """segments of nfft samples finished since the recorder was attached"""
        self._check()
        return self._st.spectrum_count()[1]

    def raw(self):
        """(P float32 [nb, oh, ow], segments): the sum over the finished segments of |DFT|^2 at each recorded bin"""
        self._check()
        return self._st.spectrum_read()

    def power(self):
        """float64 [nb, oh, ow]: P / segments (NaN before the first segment has ended)"""
        P, seg = self.raw()
        with np.errstate(all='ignore'):
            return P.astype(np.float64) / np.float64(seg)

    def peak_maps(self, fmin=None, fmax=None, halfwidth=1):
        """(kpeak int32, ppeak, pband, pnear float32), each [oh, ow], over the recorded bins between fmin and fmax (Hz; default:
        every recorded bin with frequency index >= 2): the position of the largest P (the lowest on a tie, -1 where there is
        none), P there, the sum of P over the band and over the positions within `halfwidth` of the peak"""
        self._check()
        a, b = band_positions(self.freqs(), fmin, fmax, self.bins)
        return self._st.spectrum_peak(a, b, int(halfwidth))

    def dominant_frequency(self, fmin=None, fmax=None, halfwidth=1, refine=False):
        """(df_hz, regularity) float64 [oh, ow]: the frequency of the largest peak in the band and the share pnear / pband of the
        band's power within `halfwidth` positions of it; NaN where no segment has ended.  `refine`: parabolic interpolation of
        the peak on the host"""
        kpeak, _, pband, pnear = self.peak_maps(fmin, fmax, halfwidth)
        power = self.raw()[0] if refine else None
        return dominant_from_maps(kpeak, pband, pnear, self.freqs(), power, refine)
