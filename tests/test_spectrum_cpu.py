"""the spectrum recorder's definition (tests/spectrum_ref.py) checked against a float64 DFT within its derived rounding bound,
against itself over the chunk lengths, on the literal edge cases of the peak maps, and on a paced sheet computed by the CPU
oracle; the Python layer's frequency axis, dominant-frequency maps and refusals.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref as ref  # noqa: E402

from fib_tf_amd import spectrum as sp  # noqa: E402

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_constants_match_the_binding():
    from fib_tf_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(FIBHIP_SPECTRUM_\w+)\s+(\d+)', hdr)}
    assert defs == {'FIBHIP_SPECTRUM_MAX_BINS': 128, 'FIBHIP_SPECTRUM_MAX_CHUNK': 32, 'FIBHIP_SPECTRUM_MIN_NFFT': 4,
                    'FIBHIP_SPECTRUM_MAX_NFFT': 65536}
    assert (_lib.SPECTRUM_MAX_BINS, _lib.SPECTRUM_MAX_CHUNK, _lib.SPECTRUM_MIN_NFFT, _lib.SPECTRUM_MAX_NFFT) == (128, 32, 4, 65536)
    assert (sp.MAX_BINS, sp.MAX_CHUNK, sp.MIN_NFFT, sp.MAX_NFFT) == (128, 32, 4, 65536)
    for name in ('begin', 'count', 'shape', 'read', 'peak', 'end'):
        assert 'fibhip_spectrum_' + name in _lib.SYMBOLS and re.search(r'\bint fibhip_spectrum_%s\(' % name, hdr)
    assert _lib.FRAME_REDUCE == ('point', 'mean')            # the recorder's `reduce` is the frame recorder's enum


def test_tables_are_float64_rounded_once():
    for N in (4, 12, 120, 128):
        a = 2.0 * np.pi * np.arange(N) / N
        assert np.array_equal(ref.twiddles(N), np.stack([np.cos(a), -np.sin(a)], 1).astype(F32))
        assert np.array_equal(sp.twiddle_table(N), ref.twiddles(N)) and sp.twiddle_table(N).flags.c_contiguous
        assert np.array_equal(sp.window_table('hann', N), ref.hann(N)) and ref.hann(N)[0] == 0
        assert np.array_equal(sp.window_table('rect', N), np.ones(N, F32))
    w = np.linspace(0, 1, 12)
    assert np.array_equal(sp.window_table(w, 12), w.astype(F32))


@pytest.mark.parametrize('N,window', [(12, 'hann'), (12, 'rect'), (120, 'hann'), (128, 'hann'), (250, 'rect')])
def test_ref_against_a_float64_dft_within_the_derived_bound(N, window):
    """Per Re and Im: |float32 fold - exact DFT of the float32 samples under the exact window| <= gamma * sum_s |x_s win_s|,
    gamma = (N + 4) u / (1 - (N + 4) u), u = 2^-24: one rounding each for the window entry, the twiddle entry, y and the
    product, and N - 1 additions"""
    rng = np.random.default_rng(N)
    shape = (5, 7)
    x = rng.uniform(-1.5, 2.5, (N,) + shape).astype(F32)
    bins = sorted(set([0, 1, 2, 3, N // 4, N // 2 - 1, N // 2]))
    win32 = ref.hann(N) if window == 'hann' else ref.rect(N)
    s = ref.Spectrum(shape, N, bins, win=win32, chunk=1)
    re_im = None
    for j in range(N):
        if j == N - 1:                                       # Re and Im as they stand in front of the segment's last sample ...
            pre = (s.re.copy(), s.im.copy())
        s.sample(x[j])
    # ... plus that sample, by the definition's own two operations (the fold has squared and cleared them by now)
    y = x[N - 1] * s.win[N - 1]
    m = (np.array(bins) * (N - 1)) % N
    re_im = (pre[0] + y[None] * s.tw[m, 0][:, None, None], pre[1] + y[None] * s.tw[m, 1][:, None, None])
    assert re_im[0].dtype == F32
    n = np.arange(N, dtype=np.float64)
    win64 = 0.5 - 0.5 * np.cos(2 * np.pi * n / N) if window == 'hann' else np.ones(N)
    xw = x.astype(np.float64) * win64[:, None, None]
    u = 2.0 ** -24
    gamma = (N + 4) * u / (1 - (N + 4) * u)
    bound = gamma * np.abs(xw).sum(axis=0)
    for i, k in enumerate(bins):
        ang = 2 * np.pi * ((k * np.arange(N)) % N) / N
        want_re = (xw * np.cos(ang)[:, None, None]).sum(axis=0)
        want_im = (xw * -np.sin(ang)[:, None, None]).sum(axis=0)
        assert (np.abs(re_im[0][i].astype(np.float64) - want_re) <= bound).all()
        assert (np.abs(re_im[1][i].astype(np.float64) - want_im) <= bound).all()
    P, seg = s.read()
    assert seg == 1 and P.dtype == F32
    assert P.tobytes() == ((re_im[0] * re_im[0]) + (re_im[1] * re_im[1])).tobytes()
    assert not s.re.any() and not s.im.any() and not np.signbit(s.re).any()


def test_chunk_changes_no_byte():
    rng = np.random.default_rng(12)
    shape = (3, 4)
    x = rng.uniform(-1, 1, (29,) + shape).astype(F32)        # 2 segments + 5 samples
    got = []
    for chunk in (1, 3, 4, 12):
        s = ref.Spectrum(shape, 12, [0, 1, 2, 3, 5, 6], chunk=chunk)
        for v in x:
            s.sample(v)
        P, seg = s.read()
        assert seg == 2 and s.count() == (29, 2)
        got.append(P.tobytes())
    assert len(set(got)) == 1
    only2 = ref.Spectrum(shape, 12, [0, 1, 2, 3, 5, 6], chunk=1)
    for v in x[:24]:
        only2.sample(v)
    assert only2.read()[0].tobytes() == got[0]               # the 5 samples of the unfinished segment show nowhere


def test_peak_ties_nan_and_empty():
    nan = np.nan
    P = np.array([[1, 5, 5, 2],          # a tie: the lowest position wins
                  [nan, 3, nan, 4],      # NaN never compares: skipped, also as the first term
                  [nan, nan, nan, nan],  # no number at all
                  [0, 0, 0, 0],          # all equal: the first
                  [7, 1, 2, 3]], F32).T.reshape(4, 1, 5)
    kp, pp, pb, pn = ref.peak(P, 1, 0, 3, 1)
    assert kp.dtype == np.int32 and kp.tolist() == [[1, 3, -1, 0, 0]]
    assert pp.tolist()[0][:2] == [5, 4] and np.isnan(pp[0, 2]) and pp[0, 3] == 0 and pp[0, 4] == 7
    assert pb[0, 0] == 13 and np.isnan(pb[0, 1]) and np.isnan(pb[0, 2]) and pb[0, 3] == 0 and pb[0, 4] == 13
    assert pn[0, 0] == 11 and np.isnan(pn[0, 1]) and np.isnan(pn[0, 2]) and pn[0, 3] == 0 and pn[0, 4] == 8      # (clipped at a)
    # halfwidth 0: pnear is ppeak; a one-bin band
    kp0, pp0, _, pn0 = ref.peak(P, 1, 0, 3, 0)
    assert kp0.tolist() == kp.tolist() and pn0[0, 0] == 5 and pn0[0, 4] == 7 and pn0[0, 1] == 4
    kp1, pp1, pb1, pn1 = ref.peak(P, 1, 2, 2, 1)
    assert kp1.tolist() == [[2, -1, -1, 2, 2]] and pb1[0, 0] == 5 and pn1[0, 0] == 5 and np.isnan(pp1[0, 1]) and np.isnan(pn1[0, 1])
    # no segment finished: no peak anywhere, the band sum is the sum of what is there
    kpe, ppe, pbe, pne = ref.peak(np.zeros((4, 1, 5), F32), 0, 0, 3, 1)
    assert (kpe == -1).all() and np.isnan(ppe).all() and np.isnan(pne).all() and (pbe == 0).all()
    # the sums are float32 sums in ascending order from the first term
    Q = np.array([1e8, 1, 1, 1], F32).reshape(4, 1, 1)
    assert ref.peak(Q, 1, 0, 3, 3)[2][0, 0] == F32(1e8) and ref.peak(Q, 1, 1, 3, 3)[2][0, 0] == 3


def test_freqs_and_bands():
    # every 10 ticks of 1 ms, 128 samples: 1.28 s per segment
    f = sp.freqs_of([2, 3, 64], 128, 10, 1.0)
    assert np.allclose(f, np.array([2, 3, 64]) / 1.28)
    assert sp.bins_from_band(None, None, 128, 10, 1.0) == list(range(2, 65))
    assert sp.bins_from_band(2.0, 10.0, 128, 10, 1.0) == list(range(3, 13))
    assert sp.bins_from_band(0.0, 1.0, 128, 10, 1.0) == [0, 1]
    assert sp.default_chunk(128) == 16 and sp.default_chunk(120) == 15 and sp.default_chunk(12) == 12 and sp.default_chunk(17) == 1
    with pytest.raises(ValueError):
        sp.bins_from_band(0.1, 0.2, 128, 10, 1.0)
    with pytest.raises(ValueError):
        sp.bins_from_band(None, None, 1024, 10, 1.0)        # 511 indices: more than are recorded
    assert sp.band_positions(f, None, None, [2, 3, 64]) == (0, 2)
    assert sp.band_positions(sp.freqs_of([0, 1, 2, 5], 128, 10, 1.0), None, None, [0, 1, 2, 5]) == (2, 3)
    assert sp.band_positions(f, 2.0, 3.0) == (1, 1)
    with pytest.raises(ValueError):
        sp.band_positions(f, 100.0, 200.0)


def test_dominant_frequency_on_synthetic_power():
    freqs = sp.freqs_of([2, 3, 4, 5, 6], 120, 10, 1.0)
    P = np.zeros((5, 2, 2), F32)
    P[:, 0, 0] = [1, 2, 8, 2, 1]                             # symmetric about position 2
    P[:, 0, 1] = [1, 2, 8, 4, 1]                             # leaning to the right
    P[:, 1, 0] = [9, 1, 1, 1, 1]                             # the peak at the band's edge
    kp, pp, pb, pn = ref.peak(P, 1, 0, 4, 1)
    kp[1, 1] = -1
    df, reg = sp.dominant_from_maps(kp, pb, pn, freqs)
    assert df[0, 0] == freqs[2] and df[0, 1] == freqs[2] and df[1, 0] == freqs[0] and np.isnan(df[1, 1]) and np.isnan(reg[1, 1])
    assert reg[0, 0] == 12 / 14 and reg[0, 1] == 14 / 16 and reg[1, 0] == 10 / 13
    dfr, _ = sp.dominant_from_maps(kp, pb, pn, freqs, power=P, refine=True)
    step = freqs[1] - freqs[0]
    assert dfr[0, 0] == freqs[2] and dfr[1, 0] == freqs[0] and np.isnan(dfr[1, 1])
    assert np.isclose(dfr[0, 1], freqs[2] + 0.5 * (2 - 4) / (2 - 16 + 4) * step) and freqs[2] < dfr[0, 1] < freqs[2] + 0.5 * step


def test_refusals_of_the_python_layer():
    ok = dict(every=1, nfft=12, bins=[0, 1, 2], chunk=4, block=(1, 1), reduce='mean')
    assert sp.check_args(**ok) == [0, 1, 2]
    for bad in (dict(every=0), dict(nfft=3), dict(nfft=65537), dict(chunk=5), dict(chunk=0), dict(nfft=64, chunk=64), dict(bins=[]),
                dict(bins=list(range(129)), nfft=512), dict(bins=[0, 7]), dict(bins=[-1, 2]), dict(bins=[2, 2]), dict(bins=[3, 1]),
                dict(reduce='max'), dict(block=(0, 1)), dict(block=(1, 17))):
        with pytest.raises(ValueError):
            sp.check_args(**dict(ok, **bad))
    with pytest.raises(ValueError):
        sp.window_table('hamming', 12)
    with pytest.raises(ValueError):
        sp.window_table(np.ones(11), 12)
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'width': 16, 'height': 16, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 10})
    with pytest.raises(AssertionError):
        m.record_spectrum()                                  # before define()


def test_paced_sheet_has_its_pacing_rate_everywhere():
    """Fenton 64 x 64 from rest, columns 0-5 paced to 1.0 every 300 ticks (MAX, floored at 0 elsewhere: what `pace` does); a
    sample every 10 ticks, N = 120: a segment is 1200 ticks = 4 pacing cycles, so every cell peaks at frequency index 4"""
    import oracle
    H = W = 64
    slab = np.zeros((4, H, W), F32)
    slab[1] = slab[2] = 1
    s = ref.Spectrum((H, W), 120, list(range(41)), chunk=12)
    for k in range(2400):
        oracle.fenton_run(slab, 0.1, 1.5, None, 10)
        if (k + 1) % 10 == 0:
            s.sample(ref.pixel(slab[0]))
        if k % 300 == 0:
            slab[0] = oracle.pace(slab[0], 0, H, 0, 6, 1.0, 0.0)
    assert s.count() == (240, 2)
    kp, pp, pb, pn = s.peak(2, 40, 1)
    assert (kp == 4).all()
    reg = pn.astype(np.float64) / pb.astype(np.float64)
    assert reg.min() > 0.7
    df, reg2 = sp.dominant_from_maps(kp, pb, pn, sp.freqs_of(range(41), 120, 10, 1.0))
    assert np.allclose(df, 4 / 1.2) and np.array_equal(reg2, reg)
