"""-m gpu: the spectrum recorder (include/fibhip.h fibhip_spectrum_*, fib_tf_amd/spectrum.py) on the device.

The power planes and the peak maps must EQUAL the NumPy restatement (tests/spectrum_ref.py) fed with the state read back after
every sample tick, bit for bit: no tolerance anywhere in this file.  The grids are the smallest that reach each path: 37 x 53
(one pixel per thread, odd everything), 64 x 64 (16-byte loads and stores), 20 x 130 (rows not 16-byte aligned), 96 x 100
(several tiles, multi-tick launches) and one 512 x 512 case (many workgroups)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref as ref  # noqa: E402
import tip_ref  # noqa: E402
from test_gpu_tips import MAKERS, fenton, court  # noqa: E402

pytestmark = pytest.mark.gpu

PLAN_ENV = ('FIBHIP_MT', 'FIBHIP_AHEAD', 'FIBHIP_MT_FAKE_GIVEUP', 'FIBHIP_VARIANT', 'FIBHIP_MT_MAX', 'FIBHIP_MT_IDS', 'FIBHIP_AUTOTUNE')
VARIANT_96x100 = '10,44,25,-3'                              # the forced small shape of tests/test_gpu_recovery.py: 12 tiles
PACE_V = {'fenton': 1.0, 'br': 10.0, 'court': 20.0, 'traced': 1.0}
N, BINS, CHUNKS = 12, [0, 1, 2, 3, 5, 6], (1, 3, 4, 12)
SAMPLES = 2 * N + 5                                         # two segments and five samples of a third


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), '%s: %d of %d values differ' % (what, int((got != want).sum()), got.size)


def same_maps(got, want, what):
    """the four peak maps; NaN (no peak) equals NaN"""
    for name, g, w in zip(('kpeak', 'ppeak', 'pband', 'pnear'), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.dtype, w.dtype)
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == 'f'), '%s %s: %d of %d values differ' % (what, name, int((g != w).sum()), g.size)


def wave(m, kind):
    """an S1 wave on its way (define()'s own columns) and a second one from a stimulus in the middle, a few ticks old"""
    st = m._stepper
    H, W = m.height, m.width
    st.pace(H // 3, H // 3 + 7, W // 3, W // 3 + 9, PACE_V[kind], float(m.min_v))
    for i in range(4):
        if kind == 'court' and i == 0:
            m.fire_op('slow')
        st.step(1)
    st.sync()


def variants(H, W):
    """(region, block, reduce, weighted, window): full resolution on the whole grid under the Hann window; a block mean of a
    weighted window that starts at an odd column, under no window; the upper-left cells of 4 x 4 blocks"""
    return [(None, (1, 1), 'mean', False, 'hann'), ((1, H, 5, W - 2), (2, 3), 'mean', True, 'rect'), ((0, H, 4, W), (4, 4), 'point', True, 'hann'),
            ((0, H, 0, W), (1, 1), 'point', True, 'rect')]


def attach(st, every, chunk, region, block, reduce, weight, window, nfft=N, bins=BINS):
    win = ref.hann(nfft) if window == 'hann' else ref.rect(nfft)
    st.spectrum_begin(0, region, block, reduce, weight, every, nfft, win, ref.twiddles(nfft), bins, chunk)
    return win


def check_configs(m, kind, H, W, everys=(1, 3), which=None):
    """every variant at every stride: the first chunk length is stepped one tick per call and read back after every sample — the
    restatement is fed from those states —, the others start from the same state again and run in ONE call: all four must
    give the restatement's bytes"""
    st = m._stepper
    rng = np.random.default_rng(H * 1000 + W)
    plane = rng.uniform(0.05, 1.0, (H, W)).astype(np.float32)
    state0 = st.get_state(-1).copy()
    n = varied = 0
    for every in everys:
        for vi, (region, block, reduce, weighted, window) in enumerate(variants(H, W)):
            if which is not None and vi not in which:
                continue
            weight = plane if weighted else None
            want = None
            for chunk in CHUNKS:
                what = '%s %dx%d every %d chunk %d region %s block %s %s weight %s %s' % (kind, H, W, every, chunk, region, block, reduce,
                                                                                        weighted, window)
                st.set_state(-1, state0)
                win = attach(st, every, chunk, region, block, reduce, weight, window)
                oh, ow, nb = st.spectrum_shape()
                assert nb == len(BINS)
                if want is None:
                    r = ref.Spectrum((oh, ow), N, BINS, win=win, chunk=chunk)
                    for i in range(SAMPLES * every):
                        st.step(1)
                        if (i + 1) % every == 0:
                            r.sample(ref.pixel(st.get_state(0), region, block, reduce, weight))
                    want = r
                else:
                    st.step(SAMPLES * every)
                assert st.spectrum_count() == (SAMPLES, 2), what            # the five samples are counted ...
                P, seg = st.spectrum_read()
                assert seg == 2 and want.segments == 2
                same(P, want.P, what)                                       # ... and show nowhere
                for a, b, hw in ((0, nb - 1, 1), (2, nb - 1, 2), (3, 3, 1), (1, 4, 0)):
                    same_maps(st.spectrum_peak(a, b, hw), ref.peak(P, seg, a, b, hw), '%s peak %d..%d +-%d' % (what, a, b, hw))
                st.spectrum_end()
                n += 1
            varied += len(np.unique(want.P)) > 10
    assert n > 0 and varied > 0                                             # (the planes are not constants)
    return n


@pytest.mark.parametrize('shape', [(37, 53), (64, 64), (20, 130)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_power_equals_the_restatement(gpu_lib, kind, shape):
    H, W = shape
    m = MAKERS[kind](H, W)
    wave(m, kind)
    # (the stock Fenton model takes every variant; the others the two that differ most)
    n = check_configs(m, kind, H, W, which=None if kind == 'fenton' else (0, 1))
    print('%s %dx%d: %d configurations' % (kind, H, W, n))
    m._stepper.close()


def test_multi_tick_launches(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    m = fenton(96, 100)
    wave(m, 'fenton')
    check_configs(m, 'fenton', 96, 100, everys=(3,), which=(0, 1))
    assert m._stepper.launch_stats()['mt_launches'] > 0
    m._stepper.close()


def test_many_workgroups(gpu_lib):
    """512 x 512 under a 4 x 4 mean, eight bins, one segment of 16 samples and three more"""
    m = fenton(512, 512)
    wave(m, 'fenton')
    st = m._stepper
    bins = [0, 1, 2, 3, 4, 5, 7, 8]
    win = attach(st, 1, 8, None, (4, 4), 'mean', None, 'hann', nfft=16, bins=bins)
    assert st.spectrum_shape() == (128, 128, 8)
    r = ref.Spectrum((128, 128), 16, bins, win=win, chunk=8)
    for i in range(19):
        st.step(1)
        r.sample(ref.pixel(st.get_state(0), None, (4, 4), 'mean', None))
    P, seg = st.spectrum_read()
    assert seg == 1 and st.spectrum_count() == (19, 1)
    same(P, r.P, '512x512')
    same_maps(st.spectrum_peak(2, 7, 1), r.peak(2, 7, 1), '512x512 peak')
    assert len(np.unique(P)) > 100
    st.close()


def test_other_arrays_and_no_segment_yet(gpu_lib):
    """var != 0 on a bare handle with noise in every array; before the first segment ends there is no peak anywhere"""
    st = gpu_lib.Stepper(gpu_lib.FENTON4V, 64, 64, 0.1, 1.3, flags=gpu_lib.FAST)
    rng = np.random.default_rng(2)
    st.set_state(-1, rng.uniform(0, 1, (4, 64, 64)).astype(np.float32))
    for var in (2, 3):
        st.spectrum_begin(var, (8, 56, 4, 60), (2, 2), 'mean', None, 1, 4, ref.hann(4), ref.twiddles(4), [0, 1, 2], 2)
        r = ref.Spectrum((24, 28), 4, [0, 1, 2], chunk=2)
        for i in range(3):
            st.step(1)
            r.sample(ref.pixel(st.get_state(var), (8, 56, 4, 60), (2, 2), 'mean', None))
        assert st.spectrum_count() == (3, 0)
        P, seg = st.spectrum_read()
        assert seg == 0 and not P.any()
        kp, pp, pb, pn = st.spectrum_peak(0, 2, 1)
        assert (kp == -1).all() and np.isnan(pp).all() and np.isnan(pn).all() and (pb == 0).all()
        st.step(1)
        r.sample(ref.pixel(st.get_state(var), (8, 56, 4, 60), (2, 2), 'mean', None))
        P, seg = st.spectrum_read()
        assert seg == 1
        same(P, r.P, 'var %d' % var)
        same_maps(st.spectrum_peak(0, 2, 1), r.peak(0, 2, 1), 'var %d peak' % var)
        st.spectrum_end()
    st.close()


def _plan_run(gpu_lib, monkeypatch, env, record, every=10, nfft=8, chunk=4, ticks=80):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')                                         # (plan selection happens at the first tick)
    plane = np.random.default_rng(4).uniform(0.1, 1, (96, 100)).astype(np.float32)
    out = None
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        s0 = st.launch_stats()
        if record:
            st.spectrum_begin(0, None, (2, 2), 'mean', plane, every, nfft, ref.hann(nfft), ref.twiddles(nfft), [0, 1, 2, 4], chunk)
        st.step(ticks)
        if record:
            assert st.spectrum_count() == (ticks // every, ticks // every // nfft)
        s1 = st.launch_stats()                                # (before the reads: spectrum_peak is a launch of its own)
        if record:
            out = st.spectrum_read()[0], st.spectrum_peak(0, 3, 1)
        state = st.get_state(-1)
        fb = st.fallbacks()
    st.close()
    return out, state, fb, {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}


def test_launch_count_and_plan_independence(gpu_lib, monkeypatch):
    (P, maps), state, fb, stats = _plan_run(gpu_lib, monkeypatch, {}, True)
    assert fb[0] == 0
    # between two samples the handle runs the fewest launches `every` allows: eight ten-tick launches, eight samples, two folds
    assert stats['ticks'] == 80 and stats['mt_ticks'] == 80 and stats['mt_launches'] == 8, stats
    assert stats['launches'] == 8 + 8 + 2, stats
    assert P.shape == (4, 48, 50) and len(np.unique(P)) > 100
    for env in ({'FIBHIP_MT': '0'}, {'FIBHIP_AHEAD': '0'}, {'FIBHIP_MT_FAKE_GIVEUP': '2'}):
        (P2, maps2), st2, fb2, stats2 = _plan_run(gpu_lib, monkeypatch, env, True)
        same(P2, P, str(env))
        same_maps(maps2, maps, str(env))
        assert st2.tobytes() == state.tobytes(), env
        assert stats2['ticks'] == 80, (env, stats2)
        if 'FIBHIP_MT_FAKE_GIVEUP' in env:
            assert fb2[0] == 1 and fb2[1] > 0, fb2            # one launch gave up and was recovered
        if 'FIBHIP_MT' in env:
            assert stats2['mt_ticks'] == 0
    _, plain, _, pstats = _plan_run(gpu_lib, monkeypatch, {}, False)
    assert plain.tobytes() == state.tobytes()                 # the recorder changes nothing of the state
    assert pstats['ticks'] == 80 and pstats['mt_ticks'] > 0


def _all(gpu_lib, which, ticks=60):
    """electrodes every 3, tips every 4, frames every 5 ticks, a spectrum every 2 and a stimulus program (those named in
    `which`) on one Fenton handle, one call"""
    from fib_tf_amd import egm
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    _, var2, a0, b0 = m.tip_signals
    rect, patch = egm.crop_mask(egm.create_mask(m, 60, 40, 5))
    # the stimuli are always there — they change the state every recorder sees —: events after ticks 7, 27, 47 (27 + 1 = 28 is a
    # sample tick of the tips and the spectrum: the sample comes before the stimulus)
    st.stim_begin([dict(var=0, mode='max', shape='rect', r0=70, r1=80, c0=10, c1=30, v=1.0, floor=-np.inf, first=7, period=20, count=3)])
    s0 = st.launch_stats()
    if 'el' in which:
        st.electrode_begin(0, [rect], [patch], 3, ticks // 3)
    if 'tip' in which:
        st.tips_begin(0, var2, a0, b0, None, 4, 256, ticks // 4)
    if 'fr' in which:
        st.frames_begin(0, (0, 96, 0, 100), (2, 2), 'mean', 0.0, 1.0, None, 'uint8', 5, 5, ticks // 5)
    if 'sp' in which:
        st.spectrum_begin(0, None, (2, 2), 'mean', None, 2, 10, ref.hann(10), ref.twiddles(10), [1, 2, 3], 5)
    st.step(ticks)
    out = {}
    if 'el' in which:
        out['el'] = st.electrode_read().tobytes()
    if 'tip' in which:
        c, r = st.tips_read()
        out['tip'] = (c.tobytes(), [tip_ref.sorted_records(r[s], c[s, 2], 256).tobytes() for s in range(len(c))])
    if 'fr' in which:
        out['fr'] = st.frames_read().tobytes()
    if 'sp' in which:
        P, seg = st.spectrum_read()
        assert seg == 3 and st.spectrum_count() == (30, 3) and len(np.unique(P)) > 100
        out['sp'] = P.tobytes()
    assert st.stim_count() == 3
    out['state'] = st.get_state(-1).tobytes()
    s1 = st.launch_stats()
    st.close()
    return out, {k: s1[k] - s0[k] for k in s0 if k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}


def test_beside_the_other_recorders_and_a_stimulus_program(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    everything, stats = _all(gpu_lib, ('el', 'tip', 'fr', 'sp'))
    assert stats['ticks'] == 60, stats
    for which in ('el', 'tip', 'fr', 'sp'):
        alone, _ = _all(gpu_lib, (which,))
        assert alone[which] == everything[which], which       # each records what it records alone
        assert alone['state'] == everything['state'], which


def test_court_sample_of_a_slow_array_is_taken_before_slow(gpu_lib):
    """a sample of a slow array due at the tick 'slow' would ride on: the two are not fused, the sample holds the array as the
    tick left it"""
    from fib_tf_amd.court import Courtemanche
    slow_var = Courtemanche.tip_signals[1]                    # a gate 'slow' assigns
    twin = court(64, 80)
    wave(twin, 'court')
    states = []
    for s in range(4):
        twin._stepper.step(5)
        states.append(twin._stepper.get_state(slow_var).copy())
        twin.fire_op('slow')
    assert states[0].tobytes() != twin._stepper.get_state(slow_var).tobytes()
    twin._stepper.close()
    m = court(64, 80)
    wave(m, 'court')
    st = m._stepper
    st.spectrum_begin(slow_var, None, (1, 1), 'mean', None, 5, 4, ref.rect(4), ref.twiddles(4), [0, 1, 2], 2)
    r = ref.Spectrum((64, 80), 4, [0, 1, 2], win=ref.rect(4), chunk=2)
    for s in range(4):
        st.step(5)                                            # (the last tick may be held back for 'slow' to ride on)
        m.fire_op('slow')
        r.sample(ref.pixel(states[s]))
    P, seg = st.spectrum_read()
    assert seg == 1
    same(P, r.P, 'slow array')
    st.close()


def test_refusals(gpu_lib):
    import ctypes as C
    from fib_tf_amd._lib import _fp, _ip
    m = fenton(64, 80)
    st = m._stepper
    L, h = st._L, st._h
    win, tw = ref.hann(12), ref.twiddles(12)

    def begin(handle=h, var=0, window=(0, 64, 0, 80), by=1, bx=1, reduce=1, every=1, nfft=12, bins=(0, 1, 2), chunk=4):
        w = np.ascontiguousarray(window, np.intc)
        b = np.ascontiguousarray(bins, np.intc)
        return L.fibhip_spectrum_begin(handle, var, w.ctypes.data_as(_ip), by, bx, reduce, None, every, nfft, win.ctypes.data_as(_fp),
                                       tw.ctypes.data_as(_fp), len(b), b.ctypes.data_as(_ip), chunk)
    for kw in (dict(var=-1), dict(var=st.nvar), dict(window=(0, 65, 0, 80)), dict(window=(4, 4, 0, 80)), dict(by=0), dict(bx=17),
               dict(reduce=2), dict(every=0), dict(nfft=3), dict(nfft=65537), dict(chunk=5), dict(chunk=0), dict(chunk=33),
               dict(bins=(0, 7)), dict(bins=(-1, 2)), dict(bins=(2, 2)), dict(bins=(3, 1)), dict(bins=()), dict(bins=tuple(range(129)))):
        assert begin(**kw) != 0, kw
        assert b'spectrum_begin' in L.fibhip_last_error(), kw
    k = C.c_longlong()
    assert L.fibhip_spectrum_count(h, C.byref(k), None) != 0 and b'no recorder' in L.fibhip_last_error()
    assert begin() == 0
    assert begin() != 0 and b'attached already' in L.fibhip_last_error()         # a second attach
    assert st.spectrum_count() == (0, 0)                      # the refused calls left the recorder attached
    for a, b, hw in ((-1, 2, 1), (2, 1, 1), (0, 3, 1), (0, 2, -1)):
        assert L.fibhip_spectrum_peak(h, a, b, hw, None, None, None, None) != 0 and b'spectrum_peak' in L.fibhip_last_error()
    assert L.fibhip_spectrum_end(h) == 0 and L.fibhip_spectrum_end(h) == 0      # end without begin: nothing
    st.step_edges()
    assert begin() != 0 and b'open tick' in L.fibhip_last_error()
    st.step_interior()
    st.step_commit()
    assert begin(handle=None) != 0
    st.close()
    blk = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 80, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    assert begin(handle=blk._h, window=(0, 42, 0, 80)) == -1 and b'row block' in L.fibhip_last_error()
    blk.close()
    inter = gpu_lib.Stepper(gpu_lib.FENTON4V, 64, 80, 0.1, 1.3, flags=gpu_lib.FAST | gpu_lib.ROW_INTERLEAVED)
    assert begin(handle=inter._h) == -1 and b'row-interleaved' in L.fibhip_last_error()
    inter.close()
    with pytest.raises(ValueError):
        m.record_spectrum(nfft=12, chunk=5)


def test_timeline_lists_the_sample_and_the_fold(gpu_lib):
    m = fenton(96, 130)
    st = m._stepper
    st.step(1)
    st.spectrum_begin(0, None, (1, 1), 'mean', None, 1, 4, ref.hann(4), ref.twiddles(4), [1, 2], 2)
    names = [e['name'] for _ in range(2) for e in st.trace_tick()]
    assert names.count('spectrum_sample_kernel') == 2 and names.count('spectrum_fold_kernel') == 1, names
    assert st.spectrum_count() == (2, 0)
    st.close()


def test_paced_sheet_has_its_pacing_rate_everywhere(gpu_lib):
    """the CPU suite's physics check on the device, through the public interface: Fenton 64 x 64 from rest, columns 0-5 paced
    to 1.0 every 300 ticks by a stimulus program; every cell peaks at frequency index 4 with a regularity above 0.7"""
    from fib_tf_amd.fenton import Fenton4v
    from fib_tf_amd.stimulus import Stimulus
    m = Fenton4v({'height': 64, 'width': 64, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 2400})
    m.define(s1=False)
    with m.program_stimuli([Stimulus((0, 64, 0, 6), 1.0, at_tick=0, period=300, count=0, floor=0.0)]):
        with m.record_spectrum(every=10, nfft=120, bins=list(range(41))) as rec:
            assert rec.chunk == 15 and rec.shape == (64, 64)
            m._stepper.step(2400)
            assert (rec.samples(), rec.segments()) == (240, 2)
            kp, pp, pb, pn = rec.peak_maps(halfwidth=1)
            assert (kp == 4).all()                            # positions == frequency indices here; the band is 2 .. 40
            df, reg = rec.dominant_frequency()
            assert np.allclose(df, 4 / (120 * 10 * rec.tick_ms * 1e-3)) and reg.min() > 0.7, (reg.min(), reg.max())
            power = rec.power()
            assert power.shape == (41, 64, 64) and (power[4] > power[5:].max(axis=0)).all()
    m._stepper.close()
