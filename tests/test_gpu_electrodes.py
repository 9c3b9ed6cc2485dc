"""-m gpu: the electrode recorder (include/fibhip.h fibhip_electrode_*, fib_tf_amd/egm.py) on the device.

Every sample is checked against the float64 weighted sum over the state read back at the same tick, within the bound the
header derives from the summation depth (tests/electrode_ref.py: derived, not measured); traces must not depend on the
launch plan, bit for bit; multi-tick launches must survive between two samples; and the book-keeping of the trace
(capacity, windows, refusals, re-attachment) is exercised call by call.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import electrode_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

PLAN_ENV = ('FIBHIP_MT', 'FIBHIP_AHEAD', 'FIBHIP_MT_FAKE_GIVEUP', 'FIBHIP_VARIANT')


def fenton(h, w, duration=1000):
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': h, 'width': w, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': duration})
    m.define()
    m.add_pace_op('s2', 'luq', 1.0)
    return m


def br(h, w, duration=1000):
    from fib_tf_amd.br import BeelerReuter
    m = BeelerReuter({'height': h, 'width': w, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 0.809, 'duration': duration,
                      'cheby': True, 'skip': False})
    m.define()
    m.add_pace_op('s2', 'luq', 10.0)
    return m


def court(h, w, duration=1000):
    from fib_tf_amd.court import Courtemanche
    m = Courtemanche({'height': h, 'width': w, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 0.809, 'duration': duration})
    m.define()
    m.add_pace_op('s2', 'luq', 20.0)
    return m


def traced(h, w, duration=1000):
    from traced_cases import make_model
    m = make_model('ap', h, w)
    m.duration = duration
    m.define()
    m.add_pace_op('s2', 'luq', 1.0)
    m._ensure_compiled()                                      # (a traced model builds its handle on first use)
    return m


MAKERS = {'fenton': fenton, 'br': br, 'court': court, 'traced': traced}


def three_electrodes(m):
    """(rects, patches): an interior Gaussian, one clipped by the edge, one whole-grid patch of both signs"""
    from fib_tf_amd import egm
    rng = np.random.default_rng(4)
    pairs = [egm.crop_mask(egm.create_mask(m, m.width // 2, m.height // 2, 5)),
             egm.crop_mask(egm.create_mask(m, 2, m.height - 3, 4)),
             ((0, m.height, 0, m.width), rng.uniform(-1, 1, (m.height, m.width)).astype(np.float32))]
    assert pairs[1][0][2] == 0 and pairs[1][0][1] == m.height       # (really clipped)
    return [p[0] for p in pairs], [p[1] for p in pairs]


def check_values(trace, frames, rects, patches, what=''):
    assert trace.shape == (len(frames), len(rects)), (trace.shape, len(frames))
    worst = 0.0
    for s, x in enumerate(frames):
        for e, (r, p) in enumerate(zip(rects, patches)):
            want, _ = ref.weighted_sum(x, r, p)
            b = ref.bound(x, r, p)
            err = abs(float(trace[s, e]) - want)
            worst = max(worst, err / b if b > 0 else (0.0 if err == 0 else np.inf))
            assert err <= b, '%s sample %d electrode %d: %.9g vs %.9g, |d| %.3g > bound %.3g' % (what, s, e, trace[s, e], want, err, b)
    print('%s: %d samples x %d electrodes, worst |d| / bound = %.3g' % (what, len(frames), len(rects), worst))


def wait_for_wave(m, slow, limit=2000):
    """steps until the S1 wave stands under the centre of the grid, where the first electrode sits.  The header's bound is
    the standard model of floating-point summation, which holds as long as no PRODUCT underflows; ahead of the wave the
    state is a tail of denormal numbers, whose products with the weights are lost whole in any float32 kernel (seen with the
    traced model: a sum of 3e-45 recorded as 0).  Under the wave the terms that matter are of order one."""
    st = m._stepper
    mid = 0.5 * (float(m.min_v) + float(m.max_v))
    for i in range(limit):
        if st.probe(0, m.height // 2, m.width // 2) >= mid:
            return i
        if slow and i % 10 == 0:
            m.fire_op('slow')
        st.step(1)
    raise AssertionError('the S1 wave never reached the centre of the grid')


def sampled_run(m, ticks, every, slow, s2=None, readback=True):
    """`ticks` ticks one call each with the three electrodes attached once the wave has reached them; the watched array read
    back at every tick (which must change nothing) and kept at the sample ticks"""
    st = m._stepper
    wait_for_wave(m, slow)
    rects, patches = three_electrodes(m)
    st.electrode_begin(0, rects, patches, every, ticks // every)
    frames = []
    for i in range(ticks):
        if slow and i % 10 == 0:
            m.fire_op('slow')
        if s2 is not None and i == s2:
            m.fire_op('s2')
        st.step(1)
        if readback:
            x = st.get_state(0)
            if (i + 1) % every == 0:
                frames.append(x.copy())
    assert st.electrode_count() == ticks // every
    return st.electrode_read(), frames, rects, patches


@pytest.mark.parametrize('every', [1, 3])
@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_values_within_the_derived_bound(gpu_lib, kind, every):
    m = MAKERS[kind](96, 130)
    trace, frames, rects, patches = sampled_run(m, 24, every, slow=kind == 'court', s2=7)
    assert trace.dtype == np.float32 and np.isfinite(trace).all()
    check_values(trace, frames, rects, patches, '%s every %d' % (kind, every))
    assert np.ptp(trace[:, 2]) > 0                            # (the state moved between the samples)
    m._stepper.close()


def test_whole_grid_patch_of_several_chunks(gpu_lib):
    m = fenton(300, 300)
    st = m._stepper
    rng = np.random.default_rng(8)
    rect, patch = (0, 300, 0, 300), rng.uniform(-1, 1, (300, 300)).astype(np.float32)
    small = ((10, 40, 0, 50), rng.uniform(0, 1, (30, 50)).astype(np.float32))        # (over the S1 wave)
    st.electrode_begin(0, [rect, small[0]], [patch, small[1]], 2, 5)
    frames = []
    for i in range(10):
        st.step(1)
        if i % 2 == 1:
            frames.append(st.get_state(0).copy())
    check_values(st.electrode_read(), frames, [rect, small[0]], [patch, small[1]], '300 x 300 patch')
    st.close()


def _plan_run(gpu_lib, monkeypatch, kind, env, record):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = MAKERS[kind](512, 512)
    st = m._stepper
    trace = None
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        if record:
            rects, patches = three_electrodes(m)
            st.electrode_begin(0, rects, patches, 4, 15)
        for i in range(60):
            if i == 30:
                m.fire_op('s2')
            st.step(1)
        if record:
            trace = st.electrode_read()
            assert st.electrode_count() == 15
        state = st.get_state(-1)
        fb, stats = st.fallbacks(), st.launch_stats()
    st.close()
    return trace, state, fb, stats


@pytest.mark.parametrize('kind', ['fenton', 'br'])
def test_traces_do_not_depend_on_the_launch_plan(gpu_lib, monkeypatch, kind):
    base, state, fb, stats = _plan_run(gpu_lib, monkeypatch, kind, {}, True)
    assert fb[0] == 0 and stats['mt_ticks'] > 0               # (the default plan does run multi-tick launches here)
    assert np.isfinite(base).all() and np.ptp(base[:, 0]) > 0
    for env in ({'FIBHIP_MT': '0'}, {'FIBHIP_AHEAD': '0'}, {'FIBHIP_MT_FAKE_GIVEUP': '2'}):
        got, st2, fb2, stats2 = _plan_run(gpu_lib, monkeypatch, kind, env, True)
        assert got.tobytes() == base.tobytes(), '%s: %d samples differ' % (env, int((got != base).sum()))
        assert st2.tobytes() == state.tobytes(), env
        if 'FIBHIP_MT_FAKE_GIVEUP' in env:
            assert fb2[0] == 1 and fb2[1] > 0, fb2            # one launch gave up and was recovered
        if 'FIBHIP_MT' in env:
            assert stats2['mt_ticks'] == 0
    _, plain, _, _ = _plan_run(gpu_lib, monkeypatch, kind, {}, False)
    assert plain.tobytes() == state.tobytes()                 # the recorder changes nothing of the state


def test_multi_tick_launches_survive_between_samples(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    from fib_tf_amd import egm
    a, b = fenton(512, 512), fenton(512, 512)
    sa, sb = a._stepper, b._stepper
    for st in (sa, sb):                                       # plan selection happens at the first tick
        st.step(1)
        st.sync()
    rect, patch = egm.crop_mask(egm.create_mask(a, 300, 256, 5))
    sa.electrode_begin(0, [rect], [patch], 8, 8)
    a0, b0 = sa.launch_stats(), sb.launch_stats()
    for i in range(64):
        sa.step(1)
        sb.step(1)
        if i % 8 == 7:
            sb.sync()
    assert sa.electrode_count() == 8
    trace = sa.electrode_read()
    a1, b1 = sa.launch_stats(), sb.launch_stats()
    assert a1['mt_ticks'] - a0['mt_ticks'] == 64, (a0, a1)
    assert a1['mt_launches'] - a0['mt_launches'] <= b1['mt_launches'] - b0['mt_launches'], (a0, a1, b0, b1)
    assert a1['launches'] - a0['launches'] == (a1['mt_launches'] - a0['mt_launches']) + 8
    assert sa.get_state(-1).tobytes() == sb.get_state(-1).tobytes()
    assert np.isfinite(trace).all()
    sa.close()
    sb.close()


def test_courtemanche_keeps_its_three_tick_launches(gpu_lib):
    from fib_tf_amd import egm
    a, b = court(256, 256), court(256, 256)
    sa, sb = a._stepper, b._stepper
    for st in (sa, sb):
        st.step(3)
        st.sync()
    assert sb.ticks_per_launch() == 3
    rect, patch = egm.crop_mask(egm.create_mask(a, 100, 128, 5))
    sa.electrode_begin(0, [rect], [patch], 3, 20)
    a0, b0 = sa.launch_stats()['launches'], sb.launch_stats()['launches']
    for _ in range(60):
        sa.step(1)
        sb.step(1)
    sa.sync()
    sb.sync()
    samples = sa.electrode_count()
    assert samples == 20
    assert sa.launch_stats()['launches'] - a0 - samples == sb.launch_stats()['launches'] - b0
    assert sa.get_state(-1).tobytes() == sb.get_state(-1).tobytes()
    sa.close()
    sb.close()


def test_every_tick_on_the_multi_tick_handle(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    m = fenton(512, 512)
    trace, frames, rects, patches = sampled_run(m, 64, 1, slow=False, s2=20)
    assert trace.shape[0] == 64
    check_values(trace, frames, rects, patches, 'fenton 512 every 1')
    m._stepper.close()


def test_both_recorders_at_once(gpu_lib):
    from fib_tf_amd import egm

    def play(electrodes, activation):
        m = fenton(128, 128)
        st = m._stepper
        rects, patches = three_electrodes(m)
        rec = m.record_activation() if activation else None
        if electrodes:
            st.electrode_begin(0, rects, patches, 2, 50)
        for i in range(100):
            if i == 40:
                m.fire_op('s2')
            st.step(1)
        trace = st.electrode_read() if electrodes else None
        maps = rec.maps() if activation else None
        st.close()
        return trace, maps
    both_t, both_m = play(True, True)
    only_t, _ = play(True, False)
    _, only_m = play(False, True)
    assert both_t.shape == (50, 3) and both_t.tobytes() == only_t.tobytes()
    for k in only_m:
        assert both_m[k].tobytes() == only_m[k].tobytes(), k
    assert only_m['count'].max() >= 1


def test_protocol_against_polling(gpu_lib):
    """record_on_device against record() on the strip of tests/test_gpu_physics.py: the same samples up to the summation
    error of either side, and the same conduction velocity as probe timing within the margin that test grants record()"""
    from fib_tf_amd import egm
    from fib_tf_amd.fenton import Fenton4v
    from test_gpu_physics import velocity
    cfg = {'height': 48, 'width': 420, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.0, 'duration': 700}

    def make():
        m = Fenton4v(dict(cfg))
        m.define()
        return m
    want = velocity(make(), 0.5)
    m = make()
    masks = [egm.create_mask(m, 150, 24, 5), egm.create_mask(m, 300, 24, 5)]
    frames = []
    image = m.image
    m.image = lambda: frames.append(image()) or frames[-1]     # (keeps what record() saw, for the bounds)
    polled = egm.record(m, masks[0], masks[1])
    m = make()
    dev = egm.record_on_device(m, masks[0], masks[1])
    assert dev.shape == polled.shape == (700, 2)
    cells = 48 * 420
    crops = [egm.crop_mask(k) for k in masks]
    worst = 0.0
    for s in range(700):
        for e in range(2):
            tol = (ref.bound(frames[s], *crops[e]) + ref.pairwise_mean_bound(frames[s], masks[e])) / cells
            err = abs(dev[s, e] - polled[s, e])
            worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else np.inf))
            assert err <= tol, (s, e, dev[s, e], polled[s, e], tol)
    print('record_on_device vs record: worst |d| / tolerance = %.3g' % worst)
    got = egm.conduction_velocity(dev, 150.0)
    assert abs(got / want - 1.0) < 0.03, (got, want)


def test_record_on_device_stride_three(gpu_lib):
    from fib_tf_amd import egm
    a, b = fenton(64, 160, duration=30), fenton(64, 160, duration=30)
    masks = [egm.create_mask(a, 40, 32, 5), egm.create_mask(a, 100, 32, 5)]
    polled = egm.record(a, masks[0], masks[1], every_ms=3.0)
    dev = egm.record_on_device(b, masks[0], masks[1], every_ms=3.0)
    assert dev.shape == polled.shape == (10, 2)
    assert np.abs(dev - polled).max() < 1e-6 and np.ptp(polled[:, 0]) > 1e-4


@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_capacity_windows_and_reattachment(gpu_lib, kind):
    m = MAKERS[kind](96, 130)
    st = m._stepper
    rects, patches = three_electrodes(m)
    st.electrode_begin(0, rects, patches, 2, 3)
    st.step(5)
    assert st.electrode_count() == 2                          # (ticks accepted but not launched yet count)
    if kind == 'court':
        m.fire_op('slow')                                     # rides on the launch of the last held tick
        assert st.electrode_count() == 2
    st.sync()                                                 # (launch_stats counts launched ticks, not accepted ones)
    ticks = st.launch_stats()['ticks']
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(3)                                            # would take sample number 3
    st.step(1)                                                # sample number 2 still fits: the trace is full now
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(2)
    st.sync()
    assert st.launch_stats()['ticks'] == ticks + 1            # nothing of the refused calls ran
    full = st.electrode_read()
    assert full.shape == (3, 3) and st.electrode_count() == 3
    assert st.electrode_read(1, 2).tobytes() == full[1:].tobytes()
    assert st.electrode_read(0, 1).tobytes() == full[:1].tobytes()
    assert st.electrode_read(3, 0).shape == (0, 3)
    for first, count in ((0, 4), (2, 2), (-1, 1), (4, 0), (0, -1)):
        with pytest.raises(gpu_lib.FibhipError, match='electrode_read'):
            st.electrode_read(first, count)
    x = st.get_state(0)
    for e in (1, 2):                                          # (the electrodes the S1 wave stands under already)
        assert abs(float(full[2, e]) - ref.weighted_sum(x, rects[e], patches[e])[0]) <= ref.bound(x, rects[e], patches[e])
    st.electrode_begin(0, rects[:1], patches[:1], 1, 4)       # re-attachment: an empty trace, a new origin
    assert st.electrode_count() == 0 and st.electrode_read().shape == (0, 1)
    st.step(2)
    assert st.electrode_read().shape == (2, 1)
    st.electrode_end()
    st.electrode_end()                                        # (nothing attached: nothing to do)
    with pytest.raises(gpu_lib.FibhipError, match='no recorder'):
        st.electrode_read(0, 0)
    with pytest.raises(gpu_lib.FibhipError, match='no recorder'):
        st.electrode_count()
    st.step(50)                                               # the handle runs on without a recorder
    st.electrode_begin(0, rects, patches, 1, 2)
    st.step(1)
    st.close()                                                # destroyed with a recorder attached


@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_refusals(gpu_lib, kind):
    import ctypes as C
    m = MAKERS[kind](64, 80)
    st = m._stepper
    nvar = st.nvar
    L, h = st._L, st._h
    w = np.ones(16, np.float32)
    wp = w.ctypes.data_as(C.POINTER(C.c_float))

    def begin(var=0, n=1, rect=(0, 4, 0, 4), every=1, cap=4, weights=wp, rects=True):
        r = (C.c_int * (4 * max(n, 1)))(*(list(rect) * max(n, 1)))
        return L.fibhip_electrode_begin(h, var, n, r if rects else None, weights, every, cap)
    assert begin() == 0
    for kw in (dict(var=-1), dict(var=nvar), dict(n=0), dict(n=65), dict(every=0), dict(every=-3), dict(cap=0), dict(cap=-1),
               dict(cap=2 ** 62), dict(weights=None), dict(rects=False),
               dict(rect=(0, 65, 0, 4)), dict(rect=(0, 4, 0, 81)), dict(rect=(-1, 3, 0, 4)), dict(rect=(4, 4, 0, 4)),
               dict(rect=(0, 4, 5, 3))):
        assert begin(**kw) != 0, kw
        assert b'electrode_begin' in L.fibhip_last_error()
    for bad in (np.nan, np.inf):
        w[5] = bad
        assert begin() != 0 and b'not finite' in L.fibhip_last_error()
    w[5] = 1.0
    assert st.electrode_count() == 0                          # the refused calls left the first recorder attached
    st.step_edges()
    assert begin() != 0 and b'open tick' in L.fibhip_last_error()
    st.step_interior()
    st.step_commit()
    assert st.electrode_count() == 1
    wide = np.ones((64, 80), np.float32)
    st.electrode_begin(0, [(0, 64, 0, 80)] * 64, [wide] * 64, 1, 1)       # 64 whole-grid electrodes are accepted
    st.step(1)
    got = st.electrode_read()
    assert got.shape == (1, 64) and np.all(got == got[0, 0])
    assert L.fibhip_electrode_begin(None, 0, 1, (C.c_int * 4)(0, 4, 0, 4), wp, 1, 4) != 0
    st.close()


def test_row_block_refused_by_the_library(gpu_lib):
    """a handle with ghost rows (a row block) is refused by fibhip_electrode_begin itself"""
    import ctypes as C
    blk = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    w = np.ones(16, np.float32)
    rc = blk._L.fibhip_electrode_begin(blk._h, 0, 1, (C.c_int * 4)(0, 4, 0, 4), w.ctypes.data_as(C.POINTER(C.c_float)), 1, 4)
    assert rc == -1 and b'row block' in blk._L.fibhip_last_error()
    blk.close()


@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_timeline_lists_the_sample(gpu_lib, kind):
    from fib_tf_amd import egm
    m = MAKERS[kind](96, 130)
    st = m._stepper
    rect, patch = egm.crop_mask(egm.create_mask(m, 60, 40, 5))
    st.step(1)
    st.electrode_begin(0, [rect], [patch], 1, 8)
    events = st.trace_tick()
    names = [e['name'] for e in events]
    assert any(n == 'electrode_kernel' for n in names), names
    assert st.electrode_count() == 1
    st.close()


def _bound_with_underflow(x, rect, patch):
    """the header's bound plus what the float32 format itself takes from products below the normal range: each product is
    rounded to a multiple of 2^-149, an absolute error of at most 2^-149 (2^-150 under round-to-nearest), and sums of such
    numbers are exact — m * 2^-149 for a patch of m cells.  A bound of this file's own, for the regime the relative bound
    cannot speak about."""
    r0, r1, c0, c1 = rect
    return ref.bound(x, rect, patch) + (r1 - r0) * (c1 - c0) * 2.0 ** -149


@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_quiescent_tissue_from_the_first_tick(gpu_lib, kind):
    """attached at tick 0, the S1 wave still at the left edge: the state under the first electrode is zero, denormal or at
    rest, and the products with the Gaussian's tail underflow"""
    m = MAKERS[kind](96, 130)
    st = m._stepper
    rects, patches = three_electrodes(m)
    st.electrode_begin(0, rects, patches, 1, 8)
    frames = []
    for _ in range(8):
        st.step(1)
        frames.append(st.get_state(0).copy())
    trace = st.electrode_read()
    for s, x in enumerate(frames):
        for e, (r, p) in enumerate(zip(rects, patches)):
            want, _ = ref.weighted_sum(x, r, p)
            b = _bound_with_underflow(x, r, p)
            assert abs(float(trace[s, e]) - want) <= b, (kind, s, e, trace[s, e], want, b)
    st.close()


@pytest.mark.parametrize('kind,var', [('fenton', 1), ('br', 3), ('court', 5), ('traced', 1)])
def test_another_array_and_the_slow_operation(gpu_lib, kind, var):
    """var != 0: the sums are taken of that array.  Courtemanche, var = 5 (one of the arrays 'slow' writes): 'slow' fired after
    a tick belongs to the next tick, whether or not that tick's launch could have carried it (a run without read-backs
    holds ticks back, so that 'slow' would ride on the launch of the last one) — the two runs agree bit for bit"""
    def play(readback):
        m = MAKERS[kind](96, 130)
        st = m._stepper
        rects, patches = three_electrodes(m)
        st.electrode_begin(var, rects, patches, 2, 15)
        frames = []
        for i in range(30):
            st.step(1)
            if readback:
                x = st.get_state(var)
                if i % 2 == 1:
                    frames.append(x.copy())
            if kind == 'court' and i % 5 == 0:
                m.fire_op('slow')                             # after ticks 0, 5, 10, ...: 5, 15, 25 are sample ticks
        trace = st.electrode_read()
        st.close()
        return trace, frames, rects, patches
    held, _, _, _ = play(False)
    trace, frames, rects, patches = play(True)
    assert held.tobytes() == trace.tobytes()
    assert len(frames) == 15
    for s, x in enumerate(frames):
        for e, (r, p) in enumerate(zip(rects, patches)):
            want, _ = ref.weighted_sum(x, r, p)
            b = _bound_with_underflow(x, r, p)
            assert abs(float(trace[s, e]) - want) <= b, (kind, var, s, e, trace[s, e], want, b)
    assert np.isfinite(trace).all()


def test_recorder_converts_another_array_without_the_image_affine(gpu_lib):
    m = br(64, 80)
    mask = np.ones((64, 80), np.float32)
    with m.record_electrodes([mask], var=3, capacity=2) as rec:
        assert rec.affine == (1.0, 0.0)
        m._stepper.step(1)
        x = m._stepper.get_state(3).astype(np.float64)
        got = rec.traces()
    assert got.shape == (1, 1) and abs(got[0, 0] - x.mean()) <= 1e-5 * np.abs(x).mean()
    m._stepper.close()
