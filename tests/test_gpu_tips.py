"""-m gpu: the tip recorder (include/fibhip.h fibhip_tips_*, fib_tf_amd/tips.py) on the device.

The definition is exact integer arithmetic on float32 inputs, so every sample must EQUAL the NumPy restatement
(tests/tip_ref.py) on the two arrays read back at the same tick: records sorted by (row, column), and the counts.  No
tolerance anywhere in this file.  The lists must not depend on the launch plan, multi-tick launches must survive between
two samples, and the book-keeping (capacity, windows, refusals, re-attachment) is exercised call by call.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import electrode_ref  # noqa: E402
import tip_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

PLAN_ENV = ('FIBHIP_MT', 'FIBHIP_AHEAD', 'FIBHIP_MT_FAKE_GIVEUP', 'FIBHIP_VARIANT')


SLOW_DT = 0.001         # a tick of 0.01 ms: planted tips drift for tens of ticks instead of dissolving in the first two


def fenton(h, w, duration=1000, dt=0.1):
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': h, 'width': w, 'dt': dt, 'dt_per_plot': 10, 'diff': 1.5, 'duration': duration})
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
# (var2, a0, b0) with var = 0, and the half-swing of either array the planted fields are scaled to.  The stock models' come
# from their tip_signals; the traced model (Aliev-Panfilov: u and its recovery variable, both in [0, 1]) has none.
SIGNALS = {'traced': (1, 0.5, 0.5, 0.4, 0.4)}


def signals(kind, m):
    if kind in SIGNALS:
        return SIGNALS[kind]
    _, var2, a0, b0 = m.tip_signals
    swing = {'fenton': (0.4, 0.4), 'br': (40.0, 0.1), 'court': (40.0, 0.4)}[kind]
    return (var2, a0, b0) + swing


def planted(h, w, a0, b0, sa, sb):
    """two [h, w] float32 fields around the levels with known tips: the two-vortex field (z - z1) conj(z - z2), each part
    squashed into (-1, 1) and scaled to the half-swings sa, sb, plus small vortices whose centres lie in plaquette rows 0
    and h - 2 and in plaquette columns 0, w - 2 and w - 3, and one NaN cell"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)

    def vortex(cy, cx, sign):
        z = (x - cx) + 1j * sign * (y - cy)
        return z / (1.0 + np.abs(z))                           # (the phase is what matters)
    z = ((x - 40.3) + 1j * (y - 30.6)) * np.conj((x - 90.4) + 1j * (y - 60.7))
    z = z / (1.0 + np.abs(z))
    centres = [(0.4, 20.5, 1), (h - 1.6, 50.5, -1), (45.5, 0.4, 1), (20.5, w - 1.6, -1), (70.5, w - 2.6, 1)]
    for cy, cx, sign in centres:                               # inside a disc of radius 5 the small vortex replaces the field
        near = np.hypot(x - cx, y - cy) < 5.0
        z = np.where(near, vortex(cy, cx, sign), z)
    A = (a0 + sa * z.real).astype(np.float32)
    B = (b0 + sb * z.imag).astype(np.float32)
    A[31, 42] = np.nan
    return A, B, [(int(np.floor(cy)), int(np.floor(cx))) for cy, cx, _ in centres]


def check_samples(counts, records, frames, a0, b0, max_tips, mask=None, what=''):
    assert counts.shape == (len(frames), 3) and counts.dtype == np.int32, (counts.shape, len(frames))
    total = 0
    for s, (A, B) in enumerate(frames):
        want, (pos, neg) = ref.tips(A, B, a0, b0, mask)
        assert counts[s].tolist() == [pos, neg, pos + neg], '%s sample %d: counts %s, reference %s' % (what, s, counts[s], (pos, neg))
        got = ref.sorted_records(records[s], counts[s, 2], max_tips)
        assert np.array_equal(got, want), '%s sample %d: %d records differ' % (what, s, int((got != want).any(axis=1).sum()))
        total += pos + neg
    print('%s: %d samples, %d tips in all' % (what, len(frames), total))
    return total


@pytest.mark.parametrize('every', [1, 3])
@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_samples_equal_the_reference(gpu_lib, kind, every):
    m = MAKERS[kind](96, 130)
    st = m._stepper
    var2, a0, b0, sa, sb = signals(kind, m)
    A, B, cells = planted(96, 130, a0, b0, sa, sb)
    first, _ = ref.tips(A, B, a0, b0)
    have = set(map(tuple, first[:, :2]))
    assert {(0, 20), (94, 50), (45, 0), (20, 128), (70, 127), (30, 40), (60, 90)} <= have, sorted(have)    # the planted tips are tips
    st.set_state(0, A)
    st.set_state(var2, B)
    st.tips_begin(0, var2, a0, b0, None, every, 512, 12 // every)
    frames = []
    for i in range(12):
        if kind == 'court' and i % 10 == 0:
            m.fire_op('slow')
        st.step(1)
        a, b = st.get_state(0), st.get_state(var2)
        if (i + 1) % every == 0:
            frames.append((a.copy(), b.copy()))
    assert st.tips_count() == 12 // every
    counts, records = st.tips_read()
    total = check_samples(counts, records, frames, a0, b0, 512, what='%s every %d' % (kind, every))
    assert counts[:, 2].max() >= 1 and total >= 1             # at least one sample holds a tip
    assert np.all(counts[:, 2] <= 512)
    st.close()


@pytest.fixture(scope='module')
def noise():
    rng = np.random.default_rng(0)
    A = rng.uniform(-1, 1, (96, 130)).astype(np.float32)
    B = rng.uniform(-1, 1, (96, 130)).astype(np.float32)
    want, (pos, neg) = ref.tips(A, B, 0, 0)
    assert pos + neg == 4094
    return A, B, want, pos, neg


def _noise_sample(gpu_lib, noise, max_tips, mask=None):
    """one sample of noise in Fenton's arrays 2 and 3.  set_state between two ticks belongs to the next tick, so the sample
    sees what one tick of the gates made of the fields: the frames read back at the sample tick are what the reference gets"""
    A, B = noise[0], noise[1]
    m = fenton(96, 130)
    st = m._stepper
    st.tips_begin(2, 3, 0.0, 0.0, mask, 1, max_tips, 1)        # arrays 2 and 3 (w, s): pointwise, no stencil
    st.set_state(2, A)
    st.set_state(3, B)
    st.step(1)
    fa, fb = st.get_state(2), st.get_state(3)
    counts, records = st.tips_read()
    st.close()
    return counts, records, fa, fb


def test_uniform_noise_whole_and_cut(gpu_lib, noise):
    counts, records, fa, fb = _noise_sample(gpu_lib, noise, 8192)
    want, (pos, neg) = ref.tips(fa, fb, 0, 0)
    assert pos + neg > 1024                                    # (one tick of the gates leaves the noise noise)
    check_samples(counts, records, [(fa, fb)], 0, 0, 8192, what='noise, max_tips 8192')
    counts, records, fa2, fb2 = _noise_sample(gpu_lib, noise, 1024)
    assert fa2.tobytes() == fa.tobytes() and fb2.tobytes() == fb.tobytes()
    assert counts[0].tolist() == [pos, neg, pos + neg] and counts[0, 2] > 1024      # the counters stay exact when the list is cut
    got = records[0]
    assert np.all(got[:, 3] == 0)
    rows = set(map(tuple, got[:, :3]))
    assert len(rows) == 1024 and rows <= set(map(tuple, want))                     # no duplicates, a subset of the reference


def test_mask_removes_what_the_reference_removes(gpu_lib, noise):
    mask = np.ones((96, 130), np.uint8)
    mask[30:50, 40:77] = 0
    mask[0, 0] = mask[95, 129] = mask[17, 129] = mask[60, 3] = 0
    mask[70:72, :] = 0
    counts, records, fa, fb = _noise_sample(gpu_lib, noise, 8192, mask)
    free, _ = ref.tips(fa, fb, 0, 0)
    kept, _ = ref.tips(fa, fb, 0, 0, mask)
    assert 0 < len(kept) < len(free)
    check_samples(counts, records, [(fa, fb)], 0, 0, 8192, mask, what='noise under a mask')


def test_larger_grid_of_many_workgroups(gpu_lib):
    """300 x 300 (a planar slab whose rows are 16-byte aligned: the vector path, 75 threads per row) under a mask"""
    rng = np.random.default_rng(9)
    A = rng.uniform(-1, 1, (300, 300)).astype(np.float32)
    B = rng.uniform(-1, 1, (300, 300)).astype(np.float32)
    A[::7, ::5] = np.where(rng.uniform(size=A[::7, ::5].shape) < 0.3, 0.0, A[::7, ::5])      # (zeros: b >= 0 and cross == 0 cases)
    B[::5, ::7] = 0.0
    A[100, 299] = A[299, 0] = B[150, 150] = np.nan
    mask = np.ones((300, 300), np.uint8)
    mask[120:140, 100:203] = 0
    mask[5, 296:] = 0
    m = fenton(300, 300)
    st = m._stepper
    st.tips_begin(2, 3, 0.0, 0.0, mask, 2, 32768, 2)
    frames = []
    for i in range(4):
        if i % 2 == 1:
            st.set_state(2, A if i == 1 else -A)
            st.set_state(3, B)
        st.step(1)
        if i % 2 == 1:
            frames.append((st.get_state(2), st.get_state(3)))
    counts, records = st.tips_read()
    total = check_samples(counts, records, frames, 0, 0, 32768, mask, what='300 x 300')
    assert total > 10000
    st.close()


def _plan_run(gpu_lib, monkeypatch, env, record):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fenton(128, 128, dt=SLOW_DT)
    st = m._stepper
    _, var2, a0, b0 = m.tip_signals
    A, B, _ = planted(128, 128, a0, b0, 0.4, 0.4)
    A[31, 42] = a0                                            # (no NaN here: the state is stepped for 40 ticks)
    st.set_state(0, A)
    st.set_state(var2, B)
    st.step(1)                                                # plan selection happens at the first tick
    st.sync()
    out = None
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        s0 = st.launch_stats()
        if record:
            st.tips_begin(0, var2, a0, b0, None, 10, 256, 4)
        for i in range(40):
            st.step(1)
        if record:
            assert st.tips_count() == 4
            out = st.tips_read()
        state = st.get_state(-1)
        fb, s1 = st.fallbacks(), st.launch_stats()
    st.close()
    return out, state, fb, {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}


def test_lists_do_not_depend_on_the_launch_plan(gpu_lib, monkeypatch):
    (counts, records), state, fb, stats = _plan_run(gpu_lib, monkeypatch, {}, True)
    assert fb[0] == 0 and stats['mt_ticks'] > 0               # (the default plan does run multi-tick launches here)
    # between two samples the handle runs the fewest launches `every` allows: four ten-tick launches, four samples
    assert stats['mt_ticks'] == 40 and stats['mt_launches'] == 4, stats
    assert stats['launches'] == stats['mt_launches'] + 4, stats
    base = [ref.sorted_records(records[s], counts[s, 2], 256) for s in range(4)]
    assert counts[:, 2].min() >= 1 and np.all(counts[:, 2] <= 256)      # every sample holds tips
    assert any(base[s].tobytes() != base[0].tobytes() for s in range(1, 4))    # ... and they move
    for env in ({'FIBHIP_MT': '0'}, {'FIBHIP_AHEAD': '0'}, {'FIBHIP_MT_FAKE_GIVEUP': '2'}):
        (c2, r2), st2, fb2, stats2 = _plan_run(gpu_lib, monkeypatch, env, True)
        assert c2.tobytes() == counts.tobytes(), (env, c2, counts)
        for s in range(4):
            assert ref.sorted_records(r2[s], c2[s, 2], 256).tobytes() == base[s].tobytes(), (env, s)
        assert st2.tobytes() == state.tobytes(), env
        if 'FIBHIP_MT_FAKE_GIVEUP' in env:
            assert fb2[0] == 1 and fb2[1] > 0, fb2            # one launch gave up and was recovered
        if 'FIBHIP_MT' in env:
            assert stats2['mt_ticks'] == 0
    _, plain, _, pstats = _plan_run(gpu_lib, monkeypatch, {}, False)
    assert plain.tobytes() == state.tobytes()                 # the recorder changes nothing of the state
    # a handle without a recorder: as ever — every launch is a multi-tick launch or a plain tick, nothing else is enqueued
    assert pstats['ticks'] == 40 and pstats['mt_ticks'] > 0
    assert pstats['launches'] == pstats['mt_launches'] + (pstats['ticks'] - pstats['mt_ticks']), pstats


def test_both_samplers_at_once(gpu_lib):
    """electrodes every 3 and tips every 4 ticks on one handle: each right at its own ticks"""
    from fib_tf_amd import egm
    m = fenton(96, 130, dt=SLOW_DT)
    st = m._stepper
    _, var2, a0, b0 = m.tip_signals
    A, B, _ = planted(96, 130, a0, b0, 0.4, 0.4)
    A[31, 42] = a0
    st.set_state(0, A)
    st.set_state(var2, B)
    rect, patch = egm.crop_mask(egm.create_mask(m, 60, 40, 5))
    st.electrode_begin(0, [rect], [patch], 3, 8)
    st.tips_begin(0, var2, a0, b0, None, 4, 256, 6)
    el_frames, tip_frames = [], []
    for i in range(24):
        st.step(1)
        if (i + 1) % 3 == 0 or (i + 1) % 4 == 0:
            a = st.get_state(0)
            if (i + 1) % 3 == 0:
                el_frames.append(a.copy())
            if (i + 1) % 4 == 0:
                tip_frames.append((a.copy(), st.get_state(var2)))
    assert st.electrode_count() == 8 and st.tips_count() == 6
    trace = st.electrode_read()
    assert trace.shape == (8, 1)
    for s, x in enumerate(el_frames):
        want, _ = electrode_ref.weighted_sum(x, rect, patch)
        assert abs(float(trace[s, 0]) - want) <= electrode_ref.bound(x, rect, patch), (s, trace[s, 0], want)
    counts, records = st.tips_read()
    assert check_samples(counts, records, tip_frames, a0, b0, 256, what='tips beside electrodes') >= 1
    assert counts[:, 2].min() >= 1
    # without observations in between: the launches end at the sample ticks of either, and the lists are the same
    m2 = fenton(96, 130, dt=SLOW_DT)
    s2 = m2._stepper
    s2.set_state(0, A)
    s2.set_state(var2, B)
    s2.electrode_begin(0, [rect], [patch], 3, 8)
    s2.tips_begin(0, var2, a0, b0, None, 4, 256, 6)
    s2.step(24)
    assert s2.electrode_read().tobytes() == trace.tobytes()
    c2, r2 = s2.tips_read()
    assert c2.tobytes() == counts.tobytes()
    for s in range(6):
        assert np.array_equal(ref.sorted_records(r2[s], c2[s, 2], 256), ref.sorted_records(records[s], counts[s, 2], 256))
    st.close()
    s2.close()


def test_with_the_activation_recorder_every_tick_is_one_launch(gpu_lib):
    m = fenton(128, 128)
    st = m._stepper
    _, var2, a0, b0 = m.tip_signals
    st.step(1)
    st.sync()
    rec = m.record_activation()
    st.tips_begin(0, var2, a0, b0, None, 5, 16, 4)
    s0 = st.launch_stats()
    st.step(20)
    assert st.tips_count() == 4
    counts, _ = st.tips_read()
    s1 = st.launch_stats()
    assert s1['mt_ticks'] == s0['mt_ticks'] and s1['ticks'] - s0['ticks'] == 20
    assert s1['launches'] - s0['launches'] == 20 + 20 + 4       # a tick, the activation recorder's kernel, and the samples
    assert counts.shape == (4, 3)
    rec.close()
    st.close()


@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_capacity_windows_and_reattachment(gpu_lib, kind):
    m = MAKERS[kind](96, 130)
    st = m._stepper
    var2, a0, b0, sa, sb = signals(kind, m)
    A, B, _ = planted(96, 130, a0, b0, sa, sb)
    st.set_state(0, A)
    st.set_state(var2, B)
    st.tips_begin(0, var2, a0, b0, None, 2, 64, 3)
    st.step(5)
    assert st.tips_count() == 2                               # (ticks accepted but not launched yet count)
    if kind == 'court':
        m.fire_op('slow')                                     # var2 is a slow array: the sample of tick 3 was taken before 'slow'
        assert st.tips_count() == 2
    st.sync()
    ticks = st.launch_stats()['ticks']
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(3)                                            # would take sample number 3
    st.step(1)                                                # sample number 2 still fits: the lists are full now
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(2)
    st.sync()
    assert st.launch_stats()['ticks'] == ticks + 1            # nothing of the refused calls ran
    counts, records = st.tips_read()
    assert counts.shape == (3, 3) and records.shape == (3, 64, 4) and st.tips_count() == 3
    c, r = st.tips_read(1, 2)
    assert c.tobytes() == counts[1:].tobytes()
    for s in range(2):
        assert np.array_equal(ref.sorted_records(r[s], c[s, 2], 64), ref.sorted_records(records[1 + s], counts[1 + s, 2], 64))
    c, r = st.tips_read(0, 1, records=False)
    assert c.tobytes() == counts[:1].tobytes() and r is None
    c, r = st.tips_read(3, 0)
    assert c.shape == (0, 3) and r.shape == (0, 64, 4)
    for first, count in ((0, 4), (2, 2), (-1, 1), (4, 0), (0, -1)):
        with pytest.raises(gpu_lib.FibhipError, match='tips_read'):
            st.tips_read(first, count)
    a, b = st.get_state(0), st.get_state(var2)
    check_samples(counts[2:], records[2:], [(a, b)], a0, b0, 64, what='%s last sample' % kind)
    st.tips_begin(0, var2, a0, b0, None, 1, 8, 4)             # re-attachment: empty lists, a new origin
    assert st.tips_count() == 0 and st.tips_read()[0].shape == (0, 3)
    st.step(2)
    assert st.tips_read()[1].shape == (2, 8, 4)
    st.tips_end()
    st.tips_end()                                             # (nothing attached: nothing to do)
    with pytest.raises(gpu_lib.FibhipError, match='no recorder'):
        st.tips_read(0, 0)
    with pytest.raises(gpu_lib.FibhipError, match='no recorder'):
        st.tips_count()
    st.step(50)                                               # the handle runs on without a recorder
    st.tips_begin(0, var2, a0, b0, None, 1, 8, 2)
    st.step(1)
    st.close()                                                # destroyed with a recorder attached


@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_refusals(gpu_lib, kind):
    import ctypes as C
    m = MAKERS[kind](64, 80)
    st = m._stepper
    nvar = st.nvar
    L, h = st._L, st._h

    def begin(var=0, var2=1, a0=0.5, b0=0.5, every=1, max_tips=16, cap=4):
        return L.fibhip_tips_begin(h, var, var2, a0, b0, None, every, max_tips, cap)
    assert begin() == 0
    for kw in (dict(var=-1), dict(var=nvar), dict(var2=-1), dict(var2=nvar), dict(var=1, var2=1), dict(var=0, var2=0),
               dict(a0=float('nan')), dict(b0=float('nan')), dict(every=0), dict(every=-3), dict(max_tips=0), dict(max_tips=-1),
               dict(max_tips=65537), dict(cap=0), dict(cap=-1), dict(cap=2 ** 62)):
        assert begin(**kw) != 0, kw
        assert b'tips_begin' in L.fibhip_last_error(), kw
    assert st.tips_count() == 0                               # the refused calls left the first recorder attached
    st.step_edges()
    assert begin() != 0 and b'open tick' in L.fibhip_last_error()
    st.step_interior()
    st.step_commit()
    assert st.tips_count() == 1
    st.tips_begin(0, 1, 0.5, 0.5, None, 1, 65536, 1)          # the largest list is accepted (through the binding, which sizes
    st.step(1)                                                # the arrays tips_read hands to the library from max_tips)
    counts, records = st.tips_read()
    assert counts.shape == (1, 3) and records.shape == (1, 65536, 4)
    assert L.fibhip_tips_begin(None, 0, 1, 0.5, 0.5, None, 1, 16, 4) != 0
    assert L.fibhip_tips_end(h) == 0 and L.fibhip_tips_end(h) == 0          # end without begin: nothing
    k = C.c_longlong()
    assert L.fibhip_tips_count(h, C.byref(k)) != 0 and b'no recorder' in L.fibhip_last_error()
    st.close()


def test_row_block_refused_by_the_library(gpu_lib):
    """a handle with ghost rows (a row block) is refused by fibhip_tips_begin itself"""
    blk = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    rc = blk._L.fibhip_tips_begin(blk._h, 0, 1, 0.5, 0.5, None, 1, 16, 4)
    assert rc == -1 and b'row block' in blk._L.fibhip_last_error()
    blk.close()


@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_timeline_lists_the_sample(gpu_lib, kind):
    m = MAKERS[kind](96, 130)
    st = m._stepper
    var2, a0, b0, _, _ = signals(kind, m)
    st.step(1)
    st.tips_begin(0, var2, a0, b0, None, 1, 16, 8)
    events = st.trace_tick()
    names = [e['name'] for e in events]
    assert any(n == 'tip_kernel' for n in names), names
    assert st.tips_count() == 1
    st.close()


def test_recorder_on_a_model_with_a_hole(gpu_lib):
    """TipRecorder end to end: defaults from tip_signals, the default mask from the phase field, sorted output"""
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': 96, 'width': 130, 'dt': SLOW_DT, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 0.065})    # six ticks
    m.add_hole_to_phase_field(42, 31, 9)                      # over the first vortex of the planted field
    m.define()
    st = m._stepper
    _, var2, a0, b0 = m.tip_signals
    A, B, _ = planted(96, 130, a0, b0, 0.4, 0.4)
    A[31, 42] = a0                                            # (no NaN here: it would spread over that vortex)
    st.set_state(0, A)
    st.set_state(var2, B)
    with m.record_tips(every=2) as rec:
        assert rec.capacity == 3 and np.array_equal(rec.mask != 0, m.phase > 0.5) and not rec.mask.all()
        frames = []
        for i in m.run():
            if i % 2 == 1:
                frames.append((st.get_state(0), st.get_state(var2)))
        per, counts = rec.tips(), rec.counts()
        assert rec.count() == 3 and len(per) == 3 and len(rec.truncated()) == 0
    for s, (a, b) in enumerate(frames):
        want, (pos, neg) = ref.tips(a, b, a0, b0, rec.mask)
        assert counts[s].tolist() == [pos, neg, pos + neg]
        got = np.stack([per[s]['y'] - 0.5, per[s]['x'] - 0.5, per[s]['charge']], axis=1).astype(np.int32)
        assert np.array_equal(got, want)
        assert np.all(per[s]['t_ms'] == (s + 1) * 2 * rec.tick_ms) and rec.tick_ms == pytest.approx(0.01)
        free, _ = ref.tips(a, b, a0, b0)
        assert len(free) > len(want) >= 1                     # the hole took tips away, and left some
    st.close()


S2_TICK = 30            # tests/golden/fenton_driver96.npz: 's2' = [30, 1.0]
LAST_TICK = 150
N_AFTER_S2 = 0          # samples after S2 that hold a tip in the oracle's run of the same protocol (see the test's docstring)


def _driver96(golden, s2_tick, last_tick):
    """the reference driver's S1-S2 protocol at 96 x 96 from the inputs of fenton_driver96 (initial state, phase field with
    the hole (48, 48, 8), diff 1.5, S2 = 1.0 on 'luq' fired after tick `s2_tick`), tips every 10 ticks under the default
    mask.  Returns (counts, records, frames, a0, b0, mask)."""
    from fib_tf_amd.fenton import Fenton4v
    f = golden('fenton_driver96')
    m = Fenton4v({'height': 96, 'width': 96, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': last_tick})
    m.phase = np.array(f['phase'], np.float32)
    m.define()
    m.add_pace_op('s2', 'luq', float(f['s2'][1]))
    st = m._stepper
    st.set_state(-1, np.stack([f['init_' + k] for k in 'UVWS']))
    _, var2, a0, b0 = m.tip_signals
    frames = []
    with m.record_tips(every=10) as rec:
        for i in range(last_tick):
            st.step(1)
            if i == s2_tick:
                m.fire_op('s2')
            if (i + 1) % 10 == 0:
                frames.append((st.get_state(0), st.get_state(var2)))
        counts, records = st.tips_read()
        mask = rec.mask
    st.close()
    return counts, records, frames, a0, b0, mask


def test_reference_driver_protocol(gpu_lib, golden):
    """The inputs of fenton_driver96 as they are, S2 after tick 30, to tick 150: every sample equals the reference on the frame
    read back at its tick.

    Chosen on the CPU first (cpu_engine's oracle + tip_ref, the same protocol, 400 ticks): the oracle finds NO tip in any of
    the 40 samples — after ticks 10, 20, ... 400 the counts are 0 0 0 ... 0, and sampled every tick from 1 to 80 they are 0 as
    well.  S2 after 30 ms falls on the plateau of the S1 wave, which has not left the upper-left quadrant yet: the new front
    merges with the old one, nothing breaks, no rotor.  So on these inputs the reference itself cannot satisfy "at least N
    samples after S2 hold a tip" for any N >= 1 (with S2 moved to ticks 160, 180, ... 280 it finds one tip in one sample, at
    S2 = 180: the sheet is shorter than the wave).  N is what the reference gives, 0; what is asserted is equality at every
    sample, which includes that the device invents no tip either.  Samples that do hold tips are compared in the tests above."""
    counts, records, frames, a0, b0, mask = _driver96(golden, S2_TICK, LAST_TICK)
    assert len(frames) == LAST_TICK // 10
    check_samples(counts, records, frames, a0, b0, 256, mask, what='driver96, S2 after tick 30')
    held = int(np.count_nonzero(counts[S2_TICK // 10:, 2]))
    assert held >= N_AFTER_S2 and held == 0, counts[:, 2]
