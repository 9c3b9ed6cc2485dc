"""-m gpu: the frame recorder (include/fibhip.h fibhip_frames_*, fib_tf_amd/frames.py) on the device.

Every frame must EQUAL the NumPy restatement (tests/frame_ref.py) of the state read back at the frame's tick, bit for bit: no
tolerance anywhere in this file.  The grids are the smallest that reach each path of frame_kernel: 37 x 53 (scalar, odd
everything), 64 x 64 (16-byte loads and stores), 20 x 130 (rows not 16-byte aligned), 96 x 100 (several tiles, multi-tick
launches) and one 512 x 512 case (many workgroups)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_ref as ref  # noqa: E402
import tip_ref  # noqa: E402
from test_gpu_tips import MAKERS, fenton, br, court  # noqa: E402

pytestmark = pytest.mark.gpu

PLAN_ENV = ('FIBHIP_MT', 'FIBHIP_AHEAD', 'FIBHIP_MT_FAKE_GIVEUP', 'FIBHIP_VARIANT', 'FIBHIP_MT_MAX', 'FIBHIP_MT_IDS', 'FIBHIP_AUTOTUNE')
VARIANT_96x100 = '10,44,25,-3'                              # the forced small shape of tests/test_gpu_recovery.py: 12 tiles
BLOCKS = [((1, 1), 'mean'), ((2, 3), 'mean'), ((4, 4), 'point'), ((5, 1), 'mean'), ((16, 16), 'mean')]
PACE_V = {'fenton': 1.0, 'br': 10.0, 'court': 20.0, 'traced': 1.0}


def windows(H, W, by, bx):
    """the whole grid; a window ending at the last row and column; one block (a frame of one pixel); an odd first column"""
    r, c = (H - by) // 2, (W - bx) // 2
    return [(0, H, 0, W), (min(H // 3, H - by), H, min(W // 4, W - bx), W), (r, r + by, c, c + bx), (1, H, 5, W - 2)]


def levels_of(m):
    return ref.levels(m.min_v, m.max_v)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), '%s: %d of %d pixels differ' % (what, int((got != want).sum()), got.size)


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


def check_configs(m, kind, H, W, everys=(1, 3), blocks=BLOCKS, ticks=6):
    st = m._stepper
    lo, span = levels_of(m)
    rng = np.random.default_rng(H * 1000 + W)
    plane = rng.uniform(0.05, 1.0, (H, W)).astype(np.float32)
    n = varied = 0
    for every in everys:
        for (by, bx), reduce in blocks:
            if by > H or bx > W:
                continue
            for wi, win in enumerate(windows(H, W, by, bx)):
                for fmt in ('float32', 'uint8'):
                    weight = plane if (n + wi) % 2 == 0 else None
                    n += 1
                    st.frames_begin(0, win, (by, bx), reduce, lo, span, weight, fmt, every, every, ticks // every)
                    states = []
                    for i in range(ticks):
                        st.step(1)
                        if (i + 1) % every == 0:
                            states.append(st.get_state(0).copy())
                    assert st.frames_count() == ticks // every
                    got = st.frames_read()
                    what = '%s %dx%d every %d block %s %s window %s %s weight %s' % (kind, H, W, every, (by, bx), reduce, win, fmt,
                                                                                     weight is not None)
                    assert got.shape[0] == len(states), what
                    for s, x in enumerate(states):
                        want = ref.frame(x, win, (by, bx), reduce, lo, span, weight, fmt)
                        same(got[s], want, '%s frame %d' % (what, s))
                        if wi == 0 and fmt == 'float32' and want.size > 1:
                            varied += len(np.unique(want)) > 1
    st.frames_end()
    assert n > 0 and varied > 0                               # (the frames are not constants)
    return n


@pytest.mark.parametrize('shape', [(37, 53), (64, 64), (20, 130), (96, 100)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_frames_equal_the_restatement(gpu_lib, kind, shape):
    H, W = shape
    m = MAKERS[kind](H, W)
    wave(m, kind)
    n = check_configs(m, kind, H, W)
    print('%s %dx%d: %d configurations' % (kind, H, W, n))
    m._stepper.close()


def test_many_workgroups(gpu_lib):
    m = fenton(512, 512)
    wave(m, 'fenton')
    check_configs(m, 'fenton', 512, 512, everys=(2,), blocks=[((1, 1), 'mean'), ((2, 2), 'mean'), ((3, 5), 'mean')], ticks=2)
    m._stepper.close()


def test_other_arrays(gpu_lib):
    """var != 0 on a bare handle with noise in every array, levels that are not image()'s"""
    st = gpu_lib.Stepper(gpu_lib.FENTON4V, 64, 64, 0.1, 1.3, flags=gpu_lib.FAST)
    rng = np.random.default_rng(2)
    st.set_state(-1, rng.uniform(0, 1, (4, 64, 64)).astype(np.float32))
    plane = rng.uniform(0, 1, (64, 64)).astype(np.float32)
    win = (8, 56, 4, 60)
    for var in (0, 2, 3):
        for fmt in ('float32', 'uint8'):
            st.frames_begin(var, win, (2, 2), 'mean', 0.125, 0.75, plane, fmt, 1, 1, 2)
            st.step(1)
            x1 = st.get_state(var).copy()
            st.step(1)
            x2 = st.get_state(var).copy()
            got = st.frames_read()
            for s, x in enumerate((x1, x2)):
                same(got[s], ref.frame(x, win, (2, 2), 'mean', 0.125, 0.75, plane, fmt), 'var %d %s frame %d' % (var, fmt, s))
    st.close()


def _hole_model(cls_kind, ticks):
    if cls_kind == 'fenton':
        from fib_tf_amd.fenton import Fenton4v
        m = Fenton4v({'height': 96, 'width': 100, 'dt': 0.1, 'dt_per_plot': 100, 'diff': 1.5, 'duration': 1000})
        m.add_hole_to_phase_field(50, 48, 9)
    else:
        from fib_tf_amd.br import BeelerReuter
        m = BeelerReuter({'height': 96, 'width': 100, 'dt': 0.1, 'dt_per_plot': 100, 'diff': 0.809, 'duration': 1000,
                          'cheby': True, 'skip': False})
    m.define()
    m.dt_per_plot = 10 * m.dt_per_step                        # a frame every ten ticks
    m.duration = (ticks + 0.5) * m.dt_per_step * m.dt
    return m


@pytest.mark.parametrize('kind', ['fenton', 'br'])
def test_first_1_is_the_cadence_of_run(gpu_lib, kind):
    """full-resolution float32 frames with first = 1 against a twin model polled the way run(im) paints: image() * phase after
    loop ticks 0, 10, 20, 30"""
    ticks = 35
    twin = _hole_model(kind, ticks)
    polled = []
    for i in twin.run():
        if i % 10 == 0:
            image = twin.image()
            if twin.phase is not None:
                image *= twin.phase
            polled.append(np.array(image, np.float32))
    twin._stepper.close()
    m = _hole_model(kind, ticks)
    with m.record_frames(every=10, first=1) as rec:
        assert rec.capacity == 4 and rec.shape == (96, 100) and rec.dtype == np.float32
        assert (rec.weight is None) == (m.phase is None)
        for i in m.run():
            pass
        assert rec.count() == 4
        got = rec.frames()
        assert np.allclose(rec.times(), (1 + 10 * np.arange(4)) * rec.tick_ms)
    assert len(polled) == 4
    for s in range(4):
        same(got[s], polled[s], '%s frame %d' % (kind, s))
    assert len(np.unique(got[3])) > 10
    m._stepper.close()


def _plan_run(gpu_lib, monkeypatch, env, record):
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
            st.frames_begin(0, (0, 96, 0, 100), (2, 2), 'mean', 0.0, 1.0, plane, 'float32', 10, 10, 4)
        for i in range(40):
            st.step(1)
        if record:
            assert st.frames_count() == 4
            out = st.frames_read()
        state = st.get_state(-1)
        fb, s1 = st.fallbacks(), st.launch_stats()
    st.close()
    return out, state, fb, {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}


def test_frames_do_not_depend_on_the_launch_plan(gpu_lib, monkeypatch):
    frames, state, fb, stats = _plan_run(gpu_lib, monkeypatch, {}, True)
    assert fb[0] == 0
    # between two frames the handle runs the fewest launches `every` allows: four ten-tick launches, four samples
    assert stats['ticks'] == 40 and stats['mt_ticks'] == 40 and stats['mt_launches'] == 4, stats
    assert stats['launches'] == stats['mt_launches'] + 4, stats
    assert frames.shape == (4, 48, 50) and any(frames[s].tobytes() != frames[0].tobytes() for s in range(1, 4))
    for env in ({'FIBHIP_MT': '0'}, {'FIBHIP_AHEAD': '0'}, {'FIBHIP_MT_FAKE_GIVEUP': '2'}):
        f2, st2, fb2, stats2 = _plan_run(gpu_lib, monkeypatch, env, True)
        same(f2, frames, str(env))
        assert st2.tobytes() == state.tobytes(), env
        assert stats2['ticks'] == 40, (env, stats2)
        if 'FIBHIP_MT_FAKE_GIVEUP' in env:
            assert fb2[0] == 1 and fb2[1] > 0, fb2            # one launch gave up and was recovered
        if 'FIBHIP_MT' in env:
            assert stats2['mt_ticks'] == 0
    _, plain, _, pstats = _plan_run(gpu_lib, monkeypatch, {}, False)
    assert plain.tobytes() == state.tobytes()                 # the recorder changes nothing of the state
    assert pstats['ticks'] == 40 and pstats['mt_ticks'] > 0
    assert pstats['launches'] == pstats['mt_launches'] + (pstats['ticks'] - pstats['mt_ticks']), pstats


def _three(gpu_lib, which, ticks=60):
    """electrodes every 3, tips every 4 and frames every 5 ticks (those named in `which`) on one Fenton handle, one call"""
    from fib_tf_amd import egm
    m = fenton(96, 100)
    st = m._stepper
    wave(m, 'fenton')
    _, var2, a0, b0 = m.tip_signals
    rect, patch = egm.crop_mask(egm.create_mask(m, 60, 40, 5))
    s0 = st.launch_stats()
    if 'el' in which:
        st.electrode_begin(0, [rect], [patch], 3, ticks // 3)
    if 'tip' in which:
        st.tips_begin(0, var2, a0, b0, None, 4, 256, ticks // 4)
    if 'fr' in which:
        st.frames_begin(0, (0, 96, 0, 100), (2, 2), 'mean', 0.0, 1.0, None, 'uint8', 5, 5, ticks // 5)
    st.step(ticks)
    out = {}
    if 'el' in which:
        out['el'] = st.electrode_read().tobytes()
    if 'tip' in which:
        c, r = st.tips_read()
        out['tip'] = (c.tobytes(), [tip_ref.sorted_records(r[s], c[s, 2], 256).tobytes() for s in range(len(c))])
    if 'fr' in which:
        out['fr'] = st.frames_read().tobytes()
    s1 = st.launch_stats()
    st.close()
    return out, {k: s1[k] - s0[k] for k in s0 if k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}


def test_three_samplers_on_one_handle(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    all3, stats = _three(gpu_lib, ('el', 'tip', 'fr'))
    cuts = [t for t in range(1, 61) if t % 3 == 0 or t % 4 == 0 or t % 5 == 0]
    lengths = np.diff([0] + cuts)
    samples = 60 // 3 + 60 // 4 + 60 // 5
    assert stats['ticks'] == 60, stats
    # no launch spans a sample tick of any of the three: one launch per stretch between two of them (a stretch of one tick is a
    # plain launch), and one launch per sample (the electrode is one chunk)
    assert stats['mt_launches'] == int((lengths >= 2).sum()) and stats['mt_ticks'] == int(lengths[lengths >= 2].sum()), (stats, lengths)
    assert stats['launches'] == len(cuts) + samples, (stats, len(cuts), samples)
    for which in ('el', 'tip', 'fr'):
        alone, _ = _three(gpu_lib, (which,))
        assert alone[which] == all3[which], which             # each records what it records alone


def test_with_the_activation_recorder_every_tick_is_one_launch(gpu_lib, monkeypatch):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('FIBHIP_VARIANT', VARIANT_96x100)
    frames = []
    for activation in (False, True):
        m = fenton(96, 100)
        st = m._stepper
        wave(m, 'fenton')
        rec = m.record_activation() if activation else None
        st.frames_begin(0, (0, 96, 0, 100), (1, 1), 'mean', 0.0, 1.0, None, 'float32', 5, 5, 4)
        s0 = st.launch_stats()
        st.step(20)
        assert st.frames_count() == 4
        frames.append(st.frames_read())
        s1 = st.launch_stats()
        assert s1['ticks'] - s0['ticks'] == 20
        if activation:
            assert s1['mt_ticks'] == s0['mt_ticks']
            assert s1['launches'] - s0['launches'] == 20 + 20 + 4     # a tick, the activation recorder's kernel, and the frames
            rec.close()
        else:
            assert s1['mt_launches'] - s0['mt_launches'] == 4 and s1['launches'] - s0['launches'] == 8
        st.close()
    same(frames[1], frames[0], 'with the activation recorder')


def test_court_frame_of_a_slow_array_is_taken_before_slow(gpu_lib):
    """a frame of a slow array due at the tick 'slow' would ride on: the two are not fused, the frame holds the array as the
    tick left it"""
    from fib_tf_amd.court import Courtemanche
    slow_var = Courtemanche.tip_signals[1]                    # a gate 'slow' assigns
    assert Courtemanche.VAR_NAMES[slow_var] not in ('V', '_Na_i_', '_m_', '_h_')
    twin = court(64, 80)
    wave(twin, 'court')
    twin._stepper.step(5)
    before = twin._stepper.get_state(slow_var).copy()
    twin.fire_op('slow')
    after = twin._stepper.get_state(slow_var).copy()
    twin._stepper.close()
    assert before.tobytes() != after.tobytes()
    m = court(64, 80)
    wave(m, 'court')
    st = m._stepper
    st.frames_begin(slow_var, (0, 64, 0, 80), (1, 1), 'mean', 0.0, 1.0, None, 'float32', 5, 5, 2)
    st.step(5)                                                # (the last tick may be held back for 'slow' to ride on)
    m.fire_op('slow')
    assert st.frames_count() == 1
    got = st.frames_read()
    same(got[0], ref.frame(before, None, (1, 1), 'mean', 0.0, 1.0), 'slow array')
    same(st.get_state(slow_var), after, 'the state behind it')
    st.close()


@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_capacity_windows_and_reattachment(gpu_lib, kind):
    m = MAKERS[kind](37, 53)
    wave(m, kind)
    st = m._stepper
    lo, span = levels_of(m)
    st.frames_begin(0, None, (1, 1), 'mean', lo, span, None, 'float32', 2, 2, 3)
    assert st.frames_shape() == (37, 53, np.dtype(np.float32))
    st.step(5)
    assert st.frames_count() == 2                             # (ticks accepted but not launched yet count)
    st.sync()
    ticks = st.launch_stats()['ticks']
    two = st.frames_read()
    state = st.get_state(-1)
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(3)                                            # would take frame number 3
    st.sync()
    assert st.launch_stats()['ticks'] == ticks                # nothing of the refused call ran
    assert st.get_state(-1).tobytes() == state.tobytes() and st.frames_read().tobytes() == two.tobytes()
    st.step(1)                                                # frame number 2 still fits: the cube is full now
    with pytest.raises(gpu_lib.FibhipError, match='trace full'):
        st.step(2)
    st.sync()
    assert st.launch_stats()['ticks'] == ticks + 1
    cube = st.frames_read()
    assert cube.shape == (3, 37, 53) and st.frames_count() == 3 and cube[:2].tobytes() == two.tobytes()
    same(cube[2], ref.frame(st.get_state(0), None, (1, 1), 'mean', lo, span), '%s last frame' % kind)
    assert st.frames_read(1, 2).tobytes() == cube[1:].tobytes()
    assert st.frames_read(0, 1).tobytes() == cube[:1].tobytes()
    assert st.frames_read(3, 0).shape == (0, 37, 53)
    for first, count in ((0, 4), (2, 2), (-1, 1), (4, 0), (0, -1)):
        with pytest.raises(gpu_lib.FibhipError, match='frames_read'):
            st.frames_read(first, count)
    st.frames_begin(0, (1, 36, 3, 51), (5, 4), 'point', lo, span, None, 'uint8', 3, 1, 4)       # another shape and format
    assert st.frames_count() == 0 and st.frames_shape() == (7, 12, np.dtype(np.uint8)) and st.frames_read().shape == (0, 7, 12)
    st.step(1)
    x = st.get_state(0).copy()
    st.step(2)
    assert st.frames_count() == 1                             # first = 1: after ticks 1, 4, 7, ...
    st.step(1)
    got = st.frames_read()
    assert got.shape == (2, 7, 12) and got.dtype == np.uint8
    same(got[0], ref.frame(x, (1, 36, 3, 51), (5, 4), 'point', lo, span, None, 'uint8'), 'first = 1')
    same(got[1], ref.frame(st.get_state(0), (1, 36, 3, 51), (5, 4), 'point', lo, span, None, 'uint8'), 'first = 1, second frame')
    st.frames_end()
    st.frames_end()                                           # (nothing attached: nothing to do)
    with pytest.raises(gpu_lib.FibhipError, match='no recorder'):
        st.frames_read(0, 0)
    with pytest.raises(gpu_lib.FibhipError, match='no recorder'):
        st.frames_count()
    with pytest.raises(gpu_lib.FibhipError, match='no recorder'):
        st.frames_shape()
    st.step(30)                                               # the handle runs on without a recorder
    st.frames_begin(0, None, (1, 1), 'mean', lo, span, None, 'float32', 1, 1, 2)
    st.step(1)
    st.close()                                                # destroyed with a recorder attached


def test_refusals(gpu_lib):
    import ctypes as C
    m = fenton(64, 80)
    st = m._stepper
    L, h = st._L, st._h
    plane = np.ones((64, 80), np.float32)

    def begin(var=0, win=(0, 64, 0, 80), by=1, bx=1, reduce=1, lo=0.0, span=1.0, weight=None, fmt=0, every=2, first=2, cap=4, handle=h):
        w = (C.c_int * 4)(*win) if win is not None else None
        wp = weight.ctypes.data_as(C.POINTER(C.c_float)) if weight is not None else None
        return L.fibhip_frames_begin(handle, var, w, by, bx, reduce, lo, span, wp, fmt, every, first, cap)
    assert begin(weight=plane) == 0
    bad = [dict(var=-1), dict(var=st.nvar), dict(win=None), dict(win=(-1, 64, 0, 80)), dict(win=(0, 65, 0, 80)), dict(win=(0, 64, -1, 80)),
           dict(win=(0, 64, 0, 81)), dict(win=(10, 10, 0, 80)), dict(win=(0, 64, 30, 20)), dict(by=0), dict(bx=0), dict(by=17), dict(bx=17),
           dict(by=-1), dict(win=(0, 3, 0, 80), by=4), dict(win=(0, 64, 8, 13), bx=6), dict(reduce=2), dict(reduce=-1), dict(fmt=2),
           dict(fmt=-1), dict(span=0.0), dict(span=float('inf')), dict(span=float('nan')), dict(lo=float('nan')), dict(every=0),
           dict(every=-2), dict(first=0), dict(first=3), dict(first=-1), dict(cap=0), dict(cap=-1), dict(cap=2 ** 62)]
    for kw in bad:
        assert begin(**kw) == -1, kw
        assert b'frames_begin' in L.fibhip_last_error(), kw
    assert st.frames_count() == 0 and st.frames_shape()[:2] == (64, 80)        # the refused calls left the first recorder attached
    st.step_edges()
    assert begin() != 0 and b'open tick' in L.fibhip_last_error()
    st.step_interior()
    st.step_commit()
    st.step(1)
    assert st.frames_count() == 1
    assert begin(handle=None) != 0
    oh = C.c_int()
    assert L.fibhip_frames_shape(None, C.byref(oh), None, None) != 0
    k = C.c_longlong()
    assert L.fibhip_frames_count(h, None) != 0
    assert L.fibhip_frames_read(h, 0, 1, None) != 0 and b'null destination' in L.fibhip_last_error()
    assert L.fibhip_frames_end(h) == 0 and L.fibhip_frames_end(h) == 0          # end without begin: nothing
    assert L.fibhip_frames_count(h, C.byref(k)) != 0 and b'no recorder' in L.fibhip_last_error()
    with pytest.raises(ValueError, match='weight plane'):
        st.frames_begin(weight=np.ones((3, 3), np.float32))
    st.close()


def test_row_block_refused_by_the_library(gpu_lib):
    import ctypes as C
    blk = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    rc = blk._L.fibhip_frames_begin(blk._h, 0, (C.c_int * 4)(0, 42, 0, 40), 1, 1, 1, 0.0, 1.0, None, 0, 1, 1, 4)
    assert rc == -1 and b'row block' in blk._L.fibhip_last_error()
    blk.close()


@pytest.mark.parametrize('kind', ['fenton', 'br', 'court', 'traced'])
def test_timeline_lists_the_frame(gpu_lib, kind):
    m = MAKERS[kind](96, 130)
    st = m._stepper
    st.step(1)
    st.frames_begin(0, None, (2, 2), 'mean', 0.0, 1.0, None, 'uint8', 2, 2, 8)
    names = [e['name'] for e in st.trace_tick()] + ['|'] + [e['name'] for e in st.trace_tick()]
    assert names.count('frame_kernel') == 1 and names.index('frame_kernel') > names.index('|'), names      # once per sample
    assert st.frames_count() == 1
    st.close()


def test_recorder_object(gpu_lib, tmp_path):
    """FrameRecorder end to end on a model with a hole: defaults, the image() check, save / play"""
    from fib_tf_amd import playcube
    from fib_tf_amd.screen import Screen
    m = _hole_model('fenton', 12)
    st = m._stepper
    with m.record_frames(every=4, block=(2, 2), fmt='uint8') as rec:
        assert rec.first == 4 and rec.capacity == 3 and rec.shape == (48, 50) and np.array_equal(rec.weight, m.phase)
        states = []
        for i in m.run():
            if (i + 1) % 4 == 0:
                states.append(st.get_state(0).copy())
        assert rec.count() == 3
        cube = rec.frames()
        for s, x in enumerate(states):
            same(cube[s], ref.frame(x, None, (2, 2), 'mean', 0.0, 1.0, m.phase, 'uint8'), 'frame %d' % s)
        assert np.allclose(rec.times(), [4 * rec.tick_ms, 8 * rec.tick_ms, 12 * rec.tick_ms])
        rec.save(str(tmp_path / 'cube'))
        saved = np.load(str(tmp_path / 'cube.npy'))
        assert saved.dtype == np.uint8 and saved.tobytes() == cube.tobytes()
        sc = rec.play(Screen(48, 50, keep=3))
        assert sc.count == 3 and np.array_equal(sc.frames[2], cube[2] / np.float32(255))
        assert playcube.play(str(tmp_path / 'cube.npy'), delay=0).count == 3
    with pytest.raises(AssertionError, match='closed'):
        rec.count()
    b = br(37, 53)
    with pytest.raises(ValueError, match='levels='):
        b.record_frames(levels=(0.0, 1.0))                    # image() rescales: these levels are not it
    with b.record_frames(window=(0, 37, 0, 52), block=(1, 4)) as rec:
        assert rec.levels == tuple(float(v) for v in ref.levels(-90.0, 30.0)) and rec.shape == (37, 13)
    with b.record_frames(var=3, levels=(0.5, 2.0), weight=None) as rec:     # no image() for another array: nothing to check
        b._stepper.step(1)
        same(rec.frames()[0], ref.frame(b._stepper.get_state(3), None, (1, 1), 'mean', 0.5, 2.0), 'var 3')
    with pytest.raises(ValueError, match='first'):
        b.record_frames(every=3, first=4)
    b._stepper.close()
    st.close()
