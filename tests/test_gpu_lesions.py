"""-m gpu: the lesion program (include/fibhip.h fibhip_lesion_*, fib_tf_amd/lesions.py) on the device.

No tolerance anywhere in this file.  The defining property, bit for bit: a run with a lesion after tick i EQUALS running i + 1
ticks, reading the state, building a fresh model whose phase field is the old one with the same lesion applied on the host
(tests/lesion_ref.py), define(state=...), and running the remaining ticks.  The grid is 70 x 130 — an odd width in tiles, rows
not 16-byte aligned, 3 x 3 tiles of the forced strip shapes — with a hole in the field and a plane wave from the left that
reaches the lesions within the run.

Not covered: "one tick with stale derived planes differs" — there is no way to update phi alone without a hook in the library, so
the derived planes are held by the state equality (the tick after the event reads them) only."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lesion_ref as ref  # noqa: E402
from test_gpu_frames import PACE_V, PLAN_ENV  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 70, 130
STRIP = {'fenton': '10,44,25,-3', 'br': '5,54,21,-2'}        # forced strip shapes: 3 x 3 and 4 x 3 tiles of the grid
K1 = '1,64,4,256'                                             # one sub-step per launch
CONFIG = {'fenton': dict(diff=1.5), 'br': dict(diff=0.809, cheby=True, skip=False), 'court': dict(diff=0.809)}


def set_env(monkeypatch, env):
    for k in PLAN_ENV + ('FIBHIP_K',):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


NOISE = {'on': False}                                              # test_geometry_cases: gradients everywhere, so every lesion matters


def make(kind, fast=True, phase=None, state=None, shape=(H, W)):
    """a model on the grid with `phase` (default: one hole), resumed from `state` or freshly defined with a plane wave from the
    left edge and a second one from a band in the middle (the lesions near the hole lie in its way) — or, with NOISE set, a
    potential of sub-threshold noise: a gradient in every cell"""
    from fib_tf_amd.br import BeelerReuter
    from fib_tf_amd.court import Courtemanche
    from fib_tf_amd.fenton import Fenton4v
    cls = {'fenton': Fenton4v, 'br': BeelerReuter, 'court': Courtemanche}[kind]
    m = cls(dict(CONFIG[kind], height=shape[0], width=shape[1], dt=0.1, dt_per_plot=10, duration=1000, fast_math=fast))
    m.phase = (ref.hole_field(*shape) if phase is None else np.array(phase, np.float32)) if phase is not False else None
    if state is not None:
        m.define(state=dict(zip(m.VAR_NAMES, state)))
        return m
    m.define()
    m._stepper.pace(*m.pace_rect('left'), PACE_V[kind], float(m.min_v))
    m._stepper.pace(0, shape[0], shape[1] // 2, shape[1] // 2 + 8, PACE_V[kind], float(m.min_v))
    if NOISE['on']:
        m._stepper.set_state(0, np.random.default_rng(11).uniform(0.0, 0.25, shape).astype(np.float32))
    return m


def tick(m, kind, i):
    m._stepper.step(1)
    if kind == 'court' and i % 10 == 0:
        m.fire_op('slow')


def run_program(kind, fast, program, ticks, phase=None):
    """`program`: [(site, tick)].  -> (state, field, applied)"""
    from fib_tf_amd.lesions import Lesion
    m = make(kind, fast, phase)
    with m.program_lesions([Lesion(s, at_tick=t) for s, t in program]) as prog:
        assert prog.events(ticks) == ref.events([t for _, t in program], ticks)
        for i in range(ticks):
            tick(m, kind, i)
        state, field, applied = m._stepper.get_state(-1), prog.phase(), prog.applied()
    assert m.phase.tobytes() == field.tobytes()                   # end(): model.phase is the field as it now is
    m._stepper.close()
    return state, field, applied


def run_split(kind, fast, program, ticks, phase=None):
    """the definition: at every event tick the state is read, the lesions of that tick are applied to the field on the host in
    program order, and a fresh model goes on from there"""
    m = make(kind, fast, phase)
    field = m.phase.copy()
    for i in range(ticks):
        tick_body = [s for s, t in program if t == i]
        m._stepper.step(1)
        if tick_body:
            state = m._stepper.get_state(-1)
            m._stepper.close()
            field = ref.apply_sites(field, m.height, m.width, tick_body)
            m = make(kind, fast, field, state)
        if kind == 'court' and i % 10 == 0:
            m.fire_op('slow')
    state = m._stepper.get_state(-1)
    m._stepper.close()
    return state, field


def run_plain(kind, fast, ticks, phase=None):
    m = make(kind, fast, phase)
    for i in range(ticks):
        tick(m, kind, i)
    state = m._stepper.get_state(-1)
    m._stepper.close()
    return state


def same_state(got, want, what):
    for v in range(got.shape[0]):
        assert got[v].tobytes() == want[v].tobytes(), '%s: array %d differs in %d cells' % (what, v, int((got[v] != want[v]).sum()))


# a disc in the wave's way, the ordered pair next to the hole on one tick, and a line of block later
PROGRAM = [(('disc', 30, 12, 4), 5), (ref.ORDER_PAIR[0], 9), (ref.ORDER_PAIR[1], 9), (('line', 50, 2, 60, 30, 1.5), 12)]
PLANS = [('fenton', True, 'default'), ('fenton', False, 'default'), ('fenton', True, 'strip'), ('fenton', True, 'k1'),
         ('br', True, 'default'), ('br', False, 'default'), ('br', True, 'strip'), ('court', True, 'default')]


@pytest.mark.parametrize('mt', ['mt', 'mt0'])
@pytest.mark.parametrize('kind,fast,plan', PLANS, ids=['%s-%s-%s' % (k, 'fast' if f else 'faithful', p) for k, f, p in PLANS])
def test_the_defining_property(gpu_lib, monkeypatch, kind, fast, plan, mt):
    """Fenton and Beeler-Reuter under both arithmetic policies, Courtemanche (fast) with its 'slow' on the event tick (10) and next
    to it (9, 11); the default plan, a forced strip shape and the forced one-sub-step kernel, each with multi-tick launches allowed
    and with FIBHIP_MT=0"""
    env = {'strip': {'FIBHIP_VARIANT': STRIP.get(kind, '')}, 'k1': {'FIBHIP_VARIANT': K1}, 'default': {}}[plan]
    if mt == 'mt0':
        env['FIBHIP_MT'] = '0'
    set_env(monkeypatch, env)
    program = PROGRAM if kind != 'court' else [(PROGRAM[0][0], 9), (PROGRAM[1][0], 10), (PROGRAM[2][0], 10), (PROGRAM[3][0], 11)]
    ticks = 18
    got, field, applied = run_program(kind, fast, program, ticks)
    want, wfield = run_split(kind, fast, program, ticks)
    what = '%s %s %s %s' % (kind, fast, plan, mt)
    assert applied == len(program)
    assert field.tobytes() == wfield.tobytes(), '%s: the field differs in %d cells' % (what, int((field != wfield).sum()))
    same_state(got, want, what)
    assert np.isfinite(got).all()
    plain = run_plain(kind, fast, ticks)
    assert plain[0].tobytes() != got[0].tobytes()                 # (a lesion that silently did nothing fails here)


def geometry_cases(tx, ty):
    whole = np.random.default_rng(3).uniform(0.5, 1.0, (H, W)).astype(np.float32)
    whole[whole == 1.0] = 0.75
    cell = np.ones((H, W), np.float32)
    cell[33, 71] = 0.5
    return {'four tiles meet': [('disc', ty, tx, 2)], 'row 0 and column 0': [('disc', 0, 0, 3)],
            'last row and column': [('disc', H - 1, W - 1, 3)], 'over the hole': [('disc', 40, 90, 16)], 'one cell': [cell],
            'whole grid': [whole], 'ordered pair on one tick': list(ref.ORDER_PAIR)}


@pytest.mark.parametrize('case', ['four tiles meet', 'row 0 and column 0', 'last row and column', 'over the hole', 'one cell', 'whole grid',
                                  'ordered pair on one tick'])
def test_geometry_cases(gpu_lib, monkeypatch, case):
    """Fenton at the forced 44 x 25 strip shape: 3 x 3 tiles of the 70 x 130 grid (asserted from plan_tile())"""
    set_env(monkeypatch, {'FIBHIP_VARIANT': STRIP['fenton']})
    monkeypatch.setitem(NOISE, 'on', True)
    probe = make('fenton')
    tx, ty, _ = probe._stepper.plan_tile()
    probe._stepper.close()
    assert (tx, ty) == (44, 25) and H >= 2 * ty and W >= 2 * tx
    sites = geometry_cases(tx, ty)[case]
    if case == 'four tiles meet':
        box = ref.patch(H, W, sites[0])[0]
        assert box[0] < ty < box[1] and box[2] < tx < box[3]
    if case == 'one cell':
        assert ref.patch(H, W, sites[0])[0] == (33, 34, 71, 72)
    if case == 'whole grid':
        assert ref.patch(H, W, sites[0])[0] == (0, H, 0, W)
    program = [(s, 4) for s in sites]
    got, field, applied = run_program('fenton', True, program, 10)
    want, wfield = run_split('fenton', True, program, 10)
    assert applied == len(sites) and field.tobytes() == wfield.tobytes(), (case, int((field != wfield).sum()))
    same_state(got, want, case)
    if case == 'ordered pair on one tick':                        # (the other order is another field: the test can tell)
        assert ref.apply_sites(ref.hole_field(), H, W, sites[::-1]).tobytes() != field.tobytes()
    assert run_plain('fenton', True, 10)[0].tobytes() != got[0].tobytes()


def test_ten_lesions_on_one_tick_and_a_model_without_a_field(gpu_lib, monkeypatch):
    """more entries due after one tick than one launch takes (eight), overlapping in a chain; and a model WITHOUT a phase field,
    which is given a field of ones — equal to the model defined with a field of ones"""
    set_env(monkeypatch, {})
    sites = [('disc', 30 + (i % 3), 8 + 3 * i, 2) for i in range(10)]
    program = [(s, 3) for s in sites]
    ones = np.ones((H, W), np.float32)
    got, field, applied = run_program('fenton', True, program, 8, phase=False)
    want, wfield = run_split('fenton', True, program, 8, phase=ones)
    assert applied == 10 and field.tobytes() == wfield.tobytes()
    same_state(got, want, 'ten lesions')


def test_ablate_equals_the_program(gpu_lib, monkeypatch):
    """ablate() after tick i equals the program with at_tick = i — with a tip recorder and a stimulus program attached"""
    from fib_tf_amd.lesions import Lesion
    from fib_tf_amd.stimulus import Stimulus
    set_env(monkeypatch, {'FIBHIP_VARIANT': STRIP['fenton']})
    site, at = ('disc', 30, 12, 4), 6

    def run(programmed):
        m = make('fenton')
        tips = m.record_tips(every=4)
        stim = m.program_stimuli([Stimulus('luq', 1.0, at_tick=3), Stimulus('left', 1.0, at_tick=at)])
        prog = m.program_lesions([Lesion(site, at_tick=at)]) if programmed else None
        for i in range(14):
            m._stepper.step(1)
            if not programmed and i == at:
                assert m.ablate(site) == ref.patch(H, W, site)[0]
        out = (m._stepper.get_state(-1).tobytes(), m._stepper.get_phase().tobytes(), tips.counts().tobytes(), stim.applied())
        if prog:
            assert prog.applied() == 1
            prog.end()
        assert m.phase.tobytes() == out[1]
        m._stepper.close()
        return out
    a, b = run(True), run(False)
    assert a == b and a[3] == 2
    assert a[1] == ref.apply_sites(ref.hole_field(), H, W, [site]).tobytes()


def launches_of(st, calls):
    s0 = st.launch_stats()
    marks = []
    for _ in range(calls):
        st.step(1)
        s = st.launch_stats()
        marks.append((s['mt_launches'] - s0['mt_launches'], s['mt_ticks'] - s0['mt_ticks'], s['launches'] - s0['launches']))
    st.sync()
    s1 = st.launch_stats()
    return {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}, marks


def test_launches_are_cut_at_the_events(gpu_lib, monkeypatch):
    """events after ticks 9 and 40 of 64 single-tick calls at the forced shape (launches of up to 32 ticks): the ten ticks up to
    the first event are ONE launch, issued when the tenth is waiting, the 31 up to the second are one more; each event adds its
    two kernels.  With no event left the handle goes back to the launches of a caller that just keeps stepping — 4, 8, and the
    11 left at the sync (fibhip_step: 2, 4, ... doubling from the 2 it stood at after the first launch)"""
    from fib_tf_amd.lesions import Lesion
    set_env(monkeypatch, {'FIBHIP_VARIANT': STRIP['fenton']})
    m = make('fenton')
    st = m._stepper
    st.sync()
    prog = m.program_lesions([Lesion(('disc', 30, 12, 4), at_tick=9), Lesion(('disc', 50, 60, 3), at_tick=40)])
    stats, marks = launches_of(st, 64)
    assert marks[8] == (0, 0, 0) and marks[9] == (1, 10, 3), marks[:10]
    assert marks[39] == (1, 10, 3) and marks[40] == (2, 41, 6), marks[39:41]
    assert stats['ticks'] == 64 and stats['mt_ticks'] == 64, stats
    assert stats['mt_launches'] == 5 and stats['launches'] == 5 + 4, stats
    assert prog.applied() == 2
    prog.end()
    st.close()


def test_a_handle_without_a_program_launches_as_before(gpu_lib, monkeypatch):
    """3 ticks, then 40: 3, 32 + 8 — the counts tests/test_gpu_stimulus.py holds the scheduler to — on a handle that never had a
    lesion program, on one whose program has no event left, and on one whose program was detached.  A program with an event in
    the FAR FUTURE cannot have those counts: by the launch rule a handle with events still to come sends a launch out when the
    ticks up to the next event — or a full launch of 32 — are waiting, so 3 + 40 ticks are launches of 32 and 11, whatever the
    call pattern (the stimulus program's rule, which a sampler with a long stride follows too)"""
    from fib_tf_amd.lesions import Lesion
    set_env(monkeypatch, {'FIBHIP_VARIANT': STRIP['fenton']})
    seen = []
    for how in ('never', 'no event left', 'detached'):
        m = make('fenton')
        st = m._stepper
        st.sync()
        prog = m.program_lesions([Lesion(('disc', 30, 12, 4), at_tick=2 if how == 'no event left' else 0)]) if how != 'never' else None
        if how == 'detached':
            st.step(1)
            prog.end()
        s0 = st.launch_stats()
        st.step(3)
        st.step(40)
        st.sync()
        s1 = st.launch_stats()
        d = {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
        extra = 2 if how == 'no event left' else 0                    # (the event's two kernels)
        assert d['mt_ticks'] == 43 and d['mt_launches'] == 3 and d['launches'] == 3 + extra, (how, d)
        seen.append(d['mt_launches'])
        st.close()
    assert seen == [3, 3, 3]
    m = make('fenton')
    st = m._stepper
    st.sync()
    prog = m.program_lesions([Lesion(('disc', 30, 12, 4), at_tick=10 ** 6)])
    s0 = st.launch_stats()
    st.step(3)
    mid = st.launch_stats()
    st.step(40)
    full = st.launch_stats()
    st.sync()
    s1 = st.launch_stats()
    assert mid['mt_ticks'] == s0['mt_ticks'] and full['mt_ticks'] - s0['mt_ticks'] == 32 and full['mt_launches'] - s0['mt_launches'] == 1
    assert s1['mt_ticks'] - s0['mt_ticks'] == 43 and s1['mt_launches'] - s0['mt_launches'] == 2 and s1['launches'] - s0['launches'] == 2
    assert prog.applied() == 0
    st.close()


def test_timeline_lists_both_kernels(gpu_lib, monkeypatch):
    from fib_tf_amd.lesions import Lesion
    set_env(monkeypatch, {})
    m = make('fenton')
    st = m._stepper
    st.step(1)
    tips = m.record_tips(every=1)
    prog = m.program_lesions([Lesion(('disc', 30, 12, 4), at_tick=1)])
    names = [e['name'] for e in st.trace_tick()] + ['|'] + [e['name'] for e in st.trace_tick()]
    assert names.count('lesion_apply_kernel') == 1 and names.count('lesion_prep_kernel') == 1, names
    cut = names.index('|')
    assert cut < max(i for i, n in enumerate(names) if n == 'tip_kernel') < names.index('lesion_apply_kernel') < names.index('lesion_prep_kernel')
    assert prog.applied() == 1 and len(tips.counts()) == 2
    st.close()


def test_refusals(gpu_lib, monkeypatch):
    import ctypes as C
    set_env(monkeypatch, {})
    m = make('fenton')
    st = m._stepper
    L, h = st._L, st._h
    fp = C.POINTER(C.c_float)

    def begin(n=None, nfloats=None, patch=None, handle=h, entries=None, **kw):
        entries = [dict(dict(offset=0, tick=0, r0=2, r1=4, c0=3, c1=6), **kw)] if entries is None else entries
        arr = (gpu_lib.LesionEntry * max(len(entries), 1))()
        for i, e in enumerate(entries):
            for k, val in e.items():
                setattr(arr[i], k, val)
        p = np.full(64, 0.5, np.float32) if patch is None else np.asarray(patch, np.float32)
        return L.fibhip_lesion_begin(handle, len(entries) if n is None else n, arr, p.size if nfloats is None else nfloats, p.ctypes.data_as(fp))
    bad = [(dict(r0=4, r1=4), b'entry 0: rows [4, 4) x columns [3, 6) is empty or outside the 70 x 130 grid'),
           (dict(r1=71), b'is empty or outside'), (dict(c0=-1), b'is empty or outside'), (dict(c1=131), b'is empty or outside'),
           (dict(tick=-1), b'entry 0: tick must be >= 0'), (dict(reserved=7), b'entry 0: the reserved field must be 0 (got 7)'), (dict(offset=-1), b'entry 0: a patch of 6 floats at offset -1 of 64'),
           (dict(offset=59), b'at offset 59 of 64'), (dict(n=0), b'1 .. 256 entries'), (dict(n=257), b'1 .. 256 entries'),
           (dict(nfloats=0), b'floats of patches'), (dict(nfloats=8 * H * W + 1), b'floats of patches'),
           (dict(patch=[0.5, 1.5] * 32), b'entry 0: factor 1 of the patch is 1.5'), (dict(patch=[-0.25] * 64), b'factor 0 of the patch is -0.25'),
           (dict(patch=[np.nan] * 64), b'every factor is finite and in [0, 1]'), (dict(patch=[np.inf] * 64), b'every factor is finite and in [0, 1]')]
    for kw, msg in bad:
        assert begin(**kw) == -1, kw
        err = L.fibhip_last_error()
        assert b'lesion_begin' in err and msg in err, (kw, err)
    assert begin(entries=[dict(offset=0, tick=0, r0=2, r1=4, c0=3, c1=6), dict(offset=6, tick=1, r0=0, r1=80, c0=0, c1=1)]) == -1
    assert b'entry 1' in L.fibhip_last_error()
    k = C.c_longlong()
    assert L.fibhip_lesion_count(h, C.byref(k)) != 0 and b'no program' in L.fibhip_last_error()
    assert L.fibhip_lesion_end(h) == 0                                # (nothing attached: nothing)
    assert begin() == 0
    assert begin() == -1 and b'attached already' in L.fibhip_last_error()
    assert L.fibhip_lesion_count(h, C.byref(k)) == 0 and k.value == 0 and L.fibhip_lesion_count(h, None) != 0
    st.step(1)
    assert st.lesion_count() == 1
    assert L.fibhip_lesion_end(h) == 0 and L.fibhip_lesion_end(h) == 0
    st.step_edges()
    assert begin() == -1 and b'open tick' in L.fibhip_last_error()
    box = (C.c_int * 4)(2, 4, 3, 6)
    half = np.full(6, 0.5, np.float32)
    assert L.fibhip_lesion_apply(h, box, half.ctypes.data_as(fp)) == -1 and b'open tick' in L.fibhip_last_error()
    st.step_interior()
    st.step_commit()
    assert begin(handle=None) != 0 and L.fibhip_lesion_begin(h, 1, None, 1, None) != 0
    assert L.fibhip_lesion_apply(h, None, None) != 0 and L.fibhip_get_phase(h, None) != 0
    assert L.fibhip_lesion_apply(h, (C.c_int * 4)(2, 2, 3, 6), half.ctypes.data_as(fp)) == -1 and b'is empty or outside' in L.fibhip_last_error()
    assert L.fibhip_lesion_apply(h, box, np.full(6, 2.0, np.float32).ctypes.data_as(fp)) == -1 and b'in [0, 1]' in L.fibhip_last_error()
    # a field below the floor somewhere: the identity with the whole-plane update would not hold
    low = ref.hole_field()
    low[5, 7] = 0.0
    st.set_phase(low)
    assert begin() == -1 and b'row 5, column 7' in L.fibhip_last_error()
    assert L.fibhip_lesion_apply(h, box, half.ctypes.data_as(fp)) == -1 and b'>= 1e-5 everywhere' in L.fibhip_last_error()
    st.set_phase(ref.hole_field())
    assert begin(entries=[dict(offset=0, tick=i % 7, r0=2, r1=4, c0=3, c1=6) for i in range(256)]) == 0     # 256 entries fit
    st.step(8)
    assert st.lesion_count() == 256
    with pytest.raises(ValueError, match='a patch of shape'):
        st.lesion_apply((0, 2, 0, 2), np.ones((3, 3)))
    st.close()                                                        # destroyed with a program attached
    with pytest.raises(gpu_lib.FibhipError, match='null handle'):
        st.get_phase()
    # a handle without a field has nothing to read until a lesion gives it one
    bare = gpu_lib.Stepper(gpu_lib.FENTON4V, 32, 32, 0.1, 1.0, flags=gpu_lib.FAST)
    with pytest.raises(gpu_lib.FibhipError, match='no phase field'):
        bare.get_phase()
    bare.lesion_apply((1, 3, 1, 3), np.full((2, 2), 0.5, np.float32))
    want = np.ones((32, 32), np.float32)
    want[1:3, 1:3] = 0.5
    assert bare.get_phase().tobytes() == want.tobytes()
    bare.close()
    # the program object
    from fib_tf_amd.lesions import Lesion
    m2 = make('fenton')
    prog = m2.program_lesions([Lesion(('disc', 30, 12, 4), at_tick=0)])
    with pytest.raises(gpu_lib.FibhipError, match='attached already'):
        m2.program_lesions([Lesion(('disc', 30, 12, 4), at_tick=0)])
    prog.end()
    prog.close()
    with pytest.raises(AssertionError, match='closed'):
        prog.applied()
    m2._stepper.close()


def test_row_block_and_zero_padded_model_refused(gpu_lib):
    import ctypes as C
    arr = (gpu_lib.LesionEntry * 1)()
    arr[0].r1 = arr[0].c1 = 2
    p = np.full(4, 0.5, np.float32)
    fp = p.ctypes.data_as(C.POINTER(C.c_float))
    box = (C.c_int * 4)(0, 2, 0, 2)
    blk = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    assert blk._L.fibhip_lesion_begin(blk._h, 1, arr, 4, fp) == -1 and b'row block' in blk._L.fibhip_last_error()
    assert blk._L.fibhip_lesion_apply(blk._h, box, fp) == -1 and b'row block' in blk._L.fibhip_last_error()
    blk.close()
    zp = gpu_lib.Stepper(gpu_lib.FENTON4V, 40, 40, 0.1, 1.0, flags=gpu_lib.FAST | gpu_lib.ZEROPAD)
    assert zp._L.fibhip_lesion_begin(zp._h, 1, arr, 4, fp) == -1 and b'zero-padded' in zp._L.fibhip_last_error()
    assert zp._L.fibhip_lesion_apply(zp._h, box, fp) == -1 and b'zero-padded' in zp._L.fibhip_last_error()
    zp.close()


def test_example_and_bench_tool_run(gpu_lib, tmp_path, capsys, monkeypatch):
    """examples/run_ablation.py and tools/bench_lesions.py end to end at a toy size (in this process: what is checked is that they
    run and that what they print rests on what happened)"""
    import importlib.util
    import json
    set_env(monkeypatch, {})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    ex = load('examples/run_ablation.py', 'run_ablation_under_test')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = ex.main(['--size', '96', '--s2-ms', '30', '--ablate-ms', '50', '--ms', '80', '--every', '5', '--dwell-ms', '1', '--no-plot'])
    out = capsys.readouterr().out
    assert res['applied'] == len(res['path']) >= 2 and 'lesions applied' in out
    assert len(res['tip_counts']) == len(res['wave_counts']) == 16
    assert res['phase'].shape == (96, 96) and res['phase'].min() < 0.5 and res['frame'].shape == (96, 96)
    bench = load('tools/bench_lesions.py', 'bench_lesions_under_test')
    path = tmp_path / 'lesion_cost.txt'
    r = bench.main(['--size', '96', '--ticks', '80', '--lesions', '4', '--repeats', '2', '--out', str(path)])
    text = path.read_text()
    assert json.loads(text.splitlines()[-1]) == r
    assert r['cells'] == 96 * 96 and r['lesions'] == 4 and r['applied'] == 4
    for k in ('program_ms', 'none_ms', 'host_route_ms', 'event_us', 'host_route_per_lesion_ms'):
        assert r[k] > 0, (k, r)
    assert r['extra_tick_launches'] >= 0 and r['program_mt_launches'] >= r['none_mt_launches'] and r['none_mt_launches'] > 0
