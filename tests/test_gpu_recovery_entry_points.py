"""-m gpu: every entry point that can stand behind a multi-tick launch that has not been confirmed (csrc/sched.inc, the rule
above confirm()): a launch that gave up leaves the state it started from intact only as long as nothing but another multi-tick
launch follows it, so whatever writes the state — or hands out where it lives — has to find out first.

tests/test_gpu_recovery.py covers step, get_state, probe, pace, set_state, set_phase, sync and expect on Fenton and
Beeler-Reuter handles.  Here: step_mode on a traced model, trace_tick, the raw pointer of fibhip_state_ptr, the read-back into
pageable memory, the two recorders, the counters of fibhip_launch_stats, short cycles of launch ids, and traced handles.

The yardstick is the same: the library's own one-launch-per-tick mode (FIBHIP_MT=0), bit for bit.  The give-up is the test
switch FIBHIP_MT_FAKE_GIVEUP=n (the n-th multi-tick launch finds the give-up word raised and leaves at its first boundary):
nothing waits out a bound, nothing hangs.  Every test proves that it reached the path it names:
  * the untouched run equals the FIBHIP_MT=0 run and reports no fallback;
  * the faked run reports exactly one;
  * that count is still 0 immediately before the call under test ('mark:before' — fibhip_fallbacks and fibhip_launch_stats
    read the handle's counters and synchronise nothing), so the give-up is found inside or behind that call;
  * n runs over every launch that stands unconfirmed in front of the call (counted in the untouched run).
Each is run with FIBHIP_AHEAD=0, where the launches are the caller's own, and with the default."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_recovery import SCRIPT, _hip, _state  # noqa: E402
from test_gpu_recovery import _play as _play_script  # noqa: E402
from traced_cases import MODELS, make_model  # noqa: E402

pytestmark = pytest.mark.gpu

ENV = ('FIBHIP_MT', 'FIBHIP_MT_FAKE_GIVEUP', 'FIBHIP_AHEAD', 'FIBHIP_MT_WAIT_MS', 'FIBHIP_MT_IDS', 'FIBHIP_MT_MAX', 'FIBHIP_VARIANT',
       'FIBHIP_AUTOTUNE')
# the forced small shapes of tests/test_gpu_recovery.py and tests/test_gpu_traced.py
SHAPES = {'fenton': (96, 100, '10,44,25,-3'), 'br': (70, 130, '5,54,21,-2')}
TRACED_SHAPE = (96, 130, (40, 50, 9))
PACE = {'fenton': (1.0, 0.0), 'br': (10.0, -90.0)}
AHEAD = [pytest.param(False, id='ahead0'), pytest.param(True, id='ahead')]
EL_RECTS = [(10, 30, 20, 50), (0, 64, 0, 90)]


@pytest.fixture(autouse=True)
def _restore_modules():
    saved = {k: sys.modules.get(k) for k in ('tensorflow', 'ionic', 'screen')}
    yield
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def _traced_model(name, policy):
    """one of tests/models/* at the traced shape.  The multirate model has one assign group of its own (the tick); a second
    one — the recovery variable advanced without the stencil, in the style of the reference's 'slow' ops — is registered
    here, so that the model has a mode for fibhip_step_mode AND keeps its tick-fusing strip (four sub-steps per tick)"""
    H, W, hole = TRACED_SHAPE
    m = make_model(name, H, W, hole, fast_math=(policy == 'fast'))
    m.define()
    if name == 'mrfhn':
        import fib_tf_amd.tfgraph as tf
        v, w = (a.ref for a in m._ode_op.assigns)
        assert (v.name, w.name) == ('v', 'w')
        m._ops['wslow'] = tf.group(tf.assign(w, w + 0.4 * (0.08 * (v + 0.7 - 0.8 * w))))
    m._ensure_compiled()
    return m


class _Handle:
    """a stepper of one of the kinds 'fenton', 'br', '<traced model>:<policy>' at its forced shape, in a known state"""

    def __init__(self, lib, kind, ext):
        self.lib, self.kind, self.slabs, self.mode = lib, kind, [], None
        if kind in SHAPES:
            H, W, _ = SHAPES[kind]
            nvar = 4 if kind == 'fenton' else 8
            init, phi = _state(H, W, 11 * H + W, nvar)
            if kind == 'br':
                init[0] = init[0] * 100.0 - 85.0
                init[1] *= 1e-5
                init[2:] = init[2:] * 0.98 + 0.01
            kw = {}
            if ext:                                       # caller-owned slabs (fibhip_desc.ext_slab)
                hip = _hip()
                for _ in range(2):
                    p = C.c_void_p()
                    assert hip.hipMalloc(C.byref(p), nvar * H * W * 4) == 0
                    assert hip.hipMemset(p, 0, nvar * H * W * 4) == 0
                    self.slabs.append(p)
                kw['ext_slabs'] = (self.slabs[0].value, self.slabs[1].value)
            st = lib.Stepper(lib.FENTON4V if kind == 'fenton' else lib.BR, H, W, 0.1, 1.3 if kind == 'fenton' else 0.809,
                             flags=lib.FAST, **kw)
            st.set_phase(phi)
            st.set_state(-1, init)
            self.pace_v = PACE[kind]
        else:
            name, policy = kind.split(':')
            m = _traced_model(name, policy)
            st = m._stepper
            if name == 'mrfhn':
                self.mode = m._modes[id(m._ops['wslow'])][0]
                assert self.mode >= 1
            self.pace_v = (MODELS[name][5], float(m.min_v))
            H, W = m.height, m.width
            # (the S1 columns of the model's own initial state + a stimulus: a wave is on its way from the first tick)
            st.pace(H // 2, H // 2 + 9, W // 2, W // 2 + 9, *self.pace_v)
            st.sync()
        self.st, self.H, self.W = st, H, W

    def close(self):
        self.st.close()
        for p in self.slabs:
            _hip().hipFree(p)


class _Run:
    def __init__(self):
        self.obs, self.marks, self.traces = [], {}, []


def _snapshot(st):
    s = st.launch_stats()
    return {'fb': st.fallbacks(), 'mt_launches': s['mt_launches'], 'launches': s['launches'], 'ticks': s['ticks']}


def _play(lib, monkeypatch, kind, script, env, reference=False, ext=False):
    """runs `script` on a fresh handle under `env`.  ints: step(n); ('x', n): n single-tick calls; ('rep', k, n): n calls of
    step(k); 'get' / ('get', v) / 'all' / 'sync' / 'pace' / ('expect', n) / ('probe', v, r, c) / ('scale', v) / ('phase', on):
    as in tests/test_gpu_recovery.py; ('mode', 0): fibhip_step_mode with the model's own extra mode; 'trace': trace_tick();
    'ptr_read' / ('ptr_write', row): through the raw pointer of fibhip_state_ptr; 'pageable': fibhip_get_state_direct into
    pageable memory; 'obs_begin', 'obs_maps', ('el_begin', every), 'el_read': the recorders; 'mark:<name>': the counters, read
    without synchronising.  `reference`: the control — what goes through the raw pointer elsewhere goes through get_state /
    set_state here."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if kind in SHAPES:
        monkeypatch.setenv('FIBHIP_VARIANT', SHAPES[kind][2])
    else:
        monkeypatch.setenv('FIBHIP_AUTOTUNE', '0')          # the generated header's own plan: the tick-fusing strip
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = _Handle(lib, kind, ext)
    st, H, W = h.st, h.H, h.W
    hip = _hip()
    patch = np.full((W,), 0.75 * h.pace_v[0], np.float32)
    rng = np.random.default_rng(5)
    el_patches = [rng.uniform(-1, 1, (r1 - r0, c1 - c0)).astype(np.float32) for r0, r1, c0, c1 in EL_RECTS]
    out = _Run()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for op in script:
            name = op if isinstance(op, str) else (None if isinstance(op, int) else op[0])
            if isinstance(op, int):
                st.step(op)
            elif name == 'x':
                for _ in range(op[1]):
                    st.step(1)
            elif name == 'rep':
                for _ in range(op[2]):
                    st.step(op[1])
            elif name == 'get':
                out.obs.append(st.get_state(0 if isinstance(op, str) else op[1]).copy())
            elif name == 'all':
                out.obs.append(st.get_state(-1))
            elif name == 'sync':
                st.sync()
            elif name == 'pace':
                st.pace(H // 4, H // 4 + 5, W // 3, W // 3 + 6, *h.pace_v)
            elif name == 'expect':
                st.expect(op[1])
            elif name == 'probe':
                out.obs.append(np.float32(st.probe(op[1], op[2], op[3])))
            elif name == 'scale':
                st.set_state(op[1], (st.get_state(op[1]) * np.float32(0.999)).astype(np.float32))
            elif name == 'phase':
                st.set_phase(_state(H, W, 11 * H + W)[1] if op[1] else None)
            elif name == 'mode':
                st.step_mode(h.mode)
            elif name == 'trace':
                out.traces.append([(e['name'], e['ticks']) for e in st.trace_tick()])
            elif name == 'ptr_read':
                if reference:
                    out.obs.append(st.get_state(0).copy())
                else:
                    _, ptr = st.state_buf(0)
                    st.sync()                               # (the pointer is the caller's: so is waiting for the handle's stream)
                    frame = np.empty((H, W), np.float32)
                    assert hip.hipMemcpy(frame.ctypes.data, ptr, H * W * 4, 2) == 0
                    out.obs.append(frame)
            elif name == 'ptr_write':
                if reference:
                    u = st.get_state(0).copy()
                    u[op[1]] = patch
                    st.set_state(0, u)
                else:
                    _, ptr = st.state_buf(0)
                    st.sync()
                    assert hip.hipMemcpy(ptr + op[1] * W * 4, patch.ctypes.data, W * 4, 1) == 0
            elif name == 'pageable':
                frame = np.empty((H, W), np.float32)        # (not from fibhip_host_alloc: the device cannot write it)
                st._ck(st._L.fibhip_get_state_direct(st._h, 0, frame.ctypes.data_as(C.POINTER(C.c_float))))
                out.obs.append(frame)
            elif name == 'obs_begin':
                lo, hi = h.pace_v[1], h.pace_v[0]
                st.observe_begin(0, lo + 0.5 * (hi - lo), lo + 0.1 * (hi - lo))
            elif name == 'obs_maps':
                out.obs.extend(st.observe_get(which) for which in lib.OBS_MAPS)
                out.obs.append(np.int64(st.observe_ticks()))
            elif name == 'el_begin':
                st.electrode_begin(0, EL_RECTS, el_patches, op[1], 64)
            elif name == 'el_read':
                out.obs.append(np.int64(st.electrode_count()))
                out.obs.append(st.electrode_read())
            elif name.startswith('mark:'):
                out.marks[name[5:]] = _snapshot(st)
            else:
                raise AssertionError('unknown op %r' % (op,))
        out.obs.append(st.get_state(-1))
    out.stats, out.fb, out.tpl, out.plan = st.launch_stats(), st.fallbacks(), st.ticks_per_launch(), st.launch_plan()
    out.warned = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    h.close()
    return out


def _same(got, want, what):
    assert len(got.obs) == len(want.obs) and len(got.traces) == len(want.traces)
    for i, (x, y) in enumerate(zip(got.obs, want.obs)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i, x.shape, y.shape)
        # (the NaN cells of the activation maps: 'never crossed' — equal_nan keeps the comparison bitwise in every other cell)
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == 'f' and x.ndim == 2 and bool(np.isnan(y).any())), \
            '%s: observation %d differs from the one-launch-per-tick run (%d of %d values)' % (what, i, int((x != y).sum()), x.size)
    assert got.traces == want.traces, (what, got.traces, want.traces)


def _counters(got, want, what):
    """fibhip_launch_stats across a recovery: the ticks the handle advanced are the caller's ticks, whichever way they ran"""
    assert got.stats['ticks'] == want.stats['ticks'], (what, got.stats, want.stats)
    assert 0 <= got.stats['mt_ticks'] <= got.stats['ticks'] and got.stats['mt_launches'] >= 0, (what, got.stats)
    assert got.stats['ticks_recomputed_after_give_up'] == got.fb[1] and got.stats['gave_up_recovered'] == got.fb[0], (what, got.stats)


def _thin(cand, most=12):
    if len(cand) <= most:
        return cand
    return sorted({cand[int(round(i * (len(cand) - 1) / (most - 1.0)))] for i in range(most)})


def _behind_a_give_up(lib, monkeypatch, kind, script, ahead, ext=False, env=None, window=None, nths=None, need_strip=False):
    """the three runs of one scenario and their proofs.  `script` holds 'mark:before' in front of the call under test and
    'mark:after' behind it; every multi-tick launch up to 'mark:after' is unconfirmed there (no scenario synchronises before
    its call under test), so n runs over all of them: 1 .. mt_launches at 'mark:after' of the untouched run, or what
    `window(before, after)` says the call itself started on top of those before it."""
    base = dict(env or {})
    if not ahead:
        base['FIBHIP_AHEAD'] = '0'
    want = _play(lib, monkeypatch, kind, script, dict(base, FIBHIP_MT='0'), reference=True)
    free = _play(lib, monkeypatch, kind, script, base, ext=ext)
    if need_strip:
        # a traced model runs several ticks per launch only on the tick-fusing strip of its generated header (the condition of
        # test_generated_kernels_run_several_ticks_per_launch)
        if not (free.plan[1] == 1 and free.plan[0] > 1):
            pytest.skip('the plan of this traced model is not the tick-fusing strip: %r' % (free.plan,))
        assert free.tpl > 1, 'the multi-tick form of the generated strip kernel was not used (plan %r)' % (free.plan,)
    assert want.fb == (0, 0) and not want.warned and want.stats['mt_launches'] == 0
    assert free.fb == (0, 0) and not free.warned and free.stats['mt_launches'] >= 1, free.stats
    _same(free, want, 'untouched')
    _counters(free, want, 'untouched')
    before, after = free.marks['before'], free.marks['after']
    hi = window(before, after) if window else after['mt_launches']
    if nths is None:
        assert hi >= 1, 'no multi-tick launch stands in front of the call under test: %r' % (free.marks,)
        nths = _thin(list(range(1, hi + 1)))
    for nth in nths:
        what = '%s, launch %d of %d gave up' % (kind, nth, hi)
        got = _play(lib, monkeypatch, kind, script, dict(base, FIBHIP_MT_FAKE_GIVEUP=str(nth)), ext=ext)
        assert got.marks['before']['fb'] == (0, 0), (what, 'found before the call under test', got.marks)
        assert got.fb[0] == 1, (what, got.fb)
        assert got.tpl == 1 and len(got.warned) <= 1
        _same(got, want, what)
        _counters(got, want, what)
    return want, free


# ---- fibhip_step_mode on a traced model -------------------------------------------------------------------------------------
@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('policy', ['exact', 'fast'])
def test_step_mode_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, policy, ahead):
    """single-tick calls send launches of 1 (plain), 2, 4 and 8 ticks out; then the model's second assign group, in place on the
    current slab, with no observation in between.  Behind a launch that gave up the current slab is void and the recovery
    replays ticks only: the update has to wait until the launches in front of it are confirmed, or it is lost."""
    script = [('x', 15), 'mark:before', ('mode', 0), 'mark:after', ('x', 5), ('mode', 0), 3, 'get']
    _, free = _behind_a_give_up(gpu_lib, monkeypatch, 'mrfhn:' + policy, script, ahead, need_strip=True)
    assert free.marks['before']['mt_launches'] == 3 and free.marks['before']['ticks'] == 15, free.marks


# ---- trace_tick / the timeline of run() -------------------------------------------------------------------------------------
@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('kind', ['fenton', 'br', 'ap:fast'])
def test_trace_tick_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, kind, ahead):
    """while a timeline is taken every tick is a plain launch, which writes the slab the launches in front of it read: it must
    not be queued behind one of them that gave up.  The events still list the launches of one plain tick per traced tick."""
    script = [40, 'mark:before', 'trace', 'mark:after', 'trace', 'trace', 7, 'trace', 'get']
    want, free = _behind_a_give_up(gpu_lib, monkeypatch, kind, script, ahead, need_strip=kind not in SHAPES)
    assert free.marks['before']['mt_launches'] == 2, free.marks            # 32 + 8 ticks
    fused, per_tick = want.plan
    for ev in want.traces:
        assert len(ev) == per_tick and all(t == 1 and '<K=%d,' % fused in n and 'several ticks' not in n for n, t in ev), ev


@pytest.mark.parametrize('ahead', AHEAD)
def test_timeline_of_run_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, tmp_path, ahead):
    """IonicModel.run() with config['timeline'] (the key of test_timeline_and_save_graph_keys): the traced tick follows the
    loop's own ticks.  run() synchronises in between (ionic.py: st.sync() before the timeline), which is where a give-up of
    the loop's launches is found; the traced tick and the final state are those of the one-launch-per-tick run."""
    import json
    from fib_tf_amd.fenton import Fenton4v
    name = str(tmp_path / 'timeline.json')

    def run(env):
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv('FIBHIP_VARIANT', SHAPES['fenton'][2])
        if not ahead:
            monkeypatch.setenv('FIBHIP_AHEAD', '0')
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = Fenton4v({'width': 100, 'height': 96, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 12.05, 'skip': False,
                      'cheby': True, 'timeline': True, 'timeline_name': name})
        m.add_hole_to_phase_field(50, 48, 9)
        m.define()
        with warnings.catch_warnings(record=True):
            warnings.simplefilter('always')
            for _ in m.run():
                pass
            events = [(e['name'], e['args']['ticks']) for e in json.load(open(name))['traceEvents']]
            final = m._stepper.get_state(-1)
        st = m._stepper
        res = events, final, st.launch_stats(), st.fallbacks(), st.launch_plan()
        st.close()
        return res

    ev0, x0, s0, fb0, plan = run({'FIBHIP_MT': '0'})
    ev1, x1, s1, fb1, _ = run({})
    assert fb0 == (0, 0) and fb1 == (0, 0) and s1['mt_launches'] >= 1 and s0['ticks'] == s1['ticks'] == 13
    assert len(ev0) == plan[1] and all(t == 1 for _, t in ev0) and ev1 == ev0 and np.array_equal(x1, x0)
    for nth in range(1, s1['mt_launches'] + 1):
        ev, x, s, fb, _ = run({'FIBHIP_MT_FAKE_GIVEUP': str(nth)})
        assert fb[0] == 1 and ev == ev0, (nth, fb, ev)
        assert np.array_equal(x, x0), 'launch %d of %d gave up: the state behind the timeline differs' % (nth, s1['mt_launches'])
        assert s['ticks'] == 13 and s['mt_ticks'] <= s['ticks'] and s['ticks_recomputed_after_give_up'] == fb[1], s


# ---- the raw pointer of fibhip_state_ptr ------------------------------------------------------------------------------------
@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('ext', [False, True], ids=['own_slabs', 'ext_slabs'])
@pytest.mark.parametrize('ticks', [40, 41])
def test_state_ptr_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, ticks, ext, ahead):
    """the pointer names the slab the state is in.  A recovery moves the state (back to the slab the failed launch started
    from, then on by the replayed ticks): it has to happen before the pointer is handed out, or the caller reads a void slab
    and its writes go where no tick will read them.  What is read through the pointer equals the one-launch-per-tick frame,
    and a row written through it counts like the same row written with set_state (the control), on library-owned and on
    caller-owned slabs.  (40 and 41 ticks: an even number of replayed ticks can end in the very slab the stale pointer names.)"""
    script = [ticks, 'mark:before', 'ptr_read', 'mark:after', ('ptr_write', 40), 25, 'get', ('ptr_write', 41), ('x', 6), 'ptr_read']
    _, free = _behind_a_give_up(gpu_lib, monkeypatch, 'fenton', script, ahead, ext=ext)
    assert free.marks['before']['mt_launches'] == 2, free.marks


# ---- fibhip_get_state_direct into pageable memory ---------------------------------------------------------------------------
def _launched_by_the_call(before, after):
    # (a launch that runs ahead is not among the multi-tick launches the handle counts until its ticks are handed out; it is
    # among the launches)
    return before['mt_launches'] + (after['launches'] - before['launches'])


def test_pageable_read_back_behind_a_launch_that_gave_up(gpu_lib, monkeypatch):
    """a destination the device cannot write: the copy goes first on the stream, the next series is launched right behind it
    and the event between the two is waited for.  The copy reads the current slab — void if one of the launches in front of it
    gave up, and then the frame has to be taken again after the recovery.  The next series is declared (fibhip_expect), so the
    read-back launches it behind two launches (32 + 8 ticks) that nobody has confirmed; n = 1, 2: those, n = 3: its own."""
    script = [40, ('expect', 10), 'mark:before', 'pageable', 'mark:after', ('x', 10), 'pageable', ('x', 4), 'get']
    _, free = _behind_a_give_up(gpu_lib, monkeypatch, 'fenton', script, True, window=_launched_by_the_call)
    before, after = free.marks['before'], free.marks['after']
    assert before['mt_launches'] == 2 and after['launches'] == before['launches'] + 1, \
        'the read-back did not launch the next series: the pageable branch of ahead_read_back was not taken %r' % (free.marks,)
    # nothing runs ahead: the same calls take the plain copy (and its second pass)
    _behind_a_give_up(gpu_lib, monkeypatch, 'fenton', script, False)


def test_pageable_read_back_after_equal_series(gpu_lib, monkeypatch):
    """series of equal length, each ended by a read-back into pageable memory (a driver that keeps every frame): from the second
    frame on the read-back launches the next series.  n = 3 is the launch the last read-back in front of 'mark:before' started
    (its ticks have all been handed out since), n = 4 the one the read-back under test starts."""
    script = [10, 'pageable', 10, 'pageable', 10, 'mark:before', 'pageable', 'mark:after', 10, 'pageable', 7, 'get']
    want = _play(gpu_lib, monkeypatch, 'fenton', script, {'FIBHIP_MT': '0'}, reference=True)
    free = _play(gpu_lib, monkeypatch, 'fenton', script, {})
    before, after = free.marks['before'], free.marks['after']
    assert free.fb == (0, 0) and want.fb == (0, 0)
    assert before['mt_launches'] == 3 and after['launches'] == before['launches'] + 1 and after['mt_launches'] == 3, free.marks
    _same(free, want, 'untouched')
    _counters(free, want, 'untouched')
    for nth in (1, 2, 3, 4, 5):
        got = _play(gpu_lib, monkeypatch, 'fenton', script, {'FIBHIP_MT_FAKE_GIVEUP': str(nth)})
        what = 'launch %d gave up' % nth
        if nth == 4:                                      # (1, 2: found by an earlier frame's copy; 3: by the read-back that started it)
            assert got.marks['before']['fb'] == (0, 0), got.marks
        assert got.fb[0] == 1, (what, got.fb)
        _same(got, want, what)
        _counters(got, want, what)


# ---- the recorders ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('which', ['activation', 'electrodes', 'both'])
def test_recorders_attached_behind_a_launch_that_gave_up(gpu_lib, monkeypatch, which, ahead):
    """observe_begin copies the potential it compares the first tick with, electrode_begin defines tick 0 of its trace: both
    synchronise (and so recover) before they attach.  Maps and raw traces of the ticks that follow are those of the
    one-launch-per-tick run."""
    begin = {'activation': ['obs_begin'], 'electrodes': [('el_begin', 3)], 'both': ['obs_begin', ('el_begin', 3)]}[which]
    read = {'activation': ['obs_maps'], 'electrodes': ['el_read'], 'both': ['el_read', 'obs_maps']}[which]
    script = [40, 'mark:before'] + begin + ['mark:after', ('x', 14), 9] + read + ['get']
    _, free = _behind_a_give_up(gpu_lib, monkeypatch, 'fenton', script, ahead)
    assert free.marks['before']['mt_launches'] == 2, free.marks


@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('kind', ['fenton', 'br'])
@pytest.mark.parametrize('every', [1, 3, 10])
def test_electrode_recorder_meets_a_give_up_at_every_launch(gpu_lib, monkeypatch, every, kind, ahead):
    """the recorder attached from the start, 30 ticks one call each and nothing that synchronises before the trace is read: no
    launch spans a sample tick, so there are 30 / every multi-tick launches with a sample queued behind each — and none at all
    with a sample every tick (a launch of one tick is a plain one): there the faked run is left out and what is checked is that
    nothing can give up."""
    script = [('el_begin', every), ('x', 30), 'mark:before', 'el_read', 'mark:after', ('x', 2 * every), 'el_read']
    if every == 1:
        want = _play(gpu_lib, monkeypatch, kind, script, {'FIBHIP_MT': '0'}, reference=True)
        free = _play(gpu_lib, monkeypatch, kind, script, {} if ahead else {'FIBHIP_AHEAD': '0'})
        assert free.fb == (0, 0) and free.stats['mt_launches'] == 0 and free.stats['ticks'] == 32, free.stats
        _same(free, want, 'untouched')
        return
    _, free = _behind_a_give_up(gpu_lib, monkeypatch, kind, script, ahead)
    assert free.marks['before']['mt_launches'] == 30 // every, free.marks


# ---- the counters of fibhip_launch_stats ------------------------------------------------------------------------------------
@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('nth', [1, 3, 4, 6, 8, 11])
def test_counters_across_a_recovery(gpu_lib, monkeypatch, nth, ahead):
    """the call sequence of test_a_launch_that_gives_up_does_not_cost_the_run: the ticks a recovery replays were counted when
    their launches went out and must not be counted twice"""
    base = {} if ahead else {'FIBHIP_AHEAD': '0'}
    _, s0, fb0, _, _ = _play_script(gpu_lib, 96, 100, SCRIPT, SHAPES['fenton'][2], monkeypatch, dict(base, FIBHIP_MT='0'))
    _, s1, fb1, _, _ = _play_script(gpu_lib, 96, 100, SCRIPT, SHAPES['fenton'][2], monkeypatch, base)
    _, s, fb, _, _ = _play_script(gpu_lib, 96, 100, SCRIPT, SHAPES['fenton'][2], monkeypatch, dict(base, FIBHIP_MT_FAKE_GIVEUP=str(nth)))
    assert fb0 == (0, 0) and fb1 == (0, 0) and fb[0] == 1
    assert s0['ticks'] == s1['ticks'] == s['ticks'] == sum(op if isinstance(op, int) else op[1] for op in SCRIPT if isinstance(op, int) or op[0] == 'x'), (s0, s1, s)
    assert s0['mt_ticks'] == 0 and 0 < s1['mt_ticks'] <= s1['ticks'] and 0 <= s['mt_ticks'] <= s['ticks'], (s1, s)
    assert s['mt_ticks'] + fb[1] <= s['ticks'] and s['mt_launches'] <= s1['mt_launches'], (s, s1)
    assert s['ticks_recomputed_after_give_up'] == fb[1] and s['gave_up_recovered'] == 1


# ---- short cycles of launch ids ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ahead', AHEAD)
@pytest.mark.parametrize('ids,calls,nths', [(2, 6, [6]), (3, 8, [7, 8]), (16, 25, [17, 20, 25])])
def test_give_up_beyond_a_short_cycle_of_ids(gpu_lib, monkeypatch, ids, calls, nths, ahead):
    """FIBHIP_MT_IDS: the give-up word names a launch by its id, and the ids come round.  `calls` calls of four ticks, one launch
    each (FIBHIP_MT_MAX=4), and nothing that synchronises: more launches than the cycle has ids.  The launch that gives up
    shares its id with older ones that ended well — the recovery must go back to the state THAT launch started from.  (n is
    taken behind the last point at which a journal bounded by the cycle drains the stream: the give-up is still found by the
    read-back, not by the scheduler.)"""
    script = [('rep', 4, calls), 'mark:before', 'get', 'mark:after', ('rep', 4, 3), 'get']
    assert all(n > ids for n in nths)
    _, free = _behind_a_give_up(gpu_lib, monkeypatch, 'fenton', script, ahead, env={'FIBHIP_MT_IDS': str(ids), 'FIBHIP_MT_MAX': '4'},
                                nths=nths)
    assert free.marks['before']['mt_launches'] == calls and free.marks['before']['ticks'] == 4 * calls, free.marks


# ---- random call sequences, wider vocabulary --------------------------------------------------------------------------------
def _random_script(seed, kind, nvar, H, W):
    rng = np.random.default_rng(seed)
    ops = ['step1', 'step1', 'step1', 'step1', 'stepn', 'series', 'pace', 'probe', 'get1', 'getall', 'set1', 'sync', 'expect', 'phase',
           'trace', 'ptr_read', 'ptr_write', 'pageable', 'pageable']
    if kind not in SHAPES:
        ops += ['mode', 'mode']
    script = []
    for _ in range(120):
        op = rng.choice(ops)
        if op == 'step1':
            script.append(1)
        elif op == 'stepn':
            script.append(int(rng.integers(0, 70)))
        elif op == 'series':                               # the reference driver's pattern: n ticks, a frame, n ticks, a frame
            n = int(rng.integers(2, 12))
            frame = 'pageable' if rng.integers(0, 2) else 'get'
            script += [('x', n), frame] * 3
        elif op == 'probe':
            script.append(('probe', int(rng.integers(0, nvar)), int(rng.integers(0, H)), int(rng.integers(0, W))))
        elif op == 'get1':
            script.append(('get', int(rng.integers(0, nvar))))
        elif op == 'getall':
            script.append('all')
        elif op == 'set1':
            script.append(('scale', int(rng.integers(1, nvar))))
        elif op == 'expect':
            script.append(('expect', int(rng.integers(0, 40))))
        elif op == 'phase':
            script.append(('phase', bool(rng.integers(0, 2))))
        elif op == 'ptr_write':
            script.append(('ptr_write', int(rng.integers(0, H))))
        elif op == 'mode':
            script.append(('mode', 0))
        else:
            script.append(str(op))                         # pace, sync, trace, ptr_read, pageable
    return script


@pytest.mark.parametrize('seed', range(1, 1 + int(os.environ.get('FIBTF_STRESS_SEEDS', '8'))))      # (a few hundred: a stress run)
@pytest.mark.parametrize('kind', ['fenton', 'mrfhn:fast'])
def test_give_up_anywhere_in_random_call_sequences_wider(gpu_lib, monkeypatch, kind, seed):
    """the vocabulary of test_give_up_anywhere_in_random_call_sequences plus trace_tick, reads and writes through the raw
    pointer and read-backs into pageable memory — and, on the multirate traced model, its second assign group (step_mode)"""
    H, W, nvar = (SHAPES['fenton'][0], SHAPES['fenton'][1], 4) if kind == 'fenton' else (TRACED_SHAPE[0], TRACED_SHAPE[1], 2)
    script = _random_script(seed, kind, nvar, H, W)
    want = _play(gpu_lib, monkeypatch, kind, script, {'FIBHIP_MT': '0'}, reference=True)
    free = _play(gpu_lib, monkeypatch, kind, script, {})   # (also: how many multi-tick launches this sequence has)
    assert want.fb == (0, 0) and free.fb == (0, 0) and free.stats['mt_launches'] >= 3, free.stats
    _same(free, want, 'untouched')
    _counters(free, want, 'untouched')
    nth = 1 + (seed * 7 + int(os.environ.get('FIBTF_STRESS_SALT', '0'))) % max(1, int(free.stats['mt_launches']))
    got = _play(gpu_lib, monkeypatch, kind, script, {'FIBHIP_MT_FAKE_GIVEUP': str(nth)})
    what = 'launch %d of %d gave up' % (nth, free.stats['mt_launches'])
    assert got.fb[0] == 1, (what, got.fb)
    _same(got, want, what)
    _counters(got, want, what)
