"""-m gpu: the trigger program (include/fibhip.h fibhip_trig_*, fib_tf_amd/triggers.py) on the device.

No tolerance anywhere in this file: the log and the state of a handle with a program must equal, byte for byte, those of a twin
stepped tick by tick with get_state -> tests/trigger_ref.py (which applies through tests/stim_ref.py) -> set_state.

The program of the twin tests is a closed loop that makes its own edges, so that no case passes on a quiet run.  Sensor A is a
rectangle at rest, off the waves (the core of the site the rules stimulate).  Rule 0 paces it when nothing arrived for three samples (an ESCAPE detection; MAX, held for two
samples); the site is then above the level (a RISE, which rule 0 itself ignores: it is inside its blanking time, and which rule 1
detects); rule 1 answers with a train of three ADD pulses of -0.45 of the swing, six samples later, which takes the site below the
level again (a FALL, which rule 2 detects and marks on another array).  Rule 3 watches a disc (a mask site, need > 1) and adds a
plane.  The grids are the smallest that reach each path of sense_kernel and the gated apply: 37 x 53 and 20 x 130 (scalar), 64 x
64 (16-byte loads; the sensor's and the stimulus' box start and end at odd columns), the row-interleaved slab, 96 x 100 (several
tiles, multi-tick launches)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trigger_ref as ref  # noqa: E402
from test_gpu_frames import PACE_V, PLAN_ENV, VARIANT_96x100, wave  # noqa: E402
from test_gpu_tips import MAKERS, fenton  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLES, CHECKS = 48, (10, 24, 48)          # samples per case; the state is compared after these samples
C, A, T, N, CAUSE, FIRED = range(6)


def set_env(monkeypatch, env):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def loop_program(H, W, rest, v, nvar, mark_var=1, delay=6):
    """(sensors, rules, planes) as Stepper.trig_begin takes them: the closed loop of the module's docstring"""
    swing = v - rest
    # the stimulated site, and the sensor's: its core, four cells inside (what diffuses in from the tissue the paced site has
    # excited around it takes longer than a sample to get there).  64 x 64: columns 45 .. 57 and 49 .. 53, all odd
    site = dict(r0=H - 14, r1=H - 3, c0=W - 19, c1=W - 7)
    core = dict(r0=H - 10, r1=H - 7, c0=W - 15, c1=W - 11)
    assert W != 64 or all(b[k] % 2 == 1 for b in (site, core) for k in ('c0', 'c1'))
    rows, cols = np.arange(H)[:, None], np.arange(W)[None, :]
    disc = np.hypot(rows - (H // 3 + 3), cols - (W // 3 + 4)) <= 6.5
    rng = np.random.default_rng(H * 1000 + W)
    plane = np.zeros((H, W), np.float32)
    plane[1:H // 2, 3:W // 2] = rng.uniform(-1e-3, 1e-3, (H // 2 - 1, W // 2 - 3)).astype(np.float32) * np.float32(swing)
    sensors = [dict(var=0, level=rest + 0.5 * swing, need=1, site='rect', **core),
               dict(var=0, level=rest + 0.25 * swing, need=5, site='mask', mask=disc)]
    stim = dict(var=0, shape='rect', **site)
    rules = [dict(stim, sensor=0, edge='rise', escape=3, blank=40, hold=2, mode='max', v=v, floor=-np.inf),
             dict(stim, sensor=0, edge='rise', blank=20, delay=delay, count=3, period=2, mode='add', v=-0.45 * swing, floor=0.0),
             dict(sensor=0, edge='fall', blank=1, var=mark_var, mode='add', shape='rect', r0=2, r1=9, c0=3, c1=W - 2, v=0.0078125, floor=0.0),
             dict(sensor=1, edge='fall', blank=4, escape=16, hold=2, var=0, mode='add', shape='plane', plane=0)]
    return sensors, rules, [plane]


def shows_everything(log, rules):
    """the log holds a RISE detection, a FALL detection, an escape detection, an edge ignored inside `blank`, a train of more than
    one pulse and a hold > 1 — else the comparison would pass on a quiet run"""
    seen = set()
    for r, rule in enumerate(rules):
        rows = log[:, r]
        for s in range(len(rows)):
            pa, pt = (rows[s - 1, A], rows[s - 1, T]) if s else (-1, -1)
            rise, fall = pa == 0 and rows[s, A] == 1, pa == 1 and rows[s, A] == 0
            edge = rise if rule['edge'] == 'rise' else fall
            if rows[s, CAUSE] == 1:
                seen.add('rise' if rule['edge'] == 'rise' else 'fall')
            if rows[s, CAUSE] == 2:
                seen.add('escape')
            if edge and rows[s, CAUSE] == 0 and 0 <= pt and pt + 1 < rule.get('blank', 0):
                seen.add('ignored')
            if rows[s, FIRED] and s and rows[s - 1, FIRED] and rule.get('hold', 1) > 1:
                seen.add('hold')
        fired = np.flatnonzero(rows[:, FIRED])
        if rule.get('count', 1) > 1 and len(fired) > 1 and (np.diff(fired) == rule['period']).any():
            seen.add('train')
    return seen


EVERYTHING = {'rise', 'fall', 'escape', 'ignored', 'hold', 'train'}


def run_pair(make, program, every, calls, slow_every=0, samples=SAMPLES, checks=CHECKS):
    """the program on one handle against the twin.  `calls`: 'single' (one fibhip_step per tick) or 'chunks' (several ticks per
    call, cut where the caller does something else).  -> (log, launch stats of the program handle since attach)"""
    (a, slow_a), (b, slow_b) = make(), make()
    sensors, rules, planes = program
    H, W = a.height, a.width
    ticks = samples * every
    stops = sorted({c * every for c in checks} | ({t for t in range(1, ticks + 1) if (t - 1) % slow_every == 0} if slow_every else set()))
    a.trig_begin(sensors, rules, planes, every=every, capacity=samples)
    s0 = a.launch_stats()
    twin = ref.Program(sensors, rules, planes, H, W)
    pattern, done, got, want = (1, 3, 2, 5, 7, 11), 0, [], []
    i = 0
    while done < ticks:
        nxt = min(t for t in stops if t > done)
        n = 1 if calls == 'single' else min(pattern[i % len(pattern)], nxt - done)
        i += 1
        a.step(n)
        done += n
        if slow_every and (done - 1) % slow_every == 0:
            slow_a()
        if done in [c * every for c in checks]:
            got.append(a.get_state(-1))
    for k in range(ticks):
        b.step(1)
        if (k + 1) % every == 0:
            before = b.get_state(-1)
            after = twin.sample(before)
            if after.tobytes() != before.tobytes():
                b.set_state(-1, after)
        if slow_every and k % slow_every == 0:
            slow_b()
        if k + 1 in [c * every for c in checks]:
            want.append(b.get_state(-1))
    assert a.trig_count() == samples
    log = a.trig_read()
    s1 = a.launch_stats()
    assert log.shape == (samples, len(rules), 6) and log.dtype == np.int32
    expect = twin.log()
    assert log.tobytes() == expect.tobytes(), 'the log differs first at sample %d:\n%s\n%s' % (
        int(np.flatnonzero((log != expect).any(axis=(1, 2)))[0]), log[(log != expect).any(axis=(1, 2))][:3], expect[(log != expect).any(axis=(1, 2))][:3])
    for c, g, w in zip(checks, got, want):
        for v in range(g.shape[0]):
            assert g[v].tobytes() == w[v].tobytes(), 'after sample %d: array %d differs in %d cells' % (c, v, int((g[v] != w[v]).sum()))
    assert np.array_equal(a.trig_read(3, 5), log[3:8])
    a.trig_end()
    a.close()
    b.close()
    return log, {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}


def raw_maker(gpu_lib, H, W, layout):
    """a Fenton handle without a model around it (the small grids and the row-interleaved slab): rest, and a block above threshold"""
    flags = gpu_lib.FAST | (gpu_lib.ROW_INTERLEAVED if layout == 'interleaved' else 0)
    init = np.zeros((4, H, W), np.float32)
    init[1:3] = 1.0                                                                 # (Fenton's gates at rest)
    init[0, H // 3:H // 3 + 7, W // 3:W // 3 + 9] = 1.0

    def make():
        st = gpu_lib.Stepper(gpu_lib.FENTON4V, H, W, 0.1, 1.3, flags=flags)
        st.set_state(-1, init)
        return st, None
    return make


@pytest.mark.parametrize('calls', ['single', 'chunks'])
@pytest.mark.parametrize('mt', ['mt', 'mt0'])
@pytest.mark.parametrize('shape,layout', [((37, 53), 'planar'), ((20, 130), 'planar'), ((64, 64), 'planar'), ((37, 53), 'interleaved'),
                                          ((64, 64), 'interleaved')], ids=lambda a: a if isinstance(a, str) else '%dx%d' % a)
def test_small_grids_equal_the_twin(gpu_lib, monkeypatch, shape, layout, mt, calls):
    set_env(monkeypatch, {'FIBHIP_MT': '0'} if mt == 'mt0' else {})
    H, W = shape
    program = loop_program(H, W, 0.0, 1.0, 4)
    log, _ = run_pair(raw_maker(gpu_lib, H, W, layout), program, 1, calls)
    assert shows_everything(log, program[1]) == EVERYTHING, (shows_everything(log, program[1]), log[:20, :2, :3].tolist())


def model_maker(kind):
    def make():
        m = MAKERS[kind](96, 100)
        wave(m, kind)
        return m._stepper, (lambda: m.fire_op('slow'))
    return make


@pytest.mark.parametrize('calls', ['single', 'chunks'])
@pytest.mark.parametrize('mt', ['mt', 'mt0'])
@pytest.mark.parametrize('kind,plan', [('fenton', 'forced'), ('fenton', 'default'), ('br', 'default'), ('court', 'default'),
                                       ('traced', 'default')])
def test_models_equal_the_twin(gpu_lib, monkeypatch, kind, plan, mt, calls):
    """96 x 100: the forced 12-tile shape (a Fenton shape: multi-tick launches between the samples, every = 2) and the plan each
    model chooses itself.  Courtemanche runs on aggregates with the driver's 'slow' behind the ticks 0, 10, 20, ... and every = 1,
    so that 'slow' follows SAMPLE ticks — and with delay = 7 the first pulse of rule 1's train follows the sample of tick 10:
    the order on that tick is tick, sense / stimulus, slow, as the twin does it."""
    env = {'FIBHIP_VARIANT': VARIANT_96x100} if plan == 'forced' else {}
    if mt == 'mt0':
        env['FIBHIP_MT'] = '0'
    set_env(monkeypatch, env)
    m = MAKERS[kind](96, 100)
    rest, nvar = float(m.min_v), len(m.VAR_NAMES)
    m._stepper.close()
    every = 1 if kind == 'court' else 2
    program = loop_program(96, 100, rest, PACE_V[kind], nvar, delay=7 if kind == 'court' else 6)
    log, stats = run_pair(model_maker(kind), program, every, calls, slow_every=10 if kind == 'court' else 0)
    assert shows_everything(log, program[1]) == EVERYTHING, (shows_everything(log, program[1]), log[:20, :2, :3].tolist())
    if kind == 'court':
        assert log[10, 1, FIRED] == 1 and log[10, 1, T] == 7, log[:12, 1].tolist()       # a stimulus on a tick 'slow' follows
    assert stats['ticks'] == every * SAMPLES
    if mt == 'mt0':
        assert stats['mt_ticks'] == 0
    elif kind == 'fenton' and plan == 'forced':
        assert stats['mt_ticks'] > 0


def fenton_with(monkeypatch, env=None):
    set_env(monkeypatch, dict({'FIBHIP_VARIANT': VARIANT_96x100}, **(env or {})))
    m = fenton(96, 100)
    wave(m, 'fenton')
    return m


def loop_triggers(m, floor=None):
    """the loop's first two rules through the Python layer"""
    from fib_tf_amd.triggers import Sensor, Trigger
    site = 'right'                                                                  # rows 0 .. 96, columns 95 .. 100
    a = Sensor((40, 44, 96, 99), 0.5)
    return [Trigger(a, on='rise', escape=6, blank=80, max_detections=1, site=site, v=1.0, floor=floor),
            Trigger(a, on='rise', blank=40, delay=12, count=3, period=4, max_detections=1, site=site, v=-0.4, mode='add')]


def test_closed_loop_equals_the_open_loop_replay_of_its_own_log(gpu_lib, monkeypatch):
    """as_program() through program_stimuli on a fresh model leaves the same bytes; so does fire_op for the MAX rule floored at
    min_v, on the named site 'right' (the ADD rule's pulses come from the stimulus program beside it)"""
    m = fenton_with(monkeypatch)
    with m.trigger_stimuli(loop_triggers(m, floor='min_v'), every=2, capacity=30) as prog:
        m._stepper.step(60)
        want = m._stepper.get_state(-1).tobytes()
        fired, replay = prog.fired(), prog.as_program()
        assert prog.samples() == 30 and prog.detections() == [(5, 0, 'escape'), (7, 1, 'edge')]
    # (the escape at sample 2 = tick 5; the rise one sample later, its train 6, 8 and 10 samples after that)
    assert fired == [(5, 0, 'escape'), (19, 1, 'edge'), (23, 1, 'edge'), (27, 1, 'edge')], fired
    assert prog.log()['t_ms'][0, 0] == pytest.approx(2 * prog.tick_ms)
    m._stepper.close()
    m = fenton_with(monkeypatch)
    with m.program_stimuli(replay):
        m._stepper.step(60)
        assert m._stepper.get_state(-1).tobytes() == want
    m._stepper.close()
    m = fenton_with(monkeypatch)
    m.add_pace_op('trig', 'right', 1.0)
    with m.program_stimuli([s for s in replay if s.mode == 'add']):
        for i in range(60):
            m._stepper.step(1)
            if (i, 0) in [(t, r) for t, r, _ in fired]:
                m.fire_op('trig')
        assert m._stepper.get_state(-1).tobytes() == want
    m._stepper.close()


def test_an_idle_program_changes_nothing(gpu_lib, monkeypatch):
    """rules that never detect (the level is never reached) leave the bytes of a run without a program"""
    from fib_tf_amd.triggers import Sensor, Trigger
    m = fenton_with(monkeypatch)
    with m.trigger_stimuli([Trigger(Sensor('left', 5.0), site='luq', v=1.0), Trigger(Sensor((1, 90, 3, 99), 5.0, frac=0.5), on='fall', site='luq', v=0.5, mode='add')],
                           every=3, capacity=20) as prog:
        m._stepper.step(60)
        got = m._stepper.get_state(-1).tobytes()
        assert prog.detections() == [] and prog.fired() == [] and prog.rows()[:, :, A].max() == 0
    m._stepper.close()
    m = fenton_with(monkeypatch)
    m._stepper.step(60)
    assert m._stepper.get_state(-1).tobytes() == got
    m._stepper.close()


def test_sixty_four_single_tick_calls_are_eight_launches_and_three_per_sample(gpu_lib, monkeypatch):
    m = fenton_with(monkeypatch)
    st = m._stepper
    sensors, rules, planes = loop_program(96, 100, 0.0, 1.0, 4)
    st.trig_begin(sensors, rules, planes, every=8, capacity=8)
    s0 = st.launch_stats()
    for _ in range(64):
        st.step(1)
    st.sync()
    s1 = st.launch_stats()
    d = {k: s1[k] - s0[k] for k in ('launches', 'ticks', 'mt_launches', 'mt_ticks')}
    assert d['mt_launches'] == 8 and d['mt_ticks'] == 64 and d['ticks'] == 64 and 8 < d['launches'] <= 8 + 3 * 8, d
    assert st.trig_count() == 8
    st.close()


def test_beside_a_stimulus_program_and_recorders_the_sensor_sees_the_programmed_stimulus(gpu_lib, monkeypatch):
    """a shared tick: the statistics sample comes first (it does not see the programmed stimulus), then the programmed stimulus,
    then the sensor (it does), then the triggered stimulus (the next statistics sample sees it)"""
    from fib_tf_amd.stimulus import Stimulus
    from fib_tf_amd.triggers import Sensor, Trigger
    m = fenton_with(monkeypatch)
    st = m._stepper
    site = (96 - 12, 96 - 5, 100 - 15, 100 - 7)
    with m.record_activation(), m.record_stats([(m.VAR_NAMES[0], 'max')], every=4, weight=None, mask=np.pad(np.ones((7, 8), bool), ((84, 5), (85, 7)))) as stats, \
            m.program_stimuli([Stimulus(site, 0.75, at_tick=7, floor=None)]), \
            m.trigger_stimuli([Trigger(Sensor(site, 0.5, frac=1.0), on='rise', site=site, v=1.25, floor=None)], every=4, capacity=8) as prog:
        st.step(16)
        rows, col = prog.rows()[:, 0], stats.values()[:, 0]
    assert rows[:2, A].tolist() == [0, 1] and rows[:2, C].tolist() == [0, 56] and rows[:2, CAUSE].tolist() == [0, 1], rows
    assert rows[:2, FIRED].tolist() == [0, 1] and rows[-1, N] == 1, rows
    assert col[0] < 0.5 and col[1] < 0.5 and col[2] > 0.5, col       # the statistics sample of tick 7 precedes both stimuli of that tick
    st.close()


def test_refusals(gpu_lib, monkeypatch):
    set_env(monkeypatch, {})
    st = gpu_lib.Stepper(gpu_lib.FENTON4V, 37, 53, 0.1, 1.3, flags=gpu_lib.FAST)
    sensor = dict(var=0, level=0.5, need=1, site='rect', r0=1, r1=5, c0=1, c1=9)
    rule = dict(sensor=0, edge='rise', blank=1, var=0, mode='max', shape='rect', r0=1, r1=5, c0=1, c1=9, v=1.0, floor=0.0)
    bad = [([sensor], [dict(rule, blank=4, delay=2, count=2, period=2)], 'blank'),
           ([sensor] * 9, [rule], 'sensors'), ([sensor], [rule] * 9, 'rules'),
           ([dict(sensor, need=33)], [rule], 'need'), ([dict(sensor, level=float('nan'))], [rule], 'level'),
           ([sensor], [dict(rule, sensor=1)], 'sensor'), ([sensor], [dict(rule, hold=3, period=2, count=2, blank=9)], 'hold'),
           ([sensor], [dict(rule, period=0, count=2, blank=9)], 'count'), ([dict(sensor, c1=54)], [rule], 'grid')]
    for sensors, rules, word in bad:
        with pytest.raises(RuntimeError, match=word):
            st.trig_begin(sensors, rules)
    st.trig_begin([sensor], [rule], every=2, capacity=3)
    with pytest.raises(RuntimeError, match='attached already'):
        st.trig_begin([sensor], [rule])
    st.step(6)
    with pytest.raises(RuntimeError, match='trace full'):
        st.step(2)
    st.step(1)                                                                      # (a tick that reaches no sample is fine)
    assert st.trig_count() == 3 and st.trig_read().shape == (3, 1, 6)
    with pytest.raises(RuntimeError, match='samples'):
        st.trig_read(2, 2)
    st.trig_end()
    st.trig_end()                                                                   # (no program attached: nothing)
    st.close()
    shard = gpu_lib.Stepper(gpu_lib.FENTON4V, 42, 40, 0.1, 1.0, global_height=64, row_offset=0, ghost_bottom=10)
    with pytest.raises(RuntimeError, match='row block'):
        shard.trig_begin([sensor], [rule])
    shard.close()


def test_a_slow_array_is_refused_on_aggregates(gpu_lib, monkeypatch):
    set_env(monkeypatch, {})
    m = MAKERS['court'](96, 100)
    st = m._stepper
    sensor = dict(var=0, level=0.0, need=1, site='rect', r0=1, r1=5, c0=1, c1=9)
    rule = dict(sensor=0, edge='rise', blank=1, mode='add', shape='rect', r0=1, r1=5, c0=1, c1=9, v=0.001, floor=0.0)
    slow = [4]                                                                      # (the arrays 0 .. 3 are the fast ones)
    with pytest.raises(RuntimeError, match='slow arrays'):
        st.trig_begin([sensor], [dict(rule, var=slow[0])])
    st.trig_begin([dict(sensor, var=slow[0])], [dict(rule, var=0)])               # (SENSING a slow array is fine)
    st.trig_end()
    st.close()


@pytest.mark.parametrize('shape,vec', [((64, 64), True), ((37, 53), False), ((20, 130), False)], ids=lambda a: a if isinstance(a, bool) else '%dx%d' % a)
def test_the_path_the_kernels_take(gpu_lib, monkeypatch, shape, vec):
    """the timeline names the instantiation: 64 x 64 (planar) senses and applies with 16-byte accesses, the odd widths (and the
    rows of 20 x 130, which do not start 16-byte aligned... W = 130 is no multiple of 4) one cell per thread"""
    set_env(monkeypatch, {})
    H, W = shape
    st, _ = raw_maker(gpu_lib, H, W, 'planar')()
    sensors, rules, planes = loop_program(H, W, 0.0, 1.0, 4)
    st.trig_begin(sensors, rules, planes, every=1, capacity=8)
    st.trace_begin()
    st.step(3)
    names = [e['name'] for e in st.trace_end()]
    tag = '<true>' if vec else '<false>'
    assert names.count('sense_kernel' + tag) == 3 and names.count('stim_gated_kernel' + tag) == 3 and names.count('trigger_kernel') == 3, names
    st.close()
    st, _ = raw_maker(gpu_lib, H, W, 'interleaved')()
    st.trig_begin(sensors, rules, planes, every=1, capacity=8)
    st.trace_begin()
    st.step(2)
    names = [e['name'] for e in st.trace_end()]
    assert names.count('sense_kernel<false>') == 2 and names.count('stim_gated_kernel<false>') == 2, names     # (the row-interleaved slab: scalar)
    st.close()


def load(path, name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('model', ['fenton', 'br'])
def test_the_example_fires_its_s2_from_the_waveback(gpu_lib, monkeypatch, capsys, model):
    """examples/run_closed_loop.py at a tiny size, the same arguments for both models: no tick is tuned"""
    set_env(monkeypatch, {})
    fired, counts = load('examples/run_closed_loop.py', 'run_closed_loop').main(['--model', model, '--size', '64', '--ms', '600'])
    assert len(fired) == 1 and fired[0][1:] == (0, 'edge'), fired                  # ONE S2, from a FALL detection
    assert 100 < fired[0][0] < 6000 and 'S2 after tick' in capsys.readouterr().out


def test_the_bench_tool_runs(gpu_lib, monkeypatch, capsys):
    set_env(monkeypatch, {})
    lines = load('tools/bench_triggers.py', 'bench_triggers').main(['--ticks', '40', '--configs', 'fenton96'])
    assert len(lines) == 1 and set(lines[0]) == {'config', 'cells', 'ticks', 'none_us', 'idle_us', 'waveback_us', 'polling_us', 'electrode_us',
                                                 'none_again_us'}
    assert set(lines[0]['idle_us']) == {'1', '10'} and all(lines[0][k] > 0 for k in ('none_us', 'waveback_us', 'polling_us', 'electrode_us'))
