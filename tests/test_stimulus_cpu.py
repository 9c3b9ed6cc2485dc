"""not-gpu: the stimulus program's host side — the declarations and their binding, the NumPy restatement (tests/stim_ref.py)
against the definitions it stands for (np.fmax, a float32 addition, pace_kernel's expression), the event ticks, and what
fib_tf_amd/stimulus.py does without a device: site parsing, milliseconds to ticks, the protocol helpers, every refusal."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stim_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Model:
    """what stimulus.py asks of a model: the grid, min_v, the tick, pace_rect, the array names"""
    height, width, min_v, dt, dt_per_step = 96, 100, -85.0, 0.1, 10
    VAR_NAMES = ('V', 'u', 'w', 's')

    def pace_rect(self, loc):
        from fib_tf_amd.ionic import IonicModel
        return IonicModel.pace_rect(self, loc)

    def millisecond_to_step(self, t):
        from fib_tf_amd.ionic import IonicModel
        return IonicModel.millisecond_to_step(self, t)


def test_declarations_and_binding():
    from fib_tf_amd import _lib
    C = _lib.C
    src = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    for name in ('fibhip_stim_begin', 'fibhip_stim_count', 'fibhip_stim_end'):
        assert 'int %s(' % name in src
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is C.c_int
    assert len(_lib.SYMBOLS['fibhip_stim_begin'][0]) == 5
    body = re.search(r'typedef struct fibhip_stim_entry \{(.*?)\} fibhip_stim_entry;', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        parts = decl.strip().split(None, 1)
        if len(parts) == 2:
            fields += [(n.strip(), parts[0]) for n in parts[1].split(',')]
    assert [f[0] for f in fields] == [f[0] for f in _lib.StimEntry._fields_]
    assert [{'int': C.c_int, 'float': C.c_float}[t] for _, t in fields] == [f[1] for f in _lib.StimEntry._fields_]
    assert C.sizeof(_lib.StimEntry) == 4 * len(fields) == 56
    assert tuple(k.lower() for k in re.findall(r'FIBHIP_STIM_(MAX|ADD) = \d', src)) == _lib.STIM_MODES == ref.MODES
    assert [int(v) for v in re.findall(r'FIBHIP_STIM_(?:MAX|ADD) = (\d)', src)] == [0, 1]
    assert tuple(k.lower() for k in re.findall(r'FIBHIP_STIM_(RECT|PLANE) = \d', src)) == _lib.STIM_SHAPES
    assert '#define FIBHIP_MAX_STIM_ENTRIES %d' % _lib.MAX_STIM_ENTRIES in src and _lib.MAX_STIM_ENTRIES == 64
    assert '#define FIBHIP_MAX_STIM_PLANES %d' % _lib.MAX_STIM_PLANES in src and _lib.MAX_STIM_PLANES == 8
    assert '#define FIBHIP_ABI_VERSION 1' in src


@pytest.mark.parametrize('seed', range(3))
def test_restatement_against_its_definitions(seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(37, 53)) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
    s = (rng.normal(size=(37, 53)) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
    assert ref.apply(x, s, 'max').tobytes() == np.fmax(x, s).tobytes()
    assert ref.apply(x, s, 'add').tobytes() == (x + s).tobytes() and ref.apply(x, s, 'add').dtype == np.float32
    # one float32 addition rounded on its own: the float64 sum rounded once (exact in float64, so no double rounding)
    assert ref.apply(x, s, 'add').tobytes() == (x.astype(np.float64) + s.astype(np.float64)).astype(np.float32).tobytes()


def test_nan_and_untouched_cells():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    x = np.array([[nan, 1.0, -0.0, -inf, 2.0, nan]], np.float32)
    # MAX: a NaN in X gives way to S (fmaxf), a NaN in S to X; S = -inf leaves the cell's bits — the NaN stays a NaN
    s = np.array([[0.5, nan, -inf, -inf, 3.0, -inf]], np.float32)
    got = ref.apply(x, s, 'max')
    assert got.tobytes() == np.array([[0.5, 1.0, -0.0, -inf, 3.0, nan]], np.float32).tobytes()
    assert np.signbit(got[0, 2]) and got[0].view(np.uint32)[5] == x[0].view(np.uint32)[5]
    # ADD: S = +0 or -0 leaves the bits (a plain addition would turn -0 into +0), a NaN propagates
    s = np.array([[0.0, nan, 0.0, -0.0, 0.25, 1.0]], np.float32)
    got = ref.apply(x, s, 'add')
    assert np.isnan(got[0, 0]) and np.isnan(got[0, 1]) and np.signbit(got[0, 2]) and got[0, 2] == 0 and got[0, 3] == -inf
    assert got[0, 4] == np.float32(2.25) and np.isnan(got[0, 5])
    assert got[0].view(np.uint32)[0] == x[0].view(np.uint32)[0]
    assert (np.float32(-0.0) + np.float32(0.0)).view(np.uint32) != np.float32(-0.0).view(np.uint32)        # (why the rule is needed)
    # the box the host cuts: the cells that are not untouched
    p = np.full((9, 11), -np.inf, np.float32)
    assert ref.box(p, 'max') == (0, 0, 0, 0)
    p[2, 3] = 1.0
    p[7, 5] = np.nan
    assert ref.box(p, 'max') == (2, 8, 3, 6)
    q = np.zeros((9, 11), np.float32)
    q[4, 10] = -0.0
    assert ref.box(q, 'add') == (0, 0, 0, 0)
    q[8, 0] = 1e-30
    assert ref.box(q, 'add') == (8, 9, 0, 1)
    from fib_tf_amd import stimulus
    assert stimulus.plane_box(p, 'max') == (2, 8, 3, 6) and stimulus.plane_box(q, 'add') == (8, 9, 0, 1)


def test_rectangle_with_floor_min_v_is_pace_kernels_expression():
    """csrc/pointwise.inc: pot = fmaxf(pot, sv), sv = v inside the rectangle and min_v outside"""
    rng = np.random.default_rng(5)
    H, W, min_v, v = 20, 31, np.float32(-85.0), np.float32(10.0)
    pot = rng.uniform(-100, 40, (H, W)).astype(np.float32)
    pot[3, 4] = np.nan
    r0, r1, c0, c1 = 1, H // 2, 1, W // 2
    want = pot.copy()
    for y in range(H):
        for x in range(W):
            sv = v if (r0 <= y < r1 and c0 <= x < c1) else min_v
            want[y, x] = np.fmax(pot[y, x], sv)
    got = ref.apply(pot, ref.rect_plane(H, W, r0, r1, c0, c1, v, min_v), 'max')
    assert got.tobytes() == want.tobytes() and got[3, 4] == v and (got >= min_v).all()
    # floor = -inf: the outside keeps its bits
    got = ref.apply(pot, ref.rect_plane(H, W, r0, r1, c0, c1, v, -np.inf), 'max')
    outside = np.ones((H, W), bool)
    outside[r0:r1, c0:c1] = False
    assert got[outside].tobytes() == pot[outside].tobytes() and (got[~outside] >= v).all()


def test_event_ticks():
    from fib_tf_amd import stimulus
    train = {'first': 3, 'period': 7, 'count': 5, 'hold': 1}
    assert [k for k in range(60) if ref.due(train, k)] == [3, 10, 17, 24, 31]
    held = {'first': 2, 'period': 5, 'count': 2, 'hold': 3}
    assert [k for k in range(30) if ref.due(held, k)] == [2, 3, 4, 7, 8, 9]
    once = {'first': 4, 'period': 0, 'count': 1, 'hold': 2}
    assert [k for k in range(30) if ref.due(once, k)] == [4, 5]
    forever = {'first': 0, 'period': 4, 'count': 0, 'hold': 1}
    assert [k for k in range(1000) if ref.due(forever, k)] == list(range(0, 1000, 4))
    full = {'first': 1, 'period': 2, 'count': 3, 'hold': 2}     # hold == period: applied after every tick of the train
    assert [k for k in range(20) if ref.due(full, k)] == [1, 2, 3, 4, 5, 6]
    entries = [train, held, once, forever, full]
    ev = ref.events(entries, 12)
    assert ev == sorted(ev) and ev == stimulus.expand(entries, 12)
    assert [e for e in ev if e[0] == 3] == [(3, 0), (3, 1), (3, 4)] and [e for e in ev if e[0] == 4] == [(4, 1), (4, 2), (4, 3), (4, 4)]
    # the header's rule, literally: with k ticks since attach, after the tick that makes k + 1 == first + 1 + j * period + d
    for e in entries:
        want = set()
        for j in range(e['count'] if e['count'] else 300):
            for d in range(e['hold']):
                want.add(e['first'] + 1 + j * e['period'] + d - 1)
        assert {k for k in range(200) if ref.due(e, k)} == {k for k in want if k < 200}


def test_sites_and_times():
    from fib_tf_amd.stimulus import Stimulus, compile_program, s1_train, s1s2, burst
    m = Model()
    H, W = m.height, m.width
    for name in ('left', 'right', 'top', 'bottom', 'luq', 'llq', 'ruq', 'rlq'):
        kind, rect, v, floor = Stimulus(name, 1.5, at_tick=0).shape(m)
        assert kind == 'rect' and rect == m.pace_rect(name) and v == 1.5 and floor == -85.0
    assert Stimulus((3, 9, 4, 20), 2.0, at_tick=0, floor=None).shape(m) == ('rect', (3, 9, 4, 20), 2.0, -np.inf)
    assert Stimulus((3, 9, 4, 20), 2.0, at_tick=0, mode='add').shape(m) == ('rect', (3, 9, 4, 20), 2.0, 0.0)
    assert Stimulus('left', 2.0, at_tick=0, floor=-3).shape(m)[3] == -3.0
    kind, plane = Stimulus(('disc', 40, 37.5, 6), 1.0, at_tick=0, floor=None).shape(m)
    yy, xx = np.mgrid[0:H, 0:W]
    disc = np.hypot(yy - 40, xx - 37.5) <= 6
    assert kind == 'plane' and plane.dtype == np.float32 and np.array_equal(plane == 1.0, disc) and np.all(plane[~disc] == -np.inf)
    # (the centre lies between two columns: no cell is at distance 6 straight above it, |dy| <= 5; in its row |dx| <= 5.5)
    assert ref.box(plane, 'max') == (35, 46, 32, 44)
    mask = np.zeros((H, W), bool)
    mask[5:8, 11:13] = True
    kind, plane = Stimulus(mask, 0.25, at_tick=0, mode='add').shape(m)
    assert np.array_equal(plane, np.where(mask, np.float32(0.25), np.float32(0))) and ref.box(plane, 'add') == (5, 8, 11, 13)
    kind, plane = Stimulus(mask, 0.25, at_tick=0).shape(m)           # the default floor under 'max': min_v, like fire_op
    assert np.all(plane[~mask] == np.float32(-85.0))
    field = np.random.default_rng(0).normal(size=(H, W))
    kind, plane = Stimulus(field, at_tick=0, mode='add').shape(m)
    assert kind == 'plane' and plane.tobytes() == field.astype(np.float32).tobytes()
    # milliseconds: a tick is dt_per_step * dt = 1 ms here; millisecond_to_step truncates
    assert Stimulus('left', 1.0, at_ms=23.7, period_ms=7.2, count=5, hold_ms=2.5).timing(m) == (23, 7, 5, 2)
    assert Stimulus('left', 1.0, at_tick=23, period=7, count=0, hold=3).timing(m) == (23, 7, 0, 3)
    assert Stimulus('left', 1.0, at_ms=5, hold_ms=0.2).timing(m) == (5, 0, 1, 1)
    m2 = Model()
    m2.dt_per_step, m2.dt = 5, 0.05
    assert Stimulus('left', 1.0, at_ms=10, period_ms=300).timing(m2) == (40, 1200, 1, 1)
    assert Stimulus('left', 1.0, at_tick=0, var='w').var_index(m) == 2 and Stimulus('left', 1.0, at_tick=0, var=3).var_index(m) == 3
    # the protocols
    prog = s1_train('left', 1.0, period=7, n=5) + [Stimulus('luq', 1.0, at_tick=23)]
    entries, planes = compile_program(m, prog)
    assert planes == [] and [(e['first'], e['period'], e['count'], e['hold']) for e in entries] == [(0, 7, 5, 1), (23, 0, 1, 1)]
    assert ref.events(entries, 40) == [(0, 0), (7, 0), (14, 0), (21, 0), (23, 1), (28, 0)]
    entries, planes = compile_program(m, s1s2('left', 1.0, s1_ms=300, n_s1=4, s2_ms=190, s2_site=('disc', 40, 50, 8), floor=None))
    assert [(e['first'], e['period'], e['count']) for e in entries] == [(0, 300, 4), (1090, 0, 1)] and len(planes) == 1
    assert entries[0]['shape'] == 'rect' and entries[0]['floor'] == -np.inf and entries[1]['shape'] == 'plane' and entries[1]['plane'] == 0
    entries, _ = compile_program(m, burst('right', 1.0, start_ms=500, cycle_ms=10, n=20))
    assert [(e['first'], e['period'], e['count']) for e in entries] == [(500, 10, 20)]
    entries, _ = compile_program(m, s1_train('left', 1.0, period_ms=300, n=3, start_ms=50))
    assert [(e['first'], e['period'], e['count']) for e in entries] == [(50, 300, 3)]
    # equal planes are uploaded once
    entries, planes = compile_program(m, [Stimulus(mask, 1.0, at_tick=i, floor=None) for i in range(10)])
    assert len(planes) == 1 and {e['plane'] for e in entries} == {0}


def test_refused_arguments():
    from fib_tf_amd.stimulus import Stimulus, compile_program
    m = Model()
    ok = dict(at_tick=0)
    bad = [(lambda: Stimulus('left', 1.0), 'at_ms or at_tick'), (lambda: Stimulus('left', 1.0, at_ms=1, at_tick=1), 'at_ms or at_tick'),
           (lambda: Stimulus('left', 1.0, period_ms=3, period=3, **ok), 'period_ms or period'),
           (lambda: Stimulus('left', 1.0, hold_ms=3, hold=3, **ok), 'hold_ms or hold'),
           (lambda: Stimulus('left', 1.0, mode='mul', **ok), 'mode is one of'),
           (lambda: Stimulus('left', 1.0, at_tick=-1).timing(m), 'must be >= 0'),
           (lambda: Stimulus('left', 1.0, hold=0, **ok).timing(m), 'hold must be >= 1'),
           (lambda: Stimulus('left', 1.0, period=4, hold=5, **ok).timing(m), 'hold 5 > period 4'),
           (lambda: Stimulus('left', 1.0, count=3, **ok).timing(m), 'count must be 1'),
           (lambda: Stimulus('left', 1.0, count=0, **ok).timing(m), 'count must be 1'),
           (lambda: Stimulus('left', 1.0, period=-2, **ok).timing(m), 'must be >= 0'),
           (lambda: Stimulus('left', 1.0, period=3, count=-1, **ok).timing(m), 'must be >= 0'),
           (lambda: Stimulus('left', 1.0, period_ms=0.5, **ok).timing(m), 'less than one tick'),
           (lambda: Stimulus('middle', 1.0, **ok).shape(m), 'unknown pacing site'),
           (lambda: Stimulus((5, 5, 0, 3), 1.0, **ok).shape(m), 'empty or outside'),
           (lambda: Stimulus((0, 97, 0, 3), 1.0, **ok).shape(m), 'empty or outside'),
           (lambda: Stimulus((0, 9, -1, 3), 1.0, **ok).shape(m), 'empty or outside'),
           (lambda: Stimulus('left', **ok).shape(m), 'finite number'), (lambda: Stimulus('left', float('inf'), **ok).shape(m), 'finite number'),
           (lambda: Stimulus(np.ones((96, 100), bool), float('nan'), **ok).shape(m), 'finite number'),
           (lambda: Stimulus('left', 1.0, floor='max_v', **ok).shape(m), "floor is 'min_v'"),
           (lambda: Stimulus(('disc', 300, 300, 2), 1.0, **ok).shape(m), 'holds no cell'),
           (lambda: Stimulus(np.ones((3, 3)), **ok).shape(m), 'a site of shape'),
           (lambda: Stimulus(np.ones((96, 100)), 1.0, **ok).shape(m), 'v must not be given'),
           (lambda: Stimulus('left', 1.0, var='nope', **ok).var_index(m), 'unknown array'),
           (lambda: Stimulus('left', 1.0, var=4, **ok).var_index(m), 'outside 0 .. 3'),
           (lambda: compile_program(m, []), '1 .. 64 entries'),
           (lambda: compile_program(m, [Stimulus('left', 1.0, **ok)] * 65), '1 .. 64 entries'),
           (lambda: compile_program(m, ['left']), 'not a Stimulus'),
           (lambda: compile_program(m, [Stimulus(np.full((96, 100), float(i)), mode='add', **ok) for i in range(1, 10)]), 'more than 8 different planes')]
    for call, msg in bad:
        with pytest.raises(ValueError, match=re.escape(msg)):
            call()

    class Undefined:
        _stepper = None
    from fib_tf_amd.stimulus import StimulusProgram
    with pytest.raises(AssertionError, match='after calling define'):
        StimulusProgram(Undefined(), [Stimulus('left', 1.0, **ok)])
    from fib_tf_amd.fenton import Fenton4v
    with pytest.raises(AssertionError, match='after calling define'):
        Fenton4v({'height': 32, 'width': 32, 'dt': 0.1, 'diff': 1.5, 'duration': 10, 'dt_per_plot': 10}).program_stimuli([])


def test_sharded_model_is_refused():
    """the Python guard: a model that runs as row blocks raises NotImplementedError before anything reaches the library"""
    from fib_tf_amd import stimulus
    from fib_tf_amd.sharded import ShardedStepper

    class M(Model):
        _stepper = ShardedStepper.__new__(ShardedStepper)
    M._stepper.world = 2
    with pytest.raises(NotImplementedError, match='single device only'):
        stimulus.StimulusProgram(M(), [stimulus.Stimulus('left', 1.0, at_tick=0)])
    M._stepper = None


def test_example_and_bench_tool_parse_their_arguments():
    """examples/run_s1s2.py and tools/bench_stimulus.py import without a device and refuse what they cannot run"""
    import importlib.util

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    bench = load('tools/bench_stimulus.py', 'bench_stimulus_cpu')
    assert bench.parse_config('fenton512') == ('fenton', 512) and bench.parse_config('court1024') == ('court', 1024)
    for bad in ('fenton', 'br512', 'fenton8', 'court-3'):
        with pytest.raises(ValueError, match='a configuration is'):
            bench.parse_config(bad)
    with pytest.raises(ValueError, match='a configuration is'):
        bench.main(['--configs', 'fenton512,nope'])               # refused before anything is created
    with pytest.raises(SystemExit):
        bench.main(['--ticks', 'many'])
    ex = load('examples/run_s1s2.py', 'run_s1s2_cpu')
    with pytest.raises(SystemExit):
        ex.main(['--size', 'large'])
    assert callable(ex.main)
