"""not-gpu: the lesion program's host side — the declarations and their binding, fib_tf_amd/lesions.py against the NumPy
restatement (tests/lesion_ref.py) and against add_hole_to_phase_field itself, the event arithmetic, every refusal.  Every
comparison is equality of bytes."""
import copy
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lesion_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 70, 130
# (x, y, radius): the interior, a corner, the opposite corner / edge, a large one, a centre between cells with a radius below 1
DISCS = [(40, 30, 6), (0, 0, 5), (129, 69, 3), (60, 35, 12), (64.5, 20.25, 0.5)]


def model():
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': H, 'width': W, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 10})
    m.add_hole_to_phase_field(90, 40, 9)
    return m


def test_declarations_and_binding():
    from fib_tf_amd import _lib
    C = _lib.C
    src = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    for name, nargs in (('fibhip_lesion_begin', 5), ('fibhip_lesion_count', 2), ('fibhip_lesion_end', 1), ('fibhip_lesion_apply', 3),
                        ('fibhip_get_phase', 2)):
        assert 'int %s(' % name in src
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is C.c_int and len(_lib.SYMBOLS[name][0]) == nargs
    body = re.search(r'typedef struct fibhip_lesion_entry \{(.*?)\} fibhip_lesion_entry;', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        parts = decl.strip().rsplit(None, 1) if ',' not in decl else decl.strip().split(None, 1)
        if len(parts) == 2:
            fields += [(n.strip(), parts[0]) for n in parts[1].split(',')]
    assert [f[0] for f in fields] == [f[0] for f in _lib.LesionEntry._fields_]
    assert [{'int': C.c_int, 'long long': C.c_longlong}[t] for _, t in fields] == [f[1] for f in _lib.LesionEntry._fields_]
    assert C.sizeof(_lib.LesionEntry) == 32
    assert '#define FIBHIP_MAX_LESION_ENTRIES %d' % _lib.MAX_LESION_ENTRIES in src and _lib.MAX_LESION_ENTRIES == 256
    assert '#define FIBHIP_ABI_VERSION 1' in src
    for method in ('lesion_begin', 'lesion_count', 'lesion_end', 'lesion_apply', 'get_phase'):
        assert callable(getattr(_lib.Stepper, method))


@pytest.mark.parametrize('disc', DISCS, ids=lambda d: 'x%g_y%g_r%g' % d)
def test_cropped_patch_equals_add_hole_to_phase_field(disc):
    """the patch cut to the bounding box of mask != 1.0f, applied inside the box only, leaves the bytes of
    np.maximum(phase * mask, 1e-5) on the whole plane — add_hole_to_phase_field on a copy of the model"""
    from fib_tf_amd import lesions
    x, y, r = disc
    m = model()
    assert m.phase.dtype == np.float32 and m.phase.tobytes() == ref.hole_field().tobytes() and (m.phase >= ref.FLOOR).all()
    twin = copy.copy(m)
    twin.phase = m.phase.copy()
    twin.add_hole_to_phase_field(x, y, r)
    box, p = lesions.patch(m, ('disc', y, x, r))
    rbox, rp = ref.patch(H, W, ('disc', y, x, r))
    assert box == rbox and p.dtype == np.float32 and p.tobytes() == rp.tobytes()
    got = lesions.apply_host(m.phase, box, p)
    assert got.dtype == np.float32 and got.tobytes() == twin.phase.tobytes()
    assert ref.apply_host(m.phase, rbox, rp).tobytes() == twin.phase.tobytes()
    # outside the box nothing changes; the box is about radius + 9 cells wide on each side, cut at the grid
    outside = np.ones((H, W), bool)
    outside[box[0]:box[1], box[2]:box[3]] = False
    assert got[outside].tobytes() == m.phase[outside].tobytes() and (got != m.phase).any()
    assert box[1] - box[0] <= 2 * (r + 10) + 1 and box[3] - box[2] <= 2 * (r + 10) + 1
    assert (got >= ref.FLOOR).all()


def test_program_order_is_part_of_the_definition():
    """two overlapping lesions on the outer tail of the hole: each order leaves other bytes somewhere, so a test can tell them apart"""
    from fib_tf_amd import lesions
    m = model()
    a, b = ref.ORDER_PAIR
    ab = ref.apply_sites(m.phase, H, W, [a, b])
    ba = ref.apply_sites(m.phase, H, W, [b, a])
    assert (ab != ba).sum() > 10
    (ba_box, _), (bb_box, _) = ref.patch(H, W, a), ref.patch(H, W, b)
    assert ba_box[0] < bb_box[1] and bb_box[0] < ba_box[1] and ba_box[2] < bb_box[3] and bb_box[2] < ba_box[3]        # the boxes overlap
    got = m.phase
    for s in (a, b):
        got = lesions.apply_host(got, *lesions.patch(m, s))
    assert got.tobytes() == ab.tobytes()
    # on a field of ones the two products commute: the pair has to sit where phi is neither 1 nor the floor
    ones = np.ones((H, W), np.float32)
    assert ref.apply_sites(ones, H, W, [a, b]).tobytes() == ref.apply_sites(ones, H, W, [b, a]).tobytes()


def test_line_plane_and_drag_sites():
    from fib_tf_amd import lesions
    m = model()
    for seg in ((10, 5, 60, 100, 2.5), (35, 20, 35, 129, 1.0), (3, 3, 3, 3, 2.0), (0, 64.5, 69, 64.5, 0.75)):
        want = ref.line_plane(H, W, *seg)
        got = lesions.factors(m, ('line',) + seg)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), seg
        box, p = lesions.patch(m, ('line',) + seg)
        assert (box, p.tobytes()) == (ref.patch(H, W, ('line',) + seg)[0], ref.patch(H, W, ('line',) + seg)[1].tobytes())
        assert got.min() < 0.5                                        # (the segment itself is cut)
    # a segment of no length is the disc around its point
    assert lesions.factors(m, ('line', 3, 3, 3, 3, 2.0)).tobytes() == ref.disc_plane(H, W, 3, 3, 2.0).tobytes()
    # a plane: cropped to the factors that are not 1, whatever they are
    plane = np.ones((H, W))
    plane[5:9, 100:103] = [[0.5, 1.0, 0.25]] * 4
    plane[20, 7] = 0.0
    box, p = lesions.patch(m, plane)
    assert box == (5, 21, 7, 103) and p.shape == (16, 96) and p.dtype == np.float32 and p[0, 93] == 0.5 and p[15, 0] == 0.0
    assert lesions.apply_host(m.phase, box, p).tobytes() == ref.apply_host(m.phase, box, p).tobytes()
    assert lesions.apply_host(m.phase, box, p)[20, 7] == ref.FLOOR
    # drag: one disc per point, dwell_ms apart; a tick is dt_per_step * dt = 0.1 ms on an undefined model (dt_per_step = 1)
    path = [(10, 10), (12, 14), (14, 18.5)]
    ls = lesions.drag(path, start_ms=2.0, dwell_ms=0.5, radius=3)
    assert [l.site for l in ls] == [('disc', r, c, 3) for r, c in path]
    assert [l.tick(m) for l in ls] == [m.millisecond_to_step(2.0 + 0.5 * i) for i in range(3)] == [20, 25, 30]
    entries = lesions.compile_program(m, ls)
    assert [e[0] for e in entries] == [20, 25, 30]
    for (t, box, p), (r, c) in zip(entries, path):
        rbox, rp = ref.patch(H, W, ('disc', r, c, 3))
        assert box == rbox and p.tobytes() == rp.tobytes()


def test_event_arithmetic():
    """entries in any order of ticks, several on one tick: the expansion equals a tick-by-tick walk, program order within a tick"""
    from fib_tf_amd import lesions
    m = model()
    ticks = [9, 3, 9, 0, 40, 3, 63]
    entries = lesions.compile_program(m, [lesions.Lesion(('disc', 20, 20 + i, 2), at_tick=t) for i, t in enumerate(ticks)])
    for n in (0, 1, 4, 10, 64, 100):
        assert lesions.expand(entries, n) == ref.events(ticks, n), n
    assert ref.events(ticks, 10) == [(0, 3), (3, 1), (3, 5), (9, 0), (9, 2)]
    # the library's rule (csrc/sched.inc lesion_next, lesion_advance): with k ticks launched, the entries with tick + 1 == k are
    # due and the next event tick is the smallest tick + 1 above k — walked here launch by launch as the scheduler cuts them
    k, applied = 0, []
    while True:
        nxt = min([t + 1 for t in ticks if t + 1 > k], default=None)
        if nxt is None:
            break
        k = nxt                                                       # (no launch spans an event tick: k lands on it)
        applied += [(k - 1, i) for i, t in enumerate(ticks) if t + 1 == k]
    assert applied == ref.events(ticks, 64)
    # milliseconds go through millisecond_to_step
    assert lesions.Lesion(('disc', 1, 1, 1), at_ms=2.37).tick(m) == 23


def test_refused_arguments():
    from fib_tf_amd import lesions
    from fib_tf_amd.lesions import Lesion
    m = model()
    disc = ('disc', 30, 40, 5)
    bad = [(lambda: Lesion(disc), 'at_ms or at_tick'), (lambda: Lesion(disc, at_ms=1, at_tick=1), 'at_ms or at_tick'),
           (lambda: Lesion(disc, at_tick=-1).tick(m), 'must be >= 0'),
           (lambda: lesions.patch(m, ('disc', 300, 300, 2)), 'changes no cell'),
           (lambda: lesions.patch(m, np.ones((H, W))), 'changes no cell'),
           (lambda: lesions.patch(m, ('ring', 1, 2, 3)), 'a site is'),
           (lambda: lesions.patch(m, ('disc', 1, 2)), 'a site is'),
           (lambda: lesions.patch(m, np.ones((3, 3))), 'a site of shape'),
           (lambda: lesions.patch(m, np.full((H, W), 1.5)), 'finite and in [0, 1]'),
           (lambda: lesions.patch(m, np.full((H, W), -0.1)), 'finite and in [0, 1]'),
           (lambda: lesions.patch(m, np.full((H, W), np.nan)), 'finite and in [0, 1]'),
           (lambda: lesions.compile_program(m, []), '1 .. 256 entries'),
           (lambda: lesions.compile_program(m, [Lesion(disc, at_tick=0)] * 257), '1 .. 256 entries'),
           (lambda: lesions.compile_program(m, [disc]), 'not a Lesion'),
           (lambda: lesions.compile_program(m, [Lesion(np.zeros((H, W)), at_tick=i) for i in range(9)]), 'more than 8 planes'),
           (lambda: lesions.check_field(np.zeros((H, W), np.float32)), '>= 1e-5 everywhere')]
    for call, msg in bad:
        with pytest.raises(ValueError, match=re.escape(msg)):
            call()
    lesions.check_field(None)
    lesions.check_field(m.phase)
    with pytest.raises(AssertionError, match='after calling define'):
        m.program_lesions([Lesion(disc, at_tick=0)])
    with pytest.raises(AssertionError, match='after calling define'):
        m.ablate(disc)

    class Defined:
        _stepper, phase, height, width = None, None, H, W
    with pytest.raises(AssertionError, match='after calling define'):
        lesions.LesionProgram(Defined(), [Lesion(disc, at_tick=0)])
    # a field below the floor somewhere is refused before anything reaches the library (the identity would not hold)
    Defined._stepper = object()
    Defined.phase = np.zeros((H, W), np.float32)
    with pytest.raises(ValueError, match='>= 1e-5 everywhere'):
        lesions.LesionProgram(Defined(), [Lesion(disc, at_tick=0)])
    with pytest.raises(ValueError, match='>= 1e-5 everywhere'):
        lesions.ablate(Defined(), disc)


def test_end_that_fails_leaves_the_program_open():
    """end() marks the program closed only after lesion_end() and get_phase() went through: if one raises, the program is still
    attached on the handle, the object says so, and a second end() tries again"""
    from fib_tf_amd import lesions

    class Handle:
        fail, ended = True, 0

        def lesion_begin(self, entries):
            self.entries = entries

        def lesion_end(self):
            if self.fail:
                raise RuntimeError('the device said no')
            self.ended += 1

        def get_phase(self):
            return np.full((H, W), 0.5, np.float32)

    class M:
        height, width, phase, dt, dt_per_step, _stepper = H, W, None, 0.1, 10, Handle()
    m = M()
    prog = lesions.LesionProgram(m, [lesions.Lesion(('disc', 30, 40, 5), at_tick=0)])
    with pytest.raises(RuntimeError, match='said no'):
        prog.end()
    assert prog.open and m.phase is None
    M._stepper.fail = False
    prog.end()
    prog.end()
    assert not prog.open and M._stepper.ended == 1 and m.phase[0, 0] == 0.5


def test_sharded_model_is_refused():
    """the Python guard: a model that runs as row blocks raises NotImplementedError before anything reaches the library"""
    from fib_tf_amd import lesions
    from fib_tf_amd.sharded import ShardedStepper

    class M:
        height, width, phase = H, W, None
        _stepper = ShardedStepper.__new__(ShardedStepper)
    M._stepper.world = 2
    with pytest.raises(NotImplementedError, match='single device only'):
        lesions.LesionProgram(M(), [lesions.Lesion(('disc', 30, 40, 5), at_tick=0)])
    with pytest.raises(NotImplementedError, match='single device only'):
        lesions.ablate(M(), ('disc', 30, 40, 5))
    M._stepper = None


def test_example_and_bench_tool_parse_their_arguments():
    """examples/run_ablation.py and tools/bench_lesions.py import without a device and refuse what they cannot run"""
    import importlib.util

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    bench = load('tools/bench_lesions.py', 'bench_lesions_cpu')
    with pytest.raises(SystemExit):
        bench.main(['--ticks', 'many'])
    with pytest.raises(ValueError, match='at least'):
        bench.main(['--size', '8'])
    ex = load('examples/run_ablation.py', 'run_ablation_cpu')
    with pytest.raises(SystemExit):
        ex.main(['--size', 'large'])
    assert callable(ex.main)
