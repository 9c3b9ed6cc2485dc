"""-m gpu: what the ten samplers' entry points have in common, at the C ABI — the twin of tests/test_recorder_contract_cpu.py one
layer down.  One table with a row per sampler (electrode, tips, frames, stats, leads, pmap, waves, spectrum, beats, trig), one
handle for all rows (Fenton, 64 x 80: W % 4 == 0, so the hooks' vector paths are the ones that run).  Every row calls the library
through ctypes and compares fibhip_last_error() WHOLE: the messages of _count, _read and _end with nothing attached, of _begin
with a bad var, every = 0 and capacity = 0, which refusal wins when two apply, and — behind a good attach with every = 2,
capacity = 3 and six ticks — the count, the range and null-destination refusals of _read, a second _begin (refused or accepted,
as the row says) and _end twice.  Nothing is launched beyond those ticks."""
import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_tips import fenton  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 64, 80
EVERY, CAPACITY, TICKS = 2, 3, 6
_fp, _ip, _dp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)
ONES = np.ones((H, W), np.float32)
WHOLE = (C.c_int * 4)(0, H, 0, W)

# who: the prefix of every message; noun: "recorder" / "program"; what: the word of _read's range message; begin(L, h, var, every,
# capacity): the attach with everything else good; read(L, h, first, count, dst): the ranged read (None: the sampler has none)
# and nbytes(count) the destination it needs; bad_var: the message of var = nvar; var_wins: is that the message when every = 0 as
# well?; capacity: does _begin take one?; again: a second _begin is "refused" or "accepted"
Row = namedtuple('Row', 'who noun what begin read nbytes bad_var var_wins capacity again')


def _electrode(L, h, var, every, capacity):
    return L.fibhip_electrode_begin(h, var, 1, (C.c_int * 4)(1, 3, 2, 6), (C.c_float * 8)(*[0.125] * 8), every, capacity)


def _tips(L, h, var, every, capacity):
    return L.fibhip_tips_begin(h, var, 1, 0.5, 0.5, None, every, 4, capacity)


def _frames(L, h, var, every, capacity):
    return L.fibhip_frames_begin(h, var, WHOLE, 16, 16, 1, 0.0, 1.0, None, 0, every, every, capacity)


def _stats(L, h, var, every, capacity):
    from fib_tf_amd._lib import StatCol
    return L.fibhip_stats_begin(h, 1, (StatCol * 1)(StatCol(var, 1, 0.0)), None, None, every, capacity)


def _leads(L, h, var, every, capacity):
    return L.fibhip_leads_begin(h, var, 1, (C.c_int * 3)(5, 7, 0), 1, ONES.ctypes.data_as(_fp), None, every, capacity)


def _pmap(L, h, var, every, capacity):
    return L.fibhip_pmap_begin(h, var, 1, (C.c_float * 4)(1.0, 0.5, 0.5, 0.25), None, WHOLE, 16, 16, every, capacity)


def _waves(L, h, var, every, capacity):
    return L.fibhip_waves_begin(h, var, 0, 0.5, -1, 0, 0.0, 4, None, 4, every, capacity)


def _spectrum(L, h, var, every, capacity):
    win, tw = (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 8)(1, 0, 0, -1, -1, 0, 0, 1)
    return L.fibhip_spectrum_begin(h, var, WHOLE, 16, 16, 1, None, every, 4, win, tw, 2, (C.c_int * 2)(0, 1), 2)


def _beats(L, h, var, every, capacity):
    return L.fibhip_beats_begin(h, var, WHOLE, 16, 16, 1, None, every, 0.6, 0.4, 2)


def _trig(L, h, var, every, capacity):
    from fib_tf_amd._lib import TrigRule, TrigSensor
    sensor = TrigSensor(var, 0.5, 1, 0, 1, 3, 2, 6)
    rule = TrigRule(0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 10, 12, 10, 14, 1.0, 0.0, 0)
    return L.fibhip_trig_begin(h, 1, C.byref(sensor), None, 1, C.byref(rule), 0, None, every, capacity)


def _one(name, ptr):
    return lambda L, h, first, count, dst: getattr(L, 'fibhip_%s_read' % name)(h, first, count, C.cast(dst, ptr))


def _two(name):
    """counts (three ints a sample: the destination whose null is refused) and, behind them in the same buffer, the records"""
    def read(L, h, first, count, dst):
        fn = getattr(L, 'fibhip_%s_read' % name)
        if dst is None:
            return fn(h, first, count, None, None)
        return fn(h, first, count, C.cast(dst, _ip), C.cast(C.c_void_p(C.addressof(dst) + 12 * CAPACITY), fn.argtypes[4]))
    return read


ROWS = [
    Row('electrode', 'recorder', 'samples', _electrode, _one('electrode', _fp), 4, 'electrode_begin: bad var 4', True, True, 'accepted'),
    Row('tips', 'recorder', 'samples', _tips, _two('tips'), 12 + 4 * 16, 'tips_begin: bad var 4 / 1', True, True, 'accepted'),
    Row('frames', 'recorder', 'frames', _frames, _one('frames', C.c_void_p), 4 * 5 * 4, 'frames_begin: bad var 4', True, True, 'accepted'),
    Row('stats', 'recorder', 'samples', _stats, _one('stats', _dp), 8, 'stats_begin: column 0: bad var 4', True, True, 'refused'),
    Row('leads', 'recorder', 'samples', _leads, _one('leads', _dp), 8, 'leads_begin: bad var 4', True, True, 'accepted'),
    Row('pmap', 'recorder', 'samples', _pmap, _one('pmap', _dp), 4 * 5 * 8, 'pmap_begin: bad var 4', True, True, 'accepted'),
    Row('waves', 'recorder', 'samples', _waves, _two('waves'), 12 + 4 * 40, 'waves_begin: bad var 4', True, True, 'accepted'),
    Row('spectrum', 'recorder', None, _spectrum, None, 0, 'spectrum_begin: bad var 4', True, False, 'refused'),
    Row('beats', 'recorder', None, _beats, None, 0, 'beats_begin: bad var 4', True, False, 'refused'),
    # (trig_begin looks at every and capacity before it walks its sensors: there every = 0 wins over a sensor's bad var)
    Row('trig', 'program', 'samples', _trig, _one('trig', _ip), 6 * 4, 'trig_begin: sensor 0: bad var 4', False, True, 'refused'),
]


@pytest.fixture(scope='module')
def handle(gpu_lib):
    m = fenton(H, W)
    st = m._stepper
    assert st.nvar == 4
    yield st._L, st._h
    st.close()


def _count(L, h, row):
    """(return code, samples): spectrum_count takes a second output, which stays null here"""
    n = C.c_longlong(-1)
    fn = getattr(L, 'fibhip_%s_count' % row.who)
    return (fn(h, C.byref(n), None) if row.who == 'spectrum' else fn(h, C.byref(n))), n.value


def _plain_read(L, h, row):
    """the read of a sampler without a range: every destination null (both accept that)"""
    return L.fibhip_spectrum_read(h, None, None) if row.who == 'spectrum' else L.fibhip_beats_read(h, None, None, None, None, None)


@pytest.mark.parametrize('row', ROWS, ids=[r.who for r in ROWS])
def test_entry_point_contract(handle, row):
    L, h = handle
    who = row.who
    err = lambda: L.fibhip_last_error().decode()                              # noqa: E731
    begin = lambda var=0, every=EVERY, capacity=CAPACITY: row.begin(L, h, var, every, capacity)     # noqa: E731
    end = getattr(L, 'fibhip_%s_end' % who)
    unattached = 'no %s attached (fibhip_%s_begin)' % (row.noun, who)
    buf = (C.c_ubyte * max(1, CAPACITY * row.nbytes))()

    # nothing attached
    assert _count(L, h, row)[0] == -1 and err() == '%s_count: %s' % (who, unattached)
    rc = row.read(L, h, 0, 1, buf) if row.read else _plain_read(L, h, row)
    assert rc == -1 and err() == '%s_read: %s' % (who, unattached)
    assert end(h) == 0

    # one bad argument, then two at once
    every_msg = '%s_begin: every must be >= 1 (got 0)' % who
    assert begin(var=4) == -1 and err() == row.bad_var
    assert begin(every=0) == -1 and err() == every_msg
    assert begin(var=4, every=0) == -1 and err() == (row.bad_var if row.var_wins else every_msg)
    if row.capacity:
        assert begin(capacity=0) == -1 and err() == '%s_begin: bad capacity 0' % who
        assert begin(every=0, capacity=0) == -1 and err() == every_msg
    assert _count(L, h, row)[0] == -1 and err() == '%s_count: %s' % (who, unattached)          # (none of them attached anything)

    # a good attach, six ticks
    assert begin() == 0, err()
    assert L.fibhip_step(h, TICKS) == 0, err()
    assert _count(L, h, row) == (0, TICKS // EVERY), err()
    if row.read:
        assert row.read(L, h, 2, 2, buf) == -1 and err() == '%s_read: %s [2, 4) of 3 taken' % (who, row.what)
        assert row.read(L, h, 0, 1, None) == -1 and err() == '%s_read: null destination' % who
        assert row.read(L, h, 0, 3, buf) == 0, err()
    else:
        assert _plain_read(L, h, row) == 0, err()

    # a second attach
    if row.again == 'refused':
        assert begin() == -1 and err() == '%s_begin: a %s is attached already (fibhip_%s_end first)' % (who, row.noun, who)
        assert _count(L, h, row) == (0, TICKS // EVERY)
    else:
        assert begin() == 0, err()
        assert _count(L, h, row) == (0, 0)                                    # (the old recorder went silently, the new one starts at 0)
    assert end(h) == 0 and end(h) == 0
    assert _count(L, h, row)[0] == -1 and err() == '%s_count: %s' % (who, unattached)
