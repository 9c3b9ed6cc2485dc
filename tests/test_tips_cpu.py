"""not-gpu: the tip recorder's host side — the NumPy restatement of the definition on fields with known tips, the
declarations of include/fibhip.h and their ctypes prototypes, TipRecorder over a stub stepper that follows the header, the
trajectory linker, and the refusal on row blocks (gloo ranks over the CPU test engine)."""
import multiprocessing as mp
import os
import re
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import tip_ref as ref  # noqa: E402

NAMES = ('fibhip_tips_begin', 'fibhip_tips_count', 'fibhip_tips_read', 'fibhip_tips_end')
H, W = 37, 53


def grid(h=H, w=W):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    return y, x


def two_vortices(h=H, w=W, z1=(8.5, 10.5), z2=(30.5, 40.5)):
    """(A, B) = real and imaginary part of (z - z1) * conj(z - z2), z = x + iy: a +1 tip at z1 and a -1 tip at z2 (row, column)"""
    y, x = grid(h, w)
    z = ((x - z1[1]) + 1j * (y - z1[0])) * np.conj((x - z2[1]) + 1j * (y - z2[0]))
    return z.real.astype(np.float32), z.imag.astype(np.float32)


def scalar_charges(A, B, a0, b0):
    """the definition once more, cell by cell in Python: float32 subtraction, Python floats (doubles) for the cross product"""
    a = (np.asarray(A, np.float32) - np.float32(a0)).astype(np.float32)
    b = (np.asarray(B, np.float32) - np.float32(b0)).astype(np.float32)
    out = np.zeros((a.shape[0] - 1, a.shape[1] - 1), np.int32)
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            c = [(i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j)]
            w = 0
            for e in range(4):
                a1, b1, a2, b2 = float(a[c[e]]), float(b[c[e]]), float(a[c[(e + 1) % 4]]), float(b[c[(e + 1) % 4]])
                cross = a1 * b2 - a2 * b1
                if b1 < 0 and b2 >= 0 and cross > 0:
                    w += 1
                if b2 < 0 and b1 >= 0 and cross < 0:
                    w -= 1
            out[i, j] = w
    return out


# ---- the definition on fields with known tips ----------------------------------------------------------------------
def test_one_tip_and_its_mirror():
    y, x = grid()
    A, B = x - np.float32(20.3), y - np.float32(11.6)
    rec, (pos, neg) = ref.tips(A, B, 0, 0)
    assert rec.tolist() == [[11, 20, 1]] and (pos, neg) == (1, 0)
    rec, (pos, neg) = ref.tips(A, -B, 0, 0)
    assert rec.tolist() == [[11, 20, -1]] and (pos, neg) == (0, 1)
    rec, _ = ref.tips(x, y, 20.3, 11.6)                         # the same tip through the levels
    assert rec.tolist() == [[11, 20, 1]]


def test_two_vortices_of_opposite_charge():
    A, B = two_vortices()
    rec, (pos, neg) = ref.tips(A, B, 0, 0)
    assert rec.tolist() == [[8, 10, 1], [30, 40, -1]] and (pos, neg) == (1, 1)


def test_origin_on_a_grid_corner_is_reported_once():
    y, x = grid()
    w = ref.charges(x - 20, y - 11, 0, 0)
    around = w[10:12, 19:21]
    assert np.count_nonzero(w) == 1 and np.count_nonzero(around) == 1 and w.sum() == 1


def test_nan_gives_no_crossing():
    """an edge with a NaN end has no crossing.  Where such an edge would have had none anyway the tip stands alone; where it
    would have had one, the plaquettes on either side of it lose the partner that cancelled their other crossing and report
    a charge of their own — that is the definition, and the restatements agree on it"""
    y, x = grid()
    A, B = x - np.float32(20.3), y - np.float32(11.6)
    A1 = A.copy()
    A1[11, 19] = np.nan                                         # next to the tip, not one of its corners; a < 0 there
    rec, counts = ref.tips(A1, B, 0, 0)
    assert rec.tolist() == [[11, 20, 1]] and counts == (1, 0)
    A2 = A.copy()
    A2[11, 22] = np.nan                                         # on the other side: the edges below it do cross
    rec, counts = ref.tips(A2, B, 0, 0)
    assert rec.tolist() == [[11, 20, 1], [11, 21, -1], [11, 22, 1]] and counts == (2, 1)
    B2 = B.copy()
    B2[12, 21] = np.nan                                         # a corner of the tip's plaquette
    for a, b in ((A1, B), (A2, B), (A, B2), (A2, B2)):
        assert np.array_equal(ref.charges(a, b, 0, 0), scalar_charges(a, b, 0, 0))
    assert np.count_nonzero(ref.charges(np.full((5, 7), np.nan, np.float32), B[:5, :7], 0, 0)) == 0
    assert np.count_nonzero(ref.charges(A[:5, :7], np.full((5, 7), np.nan, np.float32), 0, 0)) == 0


def test_noise_against_the_scalar_restatement():
    rng = np.random.default_rng(0)
    A = rng.uniform(-1, 1, (96, 130)).astype(np.float32)
    B = rng.uniform(-1, 1, (96, 130)).astype(np.float32)
    w = ref.charges(A, B, 0, 0)
    assert w.shape == (95, 129) and set(np.unique(w)) == {-1, 0, 1}
    assert np.count_nonzero(w) == 4094                          # (of 12 255 plaquettes)
    assert np.array_equal(w[:20, :40], scalar_charges(A[:21, :41], B[:21, :41], 0, 0))
    assert np.array_equal(ref.charges(A, B, 0.25, -0.5)[:12, :30], scalar_charges(A[:13, :31], B[:13, :31], 0.25, -0.5))
    rec, (pos, neg) = ref.tips(A, B, 0, 0)
    assert len(rec) == pos + neg == 4094 and rec.dtype == np.int32
    assert np.array_equal(rec, rec[np.lexsort((rec[:, 1], rec[:, 0]))])


def test_mask_removes_exactly_the_plaquettes_that_touch_it():
    rng = np.random.default_rng(3)
    A = rng.uniform(-1, 1, (H, W)).astype(np.float32)
    B = rng.uniform(-1, 1, (H, W)).astype(np.float32)
    mask = np.ones((H, W), np.uint8)
    mask[10:14, 20:30] = 0
    mask[0, 0] = mask[H - 1, W - 1] = mask[5, W - 1] = 0
    free, got = ref.charges(A, B, 0, 0), ref.charges(A, B, 0, 0, mask)
    touch = np.zeros((H - 1, W - 1), bool)
    for i, j in np.argwhere(mask == 0):
        touch[max(i - 1, 0):i + 1, max(j - 1, 0):j + 1] = True
    assert np.count_nonzero(free[touch]) > 0                    # (the mask does remove something)
    assert np.count_nonzero(got[touch]) == 0
    assert np.array_equal(got[~touch], free[~touch])
    assert touch.sum() == 5 * 11 + 1 + 1 + 2


def test_header_declares_and_lib_prototypes():
    from fib_tf_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(\s*fibhip_t\b' % name, src), name
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is _lib.C.c_int
    assert re.search(r'#define\s+FIBHIP_MAX_TIPS\s+65536\b', src)
    begin = _lib.SYMBOLS['fibhip_tips_begin'][0]
    assert len(begin) == 9 and begin[3] is _lib.C.c_float and begin[4] is _lib.C.c_float and begin[8] is _lib.C.c_longlong
    assert len(_lib.SYMBOLS['fibhip_tips_read'][0]) == 5
    for m in ('tips_begin', 'tips_count', 'tips_read', 'tips_end'):
        assert callable(getattr(_lib.Stepper, m))


# ---- TipRecorder over a stub stepper --------------------------------------------------------------------------------
class StubStepper:
    """keeps two state arrays on the host: a tick moves the two vortices one column to the right; the tips_* methods
    follow include/fibhip.h, the records of a sample in a shuffled order (the device's order is the order of arrival)"""
    steps_per_tick = 10

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.ticks = 0
        self.tip = None
        self.rng = np.random.default_rng(11)
        self._fields()

    def _fields(self):
        self.x = list(two_vortices(self.h, self.w, (8.5, 10.5 + self.ticks), (30.5, 20.5 + self.ticks)))

    def step(self, n):
        for _ in range(n):
            self.ticks += 1
            self._fields()
            t = self.tip
            if t is not None:
                t['k'] += 1
                if t['k'] % t['every'] == 0:
                    assert len(t['counts']) < t['cap'], 'trace full'
                    rec, (pos, neg) = ref.tips(self.x[t['var']], self.x[t['var2']], t['a0'], t['b0'], t['mask'])
                    rec = rec[self.rng.permutation(len(rec))]
                    slot = np.full((t['max'], 4), -7, np.int32)          # (beyond `stored`: whatever was there)
                    keep = min(len(rec), t['max'])
                    slot[:keep, :3] = rec[:keep]
                    slot[:keep, 3] = 0
                    t['counts'].append((pos, neg, pos + neg))
                    t['records'].append(slot)
                    t['at'].append(self.ticks - 1)

    def tips_begin(self, var, var2, a0, b0, mask=None, every=1, max_tips=256, capacity=1):
        self.tip = {'var': var, 'var2': var2, 'a0': a0, 'b0': b0, 'mask': mask, 'every': every, 'max': max_tips, 'cap': capacity,
                    'k': 0, 'counts': [], 'records': [], 'at': []}

    def tips_count(self):
        return len(self.tip['counts'])

    def tips_read(self, first=0, count=None, records=True):
        sl = slice(first, None if count is None else first + count)
        c = np.array(self.tip['counts'][sl], np.int32).reshape(-1, 3)
        r = np.array(self.tip['records'][sl], np.int32).reshape(-1, self.tip['max'], 4) if records else None
        return c, r

    def tips_end(self):
        self.last, self.tip = self.tip, None


def stub_model(h=40, w=56, duration=12.0, phase=None, cls=None):
    from fib_tf_amd.fenton import Fenton4v
    m = (cls or Fenton4v)({'height': h, 'width': w, 'dt': 0.1, 'diff': 1.0, 'duration': duration})
    m._stepper = StubStepper(h, w)
    m.defined = True
    m.dt_per_step = 10
    m.phase = phase
    return m


def test_recorder_sample_ticks_sorting_and_time():
    m = stub_model()
    st = m._stepper
    with m.record_tips(var2=1, levels=(0.0, 0.0), every=3) as rec:
        assert rec.capacity == 4 and rec.every == 3 and (rec.var, rec.var2) == (0, 1) and rec.mask is None
        st.step(12)
        assert st.tip['at'] == [2, 5, 8, 11]                        # after the ticks with (k + 1) % every == 0
        assert rec.count() == 4
        counts = rec.counts()
        assert counts.dtype == np.int32 and counts.tolist() == [[1, 1, 2]] * 4
        per = rec.tips()
        assert len(per) == 4 and len(rec.truncated()) == 0
        for s, a in enumerate(per):
            assert a.dtype.names == ('t_ms', 'y', 'x', 'charge')
            shift = 3 * (s + 1)                                    # the state after tick 3 s + 2 has moved 3 (s + 1) columns
            assert a['y'].tolist() == [8.5, 30.5] and a['x'].tolist() == [10.5 + shift, 20.5 + shift]     # sorted by (row, column)
            assert a['charge'].tolist() == [1, -1]
            assert np.all(a['t_ms'] == (s + 1) * 3 * 1.0)          # ms since attach: (s + 1) * every ticks of dt_per_step * dt
        assert [a['x'].tolist() for a in rec.tips(first=2, count=1)] == [[19.5, 29.5]]
        assert rec.tips(first=2, count=1)[0]['t_ms'][0] == 9.0
    assert st.tip is None
    with pytest.raises(AssertionError, match='closed'):
        rec.tips()
    with pytest.raises(AssertionError, match='closed'):
        rec.count()
    rec.close()                                                    # (closing twice does nothing)


def test_recorder_sorts_many_tips_and_reports_truncation():
    m = stub_model(h=30, w=44, duration=4.0)
    st = m._stepper
    rng = np.random.default_rng(5)
    noise = [rng.uniform(-1, 1, (30, 44)).astype(np.float32) for _ in range(2)]
    st._fields = lambda: setattr(st, 'x', noise if st.ticks == 2 else list(two_vortices(30, 44, (8.5, 10.5), (20.5, 30.5))))
    want, (pos, neg) = ref.tips(noise[0], noise[1], 0, 0)
    assert len(want) > 64
    with m.record_tips(var2=1, levels=(0, 0), max_tips=64) as rec:
        st.step(4)
        assert rec.truncated().tolist() == [1]
        assert rec.counts()[1].tolist() == [pos, neg, pos + neg]
        per = rec.tips()
        assert [len(a) for a in per] == [2, 64, 2, 2]
        got = np.stack([per[1]['y'] - 0.5, per[1]['x'] - 0.5], axis=1).astype(np.int32)
        assert np.array_equal(got, got[np.lexsort((got[:, 1], got[:, 0]))])      # sorted, whatever the order of arrival
        assert len(set(map(tuple, got))) == 64 and set(map(tuple, got)) <= set(map(tuple, want[:, :2]))
    with m.record_tips(var2=1, levels=(0, 0), max_tips=4096) as rec:
        st.ticks = 1
        st.step(1)
        a = rec.tips()[0]
        assert np.array_equal(np.stack([a['y'] - 0.5, a['x'] - 0.5, a['charge']], axis=1).astype(np.int32), want)


def test_default_mask_comes_from_the_phase_field():
    phase = np.ones((40, 56), np.float32)
    phase[5:12, 8:16] = 1e-5                                        # a hole over the first vortex
    m = stub_model(phase=phase)
    with m.record_tips(var2=1, levels=(0, 0)) as rec:
        got = m._stepper.tip['mask']
        assert got.dtype == np.uint8 and np.array_equal(got != 0, phase > 0.5) and rec.mask is got
        m._stepper.step(1)
        assert rec.counts().tolist() == [[0, 1, 1]]                 # the tip inside the hole does not count
    own = np.ones((40, 56), bool)
    with m.record_tips(var2=1, levels=(0, 0), mask=own):
        assert m._stepper.tip['mask'].all()
    with pytest.raises(ValueError, match='mask of shape'):
        m.record_tips(var2=1, levels=(0, 0), mask=np.ones((40, 57)))


def test_defaults_come_from_tip_signals():
    from fib_tf_amd.br import BeelerReuter
    from fib_tf_amd.court import Courtemanche
    from fib_tf_amd.court_ultra import Courtemanche as CourtemancheUltra
    from fib_tf_amd.fenton import Fenton4v
    from fib_tf_amd.ionic import IonicModel
    nvar = {Fenton4v: 4, BeelerReuter: 8, Courtemanche: 21, CourtemancheUltra: 21}
    for cls, n in nvar.items():
        var, var2, a0, b0 = cls.tip_signals
        assert var == 0 and 0 < var2 < n and np.isfinite([a0, b0]).all()
        assert 'tip_signals' in vars(cls)                           # each model states its own
    assert Fenton4v.tip_signals[1] == 1
    m = stub_model()
    with m.record_tips(every=2) as rec:
        assert (rec.var, rec.var2, rec.levels) == (0, 1, Fenton4v.tip_signals[2:])
        t = m._stepper.tip
        assert (t['var'], t['var2'], t['a0'], t['b0'], t['every'], t['max'], t['cap']) == (0, 1) + Fenton4v.tip_signals[2:] + (2, 256, 6)
    with m.record_tips(var2=2, levels=(0.1, 0.2), capacity=3, max_tips=8) as rec:
        assert (rec.var2, rec.levels, rec.capacity, rec.max_tips) == (2, (0.1, 0.2), 3, 8)
    with pytest.raises(ValueError, match='pass levels'):
        m.record_tips(var2=2)                                       # the model's level belongs to array 1

    class Bare(IonicModel):
        pass
    bare = stub_model(cls=Bare)
    with pytest.raises(ValueError, match='tip_signals'):
        bare.record_tips()
    with pytest.raises(ValueError, match='tip_signals'):
        bare.record_tips(var2=1)
    with bare.record_tips(var2=1, levels=(0, 0)) as rec:
        assert rec.levels == (0.0, 0.0)
    with pytest.raises(ValueError, match='every'):
        m.record_tips(every=0)
    with pytest.raises(AssertionError, match='after calling define'):
        Fenton4v({'height': 8, 'width': 8, 'dt': 0.1, 'diff': 1.0}).record_tips()


# ---- link ------------------------------------------------------------------------------------------------------------
def sample(t, tips):
    from fib_tf_amd.tips import TIP_DTYPE
    a = np.empty(len(tips), TIP_DTYPE)
    for k, (y, x, c) in enumerate(tips):
        a[k] = (t, y, x, c)
    return a


def test_link_two_counter_rotating_tips():
    from fib_tf_amd import tips
    per = [sample(float(s), [(8.5, 10.5 + s, 1), (9.5, 12.5 - 0.5 * s, -1)]) for s in range(6)]      # they pass close by each other
    tr = tips.link(per, max_jump=1.5)
    assert [t.charge for t in tr] == [1, -1] and [len(t.points) for t in tr] == [6, 6]
    assert tr[0].points.dtype.names == ('t_ms', 'y', 'x')
    assert tr[0].points['x'].tolist() == [10.5 + s for s in range(6)] and tr[0].points['t_ms'].tolist() == [0., 1., 2., 3., 4., 5.]
    assert tr[1].points['x'].tolist() == [12.5 - 0.5 * s for s in range(6)] and np.all(tr[1].points['y'] == 9.5)


def test_link_ends_and_starts_trajectories():
    from fib_tf_amd import tips
    per = [sample(0., [(5.5, 5.5, 1), (20.5, 20.5, -1)]),
           sample(1., [(5.5, 6.5, 1), (20.5, 21.5, -1)]),
           sample(2., [(5.5, 7.5, 1)]),                            # the -1 tip has vanished: its trajectory ends
           sample(3., [(5.5, 12.5, 1)]),                           # a jump of 5 > max_jump: a new trajectory
           sample(4., [(5.5, 13.5, 1), (5.5, 14.5, -1)]),          # the other charge never continues a trajectory
           sample(5., [])]
    tr = tips.link(per, max_jump=2.0)
    assert [(t.charge, t.points['t_ms'].tolist()) for t in tr] == [(1, [0., 1., 2.]), (-1, [0., 1.]), (1, [3., 4.]), (-1, [4.])]
    assert tips.link([], 1.0) == [] and tips.link([sample(0., [])], 1.0) == []
    # greedy by distance: the closest pair is linked first, the tip left over starts a trajectory of its own
    per = [sample(0., [(0.5, 0.5, 1), (0.5, 3.5, 1)]), sample(1., [(0.5, 2.5, 1)])]
    tr = tips.link(per, max_jump=2.5)
    assert [t.points['x'].tolist() for t in tr] == [[0.5], [3.5, 2.5]]


# ---- row blocks ------------------------------------------------------------------------------------------------------
def _sharded_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from cpu_engine import OracleEngine
        import fib_tf_amd.sharded as sharded
        from fib_tf_amd.fenton import Fenton4v

        class CpuShardedStepper(sharded.ShardedStepper):
            def __init__(self, *a, **kw):
                kw['engine_factory'] = OracleEngine
                kw.pop('library', None)
                super().__init__(*a, **kw)
        sharded.ShardedStepper = CpuShardedStepper
        m = Fenton4v({'height': 64, 'width': 16, 'dt': 0.1, 'diff': 1.0, 'duration': 1, 'halo_ticks': 1})
        m.define()
        try:
            m.record_tips()
            msg = 'no error'
        except NotImplementedError as e:
            msg = 'NotImplementedError: %s' % e
        with open(os.path.join(outdir, 'rank%d.txt' % rank), 'w') as f:
            f.write(msg)
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_row_blocks_refused(tmp_path):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    for p in procs:
        if p.is_alive():
            p.kill()
            pytest.fail('rank hung')
        assert p.exitcode == 0
    for r in range(2):
        msg = open(os.path.join(str(tmp_path), 'rank%d.txt' % r)).read()
        assert msg.startswith('NotImplementedError') and 'single device' in msg and '2 ranks' in msg, msg
