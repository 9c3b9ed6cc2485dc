"""not-gpu: the velocity fit (include/fibhip.h fibhip_beats_velocity / fibhip_observe_velocity / fibhip_velocity_fit,
fib_tf_amd/velocity.py) without a device: the NumPy restatement of tests/velocity_ref.py on synthetic rings where every quantity
is exact, the host's helpers, the refusals that need no device, the header and the bindings' argument forms."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import velocity_ref as ref  # noqa: E402
import test_stepper_bindings_cpu as tb  # noqa: E402

from fib_tf_amd import _lib, beats as bt, velocity as vel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
nan = np.nan


def plane_ring(oh, ow, depth, sy=0.75, sx=-1.25, period=64.0, beats=None):
    """beat b of every pixel at t = sy * y + sx * x + period * b, shifted to stay >= 0: dyadic, exact in float32; `beats` beats in
    a ring of `depth` slots (slot b % depth holds the newest beat that maps to it)"""
    y, x = np.mgrid[:oh, :ow]
    base = sy * y + sx * x
    base = base - base.min()
    beats = depth if beats is None else beats
    t = np.full((depth, oh, ow), nan, F32)
    for b in range(beats):
        t[b % depth] = (base + period * b).astype(F32)
    assert np.array_equal(t[np.isfinite(t)], t[np.isfinite(t)].astype(np.float64).astype(F32))
    return t, np.full((oh, ow), beats, np.int32)


def test_a_dyadic_plane_is_recovered_exactly():
    oh, ow = 24, 40
    t, n = plane_ring(oh, ow, 3)
    assert t.max() < 256
    for back in (0, 1, 2):
        nfit, gy, gx, rms = ref.fit(t, n, back=back, radius=2, max_dt=20.0)
        assert nfit.dtype == np.int32 and gy.dtype == gx.dtype == rms.dtype == F32
        fitted = nfit >= ref.default_min_cells(2)
        assert fitted.sum() > 0.9 * oh * ow
        assert (gy[fitted] == F32(0.75)).all() and (gx[fitted] == F32(-1.25)).all() and (rms[fitted] == 0).all()
        # a corner has 9 of the 25 cells: fewer than the default 13
        for cy, cx in ((0, 0), (0, ow - 1), (oh - 1, 0), (oh - 1, ow - 1)):
            assert nfit[cy, cx] == 9 and np.isnan(gy[cy, cx]) and np.isnan(gx[cy, cx]) and np.isnan(rms[cy, cx])
        assert nfit[oh // 2, ow // 2] == 25 and nfit[0, ow // 2] == 15
    # with min_cells = 9 the corners fit too
    nfit, gy, gx, rms = ref.fit(t, n, radius=2, max_dt=20.0, min_cells=9)
    assert (gy == F32(0.75)).all() and (gx == F32(-1.25)).all() and (rms == 0).all()


def test_neighbours_are_matched_by_time_not_by_beat_number():
    """per-pixel counts at random in 0 .. depth + 3: beat numbers disagree between neighbours and rings have wrapped; the planar
    wave's gradient comes back wherever the centre holds the beat and enough neighbours hold the wave it belongs to"""
    oh, ow, depth = 24, 40, 4
    rng = np.random.default_rng(3)
    y, x = np.mgrid[:oh, :ow]
    base = 0.75 * y - 1.25 * x
    base = base - base.min()
    n = rng.integers(0, depth + 4, (oh, ow)).astype(np.int32)
    # every pixel saw the waves 0 .. 6 but missed the first 7 - n of them: its beat b is wave b + 7 - n
    t = np.full((depth, oh, ow), nan, F32)
    for b in range(depth + 3):
        held = (b < n) & (b >= n - depth)
        t[b % depth] = np.where(held, (base + 32.0 * (b + 7 - n)).astype(F32), t[b % depth])
    for back in (0, 1):
        nfit, gy, gx, rms = ref.fit(t, n, back=back, radius=2, max_dt=15.0, min_cells=6)
        centre = back < np.minimum(n, depth)
        assert (nfit[~centre] == 0).all() and np.isnan(gy[~centre]).all()
        fitted = np.isfinite(gy)
        print('back %d: a fit at %d of the %d pixels whose centre holds the beat' % (back, fitted.sum(), centre.sum()))
        assert fitted.sum() > 0.95 * centre.sum()
        assert (gy[fitted] == F32(0.75)).all() and (gx[fitted] == F32(-1.25)).all() and (rms[fitted] == 0).all()


def test_one_line_has_no_plane():
    t, n = plane_ring(1, 7, 1)
    nfit, gy, gx, rms = ref.fit(t, n, radius=2, max_dt=20.0, min_cells=3)
    assert nfit.tolist() == [[3, 4, 5, 5, 5, 4, 3]] and np.isnan(gy).all() and np.isnan(gx).all() and np.isnan(rms).all()
    t, n = plane_ring(9, 9, 1)
    mask = np.zeros((9, 9), np.uint8)
    mask[:, 4] = 1                                           # one column is left
    (nfit, gy, gx, rms), seen = ref.fit(t, n, radius=2, max_dt=20.0, min_cells=3, mask=mask, trace=True)
    assert (nfit[:, 4] == [3, 4, 5, 5, 5, 5, 5, 4, 3]).all() and (nfit[:, :4] == 0).all() and np.isnan(gy).all()
    assert seen['refused_for_det'] == 9 and seen['centre_missing'] == 72 and seen['fitted'] == 0


def ring_of(values, centre):
    """a 3 x 3 plane, depth len(values): the middle pixel's neighbour to the right holds `values` as its beats, every other
    pixel the plane t = centre + 2 * dy + dx in all its slots' newest beat"""
    depth = len(values)
    y, x = np.mgrid[:3, :3]
    t = np.repeat((centre + 2.0 * (y - 1) + (x - 1)).astype(F32)[None], depth, axis=0)
    t[:, 1, 2] = values
    return t, np.full((3, 3), depth, np.int32)


def test_a_tie_keeps_the_older_beat():
    t, n = ring_of([10.0, 18.0], 14.0)                       # |d| = 4 twice: the older beat, d = -4, is kept
    older = ref.fit(t, n, back=0, radius=1, max_dt=8.0, min_cells=3)
    t2, _ = ring_of([10.0, 100.0], 14.0)
    alone = ref.fit(t2, n, back=0, radius=1, max_dt=8.0, min_cells=3)
    assert all(a[1, 1].tobytes() == b[1, 1].tobytes() for a, b in zip(older, alone))        # (at the middle pixel: the neighbour's own fit differs)
    t3, _ = ring_of([100.0, 18.0], 14.0)
    newer = ref.fit(t3, n, back=0, radius=1, max_dt=8.0, min_cells=3)
    assert older[0][1, 1] == newer[0][1, 1] == 9 and older[2][1, 1] != newer[2][1, 1]
    _, seen = ref.fit(t, n, back=0, radius=1, max_dt=8.0, min_cells=3, trace=True)
    assert seen['ties'] > 0


def test_max_dt_itself_is_used_and_nothing_beyond():
    t, n = ring_of([22.0], 14.0)                             # d = 8 == max_dt
    assert ref.fit(t, n, radius=1, max_dt=8.0, min_cells=3)[0][1, 1] == 9
    t, n = ring_of([np.nextafter(F32(22.0), F32(30.0))], 14.0)
    assert ref.fit(t, n, radius=1, max_dt=8.0, min_cells=3)[0][1, 1] == 8


@pytest.mark.parametrize('bad', [nan, np.inf, -np.inf])
def test_times_that_are_no_numbers_are_never_used(bad):
    t, n = ring_of([bad], 14.0)
    nfit, gy, gx, rms = ref.fit(t, n, radius=1, max_dt=8.0, min_cells=3)
    assert nfit[1, 1] == 8 and gy[1, 1] == 2 and gx[1, 1] == 1 and rms[1, 1] == 0
    assert nfit[1, 2] == 0 and np.isnan(gy[1, 2])            # as a centre it has no fit either
    t, n = ring_of([bad, 15.0, bad], 14.0)                   # a number among them is found
    assert ref.fit(t, n, radius=1, max_dt=8.0, min_cells=3)[0][1, 1] == 9


def test_the_crafted_rings_take_every_branch():
    """the inputs of tests/test_gpu_velocity.py's unit-op test: every shape sees centres without a beat; the two large shapes see
    every branch — refused for N, refused for det, fitted, ties —; the line and the point never fit"""
    total = {}
    for shape in ref.CRAFTED_SHAPES:
        seen = {}
        for i, case in enumerate(ref.crafted_cases(shape)):
            if shape[0] * shape[1] > 100 and (case['radius'] in (2, 3) or case['t'].shape[0] == 16):
                continue                                         # (a thinned walk keeps this test quick; the GPU test runs them all)
            _, s = ref.fit(trace=True, **case)
            for k, v in s.items():
                seen[k] = seen.get(k, 0) + v
        print(shape, seen)
        total[shape] = seen
        assert seen['centre_missing'] > 0
    for shape in ((19, 70), (33, 129)):
        assert all(total[shape][k] > 0 for k in ('refused_for_n', 'refused_for_det', 'fitted', 'ties')), total[shape]
    assert total[(1, 1)]['fitted'] == total[(1, 7)]['fitted'] == 0 and total[(1, 7)]['refused_for_det'] > 0
    assert total[(5, 3)]['fitted'] > 0
    t, count, mask = ref.crafted((33, 129), 16, 7)
    assert np.isnan(t).any() and np.isinf(t).any() and (count == 0).any() and (count > 10 ** 9).any() and ((count > 0) & (count < 16)).any()
    assert 0 < mask.sum() < mask.size


# ---- the host's helpers --------------------------------------------------------------------------------------------------
def test_speed_and_direction():
    v = {'gy': np.array([[0.0, 3.0, nan, 0.0]], F32), 'gx': np.array([[0.5, 4.0, 1.0, 0.0]], F32)}
    s = vel.speed_of(v)
    assert s.dtype == np.float64 and s[0, 0] == 2.0 and s[0, 1] == 0.2 and np.isnan(s[0, 2]) and np.isinf(s[0, 3])
    s = vel.speed_of(v, block=(3, 2))                         # pixels of 3 x 2 cells: ms per cell = ms per pixel / cells per pixel
    assert s[0, 0] == 4.0 and s[0, 1] == 1.0 / np.hypot(1.0, 2.0)
    d = vel.direction_of(v)
    assert d[0, 0] == 0.0 and d[0, 1] == np.arctan2(3.0, 4.0)
    assert vel.direction_of({'gy': np.array([1.0]), 'gx': np.array([0.0])})[0] == np.pi / 2
    assert [vel.default_min_cells(r) for r in (1, 2, 3, 4)] == [5, 13, 25, 41]


def test_cv_restitution_pairs_with_the_diastolic_interval():
    oh, ow, depth = 6, 9, 4
    t_up, n = plane_ring(oh, ow, depth, sy=0.5, sx=0.25, period=64.0, beats=6)      # the ring wrapped: beats 2 .. 5
    t_down = (t_up + F32(40.0)).astype(F32)
    t_down[(6 - 1) % depth, 2, 3] = nan                      # the newest beat of one pixel is still open
    beats = bt.order_ring(t_up, t_down, np.zeros_like(t_up), n)
    v = ref.fit_beats(t_up, n, 3, radius=1, max_dt=10.0, min_cells=4)
    assert v['gy'].shape == (3, oh, ow) and (v['gy'] == F32(0.5)).all() and (v['gx'] == F32(0.25)).all()
    di, cv = vel.cv_restitution_of(beats, v, block=(1, 1))
    want_di = bt.di_of(beats)[-3:]
    assert len(di) == len(cv) == int(np.isfinite(want_di).sum()) == 3 * oh * ow          # (the DI in front needs the beat before to be closed)
    assert (di == 24.0).all() and np.allclose(cv, 1.0 / np.hypot(0.5, 0.25), rtol=0, atol=0)
    mask = np.zeros((oh, ow), bool)
    mask[1:3] = True
    assert len(vel.cv_restitution_of(beats, v, (1, 1), mask)[0]) == 3 * 2 * ow
    v['rms'][0] = 1.0
    assert len(vel.cv_restitution_of(beats, v, (1, 1), max_rms=0.5)[0]) == 2 * oh * ow
    v['gy'][-1, 0, 0] = nan
    assert len(vel.cv_restitution_of(beats, v, (2, 2))[0]) == 3 * oh * ow - 1
    with pytest.raises(ValueError):
        vel.cv_restitution_of(beats, v, (1, 1), np.ones((2, 2), bool))


# ---- refusals and interface ----------------------------------------------------------------------------------------------
def test_check_args():
    assert vel.check_args(2, 20.0) == (2, F32(20.0), 13)
    assert vel.check_args(np.int64(4), 5, 81, depth=8, last=8) == (4, F32(5.0), 81)
    for bad in (dict(radius=0), dict(radius=5), dict(max_dt=0.0), dict(max_dt=-1.0), dict(max_dt=nan), dict(max_dt=np.inf), dict(max_dt=1e39),
                dict(min_cells=2), dict(min_cells=26), dict(depth=4, last=0), dict(depth=4, last=5)):
        with pytest.raises(ValueError) as e:
            vel.check_args(**dict(dict(radius=2, max_dt=20.0), **bad))
        assert str(e.value).startswith('velocity: '), bad
    with pytest.raises(ValueError) as e:
        vel.check_args(9, 1.0, who='record')
    assert str(e.value) == 'record: radius must be 1 .. 4 (got 9)'


def test_header_declares_the_three_functions():
    hdr = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    assert re.search(r'^#define FIBHIP_ABI_VERSION 1$', hdr, re.M) and re.search(r'^#define FIBHIP_VEL_MAX_RADIUS 4$', hdr, re.M)
    assert vel.MAX_RADIUS == _lib.VEL_MAX_RADIUS == ref.MAX_RADIUS == 4
    for name, nargs in (('beats_velocity', 10), ('observe_velocity', 10), ('velocity_fit', 15)):
        assert re.search(r'\bint fibhip_%s\(' % name, hdr)
        args, res = _lib.SYMBOLS['fibhip_' + name]
        assert res is C.c_int and len(args) == nargs


class Fake(tb.FakeLibrary):
    def _maps(self, shape, nf, gy, gx, rms):
        return (tb.fill(nf, tb.IP, np.int32, shape, 40),) + tuple(tb.fill(p, tb.FP, np.float32, shape, 41 + i) for i, p in enumerate((gy, gx, rms)))

    def _beats_shape(self, a, b, c):
        return self._shape3(5, a, b, c)

    def _beats_velocity(self, back, radius, max_dt, min_cells, mask, nf, gy, gx, rms):
        return (back, radius, max_dt, min_cells, tb.read(mask, tb.UBP, np.uint8, (tb.OH, tb.OW))) + self._maps((tb.OH, tb.OW), nf, gy, gx, rms)

    def _observe_velocity(self, which, radius, max_dt, min_cells, mask, nf, gy, gx, rms):
        return (which, radius, max_dt, min_cells, tb.read(mask, tb.UBP, np.uint8, (tb.H, tb.W))) + self._maps((tb.H, tb.W), nf, gy, gx, rms)


def fake_stepper():
    st, _ = tb.make()
    st._L = L = Fake()
    return st, L


def test_the_handle_bindings():
    st, L = fake_stepper()
    mask = (np.arange(tb.OH * tb.OW).reshape(tb.OH, tb.OW) % 3).astype(np.int64)
    got = st.beats_velocity(np.int64(2), np.int64(3), 7.3, np.int64(9), mask)
    outs = ('out int32 (3, 4)',) + ('out float32 (3, 4)',) * 3
    tb.calls(L, ('beats_shape', 'ref', 'ref', 'ref'), ('beats_velocity', 2, 3, tb.f32(7.3), 9, mask.astype(np.uint8)) + outs)
    assert type(got) is tuple and len(got) == 4
    tb.back(got[0], 40, np.int32, (tb.OH, tb.OW))
    for i in range(3):
        tb.back(got[1 + i], 41 + i, np.float32, (tb.OH, tb.OW))
    st.beats_velocity(0, 1, 20, 5)
    tb.calls(L, ('beats_shape', 'ref', 'ref', 'ref'), ('beats_velocity', 0, 1, 20.0, 5, None) + outs)
    tb.refused('beats_velocity: a mask of shape (6, 8) on a pixel plane of 3 x 4', st.beats_velocity, 0, 1, 20, 5, np.ones((tb.H, tb.W)))
    tb.calls(L, ('beats_shape', 'ref', 'ref', 'ref'))        # (the shape was asked for; the refused mask reached nothing else)
    big = (np.arange(tb.H * tb.W).reshape(tb.H, tb.W) % 2).astype(bool)
    got = st.observe_velocity('prev_up', 4, 2.5, 41, big)
    outs = ('out int32 (6, 8)',) + ('out float32 (6, 8)',) * 3
    tb.calls(L, ('observe_velocity', 2, 4, 2.5, 41, big.astype(np.uint8)) + outs)
    tb.back(got[0], 40, np.int32, (tb.H, tb.W))
    tb.back(got[3], 43, np.float32, (tb.H, tb.W))
    st.observe_velocity('first_up', 1, 1.0, 3)
    tb.calls(L, ('observe_velocity', 0, 1, 1.0, 3, None) + outs)
    tb.refused('observe_velocity: a mask of shape (3, 4) on a 6 x 8 grid', st.observe_velocity, 'last_up', 1, 1.0, 3, np.ones((3, 4)))


def test_the_unit_op_binding(monkeypatch):
    log = []

    class Unit:
        def fibhip_velocity_fit(self, device, depth, oh, ow, t, count, back, radius, max_dt, min_cells, mask, nf, gy, gx, rms):
            shape = (oh, ow)
            log.append((device, depth, oh, ow, tb.read(t, tb.FP, np.float32, (depth, oh, ow)), tb.read(count, tb.IP, np.int32, shape), back, radius,
                        max_dt, min_cells, tb.read(mask, tb.UBP, np.uint8, shape), tb.fill(nf, tb.IP, np.int32, shape, 50),
                        tb.fill(gy, tb.FP, np.float32, shape, 51), tb.fill(gx, tb.FP, np.float32, shape, 52), tb.fill(rms, tb.FP, np.float32, shape, 53)))
            return 0
    monkeypatch.setattr(_lib, 'lib', lambda: Unit())
    t = (np.arange(2 * 3 * 5).reshape(2, 3, 5) * 0.5).astype(np.float64)
    count = np.arange(15).reshape(3, 5).astype(np.int64)
    mask = np.arange(15).reshape(3, 5) % 4
    got = _lib.velocity_fit(t, count, back=1, radius=3, max_dt=7.3, mask=mask, device=0)
    want = (0, 2, 3, 5, t.astype(F32), count.astype(np.int32), 1, 3, tb.f32(7.3), 25, (mask != 0).astype(np.uint8), 'out int32 (3, 5)') + \
        ('out float32 (3, 5)',) * 3
    assert tb.same(log.pop(), want)
    tb.back(got[0], 50, np.int32, (3, 5))
    tb.back(got[2], 52, np.float32, (3, 5))
    _lib.velocity_fit(t, count, min_cells=4)
    assert tb.same(log.pop()[6:11], (0, 2, 20.0, 4, None))
    with pytest.raises(ValueError):
        _lib.velocity_fit(t, count[:2])
    with pytest.raises(ValueError):
        _lib.velocity_fit(t, count, mask=np.ones((2, 2)))


class Stub:
    """a stepper that answers beats_velocity with maps that name their `back`"""

    def __init__(self):
        self.log = []

    def beats_shape(self):
        return 3, 4, 5

    def beats_begin(self, *a):
        pass

    def beats_end(self):
        pass

    def beats_velocity(self, back, radius, max_dt, min_cells, mask):
        self.log.append((back, radius, max_dt, min_cells, mask))
        return (np.full((3, 4), back, np.int32),) + tuple(np.full((3, 4), back + 0.25 * i, F32) for i in (1, 2, 3))

    def observe_begin(self, *a):
        pass

    def observe_velocity(self, which, radius, max_dt, min_cells, mask):
        self.log.append((which, radius, max_dt, min_cells, mask))
        return (np.zeros((6, 8), np.int32),) + tuple(np.zeros((6, 8), F32) for _ in range(3))


def test_recorder_methods_order_the_beats_newest_last():
    from test_recorder_contract_cpu import Model
    st = Stub()
    rec = bt.BeatRecorder(Model(st), every=2, depth=5, block=(2, 2))
    v = rec.velocity(last=3, radius=1, max_dt=9)
    assert [c[0] for c in st.log] == [0, 1, 2] and st.log[0][1:] == (1, F32(9.0), 5, None)
    assert sorted(v) == ['gx', 'gy', 'nfit', 'rms'] and v['nfit'].dtype == np.int32 and v['gy'].dtype == F32
    assert v['nfit'][:, 0, 0].tolist() == [2, 1, 0] and v['gy'][:, 0, 0].tolist() == [2.25, 1.25, 0.25] and v['rms'][-1, 0, 0] == 0.75
    s = rec.speed(last=2)
    assert s.shape == (2, 3, 4) and s[-1, 0, 0] == 1.0 / np.hypot(0.25 / 2, 0.5 / 2)
    for kw in (dict(last=0), dict(last=6), dict(radius=5), dict(max_dt=0), dict(min_cells=2), dict(mask=np.ones((6, 8)))):
        with pytest.raises(ValueError):
            rec.velocity(**kw)
    mask = np.arange(12).reshape(3, 4) % 2
    rec.velocity(mask=mask)
    assert st.log[-1][4].dtype == np.uint8 and st.log[-1][4].tolist() == mask.tolist()
    rec.close()
    with pytest.raises(AssertionError) as e:
        rec.velocity()
    assert str(e.value) == 'the beat recorder has been closed'
    from fib_tf_amd import activation
    act = activation.ActivationRecorder(Model(st))
    got = act.velocity('prev_up', radius=3, max_dt=4)
    assert st.log[-1] == ('prev_up', 3, F32(4.0), 25, None) and sorted(got) == ['gx', 'gy', 'nfit', 'rms'] and got['nfit'].shape == (6, 8)
    with pytest.raises(ValueError):
        act.velocity('apd')
