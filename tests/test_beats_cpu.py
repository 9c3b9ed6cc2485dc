"""the beat recorder's definition (tests/beat_ref.py) on literal sample sequences and literal rings, against the activation
recorder's restatement at every = 1, and on a paced sheet computed by the CPU oracle; the Python layer's orderings and refusals.
No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beat_ref as ref  # noqa: E402
from activation_ref import ActivationRef, bit_equal  # noqa: E402

from fib_tf_amd import beats as bt  # noqa: E402

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP, DOWN = F32(0.5), F32(0.1)
nan, inf = np.nan, np.inf


def run(x0, seq, depth=4, every=1, up=UP, down=DOWN):
    """one pixel: attached at x0, fed `seq`; dt = 0.1, 10 sub-steps per tick: step = `every` ms"""
    r = ref.Beats(np.array([x0], F32), up, down, depth, every, 0.1, 10)
    for v in seq:
        r.sample(np.array([v], F32))
    return r


def ring(r):
    """(t_up, t_down, peak) of the one pixel as lists in slot order, NaN as None"""
    return tuple([None if v != v else float(v) for v in plane[:, 0]] for plane in (r.t_up, r.t_down, r.peak))


def test_header_constants_match_the_binding():
    from fib_tf_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(FIBHIP_BEATS_\w+)\s+(\d+)', hdr)}
    assert defs == {'FIBHIP_BEATS_MAX_DEPTH': 16}
    assert _lib.BEATS_MAX_DEPTH == 16 and bt.MAX_DEPTH == 16
    for name in ('begin', 'count', 'shape', 'read', 'summary', 'end'):
        assert 'fibhip_beats_' + name in _lib.SYMBOLS and re.search(r'\bint fibhip_beats_%s\(' % name, hdr)
    assert _lib.FRAME_REDUCE == ('point', 'mean')            # the recorder's `reduce` is the frame recorder's enum


def test_a_sample_exactly_at_a_level():
    # exactly `up` is an upstroke (>=), at the end of its interval; staying there is none; exactly `down` is NOT a downstroke
    # (<), the step below it is one, at the start of its interval
    r = run(0.0, [0.5, 0.5, 0.1, 0.05])
    assert ring(r) == ([1.0, None, None, None], [3.0, None, None, None], [0.5, None, None, None])
    assert r.n[0] == 1 and np.isnan(r.pk[0]) and r.xp[0] == F32(0.05)
    # xp exactly `up` is not below it: no upstroke from there
    assert run(0.5, [0.9]).n[0] == 0
    # the interpolation, every operation in float32
    r = run(0.0, [0.0, 0.75], every=3)
    assert r.step == F32(3.0) and r.t_up[0, 0] == F32(3.0) + ((UP - F32(0)) / (F32(0.75) - F32(0))) * F32(3.0)


def test_nan_and_inf_samples():
    # NaN is no event and leaves pk alone; the sample behind it compares with NaN and is no event either
    r = run(0.0, [0.8, nan, 0.05])
    assert r.n[0] == 1 and r.pk[0] == F32(0.8) and np.isnan(r.t_down[0, 0])      # NaN -> 0.05 is no downstroke: the beat stays open
    r.sample(np.array([0.0], F32))
    assert np.isnan(r.t_down[0, 0]) and r.pk[0] == F32(0.8)                      # 0.05 -> 0.0: xp < down, no downstroke
    r = run(0.0, [nan, 0.8, nan, 0.9, 0.05])                                     # NaN -> 0.8 is no upstroke either
    assert r.n[0] == 0 and np.isnan(r.pk[0]) and np.isnan(r.t_up).all()
    r = run(0.0, [0.8, nan, 0.9, 0.05])                                          # the peak goes on behind the NaN
    assert r.t_down[0, 0] == F32(3.0) + ((F32(0.9) - DOWN) / (F32(0.9) - F32(0.05))) * F32(1.0) and r.peak[0, 0] == F32(0.9)
    # +inf: an upstroke at the start of its interval ((up - xp) / inf = 0), pk = inf; the fall from it has no time (inf / inf)
    r = run(0.0, [inf, 0.0])
    assert r.t_up[0, 0] == 0.0 and r.peak[0, 0] == inf and np.isnan(r.t_down[0, 0]) and r.n[0] == 1 and np.isnan(r.pk[0])
    # -inf: a downstroke at the start of its interval, then an upstroke without a time
    r = run(0.0, [0.8, -inf, 0.8])
    assert r.t_down[0, 0] == F32(1.0) and r.n[0] == 2 and np.isnan(r.t_up[1, 0]) and r.pk[0] == F32(0.8)
    nused, apd_mean, cl_mean, apd_alt = r.summary(4)
    assert nused[0] == 1 and np.isnan(cl_mean[0]) and np.isnan(apd_alt[0])        # a time that is no number is no term


def test_an_upstroke_inside_an_open_beat():
    r = run(0.0, [0.8, 0.3, 0.9, 0.95, 0.0])
    tu, td, pe = ring(r)
    assert r.n[0] == 2 and td[0] is None and pe[0] == float(F32(0.8))            # it never finished; its peak was kept
    assert tu[1] is not None and td[1] is not None and pe[1] == float(F32(0.95))
    assert r.summary(4)[0][0] == 1                                                # one beat with an APD


def test_a_second_dip_without_an_upstroke():
    r = run(0.0, [0.8, 0.05, 0.2, 0.05, 0.3, 0.0])
    tu, td, pe = ring(r)
    assert r.n[0] == 1 and td[0] == float(F32(1.0) + ((F32(0.8) - DOWN) / (F32(0.8) - F32(0.05))) * F32(1.0)) and pe[0] == float(F32(0.8))
    assert np.isnan(r.pk[0])


def beat_train(k):
    """k beats of four samples each: up to 0.6 + 0.01 b, down to 0"""
    seq = []
    for b in range(k):
        seq += [0.6 + 0.01 * b, 0.3, 0.0, 0.0]
    return seq


def test_the_ring_wraps_around():
    r = run(0.0, beat_train(5), depth=2)
    assert r.n[0] == 5
    tu, td, pe = ring(r)                                                          # beats 4 and 3 in slots 0 and 1
    assert tu == [float(F32(16) + (UP / F32(0.64)) * F32(1)), float(F32(12) + (UP / F32(0.63)) * F32(1))]
    assert pe == [float(F32(0.64)), float(F32(0.63))] and td[0] is not None and td[1] is not None
    o = bt.order_ring(*r.read())
    assert o['t_up'][:, 0].tolist() == [tu[1], tu[0]] and o['count'][0] == 5      # index -1 is the newest
    full = run(0.0, beat_train(5), depth=8)
    assert bt.order_ring(*full.read())['t_up'][-2:, 0].tolist() == [tu[1], tu[0]]
    assert np.isnan(bt.order_ring(*full.read())['t_up'][:3, 0]).all()


def test_depth_one():
    r = run(0.0, beat_train(3) + [0.7], depth=1)
    assert r.n[0] == 4 and r.t_up.shape == (1, 1) and r.t_up[0, 0] == F32(12) + (UP / F32(0.7)) * F32(1)
    assert np.isnan(r.t_down[0, 0]) and np.isnan(r.peak[0, 0]) and r.pk[0] == F32(0.7)
    # an upstroke inside an open beat: the old beat's peak goes into the one slot and the new beat clears it
    r.sample(np.array([0.2], F32))
    r.sample(np.array([0.9], F32))
    assert r.n[0] == 5 and np.isnan(r.peak[0, 0]) and r.pk[0] == F32(0.9)
    assert bt.order_ring(*r.read())['peak'][0, 0] == F32(0.9)                     # the open beat's peak is the running one
    assert [m[0] for m in r.summary(1)][0] == 0


def test_equal_samples_cannot_be_an_event():
    # an event needs xp < up <= xc or xc < down <= xp: xc != xp, so no interpolation divides by zero
    for level in (UP, DOWN, F32(0.3)):
        r = run(level, [level] * 3)
        assert r.n[0] == 0 and np.isnan(r.t_up).all()
    r = run(0.0, [0.8, 0.1, 0.1, 0.1])                                            # an open beat resting exactly at `down`
    assert np.isnan(r.t_down).all() and r.pk[0] == F32(0.8)
    rng = np.random.default_rng(5)
    x = rng.choice(np.array([0.0, 0.1, 0.3, 0.5, 0.8], F32), (200, 50))
    r = ref.Beats(x[0], UP, DOWN, 16, 1, 0.1, 10)
    for v in x[1:]:
        r.sample(v)
    assert r.n.sum() > 100 and np.isfinite(r.t_up[r.t_up == r.t_up]).all() and np.isfinite(r.t_down[r.t_down == r.t_down]).all()


def test_the_summary_walk_on_literal_rings():
    # depth 4, six beats: beats 2 .. 5 are held, in slots 2, 3, 0, 1
    t_up = np.array([400, 500, 200, 300], F32).reshape(4, 1)
    t_down = np.array([450, 570, 260, 340], F32).reshape(4, 1)                    # APDs of beats 2 .. 5: 60, 40, 50, 70
    n = np.array([6], np.int32)
    nu, am, cm, al = ref.summary(t_up, t_down, n, 4)
    assert nu[0] == 4 and am[0] == F32(220) / F32(4) and cm[0] == F32(100)
    # pairs (2,3): d = -20, b = 3 odd: -20; (3,4): d = 10, even: -10; (4,5): d = 20, odd: 20 -> -10 / 3
    assert al[0] == F32(F32(-20) + F32(-10) + F32(20)) / F32(3)
    nu, am, cm, al = ref.summary(t_up, t_down, n, 2)                              # beats 4 and 5
    assert nu[0] == 2 and am[0] == F32(60) and cm[0] == F32(100) and al[0] == F32(20)
    nu, am, cm, al = ref.summary(t_up, t_down, n, 1)                              # one beat: an APD, no pair
    assert nu[0] == 1 and am[0] == F32(70) and np.isnan(cm[0]) and np.isnan(al[0])
    # a beat that never finished breaks the alternans pairs on both sides and is no APD term; its t_up still counts for cl
    t_down[3, 0] = nan                                                            # beat 3
    nu, am, cm, al = ref.summary(t_up, t_down, n, 4)
    assert nu[0] == 3 and am[0] == F32(F32(60) + F32(50) + F32(70)) / F32(3) and cm[0] == F32(100) and al[0] == F32(20)
    # fewer beats than `last`, and none
    nu, am, cm, al = ref.summary(t_up, t_down, np.array([1], np.int32), 4)        # beat 0 in slot 0
    assert nu[0] == 1 and am[0] == F32(50) and np.isnan(cm[0]) and np.isnan(al[0])
    nu, am, cm, al = ref.summary(t_up, t_down, np.array([0], np.int32), 4)
    assert nu[0] == 0 and np.isnan(am[0]) and np.isnan(cm[0]) and np.isnan(al[0])
    # the sums are float32 sums in ascending order from the first term
    t_up = np.zeros((4, 1), F32)
    t_down = np.array([2 ** 25, 1, 1, 1], F32).reshape(4, 1)
    assert ref.summary(t_up, t_down, np.array([4], np.int32), 4)[1][0] == F32(2 ** 25) / F32(4)
    # perfect alternans: long on the even beats, short on the odd ones -> negative, of magnitude |long - short|
    t_up = np.array([0, 100, 200, 300], F32).reshape(4, 1)
    t_down = t_up + np.array([60, 40, 60, 40], F32).reshape(4, 1)
    assert ref.summary(t_up, t_down, np.array([4], np.int32), 4)[3][0] == F32(-20)
    assert ref.summary(t_up, t_down + np.array([0, 20, 0, 20], F32).reshape(4, 1), np.array([4], np.int32), 4)[3][0] == 0


def test_orderings_and_refusals_of_the_python_layer():
    t_up = np.arange(8, dtype=F32).reshape(4, 2) + 1                              # slot order; pixel 0: 3 beats, pixel 1: 6
    t_down = t_up + F32(0.5)
    peak = t_up * 0
    count = np.array([3, 6], np.int32)
    pk = np.array([nan, 0.75], F32)
    o = bt.order_ring(t_up, t_down, peak, count, pk)
    assert np.isnan(o['t_up'][0, 0]) and o['t_up'][1:, 0].tolist() == [1, 3, 5]   # beats 0, 1, 2 in slots 0, 1, 2
    assert o['t_up'][:, 1].tolist() == [6, 8, 2, 4]                               # beats 2 .. 5 in slots 2, 3, 0, 1
    assert o['peak'][-1, 1] == F32(0.75) and o['peak'][-1, 0] == 0 and o['t_up'].dtype == F32 and o['count'].dtype == np.int32
    assert bt.apd_of(o).dtype == np.float64 and bt.apd_of(o)[-1].tolist() == [0.5, 0.5]
    assert np.isnan(bt.cl_of(o)[0]).all() and bt.cl_of(o)[1:, 1].tolist() == [2, -6, 2]
    assert bt.di_of(o)[2:, 0].tolist() == [1.5, 1.5] and np.isnan(bt.di_of(o)[:2, 0]).all()
    di, apd = bt.restitution_of(o)
    assert len(di) == len(apd) == 2 + 3 and (apd == 0.5).all()
    di, apd = bt.restitution_of(o, mask=np.array([True, False]))
    assert di.tolist() == [1.5, 1.5]
    with pytest.raises(ValueError):
        bt.restitution_of(o, mask=np.ones((3,), bool))
    ok = dict(every=1, depth=8, up=0.5, down=0.1, block=(1, 1), reduce='mean')
    bt.check_args(**ok)
    bt.check_args(**dict(ok, down=0.5))
    for bad in (dict(every=0), dict(depth=0), dict(depth=17), dict(down=0.6), dict(up=nan), dict(reduce='max'), dict(block=(0, 1)),
                dict(block=(1, 17))):
        with pytest.raises(ValueError):
            bt.check_args(**dict(ok, **bad))
    up, down = bt.default_levels(-85.0, 25.0)
    assert up == F32(-30.0) and down == F32(-74.0)
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'width': 16, 'height': 16, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.5, 'duration': 10})
    with pytest.raises(AssertionError):
        m.record_beats()                                     # before define()


def test_against_the_activation_recorder_at_every_tick():
    """every = 1, full resolution: on an input where no cell dips below `down` twice without an upstroke in between, the count
    is the activation recorder's, the newest t_up its last_up, and the newest finished beat's t_down - t_up its apd, bit for bit"""
    H, W, K, D = 24, 40, 260, 16
    rng = np.random.default_rng(24)
    period = rng.uniform(40, 90, (H, W))
    phase = rng.uniform(0, 1, (H, W))
    amp = rng.uniform(0.45, 0.7, (H, W))
    frames = [(0.45 + amp * np.sin(2 * np.pi * (k / period + phase))).astype(F32) for k in range(K + 1)]
    # the condition, on the input itself: between two downstrokes of a cell there is an upstroke
    dipped = np.zeros((H, W), bool)
    for a, b in zip(frames, frames[1:]):
        rise, fall = (a < UP) & (b >= UP), (a >= DOWN) & (b < DOWN)
        assert not (fall & dipped).any()
        dipped = (dipped | fall) & ~rise
    act = ActivationRef(frames[0], UP, DOWN, 0.1, 10)
    r = ref.Beats(frames[0], UP, DOWN, D, 1, 0.1, 10)
    assert r.step.tobytes() == act.tick.tobytes()
    for f in frames[1:]:
        act.step(f)
        r.sample(f)
    want = act.maps()
    o = bt.order_ring(*r.read()[:4])
    assert want['count'].max() < D and want['count'].min() >= 2
    assert np.array_equal(o['count'], want['count']) and bit_equal(o['t_up'][-1], want['last_up']) and bit_equal(o['t_up'][-2], want['prev_up'])
    apd = o['t_down'] - o['t_up']
    assert apd.dtype == F32
    done = apd == apd
    newest = (D - 1) - np.argmax(done[::-1], axis=0)          # the newest beat that has finished
    got = np.where(done.any(axis=0), np.take_along_axis(apd, newest[None], axis=0)[0], F32(nan))
    assert bit_equal(got, want['apd'])
    still_open = ~done[-1]
    assert 0 < still_open.sum() < H * W and (r.pk == r.pk)[still_open].all()      # both kinds of cell were there


# Measured on the oracle (the test prints the figures): by the bound below the sheet is steady from the very first cycle
# length on — beat 1 against beat 0, which started from rest: the largest |cl - 300 ms| over the sheet is 4.101 ms there, then
# 0.078, 0.014, 0.003 and below 0.001 ms for beats 2 .. 7.  The first wave needs 14.68 ms to reach the far edge.
STEADY_FROM = 1


def test_paced_sheet_one_beat_per_pace():
    """Fenton 64 x 64 from rest, columns 0-5 paced to 1.0 every 300 ticks (tests/test_spectrum_cpu.py's sheet, which captures
    1:1); a sample every 10 ticks of 1 ms, a ring of 8 beats"""
    import oracle
    H = W = 64
    every, ticks, tick_ms = 10, 2400, 1.0
    slab = np.zeros((4, H, W), F32)
    slab[1] = slab[2] = 1
    r = ref.Beats(ref.pixel(slab[0]), UP, DOWN, 8, every, 0.1, 10)
    paces = []
    for k in range(ticks):
        oracle.fenton_run(slab, 0.1, 1.5, None, 10)
        if (k + 1) % every == 0:
            r.sample(ref.pixel(slab[0]))
        if k % 300 == 0:
            slab[0] = oracle.pace(slab[0], 0, H, 0, 6, 1.0, 0.0)
            paces.append((k + 1) * tick_ms)                  # delivered right after tick k + 1
    o = bt.order_ring(*r.read())
    t_up = o['t_up'].astype(np.float64)
    assert len(paces) == 8 and np.isfinite(t_up).all()
    transit = float((t_up[0] - paces[0]).max())              # the first wave's arrival at the cell it reaches last
    assert 0 < transit < 300 * tick_ms
    delivered = sum(p + transit <= ticks * tick_ms for p in paces)
    assert delivered == 8 and (o['count'] == delivered).all()                    # 1:1, every cell
    # every upstroke time lies in a sample interval behind its pace, and every beat but the one in progress has finished
    for b, p in enumerate(paces):
        assert (t_up[b] >= p - 1).all() and (t_up[b] <= p + transit + every * tick_ms).all()
    apd = bt.apd_of(o)
    assert np.isfinite(apd).all() and (apd > 50).all() and (apd < 300 - transit).all()      # the eighth has finished too
    cl = bt.cl_of(o)
    dev = np.abs(cl[1:] - 300 * tick_ms).reshape(7, -1).max(axis=1)
    print('largest |cl - 300 ms| per beat 1 .. 7:', np.round(dev, 3).tolist(), 'transit %.2f ms' % transit)
    assert (dev[STEADY_FROM - 1:] <= 2 * every * tick_ms).all()
    di, a = bt.restitution_of(o)
    assert len(di) == 7 * H * W and (di > 0).all()           # beats 1 .. 7 have a DI in front and an APD
    nu, am, cm, al = r.summary(4)
    assert (nu == 4).all() and (np.abs(cm - 300) <= 2 * every * tick_ms).all()   # beats 4 .. 7
    assert (np.abs(al) <= 2 * every * tick_ms).all()         # no alternans at this rate
