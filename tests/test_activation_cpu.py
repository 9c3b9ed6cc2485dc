"""not-gpu: the activation recorder's semantics (include/fibhip.h fibhip_observe_*) on synthetic traces through the NumPy
restatement (tests/activation_ref.py), the public API's defaults and helpers, and its refusal on row blocks (gloo ranks
over the CPU test engine)."""
import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from activation_ref import ActivationRef, bit_equal  # noqa: E402

NAN = np.float32(np.nan)


def run(trace, up=0.5, down=0.1, dt=0.1, spt=10):
    """trace: [ticks + 1] values of one cell, the first at attach time"""
    tr = np.asarray(trace, np.float32).reshape(-1, 1, 1)
    r = ActivationRef(tr[0], up, down, dt, spt)
    for v in tr[1:]:
        r.step(v)
    return {k: v[0, 0] for k, v in r.maps().items()}


def test_one_beat_interpolated_in_float32():
    m = run([0.0, 0.2, 0.8, 1.0, 0.6, 0.05])
    tick = np.float32(0.1 * 10)
    t_up = np.float32(1.0) + ((np.float32(0.5) - np.float32(0.2)) / (np.float32(0.8) - np.float32(0.2))) * tick
    t_dn = np.float32(4.0) + ((np.float32(0.6) - np.float32(0.1)) / (np.float32(0.6) - np.float32(0.05))) * tick
    assert m['count'] == 1
    assert m['first_up'] == t_up and m['last_up'] == t_up and np.isnan(m['prev_up'])
    assert m['apd'] == np.float32(t_dn - t_up)


def test_ramp_exactly_at_threshold():
    # Vc == up is an upstroke (Vc >= up) at the very end of the tick; Vp == up afterwards is not below up: no second one
    m = run([0.0, 0.5, 0.5, 1.0])
    assert m['count'] == 1 and m['first_up'] == np.float32(1.0)
    # Vp == down is a downstroke start (Vp >= down); Vc == down is not below it
    m = run([0.0, 1.0, 0.1, 0.1, 0.0])
    assert m['count'] == 1 and m['apd'] == np.float32(3.0) - np.float32(0.5)


def test_two_beats_cycle_length_and_last_apd():
    m = run([0, 1, 0, 0, 1, 1, 0], spt=1, dt=1.0)
    assert m['count'] == 2
    assert m['first_up'] == np.float32(0.5) and m['prev_up'] == np.float32(0.5) and m['last_up'] == np.float32(3.5)
    assert m['last_up'] - m['prev_up'] == 3.0
    # downstroke through 0.1 between ticks 5 and 6: t = 5 + 0.9 / 1 = 5.9; apd of the second beat
    assert m['apd'] == np.float32(np.float32(5.0) + np.float32(0.9)) - np.float32(3.5)


def test_downstroke_before_any_upstroke_records_nothing():
    m = run([1.0, 0.0, 0.0], spt=1, dt=1.0)          # attached during a beat: the fall has no upstroke to belong to
    assert m['count'] == 0 and np.isnan(m['apd']) and np.isnan(m['first_up'])


def test_nan_inputs_record_nothing():
    m = run([0.0, NAN, 1.0, NAN, 0.0], spt=1, dt=1.0)
    assert m['count'] == 0 and all(np.isnan(m[k]) for k in ('first_up', 'last_up', 'prev_up', 'apd'))
    m = run([NAN, 0.0, 1.0], spt=1, dt=1.0)          # a NaN at attach time is simply the first Vp
    assert m['count'] == 1 and m['first_up'] == np.float32(1.5)


def test_time_origin_is_float_of_double_product():
    r = ActivationRef(np.zeros((1, 1), np.float32), 0.5, 0.1, 0.1, 10)
    for _ in range(123):
        r.step(np.zeros((1, 1), np.float32))
    r.step(np.ones((1, 1), np.float32))
    t0 = np.float32(123.0 * 0.1 * 10)
    assert r.maps()['last_up'][0, 0] == t0 + np.float32(0.5) * np.float32(1.0)


def test_maps_grid_and_bit_equal():
    rng = np.random.default_rng(3)
    frames = rng.random((40, 8, 9)).astype(np.float32)
    r = ActivationRef(frames[0], 0.5, 0.1, 0.1, 5)
    for f in frames[1:]:
        r.step(f)
    m = r.maps()
    assert set(m) == {'first_up', 'last_up', 'prev_up', 'apd', 'count'}
    assert all(v.shape == (8, 9) for v in m.values())
    assert m['count'].dtype == np.int32 and m['count'].min() > 0
    assert bit_equal(m['last_up'], r.maps()['last_up'])
    assert not bit_equal(m['last_up'], m['prev_up'])
    assert np.all(m['last_up'] >= m['first_up'])


def test_default_thresholds():
    from fib_tf_amd.activation import default_thresholds
    assert default_thresholds(0.0, 1.0) == (np.float32(0.5), np.float32(0.1))          # Fenton 4v
    assert default_thresholds(-90.0, 30.0) == (np.float32(-30.0), np.float32(-78.0))   # Beeler-Reuter
    assert default_thresholds(-100.0, 50.0) == (np.float32(-25.0), np.float32(-85.0))  # Courtemanche


def test_record_activation_needs_define():
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': 8, 'width': 8, 'dt': 0.1, 'diff': 1.0})
    with pytest.raises(AssertionError, match='after calling define'):
        m.record_activation()


def test_conduction_velocity_helper():
    from fib_tf_amd.activation import conduction_velocity
    t = np.full((3, 50), np.nan, np.float32)
    t[1, :] = 5.0 + np.arange(50) / 0.8                  # a front at 0.8 px/ms, left to right
    assert abs(conduction_velocity(t, 1, 10, 40) - 0.8) < 1e-5
    assert abs(conduction_velocity(t[:, ::-1], 1, 10, 40) - 0.8) < 1e-5    # right to left: unsigned
    t[1, 20] = np.nan
    assert abs(conduction_velocity(t, 1, 10, 40) - 0.8) < 1e-5
    assert np.isnan(conduction_velocity(t, 0, 0, 50))


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
            m.record_activation()
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
