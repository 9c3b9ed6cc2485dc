"""not-gpu: the electrode recorder's host side — crop_mask, the declarations of include/fibhip.h and their ctypes
prototypes, the conversion of raw sums into the reference's mean(image() * mask), the sample times of record_on_device,
and the refusal on row blocks (gloo ranks over the CPU test engine)."""
import multiprocessing as mp
import os
import re
import socket
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import electrode_ref as ref  # noqa: E402

NAMES = ('fibhip_electrode_begin', 'fibhip_electrode_count', 'fibhip_electrode_read', 'fibhip_electrode_end')


def _grid(h, w):
    return types.SimpleNamespace(height=h, width=w)


@pytest.mark.parametrize('x,y', [(256, 256), (0, 0), (509, 100), (3, 511)])
def test_crop_mask_is_exact_and_tight(x, y):
    from fib_tf_amd import egm
    mask = egm.create_mask(_grid(512, 512), x, y, 5)
    (r0, r1, c0, c1), patch = egm.crop_mask(mask)
    back = np.zeros_like(mask)
    back[r0:r1, c0:c1] = patch
    assert patch.dtype == np.float32 and patch.flags['C_CONTIGUOUS']
    assert back.tobytes() == mask.tobytes()
    assert patch[0].any() and patch[-1].any() and patch[:, 0].any() and patch[:, -1].any()       # the box is tight
    assert 0 <= r0 < r1 <= 512 and 0 <= c0 < c1 <= 512
    if (x, y) == (256, 256):
        assert (r1 - r0, c1 - c0) == (101, 101)          # the float32 support of exp(-(d / 5)^2)


def test_crop_mask_refuses_an_empty_mask():
    from fib_tf_amd import egm
    with pytest.raises(ValueError, match='no non-zero'):
        egm.crop_mask(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError):
        egm.crop_mask(np.zeros(8, np.float32))


def test_header_declares_and_lib_prototypes():
    from fib_tf_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'fibhip.h')).read()
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(\s*fibhip_t\b' % name, src), name
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1] is _lib.C.c_int
    assert len(_lib.SYMBOLS['fibhip_electrode_begin'][0]) == 7
    assert _lib.SYMBOLS['fibhip_electrode_begin'][0][6] is _lib.C.c_longlong
    for m in ('electrode_begin', 'electrode_count', 'electrode_read', 'electrode_end'):
        assert callable(getattr(_lib.Stepper, m))


def test_reference_electrode_bound_is_loose_and_sharp():
    """the header's bound for the reference's electrode (Gaussian, radius 5, 512 x 512) against an emulation of a conforming
    float32 summation and against a patch misplaced by one column"""
    from fib_tf_amd import egm
    rng = np.random.default_rng(1)
    mask = egm.create_mask(_grid(512, 512), 315, 256, 5)
    rect, patch = egm.crop_mask(mask)
    x = (-85.0 + 100.0 / (1.0 + np.exp(-(np.arange(512) - 312.0) / 2.0)))[None, :] + rng.normal(0, .1, (512, 512))
    x = x.astype(np.float32)
    s, _ = ref.weighted_sum(x, rect, patch)
    b = ref.bound(x, rect, patch)
    assert ref.depth(patch.size) == 56
    r0, r1, c0, c1 = rect
    prod = (patch * x[r0:r1, c0:c1]).ravel()                      # float32 products
    acc = np.zeros(256, np.float32)
    for i in range(0, prod.size, 256):                             # 256 strided accumulators ...
        chunk = prod[i:i + 256]
        acc[:chunk.size] += chunk
    while acc.size > 1:                                            # ... and an 8-level tree
        acc = acc[:acc.size // 2] + acc[acc.size // 2:]
    assert abs(float(acc[0]) - s) <= b
    shifted, _ = ref.weighted_sum(x, (r0, r1, c0 + 1, c1 + 1), patch)
    assert abs(shifted - s) > 100 * b


# ---- the recorder and record_on_device over a stub stepper ---------------------------------------------------------
class StubStepper:
    """keeps the state on the host: a tick adds `drift` to array 0; the electrode_* methods follow include/fibhip.h"""
    steps_per_tick = 10

    def __init__(self, x0, drift):
        self.x = np.array(x0, np.float32)
        self.drift = np.float32(drift)
        self.el = None
        self.ticks = 0

    def expect(self, n):
        pass

    def sync(self):
        pass

    def step(self, n):
        for _ in range(n):
            self.x = self.x + self.drift
            self.ticks += 1
            if self.el is not None:
                self.el['k'] += 1
                if self.el['k'] % self.el['every'] == 0:
                    assert len(self.el['rows']) < self.el['cap'], 'trace full'
                    self.el['rows'].append([np.float32(ref.weighted_sum(self.x, r, p)[0]) for r, p in self.el['pairs']])
                    self.el['at'].append(self.ticks - 1)

    def get_state(self, var):
        return self.x.copy()

    def electrode_begin(self, var, rects, patches, every=1, capacity=1):
        assert var == 0
        self.el = {'pairs': list(zip(rects, patches)), 'every': every, 'cap': capacity, 'k': 0, 'rows': [], 'at': []}
        self.attached = getattr(self, 'attached', []) + [self.el]

    def electrode_count(self):
        return len(self.el['rows'])

    def electrode_read(self, first=0, count=None):
        rows = self.el['rows'][first:] if count is None else self.el['rows'][first:first + count]
        return np.array(rows, np.float32).reshape(len(rows), len(self.el['pairs']))

    def electrode_end(self):
        self.el = None


def _stub_model(cls_name, x0, drift, duration):
    from fib_tf_amd.fenton import Fenton4v
    from fib_tf_amd.br import BeelerReuter
    cls = {'fenton': Fenton4v, 'br': BeelerReuter}[cls_name]
    h, w = x0.shape
    m = cls({'height': h, 'width': w, 'dt': 0.1, 'diff': 1.0, 'duration': duration})
    m._stepper = StubStepper(x0, drift)
    m.defined = True
    m.dt_per_step = 10
    if cls_name == 'fenton':
        m.image = lambda: m._stepper.get_state(0)
    else:
        m.image = lambda: (m._stepper.get_state(0) - m.min_v) / (m.max_v - m.min_v)
    return m


@pytest.mark.parametrize('kind', ['fenton', 'br'])
def test_affine_conversion_matches_mean_of_image_times_mask(kind):
    from fib_tf_amd import egm
    rng = np.random.default_rng(5)
    lo, hi = (0.0, 1.0) if kind == 'fenton' else (-85.0, 20.0)
    x0 = rng.uniform(lo, hi, (40, 56)).astype(np.float32)
    m = _stub_model(kind, x0, 0.01, 6.0)
    masks = [egm.create_mask(m, 20, 20, 5), egm.create_mask(m, 54, 2, 4)]
    want = []
    with m.record_electrodes(masks, every=2) as rec:
        assert rec.capacity == 3 and rec.every == 2
        for i in range(6):
            m._stepper.step(1)
            if i % 2 == 1:
                img = m.image().astype(np.float64)
                want.append([np.mean(img * mk.astype(np.float64)) for mk in masks])
        got = rec.traces()
        raw = rec.traces(raw=True)
        assert rec.count() == 3
    want = np.array(want)
    assert got.shape == (3, 2) and got.dtype == np.float64 and raw.dtype == np.float64
    # the stub rounds each raw sum to float32 once: that rounding, scaled like the sum, is all that separates the two
    scale = rec.affine[0]
    assert np.all(np.abs(got - want) <= scale * np.abs(raw) * 2.0 ** -24 / rec.cells + 1e-15)
    if kind == 'fenton':
        assert rec.affine == (1.0, 0.0)
    else:
        assert rec.affine[0] == pytest.approx(1.0 / (m.max_v - m.min_v)) and rec.affine[1] == pytest.approx(-m.min_v / (m.max_v - m.min_v))
    with pytest.raises(AssertionError, match='closed'):
        rec.traces()


@pytest.mark.parametrize('every_ms', [1.0, 3.0])
def test_record_on_device_samples_when_record_does(every_ms):
    from fib_tf_amd import egm
    rng = np.random.default_rng(7)
    x0 = rng.uniform(0, 1, (24, 32)).astype(np.float32)
    ticks = 11
    a, b = _stub_model('fenton', x0, 0.02, ticks * 1.0 + 1e-9), _stub_model('fenton', x0, 0.02, ticks * 1.0 + 1e-9)
    m1, m2 = egm.create_mask(a, 8, 8, 3), egm.create_mask(a, 20, 12, 3)
    fired = []
    polled = egm.record(a, m1, m2, every_ms=every_ms)
    dev = egm.record_on_device(b, m1, m2, every_ms=every_ms, on_tick=fired.append)
    assert fired == list(range(ticks))
    stride = int(every_ms)
    want_at = [i for i in range(ticks) if i % stride == 0]
    at = [t for el in b._stepper.attached for t in el['at']]
    assert at == want_at                                           # the ticks after which record() samples
    assert dev.shape == polled.shape == (len(want_at), 2) and dev.dtype == np.float64
    assert np.allclose(dev, polled, rtol=0, atol=1e-6)
    assert b._stepper.el is None                                   # detached at the end


def test_record_electrodes_needs_define_and_checks_masks():
    from fib_tf_amd.fenton import Fenton4v
    m = Fenton4v({'height': 8, 'width': 8, 'dt': 0.1, 'diff': 1.0})
    with pytest.raises(AssertionError, match='after calling define'):
        m.record_electrodes([np.ones((8, 8), np.float32)])
    m = _stub_model('fenton', np.zeros((8, 8), np.float32), 0.0, 1.0)
    with pytest.raises(ValueError, match='shape'):
        m.record_electrodes([np.ones((8, 9), np.float32)])
    with pytest.raises(ValueError, match='every'):
        m.record_electrodes([np.ones((8, 8), np.float32)], every=0)


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
            m.record_electrodes([np.ones((64, 16), np.float32)])
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


def test_affine_hook_is_checked_against_image_at_attach():
    """a model whose image() rescales but whose _image_affine() says it does not is refused when the recorder is attached"""
    m = _stub_model('fenton', np.random.default_rng(2).uniform(-80, 20, (8, 8)).astype(np.float32), 0.0, 2.0)
    m.image = lambda: (m._stepper.get_state(0) + 90.0) / 120.0
    mask = np.ones((8, 8), np.float32)
    with pytest.raises(ValueError, match='_image_affine'):
        m.record_electrodes([mask])
    assert m._stepper.el is None                             # nothing was attached
    m._image_affine = lambda: (1.0 / 120.0, 90.0 / 120.0)
    with m.record_electrodes([mask]) as rec:
        assert rec.affine == (1.0 / 120.0, 90.0 / 120.0)
