"""op tables — traced models whose outputs are ONE tf op each, the argument planes they are run on, and the float64
reference / true-ulp metric they are judged by.  Shared by tests/test_traced_ops_cpu.py, tests/test_gpu_traced_ops.py
and tools/op_accuracy.py (a helper module, not a conftest).

A table is a `fib_tf_amd.traced.IonicModel` in the style of tests/models/*: the diffusing variable `u` is held at the
constant 1 (enforce_boundary + laplace of a constant is exactly 0, so it never changes), the argument planes `x`, `y`,
`z` are assigned to themselves, and every further variable is `o_i.assign(op_i(x, y, z))`.  define() chains two solve()
calls, so the tick-fusing strip kernel and its multi-tick form exist; the outputs are idempotent because the arguments
never change.  A table has at most 12 variables (larger ones spill registers in the multi-tick kernel, which is not what
these tables are about)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import fib_tf_amd.tfgraph as tf                                    # noqa: E402
from fib_tf_amd.traced import IonicModel                           # noqa: E402

f32, f64 = np.float32, np.float64
H, W = 128, 512
CELLS = H * W
MAX_VARS = 12

# division constants: the first four pass traced.divc_is_exact (3-instruction form), DIVK does not (true division kept)
DIVC = (7.0, 30.0, -6.8, 12.0)
DIVK = 1.9999998807907104           # 2 - 2^-23: a significand of all ones is the case Markstein's theorem excludes
MAD_C, MAD_C2, MAD_Z2 = 1.7, 2.5, 0.75
CDIV = 3.0
MAX_C, MIN_C, CLIP_LO, CLIP_HI, CLIP_THI, NE_C, WH_C = 0.25, 0.75, -0.5, 0.5, 1.5, 0.5, 0.25


# ---------------------------------------------------------------------------------------------------------------------
# the tables: name -> (number of argument planes, [(output, builder(x, y, z))], [(fired output, builder)])
# ---------------------------------------------------------------------------------------------------------------------
def _heav_twins():
    """(1 + s) * 0.5 and (1 - s) * 0.5 on ONE shared sign node: it is read twice, so neither melts into g_heav"""
    memo = {}

    def s(x):
        if id(x) not in memo:
            memo[id(x)] = tf.sign(x)
        return memo[id(x)]
    return (lambda x, y, z: (1.0 + s(x)) * 0.5), (lambda x, y, z: (1.0 - s(x)) * 0.5)


def _tanh_twins():
    """1 + t and t itself on ONE shared tanh node: the sum stays 1.0f + P::tanhv(x)"""
    memo = {}

    def t(x):
        if id(x) not in memo:
            memo[id(x)] = tf.tanh(x)
        return memo[id(x)]
    return (lambda x, y, z: 1.0 + t(x)), (lambda x, y, z: t(x))


def _tables():
    heav_tw, heavn_tw = _heav_twins()
    opt_tw, tanh_tw = _tanh_twins()
    one = lambda m: tf.where(m, 1.0, 0.0)                           # noqa: E731
    return {
        'arith': (3, [
            ('add', lambda x, y, z: x + y),
            ('sub', lambda x, y, z: x - y),
            ('mul', lambda x, y, z: x * y),
            ('mad3_add', lambda x, y, z: x * y + z),
            ('mad3_rsub', lambda x, y, z: z - x * y),
            ('mad3_sub', lambda x, y, z: x * y - z),
            ('mad_c', lambda x, y, z: x * MAD_C + z),
            ('mad_cc', lambda x, y, z: MAD_Z2 - x * MAD_C2)], []),
        'div': (3, [
            ('div', lambda x, y, z: x / y),
            ('divc_7', lambda x, y, z: x / DIVC[0]),
            ('divc_30', lambda x, y, z: x / DIVC[1]),
            ('divc_m6p8', lambda x, y, z: x / DIVC[2]),
            ('divc_12', lambda x, y, z: x / DIVC[3]),
            ('divk', lambda x, y, z: x / DIVK),
            ('cdiv', lambda x, y, z: CDIV / x),
            ('rcp', lambda x, y, z: tf.reciprocal(x))], []),
        'unary': (3, [
            ('sqrt', lambda x, y, z: tf.sqrt(x)),
            ('square', lambda x, y, z: tf.square(x)),
            ('abs', lambda x, y, z: tf.abs(x)),
            ('neg', lambda x, y, z: -x),
            ('sign', lambda x, y, z: tf.sign(x)),
            ('pow_1', lambda x, y, z: tf.pow(x, 1.0)),
            ('pow_2', lambda x, y, z: tf.pow(x, 2.0)),
            ('pow_3', lambda x, y, z: tf.pow(x, 3.0))], []),
        'minmax': (3, [
            ('max_t', lambda x, y, z: tf.maximum(x, y)),
            ('min_t', lambda x, y, z: tf.minimum(x, y)),
            ('max_c', lambda x, y, z: tf.maximum(x, MAX_C)),
            ('min_c', lambda x, y, z: tf.minimum(MIN_C, x)),
            ('clip_c', lambda x, y, z: tf.clip_by_value(x, CLIP_LO, CLIP_HI)),
            ('clip_t', lambda x, y, z: tf.clip_by_value(x, y, CLIP_THI)),
            ('and', lambda x, y, z: one(tf.logical_and(x > y, x < z))),
            ('or', lambda x, y, z: one(tf.logical_or(x >= y, x <= z)))], []),
        'cmp': (3, [
            ('gt', lambda x, y, z: one(x > y)),
            ('ge', lambda x, y, z: one(x >= y)),
            ('lt', lambda x, y, z: one(x < y)),
            ('le', lambda x, y, z: one(x <= y)),
            ('eq', lambda x, y, z: one(tf.equal(x, y))),
            ('ne', lambda x, y, z: one(tf.not_equal(x, NE_C))),
            ('not', lambda x, y, z: tf.where(tf.logical_not(x > y), x, y)),
            ('where_t', lambda x, y, z: tf.where(tf.less(WH_C, x), y, z))], []),
        'heav': (3, [
            ('heav', lambda x, y, z: (1.0 + tf.sign(x)) * 0.5),
            ('heav_not', lambda x, y, z: (1.0 - tf.sign(x)) * 0.5),
            ('heav_twin', heav_tw),
            ('heav_not_twin', heavn_tw),
            ('one_plus_tanh', lambda x, y, z: 1.0 + tf.tanh(x)),
            ('one_plus_tanh_twin', opt_tw),
            ('tanh', tanh_tw),
            ('sigmoid', lambda x, y, z: tf.sigmoid(x))], []),
        'trans': (3, [
            ('exp', lambda x, y, z: tf.exp(x)),
            ('expm1', lambda x, y, z: tf.expm1(x)),
            ('log', lambda x, y, z: tf.log(x)),
            ('pow_0p5', lambda x, y, z: tf.pow(x, 0.5)),
            ('pow_1p5', lambda x, y, z: tf.pow(x, 1.5)),
            ('pow_m1', lambda x, y, z: tf.pow(x, -1.0))], []),
        # 8 variables: the table of the multi-tick form, and the one with a second assign group (pointwise_kernel)
        'forms': (2, [
            ('one_plus_tanh', lambda x, y, z: 1.0 + tf.tanh(x)),
            ('expm1', lambda x, y, z: tf.expm1(x)),
            ('mad3_add', lambda x, y, z: x * y + x)],
            [('one_plus_tanh', lambda x, y, z: 1.0 + tf.tanh(x)),
             ('expm1', lambda x, y, z: tf.expm1(x))]),
    }


TABLE_NAMES = ('arith', 'div', 'unary', 'minmax', 'cmp', 'heav', 'trans', 'forms')
ARGS = 'xyz'


class OpTable(IonicModel):
    """one table; TABLE is set by table_class()"""
    TABLE = None

    def __init__(self, props):
        IonicModel.__init__(self, props)
        self.min_v, self.max_v, self.depol = 0.0, 2.0, 0.0
        self.nargs, self.outs, self.fired = _tables()[self.TABLE]

    def solve(self, state):
        u = state[0]
        args = list(state[1:1 + self.nargs])
        xyz = args + [None] * (3 - len(args))
        u0 = self.enforce_boundary(u)
        u1 = u0 + self.diff * self.dt * self.laplace(u0)
        return (u1,) + tuple(args) + tuple(fn(*xyz) for _, fn in self.outs)

    def define(self, s1=True):
        super().define()
        shape = [self.height, self.width]
        ones, zeros = np.ones(shape, np.float32), np.zeros(shape, np.float32)
        u = tf.Variable(ones, name='u')
        args = [tf.Variable(ones, name=ARGS[i]) for i in range(self.nargs)]
        outs = [tf.Variable(zeros, name='o_' + n) for n, _ in self.outs]
        first = (u,) + tuple(args) + tuple(outs)
        state = first
        for _ in range(2):
            state = self.solve(state)
        self.dt_per_step = 2
        self._ode_op = tf.group(*[v.assign(new) for v, new in zip(first, state)])
        if self.fired:
            xyz = args + [None] * (3 - len(args))
            fired = [tf.Variable(zeros, name='p_' + n) for n, _ in self.fired]
            self._ops['ops'] = tf.group(*[p.assign(fn(*xyz)) for p, (_, fn) in zip(fired, self.fired)])
        self._u = u

    def pot(self):
        return self._u


def table_class(name):
    return type('OpTable_' + name, (OpTable,), {'TABLE': name})


def make_table(name, fast=False, height=H, width=W, device=None):
    cfg = {'height': height, 'width': width, 'dt': 0.1, 'dt_per_plot': 1, 'diff': 1.0, 'duration': 1, 'fast_math': fast}
    if device is not None:
        cfg['device'] = device
    m = table_class(name)(cfg)
    m.define()
    return m


# ---------------------------------------------------------------------------------------------------------------------
# argument planes
# ---------------------------------------------------------------------------------------------------------------------
def bits(x):
    return np.asarray(x, f32).view(np.uint32)


def _key(x):
    """float32 -> an integer that orders like the float (the two zeros share key 0)"""
    b = np.asarray(x, f32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7FFFFFFF), b)


def _unkey(k):
    k = np.asarray(k, np.int64)
    b = np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32)
    return b.view(f32)


def sweep(lo, hi, stride):
    """(a) every `stride`-th float32 bit pattern of [lo, hi] (lo < hi; the interval may cross zero)"""
    a, b = int(_key(f32(lo))), int(_key(f32(hi)))
    return _unkey(np.arange(a, b + 1, int(stride), dtype=np.int64))


def around(point, n=256):
    """(b) every float within +-n bit patterns of `point`"""
    k = int(_key(f32(point)))
    return _unkey(np.arange(k - n, k + n + 1, dtype=np.int64))


TINY, SUBMAX, MINNORM, BIG = f32(2.0 ** -149), np.uint32(0x007FFFFF).view(f32), f32(2.0 ** -126), np.finfo(f32).max
TABLE_CONSTANTS = DIVC + (DIVK, MAD_C, MAD_C2, MAD_Z2, CDIV, MAX_C, MIN_C, CLIP_LO, CLIP_HI, CLIP_THI, NE_C, WH_C, 0.5)
# worst arguments of the round-4 device record (profiles/r04_accuracy_one_plus_tanh.txt)
RECORDED_WORST = (-63.8778992, -0.356124669, -0.629270315, 0.629270315, -11.1562872, 69.2274323, 0.347814947,
                  0.249925584, -3.54805207, 0.0215849485, 0.636468709)


def special_finite():
    """(c) the fixed special set, finite part"""
    v = [0.0, -0.0]
    for p in (TINY, SUBMAX, MINNORM, f32(1.0), BIG):
        v += [p, -p]
    one = int(_key(f32(1.0)))
    v += list(_unkey([one - 1, one + 1]))
    for c in TABLE_CONSTANTS:
        k = int(_key(f32(c)))
        v += list(_unkey([k - 1, k, k + 1]))
    v += [f32(w) for w in RECORDED_WORST]
    return np.array(v, f32)


def special_nonfinite():
    return np.array([np.inf, -np.inf, np.nan], f32)


def pairs(a, b=None):
    """every ordered pair of two small sets, as two flat arrays"""
    b = a if b is None else b
    x, y = np.meshgrid(a, b, indexing='ij')
    return x.ravel().astype(f32), y.ravel().astype(f32)


def random_normal_range(n, seed, lo_exp=-20, hi_exp=20):
    """random floats of both signs, significand uniform, exponent uniform in [lo_exp, hi_exp)"""
    r = np.random.default_rng(seed)
    m = r.uniform(1.0, 2.0, n)
    e = r.integers(lo_exp, hi_exp, n)
    s = np.where(r.random(n) < 0.5, -1.0, 1.0)
    return (s * np.ldexp(m, e)).astype(f32)


def mad_plane(n=CELLS, seed=5):
    """x, y, z for the multiply-add forms: uniform in [-2, 2] (where two roundings and one differ for about a quarter
    of the cells), led by the exact cancellation triple x = y = 1 + 2^-12, z = -(1 + 2^-11): two roundings give 0,
    a fused multiply-add gives 2^-24 (cell 0, for x*y + z; cell 1 holds z = +(1 + 2^-11) for z - x*y and x*y - z)"""
    r = np.random.default_rng(seed)
    x, y, z = (r.uniform(-2.0, 2.0, n).astype(f32) for _ in range(3))
    x[:2] = y[:2] = f32(1.0 + 2.0 ** -12)
    z[0], z[1] = f32(-(1.0 + 2.0 ** -11)), f32(1.0 + 2.0 ** -11)
    return x, y, z


def divc_plane(n=CELLS, seed=6):
    return random_normal_range(n, seed, -6, 7)


def to_planes(a, fill=1.0):
    """flat samples -> [k, H, W] planes, the tail filled"""
    a = np.asarray(a, f32).ravel()
    k = max(1, -(-a.size // CELLS))
    out = np.full(k * CELLS, fill, f32)
    out[:a.size] = a
    return out.reshape(k, H, W)


def samples_trans():
    """arguments of the `trans` table: exp, expm1, log, pow"""
    return np.concatenate([
        sweep(1e-7, 88.72, 449), sweep(-87.33, -1e-7, 449),                         # exp's finite range, 1.1 M arguments
        sweep(-104.0, -87.33, 449), sweep(-1e-7, -TINY, 4001), sweep(TINY, 1e-7, 4001),   # expm1: the rest of its range
        sweep(MINNORM, BIG, 4099),                                                  # log, pow: every positive normal binade
        around(-87.33), around(88.72), around(0.0), around(-104.0), around(88.0), around(1.0), special_finite()])


def samples_tanh():
    """arguments of the `heav` table: tanh and the two forms of 1 + tanh"""
    return np.concatenate([
        sweep(-BIG, BIG, 4099),                                                     # every finite x by stride
        sweep(-60.0, -1e-7, 499), sweep(1e-7, 20.0, 499),                           # 1 + tanh's range
        sweep(0.3, 11.0, 97), sweep(-11.0, -0.3, 97),                               # both forms of tanh and their switch
        around(0.625), around(-0.625), around(10.0), around(-10.0), around(0.0), special_finite()])


def samples_cube():
    return np.concatenate([sweep(-1e12, 1e12, 4099), special_finite()])


# what tools/op_accuracy.py reports: (table, output, label, float64 function, domain[, 'abs' where the form's accuracy
# is absolute]).  Domains are those tests/test_gpu_traced_ops.py bounds the ops on: results finite and (log, pow) normal
def _between(lo, hi, lo_open=False):
    return lambda x: ((x > f32(lo)) if lo_open else (x >= f32(lo))) & (x <= f32(hi))


def _pow_dom(e):
    def dom(x):
        with np.errstate(all='ignore'):
            w = np.power(np.where(x >= MINNORM, x.astype(f64), 1.0), e)
        return (x >= MINNORM) & np.isfinite(x) & (w >= 2.0 ** -126) & (w <= float(BIG))
    return dom


ACCURACY = (
    ('trans', 'exp', 'exp', np.exp, _between(-87.33, 88.72)),
    ('trans', 'expm1', 'expm1 (x < 0)', np.expm1, lambda x: (x >= f32(-104.0)) & (x < 0)),
    ('trans', 'expm1', 'expm1 (x > 0)', np.expm1, _between(0.0, 88.0, True)),
    ('trans', 'log', 'log', np.log, lambda x: (x >= MINNORM) & np.isfinite(x)),
    ('trans', 'pow_0p5', 'pow(x, 0.5)', lambda v: np.power(v, 0.5), _pow_dom(0.5)),
    ('trans', 'pow_1p5', 'pow(x, 1.5)', lambda v: np.power(v, 1.5), _pow_dom(1.5)),
    ('trans', 'pow_m1', 'pow(x, -1)', lambda v: np.power(v, -1.0), _pow_dom(-1.0)),
    ('unary', 'pow_3', 'pow(x, 3)', lambda v: v ** 3, lambda x: np.abs(x) <= f32(1e12)),
    ('unary', 'sqrt', 'sqrt', np.sqrt, lambda x: (x >= MINNORM) & np.isfinite(x)),
    ('heav', 'tanh', 'tanh', np.tanh, np.isfinite, 'abs'),
    ('heav', 'one_plus_tanh', '1 + tanh, fused', lambda v: 1.0 + np.tanh(v), _between(-60.0, 20.0), 'abs'),
    ('heav', 'one_plus_tanh_twin', '1 + tanh, unfused', lambda v: 1.0 + np.tanh(v), _between(-60.0, 20.0), 'abs'),
    ('heav', 'sigmoid', 'sigmoid', lambda v: 1.0 / (1.0 + np.exp(-v)), _between(-87.0, 87.0), 'abs'),
)
SAMPLES = {'trans': samples_trans, 'heav': samples_tanh, 'unary': samples_cube}


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulation of float32 arithmetic, and the metric
# ---------------------------------------------------------------------------------------------------------------------
def rn(a):
    """round a float64 array to float32 (returned as float64)"""
    with np.errstate(over='ignore', under='ignore'):
        return np.asarray(a, f64).astype(f32).astype(f64)


def fma32(x, y, z):
    """RN(x*y + z) for float32 x, y, z, exactly: the product is exact in float64, the sum is formed with its error
    term (TwoSum) and rounded to odd, after which the rounding to float32 is the single rounding of a hardware fma"""
    x, y, z = (np.asarray(v, f32).astype(f64) for v in (x, y, z))
    p = x * y
    s = p + z
    bb = s - p
    e = (p - (s - bb)) + (z - bb)
    sb = s.view(np.int64)
    toward = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    s = np.where((e != 0) & ((sb & 1) == 0), toward, s)
    return s.astype(f32)


def mad_two_roundings(x, y, z):
    x, y, z = (np.asarray(v, f32) for v in (x, y, z))
    return (x * y).astype(f32) + z


def ulp_unit(want):
    """2^(max(floor(log2|want|), -126) - 23): the float32 ulp at the true value"""
    w = np.abs(np.asarray(want, f64))
    with np.errstate(divide='ignore'):
        e = np.floor(np.log2(w))
    e = np.maximum(np.where(np.isfinite(e), e, -126.0), -126.0)
    return np.exp2(e - 23.0)


def ulp_err(got, want):
    """true-ulp error of float32 `got` against the float64 value `want`"""
    return np.abs(np.asarray(got, f32).astype(f64) - np.asarray(want, f64)) / ulp_unit(want)


def same(got, want):
    """value-for-value equality of two float32 arrays: == on floats, NaN wherever `want` is NaN"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    return np.where(np.isnan(want), np.isnan(got), got == want)


# ---------------------------------------------------------------------------------------------------------------------
# running a table: on the device, and through the float32 interpreter
# ---------------------------------------------------------------------------------------------------------------------
def _state(m, planes):
    """[nvar, H, W] with u = 1, the argument planes, outputs 0"""
    names = m.VAR_NAMES
    st = np.zeros((len(names), H, W), f32)
    st[names.index('u')] = 1.0
    for n, p in planes.items():
        st[names.index(n)] = p
    return st


def _split(x, y, z, nargs):
    given = [to_planes(v) for v in (x, y, z)[:nargs] if v is not None]
    k = max(p.shape[0] for p in given)
    full = []
    for i in range(nargs):
        v = (x, y, z)[i]
        full.append(to_planes(v) if v is not None else np.ones((k, H, W), f32))
    assert all(p.shape[0] == k for p in full)
    return k, full


def run_device(table, x, y=None, z=None, fast=False, ticks=1, fired=False):
    """the table on the device (environment as the caller set it): {output: flat float32 array}, info.  One model, one
    set_state / step / get_state per plane of 65536 cells; `fired` runs the table's second assign group instead of
    the tick and returns its outputs"""
    m = make_table(table, fast=fast)
    m._ensure_compiled()
    st = m._stepper
    n = np.asarray(x).size
    k, planes = _split(x, y, z, m.nargs)
    names = m.VAR_NAMES
    res = {}
    for i in range(k):
        st.set_state(-1, _state(m, {ARGS[j]: planes[j][i] for j in range(m.nargs)}))
        if fired:
            st.step_mode(1)
        else:
            st.step(ticks)
        got = st.get_state(-1)
        assert np.array_equal(got[names.index('u')], np.ones((H, W), f32)), 'the constant plane moved'
        for j in range(m.nargs):
            assert np.array_equal(got[names.index(ARGS[j])].view(np.uint32), planes[j][i].view(np.uint32))
        for nm in names:
            if nm.startswith('p_' if fired else 'o_'):
                res.setdefault(nm[2:], []).append(got[names.index(nm)].ravel())
    info = {'plan': st.launch_plan(), 'ticks_per_launch': st.ticks_per_launch(), 'stats': st.launch_stats(),
            'library': m._library._name}
    st.close()
    m._stepper = None
    return {nm: np.concatenate(v)[:n] for nm, v in res.items()}, info


def run_interpreter(table, x, y=None, z=None, fired=False):
    """the same through oracle/graph_eval.py: one float32 NumPy operation per graph node"""
    from oracle.graph_eval import Interpreter
    m = make_table(table)
    c = m._analyze()
    it = Interpreter(c, None)
    n = np.asarray(x).size
    k, planes = _split(x, y, z, m.nargs)
    names = m.VAR_NAMES
    res = {}
    for i in range(k):
        got = it.run_mode(_state(m, {ARGS[j]: planes[j][i] for j in range(m.nargs)}), 1 if fired else 0)
        for nm in names:
            if nm.startswith('p_' if fired else 'o_'):
                res.setdefault(nm[2:], []).append(got[names.index(nm)].ravel())
    return {nm: np.concatenate(v)[:n] for nm, v in res.items()}
