"""-m gpu: every op the traced-model code generator can emit, run ONE OP PER OUTPUT on the device (tests/op_tables.py)
and judged per op: bit for bit against the float32 interpreter where the op is a single IEEE operation, in true ulps
against float64 where it is a transcendental, against bounds derived from the fast forms themselves under the fast
policy, and against the saturation / NaN contract of DESIGN.md 9 outside the finite range.

Every test sets FIBHIP_AUTOTUNE=0 and, unless it says otherwise, FIBHIP_MT=0; loads a plane with set_state(-1, ...),
calls step(1) and reads it back with get_state(-1), on a 128 x 512 grid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import op_tables as T  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
E = 2.0 ** -24                                  # unit roundoff of float32; an instruction "accurate to 1 ulp" is within 2 E
SLACK = 1.0 + 2.0 ** -10                        # second-order terms of the first-order derivations below


@pytest.fixture(autouse=True)
def _plan(monkeypatch, gpu_lib):
    monkeypatch.setenv('FIBHIP_AUTOTUNE', '0')
    monkeypatch.setenv('FIBHIP_MT', '0')
    for k in ('FIBHIP_K', 'FIBHIP_VARIANT'):
        monkeypatch.delenv(k, raising=False)


_runs = {}


def device(table, key, make, fast=False):
    """one fused-strip run of `table` on the samples make() returns, shared by the tests of this module"""
    k = (table, key, fast)
    if k not in _runs:
        args = make()
        args = args if isinstance(args, tuple) else (args,)
        out, info = T.run_device(table, *args, fast=fast)
        assert info['plan'] == (2, 1) and '#module:model_' in info['library'], info
        _runs[k] = (args, out)
    return _runs[k]


def worst(err, x):
    i = int(np.nanargmax(err))
    return float(err[i]), float(x[i])


# ======================================================================================================================
# a. rounding-faithful policy, the bit-exact class: device == float32 interpreter, value for value
# ======================================================================================================================
def _finite_args():
    """special set x special set (subnormals included), then random numbers over the whole normal range"""
    s = T.special_finite()
    x, y = T.pairs(s)
    z = np.roll(y, 17)
    n = 2 * T.CELLS - x.size
    r = [T.random_normal_range(n, seed, -126, 128) for seed in (1, 2, 3)]
    return tuple(np.concatenate(p) for p in zip((x, y, z), r))


def _nonfinite_args():
    s = np.concatenate([T.special_nonfinite(), T.special_finite()])
    x, y = T.pairs(s)
    z = np.roll(y, 5)
    return x, y, z


# table -> (outputs held bit for bit on finite arguments, those also held on NaN / +-inf arguments)
BITEXACT = {
    'arith': (('add', 'sub', 'mul', 'mad3_add', 'mad3_rsub', 'mad3_sub', 'mad_c', 'mad_cc'), ('add', 'sub', 'mul')),
    'div': (('div', 'cdiv', 'divk', 'rcp'), ('div', 'cdiv')),
    'unary': (('sqrt', 'square', 'abs', 'neg', 'sign', 'pow_1', 'pow_2'), ('sqrt', 'neg', 'abs')),
    'minmax': (('max_t', 'min_t', 'max_c', 'min_c', 'clip_c', 'clip_t', 'and', 'or'), ('and', 'or')),
    'cmp': (('gt', 'ge', 'lt', 'le', 'eq', 'ne', 'not', 'where_t'),) * 2,
    'heav': (('heav', 'heav_not', 'heav_twin', 'heav_not_twin'), ()),
}


def _assert_same(got, want, args, what):
    ok = T.same(got, want)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError('%s: %d of %d cells differ; first at x=%r y=%r z=%r: device %r, interpreter %r' % (
            what, int((~ok).sum()), ok.size, args[0][i], args[1][i], args[2][i], got[i], want[i]))


@pytest.mark.parametrize('table', sorted(BITEXACT))
def test_exact_policy_single_ieee_ops_bit_for_bit(table):
    finite_ops, nonfinite_ops = BITEXACT[table]
    for key, make, ops in (('finite', _finite_args, finite_ops), ('nonfinite', _nonfinite_args, nonfinite_ops)):
        if not ops:
            continue
        args, got = device(table, key, make)
        want = T.run_interpreter(table, *args)
        if table == 'unary':
            # pow(x, 1) = x and pow(x, 2) = RN(x * x) are what the op is; the interpreter's np.power goes through a
            # vectorised powf that is itself up to an ulp off (x = 8.05611e-21 to the power 1), so it is not asked
            with np.errstate(all='ignore'):
                want['pow_1'], want['pow_2'] = args[0], args[0] * args[0]
        for op in ops:
            _assert_same(got[op], want[op], args, '%s.%s (%s arguments)' % (table, op, key))
            if op in ('neg', 'abs'):                       # the sign of zero (and of NaN's payload-free results) too
                fin = ~np.isnan(want[op])
                assert np.array_equal(np.signbit(got[op][fin]), np.signbit(want[op][fin])), op
    if table == 'heav':                                    # the peepholes against their unfused twins, on the device itself
        _, got = device(table, 'finite', _finite_args)
        assert np.array_equal(got['heav'], got['heav_twin']) and np.array_equal(got['heav_not'], got['heav_not_twin'])
        x = _finite_args()[0]
        sub = (np.abs(x) < T.MINNORM) & (x != 0)
        assert sub.sum() >= 300                         # subnormal arguments: float32 denormals are kept by the build
        assert np.array_equal(got['heav'][sub], np.where(x[sub] > 0, f32(1), f32(0)))


def test_exact_policy_multiply_add_is_two_roundings():
    """the teeth plane: a quarter of its cells differ between RN(RN(x*y) + z) and a fused multiply-add, the first cell
    is the cancellation triple (0 against 2^-24)"""
    args, got = device('arith', 'mad', T.mad_plane)
    x, y, z = args
    want = T.run_interpreter('arith', x, y, z)
    fused = T.fma32(x, y, z)
    assert np.mean(want['mad3_add'] != fused) >= 0.20
    for op in BITEXACT['arith'][0]:
        _assert_same(got[op], want[op], args, 'arith.%s (teeth plane)' % op)
    assert got['mad3_add'][0] == 0.0 and got['mad3_rsub'][1] == 0.0 and got['mad3_sub'][1] == 0.0       # the cancellation triples


def _divc_args():
    return np.concatenate([T.special_finite(), T.divc_plane(T.CELLS - 200, 6), T.random_normal_range(T.CELLS, 7, -126, 128)])


@pytest.mark.parametrize('op,c', list(zip(('divc_7', 'divc_30', 'divc_m6p8', 'divc_12'), T.DIVC)))
def test_exact_policy_division_by_a_constant_is_ieee_division(op, c):
    """RN(x/c) wherever |x/c| >= 2^-126; at most one subnormal ulp off below"""
    (x,), got = device('div', 'divc', _divc_args)
    with np.errstate(all='ignore'):
        want = x / f32(c)
    true = x.astype(f64) / float(f32(c))
    normal = np.abs(true) >= 2.0 ** -126
    assert normal.sum() > 100000 and (~normal).sum() > 300
    bad = normal & ~T.same(got[op], want)
    assert not bad.any(), '%s: %d quotients differ from IEEE division, e.g. x = %r: %r against %r' % (
        op, int(bad.sum()), x[bad][0], got[op][bad][0], want[bad][0])
    d = np.abs(got[op][~normal].astype(f64) - want[~normal].astype(f64))
    assert d.max() <= 2.0 ** -149, '%s: subnormal quotient off by %g subnormal ulps' % (op, d.max() / 2.0 ** -149)


# ======================================================================================================================
# b. rounding-faithful policy, the ulp class: against float64 NumPy, in true ulps
# ======================================================================================================================
_trans_args, _tanh_args, _cube_args = T.samples_trans, T.samples_tanh, T.samples_cube


def _ulp_check(op, x, got, want, dom, bound, share=None):
    err = T.ulp_err(got[dom], want[dom])
    w, at = worst(err, x[dom])
    above = float(np.mean(err > 1.0))
    print('%-22s %8d samples: worst %.3f ulp at x = %.9g; above 1 ulp: %.4f %%' % (op, int(dom.sum()), w, at, 100 * above))
    assert np.isfinite(got[dom]).all() and w <= bound, '%s: %.3f ulp at x = %.9g (bound %.2f)' % (op, w, at, bound)
    if share is not None:
        assert above <= share, '%s: %.4f %% of the results are more than 1 ulp off' % (op, 100 * above)


def test_exact_policy_exp_expm1_within_their_ulp_bounds():
    (x,), got = device('trans', 'ulp', _trans_args)
    x64 = x.astype(f64)
    dom = (x >= f32(-87.33)) & (x <= f32(88.72))
    assert dom.sum() >= 1000000
    # the header's claim: 1 ulp + the 1 ulp of v_exp_f32; recorded on the device: worst 1.262, 0.057 % above 1 ulp
    _ulp_check('exp', x, got['exp'], np.exp(np.where(dom, x64, 0.0)), dom, 2.0, share=0.005)
    neg = (x >= f32(-104.0)) & (x < 0)
    assert ((np.abs(x) < T.MINNORM) & neg).sum() > 100        # subnormal arguments included
    _ulp_check('expm1 (x < 0)', x, got['expm1'], np.expm1(np.where(neg, x64, 0.0)), neg, 1.0)    # header 0.9, recorded 0.864
    pos = (x > 0) & (x <= f32(88.0))
    _ulp_check('expm1 (x > 0)', x, got['expm1'], np.expm1(np.where(pos, x64, 0.0)), pos, 1.75)   # header 1.7, recorded 1.672


def test_exact_policy_log_pow_within_their_ulp_bounds():
    """ocml logf / powf: the HIP math API documents 1 ulp; the factor 2 covers the difference between its ulp
    definition (the ulp at the returned value) and the true-ulp metric (the ulp at the true value)"""
    (x,), got = device('trans', 'ulp', _trans_args)
    x64 = x.astype(f64)
    dom = (x >= T.MINNORM) & np.isfinite(x)
    _ulp_check('log', x, got['log'], np.log(np.where(dom, x64, 1.0)), dom, 2.0)
    for op, e in (('pow_0p5', 0.5), ('pow_1p5', 1.5), ('pow_m1', -1.0)):
        with np.errstate(all='ignore'):
            want = np.power(np.where(dom, x64, 1.0), e)
        ok = dom & (want >= 2.0 ** -126) & (want <= float(T.BIG))
        assert ok.sum() > 300000
        _ulp_check(op, x, got[op], want, ok, 2.0)


def test_exact_policy_cube_within_two_roundings():
    (x,), got = device('unary', 'cube', _cube_args)
    dom = np.abs(x) <= f32(1e12)
    _ulp_check('pow(x, 3)', x, got['pow_3'], x.astype(f64) ** 3, dom, 1.5)        # two roundings of an exact cube


def test_exact_policy_tanh_within_its_ulp_bound():
    (x,), got = device('heav', 'ulp', _tanh_args)
    x64 = x.astype(f64)
    fin = np.isfinite(x)
    _ulp_check('tanh', x, got['tanh'], np.tanh(x64), fin, 1.6)                    # recorded 1.504 at +-0.62927
    far = np.abs(x) >= 10.0
    assert far.sum() > 100000 and np.array_equal(got['tanh'][far], np.sign(x[far]))   # "tanh(10) rounds to 1": exactly +-1
    sub = (np.abs(x) < T.MINNORM) & (x != 0)
    assert sub.sum() > 100 and np.array_equal(got['tanh'][sub], x[sub])          # tanh x = x below 2^-126: denormals kept


def test_exact_policy_one_plus_tanh_fused_and_unfused():
    """the peephole is NOT the same float32 function as the sum it replaces: each has its own recorded absolute bound"""
    (x,), got = device('heav', 'ulp', _tanh_args)
    dom = (x >= -60.0) & (x <= 20.0)
    want = 1.0 + np.tanh(x[dom].astype(f64))
    assert dom.sum() > 800000
    for op, bound in (('one_plus_tanh', 4.0), ('one_plus_tanh_twin', 2.5)):      # recorded 3.1 and 1.95 (x 2^-24)
        err = np.abs(got[op][dom].astype(f64) - want) / E
        w, at = worst(err, x[dom])
        print('%-22s %8d samples: worst absolute error %.3f x 2^-24 at x = %.9g' % (op, int(dom.sum()), w, at))
        assert w <= bound, '%s: %.3f x 2^-24 at x = %.9g' % (op, w, at)
    differ = float(np.mean(got['one_plus_tanh'][dom] != got['one_plus_tanh_twin'][dom]))
    print('the two forms return different floats for %.2f %% of the arguments' % (100 * differ))
    assert differ > 0


# ======================================================================================================================
# c. fast policy: bounds derived from the forms of `struct Fast` (csrc/models.hpp), written down before the first run.
#    E = 2^-24.  One float32 rounding: relative error <= E.  v_exp_f32, v_log_f32, v_rcp_f32, v_sqrt_f32: 1 ulp, i.e.
#    relative error <= 2 E.  All bounds are first order; SLACK covers the products of two errors.
# ======================================================================================================================
def _rel(got, want):
    return np.abs(got.astype(f64) - want) / np.abs(want)


def _fast_check(what, x, err, bound):
    ratio = err / bound
    w, at = worst(ratio, x)
    print('%-22s %8d samples: worst error / derived bound = %.3f at x = %.9g' % (what, err.size, w, at))
    assert w <= SLACK, '%s: %.3f times its derived bound at x = %.9g' % (what, w, at)


def test_fast_policy_exp_log():
    (x,), got = device('trans', 'ulp', _trans_args, fast=True)
    x64 = x.astype(f64)
    # exp = v_exp_f32(RN(x * RN(log2 e))): the constant and the product each carry a relative error E, an absolute error of
    # |x log2 e| 2 E in the exponent, which is a relative error of |x| 2 E in 2^t (ln 2 * log2 e = 1); the instruction adds
    # 2 E:  relative error <= (|x| + 1) 2^-23 — held here as the (|x| + 2) 2^-23 of the issue's derivation
    dom = (x >= f32(-87.33)) & (x <= f32(88.72))
    _fast_check('exp', x[dom], _rel(got['exp'][dom], np.exp(x64[dom])), (np.abs(x64[dom]) + 2.0) * 2.0 ** -23)
    # log = __logf: at most v_log_f32 (2 E relative to log2 x) times RN(ln 2) (E for the constant, E for the product):
    # relative error <= 4 E  (a compiler that expands __logf to the accurate logf stays inside this)
    dom = (x >= T.MINNORM) & np.isfinite(x) & (x != 1.0)
    _fast_check('log', x[dom], _rel(got['log'][dom], np.log(x64[dom])), np.full(int(dom.sum()), 4 * E))
    assert np.all(got['log'][x == 1.0] == 0.0)


def test_fast_policy_expm1_and_its_switch():
    def make():
        return np.concatenate([_trans_args(), T.around(0.03, 4096), T.around(-0.03, 4096), T.sweep(-0.03, 0.03, 9973)])
    (x,), got = device('trans', 'expm1g', make, fast=True)
    x64 = x.astype(f64)
    with np.errstate(over='ignore'):
        want = np.expm1(x64)
    # |x| < 0.03: x + x^2 (1/2 + x/6 + x^2/24), last step one fma.  Truncation x^4/120 relative to x: <= 0.03^4/120 = 7e-9;
    # last rounding E = 6e-8; the roundings inside x^2 p (4 E relative to a term that is <= |x|/2 of the result) 0.015 * 4 E
    # = 4e-9: < 1e-7, the documented figure
    small = (np.abs(x) < f32(0.03)) & (x != 0)
    assert small.sum() > 100000
    _fast_check('expm1 (|x| < 0.03)', x[small], _rel(got['expm1'][small], want[small]), np.full(int(small.sum()), 1e-7))
    assert np.all(got['expm1'][x == 0] == 0)
    # |x| >= 0.03: exp(x) - 1: the absolute error of exp above, (|x| + 2) 2^-23 e^x, plus the rounding of the difference
    big = (np.abs(x) >= f32(0.03)) & (x >= f32(-87.33)) & (x <= f32(88.0))
    bound = (np.abs(x64[big]) + 2.0) * 2.0 ** -23 * np.exp(x64[big]) + E * np.abs(want[big])
    _fast_check('expm1 (|x| >= 0.03)', x[big], np.abs(got['expm1'][big].astype(f64) - want[big]), bound)


def test_fast_policy_tanh_and_one_plus_tanh():
    (x,), got = device('heav', 'ulp', _tanh_args, fast=True)
    fin = np.isfinite(x)
    x64 = x[fin].astype(f64)
    a = np.minimum(np.abs(x64), 45.0)           # beyond |x| = 44 the exponential is 0 or inf and both forms return +-1 / 0 / 2
    # tanhv = 1 - 2 rcp(e + 1), e = v_exp_f32(RN(x * c)), c = 2 RN(log2 e): e carries a relative error eta <= (2|x| + 1) 2 E
    # (as exp above, argument 2x).  d/de [2/(e+1)] = -2/(e+1)^2 and e/(e+1)^2 <= 1/4: that is <= eta/2 = (2|x| + 1) E absolute;
    # RN(e + 1) and v_rcp_f32 add (E + 2 E) * 2/(e+1) <= 6 E; 2 q is exact; the last subtraction rounds a value <= 1: E.
    # ABSOLUTE error <= (2|x| + 8) E (the form has no relative accuracy near 0, and claims none)
    _fast_check('tanh', x[fin], np.abs(got['tanh'][fin].astype(f64) - np.tanh(x64)), (2 * a + 8) * E)
    # one_plus_tanh = fma(q, -2, 2), the same q: the same terms, the last rounding on a value <= 2: (2|x| + 9) E
    _fast_check('1 + tanh', x[fin], np.abs(got['one_plus_tanh'][fin].astype(f64) - (1.0 + np.tanh(x64))), (2 * a + 9) * E)
    # the unfused twin: RN(1 + tanh): tanh's error plus one rounding of a value <= 2
    _fast_check('1 + tanh (twin)', x[fin], np.abs(got['one_plus_tanh_twin'][fin].astype(f64) - (1.0 + np.tanh(x64))), (2 * a + 10) * E)


def _fast_div_args():
    r = T.random_normal_range
    x = np.concatenate([T.special_finite(), T.divc_plane(T.CELLS, 6), r(T.CELLS, 8, -60, 60)])
    y = np.concatenate([np.roll(T.special_finite(), 3), r(T.CELLS, 9, -6, 7), r(T.CELLS, 10, -60, 60)])
    return x, y, np.ones_like(x)


def test_fast_policy_divisions_and_sqrt():
    args, got = device('div', 'fast', _fast_div_args, fast=True)
    x, y, _ = args
    x64, y64 = x.astype(f64), y.astype(f64)
    normal = lambda v: (np.abs(v) >= 2.0 ** -126) & (np.abs(v) <= float(T.BIG))    # noqa: E731
    with np.errstate(all='ignore'):
        # rcp = v_rcp_f32: 2 E.  Arguments and results normal (the instruction does not take denormals)
        dom = normal(x64) & normal(1.0 / x64)
        _fast_check('reciprocal', x[dom], _rel(got['rcp'][dom], 1.0 / x64[dom]), np.full(int(dom.sum()), 2 * E))
        # div = a * rcp(b): 2 E + the product's E
        dom = normal(x64) & normal(y64) & normal(1.0 / y64) & normal(x64 / y64)
        _fast_check('x / y', x[dom], _rel(got['div'][dom], (x64 / y64)[dom]), np.full(int(dom.sum()), 3 * E))
        dom = normal(x64) & normal(1.0 / x64) & normal(T.CDIV / x64)
        _fast_check('c / x', x[dom], _rel(got['cdiv'][dom], T.CDIV / x64[dom]), np.full(int(dom.sum()), 3 * E))
        # divc / divk = a * RN(1/c): E for the constant, E for the product
        for op, c in list(zip(('divc_7', 'divc_30', 'divc_m6p8', 'divc_12'), T.DIVC)) + [('divk', T.DIVK)]:
            c64 = float(f32(c))
            dom = normal(x64) & normal(x64 / c64)
            _fast_check('x / %g' % c, x[dom], _rel(got[op][dom], x64[dom] / c64), np.full(int(dom.sum()), 2 * E))
            rc = f32(1.0) / f32(c)
            assert np.array_equal(got[op][dom], (x * rc)[dom])              # ... and exactly that product
    # sqrt = v_sqrt_f32: 2 E
    (u,), got = device('unary', 'cube', _cube_args, fast=True)
    dom = (u >= T.MINNORM)
    _fast_check('sqrt', u[dom], _rel(got['sqrt'][dom], np.sqrt(u[dom].astype(f64))), np.full(int(dom.sum()), 2 * E))


def test_fast_policy_multiply_add_is_one_fma():
    args, got = device('arith', 'mad', T.mad_plane, fast=True)
    x, y, z = args
    two = T.mad_two_roundings(x, y, z)
    want = {'mad3_add': T.fma32(x, y, z), 'mad3_rsub': T.fma32(-x, y, z), 'mad3_sub': T.fma32(x, y, -z),
            'mad_c': T.fma32(x, np.full_like(x, f32(T.MAD_C)), z),
            'mad_cc': T.fma32(x, np.full_like(x, f32(-T.MAD_C2)), np.full_like(x, f32(T.MAD_Z2)))}
    assert np.mean(want['mad3_add'] != two) >= 0.20
    for op, w in want.items():
        _assert_same(got[op], w, args, 'arith.%s (fast policy, against an emulated fma)' % op)
    assert got['mad3_add'][0] == f32(2.0 ** -24) and got['mad3_rsub'][1] == f32(-2.0 ** -24) and got['mad3_sub'][1] == f32(2.0 ** -24)


# ======================================================================================================================
# d. saturation and non-finite contract ("op contract": derived from csrc/models.hpp, IEEE 754 and the
#    fminf / fmaxf rule "a NaN operand loses", before the first run)
# ======================================================================================================================
NAN, INF = f32(np.nan), f32(np.inf)


def _outside_args():
    return np.concatenate([
        T.sweep(88.72, 1e6, 65521)[1:], T.around(88.72, 64), [1e30, 2.3e38, T.BIG],             # above exp's range
        T.sweep(-1e6, -87.33, 65521)[:-1], T.around(-87.33, 64), [-1e30, -2.3e38],              # below it (see -2.4e38 below)
        T.sweep(88.0, 88.72, 997), T.sweep(-200.0, -104.0, 997), T.sweep(-60.0, -50.0, 9973), T.sweep(10.0, 30.0, 9973),
        [0.0, -0.0, -1.0, -T.TINY, -T.BIG, 1e13, -1e13, 1e20, T.BIG, -2.4e38, 3e38]]).astype(f32)


def _near(got, want64, ulps=1.0):
    return T.ulp_err(got, want64) <= ulps


@pytest.mark.parametrize('policy', ['exact', 'fast'])
def test_finite_arguments_outside_the_ulp_domains(policy):
    fast = policy == 'fast'
    (x,), tr = device('trans', 'outside', _outside_args, fast=fast)
    x64 = x.astype(f64)
    with np.errstate(all='ignore'):
        # ---- exp above 88.72
        hi = x > f32(88.72)
        if fast:        # 2^(x log2 e): correct until it overflows, then +inf — IEEE's own answer
            over = hi & (x64 * np.log2(np.e) >= 128.0 + 1e-4)
            assert np.all(tr['exp'][over] == INF)
            ok = hi & ~over & (x64 * np.log2(np.e) < 128.0 - 1e-4)
            assert np.all((_rel(tr['exp'][ok], np.exp(x64[ok])) <= (x64[ok] + 2) * 2.0 ** -23 * SLACK) | (tr['exp'][ok] == INF))
        else:           # saturates: exp(88.72f), the last finite value
            assert np.all(_near(tr['exp'][hi], np.exp(float(f32(88.72))), 2.0))
        # ---- exp below -87.33: the correctly rounded (subnormal or zero) value, or flushed to 0; NaN once x log2(e) overflows
        lo = (x < f32(-87.33)) & (x64 * np.log2(np.e) > -float(T.BIG))
        if fast:        # v_exp_f32's RELATIVE error in the exponent's terms, as inside the range, on a subnormal grid (or flushed)
            d = np.abs(tr['exp'][lo].astype(f64) - np.exp(x64[lo]))
            assert np.all((d <= (np.abs(x64[lo]) + 2) * 2.0 ** -23 * SLACK * np.exp(x64[lo]) + 2.0 ** -149) | (tr['exp'][lo] == 0))
        else:
            assert np.all(_near(tr['exp'][lo], np.exp(x64[lo])) | (tr['exp'][lo] == 0))
        ovf = x64 * np.log2(np.e) < -float(T.BIG) * (1 + 2.0 ** -24)
        assert ovf.sum() == 2
        assert np.all(tr['exp'][ovf] == 0) if fast else np.all(np.isnan(tr['exp'][ovf]))
        # ---- expm1
        lo = x < f32(-104.0)
        assert np.all(tr['expm1'][lo] == -1.0)
        hi = x > f32(88.0)
        if fast:        # exp(x) - 1: as exp
            over = hi & (x64 * np.log2(np.e) >= 128.0 + 1e-4)
            assert np.all(tr['expm1'][over] == INF)
            ok = hi & (x64 * np.log2(np.e) < 128.0 - 1e-4)
            assert np.all(_rel(tr['expm1'][ok], np.expm1(x64[ok])) <= (x64[ok] + 3) * 2.0 ** -23 * SLACK)
        else:           # clamps to 88: expm1(88) even where the true value is still finite (88 < x <= 88.72: up to 51 % low)
            assert np.all(_near(tr['expm1'][hi], np.expm1(88.0), 1.75))
        # ---- log(0), log(< 0); pow overflow; 1/0
        assert np.all(tr['log'][x == 0] == -INF) and np.all(np.isnan(tr['log'][x < 0]))
        assert np.all(tr['pow_1p5'][x >= f32(1e30)] == INF)
        assert np.array_equal(tr['pow_m1'][x == 0], np.where(np.signbit(x[x == 0]), -INF, INF))     # pow(-0, -1) = -inf
    (x,), un = device('unary', 'outside', _outside_args, fast=fast)
    assert np.all(un['pow_3'][x >= f32(1e13)] == INF) and np.all(un['pow_3'][x <= f32(-1e13)] == -INF)
    assert np.all(np.isnan(un['sqrt'][x <= -T.MINNORM])) and np.all(un['sqrt'][x == 0] == 0)
    tiny = un['sqrt'][x == -T.TINY]                 # v_sqrt_f32 takes no denormals: a negative subnormal is its -0
    print('%s sqrt(-2^-149) = %r' % (policy, float(tiny[0])))
    assert np.all((tiny == 0) | np.isnan(tiny)) if fast else np.isnan(tiny).all()
    (x,), dv = device('div', 'outside', _outside_args, fast=fast)
    z = x == 0
    assert np.array_equal(dv['rcp'][z], np.where(np.signbit(x[z]), -INF, INF))
    assert np.array_equal(dv['cdiv'][z], np.where(np.signbit(x[z]), -INF, INF))
    # ---- 1 + tanh outside [-50, 10]: "rounds to 0 / 2 beyond"; tanh itself: +-1
    (x,), hv = device('heav', 'outside', _outside_args, fast=fast)
    for op in ('one_plus_tanh', 'one_plus_tanh_twin'):
        assert np.all(hv[op][x > 10.0] == 2.0) and np.all(hv[op][x < -50.0] == 0.0), op
    assert np.array_equal(hv['tanh'][np.abs(x) >= 45.0], np.sign(x[np.abs(x) >= 45.0]))


def _nf():
    x, y = T.pairs(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -3.0], f32))
    return x, y, np.roll(y, 3)


@pytest.mark.parametrize('policy', ['exact', 'fast'])
def test_nan_and_infinite_arguments(policy):
    fast = policy == 'fast'
    args, tr = device('trans', 'nf', _nf, fast=fast)
    x, y, _ = args
    n, p, m = np.isnan(x), x == INF, x == -INF
    sat_exp, sat_expm1 = np.exp(float(f32(88.72))), np.expm1(88.0)
    if fast:    # v_exp_f32 of a product: IEEE all the way
        assert np.isnan(tr['exp'][n]).all() and np.all(tr['exp'][p] == INF) and np.all(tr['exp'][m] == 0)
        assert np.isnan(tr['expm1'][n]).all() and np.all(tr['expm1'][p] == INF) and np.all(tr['expm1'][m] == -1)
    else:       # fminf / fmaxf drop the NaN: it leaves as the clamp value's result; -inf: inf - inf in exp's correction step
        assert np.all(_near(tr['exp'][n | p], sat_exp, 2.0)) and np.isnan(tr['exp'][m]).all()
        assert np.all(tr['expm1'][n | m] == -1) and np.all(_near(tr['expm1'][p], sat_expm1, 1.75))
    _, hv = device('heav', 'nf', _nf, fast=fast)
    assert np.isnan(hv['tanh'][n]).all() and np.all(hv['tanh'][p] == 1) and np.all(hv['tanh'][m] == -1)
    assert np.isnan(hv['one_plus_tanh_twin'][n]).all()
    if fast:        # 2 - 2 rcp(exp2(NaN) + 1): no clamp on the way
        assert np.isnan(hv['one_plus_tanh'][n]).all()
    for op, top in (('heav', 1.0), ('heav_not', 1.0)) + ((() if fast else (('one_plus_tanh', 2.0),))):   # fmed3-based: finite, in range
        v = hv[op][n]
        assert np.isfinite(v).all() and np.all((v >= 0) & (v <= top)), (op, v[:1])
        print('%s %s(NaN) = %r' % (policy, op, float(v[0])))
    assert np.all(hv['heav'][p] == 1) and np.all(hv['heav'][m] == 0) and np.all(hv['heav_not'][p] == 0) and np.all(hv['heav_not'][m] == 1)
    assert np.all(hv['one_plus_tanh'][p] == 2) and np.all(hv['one_plus_tanh'][m] == 0)
    _, un = device('unary', 'nf', _nf, fast=fast)
    assert np.all(un['sign'][n] == 0) and np.all(un['sign'][p] == 1) and np.all(un['sign'][m] == -1)
    # maximum / minimum / clip: the NaN operand loses (fmaxf, fminf); two NaNs stay one
    _, mm = device('minmax', 'nf', _nf, fast=fast)
    yn = np.isnan(y)
    for op in ('max_t', 'min_t'):
        assert np.array_equal(mm[op][n & ~yn], y[n & ~yn]) and np.array_equal(mm[op][~n & yn], x[~n & yn]) and np.isnan(mm[op][n & yn]).all()
    assert np.all(mm['max_c'][n] == f32(T.MAX_C)) and np.all(mm['min_c'][n] == f32(T.MIN_C)) and np.all(mm['clip_c'][n] == f32(T.CLIP_LO))
    assert np.array_equal(mm['clip_t'][n & ~yn], np.minimum(y[n & ~yn], f32(T.CLIP_THI)))
    assert np.all(mm['max_c'][p] == INF) and np.all(mm['min_c'][m] == -INF) and np.all(mm['clip_c'][p] == f32(T.CLIP_HI))
    # x / c through the reciprocal
    _, dv = device('div', 'nf', _nf, fast=fast)
    for op, c in zip(('divc_7', 'divc_30', 'divc_m6p8', 'divc_12'), T.DIVC):
        assert np.isnan(dv[op][n]).all()
        if fast:        # a * RN(1/c): IEEE
            assert np.all(dv[op][p] == np.copysign(INF, c)) and np.all(dv[op][m] == -np.copysign(INF, c))
            z = (x == 0)
            assert np.array_equal(np.signbit(dv[op][z]), np.signbit(x[z]) ^ (c < 0))
        else:           # r = fma(-q, c, a) = -inf + inf
            assert np.isnan(dv[op][p | m]).all()
            z = (x == 0) & np.signbit(x)
            assert np.all(dv[op][z] == 0) and (not np.signbit(dv[op][z]).any() if c > 0 else True)


# ======================================================================================================================
# e. cell isolation: a lane of the strip kernel owns R cells as one vf<R>; what one cell holds must not reach another
# ======================================================================================================================
@pytest.mark.parametrize('policy', ['exact', 'fast'])
def test_poisoned_cells_do_not_reach_their_neighbours(policy):
    r = np.random.default_rng(21)
    poison = np.array([np.nan, np.inf, -np.inf, T.BIG, -T.BIG], f32)
    clean = tuple(r.uniform(-2.0, 2.0, T.CELLS).astype(f32) for _ in range(3))
    hit = [r.random(T.CELLS) < 0.05 for _ in range(3)]
    dirty = tuple(np.where(h, poison[r.integers(0, 5, T.CELLS)], c) for h, c in zip(hit, clean))
    ref = tuple(np.where(h, f32(1.0), c) for h, c in zip(hit, clean))
    untouched = ~(hit[0] | hit[1] | hit[2])
    assert 0.8 < untouched.mean() < 0.9
    for table in T.TABLE_NAMES:
        a, info = T.run_device(table, *dirty, fast=(policy == 'fast'))
        b, _ = T.run_device(table, *ref, fast=(policy == 'fast'))
        assert info['plan'] == (2, 1)                                    # the fused strip: vf<R> lanes
        for op in a:
            same = a[op].view(np.uint32)[untouched] == b[op].view(np.uint32)[untouched]
            assert same.all(), '%s.%s (%s): %d clean cells changed with their neighbours' % (table, op, policy, int((~same).sum()))


# ======================================================================================================================
# f. forms: scalar step (K=1), stepN over vf<R> (strip), pointwise_kernel (fired group), strip_mt_kernel — the same bits
# ======================================================================================================================
def _form_args():
    s = np.concatenate([T.special_nonfinite(), T.special_finite()])
    x, y = T.pairs(s)
    x = np.concatenate([x, T.sweep(-T.BIG, T.BIG, 34001)])[:2 * T.CELLS]
    y = np.concatenate([y, T.random_normal_range(2 * T.CELLS - y.size, 31, -30, 30)])[:2 * T.CELLS]
    return x, y, np.roll(y, 11)


@pytest.mark.parametrize('policy', ['exact', 'fast'])
def test_every_form_of_a_body_returns_the_same_bits(policy, monkeypatch):
    fast = policy == 'fast'
    args = _form_args()
    assert args[0].size == 2 * T.CELLS and np.isnan(args[0]).any() and np.isinf(args[0]).any()
    bits = lambda d: {k: v.view(np.uint32) for k, v in d.items()}            # noqa: E731
    for table in T.TABLE_NAMES:
        monkeypatch.delenv('FIBHIP_K', raising=False)
        strip, info = T.run_device(table, *args, fast=fast)
        assert info['plan'] == (2, 1), info                                   # (i) both sub-steps in one strip launch
        monkeypatch.setenv('FIBHIP_K', '1')
        tick, info = T.run_device(table, *args, fast=fast)
        assert info['plan'] == (1, 2), info                                   # (ii) one tick_kernel launch per sub-step
        monkeypatch.delenv('FIBHIP_K')
        a, b = bits(strip), bits(tick)
        for op in a:
            assert np.array_equal(a[op], b[op]), '%s.%s (%s): strip and K=1 differ in %d cells' % (
                table, op, policy, int((a[op] != b[op]).sum()))
    # (iii) the fired group of `forms`: pointwise_kernel, for its subset
    strip, _ = T.run_device('forms', *args, fast=fast)
    fired, _ = T.run_device('forms', *args, fast=fast, fired=True)
    assert sorted(fired) == ['expm1', 'one_plus_tanh']
    for op in fired:
        assert np.array_equal(fired[op].view(np.uint32), strip[op].view(np.uint32)), 'forms.%s (%s): fired group differs' % (op, policy)
    # (iv) five ticks in one multi-tick launch (8 variables)
    monkeypatch.delenv('FIBHIP_MT', raising=False)
    mt, info = T.run_device('forms', *args, fast=fast, ticks=5)
    assert info['ticks_per_launch'] > 1 and info['stats']['mt_launches'] >= 1 and info['stats']['mt_ticks'] >= 5, info
    for op in mt:
        assert np.array_equal(mt[op].view(np.uint32), strip[op].view(np.uint32)), 'forms.%s (%s): multi-tick launch differs' % (op, policy)
