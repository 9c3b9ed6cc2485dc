"""not-gpu: the op tables of tests/op_tables.py on the CPU — do they cover every op and every peephole the code
generator has, do they compile for gfx950, can their argument planes tell the forms apart that the device tests are
meant to tell apart, and is the ulp metric itself right."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import op_tables as T  # noqa: E402

f32, f64 = np.float32, np.float64
STRUCTURAL = {'param', 'var', 'bnd', 'lap', 'conv3', 'apply', 'index'}     # leaves, the stencil, and what emit() refuses
HOOKS = ('P::mad(', 'P::mad3(', 'P::divc(', 'P::divk(', 'P::div(', 'P::one_plus_tanh(', 'g_heav(', 'g_heav_not(', 'g_sign(',
         'P::tanhv(', 'clipf(', 'g_min(g_max(', 'g_pow(')


def _emitter_ops():
    """every op name _Emitter.emit accepts, read from the generator itself: its three dictionaries and the names its
    dispatch compares `op` with"""
    from fib_tf_amd import traced
    ops = set(traced._BINOPS) | set(traced._CMP) | set(traced._UNARY)
    src = inspect.getsource(traced._Emitter.emit)
    for m in re.finditer(r"op == '(\w+)'", src):
        ops.add(m.group(1))
    for m in re.finditer(r"op in \(([^)]*)\)", src):
        ops |= set(re.findall(r"'(\w+)'", m.group(1)))
    return ops - STRUCTURAL


def _graph_ops(model):
    from fib_tf_amd.traced import _walk
    c = model._analyze()
    ops, seen = set(), set()
    for _, prog in c['programs']:
        for lv in prog.levels:
            for e in lv.outs.values():
                _walk(e, seen, lambda n: ops.add(n.op))
    return ops


@pytest.fixture(scope='module')
def tables():
    return {n: T.make_table(n) for n in T.TABLE_NAMES}


def test_tables_cover_every_op_of_the_emitter(tables):
    want = _emitter_ops()
    # the generator's list is what this test expects it to be made of (a renamed dictionary must not empty it)
    assert {'add', 'gt', 'tanh', 'div', 'and', 'or', 'not', 'where', 'square', 'pow', 'maximum', 'minimum', 'clip'} <= want
    import fib_tf_amd.tfgraph as tf
    assert set(tf._NP_UNARY) - {'neg'} <= want | {'neg'} and tf._MASK_OPS <= want
    have = set()
    for m in tables.values():
        have |= _graph_ops(m)
    assert not want - have, 'ops no table contains: %s' % sorted(want - have)
    # pow in each of its forms, division in each of its operand shapes
    src = '\n'.join(m.generated_source() for m in tables.values())
    for e in ('1.5f', '0.5f', '(-1.0f)'):
        assert 'g_pow(s[1], %s)' % e in src
    assert re.search(r'P::div\(3\.0f, s\[1\]\)', src) and re.search(r'P::div\(s\[1\], s\[2\]\)', src)


def test_generated_source_takes_every_peephole(tables):
    src = {n: m.generated_source() for n, m in tables.items()}
    text = '\n'.join(src.values())
    for h in HOOKS:
        assert h in text, 'no table makes the generator emit %s' % h
    # the unfused twins really are unfused: the plain forms stand next to the peepholes in the same table
    heav = src['heav']
    assert heav.count('g_heav(') == 1 and heav.count('g_heav_not(') == 1              # (two chained sub-steps of ONE kind)
    assert heav.count('g_sign(') == 1 and re.search(r'= 1\.0f \+ t\d+;\s+const T t\d+ = t\d+ \* 0\.5f;', heav)
    assert re.search(r'= 1\.0f - t\d+;\s+const T t\d+ = t\d+ \* 0\.5f;', heav)
    assert re.search(r'const T (t\d+) = P::tanhv\(s\[1\]\);\s+const T t\d+ = 1\.0f \+ \1;', heav)
    assert heav.count('P::one_plus_tanh(') == 1 and heav.count('P::tanhv(') == 1
    arith = src['arith']
    assert arith.count('P::mad3(') == 3 and 'P::mad3(-s[1], s[2], s[3])' in arith and 'P::mad3(s[1], s[2], -s[3])' in arith
    assert 'P::mad(s[1], 1.70000005f, s[3])' in arith and 'P::mad(s[1], (-2.5f), 0.75f)' in arith
    for c in T.DIVC:
        from fib_tf_amd.traced import _lit
        assert 'P::divc(s[1], %s,' % _lit(c) in src['div']
    assert 'P::divk(s[1], %s)' % _lit(T.DIVK) in src['div']
    # the second assign group exists (pointwise_kernel) and every table chains two sub-steps (strip + multi-tick form)
    assert 'NMODES = 2' in src['forms'] and 'MODE == 1' in src['forms']
    for n, s in src.items():
        assert '#define FIB_CUSTOM_K 2' in s and 'DEFAULT_STEPS = 2' in s, n


def test_divc_constants_are_what_the_tables_claim():
    from fib_tf_amd.traced import divc_is_exact
    for c in T.DIVC:
        assert divc_is_exact(c), c
    assert not divc_is_exact(T.DIVK)
    assert np.isfinite(f32(1.0) / f32(T.DIVK)) and abs(T.DIVK) > 0.1, 'the divk constant is an ordinary one'


@pytest.mark.parametrize('name', T.TABLE_NAMES)
def test_table_is_small_and_compiles_for_gfx950(name, tmp_path, monkeypatch):
    """the build the device tests use (hiprtc in this process, gfx950 as an option — no GPU needed), into a temporary
    cache directory"""
    from fib_tf_amd import traced
    m = T.make_table(name)
    c = m._analyze()
    assert len(c['slots']) <= T.MAX_VARS and c['spt'] == 2
    if name == 'forms':
        assert len(c['slots']) <= 8 and [n for n, _ in c['programs']] == ['_ode_op', 'ops']
    monkeypatch.setattr(traced, 'CACHE', str(tmp_path))
    assert traced._build(c['source'], device=None) is None
    made = sorted(os.listdir(str(tmp_path)))
    hsaco = [f for f in made if f.endswith('.hsaco')]
    assert len(hsaco) == 1 and os.path.getsize(os.path.join(str(tmp_path), hsaco[0])) > 10000, made
    import json
    with open(os.path.join(str(tmp_path), hsaco[0][:-6] + '.json')) as f:
        kinds = {(k['kind'], k['fast']) for k in json.load(f)['kernels']}
    want = {(0, 0), (0, 1), (1, 0), (1, 1), (3, 0), (3, 1)} | ({(2, 0), (2, 1)} if name == 'forms' else set())
    assert kinds == want                      # tick, strip and multi-tick kernels under both policies (+ the fired group)


# ---- teeth: the planes distinguish what the device tests are meant to distinguish --------------------------------------
def test_fma_emulation_is_exact():
    """fma32 against exact rational arithmetic on cases built to hit double rounding"""
    from fractions import Fraction
    r = np.random.default_rng(3)
    x = r.uniform(-2, 2, 2000).astype(f32)
    y = r.uniform(-2, 2, 2000).astype(f32)
    z = (-(x.astype(f64) * y.astype(f64))).astype(f32)                    # heavy cancellation
    z[::2] = r.uniform(-2, 2, 1000).astype(f32)
    z[1::4] *= f32(2.0 ** -30)                                             # z far below the product: sticky-bit cases
    got = T.fma32(x, y, z)
    for i in range(x.size):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        lo = f32(float(exact))                                             # float(Fraction) is correctly rounded to double...
        # ...so decide between the two float32 neighbours exactly
        cands = sorted({float(lo), float(np.nextafter(lo, f32(np.inf))), float(np.nextafter(lo, f32(-np.inf)))})
        best = min(cands, key=lambda c: (abs(Fraction(c) - exact), int(f32(c).view(np.uint32)) & 1))
        assert float(got[i]) == best, (x[i], y[i], z[i])


def test_mad_plane_separates_two_roundings_from_one():
    x, y, z = T.mad_plane()
    two, one = T.mad_two_roundings(x, y, z), T.fma32(x, y, z)
    assert np.mean(two != one) >= 0.20
    # the cancellation triple: two roundings give 0, a fused multiply-add gives 2^-24
    assert x[0] == y[0] == f32(1 + 2.0 ** -12) and z[0] == f32(-(1 + 2.0 ** -11))
    assert two[0] == 0.0 and one[0] == f32(2.0 ** -24)
    assert T.mad_two_roundings(x, y, -z)[1] == 0.0 and T.fma32(x, y, -z)[1] == f32(2.0 ** -24)      # cell 1: x*y - z, z - x*y
    # the same plane serves z - x*y and x*y - z (negating an operand commutes with rounding) and the constant forms
    c = f32(T.MAD_C)
    assert np.mean(((x * c).astype(f32) + z) != T.fma32(x, np.full_like(x, c), z)) >= 0.20


@pytest.mark.parametrize('c', T.DIVC)
def test_divc_plane_separates_division_from_reciprocal_multiply(c):
    x = T.divc_plane()
    c32 = f32(c)
    rc = f32(1.0) / c32
    assert np.mean((x / c32) != (x * rc)) >= 0.20


def _divc3(x, c32):
    """Exact::divc in exact float32 emulation: q = x*rc, r = fma(-q, c, x), fma(r, rc, q)"""
    rc = f32(1.0) / c32
    with np.errstate(all='ignore'):
        q = x * rc
        r = T.fma32(-q, np.full_like(x, c32), x)
        return T.fma32(r, np.full_like(x, rc), q)


@pytest.mark.parametrize('c', T.DIVC)
def test_three_instruction_division_needs_its_argument_scaled(c):
    """why generated code takes Exact::divc(a, c, rc, any_range): below |a| = 2^-102 the residual of the plain form is
    no longer exact and a NORMAL quotient can be one ulp off; with a tiny argument scaled by 2^64 first it is RN(a/c)
    wherever that is normal and within one subnormal ulp below — the claim the device test holds"""
    c32 = f32(c)
    x = np.concatenate([T.random_normal_range(400000, 7, -126, -100), T.random_normal_range(100000, 8, -100, 128),
                        T.special_finite()])
    with np.errstate(all='ignore'):
        want = x / c32
        normal = np.abs(x.astype(f64) / float(c32)) >= 2.0 ** -126
        plain = _divc3(x, c32)
        tiny = np.abs(x) < f32(2.0 ** -60)
        scaled = np.where(tiny, _divc3(x * np.where(tiny, f32(2.0 ** 64), f32(1)), c32) * f32(2.0 ** -64), plain)
    big = np.abs(x) >= f32(2.0 ** -102)
    assert np.array_equal(plain[big & normal], want[big & normal])
    if c == -6.8:                                   # a constant with a full significand: the plain form does go wrong
        assert (plain[normal] != want[normal]).sum() > 100
    assert np.array_equal(scaled[normal], want[normal])
    assert np.abs(scaled[~normal].astype(f64) - want[~normal].astype(f64)).max() <= 2.0 ** -149
    assert np.array_equal(scaled[~tiny].view(np.uint32), plain[~tiny].view(np.uint32))


def test_divk_constant_separates_division_from_reciprocal_multiply():
    x = T.divc_plane()
    c32 = f32(T.DIVK)
    assert np.mean((x / c32) != (x * (f32(1.0) / c32))) >= 0.20


def test_exp_samples_would_catch_a_missing_correction_step():
    """exp_core without its correction is 2^RN(x log2 e): even with a PERFECT 2^t the rounding of the product alone is
    |t| 2^-24 ln 2 relative, tens of ulps at |x| ~ 60 — the samples of the device test reach that, its bound is 2"""
    x = T.samples_trans()
    x = x[(x >= f32(-87.33)) & (x <= f32(88.72))]
    assert x.size >= 1000000
    t = (x * f32(1.44269504088896340736)).astype(f64)                       # the one float32 product
    with np.errstate(under='ignore'):
        uncorrected = np.exp2(t).astype(f32)
    err = T.ulp_err(uncorrected, np.exp(x.astype(f64)))
    # (the sweep is uniform in bit patterns: about 5 % of it lies in [32, 88.72], where the product's ulp is 2^-18 or more)
    assert err.max() > 20.0 and np.mean(err > 2.0) > 0.02
    # and against a correctly rounded exp the metric stays at half an ulp
    assert T.ulp_err(np.exp(x.astype(f64)).astype(f32), np.exp(x.astype(f64))).max() <= 0.5


def test_sign_and_heaviside_samples_hold_zeros_and_subnormals():
    """a sign that returned 1 at 0, or a build that flushed denormals, shows on these arguments only"""
    x = T.special_finite()
    assert (x == 0).sum() >= 2 and np.signbit(x[x == 0]).any()
    assert ((np.abs(x) < T.MINNORM) & (x != 0)).sum() >= 4
    out = T.run_interpreter('unary', x)
    assert np.all(out['sign'][x == 0] == 0) and np.all(np.abs(out['sign'][x != 0]) == 1)


# ---- the metric -------------------------------------------------------------------------------------------------------
def test_true_ulp_metric():
    v = np.array([1.0, 1.5, 3.0, 1e-3, 1e10, 2.0 ** -126, 2.0 ** -130, 0.75], f32)
    assert np.all(T.ulp_err(v, v.astype(f64)) == 0.0)
    up, dn = np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))
    assert np.all(T.ulp_err(up, v.astype(f64)) == 1.0)
    # below a power of two the spacing halves: measured at the TRUE value's binade, the lower neighbour of 1.0 is
    # half an ulp away, and 1.0 is ONE ulp away from a true value just below it
    assert T.ulp_err(dn[0], 1.0) == 0.5 and T.ulp_err(f32(1.0), float(dn[0])) == 1.0
    assert T.ulp_unit(1.0) == 2.0 ** -23 and T.ulp_unit(float(dn[0])) == 2.0 ** -24 and T.ulp_unit(2.0) == 2.0 ** -22
    # true values between two floats, subnormal and zero true values (unit 2^-149)
    assert T.ulp_err(f32(1.0), 1.0 + 2.0 ** -24) == 0.5
    assert T.ulp_unit(0.0) == T.ulp_unit(2.0 ** -140) == T.ulp_unit(2.0 ** -126) == 2.0 ** -149
    assert T.ulp_err(f32(0.0), 2.0 ** -149) == 1.0 and T.ulp_err(f32(2.0 ** -149), 0.0) == 1.0
    assert T.ulp_unit(-3.0) == 2.0 ** -22


def test_planes_and_special_set():
    s = T.special_finite()
    b = set(s.view(np.uint32).tolist())
    for pat in (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x3F800000,
                0xBF800000, 0x3F7FFFFF, 0x3F800001, 0x7F7FFFFF, 0xFF7FFFFF):
        assert pat in b, hex(pat)
    for c in T.DIVC + (T.DIVK, T.MAD_C):
        k = int(f32(c).view(np.uint32))
        assert {k - 1, k, k + 1} <= b
    assert np.isfinite(s).all() and not np.isfinite(T.special_nonfinite()).any()
    a = T.around(0.625)
    assert a.size == 513 and np.all(np.diff(a) > 0) and a[256] == f32(0.625)
    z = T.around(0.0, 4)
    assert z.size == 9 and z[4] == 0 and z[3] == -T.TINY and z[5] == T.TINY and np.all(np.diff(z.astype(f64)) > 0)
    sw = T.sweep(-1.0, 2.0, 1 << 20)
    assert sw[0] == -1.0 and np.all(np.diff(sw.astype(f64)) > 0) and sw[-1] <= 2.0
    p = T.to_planes(np.arange(T.CELLS + 5))
    assert p.shape == (2, T.H, T.W) and p[1].ravel()[5] == 1.0


def test_interpreter_runs_every_table():
    """the float32 reference of the bit-exact class: every table, on the special set, the heaviside twins equal"""
    x, y = T.pairs(T.special_finite())
    z = np.roll(y, 7)
    for name in T.TABLE_NAMES:
        out = T.run_interpreter(name, x[:T.CELLS], y[:T.CELLS], z[:T.CELLS])
        assert all(v.size == min(x.size, T.CELLS) for v in out.values())
        if name == 'heav':
            assert np.array_equal(out['heav'], out['heav_twin']) and np.array_equal(out['heav_not'], out['heav_not_twin'])
            assert set(np.unique(out['heav'])) == {0.0, 0.5, 1.0}
