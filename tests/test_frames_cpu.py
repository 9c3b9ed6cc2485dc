"""the frame recorder's definition (tests/frame_ref.py) checked against itself and against the code it stands for: the three
forms of image() times the phase field, screen.py's 8-bit quantisation, the block reductions, the sample ticks, and playcube
on an 8-bit cube.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_ref as ref  # noqa: E402

F32 = np.float32


def _states(rng, lo, hi, shape=(37, 53)):
    x = rng.uniform(lo, hi, shape).astype(F32)
    x[0, 0], x[1, 1], x[2, 2] = F32(lo), F32(hi), F32(0)
    x[3, 3] = np.nextafter(F32(lo), F32(hi))
    return x


# (min_v, max_v) of fenton.py (image() is the array itself), br.py and court.py (image() = (V - min_v) / (max_v - min_v))
IMAGES = {'fenton': (0.0, 1.0, lambda v, a, b: v),
          'br': (-90.0, 30.0, lambda v, a, b: (v - a) / (b - a)),
          'court': (-100.0, 50.0, lambda v, a, b: (v - a) / (b - a))}


@pytest.mark.parametrize('kind', sorted(IMAGES))
def test_full_resolution_frame_is_image_times_phase(kind):
    min_v, max_v, formula = IMAGES[kind]
    rng = np.random.default_rng(3)
    phase = np.maximum(rng.uniform(0, 1, (37, 53)), 1e-5).astype(F32)
    lo, span = ref.levels(min_v, max_v)
    for seed in range(4):
        x = _states(np.random.default_rng(seed), min_v - 0.2 * (max_v - min_v), max_v + 0.2 * (max_v - min_v))
        image = formula(x, min_v, max_v)                     # Python floats beside a float32 array, as in the models
        assert image.dtype == F32
        want = image * phase
        got = ref.frame(x, None, (1, 1), 'mean', lo, span, phase)
        assert got.dtype == F32 and got.tobytes() == want.tobytes()
        assert ref.frame(x, None, (1, 1), 'point', lo, span, phase).tobytes() == want.tobytes()
        assert ref.frame(x, None, (1, 1), 'mean', lo, span, None).tobytes() == image.tobytes()


def test_model_hooks_round_like_the_reference():
    from fib_tf_amd.frames import round_levels
    for min_v, max_v in ((-90.0, 30.0), (-100.0, 50.0), (0.0, 1.0), (-83.7, 41.3)):
        lo, span = ref.levels(min_v, max_v)
        assert round_levels(min_v, max_v) == (float(lo), float(span))
    from fib_tf_amd.ionic import IonicModel
    from fib_tf_amd.br import BeelerReuter
    from fib_tf_amd.court import Courtemanche
    from fib_tf_amd import court_ultra
    assert IonicModel._frame_levels(None) == (0.0, 1.0)
    assert BeelerReuter._frame_levels is not IonicModel._frame_levels
    assert Courtemanche._frame_levels is not IonicModel._frame_levels
    assert court_ultra.Courtemanche._frame_levels is Courtemanche._frame_levels


def test_u8_is_the_screens_quantisation():
    from fib_tf_amd.screen import write_png_grey  # noqa: F401  (the expression below is the one it applies)
    rng = np.random.default_rng(5)
    half = ((np.arange(255) + 0.5) / 255).astype(F32)
    vals = np.concatenate([rng.uniform(-0.5, 1.5, 4000).astype(F32), half, np.nextafter(half, F32(0)), np.nextafter(half, F32(2)),
                           np.array([0, 1, -0.0, -1, -1e-30, 2, 1 + 1e-6, np.inf, -np.inf], F32)])
    want = (np.clip(np.asarray(vals, F32), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)        # screen.py write_png_grey
    got = ref.quantise(vals)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert ref.quantise(F32(0)) == 0 and ref.quantise(F32(1)) == 255 and ref.quantise(F32(-3)) == 0 and ref.quantise(F32(7)) == 255
    assert np.array_equal(ref.quantise(np.array([np.nan, -np.nan], F32)), [0, 0])
    x = vals[:4264].reshape(52, 82)
    assert np.array_equal(ref.frame(x, fmt='uint8'), ref.quantise(x))
    x = x.copy()
    x[5, 5] = np.nan
    assert ref.frame(x, fmt='uint8')[5, 5] == 0


def test_reductions():
    rng = np.random.default_rng(7)
    x = rng.uniform(0, 1, (40, 48)).astype(F32)
    const = np.repeat(np.repeat(rng.uniform(0, 1, (8, 16)).astype(F32), 5, axis=0), 3, axis=1)       # constant 5 x 3 blocks
    got = ref.frame(const, None, (5, 3), 'mean')
    # the sum of n equal float32 numbers is not n times the number in general: compare with the same sum, and exactly where
    # the number has few bits
    few = np.round(const * 64) / 64
    assert np.array_equal(ref.frame(few.astype(F32), None, (5, 3), 'mean'), few[::5, ::3].astype(F32))
    assert np.allclose(got, const[::5, ::3], rtol=1e-6)
    point = ref.frame(x, None, (4, 6), 'point')
    assert np.array_equal(point, x[::4, ::6])
    y = x.copy()
    y[1::4] = 9
    y[:, 1::6] = -9
    assert np.array_equal(ref.frame(y, None, (4, 6), 'point'), point)        # POINT ignores the rest of the block
    # MEAN in the stated order, on one block by hand
    b = x[:2, :3]
    by_hand = (((b[0, 0] + b[0, 1]) + b[0, 2]) + ((b[1, 0] + b[1, 1]) + b[1, 2])) / F32(6)
    assert ref.frame(x, None, (2, 3), 'mean')[0, 0] == by_hand
    # the weight comes before the reduction
    w = rng.uniform(0, 1, x.shape).astype(F32)
    assert ref.frame(x, None, (1, 2), 'mean', 0.25, 0.5, w)[3, 4] == \
        (((x[3, 8] - F32(0.25)) / F32(0.5)) * w[3, 8] + ((x[3, 9] - F32(0.25)) / F32(0.5)) * w[3, 9]) / F32(2)


def test_trailing_cells_are_dropped():
    rng = np.random.default_rng(9)
    x = rng.uniform(0, 1, (37, 53)).astype(F32)
    win = (3, 36, 5, 52)                                      # 33 x 47 cells
    assert ref.out_shape(win, (4, 5)) == (8, 9)
    got = ref.frame(x, win, (4, 5), 'mean')
    assert got.shape == (8, 9)
    assert np.array_equal(got, ref.frame(x[3:35, 5:50], None, (4, 5), 'mean'))
    z = x.copy()
    z[35:, :] = 7
    z[:, 50:] = 7
    assert np.array_equal(ref.frame(z, win, (4, 5), 'mean'), got)
    assert ref.frame(x, (10, 26, 7, 23), (16, 16)).shape == (1, 1)


@pytest.mark.parametrize('every,first,want', [(1, 1, [1, 2, 3, 4, 5]), (10, 10, [10, 20, 30]), (10, 1, [1, 11, 21, 31]),
                                               (3, 2, [2, 5, 8, 11])])
def test_sample_ticks(every, first, want):
    ticks = {1: 5, 10: 35, 3: 12}[every]
    assert ref.sample_ticks(every, first, ticks) == want
    # the counter a sampler keeps: it starts at every - first and a sample is due at every multiple of `every`
    k, got = every - first, []
    for t in range(1, ticks + 1):
        k += 1
        if k % every == 0:
            assert k // every - 1 == len(got)               # ... into slot k / every - 1
            got.append(t)
    assert got == want
    if first == 1:                                            # run(im)'s cadence: a frame after loop ticks i with i % every == 0
        assert [t - 1 for t in want] == [i for i in range(ticks) if i % every == 0]


def test_playcube_shows_a_uint8_cube_over_255():
    from fib_tf_amd import playcube
    from fib_tf_amd.screen import Screen
    rng = np.random.default_rng(11)
    cube = rng.integers(0, 256, (3, 6, 7)).astype(np.uint8)
    cube[0, 0, :3] = (0, 255, 128)
    sc = playcube.play(cube, delay=0, screen=Screen(6, 7, keep=3))
    assert sc.count == 3
    for s in range(3):
        assert sc.frames[s].dtype == F32 and np.array_equal(sc.frames[s], cube[s] / F32(255))
    assert sc.frames[0][0, 1] == 1.0 and sc.frames[0][0, 0] == 0.0
    fl = rng.uniform(0, 1, (2, 6, 7)).astype(F32)             # float cubes behave as before
    sc = playcube.play(fl, delay=0, screen=Screen(6, 7, keep=2))
    assert np.array_equal(np.stack(sc.frames), fl)
