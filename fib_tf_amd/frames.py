"""frames — the movie recorded on the device while a model runs.

The reference's main product is a movie: `run(im)` paints `image() * phase` every `dt_per_plot` sub-steps, the drivers collect
the frames into `cube.npy` and `playcube` replays it.  `FrameRecorder` has the library write that frame on the device every
`every` ticks (`frame_kernel`) into a cube kept there until it is read: no read-back and no synchronisation per frame, and
between two frames the handle keeps its multi-tick launches.  The frame is a window of one state
array, optionally block-reduced, mapped the way `image()` maps it, optionally weighted by the phase field, as float32 or as
8-bit grey.  The definition is exact (include/fibhip.h, fibhip_frames_*; restated in NumPy in tests/frame_ref.py)."""
import numpy as np

from ._recorder import SampledRecorder, attach, check_every, run_ticks, tick_ms, weight_plane


def round_levels(min_v, max_v):
    """(lo, span) of a model whose image() is (V - min_v) / (max_v - min_v): the subtraction in double, both rounded to
    float32 — what NumPy makes of the Python floats in that expression"""
    return float(np.float32(min_v)), float(np.float32(float(max_v) - float(min_v)))


class FrameRecorder(SampledRecorder):
    """frames recorded on the device; see `IonicModel.record_frames`.

        with model.record_frames(every=10, first=1) as rec:      # run(im)'s own cadence: after ticks 0, 10, 20, ...
            for i in model.run():
                ...
            rec.save('cube')                     # what the drivers' np.save('cube', cube) writes; playcube replays it

    `frames()` returns [n, oh, ow] float32 (or uint8 with fmt='uint8'); `times()` the model time of every frame in ms since
    the recorder was attached: frame s follows tick first + s * every.  `count()` counts frames."""
    NOUN, END, COUNT = 'frame recorder', 'frames_end', 'frames_count'

    def __init__(self, model, every=1, first=None, window=None, block=(1, 1), reduce='mean', fmt='float32', var=0, weight='phase',
                 levels=None, capacity=None):
        self._st = st = attach(model, 'record_frames', 'frames are recorded')
        self.every = check_every('record_frames', every)
        self.first = self.every if first is None else int(first)
        if not 1 <= self.first <= self.every:
            raise ValueError('record_frames: first must be 1 .. every = %d (got %d)' % (self.every, self.first))
        self.var = int(var)
        self.window = (0, model.height, 0, model.width) if window is None else tuple(int(v) for v in window)
        self.block = (int(block[0]), int(block[1]))
        self.reduce, self.fmt = reduce, {'f32': 'float32', 'u8': 'uint8'}.get(fmt, fmt)
        self.weight = weight = weight_plane(model, weight, 'record_frames')
        given = levels is not None
        lo, span = levels if given else model._frame_levels()
        self.levels = (float(np.float32(lo)), float(np.float32(span)))
        if self.var == 0:
            # image() is what the frames stand for: the levels must reproduce it bit for bit on the state as it is now
            x = np.asarray(st.get_state(0), np.float32)
            want = np.asarray(model.image(), np.float32)
            with np.errstate(all='ignore'):
                got = (x - np.float32(self.levels[0])) / np.float32(self.levels[1])
            if want.shape != got.shape or want.tobytes() != got.tobytes():
                raise ValueError('record_frames: image() is not (X - %g) / %g on the current state, bit for bit: a model whose '
                                 'image() rescales must pass levels=(lo, span) (or override _frame_levels())' % self.levels)
        self.tick_ms = tick_ms(model)
        if capacity is None:                     # the frames of a whole run of model.duration, at least 1
            ticks = run_ticks(model)
            capacity = max(1, (ticks - self.first) // self.every + 1 if ticks >= self.first else 1)
        self.capacity = int(capacity)
        st.frames_begin(self.var, self.window, self.block, self.reduce, self.levels[0], self.levels[1], weight, self.fmt,
                        self.every, self.first, self.capacity)
        oh, ow, self.dtype = st.frames_shape()
        self.shape = (oh, ow)
        self.open = True

    def frames(self, first=0, count=None):
        """[n, oh, ow] float32 or uint8: frames [first, first + count) (count=None: all taken so far)"""
        self._check()
        return self._st.frames_read(first, count)

    def times(self, first=0, count=None):
        """float64 [n]: the model time in ms since attach at which each of those frames was taken"""
        return (self.first + (int(first) + np.arange(max(self._span(first, count), 0))) * self.every) * self.tick_ms

    def save(self, path):
        """writes the cube `playcube` replays (np.save: '.npy' is appended when missing); a uint8 cube stays uint8"""
        np.save(path, self.frames())

    def play(self, screen=None, **kw):
        """replays the frames taken so far through fib_tf_amd.playcube.play; returns the Screen"""
        from . import playcube
        kw.setdefault('delay', 0)
        return playcube.play(self.frames(), screen=screen, **kw)
