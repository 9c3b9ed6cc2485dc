"""egm — the two-electrode electrogram recorder the reference uses to measure conduction velocity
(siravan/fib_tf `egm.py:5-12,37-47`; results in `diff_conduction_velcoty.dat`).

An "electrode" is a Gaussian-weighted mean of `image()` around a pixel.  `record()` samples two of them every
millisecond while the model runs; `delay_ms()` / `conduction_velocity()` turn the two traces into a velocity
(pixels per millisecond — the reference does not record its length unit per pixel)."""
import numpy as np

from ._recorder import SampledRecorder, attach, check_every, run_capacity, run_ticks


def create_mask(model, x, y, radius):
    """float32 [height, width] Gaussian exp(-(dist/radius)^2) centred at column x, row y (egm.py:5-12)"""
    cols, rows = np.meshgrid(np.arange(model.width), np.arange(model.height))
    d = np.hypot(cols - x, rows - y)
    return np.exp(-np.square(d / radius)).astype(np.float32)


def record(model, mask1, mask2, im=None, every_ms=1.0, on_tick=None):
    """run the model to its `duration`, sampling mean(image()*mask) of both electrodes every `every_ms`
    (egm.py:41-47).  `on_tick(i)` is called first on every tick (fire S2 there).  Returns float64 [n, 2]."""
    stride = max(1, int(round(every_ms / (model.dt * model.dt_per_step))))
    rows = []
    for i in model.run(im):
        if on_tick is not None:
            on_tick(i)
        if i % stride == 0:
            frame = model.image()
            rows.append([np.mean(frame * mask1), np.mean(frame * mask2)])
    return np.asarray(rows, dtype=np.float64)


# ---- electrodes on the device (include/fibhip.h fibhip_electrode_*) --------------------------------------------------
def crop_mask(mask):
    """(rect, patch): rect = (r0, r1, c0, c1), the bounding box of the non-zero weights of a full [H, W] mask, and the
    float32 weights inside it.  Exact with respect to the full-grid product: every dropped term is a zero."""
    m = np.asarray(mask, np.float32)
    if m.ndim != 2:
        raise ValueError('crop_mask: a [height, width] mask is expected, got shape %s' % (m.shape,))
    rows, cols = np.flatnonzero(np.any(m != 0, axis=1)), np.flatnonzero(np.any(m != 0, axis=0))
    if rows.size == 0:
        raise ValueError('crop_mask: the mask has no non-zero weight')
    rect = (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1)
    return rect, np.ascontiguousarray(m[rect[0]:rect[1], rect[2]:rect[3]])


class ElectrodeRecorder(SampledRecorder):
    """electrode traces recorded on the device; see `IonicModel.record_electrodes`.

        with model.record_electrodes([mask1, mask2], every=10) as rec:
            for i in model.run():
                ...
            egm = rec.traces()                   # float64 [samples, 2]: mean(image() * mask) after ticks 9, 19, 29, ...

    Every `every` ticks the library takes the weighted sum of state array `var` over the non-zero box of each mask and
    appends it to a trace on the device; nothing is copied to the host until `traces()`.  Between two samples the handle keeps
    its multi-tick launches.

    `traces()` converts the raw sums through `model._image_affine()`: a model whose image() rescales the potential (a
    traced model's image() is the user's own) must override that hook.  With var = 0 the hook is checked against image()
    on the current state when the recorder is attached (two read-backs; `check_affine=False` skips them) and a mismatch
    raises ValueError.  For any other `var` there is no image(): `traces()` returns mean(X_var * mask)."""
    NOUN, END, COUNT = 'electrode recorder', 'electrode_end', 'electrode_count'

    def __init__(self, model, masks, every=1, capacity=None, var=0, check_affine=True):
        self._st = st = attach(model, 'record_electrodes', 'electrode traces are recorded')
        masks = [np.asarray(m, np.float32) for m in masks]
        for m in masks:
            if m.shape != (model.height, model.width):
                raise ValueError('record_electrodes: a mask of shape %s on a %d x %d grid' % (m.shape, model.height, model.width))
        self.every = check_every('record_electrodes', every)
        self.capacity = int(run_capacity(model, self.every) if capacity is None else capacity)
        self.var = int(var)
        crops = [crop_mask(m) for m in masks]
        self.rects = [c[0] for c in crops]
        self.weight_sums = np.array([np.sum(c[1], dtype=np.float64) for c in crops])
        self.cells = model.height * model.width
        self.affine = tuple(float(a) for a in model._image_affine()) if self.var == 0 else (1.0, 0.0)
        if self.var == 0 and check_affine:
            x = np.asarray(st.get_state(0), np.float64)
            want = np.asarray(model.image(), np.float64)
            got = self.affine[0] * x + self.affine[1]
            tol = 1e-5 * (abs(self.affine[0]) * float(np.abs(x).max()) + abs(self.affine[1])) + 1e-30
            if want.shape != got.shape or not np.all(np.abs(got - want) <= tol):
                raise ValueError('record_electrodes: image() is not %g * X + %g on the current state: a model whose image() '
                                 'rescales must override _image_affine()' % self.affine)
        st.electrode_begin(self.var, self.rects, [c[1] for c in crops], self.every, self.capacity)
        self.open = True

    def convert(self, raw):
        """raw float32 sums of w * X -> the reference's mean(image() * mask), in float64: image() = scale * X + offset
        (IonicModel._image_affine), so the mean is (scale * raw + offset * sum(w)) / (H * W)"""
        scale, offset = self.affine
        return (scale * np.asarray(raw, np.float64) + offset * self.weight_sums) / self.cells

    def traces(self, raw=False, first=0, count=None):
        """float64 [samples, n]: mean(image() * mask) of every electrode at every sample taken so far (raw=True: the float32
        sums of w * X as the device took them, as float64); `first`, `count`: a window of the samples"""
        self._check()
        got = self._st.electrode_read(first, count)
        return got.astype(np.float64) if raw else self.convert(got)


def record_on_device(model, mask1, mask2, im=None, every_ms=1.0, on_tick=None):
    """`record()` with the electrodes on the device: same signature, same stride rule, same sample times, same float64
    [n, 2] result — without a grid read-back per sample (a model whose image() rescales must override `_image_affine()`:
    see ElectrodeRecorder).  `record()` samples after ticks 0, stride, 2 * stride, ...; a recorder
    samples after ticks every - 1, 2 * every - 1, ...  For stride 1 the two coincide.  For a larger stride the first tick is
    recorded by a recorder of its own with every = 1 (one sample), and a second one with every = stride is attached after it:
    its samples fall after ticks stride, 2 * stride, ..."""
    stride = max(1, int(round(every_ms / (model.dt * model.dt_per_step))))
    ticks = run_ticks(model)
    if ticks < 1:
        return np.zeros((0, 2), np.float64)
    head = None
    rec = model.record_electrodes([mask1, mask2], every=1, capacity=ticks if stride == 1 else 1)
    try:
        for i in model.run(im):
            if on_tick is not None:
                on_tick(i)
            if stride > 1 and i == 0:
                head = rec.traces()
                rec.close()
                rec = model.record_electrodes([mask1, mask2], every=stride, capacity=max(1, (ticks - 1) // stride))
        out = rec.traces()
    finally:
        rec.close()
    return out if head is None else np.concatenate([head, out])


def _upstroke_time(trace, level):
    """first upward crossing of `level`, linearly interpolated, in samples; None if it never happens"""
    above = trace >= level
    idx = np.flatnonzero(~above[:-1] & above[1:])
    if idx.size == 0:
        return None
    k = int(idx[0])
    return k + (level - trace[k]) / (trace[k + 1] - trace[k])


def delay_ms(traces, every_ms=1.0, frac=0.5):
    """activation delay between the two electrodes: each trace's first crossing of `frac` of its own swing"""
    t = []
    for col in (0, 1):
        x = traces[:, col]
        lo, hi = float(x.min()), float(x.max())
        at = _upstroke_time(x, lo + frac * (hi - lo))
        if at is None:
            raise ValueError('electrode %d never activated' % (col + 1))
        t.append(at)
    return (t[1] - t[0]) * every_ms


def conduction_velocity(traces, distance_px, every_ms=1.0, frac=0.5):
    """pixels per millisecond between two electrodes `distance_px` apart along the propagation direction"""
    return distance_px / delay_ms(traces, every_ms, frac)


def main():
    """the reference's own protocol (egm.py:15-50): Beeler-Reuter 512x512, obstacle, S2, electrodes 30 px apart"""
    from .br import BeelerReuter
    from .screen import Screen
    config = {'width': 512, 'height': 512, 'dt': 0.1, 'dt_per_plot': 10, 'diff': 1.0, 'duration': 3000,
              'skip': False, 'cheby': True, 'timeline': False, 'timeline_name': 'timeline_br.json',
              'save_graph': False}
    model = BeelerReuter(config)
    model.add_hole_to_phase_field(150, 256, 50)
    model.define()
    model.add_pace_op('s2', 'luq', 10.0)
    im = Screen(model.height, model.width, 'Beeler-Reuter Model')
    s2 = model.millisecond_to_step(300)
    m1, m2 = create_mask(model, 300 + 15, 256, 5), create_mask(model, 300 - 15, 256, 5)
    out = record(model, m1, m2, im, on_tick=lambda i: model.fire_op('s2') if i == s2 else None)
    np.savetxt('test.dat', out)


if __name__ == '__main__':
    main()
