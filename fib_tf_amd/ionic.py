"""IonicModel — the reference's config-dict / define() / run() stepper API (siravan/fib_tf
`ionic.py:30-307`) on top of libfibhip.so.

Driver code written for the reference runs unchanged against this module:

    model = Fenton4v(config)
    model.add_hole_to_phase_field(256, 256, 30)
    model.define()
    model.add_pace_op('s2', 'luq', 1.0)
    for i in model.run(im):
        if i == s2:
            model.fire_op('s2')

What differs underneath: `define()` does not build a TensorFlow graph, it creates a fibhip
handle whose state lives as one SoA slab in HBM; one `run()` tick is one call of `fibhip_step`
(one fused stencil+reaction launch per tick or per few sub-steps) instead of `Session.run`.
All numerical work happens in the HIP library; there is no CPU fallback here.
"""
import json
import os
import time

import numpy as np

from . import _lib


class StateVar:
    """stand-in for the `tf.Variable` handles the reference hands out (`pot()`, `_State[s]`):
    `.eval()` copies the array from the device (ionic.py:229, fenton.py:153)."""

    def __init__(self, model, index, name):
        self._model, self.index, self.name = model, index, name

    def eval(self):
        return self._model._stepper.get_state(self.index)

    def __array__(self, dtype=None, copy=None):
        a = self.eval()
        return a if dtype is None else a.astype(dtype)


class IonicModel:
    """base class for cardiac electrophysiology simulation (ionic.py:30-42)"""

    MODEL_ID = None
    VAR_NAMES = ()

    def __init__(self, config):
        for key, val in config.items():         # every key becomes an attribute, ionic.py:35-37
            setattr(self, key, val)
        self.phase = None
        self.tensor = None              # (dyy, dxx, dxy): per-cell diffusion tensors (set_tensor / set_fibres), or None
        self._ops = {}
        self.defined = False
        self.dt_per_step = 1
        self.cl_observer = None
        self._stepper = None
        self._library = None            # a specialised build of libfibhip (None = the stock library)
        # config['fast_math'] (default True): hardware exp/log/rcp/sqrt and reciprocal-multiply for the
        # model constants; False selects the rounding-faithful policy (IEEE-equivalent division, ocml
        # expf/tanhf/expm1f/logf): one float32 rounding per reference op.  Both are parity-tested; the
        # stencil and the phase-field term are bit-identical to the reference under either.
        for key, default in (('timeline', False), ('timeline_name', 'timeline.json'), ('save_graph', False),
                             ('device', int(os.environ.get('LOCAL_RANK', '0'))), ('fast_math', True)):
            if not hasattr(self, key):
                setattr(self, key, default)
        # config['fibre_angle'] (radians from the +column axis towards the +row axis) and config['anisotropy'] (longitudinal
        # over transverse diffusion): uniform fibres over the whole sheet
        if hasattr(self, 'fibre_angle') or hasattr(self, 'anisotropy'):
            self.set_fibres(getattr(self, 'fibre_angle', 0.0), getattr(self, 'anisotropy', 1.0))

    # ---- building blocks, callable on host arrays (ionic.py:44-123); executed on the GPU -------
    def laplace(self, X0):
        """9-point Laplacian of X0 (+ phase-field correction when self.phase is set), ionic.py:44-60"""
        if self.tensor is not None:             # div(D grad X0) in the form of DESIGN.md 25, incl. its first-order term
            return _lib.unit_laplace_tensor(X0, *self.tensor, phi=self.phase, fast=self.fast_math, device=self.device)
        return _lib.unit_op(1, X0, phi=self.phase, fast=self.fast_math, device=self.device)

    def phase_field(self, X):
        """phase-field correction for the REFLECT-padded array X, ionic.py:70-81"""
        X = np.asarray(X, np.float32)
        return _lib.unit_op(2, X[1:-1, 1:-1], phi=self.phase, fast=self.fast_math, device=self.device)

    def enforce_boundary(self, X):
        """no-flux (Neumann) boundary: interior re-padded SYMMETRIC, ionic.py:107-113"""
        return _lib.unit_op(0, X, device=self.device)

    def rush_larsen(self, g, g_inf, g_tau, dt, name=None):
        """clip(g + (g - g_inf) * expm1(-dt/tau), 1e-5, 0.99999), ionic.py:115-123"""
        g = np.asarray(g, np.float32)
        gi = np.broadcast_to(np.asarray(g_inf, np.float32), g.shape)
        gt = np.broadcast_to(np.asarray(g_tau, np.float32), g.shape)
        n = g.size
        rows = max(3, -(-n // 3))                # the device op works on a [rows, 3] sheet

        def sheet(a):
            buf = np.ones(rows * 3, np.float32)
            buf[:n] = np.ravel(a)
            return buf.reshape(rows, 3)

        out = _lib.unit_op(3, sheet(g), sheet(gi), sheet(gt), dt=dt, fast=self.fast_math, device=self.device)
        return out.ravel()[:n].reshape(g.shape)

    # ---- geometry (host side, as in the reference) ---------------------------------------------
    def add_hole_to_phase_field(self, x, y, radius, neg=False):
        """multiplies a circular hole centred at column x, row y into the phase field; with
        neg=True the disc is kept and its outside is excluded (ionic.py:83-105).
        Must be called before define()."""
        if self.defined:
            raise AssertionError('add_hole_to_phase_field should be called before calling define')
        cols = np.arange(self.width)[np.newaxis, :] - x         # broadcasting instead of a meshgrid: same
        rows = np.arange(self.height)[:, np.newaxis] - y        # float64 values, bit for bit
        dist = np.hypot(cols, rows)
        # smooth indicator of the kept region: outside the disc, or (neg) inside it with a 10x softer edge
        arg = 0.1 * (radius - dist) if neg else dist - radius
        mask = np.array(0.5 * (np.tanh(arg) + 1.0), dtype=np.float32)
        base = np.ones([self.height, self.width], dtype=np.float32) if self.phase is None else self.phase
        # floor at 1e-5: phase_field divides by 4ϕ (ionic.py:104-105)
        self.phase = np.maximum(base * mask, 1e-5)

    # ---- fibres: anisotropic, heterogeneous conduction (fib_tf_amd/tensor.py) ----------------------------
    def set_tensor(self, dyy, dxx, dxy):
        """per-cell diffusion tensors D = [[dyy, dxy], [dxy, dxx]] (rows are y, columns are x), three [height, width] planes,
        dimensionless and relative to `diff`: the diffusion term becomes diff * div(D grad V).  The planes must be finite and
        positive definite with a largest eigenvalue of at most 1 (raise `diff` instead).  set_tensor(None, None, None) removes
        the tensor.  Must be called before define(); single device only, not on traced models; record_leads,
        record_potential_map, program_lesions and ablate do not go with it."""
        from . import tensor as _tensor
        if self.defined:
            raise AssertionError('set_tensor should be called before calling define')
        if dyy is None and dxx is None and dxy is None:
            self.tensor = None
            return
        planes = _tensor.check_tensor(dyy, dxx, dxy, shape=(self.height, self.width))
        _tensor.warn_if_not_monotone(*planes)
        self.tensor = tuple(planes)

    def set_fibres(self, angle, ratio, scale=1.0):
        """fibres at `angle` (radians from the +column axis towards the +row axis) with longitudinal over transverse diffusion
        `ratio` >= 1 and longitudinal diffusion `scale` * diff, scale in (0, 1]; each a scalar or a [height, width] array
        (tensor.fibre_tensor).  Must be called before define()."""
        from . import tensor as _tensor
        if self.defined:
            raise AssertionError('set_fibres should be called before calling define')
        self.set_tensor(*_tensor.fibre_tensor(angle, ratio, scale, shape=(self.height, self.width)))

    # ---- pacing ----------------------------------------------------------------------------------
    def pace_rect(self, loc):
        """rows/cols [r0,r1) x [c0,c1) of a named pacing site, ionic.py:145-160"""
        H, W = self.height, self.width
        table = {
            'left': (0, H, 0, min(5, W)),
            'right': (0, H, max(W - 5, 0), W),
            'top': (0, min(5, H), 0, W),
            'bottom': (max(H - 5, 0), H, 0, W),
            'luq': (1, H // 2, 1, W // 2),
            'llq': (H // 2, H - 1, 1, W // 2),
            'ruq': (1, H // 2, W // 2, W - 1),
            'rlq': (H // 2, H - 1, W // 2, W - 1),
        }
        return table.get(loc)

    def add_pace_op(self, name, loc, v):
        """registers the stimulus `pot = max(pot, s)`, s = v on the site and min_v elsewhere
        (ionic.py:125-163).  Must be called after define()."""
        if not self.defined:
            raise AssertionError('add_hole_to_phase_field should be called after calling define')
        rect = self.pace_rect(loc)
        if rect is None:
            print('undefined pace location')
            rect = (0, 0, 0, 0)                 # s = min_v everywhere, exactly as the reference
        self._ops[name] = ('pace', rect, float(v))

    def fire_op(self, name):
        """runs an operation registered by add_pace_op (ionic.py:165-169)"""
        op = self._ops[name]
        if op[0] == 'pace':
            (r0, r1, c0, c1), v = op[1], op[2]
            self._stepper.pace(r0, r1, c0, c1, v, float(self.min_v))
        else:
            op[1]()

    # ---- main loop -------------------------------------------------------------------------------
    def run(self, im=None, keep_state=False, block=True):
        """generator over ticks, ionic.py:171-245:

            for i in model.run(im):
                if i == s2:
                    model.fire_op('s2')

        One tick = `dt_per_step` sub-steps of dt.  Ticks are enqueued asynchronously; the
        generator only synchronises when the caller reads something back."""
        if not self.defined or self._stepper is None:
            raise AssertionError('run should be called after calling define')
        then = time.time()
        st = self._stepper
        self.samples = int(self.duration / (self.dt_per_step * self.dt))
        every = int(self.dt_per_plot / self.dt_per_step) if im else 0
        watch = {'v0': self.min_v, 'last_spike': 0}
        # run() owns the cadence (ionic.py:199-206) and says so: with a screen the ticks up to the next frame are one series,
        # without one the whole loop is (a loop body that reads something back earlier just ends the series there) — the
        # library launches a declared series at its first tick instead of learning the pattern from the call history
        if not every:
            st.expect(self.samples)
        for i in range(self.samples):
            st.step(1)                           # == sess.run(self.ode_op(i)), ionic.py:203
            yield i
            if every and i % every == 0:         # a frame every dt_per_plot sub-steps, ionic.py:206
                st.expect(min(every, self.samples - 1 - i))
                self._paint(im, i, watch)
        if keep_state:                           # ionic.py:226-229
            self.state = {}
            for s in self._State:
                self.state[s] = self._State[s].eval()
        st.sync()
        elapsed = time.time() - then
        if self.timeline:                        # ionic.py:231-241: trace one more tick, write a Chrome trace
            events = st.trace_tick()             # every launch between two HIP events (+ the halo exchange on row blocks)
            trace = {'traceEvents': [
                {'name': e['name'], 'cat': 'halo' if e.get('host_clock') else 'kernel', 'ph': 'X', 'ts': e['ts'], 'dur': e['dur'],
                 'pid': 0, 'tid': 1 if e.get('host_clock') else 0,
                 'args': {'sub_steps_fused': e['K'], 'tile': '%dx%d' % e['tile'][:2], 'rows_per_wave': e['tile'][2],
                          'ticks': e['ticks'], 'clock': 'host' if e.get('host_clock') else 'HIP events on the stream'}}
                for e in events]}
            with open(self.timeline_name, 'w') as f:
                json.dump(trace, f)
        self.elapsed = elapsed
        print('elapsed: %f sec' % elapsed)
        if block and im:
            im.wait()

    def _paint(self, im, i, watch):
        """one frame + the cycle-length detector at pixel [20, width//2] (ionic.py:207-224)"""
        image = self.image()
        if self.phase is not None:
            image *= self.phase
        im.imshow(image)
        v1 = image[20, self.width // 2]
        if v1 >= 0.5 and watch['v0'] < 0.5:      # upstroke through 0.5 = a wavefront passes
            cl = (i - watch['last_spike']) * self.dt_per_step * self.dt
            if self.cl_observer is None:
                print('wavefront reaches the middle top point at %d, cycle length is %d' % (i, cl))
            else:
                self.cl_observer(i, cl)
            watch['last_spike'] = i
        watch['v0'] = v1

    def _attachable(self, who):
        """this model, ready for a recorder or a program to attach to its handle: define() has been called, and a traced model
        (traced.py), which compiles on first use, has compiled"""
        if not self.defined:
            raise AssertionError('%s should be called after calling define' % who)
        ensure = getattr(self, '_ensure_compiled', None)
        if ensure is not None:
            ensure()
        return self

    def record_activation(self, up=None, down=None, var=0):
        """attaches an activation recorder (fib_tf_amd/activation.py) to this model's handle: per-cell maps of the first,
        last and previous upstroke through `up`, the APD down to `down` and the number of upstrokes, updated on the device
        after every tick.  Defaults: up at 50 %, down at 10 % of [min_v, max_v].  Call after define(); single device only
        (row blocks raise NotImplementedError)."""
        from .activation import ActivationRecorder
        return ActivationRecorder(self._attachable('record_activation'), up=up, down=down, var=var)

    def record_electrodes(self, masks, every=1, capacity=None, var=0):
        """attaches an electrode recorder (fib_tf_amd/egm.py) to this model's handle: every `every` ticks the weighted sum of
        state array `var` under each full-grid `mask` (its non-zero box) is appended to a trace on the device;
        `traces()` returns the reference's mean(image() * mask) for var = 0 — a model whose image() rescales must override
        `_image_affine()`, which is checked against image() at attach — and mean(X_var * mask) otherwise.  Default capacity:
        the samples of a whole run of `duration`.  Call after define(); single device only (row blocks raise
        NotImplementedError)."""
        from .egm import ElectrodeRecorder
        return ElectrodeRecorder(self._attachable('record_electrodes'), masks, every=every, capacity=capacity, var=var)

    def record_tips(self, var2=None, levels=None, every=1, max_tips=256, capacity=None, var=0, mask=None):
        """attaches a tip recorder (fib_tf_amd/tips.py) to this model's handle: every `every` ticks the phase singularities of
        (X[var] - levels[0], X[var2] - levels[1]) — the spiral tips, with their charge — are found on the device and kept
        there, up to `max_tips` per sample, until `tips()` / `counts()` read them.  `var2` and `levels` default to the
        model's `tip_signals = (var, var2, a0, b0)`; a model without that attribute (a traced model) must pass them.
        `mask` defaults to `phase > 0.5` when the model has a phase field: only plaquettes whose four corners are inside
        count.  Default capacity: the samples of a whole run of `duration`.  Call after define(); single device only (row
        blocks raise NotImplementedError)."""
        from .tips import TipRecorder
        return TipRecorder(self._attachable('record_tips'), var2=var2, levels=levels, every=every, max_tips=max_tips, capacity=capacity, var=var, mask=mask)

    def record_frames(self, every=1, first=None, window=None, block=(1, 1), reduce='mean', fmt='float32', var=0, weight='phase',
                      levels=None, capacity=None):
        """attaches a frame recorder (fib_tf_amd/frames.py) to this model's handle: after ticks first, first + every, ... (first
        defaults to every; first=1 is run(im)'s own cadence) the rows and columns `window` = (r0, r1, c0, c1) of state array
        `var` are written on the device, as one frame, into a cube kept there until `frames()` / `save()` read it.  A pixel is
        a `block` = (by, bx) of cells reduced by `reduce` ('mean' or 'point') of y = (X - lo) / span, times `weight` ('phase':
        the model's phase field if it has one; None; or an [height, width] array), stored as `fmt` 'float32' or 'uint8'.
        `levels` = (lo, span) defaults to `_frame_levels()`; for var = 0 they are checked against image() on the current
        state, bit for bit.  Default capacity: the frames of a whole run of `duration`.  Call after define(); single device
        only (row blocks raise NotImplementedError)."""
        from .frames import FrameRecorder
        return FrameRecorder(self._attachable('record_frames'), every=every, first=first, window=window, block=block, reduce=reduce, fmt=fmt, var=var,
                             weight=weight, levels=levels, capacity=capacity)

    def record_stats(self, columns, every=1, weight='phase', mask=None, capacity=None):
        """attaches a statistics recorder (fib_tf_amd/stats.py) to this model's handle: every `every` ticks one row of
        whole-tissue scalars is taken on the device and kept there until `table()` / `raw()` read it.  `columns` is a list of
        (array, kind) or (array, kind, level), `array` a name or an index of VAR_NAMES, `kind` one of 'sum', 'mean' (weighted
        by `weight`: 'phase' = the model's phase field if it has one, None, or an [height, width] array), 'min', 'max',
        'below', 'above', 'frac_below', 'frac_above', 'nonfinite' (over the cells of `mask`, which defaults to phase > 0.5
        when the model has a phase field).  Up to 64 columns, 8 on one array; each array is read once per sample.  Default
        capacity: the samples of a whole run of `duration`.  Call after define(); single device only (row blocks raise
        NotImplementedError)."""
        from .stats import StatsRecorder
        return StatsRecorder(self._attachable('record_stats'), columns, every=every, weight=weight, mask=mask, capacity=capacity)

    def record_leads(self, positions, tables, table_of=None, every=1, weight='phase', var=0, capacity=None):
        """attaches a lead recorder (fib_tf_amd/leads.py) to this model's handle: every `every` ticks the unipolar electrogram of
        every electrode of `positions` — a list of up to 64 integer cells (row, col) — is formed on the device and kept there
        until `traces()` / `raw()` read it: the float64 sum over the interior cells of K_e * (w * laplace(X)), with X the state
        array `var` behind enforce_boundary, laplace the model's own (9-point Laplacian plus the phase-field term, always in the
        exact form), `weight` w ('phase': the model's phase field if it has one; None: 1; or an [height, width] array) and
        K_e(r, c) = T[|r - row_e|][|c - col_e|] the electrode's lead field.  `tables` is one table [height, width] or up to 4
        of them (`leads.point_table` makes a point electrode's); with several, `table_of` names one per electrode.  Default
        capacity: the samples of a whole run of `duration`.  Call after define(); single device only (row blocks raise
        NotImplementedError); a model with the zero-padded Laplacian is refused."""
        from .leads import LeadRecorder
        return LeadRecorder(self._attachable('record_leads'), positions, tables, table_of=table_of, every=every, weight=weight, var=var, capacity=capacity)

    def record_potential_map(self, table, radius=None, every=10, window=None, step=(1, 1), var=0, weight='phase', max_samples=None):
        """attaches a potential-map recorder (fib_tf_amd/potential.py) to this model's handle: every `every` ticks the unipolar
        electrogram at every site of a lattice — the cells (r0 + i * sy, c0 + j * sx) of `window` = (r0, r1, c0, c1) (None: the
        whole grid) with `step` = (sy, sx), each 1 .. 16 — is formed on the device and kept there, one float64 per sample and
        site, until `maps()` or `summary()` read it: the lead recorder's source w * laplace(X) summed in float64 through the ONE
        lead-field `table` [R + 1, R + 1] truncated at `radius` R = 1 .. 32 (None: the table's; `potential.truncated_table` makes
        a point electrode's).  `weight` as for record_leads.  Default `max_samples`: the samples of a whole run of `duration`.
        Call after define(); single device only (row blocks raise NotImplementedError); a model with the zero-padded Laplacian
        is refused."""
        from .potential import PotentialMapRecorder
        return PotentialMapRecorder(self._attachable('record_potential_map'), table, radius=radius, every=every, window=window, step=step, var=var,
                                    weight=weight, max_samples=max_samples)

    def record_waves(self, level=None, kind='above', every=1, conn=4, mask=None, max_waves=256, capacity=None, var=0, also=None,
                     links=False, max_links=None):
        """attaches a wave recorder (fib_tf_amd/waves.py) to this model's handle: every `every` ticks the cells of `mask` where
        state array `var` is above (`kind` 'above') or below ('below') `level` — strict float32 compares, a NaN is never set —
        and, with `also` = (array, kind, level), a second array meets its own condition, are grouped on the device into their
        connected components under `conn` = 4 or 8, the waves: their number, and per wave its seed (smallest linear index),
        area, centroid sums and bounding box, up to `max_waves` per sample, are kept there until `counts()` / `waves()` read
        them; `labels()` is the label plane of the latest sample.  `level` defaults to the activation recorder's `up` (50 % of
        [min_v, max_v]); `mask` to `phase > 0.5` with the outer ring of the grid, the ghost copies, cleared; arrays are names
        or indices of VAR_NAMES.  Default capacity: the samples of a whole run of `duration`.  With `links=True` the device
        also keeps, per sample, which waves of the sample before share cells with which waves of this one and how many — up to
        `max_links` records (default 2 * max_waves) — for `links()`, `events()` (births, deaths, splits, merges) and `tracks()`;
        choose `every` so that a wave overlaps itself from one sample to the next.  Call after define(); single
        device only (row blocks raise NotImplementedError)."""
        from .waves import WaveRecorder
        return WaveRecorder(self._attachable('record_waves'), level=level, kind=kind, every=every, conn=conn, mask=mask, max_waves=max_waves, capacity=capacity,
                            var=var, also=also, links=links, max_links=max_links)

    def record_spectrum(self, every=10, nfft=128, fmin=None, fmax=None, bins=None, window='hann', chunk=None, var=0, block=(1, 1),
                        reduce='mean', region=None, weight=None):
        """attaches a spectrum recorder (fib_tf_amd/spectrum.py) to this model's handle: every `every` ticks a pixel plane of
        state array `var` — the rows and columns `region` = (r0, r1, c0, c1), a `block` = (by, bx) of cells per pixel reduced by
        `reduce` ('mean' or 'point'), times `weight` ('phase', None or an [height, width] array) — is folded on the device into
        a per-pixel Welch periodogram: segments of `nfft` samples (no overlap, no detrending) under `window` ('hann': periodic
        Hann, 'rect', or an array of nfft numbers), at the frequency indices `bins` (at most 128; default: those between `fmin`
        and `fmax` in Hz, from index 2 — a constant leaks into indices 0 and 1 under the Hann window — to nfft / 2).  `chunk`
        (a divisor of nfft, at most 32; default: the largest up to 16) is how many samples one fold launch takes and changes
        no result.  `power()`, `dominant_frequency()` and `peak_maps()` read the maps; nothing else leaves the device.  Call
        after define(); single device only (row blocks raise NotImplementedError)."""
        from .spectrum import SpectrumRecorder
        return SpectrumRecorder(self._attachable('record_spectrum'), every=every, nfft=nfft, fmin=fmin, fmax=fmax, bins=bins, window=window, chunk=chunk, var=var,
                                block=block, reduce=reduce, region=region, weight=weight)

    def record_beats(self, every=10, depth=8, up=None, down=None, var=0, region=None, block=(1, 1), reduce='mean', weight=None):
        """attaches a beat recorder (fib_tf_amd/beats.py) to this model's handle: every `every` ticks a pixel plane of state
        array `var` — the rows and columns `region` = (r0, r1, c0, c1), a `block` = (by, bx) of cells per pixel reduced by
        `reduce` ('mean' or 'point'), times `weight` ('phase', None or an [height, width] array) — is compared on the device
        with the plane of the previous sample, and every pixel keeps its last `depth` (1 .. 16) beats: the time of the
        upstroke through `up`, of the downstroke through `down` (default: 50 % and 10 % of [min_v, max_v], the activation
        recorder's levels, for var = 0) and the peak in between.  `beats()`, `apd()`, `di()`, `cl()` and `restitution()` read
        the ring, `summary(last)` the maps the device makes of it (mean APD and cycle length, signed alternans amplitude).
        Between two samples the handle keeps its multi-tick launches.  Call after define(); single device only (row blocks
        raise NotImplementedError)."""
        from .beats import BeatRecorder
        return BeatRecorder(self._attachable('record_beats'), every=every, depth=depth, up=up, down=down, var=var, region=region, block=block, reduce=reduce,
                            weight=weight)

    def program_stimuli(self, stimuli):
        """attaches a stimulus program (fib_tf_amd/stimulus.py) to this model's handle: a list of `Stimulus` entries — a site of
        any shape, a value, the tick (or millisecond) of its first event, a period, a count, a hold, 'max' or 'add', any state
        array — that the library applies on the device, each right after its tick, without a call per stimulus; `s1_train`,
        `s1s2` and `burst` build the usual protocols.  Tick 0 is the first tick after this call: an entry with at_tick=i comes
        where `for i in model.run(): if i == s2: model.fire_op('s2')` puts it.  add_pace_op / fire_op work as ever, also while
        a program is attached.  Call after define(); single device only (row blocks raise NotImplementedError)."""
        from .stimulus import StimulusProgram
        return StimulusProgram(self._attachable('program_stimuli'), stimuli)

    def program_lesions(self, lesions):
        """attaches a lesion program (fib_tf_amd/lesions.py) to this model's handle: a list of `Lesion` entries — a site
        (('disc', row, col, radius), ('line', r0, c0, r1, c1, halfwidth) or a plane of factors) and the tick (or millisecond)
        after which it is burnt — that the library multiplies into the phase field on the device, each right after its tick,
        while every recorder and both stimulus programs stay attached; `drag` draws a catheter along a path.  Tick 0 is the
        first tick after this call.  The state is not touched: cells inside a lesion go on with their own kinetics, uncoupled
        from the tissue, as cells inside a hole do.  A model without a phase field gets a field of ones.  On end() / __exit__
        `model.phase` becomes the field as it now is.  Call after define(); single device only (row blocks raise
        NotImplementedError); a model with the zero-padded Laplacian is refused."""
        from .lesions import LesionProgram
        return LesionProgram(self._attachable('program_lesions'), lesions)

    def ablate(self, site):
        """one lesion NOW, at the state the loop has reached (the immediate form of program_lesions: what a host-side closed
        loop uses — read rec.tips(), then ablate there).  Works with or without a program, beside every recorder; updates
        `model.phase` to the field as it now is.  Returns the box (r0, r1, c0, c1) that was visited."""
        from .lesions import ablate
        return ablate(self._attachable('ablate'), site)

    def trigger_stimuli(self, rules, every=1, capacity=None):
        """attaches a trigger program (fib_tf_amd/triggers.py) to this model's handle: a list of `Trigger` rules — a `Sensor`
        (a site, a level, the cells that must be above it), an edge ('rise': an arrival, 'fall': the waveback), a delay, a
        blanking time, an escape interval and the stimulus to fire — that the library senses, decides and applies on the
        device every `every` ticks, without the host reading the state; `s2_on_waveback`, `demand_pacer` and
        `burst_on_arrival` build the usual protocols.  Sample s follows tick (s + 1) * every - 1 after this call.  It may be
        attached beside every recorder and beside a `program_stimuli` program (whose stimulus of a tick the sensors see).
        Default capacity: the samples of a whole run of `duration`.  Call after define(); single device only (row blocks raise
        NotImplementedError)."""
        from .triggers import TriggerProgram
        return TriggerProgram(self._attachable('trigger_stimuli'), rules, every=every, capacity=capacity)

    def _frame_levels(self):
        """(lo, span) with image() == (X - lo) / span in float32, X the array pot() names: what a frame recorder maps the
        state with.  Models whose image() rescales override it."""
        return 0.0, 1.0

    def _image_affine(self):
        """(scale, offset) with image() == scale * X + offset, X the array pot() names: what turns an electrode's raw sum
        into mean(image() * mask).  Models whose image() rescales override it."""
        return 1.0, 0.0

    def millisecond_to_step(self, t):
        """milliseconds -> tick index returned by run(), ionic.py:247-252"""
        return int(t / (self.dt_per_step * self.dt))

    # ---- define(): creates the device-resident state ---------------------------------------------
    def define(self, s1=True):
        """placeholder overridden by the models (ionic.py:254-260)"""
        self.defined = True

    def _flags(self):
        return _lib.FAST if self.fast_math else 0

    def _new_stepper(self, steps_per_tick=0, shard=True):
        """a fibhip handle for the whole grid, or — when a torch.distributed process group with more
        than one rank is initialised — this rank's row block of it (fib_tf_amd/sharded.py)"""
        from .sharded import ShardedStepper, dist_world
        _, world = dist_world()
        if self.tensor is not None and shard and world > 1:
            raise NotImplementedError('set_tensor: a diffusion tensor is set on a single device only; this model runs as row blocks over %d ranks' % world)
        if shard and world > 1:
            st = ShardedStepper(self.MODEL_ID, self.height, self.width, self.dt, self.diff, flags=self._flags(),
                                device=self.device, steps_per_tick=steps_per_tick,
                                halo_ticks=getattr(self, 'halo_ticks', 0), library=self._library,
                                halo_mode=getattr(self, 'halo', None))
        else:
            st = _lib.Stepper(self.MODEL_ID, self.height, self.width, self.dt, self.diff, flags=self._flags(),
                              device=self.device, steps_per_tick=steps_per_tick, library=self._library)
        self._configure_stepper(st)
        if self.phase is not None:
            st.set_phase(self.phase)
        if self.tensor is not None:
            st.set_tensor(*self.tensor)
        return st

    def _configure_stepper(self, st):
        """model-specific constants (BeelerReuter: the Chebyshev table)"""

    def _resume_arrays(self, state):
        """`define(state=...)`: a dict name -> [H, W] array — what `run(keep_state=True)` leaves in `model.state`
        (ionic.py:226-229; court.py:87-89, 623-626 resumes from it) — as the model's arrays in variable order"""
        missing = [n for n in self.VAR_NAMES if n not in state]
        if missing:
            raise KeyError('define(state=...): missing state variables %s' % missing)
        out = []
        for n in self.VAR_NAMES:
            a = np.asarray(state[n], dtype=np.float32)
            if a.shape != (self.height, self.width):
                raise ValueError('define(state=...): %s has shape %s, the grid is %s' % (n, a.shape, (self.height, self.width)))
            out.append(a)
        return out

    def _create(self, init_arrays, steps_per_tick=0):
        """init_arrays: list of [H,W] float32 in the model's variable order"""
        if self._stepper is not None:
            self._stepper.close()
        st = self._new_stepper(steps_per_tick)
        st.set_state(-1, np.stack([np.asarray(a, np.float32) for a in init_arrays]))
        self._stepper = st
        self.dt_per_step = st.steps_per_tick
        self._State = {n: StateVar(self, i, n) for i, n in enumerate(self.VAR_NAMES)}
        return st

    def image(self):
        pass

    def pot(self):
        pass

    def ode_op(self, tick):
        """kept for API symmetry (ionic.py:277-286): the tick operation is the fibhip handle"""
        return self._stepper

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def jit_scope(self):
        """the reference returns an XLA scope when available (ionic.py:294-307); fusion is what
        the HIP kernel does already, so this is the no-op context"""
        return self
