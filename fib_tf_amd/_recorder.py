"""what the recorder and program classes share (activation, egm, tips, frames, stats, leads, waves, spectrum, beats, stimulus,
triggers, lesions): the refusals every attach starts with, the argument forms they have in common, the arithmetic of sample
times, and the open / close / `with` life of an object attached to a model's handle.  A message takes its `who` from the
caller; where two recorders word a refusal differently, the wording stays with them."""
import numpy as np


def attach(model, who, clause):
    """the model's stepper, after the two refusals that come before anything else: no handle yet, or a grid that runs as row
    blocks (`clause`: what the recorder does, as in 'frames are recorded')"""
    from .sharded import ShardedStepper
    st = model._stepper
    if st is None:
        raise AssertionError('%s should be called after calling define' % who)
    if isinstance(st, ShardedStepper):
        raise NotImplementedError('%s: %s on a single device only; this model runs as row blocks over %d ranks' % (who, clause, st.world))
    return st


def check_every(who, every):
    every = int(every)
    if every < 1:
        raise ValueError('%s: every must be >= 1' % who)
    return every


def array_index(names, var, who, check_range=True):
    """a state array given by its name in `names` (the model's VAR_NAMES) or by its index"""
    names = tuple(names)
    if isinstance(var, str):
        if var not in names:
            raise ValueError('%s: unknown array %r (the model has %s)' % (who, var, ', '.join(names)))
        return names.index(var)
    var = int(var)
    if check_range and not 0 <= var < len(names):
        raise ValueError('%s: array index %d outside 0 .. %d' % (who, var, len(names) - 1))
    return var


def weight_plane(model, weight, who, finite=False):
    """`weight` — 'phase' (the model's phase field, if it has one), None or an [height, width] array — as a float32 plane or None"""
    if isinstance(weight, str):
        if weight != 'phase':
            raise ValueError("%s: weight is 'phase', None or an [height, width] array" % who)
        weight = getattr(model, 'phase', None)
    if weight is not None:
        weight = np.ascontiguousarray(weight, np.float32)
        if weight.shape != (model.height, model.width):
            raise ValueError('%s: a weight plane of shape %s on a %d x %d grid' % (who, weight.shape, model.height, model.width))
        if finite and not np.all(np.isfinite(weight)):
            raise ValueError('%s: the weight plane has a value that is not finite' % who)
    return weight


def mask_plane(model, mask, who):
    """`mask` — an [height, width] array, non-zero where a cell counts; None: phase > 0.5 where the model has a phase field
    (inside a hole of the phase field the state is noise) — as a uint8 plane of 0 / 1, or None"""
    if mask is None and getattr(model, 'phase', None) is not None:
        mask = np.asarray(model.phase) > 0.5
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        if mask.shape != (model.height, model.width):
            raise ValueError('%s: a mask of shape %s on a %d x %d grid' % (who, mask.shape, model.height, model.width))
    return mask


def tick_ms(model):
    return float(model.dt_per_step * model.dt)


def run_ticks(model):
    """the ticks of a whole run of model.duration (whatever has run already)"""
    return int(model.duration / (model.dt_per_step * model.dt))


def run_capacity(model, every):
    """the default capacity: the samples of a whole run, at least 1"""
    return max(1, run_ticks(model) // every)


def sample_times(first, n, every, tick_ms):
    """float64 [n]: ms since attach of the samples first, first + 1, ...: sample s follows tick (s + 1) * every - 1"""
    return (int(first) + 1 + np.arange(max(n, 0))) * every * tick_ms


class DeviceRecorder:
    """something attached to a model's handle until close(): `NOUN` names it in the refusal a reader of a closed one gets,
    `END` is the stepper method that detaches it.  A subclass sets `_st` and, once its *_begin went through, `open`."""
    NOUN = END = None
    open = False

    def _check(self):
        if not self.open:
            raise AssertionError('the %s has been closed' % self.NOUN)

    def close(self):
        """detaches from the handle and frees what was kept on the device"""
        if self.open:
            self.open = False
            getattr(self._st, self.END)()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class SampledRecorder(DeviceRecorder):
    """a recorder that keeps one row per sample, read by windows [first, first + count): `COUNT` is the stepper's counter"""
    COUNT = None

    def count(self):
        """samples taken since the recorder was attached"""
        self._check()
        return getattr(self._st, self.COUNT)()

    def _span(self, first, count):
        """the samples of a window (count=None: all taken so far)"""
        return self.count() - int(first) if count is None else int(count)
