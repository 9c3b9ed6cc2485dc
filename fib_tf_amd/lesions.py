"""lesions — the tissue's geometry changed during a run, on the device: ablation points, lines of block, isolated regions.

The reference fixes the geometry before define(): add_hole_to_phase_field multiplies a smooth disc into the phase field
(ionic.py:83-105) and nothing changes it afterwards.  A `LesionProgram` hands the library a list of lesions — a site and the tick
(or millisecond) after which it is burnt — and the library applies each one right after its tick (`lesion_apply_kernel`,
`lesion_prep_kernel`), queued on the stream behind the launch that ends there, while every recorder and both stimulus programs
stay attached; `IonicModel.ablate` is the immediate form for a host-side loop (read the tips, ablate there).

A lesion is a float32 factor patch m on a box of the grid: phi = max(phi * m, 1e-5) on the box, the update of
add_hole_to_phase_field restricted to the cells where its mask is not exactly 1 — same bytes as the whole-plane update as long
as phi >= 1e-5 everywhere beforehand, which attaching checks.  The definition is exact (include/fibhip.h, fibhip_lesion_*;
restated in NumPy in tests/lesion_ref.py).  The STATE is not touched: cells inside a lesion go on with their own kinetics,
uncoupled from the tissue, exactly as cells inside a hole of the reference do.

Planes a recorder was handed at attach (weights, masks) stay what they were; kernels that read the handle's own phase planes —
the ticks, and the lead recorder's source term — see the new geometry from the sample after the event.  DESIGN.md section 22."""
import numpy as np

from ._lib import MAX_LESION_ENTRIES, MAX_STIM_PLANES
from ._recorder import DeviceRecorder, attach, tick_ms
from .tensor import refuse as refuse_tensor

FLOOR = np.float32(1e-5)


def _edge(dist, radius):
    """add_hole_to_phase_field's edge profile: float64 0.5 * (tanh(dist - radius) + 1) cast to float32"""
    return np.array(0.5 * (np.tanh(dist - radius) + 1.0), dtype=np.float32)


def factors(model, site):
    """the site as a float32 [height, width] plane of factors in [0, 1]"""
    H, W = int(model.height), int(model.width)
    if isinstance(site, (tuple, list)) and len(site) == 4 and site[0] == 'disc':
        _, row, col, radius = site
        cols = np.arange(W)[np.newaxis, :] - col            # add_hole_to_phase_field(x=col, y=row, radius), bit for bit
        rows = np.arange(H)[:, np.newaxis] - row
        return _edge(np.hypot(cols, rows), radius)
    if isinstance(site, (tuple, list)) and len(site) == 6 and site[0] == 'line':
        _, r0, c0, r1, c1, halfwidth = site
        dr, dc = float(r1) - float(r0), float(c1) - float(c0)
        rows = np.arange(H, dtype=np.float64)[:, np.newaxis] - float(r0)
        cols = np.arange(W, dtype=np.float64)[np.newaxis, :] - float(c0)
        len2 = dr * dr + dc * dc
        t = np.clip((rows * dr + cols * dc) / len2, 0.0, 1.0) if len2 > 0 else np.zeros((H, W))
        return _edge(np.hypot(cols - t * dc, rows - t * dr), halfwidth)
    if isinstance(site, (tuple, list)) and len(site) and isinstance(site[0], str):
        raise ValueError("Lesion: a site is ('disc', row, col, radius), ('line', r0, c0, r1, c1, halfwidth) or a [height, width] "
                         'plane of factors (got %r)' % (site,))
    a = np.asarray(site)
    if a.shape != (H, W):
        raise ValueError('Lesion: a site of shape %s on a %d x %d grid' % (a.shape, H, W))
    a = np.ascontiguousarray(a, np.float32)
    if not (np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all()):
        raise ValueError('Lesion: every factor of a plane is finite and in [0, 1]')
    return a


def crop(plane):
    """(box, patch): box = (r0, r1, c0, c1), the bounding box of the factors that are not exactly 1.0f, and the factors inside it"""
    hit = np.asarray(plane, np.float32) != np.float32(1.0)
    if not hit.any():
        raise ValueError('Lesion: the site changes no cell of the grid (every factor is 1)')
    rows, cols = np.flatnonzero(hit.any(axis=1)), np.flatnonzero(hit.any(axis=0))
    box = (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1)
    return box, np.ascontiguousarray(plane[box[0]:box[1], box[2]:box[3]], np.float32)


def patch(model, site):
    """(box, patch) of a site on the model's grid: what the library is handed"""
    return crop(factors(model, site))


def apply_host(phase, box, patch):
    """the lesion on a host array: phase[box] = max(phase[box] * patch, 1e-5) in float32; returns a new array"""
    r0, r1, c0, c1 = box
    out = np.array(phase, dtype=np.float32)
    out[r0:r1, c0:c1] = np.maximum(out[r0:r1, c0:c1] * np.asarray(patch, np.float32), FLOOR)
    return out


def check_field(phase):
    """the identity with the whole-plane update needs phi >= float32(1e-5) everywhere beforehand"""
    if phase is not None and not (np.asarray(phase, np.float32) >= FLOOR).all():
        raise ValueError('lesions: the phase field must be >= 1e-5 everywhere (add_hole_to_phase_field leaves it so)')


class Lesion:
    """one entry of a program.

    site     ('disc', row, col, radius) — add_hole_to_phase_field(x=col, y=row, radius)'s mask —, ('line', r0, c0, r1, c1,
             halfwidth) — the same edge profile on the distance to the segment —, or a float [height, width] plane of factors in
             [0, 1]; each is cropped to the bounding box of the factors that are not 1
    at_ms= | at_tick=          the lesion follows tick at_tick of the loop (`for i in model.run()`: i == at_tick)"""

    def __init__(self, site, at_ms=None, at_tick=None):
        if (at_ms is None) == (at_tick is None):
            raise ValueError('Lesion: give at_ms or at_tick (one of them)')
        self.site, self.at_ms, self.at_tick = site, at_ms, at_tick

    def tick(self, model):
        tick = int(self.at_tick) if self.at_tick is not None else model.millisecond_to_step(self.at_ms)
        if tick < 0:
            raise ValueError('Lesion: the lesion follows tick %d: must be >= 0 (a lesion before any tick is ablate()\'s job)' % tick)
        return tick


def drag(points, start_ms, dwell_ms, radius):
    """a catheter drawn along a path: one disc lesion per (row, col) point, `dwell_ms` apart from `start_ms` on"""
    return [Lesion(('disc', r, c, radius), at_ms=start_ms + i * dwell_ms) for i, (r, c) in enumerate(points)]


def compile_program(model, lesions):
    """[Lesion] -> [(tick, box, patch)], what Stepper.lesion_begin takes, in program order"""
    lesions = list(lesions)
    if not 1 <= len(lesions) <= MAX_LESION_ENTRIES:
        raise ValueError('program_lesions: 1 .. %d entries (got %d)' % (MAX_LESION_ENTRIES, len(lesions)))
    out, floats = [], 0
    for i, l in enumerate(lesions):
        if not isinstance(l, Lesion):
            raise ValueError('program_lesions: entry %d is not a Lesion (got %r)' % (i, l))
        box, p = patch(model, l.site)
        floats += p.size
        out.append((l.tick(model), box, p))
    budget = MAX_STIM_PLANES * int(model.height) * int(model.width)
    if floats > budget:
        raise ValueError('program_lesions: %d floats of patches, more than %d planes of the grid (%d)' % (floats, MAX_STIM_PLANES, budget))
    return out


def expand(entries, n_ticks):
    """[(tick, entry index)] of the first n_ticks ticks: by tick, entries due after the same tick in program order"""
    return sorted((t, i) for i, (t, _, _) in enumerate(entries) if t < int(n_ticks))


def _device_stepper(model, who):
    from .leads import _zero_padded
    st = attach(model, who, 'the geometry changes')
    if _zero_padded(model) or getattr(model, 'ZEROPAD', False):
        raise ValueError('%s: not on a model with the zero-padded Laplacian (ZEROPAD): its diffusion term has no phase field' % who)
    refuse_tensor(model, who, 'a lesion recomputes the phase planes, which hold the tensor\'s there')
    check_field(model.phase)
    return st


class LesionProgram(DeviceRecorder):
    """a lesion program attached to a model's handle; see `IonicModel.program_lesions`.

        tips = model.record_tips()
        with model.program_lesions(drag(path, start_ms=400, dwell_ms=5, radius=3)) as prog:
            for i in model.run():
                pass                     # nothing to call: the library burns each lesion right after its tick
            print(prog.applied(), prog.phase().min())
        # model.phase is the field as it now is

    Tick 0 is the first tick after the program was attached.  `events(n)` is the host-side expansion of the program."""
    NOUN, END = 'lesion program', 'lesion_end'

    def __init__(self, model, lesions):
        st = _device_stepper(model, 'program_lesions')
        self.lesions = list(lesions)
        self.entries = compile_program(model, self.lesions)
        self.tick_ms = tick_ms(model)
        self._model, self._st = model, st
        st.lesion_begin(self.entries)
        self.open = True

    def events(self, n_ticks):
        """[(tick, entry index)] the program applies during the first n_ticks ticks (pure Python: no device)"""
        return expand(self.entries, n_ticks)

    def applied(self):
        """lesions applied since the program was attached"""
        self._check()
        return self._st.lesion_count()

    def phase(self):
        """the device's current phase field, float32 [height, width]"""
        self._check()
        return self._st.get_phase()

    def end(self):
        """detaches the program; model.phase becomes the field as it now is, so that what follows sees the tissue as it is:
        image() * phase in run(im), laplace(), recorders attached later with weight='phase' or the default mask"""
        if self.open:
            self._st.lesion_end()
            self._model.phase = self._st.get_phase()
            self.open = False                         # (only now: had either call raised, the program would still be attached)

    close = end


def ablate(model, site):
    """one lesion now (IonicModel.ablate): applies it on the device and makes model.phase the field as it now is"""
    st = _device_stepper(model, 'ablate')
    box, p = patch(model, site)
    st.lesion_apply(box, p)
    model.phase = st.get_phase()
    return box
