"""ctypes binding of libfibhip.so (include/fibhip.h) — the only door between the Python API and
the HIP kernels.  There is deliberately no fallback: if the shared library is missing or no HIP
device is present, every entry point raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, 'libfibhip.so')
SRC = os.path.join(HERE, 'csrc', 'fibhip.hip')
HDR = os.path.join(ROOT, 'include', 'fibhip.h')

FENTON4V, BR, COURT, COURT_US, CUSTOM = 0, 1, 2, 3, 4
OBS_MAPS = ('first_up', 'last_up', 'prev_up', 'apd', 'count')     # enum fibhip_obs_map, in order
FRAME_REDUCE = ('point', 'mean')                                  # enum fibhip_frame_reduce, in order
FRAME_FORMAT = ('float32', 'uint8')                               # enum fibhip_frame_format, in order
SPECTRUM_MAX_BINS, SPECTRUM_MAX_CHUNK, SPECTRUM_MIN_NFFT, SPECTRUM_MAX_NFFT = 128, 32, 4, 65536
BEATS_MAX_DEPTH = 16
STAT_KINDS = ('sum', 'min', 'max', 'below', 'above', 'nonfinite')  # enum fibhip_stat_kind, in order
MAX_STAT_COLS, MAX_STAT_COLS_PER_ARRAY = 64, 8
MAX_LEADS, MAX_LEAD_TABLES = 64, 4
WAVE_KINDS = ('above', 'below')                                   # enum fibhip_wave_kind, in order
MAX_WAVES = 65536
# struct fibhip_wave_record (40 bytes)
WAVE_RECORD_DTYPE = np.dtype([('seed', np.int32), ('area', np.int32), ('sum_r', np.int64), ('sum_c', np.int64),
                              ('r0', np.int32), ('r1', np.int32), ('c0', np.int32), ('c1', np.int32)])
MAX_WAVE_LINKS = 65536
WAVE_LINK_DTYPE = np.dtype([('prev', np.int32), ('seed', np.int32), ('overlap', np.int32)])      # fibhip_wave_link (12 bytes)
STIM_MODES = ('max', 'add')                                       # enum fibhip_stim_mode, in order
STIM_SHAPES = ('rect', 'plane')                                   # enum fibhip_stim_shape, in order
MAX_STIM_ENTRIES, MAX_STIM_PLANES = 64, 8
MAX_LESION_ENTRIES = 256
TRIG_EDGES = ('rise', 'fall')                                     # enum fibhip_trig_edge, in order
TRIG_SITES = ('rect', 'mask')                                     # enum fibhip_trig_site, in order
TRIG_FIELDS = ('c', 'a', 't', 'n', 'cause', 'fired')              # enum fibhip_trig_field, in order: one row of the log
MAX_TRIG_SENSORS, MAX_TRIG_RULES, TRIG_MAX_TIME = 8, 8, 1 << 24
CHEBY, SKIP, CHRONIC, FAST, ALLVARS, ROW_INTERLEAVED, ZEROPAD, HOLD = 1, 2, 4, 8, 16, 32, 64, 128

# -ffp-contract=off: FMAs appear only where the source writes them (policy hook P::mad).
# -fno-slp-vectorize: SLP packs pairs of f32 ops into v_pk_* instructions, which issue at half rate on
#   gfx950 (tools/ubench/valu.hip) and need v_mov shuffles: 11 % slower on the Fenton kernel.
# -fvisibility=hidden: the library exports the C ABI of include/fibhip.h and nothing else (the header pushes default
#   visibility for its declarations).
HIPCC_FLAGS = ['-O3', '--offload-arch=gfx950', '-ffp-contract=off', '-fno-slp-vectorize', '-fvisibility=hidden', '-fPIC', '-shared',
               '-std=c++17', '-Wall', '-Wno-unused-value', '-Wno-unused-result']


def _build_tag(so_path):
    """-DFIB_BUILD_TAG for a non-stock build: every kernel symbol of the build carries it (csrc/models.hpp)"""
    import re
    return '-DFIB_BUILD_TAG=b_' + re.sub(r'[^0-9A-Za-z_]', '_', os.path.splitext(os.path.basename(so_path))[0])


class FibhipError(RuntimeError):
    pass


# ---- arrays on page-locked host memory ------------------------------------------------------------------------------
# eval() / image() return ordinary NumPy arrays; behind single-array read-backs sits a small pool of page-locked buffers
# (fibhip_host_alloc) the device writes directly, which saves the staging copy of fibhip_get_state.  A buffer returns to
# the pool when the last view of its array is gone; with more than PINNED_MAX arrays alive at once (a caller keeping
# every frame) further read-backs fall back to pageable arrays.
PINNED_MAX = 8
_pinned_free = {}          # nbytes -> [address, ...]
_pinned_out = [0]


def _pinned_release(nbytes, addr):
    _pinned_out[0] -= 1
    _pinned_free.setdefault(nbytes, []).append(addr)


def _pinned_array(L, shape):
    import weakref
    n = int(np.prod(shape))
    nbytes = 4 * n
    free = _pinned_free.get(nbytes)
    if free:
        addr = free.pop()
    else:
        if _pinned_out[0] + sum(len(v) for v in _pinned_free.values()) >= PINNED_MAX:
            other = next((v for v in _pinned_free.values() if v), None)     # an idle buffer of another size makes room
            if other is None:
                return None
            L.fibhip_host_free(other.pop())
        p = C.c_void_p()
        if L.fibhip_host_alloc(nbytes, C.byref(p)) != 0 or not p.value:
            return None
        addr = p.value
    raw = (C.c_float * n).from_address(addr)
    _pinned_out[0] += 1
    f = weakref.finalize(raw, _pinned_release, nbytes, addr)
    f.atexit = False
    return np.ctypeslib.as_array(raw).reshape(shape)


class Desc(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('model', C.c_int), ('height', C.c_int), ('width', C.c_int),
                ('dt', C.c_double), ('diff', C.c_double), ('flags', C.c_uint), ('device', C.c_int),
                ('steps_per_tick', C.c_int), ('global_height', C.c_int), ('row_offset', C.c_int),
                ('ghost_top', C.c_int), ('ghost_bottom', C.c_int), ('stream', C.c_void_p),
                ('ext_slab', C.c_void_p * 2), ('module', C.c_void_p)]


class ModuleKernel(C.Structure):
    _fields_ = [('symbol', C.c_char_p), ('kind', C.c_int), ('mode', C.c_int), ('fast', C.c_int), ('phase', C.c_int),
                ('K', C.c_int), ('TX', C.c_int), ('TY', C.c_int), ('NT', C.c_int)]


class ModuleDesc(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('nvar', C.c_int), ('steps_per_tick', C.c_int), ('nmodes', C.c_int),
                ('masks', C.c_uint * 8), ('consts_bytes', C.c_int)] + [
                    (k, C.c_int) for k in ('K', 'TX', 'TY', 'R', 'TYB', 'K2', 'TX2', 'TY2', 'R2')] + [
                    ('nkernels', C.c_int), ('kernels', C.POINTER(ModuleKernel))]


class TraceEvent(C.Structure):
    _fields_ = [('name', C.c_char * 96), ('start_us', C.c_double), ('dur_us', C.c_double), ('K', C.c_int), ('tile_w', C.c_int),
                ('tile_h', C.c_int), ('rows_per_wave', C.c_int), ('ticks', C.c_int)]


class HaloMsg(C.Structure):
    _fields_ = [('offset', C.c_longlong), ('count', C.c_longlong), ('peer', C.c_int), ('send', C.c_int)]


class StatCol(C.Structure):
    _fields_ = [('var', C.c_int), ('kind', C.c_int), ('level', C.c_float)]


class StimEntry(C.Structure):
    _fields_ = [('var', C.c_int), ('mode', C.c_int), ('shape', C.c_int), ('r0', C.c_int), ('r1', C.c_int), ('c0', C.c_int),
                ('c1', C.c_int), ('v', C.c_float), ('floor', C.c_float), ('plane', C.c_int), ('first', C.c_int), ('period', C.c_int),
                ('count', C.c_int), ('hold', C.c_int)]


class LesionEntry(C.Structure):
    _fields_ = [('offset', C.c_longlong), ('tick', C.c_int), ('r0', C.c_int), ('r1', C.c_int), ('c0', C.c_int), ('c1', C.c_int),
                ('reserved', C.c_int)]


class TrigSensor(C.Structure):
    _fields_ = [('var', C.c_int), ('level', C.c_float), ('need', C.c_int), ('site', C.c_int), ('r0', C.c_int), ('r1', C.c_int),
                ('c0', C.c_int), ('c1', C.c_int)]


class TrigRule(C.Structure):
    _fields_ = [('sensor', C.c_int), ('edge', C.c_int), ('arm', C.c_int), ('blank', C.c_int), ('escape', C.c_int), ('max_det', C.c_int),
                ('delay', C.c_int), ('count', C.c_int), ('period', C.c_int), ('hold', C.c_int), ('var', C.c_int), ('mode', C.c_int),
                ('shape', C.c_int), ('r0', C.c_int), ('r1', C.c_int), ('c0', C.c_int), ('c1', C.c_int), ('v', C.c_float), ('floor', C.c_float),
                ('plane', C.c_int)]


_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
_h = C.c_void_p

# name -> (argtypes, restype): every symbol include/fibhip.h declares
SYMBOLS = {
    'fibhip_nvar': ([C.c_int], C.c_int),
    'fibhip_default_steps_per_tick': ([C.c_int], C.c_int),
    'fibhip_abi_version': ([], C.c_int),
    'fibhip_device_count': ([], C.c_int),
    'fibhip_create': ([C.POINTER(Desc), C.POINTER(_h)], C.c_int),
    'fibhip_destroy': ([_h], C.c_int),
    'fibhip_set_phase': ([_h, _fp], C.c_int),
    'fibhip_set_state': ([_h, C.c_int, _fp], C.c_int),
    'fibhip_get_state': ([_h, C.c_int, _fp], C.c_int),
    'fibhip_set_consts': ([_h, _fp, C.c_int], C.c_int),
    'fibhip_step': ([_h, C.c_int], C.c_int),
    'fibhip_step_slow': ([_h], C.c_int),
    'fibhip_step_mode': ([_h, C.c_int], C.c_int),
    'fibhip_pace': ([_h, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float], C.c_int),
    'fibhip_probe': ([_h, C.c_int, C.c_int, C.c_int, _fp], C.c_int),
    'fibhip_sync': ([_h], C.c_int),
    'fibhip_time_steps': ([_h, C.c_int, _fp, _ip], C.c_int),
    'fibhip_time_begin': ([_h], C.c_int),
    'fibhip_time_end': ([_h, _fp, _ip], C.c_int),
    'fibhip_step_edges': ([_h], C.c_int),
    'fibhip_step_interior': ([_h], C.c_int),
    'fibhip_step_commit': ([_h], C.c_int),
    'fibhip_state_ptr': ([_h, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    'fibhip_next_ptr': ([_h, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    'fibhip_halo_vars': ([_h], C.c_int),
    'fibhip_halo_due': ([_h], C.c_int),
    'fibhip_unit_op': ([C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_double, C.c_int, _fp],
                       C.c_int),
    'fibhip_court_inter': ([C.c_int, C.c_int, _fp, C.c_int, _fp], C.c_int),
    'fibhip_halo_plan': ([_h, C.c_int, C.c_int, C.POINTER(HaloMsg), _ip], C.c_int),
    'fibhip_comm_open': ([C.c_char_p], C.c_int),
    'fibhip_comm_unique_id': ([C.c_char_p], C.c_int),
    'fibhip_comm_check': ([_h, C.c_int, C.c_int], C.c_int),
    'fibhip_comm_init': ([_h, C.c_char_p, C.c_int, C.c_int], C.c_int),
    'fibhip_comm_exchange': ([_h, C.c_int, C.c_int], C.c_int),
    'fibhip_comm_free': ([_h], C.c_int),
    'fibhip_copy_bandwidth': ([C.c_int, C.c_size_t, C.c_int, _fp], C.c_int),
    'fibhip_warm': ([C.c_int], C.c_int),
    'fibhip_module_load': ([C.c_int, C.c_void_p, C.c_size_t, C.POINTER(ModuleDesc), C.POINTER(C.c_void_p)], C.c_int),
    'fibhip_module_unload': ([C.c_void_p], C.c_int),
    'fibhip_launch_plan': ([_h, _ip, _ip], C.c_int),
    'fibhip_get_state_direct': ([_h, C.c_int, _fp], C.c_int),
    'fibhip_host_alloc': ([C.c_size_t, C.POINTER(C.c_void_p)], C.c_int),
    'fibhip_host_free': ([C.c_void_p], C.c_int),
    'fibhip_ticks_per_launch': ([_h], C.c_int),
    'fibhip_launch_stats': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_spec_stats': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_fallbacks': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_set_mt_wait_ms': ([_h, C.c_int], C.c_int),
    'fibhip_expect': ([_h, C.c_int], C.c_int),
    'fibhip_trace_begin': ([_h], C.c_int),
    'fibhip_trace_end': ([_h, C.POINTER(TraceEvent), C.c_int], C.c_int),
    'fibhip_plan_tile': ([_h, _ip, _ip, _ip], C.c_int),
    'fibhip_variant_count': ([], C.c_int),
    'fibhip_variant_info': ([C.c_int, _ip], C.c_int),
    'fibhip_observe_begin': ([_h, C.c_int, C.c_float, C.c_float], C.c_int),
    'fibhip_observe_get': ([_h, C.c_int, C.c_void_p], C.c_int),
    'fibhip_observe_ticks': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_observe_end': ([_h], C.c_int),
    'fibhip_electrode_begin': ([_h, C.c_int, C.c_int, _ip, _fp, C.c_int, C.c_longlong], C.c_int),
    'fibhip_electrode_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_electrode_read': ([_h, C.c_longlong, C.c_longlong, _fp], C.c_int),
    'fibhip_electrode_end': ([_h], C.c_int),
    'fibhip_tips_begin': ([_h, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_longlong], C.c_int),
    'fibhip_tips_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_tips_read': ([_h, C.c_longlong, C.c_longlong, _ip, _ip], C.c_int),
    'fibhip_tips_end': ([_h], C.c_int),
    'fibhip_frames_begin': ([_h, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _fp, C.c_int, C.c_int, C.c_int,
                             C.c_longlong], C.c_int),
    'fibhip_frames_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_frames_shape': ([_h, _ip, _ip, _ip], C.c_int),
    'fibhip_frames_read': ([_h, C.c_longlong, C.c_longlong, C.c_void_p], C.c_int),
    'fibhip_frames_end': ([_h], C.c_int),
    'fibhip_stats_begin': ([_h, C.c_int, C.POINTER(StatCol), _fp, C.POINTER(C.c_ubyte), C.c_int, C.c_longlong], C.c_int),
    'fibhip_stats_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_stats_read': ([_h, C.c_longlong, C.c_longlong, C.POINTER(C.c_double)], C.c_int),
    'fibhip_stats_end': ([_h], C.c_int),
    'fibhip_leads_begin': ([_h, C.c_int, C.c_int, _ip, C.c_int, _fp, _fp, C.c_int, C.c_longlong], C.c_int),
    'fibhip_leads_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_leads_read': ([_h, C.c_longlong, C.c_longlong, C.POINTER(C.c_double)], C.c_int),
    'fibhip_leads_end': ([_h], C.c_int),
    'fibhip_waves_begin': ([_h, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int,
                            C.c_longlong], C.c_int),
    'fibhip_waves_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_waves_read': ([_h, C.c_longlong, C.c_longlong, _ip, C.c_void_p], C.c_int),
    'fibhip_waves_labels': ([_h, _ip], C.c_int),
    'fibhip_waves_links_begin': ([_h, C.c_int], C.c_int),
    'fibhip_waves_links_read': ([_h, C.c_longlong, C.c_longlong, _ip, C.c_void_p], C.c_int),
    'fibhip_waves_end': ([_h], C.c_int),
    'fibhip_spectrum_begin': ([_h, C.c_int, _ip, C.c_int, C.c_int, C.c_int, _fp, C.c_int, C.c_int, _fp, _fp, C.c_int, _ip, C.c_int], C.c_int),
    'fibhip_spectrum_count': ([_h, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_spectrum_shape': ([_h, _ip, _ip, _ip], C.c_int),
    'fibhip_spectrum_read': ([_h, _fp, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_spectrum_peak': ([_h, C.c_int, C.c_int, C.c_int, _ip, _fp, _fp, _fp], C.c_int),
    'fibhip_spectrum_end': ([_h], C.c_int),
    'fibhip_beats_begin': ([_h, C.c_int, _ip, C.c_int, C.c_int, C.c_int, _fp, C.c_int, C.c_float, C.c_float, C.c_int], C.c_int),
    'fibhip_beats_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_beats_shape': ([_h, _ip, _ip, _ip], C.c_int),
    'fibhip_beats_read': ([_h, _fp, _fp, _fp, _ip, _fp], C.c_int),
    'fibhip_beats_summary': ([_h, C.c_int, _ip, _fp, _fp, _fp], C.c_int),
    'fibhip_beats_end': ([_h], C.c_int),
    'fibhip_stim_begin': ([_h, C.c_int, C.POINTER(StimEntry), C.c_int, _fp], C.c_int),
    'fibhip_stim_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_stim_end': ([_h], C.c_int),
    'fibhip_lesion_begin': ([_h, C.c_int, C.POINTER(LesionEntry), C.c_longlong, _fp], C.c_int),
    'fibhip_lesion_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_lesion_end': ([_h], C.c_int),
    'fibhip_lesion_apply': ([_h, _ip, _fp], C.c_int),
    'fibhip_get_phase': ([_h, _fp], C.c_int),
    'fibhip_trig_begin': ([_h, C.c_int, C.POINTER(TrigSensor), C.POINTER(C.c_ubyte), C.c_int, C.POINTER(TrigRule), C.c_int, _fp, C.c_int,
                           C.c_longlong], C.c_int),
    'fibhip_trig_count': ([_h, C.POINTER(C.c_longlong)], C.c_int),
    'fibhip_trig_read': ([_h, C.c_longlong, C.c_longlong, _ip], C.c_int),
    'fibhip_trig_end': ([_h], C.c_int),
    'fibhip_last_error': ([], C.c_char_p),
}

_lib = None


DEPS = [SRC, HDR] + [os.path.join(HERE, "csrc", f) for f in ("kernels.hpp", "stencil.hpp", "tick_kernel.inc", "strip_mt.hpp",
                                                             "strip_kernel.inc", "rows_kernel.inc", "pointwise.inc", "record_kernels.inc",
                                                             "models.hpp", "fenton_step.inc", "br_step.inc",
                                                             "court_step.inc", "court_inter.inc", "host_util.hpp", "launch.hpp",
                                                             "ctx.hpp", "sampler.hpp", "recorders.hpp", "tick.inc", "sched.inc", "record.inc", "plan.inc", "comm.inc",
                                                             "unit.inc")]


def build(force=False, verbose=False):
    """compile csrc/fibhip.hip for gfx950 in-tree (hipcc cross-compiles without a GPU)"""
    if not force and os.path.exists(SO) and all(os.path.getmtime(SO) >= os.path.getmtime(d) for d in DEPS):
        return SO
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc] + HIPCC_FLAGS + [SRC, '-o', SO]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd)
    return SO


def build_custom(inc_path, so_path, verbose=False):
    """the same translation unit with ONE traced model compiled in (generated header `inc_path`,
    fib_tf_amd/traced.py) and the stock models' kernels left out: a few seconds instead of a minute"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    tmp = '%s.%d.tmp' % (so_path, os.getpid())
    cmd = [hipcc] + HIPCC_FLAGS + ['-DFIB_CUSTOM_ONLY', '-DFIB_CUSTOM_MODEL_INC="%s"' % os.path.abspath(inc_path),
                                   _build_tag(so_path), SRC, '-o', tmp]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd)
    os.replace(tmp, so_path)            # atomic: several ranks may build the same model at once
    return so_path


def build_specialised(defines, so_path, verbose=False):
    """the same translation unit with model constants baked in as literals (`defines`: list of -D options);
    used by BeelerReuter for its Chebyshev table: a VALU operand from a literal issues at full rate, one from an
    SGPR (kernel argument) at ~60 % (tools/ubench/valu2.hip), and the table feeds 96 multiply-adds per cell-step"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    tmp = '%s.%d.tmp' % (so_path, os.getpid())
    cmd = [hipcc] + HIPCC_FLAGS + list(defines) + [_build_tag(so_path), SRC, '-o', tmp]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd)
    os.replace(tmp, so_path)
    return so_path


def load(path):
    """dlopen a build of the library and declare every symbol's signature"""
    L = C.CDLL(path)
    for name, (args, res) in SYMBOLS.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, res
    if L.fibhip_abi_version() != 1:
        raise FibhipError('%s: ABI version mismatch' % os.path.basename(path))
    return L


def lib():
    global _lib
    if _lib is None:
        alt = os.environ.get('FIBHIP_LIBRARY')          # tuning experiments: another build of the same source
        if alt:
            _lib = load(alt)
            return _lib
        if not os.path.exists(SO):
            raise FibhipError('libfibhip.so is not built (run `python -c "import __graft_entry__ as g; g.build()"`); '
                              'fib_tf_amd has no CPU fallback')
        _lib = load(SO)
    return _lib


_warmed = set()


def warm(device=0):
    """the stock library's code object first: called before any OTHER build of the library launches a kernel in this
    process (include/fibhip.h fibhip_warm: under rocprofv3 the opposite order dies inside the HIP runtime)"""
    if device not in _warmed:
        check(lib().fibhip_warm(device))
        _warmed.add(device)


# ---- in-process builds of traced models: hiprtc -> code object -> fibhip_module_load ------------------------------
HIPRTC = os.environ.get('FIBTF_HIPRTC', '/opt/rocm/lib/libhiprtc.so')
_rtc = None


def hiprtc():
    """libhiprtc bound through ctypes, or None when the runtime does not ship it"""
    global _rtc
    if _rtc is None:
        try:
            R = C.CDLL(HIPRTC)
        except OSError:
            _rtc = False
            return None
        pp = C.POINTER(C.c_char_p)
        R.hiprtcCreateProgram.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_char_p, C.c_int, pp, pp]
        R.hiprtcAddNameExpression.argtypes = [C.c_void_p, C.c_char_p]
        R.hiprtcCompileProgram.argtypes = [C.c_void_p, C.c_int, pp]
        R.hiprtcGetLoweredName.argtypes = [C.c_void_p, C.c_char_p, pp]
        R.hiprtcGetProgramLogSize.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        R.hiprtcGetProgramLog.argtypes = [C.c_void_p, C.c_char_p]
        R.hiprtcGetCodeSize.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        R.hiprtcGetCode.argtypes = [C.c_void_p, C.c_char_p]
        R.hiprtcDestroyProgram.argtypes = [C.POINTER(C.c_void_p)]
        _rtc = R
    return _rtc or None


def rtc_compile(source, headers, name_exprs, options):
    """compile device code in this process: (code object bytes, {name expression: lowered symbol}).
    headers: {include name: text} handed over in memory; hiprtc needs no GPU (gfx950 is an option)."""
    R = hiprtc()
    if R is None:
        raise FibhipError('libhiprtc is not available (%s)' % HIPRTC)
    prog = C.c_void_p()
    names = list(headers)
    harr = (C.c_char_p * len(names))(*[headers[n].encode() for n in names])
    narr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    rc = R.hiprtcCreateProgram(C.byref(prog), source.encode(), b'fibhip_traced.hip', len(names), harr, narr)
    if rc:
        raise FibhipError('hiprtcCreateProgram failed (%d)' % rc)
    try:
        for e in name_exprs:
            if R.hiprtcAddNameExpression(prog, e.encode()):
                raise FibhipError('hiprtcAddNameExpression refused %r' % e)
        oarr = (C.c_char_p * len(options))(*[o.encode() for o in options])
        rc = R.hiprtcCompileProgram(prog, len(options), oarr)
        if rc:
            n = C.c_size_t()
            R.hiprtcGetProgramLogSize(prog, C.byref(n))
            log = C.create_string_buffer(max(1, n.value))
            R.hiprtcGetProgramLog(prog, log)
            raise FibhipError('hiprtc could not compile the generated model (%d):\n%s' % (rc, log.value.decode('utf-8', 'replace')[-4000:]))
        lowered = {}
        for e in name_exprs:
            p = C.c_char_p()
            if R.hiprtcGetLoweredName(prog, e.encode(), C.byref(p)) or not p.value:
                raise FibhipError('hiprtcGetLoweredName failed for %r' % e)
            lowered[e] = p.value.decode()
        n = C.c_size_t()
        R.hiprtcGetCodeSize(prog, C.byref(n))
        code = C.create_string_buffer(n.value)
        R.hiprtcGetCode(prog, code)
        return code.raw, lowered
    finally:
        R.hiprtcDestroyProgram(C.byref(prog))


RTC_OPTIONS = ['--offload-arch=gfx950', '-O3', '-ffp-contract=off', '-fno-slp-vectorize', '-std=c++17',
               '-I' + os.path.join(HERE, 'csrc')]


class ModuleLibrary:
    """the stock library + ONE traced model's code object loaded into it (fibhip_module_load): stands where a
    per-model build of libfibhip stood — `Stepper(..., library=this)` creates FIBHIP_CUSTOM handles on the module"""

    def __init__(self, code, meta, device, name):
        L = lib()
        self._L, self._code, self.meta, self.device = L, code, meta, device
        self._name = '%s#module:%s' % (SO, name)
        kern = (ModuleKernel * len(meta['kernels']))()
        self._keep = []
        for i, k in enumerate(meta['kernels']):
            sym = k['symbol'].encode()
            self._keep.append(sym)
            kern[i] = ModuleKernel(sym, k['kind'], k['mode'], k['fast'], k['phase'], k['K'], k['TX'], k['TY'], k['NT'])
        d = ModuleDesc()
        d.struct_size = C.sizeof(ModuleDesc)
        d.nvar, d.steps_per_tick, d.nmodes, d.consts_bytes = meta['nvar'], meta['spt'], meta['nmodes'], meta['consts_bytes']
        for i, m in enumerate(meta['masks']):
            d.masks[i] = m
        for k in ('K', 'TX', 'TY', 'R', 'TYB', 'K2', 'TX2', 'TY2', 'R2'):
            setattr(d, k, meta['plan'][k])
        d.nkernels, d.kernels = len(kern), kern
        self.module = C.c_void_p()
        check(L.fibhip_module_load(device, code, len(code), C.byref(d), C.byref(self.module)), L)

    # model facts the stock library cannot know
    def fibhip_nvar(self, model):
        return self.meta['nvar'] if model == CUSTOM else self._L.fibhip_nvar(model)

    def fibhip_default_steps_per_tick(self, model):
        return self.meta['spt'] if model == CUSTOM else self._L.fibhip_default_steps_per_tick(model)

    def __getattr__(self, name):
        return getattr(self._L, name)


def check(rc, L=None):
    if rc < 0:
        raise FibhipError((L or lib()).fibhip_last_error().decode('utf-8', 'replace'))
    return rc


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_fp)


def unit_op(op, a, b=None, c=None, phi=None, dt=0.0, fast=False, device=0):
    a = _f32(a)
    H, W = a.shape
    b = None if b is None else _f32(b)
    c = None if c is None else _f32(c)
    phi = None if phi is None else _f32(phi)
    out = np.empty_like(a)
    check(lib().fibhip_unit_op(device, op, H, W, _ptr(a), _ptr(b), _ptr(c), _ptr(phi), float(dt), int(fast),
                               _ptr(out)))
    return out


VARIANT_FIELDS = ('model', 'mode', 'fast', 'phase', 'K', 'TX', 'TY', 'NT', 'kind', 'has_mt')   # fibhip_variant_info, in order
VM_FENTON_ZP, VM_COURT_AGG = 100, 101                   # table ids of the two kernel models that are no fibhip_model
MK_TICK, MK_STRIP, MK_POINTWISE, MK_STRIP_MT, MK_ROWS = range(5)


def variants(L=None):
    """the kernel variant table of a build of the library, in table order: a list of dicts with the keys VARIANT_FIELDS
    (include/fibhip.h fibhip_variant_info).  `L`: another loaded build (br.specialised_library), default the stock one.
    Needs no device."""
    L = L or lib()
    L = getattr(L, '_L', L)                             # (a ModuleLibrary: the table of the stock library under it)
    out = (C.c_int * len(VARIANT_FIELDS))()
    rows = []
    for i in range(check(L.fibhip_variant_count(), L)):
        check(L.fibhip_variant_info(i, out), L)
        rows.append(dict(zip(VARIANT_FIELDS, [int(x) for x in out])))
    return rows


COURT_INTER_KEYS = ('d_infinity', 'tau_d', 'f_infinity', 'tau_f', 'tau_w', 'w_infinity', 'm_inf', 'tau_m', 'h_inf',
                    'tau_h', 'j_inf', 'tau_j', 'tau_oa', 'oa_infinity', 'tau_oi', 'oi_infinity', 'tau_ua',
                    'ua_infinity', 'tau_ui', 'ui_infinity', 'tau_xr', 'xr_infinity', 'tau_xs', 'xs_infinity', 'g_Kur',
                    'f_NaK', 'i_NaCaa', 'i_NaCab', 'i_K1a', 'i_Kra', 'us_infinity', 'tau_us')


def copy_bandwidth(nbytes=1 << 30, reps=5, device=0, library=None):
    """GB/s (read + written) of a plain streaming copy on the device: the achievable-HBM yardstick.
    `library`: the build of libfibhip the caller is already running kernels from (a specialised or traced build)"""
    L = library or lib()
    out = C.c_float()
    check(L.fibhip_copy_bandwidth(device, nbytes, reps, C.byref(out)), L)
    return out.value


def court_inter(V, fast=False, device=0):
    """the voltage-only intermediates of the Courtemanche model for an array (or scalar) of voltages:
    dict key -> float32 array shaped like V (court.py:273-429, court_ultra.py:445-450)"""
    v = _f32(V)
    out = np.empty((len(COURT_INTER_KEYS), v.size), np.float32)
    check(lib().fibhip_court_inter(device, v.size, _ptr(v.reshape(-1)), int(fast), _ptr(out)))
    return {k: out[i].reshape(v.shape) for i, k in enumerate(COURT_INTER_KEYS)}


class Stepper:
    """One fibhip handle: a grid (or a row block of it) resident on one MI355X."""

    def __init__(self, model, height, width, dt, diff, flags=0, device=0, steps_per_tick=0,
                 global_height=0, row_offset=0, ghost_top=0, ghost_bottom=0, stream=None, ext_slabs=None,
                 library=None):
        L = library or lib()
        # ANY other build of the library (a Beeler-Reuter table baked in, a traced model compiled in, an experiment's
        # FIBHIP_BR_LIBRARY): the stock library's code object comes up first on this device — see `warm` — whoever the caller is
        if library is not None and not isinstance(library, ModuleLibrary) and library is not lib():
            warm(device)
        d = Desc()
        d.struct_size = C.sizeof(Desc)
        d.model, d.height, d.width = model, height, width
        d.dt, d.diff, d.flags, d.device = float(dt), float(diff), flags, device
        d.steps_per_tick = steps_per_tick
        d.global_height, d.row_offset = global_height, row_offset
        d.ghost_top, d.ghost_bottom = ghost_top, ghost_bottom
        d.stream = stream
        if ext_slabs is not None:
            d.ext_slab[0], d.ext_slab[1] = ext_slabs
        d.module = getattr(L, 'module', None)          # a traced model's run-time module (ModuleLibrary), or NULL
        self._h = _h()
        self._L = L
        self._warned = False
        self.nvar = self._ck(L.fibhip_nvar(model))
        self.height, self.width = height, width
        self.steps_per_tick = steps_per_tick or self._ck(L.fibhip_default_steps_per_tick(model))
        self._ck(L.fibhip_create(C.byref(d), C.byref(self._h)))

    def _ck(self, rc):
        return check(rc, self._L)

    def close(self):
        if getattr(self, '_h', None) and self._h.value:
            self._L.fibhip_destroy(self._h)
            self._h = _h()

    __del__ = close

    def set_phase(self, phi):
        if phi is None:
            self._ck(self._L.fibhip_set_phase(self._h, None))
        else:
            phi = _f32(phi)
            assert phi.shape == (self.height, self.width)
            self._ck(self._L.fibhip_set_phase(self._h, _ptr(phi)))

    def set_state(self, var, arr):
        arr = _f32(arr)
        want = (self.nvar, self.height, self.width) if var < 0 else (self.height, self.width)
        assert arr.shape == want, (arr.shape, want)
        self._ck(self._L.fibhip_set_state(self._h, var, _ptr(arr)))

    def get_state(self, var=-1):
        shape = (self.nvar, self.height, self.width) if var < 0 else (self.height, self.width)
        if var >= 0:                                    # one array (eval(), image()): straight into page-locked memory
            out = _pinned_array(self._L, shape)
            if out is not None:
                self._ck(self._L.fibhip_get_state_direct(self._h, var, _ptr(out)))
                self._fallback_warning()
                return out
        out = np.empty(shape, np.float32)
        self._ck(self._L.fibhip_get_state(self._h, var, _ptr(out)))
        self._fallback_warning()
        return out

    def set_consts(self, tbl):
        tbl = _f32(tbl).ravel()
        self._ck(self._L.fibhip_set_consts(self._h, _ptr(tbl), tbl.size))

    def step(self, nticks=1):
        self._ck(self._L.fibhip_step(self._h, nticks))

    def step_slow(self):
        self._ck(self._L.fibhip_step_slow(self._h))

    def step_mode(self, mode):
        self._ck(self._L.fibhip_step_mode(self._h, mode))

    def pace(self, r0, r1, c0, c1, v, min_v):
        self._ck(self._L.fibhip_pace(self._h, r0, r1, c0, c1, v, min_v))

    def probe(self, var, row, col):
        out = C.c_float()
        self._ck(self._L.fibhip_probe(self._h, var, row, col, C.byref(out)))
        return np.float32(out.value)

    def sync(self):
        self._ck(self._L.fibhip_sync(self._h))
        self._fallback_warning()

    def expect(self, nticks):
        """declares the caller's next series: `nticks` ticks without an observation in between (include/fibhip.h)"""
        self._ck(self._L.fibhip_expect(self._h, int(nticks)))

    def set_mt_wait_ms(self, ms):
        self._ck(self._L.fibhip_set_mt_wait_ms(self._h, int(ms)))

    def fallbacks(self):
        """(multi-tick launches that gave up and were recovered, ticks recomputed one launch per tick)"""
        out = (C.c_longlong * 2)()
        self._ck(self._L.fibhip_fallbacks(self._h, out))
        return int(out[0]), int(out[1])

    def _fallback_warning(self):
        if not self._warned:
            n, ticks = self.fallbacks()
            if n:
                self._warned = True
                import warnings
                warnings.warn('fib_tf_amd: a launch advancing several ticks gave up waiting for a neighbouring tile (is another '
                              'process holding the GPU, or a CU mask set?); the handle went back to the state that launch started '
                              'from, recomputed %d tick(s) and runs one launch per tick from here on — same results, slower '
                              '(FIBHIP_MT=0 selects that mode from the start)' % ticks, RuntimeWarning, stacklevel=3)

    def time_steps(self, nticks):
        ms, n = C.c_float(), C.c_int()
        self._ck(self._L.fibhip_time_steps(self._h, nticks, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def time_begin(self):
        self._ck(self._L.fibhip_time_begin(self._h))

    def time_end(self):
        """(milliseconds, launches) since time_begin, by HIP events on the handle's stream"""
        ms, n = C.c_float(), C.c_int()
        self._ck(self._L.fibhip_time_end(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def step_edges(self):
        self._ck(self._L.fibhip_step_edges(self._h))

    def step_interior(self):
        self._ck(self._L.fibhip_step_interior(self._h))

    def step_commit(self):
        self._ck(self._L.fibhip_step_commit(self._h))

    def state_buf(self, var):
        p = C.c_void_p()
        return self._ck(self._L.fibhip_state_ptr(self._h, var, C.byref(p))), p.value

    def next_buf(self, var):
        p = C.c_void_p()
        return self._ck(self._L.fibhip_next_ptr(self._h, var, C.byref(p))), p.value

    def halo_vars(self):
        return self._ck(self._L.fibhip_halo_vars(self._h))

    def halo_due(self):
        return bool(self._ck(self._L.fibhip_halo_due(self._h)))

    # ---- direct halo exchange (RCCL issued by the library on this handle's stream) ------------------------
    def comm_open(self, librccl_path=None):
        self._ck(self._L.fibhip_comm_open(librccl_path.encode() if librccl_path else None))

    def comm_unique_id(self, librccl_path=None):
        self.comm_open(librccl_path)
        buf = C.create_string_buffer(128)
        self._ck(self._L.fibhip_comm_unique_id(buf))
        return buf.raw

    def comm_check(self, rank, nranks):
        """the local checks of comm_init (no collective): raises if this rank could not join"""
        self._ck(self._L.fibhip_comm_check(self._h, rank, nranks))

    def comm_init(self, unique_id, rank, nranks, librccl_path=None):
        self._ck(self._L.fibhip_comm_open(librccl_path.encode() if librccl_path else None))
        assert len(unique_id) == 128
        self._ck(self._L.fibhip_comm_init(self._h, unique_id, rank, nranks))

    def halo_plan(self, up, down):
        """[(offset, count, peer, send)], slab index: the messages of this exchange tick (include/fibhip.h)"""
        msg = (HaloMsg * 4)()
        idx = C.c_int()
        n = self._ck(self._L.fibhip_halo_plan(self._h, -1 if up is None else up, -1 if down is None else down, msg,
                                              C.byref(idx)))
        return [(m.offset, m.count, m.peer, bool(m.send)) for m in msg[:n]], idx.value

    def comm_free(self):
        self._L.fibhip_comm_free(self._h)

    def comm_exchange(self, up, down):
        self._ck(self._L.fibhip_comm_exchange(self._h, -1 if up is None else up, -1 if down is None else down))

    def launch_plan(self):
        k, n = C.c_int(), C.c_int()
        self._ck(self._L.fibhip_launch_plan(self._h, C.byref(k), C.byref(n)))
        return k.value, n.value

    def plan_tile(self):
        """(tile width, tile height, rows per wave of a strip kernel | -threads of a flat tile kernel) of the dominant launch"""
        w, t, r = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.fibhip_plan_tile(self._h, C.byref(w), C.byref(t), C.byref(r)))
        return w.value, t.value, r.value

    def trace_begin(self):
        self._ck(self._L.fibhip_trace_begin(self._h))

    def trace_end(self):
        """[{'name', 'ts' (us from the first launch), 'dur' (us), 'K', 'tile', 'ticks'}] of the launches since trace_begin"""
        cap = 1024
        ev = (TraceEvent * cap)()
        n = self._ck(self._L.fibhip_trace_end(self._h, ev, cap))
        self.trace_truncated = n > cap                  # (more launches than the buffer holds: the first `cap` are returned)
        return [{'name': e.name.decode(), 'ts': e.start_us, 'dur': e.dur_us, 'K': e.K, 'tile': (e.tile_w, e.tile_h, e.rows_per_wave),
                 'ticks': e.ticks} for e in ev[:min(n, cap)]]

    def trace_tick(self):
        """one tick with every launch between two HIP events (the timeline of ionic.py:231-241)"""
        self.trace_begin()
        self.step(1)
        return self.trace_end()

    def launch_stats(self):
        """{'launches', 'ticks', 'mt_launches', 'mt_ticks'} since the handle was created"""
        out = (C.c_longlong * 4)()
        self._ck(self._L.fibhip_launch_stats(self._h, out))
        d = dict(zip(('launches', 'ticks', 'mt_launches', 'mt_ticks'), [int(x) for x in out]))
        sp = (C.c_longlong * 2)()
        self._ck(self._L.fibhip_spec_stats(self._h, sp))
        d.update(ahead_stopped_in_time=int(sp[0]), ahead_recomputed=int(sp[1]))
        fb = self.fallbacks()
        d.update(gave_up_recovered=fb[0], ticks_recomputed_after_give_up=fb[1])
        return d

    def ticks_per_launch(self):
        """consecutive ticks one launch can cover (Courtemanche, fast policy, one device: 3; Fenton / Beeler-Reuter on a
        grid whose tiles are all resident at once: FIBHIP_MT_MAX, default 32, and 256 while a series of 128 ticks or more
        declared with expect() is running; otherwise 1)"""
        return self._ck(self._L.fibhip_ticks_per_launch(self._h))

    # ---- activation recorder (include/fibhip.h fibhip_observe_*) --------------------------------------------------
    def observe_begin(self, var, up, down):
        """attaches (or re-attaches, clearing the maps) the per-cell activation recorder on array `var`"""
        self._ck(self._L.fibhip_observe_begin(self._h, int(var), float(up), float(down)))

    def observe_get(self, which):
        """one map as a [height, width] array: 'first_up', 'last_up', 'prev_up', 'apd' (float32) or 'count' (int32)"""
        k = OBS_MAPS.index(which)
        out = np.empty((self.height, self.width), np.int32 if which == 'count' else np.float32)
        self._ck(self._L.fibhip_observe_get(self._h, k, out.ctypes.data_as(C.c_void_p)))
        return out

    def observe_ticks(self):
        """ticks observed since observe_begin"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_observe_ticks(self._h, C.byref(k)))
        return int(k.value)

    def observe_end(self):
        self._ck(self._L.fibhip_observe_end(self._h))

    # ---- electrode recorder (include/fibhip.h fibhip_electrode_*) -------------------------------------------------
    def electrode_begin(self, var, rects, patches, every=1, capacity=1):
        """attaches (or re-attaches, with an empty trace) the electrode recorder on array `var`: `rects` is a list of
        (r0, r1, c0, c1), `patches` the float32 weight arrays of those shapes; one sample every `every` ticks, `capacity`
        samples at the most"""
        rects = np.ascontiguousarray(rects, np.intc).reshape(-1, 4)
        if len(patches) != len(rects):
            raise ValueError('electrode_begin: %d rectangles but %d weight patches' % (len(rects), len(patches)))
        flat = []
        for (r0, r1, c0, c1), w in zip(rects, patches):
            w = np.asarray(w, np.float32)
            if w.shape != (r1 - r0, c1 - c0):
                raise ValueError('electrode_begin: a patch of shape %s for rows [%d, %d) x columns [%d, %d)' % (w.shape, r0, r1, c0, c1))
            flat.append(w.ravel())
        weights = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(1), np.float32)
        self._ck(self._L.fibhip_electrode_begin(self._h, int(var), len(rects), rects.ctypes.data_as(_ip), weights.ctypes.data_as(_fp),
                                                int(every), int(capacity)))
        self._el_n = len(rects)

    def electrode_count(self):
        """samples taken since electrode_begin (ticks accepted but not launched yet included)"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_electrode_count(self._h, C.byref(k)))
        return int(k.value)

    def electrode_read(self, first=0, count=None):
        """samples [first, first + count) as a float32 [count, n] array (count=None: all taken so far); blocks like
        get_state, detaches nothing"""
        if count is None:
            count = self.electrode_count() - int(first)
        n = getattr(self, '_el_n', 0)
        out = np.empty((max(int(count), 0), n), np.float32)
        self._ck(self._L.fibhip_electrode_read(self._h, int(first), int(count), out.ctypes.data_as(_fp)))
        return out

    def electrode_end(self):
        self._ck(self._L.fibhip_electrode_end(self._h))

    # ---- tip recorder (include/fibhip.h fibhip_tips_*) ------------------------------------------------------------
    def tips_begin(self, var, var2, a0, b0, mask=None, every=1, max_tips=256, capacity=1):
        """attaches (or re-attaches, with empty lists) the tip recorder on arrays `var`, `var2` with the levels `a0`, `b0`;
        `mask`: [height, width], non-zero where a cell counts, or None; one sample every `every` ticks, `capacity` samples of
        up to `max_tips` tips at the most"""
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.shape != (self.height, self.width):
                raise ValueError('tips_begin: a mask of shape %s on a %d x %d grid' % (mask.shape, self.height, self.width))
            mp = mask.ctypes.data_as(C.POINTER(C.c_ubyte))
        self._ck(self._L.fibhip_tips_begin(self._h, int(var), int(var2), float(a0), float(b0), mp, int(every), int(max_tips),
                                           int(capacity)))
        self._tip_max = int(max_tips)

    def tips_count(self):
        """samples taken since tips_begin (ticks accepted but not launched yet included)"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_tips_count(self._h, C.byref(k)))
        return int(k.value)

    def tips_read(self, first=0, count=None, records=True):
        """samples [first, first + count) (count=None: all taken so far) as (counts, records): counts int32 [count, 3] =
        n_pos, n_neg, stored; records int32 [count, max_tips, 4] = row, column, charge, 0, of which the first
        min(stored, max_tips) of each sample are valid, in no fixed order (records=False: None).  Blocks like get_state,
        detaches nothing"""
        if count is None:
            count = self.tips_count() - int(first)
        n = max(int(count), 0)
        counts = np.zeros((n, 3), np.int32)
        recs = np.zeros((n, getattr(self, '_tip_max', 0), 4), np.int32) if records else None
        self._ck(self._L.fibhip_tips_read(self._h, int(first), int(count), counts.ctypes.data_as(_ip),
                                          recs.ctypes.data_as(_ip) if records else None))
        return counts, recs

    def tips_end(self):
        self._ck(self._L.fibhip_tips_end(self._h))

    # ---- frame recorder (include/fibhip.h fibhip_frames_*) --------------------------------------------------------
    def frames_begin(self, var=0, window=None, block=(1, 1), reduce='mean', lo=0.0, span=1.0, weight=None, fmt='float32', every=1,
                     first=None, capacity=1):
        """attaches (or re-attaches, with an empty cube) the frame recorder on array `var`: `window` = (r0, r1, c0, c1) (None:
        the whole grid), `block` = (by, bx), `reduce` 'point' / 'mean', the levels of y = (X - lo) / span, `weight` an
        [height, width] float32 plane or None, `fmt` 'float32' / 'uint8'; a frame after ticks first, first + every, ...
        (first=None: every), `capacity` frames at the most"""
        win = np.ascontiguousarray((0, self.height, 0, self.width) if window is None else window, np.intc).reshape(4)
        wp = None
        if weight is not None:
            weight = np.ascontiguousarray(weight, np.float32)
            if weight.shape != (self.height, self.width):
                raise ValueError('frames_begin: a weight plane of shape %s on a %d x %d grid' % (weight.shape, self.height, self.width))
            wp = weight.ctypes.data_as(_fp)
        self._ck(self._L.fibhip_frames_begin(self._h, int(var), win.ctypes.data_as(_ip), int(block[0]), int(block[1]),
                                             FRAME_REDUCE.index(reduce), float(lo), float(span), wp, FRAME_FORMAT.index(fmt),
                                             int(every), int(every if first is None else first), int(capacity)))

    def frames_count(self):
        """frames taken since frames_begin (ticks accepted but not launched yet included)"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_frames_count(self._h, C.byref(k)))
        return int(k.value)

    def frames_shape(self):
        """(oh, ow, dtype) of the attached recorder's frames"""
        oh, ow, bpp = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.fibhip_frames_shape(self._h, C.byref(oh), C.byref(ow), C.byref(bpp)))
        return int(oh.value), int(ow.value), np.dtype(np.uint8 if bpp.value == 1 else np.float32)

    def frames_read(self, first=0, count=None):
        """frames [first, first + count) as a [count, oh, ow] array of float32 or uint8 (count=None: all taken so far); blocks
        like get_state, detaches nothing"""
        if count is None:
            count = self.frames_count() - int(first)
        oh, ow, dtype = self.frames_shape()
        out = np.empty((max(int(count), 0), oh, ow), dtype)
        self._ck(self._L.fibhip_frames_read(self._h, int(first), int(count), out.ctypes.data_as(C.c_void_p)))
        return out

    def frames_end(self):
        self._ck(self._L.fibhip_frames_end(self._h))

    # ---- spectrum recorder (include/fibhip.h fibhip_spectrum_*) ----------------------------------------------------
    def spectrum_begin(self, var=0, window=None, block=(1, 1), reduce='mean', weight=None, every=1, nfft=128, win=None, tw=None,
                       bins=(2,), chunk=1):
        """attaches the spectrum recorder on array `var`: the frame recorder's `window`, `block`, `reduce` and `weight` (levels
        0 and 1), a sample every `every` ticks, segments of `nfft` samples weighted by `win` [nfft] float32, the twiddle table
        `tw` [nfft, 2] float32 (cos, -sin of 2 pi m / nfft), the strictly ascending frequency indices `bins` (at most 128, each
        in [0, nfft / 2]) and `chunk` (1 .. 32, a divisor of nfft): the samples folded by one launch"""
        wnd = np.ascontiguousarray((0, self.height, 0, self.width) if window is None else window, np.intc).reshape(4)
        wp = None
        if weight is not None:
            weight = np.ascontiguousarray(weight, np.float32)
            if weight.shape != (self.height, self.width):
                raise ValueError('spectrum_begin: a weight plane of shape %s on a %d x %d grid' % (weight.shape, self.height, self.width))
            wp = weight.ctypes.data_as(_fp)
        win = np.ascontiguousarray(win, np.float32)
        tw = np.ascontiguousarray(tw, np.float32)
        if win.shape != (int(nfft),) or tw.shape != (int(nfft), 2):
            raise ValueError('spectrum_begin: win must be [nfft] and tw [nfft, 2] (got %s and %s for nfft = %d)' % (win.shape, tw.shape, nfft))
        b = np.ascontiguousarray(bins, np.intc).reshape(-1)
        self._ck(self._L.fibhip_spectrum_begin(self._h, int(var), wnd.ctypes.data_as(_ip), int(block[0]), int(block[1]),
                                               FRAME_REDUCE.index(reduce), wp, int(every), int(nfft), win.ctypes.data_as(_fp),
                                               tw.ctypes.data_as(_fp), int(b.size), b.ctypes.data_as(_ip), int(chunk)))

    def spectrum_count(self):
        """(samples taken, segments finished) since spectrum_begin (ticks accepted but not launched yet included)"""
        s, g = C.c_longlong(), C.c_longlong()
        self._ck(self._L.fibhip_spectrum_count(self._h, C.byref(s), C.byref(g)))
        return int(s.value), int(g.value)

    def spectrum_shape(self):
        """(oh, ow, nb) of the attached recorder"""
        oh, ow, nb = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.fibhip_spectrum_shape(self._h, C.byref(oh), C.byref(ow), C.byref(nb)))
        return int(oh.value), int(ow.value), int(nb.value)

    def spectrum_read(self):
        """(P [nb, oh, ow] float32, segments): the power summed over the finished segments; blocks like get_state"""
        oh, ow, nb = self.spectrum_shape()
        out = np.empty((nb, oh, ow), np.float32)
        seg = C.c_longlong()
        self._ck(self._L.fibhip_spectrum_read(self._h, out.ctypes.data_as(_fp), C.byref(seg)))
        return out, int(seg.value)

    def spectrum_peak(self, a, b, halfwidth=1):
        """(kpeak int32, ppeak, pband, pnear float32), each [oh, ow], over the bin positions a <= i <= b"""
        oh, ow, _ = self.spectrum_shape()
        kp = np.empty((oh, ow), np.int32)
        pp, pb, pn = (np.empty((oh, ow), np.float32) for _ in range(3))
        self._ck(self._L.fibhip_spectrum_peak(self._h, int(a), int(b), int(halfwidth), kp.ctypes.data_as(_ip), pp.ctypes.data_as(_fp),
                                              pb.ctypes.data_as(_fp), pn.ctypes.data_as(_fp)))
        return kp, pp, pb, pn

    def spectrum_end(self):
        self._ck(self._L.fibhip_spectrum_end(self._h))

    # ---- beat recorder (include/fibhip.h fibhip_beats_*) -----------------------------------------------------------
    def beats_begin(self, var=0, window=None, block=(1, 1), reduce='mean', weight=None, every=1, up=0.5, down=0.1, depth=8):
        """attaches the beat recorder on array `var`: the frame recorder's `window`, `block`, `reduce` and `weight` (levels 0
        and 1), a sample every `every` ticks, the levels `down` <= `up` and a ring of `depth` (1 .. 16) beats per pixel"""
        wnd = np.ascontiguousarray((0, self.height, 0, self.width) if window is None else window, np.intc).reshape(4)
        wp = None
        if weight is not None:
            weight = np.ascontiguousarray(weight, np.float32)
            if weight.shape != (self.height, self.width):
                raise ValueError('beats_begin: a weight plane of shape %s on a %d x %d grid' % (weight.shape, self.height, self.width))
            wp = weight.ctypes.data_as(_fp)
        self._ck(self._L.fibhip_beats_begin(self._h, int(var), wnd.ctypes.data_as(_ip), int(block[0]), int(block[1]),
                                            FRAME_REDUCE.index(reduce), wp, int(every), float(np.float32(up)), float(np.float32(down)),
                                            int(depth)))

    def beats_count(self):
        """samples taken since beats_begin (ticks accepted but not launched yet included)"""
        s = C.c_longlong()
        self._ck(self._L.fibhip_beats_count(self._h, C.byref(s)))
        return int(s.value)

    def beats_shape(self):
        """(oh, ow, depth) of the attached recorder"""
        oh, ow, d = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.fibhip_beats_shape(self._h, C.byref(oh), C.byref(ow), C.byref(d)))
        return int(oh.value), int(ow.value), int(d.value)

    def beats_read(self):
        """(t_up, t_down, peak float32 [depth, oh, ow] in SLOT order — beat b in slot b % depth —, count int32 [oh, ow], pk
        float32 [oh, ow]); blocks like get_state"""
        oh, ow, d = self.beats_shape()
        tu, td, pe = (np.empty((d, oh, ow), np.float32) for _ in range(3))
        n = np.empty((oh, ow), np.int32)
        pk = np.empty((oh, ow), np.float32)
        self._ck(self._L.fibhip_beats_read(self._h, tu.ctypes.data_as(_fp), td.ctypes.data_as(_fp), pe.ctypes.data_as(_fp),
                                           n.ctypes.data_as(_ip), pk.ctypes.data_as(_fp)))
        return tu, td, pe, n, pk

    def beats_summary(self, last):
        """(nused int32, apd_mean, cl_mean, apd_alt float32), each [oh, ow], over the newest `last` beats"""
        oh, ow, _ = self.beats_shape()
        nu = np.empty((oh, ow), np.int32)
        am, cm, al = (np.empty((oh, ow), np.float32) for _ in range(3))
        self._ck(self._L.fibhip_beats_summary(self._h, int(last), nu.ctypes.data_as(_ip), am.ctypes.data_as(_fp), cm.ctypes.data_as(_fp),
                                              al.ctypes.data_as(_fp)))
        return nu, am, cm, al

    def beats_end(self):
        self._ck(self._L.fibhip_beats_end(self._h))

    # ---- statistics recorder (include/fibhip.h fibhip_stats_*) ----------------------------------------------------
    def stats_begin(self, cols, weight=None, mask=None, every=1, capacity=1):
        """attaches the statistics recorder: `cols` is a list of (var, kind, level) with kind one of STAT_KINDS (or its
        number), `weight` an [height, width] float32 plane or None (what SUM columns weigh with), `mask` an [height, width]
        array, non-zero where a cell counts for the other kinds, or None; one row of float64 every `every` ticks, `capacity`
        rows at the most"""
        arr = (StatCol * max(len(cols), 1))()
        for i, (var, kind, level) in enumerate(cols):
            arr[i].var, arr[i].kind = int(var), STAT_KINDS.index(kind) if isinstance(kind, str) else int(kind)
            arr[i].level = float(level)
        wp = mp = None
        if weight is not None:
            weight = np.ascontiguousarray(weight, np.float32)
            if weight.shape != (self.height, self.width):
                raise ValueError('stats_begin: a weight plane of shape %s on a %d x %d grid' % (weight.shape, self.height, self.width))
            wp = weight.ctypes.data_as(_fp)
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.shape != (self.height, self.width):
                raise ValueError('stats_begin: a mask of shape %s on a %d x %d grid' % (mask.shape, self.height, self.width))
            mp = mask.ctypes.data_as(C.POINTER(C.c_ubyte))
        self._ck(self._L.fibhip_stats_begin(self._h, len(cols), arr, wp, mp, int(every), int(capacity)))
        self._st_n = len(cols)

    def stats_count(self):
        """samples taken since stats_begin (ticks accepted but not launched yet included)"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_stats_count(self._h, C.byref(k)))
        return int(k.value)

    def stats_read(self, first=0, count=None):
        """samples [first, first + count) as a float64 [count, ncols] array (count=None: all taken so far); blocks like
        get_state, detaches nothing"""
        if count is None:
            count = self.stats_count() - int(first)
        out = np.empty((max(int(count), 0), getattr(self, '_st_n', 0)), np.float64)
        self._ck(self._L.fibhip_stats_read(self._h, int(first), int(count), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def stats_end(self):
        self._ck(self._L.fibhip_stats_end(self._h))

    # ---- lead recorder (include/fibhip.h fibhip_leads_*) ----------------------------------------------------------
    def leads_begin(self, pos, tables, weight=None, var=0, every=1, capacity=1):
        """attaches the lead recorder: `pos` is a list of (row, col, table), `tables` a float32 [ntables, height, width] array
        of lead-field tables, `weight` an [height, width] float32 plane or None (weight 1); one row of float64, one value per
        lead, every `every` ticks, `capacity` rows at the most"""
        pos = np.ascontiguousarray(pos, np.int32).reshape(-1, 3)
        tables = np.ascontiguousarray(tables, np.float32)
        if tables.ndim != 3 or tables.shape[1:] != (self.height, self.width):
            raise ValueError('leads_begin: tables of shape %s on a %d x %d grid' % (tables.shape, self.height, self.width))
        wp = None
        if weight is not None:
            weight = np.ascontiguousarray(weight, np.float32)
            if weight.shape != (self.height, self.width):
                raise ValueError('leads_begin: a weight plane of shape %s on a %d x %d grid' % (weight.shape, self.height, self.width))
            wp = weight.ctypes.data_as(_fp)
        self._ck(self._L.fibhip_leads_begin(self._h, int(var), len(pos), pos.ctypes.data_as(_ip), len(tables), tables.ctypes.data_as(_fp), wp,
                                            int(every), int(capacity)))
        self._ld_n = len(pos)

    def leads_count(self):
        """samples taken since leads_begin (ticks accepted but not launched yet included)"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_leads_count(self._h, C.byref(k)))
        return int(k.value)

    def leads_read(self, first=0, count=None):
        """samples [first, first + count) as a float64 [count, nleads] array (count=None: all taken so far); blocks like
        get_state, detaches nothing"""
        if count is None:
            count = self.leads_count() - int(first)
        out = np.empty((max(int(count), 0), getattr(self, '_ld_n', 0)), np.float64)
        self._ck(self._L.fibhip_leads_read(self._h, int(first), int(count), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def leads_end(self):
        self._ck(self._L.fibhip_leads_end(self._h))

    # ---- wave recorder (include/fibhip.h fibhip_waves_*) ----------------------------------------------------------
    def waves_begin(self, var=0, kind=0, level=0.0, var2=-1, kind2=0, level2=0.0, conn=4, mask=None, max_waves=256, every=1, capacity=1):
        """attaches (or re-attaches, with empty lists) the wave recorder: a cell is set where `mask` ([height, width], or None:
        everywhere) is non-zero and array `var` is above (`kind` 0) or below (1) `level`, and array `var2` (-1: none) meets
        (`kind2`, `level2`) too; the connected components under `conn` = 4 or 8 are the waves; one sample every `every` ticks,
        `capacity` samples of up to `max_waves` records at the most"""
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.shape != (self.height, self.width):
                raise ValueError('waves_begin: a mask of shape %s on a %d x %d grid' % (mask.shape, self.height, self.width))
            mp = mask.ctypes.data_as(C.POINTER(C.c_ubyte))
        self._ck(self._L.fibhip_waves_begin(self._h, int(var), int(kind), float(level), int(var2), int(kind2), float(level2), int(conn), mp,
                                            int(max_waves), int(every), int(capacity)))
        self._wave_max = int(max_waves)
        self._wave_link_max = 0

    def waves_links_begin(self, max_links=512):
        """turns links on for the wave recorder just attached (before its first tick): per sample, which waves of the sample
        before share cells with which waves of this one, up to `max_links` records (prev, seed, overlap)"""
        self._ck(self._L.fibhip_waves_links_begin(self._h, int(max_links)))
        self._wave_link_max = int(max_links)

    def waves_links_read(self, first=0, count=None, records=True):
        """samples [first, first + count) (count=None: all taken so far) as (counts, links): counts int32 [count, 4] = links,
        stored, cells, lost; links WAVE_LINK_DTYPE [count, max_links], of which the first `stored` of each sample are valid, in
        no fixed order (records=False: None).  Blocks like waves_read; refused while links are off"""
        if count is None:
            count = self.waves_count() - int(first)
        n = max(int(count), 0)
        counts = np.zeros((n, 4), np.int32)
        recs = np.zeros((n, getattr(self, '_wave_link_max', 0)), WAVE_LINK_DTYPE) if records else None
        self._ck(self._L.fibhip_waves_links_read(self._h, int(first), int(count), counts.ctypes.data_as(_ip),
                                                 recs.ctypes.data_as(C.c_void_p) if records else None))
        return counts, recs

    def waves_count(self):
        """samples taken since waves_begin (ticks accepted but not launched yet included)"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_waves_count(self._h, C.byref(k)))
        return int(k.value)

    def waves_read(self, first=0, count=None, records=True):
        """samples [first, first + count) (count=None: all taken so far) as (counts, records): counts int32 [count, 3] = n,
        stored, cells; records WAVE_RECORD_DTYPE [count, max_waves], of which the first `stored` of each sample are valid, in
        no fixed order (records=False: None).  Blocks like get_state, detaches nothing"""
        if count is None:
            count = self.waves_count() - int(first)
        n = max(int(count), 0)
        counts = np.zeros((n, 3), np.int32)
        recs = np.zeros((n, getattr(self, '_wave_max', 0)), WAVE_RECORD_DTYPE) if records else None
        self._ck(self._L.fibhip_waves_read(self._h, int(first), int(count), counts.ctypes.data_as(_ip),
                                           recs.ctypes.data_as(C.c_void_p) if records else None))
        return counts, recs

    def waves_labels(self):
        """the label plane of the latest sample: int32 [height, width], the seed of the cell's wave or -1"""
        out = np.empty((self.height, self.width), np.int32)
        self._ck(self._L.fibhip_waves_labels(self._h, out.ctypes.data_as(_ip)))
        return out

    def waves_end(self):
        self._ck(self._L.fibhip_waves_end(self._h))
        self._wave_link_max = 0

    # ---- stimulus program (include/fibhip.h fibhip_stim_*) --------------------------------------------------------
    def stim_begin(self, entries, planes=None):
        """attaches a stimulus program: `entries` is a list of dicts with the fields of fibhip_stim_entry (`mode` 'max' / 'add'
        or its number, `shape` 'rect' / 'plane' or its number; fields left out are 0, hold and count 1), `planes` a list of
        [height, width] float32 arrays the 'plane' entries index"""
        arr = (StimEntry * max(len(entries), 1))()
        for i, e in enumerate(entries):
            d = dict(e)
            mode, shape = d.pop('mode', 0), d.pop('shape', 0)
            arr[i].mode = STIM_MODES.index(mode) if isinstance(mode, str) else int(mode)
            arr[i].shape = STIM_SHAPES.index(shape) if isinstance(shape, str) else int(shape)
            arr[i].hold, arr[i].count = int(d.pop('hold', 1)), int(d.pop('count', 1))
            arr[i].v, arr[i].floor = float(d.pop('v', 0.0)), float(d.pop('floor', 0.0))
            for k, val in d.items():
                if k not in ('var', 'r0', 'r1', 'c0', 'c1', 'plane', 'first', 'period'):
                    raise ValueError('stim_begin: entry %d: unknown field %r' % (i, k))
                setattr(arr[i], k, int(val))
        pp, stack = None, None
        if planes is not None and len(planes):
            for p in planes:
                if np.shape(p) != (self.height, self.width):
                    raise ValueError('stim_begin: a plane of shape %s on a %d x %d grid' % (np.shape(p), self.height, self.width))
            stack = np.ascontiguousarray(np.stack([np.asarray(p, np.float32) for p in planes]), np.float32)
            pp = stack.ctypes.data_as(_fp)
        self._ck(self._L.fibhip_stim_begin(self._h, len(entries), arr, 0 if stack is None else len(stack), pp))

    def stim_count(self):
        """events applied since stim_begin (flushes: the ticks accepted so far are launched first)"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_stim_count(self._h, C.byref(k)))
        return int(k.value)

    def stim_end(self):
        self._ck(self._L.fibhip_stim_end(self._h))

    # ---- lesion program (include/fibhip.h fibhip_lesion_*) --------------------------------------------------------
    def lesion_begin(self, lesions):
        """attaches a lesion program: `lesions` is a list of (tick, (r0, r1, c0, c1), patch) — the patch a float32
        [r1 - r0, c1 - c0] array of factors in [0, 1] — applied to the phase field right after tick `tick`, in list order"""
        arr = (LesionEntry * max(len(lesions), 1))()
        flat, off = [], 0
        for i, (tick, box, patch) in enumerate(lesions):
            r0, r1, c0, c1 = (int(a) for a in box)
            p = np.ascontiguousarray(patch, np.float32)
            if p.shape != (r1 - r0, c1 - c0):
                raise ValueError('lesion_begin: entry %d: a patch of shape %s on the box rows [%d, %d) x columns [%d, %d)' % (i, p.shape, r0, r1, c0, c1))
            arr[i].offset, arr[i].tick = off, int(tick)
            arr[i].r0, arr[i].r1, arr[i].c0, arr[i].c1 = r0, r1, c0, c1
            flat.append(p.ravel())
            off += p.size
        packed = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(1), np.float32)
        self._ck(self._L.fibhip_lesion_begin(self._h, len(lesions), arr, off, packed.ctypes.data_as(_fp)))

    def lesion_count(self):
        """entries applied since lesion_begin (ticks accepted but not launched yet count)"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_lesion_count(self._h, C.byref(k)))
        return int(k.value)

    def lesion_end(self):
        self._ck(self._L.fibhip_lesion_end(self._h))

    def lesion_apply(self, box, patch):
        """one lesion now: phi = max(phi * patch, 1e-5) on the box (r0, r1, c0, c1), the derived planes recomputed around it"""
        b = np.asarray([int(a) for a in box], np.int32)
        p = np.ascontiguousarray(patch, np.float32)
        if b.shape != (4,) or p.shape != (int(b[1] - b[0]), int(b[3] - b[2])):
            raise ValueError('lesion_apply: a patch of shape %s on the box %s' % (p.shape, tuple(int(a) for a in b)))
        self._ck(self._L.fibhip_lesion_apply(self._h, b.ctypes.data_as(_ip), p.ctypes.data_as(_fp)))
        self._fallback_warning()

    def get_phase(self):
        """the handle's current phase field, float32 [height, width]"""
        out = np.empty((self.height, self.width), np.float32)
        self._ck(self._L.fibhip_get_phase(self._h, out.ctypes.data_as(_fp)))
        self._fallback_warning()
        return out

    # ---- trigger program (include/fibhip.h fibhip_trig_*) ---------------------------------------------------------
    def trig_begin(self, sensors, rules, planes=None, every=1, capacity=4096):
        """attaches a trigger program: `sensors` is a list of dicts with the fields of fibhip_trig_sensor (`site` 'rect' with r0,
        r1, c0, c1, or 'mask' with `mask`, a [height, width] array whose non-zero cells are the site), `rules` a list of dicts
        with the fields of fibhip_trig_rule (`edge` 'rise' / 'fall', `mode` 'max' / 'add', `shape` 'rect' / 'plane', or their
        numbers; fields left out are 0, count and hold 1), `planes` the [height, width] float32 arrays the 'plane' stimuli index"""
        sa = (TrigSensor * max(len(sensors), 1))()
        masks = []
        for i, q in enumerate(sensors[:MAX_TRIG_SENSORS]):
            d = dict(q)
            site = d.pop('site', 0)
            sa[i].site = TRIG_SITES.index(site) if isinstance(site, str) else int(site)
            sa[i].level, sa[i].need = float(d.pop('level', 0.0)), int(d.pop('need', 1))
            mask = d.pop('mask', None)
            if sa[i].site == 1:
                if mask is None or np.shape(mask) != (self.height, self.width):
                    raise ValueError('trig_begin: sensor %d: a mask of shape %s on a %d x %d grid' % (i, np.shape(mask), self.height, self.width))
                masks.append((np.asarray(mask) != 0).astype(np.uint8))
            for k, val in d.items():
                if k not in ('var', 'r0', 'r1', 'c0', 'c1'):
                    raise ValueError('trig_begin: sensor %d: unknown field %r' % (i, k))
                setattr(sa[i], k, int(val))
        ra = (TrigRule * max(len(rules), 1))()
        for i, q in enumerate(rules[:MAX_TRIG_RULES]):
            d = dict(q)
            edge, mode, shape = d.pop('edge', 0), d.pop('mode', 0), d.pop('shape', 0)
            ra[i].edge = TRIG_EDGES.index(edge) if isinstance(edge, str) else int(edge)
            ra[i].mode = STIM_MODES.index(mode) if isinstance(mode, str) else int(mode)
            ra[i].shape = STIM_SHAPES.index(shape) if isinstance(shape, str) else int(shape)
            ra[i].hold, ra[i].count = int(d.pop('hold', 1)), int(d.pop('count', 1))
            ra[i].v, ra[i].floor = float(d.pop('v', 0.0)), float(d.pop('floor', 0.0))
            for k, val in d.items():
                if k not in ('sensor', 'arm', 'blank', 'escape', 'max_det', 'delay', 'period', 'var', 'r0', 'r1', 'c0', 'c1', 'plane'):
                    raise ValueError('trig_begin: rule %d: unknown field %r' % (i, k))
                setattr(ra[i], k, int(val))
        mp, mstack = None, None
        if masks:
            mstack = np.ascontiguousarray(np.stack(masks), np.uint8)
            mp = mstack.ctypes.data_as(C.POINTER(C.c_ubyte))
        pp, stack = None, None
        if planes is not None and len(planes):
            for p in planes:
                if np.shape(p) != (self.height, self.width):
                    raise ValueError('trig_begin: a plane of shape %s on a %d x %d grid' % (np.shape(p), self.height, self.width))
            stack = np.ascontiguousarray(np.stack([np.asarray(p, np.float32) for p in planes]), np.float32)
            pp = stack.ctypes.data_as(_fp)
        self._ck(self._L.fibhip_trig_begin(self._h, len(sensors), sa, mp, len(rules), ra, 0 if stack is None else len(stack), pp, int(every),
                                           int(capacity)))
        self._trig_n = len(rules)

    def trig_count(self):
        """samples taken since trig_begin (ticks accepted but not launched yet included)"""
        k = C.c_longlong()
        self._ck(self._L.fibhip_trig_count(self._h, C.byref(k)))
        return int(k.value)

    def trig_read(self, first=0, count=None):
        """rows [first, first + count) of the log as an int32 [count, nrules, 6] array — c, a, t, n, cause, fired — (count=None:
        all taken so far); blocks like get_state, detaches nothing"""
        if count is None:
            count = self.trig_count() - int(first)
        out = np.empty((max(int(count), 0), getattr(self, '_trig_n', 0), len(TRIG_FIELDS)), np.int32)
        self._ck(self._L.fibhip_trig_read(self._h, int(first), int(count), out.ctypes.data_as(_ip)))
        return out

    def trig_end(self):
        self._ck(self._L.fibhip_trig_end(self._h))
