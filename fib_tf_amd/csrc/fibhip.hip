// fibhip.hip — C ABI (include/fibhip.h) over the gfx950 kernels of kernels.hpp.
//
// Host-side responsibilities: device memory for the SoA slabs (ping/pong), the per-tick launch
// plan (how many sub-steps each launch fuses), the per-variable buffer bookkeeping, the
// edge/interior split used by the row-block multi-GPU driver, and HIP-event timing.
// There is no CPU path in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <limits>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "../../include/fibhip.h"
#include "kernels.hpp"

using namespace fib;

// One translation unit, in dependency order.  fib_tf_amd/_lib.py DEPS is every *.hpp, *.inc and *.hip of this directory.
#include "host_util.hpp"    // fail, HIPCHK, the spin-waits
#include "launch.hpp"       // LaunchCtx, the launchers, the variant table
#include "ctx.hpp"          // fibhip_ctx and its parts, NEED / FLUSH / CONFIRM / SYNC_S0, the timeline
#include "recorders.hpp"    // the table of the hooks behind a committed launch, in hook order
#include "tick.inc"         // one tick: pointer tables, rows, edges / interior / commit
#include "sched.inc"        // when ticks are launched: deferral, multi-tick launches, run-ahead, journal and recovery, fibhip_step
#include "record.inc"       // the ten recorders (activation, electrode, tip, frame, statistics, lead, potential map, wave, spectrum,
                            // beat) and the velocity fit; the stimulus, trigger and lesion programs; includes attach_checks.hpp
#include "plan.inc"         // build_plan, autotune
#include "comm.inc"         // the RCCL halo path and fibhip_halo_plan
// this file: create / destroy, state get / set, pointwise modes, pace / probe / sync / timing, run-time modules, accessors and
// statistics; unit.inc (at the end): the entry points that need no handle

extern "C" int fibhip_nvar(int model)
{
    switch (model) {
    case FIBHIP_FENTON4V: return Fenton::NVAR;
    case FIBHIP_BR: return BeelerReuter::NVAR;
    case FIBHIP_COURT: return Courtemanche::NVAR;
    case FIBHIP_COURT_US: return CourtemancheUS::NVAR;
#ifdef FIB_CUSTOM_MODEL_INC
    case FIBHIP_CUSTOM: return Custom::NVAR;
#endif
    default: return fail(FIBHIP_EINVAL, "unknown model %d", model);
    }
}

extern "C" int fibhip_default_steps_per_tick(int model)
{
    switch (model) {
    case FIBHIP_FENTON4V: return Fenton::DEFAULT_STEPS;
    case FIBHIP_BR: return BeelerReuter::DEFAULT_STEPS;
    case FIBHIP_COURT: return Courtemanche::DEFAULT_STEPS;
    case FIBHIP_COURT_US: return CourtemancheUS::DEFAULT_STEPS;
#ifdef FIB_CUSTOM_MODEL_INC
    case FIBHIP_CUSTOM: return Custom::DEFAULT_STEPS;
#endif
    default: return fail(FIBHIP_EINVAL, "unknown model %d", model);
    }
}

extern "C" int fibhip_abi_version(void) { return FIBHIP_ABI_VERSION; }

extern "C" int fibhip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int create_impl(const fibhip_desc *desc, fibhip_ctx *&h)
{
    if (desc->struct_size != (int)sizeof(fibhip_desc))
        return fail(FIBHIP_EINVAL, "fibhip_desc size mismatch: caller %d, library %d", desc->struct_size,
                    (int)sizeof(fibhip_desc));
    fibhip_module *mod = (fibhip_module *)desc->module;
    if (mod && desc->model != FIBHIP_CUSTOM) return fail(FIBHIP_EINVAL, "a run-time module serves FIBHIP_CUSTOM only");
    if (mod && mod->device != desc->device)
        return fail(FIBHIP_EINVAL, "the module was loaded on device %d, the handle asks for device %d", mod->device, desc->device);
    const int nv = mod ? mod->nvar : fibhip_nvar(desc->model);
    if (nv < 0) return nv;
    const int Hg = desc->global_height ? desc->global_height : desc->height;
    if (desc->height < 3 || desc->width < 3 || Hg < 3)
        return fail(FIBHIP_EINVAL, "grid must be at least 3x3 (got %dx%d)", desc->height, desc->width);
    if (desc->row_offset < 0 || desc->row_offset + desc->height > Hg || desc->ghost_top < 0 || desc->ghost_bottom < 0 ||
        desc->ghost_top + desc->ghost_bottom >= desc->height)
        return fail(FIBHIP_EINVAL, "inconsistent row-block description");
    if ((desc->ghost_top > 0) != (desc->row_offset > 0) ||
        (desc->ghost_bottom > 0) != (desc->row_offset + desc->height < Hg))
        return fail(FIBHIP_EINVAL, "ghost rows must exist exactly on the sides that have a neighbour");
    {   // the kernels index with 32-bit ints: rows * (floats between rows) of one array view must stay below 2^31
        const long long pitch = (desc->flags & FIBHIP_ROW_INTERLEAVED) ? (long long)nv * desc->width : desc->width;
        if ((long long)desc->height * pitch >= (1LL << 31))
            return fail(FIBHIP_EINVAL, "grid too large for 32-bit indexing: %d rows x %lld floats per row", desc->height, pitch);
    }
    if (!(desc->dt > 0.0)) return fail(FIBHIP_EINVAL, "dt must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FIBHIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
    if (desc->device < 0 || desc->device >= ndev) return fail(FIBHIP_EINVAL, "device %d out of range", desc->device);
    HIPCHK(hipSetDevice(desc->device));

    h = new (std::nothrow) fibhip_ctx();
    if (!h) return fail(FIBHIP_ENOMEM, "out of host memory");
    h->d = *desc;
    h->d.global_height = Hg;
    h->nvar = nv;
    h->mod = mod;
    h->spt = desc->steps_per_tick > 0 ? desc->steps_per_tick : (mod ? mod->spt : fibhip_default_steps_per_tick(desc->model));
    h->cells = (size_t)desc->height * desc->width;
    const bool interleaved = (desc->flags & FIBHIP_ROW_INTERLEAVED) != 0;
    h->pitch = interleaved ? nv * desc->width : desc->width;
    h->vstride = interleaved ? (size_t)desc->width : h->cells;
    h->own0 = desc->ghost_top;
    h->own1 = desc->height - desc->ghost_bottom;
    h->mode = 0;
    if (desc->model == FIBHIP_BR && (desc->flags & FIBHIP_CHEBY)) h->mode = BeelerReuter::MODE_CHEBY;
    if (desc->model == FIBHIP_COURT)
        h->mode = (desc->flags & FIBHIP_ALLVARS) ? Courtemanche::MODE_ALL : Courtemanche::MODE_FAST;
    if (desc->model == FIBHIP_COURT_US) h->mode = CourtemancheUS::MODE_ALL;
    const int ming = min_ghost(*desc);
    if ((desc->flags & FIBHIP_ZEROPAD) && desc->model != FIBHIP_FENTON4V)
        return fail(FIBHIP_EINVAL, "FIBHIP_ZEROPAD exists for the Fenton 4v model only (fenton_simple.py)");
    if ((desc->flags & FIBHIP_ZEROPAD) && (desc->ghost_top || desc->ghost_bottom))
        return fail(FIBHIP_EINVAL, "FIBHIP_ZEROPAD is a single-device option (no row blocks)");
    if ((desc->ghost_top || desc->ghost_bottom) && ming < h->spt)
        return fail(FIBHIP_EINVAL, "ghost width %d < steps_per_tick %d", ming, h->spt);
    h->cycle = (desc->ghost_top || desc->ghost_bottom) ? ming / h->spt : 1;
    h->cpos = 0;
    h->span = 1;

    // scalars: every Python-float product is formed in double and rounded once
    const double dt = desc->dt, diff = desc->diff;
    h->kf.dt = (float)dt;
    h->kf.ddt = (float)(diff * dt);
    h->kf.cvp = (float)(1.0 - dt / 3.33);          // tau_vp, tau_vn, tau_wp, tau_wn (fenton.py:60-63)
    h->kf.cvn = (float)(1.0 - dt / 19.2);
    h->kf.dvn = (float)(dt / 19.2);
    h->kf.cwp = (float)(1.0 - dt / 160.0);
    h->kf.cwn = (float)(1.0 - dt / 75.0);
    h->kf.dwn = (float)(dt / 75.0);
    h->kb.dt = (float)dt;
    h->kb.ddt = (float)(diff * dt);
    h->kb.mdt = (float)(-dt);
    h->kb.mdt_skip = (float)(-(dt * 5));
    h->kb.skip = (desc->flags & FIBHIP_HOLD) ? 2 : ((desc->flags & FIBHIP_SKIP) ? 1 : 0);
    memset(h->kb.cheb, 0, sizeof h->kb.cheb);
    {
        const bool all = (desc->flags & FIBHIP_ALLVARS) != 0 || desc->model == FIBHIP_COURT_US;
        const double dts = all ? dt : dt * 10;                     // court.py:118-122
        const double chronic = (desc->flags & FIBHIP_CHRONIC) ? 1.0 : 0.0;
        h->kc.dtf = (float)dt;
        h->kc.dts = (float)dts;
        h->kc.mdt_f = (float)(-dt);
        h->kc.mdt_s = (float)(-dts);
        h->kc.ddt = (float)(diff * dt);
        h->kc.em1_fCa = expm1f((float)(-dts / 2.0));               // tau_f_Ca = 2.0, court.py:160,189
        h->kc.em1_u = expm1f((float)(-dts / 8.0));                 // tau_u = 8.0,   court.py:161,243
        h->kc.chronic = (float)chronic;
        h->kc.c_to = (float)((1.0 - 0.5 * chronic) * 100 * 0.1652);   // court.py:193
        h->kc.c_Kur = (float)((1.0 - 0.5 * chronic) * 100);           // court.py:194
        h->kc.c_CaL = (float)((1.0 - 0.7 * chronic) * 100 * 0.12375); // court.py:218
    }
    h->has_consts = !(desc->model == FIBHIP_BR && (desc->flags & FIBHIP_CHEBY));

    if (desc->stream) {
        h->s0 = (hipStream_t)desc->stream;
        h->own_s0 = false;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&h->s0, hipStreamNonBlocking));
        h->own_s0 = true;
    }
    HIPCHK(hipStreamCreateWithFlags(&h->s1, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_int, hipEventDisableTiming));
    HIPCHK(hipEventCreate(&h->ev_t0));
    HIPCHK(hipEventCreate(&h->ev_t1));
    const size_t slab_bytes = (size_t)nv * h->cells * sizeof(float);
    if (desc->ext_slab[0] && desc->ext_slab[1]) {
        h->slab[0] = (float *)desc->ext_slab[0];
        h->slab[1] = (float *)desc->ext_slab[1];
        h->own_slab = false;
    } else {
        h->own_slab = true;                       // before the loop: a partial allocation is still ours to free
        for (int i = 0; i < 2; ++i) {
            if (hipMalloc((void **)&h->slab[i], slab_bytes) != hipSuccess) {
                h->slab[i] = nullptr;
                return fail(FIBHIP_ENOMEM, "hipMalloc of %zu bytes failed", slab_bytes);
            }
            HIPCHK(hipMemsetAsync(h->slab[i], 0, slab_bytes, h->s0));
        }
    }
    HIPCHK(hipMalloc((void **)&h->phase3, 6 * h->cells * sizeof(float)));
    HIPCHK(hipMalloc((void **)&h->phi_dev, h->cells * sizeof(float)));
    HIPCHK(hipHostMalloc((void **)&h->probe_host, 64, hipHostMallocDefault));
    // (`new fibhip_ctx()` has zeroed every field: what follows are the ones that do not start at zero)
    h->multi_max = 1;
    h->mt.stale = true;
    h->mt.cur = 1;
    h->series.trust = true;
    {
        const char *e = getenv("FIBHIP_MT_IDS");
        h->mt.ids = (e && atoi(e) >= 2 && atoi(e) <= 65535) ? (unsigned)atoi(e) : 65535u;
    }
    {
        const char *e = getenv("FIBHIP_STREAM_WRITE");             // 0: notice the end of the stream's work through hipStreamQuery, as before
        h->done.off = e && atoi(e) == 0;
    }
    {
        // Run-ahead starts the caller's NEXT ticks before it has asked for them.  A caller that owns the slabs
        // (desc->ext_slab: it can write them between two calls without the library knowing) never gets it; a caller that has
        // been handed a raw pointer (fibhip_state_ptr) loses it from then on — the same rule the aggregates follow.
        const char *e = getenv("FIBHIP_AHEAD");
        h->ahead.ok = !(e && atoi(e) == 0) && h->own_slab;
    }
    {
        const char *e = getenv("FIBHIP_MT_WAIT_MS");
        h->mt.wait_ms = (e && atol(e) > 0) ? (unsigned)(atol(e) > 0xFFFFFFl ? 0xFFFFFFl : atol(e)) : 0u;
        const char *f = getenv("FIBHIP_MT_FAKE_GIVEUP");
        h->journal.fake_giveup_at = (f && atol(f) > 0) ? atol(f) : 0;
    }
    HIPCHK(hipEventCreateWithFlags(&h->ahead.ev, hipEventDisableTiming));
    {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, desc->device));
        h->ncu = prop.multiProcessorCount;
        // FIBHIP_MT=0 switches multi-tick launches off, FIBHIP_MT_MAX bounds the ticks of one launch (both caps: launch_cap)
        const char *e = getenv("FIBHIP_MT"), *em = getenv("FIBHIP_MT_MAX");
        const int env_max = (em && atoi(em) > 0) ? imin(atoi(em), MT_MAX_TICKS_ENV) : 0;
        h->mt.max = (e && atoi(e) == 0) ? 1 : (env_max ? env_max : MT_MAX_TICKS);
        if (interleaved || desc->ghost_top || desc->ghost_bottom || (long long)h->cells * ((nv + 3) / 4 * 4) * 8 >= (1LL << 31))
            h->mt.max = 1;
        // a process-wide CU mask takes compute units away that multiProcessorCount still reports: the tiles of a grid
        // "that fits" would then not all be resident (a launch would give up after its bound and the handle fall back, §2d of
        // DESIGN.md — correct, but two seconds late): never start
        for (const char *var : {"HSA_CU_MASK", "ROC_GLOBAL_CU_MASK"}) {
            const char *m = getenv(var);
            if (m && *m) h->mt.max = 1;
        }
        h->mt.max_declared = h->mt.max <= 1 ? 1 : (env_max ? env_max : MT_MAX_TICKS_DECLARED);
    }
    h->agg_dirty = true;
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
    {
        // A caller-owned slab can be written behind the library's back — except on a row-block shard, whose contract
        // is that only the ghost rows change, and only in the exchange between step_edges and step_commit.
        const char *e = getenv("FIBHIP_COURT_AGG");
        const bool shard = desc->ghost_top || desc->ghost_bottom;
        if (desc->model == FIBHIP_COURT && (desc->flags & FIBHIP_FAST) && !(desc->flags & FIBHIP_ALLVARS) &&
            (h->own_slab || shard) && !(e && atoi(e) == 0)) {
            const bool il = h->pitch != desc->width;       // row-interleaved: the aggregates share the slab's row pitch
            const size_t floats = il ? (size_t)desc->height * h->pitch : (size_t)CourtAgg::NAGG * h->cells;
            HIPCHK(hipMalloc((void **)&h->agg, floats * sizeof(float)));
            h->agg_stride = il ? (size_t)desc->width : h->cells;
            h->use_agg = true;
        }
    }
#endif
    return build_plan(h);
}

extern "C" int fibhip_create(const fibhip_desc *desc, fibhip_t *out)
{
    if (!desc || !out) return fail(FIBHIP_EINVAL, "null argument");
    fibhip_ctx *h = nullptr;
    const int rc = create_impl(desc, h);
    if (rc) {
        if (h) fibhip_destroy(h);              // releases whatever had been acquired before the failure
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int fibhip_destroy(fibhip_t h)
{
    if (!h) return 0;
    fibhip_comm_free(h);
    hipSetDevice(h->d.device);
    if (h->ahead.n > 0 && h->mt.host_word)                 // a launch that ran ahead of the caller: nobody wants its ticks any more
        __atomic_store_n(h->mt.host_word, (h->ahead.id << 16) | MT_CANCEL, __ATOMIC_RELEASE);
    if (h->s0) hipStreamSynchronize(h->s0);
    if (h->s1) hipStreamSynchronize(h->s1);
    if (h->own_slab) {
        if (h->slab[0]) hipFree(h->slab[0]);
        if (h->slab[1]) hipFree(h->slab[1]);
    }
    if (h->phase3) hipFree(h->phase3);
    if (h->phi_dev) hipFree(h->phi_dev);
    if (h->agg) hipFree(h->agg);
    if (h->tensor) hipFree(h->tensor);
    if (h->obs.buf) hipFree(h->obs.buf);
    if (h->obs.vel) hipFree(h->obs.vel);
    recorders_free(h);
    if (h->mt.xbuf) hipFree(h->mt.xbuf);
    if (h->mt.epochs) hipFree(h->mt.epochs);
    for (auto &r : h->trace) {
        if (r.e0) hipEventDestroy(r.e0);
        if (r.e1) hipEventDestroy(r.e1);
    }
    mt_forget(h);
    if (h->mt.snap_flags) hipHostFree(h->mt.snap_flags);
    if (h->done.word) hipHostFree(h->done.word);
    if (h->probe_host) hipHostFree(h->probe_host);
    if (h->stage) hipHostFree(h->stage);
    if (h->ahead.ev) hipEventDestroy(h->ahead.ev);
    if (h->ev_main) hipEventDestroy(h->ev_main);
    if (h->ev_int) hipEventDestroy(h->ev_int);
    if (h->ev_t0) hipEventDestroy(h->ev_t0);
    if (h->ev_t1) hipEventDestroy(h->ev_t1);
    if (h->s1) hipStreamDestroy(h->s1);
    if (h->own_s0 && h->s0) hipStreamDestroy(h->s0);
    delete h;
    return 0;
}

// phase3 from the field that stands: phase_prep_kernel's planes, or — on a handle with a diffusion tensor — tensor_prep_kernel's,
// with the tensor's first-order coefficients where dpy and dpx stand, and its five weight planes (pointwise.inc)
static int prep_planes(fibhip_ctx *h)
{
    const Geo g = base_geo(h);
    float *p = h->phase3;
    const size_t n = h->cells;
    if (h->has_tensor) {
        TensorPlanes t;
        t.dyy = h->tensor; t.dxx = h->tensor + n; t.dxy = h->tensor + 2 * n;
        t.wy = h->tensor + 3 * n; t.wx = h->tensor + 4 * n; t.wa = h->tensor + 5 * n; t.wb = h->tensor + 6 * n; t.wc = h->tensor + 7 * n;
        hipLaunchKernelGGL(tensor_prep_kernel, dim3(1024), dim3(256), 0, h->s0, g, h->has_phase ? (const float *)h->phi_dev : (const float *)nullptr, t,
                           p, p + n, p + 2 * n, p + 3 * n, p + 4 * n, p + 5 * n);
    } else if (h->has_phase) {
        hipLaunchKernelGGL(phase_prep_kernel, dim3(1024), dim3(256), 0, h->s0, g, h->phi_dev, p, p + n, p + 2 * n, p + 3 * n, p + 4 * n, p + 5 * n);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int fibhip_set_phase(fibhip_t h, const float *phi)
{
    NEED(h);
    FLUSH(h);
    CONFIRM(h);
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "set_phase inside an open tick");
    h->phi_floored = false;
    if (!phi) {
        h->has_phase = false;
        if (h->has_tensor) {                      // the tensor's planes without a field: ϕ = 1
            if (int rc = prep_planes(h)) return rc;
            SYNC_S0(h);
        }
        return build_plan(h);
    }
    HIPCHK(hipMemcpyAsync(h->phi_dev, phi, h->cells * sizeof(float), hipMemcpyHostToDevice, h->s0));
    h->has_phase = true;
    if (int rc = prep_planes(h)) return rc;
    SYNC_S0(h);                                   // `phi` may be a temporary of the caller
    return build_plan(h);
}

// what a diffusion tensor must be, cell by cell (fib_tf_amd/tensor.py check_tensor raises the same, in the same words)
static int tensor_check(const float *dyy, const float *dxx, const float *dxy, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        const double a = dyy[i], b = dxx[i], c = dxy[i];
        if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c)) return fail(FIBHIP_EINVAL, "set_tensor: the tensor planes are not finite everywhere");
        if (!(a > 0.0 && b > 0.0 && a * b - c * c > 0.0)) return fail(FIBHIP_EINVAL, "set_tensor: the tensor is not positive definite everywhere");
        // (the entries are float32 roundings of a tensor whose largest eigenvalue is at most 1: 1e-6 is a dozen of their ulps)
        if (0.5 * (a + b) + std::sqrt(0.25 * (a - b) * (a - b) + c * c) > 1.0 + 1e-6)
            return fail(FIBHIP_EINVAL, "set_tensor: the largest eigenvalue is above 1: the tensor is relative to diff (raise diff instead)");
    }
    return 0;
}

extern "C" int fibhip_set_tensor(fibhip_t h, const float *dyy, const float *dxx, const float *dxy)
{
    NEED(h);
    const bool off = !dyy && !dxx && !dxy;
    if (!off && (!dyy || !dxx || !dxy)) return fail(FIBHIP_EINVAL, "set_tensor: three planes, or three null pointers to remove the tensor");
    if (!off) {
        // what reads the isotropic operator or recomputes the phase planes does not go with a tensor
        if (h->d.ghost_top || h->d.ghost_bottom) return fail(FIBHIP_EINVAL, "set_tensor: not on a row block: a diffusion tensor is a single-device option");
        if (h->d.flags & FIBHIP_ZEROPAD) return fail(FIBHIP_EINVAL, "set_tensor: not on a model with the zero-padded Laplacian (FIBHIP_ZEROPAD)");
        if (h->d.model == FIBHIP_CUSTOM) return fail(FIBHIP_EINVAL, "set_tensor: not on a traced model (FIBHIP_CUSTOM): its kernels know the isotropic Laplacian only");
        if (h->pitch != h->d.width) return fail(FIBHIP_EINVAL, "set_tensor: not on a row-interleaved slab");
        if (h->ld.on || h->pm.on || h->les.on)
            return fail(FIBHIP_EINVAL, "set_tensor: not while a lead recorder, a potential-map recorder or a lesion program is attached");
        if (int rc = tensor_check(dyy, dxx, dxy, h->cells)) return rc;
    }
    FLUSH(h);
    CONFIRM(h);
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "set_tensor inside an open tick");
    if (off) {
        if (!h->has_tensor) return 0;
        h->has_tensor = false;
        if (h->agg_held) {                        // Courtemanche, fast policy: back on the aggregates, formed afresh
            h->use_agg = true;
            h->agg_dirty = true;
            h->agg_held = false;
        }
        if (int rc = prep_planes(h)) return rc;   // the phase planes of the field that stands, if one does
        SYNC_S0(h);
        return build_plan(h);
    }
    const size_t B = h->cells * sizeof(float);
    if (!h->tensor && hipMalloc((void **)&h->tensor, 8 * B) != hipSuccess) {
        h->tensor = nullptr;
        return fail(FIBHIP_ENOMEM, "set_tensor: hipMalloc of %zu bytes failed", 8 * B);
    }
    HIPCHK(hipMemcpyAsync(h->tensor, dyy, B, hipMemcpyHostToDevice, h->s0));
    HIPCHK(hipMemcpyAsync(h->tensor + h->cells, dxx, B, hipMemcpyHostToDevice, h->s0));
    HIPCHK(hipMemcpyAsync(h->tensor + 2 * h->cells, dxy, B, hipMemcpyHostToDevice, h->s0));
    if (!h->has_tensor && h->use_agg) {           // a tensor handle runs Courtemanche's plain modes (launch.hpp g_tensor_variants)
        h->use_agg = false;
        h->agg_held = true;
    }
    h->has_tensor = true;
    if (int rc = prep_planes(h)) return rc;
    SYNC_S0(h);                                   // the planes may be temporaries of the caller
    return build_plan(h);
}

extern "C" int fibhip_set_state(fibhip_t h, int var, const float *src)
{
    NEED(h);
    FLUSH(h);
    CONFIRM(h);
    if (!src || var < -1 || var >= h->nvar) return fail(FIBHIP_EINVAL, "set_state: bad var %d", var);
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "set_state inside an open tick");
    const int v0 = var < 0 ? 0 : var, v1 = var < 0 ? h->nvar : var + 1;
    for (int v = v0; v < v1; ++v) {
        const float *s = src + (size_t)(v - v0) * h->cells;
        for (int b = 0; b < 2; ++b)               // both slabs, so either may become current
            HIPCHK(hipMemcpy2DAsync(h->slab[b] + (size_t)v * h->vstride, (size_t)h->pitch * sizeof(float), s,
                                    (size_t)h->d.width * sizeof(float), (size_t)h->d.width * sizeof(float),
                                    (size_t)h->d.height, hipMemcpyHostToDevice, h->s0));
    }
    SYNC_S0(h);
    // The whole slab restarts the exchange cycle: the caller supplied fresh ghost rows of every array.  ONE array
    // does not: mid-cycle the other arrays' outer ghost rows are stale, so the cycle position stays and the rows
    // of `var` that are still live at this position are the ones the caller's copy has to be right in.
    if (var < 0) h->cpos = 0;
    h->agg_dirty = true;
    return 0;
}

// Host memory for fibhip_get_state_direct destinations: page-locked, so the device writes it at PCIe rate.
extern "C" int fibhip_host_alloc(size_t nbytes, void **out)
{
    if (!out || nbytes == 0) return fail(FIBHIP_EINVAL, "host_alloc: bad argument");
    if (hipHostMalloc(out, nbytes, hipHostMallocDefault) != hipSuccess) {
        *out = nullptr;
        return fail(FIBHIP_ENOMEM, "hipHostMalloc of %zu bytes failed", nbytes);
    }
    return 0;
}

extern "C" int fibhip_host_free(void *p)
{
    if (p) HIPCHK(hipHostFree(p));
    return 0;
}

// get_state straight into the caller's buffer, which should come from fibhip_host_alloc: no staging copy (a pageable
// destination works too, at the ~1 GB/s of an unpinned device-to-host copy)
extern "C" int fibhip_get_state_direct(fibhip_t h, int var, float *dst)
{
    NEED(h);
    FLUSH(h);
    if (!dst || var < -1 || var >= h->nvar) return fail(FIBHIP_EINVAL, "get_state_direct: bad var %d", var);
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "get_state inside an open tick");
    // one array, and the caller's next series is known: the series is launched first and carries the frame (sched.inc)
    bool delivered = false;
    if (int rc = ahead_read_back(h, var, dst, &delivered)) return rc;
    if (delivered) return 0;
    const int v0 = var < 0 ? 0 : var, v1 = var < 0 ? h->nvar : var + 1;
    for (int pass = 0; pass < 2; ++pass) {
        const long long fb0 = h->journal.n_fallbacks;
        for (int v = v0; v < v1; ++v) {
            const float *src = h->slab[h->cur[v]] + (size_t)v * h->vstride;
            float *d = dst + (size_t)(v - v0) * h->cells;
            if (h->pitch == h->d.width)
                HIPCHK(hipMemcpyAsync(d, src, h->cells * sizeof(float), hipMemcpyDeviceToHost, h->s0));
            else
                HIPCHK(hipMemcpy2DAsync(d, (size_t)h->d.width * sizeof(float), src, (size_t)h->pitch * sizeof(float),
                                        (size_t)h->d.width * sizeof(float), (size_t)h->d.height, hipMemcpyDeviceToHost, h->s0));
        }
        SYNC_S0(h);
        if (h->journal.n_fallbacks == fb0) break;           // (else: a launch in front of the copy had given up — the state has been
    }                                               // restored and recomputed meanwhile, and the copy is taken again)
    return 0;
}

extern "C" int fibhip_get_state(fibhip_t h, int var, float *dst)
{
    NEED(h);
    FLUSH(h);
    if (!dst || var < -1 || var >= h->nvar) return fail(FIBHIP_EINVAL, "get_state: bad var %d", var);
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "get_state inside an open tick");
    const int v0 = var < 0 ? 0 : var, v1 = var < 0 ? h->nvar : var + 1;
    // through a pinned staging buffer: a D2H copy into pageable memory runs at ~1 GB/s, pinned at PCIe
    // rate; the reference driver reads the potential back 100 times per simulated second (fenton.py:184-185)
    if (!h->stage) HIPCHK(hipHostMalloc((void **)&h->stage, h->cells * sizeof(float), hipHostMallocDefault));
    for (int v = v0; v < v1; ++v) {
        for (int pass = 0; pass < 2; ++pass) {
            const long long fb0 = h->journal.n_fallbacks;
            HIPCHK(hipMemcpy2DAsync(h->stage, (size_t)h->d.width * sizeof(float),
                                    h->slab[h->cur[v]] + (size_t)v * h->vstride, (size_t)h->pitch * sizeof(float),
                                    (size_t)h->d.width * sizeof(float), (size_t)h->d.height, hipMemcpyDeviceToHost, h->s0));
            SYNC_S0(h);
            if (h->journal.n_fallbacks == fb0) break;       // (a launch in front of the copy had given up: recovered, copy again)
        }
        memcpy(dst + (size_t)(v - v0) * h->cells, h->stage, h->cells * sizeof(float));
    }
    return 0;
}

extern "C" int fibhip_set_consts(fibhip_t h, const float *tbl, int n)
{
    NEED(h);
    FLUSH(h);
    CONFIRM(h);
    if (h->d.model != FIBHIP_BR || !(h->d.flags & FIBHIP_CHEBY))
        return fail(FIBHIP_EINVAL, "set_consts: only the Beeler-Reuter Chebyshev path takes a table");
    if (!tbl || n != 12 * 9) return fail(FIBHIP_EINVAL, "set_consts: expected 108 coefficients, got %d", n);
    memcpy(h->kb.cheb, tbl, sizeof h->kb.cheb);
    h->has_consts = true;
    return 0;
}

#ifdef FIB_CUSTOM_MODEL_INC
template <class P, int M_>
static launch_fn custom_mode_fn(int mode)
{
    if constexpr (M_ >= Custom::NMODES) {
        return nullptr;
    } else {
        if (mode == M_) return launch_pointwise<Custom, P, M_>;
        return custom_mode_fn<P, M_ + 1>(mode);
    }
}
#endif

extern "C" int fibhip_step_mode(fibhip_t h, int mode)
{
    NEED(h);
    const bool fast = (h->d.flags & FIBHIP_FAST) != 0;
    (void)fast;
    if (h->mod) {
        FLUSH(h);
        CONFIRM(h);                                       // (the update is in place: it must not stand behind an unconfirmed launch)
        for (const Variant &v : h->mod->variants)
            if (v.kind == MK_POINTWISE && v.mode == mode && v.fast == (fast ? 1 : 0) && mode >= 1)
                return run_pointwise_mode(h, launch_module, &v);
        return fail(FIBHIP_EINVAL, "step_mode: the traced model has no mode %d", mode);
    }
#ifdef FIB_CUSTOM_MODEL_INC
    if (h->d.model == FIBHIP_CUSTOM) {
        FLUSH(h);
        CONFIRM(h);
        launch_fn fn = mode >= 1 ? (fast ? custom_mode_fn<Fast, 1>(mode) : custom_mode_fn<Exact, 1>(mode)) : nullptr;
        if (!fn) return fail(FIBHIP_EINVAL, "step_mode: the traced model has no mode %d", mode);
        return run_pointwise_mode(h, fn);
    }
#endif
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
    if (h->d.model == FIBHIP_COURT && mode == Courtemanche::MODE_SLOW) {
        if (h->d.flags & FIBHIP_ALLVARS) return fail(FIBHIP_EINVAL, "step_slow: handle was created with FIBHIP_ALLVARS");
        if (h->pending && h->fused_fn && !slow_sample_due(h)) {   // the last deferred tick + slow as one launch
            if (int rc = launch_pending(h, h->pending - 1)) return rc;
            h->pending = 0;
            const launch_fn plain = h->plan[0].fn;
            h->plan[0].fn = h->fused_fn;
            const int rc = tick_now(h);
            h->plan[0].fn = plain;
            return rc;
        }
        FLUSH(h);
        CONFIRM(h);
        if (h->use_agg) {                                 // 'slow' on the state as it stands; the aggregates follow it
            h->agg_dirty = false;
            return run_pointwise_mode(h, launch_pointwise<CourtAgg, Fast, CourtAgg::MODE_SLOW>);
        }
        return run_pointwise_mode(h, fast ? launch_pointwise<Courtemanche, Fast, Courtemanche::MODE_SLOW>
                                          : launch_pointwise<Courtemanche, Exact, Courtemanche::MODE_SLOW>);
    }
#endif
    return fail(FIBHIP_EINVAL, "step_mode: model %d has no mode %d", h->d.model, mode);
}

extern "C" int fibhip_step_slow(fibhip_t h)
{
    NEED(h);
    if (h->d.model != FIBHIP_COURT) return fail(FIBHIP_EINVAL, "step_slow: Courtemanche only");
    return fibhip_step_mode(h, Courtemanche::MODE_SLOW);
}

extern "C" int fibhip_pace(fibhip_t h, int r0, int r1, int c0, int c1, float v, float min_v)
{
    NEED(h);
    FLUSH(h);
    CONFIRM(h);
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "pace inside an open tick");
    const Geo g = base_geo(h);
    if (int rc = trace_open(h, h->s0, "pace_kernel", 1, 0, 0, 0, 1)) return rc;
    hipLaunchKernelGGL(pace_kernel, dim3(1024), dim3(256), 0, h->s0, g, h->slab[h->cur[0]], r0, r1, c0, c1, v, min_v);   // variable 0 starts at the slab base in both layouts
    HIPCHK(hipGetLastError());
    if (int rc = trace_close(h, h->s0)) return rc;
    h->launches++;
    return 0;
}

extern "C" int fibhip_probe(fibhip_t h, int var, int row, int col, float *out)
{
    NEED(h);
    FLUSH(h);
    if (!out || var < 0 || var >= h->nvar || row < 0 || row >= h->d.height || col < 0 || col >= h->d.width)
        return fail(FIBHIP_EINVAL, "probe: out of range");
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "probe inside an open tick");
    for (int pass = 0; pass < 2; ++pass) {
        const long long fb0 = h->journal.n_fallbacks;
        HIPCHK(hipMemcpyAsync(h->probe_host, h->slab[h->cur[var]] + (size_t)var * h->vstride + (size_t)row * h->pitch + col,
                              sizeof(float), hipMemcpyDeviceToHost, h->s0));
        SYNC_S0(h);
        if (h->journal.n_fallbacks == fb0) break;           // (a launch in front of the copy had given up: recovered, copy again)
    }
    *out = *h->probe_host;
    return 0;
}

extern "C" int fibhip_sync(fibhip_t h)
{
    NEED(h);
    FLUSH(h);
    HIPCHK(wait_stream(h->s1));
    SYNC_S0(h);
    return 0;
}

extern "C" int fibhip_time_steps(fibhip_t h, int nticks, float *elapsed_ms, int *launches)
{
    NEED(h);
    FLUSH(h);
    const long l0 = h->launches;
    HIPCHK(hipEventRecord(h->ev_t0, h->s0));
    if (int rc = fibhip_step(h, nticks)) return rc;
    FLUSH(h);                                             // the timed region ends after the LAST tick's launch
    HIPCHK(hipEventRecord(h->ev_t1, h->s0));
    SYNC_S0(h);
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
    if (elapsed_ms) *elapsed_ms = ms;
    if (launches) *launches = (int)(h->launches - l0);
    return 0;
}

// HIP-event bracket on the handle's stream around whatever the caller enqueues in between (ticks, 'slow' ops,
// pacing): bench.py times the reference driver's real tick mix with it.
extern "C" int fibhip_time_begin(fibhip_t h)
{
    NEED(h);
    FLUSH(h);
    h->t_launches0 = h->launches;
    HIPCHK(hipEventRecord(h->ev_t0, h->s0));
    return 0;
}

extern "C" int fibhip_time_end(fibhip_t h, float *elapsed_ms, int *launches)
{
    NEED(h);
    FLUSH(h);
    HIPCHK(hipEventRecord(h->ev_t1, h->s0));
    SYNC_S0(h);
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
    if (elapsed_ms) *elapsed_ms = ms;
    if (launches) *launches = (int)(h->launches - h->t_launches0);
    return 0;
}

// ------------------------------------------------------------------------------------------
// run-time modules: the device code of ONE traced model, compiled in-process by the caller (hiprtc), loaded here and
// launched through the module API by the same host logic that drives the built-in models
// ------------------------------------------------------------------------------------------
extern "C" int fibhip_module_load(int device, const void *code, size_t nbytes, const fibhip_module_desc *d, fibhip_module_t *out)
{
    if (!code || !nbytes || !d || !out) return fail(FIBHIP_EINVAL, "module_load: null argument");
    if (d->struct_size != (int)sizeof(fibhip_module_desc))
        return fail(FIBHIP_EINVAL, "fibhip_module_desc size mismatch: caller %d, library %d", d->struct_size, (int)sizeof(fibhip_module_desc));
    if (d->nvar < 1 || d->nvar > FIB_MAXVAR || d->nmodes < 1 || d->nmodes > 8 || d->steps_per_tick < 1 || d->consts_bytes < 0 ||
        d->consts_bytes > 64 || d->nkernels < 1 || !d->kernels)
        return fail(FIBHIP_EINVAL, "module_load: inconsistent description");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FIBHIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(FIBHIP_EINVAL, "device %d out of range", device);
    HIPCHK(hipSetDevice(device));
    fibhip_module *m = new (std::nothrow) fibhip_module();
    if (!m) return fail(FIBHIP_ENOMEM, "out of host memory");
    m->device = device;
    m->nvar = d->nvar; m->spt = d->steps_per_tick; m->nmodes = d->nmodes; m->consts_bytes = d->consts_bytes;
    for (int i = 0; i < 8; ++i) m->masks[i] = d->masks[i];
    m->K = d->K; m->TX = d->TX; m->TY = d->TY; m->R = d->R; m->TYB = d->TYB;
    m->K2 = d->K2; m->TX2 = d->TX2; m->TY2 = d->TY2; m->R2 = d->R2;
    if (hipModuleLoadData(&m->mod, code) != hipSuccess) {
        delete m;
        return fail(FIBHIP_EHIP, "module_load: hipModuleLoadData refused the code object");
    }
    for (int i = 0; i < d->nkernels; ++i) {
        const fibhip_module_kernel &k = d->kernels[i];
        Variant v;
        v.model = FIBHIP_CUSTOM; v.mode = k.mode; v.fast = k.fast; v.phase = k.phase;
        v.K = k.K; v.TX = k.TX; v.TY = k.TY; v.NT = k.NT;
        v.fn = launch_module;
        v.kind = k.kind;
        if (k.kind == MK_STRIP_MT) {                    // the multi-tick form of a strip kernel listed before it
            Variant *base = nullptr;
            for (Variant &b : m->variants)
                if (b.kind == MK_STRIP && b.mode == k.mode && b.fast == k.fast && b.phase == k.phase && b.K == k.K && b.TX == k.TX &&
                    b.TY == k.TY && b.NT == k.NT)
                    base = &b;
            if (!base || !k.symbol || hipModuleGetFunction(&base->kern_mt, m->mod, k.symbol) != hipSuccess) {
                hipModuleUnload(m->mod);
                delete m;
                return fail(FIBHIP_EINVAL, "module_load: kernel %d (%s): no strip kernel of that shape before it, or missing from the code object", i,
                            k.symbol ? k.symbol : "(null)");
            }
            base->fn_mt = launch_module;
            continue;
        }
        const bool ok_shape = k.kind == MK_POINTWISE ||
                              (k.kind == MK_TICK && k.NT >= 64 && k.NT <= 1024 && k.K >= 1 && k.TX >= 1 && k.TY >= 1) ||
                              (k.kind == MK_STRIP && k.NT < 0 && k.NT > -32 && k.K >= 2 && k.TX + 2 * (k.K - 1) <= 62 &&
                               (k.TY + 2 * (k.K - 1) + (-k.NT) - 1) / (-k.NT) <= 16);
        if (!k.symbol || !ok_shape || hipModuleGetFunction(&v.kern, m->mod, k.symbol) != hipSuccess) {
            hipModuleUnload(m->mod);
            delete m;
            return fail(FIBHIP_EINVAL, "module_load: kernel %d (%s) is missing from the code object or has an impossible shape", i,
                        k.symbol ? k.symbol : "(null)");
        }
        m->variants.push_back(v);
    }
    *out = m;
    return 0;
}

extern "C" int fibhip_module_unload(fibhip_module_t m)
{
    if (!m) return 0;
    hipSetDevice(m->device);
    if (m->mod) hipModuleUnload(m->mod);
    delete m;
    return 0;
}

extern "C" int fibhip_state_ptr(fibhip_t h, int var, void **dev_ptr)
{
    if (!h || !dev_ptr || var < 0 || var >= h->nvar) return fail(FIBHIP_EINVAL, "state_ptr: bad argument");
    FLUSH(h);
    // the pointer names the CURRENT slab: a launch that gave up is recovered first (recovery moves the state back to the other
    // slab), and what the caller writes through the pointer must not be what a later recovery returns to or replays over
    CONFIRM(h);
    // the caller may write the state through this pointer at any time, between any two calls: nothing may run ahead of it
    // any more (a launch started before the caller asked for its ticks would read the state before such a write, or race it)
    h->ahead.ok = false;
    if (h->use_agg && !h->d.ghost_top && !h->d.ghost_bottom) {   // the caller may write through the pointer at any time: back to
                                                                 // the plain kernels (a shard's ghost rows: see create_impl)
        h->use_agg = false;
        if (int rc = build_plan(h)) return rc;
    }
    *dev_ptr = h->slab[h->cur[var]] + (size_t)var * h->vstride;
    return h->cur[var];
}

extern "C" int fibhip_next_ptr(fibhip_t h, int var, void **dev_ptr)
{
    if (!h || !dev_ptr || var < 0 || var >= h->nvar) return fail(FIBHIP_EINVAL, "next_ptr: bad argument");
    if (h->phase_of_tick == 0) return fail(FIBHIP_EINVAL, "next_ptr: no tick in flight");
    *dev_ptr = h->slab[h->nxt[var]] + (size_t)var * h->vstride;
    return h->nxt[var];
}

extern "C" int fibhip_halo_vars(fibhip_t h)
{
    if (!h) return fail(FIBHIP_EINVAL, "null handle");
    return (h->spt > 1 || h->cycle > 1) ? h->nvar : 1;
}

extern "C" int fibhip_halo_due(fibhip_t h)
{
    if (!h) return fail(FIBHIP_EINVAL, "null handle");
    // (ticks fibhip_step has accepted but not launched yet count: the NEXT tick is the one asked about)
    return ((h->d.ghost_top || h->d.ghost_bottom) && (h->cpos + h->pending) % h->cycle == h->cycle - 1) ? 1 : 0;
}

extern "C" int fibhip_plan_tile(fibhip_t h, int *tile_w, int *tile_h, int *rows_per_wave)
{
    if (!h) return fail(FIBHIP_EINVAL, "null handle");
    if (h->plan.empty()) return fail(FIBHIP_EINVAL, "no plan");
    const PlanItem &it = (h->multi_max > 1 && !h->plan_multi[h->multi_max].empty()) ? h->plan_multi[h->multi_max][0] : h->plan[0];
    // (the exchange-period row, where the multi-tick launches run one: the tile the handle's ticks are computed in)
    const Variant *pv = mt_variant(h, true);
    if (!(pv && pv->period)) pv = nullptr;
    if (tile_w) *tile_w = pv ? pv->TX : it.TX;
    if (tile_h) *tile_h = pv ? pv->TY : it.TY;
    if (rows_per_wave) *rows_per_wave = pv ? -pv->NT : (it.v ? -it.v->NT : 0);
    return 0;
}

extern "C" int fibhip_variant_count(void) { return g_nvariants; }

extern "C" int fibhip_variant_info(int i, int out[10])
{
    if (i < 0 || i >= g_nvariants || !out) return fail(FIBHIP_EINVAL, "variant_info: bad argument");
    const Variant &v = g_variants[i];
    out[0] = v.model; out[1] = v.mode; out[2] = v.fast; out[3] = v.phase;
    out[4] = v.K; out[5] = v.TX; out[6] = v.TY; out[7] = v.NT;
    // (the rows of g_variants carry their kind in how they list NT — see V4 / S4 / W4 — Variant::kind is a module's)
    out[8] = v.NT > 0 ? MK_TICK : (v.NT > -32 ? MK_STRIP : MK_ROWS);
    // (1: a multi-tick launch that exchanges once per tick, K = the tick's sub-steps; an exchange-period row is listed as the
    // plain strip launch of K sub-steps it also is)
    out[9] = v.fn_mt && !v.period ? 1 : 0;
    return 0;
}

// the second table: the kernels of handles with a diffusion tensor (launch.hpp g_tensor_variants), the same ten fields
extern "C" int fibhip_tensor_variant_count(void) { return g_ntensor_variants; }

extern "C" int fibhip_tensor_variant_info(int i, int out[10])
{
    if (i < 0 || i >= g_ntensor_variants || !out) return fail(FIBHIP_EINVAL, "tensor_variant_info: bad argument");
    const Variant &v = g_tensor_variants[i];
    out[0] = v.model; out[1] = v.mode; out[2] = v.fast; out[3] = v.phase;
    out[4] = v.K; out[5] = v.TX; out[6] = v.TY; out[7] = v.NT;
    out[8] = MK_TICK;
    out[9] = 0;
    return 0;
}

extern "C" int fibhip_ticks_per_launch(fibhip_t h)
{
    if (!h) return fail(FIBHIP_EINVAL, "null handle");
    if (mt_variant(h)) return launch_cap(h, h->series.expect > 0);      // (a declared series is running: its cap)
    return multi_cap(h);
}

extern "C" int fibhip_trace_begin(fibhip_t h)
{
    NEED(h);
    FLUSH(h);
    CONFIRM(h);                                           // every traced tick is a plain launch: none behind an unconfirmed one
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "trace_begin inside an open tick");
    for (auto &r : h->trace) {
        if (r.e0) hipEventDestroy(r.e0);
        if (r.e1) hipEventDestroy(r.e1);
    }
    h->trace.clear();
    h->tracing = true;
    return 0;
}

extern "C" int fibhip_trace_end(fibhip_t h, fibhip_trace_event *out, int max_events)
{
    NEED(h);
    if (!h->tracing) return fail(FIBHIP_EINVAL, "trace_end without trace_begin");
    if (!out || max_events < 1) return fail(FIBHIP_EINVAL, "trace_end: bad argument");
    FLUSH(h);
    h->tracing = false;
    HIPCHK(wait_stream(h->s1));
    SYNC_S0(h);
    int n = 0;
    for (const auto &r : h->trace) {
        if (n >= max_events) {                        // (like snprintf: the return value says how many there were)
            n = (int)h->trace.size();
            break;
        }
        float t0 = 0.f, dur = 0.f;
        HIPCHK(hipEventElapsedTime(&t0, h->trace[0].e0, r.e0));
        HIPCHK(hipEventElapsedTime(&dur, r.e0, r.e1));
        fibhip_trace_event &e = out[n++];
        memcpy(e.name, r.name, sizeof e.name);
        e.start_us = t0 * 1e3;
        e.dur_us = dur * 1e3;
        e.K = r.K; e.tile_w = r.TX; e.tile_h = r.TY; e.rows_per_wave = r.R; e.ticks = r.ticks;
    }
    return n;
}

extern "C" int fibhip_launch_stats(fibhip_t h, long long out[4])
{
    if (!h || !out) return fail(FIBHIP_EINVAL, "launch_stats: null argument");
    out[0] = h->launches;
    out[1] = h->n_ticks;
    out[2] = h->mt.n_launches;
    out[3] = h->mt.n_ticks;
    return 0;
}

extern "C" int fibhip_spec_stats(fibhip_t h, long long out[2])
{
    if (!h || !out) return fail(FIBHIP_EINVAL, "spec_stats: null argument");
    out[0] = h->ahead.n_kept;
    out[1] = h->ahead.n_redone;
    return 0;
}

extern "C" int fibhip_fallbacks(fibhip_t h, long long out[2])
{
    if (!h || !out) return fail(FIBHIP_EINVAL, "fallbacks: null argument");
    out[0] = h->journal.n_fallbacks;
    out[1] = h->journal.n_replayed;
    return 0;
}

extern "C" int fibhip_set_mt_wait_ms(fibhip_t h, int ms)
{
    if (!h || ms < 0 || ms > 0xFFFFFF) return fail(FIBHIP_EINVAL, "set_mt_wait_ms: 0 (the default, 2000) .. 16777215");
    h->mt.wait_ms = (unsigned)ms;
    return 0;
}

extern "C" int fibhip_launch_plan(fibhip_t h, int *fused_steps, int *launches_per_tick)
{
    if (!h) return fail(FIBHIP_EINVAL, "null handle");
    if (!h->tuned && h->phase_of_tick == 0 && !h->pending && check_ready(h) == 0) {   // report the plan that will run
        HIPCHK(hipSetDevice(h->d.device));
        if (int rc = autotune(h)) return rc;
    }
    if (fused_steps) *fused_steps = h->plan.empty() ? 0 : h->plan[0].K;
    if (launches_per_tick) *launches_per_tick = (int)h->plan.size();
    // multi-tick launches in exchange periods: (sub-steps of a period, 1) — fibhip_ticks_per_launch still counts ticks
    if (const Variant *pv = mt_variant(h, true))
        if (pv->period) {
            if (fused_steps) *fused_steps = pv->K;
            if (launches_per_tick) *launches_per_tick = 1;
        }
    return 0;
}

#include "unit.inc"
