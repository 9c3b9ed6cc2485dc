// launch.hpp — how one launch reaches a kernel of kernels.hpp: the launch context, the launchers, and the table of
// kernel variants the plans are chosen from.
#pragma once

// ------------------------------------------------------------------------------------------
// kernel variants
// ------------------------------------------------------------------------------------------
constexpr int FIB_MAXVAR = 26;   // CourtAgg: 21 state arrays + 5 aggregates (CourtemancheUS: 22)

struct LaunchCtx {
    Geo g;
    const float *in[FIB_MAXVAR];
    float *out[FIB_MAXVAR];
    PhaseTab ph;
    const void *consts;
    int sub0;
    // a kernel of a code object loaded at run time (fibhip_module_load) instead of one linked into this library
    hipFunction_t kern;
    int kind, K, TX, TY, NT, nvar, consts_bytes;
    MtArgs mt;                      // MK_STRIP_MT only: the ticks of this launch and what its tiles exchange through
};

typedef hipError_t (*launch_fn)(hipStream_t, const LaunchCtx &);

// kernel kinds: 0 .. 3 are also the `kind` of a run-time module's kernels (include/fibhip.h); rows_kernel is built in only
enum { MK_TICK = 0, MK_STRIP = 1, MK_POINTWISE = 2, MK_STRIP_MT = 3, MK_ROWS = 4 };

// tiles of TX x TY over the rows [r0, r1) and, with `bands`, over the second band [rb0, rb1) behind them: fills the tile
// fields of `g` and returns the grid size (xcd_tile() needs a multiple of 8).  A multi-tick launch has one band: the
// whole, unsharded grid.
static inline int tile_grid(Geo &g, int TX, int TY, bool bands)
{
    g.tiles_x = (g.W + TX - 1) / TX;
    g.ty_a = (g.r1 > g.r0) ? (g.r1 - g.r0 + TY - 1) / TY : 0;
    const int ty_b = (bands && g.rb1 > g.rb0) ? (g.rb1 - g.rb0 + TY - 1) / TY : 0;
    g.ntiles = g.tiles_x * (g.ty_a + ty_b);
    return ((g.ntiles + 7) / 8) * 8;
}

// threads of a workgroup: N of them for a flat tile (tick_kernel); for the strip kernels one wave per N rows of the
// tile grown by the rim of the K - 1 sub-steps still to come
constexpr int threads_of(int kind, int K, int TY, int N)
{
    return kind == MK_TICK ? N : 64 * ((TY + 2 * (K - 1) + N - 1) / N);
}

template <class M>
static inline PtrTab<M::NVAR> ptr_tab(const LaunchCtx &c)
{
    PtrTab<M::NVAR> pt;
    for (int v = 0; v < M::NVAR; ++v) {
        pt.in[v] = c.in[v];
        pt.out[v] = c.out[v];
    }
    return pt;
}

// One launcher for the four tile kernels; N = threads (MK_TICK) or rows per wave.  MK_STRIP_MT advances c.mt.nticks ticks
// in one launch: the caller has checked that all tiles can be resident.
template <int KIND, class M, class P, int MODE, int K, int TX, int TY, int N, bool PHASE>
static hipError_t launch_tiles(hipStream_t st, const LaunchCtx &c)
{
    Geo g = c.g;
    const int grid = tile_grid(g, TX, TY, KIND != MK_STRIP_MT);
    if (g.ntiles <= 0) return hipSuccess;
    const PtrTab<M::NVAR> pt = ptr_tab<M>(c);
    const typename M::Consts &k = *static_cast<const typename M::Consts *>(c.consts);
    constexpr int NT = threads_of(KIND, K, TY, N);
    if constexpr (KIND == MK_TICK)
        hipLaunchKernelGGL((tick_kernel<M, P, MODE, K, TX, TY, N, PHASE>), dim3(grid), dim3(NT), 0, st, g, pt, c.ph, k, c.sub0);
    else if constexpr (KIND == MK_STRIP)
        hipLaunchKernelGGL((strip_kernel<M, P, MODE, K, TX, TY, N, PHASE>), dim3(grid), dim3(NT), 0, st, g, pt, c.ph, k, c.sub0);
    else if constexpr (KIND == MK_ROWS)
        hipLaunchKernelGGL((rows_kernel<M, P, MODE, K, TX, TY, N, PHASE>), dim3(grid), dim3(NT), 0, st, g, pt, c.ph, k, c.sub0);
    else
        hipLaunchKernelGGL((strip_mt_kernel<M, P, MODE, K, TX, TY, N, PHASE>), dim3(grid), dim3(NT), 0, st, g, pt, c.ph, k, c.sub0, c.mt);
    return hipGetLastError();
}

template <class M, class P, int MODE>
static hipError_t launch_pointwise(hipStream_t st, const LaunchCtx &c)
{
    const PtrTab<M::NVAR> pt = ptr_tab<M>(c);
    const long n = (long)(c.g.r1 - c.g.r0) * c.g.W;
    if (n <= 0) return hipSuccess;
    const int grid = (int)((n + 255) / 256);
    hipLaunchKernelGGL((pointwise_kernel<M, P, MODE>), dim3(grid), dim3(256), 0, st, c.g, pt,
                       *static_cast<const typename M::Consts *>(c.consts));
    return hipGetLastError();
}

// One launcher for every kernel of a run-time module (a traced model compiled in-process by hiprtc): the same grids
// as launch_tiles / launch_pointwise, the kernel arguments laid out by hand as the compiler lays out
// (Geo, PtrTab<NVAR>, PhaseTab, Consts, int) — every argument at its natural alignment, in order.
static hipError_t launch_module(hipStream_t st, const LaunchCtx &c)
{
    Geo g = c.g;
    int threads, grid;
    if (c.kind == MK_POINTWISE) {
        const long n = (long)(g.r1 - g.r0) * g.W;
        if (n <= 0) return hipSuccess;
        threads = 256;
        grid = (int)((n + 255) / 256);
    } else {
        grid = tile_grid(g, c.TX, c.TY, c.kind != MK_STRIP_MT);
        if (g.ntiles <= 0) return hipSuccess;
        threads = threads_of(c.kind, c.K, c.TY, c.kind == MK_TICK ? c.NT : -c.NT);
    }
    alignas(8) char buf[sizeof(Geo) + 8 + 2 * FIB_MAXVAR * sizeof(void *) + sizeof(PhaseTab) + 64 + 16 + sizeof(MtArgs) + 8];
    size_t off = 0;
    auto put = [&](const void *p, size_t n, size_t align) {
        off = (off + align - 1) & ~(align - 1);
        memcpy(buf + off, p, n);
        off += n;
    };
    put(&g, sizeof g, alignof(Geo));
    off = (off + 7) & ~(size_t)7;                                   // PtrTab<NVAR>: in[NVAR] then out[NVAR]
    memcpy(buf + off, c.in, (size_t)c.nvar * sizeof(void *));
    off += (size_t)c.nvar * sizeof(void *);
    memcpy(buf + off, c.out, (size_t)c.nvar * sizeof(void *));
    off += (size_t)c.nvar * sizeof(void *);
    if (c.kind != MK_POINTWISE) put(&c.ph, sizeof c.ph, alignof(PhaseTab));
    const char zeros[64] = {0};
    if (c.consts_bytes > 0) put(c.consts ? c.consts : zeros, (size_t)c.consts_bytes, 4);
    if (c.kind != MK_POINTWISE) put(&c.sub0, sizeof c.sub0, alignof(int));
    if (c.kind == MK_STRIP_MT) put(&c.mt, sizeof c.mt, alignof(MtArgs));      // strip_mt_kernel's last argument
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, buf, HIP_LAUNCH_PARAM_BUFFER_SIZE, &off, HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(c.kern, grid, 1, 1, threads, 1, 1, 0, st, nullptr, config);
}

constexpr int VM_FENTON_ZP = 100;   // variant-table id of FentonZP (not a fibhip_model: selected by FIBHIP_ZEROPAD)
constexpr int VM_COURT_AGG = 101;   // variant-table id of CourtAgg (Courtemanche, fast policy: fibhip_ctx::use_agg)

struct Variant {
    int model, mode, fast, phase;
    int K, TX, TY, NT;
    launch_fn fn;
    hipFunction_t kern = nullptr;   // run-time module kernels only (fn == launch_module)
    int kind = 0;
    launch_fn fn_mt = nullptr;      // the same shape advancing several ticks per launch (strip_mt_kernel), or null
    hipFunction_t kern_mt = nullptr;        // ... of a run-time module (fn_mt == launch_module, kind MK_STRIP_MT)
    int period = 0;                 // 1: fn_mt exchanges every K sub-steps with K below the tick's sub-steps (an exchange-period row:
                                    // strip_kernel.inc PERIODS); fn, the plain launch of K sub-steps, is the rows' own check
};

// One row of the table: launcher kind L of one policy and phase — and, with MT = 1, the same shape advancing several ticks per
// launch.  N = threads of a flat tile or rows per wave of a strip; CODE = how the table lists it (Variant::NT).
#define VROW_MT_0(MODEL, P, MODE, K, TX, TY, N, PH) nullptr
#define VROW_MT_1(MODEL, P, MODE, K, TX, TY, N, PH) launch_tiles<MK_STRIP_MT, MODEL, P, MODE, K, TX, TY, N, PH>
#define VROW_MT_2(MODEL, P, MODE, K, TX, TY, N, PH) launch_tiles<MK_STRIP_MT, MODEL, P, MODE, K, TX, TY, N, PH>, nullptr, 1
#define VROW(L, MT, P, FAST, PH, MODEL, MID, MODE, K, TX, TY, N, CODE)                                                 \
    {MID, MODE, FAST, PH, K, TX, TY, CODE, launch_tiles<L, MODEL, P, MODE, K, TX, TY, N, PH>, nullptr, 0,              \
     VROW_MT_##MT(MODEL, P, MODE, K, TX, TY, N, PH)}
#define VFAST(L, MT, ...) VROW(L, MT, Fast, 1, false, __VA_ARGS__), VROW(L, MT, Fast, 1, true, __VA_ARGS__)
#define VBOTH(L, MT, ...) VROW(L, MT, Exact, 0, false, __VA_ARGS__), VROW(L, MT, Exact, 0, true, __VA_ARGS__), VFAST(L, MT, __VA_ARGS__)

#define V4(MODEL, MID, MODE, K, TX, TY, NT) VBOTH(MK_TICK, 0, MODEL, MID, MODE, K, TX, TY, NT, NT)
// fast-policy-only models (CourtAgg)
#define F2(MODEL, MID, MODE, K, TX, TY, NT) VFAST(MK_TICK, 0, MODEL, MID, MODE, K, TX, TY, NT, NT)
#define FS2(MODEL, MID, MODE, K, TX, TY, R) VFAST(MK_STRIP, 0, MODEL, MID, MODE, K, TX, TY, R, -(R))
// strip kernels are listed with NT = -R (rows per wave)
#define S4(MODEL, MID, MODE, K, TX, TY, R) VBOTH(MK_STRIP, 0, MODEL, MID, MODE, K, TX, TY, R, -(R))
// strip kernels that also exist as multi-tick launches (K = the model's sub-steps per tick)
#define S4M(MODEL, MID, MODE, K, TX, TY, R) VBOTH(MK_STRIP, 1, MODEL, MID, MODE, K, TX, TY, R, -(R))
// strip kernels whose multi-tick launch exchanges every K sub-steps, K below the tick's sub-steps (models with UNIFORM_SUBSTEPS):
// the period decides the rim depth K - 1, the tile width 64 - 2K and how the box's strips land on the four SIMDs
#define S4P(MODEL, MID, MODE, K, TX, TY, R) VBOTH(MK_STRIP, 2, MODEL, MID, MODE, K, TX, TY, R, -(R))
// rows kernels (potential in registers, DPP taps) are listed with NT = -(32 + R)
#define W4(MODEL, MID, MODE, K, TX, TY, R) VBOTH(MK_ROWS, 0, MODEL, MID, MODE, K, TX, TY, R, -(32 + (R)))

// The first matching entry with the wanted K is the default; FIBHIP_VARIANT="K,TX,TY,NT" overrides
// (tuning sweeps).  Tile shapes: K=1 tiles are wide (coalesced 256-B rows); K>1 tiles are square-ish
// to keep the redundant rim small.
static const Variant g_variants[] = {
#ifdef FIB_CUSTOM_MODEL_INC
    // ---- the traced model this copy of the library was built for (constants from the generated header) ----
    V4(Custom, FIBHIP_CUSTOM, 0, 1, 64, 4, 256),
#if FIB_CUSTOM_K > 1
    S4(Custom, FIBHIP_CUSTOM, 0, FIB_CUSTOM_K, FIB_CUSTOM_TX, FIB_CUSTOM_TY, FIB_CUSTOM_R),
#if FIB_CUSTOM_TYB > 0
    S4(Custom, FIBHIP_CUSTOM, 0, FIB_CUSTOM_K, FIB_CUSTOM_TX, FIB_CUSTOM_TYB, FIB_CUSTOM_R),
#endif
#endif
#if FIB_CUSTOM_K2 > 1 && FIB_CUSTOM_K2 != FIB_CUSTOM_K
    S4(Custom, FIBHIP_CUSTOM, 0, FIB_CUSTOM_K2, FIB_CUSTOM_TX2, FIB_CUSTOM_TY2, FIB_CUSTOM_R2),
#endif
#endif
#ifndef FIB_CUSTOM_ONLY
#ifndef FIB_ONLY_BR
    // ---- Fenton 4v ----
    // K = 10 (the whole tick in one launch) and K = 5 strips of growing tile height: build_plan picks the shape
    // that gives every CU at most one tile (or the fewest rounds) for the grid at hand
    S4M(Fenton, FIBHIP_FENTON4V, 0, 10, 44, 25, 3),
    S4M(Fenton, FIBHIP_FENTON4V, 0, 10, 44, 28, 3),
    S4M(Fenton, FIBHIP_FENTON4V, 0, 10, 44, 27, 3),
    S4M(Fenton, FIBHIP_FENTON4V, 0, 10, 44, 30, 3),
    S4M(Fenton, FIBHIP_FENTON4V, 0, 10, 44, 32, 4),
    S4M(Fenton, FIBHIP_FENTON4V, 0, 10, 44, 36, 4),
    S4M(Fenton, FIBHIP_FENTON4V, 0, 10, 44, 40, 4),
    S4M(Fenton, FIBHIP_FENTON4V, 0, 10, 44, 44, 4),
    // an exchange period of 6 sub-steps (512^2: 250 tiles of 16 two-row strips; tools/dbg/period_model.py): a candidate of
    // autotune beside the rows above, never the rule-based plan.  (Measured at 512^2 and not kept, profiles/exchange_period_ab.txt:
    // K = 8 in 48 x 23, 3 rows per wave — 11.68 against 11.40 us per tick, and two spilled registers with a phase field; K = 7
    // in 50 x 23, 3 rows per wave, three waves per SIMD — 12.87.  And profiles/lean_prefix_ab.txt: K = 6 in 52 x 22, sixteen full
    // strips, 240 tiles, 30 per XCD — 11.28 / 11.44 against 11.13 / 11.13 for 52 x 21 in the same build: the busiest SIMD has
    // the same 43 row-steps per period, and every tile is on a compute unit of its own either way.)
    S4P(Fenton, FIBHIP_FENTON4V, 0, 6, 52, 21, 2),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 21, 3),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 23, 3),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 22, 4),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 27, 3),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 25, 3),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 28, 3),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 31, 3),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 34, 3),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 32, 4),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 40, 3),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 44, 4),
    S4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 56, 4),
    S4(Fenton, FIBHIP_FENTON4V, 0, 2, 60, 18, 4),
    // the same blocking with the potential in registers and DPP taps (rows_kernel): selectable, not a default
    W4(Fenton, FIBHIP_FENTON4V, 0, 10, 44, 25, 3),
    W4(Fenton, FIBHIP_FENTON4V, 0, 5, 54, 21, 3),
    V4(Fenton, FIBHIP_FENTON4V, 0, 10, 32, 32, 512),
    V4(Fenton, FIBHIP_FENTON4V, 0, 10, 32, 32, 1024),
    V4(Fenton, FIBHIP_FENTON4V, 0, 10, 32, 32, 256),
    V4(Fenton, FIBHIP_FENTON4V, 0, 5, 32, 32, 256),
    V4(Fenton, FIBHIP_FENTON4V, 0, 5, 32, 32, 512),
    V4(Fenton, FIBHIP_FENTON4V, 0, 5, 32, 16, 256),
    V4(Fenton, FIBHIP_FENTON4V, 0, 2, 64, 16, 256),
    V4(Fenton, FIBHIP_FENTON4V, 0, 2, 32, 32, 256),
    V4(Fenton, FIBHIP_FENTON4V, 0, 1, 64, 4, 256),
    V4(Fenton, FIBHIP_FENTON4V, 0, 1, 64, 16, 256),
    // ---- Fenton 4v with the zero-padded convolution Laplacian (FIBHIP_ZEROPAD), flat kernels only ----
    V4(FentonZP, VM_FENTON_ZP, 0, 10, 32, 32, 1024),
    V4(FentonZP, VM_FENTON_ZP, 0, 5, 32, 32, 512),
    V4(FentonZP, VM_FENTON_ZP, 0, 2, 64, 16, 256),
    V4(FentonZP, VM_FENTON_ZP, 0, 1, 64, 4, 256),
#endif
    // ---- Beeler-Reuter (mode 0 direct gates, 1 Chebyshev) ----
    S4M(BeelerReuter, FIBHIP_BR, 0, 5, 54, 21, 2),
    S4M(BeelerReuter, FIBHIP_BR, 0, 5, 54, 24, 2),
    S4M(BeelerReuter, FIBHIP_BR, 0, 5, 54, 27, 3),
    S4M(BeelerReuter, FIBHIP_BR, 0, 5, 54, 28, 3),
    S4M(BeelerReuter, FIBHIP_BR, 0, 5, 54, 16, 2),
    S4M(BeelerReuter, FIBHIP_BR, 0, 5, 54, 40, 3),
    V4(BeelerReuter, FIBHIP_BR, 0, 1, 64, 4, 256),
#ifndef FIB_ONLY_BR                     // tuning alternatives (tools/sweep.py); a specialised build keeps the two defaults
    S4(BeelerReuter, FIBHIP_BR, 0, 5, 54, 21, 3),
    S4(BeelerReuter, FIBHIP_BR, 0, 3, 58, 19, 2),
    S4(BeelerReuter, FIBHIP_BR, 0, 2, 60, 19, 2),
    S4(BeelerReuter, FIBHIP_BR, 0, 2, 60, 19, 3),
    V4(BeelerReuter, FIBHIP_BR, 0, 5, 32, 32, 256),
    V4(BeelerReuter, FIBHIP_BR, 0, 5, 32, 32, 512),
    V4(BeelerReuter, FIBHIP_BR, 0, 1, 64, 16, 256),
#endif
    S4M(BeelerReuter, FIBHIP_BR, 1, 5, 54, 21, 2),
    S4M(BeelerReuter, FIBHIP_BR, 1, 5, 54, 24, 2),
    S4M(BeelerReuter, FIBHIP_BR, 1, 5, 54, 27, 3),
    S4M(BeelerReuter, FIBHIP_BR, 1, 5, 54, 28, 3),
    S4M(BeelerReuter, FIBHIP_BR, 1, 5, 54, 16, 2),
    S4M(BeelerReuter, FIBHIP_BR, 1, 5, 54, 40, 3),
    V4(BeelerReuter, FIBHIP_BR, 1, 1, 64, 4, 256),
#ifndef FIB_ONLY_BR                     // tuning alternatives (tools/sweep.py); a specialised build keeps the two defaults
    S4(BeelerReuter, FIBHIP_BR, 1, 5, 54, 21, 3),
    S4(BeelerReuter, FIBHIP_BR, 1, 3, 58, 19, 2),
    S4(BeelerReuter, FIBHIP_BR, 1, 2, 60, 19, 2),
    S4(BeelerReuter, FIBHIP_BR, 1, 2, 60, 19, 3),
    V4(BeelerReuter, FIBHIP_BR, 1, 5, 32, 32, 256),
    V4(BeelerReuter, FIBHIP_BR, 1, 5, 32, 32, 512),
    V4(BeelerReuter, FIBHIP_BR, 1, 1, 64, 16, 256),
#endif
#ifndef FIB_ONLY_BR
    // ---- Courtemanche (mode 0 fast set, 2 all variables) ----
    V4(Courtemanche, FIBHIP_COURT, Courtemanche::MODE_FAST, 1, 64, 4, 256),
    V4(Courtemanche, FIBHIP_COURT, Courtemanche::MODE_FAST, 1, 64, 8, 256),
    V4(Courtemanche, FIBHIP_COURT, Courtemanche::MODE_ALL, 1, 64, 4, 256),
    V4(Courtemanche, FIBHIP_COURT, Courtemanche::MODE_FASTSLOW, 1, 64, 4, 256),
    // the fast tick on the five per-cell aggregates of the slow variables (models.hpp CourtAgg)
    F2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 1, 64, 4, 256),
    F2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 1, 64, 8, 256),
    F2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FASTSLOW, 1, 64, 4, 256),
    // two and three consecutive fast ticks in one launch (fibhip_step defers ticks: see tick_multi); first entry of
    // each K = default, the others for tools/sweep.py (FIBHIP_COURT_MULTI2 / FIBHIP_COURT_MULTI3 = "TX,TY,NT")
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 20, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 14, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 16, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 18, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 22, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 24, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 25, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 28, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 26, 3),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 58, 12, 1),
    F2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 3, 32, 32, 256),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 2, 60, 14, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 2, 60, 12, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 2, 60, 16, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 2, 60, 18, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 2, 60, 22, 2),
    FS2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 2, 60, 30, 2),
    F2(CourtAgg, VM_COURT_AGG, CourtAgg::MODE_FAST, 2, 64, 16, 256),
    // ---- court_ultra.py with the ultra-slow `_us_` gate: 22 variables, single rate ----
    V4(CourtemancheUS, FIBHIP_COURT_US, CourtemancheUS::MODE_ALL, 1, 64, 4, 256),
#endif
#endif
};
static const int g_nvariants = (int)(sizeof g_variants / sizeof g_variants[0]);

// The kernels of a handle with per-cell diffusion tensors (fibhip_set_tensor; models.hpp Tensor<M>): a table of its own, so that
// g_variants and what fibhip_variant_count / _info enumerate stay what they are.  Flat tiles only — the tensor Laplacian exists in
// tick_kernel alone, as FentonZP's does — and PHASE = true only: a tensor always has a first-order term, which rides on the phase
// planes (pointwise.inc tensor_prep_cell; ϕ = 1 where the model has no field).  No aggregates: Courtemanche runs its plain modes.
// Listed under the model's own id; the first row of a K is the default, FIBHIP_VARIANT / FIBHIP_K choose among them.
#define T2(MODEL, MID, MODE, K, TX, TY, NT)                                                                            \
    VROW(MK_TICK, 0, Exact, 0, true, Tensor<MODEL>, MID, MODE, K, TX, TY, NT, NT), VROW(MK_TICK, 0, Fast, 1, true, Tensor<MODEL>, MID, MODE, K, TX, TY, NT, NT)
static const Variant g_tensor_variants[] = {
#ifndef FIB_CUSTOM_ONLY
#ifndef FIB_ONLY_BR
    T2(Fenton, FIBHIP_FENTON4V, 0, 10, 32, 32, 1024),
    T2(Fenton, FIBHIP_FENTON4V, 0, 5, 32, 32, 512),
    T2(Fenton, FIBHIP_FENTON4V, 0, 2, 64, 16, 256),
    T2(Fenton, FIBHIP_FENTON4V, 0, 1, 64, 4, 256),
#endif
    T2(BeelerReuter, FIBHIP_BR, 0, 5, 32, 32, 512),
    T2(BeelerReuter, FIBHIP_BR, 0, 1, 64, 4, 256),
    T2(BeelerReuter, FIBHIP_BR, 1, 5, 32, 32, 512),
    T2(BeelerReuter, FIBHIP_BR, 1, 1, 64, 4, 256),
#ifndef FIB_ONLY_BR
    T2(Courtemanche, FIBHIP_COURT, Courtemanche::MODE_FAST, 1, 64, 4, 256),
    T2(Courtemanche, FIBHIP_COURT, Courtemanche::MODE_ALL, 1, 64, 4, 256),
    T2(Courtemanche, FIBHIP_COURT, Courtemanche::MODE_FASTSLOW, 1, 64, 4, 256),
    T2(CourtemancheUS, FIBHIP_COURT_US, CourtemancheUS::MODE_ALL, 1, 64, 4, 256),
#endif
#endif
    {-1, 0, 0, 0, 0, 0, 0, 0, nullptr},             // (ends the table: a build for one traced model has no row)
};
static const int g_ntensor_variants = (int)(sizeof g_tensor_variants / sizeof g_tensor_variants[0]) - 1;
