// strip_kernel.inc — the strip kernels: strip_kernel (K sub-steps of one tick per launch) and strip_mt_kernel (several ticks per
// launch, strip_mt.hpp), one body.  (included by kernels.hpp)

#ifdef FIB_STAMPS   // diagnostic build only (tools/ubench/stamp_strip.hip): per-wave s_memtime stamps
__device__ unsigned long long fib_stamps[4096 * 16];
#define FIB_STAMP(slot)                                                                          \
    do {                                                                                         \
        if ((threadIdx.x & 63) == 0 && (slot) < 16)                                              \
            fib_stamps[(blockIdx.x * 16 + (threadIdx.x >> 6)) % 4096 * 16 + (slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// (tools/ubench/stamp_mt.hip: the phases of a tick boundary inside a multi-tick launch; the last boundary's values stay)
__device__ unsigned long long fib_bstamps[4096 * 16];
#define FIB_BSTAMP(slot)                                                                         \
    do {                                                                                         \
        if ((threadIdx.x & 63) == 0)                                                             \
            fib_bstamps[(blockIdx.x * 16 + (threadIdx.x >> 6)) % 4096 * 16 + (slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#define FIB_BSTAMP_WAIT() __builtin_amdgcn_s_waitcnt(0x0070)      /* vmcnt(0) lgkmcnt(0): the phase's loads have landed */
// (round 4: when a wave ARRIVES at the barrier of a sub-step — arithmetic done, new potential written — against FIB_STAMP's
// "barrier passed and next window read": what a sub-step spends computing and what it spends waiting)
__device__ unsigned long long fib_wstamps[4096 * 16];
#define FIB_WSTAMP(slot)                                                                         \
    do {                                                                                         \
        if ((threadIdx.x & 63) == 0 && (slot) < 16)                                              \
            fib_wstamps[(blockIdx.x * 16 + (threadIdx.x >> 6)) % 4096 * 16 + (slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define FIB_WSTAMP(slot) do { } while (0)
#define FIB_STAMP(slot) do { } while (0)
#define FIB_BSTAMP(slot) do { } while (0)
#define FIB_BSTAMP_WAIT() do { } while (0)
#endif

// M::pinned(k), or M::pinned_spare(k) where a model offers it and the kernel asks for it (one register less)
template <class M, class = void>
struct HasPinnedSpare {
    static constexpr bool value = false;
};
template <class M>
struct HasPinnedSpare<M, void_of<decltype(&M::pinned_spare)>> {
    static constexpr bool value = true;
};
template <class A, class B>
struct SameType {
    static constexpr bool value = false;
};
template <class A>
struct SameType<A, A> {
    static constexpr bool value = true;
};
// M::UNIFORM_SUBSTEPS where a model declares it (models.hpp Fenton): its sub-steps are all the same operation
template <class M, class = void>
struct UniformSubsteps {
    static constexpr int steps = 0;
};
template <class M>
struct UniformSubsteps<M, void_of<decltype(M::UNIFORM_SUBSTEPS)>> {
    static constexpr int steps = M::UNIFORM_SUBSTEPS ? M::DEFAULT_STEPS : 0;
};
template <class M, bool SPARE, class C>
static FIB_DEV decltype(auto) pinned_for(const C &k)
{
    if constexpr (SPARE && HasPinnedSpare<M>::value)
        return M::pinned_spare(k);
    else
        return M::pinned(k);
}

// strip_kernel<M,P,MODE,K,TX,TY,R,PHASE> — the K > 1 workhorse.
//   Same temporal blocking as tick_kernel, different work layout: the LDS tile is exactly 64 words
//   wide (compute box CX = TX + 2(K-1) <= 62 plus the two ring columns), lane l of every wave owns
//   column l, and wave w owns the R consecutive rows [wR, wR+R) of the compute box.  Consequences:
//     * every LDS access of a wave is 64 consecutive words: conflict-free, and a thread reads the
//       3 x (R+2) window of its R cells once per sub-step (3(R+2)/R instead of 9 reads per cell);
//     * rows are wave-uniform, so the rows that have gone stale (one more ring per sub-step) are
//       skipped with scalar branches — the box shrinks in y as the sub-steps proceed;
//     * the vertical border/ghost refresh is wave-uniform too; only the two edge columns need a
//       per-lane predicate.
//
// The multi-tick kernels sit at their register limits (Fenton: 128 vector registers, and scalar registers spilled into vector
// lanes): an edit ANYWHERE in them — one `& 0xFF` in the prologue — re-draws the register allocation and moves the kernel by 2-3 %
// (round 4, profiles/r04_ab_kernel_variants.txt: round 3's text 12.28 us per tick, the same with the give-up word set by
// compare-and-swap 12.60, by a plain store 12.29, the wait bound as a shift 12.60 or 12.24 depending on what else is in, ...).
// The forms in the tree are the combination that lost nothing against round 3's kernel for Fenton (12.32 / 12.28) and is the
// fastest measured for the other two (rounding-faithful Fenton 18.8 against 21.5, Beeler-Reuter 15.36 against 15.75).  Measure
// any edit here against the kernel it replaces on one box (tools/ubench/mt_ab.hip, br_mt_ab.hip).
// That holds for edits that compute the same thing, too.  (tried: the Laplacian of the strip's rows, the live-row mask and "publish
// the live rows and the REFLECT copies" — each written two or three times below — as forced-inline lambdas inside strip_body that
// capture by reference: the code of 276 kernels of the stock build changes, strip_kernel's as well as strip_mt_kernel's, .text
// 11 707 872 -> 11 696 864 bytes; with the units of the tick boundary and the read-back as such lambdas on top, 11 726 816.  A
// forced-inline free function for the Laplacian alone: 11 706 592.  None of them measured on a device, so the blocks stay as they are.)
//
// strip_kernel<M,P,MODE,K,TX,TY,R,PHASE> / strip_mt_kernel<...> share this body (MT = several ticks per launch)
template <class M, class P, int MODE, int K, int TX, int TY, int R, bool PHASE, bool MT>
static FIB_DEV void strip_body(const Geo &g, const PtrTab<M::NVAR> &pt, const PhaseTab &ph, const typename M::Consts &k, int sub0,
                               const MtArgs &mt)
{
    constexpr int NV = M::NVAR;
    constexpr int CX = TX + 2 * (K - 1), CY = TY + 2 * (K - 1);
    static_assert(CX <= 62 && K > 1, "strip_kernel: compute box must fit 62 lanes");
    static_assert(!MT || (CX == 62 && TX >= K && TY >= K), "multi-tick launches: 62-column box, the rim inside the eight neighbours");
    // Exchange periods.  A model whose sub-steps are all alike (M::UNIFORM_SUBSTEPS) has nothing in its arithmetic that knows
    // where a tick ends, so a multi-tick launch of it may hand its rims over every K sub-steps with K SMALLER than the tick: a
    // shallower rim (K - 1), a wider tile (TX = 64 - 2K) and a lower box, which decides how many strips land on each of the four
    // SIMDs.  Such an instantiation loops over PERIODS where the others loop over ticks: `mt.ticks_id` counts periods, every period
    // runs K sub-steps except the last, which runs the `sub0` sub-steps that complete the launch's ticks (the step functions
    // ignore the index sub0 stands for elsewhere), and everything between two periods — parities, epochs, the host's word, the
    // read-back — is the tick boundary below, word for word.  All of it sits behind `if constexpr (PERIODS)`: the instantiations
    // with K = the tick's sub-steps compile to the instructions they compiled to before.
    constexpr bool PERIODS = MT && K < UniformSubsteps<M>::steps;
    constexpr int NW = (CY + R - 1) / R;
    constexpr int LP = 64, LQ = NW * R + 2, NL = LP * LQ;
    constexpr unsigned WMASK = M::mask(MODE);
    // The LDS image of the potential.  Strips of an ODD number of rows: row-major, one dword per cell, the 3 x (R+2) window read
    // as ds_read_b32.  Strips of an EVEN number of rows (round 4): rows 2k and 2k+1 of a column form one aligned 8-byte word —
    // element (row, col) at dword (row >> 1) * 128 + 2 col + (row & 1) — and the window, which then starts on an even row and has an
    // even number of rows, is read as 3 x (R+2)/2 ds_read_b64.  The LDS array serves a wave's ds_read_b64 in the two cycles it takes
    // for a ds_read_b32 (MI355X_MICROARCH.md, LDS: 256 against 128 B/clk), and the window reload of ALL waves at once, right behind
    // a sub-step's barrier, is LDS-bandwidth time on everybody's critical path (stamped build, profiles/r04_stamps_substeps.txt:
    // the LAST wave to reach the barrier still waits 450-560 cycles for its window — 15 waves x 15 dwords x 2 cycles).
    // Beeler-Reuter's two-row strips: 15.4 -> 15.1 us per tick.  Three-row strips would need two copies of the tile program (a
    // window starts on an even row in every other wave only): built and measured — the registers it costs the Fenton kernel, which
    // sits at its 128, outweigh the LDS cycles (12.3 -> 13.0 us per tick; four-row strips with the paired image: 13.8).
    // (only where ONE workgroup has the compute unit to itself: with several resident, as on grids beyond 704^2, another workgroup
    // computes while this one reloads its windows, and the opaque addresses of the separate ds_read_b64 only cost — Beeler-Reuter
    // 2048^2 with the paired image in strip_kernel: 180.9 -> 184.5 us per tick)
    constexpr bool PAIR = MT && (R % 2 == 0);
    constexpr int SPARE = PAIR ? R + 6 : R + 4;
    __shared__ __attribute__((aligned(16))) float lds[2][NL + SPARE * 64];   // (+ spare rows: see `wi`)
    __shared__ int mt_abort;
    __shared__ float snapl[MT ? NW * R * 64 : 1];                    // multi-tick launches: the frame's values, parked for one tick

    const int tile = xcd_tile(blockIdx.x, g.ntiles);
    if (tile >= g.ntiles) return;
    FIB_STAMP(0);
    if (MT && threadIdx.x == 0) mt_abort = 0;                       // (read after the first tick's barriers)
    auto &&kk = pinned_for<M, (MT && SameType<P, Exact>::value)>(k);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int by = tile / g.tiles_x, bx = tile - by * g.tiles_x;
    int y0, rend;
    tile_rows(g, by, TY, y0, rend);
    const int x0 = bx * TX;
    const int cx0 = x0 - (K - 1), cy0 = y0 - (K - 1);
    const int gx = cx0 - 1 + lane;                                  // this lane's global column
    const int c0 = wave * R;                                        // first box row of this wave's strip

    // ---- the three tap columns of this lane, through the boundary clamp ------------------------------------
    // enforce_boundary + REFLECT: a tap at column c reads the raw potential of column clamp(c, 1, W-2).  The clamp
    // is a property of the LANE, so it lives in the tap ADDRESSES (computed once here) and the tile only ever holds
    // raw values at their own positions: border and ghost columns need no copies after a sub-step, and a tile at
    // the left or right edge of the domain costs what an interior tile costs.
    const int bW = clampi(gx - 1, 1, g.W - 2), bC = clampi(gx, 1, g.W - 2), bE = clampi(gx + 1, 1, g.W - 2);
    const int jW = clampi(bW - (cx0 - 1), 0, 63), jC = clampi(bC - (cx0 - 1), 0, 63), jE = clampi(bE - (cx0 - 1), 0, 63);
    auto brow = [&](int grow) {                                     // global row -> local row through the boundary clamp
        return clampi(clampi(grow, 1, g.Hg - 2) - g.row_off, 0, g.H - 1);
    };

    // ---- prologue: all global loads are issued before anything waits; the first sub-step's 3 x (R+2) window comes
    // straight from global memory (no tile fill, no barrier before the step loop)
    const float *vin = pt.in[0];
    float win[R + 2][3];
#pragma unroll
    for (int q = 0; q < R + 2; ++q) {
        const float *row = vin + (size_t)brow(cy0 + c0 - 1 + q + g.row_off) * g.pitch;
        win[q][0] = row[bW];
        win[q][1] = row[bC];
        win[q][2] = row[bE];
    }
    const bool lane_in = lane >= 1 && lane <= CX && gx >= 0 && gx < g.W;
    const bool col_border = gx == 0 || gx == g.W - 1;
    const bool store_col = lane_in && gx >= x0 && gx < x0 + TX;
    const bool wr = lane_in && !col_border;                         // this lane's cells are somebody's taps
    float s[R][NV];
    PhaseCoef<P> pc[R];
    int off[R];
    bool own[R];                                                    // the cells this thread stores: the tile proper
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int gy = cy0 + c0 + r;
        const int oy = clampi(gy, 0, g.H - 1), ox = clampi(gx, 0, g.W - 1);
        off[r] = oy * g.pitch + ox;
        own[r] = store_col && gy >= y0 && gy < min(y0 + TY, rend) && gy < g.H;
#pragma unroll
        for (int v = 0; v < NV; ++v) s[r][v] = pt.in[v][off[r]];
        if (PHASE) pc[r].load(ph, oy * g.W + ox);                   // (the phase arrays are always planar)
    }
    // read-back inside the launch: this tile's cells of one array of the state the launch STARTS from go straight into
    // page-locked host memory, by system-scope (write-through) stores: plain stores stay in the L2 — frames came back with
    // cells of the previous read-back — and the L2 write-back of a system-scope release fence in every tile at the same
    // moment cost 15 us per launch.  The values are taken here; the stores are issued at the start of the SECOND tick and the
    // tile's word is raised at the boundary after it: issued here they had to drain at the first boundary together with the
    // tile's exchange stores, and a 1 MiB frame of PCIe writes kept every tile waiting ~10 us there.  (Launches of two ticks
    // have one boundary: stores here, word there.  Tried: the frame in three parts over three ticks, values re-read from the
    // slab — no faster, and the extra registers cost 2.7 %.)
    // (parked in LDS meanwhile: in registers they pushed the kernel to its 128-register budget and into scratch)
    const int snap_at = (MT && mt.snap) ? ((int)(mt.ticks_id & 0xFFFFu) >= 3 ? 1 : 0) : -1;
    if constexpr (MT) {
        if (mt.snap) {                                              // (wave-uniform)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float x = s[r][0];
#pragma unroll
                for (int v = 1; v < NV; ++v) x = (mt.snap_var & 0xFF) == v ? s[r][v] : x;
                snapl[(c0 + r) * 64 + lane] = x;                    // (read back by the same thread: no barrier needed)
            }
        }
    }
    // rows of the compute box that can still be correct at sub-step st: [lo0+st.., hi0-st..) unless
    // the box reaches the domain edge on that side (no staleness enters through a real boundary)
    const bool top_open = cy0 + g.row_off > 0, bot_open = cy0 + CY + g.row_off < g.Hg;
    // window addresses of this strip (paired image: of the 8-byte word that holds its first two rows)
    const int aW = PAIR ? (c0 >> 1) * 128 + 2 * jW : c0 * LP + jW, aC = PAIR ? (c0 >> 1) * 128 + 2 * jC : c0 * LP + jC,
              aE = PAIR ? (c0 >> 1) * 128 + 2 * jE : c0 * LP + jE;
    // dword offset of the row k rows below a strip's first row (tile row c0 + 1: always odd in the paired image), from that row's
    // address as `cell_at` gives it (paired image: the address of the row's 8-byte word)
    auto ro = [](int k) constexpr { return PAIR ? ((1 + k) >> 1) * 128 + ((1 + k) & 1) : k * LP; };
    auto cell_at = [](int row, int col) { return PAIR ? (row >> 1) * 128 + 2 * col : row * LP + col; };
    constexpr int SPARE_ROW = PAIR ? LQ + 3 : LQ + 2;                    // a strip's worth of rows nobody reads, behind the tile
    auto window = [&](const float *Bq, float (&w)[R + 2][3]) {          // the strip's 3 x (R+2) window out of the image Bq
        if constexpr (PAIR) {
            typedef float v2f __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int m = 0; m < (R + 2) / 2; ++m) {
                // (the second and later words of a column from addresses the compiler cannot relate to the first: it would fuse
                // two reads into one ds_read2st64_b64, which the LDS serves in 8 cycles where two ds_read_b64 take 4)
                int oW = aW + m * 128, oC = aC + m * 128, oE = aE + m * 128;
                if (m > 0) asm volatile("" : "+v"(oW));
                const v2f a = *reinterpret_cast<const v2f *>(Bq + oW);
                if (m > 0) asm volatile("" : "+v"(oC));
                const v2f b = *reinterpret_cast<const v2f *>(Bq + oC);
                if (m > 0) asm volatile("" : "+v"(oE));
                const v2f c = *reinterpret_cast<const v2f *>(Bq + oE);
                w[2 * m][0] = a.x; w[2 * m + 1][0] = a.y;
                w[2 * m][1] = b.x; w[2 * m + 1][1] = b.y;
                w[2 * m][2] = c.x; w[2 * m + 1][2] = c.y;
            }
        } else {
#pragma unroll
            for (int q = 0; q < R + 2; ++q) {
                w[q][0] = Bq[aW + q * LP];
                w[q][1] = Bq[aC + q * LP];
                w[q][2] = Bq[aE + q * LP];
            }
        }
    };
    // ---- everything about the strip's rows that does not change from sub-step to sub-step, as wave-uniform scalars
    // (the step loop then spends its scalar instructions on two min/max and a few bit tests)
    const int g0 = cy0 + c0 + g.row_off;                            // global row of the strip's first row
    // rows that may ever be computed: inside the grid and inside this slab
    const int ra_fix = max(max(0, -g0), -(cy0 + c0));
    const int rb_fix = min(min(R, CY - c0), min(g.Hg - g.row_off, g.H) - (cy0 + c0));
    unsigned pub = 0;                                               // rows whose value other cells tap (not a border row)
    int top_r = -1, bot_r = -1;                                     // the strip row that is the grid's row 1 / H-2, if any
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (g0 + r != 0 && g0 + r != g.Hg - 1) pub |= 1u << r;
        if (g0 + r == 1) top_r = r;
        if (g0 + r == g.Hg - 2) bot_r = r;
    }
    // lanes whose cells nobody taps write to spare rows behind the tile instead of being masked out (row offsets
    // -2 .. R+1 are applied to this address)
    const int wi = wr ? cell_at(c0 + 1, lane) : cell_at(SPARE_ROW, lane);
    FIB_STAMP(1);
    // all prologue loads are consumed by the first sub-step anyway: drain them once here, so that the
    // compiler does not carry per-use `s_waitcnt vmcnt(n)` into every iteration of the step loop
    __builtin_amdgcn_s_waitcnt(0x0F70);                             // vmcnt(0) only
    FIB_STAMP(2);

    // two sub-steps per loop body: the loop-carried state then needs no register moves at the back edge (measured:
    // -5 % under Exact, -7 % for R = 4 strips, nothing for Fast R = 3; DESIGN.md 6, round 2)
    constexpr int STEP_UNROLL = 2;
    // A strip that stays whole for all K sub-steps — no row of it goes stale inside the tick, none is a border or a
    // ghost-source row of the grid (more than half of a tile's strips, and the ones that carry its own cells) — runs the
    // step loop without any of the row bookkeeping: ~35 scalar instructions and a dozen branches fewer per sub-step.
    // Only in the multi-tick kernel: the second copy of the step loop costs ~30 registers, which a grid with several
    // workgroups per compute unit pays with its occupancy (measured with the specialisation in every strip kernel: 512x512
    // multi-tick 12.53 -> 11.93 us per tick, but 4096x4096 388 -> 627 us and 1024x1024 35.0 -> 38.3); multi-tick grids have
    // at most one workgroup per compute unit by construction.
    // (and only where the registers are there and the bookkeeping is a visible share of the sub-step: four-row strips spilled
    // with the second loop — at 16 waves per workgroup the budget is 128 registers — and Beeler-Reuter's eight arrays with ~270
    // instructions per cell ran 1.5-3 % slower with it; both keep one loop)
    constexpr int WHOLE_NVR = 12;                                   // state registers per lane (NV x R) up to which it pays
    constexpr bool WHOLE_LOOP = MT && NV * R <= WHOLE_NVR;
    const bool whole = WHOLE_LOOP && ra_fix == 0 && rb_fix == R && (!top_open || c0 >= K - 1) && (!bot_open || c0 + R <= CY - (K - 1)) &&
                       pub == (1u << R) - 1u && top_r < 0 && bot_r < 0;
    // A whole PREFIX for the strips of the rim (exchange-period kernels with two-row strips: K = 6, 52 x 21 — strips 1, 2, 13 and
    // 14 of its 16 are fully live for the first 3, 5, 4 and 2 of a period's 6 sub-steps, and two of them sit on the busiest
    // SIMD): `n_whole` is the number of leading sub-steps of a full period during which the strip is what `whole` asks for
    // (`whole` is n_whole == K), and the loop with the row bookkeeping runs those sub-steps as the lean loop does — no live-row
    // range, no masks, every row published.  A short last period takes the bookkeeping throughout.
    // The prefix ends on an EVEN sub-step, at the top of a pass of the loop unrolled by two: a strip that changes from lean to
    // bookkeeping between the two sub-steps of one pass (prefixes of 3 and 5) cost more than the lean sub-step saves — 512 x 512,
    // µs per tick by HIP events, fast / rounding-faithful: no prefix 11.04 / 15.65, prefixes 3, 5, 4, 2: 11.14 / 15.41, prefixes
    // 2, 4, 4, 2: 10.84 / 15.15 (profiles/lean_prefix_ab.txt).
    // (only where the registers are there: the K = 6 kernels sit at 103-107 of 128 with it)
    constexpr bool LEAN_PREFIX = WHOLE_LOOP && PERIODS && NV * R <= 8;
    [[maybe_unused]] int n_whole = 0;
    if constexpr (LEAN_PREFIX) {
        if (ra_fix == 0 && rb_fix == R && pub == (1u << R) - 1u && top_r < 0 && bot_r < 0)
            n_whole = min(top_open ? min(K, c0 + 1) : K, bot_open ? CY - R - c0 + 1 : K);
        if (n_whole < K) n_whole &= ~1;
    }
    // (the tick loop aligned to 32-256 bytes in the instruction stream: 12.55 +- 0.03 us per tick for every alignment;
    // profiles/r04_ab_kernel_variants.txt)
#pragma unroll 1
    for (int tick = 0;; ++tick) {
    // the host's word is read over PCIe by ONE thread of the grid at the START of a tick and looked at at the tick's end: the
    // round trip hides behind the sub-steps, at the price of seeing the word a tick late (see the tick boundary below).
    // Issued HERE — nothing is outstanding at this point (the counter of outstanding loads is in order: in front of the rim
    // loads of a boundary the PCIe round trip would hold their wait back) — and defined and used inside one pass of the tick
    // loop: carried around the loop's back edge, the compiler waited for the load right where it was issued.
    unsigned hw = 0u;
    if constexpr (MT) {
        if (tile == 0 && threadIdx.x == 0) {
            typedef const __attribute__((address_space(1))) unsigned *gptr;     // (global, not flat: a flat load also counts
            gptr p = (gptr)(mt.snap_flag + MT_HOST_WORD_AT);                                        // as an LDS operation, which every barrier waits for)
            asm volatile("" : "+s"(p));                             // (a new address for the compiler in every tick: it had moved
            hw = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // the load in front of the tick loop)
        }
    }
    if constexpr (MT) {
        if (tick == snap_at) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (own[r]) __hip_atomic_store(mt.snap + off[r], snapl[(c0 + r) * 64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // write-through
        }
    }
    // a launch's last period is short where the launch's sub-steps are no multiple of K: it runs `sub0` of them (wave-uniform;
    // once per launch, so it takes the loop with the row bookkeeping whatever the strip).  (A flag, and the bound read from the
    // kernel's argument where it is needed: a bound kept live across the period cost the 48 x 23 kernel a third spilled register.)
    [[maybe_unused]] bool short_last = false;
    if constexpr (PERIODS) short_last = tick + 1 >= (int)(mt.ticks_id & 0xFFFFu) && sub0 < K;
    if (WHOLE_LOOP && whole && (!PERIODS || !short_last)) {
#pragma unroll STEP_UNROLL
        for (int st = 0; st < K; ++st) {
            float *B = lds[(st & 1) ^ 1];
            float lp[R], cc[R];
            // (tried: the reaction term issued before the wait for the window, behind a sched_barrier or ordered asm statements:
            // 12.24-12.84 against 12.14 us per tick, rounding-faithful 19.1-19.8 against 18.5; profiles/r04_ab_reaction_first.txt)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float l = lap9<P>(win[r][1], win[r + 2][1], win[r + 1][0], win[r + 1][2], win[r][0], win[r + 2][0],
                                  win[r][2], win[r + 2][2], win[r + 1][1]);
                if (PHASE) l = pc[r].add(l, win[r][1], win[r + 2][1], win[r + 1][0], win[r + 1][2]);
                lp[r] = l;
                cc[r] = win[r + 1][1];
            }
            if constexpr (M::HAS_VEC) {
                M::template stepN<P, MODE, R>(s, cc, lp, kk, sub0 + st);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) M::template step<P, MODE>(s[r], cc[r], lp[r], kk, sub0 + st);
            }
            if (st + 1 < K) {
#pragma unroll
                for (int r = 0; r < R; ++r) B[wi + ro(r)] = s[r][0];
                FIB_WSTAMP(st);
                __syncthreads();
                window(B, win);
            }
            FIB_STAMP(3 + st);
        }
    } else {
    [[maybe_unused]] int n_lean = 0;                                // sub-steps of this period that need no bookkeeping (LEAN_PREFIX)
    if constexpr (LEAN_PREFIX) n_lean = short_last ? 0 : n_whole;
#pragma unroll STEP_UNROLL
    for (int st = 0; st < K; ++st) {
        float *B = lds[(st & 1) ^ 1];
        bool lean = false;
        if constexpr (LEAN_PREFIX) lean = st < n_lean;
        // rows [ra, rb) of this wave's strip are live at this sub-step (wave-uniform): the box loses one ring per
        // sub-step on every side that is not the domain's edge
        int ra = 0, rb = R;
        if (!lean) {
            ra = top_open ? max(ra_fix, st - c0) : ra_fix;
            rb = bot_open ? min(rb_fix, CY - st - c0) : rb_fix;
        }
        if (lean || (ra == 0 && rb == R)) {
            // ---- whole strip live: one straight-line block.  The R cells of a lane are independent,
            // so the scheduler can interleave their dependency chains; the 3 x (R+2) window is read once.
            float lp[R], cc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float l = lap9<P>(win[r][1], win[r + 2][1], win[r + 1][0], win[r + 1][2], win[r][0], win[r + 2][0],
                                  win[r][2], win[r + 2][2], win[r + 1][1]);
                if (PHASE) l = pc[r].add(l, win[r][1], win[r + 2][1], win[r + 1][0], win[r + 1][2]);
                lp[r] = l;
                cc[r] = win[r + 1][1];
            }
            if constexpr (M::HAS_VEC) {
                M::template stepN<P, MODE, R>(s, cc, lp, kk, sub0 + st);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) M::template step<P, MODE>(s[r], cc[r], lp[r], kk, sub0 + st);
            }
        } else {
            // (a strip of which only some rows are still live: at most two strips of a tile at any sub-step.  Running
            // the block above on all R rows instead was measured: 1 % slower under Fast, 4 % under Exact.)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= ra && r < rb) {                            // scalar branch
                    float l = lap9<P>(win[r][1], win[r + 2][1], win[r + 1][0], win[r + 1][2], win[r][0], win[r + 2][0],
                                      win[r][2], win[r + 2][2], win[r + 1][1]);
                    if (PHASE) l = pc[r].add(l, win[r][1], win[r + 2][1], win[r + 1][0], win[r + 1][2]);
                    M::template step<P, MODE>(s[r], win[r + 1][1], l, kk, sub0 + st);
                }
            }
        }
        // ---- publish the new potential, then fetch the next sub-step's window ---------------------------
        if (st + 1 < K) {
            if (lean) {                                             // (never in a short last period)
#pragma unroll
                for (int r = 0; r < R; ++r) B[wi + ro(r)] = s[r][0];
                FIB_WSTAMP(st);
                __syncthreads();
                window(B, win);
                FIB_STAMP(3 + st);
                continue;
            }
            // (a short last period ends here.  The loop keeps its constant trip count: with a bound read at run time the
            // compiler does not unroll a loop that holds a barrier)
            if constexpr (PERIODS) {
                if (short_last && st + 1 >= sub0) break;
            }
            const unsigned live = ra < rb ? ((1u << rb) - 1u) & ~((1u << ra) - 1u) : 0u;
            const unsigned m = live & pub;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if ((m >> r) & 1u) B[wi + ro(r)] = s[r][0];         // wave-uniform branch, no lane mask
            if (top_r >= 0 || bot_r >= 0) {                         // a strip that holds the grid's row 1 or H-2
                // enforce_boundary + REFLECT: the border and ghost rows above row 1 / below row H-2 take its new value
                // (the columns need nothing: their clamp is in the tap addresses)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r == top_r && ((live >> r) & 1u)) {
                        B[wi + ro(r - 1)] = s[r][0];
                        if (c0 + r >= 1) B[wi + ro(r - 2)] = s[r][0];
                    }
                    if (r == bot_r && ((live >> r) & 1u)) {
                        B[wi + ro(r + 1)] = s[r][0];
                        if (c0 + r + 1 < LQ - 2) B[wi + ro(r + 2)] = s[r][0];
                    }
                }
            }
            FIB_WSTAMP(st);
            __syncthreads();
            window(B, win);
        }
        FIB_STAMP(3 + st);
    }
    }
    if (!MT || tick + 1 >= (int)(mt.ticks_id & 0xFFFFu)) break;

    // ================= between two ticks of one launch =================
    if constexpr (MT) {
        constexpr int NC4 = (NV + 3) / 4;                           // 16-byte cells per grid cell (the last one padded)
        const unsigned plane16 = (unsigned)(g.H * g.W) * 16u;       // bytes of one [H*W] array of 16-byte cells
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(mt.xb, 0, (int)(2u * NC4 * plane16), 0x00020000);
        const unsigned pbase = (unsigned)(tick & 1) * NC4 * plane16;
        FIB_BSTAMP(0);
        // ---- publish the tile: 16-byte cells, write-through -------------------------------------------------
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (own[r]) {
#pragma unroll
                for (int c = 0; c < NC4; ++c) {
                    // (a model whose arrays are not a multiple of four pads its last cell: the index is folded after unrolling)
                    const int i1 = 4 * c + 1 < NV ? 4 * c + 1 : NV - 1, i2 = 4 * c + 2 < NV ? 4 * c + 2 : NV - 1,
                              i3 = 4 * c + 3 < NV ? 4 * c + 3 : NV - 1;
                    const fib_v4f v = {s[r][4 * c], s[r][i1], s[r][i2], s[r][i3]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(fib_v4u, v), rs, (int)(pbase + c * plane16 + (unsigned)off[r] * 16u), 0, 16);
                }
            }
        }
        FIB_BSTAMP(1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // EVERY storing wave, before the barrier / before it is counted
        FIB_BSTAMP(2);
        const unsigned want = mt.epoch0 + (unsigned)tick + 1u;
        // (tried: no barrier here — every wave counts itself in LDS once its stores are acknowledged, the last raises the word:
        // 12.67 against 12.15 us per tick, Beeler-Reuter 15.7 against 15.1; profiles/r04_ab_boundary_and_br.txt)
        __syncthreads();
        FIB_BSTAMP(3);
        // (tried: the tick count pushed into a word of each neighbour's own line, so that a tile polls one line instead of eight:
        // 12.37 against 12.38 us per tick, Beeler-Reuter 15.34 against 15.27; profiles/r04_ab_boundary_and_br.txt)
        if (threadIdx.x == 0) {
            __hip_atomic_store(mt.epoch + (size_t)tile * MT_EPOCH_STRIDE, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // every wave's write-through stores to the host frame have been acknowledged (vmcnt(0) before the barrier above):
            // the word follows them
            if (tick == snap_at) {
                __hip_atomic_store(mt.snap_flag + (size_t)tile * MT_SNAP_STRIDE, mt.snap_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        // ---- wait for the eight neighbours (bounded) ---------------------------------------------------------
        if (wave == 0) {
            const int tiles_y = g.ntiles / g.tiles_x;
            const int d = lane < 4 ? lane : lane + 1;               // 0..8 without the centre
            const int ny = by + d / 3 - 1, nx = bx + d % 3 - 1;
            const bool need = lane < 8 && ny >= 0 && ny < tiles_y && nx >= 0 && nx < g.tiles_x;
            // lane 8 watches the give-up word instead, lane 9 the host's word {launch id, n} (one line further; a launch that
            // ran ahead of the caller, fibhip.hip `run-ahead`): not this launch's id (or 0) = go on; n = MT_CANCEL: the results
            // are not wanted at all; else the caller wants the state after n ticks of this launch — this boundary if n ticks are
            // done now (leave through the write-back), not this tile's business yet if n is still ahead, too late if it is
            // behind.  (The id: earlier launches of the handle may still be queued or running when the word is written.)
            // The word gets here through tile 0, which reads the host's page-locked copy over PCIe — ONE read per tick for the
            // whole grid, issued at the start of a tick and looked at at its end, so the round trip hides behind the sub-steps —
            // and passes it on.  (Measured: a copy through a second stream does not land before the launch has ended, 238-387 us
            // at 512x512; every tile reading host memory itself costs 28 us per tick.)
            if (tile == 0) {
                const unsigned hws = __builtin_amdgcn_readfirstlane(hw);
                if ((hws >> 16) == (mt.ticks_id >> 16) && lane == 0)
                    __hip_atomic_store(mt.err + MT_EPOCH_STRIDE, hws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const unsigned *f = lane == 8 ? mt.err : (lane == 9 ? mt.err + MT_EPOCH_STRIDE
                                                                : mt.epoch + (size_t)(need ? ny * g.tiles_x + nx : tile) * MT_EPOCH_STRIDE);
            const unsigned done = (unsigned)tick + 1u;
            // (tried: the bound as a constant, 12.29 us per tick, or as a shift, 12.24-12.60, against 12.32 in milliseconds;
            // rounding-faithful Fenton 19.4 / 19.0 against 18.8; profiles/r04_ab_kernel_variants.txt)
            const unsigned wait_ms = (unsigned)mt.snap_var >> 8;
            const unsigned long long t_end = __builtin_amdgcn_s_memrealtime() + (wait_ms ? (unsigned long long)wait_ms * 100000ull : MT_WAIT_TICKS);
            for (;;) {
                const unsigned e = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // one ballot for everything that is not the ordinary case: a tile gave up (lane 8), or the host's word concerns
                // this boundary (lane 9)
                const unsigned n_host = e & 0xFFFFu;
                const bool special = lane == 8 ? e != 0u
                                               : (lane == 9 && (e >> 16) == (mt.ticks_id >> 16) && (n_host == MT_CANCEL || n_host <= done));
                // (epochs are compared as differences: they may wrap)
                const bool wait_more = need && (int)(e - want) < 0;
                if (__builtin_amdgcn_ballot_w64(special || wait_more) == 0ull) break;      // the ordinary way out: ONE test
                const unsigned long long sp = __builtin_amdgcn_ballot_w64(special);
                if (sp != 0ull) {
                    const bool gave_up = (sp >> 8) & 1ull;
                    const bool stop_here = !gave_up && (__builtin_amdgcn_readlane(e, 9) & 0xFFFFu) == done;
                    if (lane == 0) {
                        // (the give-up word stands already — it names the launch whose tile gave up first — and stays as it is)
                        mt_abort = stop_here ? 2 : 1;               // 2: leave through the write-back (no neighbour is waited for: it
                    }                                               // may have left already); 1: the results are not wanted / void
                    break;
                }
                if (__builtin_amdgcn_s_memrealtime() > t_end) {
                    if (lane == 0) {
                        // the give-up word names the launch (its id is never 0): the host replays from the state THAT launch
                        // started from (fibhip.hip, `recover`); launches queued behind it find the word and leave at their first
                        // boundary without writing anything.  (A plain store: every tile of a launch writes the same id, and a launch
                        // queued behind one that gave up finds the word before its own wait can run out.  Compare-and-swap: 12.60
                        // against 12.29 us per tick, profiles/r04_ab_kernel_variants.txt.)
                        __hip_atomic_store(mt.err, mt.ticks_id >> 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        mt_abort = 1;
                    }
                    break;
                }
                __builtin_amdgcn_s_sleep(MT_POLL_SLEEP);
            }
        }
        FIB_BSTAMP(4);
        __syncthreads();
        FIB_BSTAMP(5);
        if (mt_abort == 1) {                                        // whole workgroup: the results of this launch are void
            // A tile that leaves because some tile gave up tells the host WHICH launch that was, in the host's own memory (page-
            // locked, behind the host's word): a synchronising call then reads a word of host memory instead of copying one from
            // the device behind every launch.  (Here, on the way out, and not where the wait runs out: the 64-bit address of a
            // system-scope store inside the poll loop cost the Fenton kernel, which sits at its 128 registers, three spills and
            // 2 % of its speed — same-box A/B against round 3's kernel, profiles/r04_ab_pair_lds.txt.)
            if (threadIdx.x == 0) {
                const unsigned who = __hip_atomic_load(mt.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (who != 0u)
                    __hip_atomic_store(mt.snap_flag + MT_HOST_WORD_AT + MT_GIVEUP_WORD, who, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            return;
        }
        if (mt_abort == 2) {                                        // the caller wants exactly the ticks done so far: write them back
            if (threadIdx.x == 0) __hip_atomic_fetch_add(mt.err + 2 * MT_EPOCH_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        // ---- the rim of the compute box, from what the neighbours published ------------------------------
        // (every load of handed-over bytes is an sc1 load; a thread outside the box or the grid reads a clamped
        // address like the prologue does: its values are never used)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!own[r]) {
#pragma unroll
                for (int c = 0; c < NC4; ++c) {
                    // (whole-vector bit cast: __builtin_bit_cast of ONE element of a vector reads element 0 for every index
                    // with this compiler)
                    const fib_v4f v = __builtin_bit_cast(
                        fib_v4f, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(pbase + c * plane16 + (unsigned)off[r] * 16u), 0, 16));
                    s[r][4 * c] = v.x;
                    if (4 * c + 1 < NV) s[r][4 * c + 1 < NV ? 4 * c + 1 : 0] = v.y;
                    if (4 * c + 2 < NV) s[r][4 * c + 2 < NV ? 4 * c + 2 : 0] = v.z;
                    if (4 * c + 3 < NV) s[r][4 * c + 3 < NV ? 4 * c + 3 : 0] = v.w;
                }
            }
        }
        // the potential of the two ring rows around the box (tapped by the first sub-step only), where they are
        // interior rows of the grid: loaded by the first / last wave
        const int gtop = cy0 - 1 + g.row_off, gbot = cy0 + CY + g.row_off;
        const int cxx = clampi(gx, 0, g.W - 1);
        float ring = 0.0f;
        const bool ring_top = wave == 0 && gtop >= 1 && gtop <= g.Hg - 2;
        const bool ring_bot = wave == NW - 1 && gbot >= 1 && gbot <= g.Hg - 2;
        if (ring_top)
            ring = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(pbase + (unsigned)((cy0 - 1) * g.W + cxx) * 16u), 0, 16));
        if (ring_bot)
            ring = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(pbase + (unsigned)((cy0 + CY) * g.W + cxx) * 16u), 0, 16));
        FIB_BSTAMP_WAIT();
        FIB_BSTAMP(6);
        // ---- the whole box's potential into the tile, as after a sub-step — plus the ring (columns 0 and 63 of the
        // tile, rows 0 and CY+1), which the sub-steps never write
        float *B0 = lds[0];
        const int wib = (gx >= 1 && gx <= g.W - 2) ? cell_at(c0 + 1, lane) : cell_at(SPARE_ROW, lane);
        {
            const unsigned live = ra_fix < rb_fix ? ((1u << rb_fix) - 1u) & ~((1u << ra_fix) - 1u) : 0u;
            const unsigned m = live & pub;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if ((m >> r) & 1u) B0[wib + ro(r)] = s[r][0];
            if (top_r >= 0 || bot_r >= 0) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r == top_r && ((live >> r) & 1u)) {
                        B0[wib + ro(r - 1)] = s[r][0];
                        if (c0 + r >= 1) B0[wib + ro(r - 2)] = s[r][0];
                    }
                    if (r == bot_r && ((live >> r) & 1u)) {
                        B0[wib + ro(r + 1)] = s[r][0];
                        if (c0 + r + 1 < LQ - 2) B0[wib + ro(r + 2)] = s[r][0];
                    }
                }
            }
            // (tile rows 0 and CY + 1; in the paired image an even row sits at its word's first dword, an odd one at the second)
            constexpr int RING_BOT = PAIR ? ((CY + 1) >> 1) * 128 + ((CY + 1) & 1) : (CY + 1) * LP;
            const int col = PAIR ? 2 * lane : lane, nobody = cell_at(SPARE_ROW, lane);
            if (ring_top) B0[(gx >= 1 && gx <= g.W - 2) ? col : nobody] = ring;
            if (ring_bot) B0[(gx >= 1 && gx <= g.W - 2) ? RING_BOT + col : nobody] = ring;
        }
        FIB_BSTAMP(7);
        __syncthreads();
        FIB_BSTAMP(8);
        window(B0, win);
        FIB_BSTAMP_WAIT();
        FIB_BSTAMP(9);
    }
    }

    // ---- write back ---------------------------------------------------------------------------------
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (own[r]) {
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if ((WMASK >> v) & 1u) pt.out[v][off[r]] = s[r][v];
        }
    }
    FIB_STAMP(14);
}

template <class M, class P, int MODE, int K, int TX, int TY, int R, bool PHASE>
__global__ void __launch_bounds__(64 * ((TY + 2 * (K - 1) + R - 1) / R))
strip_kernel(Geo g, PtrTab<M::NVAR> pt, PhaseTab ph, typename M::Consts k, int sub0)
{
    strip_body<M, P, MODE, K, TX, TY, R, PHASE, false>(g, pt, ph, k, sub0, MtArgs{});
}

// the same tile program advancing `mt.nticks` ticks of K sub-steps each (K = the tick's sub-steps) in one launch
template <class M, class P, int MODE, int K, int TX, int TY, int R, bool PHASE>
__global__ void __launch_bounds__(64 * ((TY + 2 * (K - 1) + R - 1) / R))
strip_mt_kernel(Geo g, PtrTab<M::NVAR> pt, PhaseTab ph, typename M::Consts k, int sub0, MtArgs mt)
{
    // The host launches this kernel on whole single-device grids only (fibhip.hip mt_eligible: planar slab, no ghost rows, one band
    // of rows): say so, and seven of Geo's twelve scalars are constants or copies instead of live scalar registers — the kernel
    // spills scalar registers into vector lanes as it is, and sits at its 128 vector registers.  (Against the full Geo:
    // profiles/r04_ab_kernel_variants.txt, block 3.)
    g.pitch = g.W;
    g.Hg = g.H;
    g.row_off = 0;
    g.r0 = 0;
    g.r1 = g.H;
    g.rb0 = g.rb1 = 0;
    g.ty_a = 0x7fffffff;
    strip_body<M, P, MODE, K, TX, TY, R, PHASE, true>(g, pt, ph, k, sub0, mt);
}
