// record.inc — what runs on the device behind the ticks while a model runs.  Ten recorders: the per-cell activation maps
// (fibhip_observe_*), the electrode traces (fibhip_electrode_*), the spiral-tip lists (fibhip_tips_*), the movie cube
// (fibhip_frames_*), the tissue statistics (fibhip_stats_*), the unipolar electrograms (fibhip_leads_*), the potential map
// (fibhip_pmap_*), the excited domains and their links from sample to sample (fibhip_waves_*), the per-cell power spectra
// (fibhip_spectrum_*) and the per-cell beat history (fibhip_beats_*), with the velocity fit on the beat and activation
// recorders' planes (fibhip_beats_velocity, fibhip_observe_velocity); the two hooks that write the state: the stimulus program
// (fibhip_stim_*) and the trigger program (fibhip_trig_*), which senses, decides and fires on the device; and the one that
// writes the phase field: the lesion program (fibhip_lesion_*, with fibhip_lesion_apply and fibhip_get_phase beside it).
// The file has three parts: the helpers every recorder shares; the hooks — per recorder its _advance (behind a launch that the
// handle's state has moved with) and its _free, the two functions its row of RECORDERS (recorders.hpp) names —; and the entry
// points, which are one routine with per-recorder content: the argument checks of attach_checks.hpp, attach_ready, Attach,
// sampler_count, ranged_read and detach.  Every hook but the activation recorder's (it sees every tick) and the two programs'
// (stimulus, lesion: event-driven, their own k and next) counts with a Sampler (sampler.hpp) and computes the slot it writes
// from that counter alone, so a replay (sched.inc recover()) writes the same slots again.  What the recorders ask of the
// scheduler is stated in sched.inc ("what the recorders ask of the scheduler").
// (included by fibhip.hip, behind sched.inc)
#include "attach_checks.hpp"    // var, every, capacity, a finite plane, a rectangle, a window, the range of a _read

// ---- helpers ------------------------------------------------------------------------------------------------------------
// where array `var` of the state lives now
static inline float *array_of(const fibhip_ctx *h, int var) { return h->slab[h->cur[var]] + (size_t)var * h->vstride; }
// does `var` name an array Courtemanche's 'slow' assigns (one the aggregates are formed from)?
static inline bool slow_array(int var)
{
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
    return !((Courtemanche::FAST_MASK >> var) & 1u);
#else
    return false;
#endif
}
// the word the kernels of a hook behind an unconfirmed multi-tick launch read first (null: nothing to gate on)
static inline const unsigned *give_up_of(const fibhip_ctx *h, bool behind_mt) { return behind_mt && h->mt.epochs ? h->mt.give_up_word() : nullptr; }
static inline unsigned qnan_bits()
{
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    unsigned bits;
    memcpy(&bits, &qnan, sizeof bits);
    return bits;
}
template <class T>
static inline void dev_free(T *&p)
{
    if (p) hipFree(p);
    p = nullptr;
}
// one kernel on s0 as one event `name` of the timeline; `launch` is the hipLaunchKernelGGL
template <class F>
static int launch_traced(fibhip_ctx *h, const char *name, int K, F launch)
{
    if (int rc = trace_open(h, h->s0, name, K, 0, 0, 0, 1)) return rc;
    launch();
    HIPCHK(hipGetLastError());
    if (int rc = trace_close(h, h->s0)) return rc;
    h->launches++;
    return 0;
}
static inline dim3 blocks_of(size_t threads) { return dim3((unsigned)((threads + 255) / 256)); }
// may a kernel read four cells of a row with one 16-byte load?  The arrays are not row-interleaved, a row is a whole number of
// such loads, and every pointer ORed into `align` is 16-byte aligned
static inline bool rows_vec_ok(const fibhip_ctx *h, uintptr_t align) { return h->pitch == h->d.width && h->d.width % 4 == 0 && (align & 15u) == 0; }
// the four planes of the phase field that the source term of the lead and potential-map recorders reads (LeadArgs,
// PMapSourceArgs), null on a handle without a field
template <class Args>
static inline void phase_planes_fill(const fibhip_ctx *h, Args &a)
{
    a.dpy = h->has_phase ? h->phase3 : nullptr;
    a.dpx = h->has_phase ? h->phase3 + h->cells : nullptr;
    a.q4 = h->has_phase ? h->phase3 + 2 * h->cells : nullptr;
    a.r4 = h->has_phase ? h->phase3 + 3 * h->cells : nullptr;
}

// what no recorder attaches to: a row block, an open tick
static int attach_refusals(const fibhip_ctx *h, const char *who)
{
    if (is_shard(h)) return fail(FIBHIP_EINVAL, "%s: not on a row block (a handle with ghost rows)", who);
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "%s inside an open tick", who);
    return 0;
}
// The step in front of every attach, before anything is allocated: attach_refusals, then the refusals of the recorder's own
// that come behind them (`late`, which returns a status), then the recorder that may still be attached goes (`release`).  In
// between, everything accepted so far runs unrecorded and is confirmed: a multi-tick launch that gave up is recovered HERE,
// before tick k = 0 of the new recorder is defined and before anything of the state is copied for it — it must not start from
// the slab such a launch left void.  The scheduler depends on the order: every journal record is younger than every recorder
// (recorders.hpp recorders_rewind), so `on` is set last, behind the uploads and the wait (Attach)
template <class F>
static int attach_ready(fibhip_ctx *h, const char *who, recorder_free_fn *release, F late)
{
    if (int rc = attach_refusals(h, who)) return rc;
    if (int rc = late()) return rc;
    FLUSH(h);
    SYNC_S0(h);
    if (release) release(h);
    return 0;
}
static int attach_ready(fibhip_ctx *h, const char *who, recorder_free_fn *release)
{
    return attach_ready(h, who, release, [] { return 0; });
}
// The device buffers of one attach, each named ONCE with how it starts — alloc: n elements of T, left as they are or filled
// whole with a byte (0, 0xFF) or with quiet NaNs (QNAN: 4-byte elements); upload: n elements of T from the host; alloc_bytes: a
// buffer that holds more than one type — and then the sequence every _begin runs:
//   the allocations happen as they are named; the first failure sticks and the later ones are skipped;
//   failed(): on failure the HIP error is cleared and the recorder's _free releases what had been allocated — the caller
//             returns FIBHIP_ENOMEM with its own message;
//   enqueue(): the fills and uploads, on s0 — none before every allocation has succeeded, so the failure path has no work in
//             flight on buffers being released;
//   wait(): the stream is waited for: the host tables and the caller's arrays are free again.  finish() is both.
// Not an allocator: it owns nothing once _begin returns, and the _free functions stay the lists they are.
struct Attach {
    enum Fill { KEEP = -1, ZERO = 0, ONES = 0xFF, QNAN = 0x100 };
    struct Start {
        void *dst;
        const void *src;        // an upload, or null: a fill (or nothing)
        Fill fill;
        size_t bytes;
    };
    fibhip_ctx *h;
    hipError_t err = hipSuccess;
    std::vector<Start> starts;
    explicit Attach(fibhip_ctx *h_) : h(h_) {}
    template <class T>
    void alloc_bytes(T *&p, size_t bytes, Fill fill = KEEP, const void *src = nullptr)
    {
        if (err != hipSuccess) return;
        err = hipMalloc((void **)&p, bytes);
        if (err == hipSuccess && (src || fill != KEEP)) starts.push_back({p, src, fill, bytes});
    }
    template <class T>
    void alloc(T *&p, size_t n, Fill fill = KEEP)
    {
        alloc_bytes(p, n * sizeof(T), fill);
    }
    template <class T>
    void upload(T *&p, size_t n, const T *src) { alloc_bytes(p, n * sizeof(T), KEEP, src); }
    bool failed(recorder_free_fn *release)
    {
        if (err == hipSuccess) return false;
        (void)hipGetLastError();
        release(h);
        return true;
    }
    int enqueue()
    {
        for (const Start &s : starts) {
            if (s.src) HIPCHK(hipMemcpyAsync(s.dst, s.src, s.bytes, hipMemcpyHostToDevice, h->s0));
            else if (s.fill == QNAN) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)s.dst, (int)qnan_bits(), s.bytes / 4, h->s0));
            else HIPCHK(hipMemsetAsync(s.dst, (int)s.fill, s.bytes, h->s0));
        }
        starts.clear();
        return 0;
    }
    int wait()
    {
        HIPCHK(wait_stream(h->s0));
        return 0;
    }
    int finish()
    {
        if (int rc = enqueue()) return rc;
        return wait();
    }
};
// the pixel plane of the frame, spectrum and beat recorders from the caller's window, block and reduction
static int window_from(const fibhip_ctx *h, const char *who, const int *window, int by, int bx, int reduce, Window &out)
{
    if (int rc = window_check(who, h->d.height, h->d.width, window, by, bx, reduce, out.oh, out.ow)) return rc;
    out.r0 = window[0]; out.c0 = window[2]; out.by = by; out.bx = bx;
    out.reduce = reduce;
    out.w = nullptr;
    return 0;
}
// every row of the window starts 16-byte aligned in the array `x` and in the weight plane, and four pixels are four cells or
// whole blocks of them: what the three pixel kernels' vector paths share (each adds the alignment of what it writes)
static inline bool window_vec_ok(const fibhip_ctx *h, const Window &p, const float *x)
{
    return rows_vec_ok(h, reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(p.w)) && p.c0 % 4 == 0 && p.ow % 4 == 0;
}
// the window's part of FrameArgs, SpecSampleArgs and BeatArgs
template <class Args>
static inline void window_fill(const fibhip_ctx *h, const Window &p, int var, Args &a)
{
    a.x = array_of(h, var);
    a.w = p.w;
    a.pitch = h->pitch;
    a.wpitch = h->d.width;
    a.r0 = p.r0; a.c0 = p.c0; a.oh = p.oh; a.ow = p.ow; a.by = p.by; a.bx = p.bx;
}
// A read-back: `copies` enqueues it on s0 (launches and asynchronous copies; it returns a status), then the stream is waited
// for.  If that wait found a launch in front of the copies that had given up, the state was recovered and the lost samples
// were taken again: the copies are enqueued once more
template <class F>
static int read_confirmed(fibhip_ctx *h, F copies)
{
    for (int pass = 0; pass < 2; ++pass) {
        const long long fb0 = h->journal.n_fallbacks;
        if (int rc = copies()) return rc;
        SYNC_S0(h);
        if (h->journal.n_fallbacks == fb0) break;
    }
    return 0;
}
// "<who>: no recorder attached (fibhip_<begin>)" (`noun`: the trigger program is a "program")
static int need_attached(bool on, const char *who, const char *begin, const char *noun = "recorder")
{
    if (!on) return fail(FIBHIP_EINVAL, "%s: no %s attached (%s)", who, noun, begin);
    return 0;
}
// every _count.  count_taken is the part the spectrum and beat recorders share with the rest (their outputs may be null)
static int count_taken(fibhip_ctx *h, const Sampler &r, const char *who, const char *begin, const char *noun, long long *n)
{
    if (int rc = need_attached(r.on, who, begin, noun)) return rc;
    SYNC_S0(h);                                        // (a launch that gave up is recovered before anybody counts on its samples)
    *n = r.taken_with(h->pending);                     // (ticks accepted but not launched yet are sampled when they are)
    return 0;
}
static int sampler_count(fibhip_ctx *h, const Sampler &r, const char *who, const char *begin, long long *samples, const char *noun = "recorder")
{
    if (!samples) return fail(FIBHIP_EINVAL, "%s: null argument", who);
    return count_taken(h, r, who, begin, noun, samples);
}
// every _read that takes a range, behind the caller's "attached?": the pending ticks are launched, [first, first + count) is
// checked against the samples taken (`what`: "samples", "frames"), and each copy moves `count` samples of `per` bytes from
// `src` + first * per to `dst`.  The first destination must not be null; a later one that is null is left out
struct ReadCopy {
    void *dst;
    const void *src;
    size_t per;
};
static int ranged_read(fibhip_ctx *h, const Sampler &r, const char *who, const char *what, long long first, long long count,
                       std::initializer_list<ReadCopy> copies)
{
    FLUSH(h);
    if (int rc = range_check(who, what, first, count, r.taken())) return rc;
    if (count > 0 && !copies.begin()->dst) return fail(FIBHIP_EINVAL, "%s: null destination", who);
    return read_confirmed(h, [&] {
        for (const ReadCopy &c : copies)
            if (count > 0 && c.dst)
                HIPCHK(hipMemcpyAsync(c.dst, static_cast<const char *>(c.src) + (size_t)first * c.per, (size_t)count * c.per, hipMemcpyDeviceToHost, h->s0));
        return 0;
    });
}
// every _end: nothing to do unless attached; else the ticks accepted while attached are sampled (their events applied), and
// confirmed, so that no replay is left that would want the recorder; then its buffers go
static int detach(fibhip_ctx *h, bool on, recorder_free_fn *release)
{
    if (!on) return 0;
    FLUSH(h);
    SYNC_S0(h);
    release(h);
    return 0;
}
// the four maps of a _peak or a _summary, `npix` 4-byte values each, to the destinations that are not null
static int copy_maps(fibhip_ctx *h, const float *maps, size_t npix, void *const dst[4])
{
    for (int i = 0; i < 4; ++i)
        if (dst[i]) HIPCHK(hipMemcpyAsync(dst[i], maps + (size_t)i * npix, npix * sizeof(float), hipMemcpyDeviceToHost, h->s0));
    return 0;
}

// ---- the hooks ----------------------------------------------------------------------------------------------------------
// the activation recorder's update for the tick just committed (observed tick k = obs_k), on s0 behind it
static int observe_enqueue(fibhip_ctx *h)
{
    const size_t n = h->cells;
    const float *pot = array_of(h, h->obs.var);
    ObsMaps m;
    m.first = h->obs.buf + n;
    m.last = h->obs.buf + 2 * n;
    m.prev = h->obs.buf + 3 * n;
    m.apd = h->obs.buf + 4 * n;
    m.count = reinterpret_cast<int *>(h->obs.buf + 5 * n);
    const float tick = (float)(h->d.dt * h->spt);
    const float t0 = (float)((double)h->obs.k * h->d.dt * h->spt);
    const bool vec = h->pitch == h->d.width && (reinterpret_cast<uintptr_t>(pot) & 15u) == 0;
    const size_t threads = vec ? n / 4 + n % 4 : n;
    const Geo g = base_geo(h);
    const dim3 grid = blocks_of(threads);
    if (int rc = launch_traced(h, "observe_kernel", 0, [&] {
            if (vec) hipLaunchKernelGGL(observe_kernel<true>, grid, dim3(256), 0, h->s0, g, pot, h->obs.buf, m, h->obs.up, h->obs.down, t0, tick);
            else hipLaunchKernelGGL(observe_kernel<false>, grid, dim3(256), 0, h->s0, g, pot, h->obs.buf, m, h->obs.up, h->obs.down, t0, tick);
        }))
        return rc;
    h->obs.k++;
    return 0;
}

// The electrode recorder's hook behind a launch of `ticks` ticks (plain: commit_impl; multi-tick: mt_launch).  A sample that is
// due is enqueued on s0 behind that launch and reads the state the handle has just moved to.  The slot is a kernel argument
// computed from the host's counter, never a pointer kept on the device: a replay (recover()) writes the same slots again.
static int electrode_advance(fibhip_ctx *h, int ticks, bool)
{
    ElRec &r = h->el;
    long long s;
    if (!r.advance(ticks, &s)) return 0;
    if (s >= r.cap) return fail(FIBHIP_EINVAL, "electrode recorder: trace full");              // (fibhip_step refuses before this)
    const float *x = array_of(h, r.var);
    float *row = r.trace + (size_t)s * r.n;
    if (int rc = launch_traced(h, "electrode_kernel", 0, [&] {
            hipLaunchKernelGGL(electrode_kernel, dim3((unsigned)r.nchunks), dim3(EL_THREADS), 0, h->s0, x, h->pitch, r.chunks, r.w, row, r.part);
        }))
        return rc;
    if (!r.ncomb) return 0;
    return launch_traced(h, "electrode_combine_kernel", 0,
                         [&] { hipLaunchKernelGGL(electrode_combine_kernel, dim3((unsigned)r.ncomb), dim3(256), 0, h->s0, r.comb, r.part, row); });
}
static void electrode_free(fibhip_ctx *h)
{
    dev_free(h->el.chunks);
    dev_free(h->el.comb);
    dev_free(h->el.w);
    dev_free(h->el.part);
    dev_free(h->el.trace);
    h->el.on = false;
}

// The tip recorder's hook: at a sample tick the sample's three counters are zeroed and tip_kernel is enqueued behind them on
// s0.  Slot and counters are addressed from the host's counter, so a replay zeroes and fills the same slot again; records
// beyond `stored` are never looked at, so the list itself is not cleared.
static int tips_advance(fibhip_ctx *h, int ticks, bool)
{
    TipRec &r = h->tip;
    long long s;
    if (!r.advance(ticks, &s)) return 0;
    if (s >= r.cap) return fail(FIBHIP_EINVAL, "tip recorder: trace full");                    // (fibhip_step refuses before this)
    const float *a = array_of(h, r.var), *b = array_of(h, r.var2);
    int *cnt = r.counts + 3 * (size_t)s;
    int4 *rec = reinterpret_cast<int4 *>(r.records) + (size_t)s * (size_t)r.max_tips;
    const Geo g = base_geo(h);
    const bool vec = rows_vec_ok(h, reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b));
    const dim3 grid = blocks_of((size_t)(g.H - 1) * (size_t)(vec ? g.W / 4 : g.W - 1));
    HIPCHK(hipMemsetAsync(cnt, 0, 3 * sizeof(int), h->s0));
    return launch_traced(h, "tip_kernel", 0, [&] {
        if (vec) hipLaunchKernelGGL(tip_kernel<true>, grid, dim3(256), 0, h->s0, g, a, b, r.a0, r.b0, r.mask, cnt, rec, r.max_tips);
        else hipLaunchKernelGGL(tip_kernel<false>, grid, dim3(256), 0, h->s0, g, a, b, r.a0, r.b0, r.mask, cnt, rec, r.max_tips);
    });
}
static void tips_free(fibhip_ctx *h)
{
    dev_free(h->tip.mask);
    dev_free(h->tip.counts);
    dev_free(h->tip.records);
    h->tip.on = false;
}

// The frame recorder's hook.  Its counter started at every - first (fibhip_frames_begin), so a sample is due when it lands on a
// multiple of `every`, like the others'; the frame's slot in the cube is a kernel argument computed from that counter, so a
// replay fills the same slot again.
template <bool U8, bool MEAN>
static void frame_launch(const FrameArgs &a, bool vec, size_t threads, hipStream_t st)
{
    const dim3 grid = blocks_of(threads), block(256);
    if (vec) hipLaunchKernelGGL((frame_kernel<U8, MEAN, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((frame_kernel<U8, MEAN, false>), grid, block, 0, st, a);
}

static int frames_advance(fibhip_ctx *h, int ticks, bool)
{
    FrRec &f = h->fr;
    long long s;
    if (!f.advance(ticks, &s)) return 0;
    if (s >= f.cap) return fail(FIBHIP_EINVAL, "frame recorder: trace full");                 // (fibhip_step refuses before this)
    FrameArgs a;
    window_fill(h, f, f.var, a);
    a.out = f.cube + (size_t)s * f.frame_bytes();
    a.lo = f.lo; a.span = f.span;
    // ... and so does every row of the frame (four pixels are 16 bytes of a float32 frame and 4 bytes of an 8-bit one)
    const bool u8 = f.format == FIBHIP_FRAME_U8, mean = f.reduce == FIBHIP_FRAME_MEAN;
    const bool vec = window_vec_ok(h, f, a.x) && (reinterpret_cast<uintptr_t>(a.out) & (u8 ? 3u : 15u)) == 0;
    const size_t threads = (size_t)f.oh * (size_t)(vec ? f.ow / 4 : f.ow);
    return launch_traced(h, "frame_kernel", 0, [&] {
        if (u8 && mean) frame_launch<true, true>(a, vec, threads, h->s0);
        else if (u8) frame_launch<true, false>(a, vec, threads, h->s0);
        else if (mean) frame_launch<false, true>(a, vec, threads, h->s0);
        else frame_launch<false, false>(a, vec, threads, h->s0);
    });
}
static void frames_free(fibhip_ctx *h)
{
    dev_free(h->fr.w);
    dev_free(h->fr.cube);
    h->fr.on = false;
}

static_assert(ST_SLOTS == FIBHIP_MAX_STAT_COLS_PER_ARRAY && (int)ST_KINDS == (int)FIBHIP_STAT_NONFINITE + 1 && (int)ST_SUM == (int)FIBHIP_STAT_SUM &&
                  (int)ST_BELOW == (int)FIBHIP_STAT_BELOW && ST_MAX_CHUNKS == 4 * 64 && ST_MIN_CHUNK % 4 == 0,
              "stats_kernel's constants follow include/fibhip.h; stats_combine_kernel folds four chunks per lane of one wave");
// The statistics recorder's hook: at a sample tick stats_kernel is enqueued on s0 behind the launch that ended there (one
// partial per column and chunk), and stats_combine_kernel behind it (the sample's row).  The row's slot is a kernel argument
// computed from the host's counter, so a replay (recover()) writes the same slot again; the partials are rewritten whole by
// every sample.
static int stats_advance(fibhip_ctx *h, int ticks, bool)
{
    StRec &r = h->st;
    long long s;
    if (!r.advance(ticks, &s)) return 0;
    if (s >= r.cap) return fail(FIBHIP_EINVAL, "statistics recorder: trace full");             // (fibhip_step refuses before this)
    StArgs a;
    a.slab0 = h->slab[0];
    a.slab1 = h->slab[1];
    a.cur_mask = 0u;
    uintptr_t align = reinterpret_cast<uintptr_t>(r.w) | reinterpret_cast<uintptr_t>(r.mask);
    for (int i = 0; i < r.narr; ++i) {
        const int v = r.vars[i];
        if (h->cur[v]) a.cur_mask |= 1u << v;
        align |= reinterpret_cast<uintptr_t>(array_of(h, v));
    }
    a.W = h->d.width;
    a.pitch = h->pitch;
    a.vstride = h->vstride;
    a.chunks = r.chunks;
    a.arrs = r.arrs;
    a.w = r.w;
    a.mask = r.mask;
    a.part = r.part;
    a.nchunks = r.nchunks;
    // (the chunk table was cut for the vector path exactly when pitch == W and W % 4 == 0; the pointers are looked at here)
    const bool vec = rows_vec_ok(h, align);
    const dim3 grid((unsigned)r.nchunks, (unsigned)r.narr);
    if (int rc = launch_traced(h, "stats_kernel", 0, [&] {
            if (vec) hipLaunchKernelGGL(stats_kernel<true>, grid, dim3(ST_THREADS), 0, h->s0, a);
            else hipLaunchKernelGGL(stats_kernel<false>, grid, dim3(ST_THREADS), 0, h->s0, a);
        }))
        return rc;
    return launch_traced(h, "stats_combine_kernel", 0, [&] {
        hipLaunchKernelGGL(stats_combine_kernel, dim3(1), dim3(256), 0, h->s0, r.cols, r.ncols, r.part, r.nchunks, r.trace + (size_t)s * r.ncols);
    });
}
static void stats_free(fibhip_ctx *h)
{
    dev_free(h->st.chunks);
    dev_free(h->st.arrs);
    dev_free(h->st.cols);
    dev_free(h->st.w);
    dev_free(h->st.mask);
    dev_free(h->st.part);
    dev_free(h->st.trace);
    h->st.on = false;
}

static_assert(LD_MAX == FIBHIP_MAX_LEADS && LD_MAX % LD_GROUP == 0 && LD_THREADS == 256 && LD_TY % (LD_THREADS / 64) == 0,
              "lead_kernel's constants follow include/fibhip.h; four waves, each LD_CPT rows of the tile");
// The lead recorder's hook: at a sample tick lead_kernel is enqueued on s0 behind the launch that ended there (one partial per
// lead and tile) and lead_combine_kernel behind it (the sample's row).  The row's slot is a kernel argument computed from the
// host's counter, so a replay (recover()) writes the same slot again; the partials are rewritten whole by every sample.
static int leads_advance(fibhip_ctx *h, int ticks, bool)
{
    LeadRec &r = h->ld;
    long long s;
    if (!r.advance(ticks, &s)) return 0;
    if (s >= r.cap) return fail(FIBHIP_EINVAL, "lead recorder: trace full");                   // (fibhip_step refuses before this)
    LeadArgs a;
    a.x = array_of(h, r.var);
    a.w = r.weight;
    phase_planes_fill(h, a);
    a.pos = r.pos;
    a.tables = r.tables;
    a.part = r.part;
    a.H = h->d.height; a.W = h->d.width; a.pitch = h->pitch; a.n = r.n;
    const dim3 grid((unsigned)r.tiles_x, (unsigned)r.tiles_y);
    if (int rc = launch_traced(h, "lead_kernel", 0, [&] { hipLaunchKernelGGL(lead_kernel, grid, dim3(LD_THREADS), 0, h->s0, a); })) return rc;
    double *row = r.rows + (size_t)s * (size_t)r.n;
    return launch_traced(h, "lead_combine_kernel", 0, [&] {
        hipLaunchKernelGGL(lead_combine_kernel, dim3((unsigned)r.n), dim3(256), 0, h->s0, (const double *)r.part, r.tiles_x * r.tiles_y, row);
    });
}
static void leads_free(fibhip_ctx *h)
{
    dev_free(h->ld.pos);
    dev_free(h->ld.tables);
    dev_free(h->ld.weight);
    dev_free(h->ld.part);
    dev_free(h->ld.rows);
    h->ld.on = false;
}

static_assert(PM_MAX_RADIUS == FIBHIP_PMAP_MAX_RADIUS && PM_MAX_STEP == FIBHIP_PMAP_MAX_STEP && PM_THREADS == 256 && PM_TY % (PM_THREADS / 64) == 0 &&
                  PM_MAX_STEP * (PM_TX - 1 + (2 * PM_MAX_RADIUS + PM_MAX_STEP) / PM_MAX_STEP) <= PM_LDS_FLOATS,
              "pmap_conv_kernel's constants follow include/fibhip.h; four waves, PM_SPL site rows each; one row of the widest span fits in LDS");
// The potential-map recorder's hook: at a sample tick pmap_source_kernel is enqueued on s0 behind the launch that ended there
// (every cell of the scratch plane) and pmap_conv_kernel behind it (every site of the sample's slot).  The slot is a kernel
// argument computed from the host's counter, so a replay (recover()) writes the same slot again.
static int pmap_advance(fibhip_ctx *h, int ticks, bool)
{
    PMapRec &r = h->pm;
    long long s;
    if (!r.advance(ticks, &s)) return 0;
    if (s >= r.cap) return fail(FIBHIP_EINVAL, "potential-map recorder: trace full");          // (fibhip_step refuses before this)
    const int H = h->d.height, W = h->d.width;
    PMapSourceArgs q;
    q.x = array_of(h, r.var);
    q.w = r.weight;
    phase_planes_fill(h, q);
    q.q = r.q;
    q.H = H; q.W = W; q.pitch = h->pitch; q.R = r.R;
    const dim3 qgrid((unsigned)((W + LD_TX - 1) / LD_TX), (unsigned)((H + LD_TY - 1) / LD_TY));
    if (int rc = launch_traced(h, "pmap_source_kernel", 0, [&] { hipLaunchKernelGGL(pmap_source_kernel, qgrid, dim3(LD_THREADS), 0, h->s0, q); }))
        return rc;
    PMapArgs a;
    a.q = r.q;
    a.tab = r.tab;
    a.out = r.cube + (size_t)s * r.npix();
    a.R = r.R; a.r0 = r.r0; a.c0 = r.c0; a.sy = r.sy; a.sx = r.sx; a.oh = r.oh; a.ow = r.ow;
    a.qh = H + 2 * r.R; a.qw = W + 2 * r.R;
    a.pw = r.pw; a.roww = r.roww; a.slab = r.slab;
    // a tile is 64 sites wide and four site rows per wave high: a small lattice gets workgroups of fewer waves, so that there are
    // workgroups for the machine's 256 compute units (the sums do not depend on the tile: their order is R's alone)
    const int tiles_x = (r.ow + PM_TX - 1) / PM_TX;
    int waves = PM_THREADS / 64;
    while (waves > 1 && tiles_x * ((r.oh + waves * PM_SPL - 1) / (waves * PM_SPL)) < 256) waves /= 2;
    const dim3 grid((unsigned)tiles_x, (unsigned)((r.oh + waves * PM_SPL - 1) / (waves * PM_SPL)));
    return launch_traced(h, "pmap_conv_kernel", 0, [&] {
        if (r.sx == 1) hipLaunchKernelGGL(pmap_conv_kernel<true>, grid, dim3(64 * waves), 0, h->s0, a);
        else hipLaunchKernelGGL(pmap_conv_kernel<false>, grid, dim3(64 * waves), 0, h->s0, a);
    });
}
static void pmap_free(fibhip_ctx *h)
{
    dev_free(h->pm.weight);
    dev_free(h->pm.tab);
    dev_free(h->pm.q);
    dev_free(h->pm.cube);
    dev_free(h->pm.maps);
    h->pm.on = false;
}

static_assert(sizeof(WaveRecord) == sizeof(fibhip_wave_record) && offsetof(WaveRecord, sum_r) == offsetof(fibhip_wave_record, sum_r) &&
                  offsetof(WaveRecord, r0) == offsetof(fibhip_wave_record, r0) && sizeof(WaveRecord) == 40 && WV_THREADS == 256 &&
                  WV_TX == 64 && WV_TY % (WV_THREADS / 64) == 0,
              "the wave kernels' record is include/fibhip.h's; a tile row is one wave, four waves share the rows of a tile");
static_assert(sizeof(WaveLink) == sizeof(fibhip_wave_link) && sizeof(WaveLink) == 12 && offsetof(WaveLink, seed) == offsetof(fibhip_wave_link, seed) &&
                  offsetof(WaveLink, overlap) == offsetof(fibhip_wave_link, overlap) && WV_LINK_PROBES == 32 &&
                  4ll * FIBHIP_MAX_WAVE_LINKS <= 0x40000000ll,
              "the link kernels' record is include/fibhip.h's; a table of <= 32 entries is covered by one probe sequence; T fits 32 bits");
// The wave recorder's hook: at a sample tick the sample's three counts are zeroed and the four kernels are enqueued behind them
// on s0 (the merge only where the grid has more than one tile).  Counts and records are addressed from the host's counter, so a
// replay zeroes and fills the same slot again; the two planes belong to whichever sample is the latest.  With links on, a clear
// of the table and of the sample's link counts and the two link kernels follow on the same stream; those two are gated
// (`behind_mt`), the four in front of them are not: `labels` stays scratch, `prev` stays the plane of the last good sample.
static int waves_advance(fibhip_ctx *h, int ticks, bool behind_mt)
{
    WaveRec &r = h->wv;
    long long s;
    if (!r.advance(ticks, &s)) return 0;
    if (s >= r.cap) return fail(FIBHIP_EINVAL, "wave recorder: trace full");                   // (fibhip_step refuses before this)
    const int H = h->d.height, W = h->d.width, ncells = (int)h->cells;
    int *cnt = r.counts + 3 * (size_t)s;
    WaveRecord *rec = r.records + (size_t)s * (size_t)r.max_waves;
    WaveArgs a;
    a.x = array_of(h, r.var);
    a.x2 = r.var2 >= 0 ? array_of(h, r.var2) : nullptr;
    a.mask = r.mask;
    a.labels = r.labels;
    a.cnt = cnt;
    a.H = H; a.W = W; a.pitch = h->pitch;
    a.kind = r.kind; a.kind2 = r.kind2; a.conn = r.conn;
    a.level = r.level; a.level2 = r.level2;
    const size_t tiles = (size_t)((W + WV_TX - 1) / WV_TX) * (size_t)((H + WV_TY - 1) / WV_TY);
    const int nbr = (H - 1) / WV_TY, nbc = (W - 1) / WV_TX;
    const size_t border = (size_t)nbr * (size_t)W + (size_t)nbc * (size_t)H;
    const dim3 cells = blocks_of(h->cells);
    HIPCHK(hipMemsetAsync(cnt, 0, 3 * sizeof(int), h->s0));
    if (int rc = launch_traced(h, "wave_label_kernel", 0,
                               [&] { hipLaunchKernelGGL(wave_label_kernel, dim3((unsigned)tiles), dim3(WV_THREADS), 0, h->s0, a); }))
        return rc;
    if (border)
        if (int rc = launch_traced(h, "wave_merge_kernel", 0, [&] {
                hipLaunchKernelGGL(wave_merge_kernel, blocks_of(border), dim3(256), 0, h->s0, r.labels, H, W, r.conn, nbr, nbc);
            }))
            return rc;
    if (int rc = launch_traced(h, "wave_root_kernel", 0, [&] {
            hipLaunchKernelGGL(wave_root_kernel, cells, dim3(256), 0, h->s0, r.labels, r.slots, ncells, cnt, rec, r.max_waves);
        }))
        return rc;
    if (int rc = launch_traced(h, "wave_reduce_kernel", 0, [&] {
            hipLaunchKernelGGL(wave_reduce_kernel, blocks_of((h->cells + WV_RED_CPT - 1) / WV_RED_CPT), dim3(256), 0, h->s0, (const int *)r.labels, (const int *)r.slots, ncells, W, rec, r.max_waves);
        }))
        return rc;
    if (!r.max_links) return 0;
    // links: the table and the sample's four counts are cleared (the table is scratch; a void sample's counts stay zero until
    // the replay takes it again), then the two kernels, which look at the give-up word behind an unconfirmed launch
    const unsigned *give_up = give_up_of(h, behind_mt);
    const unsigned T = r.link_entries;
    int *lcnt = r.link_counts + 4 * (size_t)s;
    WaveLink *lrec = r.link_records + (size_t)s * (size_t)r.max_links;
    HIPCHK(hipMemsetAsync(r.link_table, 0, (size_t)T * (sizeof(unsigned long long) + sizeof(int)), h->s0));
    HIPCHK(hipMemsetAsync(lcnt, 0, 4 * sizeof(int), h->s0));
    if (int rc = launch_traced(h, "wave_link_kernel", 0, [&] {
            hipLaunchKernelGGL(wave_link_kernel, blocks_of((h->cells + WV_LINK_CPT - 1) / WV_LINK_CPT), dim3(256), 0, h->s0, (const int *)r.labels, r.prev, ncells, r.link_table, T - 1u, lcnt, give_up);
        }))
        return rc;
    return launch_traced(h, "wave_link_pack_kernel", 0, [&] {
        hipLaunchKernelGGL(wave_link_pack_kernel, blocks_of(T), dim3(256), 0, h->s0, (const unsigned long long *)r.link_table, T, lcnt, lrec, r.max_links, give_up);
    });
}
static void wave_links_free(fibhip_ctx *h)
{
    dev_free(h->wv.prev);
    dev_free(h->wv.link_table);
    dev_free(h->wv.link_counts);
    dev_free(h->wv.link_records);
    h->wv.max_links = 0;
    h->wv.link_entries = 0;
}
static void waves_free(fibhip_ctx *h)
{
    wave_links_free(h);
    dev_free(h->wv.mask);
    dev_free(h->wv.labels);
    dev_free(h->wv.slots);
    dev_free(h->wv.counts);
    dev_free(h->wv.records);
    h->wv.on = false;
}

static_assert(SPEC_MAX_BINS == FIBHIP_SPECTRUM_MAX_BINS && SPEC_MAX_CHUNK == FIBHIP_SPECTRUM_MAX_CHUNK &&
                  FIBHIP_SPECTRUM_MAX_NFFT / 2 * (long long)(FIBHIP_SPECTRUM_MAX_NFFT - 1) <= 0xFFFFFFFFll,
              "the spectrum kernels' constants follow include/fibhip.h; spectrum_fold_kernel's k * j fits 32 bits unsigned");
typedef void (*spec_fold_fn)(const float *, float *, float *, float *, const float *, const float2 *, const int *, size_t, int, int, int, int,
                             const unsigned *);
template <int... C>
static spec_fold_fn spec_fold_pick(int chunk, std::integer_sequence<int, C...>)
{
    static const spec_fold_fn table[] = {spectrum_fold_kernel<C + 1>...};      // chunk = 1 .. SPEC_MAX_CHUNK
    return table[chunk - 1];
}
// The spectrum recorder's hook behind a launch of `ticks` ticks: at a sample tick spectrum_sample_kernel writes the pixel plane
// into slot s mod chunk of the ring, and behind the sample that fills the ring spectrum_fold_kernel folds the chunk.  Slot,
// segment position and whether the chunk ends a segment are kernel arguments computed from the host's counter.  `behind_mt`: as
// for stim_advance — both kernels are handed the give-up word and write nothing once a launch in front of them gave up (the
// fold accumulates, and a void sample must not overwrite a slot whose fold was skipped: record_kernels.inc); recover() rewinds
// the counter and the replay comes through here again.
static int spectrum_advance(fibhip_ctx *h, int ticks, bool behind_mt)
{
    SpRec &r = h->sp;
    long long s;
    if (!r.advance(ticks, &s)) return 0;
    const unsigned *give_up = give_up_of(h, behind_mt);
    const size_t npix = r.npix();
    SpecSampleArgs a;
    window_fill(h, r, r.var, a);
    a.out = r.ring + (size_t)(s % r.chunk) * npix;
    a.give_up = give_up;
    const bool mean = r.reduce == FIBHIP_FRAME_MEAN;
    const bool vec = r.by == 1 && r.bx == 1 && window_vec_ok(h, r, a.x) && (reinterpret_cast<uintptr_t>(a.out) & 15u) == 0;
    const dim3 grid = blocks_of((size_t)r.oh * (size_t)(vec ? r.ow / 4 : r.ow)), block(256);
    if (int rc = launch_traced(h, "spectrum_sample_kernel", 0, [&] {
            if (vec) hipLaunchKernelGGL((spectrum_sample_kernel<false, true>), grid, block, 0, h->s0, a);
            else if (mean) hipLaunchKernelGGL((spectrum_sample_kernel<true, false>), grid, block, 0, h->s0, a);
            else hipLaunchKernelGGL((spectrum_sample_kernel<false, false>), grid, block, 0, h->s0, a);
        }))
        return rc;
    if ((s + 1) % r.chunk) return 0;
    const int j0 = (int)((s + 1 - r.chunk) % r.nfft);                // the segment position of ring slot 0 (a chunk never straddles a segment)
    const size_t plane = (size_t)r.nb * npix;
    return launch_traced(h, "spectrum_fold_kernel", 0, [&] {
        hipLaunchKernelGGL(spec_fold_pick(r.chunk, std::make_integer_sequence<int, SPEC_MAX_CHUNK>()), blocks_of(npix), block, 0, h->s0,
                           (const float *)r.ring, r.acc, r.acc + plane, r.acc + 2 * plane, (const float *)r.win,
                           reinterpret_cast<const float2 *>(r.tw), (const int *)r.bins, npix, r.nfft, r.nb, j0, j0 + r.chunk == r.nfft ? 1 : 0, give_up);
    });
}
static void spectrum_free(fibhip_ctx *h)
{
    SpRec &r = h->sp;
    dev_free(r.w);
    dev_free(r.win);
    dev_free(r.tw);
    dev_free(r.bins);
    dev_free(r.ring);
    dev_free(r.acc);
    dev_free(r.maps);
    r.on = false;
}

static_assert(BEAT_MAX_DEPTH == FIBHIP_BEATS_MAX_DEPTH, "beat_summary_kernel's walk follows include/fibhip.h");
// beat_kernel over the recorder's map: `init` — the launch of beats_begin, xp = the pixel of the current state; otherwise sample
// `s` (0-based), whose t0 and step follow from s and the stride alone
static int beats_launch(fibhip_ctx *h, bool init, long long s, const unsigned *give_up)
{
    BeatRec &r = h->bt;
    const size_t npix = r.npix();
    BeatArgs a;
    window_fill(h, r, r.var, a);
    a.xp = r.state;
    a.pk = r.state + npix;
    a.n = reinterpret_cast<int *>(r.state + 2 * npix);
    a.t_up = r.ring;
    a.t_down = r.ring + (size_t)r.depth * npix;
    a.peak = r.ring + 2 * (size_t)r.depth * npix;
    a.depth = r.depth;
    a.init = init ? 1 : 0;
    a.up = r.up;
    a.down = r.down;
    a.step = (float)((double)r.every * h->d.dt * h->spt);
    a.t0 = (float)((double)(s * r.every) * h->d.dt * h->spt);
    a.give_up = give_up;
    const bool mean = r.reduce == FIBHIP_FRAME_MEAN;
    // (the recorder's planes come from hipMalloc and npix is a multiple of 4 here: xp, pk and every row of them are aligned)
    const bool vec = r.by == 1 && r.bx == 1 && window_vec_ok(h, r, a.x) &&
                     ((reinterpret_cast<uintptr_t>(a.xp) | reinterpret_cast<uintptr_t>(a.pk)) & 15u) == 0;
    const dim3 grid = blocks_of((size_t)r.oh * (size_t)(vec ? r.ow / 4 : r.ow)), block(256);
    // (the timeline event's K says which path ran: the pixels per thread, 4 on the vector path and 1 on the scalar one)
    return launch_traced(h, "beat_kernel", vec ? 4 : 1, [&] {
        if (vec) hipLaunchKernelGGL((beat_kernel<false, true>), grid, block, 0, h->s0, a);
        else if (mean) hipLaunchKernelGGL((beat_kernel<true, false>), grid, block, 0, h->s0, a);
        else hipLaunchKernelGGL((beat_kernel<false, false>), grid, block, 0, h->s0, a);
    });
}

// The beat recorder's hook behind a launch of `ticks` ticks: at a sample tick beat_kernel compares the pixel plane with the
// previous sample's and records the events.  `behind_mt`: as for spectrum_advance — the kernel is handed the give-up word and
// writes nothing once a launch in front of it gave up; recover() rewinds the counter and the replay comes through here again,
// with the same sample index.
static int beats_advance(fibhip_ctx *h, int ticks, bool behind_mt)
{
    long long s;
    return h->bt.advance(ticks, &s) ? beats_launch(h, false, s, give_up_of(h, behind_mt)) : 0;
}
static void beats_free(fibhip_ctx *h)
{
    BeatRec &r = h->bt;
    dev_free(r.w);
    dev_free(r.state);
    dev_free(r.ring);
    dev_free(r.maps);
    r.on = false;
}

// What the stimulus program and the trigger program share.  stim_entry_from: one stimulus {var, mode, shape, rectangle, v, floor,
// plane} as the caller gave it -> a validated StimEntry with its visit box cut (the timing fields are the caller's); `who` and
// `what` name the entry point and the thing ("stim_begin", "entry" / "trig_begin", "rule") in the message.  stim_due_fill: a
// StimEntry -> the StimDue a kernel takes by value, on the slab that holds the array now.
static int stim_entry_from(const fibhip_ctx *h, const char *who, const char *what, int i, int var, int mode, int shape, int r0, int r1, int c0,
                           int c1, float v, float floor, int plane, int nplanes, const float *planes, StimEntry &e)
{
    const int H = h->d.height, W = h->d.width;
    const float ninf = -std::numeric_limits<float>::infinity();
    if (int rc = var_check(var, h->nvar, "%s: %s %d", who, what, i)) return rc;
    if (mode != FIBHIP_STIM_MAX && mode != FIBHIP_STIM_ADD) return fail(FIBHIP_EINVAL, "%s: %s %d: unknown mode %d", who, what, i, mode);
    if (shape != FIBHIP_STIM_RECT && shape != FIBHIP_STIM_PLANE) return fail(FIBHIP_EINVAL, "%s: %s %d: unknown shape %d", who, what, i, shape);
    e.var = var; e.mode = mode;
    const float untouched = mode == FIBHIP_STIM_MAX ? ninf : 0.f;
    if (shape == FIBHIP_STIM_RECT) {
        if (int rc = rect_check(h->d.height, h->d.width, r0, r1, c0, c1, "%s: %s %d: ", who, what, i)) return rc;
        if (!std::isfinite(v)) return fail(FIBHIP_EINVAL, "%s: %s %d: v must be finite (got %g)", who, what, i, v);
        if (!(std::isfinite(floor) || (mode == FIBHIP_STIM_MAX && floor == ninf)))
            return fail(FIBHIP_EINVAL, "%s: %s %d: floor must be finite%s (got %g)", who, what, i, mode == FIBHIP_STIM_MAX ? " or -inf" : "", floor);
        e.plane = -1;
        e.r0 = r0; e.r1 = r1; e.c0 = c0; e.c1 = c1;
        e.v = v; e.floor = floor;
        const bool outside_untouched = floor == untouched;
        e.b_r0 = outside_untouched ? r0 : 0; e.b_r1 = outside_untouched ? r1 : H;
        e.b_c0 = outside_untouched ? c0 : 0; e.b_c1 = outside_untouched ? c1 : W;
    } else {
        if (plane < 0 || plane >= nplanes) return fail(FIBHIP_EINVAL, "%s: %s %d: plane %d of %d", who, what, i, plane, nplanes);
        e.plane = plane;
        const float *p = planes + (size_t)plane * h->cells;
        int b_r0 = H, b_r1 = 0, b_c0 = W, b_c1 = 0;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (!(p[(size_t)y * W + x] == untouched)) {         // (a NaN is not "untouched")
                    b_r0 = imin(b_r0, y); b_r1 = imax(b_r1, y + 1);
                    b_c0 = imin(b_c0, x); b_c1 = imax(b_c1, x + 1);
                }
        if (b_r0 >= b_r1) b_r0 = b_r1 = b_c0 = b_c1 = 0;
        e.b_r0 = b_r0; e.b_r1 = b_r1; e.b_c0 = b_c0; e.b_c1 = b_c1;
    }
    e.slow = h->d.model == FIBHIP_COURT && slow_array(var);
    return 0;
}
static void stim_due_fill(const fibhip_ctx *h, const StimEntry &e, float *planes, StimDue &d)
{
    d.x = array_of(h, e.var);
    d.plane = e.plane >= 0 ? planes + (size_t)e.plane * h->cells : nullptr;
    d.mode = e.mode;
    d.b_r0 = e.b_r0; d.b_r1 = e.b_r1; d.b_c0 = e.b_c0; d.b_c1 = e.b_c1;
    d.r0 = e.r0; d.r1 = e.r1; d.c0 = e.c0; d.c1 = e.c1;
    d.v = e.v; d.floor = e.floor;
}
// The StimArgs of one launch of stim_kernel or stim_gated_kernel.  stim_args_add: entry `e` becomes a.e[i], its visit box joins
// the launch's and its pointers join `align`.  stim_args_finish: the launch visits the union of the boxes — false: planes that
// leave every cell untouched, nothing to visit —, four cells per thread (`vec`) where the slab allows it
static void stim_args_begin(StimArgs &a)
{
    memset(&a, 0, sizeof a);
    a.r0 = a.c0 = INT_MAX;
}
static StimDue &stim_args_add(const fibhip_ctx *h, const StimEntry &e, float *planes, StimArgs &a, size_t i, uintptr_t &align)
{
    StimDue &d = a.e[i];
    stim_due_fill(h, e, planes, d);
    align |= reinterpret_cast<uintptr_t>(d.x) | reinterpret_cast<uintptr_t>(d.plane);
    if (e.b_r0 < e.b_r1) {
        a.r0 = imin(a.r0, e.b_r0); a.r1 = imax(a.r1, e.b_r1);
        a.c0 = imin(a.c0, e.b_c0); a.c1 = imax(a.c1, e.b_c1);
    }
    return d;
}
static bool stim_args_finish(const fibhip_ctx *h, StimArgs &a, int n, uintptr_t align, bool behind_mt, bool &vec, dim3 &grid)
{
    if (a.r0 >= a.r1) return false;
    const int W = h->d.width;
    a.n = n;
    a.W = W;
    a.pitch = h->pitch;
    a.give_up = give_up_of(h, behind_mt);
    vec = rows_vec_ok(h, align);
    if (vec) {
        a.c0 = a.c0 / 4 * 4;
        a.c1 = (a.c1 + 3) / 4 * 4;                                  // (<= W: W is a multiple of 4)
    }
    grid = blocks_of((size_t)(a.r1 - a.r0) * (size_t)((a.c1 - a.c0) / (vec ? 4 : 1)));
    return true;
}

static_assert(STIM_MAX_DUE <= FIBHIP_MAX_STIM_ENTRIES && (int)STIM_MAX == (int)FIBHIP_STIM_MAX && (int)STIM_ADD == (int)FIBHIP_STIM_ADD,
              "stim_kernel's constants follow include/fibhip.h");
// The stimulus program's hook behind a launch of `ticks` ticks (plain: commit_impl; multi-tick: mt_launch), behind the samples of
// that tick.  No launch spans an event tick (stim_room), so the entries due are those of the tick the counter has landed on.
// They go out in program order, grouped by array (stable: see stim_kernel), STIM_MAX_DUE per launch, on s0 behind the launch
// that ended there — WITHOUT confirming it.  `behind_mt`: that launch is a multi-tick launch, which nobody may have confirmed:
// stim_kernel is then handed the give-up word and writes nothing once a launch in front of it gave up, so the state such a
// launch started from stays intact; recover() rewinds the counter and the replay comes through here again.  Behind a PLAIN tick
// the kernel gets no word: every plain tick is issued behind a confirmed stream, and the device's word has a life of its own
// outside multi-tick launches (an autotune candidate that gave up leaves it raised until the next mt_launch zeroes it,
// plan.inc) — a stimulus must not be dropped for that.  What is due follows from the host's counter alone: nothing about the
// program lives on the device but the planes.
static int stim_advance(fibhip_ctx *h, int ticks, bool behind_mt)
{
    StimRec &r = h->stim;
    r.k += ticks;
    if (r.k < r.next) return 0;                                     // (no launch spans an event tick: k lands on it or stays below)
    std::vector<const StimEntry *> due;
    for (const StimEntry &e : r.entries)
        if (stim_due(e, r.k)) due.push_back(&e);
    r.next = stim_next(r);
    if (due.empty()) return 0;
    std::stable_sort(due.begin(), due.end(), [](const StimEntry *a, const StimEntry *b) { return a->var < b->var; });
    for (size_t first = 0; first < due.size(); first += STIM_MAX_DUE) {
        const size_t n = due.size() - first < (size_t)STIM_MAX_DUE ? due.size() - first : (size_t)STIM_MAX_DUE;
        StimArgs a;
        stim_args_begin(a);
        uintptr_t align = 0;
        for (size_t i = 0; i < n; ++i) {
            const StimEntry &e = *due[first + i];
            StimDue &d = stim_args_add(h, e, r.planes, a, i, align);
            d.load = i == 0 || due[first + i - 1]->var != e.var;
            d.store = i + 1 == n || due[first + i + 1]->var != e.var;
            if (e.slow && h->use_agg) h->agg_dirty = true;          // as fibhip_set_state: the next tick forms the aggregates afresh
        }
        bool vec;
        dim3 grid;
        if (!stim_args_finish(h, a, (int)n, align, behind_mt, vec, grid)) continue;
        if (int rc = launch_traced(h, "stim_kernel", 0, [&] {
                if (vec) hipLaunchKernelGGL(stim_kernel<true>, grid, dim3(256), 0, h->s0, a);
                else hipLaunchKernelGGL(stim_kernel<false>, grid, dim3(256), 0, h->s0, a);
            }))
            return rc;
    }
    return 0;
}
static void stim_free(fibhip_ctx *h)
{
    dev_free(h->stim.planes);
    h->stim.entries.clear();
    h->stim.on = false;
}

// The lesions `due` (boxes validated at attach; `patches`: the device buffer their offsets index), applied IN ORDER to the phase
// field and the derived planes recomputed around them: lesion_apply_kernel, LESION_MAX_DUE entries per launch, then
// lesion_prep_kernel for the same entries — what the program's hook and fibhip_lesion_apply share.  The launch shape comes
// from the boxes: entries whose boxes overlap, directly or through others, form a cluster (grid.y; a cell's entries are all in
// one cluster, which is what keeps their order), grid.x covers the largest cluster's bounding box; the prep launch has one
// grid.y per entry's dilated box.  A lesion is a few hundred to a few thousand cells: what costs is the two launches.
static int lesion_launch(fibhip_ctx *h, const std::vector<const LesionEntry *> &due, const float *patches, bool behind_mt)
{
    const int H = h->d.height, W = h->d.width;
    for (int pass = 0; pass < 2; ++pass)
        for (size_t first = 0; first < due.size(); first += LESION_MAX_DUE) {
            const int n = (int)(due.size() - first < (size_t)LESION_MAX_DUE ? due.size() - first : (size_t)LESION_MAX_DUE);
            LesionArgs a;
            memset(&a, 0, sizeof a);
            a.n = n;
            a.give_up = give_up_of(h, behind_mt);
            int root[LESION_MAX_DUE];
            for (int i = 0; i < n; ++i) {
                const LesionEntry &e = *due[first + i];
                a.e[i].patch = patches + e.off;
                a.e[i].r0 = e.r0; a.e[i].r1 = e.r1; a.e[i].c0 = e.c0; a.e[i].c1 = e.c1;
                root[i] = i;
            }
            size_t most = 0;
            if (pass == 0) {
                // clusters: the classes of "the boxes share a cell" (n <= 8: merged until nothing moves)
                for (bool moved = true; moved;) {
                    moved = false;
                    for (int i = 0; i < n; ++i)
                        for (int j = 0; j < i; ++j) {
                            const LesionDue &p = a.e[i], &q = a.e[j];
                            if (root[i] != root[j] && p.r0 < q.r1 && q.r0 < p.r1 && p.c0 < q.c1 && q.c0 < p.c1) {
                                const int from = imax(root[i], root[j]), to = imin(root[i], root[j]);
                                for (int k = 0; k < n; ++k)
                                    if (root[k] == from) root[k] = to;
                                moved = true;
                            }
                        }
                }
                for (int i = 0; i < n; ++i) {
                    if (root[i] != i) continue;
                    LesionBox &b = a.box[a.nbox++];
                    b.r0 = H; b.c0 = W; b.r1 = b.c1 = 0;
                    for (int k = 0; k < n; ++k)
                        if (root[k] == i) {
                            b.r0 = imin(b.r0, a.e[k].r0); b.r1 = imax(b.r1, a.e[k].r1);
                            b.c0 = imin(b.c0, a.e[k].c0); b.c1 = imax(b.c1, a.e[k].c1);
                            b.member |= 1u << k;
                        }
                }
            } else {
                for (int i = 0; i < n; ++i) {
                    LesionBox &b = a.box[a.nbox++];
                    b.r0 = imax(a.e[i].r0 - 1, 0); b.r1 = imin(a.e[i].r1 + 1, H);
                    b.c0 = imax(a.e[i].c0 - 1, 0); b.c1 = imin(a.e[i].c1 + 1, W);
                }
            }
            for (int c = 0; c < a.nbox; ++c) {
                const size_t area = (size_t)(a.box[c].r1 - a.box[c].r0) * (size_t)(a.box[c].c1 - a.box[c].c0);
                if (area > most) most = area;
            }
            const dim3 grid(blocks_of(most).x, (unsigned)a.nbox);
            if (pass == 0) {
                if (int rc = launch_traced(h, "lesion_apply_kernel", 0, [&] {
                        hipLaunchKernelGGL(lesion_apply_kernel, grid, dim3(256), 0, h->s0, a, h->phi_dev, W);
                    }))
                    return rc;
            } else {
                const Geo g = base_geo(h);
                float *p3 = h->phase3;
                const size_t cells = h->cells;
                if (int rc = launch_traced(h, "lesion_prep_kernel", 0, [&] {
                        hipLaunchKernelGGL(lesion_prep_kernel, grid, dim3(256), 0, h->s0, a, g, (const float *)h->phi_dev, p3, p3 + cells,
                                           p3 + 2 * cells, p3 + 3 * cells, p3 + 4 * cells, p3 + 5 * cells);
                    }))
                    return rc;
            }
        }
    return 0;
}
// The lesion program's hook behind a launch of `ticks` ticks, the LAST hook of the tick (recorders.hpp says why).  No launch
// spans an event tick (lesion_room), so the entries due are those of the tick the counter has landed on, in program order.
// `behind_mt`: as for stim_advance — the apply is handed the give-up word and writes nothing once a launch in front of it gave
// up; behind a plain tick, which stands behind a confirmed stream, it gets no word.  What is due follows from the host's counter
// alone: nothing about the program lives on the device but the patches.
static int lesion_advance(fibhip_ctx *h, int ticks, bool behind_mt)
{
    LesionRec &r = h->les;
    r.k += ticks;
    if (r.k < r.next) return 0;                                     // (no launch spans an event tick: k lands on it or stays below)
    std::vector<const LesionEntry *> due;
    for (const LesionEntry &e : r.entries)
        if (e.tick + 1 == r.k) due.push_back(&e);
    r.next = lesion_next(r);
    if (due.empty()) return 0;
    return lesion_launch(h, due, r.patches, behind_mt);
}
static void lesion_free(fibhip_ctx *h)
{
    dev_free(h->les.patches);
    h->les.entries.clear();
    h->les.on = false;
}

static_assert(TRIG_MAX == FIBHIP_MAX_TRIG_SENSORS && TRIG_MAX == FIBHIP_MAX_TRIG_RULES && TRIG_MAX <= STIM_MAX_DUE && TRIG_ROW == FIBHIP_TRIG_ROW &&
                  (int)TRIG_RISE == (int)FIBHIP_TRIG_RISE && (int)TRIG_FALL == (int)FIBHIP_TRIG_FALL && SENSE_MAX_CHUNKS == 4 * 64 &&
                  SENSE_MIN_CHUNK % SENSE_THREADS == 0,
              "the trigger kernels' constants follow include/fibhip.h; trigger_kernel folds four chunks per lane of one wave");
// The trigger program's hook behind a launch of `ticks` ticks, behind the samples and the programmed stimuli of that tick.  At a
// sample tick three launches go out on s0 behind the launch that ended there, WITHOUT confirming it: sense_kernel (one partial
// count per sensor and chunk), trigger_kernel (row s of the log and the fire mask of sample s) and the gated apply (the rules'
// stimuli, all by value; entry r is rule r's).  The slot s is a kernel argument computed from the host's counter, so a replay
// (recover()) writes the same rows again.  `behind_mt`: as for stim_advance — the gated apply is handed the give-up word and
// writes nothing once a launch in front of it gave up.
static int trig_advance(fibhip_ctx *h, int ticks, bool behind_mt)
{
    TrigRec &r = h->trig;
    long long s;
    if (!r.advance(ticks, &s)) return 0;
    if (s >= r.cap) return fail(FIBHIP_EINVAL, "trigger program: log full");                    // (fibhip_step refuses before this)
    SenseArgs a;
    a.slab0 = h->slab[0];
    a.slab1 = h->slab[1];
    a.cur_mask = 0u;
    uintptr_t align = reinterpret_cast<uintptr_t>(r.masks);
    for (int i = 0; i < r.nsensors; ++i) {
        const int v = r.vars[i];
        if (h->cur[v]) a.cur_mask |= 1u << v;
        align |= reinterpret_cast<uintptr_t>(array_of(h, v));
    }
    a.W = h->d.width;
    a.pitch = h->pitch;
    a.vstride = h->vstride;
    a.cells = h->cells;
    a.sites = r.sites;
    a.masks = r.masks;
    a.part = r.part;
    const bool vec = r.cut_vec && (align & 15u) == 0;
    const dim3 sgrid((unsigned)r.max_chunks[vec], (unsigned)r.nsensors);
    if (int rc = launch_traced(h, vec ? "sense_kernel<true>" : "sense_kernel<false>", 0, [&] {
            if (vec) hipLaunchKernelGGL(sense_kernel<true>, sgrid, dim3(SENSE_THREADS), 0, h->s0, a);
            else hipLaunchKernelGGL(sense_kernel<false>, sgrid, dim3(SENSE_THREADS), 0, h->s0, a);
        }))
        return rc;
    if (int rc = launch_traced(h, "trigger_kernel", 0, [&] {
            hipLaunchKernelGGL(trigger_kernel, dim3(1), dim3(256), 0, h->s0, r.sites, r.nsensors, vec ? 1 : 0, r.part, r.rules, r.nrules, r.rows,
                               r.fire, (int)s);
        }))
        return rc;
    // the gated apply: the union of the rules' visit boxes, every sample (its workgroups leave after two scalar loads when no
    // rule fires)
    StimArgs g;
    stim_args_begin(g);
    uintptr_t galign = 0;
    for (int i = 0; i < r.nrules; ++i) {
        StimDue &d = stim_args_add(h, r.stims[i], r.planes, g, (size_t)i, galign);
        d.load = d.store = 1;
    }
    bool gvec;
    dim3 grid;
    if (!stim_args_finish(h, g, r.nrules, galign, behind_mt, gvec, grid)) return 0;
    return launch_traced(h, gvec ? "stim_gated_kernel<true>" : "stim_gated_kernel<false>", 0, [&] {
        if (gvec) hipLaunchKernelGGL(stim_gated_kernel<true>, grid, dim3(256), 0, h->s0, g, (const unsigned *)(r.fire + s));
        else hipLaunchKernelGGL(stim_gated_kernel<false>, grid, dim3(256), 0, h->s0, g, (const unsigned *)(r.fire + s));
    });
}
static void trig_free(fibhip_ctx *h)
{
    TrigRec &r = h->trig;
    dev_free(r.sites);
    dev_free(r.rules);
    dev_free(r.masks);
    dev_free(r.planes);
    dev_free(r.part);
    dev_free(r.rows);
    dev_free(r.fire);
    r.stims.clear();
    r.on = false;
}

// ---- the entry points ---------------------------------------------------------------------------------------------------
// ---- activation recorder ------------------------------------------------------------------------------------------------
extern "C" int fibhip_observe_begin(fibhip_t h, int var, float up, float down)
{
    NEED(h);
    if (int rc = var_check(var, h->nvar, "observe_begin")) return rc;
    if (std::isnan(up) || std::isnan(down) || down > up)
        return fail(FIBHIP_EINVAL, "observe_begin: thresholds must be numbers with down <= up (got up %g, down %g)", up, down);
    if (int rc = attach_ready(h, "observe_begin", nullptr)) return rc;     // (the planes are kept from attach to attach: nothing to release)
    const size_t n = h->cells;
    if (!h->obs.buf) HIPCHK(hipMalloc((void **)&h->obs.buf, 6 * n * sizeof(float)));
    HIPCHK(hipMemcpy2DAsync(h->obs.buf, (size_t)h->d.width * sizeof(float), array_of(h, var), (size_t)h->pitch * sizeof(float),
                            (size_t)h->d.width * sizeof(float), (size_t)h->d.height, hipMemcpyDeviceToDevice, h->s0));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(h->obs.buf + n), (int)qnan_bits(), 4 * n, h->s0));   // first | last | prev | apd
    HIPCHK(hipMemsetAsync(h->obs.buf + 5 * n, 0, n * sizeof(int), h->s0));                      // count
    h->obs.on = true;
    h->obs.var = var;
    h->obs.up = up;
    h->obs.down = down;
    h->obs.k = 0;
    return 0;
}

extern "C" int fibhip_observe_get(fibhip_t h, int which, void *dst)
{
    NEED(h);
    FLUSH(h);
    if (!h->obs.on) return fail(FIBHIP_EINVAL, "observe_get: no recorder attached (fibhip_observe_begin)");
    if (!dst || which < 0 || which > FIBHIP_OBS_COUNT) return fail(FIBHIP_EINVAL, "observe_get: bad argument (which %d)", which);
    if (!h->stage) HIPCHK(hipHostMalloc((void **)&h->stage, h->cells * sizeof(float), hipHostMallocDefault));
    HIPCHK(hipMemcpyAsync(h->stage, h->obs.buf + (size_t)(1 + which) * h->cells, h->cells * sizeof(float), hipMemcpyDeviceToHost, h->s0));
    SYNC_S0(h);
    memcpy(dst, h->stage, h->cells * sizeof(float));
    return 0;
}

extern "C" int fibhip_observe_ticks(fibhip_t h, long long *k)
{
    if (!h || !k) return fail(FIBHIP_EINVAL, "observe_ticks: null argument");
    if (!h->obs.on) return fail(FIBHIP_EINVAL, "observe_ticks: no recorder attached (fibhip_observe_begin)");
    *k = h->obs.k + h->pending;                        // (ticks accepted but not launched yet are observed when they are)
    return 0;
}

extern "C" int fibhip_observe_end(fibhip_t h)
{
    NEED(h);
    FLUSH(h);                                          // the ticks accepted while attached are observed
    if (h->obs.buf) {
        HIPCHK(wait_stream(h->s0));
        HIPCHK(hipFree(h->obs.buf));
        h->obs.buf = nullptr;
    }
    if (h->obs.vel) {                                  // (fibhip_observe_velocity's maps: every call waited for its own copies)
        HIPCHK(hipFree(h->obs.vel));
        h->obs.vel = nullptr;
    }
    h->obs.on = false;
    return 0;
}

// ---- electrode recorder -------------------------------------------------------------------------------------------------
extern "C" int fibhip_electrode_begin(fibhip_t h, int var, int n, const int *rects, const float *weights, int every, long long capacity)
{
    NEED(h);
    if (!rects || !weights) return fail(FIBHIP_EINVAL, "electrode_begin: null argument");
    if (int rc = var_check(var, h->nvar, "electrode_begin")) return rc;
    if (n < 1 || n > FIBHIP_MAX_ELECTRODES) return fail(FIBHIP_EINVAL, "electrode_begin: 1 .. %d electrodes (got %d)", FIBHIP_MAX_ELECTRODES, n);
    if (int rc = every_check("electrode_begin", every)) return rc;
    if (int rc = capacity_check("electrode_begin", capacity, (size_t)n * sizeof(float))) return rc;
    // the chunk table: one chunk per patch of up to EL_CHUNK cells, larger patches in at most 256 equal chunks
    std::vector<ElChunk> chunks;
    std::vector<ElComb> combs;
    size_t woff = 0;
    int nparts = 0;
    const auto cut = [&] {
        for (int e = 0; e < n; ++e) {
            const int r0 = rects[4 * e], r1 = rects[4 * e + 1], c0 = rects[4 * e + 2], c1 = rects[4 * e + 3];
            if (int rc = rect_check(h->d.height, h->d.width, r0, r1, c0, c1, "electrode_begin: electrode %d: ", e)) return rc;
            const size_t m = (size_t)(r1 - r0) * (size_t)(c1 - c0);
            if (woff + m > 0x7FFFFFFFu) return fail(FIBHIP_EINVAL, "electrode_begin: more than 2^31 - 1 weights");
            for (size_t i = 0; i < m; ++i)
                if (!std::isfinite(weights[woff + i])) return fail(FIBHIP_EINVAL, "electrode_begin: electrode %d has a weight that is not finite", e);
            const size_t cs = m <= EL_CHUNK ? m : (m + 255) / 256 > EL_CHUNK ? (m + 255) / 256 : (size_t)EL_CHUNK;
            const int nc = (int)((m + cs - 1) / cs);                   // <= 256
            if (nc > 1) {
                ElComb cb;
                cb.e = e; cb.part0 = nparts; cb.nparts = nc;
                combs.push_back(cb);
            }
            for (int k = 0; k < nc; ++k) {
                ElChunk c;
                c.r0 = r0; c.c0 = c0; c.pw = c1 - c0;
                c.first = (unsigned)((size_t)k * cs);
                c.count = (unsigned)((size_t)(k + 1) * cs <= m ? cs : m - (size_t)k * cs);
                c.woff = (unsigned)woff;
                c.out = nc > 1 ? -1 - nparts++ : e;
                chunks.push_back(c);
            }
            woff += m;
        }
        return 0;
    };
    if (int rc = attach_ready(h, "electrode_begin", electrode_free, cut)) return rc;    // (the rectangles are looked at behind attach_refusals)
    Attach a(h);
    a.upload(h->el.chunks, chunks.size(), chunks.data());
    a.upload(h->el.w, woff, weights);
    a.alloc(h->el.trace, (size_t)capacity * (size_t)n, Attach::ZERO);
    if (nparts) {
        a.upload(h->el.comb, combs.size(), combs.data());
        a.alloc(h->el.part, (size_t)nparts);
    }
    if (a.failed(electrode_free))
        return fail(FIBHIP_ENOMEM, "electrode_begin: hipMalloc of the recorder's buffers failed (%lld samples of %d electrodes)", capacity, n);
    if (int rc = a.finish()) return rc;                // `chunks`, `combs` and the caller's arrays are free again
    h->el.on = true;
    h->el.start(every, capacity);
    h->el.before_slow = slow_array(var);
    h->el.var = var;
    h->el.n = n;
    h->el.nchunks = (int)chunks.size();
    h->el.ncomb = (int)combs.size();
    return 0;
}

extern "C" int fibhip_electrode_count(fibhip_t h, long long *samples)
{
    NEED(h);
    return sampler_count(h, h->el, "electrode_count", "fibhip_electrode_begin", samples);
}

extern "C" int fibhip_electrode_read(fibhip_t h, long long first, long long count, float *dst)
{
    NEED(h);
    if (int rc = need_attached(h->el.on, "electrode_read", "fibhip_electrode_begin")) return rc;
    return ranged_read(h, h->el, "electrode_read", "samples", first, count, {{dst, h->el.trace, h->el.n * sizeof(float)}});
}

extern "C" int fibhip_electrode_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->el.on, electrode_free);
}

// ---- tip recorder -------------------------------------------------------------------------------------------------------
extern "C" int fibhip_tips_begin(fibhip_t h, int var, int var2, float a0, float b0, const unsigned char *mask, int every, int max_tips,
                                 long long capacity)
{
    NEED(h);
    if (var < 0 || var >= h->nvar || var2 < 0 || var2 >= h->nvar) return fail(FIBHIP_EINVAL, "tips_begin: bad var %d / %d", var, var2);
    if (var == var2) return fail(FIBHIP_EINVAL, "tips_begin: the two watched arrays must differ (got %d twice)", var);
    if (std::isnan(a0) || std::isnan(b0)) return fail(FIBHIP_EINVAL, "tips_begin: the levels must be numbers");
    if (int rc = every_check("tips_begin", every)) return rc;
    if (max_tips < 1 || max_tips > FIBHIP_MAX_TIPS) return fail(FIBHIP_EINVAL, "tips_begin: 1 .. %d tips per sample (got %d)", FIBHIP_MAX_TIPS, max_tips);
    if (int rc = capacity_check("tips_begin", capacity, (size_t)max_tips * 4 * sizeof(int))) return rc;
    if (int rc = attach_ready(h, "tips_begin", tips_free, [&] {
            if (h->d.height < 2 || h->d.width < 2) return fail(FIBHIP_EINVAL, "tips_begin: a %d x %d grid has no plaquette", h->d.height, h->d.width);
            return 0;
        }))
        return rc;
    Attach a(h);
    a.alloc(h->tip.counts, (size_t)capacity * 3, Attach::ZERO);
    a.alloc(h->tip.records, (size_t)capacity * (size_t)max_tips * 4);
    if (mask) a.upload(h->tip.mask, h->cells, mask);
    if (a.failed(tips_free))
        return fail(FIBHIP_ENOMEM, "tips_begin: hipMalloc of the recorder's buffers failed (%lld samples of %d tips)", capacity, max_tips);
    if (int rc = a.finish()) return rc;                // the caller's mask is free again
    h->tip.on = true;
    h->tip.start(every, capacity);
    h->tip.before_slow = slow_array(var) || slow_array(var2);
    h->tip.var = var;
    h->tip.var2 = var2;
    h->tip.a0 = a0;
    h->tip.b0 = b0;
    h->tip.max_tips = max_tips;
    return 0;
}

extern "C" int fibhip_tips_count(fibhip_t h, long long *samples)
{
    NEED(h);
    return sampler_count(h, h->tip, "tips_count", "fibhip_tips_begin", samples);
}

extern "C" int fibhip_tips_read(fibhip_t h, long long first, long long count, int *counts, int *records)
{
    NEED(h);
    if (int rc = need_attached(h->tip.on, "tips_read", "fibhip_tips_begin")) return rc;
    return ranged_read(h, h->tip, "tips_read", "samples", first, count,
                       {{counts, h->tip.counts, 3 * sizeof(int)}, {records, h->tip.records, (size_t)h->tip.max_tips * 4 * sizeof(int)}});
}

extern "C" int fibhip_tips_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->tip.on, tips_free);
}

// ---- frame recorder -----------------------------------------------------------------------------------------------------
extern "C" int fibhip_frames_begin(fibhip_t h, int var, const int *window, int by, int bx, int reduce, float lo, float span,
                                   const float *weight, int format, int every, int first, long long capacity)
{
    NEED(h);
    if (!window) return fail(FIBHIP_EINVAL, "frames_begin: null window");
    if (int rc = var_check(var, h->nvar, "frames_begin")) return rc;
    Window px;
    if (int rc = window_from(h, "frames_begin", window, by, bx, reduce, px)) return rc;
    const int oh = px.oh, ow = px.ow;
    if (format != FIBHIP_FRAME_F32 && format != FIBHIP_FRAME_U8) return fail(FIBHIP_EINVAL, "frames_begin: bad format %d", format);
    if (std::isnan(lo)) return fail(FIBHIP_EINVAL, "frames_begin: the level lo must be a number");
    if (!std::isfinite(span) || span == 0.f) return fail(FIBHIP_EINVAL, "frames_begin: span must be finite and not zero (got %g)", span);
    if (int rc = every_check("frames_begin", every)) return rc;
    if (first < 1 || first > every) return fail(FIBHIP_EINVAL, "frames_begin: first must be 1 .. every = %d (got %d)", every, first);
    const size_t per = (size_t)oh * (size_t)ow * (format == FIBHIP_FRAME_U8 ? 1u : 4u);
    if (int rc = capacity_check("frames_begin", capacity, per, LLONG_MAX, SIZE_MAX / 2)) return rc;
    if (int rc = attach_ready(h, "frames_begin", frames_free)) return rc;
    static_cast<Window &>(h->fr) = px;
    Attach a(h);
    a.alloc(h->fr.cube, (size_t)capacity * per);       // (not filled: a frame is written whole before it can be read)
    if (weight) a.upload(h->fr.w, h->cells, weight);
    if (a.failed(frames_free))
        return fail(FIBHIP_ENOMEM, "frames_begin: hipMalloc of the cube failed (%lld frames of %d x %d, %zu bytes each)", capacity, oh, ow, per);
    if (int rc = a.finish()) return rc;                // the caller's plane is free again
    h->fr.on = true;
    h->fr.start(every, capacity, every - first);       // sample s follows tick first + s * every, ticks counted from 1 here
    h->fr.before_slow = slow_array(var);
    h->fr.var = var;
    h->fr.format = format;
    h->fr.lo = lo;
    h->fr.span = span;
    return 0;
}

extern "C" int fibhip_frames_count(fibhip_t h, long long *samples)
{
    NEED(h);
    return sampler_count(h, h->fr, "frames_count", "fibhip_frames_begin", samples);
}

extern "C" int fibhip_frames_shape(fibhip_t h, int *oh, int *ow, int *bytes_per_pixel)
{
    if (!h) return fail(FIBHIP_EINVAL, "null handle");
    if (!h->fr.on) return fail(FIBHIP_EINVAL, "frames_shape: no recorder attached (fibhip_frames_begin)");
    if (oh) *oh = h->fr.oh;
    if (ow) *ow = h->fr.ow;
    if (bytes_per_pixel) *bytes_per_pixel = h->fr.format == FIBHIP_FRAME_U8 ? 1 : 4;
    return 0;
}

extern "C" int fibhip_frames_read(fibhip_t h, long long first, long long count, void *dst)
{
    NEED(h);
    if (int rc = need_attached(h->fr.on, "frames_read", "fibhip_frames_begin")) return rc;
    return ranged_read(h, h->fr, "frames_read", "frames", first, count, {{dst, h->fr.cube, h->fr.frame_bytes()}});
}

extern "C" int fibhip_frames_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->fr.on, frames_free);
}

// ---- statistics recorder ------------------------------------------------------------------------------------------------
extern "C" int fibhip_stats_begin(fibhip_t h, int ncols, const fibhip_stat_col *cols, const float *weight, const unsigned char *mask,
                                  int every, long long capacity)
{
    NEED(h);
    if (!cols) return fail(FIBHIP_EINVAL, "stats_begin: null argument");
    if (ncols < 1 || ncols > FIBHIP_MAX_STAT_COLS) return fail(FIBHIP_EINVAL, "stats_begin: 1 .. %d columns (got %d)", FIBHIP_MAX_STAT_COLS, ncols);
    std::vector<StArr> arrs;
    std::vector<StCol> table;
    bool need_w = false, need_m = false;
    for (int c = 0; c < ncols; ++c) {
        const fibhip_stat_col &col = cols[c];
        if (int rc = var_check(col.var, h->nvar, "stats_begin: column %d", c)) return rc;
        if (col.kind < 0 || col.kind >= ST_KINDS) return fail(FIBHIP_EINVAL, "stats_begin: column %d: unknown kind %d", c, col.kind);
        if ((col.kind == FIBHIP_STAT_BELOW || col.kind == FIBHIP_STAT_ABOVE) && std::isnan(col.level))
            return fail(FIBHIP_EINVAL, "stats_begin: column %d: the level must be a number", c);
        size_t a = 0;
        while (a < arrs.size() && arrs[a].var != col.var) ++a;
        if (a == arrs.size()) {
            StArr n;
            memset(&n, 0, sizeof n);
            n.var = col.var;
            arrs.push_back(n);
        }
        StArr &A = arrs[a];
        if (A.ncols == FIBHIP_MAX_STAT_COLS_PER_ARRAY)
            return fail(FIBHIP_EINVAL, "stats_begin: column %d: more than %d columns on array %d", c, FIBHIP_MAX_STAT_COLS_PER_ARRAY, col.var);
        A.kind[A.ncols] = col.kind;
        A.level[A.ncols] = col.level;
        (col.kind == FIBHIP_STAT_SUM ? A.need_w : A.need_m) = 1;
        (col.kind == FIBHIP_STAT_SUM ? need_w : need_m) = true;
        StCol t;
        t.arr = (int)a; t.slot = A.ncols; t.kind = col.kind; t.pad = 0;
        table.push_back(t);
        A.ncols++;
    }
    if (int rc = every_check("stats_begin", every)) return rc;
    if (int rc = capacity_check("stats_begin", capacity, (size_t)ncols * sizeof(double))) return rc;
    if (weight)
        if (int rc = finite_check("stats_begin", weight, (size_t)h->d.height, (size_t)h->d.width, "the weight plane")) return rc;
    // the chunk table, from H, W and the pitch alone: at most ST_MAX_CHUNKS equal chunks of at least ST_MIN_CHUNK cells, a
    // multiple of four cells each where the vector path may run (so that every chunk starts 16-byte aligned there)
    std::vector<StChunk> chunks;
    {
        const size_t n = h->cells;
        size_t cs = (n + ST_MAX_CHUNKS - 1) / ST_MAX_CHUNKS;
        if (cs < ST_MIN_CHUNK) cs = ST_MIN_CHUNK;
        if (h->pitch == h->d.width && h->d.width % 4 == 0) cs = (cs + 3) / 4 * 4;
        for (size_t first = 0; first < n; first += cs) {
            StChunk c;
            c.first = (unsigned)first;
            c.count = (unsigned)(first + cs <= n ? cs : n - first);
            chunks.push_back(c);
        }
    }
    if (int rc = attach_ready(h, "stats_begin", stats_free, [&] {
            if (h->st.on) return fail(FIBHIP_EINVAL, "stats_begin: a recorder is attached already (fibhip_stats_end first)");
            // stats_kernel counts cells in 32 bits, and a thread looks up to one batch beyond its chunk's end before it drops the cell
            if (h->cells > (size_t)UINT_MAX - 4u * ST_VBATCH * ST_THREADS)
                return fail(FIBHIP_EINVAL, "stats_begin: a grid of %zu cells is too large for the recorder's 32-bit cell index", h->cells);
            return 0;
        }))
        return rc;
    StRec &r = h->st;
    Attach a(h);
    a.upload(r.chunks, chunks.size(), chunks.data());
    a.upload(r.arrs, arrs.size(), arrs.data());
    a.upload(r.cols, table.size(), table.data());
    a.alloc(r.part, arrs.size() * ST_SLOTS * chunks.size());
    a.alloc(r.trace, (size_t)capacity * (size_t)ncols, Attach::ZERO);
    if (weight && need_w) a.upload(r.w, h->cells, weight);
    if (mask && need_m) a.upload(r.mask, h->cells, mask);
    if (a.failed(stats_free))
        return fail(FIBHIP_ENOMEM, "stats_begin: hipMalloc of the recorder's buffers failed (%lld samples of %d columns)", capacity, ncols);
    if (int rc = a.finish()) return rc;                // the tables and the caller's planes are free again
    r.on = true;
    r.start(every, capacity);
    r.ncols = ncols;
    r.narr = (int)arrs.size();
    r.before_slow = false;
    for (int a = 0; a < r.narr; ++a) {
        r.vars[a] = arrs[a].var;
        r.before_slow |= slow_array(r.vars[a]);
    }
    r.nchunks = (int)chunks.size();
    return 0;
}

extern "C" int fibhip_stats_count(fibhip_t h, long long *samples)
{
    NEED(h);
    return sampler_count(h, h->st, "stats_count", "fibhip_stats_begin", samples);
}

extern "C" int fibhip_stats_read(fibhip_t h, long long first, long long count, double *dst)
{
    NEED(h);
    if (int rc = need_attached(h->st.on, "stats_read", "fibhip_stats_begin")) return rc;
    return ranged_read(h, h->st, "stats_read", "samples", first, count, {{dst, h->st.trace, h->st.ncols * sizeof(double)}});
}

extern "C" int fibhip_stats_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->st.on, stats_free);
}

// ---- lead recorder ------------------------------------------------------------------------------------------------------
// does the handle's diffusion term use the zero-padded convolution Laplacian (fenton_simple.py)?
static inline bool zero_padded(const fibhip_ctx *h)
{
    if (h->d.flags & FIBHIP_ZEROPAD) return true;
#ifdef FIB_CUSTOM_MODEL_INC
    if (h->d.model == FIBHIP_CUSTOM && !h->mod && ZeroPadOf<Custom>::value) return true;
#endif
    return false;
}

extern "C" int fibhip_leads_begin(fibhip_t h, int var, int n, const int *pos, int ntables, const float *tables, const float *weight, int every,
                                  long long capacity)
{
    NEED(h);
    if (!pos || !tables) return fail(FIBHIP_EINVAL, "leads_begin: null argument");
    if (int rc = var_check(var, h->nvar, "leads_begin")) return rc;
    if (n < 1 || n > FIBHIP_MAX_LEADS) return fail(FIBHIP_EINVAL, "leads_begin: 1 .. %d leads (got %d)", FIBHIP_MAX_LEADS, n);
    if (ntables < 1 || ntables > FIBHIP_MAX_LEAD_TABLES)
        return fail(FIBHIP_EINVAL, "leads_begin: 1 .. %d lead-field tables (got %d)", FIBHIP_MAX_LEAD_TABLES, ntables);
    if (int rc = every_check("leads_begin", every)) return rc;
    if (int rc = capacity_check("leads_begin", capacity, (size_t)n * sizeof(double))) return rc;
    const int H = h->d.height, W = h->d.width;
    if (H < 3 || W < 3) return fail(FIBHIP_EINVAL, "leads_begin: a %d x %d grid has no interior cell", H, W);
    if (zero_padded(h))
        return fail(FIBHIP_EINVAL, "leads_begin: not on a model with the zero-padded Laplacian (FIBHIP_ZEROPAD): its diffusion term is not this source");
    if (h->has_tensor)
        return fail(FIBHIP_EINVAL, "leads_begin: not on a handle with a diffusion tensor (fibhip_set_tensor): its diffusion term is not this source");
    std::vector<int> table(4 * (size_t)n);
    for (int e = 0; e < n; ++e) {
        const int r = pos[3 * e], c = pos[3 * e + 1], t = pos[3 * e + 2];
        if (r < 0 || r >= H || c < 0 || c >= W) return fail(FIBHIP_EINVAL, "leads_begin: lead %d: cell (%d, %d) is outside the %d x %d grid", e, r, c, H, W);
        if (t < 0 || t >= ntables) return fail(FIBHIP_EINVAL, "leads_begin: lead %d: table %d of %d", e, t, ntables);
        table[4 * e] = r; table[4 * e + 1] = c; table[4 * e + 2] = t; table[4 * e + 3] = 0;
    }
    for (int t = 0; t < ntables; ++t)
        if (int rc = finite_check("leads_begin", tables + (size_t)t * h->cells, (size_t)H, (size_t)W, "table %d", t)) return rc;
    if (weight)
        if (int rc = finite_check("leads_begin", weight, (size_t)H, (size_t)W, "the weight plane")) return rc;
    if (int rc = attach_ready(h, "leads_begin", leads_free)) return rc;
    LeadRec &r = h->ld;
    const int tiles_x = (W + LD_TX - 1) / LD_TX, tiles_y = (H + LD_TY - 1) / LD_TY;
    Attach a(h);
    a.upload(r.pos, table.size(), table.data());
    a.upload(r.tables, (size_t)ntables * h->cells, tables);
    a.alloc(r.part, (size_t)n * (size_t)tiles_x * (size_t)tiles_y);
    a.alloc(r.rows, (size_t)capacity * (size_t)n, Attach::ZERO);
    if (weight) a.upload(r.weight, h->cells, weight);
    if (a.failed(leads_free))
        return fail(FIBHIP_ENOMEM, "leads_begin: hipMalloc of the recorder's buffers failed (%lld samples of %d leads, %d tables)", capacity, n, ntables);
    if (int rc = a.finish()) return rc;                // `table` and the caller's arrays are free again
    r.on = true;
    r.start(every, capacity);
    r.before_slow = slow_array(var);
    r.var = var;
    r.n = n;
    r.tiles_x = tiles_x;
    r.tiles_y = tiles_y;
    return 0;
}

extern "C" int fibhip_leads_count(fibhip_t h, long long *samples)
{
    NEED(h);
    return sampler_count(h, h->ld, "leads_count", "fibhip_leads_begin", samples);
}

extern "C" int fibhip_leads_read(fibhip_t h, long long first, long long count, double *dst)
{
    NEED(h);
    if (int rc = need_attached(h->ld.on, "leads_read", "fibhip_leads_begin")) return rc;
    return ranged_read(h, h->ld, "leads_read", "samples", first, count, {{dst, h->ld.rows, h->ld.n * sizeof(double)}});
}

extern "C" int fibhip_leads_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->ld.on, leads_free);
}

// ---- potential-map recorder ---------------------------------------------------------------------------------------------
extern "C" int fibhip_pmap_begin(fibhip_t h, int var, int radius, const float *table, const float *weight, const int *window, int sy, int sx,
                                 int every, long long capacity)
{
    NEED(h);
    if (!table || !window) return fail(FIBHIP_EINVAL, "pmap_begin: null argument");
    if (int rc = var_check(var, h->nvar, "pmap_begin")) return rc;
    if (radius < 1 || radius > FIBHIP_PMAP_MAX_RADIUS)
        return fail(FIBHIP_EINVAL, "pmap_begin: radius must be 1 .. %d (got %d)", FIBHIP_PMAP_MAX_RADIUS, radius);
    if (sy < 1 || sy > FIBHIP_PMAP_MAX_STEP || sx < 1 || sx > FIBHIP_PMAP_MAX_STEP)
        return fail(FIBHIP_EINVAL, "pmap_begin: a step is 1 .. %d cells each way (got %d x %d)", FIBHIP_PMAP_MAX_STEP, sy, sx);
    if (int rc = every_check("pmap_begin", every)) return rc;
    const int H = h->d.height, W = h->d.width, R = radius, K = 2 * R + 1;
    if (H < 3 || W < 3) return fail(FIBHIP_EINVAL, "pmap_begin: a %d x %d grid has no interior cell", H, W);
    if (int rc = rect_check(h->d.height, h->d.width, window[0], window[1], window[2], window[3], "pmap_begin: the window ")) return rc;
    const int r0 = window[0], c0 = window[2], oh = (window[1] - r0 + sy - 1) / sy, ow = (window[3] - c0 + sx - 1) / sx;
    const size_t npix = (size_t)oh * (size_t)ow;
    if (int rc = capacity_check("pmap_begin", capacity, npix * sizeof(double), INT_MAX)) return rc;
    if (zero_padded(h))
        return fail(FIBHIP_EINVAL, "pmap_begin: not on a model with the zero-padded Laplacian (FIBHIP_ZEROPAD): its diffusion term is not this source");
    if (h->has_tensor)
        return fail(FIBHIP_EINVAL, "pmap_begin: not on a handle with a diffusion tensor (fibhip_set_tensor): its diffusion term is not this source");
    if (int rc = finite_check("pmap_begin", table, (size_t)R + 1, (size_t)R + 1, "the table")) return rc;
    if (weight)
        if (int rc = finite_check("pmap_begin", weight, (size_t)H, (size_t)W, "the weight plane")) return rc;
    // the table's rows as pmap_conv_kernel walks them: float64, dc = -R .. R
    std::vector<double> tab((size_t)(R + 1) * K);
    for (int a = 0; a <= R; ++a)
        for (int x = 0; x < K; ++x) tab[(size_t)a * K + x] = (double)table[a * (R + 1) + std::abs(x - R)];
    if (int rc = attach_ready(h, "pmap_begin", pmap_free)) return rc;
    PMapRec &r = h->pm;
    Attach a(h);
    a.alloc(r.cube, (size_t)capacity * npix, Attach::ZERO);
    a.upload(r.tab, tab.size(), tab.data());
    a.alloc(r.q, (size_t)(H + 2 * R) * (size_t)(W + 2 * R), Attach::ZERO);      // (the border stays: the kernel writes the grid's cells only)
    a.alloc_bytes(r.maps, npix * (3 * sizeof(double) + 3 * sizeof(int)));
    if (weight) a.upload(r.weight, h->cells, weight);
    if (a.failed(pmap_free))
        return fail(FIBHIP_ENOMEM, "pmap_begin: hipMalloc of the recorder's buffers failed (%lld samples of %d x %d sites)", capacity, oh, ow);
    if (int rc = a.finish()) return rc;                // `tab` and the caller's arrays are free again
    r.on = true;
    r.start(every, capacity);
    r.before_slow = slow_array(var);
    r.var = var;
    r.R = R;
    r.r0 = r0; r.c0 = c0; r.sy = sy; r.sx = sx; r.oh = oh; r.ow = ow;
    r.pw = PM_TX - 1 + (K + sx - 1) / sx;              // ceil(((PM_TX - 1) * sx + K) / sx)
    r.roww = sx * r.pw;
    r.slab = PM_LDS_FLOATS / r.roww;
    return 0;
}

extern "C" int fibhip_pmap_count(fibhip_t h, long long *samples)
{
    NEED(h);
    return sampler_count(h, h->pm, "pmap_count", "fibhip_pmap_begin", samples);
}

extern "C" int fibhip_pmap_read(fibhip_t h, long long first, long long count, double *dst)
{
    NEED(h);
    if (int rc = need_attached(h->pm.on, "pmap_read", "fibhip_pmap_begin")) return rc;
    return ranged_read(h, h->pm, "pmap_read", "samples", first, count, {{dst, h->pm.cube, h->pm.npix() * sizeof(double)}});
}

extern "C" int fibhip_pmap_summary(fibhip_t h, long long first, long long count, double *vmin, double *vmax, double *dmin, int *kmin, int *kmax,
                                   int *kd)
{
    NEED(h);
    if (!h->pm.on) return fail(FIBHIP_EINVAL, "pmap_summary: no recorder attached (fibhip_pmap_begin)");
    FLUSH(h);
    if (int rc = range_check("pmap_summary", "samples", first, count, h->pm.taken())) return rc;
    if (count < 2) return fail(FIBHIP_EINVAL, "pmap_summary: a summary takes at least 2 samples (got %lld)", count);
    const PMapRec &r = h->pm;
    const size_t npix = r.npix();
    PMapSummaryArgs a;
    a.cube = r.cube;
    a.npix = npix;
    a.first = (int)first; a.count = (int)count;
    a.vmin = r.maps; a.vmax = r.maps + npix; a.dmin = r.maps + 2 * npix;
    a.kmin = reinterpret_cast<int *>(r.maps + 3 * npix); a.kmax = a.kmin + npix; a.kd = a.kmin + 2 * npix;
    void *const dst[6] = {vmin, vmax, dmin, kmin, kmax, kd};
    const void *const src[6] = {a.vmin, a.vmax, a.dmin, a.kmin, a.kmax, a.kd};
    // the samples read are confirmed ones when the copies are taken: a launch that gave up in front is recovered and the kernel
    // runs again (read_confirmed), as for beats_summary
    return read_confirmed(h, [&] {
        if (int rc = launch_traced(h, "pmap_summary_kernel", 0, [&] { hipLaunchKernelGGL(pmap_summary_kernel, blocks_of(npix), dim3(256), 0, h->s0, a); }))
            return rc;
        for (int i = 0; i < 6; ++i)
            if (dst[i]) HIPCHK(hipMemcpyAsync(dst[i], src[i], npix * (i < 3 ? sizeof(double) : sizeof(int)), hipMemcpyDeviceToHost, h->s0));
        return 0;
    });
}

extern "C" int fibhip_pmap_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->pm.on, pmap_free);
}

// ---- wave recorder ------------------------------------------------------------------------------------------------------
extern "C" int fibhip_waves_begin(fibhip_t h, int var, int kind, float level, int var2, int kind2, float level2, int conn,
                                  const unsigned char *mask, int max_waves, int every, long long capacity)
{
    NEED(h);
    if (int rc = var_check(var, h->nvar, "waves_begin")) return rc;
    if (var2 < -1 || var2 >= h->nvar) return fail(FIBHIP_EINVAL, "waves_begin: bad var2 %d (-1: none)", var2);
    if (kind != FIBHIP_WAVE_ABOVE && kind != FIBHIP_WAVE_BELOW) return fail(FIBHIP_EINVAL, "waves_begin: bad kind %d", kind);
    if (!std::isfinite(level)) return fail(FIBHIP_EINVAL, "waves_begin: the level must be finite");
    if (var2 >= 0) {
        if (kind2 != FIBHIP_WAVE_ABOVE && kind2 != FIBHIP_WAVE_BELOW) return fail(FIBHIP_EINVAL, "waves_begin: bad kind2 %d", kind2);
        if (!std::isfinite(level2)) return fail(FIBHIP_EINVAL, "waves_begin: level2 must be finite");
    }
    if (conn != 4 && conn != 8) return fail(FIBHIP_EINVAL, "waves_begin: conn is 4 or 8 (got %d)", conn);
    if (max_waves < 1 || max_waves > FIBHIP_MAX_WAVES)
        return fail(FIBHIP_EINVAL, "waves_begin: 1 .. %d waves per sample (got %d)", FIBHIP_MAX_WAVES, max_waves);
    if (int rc = every_check("waves_begin", every)) return rc;
    if (int rc = capacity_check("waves_begin", capacity, (size_t)max_waves * sizeof(WaveRecord))) return rc;
    if (int rc = attach_ready(h, "waves_begin", waves_free)) return rc;
    WaveRec &r = h->wv;
    Attach a(h);
    a.alloc(r.counts, (size_t)capacity * 3, Attach::ZERO);
    a.alloc(r.records, (size_t)capacity * (size_t)max_waves);
    a.alloc(r.labels, h->cells, Attach::ONES);
    a.alloc(r.slots, h->cells, Attach::ONES);
    if (mask) a.upload(r.mask, h->cells, mask);
    if (a.failed(waves_free))
        return fail(FIBHIP_ENOMEM, "waves_begin: hipMalloc of the recorder's buffers failed (%lld samples of %d waves)", capacity, max_waves);
    if (int rc = a.finish()) return rc;                // the caller's mask is free again
    r.on = true;
    r.start(every, capacity);
    r.before_slow = slow_array(var) || (var2 >= 0 && slow_array(var2));
    r.var = var; r.kind = kind; r.level = level;
    r.var2 = var2; r.kind2 = kind2; r.level2 = level2;
    r.conn = conn;
    r.max_waves = max_waves;
    return 0;
}

extern "C" int fibhip_waves_count(fibhip_t h, long long *samples)
{
    NEED(h);
    return sampler_count(h, h->wv, "waves_count", "fibhip_waves_begin", samples);
}

extern "C" int fibhip_waves_read(fibhip_t h, long long first, long long count, int *counts, fibhip_wave_record *records)
{
    NEED(h);
    if (int rc = need_attached(h->wv.on, "waves_read", "fibhip_waves_begin")) return rc;
    return ranged_read(h, h->wv, "waves_read", "samples", first, count,
                       {{counts, h->wv.counts, 3 * sizeof(int)}, {records, h->wv.records, (size_t)h->wv.max_waves * sizeof(WaveRecord)}});
}

extern "C" int fibhip_waves_links_begin(fibhip_t h, int max_links)
{
    NEED(h);
    WaveRec &r = h->wv;
    if (int rc = need_attached(r.on, "waves_links_begin", "fibhip_waves_begin")) return rc;
    if (r.max_links) return fail(FIBHIP_EINVAL, "waves_links_begin: links are on already (%d per sample)", r.max_links);
    if (max_links < 1 || max_links > FIBHIP_MAX_WAVE_LINKS)
        return fail(FIBHIP_EINVAL, "waves_links_begin: 1 .. %d links per sample (got %d)", FIBHIP_MAX_WAVE_LINKS, max_links);
    if (r.cap > (long long)(SIZE_MAX / sizeof(WaveLink) / (size_t)max_links))
        return fail(FIBHIP_EINVAL, "waves_links_begin: %lld samples of %d links do not fit", r.cap, max_links);
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "waves_links_begin inside an open tick");
    // sample s links to sample s - 1: links start with the recorder or not at all
    if (r.k != 0 || h->pending != 0)
        return fail(FIBHIP_EINVAL, "waves_links_begin: the recorder has seen ticks already (%lld launched, %lld pending): call it right behind fibhip_waves_begin",
                    r.k, (long long)h->pending);
    SYNC_S0(h);
    unsigned T = 4;
    while (T < 4u * (unsigned)max_links) T <<= 1;
    Attach a(h);
    a.alloc(r.prev, h->cells, Attach::ONES);
    a.alloc_bytes(r.link_table, (size_t)T * (sizeof(unsigned long long) + sizeof(int)));
    a.alloc(r.link_counts, (size_t)r.cap * 4, Attach::ZERO);
    a.alloc(r.link_records, (size_t)r.cap * (size_t)max_links);
    if (a.failed(wave_links_free))                     // (the wave recorder stays attached, without links)
        return fail(FIBHIP_ENOMEM, "waves_links_begin: hipMalloc of the link buffers failed (%lld samples of %d links)", r.cap, max_links);
    if (int rc = a.finish()) return rc;
    r.max_links = max_links;
    r.link_entries = T;
    return 0;
}

extern "C" int fibhip_waves_links_read(fibhip_t h, long long first, long long count, int *counts, fibhip_wave_link *links)
{
    NEED(h);
    if (int rc = need_attached(h->wv.on, "waves_links_read", "fibhip_waves_begin")) return rc;
    if (!h->wv.max_links) return fail(FIBHIP_EINVAL, "waves_links_read: links are off (fibhip_waves_links_begin)");
    return ranged_read(h, h->wv, "waves_links_read", "samples", first, count,
                       {{counts, h->wv.link_counts, 4 * sizeof(int)}, {links, h->wv.link_records, (size_t)h->wv.max_links * sizeof(WaveLink)}});
}

extern "C" int fibhip_waves_labels(fibhip_t h, int *dst)
{
    NEED(h);
    if (!h->wv.on) return fail(FIBHIP_EINVAL, "waves_labels: no recorder attached (fibhip_waves_begin)");
    if (!dst) return fail(FIBHIP_EINVAL, "waves_labels: null destination");
    FLUSH(h);
    if (h->wv.taken() < 1) return fail(FIBHIP_EINVAL, "waves_labels: no sample has been taken yet");
    return read_confirmed(h, [&] {
        HIPCHK(hipMemcpyAsync(dst, h->wv.labels, h->cells * sizeof(int), hipMemcpyDeviceToHost, h->s0));
        return 0;
    });
}

extern "C" int fibhip_waves_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->wv.on, waves_free);
}

// ---- spectrum recorder --------------------------------------------------------------------------------------------------
extern "C" int fibhip_spectrum_begin(fibhip_t h, int var, const int *window, int by, int bx, int reduce, const float *weight, int every,
                                     int nfft, const float *win, const float *tw, int nb, const int *bins, int chunk)
{
    NEED(h);
    if (!window || !win || !tw || !bins) return fail(FIBHIP_EINVAL, "spectrum_begin: null argument");
    if (int rc = var_check(var, h->nvar, "spectrum_begin")) return rc;
    Window px;
    if (int rc = window_from(h, "spectrum_begin", window, by, bx, reduce, px)) return rc;
    const int oh = px.oh, ow = px.ow;
    if (int rc = every_check("spectrum_begin", every)) return rc;
    if (nfft < FIBHIP_SPECTRUM_MIN_NFFT || nfft > FIBHIP_SPECTRUM_MAX_NFFT)
        return fail(FIBHIP_EINVAL, "spectrum_begin: nfft must be %d .. %d (got %d)", FIBHIP_SPECTRUM_MIN_NFFT, FIBHIP_SPECTRUM_MAX_NFFT, nfft);
    if (chunk < 1 || chunk > FIBHIP_SPECTRUM_MAX_CHUNK || nfft % chunk)
        return fail(FIBHIP_EINVAL, "spectrum_begin: chunk must be 1 .. %d and divide nfft = %d (got %d)", FIBHIP_SPECTRUM_MAX_CHUNK, nfft, chunk);
    if (nb < 1 || nb > FIBHIP_SPECTRUM_MAX_BINS) return fail(FIBHIP_EINVAL, "spectrum_begin: 1 .. %d bins (got %d)", FIBHIP_SPECTRUM_MAX_BINS, nb);
    for (int i = 0; i < nb; ++i) {
        if (bins[i] < 0 || bins[i] > nfft / 2)
            return fail(FIBHIP_EINVAL, "spectrum_begin: bin %d names frequency index %d outside [0, nfft / 2 = %d]", i, bins[i], nfft / 2);
        if (i > 0 && bins[i] <= bins[i - 1]) return fail(FIBHIP_EINVAL, "spectrum_begin: the bins must be strictly ascending (bin %d)", i);
    }
    if (int rc = attach_ready(h, "spectrum_begin", spectrum_free, [&] {
            if (h->pitch != h->d.width) return fail(FIBHIP_EINVAL, "spectrum_begin: not on a row-interleaved slab");
            if (h->sp.on) return fail(FIBHIP_EINVAL, "spectrum_begin: a recorder is attached already (fibhip_spectrum_end first)");
            return 0;
        }))
        return rc;
    SpRec &r = h->sp;
    static_cast<Window &>(r) = px;
    const size_t npix = px.npix();
    Attach a(h);
    a.alloc(r.ring, (size_t)chunk * npix);
    a.alloc(r.acc, 3 * (size_t)nb * npix, Attach::ZERO);                     // Re = Im = P = +0
    a.alloc(r.maps, 4 * npix);
    a.upload(r.win, (size_t)nfft, win);
    a.upload(r.tw, 2 * (size_t)nfft, tw);
    a.upload(r.bins, (size_t)nb, bins);
    if (weight) a.upload(r.w, h->cells, weight);
    if (a.failed(spectrum_free))
        return fail(FIBHIP_ENOMEM, "spectrum_begin: hipMalloc failed (%d bins and %d ring planes of %d x %d pixels)", nb, chunk, oh, ow);
    if (int rc = a.finish()) return rc;                // the caller's tables are free again
    r.on = true;
    r.start(every, LLONG_MAX);                         // sample s follows tick (s + 1) * every, ticks counted from 1 here
    r.before_slow = slow_array(var);
    r.var = var;
    r.nfft = nfft; r.nb = nb; r.chunk = chunk;
    return 0;
}

extern "C" int fibhip_spectrum_count(fibhip_t h, long long *samples, long long *segments)
{
    NEED(h);
    long long n;
    if (int rc = count_taken(h, h->sp, "spectrum_count", "fibhip_spectrum_begin", "recorder", &n)) return rc;
    if (samples) *samples = n;
    if (segments) *segments = n / h->sp.nfft;
    return 0;
}

extern "C" int fibhip_spectrum_shape(fibhip_t h, int *oh, int *ow, int *nb)
{
    if (!h) return fail(FIBHIP_EINVAL, "null handle");
    if (!h->sp.on) return fail(FIBHIP_EINVAL, "spectrum_shape: no recorder attached (fibhip_spectrum_begin)");
    if (oh) *oh = h->sp.oh;
    if (ow) *ow = h->sp.ow;
    if (nb) *nb = h->sp.nb;
    return 0;
}

extern "C" int fibhip_spectrum_read(fibhip_t h, float *P, long long *segments)
{
    NEED(h);
    if (!h->sp.on) return fail(FIBHIP_EINVAL, "spectrum_read: no recorder attached (fibhip_spectrum_begin)");
    FLUSH(h);
    const SpRec &r = h->sp;
    const size_t plane = (size_t)r.nb * r.npix();
    if (int rc = read_confirmed(h, [&] {
            if (P) HIPCHK(hipMemcpyAsync(P, r.acc + 2 * plane, plane * sizeof(float), hipMemcpyDeviceToHost, h->s0));
            return 0;
        }))
        return rc;
    if (segments) *segments = r.taken() / r.nfft;
    return 0;
}

extern "C" int fibhip_spectrum_peak(fibhip_t h, int a, int b, int halfwidth, int *kpeak, float *ppeak, float *pband, float *pnear)
{
    NEED(h);
    if (!h->sp.on) return fail(FIBHIP_EINVAL, "spectrum_peak: no recorder attached (fibhip_spectrum_begin)");
    const SpRec &r = h->sp;
    if (a < 0 || b < a || b >= r.nb) return fail(FIBHIP_EINVAL, "spectrum_peak: the band is bin positions 0 <= a <= b < %d (got %d, %d)", r.nb, a, b);
    if (halfwidth < 0) return fail(FIBHIP_EINVAL, "spectrum_peak: halfwidth must be >= 0 (got %d)", halfwidth);
    FLUSH(h);
    const size_t npix = r.npix(), plane = (size_t)r.nb * npix;
    void *const dst[4] = {kpeak, ppeak, pband, pnear};
    return read_confirmed(h, [&] {
        const int have = r.taken() / r.nfft > 0 ? 1 : 0;
        if (int rc = launch_traced(h, "spectrum_peak_kernel", 0, [&] {
                hipLaunchKernelGGL(spectrum_peak_kernel, blocks_of(npix), dim3(256), 0, h->s0, (const float *)(r.acc + 2 * plane), npix, a, b,
                                   halfwidth, have, reinterpret_cast<int *>(r.maps), r.maps + npix, r.maps + 2 * npix, r.maps + 3 * npix);
            }))
            return rc;
        return copy_maps(h, r.maps, npix, dst);
    });
}

extern "C" int fibhip_spectrum_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->sp.on, spectrum_free);
}

// ---- beat recorder ------------------------------------------------------------------------------------------------------
extern "C" int fibhip_beats_begin(fibhip_t h, int var, const int *window, int by, int bx, int reduce, const float *weight, int every,
                                  float up, float down, int depth)
{
    NEED(h);
    if (!window) return fail(FIBHIP_EINVAL, "beats_begin: null argument");
    if (int rc = var_check(var, h->nvar, "beats_begin")) return rc;
    Window px;
    if (int rc = window_from(h, "beats_begin", window, by, bx, reduce, px)) return rc;
    const int oh = px.oh, ow = px.ow;
    if (int rc = every_check("beats_begin", every)) return rc;
    if (!(down <= up)) return fail(FIBHIP_EINVAL, "beats_begin: the levels must be numbers with down <= up (got down %g, up %g)", (double)down, (double)up);
    if (depth < 1 || depth > FIBHIP_BEATS_MAX_DEPTH)
        return fail(FIBHIP_EINVAL, "beats_begin: depth must be 1 .. %d (got %d)", FIBHIP_BEATS_MAX_DEPTH, depth);
    if (int rc = attach_ready(h, "beats_begin", beats_free, [&] {
            if (h->pitch != h->d.width) return fail(FIBHIP_EINVAL, "beats_begin: not on a row-interleaved slab");
            if (h->bt.on) return fail(FIBHIP_EINVAL, "beats_begin: a recorder is attached already (fibhip_beats_end first)");
            return 0;
        }))
        return rc;
    BeatRec &r = h->bt;
    static_cast<Window &>(r) = px;
    const size_t npix = px.npix();
    Attach a(h);
    a.alloc(r.state, 3 * npix);                        // xp | pk | n: three planes that start differently, filled below
    a.alloc(r.ring, 3 * (size_t)depth * npix, Attach::QNAN);                  // t_up = t_down = peak = NaN
    a.alloc(r.maps, 4 * npix);
    if (weight) a.upload(r.w, h->cells, weight);
    if (a.failed(beats_free)) return fail(FIBHIP_ENOMEM, "beats_begin: hipMalloc failed (a ring of %d beats of %d x %d pixels)", depth, oh, ow);
    if (int rc = a.enqueue()) return rc;
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(r.state + npix), (int)qnan_bits(), npix, h->s0));   // pk = NaN
    HIPCHK(hipMemsetAsync(r.state + 2 * npix, 0, npix * sizeof(int), h->s0));                    // n = 0
    r.start(every, LLONG_MAX);                         // sample s follows tick (s + 1) * every, ticks counted from 1 here
    r.before_slow = slow_array(var);
    r.var = var;
    r.up = up; r.down = down;
    r.depth = depth;
    if (int rc = beats_launch(h, true, 0, nullptr)) {  // xp = the pixel of the current state (confirmed above: nothing to gate on)
        beats_free(h);
        return rc;
    }
    if (int rc = a.wait()) return rc;                  // the caller's weight plane is free again
    r.on = true;
    return 0;
}

extern "C" int fibhip_beats_count(fibhip_t h, long long *samples)
{
    NEED(h);
    long long n;
    if (int rc = count_taken(h, h->bt, "beats_count", "fibhip_beats_begin", "recorder", &n)) return rc;
    if (samples) *samples = n;
    return 0;
}

extern "C" int fibhip_beats_shape(fibhip_t h, int *oh, int *ow, int *depth)
{
    if (!h) return fail(FIBHIP_EINVAL, "null handle");
    if (!h->bt.on) return fail(FIBHIP_EINVAL, "beats_shape: no recorder attached (fibhip_beats_begin)");
    if (oh) *oh = h->bt.oh;
    if (ow) *ow = h->bt.ow;
    if (depth) *depth = h->bt.depth;
    return 0;
}

extern "C" int fibhip_beats_read(fibhip_t h, float *t_up, float *t_down, float *peak, int *count, float *pk)
{
    NEED(h);
    if (!h->bt.on) return fail(FIBHIP_EINVAL, "beats_read: no recorder attached (fibhip_beats_begin)");
    FLUSH(h);
    const BeatRec &r = h->bt;
    const size_t npix = r.npix(), plane = (size_t)r.depth * npix;
    return read_confirmed(h, [&] {
        if (t_up) HIPCHK(hipMemcpyAsync(t_up, r.ring, plane * sizeof(float), hipMemcpyDeviceToHost, h->s0));
        if (t_down) HIPCHK(hipMemcpyAsync(t_down, r.ring + plane, plane * sizeof(float), hipMemcpyDeviceToHost, h->s0));
        if (peak) HIPCHK(hipMemcpyAsync(peak, r.ring + 2 * plane, plane * sizeof(float), hipMemcpyDeviceToHost, h->s0));
        if (count) HIPCHK(hipMemcpyAsync(count, r.state + 2 * npix, npix * sizeof(int), hipMemcpyDeviceToHost, h->s0));
        if (pk) HIPCHK(hipMemcpyAsync(pk, r.state + npix, npix * sizeof(float), hipMemcpyDeviceToHost, h->s0));
        return 0;
    });
}

extern "C" int fibhip_beats_summary(fibhip_t h, int last, int *nused, float *apd_mean, float *cl_mean, float *apd_alt)
{
    NEED(h);
    if (!h->bt.on) return fail(FIBHIP_EINVAL, "beats_summary: no recorder attached (fibhip_beats_begin)");
    const BeatRec &r = h->bt;
    if (last < 1 || last > r.depth) return fail(FIBHIP_EINVAL, "beats_summary: last must be 1 .. depth = %d (got %d)", r.depth, last);
    FLUSH(h);
    const size_t npix = r.npix(), plane = (size_t)r.depth * npix;
    void *const dst[4] = {nused, apd_mean, cl_mean, apd_alt};
    return read_confirmed(h, [&] {
        if (int rc = launch_traced(h, "beat_summary_kernel", 0, [&] {
                hipLaunchKernelGGL(beat_summary_kernel, blocks_of(npix), dim3(256), 0, h->s0, reinterpret_cast<const int *>(r.state + 2 * npix),
                                   (const float *)r.ring, (const float *)(r.ring + plane), npix, r.depth, last, reinterpret_cast<int *>(r.maps),
                                   r.maps + npix, r.maps + 2 * npix, r.maps + 3 * npix);
            }))
            return rc;
        return copy_maps(h, r.maps, npix, dst);
    });
}

// ---- velocity fit: what fibhip_beats_velocity, fibhip_observe_velocity and fibhip_velocity_fit (unit.inc) share ------------
static_assert(VEL_MAX_RADIUS == FIBHIP_VEL_MAX_RADIUS, "velocity_fit_kernel's LDS tile follows include/fibhip.h");
// the refusals that need no plane; `who` names the function
static int vel_refusals(const char *who, int depth, int back, int radius, float max_dt, int min_cells)
{
    if (depth < 1 || depth > FIBHIP_BEATS_MAX_DEPTH) return fail(FIBHIP_EINVAL, "%s: depth must be 1 .. %d (got %d)", who, FIBHIP_BEATS_MAX_DEPTH, depth);
    if (back < 0 || back >= depth) return fail(FIBHIP_EINVAL, "%s: back must be 0 .. depth - 1 = %d (got %d)", who, depth - 1, back);
    if (radius < 1 || radius > FIBHIP_VEL_MAX_RADIUS)
        return fail(FIBHIP_EINVAL, "%s: radius must be 1 .. %d (got %d)", who, FIBHIP_VEL_MAX_RADIUS, radius);
    if (!std::isfinite(max_dt) || !(max_dt > 0.f)) return fail(FIBHIP_EINVAL, "%s: max_dt must be finite and > 0 (got %g)", who, (double)max_dt);
    const int window = (2 * radius + 1) * (2 * radius + 1);
    if (min_cells < 3 || min_cells > window)
        return fail(FIBHIP_EINVAL, "%s: min_cells must be 3 .. (2 * radius + 1)^2 = %d (got %d)", who, window, min_cells);
    return 0;
}
static inline VelArgs vel_args(const float *t, const int *n, const unsigned char *mask, int depth, int oh, int ow, int back, int radius,
                               float max_dt, int min_cells, float *maps)
{
    const size_t npix = (size_t)oh * (size_t)ow;
    VelArgs a;
    a.t = t; a.n = n; a.mask = mask;
    a.depth = depth; a.oh = oh; a.ow = ow;
    a.back = back; a.radius = radius; a.min_cells = min_cells;
    a.max_dt = max_dt;
    a.nfit = reinterpret_cast<int *>(maps);
    a.gy = maps + npix; a.gx = maps + 2 * npix; a.rms = maps + 3 * npix;
    return a;
}
static inline dim3 vel_grid(int oh, int ow) { return dim3((unsigned)((ow + VEL_TX - 1) / VEL_TX), (unsigned)((oh + VEL_TY - 1) / VEL_TY)); }
static inline void vel_launch(const VelArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(velocity_fit_kernel, vel_grid(a.oh, a.ow), dim3(256), 0, st, a);
}
// the fit on planes of the handle, behind whatever is pending: the caller's mask goes up for the call, the four maps come back
// through read_confirmed — the planes read are confirmed ones, like beats_summary's
static int vel_on_handle(fibhip_ctx *h, const char *who, const float *t, const int *n, int depth, int oh, int ow, int back, int radius,
                         float max_dt, int min_cells, const unsigned char *mask, float *maps, void *const dst[4])
{
    const size_t npix = (size_t)oh * (size_t)ow;
    unsigned char *dmask = nullptr;
    if (mask) {
        if (hipMalloc((void **)&dmask, npix) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FIBHIP_ENOMEM, "%s: hipMalloc failed (a mask of %d x %d pixels)", who, oh, ow);
        }
        if (hipMemcpyAsync(dmask, mask, npix, hipMemcpyHostToDevice, h->s0) != hipSuccess) {
            hipFree(dmask);
            return fail(FIBHIP_EHIP, "%s: the mask's copy to the device failed", who);
        }
    }
    const VelArgs a = vel_args(t, n, dmask, depth, oh, ow, back, radius, max_dt, min_cells, maps);
    const int rc = read_confirmed(h, [&] {
        if (int rc = launch_traced(h, "velocity_fit_kernel", 0, [&] { vel_launch(a, h->s0); })) return rc;
        return copy_maps(h, maps, npix, dst);
    });
    if (dmask) hipFree(dmask);                         // (read_confirmed waited for the stream; after a failure hipFree waits itself)
    return rc;
}

extern "C" int fibhip_beats_velocity(fibhip_t h, int back, int radius, float max_dt, int min_cells, const unsigned char *mask, int *nfit,
                                     float *gy, float *gx, float *rms)
{
    NEED(h);
    if (!h->bt.on) return fail(FIBHIP_EINVAL, "beats_velocity: no recorder attached (fibhip_beats_begin)");
    const BeatRec &r = h->bt;
    if (int rc = vel_refusals("beats_velocity", r.depth, back, radius, max_dt, min_cells)) return rc;
    FLUSH(h);
    void *const dst[4] = {nfit, gy, gx, rms};
    return vel_on_handle(h, "beats_velocity", r.ring, reinterpret_cast<const int *>(r.state + 2 * r.npix()), r.depth, r.oh, r.ow, back, radius,
                         max_dt, min_cells, mask, r.maps, dst);
}

extern "C" int fibhip_observe_velocity(fibhip_t h, int which, int radius, float max_dt, int min_cells, const unsigned char *mask, int *nfit,
                                       float *gy, float *gx, float *rms)
{
    NEED(h);
    if (!h->obs.on) return fail(FIBHIP_EINVAL, "observe_velocity: no recorder attached (fibhip_observe_begin)");
    if (which != FIBHIP_OBS_FIRST_UP && which != FIBHIP_OBS_LAST_UP && which != FIBHIP_OBS_PREV_UP)
        return fail(FIBHIP_EINVAL, "observe_velocity: which must be FIRST_UP, LAST_UP or PREV_UP (got %d)", which);
    if (int rc = vel_refusals("observe_velocity", 1, 0, radius, max_dt, min_cells)) return rc;
    FLUSH(h);
    const size_t n = h->cells;
    if (!h->obs.vel && hipMalloc((void **)&h->obs.vel, 4 * n * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        h->obs.vel = nullptr;
        return fail(FIBHIP_ENOMEM, "observe_velocity: hipMalloc failed (four maps of %d x %d cells)", h->d.height, h->d.width);
    }
    void *const dst[4] = {nfit, gy, gx, rms};
    return vel_on_handle(h, "observe_velocity", h->obs.buf + (size_t)(1 + which) * n, reinterpret_cast<const int *>(h->obs.buf + 5 * n), 1,
                         h->d.height, h->d.width, 0, radius, max_dt, min_cells, mask, h->obs.vel, dst);
}

extern "C" int fibhip_beats_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->bt.on, beats_free);
}

// ---- stimulus program ---------------------------------------------------------------------------------------------------
extern "C" int fibhip_stim_begin(fibhip_t h, int n, const fibhip_stim_entry *entries, int nplanes, const float *planes)
{
    NEED(h);
    if (!entries) return fail(FIBHIP_EINVAL, "stim_begin: null argument");
    if (n < 1 || n > FIBHIP_MAX_STIM_ENTRIES) return fail(FIBHIP_EINVAL, "stim_begin: 1 .. %d entries (got %d)", FIBHIP_MAX_STIM_ENTRIES, n);
    if (nplanes < 0 || nplanes > FIBHIP_MAX_STIM_PLANES || (nplanes > 0 && !planes))
        return fail(FIBHIP_EINVAL, "stim_begin: 0 .. %d planes (got %d%s)", FIBHIP_MAX_STIM_PLANES, nplanes, nplanes > 0 && !planes ? ", null" : "");
    std::vector<StimEntry> list;
    for (int i = 0; i < n; ++i) {
        const fibhip_stim_entry &s = entries[i];
        StimEntry e;
        memset(&e, 0, sizeof e);
        if (s.first < 0) return fail(FIBHIP_EINVAL, "stim_begin: entry %d: first must be >= 0 (got %d)", i, s.first);
        if (s.hold < 1) return fail(FIBHIP_EINVAL, "stim_begin: entry %d: hold must be >= 1 (got %d)", i, s.hold);
        if (s.period < 0 || s.count < 0) return fail(FIBHIP_EINVAL, "stim_begin: entry %d: period and count must be >= 0 (got %d, %d)", i, s.period, s.count);
        if (s.period == 0 && s.count != 1) return fail(FIBHIP_EINVAL, "stim_begin: entry %d: period 0 means one event: count must be 1 (got %d)", i, s.count);
        if (s.period > 0 && s.hold > s.period) return fail(FIBHIP_EINVAL, "stim_begin: entry %d: hold %d > period %d", i, s.hold, s.period);
        e.first = s.first; e.period = s.period; e.count = s.count; e.hold = s.hold;
        if (int rc = stim_entry_from(h, "stim_begin", "entry", i, s.var, s.mode, s.shape, s.r0, s.r1, s.c0, s.c1, s.v, s.floor, s.plane, nplanes, planes, e))
            return rc;
        list.push_back(e);
    }
    if (int rc = attach_ready(h, "stim_begin", stim_free, [&] {
            if (h->stim.on) return fail(FIBHIP_EINVAL, "stim_begin: a program is attached already (fibhip_stim_end first)");
            return 0;
        }))
        return rc;
    Attach a(h);
    if (nplanes > 0) a.upload(h->stim.planes, (size_t)nplanes * h->cells, planes);
    if (a.failed(stim_free)) return fail(FIBHIP_ENOMEM, "stim_begin: hipMalloc of %d planes failed", nplanes);
    if (int rc = a.finish()) return rc;                // the caller's planes are free again
    h->stim.entries.swap(list);
    h->stim.k = 0;
    h->stim.next = stim_next(h->stim);
    h->stim.on = true;
    return 0;
}

extern "C" int fibhip_stim_count(fibhip_t h, long long *applied)
{
    NEED(h);
    if (!applied) return fail(FIBHIP_EINVAL, "stim_count: null argument");
    if (!h->stim.on) return fail(FIBHIP_EINVAL, "stim_count: no program attached (fibhip_stim_begin)");
    FLUSH(h);                                          // the ticks accepted so far are launched, their events applied
    long long total = 0;
    for (const StimEntry &e : h->stim.entries) total += stim_events_upto(e, h->stim.k);
    *applied = total;
    return 0;
}

extern "C" int fibhip_stim_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->stim.on, stim_free);
}

// ---- trigger program ----------------------------------------------------------------------------------------------------
extern "C" int fibhip_trig_begin(fibhip_t h, int nsensors, const fibhip_trig_sensor *sensors, const unsigned char *masks, int nrules,
                                 const fibhip_trig_rule *rules, int nplanes, const float *planes, int every, long long capacity)
{
    NEED(h);
    if (!sensors || !rules) return fail(FIBHIP_EINVAL, "trig_begin: null argument");
    if (nsensors < 1 || nsensors > FIBHIP_MAX_TRIG_SENSORS)
        return fail(FIBHIP_EINVAL, "trig_begin: 1 .. %d sensors (got %d)", FIBHIP_MAX_TRIG_SENSORS, nsensors);
    if (nrules < 1 || nrules > FIBHIP_MAX_TRIG_RULES) return fail(FIBHIP_EINVAL, "trig_begin: 1 .. %d rules (got %d)", FIBHIP_MAX_TRIG_RULES, nrules);
    if (nplanes < 0 || nplanes > FIBHIP_MAX_STIM_PLANES || (nplanes > 0 && !planes))
        return fail(FIBHIP_EINVAL, "trig_begin: 0 .. %d planes (got %d%s)", FIBHIP_MAX_STIM_PLANES, nplanes, nplanes > 0 && !planes ? ", null" : "");
    if (int rc = every_check("trig_begin", every)) return rc;
    if (int rc = capacity_check("trig_begin", capacity, (size_t)nrules * TRIG_ROW * sizeof(int), INT_MAX)) return rc;
    const int H = h->d.height, W = h->d.width;
    if (h->cells > (size_t)INT_MAX) return fail(FIBHIP_EINVAL, "trig_begin: a grid of %zu cells is too large for the 32-bit counts", h->cells);
    const bool cut_vec = h->pitch == W && W % 4 == 0;
    std::vector<SenseSite> sites;
    int nmasks = 0, max_chunks[2] = {1, 1}, vars[TRIG_MAX] = {0};
    for (int i = 0; i < nsensors; ++i) {
        const fibhip_trig_sensor &q = sensors[i];
        SenseSite d;
        memset(&d, 0, sizeof d);
        if (int rc = var_check(q.var, h->nvar, "trig_begin: sensor %d", i)) return rc;
        if (std::isnan(q.level)) return fail(FIBHIP_EINVAL, "trig_begin: sensor %d: the level must be a number", i);
        long long cells_of_site = 0;
        if (q.site == FIBHIP_TRIG_RECT) {
            if (int rc = rect_check(h->d.height, h->d.width, q.r0, q.r1, q.c0, q.c1, "trig_begin: sensor %d: ", i)) return rc;
            d.r0 = q.r0; d.r1 = q.r1; d.c0 = q.c0; d.c1 = q.c1;
            d.mask = -1;
            cells_of_site = (long long)(q.r1 - q.r0) * (q.c1 - q.c0);
        } else if (q.site == FIBHIP_TRIG_MASK) {
            if (!masks) return fail(FIBHIP_EINVAL, "trig_begin: sensor %d: a mask site without masks", i);
            const unsigned char *m = masks + (size_t)nmasks * h->cells;
            int r0 = H, r1 = 0, c0 = W, c1 = 0;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (m[(size_t)y * W + x]) {
                        r0 = imin(r0, y); r1 = imax(r1, y + 1);
                        c0 = imin(c0, x); c1 = imax(c1, x + 1);
                        ++cells_of_site;
                    }
            if (cells_of_site == 0) return fail(FIBHIP_EINVAL, "trig_begin: sensor %d: the mask holds no cell", i);
            d.r0 = r0; d.r1 = r1; d.c0 = c0; d.c1 = c1;
            d.mask = nmasks++;
        } else {
            return fail(FIBHIP_EINVAL, "trig_begin: sensor %d: unknown site kind %d", i, q.site);
        }
        if (q.need < 1 || q.need > cells_of_site)
            return fail(FIBHIP_EINVAL, "trig_begin: sensor %d: need must be 1 .. %lld, the cells of the site (got %d)", i, cells_of_site, q.need);
        d.var = q.var; d.level = q.level; d.need = q.need;
        vars[i] = q.var;
        for (int v = 0; v < 2; ++v) {
            const unsigned per_row = v ? (unsigned)(((d.c1 + 3) / 4 * 4 - d.c0 / 4 * 4) / 4) : (unsigned)(d.c1 - d.c0);
            const unsigned items = (unsigned)(d.r1 - d.r0) * per_row;
            unsigned pc = (items + SENSE_MAX_CHUNKS - 1) / SENSE_MAX_CHUNKS;
            pc = (pc + SENSE_THREADS - 1) / SENSE_THREADS * SENSE_THREADS;
            if (pc < SENSE_MIN_CHUNK) pc = SENSE_MIN_CHUNK;
            d.per_row[v] = per_row; d.items[v] = items; d.per_chunk[v] = pc;
            d.nchunks[v] = (int)((items + pc - 1) / pc);                // (<= SENSE_MAX_CHUNKS: pc >= items / SENSE_MAX_CHUNKS)
            max_chunks[v] = imax(max_chunks[v], d.nchunks[v]);
        }
        sites.push_back(d);
    }
    std::vector<TrigRule> table;
    std::vector<StimEntry> stims;
    for (int i = 0; i < nrules; ++i) {
        const fibhip_trig_rule &q = rules[i];
        if (q.sensor < 0 || q.sensor >= nsensors) return fail(FIBHIP_EINVAL, "trig_begin: rule %d: sensor %d of %d", i, q.sensor, nsensors);
        if (q.edge != FIBHIP_TRIG_RISE && q.edge != FIBHIP_TRIG_FALL) return fail(FIBHIP_EINVAL, "trig_begin: rule %d: unknown edge %d", i, q.edge);
        const int times[] = {q.arm, q.blank, q.escape, q.max_det, q.delay, q.period};
        for (int t : times)
            if (t < 0 || t > FIBHIP_TRIG_MAX_TIME)
                return fail(FIBHIP_EINVAL, "trig_begin: rule %d: arm, blank, escape, max_det, delay and period must be 0 .. %d", i, FIBHIP_TRIG_MAX_TIME);
        if (q.count < 1 || q.count > FIBHIP_TRIG_MAX_TIME || q.hold < 1 || q.hold > FIBHIP_TRIG_MAX_TIME)
            return fail(FIBHIP_EINVAL, "trig_begin: rule %d: count and hold must be >= 1 (got %d, %d)", i, q.count, q.hold);
        if (q.period == 0 && q.count != 1) return fail(FIBHIP_EINVAL, "trig_begin: rule %d: period 0 means one pulse: count must be 1 (got %d)", i, q.count);
        if (q.period > 0 && q.hold > q.period) return fail(FIBHIP_EINVAL, "trig_begin: rule %d: hold %d > period %d", i, q.hold, q.period);
        const long long train = (long long)q.delay + (long long)(q.count - 1) * q.period + q.hold;
        if ((long long)q.blank < train)
            return fail(FIBHIP_EINVAL, "trig_begin: rule %d: blank %d is too short: a train must not be cut by a new detection, blank >= delay + (count - 1) * period + hold = %lld",
                        i, q.blank, train);
        TrigRule k = {q.sensor, q.edge, q.arm, q.blank, q.escape, q.max_det, q.delay, q.count, q.period, q.hold};
        table.push_back(k);
        // the stimulus: the stimulus program's rules for an entry
        StimEntry e;
        memset(&e, 0, sizeof e);
        if (int rc = stim_entry_from(h, "trig_begin", "rule", i, q.var, q.mode, q.shape, q.r0, q.r1, q.c0, q.c1, q.v, q.floor, q.plane, nplanes, planes, e))
            return rc;
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
        // the host cannot know when a rule fires, so it cannot mark the aggregates stale: on a handle that runs on them a rule's
        // stimulus names one of the four fast arrays
        if (h->use_agg && h->d.model == FIBHIP_COURT && !((Courtemanche::FAST_MASK >> q.var) & 1u))
            return fail(FIBHIP_EINVAL, "trig_begin: rule %d: array %d is one of the slow arrays the aggregates are formed from (a triggered stimulus "
                        "cannot name it on a handle that runs on aggregates)", i, q.var);
#endif
        stims.push_back(e);
    }
    if (int rc = attach_ready(h, "trig_begin", trig_free, [&] {
            if (h->trig.on) return fail(FIBHIP_EINVAL, "trig_begin: a program is attached already (fibhip_trig_end first)");
            return 0;
        }))
        return rc;
    TrigRec &r = h->trig;
    Attach a(h);
    a.upload(r.sites, sites.size(), sites.data());
    a.upload(r.rules, table.size(), table.data());
    a.alloc(r.part, (size_t)nsensors * SENSE_MAX_CHUNKS, Attach::ZERO);
    a.alloc(r.rows, (size_t)capacity * (size_t)nrules * TRIG_ROW, Attach::ZERO);
    a.alloc(r.fire, (size_t)capacity, Attach::ZERO);
    if (nmasks > 0) a.upload(r.masks, (size_t)nmasks * h->cells, masks);
    if (nplanes > 0) a.upload(r.planes, (size_t)nplanes * h->cells, planes);
    if (a.failed(trig_free))
        return fail(FIBHIP_ENOMEM, "trig_begin: hipMalloc of the program's buffers failed (%lld samples of %d rules)", capacity, nrules);
    if (int rc = a.finish()) return rc;                // the tables and the caller's masks and planes are free again
    r.on = true;
    r.start(every, capacity);
    r.before_slow = true;                              // tick, sense / stimulus, slow: whatever arrays it names
    r.nsensors = nsensors;
    r.nrules = nrules;
    r.cut_vec = cut_vec;
    r.max_chunks[0] = max_chunks[0];
    r.max_chunks[1] = max_chunks[1];
    memcpy(r.vars, vars, sizeof vars);
    r.stims.swap(stims);
    return 0;
}

extern "C" int fibhip_trig_count(fibhip_t h, long long *samples)
{
    NEED(h);
    return sampler_count(h, h->trig, "trig_count", "fibhip_trig_begin", samples, "program");
}

extern "C" int fibhip_trig_read(fibhip_t h, long long first, long long count, int *dst)
{
    NEED(h);
    if (int rc = need_attached(h->trig.on, "trig_read", "fibhip_trig_begin", "program")) return rc;
    return ranged_read(h, h->trig, "trig_read", "samples", first, count, {{dst, h->trig.rows, (size_t)h->trig.nrules * TRIG_ROW * sizeof(int)}});
}

extern "C" int fibhip_trig_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->trig.on, trig_free);
}

// ---- lesion program -----------------------------------------------------------------------------------------------------
static_assert(LESION_MAX_DUE <= FIBHIP_MAX_LESION_ENTRIES, "lesion_apply_kernel's constants follow include/fibhip.h");
// what no lesion is applied to: a row block, an open tick, a model without a phase term
static int lesion_refusals(const fibhip_ctx *h, const char *who)
{
    if (int rc = attach_refusals(h, who)) return rc;
    if (zero_padded(h))
        return fail(FIBHIP_EINVAL, "%s: not on a model with the zero-padded Laplacian (FIBHIP_ZEROPAD): its diffusion term has no phase field", who);
    if (h->has_tensor)
        return fail(FIBHIP_EINVAL, "%s: not on a handle with a diffusion tensor (fibhip_set_tensor): a lesion recomputes the phase planes, which hold the tensor's there", who);
    return 0;
}
// one lesion's box and factors: the box inside the grid and not empty, every factor finite and in [0, 1]
static int lesion_check(const fibhip_ctx *h, const char *who, int i, int r0, int r1, int c0, int c1, const float *patch)
{
    if (int rc = rect_check(h->d.height, h->d.width, r0, r1, c0, c1, "%s: entry %d: ", who, i)) return rc;
    const size_t n = (size_t)(r1 - r0) * (size_t)(c1 - c0);
    for (size_t j = 0; j < n; ++j)
        if (!(patch[j] >= 0.0f && patch[j] <= 1.0f))                // (a NaN fails both compares)
            return fail(FIBHIP_EINVAL, "%s: entry %d: factor %zu of the patch is %g: every factor is finite and in [0, 1]", who, i, j, (double)patch[j]);
    return 0;
}
// The field a lesion multiplies into: a handle without one is given a field of ones first, through fibhip_set_phase (the kernels
// switch to their phase variants from then on: the one visible effect of attaching to a model without a field); and the identity
// with add_hole_to_phase_field's whole-plane update needs phi >= 1e-5f everywhere beforehand — checked once per field
// (fibhip_set_phase resets the mark).  Behind a FLUSH and a confirmed stream.
static int lesion_field_ready(fibhip_ctx *h, const char *who)
{
    if (!h->has_phase) {
        const std::vector<float> ones(h->cells, 1.0f);
        if (int rc = fibhip_set_phase(h, ones.data())) return rc;
    }
    if (h->phi_floored) return 0;
    std::vector<float> phi(h->cells);
    HIPCHK(hipMemcpyAsync(phi.data(), h->phi_dev, h->cells * sizeof(float), hipMemcpyDeviceToHost, h->s0));
    HIPCHK(wait_stream(h->s0));
    for (size_t j = 0; j < h->cells; ++j)
        if (!(phi[j] >= LESION_FLOOR))
            return fail(FIBHIP_EINVAL, "%s: the phase field is %g at row %zu, column %zu: a lesion needs a field that is >= 1e-5 everywhere", who,
                        (double)phi[j], j / (size_t)h->d.width, j % (size_t)h->d.width);
    h->phi_floored = true;
    return 0;
}

extern "C" int fibhip_lesion_begin(fibhip_t h, int n, const fibhip_lesion_entry *entries, long long nfloats, const float *patches)
{
    NEED(h);
    if (!entries || !patches) return fail(FIBHIP_EINVAL, "lesion_begin: null argument");
    if (n < 1 || n > FIBHIP_MAX_LESION_ENTRIES) return fail(FIBHIP_EINVAL, "lesion_begin: 1 .. %d entries (got %d)", FIBHIP_MAX_LESION_ENTRIES, n);
    const long long budget = (long long)FIBHIP_MAX_STIM_PLANES * (long long)h->cells;
    if (nfloats < 1 || nfloats > budget)
        return fail(FIBHIP_EINVAL, "lesion_begin: 1 .. %lld floats of patches (%d planes of the grid; got %lld)", budget, FIBHIP_MAX_STIM_PLANES, nfloats);
    if (int rc = lesion_refusals(h, "lesion_begin")) return rc;
    std::vector<LesionEntry> list;
    for (int i = 0; i < n; ++i) {
        const fibhip_lesion_entry &s = entries[i];
        if (s.tick < 0) return fail(FIBHIP_EINVAL, "lesion_begin: entry %d: tick must be >= 0 (got %d)", i, s.tick);
        if (s.reserved != 0) return fail(FIBHIP_EINVAL, "lesion_begin: entry %d: the reserved field must be 0 (got %d)", i, s.reserved);
        if (int rc = rect_check(h->d.height, h->d.width, s.r0, s.r1, s.c0, s.c1, "lesion_begin: entry %d: ", i)) return rc;
        const long long area = (long long)(s.r1 - s.r0) * (long long)(s.c1 - s.c0);
        if (s.offset < 0 || s.offset + area > nfloats)
            return fail(FIBHIP_EINVAL, "lesion_begin: entry %d: a patch of %lld floats at offset %lld of %lld", i, area, s.offset, nfloats);
        if (int rc = lesion_check(h, "lesion_begin", i, s.r0, s.r1, s.c0, s.c1, patches + s.offset)) return rc;
        LesionEntry e;
        e.tick = s.tick;
        e.r0 = s.r0; e.r1 = s.r1; e.c0 = s.c0; e.c1 = s.c1;
        e.off = (size_t)s.offset;
        list.push_back(e);
    }
    if (h->les.on) return fail(FIBHIP_EINVAL, "lesion_begin: a program is attached already (fibhip_lesion_end first)");
    // attach_ready's step, written out: this program's refusals stand in front of its entries, and it confirms as well —
    // everything accepted so far runs on the old geometry, and the field is looked at and maybe made behind a confirmed stream
    FLUSH(h);
    CONFIRM(h);
    SYNC_S0(h);
    if (int rc = lesion_field_ready(h, "lesion_begin")) return rc;
    lesion_free(h);
    Attach a(h);
    a.upload(h->les.patches, (size_t)nfloats, patches);
    if (a.failed(lesion_free)) return fail(FIBHIP_ENOMEM, "lesion_begin: hipMalloc of %lld floats of patches failed", nfloats);
    if (int rc = a.finish()) return rc;                // the caller's patches are free again
    h->les.entries.swap(list);
    h->les.k = 0;
    h->les.next = lesion_next(h->les);
    h->les.on = true;
    return 0;
}

extern "C" int fibhip_lesion_count(fibhip_t h, long long *applied)
{
    NEED(h);
    if (!applied) return fail(FIBHIP_EINVAL, "lesion_count: null argument");
    if (!h->les.on) return fail(FIBHIP_EINVAL, "lesion_count: no program attached (fibhip_lesion_begin)");
    SYNC_S0(h);                                        // (a launch that gave up is recovered before anybody counts on its events)
    const long long k = h->les.k + h->pending;         // (ticks accepted but not launched yet get their events when they are)
    long long total = 0;
    for (const LesionEntry &e : h->les.entries) total += e.tick + 1 <= k;
    *applied = total;
    return 0;
}

extern "C" int fibhip_lesion_end(fibhip_t h)
{
    NEED(h);
    return detach(h, h->les.on, lesion_free);
}

// One lesion NOW, at the state the caller has reached — with or without a program, beside every recorder: what a host-side
// closed loop uses (read the tips, ablate there).  The pending ticks run on the old geometry first and are confirmed (a host
// write never stands behind an unconfirmed launch: the rule above confirm()), so the kernels get no give-up word.
extern "C" int fibhip_lesion_apply(fibhip_t h, const int *box, const float *patch)
{
    NEED(h);
    if (!box || !patch) return fail(FIBHIP_EINVAL, "lesion_apply: null argument");
    if (int rc = lesion_refusals(h, "lesion_apply")) return rc;
    if (int rc = lesion_check(h, "lesion_apply", 0, box[0], box[1], box[2], box[3], patch)) return rc;
    FLUSH(h);
    CONFIRM(h);
    if (int rc = lesion_field_ready(h, "lesion_apply")) return rc;
    LesionEntry e;
    e.tick = 0;
    e.r0 = box[0]; e.r1 = box[1]; e.c0 = box[2]; e.c1 = box[3];
    e.off = 0;
    const size_t bytes = (size_t)(e.r1 - e.r0) * (size_t)(e.c1 - e.c0) * sizeof(float);
    float *dev = nullptr;
    if (hipMalloc((void **)&dev, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FIBHIP_ENOMEM, "lesion_apply: hipMalloc of %zu bytes failed", bytes);
    }
    int rc = hipMemcpyAsync(dev, patch, bytes, hipMemcpyHostToDevice, h->s0) == hipSuccess ? 0 : fail(FIBHIP_EHIP, "lesion_apply: the upload failed");
    if (!rc) rc = lesion_launch(h, std::vector<const LesionEntry *>(1, &e), dev, false);
    if (!rc) rc = sync_s0(h);
    else (void)hipStreamSynchronize(h->s0);
    hipFree(dev);
    return rc;
}

// the current phase field as [H][W].  A reader: it synchronises behind its copy and takes the copy again when a recovery
// happened in between (the events of the replayed ticks are applied again by then)
extern "C" int fibhip_get_phase(fibhip_t h, float *dst)
{
    NEED(h);
    if (!dst) return fail(FIBHIP_EINVAL, "get_phase: null destination");
    if (!h->has_phase) return fail(FIBHIP_EINVAL, "get_phase: the handle has no phase field (fibhip_set_phase)");
    FLUSH(h);
    return read_confirmed(h, [&] {
        HIPCHK(hipMemcpyAsync(dst, h->phi_dev, h->cells * sizeof(float), hipMemcpyDeviceToHost, h->s0));
        return 0;
    });
}
