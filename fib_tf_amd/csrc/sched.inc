// sched.inc — the tick scheduler: WHEN the ticks fibhip_step accepts are launched, and how many per launch.
//
//  * fibhip_step accepts ticks (`pending`) and launches them when a launch is full; every entry point that observes or changes
//    the state launches what is pending first (flush / FLUSH).
//  * On grids whose tiles are all resident at once consecutive ticks become ONE multi-tick launch (mt_launch).  Each is
//    journalled until the stream is known good (sync_s0); one that gave up is undone and its ticks replayed (recover).
//  * The caller's series — the ticks between two observations — are remembered (series_close) and predicted
//    (predict_series); a predicted or declared (fibhip_expect) series may be launched AHEAD of the caller's calls
//    (may_run_ahead, ahead_begin), is handed out tick by tick (ahead_take) and stopped or recomputed when the caller
//    does something else (ahead_settle, in flush).
//  * What an attached recorder forbids is stated in one block: "what the recorders ask of the scheduler".
// (included by fibhip.hip, behind tick.inc)

// A multi-tick launch gave up (the give-up word names it).  The stream is idle.  The launch wrote the other slab only, and
// every multi-tick launch queued behind it left at its first boundary without writing: the state it STARTED from is where its
// journal record says.  Go back there, switch multi-tick launches off for this handle, and recompute — one launch per tick,
// bit-identical by construction — the ticks the handle's state had already moved past.  (The replay stays one launch per tick
// however long the lost launches were: the fallback leaves no multi-tick launch to replay with, mt.max is 1 from here on.
// Its cost is bounded by what the journal holds, MT_MAX_TICKS_IN_FLIGHT ticks and one launch: journal_bound.)
static int recover(fibhip_ctx *h, unsigned id)
{
    size_t i = 0;
    while (i < h->journal.recs.size() && h->journal.recs[i].id != id) ++i;
    if (i == h->journal.recs.size() || h->journal.recovering) {
        h->dead = true;
        return fail(FIBHIP_EHIP, "%s", MT_DEAD_MSG);
    }
    // the ticks the state had moved past are taken off the counters of fibhip_launch_stats here: the replay below counts them
    // again, as the plain ticks they now are
    int lost = 0;
    for (size_t j = i; j < h->journal.recs.size(); ++j)
        if (h->journal.recs[j].counted) {
            lost += h->journal.recs[j].T;
            h->mt.n_launches--;
        }
    h->mt.n_ticks -= lost;
    h->n_ticks -= lost;
    memcpy(h->cur, h->journal.recs[i].src, sizeof h->cur);
    h->journal.recs.clear();
    h->journal.ticks = 0;
    h->mt.max = h->mt.max_declared = 1;               // (mt_variant() is null from here on: no run-ahead, no series either)
    h->mt.cur = 1;
    h->mt.stale = true;
    HIPCHK(hipMemsetAsync(h->mt.give_up_word(), 0, MtState::tail_bytes(), h->s0));
    __atomic_store_n(h->mt.host_give_up(), 0u, __ATOMIC_RELEASE);
    h->journal.n_fallbacks++;
    h->journal.n_replayed += lost;
    // the samples queued behind the lost launches were taken from a void slab: the replay below (tick_now -> commit_impl)
    // takes them again, into the same slots — the slot is the host's tick counter, so every counter goes back first
    // (recorders.hpp says, row by row, why that is all it takes)
    recorders_rewind(h, lost);
    h->journal.recovering = true;
    int rc = 0;
    for (int t = 0; t < lost && rc == 0; ++t) rc = tick_now(h);
    h->journal.recovering = false;
    if (rc) {
        h->dead = true;
        return rc;
    }
    HIPCHK(wait_stream(h->s0));
    return 0;
}

static int sync_s0(fibhip_ctx *h)
{
    HIPCHK(wait_done(h->done, h->s0));
    if (h->mt.inflight && h->mt.epochs) {
        // the tile that gave up first has written its launch's id into HOST memory (page-locked, behind the host's own word):
        // nothing is copied from the device behind every launch (a 4-byte device-to-host copy at the end of every
        // synchronising call cost a 20-tick benchmark region 5-7 us of its 250)
        h->mt.inflight = false;
        const unsigned gave_up = __atomic_load_n(h->mt.host_give_up(), __ATOMIC_ACQUIRE);
        if (gave_up) return recover(h, gave_up);
        h->journal.recs.clear();                           // every launch so far has ended, and ended well
        h->journal.ticks = 0;
    }
    return 0;
}
// Nothing but another multi-tick launch is ever queued behind a multi-tick launch that has not been confirmed: a launch that
// gave up leaves the state it started from intact only as long as whatever follows it writes nothing — multi-tick launches find
// the give-up word and leave; a plain tick, a pace, a host write would not.  So those wait for the stream first.
// The entry points that confirm, each right behind its flush: fibhip_set_phase, fibhip_set_state, fibhip_set_consts,
// fibhip_pace, fibhip_lesion_apply, fibhip_step_mode (every branch: a pointwise update is in place), fibhip_step_edges, fibhip_state_ptr (the
// pointer must name the slab the state is in AFTER a recovery, and the caller writes through it), fibhip_trace_begin (every
// traced tick is a plain launch) — and inside the scheduler tick_mt for a launch of one tick and fibhip_step in front of its
// plain launches.  The entry points that only READ synchronise behind their copy (sync_s0) and take the copy again when a
// recovery happened in between: fibhip_get_state, fibhip_get_state_direct (both branches of ahead_read_back hand the frame
// back to that loop when the give-up word stands), fibhip_probe, fibhip_electrode_read, fibhip_tips_read, fibhip_frames_read, fibhip_stats_read, fibhip_leads_read, fibhip_waves_read / _labels, fibhip_spectrum_read / _peak, fibhip_beats_read / _summary / _velocity, fibhip_observe_velocity, fibhip_get_phase; fibhip_observe_begin,
// fibhip_electrode_begin / _end, fibhip_tips_begin / _end, fibhip_frames_begin / _end, fibhip_stats_begin / _end, fibhip_leads_begin / _end, fibhip_waves_begin / _end, fibhip_spectrum_begin / _end and fibhip_beats_begin / _end synchronise
// outright.
static int confirm(fibhip_ctx *h)
{
    return (h->mt.inflight && h->mt.epochs) ? sync_s0(h) : 0;
}

// ---- several ticks per launch (strip_mt_kernel) -----------------------------------------------------------------
// The tile program of a tick loops over T ticks inside one launch and re-reads only the rim of its compute box from its
// eight neighbours between two ticks (strip_mt.hpp: the protocol and MtArgs; strip_kernel.inc: strip_body).  That needs every tile resident at the same time: the plan
// must be ONE strip launch per tick whose tiles number at most the device's compute units — and no second such launch
// of this process on the device at the same time (two half-resident grids would wait for each other until both
// give up), which g_mt below guarantees.
// How many ticks will the caller's next series (the ticks between two observations of the state) have?  From the lengths of
// its last series: the same again if the last two were equal; if the lengths repeat with a period of 2, 3 or 4 — run() with an
// image() every 10 ticks inside benchmark regions of 20 ticks that start 6 ticks before a read-back: 6, 10, 4, 6, 10, 4, ... —
// the one that followed the last series' twin a period ago; else the last length (one sample).  `*repeat`: the prediction rests
// on a repetition, not on one sample.  Wrong predictions cost little: too long, the launch is stopped at the tick the caller
// reached (flush()); too short, the remaining ticks are launched the ordinary way.
static int predict_series(const fibhip_ctx *h, bool *repeat)
{
    const int n = h->series.nhist;
    if (repeat) *repeat = false;
    if (n == 0) return 0;
    const int *e = h->series.hist + n;                         // e[-1] = the last series
    if (n >= 2 && e[-1] == e[-2]) {
        if (repeat) *repeat = true;
        return e[-1];
    }
    for (int p = 2; p <= 4; ++p)
        if (n >= p + 1 && e[-1] == e[-1 - p]) {         // (ONE match is enough: a wrong guess is stopped or topped up)
            if (repeat) *repeat = true;
            return e[-p];
        }
    return e[-1];
}

// sub-steps one multi-tick launch of shape `v` advances between two exchanges: the tick's — or, for an exchange-period row
// (Variant::period), its own K
static inline bool period_row_ok(const fibhip_ctx *h, const Variant *v)
{
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
    // (the model declares its sub-steps alike — the kernel ignores where a tick ends — and the period is shorter than the tick)
    return !h->mod && h->d.model == FIBHIP_FENTON4V && Fenton::UNIFORM_SUBSTEPS && v->K < h->spt;
#else
    return false;
#endif
}
// periods of a launch of T ticks of an exchange-period row, and the sub-steps of the last one (1 .. K)
static inline int periods_of(const fibhip_ctx *h, const Variant *v, int T, int *last = nullptr)
{
    const int S = T * h->spt, P = (S + v->K - 1) / v->K;
    if (last) *last = S - (P - 1) * v->K;
    return P;
}

static bool mt_eligible(const fibhip_ctx *h, const Variant *v)
{
    if (h->mt.max <= 1 || !v || !v->fn_mt || h->use_agg) return false;
    if (v->period ? !period_row_ok(h, v) : v->K != h->spt) return false;
    const long tiles = tiles_of(h, v->TX, v->TY);
    return tiles <= h->ncu && tiles <= MT_MAX_TILES && h->d.device < 16;
}
// the shape the handle runs several ticks per launch with, or null (h->obs.on: see "what the recorders ask of the scheduler")
// `long_declared`: the launch belongs to a series the caller has declared, long enough for the declared cap (launch_cap), and
// carries no read-back
static const Variant *mt_variant(const fibhip_ctx *h, bool long_declared = false)
{
    if (h->obs.on || h->fused_fn) return nullptr;
    // An exchange-period row runs multi-tick launches while h->plan stays what a plain tick is made of (a tick on its own, the
    // replay of recover(), FIBHIP_MT=0): K is no divisor of the tick there.  A row the caller forced runs every multi-tick
    // launch.  A row autotune() chose runs the launches of long declared series only: measured at 512x512, a launch of ten ticks
    // that carries a frame pays more for its extra boundaries and its short last period than its sub-steps gain (5000 ticks
    // with a read-back every 10: 66.50 against 66.11 ms, profiles/exchange_period_ab.txt), and such launches are also the ones
    // a caller cuts short, which a period row can honour at every K / gcd(K, spt)-th tick only (ahead_settle).
    if (h->period_v && h->period_forced && mt_eligible(h, h->period_v)) return h->period_v;
    // (a chosen row rides beside a plan that runs several ticks per launch itself: no such plan, no multi-tick launches at all)
    if (h->plan.size() != 1 || !mt_eligible(h, h->plan[0].v)) return nullptr;
    if (h->period_v && long_declared && mt_eligible(h, h->period_v)) return h->period_v;
    return h->plan[0].v;
}

// ---- what the recorders ask of the scheduler ---------------------------------------------------------------------------
// Every constraint an attached recorder (record.inc) puts on the launches is stated HERE and nowhere else:
//  * activation recorder (h->obs.on): it observes every tick through commit_impl, so nothing fuses ticks — no multi-tick
//    launches (mt_variant, above, is null: hence no run-ahead and no launched series either), one tick per plain launch (multi_cap);
//  * the samplers — every row of RECORDERS (recorders.hpp) that has a Sampler, each with a stride of its own: no launch spans
//    a sample tick of any of them (sample_room, the minimum over the attached ones, bounds next_launch_ticks and multi_cap);
//    nothing runs ahead (may_run_ahead: a launch that runs ahead is handed out tick by tick and may be stopped or recomputed,
//    so a sample cannot be queued behind it, DESIGN.md section 11); a sample of a SLOW Courtemanche array — the Sampler's
//    before_slow, set at attach — is taken before 'slow' rides on its tick (slow_sample_due); one that has no slot left refuses further
//    ticks (sampler_full; the spectrum and the beat recorder never fill up, their cap is LLONG_MAX).  On a shared tick the
//    samples go out in the table's order, behind a multi-tick launch unconfirmed (recorders_advance);
//  * the stimulus program (h->stim.on), a row without a Sampler and the one hook that WRITES the state on the host's
//    word: no launch spans an event tick (stim_room, one more
//    term of sample_room), and while events are still to come a launch goes out when the ticks up to the next one are waiting
//    (cutting); nothing runs ahead while a program is attached (may_run_ahead: a stimulus cannot be queued behind a launch that
//    may be stopped or recomputed); a tick with an event due is never fused with the 'slow' behind it, whatever array the event
//    names — the stimulus comes right after its tick (slow_sample_due).  The stimulus is queued behind its launch WITHOUT
//    confirming it: stim_kernel writes nothing once a launch in front of it gave up (the rule above confirm());
//  * the trigger program, the last row that writes the STATE: a sampler like the others (launches are cut at its samples and nothing runs ahead)
//    whose sample also WRITES the state: sense, decide and the gated apply come behind the programmed stimuli of the tick,
//    unconfirmed like them (the gated apply reads the give-up word first); every sample tick comes before the 'slow' behind it
//    (its before_slow is always true), whatever arrays it names;
//  * the lesion program (h->les.on), the LAST row of the table, the other row without a Sampler and the one hook that writes the PHASE FIELD: it asks what
//    the stimulus program asks — no launch spans an event tick (lesion_room, one more term of sample_room); while events are
//    still to come a launch goes out when the ticks up to the next one are waiting (cutting); nothing runs ahead while a program
//    is attached (may_run_ahead, and the first-tick series launch of fibhip_step); the lesion is queued behind its launch
//    WITHOUT confirming it, lesion_apply_kernel writes nothing once a launch in front of it gave up.  One thing it does NOT ask:
//    a tick with a lesion due MAY be fused with the 'slow' behind it (slow_sample_due does not look at the program) — 'slow' is
//    pointwise and never reads the geometry, so tick, slow, lesion leaves the bytes of tick, lesion, slow, and not asking is
//    the simpler of the two.  A handle without a lesion program launches exactly as before: every term here is INT_MAX or false.
// (sample_room and cutting are on fibhip_step's per-call path: they read the Samplers through the rows' offsets and call nothing)
static inline bool sampling(const fibhip_ctx *h)
{
    for (const Recorder &r : RECORDERS)
        if (r.sampler != NO_SAMPLER && sampler_of(h, r)->on) return true;
    return false;
}
// Is entry `e` due right after the n-th tick since attach (n >= 1)?  The events of an entry follow the ticks number
// first + 1 + j * period + d, j = 0 .. count - 1 (count == 0: without end), d = 0 .. hold - 1 (include/fibhip.h).
static inline bool stim_due(const StimEntry &e, long long n)
{
    const long long m = n - (e.first + 1);
    if (m < 0) return false;
    if (e.period == 0) return m < e.hold;
    return m % e.period < e.hold && (e.count == 0 || m / e.period < e.count);
}
// the events of entry `e` that follow the ticks 1 .. n
static inline long long stim_events_upto(const StimEntry &e, long long n)
{
    const long long m = n - (e.first + 1);
    if (m < 0) return 0;
    if (e.period == 0) return m + 1 < e.hold ? m + 1 : e.hold;
    const long long full = m / e.period, rem = m % e.period;
    if (e.count != 0 && full >= e.count) return e.count * e.hold;
    return full * e.hold + (rem + 1 < e.hold ? rem + 1 : e.hold);
}
// the tick count of the program's next event tick behind the r.k ticks launched so far (LLONG_MAX: no event left).  Walks the
// entries, so it is kept in StimRec::next and asked only where the counter moves: at attach, in stim_advance and in recover().
static long long stim_next(const StimRec &r)
{
    const long long k = r.k;
    long long best = LLONG_MAX;
    for (const StimEntry &e : r.entries) {
        long long next = LLONG_MAX;
        if (k < e.first + 1) next = e.first + 1;
        else if (stim_due(e, k + 1)) next = k + 1;
        else if (e.period > 0) {                                   // the start of the next train element, if there is one
            const long long j = (k + 1 - (e.first + 1)) / e.period + 1;
            if (e.count == 0 || j < e.count) next = e.first + 1 + j * e.period;
        }
        if (next < best) best = next;
    }
    return best;
}
// ticks up to and including the next event tick of the attached program (INT_MAX: none attached, or no event left): one compare
// on the host's per-call path
static inline int stim_room(const fibhip_ctx *h)
{
    if (!h->stim.on || h->stim.next == LLONG_MAX) return INT_MAX;
    const long long room = h->stim.next - h->stim.k;
    return room < (long long)INT_MAX ? (int)room : INT_MAX;
}
// the lesion program's next event tick (LLONG_MAX: no event left) behind the r.k ticks launched so far: an entry is applied when
// k == tick + 1.  Kept in LesionRec::next like the stimulus program's: asked at attach, in lesion_advance and in recover()
static long long lesion_next(const LesionRec &r)
{
    long long best = LLONG_MAX;
    for (const LesionEntry &e : r.entries)
        if (e.tick + 1 > r.k && e.tick + 1 < best) best = e.tick + 1;
    return best;
}
static inline int lesion_room(const fibhip_ctx *h)
{
    if (!h->les.on || h->les.next == LLONG_MAX) return INT_MAX;
    const long long room = h->les.next - h->les.k;
    return room < (long long)INT_MAX ? (int)room : INT_MAX;
}
// ... and of any attached sampler, and of the two programs: no launch may span one
static inline int sample_room(const fibhip_ctx *h)
{
    int room = imin(stim_room(h), lesion_room(h));
    for (const Recorder &r : RECORDERS)
        if (r.sampler != NO_SAMPLER) room = imin(room, sampler_of(h, r)->room());
    return room;
}
// launches are cut at ticks still to come: a launch goes out when the ticks up to the next cut are waiting (fibhip_step)
static inline bool cutting(const fibhip_ctx *h) { return sampling(h) || stim_room(h) != INT_MAX || lesion_room(h) != INT_MAX; }
// consecutive ticks one plain launch may fuse (Courtemanche on aggregates: up to multi_max; one while an activation recorder
// is attached; never across a sample tick)
static inline int multi_cap(const fibhip_ctx *h) { return h->obs.on ? 1 : imin(h->multi_max, sample_room(h)); }
// The two caps on the ticks of one multi-tick launch.  A predicted series, and the 2, 4, ... ticks of a caller that just keeps
// stepping, may be broken at any call: MT_MAX_TICKS (mt.max).  Ticks the caller has DECLARED (fibhip_expect), in a series of
// MT_DECLARED_MIN_TICKS or more (Series::expect_long; a shorter one keeps the launches it had), go out
// MT_MAX_TICKS_DECLARED (mt.max_declared) at a time: a launch's first and last tick cost what no tick boundary inside it does
// (the prologue that reads the tile, the write-back and its drain, the kernel boundary: DESIGN.md section 6), and a declared
// launch is as cheap to stop as a short one — the tiles read the host's word at every tick (ahead_settle).
static inline int launch_cap(const fibhip_ctx *h, bool declared)
{
    return declared && h->series.expect_long ? h->mt.max_declared : h->mt.max;
}
// every pending tick was declared when it was accepted (Series::covered counts from the youngest)
static inline bool pending_declared(const fibhip_ctx *h) { return h->pending > 0 && h->series.covered >= h->pending; }
// ... in a declaration long enough for the declared cap: what mt_variant calls `long_declared`
static inline bool pending_long_declared(const fibhip_ctx *h) { return pending_declared(h) && h->series.expect_long; }
// ticks of the next multi-tick launch when `waiting` of the pending ticks wait for it
static inline int next_launch_ticks(const fibhip_ctx *h, int waiting)
{
    return imin(imin(waiting, launch_cap(h, pending_declared(h))), sample_room(h));
}
// `T` of the pending ticks are being launched (the oldest)
static inline void take_pending(fibhip_ctx *h, int T)
{
    h->pending -= T;
    h->series.covered = imin(h->series.covered, h->pending);
}
// the last pending tick ends on a sample of an array 'slow' assigns: the sample must see it before 'slow', which belongs to the
// next tick — the two are not fused then (fibhip_step_mode)
static inline bool slow_sample_due(const fibhip_ctx *h)
{
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
    // (a stimulus due after the last pending tick comes before 'slow' too, whatever array it names)
    if (h->stim.on && h->stim.k + h->pending == h->stim.next) return true;
    // (... and so does a sample of the trigger program — tick, sense / stimulus, slow — and a sample that reads a slow array)
    for (const Recorder &r : RECORDERS) {
        const Sampler *s = sampler_of(h, r);
        if (s && s->on && s->before_slow && s->due_after(h->pending)) return true;
    }
    return false;
#else
    return false;
#endif
}
// the sampler that has no slot left for the samples of `more` further ticks (pending ones included), or null; `cap`: the samples
// it holds
static inline const char *sampler_full(const fibhip_ctx *h, int more, long long *cap = nullptr)
{
    for (const Recorder &r : RECORDERS) {
        const Sampler *s = sampler_of(h, r);
        if (s && s->on && s->full_after(more)) {
            if (cap) *cap = s->cap;
            return r.noun;
        }
    }
    return nullptr;
}

static struct {
    std::mutex mu;
    fibhip_ctx *owner[16] = {nullptr};              // per device: the handle whose stream carries the last such launch
} g_mt;

static void mt_forget(fibhip_ctx *h)
{
    std::lock_guard<std::mutex> lock(g_mt.mu);
    for (fibhip_ctx *&o : g_mt.owner)
        if (o == h) o = nullptr;                     // (fibhip_destroy has drained the stream)
}

// one launch advancing T >= 2 ticks from the current slab into the other one; `commit`: the handle's state moves with it
// (autotune times such launches without moving the state)
static int mt_launch(fibhip_t h, const Variant *v, int T, bool commit, int *nxt_out, float *snap = nullptr, int snap_var = 0)
{
    if (!h->mt.xbuf) {
        if (hipMalloc((void **)&h->mt.xbuf, 2 * (size_t)((h->nvar + 3) / 4 * 4) * h->cells * sizeof(float)) != hipSuccess) {
            h->mt.xbuf = nullptr;
            return fail(FIBHIP_ENOMEM, "hipMalloc of the tick-exchange buffer failed");
        }
        if (hipMalloc((void **)&h->mt.epochs, MtState::words_bytes()) != hipSuccess) {
            h->mt.epochs = nullptr;
            return fail(FIBHIP_ENOMEM, "hipMalloc of the epoch words failed");
        }
        h->mt.stale = true;
        // page-locked: the tiles' words of a read-back inside a launch, and behind them the host's word (flush())
        if (hipHostMalloc((void **)&h->mt.snap_flags, ((size_t)MT_HOST_WORD_AT + 16) * sizeof(unsigned), hipHostMallocDefault) != hipSuccess) {
            h->mt.snap_flags = nullptr;
            return fail(FIBHIP_ENOMEM, "hipHostMalloc of the host-side words failed");
        }
        memset(h->mt.snap_flags, 0, ((size_t)MT_HOST_WORD_AT + 16) * sizeof(unsigned));
        HIPCHK(hipHostGetDevicePointer((void **)&h->mt.snap_flags_dev, h->mt.snap_flags, 0));
        h->mt.host_word = h->mt.snap_flags + MT_HOST_WORD_AT;
    }
    const bool trial = !commit && !nxt_out;           // (autotune: timed and checked on the spot, never part of the state)
    // A handle whose chosen exchange-period row runs beside its plan alternates between two tilings.  Tiles store absolute epoch
    // values and a word nobody wrote for a while is only ever OLDER than wanted, so a stale word makes its reader wait for the
    // store that is coming anyway — until it is 2^31 boundaries behind, when the wrapping compare reads it as ahead (hours of
    // nothing but launches of the other shape).  So the tiles' words start equal again whenever the shape changes: queued on the
    // same stream, and the tiles' words only — the give-up word behind them must stand for the launches queued behind a launch
    // that gave up.  (autotune's trials alternate shapes eight ticks at a time and zero all words behind the last of them.)
    if (!trial) {
        if (h->mt.last_v && h->mt.last_v != v && !h->mt.stale) {
            HIPCHK(hipMemsetAsync(h->mt.epochs, 0, MtState::words_bytes() - MtState::tail_bytes(), h->s0));
            h->mt.epoch_base = 0;
        }
        h->mt.last_v = v;
    }
    if (h->mt.stale) {                            // first use, or the tiling may have changed: all words equal again
        HIPCHK(hipMemsetAsync(h->mt.epochs, 0, MtState::words_bytes(), h->s0));
        h->mt.epoch_base = 0;
        h->mt.stale = false;
    }
    LaunchCtx c;
    int nxt[FIB_MAXVAR];
    fill_ptrs(h, c, v->K, h->cur, nxt);
    c.sub0 = 0;
    c.g = base_geo(h);
    c.mt.xb = h->mt.xbuf;
    c.mt.epoch = h->mt.epochs;
    c.mt.err = h->mt.give_up_word();
    c.mt.epoch0 = h->mt.epoch_base;
    h->mt.seq = h->mt.seq % h->mt.ids + 1u;           // 1 .. 65535 (FIBHIP_MT_IDS: a smaller cycle, for the tests)
    // (the host's word keeps naming the last launch it was written for: that id is not given out again while it stands there)
    if (h->mt.host_word && (__atomic_load_n(h->mt.host_word, __ATOMIC_RELAXED) >> 16) == h->mt.seq) h->mt.seq = h->mt.seq % h->mt.ids + 1u;
    // (an exchange-period row: the low half counts PERIODS, and the sub-steps of the last one travel in `sub0`, which no model
    // with uniform sub-steps reads)
    int last_steps = v->K;
    const int nbound = v->period ? periods_of(h, v, T, &last_steps) : T;      // passes of the kernel's outer loop
    if (v->period) c.sub0 = last_steps;
    c.mt.ticks_id = (unsigned)nbound | (h->mt.seq << 16);
    if (v->kern_mt) module_kernel(c, h, v->kern_mt, MK_STRIP_MT, v);
    c.mt.snap = snap;
    c.mt.snap_flag = h->mt.snap_flags_dev;
    c.mt.snap_seq = h->ahead.snap_seq;
    c.mt.snap_var = (snap_var & 0xFF) | (int)(h->mt.wait_ms << 8);
    if (!trial) {
        MtRec rec;
        rec.id = h->mt.seq;
        rec.T = T;
        rec.counted = commit;
        memcpy(rec.src, h->cur, sizeof rec.src);
        h->journal.recs.push_back(rec);
        h->journal.ticks += T;
        if (h->journal.fake_giveup_at > 0 && ++h->journal.fake_seen == h->journal.fake_giveup_at) {
            // test switch: this launch finds the give-up word raised in its name — what its tiles would have written had one
            // of them waited out its bound — and leaves at its first boundary, like every launch behind it
            unsigned *w = (unsigned *)(h->probe_host + 12);
            *w = h->mt.seq;
            HIPCHK(hipMemcpyAsync(c.mt.err, w, sizeof(unsigned), hipMemcpyHostToDevice, h->s0));
            __atomic_store_n(h->mt.host_give_up(), h->mt.seq, __ATOMIC_RELEASE);      // (what that tile would also have written)
        }
    }
    {
        std::lock_guard<std::mutex> lock(g_mt.mu);
        fibhip_ctx *&owner = g_mt.owner[h->d.device];
        if (owner && owner != h) {                    // behind the other handle's launches, never beside them
            HIPCHK(hipEventRecord(owner->ev_main, owner->s0));
            HIPCHK(hipStreamWaitEvent(h->s0, owner->ev_main, 0));
        }
        if (int rc = trace_open(h, h->s0, "strip_mt_kernel", v->K, v->TX, v->TY, v->NT, T)) return rc;
        HIPCHK(v->fn_mt(h->s0, c));
        if (int rc = trace_close(h, h->s0)) return rc;
        owner = h;
    }
    h->launches++;
    if (commit) {
        h->mt.n_launches++;
        h->mt.n_ticks += T;
        h->n_ticks += T;
    }
    h->mt.inflight = true;
    h->mt.epoch_base += (unsigned)(nbound - 1);          // every tile raised its word once per tick (period) boundary
    if (commit) memcpy(h->cur, nxt, sizeof nxt);
    if (nxt_out) memcpy(nxt_out, nxt, sizeof nxt);
    // (the hooks stand behind this launch unconfirmed: a sample reads the state and writes the recorder's own buffers only, and
    // whatever accumulates or writes the state leaves without writing when this launch or one in front of it gave up)
    return commit ? recorders_advance(h, T, true) : 0;
}

// A caller that never synchronises must not grow the journal without bound: every 256 multi-tick launches, or
// MT_MAX_TICKS_IN_FLIGHT ticks if that is sooner (launches of a declared series), the stream is
// drained once (20 us in 100 ms of work) and the launches so far are confirmed — or the first that gave up is found.
// The bound in ticks is also what keeps every wait behind unconfirmed launches short whatever a launch holds: confirm(),
// the stop of ahead_settle and the frame poll of ahead_read_back wait for that many ticks and one launch at most.
// The give-up word names a launch by its 16-bit id, and recover() looks the id up in the journal: the journal never holds more
// records than a cycle of ids has distinct values (ids - 1: the id the host's word names is skipped), or the id of the launch
// that gave up could also be that of an older one that ended well (FIBHIP_MT_IDS shortens the cycle, for the tests).
static int journal_bound(fibhip_ctx *h)
{
    const size_t most = h->mt.ids - 1u < 256u ? (size_t)(h->mt.ids - 1u) : (size_t)256;
    if ((h->journal.recs.size() < most && h->journal.ticks < MT_MAX_TICKS_IN_FLIGHT) || h->ahead.n > 0) return 0;
    return sync_s0(h);
}

static int tick_mt(fibhip_t h, const Variant *v, int T)
{
    if (T <= 1) {
        CONFIRM(h);
        return tick_now(h);
    }
    if (h->phase_of_tick != 0) return fail(FIBHIP_EINVAL, "step: previous tick not committed");
    if (int rc = check_ready(h)) return rc;
    if (int rc = journal_bound(h)) return rc;
    if (h->mt.max <= 1) {                             // (a launch among those just confirmed had given up: one launch per tick now)
        for (int t = 0; t < T; ++t)
            if (int rc = tick_now(h)) return rc;
        return 0;
    }
    return mt_launch(h, v, T, true, nullptr);
}

// On a row block a fused launch stays inside the exchange cycle: the tick that ends it is the caller's
// step_edges / exchange / step_interior / step_commit.
static inline int cycle_clamp(const fibhip_ctx *h, int T) { return is_shard(h) ? imax(1, imin(T, h->cycle - 1 - h->cpos)) : T; }

// T consecutive ticks as one plain launch (T <= multi_cap, inside the exchange cycle: cycle_clamp)
static int tick_multi(fibhip_t h, int T)
{
    if (T <= 1) return tick_now(h);
    h->plan.swap(h->plan_multi[T]);
    h->span = T;
    const int rc = tick_now(h);
    h->span = 1;
    h->plan.swap(h->plan_multi[T]);
    return rc;
}

// launch `n` of the ticks fibhip_step has deferred, the fewest launches first
static int launch_pending(fibhip_t h, int n)
{
    if (n > 0 && !h->tracing)
        if (mt_variant(h)) {
            while (n > 0) {
                const Variant *v = mt_variant(h, pending_long_declared(h));
                const int T = next_launch_ticks(h, n);
                take_pending(h, T);
                n -= T;
                if (int rc = tick_mt(h, v, T)) return rc;
                h->series.run += T;
            }
            return 0;
        }
    while (n > 0) {
        const int T = cycle_clamp(h, imin(multi_cap(h), n));
        take_pending(h, T);
        n -= T;
        if (int rc = tick_multi(h, T)) return rc;
    }
    return 0;
}

// ---- run-ahead -------------------------------------------------------------------------------------------------------
// A launch of L ticks the caller has not asked for yet.  It reads the current slab and writes the other one, so until its
// ticks are handed out the handle's state is untouched: ahead_begin starts it, fibhip_step hands its ticks out call by call
// (ahead_take) and moves the state when the last is taken (ahead_adopt); a caller that does anything else first has it
// stopped at the tick it reached, or cancelled (ahead_settle, from flush).
enum AheadFrom { AHEAD_FROM_STEP, AHEAD_FROM_READ_BACK };

// May a launch of the L ticks this handle expects next start now, ahead of the caller's calls?  `repeats`: L rests on a
// repetition of the caller's series or on its declaration, not on one sample; `declared`: on its declaration, which covers
// all L ticks (launch_cap).  (What belongs to the CALL rather than to the
// handle stays with the caller: fibhip_step asks only when the call leaves part of the series open, 0 < nticks < L; the
// read-back only for one array, var >= 0.)
static bool may_run_ahead(const fibhip_ctx *h, int L, bool repeats, bool declared, AheadFrom from)
{
    // the series is worth a launch of its own and fits one (this implies mt.max > 1)
    if (L < 2 || L > launch_cap(h, declared)) return false;
    // nothing forbids it: the switch and the caller's access to the state (Ahead::ok), no launch ahead already, no sampler
    // (see "what the recorders ask of the scheduler"), no timeline being taken (every launch there is the caller's own)
    if (!h->ahead.ok || h->ahead.n != 0 || sampling(h) || h->stim.on || h->les.on || h->tracing) return false;
    // the launch is the one the handle would make anyway: its plan is chosen (`tuned`, which is only ever set behind
    // check_ready — so has_consts holds with it and is stated for the reader, not tested twice), the slab is planar.
    // Nothing accepted is still waiting and no tick is open: fibhip_step refuses an open tick and tests `pending` here; at the
    // read-back flush() has just run (pending == 0, ahead.n == 0) and an open tick was refused before.
    if (!h->tuned || !h->has_consts || h->pitch != h->d.width || h->pending != 0 || h->phase_of_tick != 0) return false;
    switch (from) {
    case AHEAD_FROM_STEP:
        // the first tick of a series is here: ONE sample of the caller's pattern is believed as long as it has not been
        // wrong since the last two equal series (Series::trust) — being wrong costs a stopped launch, waiting for a
        // repetition costs every second series of a regular caller
        return repeats || h->series.trust;
    case AHEAD_FROM_READ_BACK:
        // no tick of the next series has been asked for: only a repetition (or a declaration) is believed, and only if ticks
        // have run since the last observation — a second read-back of the same state starts nothing — or the caller has
        // declared a series none of whose ticks it has asked for yet
        return repeats && (h->series.fresh || (h->series.expect > 0 && h->series.expect_fresh));
    }
    return false;
}

// starts the launch; `snap`: it also carries the read-back of array `snap_var` into that (device-visible) host buffer
static int ahead_begin(fibhip_ctx *h, const Variant *v, int L, float *snap = nullptr, int snap_var = 0)
{
    if (int rc = mt_launch(h, v, L, false, h->ahead.nxt, snap, snap_var)) return rc;
    h->ahead.n = L;
    h->ahead.used = 0;
    h->ahead.id = h->mt.seq;
    h->ahead.v = v;
    return 0;
}

// nothing of the launch counts (its journal record stays uncounted): the state it started from stands
static inline void ahead_drop(fibhip_ctx *h) { h->ahead.n = h->ahead.used = 0; }

// the state moves to where the launch put it after `ticks` ticks (all of them, or the tick it was stopped at)
static void ahead_adopt(fibhip_ctx *h, int ticks)
{
    for (auto &r : h->journal.recs)                 // (the launch's journal record: what it did)
        if (r.id == h->ahead.id) {
            h->journal.ticks -= r.T - ticks;
            r.T = ticks;
            r.counted = true;
        }
    memcpy(h->cur, h->ahead.nxt, sizeof h->cur);
    h->mt.n_launches++;
    h->mt.n_ticks += ticks;
    h->n_ticks += ticks;
    ahead_drop(h);
}

// hands out up to `nticks` of the ticks computed ahead; returns how many of the caller's ticks that covers
static int ahead_take(fibhip_ctx *h, int nticks)
{
    const int take = imin(nticks, h->ahead.n - h->ahead.used);
    h->ahead.used += take;
    h->series.run += take;
    if (h->ahead.used == h->ahead.n) ahead_adopt(h, h->ahead.n);     // all handed out
    return take;
}

// The caller did not go on as predicted.  The launch that ran ahead is told so through the host's word (page-locked
// host memory; ONE thread of the grid reads it at the start of every tick and passes it on at the tick's end):
//  * some of its ticks have been handed out: "stop after ahead.used ticks" — a tile leaves through its write-back at
//    that boundary, and counts itself.  The interpreter hands ticks out faster than the device computes them, so the
//    boundary is normally still ahead of every tile and nothing is computed twice; if a tile was past it already (it
//    then leaves without writing) the count falls short and the ticks are recomputed from the state the launch
//    started from — still intact: the launch writes the other slab only;
//  * none has: the launch is simply cancelled.
static int ahead_settle(fibhip_ctx *h)
{
    const int redo = h->ahead.used;
    bool kept = false;
    if (h->mt.epochs) {
        // (the word names the launch: earlier launches of this handle may still be queued or running)
        unsigned stop_at = redo > 0 ? (unsigned)redo : MT_CANCEL;
        const Variant *av = h->ahead.v;                 // (the shape THAT launch runs)
        if (redo > 0 && av && av->period) {
            // an exchange-period launch counts periods, and holds the state after `redo` ticks only at a boundary that falls on
            // that tick's end.  Between two boundaries there is nothing to stop at — a period is never shortened on the fly: tiles
            // that saw the word at different times would disagree — so the launch is cancelled and the ticks handed out are
            // recomputed from the slab it started from, the way out a stop that came too late takes below.
            const int sub = redo * h->spt;
            stop_at = sub % av->K == 0 ? (unsigned)(sub / av->K) : MT_CANCEL;
        }
        const bool stop = stop_at != MT_CANCEL;
        unsigned word = (h->ahead.id << 16) | stop_at;
        // (a plain store: the tiles read this word over PCIe.  A copy through the second stream does not reach a device
        // whose compute units are all taken before the launch has ended: measured at 512x512, 238-387 us)
        __atomic_store_n(h->mt.host_word, word, __ATOMIC_RELEASE);
        h->mt.stale = true;
        if (stop) {
            HIPCHK(hipMemcpyAsync(h->probe_host + 10, h->mt.stop_count_word(), sizeof(unsigned), hipMemcpyDeviceToHost, h->s0));
            SYNC_S0(h);
            unsigned stopped;
            memcpy(&stopped, h->probe_host + 10, sizeof stopped);
            kept = (long)stopped == (av ? tiles_of(h, av->TX, av->TY) : -1);
        }
    }
    if (kept) {                                     // the state after `redo` ticks is where the launch wrote it
        ahead_adopt(h, redo);
        h->ahead.n_kept++;
        return 0;
    }
    ahead_drop(h);
    h->series.run -= redo;
    h->pending += redo;                             // (in front of whatever is pending: Series::covered stands)
    if (redo > 0) {
        h->ahead.n_redone++;
        h->series.trust = false;                    // ONE sample is not believed again until two equal series were seen
    }
    return 0;
}

// the caller is about to look at the state: the ticks since its last look were one series, the next tick starts a new one
static void series_close(fibhip_ctx *h)
{
    Series &s = h->series;
    s.fresh = s.run > 0;
    if (s.run > 0) {
        if (s.nhist == 8) {
            memmove(s.hist, s.hist + 1, 7 * sizeof(int));
            s.nhist = 7;
        }
        s.hist[s.nhist++] = s.run;
        s.run = 0;
        if (s.nhist >= 2 && s.hist[s.nhist - 1] == s.hist[s.nhist - 2]) s.trust = true;
    }
    h->mt.cur = 1;
    if (!s.expect_fresh) s.expect = 0;              // an observation inside a declared series ends the declaration
}

// launch the ticks fibhip_step left pending; every entry point that observes or changes the state calls this first
static int flush(fibhip_t h)
{
    if (h->ahead.n > 0)
        if (int rc = ahead_settle(h)) return rc;
    const int rc = launch_pending(h, h->pending);
    series_close(h);
    return rc;
}

// The read-back of ONE array as the start of the caller's next series (fibhip_get_state_direct, behind its flush).
// A caller that alternates series of n ticks with one read-back — IonicModel.run() with image() every n
// ticks, fenton.py:184-185 — would leave the device idle for the whole read-back (34 us of a 125 us series at
// 512x512).  When the lengths of the last series repeat (predict_series), the next n ticks are launched HERE, before the frame is waited
// for (the launch reads the slab the frame comes from and writes the other one).  fibhip_step then hands those ticks out
// without launching anything; any other call first makes the state what the caller has been told it is (flush()).
// The frame itself travels INSIDE that launch when the destination is page-locked memory the device can write
// (fibhip_host_alloc: what the Python binding hands in): every tile stores its cells of the array straight into it
// while it starts computing and raises a word in host memory at its first tick boundary; this thread polls those words.
// No copy engine, no blit kernel (which beside a grid that holds every compute unit would crawl: measured), no gap
// between two series.  Any other destination: the copy goes first on the same stream and the launch right behind it.
// `*delivered`: the frame is in `dst`; else the caller copies it the plain way.
static int ahead_read_back(fibhip_ctx *h, int var, float *dst, bool *delivered)
{
    *delivered = false;
    if (int rc = journal_bound(h)) return rc;
    bool repeats = false;
    int L = predict_series(h, &repeats);
    const bool declared = h->series.expect > 0 && h->series.expect_fresh;
    if (declared) {                                         // the caller has said how many ticks it will ask for next (fibhip_expect)
        L = imin(h->series.expect, launch_cap(h, true));
        repeats = true;
    }
    if (var < 0 || !may_run_ahead(h, L, repeats, declared, AHEAD_FROM_READ_BACK)) return 0;
    const Variant *mv = mt_variant(h);
    if (!mv) return 0;
    void *dev_dst = nullptr;
    const bool in_launch = hipHostGetDevicePointer(&dev_dst, dst, 0) == hipSuccess && dev_dst != nullptr;
    if (!in_launch) (void)hipGetLastError();
    if (in_launch) {
        h->ahead.snap_seq++;
        if (int rc = ahead_begin(h, mv, L, (float *)dev_dst, var)) return rc;
    } else {
        HIPCHK(hipMemcpyAsync(dst, h->slab[h->cur[var]] + (size_t)var * h->vstride, h->cells * sizeof(float), hipMemcpyDeviceToHost, h->s0));
        HIPCHK(hipEventRecord(h->ahead.ev, h->s0));
        if (int rc = ahead_begin(h, mv, L)) return rc;
    }
    h->series.fresh = false;
    if (!in_launch) {
        HIPCHK(wait_event(h->ahead.ev));
        // as below: a launch in front of the copy that gave up has said so in the host's memory before the copy ended, and
        // the frame is then one of a void slab — nothing of the launch just started counts, the state is restored and
        // recomputed and the caller copies the frame the plain way
        if (__atomic_load_n(h->mt.host_give_up(), __ATOMIC_ACQUIRE) != 0u) {
            ahead_drop(h);
            SYNC_S0(h);
            return 0;
        }
        *delivered = true;
        return 0;
    }
    // every tile's word at this read-back's sequence number = every cell of the frame has landed
    const int ntiles = (int)tiles_of(h, mv->TX, mv->TY);
    volatile unsigned *fl = h->mt.snap_flags;
    const unsigned want = h->ahead.snap_seq;
    const auto t0 = std::chrono::steady_clock::now();
    int next = 0;
    long spins = 0;
    while (next < ntiles) {
        if (fl[(size_t)next * MT_SNAP_STRIDE] == want) {
            ++next;
            continue;
        }
        if ((++spins & 1023) == 0) {
            // a launch that has ended without raising every word gave up (or was never resident): report it
            if (hipStreamQuery(h->s0) == hipSuccess && fl[(size_t)next * MT_SNAP_STRIDE] != want) {
                // the launch gave up (or found the give-up word raised): nothing of it counts, the state it started
                // from stands (sync_s0 -> recover), and the frame comes the plain way
                ahead_drop(h);
                SYNC_S0(h);
                if (mt_variant(h)) return fail(FIBHIP_EHIP, "the launch that carried the read-back ended without delivering it");
                return 0;
            }
            (void)hipGetLastError();
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                h->dead = true;
                return fail(FIBHIP_EHIP, "%s", MT_DEAD_MSG);
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    // The frame is the state the launch STARTED from.  If a launch in front of it gave up, that state is void — and the
    // tiles of that launch have said so in the host's memory before this launch's tiles could raise their words (one
    // stream: this launch started after that one had ended).  Then nothing of this launch counts: the state is restored
    // and recomputed (sync_s0 -> recover) and the frame comes the plain way.  (Found by the stress run of
    // tests/test_gpu_recovery.py: 7 of 400 random call sequences returned a frame of a void state.)
    if (__atomic_load_n(h->mt.host_give_up(), __ATOMIC_ACQUIRE) != 0u) {
        ahead_drop(h);
        SYNC_S0(h);
        return 0;
    }
    *delivered = true;
    return 0;
}

extern "C" int fibhip_step_edges(fibhip_t h)
{
    NEED(h);
    FLUSH(h);
    CONFIRM(h);
    if (const char *who = sampler_full(h, 1)) return fail(FIBHIP_EINVAL, "step_edges: trace full (%s recorder)", who);
    return edges_impl(h);
}

extern "C" int fibhip_step_interior(fibhip_t h)
{
    NEED(h);
    return interior_impl(h);
}

extern "C" int fibhip_step_commit(fibhip_t h)
{
    NEED(h);
    return commit_impl(h);
}

extern "C" int fibhip_step(fibhip_t h, int nticks)
{
    NEED(h);
    if (nticks < 0) return fail(FIBHIP_EINVAL, "negative tick count");
    if (h->phase_of_tick != 0) return fail(FIBHIP_EINVAL, "step inside an open tick");
    // Ticks are accepted here and launched when a launch is full: up to multi_max ticks go into one kernel (CourtAgg),
    // and the last accepted tick is held back when the next call may be a step_slow, which then rides on its launch
    // (fused_fn).  Whatever is held back is launched by the next entry point that observes or changes the state.
    // Fenton / Beeler-Reuter on a grid whose tiles are all resident at once: consecutive ticks become ONE launch whose
    // tiles hand their rims to each other (tick_mt).  A launch goes out as soon as `mt.cur` ticks are waiting and takes
    // every waiting tick, up to mt.max.  mt.cur is 1 after any call that observes the state, so the device starts at once;
    // then the rest of the series if the caller works in series of equal length (run() with an image() every n ticks, a
    // benchmark region: the ticks between the last two observations), else 2, 4, ... mt.max while the caller keeps stepping.
    // A series is launched WHOLE at its first tick when the caller's last series had that length (a benchmark region, run()
    // with a probe or a sync every n ticks): one launch of n ticks instead of the first tick at once + the other n-1 when the
    // last of them has arrived (at 512x512: the device idle while the interpreter makes its 19 other calls, and two launch
    // prologues instead of one — 270 -> 247 us per 20-tick region).  It is the run-ahead of ahead_read_back started
    // from here: the ticks are handed out below call by call, and a caller that does anything else first gets them recomputed
    // / cancelled by flush() — after which ONE sample is not believed again until two equal series have been seen.
    // A caller that KNOWS its series says so (fibhip_expect: IonicModel.run() does, from its frame period and tick count) and
    // nothing is guessed: the declared ticks are launched at the first of them, mt.max_declared at a time (launch_cap: 256 by
    // default against the 32 of everything above.  At Fenton 512x512 the 5000 declared ticks of a benchmark region take
    // 11.58 us per tick as 157 launches of 32 and 11.44 as 20 of 256, 1.2 %; the kernel trace shows no gap between two
    // launches either way, a launch's first and last tick are what costs — profiles/series_launch_ab.txt).
    long long full_cap = 0;
    if (const char *who = sampler_full(h, h->pending + nticks, &full_cap))
        return fail(FIBHIP_EINVAL, "step: trace full (the %s recorder holds %lld samples; read it, then detach or re-attach)", who, full_cap);
    if (int rc = journal_bound(h)) return rc;
    // (the guards in front are may_run_ahead's own, taken first because most calls end at one of them)
    if (nticks > 0 && h->ahead.n == 0 && h->mt.max > 1 && !sampling(h) && !h->stim.on && !h->les.on) {
        bool repeats = false;
        const bool declared = h->series.expect > 0;
        int L = 0;
        if (declared) {
            L = imin(h->series.expect, launch_cap(h, true));
            repeats = true;
        } else if (h->series.run == 0) {
            L = predict_series(h, &repeats);
        }
        if (nticks < L && may_run_ahead(h, L, repeats, declared, AHEAD_FROM_STEP))
            if (const Variant *v = mt_variant(h, declared && h->series.expect_long))
                if (int rc = ahead_begin(h, v, L)) return rc;
    }
    int covered = 0;                                   // how many of this call's ticks the declaration covers (its first)
    if (h->series.expect > 0 && nticks > 0) {          // (the declared series has begun / goes on)
        covered = imin(nticks, h->series.expect);
        h->series.expect -= covered;
        h->series.expect_fresh = false;
    }
    if (h->ahead.n > 0 && nticks > 0) {                // ticks that have been computed ahead already
        const int took = ahead_take(h, nticks);
        nticks -= took;
        covered = imax(0, covered - took);
        if (nticks == 0) return 0;
    }
    if (h->mt.max > 1 && nticks > 0 && !h->tracing) {
        if (int rc = check_ready(h)) return rc;
        if (!h->tuned)
            if (int rc = autotune(h)) return rc;
        if (mt_variant(h)) {
            h->pending += nticks;
            // (a call that goes past the end of its declaration leaves undeclared ticks behind the declared ones: none counts)
            h->series.covered = covered == nticks ? h->series.covered + covered : 0;
            // With a sampler attached (or a stimulus or lesion program with events to come) a launch goes out when the ticks up to the next sample tick are waiting (or mt.max of
            // them) and ends there: between two samples the handle runs the fewest launches `every` allows, whatever the
            // caller's call pattern.  (Without one: mt.cur, as described above.)
            while (h->pending >= (cutting(h) ? imin(sample_room(h), launch_cap(h, pending_declared(h))) : h->mt.cur)) {
                const Variant *v = mt_variant(h, pending_long_declared(h));
                const int T = next_launch_ticks(h, h->pending);
                take_pending(h, T);
                if (int rc = tick_mt(h, v, T)) return rc;
                const bool first = h->series.run == 0;
                h->series.run += T;
                const int rest = predict_series(h, nullptr) - h->series.run;
                h->mt.cur = (first && rest >= 2) ? imin(rest, h->mt.max) : imin(2 * h->mt.cur, h->mt.max);
            }
            return 0;
        }
    }
    // plain launches from here on: none behind an unconfirmed multi-tick launch.  (Nothing to launch: nothing to wait for — a
    // call of no ticks beside a launch that runs ahead leaves that launch to the call that settles it, flush().)
    if (h->pending + nticks > 0) CONFIRM(h);
    const int reserve = (h->fused_fn && !h->tracing) ? 1 : 0;
    // (multi_cap moves with the samplers' tick counters: the bound is taken afresh for every launch)
    auto held = [&] { return ((multi_cap(h) > 1 && !h->tracing) ? multi_cap(h) - 1 : 0) + reserve; };
    const int cap = held();
    if (cap > 0 && nticks > 0) {
        if (int rc = check_ready(h)) return rc;           // a deferred tick must not fail later, in someone else's call
        if (!h->tuned)                                    // (here, not inside a launch: the plans are being chosen)
            if (int rc = autotune(h)) return rc;
    }
    h->pending += nticks;
    while (h->pending > held()) {
        const int T = cycle_clamp(h, h->tracing ? 1 : imin(multi_cap(h), h->pending - reserve));
        take_pending(h, T);
        if (int rc = tick_multi(h, T)) return rc;
    }
    return 0;
}

extern "C" int fibhip_expect(fibhip_t h, int nticks)
{
    if (!h || nticks < 0) return fail(FIBHIP_EINVAL, "expect: bad argument");
    h->series.expect = nticks;
    h->series.expect_fresh = nticks > 0;
    h->series.expect_long = nticks >= MT_DECLARED_MIN_TICKS;
    return 0;
}
