// recorders.hpp — the ONE list of the hooks that stand behind a committed launch (record.inc), in hook order.  Whatever
// enumerates recorders walks this table: the hooks behind a plain tick and behind a multi-tick launch (recorders_advance), what
// they ask of the scheduler (sched.inc: sampling, sample_room, slow_sample_due, sampler_full), the rewind of a recovery
// (recorders_rewind) and the release of their buffers (recorders_free).  A new recorder is one row here.  The table is a
// constant: the loops over it unroll, the offsets fold and the hooks are called directly — nothing on fibhip_step's per-call path
// goes through a pointer.
// (included by fibhip.hip between ctx.hpp and tick.inc; the functions the rows name are record.inc's)
#pragma once

typedef int recorder_advance_fn(fibhip_ctx *h, int ticks, bool behind_mt);
typedef void recorder_free_fn(fibhip_ctx *h);
typedef bool recorder_on_fn(const fibhip_ctx *h);
typedef void recorder_rewind_fn(fibhip_ctx *h, int lost);
struct Recorder {
    const char *noun;                   // what sampler_full calls it
    size_t sampler;                     // where its Sampler lives in the handle; NO_SAMPLER: an event-driven row (the two programs)
    recorder_advance_fn *advance;       // the hook behind a launch of `ticks` ticks
    recorder_free_fn *release;          // frees its device buffers and detaches it
    // event-driven rows only (a Sampler answers both itself): is it attached, and the rewind of a recovery — the counter goes
    // back by the ticks the replay takes again and `next` is formed afresh from it
    recorder_on_fn *on = nullptr;
    recorder_rewind_fn *rewind = nullptr;
};
constexpr size_t NO_SAMPLER = ~(size_t)0;

static recorder_advance_fn electrode_advance, tips_advance, frames_advance, stats_advance, leads_advance, pmap_advance, waves_advance, spectrum_advance, beats_advance, stim_advance, trig_advance, lesion_advance;
static recorder_free_fn electrode_free, tips_free, frames_free, stats_free, leads_free, pmap_free, waves_free, spectrum_free, beats_free, stim_free, trig_free, lesion_free;
static long long stim_next(const StimRec &r);                   // sched.inc
static long long lesion_next(const LesionRec &r);               // sched.inc
static inline bool stim_on(const fibhip_ctx *h) { return h->stim.on; }
static inline bool lesion_on(const fibhip_ctx *h) { return h->les.on; }
static inline void stim_rewind(fibhip_ctx *h, int lost)
{
    h->stim.k -= lost;
    h->stim.next = stim_next(h->stim);
}
static inline void lesion_rewind(fibhip_ctx *h, int lost)
{
    h->les.k -= lost;
    h->les.next = lesion_next(h->les);
}

// (`on` is the Sampler's first member; the handle holds vectors, which is all that makes offsetof conditionally supported here)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
#define SAMPLER_AT(member) offsetof(fibhip_ctx, member.on)
// The ORDER is the order of the launches behind a tick and is load-bearing: the samplers see the state as the tick left it; the
// stimulus belongs to the next tick and comes behind them; the trigger program senses what the stimulus left and fires; the lesion program
// changes the geometry for the next tick, behind everything that looks at this one.
// Behind a multi-tick launch every hook stands UNCONFIRMED (behind_mt), and a recovery rewinds every counter by the ticks it
// replays — the slot is the host's counter, so the replay fills the same slots again.  Why each row may be rewound:
static constexpr Recorder RECORDERS[] = {
    // these four read the state and rewrite whole slots of their own buffers: a sample taken from a void slab is overwritten
    {"electrode", SAMPLER_AT(el), electrode_advance, electrode_free},
    {"tip", SAMPLER_AT(tip), tips_advance, tips_free},
    {"frame", SAMPLER_AT(fr), frames_advance, frames_free},
    {"statistics", SAMPLER_AT(st), stats_advance, stats_free},
    // ... and so does the lead recorder, a fifth of that kind: lead_kernel reads the state, the phase arrays and the recorder's
    // own constant tables and writes every partial of its (lead, tile) slots whole; lead_combine_kernel writes the sample's row
    // whole from those partials.  Nothing is accumulated across samples and the slot follows from the counter, so a sample taken
    // from a void slab is overwritten, partials and row, when the replay takes it again
    {"lead", SAMPLER_AT(ld), leads_advance, leads_free},
    // ... and the potential-map recorder, of the same kind: pmap_source_kernel reads the state, the phase arrays and the
    // recorder's weight plane and writes EVERY cell of the scratch plane q (its border of zeros is written at attach and by
    // nobody after); pmap_conv_kernel reads q and the recorder's constant table and writes every site of the sample's slot
    // with plain stores.  Nothing is accumulated across samples and the slot follows from the counter: a sample taken from a
    // void slab is overwritten, scratch plane and slot, when the replay takes it again.  No give-up word is needed: both
    // kernels end on any state.  (pmap_summary_kernel runs at read time, behind a confirmed stream: read_confirmed)
    {"potential map", SAMPLER_AT(pm), pmap_advance, pmap_free},
    // ... and the wave recorder, a sixth: the label plane and the slot plane are scratch that every sample rewrites before it
    // reads them (wave_label_kernel writes every label from the state, wave_root_kernel every slot that is read); the sample's
    // counts are zeroed in front of its kernels and its records initialised and filled whole; the slot follows from the counter.
    // A sample taken from a void slab is overwritten, counts, records and planes, when the replay takes it again.  No give-up
    // word is needed: nothing is accumulated across samples, and its kernels end on any state (no loop waits for anything).
    // With LINKS on (fibhip_waves_links_begin) one thing IS carried from sample to sample: `prev`, the label plane of the sample
    // before.  The row may still be rewound, by the beat recorder's argument below: the two link kernels read the give-up word
    // first and write nothing once a launch in front of them gave up — not prev, not the table, not the sample's slot — so
    // however many void samples were queued, prev stays the plane of the last GOOD sample (a double buffer of planes would not
    // do: several samples can stand unconfirmed); the replay, plain ticks with no word to look at, takes the lost samples again
    // IN ORDER from that plane, and their slots follow from the counter.  The four kernels in front stay ungated (`labels` is
    // scratch), and the row keeps its place: the launch order on a shared tick is tested
    {"wave", SAMPLER_AT(wv), waves_advance, waves_free},
    // these two ACCUMULATE (the fold and the short ring; the count, the open beat's peak, the ring): their kernels read the
    // give-up word first and write nothing once a launch in front of them gave up, and how far they have come follows from the
    // counter alone — the replay takes the lost samples and issues the lost folds again, in order.  Neither ever fills up
    {"spectrum", SAMPLER_AT(sp), spectrum_advance, spectrum_free},
    {"beat", SAMPLER_AT(bt), beats_advance, beats_free},
    // it WRITES the state, the slab the launch wrote: stim_kernel reads the give-up word first, so the state the first lost
    // launch started from stays intact; the replay applies the events of the replayed ticks again, and no others — the events
    // of older ticks stand in the restored state.  Its rewind recomputes `next` (recorders_rewind)
    {"stimulus", NO_SAMPLER, stim_advance, stim_free, stim_on, stim_rewind},
    // its automaton's state is the log itself, row s a pure function of row s - 1 and the state.  The rows the lost samples
    // wrote were made from a void slab, and the gated apply behind them wrote nothing (it reads the give-up word first).  The
    // replay rewrites those rows IN ORDER, each from a predecessor that is older than the lost launch (good: trig_begin
    // confirms before it attaches) or has just been rewritten: no detection lost, none doubled, and a delay or a train that
    // straddles the lost launch goes on as in the untouched run
    {"trigger", SAMPLER_AT(trig), trig_advance, trig_free},
    // the lesion program, LAST: the geometry a lesion leaves belongs to the next tick, so every sample of the event tick — the
    // lead recorder's, whose source term reads the handle's phase planes, included — and every stimulus of it sees the geometry
    // the tick was computed with.  It WRITES the phase field, which no tick writes; the stimulus row's argument carries over:
    // lesion_apply_kernel reads the give-up word first, so the field the first lost launch started from stays intact — every
    // launch behind the one that gave up left without writing, and so did every lesion queued behind those; an event OLDER than
    // the first lost launch stands in the field and is not applied again, because what is due follows from `k` alone and `next`
    // is formed afresh from the rewound `k` (lesion_rewind); the replay, plain ticks behind a confirmed stream, applies the
    // events of the replayed ticks again, in order, and no others.  lesion_prep_kernel is ungated: it is a pure function of phi
    // (idempotent), and behind an apply that wrote nothing it rewrites the values that stand there
    {"lesion", NO_SAMPLER, lesion_advance, lesion_free, lesion_on, lesion_rewind},
};
#undef SAMPLER_AT
#pragma clang diagnostic pop

static inline Sampler *sampler_of(fibhip_ctx *h, const Recorder &r)
{
    return r.sampler == NO_SAMPLER ? nullptr : reinterpret_cast<Sampler *>(reinterpret_cast<char *>(h) + r.sampler);
}
static inline const Sampler *sampler_of(const fibhip_ctx *h, const Recorder &r) { return sampler_of(const_cast<fibhip_ctx *>(h), r); }
static inline bool attached(const fibhip_ctx *h, const Recorder &r)
{
    const Sampler *s = sampler_of(h, r);
    return s ? s->on : r.on(h);
}

// the hooks behind a launch of `ticks` ticks the handle's state has moved with.  `behind_mt`: that launch is a multi-tick launch
// nobody may have confirmed — the hooks that accumulate or write the state hand their kernels the give-up word then.  A plain
// tick never stands behind an unconfirmed multi-tick launch (tick_mt, fibhip_step and recover() confirm first)
static int recorders_advance(fibhip_ctx *h, int ticks, bool behind_mt)
{
    for (const Recorder &r : RECORDERS)
        if (attached(h, r))
            if (int rc = r.advance(h, ticks, behind_mt)) return rc;
    return 0;
}

// recover(): the samples and stimuli queued behind the lost launches were taken from, or kept off, a void slab; the replay
// (tick_now -> commit_impl) comes through the hooks again.  (Every journal record is younger than every recorder: each _begin
// confirms, and so empties the journal, before it attaches.)
static void recorders_rewind(fibhip_ctx *h, int lost)
{
    for (const Recorder &r : RECORDERS) {
        if (!attached(h, r)) continue;
        if (Sampler *s = sampler_of(h, r)) {
            s->rewind(lost);
        } else {
            r.rewind(h, lost);
        }
    }
}

static void recorders_free(fibhip_ctx *h)
{
    for (const Recorder &r : RECORDERS) r.release(h);
}
