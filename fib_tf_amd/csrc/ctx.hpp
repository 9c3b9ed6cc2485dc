// ctx.hpp — the handle behind fibhip_t: what it owns, grouped by who changes it, and the few helpers every file reads it with.
#pragma once
#include "sampler.hpp"

constexpr int MT_MAX_TICKS = 32;          // default bound on the ticks of one launch of a predicted or undeclared series
constexpr int MT_MAX_TICKS_DECLARED = 256;      // ... of a launch whose ticks the caller has all DECLARED (fibhip_expect): the smallest setting
                                                // within 0.3 % of the best measured one (profiles/series_launch_ab.txt); see launch_cap
// A declaration shorter than this keeps the launches it had, MT_MAX_TICKS at a time (run() with a frame every 10 ticks, the
// 20-tick regions of the driver, a 70-tick series as 32 + 32 + 6): the gain was measured on series of thousands of ticks, and
// the launches of short declared series are what their callers and the suite have seen so far.
constexpr int MT_DECLARED_MIN_TICKS = 128;
constexpr int MT_MAX_TICKS_ENV = 4096;          // the most FIBHIP_MT_MAX accepts (MT_CANCEL, 0xFFFF, is not a tick count)
// ticks in unconfirmed launches before the stream is drained once (journal_bound): what 256 launches of MT_MAX_TICKS hold,
// 0.1 s of Fenton 512x512 — whatever waits behind them (confirm(), the frame poll of ahead_read_back) waits that long at most
constexpr int MT_MAX_TICKS_IN_FLIGHT = 256 * MT_MAX_TICKS;
static_assert(MT_MAX_TICKS <= MT_MAX_TICKS_DECLARED && MT_MAX_TICKS_DECLARED <= MT_MAX_TICKS_ENV && MT_MAX_TICKS_ENV < (int)MT_CANCEL,
              "a launch's tick count shares its 16 bits with MT_CANCEL");
constexpr int AT_MT_TICKS = 8;           // autotune times a multi-tick candidate as one launch of this many ticks
static const char *const MT_DEAD_MSG =
    "a multi-tick launch gave up (a tile waited its full bound for a neighbouring tile: were all workgroups resident? is another "
    "process holding the GPU?) and the state it started from could not be restored; the state of this handle is void — "
    "FIBHIP_MT=0 runs one launch per tick";

struct PlanItem {
    int K;
    launch_fn fn;
    int TY, TX;
    const Variant *v = nullptr;     // the table entry it came from (run-time module kernels carry their launch data there)
};

// a traced model's device code loaded at run time (fibhip_module_load)
struct fibhip_module {
    hipModule_t mod = nullptr;
    int device = 0;
    int nvar = 0, spt = 1, nmodes = 1, consts_bytes = 4;
    unsigned masks[8] = {0};
    int K = 1, TX = 64, TY = 4, R = 3, TYB = 0, K2 = 1, TX2 = 64, TY2 = 4, R2 = 4;   // plan hints of the generated header
    std::vector<Variant> variants;
};

// ---- the scheduler's state (sched.inc) ---------------------------------------------------------------------------------
// several TICKS per launch (strip_mt_kernel): grids whose tiles are all resident at once, one device, planar slab
struct MtState {
    float *xbuf;            // exchange buffer of 16-byte cells [2][nvar/4][cells], allocated on first use
    unsigned *epochs;       // one epoch word per tile, 256 bytes apart, + three words behind them (MtArgs::err)
    unsigned epoch_base;    // value of every epoch word between two launches
    bool stale;             // the tiling may have changed since the words were last written: zero them first
    int max;                // most ticks one launch advances (<= 1: never)
    int max_declared;       // ... when the caller has declared every one of them (>= max by default; FIBHIP_MT_MAX sets both; 1 with max)
    int cur;                // ticks the next launch waits for: 1 after any observation of the state, then see fibhip_step
    unsigned *snap_flags;   // page-locked: one word per tile, raised by the tiles of a launch that carries a read-back
    unsigned *snap_flags_dev;       // device address of snap_flags
    unsigned *host_word;    // page-locked (behind snap_flags), read by tile 0 over PCIe: {launch id << 16 | n}, see ahead_settle
    unsigned ids;           // launch ids cycle through 1 .. ids
    const Variant *last_v;  // shape of the last multi-tick launch that was not a trial (mt_launch: another shape zeroes the words first)
    unsigned seq;           // id of the last multi-tick launch (the host's word names the launch it is meant for)
    bool inflight;          // a multi-tick launch has been issued since the give-up word was last read
    unsigned wait_ms;       // a tile's bound on its wait for a neighbour (FIBHIP_MT_WAIT_MS, fibhip_set_mt_wait_ms); 0 = 2 s
    long long n_launches, n_ticks;  // fibhip_launch_stats

    // the three words behind the tiles' epoch words, MT_EPOCH_STRIDE apart: [0] the id of a launch whose tile gave up,
    // [1] the host's word as tile 0 passed it on, [2] the tiles that stopped at the tick the host named
    unsigned *give_up_word() const { return epochs + (size_t)MT_MAX_TILES * MT_EPOCH_STRIDE; }
    unsigned *stop_count_word() const { return give_up_word() + 2 * MT_EPOCH_STRIDE; }
    static constexpr size_t tail_bytes() { return 3 * MT_EPOCH_STRIDE * sizeof(unsigned); }
    static constexpr size_t words_bytes() { return (size_t)MT_MAX_TILES * MT_EPOCH_STRIDE * sizeof(unsigned) + tail_bytes(); }
    // the host-side word a tile that gave up writes its launch's id into (behind host_word)
    unsigned *host_give_up() const { return host_word + MT_GIVEUP_WORD; }
};

// the caller's series: the ticks between two observations of the state
struct Series {
    int run;                // ticks launched since the last observation of the state
    int hist[8], nhist;     // lengths of the last series of ticks, oldest first (predict_series)
    bool fresh;             // ticks have run since the last observation of the state
    bool trust;             // the caller has not broken a predicted series since its last two equal ones
    int expect;             // ticks the caller has DECLARED to come in one series (fibhip_expect) and that have not been asked for yet, or 0
    int covered;            // the last so many of the `pending` ticks were declared when fibhip_step accepted them
    bool expect_fresh;      // ... none of them has been asked for yet: the observation the caller makes first does not end the series
    bool expect_long;       // the declaration held MT_DECLARED_MIN_TICKS or more when it was made: its launches take the declared cap
};

// run-ahead: a caller that alternates series of n ticks with ONE read-back (run() with image() every n ticks) gets the
// next n ticks launched BEFORE the read-back's copy is waited for; see ahead_read_back
struct Ahead {
    bool ok;                // nothing forbids it for good: not FIBHIP_AHEAD=0, not a caller-owned slab (fibhip_create), and no
                            // raw pointer handed out (fibhip_state_ptr) — a caller that can write the state at any time
    int n, used;            // ticks computed ahead of the caller / how many of them fibhip_step has handed out
    unsigned id;            // ... of the launch that ran ahead
    const Variant *v;       // ... and the shape it runs
    int nxt[FIB_MAXVAR];    // where the state lives once all of them are handed out
    hipEvent_t ev;
    unsigned snap_seq;
    long long n_kept, n_redone;     // series launched ahead that the caller cut short: stopped in time / recomputed
};

// A multi-tick launch that gives up must not cost the run (ionic.py:202-204 has no such failure).  Every such launch since
// the stream was last known good is remembered with the buffers it READ: a launch writes the other slab only and the
// launches queued behind a failed one find the give-up word at their first boundary and leave without writing, so the
// state the FIRST failed launch started from is intact when the host finds out (`recover`).
struct MtRec {
    unsigned id;        // the launch's id (the give-up word names it)
    int T;              // ticks it advances (a launch that ran ahead and was stopped in time: the ticks it did)
    bool counted;       // the handle's state has moved past these ticks (false: a run-ahead not handed out yet)
    int src[FIB_MAXVAR];
};
struct Journal {
    std::vector<MtRec> recs;
    long long ticks;        // ... and the ticks they hold (journal_bound)
    bool recovering;
    long long n_fallbacks, n_replayed;      // launches that gave up and were recovered / ticks recomputed one launch per tick
    long fake_giveup_at, fake_seen;         // test switch FIBHIP_MT_FAKE_GIVEUP=n: the n-th multi-tick launch finds the give-up word raised
};

// ---- the recorders (record.inc) ----------------------------------------------------------------------------------------
// Every recorder but the activation recorder and the two event-driven programs (stimulus, lesion) is a Sampler (sampler.hpp): `on`, `every`, `k` — the ticks
// LAUNCHED since it was attached, which recover() rewinds by the ticks it replays — and `cap`.  recorders.hpp lists them in hook
// order; what they ask of the scheduler is stated in sched.inc.

// activation recorder (fibhip_observe_begin): while `on`, commit_impl enqueues observe_kernel behind every tick
struct ObsRec {
    bool on;
    int var;
    float up, down;
    float *buf;             // 6 planes of `cells` (W-pitched): Vp | first_up | last_up | prev_up | apd | count (int32)
    float *vel;             // fibhip_observe_velocity's four maps, `cells` each: made on first use, freed with the recorder
    long long k;            // observed ticks since the recorder was attached
};
// electrode recorder (fibhip_electrode_begin): electrode_kernel behind the launch that ends a sample tick
struct ElRec : Sampler {
    int var, n;
    int nchunks, ncomb;     // workgroups of electrode_kernel / of electrode_combine_kernel (0: no electrode has several chunks)
    ElChunk *chunks;        // device: the chunk table
    ElComb *comb;           // device: the electrodes of several chunks
    float *w;               // device: the weight patches, back to back
    float *part;            // device: one partial per chunk of such electrodes
    float *trace;           // device: [cap][n]
};
// tip recorder (fibhip_tips_begin): tip_kernel behind the launch that ends a sample tick
struct TipRec : Sampler {
    int var, var2, max_tips;
    float a0, b0;
    unsigned char *mask;    // device: [H][W], or null (every plaquette counts)
    int *counts;            // device: [cap][3] = n_pos, n_neg, stored
    int *records;           // device: [cap][max_tips][4] = row, col, charge, 0
};

// the pixel plane the frame, spectrum and beat recorders sample: a window of the grid cut into blocks, one pixel per block
struct Window {
    int r0, c0, oh, ow, by, bx;     // the window's first cell, the plane's shape in pixels, the block
    int reduce;                     // FIBHIP_FRAME_POINT / _MEAN
    float *w;                       // device: the weight plane [H][W], or null
    size_t npix() const { return (size_t)oh * (size_t)ow; }
};

// frame recorder (fibhip_frames_begin): frame_kernel behind the launch that ends a sample tick.  Its counter starts at
// every - first, so that its first sample may come early
struct FrRec : Sampler, Window {
    int var;
    int format;             // FIBHIP_FRAME_F32 / _U8
    float lo, span;
    unsigned char *cube;    // device: [cap][oh][ow] float32 or uint8
    size_t frame_bytes() const { return npix() * (format == FIBHIP_FRAME_U8 ? 1u : 4u); }
};

// statistics recorder (fibhip_stats_begin): stats_kernel and stats_combine_kernel behind the launch that ends a sample tick
struct StRec : Sampler {
    int ncols, narr;
    int vars[FIB_MAXVAR];   // the distinct arrays the columns name, in order of first appearance
    int nchunks;            // chunks of one array: stats_kernel's grid is (nchunks, narr)
    StChunk *chunks;        // device: the chunk table
    StArr *arrs;            // device: the columns of every array
    StCol *cols;            // device: where column c of a row comes from
    float *w;               // device: the weight plane [H][W], or null
    unsigned char *mask;    // device: [H][W], or null
    unsigned long long *part;       // device: [narr][ST_SLOTS][nchunks], one partial per (column, chunk)
    double *trace;          // device: [cap][ncols]
};

// lead recorder (fibhip_leads_begin): lead_kernel and lead_combine_kernel behind the launch that ends a sample tick.  Both rewrite
// whole slots (the partials, the sample's row) from the state alone
struct LeadRec : Sampler {
    int var, n;
    int tiles_x, tiles_y;   // lead_kernel's grid, from H and W alone
    int *pos;               // device: [n][4] = row, col, table, 0
    float *tables;          // device: [ntables][H][W]
    float *weight;          // device: the weight plane [H][W], or null (weight 1)
    double *part;           // device: [n][tiles_x * tiles_y], one partial per (lead, tile)
    double *rows;           // device: [cap][n]
};

// potential-map recorder (fibhip_pmap_begin): pmap_source_kernel and pmap_conv_kernel behind the launch that ends a sample tick.
// Both rewrite whole slots (every cell of the scratch plane, every site of the sample's slot) from the state alone
struct PMapRec : Sampler {
    int var, R;
    int r0, c0, sy, sx, oh, ow;     // the lattice: site (i, j) at the cell (r0 + i * sy, c0 + j * sx)
    int pw, roww, slab;             // pmap_conv_kernel's LDS layout, from R and sx alone
    float *weight;          // device: the weight plane [H][W], or null (weight 1)
    double *tab;            // device: [R + 1][2R + 1], the table's rows in float64, mirrored about dc = 0
    float *q;               // device: the source plane [H + 2R][W + 2R], R zeros on every side
    double *cube;           // device: [cap][oh][ow]
    double *maps;           // device: the summary's planes, 3 x float64 [oh][ow] then 3 x int32 [oh][ow]
    size_t npix() const { return (size_t)oh * (size_t)ow; }
};

// wave recorder (fibhip_waves_begin): wave_label_kernel, wave_merge_kernel, wave_root_kernel and wave_reduce_kernel behind the
// launch that ends a sample tick.  The two planes are scratch that every sample rewrites before it reads them; the sample's
// counts are zeroed and its records written whole
struct WaveRec : Sampler {
    int var, var2, kind, kind2, conn, max_waves;
    float level, level2;
    unsigned char *mask;    // device: [H][W], or null (every cell counts)
    int *labels;            // device: [H][W], the label plane of the latest sample
    int *slots;             // device: [H][W], a root's slot in its sample's records
    int *counts;            // device: [cap][3] = n, stored, cells
    WaveRecord *records;    // device: [cap][max_waves]
    // links (fibhip_waves_links_begin; max_links = 0: off): `prev` is the ONE thing here that is carried from sample to sample.
    // The two link kernels read the give-up word first and write nothing once a launch in front of them gave up, so it stays
    // the label plane of the last good sample until the replay takes the lost samples again, in order
    int max_links;
    unsigned link_entries;  // T: the smallest power of two >= 4 * max_links
    int *prev;              // device: [H][W], the label plane of the sample before (-1 everywhere before the first)
    unsigned long long *link_table;     // device: T keys (pair + 1; 0: empty), then T int32 cell counts; scratch of one sample
    int *link_counts;       // device: [cap][4] = links, stored, cells, lost
    WaveLink *link_records; // device: [cap][max_links]
};

// spectrum recorder (fibhip_spectrum_begin): spectrum_sample_kernel behind the launch that ends a sample tick and, behind the
// sample that fills the ring, spectrum_fold_kernel.  It ACCUMULATES: both kernels read the give-up word first, and everything
// about its progress follows from `k` alone — samples k / every, the ring slot and the segment position of a sample, the folds
// issued samples / chunk, the segments samples / nfft — so a rewind of `k` leaves nothing behind.  It never fills up
struct SpRec : Sampler, Window {
    int var;
    int nfft, nb, chunk;
    float *win;             // device: [nfft]
    float *tw;              // device: [nfft][2]
    int *bins;              // device: [nb]
    float *ring;            // device: [chunk][oh][ow]
    float *acc;             // device: Re | Im | P, each [nb][oh][ow]
    float *maps;            // device: kpeak (int32) | ppeak | pband | pnear, each [oh][ow]
};

// beat recorder (fibhip_beats_begin): beat_kernel behind the launch that ends a sample tick.  It ACCUMULATES (the count, the
// open beat's peak, the ring): the kernel reads the give-up word first, and the sample index — with it t0 — follows from `k`
// alone, so a rewind of `k` leaves nothing behind.  A ring never fills up
struct BeatRec : Sampler, Window {
    int var;
    float up, down;
    int depth;
    float *state;           // device: xp | pk | n (int32), each [oh][ow]
    float *ring;            // device: t_up | t_down | peak, each [depth][oh][ow]
    float *maps;            // device: nused (int32) | apd_mean | cl_mean | apd_alt, each [oh][ow]
};

// stimulus program (fibhip_stim_begin): the actuator beside the recorders, driven by its events and not by a stride — no launch
// spans an event tick (stim_room, a term of sample_room), and stim_kernel goes behind the launch that ends one, behind the
// samples of that tick
struct StimEntry {
    int var, mode;
    long long first, period, count, hold;   // fibhip_stim_entry's, validated
    int plane;              // index into StimRec::planes, or -1: a rectangle
    int r0, r1, c0, c1;     // rectangle
    float v, floor;
    int b_r0, b_r1, b_c0, b_c1;     // the visit box (empty: b_r0 == b_r1), cut at attach
    bool slow;              // Courtemanche on aggregates: the entry names an array the aggregates are formed from
};
struct StimRec {
    bool on;
    long long k;            // ticks LAUNCHED since the program was attached (recover() rewinds it by the ticks it replays)
    long long next;         // the tick count (k) of the next event tick, LLONG_MAX: no event left; follows from k and the entries
                            // alone (stim_next): set at attach, in stim_advance and in recover()
    std::vector<StimEntry> entries;
    float *planes;          // device: the planes, [nplanes][H][W], or null
};

// trigger program (fibhip_trig_begin): the closed loop — a sampler whose hook (behind the stimulus program's) enqueues
// sense_kernel, trigger_kernel and the gated apply behind the launch that ends a sample tick.  The automaton's state IS the log
// on the device: row s follows from row s - 1 and the state alone, and the host knows only the slot
struct TrigRec : Sampler {
    int nsensors, nrules;
    bool cut_vec;           // the item tables' [1] entries may be used (pitch == W, W a multiple of 4)
    int max_chunks[2];      // sense_kernel's grid.x, scalar / VEC
    std::vector<StimEntry> stims;   // rule r's stimulus (first / period / count / hold unused: the automaton times it)
    int vars[TRIG_MAX];     // the sensors' arrays
    SenseSite *sites;       // device: the sensors
    TrigRule *rules;        // device: the rules
    unsigned char *masks;   // device: the mask sensors' masks, [nmasks][H][W], or null
    float *planes;          // device: the stimulus planes, [nplanes][H][W], or null
    unsigned *part;         // device: [nsensors][SENSE_MAX_CHUNKS]
    int *rows;              // device: [cap][nrules][TRIG_ROW]
    unsigned *fire;         // device: [cap], bit r: rule r fires after sample s
};

// lesion program (fibhip_lesion_begin): the second event-driven actuator — its hook writes the PHASE FIELD, not the state.  No
// Sampler, like StimRec: no launch spans an event tick (lesion_room, a term of sample_room), and lesion_apply_kernel and
// lesion_prep_kernel go behind the launch that ends one, behind every sample and stimulus of that tick (the last row of
// RECORDERS: the geometry a lesion leaves belongs to the next tick)
struct LesionEntry {
    long long tick;         // applied right after tick `tick` since attach: when k == tick + 1
    int r0, r1, c0, c1;     // the box
    size_t off;             // where its patch starts in LesionRec::patches, in floats
};
struct LesionRec {
    bool on;
    long long k;            // ticks LAUNCHED since the program was attached (recover() rewinds it by the ticks it replays)
    long long next;         // the tick count (k) of the next event tick, LLONG_MAX: no event left; follows from k and the entries
                            // alone (lesion_next): set at attach, in lesion_advance and in recover()
    std::vector<LesionEntry> entries;
    float *patches;         // device: the patches, packed back to back
};

// fibhip_trace_begin / _end: the launches in between, each between two HIP events
struct TraceRec {
    hipEvent_t e0, e1;
    char name[96];
    int K, TX, TY, R, ticks;
};

struct fibhip_ctx {
    fibhip_desc d;
    int nvar, spt, mode;
    size_t cells;
    int pitch;              // floats between rows of one state array (W planar, nvar*W row-interleaved)
    size_t vstride;         // floats between the first rows of consecutive state arrays (cells / W)
    hipStream_t s0, s1;
    bool own_s0;
    float *slab[2];
    bool own_slab;
    float *phase3;          // dpy | dpx | q4 | r4 | dpy*r4 | dpx*r4, each `cells` floats
    float *phi_dev;
    bool has_phase;
    bool phi_floored;       // phi >= 1e-5f everywhere has been checked for the field that stands (lesion_field_ready; set_phase resets it)
    int cur[FIB_MAXVAR];            // which slab holds variable v
    int nxt[FIB_MAXVAR];            // where the tick in flight writes it (valid between edges and commit)
    bool has_consts;
    Fenton::Consts kf;
    BeelerReuter::Consts kb;
    Courtemanche::Consts kc;
#ifdef FIB_CUSTOM_MODEL_INC
    Custom::Consts ku;
#endif
    // ---- the plan (plan.inc) ----
    std::vector<PlanItem> plan;
    std::vector<PlanItem> plan_multi[4];    // [T]: the one-launch plan of T ticks, T = 2..multi_max
    int multi_max;          // up to this many consecutive ticks go into one launch (1 = never; CourtAgg: 3)
    launch_fn fused_fn;     // Courtemanche: tick + 'slow' in one launch, or null
    const Variant *period_v;        // the exchange-period row multi-tick launches run (sched.inc mt_variant) beside `plan`, or null
    bool period_forced;             // ... because the caller forced it (FIBHIP_VARIANT, FIBHIP_K): it runs EVERY multi-tick launch
    bool tuned;             // the plan has been checked against the other tile shapes on this very geometry (autotune)
    int ncu;                // compute units of the device
    fibhip_module *mod;     // FIBHIP_CUSTOM on a run-time module (fibhip_module_load), or null
    // ---- one tick (tick.inc) ----
    hipEvent_t ev_main, ev_int, ev_t0, ev_t1;
    int phase_of_tick;      // 0 idle, 1 edges issued, 2 interior issued
    long launches, t_launches0;
    long long n_ticks;      // fibhip_launch_stats
    int own0, own1;         // owned local rows
    bool whole_in_edges;    // this tick's last launch was issued entirely by step_edges
    int cycle, cpos;        // ghost zone = cycle * steps_per_tick rows: the halo is exchanged every `cycle` ticks;
                            // cpos = ticks done since the last exchange
    int span;               // ticks the launch being issued covers (1; T while tick_multi fuses T Courtemanche ticks)
    // ---- the scheduler (sched.inc) ----
    int pending;            // ticks fibhip_step has accepted but not launched yet (see fibhip_step)
    MtState mt;
    Series series;
    Ahead ahead;
    Journal journal;
    bool dead;              // a multi-tick launch gave up waiting and the state could not be restored: void
    // ---- the recorders (record.inc) ----
    ObsRec obs;
    ElRec el;
    TipRec tip;
    FrRec fr;
    StRec st;
    LeadRec ld;
    PMapRec pm;
    WaveRec wv;
    SpRec sp;
    BeatRec bt;
    StimRec stim;
    TrigRec trig;
    LesionRec les;
    std::vector<TraceRec> trace;
    bool tracing;
    // ---- the rest ----
    DoneWord done;          // sync_s0's way of noticing the end of the stream's work
    void *comm;             // ncclComm_t of the direct halo path (fibhip_comm_*), or null
    float *probe_host;      // pinned
    float *stage;           // pinned staging buffer for get_state/set_state (one array), allocated on first use
    // Courtemanche, fast policy: the fast tick reads five per-cell aggregates of the slow
    // variables (models.hpp CourtAgg) instead of the variables themselves.  'slow' rewrites them; any other write to the
    // state (set_state) marks them stale and the next tick recomputes them first.
    float *agg;             // CourtAgg::NAGG arrays laid out like the state arrays (planar, or row-interleaved at the
    size_t agg_stride;      // slab's pitch on row-block shards), `agg_stride` floats apart; or null
    bool use_agg, agg_dirty;
    bool agg_ghost_dirty;   // row-block shards: a halo exchange has rewritten the ghost rows' slow variables
    // ---- per-cell diffusion tensors (fibhip_set_tensor) ----
    float *tensor;          // dyy | dxx | dxy | wy | wx | wa | wb | wc, each `cells` floats; null until a tensor is first set
    bool has_tensor;        // a tensor stands: the plan comes from g_tensor_variants, and phase3 holds tensor_prep_kernel's planes
    bool agg_held;          // use_agg as it stood when the tensor was set (a tensor handle runs Courtemanche's plain modes)
    Tensor<Fenton>::Consts tkf;             // what a tensor kernel is launched with: the model's constants as they stand at the
    Tensor<BeelerReuter>::Consts tkb;       // launch, and the five weight planes (tick_consts_of)
    Tensor<Courtemanche>::Consts tkc;
};

static const void *consts_of(fibhip_ctx *h)
{
    if (h->mod) return nullptr;                    // generated models carry their constants as literals
    switch (h->d.model) {
    case FIBHIP_FENTON4V: return &h->kf;
    case FIBHIP_BR: return &h->kb;
#ifdef FIB_CUSTOM_MODEL_INC
    case FIBHIP_CUSTOM: return &h->ku;
#endif
    default: return &h->kc;
    }
}

// ... of a launch of the handle's PLAN: a tensor handle's kernels take Tensor<M>::Consts
static const void *tick_consts_of(fibhip_ctx *h)
{
    if (!h->has_tensor) return consts_of(h);
    const float *w = h->tensor + 3 * h->cells;
    auto planes = [&](auto &k) {
        k.wy = w;
        k.wx = w + h->cells;
        k.wa = w + 2 * h->cells;
        k.wb = w + 3 * h->cells;
        k.wc = w + 4 * h->cells;
        return (const void *)&k;
    };
    switch (h->d.model) {
    case FIBHIP_FENTON4V: h->tkf.m = h->kf; return planes(h->tkf);
    case FIBHIP_BR: h->tkb.m = h->kb; return planes(h->tkb);
    default: h->tkc.m = h->kc; return planes(h->tkc);
    }
}

static Geo base_geo(const fibhip_ctx *h)
{
    Geo g;
    g.H = h->d.height;
    g.W = h->d.width;
    g.pitch = h->pitch;
    g.Hg = h->d.global_height;
    g.row_off = h->d.row_offset;
    g.r0 = 0;
    g.r1 = h->d.height;
    g.rb0 = g.rb1 = 0;
    g.ty_a = 0;
    g.tiles_x = g.ntiles = 0;
    return g;
}

// tiles of TX x TY that cover `rows` rows of the handle's width (rows < 0: the whole block)
static inline long tiles_of(const fibhip_ctx *h, int TX, int TY, long rows = -1)
{
    if (rows < 0) rows = h->d.height;
    return (long)((h->d.width + TX - 1) / TX) * ((rows + TY - 1) / TY);
}

static inline bool is_shard(const fibhip_ctx *h) { return h->d.ghost_top || h->d.ghost_bottom; }
// the shallower ghost zone of the sides that have one (0: no ghost rows at all)
static inline int min_ghost(const fibhip_desc &d)
{
    return (d.ghost_top && d.ghost_bottom) ? imin(d.ghost_top, d.ghost_bottom) : imax(d.ghost_top, d.ghost_bottom);
}

// `c` launches a kernel of the handle's run-time module through launch_module, which lays the arguments out from these
static inline void module_kernel(LaunchCtx &c, const fibhip_ctx *h, hipFunction_t kern, int kind, const Variant *v)
{
    c.kern = kern;
    c.kind = kind;
    c.K = v->K; c.TX = v->TX; c.TY = v->TY; c.NT = v->NT;
    c.nvar = h->nvar;
    c.consts_bytes = h->mod ? h->mod->consts_bytes : 0;
}

// ---- what every entry point starts with ---------------------------------------------------------------------------------
#define NEED(h)                                                  \
    do {                                                         \
        if (!(h)) return fail(FIBHIP_EINVAL, "null handle");     \
        if ((h)->dead) return fail(FIBHIP_EHIP, "%s", MT_DEAD_MSG);  \
        HIPCHK(hipSetDevice((h)->d.device));                     \
    } while (0)
// launches the ticks fibhip_step may have left pending (sched.inc `flush`); every entry point that observes or changes the
// state starts with it
#define FLUSH(h)                                                                                   \
    do {                                                                                           \
        if (int rc_ = flush(h)) return rc_;                                                        \
    } while (0)
// waits until no unconfirmed multi-tick launch is in flight (sched.inc `confirm`): in front of whatever writes the state
#define CONFIRM(h)                                                                                 \
    do {                                                                                           \
        if (int rc_ = confirm(h)) return rc_;                                                      \
    } while (0)
// waits for everything enqueued on the handle's stream; recovers from a multi-tick launch that gave up (sched.inc `sync_s0`)
#define SYNC_S0(h)                                                                                 \
    do {                                                                                           \
        if (int rc_ = sync_s0(h)) return rc_;                                                      \
    } while (0)

// ---- timeline (fibhip_trace_begin / _end) ------------------------------------------------------------------------------
static int trace_open(fibhip_ctx *h, hipStream_t st, const char *family, int K, int TX, int TY, int NT, int ticks)
{
    if (!h->tracing) return 0;
    TraceRec r;
    r.e0 = r.e1 = nullptr;
    HIPCHK(hipEventCreate(&r.e0));
    HIPCHK(hipEventCreate(&r.e1));
    r.K = K; r.TX = TX; r.TY = TY; r.R = NT < 0 ? (NT < -32 ? -NT - 32 : -NT) : 0; r.ticks = ticks;
    if (TX > 0 && NT < 0)
        snprintf(r.name, sizeof r.name, "%s<K=%d, tile %dx%d, %d rows per wave%s>", family, K, TX, TY, r.R,
                 ticks > 1 ? ", several ticks" : "");
    else if (TX > 0)
        snprintf(r.name, sizeof r.name, "%s<K=%d, tile %dx%d, %d threads>", family, K, TX, TY, NT);
    else
        snprintf(r.name, sizeof r.name, "%s", family);
    HIPCHK(hipEventRecord(r.e0, st));
    h->trace.push_back(r);
    return 0;
}
static int trace_close(fibhip_ctx *h, hipStream_t st)
{
    if (!h->tracing || h->trace.empty()) return 0;
    HIPCHK(hipEventRecord(h->trace.back().e1, st));
    return 0;
}
