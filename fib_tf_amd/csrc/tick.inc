// tick.inc — ONE tick: which buffers a launch reads and writes, the launches of the plan over the rows they have to produce,
// and the edges / interior / commit phases the row-block driver interleaves its halo exchange with.
// (included by fibhip.hip)

static int autotune(fibhip_ctx *h);                               // plan.inc: the first tick of a handle chooses its plan
static int observe_enqueue(fibhip_ctx *h);                       // record.inc: the activation recorder's hook behind a committed tick

// ------------------------------------------------------------------------------------------
// stepping
// ------------------------------------------------------------------------------------------
// Buffer rule for one launch: the potential always ping-pongs (its neighbours are read by other
// workgroups).  When the launch fuses K > 1 sub-steps every variable ping-pongs, because the halo
// cells of a tile are owned (and rewritten) by a neighbouring tile.  With K == 1 the pointwise
// variables are read and written by the same thread only, so they are updated in place — which is
// also what lets Courtemanche's fast tick assign 4 of its 21 arrays and leave the rest untouched.
// which variables the tick op of this handle assigns (M::mask(mode))
static unsigned tick_mask(const fibhip_ctx *h)
{
    if (h->mod) return h->mod->masks[h->mode];
    switch (h->d.model) {
    case FIBHIP_FENTON4V: return Fenton::mask(h->mode);
    case FIBHIP_BR: return BeelerReuter::mask(h->mode);
    case FIBHIP_COURT: return h->use_agg ? CourtAgg::mask(h->mode) : Courtemanche::mask(h->mode);
    case FIBHIP_COURT_US: return CourtemancheUS::mask(h->mode);
#ifdef FIB_CUSTOM_MODEL_INC
    case FIBHIP_CUSTOM: return Custom::mask(h->mode);
#endif
    default: return ~0u;
    }
}

// the aggregate arrays follow the state arrays in the pointer table of the CourtAgg kernels (read and written in place)
static void agg_ptrs(const fibhip_ctx *h, LaunchCtx &c)
{
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
    if (!h->use_agg) return;
    for (int a = 0; a < CourtAgg::NAGG; ++a)
        c.in[Courtemanche::NVAR + a] = c.out[Courtemanche::NVAR + a] = h->agg + (size_t)a * h->agg_stride;
#endif
}

static void fill_ptrs(fibhip_ctx *h, LaunchCtx &c, int K, const int *cur, int *nxt)
{
    const unsigned wmask = tick_mask(h);
    for (int v = 0; v < h->nvar; ++v) {
        // a variable the op never assigns is read-only for the whole launch: it stays where it is (Courtemanche's
        // fast tick: 17 of 21 arrays)
        const bool flip = (v == 0) || (K > 1 && ((wmask >> v) & 1u));
        nxt[v] = flip ? (cur[v] ^ 1) : cur[v];
        c.in[v] = h->slab[cur[v]] + (size_t)v * h->vstride;
        c.out[v] = h->slab[nxt[v]] + (size_t)v * h->vstride;
    }
    agg_ptrs(h, c);
    c.ph.dpy = h->phase3;
    c.ph.dpx = h->phase3 + h->cells;
    c.ph.q4 = h->phase3 + 2 * h->cells;
    c.ph.r4 = h->phase3 + 3 * h->cells;
    c.ph.pyr = h->phase3 + 4 * h->cells;
    c.ph.pxr = h->phase3 + 5 * h->cells;
    c.ph.phi = h->phi_dev;
    c.consts = tick_consts_of(h);
}

static const char *family_of(const Variant *v)
{
    if (!v) return "kernel";
    if (v->kern) return v->kind == MK_POINTWISE ? "pointwise_kernel (generated)" : (v->kind == MK_STRIP ? "strip_kernel (generated)" : "tick_kernel (generated)");
    return v->NT < -32 ? "rows_kernel" : (v->NT < 0 ? "strip_kernel" : "tick_kernel");
}

// one launch over the rows [r0, r1) and, optionally, a second band [rb0, rb1)
static int launch_range(fibhip_ctx *h, hipStream_t st, const PlanItem &it, LaunchCtx &c, int r0, int r1, int rb0 = 0,
                        int rb1 = 0)
{
    if (r1 <= r0 && rb1 <= rb0) return 0;
    c.g = base_geo(h);
    c.g.r0 = r0;
    c.g.r1 = r1 > r0 ? r1 : r0;
    c.g.rb0 = rb0;
    c.g.rb1 = rb1 > rb0 ? rb1 : rb0;
    if (it.v && it.v->kern) module_kernel(c, h, it.v->kern, it.v->kind, it.v);
    if (int rc = trace_open(h, st, family_of(it.v), it.K, it.TX, it.TY, it.v ? it.v->NT : 0, it.K > h->spt ? it.K / h->spt : 1)) return rc;
    HIPCHK(it.fn(st, c));
    if (int rc = trace_close(h, st)) return rc;
    h->launches++;
    return 0;
}

// rows launch `l` of the plan has to produce: the owned rows grown by the sub-steps still to come
// (those rows are the halo of the later launches of the same tick), clipped to the slab
// Communication-avoiding ghost zone: with ghost = cycle * steps_per_tick rows the neighbours' rows are
// exchanged only every `cycle` ticks; tick j of a cycle also advances the (cycle-1-j) * spt ghost rows
// next to the owned block, which are the halo of the ticks still to come.
// (a launch that fuses `span` ticks leaves the rows the ticks AFTER it still need)
static inline int ext_rows(const fibhip_ctx *h) { return (h->cycle - h->cpos - h->span) * h->spt; }
static inline bool ends_cycle(const fibhip_ctx *h)
{
    return (h->d.ghost_top || h->d.ghost_bottom) && h->cpos + h->span == h->cycle;
}
// On the tick that ends a cycle the strips the neighbours wait for can be launched first (main stream) and
// the rest of the block on a second stream, so that the messages overlap the interior.  A fused launch is
// latency-bound (~20 us however few tiles it has; measured: the split costs a 512-row block 44 us per tick
// instead of 22), so it only pays when the interior is several rounds of CUs long.
static inline bool split_tick(const fibhip_ctx *h, const PlanItem &it)
{
    if (!ends_cycle(h)) return false;
    if (const char *e = getenv("FIBHIP_SPLIT")) return atoi(e) != 0;
    const int hw = imax(h->d.ghost_top, h->d.ghost_bottom);
    const int edge = ((hw + it.TY - 1) / it.TY) * it.TY;
    const long interior_rows = (long)(h->own1 - h->own0) - ((h->d.ghost_top ? edge : 0) + (h->d.ghost_bottom ? edge : 0));
    return interior_rows > 0 && tiles_of(h, it.TX, it.TY, interior_rows) >= 4 * 256;
}

static void rows_of_launch(const fibhip_ctx *h, size_t l, int &r0, int &r1)
{
    int rem = ext_rows(h);
    for (size_t m = l + 1; m < h->plan.size(); ++m) rem += h->plan[m].K;
    r0 = imax(0, h->own0 - (h->d.ghost_top ? rem : 0));
    r1 = imin(h->d.height, h->own1 + (h->d.ghost_bottom ? rem : 0));
}

static int check_ready(fibhip_ctx *h)
{
    if (!h->has_consts) return fail(FIBHIP_EINVAL, "Chebyshev table not set (fibhip_set_consts)");
    return 0;
}

// re-evaluation of the model on the current state, in place, without the stencil: assigns mask(mode)
static int run_pointwise_mode(fibhip_t h, launch_fn fn, const Variant *mv = nullptr, int row0 = -1, int row1 = -1)
{
    if (h->phase_of_tick) return fail(FIBHIP_EINVAL, "step_mode inside an open tick");
    LaunchCtx c;
    if (mv) module_kernel(c, h, mv->kern, MK_POINTWISE, mv);
    for (int v = 0; v < h->nvar; ++v) {
        c.in[v] = h->slab[h->cur[v]] + (size_t)v * h->vstride;
        c.out[v] = h->slab[h->cur[v]] + (size_t)v * h->vstride;   // in place
    }
    agg_ptrs(h, c);
    c.consts = consts_of(h);
    c.g = base_geo(h);
    // the ghost rows that later ticks of this cycle still advance must get the update too
    const int live = (h->cpos == 0 ? h->cycle : h->cycle - h->cpos) * h->spt;
    c.g.r0 = imax(0, h->own0 - (h->d.ghost_top ? live : 0));
    c.g.r1 = imin(h->d.height, h->own1 + (h->d.ghost_bottom ? live : 0));
    if (row0 >= 0) {                                      // an explicit band of rows instead
        c.g.r0 = row0;
        c.g.r1 = row1;
    }
    c.sub0 = 0;
    if (int rc = trace_open(h, h->s0, mv ? "pointwise_kernel (generated)" : "pointwise_kernel", 1, 0, 0, 0, 1)) return rc;
    HIPCHK(fn(h->s0, c));
    if (int rc = trace_close(h, h->s0)) return rc;
    h->launches++;
    return 0;
}

// Courtemanche on aggregates: recompute them if the state was written from outside since they were formed
static int refresh_agg(fibhip_t h)
{
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
    if (h->use_agg && h->agg_dirty) {
        if (int rc = run_pointwise_mode(h, launch_pointwise<CourtAgg, Fast, CourtAgg::MODE_AGG>, nullptr)) return rc;
        h->agg_dirty = false;
    }
    if (h->use_agg && h->agg_ghost_dirty) {               // the rows a neighbour's message has just replaced
        const launch_fn fn = launch_pointwise<CourtAgg, Fast, CourtAgg::MODE_AGG>;
        if (h->d.ghost_top)
            if (int rc = run_pointwise_mode(h, fn, nullptr, 0, h->d.ghost_top)) return rc;
        if (h->d.ghost_bottom)
            if (int rc = run_pointwise_mode(h, fn, nullptr, h->d.height - h->d.ghost_bottom, h->d.height)) return rc;
        h->agg_ghost_dirty = false;
    }
#endif
    return 0;
}

static int edges_impl(fibhip_t h)
{
    if (h->phase_of_tick != 0) return fail(FIBHIP_EINVAL, "step_edges: previous tick not committed");
    if (int rc = check_ready(h)) return rc;
    if (!h->tuned)
        if (int rc = autotune(h)) return rc;
    if (int rc = refresh_agg(h)) return rc;
    int cur[FIB_MAXVAR];
    memcpy(cur, h->cur, sizeof cur);
    int sub = 0;
    for (size_t l = 0; l < h->plan.size(); ++l) {
        const PlanItem &it = h->plan[l];
        LaunchCtx c;
        int nxt[FIB_MAXVAR];
        fill_ptrs(h, c, it.K, cur, nxt);
        c.sub0 = sub;
        int r0, r1;
        rows_of_launch(h, l, r0, r1);
        if (l + 1 < h->plan.size()) {
            if (int rc = launch_range(h, h->s0, it, c, r0, r1)) return rc;
            memcpy(cur, nxt, sizeof cur);
            sub += it.K;
            continue;
        }
        // last launch: only the strips a neighbour is waiting for — and only on the tick that ends a cycle.
        // The interior part (step_interior, second stream) depends on everything enqueued on s0 up to HERE
        // — the earlier launches of this tick and the previous tick's halo refresh — but not on the strips.
        const bool split = split_tick(h, it);
        h->whole_in_edges = ends_cycle(h) && !split;      // the caller exchanges right after step_edges:
        if (h->whole_in_edges) {                          // everything it sends must be computed by then
            if (int rc = launch_range(h, h->s0, it, c, r0, r1)) return rc;
        } else {
            if (split) HIPCHK(hipEventRecord(h->ev_main, h->s0));
            const int hw = split ? imax(h->d.ghost_top, h->d.ghost_bottom) : 0;
            const int e = hw > 0 ? ((hw + it.TY - 1) / it.TY) * it.TY : 0;
            int t1 = (hw && h->d.ghost_top) ? imin(r0 + e, r1) : r0;          // top strip [r0, t1)
            int b0 = (hw && h->d.ghost_bottom) ? imax(r1 - e, t1) : r1;        // bottom strip [b0, r1)
            if (int rc = launch_range(h, h->s0, it, c, r0, t1, b0, r1)) return rc;   // both strips, one launch
        }
        memcpy(h->nxt, nxt, sizeof nxt);
    }
    h->phase_of_tick = 1;
    return 0;
}

static int interior_impl(fibhip_t h)
{
    if (h->phase_of_tick != 1) return fail(FIBHIP_EINVAL, "step_interior: call step_edges first");
    if (h->whole_in_edges) {                              // step_edges already launched the whole block
        h->phase_of_tick = 2;
        return 0;
    }
    // recompute the last launch's geometry (same arithmetic as step_edges)
    int cur[FIB_MAXVAR];
    memcpy(cur, h->cur, sizeof cur);
    int sub = 0;
    for (size_t l = 0; l + 1 < h->plan.size(); ++l) {
        LaunchCtx tmp;
        int nxt[FIB_MAXVAR];
        fill_ptrs(h, tmp, h->plan[l].K, cur, nxt);
        memcpy(cur, nxt, sizeof cur);
        sub += h->plan[l].K;
    }
    const PlanItem &it = h->plan.back();
    LaunchCtx c;
    int nxt[FIB_MAXVAR];
    fill_ptrs(h, c, it.K, cur, nxt);
    c.sub0 = sub;
    int r0, r1;
    rows_of_launch(h, h->plan.size() - 1, r0, r1);
    const bool split = split_tick(h, it);
    const int hw = split ? imax(h->d.ghost_top, h->d.ghost_bottom) : 0;
    const int e = hw > 0 ? ((hw + it.TY - 1) / it.TY) * it.TY : 0;
    const int t1 = (hw && h->d.ghost_top) ? imin(r0 + e, r1) : r0;
    const int b0 = (hw && h->d.ghost_bottom) ? imax(r1 - e, t1) : r1;
    hipStream_t st = split ? h->s1 : h->s0;
    if (split) HIPCHK(hipStreamWaitEvent(h->s1, h->ev_main, 0));   // recorded in step_edges, before the strips
    if (int rc = launch_range(h, st, it, c, t1, b0)) return rc;
    if (split) HIPCHK(hipEventRecord(h->ev_int, h->s1));
    h->phase_of_tick = 2;
    return 0;
}

static int commit_impl(fibhip_t h)
{
    if (h->phase_of_tick != 2) return fail(FIBHIP_EINVAL, "step_commit: call step_interior first");
    if (split_tick(h, h->plan.back())) HIPCHK(hipStreamWaitEvent(h->s0, h->ev_int, 0));
    memcpy(h->cur, h->nxt, sizeof h->cur);
    const int ticks = h->plan.empty() ? 1 : (h->plan[0].K > h->spt ? h->plan[0].K / h->spt : 1);
    h->n_ticks += ticks;
    if (h->use_agg && ends_cycle(h)) h->agg_ghost_dirty = true;   // the exchange of this tick replaced the ghost rows
    h->cpos = (h->cpos + h->span) % h->cycle;
    h->phase_of_tick = 0;
    // the recorder sees every tick on its own: while it is attached nothing fuses ticks (multi_cap, mt_variant), span is 1
    if (h->obs.on)
        if (int rc = observe_enqueue(h)) return rc;
    // ... then the hooks of recorders.hpp, in its order (a plain tick stands behind a confirmed stream: no give-up word to look at)
    return recorders_advance(h, ticks, false);
}

static int tick_now(fibhip_t h)
{
    if (int rc = edges_impl(h)) return rc;
    if (int rc = interior_impl(h)) return rc;
    return commit_impl(h);
}
