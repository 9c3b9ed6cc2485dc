// plan.inc — which kernels make up one tick of a handle: the rule-based plan (build_plan) and the choice by
// measurement on the handle's own geometry (autotune).
// (included by fibhip.hip, behind sched.inc: autotune times real launches)

// (`period_ok`: an exchange-period row may be the answer — only where the caller's environment named it, see build_plan)
static const Variant *find_variant(const fibhip_ctx *h, int K, const int *want /*TX,TY,NT or null*/, int mode = -1, bool period_ok = false)
{
    const int fast = (h->d.flags & FIBHIP_FAST) ? 1 : 0, phase = h->has_phase ? 1 : 0;
    if (mode < 0) mode = h->mode;
    // fenton_simple.py's Laplacian is a property of the kernel's model type (FentonZP): its own rows of the table
    const int vmodel = (h->d.model == FIBHIP_FENTON4V && (h->d.flags & FIBHIP_ZEROPAD)) ? VM_FENTON_ZP
                       : (h->use_agg ? VM_COURT_AGG : h->d.model);
    if (h->has_tensor) {
        // per-cell diffusion tensors are a property of the kernel's model type too (Tensor<M>): their own table, phase rows only
        for (int i = 0; i < g_ntensor_variants; ++i) {
            const Variant &v = g_tensor_variants[i];
            if (v.model != h->d.model || v.mode != mode || v.fast != fast || v.K != K) continue;
            if (want && (v.TX != want[0] || v.TY != want[1] || v.NT != want[2])) continue;
            return &v;
        }
        return nullptr;
    }
    const Variant *tab = h->mod ? h->mod->variants.data() : g_variants;
    const int ntab = h->mod ? (int)h->mod->variants.size() : g_nvariants;
    for (int i = 0; i < ntab; ++i) {
        const Variant &v = tab[i];
        if (v.kind == MK_POINTWISE || (v.period && !period_ok)) continue;
        if (v.model != vmodel || v.mode != mode || v.fast != fast || v.phase != phase || v.K != K) continue;
        if (want && (v.TX != want[0] || v.TY != want[1] || v.NT != want[2])) continue;
        return &v;
    }
    return nullptr;
}

// Decompose one tick of `spt` sub-steps into launches.  Default fusion depth per model comes from
// the measurements recorded in DESIGN.md; FIBHIP_K / FIBHIP_VARIANT override it for sweeps.
static int build_plan(fibhip_ctx *h)
{
    h->plan.clear();
    h->period_v = nullptr;
    h->period_forced = false;
    h->tuned = false;
    h->mt.stale = true;
    int prefK = 0, want[3], nwant = 0;
    bool env_variant = false, env_k = false;
    if (const char *e = getenv("FIBHIP_VARIANT")) {
        int k = 0;
        if (sscanf(e, "%d,%d,%d,%d", &k, &want[0], &want[1], &want[2]) == 4) {
            prefK = k;
            nwant = 1;
            env_variant = true;
        }
    }
    if (!prefK)
        if (const char *e = getenv("FIBHIP_K")) {
            prefK = atoi(e);
            env_k = prefK > 0;
        }
    const int envK = (env_variant || env_k) ? prefK : 0;
    if (!prefK) {
        // Measured on MI355X (DESIGN.md §6, tools/sweep.py).  Beeler-Reuter / Courtemanche spend their time
        // in the transcendental pipe (64 / ~70 per cell-step): redundant rim cells cost more than the
        // launches they save, so one sub-step per launch.  Fenton is cheap per cell: fuse — as deep as the
        // tick when the grid gives each CU about one tile (launch/latency-bound), 5 sub-steps with a
        // smaller rim when there are many tiles per CU (throughput-bound), fatter waves when there are
        // very many (occupancy).
        prefK = 1;
        // rows of the largest launch: the first tick of an exchange cycle also advances the ghost rows
        const int ext = (h->cycle - 1) * h->spt;
        const int rows = (h->own1 - h->own0) + (h->d.ghost_top ? ext : 0) + (h->d.ghost_bottom ? ext : 0);
        if (h->mod) {
            // the same rule as the FIB_CUSTOM_* block below, with the generated header's numbers at run time
            const fibhip_module &m = *h->mod;
            const long tiles = tiles_of(h, m.TX, m.TY, rows);
            prefK = tiles <= (m.K2 > 1 ? 256 : 512) ? m.K : m.K2;
            if (m.TYB > 0 && prefK == m.K && prefK > 1) {
                const long tiles_b = tiles_of(h, m.TX, m.TYB, rows);
                want[0] = m.TX; want[1] = tiles_b <= 256 ? m.TYB : m.TY; want[2] = -m.R;
                nwant = 1;
            }
        }
#ifdef FIB_CUSTOM_MODEL_INC
        if (h->d.model == FIBHIP_CUSTOM) {
            // one tile per CU or two: latency-bound, fuse the whole tick; more: throughput-bound (see the generator)
            const long tiles = tiles_of(h, FIB_CUSTOM_TX, FIB_CUSTOM_TY, rows);
            // a cheap graph has a shallower fusion to fall back to (K2 > 1): deep fusion only while every CU has at
            // most one tile (the measured Fenton rule); a heavy graph (K2 == 1) keeps it up to two tiles per CU
            // (the measured Beeler-Reuter rule)
            prefK = tiles <= (FIB_CUSTOM_K2 > 1 ? 256 : 512) ? FIB_CUSTOM_K : FIB_CUSTOM_K2;
#if FIB_CUSTOM_TYB > 0
            // the 15-wave tile when it still gives every CU at most one tile (measured on Fenton: 18.5 vs 19.6 us)
            const long tiles_b = tiles_of(h, FIB_CUSTOM_TX, FIB_CUSTOM_TYB, rows);
            if (prefK == FIB_CUSTOM_K && prefK > 1) {
                want[0] = FIB_CUSTOM_TX; want[1] = tiles_b <= 256 ? FIB_CUSTOM_TYB : FIB_CUSTOM_TY; want[2] = -FIB_CUSTOM_R;
                nwant = 1;
            }
#endif
        }
#endif
        if (h->d.model == FIBHIP_BR) {
            // up to two tiles per CU: the tick is launch/latency-bound, so all 5 sub-steps in one launch;
            // large grids are bound by the transcendental pipe, where the redundant rim costs more than launches
            const long tiles = tiles_of(h, 54, 21, rows);
            if (tiles <= 512 && h->spt == 5) {
                prefK = 5; want[0] = 54; want[1] = 21; want[2] = -2;      // measured: profiles/r01_sweep_br512.txt
                nwant = 1;
            }
        }
        if (h->d.model == FIBHIP_FENTON4V) {
            const long tiles10 = tiles_of(h, 44, 25, rows), t28 = tiles_of(h, 44, 28, rows);
            const long t21 = tiles_of(h, 54, 21, rows), t23 = tiles_of(h, 54, 23, rows);
            const long r21 = (t21 + 255) / 256, r23 = (t23 + 255) / 256;       // tiles per CU, rounded up
            const bool sharded = h->d.ghost_top || h->d.ghost_bottom;
            // Measured (tools/sweep_sizes.py, profiles/r01_sweep_sizes.txt): what matters is how many tiles a CU gets.
            // K=10: 18 us with <= 1 tile per CU, ~34 us with 2.  K=5 (two launches), R=3: 27 us with <= 2 per CU, 38 us
            // with 3; the 23-row tile fills its 11 waves exactly (33 rows) and is taken when it saves a whole round
            // of tiles.  Beyond that the fatter R=4 waves win, with the wave-exact 22-row tile.
            if ((h->d.flags & FIBHIP_ZEROPAD) || h->has_tensor) {
                // fenton_simple.py's Laplacian exists in the flat tick_kernel only (measured at 512^2: 10 x 32x32 x 1024
                // threads 20.8 us per 10 steps, 5 x 32x32 x 512 25.4); so does the tensor Laplacian, whose table has the same
                // flat rows (Beeler-Reuter's rule above names a strip: a tensor handle gets the flat row of that K instead)
                const long t32 = tiles_of(h, 32, 32, rows);
                prefK = t32 <= 512 ? 10 : 5; want[0] = 32; want[1] = 32; want[2] = t32 <= 512 ? 1024 : 512;
            } else if (tiles10 <= 256 || t28 <= 256) {
                prefK = 10; want[0] = 44; want[1] = tiles10 <= 256 ? 25 : 28; want[2] = -3;
            } else if (sharded && tiles10 <= 512) {
                // row blocks: the launch is sized for the first tick of an exchange cycle, later ticks have fewer
                // ghost rows to advance (measured 21.6 us per tick for 512 + 2 x 40 rows)
                prefK = 10; want[0] = 44; want[1] = 25; want[2] = -3;
            } else if (r21 <= 2 || r23 <= 2) {
                prefK = 5; want[0] = 54; want[1] = r21 <= 2 ? 21 : 23; want[2] = -3;
            } else if (tiles10 <= 512 || t28 <= 512) {
                prefK = 10; want[0] = 44; want[1] = tiles10 <= 512 ? 25 : 28; want[2] = -3;
            } else if (r21 <= 3 || r23 <= 3) {
                prefK = 5; want[0] = 54; want[1] = r21 <= 3 ? 21 : 23; want[2] = -3;
            } else {
                prefK = 5; want[0] = 54; want[1] = 22; want[2] = -4;      // measured best at 1024^2 .. 4096^2
            }
            nwant = 1;
        }
    }
    const int maxghost = is_shard(h) ? min_ghost(h->d) : 1 << 30;
    int rem = h->spt;
    while (rem > 0) {
        const Variant *best = nullptr;
        for (int K = (prefK < rem ? prefK : rem); K >= 1 && !best; --K) {
            if (K > maxghost) continue;
            // (an exchange-period row is taken only where FIBHIP_VARIANT names that very row or FIBHIP_K its K: never by a rule, by
            // the descent to a shallower K — a tick of 7, 8 or 9 sub-steps, FIBHIP_K=7 — or as the stand-in for a shape that
            // names no row)
            best = find_variant(h, K, nwant ? want : nullptr, -1, K == envK);
            if (!best && nwant) best = find_variant(h, K, nullptr);
        }
        if (!best) return fail(FIBHIP_EINVAL, "no kernel variant for model %d mode %d", h->d.model, h->mode);
        h->plan.push_back({best->K, best->fn, best->TY, best->TX, best});
        rem -= best->K;
    }
    // a forced exchange-period row (FIBHIP_VARIANT, FIBHIP_K): its K sub-steps and the shallower launches that complete the tick
    // are the plain tick; the multi-tick launches run the row itself, in periods of K (sched.inc mt_variant)
    if (h->plan[0].v && h->plan[0].v->period) {           // (only ever the row the environment named: find_variant's period_ok)
        h->period_v = h->plan[0].v;
        h->period_forced = true;
    }
    // FIBHIP_PERIOD_ROW="K,TX,TY,NT": that exchange-period row rides beside the plan as if autotune() had chosen it — the launches
    // of long declared series only (sched.inc mt_variant) — on any grid (tuning sweeps, and the tests of that path on small grids)
    if (!h->period_v)
        if (const char *e = getenv("FIBHIP_PERIOD_ROW")) {
            int k = 0, w[3];
            if (sscanf(e, "%d,%d,%d,%d", &k, &w[0], &w[1], &w[2]) == 4) {
                const Variant *v = find_variant(h, k, w, -1, true);
                if (v && v->period) h->period_v = v;
            }
        }
    // Courtemanche: the reference's driver fires 'slow' right after every 10th tick (court.py:612-617).  When the
    // last tick of a fibhip_step call is still pending at that moment, both run as ONE launch (MODE_FASTSLOW): the
    // 21 arrays are read once instead of twice.  Requirements: a single K=1 launch per tick, no ghost rows, and
    // every border cell's inward neighbour inside the border cell's own tile.
    h->fused_fn = nullptr;
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
    if (h->d.model == FIBHIP_COURT && h->mode == Courtemanche::MODE_FAST && h->plan.size() == 1 && h->plan[0].K == 1 &&
        !h->d.ghost_top && !h->d.ghost_bottom && !getenv("FIBHIP_NO_LAZY")) {
        const int want1[3] = {h->plan[0].TX, h->plan[0].TY, 256};
        const Variant *v = find_variant(h, 1, want1, Courtemanche::MODE_FASTSLOW);
        if (v && (h->d.height - 1) % v->TY != 0 && (h->d.width - 1) % v->TX != 0) h->fused_fn = v->fn;
    }
    // Courtemanche on aggregates: one tick is one sub-step and moves 16 arrays for ~300 instructions per cell, so
    // two or three consecutive ticks are blocked in time like the sub-steps of a Fenton tick (fibhip_step defers
    // ticks until a launch is full; every entry point that observes the state launches what is pending first)
    h->multi_max = 1;
    for (int T = 2; T <= 3; ++T) h->plan_multi[T].clear();
    // (row blocks: the ticks between two halo exchanges are fused the same way — the ghost zone must be deep enough for the
    // fused ticks to stay inside the exchange cycle; the tick that ends the cycle stays a launch of its own)
    const bool shard = h->d.ghost_top || h->d.ghost_bottom;
    if (h->use_agg && h->mode == CourtAgg::MODE_FAST && h->plan.size() == 1 && h->plan[0].K == 1 && (!shard || h->cycle >= 3) &&
        !getenv("FIBHIP_NO_MULTI")) {
        for (int T = 2; T <= (shard ? imin(3, h->cycle - 1) : 3); ++T) {
            int w[3];
            const char *e = getenv(T == 2 ? "FIBHIP_COURT_MULTI2" : "FIBHIP_COURT_MULTI3");
            const bool have = e && sscanf(e, "%d,%d,%d", &w[0], &w[1], &w[2]) == 3;
            const Variant *v = find_variant(h, T, have ? w : nullptr, CourtAgg::MODE_FAST);
            if (!v) break;
            h->plan_multi[T].push_back({v->K, v->fn, v->TY, v->TX, v});
            h->multi_max = T;
        }
    }
#endif
    return 0;
}

// Plan selection by measurement (Fenton 4v and Beeler-Reuter).  The K-fused kernels exist in a family of tile shapes
// (Fenton: K = 10 or 5, tile heights 21..56; Beeler-Reuter: K = 5, heights 21..40, or one sub-step per launch): which
// one is fastest depends on how the grid's tiles land on the 256 CUs — a launch costs about the
// same whether a CU gets one tile or none, and nearly twice as much with two — so fixed size thresholds leave cliffs
// (576^2: 26.7 us per tick with the 512^2 choice, 18.9 with a taller tile).  The first tick of a handle therefore
// times every candidate ONCE on the handle's own geometry (its real launch: same buffers, same rows; a candidate
// writes what the real launch overwrites) and keeps the fastest.  All candidates are bit-identical in their results
// (tests/test_gpu_variant_table.py runs EVERY row of the table, enumerated through fibhip_variant_info, against the
// one-sub-step-per-launch kernel), so the choice changes speed only — ranks of
// a sharded grid may choose differently.  FIBHIP_AUTOTUNE=0, FIBHIP_VARIANT or FIBHIP_K switch it off.
// Courtemanche on aggregates: which tile shape for the launches of two and of three ticks, on this very geometry
static int autotune_multi(fibhip_ctx *h)
{
#if !defined(FIB_CUSTOM_ONLY) && !defined(FIB_ONLY_BR)
    if (const char *e = getenv("FIBHIP_AUTOTUNE"))
        if (atoi(e) == 0) return 0;
    if (int rc = refresh_agg(h)) return rc;                       // time the kernels on real values
    const int phase = h->has_phase ? 1 : 0;
    const long launches0 = h->launches;
    for (int T = 2; T <= h->multi_max; ++T) {
        if (getenv(T == 2 ? "FIBHIP_COURT_MULTI2" : "FIBHIP_COURT_MULTI3")) continue;
        std::vector<PlanItem> cand;
        for (int i = 0; i < g_nvariants; ++i) {
            const Variant &v = g_variants[i];
            if (v.model != VM_COURT_AGG || v.mode != CourtAgg::MODE_FAST || v.fast != 1 || v.phase != phase || v.K != T) continue;
            cand.push_back({v.K, v.fn, v.TY, v.TX, &v});
        }
        std::vector<float> best_of(cand.size(), 1e30f);
        for (int round = 0; round < 4; ++round)                   // rounds over all candidates: see autotune()
            for (size_t t = 0; t < cand.size(); ++t) {
                HIPCHK(hipEventRecord(h->ev_t0, h->s0));
                LaunchCtx c;
                int nxt[FIB_MAXVAR];
                fill_ptrs(h, c, T, h->cur, nxt);                  // current slab -> other slab: the state stays put
                c.sub0 = 0;
                if (int rc = launch_range(h, h->s0, cand[t], c, 0, h->d.height)) return rc;
                HIPCHK(hipEventRecord(h->ev_t1, h->s0));
                HIPCHK(wait_event(h->ev_t1));
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
                if (round > 0 && ms < best_of[t]) best_of[t] = ms;
            }
        float best_ms = 1e30f;
        for (size_t t = 0; t < cand.size(); ++t)
            if (best_of[t] < best_ms) {
                best_ms = best_of[t];
                h->plan_multi[T].assign(1, cand[t]);
            }
        if (getenv("FIBHIP_PRINT_PLAN") && !h->plan_multi[T].empty())
            fprintf(stderr, "fibhip: %dx%d Courtemanche on aggregates: %d ticks per launch in tiles of %dx%d (%.2f us when chosen)\n",
                    h->d.height, h->d.width, T, h->plan_multi[T][0].TX, h->plan_multi[T][0].TY, best_ms * 1e3f);
    }
    h->launches = launches0;
#endif
    return 0;
}

static int autotune(fibhip_ctx *h)
{
    h->tuned = true;
    if (h->use_agg && h->multi_max > 1) return autotune_multi(h);
    if ((h->d.model != FIBHIP_FENTON4V && h->d.model != FIBHIP_BR && h->d.model != FIBHIP_CUSTOM) ||
        (h->d.flags & FIBHIP_ZEROPAD) || h->has_tensor || h->spt < 2)     // (a tensor handle: its rule is its plan; no strips to time)
        return 0;
    if (getenv("FIBHIP_VARIANT") || getenv("FIBHIP_K")) return 0;
    if (const char *e = getenv("FIBHIP_AUTOTUNE"))
        if (atoi(e) == 0) return 0;
    const int maxghost = is_shard(h) ? min_ghost(h->d) : 1 << 30;
    const int fast = (h->d.flags & FIBHIP_FAST) ? 1 : 0, phase = h->has_phase ? 1 : 0;
    const std::vector<PlanItem> heuristic = h->plan;
    const long launches0 = h->launches;
    // (a traced model on a run-time module brings its own, short, table: the shapes its generated header asked for)
    const Variant *tab = h->mod ? h->mod->variants.data() : g_variants;
    const int ntab = h->mod ? (int)h->mod->variants.size() : g_nvariants;
    std::vector<std::vector<PlanItem>> trials;
    std::vector<const Variant *> period_of;                       // per trial: the exchange-period row it times, or null
    trials.push_back(heuristic);                                  // the rule-based plan is a candidate like any other
    period_of.push_back(nullptr);
    for (int i = 0; i < ntab; ++i) {
        const Variant &v = tab[i];
        if (v.kind == MK_POINTWISE) continue;
        if (v.model != h->d.model || v.mode != h->mode || v.fast != fast || v.phase != phase) continue;
        // strip kernels of every fusion depth, and the one-sub-step-per-launch tiles
        const bool strip = v.NT < 0 && v.NT > -32 && v.K >= 2, single = v.NT > 0 && v.K == 1;
        if (v.period) {
            if (getenv("FIBHIP_PERIOD_ROW")) continue;            // (the row beside the plan is the caller's choice)
            // an exchange-period row is a candidate as what it is for: the multi-tick launch, timed like the other rows' (the
            // trial's plan stays the rule-based one: what a plain tick would run beside it)
            // (... on grids that fill more than half of the device: what a period buys is the balance of a FULL device's SIMDs and
            // its rim traffic, measured at 512x512; eight ticks of a handful of tiles time the launch's ends and little else)
            if (!mt_eligible(h, &v) || 2 * tiles_of(h, v.TX, v.TY) <= h->ncu) continue;
            trials.push_back(heuristic);
            period_of.push_back(&v);
            continue;
        }
        if (!(strip || single) || h->spt % v.K != 0 || v.K > maxghost) continue;
        if (!heuristic.empty() && heuristic[0].fn == v.fn) continue;
        std::vector<PlanItem> trial;
        for (int n = 0; n < h->spt / v.K; ++n) trial.push_back({v.K, v.fn, v.TY, v.TX, &v});
        trials.push_back(trial);
        period_of.push_back(nullptr);
    }
    // One tick of a candidate, back to back between one pair of events (the gaps between its launches are part of its
    // cost).  The candidates are timed in ROUNDS — every candidate once per round, the first round a warm-up (code
    // objects, caches), the minimum over the other rounds kept: the clocks of a GPU that has just been idle rise for
    // many milliseconds, and timing the candidates one after the other would favour whichever come last.
    std::vector<float> best_of(trials.size(), 1e30f);
    std::vector<bool> failed(trials.size(), false);
    for (int round = 0; round < 4; ++round) {
        for (size_t t = 0; t < trials.size(); ++t) {
            if (failed[t] || trials[t].empty()) continue;
            const std::vector<PlanItem> &trial = trials[t];
            h->plan = trial;
            // a shape that will run several ticks per launch is timed as that: AT_MT_TICKS ticks in one launch, per tick
            const Variant *mtv = period_of[t] ? period_of[t] : (trial.size() == 1 ? trial[0].v : nullptr);
            const bool as_mt = mt_eligible(h, mtv);
            HIPCHK(hipEventRecord(h->ev_t0, h->s0));
            int sub = 0;
            if (as_mt) {
                if (mt_launch(h, mtv, AT_MT_TICKS, false, nullptr)) failed[t] = true;
            } else
            for (size_t l = 0; l < trial.size(); ++l) {           // every launch with the rows edges_impl gives it
                LaunchCtx c;
                int nxt[FIB_MAXVAR];
                fill_ptrs(h, c, trial[l].K, h->cur, nxt);         // ALWAYS current slab -> other slab: the state stays put
                for (int v = 0; v < h->nvar; ++v)                 // (a K = 1 launch would update the pointwise arrays in place)
                    c.out[v] = h->slab[h->cur[v] ^ 1] + (size_t)v * h->vstride;
                c.sub0 = sub;
                int r0, r1;
                rows_of_launch(h, l, r0, r1);
                if (launch_range(h, h->s0, trial[l], c, r0, r1)) { failed[t] = true; break; }
                sub += trial[l].K;
            }
            if (failed[t]) {
                // a shape that cannot be launched here is dropped — audibly, and a failure of the rule-based plan itself is
                // the caller's error to see
                (void)hipGetLastError();
                if (getenv("FIBHIP_PRINT_PLAN"))
                    fprintf(stderr, "fibhip: %dx%d model %d: candidate K=%d tile %dx%d could not be launched: %s\n", h->d.height,
                            h->d.width, h->d.model, mtv ? mtv->K : trial[0].K, mtv ? mtv->TX : trial[0].TX, mtv ? mtv->TY : trial[0].TY, g_err);
                if (t == 0) {
                    h->plan = heuristic;
                    return FIBHIP_EHIP;
                }
                HIPCHK(wait_stream(h->s0));
                continue;
            }
            HIPCHK(hipEventRecord(h->ev_t1, h->s0));
            HIPCHK(wait_event(h->ev_t1));
            if (as_mt) {
                // a candidate whose tiles could not all become resident (a CU mask, another process on the device) gave up
                // waiting: it is dropped like one that could not be launched — the state is untouched, a trial writes the
                // other slab only — and the words are cleared for the next candidate
                const unsigned gave_up = __atomic_load_n(h->mt.host_give_up(), __ATOMIC_ACQUIRE);
                if (gave_up) {
                    failed[t] = true;
                    h->mt.stale = true;
                    __atomic_store_n(h->mt.host_give_up(), 0u, __ATOMIC_RELEASE);
                    if (getenv("FIBHIP_PRINT_PLAN"))
                        fprintf(stderr, "fibhip: %dx%d model %d: candidate K=%d tile %dx%d gave up waiting as a multi-tick launch: dropped\n",
                                h->d.height, h->d.width, h->d.model, mtv->K, mtv->TX, mtv->TY);
                    continue;
                }
            }
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
            if (as_mt) ms /= (float)AT_MT_TICKS;
            if (round > 0 && ms < best_of[t]) best_of[t] = ms;
        }
    }
    // the fastest plan of whole ticks — and, if it is faster still, the exchange-period row for the multi-tick launches beside it
    std::vector<PlanItem> best_plan = heuristic;
    float best_ms = 1e30f, best_period_ms = 1e30f;
    const Variant *best_period = nullptr;
    for (size_t t = 0; t < trials.size(); ++t) {
        if (failed[t] || trials[t].empty()) continue;
        if (period_of[t]) {
            if (best_of[t] < best_period_ms) {
                best_period_ms = best_of[t];
                best_period = period_of[t];
            }
        } else if (best_of[t] < best_ms) {
            best_ms = best_of[t];
            best_plan = trials[t];
        }
    }
    h->plan = best_plan;
    if (!getenv("FIBHIP_PERIOD_ROW")) h->period_v = best_period_ms < best_ms ? best_period : nullptr;
    h->period_forced = false;                             // (chosen here, or named by FIBHIP_PERIOD_ROW: long declared series only)
    if (getenv("FIBHIP_PRINT_PLAN") && h->period_v)
        fprintf(stderr, "fibhip: %dx%d model %d: several ticks per launch in exchange periods of K=%d sub-steps, tile %dx%d, %d rows per "
                        "wave, for declared series of %d ticks or more (%.2f us per tick when chosen; everything else runs the plan below)\n",
                h->d.height, h->d.width, h->d.model, h->period_v->K, h->period_v->TX, h->period_v->TY, -h->period_v->NT, MT_DECLARED_MIN_TICKS, best_period_ms * 1e3f);
    h->mt.stale = true;
    h->launches = launches0;
    if (getenv("FIBHIP_PRINT_PLAN") && !best_plan.empty())
        fprintf(stderr, "fibhip: %dx%d model %d: %zu launch(es) per tick of K=%d, tile %dx%d, %s (%.2f us per tick when chosen)\n",
                h->d.height, h->d.width, h->d.model, best_plan.size(), best_plan[0].K, best_plan[0].TX, best_plan[0].TY,
                best_plan[0].v ? (best_plan[0].v->NT < 0 ? (best_plan.size() == 1 && mt_eligible(h, best_plan[0].v)
                                                                ? "strips, several ticks per launch" : "strips") : "flat tiles") : "rule-based",
                best_ms * 1e3f);
    return 0;
}
