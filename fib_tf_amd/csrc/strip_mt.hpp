// strip_mt.hpp — the contract between the host and a launch of several ticks (strip_mt_kernel, strip_kernel.inc): the protocol,
// its arguments and its constants.  (included by kernels.hpp)

// ---- several ticks in ONE launch: what a tile needs from its neighbours between two ticks ---------------------------
// A launch of `nticks` ticks keeps every workgroup resident on its tile: the tile's own cells stay in registers from
// tick to tick, and only the K-deep rim of the compute box (which went stale during the tick) is re-read — from what
// the up to eight neighbouring tiles published at the end of their tick.  No grid-wide barrier: a tile waits for its
// neighbours only.
//   * Payload: an exchange buffer of 16-byte cells [2 parities][NVAR/4][H*W] (the state arrays themselves are read at
//     the first tick and written at the last one only).  Stores and loads are write-through / L1-bypassing (sc1): the
//     vector L1 of a CU is never refreshed by another CU's stores and the XCDs' L2s are not coherent with each other
//     (MI355X_MICROARCH.md, "inter-workgroup visibility"); every wave drains its stores (s_waitcnt vmcnt(0)) before the
//     workgroup's barrier, after which ONE lane raises the tile's epoch word.
//   * Epoch words: one per tile, 256 bytes apart (words sharing a line serialise the pollers of a whole tile row on one
//     memory channel: measured 5.5 us per tick boundary against 3.1, tools/ubench/handoff.hip); they count ticks over
//     the life of the handle (epoch0 = their common value when the launch starts), so nothing is reset between launches.
//   * Two parities: a tile overwrites parity p two ticks after it published there, and by then every neighbour has
//     published the tick in between, for which it had to read p first.
//   * Every wait is BOUNDED (s_memrealtime, MT_WAIT_TICKS of 10 ns): a tile that gives up raises err[0], which every
//     waiting tile also polls, so the launch drains instead of hanging; the host reports the failure at its next
//     synchronisation point.  The host only uses this kernel when all tiles can be resident at once (tiles <= CUs)
//     and never runs two such launches of one process at the same time.
//   * Exchange periods (strip_kernel.inc PERIODS; launch.hpp S4P rows).  How often tiles exchange is a parameter of the row, not
//     the tick: a model whose sub-steps are all alike (Fenton: UNIFORM_SUBSTEPS) may run this protocol every K sub-steps with K
//     below the tick's.  "Tick" in everything above then reads "period": the low half of `ticks_id` counts periods, the epoch
//     words count periods, the parities alternate per period, the host's word names a period count — the host translates: the
//     state after n ticks exists inside such a launch only where n ticks end on a period boundary (n * spt a multiple of K); any
//     other request cancels the launch and its ticks are recomputed from the slab it started from (sched.inc ahead_settle).  A
//     launch of T ticks runs ceil(T * spt / K) periods, all of K sub-steps but the last, whose sub-steps travel in the kernel's
//     `sub0` argument.  A period is never shortened on the fly: tiles that saw the host's word at different times would disagree.
struct MtArgs {
    float *xb;            // exchange buffer
    unsigned *epoch;      // one word per tile, MT_EPOCH_STRIDE words apart
    unsigned *err;        // [0]: a tile gave up waiting; [MT_EPOCH_STRIDE]: the host's word as tile 0 passed it on; [2 * MT_EPOCH_STRIDE]:
                          // tiles that stopped where it said (counted)
    unsigned epoch0;      // value of every epoch word when the launch starts
    unsigned ticks_id;    // low half: ticks this launch advances (an exchange-period row: periods); high half: the launch's id, 1 .. 65535 (the host's word names
                          // the launch it is meant for).  One word, and the host's word behind the tiles' words of `snap_flag`
                          // instead of a pointer of its own: Beeler-Reuter's kernel spills scalar registers as it is, and three
                          // more kernel arguments cost it 2.5 % (same-box A/B)
    // read-back inside the launch (fibhip.hip `run-ahead`): every tile also writes array `snap_var` of the state the launch
    // STARTS from into page-locked host memory during its first ticks and then raises its word in `snap_flag` (host memory
    // too, 64 bytes apart) to `snap_seq` — the host has the frame while the launch is still computing
    float *snap;
    unsigned *snap_flag;  // page-locked HOST memory (device address): MT_MAX_TILES words MT_SNAP_STRIDE apart, then the host's
                          // word {launch id << 16 | n}, written by the host while a launch runs — n = MT_CANCEL: not wanted any
                          // more, else: stop after n ticks (always allocated, with or without a frame to deliver)
    unsigned snap_seq;
    int snap_var;         // low byte: which array the frame is; the other three: the bound on a tile's wait for its neighbours in
                          // milliseconds (0 = MT_WAIT_TICKS; packed, not an argument of its own: see ticks_id)
};
constexpr int MT_SNAP_STRIDE = 16;                    // words between two tiles' words in snap_flag
constexpr int MT_MAX_TILES = 1024;                    // epoch / snap words allocated per handle (only grids of <= ncu tiles use them)
constexpr int MT_HOST_WORD_AT = MT_MAX_TILES * MT_SNAP_STRIDE;   // the host's word, in words from snap_flag
constexpr int MT_GIVEUP_WORD = 8;                     // ... and, this many words behind it, the id of the launch whose tile gave up first
constexpr int MT_EPOCH_STRIDE = 64;                   // words (256 bytes)
constexpr unsigned MT_CANCEL = 0xFFFFu;               // the host's word, low half: this launch is not wanted any more
constexpr unsigned long long MT_WAIT_TICKS = 200000000ull;   // 2 s of the 100 MHz s_memrealtime clock
constexpr int MT_POLL_SLEEP = 1;                             // s_sleep between two polls of the neighbours' words
