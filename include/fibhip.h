/*
 * fibhip.h — C ABI of libfibhip.so: the MI355X (gfx950) explicit time-stepper for 2D cardiac
 * reaction-diffusion.
 *
 * What this boundary replaces.  The reference (siravan/fib_tf) has no FFI for its hot path:
 * the lower face of its stepper is `tf.Session.run(op)` on ops built by `define()`
 * (ionic.py:188-204).  Every entry point below names the reference call it stands in for.
 * The upper face (IonicModel / define() / run() / add_pace_op() / fire_op() / image()) is
 * kept in Python (fib_tf_amd/ionic.py ...) and binds these symbols through ctypes
 * (fib_tf_amd/_lib.py; INTEGRATION.md shows the stub a maintainer of the reference would add).
 *
 * Conventions: plain C, opaque handle, every function returns 0 on success or a negative
 * FIBHIP_E* code; fibhip_last_error() returns a thread-local message for the last failure.
 * Host buffers are caller-owned float32, row-major; "slab" = SoA [nvar][height][width].
 * Work is enqueued asynchronously on the handle's HIP stream; only get/probe/sync/time block.
 * A handle is not re-entrant.  There is NO CPU fallback: without a HIP device create() fails.
 *
 * Variable order (index `var`), as the reference declares its state:
 *   FENTON4V : U V W S                                   (fenton.py:128-131)
 *   BR       : V C M H J D F XI                          (br.py:87-94)
 *   COURT    : V Na_i m h j K_i oa oi ua ui xr xs Ca_i d f f_Ca Ca_rel u v w Ca_up
 *                                                        (court.py:57-78)
 * Variable 0 is always the transmembrane potential (the only array the stencil touches).
 */
#ifndef FIBHIP_H
#define FIBHIP_H

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: these entry points are ALL it exports (no kernel handle, host stub or
 * template instance of one build can meet its namesake of another build of the same sources in one process). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define FIBHIP_ABI_VERSION 1

typedef struct fibhip_ctx *fibhip_t;

enum fibhip_model {
    FIBHIP_FENTON4V = 0, FIBHIP_BR = 1, FIBHIP_COURT = 2,
    FIBHIP_COURT_US = 3,  /* court_ultra.py with config['ultra_slow']: a 22nd array `_us_` (court_ultra.py:81-82,  */
                          /* 198-199,221-222,445-450); always single-rate (implies FIBHIP_ALLVARS)                */
    FIBHIP_CUSTOM = 4     /* a user-written IonicModel subclass in the reference's style, traced by               */
                          /* fib_tf_amd/traced.py and compiled into its own copy of this library                  */
                          /* (-DFIB_CUSTOM_MODEL_INC=...); the stock library rejects it                           */
};

enum fibhip_flags {
    FIBHIP_CHEBY   = 1u << 0, /* BR: Chebyshev gates, config['cheby'] (br.py:132-135); needs set_consts   */
    FIBHIP_SKIP    = 1u << 1, /* BR: multirate slow gates, config['skip'] (br.py:98-103)                  */
    FIBHIP_CHRONIC = 1u << 2, /* COURT: self.chronic (court.py:41,167-170)                                */
    FIBHIP_FAST    = 1u << 3, /* hardware-rate division/exp/tanh instead of the rounding-faithful forms;  */
                              /* looser parity tolerance, see DESIGN.md                                    */
    FIBHIP_ALLVARS = 1u << 4, /* COURT: every tick updates all 21 variables with dt (court_ultra.py:      */
                              /* 107-111,127-128) instead of the fast/slow split                           */
    FIBHIP_ZEROPAD = 1u << 6, /* Laplacian of fenton_simple.py / fenton_jit.py: a 3x3 convolution with zero padding        */
                              /* (fenton_simple.py:38-49) instead of IonicModel.laplace; single device only              */
    FIBHIP_HOLD    = 1u << 7, /* BR: the slow gates xi, j, d, f are not advanced at all: BeelerReuter.solve(state, 0),  */
                              /* the sub-steps 1..4 of a `skip` tick taken on their own (br.py:98-103,195-205)         */
    FIBHIP_ROW_INTERLEAVED = 1u << 5 /* device slab layout [height][nvar][width] instead of               */
                              /* [nvar][height][width]: the rows a row block exchanges with a neighbour    */
                              /* (all arrays) are then ONE contiguous block.  Host-side get/set_state keep  */
                              /* the planar [nvar][height][width] view.                                     */
};

enum fibhip_err {
    FIBHIP_OK = 0,
    FIBHIP_EINVAL = -1,   /* bad argument / call order                                   */
    FIBHIP_EHIP = -2,     /* a HIP runtime call failed (message has the HIP error text)  */
    FIBHIP_ENODEV = -3,   /* no usable HIP device                                        */
    FIBHIP_ENOMEM = -4
};

typedef struct fibhip_desc {
    int struct_size;     /* sizeof(fibhip_desc): ABI check                                                */
    int model;           /* enum fibhip_model                                                             */
    int height, width;   /* rows/cols of THIS handle's slab (for a row block: owned + ghost rows)         */
    double dt;           /* config['dt']   (fenton.py:159)                                                */
    double diff;         /* config['diff'] (fenton.py:161); diff*dt is formed in double, rounded once     */
    unsigned flags;      /* enum fibhip_flags                                                             */
    int device;          /* HIP device ordinal                                                            */
    int steps_per_tick;  /* sub-steps one tick advances; 0 = the reference's unroll factor               */
                         /* (Fenton 10 fenton.py:135-138, BR 5 br.py:98-107, Courtemanche 1 court.py:92)  */
    /* row-block domain decomposition (all 0 for a single device):                                       */
    int global_height;   /* rows of the whole grid; 0 = height                                            */
    int row_offset;      /* global row index of local row 0                                               */
    int ghost_top;       /* rows at the top of the slab that mirror the upper neighbour's rows            */
    int ghost_bottom;    /* same at the bottom; a ghost width must be >= steps_per_tick.  A width of      */
                         /* m * steps_per_tick makes the halo exchange due only every m-th tick           */
                         /* (fibhip_halo_due): the ticks in between also advance the ghost rows they      */
                         /* still need (communication-avoiding, redundant compute instead of messages)    */
    void *stream;        /* hipStream_t to enqueue on (e.g. the caller's torch stream); NULL = own stream */
    void *ext_slab[2];   /* optional caller-owned DEVICE slabs, each nvar*height*width floats             */
                         /* (so that the caller can hand them to RCCL); NULL = library allocates          */
    void *module;        /* model == FIBHIP_CUSTOM on the stock library: a fibhip_module_t (fibhip_module_load)  */
                         /* holding the traced model's kernels; NULL otherwise                            */
} fibhip_desc;

/* model facts, usable before create: number of state arrays / default steps per tick */
int fibhip_nvar(int model);
int fibhip_default_steps_per_tick(int model);
int fibhip_abi_version(void);
int fibhip_device_count(void);

/* == define(): tf.Variable creation + graph build (fenton.py:126-147, br.py:85-122, court.py:85-112) */
int fibhip_create(const fibhip_desc *desc, fibhip_t *out);
int fibhip_destroy(fibhip_t h);

/* == self.ϕ = tf.Variable(self.phase) (ionic.py:55-57).  phi: host [height*width] (local rows). Must
 * precede the first step.  NULL removes the phase field.                                               */
int fibhip_set_phase(fibhip_t h, const float *phi);

/* Per-cell diffusion tensors: anisotropic, heterogeneous conduction.  dyy, dxx, dxy: host [height*width] each, the tensor
 * D = [[dyy, dxy], [dxy, dxx]] of every cell (rows are y, columns are x), dimensionless and relative to `diff`; the handle's
 * diffusion term becomes diff * div(D grad V) in the second-order 9-point form of DESIGN.md 25, which is the isotropic
 * stencil, value for value, at D = I.  All three NULL removes the tensor.  The rules are fibhip_set_phase's: launches what is
 * pending, waits for an unconfirmed launch, is refused inside an open tick, and chooses the plan again — a tensor handle runs
 * the flat-tile kernels fibhip_tensor_variant_info lists, one launch per K sub-steps, never several ticks per launch, and
 * Courtemanche under FIBHIP_FAST runs its plain modes, not the aggregates.  fibhip_set_phase on a tensor handle prepares the
 * tensor's planes again.  Every recorder and program that only reads the state works beside it.
 * Refused (FIBHIP_EINVAL): row blocks, FIBHIP_ZEROPAD, FIBHIP_CUSTOM and row-interleaved slabs; planes that are not finite,
 * not positive definite, or whose largest eigenvalue is above 1 by more than rounding (raise diff instead); while a lead
 * recorder, a potential-map recorder or a lesion program is attached.  On a tensor handle fibhip_leads_begin,
 * fibhip_pmap_begin, fibhip_lesion_begin and fibhip_lesion_apply are refused: they read the isotropic operator or recompute
 * the phase planes.                                                                                                       */
int fibhip_set_tensor(fibhip_t h, const float *dyy, const float *dxx, const float *dxy);

/* == tf.Variable(init) / define(state=...) (court.py:87-89).  var = -1: whole slab (restarts a row block's
 * exchange cycle: the ghost rows come with it); var >= 0: one array, the cycle position is kept.          */
int fibhip_set_state(fibhip_t h, int var, const float *src);

/* == Variable.eval() (fenton.py:152-153, ionic.py:226-229).  Blocks until preceding ticks are done.     */
int fibhip_get_state(fibhip_t h, int var, float *dst);
/* The same read-back without the staging copy: `dst` should be page-locked memory from fibhip_host_alloc (the Python
 * binding keeps a small pool of such buffers behind the arrays `eval()` / `image()` return: the reference driver reads
 * the potential back 100 times per simulated second, fenton.py:184-185).
 * Run-ahead: when the lengths of the caller's last series of ticks repeat (the same again, or with a period of up to four:
 * that very driver, also inside benchmark regions), this call launches the NEXT series before it returns — the frame
 * then travels inside that launch
 * (the device writes `dst` itself) — and fibhip_step hands those ticks out without launching; any other call on the
 * handle first restores exactly the state the caller has been told about (the launch is stopped at the tick the caller
 * has reached; if a tile is past it already, those ticks are recomputed and the rest cancelled).
 * Invisible except in time; FIBHIP_AHEAD=0 switches it off.  Never on caller-owned slabs (fibhip_desc.ext_slab) and never
 * again once fibhip_state_ptr has handed out a raw pointer: such a caller may write the state between two calls.        */
int fibhip_get_state_direct(fibhip_t h, int var, float *dst);
int fibhip_host_alloc(size_t nbytes, void **out);
int fibhip_host_free(void *p);

/* == constants baked into the graph at define time.  BR + FIBHIP_CHEBY: the 12x9 float32 table `d` of
 * br.py:327 in row order m_inf,h_inf,m_tau,h_tau,xi_inf,j_inf,d_inf,f_inf,xi_tau,j_tau,d_tau,f_tau
 * (br.py:223-240).                                                                                      */
int fibhip_set_consts(fibhip_t h, const float *tbl, int n);

/* == nticks x sess.run(self._ode_op) (ionic.py:202-203).  Asynchronous: an ENQUEUE.  The library may hold ticks back
 * until a launch is worth issuing — the last tick of a call (fibhip_step_slow fuses with it), up to three ticks
 * (Courtemanche, fast policy) or up to 32 (Fenton / Beeler-Reuter on grids whose tiles are all resident at once: one
 * launch loops over them, see fibhip_ticks_per_launch) — and any call on the handle that observes or changes the state
 * launches what is held first: invisible to the caller except that work may be enqueued a few calls later — or
 * EARLIER: a caller whose last series of ticks (between two observations) had n ticks gets the next n launched at the
 * first of them and handed out call by call; if it then stops after fewer, the running launch is told to stop at that
 * tick (or, too late for that, those ticks are recomputed).  fibhip_spec_stats counts both outcomes.                 */
int fibhip_step(fibhip_t h, int nticks);
/* == the loop bounds of IonicModel.run() (ionic.py:199-206: `for i in range(samples)`, a frame every dt_per_plot ticks): the
 * caller DECLARES that it will ask for the next `nticks` ticks as one series — no observation or change of the state in
 * between; one observation may still come first (the frame that starts the series).  A declared series is launched at its
 * first tick, up to fibhip_ticks_per_launch at a time, and handed out call by call; nothing is guessed from the call
 * history (what fibhip_step does for callers that do not say).  A caller that breaks its word is served like one whose
 * predicted series was wrong: the running launch is stopped at the tick reached.  0 withdraws the declaration.
 * TensorFlow has no counterpart: sess.run is synchronous (ionic.py:202-204).                                          */
int fibhip_expect(fibhip_t h, int nticks);

/* == fire_op('slow') of Courtemanche (court.py:103,615-617): re-evaluates solve on the current state and
 * assigns the 17 slow variables.                                                                        */
int fibhip_step_slow(fibhip_t h);
/* == sess.run(op) of any further assign group of a traced model (mode >= 1; FIBHIP_COURT: mode 1 is the 'slow'
 * op): the model is re-evaluated on the current state without the Laplacian and the mode's variables assigned  */
int fibhip_step_mode(fibhip_t h, int mode);

/* == fire_op(name) of an add_pace_op (ionic.py:144-169): pot = max(pot, s) with s = v inside the GLOBAL
 * rectangle rows [r0,r1) x cols [c0,c1) and min_v outside.                                              */
int fibhip_pace(fibhip_t h, int r0, int r1, int c0, int c1, float v, float min_v);

/* == the 'trend' probe (court.py:107-111): one value at LOCAL (row, col).  Blocks.                       */
int fibhip_probe(fibhip_t h, int var, int row, int col, float *out);

int fibhip_sync(fibhip_t h);

/* Runs `nticks` ticks bracketed by HIP events on the handle's stream and returns the elapsed
 * milliseconds and the number of kernel launches in between (for the roofline line of bench.py).        */
int fibhip_time_steps(fibhip_t h, int nticks, float *elapsed_ms, int *launches);
/* The same bracket around whatever the caller enqueues between the two calls (ticks, 'slow' ops, pacing):
 * the real tick mix of a reference driver loop (court.py:612-617) timed on the kernels' own stream.      */
int fibhip_time_begin(fibhip_t h);
int fibhip_time_end(fibhip_t h, float *elapsed_ms, int *launches);

/* ---- row-block decomposition plumbing (multi-GPU; the halo exchange itself is the caller's RCCL) ----
 * One tick = step_edges (the tiles that produce the rows a neighbour needs; main stream) +
 * step_interior (everything else; second stream, concurrent with the caller's halo exchange) +
 * step_commit (join the streams, flip the ping-pong buffers).  fibhip_step == the three in sequence.   */
int fibhip_step_edges(fibhip_t h);
int fibhip_step_interior(fibhip_t h);
int fibhip_step_commit(fibhip_t h);
/* Which of the two slabs currently holds `var` AFTER the last commit (0/1), and its device address.
 * Between step_edges and step_commit, `fibhip_next_ptr` gives the buffer being written.                 */
int fibhip_state_ptr(fibhip_t h, int var, void **dev_ptr);
int fibhip_next_ptr(fibhip_t h, int var, void **dev_ptr);
/* number of state arrays whose ghost rows must be refreshed after each tick (all of them when a tick
 * fuses several sub-steps, only the potential when steps_per_tick == 1)                                 */
int fibhip_halo_vars(fibhip_t h);
/* 1 if the tick that is open (or, between ticks, the next one) ends an exchange cycle: the caller must then
 * refresh ALL ghost rows of the fibhip_halo_vars arrays between step_edges and step_commit; 0 otherwise
 * (step_edges launches everything, step_interior nothing, no exchange)                                    */
int fibhip_halo_due(fibhip_t h);

/* IonicModel's public building blocks as stand-alone array ops on HOST arrays [H*W] (unit-level parity):
 * op 0 = enforce_boundary(a)            ionic.py:107-113
 *    1 = laplace(a) (+ phase term if phi) ionic.py:44-60
 *    2 = phase_field(REFLECT-pad(a)), phi ionic.py:70-81
 *    3 = rush_larsen(a=g, b=g_inf, c=tau, dt)  ionic.py:115-123                                         */
int fibhip_unit_op(int device, int op, int height, int width, const float *a, const float *b, const float *c,
                   const float *phi, double dt, int fast, float *out);

/* laplace(a) of a handle with the diffusion tensor (dyy, dxx, dxy) and the phase field phi (NULL: none) as a stand-alone
 * array op on HOST arrays [H*W]: the device functions of the tensor kernels, under the policy `fast` names.          */
int fibhip_unit_laplace_tensor(int device, int height, int width, const float *a, const float *phi, const float *dyy,
                               const float *dxx, const float *dxy, int fast, float *out);

/* Courtemanche.calc_inter(V, mod) (court.py:273-429; court_ultra.py:445-450 for the last two) on a HOST array
 * of n voltages: out[k*n + i] = k-th intermediate of V[i], k in the insertion order of the reference's dict:
 * d_infinity tau_d f_infinity tau_f tau_w w_infinity m_inf tau_m h_inf tau_h j_inf tau_j tau_oa oa_infinity
 * tau_oi oi_infinity tau_ua ua_infinity tau_ui ui_infinity tau_xr xr_infinity tau_xs xs_infinity g_Kur f_NaK
 * i_NaCaa i_NaCab i_K1a i_Kra us_infinity tau_us   (FIBHIP_COURT_NINTER = 32 rows)                        */
/* Direct halo exchange (opt-in, FIBTF_HALO=direct): the ghost rows move by ncclSend/ncclRecv issued by the library
 * itself on the handle's stream, one RCCL kernel per exchange, instead of through the caller's communication
 * library.  RCCL is bound with dlopen: pass the path of the librccl the process uses (NULL if it is already loaded).
 *   fibhip_comm_open       once per process
 *   fibhip_comm_unique_id  on one rank; the caller broadcasts the 128 bytes
 *   fibhip_comm_check      every local reason fibhip_comm_init could refuse, without the collective: run it on every
 *                          rank and agree on the outcome BEFORE any rank enters fibhip_comm_init
 *   fibhip_comm_init       collective: every rank of the group, same id
 *   fibhip_comm_exchange   on an exchange tick (fibhip_halo_due), between step_edges and step_commit; -1 = no
 *                          neighbour on that side.  Needs FIBHIP_ROW_INTERLEAVED (one block per message).         */
typedef struct fibhip_halo_msg {
    long long offset;   /* floats from the base of the slab fibhip_halo_plan names */
    long long count;    /* floats */
    int peer;           /* rank of the neighbour */
    int send;           /* 1 = my rows go out, 0 = the neighbour's rows come in (my ghost rows) */
} fibhip_halo_msg;
/* the (at most 4) messages of one halo exchange of the open tick, in posting order; returns their number.
 * *slab_index = which of the two slabs (ext_slab[i]) they refer to.                                              */
int fibhip_halo_plan(fibhip_t h, int up_rank, int down_rank, fibhip_halo_msg *out4, int *slab_index);
int fibhip_comm_open(const char *librccl_path);
int fibhip_comm_unique_id(char *out128);
int fibhip_comm_check(fibhip_t h, int rank, int nranks);   /* the local (non-collective) checks of comm_init */
int fibhip_comm_init(fibhip_t h, const char *id128, int rank, int nranks);
int fibhip_comm_exchange(fibhip_t h, int up_rank, int down_rank);
int fibhip_comm_free(fibhip_t h);

/* Run-time modules: a traced model (FIBHIP_CUSTOM) without a compiler on the box and without a library of its own.
 * The caller compiles the model's DEVICE code in-process (hiprtc: the generated `struct Custom` + csrc/kernels.hpp and the kernel files it includes,
 * one name expression per kernel below) and hands the code object over; the stock library loads it and drives its
 * kernels with the same host logic as the built-in models.  `fibhip_desc.module` then selects it at fibhip_create.  */
typedef struct fibhip_module_kernel {
    const char *symbol;  /* lowered (mangled) name of the kernel in the code object                           */
    int kind;            /* 0 tick_kernel<Custom,P,MODE,K,TX,TY,NT,PHASE>, 1 strip_kernel<...,K,TX,TY,R,PHASE>,  */
                         /* 2 pointwise_kernel<Custom,P,MODE> (an assign group fired by fibhip_step_mode)       */
    int mode, fast, phase;
    int K, TX, TY, NT;   /* NT: threads per workgroup (tick) or -R (strip), as csrc/fibhip.hip lists its own    */
} fibhip_module_kernel;
typedef struct fibhip_module_desc {
    int struct_size;     /* sizeof(fibhip_module_desc)                                                        */
    int nvar;            /* Custom::NVAR                                                                      */
    int steps_per_tick;  /* Custom::DEFAULT_STEPS                                                             */
    int nmodes;          /* Custom::NMODES (assign groups; mode 0 = the tick op)                              */
    unsigned masks[8];   /* Custom::mask(mode): which arrays each group assigns                               */
    int consts_bytes;    /* sizeof(Custom::Consts)                                                            */
    int K, TX, TY, R, TYB, K2, TX2, TY2, R2;   /* FIB_CUSTOM_* plan hints of the generated header              */
    int nkernels;
    const fibhip_module_kernel *kernels;
} fibhip_module_desc;
typedef struct fibhip_module *fibhip_module_t;
int fibhip_module_load(int device, const void *code, size_t nbytes, const fibhip_module_desc *d, fibhip_module_t *out);
int fibhip_module_unload(fibhip_module_t m);   /* after every handle created on it has been destroyed */

/* measurement aid: best-of-`reps` rate of a plain device-to-device streaming copy of nbytes (read + written bytes
 * per second, GB/s) — the achievable-bandwidth yardstick printed next to the roofline peak                  */
int fibhip_copy_bandwidth(int device, size_t nbytes, int reps, float *gb_per_s);

/* Launches one empty kernel of THIS build of the library on `device`, so that its code object is the first one the HIP
 * runtime brings up.  fib_tf_amd calls it on the stock library before it uses any other build (a Beeler-Reuter table
 * baked in, a traced model compiled in): under rocprofv3 (ROCm 7.2) the first launch from the stock library AFTER
 * another build's kernels have run dies inside libamdhip64's launch path; the other order is fine.   */
int fibhip_warm(int device);

#define FIBHIP_COURT_NINTER 32
int fibhip_court_inter(int device, int n, const float *V, int fast, float *out);

/* introspection for DESIGN/bench: sub-steps fused per launch and launches per tick.  A handle whose multi-tick launches
 * exchange every K sub-steps with K below the tick's (Fenton 4v, an exchange-period row of the table: FIBHIP_VARIANT or
 * FIBHIP_K force one for every multi-tick launch) reports (K, 1); fibhip_ticks_per_launch still counts ticks, and
 * fibhip_plan_tile names that row's tile.  Where the first tick's measurement chose the row (or FIBHIP_PERIOD_ROW named it)
 * it runs the launches of LONG DECLARED series only (fibhip_expect of 128 ticks or more): both calls then name the shape
 * of those launches — every other launch of the handle runs the K = the tick's sub-steps plan                          */
int fibhip_launch_plan(fibhip_t h, int *fused_steps, int *launches_per_tick);
/* ... and the tile of the first launch: width, height, and rows per wave (strip kernels) or -threads per workgroup
 * (flat tile kernels)                                                                                              */
int fibhip_plan_tile(fibhip_t h, int *tile_w, int *tile_h, int *rows_per_wave);
/* The table of kernel variants THIS build of the library chooses its plans from (a specialised or a traced-model build
 * answers for its own table); neither call needs a device or a handle.  fibhip_variant_info fills out[0..9] with
 * model, mode, fast, phase, K, TX, TY, NT as the table lists them (model: a fibhip_model, 100 = Fenton 4v with the
 * zero-padded Laplacian, 101 = Courtemanche on aggregates; NT: threads of a flat tile, -rows per wave of a strip kernel,
 * -(32 + rows per wave) of a rows kernel), then the kernel kind (0 flat tile, 1 strip, 4 rows), then 1 if the row also
 * exists as a launch that advances several ticks of K sub-steps each (K = the tick's sub-steps; Fenton's row with K = 6 runs
 * several ticks per launch too, in exchange periods of K sub-steps, and is listed 0: as the plain strip launch of K
 * sub-steps it also is).  The kernels of a run-time module are not part of this table.                     */
int fibhip_variant_count(void);
int fibhip_variant_info(int i, int out[10]);
/* ... and the second table: the kernels of a handle with a diffusion tensor (fibhip_set_tensor), the same ten fields.  Flat
 * tiles, phase = 1 (the tensor's first-order term rides on the phase planes, with or without a field), both policies; the
 * model is the fibhip_model itself.  A build for one traced model has no row.                                      */
int fibhip_tensor_variant_count(void);
int fibhip_tensor_variant_info(int i, int out[10]);
/* Consecutive ticks one launch can cover (1 = every tick is its own launch or launches).  Courtemanche under
 * FIBHIP_FAST on one device returns 3: fibhip_step() accepts ticks and launches them three at a time, temporally
 * blocked; whatever has been accepted but not launched is launched by the next call that observes or changes the
 * state (get/set_state, probe, pace, sync, step_slow ...), so no caller can see the difference.
 * Fenton / Beeler-Reuter grids whose tiles are all resident on the device at once (tiles <= compute units; one device,
 * planar slab) return FIBHIP_MT_MAX (default 32): one launch then loops over up to that many ticks, its tiles re-reading
 * only the rim of their compute box from their neighbours between two ticks (no TensorFlow counterpart: ionic.py:202-204
 * issues one sess.run per tick).  A launch goes out as soon as the device would otherwise idle (see fibhip_step in
 * csrc/fibhip.hip); FIBHIP_MT=0 switches the mode off.  A tile of such a launch that waits 2 s for a neighbour gives up:
 * the next synchronising call restores the state that launch started from and goes on with one launch per tick
 * (fibhip_fallbacks).                                                                                             */
int fibhip_ticks_per_launch(fibhip_t h);
/* counters since fibhip_create: out[0] launches of any kernel, out[1] ticks advanced, out[2] multi-tick launches,
 * out[3] ticks those advanced (profiling scripts turn per-launch hardware counters into per-tick figures with them)  */
int fibhip_launch_stats(fibhip_t h, long long out[4]);
/* series of ticks that were launched ahead of the caller (fibhip_step: a whole series at its first tick when the last
 * series had that length; fibhip_get_state_direct: the next series before the frame is waited for) and that the caller
 * then cut short: out[0] launches that were stopped at the tick the caller had reached (nothing computed twice), out[1]
 * launches whose handed-out ticks had to be recomputed.  No TensorFlow counterpart (ionic.py:202-204 is synchronous).   */
int fibhip_spec_stats(fibhip_t h, long long out[2]);
/* Multi-tick launches that gave up waiting (a tile waited its full bound for a neighbour: not every workgroup was resident —
 * a CU mask, another process holding the device) and were RECOVERED: the handle went back to the state the launch had
 * started from (a launch writes the other slab only), switched multi-tick launches off for good and recomputed the lost
 * ticks one launch per tick — bit-identical, only slower.  out[0] such launches, out[1] ticks recomputed.  Non-zero out[0]
 * is worth a warning (fib_tf_amd prints one).  No TensorFlow counterpart (ionic.py:202-204 cannot fail this way).
 * fibhip_set_mt_wait_ms: the bound, per handle (default 2000; FIBHIP_MT_WAIT_MS presets it).                          */
int fibhip_fallbacks(fibhip_t h, long long out[2]);
int fibhip_set_mt_wait_ms(fibhip_t h, int ms);

/* Timeline of the launches of a tick (ionic.py:231-241 traces one sess.run with TensorFlow's timeline and writes a
 * Chrome trace): between trace_begin and trace_end every kernel launch of the handle is bracketed by a pair of HIP
 * events on its stream and nothing is deferred (one launch = one tick); trace_end waits for the stream and returns
 * the events: kernel family and shape, start relative to the first event and duration in microseconds.            */
typedef struct fibhip_trace_event {
    char name[96];            /* e.g. "strip_kernel<K=10, tile 44x25, 3 rows per wave>" */
    double start_us, dur_us;
    int K, tile_w, tile_h, rows_per_wave, ticks;
} fibhip_trace_event;
int fibhip_trace_begin(fibhip_t h);
int fibhip_trace_end(fibhip_t h, fibhip_trace_event *out, int max_events);   /* returns the number of events traced; the first */
                                                                              /* max_events of them are written (more = truncated) */

/* Activation recorder: per-cell maps of local activation time, cycle length and action-potential duration, kept on the
 * device and updated after every tick (no TensorFlow counterpart: the reference's drivers poll image(), ionic.py:207-224).
 * It watches state array `var` against two thresholds down <= up (units of that array).  Its own plane Vp holds the array
 * at the end of the previous observed tick (at observe_begin: the current state).  After observed tick k (k = 0 is the
 * first tick after observe_begin), with Vc the array now, tick = (float)(dt * steps_per_tick) and
 * t0 = (float)((double)k * dt * steps_per_tick), in float32, every operation rounded on its own, IEEE division:
 *   upstroke   Vp < up && Vc >= up:               t = t0 + ((up - Vp) / (Vc - Vp)) * tick; prev_up = last_up; last_up = t;
 *                                                  first_up = t if count == 0; count += 1
 *   downstroke Vp >= down && Vc < down, count > 0: t = t0 + ((Vp - down) / (Vp - Vc)) * tick; apd = t - last_up
 * and Vp = Vc.  first_up, last_up, prev_up, apd start as NaN, count (int32) as 0; NaN potentials record nothing.  Pacing
 * and set_state between two ticks count as part of the next tick.  While a recorder is attached every tick is one plain
 * launch (no multi-tick launches, no run-ahead) followed by the recorder's kernel.  Single-device handles only (no ghost
 * rows).
 *   fibhip_observe_begin  flushes and synchronises pending work, then attaches (again: re-attaches and clears the maps)
 *   fibhip_observe_get    one map, [height*width] float32 (which = FIRST..APD) or int32 (COUNT); blocks like get_state
 *   fibhip_observe_ticks  ticks observed since observe_begin (accepted ticks included)
 *   fibhip_observe_end    detaches and frees the maps; fibhip_destroy does the same                                      */
enum fibhip_obs_map { FIBHIP_OBS_FIRST_UP = 0, FIBHIP_OBS_LAST_UP = 1, FIBHIP_OBS_PREV_UP = 2, FIBHIP_OBS_APD = 3, FIBHIP_OBS_COUNT = 4 };
int fibhip_observe_begin(fibhip_t h, int var, float up, float down);
int fibhip_observe_get(fibhip_t h, int which, void *dst);
int fibhip_observe_ticks(fibhip_t h, long long *k);
int fibhip_observe_end(fibhip_t h);

/* Electrode recorder: weighted sums of one state array over rectangular patches, taken on the device every `every` ticks
 * and appended to a trace that stays on the device until it is read (the reference's electrodes: egm.py multiplies image()
 * by a Gaussian mask and takes the mean, once per millisecond; court_ultra.py keeps phi-weighted means of the same kind).
 * Electrode e is a rectangle [r0, r1) x [c0, c1) inside the grid and a dense float32 weight patch w_e of that shape,
 * row-major.  A recorder holds n electrodes (1 .. FIBHIP_MAX_ELECTRODES), the watched array `var`, a stride every >= 1 and
 * a capacity >= 1 in samples.  With k = ticks since electrode_begin (the first tick after it is k = 0), after every tick
 * with (k + 1) % every == 0 sample s = (k + 1) / every - 1 is taken:
 *     trace[s][e] = sum over (i, j) in rect_e of  w_e[i - r0, j - c0] * X_var[i, j]      (raw state values, float32)
 * The sum is float32 in a FIXED order that depends on the rectangle alone: the same state gives the same bits on every run,
 * whatever the launch plan (multi-tick launches on or off, after a recovered give-up, fused Courtemanche ticks).  No
 * floating-point atomics.  Accuracy: every product is rounded to float32 (or fused), and no term passes through more than
 * D(m) = ceil(m / 256) + 16 float32 additions, m = cells of the patch; hence against the exact sum S
 *     |trace - S| <= g * sum |w * X|,   g = (D + 1) u / (1 - (D + 1) u),   u = 2^-24
 * (the standard model: as long as no product underflows — a product below 2^-126 keeps fewer bits, below 2^-150 none).
 * Pacing, set_state and step_slow / step_mode between two ticks belong to the next tick.  Patches of any size up to the
 * whole grid are accepted.  The trace does not wrap: a fibhip_step that would take sample number `capacity` is refused with
 * FIBHIP_EINVAL ("trace full") before anything of that call is enqueued, and the handle stays usable (read, detach,
 * re-attach).  While a recorder is attached no launch spans a sample tick — between two samples the handle keeps its
 * multi-tick launches, cut at the sample ticks — and nothing runs ahead of the caller; a handle without one runs as ever.
 * A handle that runs multi-tick launches sends a launch only when the ticks up to the next sample tick (or as many as one
 * launch takes) have been accepted: a caller that steps tick by tick without observing anything leaves the device idle for
 * up to every - 1 of its calls; any call that observes the state launches what waits.  Courtemanche's tick is not fused
 * with the 'slow' operation behind it when a sample of one of the slow arrays is due at that tick.
 * Refused with FIBHIP_EINVAL: a row block (a handle with ghost rows), inside an open tick, a rectangle that is empty or not
 * inside the grid, n, every, capacity or var out of range, null pointers, weights that are not finite.
 *   fibhip_electrode_begin  flushes, synchronises and confirms pending work, copies rectangles (n x {r0, r1, c0, c1}) and
 *                           weights (the patches back to back) to the device and attaches; again: re-attaches, empty trace
 *   fibhip_electrode_count  samples taken so far (ticks accepted but not launched yet included)
 *   fibhip_electrode_read   samples [first, first + count) as [count][n] float32; flushes and blocks like get_state; does not
 *                           detach and does not reset the sample index, so a long run can be read in pieces
 *   fibhip_electrode_end    detaches and frees the trace (no recorder attached: nothing); fibhip_destroy does the same      */
#define FIBHIP_MAX_ELECTRODES 64
int fibhip_electrode_begin(fibhip_t h, int var, int n, const int *rects, const float *weights, int every, long long capacity);
int fibhip_electrode_count(fibhip_t h, long long *samples);
int fibhip_electrode_read(fibhip_t h, long long first, long long count, float *dst);
int fibhip_electrode_end(fibhip_t h);

/* Tip recorder: the phase singularities (spiral-wave tips, rotors) of two state arrays of the same tick, found on the device
 * every `every` ticks and kept there as compacted lists until they are read.  A = X[var] and B = X[var2] (var != var2) are
 * watched against the levels a0, b0: the state-space phase atan2(B - b0, A - a0).  The definition is exact integer
 * arithmetic on float32 inputs (restated in NumPy in tests/tip_ref.py; the device equals it bit for bit).  For every plaquette
 * with upper-left cell (i, j), 0 <= i < height - 1, 0 <= j < width - 1, take the corners in the order
 * (i,j) -> (i,j+1) -> (i+1,j+1) -> (i+1,j) -> (i,j) and at each a = A - a0, b = B - b0 (float32 subtractions).  For each of the
 * four edges (a1,b1) -> (a2,b2), cross = (double)a1 * (double)b2 - (double)a2 * (double)b1 (both products are exact in double,
 * so the sign is the exact sign):
 *     upward edge   (b1 < 0 && b2 >= 0): w += 1 if cross > 0
 *     downward edge (b2 < 0 && b1 >= 0): w -= 1 if cross < 0
 * NaN compares false: no crossing.  w in {-1, 0, +1} is the plaquette's charge; a tip is a plaquette with w != 0, at the
 * plaquette centre (i + 0.5, j + 0.5).  With a mask ([height*width] bytes) a plaquette counts only if all four corners have
 * a non-zero mask.  Sample s is taken after the tick with (k + 1) % every == 0, k = ticks since tips_begin: s = (k + 1) / every
 * - 1, the electrode recorder's rule.  Per sample the device keeps three int32 counters — n_pos, n_neg (tips of charge +1 /
 * -1: exact whatever max_tips is) and stored = n_pos + n_neg — and the first min(stored, max_tips) records {row i, column j,
 * charge, 0} in the order of arrival, which is not fixed: sort them.  stored > max_tips means the list was cut.
 * Pacing, set_state and step_slow / step_mode between two ticks belong to the next tick.  The lists do not wrap: a fibhip_step
 * that would take sample number `capacity` is refused with FIBHIP_EINVAL ("trace full") before anything of that call is
 * enqueued.  What holds for the electrode recorder holds here: no launch spans a sample tick, multi-tick launches go on
 * between two samples, nothing runs ahead, a launch goes out when the ticks up to the next sample tick have been accepted,
 * and Courtemanche's tick is not fused with 'slow' when a sample of a slow array (var or var2) is due at that tick.  Both
 * recorders may be attached at once, each with its own stride.
 * Refused with FIBHIP_EINVAL: a row block, inside an open tick, var or var2 out of range or equal, levels that are not
 * numbers, every < 1, max_tips outside 1 .. FIBHIP_MAX_TIPS, capacity < 1 or too large, a grid without a plaquette.
 *   fibhip_tips_begin  flushes, synchronises and confirms pending work, copies the mask (or none: NULL) and attaches; again:
 *                      re-attaches, empty lists
 *   fibhip_tips_count  samples taken so far (ticks accepted but not launched yet included)
 *   fibhip_tips_read   samples [first, first + count): counts as [count][3] = n_pos, n_neg, stored, and (unless NULL) records
 *                      as [count][max_tips][4]; flushes and blocks like get_state; does not detach
 *   fibhip_tips_end    detaches and frees (no recorder attached: nothing); fibhip_destroy does the same                       */
#define FIBHIP_MAX_TIPS 65536
int fibhip_tips_begin(fibhip_t h, int var, int var2, float a0, float b0, const unsigned char *mask /* [H*W] or NULL */,
                      int every, int max_tips, long long capacity);
int fibhip_tips_count(fibhip_t h, long long *samples);
int fibhip_tips_read(fibhip_t h, long long first, long long count,
                     int *counts  /* [count][3] = n_pos, n_neg, stored (may exceed max_tips: the list was cut) */,
                     int *records /* [count][max_tips][4], the first min(stored, max_tips) of each sample valid; may be NULL */);
int fibhip_tips_end(fibhip_t h);

/* Frame recorder: the movie.  Every `every` ticks a window of ONE state array is written on the device, as a frame, into a
 * cube that stays there until it is read (the reference's run(im) paints image() * phase every dt_per_plot sub-steps and its
 * drivers collect the frames into cube.npy).  Parameters: the watched array `var`; a window rows [r0, r1) x columns [c0, c1)
 * inside the grid; a block (by, bx), each 1 .. FIBHIP_MAX_FRAME_BLOCK; a reduction, POINT or MEAN; two float32 levels lo and
 * span (lo a number, span finite and not zero); a weight plane [height*width] float32 or NULL; a format, F32 or U8; every >= 1;
 * first in 1 .. every; capacity >= 1 frames.  A frame has oh = (r1 - r0) / by rows of ow = (c1 - c0) / bx pixels (integer
 * division: trailing cells are dropped; both must be >= 1).  Restated in NumPy in tests/frame_ref.py; the device equals that
 * bit for bit.  Per cell, in float32, every operation rounded on its own (no contraction, correctly rounded division):
 *     y = (X - lo) / span;      y = y * w   when a weight plane is given
 * With lo = (float)min_v, span = (float)(max_v - min_v), w = the phase field this is image() * phase of the stock models.
 *     POINT  the pixel is y of the block's upper-left cell
 *     MEAN   every block row is summed left to right, starting from its first cell; the row sums are added top to bottom,
 *            starting from the first row's; the total is divided by (float)(by * bx).  The order depends on the block alone:
 *            the same state gives the same bits under every launch plan.
 *     F32    stores the pixel
 *     U8     stores (unsigned char)(q * 255.0f + 0.5f), truncated, q = the pixel with NaN replaced by 0, then clamped to [0, 1]
 * Sample s follows tick number first + s * every, ticks counted from 1 at frames_begin: first = every is the cadence of the
 * electrode and tip recorders, first = 1 that of run(im) (a frame after ticks 0, every, 2 * every, ... of its loop).  Pacing,
 * set_state and step_slow / step_mode between two ticks belong to the next tick.  The cube does not wrap: a fibhip_step that
 * would take frame number `capacity` is refused with FIBHIP_EINVAL ("trace full") before anything of that call is enqueued.
 * What holds for the electrode and tip recorders holds here: no launch spans a sample tick, multi-tick launches go on between
 * two samples, nothing runs ahead, a launch goes out when the ticks up to the next sample tick have been accepted, and
 * Courtemanche's tick is not fused with 'slow' when a frame of a slow array is due at that tick.  All three may be attached
 * at once, each with its own stride.
 * Refused with FIBHIP_EINVAL: a row block, inside an open tick, and every argument outside the ranges above; a cube that cannot
 * be allocated: FIBHIP_ENOMEM.
 *   fibhip_frames_begin  flushes, synchronises and confirms pending work, copies the weight plane and attaches; again:
 *                        re-attaches, empty cube
 *   fibhip_frames_count  frames taken so far (ticks accepted but not launched yet included)
 *   fibhip_frames_shape  oh, ow and the bytes per pixel (4 or 1) of the attached recorder
 *   fibhip_frames_read   frames [first, first + count) as [count][oh][ow] float32 or uint8; flushes and blocks like get_state;
 *                        does not detach
 *   fibhip_frames_end    detaches and frees the cube (no recorder attached: nothing); fibhip_destroy does the same            */
#define FIBHIP_MAX_FRAME_BLOCK 16
enum fibhip_frame_reduce { FIBHIP_FRAME_POINT = 0, FIBHIP_FRAME_MEAN = 1 };
enum fibhip_frame_format { FIBHIP_FRAME_F32 = 0, FIBHIP_FRAME_U8 = 1 };
int fibhip_frames_begin(fibhip_t h, int var, const int *window /* r0, r1, c0, c1 */, int by, int bx, int reduce, float lo, float span,
                        const float *weight /* [H*W] or NULL */, int format, int every, int first, long long capacity);
int fibhip_frames_count(fibhip_t h, long long *samples);
int fibhip_frames_shape(fibhip_t h, int *oh, int *ow, int *bytes_per_pixel);
int fibhip_frames_read(fibhip_t h, long long first, long long count, void *dst);
int fibhip_frames_end(fibhip_t h);

/* Statistics recorder: whole-tissue scalars of several state arrays at once, taken on the device every `every` ticks and appended,
 * one row per sample, to a trace that stays on the device until it is read (the reference's court_ultra.py keeps phase-weighted
 * means of _Na_i_, _f_Ca_ and _us_ and the repolarised share of the tissue by reading whole arrays back; ionic.py has a NaN
 * detector commented out).  A recorder has ncols columns, 1 .. FIBHIP_MAX_STAT_COLS, at most FIBHIP_MAX_STAT_COLS_PER_ARRAY of
 * them on the same array; a column is {var, kind, level}.  It has an optional float32 weight plane [height*width], an optional
 * byte mask [height*width] (non-zero: the cell counts) and a stride every >= 1.  With k = ticks since stats_begin (the first
 * tick after it is k = 0), after every tick with (k + 1) % every == 0 sample s = (k + 1) / every - 1 is taken — the rule of the
 * electrode and tip recorders.  One sample is one row of ncols float64 values (restated in NumPy in tests/stats_ref.py):
 *     SUM        sum of (double)w * (double)X over the cells with w != 0; without a weight plane w = 1.  The product of two
 *                float32 numbers is exact in double; every addition is a float64 addition rounded on its own (the product is
 *                NOT fused into it: no fma), in an order fixed by height, width and the pitch alone.  No floating-point atomics.
 *                A NaN or Inf under a non-zero weight propagates; under a zero weight it is not looked at.  Against the exact
 *                sum S of the n terms: |SUM - S| <= n * 2^-53 * sum |w * X|.
 *     MIN, MAX   over the cells with mask != 0 (all cells without a mask), ignoring NaN; +-Inf take part.  No such cell (or
 *                NaN only): +inf for MIN, -inf for MAX.  -0 and +0 compare equal; which of them is stored is not specified.
 *     BELOW, ABOVE   the number of masked cells with X < level / X > level, compared in float32.  NaN counts in neither.
 *     NONFINITE  the number of masked cells whose X is NaN or +-Inf.
 * Counts are accumulated as integers (64-bit where they are combined) and stored converted to double, which is exact.  The
 * same state gives the same bytes under every launch plan: multi-tick launches on or off, run-ahead on or off, a forced tile
 * shape, after a recovered give-up.  The row of a sample is addressed from the host's tick counter, so a replay writes the same
 * row again.  Pacing, set_state and step_slow / step_mode between two ticks belong to the next tick.  The trace does not wrap:
 * a fibhip_step that would take sample number `capacity` is refused with FIBHIP_EINVAL ("trace full") before anything of that
 * call is enqueued.  What holds for the other samplers holds here: no launch spans a sample tick, multi-tick launches go on
 * between two samples, nothing runs ahead, a launch goes out when the ticks up to the next sample tick have been accepted, and
 * Courtemanche's tick is not fused with 'slow' when a sample is due at that tick and any column names a slow array.  The
 * recorder may be attached beside every other recorder, each with its own stride.
 * Refused with FIBHIP_EINVAL, the message naming the offender: var out of range, an unknown kind, a NaN level on BELOW or ABOVE,
 * a weight that is not finite, more than FIBHIP_MAX_STAT_COLS_PER_ARRAY columns on one array, ncols out of range, every < 1,
 * capacity < 1, a second stats_begin without a stats_end, inside an open tick, a row block (a handle with ghost rows).
 *   fibhip_stats_begin  flushes, synchronises and confirms pending work, copies the planes and attaches
 *   fibhip_stats_count  samples taken so far (ticks accepted but not launched yet included)
 *   fibhip_stats_read   samples [first, first + count) as [count][ncols] float64; flushes and blocks like get_state; does not
 *                       detach and does not reset the sample index
 *   fibhip_stats_end    detaches and frees the trace (no recorder attached: nothing); fibhip_destroy does the same             */
#define FIBHIP_MAX_STAT_COLS 64
#define FIBHIP_MAX_STAT_COLS_PER_ARRAY 8
enum fibhip_stat_kind { FIBHIP_STAT_SUM = 0, FIBHIP_STAT_MIN = 1, FIBHIP_STAT_MAX = 2, FIBHIP_STAT_BELOW = 3, FIBHIP_STAT_ABOVE = 4,
                        FIBHIP_STAT_NONFINITE = 5 };
typedef struct { int var; int kind; float level; } fibhip_stat_col;     /* kind: FIBHIP_STAT_SUM ... _NONFINITE */
int fibhip_stats_begin(fibhip_t h, int ncols, const fibhip_stat_col *cols, const float *weight /* [H*W] or NULL */,
                       const unsigned char *mask /* [H*W] or NULL */, int every, long long capacity);
int fibhip_stats_count(fibhip_t h, long long *samples);
int fibhip_stats_read(fibhip_t h, long long first, long long count, double *dst /* [count][ncols] */);
int fibhip_stats_end(fibhip_t h);

/* Lead recorder: unipolar electrograms.  An extracellular electrode sees the transmembrane current of every cell through a lead
 * field; the recorder forms that current from the watched array on the device every `every` ticks and appends one float64 per
 * lead to a trace that stays on the device until it is read.  With X the array `var` on the height x width grid, one sample is
 * (restated in NumPy in tests/lead_ref.py):
 *     source  on the interior cells 1 <= r <= height - 2, 1 <= c <= width - 2 only (the outer ring holds ghost copies and
 *             contributes nothing): S = the 9-point Laplacian in the reference's order over taps read at
 *             X[clamp(r + dr, 1, height - 2)][clamp(c + dc, 1, width - 2)], plus the phase-field term with the correctly
 *             rounded quotient where the handle has a phase field — laplace(enforce_boundary(X)) of the stand-alone array ops,
 *             always in the exact form, whatever the handle's arithmetic policy; float32, every operation rounded on its own.
 *     weight  q = w * S, one float32 product rounded on its own; w is the caller's plane [height*width], or 1 without one.
 *     lead    lead e sits at the cell (row_e, col_e) and names one of the ntables lead-field tables T, each float32
 *             [height][width]: K_e(r, c) = T[|r - row_e|][|c - col_e|].  Its term of a cell is (double)K_e * (double)q, exact;
 *             its value the float64 sum of the terms over the interior cells, every addition rounded on its own (no fma), in an
 *             order fixed by height and width alone — not by the number of leads, the stride, the launch plan or the run.
 *             Against the exact sum of the n terms: |value - sum| <= n * 2^-53 / (1 - n * 2^-53) * sum |term|.
 * A NaN in the interior makes every lead NaN.  The sample ticks, the capacity rule ("trace full"), the launches and the 'slow'
 * rule are those of the statistics recorder; the recorder may be attached beside every other recorder, each with its own stride.
 * Refused with FIBHIP_EINVAL, the message naming the offender: var out of range, n outside 1 .. FIBHIP_MAX_LEADS, ntables
 * outside 1 .. FIBHIP_MAX_LEAD_TABLES, a lead outside the grid or naming a table that is not there, a table or weight value that
 * is not finite, every < 1, capacity < 1, a grid smaller than 3 x 3, a handle with the zero-padded Laplacian (FIBHIP_ZEROPAD: its
 * diffusion term is not this source), inside an open tick, a row block (a handle with ghost rows).
 *   fibhip_leads_begin  flushes, synchronises and confirms pending work, copies positions, tables and the plane and attaches
 *   fibhip_leads_count  samples taken so far (ticks accepted but not launched yet included)
 *   fibhip_leads_read   samples [first, first + count) as [count][n] float64; flushes and blocks like get_state; does not detach
 *                       and does not reset the sample index
 *   fibhip_leads_end    detaches and frees the trace (no recorder attached: nothing); fibhip_destroy does the same             */
#define FIBHIP_MAX_LEADS 64
#define FIBHIP_MAX_LEAD_TABLES 4
int fibhip_leads_begin(fibhip_t h, int var, int n, const int *pos /* [n][3] = row, col, table */, int ntables,
                       const float *tables /* [ntables][H*W] */, const float *weight /* [H*W] or NULL */, int every, long long capacity);
int fibhip_leads_count(fibhip_t h, long long *samples);
int fibhip_leads_read(fibhip_t h, long long first, long long count, double *dst /* [count][n] */);
int fibhip_leads_end(fibhip_t h);

/* Potential-map recorder: the unipolar electrogram at every site of a lattice.  The lead recorder's source, seen through ONE
 * lead-field table truncated at a radius R, at as many sites as the grid has cells: every `every` ticks one float64 per site is
 * appended to a cube that stays on the device until it is read.  With X the array `var` on the height x width grid, one sample is
 * (restated in NumPy in tests/potential_ref.py):
 *     source   the plane q, float32: on the interior cells q = w * S exactly as the lead recorder forms it (S the 9-point
 *              Laplacian of the boundary-enforced array plus the phase-field term where the handle has a phase field, read from
 *              the handle's CURRENT phase planes — a lesion shows from the next sample on —, always in the exact form; w the
 *              caller's plane, or 1 without one); q = +0.0 on the outer ring of the grid and off the grid.
 *     sites    the window (r0, r1, c0, c1) and the step (sy, sx), each 1 .. FIBHIP_PMAP_MAX_STEP: site (i, j) sits at the cell
 *              (r0 + i * sy, c0 + j * sx), oh = ceil((r1 - r0) / sy) rows of ow = ceil((c1 - c0) / sx) sites.  A site may be
 *              any cell of the grid, the outer ring included.
 *     table    ONE float32 table T[R + 1][R + 1], R = 1 .. FIBHIP_PMAP_MAX_RADIUS: the weight of the cell (r + dr, c + dc) for
 *              the site at (r, c) is T[|dr|][|dc|], |dr|, |dc| <= R.
 *     sum      phi = +0.0; for dr = -R .. R ascending: p = +0.0; for dc = -R .. R ascending:
 *              p = p + (double)T[|dr|][|dc|] * (double)q[r + dr][c + dc]; then phi = phi + p.  Every addition is rounded on its
 *              own in float64; the product of two float32 values is exact in float64, so a fused multiply-add gives the same
 *              bits and is what the device uses.  The order depends on R alone — not on the grid, the lattice, the launch plan,
 *              the stride or the run.  Against the exact sum of the (2R + 1)^2 terms: |phi - sum| <= n u / (1 - n u) * sum |term|,
 *              n = (2R + 1)^2 + 2R + 1, u = 2^-53.
 * A NaN in one cell of X makes the sites within Chebyshev distance R + 1 of it NaN and no others.  The sample ticks, the
 * capacity rule ("trace full"), and the 'slow' rule are those of the lead recorder; the recorder may be attached beside every
 * other recorder, each with its own stride; on a shared tick its two kernels come directly behind the lead recorder's.
 *     summary  over the samples [first, first + count), count >= 2, per site, made on the device where the cube lies: vmin and
 *              vmax with the sample indices kmin and kmax (counted from the recorder's first sample), and dmin, the most
 *              negative d[s] = phi[s] - phi[s - 1] (one rounded subtraction) over s = first + 1 .. first + count - 1, with its
 *              index kd = s.  Strict compares, the first occurrence wins; each value starts from the first element (vmin = vmax
 *              = phi[first], dmin = d[first + 1]), so a NaN that is not first never replaces anything and one that is first stays.
 * Refused with FIBHIP_EINVAL, the message naming the offender: var out of range, a radius outside 1 .. FIBHIP_PMAP_MAX_RADIUS, a
 * step outside 1 .. FIBHIP_PMAP_MAX_STEP, a window that is empty or outside the grid, a table or weight value that is not
 * finite, every < 1, capacity < 1, a grid smaller than 3 x 3, a handle with the zero-padded Laplacian, inside an open tick, a
 * row block; with FIBHIP_ENOMEM, and nothing attached, a cube that cannot be allocated.
 *   fibhip_pmap_begin    flushes, synchronises and confirms pending work, copies the table and the plane and attaches
 *   fibhip_pmap_count    samples taken so far (ticks accepted but not launched yet included)
 *   fibhip_pmap_read     samples [first, first + count) as [count][oh][ow] float64; flushes and blocks like get_state; does not
 *                        detach and does not reset the sample index
 *   fibhip_pmap_summary  the six planes [oh][ow] of the summary (a null destination is skipped); flushes and blocks like _read
 *   fibhip_pmap_end      detaches and frees the cube (no recorder attached: nothing); fibhip_destroy does the same             */
#define FIBHIP_PMAP_MAX_RADIUS 32
#define FIBHIP_PMAP_MAX_STEP 16
int fibhip_pmap_begin(fibhip_t h, int var, int radius, const float *table /* [(R+1)*(R+1)] */, const float *weight /* [H*W] or NULL */,
                      const int *window /* r0, r1, c0, c1 */, int sy, int sx, int every, long long capacity);
int fibhip_pmap_count(fibhip_t h, long long *samples);
int fibhip_pmap_read(fibhip_t h, long long first, long long count, double *dst /* [count][oh][ow] */);
int fibhip_pmap_summary(fibhip_t h, long long first, long long count, double *vmin, double *vmax, double *dmin, int *kmin, int *kmax,
                        int *kd /* [oh][ow] each */);
int fibhip_pmap_end(fibhip_t h);

/* Wave recorder: the excited domains of the sheet, labelled and measured on the device.  Every `every` ticks the cells that meet
 * a condition are grouped into connected components, the WAVES; their number, and per wave its size, centroid sums and bounding
 * box, are appended to lists that stay on the device until they are read.  Restated in NumPy in tests/wave_ref.py.
 *     set     the cell (r, c) of the height x width grid is SET when mask[r][c] != 0 (NULL: every cell), the condition holds on
 *             the array `var` — kind FIBHIP_WAVE_ABOVE: X > level, FIBHIP_WAVE_BELOW: X < level, strict float32 compares, so a
 *             NaN is never set — and, if var2 >= 0, the condition (kind2, level2) holds on the array `var2` as well (var2 = -1:
 *             none).
 *     wave    two set cells are neighbours under conn = 4 (N, S, W, E) or conn = 8 (the diagonals too); a wave is a connected
 *             component of set cells.  Its SEED is the smallest linear index r * width + c among its cells: the wave's
 *             identity, a function of the plane alone.
 *     record  fibhip_wave_record: seed, area (cells), sum_r and sum_c (the 64-bit sums of the rows and the columns of its cells;
 *             the centroid is sum / area), and the inclusive bounding box r0 <= r <= r1, c0 <= c <= c1.
 *     counts  per sample int32[3] = n, stored, cells: the number of waves (exact however many there are), the number of
 *             records written = min(n, max_waves), and the number of set cells (exact).
 *     records up to max_waves per sample, in the order of arrival (sort by seed).  Where n > max_waves, WHICH waves are stored
 *             is unspecified (the tip recorder's contract); every stored record is whole and exact and no seed appears twice.
 *     labels  the int32 plane [height][width] of the LATEST sample: the seed of the cell's wave, -1 for a cell that is not set.
 * Everything is integer arithmetic on the outcome of the compares: the same on every launch plan, stride and policy.  The sample
 * ticks, the capacity rule ("trace full"), the launches and the 'slow' rule are those of the tip recorder; the recorder may be
 * attached beside every other recorder, each with its own stride.
 * Refused with FIBHIP_EINVAL, the message naming the offender: var out of range, var2 neither -1 nor in range, a kind that is
 * neither ABOVE nor BELOW, a level that is not finite, conn other than 4 or 8, max_waves outside 1 .. FIBHIP_MAX_WAVES,
 * every < 1, capacity < 1 or too large, inside an open tick, a row block (a handle with ghost rows).
 *   fibhip_waves_begin   flushes, synchronises and confirms pending work, copies the mask (or none: NULL) and attaches; again:
 *                        re-attaches with empty lists
 *   fibhip_waves_count   samples taken so far (ticks accepted but not launched yet included)
 *   fibhip_waves_read    samples [first, first + count): counts as [count][3] and (unless NULL) records as [count][max_waves],
 *                        of which the first `stored` of each sample are valid; flushes and blocks like get_state; does not detach
 *   fibhip_waves_labels  the label plane of the latest sample taken, confirmed; refused before the first sample
 *   fibhip_waves_end     detaches and frees (no recorder attached: nothing); fibhip_destroy does the same                      */
#define FIBHIP_MAX_WAVES 65536
enum fibhip_wave_kind { FIBHIP_WAVE_ABOVE = 0, FIBHIP_WAVE_BELOW = 1 };
typedef struct fibhip_wave_record {
    int seed, area;
    long long sum_r, sum_c;
    int r0, r1, c0, c1;
} fibhip_wave_record;               /* 40 bytes */
int fibhip_waves_begin(fibhip_t h, int var, int kind, float level, int var2, int kind2, float level2, int conn,
                       const unsigned char *mask /* [H*W] or NULL */, int max_waves, int every, long long capacity);
int fibhip_waves_count(fibhip_t h, long long *samples);
int fibhip_waves_read(fibhip_t h, long long first, long long count, int *counts /* [count][3] */,
                      fibhip_wave_record *records /* [count][max_waves] or NULL */);
int fibhip_waves_labels(fibhip_t h, int *dst /* [H*W] */);
int fibhip_waves_end(fibhip_t h);
/* Links: which wave of the sample before a wave of this sample shares cells with — what a host needs to tell a wave that split
 * from one that died while another was born beside it.  Opt-in; with links off the recorder launches and writes what it always
 * did.  Restated in tests/wave_link_ref.py.  With L[s] the label plane of sample s:
 *     link    for s >= 1 a pair (prev, seed) such that some cell c has L[s-1][c] = prev >= 0 and L[s][c] = seed >= 0; its
 *             OVERLAP is the number of such cells.  Sample 0 has no links.  Links depend on the label planes alone, not on
 *             max_waves or on which records were stored.
 *     counts  per sample int32[4] = links, stored, cells, lost: the number of distinct pairs that found a place in the sample's
 *             table; the records written = min(links, max_links); the cells set in both planes (always exact); and the cells
 *             whose pair found no place in the table.  While lost == 0, `links` is the exact number of distinct pairs.
 *     records fibhip_wave_link, up to max_links per sample, in the order of arrival (sort by (prev, seed)).  Every stored record
 *             is whole, its overlap exact, and no pair appears twice; where links > max_links, WHICH pairs are stored is
 *             unspecified.
 *     table   the pairs of a sample are collected in a hash table of T entries, T the smallest power of two >= 4 * max_links,
 *             probed at most 32 times per insertion (the walk visits every entry of a table of T <= 32).  A sample with at
 *             most max_links pairs loses none when T <= 32 and otherwise one with probability <= 4^-32 per pair.
 *   fibhip_waves_links_begin   turns links on for the attached wave recorder: right behind fibhip_waves_begin — refused once the
 *                              recorder has seen a tick (launched or pending), when links are on already, without a recorder,
 *                              inside an open tick, for max_links outside 1 .. FIBHIP_MAX_WAVE_LINKS or lists that would not
 *                              fit size_t.  FIBHIP_ENOMEM leaves the wave recorder attached without links
 *   fibhip_waves_links_read    samples [first, first + count): counts as [count][4] and (unless NULL) records as
 *                              [count][max_links], the first `stored` of each sample valid; flushes and blocks like
 *                              fibhip_waves_read; refused while links are off
 * fibhip_waves_end, fibhip_waves_begin (again) and fibhip_destroy free the link buffers with the rest.                            */
#define FIBHIP_MAX_WAVE_LINKS 65536
typedef struct { int prev, seed, overlap; } fibhip_wave_link;      /* 12 bytes */
int fibhip_waves_links_begin(fibhip_t h, int max_links);
int fibhip_waves_links_read(fibhip_t h, long long first, long long count, int *counts /* [count][4] */,
                            fibhip_wave_link *links /* [count][max_links] or NULL */);

/* Spectrum recorder: per-cell power spectra (a Welch periodogram) folded on the device while the run goes on, and the
 * dominant-frequency maps made from them — the sixth recorder and the fifth sampler.  All device arithmetic is float32, every
 * operation rounded on its own (no contraction), in the order written; no transcendental is evaluated on the device.
 * Parameters: the watched array `var`; a window rows [r0, r1) x columns [c0, c1), a block (by, bx), each 1 ..
 * FIBHIP_MAX_FRAME_BLOCK, and a reduction POINT or MEAN — exactly the frame recorder's, with its pixel definition, its
 * summation order and oh, ow as there, at the fixed levels lo = 0, span = 1: a pixel is the array's own value or block mean —;
 * an optional weight plane; every >= 1: sample s follows tick (s + 1) * every, ticks counted from 1 at spectrum_begin;
 * nfft = N, FIBHIP_SPECTRUM_MIN_NFFT .. FIBHIP_SPECTRUM_MAX_NFFT, the segment length in samples; win[N] float32 and tw[N][2]
 * float32, supplied by the caller (the Python layer fills tw[m] with cos(2 pi m / N) and -sin(2 pi m / N), computed in float64
 * and then rounded); bins[nb], nb = 1 .. FIBHIP_SPECTRUM_MAX_BINS strictly ascending integers in [0, N / 2]; chunk,
 * 1 .. FIBHIP_SPECTRUM_MAX_CHUNK with N % chunk == 0.
 * Fold.  Sample s has position j = s mod N in its segment and pixel value x.  y = x * win[j].  For every bin i with frequency
 * index k = bins[i], m = (k * j) mod N in integers, and  Re_i = Re_i + y * tw[m][0],  Im_i = Im_i + y * tw[m][1].  Samples are
 * folded in ascending s; Re and Im start every segment at +0.
 * Segment end.  After the sample with j = N - 1:  P_i = P_i + ((Re_i * Re_i) + (Im_i * Im_i)), then Re_i = Im_i = +0, then
 * segments += 1.  P starts at +0 at spectrum_begin.  No overlap, no detrending (with the periodic Hann window a constant leaks
 * into bins 0 and +-1 only).  The samples of an unfinished segment are part of nothing that can be read.
 * The result is a pure function of the sampled states: it does not depend on `chunk` (how many samples one fold launch takes)
 * or on the launch plan.
 * Peak maps over the bin POSITIONS a <= i <= b (0 <= a <= b < nb), halfwidth >= 0, each [oh][ow]:
 *   kpeak (int32)  walk i = a .. b: the first P_i that is a number (P_i == P_i) is taken, after that every P_i strictly greater
 *                  (>) than the one held; kpeak is the position held at the end — the largest P, the lowest position on a tie.
 *                  -1 when segments == 0 or no P_i is a number
 *   ppeak          P at that position; NaN where kpeak = -1
 *   pband          the float32 sum of P_i, i = a .. b ascending, starting from its first term
 *   pnear          the same sum over max(a, kpeak - halfwidth) .. min(b, kpeak + halfwidth); NaN where kpeak = -1
 * It may be attached beside every other recorder and both stimulus programs (on a shared tick its sample is taken before that
 * tick's stimuli); not on a handle with ghost rows or a row-interleaved slab; one at a time.  While attached nothing runs
 * ahead and no launch spans a sample tick.
 *   fibhip_spectrum_begin  validates, flushes, synchronises and confirms pending work, copies the tables and attaches
 *   fibhip_spectrum_count  samples taken and segments finished (ticks accepted but not launched yet included); either may be NULL
 *   fibhip_spectrum_shape  oh, ow and nb of the attached recorder
 *   fibhip_spectrum_read   the raw P as [nb][oh][ow] float32 and the segment count; flushes and blocks like get_state
 *   fibhip_spectrum_peak   the four maps (any may be NULL); flushes and blocks like get_state
 *   fibhip_spectrum_end    detaches and frees (no recorder attached: nothing); fibhip_destroy does the same                  */
#define FIBHIP_SPECTRUM_MAX_BINS 128
#define FIBHIP_SPECTRUM_MAX_CHUNK 32
#define FIBHIP_SPECTRUM_MIN_NFFT 4
#define FIBHIP_SPECTRUM_MAX_NFFT 65536
int fibhip_spectrum_begin(fibhip_t h, int var, const int *window /* r0, r1, c0, c1 */, int by, int bx, int reduce,
                          const float *weight /* [H*W] or NULL */, int every, int nfft, const float *win /* [nfft] */,
                          const float *tw /* [nfft][2] */, int nb, const int *bins /* [nb] */, int chunk);
int fibhip_spectrum_count(fibhip_t h, long long *samples, long long *segments);
int fibhip_spectrum_shape(fibhip_t h, int *oh, int *ow, int *nb);
int fibhip_spectrum_read(fibhip_t h, float *P /* [nb][oh][ow] */, long long *segments);
int fibhip_spectrum_peak(fibhip_t h, int a, int b, int halfwidth, int *kpeak, float *ppeak, float *pband, float *pnear /* [oh][ow] each */);
int fibhip_spectrum_end(fibhip_t h);

/* Beat recorder: a per-cell history of the last `depth` beats — upstroke time, downstroke time and peak of each — kept on the
 * device while the run goes on, and the summary maps made from it (APD, cycle length, alternans): the seventh recorder and the
 * sixth sampler.  All device arithmetic is float32, every operation rounded on its own (no contraction), in the order written;
 * division is IEEE — the activation recorder's contract.
 * Parameters: the watched array `var`; a window rows [r0, r1) x columns [c0, c1), a block (by, bx), each 1 ..
 * FIBHIP_MAX_FRAME_BLOCK, a reduction POINT or MEAN and an optional weight plane — exactly the frame recorder's, with its pixel
 * definition, its summation order and oh, ow as there, at the fixed levels lo = 0, span = 1 (the spectrum recorder's pixel);
 * every >= 1; two levels down <= up; depth = 1 .. FIBHIP_BEATS_MAX_DEPTH.
 * Samples.  Sample s (0-based) follows tick (s + 1) * every, ticks counted from 1 at beats_begin.  With dt and steps_per_tick
 * the handle's:  step = (float)((double)every * dt * steps_per_tick),  t0 = (float)((double)(s * every) * dt * steps_per_tick);
 * at every = 1 these are the activation recorder's `tick` and `t0`.  Times are milliseconds since beats_begin.
 * State per pixel: xp, the pixel at the previous sample (at beats_begin: the pixel of the current state); pk, the running peak
 * of the beat in progress (NaN outside a beat and at beats_begin); n, the int32 count of upstrokes.  The ring: three planes
 * t_up, t_down, peak, each [depth][oh * ow], all NaN at beats_begin; beat number b lives in slot b mod depth.
 * Per sample, xc the pixel now:
 *   1. upstroke, when xp < up && xc >= up:  if pk is a number (a beat was still open) peak[(n - 1) mod depth] = pk, and that
 *      beat's t_down stays NaN; then t = t0 + ((up - xp) / (xc - xp)) * step; slot n mod depth gets t_up = t, t_down = NaN,
 *      peak = NaN; pk = xc; n += 1
 *   2. downstroke, when xp >= down && xc < down and pk is a number:  t = t0 + ((xp - down) / (xp - xc)) * step; slot
 *      (n - 1) mod depth gets t_down = t, peak = pk; pk = NaN.  (The first downstroke closes the beat: a later dip without an
 *      upstroke in between finds pk = NaN and records nothing)
 *   3. otherwise, if pk is a number:  pk = (xc > pk) ? xc : pk
 *   4. then xp = xc
 * NaN compares false: a NaN sample is no event and leaves pk alone.  With down <= up cases 1 and 2 exclude each other.  What
 * fibhip_pace, a stimulus or fibhip_set_state writes between two samples belongs to the next sample.
 * Summary maps over the newest `last` beats (1 .. depth), each [oh][ow].  For a pixel with count n the walk is the beats
 * b = max(0, n - min(n, depth), n - last) .. n - 1, ascending, with apd_b = t_down_b - t_up_b:
 *   nused (int32)  the beats of the walk whose apd_b is a number
 *   apd_mean       the float32 sum of those apd_b, ascending, starting from its first term, divided by (float)nused
 *   cl_mean        the same over cl_b = t_up_b - t_up_(b-1) for the pairs (b - 1, b) both in the walk: the terms that are
 *                  numbers, summed ascending from the first, divided by (float) their number
 *   apd_alt        over the pairs (b - 1, b) both in the walk whose APDs are both numbers: d = apd_b - apd_(b-1), the term is d
 *                  for odd b and -d for even b; summed ascending from the first term and divided by (float) the number of
 *                  pairs.  Its magnitude is the alternans amplitude; a change of its sign across the sheet is discordant alternans
 * Each map is NaN where it has no term; nused is 0 there.
 * It may be attached beside every other recorder and both stimulus programs (on a shared tick its sample is taken before that
 * tick's stimuli); not on a handle with ghost rows or a row-interleaved slab; one at a time.  While attached nothing runs
 * ahead and no launch spans a sample tick; the result does not depend on the launch plan.
 *   fibhip_beats_begin    validates, flushes, synchronises and confirms pending work, makes xp from the current state, attaches
 *   fibhip_beats_count    samples taken (ticks accepted but not launched yet included)
 *   fibhip_beats_shape    oh, ow and depth of the attached recorder
 *   fibhip_beats_read     the ring planes in SLOT order, [depth][oh][ow] float32 each, the counts [oh][ow] int32 and the live pk
 *                         [oh][ow] float32 (any may be NULL); flushes and blocks like get_state
 *   fibhip_beats_summary  the four maps (any may be NULL); flushes and blocks like get_state
 *   fibhip_beats_end      detaches and frees (no recorder attached: nothing); fibhip_destroy does the same                   */
#define FIBHIP_BEATS_MAX_DEPTH 16
int fibhip_beats_begin(fibhip_t h, int var, const int *window /* r0, r1, c0, c1 */, int by, int bx, int reduce,
                       const float *weight /* [H*W] or NULL */, int every, float up, float down, int depth);
int fibhip_beats_count(fibhip_t h, long long *samples);
int fibhip_beats_shape(fibhip_t h, int *oh, int *ow, int *depth);
int fibhip_beats_read(fibhip_t h, float *t_up, float *t_down, float *peak /* [depth][oh][ow] each */, int *count, float *pk /* [oh][ow] each */);
int fibhip_beats_summary(fibhip_t h, int last, int *nused, float *apd_mean, float *cl_mean, float *apd_alt /* [oh][ow] each */);
int fibhip_beats_end(fibhip_t h);

/* Velocity fit: the gradient of activation time at every pixel, from a plane fitted to the activation times of a space-time
 * window around it (Bayly et al. 1998) — made on the device at read time from the planes the beat recorder and the activation
 * recorder keep there, like the summary maps.  The conduction velocity is the gradient's reciprocal (fib_tf_amd/velocity.py).
 * Inputs: a ring of time planes t[depth][oh * ow] (float32, ms) and a count plane n[oh * ow] (int32): beat b of a pixel lies in
 * slot b mod depth, and the pixel HOLDS the beats n - min(n, depth) .. n - 1 (none for n <= 0).  back >= 0, the beat under the
 * fit, counted from the newest; radius R = 1 .. FIBHIP_VEL_MAX_RADIUS; max_dt, float32, finite and > 0; min_cells =
 * 3 .. (2R + 1)^2; an optional mask [oh * ow] of bytes, non-zero where a pixel counts.
 * Centre.  Pixel p = (y, x) with beat b = n[p] - 1 - back.  If b is not held, the mask excludes p, or tc = t[b mod depth][p] is
 * NaN: nfit = 0 and gy = gx = rms = NaN.
 * Neighbour matching.  The offsets (dy, dx) are visited dy = -R .. R outermost, dx = -R .. R inside it.  A neighbour
 * q = (y + dy, x + dx) takes part if it lies inside the plane and inside the mask.  Its held beats are walked in ascending beat
 * number with d = t_q - tc, ONE float32 subtraction; the beat with the smallest |d| under a strict < is kept (a tie keeps the
 * older beat; a NaN d is never kept); q is USED if a beat was kept and |d| <= max_dt.  The centre meets itself with d = 0, no
 * special case.  Neighbours whose beat numbers differ from the centre's (a missed beat, a ring that wrapped) are so matched by
 * time, not by index.
 * Sums over the used cells in visiting order.  Integers, exact: N, Sy = sum dy, Sx = sum dx, Syy, Sxx, Sxy.  float64:
 * St = sum d, Syt = sum dy * d, Sxt = sum dx * d, Stt = sum d * d, each product formed in float64 from the float32 d, every
 * addition rounded on its own (no fma), each sum starting from +0.
 * Solve.  Integers: cyy = N Syy - Sy^2, cxx = N Sxx - Sx^2, cxy = N Sxy - Sy Sx, det = cyy cxx - cxy^2.  float64, in the order
 * written: cyt = N Syt - Sy St, cxt = N Sxt - Sx St.  If N < min_cells or det == 0: nfit = N, the rest NaN.  Otherwise
 *   gy  = (cxx cyt - cxy cxt) / det
 *   gx  = (cyy cxt - cxy cyt) / det
 *   a   = (St - (gy Sy + gx Sx)) / N
 *   sse = Stt - ((a St + gy Syt) + gx Sxt)
 *   rms = sqrt(max(sse, 0) / N)
 * with IEEE float64 division and square root.  Stored: nfit = N (int32); gy, gx, rms rounded once to float32.  gy and gx are the
 * gradient of activation time in ms per pixel along rows and columns, rms the residual of the fit in ms.
 *   fibhip_beats_velocity    on the beat recorder's t_up ring and counts (depth its own; back = 0 .. depth - 1); the mask is
 *                            [oh][ow] of its pixel plane, or NULL.  Any map may be NULL; flushes and blocks like beats_summary
 *   fibhip_observe_velocity  the same at depth 1, back 0 on one time plane of the activation recorder, which = FIBHIP_OBS_FIRST_UP,
 *                            _LAST_UP or _PREV_UP, with its count plane: a NaN time (prev_up after one upstroke) is never used.
 *                            The mask is [height][width] or NULL
 *   fibhip_velocity_fit      the same on host planes copied through `device`, without a handle (for the tests)               */
#define FIBHIP_VEL_MAX_RADIUS 4
int fibhip_beats_velocity(fibhip_t h, int back, int radius, float max_dt, int min_cells, const unsigned char *mask /* [oh*ow] or NULL */,
                          int *nfit, float *gy, float *gx, float *rms /* [oh][ow] each */);
int fibhip_observe_velocity(fibhip_t h, int which, int radius, float max_dt, int min_cells, const unsigned char *mask /* [H*W] or NULL */,
                            int *nfit, float *gy, float *gx, float *rms /* [height][width] each */);
int fibhip_velocity_fit(int device, int depth, int oh, int ow, const float *t /* [depth][oh*ow] */, const int *count /* [oh*ow] */, int back,
                        int radius, float max_dt, int min_cells, const unsigned char *mask /* [oh*ow] or NULL */, int *nfit, float *gy,
                        float *gx, float *rms /* [oh][ow] each */);

/* Stimulus program: stimuli applied on the device at programmed ticks, from sites of any shape, without a call per stimulus
 * (the reference's only stimulus is add_pace_op / fire_op, fired from the caller's loop body: `if i == s2: fire_op('s2')`;
 * fibhip_pace stands in for it and stays as it is).  A program is 1 .. FIBHIP_MAX_STIM_ENTRIES entries
 * {var, mode, shape, first, period, count, hold} and up to FIBHIP_MAX_STIM_PLANES float32 planes [height*width].  Restated in
 * NumPy in tests/stim_ref.py; the device equals that bit for bit.
 * Event ticks.  With k = ticks since stim_begin (the first tick after it is k = 0), entry e is applied right after the tick that
 * makes k + 1 == first + 1 + j * period + d, for j = 0 .. count - 1 and d = 0 .. hold - 1.  first >= 0; hold >= 1; period == 0
 * means one event (count must be 1); count == 0 with period > 0 means without end; hold <= period when period > 0.  first = i is
 * "after tick i of the loop", where `for i in m.run(): if i == s2: m.fire_op('s2')` puts it; a stimulus before any tick stays
 * fibhip_pace's job.
 * Modes, on the cells of array `var` (any state array; 0 is the potential), S the entry's value at the cell:
 *     MAX   X = fmaxf(X, S)       fibhip_pace's operation (NumPy: np.fmax)
 *     ADD   X = X + S             one float32 addition, rounded on its own
 * A cell whose S is the mode's "untouched" value — -inf for MAX, +0 or -0 for ADD — is not written: its bits stay whatever they
 * are (a NaN stays that NaN, -0 stays -0).
 * Shapes.
 *     RECT   rows [r0, r1) x columns [c0, c1), inside the grid and not empty: S = v inside (finite), `floor` outside (finite; -inf
 *            for MAX).  MAX with floor = min_v is fibhip_pace(r0, r1, c0, c1, v, min_v), bit for bit; floor = -inf (MAX) or 0 (ADD)
 *            leaves the outside untouched.
 *     PLANE  S = planes[plane][cell].  At attach the host takes the bounding box of the cells that are not "untouched"; only that
 *            box is visited.
 * Order.  The entries due after the same tick are applied in program order in one launch (eight entries per launch; a thread
 * reads each of its cells once and writes it once, whatever the number of entries).  Samples of the samplers and the activation
 * recorder's update of that tick come first: a stimulus belongs to the next tick, as fibhip_pace between two ticks does.
 * Courtemanche: a tick with an event due is never fused with the fibhip_step_slow behind it (the stimulus comes right after its
 * tick, before anything the caller does next), and on a handle that runs on aggregates an entry on one of the 17 slow arrays
 * marks them stale, as fibhip_set_state does.
 * Launches.  No launch spans an event tick; between events the handle keeps its multi-tick launches, and a launch goes out when
 * the ticks up to the next event have been accepted (the samplers' rule).  Nothing runs ahead of the caller while a program is
 * attached.  The stimulus is queued on the handle's stream behind the launch that ends at its tick; nothing waits for it.  A
 * multi-tick launch that gave up is recovered as ever: the replay applies the events of the replayed ticks again and no others.
 * The same program gives the same bytes under every launch plan.
 * Refused with FIBHIP_EINVAL, the message naming the entry: var, mode, shape or plane index out of range, a rectangle that is
 * empty or not inside the grid, v or floor that is not finite (floor = -inf is MAX's "untouched"), first < 0, hold < 1, hold >
 * period, period == 0 with count != 1, negative period or count; n or nplanes out of range, a second stim_begin without a
 * stim_end, inside an open tick, a row block (a handle with ghost rows).
 *   fibhip_stim_begin  flushes, synchronises and confirms pending work, copies the planes and attaches
 *   fibhip_stim_count  flushes, then the number of events applied so far (every (entry, tick) pair counts once)
 *   fibhip_stim_end    flushes, synchronises, detaches and frees (no program attached: nothing); fibhip_destroy frees too       */
#define FIBHIP_MAX_STIM_ENTRIES 64
#define FIBHIP_MAX_STIM_PLANES 8
enum fibhip_stim_mode { FIBHIP_STIM_MAX = 0, FIBHIP_STIM_ADD = 1 };
enum fibhip_stim_shape { FIBHIP_STIM_RECT = 0, FIBHIP_STIM_PLANE = 1 };
typedef struct fibhip_stim_entry {
    int var, mode, shape;       /* state array; FIBHIP_STIM_MAX / _ADD; FIBHIP_STIM_RECT / _PLANE */
    int r0, r1, c0, c1;         /* RECT */
    float v, floor;             /* RECT */
    int plane;                  /* PLANE: index into the planes */
    int first, period, count, hold;
} fibhip_stim_entry;
int fibhip_stim_begin(fibhip_t h, int n, const fibhip_stim_entry *entries, int nplanes, const float *planes /* [nplanes][H*W] or NULL */);
int fibhip_stim_count(fibhip_t h, long long *applied);
int fibhip_stim_end(fibhip_t h);

/* Trigger program: triggered stimulation — sense a site, decide, fire a stimulus, all on the device.  A stimulus program
 * (above) applies each entry at a tick fixed before the run; a trigger program applies a stimulus at a time that depends on the
 * STATE: an S2 a fixed delay after the S1 waveback has passed a probe, a demand pacer that fires when nothing arrived within an
 * escape interval, a burst on detection of an arrival.  A program is 1 .. FIBHIP_MAX_TRIG_SENSORS sensors, 1 ..
 * FIBHIP_MAX_TRIG_RULES rules, a stride `every` >= 1 in ticks and a `capacity` in samples.  One program per handle.  Restated in
 * NumPy in tests/trigger_ref.py; the device equals that bit for bit — everything here is integer arithmetic on float32
 * comparisons, there is no tolerance.
 * Samples.  Sample s = 0, 1, ... is taken after tick (s + 1) * every - 1 since trig_begin (the first tick after it is tick 0):
 * the other samplers' cadence.  ALL times of a rule are in samples.
 * Order on a tick.  The recorders' samples and the activation recorder's update come first, then the stimuli of an attached
 * stimulus program due after that tick, then sense, decide and the triggered stimuli: a sensor therefore SEES that tick's
 * programmed stimulus.  Courtemanche: a sample tick is never fused with the fibhip_step_slow behind it (tick, sense / stimulus,
 * slow).
 * Sensor {var, level, need, site}: site is FIBHIP_TRIG_RECT (rows [r0, r1) x columns [c0, c1), inside the grid, not empty) or
 * FIBHIP_TRIG_MASK (the cells where the sensor's uint8 mask [height*width] is not 0; the masks of the MASK sensors lie back to
 * back in `masks`, in sensor order; the host cuts each mask's bounding box at attach).  The count is
 *     c = #{cells of the site with X_var > level}        a strict float32 comparison: a NaN does not count
 * and the sensor is active when a = (c >= need), 1 <= need <= cells of the site.  An integer, independent of order — deliberately
 * not a float sum: the electrode sums carry an error bound, a decision must not.
 * Rule {sensor, edge, arm, blank, escape, max_det, delay, count, period, hold} + a stimulus {var, mode, shape, r0, r1, c0, c1, v,
 * floor, plane}: fibhip_stim_entry's fields with its rules (MAX / ADD, RECT / PLANE, the "untouched" value of a mode).  Per rule,
 * row s of the log holds the int32 fields {c, a, t, n, cause, fired}: the sensor's count and activity, samples since the last
 * detection (-1: none yet), detections so far, the cause of a detection at this sample (0 none, 1 an edge, 2 the escape
 * interval) and whether the stimulus is applied after this sample.  The virtual row -1 is a = -1 (unknown), t = -1, n = 0.
 * With p the previous row:
 *     e       = p.a >= 0 and (edge == RISE ? (p.a == 0 and a == 1) : (p.a == 1 and a == 0))
 *     listen  = s >= arm and (max_det == 0 or p.n < max_det) and (p.t < 0 or p.t + 1 >= blank)
 *     quiet   = escape > 0 and listen and ((p.t < 0 ? s - arm : p.t) + 1 >= escape)
 *     det     = listen and (e or quiet);   cause = det ? (e ? 1 : 2) : 0
 *     t       = det ? 0 : (p.t < 0 ? -1 : p.t + 1);      n = p.n + det
 *     u       = t - delay
 *     fired   = t >= 0 and u >= 0 and (period == 0 ? u < hold : (u / period < count and u % period < hold))
 * (the first sample is never an edge: its predecessor is unknown).  The stimuli of the rules with `fired` are applied right after
 * sample s, in rule order, with the stimulus program's operations: a triggered MAX on a rectangle floored at min_v equals
 * fibhip_pace bit for bit.
 * Launches.  No launch spans a sample tick; between samples the handle keeps its multi-tick launches, a launch goes out when the
 * ticks up to the next sample have been accepted, nothing runs ahead of the caller while a program is attached.  A sample is
 * three small launches queued on the handle's stream behind the launch that ends at its tick; nothing waits for them.  A
 * multi-tick launch that gave up is recovered as ever: the replay rewrites the rows of the replayed samples in order, the
 * stimuli behind the lost launch wrote nothing — no detection is lost or doubled.  The same program gives the same bytes under
 * every launch plan.  The rows stay on the device until they are read; a fibhip_step that would overflow `capacity` is refused
 * before it enqueues anything.
 * Refused with FIBHIP_EINVAL, the message naming the sensor or rule: counts, var, site, edge, mode, shape or plane out of range;
 * a level that is NaN; need outside 1 .. cells of the site; a time that is negative or above FIBHIP_TRIG_MAX_TIME; count < 1,
 * hold < 1, hold > period when period > 0, period == 0 with count != 1; blank < delay + (count - 1) * period + hold (a train is
 * never cut by a new detection); every < 1, a bad capacity; a second trig_begin without a trig_end; inside an open tick; a row
 * block (a handle with ghost rows); on a Courtemanche handle that runs on aggregates, a rule whose stimulus names one of the 17
 * slow arrays (the host cannot know when it fires, so it cannot mark the aggregates stale; the four fast arrays are fine).
 *   fibhip_trig_begin  flushes, synchronises and confirms pending work, copies masks and planes and attaches
 *   fibhip_trig_count  the samples taken so far (ticks accepted but not launched yet count)
 *   fibhip_trig_read   flushes, copies rows [first, first + count) out as [count][nrules][FIBHIP_TRIG_ROW] int32, synchronises;
 *                      copies again when a launch in front had given up and was recovered
 *   fibhip_trig_end    flushes, synchronises, detaches and frees (no program attached: nothing); fibhip_destroy frees too       */
#define FIBHIP_MAX_TRIG_SENSORS 8
#define FIBHIP_MAX_TRIG_RULES 8
#define FIBHIP_TRIG_ROW 6
#define FIBHIP_TRIG_MAX_TIME (1 << 24)
enum fibhip_trig_edge { FIBHIP_TRIG_RISE = 0, FIBHIP_TRIG_FALL = 1 };
enum fibhip_trig_site { FIBHIP_TRIG_RECT = 0, FIBHIP_TRIG_MASK = 1 };
enum fibhip_trig_field { FIBHIP_TRIG_C = 0, FIBHIP_TRIG_A = 1, FIBHIP_TRIG_T = 2, FIBHIP_TRIG_N = 3, FIBHIP_TRIG_CAUSE = 4, FIBHIP_TRIG_FIRED = 5 };
typedef struct fibhip_trig_sensor {
    int var;
    float level;
    int need;
    int site;                   /* FIBHIP_TRIG_RECT / _MASK */
    int r0, r1, c0, c1;         /* RECT */
} fibhip_trig_sensor;
typedef struct fibhip_trig_rule {
    int sensor, edge;           /* index of the sensor; FIBHIP_TRIG_RISE / _FALL */
    int arm, blank, escape, max_det, delay, count, period, hold;       /* in samples */
    int var, mode, shape;       /* the stimulus: fibhip_stim_entry's fields */
    int r0, r1, c0, c1;
    float v, floor;
    int plane;
} fibhip_trig_rule;
int fibhip_trig_begin(fibhip_t h, int nsensors, const fibhip_trig_sensor *sensors, const unsigned char *masks /* [nmasks][H*W] or NULL */,
                      int nrules, const fibhip_trig_rule *rules, int nplanes, const float *planes /* [nplanes][H*W] or NULL */, int every,
                      long long capacity);
int fibhip_trig_count(fibhip_t h, long long *samples);
int fibhip_trig_read(fibhip_t h, long long first, long long count, int *dst /* [count][nrules][6] */);
int fibhip_trig_end(fibhip_t h);

/* Lesion program: the tissue's geometry changed during a run, on the device — ablating a rotor's core, drawing a line of block,
 * isolating a region — while every recorder and both stimulus programs stay attached.  The second event-driven program: its
 * hook writes the PHASE FIELD instead of the state.  The definition is exact (no tolerance anywhere; restated in NumPy in
 * tests/lesion_ref.py; the device equals that bit for bit).
 * A lesion is a float32 factor patch m on a box [r0, r1) x [c0, c1) of the grid.  Applying it is
 *     phi[r][c] = fmaxf(phi[r][c] * m[r - r0][c - c0], 1e-5f)       for the cells of the box
 * in plain float32 (one multiplication, one maximum, nothing contracted), followed by the six derived planes (dpy, dpx, 4 phi,
 * 1 / (4 phi), dpy / (4 phi), dpx / (4 phi)) recomputed, with fibhip_set_phase's arithmetic and reflection, on the box dilated
 * by one cell and cut at the grid.  This is add_hole_to_phase_field's update (ionic.py:83-105) restricted to the cells where its
 * mask is not exactly 1.0f; the identity needs phi >= 1e-5f everywhere beforehand, which attaching checks.
 * Event ticks.  With k = ticks since lesion_begin (the first tick after it is k = 0), entry e is applied right after tick e.tick:
 * where `for i in m.run(): if i == e.tick: ...` stands, and where the stimulus program puts a stimulus with first = e.tick.  A
 * run with a lesion after tick i EQUALS: run i + 1 ticks, read the state, create a handle whose phase field is the old one with
 * the same lesion applied on the host, set the state, run the remaining ticks.  Entries due after the same tick are applied IN
 * PROGRAM ORDER, each with its own floor (float32 products do not commute with the floor).
 * The state is not touched: cells inside a lesion go on with their own kinetics, uncoupled from the tissue, exactly as cells
 * inside a hole of the reference do.
 * Order on a tick.  The lesion comes LAST, behind every recorder's sample and every stimulus of that tick: the geometry it leaves
 * belongs to the next tick, and every sample of the event tick — the lead recorder's, whose source term reads the handle's phase
 * planes, included — sees the geometry the tick was computed with.  Planes a recorder was handed at attach (weights, masks) stay
 * what they were.  Courtemanche: a tick with a lesion due MAY be fused with the fibhip_step_slow behind it — 'slow' is pointwise
 * and never reads the geometry, so the bytes are the same.
 * Launches.  No launch spans an event tick; while events are still to come a launch goes out when the ticks up to the next one
 * are waiting, and nothing runs ahead of the caller while a program is attached.  The two kernels are queued on the handle's
 * stream behind the launch that ends at the event tick; nothing waits for them.  A multi-tick launch that gives up is recovered
 * as ever: a lesion queued behind it wrote nothing, an older one stands, and the replay applies the lost ones again, once.
 * A handle WITHOUT a phase field is given a field of ones first (through fibhip_set_phase): its kernels are the phase variants
 * from then on — the one visible effect of attaching to such a handle.
 * Refused: a row block (a handle with ghost rows), a handle with the zero-padded Laplacian (FIBHIP_ZEROPAD: no phase term), an
 * open tick, an empty box or one outside the grid, a factor that is not finite or not in [0, 1], tick < 0, reserved != 0, an offset outside the
 * patches, n or nfloats out of range (1 .. FIBHIP_MAX_LESION_ENTRIES entries, up to FIBHIP_MAX_STIM_PLANES * height * width
 * floats of patches), a second lesion_begin without a lesion_end, a phase field below 1e-5f somewhere.
 *   fibhip_lesion_begin  flushes, confirms and synchronises pending work, copies the patches and attaches
 *   fibhip_lesion_count  the number of entries applied so far (ticks accepted but not launched yet count: their events are
 *                        applied when they are)
 *   fibhip_lesion_end    flushes, synchronises, detaches and frees (no program attached: nothing); fibhip_destroy frees too
 *   fibhip_lesion_apply  ONE lesion now, at the state the caller has reached: flushes, confirms, uploads, the same two kernels,
 *                        synchronises.  With or without a program, beside every recorder: what a host-side closed loop uses
 *                        (read the tips, ablate there).  box = {r0, r1, c0, c1}, patch [r1 - r0][c1 - c0]
 *   fibhip_get_phase     the current phase field as [height][width]; refused on a handle that has none                          */
#define FIBHIP_MAX_LESION_ENTRIES 256
typedef struct fibhip_lesion_entry {
    long long offset;           /* where the entry's patch [r1 - r0][c1 - c0] starts in `patches`, in floats */
    int tick;
    int r0, r1, c0, c1;
    int reserved;               /* 0 */
} fibhip_lesion_entry;
int fibhip_lesion_begin(fibhip_t h, int n, const fibhip_lesion_entry *entries, long long nfloats, const float *patches /* [nfloats] */);
int fibhip_lesion_count(fibhip_t h, long long *applied);
int fibhip_lesion_end(fibhip_t h);
int fibhip_lesion_apply(fibhip_t h, const int *box /* [4] */, const float *patch);
int fibhip_get_phase(fibhip_t h, float *dst /* [height*width] */);

const char *fibhip_last_error(void);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FIBHIP_H */
