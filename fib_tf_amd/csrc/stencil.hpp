// stencil.hpp — what every kernel family shares: the launch geometry and pointer tables the host fills in, the 9-point
// Laplacian and the phase-field term under the two arithmetic policies, and the tile -> XCD map.
// (included by kernels.hpp, inside namespace fib)

struct Geo {
    int H, W;        // rows / cols of this slab
    int pitch;       // floats between consecutive rows of ONE state array: W for the planar slab
                     // [nvar][H][W]; nvar*W for the row-interleaved slab [H][nvar][W] that row-block shards
                     // use (there the g halo rows of all arrays are one contiguous block = one message)
    int Hg;          // rows of the whole grid
    int row_off;     // global row of local row 0
    int r0, r1;      // local rows [r0, r1) this launch computes and stores ...
    int rb0, rb1;    // ... and, when ty_a < tile rows, a second band [rb0, rb1) served by the same launch
    int ty_a;        //     (the two edge strips of a row block); tile rows >= ty_a belong to the second band
    int tiles_x, ntiles;
};

// tile row `by` -> first local row of the tile and the end of the band it belongs to
static FIB_DEV void tile_rows(const Geo &g, int by, int TY, int &y0, int &rend)
{
    if (by < g.ty_a) {
        y0 = g.r0 + by * TY;
        rend = g.r1;
    } else {
        y0 = g.rb0 + (by - g.ty_a) * TY;
        rend = g.rb1;
    }
}

template <int NVAR>
struct PtrTab {
    const float *in[NVAR];
    float *out[NVAR];
};

struct PhaseTab {    // derived from ϕ once at set_phase (ionic.py:78-80)
    const float *dpy;   // ϕ[r+1,c] - ϕ[r-1,c]   (REFLECT-padded)
    const float *dpx;   // ϕ[r,c+1] - ϕ[r,c-1]
    const float *q4;    // 4 * ϕ[r,c]
    const float *r4;    // RN(1 / q4): lets the division by 4ϕ run as a 3-instruction exact form
    const float *pyr;   // RN(dpy * r4), RN(dpx * r4): all the fast policy needs of ϕ (its phase term is two FMAs on these
    const float *pxr;   //   products; formed per launch until round 3, now once at set_phase: 8 B per cell instead of 16)
    const float *phi;   // ϕ itself: one-sub-step launches stage a ϕ tile in LDS and difference it on the fly
                        // (4 B per cell of traffic instead of 16; the K-fused kernels read the prepared arrays
                        // once per K sub-steps and keep them in registers)
};

enum : unsigned {
    F_ACTIVE = 1u, F_WLDS = 2u, F_STORE = 4u,
    F_TOP = 8u, F_BOT = 16u, F_LEFT = 32u, F_RIGHT = 64u,
    F_TOP2 = 128u, F_BOT2 = 256u, F_LEFT2 = 512u, F_RIGHT2 = 1024u,
    F_EDGE_V = F_TOP | F_BOT, F_EDGE_H = F_LEFT | F_RIGHT
};

static FIB_DEV int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// 9-point Laplacian in the reference's evaluation order, ionic.py:51-53
static FIB_DEV float stencil9(float N, float S, float Wv, float E, float NW, float SW, float NE, float SE, float C)
{
    const float l = (((N + S) + Wv) + E) + 0.5f * (((NW + SW) + NE) + SE);
    return l - 6.0f * C;
}
// The 3x3 convolution of fenton_simple.py:38-49 ([[.5,1,.5],[1,-6,1],[.5,1,.5]], padding SAME).  TensorFlow does
// not specify its accumulation order; this is the kernel's row-major order, as in tests/golden/_standin.
static FIB_DEV float stencil9_conv(float N, float S, float Wv, float E, float NW, float SW, float NE, float SE, float C)
{
    float a = 0.5f * NW;
    a = a + N;
    a = a + 0.5f * NE;
    a = a + Wv;
    a = a + (-6.0f * C);
    a = a + E;
    a = a + 0.5f * SW;
    a = a + S;
    return a + 0.5f * SE;
}
// phase-field correction, ionic.py:78-80, from the pre-differenced ϕ terms
// (the division is always the correctly rounded form: the Laplacian incl. its phase term is pure
// arithmetic and stays bit-identical to the reference under both arithmetic policies)
template <class P>
static FIB_DEV float phase_term(float N, float S, float Wv, float E, float dpy, float dpx, float q4, float r4)
{
    return Exact::divc((S - N) * dpy + (E - Wv) * dpx, q4, r4);
}

// The Laplacian of the FUSED kernels under the two arithmetic policies.  Exact: the reference's operations, one
// rounding each (stencil9 / phase_term).  Fast: re-associated row by row with the scalings (0.5*, -6*) and the phase
// quotient contracted into FMAs; every fused kernel uses these two functions, so fusion depth and tile shape still
// never change a bit of the result within a policy.  (The stand-alone array ops
// IonicModel.laplace / phase_field keep the exact form under both policies.)
template <class P>
static FIB_DEV float lap9(float N, float S, float Wv, float E, float NW, float SW, float NE, float SE, float C)
{
    if constexpr (same_type<P, Fast>::value) {
        // row by row: a(row) = centre + 0.5 (west + east) for the rows above and below, b = (west + east) - 6 centre for
        // the cell's own row.  The R cells of a lane share these row terms (a of the row below cell r is a of the row
        // above cell r+2, west + east of a row serves both forms): 19 operations for three cells instead of 24.
        const float an = __builtin_fmaf(0.5f, NW + NE, N), as = __builtin_fmaf(0.5f, SW + SE, S);
        return (an + as) + __builtin_fmaf(-6.0f, C, Wv + E);
    } else {
        return stencil9(N, S, Wv, E, NW, SW, NE, SE, C);
    }
}
template <class P>
static FIB_DEV float add_phase(float lap, float N, float S, float Wv, float E, float dpy, float dpx, float q4, float r4)
{
    if constexpr (same_type<P, Fast>::value)   // (dpx*r4 and dpy*r4 do not change during a launch: formed once, before the step loop)
        return __builtin_fmaf(E - Wv, dpx * r4, __builtin_fmaf(S - N, dpy * r4, lap));
    else
        return lap + phase_term<P>(N, S, Wv, E, dpy, dpx, q4, r4);
}

// What a thread of a K-fused kernel keeps of ϕ per cell, by arithmetic policy.  Exact: the four prepared arrays (the
// quotient by 4ϕ is the correctly rounded one).  Fast: the two products dpy*r4, dpx*r4 — prepared by phase_prep_kernel
// with the same single rounding the kernels used to apply per launch, so results are bit-identical to the four-array form.
template <class P>
struct PhaseCoef {
    float dpy, dpx, q4, r4;
    FIB_DEV void load(const PhaseTab &ph, int op)
    {
        dpy = ph.dpy[op];
        dpx = ph.dpx[op];
        q4 = ph.q4[op];
        r4 = ph.r4[op];
    }
    FIB_DEV float add(float lap, float N, float S, float Wv, float E) const
    {
        return add_phase<P>(lap, N, S, Wv, E, dpy, dpx, q4, r4);
    }
};
template <>
struct PhaseCoef<Fast> {
    float ay, ax;
    FIB_DEV void load(const PhaseTab &ph, int op)
    {
        ay = ph.pyr[op];
        ax = ph.pxr[op];
    }
    FIB_DEV float add(float lap, float N, float S, float Wv, float E) const
    {
        return __builtin_fmaf(E - Wv, ax, __builtin_fmaf(S - N, ay, lap));
    }
};

// blocks b and b+8 share an XCD (round-robin dispatch): give each XCD one contiguous run of tiles so
// that the halos neighbouring tiles share are served by the same L2.  Speed only, never correctness.
static FIB_DEV int xcd_tile(int b, int ntiles)
{
    const int per = (ntiles + 7) >> 3;
    return (b & 7) * per + (b >> 3);
}

// FIBHIP_ZEROPAD — the Laplacian of fenton_simple.py: taps outside the grid read 0 and the nine products are
// accumulated in the kernel's row-major order.  A compile-time property of the model type (FentonZP), so that the
// other models' kernels carry none of it; tick_kernel only.
template <class M, class = void>
struct ZeroPadOf {
    static constexpr bool value = false;
};
template <class M>
struct ZeroPadOf<M, void_of<decltype(M::ZEROPAD)>> {
    static constexpr bool value = M::ZEROPAD;
};

// fibhip_set_tensor — per-cell diffusion tensors D = [[dyy, dxy], [dxy, dxx]] (rows y, columns x; relative to diff).  A
// compile-time property of the model type (models.hpp Tensor<M>), tick_kernel only, as ZEROPAD is.
template <class M, class = void>
struct TensorOf {
    static constexpr bool value = false;
};
template <class M>
struct TensorOf<M, void_of<decltype(M::TENSOR)>> {
    static constexpr bool value = M::TENSOR;
};

// The five weights of one cell, as tensor_prep_kernel forms them (one rounding per line, no contraction):
//     wd = 0.25 (dyy + dxx)      wy = 1.5 dyy - 0.5 dxx  (N, S)      wx = 1.5 dxx - 0.5 dyy  (W, E)
//     wa = wd + dxy  (NW, SE)    wb = wd - dxy  (NE, SW)              wc = 12 wd  (centre)
// 2 h^2 D : grad grad V, second-order, with the 9-point blend that gives stencil9's weights (1, 1, 0.5, 0.5, 6) at D = I.
struct TensorW {
    float wy, wx, wa, wb, wc;
};
static FIB_DEV TensorW tensor_weights(float dyy, float dxx, float dxy)
{
    TensorW w;
    const float wd = 0.25f * (dyy + dxx);
    w.wy = 1.5f * dyy - 0.5f * dxx;
    w.wx = 1.5f * dxx - 0.5f * dyy;
    w.wa = wd + dxy;
    w.wb = wd - dxy;
    w.wc = 12.0f * wd;
    return w;
}
// The second-order part under the two arithmetic policies.  Exact: every product and sum rounded once, in stencil9's order — at
// D = I every product is exact and the value is stencil9's.  Fast: opposite taps share a weight, so they are summed first and
// the five products contracted into FMAs:
//     t = fma(wx, W + E, wy * (N + S))     u = fma(wb, SW + NE, wa * (NW + SE))     l = fma(-wc, C, t + u)
// Rounded operations on the longest path: the pair sum (1), the product (2), the FMA (3), t + u (4), the last FMA (5); a weight
// brings up to 3 of its own (wa: the sum, the scaling by 0.25, the sum with dxy): 8 for the second-order part alone.  With the
// first-order term (PhaseCoef<Fast>::add: two more FMAs behind l) the Laplacian's terms see 10; so do the first-order ones:
// gy or gx 5 (tensor_prep_cell), r4 1, their product 1, the tap difference 1 beside them, the two FMAs 2.  n = 10.
template <class P>
static FIB_DEV float lap9_tensor(float N, float S, float Wv, float E, float NW, float SW, float NE, float SE, float C, float wy, float wx,
                                 float wa, float wb, float wc)
{
    if constexpr (same_type<P, Fast>::value) {
        const float t = __builtin_fmaf(wx, Wv + E, wy * (N + S));
        const float u = __builtin_fmaf(wb, SW + NE, wa * (NW + SE));
        return __builtin_fmaf(-wc, C, t + u);
    } else {
        const float l = ((((wy * N + wy * S) + wx * Wv) + wx * E) + (((wa * NW + wb * SW) + wb * NE) + wa * SE));
        return l - wc * C;
    }
}

// does MODE ask for two evaluations in one launch (Courtemanche::MODE_FASTSLOW)?
template <class M, class = void>
struct TwoPass {
    static constexpr bool of(int) { return false; }
    static constexpr int first(int mode) { return mode; }
    static constexpr int second(int mode) { return mode; }
};
template <class M>
struct TwoPass<M, void_of<decltype(M::MODE_FASTSLOW)>> {
    static constexpr bool of(int mode) { return mode == M::MODE_FASTSLOW; }
    static constexpr int first(int mode) { return mode == M::MODE_FASTSLOW ? M::MODE_FAST : mode; }
    static constexpr int second(int mode) { return mode == M::MODE_FASTSLOW ? M::MODE_SLOW : mode; }
};

// 16-byte vectors: the multi-tick exchange cells, the recorders' and the copy kernel's loads and stores
typedef unsigned fib_v4u __attribute__((ext_vector_type(4)));
typedef float fib_v4f __attribute__((ext_vector_type(4)));
