// pointwise.inc — the kernels without a tile: pointwise re-evaluation, the stand-alone array ops, phase preparation, pacing
// and Courtemanche's voltage-only intermediates.  (included by kernels.hpp)

// Pointwise re-evaluation without the stencil: Courtemanche's 'slow' op (court.py:103,615-617).
// Vc is the boundary-enforced potential of the cell, read straight through the clamp.
template <class M, class P, int MODE>
__global__ void __launch_bounds__(256)
pointwise_kernel(Geo g, PtrTab<M::NVAR> pt, typename M::Consts k)
{
    constexpr int NV = M::NVAR;
    constexpr unsigned WMASK = M::mask(MODE);
    const int n = (g.r1 - g.r0) * g.W;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int gy = g.r0 + e / g.W, gx = e % g.W;
        int yy = clampi(gy + g.row_off, 1, g.Hg - 2) - g.row_off;
        yy = clampi(yy, 0, g.H - 1);
        const int xx = clampi(gx, 1, g.W - 2);
        const float Vc = pt.in[0][(size_t)yy * g.pitch + xx];
        const int o = gy * g.pitch + gx;
        float s[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) s[v] = pt.in[v][o];
        M::template step<P, MODE>(s, Vc, 0.0f, k, 0);
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if ((WMASK >> v) & 1u) pt.out[v][o] = s[v];
    }
}

// The building blocks of IonicModel as stand-alone array ops (IonicModel.enforce_boundary / laplace /
// phase_field / rush_larsen are public methods of the reference, ionic.py:44-123).  Same device
// functions as the fused kernel; used for unit-level parity tests.
enum { OP_BOUNDARY = 0, OP_LAPLACE = 1, OP_PHASE = 2, OP_RUSH_LARSEN = 3 };
template <class P>
__global__ void unit_op_kernel(int op, int H, int W, const float *a, const float *b, const float *c,
                               const float *ph3, float mdt, float *out)
{
    const int n = H * W;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int y = e / W, x = e % W;
        if (op == OP_BOUNDARY) {
            out[e] = a[clampi(y, 1, H - 2) * W + clampi(x, 1, W - 2)];
        } else if (op == OP_RUSH_LARSEN) {
            out[e] = rush_larsen<P>(a[e], b[e], c[e], mdt);
        } else {   // REFLECT pad: ghost index -1 -> 1, H -> H-2
            const int yn = y == 0 ? 1 : y - 1, ys = y == H - 1 ? H - 2 : y + 1;
            const int xw = x == 0 ? 1 : x - 1, xe = x == W - 1 ? W - 2 : x + 1;
            const float N = a[yn * W + x], S = a[ys * W + x], Wv = a[y * W + xw], E = a[y * W + xe];
            float r = 0.0f;
            if (op == OP_LAPLACE)
                r = stencil9(N, S, Wv, E, a[yn * W + xw], a[ys * W + xw], a[yn * W + xe], a[ys * W + xe], a[e]);
            if (ph3) {
                const float f = phase_term<P>(N, S, Wv, E, ph3[e], ph3[n + e], ph3[2 * n + e], ph3[3 * n + e]);
                r = (op == OP_LAPLACE) ? r + f : f;
            }
            out[e] = r;
        }
    }
}

// ϕ -> (dpy, dpx, q4, r4) and the fast policy's two products, REFLECT-padded in GLOBAL coordinates (ionic.py:75-80)
// (one cell of it: lesion_prep_kernel, record_kernels.inc, recomputes the cells around a lesion with the same expression)
static FIB_DEV void phase_prep_cell(const Geo &g, int y, int x, const float *phi, float *dpy, float *dpx, float *q4, float *r4, float *pyr,
                                    float *pxr)
{
    const int e = y * g.W + x, yg = y + g.row_off;
    int yn = yg - 1, ys = yg + 1, xw = x - 1, xe = x + 1;
    if (yn < 0) yn = 1;
    if (ys > g.Hg - 1) ys = g.Hg - 2;
    if (xw < 0) xw = 1;
    if (xe > g.W - 1) xe = g.W - 2;
    yn = clampi(yn - g.row_off, 0, g.H - 1);
    ys = clampi(ys - g.row_off, 0, g.H - 1);
    dpy[e] = phi[ys * g.W + x] - phi[yn * g.W + x];
    dpx[e] = phi[y * g.W + xe] - phi[y * g.W + xw];
    q4[e] = 4.0f * phi[e];
    r4[e] = 1.0f / q4[e];                           // IEEE division: correctly rounded reciprocal
    if (pyr) {                                      // one rounding each (-ffp-contract=off), as add_phase<Fast> forms them
        pyr[e] = dpy[e] * r4[e];
        pxr[e] = dpx[e] * r4[e];
    }
}
__global__ void phase_prep_kernel(Geo g, const float *phi, float *dpy, float *dpx, float *q4, float *r4, float *pyr, float *pxr)
{
    const int n = g.H * g.W;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x)
        phase_prep_cell(g, e / g.W, e % g.W, phi, dpy, dpx, q4, r4, pyr, pxr);
}

// A tensor handle's prepared planes (fibhip_set_tensor): the five weights of lap9_tensor, and PhaseTab's six planes with the
// first-order coefficients in the place of dpy, dpx —
//     gy = (dyy dpy + dxy dpx) + (2ϕ) (δy dyy + δx dxy)        gx = (dxy dpy + dxx dpx) + (2ϕ) (δy dxy + δx dxx)
// δ: phase_prep_cell's REFLECT-padded central difference without the 1/2; q4, r4 and the two products as there, so that
// PhaseCoef<P>::add runs unchanged.  The ϕ part keeps the reference's weight (ionic.py:78-80: half of what a consistent
// discretisation of D grad ϕ . grad V / ϕ would carry), the div D part the consistent one.  At D = I: gy == dpy, gx == dpx.
// `phi` null: ϕ = 1 everywhere.  One rounding per operation (-ffp-contract=off).
struct TensorPlanes {
    const float *dyy, *dxx, *dxy;
    float *wy, *wx, *wa, *wb, *wc;
};
static FIB_DEV void tensor_prep_cell(const Geo &g, int y, int x, const float *phi, const TensorPlanes &t, float *gy, float *gx, float *q4,
                                     float *r4, float *pyr, float *pxr)
{
    const int e = y * g.W + x, yg = y + g.row_off;
    int yn = yg - 1, ys = yg + 1, xw = x - 1, xe = x + 1;
    if (yn < 0) yn = 1;
    if (ys > g.Hg - 1) ys = g.Hg - 2;
    if (xw < 0) xw = 1;
    if (xe > g.W - 1) xe = g.W - 2;
    yn = clampi(yn - g.row_off, 0, g.H - 1);
    ys = clampi(ys - g.row_off, 0, g.H - 1);
    const int n = yn * g.W + x, s = ys * g.W + x, w = y * g.W + xw, ea = y * g.W + xe;
    const float dyy = t.dyy[e], dxx = t.dxx[e], dxy = t.dxy[e];
    const TensorW tw = tensor_weights(dyy, dxx, dxy);
    t.wy[e] = tw.wy;
    t.wx[e] = tw.wx;
    t.wa[e] = tw.wa;
    t.wb[e] = tw.wb;
    t.wc[e] = tw.wc;
    const float p = phi ? phi[e] : 1.0f;
    const float dpy = phi ? phi[s] - phi[n] : 0.0f, dpx = phi ? phi[ea] - phi[w] : 0.0f;
    const float p2 = 2.0f * p;
    const float vy = (dyy * dpy + dxy * dpx) + p2 * ((t.dyy[s] - t.dyy[n]) + (t.dxy[ea] - t.dxy[w]));
    const float vx = (dxy * dpy + dxx * dpx) + p2 * ((t.dxy[s] - t.dxy[n]) + (t.dxx[ea] - t.dxx[w]));
    gy[e] = vy;
    gx[e] = vx;
    const float q = 4.0f * p;
    q4[e] = q;
    const float r = 1.0f / q;                       // IEEE division: correctly rounded reciprocal
    r4[e] = r;
    if (pyr) {
        pyr[e] = vy * r;
        pxr[e] = vx * r;
    }
}
__global__ void tensor_prep_kernel(Geo g, const float *phi, TensorPlanes t, float *gy, float *gx, float *q4, float *r4, float *pyr, float *pxr)
{
    const int n = g.H * g.W;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x)
        tensor_prep_cell(g, e / g.W, e % g.W, phi, t, gy, gx, q4, r4, pyr, pxr);
}

// The tensor operator as a stand-alone array op (fibhip_unit_laplace_tensor): lap9_tensor and PhaseCoef<P>::add on the planes
// tensor_prep_kernel made — the device functions of tick_kernel's tensor variants; `a` is read through the REFLECT pad, as
// unit_op_kernel's laplace reads it.
template <class P>
__global__ void unit_tensor_kernel(int H, int W, const float *a, TensorPlanes t, PhaseTab ph, float *out)
{
    const int n = H * W;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int y = e / W, x = e % W;
        const int yn = y == 0 ? 1 : y - 1, ys = y == H - 1 ? H - 2 : y + 1;
        const int xw = x == 0 ? 1 : x - 1, xe = x == W - 1 ? W - 2 : x + 1;
        const float N = a[yn * W + x], S = a[ys * W + x], Wv = a[y * W + xw], E = a[y * W + xe];
        const float l = lap9_tensor<P>(N, S, Wv, E, a[yn * W + xw], a[ys * W + xw], a[yn * W + xe], a[ys * W + xe], a[e], t.wy[e], t.wx[e],
                                       t.wa[e], t.wb[e], t.wc[e]);
        PhaseCoef<P> pc;
        pc.load(ph, e);
        out[e] = pc.add(l, N, S, Wv, E);
    }
}

// pace op, ionic.py:144-163:  pot = max(pot, s), s = v inside the global rectangle, min_v outside
__global__ void pace_kernel(Geo g, float *pot, int r0, int r1, int c0, int c1, float v, float min_v)
{
    const int n = g.H * g.W;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int y = e / g.W, yg = y + g.row_off, x = e % g.W;
        const float sv = (yg >= r0 && yg < r1 && x >= c0 && x < c1) ? v : min_v;
        const size_t o = (size_t)y * g.pitch + x;
        pot[o] = fmaxf(pot[o], sv);
    }
}

// calc_inter(V, mod) as a stand-alone op (court.py:273-429, court_ultra.py:445-450): the 32 voltage-only
// intermediates of n voltages, row k of `out` = k-th key in the reference dict's insertion order.
constexpr int COURT_NINTER = 32;
template <class P>
__global__ void court_inter_kernel(int n, const float *__restrict__ V, float *__restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        CourtemancheUS::Inter q;
        CourtemancheUS::calc_inter<P>(V[i], q);
        const float v[COURT_NINTER] = {q.d_inf, q.tau_d, q.f_inf, q.tau_f, q.tau_w, q.w_inf, q.m_inf, q.tau_m,
                                       q.h_inf, q.tau_h, q.j_inf, q.tau_j, q.tau_oa, q.oa_inf, q.tau_oi, q.oi_inf,
                                       q.tau_ua, q.ua_inf, q.tau_ui, q.ui_inf, q.tau_xr, q.xr_inf, q.tau_xs, q.xs_inf,
                                       q.g_Kur, q.f_NaK, q.i_NaCaa, q.i_NaCab, q.i_K1a, q.i_Kra, q.us_inf, q.tau_us};
#pragma unroll
        for (int k = 0; k < COURT_NINTER; ++k) out[(size_t)k * n + i] = v[k];
    }
}
