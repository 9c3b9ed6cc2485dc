// tick_kernel.inc — the flat-tile fused stencil + reaction kernel.  (included by kernels.hpp)
//
// tick_kernel<M,P,MODE,K,TX,TY,NT,PHASE>
//   One workgroup advances one TX x TY tile of the grid by K sub-steps in a single launch
//   (temporal blocking).  K = 1 is the classic LDS-tiled fused step; K > 1 keeps the tile resident:
//   the potential lives in a double-buffered LDS tile with a halo, every other state variable and
//   the phase-field coefficients stay in registers of the thread that owns the cell, and HBM/L2 is
//   touched once per K steps.  The compute box is the tile grown by K-1 cells per side; its outer
//   ring goes stale by one cell per sub-step, so after K steps exactly the tile itself is still
//   exact — redundant rim compute instead of a grid-wide barrier per step (a launch boundary or a
//   grid barrier costs more than a whole 512x512 step).
//
//   Boundary conditions.  enforce_boundary (ionic.py:107-113) followed by the REFLECT pad of
//   laplace (ionic.py:49-50) means: every stencil tap at (r+dr, c+dc) reads the raw potential at
//   (clamp(r+dr,1,H-2), clamp(c+dc,1,W-2)).  The LDS tile is therefore filled through that clamp,
//   and after each sub-step the cells on domain row/col 1 and H-2/W-2 also refresh the border and
//   ghost copies next to them.  Border cells keep their own raw value in a register: Fenton's
//   reaction term reads it (fenton.py:101), nobody else does.
//
//   Cell -> thread map: the compute box is flattened row-major and dealt round-robin to the NT
//   threads, so consecutive lanes touch consecutive LDS words for all nine taps (conflict-free for
//   any tile shape) and every lane of every wave has work.
template <class M, class P, int MODE, int K, int TX, int TY, int NT, bool PHASE>
__global__ void __launch_bounds__(NT)
tick_kernel(Geo g, PtrTab<M::NVAR> pt, PhaseTab ph, typename M::Consts k, int sub0)
{
    constexpr int NV = M::NVAR;
    constexpr int CX = TX + 2 * (K - 1), CY = TY + 2 * (K - 1);   // compute box
    constexpr int LP = CX + 2, LQ = CY + 2;                        // LDS tile (box + ring)
    constexpr int NC = CX * CY, CPT = (NC + NT - 1) / NT, NL = LP * LQ;
    constexpr unsigned WMASK = M::mask(MODE);
    constexpr bool TENSOR = TensorOf<M>::value;                    // per-cell diffusion tensors (models.hpp Tensor<M>)
    constexpr bool PHI_TILE = PHASE && K == 1 && !TENSOR;          // (a tensor's first-order planes are prepared ones: never from a ϕ tile)
    constexpr bool ZP = ZeroPadOf<M>::value;
    __shared__ float lds[(K > 1) ? 2 : 1][NL];
    __shared__ float lphi[PHI_TILE ? NL : 1];

    const int tile = xcd_tile(blockIdx.x, g.ntiles);
    if (tile >= g.ntiles) return;                                  // whole workgroup, before any barrier
    auto &&kk = M::pinned(k);
    const int tid = threadIdx.x;
    const int by = tile / g.tiles_x, bx = tile - by * g.tiles_x;
    int y0, rend;
    tile_rows(g, by, TY, y0, rend);
    const int x0 = bx * TX;                                        // tile origin (local rows: y0)
    const int cx0 = x0 - (K - 1), cy0 = y0 - (K - 1);              // compute-box origin

    // ---- potential tile, through the boundary clamp -------------------------------------------
    const float *vin = pt.in[0];
    for (int i = tid; i < NL; i += NT) {
        const int ly = i / LP, lx = i - ly * LP;
        int yy = clampi(cy0 - 1 + ly + g.row_off, 1, g.Hg - 2) - g.row_off;
        yy = clampi(yy, 0, g.H - 1);                               // stay inside this slab
        const int xx = clampi(cx0 - 1 + lx, 1, g.W - 2);
        float v = vin[(size_t)yy * g.pitch + xx];
        if (ZP) {                                                  // outside the grid: 0 (conv2d padding='SAME')
            const int gyy = cy0 - 1 + ly + g.row_off, gxx = cx0 - 1 + lx;
            if (gyy < 0 || gyy > g.Hg - 1 || gxx < 0 || gxx > g.W - 1) v = 0.0f;
        }
        lds[0][i] = v;
        if (K > 1) lds[K > 1 ? 1 : 0][i] = v;
        if (PHI_TILE) {                                            // ϕ is REFLECT-padded, not clamped (ionic.py:75-76)
            int py = cy0 - 1 + ly + g.row_off, px = cx0 - 1 + lx;
            py = py < 0 ? -py : (py > g.Hg - 1 ? 2 * (g.Hg - 1) - py : py);
            px = px < 0 ? -px : (px > g.W - 1 ? 2 * (g.W - 1) - px : px);
            py = clampi(py - g.row_off, 0, g.H - 1);
            px = clampi(px, 0, g.W - 1);
            lphi[i] = ph.phi[(size_t)py * g.W + px];
        }
    }

    // ---- per-cell registers -------------------------------------------------------------------
    float s[CPT][NV];
    PhaseCoef<P> pc[CPT];
    TensorW tw[TENSOR ? CPT : 1];
    int li[CPT], off[CPT];
    unsigned fl[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int e = tid + j * NT;
        const bool valid = e < NC;
        const int ee = valid ? e : 0;
        const int cyy = ee / CX, cxx = ee - cyy * CX;
        li[j] = (cyy + 1) * LP + cxx + 1;
        const int gy = cy0 + cyy, gx = cx0 + cxx, gyg = gy + g.row_off;
        const bool indom = valid && gx >= 0 && gx < g.W && gyg >= 0 && gyg < g.Hg && gy >= 0 && gy < g.H;
        const int oy = clampi(gy, 0, g.H - 1), ox = clampi(gx, 0, g.W - 1);
        off[j] = oy * g.pitch + ox;
#pragma unroll
        for (int v = 0; v < NV; ++v) s[j][v] = pt.in[v][off[j]];
        if (PHASE && !PHI_TILE) pc[j].load(ph, oy * g.W + ox);    // (the phase arrays are always planar)
        if constexpr (TENSOR) {                                    // the cell's five weights, once per launch
            const int op = oy * g.W + ox;
            tw[j] = TensorW{k.wy[op], k.wx[op], k.wa[op], k.wb[op], k.wc[op]};
        }
        const bool border = gyg == 0 || gyg == g.Hg - 1 || gx == 0 || gx == g.W - 1;
        unsigned f = 0;
        if (indom) {
            f |= F_ACTIVE;
            if (!border) {
                f |= F_WLDS;
                constexpr bool ghost = !ZP;                        // the cells beyond the border stay 0 there
                if (gyg == 1) f |= F_TOP | (cyy >= 1 && ghost ? F_TOP2 : 0u);
                if (gyg == g.Hg - 2) f |= F_BOT | (cyy <= CY - 2 && ghost ? F_BOT2 : 0u);
                if (gx == 1) f |= F_LEFT | (cxx >= 1 && ghost ? F_LEFT2 : 0u);
                if (gx == g.W - 2) f |= F_RIGHT | (cxx <= CX - 2 && ghost ? F_RIGHT2 : 0u);
            }
            if (gy >= y0 && gy < min(y0 + TY, rend) && gx >= x0 && gx < x0 + TX) f |= F_STORE;
        }
        fl[j] = f;
    }
    __syncthreads();

    // ---- K fused sub-steps --------------------------------------------------------------------
#pragma unroll 1
    for (int st = 0; st < K; ++st) {
        const float *A = lds[(K > 1) ? (st & 1) : 0];
        float *B = lds[(K > 1) ? ((st & 1) ^ 1) : 0];
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            if (fl[j] & F_ACTIVE) {
                const int i = li[j];
                const float N = A[i - LP], S = A[i + LP], Wv = A[i - 1], E = A[i + 1];
                const float NW = A[i - LP - 1], SW = A[i + LP - 1], NE = A[i - LP + 1], SE = A[i + LP + 1];
                const float C = A[i];
                float l;
                if constexpr (TENSOR)
                    l = lap9_tensor<P>(N, S, Wv, E, NW, SW, NE, SE, C, tw[j].wy, tw[j].wx, tw[j].wa, tw[j].wb, tw[j].wc);
                else
                    l = ZP ? stencil9_conv(N, S, Wv, E, NW, SW, NE, SE, C) : lap9<P>(N, S, Wv, E, NW, SW, NE, SE, C);
                if (PHI_TILE) {     // same arithmetic as phase_prep_kernel + add_phase (IEEE division = Exact::divc)
                    const float dy = lphi[i + LP] - lphi[i - LP], dx = lphi[i + 1] - lphi[i - 1];
                    if constexpr (same_type<P, Fast>::value) {
                        const float q4 = 4.0f * lphi[i];
                        l = add_phase<P>(l, N, S, Wv, E, dy, dx, q4, 1.0f / q4);           // r4 exactly as phase_prep_kernel forms it
                    } else {
                        l = l + ((S - N) * dy + (E - Wv) * dx) / (4.0f * lphi[i]);
                    }
                } else if (PHASE) {
                    l = pc[j].add(l, N, S, Wv, E);                                         // ionic.py:58
                }
                M::template step<P, TwoPass<M>::first(MODE)>(s[j], C, l, kk, sub0 + st);
            }
        }
        if (K > 1 && st + 1 < K) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const unsigned f = fl[j];
                const int i = li[j];
                const float u = s[j][0];
                if (f & F_WLDS) B[i] = u;
                // refresh border + ghost copies (enforce_boundary + REFLECT), only in waves that own
                // such cells
                if (__builtin_amdgcn_ballot_w64((f & (F_EDGE_V | F_EDGE_H)) != 0)) {
                    if (f & F_TOP) B[i - LP] = u;
                    if (f & F_TOP2) B[i - 2 * LP] = u;
                    if (f & F_BOT) B[i + LP] = u;
                    if (f & F_BOT2) B[i + 2 * LP] = u;
                    if (f & F_LEFT) B[i - 1] = u;
                    if (f & F_LEFT2) B[i - 2] = u;
                    if (f & F_RIGHT) B[i + 1] = u;
                    if (f & F_RIGHT2) B[i + 2] = u;
                    if ((f & F_EDGE_V) && (f & F_EDGE_H)) {                // the four domain corners
                        const unsigned vf[4] = {F_TOP, F_TOP2, F_BOT, F_BOT2};
                        const int vo[4] = {-LP, -2 * LP, LP, 2 * LP};
                        const unsigned hf[4] = {F_LEFT, F_LEFT2, F_RIGHT, F_RIGHT2};
                        const int ho[4] = {-1, -2, 1, 2};
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int b = 0; b < 4; ++b)
                                if ((f & vf[a]) && (f & hf[b])) B[i + vo[a] + ho[b]] = u;
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- second evaluation on the post-update state (Courtemanche's 'slow' op, court.py:612-617) ----------
    // It sees the boundary-enforced NEW potential: a border cell reads its inward neighbour's new value, which
    // the host guarantees to be a cell of this same tile (fibhip.hip: lazy_fusable).
    if constexpr (TwoPass<M>::of(MODE)) {
        static_assert(K == 1, "two-pass modes are one sub-step per launch");
        __syncthreads();                                           // all taps of the old tile have been read
#pragma unroll
        for (int j = 0; j < CPT; ++j)
            if (fl[j] & F_ACTIVE) lds[0][li[j]] = s[j][0];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            if (fl[j] & F_ACTIVE) {
                const int cyy = li[j] / LP - 1, cxx = li[j] - (cyy + 1) * LP - 1;
                const int ty = clampi(cy0 + cyy + g.row_off, 1, g.Hg - 2) - g.row_off;
                const int tx = clampi(cx0 + cxx, 1, g.W - 2);
                const float Vc = lds[0][(ty - cy0 + 1) * LP + (tx - cx0 + 1)];
                M::template step<P, TwoPass<M>::second(MODE)>(s[j], Vc, 0.0f, kk, 0);
            }
        }
    }

    // ---- write back the tile ------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        if (fl[j] & F_STORE) {
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if ((WMASK >> v) & 1u) pt.out[v][off[j]] = s[j][v];
        }
    }
}
