// rows_kernel.inc — temporal blocking with the potential in registers: the DPP lane helpers, rows_body, rows_kernel.
// (included by kernels.hpp)

// ---- wavefront-level neighbour access (gfx9 DPP wavefront shifts) -----------------------------------
// lane i reads the value lane i-1 / i+1 holds: the W / E taps of a row whose columns are the lanes of a
// wave.  The compiler folds the move into the consuming v_add/v_sub (`v_add_f32_dpp ... wave_shr:1`), so a
// horizontal tap costs no instruction of its own and no LDS access.  Lane 0 / lane 63 receive 0: they are
// the ring columns of the compute box, whose results are never used.
static FIB_DEV float lane_west(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, true));
}
static FIB_DEV float lane_east(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xF, 0xF, true));
}
static FIB_DEV float lane_get(float v, int lane)     // lane: wave-uniform
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// 9-point Laplacian (+ phase term) of the cell whose row neighbours N, S and own value C sit in THIS lane's
// registers and whose column neighbours sit in the adjacent lanes.  Same operations in the same order as
// stencil9 / phase_term: NW + SW is the neighbouring lane's own N + S (the same float32 addition of the same
// two numbers), so `lane_west(N + S)` is bit-identical to forming it here.
template <class P, bool PHASE>
static FIB_DEV float stencil9_lanes(float N, float S, float C, const PhaseCoef<P> &pc)
{
    const float ns = N + S;
    const float Wv = lane_west(C), E = lane_east(C);
    const float l1 = (ns + Wv) + E, d = (lane_west(ns) + lane_east(N)) + lane_east(S);
    float r;
    if constexpr (same_type<P, Fast>::value)                      // lap9<Fast>'s row-by-row form, the taps by lane shifts
        r = (__builtin_fmaf(0.5f, lane_west(N) + lane_east(N), N) + __builtin_fmaf(0.5f, lane_west(S) + lane_east(S), S)) +
            __builtin_fmaf(-6.0f, C, Wv + E);
    else
        r = (l1 + 0.5f * d) - 6.0f * C;
    if (PHASE) r = pc.add(r, N, S, Wv, E);
    return r;
}

// rows_kernel<M,P,MODE,K,TX,TY,R,PHASE> — temporal blocking with the potential in REGISTERS.
//   Work layout as strip_kernel (lane = column of a 64-wide box, wave = R consecutive rows, K sub-steps per
//   launch on a box that shrinks by one ring per sub-step), but the potential never lives in an LDS tile:
//     * a lane keeps the R values of its column strip in registers; the N/S taps of the strip's inner rows are
//       those registers, the W/E/diagonal taps are DPP wavefront shifts of them (lane_west / lane_east);
//     * only the strip's first and last row travel between waves: 2 ds_write + 2 ds_read per wave and sub-step
//       (strip_kernel: 3(R+2) reads + R writes) through a double-buffered [wave][top|bottom][lane] exchange
//       array, one s_barrier per sub-step;
//     * sub-step 0 takes its halo rows straight from global memory: no LDS fill, no barrier in the prologue.
//   Boundary rule (enforce_boundary + REFLECT): a tap at (r, c) reads the raw potential at
//   (clamp(r,1,H-2), clamp(c,1,W-2)).  Each lane therefore carries, next to the raw value of its cell (Fenton's
//   reaction reads it on border cells), the ENFORCED value `e` its neighbours see; after a sub-step border and
//   ghost rows/columns take the new value of the adjacent interior row/column — register copies inside a wave
//   (readlane across columns), the exchanged edge row between waves.  Only tiles that touch the domain edge
//   run that code (block-uniform branch; EDGE = false compiles it away).
template <class M, class P, int MODE, int K, int TX, int TY, int R, bool PHASE, bool EDGE>
static FIB_DEV void rows_body(const Geo &g, const PtrTab<M::NVAR> &pt, const PhaseTab &ph, const typename M::Consts &k, int sub0,
                              int tile, float (*ex)[64])
{
    constexpr int NV = M::NVAR;
    constexpr int CX = TX + 2 * (K - 1), CY = TY + 2 * (K - 1);
    constexpr int NW = (CY + R - 1) / R;
    constexpr unsigned WMASK = M::mask(MODE);
    auto &&kk = M::pinned(k);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int by = tile / g.tiles_x, bx = tile - by * g.tiles_x;
    int y0, rend;
    tile_rows(g, by, TY, y0, rend);
    const int x0 = bx * TX;
    const int cx0 = x0 - (K - 1), cy0 = y0 - (K - 1);
    const int gx = cx0 - 1 + lane;                                  // this lane's global column
    const int c0 = wave * R;                                        // first box row of this wave
    const int g0 = cy0 + c0 + g.row_off, glast = g0 + R - 1;        // global rows of the strip's first / last row
    const bool lane_in = lane >= 1 && lane <= CX && gx >= 0 && gx < g.W;
    const bool store_col = lane_in && gx >= x0 && gx < x0 + TX;
    const int ox = clampi(gx, 0, g.W - 1);
    const int bxx = clampi(gx, 1, g.W - 2);                         // column through the boundary clamp
    FIB_STAMP(0);

    // ---- prologue: every global load is issued before anything waits -------------------------------------
    float s[R][NV], e[R];
    PhaseCoef<P> pc[R];
    int off[R];
    auto brow = [&](int grow) {                                     // global row -> local row through the boundary clamp
        return clampi(clampi(grow, 1, g.Hg - 2) - g.row_off, 0, g.H - 1);
    };
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int gy = cy0 + c0 + r;
        const int oy = clampi(gy, 0, g.H - 1);
        off[r] = oy * g.pitch + ox;
#pragma unroll
        for (int v = 0; v < NV; ++v) s[r][v] = pt.in[v][off[r]];
        if (EDGE) e[r] = pt.in[0][(size_t)brow(g0 + r) * g.pitch + bxx];
        if (PHASE) pc[r].load(ph, oy * g.W + ox);                   // (the phase arrays are always planar)
    }
    float eN = pt.in[0][(size_t)brow(g0 - 1) * g.pitch + bxx];      // the rows above / below the strip
    float eS = pt.in[0][(size_t)brow(glast + 1) * g.pitch + bxx];
    if (!EDGE) {
#pragma unroll
        for (int r = 0; r < R; ++r) e[r] = s[r][0];
    }
    const bool top_open = cy0 + g.row_off > 0, bot_open = cy0 + CY + g.row_off < g.Hg;
    // lanes that hold column 1 / W-2 (sources of the border and ghost columns), block-uniform
    const int l_c1 = clampi(2 - cx0, 0, 63), l_cw = clampi(g.W - 1 - cx0, 0, 63);
    const bool edge_h = (cx0 <= 1) || (cx0 + CX >= g.W - 1);
    const bool west_copy = gx <= 0, east_copy = gx >= g.W - 1;
    FIB_STAMP(1);
#ifdef FIB_STAMPS
    __builtin_amdgcn_s_waitcnt(0x0F70);                             // diagnostic build: the load latency gets its own stamp
#endif
    FIB_STAMP(2);

#pragma unroll 1
    for (int st = 0; st < K; ++st) {
        const int need0 = top_open ? st : 0, need1 = bot_open ? CY - st : CY;
        int ra = max(0, need0 - c0), rb = min(R, need1 - c0);       // live rows of this strip (wave-uniform)
        ra = max(ra, -(cy0 + c0 + g.row_off));                      // global row >= 0
        rb = min(rb, min(g.Hg - g.row_off, g.H) - (cy0 + c0));      // global row < Hg, local row < H
        ra = max(ra, -(cy0 + c0));                                  // local row >= 0
        if (ra == 0 && rb == R) {
            float lp[R];
#pragma unroll
            for (int r = 0; r < R; ++r)
                lp[r] = stencil9_lanes<P, PHASE>(r == 0 ? eN : e[r - 1], r == R - 1 ? eS : e[r + 1], e[r], pc[r]);
            if constexpr (M::HAS_VEC) {
                M::template stepN<P, MODE, R>(s, e, lp, kk, sub0 + st);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) M::template step<P, MODE>(s[r], e[r], lp[r], kk, sub0 + st);
            }
        } else if (ra < rb) {
            // (all lanes stay active: the DPP taps of a live row need every lane's registers)
            float lp[R];
#pragma unroll
            for (int r = 0; r < R; ++r)
                lp[r] = stencil9_lanes<P, PHASE>(r == 0 ? eN : e[r - 1], r == R - 1 ? eS : e[r + 1], e[r], pc[r]);
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r >= ra && r < rb) M::template step<P, MODE>(s[r], e[r], lp[r], kk, sub0 + st);   // scalar branch
        }
        if (st + 1 < K) {
            // ---- the enforced values the next sub-step's taps read --------------------------------------
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (!EDGE || (r >= ra && r < rb)) e[r] = s[r][0];
            if (EDGE) {
                if (edge_h) {                                       // border + ghost columns <- column 1 / W-2
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float a = lane_get(e[r], l_c1), b = lane_get(e[r], l_cw);
                        e[r] = west_copy ? a : (east_copy ? b : e[r]);
                    }
                }
                // border + ghost rows whose source row lives in this strip
#pragma unroll
                for (int r = R - 2; r >= 0; --r)
                    if (g0 + r == 0 || g0 + r == -1) e[r] = e[r + 1];
#pragma unroll
                for (int r = 1; r < R; ++r)
                    if (g0 + r == g.Hg - 1 || g0 + r == g.Hg) e[r] = e[r - 1];
            }
            // ---- the strip's edge rows, for the waves above and below --------------------------------------
            float(*slot)[64] = ex + ((st & 1) * NW) * 2;
            slot[wave * 2 + 0][lane] = e[0];
            slot[wave * 2 + 1][lane] = e[R - 1];
            __syncthreads();
            eN = slot[max(wave - 1, 0) * 2 + 1][lane];
            eS = slot[min(wave + 1, NW - 1) * 2 + 0][lane];
            if (EDGE) {
                if (g0 == 1 || g0 == 0) eN = e[0];                  // the row above is border row 0 / ghost row -1
                if (glast == g.Hg - 2 || glast == g.Hg - 1) eS = e[R - 1];
                if (glast == 0) {                                   // my last row is border row 0: row 1 is the next strip's
                    e[R - 1] = eS;
                    if (R >= 2) e[R - 2] = eS;
                }
                if (g0 == g.Hg - 1) {
                    e[0] = eN;
                    if (R >= 2) e[1] = eN;
                }
            }
        }
        FIB_STAMP(3 + st);
    }

    // ---- write back -------------------------------------------------------------------------------------
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int gy = cy0 + c0 + r;
        if (store_col && gy >= y0 && gy < min(y0 + TY, rend) && gy < g.H) {
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if ((WMASK >> v) & 1u) pt.out[v][off[r]] = s[r][v];
        }
    }
    FIB_STAMP(14);
}

template <class M, class P, int MODE, int K, int TX, int TY, int R, bool PHASE>
__global__ void __launch_bounds__(64 * ((TY + 2 * (K - 1) + R - 1) / R))
rows_kernel(Geo g, PtrTab<M::NVAR> pt, PhaseTab ph, typename M::Consts k, int sub0)
{
    constexpr int CX = TX + 2 * (K - 1), CY = TY + 2 * (K - 1);
    static_assert(CX <= 62 && K > 1 && R >= 2, "rows_kernel: compute box must fit 62 lanes, strips of at least 2 rows");
    constexpr int NW = (CY + R - 1) / R;
    static_assert(NW <= 16, "rows_kernel: a workgroup has at most 16 waves");
    __shared__ float ex[2 * NW * 2][64];                            // [parity][wave][top|bottom][lane]

    const int tile = xcd_tile(blockIdx.x, g.ntiles);
    if (tile >= g.ntiles) return;
    const int by = tile / g.tiles_x, bx = tile - by * g.tiles_x;
    int y0, rend;
    tile_rows(g, by, TY, y0, rend);
    const int cx0 = bx * TX - (K - 1), cy0 = y0 - (K - 1) + g.row_off;
    // does the compute box (with its ring) reach the domain's border rows / columns?  block-uniform
    const bool edge = cx0 <= 1 || cx0 + CX >= g.W - 1 || cy0 <= 1 || cy0 + NW * R >= g.Hg - 1;
    if (edge)
        rows_body<M, P, MODE, K, TX, TY, R, PHASE, true>(g, pt, ph, k, sub0, tile, ex);
    else
        rows_body<M, P, MODE, K, TX, TY, R, PHASE, false>(g, pt, ph, k, sub0, tile, ex);
}
