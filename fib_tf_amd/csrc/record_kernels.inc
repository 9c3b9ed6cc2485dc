// record_kernels.inc — the streaming kernels behind a committed tick: the activation, electrode, tip, frame, statistics, spectrum, beat, lead, potential-map and wave recorders, and the
// plain copy whose shape they take (the bandwidth yardstick).  (included by kernels.hpp; the host side is record.inc)

// ---- activation recorder (fibhip_observe_begin): per-cell event maps, updated after every observed tick ----------------
// Vp = the watched array at the end of the previous observed tick (the recorder's own plane), Vc = the array now.
//   upstroke   Vp < up && Vc >= up:               t = t0 + ((up - Vp) / (Vc - Vp)) * tick;  prev = last; last = t;
//                                                  first = t if count == 0;  count += 1
//   downstroke Vp >= down && Vc < down, count > 0: t = t0 + ((Vp - down) / (Vp - Vc)) * tick; apd = t - last
// float32, every operation rounded on its own (-ffp-contract=off, IEEE division); NaN compares false: no event.  With
// down <= up the two cases exclude each other.  The maps are touched only where an event happens, so the steady traffic
// is Vc read, Vp read and Vp written: 12 bytes per cell.
struct ObsMaps {
    float *first, *last, *prev, *apd;
    int *count;
};

static FIB_DEV void observe_cell(float vp, float vc, size_t i, const ObsMaps &m, float up, float down, float t0, float tick)
{
    if (vp < up && vc >= up) {
        const float t = t0 + ((up - vp) / (vc - vp)) * tick;
        const int n = m.count[i];
        m.prev[i] = m.last[i];
        m.last[i] = t;
        if (n == 0) m.first[i] = t;
        m.count[i] = n + 1;
    } else if (vp >= down && vc < down && m.count[i] > 0) {
        const float t = t0 + ((vp - down) / (vp - vc)) * tick;
        m.apd[i] = t - m.last[i];
    }
}

// One element per thread and as many workgroups as that takes (the shape of copy_kernel below, the fastest streaming
// shape measured; 512x512 = 256 workgroups, one per CU).  VEC: the watched array is contiguous (planar slab, pitch == W)
// and 16-byte aligned — thread i < n/4 takes cells 4i .. 4i+3 with 16-byte loads and stores, the n % 4 threads after them
// one cell each.  Otherwise (row-interleaved slab, or an unaligned array): one cell per thread, scalar.
template <bool VEC>
__global__ void __launch_bounds__(256) observe_kernel(Geo g, const float *__restrict__ pot, float *__restrict__ vprev, ObsMaps m,
                                                      float up, float down, float t0, float tick)
{
    const size_t n = (size_t)g.H * g.W;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const size_t n4 = n / 4;
        if (i < n4) {
            const fib_v4f vc = reinterpret_cast<const fib_v4f *>(pot)[i];
            const fib_v4f vp = reinterpret_cast<const fib_v4f *>(vprev)[i];
            reinterpret_cast<fib_v4f *>(vprev)[i] = vc;
#pragma unroll
            for (int j = 0; j < 4; ++j) observe_cell(vp[j], vc[j], 4 * i + j, m, up, down, t0, tick);
        } else if (i < n4 + n % 4) {
            const size_t e = 4 * n4 + (i - n4);
            const float vc = pot[e], vp = vprev[e];
            vprev[e] = vc;
            observe_cell(vp, vc, e, m, up, down, t0, tick);
        }
    } else if (i < n) {
        const size_t y = i / (size_t)g.W, x = i % (size_t)g.W;
        const float vc = pot[y * (size_t)g.pitch + x], vp = vprev[i];
        vprev[i] = vc;
        observe_cell(vp, vc, i, m, up, down, t0, tick);
    }
}

// ---- electrode recorder (fibhip_electrode_begin): weighted sums of one state array over small patches ------------------
// One workgroup of EL_THREADS threads per CHUNK of a patch (the host cuts patches at attach: one chunk up to EL_CHUNK cells,
// larger patches into at most 256 equal chunks).  Thread t takes the chunk's cells t, t + EL_THREADS, ... in that order
// into ONE float32 accumulator (product rounded, then added: -ffp-contract=off), EL_BATCH cells' loads in flight at a
// time: the kernel is latency-bound (the reference's two Gaussian electrodes are 2 x 10 201 cells), so what counts is the
// number of dependent memory round trips — two at that size.  Then 6 levels of __shfl_down inside each wave, the 16 wave
// sums through LDS, 4 more levels by wave 0, one plain store: no term passes through more than ceil(cells / 1024) + 10
// additions, in an order fixed by the chunk table alone.  An electrode of one chunk stores straight into its trace slot;
// an electrode of several stores one partial per chunk, which electrode_combine_kernel (a second launch on the same
// stream, only enqueued when such an electrode exists) adds in a fixed 8-level tree: together within the
// ceil(m / 256) + 16 of include/fibhip.h.  No floating-point atomics anywhere.
#define EL_THREADS 1024
#define EL_BATCH 8
#define EL_CHUNK 16384
struct ElChunk {
    int r0, c0, pw;         // the patch's first row and column in the grid, and its width
    unsigned first, count;  // this chunk's cells [first, first + count) of the patch, row-major
    unsigned woff;          // float offset of the patch in the weights
    int out;                // >= 0: electrode index (store into the sample's row); < 0: partial slot -1 - out
};
struct ElComb {
    int e, part0, nparts;   // electrode, its first partial slot, its chunks (<= 256)
};

static FIB_DEV float el_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(EL_THREADS) electrode_kernel(const float *__restrict__ x, int pitch, const ElChunk *__restrict__ chunks,
                                                               const float *__restrict__ weights, float *__restrict__ row,
                                                               float *__restrict__ part)
{
    __shared__ float wsum[EL_THREADS / 64];
    const ElChunk c = chunks[blockIdx.x];
    const float *__restrict__ w = weights + c.woff;
    const unsigned end = c.first + c.count;
    float acc = 0.f;
    for (unsigned p0 = c.first + threadIdx.x; p0 < end; p0 += EL_BATCH * EL_THREADS) {
        float xv[EL_BATCH], wv[EL_BATCH];
#pragma unroll
        for (int j = 0; j < EL_BATCH; ++j) {
            const unsigned p = p0 + (unsigned)j * EL_THREADS;
            const bool in = p < end;
            const unsigned q = in ? p : c.first;                       // (an in-range address; the term is dropped below)
            const unsigned r = q / (unsigned)c.pw, col = q - r * (unsigned)c.pw;
            xv[j] = x[(size_t)(c.r0 + (int)r) * (size_t)pitch + (size_t)(c.c0 + (int)col)];
            wv[j] = w[q];
        }
#pragma unroll
        for (int j = 0; j < EL_BATCH; ++j)
            if (p0 + (unsigned)j * EL_THREADS < end) acc += wv[j] * xv[j];
    }
    acc = el_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        float v = threadIdx.x < EL_THREADS / 64 ? wsum[threadIdx.x] : 0.f;
#pragma unroll
        for (int off = EL_THREADS / 128; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (threadIdx.x == 0) {
            if (c.out >= 0) row[c.out] = v;
            else part[-1 - c.out] = v;
        }
    }
}

// one 256-thread workgroup per electrode of several chunks: its partials, one per thread, through the same tree
__global__ void __launch_bounds__(256) electrode_combine_kernel(const ElComb *__restrict__ combs, const float *__restrict__ part,
                                                                float *__restrict__ row)
{
    __shared__ float wsum[4];
    const ElComb c = combs[blockIdx.x];
    float v = (int)threadIdx.x < c.nparts ? part[c.part0 + threadIdx.x] : 0.f;
    v = el_wave_sum(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) row[c.e] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ---- tip recorder (fibhip_tips_begin): the phase singularities of (A - a0, B - b0), compacted ---------------------------
// A plaquette (i, j) has the corners (i,j) -> (i,j+1) -> (i+1,j+1) -> (i+1,j) -> (i,j); a = A - a0 and b = B - b0 are float32
// subtractions.  An edge (a1,b1) -> (a2,b2) crosses the positive a half-axis upwards when b1 < 0 <= b2 and
// cross = a1 b2 - a2 b1 > 0, downwards when b2 < 0 <= b1 and cross < 0.  Both products of two float32 numbers are exact in
// double (48 bits), so the rounded difference has the exact sign, fused or not.  NaN compares false: no crossing.  The charge
// of the plaquette is the number of upward minus the number of downward crossings, in {-1, 0, +1}.
static FIB_DEV int tip_edge(float a1, float b1, float a2, float b2)
{
    const double cross = (double)a1 * (double)b2 - (double)a2 * (double)b1;
    int w = 0;
    if (b1 < 0.f && b2 >= 0.f && cross > 0.0) w = 1;
    if (b2 < 0.f && b1 >= 0.f && cross < 0.0) w = -1;
    return w;
}
// corners in the order above: 0 = (i,j), 1 = (i,j+1), 2 = (i+1,j+1), 3 = (i+1,j)
static FIB_DEV int tip_charge(const float a[4], const float b[4])
{
    return tip_edge(a[0], b[0], a[1], b[1]) + tip_edge(a[1], b[1], a[2], b[2]) + tip_edge(a[2], b[2], a[3], b[3]) +
           tip_edge(a[3], b[3], a[0], b[0]);
}

// One sample's output: cnt = {n_pos, n_neg, stored} (zeroed by the host in front of the launch), rec = [max_tips] records of
// {row, col, charge, 0}.  Tips are rare, so each WAVE compacts its hits: a ballot per plaquette slot, one integer atomicAdd of
// the wave's hit count on `stored` by lane 0 (which returns the wave's base), and every hit lane stores its record at
// base + its rank among the wave's hits while that is below max_tips.  n_pos and n_neg are added the same way, one atomic per
// wave that has such hits, and so stay exact when the list is cut.  The order of the records is the order of arrival.
// NP plaquettes per thread (w[p] = 0: none there).  Every lane of the wave must come here (no early return in front).
template <int NP>
static FIB_DEV void tip_emit(const int (&w)[NP], int row, const int (&col)[NP], int *__restrict__ cnt, int4 *__restrict__ rec, int max_tips)
{
    unsigned long long hit[NP];
    int total = 0, pos = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        hit[p] = __ballot(w[p] != 0);
        total += __popcll(hit[p]);
        pos += __popcll(__ballot(w[p] > 0));
    }
    if (total == 0) return;                                   // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    int base = 0;
    if (lane == 0) {
        base = atomicAdd(&cnt[2], total);
        if (pos) atomicAdd(&cnt[0], pos);
        if (total - pos) atomicAdd(&cnt[1], total - pos);
    }
    base = __shfl(base, 0, 64);
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int at = base + __popcll(hit[p] & below);
        if (w[p] != 0 && at < max_tips) rec[at] = make_int4(row, col[p], w[p], 0);
        base += __popcll(hit[p]);
    }
}

// One pass over the plaquettes, in the shape of copy_kernel: as many 256-thread workgroups as it takes, nothing in LDS.
// VEC (planar slab, pitch == W, W a multiple of 4, both arrays 16-byte aligned): a thread takes the four plaquettes whose
// upper-left cells are (i, 4g .. 4g+3): one 16-byte load per array and row plus the cell to their right (the last group of a
// row has none and three plaquettes), the mask as one 32-bit load and one byte per row.  Otherwise (row-interleaved slab, or
// a width that leaves rows unaligned): one plaquette per thread, scalar.  Row i + 1 is loaded again by the thread of the
// plaquette below: that thread is in the same or the next workgroup, so the second read comes from the cache.
template <bool VEC>
__global__ void __launch_bounds__(256) tip_kernel(Geo g, const float *__restrict__ A, const float *__restrict__ B, float a0, float b0,
                                                  const unsigned char *__restrict__ mask, int *__restrict__ cnt, int4 *__restrict__ rec,
                                                  int max_tips)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t pitch = (size_t)g.pitch;
    if (VEC) {
        const size_t w4 = (size_t)g.W / 4;
        const size_t i = t / w4, c = 4 * (t % w4);
        int w[4] = {0, 0, 0, 0};
        const int col[4] = {(int)c, (int)c + 1, (int)c + 2, (int)c + 3};
        if (i + 1 < (size_t)g.H) {
            const bool last = c + 4 >= (size_t)g.W;                   // no cell to the right: three plaquettes
            const size_t up = i * pitch + c, dn = up + pitch;
            float a[2][5], b[2][5];
            bool in[2][5];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const size_t at = r ? dn : up;
                const fib_v4f va = *reinterpret_cast<const fib_v4f *>(A + at), vb = *reinterpret_cast<const fib_v4f *>(B + at);
                const unsigned m = mask ? *reinterpret_cast<const unsigned *>(mask + (i + r) * (size_t)g.W + c) : 0x01010101u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[r][j] = va[j] - a0;
                    b[r][j] = vb[j] - b0;
                    in[r][j] = ((m >> (8 * j)) & 0xFFu) != 0;
                }
                a[r][4] = last ? 0.f : A[at + 4] - a0;
                b[r][4] = last ? 0.f : B[at + 4] - b0;
                in[r][4] = !last && (!mask || mask[(i + r) * (size_t)g.W + c + 4] != 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float pa[4] = {a[0][j], a[0][j + 1], a[1][j + 1], a[1][j]};
                const float pb[4] = {b[0][j], b[0][j + 1], b[1][j + 1], b[1][j]};
                if (in[0][j] && in[0][j + 1] && in[1][j + 1] && in[1][j]) w[j] = tip_charge(pa, pb);
            }
        }
        tip_emit<4>(w, (int)i, col, cnt, rec, max_tips);
    } else {
        const size_t wp = (size_t)g.W - 1;                            // plaquettes per row
        const size_t i = t / wp, c = t % wp;
        int w[1] = {0};
        const int col[1] = {(int)c};
        if (i + 1 < (size_t)g.H) {
            const size_t up = i * pitch + c, dn = up + pitch;
            const size_t mu = i * (size_t)g.W + c, md = mu + (size_t)g.W;
            if (!mask || (mask[mu] && mask[mu + 1] && mask[md + 1] && mask[md])) {
                const float pa[4] = {A[up] - a0, A[up + 1] - a0, A[dn + 1] - a0, A[dn] - a0};
                const float pb[4] = {B[up] - b0, B[up + 1] - b0, B[dn + 1] - b0, B[dn] - b0};
                w[0] = tip_charge(pa, pb);
            }
        }
        tip_emit<1>(w, (int)i, col, cnt, rec, max_tips);
    }
}

// ---- frame recorder (fibhip_frames_begin): a window of one state array as a frame of the movie cube ---------------------
// Per cell, float32, every operation rounded on its own (-ffp-contract=off, IEEE division):  y = (X - lo) / span, then
// y = y * w where a weight plane is given.  A pixel is a block of by x bx cells: POINT takes y of its upper-left cell; MEAN sums
// each block row left to right (the row's first cell starts the sum), adds the row sums top to bottom (the first row's sum
// starts the total) and divides by (float)(by * bx) — an order fixed by the block alone.  F32 stores the pixel; U8 stores
// (unsigned char)(q * 255.0f + 0.5f), q the pixel with NaN -> 0, clamped to [0, 1].
struct FrameArgs {
    const float *x;         // the watched array (its first row), `pitch` floats between rows
    const float *w;         // the weight plane [H][W] (wpitch floats between rows), or null
    void *out;              // this sample's frame: [oh][ow] float32 or uint8
    int pitch, wpitch;
    int r0, c0, oh, ow, by, bx;
    float lo, span;
};

static FIB_DEV float frame_cell(float x, float lo, float span) { return (x - lo) / span; }
static FIB_DEV unsigned frame_u8(float p)
{
    float q = p != p ? 0.f : p;
    q = q < 0.f ? 0.f : (q > 1.f ? 1.f : q);
    return (unsigned)(unsigned char)(q * 255.0f + 0.5f);
}

// One pass in the shape of copy_kernel: as many 256-thread workgroups as it takes, nothing in LDS, no atomics.
// VEC (planar slab, every row of the window starts 16-byte aligned in the array and in the weight plane, ow a multiple of 4):
// a thread makes four consecutive pixels of one frame row.  It walks the 4 * bx cells under them as bx 16-byte pieces per
// block row, left to right, one 16-byte load of the state and one of the weights per piece, and stores the four pixels with
// one 16-byte (F32) or one 32-bit (U8) store.  At full resolution (bx = 1) consecutive lanes read consecutive pieces; a wider
// block makes a lane's pieces consecutive and a wave's loads of one block row cover one contiguous span, every byte of
// which is used.  The cell -> pixel bookkeeping (pos, k) depends on the loop counters alone: wave-uniform, kept in scalar
// registers; the four accumulators are addressed by selects, never by a run-time index (no scratch).
// Otherwise (row-interleaved slab, a window or a width that leaves rows unaligned, ow not a multiple of 4): one pixel per
// thread, scalar loads and one scalar store.
template <bool U8, bool MEAN, bool VEC>
__global__ void __launch_bounds__(256) frame_kernel(FrameArgs a)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const float n_cells = (float)(a.by * a.bx);
    if (VEC) {
        const size_t ow4 = (size_t)a.ow / 4;
        if (t >= (size_t)a.oh * ow4) return;
        const size_t oy = t / ow4, g = t % ow4;
        const size_t row0 = (size_t)a.r0 + oy * (size_t)a.by, col0 = (size_t)a.c0 + 4 * g * (size_t)a.bx;
        float pix[4] = {0.f, 0.f, 0.f, 0.f};
        if (!MEAN || (a.by == 1 && a.bx == 1)) {
            if (a.bx == 1) {
                const size_t at = row0 * (size_t)a.pitch + col0;
                const fib_v4f v = *reinterpret_cast<const fib_v4f *>(a.x + at);
#pragma unroll
                for (int e = 0; e < 4; ++e) pix[e] = frame_cell(v[e], a.lo, a.span);
                if (a.w) {
                    const fib_v4f wv = *reinterpret_cast<const fib_v4f *>(a.w + row0 * (size_t)a.wpitch + col0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) pix[e] = pix[e] * wv[e];
                }
            } else {                                                  // POINT under a wider block: the four upper-left cells only
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const size_t c = col0 + (size_t)e * (size_t)a.bx;
                    pix[e] = frame_cell(a.x[row0 * (size_t)a.pitch + c], a.lo, a.span);
                    if (a.w) pix[e] = pix[e] * a.w[row0 * (size_t)a.wpitch + c];
                }
            }
            if (MEAN) {
#pragma unroll
                for (int e = 0; e < 4; ++e) pix[e] = pix[e] / n_cells;
            }
        } else {
            for (int dy = 0; dy < a.by; ++dy) {
                const size_t xr = (row0 + (size_t)dy) * (size_t)a.pitch + col0, wr = (row0 + (size_t)dy) * (size_t)a.wpitch + col0;
                float rs[4] = {0.f, 0.f, 0.f, 0.f};
                int pos = 0, k = 0;                                   // the cell's place in its pixel, and the pixel: wave-uniform
                for (int j = 0; j < a.bx; ++j) {
                    const fib_v4f v = *reinterpret_cast<const fib_v4f *>(a.x + xr + 4 * (size_t)j);
                    fib_v4f wv = {1.f, 1.f, 1.f, 1.f};
                    if (a.w) wv = *reinterpret_cast<const fib_v4f *>(a.w + wr + 4 * (size_t)j);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float y = frame_cell(v[e], a.lo, a.span);
                        if (a.w) y = y * wv[e];
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (k == q) rs[q] = pos == 0 ? y : rs[q] + y;
                        if (++pos == a.bx) {
                            pos = 0;
                            ++k;
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) pix[q] = dy == 0 ? rs[q] : pix[q] + rs[q];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) pix[q] = pix[q] / n_cells;
        }
        const size_t o = oy * (size_t)a.ow + 4 * g;
        if (U8) {
            const unsigned packed = frame_u8(pix[0]) | (frame_u8(pix[1]) << 8) | (frame_u8(pix[2]) << 16) | (frame_u8(pix[3]) << 24);
            *reinterpret_cast<unsigned *>(static_cast<unsigned char *>(a.out) + o) = packed;
        } else {
            fib_v4f p4 = {pix[0], pix[1], pix[2], pix[3]};
            *reinterpret_cast<fib_v4f *>(static_cast<float *>(a.out) + o) = p4;
        }
    } else {
        if (t >= (size_t)a.oh * (size_t)a.ow) return;
        const size_t oy = t / (size_t)a.ow, ox = t % (size_t)a.ow;
        const size_t row0 = (size_t)a.r0 + oy * (size_t)a.by, col0 = (size_t)a.c0 + ox * (size_t)a.bx;
        float pix = 0.f;
        if (!MEAN) {
            pix = frame_cell(a.x[row0 * (size_t)a.pitch + col0], a.lo, a.span);
            if (a.w) pix = pix * a.w[row0 * (size_t)a.wpitch + col0];
        } else {
            for (int dy = 0; dy < a.by; ++dy) {
                const size_t xr = (row0 + (size_t)dy) * (size_t)a.pitch + col0, wr = (row0 + (size_t)dy) * (size_t)a.wpitch + col0;
                float rs = 0.f;
                for (int dx = 0; dx < a.bx; ++dx) {
                    float y = frame_cell(a.x[xr + (size_t)dx], a.lo, a.span);
                    if (a.w) y = y * a.w[wr + (size_t)dx];
                    rs = dx == 0 ? y : rs + y;
                }
                pix = dy == 0 ? rs : pix + rs;
            }
            pix = pix / n_cells;
        }
        if (U8) static_cast<unsigned char *>(a.out)[t] = (unsigned char)frame_u8(pix);
        else static_cast<float *>(a.out)[t] = pix;
    }
}

// ---- statistics recorder (fibhip_stats_begin): whole-tissue scalars of several state arrays, one row per sample -----------
// A column is {array, kind, level}; the host groups the columns by array (StArr: up to ST_SLOTS columns each) and cuts the
// H x W cells, row-major, into chunks (StChunk) from H, W and the pitch alone.  Grid (chunks, arrays): a workgroup of
// ST_THREADS threads walks ONE chunk of ONE array once and evaluates every column on that array, so each array named is read
// once per sample; the weight plane is read where the array has a SUM column, the mask where it has any other.
//   SUM        acc = acc + (double)w * (double)x over the cells with w != 0 (w = 1 without a plane): the product of two float32
//              is exact in double, the addition is rounded on its own (-ffp-contract=off: no fma)
//   MIN, MAX   over the masked cells, `x < acc` / `x > acc` from +inf / -inf: a NaN compares false and is ignored
//   BELOW, ABOVE, NONFINITE   32-bit counts per thread, 64-bit from the wave on
// VEC (planar slab, pitch == W, W a multiple of 4, every pointer 16-byte aligned): thread t takes the chunk's 16-byte groups
// t, t + ST_THREADS, ... with ST_VBATCH groups' loads in flight, the mask as one 32-bit load per group.  Otherwise thread t
// takes the cells t, t + ST_THREADS, ... one load each, ST_SBATCH in flight.  A cell beyond the chunk's end gets w = 0 and
// mask = 0 (and an in-range address), which drops it from every column.  The kernel is a pure streaming read.
// The accumulators of the up to ST_SLOTS columns are addressed by fully unrolled loops only (a run-time index would put them
// in scratch: frame_kernel's note); the column's kind is wave-uniform, so the switch is a scalar branch per batch, not per
// cell.  Per thread the order is fixed; then six levels of __shfl_down in each wave, the wave results through LDS, a fixed
// tree over the four of them by one thread per column, and ONE plain 64-bit store per (column, chunk) into the partials
// [array][slot][chunk].  stats_combine_kernel — a second launch on the same stream, the launch-boundary reduce that makes
// float sums reproducible bit for bit — folds the chunks of every column in a fixed tree and writes the sample's row.
// No floating-point atomics, no atomics at all.
#define ST_THREADS 256
#define ST_VBATCH 4
#define ST_SBATCH 8
#define ST_SLOTS 8              // columns on one array
#define ST_MAX_CHUNKS 256       // chunks of one array: what stats_combine_kernel folds per column, four per lane
#define ST_MIN_CHUNK 1024       // cells (a multiple of 4): one 16-byte group per thread
enum { ST_SUM = 0, ST_MIN = 1, ST_MAX = 2, ST_BELOW = 3, ST_ABOVE = 4, ST_NONFINITE = 5, ST_KINDS = 6 };
struct StChunk {
    unsigned first, count;      // cells [first, first + count) of the grid, row-major; both multiples of 4 on the VEC path
};
struct StArr {
    int var, ncols;
    int need_w, need_m;         // a SUM column / a column of any other kind
    int kind[ST_SLOTS];
    float level[ST_SLOTS];
};
struct StCol {
    int arr, slot, kind, pad;   // where column c of the row comes from
};
struct StArgs {
    const float *slab0, *slab1;
    unsigned cur_mask;          // bit v: array v lives in slab1
    int W, pitch;
    unsigned long long vstride;
    const StChunk *chunks;
    const StArr *arrs;
    const float *w;             // [H][W] or null
    const unsigned char *mask;  // [H][W] or null
    unsigned long long *part;   // [narr][ST_SLOTS][nchunks]
    int nchunks;
};

static FIB_DEV unsigned long long st_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
static FIB_DEV double st_dbl(unsigned long long b) { return __longlong_as_double((long long)b); }
static FIB_DEV unsigned long long st_identity(int kind)
{
    return kind == ST_MIN ? st_bits(__builtin_huge_val()) : kind == ST_MAX ? st_bits(-__builtin_huge_val()) : 0ull;
}
// a (the earlier operand) combined with b: a double sum, the smaller / larger double (no NaN gets this far), or an integer sum
static FIB_DEV unsigned long long st_fold(int kind, unsigned long long a, unsigned long long b)
{
    if (kind == ST_SUM) return st_bits(st_dbl(a) + st_dbl(b));
    if (kind == ST_MIN) return st_dbl(b) < st_dbl(a) ? b : a;
    if (kind == ST_MAX) return st_dbl(b) > st_dbl(a) ? b : a;
    return a + b;
}
static FIB_DEV unsigned long long st_wave_fold(int kind, unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = st_fold(kind, v, __shfl_down(v, off, 64));
    return v;
}

// N cells of one thread (x, weight, mask: registers) into the accumulators of the array's columns
template <int N>
static FIB_DEV void st_take(const StArr *__restrict__ d, const float (&x)[N], const float (&w)[N], const bool (&m)[N],
                            double (&sd)[ST_SLOTS], unsigned (&sn)[ST_SLOTS])
{
    const int ncols = d->ncols;
#pragma unroll
    for (int j = 0; j < ST_SLOTS; ++j) {
        if (j >= ncols) continue;                                     // (wave-uniform, like `kind`)
        const int kind = d->kind[j];
        const float level = d->level[j];
        if (kind == ST_SUM) {
#pragma unroll
            for (int e = 0; e < N; ++e)
                if (w[e] != 0.f) sd[j] = sd[j] + (double)w[e] * (double)x[e];
        } else if (kind == ST_MIN) {
#pragma unroll
            for (int e = 0; e < N; ++e)
                if (m[e] && (double)x[e] < sd[j]) sd[j] = (double)x[e];
        } else if (kind == ST_MAX) {
#pragma unroll
            for (int e = 0; e < N; ++e)
                if (m[e] && (double)x[e] > sd[j]) sd[j] = (double)x[e];
        } else if (kind == ST_BELOW) {
#pragma unroll
            for (int e = 0; e < N; ++e) sn[j] += (m[e] && x[e] < level) ? 1u : 0u;
        } else if (kind == ST_ABOVE) {
#pragma unroll
            for (int e = 0; e < N; ++e) sn[j] += (m[e] && x[e] > level) ? 1u : 0u;
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) sn[j] += (m[e] && !(__builtin_fabsf(x[e]) < __builtin_huge_valf())) ? 1u : 0u;
        }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(ST_THREADS) stats_kernel(StArgs a)
{
    __shared__ unsigned long long wres[ST_THREADS / 64][ST_SLOTS];
    const StArr *__restrict__ d = a.arrs + blockIdx.y;
    const StChunk c = a.chunks[blockIdx.x];
    const float *__restrict__ x = (((a.cur_mask >> d->var) & 1u) ? a.slab1 : a.slab0) + (size_t)d->var * (size_t)a.vstride;
    const float *__restrict__ wp = d->need_w ? a.w : nullptr;
    const unsigned char *__restrict__ mp = d->need_m ? a.mask : nullptr;
    const unsigned end = c.first + c.count;
    double sd[ST_SLOTS];
    unsigned sn[ST_SLOTS];
#pragma unroll
    for (int j = 0; j < ST_SLOTS; ++j) {
        sd[j] = j < d->ncols ? st_dbl(st_identity(d->kind[j])) : 0.0;
        sn[j] = 0u;
    }
    if (VEC) {
        for (unsigned p0 = c.first + 4u * threadIdx.x; p0 < end; p0 += 4u * ST_VBATCH * ST_THREADS) {
            fib_v4f xv[ST_VBATCH], wv[ST_VBATCH];
            unsigned mv[ST_VBATCH];
#pragma unroll
            for (int b = 0; b < ST_VBATCH; ++b) {
                const unsigned p = p0 + 4u * (unsigned)b * ST_THREADS;
                const bool in = p < end;
                const unsigned q = in ? p : c.first;                  // (an in-range address; the cells are dropped below)
                xv[b] = *reinterpret_cast<const fib_v4f *>(x + q);
                const fib_v4f one = {1.f, 1.f, 1.f, 1.f};
                wv[b] = wp ? *reinterpret_cast<const fib_v4f *>(wp + q) : one;
                mv[b] = mp ? *reinterpret_cast<const unsigned *>(mp + q) : 0x01010101u;
                if (!in) {
                    const fib_v4f zero = {0.f, 0.f, 0.f, 0.f};
                    wv[b] = zero;
                    mv[b] = 0u;
                }
            }
            float xs[4 * ST_VBATCH], ws[4 * ST_VBATCH];
            bool ms[4 * ST_VBATCH];
#pragma unroll
            for (int b = 0; b < ST_VBATCH; ++b)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xs[4 * b + e] = xv[b][e];
                    ws[4 * b + e] = wv[b][e];
                    ms[4 * b + e] = ((mv[b] >> (8 * e)) & 0xFFu) != 0u;
                }
            st_take<4 * ST_VBATCH>(d, xs, ws, ms, sd, sn);
        }
    } else {
        for (unsigned p0 = c.first + threadIdx.x; p0 < end; p0 += ST_SBATCH * ST_THREADS) {
            float xs[ST_SBATCH], ws[ST_SBATCH];
            bool ms[ST_SBATCH];
#pragma unroll
            for (int b = 0; b < ST_SBATCH; ++b) {
                const unsigned p = p0 + (unsigned)b * ST_THREADS;
                const bool in = p < end;
                const unsigned q = in ? p : c.first;
                const unsigned r = q / (unsigned)a.W, col = q - r * (unsigned)a.W;
                xs[b] = x[(size_t)r * (size_t)a.pitch + col];
                const float wq = wp ? wp[q] : 1.f;
                const bool mq = mp ? mp[q] != 0 : true;
                ws[b] = in ? wq : 0.f;
                ms[b] = in && mq;
            }
            st_take<ST_SBATCH>(d, xs, ws, ms, sd, sn);
        }
    }
#pragma unroll
    for (int j = 0; j < ST_SLOTS; ++j) {
        if (j >= d->ncols) continue;
        const int kind = d->kind[j];
        const unsigned long long v = st_wave_fold(kind, kind <= ST_MAX ? st_bits(sd[j]) : (unsigned long long)sn[j]);
        if ((threadIdx.x & 63) == 0) wres[threadIdx.x >> 6][j] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < d->ncols) {
        const int kind = a.arrs[blockIdx.y].kind[threadIdx.x];         // (from memory: the slot is a run-time index here)
        const unsigned long long v = st_fold(kind, st_fold(kind, wres[0][threadIdx.x], wres[1][threadIdx.x]),
                                             st_fold(kind, wres[2][threadIdx.x], wres[3][threadIdx.x]));
        a.part[((size_t)blockIdx.y * ST_SLOTS + threadIdx.x) * (size_t)a.nchunks + blockIdx.x] = v;
    }
}

// ONE workgroup of four waves; wave v folds the columns v, v + 4, ...: lane l takes the partials of chunks 4l .. 4l + 3 as
// (p0 . p1) . (p2 . p3) (the identity where the array has fewer chunks), then the six levels of the wave.  Counts are stored
// converted to double, which is exact.
__global__ void __launch_bounds__(256) stats_combine_kernel(const StCol *__restrict__ cols, int ncols, const unsigned long long *__restrict__ part,
                                                            int nchunks, double *__restrict__ row)
{
    const int lane = (int)(threadIdx.x & 63u);
    for (int c = (int)(threadIdx.x >> 6); c < ncols; c += 4) {
        const StCol col = cols[c];
        const unsigned long long *__restrict__ p = part + ((size_t)col.arr * ST_SLOTS + (size_t)col.slot) * (size_t)nchunks;
        const unsigned long long id = st_identity(col.kind);
        unsigned long long q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = 4 * lane + e < nchunks ? p[4 * lane + e] : id;
        unsigned long long v = st_fold(col.kind, st_fold(col.kind, q[0], q[1]), st_fold(col.kind, q[2], q[3]));
        v = st_wave_fold(col.kind, v);
        if (lane == 0) row[c] = col.kind <= ST_MAX ? st_dbl(v) : (double)v;
    }
}

// plain streaming copy, one 16-byte element per thread and as many workgroups as that takes: the bandwidth yardstick
// bench.py prints next to the roofline peak.  (tools/ubench/copybw.hip -> profiles/r02_copy_bandwidth_shapes.txt: this
// shape reaches the 6.3 TB/s the microarch guide quotes; grid-stride loops with non-temporal accesses stay at 4.6-5.7,
// reads alone run at 7.0, writes alone at 4.4 TB/s)
__global__ void __launch_bounds__(256) copy_kernel(const fib_v4f *__restrict__ src, fib_v4f *__restrict__ dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- stimulus program (fibhip_stim_begin): the entries due after one tick, applied to the state in ONE pass -------------------
// The one kernel here that WRITES the state: the actuator beside the five sensors above.  An entry is a mode (MAX: X = fmaxf(X, S),
// pace_kernel's operation; ADD: X = X + S, one float32 addition rounded on its own under -ffp-contract=off), a target array and a
// shape that gives S per cell: a rectangle (v inside, `floor` outside) or a plane [H][W].  A cell whose S is the mode's
// "untouched" value (-inf for MAX, +-0 for ADD) is not changed at all, whatever its bits; the host has cut each entry's VISIT
// box around the cells that are not (fibhip_stim_begin) and the launch covers the union of the due entries' boxes.
// The due entries — at most STIM_MAX_DUE, the host issues further launches in program order beyond that — travel BY VALUE in the
// kernel argument and are walked by a fully unrolled loop: every field is wave-uniform and stays in scalar registers (a run-time
// index into a per-thread copy would put it in scratch: frame_kernel's note).  The host has grouped them by array (stable: the
// program order of the entries on one array stands, entries on different arrays touch different memory and commute) and marked
// where an array's run begins (`load`) and ends (`store`): a thread loads its cells of an array once and stores them once,
// whatever the number of entries.  VEC (planar slab, W a multiple of 4, every pointer 16-byte aligned; the union box widened
// to whole groups of four columns): four consecutive cells of one row per thread, 16-byte loads and stores of the state and
// the planes.  Otherwise (odd widths, rows that start unaligned, the row-interleaved slab): one cell per thread.  No LDS, no
// atomics.  `give_up`: the give-up word of the multi-tick launches (null: the handle never made one) — a launch in front that
// gave up left the word raised, the state it started from is what recover() goes back to, and this kernel then writes NOTHING,
// like the multi-tick launches queued behind such a launch (sched.inc, the rule above confirm()).
#define STIM_MAX_DUE 8
enum { STIM_MAX = 0, STIM_ADD = 1 };
struct StimDue {
    float *x;               // the target array in the slab that holds it now (its first row), `pitch` floats between rows
    const float *plane;     // S per cell, [H][W], or null: a rectangle
    int mode;               // STIM_MAX / STIM_ADD
    int load, store;        // first / last entry of its array's run in this launch
    int b_r0, b_r1, b_c0, b_c1;     // the visit box: outside it the entry leaves every cell untouched
    int r0, r1, c0, c1;     // rectangle: S = v inside, floor outside
    float v, floor;
};
struct StimArgs {
    StimDue e[STIM_MAX_DUE];
    int n;
    int W, pitch;
    int r0, r1, c0, c1;     // the union of the due entries' visit boxes (VEC: c0 and c1 multiples of 4)
    const unsigned *give_up;
};

static FIB_DEV float stim_cell(float x, float s, int mode)
{
    if (mode == STIM_MAX) return s == -__builtin_huge_valf() ? x : fmaxf(x, s);
    return s == 0.f ? x : x + s;
}

template <bool VEC>
__global__ void __launch_bounds__(256) stim_kernel(StimArgs a)
{
    constexpr int N = VEC ? 4 : 1;
    if (a.give_up && *a.give_up != 0u) return;                        // (wave-uniform: one scalar load)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per_row = (size_t)(a.c1 - a.c0) / N;
    if (t >= (size_t)(a.r1 - a.r0) * per_row) return;
    const int y = a.r0 + (int)(t / per_row), x0 = a.c0 + N * (int)(t % per_row);
    const size_t at = (size_t)y * (size_t)a.pitch + (size_t)x0;
    float x[N];
#pragma unroll
    for (int i = 0; i < STIM_MAX_DUE; ++i) {
        if (i >= a.n) continue;                                       // (wave-uniform, like every field of a.e[i])
        const StimDue &d = a.e[i];
        if (d.load) {
            if (VEC) {
                const fib_v4f v = *reinterpret_cast<const fib_v4f *>(d.x + at);
#pragma unroll
                for (int j = 0; j < N; ++j) x[j] = v[j];
            } else {
                x[0] = d.x[at];
            }
        }
        if (y >= d.b_r0 && y < d.b_r1 && x0 + N > d.b_c0 && x0 < d.b_c1) {
            float s[N];
            if (d.plane) {
                const size_t pat = (size_t)y * (size_t)a.W + (size_t)x0;
                if (VEC) {
                    const fib_v4f v = *reinterpret_cast<const fib_v4f *>(d.plane + pat);
#pragma unroll
                    for (int j = 0; j < N; ++j) s[j] = v[j];
                } else {
                    s[0] = d.plane[pat];
                }
            } else {
#pragma unroll
                for (int j = 0; j < N; ++j) s[j] = (y >= d.r0 && y < d.r1 && x0 + j >= d.c0 && x0 + j < d.c1) ? d.v : d.floor;
            }
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (x0 + j >= d.b_c0 && x0 + j < d.b_c1) x[j] = stim_cell(x[j], s[j], d.mode);
        }
        if (d.store) {
            if (VEC) {
                fib_v4f v;
#pragma unroll
                for (int j = 0; j < N; ++j) v[j] = x[j];
                *reinterpret_cast<fib_v4f *>(d.x + at) = v;
            } else {
                d.x[at] = x[0];
            }
        }
    }
}

// ---- trigger program (fibhip_trig_begin): sense a site, decide, fire — three small launches behind a sample tick -------------
// sense_kernel counts, per sensor, the cells of its site with X > level (strict float32 compare: a NaN does not count).  The
// count is an INTEGER and independent of order — a decision must not hang on the rounding of a float sum — so there is no fixed
// tree here: wave ballots, popcounts, integer adds.  Grid (chunks, sensors): a workgroup of SENSE_THREADS threads walks one
// chunk of the items of one sensor's box, row-major (an item: VEC — planar slab, W a multiple of 4, every pointer 16-byte
// aligned, the box widened to whole groups of four columns — four consecutive cells of one row, one 16-byte load and the
// mask's four bytes as one 32-bit load; otherwise one cell).  The loop is wave-uniform (an item beyond the chunk's end gets an
// in-range address and a false predicate), each predicate goes through __ballot and the popcount lands in a scalar register;
// lane 0 of each wave hands its count through LDS, one thread adds the four and writes ONE plain 32-bit vector store per
// (sensor, chunk).  Workgroups beyond a sensor's last chunk leave at once.  No atomics, no float arithmetic at all.
#define TRIG_MAX 8                  // sensors / rules of one program (== STIM_MAX_DUE: the rules' stimuli fit one launch)
#define SENSE_THREADS 256
#define SENSE_MAX_CHUNKS 256        // chunks of one sensor: what trigger_kernel folds, four per lane of one wave
#define SENSE_MIN_CHUNK 1024        // items (a multiple of SENSE_THREADS)
struct SenseSite {
    int var;
    float level;
    int need;
    int r0, r1, c0, c1;             // the site's box: the cells inside it count (and where the mask is not 0, if there is one)
    int mask;                       // index into the masks, or -1: the rectangle itself
    // [0]: one cell per item; [1]: VEC, columns [c0 / 4 * 4, (c1 + 3) / 4 * 4) in groups of four
    unsigned per_row[2], items[2], per_chunk[2];
    int nchunks[2];
};
struct SenseArgs {
    const float *slab0, *slab1;
    unsigned cur_mask;              // bit v: array v lives in slab1
    int W, pitch;
    unsigned long long vstride, cells;
    const SenseSite *sites;
    const unsigned char *masks;     // [nmasks][H][W] or null
    unsigned *part;                 // [nsensors][SENSE_MAX_CHUNKS]
};

template <bool VEC>
__global__ void __launch_bounds__(SENSE_THREADS) sense_kernel(SenseArgs a)
{
    constexpr int N = VEC ? 4 : 1;
    __shared__ unsigned wres[SENSE_THREADS / 64];
    const SenseSite *__restrict__ d = a.sites + blockIdx.y;               // (wave-uniform: scalar loads)
    if ((int)blockIdx.x >= d->nchunks[VEC]) return;
    const float *__restrict__ x = (((a.cur_mask >> d->var) & 1u) ? a.slab1 : a.slab0) + (size_t)d->var * (size_t)a.vstride;
    const unsigned char *__restrict__ mp = d->mask >= 0 ? a.masks + (size_t)d->mask * (size_t)a.cells : nullptr;
    const float level = d->level;
    const int r0 = d->r0, c0 = d->c0, c1 = d->c1, cv0 = VEC ? c0 / 4 * 4 : c0;
    const unsigned per_row = d->per_row[VEC], items = d->items[VEC], per_chunk = d->per_chunk[VEC];
    const unsigned first = blockIdx.x * per_chunk;                        // (< items: blockIdx.x < nchunks)
    const unsigned end = items - first < per_chunk ? items : first + per_chunk;
    unsigned count = 0u;                                                  // (wave-uniform: sums of popcounts)
    for (unsigned base = first; base < end; base += SENSE_THREADS) {
        const unsigned t = base + threadIdx.x;
        const bool in = t < end;
        const unsigned q = in ? t : first;                                // (an in-range address; the predicate drops it)
        const int y = r0 + (int)(q / per_row), x0 = cv0 + N * (int)(q % per_row);
        const size_t at = (size_t)y * (size_t)a.pitch + (size_t)x0, mat = (size_t)y * (size_t)a.W + (size_t)x0;
        float xs[N];
        unsigned m;
        if (VEC) {
            const fib_v4f v = *reinterpret_cast<const fib_v4f *>(x + at);
#pragma unroll
            for (int j = 0; j < N; ++j) xs[j] = v[j];
            m = mp ? *reinterpret_cast<const unsigned *>(mp + mat) : 0x01010101u;
        } else {
            xs[0] = x[at];
            m = mp ? (unsigned)mp[mat] : 1u;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const bool hit = in && x0 + j >= c0 && x0 + j < c1 && ((m >> (8 * j)) & 0xFFu) != 0u && xs[j] > level;
            count += (unsigned)__popcll(__ballot(hit));
        }
    }
    if ((threadIdx.x & 63u) == 0u) wres[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) a.part[(size_t)blockIdx.y * SENSE_MAX_CHUNKS + blockIdx.x] = (wres[0] + wres[1]) + (wres[2] + wres[3]);
}

// trigger_kernel: ONE workgroup of four waves; the waves 1 .. 3 only fold (they leave behind the barrier), wave 0 folds and then
// runs the rules, one per lane.  Wave w folds the partials of the sensors w, w + 4 (lane l: chunks 4l .. 4l + 3,
// then six levels of __shfl_down; integer adds, so the order is free) into c_s and a_s = (c_s >= need).  Then thread r < nrules
// runs rule r's automaton (include/fibhip.h: the normative text; tests/trigger_ref.py: the restatement) from row s - 1 — the
// virtual row a = -1, t = -1, n = 0 when s == 0 — and the sensor's a_s, writes row s = {c, a, t, n, cause, fired} and, through
// one ballot, the fire-mask word of sample s (bit r: rule r fires).  The slot s is a kernel ARGUMENT computed from the host's
// counter: nothing on the device says where the log ends, so a replay (recover()) rewrites the rows of the lost samples in
// place, each from a predecessor that is older than the lost launch or already rewritten.
enum { TRIG_RISE = 0, TRIG_FALL = 1, TRIG_ROW = 6 };
struct TrigRule {
    int sensor, edge, arm, blank, escape, max_det, delay, count, period, hold;
};
__global__ void __launch_bounds__(256) trigger_kernel(const SenseSite *__restrict__ sites, int nsensors, int vec, const unsigned *__restrict__ part,
                                                      const TrigRule *__restrict__ rules, int nrules, int *__restrict__ rows,
                                                      unsigned *__restrict__ fire, int s)
{
    __shared__ int cs[TRIG_MAX];
    const int lane = (int)(threadIdx.x & 63u);
    for (int i = (int)(threadIdx.x >> 6); i < nsensors; i += 4) {
        const int nchunks = sites[i].nchunks[vec];
        const unsigned *__restrict__ p = part + (size_t)i * SENSE_MAX_CHUNKS;
        unsigned v = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) v += 4 * lane + e < nchunks ? p[4 * lane + e] : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) cs[i] = (int)v;
    }
    __syncthreads();
    if (threadIdx.x >= 64u) return;
    const int r = (int)threadIdx.x;
    bool fired = false;
    if (r < nrules) {
        const TrigRule k = rules[r];
        const int c = cs[k.sensor], a = c >= sites[k.sensor].need ? 1 : 0;
        int pa = -1, pt = -1, pn = 0;
        if (s > 0) {
            const int *__restrict__ p = rows + ((size_t)(s - 1) * (size_t)nrules + (size_t)r) * TRIG_ROW;
            pa = p[1]; pt = p[2]; pn = p[3];
        }
        const bool e = pa >= 0 && (k.edge == TRIG_RISE ? (pa == 0 && a == 1) : (pa == 1 && a == 0));
        const bool listen = s >= k.arm && (k.max_det == 0 || pn < k.max_det) && (pt < 0 || pt + 1 >= k.blank);
        const bool quiet = k.escape > 0 && listen && ((pt < 0 ? s - k.arm : pt) + 1 >= k.escape);
        const bool det = listen && (e || quiet);
        const int cause = det ? (e ? 1 : 2) : 0;
        const int t = det ? 0 : (pt < 0 ? -1 : pt + 1);
        const int n = pn + (det ? 1 : 0);
        const int u = t - k.delay;
        fired = t >= 0 && u >= 0 && (k.period == 0 ? u < k.hold : (u / k.period < k.count && u % k.period < k.hold));
        int *__restrict__ o = rows + ((size_t)s * (size_t)nrules + (size_t)r) * TRIG_ROW;
        o[0] = c; o[1] = a; o[2] = t; o[3] = n; o[4] = cause; o[5] = fired ? 1 : 0;
    }
    const unsigned long long f = __ballot(fired);
    if (r == 0) fire[s] = (unsigned)f;
}

// The gated apply: stim_kernel's operations on the rules' stimuli — all of them by value in every launch (TRIG_MAX ==
// STIM_MAX_DUE), entry r is rule r's, walked by the same fully unrolled loop (every field wave-uniform, in scalar registers).  It
// reads the give-up word first (null behind a plain tick), then the fire mask of sample s: both wave-uniform scalar loads.  It
// leaves without writing when a launch in front gave up — the mask it would read was then made from a void slab — or when no
// rule fires.  An entry whose bit is clear is skipped; one whose bit is set loads, changes and stores its own cells inside its
// visit box (a skipped neighbour cannot load or store for it, so the `load` / `store` marks of stim_kernel are not used; entries
// on one array follow each other in rule order through memory, each thread its own cells).  A sibling of stim_kernel rather than
// a template parameter of it: stim_kernel<true / false> stay exactly the code they were.  No LDS, no atomics.
template <bool VEC>
__global__ void __launch_bounds__(256) stim_gated_kernel(StimArgs a, const unsigned *__restrict__ fire)
{
    constexpr int N = VEC ? 4 : 1;
    if (a.give_up && *a.give_up != 0u) return;
    const unsigned f = *fire;
    if (f == 0u) return;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per_row = (size_t)(a.c1 - a.c0) / N;
    if (t >= (size_t)(a.r1 - a.r0) * per_row) return;
    const int y = a.r0 + (int)(t / per_row), x0 = a.c0 + N * (int)(t % per_row);
    const size_t at = (size_t)y * (size_t)a.pitch + (size_t)x0;
#pragma unroll
    for (int i = 0; i < STIM_MAX_DUE; ++i) {
        if (i >= a.n || !((f >> i) & 1u)) continue;                   // (wave-uniform, like every field of a.e[i])
        const StimDue &d = a.e[i];
        if (!(y >= d.b_r0 && y < d.b_r1 && x0 + N > d.b_c0 && x0 < d.b_c1)) continue;
        float x[N], s[N];
        if (VEC) {
            const fib_v4f v = *reinterpret_cast<const fib_v4f *>(d.x + at);
#pragma unroll
            for (int j = 0; j < N; ++j) x[j] = v[j];
        } else {
            x[0] = d.x[at];
        }
        if (d.plane) {
            const size_t pat = (size_t)y * (size_t)a.W + (size_t)x0;
            if (VEC) {
                const fib_v4f v = *reinterpret_cast<const fib_v4f *>(d.plane + pat);
#pragma unroll
                for (int j = 0; j < N; ++j) s[j] = v[j];
            } else {
                s[0] = d.plane[pat];
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) s[j] = (y >= d.r0 && y < d.r1 && x0 + j >= d.c0 && x0 + j < d.c1) ? d.v : d.floor;
        }
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (x0 + j >= d.b_c0 && x0 + j < d.b_c1) x[j] = stim_cell(x[j], s[j], d.mode);
        if (VEC) {
            fib_v4f v;
#pragma unroll
            for (int j = 0; j < N; ++j) v[j] = x[j];
            *reinterpret_cast<fib_v4f *>(d.x + at) = v;
        } else {
            d.x[at] = x[0];
        }
    }
}

// ---- spectrum recorder (fibhip_spectrum_begin): a per-pixel Welch periodogram folded while the run goes on --------------------
// Three kernels.  spectrum_sample_kernel writes the pixel plane of a sample tick — the frame recorder's pixel at lo = 0,
// span = 1, float32 — into slot s mod chunk of a ring of `chunk` planes; spectrum_fold_kernel, behind the sample that fills the
// ring, adds the ring's samples to the running DFT sums Re / Im of the recorded bins and, when the chunk ends a segment, the
// segment's power to P; spectrum_peak_kernel makes the four peak maps from P on demand.  Planes are [nb][oh * ow], consecutive
// lanes take consecutive pixels; no LDS, no atomics.
// Both the sample and the fold read the give-up word of the multi-tick launches first (`give_up`, null behind plain ticks:
// stim_kernel's note) and write NOTHING when it is raised.  The fold because it accumulates: a fold replayed by recover() must
// not find its samples folded already.  The sample because the ring is shorter than what may be queued behind an unconfirmed
// launch: a sample of a void slab, taken behind a launch that gave up, would overwrite a slot whose good sample — older than
// that launch, so never replayed — has not been folded yet (its fold, gated, did nothing).  That is also why the sample is a
// sibling of frame_kernel and not frame_kernel itself, whose code stays as it is.
struct SpecSampleArgs {
    const float *x;         // the watched array (its first row), `pitch` floats between rows
    const float *w;         // the weight plane [H][W] (wpitch floats between rows), or null
    float *out;             // the ring slot: [oh][ow]
    int pitch, wpitch;
    int r0, c0, oh, ow, by, bx;
    const unsigned *give_up;
};

// One pixel per thread, frame_kernel's scalar path at lo = 0, span = 1 (the subtraction and the division are kept: a pixel is
// the frame recorder's bit for bit); VEC (planar slab, full resolution, every row of the window 16-byte aligned in the array,
// the weight plane and the slot): four consecutive pixels per thread, one 16-byte load each and one 16-byte store (a block of
// one cell: MEAN divides by 1.0f, which changes nothing).
template <bool MEAN, bool VEC>
__global__ void __launch_bounds__(256) spectrum_sample_kernel(SpecSampleArgs a)
{
    if (a.give_up && *a.give_up != 0u) return;                        // (wave-uniform: one scalar load)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {                                                        // by == bx == 1
        const size_t ow4 = (size_t)a.ow / 4;
        if (t >= (size_t)a.oh * ow4) return;
        const size_t oy = t / ow4, g = t % ow4;
        const size_t row = (size_t)a.r0 + oy, col = (size_t)a.c0 + 4 * g;
        const fib_v4f v = *reinterpret_cast<const fib_v4f *>(a.x + row * (size_t)a.pitch + col);
        fib_v4f p;
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = frame_cell(v[e], 0.f, 1.f);
        if (a.w) {
            const fib_v4f wv = *reinterpret_cast<const fib_v4f *>(a.w + row * (size_t)a.wpitch + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = p[e] * wv[e];
        }
        *reinterpret_cast<fib_v4f *>(a.out + oy * (size_t)a.ow + 4 * g) = p;
    } else {
        if (t >= (size_t)a.oh * (size_t)a.ow) return;
        const size_t oy = t / (size_t)a.ow, ox = t % (size_t)a.ow;
        const size_t row0 = (size_t)a.r0 + oy * (size_t)a.by, col0 = (size_t)a.c0 + ox * (size_t)a.bx;
        float pix = 0.f;
        if (!MEAN) {
            pix = frame_cell(a.x[row0 * (size_t)a.pitch + col0], 0.f, 1.f);
            if (a.w) pix = pix * a.w[row0 * (size_t)a.wpitch + col0];
        } else {
            const float n_cells = (float)(a.by * a.bx);
            for (int dy = 0; dy < a.by; ++dy) {
                const size_t xr = (row0 + (size_t)dy) * (size_t)a.pitch + col0, wr = (row0 + (size_t)dy) * (size_t)a.wpitch + col0;
                float rs = 0.f;
                for (int dx = 0; dx < a.bx; ++dx) {
                    float y = frame_cell(a.x[xr + (size_t)dx], 0.f, 1.f);
                    if (a.w) y = y * a.w[wr + (size_t)dx];
                    rs = dx == 0 ? y : rs + y;
                }
                pix = dy == 0 ? rs : pix + rs;
            }
            pix = pix / n_cells;
        }
        a.out[t] = pix;
    }
}

// The fold of one chunk: ring slot c holds the sample at segment position j0 + c.  A thread owns one pixel: it reads the pixel's
// CHUNK ring values once and forms y = x * win[j] once (CHUNK registers, statically indexed: CHUNK is a template parameter),
// then walks the bins with Re and Im in registers:  Re = Re + y * tw[m][0], Im = Im + y * tw[m][1], m = (k * j) mod N, samples
// ascending, every operation rounded on its own (-ffp-contract=off).  j, k, m, the window entry and the twiddle pair depend on
// kernel arguments and loop counters alone: wave-uniform, scalar loads into scalar registers — never a per-lane gather.  m is
// carried, not divided for: one modulus per bin, then m += k, minus N on overflow (k <= N / 2 <= 32768 and j < N <= 65536: k * j
// fits 32 bits unsigned).
// A chunk that starts a segment (j0 == 0) starts Re and Im at +0 without reading them; one that ends a segment (`seg_end`) adds
// (Re * Re) + (Im * Im) to P and stores +0.  Traffic per pixel: CHUNK * 4 + nb * 16 bytes, plus 8 per bin at a segment end.
#define SPEC_MAX_BINS 128
#define SPEC_MAX_CHUNK 32
template <int CHUNK>
__global__ void __launch_bounds__(256)
spectrum_fold_kernel(const float *__restrict__ ring /* [CHUNK][npix] */, float *__restrict__ re_p, float *__restrict__ im_p,
                     float *__restrict__ P /* [nb][npix] each */, const float *__restrict__ win /* [N] */,
                     const float2 *__restrict__ tw /* [N] */, const int *__restrict__ bins /* [nb] */, size_t npix, int N, int nb, int j0,
                     int seg_end, const unsigned *give_up)
{
    if (give_up && *give_up != 0u) return;                            // (wave-uniform: one scalar load)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix) return;
    float y[CHUNK];
#pragma unroll
    for (int c = 0; c < CHUNK; ++c) y[c] = ring[(size_t)c * npix + t] * win[j0 + c];
    const bool fresh = j0 == 0;
    for (int i = 0; i < nb; ++i) {
        const unsigned k = (unsigned)bins[i];
        unsigned m = k * (unsigned)j0 % (unsigned)N;                   // (k <= 32768, j0 < 65536: the product fits 32 bits unsigned)
        const size_t at = (size_t)i * npix + t;
        float re = 0.f, im = 0.f;
        if (!fresh) {
            re = re_p[at];
            im = im_p[at];
        }
#pragma unroll
        for (int c = 0; c < CHUNK; ++c) {
            const float2 w = tw[m];
            re = re + y[c] * w.x;
            im = im + y[c] * w.y;
            m += k;
            if (m >= (unsigned)N) m -= (unsigned)N;
        }
        if (seg_end) {
            P[at] = P[at] + ((re * re) + (im * im));
            re = 0.f;
            im = 0.f;
        }
        re_p[at] = re;
        im_p[at] = im;
    }
}

// The peak maps over the bin positions a <= i <= b, one pixel per thread, one pass over P for kpeak, ppeak and pband and a
// second one over the at most 2 * halfwidth + 1 positions around the peak for pnear (include/fibhip.h has the definition).
__global__ void __launch_bounds__(256) spectrum_peak_kernel(const float *__restrict__ P, size_t npix, int a, int b, int halfwidth, int have,
                                                            int *__restrict__ kpeak, float *__restrict__ ppeak, float *__restrict__ pband,
                                                            float *__restrict__ pnear)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix) return;
    int kp = -1;
    float best = __builtin_nanf(""), band = 0.f;
    for (int i = a; i <= b; ++i) {
        const float p = P[(size_t)i * npix + t];
        band = i == a ? p : band + p;
        if (have && (kp < 0 ? p == p : p > best)) {
            best = p;
            kp = i;
        }
    }
    float near = __builtin_nanf("");
    if (kp >= 0) {
        const int lo = kp - halfwidth > a ? kp - halfwidth : a, hi = kp + halfwidth < b ? kp + halfwidth : b;
        for (int i = lo; i <= hi; ++i) {
            const float p = P[(size_t)i * npix + t];
            near = i == lo ? p : near + p;
        }
    }
    kpeak[t] = kp;
    ppeak[t] = best;
    pband[t] = band;
    pnear[t] = near;
}

// ---- beat recorder (fibhip_beats_begin): a per-pixel history of the last `depth` beats ------------------------------------------
// Two kernels.  beat_kernel, behind a sample tick, forms the pixel xc — the frame recorder's pixel at lo = 0, span = 1, the one
// spectrum_sample_kernel takes — and compares it with the pixel of the previous sample, xp (the recorder's own plane):
//   upstroke   xp < up && xc >= up:                 a beat still open (pk a number) leaves peak[(n - 1) % depth] = pk; then
//                                                   t = t0 + ((up - xp) / (xc - xp)) * step; slot n % depth gets t_up = t,
//                                                   t_down = NaN, peak = NaN; pk = xc; n += 1
//   downstroke xp >= down && xc < down, pk a number: t = t0 + ((xp - down) / (xp - xc)) * step; slot (n - 1) % depth gets
//                                                   t_down = t, peak = pk; pk = NaN
//   otherwise, pk a number:                         pk = xc > pk ? xc : pk
// and then xp = xc.  float32, every operation rounded on its own (-ffp-contract=off, IEEE division); NaN compares false: no
// event, and pk stays.  The ring planes t_up, t_down, peak are [depth][oh * ow] and touched only where an event happens; the slot
// is formed per lane inside the event branches.  The steady traffic at full resolution is x read, xp and pk read and written:
// 20 bytes per pixel.  beat_summary_kernel makes the four summary maps from the ring on demand.  No LDS, no atomics.
// The recorder accumulates (n, pk, the ring), so beat_kernel reads the give-up word of the multi-tick launches first (`give_up`,
// null behind plain ticks: stim_kernel's note) and writes NOTHING when it is raised, like spectrum_sample_kernel: recover()
// rewinds the host's tick counter and the replay takes the lost samples again, in order, from good state.
#define BEAT_MAX_DEPTH 16
struct BeatArgs {
    const float *x;         // the watched array (its first row), `pitch` floats between rows
    const float *w;         // the weight plane [H][W] (wpitch floats between rows), or null
    float *xp, *pk;         // [oh * ow] each
    int *n;                 // [oh * ow]
    float *t_up, *t_down, *peak;    // [depth][oh * ow] each
    int pitch, wpitch;
    int r0, c0, oh, ow, by, bx;
    int depth;
    int init;               // 1: the launch of beats_begin — xp = the pixel of the current state, nothing else
    float up, down, t0, step;
    const unsigned *give_up;
};

// the events of pixel i; returns the new pk
static FIB_DEV float beat_events(float xp, float xc, float pk, size_t i, const BeatArgs &a)
{
    const bool open = pk == pk;
    const size_t npix = (size_t)a.oh * (size_t)a.ow;
    if (xp < a.up && xc >= a.up) {
        const int n = a.n[i];
        if (open) a.peak[(size_t)((n - 1) % a.depth) * npix + i] = pk;        // (open: n >= 1)
        const float t = a.t0 + ((a.up - xp) / (xc - xp)) * a.step;
        const size_t at = (size_t)(n % a.depth) * npix + i;
        a.t_up[at] = t;
        a.t_down[at] = __builtin_nanf("");
        a.peak[at] = __builtin_nanf("");
        a.n[i] = n + 1;
        return xc;
    }
    if (xp >= a.down && xc < a.down && open) {
        const float t = a.t0 + ((xp - a.down) / (xp - xc)) * a.step;
        const size_t at = (size_t)((a.n[i] - 1) % a.depth) * npix + i;
        a.t_down[at] = t;
        a.peak[at] = pk;
        return __builtin_nanf("");
    }
    if (open) return xc > pk ? xc : pk;
    return pk;
}

// One pixel per thread, frame_kernel's scalar path at lo = 0, span = 1 (the subtraction and the division are kept: a pixel is
// the frame recorder's bit for bit); VEC (planar slab, full resolution, every row of the window 16-byte aligned in the array,
// the weight plane and the recorder's planes): four consecutive pixels per thread — x, xp and pk one 16-byte load each, xp and
// pk one 16-byte store each —, the events per lane behind that, as in observe_kernel (a block of one cell: MEAN divides by
// 1.0f, which changes nothing).
template <bool MEAN, bool VEC>
__global__ void __launch_bounds__(256) beat_kernel(BeatArgs a)
{
    if (a.give_up && *a.give_up != 0u) return;                        // (wave-uniform: one scalar load)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {                                                        // by == bx == 1
        const size_t ow4 = (size_t)a.ow / 4;
        if (t >= (size_t)a.oh * ow4) return;
        const size_t oy = t / ow4, g = t % ow4;
        const size_t row = (size_t)a.r0 + oy, col = (size_t)a.c0 + 4 * g;
        const fib_v4f v = *reinterpret_cast<const fib_v4f *>(a.x + row * (size_t)a.pitch + col);
        fib_v4f xc;
#pragma unroll
        for (int e = 0; e < 4; ++e) xc[e] = frame_cell(v[e], 0.f, 1.f);
        if (a.w) {
            const fib_v4f wv = *reinterpret_cast<const fib_v4f *>(a.w + row * (size_t)a.wpitch + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) xc[e] = xc[e] * wv[e];
        }
        const size_t i0 = oy * (size_t)a.ow + 4 * g;
        if (a.init) {
            *reinterpret_cast<fib_v4f *>(a.xp + i0) = xc;
            return;
        }
        const fib_v4f xp = *reinterpret_cast<const fib_v4f *>(a.xp + i0);
        fib_v4f pk = *reinterpret_cast<const fib_v4f *>(a.pk + i0);
        *reinterpret_cast<fib_v4f *>(a.xp + i0) = xc;
#pragma unroll
        for (int e = 0; e < 4; ++e) pk[e] = beat_events(xp[e], xc[e], pk[e], i0 + (size_t)e, a);
        *reinterpret_cast<fib_v4f *>(a.pk + i0) = pk;
    } else {
        if (t >= (size_t)a.oh * (size_t)a.ow) return;
        const size_t oy = t / (size_t)a.ow, ox = t % (size_t)a.ow;
        const size_t row0 = (size_t)a.r0 + oy * (size_t)a.by, col0 = (size_t)a.c0 + ox * (size_t)a.bx;
        float xc = 0.f;
        if (!MEAN) {
            xc = frame_cell(a.x[row0 * (size_t)a.pitch + col0], 0.f, 1.f);
            if (a.w) xc = xc * a.w[row0 * (size_t)a.wpitch + col0];
        } else {
            const float n_cells = (float)(a.by * a.bx);
            for (int dy = 0; dy < a.by; ++dy) {
                const size_t xr = (row0 + (size_t)dy) * (size_t)a.pitch + col0, wr = (row0 + (size_t)dy) * (size_t)a.wpitch + col0;
                float rs = 0.f;
                for (int dx = 0; dx < a.bx; ++dx) {
                    float y = frame_cell(a.x[xr + (size_t)dx], 0.f, 1.f);
                    if (a.w) y = y * a.w[wr + (size_t)dx];
                    rs = dx == 0 ? y : rs + y;
                }
                xc = dy == 0 ? rs : xc + rs;
            }
            xc = xc / n_cells;
        }
        if (a.init) {
            a.xp[t] = xc;
            return;
        }
        const float xp = a.xp[t];
        a.xp[t] = xc;
        a.pk[t] = beat_events(xp, xc, a.pk[t], t, a);
    }
}

// The summary maps of the newest `last` beats, one pixel per thread (include/fibhip.h has the definition): a walk over the beats
// b0 .. n - 1 for nused, apd_mean and apd_alt, a second one for cl_mean; at most BEAT_MAX_DEPTH ring entries each.
__global__ void __launch_bounds__(256)
beat_summary_kernel(const int *__restrict__ count, const float *__restrict__ t_up, const float *__restrict__ t_down, size_t npix, int depth,
                    int last, int *__restrict__ nused, float *__restrict__ apd_mean, float *__restrict__ cl_mean, float *__restrict__ apd_alt)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix) return;
    const int n = count[t];
    const int held = n < depth ? n : depth;
    int b0 = n - held > n - last ? n - held : n - last;
    if (b0 < 0) b0 = 0;
    int used = 0, pairs = 0;
    float sum = 0.f, alt = 0.f, before = __builtin_nanf("");          // `before`: the APD of beat b - 1 (NaN: none in the walk)
    for (int b = b0; b < n; ++b) {
        const size_t at = (size_t)(b % depth) * npix + t;
        const float apd = t_down[at] - t_up[at];
        if (apd == apd) {
            sum = used == 0 ? apd : sum + apd;
            used++;
            if (before == before) {
                const float d = apd - before;
                const float term = (b & 1) ? d : -d;
                alt = pairs == 0 ? term : alt + term;
                pairs++;
            }
        }
        before = apd;
    }
    int ncl = 0;
    float cls = 0.f;
    for (int b = b0 + 1; b < n; ++b) {
        const float cl = t_up[(size_t)(b % depth) * npix + t] - t_up[(size_t)((b - 1) % depth) * npix + t];
        if (cl == cl) {
            cls = ncl == 0 ? cl : cls + cl;
            ncl++;
        }
    }
    nused[t] = used;
    apd_mean[t] = used ? sum / (float)used : __builtin_nanf("");
    cl_mean[t] = ncl ? cls / (float)ncl : __builtin_nanf("");
    apd_alt[t] = pairs ? alt / (float)pairs : __builtin_nanf("");
}

// ---- velocity fit (fibhip_beats_velocity, fibhip_observe_velocity, fibhip_velocity_fit): a plane fitted to the activation times
// in a space-time window around every pixel (include/fibhip.h has the definition).  Launched at read time on a ring of time
// planes t[depth][oh * ow] with its count plane, like beat_summary_kernel; one pixel per thread.
//   velocity_fit_kernel, grid (ceil(ow / VEL_TX), ceil(oh / VEL_TY)), 256 threads: a workgroup stages its tile with a ring of R
//   pixels in LDS — one word per cell that packs how many beats the cell holds and the slot of the oldest (0 beats for a cell
//   outside the plane or the mask: it then takes no part, and as a centre it has no beat), and the held slots of its ring; wave v
//   stages the rows v, v + 4, ..., lane l the column l: consecutive lanes, consecutive words, in global memory and in LDS, and
//   the one modulo by `depth` of a cell is taken here —, then walks the window from LDS.  The 32 lanes that share the banks of a
//   4-byte LDS read are one row of the tile, consecutive words; a slot's stride, 640 words, is a multiple of the 32 banks, so
//   lanes that stand at different slots of neighbouring cells (their counts differ) still hit different banks.
// `depth` and R are run-time values: the ten sums live in registers and nothing is indexed with a run-time index (no scratch).
// The obvious form — every ring entry of the window straight from L2 — was measured beside this one on the MI355X and is not
// kept: 46.2 against 43.7 us at 512 x 512, depth 8, R = 2; 2294 against 1390 us at 2048 x 2048, R = 4 (profiles/velocity_cost.txt).
// The float64 arithmetic is written one operation per statement where the order matters; -ffp-contract=off keeps it so.
#define VEL_MAX_RADIUS 4        // FIBHIP_VEL_MAX_RADIUS
#define VEL_TX 32
#define VEL_TY 8
#define VEL_LW (VEL_TX + 2 * VEL_MAX_RADIUS)
#define VEL_LH (VEL_TY + 2 * VEL_MAX_RADIUS)
#define VEL_CELLS (VEL_LW * VEL_LH)             // 640 words per slot: 16 slots and the packed counts are 43520 bytes
struct VelArgs {
    const float *t;             // [depth][oh * ow]
    const int *n;               // [oh * ow]
    const unsigned char *mask;  // [oh * ow], or null (every pixel counts)
    int depth, oh, ow;
    int back, radius, min_cells;
    float max_dt;
    int *nfit;                  // [oh * ow] each
    float *gy, *gx, *rms;
};

// the sums over the used cells of one window, and the solve
struct VelSums {
    int N, Sy, Sx, Syy, Sxx, Sxy;
    double St, Syt, Sxt, Stt;
    FIB_DEV void clear() { N = Sy = Sx = Syy = Sxx = Sxy = 0; St = Syt = Sxt = Stt = 0.0; }
    FIB_DEV void add(int dy, int dx, float d)
    {
        const double dd = (double)d;
        N += 1;
        Sy += dy; Sx += dx;
        Syy += dy * dy; Sxx += dx * dx; Sxy += dy * dx;
        St = St + dd;
        Syt = Syt + (double)dy * dd;
        Sxt = Sxt + (double)dx * dd;
        Stt = Stt + dd * dd;
    }
};

static FIB_DEV void vel_store(const VelArgs &a, size_t p, const VelSums &s)
{
    const float nanf_ = __builtin_nanf("");
    float gy = nanf_, gx = nanf_, rms = nanf_;
    const long long N = s.N, Sy = s.Sy, Sx = s.Sx;
    const long long cyy = N * s.Syy - Sy * Sy, cxx = N * s.Sxx - Sx * Sx, cxy = N * s.Sxy - Sy * Sx;
    const long long det = cyy * cxx - cxy * cxy;
    if (s.N >= a.min_cells && det != 0) {
        const double n = (double)N;
        const double cyt = n * s.Syt - (double)Sy * s.St;
        const double cxt = n * s.Sxt - (double)Sx * s.St;
        const double g_y = ((double)cxx * cyt - (double)cxy * cxt) / (double)det;
        const double g_x = ((double)cyy * cxt - (double)cxy * cyt) / (double)det;
        const double c = (s.St - (g_y * (double)Sy + g_x * (double)Sx)) / n;
        const double sse = s.Stt - ((c * s.St + g_y * s.Syt) + g_x * s.Sxt);
        const double r = __dsqrt_rn((sse > 0.0 ? sse : 0.0) / n);
        gy = (float)g_y; gx = (float)g_x; rms = (float)r;
    }
    if (a.nfit) a.nfit[p] = s.N;
    if (a.gy) a.gy[p] = gy;
    if (a.gx) a.gx[p] = gx;
    if (a.rms) a.rms[p] = rms;
}

__global__ void __launch_bounds__(256) velocity_fit_kernel(VelArgs a)
{
    __shared__ float ts[BEAT_MAX_DEPTH * VEL_CELLS];
    __shared__ int ns[VEL_CELLS];                                     // held beats | slot of the oldest << 8
    const int R = a.radius, depth = a.depth;
    const int lw = VEL_TX + 2 * R, lh = VEL_TY + 2 * R;               // <= VEL_LW, VEL_LH: the host refuses R > VEL_MAX_RADIUS
    const int x0 = (int)blockIdx.x * VEL_TX - R, y0 = (int)blockIdx.y * VEL_TY - R;
    const size_t npix = (size_t)a.oh * (size_t)a.ow;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane < lw) {
        for (int r = wv; r < lh; r += 4) {
            const int y = y0 + r, x = x0 + lane;
            const int cell = r * VEL_LW + lane;
            int held = 0, first = 0;
            if (y >= 0 && y < a.oh && x >= 0 && x < a.ow) {
                const size_t q = (size_t)y * (size_t)a.ow + (size_t)x;
                const int n = (!a.mask || a.mask[q]) ? a.n[q] : 0;
                if (n > 0) {
                    held = n < depth ? n : depth;
                    first = n < depth ? 0 : n % depth;                // (n - held) % depth
                    for (int s = 0; s < held; ++s) ts[s * VEL_CELLS + cell] = a.t[(size_t)s * npix + q];
                }
            }
            ns[cell] = held | (first << 8);
        }
    }
    __syncthreads();
    const int tx = threadIdx.x & (VEL_TX - 1), ty = threadIdx.x / VEL_TX;
    const int x = (int)blockIdx.x * VEL_TX + tx, y = (int)blockIdx.y * VEL_TY + ty;
    if (x >= a.ow || y >= a.oh) return;
    const size_t p = (size_t)y * (size_t)a.ow + (size_t)x;
    const int c = (ty + R) * VEL_LW + tx + R;
    VelSums s;
    s.clear();
    const int nc = ns[c], heldc = nc & 255;
    float tc = __builtin_nanf("");
    if (a.back < heldc) {                                             // beat n - 1 - back is held
        int slot = (nc >> 8) + heldc - 1 - a.back;                    // < 2 * depth
        if (slot >= depth) slot -= depth;
        tc = ts[slot * VEL_CELLS + c];
    }
    if (tc == tc) {
        for (int dy = -R; dy <= R; ++dy) {
            for (int dx = -R; dx <= R; ++dx) {
                const int cell = c + dy * VEL_LW + dx;
                const int nq = ns[cell], held = nq & 255;
                int slot = nq >> 8;
                float best = __builtin_inff(), bd = 0.f;
                for (int j = 0; j < held; ++j) {                      // ascending beat number; a tie keeps the older beat
                    const float d = ts[slot * VEL_CELLS + cell] - tc;
                    const float ad = __builtin_fabsf(d);
                    if (ad < best) { best = ad; bd = d; }             // (a NaN compares false)
                    slot = slot + 1 == depth ? 0 : slot + 1;
                }
                if (best <= a.max_dt) s.add(dy, dx, bd);              // (max_dt is finite: nothing kept, nothing used)
            }
        }
    }
    vel_store(a, p, s);
}

// ---- lead recorder (fibhip_leads_begin): unipolar electrograms, the membrane current seen through a lead field ---------------
// The SOURCE at an interior cell (1 <= r <= H - 2, 1 <= c <= W - 2) of the watched array X is the stand-alone laplace() of
// the boundary-enforced array: stencil9 over taps read at (clamp(r + dr, 1, H - 2), clamp(c + dc, 1, W - 2)) — tick_kernel's
// rule —, plus phase_term<Exact> from the prepared dpy, dpx, q4, r4 where the handle has a phase field.  Always the exact form,
// whatever the handle's policy, float32, every operation rounded on its own (-ffp-contract=off).  q = w * S is one more float32
// product (no plane: q = S); the outer ring of the grid holds ghost copies and contributes nothing.  Lead e sits at cell (re, ce)
// and names a table T: its weight of cell (r, c) is T[|r - re|][|c - ce|], its term (double)T * (double)q — exact, the product
// of two float32 — and its sample the float64 sum of the terms, every addition rounded on its own (no fma), in an order fixed
// by H and W alone:
//   lead_kernel, grid (ceil(W / LD_TX), ceil(H / LD_TY)), LD_THREADS threads: a workgroup stages its tile of X with a one-cell
//   ring in LDS through the clamp (consecutive lanes, consecutive words: conflict-free for all nine taps) and lane l of wave v
//   forms q ONCE for the cells (row v + 4j, column l) of the tile, j = 0 .. LD_CPT - 1, in registers.  Then the leads in groups
//   of LD_GROUP: the group's float64 accumulators are addressed by fully unrolled loops only (a run-time index would put them
//   in scratch: frame_kernel's note), a lead's cell and table are wave-uniform (scalar loads), the group's table loads are
//   issued together in front of its arithmetic (a slot beyond the last lead repeats the last lead and is dropped), and a
//   wave's table loads for one row of cells are consecutive addresses, ascending or descending.  A thread adds its cells in the
//   order of j; then six shuffle levels in each wave (lead_group_sum: the group's eight sums as one butterfly, a fixed tree per
//   lead), the wave sums through LDS, (w0 + w1) + (w2 + w3) by one thread
//   per lead, and ONE plain 64-bit store per (lead, tile) into part[lead][tile].  X, the weight plane and the phase arrays are
//   read once per sample however many leads there are.
//   lead_combine_kernel, one workgroup per lead, a second launch on the same stream: thread t adds the tiles t, t + 256, ...
//   in that order (any tile count), then the same wave and workgroup tree, and writes the lead's entry of the sample's row.
// A cell outside the interior adds the term +0.0 (its table address is clamped into the table).  No atomics of any kind.
#define LD_TX 64
#define LD_TY 16
#define LD_THREADS 256
#define LD_CPT (LD_TY / (LD_THREADS / 64))      // cells per thread
#define LD_GROUP 8
#define LD_MAX 64               // leads (FIBHIP_MAX_LEADS)
struct LeadArgs {
    const float *x;             // the watched array (its first row), `pitch` floats between rows
    const float *w;             // the weight plane [H][W], or null
    const float *dpy, *dpx, *q4, *r4;   // the prepared phase arrays [H][W], or all null: no phase field
    const int *pos;             // [n][4] = row, col, table, 0
    const float *tables;        // [ntables][H][W]
    double *part;               // [n][tiles]
    int H, W, pitch, n;
};

// q of one interior cell, what lead_kernel and pmap_source_kernel share: `t` points at the cell's word of an LDS tile of X that
// has its one-cell ring staged through the clamp, LP floats per row; `o` is the cell's index r * W + c in the [H][W] planes
template <int LP>
static FIB_DEV float membrane_source(const float *t, size_t o, const float *w, const float *dpy, const float *dpx, const float *q4, const float *r4)
{
    const float N = t[-LP], S = t[LP], Wv = t[-1], E = t[1];
    float s = stencil9(N, S, Wv, E, t[-LP - 1], t[LP - 1], t[-LP + 1], t[LP + 1], t[0]);
    if (dpy) s = s + phase_term<Exact>(N, S, Wv, E, dpy[o], dpx[o], q4[o], r4[o]);
    return w ? w[o] * s : s;
}

static FIB_DEV double lead_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

// The LD_GROUP = 8 sums of a group over the 64 lanes of a wave as ONE butterfly: at the levels 32, 16 and 8 a lane hands the half
// of its values its partner keeps to that partner (lane ^ level) and adds what it receives to the half it keeps — 4, 2 and 1
// shuffles instead of 8 each —, after which it holds one value, that of slot 4 * bit 5 + 2 * bit 4 + bit 3 of its lane number
// (returned); the levels 4, 2 and 1 finish that one.  Which value a lane keeps is a select, never a run-time index.  Every
// slot's sum is the same tree — pairs 32 apart, then 16, 8, 4, 2, 1 — and IEEE addition commutes, so a lead's sum does not
// depend on the slot it has in its group: its bits are those of the six plain levels over (lane, lane ^ level).  The sum is
// left in acc[0] of the lanes that hold the slot.
static FIB_DEV int lead_group_sum(double (&acc)[LD_GROUP], int lane)
{
    static_assert(LD_GROUP == 8, "three halving levels");
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double keep = b5 ? acc[i + 4] : acc[i], send = b5 ? acc[i] : acc[i + 4];
        acc[i] = keep + __shfl_xor(send, 32, 64);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double keep = b4 ? acc[i + 2] : acc[i], send = b4 ? acc[i] : acc[i + 2];
        acc[i] = keep + __shfl_xor(send, 16, 64);
    }
    {
        const double keep = b3 ? acc[1] : acc[0], send = b3 ? acc[0] : acc[1];
        acc[0] = keep + __shfl_xor(send, 8, 64);
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) acc[0] = acc[0] + __shfl_xor(acc[0], off, 64);
    return (b5 ? 4 : 0) + (b4 ? 2 : 0) + (b3 ? 1 : 0);
}

__global__ void __launch_bounds__(LD_THREADS) lead_kernel(LeadArgs a)
{
    constexpr int LP = LD_TX + 2, LQ = LD_TY + 2, NW = LD_THREADS / 64;
    __shared__ float tile[LQ * LP];
    __shared__ double wres[NW][LD_MAX];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)blockIdx.x * LD_TX, y0 = (int)blockIdx.y * LD_TY;
    const int H = a.H, W = a.W;
    for (int i = tid; i < LQ * LP; i += LD_THREADS) {
        const int ly = i / LP, lx = i - ly * LP;
        const int yy = clampi(y0 - 1 + ly, 1, H - 2), xx = clampi(x0 - 1 + lx, 1, W - 2);
        tile[i] = a.x[(size_t)yy * (size_t)a.pitch + (size_t)xx];
    }
    __syncthreads();
    const int c = x0 + lane;
    const int ca = min(c, W - 1);                                    // (the column a table address is formed from)
    float q[LD_CPT];
    int ra[LD_CPT];
#pragma unroll
    for (int j = 0; j < LD_CPT; ++j) {
        const int ly = wave + NW * j, r = y0 + ly;
        ra[j] = min(r, H - 1);
        q[j] = 0.f;
        if (r >= 1 && r <= H - 2 && c >= 1 && c <= W - 2) {
            q[j] = membrane_source<LP>(tile + (ly + 1) * LP + lane + 1, (size_t)r * (size_t)W + (size_t)c, a.w, a.dpy, a.dpx, a.q4, a.r4);
        }
    }
    const size_t cells = (size_t)H * (size_t)W;
    for (int g0 = 0; g0 < a.n; g0 += LD_GROUP) {
        // all of the group's table loads first, with no branch between them, so that they are in flight together; a slot beyond
        // the last lead repeats the last lead (the same addresses once more) and its sum is dropped
        float k[LD_GROUP][LD_CPT];
#pragma unroll
        for (int e = 0; e < LD_GROUP; ++e) {
            const int *__restrict__ p = a.pos + 4 * min(g0 + e, a.n - 1);
            const int re = p[0], ce = p[1];
            const float *__restrict__ T = a.tables + (size_t)p[2] * cells + (size_t)__builtin_abs(ca - ce);
#pragma unroll
            for (int j = 0; j < LD_CPT; ++j) k[e][j] = T[(size_t)__builtin_abs(ra[j] - re) * (size_t)W];
        }
        double acc[LD_GROUP];
#pragma unroll
        for (int e = 0; e < LD_GROUP; ++e) {
            acc[e] = 0.0;
#pragma unroll
            for (int j = 0; j < LD_CPT; ++j) acc[e] = acc[e] + (double)k[e][j] * (double)q[j];
        }
        const int e = lead_group_sum(acc, lane);
        if ((lane & 7) == 0 && g0 + e < a.n) wres[wave][g0 + e] = acc[0];
    }
    __syncthreads();
    if (tid < a.n) {
        const double v = (wres[0][tid] + wres[1][tid]) + (wres[2][tid] + wres[3][tid]);
        a.part[(size_t)tid * ((size_t)gridDim.x * gridDim.y) + ((size_t)blockIdx.y * gridDim.x + blockIdx.x)] = v;
    }
}

__global__ void __launch_bounds__(256) lead_combine_kernel(const double *__restrict__ part, int ntiles, double *__restrict__ row)
{
    __shared__ double wres[4];
    const double *__restrict__ p = part + (size_t)blockIdx.x * (size_t)ntiles;
    double v = 0.0;
    for (int t = (int)threadIdx.x; t < ntiles; t += 256) v = v + p[t];
    v = lead_wave_sum(v);
    if ((threadIdx.x & 63u) == 0) wres[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) row[blockIdx.x] = (wres[0] + wres[1]) + (wres[2] + wres[3]);
}

// ---- potential-map recorder (fibhip_pmap_begin): the unipolar electrogram at every site of a lattice -----------------------
// The source plane q is the lead recorder's (membrane_source on the interior cells, +0.0 on the outer ring).  Site (i, j) of the
// lattice sits at the cell (r, c) = (r0 + i * sy, c0 + j * sx); its value is the truncated convolution of q with the table
// T[R + 1][R + 1], summed in float64 in an order that R alone fixes:
//     phi = +0.0;  for dr = -R .. R:  p = +0.0;  for dc = -R .. R:  p = fma((double)T[|dr|][|dc|], (double)q[r + dr][c + dc], p);
//                                     phi = phi + p
// with q = +0.0 off the grid.  The product of two float32 values is exact in float64, so the fma rounds what multiply-then-add
// rounds: the same bits.  Three kernels:
//   pmap_source_kernel, lead_kernel's grid and tile: writes q of every cell of the grid into a scratch plane that carries R
//     zeros on every side (zeroed at attach, never written), cell (r, c) at (r + R, c + R): the window of a site at (r, c)
//     starts at (r, c) of the padded plane and the convolution needs no bounds logic on the grid.
//   pmap_conv_kernel, a workgroup of 4, 2 or 1 waves (the host's choice: more workgroups for a small lattice; the sums do not
//     depend on it) owns a tile of PM_TX x (PM_SPL * waves) sites: lane l of wave v owns the sites (row PM_SPL * v + j, column
//     l) of the tile, j = 0 .. PM_SPL - 1, one float64 accumulator each.  The q rows the tile needs —
//     its span plus 2R — are staged in LDS in slabs of as many rows as PM_LDS_FLOATS hold (step 1: the whole span at any
//     radius, 80 x 128 floats at R = 32), ascending, so every site meets its rows in the order of dr.  A row is stored
//     de-interleaved by the column step: column x of the span at (x % sx) * pw + x / sx, so that for every tap the 64 lanes
//     read 64 consecutive words whatever the step — no bank conflict.  For a q row that all PM_SPL sites of the lane use (at
//     step 1 and R = 32: 62 of a wave's 68 rows) one LDS word and one conversion serve PM_SPL fmas on independent chains;
//     a row that only some use is walked site by site.  Which sites a row serves, the table row of each and the LDS address
//     are wave-uniform: the table (float64, expanded to [R + 1][2R + 1] at attach) comes through scalar loads.  Plain 64-bit
//     stores into the sample's slot; no atomics.
//   pmap_summary_kernel, one thread per site, at read time on the cube where it lies: walks the samples [first, first + count).
#define PM_TX 64
#define PM_TY 16
#define PM_THREADS 256
#define PM_SPL (PM_TY / (PM_THREADS / 64))      // sites per lane
#define PM_MAX_RADIUS 32        // FIBHIP_PMAP_MAX_RADIUS
#define PM_MAX_STEP 16          // FIBHIP_PMAP_MAX_STEP
#define PM_LDS_FLOATS (80 * 128)
struct PMapSourceArgs {
    const float *x;             // the watched array (its first row), `pitch` floats between rows
    const float *w;             // the weight plane [H][W], or null
    const float *dpy, *dpx, *q4, *r4;   // the prepared phase arrays [H][W], or all null: no phase field
    float *q;                   // the padded plane [H + 2R][W + 2R]
    int H, W, pitch, R;
};
struct PMapArgs {
    const float *q;             // the padded plane [qh][qw]
    const double *tab;          // [R + 1][2R + 1]: tab[a][x] = (double)T[a][|x - R|]
    double *out;                // the sample's slot [oh][ow]
    int R, r0, c0, sy, sx, oh, ow, qh, qw;
    int pw, roww, slab;         // the LDS layout: words per phase of a row, words per row (sx * pw), rows per slab
};
struct PMapSummaryArgs {
    const double *cube;         // [samples][npix]
    size_t npix;
    int first, count;           // count >= 2
    double *vmin, *vmax, *dmin; // [npix] each
    int *kmin, *kmax, *kd;
};

__global__ void __launch_bounds__(LD_THREADS) pmap_source_kernel(PMapSourceArgs a)
{
    constexpr int LP = LD_TX + 2, LQ = LD_TY + 2, NW = LD_THREADS / 64;
    __shared__ float tile[LQ * LP];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)blockIdx.x * LD_TX, y0 = (int)blockIdx.y * LD_TY;
    const int H = a.H, W = a.W;
    for (int i = tid; i < LQ * LP; i += LD_THREADS) {
        const int ly = i / LP, lx = i - ly * LP;
        const int yy = clampi(y0 - 1 + ly, 1, H - 2), xx = clampi(x0 - 1 + lx, 1, W - 2);
        tile[i] = a.x[(size_t)yy * (size_t)a.pitch + (size_t)xx];
    }
    __syncthreads();
    const int c = x0 + lane;
    const size_t qw = (size_t)W + 2 * (size_t)a.R;
#pragma unroll
    for (int j = 0; j < LD_CPT; ++j) {
        const int ly = wave + NW * j, r = y0 + ly;
        if (r >= H || c >= W) continue;
        float q = 0.f;
        if (r >= 1 && r <= H - 2 && c >= 1 && c <= W - 2)
            q = membrane_source<LP>(tile + (ly + 1) * LP + lane + 1, (size_t)r * (size_t)W + (size_t)c, a.w, a.dpy, a.dpx, a.q4, a.r4);
        a.q[(size_t)(r + a.R) * qw + (size_t)(c + a.R)] = q;
    }
}

// N taps of one q row for the four sites of a lane: the 4 N table values (wave-uniform: scalar loads) and the N words of the row
// are all asked for in front of the arithmetic, so that one wait covers them — a scalar load per tap, waited for on its own,
// cost the first version of this kernel most of its time.  `x0` is the first tap, (ph, ix) the place of tap x0 in a row that is
// de-interleaved by the column step (UNIT: the step is 1 and the place is x0 itself)
template <int N, bool UNIT>
static FIB_DEV void pmap_taps4(const float *row, const double *__restrict__ t0, const double *__restrict__ t1, const double *__restrict__ t2,
                               const double *__restrict__ t3, int x0, int &ph, int &ix, int sx, int pw, double &p0, double &p1, double &p2,
                               double &p3)
{
    double a0[N], a1[N], a2[N], a3[N];
    float q[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        a0[i] = t0[x0 + i]; a1[i] = t1[x0 + i]; a2[i] = t2[x0 + i]; a3[i] = t3[x0 + i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        q[i] = row[UNIT ? x0 + i : ph * pw + ix];
        if (!UNIT && ++ph == sx) { ph = 0; ++ix; }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double qd = (double)q[i];
        p0 = __builtin_fma(a0[i], qd, p0);
        p1 = __builtin_fma(a1[i], qd, p1);
        p2 = __builtin_fma(a2[i], qd, p2);
        p3 = __builtin_fma(a3[i], qd, p3);
    }
}
// ... and for ONE site of the lane
template <int N, bool UNIT>
static FIB_DEV void pmap_taps1(const float *row, const double *__restrict__ t, int x0, int &ph, int &ix, int sx, int pw, double &p)
{
    double a[N];
    float q[N];
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] = t[x0 + i];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        q[i] = row[UNIT ? x0 + i : ph * pw + ix];
        if (!UNIT && ++ph == sx) { ph = 0; ++ix; }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) p = __builtin_fma(a[i], (double)q[i], p);
}
// one q row for ONE site of the lane: p = the sum over the row's K taps, ascending; `t` is the site's table row (wave-uniform)
template <bool UNIT>
static FIB_DEV double pmap_row1(const float *row, const double *__restrict__ t, int K, int sx, int pw)
{
    double p = 0.0;
    int x = 0, ph = 0, ix = 0;
    for (; x + 16 <= K; x += 16) pmap_taps1<16, UNIT>(row, t, x, ph, ix, sx, pw, p);
    if (x + 8 <= K) { pmap_taps1<8, UNIT>(row, t, x, ph, ix, sx, pw, p); x += 8; }
    if (x + 4 <= K) { pmap_taps1<4, UNIT>(row, t, x, ph, ix, sx, pw, p); x += 4; }
    if (x + 2 <= K) { pmap_taps1<2, UNIT>(row, t, x, ph, ix, sx, pw, p); x += 2; }
    if (x < K) pmap_taps1<1, UNIT>(row, t, x, ph, ix, sx, pw, p);
    return p;
}

template <bool UNIT>
__global__ void __launch_bounds__(PM_THREADS) pmap_conv_kernel(PMapArgs a)
{
    static_assert(PM_SPL == 4, "the shared row below names four sites");
    __shared__ float lds[PM_LDS_FLOATS];
    const int tid = (int)threadIdx.x, lane = tid & 63, threads = (int)blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // (wave-uniform, and known to be)
    const int ty = (threads >> 6) * PM_SPL;                             // site rows of a tile: 4 per wave of the workgroup
    const int R = a.R, K = 2 * R + 1, sy = a.sy, sx = UNIT ? 1 : a.sx, pw = a.pw;
    const int sr0 = (int)blockIdx.y * ty, sc0 = (int)blockIdx.x * PM_TX;         // the tile's first site
    const int py0 = a.r0 + sr0 * sy, px0 = a.c0 + sc0 * sx;                      // where its span starts in the padded plane
    const int span = (min(ty, a.oh - sr0) - 1) * sy + K;                         // q rows the tile needs
    const int width = (PM_TX - 1) * sx + K;                                      // q columns of a full tile
    // the lane's sites: site j's window starts at row top[j] of the span; a site below the lattice's last row is left out
    int top[PM_SPL];
    bool have[PM_SPL];
#pragma unroll
    for (int j = 0; j < PM_SPL; ++j) {
        top[j] = (wave * PM_SPL + j) * sy;
        have[j] = sr0 + wave * PM_SPL + j < a.oh;
    }
    double phi[PM_SPL] = {0.0, 0.0, 0.0, 0.0};
    for (int s0 = 0; s0 < span; s0 += a.slab) {
        const int ns = min(a.slab, span - s0);
        __syncthreads();                                                         // (the slab before has been read)
        // (every load is made from an address clamped into the plane and its value dropped where the cell is outside: with no
        // branch around them, eight loads of a thread are in flight together — one at a time, their latency was the sample's time)
#pragma unroll 8
        for (int i = tid; i < ns * a.roww; i += threads) {
            const int ly = i / a.roww, p = i - ly * a.roww;
            int x = p;
            if (!UNIT) {
                const int ph = p / pw, ix = p - ph * pw;
                x = ix * sx + ph;
            }
            const int gy = py0 + s0 + ly, gx = px0 + x;
            const float v = a.q[(size_t)min(gy, a.qh - 1) * (size_t)a.qw + (size_t)min(gx, a.qw - 1)];
            lds[i] = (x < width && gy < a.qh && gx < a.qw) ? v : 0.f;
        }
        __syncthreads();
        if (!have[0]) continue;                                                  // (a wave with no site of the lattice: it only stages)
        const int ylo = max(s0, top[0]), yhi = min(s0 + ns, top[PM_SPL - 1] + K);
        for (int y = ylo; y < yhi; ++y) {
            const float *row = lds + (y - s0) * a.roww + lane;
            int d[PM_SPL];                                                       // dr + R of this row for site j
            bool act[PM_SPL];
#pragma unroll
            for (int j = 0; j < PM_SPL; ++j) {
                d[j] = y - top[j];
                act[j] = have[j] && d[j] >= 0 && d[j] < K;
            }
            if (act[0] && act[1] && act[2] && act[3]) {
                const double *__restrict__ t0 = a.tab + (size_t)__builtin_abs(d[0] - R) * K;
                const double *__restrict__ t1 = a.tab + (size_t)__builtin_abs(d[1] - R) * K;
                const double *__restrict__ t2 = a.tab + (size_t)__builtin_abs(d[2] - R) * K;
                const double *__restrict__ t3 = a.tab + (size_t)__builtin_abs(d[3] - R) * K;
                double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
                int x = 0, ph = 0, ix = 0;
                for (; x + 8 <= K; x += 8) pmap_taps4<8, UNIT>(row, t0, t1, t2, t3, x, ph, ix, sx, pw, p0, p1, p2, p3);
                if (x + 4 <= K) { pmap_taps4<4, UNIT>(row, t0, t1, t2, t3, x, ph, ix, sx, pw, p0, p1, p2, p3); x += 4; }
                if (x + 2 <= K) { pmap_taps4<2, UNIT>(row, t0, t1, t2, t3, x, ph, ix, sx, pw, p0, p1, p2, p3); x += 2; }
                if (x < K) pmap_taps4<1, UNIT>(row, t0, t1, t2, t3, x, ph, ix, sx, pw, p0, p1, p2, p3);
                phi[0] = phi[0] + p0;
                phi[1] = phi[1] + p1;
                phi[2] = phi[2] + p2;
                phi[3] = phi[3] + p3;
            } else {
#pragma unroll
                for (int j = 0; j < PM_SPL; ++j)
                    if (act[j]) phi[j] = phi[j] + pmap_row1<UNIT>(row, a.tab + (size_t)__builtin_abs(d[j] - R) * K, K, sx, pw);
            }
        }
    }
    const int sc = sc0 + lane;
    if (sc < a.ow) {
#pragma unroll
        for (int j = 0; j < PM_SPL; ++j) {
            const int sr = sr0 + wave * PM_SPL + j;
            if (sr < a.oh) a.out[(size_t)sr * (size_t)a.ow + (size_t)sc] = phi[j];
        }
    }
}

__global__ void __launch_bounds__(256) pmap_summary_kernel(PMapSummaryArgs a)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.npix) return;
    const double *__restrict__ c = a.cube + (size_t)a.first * a.npix + p;
    double prev = c[0], lo = prev, hi = prev, dm = 0.0;
    int klo = a.first, khi = a.first, kd = a.first + 1;
    for (int s = 1; s < a.count; ++s) {
        const double v = c[(size_t)s * a.npix];
        if (v < lo) { lo = v; klo = a.first + s; }
        if (v > hi) { hi = v; khi = a.first + s; }
        const double d = v - prev;
        if (s == 1 || d < dm) { dm = d; kd = a.first + s; }
        prev = v;
    }
    a.vmin[p] = lo; a.vmax[p] = hi; a.dmin[p] = dm;
    a.kmin[p] = klo; a.kmax[p] = khi; a.kd[p] = kd;
}

// ---- wave recorder (fibhip_waves_begin): connected components of the cells that meet a condition -------------------------
// A cell is SET when its mask byte is non-zero (no mask: every cell) and X > level (kind 0) or X < level (kind 1) holds on the
// watched array, and on the second array with its own kind and level where there is one: strict float32 compares, a NaN is never
// set.  Set cells that touch under conn = 4 or 8 form a WAVE; its SEED is the smallest linear index r * W + c among its cells.
// Four kernels on one stream per sample, behind a 12-byte memset of the sample's counts {n, stored, cells}; everything is integer
// arithmetic and the only thing the order of arrival decides is the order of the records:
//   wave_label_kernel  one workgroup per tile of WV_TX x WV_TY cells, lane l of wave v owns the cells (row v + 4j, column l) of the
//     tile (lead_kernel's ownership), so a tile row is one ballot.  `cells` takes one atomicAdd per wave that has set cells.  In
//     LDS every set cell starts as the child of the first cell of its horizontal RUN (from the ballot, no union), then the runs
//     of consecutive rows are united where they touch — one union per contact, not per cell: a cell whose left, upper-left and
//     upper neighbours are all set leaves its upper contact to its left neighbour — by the lock-free union below on LDS.  Behind
//     a barrier every cell of the tile inside the grid writes the global label plane: the global linear index of its local
//     root (local and global order agree inside a tile, so that is the smallest index of its local component), or -1.
//   wave_merge_kernel  one thread per cell of a tile's top row and per cell of a tile's left column (no tile border: not
//     launched): a set cell is united with its set neighbours across the border — above, and under conn = 8 above-left and
//     above-right, for a top row; left, and under conn = 8 above-left and below-left, for a left column; between them these are
//     all pairs of neighbours in different tiles, the two diagonals across a tile corner included — on the global plane.
//   wave_root_kernel   one thread per cell: a set cell replaces its label by its root.  A cell that is its own root takes a slot
//     (one atomicAdd on `n` per wave of the GPU that has roots), writes it into the slot plane — written by roots, read at
//     roots' entries only — and, if the slot is below max_waves, counts itself in `stored` and initialises its record.
//   wave_reduce_kernel one thread per cell: a set cell whose root's slot is below max_waves adds itself to that record, area by
//     a 32-bit atomicAdd, the row and column sums by 64-bit atomicAdds, the box by atomicMin / atomicMax.  Where the contributing
//     lanes of a wave of the GPU all name ONE slot (inside a large domain: always) they are reduced across the wave first and one
//     lane issues the seven atomics.
// The union (wave_unite): find both roots, hang the larger under the smaller with atomicMin, and where the atomicMin met a label
// that was no longer a root go on from what it returned.  A label never exceeds its cell's index, so every path descends and
// every loop is bounded by the plane; no kernel waits for another workgroup, and each ends whatever the state holds.  Linear
// indices are int32 (H * W < 2^31); offsets into the state are size_t.
#define WV_TX 64
#define WV_TY 16
#define WV_THREADS 256
#define WV_CPT (WV_TY / (WV_THREADS / 64))      // cells per thread
struct WaveRecord {             // fibhip_wave_record
    int seed, area;
    long long sum_r, sum_c;
    int r0, r1, c0, c1;
};
struct WaveArgs {
    const float *x, *x2;        // the watched arrays (their first rows), `pitch` floats between rows; x2 null: one condition
    const unsigned char *mask;  // [H][W], or null
    int *labels;                // [H][W]
    int *cnt;                   // this sample's {n, stored, cells}
    int H, W, pitch, kind, kind2, conn;
    float level, level2;
};

template <int SCOPE>
static FIB_DEV int wave_find(const int *L, int i)
{
    for (;;) {
        const int p = __hip_atomic_load(L + i, __ATOMIC_RELAXED, SCOPE);
        if (p >= i || p < 0) return i;                  // (a root holds its own index; anything else that does not descend ends the walk too)
        i = p;
    }
}
template <int SCOPE>
static FIB_DEV void wave_unite(int *L, int a, int b)
{
    for (;;) {
        a = wave_find<SCOPE>(L, a);
        b = wave_find<SCOPE>(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);     // b < a: labels only ever descend
        if (old == a || old < 0) return;
        a = old;                                        // `a` had been hung elsewhere meanwhile: a + b has dropped, go on from there
    }
}
static FIB_DEV bool wave_cond(float x, int kind, float level) { return kind ? x < level : x > level; }

__global__ void __launch_bounds__(WV_THREADS) wave_label_kernel(WaveArgs a)
{
    constexpr int NW = WV_THREADS / 64, WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    __shared__ int lab[WV_TX * WV_TY];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (a.W + WV_TX - 1) / WV_TX;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * WV_TX, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * WV_TY;
    const int c = x0 + lane;
    const unsigned long long below = (1ull << lane) - 1ull;
    bool set[WV_CPT];
    int total = 0;
#pragma unroll
    for (int j = 0; j < WV_CPT; ++j) {
        const int ly = wave + NW * j, r = y0 + ly;
        bool s = false;
        if (r < a.H && c < a.W && (!a.mask || a.mask[(size_t)r * (size_t)a.W + (size_t)c] != 0)) {
            const size_t o = (size_t)r * (size_t)a.pitch + (size_t)c;
            s = wave_cond(a.x[o], a.kind, a.level);
            if (s && a.x2) s = wave_cond(a.x2[o], a.kind2, a.level2);
        }
        const unsigned long long m = __ballot(s);
        total += __popcll(m);
        const unsigned long long gap = ~m & below;      // the unset cells to the left: the run starts behind the last of them
        const int start = gap ? 64 - __builtin_clzll(gap) : 0;
        set[j] = s;
        lab[ly * WV_TX + lane] = s ? ly * WV_TX + start : -1;
    }
    if (total && lane == 0) atomicAdd(&a.cnt[2], total);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WV_CPT; ++j) {
        const int ly = wave + NW * j, i = ly * WV_TX + lane;
        if (!set[j] || ly == 0) continue;
        // (whether a cell is set never changes: only the labels of set cells move)
        const bool up = lab[i - WV_TX] >= 0;
        const bool left = lane > 0 && lab[i - 1] >= 0, upleft = lane > 0 && lab[i - WV_TX - 1] >= 0;
        const bool upright = lane < WV_TX - 1 && lab[i - WV_TX + 1] >= 0;
        if (up && !(left && upleft)) wave_unite<WG>(lab, i, i - WV_TX);
        if (a.conn == 8 && !up) {
            if (upleft && !left) wave_unite<WG>(lab, i, i - WV_TX - 1);
            if (upright) wave_unite<WG>(lab, i, i - WV_TX + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WV_CPT; ++j) {
        const int ly = wave + NW * j, r = y0 + ly;
        if (r >= a.H || c >= a.W) continue;
        int out = -1;
        if (set[j]) {
            const int root = wave_find<WG>(lab, ly * WV_TX + lane);
            out = (y0 + root / WV_TX) * a.W + x0 + root % WV_TX;
        }
        a.labels[(size_t)r * (size_t)a.W + (size_t)c] = out;
    }
}

// thread t < nbr * W: the cell (16 (t / W + 1), t % W) of a top row; else, with u = t - nbr * W, the cell (u % H, 64 (u / H + 1)) of
// a left column; nbr = (H - 1) / WV_TY and nbc = (W - 1) / WV_TX border rows and columns.  One union per CONTACT, as inside a
// tile: where the cell before it along the border lies in the same tile and it and its straight neighbour are set too, that
// cell (or one before it) has made the contact, and the label kernel has joined both pairs along the border.  At the first cell
// of a tile nothing is left to others: the cell before it is joined to it by the OTHER border's thread, which may rely on this one.
// A diagonal is looked at only where the straight neighbour is not set (else it touches the straight neighbour, and whoever
// owns that pair joins them)
__global__ void __launch_bounds__(256) wave_merge_kernel(int *__restrict__ labels, int H, int W, int conn, int nbr, int nbc)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long rows = (long long)nbr * W;
    if (t >= rows + (long long)nbc * H) return;
    int r, c, dr, dc;                   // the cell; the straight neighbour across the border is (r - dr, c - dc)
    if (t < rows) {
        r = ((int)(t / W) + 1) * WV_TY; c = (int)(t % W); dr = 1; dc = 0;
    } else {
        const long long u = t - rows;
        c = ((int)(u / H) + 1) * WV_TX; r = (int)(u % H); dr = 0; dc = 1;
    }
    const int i = r * W + c;
    // (whether a cell is set does not change here: plain loads will do)
    auto is_set = [&](int rr, int cc) { return rr >= 0 && rr < H && cc >= 0 && cc < W && labels[rr * W + cc] >= 0; };
    if (!is_set(r, c)) return;
    const int pr = r - dc, pc = c - dr;                                 // the cell before this one along the border
    const bool same_tile = dr ? c % WV_TX != 0 : r % WV_TY != 0;        // ... lies in this cell's tile
    const bool before = same_tile && is_set(pr, pc);
    if (is_set(r - dr, c - dc)) {
        if (!(before && is_set(pr - dr, pc - dc))) wave_unite<AG>(labels, i, (r - dr) * W + (c - dc));
    } else if (conn == 8) {
        if (!before && is_set(pr - dr, pc - dc)) wave_unite<AG>(labels, i, (pr - dr) * W + (pc - dc));
        const int fr = r - dr + dc, fc = c - dc + dr;
        if (is_set(fr, fc)) wave_unite<AG>(labels, i, fr * W + fc);
    }
}

__global__ void __launch_bounds__(256) wave_root_kernel(int *__restrict__ labels, int *__restrict__ slots, int ncells,
                                                        int *__restrict__ cnt, WaveRecord *__restrict__ rec, int max_waves)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)t;
    bool root = false;
    if (t < ncells) {
        const int l = labels[i];
        if (l >= 0) {
            const int rt = wave_find<AG>(labels, l);
            root = rt == i;
            if (rt != l) __hip_atomic_store(labels + i, rt, __ATOMIC_RELAXED, AG);      // (a path through this cell stays a path)
        }
    }
    // every lane of the wave comes here
    const unsigned long long roots = __ballot(root);
    if (!roots) return;
    const int lane = (int)(threadIdx.x & 63u);
    int base = 0;
    if (lane == 0) base = atomicAdd(&cnt[0], __popcll(roots));
    base = __shfl(base, 0, 64);
    const int slot = base + __popcll(roots & ((1ull << lane) - 1ull));
    const bool keep = root && slot < max_waves;
    const unsigned long long kept = __ballot(keep);
    if (kept && lane == 0) atomicAdd(&cnt[1], __popcll(kept));
    if (root) slots[i] = slot;
    if (keep) {
        WaveRecord w;
        w.seed = i; w.area = 0;
        w.sum_r = 0; w.sum_c = 0;
        w.r0 = 0x7fffffff; w.r1 = -1; w.c0 = 0x7fffffff; w.c1 = -1;
        rec[slot] = w;
    }
}

template <class T, class F>
static FIB_DEV T wave_all(T v, F f)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = f(v, __shfl_xor(v, off, 64));
    return v;
}
// what a set of cells adds to its wave's record
struct WaveSum {
    int area;
    long long sr, sc;
    int r0, r1, c0, c1;
    FIB_DEV void clear()
    {
        area = 0; sr = 0; sc = 0;
        r0 = 0x7fffffff; r1 = -1; c0 = 0x7fffffff; c1 = -1;
    }
    FIB_DEV void cell(int r, int c)
    {
        area += 1; sr += r; sc += c;
        r0 = min(r0, r); r1 = max(r1, r); c0 = min(c0, c); c1 = max(c1, c);
    }
    FIB_DEV void fold(const WaveSum &o)
    {
        area += o.area; sr += o.sr; sc += o.sc;
        r0 = min(r0, o.r0); r1 = max(r1, o.r1); c0 = min(c0, o.c0); c1 = max(c1, o.c1);
    }
    // over the 64 lanes; every lane of the wave must come here
    FIB_DEV void across_the_wave()
    {
        area = wave_all<int>(area, [](int x, int y) { return x + y; });
        sr = wave_all<long long>(sr, [](long long x, long long y) { return x + y; });
        sc = wave_all<long long>(sc, [](long long x, long long y) { return x + y; });
        r0 = wave_all<int>(r0, [](int x, int y) { return min(x, y); });
        c0 = wave_all<int>(c0, [](int x, int y) { return min(x, y); });
        r1 = wave_all<int>(r1, [](int x, int y) { return max(x, y); });
        c1 = wave_all<int>(c1, [](int x, int y) { return max(x, y); });
    }
    FIB_DEV void add_to(WaveRecord *w) const
    {
        atomicAdd(&w->area, area);
        atomicAdd(reinterpret_cast<unsigned long long *>(&w->sum_r), (unsigned long long)sr);
        atomicAdd(reinterpret_cast<unsigned long long *>(&w->sum_c), (unsigned long long)sc);
        atomicMin(&w->r0, r0);
        atomicMax(&w->r1, r1);
        atomicMin(&w->c0, c0);
        atomicMax(&w->c1, c1);
    }
};

// A workgroup takes WV_RED_CPT * 256 consecutive cells, thread t the cells base + 256 j + t: all labels are loaded first, then all
// slots (two round trips, not 2 * WV_RED_CPT).  While the contributing lanes of a wave all name one slot, and the same slot as
// before, every lane adds its cells up in registers — nothing crosses lanes; when that ends (another slot, or several in one
// step) what has run up is folded across the wave and one lane issues its seven atomics, and a step with several slots goes
// lane by lane.  What is left at the end is folded across the wave, the four waves' sums meet in LDS, and thread 0 folds
// neighbours of equal slot before it issues the atomics: inside a large domain a workgroup of 4096 cells issues seven.  (One
// cell per thread and the fold per wave took 197 us at 512^2 on a spiral of 150 000 cells: 17 000 atomics on one cache line.)
#define WV_RED_CPT 16
__global__ void __launch_bounds__(256) wave_reduce_kernel(const int *__restrict__ labels, const int *__restrict__ slots, int ncells, int W,
                                                          WaveRecord *__restrict__ rec, int max_waves)
{
    __shared__ int wslot[4];
    __shared__ WaveSum wsum[4];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const long long base = (long long)blockIdx.x * (256 * WV_RED_CPT) + threadIdx.x;
    int slot[WV_RED_CPT];
#pragma unroll
    for (int j = 0; j < WV_RED_CPT; ++j) {
        const long long t = base + 256 * j;
        slot[j] = t < ncells ? labels[t] : -1;                  // (the root, for now)
    }
#pragma unroll
    for (int j = 0; j < WV_RED_CPT; ++j) {
        const int s = slot[j] >= 0 ? slots[slot[j]] : -1;
        slot[j] = s >= 0 && s < max_waves ? s : -1;
    }
    int run = -1;                                               // (wave-uniform) the slot the lanes' sums belong to, -1: none
    WaveSum mine;
    mine.clear();
#pragma unroll
    for (int j = 0; j < WV_RED_CPT; ++j) {
        const unsigned long long act = __ballot(slot[j] >= 0);
        if (!act) continue;                                     // (wave-uniform)
        const int i = (int)(base + 256 * j), r = i / W, c = i - r * W;
        const int first = __shfl(slot[j], __builtin_ctzll(act), 64);
        const bool one = __ballot(slot[j] >= 0 && slot[j] != first) == 0;
        if (!(one && (run < 0 || run == first))) {
            if (run >= 0) {
                mine.across_the_wave();
                if (lane == 0) mine.add_to(rec + run);
                mine.clear();
            }
            run = -1;
        }
        if (one) {
            run = first;
            if (slot[j] >= 0) mine.cell(r, c);
        } else if (slot[j] >= 0) {
            WaveSum w;
            w.clear();
            w.cell(r, c);
            w.add_to(rec + slot[j]);
        }
    }
    mine.across_the_wave();
    if (lane == 0) {
        wslot[wave] = run;
        wsum[wave] = mine;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < 4; ++w) {
            if (wslot[w] < 0) continue;
            if (w + 1 < 4 && wslot[w + 1] == wslot[w]) wsum[w + 1].fold(wsum[w]);
            else wsum[w].add_to(rec + wslot[w]);
        }
    }
}

// ---- links (fibhip_waves_links_begin): which wave of the sample before does a wave of this sample share cells with ---------------
// With L[s] the label plane of sample s, a LINK of sample s >= 1 is a pair (prev, seed) for which some cell c has
// L[s - 1][c] = prev >= 0 and L[s][c] = seed >= 0; its OVERLAP is the number of such cells.  Two kernels behind the sample's four,
// behind a memset of the table and of the sample's four counts {links, stored, cells, lost}:
//   wave_link_kernel       one pass over the cells: a cell that is set in both planes adds itself to its pair's entry of an
//     open-addressing table in global memory, then prev[c] = labels[c] — by the cell's own thread, the only one that touches it.
//     A key is the 64-bit pair plus one (0: empty; a memset clears keys and counts at once); an insertion is a relaxed
//     agent-scope 64-bit compare-exchange on the key, then a 32-bit atomicAdd on the entry's count.  T entries, a power of two;
//     double hashing: a 64-bit mixer gives the first entry and an ODD step, so T <= 32 entries are all visited within the
//     WV_LINK_PROBES = 32 probes that bound the walk.  A pair that finds neither itself nor an empty entry within the bound
//     adds its cells to `lost` and is gone; nothing is ever deleted, so a pair that is in the table is found again by the same
//     walk and its overlap is exact whatever else was lost.  Contention as in wave_reduce_kernel: while the contributing lanes of a
//     wave all name one pair they count in registers, the counts are folded across the wave and the four waves' through LDS
//     (inside a large domain a workgroup of 4096 cells issues ONE insertion); a step with several pairs peels off up to
//     WV_LINK_PEEL of them, one insertion each by ballot and popcount, and whatever is left goes lane by lane.  `cells` and
//     `lost` take one atomicAdd per workgroup.
//   wave_link_pack_kernel  one thread per entry: an occupied entry takes a rank (one atomicAdd on `links` per wave of the GPU, ranks
//     by ballot: wave_root_kernel's way) and, if that is below max_links, counts itself in `stored` and writes its record.
// Both read the give-up word first and write NOTHING once it is raised — not prev, not the table, not the slot: prev is carried
// from sample to sample and has to stay the plane of the last good sample (recorders.hpp).  Integer atomics only, no kernel waits
// for another workgroup, every loop is bounded by a constant; they end whatever the planes hold.
#define WV_LINK_PROBES 32
#define WV_LINK_CPT 16
#define WV_LINK_PEEL 4
struct WaveLink {               // fibhip_wave_link
    int prev, seed, overlap;
};
static FIB_DEV unsigned long long wave_link_mix(unsigned long long x)      // (the finaliser of splitmix64)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// `n` cells for the pair behind `key` (never 0); -> the cells that found no room (0 or n).  tmask = T - 1, T >= 4
static FIB_DEV int wave_link_insert(unsigned long long *keys, int *vals, unsigned tmask, unsigned long long key, int n)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const unsigned long long h = wave_link_mix(key);
    unsigned i = (unsigned)h & tmask;
    const unsigned step = ((unsigned)(h >> 32) | 1u) & tmask;
    for (int p = 0; p < WV_LINK_PROBES; ++p) {
        unsigned long long k = __hip_atomic_load(keys + i, __ATOMIC_RELAXED, AG);
        if (k == 0ull && __hip_atomic_compare_exchange_strong(keys + i, &k, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, AG)) k = key;
        // (a compare-exchange that failed has left in k what it met)
        if (k == key) {
            atomicAdd(vals + i, n);
            return 0;
        }
        i = (i + step) & tmask;
    }
    return n;
}

__global__ void __launch_bounds__(256) wave_link_kernel(const int *__restrict__ labels, int *__restrict__ prev, int ncells,
                                                        unsigned long long *__restrict__ keys, unsigned tmask, int *__restrict__ cnt,
                                                        const unsigned *__restrict__ give_up)
{
    if (give_up && *give_up != 0u) return;                      // (wave-uniform: one scalar load)
    __shared__ unsigned long long wkey[4];
    __shared__ int wn[4], wcells[4], wlost[4];
    int *vals = reinterpret_cast<int *>(keys + (size_t)tmask + 1);
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const long long base = (long long)blockIdx.x * (256 * WV_LINK_CPT) + threadIdx.x;
    int now[WV_LINK_CPT], was[WV_LINK_CPT];
#pragma unroll
    for (int j = 0; j < WV_LINK_CPT; ++j) {
        const long long t = base + 256 * j;
        now[j] = t < ncells ? labels[t] : -1;
        was[j] = t < ncells ? prev[t] : -1;
    }
    unsigned long long key[WV_LINK_CPT];                        // 0: the cell contributes nothing
#pragma unroll
    for (int j = 0; j < WV_LINK_CPT; ++j) {
        const long long t = base + 256 * j;
        if (t < ncells && now[j] != was[j]) prev[t] = now[j];
        key[j] = now[j] >= 0 && was[j] >= 0 ? (((unsigned long long)(unsigned)was[j] << 32) | (unsigned long long)(unsigned)now[j]) + 1ull : 0ull;
    }
    unsigned long long run = 0ull;                              // (wave-uniform) the pair the lanes' counts belong to, 0: none
    int mine = 0, cells = 0, lost = 0;
#pragma unroll
    for (int j = 0; j < WV_LINK_CPT; ++j) {
        const bool on = key[j] != 0ull;
        const unsigned long long act = __ballot(on);
        if (!act) continue;                                     // (wave-uniform)
        cells += on ? 1 : 0;
        const unsigned long long first = __shfl(key[j], __builtin_ctzll(act), 64);
        const bool one = __ballot(on && key[j] != first) == 0;
        if (!(one && (run == 0ull || run == first))) {
            if (run != 0ull) {
                mine = wave_all<int>(mine, [](int x, int y) { return x + y; });
                if (lane == 0) lost += wave_link_insert(keys, vals, tmask, run, mine);
                mine = 0;
            }
            run = 0ull;
        }
        if (one) {
            run = first;
            mine += on ? 1 : 0;
        } else {
            unsigned long long rest = act;                      // (wave-uniform, and so is the loop)
#pragma unroll
            for (int p = 0; p < WV_LINK_PEEL; ++p) {
                if (!rest) break;
                const int leader = __builtin_ctzll(rest);
                const unsigned long long k = __shfl(key[j], leader, 64);
                const unsigned long long same = __ballot(on && key[j] == k);
                if (lane == leader) lost += wave_link_insert(keys, vals, tmask, k, __popcll(same));
                rest &= ~same;
            }
            if ((rest >> lane) & 1ull) lost += wave_link_insert(keys, vals, tmask, key[j], 1);
        }
    }
    mine = wave_all<int>(mine, [](int x, int y) { return x + y; });
    cells = wave_all<int>(cells, [](int x, int y) { return x + y; });
    lost = wave_all<int>(lost, [](int x, int y) { return x + y; });
    if (lane == 0) {
        wkey[wave] = run;
        wn[wave] = mine;
        wcells[wave] = cells;
        wlost[wave] = lost;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0, l = 0;
        for (int w = 0; w < 4; ++w) {
            c += wcells[w];
            l += wlost[w];
            if (wkey[w] == 0ull) continue;
            if (w + 1 < 4 && wkey[w + 1] == wkey[w]) wn[w + 1] += wn[w];
            else l += wave_link_insert(keys, vals, tmask, wkey[w], wn[w]);
        }
        if (c) atomicAdd(&cnt[2], c);
        if (l) atomicAdd(&cnt[3], l);
    }
}

__global__ void __launch_bounds__(256) wave_link_pack_kernel(const unsigned long long *__restrict__ keys, unsigned entries, int *__restrict__ cnt,
                                                             WaveLink *__restrict__ rec, int max_links, const unsigned *__restrict__ give_up)
{
    if (give_up && *give_up != 0u) return;                      // (wave-uniform: one scalar load)
    const int *vals = reinterpret_cast<const int *>(keys + (size_t)entries);
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const unsigned long long key = t < entries ? keys[t] : 0ull;
    // every lane of the wave comes here
    const unsigned long long full = __ballot(key != 0ull);
    if (!full) return;
    const int lane = (int)(threadIdx.x & 63u);
    int base = 0;
    if (lane == 0) base = atomicAdd(&cnt[0], __popcll(full));
    base = __shfl(base, 0, 64);
    const int rank = base + __popcll(full & ((1ull << lane) - 1ull));
    const bool keep = key != 0ull && rank < max_links;
    const unsigned long long kept = __ballot(keep);
    if (kept && lane == 0) atomicAdd(&cnt[1], __popcll(kept));
    if (keep) {
        const unsigned long long pair = key - 1ull;
        WaveLink w;
        w.prev = (int)(unsigned)(pair >> 32); w.seed = (int)(unsigned)(pair & 0xffffffffull);
        w.overlap = vals[t];
        rec[rank] = w;
    }
}

// ---- lesion program (fibhip_lesion_begin, fibhip_lesion_apply): the hook that writes the PHASE FIELD, not the state ----------
// A lesion is a float32 factor patch m on a box [r0, r1) x [c0, c1): phi = fmaxf(phi * m, 1e-5f) on the cells of the box — one
// multiplication rounded on its own (-ffp-contract=off) and one maximum, add_hole_to_phase_field's update restricted to the
// cells where its mask is not 1.0f.  The entries due after one tick — at most LESION_MAX_DUE per launch, the host issues further
// launches in program order beyond that — travel BY VALUE in the kernel argument (stim_kernel's note: every field is
// wave-uniform).  The product does not commute with the floor, so a cell takes the entries that hold it IN PROGRAM ORDER: the
// host has put entries whose boxes overlap, directly or through others, into one CLUSTER (two entries of different clusters
// share no cell and commute); grid.y is the cluster, grid.x covers the bounding box of the largest one, one cell per thread, and
// a thread walks the entries of its cluster (`member`, a bit per entry) in order with the cell in a register.  It loads phi
// once and stores it once, and only if an entry held the cell: the bounding box of a cluster may reach into another cluster's
// cells, which are that cluster's to write.  Only the boxes are visited, never the grid.  The patches are plain cached loads,
// the store a plain vector store; no LDS, no atomics.  `give_up`: the give-up word of the multi-tick launches (null behind a
// plain tick and in fibhip_lesion_apply, which confirm first) — once a launch in front gave up this kernel writes NOTHING, so
// the field that launch started from is intact when recover() replays its ticks and applies the events of those ticks again.
#define LESION_MAX_DUE 8
struct LesionDue {
    const float *patch;     // the factors, [r1 - r0][c1 - c0]
    int r0, r1, c0, c1;
};
struct LesionBox {
    int r0, r1, c0, c1;
    unsigned member;        // apply: bit i — entry i belongs to this cluster
};
struct LesionArgs {
    LesionDue e[LESION_MAX_DUE];
    LesionBox box[LESION_MAX_DUE];  // apply: the clusters' bounding boxes; prep: the entries' boxes dilated by one cell, cut at the grid
    int n, nbox;
    const unsigned *give_up;
};
#define LESION_FLOOR 1e-5f

__global__ void __launch_bounds__(256) lesion_apply_kernel(LesionArgs a, float *__restrict__ phi, int W)
{
    if (a.give_up && *a.give_up != 0u) return;                        // (wave-uniform: one scalar load)
    LesionBox b = a.box[0];
#pragma unroll
    for (int i = 1; i < LESION_MAX_DUE; ++i)
        if ((int)blockIdx.y == i) b = a.box[i];                       // (no run-time index into the argument)
    const int bw = b.c1 - b.c0;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)(b.r1 - b.r0) * (size_t)bw) return;
    const int y = b.r0 + (int)(t / (size_t)bw), x = b.c0 + (int)(t % (size_t)bw);
    const size_t at = (size_t)y * (size_t)W + (size_t)x;
    float p = phi[at];
    bool held = false;
#pragma unroll
    for (int i = 0; i < LESION_MAX_DUE; ++i) {
        if (i >= a.n || !((b.member >> i) & 1u)) continue;            // (wave-uniform)
        const LesionDue &d = a.e[i];
        if (y >= d.r0 && y < d.r1 && x >= d.c0 && x < d.c1) {
            const float m = d.patch[(size_t)(y - d.r0) * (size_t)(d.c1 - d.c0) + (size_t)(x - d.c0)];
            p = fmaxf(p * m, LESION_FLOOR);
            held = true;
        }
    }
    if (held) phi[at] = p;
}

// The six derived planes (dpy, dpx, q4, r4, dpy*r4, dpx*r4) on the boxes dilated by one cell and cut at the grid, from the new
// phi: phase_prep_kernel's own expression and reflection (phase_prep_cell), one cell per thread, grid.y the box.  A launch of
// its own BEHIND lesion_apply_kernel: a cell reads its neighbours' phi, which other threads have just written.  It is a pure
// function of phi — idempotent — so it needs no gate: behind an apply that wrote nothing it rewrites the values that stand
// there, and two dilated boxes that overlap write the same values twice.
__global__ void __launch_bounds__(256) lesion_prep_kernel(LesionArgs a, Geo g, const float *phi, float *dpy, float *dpx, float *q4, float *r4,
                                                          float *pyr, float *pxr)
{
    LesionBox b = a.box[0];
#pragma unroll
    for (int i = 1; i < LESION_MAX_DUE; ++i)
        if ((int)blockIdx.y == i) b = a.box[i];
    const int bw = b.c1 - b.c0;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)(b.r1 - b.r0) * (size_t)bw) return;
    phase_prep_cell(g, b.r0 + (int)(t / (size_t)bw), b.c0 + (int)(t % (size_t)bw), phi, dpy, dpx, q4, r4, pyr, pxr);
}
