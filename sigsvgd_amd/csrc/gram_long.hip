// Signature-kernel Gram matrix and gradient for the built-in static kernels on long paths.
//
// The fused Gram kernels keep a pair's whole-grid state in LDS and refuse paths past it (the coverage kernel from about
// T = 250 at order 0, and refined grids whose tables outgrow 160 KB).  This kernel takes those launches with the ring sweep of
// ring_sweep.h, which sig_pde_kernel (sig_pde.hip) runs too: one wavefront per pair in a persistent grid, bands of 64 rows of
// the refined P x Q grid, one row per lane, swept anti-diagonal by anti-diagonal, the band's boundary row in LDS, and an LDS
// ring of the band's fp64 increments refilled between blocks of 64 sweep steps.  What differs is where the ring's values come
// from: the fill evaluates the static kernel itself,
//   D[a][b] = k(x_{a+1}, y_{b+1}) - k(x_{a+1}, y_b) - k(x_a, y_{b+1}) + k(x_a, y_b)      (fp64)
// from the band's nrow + 1 points of X_i (staged in LDS) and the columns of Y_j (one static-kernel column per lane, read from
// global memory), so the [A, B, M, N] grid never exists.  Increments, sweeps and the gradient are fp64; the stored forward
// solution and the S partials are fp32, as in sig_pde.
//
// Backward: the shared reverse sweep (the reference's GG convention), then the pair's coarse S is chained through the
// static kernel into the gradient of x_i:  gX_i[m] += w_ij sum_n dG[m][n] dk(x_m, y_n)/dx_m, with dG the 4-corner scatter of S
// and dk/dx = -2 inv_h (x - y) k (RBF) or y (linear).  Lanes own points m; k is evaluated again there.  A work item is
// (i, chunk of JC columns j): its pairs add into one [TX][d] fp64 slab in j order (the same lane always owns the same entry),
// and long2_reduce_kernel adds the slabs of a row i in chunk order.  No floating-point atomics: the bits depend on the inputs.
//
// Paired mode (PAIRED): work item i is the one pair (X_i, Y_i), K_out[i] = k_sig(X_i, Y_i) from the
// same fill and sweeps.  From the pair's one S the gradient pass writes gX_i straight into the caller's buffer, and the same
// pass with lanes owning points n of Y_i and walking m chains S through dk/dy into gY_i[n] = w_i sum_m dG[m][n] dk(x_m, y_n)/dy_n
// (dk/dy = 2 inv_h (x - y) k for RBF, x for linear).  Either output may be skipped; no slabs and no reduce kernel.
// Where a pair has bands enough for it to pay (pair_use_bands), pair_launch hands the launch to pair_bands.hip (a workgroup per
// pair, its bands dealt to the wavefronts): same bits, same workspace.  The static kernels' device
// helpers both files use are in long_static.h.
//
// Two-sided Gram mode (gram_long2_kernel): a work item is a tile of IC rows x JC columns whose pairs
// are walked row by row.  After a pair's one reverse sweep the row-side pass adds w_row dk/dx into the tile's fp64 slab of
// row i and the column-side pass adds w_col dk/dy into its slab of column j; long2_reduce_kernel adds a row's (a column's)
// slabs in tile order.  With Y = X (yx) the items are the tiles of the upper triangle, only pairs i <= j are solved, K is
// mirrored, and the column side of pair (i, j) is row j's first-slot gradient of the pair (j, i): both sides meet in gX.
//
// Partial mode (gram_long_part_kernel): one rank's share of the Y-is-X launch for the sharded SVGD
// step.  The launch owns row tiles (TileMap, folded or cyclic), an item is a rectangle of R rows x JC columns of an owned
// tile from its first row on, the slabs cover the owned tiles only, and long_part_reduce_kernel writes the fp64 partial
// gradient of every row (zero where nothing arrived).  The host picks (R, JC) by search (part_pick).
//
// Bandwidth launches (BW): the paired and the two-sided kernel with one more pass per pair behind the
// gradient passes, static_bw_pass (long_static.h), which contracts the same S with the static kernel's derivative in inv_h and
// stores the pair's dK / d inv_h, unweighted.  A compile-time flag: the instantiations without it are the code they were.
//
// The Matern kinds are instantiated in gram_long_matern.hip, which includes this file for its kernels
// and families (long_matern_launch below); family_launch sends their launches there.
//
// The per-pair solve (staging, fill, forward sweep, K store, reverse sweep) is written out in each of the three kernels, and K's
// bit-identity across the modes rests on the copies staying equal.  One shared function (long_solve_pair over a PairSource, with
// one two_sided_grad block) gave the same bits and the same registers, scratch and occupancy, but was measured slower on the
// MI355X: forward-only launches by 1.5-4 %, the partial kernel by 1-1.4 %, ranges of run-medians apart
// (profiles/long_shared_solve_ab.txt).  So the copies stay.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <vector>

#include "long_static.h"
#include "pair_bands.h"
#include "ring_sweep.h"

namespace sigsvgd {

struct LongArgs {
    const void *X, *Y, *grad_out;
    void *K_out;
    double *partials;     // [A][nchunks][TX * d]
    float *wsk;           // [grid][wsk_per_block]: forward solution, then S partials (+ one spare row)
    size_t wsk_per_block; // floats
    int A, B, M, N, d, n, r, P, Q, nbands, nsteps, nrow, W, JC, nchunks, sym;
    long long items;
    double inv_h, inv_r2;
};
// the paired mode's arguments: LongArgs (B = 1 chunk per row, partials unused) and the two gradient outputs (caller's dtype,
// either may be NULL).  A type of its own, so the Gram kernels' argument layout stays as it is.
struct PairArgs : LongArgs {
    void *gradX, *gradY; // [A][TX][d], [A][TY][d]
};
// the two-sided Gram mode's arguments: LongArgs (JC, nchunks: the column tiles; partials: the row slabs [A][nchunks][TX * d],
// or with yx [A][nti + 1][TX * d]: row k's column-side slabs of tile rows 0 .. k / IC, then its row-side slabs) and the column
// side.  Again a type of its own.
struct Long2Args : LongArgs {
    double *colpart; // [B][nti][TY * d] (NULL with yx, or when gradY is not wanted)
    int IC, nti, yx, want_row, want_col;
};
// the partial mode's arguments: LongArgs (A = B paths of M = N points; JC: the columns of an item;
// partials: the row-side slabs, one [TX * d] per (row of an owned tile, column chunk), owned tiles in the order of `tm`) and
// the column-side slabs, one per (owned tile, row j from the tile's first row on): TileMap::start gives a tile's first.
// The bandwidth launches' arguments: the paired mode's and the two-sided mode's with the output of the
// per-pair dK / d inv_h (caller's dtype).  Types of their own once more: the launches without it keep their argument layout.
struct PairHArgs : PairArgs {
    void *dK_dinvh; // [A]
};
struct Long2HArgs : Long2Args {
    void *dK_dinvh; // [A][B]
};
struct PartArgs : LongArgs {
    double *colpart;
    TileMap tm;      // the row tiles this launch owns, R rows each
    int R;
    long long nfull; // items of the first pass (the chunks strictly between a tile's first and last)
};


// BW (paired mode only): after the pair's gradient passes one more pass chains the same S through the
// static kernel's derivative in the bandwidth and stores the pair's dK / d inv_h; a compile-time branch, so the instantiations
// without it keep their code.
template <typename IO, bool NAIVE, bool GRAD, int KIND, bool PAIRED = false, bool BW = false>
__global__ __launch_bounds__(64) void gram_long_kernel(
    std::conditional_t<BW, PairHArgs, std::conditional_t<PAIRED, PairArgs, LongArgs>> a)
{
    static_assert(!BW || (PAIRED && GRAD), "the bandwidth pass needs the paired mode's reverse sweep");
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const int M = a.M, N = a.N, W = a.W, nrow = a.nrow, d = a.d;
    const RingWave rw = ring_wave<GRAD>(a, smem_raw);
    double *ring = rw.ring;
    double *xs = rw.dump + kWave; // [nrow + 1][d]: points a0 .. a0 + nrow of X_i (clamped to M - 1)
    const IO *GO = static_cast<const IO *>(a.grad_out);

    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int i = PAIRED ? (int)item : (int)(item / a.nchunks);
        const int j0 = PAIRED ? i : (int)(item % a.nchunks) * a.JC, j1 = PAIRED ? i + 1 : min(a.B, j0 + a.JC);
        const IO *xi = static_cast<const IO *>(a.X) + (size_t)i * M * d;
        double *slab = GRAD && !PAIRED ? a.partials + (size_t)item * M * d : nullptr;

        for (int j = j0; j < j1; ++j) {
            const IO *yj = static_cast<const IO *>(a.Y) + (size_t)j * N * d;
            // the band's points of X_i (before the band's first fill, whose barrier publishes them)
            auto stage_x = [&](int a0) {
                for (int e = lane; e < (nrow + 1) * d; e += kWave) {
                    const int k = e / d;
                    xs[e] = (double)xi[(size_t)min(a0 + k, M - 1) * d + (e - k * d)];
                }
            };
            // coarse columns b_lo .. b_hi of the increment rows a0 .. a0 + nrow - 1 into the ring: lane l evaluates the static
            // kernel at column b0 + l down the band's points, the next lane's value gives the column difference (63 increment
            // columns per pass); every evaluation is unconditional at a clamped column
            auto fill = [&](int a0, int b_lo, int b_hi) {
                __syncthreads(); // (the sweep's reads of the slots this overwrites are done; xs is staged)
                for (int b0 = b_lo; b0 <= b_hi; b0 += kWave - 1) {
                    const int b = b0 + lane;
                    const bool ok = lane < kWave - 1 && b <= b_hi;
                    const IO *yb = yj + (size_t)min(b, N - 1) * d;
                    // (up to 16 channels the lane's point stays in registers for the whole column: one round of loads)
                    double yv[16];
#pragma unroll
                    for (int c = 0; c < 16; ++c) yv[c] = (double)yb[min(c, d - 1)];
                    double rd_prev = 0.0;
                    for (int k = 0; k <= nrow; ++k) {
                        const double g = d <= 16 ? static_k16<KIND>(xs + k * d, yv, d, a.inv_h)
                                                 : static_k<KIND>(xs + k * d, yb, d, a.inv_h);
                        const double rd = shfl_down_f64(g) - g; // k(x_{a0+k}, y_{b+1}) - k(x_{a0+k}, y_b)
                        if (k >= 1 && ok) ring[(k - 1) * W + (b & (W - 1))] = (a0 + k < M) ? rd - rd_prev : 0.0;
                        rd_prev = rd;
                    }
                }
                __syncthreads();
            };

            const double Kval = ring_forward<NAIVE, GRAD>(rw, fill, stage_x);
            if (((rw.P - 1) & (kWave - 1)) == lane) static_cast<IO *>(a.K_out)[PAIRED ? (size_t)i : (size_t)i * a.B + j] = (IO)Kval;
            if (!GRAD) {
                __syncthreads(); // (the next pair's first fill overwrites the ring, its sweep the boundary row)
                continue;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the forward solution is in L2 before it is read back
            __syncthreads();
            ring_reverse<NAIVE>(rw, fill, stage_x);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // S is in L2 before it is read back
            __syncthreads();

            // ---- gradient: S -> dG (4-corner scatter) -> static-kernel derivative -> gX_i (and gY_i, paired) ---------------
            double w = GO ? (double)GO[PAIRED ? (size_t)i : (size_t)i * a.B + j] : 1.0;
            if (!PAIRED && a.sym) w += GO ? (double)GO[(size_t)j * a.B + i] : 1.0;
            if constexpr (PAIRED) { // (either output skipped when NULL)
                IO *gX = static_cast<IO *>(a.gradX), *gY = static_cast<IO *>(a.gradY);
                if (gX)
                    static_grad_pass<KIND, true>(rw, xi, M, yj, N, d, a.inv_h, [&](int m, int c, double g) {
                        gX[((size_t)i * M + m) * d + c] = (IO)(w * g);
                    });
                if (gY)
                    static_grad_pass<KIND, false>(rw, yj, N, xi, M, d, a.inv_h, [&](int nn, int c, double g) {
                        gY[((size_t)i * N + nn) * d + c] = (IO)(w * g);
                    });
                if constexpr (BW) { // (unweighted: K's own derivative)
                    const double dk = static_bw_pass<KIND>(rw, xi, M, yj, N, d, a.inv_h);
                    if (lane == 0) static_cast<IO *>(a.dK_dinvh)[i] = (IO)dk;
                }
            } else { // into the item's slab, in j order
                static_grad_pass<KIND, true>(rw, xi, M, yj, N, d, a.inv_h, [&](int m, int c, double g) {
                    double *o = slab + (size_t)m * d + c;
                    *o = j == j0 ? w * g : __builtin_fma(w, g, *o);
                });
            }
            __syncthreads(); // (the next pair's forward sweep overwrites the scratch and the ring)
        }
    }
}

// The two-sided Gram mode, a kernel of its own so that gram_long_kernel's instantiations keep
// their code: the same staging, fill and sweeps per pair (K has the same bits), the items and the gradient passes differ.
// BW: the bandwidth pass behind the pair's gradient passes, as in gram_long_kernel; with yx the pair
// (i, j) stores its derivative at [i][j] and [j][i], as K's mirror does.
template <typename IO, bool NAIVE, bool GRAD, int KIND, bool BW = false>
__global__ __launch_bounds__(64) void gram_long2_kernel(std::conditional_t<BW, Long2HArgs, Long2Args> a)
{
    static_assert(!BW || GRAD, "the bandwidth pass needs the reverse sweep");
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const int M = a.M, N = a.N, W = a.W, nrow = a.nrow, d = a.d;
    const RingWave rw = ring_wave<GRAD>(a, smem_raw);
    double *ring = rw.ring;
    double *xs = rw.dump + kWave; // [nrow + 1][d]: points a0 .. a0 + nrow of X_i (clamped to M - 1)
    const IO *GO = static_cast<const IO *>(a.grad_out);

    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        // the item's tile (ti, tj): rows i0 .. i1 - 1 x columns j0 .. j1 - 1, walked row by row
        int ti = 0, tj = 0;
        if (!a.yx) {
            ti = (int)(item / a.nchunks);
            tj = (int)(item % a.nchunks);
        } else if (item < a.nti) { // the diagonal tiles (half empty) first, so that the grid's last round is full tiles
            ti = tj = (int)item;
        } else { // then the tiles above the diagonal, row by row
            long long rem = item - a.nti;
            for (; rem >= a.nti - 1 - ti; ++ti) rem -= a.nti - 1 - ti;
            tj = ti + 1 + (int)rem;
        }
        const int i0 = ti * a.IC, i1 = min(a.A, i0 + a.IC), j0 = tj * a.JC, j1 = min(a.B, j0 + a.JC);

        for (int i = i0; i < i1; ++i) {
            const IO *xi = static_cast<const IO *>(a.X) + (size_t)i * M * d;
            const int jfirst = a.yx ? max(j0, i) : j0; // (yx: the pairs i <= j only)

            for (int j = jfirst; j < j1; ++j) {
                const IO *yj = static_cast<const IO *>(a.Y) + (size_t)j * N * d;
                // staging and fill: gram_long_kernel's, statement for statement (K must have its bits); a copy because
                // the shared helper measured slower (profiles/long_shared_solve_ab.txt)
                auto stage_x = [&](int a0) {
                    for (int e = lane; e < (nrow + 1) * d; e += kWave) {
                        const int k = e / d;
                        xs[e] = (double)xi[(size_t)min(a0 + k, M - 1) * d + (e - k * d)];
                    }
                };
                auto fill = [&](int a0, int b_lo, int b_hi) {
                    __syncthreads(); // (the sweep's reads of the slots this overwrites are done; xs is staged)
                    for (int b0 = b_lo; b0 <= b_hi; b0 += kWave - 1) {
                        const int b = b0 + lane;
                        const bool ok = lane < kWave - 1 && b <= b_hi;
                        const IO *yb = yj + (size_t)min(b, N - 1) * d;
                        // (up to 16 channels the lane's point stays in registers for the whole column: one round of loads)
                        double yv[16];
#pragma unroll
                        for (int c = 0; c < 16; ++c) yv[c] = (double)yb[min(c, d - 1)];
                        double rd_prev = 0.0;
                        for (int k = 0; k <= nrow; ++k) {
                            const double g = d <= 16 ? static_k16<KIND>(xs + k * d, yv, d, a.inv_h)
                                                     : static_k<KIND>(xs + k * d, yb, d, a.inv_h);
                            const double rd = shfl_down_f64(g) - g; // k(x_{a0+k}, y_{b+1}) - k(x_{a0+k}, y_b)
                            if (k >= 1 && ok) ring[(k - 1) * W + (b & (W - 1))] = (a0 + k < M) ? rd - rd_prev : 0.0;
                            rd_prev = rd;
                        }
                    }
                    __syncthreads();
                };

                const double Kval = ring_forward<NAIVE, GRAD>(rw, fill, stage_x);
                if (((rw.P - 1) & (kWave - 1)) == lane) {
                    static_cast<IO *>(a.K_out)[(size_t)i * a.B + j] = (IO)Kval;
                    if (a.yx) static_cast<IO *>(a.K_out)[(size_t)j * a.B + i] = (IO)Kval; // the mirror: same bits
                }
                if (!GRAD) {
                    __syncthreads(); // (the next pair's first fill overwrites the ring, its sweep the boundary row)
                    continue;
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the forward solution is in L2 before it is read back
                __syncthreads();
                ring_reverse<NAIVE>(rw, fill, stage_x);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // S is in L2 before it is read back
                __syncthreads();

                // ---- gradient: both sides from the pair's one S, each into its slab in the tile's pair order ----------------
                double w = GO ? (double)GO[(size_t)i * a.B + j] : 1.0, wc = w; // the row side's and the column side's weight
                if (a.sym || a.yx) {
                    const double wt = GO ? (double)GO[(size_t)j * a.B + i] : 1.0;
                    if (a.sym)
                        w = wc = w + wt;
                    else
                        wc = wt; // yx: the column side is d k(X_j, X_i) / d X_j
                }
                // yx: row k's slabs are [nti + 1]: the column side's of tile rows 0 .. k / IC, then the row side's
                const int TDx = M * d, TDy = N * d;
                double *rs = a.partials + (a.yx ? (size_t)i * (a.nti + 1) + tj + 1 : (size_t)i * a.nchunks + tj) * TDx;
                double *cs = a.yx ? a.partials + ((size_t)j * (a.nti + 1) + ti) * TDx
                                  : a.colpart + ((size_t)j * a.nti + ti) * TDy;
                if (a.want_row)
                    static_grad_pass<KIND, true>(rw, xi, M, yj, N, d, a.inv_h, [&](int m, int c, double g) {
                        double *o = rs + (size_t)m * d + c;
                        *o = j == jfirst ? w * g : __builtin_fma(w, g, *o);
                    });
                if (a.want_col && !(a.yx && i == j)) // (a diagonal pair of yx has one slot: the row side took it)
                    static_grad_pass<KIND, false>(rw, yj, N, xi, M, d, a.inv_h, [&](int nn, int c, double g) {
                        double *o = cs + (size_t)nn * d + c;
                        *o = i == i0 ? wc * g : __builtin_fma(wc, g, *o);
                    });
                if constexpr (BW) { // (unweighted: K's own derivative)
                    const double dk = static_bw_pass<KIND>(rw, xi, M, yj, N, d, a.inv_h);
                    if (lane == 0) {
                        static_cast<IO *>(a.dK_dinvh)[(size_t)i * a.B + j] = (IO)dk;
                        if (a.yx) static_cast<IO *>(a.dK_dinvh)[(size_t)j * a.B + i] = (IO)dk; // the mirror: same bits
                    }
                }
                __syncthreads(); // (the next pair's forward sweep overwrites the scratch and the ring)
            }
        }
    }
}

// ---- partial mode: this launch's share of the Y-is-X solve --------------------------------------
// Row tile t (R rows) owns the pairs (i, j), i in the tile, j >= i; the launch owns the tiles of `tm`.  An item is (owned
// tile kq, chunk c): the tile's rows x the columns i0 + c JC .. i0 + (c + 1) JC - 1 (i0 the tile's first row; the first chunk
// is ragged by the diagonal, the last by the matrix edge).  Items are taken in three passes -- the chunks strictly between a
// tile's first and last (whole rectangles when JC >= R), then every tile's first chunk, then the last chunks -- so the grid's
// last, partly filled round gets the small items.  The helpers below are the host plan's too.
__host__ __device__ inline int part_rows(const TileMap &tm, int kq, int A, int R)
{
    const int i0 = tm.tile_of(kq) * R;
    return (A < i0 + R ? A : i0 + R) - i0;
}
__host__ __device__ inline int part_chunks(const TileMap &tm, int kq, int A, int R, int JC)
{
    return (A - tm.tile_of(kq) * R + JC - 1) / JC;
}
// item -> (kq, c)
__host__ __device__ inline void part_decode(const TileMap &tm, long long item, long long nfull, int A, int R, int JC, int &kq,
                                            int &c)
{
    kq = 0;
    if (item < nfull) {
        for (;; ++kq) {
            const int n = part_chunks(tm, kq, A, R, JC) - 2;
            if (n > 0) {
                if (item < n) break;
                item -= n;
            }
        }
        c = 1 + (int)item;
    } else if ((item -= nfull) < tm.owned) {
        kq = (int)item;
        c = 0;
    } else {
        item -= tm.owned;
        for (;; ++kq)
            if (part_chunks(tm, kq, A, R, JC) >= 2 && item-- == 0) break;
        c = part_chunks(tm, kq, A, R, JC) - 1;
    }
}
// row-side slabs of the owned tiles before kq
__host__ __device__ inline long long part_row_base(const TileMap &tm, int kq, int A, int R, int JC)
{
    long long s = 0;
    for (int q = 0; q < kq; ++q) s += (long long)part_rows(tm, q, A, R) * part_chunks(tm, q, A, R, JC);
    return s;
}

// A kernel of its own, as the two-sided mode is: gram_long_kernel's and gram_long2_kernel's instantiations keep their code.
// Per pair the staging, fill, sweeps and gradient passes are gram_long2_kernel's with Y = X (K has the same bits).
template <typename IO, bool NAIVE, int KIND>
__global__ __launch_bounds__(64) void gram_long_part_kernel(PartArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const int M = a.M, N = a.N, W = a.W, nrow = a.nrow, d = a.d, TD = a.M * a.d;
    const RingWave rw = ring_wave<true>(a, smem_raw);
    double *ring = rw.ring;
    double *xs = rw.dump + kWave; // [nrow + 1][d]: points a0 .. a0 + nrow of X_i (clamped to M - 1)
    const IO *GO = static_cast<const IO *>(a.grad_out);

    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        int kq, c;
        part_decode(a.tm, item, a.nfull, a.A, a.R, a.JC, kq, c);
        const int nck = part_chunks(a.tm, kq, a.A, a.R, a.JC);
        const int i0 = a.tm.tile_of(kq) * a.R, i1 = min(a.A, i0 + a.R), j0 = i0 + c * a.JC, j1 = min(a.A, j0 + a.JC);
        double *rowslabs = a.partials + (size_t)part_row_base(a.tm, kq, a.A, a.R, a.JC) * TD; // [rows][nck][TD]
        double *colslabs = a.colpart + (size_t)a.tm.start(kq, a.A, a.R, 1) * TD;              // [j - i0][TD]

        for (int i = i0; i < i1; ++i) {
            const IO *xi = static_cast<const IO *>(a.X) + (size_t)i * M * d;
            const int jfirst = max(j0, i); // the pairs i <= j only

            for (int j = jfirst; j < j1; ++j) {
                const IO *yj = static_cast<const IO *>(a.X) + (size_t)j * N * d;
                // staging and fill: gram_long_kernel's, statement for statement (K must have its bits); a copy because
                // the shared helper measured slower (profiles/long_shared_solve_ab.txt)
                auto stage_x = [&](int a0) {
                    for (int e = lane; e < (nrow + 1) * d; e += kWave) {
                        const int k = e / d;
                        xs[e] = (double)xi[(size_t)min(a0 + k, M - 1) * d + (e - k * d)];
                    }
                };
                auto fill = [&](int a0, int b_lo, int b_hi) {
                    __syncthreads(); // (the sweep's reads of the slots this overwrites are done; xs is staged)
                    for (int b0 = b_lo; b0 <= b_hi; b0 += kWave - 1) {
                        const int b = b0 + lane;
                        const bool ok = lane < kWave - 1 && b <= b_hi;
                        const IO *yb = yj + (size_t)min(b, N - 1) * d;
                        double yv[16];
#pragma unroll
                        for (int cc = 0; cc < 16; ++cc) yv[cc] = (double)yb[min(cc, d - 1)];
                        double rd_prev = 0.0;
                        for (int k = 0; k <= nrow; ++k) {
                            const double g = d <= 16 ? static_k16<KIND>(xs + k * d, yv, d, a.inv_h)
                                                     : static_k<KIND>(xs + k * d, yb, d, a.inv_h);
                            const double rd = shfl_down_f64(g) - g; // k(x_{a0+k}, y_{b+1}) - k(x_{a0+k}, y_b)
                            if (k >= 1 && ok) ring[(k - 1) * W + (b & (W - 1))] = (a0 + k < M) ? rd - rd_prev : 0.0;
                            rd_prev = rd;
                        }
                    }
                    __syncthreads();
                };

                const double Kval = ring_forward<NAIVE, true>(rw, fill, stage_x);
                if (((rw.P - 1) & (kWave - 1)) == lane) {
                    static_cast<IO *>(a.K_out)[(size_t)i * a.A + j] = (IO)Kval;
                    static_cast<IO *>(a.K_out)[(size_t)j * a.A + i] = (IO)Kval; // the mirror: same bits
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the forward solution is in L2 before it is read back
                __syncthreads();
                ring_reverse<NAIVE>(rw, fill, stage_x);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // S is in L2 before it is read back
                __syncthreads();

                // ---- gradient: both sides from the pair's one S, each into its slab in the item's pair order ----------------
                double w = GO ? (double)GO[(size_t)i * a.A + j] : 1.0; // the row side's weight
                double wc = GO ? (double)GO[(size_t)j * a.A + i] : 1.0; // the column side is d k(X_j, X_i) / d X_j
                if (a.sym) w = wc = w + wc;
                double *rs = rowslabs + ((size_t)(i - i0) * nck + c) * TD, *cs = colslabs + (size_t)(j - i0) * TD;
                static_grad_pass<KIND, true>(rw, xi, M, yj, N, d, a.inv_h, [&](int m, int cc, double g) {
                    double *o = rs + (size_t)m * d + cc;
                    *o = j == jfirst ? w * g : __builtin_fma(w, g, *o);
                });
                if (i != j) // (a diagonal pair has one slot: the row side took it)
                    static_grad_pass<KIND, false>(rw, yj, N, xi, M, d, a.inv_h, [&](int nn, int cc, double g) {
                        double *o = cs + (size_t)nn * d + cc;
                        *o = i == i0 ? wc * g : __builtin_fma(wc, g, *o);
                    });
                __syncthreads(); // (the next pair's forward sweep overwrites the scratch and the ring)
            }
        }
    }
}

namespace {
// the kernel families of this file for ring_launch (ring_sweep.h); id: the family's number in long_matern_launch, bandwidth: a
// family of the bandwidth launches (always the reverse sweep, kinds that have a bandwidth)
template <bool PAIRED>
struct LongFamily {
    using Args = std::conditional_t<PAIRED, PairArgs, LongArgs>;
    static constexpr bool has_kind = true, has_fwd_only = true, bandwidth = false;
    static constexpr int id = PAIRED ? 1 : 0;
    static constexpr const char *attr_failed = PAIRED ? "hipFuncSetAttribute(gram_long paired)"
                                                      : "hipFuncSetAttribute(gram_long)";
    static constexpr const char *launch_failed = PAIRED ? "launch gram_long_kernel (paired)" : "launch gram_long_kernel";
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long_kernel<IO, NAIVE, GRAD, KIND, PAIRED>; }
};
struct Long2Family {
    using Args = Long2Args;
    static constexpr bool has_kind = true, has_fwd_only = true, bandwidth = false;
    static constexpr int id = 2;
    static constexpr const char *attr_failed = "hipFuncSetAttribute(gram_long2)", *launch_failed = "launch gram_long2_kernel";
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long2_kernel<IO, NAIVE, GRAD, KIND>; }
};
// the bandwidth launches (always with the reverse sweep; RBF and the radial kinds: bw_launch below names their instantiations)
struct PairHFamily {
    using Args = PairHArgs;
    static constexpr bool bandwidth = true;
    static constexpr int id = 3;
    static constexpr const char *attr_failed = "hipFuncSetAttribute(gram_long paired, bandwidth)",
                                *launch_failed = "launch gram_long_kernel (paired, bandwidth)";
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long_kernel<IO, NAIVE, true, KIND, true, true>; }
};
struct Long2HFamily {
    using Args = Long2HArgs;
    static constexpr bool bandwidth = true;
    static constexpr int id = 4;
    static constexpr const char *attr_failed = "hipFuncSetAttribute(gram_long2, bandwidth)",
                                *launch_failed = "launch gram_long2_kernel (bandwidth)";
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long2_kernel<IO, NAIVE, true, KIND, true>; }
};
struct PartFamily { // (always with the gradient)
    using Args = PartArgs;
    static constexpr bool has_kind = true, has_fwd_only = false, bandwidth = false;
    static constexpr int id = 5;
    static constexpr const char *attr_failed = "hipFuncSetAttribute(gram_long_part)",
                                *launch_failed = "launch gram_long_part_kernel";
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel()
    {
        static_assert(GRAD, "gram_long_part_kernel has no forward-only form");
        return &gram_long_part_kernel<IO, NAIVE, KIND>;
    }
};
} // namespace

// The Matern kinds' instantiations of every family above compile in a translation unit of their own,
// gram_long_matern.hip, which includes this file with SIGSVGD_GRAM_LONG_MATERN defined and builds the kernels, the families and
// this one function: the launch of family `family` (F::id) at the plan's grid and LDS bytes, default stencil only; args: the
// family's F::Args.  Everything else of this file is the other translation unit's.
hipError_t long_matern_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                              const void *args);
#ifdef SIGSVGD_GRAM_LONG_MATERN
namespace {
struct MaternPlan {
    int grid;
    size_t lds;
};
template <typename F, typename IO>
hipError_t matern_launch_io(int kind, bool grad, const MaternPlan &pl, hipStream_t stream, const typename F::Args &a)
{
    if constexpr (F::bandwidth)
        return kind == SIGSVGD_STATIC_MATERN32 ? ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_MATERN32>(pl, stream, a)
                                               : ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_MATERN52>(pl, stream, a);
    else
        return kind == SIGSVGD_STATIC_MATERN32 ? ring_launch_solver<F, IO, SIGSVGD_STATIC_MATERN32>(false, grad, pl, stream, a)
                                               : ring_launch_solver<F, IO, SIGSVGD_STATIC_MATERN52>(false, grad, pl, stream, a);
}
template <typename F>
hipError_t matern_launch_family(int dtype, int kind, bool grad, const MaternPlan &pl, hipStream_t stream, const void *args)
{
    const typename F::Args &a = *static_cast<const typename F::Args *>(args);
    return dtype == SIGSVGD_F64 ? matern_launch_io<F, double>(kind, grad, pl, stream, a)
                                : matern_launch_io<F, float>(kind, grad, pl, stream, a);
}
} // namespace
hipError_t long_matern_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                              const void *args)
{
    if (kind != SIGSVGD_STATIC_MATERN32 && kind != SIGSVGD_STATIC_MATERN52) return hipErrorInvalidValue;
    const MaternPlan pl{grid, lds};
    switch (family) {
    case LongFamily<false>::id: return matern_launch_family<LongFamily<false>>(dtype, kind, grad, pl, stream, args);
    case LongFamily<true>::id: return matern_launch_family<LongFamily<true>>(dtype, kind, grad, pl, stream, args);
    case Long2Family::id: return matern_launch_family<Long2Family>(dtype, kind, grad, pl, stream, args);
    case PairHFamily::id: return matern_launch_family<PairHFamily>(dtype, kind, grad, pl, stream, args);
    case Long2HFamily::id: return matern_launch_family<Long2HFamily>(dtype, kind, grad, pl, stream, args);
    case PartFamily::id: return matern_launch_family<PartFamily>(dtype, kind, grad, pl, stream, args);
    }
    return hipErrorInvalidValue;
}
#else

// grad_partial[k][e] (fp64, whatever the I/O dtype) = row k's column-side slabs in the order of the owned tiles, then, where
// the launch owns k's tile, its row-side slabs in chunk order; slabs no pair wrote are skipped (the column side of a tile's
// first row; chunks that end at or before the diagonal), and a row that received nothing gets zero.  One block per row.
__global__ void long_part_reduce_kernel(const double *rowpart, const double *colpart, double *out, int A, int TD, int R, int JC,
                                        TileMap tm)
{
    const int k = blockIdx.x;
    const int own = tm.kq_of_tile(k / R);
    int oi0 = 0, onc = 0;
    const double *rows = nullptr;
    if (own >= 0) {
        oi0 = tm.tile_of(own) * R;
        onc = part_chunks(tm, own, A, R, JC);
        rows = rowpart + ((size_t)part_row_base(tm, own, A, R, JC) + (size_t)(k - oi0) * onc) * TD;
    }
    for (int e = threadIdx.x; e < TD; e += blockDim.x) {
        double s = 0.0;
        for (int kq = 0; kq < tm.owned; ++kq) {
            const int i0 = tm.tile_of(kq) * R;
            if (i0 < k) s += colpart[(size_t)(tm.start(kq, A, R, 1) + (k - i0)) * TD + e];
        }
        for (int c = 0; c < onc; ++c)
            if (oi0 + (c + 1) * JC > k) s += rows[(size_t)c * TD + e];
        out[(size_t)k * TD + e] = s;
    }
}

// out[k][e] = sum over slab c of partials[k][c][e], c = 0 .. nslabs - 1 in order (reproducible bits).  skip > 0 (yx): row k's
// column-side slab of its own diagonal tile, c = k / skip, was never written when k is that tile's first row (no pair i < k
// in it), and is left out.
template <typename IO>
__global__ void long2_reduce_kernel(const double *partials, IO *out, int rows, int nslabs, int TD, int skip)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)rows * TD) return;
    const size_t k = idx / TD, e = idx % TD;
    const int none = skip > 0 && k % skip == 0 ? (int)(k / skip) : -1;
    double s = 0.0;
    for (int c = 0; c < nslabs; ++c)
        if (c != none) s += partials[(k * nslabs + c) * TD + e];
    out[idx] = (IO)s;
}

namespace {
struct LongPlan : RingPlan {
    int JC, nchunks, grid;
    long long items;
    size_t wsk_bytes, partial_bytes, col_bytes = 0; // the forward scratch, the row-side slabs, the column-side slabs
    size_t total() const { return ring_ws_total(wsk_bytes + partial_bytes + col_bytes); }
};

// The grid of a launch of pl.items work items and its forward scratch: one wavefront per item up to what the device holds,
// fewer (at least one) where their scratch would pass kRingMaxScratch; the scratch is rounded to 256 B.
void long_set_grid(LongPlan &pl)
{
    long long grid = pl.resident < pl.items ? pl.resident : pl.items;
    if (pl.per_wave * (size_t)grid > kRingMaxScratch) { // (per_wave is 0 for forward-only launches)
        grid = (long long)(kRingMaxScratch / pl.per_wave);
        if (grid < 1) grid = 1;
    }
    pl.grid = (int)grid;
    pl.wsk_bytes = ((pl.per_wave * (size_t)grid) + 255) & ~(size_t)255;
}

int long_make_plan(int A, int B, int M, int N, int d, int n, int want_grad, LongPlan &pl, const char *who = "gram_long")
{
    const int rc = ring_make_plan(M, N, n, want_grad, d, who, pl); // (+ the band's nrow + 1 points of X_i in LDS)
    if (rc) return rc;
    // work items (i, chunk of JC columns): enough to give every resident wave one, few enough gradient slabs
    int JC = 32;
    while (JC > 1 && (long long)A * ((B + JC - 1) / JC) < pl.resident) JC >>= 1;
    pl.JC = JC;
    pl.nchunks = (B + JC - 1) / JC;
    pl.items = (long long)A * pl.nchunks;
    long_set_grid(pl);
    pl.partial_bytes = want_grad ? (size_t)A * pl.nchunks * M * d * sizeof(double) : 0;
    return SIGSVGD_OK;
}

// the paired plan: the Gram plan of one column (items = A pairs, one per wavefront, grid = min(resident waves, A), the same
// LDS, cell limits and 1 GiB scratch cap); the gradients are written straight to the outputs, so there are no slabs
int pair_make_plan(int A, int M, int N, int d, int n, int want_grad, LongPlan &pl)
{
    const int rc = long_make_plan(A, 1, M, N, d, n, want_grad, pl, "pair");
    if (rc) return rc;
    pl.JC = 1;
    pl.partial_bytes = 0;
    return SIGSVGD_OK;
}

// The two-sided plan: tiles of IC rows x JC columns, the largest powers of two <= 32 that still give every resident wave an
// item (the wider side is halved first); yx: square tiles of the upper triangle.  Slabs: a row has one per column tile, a
// column one per row tile, so their bytes are (A ntj TX + B nti TY) d 8 at most; yx keeps the nti + 1 slabs a row can have
// (column side: tile rows 0 .. its own, row side: its own .. nti - 1) in one array.
struct Long2Plan : LongPlan {
    int IC, nti;
};

// want_bw (the bandwidth launch): the per-wave scratch of a reverse sweep whatever gradients are wanted, and nothing else.
int long2_make_plan(int A, int B, int M, int N, int d, int n, bool want_row, bool want_col, bool yx, Long2Plan &pl,
                    bool want_bw = false)
{
    const int want_grad = want_row || want_col;
    const int rc = ring_make_plan(M, N, n, want_grad || want_bw, d, "gram_long", pl);
    if (rc) return rc;
    auto tiles = [](int rows, int chunk) { return (rows + chunk - 1) / chunk; };
    int IC = 32, JC = 32;
    if (yx) {
        auto tri = [&](int c) { return (long long)tiles(A, c) * (tiles(A, c) + 1) / 2; };
        while (IC > 1 && tri(IC) < pl.resident) IC >>= 1;
        JC = IC;
        pl.items = tri(IC);
    } else {
        while ((IC > 1 || JC > 1) && (long long)tiles(A, IC) * tiles(B, JC) < pl.resident) {
            if (JC >= IC)
                JC >>= 1;
            else
                IC >>= 1;
        }
        pl.items = (long long)tiles(A, IC) * tiles(B, JC);
    }
    pl.IC = IC;
    pl.JC = JC;
    pl.nti = tiles(A, IC);
    pl.nchunks = tiles(B, JC);
    long_set_grid(pl);
    const size_t rowslabs = yx ? (want_grad ? pl.nti + 1 : 0) : (want_row ? pl.nchunks : 0);
    pl.partial_bytes = (size_t)A * rowslabs * M * d * sizeof(double);
    pl.col_bytes = !yx && want_col ? (size_t)B * pl.nti * N * d * sizeof(double) : 0;
    return SIGSVGD_OK;
}

// ---- the partial plan ------------------------------------------------------------------------------
// One rank's share under a candidate (R, JC): its pairs, the most pairs one wavefront walks when item k goes to wave
// k % grid (the kernel's persistent loop), its slabs (units of TX * d doubles) and its items.  The items are enumerated in
// the order of part_decode.
struct PartShare {
    long long pairs = 0, makespan = 0, slabs = 0, items = 0, nfull = 0;
    TileMap tm;
};
PartShare part_share(int A, int R, int JC, int off, int stride, bool fold, long long resident)
{
    PartShare sh;
    sh.tm = make_tilemap((A + R - 1) / R, off, stride, fold);
    const TileMap &tm = sh.tm;
    for (int kq = 0; kq < tm.owned; ++kq) {
        const int nc = part_chunks(tm, kq, A, R, JC);
        sh.items += nc;
        sh.nfull += nc > 2 ? nc - 2 : 0;
        sh.slabs += (long long)part_rows(tm, kq, A, R) * nc + (A - tm.tile_of(kq) * R);
    }
    const long long grid = sh.items < resident ? (sh.items > 0 ? sh.items : 1) : resident;
    std::vector<long long> load((size_t)grid, 0);
    long long k = 0;
    auto take = [&](int kq, int c) {
        const int i0 = tm.tile_of(kq) * R, i1 = std::min(A, i0 + R), j0 = i0 + c * JC, j1 = std::min(A, j0 + JC);
        long long p = 0;
        for (int i = i0; i < i1; ++i) p += std::max(0, j1 - std::max(j0, i));
        sh.pairs += p;
        load[(size_t)(k++ % grid)] += p;
    };
    for (int kq = 0; kq < tm.owned; ++kq)
        for (int c = 1; c < part_chunks(tm, kq, A, R, JC) - 1; ++c) take(kq, c);
    for (int kq = 0; kq < tm.owned; ++kq) take(kq, 0);
    for (int kq = 0; kq < tm.owned; ++kq)
        if (part_chunks(tm, kq, A, R, JC) >= 2) take(kq, part_chunks(tm, kq, A, R, JC) - 1);
    sh.makespan = *std::max_element(load.begin(), load.end());
    return sh;
}

// The item rule: the largest R * JC (R a power of two <= 32 with at least two row tiles per rank, JC <= 64; ties: the larger
// R) under which, for every rank of `stride` with folded ownership,
//   schedule  ceil(pairs / resident) / makespan >= 0.9,
//   memory    slabs <= A * A / 4 where the share holds more than 16 pairs per resident wave, else <= 2 pairs + A (what
//             single-pair items cost),
//   balance   the fullest rank's pairs <= 1.05 x the mean.
// A share of no more pairs than resident waves gets single pairs by the schedule condition alone.  Where nothing meets all
// three (few rows on many ranks), the memory condition holds and the best balance, then schedule, is taken.  It depends on
// (A, stride, resident) only -- never on the rank -- and is searched once per such triple and process.
void part_pick(int A, int stride, long long resident, int &R_out, int &JC_out)
{
    static std::mutex mu;
    static std::map<std::tuple<int, int, long long>, std::pair<int, int>> cache;
    const auto key = std::make_tuple(A, stride, resident);
    std::lock_guard<std::mutex> lock(mu);
    const auto hit = cache.find(key);
    if (hit != cache.end()) {
        R_out = hit->second.first;
        JC_out = hit->second.second;
        return;
    }
    std::vector<std::pair<int, int>> cands;
    for (int R = 32; R >= 1; R >>= 1)
        for (int JC = 64; JC >= 1; --JC) cands.emplace_back(R, JC);
    std::stable_sort(cands.begin(), cands.end(), [](const std::pair<int, int> &x, const std::pair<int, int> &y) {
        return x.first * x.second > y.first * y.second;
    });
    const long long total = (long long)A * (A + 1) / 2;
    std::pair<int, int> best{1, 1};
    bool have = false, best_bal = false;
    double best_eff = -1.0;
    for (const auto &cd : cands) {
        const int R = cd.first, JC = cd.second;
        if (R > 1 && (A + R - 1) / R < 2 * stride) continue;
        bool mem_ok = true;
        double eff = 1.0;
        long long most = 0;
        for (int off = 0; off < stride && mem_ok; ++off) {
            const PartShare sh = part_share(A, R, JC, off, stride, true, resident);
            const long long bound = sh.pairs > 16 * resident ? (long long)A * A / 4 : 2 * sh.pairs + A;
            mem_ok = sh.slabs <= bound;
            if (sh.pairs > 0) eff = std::min(eff, (double)((sh.pairs + resident - 1) / resident) / (double)sh.makespan);
            most = std::max(most, sh.pairs);
        }
        if (!mem_ok) continue;
        const bool bal = (double)most * stride <= 1.05 * (double)total;
        if (eff >= 0.9 && bal) {
            best = cd;
            break;
        }
        if (!have || (bal && !best_bal) || (bal == best_bal && eff > best_eff)) {
            have = true;
            best = cd;
            best_bal = bal;
            best_eff = eff;
        }
    }
    cache[key] = best;
    R_out = best.first;
    JC_out = best.second;
}

struct PartPlan : LongPlan {
    int R;
    TileMap tm;
    long long nfull;
};

// the plan of rank `off` of `stride`; off < 0: the tile size only (sigsvgd_gram_long_partial_plan)
int part_make_plan(int A, int T, int d, int n, int off, int stride, bool fold, PartPlan &pl)
{
    const int rc = ring_make_plan(T, T, n, 1, d, "gram_long", pl);
    if (rc) return rc;
    part_pick(A, stride, pl.resident, pl.R, pl.JC);
    if (off < 0) return SIGSVGD_OK;
    const PartShare sh = part_share(A, pl.R, pl.JC, off, stride, fold, pl.resident);
    pl.tm = sh.tm;
    pl.items = sh.items;
    pl.nfull = sh.nfull;
    pl.nchunks = 0;
    long_set_grid(pl);
    const size_t TD = (size_t)T * d;
    pl.col_bytes = (size_t)sh.tm.start(sh.tm.owned, A, pl.R, 1) * TD * sizeof(double);
    pl.partial_bytes = (size_t)sh.slabs * TD * sizeof(double) - pl.col_bytes;
    return SIGSVGD_OK;
}

// The arguments every mode takes from the problem, its plan and the caller's workspace (checked against the plan's total; the
// row-side slabs follow the forward scratch).  B: the columns of the launch (1 in the paired mode).
int long_args(const char *who, const LongPlan &pl, const LongProblem &p, int B, LongArgs &a)
{
    unsigned char *base = nullptr;
    const int rc = ring_ws_base(who, p.ws, p.ws_bytes, pl.total(), base);
    if (rc) return rc;
    a.X = p.X; a.Y = p.Y; a.grad_out = p.grad_out; a.K_out = p.K_out;
    a.wsk = reinterpret_cast<float *>(base);
    a.partials = pl.partial_bytes ? reinterpret_cast<double *>(base + pl.wsk_bytes) : nullptr;
    a.wsk_per_block = pl.per_wave / sizeof(float);
    a.A = p.A; a.B = B; a.M = p.TX; a.N = p.TY; a.d = p.d; a.n = p.n; a.r = pl.r; a.P = pl.P; a.Q = pl.Q;
    a.nbands = pl.nbands; a.nsteps = pl.nsteps; a.nrow = pl.nrow; a.W = pl.W; a.JC = pl.JC; a.nchunks = pl.nchunks;
    a.sym = (p.flags & SIGSVGD_FLAG_SYM) ? 1 : 0; a.items = pl.items; a.inv_h = p.inv_h;
    a.inv_r2 = 1.0 / ((double)pl.r * (double)pl.r);
    return SIGSVGD_OK;
}
// the column-side slabs of the two-sided and partial modes: behind the forward scratch and the row-side slabs
double *long_colpart(const LongPlan &pl, const LongArgs &a)
{
    return pl.col_bytes ? reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(a.wsk) + pl.wsk_bytes + pl.partial_bytes)
                        : nullptr;
}
bool long_naive(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_NAIVE_SOLVER) != 0; }
bool long_yx(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_Y_IS_X) != 0; }
bool long_fold(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_FOLD_TILES) != 0; }

// out (the launch's dtype) = the sums of `rows` rows' slabs, long2_reduce_kernel
int long2_reduce(const LongProblem &p, const double *partials, void *out, int rows, int nslabs, int TD, int skip,
                 const char *what)
{
    const int bs = 256;
    const unsigned gs = (unsigned)(((size_t)rows * TD + bs - 1) / bs);
    if (p.dtype == SIGSVGD_F64)
        hipLaunchKernelGGL(long2_reduce_kernel<double>, dim3(gs), dim3(bs), 0, p.stream, partials, static_cast<double *>(out),
                           rows, nslabs, TD, skip);
    else
        hipLaunchKernelGGL(long2_reduce_kernel<float>, dim3(gs), dim3(bs), 0, p.stream, partials, static_cast<float *>(out),
                           rows, nslabs, TD, skip);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? hip_fail(e, what) : SIGSVGD_OK;
}

// ring_launch for the bandwidth families: the kinds that have a bandwidth, the first-order stencil where the route has it (RBF)
template <typename F, typename IO, typename Plan>
hipError_t bw_launch_kind(int kind, bool naive, const Plan &pl, hipStream_t stream, const typename F::Args &a)
{
    if (kind == SIGSVGD_STATIC_IMQ || kind == SIGSVGD_STATIC_RQ) {
        if (naive) return hipErrorInvalidValue; // (the entry points refuse it before this)
        return kind == SIGSVGD_STATIC_IMQ ? ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_IMQ>(pl, stream, a)
                                          : ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_RQ>(pl, stream, a);
    }
    if (kind != SIGSVGD_STATIC_RBF) return hipErrorInvalidValue;
    return naive ? ring_launch_one<F, IO, true, true, SIGSVGD_STATIC_RBF>(pl, stream, a)
                 : ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_RBF>(pl, stream, a);
}
template <typename F, typename Plan>
int bw_launch(int dtype, int kind, bool naive, const Plan &pl, hipStream_t stream, const typename F::Args &a)
{
    hipError_t e = dtype == SIGSVGD_F64 ? bw_launch_kind<F, double>(kind, naive, pl, stream, a)
                                        : bw_launch_kind<F, float>(kind, naive, pl, stream, a);
    if (e != hipSuccess) return hip_fail(e, F::attr_failed);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, F::launch_failed);
    return SIGSVGD_OK;
}
// the launch of family F: ring_launch or bw_launch, and for the Matern kinds gram_long_matern.hip's instantiations
template <typename F, typename Plan>
int family_launch(int dtype, int kind, bool naive, bool grad, const Plan &pl, hipStream_t stream, const typename F::Args &a)
{
    if (kind != SIGSVGD_STATIC_MATERN32 && kind != SIGSVGD_STATIC_MATERN52) {
        if constexpr (F::bandwidth)
            return bw_launch<F>(dtype, kind, naive, pl, stream, a);
        else
            return ring_launch<F>(dtype, kind, naive, grad, pl, stream, a);
    }
    // (the entry points refuse NAIVE_SOLVER with these kinds before this)
    hipError_t e = naive ? hipErrorInvalidValue : long_matern_launch(F::id, dtype, kind, grad, pl.grid, pl.lds, stream, &a);
    if (e != hipSuccess) return hip_fail(e, F::attr_failed);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, F::launch_failed);
    return SIGSVGD_OK;
}
} // namespace

// ---- workspace queries and launches; the argument checks are the entry points' (capi.hip) ----------------------------------
// Bytes of a launch's workspace (0 for forward-only launches: the forward sweep keeps nothing; 0 for a rank of the partial mode
// that owns no tile).  The queries read the problem's shape, order and flags only.
int long_workspace(const LongProblem &p, int want_grad, size_t *bytes)
{
    return ring_plan_total<LongPlan>(
        bytes, [&](LongPlan &pl) { return long_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_grad, pl); });
}
int pair_workspace(const LongProblem &p, int want_grad, size_t *bytes)
{
    return ring_plan_total<LongPlan>(
        bytes, [&](LongPlan &pl) { return pair_make_plan(p.A, p.TX, p.TY, p.d, p.n, want_grad, pl); });
}
int long2_workspace(const LongProblem &p, int want_gradX, int want_gradY, size_t *bytes)
{
    return ring_plan_total<Long2Plan>(bytes, [&](Long2Plan &pl) {
        return long2_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_gradX != 0, want_gradY != 0, long_yx(p), pl);
    });
}
// the two-sided bandwidth launch: the scratch also where neither coordinate gradient is wanted (the paired one's workspace is
// pair_workspace's with the gradient: the scratch alone)
int long2_h_workspace(const LongProblem &p, int want_gradX, int want_gradY, size_t *bytes)
{
    return ring_plan_total<Long2Plan>(bytes, [&](Long2Plan &pl) {
        return long2_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_gradX != 0, want_gradY != 0, long_yx(p), pl, true);
    });
}
int long_part_workspace(const LongProblem &p, int off, int stride, size_t *bytes)
{
    return ring_plan_total<PartPlan>(
        bytes, [&](PartPlan &pl) { return part_make_plan(p.A, p.TX, p.d, p.n, off, stride, long_fold(p), pl); });
}
// the partial mode's tile: R rows x JC columns, the same for every rank of `stride` (host only)
int long_part_tiles(const LongProblem &p, int stride, int *R, int *JC)
{
    PartPlan pl;
    const int rc = part_make_plan(p.A, p.TX, p.d, p.n, -1, stride, true, pl);
    if (rc) return rc;
    *R = pl.R;
    *JC = pl.JC;
    return SIGSVGD_OK;
}

// gradX_out == NULL: forward only
int long_launch(const LongProblem &p)
{
    const bool want_grad = p.gradX_out != nullptr;
    LongPlan pl;
    LongArgs a;
    int rc = long_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_grad, pl);
    if (!rc) rc = long_args("gram_long", pl, p, p.B, a);
    if (!rc) rc = family_launch<LongFamily<false>>(p.dtype, p.kind, long_naive(p), want_grad, pl, p.stream, a);
    if (!rc && want_grad) // a row's slabs in chunk order
        rc = long2_reduce(p, a.partials, p.gradX_out, p.A, pl.nchunks, p.TX * p.d, 0, "launch long2_reduce_kernel (rows)");
    return rc;
}

// ---- the paired mode's schedule: one wavefront per pair (gram_long_kernel) or a workgroup per pair (pair_bands.hip) --------
namespace {
PairGeom pair_geom(const LongPlan &pl)
{
    return PairGeom{pl.r, pl.P, pl.Q, pl.nbands, pl.nsteps, pl.nrow, pl.grid, pl.per_wave / sizeof(float)};
}
// Whether a paired launch runs the band-parallel kernel under plan bp.  SIGSVGD_PAIR_MODE=serial|bands (read per launch; tests
// and measurements only, the results have the same bits; any other value is ignored) pins it wherever the plan has two waves
// or more.  Default rule: bands where its dependent steps, over the rounds the launch takes, are
// fewer than a third of the serial schedule's,
//   3 * rounds_bands * phases * 16  <  rounds_serial * nbands * nsteps,      rounds = ceil(A / workgroups or waves in flight).
// The 3 is the measured cost of a band-parallel step against a serial one (2.2 - 2.6: two waves share a SIMD, and a barrier
// every 16 steps), rounded up.  Few bands per pair, or pairs enough to fill the device in both schedules, stay serial.
bool pair_use_bands(int A, const LongPlan &pl, const PairBandsPlan &bp)
{
    if (bp.NB < 2) return false;
    const char *e = getenv("SIGSVGD_PAIR_MODE");
    if (e && !strcmp(e, "serial")) return false;
    if (e && !strcmp(e, "bands")) return true;
    const long long rounds_b = (A + bp.grid - 1) / bp.grid, rounds_s = (A + pl.grid - 1) / pl.grid;
    return 3 * rounds_b * bp.phases * 16 < rounds_s * (long long)pl.nbands * pl.nsteps;
}
} // namespace

// what a paired launch would run now (host only): waves per pair, workgroups, LDS bytes per workgroup
int pair_schedule(const LongProblem &p, int want_grad, int *waves_per_pair, int *grid, size_t *lds_bytes)
{
    LongPlan pl;
    const int rc = pair_make_plan(p.A, p.TX, p.TY, p.d, p.n, want_grad, pl);
    if (rc) return rc;
    PairBandsPlan bp;
    pair_bands_plan(p.A, p.TX, p.TY, p.d, p.n, pair_geom(pl), bp);
    const bool bands = pair_use_bands(p.A, pl, bp);
    *waves_per_pair = bands ? bp.NB : 1;
    *grid = bands ? bp.grid : pl.grid;
    *lds_bytes = bands ? bp.lds : pl.lds;
    return SIGSVGD_OK;
}

// gradX_out and gradY_out both NULL: forward only
int pair_launch(const LongProblem &p)
{
    const bool want_grad = p.gradX_out != nullptr || p.gradY_out != nullptr;
    LongPlan pl;
    PairArgs a;
    int rc = pair_make_plan(p.A, p.TX, p.TY, p.d, p.n, want_grad, pl);
    if (!rc) rc = long_args("pair", pl, p, 1, a);
    if (rc) return rc;
    PairBandsPlan bp;
    pair_bands_plan(p.A, p.TX, p.TY, p.d, p.n, pair_geom(pl), bp);
    if (pair_use_bands(p.A, pl, bp)) return pair_bands_launch(p, pair_geom(pl), bp, a.wsk); // the same scratch slots, fewer used
    a.gradX = p.gradX_out; a.gradY = p.gradY_out;
    return family_launch<LongFamily<true>>(p.dtype, p.kind, long_naive(p), want_grad, pl, p.stream, a);
}

// The paired launch with the bandwidth derivative: dk_out[A] = dK_i / d inv_h.  Always the one-wavefront
// schedule (pair_bands.hip has no bandwidth pass) with the reverse sweep; gradX_out and gradY_out may both be NULL.
int pair_h_launch(const LongProblem &p, void *dk_out)
{
    LongPlan pl;
    PairHArgs a;
    int rc = pair_make_plan(p.A, p.TX, p.TY, p.d, p.n, 1, pl);
    if (!rc) rc = long_args("pair", pl, p, 1, a);
    if (rc) return rc;
    a.gradX = p.gradX_out; a.gradY = p.gradY_out; a.dK_dinvh = dk_out;
    return family_launch<PairHFamily>(p.dtype, p.kind, long_naive(p), true, pl, p.stream, a);
}

// The two-sided launch, with the bandwidth derivative where dk_out is given (dk_out[A][B] =
// dK_ij / d inv_h; the reverse sweep then runs whatever gradients are wanted, and the plan of the gradients' slabs and tiles is
// the one the launch without dk_out makes).
// gradX_out and gradY_out both NULL: forward only.  Y_IS_X: A == B, TX == TY, no gradY_out; gradX_out then gets both sides of
// every unordered pair.
namespace {
template <bool BW>
int long2_launch_any(const LongProblem &p, void *dk_out)
{
    const bool yx = long_yx(p), want_row = p.gradX_out != nullptr, want_col = p.gradY_out != nullptr || (yx && want_row);
    Long2Plan pl;
    std::conditional_t<BW, Long2HArgs, Long2Args> a;
    int rc = long2_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_row, p.gradY_out != nullptr, yx, pl, BW);
    if (!rc) rc = long_args("gram_long", pl, p, p.B, a);
    if (rc) return rc;
    a.colpart = long_colpart(pl, a);
    a.IC = pl.IC; a.nti = pl.nti; a.yx = yx ? 1 : 0; a.want_row = want_row ? 1 : 0; a.want_col = want_col ? 1 : 0;
    if constexpr (BW) {
        a.dK_dinvh = dk_out;
        rc = family_launch<Long2HFamily>(p.dtype, p.kind, long_naive(p), true, pl, p.stream, a);
    } else {
        rc = family_launch<Long2Family>(p.dtype, p.kind, long_naive(p), want_row || want_col, pl, p.stream, a);
    }
    if (!rc && want_row) // yx: a row's nti + 1 slabs, column side first
        rc = long2_reduce(p, a.partials, p.gradX_out, p.A, yx ? pl.nti + 1 : pl.nchunks, p.TX * p.d, yx ? pl.IC : 0,
                          "launch long2_reduce_kernel (rows)");
    if (!rc && p.gradY_out)
        rc = long2_reduce(p, a.colpart, p.gradY_out, p.B, pl.nti, p.TY * p.d, 0, "launch long2_reduce_kernel (columns)");
    return rc;
}
} // namespace
int long2_launch(const LongProblem &p) { return long2_launch_any<false>(p, nullptr); }
int long2_h_launch(const LongProblem &p, void *dk_out) { return long2_launch_any<true>(p, dk_out); }

// The share of rank `off` of `stride` (Y = X: B = A, TY = TX).  K_out gets the owned pairs and their mirror images, gradX_out
// (fp64 whatever the dtype) is overwritten whole; a rank that owns no tile launches the reduction alone, which writes zeros.
int long_part_launch(const LongProblem &p, int off, int stride)
{
    PartPlan pl;
    PartArgs a;
    int rc = part_make_plan(p.A, p.TX, p.d, p.n, off, stride, long_fold(p), pl);
    if (!rc) rc = long_args("gram_long_sym_partial", pl, p, p.A, a);
    if (rc) return rc;
    a.colpart = long_colpart(pl, a);
    a.tm = pl.tm; a.R = pl.R; a.nfull = pl.nfull;
    if (pl.items > 0) rc = family_launch<PartFamily>(p.dtype, p.kind, long_naive(p), true, pl, p.stream, a);
    if (rc) return rc;
    hipLaunchKernelGGL(long_part_reduce_kernel, dim3(p.A), dim3(256), 0, p.stream, a.partials, a.colpart,
                       static_cast<double *>(p.gradX_out), p.A, p.TX * p.d, pl.R, pl.JC, pl.tm);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch long_part_reduce_kernel");
    return SIGSVGD_OK;
}

#endif // SIGSVGD_GRAM_LONG_MATERN
} // namespace sigsvgd
