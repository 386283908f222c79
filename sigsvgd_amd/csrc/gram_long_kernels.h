// The long-path kernels (gram_long_kernel, gram_long2_kernel, gram_long_part_kernel), their argument structs and their
// families for ring_launch (ring_sweep.h).  Included by gram_long.hip (plans, reduce kernels, launchers; every kind but Matern),
// by gram_long_matern.hip (the Matern kinds' instantiations), by gram_long_exact.hip and gram_long_exact_matern.hip (the
// exact adjoint's instantiations), by gram_long_nantail.hip and gram_long_nantail_matern.hip (the
// instantiations for batches of paths of different lengths) and by gram_long_logk.hip and
// gram_long_logk_matern.hip (the log-domain instantiations), and by gram_long_norm.hip and
// gram_long_norm_matern.hip (the normalised kernel's instantiations).
//
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
// The per-pair solve (staging, fill, forward sweep, K store, reverse sweep) is written out in each of the three kernels, and K's
// bit-identity across the modes rests on the copies staying equal.  One shared function (long_solve_pair over a PairSource, with
// one two_sided_grad block) gave the same bits and the same registers, scratch and occupancy, but was measured slower on the
// MI355X: forward-only launches by 1.5-4 %, the partial kernel by 1-1.4 %, ranges of run-medians apart
// (profiles/long_shared_solve_ab.txt).  So the copies stay.
#pragma once

#include <type_traits>

#include "long_static.h"
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


// NaN-marked tails: the helpers of the NanTailIO instantiations of the two kernels below.
namespace {
// the launch's view with the geometry of a pair of Mp x Np points: the plan's LDS and scratch layout, a prefix of each used
__device__ __forceinline__ RingWave nan_tail_wave(const RingWave &rw, int Mp, int Np)
{
    RingWave w = rw;
    w.N = Np;
    w.P = rw.r * (Mp - 1);
    w.Q = rw.r * (Np - 1);
    w.nbands = (w.P + kWave - 1) / kWave;
    w.nsteps = w.Q + kWave - 1;
    return w;
}
template <bool NT>
__device__ __forceinline__ const RingWave &nan_tail_pick(const RingWave &launch, const RingWave &pair)
{
    if constexpr (NT)
        return pair;
    else
        return launch;
}
// exact zeros into rows from .. to - 1 of the [to][d] block that starts at row `row0` of out (out may be NULL: nothing)
template <typename T>
__device__ __forceinline__ void nan_tail_zero_rows(T *out, size_t row0, int from, int to, int d)
{
    if (!out) return;
    T *o = out + row0 * d;
    for (int e = from * d + (int)threadIdx.x; e < to * d; e += kWave) o[e] = (T)0;
}
} // namespace

// BW (paired mode only): after the pair's gradient passes one more pass chains the same S through the
// static kernel's derivative in the bandwidth and stores the pair's dK / d inv_h; a compile-time branch, so the instantiations
// without it keep their code.
// IOX: float, double, or ExactIO<float>, ExactIO<double> (ring_sweep.h): the sweeps of the exact adjoint
// (default stencil, gradient launches); everything behind S is the same code.  Instantiated in gram_long_exact.hip and
// gram_long_exact_matern.hip.
template <typename IOX, bool NAIVE, bool GRAD, int KIND, bool PAIRED = false, bool BW = false>
__global__ __launch_bounds__(64) void gram_long_kernel(
    std::conditional_t<BW, PairHArgs, std::conditional_t<PAIRED, PairArgs, LongArgs>> a)
{
    using IO = typename RingIO<IOX>::type;
    constexpr bool EXACT = RingIO<IOX>::exact;
    constexpr bool NT = RingIO<IOX>::nan_tails; // (the paired mode only, no bandwidth pass)
    constexpr bool LOGK = RingIO<IOX>::log_k;   // (the same; K_out gets ln K, the gradients those of ln K)
    static_assert(!BW || (PAIRED && GRAD), "the bandwidth pass needs the paired mode's reverse sweep");
    static_assert(!NT || (PAIRED && !BW), "NaN-marked tails: the paired mode without the bandwidth pass");
    // (the diagonal pass of a normalised launch, Y = X pair by pair; K_out is double[A] and gets ln K
    // unrounded, gradX double[A][TX][d] and gets the pair's unit-weight gradient in both slots, gX + gY)
    constexpr bool NORM = RingIO<IOX>::normalized;
    static_assert(!LOGK || (PAIRED && !BW), "the log-domain solve: the paired mode without the bandwidth pass");
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const int M = a.M, N = a.N, W = a.W, nrow = a.nrow, d = a.d;
    const RingWave rw = ring_wave<GRAD>(a, smem_raw);
    double *ring = rw.ring;
    double *xs = rw.dump + kWave; // [nrow + 1][d]: points a0 .. a0 + nrow of X_i (clamped to M - 1)
    const IO *GO = static_cast<const IO *>(a.grad_out);
    [[maybe_unused]] const int *lenX = nullptr, *lenY = nullptr;
    if constexpr (NT) {
        lenX = nan_tail_lengths(a.wsk, a.A, a.A);
        lenY = lenX + a.A;
    }
    [[maybe_unused]] RingLog lg;
    if constexpr (LOGK) lg = ring_log<GRAD>(a, rw, xs + (nrow + 1) * d); // (its block exponents: behind the band's points)

    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int i = PAIRED ? (int)item : (int)(item / a.nchunks);
        const int j0 = PAIRED ? i : (int)(item % a.nchunks) * a.JC, j1 = PAIRED ? i + 1 : min(a.B, j0 + a.JC);
        const IO *xi = static_cast<const IO *>(a.X) + (size_t)i * M * d;
        double *slab = GRAD && !PAIRED ? a.partials + (size_t)item * M * d : nullptr;

        for (int j = j0; j < j1; ++j) {
            const IO *yj = static_cast<const IO *>(a.Y) + (size_t)j * N * d;
            // NaN-marked tails: the pair's own lengths and grid (Mp = M, Np = N and rp = rw otherwise)
            int Mp = M, Np = N;
            [[maybe_unused]] RingWave rwl;
            if constexpr (NT) {
                Mp = __builtin_amdgcn_readfirstlane(lenX[i]);
                Np = __builtin_amdgcn_readfirstlane(lenY[j]);
                if constexpr (PAIRED) {
                    if (Mp < 2 || Np < 2) { // a one-point path: K = 1 exactly, no gradient
                        if (lane == 0) static_cast<IO *>(a.K_out)[i] = (IO)1.0;
                        if constexpr (GRAD) {
                            nan_tail_zero_rows(static_cast<IO *>(a.gradX), (size_t)i * M, 0, M, d);
                            nan_tail_zero_rows(static_cast<IO *>(a.gradY), (size_t)i * N, 0, N, d);
                        }
                        continue;
                    }
                }
                rwl = nan_tail_wave(rw, Mp, Np);
            }
            const RingWave &rp = nan_tail_pick<NT>(rw, rwl);
            // the band's points of X_i (before the band's first fill, whose barrier publishes them)
            auto stage_x = [&](int a0) {
                for (int e = lane; e < (nrow + 1) * d; e += kWave) {
                    const int k = e / d;
                    xs[e] = (double)xi[(size_t)min(a0 + k, Mp - 1) * d + (e - k * d)];
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
                    const IO *yb = yj + (size_t)min(b, Np - 1) * d;
                    // (up to 16 channels the lane's point stays in registers for the whole column: one round of loads)
                    double yv[16];
#pragma unroll
                    for (int c = 0; c < 16; ++c) yv[c] = (double)yb[min(c, d - 1)];
                    double rd_prev = 0.0;
                    for (int k = 0; k <= nrow; ++k) {
                        const double g = d <= 16 ? static_k16<KIND>(xs + k * d, yv, d, a.inv_h)
                                                 : static_k<KIND>(xs + k * d, yb, d, a.inv_h);
                        const double rd = shfl_down_f64(g) - g; // k(x_{a0+k}, y_{b+1}) - k(x_{a0+k}, y_b)
                        if (k >= 1 && ok) ring[(k - 1) * W + (b & (W - 1))] = (a0 + k < Mp) ? rd - rd_prev : 0.0;
                        rd_prev = rd;
                    }
                }
                __syncthreads();
            };

            double Kval = ring_forward<NAIVE, GRAD, EXACT, LOGK>(rp, fill, stage_x, LOGK ? &lg : nullptr);
            if constexpr (LOGK) Kval = ring_log_finish(rp, Kval, lg); // ln K
            if constexpr (NORM) {
                if (((rp.P - 1) & (kWave - 1)) == lane) static_cast<double *>(a.K_out)[i] = Kval;
            } else {
                if (((rp.P - 1) & (kWave - 1)) == lane) static_cast<IO *>(a.K_out)[PAIRED ? (size_t)i : (size_t)i * a.B + j] = (IO)Kval;
            }
            if (!GRAD) {
                __syncthreads(); // (the next pair's first fill overwrites the ring, its sweep the boundary row)
                continue;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the forward solution is in L2 before it is read back
            __syncthreads();
            ring_reverse<NAIVE, EXACT, LOGK>(rp, fill, stage_x, LOGK ? &lg : nullptr);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // S is in L2 before it is read back
            __syncthreads();

            // ---- gradient: S -> dG (4-corner scatter) -> static-kernel derivative -> gX_i (and gY_i, paired) ---------------
            double w = GO ? (double)GO[PAIRED ? (size_t)i : (size_t)i * a.B + j] : 1.0;
            if (!PAIRED && a.sym) w += GO ? (double)GO[(size_t)j * a.B + i] : 1.0;
            if constexpr (NORM) { // (M == N: a point's entry has the same lane in both passes, which adds to its own store)
                double *gD = static_cast<double *>(a.gradX);
                static_grad_pass<KIND, true>(rp, xi, Mp, yj, Np, d, a.inv_h, [&](int m, int c, double g) {
                    gD[((size_t)i * M + m) * d + c] = g;
                });
                static_grad_pass<KIND, false>(rp, yj, Np, xi, Mp, d, a.inv_h, [&](int nn, int c, double g) {
                    double *o = gD + ((size_t)i * N + nn) * d + c;
                    *o += g;
                });
            } else if constexpr (PAIRED) { // (either output skipped when NULL)
                IO *gX = static_cast<IO *>(a.gradX), *gY = static_cast<IO *>(a.gradY);
                if (gX)
                    static_grad_pass<KIND, true>(rp, xi, Mp, yj, Np, d, a.inv_h, [&](int m, int c, double g) {
                        gX[((size_t)i * M + m) * d + c] = (IO)(w * g);
                    });
                if (gY)
                    static_grad_pass<KIND, false>(rp, yj, Np, xi, Mp, d, a.inv_h, [&](int nn, int c, double g) {
                        gY[((size_t)i * N + nn) * d + c] = (IO)(w * g);
                    });
                if constexpr (NT) { // the rows past the path's end: exact zeros
                    nan_tail_zero_rows(gX, (size_t)i * M, Mp, M, d);
                    nan_tail_zero_rows(gY, (size_t)i * N, Np, N, d);
                }
                if constexpr (BW) { // (unweighted: K's own derivative)
                    const double dk = static_bw_pass<KIND>(rp, xi, Mp, yj, Np, d, a.inv_h);
                    if (lane == 0) static_cast<IO *>(a.dK_dinvh)[i] = (IO)dk;
                }
            } else { // into the item's slab, in j order
                static_grad_pass<KIND, true>(rp, xi, Mp, yj, Np, d, a.inv_h, [&](int m, int c, double g) {
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
// IOX: as in gram_long_kernel.
template <typename IOX, bool NAIVE, bool GRAD, int KIND, bool BW = false>
__global__ __launch_bounds__(64) void gram_long2_kernel(std::conditional_t<BW, Long2HArgs, Long2Args> a)
{
    using IO = typename RingIO<IOX>::type;
    constexpr bool EXACT = RingIO<IOX>::exact;
    constexpr bool NT = RingIO<IOX>::nan_tails; // (no bandwidth pass)
    constexpr bool LOGK = RingIO<IOX>::log_k;   // (the same; K_out gets ln K, the gradients those of ln K)
    static_assert(!BW || GRAD, "the bandwidth pass needs the reverse sweep");
    static_assert(!NT || !BW, "NaN-marked tails: no bandwidth pass");
    static_assert(!LOGK || !BW, "the log-domain solve: no bandwidth pass");
    // (the log-domain solve, then K_out gets K^ = exp(ln K - (a_i + b_j) / 2) and the pair's weight K^ too)
    constexpr bool NORM = RingIO<IOX>::normalized;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const int M = a.M, N = a.N, W = a.W, nrow = a.nrow, d = a.d;
    const RingWave rw = ring_wave<GRAD>(a, smem_raw);
    double *ring = rw.ring;
    double *xs = rw.dump + kWave; // [nrow + 1][d]: points a0 .. a0 + nrow of X_i (clamped to M - 1)
    const IO *GO = static_cast<const IO *>(a.grad_out);
    [[maybe_unused]] const double *lnA = nullptr, *lnB = nullptr;
    if constexpr (NORM) { // (yx: one array serves both slots)
        lnA = norm_logs(a.wsk, a.A, a.yx ? 0 : a.B);
        lnB = a.yx ? lnA : lnA + a.A;
    }
    [[maybe_unused]] const int *lenX = nullptr, *lenY = nullptr;
    if constexpr (NT) { // (yx: one array serves both slots)
        lenX = nan_tail_lengths(a.wsk, a.A, a.yx ? 0 : a.B);
        lenY = a.yx ? lenX : lenX + a.A;
    }
    [[maybe_unused]] RingLog lg;
    if constexpr (LOGK) lg = ring_log<GRAD>(a, rw, xs + (nrow + 1) * d); // (its block exponents: behind the band's points)

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
                // NaN-marked tails: the pair's own lengths and grid (Mp = M, Np = N and rp = rw otherwise)
                int Mp = M, Np = N;
                [[maybe_unused]] RingWave rwl;
                if constexpr (NT) {
                    Mp = __builtin_amdgcn_readfirstlane(lenX[i]);
                    Np = __builtin_amdgcn_readfirstlane(lenY[j]);
                    if (Mp < 2 || Np < 2) { // a one-point path: K = 1 exactly, no gradient; a slab's first pair stores it whole
                        if (lane == 0) {
                            static_cast<IO *>(a.K_out)[(size_t)i * a.B + j] = (IO)1.0;
                            if (a.yx) static_cast<IO *>(a.K_out)[(size_t)j * a.B + i] = (IO)1.0;
                        }
                        if constexpr (GRAD) {
                            if (a.want_row && j == jfirst)
                                nan_tail_zero_rows(a.partials, (a.yx ? (size_t)i * (a.nti + 1) + tj + 1 : (size_t)i * a.nchunks + tj) * M,
                                                   0, M, d);
                            if (a.want_col && !(a.yx && i == j) && i == i0)
                                nan_tail_zero_rows(a.yx ? a.partials : a.colpart,
                                                   (a.yx ? (size_t)j * (a.nti + 1) + ti : (size_t)j * a.nti + ti) * N, 0, N, d);
                        }
                        continue;
                    }
                    rwl = nan_tail_wave(rw, Mp, Np);
                }
                const RingWave &rp = nan_tail_pick<NT>(rw, rwl);
                // staging and fill: gram_long_kernel's, statement for statement (K must have its bits); a copy because
                // the shared helper measured slower (profiles/long_shared_solve_ab.txt)
                auto stage_x = [&](int a0) {
                    for (int e = lane; e < (nrow + 1) * d; e += kWave) {
                        const int k = e / d;
                        xs[e] = (double)xi[(size_t)min(a0 + k, Mp - 1) * d + (e - k * d)];
                    }
                };
                auto fill = [&](int a0, int b_lo, int b_hi) {
                    __syncthreads(); // (the sweep's reads of the slots this overwrites are done; xs is staged)
                    for (int b0 = b_lo; b0 <= b_hi; b0 += kWave - 1) {
                        const int b = b0 + lane;
                        const bool ok = lane < kWave - 1 && b <= b_hi;
                        const IO *yb = yj + (size_t)min(b, Np - 1) * d;
                        // (up to 16 channels the lane's point stays in registers for the whole column: one round of loads)
                        double yv[16];
#pragma unroll
                        for (int c = 0; c < 16; ++c) yv[c] = (double)yb[min(c, d - 1)];
                        double rd_prev = 0.0;
                        for (int k = 0; k <= nrow; ++k) {
                            const double g = d <= 16 ? static_k16<KIND>(xs + k * d, yv, d, a.inv_h)
                                                     : static_k<KIND>(xs + k * d, yb, d, a.inv_h);
                            const double rd = shfl_down_f64(g) - g; // k(x_{a0+k}, y_{b+1}) - k(x_{a0+k}, y_b)
                            if (k >= 1 && ok) ring[(k - 1) * W + (b & (W - 1))] = (a0 + k < Mp) ? rd - rd_prev : 0.0;
                            rd_prev = rd;
                        }
                    }
                    __syncthreads();
                };

                double Kval = ring_forward<NAIVE, GRAD, EXACT, LOGK>(rp, fill, stage_x, LOGK ? &lg : nullptr);
                if constexpr (LOGK) Kval = ring_log_finish(rp, Kval, lg); // ln K
                if constexpr (NORM) Kval = exp64(Kval - (0.5 * lnA[i] + 0.5 * lnB[j])); // K^, fp64 until the store rounds it
                if (((rp.P - 1) & (kWave - 1)) == lane) {
                    static_cast<IO *>(a.K_out)[(size_t)i * a.B + j] = (IO)Kval;
                    if (a.yx) static_cast<IO *>(a.K_out)[(size_t)j * a.B + i] = (IO)Kval; // the mirror: same bits
                }
                if (!GRAD) {
                    __syncthreads(); // (the next pair's first fill overwrites the ring, its sweep the boundary row)
                    continue;
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the forward solution is in L2 before it is read back
                __syncthreads();
                ring_reverse<NAIVE, EXACT, LOGK>(rp, fill, stage_x, LOGK ? &lg : nullptr);
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
                if constexpr (NORM) { // the gradients behind S are those of ln K: times K^ they are K^'s at fixed diagonals
                    // (yx: a diagonal pair's K^ is the constant 1.  Its two terms would cancel only to the fp32 rounding of the
                    // stored S, so it is left out of both: weight 0 here and in long_norm_sums' row)
                    const double u = a.yx && i == j ? 0.0 : Kval;
                    w *= u;
                    wc *= u;
                    if (lane == 0) { // U for the sums of the diagonals' terms (yx: the column side's is row j's entry)
                        double *U = norm_weights(a.wsk, a.A, a.yx ? 0 : a.B, a.A, a.B);
                        U[(size_t)i * a.B + j] = w;
                        if (a.yx) U[(size_t)j * a.B + i] = wc;
                    }
                }
                // yx: row k's slabs are [nti + 1]: the column side's of tile rows 0 .. k / IC, then the row side's
                const int TDx = M * d, TDy = N * d;
                double *rs = a.partials + (a.yx ? (size_t)i * (a.nti + 1) + tj + 1 : (size_t)i * a.nchunks + tj) * TDx;
                double *cs = a.yx ? a.partials + ((size_t)j * (a.nti + 1) + ti) * TDx
                                  : a.colpart + ((size_t)j * a.nti + ti) * TDy;
                if (a.want_row)
                    static_grad_pass<KIND, true>(rp, xi, Mp, yj, Np, d, a.inv_h, [&](int m, int c, double g) {
                        double *o = rs + (size_t)m * d + c;
                        *o = j == jfirst ? w * g : __builtin_fma(w, g, *o);
                    });
                if (a.want_col && !(a.yx && i == j)) // (a diagonal pair of yx has one slot: the row side took it)
                    static_grad_pass<KIND, false>(rp, yj, Np, xi, Mp, d, a.inv_h, [&](int nn, int c, double g) {
                        double *o = cs + (size_t)nn * d + c;
                        *o = i == i0 ? wc * g : __builtin_fma(wc, g, *o);
                    });
                if constexpr (NT) { // slabs are stored, not accumulated: their first pair stores the zeros past the path's end
                    if (a.want_row && j == jfirst) nan_tail_zero_rows(rs, 0, Mp, M, d);
                    if (a.want_col && !(a.yx && i == j) && i == i0) nan_tail_zero_rows(cs, 0, Np, N, d);
                }
                if constexpr (BW) { // (unweighted: K's own derivative)
                    const double dk = static_bw_pass<KIND>(rp, xi, Mp, yj, Np, d, a.inv_h);
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
// the exact adjoint's families: their base's arguments, ids and texts, the exact kernels (default
// stencil, always the reverse sweep)
template <bool PAIRED>
struct LongExactFamily : LongFamily<PAIRED> {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long_kernel<ExactIO<IO>, false, true, KIND, PAIRED>; }
};
struct Long2ExactFamily : Long2Family {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long2_kernel<ExactIO<IO>, false, true, KIND>; }
};
struct PairHExactFamily : PairHFamily {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long_kernel<ExactIO<IO>, false, true, KIND, true, true>; }
};
struct Long2HExactFamily : Long2HFamily {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long2_kernel<ExactIO<IO>, false, true, KIND, true>; }
};
// the launch of family `family` (F::id; not the partial mode's) with the exact kernel of `kind`, for the two units that build
// them: the unit names its kinds, K0 .. (a kind of another unit: hipErrorInvalidValue)
struct ExactPlan {
    int grid;
    size_t lds;
};
template <typename F, typename IO, int K0, int... KS>
hipError_t exact_launch_kind(int kind, const ExactPlan &pl, hipStream_t stream, const typename F::Args &a)
{
    if (kind == K0) {
        if constexpr (F::bandwidth && K0 == SIGSVGD_STATIC_LINEAR)
            return hipErrorInvalidValue; // (no bandwidth: the entry points refuse it before this)
        else
            return ring_launch_one<F, IO, false, true, K0>(pl, stream, a);
    }
    if constexpr (sizeof...(KS) > 0)
        return exact_launch_kind<F, IO, KS...>(kind, pl, stream, a);
    else
        return hipErrorInvalidValue;
}
template <typename F, int... KS>
hipError_t exact_launch_family(int dtype, int kind, const ExactPlan &pl, hipStream_t stream, const void *args)
{
    const typename F::Args &a = *static_cast<const typename F::Args *>(args);
    return dtype == SIGSVGD_F64 ? exact_launch_kind<F, double, KS...>(kind, pl, stream, a)
                                : exact_launch_kind<F, float, KS...>(kind, pl, stream, a);
}
template <int... KS>
hipError_t exact_launch_any(int family, int dtype, int kind, int grid, size_t lds, hipStream_t stream, const void *args)
{
    const ExactPlan pl{grid, lds};
    switch (family) {
    case LongFamily<false>::id: return exact_launch_family<LongExactFamily<false>, KS...>(dtype, kind, pl, stream, args);
    case LongFamily<true>::id: return exact_launch_family<LongExactFamily<true>, KS...>(dtype, kind, pl, stream, args);
    case Long2Family::id: return exact_launch_family<Long2ExactFamily, KS...>(dtype, kind, pl, stream, args);
    case PairHFamily::id: return exact_launch_family<PairHExactFamily, KS...>(dtype, kind, pl, stream, args);
    case Long2HFamily::id: return exact_launch_family<Long2HExactFamily, KS...>(dtype, kind, pl, stream, args);
    }
    return hipErrorInvalidValue;
}
// the families of launches with SIGSVGD_FLAG_NAN_TAILS: their base's arguments, ids and texts, the
// NanTailIO kernels (forward-only and gradient, both stencils where the kind has both); the Gram mode of gram_long_kernel has none
struct PairNanTailFamily : LongFamily<true> {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long_kernel<NanTailIO<IO>, NAIVE, GRAD, KIND, true>; }
};
struct Long2NanTailFamily : Long2Family {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long2_kernel<NanTailIO<IO>, NAIVE, GRAD, KIND>; }
};
// the launch of family `family` (the paired or the two-sided one) with the NanTailIO kernel of `kind`, for the two units that
// build them: the unit names its kinds, K0 .. (a kind of another unit: hipErrorInvalidValue)
template <typename F, typename IO, int K0, int... KS>
hipError_t nan_tail_launch_kind(int kind, bool naive, bool grad, const ExactPlan &pl, hipStream_t stream,
                                const typename F::Args &a)
{
    if (kind == K0) return ring_launch_solver<F, IO, K0>(naive, grad, pl, stream, a);
    if constexpr (sizeof...(KS) > 0)
        return nan_tail_launch_kind<F, IO, KS...>(kind, naive, grad, pl, stream, a);
    else
        return hipErrorInvalidValue;
}
template <typename F, int... KS>
hipError_t nan_tail_launch_family(int dtype, int kind, bool naive, bool grad, const ExactPlan &pl, hipStream_t stream,
                                  const void *args)
{
    const typename F::Args &a = *static_cast<const typename F::Args *>(args);
    return dtype == SIGSVGD_F64 ? nan_tail_launch_kind<F, double, KS...>(kind, naive, grad, pl, stream, a)
                                : nan_tail_launch_kind<F, float, KS...>(kind, naive, grad, pl, stream, a);
}
template <int... KS>
hipError_t nan_tail_launch_any(int family, int dtype, int kind, bool naive, bool grad, int grid, size_t lds,
                               hipStream_t stream, const void *args)
{
    const ExactPlan pl{grid, lds};
    switch (family) {
    case LongFamily<true>::id: return nan_tail_launch_family<PairNanTailFamily, KS...>(dtype, kind, naive, grad, pl, stream, args);
    case Long2Family::id: return nan_tail_launch_family<Long2NanTailFamily, KS...>(dtype, kind, naive, grad, pl, stream, args);
    }
    return hipErrorInvalidValue;
}
// the families of launches with SIGSVGD_FLAG_LOG_K: their base's arguments, ids and texts, the LogIO
// kernels (forward-only and gradient, default stencil); the Gram mode of gram_long_kernel has none
struct PairLogFamily : LongFamily<true> {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long_kernel<LogIO<IO>, false, GRAD, KIND, true>; }
};
struct Long2LogFamily : Long2Family {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long2_kernel<LogIO<IO>, false, GRAD, KIND>; }
};
// the launch of family `family` (the paired or the two-sided one) with the LogIO kernel of `kind`, for the two units that build
// them: the unit names its kinds, K0 .. (a kind of another unit: hipErrorInvalidValue)
template <typename F, typename IO, int K0, int... KS>
hipError_t log_k_launch_kind(int kind, bool grad, const ExactPlan &pl, hipStream_t stream, const typename F::Args &a)
{
    if (kind == K0)
        return grad ? ring_launch_one<F, IO, false, true, K0>(pl, stream, a) : ring_launch_one<F, IO, false, false, K0>(pl, stream, a);
    if constexpr (sizeof...(KS) > 0)
        return log_k_launch_kind<F, IO, KS...>(kind, grad, pl, stream, a);
    else
        return hipErrorInvalidValue;
}
template <typename F, int... KS>
hipError_t log_k_launch_family(int dtype, int kind, bool grad, const ExactPlan &pl, hipStream_t stream, const void *args)
{
    const typename F::Args &a = *static_cast<const typename F::Args *>(args);
    return dtype == SIGSVGD_F64 ? log_k_launch_kind<F, double, KS...>(kind, grad, pl, stream, a)
                                : log_k_launch_kind<F, float, KS...>(kind, grad, pl, stream, a);
}
template <int... KS>
hipError_t log_k_launch_any(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                            const void *args)
{
    const ExactPlan pl{grid, lds};
    switch (family) {
    case LongFamily<true>::id: return log_k_launch_family<PairLogFamily, KS...>(dtype, kind, grad, pl, stream, args);
    case Long2Family::id: return log_k_launch_family<Long2LogFamily, KS...>(dtype, kind, grad, pl, stream, args);
    }
    return hipErrorInvalidValue;
}
// the families of launches with SIGSVGD_FLAG_NORMALIZED: the NormIO kernels (forward-only and gradient,
// default stencil), the paired one for the diagonal pass and the two-sided one for the launch itself; launched as the LogIO ones
struct PairNormFamily : LongFamily<true> {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long_kernel<NormIO<IO>, false, GRAD, KIND, true>; }
};
struct Long2NormFamily : Long2Family {
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &gram_long2_kernel<NormIO<IO>, false, GRAD, KIND>; }
};
template <int... KS>
hipError_t norm_launch_any(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                           const void *args)
{
    const ExactPlan pl{grid, lds};
    switch (family) {
    case LongFamily<true>::id: return log_k_launch_family<PairNormFamily, KS...>(dtype, kind, grad, pl, stream, args);
    case Long2Family::id: return log_k_launch_family<Long2NormFamily, KS...>(dtype, kind, grad, pl, stream, args);
    }
    return hipErrorInvalidValue;
}
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

// gram_long_matern.hip: the launch of the Matern kinds' instantiation of family `family` (F::id) at the
// plan's grid and LDS bytes, default stencil only; args: the family's F::Args.  gram_long.hip's family_launch calls it.
hipError_t long_matern_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                              const void *args);
// gram_long_exact.hip: the launch of family `family`'s exact-adjoint instantiation for `kind` (default
// stencil, gradient launches; the Matern kinds from gram_long_exact_matern.hip).  gram_long.hip's family_launch calls it.
hipError_t long_exact_launch(int family, int dtype, int kind, int grid, size_t lds, hipStream_t stream, const void *args);
hipError_t long_exact_matern_launch(int family, int dtype, int kind, int grid, size_t lds, hipStream_t stream,
                                    const void *args);
// gram_long_nantail.hip: the launch of the paired or the two-sided family's NanTailIO instantiation for
// `kind` (the Matern kinds from gram_long_nantail_matern.hip), and the length pass that goes before it: lens[0 .. nX) = the
// lengths of X's paths, lens[nX .. nX + nY) those of Y's (Y == NULL: none), each the index of the path's first point whose
// channel 0 is NaN (T where there is none; at least 1).  gram_long.hip calls both.
hipError_t long_nan_tail_launch(int family, int dtype, int kind, bool naive, bool grad, int grid, size_t lds,
                                hipStream_t stream, const void *args);
hipError_t long_nan_tail_matern_launch(int family, int dtype, int kind, bool naive, bool grad, int grid, size_t lds,
                                       hipStream_t stream, const void *args);
hipError_t long_nan_tail_lengths(int dtype, const void *X, int nX, int TX, const void *Y, int nY, int TY, int d, int *lens,
                                 hipStream_t stream);
// gram_long_logk.hip: the launch of the paired or the two-sided family's LogIO instantiation for `kind`
// (the Matern kinds from gram_long_logk_matern.hip), default stencil.  gram_long.hip's family_launch calls it.
hipError_t long_log_k_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                             const void *args);
hipError_t long_log_k_matern_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                                    const void *args);
// gram_long_norm.hip: the launch of the paired or the two-sided family's NormIO instantiation for `kind`
// (the Matern kinds from gram_long_norm_matern.hip), default stencil, and the two small kernels behind a normalised launch:
// long_norm_sums: rowsum[i] = sum_j U_ij (where given) and colsum[j] = sum_i U_ij (where given) of the weights U [A][B] the
// two-sided kernel stored (norm_weights); long_norm_reduce: out[k][e] = the sum of row k's slabs as long2_reduce_kernel
// adds them, minus sums[k] / 2 times diag[k][e], rounded once.  gram_long.hip calls them.
hipError_t long_norm_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                            const void *args);
hipError_t long_norm_matern_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                                   const void *args);
hipError_t long_norm_sums(const double *U, int A, int B, double *rowsum, double *colsum, hipStream_t stream);
hipError_t long_norm_reduce(int dtype, const double *partials, void *out, int rows, int nslabs, int TD, int skip,
                            const double *sums, const double *diag, hipStream_t stream);

} // namespace sigsvgd
