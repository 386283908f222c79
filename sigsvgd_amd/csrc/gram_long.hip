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
// and long_reduce_kernel adds the slabs of a row i in chunk order.  No floating-point atomics: the bits depend on the inputs.
//
// Paired mode (PAIRED): work item i is the one pair (X_i, Y_i), K_out[i] = k_sig(X_i, Y_i) from the
// same fill and sweeps.  From the pair's one S the gradient pass writes gX_i straight into the caller's buffer, and the same
// pass with lanes owning points n of Y_i and walking m chains S through dk/dy into gY_i[n] = w_i sum_m dG[m][n] dk(x_m, y_n)/dy_n
// (dk/dy = 2 inv_h (x - y) k for RBF, x for linear).  Either output may be skipped; no slabs and no reduce kernel.
//
// Two-sided Gram mode (gram_long2_kernel): a work item is a tile of IC rows x JC columns whose pairs
// are walked row by row.  After a pair's one reverse sweep the row-side pass adds w_row dk/dx into the tile's fp64 slab of
// row i and the column-side pass adds w_col dk/dy into its slab of column j; long2_reduce_kernel adds a row's (a column's)
// slabs in tile order.  With Y = X (yx) the items are the tiles of the upper triangle, only pairs i <= j are solved, K is
// mirrored, and the column side of pair (i, j) is row j's first-slot gradient of the pair (j, i): both sides meet in gX.
#include <type_traits>

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

namespace {
// the static kernel of x (LDS, fp64) and y (global, the caller's dtype)
template <int KIND, typename IO>
__device__ __forceinline__ double static_k(const double *x, const IO *y, int d, double inv_h)
{
    double s = 0.0;
    if (KIND == SIGSVGD_STATIC_RBF) {
        for (int c = 0; c < d; ++c) {
            const double t = x[c] - (double)y[c];
            s = __builtin_fma(t, t, s);
        }
        return exp64(-s * inv_h);
    }
    for (int c = 0; c < d; ++c) s = __builtin_fma(x[c], (double)y[c], s);
    return s;
}
// the same with y's first min(d, 16) coordinates in registers (d <= 16; the branches on d are wave-uniform)
template <int KIND>
__device__ __forceinline__ double static_k16(const double *x, const double (&y)[16], int d, double inv_h)
{
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < d) {
            if (KIND == SIGSVGD_STATIC_RBF) {
                const double t = x[c] - y[c];
                s = __builtin_fma(t, t, s);
            } else {
                s = __builtin_fma(x[c], y[c], s);
            }
        }
    }
    return KIND == SIGSVGD_STATIC_RBF ? exp64(-s * inv_h) : s;
}

// The pair's coarse S chained through the static kernel's derivative into the gradient of the points of one of its paths.
// Lanes own points o of that path, 63 per pass (lane l holds o = o0 - 1 + l and, from lane 1 on, its gradient; S at o - 1
// arrives from the lane below), and walk the points t of the other path in order.  dG[m][n] / w = (S[m-1][n-1] + S[m][n]) -
// (S[m-1][n] + S[m][n-1]), S = 0 outside the coarse grid; store(o, c, g) takes coordinate c of own point o's gradient.
// OWN_X: the points are X's, dk/dx = -2 inv_h (x - y) k (RBF) or y (linear); else Y's, dk/dy = 2 inv_h (x - y) k or x.
template <int KIND, bool OWN_X, typename IO, typename Store>
__device__ __forceinline__ void static_grad_pass(const RingWave &rw, const IO *own, int To, const IO *oth, int Tt, int d,
                                                 double inv_h, Store &&store)
{
    const int lane = threadIdx.x;
    for (int o0 = 0; o0 < To; o0 += kWave - 1) {
        const int o = o0 - 1 + lane;
        const bool valid = lane >= 1 && o < To;
        const IO *po = own + (size_t)min(max(o, 0), To - 1) * d;
        for (int c0 = 0; c0 < d; c0 += 16) {
            double accv[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) accv[c] = 0.0;
            double s_prev = 0.0, nb_prev = 0.0; // S at (o, t - 1), (o - 1, t - 1)
            for (int t = 0; t < Tt; ++t) {
                const int oc = min(max(o, 0), To - 2), tc = min(t, Tt - 2); // (read at a clamped block, then dropped)
                const double s = OWN_X ? ring_S(rw, oc, tc) : ring_S(rw, tc, oc);
                const double s_cur = o >= 0 && o < To - 1 && t < Tt - 1 ? s : 0.0;
                const double nb = shfl_up_f64(s_cur); // S at (o - 1, t)
                const double R = (nb_prev + s_cur) - (nb + s_prev); // dG / w
                s_prev = s_cur;
                nb_prev = nb;
                const IO *pt = oth + (size_t)t * d;
                const IO *xm = OWN_X ? po : pt, *yn = OWN_X ? pt : po;
                if (KIND == SIGSVGD_STATIC_RBF) {
                    double dist = 0.0;
                    for (int c = 0; c < d; ++c) {
                        const double u = (double)xm[c] - (double)yn[c];
                        dist = __builtin_fma(u, u, dist);
                    }
                    const double rk = R * exp64(-dist * inv_h);
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (c0 + c < d) accv[c] = __builtin_fma(rk, (double)xm[c0 + c] - (double)yn[c0 + c], accv[c]);
                } else {
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (c0 + c < d) accv[c] = __builtin_fma(R, (double)pt[c0 + c], accv[c]);
                }
            }
            if (valid) {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c0 + c < d)
                        store(o, c0 + c, KIND == SIGSVGD_STATIC_RBF ? ((OWN_X ? -2.0 : 2.0) * inv_h) * accv[c] : accv[c]);
            }
        }
    }
}
} // namespace

template <typename IO, bool NAIVE, bool GRAD, int KIND, bool PAIRED = false>
__global__ __launch_bounds__(64) void gram_long_kernel(std::conditional_t<PAIRED, PairArgs, LongArgs> a)
{
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
template <typename IO, bool NAIVE, bool GRAD, int KIND>
__global__ __launch_bounds__(64) void gram_long2_kernel(Long2Args a)
{
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
                // staging and fill: gram_long_kernel's, statement for statement (K must have its bits)
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
                __syncthreads(); // (the next pair's forward sweep overwrites the scratch and the ring)
            }
        }
    }
}

// gradX[i][e] = sum over the chunks of row i of partials[i][chunk][e], in chunk order (reproducible bits)
template <typename IO>
__global__ void long_reduce_kernel(const double *partials, IO *gradX, int A, int nchunks, int TD)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)A * TD) return;
    const size_t i = idx / TD, e = idx % TD;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += partials[(i * nchunks + c) * TD + e];
    gradX[idx] = (IO)s;
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
    size_t wsk_bytes, partial_bytes;
    size_t total() const { return ring_ws_total(wsk_bytes + partial_bytes); }
};

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
    long long grid = pl.resident < pl.items ? pl.resident : pl.items;
    if (want_grad && pl.per_wave * (size_t)grid > kRingMaxScratch) {
        grid = (long long)(kRingMaxScratch / pl.per_wave);
        if (grid < 1) grid = 1;
    }
    pl.grid = (int)grid;
    pl.wsk_bytes = ((pl.per_wave * (size_t)grid) + 255) & ~(size_t)255;
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
    size_t col_bytes;
    size_t total() const { return ring_ws_total(wsk_bytes + partial_bytes + col_bytes); }
};

int long2_make_plan(int A, int B, int M, int N, int d, int n, bool want_row, bool want_col, bool yx, Long2Plan &pl)
{
    const int want_grad = want_row || want_col;
    const int rc = ring_make_plan(M, N, n, want_grad, d, "gram_long", pl);
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
    long long grid = pl.resident < pl.items ? pl.resident : pl.items;
    if (want_grad && pl.per_wave * (size_t)grid > kRingMaxScratch) {
        grid = (long long)(kRingMaxScratch / pl.per_wave);
        if (grid < 1) grid = 1;
    }
    pl.grid = (int)grid;
    pl.wsk_bytes = ((pl.per_wave * (size_t)grid) + 255) & ~(size_t)255;
    const size_t rowslabs = yx ? (want_grad ? pl.nti + 1 : 0) : (want_row ? pl.nchunks : 0);
    pl.partial_bytes = (size_t)A * rowslabs * M * d * sizeof(double);
    pl.col_bytes = !yx && want_col ? (size_t)B * pl.nti * N * d * sizeof(double) : 0;
    return SIGSVGD_OK;
}

// the arguments of a Gram launch (B columns) or a paired one (B = 1, no sym), from the plan and the caller's workspace
// (checked against `need`, the plan's total; the Gram mode's slabs follow the forward scratch)
int long_args(const char *who, const LongPlan &pl, size_t need, void *ws, size_t ws_bytes, const void *X, const void *Y,
              const void *grad_out, void *K_out, int A, int B, int M, int N, int d, int n, bool sym, double inv_h, LongArgs &a)
{
    unsigned char *base = nullptr;
    const int rc = ring_ws_base(who, ws, ws_bytes, need, base);
    if (rc) return rc;
    a.X = X; a.Y = Y; a.grad_out = grad_out; a.K_out = K_out;
    a.wsk = reinterpret_cast<float *>(base);
    a.partials = pl.partial_bytes ? reinterpret_cast<double *>(base + pl.wsk_bytes) : nullptr;
    a.wsk_per_block = pl.per_wave / sizeof(float);
    a.A = A; a.B = B; a.M = M; a.N = N; a.d = d; a.n = n; a.r = pl.r; a.P = pl.P; a.Q = pl.Q;
    a.nbands = pl.nbands; a.nsteps = pl.nsteps; a.nrow = pl.nrow; a.W = pl.W; a.JC = pl.JC; a.nchunks = pl.nchunks;
    a.sym = sym ? 1 : 0; a.items = pl.items; a.inv_h = inv_h;
    a.inv_r2 = 1.0 / ((double)pl.r * (double)pl.r);
    return SIGSVGD_OK;
}

template <bool PAIRED>
using LongArgsOf = std::conditional_t<PAIRED, PairArgs, LongArgs>;

template <typename IO, bool NAIVE, bool GRAD, int KIND, bool PAIRED>
hipError_t long_launch_one(const LongPlan &pl, hipStream_t stream, const LongArgsOf<PAIRED> &a)
{
    const hipError_t e = raise_lds_limit<&gram_long_kernel<IO, NAIVE, GRAD, KIND, PAIRED>>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((gram_long_kernel<IO, NAIVE, GRAD, KIND, PAIRED>), dim3(pl.grid), dim3(kWave), pl.lds, stream, a);
    return hipSuccess;
}
template <typename IO, int KIND, bool PAIRED>
hipError_t long_dispatch2(bool naive, bool grad, const LongPlan &pl, hipStream_t stream, const LongArgsOf<PAIRED> &a)
{
    if (naive)
        return grad ? long_launch_one<IO, true, true, KIND, PAIRED>(pl, stream, a)
                    : long_launch_one<IO, true, false, KIND, PAIRED>(pl, stream, a);
    return grad ? long_launch_one<IO, false, true, KIND, PAIRED>(pl, stream, a)
                : long_launch_one<IO, false, false, KIND, PAIRED>(pl, stream, a);
}
template <typename IO, bool PAIRED = false>
hipError_t long_dispatch(int kind, bool naive, bool grad, const LongPlan &pl, hipStream_t stream, const LongArgsOf<PAIRED> &a)
{
    return kind == SIGSVGD_STATIC_RBF ? long_dispatch2<IO, SIGSVGD_STATIC_RBF, PAIRED>(naive, grad, pl, stream, a)
                                      : long_dispatch2<IO, SIGSVGD_STATIC_LINEAR, PAIRED>(naive, grad, pl, stream, a);
}

// the two-sided kernel's launch
template <typename IO, bool NAIVE, bool GRAD, int KIND>
hipError_t long2_launch_one(const LongPlan &pl, hipStream_t stream, const Long2Args &a)
{
    const hipError_t e = raise_lds_limit<&gram_long2_kernel<IO, NAIVE, GRAD, KIND>>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((gram_long2_kernel<IO, NAIVE, GRAD, KIND>), dim3(pl.grid), dim3(kWave), pl.lds, stream, a);
    return hipSuccess;
}
template <typename IO, int KIND>
hipError_t long2_dispatch2(bool naive, bool grad, const LongPlan &pl, hipStream_t stream, const Long2Args &a)
{
    if (naive)
        return grad ? long2_launch_one<IO, true, true, KIND>(pl, stream, a)
                    : long2_launch_one<IO, true, false, KIND>(pl, stream, a);
    return grad ? long2_launch_one<IO, false, true, KIND>(pl, stream, a)
                : long2_launch_one<IO, false, false, KIND>(pl, stream, a);
}
template <typename IO>
hipError_t long2_dispatch(int kind, bool naive, bool grad, const LongPlan &pl, hipStream_t stream, const Long2Args &a)
{
    return kind == SIGSVGD_STATIC_RBF ? long2_dispatch2<IO, SIGSVGD_STATIC_RBF>(naive, grad, pl, stream, a)
                                      : long2_dispatch2<IO, SIGSVGD_STATIC_LINEAR>(naive, grad, pl, stream, a);
}

template <typename IO>
hipError_t long2_reduce(hipStream_t stream, const double *partials, void *out, int rows, int nslabs, int TD, int skip)
{
    const int bs = 256;
    const unsigned gs = (unsigned)(((size_t)rows * TD + bs - 1) / bs);
    hipLaunchKernelGGL(long2_reduce_kernel<IO>, dim3(gs), dim3(bs), 0, stream, partials, static_cast<IO *>(out), rows, nslabs,
                       TD, skip);
    return hipGetLastError();
}
} // namespace

// bytes of the launch's workspace (0 for forward-only launches: the forward sweep keeps nothing)
int long_workspace(int A, int B, int M, int N, int d, int n, int want_grad, size_t *bytes)
{
    LongPlan pl;
    const int rc = long_make_plan(A, B, M, N, d, n, want_grad, pl);
    if (rc) return rc;
    *bytes = pl.total();
    return SIGSVGD_OK;
}

// the argument checks are the entry points' (capi.hip); gradX_out == NULL: forward only
int long_launch(const void *X, const void *Y, int A, int B, int M, int N, int d, int dtype, double inv_h, int n, int kind,
                bool naive, bool sym, const void *grad_out, void *K_out, void *gradX_out, void *ws, size_t ws_bytes,
                hipStream_t stream)
{
    const int want_grad = gradX_out != nullptr;
    LongPlan pl;
    LongArgs a;
    int rc = long_make_plan(A, B, M, N, d, n, want_grad, pl);
    if (!rc) rc = long_args("gram_long", pl, pl.total(), ws, ws_bytes, X, Y, grad_out, K_out, A, B, M, N, d, n, sym, inv_h, a);
    if (rc) return rc;
    hipError_t e = dtype == SIGSVGD_F64 ? long_dispatch<double>(kind, naive, want_grad != 0, pl, stream, a)
                                        : long_dispatch<float>(kind, naive, want_grad != 0, pl, stream, a);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(gram_long)");
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch gram_long_kernel");
    if (want_grad) {
        const int TD = M * d;
        const size_t tot = (size_t)A * TD;
        const int bs = 256;
        const unsigned gs = (unsigned)((tot + bs - 1) / bs);
        if (dtype == SIGSVGD_F64)
            hipLaunchKernelGGL(long_reduce_kernel<double>, dim3(gs), dim3(bs), 0, stream, a.partials,
                               static_cast<double *>(gradX_out), A, pl.nchunks, TD);
        else
            hipLaunchKernelGGL(long_reduce_kernel<float>, dim3(gs), dim3(bs), 0, stream, a.partials,
                               static_cast<float *>(gradX_out), A, pl.nchunks, TD);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "launch long_reduce_kernel");
    }
    return SIGSVGD_OK;
}

// bytes of a paired launch's workspace (0 for forward-only launches)
int pair_workspace(int A, int M, int N, int d, int n, int want_grad, size_t *bytes)
{
    LongPlan pl;
    const int rc = pair_make_plan(A, M, N, d, n, want_grad, pl);
    if (rc) return rc;
    *bytes = pl.total();
    return SIGSVGD_OK;
}

// the argument checks are the entry points' (capi.hip); gradX_out and gradY_out both NULL: forward only
int pair_launch(const void *X, const void *Y, int A, int M, int N, int d, int dtype, double inv_h, int n, int kind, bool naive,
                const void *grad_out, void *K_out, void *gradX_out, void *gradY_out, void *ws, size_t ws_bytes,
                hipStream_t stream)
{
    const int want_grad = gradX_out != nullptr || gradY_out != nullptr;
    LongPlan pl;
    PairArgs a;
    int rc = pair_make_plan(A, M, N, d, n, want_grad, pl);
    if (!rc) rc = long_args("pair", pl, pl.total(), ws, ws_bytes, X, Y, grad_out, K_out, A, 1, M, N, d, n, false, inv_h, a);
    if (rc) return rc;
    a.gradX = gradX_out; a.gradY = gradY_out;
    const hipError_t e = dtype == SIGSVGD_F64 ? long_dispatch<double, true>(kind, naive, want_grad != 0, pl, stream, a)
                                              : long_dispatch<float, true>(kind, naive, want_grad != 0, pl, stream, a);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(gram_long paired)");
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return hip_fail(le, "launch gram_long_kernel (paired)");
    return SIGSVGD_OK;
}

// bytes of a two-sided launch's workspace (0 for forward-only launches)
int long2_workspace(int A, int B, int M, int N, int d, int n, int want_gradX, int want_gradY, bool yx, size_t *bytes)
{
    Long2Plan pl;
    const int rc = long2_make_plan(A, B, M, N, d, n, want_gradX != 0, want_gradY != 0, yx, pl);
    if (rc) return rc;
    *bytes = pl.total();
    return SIGSVGD_OK;
}

// the argument checks are the entry point's (capi.hip); gradX_out and gradY_out both NULL: forward only.  yx: A == B,
// M == N, no gradY_out; gradX_out then gets both sides of every unordered pair.
int long2_launch(const void *X, const void *Y, int A, int B, int M, int N, int d, int dtype, double inv_h, int n, int kind,
                 bool naive, bool sym, bool yx, const void *grad_out, void *K_out, void *gradX_out, void *gradY_out, void *ws,
                 size_t ws_bytes, hipStream_t stream)
{
    const bool want_row = gradX_out != nullptr, want_col = gradY_out != nullptr || (yx && want_row);
    const bool want_grad = want_row || want_col;
    Long2Plan pl;
    Long2Args a;
    int rc = long2_make_plan(A, B, M, N, d, n, want_row, gradY_out != nullptr, yx, pl);
    if (!rc) rc = long_args("gram_long", pl, pl.total(), ws, ws_bytes, X, Y, grad_out, K_out, A, B, M, N, d, n, sym, inv_h, a);
    if (rc) return rc;
    a.colpart = pl.col_bytes // (behind the forward scratch and the row slabs)
                    ? reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(a.wsk) + pl.wsk_bytes + pl.partial_bytes)
                    : nullptr;
    a.IC = pl.IC; a.nti = pl.nti; a.yx = yx ? 1 : 0; a.want_row = want_row ? 1 : 0; a.want_col = want_col ? 1 : 0;
    hipError_t e = dtype == SIGSVGD_F64 ? long2_dispatch<double>(kind, naive, want_grad, pl, stream, a)
                                        : long2_dispatch<float>(kind, naive, want_grad, pl, stream, a);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(gram_long2)");
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch gram_long2_kernel");
    const bool f64 = dtype == SIGSVGD_F64;
    if (want_row) { // yx: a row's nti + 1 slabs, column side first
        const int nslabs = yx ? pl.nti + 1 : pl.nchunks, skip = yx ? pl.IC : 0;
        e = f64 ? long2_reduce<double>(stream, a.partials, gradX_out, A, nslabs, M * d, skip)
                : long2_reduce<float>(stream, a.partials, gradX_out, A, nslabs, M * d, skip);
        if (e != hipSuccess) return hip_fail(e, "launch long2_reduce_kernel (rows)");
    }
    if (gradY_out) {
        e = f64 ? long2_reduce<double>(stream, a.colpart, gradY_out, B, pl.nti, N * d, 0)
                : long2_reduce<float>(stream, a.colpart, gradY_out, B, pl.nti, N * d, 0);
        if (e != hipSuccess) return hip_fail(e, "launch long2_reduce_kernel (columns)");
    }
    return SIGSVGD_OK;
}

} // namespace sigsvgd
