// Signature-kernel Gram matrix and gradient for the built-in static kernels on long paths.
//
// The fused Gram kernels keep a pair's whole-grid state in LDS and refuse paths past it (the coverage kernel from about
// T = 250 at order 0, and refined grids whose tables outgrow 160 KB).  This kernel takes those launches with the layout of
// sig_pde_kernel (sig_pde.hip): one wavefront per pair in a persistent grid, bands of 64 rows of the refined P x Q grid, one
// row per lane, swept anti-diagonal by anti-diagonal, the band's boundary row in LDS, and an LDS ring of the band's fp64
// increments refilled between blocks of 64 sweep steps.  What differs is where the ring's values come from: the fill
// evaluates the static kernel itself,
//   D[a][b] = k(x_{a+1}, y_{b+1}) - k(x_{a+1}, y_b) - k(x_a, y_{b+1}) + k(x_a, y_b)      (fp64)
// from the band's nrow + 1 points of X_i (staged in LDS) and the columns of Y_j (one static-kernel column per lane, read from
// global memory), so the [A, B, M, N] grid never exists.  Increments, sweeps and the gradient are fp64; the stored forward
// solution and the S partials are fp32, as in sig_pde.
//
// Backward: the reverse sweep is sig_pde's (the reference's GG convention), then the pair's coarse S is chained through the
// static kernel into the gradient of x_i:  gX_i[m] += w_ij sum_n dG[m][n] dk(x_m, y_n)/dx_m, with dG the 4-corner scatter of S
// and dk/dx = -2 inv_h (x - y) k (RBF) or y (linear).  Lanes own points m; k is evaluated again there.  A work item is
// (i, chunk of JC columns j): its pairs add into one [TX][d] fp64 slab in j order (the same lane always owns the same entry),
// and long_reduce_kernel adds the slabs of a row i in chunk order.  No floating-point atomics: the bits depend on the inputs.
//
// Paired mode (PAIRED): work item i is the one pair (X_i, Y_i), K_out[i] = k_sig(X_i, Y_i) from the
// same fill and sweeps.  From the pair's one S the gradient pass writes gX_i straight into the caller's buffer, and a second
// pass, lanes owning points n of Y_i and walking m, chains S through dk/dy into gY_i[n] = w_i sum_m dG[m][n] dk(x_m, y_n)/dy_n
// (dk/dy = 2 inv_h (x - y) k for RBF, x for linear).  Either output may be skipped; no slabs and no reduce kernel.
#include <type_traits>

#include "sig_common.h"

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

namespace {
constexpr int kLongMaxCells = 8192;                 // P and Q
constexpr size_t kLongRingDoubles = 8192;           // 64 KB of increments per wave
constexpr size_t kLongMaxScratch = (size_t)1 << 30; // the per-wave scratch of a launch: the grid is lowered to stay below it

// ring of nrow x W fp64 increments + boundary row [Q + 2] + per-lane dump cells [64] + the band's points of X_i [nrow + 1][d]
size_t long_lds_bytes(int nrow, int W, int Q, int d)
{
    return ((size_t)nrow * W + Q + 2 + kWave + (size_t)(nrow + 1) * d) * sizeof(double);
}

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
} // namespace

template <typename IO, bool NAIVE, bool GRAD, int KIND, bool PAIRED = false>
__global__ __launch_bounds__(64) void gram_long_kernel(std::conditional_t<PAIRED, PairArgs, LongArgs> a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const int M = a.M, N = a.N, n = a.n, P = a.P, Q = a.Q, W = a.W, nrow = a.nrow, nsteps = a.nsteps, d = a.d;
    double *ring = reinterpret_cast<double *>(smem_raw); // [nrow][W]: D[a0 + row][b] at column slot b & (W - 1)
    double *rowbuf = ring + (size_t)nrow * W;            // [Q + 2]
    double *dump = rowbuf + (Q + 2);                     // [64]: where the lanes that have nothing to hand over store
    double *xs = dump + kWave;                           // [nrow + 1][d]: points a0 .. a0 + nrow of X_i (clamped to M - 1)
    const IO *GO = static_cast<const IO *>(a.grad_out);
    float *wsk = GRAD ? a.wsk + (size_t)blockIdx.x * a.wsk_per_block : nullptr;
    float *wss = GRAD ? wsk + (size_t)a.nbands * nsteps * kWave : nullptr; // S partials, same order as the forward solution
    float *spare = GRAD ? wss + (size_t)a.nbands * nsteps * kWave + lane : nullptr;

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

            // ---- forward sweep (sig_pde_kernel's) ---------------------------------------------------------------------
            double Kval = 1.0;
            for (int kb = 0; kb < a.nbands; ++kb) {
                const int p = kb * kWave + lane;
                const bool rowvalid = p < P;
                const bool first = kb == 0;
                const int a0 = (kb * kWave) >> n;
                stage_x(a0);
                const double *Drow = ring + (size_t)((min(p, P - 1) >> n) - a0) * W;
                float *wp = GRAD ? wsk + (size_t)kb * nsteps * kWave + lane : nullptr;
                double cur = 1.0, upprev = 1.0;
                double rb = first ? 1.0 : rowbuf[1]; // lane 0's upper neighbour on step s: rowbuf[s + 1]
                int have = -1;                       // coarse columns 0 .. have are in the ring (the last ones filled)
                for (int s0 = 0; s0 < nsteps; s0 += kWave) {
                    const int lo = max(s0 - (kWave - 1), 0) >> n, hi = min((s0 + kWave - 1) >> n, N - 2);
                    if (hi > have) { // every column this block and as many later ones as the ring holds
                        const int to = min(N - 2, lo + W - 1);
                        fill(a0, have + 1, to);
                        have = to;
                    }
                    double gf = Drow[(min(max(s0 - lane, 0), Q - 1) >> n) & (W - 1)];
                    const int s1 = min(s0 + kWave, nsteps);
                    for (int s = s0; s < s1; ++s) {
                        const int q = s - lane;
                        const bool active = rowvalid && q >= 0 && q < Q;
                        const double gfn = Drow[(min(max(q + 1, 0), Q - 1) >> n) & (W - 1)];
                        const double rbr = rowbuf[min(s + 2, Q)];
                        const double rbn = first ? 1.0 : rbr;
                        double up_in = shfl_up_f64(cur);
                        up_in = (lane == 0) ? rb : up_in;
                        const double nw = stencil(cur, up_in, upprev, gf * a.inv_r2, NAIVE);
                        if (GRAD) { // K_fwd[p][q] at [step][lane] (issued from inline asm: no wait for the previous step's store)
                            const float kst = (float)upprev;
                            asm volatile("global_store_dword %0, %1, off" ::"v"(wp + (size_t)s * kWave), "v"(kst));
                        }
                        *((lane == kWave - 1 && active) ? rowbuf + (q + 1) : dump + lane) = nw;
                        cur = active ? nw : cur;
                        upprev = active ? up_in : upprev;
                        gf = gfn;
                        rb = rbn;
                    }
                }
                if (p == P - 1) Kval = cur;
            }
            if (((P - 1) & (kWave - 1)) == lane) static_cast<IO *>(a.K_out)[PAIRED ? (size_t)i : (size_t)i * a.B + j] = (IO)Kval;
            if (!GRAD) {
                __syncthreads(); // (the next pair's first fill overwrites the ring, its sweep the boundary row)
                continue;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the forward solution is in L2 before it is read back
            __syncthreads();

            // ---- reverse sweep (sig_pde_kernel's): GG = K_fwd[p][q] K_rev[p+1][q+1], summed over the r columns of a block --
            for (int kb = a.nbands - 1; kb >= 0; --kb) {
                const int p = kb * kWave + lane;
                const bool rowvalid = p < P;
                const int L = min(kWave, P - kb * kWave);
                const int a0 = (kb * kWave) >> n;
                stage_x(a0);
                const double *Drow = ring + (size_t)((min(p, P - 1) >> n) - a0) * W;
                float *wsrow = wss + (size_t)kb * nsteps * kWave + lane;
                const float *wrow = wsk + (size_t)kb * nsteps * kWave + lane; // K_fwd[p][q] at step lane + q
                const bool lastband = kb == a.nbands - 1;
                const bool hands_over = lane == 0 && kb > 0;
                double cur = 1.0, dprev = 1.0, sb = 0.0;
                const int nsp = Q + L - 1;
                int q = Q - 1 + (L - 1 - lane);
                int R = Q - 1 + L - 1; // row of the stored forward solution on reverse step 0
                double rb = lastband ? 1.0 : rowbuf[Q - 1]; // lane L-1's lower neighbour on step sp: rowbuf[Q - 1 - sp]
                constexpr int KPF = 8; // ring of the next KPF rows of the forward solution (an L2 round trip is ~8 steps long)
                float kfr[KPF];
#pragma unroll
                for (int u = 0; u < KPF; ++u) kfr[u] = wrow[(size_t)max(R - u, 0) * kWave];
                int low = N - 1; // coarse columns low .. N - 2 are in the ring
                for (int sp0 = 0; sp0 < nsp; sp0 += kWave) {
                    const int qhi = Q + L - 2 - sp0; // the columns of this block: qhi - 126 .. qhi
                    const int need_hi = min(qhi, Q - 1) >> n, need_lo = max(qhi - 2 * (kWave - 1), 0) >> n;
                    if (need_lo < low) {
                        const int from = max(0, need_hi - W + 1);
                        fill(a0, from, low - 1);
                        low = from;
                    }
                    double gf = Drow[(min(max(q, 0), Q - 1) >> n) & (W - 1)];
                    double rbk = rowbuf[max(Q - 1 - sp0, 0)];
                    rb = lastband ? 1.0 : rbk;
                    for (int sp1 = sp0; sp1 < sp0 + kWave; sp1 += KPF) {
#pragma unroll
                        for (int u = 0; u < KPF; ++u, --q, --R) {
                            const int sp = sp1 + u;
                            const bool active = rowvalid && q >= 0 && q < Q;
                            const double gfn = Drow[(min(max(q - 1, 0), Q - 1) >> n) & (W - 1)];
                            const double rbr = rowbuf[max(Q - 2 - sp, 0)];
                            const double rbn = lastband ? 1.0 : rbr;
                            const double kf = (double)kfr[u];
                            kfr[u] = wrow[(size_t)max(R - KPF, 0) * kWave];
                            double down_in = shfl_down_f64(cur);
                            down_in = (lane == L - 1) ? rb : down_in;
                            sb = active ? __builtin_fma(kf, dprev, sb) : sb;
                            const bool done = active && (q & (a.r - 1)) == 0; // the block's last (lowest) column
                            const float sst = done ? (float)(sb * a.inv_r2) : 0.f;
                            asm volatile("global_store_dword %0, %1, off" ::"v"(R >= 0 ? wsrow + (size_t)R * kWave : spare), "v"(sst));
                            sb = done ? 0.0 : sb;
                            const double nw = stencil(cur, down_in, dprev, gf * a.inv_r2, NAIVE);
                            *((hands_over && active) ? rowbuf + q : dump + lane) = nw;
                            cur = active ? nw : cur;
                            dprev = active ? down_in : dprev;
                            gf = gfn;
                            rb = rbn;
                        }
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // S is in L2 before it is read back
            __syncthreads();

            // ---- gradient: S -> dG (4-corner scatter) -> static-kernel derivative -> gX_i -------------------------------
            // S[aa][bb] = the r lane partials of block (aa, bb) in row order (lane pp & 63 of band pp >> 6 filed the partial
            // of row pp, block column bb, on reverse step (pp & 63) + bb r); S = 0 outside the coarse grid.
            const int r = a.r, Mm = M - 1, Nm = N - 1;
            auto Sat = [&](int aa, int bb) -> double {
                const bool in = aa >= 0 && aa < Mm && bb < Nm;
                aa = min(max(aa, 0), Mm - 1);
                bb = min(bb, Nm - 1);
                double s = 0.0;
                for (int t = 0; t < r; ++t) {
                    const int pp = aa * r + t, l = pp & (kWave - 1);
                    s += (double)wss[((size_t)(pp >> 6) * nsteps + l + (size_t)bb * r) * kWave + l];
                }
                return in ? s : 0.0;
            };
            double w = GO ? (double)GO[PAIRED ? (size_t)i : (size_t)i * a.B + j] : 1.0;
            if (!PAIRED && a.sym) w += GO ? (double)GO[(size_t)j * a.B + i] : 1.0;
            // a pass of 63 points: lane l holds row m0 - 1 + l of S and, from lane 1 on, the gradient of point m = m0 - 1 + l
            // (S[m - 1][*] arrives from the lane below it)
            int mx_end = M;
            if constexpr (PAIRED) mx_end = a.gradX ? M : 0; // (paired: gX skipped when its output is NULL)
            for (int m0 = 0; m0 < mx_end; m0 += kWave - 1) {
                const int m = m0 - 1 + lane;
                const bool mvalid = lane >= 1 && m < M;
                const IO *xm = xi + (size_t)min(max(m, 0), M - 1) * d;
                for (int c0 = 0; c0 < d; c0 += 16) {
                    double accv[16];
#pragma unroll
                    for (int c = 0; c < 16; ++c) accv[c] = 0.0;
                    double s_prev = 0.0, su_prev = 0.0; // S[m][n - 1], S[m - 1][n - 1]
                    for (int nn = 0; nn < N; ++nn) {
                        const double s_cur = Sat(m, nn);
                        const double su = shfl_up_f64(s_cur);
                        const double R = (su_prev + s_cur) - (su + s_prev); // dG[m][nn] / w
                        s_prev = s_cur;
                        su_prev = su;
                        const IO *yn = yj + (size_t)nn * d;
                        if (KIND == SIGSVGD_STATIC_RBF) {
                            double dist = 0.0;
                            for (int c = 0; c < d; ++c) {
                                const double t = (double)xm[c] - (double)yn[c];
                                dist = __builtin_fma(t, t, dist);
                            }
                            const double rk = R * exp64(-dist * a.inv_h);
#pragma unroll
                            for (int c = 0; c < 16; ++c)
                                if (c0 + c < d) accv[c] = __builtin_fma(rk, (double)xm[c0 + c] - (double)yn[c0 + c], accv[c]);
                        } else {
#pragma unroll
                            for (int c = 0; c < 16; ++c)
                                if (c0 + c < d) accv[c] = __builtin_fma(R, (double)yn[c0 + c], accv[c]);
                        }
                    }
                    if (mvalid) {
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            if (c0 + c < d) {
                                const double val = KIND == SIGSVGD_STATIC_RBF ? (-2.0 * a.inv_h) * accv[c] : accv[c];
                                if constexpr (PAIRED) {
                                    static_cast<IO *>(a.gradX)[((size_t)i * M + m) * d + c0 + c] = (IO)(w * val);
                                } else {
                                    double *o = slab + (size_t)m * d + c0 + c;
                                    *o = j == j0 ? w * val : __builtin_fma(w, val, *o);
                                }
                            }
                        }
                    }
                }
            }
            if constexpr (PAIRED) {
                // ---- paired: S -> dG -> dk/dy -> gY_i, the X pass with the roles of the two paths swapped -------------------
                // lane l holds column n0 - 1 + l of S and, from lane 1 on, the gradient of point n = n0 - 1 + l of Y_i
                // (S[*][n - 1] arrives from the lane below it); m walks the points of X_i in order (x_m is wave-uniform)
                auto SatY = [&](int aa, int bb) -> double {
                    const bool in = aa < Mm && bb >= 0 && bb < Nm;
                    aa = min(aa, Mm - 1);
                    bb = min(max(bb, 0), Nm - 1);
                    double s = 0.0;
                    for (int t = 0; t < r; ++t) {
                        const int pp = aa * r + t, l = pp & (kWave - 1);
                        s += (double)wss[((size_t)(pp >> 6) * nsteps + l + (size_t)bb * r) * kWave + l];
                    }
                    return in ? s : 0.0;
                };
                const int ny_end = a.gradY ? N : 0;
                for (int n0 = 0; n0 < ny_end; n0 += kWave - 1) {
                    const int nn = n0 - 1 + lane;
                    const bool nvalid = lane >= 1 && nn < N;
                    const IO *yn = yj + (size_t)min(max(nn, 0), N - 1) * d;
                    for (int c0 = 0; c0 < d; c0 += 16) {
                        double accv[16];
#pragma unroll
                        for (int c = 0; c < 16; ++c) accv[c] = 0.0;
                        double s_prev = 0.0, sl_prev = 0.0; // S[m - 1][n], S[m - 1][n - 1]
                        for (int mm = 0; mm < M; ++mm) {
                            const double s_cur = SatY(mm, nn);
                            const double sl = shfl_up_f64(s_cur); // S[m][n - 1]
                            const double R = (sl_prev + s_cur) - (sl + s_prev); // dG[m][n] / w
                            s_prev = s_cur;
                            sl_prev = sl;
                            const IO *xm = xi + (size_t)mm * d;
                            if (KIND == SIGSVGD_STATIC_RBF) {
                                double dist = 0.0;
                                for (int c = 0; c < d; ++c) {
                                    const double t = (double)xm[c] - (double)yn[c];
                                    dist = __builtin_fma(t, t, dist);
                                }
                                const double rk = R * exp64(-dist * a.inv_h);
#pragma unroll
                                for (int c = 0; c < 16; ++c)
                                    if (c0 + c < d) accv[c] = __builtin_fma(rk, (double)xm[c0 + c] - (double)yn[c0 + c], accv[c]);
                            } else {
#pragma unroll
                                for (int c = 0; c < 16; ++c)
                                    if (c0 + c < d) accv[c] = __builtin_fma(R, (double)xm[c0 + c], accv[c]);
                            }
                        }
                        if (nvalid) {
#pragma unroll
                            for (int c = 0; c < 16; ++c) {
                                if (c0 + c < d) {
                                    const double val = KIND == SIGSVGD_STATIC_RBF ? (2.0 * a.inv_h) * accv[c] : accv[c];
                                    static_cast<IO *>(a.gradY)[((size_t)i * N + nn) * d + c0 + c] = (IO)(w * val);
                                }
                            }
                        }
                    }
                }
            }
            __syncthreads(); // (the next pair's forward sweep overwrites the scratch and the ring)
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

namespace {
struct LongPlan {
    int r, P, Q, nbands, nsteps, nrow, W, JC, nchunks, grid;
    long long items;
    size_t lds, wsk_per_block, wsk_bytes, partial_bytes;
    size_t total() const { return wsk_bytes + partial_bytes ? wsk_bytes + partial_bytes + 256 : 0; }
};

int long_make_plan(int A, int B, int M, int N, int d, int n, int want_grad, LongPlan &pl, const char *who = "gram_long")
{
    pl.r = 1 << n;
    const long long P = (long long)pl.r * (M - 1), Q = (long long)pl.r * (N - 1);
    pl.nbands = (int)((P + kWave - 1) / kWave);
    pl.nsteps = (int)(Q + kWave - 1);
    const size_t per_wave = want_grad ? ((size_t)2 * pl.nbands * pl.nsteps * kWave + kWave) * sizeof(float) : 0;
    if (P > kLongMaxCells || Q > kLongMaxCells) {
        set_error("%s: refined grid %lld x %lld exceeds %d x %d (one wave's scratch would be %zu B)", who, P, Q,
                  kLongMaxCells, kLongMaxCells, per_wave);
        return SIGSVGD_E_UNSUPPORTED;
    }
    pl.P = (int)P;
    pl.Q = (int)Q;
    pl.nrow = n <= 6 ? (kWave >> n) : 1; // coarse rows of a band of 64 rows
    int W = 1;
    while (W < N - 1) W <<= 1;
    int Wcap = 1;
    while ((size_t)Wcap * 2 * pl.nrow <= kLongRingDoubles) Wcap <<= 1;
    pl.W = W < Wcap ? W : Wcap; // >= the (126 >> n) + 2 columns a block of 64 steps can touch
    pl.lds = long_lds_bytes(pl.nrow, pl.W, pl.Q, d);
    if (pl.lds > 160 * 1024) {
        set_error("%s: per-wave state needs %zu B of LDS (> 160 KiB): d=%d", who, pl.lds, d);
        return SIGSVGD_E_UNSUPPORTED;
    }
    const long long cus = device_cu_count();
    const int per_cu = (int)((160 * 1024) / pl.lds);
    const long long resident = cus * (per_cu > 8 ? 8 : per_cu);
    // work items (i, chunk of JC columns): enough to give every resident wave one, few enough gradient slabs
    int JC = 32;
    while (JC > 1 && (long long)A * ((B + JC - 1) / JC) < resident) JC >>= 1;
    pl.JC = JC;
    pl.nchunks = (B + JC - 1) / JC;
    pl.items = (long long)A * pl.nchunks;
    long long grid = resident < pl.items ? resident : pl.items;
    if (want_grad && per_wave * (size_t)grid > kLongMaxScratch) {
        grid = (long long)(kLongMaxScratch / per_wave);
        if (grid < 1) grid = 1;
    }
    pl.grid = (int)grid;
    pl.wsk_per_block = per_wave / sizeof(float);
    pl.wsk_bytes = ((per_wave * (size_t)grid) + 255) & ~(size_t)255;
    pl.partial_bytes = want_grad ? (size_t)A * pl.nchunks * M * d * sizeof(double) : 0;
    return SIGSVGD_OK;
}

// the paired plan: the Gram plan of one column (items = A pairs, one per wavefront, grid = min(resident waves, A), the same
// LDS, cell limits and 1 GiB scratch cap); the gradients are written straight to the outputs, so there are no slabs
int pair_make_plan(int A, int M, int N, int d, int n, int want_grad, LongPlan &pl)
{
    const int rc = long_make_plan(A, 1, M, N, d, n, want_grad, pl, "pair");
    if (rc) return rc;
    pl.partial_bytes = 0;
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
    const int rc = long_make_plan(A, B, M, N, d, n, want_grad, pl);
    if (rc) return rc;
    const size_t need = pl.total();
    if (ws_bytes < need || (need && !ws)) {
        set_error("gram_long: workspace %zu B too small, required %zu B", ws_bytes, need);
        return SIGSVGD_E_WORKSPACE;
    }
    unsigned char *base = need ? reinterpret_cast<unsigned char *>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255)
                               : nullptr;
    LongArgs a;
    a.X = X; a.Y = Y; a.grad_out = grad_out; a.K_out = K_out;
    a.wsk = want_grad ? reinterpret_cast<float *>(base) : nullptr;
    a.partials = want_grad ? reinterpret_cast<double *>(base + pl.wsk_bytes) : nullptr;
    a.wsk_per_block = pl.wsk_per_block;
    a.A = A; a.B = B; a.M = M; a.N = N; a.d = d; a.n = n; a.r = pl.r; a.P = pl.P; a.Q = pl.Q;
    a.nbands = pl.nbands; a.nsteps = pl.nsteps; a.nrow = pl.nrow; a.W = pl.W; a.JC = pl.JC; a.nchunks = pl.nchunks;
    a.sym = sym ? 1 : 0; a.items = pl.items; a.inv_h = inv_h;
    a.inv_r2 = 1.0 / ((double)pl.r * (double)pl.r);
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
    const int rc = pair_make_plan(A, M, N, d, n, want_grad, pl);
    if (rc) return rc;
    const size_t need = pl.total();
    if (ws_bytes < need || (need && !ws)) {
        set_error("pair: workspace %zu B too small, required %zu B", ws_bytes, need);
        return SIGSVGD_E_WORKSPACE;
    }
    unsigned char *base = need ? reinterpret_cast<unsigned char *>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255)
                               : nullptr;
    PairArgs a;
    a.X = X; a.Y = Y; a.grad_out = grad_out; a.K_out = K_out;
    a.wsk = want_grad ? reinterpret_cast<float *>(base) : nullptr;
    a.partials = nullptr;
    a.wsk_per_block = pl.wsk_per_block;
    a.A = A; a.B = 1; a.M = M; a.N = N; a.d = d; a.n = n; a.r = pl.r; a.P = pl.P; a.Q = pl.Q;
    a.nbands = pl.nbands; a.nsteps = pl.nsteps; a.nrow = pl.nrow; a.W = pl.W; a.JC = 1; a.nchunks = 1;
    a.sym = 0; a.items = pl.items; a.inv_h = inv_h;
    a.inv_r2 = 1.0 / ((double)pl.r * (double)pl.r);
    a.gradX = gradX_out; a.gradY = gradY_out;
    const hipError_t e = dtype == SIGSVGD_F64 ? long_dispatch<double, true>(kind, naive, want_grad != 0, pl, stream, a)
                                              : long_dispatch<float, true>(kind, naive, want_grad != 0, pl, stream, a);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(gram_long paired)");
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return hip_fail(le, "launch gram_long_kernel (paired)");
    return SIGSVGD_OK;
}

} // namespace sigsvgd
