// Signature PDE on a caller-supplied static-kernel grid (user static kernels).
//
// Input: npairs grids G[pair][M][N] (the static kernel k(x_a, y_b) of one pair of paths, evaluated by the caller), fp32 or
// fp64.  Forward: the 4-corner increments D[a][b] = (G[a+1][b+1] - G[a+1][b]) - (G[a][b+1] - G[a][b]) in fp64, refined to
// g[p][q] = D[p >> n][q >> n] / r^2 on the P x Q grid (r = 2^n, P = r (M-1), Q = r (N-1)), one Goursat sweep in fp64, and
// K[pair] = sol[P][Q].  Backward: the reference's convention (oracle/sigkernel_oracle.py gram_backward): GG[p][q] =
// K_fwd[p][q] K_rev[p+1][q+1], S[a][b] = r^-2 sum of GG over the block of (a, b), and dG[m][n] = grad_out (S[m-1][n-1] +
// S[m][n] - S[m-1][n] - S[m][n-1]) with S = 0 outside the grid.
//
// Layout (the long-path mode of gram_generic_kernel): one wavefront per pair in a persistent grid; the grid is swept in bands
// of 64 rows, one row per lane, anti-diagonal by anti-diagonal (lane l is at column s - l on step s); the band's boundary row
// is in LDS.  The band's fp64 increments live in an LDS ring of W coarse columns of the band's coarse rows; it is refilled
// from G in global memory between blocks of 64 sweep steps (never inside a step), with every column the next block can
// touch, so W = 128 columns at dyadic order 0 hold grids of any width.  For the backward pass the forward solution goes to
// the wave's scratch in [band][step][lane] order (fp32, coalesced 256-B rows); the reverse sweep writes each lane's partial
// block sum of GG (over the r columns of a block) in the same order, and the assembly adds the r rows of a block in row order:
// no floating-point atomics, the bits depend on the inputs only.
#include "sig_common.h"

namespace sigsvgd {

struct PdeArgs {
    const void *G, *grad_out;
    void *K_out, *dG_out;
    float *wsk;           // [grid][wsk_per_block]: forward solution, then S partials (+ one spare row)
    size_t wsk_per_block; // floats
    int npairs, M, N, n, r, P, Q, nbands, nsteps, nrow, W;
    double inv_r2;
};

namespace {
constexpr int kPdeMaxCells = 8192;            // P and Q
constexpr size_t kPdeRingDoubles = 8192;      // 64 KB of increments per wave
constexpr size_t kPdeMaxScratch = (size_t)1 << 30; // the launch's scratch: the residency is lowered to stay below this

// ring of nrow x W fp64 increments + boundary row [Q + 2] + per-lane dump cells [64]
size_t pde_lds_bytes(int nrow, int W, int Q) { return ((size_t)nrow * W + Q + 2 + kWave) * sizeof(double); }
} // namespace

template <typename IO, bool NAIVE, bool GRAD>
__global__ __launch_bounds__(64) void sig_pde_kernel(PdeArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const int M = a.M, N = a.N, n = a.n, P = a.P, Q = a.Q, W = a.W, nrow = a.nrow, nsteps = a.nsteps;
    double *ring = reinterpret_cast<double *>(smem_raw); // [nrow][W]: D[a0 + row][b] at column slot b & (W - 1)
    double *rowbuf = ring + (size_t)nrow * W;            // [Q + 2]
    double *dump = rowbuf + (Q + 2);                     // [64]: where the lanes that have nothing to hand over store
    const IO *GO = static_cast<const IO *>(a.grad_out);
    float *wsk = GRAD ? a.wsk + (size_t)blockIdx.x * a.wsk_per_block : nullptr;
    float *wss = GRAD ? wsk + (size_t)a.nbands * nsteps * kWave : nullptr; // S partials, same order as the forward solution
    float *spare = GRAD ? wss + (size_t)a.nbands * nsteps * kWave + lane : nullptr;

    for (int pair = blockIdx.x; pair < a.npairs; pair += gridDim.x) {
        const IO *G = static_cast<const IO *>(a.G) + (size_t)pair * M * N;
        // coarse columns b_lo .. b_hi of the increment rows a0 .. a0 + nrow - 1 into the ring: lane = column, down the G rows
        // (every load unconditional at a clamped address, so the compiler can issue them back to back)
        auto fill = [&](int a0, int b_lo, int b_hi) {
            __syncthreads(); // (the sweep's reads of the slots this overwrites are done)
            for (int b0 = b_lo; b0 <= b_hi; b0 += kWave) {
                const int b = b0 + lane;
                const bool ok = b <= b_hi;
                const IO *gc = G + min(b, N - 2);
                double rd_prev = 0.0;
#pragma unroll 4
                for (int k = 0; k <= nrow; ++k) {
                    const int ga = min(a0 + k, M - 1);
                    const double rd = (double)gc[(size_t)ga * N + 1] - (double)gc[(size_t)ga * N];
                    if (k >= 1 && ok) ring[(k - 1) * W + (b & (W - 1))] = (a0 + k < M) ? rd - rd_prev : 0.0;
                    rd_prev = rd;
                }
            }
            __syncthreads();
        };

        // ---- forward sweep ------------------------------------------------------------------------------------------
        // (the step of gram_generic_kernel: branch-free, results of lanes outside the grid dropped by selects, the operands of
        //  step s + 1 fetched during step s)
        double Kval = 1.0;
        for (int kb = 0; kb < a.nbands; ++kb) {
            const int p = kb * kWave + lane;
            const bool rowvalid = p < P;
            const bool first = kb == 0;
            const int a0 = (kb * kWave) >> n;
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
        if (((P - 1) & (kWave - 1)) == lane) static_cast<IO *>(a.K_out)[pair] = (IO)Kval;
        if (!GRAD) continue;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the forward solution is in L2 before it is read back
        __syncthreads();

        // ---- reverse sweep: GG = K_fwd[p][q] K_rev[p+1][q+1], summed over the r columns of a block per lane ---------------
        for (int kb = a.nbands - 1; kb >= 0; --kb) {
            const int p = kb * kWave + lane;
            const bool rowvalid = p < P;
            const int L = min(kWave, P - kb * kWave);
            const int a0 = (kb * kWave) >> n;
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
                // (the groups past nsp have no lane inside the grid and change nothing; their S stores go to the spare row)
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
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // S is in L2 before the assembly reads it
        __syncthreads();

        // ---- assembly: S[a][b] = the r lane partials of block (a, b) in row order; dG = grad_out * 4-corner scatter of S ----
        // (lane p & 63 of band p >> 6 filed the partial of row p, block column b, on reverse step R = (p & 63) + b r)
        const int r = a.r, Mm = M - 1, Nm = N - 1;
        auto Sat = [&](int aa, int bb) -> double {
            double s = 0.0;
            for (int i = 0; i < r; ++i) {
                const int pp = aa * r + i, l = pp & (kWave - 1);
                s += (double)wss[((size_t)(pp >> 6) * nsteps + l + (size_t)bb * r) * kWave + l];
            }
            return s;
        };
        const double w = GO ? (double)GO[pair] : 1.0;
        IO *dG = static_cast<IO *>(a.dG_out) + (size_t)pair * M * N;
        for (int e = lane; e < M * N; e += kWave) {
            const int m = e / N, nn = e - m * N;
            double Rv = 0.0;
            if (m >= 1 && nn >= 1) Rv += Sat(m - 1, nn - 1);
            if (m < Mm && nn < Nm) Rv += Sat(m, nn);
            if (m >= 1 && nn < Nm) Rv -= Sat(m - 1, nn);
            if (m < Mm && nn >= 1) Rv -= Sat(m, nn - 1);
            dG[e] = (IO)(w * Rv);
        }
        __syncthreads(); // (the next pair's forward sweep overwrites the scratch and the ring)
    }
}

namespace {
struct PdePlan {
    int r, P, Q, nbands, nsteps, nrow, W, grid;
    size_t lds, wsk_per_block, ws_bytes;
};

int pde_make_plan(int npairs, int M, int N, int n, int want_grad, PdePlan &pl)
{
    pl.r = 1 << n;
    const long long P = (long long)pl.r * (M - 1), Q = (long long)pl.r * (N - 1);
    pl.nbands = (int)((P + kWave - 1) / kWave);
    pl.nsteps = (int)(Q + kWave - 1);
    const size_t per_wave = want_grad ? ((size_t)2 * pl.nbands * pl.nsteps * kWave + kWave) * sizeof(float) : 0;
    if (P > kPdeMaxCells || Q > kPdeMaxCells) {
        set_error("pde: refined grid %lld x %lld exceeds %d x %d (one wave's scratch would be %zu B)", P, Q, kPdeMaxCells,
                  kPdeMaxCells, per_wave);
        return SIGSVGD_E_UNSUPPORTED;
    }
    pl.P = (int)P;
    pl.Q = (int)Q;
    pl.nrow = n <= 6 ? (kWave >> n) : 1; // coarse rows of a band of 64 rows
    int W = 1;
    while (W < N - 1) W <<= 1;
    int Wcap = 1;
    while ((size_t)Wcap * 2 * pl.nrow <= kPdeRingDoubles) Wcap <<= 1;
    pl.W = W < Wcap ? W : Wcap; // >= the (126 >> n) + 2 columns a block of 64 steps can touch
    pl.lds = pde_lds_bytes(pl.nrow, pl.W, pl.Q);
    if (pl.lds > 160 * 1024) {
        set_error("pde: per-wave state needs %zu B of LDS (> 160 KiB)", pl.lds);
        return SIGSVGD_E_UNSUPPORTED;
    }
    // the scratch covers 8 waves per CU whatever the LDS allows (so it never shrinks as the grid grows), fewer where one wave's
    // scratch is large; the launch runs the waves the LDS lets the CUs hold, at most that many
    // (beyond kPdeMaxScratch the size is that cap -- or one wave's scratch -- so it does not shrink either)
    const long long cus = device_cu_count();
    long long slots = cus * 8 < npairs ? cus * 8 : npairs;
    pl.ws_bytes = per_wave * (size_t)slots;
    if (pl.ws_bytes > kPdeMaxScratch) {
        slots = (long long)(kPdeMaxScratch / per_wave);
        if (slots < 1) slots = 1;
        pl.ws_bytes = per_wave > kPdeMaxScratch ? per_wave : kPdeMaxScratch;
    }
    const int per_cu = (int)((160 * 1024) / pl.lds);
    const long long resident = cus * (per_cu > 8 ? 8 : per_cu);
    pl.grid = (int)(resident < slots ? resident : slots);
    pl.wsk_per_block = per_wave / sizeof(float);
    return SIGSVGD_OK;
}

template <typename IO, bool NAIVE, bool GRAD>
hipError_t pde_launch_one(const PdePlan &pl, hipStream_t stream, const PdeArgs &a)
{
    const hipError_t e = raise_lds_limit<&sig_pde_kernel<IO, NAIVE, GRAD>>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((sig_pde_kernel<IO, NAIVE, GRAD>), dim3(pl.grid), dim3(kWave), pl.lds, stream, a);
    return hipSuccess;
}
template <typename IO>
hipError_t pde_dispatch(bool naive, bool grad, const PdePlan &pl, hipStream_t stream, const PdeArgs &a)
{
    if (naive) return grad ? pde_launch_one<IO, true, true>(pl, stream, a) : pde_launch_one<IO, true, false>(pl, stream, a);
    return grad ? pde_launch_one<IO, false, true>(pl, stream, a) : pde_launch_one<IO, false, false>(pl, stream, a);
}
} // namespace

// bytes of the launch's scratch (0 for forward-only launches: the forward sweep keeps nothing)
int pde_workspace(int npairs, int M, int N, int n, int want_grad, size_t *bytes)
{
    PdePlan pl;
    const int rc = pde_make_plan(npairs, M, N, n, want_grad, pl);
    if (rc) return rc;
    *bytes = pl.ws_bytes ? pl.ws_bytes + 256 : 0; // (+ the slack of aligning the caller's pointer)
    return SIGSVGD_OK;
}

// the argument checks are the entry points' (capi.hip); dG_out == NULL: forward only
int pde_launch(const void *G, int npairs, int M, int N, int dtype, int n, bool naive, const void *grad_out, void *K_out,
               void *dG_out, void *ws, size_t ws_bytes, hipStream_t stream)
{
    const int want_grad = dG_out != nullptr;
    PdePlan pl;
    int rc = pde_make_plan(npairs, M, N, n, want_grad, pl);
    if (rc) return rc;
    const size_t need = pl.ws_bytes ? pl.ws_bytes + 256 : 0;
    if (ws_bytes < need || (need && !ws)) {
        set_error("pde: workspace %zu B too small, required %zu B", ws_bytes, need);
        return SIGSVGD_E_WORKSPACE;
    }
    PdeArgs a;
    a.G = G; a.grad_out = grad_out; a.K_out = K_out; a.dG_out = dG_out;
    a.wsk = need ? reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255) : nullptr;
    a.wsk_per_block = pl.wsk_per_block;
    a.npairs = npairs; a.M = M; a.N = N; a.n = n; a.r = pl.r; a.P = pl.P; a.Q = pl.Q;
    a.nbands = pl.nbands; a.nsteps = pl.nsteps; a.nrow = pl.nrow; a.W = pl.W;
    a.inv_r2 = 1.0 / ((double)pl.r * (double)pl.r);
    hipError_t e = dtype == SIGSVGD_F64 ? pde_dispatch<double>(naive, want_grad != 0, pl, stream, a)
                                        : pde_dispatch<float>(naive, want_grad != 0, pl, stream, a);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(sig_pde)");
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch sig_pde_kernel");
    return SIGSVGD_OK;
}

} // namespace sigsvgd
