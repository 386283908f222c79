// The long-path PDE sweep shared by sig_pde_kernel (sig_pde.hip) and the kernels of gram_long.hip, DESIGN.md sections
// 5.9 - 5.13: the ring plan's geometry, the launch of a kernel family on it, the forward and reverse sweeps of one pair, and
// the reader of the pair's coarse S.
//
// One wavefront per pair; the refined P x Q grid is swept in bands of 64 rows, one row per lane, anti-diagonal by
// anti-diagonal (lane l is at column s - l on step s); the band's boundary row is in LDS.  The band's fp64 increments live in
// an LDS ring of W coarse columns of the band's nrow coarse rows; the caller's fill refills it between blocks of 64 sweep
// steps (never inside a step), with every column the next block can touch, so W = 128 columns at dyadic order 0 hold grids
// of any width.  For the backward pass the forward solution goes to the wave's scratch in [band][step][lane] order (fp32,
// coalesced 256-B rows); the reverse sweep writes each lane's partial block sum of GG (over the r columns of a block) in the
// same order, and ring_S adds the r rows of a block in row order: no floating-point atomics, the bits depend on the inputs.
#pragma once

#include "sig_common.h"

namespace sigsvgd {
// The exact adjoint is a compile-time variant of the kernels on this sweep, named through their I/O
// type: ExactIO<float> / ExactIO<double> in the place of float / double.  A flag of its own among the template parameters would
// rename every instantiation the kernels already have; this way those keep their names and, statement for statement, their code.
// NaN-marked tails are named the same way: NanTailIO<float> / NanTailIO<double>.  Their kernels read each
// path's length (nan_tail_lengths below) and solve each pair on its own grid; the sweeps are the unflagged ones.
// The log-domain solve again: LogIO<float> / LogIO<double>.  Its sweeps carry a running power-of-two
// scale (ring_forward / ring_reverse with LOG), the kernels store ln K and file the S partials already divided by K.
// The normalised kernel once more: NormIO<float> / NormIO<double>, log_k as well, so the sweeps are LogIO's.
// Behind ring_log_finish the two-sided kernel forms K^ = exp(ln K - (a_i + b_j) / 2) from the diagonals' logarithms (norm_logs
// below), stores it and weights the pair's gradient by it; the paired kernel is the diagonal pass that writes those logarithms.
template <typename T>
struct ExactIO {};
template <typename T>
struct NanTailIO {};
template <typename T>
struct LogIO {};
template <typename T>
struct NormIO {};
template <typename T>
struct RingIO {
    using type = T;
    static constexpr bool exact = false, nan_tails = false, log_k = false, normalized = false;
};
template <typename T>
struct RingIO<ExactIO<T>> {
    using type = T;
    static constexpr bool exact = true, nan_tails = false, log_k = false, normalized = false;
};
template <typename T>
struct RingIO<NanTailIO<T>> {
    using type = T;
    static constexpr bool exact = false, nan_tails = true, log_k = false, normalized = false;
};
template <typename T>
struct RingIO<LogIO<T>> {
    using type = T;
    static constexpr bool exact = false, nan_tails = false, log_k = true, normalized = false;
};
template <typename T>
struct RingIO<NormIO<T>> {
    using type = T;
    static constexpr bool exact = false, nan_tails = false, log_k = true, normalized = true;
};

// The lengths of a launch with SIGSVGD_FLAG_NAN_TAILS: int lenX[nX], then int lenY[nY] (nY = 0 where Y is X: one array serves
// both slots), padded to 256 B, at the head of the workspace right before the forward scratch.  The kernels find them from the
// scratch pointer they already have, so no argument struct changes.
__host__ __device__ inline size_t nan_tail_bytes(int nX, int nY)
{
    return (((size_t)nX + (size_t)nY) * sizeof(int) + 255) & ~(size_t)255;
}
__device__ __forceinline__ const int *nan_tail_lengths(const float *wsk, int nX, int nY)
{
    return reinterpret_cast<const int *>(reinterpret_cast<const unsigned char *>(wsk) - nan_tail_bytes(nX, nY));
}


// The diagonals' logarithms of a launch with SIGSVGD_FLAG_NORMALIZED: double a[nX] = ln K(X_i, X_i),
// then double b[nY] = ln K(Y_j, Y_j) (nY = 0 where Y is X: one array serves both slots), padded to 256 B, at the head of the
// workspace right before the forward scratch, where the lengths of a launch with NaN-marked tails are (the two flags exclude
// each other).  The kernels find them from the scratch pointer they already have, so no argument struct changes.
__host__ __device__ inline size_t norm_log_bytes(int nX, int nY)
{
    return (((size_t)nX + (size_t)nY) * sizeof(double) + 255) & ~(size_t)255;
}
__device__ __forceinline__ const double *norm_logs(const float *wsk, int nX, int nY)
{
    return reinterpret_cast<const double *>(reinterpret_cast<const unsigned char *>(wsk) - norm_log_bytes(nX, nY));
}
// A gradient launch keeps the pairs' weights U_ij = w_ij K^_ij too, double U[A][B] padded to 256 B right before the logarithms:
// the two-sided kernel stores each as it forms it, in fp64 (a K^ below the I/O type's range still counts under a large w), and
// long_norm_sums adds the rows and columns.
__host__ __device__ inline size_t norm_weight_bytes(int A, int B)
{
    return ((size_t)A * (size_t)B * sizeof(double) + 255) & ~(size_t)255;
}
__device__ __forceinline__ double *norm_weights(float *wsk, int nX, int nY, int A, int B)
{
    return reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(wsk) - norm_log_bytes(nX, nY) - norm_weight_bytes(A, B));
}

namespace {
constexpr int kRingMaxCells = 8192;                 // P and Q
constexpr size_t kRingDoubles = 8192;               // 64 KB of increments per wave
constexpr size_t kRingMaxScratch = (size_t)1 << 30; // the launch's scratch: each family lowers its grid to stay below it
constexpr size_t kRingMaxLds = 160 * 1024;

struct RingPlan {
    int r, P, Q, nbands, nsteps, nrow, W;
    size_t per_wave;    // bytes of one wave's scratch (0 for forward-only launches: the forward sweep keeps nothing)
    size_t lds;         // bytes of one wave's LDS
    long long resident; // waves the device holds at that LDS (at most 8 per CU)
};

// The geometry of a launch on M x N coarse grids at dyadic order n.  The LDS is the ring of nrow x W fp64 increments, the
// boundary row [Q + 2], the per-lane dump cells [64], and the caller's [nrow + 1][row_doubles] behind them.  Refuses grids
// past kRingMaxCells and LDS past 160 KiB (messages prefixed by `who`).
int ring_make_plan(int M, int N, int n, int want_grad, int row_doubles, const char *who, RingPlan &pl)
{
    pl.r = 1 << n;
    const long long P = (long long)pl.r * (M - 1), Q = (long long)pl.r * (N - 1);
    pl.nbands = (int)((P + kWave - 1) / kWave);
    pl.nsteps = (int)(Q + kWave - 1);
    pl.per_wave = want_grad ? ((size_t)2 * pl.nbands * pl.nsteps * kWave + kWave) * sizeof(float) : 0;
    if (P > kRingMaxCells || Q > kRingMaxCells) {
        set_error("%s: refined grid %lld x %lld exceeds %d x %d (one wave's scratch would be %zu B)", who, P, Q,
                  kRingMaxCells, kRingMaxCells, pl.per_wave);
        return SIGSVGD_E_UNSUPPORTED;
    }
    pl.P = (int)P;
    pl.Q = (int)Q;
    pl.nrow = n <= 6 ? (kWave >> n) : 1; // coarse rows of a band of 64 rows
    int W = 1;
    while (W < N - 1) W <<= 1;
    int Wcap = 1;
    while ((size_t)Wcap * 2 * pl.nrow <= kRingDoubles) Wcap <<= 1;
    pl.W = W < Wcap ? W : Wcap; // >= the (126 >> n) + 2 columns a block of 64 steps can touch
    pl.lds = ((size_t)pl.nrow * pl.W + pl.Q + 2 + kWave + (size_t)(pl.nrow + 1) * row_doubles) * sizeof(double);
    if (pl.lds > kRingMaxLds) {
        set_error("%s: per-wave state needs %zu B of LDS (> 160 KiB)", who, pl.lds);
        return SIGSVGD_E_UNSUPPORTED;
    }
    const int per_cu = (int)(kRingMaxLds / pl.lds);
    pl.resident = (long long)device_cu_count() * (per_cu > 8 ? 8 : per_cu);
    return SIGSVGD_OK;
}

// A launch with SIGSVGD_FLAG_LOG_K on plan pl: one int per block of 64 sweep steps beside the boundary
// row in LDS (behind the caller's rows), and the forward sweep's [band][block] exponents in the wave's scratch, behind its spare
// row (a forward-only launch keeps them too, alone: one forward sweep for both).  The resident waves follow the larger LDS;
// refuses as ring_make_plan does.
__host__ __device__ inline int ring_log_blocks(int nsteps) { return (nsteps + kWave - 1) / kWave; }
int ring_log_plan(const char *who, RingPlan &pl)
{
    const size_t nblk = (size_t)ring_log_blocks(pl.nsteps);
    pl.lds += ((nblk + 1) * sizeof(int) + 7) & ~(size_t)7;
    pl.per_wave += (size_t)pl.nbands * nblk * sizeof(int);
    if (pl.lds > kRingMaxLds) {
        set_error("%s: per-wave state needs %zu B of LDS (> 160 KiB) with SIGSVGD_FLAG_LOG_K", who, pl.lds);
        return SIGSVGD_E_UNSUPPORTED;
    }
    const int per_cu = (int)(kRingMaxLds / pl.lds);
    pl.resident = (long long)device_cu_count() * (per_cu > 8 ? 8 : per_cu);
    return SIGSVGD_OK;
}

// the bytes a caller gives for `bytes` of workspace (+ the slack of aligning its pointer; 0 when nothing is needed)
size_t ring_ws_total(size_t bytes) { return bytes ? bytes + 256 : 0; }

// `base` = ws aligned to 256 B (NULL when need is 0); SIGSVGD_E_WORKSPACE when the caller's buffer is smaller than `need`
int ring_ws_base(const char *who, void *ws, size_t ws_bytes, size_t need, unsigned char *&base)
{
    if (ws_bytes < need || (need && !ws)) {
        set_error("%s: workspace %zu B too small, required %zu B", who, ws_bytes, need);
        return SIGSVGD_E_WORKSPACE;
    }
    base = need ? reinterpret_cast<unsigned char *>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255) : nullptr;
    return SIGSVGD_OK;
}

// a workspace query: *bytes = the total() of the plan that make(plan) fills
template <typename Plan, typename Make>
int ring_plan_total(size_t *bytes, Make &&make)
{
    Plan pl;
    const int rc = make(pl);
    if (rc) return rc;
    *bytes = pl.total();
    return SIGSVGD_OK;
}

// ---- the launch of a kernel family on the ring sweep -----------------------------------------------------------------------
// A family F names its kernels: F::Args (the kernel's one argument), F::kernel<IO, NAIVE, GRAD, KIND>() (the instantiation's
// address), F::has_kind (false: one kernel for every static kernel, KIND = 0), F::has_fwd_only (false: GRAD = true only) and
// the two texts of a failure.  ring_launch maps the runtime (dtype, kind, naive, grad) to the instantiation, raises its LDS
// limit and launches pl.grid wavefronts with pl.lds bytes of LDS each; only instantiations the family has are named.  The
// kinds SIGSVGD_STATIC_IMQ and _RQ are instantiated with the default stencil only, and so are the
// Matern kinds, which ring_launch_solver serves but ring_launch_kind does not name: gram_long.hip launches them from a
// translation unit of their own.
template <typename F, typename IO, bool NAIVE, bool GRAD, int KIND, typename Plan>
hipError_t ring_launch_one(const Plan &pl, hipStream_t stream, const typename F::Args &a)
{
    constexpr auto kernel = F::template kernel<IO, NAIVE, GRAD, KIND>();
    const hipError_t e = raise_lds_limit<kernel>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(kWave), pl.lds, stream, a);
    return hipSuccess;
}
template <typename F, typename IO, int KIND, typename Plan>
hipError_t ring_launch_solver(bool naive, bool grad, const Plan &pl, hipStream_t stream, const typename F::Args &a)
{
    // (IMQ, rational quadratic and Matern have the default stencil only: the entry points refuse NAIVE_SOLVER before this)
    constexpr bool has_naive = KIND == SIGSVGD_STATIC_RBF || KIND == SIGSVGD_STATIC_LINEAR;
    if constexpr (!has_naive) {
        if (naive) return hipErrorInvalidValue;
        if constexpr (F::has_fwd_only) {
            if (!grad) return ring_launch_one<F, IO, false, false, KIND>(pl, stream, a);
        }
        return ring_launch_one<F, IO, false, true, KIND>(pl, stream, a);
    } else {
        if constexpr (F::has_fwd_only) {
            if (!grad)
                return naive ? ring_launch_one<F, IO, true, false, KIND>(pl, stream, a)
                             : ring_launch_one<F, IO, false, false, KIND>(pl, stream, a);
        }
        return naive ? ring_launch_one<F, IO, true, true, KIND>(pl, stream, a)
                     : ring_launch_one<F, IO, false, true, KIND>(pl, stream, a);
    }
}
template <typename F, typename IO, typename Plan>
hipError_t ring_launch_kind(int kind, bool naive, bool grad, const Plan &pl, hipStream_t stream, const typename F::Args &a)
{
    if constexpr (F::has_kind) {
        if (kind == SIGSVGD_STATIC_IMQ) return ring_launch_solver<F, IO, SIGSVGD_STATIC_IMQ>(naive, grad, pl, stream, a);
        if (kind == SIGSVGD_STATIC_RQ) return ring_launch_solver<F, IO, SIGSVGD_STATIC_RQ>(naive, grad, pl, stream, a);
        if (kind != SIGSVGD_STATIC_RBF) return ring_launch_solver<F, IO, SIGSVGD_STATIC_LINEAR>(naive, grad, pl, stream, a);
    }
    return ring_launch_solver<F, IO, SIGSVGD_STATIC_RBF>(naive, grad, pl, stream, a);
}
template <typename F, typename Plan>
int ring_launch(int dtype, int kind, bool naive, bool grad, const Plan &pl, hipStream_t stream, const typename F::Args &a)
{
    hipError_t e = dtype == SIGSVGD_F64 ? ring_launch_kind<F, double>(kind, naive, grad, pl, stream, a)
                                        : ring_launch_kind<F, float>(kind, naive, grad, pl, stream, a);
    if (e != hipSuccess) return hip_fail(e, F::attr_failed);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, F::launch_failed);
    return SIGSVGD_OK;
}

// one wave's view of the plan: its geometry, its LDS and (GRAD) its scratch
struct RingWave {
    int N, n, r, P, Q, W, nbands, nsteps;
    double inv_r2;
    double *ring;   // [nrow][W]: D[a0 + row][b] at column slot b & (W - 1)
    double *rowbuf; // [Q + 2]
    double *dump;   // [64]: where the lanes that have nothing to hand over store; the caller's LDS follows
    float *wsk;     // forward solution [band][step][lane]
    float *wss;     // S partials, same order as the forward solution
    float *spare;   // the lane's cell of the spare row
};
template <bool GRAD, typename Args>
__device__ __forceinline__ RingWave ring_wave(const Args &a, unsigned char *smem)
{
    RingWave w;
    w.N = a.N; w.n = a.n; w.r = a.r; w.P = a.P; w.Q = a.Q; w.W = a.W; w.nbands = a.nbands; w.nsteps = a.nsteps;
    w.inv_r2 = a.inv_r2;
    w.ring = reinterpret_cast<double *>(smem);
    w.rowbuf = w.ring + (size_t)a.nrow * a.W;
    w.dump = w.rowbuf + (a.Q + 2);
    const size_t area = (size_t)a.nbands * a.nsteps * kWave;
    w.wsk = GRAD ? a.wsk + (size_t)blockIdx.x * a.wsk_per_block : nullptr;
    w.wss = GRAD ? w.wsk + area : nullptr;
    w.spare = GRAD ? w.wss + area + threadIdx.x : nullptr;
    return w;
}

// ---- the log-domain solve (SIGSVGD_FLAG_LOG_K) -------------------------------------------------------
// Both sweeps are linear in the solution, so a band may carry it times 2^-E: between blocks of 64 sweep steps the wave takes the
// largest exponent of its lanes' live values and, once that has drifted past kLogDrift, multiplies them by its power of two and
// adds it to the running exponent E (F in the reverse sweep).  Powers of two only: every rounding of the sweep commutes with
// them, so the mantissas are the unscaled solve's.  Every band starts at E = 0 (its first cells sit on the grid's edge, where
// the solution is 1).  What a band leaves for the next one in the boundary row is under the exponent of the block that wrote it:
// etab keeps one int per block beside the row, and each block brings the 64 entries it is about to read to its own exponent
// first (one entry per lane) before it puts its own exponent in the table, in place.  The stored forward solution is the scaled
// one, with the [band][block] exponents in ews; the reverse sweep multiplies each value it reads back by 2^(E_fwd + F - E) / m
// (m 2^E the pair's K), so what it files in wss is the relative sensitivity GG / K, O(1), and everything behind S is unchanged.
struct RingLog {
    int *etab;    // LDS [blocks + 1]
    int *ews;     // the wave's scratch [nbands][blocks]: the forward sweep's exponents
    int nblk;
    int E;        // the exponent of the value ring_forward returned
    double inv_m; // 1 / that value (NaN where it is <= 0: the pair's gradient is NaN, as its ln K)
};
constexpr int kLogDrift = 8;
template <bool GRAD, typename Args>
__device__ __forceinline__ RingLog ring_log(const Args &a, const RingWave &w, void *lds_behind_rows)
{
    RingLog lg;
    lg.etab = static_cast<int *>(lds_behind_rows);
    lg.ews = reinterpret_cast<int *>(GRAD ? w.spare - threadIdx.x + kWave : a.wsk + (size_t)blockIdx.x * a.wsk_per_block);
    lg.nblk = ring_log_blocks(w.nsteps);
    lg.E = 0;
    lg.inv_m = 1.0;
    return lg;
}
// the largest binary exponent of a and b over the lanes with `valid` (the same in every lane, from a scalar register)
__device__ __forceinline__ int wave_max_exp(bool valid, double a, double b)
{
    int e = valid ? max(__builtin_amdgcn_frexp_exp(a), __builtin_amdgcn_frexp_exp(b)) : -4096;
#pragma unroll
    for (int o = kWave / 2; o; o >>= 1) e = max(e, __shfl_xor(e, o));
    return __builtin_amdgcn_readfirstlane(e);
}
// ln K of the pair from the forward sweep's value (in the lane that holds row P - 1) and exponent, in every lane; sets inv_m.
// As much of the exponent as fp64 holds goes back into the value before the logarithm (a K of order 1 under a large wave-wide
// exponent would otherwise be the difference of two large terms): where K fits fp64 the result is log(K) itself.
__device__ __forceinline__ double ring_log_finish(const RingWave &w, double Kval, RingLog &lg)
{
    const double m = __shfl(Kval, (w.P - 1) & (kWave - 1));
    const bool pos = m > 0.0;
    lg.inv_m = pos ? 1.0 / m : __builtin_nan("");
    const int e0 = min(max(lg.E, -900), 900); // (m is within 2^-120 .. 2^120 of the wave's largest value, which is near 1)
    return pos ? __builtin_fma((double)(lg.E - e0), 6.93147180559945309417e-01, log(ldexp(m, e0))) : __builtin_nan("");
}

// ---- forward sweep of one pair over all bands: returns the final value of the lane that holds row P - 1 ----------------------
// fill(a0, b_lo, b_hi): coarse columns b_lo .. b_hi of the increment rows a0 .. a0 + nrow - 1 into the ring, between barriers;
// band(a0): called as each band starts, before its first fill.  (The step of gram_generic_kernel: branch-free, results of
// lanes outside the grid dropped by selects, the operands of step s + 1 fetched during step s.)
// EXACT (default stencil with GRAD only): what the sweep keeps for the reverse sweep is not K00 =
// K_fwd[p][q] but the cell's derivative of the step in its increment, c = (K10 + K01) (1/2 + g/6) + K00 g/6, in the same slot;
// the arithmetic that produces K is the same.
// LOG (see RingLog above): the value returned is times 2^-lg->E.
template <bool NAIVE, bool GRAD, bool EXACT = false, bool LOG = false, typename Fill, typename Band>
__device__ __forceinline__ double ring_forward(const RingWave &w, Fill &&fill, Band &&band, [[maybe_unused]] RingLog *lg = nullptr)
{
    static_assert(!EXACT || (GRAD && !NAIVE), "the exact adjoint is the default stencil's, and a gradient launch's");
    static_assert(!LOG || (!EXACT && !NAIVE), "the log-domain solve is the default stencil's GG solve");
    const int lane = threadIdx.x;
    const int N = w.N, n = w.n, P = w.P, Q = w.Q, W = w.W, nsteps = w.nsteps;
    double *rowbuf = w.rowbuf;
    double Kval = 1.0;
    [[maybe_unused]] int E = 0;        // LOG: the band's values are times 2^-E
    [[maybe_unused]] double one = 1.0; // LOG: 2^-E, the grid's upper edge
    for (int kb = 0; kb < w.nbands; ++kb) {
        const int p = kb * kWave + lane;
        const bool rowvalid = p < P;
        const bool first = kb == 0;
        if constexpr (LOG) {
            E = 0;
            one = 1.0;
        }
        const int a0 = (kb * kWave) >> n;
        band(a0);
        const double *Drow = w.ring + (size_t)((min(p, P - 1) >> n) - a0) * W;
        float *wp = GRAD ? w.wsk + (size_t)kb * nsteps * kWave + lane : nullptr;
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
            if constexpr (LOG) {
                if (s0 > 0) {
                    const int e = wave_max_exp(rowvalid, cur, upprev);
                    if (e > kLogDrift || e < -kLogDrift) {
                        cur = ldexp(cur, -e);
                        upprev = ldexp(upprev, -e);
                        rb = ldexp(rb, -e);
                        E += e;
                        one = ldexp(1.0, -E);
                    }
                }
                // the entries of the boundary row this block reads, s0 + 2 .. s0 + 65 (lane 63 of the band above stored entry
                // k on its step k + 62), to this block's exponent; then the block's own exponent for the band below
                const int idx = s0 + 2 + lane;
                if (!first && idx <= Q) rowbuf[idx] = ldexp(rowbuf[idx], lg->etab[(idx + kWave - 2) >> 6] - E);
                if (lane == 0) lg->etab[s0 >> 6] = lg->ews[kb * lg->nblk + (s0 >> 6)] = E;
                __syncthreads();
            }
            double gf = Drow[(min(max(s0 - lane, 0), Q - 1) >> n) & (W - 1)];
            const int s1 = min(s0 + kWave, nsteps);
            for (int s = s0; s < s1; ++s) {
                const int q = s - lane;
                const bool active = rowvalid && q >= 0 && q < Q;
                const double gfn = Drow[(min(max(q + 1, 0), Q - 1) >> n) & (W - 1)];
                const double rbr = rowbuf[min(s + 2, Q)];
                const double rbn = first ? (LOG ? one : 1.0) : rbr;
                double up_in = shfl_up_f64(cur);
                up_in = (lane == 0) ? rb : up_in;
                const double nw = stencil(cur, up_in, upprev, gf * w.inv_r2, NAIVE);
                if constexpr (EXACT) { // c[p][q] at [step][lane], where K_fwd[p][q] goes otherwise
                    const double g6 = gf * w.inv_r2 * (1.0 / 6.0);
                    const float kst = (float)__builtin_fma(cur + up_in, 0.5 + g6, upprev * g6);
                    asm volatile("global_store_dword %0, %1, off" ::"v"(wp + (size_t)s * kWave), "v"(kst));
                } else if (GRAD) { // K_fwd[p][q] at [step][lane] (issued from inline asm: no wait for the previous step's store)
                    const float kst = (float)upprev;
                    asm volatile("global_store_dword %0, %1, off" ::"v"(wp + (size_t)s * kWave), "v"(kst));
                }
                *((lane == kWave - 1 && active) ? rowbuf + (q + 1) : w.dump + lane) = nw;
                cur = active ? nw : cur;
                upprev = active ? up_in : upprev;
                gf = gfn;
                rb = rbn;
            }
        }
        if (p == P - 1) Kval = cur;
    }
    if constexpr (LOG) lg->E = E;
    return Kval;
}

// ---- reverse sweep: GG = K_fwd[p][q] K_rev[p+1][q+1], summed over the r columns of a block per lane, into w.wss -------------
// (fill and band as in ring_forward; the caller makes the forward solution visible first)
// EXACT: the adjoint of the default stencil itself.  With lambda(p, q) = dK[P][Q] / dK[p+1][q+1],
// alpha = A(g) lambda and beta = B(g) lambda of the lane's own cell (A = 1 + g/2 + g^2/12, B = 1 - g^2/12),
//   lambda(p, q) = alpha(p, q+1) + h(p+1, q),   h(p+1, q) = alpha(p+1, q) - beta(p+1, q+1),   lambda(P-1, Q-1) = 1,
// alpha = beta = 0 outside the grid.  Lane p + 1 is one column ahead, so h is the one number it formed on the step before
// (its newest alpha less the beta of the step before that): the one shfl_down_f64 of the step moves it, and the band below
// hands its row of h over in rowbuf.  The sum filed in w.wss is lambda c, c from ring_forward<.., EXACT>.
// LOG (see RingLog above): the same scheme under a running exponent F of its own; the sum filed in
// w.wss is GG / K, from lg->E and lg->inv_m of the forward sweep.
template <bool NAIVE, bool EXACT = false, bool LOG = false, typename Fill, typename Band>
__device__ __forceinline__ void ring_reverse(const RingWave &w, Fill &&fill, Band &&band, [[maybe_unused]] RingLog *lg = nullptr)
{
    static_assert(!EXACT || !NAIVE, "the exact adjoint is the default stencil's");
    static_assert(!LOG || (!EXACT && !NAIVE), "the log-domain solve is the default stencil's GG solve");
    const int lane = threadIdx.x;
    const int N = w.N, n = w.n, P = w.P, Q = w.Q, W = w.W, nsteps = w.nsteps;
    double *rowbuf = w.rowbuf;
    for (int kb = w.nbands - 1; kb >= 0; --kb) {
        const int p = kb * kWave + lane;
        const bool rowvalid = p < P;
        const int L = min(kWave, P - kb * kWave);
        const int a0 = (kb * kWave) >> n;
        band(a0);
        const double *Drow = w.ring + (size_t)((min(p, P - 1) >> n) - a0) * W;
        float *wsrow = w.wss + (size_t)kb * nsteps * kWave + lane;
        const float *wrow = w.wsk + (size_t)kb * nsteps * kWave + lane; // K_fwd[p][q] at step lane + q
        const bool lastband = kb == w.nbands - 1;
        const bool hands_over = lane == 0 && kb > 0;
        double cur = 1.0, dprev = 1.0, sb = 0.0;
        [[maybe_unused]] double bprev = 0.0; // EXACT: cur = h, dprev = the lane's newest alpha, bprev = its newest beta
        if constexpr (EXACT) cur = dprev = 0.0;
        [[maybe_unused]] int F = 0, Rsplit = 0;                   // LOG: the band's values are times 2^-F
        [[maybe_unused]] double one = 1.0, fsA = 1.0, fsB = 1.0; // LOG: 2^-F; what a stored row >= / < Rsplit is multiplied by
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
            if constexpr (LOG) {
                if (sp0 > 0) {
                    const int e = wave_max_exp(rowvalid, cur, dprev);
                    if (e > kLogDrift || e < -kLogDrift) {
                        cur = ldexp(cur, -e);
                        dprev = ldexp(dprev, -e);
                        F += e;
                        one = ldexp(1.0, -F);
                    }
                }
                // the entries of the boundary row this block reads, Q - 1 - sp0 down to Q - 64 - sp0 (lane 0 of the band below,
                // of Lb rows, stored entry k on its step Q + Lb - 2 - k), to this block's exponent; the table entries are read
                // before the block's own exponent goes in
                const int idx = Q - 1 - sp0 - lane, Lb = min(kWave, P - (kb + 1) * kWave);
                const bool mine = !lastband && idx >= 0;
                const int fb = mine ? lg->etab[(Q + Lb - 2 - idx) >> 6] : 0;
                __syncthreads();
                if (mine) rowbuf[idx] = ldexp(rowbuf[idx], fb - F);
                if (lane == 0) lg->etab[sp0 >> 6] = F;
                __syncthreads();
                // the stored forward rows of this block are R down to R - 63: at most two blocks of the forward sweep
                const int *ef = lg->ews + kb * lg->nblk, hb = max(R, 0) >> 6;
                Rsplit = hb << 6;
                fsA = ldexp(lg->inv_m, ef[hb] + F - lg->E);
                fsB = ldexp(lg->inv_m, ef[max(hb - 1, 0)] + F - lg->E);
            }
            double gf = Drow[(min(max(q, 0), Q - 1) >> n) & (W - 1)];
            double rbk = rowbuf[max(Q - 1 - sp0, 0)];
            rb = lastband ? (LOG ? one : 1.0) : rbk;
            if constexpr (EXACT) rb = lastband ? (sp0 == 0 ? 1.0 : 0.0) : rbk; // (below the grid 0; the 1 is lambda(P-1, Q-1))
            // (the groups past nsp have no lane inside the grid and change nothing; their S stores go to the spare row)
            for (int sp1 = sp0; sp1 < sp0 + kWave; sp1 += KPF) {
#pragma unroll
                for (int u = 0; u < KPF; ++u, --q, --R) {
                    const int sp = sp1 + u;
                    const bool active = rowvalid && q >= 0 && q < Q;
                    const double gfn = Drow[(min(max(q - 1, 0), Q - 1) >> n) & (W - 1)];
                    const double rbr = rowbuf[max(Q - 2 - sp, 0)];
                    double rbn = lastband ? (LOG ? one : 1.0) : rbr;
                    if constexpr (EXACT) rbn = lastband ? 0.0 : rbr;
                    double kf = (double)kfr[u];
                    if constexpr (LOG) kf *= R >= Rsplit ? fsA : fsB;
                    kfr[u] = wrow[(size_t)max(R - KPF, 0) * kWave];
                    double down_in = shfl_down_f64(cur);
                    down_in = (lane == L - 1) ? rb : down_in;
                    if constexpr (EXACT) {
                        const double g = gf * w.inv_r2, b12 = g * g * (1.0 / 12.0);
                        const double lam = dprev + down_in;
                        const double al = __builtin_fma(lam, __builtin_fma(g, 0.5, b12), lam); // alpha
                        const double be = __builtin_fma(-lam, b12, lam);                       // beta
                        const double h = al - bprev;
                        sb = active ? __builtin_fma(kf, lam, sb) : sb;
                        const bool done = active && (q & (w.r - 1)) == 0; // the block's last (lowest) column
                        const float sst = done ? (float)(sb * w.inv_r2) : 0.f;
                        asm volatile("global_store_dword %0, %1, off" ::"v"(R >= 0 ? wsrow + (size_t)R * kWave : w.spare), "v"(sst));
                        sb = done ? 0.0 : sb;
                        *((hands_over && active) ? rowbuf + q : w.dump + lane) = h;
                        cur = active ? h : cur;
                        dprev = active ? al : dprev;
                        bprev = active ? be : bprev;
                    } else {
                        sb = active ? __builtin_fma(kf, dprev, sb) : sb;
                        const bool done = active && (q & (w.r - 1)) == 0; // the block's last (lowest) column
                        const float sst = done ? (float)(sb * w.inv_r2) : 0.f;
                        asm volatile("global_store_dword %0, %1, off" ::"v"(R >= 0 ? wsrow + (size_t)R * kWave : w.spare), "v"(sst));
                        sb = done ? 0.0 : sb;
                        const double nw = stencil(cur, down_in, dprev, gf * w.inv_r2, NAIVE);
                        *((hands_over && active) ? rowbuf + q : w.dump + lane) = nw;
                        cur = active ? nw : cur;
                        dprev = active ? down_in : dprev;
                    }
                    gf = gfn;
                    rb = rbn;
                }
            }
        }
    }
}

// S[aa][bb]: the r lane partials of block (aa, bb) in row order (lane pp & 63 of band pp >> 6 filed the partial of row pp,
// block column bb, on reverse step (pp & 63) + bb r); the caller makes the reverse sweep's stores visible first
__device__ __forceinline__ double ring_S(const RingWave &w, int aa, int bb)
{
    double s = 0.0;
    for (int i = 0; i < w.r; ++i) {
        const int pp = aa * w.r + i, l = pp & (kWave - 1);
        s += (double)w.wss[((size_t)(pp >> 6) * w.nsteps + l + (size_t)bb * w.r) * kWave + l];
    }
    return s;
}
} // namespace
} // namespace sigsvgd
