// pair_bands_kernel, its arguments and the launchers of its instantiations (bands_launch_one / _solver / _kind).  Included by
// pair_bands.hip (plan, launch and the fp64-I/O instantiations), pair_bands_f32.hip (fp32 I/O) and pair_bands_matern.hip (the
// Matern kinds, both I/O types).
//
// Band-parallel schedule of the paired long-path solver.
//
// gram_long_kernel's paired mode walks the nbands = ceil(P / 64) bands of a pair one after the other on one wavefront.  Here
// a workgroup of NB wavefronts takes one pair: wavefront w sweeps bands w, w + NB, w + 2 NB, ... and the bands run as a
// pipeline, each a fixed number of phases behind the band it depends on.  The per-cell arithmetic is the serial kernel's --
// the same static-kernel evaluations, the increment formed as (k(x_{a+1}, y_{b+1}) - k(x_{a+1}, y_b)) - (k(x_a, y_{b+1}) -
// k(x_a, y_b)), the same stencil, the same per-lane block sums of the reverse sweep in the same [band][step][lane] scratch --
// so K and both gradients have the serial kernel's bits.
//
// Synchronisation is one __syncthreads() per phase of kPH = 16 sweep steps, in a loop whose trip count comes from the plan:
// every wave reaches every barrier, a wave without work in a phase skips the work only.
//
// Forward lag.  Band b on step s (lane l at column q = s - l) gives lane 0 the boundary entry s + 1 and prefetches entry
// min(s + 2, Q); entry e = q + 1 is the value lane 63 of band b - 1 computes at column q, on its step e + 62.  Phase c of the
// consumer (steps 16 c .. 16 c + 15) therefore reads entries up to 16 c + 17, which the producer writes on steps up to
// 16 c + 79: inside its phase c + 4.  The consumer's phase c may run once the producer has finished phase c + 4, i.e. the
// consumer runs kLag = 5 phases behind, and everything it reads was written before the last barrier.  (With phases of 64
// steps the same count gives entries up to 64 c + 65 on step 64 c + 127, a lag of 2 phases = 128 steps against 80 here.)
// While the consumer reads entries 16 c + 1 .. 16 c + 17 the producer, in its phase c + 5, writes 16 c + 18 .. 16 c + 33: the
// forward sweep needs a circular window of 33 entries.  The reverse sweep needs more (below); kWin = 128 holds both.
//
// Reverse lag.  The last band leads and lane 0 hands over.  Count entries from the right edge, e' = Q - 1 - q.  A band of L
// rows has lane l at column Q - 1 + (L - 1 - l) - sp on step sp, so its lane 0 writes entry e' on step e' + L - 1 <= e' + 63
// (the last band's L < 64 rows only make it earlier).  The consumer (always 64 rows) gives lane 63 entry sp on step sp and
// prefetches entry sp + 1: phase c reads entries up to 16 c + 16, written by step 16 c + 79 at the latest, again inside the
// producer's phase c + 4.  The same lag of 5 holds.  The window is another matter: a last band of L rows runs ahead of its
// consumer, in its phase c + 5 it writes entries up to 16 (c + 5) + 15 - (L - 1), that is 16 c + 95 when L = 1, while the
// consumer still reads from entry 16 c on: (kLag + 1) kPH = 96 entries are live at once (static_assert below).
//
// Schedule.  Band k NB + j (reverse: counted from the last band) starts at kernel phase k stride + kLag j with
// stride = max(nph + kLag, kLag NB), nph the phases of one band.  The kLag on top of nph keeps a wave's next band from
// writing the first entries of a window while the neighbour still reads the last entries of the band before through it.
// Inside a round every interface is the 128-entry window.  The seam between rounds (wave NB - 1 to wave 0) is different: wave
// 0 cannot start band (k + 1) NB before it has finished band k NB, which is up to nph - kLag (NB - 1) phases after the
// producer started, so the seam keeps a full boundary row of Q + 2 doubles, once per workgroup, and only when nbands > NB.
//
// Increments.  At order 0 there is no ring: in the throughput half of a phase each lane evaluates the static kernel of its
// row's lower point x_{p+1} at the 17 columns of the phase, the column differences rd of the upper point x_p arrive from the
// lane above (which was at the same column one step earlier; lane 0 takes them from the boundary window, the first band
// evaluates x_0 itself) and the 16 increments stay in registers for the dependent half.  The reverse sweep mirrors it with the
// upper point evaluated and the lower one shifted in from the lane below.  From order 1 on each wave keeps the serial
// kernel's increment ring with the (126 >> n) + 2 columns a block of 64 steps can touch instead of the 64 KB cap, filled by
// the serial kernel's column-owner loop.
#pragma once

#include "long_static.h"
#include "pair_bands.h"

namespace sigsvgd {

struct BandsArgs {
    const void *X, *Y, *grad_out;
    void *K_out, *gradX, *gradY;
    float *wsk;
    size_t wsk_per_block; // floats
    int A, M, N, d, n, r, P, Q, nbands, nsteps, nrow, W, NB, nph, stride, phases, seam;
    unsigned wave_doubles, seam_doubles;
    double inv_h, inv_r2;
};

namespace {
constexpr int kPH = 16;   // sweep steps per phase
constexpr int kLag = 5;   // phases between neighbouring bands (derivation above)
constexpr int kWin = 128; // entries of a boundary window, a power of two
static_assert(kWin >= (kLag + 1) * kPH && (kWin & (kWin - 1)) == 0,
              "a one-row last band writes up to (kLag + 1) kPH entries ahead of what its consumer still reads");
constexpr int kMaxNB = 8;   // waves per pair: 512 threads leave the kernel 256 VGPRs; at 16 waves (128 VGPRs) it spills


// LDS writes of this wave before, reads of them after: LDS operations of one wave complete in order, the fence keeps the
// compiler from moving them across
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// static_grad_pass (long_static.h) with its outer passes dealt round-robin to the NB waves of the workgroup: every output
// entry is still written once, by one lane, from the same sum in the same order
template <int KIND, bool OWN_X, typename IO, typename Store>
__device__ __forceinline__ void static_grad_pass_rr(const RingWave &rw, const IO *own, int To, const IO *oth, int Tt, int d,
                                                    double inv_h, int lane, int wave, int NB, Store &&store)
{
    int turn = 0;
    for (int o0 = 0; o0 < To; o0 += kWave - 1, turn = turn + 1 == NB ? 0 : turn + 1)
        if (turn == wave) static_grad_pass_one<KIND, OWN_X>(rw, own, To, oth, Tt, d, inv_h, lane, o0, store);
}
} // namespace

template <typename IO, bool NAIVE, bool GRAD, int KIND>
__global__ __launch_bounds__(kMaxNB * kWave) void pair_bands_kernel(BandsArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int M = a.M, N = a.N, d = a.d, n = a.n, P = a.P, Q = a.Q, W = a.W, nrow = a.nrow, NB = a.NB, nsteps = a.nsteps;
    const bool reg = n == 0; // increments formed in registers (no ring)
    double *lds = reinterpret_cast<double *>(smem_raw);
    // LDS: [seam row (and, order 0, its rd row)] then per wave [window (and rd window)][dump 64][xs (nrow + 1) d][ring nrow W]
    const int win_doubles = reg ? 2 * kWin : kWin;
    double *mine = lds + a.seam_doubles + (size_t)wave * a.wave_doubles;
    double *dump = mine + win_doubles;
    double *xs = dump + kWave; // points a0 .. a0 + nrow of X_i (clamped to M - 1) of the band this wave sweeps
    double *ring = xs + (size_t)(nrow + 1) * d;
    // the boundary this wave writes (its own window; the last wave writes the seam row when there is one) and the one it
    // reads (the window of the wave before; wave 0 reads the seam row, or, without one, its own window: only the bands that
    // have no neighbour run there and they drop what they read).  rd: the same entries of the column differences (order 0).
    const bool out_seam = a.seam && wave == NB - 1, in_seam = a.seam && wave == 0;
    double *outb = out_seam ? lds : mine;
    const double *inb = in_seam ? lds : (wave == 0 ? mine : mine - a.wave_doubles);
    double *outrd = outb + (out_seam ? Q + 2 : kWin);
    const double *inrd = inb + (in_seam ? Q + 2 : kWin);
    const int outmask = out_seam ? 0x7fffffff : kWin - 1, inmask = in_seam ? 0x7fffffff : kWin - 1;
    const IO *GO = static_cast<const IO *>(a.grad_out);

    // the band (in sweep order) this wave runs in kernel phase t and the band's phase c; false: the wave idles
    auto sched = [&](int t, int &bi, int &c) {
        int k = t / a.stride;
        c = t - k * a.stride - kLag * wave;
        if (c < 0) {
            --k;
            c += a.stride;
        }
        bi = k * NB + wave;
        return k >= 0 && c < a.nph && bi < a.nbands;
    };

    for (int item = blockIdx.x; item < a.A; item += gridDim.x) {
        const int i = item;
        const IO *xi = static_cast<const IO *>(a.X) + (size_t)i * M * d;
        const IO *yj = static_cast<const IO *>(a.Y) + (size_t)i * N * d;
        RingWave rw;
        rw.N = N; rw.n = n; rw.r = a.r; rw.P = P; rw.Q = Q; rw.W = W; rw.nbands = a.nbands; rw.nsteps = nsteps;
        rw.inv_r2 = a.inv_r2;
        rw.ring = ring; rw.rowbuf = nullptr; rw.dump = dump;
        const size_t area = (size_t)a.nbands * nsteps * kWave;
        rw.wsk = GRAD ? a.wsk + (size_t)blockIdx.x * a.wsk_per_block : nullptr;
        rw.wss = GRAD ? rw.wsk + area : nullptr;
        rw.spare = GRAD ? rw.wss + area + lane : nullptr;

        auto stage_x = [&](int a0) {
            for (int e = lane; e < (nrow + 1) * d; e += kWave) {
                const int k = e / d;
                xs[e] = (double)xi[(size_t)min(a0 + k, M - 1) * d + (e - k * d)];
            }
        };
        // the static kernel of a staged point of X_i and column `col` of Y_i (the serial fill's evaluation)
        auto kval = [&](const double *x, int col) {
            const IO *yb = yj + (size_t)min(max(col, 0), N - 1) * d;
            if (d <= 16) {
                double yv[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) yv[c] = c < d ? (double)yb[c] : 0.0;
                return static_k16<KIND>(x, yv, d, a.inv_h);
            }
            return static_k<KIND>(x, yb, d, a.inv_h);
        };
        // gram_long_kernel's fill into this wave's ring (orders >= 1), between wave-level fences instead of barriers
        auto fill = [&](int a0, int b_lo, int b_hi) {
            wave_lds_fence();
            for (int b0 = b_lo; b0 <= b_hi; b0 += kWave - 1) {
                const int b = b0 + lane;
                const bool ok = lane < kWave - 1 && b <= b_hi;
                const IO *yb = yj + (size_t)min(b, N - 1) * d;
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
            wave_lds_fence();
        };

        // ---- forward sweep ---------------------------------------------------------------------------------------------
        {
            double cur = 1.0, upprev = 1.0, rb = 1.0, rd_last = 0.0;
            int have = -1;
            for (int t = 0; t < a.phases; ++t) {
                int kb, c;
                if (sched(t, kb, c)) {
                    const int p = kb * kWave + lane;
                    const bool rowvalid = p < P, first = kb == 0;
                    const int a0 = (kb * kWave) >> n;
                    const int s0 = c * kPH;
                    if (c == 0) {
                        wave_lds_fence(); // (the gradient pass / the band before is done with xs)
                        stage_x(a0);
                        wave_lds_fence();
                        cur = 1.0;
                        upprev = 1.0;
                        rd_last = 0.0;
                        have = -1;
                        const double rb1 = inb[1 & inmask];
                        rb = first ? 1.0 : rb1; // lane 0's upper neighbour on step s: entry s + 1
                    }
                    double D[kPH];
                    if (reg) {
                        const int q0 = s0 - lane;
                        const double *xlo = xs + (size_t)(lane + 1) * d;
                        double gprev = kval(xlo, q0), g0prev = first ? kval(xs, q0) : 0.0, rprev = rd_last;
#pragma unroll
                        for (int u = 0; u < kPH; ++u) {
                            const double gn = kval(xlo, q0 + u + 1);
                            const double rd = gn - gprev; // k(x_{p+1}, y_{q+1}) - k(x_{p+1}, y_q), q = q0 + u
                            gprev = gn;
                            double up = shfl_up_f64(rprev); // the same difference at x_p: the lane above, one step ago
                            if (first) {
                                const double g0n = kval(xs, q0 + u + 1);
                                up = lane == 0 ? g0n - g0prev : up;
                                g0prev = g0n;
                            } else {
                                const double rin = inrd[min(s0 + u + 1, Q + 1) & inmask];
                                up = lane == 0 ? rin : up;
                            }
                            D[u] = rd - up;
                            const int q = q0 + u;
                            *((lane == kWave - 1 && rowvalid && q >= 0 && q < Q) ? outrd + ((q + 1) & outmask) : dump + lane) = rd;
                            rprev = rd;
                        }
                        rd_last = rprev;
                    } else {
                        if ((c & 3) == 0 && s0 < nsteps) { // a block of 64 steps starts: the serial kernel's refill rule
                            const int lo = max(s0 - (kWave - 1), 0) >> n, hi = min((s0 + kWave - 1) >> n, N - 2);
                            if (hi > have) {
                                const int to = min(N - 2, lo + W - 1);
                                fill(a0, have + 1, to);
                                have = to;
                            }
                        }
                        const double *Drow = ring + (size_t)((min(p, P - 1) >> n) - a0) * W;
#pragma unroll
                        for (int u = 0; u < kPH; ++u) D[u] = Drow[(min(max(s0 + u - lane, 0), Q - 1) >> n) & (W - 1)];
                    }
                    float *wp = GRAD ? rw.wsk + (size_t)kb * nsteps * kWave + lane : nullptr;
#pragma unroll
                    for (int u = 0; u < kPH; ++u) {
                        const int s = s0 + u, q = s - lane;
                        const bool active = rowvalid && q >= 0 && q < Q;
                        const double rbr = inb[min(s + 2, Q) & inmask];
                        const double rbn = first ? 1.0 : rbr;
                        double up_in = shfl_up_f64(cur);
                        up_in = (lane == 0) ? rb : up_in;
                        const double nw = stencil(cur, up_in, upprev, D[u] * a.inv_r2, NAIVE);
                        if (GRAD && s < nsteps) { // K_fwd[p][q] at [step][lane]
                            const float kst = (float)upprev;
                            asm volatile("global_store_dword %0, %1, off" ::"v"(wp + (size_t)s * kWave), "v"(kst));
                        }
                        *((lane == kWave - 1 && active) ? outb + ((q + 1) & outmask) : dump + lane) = nw;
                        cur = active ? nw : cur;
                        upprev = active ? up_in : upprev;
                        rb = rbn;
                    }
                    if (c == a.nph - 1 && p == P - 1) static_cast<IO *>(a.K_out)[i] = (IO)cur;
                }
                __syncthreads();
            }
        }
        if (!GRAD) continue; // (the phase loop's last barrier separates the pairs)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the forward solution is in L2 before it is read back
        __syncthreads();

        // ---- reverse sweep: the bands in descending order --------------------------------------------------------------
        {
            double cur = 1.0, dprev = 1.0, sb = 0.0, rb = 1.0, rd_last = 0.0;
            int low = N - 1;
            for (int t = 0; t < a.phases; ++t) {
                int bi, c;
                if (sched(t, bi, c)) {
                    const int kb = a.nbands - 1 - bi;
                    const int p = kb * kWave + lane;
                    const bool rowvalid = p < P, lastband = bi == 0;
                    const int L = min(kWave, P - kb * kWave);
                    const int a0 = (kb * kWave) >> n;
                    const int sp0 = c * kPH;
                    const bool hands_over = lane == 0 && kb > 0;
                    if (c == 0) {
                        wave_lds_fence();
                        stage_x(a0);
                        wave_lds_fence();
                        cur = 1.0;
                        dprev = 1.0;
                        sb = 0.0;
                        rd_last = 0.0;
                        low = N - 1;
                        const double rb0 = inb[0];
                        rb = lastband ? 1.0 : rb0; // lane L-1's lower neighbour on step sp: entry sp (from the right edge)
                    }
                    const int qtop = Q - 1 + (L - 1 - lane); // the lane's column on step 0
                    double D[kPH];
                    if (reg) {
                        const int q0 = qtop - sp0;
                        const double *xup = xs + (size_t)lane * d, *xlo = xs + (size_t)(lane + 1) * d;
                        double gprev = kval(xup, q0 + 1), g1prev = lastband ? kval(xlo, q0 + 1) : 0.0, rprev = rd_last;
#pragma unroll
                        for (int u = 0; u < kPH; ++u) {
                            const int q = q0 - u;
                            const double gn = kval(xup, q);
                            const double rd = gprev - gn; // k(x_p, y_{q+1}) - k(x_p, y_q)
                            gprev = gn;
                            double lo = shfl_down_f64(rprev); // the same difference at x_{p+1}: the lane below, one step ago
                            if (lastband) {
                                const double g1n = kval(xlo, q);
                                lo = lane == L - 1 ? g1prev - g1n : lo;
                                g1prev = g1n;
                            } else {
                                const double rin = inrd[min(sp0 + u, Q + 1) & inmask];
                                lo = lane == L - 1 ? rin : lo;
                            }
                            D[u] = lo - rd;
                            *((hands_over && q >= 0 && q < Q) ? outrd + ((Q - 1 - q) & outmask) : dump + lane) = rd;
                            rprev = rd;
                        }
                        rd_last = rprev;
                    } else {
                        const int nsp = Q + L - 1;
                        if ((c & 3) == 0 && sp0 < nsp) { // a block of 64 steps starts: the serial kernel's refill rule
                            const int qhi = Q + L - 2 - sp0;
                            const int need_hi = min(qhi, Q - 1) >> n, need_lo = max(qhi - 2 * (kWave - 1), 0) >> n;
                            if (need_lo < low) {
                                const int from = max(0, need_hi - W + 1);
                                fill(a0, from, low - 1);
                                low = from;
                            }
                        }
                        const double *Drow = ring + (size_t)((min(p, P - 1) >> n) - a0) * W;
#pragma unroll
                        for (int u = 0; u < kPH; ++u) D[u] = Drow[(min(max(qtop - sp0 - u, 0), Q - 1) >> n) & (W - 1)];
                    }
                    float *wsrow = rw.wss + (size_t)kb * nsteps * kWave + lane;
                    const float *wrow = rw.wsk + (size_t)kb * nsteps * kWave + lane; // K_fwd[p][q] at step lane + q
                    const int R0 = Q - 1 + L - 1 - sp0; // row of the stored forward solution on the phase's first step
                    float kfv[kPH];
#pragma unroll
                    for (int u = 0; u < kPH; ++u) kfv[u] = wrow[(size_t)max(R0 - u, 0) * kWave];
#pragma unroll
                    for (int u = 0; u < kPH; ++u) {
                        const int sp = sp0 + u, q = qtop - sp, R = R0 - u;
                        const bool active = rowvalid && q >= 0 && q < Q;
                        const double rbr = inb[min(sp + 1, Q - 1) & inmask];
                        const double rbn = lastband ? 1.0 : rbr;
                        const double kf = (double)kfv[u];
                        double down_in = shfl_down_f64(cur);
                        down_in = (lane == L - 1) ? rb : down_in;
                        sb = active ? __builtin_fma(kf, dprev, sb) : sb;
                        const bool done = active && (q & (a.r - 1)) == 0; // the block's last (lowest) column
                        const float sst = done ? (float)(sb * a.inv_r2) : 0.f;
                        asm volatile("global_store_dword %0, %1, off" ::"v"(R >= 0 ? wsrow + (size_t)R * kWave : rw.spare), "v"(sst));
                        sb = done ? 0.0 : sb;
                        const double nw = stencil(cur, down_in, dprev, D[u] * a.inv_r2, NAIVE);
                        *((hands_over && active) ? outb + ((Q - 1 - q) & outmask) : dump + lane) = nw;
                        cur = active ? nw : cur;
                        dprev = active ? down_in : dprev;
                        rb = rbn;
                    }
                }
                __syncthreads();
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // S is in L2 before it is read back
        __syncthreads();

        // ---- gradient: the serial kernel's passes, their outer loops dealt to the waves --------------------------------
        const double w = GO ? (double)GO[i] : 1.0;
        IO *gX = static_cast<IO *>(a.gradX), *gY = static_cast<IO *>(a.gradY);
        if (gX)
            static_grad_pass_rr<KIND, true>(rw, xi, M, yj, N, d, a.inv_h, lane, wave, NB, [&](int m, int c, double g) {
                gX[((size_t)i * M + m) * d + c] = (IO)(w * g);
            });
        if (gY)
            static_grad_pass_rr<KIND, false>(rw, yj, N, xi, M, d, a.inv_h, lane, wave, NB, [&](int nn, int c, double g) {
                gY[((size_t)i * N + nn) * d + c] = (IO)(w * g);
            });
        __syncthreads(); // (the next pair's forward sweep overwrites the scratch)
    }
}

namespace {
template <typename IO, bool NAIVE, bool GRAD, int KIND>
hipError_t bands_launch_one(const PairBandsPlan &bp, hipStream_t stream, const BandsArgs &a)
{
    constexpr auto kernel = &pair_bands_kernel<IO, NAIVE, GRAD, KIND>;
    const hipError_t e = raise_lds_limit<kernel>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(bp.grid), dim3(bp.NB * kWave), bp.lds, stream, a);
    return hipSuccess;
}
template <typename IO, int KIND>
hipError_t bands_launch_solver(bool naive, bool grad, const PairBandsPlan &bp, hipStream_t stream, const BandsArgs &a)
{
    // (IMQ, rational quadratic and Matern have the default stencil only, as in the serial kernel)
    constexpr bool has_naive = KIND == SIGSVGD_STATIC_RBF || KIND == SIGSVGD_STATIC_LINEAR;
    if constexpr (has_naive) {
        if (naive)
            return grad ? bands_launch_one<IO, true, true, KIND>(bp, stream, a)
                        : bands_launch_one<IO, true, false, KIND>(bp, stream, a);
    } else {
        if (naive) return hipErrorInvalidValue;
    }
    return grad ? bands_launch_one<IO, false, true, KIND>(bp, stream, a)
                : bands_launch_one<IO, false, false, KIND>(bp, stream, a);
}
template <typename IO>
hipError_t bands_launch_kind(int kind, bool naive, bool grad, const PairBandsPlan &bp, hipStream_t stream, const BandsArgs &a)
{
    if (kind == SIGSVGD_STATIC_IMQ) return bands_launch_solver<IO, SIGSVGD_STATIC_IMQ>(naive, grad, bp, stream, a);
    if (kind == SIGSVGD_STATIC_RQ) return bands_launch_solver<IO, SIGSVGD_STATIC_RQ>(naive, grad, bp, stream, a);
    if (kind != SIGSVGD_STATIC_RBF) return bands_launch_solver<IO, SIGSVGD_STATIC_LINEAR>(naive, grad, bp, stream, a);
    return bands_launch_solver<IO, SIGSVGD_STATIC_RBF>(naive, grad, bp, stream, a);
}
} // namespace

// pair_bands_f32.hip: the fp32-I/O instantiations, side by side with the fp64-I/O ones of pair_bands.hip (half the build time)
hipError_t pair_bands_launch_f32(int kind, bool naive, bool grad, const PairBandsPlan &bp, hipStream_t stream, const BandsArgs &a);
// pair_bands_matern.hip: the Matern kinds' instantiations (both I/O types, default stencil only)
hipError_t pair_bands_launch_matern(int dtype, int kind, bool grad, const PairBandsPlan &bp, hipStream_t stream,
                                    const BandsArgs &a);

} // namespace sigsvgd
