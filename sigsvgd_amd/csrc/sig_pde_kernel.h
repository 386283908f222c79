// sig_pde_kernel (sig_pde.hip has the description, the plan and the launcher) and its arguments.  Included by sig_pde.hip and by
// sig_pde_exact.hip (the exact adjoint's instantiations).
#pragma once

#include "ring_sweep.h"

namespace sigsvgd {

struct PdeArgs {
    const void *G, *grad_out;
    void *K_out, *dG_out;
    float *wsk;           // [grid][wsk_per_block]: forward solution, then S partials (+ one spare row)
    size_t wsk_per_block; // floats
    int npairs, M, N, n, r, P, Q, nbands, nsteps, nrow, W;
    double inv_r2;
};

// IOX: float, double, or ExactIO<float>, ExactIO<double> (ring_sweep.h): the sweeps of the exact adjoint
// (default stencil, gradient launches), the assembly of dG from S being the same code.  Instantiated in sig_pde_exact.hip.
template <typename IOX, bool NAIVE, bool GRAD>
__global__ __launch_bounds__(64) void sig_pde_kernel(PdeArgs a)
{
    using IO = typename RingIO<IOX>::type;
    constexpr bool EXACT = RingIO<IOX>::exact;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int lane = threadIdx.x;
    const int M = a.M, N = a.N, W = a.W, nrow = a.nrow;
    const RingWave rw = ring_wave<GRAD>(a, smem_raw);
    double *ring = rw.ring;
    const IO *GO = static_cast<const IO *>(a.grad_out);
    const auto no_band = [](int) {};

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

        const double Kval = ring_forward<NAIVE, GRAD, EXACT>(rw, fill, no_band);
        if (((rw.P - 1) & (kWave - 1)) == lane) static_cast<IO *>(a.K_out)[pair] = (IO)Kval;
        if (!GRAD) continue;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the forward solution is in L2 before it is read back
        __syncthreads();
        ring_reverse<NAIVE, EXACT>(rw, fill, no_band);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // S is in L2 before the assembly reads it
        __syncthreads();

        // ---- assembly: dG = grad_out * 4-corner scatter of S ------------------------------------------------------------
        const int Mm = M - 1, Nm = N - 1;
        const double w = GO ? (double)GO[pair] : 1.0;
        IO *dG = static_cast<IO *>(a.dG_out) + (size_t)pair * M * N;
        for (int e = lane; e < M * N; e += kWave) {
            const int m = e / N, nn = e - m * N;
            double Rv = 0.0;
            if (m >= 1 && nn >= 1) Rv += ring_S(rw, m - 1, nn - 1);
            if (m < Mm && nn < Nm) Rv += ring_S(rw, m, nn);
            if (m >= 1 && nn < Nm) Rv -= ring_S(rw, m - 1, nn);
            if (m < Mm && nn >= 1) Rv -= ring_S(rw, m, nn - 1);
            dG[e] = (IO)(w * Rv);
        }
        __syncthreads(); // (the next pair's forward sweep overwrites the scratch and the ring)
    }
}

// sig_pde_exact.hip: the launch of sig_pde_exact_kernel at the plan's grid and LDS bytes; sig_pde.hip's pde_launch calls it
hipError_t pde_exact_launch(int dtype, int grid, size_t lds, hipStream_t stream, const PdeArgs &a);

} // namespace sigsvgd
