// The NaN-marked-tail instantiations of the long-path kernels (gram_long_kernels.h) for the RBF, linear,
// IMQ and rational-quadratic kinds, a translation unit of their own as the exact adjoint's are: long_nan_tail_launch, which
// gram_long.hip's family_launch calls for launches with SIGSVGD_FLAG_NAN_TAILS, and the length pass that goes before it.
#include "gram_long_kernels.h"

namespace sigsvgd {

// One wavefront per path: lens[path] = the index of the path's first point whose channel 0 is NaN, T where there is none.  The
// wave reads channel 0 of 64 points at a time and takes the lowest set bit of the ballot.  A path that starts with NaN (the
// caller's error) gets 1, so every length is in [1, T].  X's nX paths first, then Y's nY.
template <typename IO>
__global__ __launch_bounds__(256) void nan_tail_length_kernel(const IO *X, int nX, int TX, const IO *Y, int nY, int TY, int d,
                                                              int *lens)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int path = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (path >= nX + nY) return; // (the whole wave)
    const bool isx = path < nX;
    const int T = isx ? TX : TY;
    const IO *p = isx ? X + (size_t)path * TX * d : Y + (size_t)(path - nX) * TY * d;
    int L = T;
    for (int t0 = 0; t0 < T; t0 += kWave) {
        const int t = t0 + lane;
        const bool nan = t < T && p[(size_t)t * d] != p[(size_t)t * d];
        const unsigned long long m = __ballot(nan);
        if (m) {
            L = t0 + __ffsll((long long)m) - 1;
            break;
        }
    }
    if (lane == 0) lens[path] = L < 1 ? 1 : L;
}

hipError_t long_nan_tail_lengths(int dtype, const void *X, int nX, int TX, const void *Y, int nY, int TY, int d, int *lens,
                                 hipStream_t stream)
{
    const int waves = 256 / kWave;
    const unsigned gs = (unsigned)((nX + nY + waves - 1) / waves);
    if (dtype == SIGSVGD_F64)
        hipLaunchKernelGGL(nan_tail_length_kernel<double>, dim3(gs), dim3(256), 0, stream, static_cast<const double *>(X), nX, TX,
                           static_cast<const double *>(Y), nY, TY, d, lens);
    else
        hipLaunchKernelGGL(nan_tail_length_kernel<float>, dim3(gs), dim3(256), 0, stream, static_cast<const float *>(X), nX, TX,
                           static_cast<const float *>(Y), nY, TY, d, lens);
    return hipGetLastError();
}

hipError_t long_nan_tail_launch(int family, int dtype, int kind, bool naive, bool grad, int grid, size_t lds,
                                hipStream_t stream, const void *args)
{
    if (kind == SIGSVGD_STATIC_MATERN32 || kind == SIGSVGD_STATIC_MATERN52)
        return long_nan_tail_matern_launch(family, dtype, kind, naive, grad, grid, lds, stream, args);
    return nan_tail_launch_any<SIGSVGD_STATIC_RBF, SIGSVGD_STATIC_LINEAR, SIGSVGD_STATIC_IMQ, SIGSVGD_STATIC_RQ>(
        family, dtype, kind, naive, grad, grid, lds, stream, args);
}

} // namespace sigsvgd
