// The normalised kernel's instantiations of the long-path kernels (gram_long_kernels.h) for the RBF,
// linear, IMQ and rational-quadratic kinds, a translation unit of their own as the log-domain ones are: long_norm_launch, which
// gram_long.hip's family_launch calls for launches with SIGSVGD_FLAG_NORMALIZED, and the two small kernels behind such a launch:
// the row and column sums of the pairs' weights w K^ and the slab reduction that adds the diagonals' terms.
#include "gram_long_kernels.h"

namespace sigsvgd {

// sums[r] = sum over c of U[r][c] for the A rows r of the pairs' weights U [A][B] (norm_weights: w K^ as the two-sided kernel
// formed them, fp64, SYM and Y_IS_X applied, 0 on the diagonal of a Y_IS_X launch) -- blocks 0 .. A - 1, where rowsum is given --
// then the same down the B columns (the blocks behind them, where colsum is given).  One wavefront per sum: lane l adds its
// entries l, l + 64, .. in order, wave_sum_f64 adds the lanes; no atomics, the bits depend on the inputs alone.
__global__ __launch_bounds__(64) void long_norm_sums_kernel(const double *U, int A, int B, double *rowsum, double *colsum,
                                                            int nrowblocks)
{
    const bool col = (int)blockIdx.x >= nrowblocks;
    const int r = col ? (int)blockIdx.x - nrowblocks : (int)blockIdx.x, n = col ? A : B;
    double acc = 0.0;
    for (int c = threadIdx.x; c < n; c += kWave) acc += U[col ? (size_t)c * B + r : (size_t)r * B + c];
    acc = wave_sum_f64(acc);
    if (threadIdx.x == 0) (col ? colsum : rowsum)[r] = acc;
}

// long2_reduce_kernel (gram_long.hip) with the diagonal's term: out[k][e] = sum over slab c of partials[k][c][e] in order
// (skip as there), then - sums[k] / 2 times diag[k][e] in one fma, and the one rounding to the I/O type.
template <typename IO>
__global__ void long_norm_reduce_kernel(const double *partials, IO *out, int rows, int nslabs, int TD, int skip,
                                        const double *sums, const double *diag)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)rows * TD) return;
    const size_t k = idx / TD, e = idx % TD;
    const int none = skip > 0 && k % skip == 0 ? (int)(k / skip) : -1;
    double s = 0.0;
    for (int c = 0; c < nslabs; ++c)
        if (c != none) s += partials[(k * nslabs + c) * TD + e];
    out[idx] = (IO)__builtin_fma(-0.5 * sums[k], diag[idx], s);
}

hipError_t long_norm_sums(const double *U, int A, int B, double *rowsum, double *colsum, hipStream_t stream)
{
    const int nrb = rowsum ? A : 0, grid = nrb + (colsum ? B : 0);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(long_norm_sums_kernel, dim3(grid), dim3(kWave), 0, stream, U, A, B, rowsum, colsum, nrb);
    return hipGetLastError();
}

hipError_t long_norm_reduce(int dtype, const double *partials, void *out, int rows, int nslabs, int TD, int skip,
                            const double *sums, const double *diag, hipStream_t stream)
{
    const int bs = 256;
    const unsigned gs = (unsigned)(((size_t)rows * TD + bs - 1) / bs);
    if (dtype == SIGSVGD_F64)
        hipLaunchKernelGGL(long_norm_reduce_kernel<double>, dim3(gs), dim3(bs), 0, stream, partials, static_cast<double *>(out),
                           rows, nslabs, TD, skip, sums, diag);
    else
        hipLaunchKernelGGL(long_norm_reduce_kernel<float>, dim3(gs), dim3(bs), 0, stream, partials, static_cast<float *>(out),
                           rows, nslabs, TD, skip, sums, diag);
    return hipGetLastError();
}

hipError_t long_norm_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                            const void *args)
{
    if (kind == SIGSVGD_STATIC_MATERN32 || kind == SIGSVGD_STATIC_MATERN52)
        return long_norm_matern_launch(family, dtype, kind, grad, grid, lds, stream, args);
    return norm_launch_any<SIGSVGD_STATIC_RBF, SIGSVGD_STATIC_LINEAR, SIGSVGD_STATIC_IMQ, SIGSVGD_STATIC_RQ>(
        family, dtype, kind, grad, grid, lds, stream, args);
}

} // namespace sigsvgd
