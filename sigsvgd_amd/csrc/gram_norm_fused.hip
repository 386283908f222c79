// The two small kernels around the pair solve of a fused Gram launch with SIGSVGD_FLAG_NORMALIZED_FUSED (DESIGN.md section
// 5.23; the pipeline itself is capi.hip's gram_norm_fused): with a_i = ln K(X_i, X_i), b_j = ln K(Y_j, Y_j) from the diagonal
// pass (gram_long.hip's norm_diag_launch) and s_ij = exp(-(a_i + b_j) / 2) in fp64,
//   norm_fused_weights   W'[i][j] = (IO)(w_ij s_ij), the weights the unflagged launch then runs under, and
//   norm_fused_finish    K_out[i][j] *= s_ij in place, U_i = sum_j w_ij K^_ij, gradX_out[i] += -U_i / 2 grad a_i.
// Neither touches a pair kernel; both store through vector stores only and add in an order fixed by the shape.
#include "long_static.h"

namespace sigsvgd {

// the weight of pair (i, j): grad_out (NULL: ones), with SYM grad_out + grad_out^T (A == B)
template <typename IO>
__device__ __forceinline__ double norm_fused_w(const IO *go, int B, int i, int j, int sym)
{
    double w = go ? (double)go[(size_t)i * B + j] : 1.0;
    if (sym) w += go ? (double)go[(size_t)j * B + i] : 1.0;
    return w;
}

// W'[i][j] = (IO)(w_ij s_ij), one thread per entry; yx (Y_IS_X): the diagonal pair, whose K^ is the constant 1, gets 0.
// lnB is lnA where Y is X.  Always written whole, also where grad_out is NULL.
template <typename IO>
__global__ __launch_bounds__(256) void norm_fused_weights_kernel(const IO *go, const double *lnA, const double *lnB, IO *W,
                                                                 int A, int B, int sym, int yx)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)A * B) return;
    const int i = (int)(idx / B), j = (int)(idx % B);
    const double s = exp64(-0.5 * (lnA[i] + lnB[j]));
    W[idx] = yx && i == j ? (IO)0 : (IO)(norm_fused_w(go, B, i, j, sym) * s);
}

// One wavefront per row i.  K[i][j] (the unflagged launch's, I/O type) becomes K^_ij = K_ij s_ij, the product in fp64 and
// rounded once; yx: the diagonal is stored as exactly 1 (s_ij is symmetric in i and j there, so a bit-symmetric K stays so).
// Gradient launches (gradX given): lane l adds w_ij K^_ij (fp64, unrounded; yx: without the diagonal) over its columns
// l, l + 64, .. in order, wave_sum_f64 adds the lanes (no atomics: the bits depend on the inputs alone), sums[i] keeps U_i,
// and gradX[i][e] = (IO) fma(-U_i / 2, diag[i][e], (double)gradX[i][e]) over the row's TD entries, diag the fp64 gradient of a_i.
template <typename IO>
__global__ __launch_bounds__(64) void norm_fused_finish_kernel(IO *K, const IO *go, const double *lnA, const double *lnB, int A,
                                                               int B, int sym, int yx, IO *gradX, const double *diag,
                                                               double *sums, int TD)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= A) return;
    const double ai = lnA[i];
    double acc = 0.0;
    for (int j = lane; j < B; j += kWave) {
        const size_t idx = (size_t)i * B + j;
        const double kh = (double)K[idx] * exp64(-0.5 * (ai + lnB[j]));
        const bool dg = yx && i == j;
        K[idx] = dg ? (IO)1 : (IO)kh;
        if (gradX && !dg) acc += norm_fused_w(go, B, i, j, sym) * kh;
    }
    if (!gradX) return;
    acc = wave_sum_f64(acc);
    if (lane == 0) sums[i] = acc;
    const double h = -0.5 * acc;
    IO *g = gradX + (size_t)i * TD;
    const double *dgi = diag + (size_t)i * TD;
    for (int e = lane; e < TD; e += kWave) g[e] = (IO)__builtin_fma(h, dgi[e], (double)g[e]);
}

hipError_t norm_fused_weights(int dtype, const void *go, const double *lnA, const double *lnB, void *W, int A, int B, bool sym,
                              bool yx, hipStream_t stream)
{
    const int bs = 256;
    const unsigned gs = (unsigned)(((size_t)A * B + bs - 1) / bs);
    if (dtype == SIGSVGD_F64)
        hipLaunchKernelGGL(norm_fused_weights_kernel<double>, dim3(gs), dim3(bs), 0, stream, static_cast<const double *>(go), lnA,
                           lnB, static_cast<double *>(W), A, B, sym ? 1 : 0, yx ? 1 : 0);
    else
        hipLaunchKernelGGL(norm_fused_weights_kernel<float>, dim3(gs), dim3(bs), 0, stream, static_cast<const float *>(go), lnA,
                           lnB, static_cast<float *>(W), A, B, sym ? 1 : 0, yx ? 1 : 0);
    return hipGetLastError();
}

// gradX == NULL: a forward-only launch, the scaling alone (go, diag and sums are not read)
hipError_t norm_fused_finish(int dtype, void *K, const void *go, const double *lnA, const double *lnB, int A, int B, bool sym,
                             bool yx, void *gradX, const double *diag, double *sums, int TD, hipStream_t stream)
{
    if (dtype == SIGSVGD_F64)
        hipLaunchKernelGGL(norm_fused_finish_kernel<double>, dim3(A), dim3(kWave), 0, stream, static_cast<double *>(K),
                           static_cast<const double *>(go), lnA, lnB, A, B, sym ? 1 : 0, yx ? 1 : 0, static_cast<double *>(gradX),
                           diag, sums, TD);
    else
        hipLaunchKernelGGL(norm_fused_finish_kernel<float>, dim3(A), dim3(kWave), 0, stream, static_cast<float *>(K),
                           static_cast<const float *>(go), lnA, lnB, A, B, sym ? 1 : 0, yx ? 1 : 0, static_cast<float *>(gradX),
                           diag, sums, TD);
    return hipGetLastError();
}

} // namespace sigsvgd
