// The log-domain instantiations of the long-path kernels (gram_long_kernels.h) for the RBF, linear, IMQ
// and rational-quadratic kinds, a translation unit of their own as the exact adjoint's and the NaN-marked tails' are:
// long_log_k_launch, which gram_long.hip's family_launch calls for launches with SIGSVGD_FLAG_LOG_K.
#include "gram_long_kernels.h"

namespace sigsvgd {

hipError_t long_log_k_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                             const void *args)
{
    if (kind == SIGSVGD_STATIC_MATERN32 || kind == SIGSVGD_STATIC_MATERN52)
        return long_log_k_matern_launch(family, dtype, kind, grad, grid, lds, stream, args);
    return log_k_launch_any<SIGSVGD_STATIC_RBF, SIGSVGD_STATIC_LINEAR, SIGSVGD_STATIC_IMQ, SIGSVGD_STATIC_RQ>(
        family, dtype, kind, grad, grid, lds, stream, args);
}

} // namespace sigsvgd
