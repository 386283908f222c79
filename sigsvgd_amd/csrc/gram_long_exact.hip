// The exact-adjoint instantiations of the long-path gradient kernels (gram_long_kernels.h) for the RBF,
// linear, IMQ and rational-quadratic kinds, a translation unit of their own as the Matern kinds' are: long_exact_launch, which
// gram_long.hip's family_launch calls for launches with SIGSVGD_FLAG_EXACT_ADJOINT.
#include "gram_long_kernels.h"

namespace sigsvgd {

hipError_t long_exact_launch(int family, int dtype, int kind, int grid, size_t lds, hipStream_t stream, const void *args)
{
    if (kind == SIGSVGD_STATIC_MATERN32 || kind == SIGSVGD_STATIC_MATERN52)
        return long_exact_matern_launch(family, dtype, kind, grid, lds, stream, args);
    return exact_launch_any<SIGSVGD_STATIC_RBF, SIGSVGD_STATIC_LINEAR, SIGSVGD_STATIC_IMQ, SIGSVGD_STATIC_RQ>(
        family, dtype, kind, grid, lds, stream, args);
}

} // namespace sigsvgd
