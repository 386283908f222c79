// The normalised kernel's instantiations of the long-path kernels for the Matern-3/2 and -5/2 kinds (gram_long_kernels.h;
// DESIGN.md section 5.22): long_norm_matern_launch, which gram_long_norm.hip's long_norm_launch calls.
#include "gram_long_kernels.h"

namespace sigsvgd {

hipError_t long_norm_matern_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                                   const void *args)
{
    return norm_launch_any<SIGSVGD_STATIC_MATERN32, SIGSVGD_STATIC_MATERN52>(family, dtype, kind, grad, grid, lds, stream, args);
}

} // namespace sigsvgd
