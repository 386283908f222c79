// The exact-adjoint instantiations of the long-path gradient kernels for the Matern-3/2 and -5/2 kinds (gram_long_kernels.h;
// DESIGN.md section 5.19): long_exact_matern_launch, which gram_long_exact.hip's long_exact_launch calls.
#include "gram_long_kernels.h"

namespace sigsvgd {

hipError_t long_exact_matern_launch(int family, int dtype, int kind, int grid, size_t lds, hipStream_t stream,
                                    const void *args)
{
    return exact_launch_any<SIGSVGD_STATIC_MATERN32, SIGSVGD_STATIC_MATERN52>(family, dtype, kind, grid, lds, stream, args);
}

} // namespace sigsvgd
