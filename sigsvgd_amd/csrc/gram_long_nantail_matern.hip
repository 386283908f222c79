// The NaN-marked-tail instantiations of the long-path kernels for the Matern-3/2 and -5/2 kinds (gram_long_kernels.h; DESIGN.md
// section 5.20): long_nan_tail_matern_launch, which gram_long_nantail.hip's long_nan_tail_launch calls.
#include "gram_long_kernels.h"

namespace sigsvgd {

hipError_t long_nan_tail_matern_launch(int family, int dtype, int kind, bool naive, bool grad, int grid, size_t lds,
                                       hipStream_t stream, const void *args)
{
    return nan_tail_launch_any<SIGSVGD_STATIC_MATERN32, SIGSVGD_STATIC_MATERN52>(family, dtype, kind, naive, grad, grid, lds,
                                                                                 stream, args);
}

} // namespace sigsvgd
