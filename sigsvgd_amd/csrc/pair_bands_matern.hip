// The Matern-3/2 and -5/2 instantiations of pair_bands_kernel (pair_bands_kernel.h), both I/O types, a
// translation unit of their own so that they build beside the other kinds'; pair_bands.hip's pair_bands_launch calls this.
#include "pair_bands_kernel.h"

namespace sigsvgd {

hipError_t pair_bands_launch_matern(int dtype, int kind, bool grad, const PairBandsPlan &bp, hipStream_t stream,
                                    const BandsArgs &a)
{
    if (kind != SIGSVGD_STATIC_MATERN32 && kind != SIGSVGD_STATIC_MATERN52) return hipErrorInvalidValue;
    if (dtype == SIGSVGD_F64)
        return kind == SIGSVGD_STATIC_MATERN32 ? bands_launch_solver<double, SIGSVGD_STATIC_MATERN32>(false, grad, bp, stream, a)
                                               : bands_launch_solver<double, SIGSVGD_STATIC_MATERN52>(false, grad, bp, stream, a);
    return kind == SIGSVGD_STATIC_MATERN32 ? bands_launch_solver<float, SIGSVGD_STATIC_MATERN32>(false, grad, bp, stream, a)
                                           : bands_launch_solver<float, SIGSVGD_STATIC_MATERN52>(false, grad, bp, stream, a);
}

} // namespace sigsvgd
