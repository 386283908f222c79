// The fp32-I/O instantiations of pair_bands_kernel (pair_bands_kernel.h), a translation unit of their own so that they build
// beside the fp64-I/O ones of pair_bands.hip, whose pair_bands_launch calls this.
#include "pair_bands_kernel.h"

namespace sigsvgd {

hipError_t pair_bands_launch_f32(int kind, bool naive, bool grad, const PairBandsPlan &bp, hipStream_t stream, const BandsArgs &a)
{
    return bands_launch_kind<float>(kind, naive, grad, bp, stream, a);
}

} // namespace sigsvgd
