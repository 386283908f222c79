// The fp32-I/O instantiations of pair_bands_kernel (pair_bands.hip), a translation unit of their own so that they build
// beside the fp64-I/O ones.
#define SIGSVGD_PAIR_BANDS_F32
#include "pair_bands.hip"
