// The Matern-3/2 and -5/2 instantiations of pair_bands_kernel (pair_bands.hip), both I/O types, a
// translation unit of their own so that they build beside the other kinds'.
#define SIGSVGD_PAIR_BANDS_MATERN
#include "pair_bands.hip"
