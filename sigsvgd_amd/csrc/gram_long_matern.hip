// The Matern-3/2 and -5/2 instantiations of the long-path kernels (gram_long.hip), a translation unit of
// their own so that they build beside the other kinds' and no source grows past the longest of the build.
#define SIGSVGD_GRAM_LONG_MATERN
#include "gram_long.hip"
