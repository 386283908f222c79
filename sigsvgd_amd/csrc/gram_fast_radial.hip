// The inverse-multiquadric and rational-quadratic instantiations of the register-resident kernel (gram_fast.hip, RADIAL = 1;
// DESIGN.md section 5.18), a translation unit of their own so that they build beside the RBF ones and gram_fast.hip, the longest
// compile of the build, does not grow.
#define SIGSVGD_GRAM_FAST_RADIAL
#include "gram_fast.hip"
