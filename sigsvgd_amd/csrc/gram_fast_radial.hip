// The inverse-multiquadric and rational-quadratic instantiations of the register-resident kernel (gram_fast_kernel.h, RADIAL = 1;
// DESIGN.md section 5.18), a translation unit of their own so that they build beside the RBF ones of gram_fast.hip, whose
// `run` sends the launches of these kinds here.
#include "gram_fast_kernel.h"

namespace sigsvgd {

int fast_radial_dispatch(const GramProblem &p, FastArgs &a, const WsPlan &w, bool grad, bool sym, int &tile_rows)
{
    return dispatch_variant<1>(p, a, w, grad, sym, tile_rows);
}

} // namespace sigsvgd

SIG_EXEC_DEBUG_GETTER(fast_radial)
