// The exact-adjoint instantiations of sig_pde_kernel (sig_pde_kernel.h), a translation unit of their
// own: pde_exact_launch, which sig_pde.hip's pde_launch calls for gradient launches with SIGSVGD_FLAG_EXACT_ADJOINT.
#include "sig_pde_kernel.h"

namespace sigsvgd {

namespace {
struct PdeExactPlan {
    int grid;
    size_t lds;
};
struct PdeExactFamily {
    using Args = PdeArgs;
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &sig_pde_kernel<ExactIO<IO>, false, true>; }
};
} // namespace

hipError_t pde_exact_launch(int dtype, int grid, size_t lds, hipStream_t stream, const PdeArgs &a)
{
    const PdeExactPlan pl{grid, lds};
    return dtype == SIGSVGD_F64 ? ring_launch_one<PdeExactFamily, double, false, true, 0>(pl, stream, a)
                                : ring_launch_one<PdeExactFamily, float, false, true, 0>(pl, stream, a);
}

} // namespace sigsvgd
