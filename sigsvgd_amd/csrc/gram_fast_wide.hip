// The 32-channel instantiations of the register-resident kernel (gram_fast_kernel.h, DPAD = 32): RBF paths
// of 17 to 32 channels with SIGSVGD_FLAG_FP32_SWEEPS, a translation unit of their own so that they build beside the ones of
// gram_fast.hip, whose `run` sends the launches with d > 16 here.  4-wave workgroups, one wave per SIMD (the 512-register budget),
// one workgroup per CU, the 64-slot ring with general windows at every length; d = 31 has the instantiations that drop the padded
// channel (the kernel's LP), every other d is zero-padded to 32 channels.
#include "gram_fast_kernel.h"

namespace sigsvgd {

int fast_wide_dispatch(const GramProblem &p, FastArgs &a, const WsPlan &w, bool grad, bool sym, int &tile_rows)
{
    return launch_variant<0, 32, 4>(p, a, w, grad, sym, tile_rows);
}

} // namespace sigsvgd

SIG_EXEC_DEBUG_GETTER(fast_wide)
