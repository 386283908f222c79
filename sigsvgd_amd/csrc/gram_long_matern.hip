// The Matern-3/2 and -5/2 instantiations of the long-path kernels (gram_long_kernels.h), a translation
// unit of their own so that they build beside the other kinds' and no source grows past the longest of the build:
// long_matern_launch, which gram_long.hip's family_launch calls.
#include "gram_long_kernels.h"

namespace sigsvgd {

namespace {
struct MaternPlan {
    int grid;
    size_t lds;
};
template <typename F, typename IO>
hipError_t matern_launch_io(int kind, bool grad, const MaternPlan &pl, hipStream_t stream, const typename F::Args &a)
{
    if constexpr (F::bandwidth)
        return kind == SIGSVGD_STATIC_MATERN32 ? ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_MATERN32>(pl, stream, a)
                                               : ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_MATERN52>(pl, stream, a);
    else
        return kind == SIGSVGD_STATIC_MATERN32 ? ring_launch_solver<F, IO, SIGSVGD_STATIC_MATERN32>(false, grad, pl, stream, a)
                                               : ring_launch_solver<F, IO, SIGSVGD_STATIC_MATERN52>(false, grad, pl, stream, a);
}
template <typename F>
hipError_t matern_launch_family(int dtype, int kind, bool grad, const MaternPlan &pl, hipStream_t stream, const void *args)
{
    const typename F::Args &a = *static_cast<const typename F::Args *>(args);
    return dtype == SIGSVGD_F64 ? matern_launch_io<F, double>(kind, grad, pl, stream, a)
                                : matern_launch_io<F, float>(kind, grad, pl, stream, a);
}
} // namespace
hipError_t long_matern_launch(int family, int dtype, int kind, bool grad, int grid, size_t lds, hipStream_t stream,
                              const void *args)
{
    if (kind != SIGSVGD_STATIC_MATERN32 && kind != SIGSVGD_STATIC_MATERN52) return hipErrorInvalidValue;
    const MaternPlan pl{grid, lds};
    switch (family) {
    case LongFamily<false>::id: return matern_launch_family<LongFamily<false>>(dtype, kind, grad, pl, stream, args);
    case LongFamily<true>::id: return matern_launch_family<LongFamily<true>>(dtype, kind, grad, pl, stream, args);
    case Long2Family::id: return matern_launch_family<Long2Family>(dtype, kind, grad, pl, stream, args);
    case PairHFamily::id: return matern_launch_family<PairHFamily>(dtype, kind, grad, pl, stream, args);
    case Long2HFamily::id: return matern_launch_family<Long2HFamily>(dtype, kind, grad, pl, stream, args);
    case PartFamily::id: return matern_launch_family<PartFamily>(dtype, kind, grad, pl, stream, args);
    }
    return hipErrorInvalidValue;
}

} // namespace sigsvgd
