// Plan and launch of the band-parallel paired solver (pair_bands.h), and the fp64-I/O instantiations
// of pair_bands_kernel (pair_bands_kernel.h); the fp32-I/O and the Matern ones are pair_bands_f32.hip's and
// pair_bands_matern.hip's.
#include "pair_bands_kernel.h"

namespace sigsvgd {

// ---- plan and launch ----------------------------------------------------------------------------------------------------------
void pair_bands_plan(int A, int M, int N, int d, int n, const PairGeom &g, PairBandsPlan &bp)
{
    (void)M;
    bp = PairBandsPlan{};
    bp.NB = 1;
    if (g.nbands < 2) return; // paths of one band stay serial
    int W = 0;
    if (n > 0) { // the columns a block of 64 steps can touch, as a power of two, and no more than the grid has
        W = 2;
        while (W < (126 >> n) + 2) W <<= 1;
        int Wn = 1;
        while (Wn < N - 1) Wn <<= 1;
        W = W < Wn ? W : Wn;
    }
    const int rows = n == 0 ? 2 : 1; // boundary values, and at order 0 the column differences beside them
    const size_t wave_doubles = (size_t)rows * kWin + kWave + (size_t)(g.nrow + 1) * d + (size_t)g.nrow * W;
    const int nph = (g.nsteps + kPH - 1) / kPH;
    const size_t max_lds = 160 * 1024;
    int NB = g.nbands < kMaxNB ? g.nbands : kMaxNB;
    size_t seam_doubles = 0, lds = 0;
    for (; NB >= 2; --NB) {
        seam_doubles = g.nbands > NB ? (size_t)rows * (g.Q + 2) : 0;
        lds = (seam_doubles + NB * wave_doubles) * sizeof(double);
        if (lds <= max_lds) break;
    }
    if (NB < 2) return; // LDS admits no second wave
    bp.NB = NB;
    bp.W = W;
    bp.nph = nph;
    bp.stride = nph + kLag > kLag * NB ? nph + kLag : kLag * NB;
    const int last = g.nbands - 1;
    bp.phases = (last / NB) * bp.stride + kLag * (last % NB) + nph;
    bp.seam = g.nbands > NB ? 1 : 0;
    bp.seam_doubles = seam_doubles;
    bp.wave_doubles = wave_doubles;
    bp.lds = lds;
    int per_cu = (int)(max_lds / lds);
    const int by_waves = 8 / NB; // 2 wavefronts per SIMD at the kernel's 174 - 221 VGPRs: 8 per CU, as ring_make_plan counts
    per_cu = per_cu < by_waves ? per_cu : by_waves;
    bp.resident = (long long)device_cu_count() * (per_cu < 1 ? 1 : per_cu);
    long long grid = bp.resident < A ? bp.resident : A;
    if (grid > g.serial_grid) grid = g.serial_grid; // the scratch slots of the (possibly lowered) serial plan
    bp.grid = (int)grid;
}

int pair_bands_launch(const LongProblem &p, const PairGeom &g, const PairBandsPlan &bp, float *wsk)
{
    const bool grad = p.gradX_out != nullptr || p.gradY_out != nullptr;
    BandsArgs a;
    a.X = p.X; a.Y = p.Y; a.grad_out = p.grad_out; a.K_out = p.K_out; a.gradX = p.gradX_out; a.gradY = p.gradY_out;
    a.wsk = wsk; a.wsk_per_block = g.wsk_per_block;
    a.A = p.A; a.M = p.TX; a.N = p.TY; a.d = p.d; a.n = p.n; a.r = g.r; a.P = g.P; a.Q = g.Q; a.nbands = g.nbands;
    a.nsteps = g.nsteps; a.nrow = g.nrow; a.W = bp.W; a.NB = bp.NB; a.nph = bp.nph; a.stride = bp.stride;
    a.phases = bp.phases; a.seam = bp.seam;
    a.wave_doubles = (unsigned)bp.wave_doubles; a.seam_doubles = (unsigned)bp.seam_doubles;
    a.inv_h = p.inv_h; a.inv_r2 = 1.0 / ((double)g.r * (double)g.r);
    const bool naive = (p.flags & SIGSVGD_FLAG_NAIVE_SOLVER) != 0;
    const bool matern = p.kind == SIGSVGD_STATIC_MATERN32 || p.kind == SIGSVGD_STATIC_MATERN52;
    hipError_t e = matern ? (naive ? hipErrorInvalidValue // (the entry points refuse it before this)
                                   : pair_bands_launch_matern(p.dtype, p.kind, grad, bp, p.stream, a))
                   : p.dtype == SIGSVGD_F64 ? bands_launch_kind<double>(p.kind, naive, grad, bp, p.stream, a)
                                            : pair_bands_launch_f32(p.kind, naive, grad, bp, p.stream, a);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(pair_bands)");
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch pair_bands_kernel");
    return SIGSVGD_OK;
}

} // namespace sigsvgd
