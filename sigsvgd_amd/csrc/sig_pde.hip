// Signature PDE on a caller-supplied static-kernel grid (user static kernels).
//
// Input: npairs grids G[pair][M][N] (the static kernel k(x_a, y_b) of one pair of paths, evaluated by the caller), fp32 or
// fp64.  Forward: the 4-corner increments D[a][b] = (G[a+1][b+1] - G[a+1][b]) - (G[a][b+1] - G[a][b]) in fp64, refined to
// g[p][q] = D[p >> n][q >> n] / r^2 on the P x Q grid (r = 2^n, P = r (M-1), Q = r (N-1)), one Goursat sweep in fp64, and
// K[pair] = sol[P][Q].  Backward: the reference's convention (oracle/sigkernel_oracle.py gram_backward): GG[p][q] =
// K_fwd[p][q] K_rev[p+1][q+1], S[a][b] = r^-2 sum of GG over the block of (a, b), and dG[m][n] = grad_out (S[m-1][n-1] +
// S[m][n] - S[m-1][n] - S[m][n-1]) with S = 0 outside the grid.
//
// Layout: the ring sweep of ring_sweep.h (the long-path mode of gram_generic_kernel), its ring filled from G in global
// memory; the assembly reads S with ring_S.  The kernel is in sig_pde_kernel.h.  With SIGSVGD_FLAG_EXACT_ADJOINT (default
// stencil, gradient launches) S is the exact derivative of the discrete K in the increments.
#include "sig_pde_kernel.h"

namespace sigsvgd {

namespace {
struct PdePlan : RingPlan {
    int grid;
    size_t ws_bytes;
    size_t total() const { return ring_ws_total(ws_bytes); }
};

// (not gram_long.hip's long_set_grid: this scratch is sized for 8 waves per CU and does not shrink with the grid)
int pde_make_plan(int npairs, int M, int N, int n, int want_grad, PdePlan &pl)
{
    const int rc = ring_make_plan(M, N, n, want_grad, 0, "pde", pl);
    if (rc) return rc;
    // the scratch covers 8 waves per CU whatever the LDS allows (so it never shrinks as the grid grows), fewer where one wave's
    // scratch is large; the launch runs the waves the LDS lets the CUs hold, at most that many
    // (beyond kRingMaxScratch the size is that cap -- or one wave's scratch -- so it does not shrink either)
    const long long cus = device_cu_count();
    long long slots = cus * 8 < npairs ? cus * 8 : npairs;
    pl.ws_bytes = pl.per_wave * (size_t)slots;
    if (pl.ws_bytes > kRingMaxScratch) {
        slots = (long long)(kRingMaxScratch / pl.per_wave);
        if (slots < 1) slots = 1;
        pl.ws_bytes = pl.per_wave > kRingMaxScratch ? pl.per_wave : kRingMaxScratch;
    }
    pl.grid = (int)(pl.resident < slots ? pl.resident : slots);
    return SIGSVGD_OK;
}

// the kernel family for ring_launch (ring_sweep.h): one kernel, whatever static kernel made the grid
struct PdeFamily {
    using Args = PdeArgs;
    static constexpr bool has_kind = false, has_fwd_only = true;
    static constexpr const char *attr_failed = "hipFuncSetAttribute(sig_pde)", *launch_failed = "launch sig_pde_kernel";
    template <typename IO, bool NAIVE, bool GRAD, int KIND>
    static constexpr auto kernel() { return &sig_pde_kernel<IO, NAIVE, GRAD>; }
};
} // namespace

// bytes of the launch's scratch (0 for forward-only launches: the forward sweep keeps nothing)
int pde_workspace(int npairs, int M, int N, int n, int want_grad, size_t *bytes)
{
    return ring_plan_total<PdePlan>(bytes, [&](PdePlan &pl) { return pde_make_plan(npairs, M, N, n, want_grad, pl); });
}

// the argument checks are the entry points' (capi.hip); dG_out == NULL: forward only
int pde_launch(const void *G, int npairs, int M, int N, int dtype, int n, bool naive, bool exact, const void *grad_out,
               void *K_out, void *dG_out, void *ws, size_t ws_bytes, hipStream_t stream)
{
    const int want_grad = dG_out != nullptr;
    PdePlan pl;
    int rc = pde_make_plan(npairs, M, N, n, want_grad, pl);
    unsigned char *base = nullptr;
    if (!rc) rc = ring_ws_base("pde", ws, ws_bytes, pl.total(), base);
    if (rc) return rc;
    PdeArgs a;
    a.G = G; a.grad_out = grad_out; a.K_out = K_out; a.dG_out = dG_out;
    a.wsk = reinterpret_cast<float *>(base);
    a.wsk_per_block = pl.per_wave / sizeof(float);
    a.npairs = npairs; a.M = M; a.N = N; a.n = n; a.r = pl.r; a.P = pl.P; a.Q = pl.Q;
    a.nbands = pl.nbands; a.nsteps = pl.nsteps; a.nrow = pl.nrow; a.W = pl.W;
    a.inv_r2 = 1.0 / ((double)pl.r * (double)pl.r);
    if (exact && want_grad && !naive) { // (with the first-order stencil GG is the exact adjoint: the launch below)
        hipError_t e = pde_exact_launch(dtype, pl.grid, pl.lds, stream, a);
        if (e != hipSuccess) return hip_fail(e, PdeFamily::attr_failed);
        e = hipGetLastError();
        return e != hipSuccess ? hip_fail(e, PdeFamily::launch_failed) : SIGSVGD_OK;
    }
    return ring_launch<PdeFamily>(dtype, SIGSVGD_STATIC_RBF, naive, want_grad != 0, pl, stream, a);
}

} // namespace sigsvgd
