// Host side of the register-resident fast path (n == 0, T <= 64): which shapes it takes, its workspace plan and its two entry
// points.  The kernel and the launchers of its instantiations are in gram_fast_kernel.h; this unit builds the RBF ones and
// sends the IMQ / rational-quadratic launches to gram_fast_radial.hip and the RBF launches of 17 to 32 channels to
// gram_fast_wide.hip.  The shared launch tail is sweep_host.hip's.
#include <cstdlib>

#include "gram_fast_kernel.h"

namespace sigsvgd {

bool fast_supported(int T, int d, int n) { return n == 0 && T >= 3 && T <= 64 && d <= 16; }
// the shapes of the 32-channel layout (gram_fast_wide.hip; RBF with SIGSVGD_FLAG_FP32_SWEEPS only: gram_route)
bool fast_wide_supported(int T, int d, int n) { return n == 0 && T >= 3 && T <= 64 && d >= 17 && d <= 32; }

namespace {
// geometry of a GRADIENT launch (the forward-only launches keep no partial sums): rows per tile, workgroups a CU holds
inline int grad_nw(int T, int d) { return (d <= 8) ? 8 : 4; } // (T <= 32: 4 wavefronts of two rows each)
inline int grad_wg_per_cu(int T, int d) { return (d <= 8 && T <= 32) ? 3 : 1; }
GradGeom fast_geometry(int A, int B, int T, int d, bool sym, int off, int stride, bool fold)
{
    return grad_geometry(A, B, T * d, sym, off, stride, fold, grad_nw(T, d), (long long)device_cu_count() * grad_wg_per_cu(T, d));
}
} // namespace

int sym_tile_rows_fast(int T, int d) { return grad_nw(T, d); }

// Gradient launches of 64-point paths run the kernel whose sweeps build their EXEC windows from immediates (PFIX = 63).
// SIGSVGD_SWEEP_WINDOWS=table (read per launch, here, like SIGSVGD_BAND_MODE in capi.hip) keeps them on the table form: the tests compare
// the two on one build.  Every other length, and the forward-only launches, have the table form only.
static bool fixed_windows(int T, int want_grad)
{
    if (T != 64 || !want_grad) return false;
    const char *e = getenv("SIGSVGD_SWEEP_WINDOWS");
    return !(e && e[0] == 't');
}

// ... and, where that kernel has a wave-balance twin (fast_has_balance, gram_fast_kernel.h), the twin, unless
// SIGSVGD_WAVE_BALANCE=off (read per launch, like SIGSVGD_SWEEP_WINDOWS above)
static bool wave_balance(int T, int d, int want_grad, bool sym)
{
    if (!sym || d > 8 || !fast_has_balance<8, true>() || !fixed_windows(T, want_grad)) return false;
    const char *e = getenv("SIGSVGD_WAVE_BALANCE");
    return !(e && e[0] == 'o' && e[1] == 'f');
}

// ... or, for d = 7 (fast_has_half), the half-offset twin, unless SIGSVGD_HALF_OFFSET=off (read per launch, like the two above)
static bool half_offset(int T, int d, int want_grad, bool sym)
{
    if (!sym || d != 7 || !fast_has_half<8, true, true>() || !fixed_windows(T, want_grad)) return false;
    const char *e = getenv("SIGSVGD_HALF_OFFSET");
    return !(e && e[0] == 'o' && e[1] == 'f');
}

// ... and there the twin that stages every column from its image (the kernel's HALF = 2), unless SIGSVGD_COLUMN_IMAGES=off (read
// per launch, like the three above); the plan records the choice, so the workspace query and the launch agree
static bool column_images()
{
    const char *e = getenv("SIGSVGD_COLUMN_IMAGES");
    return !(e && e[0] == 'o' && e[1] == 'f');
}

// ---- column images of the HALF = 2 twin (gram_fast_kernel.h, IMG) -----------------------------------------------------------
constexpr int COLIMG_DOUBLES = 64 * 8 + 8; // [64][8] as the kernel's yd holds a column, then the 8 doubles of its yref
inline size_t colimg_bytes(int B) { return ((size_t)B * COLIMG_DOUBLES * sizeof(double) + 255) & ~(size_t)255; }

// The scaled norm of a point, nscale * |y~_t|^2, as stage_store of gram_fast_kernel forms it in lane c == 0 of the point's eight
// lanes -- the number phase 1 adds to every exponent of the column, so its bits are the result's bits.  There the source reads
// `s = v * v * nscale; s += shfl_xor(s, 1); s += shfl_xor(s, 2); s += shfl_xor(s, 4)` and hipcc contracts the first level: the
// lane's own product enters as a fused multiply-add, the neighbour's arrives rounded.  Stated here operation by operation.
__device__ __forceinline__ double column_norm(double v, double nscale)
{
#pragma clang fp contract(off)
    const double vv = v * v;
    const double s = vv * nscale;
    double r = __builtin_fma(nscale, vv, __shfl_xor(s, 1, 64));
    r = r + __shfl_xor(r, 2, 64);
    r = r + __shfl_xor(r, 4, 64);
    return r;
}

// One workgroup per column j, thread e = element (t = e / 8, c = e % 8) as in stage_store: channels 0..6 the point centred on the
// column's first point (fp64 of the fp32 or fp64 input), channel 7 the scaled norm; then the first point itself (channel 7: 0).
// Every double of the image is written: the workspace comes as it is.
__global__ __launch_bounds__(512) void fast_column_image_kernel(const void *Y, double *img, int io64, double inv_h)
{
    constexpr int T = 64, d = 7, DPAD = 8;
    const int j = blockIdx.x, e = threadIdx.x, t = e / DPAD, c = e % DPAD;
    const double nscale = -inv_h * 1.4426950408889634074; // (the kernel's, RBF)
    double sv = 0.0, sr = 0.0;
    if (c < d) {
        sv = load_any(Y, ((size_t)j * T + t) * d + c, io64);
        sr = load_any(Y, (size_t)j * T * d + c, io64);
    }
    const double v = sv - sr;
    const double s = column_norm(v, nscale);
    double *o = img + (size_t)j * COLIMG_DOUBLES;
    if (c < d) o[e] = v;
    if (c == 0) o[e + DPAD - 1] = s;
    if (t == 0) o[T * DPAD + c] = sr;
}

// [flags (the 4-channel instantiations, i.e. paths in one to four channels: see the kernel)][row segments][column slab][column images]
// (kind: the IMQ and rational-quadratic launches have the general-window kernels only; the areas are kind-independent)
WsPlan fast_plan(int A, int B, int T, int d, int want_grad, bool sym, int off, int stride, bool fold, int kind)
{
    WsPlan w;
    const bool rbf = kind == SIGSVGD_STATIC_RBF;
    w.fixed_windows = rbf && d <= 16 && fixed_windows(T, want_grad) ? 1 : 0; // (the 32-channel kernels: general windows only)
    w.wave_balance = rbf && wave_balance(T, d, want_grad, sym) ? 1 : 0;
    w.half_offset = rbf && half_offset(T, d, want_grad, sym) ? 1 : 0;
    if (d <= 4) w.kflag = w.take(flag_area_bytes(A, B));
    if (want_grad) {
        w.g = fast_geometry(A, B, T, d, sym, off, stride, fold);
        w.rseg = w.take(w.g.rseg_bytes);
        w.cslab = w.take(w.g.cslab_bytes);
    }
    w.column_images = w.half_offset && column_images() ? 1 : 0;
    // (after the areas every fast launch has: their offsets stay.  The areas are kind-independent -- an IMQ / rational-quadratic
    //  launch is sized like the RBF launch of its shape, tests/test_fp32_static_cabi.py -- so those take the area and leave it unused)
    if (half_offset(T, d, want_grad, sym) && column_images()) w.colimg = w.take(colimg_bytes(B));
    return w;
}

namespace {
// cut the workspace from the plan, enqueue the kernel over the row tiles `own` says (off / stride / fold: the tile count is the
// kernel's), the fp64 pass and (gradient) the reduction into `out`
int run(const GramProblem &p, const WsPlan &w, bool sym, const TileMap &own, void *out, int out64)
{
    unsigned char *base = nullptr;
    int rc = ws_base(p, w, "fast", base);
    if (rc) return rc;
    FastArgs a{};
    fill_sweep_args(a, p, w, base);
    a.tm = own;
    if (w.column_images) { // the HALF = 2 twin reads the columns from their images: formed here, in front of it on the same stream
        double *img = ws_at<double>(base, w.colimg);
        hipLaunchKernelGGL(fast_column_image_kernel, dim3((unsigned)p.B), dim3(512), 0, p.stream, p.Y, img, a.io64, p.inv_h);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "launch fast_column_image_kernel");
        a.Y = img;
    }
    int tile_rows = 0;
    rc = p.kind != SIGSVGD_STATIC_RBF ? fast_radial_dispatch(p, a, w, out != nullptr, sym, tile_rows)
         : p.d > 16                   ? fast_wide_dispatch(p, a, w, out != nullptr, sym, tile_rows)
                                      : dispatch_variant<0>(p, a, w, out != nullptr, sym, tile_rows);
    if (rc) return rc;
    return finish_launch(p, w, base, sym, a.tm, tile_rows, out, out64);
}
} // namespace

int fast_launch(const GramProblem &p)
{
    const bool sym = (p.flags & SIGSVGD_FLAG_Y_IS_X) && p.A == p.B; // Y is X: each unordered pair once, K mirrored
    const WsPlan w = fast_plan(p.A, p.B, p.T, p.d, p.gradX_out != nullptr, sym, 0, 1, false, p.kind);
    return run(p, w, sym, make_tilemap(1, 0, 1, false), p.gradX_out, p.dtype == SIGSVGD_F64);
}

// Symmetric partial solve for particle sharding: this launch owns the row tiles tile_offset + k*tile_stride of the upper
// triangle of Gram(X, X).  K_partial[N,N] (caller-zeroed) receives both orientations of every owned pair;
// grad_partial[N,T,d] (fp64) is OVERWRITTEN with this launch's share of the gradient (rows it does not touch get 0).
int fast_sym_partial(const GramProblem &p, int tile_offset, int tile_stride, bool fold, double *grad_partial)
{
    const WsPlan w = fast_plan(p.A, p.B, p.T, p.d, 1, true, tile_offset, tile_stride, fold, p.kind);
    return run(p, w, true, make_tilemap((p.A + grad_nw(p.T, p.d) - 1) / grad_nw(p.T, p.d), tile_offset, tile_stride, fold),
               grad_partial, 1);
}

} // namespace sigsvgd

SIG_EXEC_DEBUG_GETTER(fast)
