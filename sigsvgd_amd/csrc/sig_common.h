// Shared device helpers for the signature-kernel HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#ifdef SIGSVGD_PHASE_STAMPS
#include <cstdarg>
#include <cstdio>
#endif

#include "../../include/sigsvgd_hip.h"

namespace sigsvgd {

constexpr int kWave = 64;

// ---- error plumbing (host) -------------------------------------------------------------------
void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);

// ---- fp64 exp -----------------------------------------------------------------------------
// exp(a) = 2^k * P(r), k = rint(a*log2e), r = a - k*ln2 (two-word ln2), P = degree-11 Taylor/Horner
// on |r| <= ln2/2.  Relative error < 3e-16 * few; enough for the 4-corner cancellation in the
// kernel increments (needs ~1e-10).  One v_rndne_f64 + v_cvt_i32_f64 + v_ldexp_f64 + 14 FMA/MUL.
__device__ __forceinline__ double exp64(double a0)
{
    double a = fmin(fmax(a0, -1000.0), 700.0); // (fmax / fmin drop a NaN: it is put back at the end)
    const double kf = __builtin_rint(a * 1.4426950408889634074);
    double r = __builtin_fma(kf, -6.93147180369123816490e-01, a);
    r = __builtin_fma(kf, -1.90821492927058770002e-10, r);
    double p = 2.50521083854417187751e-08;              // 1/11!
    p = __builtin_fma(p, r, 2.75573192239858906526e-07); // 1/10!
    p = __builtin_fma(p, r, 2.75573192239858906526e-06); // 1/9!
    p = __builtin_fma(p, r, 2.48015873015873015873e-05); // 1/8!
    p = __builtin_fma(p, r, 1.98412698412698412698e-04); // 1/7!
    p = __builtin_fma(p, r, 1.38888888888888888889e-03); // 1/6!
    p = __builtin_fma(p, r, 8.33333333333333333333e-03); // 1/5!
    p = __builtin_fma(p, r, 4.16666666666666666667e-02); // 1/4!
    p = __builtin_fma(p, r, 1.66666666666666666667e-01); // 1/3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    const double e = ldexp(p, (int)kf);
    return (a0 != a0) ? a0 : e; // a NaN in a path poisons its own row / column of K, as in the reference
}

// The Matern static kernels of the fp64 routes, k = phi(s) with s = |x - y|^2 inv_h: u = sqrt(3 s) and
// phi = (1 + u) e^-u, -phi' = (3/2) e^-u (Matern-3/2); u = sqrt(5 s) and phi = (1 + u + u^2 / 3) e^-u, -phi' = (5/6) (1 + u) e^-u
// (Matern-5/2).  One sqrt and one exp64 each; -phi'(0) is finite, so coincident points have a zero gradient term.
template <int KIND>
inline constexpr bool kMaternKind = KIND == SIGSVGD_STATIC_MATERN32 || KIND == SIGSVGD_STATIC_MATERN52;
// m32: Matern-3/2, else Matern-5/2 (a constant where the kind is a template parameter, wave-uniform in the coverage kernel).
// u from s clamped at 0: a distance formed as xn + yn - 2 dot can round a few ulp below 0 for coincident points (a NaN stays
// one: it poisons its row / column of K as for the other kinds)
__device__ __forceinline__ double matern_u(bool m32, double s)
{
    return sqrt((m32 ? 3.0 : 5.0) * (s < 0.0 ? 0.0 : s));
}
// (Both values end in an explicit fma, e + (u e) (1 + u / 3) for Matern-5/2: a product as the last operation could be
// contracted with the subtraction that follows it in one kernel's increments and not in another's, and the schedules and modes
// of the long route must agree bit for bit.)
__device__ __forceinline__ double matern_phi(bool m32, double u)
{
    const double e = exp64(-u);
    return m32 ? __builtin_fma(u, e, e) : __builtin_fma(u * e, __builtin_fma(u, 1.0 / 3.0, 1.0), e);
}
__device__ __forceinline__ double matern_slope(bool m32, double u) // -phi'(s)
{
    const double e = exp64(-u);
    return m32 ? 1.5 * e : (5.0 / 6.0) * __builtin_fma(u, e, e);
}

// 2^t for the register-resident kernels: t arrives already scaled by log2(e) (the scale is folded into the particle
// coordinates), so the reduction is exact: k = rint(t), f = t - k in [-1/2, 1/2], and 2^f is a degree-7 polynomial (max
// relative error 5.5e-11 on [-1/2, 1/2]; the kernels' increments are rounded to fp32, 6e-8 relative, right after).
struct Exp2Coef7 {
    double c7, c6, c5, c4, c3, c2, c1, c0;
};
__device__ __forceinline__ Exp2Coef7 exp2_coef7()
{
    return Exp2Coef7{1.5303701161442145e-05, 1.5469729221575116e-04, 1.3333478471058548e-03, 9.618025613268967e-03,
                     5.5504109063307244e-02, 2.4022651213498578e-01, 6.931471805568296e-01,  0.9999999999595621};
}
// A caller under register pressure keeps the coefficients in scalar registers: it makes them once and pins them in every
// iteration of its rolled loop (an empty `asm volatile("" : "+s"(c))`); hipcc otherwise materialises them as VGPR pairs
// (one v_mov_b64 per Horner step to feed v_fmac_f64) and may spill those (gram_quad.hip: 16 scratch round trips per use
// site).
__device__ __forceinline__ void exp2_coef7_pin(Exp2Coef7 &k)
{
    asm volatile("" : "+s"(k.c7), "+s"(k.c6), "+s"(k.c5), "+s"(k.c4), "+s"(k.c3), "+s"(k.c2), "+s"(k.c1), "+s"(k.c0));
}
__device__ __forceinline__ double exp2_p7(double t, const Exp2Coef7 &k)
{
    const double kf = __builtin_rint(t);
    const double f = t - kf;
    double p = __builtin_fma(k.c7, f, k.c6);
    p = __builtin_fma(p, f, k.c5);
    p = __builtin_fma(p, f, k.c4);
    p = __builtin_fma(p, f, k.c3);
    p = __builtin_fma(p, f, k.c2);
    p = __builtin_fma(p, f, k.c1);
    p = __builtin_fma(p, f, k.c0);
    return ldexp(p, (int)kf);
}
__device__ __forceinline__ double exp2_p7(double t) { return exp2_p7(t, exp2_coef7()); }

// ---- Goursat stencils -------------------------------------------------------------------------
// default (second order):  K11 = (K10 + K01)*(1 + g/2 + g^2/12) - K00*(1 - g^2/12)
// written in delta form so that the O(1) parts cancel exactly in fp64:
//   K11 = (t - K00) + t*a + K00*b,  t = K10 + K01, a = g/2 + g^2/12, b = g^2/12
// naive (first order):     K11 = K10 + K01 + K00*(g - 1)
__device__ __forceinline__ double stencil(double k10, double k01, double k00, double g, bool naive)
{
    const double t = k10 + k01;
    if (naive) return __builtin_fma(k00, g, t - k00);
    const double b = g * g * (1.0 / 12.0);
    const double a = __builtin_fma(g, 0.5, b);
    double u = t - k00;
    u = __builtin_fma(t, a, u);
    return __builtin_fma(k00, b, u);
}

// one element of the fp32 / fp64 (io64) I/O arrays as a double, and a double stored back
__device__ __forceinline__ double load_any(const void *b, size_t i, int io64)
{
    return io64 ? static_cast<const double *>(b)[i] : (double)static_cast<const float *>(b)[i];
}
__device__ __forceinline__ void store_any(void *b, size_t i, double v, int io64)
{
    if (io64)
        static_cast<double *>(b)[i] = v;
    else
        static_cast<float *>(b)[i] = (float)v;
}

// Neighbour-lane moves as DPP moves (wave_shr:1 / wave_shl:1).  __shfl_up / __shfl_down lower to ds_bpermute: an LDS round
// trip (~100 cycles) on the dependent chain of every PDE step, against ~8 cycles here.  Compiler-visible DPP: hipcc pads
// their hazards itself.
__device__ __forceinline__ double shfl_up_f64(double v) // lane l <- lane l-1 (lane 0 keeps own)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), 0x138, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), 0x138, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_down_f64(double v, double old) // lane l <- lane l+1 (lane 63 gets `old`)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), 0x130, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), 0x130, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_down_f64(double v) { return shfl_down_f64(v, v); } // (lane 63 keeps own)
__device__ __forceinline__ float shfl_up_zero(float v) // lane l <- lane l-1, lane 0 gets 0
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138, 0xF, 0xF, true));
}

// Sum over the lanes in DPP adds (no LDS round trip).  Lane 31 ends with the total of lanes 0 .. 31; lane 63 with the
// total of ALL 64 lanes if `WHOLE`, else of lanes 32 .. 63 (two pairs per wavefront in gram_fast_kernel.h).
template <bool WHOLE>
__device__ __forceinline__ float wave_sum_dpp(float v)
{
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, true)); // row_shr:1
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xF, 0xF, true)); // row_shr:2
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xF, 0xF, true)); // row_shr:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xF, 0xF, true)); // row_shr:8 (lane 15 of a row: its total)
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xA, 0xF, true)); // row_bcast:15 into rows 1, 3
    if (WHOLE) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xC, 0xF, true)); // row_bcast:31 into rows 2, 3
    return v;
}
// max(m, |a|, |b|) in one v_max3_f32
__device__ __forceinline__ float max3_abs(float m, float a, float b)
{
    asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(m) : "v"(a), "v"(b));
    return m;
}

// ---- phase stamps (diagnostic build -DSIGSVGD_PHASE_STAMPS, scripts/dev/phase_stamps.py) -----------------------------------
// s_memtime around the phases of a kernel, summed per wave in scalar registers (the kernel declares `ph_[phases]` and `tlast_`)
// and added to a buffer no output depends on; the launcher prints each phase's share.  Compiled out of the product.
#ifdef SIGSVGD_PHASE_STAMPS
#define SIG_STAMP(i)                                                         \
    {                                                                        \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();        \
        ph_[i] += now_ - tlast_;                                             \
        tlast_ = now_;                                                       \
    }
constexpr int kMaxPhases = 32; // (gram_fast_kernel.h keeps two sets of its 9: one per half of the workgroup)
// the per-phase totals of the next launch on `stream`, zeroed (one buffer: every report below synchronises)
inline unsigned long long *phase_stamps_begin(hipStream_t stream)
{
    static unsigned long long *buf = nullptr;
    if (!buf) (void)hipMalloc(&buf, kMaxPhases * sizeof(unsigned long long));
    (void)hipMemsetAsync(buf, 0, kMaxPhases * sizeof(unsigned long long), stream);
    return buf;
}
// after the launch: one stderr line "<printf(fmt, ...)><name> <share>% | ... total <n> wave-cycles" over the phases named
template <int N>
void phase_stamps_report(hipStream_t stream, const unsigned long long *buf, const char *const (&names)[N], const char *fmt, ...)
{
    static_assert(N <= kMaxPhases, "more phases than the buffer holds");
    unsigned long long h[kMaxPhases];
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost);
    double tot = 0;
    for (int k = 0; k < kMaxPhases; ++k) tot += (double)h[k];
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    for (int k = 0; k < N; ++k) fprintf(stderr, "%s %.1f%% | ", names[k], 100.0 * (double)h[k] / tot);
    fprintf(stderr, "total %.3e wave-cycles\n", tot);
}
// The same for a kernel that keeps the N phases twice, [0, N) summed over the older half of every workgroup (waves 0 ..
// NW/2 - 1) and [N, 2N) over the younger half: the line above over both halves together, then one line with the two halves side
// by side, each phase as a share of its own half's total.
template <int N>
void phase_stamps_report_halves(hipStream_t stream, const unsigned long long *buf, const char *const (&names)[N], const char *fmt, ...)
{
    static_assert(2 * N <= kMaxPhases, "more phases than the buffer holds");
    unsigned long long h[kMaxPhases];
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost);
    double tot[2] = {0, 0};
    for (int k = 0; k < N; ++k) {
        tot[0] += (double)h[k];
        tot[1] += (double)h[N + k];
    }
    char head[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(head, sizeof(head), fmt, ap);
    va_end(ap);
    fprintf(stderr, "%s", head);
    for (int k = 0; k < N; ++k) fprintf(stderr, "%s %.1f%% | ", names[k], 100.0 * (double)(h[k] + h[N + k]) / (tot[0] + tot[1]));
    fprintf(stderr, "total %.3e wave-cycles\n", tot[0] + tot[1]);
    fprintf(stderr, "%solder | younger half: ", head);
    for (int k = 0; k < N; ++k)
        fprintf(stderr, "%s %.1f%% | %.1f%% ; ", names[k], 100.0 * (double)h[k] / tot[0], 100.0 * (double)h[N + k] / tot[1]);
    fprintf(stderr, "total %.3e | %.3e wave-cycles\n", tot[0], tot[1]);
}
#else
#define SIG_STAMP(i)
#endif

// ---- EXEC discipline of the hand-written sweep statements ----------------------------------------------------------------
// The sweep statements (gram_fast_kernel.h sweep_fwd8 / sweep_rev8, quad_sweeps.h) move lane windows into EXEC and leave it at
// all ones.  EXEC is a reserved register for hipcc: a clobber on it is ignored with a warning ("inline asm clobber list
// contains reserved registers"), so the compiler cannot be told.  The statements are therefore only correct where the
// compiler's own EXEC is all ones too, i.e. in wave-uniform control flow -- which every call site is by construction (the
// conditions around them are functions of kernel arguments, block and wavefront indices).  -DSIGSVGD_CHECK_EXEC turns that
// into a run-time check: each statement group first compares EXEC with all ones and records a violation in a device-side
// sticky word per translation unit (scripts/dev/check_exec.py builds that variant, runs the kernel families through it and
// reads the words back; profiles/r04_exec_check.txt).
#ifdef SIGSVGD_CHECK_EXEC
static __device__ unsigned g_exec_violations; // one per translation unit; read back by sigsvgd_debug_exec_violations_<unit>()
#define SIG_EXEC_MUST_BE_FULL(what)                                                        \
    do {                                                                                   \
        if (__builtin_amdgcn_read_exec() != ~0ull) g_exec_violations = 1u;                 \
    } while (0)
#define SIG_EXEC_DEBUG_GETTER(unit)                                                        \
    extern "C" unsigned sigsvgd_debug_exec_violations_##unit(void)                         \
    {                                                                                      \
        unsigned v = 0xffffffffu;                                                          \
        (void)hipDeviceSynchronize();                                                      \
        (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(sigsvgd::g_exec_violations), sizeof(v));  \
        return v;                                                                          \
    }
#else
#define SIG_EXEC_MUST_BE_FULL(what)
#define SIG_EXEC_DEBUG_GETTER(unit)
#endif

// ---- launch descriptors shared by host code -----------------------------------------------------
struct GramProblem {
    const void *X, *Y;
    int A, B, T, d, dtype;
    double inv_h;
    int n;            // dyadic order
    int kind;         // SIGSVGD_STATIC_*
    unsigned flags;
    const void *grad_out; // nullable
    void *K_out;
    void *gradX_out;  // nullable => forward only
    void *ws;
    size_t ws_bytes;
    hipStream_t stream;
};

// A launch of the long-path route (gram_long.hip): the Gram and two-sided modes, the paired mode (B unused) and the partial
// mode (Y = X, B = A, TY = TX; gradX_out is the fp64 partial gradient).  The workspace queries read shape, order and flags only.
struct LongProblem {
    const void *X, *Y;
    int A, B, TX, TY, d, dtype;
    double inv_h;
    int n;            // dyadic order
    int kind;         // SIGSVGD_STATIC_*
    unsigned flags;
    const void *grad_out; // nullable
    void *K_out;
    void *gradX_out, *gradY_out; // nullable; both NULL => forward only
    void *ws;
    size_t ws_bytes;
    hipStream_t stream;
};

// fixed-order reduction of the gradient partial sums shared by the register-resident and the quadrant kernel -- sweep_host.hip
// Which row tiles a launch owns and the order it enumerates them in (kq = 0 .. owned-1).  A full launch owns all of
// them (off 0, stride 1).  The sharded partial solve of rank `off` of `stride` owns the tiles off + k*stride (cyclic), or
// -- SIGSVGD_FLAG_FOLD_TILES -- those AND their mirror images ntile-1 - (off + k*stride): in the upper triangle tile t
// has B - t*NW columns, so a tile and its mirror image together always cost the same and every rank gets the same
// number of items (cyclic ownership alone gives rank 0 5.4 % more than the mean at N=1024 on 8 ranks).
struct TileMap {
    int off, stride, ntile, owned, m0, fold; // m0 tiles of the first kind (off + k*stride), then owned - m0 mirror images
    __host__ __device__ int tile_of(int kq) const
    {
        return kq < m0 ? off + kq * stride : ntile - 1 - (off + (kq - m0) * stride);
    }
    __host__ __device__ int kq_of_tile(int ti) const // -1: not owned
    {
        if (ti >= off && (ti - off) % stride == 0 && (ti - off) / stride < m0) return (ti - off) / stride;
        const int p = ntile - 1 - ti;
        if (p >= off && (p - off) % stride == 0 && (p - off) / stride < owned - m0) return m0 + (p - off) / stride;
        return -1;
    }
    // items of the owned tiles 0 .. kq-1 in the tile-major enumeration of the kernels: symmetric launches count the
    // columns from the tile's first row on (B - tile*NW), ordered ones all B
    __host__ __device__ long long start(int kq, int B, int NW, int sym) const
    {
        if (!sym) return (long long)kq * B;
        const long long k1 = kq < m0 ? kq : m0, k2 = kq - k1;
        long long s = k1 * B - (long long)NW * ((long long)stride * k1 * (k1 - 1) / 2 + (long long)off * k1);
        s += k2 * ((long long)B - (long long)(ntile - 1 - off) * NW) + (long long)NW * stride * k2 * (k2 - 1) / 2;
        return s;
    }
};
TileMap make_tilemap(int ntile, int off, int stride, bool fold);

struct GradGeom {
    int NW, grid;
    TileMap tm;
    long long nitems;
    size_t rseg_bytes, cslab_bytes;
};
int device_cu_count();
GradGeom grad_geometry(int A, int B, int TD, bool sym, int off, int stride, bool fold, int NW, long long resident);
int grad_reduce_launch(const GradGeom &g, const double *rseg, const float *cslab, void *out, int out64, int A, int B, int TD,
                       bool sym, hipStream_t stream);

// ---- workspace plans ------------------------------------------------------------------------------------------------------
// One launch's workspace: areas at byte offsets from the 256-B aligned base of the caller's buffer (an area of 0 bytes is not
// used) and `total()`, the bytes the caller gives (alignment slack included).  Every family has one plan function; its launcher
// checks the caller's size against that plan and cuts the buffer from it, and sigsvgd_gram_workspace_bytes returns the
// largest total of the launches a call can reach.  `sym` below is the Y_IS_X orientation (each unordered pair once).
struct WsArea {
    size_t off = 0, bytes = 0;
};
struct WsPlan {
    GradGeom g{}; // geometry of the fp32-sweep kernels' launch (grad_reduce_launch re-derives its segments from it)
    WsArea kflag;        // [A][B] cancellation flags the fp64 pass reads
    WsArea rseg, cslab;  // row segments, column slab of the gradient
    WsArea colimg;       // gram_fast.hip: [B] column images of the half-offset twin that stages from them (column_images below)
    WsArea crec, rowg, dcache; // gram_quad.hip: column records, row accumulators, increment scratch
    WsArea wsk;          // forward-solution scratch (gram_band.hip, gram_generic.hip)
    WsArea counter, partials, colslab; // gram_generic.hip: work counter, gradient partials, column-side slab
    int fixed_windows = 0; // gram_fast.hip: the launch runs the kernel whose sweeps have their EXEC windows as immediates
    int wave_balance = 0;  // gram_fast.hip: ... and, where that kernel has a wave-balance twin, the twin
    int half_offset = 0;   // gram_fast.hip: ... or, where it has one, the twin that runs the halves of a workgroup half a pair apart
    int column_images = 0; // gram_fast.hip: ... and stages every column from its LDS image, formed once per launch into `colimg`
    size_t end = 0; // bytes of the areas
    WsArea take(size_t bytes) // the next area, behind the ones taken so far
    {
        const WsArea a{end, bytes};
        end += bytes;
        return a;
    }
    size_t total() const { return end + 256; } // (+ the slack of aligning the caller's pointer)
};
inline size_t flag_area_bytes(int A, int B) { return ((size_t)A * B + 255) & ~(size_t)255; }
template <typename T>
inline T *ws_at(unsigned char *base, const WsArea &a)
{
    return a.bytes ? reinterpret_cast<T *>(base + a.off) : nullptr;
}
// `base` = p.ws aligned to 256 B; SIGSVGD_E_WORKSPACE (message "<family>: workspace ... required N B") when the caller's
// buffer is smaller than w.total() -- a plan without areas takes any buffer, NULL included -- sweep_host.hip, as finish_launch
int ws_base(const GramProblem &p, const WsPlan &w, const char *family, unsigned char *&base);
// the tail of the fp32-sweep launches: the fp64 pass over the flagged pairs of the rows of the tiles `tm` owns (tile_rows rows
// each), then the fixed-order gradient reduction into `out` (fp64 when out64; NULL: a forward-only launch)
int finish_launch(const GramProblem &p, const WsPlan &w, unsigned char *base, bool sym, const TileMap &tm, int tile_rows,
                  void *out, int out64);

// the arguments every fp32-sweep family (FastArgs, QuadArgs, DyadArgs, BandArgs) takes from the problem and from its plan's
// workspace; the launchers set the rest
template <typename Args>
void fill_sweep_args(Args &a, const GramProblem &p, const WsPlan &w, unsigned char *base)
{
    a.X = p.X; a.Y = p.Y; a.go = p.grad_out; a.K = p.K_out;
    a.kflag = ws_at<unsigned char>(base, w.kflag); a.rseg = ws_at<double>(base, w.rseg); a.cslab = ws_at<float>(base, w.cslab);
    a.io64 = p.dtype == SIGSVGD_F64; a.A = p.A; a.B = p.B; a.T = p.T; a.d = p.d;
    a.symw = (p.flags & SIGSVGD_FLAG_SYM) ? 1 : 0; a.inv_h = p.inv_h;
}

// Raises the dynamic-LDS limit of `KERNEL` to the 160 KB of a CU, once per instantiation and device: the call costs ~10 us
// of host time, which a small launch -- the fp64 pass behind a 50-us kernel -- would pay every time, and the attribute
// belongs to the current device's copy of the function (a process may drive several; devices >= 64: raised every time).
template <auto KERNEL>
hipError_t raise_lds_limit()
{
    static std::atomic<unsigned long long> raised{0}; // bit = device ordinal
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !((raised.load(std::memory_order_acquire) >> dev) & 1ull)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           160 * 1024);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) raised.fetch_or(1ull << dev, std::memory_order_release);
    }
    return hipSuccess;
}

// ---- kernel families --------------------------------------------------------------------------------------------------
// *_supported: the shapes a family's kernels take (dyadic order n; RBF static kernel, second-order solver).  Only gram_route
// (capi.hip) combines them into the choice of kernel.

// generic (any T, n, d that fits LDS) -- gram_generic.hip
// precise: fp64 increments wherever they fit (FORCE_GENERIC); any_size: symmetric launches solve each unordered pair once
// (mirrored K) whatever their pair count
int generic_plan(int A, int B, int T, int d, int n, int want_grad, bool sym, bool precise, bool any_size, WsPlan &w);
int generic_launch(const GramProblem &p, bool precise, bool any_size);
// fp64 pass of the coverage kernel over the pairs a fp32-sweep kernel flagged (flags [A][B] bytes; `sym`: the pairs j >= i,
// K mirrored; rows of the tiles `tm` owns, `tile_rows` rows each) -- gram_generic.hip
int generic_repair_launch(const GramProblem &p, const unsigned char *flags, bool sym, const TileMap &tm, int tile_rows);

// register-resident fast path (n == 0, T <= 64) -- gram_fast.hip (kernel: gram_fast_kernel.h); off / stride / fold: the row tiles a partial solve owns
bool fast_supported(int T, int d, int n);
bool fast_wide_supported(int T, int d, int n); // 17 .. 32 channels: gram_fast_wide.hip, RBF with SIGSVGD_FLAG_FP32_SWEEPS only
WsPlan fast_plan(int A, int B, int T, int d, int want_grad, bool sym, int off = 0, int stride = 1, bool fold = false,
                 int kind = SIGSVGD_STATIC_RBF); // (IMQ / rational quadratic with SIGSVGD_FLAG_FP32_SWEEPS: general windows only)
int fast_launch(const GramProblem &p);
int fast_sym_partial(const GramProblem &p, int tile_offset, int tile_stride, bool fold, double *grad_partial);
int sym_tile_rows_fast(int T, int d); // rows per tile of the gradient launches (ownership unit of the partial solve)

// long paths, stored forward solution, 2 x 2 quadrants of 64 x 64 cells at two waves per SIMD -- gram_quad.hip
bool quad_supported(int T, int d, int n);
WsPlan quad_plan(int A, int B, int T, int d, int want_grad, bool sym, int off = 0, int stride = 1, bool fold = false);
int quad_launch(const GramProblem &p);
int quad_sym_partial(const GramProblem &p, int tile_offset, int tile_stride, bool fold, double *grad_partial);

// short paths with dyadic refinement, refined grid of 64 .. 128 cells per side, on the quadrant sweep engine -- gram_dyad.hip
bool dyad_supported(int T, int d, int n);
WsPlan dyad_plan(int A, int B, int T, int d, int want_grad, bool sym);
int dyad_launch(const GramProblem &p);

// refined grids of 64 .. 256 cells per side, one wavefront per band of 64 rows of a pair (band-parallel) or per pair
// (serial) -- gram_band.hip
bool band_supported(int T, int d, int n);
int band_wg_per_cu(int T, int d, int n, bool serial); // workgroups of a schedule a CU holds
WsPlan band_plan(int A, int B, int T, int d, int n, int want_grad, bool sym, bool serial);
int band_launch(const GramProblem &p, bool serial);

} // namespace sigsvgd
