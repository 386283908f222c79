// extern "C" entry points of libsigsvgd_hip.so (declared in include/sigsvgd_hip.h).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>

#include "sig_common.h"

namespace sigsvgd {

static thread_local char g_err[512] = "";

static void set_error_v(const char *fmt, va_list ap) { vsnprintf(g_err, sizeof(g_err), fmt, ap); }

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    set_error_v(fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what)
{
    set_error("%s: %s", what, hipGetErrorString(e));
    return SIGSVGD_E_HIP;
}

// a refused argument: set_error with the message, and the status every such refusal returns
static int bad_arg(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    set_error_v(fmt, ap);
    va_end(ap);
    return SIGSVGD_E_BADARG;
}

int phi_launch(const float *K, const float *score, const float *grad_k, const float *mask, int N, int D,
               float *v_out, const float *X_in, float *X_out, float lr, float *adagrad, hipStream_t stream,
               float *exp_avg = nullptr, float *exp_avg_sq = nullptr, int *step_dev = nullptr, double lr_adam = 0.0,
               double beta1 = 0.0, double beta2 = 0.0, float eps = 0.f);
int update_launch(const float *v_in, const float *mask, int N, int D, float *v_out, const float *X_in, float *X_out,
                  float lr, float *adagrad, hipStream_t stream, float *exp_avg, float *exp_avg_sq, int *step_dev,
                  double lr_adam, double beta1, double beta2, float eps);

int vec_sqdist_launch(const void *X, const void *Y, const void *XM, const void *YM, int A, int B, int D, int dtype,
                      void *sq, hipStream_t stream);
int vec_kgrad_launch(const void *sq, const void *XM, const void *YM, const void *go, int A, int B, int D, int dtype,
                     int kind, double inv_h2, double grad_scale, void *K, void *dK, hipStream_t stream);
bool vec_fused_supported(int D, int dtype);
int vec_fused_launch(const void *X, const void *Y, const void *XM, const void *YM, const void *go, int A, int B, int D,
                     int kind, double inv_h2, double grad_scale, void *K, void *dK, void *ws, size_t ws_bytes, hipStream_t stream);
size_t vec_fused_workspace_bytes(int A, int B, int D);
long long signature_channels(int C, int depth);
int obstacle_cost_launch(const float *x, int N, int Kx, int d, const float *start, const float *target, const float *basis,
                         int Tt, const float *logw, const float *mean, const float *stdv, int M, float w_obst, float w_len,
                         float *cost, float *traj, float *grad_x, hipStream_t stream);
int signature_launch(const void *X, int N, int L, int C, int depth, int basepoint, int dtype, void *out,
                     hipStream_t stream);
int signature_bwd_launch(const void *X, const void *gsig, int N, int L, int C, int depth, int basepoint, int dtype, void *gX,
                         long long sigdim, hipStream_t stream);
int pde_workspace(int npairs, int M, int N, int n, int want_grad, size_t *bytes);
int pde_launch(const void *G, int npairs, int M, int N, int dtype, int n, bool naive, bool exact, const void *grad_out,
               void *K_out, void *dG_out, void *ws, size_t ws_bytes, hipStream_t stream);
// the long-path route (gram_long.hip); the queries read the problem's shape, order and flags only
int long_workspace(const LongProblem &p, int want_grad, size_t *bytes);
int long_launch(const LongProblem &p);
int pair_workspace(const LongProblem &p, int want_grad, size_t *bytes);
int pair_launch(const LongProblem &p);
int pair_schedule(const LongProblem &p, int want_grad, int *waves_per_pair, int *grid, size_t *lds_bytes);
int long2_workspace(const LongProblem &p, int want_gradX, int want_gradY, size_t *bytes);
int long2_launch(const LongProblem &p);
int pair_h_launch(const LongProblem &p, void *dk_out);
int long2_h_workspace(const LongProblem &p, int want_gradX, int want_gradY, size_t *bytes);
int long2_h_launch(const LongProblem &p, void *dk_out);
int long_part_tiles(const LongProblem &p, int stride, int *R, int *JC);
int long_part_workspace(const LongProblem &p, int off, int stride, size_t *bytes);
int long_part_launch(const LongProblem &p, int off, int stride);
// the fused route's normalised launch: the diagonal pass (gram_long.hip) and the two kernels around
// the pair solve (gram_norm_fused.hip)
int norm_diag_workspace(int rows, int T, int d, int n, int want_grad, size_t *bytes);
int norm_diag_launch(const LongProblem &p, double *ln_out, double *grad);
hipError_t norm_fused_weights(int dtype, const void *go, const double *lnA, const double *lnB, void *W, int A, int B, bool sym,
                              bool yx, hipStream_t stream);
hipError_t norm_fused_finish(int dtype, void *K, const void *go, const double *lnA, const double *lnB, int A, int B, bool sym,
                             bool yx, void *gradX, const double *diag, double *sums, int TD, hipStream_t stream);
// the distance select (sqdist_select.hip)
size_t select_workspace_bytes();
int select_launch(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, unsigned flags,
                  unsigned long long rank, unsigned long long n, double *out, void *ws, size_t ws_bytes, hipStream_t stream);

// the refusal of a workspace query without a place for its answer
static bool no_bytes(const size_t *bytes)
{
    if (!bytes) set_error("bytes == NULL");
    return !bytes;
}

// the static kernels the library evaluates itself, and those of them that are functions of |x - y|^2 inv_h (inv_h > 0)
// (an explicit set: the values 4 and 5 between the rational quadratic and the Matern kinds are reserved and refused)
static bool static_kind_known(int kind)
{
    switch (kind) {
    case SIGSVGD_STATIC_RBF:
    case SIGSVGD_STATIC_LINEAR:
    case SIGSVGD_STATIC_IMQ:
    case SIGSVGD_STATIC_RQ:
    case SIGSVGD_STATIC_MATERN32:
    case SIGSVGD_STATIC_MATERN52: return true;
    default: return false;
    }
}
static bool static_kind_radial(int kind) { return static_kind_known(kind) && kind != SIGSVGD_STATIC_LINEAR; }
// the kinds that have fp64 kernels only, with the default stencil only on the long-path route (DESIGN.md sections 5.15, 5.17)
static bool static_kind_fp64_only(int kind) { return static_kind_radial(kind) && kind != SIGSVGD_STATIC_RBF; }
static const char *static_kind_name(int kind)
{
    switch (kind) {
    case SIGSVGD_STATIC_RBF: return "RBF";
    case SIGSVGD_STATIC_IMQ: return "IMQ";
    case SIGSVGD_STATIC_MATERN32: return "Matern-3/2";
    case SIGSVGD_STATIC_MATERN52: return "Matern-5/2";
    default: return "rational-quadratic";
    }
}

// ---- which entry point takes which flag: the table of include/sigsvgd_hip.h, stated by tests/test_flag_contract_cpu.py ----
// A new flag is a row of kFlags, a bit in the rules of the families that take it and, where it excludes others, a row of
// kNotBuiltWith.  Every refusal here comes before any device work.
enum : unsigned {
    NV = SIGSVGD_FLAG_NAIVE_SOLVER, SYM = SIGSVGD_FLAG_SYM, YX = SIGSVGD_FLAG_Y_IS_X, FG = SIGSVGD_FLAG_FORCE_GENERIC,
    WC = SIGSVGD_FLAG_WS_CLEAN, SF = SIGSVGD_FLAG_STORED_FORWARD, FOLD = SIGSVGD_FLAG_FOLD_TILES, FP32 = SIGSVGD_FLAG_FP32_SWEEPS,
    EX = SIGSVGD_FLAG_EXACT_ADJOINT, NT = SIGSVGD_FLAG_NAN_TAILS, LK = SIGSVGD_FLAG_LOG_K, NM = SIGSVGD_FLAG_NORMALIZED,
    NF = SIGSVGD_FLAG_NORMALIZED_FUSED
};
// the flags in the order of their bits; not_built_for: what an entry point without kernels for the bit says of itself and of
// those that have them (the flags no rule lists under `not_built` have none)
struct FlagName { unsigned bit; const char *name, *not_built_for; };
static const FlagName kFlags[] = {
    {NV, "NAIVE_SOLVER"}, {SYM, "SYM"}, {YX, "Y_IS_X"}, {FG, "FORCE_GENERIC"}, {WC, "WS_CLEAN"}, {SF, "STORED_FORWARD"},
    {FOLD, "FOLD_TILES"}, {FP32, "FP32_SWEEPS"},
    {EX, "EXACT_ADJOINT", "this route (the gradient launches of sigsvgd_pde_fwd_bwd, sigsvgd_gram_long_fwd_bwd / _fwd_bwd2 / "
                          "_fwd_bwd_h and sigsvgd_pair_fwd_bwd / _fwd_bwd_h take it)"},
    {NT, "NAN_TAILS", "this entry point (sigsvgd_gram_long_fwd_bwd2, sigsvgd_pair_fwd, sigsvgd_pair_fwd_bwd, "
                      "sigsvgd_pair_schedule and their workspace queries take it)"},
    {LK, "LOG_K"}, {NM, "NORMALIZED"},
    {NF, "NORMALIZED_FUSED", "the partial solve (sigsvgd_gram_fwd, sigsvgd_gram_fwd_bwd and sigsvgd_gram_workspace_bytes take it)"},
};
// the pairs that are not built (DESIGN.md sections 5.20 to 5.23), each once: wherever `flag` is taken, none of `others` may
// be set beside it; the refusal names the first of them that is
struct NotBuiltWith { unsigned flag, others[4]; const char *why; };
static const NotBuiltWith kNotBuiltWith[] = {
    {NT, {EX}, "the exact adjoint's kernels solve every pair on the launch's grid"},
    {LK, {NV, EX, NT}, "the log-domain kernels are the default stencil's GG solve on the launch's grid"},
    {NM, {NV, EX, NT, LK}, "the normalised kernels are the log-domain solve of the default stencil on the launch's grid, and "
                           "store K^ where that flag stores ln K"},
    {NF, {NV}, "the diagonal pass is the log-domain solve of the default stencil"},
};
// One family of entry points: the name its refusals carry, the bits it takes (acts on, or accepts without effect), those only
// its forms with the reverse sweep take, and those it answers SIGSVGD_E_UNSUPPORTED ahead of every other check.  The fused
// route's entry points never refused the bits they do not know (`refuses_unknown` false): there those bits change nothing.
struct FlagRule { const char *who; unsigned taken, grad_taken, not_built; bool refuses_unknown = true; };
static const unsigned kFusedBits = NV | SYM | YX | FG | WC | SF | FOLD | FP32 | NF;
// (who, taken, grad_taken, not_built, refuses_unknown)
static const FlagRule kGramQuery{"gram_workspace_bytes", kFusedBits, 0, EX, false};
static const FlagRule kGramFwd{"gram_fwd", kFusedBits, 0, 0, false}; // (EX: ignored here, as it always was)
static const FlagRule kGramFwdBwd{"gram_fwd_bwd", kFusedBits, 0, EX, false};
static const FlagRule kSymPartial{"sym_partial", kFusedBits & ~NF, 0, EX | NF, false};
static const FlagRule kPde{"pde", NV, EX, 0};
static const FlagRule kLong{"gram_long", NV | SYM | YX, EX, NT};
static const FlagRule kLong2{"gram_long", NV | SYM | YX | NT | LK | NM, EX, 0};
static const FlagRule kLongH{"gram_long", NV | SYM | YX | EX, 0, NT};
static const FlagRule kLongPartial{"gram_long", NV | SYM | YX | FOLD, 0, EX | NT};
static const FlagRule kPair{"pair", NV | NT | LK, EX, 0};
static const FlagRule kPairH{"pair", NV | EX, 0, NT};
static const FlagRule kSelect{"sqdist_select", YX, 0, 0};

enum Form { QUERY, LAUNCH };      // what a check can know: a query's shape, order, kind and flags; a launch's pointers, dtype, inv_h too
enum Sweeps { FORWARD, REVERSE }; // REVERSE: the form runs the reverse sweep (a gradient launch, or its query)
static Sweeps reverse_if(bool grad) { return grad ? REVERSE : FORWARD; }
enum FlagChecks { NOT_BUILT = 1, UNKNOWN = 2, EVERY_CHECK = 3 };

static const char *flag_name(unsigned bit)
{
    for (const FlagName &f : kFlags)
        if (f.bit == bit) return f.name;
    return "?";
}

// The flags of one call against its family's rule, in this order: the bits the family has no kernels for, the pairs that are
// not built (both UNSUPPORTED), then the bits it does not know (BADARG; the message lists the ones it takes).  `which`: the
// long-path families check their pointers and shape between the second and the third.
static int check_flags(const FlagRule &r, unsigned flags, Sweeps sweeps = FORWARD, int which = EVERY_CHECK)
{
    for (const FlagName &f : kFlags) {
        if (!(which & NOT_BUILT) || !(flags & r.not_built & f.bit)) continue;
        set_error("%s: SIGSVGD_FLAG_%s is not built for %s", r.who, f.name, f.not_built_for);
        return SIGSVGD_E_UNSUPPORTED;
    }
    for (const NotBuiltWith &pair : kNotBuiltWith) {
        if (!(which & NOT_BUILT) || !(flags & r.taken & pair.flag)) continue;
        for (unsigned other : pair.others) {
            if (!(flags & other)) continue;
            set_error("%s: SIGSVGD_FLAG_%s together with SIGSVGD_FLAG_%s is not built (%s)", r.who, flag_name(pair.flag),
                      flag_name(other), pair.why);
            return SIGSVGD_E_UNSUPPORTED;
        }
    }
    const unsigned taken = r.taken | (sweeps == REVERSE ? r.grad_taken : 0u), unknown = flags & ~taken;
    if (!(which & UNKNOWN) || !r.refuses_unknown || !unknown) return SIGSVGD_OK;
    char list[128] = "";
    for (const FlagName &f : kFlags)
        if (taken & f.bit) snprintf(list + strlen(list), sizeof(list) - strlen(list), "%s%s", list[0] ? ", " : "", f.name);
    return bad_arg("%s: unknown flag bits 0x%x (%s only)", r.who, unknown, list);
}

static int check_common(const void *X, const void *Y, int A, int B, int T, int d, int dtype, double inv_h,
                        int n, int kind, unsigned flags, const void *K_out)
{
    if (!X || !Y || !K_out) return bad_arg("null pointer argument");
    if (A < 1 || B < 1 || T < 2 || d < 1)
        return bad_arg("bad shape A=%d B=%d T=%d d=%d (need A,B,d >= 1 and T >= 2)", A, B, T, d);
    if (dtype != SIGSVGD_F32 && dtype != SIGSVGD_F64) return bad_arg("bad dtype %d", dtype);
    if (!static_kind_known(kind)) return bad_arg("bad static kernel kind %d", kind);
    if (n < 0 || n > 10) return bad_arg("bad dyadic order %d", n);
    if (static_kind_radial(kind) && !(inv_h > 0.0))
        return bad_arg("%s static kernel needs inv_h > 0 (got %g)", static_kind_name(kind), inv_h);
    if ((flags & SIGSVGD_FLAG_SYM) && A != B) return bad_arg("sym backward needs A == B");
    return SIGSVGD_OK;
}

// the shape, dtype, order and flag checks of the PDE entry points (sig_pde.hip)
static int check_pde(int npairs, int M, int N, int dtype, int n, unsigned flags, const FlagRule &rule, Sweeps sweeps)
{
    if (npairs < 1 || M < 2 || N < 2)
        return bad_arg("pde: bad shape npairs=%d M=%d N=%d (need npairs >= 1, M, N >= 2)", npairs, M, N);
    if (dtype != SIGSVGD_F32 && dtype != SIGSVGD_F64) return bad_arg("pde: bad dtype %d", dtype);
    if (n < 0 || n > 10) return bad_arg("pde: bad dyadic order %d", n);
    return check_flags(rule, flags, sweeps);
}

// The checks of the long-path entry points (gram_long.hip), each condition in one place.  check_long: the Gram mode's, which
// every mode shares -- for a LAUNCH the pointers, dtype and inv_h too, for a QUERY what a workspace query can know -- around
// the flags `rule` lets through: SIGSVGD_FLAG_SYM needs A == B and TX == TY, SIGSVGD_FLAG_NAIVE_SOLVER is built for RBF and
// linear only (UNSUPPORTED with IMQ, rational quadratic and Matern), SIGSVGD_FLAG_Y_IS_X has no effect in the Gram mode.
static int check_long(const LongProblem &p, Form form, const FlagRule &rule, Sweeps sweeps)
{
    const bool launch = form == LAUNCH;
    if (check_flags(rule, p.flags, sweeps, NOT_BUILT)) return SIGSVGD_E_UNSUPPORTED;
    if (launch && (!p.X || !p.Y || !p.K_out)) return bad_arg("gram_long: null pointer argument");
    if (p.A < 1 || p.B < 1 || p.TX < 2 || p.TY < 2 || p.d < 1)
        return bad_arg("gram_long: bad shape A=%d B=%d TX=%d TY=%d d=%d (need A, B, d >= 1 and TX, TY >= 2)", p.A, p.B, p.TX,
                       p.TY, p.d);
    if (!static_kind_known(p.kind)) return bad_arg("gram_long: bad static kernel kind %d", p.kind);
    if (p.n < 0 || p.n > 10) return bad_arg("gram_long: bad dyadic order %d", p.n);
    if (check_flags(rule, p.flags, sweeps, UNKNOWN)) return SIGSVGD_E_BADARG;
    if ((p.flags & SIGSVGD_FLAG_SYM) && (p.A != p.B || p.TX != p.TY))
        return bad_arg("gram_long: sym backward needs A == B and TX == TY (got A=%d B=%d TX=%d TY=%d)", p.A, p.B, p.TX, p.TY);
    if (launch && p.dtype != SIGSVGD_F32 && p.dtype != SIGSVGD_F64) return bad_arg("gram_long: bad dtype %d", p.dtype);
    if (launch && static_kind_radial(p.kind) && !(p.inv_h > 0.0))
        return bad_arg("gram_long: %s static kernel needs inv_h > 0 (got %g)", static_kind_name(p.kind), p.inv_h);
    // (the long-path kernels are built with the default stencil only for the newer kinds: DESIGN.md sections 5.15, 5.17)
    if ((p.flags & SIGSVGD_FLAG_NAIVE_SOLVER) && static_kind_fp64_only(p.kind)) {
        set_error("gram_long: SIGSVGD_FLAG_NAIVE_SOLVER is not built for the %s static kernel on the long-path route "
                  "(default stencil only)", static_kind_name(p.kind));
        return SIGSVGD_E_UNSUPPORTED;
    }
    return SIGSVGD_OK;
}

// the two-sided entry points: check_long's, and there SIGSVGD_FLAG_Y_IS_X means what it says: one batch in both slots
// (A == B, TX == TY), whose gradient has one slot; SYM too weights one slot only
static int check_long2(const LongProblem &p, Form form, const FlagRule &rule, Sweeps sweeps, bool want_gradY)
{
    const int rc = check_long(p, form, rule, sweeps);
    if (rc) return rc;
    if ((p.flags & SIGSVGD_FLAG_Y_IS_X) && (p.A != p.B || p.TX != p.TY))
        return bad_arg("gram_long2: Y_IS_X needs A == B and TX == TY (got A=%d B=%d TX=%d TY=%d)", p.A, p.B, p.TX, p.TY);
    if ((p.flags & (SIGSVGD_FLAG_Y_IS_X | SIGSVGD_FLAG_SYM)) && want_gradY)
        return bad_arg("gram_long2: Y_IS_X and SYM give the first-slot gradient only (gradY_out must be NULL)");
    return SIGSVGD_OK;
}

// the partial entry points: check_long's for one batch in both slots, and the rank's tiles: tile_offset in [0, tile_stride).
// SIGSVGD_FLAG_EXACT_ADJOINT (gram_long_part_kernel has the GG sweep only) is refused first, under the launch's own name
static int check_long_partial(const LongProblem &p, Form form, const FlagRule &rule, int tile_offset, int tile_stride)
{
    const FlagRule own{"gram_long_sym_partial", 0, 0, rule.not_built & EX, false};
    int rc = check_flags(own, p.flags);
    if (!rc) rc = check_long(p, form, rule, FORWARD);
    if (rc) return rc;
    if (tile_stride < 1 || tile_offset < 0 || tile_offset >= tile_stride)
        return bad_arg("gram_long_sym_partial: bad tile_offset/stride %d/%d", tile_offset, tile_stride);
    return SIGSVGD_OK;
}

// the paired entry points (B = 1: one column of pairs): the pointers, flags and shape under the mode's own name, then
// check_long's remaining conditions
static int check_pair(const LongProblem &p, Form form, const FlagRule &rule, Sweeps sweeps)
{
    if (check_flags(rule, p.flags, sweeps, NOT_BUILT)) return SIGSVGD_E_UNSUPPORTED;
    if (form == LAUNCH && (!p.X || !p.Y || !p.K_out)) return bad_arg("pair: null pointer argument");
    if (check_flags(rule, p.flags, sweeps, UNKNOWN)) return SIGSVGD_E_BADARG;
    if (p.A < 1 || p.TX < 2 || p.TY < 2 || p.d < 1)
        return bad_arg("pair: bad shape A=%d TX=%d TY=%d d=%d (need A, d >= 1 and TX, TY >= 2)", p.A, p.TX, p.TY, p.d);
    return check_long(p, form, rule, sweeps);
}

// the bandwidth entry points, after their mode's own checks: a static kernel that has a bandwidth,
// and for a LAUNCH a place for the derivative
static int check_bandwidth(const char *who, const LongProblem &p, Form form, const void *dK_dinvh_out)
{
    if (!static_kind_radial(p.kind))
        return bad_arg("%s: the linear static kernel has no bandwidth (SIGSVGD_STATIC_RBF, _IMQ, _RQ, _MATERN32 or _MATERN52)", who);
    if (form == LAUNCH && !dK_dinvh_out) return bad_arg("%s: dK_dinvh_out == NULL", who);
    return SIGSVGD_OK;
}

// the distance select's (sqdist_select.hip): the shape, its flags (SIGSVGD_FLAG_Y_IS_X: one batch in both slots)
// and the element count n = A B TX TY, which must stay below 2^63
static int check_select(int A, int B, int TX, int TY, int d, unsigned flags, const FlagRule &rule, unsigned long long *n)
{
    if (A < 1 || B < 1 || TX < 1 || TY < 1 || d < 1)
        return bad_arg("sqdist_select: bad shape A=%d B=%d TX=%d TY=%d d=%d (need all >= 1)", A, B, TX, TY, d);
    if (check_flags(rule, flags)) return SIGSVGD_E_BADARG;
    if ((flags & SIGSVGD_FLAG_Y_IS_X) && (A != B || TX != TY))
        return bad_arg("sqdist_select: Y_IS_X needs A == B and TX == TY (got A=%d B=%d TX=%d TY=%d)", A, B, TX, TY);
    const unsigned __int128 count = (unsigned __int128)((unsigned long long)A * (unsigned long long)B) *
                                    ((unsigned long long)TX * (unsigned long long)TY);
    if (count >> 63) return bad_arg("sqdist_select: A B TX TY = %d x %d x %d x %d elements, 2^63 or more", A, B, TX, TY);
    *n = (unsigned long long)count;
    return SIGSVGD_OK;
}

// ---- roctx ranges around the launches (the tracing hook of this path) ------------------------------
// Enabled with SIGSVGD_ROCTX=1: libroctx64.so is looked up at run time (no link-time dependency), every entry
// point that enqueues work brackets its launches with roctxRangePush/Pop, so `rocprofv3 --marker-trace` shows
// which API call a kernel belongs to.  Off by default: zero cost beyond one branch.
namespace {
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        const char *on = getenv("SIGSVGD_ROCTX");
        if (!on || on[0] == '0') return;
        void *h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
struct Range {
    const Roctx &r;
    explicit Range(const char *name) : r(instance())
    {
        if (r.push) r.push(name);
    }
    ~Range()
    {
        if (r.push) r.pop();
    }
    static const Roctx &instance()
    {
        static Roctx x;
        return x;
    }
};
} // namespace

// ---- which kernel runs a Gram launch (the one place that combines the families' *_supported) ----------
enum class GramRoute { Fast, Quad, Dyad, BandParallel, BandSerial, Generic, GenericPrecise, GenericOneChannel };

// Band kernel schedule.  Band-parallel wins while its workgroups (one pair each) pass through the chip in a few rounds -- its
// wavefronts idle BLAG (nb - 1) phases of every sweep, which other workgroups on the CU fill, but the sum of a pair's wavefront
// time is nb / (1 + BLAG (nb - 1) BGS / (P + 63)) times the serial schedule's.  Measured (Gram + gradient, symmetric, ms,
// parallel / serial): 10 points order 4 (3 bands, 1,280 resident workgroups) -- N = 50 / 70 / 100 / 150: 0.105 / 0.189 /
// 0.364 / 0.78 against 0.125 / 0.205 / 0.424 / 0.737; 30 points order 3 (4 bands, 1,024) -- N = 35 / 60 / 100: 0.138 / 0.317 /
// 0.832 against 0.239 / 0.300 / 0.835.  Rule: at most five rounds with three bands, one and a half with four.  With two bands
// (65 .. 128 cells) it beats the refined-grid kernel of gram_dyad.hip at every size measured (N = 64 .. 400: 20 points order 2
// 0.156 / 0.423 / 1.52 against 0.170 / 0.477 / 1.78; 5 points order 5 0.80 / 3.13 against 0.92 / 3.52): always.
// SIGSVGD_BAND_MODE=serial|parallel (read per launch) overrides it: the tests drive both schedules over the same shapes (serial
// sends grids of up to 128 cells back to gram_dyad.hip).
static bool band_parallel(int A, int B, int T, int d, int n, bool sym)
{
    const char *e = getenv("SIGSVGD_BAND_MODE");
    if (e && e[0] == 's') return false;
    if (e && e[0] == 'p') return true;
    const long long pairs = sym ? (long long)A * (A + 1) / 2 : (long long)A * B;
    const int nb = (((T - 1) << n) + 63) >> 6;
    if (nb <= 2) return true;
    return 2 * pairs <= (nb >= 4 ? 3ll : 10ll) * device_cu_count() * band_wg_per_cu(T, d, n, false);
}

// The kernel of a launch: FORCE_GENERIC first, then the first family in the order below whose shapes hold it.  The fp32-sweep
// families (everything but the coverage kernel) take the RBF static kernel with the second-order solver only; the linear, IMQ
// and rational-quadratic kernels always take the coverage kernel.
// Gram + gradient of paths in ONE channel at dyadic order 0 runs on the coverage kernel with fp64 increments and sweeps (what
// SIGSVGD_FLAG_FORCE_GENERIC does).  Very smooth one-channel paths (|step|^2 / h ~ 1e-5: K = 1 + O(1e-4)) left the gradient of
// the fp32-sweep kernels at 1.2 .. 2.0e-5 of its largest entry (T = 20, 33: register-resident kernel; T = 128: quadrant
// kernel), the coverage kernel at <= 4.2e-6 (tests/test_gpu_precision.py::test_smooth_one_channel_order0).  Forward-only
// launches keep the fp32 route: K is within 1e-6 there.  With Y_IS_X every unordered pair is solved once at any pair count,
// so K is mirrored bit for bit as on the fp32 route.  No reference caller is one-channel; the cost is DESIGN.md section 3.
// Refined grids of 64 .. 128 cells (gram_dyad.hip's shapes) go to the band-parallel schedule from two bands on (65 cells and
// more, r >= 4) and, for one-channel paths, at 64 cells too: their very smooth regime wants the two-float add in both sweeps.
// `partial`: the symmetric partial solve, which has the register-resident and quadrant kernels only (any other route: it does
// not take the launch) and keeps them for one-channel paths.
// SIGSVGD_FLAG_FP32_SWEEPS is the caller's opt-in to the register-resident kernel for the IMQ and
// rational-quadratic kernels with the default stencil at that kernel's shapes -- the one-channel gradient rule first, as for RBF.
// For RBF with the default stencil it is the opt-in to the same kernel's 32-channel layout for paths of 17 to 32 channels
// (fast_wide_supported) -- ordered and Y_IS_X launches only: the partial solve, whose ownership unit
// sigsvgd_gram_sym_tile_rows answers without a flags argument, keeps refusing d > 16.
// In every other case the bit changes nothing: without it every route is what it was.
static GramRoute gram_route(int A, int B, int T, int d, int n, int kind, unsigned flags, int want_grad, bool partial = false)
{
    const bool fp32 = kind == SIGSVGD_STATIC_RBF && !(flags & SIGSVGD_FLAG_NAIVE_SOLVER);
    if (flags & SIGSVGD_FLAG_FORCE_GENERIC) return GramRoute::GenericPrecise;
    if ((flags & SIGSVGD_FLAG_FP32_SWEEPS) && (kind == SIGSVGD_STATIC_IMQ || kind == SIGSVGD_STATIC_RQ) &&
        !(flags & SIGSVGD_FLAG_NAIVE_SOLVER) && fast_supported(T, d, n) && (partial || !(want_grad && d == 1)))
        return GramRoute::Fast;
    if ((flags & SIGSVGD_FLAG_FP32_SWEEPS) && fp32 && !partial && fast_wide_supported(T, d, n)) return GramRoute::Fast;
    // IMQ, the rational quadratic and the Matern kernels have fp64 kernels only and are held to fp64 results: the plan that keeps
    // the increments in fp64 wherever their table (or the per-band layout) fits, what FORCE_GENERIC selects (DESIGN.md sections
    // 5.15, 5.17)
    if (!partial && static_kind_fp64_only(kind)) return GramRoute::GenericPrecise;
    if (!partial && fp32 && want_grad && d == 1 && n == 0 && T >= 3 && T <= 128) return GramRoute::GenericOneChannel;
    if (fp32 && fast_supported(T, d, n)) return GramRoute::Fast;
    if (fp32 && quad_supported(T, d, n)) return GramRoute::Quad;
    if (!fp32 || partial) return GramRoute::Generic;
    const bool sym = (flags & SIGSVGD_FLAG_Y_IS_X) && A == B;
    if (dyad_supported(T, d, n)) {
        const bool band = band_supported(T, d, n) && (((T - 1) << n) > 64 || d == 1) && band_parallel(A, B, T, d, n, sym);
        return band ? GramRoute::BandParallel : GramRoute::Dyad;
    }
    if (band_supported(T, d, n)) return band_parallel(A, B, T, d, n, sym) ? GramRoute::BandParallel : GramRoute::BandSerial;
    return GramRoute::Generic;
}
static GramRoute gram_route(const GramProblem &p, bool partial = false)
{
    return gram_route(p.A, p.B, p.T, p.d, p.n, p.kind, p.flags, p.gradX_out != nullptr, partial);
}

// the workspace plan of a launch on route r; sym: the Y_IS_X orientation
static int route_plan(GramRoute r, int A, int B, int T, int d, int n, int kind, int want_grad, bool sym, WsPlan &w)
{
    switch (r) {
    case GramRoute::Fast: w = fast_plan(A, B, T, d, want_grad, sym, 0, 1, false, kind); return SIGSVGD_OK;
    case GramRoute::Quad: w = quad_plan(A, B, T, d, want_grad, sym); return SIGSVGD_OK;
    case GramRoute::Dyad: w = dyad_plan(A, B, T, d, want_grad, sym); return SIGSVGD_OK;
    case GramRoute::BandParallel: w = band_plan(A, B, T, d, n, want_grad, sym, false); return SIGSVGD_OK;
    case GramRoute::BandSerial: w = band_plan(A, B, T, d, n, want_grad, sym, true); return SIGSVGD_OK;
    case GramRoute::Generic: return generic_plan(A, B, T, d, n, want_grad, sym, false, false, w);
    case GramRoute::GenericPrecise: return generic_plan(A, B, T, d, n, want_grad, sym, true, false, w);
    case GramRoute::GenericOneChannel: return generic_plan(A, B, T, d, n, want_grad, sym, true, true, w);
    }
    return SIGSVGD_E_BADARG;
}

static int dispatch(const GramProblem &p)
{
    switch (gram_route(p)) {
    case GramRoute::Fast: return fast_launch(p);
    case GramRoute::Quad: return quad_launch(p);
    case GramRoute::Dyad: return dyad_launch(p);
    case GramRoute::BandParallel: return band_launch(p, false);
    case GramRoute::BandSerial: return band_launch(p, true);
    case GramRoute::Generic: return generic_launch(p, false, false);
    case GramRoute::GenericPrecise: return generic_launch(p, true, false);
    case GramRoute::GenericOneChannel: return generic_launch(p, true, true);
    }
    return SIGSVGD_E_BADARG;
}

// The bytes sigsvgd_gram_workspace_bytes reports for launches without SIGSVGD_FLAG_NORMALIZED_FUSED: the largest plan of the
// launches these arguments can reach (the rule of include/sigsvgd_hip.h): with Y_IS_X and A == B the symmetric launch and --
// gradient queries -- the symmetric partial solve of the shape; otherwise the ordered launch and, when A == B, the symmetric one.
static int gram_workspace(int A, int B, int T, int d, int n, int kind, int want_grad, unsigned flags, size_t *bytes)
{
    size_t most = 0;
    auto cover = [&](bool sym, bool partial) {
        const unsigned f = sym ? flags | SIGSVGD_FLAG_Y_IS_X : flags & ~SIGSVGD_FLAG_Y_IS_X;
        const GramRoute r = gram_route(A, B, T, d, n, kind, f, want_grad, partial);
        if (partial && r != GramRoute::Fast && r != GramRoute::Quad) return (int)SIGSVGD_OK; // (not a partial-solve shape)
        WsPlan w;
        const int rc = route_plan(r, A, B, T, d, n, kind, want_grad, sym, w);
        if (w.total() > most) most = w.total();
        return rc;
    };
    const bool yx = (flags & SIGSVGD_FLAG_Y_IS_X) && A == B;
    int rc = cover(yx, false);
    if (!rc && !yx && A == B) rc = cover(true, false);
    if (!rc && yx && want_grad) rc = cover(true, true);
    if (rc) return rc;
    *bytes = most;
    return SIGSVGD_OK;
}

// ---- SIGSVGD_FLAG_NORMALIZED_FUSED: the normalised kernel around an unchanged fused launch ---------
// The workspace of such a launch, from its 256-B aligned base: the unflagged launch's whole workspace (what gram_workspace
// reports for the flags without the bit), the diagonals' logarithms double[A] and, unless yx, double[B], the diagonal pass's
// scratch (the larger of the two passes'), and for a gradient launch the weights W' [A][B] (sized for fp64 I/O: the query has
// no dtype), the fp64 diagonal gradients [A][T][d] and the sums [A]; each padded to 256 B, then the slack of aligning.
struct NormFusedPlan {
    size_t inner = 0, logs = 0, scratch = 0, weights = 0, diag = 0, sums = 0;
    size_t total() const { return inner + logs + scratch + weights + diag + sums + 256; }
};
static int norm_fused_plan(int A, int B, int T, int d, int n, int kind, int want_grad, unsigned flags, NormFusedPlan &np)
{
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const bool yx = (flags & SIGSVGD_FLAG_Y_IS_X) && A == B;
    size_t inner = 0, sx = 0, sy = 0;
    int rc = gram_workspace(A, B, T, d, n, kind, want_grad, flags & ~SIGSVGD_FLAG_NORMALIZED_FUSED, &inner);
    if (!rc) rc = norm_diag_workspace(A, T, d, n, want_grad, &sx);
    if (!rc && !yx) rc = norm_diag_workspace(B, T, d, n, 0, &sy);
    if (rc) return rc;
    np.inner = pad(inner);
    np.logs = pad(((size_t)A + (yx ? 0 : (size_t)B)) * sizeof(double));
    np.scratch = pad(sx > sy ? sx : sy);
    if (want_grad) {
        np.weights = pad((size_t)A * B * sizeof(double));
        np.diag = pad((size_t)A * T * d * sizeof(double));
        np.sums = pad((size_t)A * sizeof(double));
    }
    return SIGSVGD_OK;
}

// The launch, all on p's stream, no host synchronisation, no allocation: the diagonal pass on (X, X) -- with the gradient of
// ln K(X_i, X_i) for a gradient launch -- and, unless yx, forward only on (Y, Y); W' = w s (SYM applied there: the inner
// launch runs without the bit, s_ij is not s_ji between two batches); the unflagged launch dispatch(p) on whatever route
// gram_route picks, with grad_out = W'; the finish kernel over K_out and gradX_out in place.  Every refusal -- the shape's, the
// diagonal plan's, the workspace's -- comes from the plan, before any device work.
static int gram_norm_fused(const GramProblem &p)
{
    const bool yx = (p.flags & SIGSVGD_FLAG_Y_IS_X) != 0, sym = (p.flags & SIGSVGD_FLAG_SYM) != 0;
    const bool grad = p.gradX_out != nullptr;
    if (yx && p.A != p.B) return bad_arg("gram_norm_fused: Y_IS_X needs A == B");
    NormFusedPlan np;
    int rc = norm_fused_plan(p.A, p.B, p.T, p.d, p.n, p.kind, grad, p.flags, np);
    if (rc) return rc;
    if (p.ws_bytes < np.total() || !p.ws) {
        set_error("gram_norm_fused: workspace %zu B too small, required %zu B", p.ws_bytes, np.total());
        return SIGSVGD_E_WORKSPACE;
    }
    unsigned char *base = reinterpret_cast<unsigned char *>((reinterpret_cast<uintptr_t>(p.ws) + 255) & ~(uintptr_t)255);
    double *lnA = reinterpret_cast<double *>(base + np.inner), *lnB = yx ? lnA : lnA + p.A;
    unsigned char *scratch = base + np.inner + np.logs;
    void *W = scratch + np.scratch;
    double *diag = reinterpret_cast<double *>(scratch + np.scratch + np.weights);
    double *sums = reinterpret_cast<double *>(scratch + np.scratch + np.weights + np.diag);

    LongProblem q{p.X, p.X, p.A, 1, p.T, p.T, p.d, p.dtype, p.inv_h, p.n, p.kind, 0u, nullptr, nullptr, nullptr, nullptr,
                  scratch, np.scratch, p.stream};
    rc = norm_diag_launch(q, lnA, grad ? diag : nullptr);
    if (!rc && !yx) {
        q.X = q.Y = p.Y;
        q.A = p.B;
        rc = norm_diag_launch(q, lnB, nullptr);
    }
    if (rc) return rc;
    GramProblem in = p;
    in.flags &= ~(unsigned)(SIGSVGD_FLAG_NORMALIZED_FUSED | SIGSVGD_FLAG_SYM);
    in.ws = base;
    in.ws_bytes = np.inner;
    if (grad) {
        const hipError_t e = norm_fused_weights(p.dtype, p.grad_out, lnA, lnB, W, p.A, p.B, sym, yx, p.stream);
        if (e != hipSuccess) return hip_fail(e, "launch norm_fused_weights_kernel");
        in.grad_out = W;
    }
    rc = dispatch(in);
    if (rc) return rc;
    const hipError_t e = norm_fused_finish(p.dtype, p.K_out, p.grad_out, lnA, lnB, p.A, p.B, sym, yx, p.gradX_out, diag, sums,
                                           p.T * p.d, p.stream);
    return e != hipSuccess ? hip_fail(e, "launch norm_fused_finish_kernel") : SIGSVGD_OK;
}

} // namespace sigsvgd

using namespace sigsvgd;

extern "C" {

int sigsvgd_abi_version(void) { return SIGSVGD_ABI_VERSION; }

const char *sigsvgd_last_error(void) { return g_err; }

int sigsvgd_gram_workspace_bytes(int A, int B, int T, int d, int dyadic_order, int static_kind, int want_grad,
                                 unsigned flags, size_t *bytes)
{
    if (no_bytes(bytes)) return SIGSVGD_E_BADARG;
    if (!static_kind_known(static_kind)) return bad_arg("bad static kernel kind %d", static_kind);
    if (check_flags(kGramQuery, flags)) return SIGSVGD_E_UNSUPPORTED;
    if (!(flags & SIGSVGD_FLAG_NORMALIZED_FUSED))
        return gram_workspace(A, B, T, d, dyadic_order, static_kind, want_grad, flags, bytes);
    if (A < 1 || B < 1 || T < 2 || d < 1 || dyadic_order < 0 || dyadic_order > 10)
        return bad_arg("bad shape A=%d B=%d T=%d d=%d order %d (need A,B,d >= 1, T >= 2 and 0 <= order <= 10)", A, B, T, d,
                       dyadic_order);
    NormFusedPlan np;
    const int rc = norm_fused_plan(A, B, T, d, dyadic_order, static_kind, want_grad ? 1 : 0, flags, np);
    if (rc) return rc;
    *bytes = np.total();
    return SIGSVGD_OK;
}

int sigsvgd_gram_fwd(const void *X, const void *Y, int A, int B, int T, int d, int dtype, double inv_h,
                     int dyadic_order, int static_kind, unsigned flags, void *K_out, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    int rc = check_common(X, Y, A, B, T, d, dtype, inv_h, dyadic_order, static_kind, flags, K_out);
    if (rc) return rc;
    GramProblem p{X, Y, A, B, T, d, dtype, inv_h, dyadic_order, static_kind, flags, nullptr,
                  K_out, nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    if (check_flags(kGramFwd, flags)) return SIGSVGD_E_UNSUPPORTED;
    Range range("sigsvgd_gram_fwd");
    if (flags & SIGSVGD_FLAG_NORMALIZED_FUSED) return gram_norm_fused(p);
    return dispatch(p);
}

int sigsvgd_gram_fwd_bwd(const void *X, const void *Y, int A, int B, int T, int d, int dtype, double inv_h,
                         int dyadic_order, int static_kind, unsigned flags, const void *grad_out, void *K_out,
                         void *gradX_out, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_common(X, Y, A, B, T, d, dtype, inv_h, dyadic_order, static_kind, flags, K_out);
    if (rc) return rc;
    if (!gradX_out) return bad_arg("gradX_out == NULL (use sigsvgd_gram_fwd for forward only)");
    if ((flags & SIGSVGD_FLAG_Y_IS_X) && A != B) return bad_arg("Y_IS_X needs A == B");
    if (check_flags(kGramFwdBwd, flags)) return SIGSVGD_E_UNSUPPORTED;
    GramProblem p{X, Y, A, B, T, d, dtype, inv_h, dyadic_order, static_kind, flags, grad_out,
                  K_out, gradX_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    Range range("sigsvgd_gram_fwd_bwd");
    if (flags & SIGSVGD_FLAG_NORMALIZED_FUSED) return gram_norm_fused(p);
    return dispatch(p);
}

int sigsvgd_gram_sym_partial(const void *X, int N, int T, int d, int dtype, double inv_h, int static_kind,
                             unsigned flags, int tile_offset, int tile_stride, const void *grad_out,
                             void *K_partial, double *grad_partial, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    int rc = check_common(X, X, N, N, T, d, dtype, inv_h, 0, static_kind, flags, K_partial);
    if (rc) return rc;
    if (!grad_partial) return bad_arg("grad_partial == NULL");
    if (check_flags(kSymPartial, flags)) return SIGSVGD_E_UNSUPPORTED;
    GramProblem p{X, X, N, N, T, d, dtype, inv_h, 0, static_kind, flags | SIGSVGD_FLAG_Y_IS_X, grad_out,
                  K_partial, grad_partial, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    const GramRoute r = gram_route(p, true);
    if (r != GramRoute::Fast && r != GramRoute::Quad) {
        set_error("sym_partial: shape/kernel outside the register-resident and quadrant kernels (need 3<=T<=128, d<=16 and RBF, or "
                  "3<=T<=64, d<=16 and IMQ / rational quadratic with SIGSVGD_FLAG_FP32_SWEEPS)");
        return SIGSVGD_E_UNSUPPORTED;
    }
    if (tile_stride < 1 || tile_offset < 0 || tile_offset >= tile_stride)
        return bad_arg("sym_partial: bad tile_offset/stride %d/%d", tile_offset, tile_stride);
    Range range("sigsvgd_gram_sym_partial");
    const bool fold = (flags & SIGSVGD_FLAG_FOLD_TILES) != 0;
    return r == GramRoute::Fast ? fast_sym_partial(p, tile_offset, tile_stride, fold, grad_partial)
                                : quad_sym_partial(p, tile_offset, tile_stride, fold, grad_partial);
}

int sigsvgd_gram_sym_tile_rows(int T, int d)
{
    switch (gram_route(1, 1, T, d, 0, SIGSVGD_STATIC_RBF, SIGSVGD_FLAG_Y_IS_X, 1, true)) {
    case GramRoute::Fast: return sym_tile_rows_fast(T, d);
    case GramRoute::Quad: return 8;
    default: return 0;
    }
}

int sigsvgd_svgd_phi(const float *K, const float *score, const float *grad_k, const float *mask, int N, int D,
                     float *v_out, const float *X_in, float *X_out, float lr, void *stream)
{
    Range range("sigsvgd_svgd_phi");
    return phi_launch(K, score, grad_k, mask, N, D, v_out, X_in, X_out, lr, nullptr, static_cast<hipStream_t>(stream));
}

int sigsvgd_svgd_step(const float *K, const float *score, const float *grad_k, const float *mask, int N, int D,
                      float *v_out, const float *X_in, float *X_out, float lr, float *adagrad_state, void *stream)
{
    Range range("sigsvgd_svgd_step");
    return phi_launch(K, score, grad_k, mask, N, D, v_out, X_in, X_out, lr, adagrad_state,
                      static_cast<hipStream_t>(stream));
}

int sigsvgd_svgd_adam_step(const float *K, const float *score, const float *grad_k, const float *mask, int N, int D,
                           float *v_out, const float *X_in, float *X_out, double lr, double beta1, double beta2, double eps,
                           float *exp_avg, float *exp_avg_sq, int *step_dev, void *stream)
{
    if (!exp_avg || !exp_avg_sq || !step_dev || !X_in || !X_out)
        return bad_arg("svgd_adam_step: null state / particle pointer");
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0))
        return bad_arg("svgd_adam_step: bad hyper-parameters beta1=%g beta2=%g eps=%g", beta1, beta2, eps);
    Range range("sigsvgd_svgd_adam_step");
    return phi_launch(K, score, grad_k, mask, N, D, v_out, X_in, X_out, (float)lr, nullptr,
                      static_cast<hipStream_t>(stream), exp_avg, exp_avg_sq, step_dev, lr, beta1, beta2, (float)eps);
}

int sigsvgd_svgd_update(const float *v_in, const float *mask, int N, int D, float *v_out, const float *X_in, float *X_out,
                        double lr, float *adagrad_state, float *exp_avg, float *exp_avg_sq, int *step_dev, double beta1,
                        double beta2, double eps, void *stream)
{
    if ((exp_avg || exp_avg_sq || step_dev) && !(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0))
        return bad_arg("svgd_update: bad hyper-parameters beta1=%g beta2=%g eps=%g", beta1, beta2, eps);
    Range range("sigsvgd_svgd_update");
    return update_launch(v_in, mask, N, D, v_out, X_in, X_out, (float)lr, adagrad_state, static_cast<hipStream_t>(stream),
                         exp_avg, exp_avg_sq, step_dev, lr, beta1, beta2, (float)eps);
}

int sigsvgd_vec_sqdist(const void *X, const void *Y, const void *XM, const void *YM, int A, int B, int D, int dtype,
                       void *sq_out, void *stream)
{
    if (!X || !Y || !sq_out || (XM == nullptr) != (YM == nullptr))
        return bad_arg("vec_sqdist: null pointer argument (XM and YM must both be given or both be NULL)");
    if (A < 1 || B < 1 || D < 1 || (dtype != SIGSVGD_F32 && dtype != SIGSVGD_F64))
        return bad_arg("vec_sqdist: bad arguments A=%d B=%d D=%d dtype=%d", A, B, D, dtype);
    return vec_sqdist_launch(X, Y, XM, YM, A, B, D, dtype, sq_out, static_cast<hipStream_t>(stream));
}

int sigsvgd_vec_fused_workspace_bytes(int A, int B, int D, size_t *bytes)
{
    if (!bytes || A < 1 || B < 1 || D < 1)
        return bad_arg("vec_fused_workspace_bytes: bad arguments A=%d B=%d D=%d", A, B, D);
    *bytes = vec_fused_workspace_bytes(A, B, D);
    return SIGSVGD_OK;
}

int sigsvgd_vec_kernel_fused(const void *X, const void *Y, const void *XM, const void *YM, const void *grad_out, int A,
                             int B, int D, int dtype, int kind, double inv_h2, double grad_scale, void *K_out,
                             void *dK_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!X || !Y || (!K_out && !dK_out) || (XM == nullptr) != (YM == nullptr))
        return bad_arg("vec_kernel_fused: null pointer argument (XM and YM must both be given or both be NULL)");
    if (A < 1 || B < 1 || D < 1 || (dtype != SIGSVGD_F32 && dtype != SIGSVGD_F64))
        return bad_arg("vec_kernel_fused: bad arguments A=%d B=%d D=%d dtype=%d", A, B, D, dtype);
    if (kind != SIGSVGD_VEC_GAUSSIAN && kind != SIGSVGD_VEC_IMQ && kind != SIGSVGD_VEC_UNIT)
        return bad_arg("vec_kernel_fused: bad kind %d", kind);
    if (!vec_fused_supported(D, dtype)) {
        set_error("vec_kernel_fused: fp32 with D <= 512 only (got dtype=%d D=%d); use sigsvgd_vec_sqdist + sigsvgd_vec_kernel",
                  dtype, D);
        return SIGSVGD_E_UNSUPPORTED;
    }
    Range range("sigsvgd_vec_kernel_fused");
    return vec_fused_launch(X, Y, XM, YM, grad_out, A, B, D, kind, inv_h2, grad_scale, K_out, dK_out, workspace, workspace_bytes,
                            static_cast<hipStream_t>(stream));
}

int sigsvgd_vec_kernel(const void *sq, const void *XM, const void *YM, const void *grad_out, int A, int B, int D,
                       int dtype, int kind, double inv_h2, double grad_scale, void *K_out, void *dK_out, void *stream)
{
    if (!sq || (!K_out && !dK_out) || (dK_out && (!XM || !YM))) return bad_arg("vec_kernel: null pointer argument");
    if (A < 1 || B < 1 || D < 1 || (dtype != SIGSVGD_F32 && dtype != SIGSVGD_F64))
        return bad_arg("vec_kernel: bad arguments A=%d B=%d D=%d dtype=%d", A, B, D, dtype);
    if (kind != SIGSVGD_VEC_GAUSSIAN && kind != SIGSVGD_VEC_IMQ && kind != SIGSVGD_VEC_UNIT)
        return bad_arg("vec_kernel: bad kind %d", kind);
    if (kind == SIGSVGD_VEC_UNIT && (K_out || !dK_out))
        return bad_arg("vec_kernel: SIGSVGD_VEC_UNIT computes only dK_out (K_out must be NULL)");
    if (kind != SIGSVGD_VEC_UNIT && !(inv_h2 > 0.0)) return bad_arg("vec_kernel: needs 1/h^2 > 0 (got %g)", inv_h2);
    return vec_kgrad_launch(sq, XM, YM, grad_out, A, B, D, dtype, kind, inv_h2, grad_scale, K_out, dK_out,
                            static_cast<hipStream_t>(stream));
}

int sigsvgd_obstacle_cost(const float *x, int N, int knots, int d, const float *start, const float *target,
                          const float *basis, int samples, const float *log_weights, const float *mean, const float *std,
                          int components, float w_obstacle, float w_length, float *cost, float *traj, float *grad_x,
                          void *stream)
{
    Range range("sigsvgd_obstacle_cost");
    return obstacle_cost_launch(x, N, knots, d, start, target, basis, samples, log_weights, mean, std, components,
                                w_obstacle, w_length, cost, traj, grad_x, static_cast<hipStream_t>(stream));
}

int sigsvgd_signature(const void *X, int N, int L, int C, int depth, int basepoint, int dtype, void *out,
                      long long *channels, void *stream)
{
    if (N < 1 || L < 1 || C < 1 || depth < 1 || (dtype != SIGSVGD_F32 && dtype != SIGSVGD_F64))
        return bad_arg("signature: bad arguments N=%d L=%d C=%d depth=%d dtype=%d", N, L, C, depth, dtype);
    const long long ch = signature_channels(C, depth);
    if (ch < 0) {
        set_error("signature: C=%d depth=%d overflows", C, depth);
        return SIGSVGD_E_UNSUPPORTED;
    }
    if (channels) *channels = ch;
    if (!out) {
        if (channels) return SIGSVGD_OK;
        return bad_arg("signature: out == NULL and channels == NULL");
    }
    if (!X) return bad_arg("signature: X == NULL");
    return signature_launch(X, N, L, C, depth, basepoint, dtype, out, static_cast<hipStream_t>(stream));
}

int sigsvgd_signature_backward(const void *X, const void *grad_sig, int N, int L, int C, int depth, int basepoint, int dtype,
                               void *grad_X, void *stream)
{
    if (N < 1 || L < 1 || C < 1 || depth < 1 || (dtype != SIGSVGD_F32 && dtype != SIGSVGD_F64))
        return bad_arg("signature_backward: bad arguments N=%d L=%d C=%d depth=%d dtype=%d", N, L, C, depth, dtype);
    if (!X || !grad_sig || !grad_X) return bad_arg("signature_backward: null pointer argument");
    const long long ch = signature_channels(C, depth);
    if (ch < 0) {
        set_error("signature_backward: C=%d depth=%d overflows", C, depth);
        return SIGSVGD_E_UNSUPPORTED;
    }
    Range range("sigsvgd_signature_backward");
    return signature_bwd_launch(X, grad_sig, N, L, C, depth, basepoint, dtype, grad_X, ch, static_cast<hipStream_t>(stream));
}

int sigsvgd_pde_workspace_bytes(int npairs, int M, int N, int dyadic_order, int want_grad, unsigned flags, size_t *bytes)
{
    if (no_bytes(bytes)) return SIGSVGD_E_BADARG;
    const int rc = check_pde(npairs, M, N, SIGSVGD_F64, dyadic_order, flags, kPde, reverse_if(want_grad));
    if (rc) return rc;
    return pde_workspace(npairs, M, N, dyadic_order, want_grad ? 1 : 0, bytes);
}

int sigsvgd_pde_fwd(const void *G, int npairs, int M, int N, int dtype, int dyadic_order, unsigned flags, void *K_out,
                    void *workspace, size_t workspace_bytes, void *stream)
{
    if (!G || !K_out) return bad_arg("pde_fwd: null pointer argument");
    const int rc = check_pde(npairs, M, N, dtype, dyadic_order, flags, kPde, FORWARD);
    if (rc) return rc;
    Range range("sigsvgd_pde_fwd");
    return pde_launch(G, npairs, M, N, dtype, dyadic_order, (flags & SIGSVGD_FLAG_NAIVE_SOLVER) != 0, false, nullptr, K_out,
                      nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int sigsvgd_pde_fwd_bwd(const void *G, int npairs, int M, int N, int dtype, int dyadic_order, unsigned flags,
                        const void *grad_out, void *K_out, void *dG_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!G || !K_out || !dG_out) return bad_arg("pde_fwd_bwd: null pointer argument");
    const int rc = check_pde(npairs, M, N, dtype, dyadic_order, flags, kPde, REVERSE);
    if (rc) return rc;
    Range range("sigsvgd_pde_fwd_bwd");
    return pde_launch(G, npairs, M, N, dtype, dyadic_order, (flags & SIGSVGD_FLAG_NAIVE_SOLVER) != 0,
                      (flags & SIGSVGD_FLAG_EXACT_ADJOINT) != 0, grad_out, K_out, dG_out, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream));
}

// ---- the long-path route (gram_long.hip): each entry point fills one LongProblem, checks it and hands it on ----------------
// (a workspace or plan query fills the shape, order, kind and flags)
int sigsvgd_gram_long_workspace_bytes(int A, int B, int TX, int TY, int d, int dyadic_order, int static_kind, int want_grad,
                                      unsigned flags, size_t *bytes)
{
    if (no_bytes(bytes)) return SIGSVGD_E_BADARG;
    const LongProblem p{nullptr, nullptr, A, B, TX, TY, d, SIGSVGD_F32, 0.0, dyadic_order, static_kind, flags};
    const int rc = check_long(p, QUERY, kLong, reverse_if(want_grad));
    if (rc) return rc;
    return long_workspace(p, want_grad ? 1 : 0, bytes);
}

int sigsvgd_gram_long_fwd(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, double inv_h,
                          int dyadic_order, int static_kind, unsigned flags, void *K_out, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    const LongProblem p{X, Y, A, B, TX, TY, d, dtype, inv_h, dyadic_order, static_kind, flags, nullptr, K_out, nullptr, nullptr,
                        workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    const int rc = check_long(p, LAUNCH, kLong, FORWARD);
    if (rc) return rc;
    Range range("sigsvgd_gram_long_fwd");
    return long_launch(p);
}

int sigsvgd_gram_long_fwd_bwd(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, double inv_h,
                              int dyadic_order, int static_kind, unsigned flags, const void *grad_out, void *K_out,
                              void *gradX_out, void *workspace, size_t workspace_bytes, void *stream)
{
    const LongProblem p{X, Y, A, B, TX, TY, d, dtype, inv_h, dyadic_order, static_kind, flags, grad_out, K_out, gradX_out,
                        nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    const int rc = check_long(p, LAUNCH, kLong, REVERSE);
    if (rc) return rc;
    if (!gradX_out) return bad_arg("gradX_out == NULL (use sigsvgd_gram_long_fwd for forward only)");
    Range range("sigsvgd_gram_long_fwd_bwd");
    return long_launch(p);
}

int sigsvgd_pair_workspace_bytes(int A, int TX, int TY, int d, int dyadic_order, int static_kind, int want_grad,
                                 unsigned flags, size_t *bytes)
{
    if (no_bytes(bytes)) return SIGSVGD_E_BADARG;
    const LongProblem p{nullptr, nullptr, A, 1, TX, TY, d, SIGSVGD_F32, 0.0, dyadic_order, static_kind, flags};
    const int rc = check_pair(p, QUERY, kPair, reverse_if(want_grad));
    if (rc) return rc;
    return pair_workspace(p, want_grad ? 1 : 0, bytes);
}

int sigsvgd_pair_schedule(int A, int TX, int TY, int d, int dyadic_order, int static_kind, int want_grad, unsigned flags,
                          int *waves_per_pair, int *grid, size_t *lds_bytes)
{
    if (!waves_per_pair || !grid || !lds_bytes) return bad_arg("pair: schedule query without a place for its answer");
    const LongProblem p{nullptr, nullptr, A, 1, TX, TY, d, SIGSVGD_F32, 0.0, dyadic_order, static_kind, flags};
    const int rc = check_pair(p, QUERY, kPair, reverse_if(want_grad));
    if (rc) return rc;
    return pair_schedule(p, want_grad ? 1 : 0, waves_per_pair, grid, lds_bytes);
}

int sigsvgd_pair_fwd(const void *X, const void *Y, int A, int TX, int TY, int d, int dtype, double inv_h,
                     int dyadic_order, int static_kind, unsigned flags, void *K_out, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    const LongProblem p{X, Y, A, 1, TX, TY, d, dtype, inv_h, dyadic_order, static_kind, flags, nullptr, K_out, nullptr, nullptr,
                        workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    const int rc = check_pair(p, LAUNCH, kPair, FORWARD);
    if (rc) return rc;
    Range range("sigsvgd_pair_fwd");
    return pair_launch(p);
}

int sigsvgd_pair_fwd_bwd(const void *X, const void *Y, int A, int TX, int TY, int d, int dtype, double inv_h,
                         int dyadic_order, int static_kind, unsigned flags, const void *grad_out, void *K_out,
                         void *gradX_out, void *gradY_out, void *workspace, size_t workspace_bytes, void *stream)
{
    const LongProblem p{X, Y, A, 1, TX, TY, d, dtype, inv_h, dyadic_order, static_kind, flags, grad_out, K_out, gradX_out,
                        gradY_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    const int rc = check_pair(p, LAUNCH, kPair, REVERSE);
    if (rc) return rc;
    if (!gradX_out && !gradY_out)
        return bad_arg("pair: gradX_out and gradY_out both NULL (use sigsvgd_pair_fwd for forward only)");
    Range range("sigsvgd_pair_fwd_bwd");
    return pair_launch(p);
}

int sigsvgd_gram_long2_workspace_bytes(int A, int B, int TX, int TY, int d, int dyadic_order, int static_kind,
                                       int want_gradX, int want_gradY, unsigned flags, size_t *bytes)
{
    if (no_bytes(bytes)) return SIGSVGD_E_BADARG;
    const LongProblem p{nullptr, nullptr, A, B, TX, TY, d, SIGSVGD_F32, 0.0, dyadic_order, static_kind, flags};
    const int rc = check_long2(p, QUERY, kLong2, reverse_if(want_gradX || want_gradY), want_gradY != 0);
    if (rc) return rc;
    return long2_workspace(p, want_gradX ? 1 : 0, want_gradY ? 1 : 0, bytes);
}

int sigsvgd_gram_long_fwd_bwd2(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, double inv_h,
                               int dyadic_order, int static_kind, unsigned flags, const void *grad_out, void *K_out,
                               void *gradX_out, void *gradY_out, void *workspace, size_t workspace_bytes, void *stream)
{
    const LongProblem p{X, Y, A, B, TX, TY, d, dtype, inv_h, dyadic_order, static_kind, flags, grad_out, K_out, gradX_out,
                        gradY_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    const int rc = check_long2(p, LAUNCH, kLong2, reverse_if(gradX_out || gradY_out), gradY_out != nullptr);
    if (rc) return rc;
    Range range("sigsvgd_gram_long_fwd_bwd2");
    return long2_launch(p);
}

int sigsvgd_gram_long_h_workspace_bytes(int A, int B, int TX, int TY, int d, int dyadic_order, int static_kind,
                                        int want_gradX, int want_gradY, unsigned flags, size_t *bytes)
{
    if (no_bytes(bytes)) return SIGSVGD_E_BADARG;
    const LongProblem p{nullptr, nullptr, A, B, TX, TY, d, SIGSVGD_F32, 0.0, dyadic_order, static_kind, flags};
    int rc = check_long2(p, QUERY, kLongH, REVERSE, want_gradY != 0); // (the launch always runs the reverse sweep)
    if (!rc) rc = check_bandwidth("gram_long_h", p, QUERY, nullptr);
    if (rc) return rc;
    return long2_h_workspace(p, want_gradX ? 1 : 0, want_gradY ? 1 : 0, bytes);
}

int sigsvgd_gram_long_fwd_bwd_h(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, double inv_h,
                                int dyadic_order, int static_kind, unsigned flags, const void *grad_out, void *K_out,
                                void *gradX_out, void *gradY_out, void *dK_dinvh_out, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    const LongProblem p{X, Y, A, B, TX, TY, d, dtype, inv_h, dyadic_order, static_kind, flags, grad_out, K_out, gradX_out,
                        gradY_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    int rc = check_long2(p, LAUNCH, kLongH, REVERSE, gradY_out != nullptr);
    if (!rc) rc = check_bandwidth("gram_long_h", p, LAUNCH, dK_dinvh_out);
    if (rc) return rc;
    Range range("sigsvgd_gram_long_fwd_bwd_h");
    return long2_h_launch(p, dK_dinvh_out);
}

int sigsvgd_pair_h_workspace_bytes(int A, int TX, int TY, int d, int dyadic_order, int static_kind, unsigned flags,
                                   size_t *bytes)
{
    if (no_bytes(bytes)) return SIGSVGD_E_BADARG;
    const LongProblem p{nullptr, nullptr, A, 1, TX, TY, d, SIGSVGD_F32, 0.0, dyadic_order, static_kind, flags};
    int rc = check_pair(p, QUERY, kPairH, REVERSE);
    if (!rc) rc = check_bandwidth("pair_h", p, QUERY, nullptr);
    if (rc) return rc;
    return pair_workspace(p, 1, bytes); // (the launch always runs the reverse sweep)
}

int sigsvgd_pair_fwd_bwd_h(const void *X, const void *Y, int A, int TX, int TY, int d, int dtype, double inv_h,
                           int dyadic_order, int static_kind, unsigned flags, const void *grad_out, void *K_out,
                           void *gradX_out, void *gradY_out, void *dK_dinvh_out, void *workspace, size_t workspace_bytes,
                           void *stream)
{
    const LongProblem p{X, Y, A, 1, TX, TY, d, dtype, inv_h, dyadic_order, static_kind, flags, grad_out, K_out, gradX_out,
                        gradY_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    int rc = check_pair(p, LAUNCH, kPairH, REVERSE);
    if (!rc) rc = check_bandwidth("pair_h", p, LAUNCH, dK_dinvh_out);
    if (rc) return rc;
    Range range("sigsvgd_pair_fwd_bwd_h");
    return pair_h_launch(p, dK_dinvh_out);
}

int sigsvgd_gram_long_partial_plan(int N, int T, int d, int dyadic_order, int static_kind, unsigned flags, int tile_stride,
                                   int *tile_rows, int *tile_cols)
{
    if (!tile_rows || !tile_cols) return bad_arg("gram_long_partial_plan: tile_rows / tile_cols == NULL");
    const LongProblem p{nullptr, nullptr, N, N, T, T, d, SIGSVGD_F32, 0.0, dyadic_order, static_kind, flags};
    const int rc = check_long_partial(p, QUERY, kLongPartial, 0, tile_stride);
    if (rc) return rc;
    return long_part_tiles(p, tile_stride, tile_rows, tile_cols);
}

int sigsvgd_gram_long_partial_workspace_bytes(int N, int T, int d, int dyadic_order, int static_kind, unsigned flags,
                                              int tile_offset, int tile_stride, size_t *bytes)
{
    if (no_bytes(bytes)) return SIGSVGD_E_BADARG;
    const LongProblem p{nullptr, nullptr, N, N, T, T, d, SIGSVGD_F32, 0.0, dyadic_order, static_kind, flags};
    const int rc = check_long_partial(p, QUERY, kLongPartial, tile_offset, tile_stride);
    if (rc) return rc;
    return long_part_workspace(p, tile_offset, tile_stride, bytes);
}

int sigsvgd_gram_long_sym_partial(const void *X, int N, int T, int d, int dtype, double inv_h, int dyadic_order,
                                  int static_kind, unsigned flags, int tile_offset, int tile_stride, const void *grad_out,
                                  void *K_partial, double *grad_partial, void *workspace, size_t workspace_bytes, void *stream)
{
    const LongProblem p{X, X, N, N, T, T, d, dtype, inv_h, dyadic_order, static_kind, flags, grad_out, K_partial, grad_partial,
                        nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    const int rc = check_long_partial(p, LAUNCH, kLongPartial, tile_offset, tile_stride);
    if (rc) return rc;
    if (!grad_partial) return bad_arg("gram_long_sym_partial: grad_partial == NULL");
    Range range("sigsvgd_gram_long_sym_partial");
    return long_part_launch(p, tile_offset, tile_stride);
}

// ---- the distance select (sqdist_select.hip) ------------------------------------------------------------------------------
int sigsvgd_sqdist_select_workspace_bytes(int A, int B, int TX, int TY, int d, unsigned flags, size_t *bytes)
{
    if (no_bytes(bytes)) return SIGSVGD_E_BADARG;
    unsigned long long n = 0;
    const int rc = check_select(A, B, TX, TY, d, flags, kSelect, &n);
    if (rc) return rc;
    *bytes = select_workspace_bytes();
    return SIGSVGD_OK;
}

int sigsvgd_sqdist_select(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, unsigned flags,
                          unsigned long long rank, double *out_device, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!X || !Y || !out_device) return bad_arg("sqdist_select: null pointer argument");
    unsigned long long n = 0;
    const int rc = check_select(A, B, TX, TY, d, flags, kSelect, &n);
    if (rc) return rc;
    if (dtype != SIGSVGD_F32 && dtype != SIGSVGD_F64) return bad_arg("sqdist_select: bad dtype %d", dtype);
    if (rank >= n) return bad_arg("sqdist_select: rank %llu outside the %llu elements", rank, n);
    Range range("sigsvgd_sqdist_select");
    return select_launch(X, Y, A, B, TX, TY, d, dtype, flags, rank, n, out_device, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream));
}

} // extern "C"
