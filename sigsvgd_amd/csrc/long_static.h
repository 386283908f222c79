// The built-in static kernels of the long-path route (DESIGN.md sections 5.10, 5.15, 5.17), shared by the kernels of gram_long.hip
// and pair_bands.hip: the kernel's value at a point of X (LDS, fp64) and a point of Y, the gradient pass that chains a
// pair's coarse S through the static kernel's derivative, and the pass that chains it through the kernel's derivative in the
// bandwidth (gram_long.hip only).
#pragma once

#include "ring_sweep.h"

namespace sigsvgd {
namespace {
// The radial kinds beside RBF: k = phi(s), s = |x - y|^2 inv_h.  radial_phi: phi(s); radial_slope:
// -phi'(s), which takes the place of RBF's exp(-s) in the gradient contraction (IMQ: k^3 / 2, rational quadratic: k^2).
// (the Matern kinds, DESIGN.md section 5.17: kMaternKind, matern_u, matern_phi and matern_slope of sig_common.h)
template <int KIND>
inline constexpr bool kRadialKind = KIND == SIGSVGD_STATIC_IMQ || KIND == SIGSVGD_STATIC_RQ || kMaternKind<KIND>;
template <int KIND>
__device__ __forceinline__ double radial_phi(double s)
{
    if constexpr (kMaternKind<KIND>) return matern_phi(KIND == SIGSVGD_STATIC_MATERN32, matern_u(KIND == SIGSVGD_STATIC_MATERN32, s));
    return KIND == SIGSVGD_STATIC_IMQ ? rsqrt(1.0 + s) : 1.0 / (1.0 + s);
}
template <int KIND>
__device__ __forceinline__ double radial_slope(double s)
{
    if constexpr (kMaternKind<KIND>) return matern_slope(KIND == SIGSVGD_STATIC_MATERN32, matern_u(KIND == SIGSVGD_STATIC_MATERN32, s));
    const double k = radial_phi<KIND>(s);
    return KIND == SIGSVGD_STATIC_IMQ ? 0.5 * (k * k * k) : k * k;
}

// the static kernel of x (LDS, fp64) and y (global, the caller's dtype)
template <int KIND, typename IO>
__device__ __forceinline__ double static_k(const double *x, const IO *y, int d, double inv_h)
{
    double s = 0.0;
    if constexpr (kRadialKind<KIND>) {
        for (int c = 0; c < d; ++c) {
            const double t = x[c] - (double)y[c];
            s = __builtin_fma(t, t, s);
        }
        return radial_phi<KIND>(s * inv_h);
    }
    if (KIND == SIGSVGD_STATIC_RBF) {
        for (int c = 0; c < d; ++c) {
            const double t = x[c] - (double)y[c];
            s = __builtin_fma(t, t, s);
        }
        return exp64(-s * inv_h);
    }
    for (int c = 0; c < d; ++c) s = __builtin_fma(x[c], (double)y[c], s);
    return s;
}
// the same with y's first min(d, 16) coordinates in registers (d <= 16; the branches on d are wave-uniform)
template <int KIND>
__device__ __forceinline__ double static_k16(const double *x, const double (&y)[16], int d, double inv_h)
{
    double s = 0.0;
    if constexpr (kRadialKind<KIND>) {
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            if (c < d) {
                const double t = x[c] - y[c];
                s = __builtin_fma(t, t, s);
            }
        }
        return radial_phi<KIND>(s * inv_h);
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < d) {
            if (KIND == SIGSVGD_STATIC_RBF) {
                const double t = x[c] - y[c];
                s = __builtin_fma(t, t, s);
            } else {
                s = __builtin_fma(x[c], y[c], s);
            }
        }
    }
    return KIND == SIGSVGD_STATIC_RBF ? exp64(-s * inv_h) : s;
}

// The pair's coarse S chained through the static kernel's derivative into the gradient of the points of one of its paths.
// Lanes own points o of that path, 63 per pass (lane l holds o = o0 - 1 + l and, from lane 1 on, its gradient; S at o - 1
// arrives from the lane below), and walk the points t of the other path in order.  dG[m][n] / w = (S[m-1][n-1] + S[m][n]) -
// (S[m-1][n] + S[m][n-1]), S = 0 outside the coarse grid; store(o, c, g) takes coordinate c of own point o's gradient.
// OWN_X: the points are X's, dk/dx = -2 inv_h (x - y) k (RBF) or y (linear); else Y's, dk/dy = 2 inv_h (x - y) k or x.
// The radial kinds: RBF's with -phi'(s) for k.
template <int KIND, bool OWN_X, typename IO, typename Store>
__device__ __forceinline__ void static_grad_pass(const RingWave &rw, const IO *own, int To, const IO *oth, int Tt, int d,
                                                 double inv_h, Store &&store)
{
    const int lane = threadIdx.x;
    for (int o0 = 0; o0 < To; o0 += kWave - 1) {
        const int o = o0 - 1 + lane;
        const bool valid = lane >= 1 && o < To;
        const IO *po = own + (size_t)min(max(o, 0), To - 1) * d;
        for (int c0 = 0; c0 < d; c0 += 16) {
            double accv[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) accv[c] = 0.0;
            double s_prev = 0.0, nb_prev = 0.0; // S at (o, t - 1), (o - 1, t - 1)
            for (int t = 0; t < Tt; ++t) {
                const int oc = min(max(o, 0), To - 2), tc = min(t, Tt - 2); // (read at a clamped block, then dropped)
                const double s = OWN_X ? ring_S(rw, oc, tc) : ring_S(rw, tc, oc);
                const double s_cur = o >= 0 && o < To - 1 && t < Tt - 1 ? s : 0.0;
                const double nb = shfl_up_f64(s_cur); // S at (o - 1, t)
                const double R = (nb_prev + s_cur) - (nb + s_prev); // dG / w
                s_prev = s_cur;
                nb_prev = nb;
                const IO *pt = oth + (size_t)t * d;
                const IO *xm = OWN_X ? po : pt, *yn = OWN_X ? pt : po;
                if constexpr (kRadialKind<KIND>) { // RBF's contraction with -phi'(s) in place of exp(-s)
                    double dist = 0.0;
                    for (int c = 0; c < d; ++c) {
                        const double u = (double)xm[c] - (double)yn[c];
                        dist = __builtin_fma(u, u, dist);
                    }
                    const double rk = R * radial_slope<KIND>(dist * inv_h);
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (c0 + c < d) accv[c] = __builtin_fma(rk, (double)xm[c0 + c] - (double)yn[c0 + c], accv[c]);
                } else if (KIND == SIGSVGD_STATIC_RBF) {
                    double dist = 0.0;
                    for (int c = 0; c < d; ++c) {
                        const double u = (double)xm[c] - (double)yn[c];
                        dist = __builtin_fma(u, u, dist);
                    }
                    const double rk = R * exp64(-dist * inv_h);
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (c0 + c < d) accv[c] = __builtin_fma(rk, (double)xm[c0 + c] - (double)yn[c0 + c], accv[c]);
                } else {
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (c0 + c < d) accv[c] = __builtin_fma(R, (double)pt[c0 + c], accv[c]);
                }
            }
            if (valid) {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c0 + c < d)
                        store(o, c0 + c, KIND == SIGSVGD_STATIC_RBF || kRadialKind<KIND>
                                             ? ((OWN_X ? -2.0 : 2.0) * inv_h) * accv[c]
                                             : accv[c]);
            }
        }
    }
}
// One outer pass of static_grad_pass, statement for statement: the 63 points o0 - 1 + lane of lanes 1 .. 63 (lane: the thread's
// lane in its wave), for kernels that deal the passes to several waves (pair_bands.hip).  static_grad_pass itself does not call
// it: built as a loop over this function the serial kernels of gram_long.hip compile to different code (branch polarity and
// block order in every gradient instantiation), and their code is kept as it is (see the note on shared solves there).  A change
// to either body belongs in both; tests/test_gpu_pair_bands.py holds the two bit-identical for every static kernel.
template <int KIND, bool OWN_X, typename IO, typename Store>
__device__ __forceinline__ void static_grad_pass_one(const RingWave &rw, const IO *own, int To, const IO *oth, int Tt, int d,
                                                     double inv_h, int lane, int o0, Store &&store)
{
    const int o = o0 - 1 + lane;
    const bool valid = lane >= 1 && o < To;
    const IO *po = own + (size_t)min(max(o, 0), To - 1) * d;
    for (int c0 = 0; c0 < d; c0 += 16) {
        double accv[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) accv[c] = 0.0;
        double s_prev = 0.0, nb_prev = 0.0; // S at (o, t - 1), (o - 1, t - 1)
        for (int t = 0; t < Tt; ++t) {
            const int oc = min(max(o, 0), To - 2), tc = min(t, Tt - 2); // (read at a clamped block, then dropped)
            const double s = OWN_X ? ring_S(rw, oc, tc) : ring_S(rw, tc, oc);
            const double s_cur = o >= 0 && o < To - 1 && t < Tt - 1 ? s : 0.0;
            const double nb = shfl_up_f64(s_cur); // S at (o - 1, t)
            const double R = (nb_prev + s_cur) - (nb + s_prev); // dG / w
            s_prev = s_cur;
            nb_prev = nb;
            const IO *pt = oth + (size_t)t * d;
            const IO *xm = OWN_X ? po : pt, *yn = OWN_X ? pt : po;
            if constexpr (kRadialKind<KIND>) { // RBF's contraction with -phi'(s) in place of exp(-s)
                double dist = 0.0;
                for (int c = 0; c < d; ++c) {
                    const double u = (double)xm[c] - (double)yn[c];
                    dist = __builtin_fma(u, u, dist);
                }
                const double rk = R * radial_slope<KIND>(dist * inv_h);
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c0 + c < d) accv[c] = __builtin_fma(rk, (double)xm[c0 + c] - (double)yn[c0 + c], accv[c]);
            } else if (KIND == SIGSVGD_STATIC_RBF) {
                double dist = 0.0;
                for (int c = 0; c < d; ++c) {
                    const double u = (double)xm[c] - (double)yn[c];
                    dist = __builtin_fma(u, u, dist);
                }
                const double rk = R * exp64(-dist * inv_h);
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c0 + c < d) accv[c] = __builtin_fma(rk, (double)xm[c0 + c] - (double)yn[c0 + c], accv[c]);
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c0 + c < d) accv[c] = __builtin_fma(R, (double)pt[c0 + c], accv[c]);
            }
        }
        if (valid) {
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (c0 + c < d)
                    store(o, c0 + c, KIND == SIGSVGD_STATIC_RBF || kRadialKind<KIND>
                                         ? ((OWN_X ? -2.0 : 2.0) * inv_h) * accv[c]
                                         : accv[c]);
        }
    }
}

// The sum of v over the wavefront, the same bits in every lane: a butterfly whose adds have a fixed shape (lane l adds its
// partner l ^ 32, then l ^ 16, ... l ^ 1; the two lanes of an exchange form the same sum, a + b and b + a).
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// The pair's coarse S chained through the static kernel's derivative in the bandwidth: returns
//   dK / d inv_h = - sum_{m,n} R[m][n] slope(dist inv_h) dist,   dist = |x_m - y_n|^2,
// R = dG / w as in static_grad_pass and slope = exp(-s) (RBF) or radial_slope (the radial kinds): the contraction of
// static_grad_pass<KIND, true> with the scalar dist in place of (x_m - y_n) -2 inv_h.  Lanes own points m of X, 63 per pass,
// and walk the points n of Y; the 63 sums of a pass are added by wave_sum_f64 and the passes in order, so the bits depend on
// the inputs alone.  Every lane returns the value.  The radial kinds and RBF only: the linear kernel has no bandwidth.
template <int KIND, typename IO>
__device__ __forceinline__ double static_bw_pass(const RingWave &rw, const IO *X, int M, const IO *Y, int N, int d,
                                                 double inv_h)
{
    static_assert(KIND == SIGSVGD_STATIC_RBF || kRadialKind<KIND>, "the bandwidth pass is for the kernels of |x - y|^2 inv_h");
    const int lane = threadIdx.x;
    double total = 0.0;
    for (int o0 = 0; o0 < M; o0 += kWave - 1) {
        const int o = o0 - 1 + lane;
        const bool valid = lane >= 1 && o < M;
        const IO *xm = X + (size_t)min(max(o, 0), M - 1) * d;
        double acc = 0.0;
        double s_prev = 0.0, nb_prev = 0.0; // S at (o, t - 1), (o - 1, t - 1)
        for (int t = 0; t < N; ++t) {
            const int oc = min(max(o, 0), M - 2), tc = min(t, N - 2); // (read at a clamped block, then dropped)
            const double s = ring_S(rw, oc, tc);
            const double s_cur = o >= 0 && o < M - 1 && t < N - 1 ? s : 0.0;
            const double nb = shfl_up_f64(s_cur); // S at (o - 1, t)
            const double R = (nb_prev + s_cur) - (nb + s_prev); // dG / w
            s_prev = s_cur;
            nb_prev = nb;
            const IO *yn = Y + (size_t)t * d;
            double dist = 0.0;
            for (int c = 0; c < d; ++c) {
                const double u = (double)xm[c] - (double)yn[c];
                dist = __builtin_fma(u, u, dist);
            }
            double rk;
            if constexpr (kRadialKind<KIND>)
                rk = R * radial_slope<KIND>(dist * inv_h);
            else
                rk = R * exp64(-dist * inv_h);
            acc = __builtin_fma(rk, dist, acc);
        }
        total += wave_sum_f64(valid ? acc : 0.0);
    }
    return -total;
}
} // namespace
} // namespace sigsvgd
