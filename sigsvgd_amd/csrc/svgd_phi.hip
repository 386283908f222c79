// SVGD velocity: v = -((K @ score - grad_k) / N) [* mask], optionally fused with the simple Adagrad
// scaling of the reference (svgd.py:110-113) and the optimizer=None particle update X_out = X_in - lr * v
// (reference src/inference/svgd.py:82-83,115; mask: src/inference/trajectory_svgd.py:84), or with the update of
// the reference's DEFAULT optimizer, torch.optim.Adam driven through a closure that sets X.grad = v
// (svgd.py:20,100-107): exp_avg / exp_avg_sq updated in place, bias corrections from a step counter that lives
// on the device (so the launch can be replayed from a captured graph), X_out = X_in - lr/bc1 * m / (sqrt(v2)/sqrt(bc2) + eps).
//
// The N x N x D product is the only GEMM-shaped piece of the hot path and runs on the fp32 MFMA
// (v_mfma_f32_16x16x4_f32: exact fp32 FMA chain, same numerics as the reference's fp32 matmul).
// It is small (0.94 GFLOP at N=1024, D=448) and latency-bound, so the kernel is organised for
// overlap rather than tile size: a workgroup of 4 wavefronts owns a 32 x 64 output tile (224
// workgroups at C4: one per CU), every wavefront computes the whole tile over ITS quarter of each
// 64-deep k stage (split-K inside the workgroup, combined through LDS at the end), global loads are
// 16 B per lane and the next stage is fetched into registers while the current one is multiplied.
//
// svgd_update_kernel applies the same update rules (update_element, shared with the epilogue above) to a velocity the
// caller already has: the particle-sharded step, whose velocity is a sum over ranks (sigsvgd_svgd_update).
#include <algorithm>

#include "sig_common.h"

namespace sigsvgd {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int PM = 32;  // rows per workgroup
constexpr int PN = 64;  // cols per workgroup
constexpr int PK = 64;  // k per stage (16 per wavefront)
constexpr int KS = PK + 4; // LDS row strides (floats), padded: 16-B aligned, conflict-light
constexpr int SS = PN + 16; // = 16 mod 32: the two k rows a 32-lane read touches land on disjoint banks

struct AdamArgs {
    float *exp_avg, *exp_avg_sq; // [N, D] fp32 state, updated in place; exp_avg == NULL: no Adam
    const int *step;             // device counter: updates done so far (this launch is update *step + 1)
    double lr, beta1, beta2;     // doubles as torch holds them: 1 - beta and the bias corrections are formed in fp64
    float eps;
};

__global__ void counter_inc_kernel(int *ctr) { *ctr += 1; }

// The update rules of one element, shared by the fused epilogue of svgd_phi_kernel and by svgd_update_kernel (which gets
// its velocity from memory): the arithmetic, its order and the fp64 formation of the Adam scalars are here and nowhere else.
struct UpdateScalars {
    float lr, step_size, inv_sqrt_bc2, omb1, omb2, b2, eps;
};

__device__ __forceinline__ UpdateScalars update_scalars(float lr, const AdamArgs &adam)
{
    UpdateScalars c{lr, lr, 1.f, 0.f, 0.f, 0.f, adam.eps};
    if (adam.exp_avg) { // torch.optim.Adam (amsgrad=False, weight_decay=0, maximize=False): scalars in fp64 as torch
        const double t = (double)(*adam.step + 1);
        c.step_size = (float)(adam.lr / (1.0 - pow(adam.beta1, t)));
        c.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(adam.beta2, t)));
        c.omb1 = (float)(1.0 - adam.beta1);
        c.omb2 = (float)(1.0 - adam.beta2);
        c.b2 = (float)adam.beta2;
    }
    return c;
}

// v_raw = -((K @ score - grad_k)/N) of the element, mv its mask value (1 without a mask).  Returns the velocity after mask
// and Adagrad (what v_out receives).  In place: ag the Adagrad sum (with_adagrad), m / q Adam's exp_avg / exp_avg_sq
// (with_adam), x the particle: x - step_size * m / (sqrt(q)/sqrt(bc2) + eps) under Adam, else x - lr * v.
__device__ __forceinline__ float update_element(float v_raw, float mv, bool with_adagrad, bool with_adam,
                                                const UpdateScalars &c, float &ag, float &m, float &q, float &x)
{
    // Which products are fused with their sums is WRITTEN here, not left to the compiler's contraction: that choice depends
    // on the code around the call, and the two kernels must agree bit for bit (with each other and with every earlier build
    // of the fused kernel, whose choices these are).
#pragma clang fp contract(off)
    float v = v_raw * mv;
    if (with_adagrad) { // reference svgd.py:110-113: running sum of squared gradients, g / sqrt(sum + 1e-12)
        ag = fmaf(v, v, ag);
        v = v / sqrtf(ag + 1e-12f);
    }
    if (with_adam) {
        m = fmaf(c.omb1, v - m, m); // lerp
        q = c.b2 * q + c.omb2 * (v * v); // two products and a sum
        x = fmaf(-c.step_size, m / fmaf(sqrtf(q), c.inv_sqrt_bc2, c.eps), x);
    } else
        x = fmaf(-c.lr, v, x);
    return v;
}

__global__ __launch_bounds__(256) void svgd_phi_kernel(const float *__restrict__ K, const float *__restrict__ S,
                                                       const float *__restrict__ gk, const float *__restrict__ mask,
                                                       int N, int D, float *__restrict__ v_out,
                                                       // (no __restrict__ on the particles: the in-place update passes the
                                                       //  same buffer as X_in and X_out; every element is read and then
                                                       //  written by the same thread)
                                                       const float *X_in, float *X_out, float lr,
                                                       float *__restrict__ adagrad, AdamArgs adam)
{
    __shared__ __align__(16) float kt[PM * KS];     // K tile      [row][k]
    __shared__ __align__(16) float st[PK * SS];     // score tile  [k][col]
    __shared__ __align__(16) float red[4 * PM * PN]; // partial tiles of the four wavefronts (k quarters)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.y * PM, col0 = blockIdx.x * PN;
    const bool vecK = (N % 4) == 0 && (reinterpret_cast<uintptr_t>(K) & 15) == 0;
    const bool vecS = (D % 4) == 0 && (reinterpret_cast<uintptr_t>(S) & 15) == 0;

    // this thread's share of a stage: K tile 32x64 = 512 float4 (2 per thread), score tile 64x64 = 1024 float4 (4)
    f32x4 ka[2], sa[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + u * 256, r = e / (PK / 4), c4 = (e % (PK / 4)) * 4;
            const int gr = row0 + r, gc = k0 + c4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gr < N) {
                if (vecK && gc + 3 < N)
                    v = *reinterpret_cast<const f32x4 *>(K + (size_t)gr * N + gc);
                else
#pragma unroll
                    for (int x = 0; x < 4; ++x)
                        if (gc + x < N) v[x] = K[(size_t)gr * N + gc + x];
            }
            ka[u] = v;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + u * 256, r = e / (PN / 4), c4 = (e % (PN / 4)) * 4;
            const int gr = k0 + r, gc = col0 + c4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gr < N) {
                if (vecS && gc + 3 < D)
                    v = *reinterpret_cast<const f32x4 *>(S + (size_t)gr * D + gc);
                else
#pragma unroll
                    for (int x = 0; x < 4; ++x)
                        if (gc + x < D) v[x] = S[(size_t)gr * D + gc + x];
            }
            sa[u] = v;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + u * 256, r = e / (PK / 4), c4 = (e % (PK / 4)) * 4;
            *reinterpret_cast<f32x4 *>(&kt[r * KS + c4]) = ka[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + u * 256, r = e / (PN / 4), c4 = (e % (PN / 4)) * 4;
            *reinterpret_cast<f32x4 *>(&st[r * SS + c4]) = sa[u];
        }
    };

    f32x4 acc[2][4]; // [row half][col quarter] 16x16 accumulators of this wavefront's k quarter
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    for (int k0 = 0; k0 < N; k0 += PK) {
        __syncthreads(); // previous stage fully consumed
        stash();
        __syncthreads();
        if (k0 + PK < N) fetch(k0 + PK); // in flight during the MFMAs below
        // A operand (16x16x4): A[i = lane&15][k = lane>>4]; B[k = lane>>4][j = lane&15]
        const int kk = lane >> 4, ij = lane & 15, kw = wave * 16;
#pragma unroll
        for (int ks = 0; ks < 16; ks += 4) {
            const float a0 = kt[ij * KS + kw + ks + kk];
            const float a1 = kt[(16 + ij) * KS + kw + ks + kk];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float bv = st[(kw + ks + kk) * SS + b * 16 + ij];
                acc[0][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][b], 0, 0, 0);
                acc[1][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][b], 0, 0, 0);
            }
        }
    }
    // combine the four k-quarters: C/D map (16x16): col = lane&15, row = (lane>>4)*4 + reg.  Every wavefront parks its
    // partial tile, then ALL 256 threads run the epilogue, 8 outputs each with consecutive threads on consecutive columns
    // (round 2 left it to wavefront 0: 32 outputs per lane, one load-compute-store chain after the other -- 46 of the
    // kernel's 47 us at C4 were this tail)
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                red[wave * PM * PN + (a * 16 + (lane >> 4) * 4 + r) * PN + b * 16 + (lane & 15)] = acc[a][b][r];
    __syncthreads();
    const float invN = 1.0f / (float)N;
    const UpdateScalars c = update_scalars(lr, adam);
    constexpr int EPT = PM * PN / 256; // outputs per thread
    float sv[EPT], gv[EPT], xv[EPT], mv[EPT], av[EPT], e1[EPT], e2[EPT];
    bool ok[EPT];
#pragma unroll
    for (int u = 0; u < EPT; ++u) { // all loads first: one round trip for the lot
        const int el = tid + u * 256, lr_ = el / PN, lc = el % PN;
        const int gr = row0 + lr_, gc = col0 + lc;
        ok[u] = gr < N && gc < D;
        const size_t idx = ok[u] ? (size_t)gr * D + gc : 0;
        sv[u] = ((red[lr_ * PN + lc] + red[PM * PN + lr_ * PN + lc]) + red[2 * PM * PN + lr_ * PN + lc]) +
                red[3 * PM * PN + lr_ * PN + lc];
        gv[u] = gk[idx];
        mv[u] = mask ? mask[idx] : 1.f;
        av[u] = adagrad ? adagrad[idx] : 0.f;
        xv[u] = X_in ? X_in[idx] : 0.f;
        e1[u] = adam.exp_avg ? adam.exp_avg[idx] : 0.f;
        e2[u] = adam.exp_avg ? adam.exp_avg_sq[idx] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < EPT; ++u) {
        if (!ok[u]) continue;
        const int el = tid + u * 256;
        const size_t idx = (size_t)(row0 + el / PN) * D + col0 + el % PN;
        v_out[idx] = update_element(-((sv[u] - gv[u]) * invN), mv[u], adagrad != nullptr, adam.exp_avg != nullptr, c,
                                    av[u], e1[u], e2[u], xv[u]);
        if (adagrad) adagrad[idx] = av[u];
        if (adam.exp_avg) {
            adam.exp_avg[idx] = e1[u];
            adam.exp_avg_sq[idx] = e2[u];
        }
        if (X_out) X_out[idx] = xv[u];
    }
}

// The same update rules on a velocity that is GIVEN (the sharded step: the reduce-scatter's sum over ranks, on this rank's
// rows -- mask, Adagrad and Adam are not linear, so they cannot run before it).  Elementwise over n = N*D, grid-stride, W
// elements per access; every element is read and then written by the same thread, so X_in == X_out (and v_in == v_out) is
// legal.
template <int W> __device__ __forceinline__ void load_lanes(const float *p, float (&e)[W])
{
    if constexpr (W == 4) { // one 16-byte load (the caller has checked the alignment)
        const f32x4 t = *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = t[k];
    } else
        e[0] = *p;
}

template <int W> __device__ __forceinline__ void store_lanes(float *p, const float (&e)[W])
{
    if constexpr (W == 4)
        *reinterpret_cast<f32x4 *>(p) = f32x4{e[0], e[1], e[2], e[3]};
    else
        *p = e[0];
}

template <int W>
__device__ __forceinline__ void update_span(const float *v_in, const float *mask, size_t n, float *v_out, const float *X_in,
                                            float *X_out, float *adagrad, const AdamArgs &adam, const UpdateScalars &c)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / W; i += stride) {
        const size_t o = i * W;
        float vv[W], mv[W], av[W], xv[W], e1[W], e2[W], vo[W];
#pragma unroll
        for (int k = 0; k < W; ++k) mv[k] = 1.f, av[k] = xv[k] = e1[k] = e2[k] = 0.f;
        load_lanes<W>(v_in + o, vv); // all loads first; the null tests are uniform over the launch
        if (mask) load_lanes<W>(mask + o, mv);
        if (adagrad) load_lanes<W>(adagrad + o, av);
        if (X_in) load_lanes<W>(X_in + o, xv);
        if (adam.exp_avg) {
            load_lanes<W>(adam.exp_avg + o, e1);
            load_lanes<W>(adam.exp_avg_sq + o, e2);
        }
#pragma unroll
        for (int k = 0; k < W; ++k)
            vo[k] = update_element(vv[k], mv[k], adagrad != nullptr, adam.exp_avg != nullptr, c, av[k], e1[k], e2[k], xv[k]);
        if (adagrad) store_lanes<W>(adagrad + o, av);
        if (v_out) store_lanes<W>(v_out + o, vo);
        if (adam.exp_avg) {
            store_lanes<W>(adam.exp_avg + o, e1);
            store_lanes<W>(adam.exp_avg_sq + o, e2);
        }
        if (X_out) store_lanes<W>(X_out + o, xv);
    }
}

__global__ __launch_bounds__(256) void svgd_update_kernel(const float *v_in, const float *__restrict__ mask, int N, int D,
                                                          float *v_out, const float *X_in, float *X_out, float lr,
                                                          float *adagrad, AdamArgs adam)
{
    const UpdateScalars c = update_scalars(lr, adam);
    const size_t n = (size_t)N * D;
    // 16-byte accesses where every row starts on a 16-byte boundary: the test svgd_phi_kernel's fetch makes
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(v_in) | reinterpret_cast<uintptr_t>(mask) |
                           reinterpret_cast<uintptr_t>(v_out) | reinterpret_cast<uintptr_t>(X_in) |
                           reinterpret_cast<uintptr_t>(X_out) | reinterpret_cast<uintptr_t>(adagrad) |
                           reinterpret_cast<uintptr_t>(adam.exp_avg) | reinterpret_cast<uintptr_t>(adam.exp_avg_sq);
    if ((D % 4) == 0 && (ptrs & 15) == 0)
        update_span<4>(v_in, mask, n, v_out, X_in, X_out, adagrad, adam, c);
    else
        update_span<1>(v_in, mask, n, v_out, X_in, X_out, adagrad, adam, c);
}

int phi_launch(const float *K, const float *score, const float *grad_k, const float *mask, int N, int D,
               float *v_out, const float *X_in, float *X_out, float lr, float *adagrad, hipStream_t stream,
               float *exp_avg, float *exp_avg_sq, int *step_dev, double lr_adam, double beta1, double beta2, float eps)
{
    if (N < 1 || D < 1 || !K || !score || !grad_k || !v_out) {
        set_error("svgd_phi: bad arguments N=%d D=%d", N, D);
        return SIGSVGD_E_BADARG;
    }
    if ((X_in == nullptr) != (X_out == nullptr)) {
        set_error("svgd_phi: X_in and X_out must both be given or both be NULL");
        return SIGSVGD_E_BADARG;
    }
    AdamArgs adam{exp_avg, exp_avg_sq, step_dev, lr_adam, beta1, beta2, eps};
    if (exp_avg && (!exp_avg_sq || !step_dev || !X_in || adagrad)) {
        set_error("svgd_adam_step: needs exp_avg, exp_avg_sq, step, X_in/X_out (and no Adagrad state)");
        return SIGSVGD_E_BADARG;
    }
    dim3 grid((D + PN - 1) / PN, (N + PM - 1) / PM);
    hipLaunchKernelGGL(svgd_phi_kernel, grid, dim3(256), 0, stream, K, score, grad_k, mask, N, D, v_out, X_in, X_out, lr,
                       adagrad, adam);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch svgd_phi_kernel");
    if (exp_avg) { // the counter moves only after every workgroup of the update has read it (stream order)
        hipLaunchKernelGGL(counter_inc_kernel, dim3(1), dim3(1), 0, stream, step_dev);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "launch counter_inc_kernel");
    }
    return SIGSVGD_OK;
}

int update_launch(const float *v_in, const float *mask, int N, int D, float *v_out, const float *X_in, float *X_out,
                  float lr, float *adagrad, hipStream_t stream, float *exp_avg, float *exp_avg_sq, int *step_dev,
                  double lr_adam, double beta1, double beta2, float eps)
{
    if (N < 1 || D < 1 || !v_in) {
        set_error("svgd_update: bad arguments N=%d D=%d", N, D);
        return SIGSVGD_E_BADARG;
    }
    if ((X_in == nullptr) != (X_out == nullptr)) {
        set_error("svgd_update: X_in and X_out must both be given or both be NULL");
        return SIGSVGD_E_BADARG;
    }
    const bool want_adam = exp_avg || exp_avg_sq || step_dev;
    if (want_adam && (!exp_avg || !exp_avg_sq || !step_dev || !X_in || adagrad)) {
        set_error("svgd_update: Adam needs exp_avg, exp_avg_sq, step, X_in/X_out (and no Adagrad state)");
        return SIGSVGD_E_BADARG;
    }
    if (!v_out && !X_out && !adagrad) {
        set_error("svgd_update: nothing to write (v_out, X_out and the state are all NULL)");
        return SIGSVGD_E_BADARG;
    }
    AdamArgs adam{exp_avg, exp_avg_sq, step_dev, lr_adam, beta1, beta2, eps};
    // about four accesses per thread: the launch is latency-bound at shard sizes (a [1024, 448] shard is 112 workgroups)
    const size_t work = ((size_t)N * D + 3) / 4;
    const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>((work + 4 * 256 - 1) / (4 * 256), 1), 4096);
    hipLaunchKernelGGL(svgd_update_kernel, dim3(grid), dim3(256), 0, stream, v_in, mask, N, D, v_out, X_in, X_out, lr,
                       adagrad, adam);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch svgd_update_kernel");
    if (exp_avg) { // as in phi_launch: the counter moves behind the update, in stream order
        hipLaunchKernelGGL(counter_inc_kernel, dim3(1), dim3(1), 0, stream, step_dev);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "launch counter_inc_kernel");
    }
    return SIGSVGD_OK;
}

} // namespace sigsvgd
