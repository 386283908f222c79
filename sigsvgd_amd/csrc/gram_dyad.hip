// Signature-kernel Gram forward/backward for SHORT paths with DYADIC REFINEMENT -- the shapes the reference's own
// scripts use (T = 3 .. 33 points, dyadic order 2 .. 6: examples/script_planning_obstacle_field.py:156-158,325,
// script_planning_robot.py:391, BASELINE.json config C1) -- on the register-resident sweep engine of the quadrant kernel.
//
// The refined PDE grid has P = (T - 1) * 2^n cells per side, 64 <= P <= 128 here: 2 x 2 quadrants of <= 64 x 64 cells,
// swept with the hand-written statements of quad_sweeps.h (one wavefront per trajectory pair, lane = cell row, slot =
// (column + lane) & 63, fp32 difference form, EXEC windows, quadrant hand-over through LDS rows).  What differs from
// gram_quad.hip is everything around the sweeps, and all of it is small because it lives on the COARSE grid:
//   * static kernel: T x T values per pair in fp64 (lane = point row), 4-corner increments D_coarse[(T-1)^2] -> LDS (fp32,
//     scaled by 1 / (r^2 sqrt(12)): the refined increment of every fine cell of a coarse cell, as the stencil wants it);
//   * a quadrant's increments are GATHERED from that table into the slot registers (64 LDS reads per visit): nothing to
//     keep between visits, no scratch in global memory;
//   * after a quadrant's reverse sweep its S = K_fwd * U values are block-summed into S_coarse[(T-1)^2] (fp64, LDS adds
//     by one wavefront in program order), which is dL/dD_coarse up to 1 / r^2;
//   * the 4-corner scatter R, the RBF derivative and both contractions run once per pair on the coarse grid, fp32 on the
//     differences x_m - y_n as in the other kernels.
// Gradient partial sums leave through the segment / item slabs of grad_reduce_kernel (gram_fast.hip): no atomics between
// wavefronts, bit-reproducible results.  Until round 3 these shapes ran on the coverage kernel (one wavefront per pair,
// 53 instructions per PDE step on one dependent chain: 86 us for C1's 136 pairs).
//
// Reference semantics: sigkernel _SigKernelGram.forward/backward [RECALLED, SURVEY.md App. A]; static kernel
// src/kernels/_traj_kernels.py:176-195; callers src/inference/score.py:68-69.
#include "sig_common.h"
#include "sweep_scaffold.h"

namespace sigsvgd {

struct DyadArgs {
    const void *X, *Y, *go;
    void *K;
    double *rseg; // [owned tiles + workgroups][8][T*d]
    float *cslab; // [items][T*d] (symmetric launches)
    int io64, A, B, T, d, n, symw;
    TileMap tm;
    long long nitems;
    double inv_h;
    unsigned char *kflag; // [A][B]: 1 where the repair rule of sweep_scaffold.h flags the pair: the launcher lets the coverage kernel
                          // solve those pairs' K again in fp64
};

namespace {
// wavefronts (rows i) per workgroup: 8 (two per SIMD) when there are pairs to fill the chip, 4 (one per SIMD: a wavefront's
// dependent chain then has the SIMD to itself) when the launch is a handful of workgroups (C1: 136 pairs)
constexpr int DTMAX = 33; // coarse points per path
constexpr int DHN = 136;  // hand-over rows: entries 0 .. 129 are read

#include "quad_sweeps.h"
} // namespace

// FEW (forward-only launches of paths in <= 3 channels, 8-channel layout): the forward steps also accumulate sum |K_fwd * D|,
// the bound on the condition number of sweep_scaffold.h ("the repair rule"); gradient launches take the condition number itself
// from the coarse tables (sum |S_coarse D_coarse|, one pass over (T-1)^2 entries per pair)
template <int DPAD, bool GRAD, bool SYM, int DNW, bool FEW = false>
__global__ __launch_bounds__(DNW * 64) __attribute__((amdgpu_waves_per_eu(DNW == 8 ? 2 : 1, 2))) void gram_dyad_kernel(DyadArgs a)
{
    constexpr int NT = DNW * 64;
    constexpr int TM = DTMAX - 1; // coarse cells per side at most
    __shared__ __align__(16) double yd[DTMAX * (DPAD + 1)]; // y~_n in fp64 (centred on y[0]), [DPAD] = -|y~_n|^2 / h
    __shared__ __align__(16) float yf[DTMAX * DPAD];        // the same in fp32 for the coarse contraction
    __shared__ double yref[DPAD];
    __shared__ float ones[DHN];
    struct WaveLds {
        double Sc[TM * TM];    // block sums of S = K_fwd * U over the fine cells of every coarse cell
        float Dc[TM * TM];     // coarse increments / (r^2 sqrt(12)); after the last gather: the parked column-side sums
        float hK[DHN], hU[DHN], hdummy[64];
        float rowacc[DTMAX * DPAD]; // row-side gradient of the wavefront's particle over the columns of a segment
    };
    __shared__ WaveLds wl_all[DNW];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = a.T, d = a.d, n = a.n, io64 = a.io64, Tm = T - 1;
    const int P = Tm << n, nrows1 = P - 64; // cell rows of band 1 = cell columns of half 1 (0 .. 64)
    const double inv_h = a.inv_h;
    const float m2h = (float)(-2.0 * inv_h);
    const double dscale = 1.0 / ((double)(1 << n) * (double)(1 << n) * 3.46410161513775459); // 1 / (r^2 sqrt(12))
    const double inv_r2 = 1.0 / ((double)(1 << n) * (double)(1 << n));
    WaveLds &wl = wl_all[wave];
    float *hK = wl.hK, *hU = wl.hU, *hdummy = wl.hdummy;
    for (int e = tid; e < DHN; e += NT) ones[e] = 1.f;
    for (int e = lane; e < DHN; e += 64) hK[e] = 1.f, hU[e] = 1.f;

    // static item ranges: (owned row tile, column), tile-major; symmetric launches only the columns from the tile's first row
    const long long it0 = a.nitems * blockIdx.x / gridDim.x, it1 = a.nitems * (blockIdx.x + 1) / gridDim.x;
    int remaining = (int)(it1 - it0);
    long long item = it0;
    const ItemSeek seek = item_seek<SYM>(a.tm, a.B, DNW, it0);
    int kq = seek.kq, cstart = seek.cstart;
#pragma unroll 1
    while (remaining > 0) {
    const TileRange tr = tile_range<SYM>(a.tm, a.B, DNW, kq, cstart, remaining);
    const int i = tr.i0 + wave;
    const int j0 = tr.cfirst + cstart, j1 = j0 + tr.ncol;
    const bool row_ok = i < a.A;
    if (GRAD)
        for (int e = lane; e < DTMAX * DPAD; e += 64) wl.rowacc[e] = 0.f;

#pragma unroll 1
    for (int j = j0; j < j1; ++j, ++item) {
        int lanep = lane;
        asm volatile("" : "+v"(lanep));
        // ---- stage y_j (coarse points, centred on its first point) ------------------------------------------------
        // (the same loop as in gram_band.hip, kept as a copy: through a stage_coarse_column helper three band kernels change
        //  their VGPR count -- gram_bandp_kernel<8, true, false, false, false> 120 -> 121)
        __syncthreads();
        for (int e = tid; e < T * DPAD; e += NT) {
            const int t = e / DPAD, c = e % DPAD;
            const double r0 = c < d ? load_any(a.Y, (size_t)j * T * d + c, io64) : 0.0;
            const double v = c < d ? load_any(a.Y, ((size_t)j * T + t) * d + c, io64) - r0 : 0.0;
            yd[t * (DPAD + 1) + c] = v;
            yf[t * DPAD + c] = (float)v;
            if (t == 0) yref[c] = r0;
            double s = v * v;
#pragma unroll
            for (int off = 1; off < DPAD; off <<= 1) s += __shfl_xor(s, off, 64);
            if (c == 0) yd[t * (DPAD + 1) + DPAD] = -s * inv_h;
        }
        __syncthreads();

        if (row_ok && (!SYM || j >= i)) {
            // (pair_weights of sweep_scaffold.h, kept as a copy: through the helper the 8-wave 16-channel symmetric gradient kernel
            //  spills 67 VGPRs instead of 68 -- resources must be equal -- profiles/sweep_scaffold_resources.txt)
            float w_ij = 1.f, w_ji = 1.f;
            if (GRAD) {
                if (a.go) {
                    w_ij = (float)load_any(a.go, (size_t)i * a.B + j, io64);
                    if (SYM || a.symw) w_ji = (float)load_any(a.go, (size_t)j * a.B + i, io64);
                    if (a.symw) { w_ij += w_ji; w_ji = w_ij; }
                } else if (a.symw) {
                    w_ij = 2.f; w_ji = 2.f;
                }
                if (SYM && j == i) w_ji = 0.f; // diagonal pair: first-slot derivative only
            }
            // ---- coarse static kernel: lane m = point row m; G[m][b] in fp64, row differences, 4-corner increments --------
            // (gram_band.hip's up to stride and offset of the table, kept as a copy: through a coarse_static_kernel helper
            //  gram_dyad_kernel<8, true, false, 8> spills 35 VGPRs for 36, scratch 136 B for 140)
            float xf[DPAD]; // x~_m in fp32 for the coarse contraction
            {
                const int m = min(lanep, T - 1);
                double xs[DPAD], xn = 0.0;
#pragma unroll
                for (int c = 0; c < DPAD; ++c) {
                    const double xc = c < d ? load_any(a.X, ((size_t)i * T + m) * d + c, io64) - yref[c] : 0.0;
                    xn = __builtin_fma(xc, xc, xn);
                    xs[c] = xc * (2.0 * inv_h);
                    xf[c] = (float)xc;
                }
                xn = -xn * inv_h;
                double gprev = 0.0;
                for (int b = 0; b < T; ++b) {
                    const double *yr = yd + b * (DPAD + 1);
                    double e2 = xn + yr[DPAD];
#pragma unroll
                    for (int c = 0; c < DPAD; ++c) e2 = __builtin_fma(xs[c], yr[c], e2);
                    const double g = exp64(e2);
                    const double rd = g - gprev; // G[m][b] - G[m][b-1]
                    gprev = g;
                    const double nb = shfl_down_f64(rd); // row m + 1
                    if (b >= 1 && lanep < Tm) wl.Dc[lanep * Tm + (b - 1)] = (float)((nb - rd) * dscale);
                }
                if (GRAD)
                    for (int e = lanep; e < Tm * Tm; e += 64) wl.Sc[e] = 0.0;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);

            float Dsl[64], Ssl[64];
            // (The chain state and the set-up of both sweeps are gram_quad.hip's, kept as a copy: as a QuadChain struct with
            //  quad_visit_forward / quad_visit_reverse helpers -- six forms -- gram_dyad_kernel<16, true, true, 8> spills 67 VGPRs for 68.)
            float fc = 1.f, fuA = 1.f, fuB = 1.f, fV = 0.f;
            float svc = 1.f, svA = 1.f, svB = 1.f, svV = 0.f;
            int fwd_prev = -1;
            float rc = 1.f, rdA = 1.f, rdB = 1.f, rV = 0.f;
            int rev_band = -1;
            bool kdone = false;
            float kmax = 1.f; // largest |K| this lane has seen on the pair's grid (boundary: 1)
            float cnd = 0.f;  // FEW: this lane's share of sum |K_fwd * gamma|
            float kfin_keep = 0.f;
            bool canc_keep = false;
            const QuadVisits qv = quad_visit_list(GRAD, nrows1, 0, 0); // (quad_sweeps.h; none of gram_quad.hip's scratch bits)
            const int b_last = nrows1 > 0 ? 1 : 0, h_last = nrows1 > 0 ? 1 : 0;

#pragma unroll 1
            for (int v = 0; v < qv.nv; ++v) {
                const int code = (int)((qv.vis >> (8 * v)) & 255);
                const int b = code & 1, h = (code >> 1) & 1;
                const bool rev = (code & 4) != 0, leave_k = (code & 8) != 0;
                const int nrows = b ? nrows1 : 64, ncols = h ? nrows1 : 64;
                int lv = lanep;
                asm volatile("" : "+v"(lv));
                const unsigned long long rows = nrows >= 64 ? ~0ull : ((1ull << nrows) - 1ull);
                const unsigned long long wr = ncols >= 64 ? ~0ull : (ncols > 0 ? ~0ull << (64 - ncols) : 0ull);

                // ---- increments of the quadrant: slot k of lane l is local column (k - l) & 63 -----------------------
                const int arow = min((64 * b + lv) >> n, Tm - 1);
                const float *dcrow = wl.Dc + arow * Tm;
                {
                    int cl = (64 - lv) & 63; // local column of slot 0
#pragma unroll
                    for (int k = 0; k < 64; ++k) {
                        Dsl[k] = dcrow[min((64 * h + cl) >> n, Tm - 1)];
                        cl = (cl + 1) & 63;
                    }
                }
                // ---- forward sweep ---------------------------------------------------------------------------------
                {
                    const float *topb = (b ? hK : ones) + 64 * h;
                    if (h == 0) {
                        fc = 1.f;
                        fV = 0.f;
                        fuA = (lanep == 0) ? topb[1] : 1.f;
                        fuB = (lanep == 0) ? topb[0] : 1.f;
                    } else if (fwd_prev != b) {
                        fc = svc;
                        fV = svV;
                        fuA = svA;
                        fuB = svB;
                    }
                    fwd_prev = b + 2 * h;
                    const unsigned ho = (unsigned)(size_t)(leave_k ? hK + 64 * h + 1 : hdummy + 63);
                    int haddr = (int)((lv == 63) ? ho : (unsigned)(size_t)(hdummy + lv));
                    const int hinc = (lanep == 63 && leave_k) ? 4 : 0;
                    float r3 = 1.7320508075688772f;
                    asm volatile("" : "+s"(r3));
#pragma unroll
                    for (int k = 0; k < 64; ++k) Ssl[k] = 0.f;
                    const float hbf = topb[lv + 2];
                    asm volatile("" ::: "memory");
                    quad_fwd_all<0, true, FEW ? 1 : 0>(fc, fuA, fuB, fV, Dsl, Ssl, wr, rows, hbf, haddr, hinc, r3, nrows + ncols, cnd);
                    asm volatile("" ::: "memory");
                    if (!kdone) { // (the slots: K at the cells' upper left corners; fc: the row's last value so far)
                        kmax = max3_abs(kmax, fc, fc);
#pragma unroll
                        for (int k = 0; k < 64; k += 2) kmax = max3_abs(kmax, Ssl[k], Ssl[k + 1]);
                    }
                }
                if (b == 0 && h == 0) {
                    svc = fc;
                    svV = fV;
                    svA = fuA;
                    svB = fuB;
                }
                if (!kdone && b == b_last && h == h_last) {
                    kdone = true;
                    // a pair whose solution cancelled (rough paths in few channels: DESIGN.md section 3) is marked for the fp64 pass
                    const float kfin = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fc), nrows - 1));
                    // Refined grids: the one full-magnitude add per cell rounds with the same sign row after row where the
                    // increments of neighbouring cells are (nearly) identical, i.e. the fp32 sweeps lose up to ~6e-8 per ROW of the
                    // largest value on the grid -- 5e-6 over 128 rows at dyadic order >= 5, where whole blocks of cells share one
                    // increment (round 3's sweep: 5.7e-6 on smooth paths with K ~ 1).  A pair that merely decays from the boundary
                    // value 1 to K = 0.18 therefore came out 1.7e-5 off (soak of round 4, case 504: T = 3, order 6, d = 2): at order
                    // >= 5 every pair whose grid maximum exceeds 1.5 max(|K|, 0.1) goes to the fp64 pass, and below that order the
                    // round-3 ratios apply WITHOUT the floor "grid maximum > 2" (the boundary value alone is a maximum of 1).
                    const float kden = repair_den(kfin);
                    bool fl = kmax > (n >= 5 ? 1.5f : repair_ratio(d)) * kden; // (order >= 5: 1.5, rounding per row of shared increments, above)
                    if constexpr (FEW) { // conditioning bound of a forward-only launch; sqrt(12) gamma = the fine increment
                        const float sds = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_sum_dpp<true>(cnd)), 63));
                        fl = fl || repair_fwd_bound(sds, kmax, kden);
                    }
                    const bool cancelled = __builtin_amdgcn_ballot_w64(kfin == kfin && fl) != 0;
                    if (lanep == nrows - 1) {
                        store_any(a.K, (size_t)i * a.B + j, (double)fc, io64);
                        if (SYM && j != i) store_any(a.K, (size_t)j * a.B + i, (double)fc, io64);
                        if (!GRAD) a.kflag[(size_t)i * a.B + j] = cancelled ? 1 : 0; // (gradient launches: with the condition number, below)
                    }
                    kfin_keep = kfin;
                    canc_keep = cancelled;
                }
                if (!GRAD || !rev) continue;

                // ---- reverse sweep (S = K_fwd * U replaces K_fwd slot by slot) ---------------------------------------
                {
                    const bool below = (b == 0) && nrows1 > 0;
                    const float *botb = (below ? hU : ones) + 64 * h;
                    if (rev_band != b) {
                        rev_band = b;
                        rc = 1.f;
                        rV = 0.f;
                        const float c1 = botb[ncols], c0 = botb[ncols - 1];
                        const bool odd = ((62 + ncols) & 1) != 0;
                        rdA = (lanep == 63) ? (odd ? c0 : c1) : 1.f;
                        rdB = (lanep == 63) ? (odd ? c1 : c0) : 1.f;
                    }
                    const bool leave_u = (b == 1);
                    const unsigned ho = (unsigned)(size_t)(leave_u ? hU + 64 * h + ncols - 1 : hdummy);
                    int haddr = (int)((lv == 0) ? ho : (unsigned)(size_t)(hdummy + lv));
                    const int hinc = (lanep == 0 && leave_u) ? -4 : 0;
                    float r3 = 1.7320508075688772f;
                    asm volatile("" : "+s"(r3));
                    const float hbr = botb[lv], bmr = botb[-h];
                    asm volatile("" ::: "memory");
                    quad_rev_all<124, true>(rc, rdA, rdB, rV, Dsl, Ssl, wr, rows, hbr, bmr, haddr, hinc, r3, nrows + ncols);
                    asm volatile("" ::: "memory");
                }
                // ---- block sums of S into the coarse grid (cells outside the grid hold S = 0) -------------------------
                // A lane's slots walk its row's local columns in order, so the cells of one coarse column form a run: the run
                // is summed in the lane and added when the coarse column changes.  Lanes of one row block reach those run ends
                // on different slots, so the adds of one instruction never meet on an address (one add per cell instead -- r
                // lanes times r slots on the same address -- took 2/3 of the kernel at order 5).  The LAST slot is different: it
                // ends every lane's run at once, and the r lanes of a row block (an aligned group: local column 63 - lane) then
                // hold pieces of the SAME coarse cell -- r same-address adds in one instruction, whose order is the LDS unit's
                // business.  Their pieces are therefore summed across the group in a fixed butterfly first and
                // one lane adds: the bits of S_coarse are a function of the launch geometry only.
                {
                    double *scrow = wl.Sc + arow * Tm;
                    int cl = (64 - lv) & 63;
                    int bcur = min((64 * h + cl) >> n, Tm - 1);
                    float run = 0.f;
#pragma unroll
                    for (int k = 0; k < 64; ++k) {
                        run += Ssl[k];
                        cl = (cl + 1) & 63;
                        const int bnext = min((64 * h + cl) >> n, Tm - 1);
                        if (k == 63) {
                            for (int off = 1; off < (1 << n); off <<= 1) run += __shfl_xor(run, off, 64);
                            if ((lv & ((1 << n) - 1)) == 0) unsafeAtomicAdd(scrow + bcur, (double)run);
                        } else if (bnext != bcur) {
                            unsafeAtomicAdd(scrow + bcur, (double)run); // ds_add_f64
                            run = 0.f;
                        }
                        bcur = bnext;
                    }
                }
            } // quadrant visits

            if (GRAD) {
                // ---- coarse gradient: R = 4-corner scatter of S_coarse / r^2, RBF derivative, both contractions ----------
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xc07f);
                // the pair's verdict for the exact fp64 pass: the grid maximum (above) or, in <= 3 channels, the condition number
                // of K in the STORED increments -- one fp32 value per coarse cell, shared by its r^2 fine cells, so
                // dK/dD_coarse = the block sum of S: c1 = sqrt(12) sum |Sc * Dc| / max(|K|, 0.1) > 150 (sweep_scaffold.h, "the repair rule")
                {
                    bool ill = false;
                    if (d <= 3) {
                        float cs = 0.f;
                        for (int e = lanep; e < Tm * Tm; e += 64) cs = __builtin_fmaf(fabsf((float)wl.Sc[e]), fabsf(wl.Dc[e]), cs);
                        const float c1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_sum_dpp<true>(cs)), 63));
                        ill = kfin_keep == kfin_keep && repair_ill(c1, repair_den(kfin_keep));
                    }
                    // (`lane`, not the per-pair opaque copy `lanep`: with `lanep == 0` hipcc reuses the mask it formed for the sweeps'
                    //  boundary lanes at the top of the pair, keeps it live across every sweep statement, and the 16-channel
                    //  4-wavefront symmetric instantiation -- the one that parks spilled values in AGPRs -- then returned column-side
                    //  sums that were wrong at the first and last point (soak of round 4, 91 of 6,000 cases); with `lane == 0`, or with
                    //  every lane storing, the same kernel is right.  Not understood beyond that: tests/test_gpu_dyadic.py pins the
                    //  instantiation.)
                    if (lane == 0) a.kflag[(size_t)i * a.B + j] = (canc_keep || ill) ? 1 : 0;
                }
                const float ns32 = (float)(-inv_h * 1.4426950408889634074);
                auto Sat = [&](int aa, int bb) -> float {
                    return (aa >= 0 && aa < Tm && bb >= 0 && bb < Tm) ? (float)(wl.Sc[aa * Tm + bb] * inv_r2) : 0.f;
                };
                // row side: lane m sums over the columns n
                if (lanep < T) {
                    const int m = lanep;
                    float acc[DPAD];
#pragma unroll
                    for (int c = 0; c < DPAD; ++c) acc[c] = 0.f;
                    for (int nn = 0; nn < T; ++nn) {
                        const float R = (Sat(m - 1, nn - 1) + Sat(m, nn)) - (Sat(m - 1, nn) + Sat(m, nn - 1));
                        const float *yr = yf + nn * DPAD;
                        float df[DPAD], e2 = 0.f;
#pragma unroll
                        for (int c = 0; c < DPAD; ++c) {
                            df[c] = xf[c] - yr[c];
                            e2 = __builtin_fmaf(df[c], df[c], e2);
                        }
                        const float rg = R * __builtin_amdgcn_exp2f(e2 * ns32);
#pragma unroll
                        for (int c = 0; c < DPAD; ++c) acc[c] = __builtin_fmaf(rg, df[c], acc[c]);
                    }
#pragma unroll
                    for (int c = 0; c < DPAD; ++c)
                        if (c < d) wl.rowacc[m * DPAD + c] += w_ij * m2h * acc[c];
                }
                // column side (Y is X): lane n sums over the rows m; x~_m comes from the lanes through LDS (the parked area)
                if (SYM) {
                    float *xl = wl.Dc; // (the increments are not needed any more) x~ rows [T][DPAD], then the parked sums
                    if (lanep < T) {
#pragma unroll
                        for (int c = 0; c < DPAD; ++c) xl[lanep * DPAD + c] = xf[c];
                    }
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                    float acc[DPAD];
#pragma unroll
                    for (int c = 0; c < DPAD; ++c) acc[c] = 0.f;
                    const int nn = min(lanep, T - 1);
                    const float *yr = yf + nn * DPAD;
                    for (int m = 0; m < T; ++m) {
                        const float R = (Sat(m - 1, nn - 1) + Sat(m, nn)) - (Sat(m - 1, nn) + Sat(m, nn - 1));
                        const float *xr = xl + m * DPAD;
                        float df[DPAD], e2 = 0.f;
#pragma unroll
                        for (int c = 0; c < DPAD; ++c) {
                            df[c] = xr[c] - yr[c];
                            e2 = __builtin_fmaf(df[c], df[c], e2);
                        }
                        const float rg = R * __builtin_amdgcn_exp2f(e2 * ns32);
#pragma unroll
                        for (int c = 0; c < DPAD; ++c) acc[c] = __builtin_fmaf(rg, df[c], acc[c]);
                    }
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                    if (lanep < T) { // d k(x_j, x_i) / d y_n = -(2/h) sum_m R G (y~_n - x~_m)
#pragma unroll
                        for (int c = 0; c < DPAD; ++c) xl[lanep * DPAD + c] = -(w_ji * m2h) * acc[c];
                    }
                }
            }
        } else if (GRAD && SYM) {
            for (int e = lane; e < T * DPAD; e += 64) wl.Dc[e] = 0.f; // idle wavefront: nothing to add to the column
        }

        if (GRAD && SYM) {
            __syncthreads(); // every wavefront has parked its column-side sums
            float *dstc = a.cslab + (size_t)item * (T * d);
            for (int e = tid; e < T * d; e += NT) {
                const int nn = e / d, c = e - nn * d;
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < DNW; ++w) s += wl_all[w].Dc[nn * DPAD + c];
                dstc[e] = s;
            }
        }
    }
    if (GRAD && row_ok) { // the segment's row-side sums
        const int tot = T * d;
        // (rseg_slot of sweep_scaffold.h, kept as a copy: it renumbers the registers of all 8 gradient kernels, and with the
        //  weights' copy above the unit is the parent's instruction for instruction)
        double *dstr = a.rseg + (((size_t)(kq + (int)blockIdx.x)) * DNW + wave) * (size_t)tot;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        for (int e = lane; e < tot; e += 64) {
            const int m = e / d, c = e - m * d;
            dstr[e] = (double)wl.rowacc[m * DPAD + c];
        }
    }
    remaining -= tr.ncol;
    ++kq;
    cstart = 0;
    } // row tiles of the range
}

bool dyad_supported(int T, int d, int n)
{
    if (n < 1 || n > 6 || T < 3 || T > DTMAX || d > 16) return false;
    const int P = (T - 1) << n;
    return P >= 64 && P <= 128;
}

// every launch: [A][B] bytes of cancellation flags for the fp64 pass; gradient launches behind them: [row segments][column slab].
// Small launches: every 4-row workgroup gets a CU of its own (measured, Gram + gradient, symmetric: N=16 T=20 order 2
// 0.086 -> 0.071 ms, N=30 T=5 order 5 0.091 -> 0.076; with two such workgroups per CU the 8-row form is faster again:
// N=64 T=20 0.165 against 0.257 ms -- half the rows per staged column trajectory)
WsPlan dyad_plan(int A, int B, int T, int d, int want_grad, bool sym)
{
    WsPlan w;
    const long long pairs = sym ? (long long)A * (A + 1) / 2 : (long long)A * B;
    const int nw = pairs <= 4ll * device_cu_count() ? 4 : 8;
    w.g = grad_geometry(A, B, T * d, sym, 0, 1, false, nw, (long long)device_cu_count());
    w.kflag = w.take(flag_area_bytes(A, B));
    if (want_grad) {
        w.rseg = w.take(w.g.rseg_bytes);
        w.cslab = w.take(w.g.cslab_bytes);
    }
    return w;
}

namespace {
template <int DPAD, int DNW>
int dyad_launch_variant(const GramProblem &p, DyadArgs &a, const GradGeom &g, bool grad, bool sym)
{
    if (g.tm.owned <= 0 || g.nitems <= 0) return SIGSVGD_OK;
    a.tm = g.tm;
    a.nitems = g.nitems;
    dim3 grid((unsigned)g.grid), block(DNW * 64);
    if (grad && sym)
        hipLaunchKernelGGL((gram_dyad_kernel<DPAD, true, true, DNW>), grid, block, 0, p.stream, a);
    else if (grad)
        hipLaunchKernelGGL((gram_dyad_kernel<DPAD, true, false, DNW>), grid, block, 0, p.stream, a);
    else if (DPAD == 8 && p.d <= 3 && sym)
        hipLaunchKernelGGL((gram_dyad_kernel<8, false, true, DNW, true>), grid, block, 0, p.stream, a);
    else if (DPAD == 8 && p.d <= 3)
        hipLaunchKernelGGL((gram_dyad_kernel<8, false, false, DNW, true>), grid, block, 0, p.stream, a);
    else if (sym)
        hipLaunchKernelGGL((gram_dyad_kernel<DPAD, false, true, DNW>), grid, block, 0, p.stream, a);
    else
        hipLaunchKernelGGL((gram_dyad_kernel<DPAD, false, false, DNW>), grid, block, 0, p.stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch gram_dyad_kernel");
    return SIGSVGD_OK;
}
} // namespace

int dyad_launch(const GramProblem &p)
{
    const bool grad = p.gradX_out != nullptr;
    const bool sym = (p.flags & SIGSVGD_FLAG_Y_IS_X) && p.A == p.B;
    const WsPlan w = dyad_plan(p.A, p.B, p.T, p.d, grad, sym);
    unsigned char *base = nullptr;
    int rc = ws_base(p, w, "dyad", base);
    if (rc) return rc;
    DyadArgs a{}; // (dyad_launch_variant takes the plan's tile map)
    fill_sweep_args(a, p, w, base);
    a.n = p.n;
    const GradGeom &g = w.g;
    if (g.NW == 4)
        rc = p.d <= 8 ? dyad_launch_variant<8, 4>(p, a, g, grad, sym) : dyad_launch_variant<16, 4>(p, a, g, grad, sym);
    else
        rc = p.d <= 8 ? dyad_launch_variant<8, 8>(p, a, g, grad, sym) : dyad_launch_variant<16, 8>(p, a, g, grad, sym);
    if (rc) return rc;
    return finish_launch(p, w, base, sym, g.tm, g.NW, p.gradX_out, p.dtype == SIGSVGD_F64);
}

} // namespace sigsvgd

SIG_EXEC_DEBUG_GETTER(dyad)
