// gram_fast_kernel and what launches an instantiation of it: the argument structs, the sweep statements, the kernel template,
// launch_grad / launch_variant / dispatch_variant.  Included by gram_fast.hip (RBF, RADIAL = 0: plans and entry points), by
// gram_fast_radial.hip (IMQ / rational quadratic, RADIAL = 1) and by gram_fast_wide.hip (RBF, the 32-channel layout DPAD = 32 for
// paths of 17 to 32 channels); no host state and no environment reads in here.
//
// Register-resident signature-kernel Gram forward/backward for the headline shapes:
// dyadic order 0, path length T <= 64, RBF static kernel, second-order stencil.
//
// Mapping (one wavefront per trajectory pair, as BASELINE.json north_star asks):
//   * lane l owns row l of the T x T static-kernel matrix G, row l of the (T-1)^2 increment matrix D,
//     row l+1 of the forward PDE solution K and row l of the reverse solution U;
//   * on anti-diagonal sigma (= row + column) every lane works on column sigma - l, so every
//     per-cell quantity a lane will need again (D, K_fwd / S, G) is filed under slot sigma & 63:
//     the slot index is a compile-time constant of the (fully unrolled) step, the same for all
//     lanes, so D and K_fwd live in 2 x 64 VGPRs and G in a [slot][lane] LDS image;
//   * neighbour rows are reached with wave-wide DPP shifts (no LDS round trip in the recurrence);
//   * the static kernel and the 4-corner increments run in fp64 (the increments cancel ~1e-2 of G); the two PDE
//     sweeps run in fp32 in DIFFERENCE FORM (a lane carries V = K[l+1][q] - K[l][q] along its row, see phase 2:
//     1.5e-7 on K, 1.9e-7 on the gradient against the fp64 oracle, where the plain fp32 stencil loses 1e-5);
//     everything that is only stored or contracted (D, K_fwd, G, S = K_fwd*U, R, gradient sums per pair) is fp32,
//     the reduction over pairs is fp64 (row side in registers, column side in grad_reduce_kernel).
//
// Per pair: phase 1 static kernel + increments (wrap-around skew, all lanes busy, 66 iterations);
// phase 2 forward sweep (K_fwd into the slots); phase 3 reverse sweep (U recurrence only, S = K_fwd*U
// overwrites K_fwd in its slot); phase 4 scatter R, R*G and both contractions in a second wrap-around
// pass (66 iterations, all lanes busy).  The two sweeps have on average half of their lanes outside the
// grid: their steps are hand-written (8 VALU + 2 SALU) and the idle lanes are switched off through EXEC windows
// read from a constant table (gradient launches of 64-point paths: built from immediates, "fixed windows" below).
// The kernel is bound by vector-instruction issue at two waves per SIMD, i.e. by its instruction count (5,430 per
// pair at C4): see DESIGN.md 5.1 / 5.1.1.
//
// A workgroup is NW wavefronts = NW consecutive rows i of X against a chunk of columns j; the
// column trajectory (centred on its first point, fp64 + fp32 copies) is staged once per j in LDS
// and shared by the NW pairs.  With Y == X each unordered pair {i<j} is solved once: the row-side
// contraction gives d k(x_i,x_j)/d x_i, the column-side sums (travelling accumulators, one wave
// rotation per sum and iteration) give d k(x_j,x_i)/d x_j.  Row-side gradients stay in per-lane fp64
// registers while a workgroup works on a row tile of its item range; column-side results of the NW waves
// are summed in fixed order through LDS.  Both leave the kernel through plain stores into per-segment /
// per-item slabs that grad_reduce_kernel adds up in a fixed order: no atomics, bit-reproducible results.
//
// Reference semantics: sigkernel _SigKernelGram.forward/backward [RECALLED, SURVEY.md App. A];
// static kernel src/kernels/_traj_kernels.py:176-195; callers src/inference/score.py:68-69.
#pragma once

#include <type_traits>

#include "sig_common.h"
#include "sweep_scaffold.h"

namespace sigsvgd {

// A wave's priority falls as it advances through its pair (static kernel 3, forward sweep 2, reverse sweep 1, gradient
// pass 0), so that the wave that is behind on a SIMD gets the issue slots and the waves stay in complementary phases.
// At C4: ordered gradient launches 8.47 -> 8.12 ms, forward-only 5.51 -> 5.12 ordered and 2.76 -> 2.59 symmetric.
// Symmetric gradient launches lose 1 % with it at two waves per SIMD (their gradient pass is twice as long) and keep the
// default arbitration there; at three waves per SIMD (paths of <= 32 points) they gain 3-8 % and use it; other priority patterns and a fixed priority for the younger half of the
// workgroup changed them by less than 0.5 %.
#define SIG_PRIO(n)                                                          \
    if (!GRAD || !SYM || (RING == 32 && NW == 4)) __builtin_amdgcn_s_setprio(n);

// Wave balance (the kernel's BAL): the launches that opt out of SIG_PRIO -- symmetric gradient kernels of
// 8-wave workgroups with fixed windows -- give the two waves of a SIMD one favoured stretch of a pair each instead.  A uniform
// schedule cannot separate two waves that are in the same phase, and a fixed priority only swaps winner and loser; here the
// half of the workgroup that goes first (the younger one, waves NW/2 .. NW-1: the loser of the default arbitration; BAL & 4:
// the older one) holds `s_setprio 1` from the top of the pair to a switch point, the other half from there to the pair's
// closing barrier.  BAL & 3 is the switch point: 1 the end of phase 1, 2 the end of phase 2, 3 between the two rounds of the
// reverse sweep.  Two s_setprio per wave and pair, each under a SCALAR branch on the wave index (s_setprio ignores EXEC: under a
// per-lane condition it would run in every wave).  Priorities change no arithmetic: the results are the BAL = 0 twin's bit for bit.
template <int BAL>
__device__ __forceinline__ void bal_top(bool first)
{
    if constexpr (BAL != 0) {
        if (first) __builtin_amdgcn_s_setprio(1);
    }
}
template <int BAL, int AT>
__device__ __forceinline__ void bal_switch(bool first)
{
    if constexpr (BAL != 0 && (BAL & 3) == AT) {
        if (first) __builtin_amdgcn_s_setprio(0);
        else __builtin_amdgcn_s_setprio(1);
    }
}
template <int BAL>
__device__ __forceinline__ void bal_end(bool first)
{
    if constexpr (BAL != 0) {
        if (!first) __builtin_amdgcn_s_setprio(0);
    }
}

constexpr int SIG_FAST_PHASES = 9; // stamp slots of the diagnostic build (launch_variant names them), per half of the workgroup

struct FastArgs {
    const void *X, *Y, *go; // (HALF = 2: Y is the launch's column images, [B][64 * 8 + 8] doubles, not the paths)
    void *K;
    // Gradient partial sums leave the kernel through plain stores into slabs that the reduction kernel below adds up in
    // a FIXED order (no atomics: the result is bit-reproducible run to run, and nothing needs zeroing):
    double *rseg; // [owned tiles + workgroups][NW][T*d] fp64: row-side sums of one (workgroup, row tile) segment
    float *cslab; // [items][T*d] fp32: column-side sums of one (row tile, column) item (symmetric launches)
    int io64, A, B, T, d, symw;
    TileMap tm;                   // row tiles owned by this launch, in the order of the enumeration (multi-GPU sharding)
    long long nitems;             // (owned row tile, column) items of the launch
    double inv_h;
    unsigned char *kflag;         // [A][B] (d <= 4 only): 1 where the pair's fp32 solution cancelled or K is ill-conditioned in
                                  // the increments: the launcher lets the coverage kernel solve those pairs exactly (fp64)
#ifdef SIGSVGD_PHASE_STAMPS
    unsigned long long *stamps; // diagnostic build only: [2][SIG_FAST_PHASES] shader-clock totals per phase, summed over the
                                // waves of the older and of the younger half of every workgroup
#endif
};
// The arguments of the RADIAL instantiations: FastArgs and the static kernel's kind, SIGSVGD_STATIC_IMQ or _RQ
// (wave-uniform).  A struct of its own, so that the RBF kernels keep their argument layout and with it their code.
struct FastRadialArgs : FastArgs {
    int kind;
};
template <int RADIAL>
using FastArgsOf = std::conditional_t<RADIAL != 0, FastRadialArgs, FastArgs>;

// ---- wave-wide shifts on the DPP path ----------------------------------------------------------
// wave_shr:1 (0x138): lane l reads lane l-1; wave_shl:1 (0x130): lane l reads lane l+1.
// With bound_ctrl = 0 a lane without a source keeps `old`, which carries the PDE boundary value.
__device__ __forceinline__ int dpp_shr1_i(int v, int bound)
{
    return __builtin_amdgcn_update_dpp(bound, v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ int dpp_shl1_i(int v, int bound)
{
    return __builtin_amdgcn_update_dpp(bound, v, 0x130, 0xF, 0xF, false);
}
// bound_ctrl = 1 forms: a lane without a source gets 0 and no `old` register has to be initialised.
__device__ __forceinline__ int dpp_shr1_z(int v) { return __builtin_amdgcn_mov_dpp(v, 0x138, 0xF, 0xF, true); }
__device__ __forceinline__ int dpp_shl1_z(int v) { return __builtin_amdgcn_mov_dpp(v, 0x130, 0xF, 0xF, true); }
// shifts carrying the PDE boundary value 1.0 = {hi 0x3FF00000, lo 0}: only the high word needs `old`
__device__ __forceinline__ double dpp_shr1_one(double v)
{
    const int lo = dpp_shr1_z(__double2loint(v));
    const int hi = dpp_shr1_i(__double2hiint(v), 0x3FF00000);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double dpp_shl1_one(double v)
{
    const int lo = dpp_shl1_z(__double2loint(v));
    const int hi = dpp_shl1_i(__double2hiint(v), 0x3FF00000);
    return __hiloint2double(hi, lo);
}
// Same shifts with the 1.0 boundary kept in a PERSISTENT destination: the lane without a source
// (0 for shr, 63 for shl) is never written, so once `dst` holds 1.0 there it stays -- no per-step
// re-initialisation of the DPP `old` operand.  (asm: hipcc would re-materialise `old` every step.)
// Hazard note (gfx9: VALU write of a VGPR -> DPP read of it needs 2 wait states; hipcc pads its own
// instructions, not the inside of an asm statement): the DPP source is the stencil result of the step
// before, and whether two instructions separate them is hipcc's scheduling decision, not a property of
// this source.  `scripts/check_dpp_hazards.py` therefore checks every DPP instruction of the built
// library on its disassembly; `_lib.build()` runs it and refuses a library that violates the rule, and
// tests/test_dpp_hazards.py runs it again in the CPU suite.  (An `s_nop 1` inside the asm string would
// also do, at ~5 % of the launch: measured.)
__device__ __forceinline__ void dpp_shr1_keep(double &dst, double v)
{
    int dlo = __double2loint(dst), dhi = __double2hiint(dst);
    asm("v_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(dlo) : "v"(__double2loint(v)));
    asm("v_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(dhi) : "v"(__double2hiint(v)));
    dst = __hiloint2double(dhi, dlo);
}
__device__ __forceinline__ void dpp_shl1_keep(double &dst, double v)
{
    int dlo = __double2loint(dst), dhi = __double2hiint(dst);
    asm("v_mov_b32_dpp %0, %1 wave_shl:1 row_mask:0xf bank_mask:0xf" : "+v"(dlo) : "v"(__double2loint(v)));
    asm("v_mov_b32_dpp %0, %1 wave_shl:1 row_mask:0xf bank_mask:0xf" : "+v"(dhi) : "v"(__double2hiint(v)));
    dst = __hiloint2double(dhi, dlo);
}
// fp32 forms of the persistent-boundary shifts (the PDE sweeps run in fp32, see the kernel header)
__device__ __forceinline__ void dpp_shr1_keep(float &dst, float v)
{
    asm("v_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(dst) : "v"(v));
}
__device__ __forceinline__ void dpp_shl1_keep(float &dst, float v)
{
    asm("v_mov_b32_dpp %0, %1 wave_shl:1 row_mask:0xf bank_mask:0xf" : "+v"(dst) : "v"(v));
}
__device__ __forceinline__ double dpp_shl1_zero(double v)
{
    return __hiloint2double(dpp_shl1_z(__double2hiint(v)), dpp_shl1_z(__double2loint(v)));
}
// wave_rol:1 (0x134): lane l reads lane l+1, lane 63 reads lane 0 (full-wave rotation)
__device__ __forceinline__ float dpp_rol1(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x134, 0xF, 0xF, false));
}
// rotate-and-add in ONE VALU instruction: returns acc[lane+1] + v.  (hipcc does not fold a wave_rol
// v_mov_b32_dpp into the add.)  `acc` is the shuffled source: same hazard, same build-time check as above.
__device__ __forceinline__ float add_rol1(float acc, float v)
{
    float out;
    asm("v_add_f32_dpp %0, %1, %2 wave_rol:1 row_mask:0xf bank_mask:0xf" : "=v"(out) : "v"(acc), "v"(v));
    return out;
}

// ---- one step of a PDE sweep, hand-scheduled (fp32 difference form, see phase 2 in the kernel) ------------------
// Every instruction of a step is listed here because the properties that make it fast are scheduling properties.
// Lanes outside the grid on a step (about half of them, averaged over a sweep) are switched off through EXEC, not
// through v_cmp / v_cndmask: the window of active lanes of anti-diagonal sigma, rows max(0, sigma-P+1) ..
// min(sigma, P-1), is a 64-bit constant per (P, sigma), read from a table in constant memory with scalar loads
// (SWEEP_MASK below) and moved into EXEC with one s_mov_b64.  Measured on MI355X at the kernel's occupancy
// (scripts/micro/exec_step.hip, two waves per SIMD): the v_cmp + 2 x v_cndmask step (11 VALU) 20.2 ns per step and
// wave, the EXEC step (8 VALU + 2 SALU) 10.4-11.0 ns -- the scalar moves issue in the shadow of the other wave's
// vector instructions, while the VCC round trip of the compare form stalls the chain far beyond its three
// instructions.  Per step:
//   s_mov exec,-1 ; DPP shift of `cur` into UP for EVERY lane (lane l reads l-1; a lane that has not started reads the
//     1.0 its neighbour still holds, so its diagonal operand is right when it starts; lane 0 keeps the boundary 1.0)
//   s_mov exec,window ; the stencil in difference form (5 VALU), the K_fwd slot store, only for lanes inside the grid:
//     a lane before its row starts keeps cur = 1, a finished lane keeps its last value (lane P-1: K[P,P]), and a
//     slot without a grid cell is never written (phase 4 relies on their zeros).
// The instruction after `v_add cur` and the s_mov are the 2 wait states of the gfx9 VALU-write -> DPP-read hazard
// (hipcc does not pad inside asm; scripts/check_dpp_hazards.py checks the built library).
// Eight steps form ONE asm statement (hipcc pads every asm statement with an `s_nop 0`, an issue slot of its own);
// EXEC is all ones again when the statement ends (the code around it may reload spilled registers).
struct SweepMasks {
    unsigned long long m[64][128]; // [P][sigma]
    constexpr SweepMasks() : m()
    {
        for (int P = 1; P < 64; ++P)
            for (int s = 0; s <= 2 * P - 2; ++s) {
                const int lo = s - P + 1 > 0 ? s - P + 1 : 0, hi = s < P - 1 ? s : P - 1;
                unsigned long long w = 0;
                for (int l = lo; l <= hi; ++l) w |= 1ull << l;
                m[P][s] = w;
            }
    }
};
__constant__ const SweepMasks SWEEP_MASK = SweepMasks();
// The same for paths of <= 32 points on the 32-slot ring (RING = 32 below): lanes 32..63 mirror lanes 0..31 (they own
// the same rows), so every window appears in both halves.
struct SweepMasks32 {
    unsigned long long m[32][64]; // [P][sigma]
    constexpr SweepMasks32() : m()
    {
        for (int P = 1; P < 32; ++P)
            for (int s = 0; s <= 2 * P - 2; ++s) {
                const int lo = s - P + 1 > 0 ? s - P + 1 : 0, hi = s < P - 1 ? s : P - 1;
                unsigned long long w = 0;
                for (int l = lo; l <= hi; ++l) w |= (1ull << l) | (1ull << (l + 32));
                m[P][s] = w;
            }
    }
};
__constant__ const SweepMasks32 SWEEP_MASK32 = SweepMasks32();

// EXECW writes the step's window into EXEC: SIG_WIN_TAB from the SGPR pair the table load filled, SIG_WIN_FIX (path length
// known at compile time, see "fixed windows" below) from two inline constants.
#define SIG_WIN_TAB(M) "s_mov_b64 exec, %[" M "]\n\t"
#define SIG_WIN_FIX(N) "s_bfm_b64 exec, %[w" N "], %[o" N "]\n\t"
#define SIG_FWD_STEP_X(UP, DIAG, G, KSL, EXECW)                                               \
    "s_mov_b64 exec, -1\n\t"                                                                  \
    "v_mov_b32_dpp %[" UP "], %[cur] wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"               \
    EXECW                                                                                     \
    "v_add_f32 %[t], %[cur], %[" UP "]\n\t"                                                   \
    "v_mul_f32 %[y], %[r3], %[t]\n\t"                                                         \
    "v_add_f32 %[t], %[t], %[" DIAG "]\n\t"                                                   \
    "v_fmac_f32 %[y], %[t], %[" G "]\n\t"                                                     \
    "v_fmac_f32 %[V], %[" G "], %[y]\n\t"                                                     \
    "v_add_f32 %[cur], %[" UP "], %[V]\n\t" KSL
#define SIG_FWD_STEP(UP, DIAG, G, KSL, M) SIG_FWD_STEP_X(UP, DIAG, G, KSL, SIG_WIN_TAB(M))
#define SIG_FWD_KSL(DIAG, K) "v_mov_b32 %[" K "], %[" DIAG "]\n\t"
#define SIG_FWD_NOKSL "v_max_f32 %[km], |%[cur]|, %[km]\n\t" // (forward-only launches: the largest |K| of the grid, in the hazard slot)
// few-channel forward-only launches also sum |K[l][q] * gamma[l][q]| over the cells: the forward half of the condition
// estimate sum |S * D| / |K| that decides whether the pair goes to the exact fp64 pass (sweep_scaffold.h, "the repair rule")
#define SIG_FWD_NOKSL_SD(DIAG, G) "v_max_f32 %[km], |%[cur]|, %[km]\n\tv_fma_f32 %[sd], |%[" DIAG "]|, |%[" G "]|, %[sd]\n\t"
#define SIG_REV_STEP_X(DN, DDIAG, G, K, EXECW)                                                \
    "s_mov_b64 exec, -1\n\t"                                                                  \
    "v_mov_b32_dpp %[" DN "], %[cur] wave_shl:1 row_mask:0xf bank_mask:0xf\n\t"               \
    EXECW                                                                                     \
    "v_add_f32 %[t], %[cur], %[" DN "]\n\t"                                                   \
    "v_mul_f32 %[y], %[r3], %[t]\n\t"                                                         \
    "v_add_f32 %[t], %[t], %[" DDIAG "]\n\t"                                                  \
    "v_fmac_f32 %[y], %[t], %[" G "]\n\t"                                                     \
    "v_fmac_f32 %[V], %[" G "], %[y]\n\t"                                                     \
    "v_add_f32 %[cur], %[" DN "], %[V]\n\t"                                                   \
    "v_mul_f32 %[" K "], %[" K "], %[" DDIAG "]\n\t"
#define SIG_REV_STEP(DN, DDIAG, G, K, M) SIG_REV_STEP_X(DN, DDIAG, G, K, SIG_WIN_TAB(M))

// steps sigma0 .. sigma0+7 of the forward sweep (sigma0 even): g, ksl point at slots sigma0 & 63 ..; mk at the
// windows of sigma0 ..
// MODE 0: K_fwd into the slots (gradient launches); 1: forward only, row maximum; 2: forward only, row maximum and the
// sum of |K00 * gamma| (few-channel launches)
template <int MODE>
__device__ __forceinline__ void sweep_fwd8(float &cur, float &upA, float &upB, float &V, const float *g, float *ksl,
                                           const unsigned long long *mk, const float r3, float &km, float &sd)
{
    float t, y;
    SIG_EXEC_MUST_BE_FULL("sweep_fwd8");
    const unsigned long long m0 = mk[0], m1 = mk[1], m2 = mk[2], m3 = mk[3], m4 = mk[4], m5 = mk[5], m6 = mk[6], m7 = mk[7];
    if constexpr (MODE == 2)
        asm volatile(SIG_FWD_STEP("upA", "upB", "g0", SIG_FWD_NOKSL_SD("upB", "g0"), "m0") SIG_FWD_STEP("upB", "upA", "g1", SIG_FWD_NOKSL_SD("upA", "g1"), "m1")
                     SIG_FWD_STEP("upA", "upB", "g2", SIG_FWD_NOKSL_SD("upB", "g2"), "m2") SIG_FWD_STEP("upB", "upA", "g3", SIG_FWD_NOKSL_SD("upA", "g3"), "m3")
                     SIG_FWD_STEP("upA", "upB", "g4", SIG_FWD_NOKSL_SD("upB", "g4"), "m4") SIG_FWD_STEP("upB", "upA", "g5", SIG_FWD_NOKSL_SD("upA", "g5"), "m5")
                     SIG_FWD_STEP("upA", "upB", "g6", SIG_FWD_NOKSL_SD("upB", "g6"), "m6") SIG_FWD_STEP("upB", "upA", "g7", SIG_FWD_NOKSL_SD("upA", "g7"), "m7")
                     "s_mov_b64 exec, -1\n\t"
                     : [cur] "+v"(cur), [upA] "+v"(upA), [upB] "+v"(upB), [V] "+v"(V), [t] "=&v"(t), [y] "=&v"(y), [km] "+v"(km), [sd] "+v"(sd)
                     : [g0] "v"(g[0]), [g1] "v"(g[1]), [g2] "v"(g[2]), [g3] "v"(g[3]), [g4] "v"(g[4]), [g5] "v"(g[5]),
                       [g6] "v"(g[6]), [g7] "v"(g[7]), [r3] "s"(r3), [m0] "s"(m0), [m1] "s"(m1), [m2] "s"(m2),
                       [m3] "s"(m3), [m4] "s"(m4), [m5] "s"(m5), [m6] "s"(m6), [m7] "s"(m7));
    else if constexpr (MODE == 0)
        asm volatile(SIG_FWD_STEP("upA", "upB", "g0", SIG_FWD_KSL("upB", "k0"), "m0")
                     SIG_FWD_STEP("upB", "upA", "g1", SIG_FWD_KSL("upA", "k1"), "m1")
                     SIG_FWD_STEP("upA", "upB", "g2", SIG_FWD_KSL("upB", "k2"), "m2")
                     SIG_FWD_STEP("upB", "upA", "g3", SIG_FWD_KSL("upA", "k3"), "m3")
                     SIG_FWD_STEP("upA", "upB", "g4", SIG_FWD_KSL("upB", "k4"), "m4")
                     SIG_FWD_STEP("upB", "upA", "g5", SIG_FWD_KSL("upA", "k5"), "m5")
                     SIG_FWD_STEP("upA", "upB", "g6", SIG_FWD_KSL("upB", "k6"), "m6")
                     SIG_FWD_STEP("upB", "upA", "g7", SIG_FWD_KSL("upA", "k7"), "m7")
                     "s_mov_b64 exec, -1\n\t"
                     : [cur] "+v"(cur), [upA] "+v"(upA), [upB] "+v"(upB), [V] "+v"(V), [t] "=&v"(t), [y] "=&v"(y),
                       [k0] "+v"(ksl[0]), [k1] "+v"(ksl[1]), [k2] "+v"(ksl[2]), [k3] "+v"(ksl[3]), [k4] "+v"(ksl[4]),
                       [k5] "+v"(ksl[5]), [k6] "+v"(ksl[6]), [k7] "+v"(ksl[7])
                     : [g0] "v"(g[0]), [g1] "v"(g[1]), [g2] "v"(g[2]), [g3] "v"(g[3]), [g4] "v"(g[4]), [g5] "v"(g[5]),
                       [g6] "v"(g[6]), [g7] "v"(g[7]), [r3] "s"(r3), [m0] "s"(m0), [m1] "s"(m1), [m2] "s"(m2),
                       [m3] "s"(m3), [m4] "s"(m4), [m5] "s"(m5), [m6] "s"(m6), [m7] "s"(m7));
    else
        asm volatile(SIG_FWD_STEP("upA", "upB", "g0", SIG_FWD_NOKSL, "m0") SIG_FWD_STEP("upB", "upA", "g1", SIG_FWD_NOKSL, "m1")
                     SIG_FWD_STEP("upA", "upB", "g2", SIG_FWD_NOKSL, "m2") SIG_FWD_STEP("upB", "upA", "g3", SIG_FWD_NOKSL, "m3")
                     SIG_FWD_STEP("upA", "upB", "g4", SIG_FWD_NOKSL, "m4") SIG_FWD_STEP("upB", "upA", "g5", SIG_FWD_NOKSL, "m5")
                     SIG_FWD_STEP("upA", "upB", "g6", SIG_FWD_NOKSL, "m6") SIG_FWD_STEP("upB", "upA", "g7", SIG_FWD_NOKSL, "m7")
                     "s_mov_b64 exec, -1\n\t"
                     : [cur] "+v"(cur), [upA] "+v"(upA), [upB] "+v"(upB), [V] "+v"(V), [t] "=&v"(t), [y] "=&v"(y), [km] "+v"(km)
                     : [g0] "v"(g[0]), [g1] "v"(g[1]), [g2] "v"(g[2]), [g3] "v"(g[3]), [g4] "v"(g[4]), [g5] "v"(g[5]),
                       [g6] "v"(g[6]), [g7] "v"(g[7]), [r3] "s"(r3), [m0] "s"(m0), [m1] "s"(m1), [m2] "s"(m2),
                       [m3] "s"(m3), [m4] "s"(m4), [m5] "s"(m5), [m6] "s"(m6), [m7] "s"(m7));
}
// steps sigma0+7 .. sigma0 of the reverse sweep (descending; sigma0 even): lower neighbour through wave_shl,
// S = K_fwd * U[l+1][q+1] replaces K_fwd in its slot
__device__ __forceinline__ void sweep_rev8(float &cur, float &dnA, float &dnB, float &V, const float *g, float *ksl,
                                           const unsigned long long *mk, const float r3)
{
    float t, y;
    SIG_EXEC_MUST_BE_FULL("sweep_rev8");
    const unsigned long long m0 = mk[0], m1 = mk[1], m2 = mk[2], m3 = mk[3], m4 = mk[4], m5 = mk[5], m6 = mk[6], m7 = mk[7];
    asm volatile(SIG_REV_STEP("dnA", "dnB", "g7", "k7", "m7") SIG_REV_STEP("dnB", "dnA", "g6", "k6", "m6")
                 SIG_REV_STEP("dnA", "dnB", "g5", "k5", "m5") SIG_REV_STEP("dnB", "dnA", "g4", "k4", "m4")
                 SIG_REV_STEP("dnA", "dnB", "g3", "k3", "m3") SIG_REV_STEP("dnB", "dnA", "g2", "k2", "m2")
                 SIG_REV_STEP("dnA", "dnB", "g1", "k1", "m1") SIG_REV_STEP("dnB", "dnA", "g0", "k0", "m0")
                 "s_mov_b64 exec, -1\n\t"
                 : [cur] "+v"(cur), [dnA] "+v"(dnA), [dnB] "+v"(dnB), [V] "+v"(V), [t] "=&v"(t), [y] "=&v"(y),
                   [k0] "+v"(ksl[0]), [k1] "+v"(ksl[1]), [k2] "+v"(ksl[2]), [k3] "+v"(ksl[3]), [k4] "+v"(ksl[4]),
                   [k5] "+v"(ksl[5]), [k6] "+v"(ksl[6]), [k7] "+v"(ksl[7])
                 : [g0] "v"(g[0]), [g1] "v"(g[1]), [g2] "v"(g[2]), [g3] "v"(g[3]), [g4] "v"(g[4]), [g5] "v"(g[5]),
                   [g6] "v"(g[6]), [g7] "v"(g[7]), [r3] "s"(r3), [m0] "s"(m0), [m1] "s"(m1), [m2] "s"(m2), [m3] "s"(m3),
                   [m4] "s"(m4), [m5] "s"(m5), [m6] "s"(m6), [m7] "s"(m7));
}

// ---- fixed windows: the sweep statements of a path length known at compile time ---------------------------------------------
// The table costs every statement a 16-SGPR scalar load and a wait on it, and the load cannot start before the statement
// before has ended (the same SGPRs hold its windows).  Where P is a template constant (the kernel's PFIX: paths of PFIX + 1
// points) the window of step sigma, lanes lo .. hi, is `s_bfm_b64 exec, hi - lo + 1, lo` with two inline constants (both
// <= 63; an empty window is width 0): no table, no load, no mask operands.  Everything else of a step -- instructions, order,
// operand roles, the alternating up / down registers, the slot stores, the EXEC = -1 around the DPP move and at the end of
// the statement -- is the table form's, so the results are the same bit for bit.  The windows differ from round to round, so
// each round has statements of its own; steps past 2P - 2 have no cell and no statement (they only shifted `cur` into an up /
// down register nobody reads again: forward, or that holds the same 1.0 already: reverse), so the last statement of a
// sweep of 2P - 1 = 125 (61) steps has five steps.
constexpr int sweep_win_lo(int P, int s) { return s - P + 1 > 0 ? s - P + 1 : 0; }
constexpr int sweep_win_hi(int P, int s) { return s < P - 1 ? s : P - 1; }
constexpr int sweep_win_w(int P, int s) { return sweep_win_hi(P, s) >= sweep_win_lo(P, s) ? sweep_win_hi(P, s) - sweep_win_lo(P, s) + 1 : 0; }
constexpr int sweep_win_o(int P, int s) { return sweep_win_w(P, s) ? sweep_win_lo(P, s) : 0; }
// what s_bfm_b64 D, w, o computes: ((1 << w[5:0]) - 1) << o[5:0]
constexpr unsigned long long sweep_bfm64(int w, int o) { return ((1ull << (w & 63)) - 1ull) << (o & 63); }
constexpr unsigned sweep_bfm32(int w, int o) { return ((1u << (w & 31)) - 1u) << (o & 31); }
// the immediates reproduce the tables bit for bit, empty steps included (the 32-slot ring: the same window in both halves of EXEC,
// one s_bfm_b32 each)
constexpr bool sweep_windows_match(int P)
{
    const SweepMasks tab;
    const SweepMasks32 tab32;
    for (int s = 0; s < 128; ++s) {
        const int w = sweep_win_w(P, s), o = sweep_win_o(P, s);
        if (w < 0 || w > 63 || o < 0 || o > 63) return false;
        if (sweep_bfm64(w, o) != tab.m[P][s]) return false;
        if (P < 32 && s < 64) {
            if (w > 31 || o > 31) return false;
            const unsigned h = sweep_bfm32(w, o);
            if ((((unsigned long long)h << 32) | h) != tab32.m[P][s]) return false;
        }
    }
    return true;
}
static_assert(sweep_windows_match(63), "fixed EXEC windows differ from SWEEP_MASK at P = 63");
static_assert(sweep_windows_match(31), "fixed EXEC windows differ from SWEEP_MASK / SWEEP_MASK32 at P = 31");

#define SIG_WIN_OPS(k) [w##k] "n"(sweep_win_w(PFIX, SIGMA0 + k)), [o##k] "n"(sweep_win_o(PFIX, SIGMA0 + k))
// steps SIGMA0 .. SIGMA0 + NS - 1 of the forward sweep of a gradient launch (sweep_fwd8<0> with immediates); NS = 8, or 5 for
// the statement that ends the sweep
template <int PFIX, int SIGMA0, int NS>
__device__ __forceinline__ void sweep_fwd_fixed(float &cur, float &upA, float &upB, float &V, const float *g, float *ksl, const float r3)
{
    static_assert((NS == 8 || NS == 5) && SIGMA0 % 8 == 0 && SIGMA0 + NS <= 2 * PFIX - 1, "statement shape");
    float t, y;
    SIG_EXEC_MUST_BE_FULL("sweep_fwd_fixed");
    if constexpr (NS == 8)
        asm volatile(SIG_FWD_STEP_X("upA", "upB", "g0", SIG_FWD_KSL("upB", "k0"), SIG_WIN_FIX("0"))
                     SIG_FWD_STEP_X("upB", "upA", "g1", SIG_FWD_KSL("upA", "k1"), SIG_WIN_FIX("1"))
                     SIG_FWD_STEP_X("upA", "upB", "g2", SIG_FWD_KSL("upB", "k2"), SIG_WIN_FIX("2"))
                     SIG_FWD_STEP_X("upB", "upA", "g3", SIG_FWD_KSL("upA", "k3"), SIG_WIN_FIX("3"))
                     SIG_FWD_STEP_X("upA", "upB", "g4", SIG_FWD_KSL("upB", "k4"), SIG_WIN_FIX("4"))
                     SIG_FWD_STEP_X("upB", "upA", "g5", SIG_FWD_KSL("upA", "k5"), SIG_WIN_FIX("5"))
                     SIG_FWD_STEP_X("upA", "upB", "g6", SIG_FWD_KSL("upB", "k6"), SIG_WIN_FIX("6"))
                     SIG_FWD_STEP_X("upB", "upA", "g7", SIG_FWD_KSL("upA", "k7"), SIG_WIN_FIX("7"))
                     "s_mov_b64 exec, -1\n\t"
                     : [cur] "+v"(cur), [upA] "+v"(upA), [upB] "+v"(upB), [V] "+v"(V), [t] "=&v"(t), [y] "=&v"(y),
                       [k0] "+v"(ksl[0]), [k1] "+v"(ksl[1]), [k2] "+v"(ksl[2]), [k3] "+v"(ksl[3]), [k4] "+v"(ksl[4]),
                       [k5] "+v"(ksl[5]), [k6] "+v"(ksl[6]), [k7] "+v"(ksl[7])
                     : [g0] "v"(g[0]), [g1] "v"(g[1]), [g2] "v"(g[2]), [g3] "v"(g[3]), [g4] "v"(g[4]), [g5] "v"(g[5]),
                       [g6] "v"(g[6]), [g7] "v"(g[7]), [r3] "s"(r3), SIG_WIN_OPS(0), SIG_WIN_OPS(1), SIG_WIN_OPS(2),
                       SIG_WIN_OPS(3), SIG_WIN_OPS(4), SIG_WIN_OPS(5), SIG_WIN_OPS(6), SIG_WIN_OPS(7));
    else
        asm volatile(SIG_FWD_STEP_X("upA", "upB", "g0", SIG_FWD_KSL("upB", "k0"), SIG_WIN_FIX("0"))
                     SIG_FWD_STEP_X("upB", "upA", "g1", SIG_FWD_KSL("upA", "k1"), SIG_WIN_FIX("1"))
                     SIG_FWD_STEP_X("upA", "upB", "g2", SIG_FWD_KSL("upB", "k2"), SIG_WIN_FIX("2"))
                     SIG_FWD_STEP_X("upB", "upA", "g3", SIG_FWD_KSL("upA", "k3"), SIG_WIN_FIX("3"))
                     SIG_FWD_STEP_X("upA", "upB", "g4", SIG_FWD_KSL("upB", "k4"), SIG_WIN_FIX("4"))
                     "s_mov_b64 exec, -1\n\t"
                     : [cur] "+v"(cur), [upA] "+v"(upA), [upB] "+v"(upB), [V] "+v"(V), [t] "=&v"(t), [y] "=&v"(y),
                       [k0] "+v"(ksl[0]), [k1] "+v"(ksl[1]), [k2] "+v"(ksl[2]), [k3] "+v"(ksl[3]), [k4] "+v"(ksl[4])
                     : [g0] "v"(g[0]), [g1] "v"(g[1]), [g2] "v"(g[2]), [g3] "v"(g[3]), [g4] "v"(g[4]), [r3] "s"(r3),
                       SIG_WIN_OPS(0), SIG_WIN_OPS(1), SIG_WIN_OPS(2), SIG_WIN_OPS(3), SIG_WIN_OPS(4));
}
// steps SIGMA0 + NS - 1 .. SIGMA0 of the reverse sweep (sweep_rev8 with immediates): a step keeps the down registers it has
// in the 8-step statement (even steps dnB, odd steps dnA), so the 5-step statement starts on dnB
template <int PFIX, int SIGMA0, int NS>
__device__ __forceinline__ void sweep_rev_fixed(float &cur, float &dnA, float &dnB, float &V, const float *g, float *ksl, const float r3)
{
    static_assert((NS == 8 || NS == 5) && SIGMA0 % 8 == 0 && SIGMA0 + NS <= 2 * PFIX - 1, "statement shape");
    float t, y;
    SIG_EXEC_MUST_BE_FULL("sweep_rev_fixed");
    if constexpr (NS == 8)
        asm volatile(SIG_REV_STEP_X("dnA", "dnB", "g7", "k7", SIG_WIN_FIX("7")) SIG_REV_STEP_X("dnB", "dnA", "g6", "k6", SIG_WIN_FIX("6"))
                     SIG_REV_STEP_X("dnA", "dnB", "g5", "k5", SIG_WIN_FIX("5")) SIG_REV_STEP_X("dnB", "dnA", "g4", "k4", SIG_WIN_FIX("4"))
                     SIG_REV_STEP_X("dnA", "dnB", "g3", "k3", SIG_WIN_FIX("3")) SIG_REV_STEP_X("dnB", "dnA", "g2", "k2", SIG_WIN_FIX("2"))
                     SIG_REV_STEP_X("dnA", "dnB", "g1", "k1", SIG_WIN_FIX("1")) SIG_REV_STEP_X("dnB", "dnA", "g0", "k0", SIG_WIN_FIX("0"))
                     "s_mov_b64 exec, -1\n\t"
                     : [cur] "+v"(cur), [dnA] "+v"(dnA), [dnB] "+v"(dnB), [V] "+v"(V), [t] "=&v"(t), [y] "=&v"(y),
                       [k0] "+v"(ksl[0]), [k1] "+v"(ksl[1]), [k2] "+v"(ksl[2]), [k3] "+v"(ksl[3]), [k4] "+v"(ksl[4]),
                       [k5] "+v"(ksl[5]), [k6] "+v"(ksl[6]), [k7] "+v"(ksl[7])
                     : [g0] "v"(g[0]), [g1] "v"(g[1]), [g2] "v"(g[2]), [g3] "v"(g[3]), [g4] "v"(g[4]), [g5] "v"(g[5]),
                       [g6] "v"(g[6]), [g7] "v"(g[7]), [r3] "s"(r3), SIG_WIN_OPS(0), SIG_WIN_OPS(1), SIG_WIN_OPS(2),
                       SIG_WIN_OPS(3), SIG_WIN_OPS(4), SIG_WIN_OPS(5), SIG_WIN_OPS(6), SIG_WIN_OPS(7));
    else
        asm volatile(SIG_REV_STEP_X("dnB", "dnA", "g4", "k4", SIG_WIN_FIX("4"))
                     SIG_REV_STEP_X("dnA", "dnB", "g3", "k3", SIG_WIN_FIX("3")) SIG_REV_STEP_X("dnB", "dnA", "g2", "k2", SIG_WIN_FIX("2"))
                     SIG_REV_STEP_X("dnA", "dnB", "g1", "k1", SIG_WIN_FIX("1")) SIG_REV_STEP_X("dnB", "dnA", "g0", "k0", SIG_WIN_FIX("0"))
                     "s_mov_b64 exec, -1\n\t"
                     : [cur] "+v"(cur), [dnA] "+v"(dnA), [dnB] "+v"(dnB), [V] "+v"(V), [t] "=&v"(t), [y] "=&v"(y),
                       [k0] "+v"(ksl[0]), [k1] "+v"(ksl[1]), [k2] "+v"(ksl[2]), [k3] "+v"(ksl[3]), [k4] "+v"(ksl[4])
                     : [g0] "v"(g[0]), [g1] "v"(g[1]), [g2] "v"(g[2]), [g3] "v"(g[3]), [g4] "v"(g[4]), [r3] "s"(r3),
                       SIG_WIN_OPS(0), SIG_WIN_OPS(1), SIG_WIN_OPS(2), SIG_WIN_OPS(3), SIG_WIN_OPS(4));
}
// the statements of steps S0 .. S1 - 1 of one round (S0 a multiple of 8), ascending / descending; slots are sigma & 63
template <int PFIX, int S0, int S1>
__device__ __forceinline__ void sweep_fwd_fixed_round(float &cur, float &upA, float &upB, float &V, const float *Dsl, float *Ksl, const float r3)
{
    if constexpr (S0 < S1) {
        sweep_fwd_fixed<PFIX, S0, (S1 - S0 < 8 ? S1 - S0 : 8)>(cur, upA, upB, V, Dsl + (S0 & 63), Ksl + (S0 & 63), r3);
        sweep_fwd_fixed_round<PFIX, S0 + 8, S1>(cur, upA, upB, V, Dsl, Ksl, r3);
    }
}
template <int PFIX, int S0, int S1>
__device__ __forceinline__ void sweep_rev_fixed_round(float &cur, float &dnA, float &dnB, float &V, const float *Dsl, float *Ksl, const float r3)
{
    if constexpr (S0 < S1) {
        sweep_rev_fixed_round<PFIX, S0 + 8, S1>(cur, dnA, dnB, V, Dsl, Ksl, r3);
        sweep_rev_fixed<PFIX, S0, (S1 - S0 < 8 ? S1 - S0 : 8)>(cur, dnA, dnB, V, Dsl + (S0 & 63), Ksl + (S0 & 63), r3);
    }
}

// ---- fp64 forward sweep of a pair whose fp32 solution cancelled ----------------------------------------------------
// The fp32 sweeps resolve K to ~1e-7 of the LARGEST value on the pair's grid.  Where the discrete solution oscillates
// (rough paths in few channels against a narrow static kernel: K(x, y) passes through zero, turns negative), the value at
// the far corner can be a small remainder of much larger intermediate values and its relative error grows by their ratio
// (measured: up to 1.9e-5 per entry at T = 64, d = 2, against 1e-6 without cancellation).  A wavefront that sees
// max |K_grid| > 4 * max(|K[P][P]|, 0.1) in one of its pairs therefore repeats the forward sweep in fp64 from the
// increments it still holds (fp32 storage of fp64 differences: 2e-8) and stores that value over the first; the gradient
// keeps the fp32 solution (its error is relative to the largest gradient entry: 1.4e-6 in those regimes).  Fully unrolled
// (the slots are registers), plain selects instead of EXEC windows: it runs on a few pairs of a rough launch and on none of
// a smooth one.  Same indexing as the fp32 step: lane l computes K[l+1][q+1] on step sigma = l + q from cur = K[l+1][q],
// up = K[l][q+1] (lane l-1 before its own step) and the up of the step before = K[l][q].
// What the block costs the pairs that do not take it (same-box A/B against the build without it): C4 4.90 -> 4.88 ms,
// N=1024 T=32 1.36 -> 1.34 ms, forward-only launches +2 %, and +4 us on the 41 us launch of N=128, T=32 -- there the
// 168-register kernel now reloads ~20 loop invariants per pair from scratch, whatever shape the block takes (a rolled
// re-solve from the staged coordinates, a call, parking live values in memory around it: all measured, all worse).
template <int RING>
__device__ __forceinline__ double resweep_fwd_fp64(const float (&Dsl)[RING], int P, int lrow)
{
    double cur = 1.0, upprev = 1.0;
    // (opaque copies: the compiler otherwise hoists the 126 lane-window predicates out of the kernel's pair loop -- they
    //  depend on nothing a pair changes -- and keeps them in spilled SGPRs for the whole kernel)
    asm volatile("" : "+v"(lrow), "+s"(P));
    const bool rowv = lrow < P;
#pragma unroll
    for (int s0 = 0; s0 < 2 * RING - 3; s0 += 8) {
        if (s0 <= 2 * P - 2) { // (uniform; steps past 2P-2 have no lane inside the grid)
#pragma unroll
            for (int s = s0; s < s0 + 8 && s < 2 * RING - 3; ++s) {
                const double up = dpp_shr1_one(cur); // lane 0 (and, two rows per wavefront, the lane after the idle row 31): 1.0
                float gf = Dsl[s & (RING - 1)];
                asm volatile("" : "+v"(gf)); // (a slot serves steps s and s + RING: converted twice, not kept as a double in between)
                const double g = (double)gf;
                const double t = cur + up;
                const double nw = (t - upprev) + g * __builtin_fma(g, t + upprev, 1.7320508075688772 * t);
                cur = (rowv && (unsigned)(s - lrow) < (unsigned)P) ? nw : cur;
                upprev = up;
            }
        }
    }
    return cur;
}

// ---- the heavy-tailed static kernels of the RADIAL instantiations --------------------------------------------
// 1 / sqrt(x) for x = 1 + s >= 1: the hardware estimate and one step of third order (e = 1 - x y^2; y (1 + e/2 + 3 e^2/8)),
// which is what the math library's rsqrt does after its range and special-value handling -- none of which 1 + s needs (a NaN
// stays a NaN and poisons its row / column of K, as RBF's does).  The increments are rounded to fp32 right after.
__device__ __forceinline__ double rsqrt_ge1(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    const double e = __builtin_fma(-(x * y), y, 1.0);
    return __builtin_fma(y * e, __builtin_fma(e, 0.375, 0.5), y);
}

// [slot][lane] image of G (then R*G) with row stride 65 floats: every in-sweep access is
// lane*4 + constant (one ds instruction with an immediate offset, nothing to keep in registers),
// and the transposed read of the symmetric pass ((m+n)&63)*65 + m hits 32 distinct banks.
constexpr int GS_STRIDE = 65;
constexpr int GS_WAVE = 64 * GS_STRIDE;
using f32x2 = __attribute__((ext_vector_type(2))) float;

__device__ __forceinline__ int gs_index(int slot, int lane) { return slot * GS_STRIDE + lane; }

// DPAD: channels of the layout, 4, 8, 16 or 32 (d is zero-padded to it).  32 (gram_fast_wide.hip): 4-wave
// workgroups at one wave per SIMD, phase 1 in two blocks of 16 channels, general windows only.
// LP: the last of the DPAD channels is padding (d == DPAD - 1, e.g. the 7-DoF arm at DPAD = 8; DPAD = 4, 8 and 32): its FMA in the
// static kernel and its travelling column sum are dropped.
// RING: slots per lane = length of the column ring.  64 in general; 32 for paths of <= 32 points (T <= 32), where the
// skewed phases 1 and 4 take 34 iterations instead of 66 and a wavefront solves TWO pairs at once: lanes 0..31 own the
// points of trajectory i, lanes 32..63 those of trajectory i + 1, against the SAME column trajectory j (time index =
// lane & 31).  The wave-wide machinery stays intact: the lane next to the seam, row 31, has no cells for T <= 32 and
// therefore holds the boundary value 1 that row 0 of the second pair needs from its DPP shift (and S = 0 for the
// scatter); each of the 64 travelling column sums collects one of the two rows at every time index on its way through 32
// consecutive lanes, and the two sums of a column (they end 32 lanes apart) are added when the workgroup's waves are --
// exactly the sum over the tile's rows the column side wants.  (Round 2 let lanes 32..63 mirror lanes 0..31: the same
// work twice.)
// PFIX: 0, or the launch's P = T - 1 as a compile-time constant: the sweeps then build their EXEC windows from immediates (see
// "fixed windows" above; gradient kernels of the 64-slot ring at T = 64).  Nothing else of the kernel depends on it.
// BAL: 0, or the wave-balance schedule of the pair (see bal_top above); it adds the s_setprio and their branches, nothing else.
// HALF: 0, or 1: the younger half of the workgroup runs half a pair behind the older one (see half_younger in the kernel; DESIGN.md
// 5.1.2).  The symmetric 7-of-8-channel gradient kernel with fixed windows only; it has its own priority schedule (BAL = 0).
// 2: the same, and the columns are staged from images that fast_column_image_kernel formed once per launch (see IMG in the kernel;
// a value of HALF and not a parameter of its own, so that every other instantiation keeps its name).
// RADIAL: 0 the RBF static kernel; 1 the inverse multiquadric or the rational quadratic, told apart by the wave-uniform a.kind
// (DESIGN.md 5.18).  Phase 1 then evaluates k = phi(s), s = |x~ - y~|^2 inv_h clamped at 0, in place of the exponential, and the
// G image holds -phi'(s) where RBF's holds k (for RBF the two are the same number); nothing after `rd = g - gprev` depends on it.
// General windows only (no PFIX, no BAL); instantiated in gram_fast_radial.hip.
template <int DPAD, int NW, bool GRAD, bool SYM, bool LP, int RING = 64, int PFIX = 0, int BAL = 0, int RADIAL = 0, int HALF = 0>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(
    GRAD ? ((RING == 32 && NW == 4 && DPAD <= 8) ? 3 : 1) : ((DPAD <= 8) ? 3 : (DPAD <= 16) ? 2 : 1),
    GRAD ? ((RING == 32 && NW == 4 && DPAD <= 8) ? 3 : (DPAD <= 16) ? 2 : 1) : ((DPAD <= 8) ? 3 : (DPAD <= 16) ? 2 : 1)))) void gram_fast_kernel(FastArgsOf<RADIAL> a)
{
    constexpr int DC = LP ? DPAD - 1 : DPAD; // channels that can be non-zero
    constexpr int NT = NW * 64;
    constexpr int RM = RING - 1;
    constexpr int RPW = (RING == 32) ? 2 : 1; // rows (trajectories i) per wavefront
    constexpr int NWR = NW * RPW;             // rows per tile
    static_assert(RADIAL == 0 || (PFIX == 0 && BAL == 0), "the radial kinds: general windows, no wave balance");
    static_assert(BAL == 0 || (GRAD && SYM && RING == 64 && NW == 8 && PFIX != 0 && (BAL & 3) != 0 && BAL < 8),
                  "wave balance: the symmetric gradient kernels with fixed windows on 8-wave workgroups (the ones SIG_PRIO leaves alone)");
    static_assert(HALF == 0 || (GRAD && SYM && LP && DPAD == 8 && RING == 64 && NW == 8 && PFIX != 0 && BAL == 0 && RADIAL == 0),
                  "half offset: the symmetric 7-of-8-channel gradient kernel with fixed windows on 8-wave workgroups; a schedule of its own");
    // y rows are stored twice (row r and r + 64) so that the skewed row (t - lane) & 63 becomes
    // (64 - lane) + t: a per-lane base plus a compile-time offset.
    // Row strides are padded (YDS doubles / YFS floats) so that the 16 lanes a ds_read_b128 services per
    // cycle -- consecutive rows, one per lane -- start on 16 distinct 16-byte bank groups: with the
    // natural 64-B (fp64, d<=8) / 32-B (fp32) rows they alias 4-way / 2-way (measured: 54 % of all LDS
    // cycles were bank-conflict cycles).
    constexpr int YDS = DPAD + 2; // doubles per fp64 row: 80 B at DPAD=8 -> 80*l mod 256 distinct for 16 l
    constexpr int YFS = (DPAD == 4) ? 12 : DPAD + 4; // floats per fp32 row: 48 B at DPAD<=8, 80 B at 16
    // (sized by the ring: with 32 slots a 4-wave workgroup needs 47 KB instead of 84, three of them fit a CU)
    constexpr int GSS = HALF ? 64 : GS_STRIDE; // (HALF: no padding word per slot -- every access is [slot][lane], and the LDS is needed)
    constexpr int GSW = RING * GSS; // floats of a wavefront's [slot][lane] image
    __shared__ float Gs_all[GRAD ? NW * GSW : 1];
    __shared__ __align__(16) double yd[2 * RING * YDS];
    __shared__ double ynd[HALF ? 1 : 2 * RING]; // (HALF is LP: the norm rides in the padded channel of yd, nobody reads ynd)
    // HALF: the younger half of the workgroup runs its phases 3-4 on column j while the older half runs them on column j + 1, so
    // what those phases read of a column -- yf and yref -- exists twice, [pb] = the pair's parity in the workgroup's range
    constexpr int YFB = 2 * RING * YFS; // floats of one yf buffer
    __shared__ double yref[HALF ? 2 * DPAD : DPAD];
    __shared__ __align__(16) float yf[GRAD ? (HALF ? 2 : 1) * YFB : 1];
    // HALF: the younger half's parked column sums [wave - NW/2][column][c] (its G image is rewritten by its next phase 1 before
    // the sync that adds them up), and the older half's partial block sum of an item, kept until that sync
    __shared__ float ypark[HALF ? (NW / 2) * RING * DC : 1];
    __shared__ float ycarry[HALF ? RING * DC : 1];

    const int tid = threadIdx.x, lane = tid & 63;
    // (scalar: row index, row pointers and the per-wave LDS bases then live in SGPRs; as a vector value hipcc hoists the
    //  row's element addresses out of the column loop as 64-bit VGPR pairs and spills them)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & RM; // the row this lane owns
    const bool bal_first = (BAL & 4) ? wave < NW / 2 : wave >= NW / 2; // (BAL: this wave's half holds the priority first; scalar)
    // Half offset (the kernel's HALF): the younger half of the workgroup (waves NW/2 .. NW-1) passes the pair's
    // sync block between phase 2 and phase 3 instead of after phase 4.  Between two syncs it then runs [phases 3-4 of pair j,
    // phases 0-2 of pair j + 1] beside the older half's [phases 0-2, phases 3-4 of pair j + 1]: each SIMD holds one wave in the
    // fp64 static kernel or the forward sweep and one in the reverse sweep or the gradient pass.  One copy of the phases; the two
    // sync sites are the same barrier events, each under a scalar branch on the wave index.
    const bool half_younger = HALF != 0 && wave >= NW / 2; // (scalar)
    int pb = 0; // HALF: which yf / yref buffer holds the column of the pair in work (flips with every pair of the range; scalar)
    const int T = a.T, d = a.d, P = T - 1, io64 = a.io64;
    // Work distribution: the items of a launch -- (owned row tile, column), tile-major; symmetric launches only the
    // columns from the tile's first row on -- all cost the same (the NW waves of a workgroup meet at a barrier per
    // column), so they are split into contiguous equal ranges, one per workgroup of a grid that fills the chip once.
    // A range touches few row tiles: the per-lane row-side gradient accumulators live in registers across the columns of
    // a tile and are stored to the (workgroup, tile) segment's slot when the range leaves it; and every next column is known
    // in advance, so its loads are in flight during the current pair (the round-1/2 work queue exposed an atomic and a
    // load round trip per chunk: 63 % of the wave cycles at N=128, T=32 with its single-column chunks).
#ifdef SIGSVGD_PHASE_STAMPS
    unsigned long long ph_[SIG_FAST_PHASES] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tlast_ = __builtin_amdgcn_s_memtime();
#endif
    int j0 = 0, j1 = 0;
    float *Gs = Gs_all + (GRAD ? wave * GSW : 0);
    const double inv_h = a.inv_h;
    const float m2h = (float)(-2.0 * inv_h * 3.46410161513775459); // the G image holds G / sqrt(12)

    // K_fwd, then S = K_fwd * U, of this lane's row, one slot per anti-diagonal (slot = (column + lane) & 63).
    // Zeroed per pair right before the forward sweep (64 moves, 0.5 % of a pair): the sweeps write a slot only while
    // its cell is inside the grid, so the slots without a grid cell (column >= P or lane >= P) read 0 in the phase-4
    // pass, which takes all 64 slots unmasked -- and the 64 registers are free during staging and phase 1.
    float Ksl[RING];
    double gacc[DPAD]; // per-lane fp64 accumulators of d sum_j w_ij k(x_i, y_j) / d x_i[lane, c]
    double xraw[DPAD]; // raw row of x_i owned by this lane (fp64 copy of the fp32/fp64 input; exact)

    // ---- staging of column trajectory y_j: element e -> (t = e / DPAD, c = e % DPAD) -------------
    constexpr int EPT = (64 * DPAD + NT - 1) / NT; // elements per thread
    // RAW_STAGE: the loads of the next column are issued at the top of a pair "to be in flight during it", but load_any's
    // conversion is a use: an s_waitcnt vmcnt(0) after each of two dependent round trips to memory at the top of every pair,
    // in all waves of the workgroup at once (the "loop top" stamp: 2.7 % of the wave-cycles of a C4 launch).  With RAW_STAGE
    // stage_load keeps the raw bits and stage_store converts; the row x_i is consumed once per tile and the staged words
    // once before the pair's closing barrier (below), so that no wait stands between the top of a pair and its end.
    // Measured per launch kind against the build without it: the symmetric 8-channel gradient kernels of
    // the 64-slot ring gain (C4: -1 ... -2 %); ordered and forward-only launches, the 4-channel kernels and the 32-slot ring
    // LOSE 0.5-4 % and keep the conversion at the load.
    constexpr bool RAW_STAGE = GRAD && SYM && RING == 64 && DPAD == 8;
    struct RawElem { unsigned lo, hi; }; // the element's bits: an fp32 value in `lo`, an fp64 value in both words
    RawElem raw_v[EPT], raw_r[EPT];      // (RAW_STAGE)
    double stage_v[EPT], stage_r[EPT];
    // Column images (HALF = 2; DESIGN.md 5.1, "Column images"): a launch stages 66,048 items at C4 and has 1,024 distinct columns,
    // and what stage_store forms of a column -- the centred fp64 values, the scaled norm of every point (an xor tree of three
    // dependent LDS round trips) and the first point -- is the same for every item of the column.  fast_column_image_kernel
    // (gram_fast.hip) forms it once per launch, [64][8] doubles as yd holds them (channel 7: the norm) and the 8 doubles of yref;
    // a.Y points at these images, stage_load is one 8-byte load per thread (eight threads: one more for yref) and stage_store
    // converts for yf and stores.  Same operands, same operations, same bits as HALF = 1.
    constexpr bool IMG = HALF == 2;
    constexpr int IMG_DOUBLES = 64 * 8 + 8; // doubles of one column's image (4,160 B)
    // -DSIG_EXPERIMENT_STAGE_COPY, timing experiment only (results are garbage; profiles/column_images_bound.txt): the bound that
    // was taken before the images were built.  The HALF = 1 twin (SIGSVGD_COLUMN_IMAGES=off) stages a column as if its image lay
    // ready in memory -- one 8-byte load per thread at the loop top, plain stores in the window, no subtraction, no norm tree.
#ifdef SIG_EXPERIMENT_STAGE_COPY
    constexpr bool STAGE_COPY = HALF == 1;
#else
    constexpr bool STAGE_COPY = false;
#endif
    // (word by word, the high word under its own condition: one register per word on both paths, nothing to move or widen
    //  -- which would be a use -- after the load)
    auto load_raw = [&](const void *b, size_t idx) -> RawElem {
        const char *p = static_cast<const char *>(b) + (idx << (io64 ? 3 : 2));
        RawElem r;
        r.lo = *reinterpret_cast<const unsigned *>(p);
        r.hi = 0u;
        if (io64) r.hi = *reinterpret_cast<const unsigned *>(p + 4);
        return r;
    };
    auto raw_value = [&](const RawElem &r) -> double { // what load_any returns for the same element
        return io64 ? __hiloint2double((int)r.hi, (int)r.lo) : (double)__uint_as_float(r.lo);
    };
    auto stage_load = [&](int j) {
        if constexpr (IMG) {
            static_assert(EPT == 1 && NT == 64 * DPAD, "column images: thread e holds element e");
            raw_v[0] = raw_r[0] = RawElem{0u, 0u};
            if (j < a.B) {
                const uint2 *img = reinterpret_cast<const uint2 *>(static_cast<const double *>(a.Y) + (size_t)j * IMG_DOUBLES);
                const uint2 w = img[tid];
                raw_v[0] = RawElem{w.x, w.y};
                if (tid < DPAD) { // (the threads that store yref)
                    const uint2 r = img[64 * DPAD + tid];
                    raw_r[0] = RawElem{r.x, r.y};
                }
            }
            return;
        }
        if constexpr (STAGE_COPY) {
            // one 8-byte word of the column's own [T][d] fp32 block (224 of them; thread tid takes word (tid & 127) + 96 * bit 7 of
            // tid < 224, so every address is inside the column whatever the launch's B)
            static_assert(EPT == 1, "stage copy: one element per thread");
            raw_v[0] = raw_r[0] = RawElem{0u, 0u};
            if (j < a.B) {
                const uint2 w = *reinterpret_cast<const uint2 *>(static_cast<const char *>(a.Y) + (size_t)j * (64 * 7 * 4) +
                                                                 (size_t)(((tid & 127) + ((tid >> 7) & 1) * 96) * 8));
                raw_v[0] = RawElem{w.x, w.y};
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int e = tid + k * NT;
            const int t = e / DPAD, c = e % DPAD;
            const bool ok = e < RING * DPAD && t < T && c < d && j < a.B;
            if constexpr (RAW_STAGE) {
                raw_v[k] = raw_r[k] = RawElem{0u, 0u}; // (+0.0 in either format)
                if (ok) {
                    raw_v[k] = load_raw(a.Y, ((size_t)j * T + t) * d + c);
                    raw_r[k] = load_raw(a.Y, (size_t)j * T * d + c);
                }
            } else {
                stage_v[k] = ok ? load_any(a.Y, ((size_t)j * T + t) * d + c, io64) : 0.0;
                stage_r[k] = ok ? load_any(a.Y, (size_t)j * T * d + c, io64) : 0.0;
            }
        }
    };
    // (RADIAL: the plain scale of s = |x~ - y~|^2 inv_h -- no log2 e, positive)
    const double nscale = RADIAL ? inv_h : -inv_h * 1.4426950408889634074; // exponent scale: exp(-d/h) = 2^(nscale*d)
    auto stage_store = [&](int buf) { // (buf: HALF only, the yf / yref buffer of the column; 0 otherwise)
        if constexpr (IMG) {
            const int t = tid / DPAD, c = tid % DPAD;
            const double v = __hiloint2double((int)raw_v[0].hi, (int)raw_v[0].lo); // (c == DPAD - 1: the norm)
            yd[t * YDS + c] = v;
            yd[(t + RING) * YDS + c] = v;
            const float vf = (c == DPAD - 1) ? 0.f : (float)v; // (the padded channel of yf holds 0, as stage_store leaves it)
            float *yfb = yf + buf * YFB;
            yfb[t * YFS + c] = vf;
            yfb[(t + RING) * YFS + c] = vf;
            if (t == 0) yref[buf * DPAD + c] = __hiloint2double((int)raw_r[0].hi, (int)raw_r[0].lo);
            return;
        }
        if constexpr (STAGE_COPY) {
            // the loaded bits, with the fp64 exponent forced to 2^-10 (one v_and_or_b32): every exponent of the static kernel then
            // stays tame, K comes out near 1 and the fp64 re-sweep, which a grid of garbage would trigger, never fires
            const int t = tid / DPAD, c = tid % DPAD;
            const double v = __hiloint2double((int)((raw_v[0].hi & 0x800FFFFFu) | 0x3F500000u), (int)raw_v[0].lo);
            yd[t * YDS + c] = v;
            yd[(t + RING) * YDS + c] = v;
            float *yfb = yf + buf * YFB;
            yfb[t * YFS + c] = __uint_as_float(raw_v[0].lo);
            yfb[(t + RING) * YFS + c] = __uint_as_float(raw_v[0].lo);
            if (t == 0) yref[buf * DPAD + c] = v;
            return;
        }
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int e = tid + k * NT;
            if (e < RING * DPAD) {
                const int t = e / DPAD, c = e % DPAD;
                if constexpr (RAW_STAGE) {
                    stage_v[k] = raw_value(raw_v[k]);
                    stage_r[k] = raw_value(raw_r[k]);
                }
                const double v = stage_v[k] - stage_r[k];
                if (!(LP && c == DPAD - 1)) { // (LP: that slot receives the norm below)
                    yd[t * YDS + c] = v;
                    yd[(t + RING) * YDS + c] = v;
                }
                if (GRAD) {
                    float *yfb = yf + (HALF ? buf * YFB : 0);
                    yfb[t * YFS + c] = (float)v;
                    yfb[(t + RING) * YFS + c] = (float)v;
                }
                if (t == 0) yref[(HALF ? buf * DPAD : 0) + c] = stage_r[k];
                double s = v * v * nscale; // -log2(e)/h * |y~_t|^2 via xor-reduction over the DPAD lanes of a row
#pragma unroll
                for (int off = 1; off < DPAD; off <<= 1) s += __shfl_xor(s, off, 64);
                if (c == 0) {
                    if constexpr (!HALF) {
                        ynd[t] = s;
                        ynd[t + RING] = s;
                    }
                    if (LP) { // the padded channel of the fp64 row carries the norm: phase 1 needs no separate read
                        yd[t * YDS + DPAD - 1] = s;
                        yd[(t + RING) * YDS + DPAD - 1] = s;
                    }
                }
            }
        }
    };

    // this workgroup's range of items, and the tile / column it starts in
    const long long it0 = a.nitems * blockIdx.x / gridDim.x, it1 = a.nitems * (blockIdx.x + 1) / gridDim.x;
    int remaining = (int)(it1 - it0);
    long long item = it0; // index of the (row tile, column) item in work
    const ItemSeek seek = item_seek<SYM>(a.tm, a.B, NWR, it0);
    int kq = seek.kq, cstart = seek.cstart;
    bool staged = false;
    while (remaining > 0) {
    const TileRange tr = tile_range<SYM>(a.tm, a.B, NWR, kq, cstart, remaining);
    const int cfirst = tr.cfirst, ncol = tr.ncol;
    const int jnext_tile = SYM ? a.tm.tile_of(kq + 1) * NWR : 0; // where the range goes on, on the next owned tile
    const bool more_tiles = remaining > ncol;
    const int i0 = tr.i0 + wave * RPW;                      // first (or only) row of this wavefront: scalar
    const int i = (RING == 32) ? i0 + (lane >> 5) : i0;     // the row this LANE works for
    const bool row_ok = i < a.A;
#pragma unroll
    for (int c = 0; c < DPAD; ++c) {
        gacc[c] = 0.0;
        xraw[c] = (row_ok && lrow < T && c < d) ? load_any(a.X, ((size_t)i * T + lrow) * d + c, io64) : 0.0;
    }
    if constexpr (RAW_STAGE) {
        // (the row has arrived HERE, once per tile: left pending, its first use in the column loop -- phase 0 -- waits for
        //  every load issued before it, the next column's included)
#pragma unroll
        for (int c = 0; c < DPAD; ++c) asm volatile("" : "+v"(xraw[c]));
    }
    j0 = cfirst + cstart;
    j1 = j0 + ncol;
    if (!staged) { // the range's first column: the only exposed load round trip
        staged = true;
        stage_load(j0);
        stage_store(pb);
        __syncthreads();
    }

    for (int j = j0; j < j1; ++j) {
        // (two rows per wavefront: the second one is the later row, so the first decides whether there is work at all;
        //  a half without a pair of its own -- row beyond A, or left of the diagonal -- computes along and is dropped)
        const bool pair_ok = i0 < a.A && (!SYM || j >= i0);
        const bool mine = row_ok && (!SYM || j >= i); // this lane's pair exists
        const bool last = j + 1 == j1;
        const bool more = !last || more_tiles;
        if (more) stage_load(last ? jnext_tile : j + 1); // in flight during the pair

        float Dsl[RING]; // increments / sqrt(12) (the scale the difference-form stencil wants), one slot per anti-diagonal
        const double *yrefp = yref + (HALF ? pb * DPAD : 0); // first point of y_j
        // the pair's sync block: barrier, block sum + stage_store, barrier.  One call site, at the end of the pair; HALF: the older
        // half's, the younger half passes it after phase 2 (waves without a pair included: the same barrier events).
        auto pair_sync = [&]() __attribute__((always_inline)) {
            SIG_STAMP(5)
#ifndef SIG_EXPERIMENT_NO_PAIR_BARRIER // timing experiment only (results are garbage without it)
            __syncthreads(); // every wave is done with y_j (and has parked its column-side result)
#endif
            SIG_STAMP(6)
            if constexpr (HALF != 0) {
                // At this sync the older half has parked the column sums of item j (its G regions) and the younger half those of
                // item j - 1 (ypark).  The item's block sum s = 0; s += w0; ... s += w7 is therefore split: waves 0..3 of item j
                // into ycarry now, ycarry + w4 + ... + w7 to the slab row at the next sync (or the tile's closing one, below) --
                // the same operands in the same order, the same bits.  Element e is read and written by thread e alone.
                const float inv_d = 1.0f / (float)d;
                const bool pend = j > j0; // item j - 1 of this tile waits in ycarry / ypark
                float *dstp = a.cslab + (size_t)(item - 1) * (T * d);
                for (int e = tid; e < T * d; e += NT) {
                    const int n = (int)(((float)e + 0.5f) * inv_d), c = e - n * d; // exact for e < 2^20
                    if (pend) {
                        float s = ycarry[e];
#pragma unroll
                        for (int w = 0; w < NW / 2; ++w) s += ypark[w * RING * DC + e]; // (d == DC, T == RING: [column][c] is e)
                        dstp[e] = s;
                    }
                    float s = 0.f;
#pragma unroll
                    for (int w = 0; w < NW / 2; ++w) s += Gs_all[w * GSW + n * DPAD + c];
                    ycarry[e] = s;
                }
            } else if (GRAD && SYM) {
                // thread e takes element e of the column's [T][d] block: the NW waves' sums are added in wave order and the
                // item's partial goes to its own row of the slab with one coalesced store per element (grad_reduce_kernel
                // adds the rows of a column in tile order).  Rounds 1-2 sent it with one atomic per element into a shared
                // accumulator: 29.6 M memory-side atomics per C4 launch, and a result that depended on their order.
                const float inv_d = 1.0f / (float)d;
                float *dst = a.cslab + (size_t)item * (T * d);
                for (int e = tid; e < T * d; e += NT) {
                    const int n = (int)(((float)e + 0.5f) * inv_d), c = e - n * d; // exact for e < 2^20
                    float s = 0.f;
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        s += Gs_all[w * GSW + n * DPAD + c];
                        if (RING == 32) s += Gs_all[w * GSW + (RING + n) * DPAD + c]; // the wavefront's second row
                    }
                    dst[e] = s;
                }
            }
            ++item;
            if (more) stage_store(HALF ? pb ^ 1 : 0); // (HALF: the next pair's buffer)
            SIG_STAMP(7)
#ifndef SIG_EXPERIMENT_NO_PAIR_BARRIER
            __syncthreads();
#endif
            SIG_STAMP(8)
        };
        auto younger_sync = [&]() __attribute__((always_inline)) { // (RAW_STAGE: the next column has arrived, as at the end of the pair)
            if constexpr (RAW_STAGE) {
#pragma unroll
                for (int k = 0; k < EPT; ++k)
                    asm volatile("" : "+v"(raw_v[k].lo), "+v"(raw_v[k].hi), "+v"(raw_r[k].lo), "+v"(raw_r[k].hi));
            }
            pair_sync();
        };

        SIG_STAMP(0)
        SIG_PRIO(3)
        if (pair_ok) {
            bal_top<BAL>(bal_first);
            // ---- phase 0: centre x_i on y_j[0] ----------------------------------------------------
            // x~ pre-scaled so that the exponent argument in base 2 is one fused dot product:
            //   log2(e) * (-|x~ - y~|^2 / h) = xn + ynd[q] + sum_c xs[c] * y~[q][c]
            double xs[DPAD];
            double xn = 0.0;
#pragma unroll
            for (int c = 0; c < DPAD; ++c) {
                const double xc = (lrow < T && c < d) ? xraw[c] - yrefp[c] : 0.0;
                xn = __builtin_fma(xc, xc, xn);
                xs[c] = xc * (-2.0 * nscale);
            }
            // everything downstream of the static kernel works with G / sqrt(12): the increments become
            // gamma = D / sqrt(12) (stencil below), and the gradient pass multiplies the scale back (m2h)
            if constexpr (RADIAL) xn = xn * nscale; // (the 1 / sqrt(12) is a factor of k, below)
            else
            xn = __builtin_fma(xn, nscale, -1.79248125036057809); // - log2(sqrt(12))

            // ---- phase 1: G rows (skewed: column (t - lane) & 63 on iteration t) -> D slots --------
            {
                double g0 = 0.0, g1 = 0.0, gprev = 0.0, rdprev = 0.0;
                const double *ybase = yd + (RING - lrow) * YDS; // row (t - lrow) & RM == ybase + t*YDS
                const double *nbase = ynd + (RING - lrow);
                // the y~ row of column t+1 is fetched while column t is computed (one s_waitcnt per
                // column instead of one per ds_read, and the LDS latency is off the exp chain)
                // (32 channels: the row in two blocks of 16, see below -- a half row ahead)
                constexpr int YPF = (DPAD > 16) ? DPAD / 2 : DPAD; // doubles of y~ fetched ahead
                double ynx[YPF], nnx;
#pragma unroll
                for (int c = 0; c < YPF; ++c) ynx[c] = ybase[c];
                nnx = LP ? 0.0 : nbase[0];
#pragma unroll
                for (int t = 0; t < RING + 2; ++t) {
                    double g;
                    if (t < RING) {
                        double e2;
                        if constexpr (DPAD > 16) {
                            // The 32-channel layout walks the dot product in two blocks of 16 channels: block 1 of column t is
                            // fetched while block 0 is multiplied, block 0 of column t + 1 while block 1 is, so that 16 + 16
                            // doubles of y~ are live beside the row's 32 of x~ -- the 16-channel kernel's figure -- instead of 32 + 32.
                            constexpr int HB = DPAD / 2;
                            double ycu[HB];
#pragma unroll
                            for (int c = 0; c < HB; ++c) ycu[c] = ynx[c];
                            e2 = LP ? xn : xn + nnx;
                            {
                                const double *yr = ybase + t * YDS + HB;
#pragma unroll
                                for (int c = 0; c < HB; ++c) ynx[c] = yr[c];
                                if (!LP && t < RING - 1) nnx = nbase[t + 1];
                            }
#pragma unroll
                            for (int c = 0; c < HB; ++c) e2 = __builtin_fma(xs[c], ycu[c], e2);
#pragma unroll
                            for (int c = 0; c < HB; ++c) ycu[c] = ynx[c];
                            if (t < RING - 1) {
                                const double *yr = ybase + (t + 1) * YDS;
#pragma unroll
                                for (int c = 0; c < HB; ++c) ynx[c] = yr[c];
                            }
                            if (LP) e2 += ycu[HB - 1]; // LP: the row's last slot is the norm
#pragma unroll
                            for (int c = HB; c < DC; ++c) e2 = __builtin_fma(xs[c], ycu[c - HB], e2);
                        } else {
                        double ycu[DPAD];
#pragma unroll
                        for (int c = 0; c < DPAD; ++c) ycu[c] = ynx[c];
                        e2 = LP ? xn + ycu[DPAD - 1] : xn + nnx; // LP: the row's last slot is the norm
                        if (t < RING - 1) {
                            const double *yr = ybase + (t + 1) * YDS;
#pragma unroll
                            for (int c = 0; c < DPAD; ++c) ynx[c] = yr[c];
                            if (!LP) nnx = nbase[t + 1];
                        }
#pragma unroll
                        for (int c = 0; c < DC; ++c) e2 = __builtin_fma(xs[c], ycu[c], e2);
                        }
                        if constexpr (RADIAL) {
                            // e2 is s (rounding leaves it a few ulp below 0 for coincident points; a NaN stays one).  k_imq =
                            // (1 + s)^-1/2 and k_rq = k_imq^2; -phi' = k_imq^3 / 2 and k_imq^4; both carry the 1 / sqrt(12)
                            const double ki = rsqrt_ge1(1.0 + (e2 < 0.0 ? 0.0 : e2)), ki2 = ki * ki;
                            const bool rq = a.kind == SIGSVGD_STATIC_RQ;
                            g = (rq ? ki2 : ki) * 0.28867513459481288225;
                            if (GRAD) Gs[t * GSS + lane] = (float)((rq ? ki2 : 0.5 * ki) * (ki2 * 0.28867513459481288225));
                        } else {
                        g = exp2_p7(e2);
                        if (GRAD) Gs[t * GSS + lane] = (float)g;
                        }
                        if (t == 0) g0 = g;
                        if (t == 1) g1 = g;
                    } else {
                        g = (t == RING) ? g0 : g1;
                    }
                    const double rd = g - gprev; // G[l, q] - G[l, q-1]
                    gprev = g;
                    if (t >= 2) {
                        // lane l+1 holds the same column difference one iteration later
                        const double nb = dpp_shl1_zero(rd);
                        Dsl[(t - 2) & RM] = (float)(nb - rdprev);
                        asm volatile("" : "+v"(Dsl[(t - 2) & RM])); // formed HERE: hipcc otherwise sinks the fp64 difference to the sweep
                    }
                    rdprev = rd;
                    __builtin_amdgcn_sched_barrier(0); // one column per scheduling region: bounds live ranges
                }
            }

            SIG_STAMP(1)
            SIG_PRIO(2)
            bal_switch<BAL, 1>(bal_first);
            float kf_keep = 0.f;                   // K[P][P] of this lane's pair and the cancellation verdicts of phase 2, for the
            bool x0_keep = false, x1_keep = false; // conditioning check after the reverse sweep (4-channel gradient kernels)
            // ---- phase 2: forward sweep, anti-diagonal sigma = 0 .. 2P-2, in fp32 DIFFERENCE FORM ----------
            // With gamma = g / sqrt(12) the second-order stencil reads
            //     K11 - K01 = (K10 - K00) + F,   F = gamma * (sqrt(3) * t + gamma * (t + K00)),  t = K10 + K01,
            // so the lane carries V = K[l+1][q] - K[l][q] along its row (V += F: a lane-local recurrence whose
            // rounding errors are relative to |V| << |K|) and forms K11 = K01 + V with ONE full-magnitude add
            // that never feeds back into V.  In fp32 this is within 2e-7 of the fp64 recurrence for K and for
            // the gradient (scripts/dev/precision_vform.py: 1.5e-7 / 1.9e-7 at the C4 shape, where the plain
            // fp32 stencil loses 4e-6..2e-5), at 10 fp32-rate instructions per step instead of 12.5, seven of
            // them fp64-rate (measured cost per SIMD at two waves: fp64 2.4 ns, fp32 1.4 ns, DPP move 1.9 ns).
            {
                // `up` persists (lane 0 keeps the boundary K[0][.] = 1) in TWO registers used on alternate steps:
                // the diagonal neighbour K[l][q] of a step is the upper neighbour of the step before, whether or
                // not this lane was active then (a lane's value is 1.0 until its row starts and frozen after it
                // ends), so it needs no copy.
                float cur = 1.f, upA = 1.f, upB = 1.f, V = 0.f, km = 1.f, sd = 0.f;
                const int smax = 2 * P - 2;
                if (GRAD) {
#pragma unroll
                    for (int k = 0; k < RING; ++k) Ksl[k] = 0.f;
                }
                if constexpr (PFIX != 0) { // windows from immediates: a round of 64 steps, then the 61 that are left
                    static_assert(GRAD && RING == 64 && PFIX == 63, "fixed windows: gradient kernels of the 64-slot ring at T = 64");
                    float r3 = 1.7320508075688772f;
                    asm volatile("" : "+s"(r3));
                    sweep_fwd_fixed_round<PFIX, 0, 64>(cur, upA, upB, V, Dsl, Ksl, r3);
                    asm volatile("" : "+s"(r3));
                    sweep_fwd_fixed_round<PFIX, 64, 2 * PFIX - 1>(cur, upA, upB, V, Dsl, Ksl, r3);
                } else
                for (int rnd = 0; rnd < (RING == 64 ? 2 : 1); ++rnd) { // (RING = 32: 2P-2 <= 60, one round of 64 steps)
                    if (rnd * 64 > smax) break;
                    float r3 = 1.7320508075688772f;
                    asm volatile("" : "+s"(r3)); // opaque per round: nothing of the step is round-invariant
                    const unsigned long long *mk = (RING == 64 ? SWEEP_MASK.m[P] : SWEEP_MASK32.m[P]) + rnd * 64; // EXEC windows
#pragma unroll
                    for (int k0 = 0; k0 < 64; k0 += 8) // Ksl[k] <- K[l, q]
                        sweep_fwd8<GRAD ? 0 : (DPAD == 4 ? 2 : 1)>(cur, upA, upB, V, &Dsl[k0 & RM], &Ksl[k0 & RM], mk + k0, r3, km, sd);
                }
                // largest |K| on this lane's row against the pair's result: cancellation -> fp64 (resweep_fwd_fp64 above)
                if (GRAD) {
                    km = fabsf(cur); // K[l+1][P]; the slots: K[l][q], q < P
#pragma unroll
                    for (int k = 0; k < RING; k += 2) km = max3_abs(km, Ksl[k], Ksl[k + 1]);
                }
                float kf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur), P - 1));
                if (RING == 32) {
                    const float kf1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur), 32 + P - 1));
                    kf = (lane >> 5) ? kf1 : kf;
                }
                // Paths in one to four channels (the 4-channel instantiations; the launcher passes a flag array for d <= 4 only --
                // d = 4 since a soak case with T = 33, d = 4 showed an entry of |K| ~ 0.005 off by 1.7e-5 RELATIVE after the fp64
                // re-sweep on fp32 increments: tiny entries need the exact pass whatever their conditioning):
                // the fp64 re-sweep below runs on fp32 increments, which is not enough where the discrete solution is
                // ill-conditioned, so such pairs are flagged for the exact fp64 pass by the repair rule of sweep_scaffold.h
                // (gradient launches: the condition number, after the reverse sweep -- below, "conditioning").
                // Compiled into the 4-channel kernels only: in the 8-channel ones the ballot and the byte
                // store cost the headline launch 1.7 % (same-box A/B), and no pair of >= 4 channels needs it (worst entry 9e-7 in
                // the roughest regimes of the study).
                bool x0 = false, x1 = false;
                if constexpr (DPAD == 4) {
                    if (a.kflag) {
                        const float kden = repair_den(kf);
                        // (the grid maximum above 4 max(|K|, 0.1), 2 in one channel, in this kernel's three and four channels too: its
                        //  fp32 sweeps resolve ~1e-6 of the largest value on the grid, the boundary value 1 included)
                        bool fl = km > repair_ratio(d, 4.f) * kden;
                        if constexpr (!GRAD) { // sum over the pair's lanes of sum_q |K[l][q] gamma[l][q]|, times sqrt(12): in units of D
                            const float wsum = wave_sum_dpp<RING == 64>(sd);
                            float sds = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wsum), 63));
                            if (RING == 32) {
                                const float s0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wsum), 31));
                                sds = (lane >> 5) ? sds : s0;
                            }
                            fl = fl || repair_fwd_bound(sds, km, kden);
                        }
                        const unsigned long long xbal = __builtin_amdgcn_ballot_w64(mine && kf == kf && fl);
                        x0 = (RING == 64) ? xbal != 0 : (unsigned)xbal != 0u;
                        x1 = (xbal >> 32) != 0;
                    }
                }
                if (lrow == P - 1 && mine) { // this lane's last value is K[P, P]
                    store_any(a.K, (size_t)i * a.B + j, (double)cur, io64);
                    if (SYM && j != i) store_any(a.K, (size_t)j * a.B + i, (double)cur, io64);
                    if constexpr (DPAD == 4 && !GRAD) { // (two rows per wavefront: each half of the ballot is one pair)
                        if (a.kflag) a.kflag[(size_t)i * a.B + j] = (RING == 32 && (lane >> 5)) ? x1 : x0;
                    }
                }
                kf_keep = kf;
                x0_keep = x0;
                x1_keep = x1;
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(mine && km > kResweepRatio * repair_den(kf)) != 0, 0)) {
                    const double k64 = resweep_fwd_fp64<RING>(Dsl, P, lrow);
                    if (lrow == P - 1 && mine) { // (same lane, same addresses as the first store: the later one stands)
                        store_any(a.K, (size_t)i * a.B + j, k64, io64);
                        if (SYM && j != i) store_any(a.K, (size_t)j * a.B + i, k64, io64);
                    }
                }
            }

            SIG_STAMP(2)
            SIG_PRIO(1)
            bal_switch<BAL, 2>(bal_first);
            if constexpr (HALF != 0) {
                // the younger half's sync site: it keeps its increments and K_fwd slots across it (the sync code touches neither).
                // Then every wave holds `s_setprio 1` through its phases 3-4: without it the younger half loses the arbitration
                // there and the older half waits a third of its time at the sync (profiles/half_offset_bound.txt).
                if (half_younger) younger_sync();
                __builtin_amdgcn_s_setprio(1);
            }
            if (GRAD) {
                // (pair_weights of sweep_scaffold.h is not used here: this kernel's weights are per LANE -- `mine`, `wcol`, two rows
                //  per wavefront -- and the diagonal rule lives in `wcol`; the same holds for rseg_slot and the slot `rslot` below)
                // weights of this lane's pair: row side w_ij, column side w_ji (per lane with two rows per wavefront,
                // uniform otherwise; fetched here so that the loads are long back when the gradient pass needs them)
                float w_ij = 1.f, w_ji = 1.f; // (per lane with two rows per wavefront; uniform otherwise)
                if (!mine) {
                    w_ij = 0.f; w_ji = 0.f;
                } else if (a.go) {
                    w_ij = (float)load_any(a.go, (size_t)i * a.B + j, io64);
                    if (SYM || a.symw) w_ji = (float)load_any(a.go, (size_t)j * a.B + i, io64);
                    if (a.symw) { w_ij += w_ji; w_ji = w_ij; }
                } else if (a.symw) {
                    w_ij = 2.f; w_ji = 2.f;
                }
                const float wcol = (mine && j != i) ? w_ji : 0.f; // the diagonal pair has no column side
                // ---- phase 3: reverse sweep (U recurrence; S replaces K_fwd slot by slot) -----------------
                float cur = 1.f, downA = 1.f, downB = 1.f, V = 0.f; // `down` persists (lane 63 keeps U[P][.] = 1), alternating as above
                float Sb = 0.f, eprev = 0.f;
                f32x2 acc[DPAD / 2]; // packed pairs: the contraction runs on v_pk_fma_f32
#pragma unroll
                for (int c = 0; c < DPAD / 2; ++c) acc[c] = f32x2{0.f, 0.f};
                const int smax = 2 * P - 2;

                // x~ of this lane's row as packed fp32 pairs (row-side closing formula; column-side products)
                f32x2 xc2[DPAD / 2];
#pragma unroll
                for (int c = 0; c < DPAD / 2; ++c) {
                    const bool ok0 = lrow < T && 2 * c < d, ok1 = lrow < T && 2 * c + 1 < d;
                    xc2[c] = f32x2{ok0 ? (float)(xraw[2 * c] - yrefp[2 * c]) : 0.f,
                                   ok1 ? (float)(xraw[2 * c + 1] - yrefp[2 * c + 1]) : 0.f};
                }
                // column-side (SYM): accumulators that TRAVEL one lane down per step.  On step sigma lane m
                // holds R*G[m, n] with n = sigma+2-m; on the next step lane m-1 holds the same column n, so
                // sum_m R*G[m,n] * x~_m rides a wave rotation (v_add_f32 with a wave_rol:1 DPP source) and
                // never needs a transposed pass: finished columns wrap past lane 0 through lanes that
                // are already idle, and after the last step column n sits in lane (64 - n) & 63.
                float tacc[DPAD];
#pragma unroll
                for (int c = 0; c < DPAD; ++c) tacc[c] = 0.f;

                int yfrow = RING - lrow + (HALF ? pb * 2 * RING : 0); // row (sigma + 2 - lrow) & RM == yfrow + k2 (HALF: of this pair's buffer)
                int gsoff = (GRAD ? wave * GSW : 0) + lane; // this wave's [slot][lane] image
                // one iteration of the phase-4 pass (below); `gcu`, `ycu`: G[l][n] and the y~_n row, fetched one
                // iteration ahead so that the LDS latency is off the chain and one s_waitcnt serves the iteration
                auto grad_part = [&](float Snew, bool accumulate, float gcu, const f32x2 *ycu) {
                    // R[l][q+2] = (S[l][q+2] - S[l][q+1]) - (S[l-1][q+2] - S[l-1][q+1]): the column difference
                    // e = S[l][q+1] - S[l][q] of this iteration serves this lane on the NEXT iteration and, through the wave
                    // shift, lane l+1 on this one (its column is one behind) -- each difference is formed once (rounds 1-2
                    // shifted S and formed the neighbour's difference a second time: one instruction more per iteration,
                    // 5.38 -> 5.25 ms per C4 launch in a same-box A/B; the result is the same bit for bit)
                    const float e = Sb - Snew;
                    const float up = shfl_up_zero(e); // lane l-1: S[l-1][q+2] - S[l-1][q+1]; lane 0: no row above
                    const float R = eprev - up;
                    eprev = e;
                    Sb = Snew;
                    if (!accumulate) return; // warm-up iteration: only the two-deep history is filled
                    const float rg = R * gcu;
                    const f32x2 rg2 = {rg, rg};
                    // Both contractions take the DIFFERENCE x~_m - y~_n (one packed subtraction per channel pair, shared
                    // by the two sides).  Rounds 1-2 accumulated sum R G y~_n and sum R G separately and closed with
                    // x~_m * sum - sum: when consecutive points lie more than a bandwidth apart, G is concentrated where
                    // x~_m - y~_n is smallest and that closing cancels catastrophically (gradient error 1e-3 relative to
                    // its maximum at |step|^2 / h ~ 30, profiles/r03_precision_sweep.md; 3e-6 in this form).
                    f32x2 df[DPAD / 2];
#pragma unroll
                    for (int c = 0; c < DPAD / 2; ++c) df[c] = xc2[c] - ycu[c];
#pragma unroll
                    for (int c = 0; c < DPAD / 2; ++c) acc[c] = __builtin_elementwise_fma(rg2, df[c], acc[c]);
                    // pin the running sums here: the contraction must stay inside its step
#pragma unroll
                    for (int c = 0; c < DPAD / 2; ++c) asm volatile("" : "+v"(acc[c]));
                    if (SYM) {
                        // (two rows per wavefront: a travelling sum collects BOTH rows on its way, so each contribution
                        //  carries its own pair's weight; with one row the weight is applied once, when the sums are parked)
                        const float rgc = (RING == 32) ? rg * wcol : rg;
                        const f32x2 rgc2 = {rgc, rgc};
#pragma unroll
                        for (int c = 0; c < DPAD / 2; ++c) {
                            const f32x2 pr = rgc2 * df[c];
                            tacc[2 * c] = add_rol1(tacc[2 * c], pr[0]);
                            if (2 * c + 1 < DC) tacc[2 * c + 1] = add_rol1(tacc[2 * c + 1], pr[1]);
                        }
#pragma unroll
                        for (int c = 0; c < DPAD; ++c) asm volatile("" : "+v"(tacc[c]));
                    }
                };

                if constexpr (PFIX != 0) {
                    asm volatile("" : "+v"(yfrow), "+v"(gsoff)); // (as in the table form below, once per round)
                    float r3 = 1.7320508075688772f;
                    asm volatile("" : "+s"(r3));
                    sweep_rev_fixed_round<PFIX, 64, 2 * PFIX - 1>(cur, downA, downB, V, Dsl, Ksl, r3);
                    bal_switch<BAL, 3>(bal_first);
                    asm volatile("" : "+v"(yfrow), "+v"(gsoff));
                    asm volatile("" : "+s"(r3));
                    sweep_rev_fixed_round<PFIX, 0, 64>(cur, downA, downB, V, Dsl, Ksl, r3);
                } else
                for (int rnd = (RING == 64 ? 1 : 0); rnd >= 0; --rnd) {
                    if (rnd * 64 > smax) continue;
                    // (keeps the phase-4 LDS addresses out of this loop's invariants: without the pin hipcc
                    //  rearranges the pass that follows and the C4 launch goes from 6.9 to 10.9 ms)
                    asm volatile("" : "+v"(yfrow), "+v"(gsoff));
                    float r3 = 1.7320508075688772f;
                    asm volatile("" : "+s"(r3));
                    const unsigned long long *mk = (RING == 64 ? SWEEP_MASK.m[P] : SWEEP_MASK32.m[P]) + rnd * 64;
                    // same difference form, V = U[l][q] - U[l+1][q] carried towards smaller q; `down` alternates between
                    // two registers like `up` (the diagonal neighbour U[l+1][q+1] is the lower neighbour one step ago)
#pragma unroll
                    for (int k0 = 56; k0 >= 0; k0 -= 8) sweep_rev8(cur, downA, downB, V, &Dsl[k0 & RM], &Ksl[k0 & RM], mk + k0, r3);
                }

                // ---- conditioning (4-channel kernels with a flag array, i.e. d <= 4): c1 = sum |S * D| / max(|K|, 0.1) ------
                // The slots hold S = K_fwd * U (0 where there is no cell) and gamma = D / sqrt(12): 64 multiply-adds per lane, a
                // wave sum, one byte per pair (see phase 2 for the rule and its measurement).  C3 (d = 3): +1.2 % instructions.
                if constexpr (DPAD == 4) {
                    if (a.kflag) {
                        float cs = 0.f;
#pragma unroll
                        for (int k = 0; k < RING; ++k) cs = __builtin_fmaf(fabsf(Ksl[k]), fabsf(Dsl[k]), cs);
                        const float wsum = wave_sum_dpp<RING == 64>(cs);
                        float c1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wsum), 63));
                        if (RING == 32) {
                            const float c10 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wsum), 31));
                            c1 = (lane >> 5) ? c1 : c10;
                        }
                        const bool ill = kf_keep == kf_keep && repair_ill(c1, repair_den(kf_keep));
                        if (lrow == P - 1 && mine)
                            a.kflag[(size_t)i * a.B + j] = (((RING == 32 && (lane >> 5)) ? x1_keep : x0_keep) || ill) ? 1 : 0;
                    }
                }
                SIG_STAMP(3)
                SIG_PRIO(0)
                // ---- phase 4: 4-corner scatter R and both contractions, one column per lane and iteration ----
                // The reverse sweep has only half of its lanes inside the grid at any step, so nothing but the
                // recurrence is left in it.  Here every lane is busy on every iteration: lane l takes the slots in
                // descending order, i.e. column q = (63 - it - l) & 63 with wrap-around; slots without a grid cell
                // (column >= P, row >= P) hold S = 0 (see Ksl), which is also exactly what the scatter needs at the
                // wrap (S[.][-1] = S[.][63] = 0).  Two warm-up iterations fill the history, the next 64 visit
                // every column n = q + 2 once; the travelling sums rotate as before and end in lane (64 - n) & 63.
                float gnx = 0.f, Svn = Ksl[RM];
                f32x2 ynx[DPAD / 2];
#pragma unroll
                for (int c = 0; c < DPAD / 2; ++c) ynx[c] = f32x2{0.f, 0.f};
                if constexpr (DPAD > 16) {
                // The 32-channel layout: the same loop, stated a second time for its pragma alone.  66 iterations of 32 channels pass
                // the size up to which `#pragma unroll` unrolls completely; left rolled, the slot index is a run-time value and the
                // K slots live in scratch memory.  (Sharing the body through a lambda, or giving the loop below this pragma, changes
                // the code of existing instantiations -- scripts/compare_device_code.py --, which stay as they are.)
#pragma clang loop unroll(full)
                for (int it = 0; it < RING + 2; ++it) {
                    const float Sv = Svn, gcu = gnx;
                    f32x2 ycu[DPAD / 2];
#pragma unroll
                    for (int c = 0; c < DPAD / 2; ++c) ycu[c] = ynx[c];
                    if (it + 1 < RING + 2) { // next iteration's operands: slot (RING-2 - it) & RM, column slot (RING - it) & RM
                        Svn = Ksl[(RING - 2 - it) & RM];
                        if (it + 1 >= 2) {
                            const int k2n = (RING - it) & RM;
                            gnx = Gs_all[gsoff + k2n * GSS];
                            const f32x2 *yr = reinterpret_cast<const f32x2 *>(yf + (yfrow + k2n) * YFS);
#pragma unroll
                            for (int c = 0; c < DPAD / 2; ++c) ynx[c] = yr[c];
                        }
                    }
                    grad_part(Sv, it >= 2, gcu, ycu);
                    __builtin_amdgcn_sched_barrier(0);
                }
                } else {
#pragma unroll
                for (int it = 0; it < RING + 2; ++it) {
                    const float Sv = Svn, gcu = gnx;
                    f32x2 ycu[DPAD / 2];
#pragma unroll
                    for (int c = 0; c < DPAD / 2; ++c) ycu[c] = ynx[c];
                    if (it + 1 < RING + 2) { // next iteration's operands: slot (RING-2 - it) & RM, column slot (RING - it) & RM
                        Svn = Ksl[(RING - 2 - it) & RM];
                        if (it + 1 >= 2) {
                            const int k2n = (RING - it) & RM;
                            gnx = Gs_all[gsoff + k2n * GSS];
                            const f32x2 *yr = reinterpret_cast<const f32x2 *>(yf + (yfrow + k2n) * YFS);
#pragma unroll
                            for (int c = 0; c < DPAD / 2; ++c) ynx[c] = yr[c];
                        }
                    }
                    grad_part(Sv, it >= 2, gcu, ycu);
                    __builtin_amdgcn_sched_barrier(0);
                }
                }

                SIG_STAMP(4)
                // row-side gradient of this pair: -(2/h) * sum_n R G (x~_m - y~_n); column side: the same sum over m, negated
#pragma unroll
                for (int c = 0; c < DPAD; ++c) {
                    gacc[c] += (double)(w_ij * m2h * acc[c / 2][c % 2]);
                }

                if (SYM) {
                    // park the column-side result in this wave's own G region ([half][column][c]) for the block sum; the
                    // diagonal pair has no column side, a half without a pair contributes nothing
                    const int ncol = (RING - lrow) & RM; // the column whose finished sums this lane ended up with
                    const float wpark = (ncol <= P) ? ((RING == 32) ? -m2h : -(wcol * m2h)) : 0.f;
                    if (HALF != 0 && half_younger) { // (its G image belongs to its next phase 1 before the sums are added up)
                        float *pk = ypark + ((wave - NW / 2) * RING + ncol) * DC;
#pragma unroll
                        for (int c = 0; c < DC; ++c) pk[c] = wpark * tacc[c];
                    } else {
                    float *pk = Gs + ((RING == 32 ? (lane >> 5) * RING : 0) + ncol) * DPAD;
#pragma unroll
                    for (int c = 0; c < DPAD; ++c) pk[c] = wpark * tacc[c];
                    }
                }
            }
        } else if (GRAD && SYM) {
            if (HALF != 0 && half_younger) {
                younger_sync();
#pragma unroll
                for (int c = 0; c < DC; ++c) ypark[((wave - NW / 2) * RING + lane) * DC + c] = 0.f;
            } else {
#pragma unroll
            for (int c = 0; c < DPAD; ++c) Gs[lane * DPAD + c] = 0.f; // idle wave contributes nothing
            }
        }
        // (RAW_STAGE: the next column arrived long ago; saying so HERE, on every path, keeps that wait out of the window
        //  after the barrier: the compiler cannot see that the loads at the loop top and the store that consumes them run
        //  under the same condition)
        if constexpr (RAW_STAGE) {
#pragma unroll
            for (int k = 0; k < EPT; ++k)
                asm volatile("" : "+v"(raw_v[k].lo), "+v"(raw_v[k].hi), "+v"(raw_r[k].lo), "+v"(raw_r[k].hi));
        }
        bal_end<BAL>(bal_first); // (a wave without a pair never raised it: then this changes nothing)
        if constexpr (HALF != 0) __builtin_amdgcn_s_setprio(0);
        if (!half_younger) pair_sync(); // (HALF: the younger half has passed it after phase 2)
        if constexpr (HALF != 0) pb ^= 1; // (after the sync: it stages the next column into the other buffer)
    }
    if constexpr (HALF != 0) {
        // the tile's closing sync: the younger half has just finished phases 3-4 of the last item (the older half waits here
        // meanwhile: half an interval per workgroup and tile; the first interval of a tile mirrors it); the item's block sum
        // leaves as above.  One barrier: the next writes of ycarry / ypark come after the next sync's first one.
        __syncthreads();
        float *dstp = a.cslab + (size_t)(item - 1) * (T * d);
        for (int e = tid; e < T * d; e += NT) {
            float s = ycarry[e];
#pragma unroll
            for (int w = 0; w < NW / 2; ++w) s += ypark[w * RING * DC + e];
            dstp[e] = s;
        }
    }

    if (GRAD && row_ok && lrow < T) { // this (workgroup, row tile) segment's own slot: segments are numbered kq + workgroup
        const int rslot = wave * RPW + (RING == 32 ? (lane >> 5) : 0);
        double *dst = a.rseg + (((size_t)(kq + (int)blockIdx.x)) * NWR + rslot) * (size_t)(T * d) + lrow * d;
#pragma unroll
        for (int c = 0; c < DPAD; ++c)
            if (c < d) dst[c] = gacc[c];
    }
    remaining -= ncol;
    ++kq;
    cstart = 0;
    } // row tiles of the range
#ifdef SIGSVGD_PHASE_STAMPS
    SIG_STAMP(0)
    if (lane == 0 && a.stamps) // the older half of the workgroup (waves 0 .. NW/2 - 1) and the younger one apart
        for (int k = 0; k < SIG_FAST_PHASES; ++k) atomicAdd(&a.stamps[(wave >= NW / 2 ? SIG_FAST_PHASES : 0) + k], ph_[k]);
#endif
}

// ---- launching an instantiation (both translation units) ------------------------------------------------------------------
// The symmetric 4- and 8-channel gradient kernels with fixed windows have a twin with the wave-balance schedule (BAL, see bal_top);
// launches that reach them run the twin.  SIGSVGD_WAVE_BALANCE=off, read per launch next to SIGSVGD_SWEEP_WINDOWS (gram_fast.hip's
// wave_balance), keeps them on the kernel without it: the tests compare the two on one build, and so do the A/B runs.
// FAST_BAL: the schedule the twin is built with: 6, the older half first, the younger half from the end of phase 2 on -- the
// fastest of the six measured at C4 (1, 2, 3 and their mirror images: profiles/wave_balance_ab.txt).
// -DSIG_EXPERIMENT_BALANCE=n builds another one to measure; 0: no twin.
#ifndef SIG_EXPERIMENT_BALANCE
#define SIG_EXPERIMENT_BALANCE 6
#endif
constexpr int FAST_BAL = SIG_EXPERIMENT_BALANCE;
// Which kernels have the twin: the symmetric ones on 8-wave workgroups, 8 channels (C4: -1.6 ... -2.2 %) and 4 channels (C3: -4 ... -5 %).  The
// ordered 8-channel kernel was built with it in place of SIG_PRIO and lost 0.6-1.3 %: it keeps SIG_PRIO.
template <int DPAD, bool SYM>
constexpr bool fast_has_balance() { return FAST_BAL != 0 && SYM && DPAD <= 8; }

// The half-offset twin (the kernel's HALF): the symmetric 7-of-8-channel kernel, the headline's.  d = 8 has no LDS left for it (the
// norm array cannot go), the 4-channel kernels keep the wave-balance twin.  SIGSVGD_HALF_OFFSET=off, read per launch next to
// SIGSVGD_WAVE_BALANCE (gram_fast.hip's half_offset), keeps a launch on the wave-balance twin.
template <int DPAD, bool SYM, bool LP>
constexpr bool fast_has_half() { return SYM && LP && DPAD == 8; }

// gram_fast_radial.hip: dispatch_variant<1> below (RADIAL = 1: IMQ and rational quadratic, a.kind), called from gram_fast.hip's `run`
int fast_radial_dispatch(const GramProblem &p, FastArgs &a, const WsPlan &w, bool grad, bool sym, int &tile_rows);
// gram_fast_wide.hip: the 32-channel layout (RBF, 17 <= d <= 32), called from gram_fast.hip's `run`
int fast_wide_dispatch(const GramProblem &p, FastArgs &a, const WsPlan &w, bool grad, bool sym, int &tile_rows);

namespace {
// a gradient instantiation, or (64-slot ring, `fix`: the plan's fixed_windows) its fixed-window twin for 64-point paths, or
// (`bal`: the plan's wave_balance) that twin's twin with the wave-balance schedule, or (`half`: the plan's half_offset) its twin with
// the halves of the workgroup half a pair apart, or (`img`: the plan's column_images) that twin's twin which stages the columns from
// their images; RADIAL has none of them
template <int DPAD, int NW, bool SYM, bool LP, int RING, int RADIAL>
void launch_grad(bool fix, bool bal, bool half, bool img, dim3 grid, dim3 block, hipStream_t stream, const FastArgsOf<RADIAL> &a)
{
    if constexpr (RADIAL == 0 && RING == 64 && DPAD <= 16 && NW == (DPAD <= 8 ? 8 : 4)) { // (the workgroup shapes dispatch_variant gives gradient launches; the 32-channel kernels: general windows only)
        if constexpr (fast_has_half<DPAD, SYM, LP>()) {
            if (fix && half && img) { // (a.Y: the column images, see gram_fast.hip's `run`)
                hipLaunchKernelGGL((gram_fast_kernel<DPAD, NW, true, SYM, LP, RING, 63, 0, 0, 2>), grid, block, 0, stream, a);
                return;
            }
            if (fix && half) {
                hipLaunchKernelGGL((gram_fast_kernel<DPAD, NW, true, SYM, LP, RING, 63, 0, 0, 1>), grid, block, 0, stream, a);
                return;
            }
        }
        if constexpr (fast_has_balance<DPAD, SYM>()) {
            if (fix && bal) {
                hipLaunchKernelGGL((gram_fast_kernel<DPAD, NW, true, SYM, LP, RING, 63, FAST_BAL>), grid, block, 0, stream, a);
                return;
            }
        }
        if (fix) {
            hipLaunchKernelGGL((gram_fast_kernel<DPAD, NW, true, SYM, LP, RING, 63>), grid, block, 0, stream, a);
            return;
        }
    }
    hipLaunchKernelGGL((gram_fast_kernel<DPAD, NW, true, SYM, LP, RING, 0, 0, RADIAL>), grid, block, 0, stream, a);
}

template <int RADIAL, int DPAD, int NW, int RING = 64>
int launch_variant(const GramProblem &p, FastArgs &a, const WsPlan &w, bool grad, bool sym, int &tile_rows)
{
    // items of this launch: (owned row tile, column); symmetric launches only the columns from the tile's first row on
    constexpr int NWR = NW * (RING == 32 ? 2 : 1); // rows per tile: the 32-slot ring solves two rows per wavefront
    tile_rows = NWR;
    const TileMap tm = make_tilemap((p.A + NWR - 1) / NWR, a.tm.off, a.tm.stride, a.tm.fold != 0);
    if (tm.owned <= 0) return SIGSVGD_OK;
    const long long total = tm.start(tm.owned, p.B, NWR, sym ? 1 : 0);
    if (total <= 0) return SIGSVGD_OK;
    const int ncu = device_cu_count();
    a.tm = tm;
    a.nitems = total;
#ifdef SIGSVGD_PHASE_STAMPS
    a.stamps = phase_stamps_begin(p.stream);
#endif
    const long long resident = (long long)ncu * (grad ? ((RING == 32 && NW == 4 && DPAD <= 8) ? 3 : 1) : (NW == 4 ? ((DPAD <= 8) ? 3 : (DPAD <= 16) ? 2 : 1) : 1)); // workgroups the chip holds at once (LDS / VGPR bound)
    dim3 grid((unsigned)(total < resident ? total : resident), 1);
    dim3 block(NW * 64);
    if (grad) { // the reduction kernel re-derives the segments from this geometry: it must be the one the workspace was cut for
        const GradGeom &g = w.g;
        if (g.NW != NWR || g.grid != (int)grid.x || g.nitems != total) {
            set_error("fast: launch geometry mismatch (rows per tile %d/%d grid %d/%u items %lld/%lld)", g.NW, NWR, g.grid, grid.x,
                      g.nitems, total);
            return SIGSVGD_E_BADARG;
        }
    }
    constexpr bool HAS_LP = DPAD <= 8 || DPAD == 32; // the d == DPAD - 1 instantiations exist for the 4-, 8- and 32-channel layouts
    const bool lp = HAS_LP && grad && p.d == DPAD - 1;
    FastArgsOf<RADIAL> ka{}; // the kernel's arguments: `a`, and for the radial kinds the kind
    static_cast<FastArgs &>(ka) = a;
    if constexpr (RADIAL != 0) ka.kind = p.kind;
    const bool fix = grad && w.fixed_windows && p.T == 64; // (the kernel's PFIX must be the launch's T - 1)
    const bool bal = fix && w.wave_balance;
    const bool half = fix && w.half_offset;
    const bool img = half && w.column_images; // (gram_fast.hip's `run` has formed the images and pointed a.Y at them)
    if (!grad && sym)
        hipLaunchKernelGGL((gram_fast_kernel<DPAD, NW, false, true, false, RING, 0, 0, RADIAL>), grid, block, 0, p.stream, ka);
    else if (!grad)
        hipLaunchKernelGGL((gram_fast_kernel<DPAD, NW, false, false, false, RING, 0, 0, RADIAL>), grid, block, 0, p.stream, ka);
    else if (sym && lp)
        launch_grad<DPAD, NW, true, HAS_LP, RING, RADIAL>(fix, bal, half, img, grid, block, p.stream, ka);
    else if (sym)
        launch_grad<DPAD, NW, true, false, RING, RADIAL>(fix, bal, half, img, grid, block, p.stream, ka);
    else if (lp)
        launch_grad<DPAD, NW, false, HAS_LP, RING, RADIAL>(fix, bal, half, img, grid, block, p.stream, ka);
    else
        launch_grad<DPAD, NW, false, false, RING, RADIAL>(fix, bal, half, img, grid, block, p.stream, ka);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch gram_fast_kernel");
#ifdef SIGSVGD_PHASE_STAMPS
    // ("loop top" + "block sum + stage store" + "second barrier" = the "staging/other" of the profiles before the split)
    static const char *const nm[] = {"loop top", "phase 0+1 static kernel", "phase 2 forward sweep", "phase 3 reverse sweep",
                                      "phase 4 gradient pass", "pair epilogue", "barrier after the pair",
                                      "block sum + stage store", "second barrier"};
    static_assert(sizeof(nm) / sizeof(nm[0]) == SIG_FAST_PHASES, "one name per stamp slot");
    phase_stamps_report_halves(p.stream, a.stamps, nm, "[phase stamps] A=%d T=%d d=%d grad=%d sym=%d: ", p.A, p.T, p.d, (int)grad, (int)sym);
#endif
    return SIGSVGD_OK;
}

template <int RADIAL>
int dispatch_variant(const GramProblem &p, FastArgs &a, const WsPlan &w, bool grad, bool sym, int &tile_rows)
{
    if (!grad && p.d <= 4) // forward only: no G image, <=168 VGPRs -> 4-wave workgroups pack 3 waves per SIMD
        return p.T <= 32 ? launch_variant<RADIAL, 4, 4, 32>(p, a, w, false, sym, tile_rows) : launch_variant<RADIAL, 4, 4>(p, a, w, false, sym, tile_rows);
    if (!grad && p.d <= 8)
        return p.T <= 32 ? launch_variant<RADIAL, 8, 4, 32>(p, a, w, false, sym, tile_rows) : launch_variant<RADIAL, 8, 4>(p, a, w, false, sym, tile_rows);
    if (p.d <= 4) // (paths of <= 32 points: the 32-slot ring on 4-wave workgroups, three per CU = 3 waves per SIMD)
        return p.T <= 32 ? launch_variant<RADIAL, 4, 4, 32>(p, a, w, grad, sym, tile_rows) : launch_variant<RADIAL, 4, 8>(p, a, w, grad, sym, tile_rows);
    if (p.d <= 8)
        return p.T <= 32 ? launch_variant<RADIAL, 8, 4, 32>(p, a, w, grad, sym, tile_rows) : launch_variant<RADIAL, 8, 8>(p, a, w, grad, sym, tile_rows);
    return launch_variant<RADIAL, 16, 4>(p, a, w, grad, sym, tile_rows); // 1 wave per SIMD: 512-VGPR budget, no spills
}
} // namespace
} // namespace sigsvgd
