// What the four fp32-sweep Gram families (gram_fast_kernel.h, gram_quad.hip, gram_dyad.hip, gram_band.hip) have in common
// on the device, around their four different sweeps: the walk over a workgroup's range of items, the weights of a pair's
// two gradient sides and the rule that sends a pair to the exact fp64 pass.  Device-only value helpers, no kernel: every
// one returns a small struct or a scalar by value (through reference out-parameters hipcc schedules the callers differently).
#pragma once

#include "sig_common.h"

namespace sigsvgd {

// ---- item walk ---------------------------------------------------------------------------------------------------------
// The items of a launch -- (owned row tile, column), tile-major; symmetric launches only the columns from the tile's first
// row on -- all cost the same, so a grid of at most one workgroup per CU cuts them into contiguous equal ranges
// [nitems * b / grid, nitems * (b + 1) / grid).  A range touches few row tiles: the row-side sums of a wavefront's particle
// stay on the chip across the columns of a tile and go to the (workgroup, tile) segment's slot when the range leaves it.
struct ItemSeek {
    int kq, cstart; // the owned tile (in the launch's enumeration) and the column offset inside it where item `it0` lies
};
template <bool SYM>
__device__ __forceinline__ ItemSeek item_seek(const TileMap &tm, int B, int NW, long long it0)
{
    int kq = 0;
    long long rem = it0;
    for (;; ++kq) {
        const int cn = B - (SYM ? tm.tile_of(kq) * NW : 0);
        if (rem < cn) break;
        rem -= cn;
    }
    return {kq, (int)rem};
}
// the part of the range that lies in owned tile kq: rows i0 .. i0 + NW - 1 against the columns j0 .. j1 - 1
struct TileRange {
    int i0, cfirst, ncol; // first row; first column the tile has at all (SYM: the one that touches the diagonal); columns of the range in it
};
template <bool SYM>
__device__ __forceinline__ TileRange tile_range(const TileMap &tm, int B, int NW, int kq, int cstart, int remaining)
{
    const int itile = tm.tile_of(kq);
    const int cfirst = SYM ? itile * NW : 0;
    return {itile * NW, cfirst, min(B - cfirst - cstart, remaining)};
}
// where wavefront `wave` of this workgroup leaves the row-side sums (tot values) of its row of owned tile kq: a workgroup's
// range starts in at most one tile that another workgroup also works on, hence the segment kq + blockIdx.x (grad_geometry)
__device__ __forceinline__ double *rseg_slot(double *rseg, int kq, int NW, int wave, int tot)
{
    return rseg + (((size_t)(kq + (int)blockIdx.x)) * NW + wave) * (size_t)tot;
}

// ---- pair weights ------------------------------------------------------------------------------------------------------
// ij weighs d k(x_i, y_j) / d x_i (row side), ji the column side d k(x_i, x_j) / d x_j of a symmetric launch.  Without
// grad_out both are 1; `symw` (FLAG_SYM: the caller's weights are to be symmetrised) gives both sides w_ij + w_ji; the
// diagonal pair of a symmetric launch has its first-slot derivative only.
struct PairWeights {
    float ij, ji;
};
template <bool GRAD, bool SYM>
__device__ __forceinline__ PairWeights pair_weights(const void *go, int symw, int B, int i, int j, int io64)
{
    float w_ij = 1.f, w_ji = 1.f;
    if (GRAD) {
        if (go) {
            w_ij = (float)load_any(go, (size_t)i * B + j, io64);
            if (SYM || symw) w_ji = (float)load_any(go, (size_t)j * B + i, io64);
            if (symw) { w_ij += w_ji; w_ji = w_ij; }
        } else if (symw) {
            w_ij = 2.f; w_ji = 2.f;
        }
        if (SYM && j == i) w_ji = 0.f;
    }
    return {w_ij, w_ji};
}

// ---- the repair rule: which pairs the coverage kernel solves again in exact fp64 ------------------------------------------
// The fp32 sweeps run on fp32 increments; that is not enough where the discrete solution cancels or is ill-conditioned, so
// such pairs are flagged (one byte per pair, `kflag`) for the EXACT fp64 pass of the coverage kernel that follows the launch
// (fp64 static kernel, increments and sweeps: 6e-8).  The accuracy contract of include/sigsvgd_hip.h rests on this rule.
// With kden = max(|K[P][P]|, kRepairFloor), either of two findings flags the pair:
//   * CANCELLATION of magnitudes: the largest |K| on the pair's grid exceeds repair_ratio(d) * kden.  The fp32 sweeps
//     resolve about 5e-7 (T = 64) .. 2e-6 (T = 128) of the LARGEST value on the grid, the boundary value 1 included (an
//     earlier form also asked for a grid maximum above 2, which left pairs that merely decay to K < 1 / ratio unchecked:
//     they lose the same share of the largest value as pairs that oscillate).  The ratio is 2 in one channel, 4 in two,
//     8 beyond; the families' departures from it are stated where they call repair_ratio.
//     OPEN: the band kernels without the two-float add flag from 4 in three channels and more (repair_ratio(d, COMP ? 8 : 4)).
//     Neither DESIGN.md nor CHANGELOG.md records why; it is kept as it was, since 4 only sends more pairs to the exact pass.
//   * CONDITIONING (paths in few channels): K[P][P] as a function of the increments has the first-order condition number
//     c1 = sum |S * D| / |K| (S = K_fwd * U is dK/dD up to the stencil's second-order terms), and the fp32 STORAGE of the
//     increments (6e-8 each) costs K up to 2.7e-8 c1 whatever the precision of the sweeps (measured over 5,000 pairs of 25
//     roughness regimes, scripts/dev/cond_study.py: error <= 2.7e-8 c1, every pair beyond 3e-6 has c1 > 230; smooth paths
//     -- the bench inputs at d <= 3 -- stay below 100 at T <= 128).  The kernels hold gamma = D / sqrt(12), hence kSqrt12f.
//     Gradient launches have S after the reverse sweep and flag c1 > kRepairCond (repair_ill).  Forward-only launches have
//     no U and use the bound  sum |K_fwd * D| * max(grid maximum, 1) / kden > kRepairFwdBound  (repair_fwd_bound: >= c1 up
//     to 15 % in every pair of the study, within a factor 7 of it for three channels; no pair beyond 2.5e-6 stays below it).
//     So a forward-only and a gradient launch may flag different pairs: their K agree within the tolerance, not in the bits.
// A pair that came out NaN (a NaN in its inputs) is not marked: the coverage kernel's clamped exponential would turn it
// into a number.  The register-resident kernel also repairs in place: above kResweepRatio * kden it sweeps the pair again
// in fp64 on the same fp32 increments (resweep_fwd_fp64), which cures cancellation but not conditioning.
constexpr float kRepairFloor = 0.1f;
constexpr float kSqrt12f = 3.46410161513775459f;
constexpr float kRepairFwdBound = 300.f;
constexpr float kRepairCond = 150.f;
constexpr float kResweepRatio = 4.f;
__device__ __forceinline__ float repair_den(float kfin) { return fmaxf(fabsf(kfin), kRepairFloor); }
// (`wide`: the ratio from three channels on, for the families that depart from 8 there)
__device__ constexpr float repair_ratio(int d, float wide = 8.f) { return d == 1 ? 2.f : d == 2 ? 4.f : wide; }
// sds = sum |K_fwd * gamma| over the pair's cells, kmax = the grid maximum
__device__ __forceinline__ bool repair_fwd_bound(float sds, float kmax, float kden)
{
    return sds * kSqrt12f * fmaxf(kmax, 1.f) > kRepairFwdBound * kden;
}
// c1 = sum |S * gamma| over the pair's cells.  (The NaN test `kfin == kfin &&` stays with the caller, as on the forward side:
//  inside the helper hipcc turns the short circuit into a select and the gradient kernels come out three instructions apart.)
__device__ __forceinline__ bool repair_ill(float c1, float kden) { return c1 * kSqrt12f > kRepairCond * kden; }

} // namespace sigsvgd
