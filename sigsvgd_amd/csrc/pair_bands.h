// The band-parallel schedule of the paired long-path solver (pair_bands.hip): its plan and its
// launch, as gram_long.hip's pair_launch sees them.
#pragma once

#include "sig_common.h"

namespace sigsvgd {

// the geometry of the serial paired plan that the band-parallel plan is built on (ring_make_plan's, as plain numbers)
struct PairGeom {
    int r, P, Q, nbands, nsteps, nrow;
    int serial_grid;      // the serial plan's grid: the per-pair scratch slots the workspace holds
    size_t wsk_per_block; // floats of one pair's scratch (0: forward only)
};

struct PairBandsPlan {
    int NB;                   // wavefronts per pair (1: the launch stays on the serial kernel)
    int W;                    // increment ring columns per wave (0 at order 0: increments are formed in registers)
    int nph, stride, phases;  // phases of one band, between the starts of a wave's bands, of one sweep of a pair
    int seam;                 // 1: more bands than waves, the last wave hands over to the first through a full boundary row
    int grid;                 // workgroups: min(resident, A, the serial grid)
    long long resident;       // workgroups the device holds
    size_t seam_doubles, wave_doubles, lds; // LDS: the seam row(s), one wave's share, the workgroup's bytes
};

// the plan of A pairs on M x N coarse grids in d channels at order n; bp.NB == 1 where the cooperative kernel has nothing to
// offer (one band, or LDS for one wave only)
void pair_bands_plan(int A, int M, int N, int d, int n, const PairGeom &g, PairBandsPlan &bp);
// wsk: the 256-B aligned scratch of the launch (NULL forward only)
int pair_bands_launch(const LongProblem &p, const PairGeom &g, const PairBandsPlan &bp, float *wsk);

} // namespace sigsvgd
