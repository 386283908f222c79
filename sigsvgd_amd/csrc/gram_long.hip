// Host side of the long-path route (DESIGN.md sections 5.10 - 5.16): the slab reduce kernels, the plans of the four modes,
// the workspace queries and the launchers.  The kernels and their families are in gram_long_kernels.h; this unit builds every
// kind but the Matern ones, which family_launch sends to gram_long_matern.hip, and launches with SIGSVGD_FLAG_EXACT_ADJOINT
//  go to gram_long_exact.hip: the plans, the workspace and everything behind the kernel are the same.
// Launches with SIGSVGD_FLAG_NORMALIZED are a short pipeline of their own, long2_norm_launch below; its
// diagonal pass, norm_diagonal_pass, also serves the fused Gram route's SIGSVGD_FLAG_NORMALIZED_FUSED (section 5.23; norm_diag_launch).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <vector>

#include "gram_long_kernels.h"
#include "pair_bands.h"

namespace sigsvgd {

// grad_partial[k][e] (fp64, whatever the I/O dtype) = row k's column-side slabs in the order of the owned tiles, then, where
// the launch owns k's tile, its row-side slabs in chunk order; slabs no pair wrote are skipped (the column side of a tile's
// first row; chunks that end at or before the diagonal), and a row that received nothing gets zero.  One block per row.
__global__ void long_part_reduce_kernel(const double *rowpart, const double *colpart, double *out, int A, int TD, int R, int JC,
                                        TileMap tm)
{
    const int k = blockIdx.x;
    const int own = tm.kq_of_tile(k / R);
    int oi0 = 0, onc = 0;
    const double *rows = nullptr;
    if (own >= 0) {
        oi0 = tm.tile_of(own) * R;
        onc = part_chunks(tm, own, A, R, JC);
        rows = rowpart + ((size_t)part_row_base(tm, own, A, R, JC) + (size_t)(k - oi0) * onc) * TD;
    }
    for (int e = threadIdx.x; e < TD; e += blockDim.x) {
        double s = 0.0;
        for (int kq = 0; kq < tm.owned; ++kq) {
            const int i0 = tm.tile_of(kq) * R;
            if (i0 < k) s += colpart[(size_t)(tm.start(kq, A, R, 1) + (k - i0)) * TD + e];
        }
        for (int c = 0; c < onc; ++c)
            if (oi0 + (c + 1) * JC > k) s += rows[(size_t)c * TD + e];
        out[(size_t)k * TD + e] = s;
    }
}

// out[k][e] = sum over slab c of partials[k][c][e], c = 0 .. nslabs - 1 in order (reproducible bits).  skip > 0 (yx): row k's
// column-side slab of its own diagonal tile, c = k / skip, was never written when k is that tile's first row (no pair i < k
// in it), and is left out.
template <typename IO>
__global__ void long2_reduce_kernel(const double *partials, IO *out, int rows, int nslabs, int TD, int skip)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)rows * TD) return;
    const size_t k = idx / TD, e = idx % TD;
    const int none = skip > 0 && k % skip == 0 ? (int)(k / skip) : -1;
    double s = 0.0;
    for (int c = 0; c < nslabs; ++c)
        if (c != none) s += partials[(k * nslabs + c) * TD + e];
    out[idx] = (IO)s;
}

namespace {
struct LongPlan : RingPlan {
    int JC, nchunks, grid;
    long long items;
    size_t wsk_bytes, partial_bytes, col_bytes = 0; // the forward scratch, the row-side slabs, the column-side slabs
    size_t len_bytes = 0; // SIGSVGD_FLAG_NAN_TAILS: the paths' lengths, ahead of the forward scratch
    bool log_k = false;   // SIGSVGD_FLAG_LOG_K: ring_log_plan's block exponents in LDS and scratch
    // SIGSVGD_FLAG_NORMALIZED: log_k, len_bytes holds the diagonals' logarithms, and behind the slabs
    // come the diagonals' gradients and the weighted sums (long2_norm_plan)
    size_t norm_bytes = 0;
    size_t total() const { return ring_ws_total(len_bytes + wsk_bytes + partial_bytes + col_bytes + norm_bytes); }
};

// The grid of a launch of pl.items work items and its forward scratch: one wavefront per item up to what the device holds,
// fewer (at least one) where their scratch would pass kRingMaxScratch; the scratch is rounded to 256 B.
void long_set_grid(LongPlan &pl)
{
    long long grid = pl.resident < pl.items ? pl.resident : pl.items;
    if (pl.per_wave * (size_t)grid > kRingMaxScratch) { // (per_wave is 0 for forward-only launches)
        grid = (long long)(kRingMaxScratch / pl.per_wave);
        if (grid < 1) grid = 1;
    }
    pl.grid = (int)grid;
    pl.wsk_bytes = ((pl.per_wave * (size_t)grid) + 255) & ~(size_t)255;
}

int long_make_plan(int A, int B, int M, int N, int d, int n, int want_grad, LongPlan &pl, const char *who = "gram_long")
{
    int rc = ring_make_plan(M, N, n, want_grad, d, who, pl); // (+ the band's nrow + 1 points of X_i in LDS)
    if (!rc && pl.log_k) rc = ring_log_plan(who, pl);
    if (rc) return rc;
    // work items (i, chunk of JC columns): enough to give every resident wave one, few enough gradient slabs
    int JC = 32;
    while (JC > 1 && (long long)A * ((B + JC - 1) / JC) < pl.resident) JC >>= 1;
    pl.JC = JC;
    pl.nchunks = (B + JC - 1) / JC;
    pl.items = (long long)A * pl.nchunks;
    long_set_grid(pl);
    pl.partial_bytes = want_grad ? (size_t)A * pl.nchunks * M * d * sizeof(double) : 0;
    return SIGSVGD_OK;
}

// the paired plan: the Gram plan of one column (items = A pairs, one per wavefront, grid = min(resident waves, A), the same
// LDS, cell limits and 1 GiB scratch cap); the gradients are written straight to the outputs, so there are no slabs
int pair_make_plan(int A, int M, int N, int d, int n, int want_grad, LongPlan &pl)
{
    const int rc = long_make_plan(A, 1, M, N, d, n, want_grad, pl, "pair");
    if (rc) return rc;
    pl.JC = 1;
    pl.partial_bytes = 0;
    return SIGSVGD_OK;
}

// The two-sided plan: tiles of IC rows x JC columns, the largest powers of two <= 32 that still give every resident wave an
// item (the wider side is halved first); yx: square tiles of the upper triangle.  Slabs: a row has one per column tile, a
// column one per row tile, so their bytes are (A ntj TX + B nti TY) d 8 at most; yx keeps the nti + 1 slabs a row can have
// (column side: tile rows 0 .. its own, row side: its own .. nti - 1) in one array.
struct Long2Plan : LongPlan {
    int IC, nti;
};

// want_bw (the bandwidth launch): the per-wave scratch of a reverse sweep whatever gradients are wanted, and nothing else.
int long2_make_plan(int A, int B, int M, int N, int d, int n, bool want_row, bool want_col, bool yx, Long2Plan &pl,
                    bool want_bw = false)
{
    const int want_grad = want_row || want_col;
    int rc = ring_make_plan(M, N, n, want_grad || want_bw, d, "gram_long", pl);
    if (!rc && pl.log_k) rc = ring_log_plan("gram_long", pl);
    if (rc) return rc;
    auto tiles = [](int rows, int chunk) { return (rows + chunk - 1) / chunk; };
    int IC = 32, JC = 32;
    if (yx) {
        auto tri = [&](int c) { return (long long)tiles(A, c) * (tiles(A, c) + 1) / 2; };
        while (IC > 1 && tri(IC) < pl.resident) IC >>= 1;
        JC = IC;
        pl.items = tri(IC);
    } else {
        while ((IC > 1 || JC > 1) && (long long)tiles(A, IC) * tiles(B, JC) < pl.resident) {
            if (JC >= IC)
                JC >>= 1;
            else
                IC >>= 1;
        }
        pl.items = (long long)tiles(A, IC) * tiles(B, JC);
    }
    pl.IC = IC;
    pl.JC = JC;
    pl.nti = tiles(A, IC);
    pl.nchunks = tiles(B, JC);
    long_set_grid(pl);
    const size_t rowslabs = yx ? (want_grad ? pl.nti + 1 : 0) : (want_row ? pl.nchunks : 0);
    pl.partial_bytes = (size_t)A * rowslabs * M * d * sizeof(double);
    pl.col_bytes = !yx && want_col ? (size_t)B * pl.nti * N * d * sizeof(double) : 0;
    return SIGSVGD_OK;
}

// What a launch with SIGSVGD_FLAG_NORMALIZED adds to its two-sided plan `pl`.  dx, dy: the paired
// log-domain plans of the diagonal passes (X_i, X_i) and, unless yx, (Y_j, Y_j), with the reverse sweep where that side's
// gradient is wanted; their scratch aliases the launch's, which grows to the largest of the three.  Behind the slabs: the fp64
// unit-weight gradients of the diagonal pairs, [A][TX][d] and [B][TY][d], then the weighted sums [A] and [B], each padded to
// 256 B and only where its side's gradient is wanted; and at the head, before the logarithms, the pairs' weights U [A][B]
// (norm_weights) of a gradient launch.  A forward-only launch adds neither.
struct NormPlan {
    LongPlan dx, dy;
    size_t diagX_bytes = 0, diagY_bytes = 0, sumX_bytes = 0, sumY_bytes = 0;
};
int long2_norm_plan(const LongProblem &p, bool want_row, bool want_gradY, bool yx, Long2Plan &pl, NormPlan &np)
{
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    np.dx.log_k = true;
    int rc = pair_make_plan(p.A, p.TX, p.TX, p.d, p.n, want_row, np.dx);
    if (rc) return rc;
    pl.wsk_bytes = std::max(pl.wsk_bytes, np.dx.wsk_bytes);
    if (!yx) {
        np.dy.log_k = true;
        rc = pair_make_plan(p.B, p.TY, p.TY, p.d, p.n, want_gradY, np.dy);
        if (rc) return rc;
        pl.wsk_bytes = std::max(pl.wsk_bytes, np.dy.wsk_bytes);
    }
    np.diagX_bytes = want_row ? pad((size_t)p.A * p.TX * p.d * sizeof(double)) : 0;
    np.diagY_bytes = want_gradY ? pad((size_t)p.B * p.TY * p.d * sizeof(double)) : 0;
    np.sumX_bytes = want_row ? pad((size_t)p.A * sizeof(double)) : 0;
    np.sumY_bytes = want_gradY ? pad((size_t)p.B * sizeof(double)) : 0;
    pl.norm_bytes = np.diagX_bytes + np.diagY_bytes + np.sumX_bytes + np.sumY_bytes;
    if (want_row || want_gradY) pl.len_bytes += norm_weight_bytes(p.A, p.B); // (ahead of the logarithms: long_set_lengths)
    return SIGSVGD_OK;
}

// ---- the partial plan ------------------------------------------------------------------------------
// One rank's share under a candidate (R, JC): its pairs, the most pairs one wavefront walks when item k goes to wave
// k % grid (the kernel's persistent loop), its slabs (units of TX * d doubles) and its items.  The items are enumerated in
// the order of part_decode.
struct PartShare {
    long long pairs = 0, makespan = 0, slabs = 0, items = 0, nfull = 0;
    TileMap tm;
};
PartShare part_share(int A, int R, int JC, int off, int stride, bool fold, long long resident)
{
    PartShare sh;
    sh.tm = make_tilemap((A + R - 1) / R, off, stride, fold);
    const TileMap &tm = sh.tm;
    for (int kq = 0; kq < tm.owned; ++kq) {
        const int nc = part_chunks(tm, kq, A, R, JC);
        sh.items += nc;
        sh.nfull += nc > 2 ? nc - 2 : 0;
        sh.slabs += (long long)part_rows(tm, kq, A, R) * nc + (A - tm.tile_of(kq) * R);
    }
    const long long grid = sh.items < resident ? (sh.items > 0 ? sh.items : 1) : resident;
    std::vector<long long> load((size_t)grid, 0);
    long long k = 0;
    auto take = [&](int kq, int c) {
        const int i0 = tm.tile_of(kq) * R, i1 = std::min(A, i0 + R), j0 = i0 + c * JC, j1 = std::min(A, j0 + JC);
        long long p = 0;
        for (int i = i0; i < i1; ++i) p += std::max(0, j1 - std::max(j0, i));
        sh.pairs += p;
        load[(size_t)(k++ % grid)] += p;
    };
    for (int kq = 0; kq < tm.owned; ++kq)
        for (int c = 1; c < part_chunks(tm, kq, A, R, JC) - 1; ++c) take(kq, c);
    for (int kq = 0; kq < tm.owned; ++kq) take(kq, 0);
    for (int kq = 0; kq < tm.owned; ++kq)
        if (part_chunks(tm, kq, A, R, JC) >= 2) take(kq, part_chunks(tm, kq, A, R, JC) - 1);
    sh.makespan = *std::max_element(load.begin(), load.end());
    return sh;
}

// The item rule: the largest R * JC (R a power of two <= 32 with at least two row tiles per rank, JC <= 64; ties: the larger
// R) under which, for every rank of `stride` with folded ownership,
//   schedule  ceil(pairs / resident) / makespan >= 0.9,
//   memory    slabs <= A * A / 4 where the share holds more than 16 pairs per resident wave, else <= 2 pairs + A (what
//             single-pair items cost),
//   balance   the fullest rank's pairs <= 1.05 x the mean.
// A share of no more pairs than resident waves gets single pairs by the schedule condition alone.  Where nothing meets all
// three (few rows on many ranks), the memory condition holds and the best balance, then schedule, is taken.  It depends on
// (A, stride, resident) only -- never on the rank -- and is searched once per such triple and process.
void part_pick(int A, int stride, long long resident, int &R_out, int &JC_out)
{
    static std::mutex mu;
    static std::map<std::tuple<int, int, long long>, std::pair<int, int>> cache;
    const auto key = std::make_tuple(A, stride, resident);
    std::lock_guard<std::mutex> lock(mu);
    const auto hit = cache.find(key);
    if (hit != cache.end()) {
        R_out = hit->second.first;
        JC_out = hit->second.second;
        return;
    }
    std::vector<std::pair<int, int>> cands;
    for (int R = 32; R >= 1; R >>= 1)
        for (int JC = 64; JC >= 1; --JC) cands.emplace_back(R, JC);
    std::stable_sort(cands.begin(), cands.end(), [](const std::pair<int, int> &x, const std::pair<int, int> &y) {
        return x.first * x.second > y.first * y.second;
    });
    const long long total = (long long)A * (A + 1) / 2;
    std::pair<int, int> best{1, 1};
    bool have = false, best_bal = false;
    double best_eff = -1.0;
    for (const auto &cd : cands) {
        const int R = cd.first, JC = cd.second;
        if (R > 1 && (A + R - 1) / R < 2 * stride) continue;
        bool mem_ok = true;
        double eff = 1.0;
        long long most = 0;
        for (int off = 0; off < stride && mem_ok; ++off) {
            const PartShare sh = part_share(A, R, JC, off, stride, true, resident);
            const long long bound = sh.pairs > 16 * resident ? (long long)A * A / 4 : 2 * sh.pairs + A;
            mem_ok = sh.slabs <= bound;
            if (sh.pairs > 0) eff = std::min(eff, (double)((sh.pairs + resident - 1) / resident) / (double)sh.makespan);
            most = std::max(most, sh.pairs);
        }
        if (!mem_ok) continue;
        const bool bal = (double)most * stride <= 1.05 * (double)total;
        if (eff >= 0.9 && bal) {
            best = cd;
            break;
        }
        if (!have || (bal && !best_bal) || (bal == best_bal && eff > best_eff)) {
            have = true;
            best = cd;
            best_bal = bal;
            best_eff = eff;
        }
    }
    cache[key] = best;
    R_out = best.first;
    JC_out = best.second;
}

struct PartPlan : LongPlan {
    int R;
    TileMap tm;
    long long nfull;
};

// the plan of rank `off` of `stride`; off < 0: the tile size only (sigsvgd_gram_long_partial_plan)
int part_make_plan(int A, int T, int d, int n, int off, int stride, bool fold, PartPlan &pl)
{
    const int rc = ring_make_plan(T, T, n, 1, d, "gram_long", pl);
    if (rc) return rc;
    part_pick(A, stride, pl.resident, pl.R, pl.JC);
    if (off < 0) return SIGSVGD_OK;
    const PartShare sh = part_share(A, pl.R, pl.JC, off, stride, fold, pl.resident);
    pl.tm = sh.tm;
    pl.items = sh.items;
    pl.nfull = sh.nfull;
    pl.nchunks = 0;
    long_set_grid(pl);
    const size_t TD = (size_t)T * d;
    pl.col_bytes = (size_t)sh.tm.start(sh.tm.owned, A, pl.R, 1) * TD * sizeof(double);
    pl.partial_bytes = (size_t)sh.slabs * TD * sizeof(double) - pl.col_bytes;
    return SIGSVGD_OK;
}

// The arguments every mode takes from the problem, its plan and the caller's workspace (checked against the plan's total; the
// row-side slabs follow the forward scratch).  B: the columns of the launch (1 in the paired mode).
int long_args(const char *who, const LongPlan &pl, const LongProblem &p, int B, LongArgs &a)
{
    unsigned char *base = nullptr;
    const int rc = ring_ws_base(who, p.ws, p.ws_bytes, pl.total(), base);
    if (rc) return rc;
    a.X = p.X; a.Y = p.Y; a.grad_out = p.grad_out; a.K_out = p.K_out;
    a.wsk = reinterpret_cast<float *>(base + pl.len_bytes); // (behind the lengths of a launch with NaN-marked tails)
    a.partials = pl.partial_bytes ? reinterpret_cast<double *>(base + pl.len_bytes + pl.wsk_bytes) : nullptr;
    a.wsk_per_block = pl.per_wave / sizeof(float);
    a.A = p.A; a.B = B; a.M = p.TX; a.N = p.TY; a.d = p.d; a.n = p.n; a.r = pl.r; a.P = pl.P; a.Q = pl.Q;
    a.nbands = pl.nbands; a.nsteps = pl.nsteps; a.nrow = pl.nrow; a.W = pl.W; a.JC = pl.JC; a.nchunks = pl.nchunks;
    a.sym = (p.flags & SIGSVGD_FLAG_SYM) ? 1 : 0; a.items = pl.items; a.inv_h = p.inv_h;
    a.inv_r2 = 1.0 / ((double)pl.r * (double)pl.r);
    return SIGSVGD_OK;
}
// the column-side slabs of the two-sided and partial modes: behind the forward scratch and the row-side slabs
double *long_colpart(const LongPlan &pl, const LongArgs &a)
{
    return pl.col_bytes ? reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(a.wsk) + pl.wsk_bytes + pl.partial_bytes)
                        : nullptr;
}
bool long_naive(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_NAIVE_SOLVER) != 0; }
bool long_yx(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_Y_IS_X) != 0; }
bool long_fold(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_FOLD_TILES) != 0; }
// SIGSVGD_FLAG_EXACT_ADJOINT where it changes the launch: with the first-order stencil GG is the exact
// adjoint already, and the launch is the unflagged one
bool long_exact(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_EXACT_ADJOINT) != 0 && !long_naive(p); }
// SIGSVGD_FLAG_NAN_TAILS: the bytes of the launch's length arrays (nY: Y's paths, 0 where Y is X), and
// the length pass into them, ahead of the launch on its stream (a: the launch's arguments, whose scratch follows the arrays)
bool long_nan_tails(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_NAN_TAILS) != 0; }
// SIGSVGD_FLAG_LOG_K (the entry points refuse it with NAIVE_SOLVER, EXACT_ADJOINT and NAN_TAILS)
bool long_log_k(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_LOG_K) != 0; }
// SIGSVGD_FLAG_NORMALIZED (the two-sided entry points only, which refuse it with the four flags above)
bool long_normalized(const LongProblem &p) { return (p.flags & SIGSVGD_FLAG_NORMALIZED) != 0; }
// Which instantiations a launch runs (family_launch).  The flags behind the modes exclude each other: the entry points refuse
// every pair of them, and an entry point that has no kernels of a mode refuses its flag, so any family may ask.
enum class LongMode { Plain, Exact, NanTails, LogK, Normalized };
LongMode long_mode(const LongProblem &p)
{
    return long_normalized(p) ? LongMode::Normalized
           : long_log_k(p)    ? LongMode::LogK
           : long_nan_tails(p) ? LongMode::NanTails
           : long_exact(p)     ? LongMode::Exact
                               : LongMode::Plain;
}
// what the plan of a launch takes from its flags, before it is made
void long_set_lengths(const LongProblem &p, int nY, LongPlan &pl)
{
    pl.len_bytes = long_nan_tails(p) ? nan_tail_bytes(p.A, nY) : long_normalized(p) ? norm_log_bytes(p.A, nY) : 0;
    pl.log_k = long_log_k(p) || long_normalized(p);
}
int long_find_lengths(const LongProblem &p, int nY, const LongPlan &pl, const LongArgs &a)
{
    if (!long_nan_tails(p)) return SIGSVGD_OK;
    int *lens = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(a.wsk) - pl.len_bytes);
    const hipError_t e = long_nan_tail_lengths(p.dtype, p.X, p.A, p.TX, nY ? p.Y : nullptr, nY, p.TY, p.d, lens, p.stream);
    return e != hipSuccess ? hip_fail(e, "launch nan_tail_length_kernel") : SIGSVGD_OK;
}

// out (the launch's dtype) = the sums of `rows` rows' slabs, long2_reduce_kernel
int long2_reduce(const LongProblem &p, const double *partials, void *out, int rows, int nslabs, int TD, int skip,
                 const char *what)
{
    const int bs = 256;
    const unsigned gs = (unsigned)(((size_t)rows * TD + bs - 1) / bs);
    if (p.dtype == SIGSVGD_F64)
        hipLaunchKernelGGL(long2_reduce_kernel<double>, dim3(gs), dim3(bs), 0, p.stream, partials, static_cast<double *>(out),
                           rows, nslabs, TD, skip);
    else
        hipLaunchKernelGGL(long2_reduce_kernel<float>, dim3(gs), dim3(bs), 0, p.stream, partials, static_cast<float *>(out),
                           rows, nslabs, TD, skip);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? hip_fail(e, what) : SIGSVGD_OK;
}

// ring_launch for the bandwidth families: the kinds that have a bandwidth, the first-order stencil where the route has it (RBF)
template <typename F, typename IO, typename Plan>
hipError_t bw_launch_kind(int kind, bool naive, const Plan &pl, hipStream_t stream, const typename F::Args &a)
{
    if (kind == SIGSVGD_STATIC_IMQ || kind == SIGSVGD_STATIC_RQ) {
        if (naive) return hipErrorInvalidValue; // (the entry points refuse it before this)
        return kind == SIGSVGD_STATIC_IMQ ? ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_IMQ>(pl, stream, a)
                                          : ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_RQ>(pl, stream, a);
    }
    if (kind != SIGSVGD_STATIC_RBF) return hipErrorInvalidValue;
    return naive ? ring_launch_one<F, IO, true, true, SIGSVGD_STATIC_RBF>(pl, stream, a)
                 : ring_launch_one<F, IO, false, true, SIGSVGD_STATIC_RBF>(pl, stream, a);
}
template <typename F, typename Plan>
int bw_launch(int dtype, int kind, bool naive, const Plan &pl, hipStream_t stream, const typename F::Args &a)
{
    hipError_t e = dtype == SIGSVGD_F64 ? bw_launch_kind<F, double>(kind, naive, pl, stream, a)
                                        : bw_launch_kind<F, float>(kind, naive, pl, stream, a);
    if (e != hipSuccess) return hip_fail(e, F::attr_failed);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, F::launch_failed);
    return SIGSVGD_OK;
}
// the launch of family F in mode `mode`.  Plain: ring_launch or bw_launch, and for the Matern kinds gram_long_matern.hip's
// instantiations; Exact (long_exact above; it changes a gradient launch with the default stencil only):
// gram_long_exact.hip's, for every kind; NanTails (SIGSVGD_FLAG_NAN_TAILS, the paired and the two-sided family):
// gram_long_nantail.hip's, for every kind and both stencils; LogK (SIGSVGD_FLAG_LOG_K, the same two families):
// gram_long_logk.hip's, for every kind; Normalized (SIGSVGD_FLAG_NORMALIZED, the same two): gram_long_norm.hip's, for every kind
template <typename F, typename Plan>
int family_launch(int dtype, int kind, bool naive, bool grad, const Plan &pl, hipStream_t stream, const typename F::Args &a,
                  LongMode mode = LongMode::Plain)
{
    if (mode == LongMode::Normalized) { // (the entry points refuse it with the other three and with the first-order stencil)
        hipError_t e = long_norm_launch(F::id, dtype, kind, grad, pl.grid, pl.lds, stream, &a);
        if (e != hipSuccess) return hip_fail(e, F::attr_failed);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, F::launch_failed);
        return SIGSVGD_OK;
    }
    if (mode == LongMode::LogK) { // (the entry points refuse it with the other two and with the first-order stencil)
        hipError_t e = long_log_k_launch(F::id, dtype, kind, grad, pl.grid, pl.lds, stream, &a);
        if (e != hipSuccess) return hip_fail(e, F::attr_failed);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, F::launch_failed);
        return SIGSVGD_OK;
    }
    if (mode == LongMode::NanTails) { // (the entry points refuse it with the exact adjoint and on families without such kernels)
        hipError_t e = long_nan_tail_launch(F::id, dtype, kind, naive, grad, pl.grid, pl.lds, stream, &a);
        if (e != hipSuccess) return hip_fail(e, F::attr_failed);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, F::launch_failed);
        return SIGSVGD_OK;
    }
    if (mode == LongMode::Exact && grad && !naive) {
        hipError_t e = long_exact_launch(F::id, dtype, kind, pl.grid, pl.lds, stream, &a);
        if (e != hipSuccess) return hip_fail(e, F::attr_failed);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, F::launch_failed);
        return SIGSVGD_OK;
    }
    if (kind != SIGSVGD_STATIC_MATERN32 && kind != SIGSVGD_STATIC_MATERN52) {
        if constexpr (F::bandwidth)
            return bw_launch<F>(dtype, kind, naive, pl, stream, a);
        else
            return ring_launch<F>(dtype, kind, naive, grad, pl, stream, a);
    }
    // (the entry points refuse NAIVE_SOLVER with these kinds before this)
    hipError_t e = naive ? hipErrorInvalidValue : long_matern_launch(F::id, dtype, kind, grad, pl.grid, pl.lds, stream, &a);
    if (e != hipSuccess) return hip_fail(e, F::attr_failed);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, F::launch_failed);
    return SIGSVGD_OK;
}
} // namespace

// ---- workspace queries and launches; the argument checks are the entry points' (capi.hip) ----------------------------------
// Bytes of a launch's workspace (0 for forward-only launches: the forward sweep keeps nothing; 0 for a rank of the partial mode
// that owns no tile).  The queries read the problem's shape, order and flags only.
int long_workspace(const LongProblem &p, int want_grad, size_t *bytes)
{
    return ring_plan_total<LongPlan>(
        bytes, [&](LongPlan &pl) { return long_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_grad, pl); });
}
int pair_workspace(const LongProblem &p, int want_grad, size_t *bytes)
{
    return ring_plan_total<LongPlan>(bytes, [&](LongPlan &pl) {
        long_set_lengths(p, p.A, pl);
        return pair_make_plan(p.A, p.TX, p.TY, p.d, p.n, want_grad, pl);
    });
}
int long2_workspace(const LongProblem &p, int want_gradX, int want_gradY, size_t *bytes)
{
    return ring_plan_total<Long2Plan>(bytes, [&](Long2Plan &pl) {
        long_set_lengths(p, long_yx(p) ? 0 : p.B, pl);
        int rc = long2_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_gradX != 0, want_gradY != 0, long_yx(p), pl);
        NormPlan np;
        if (!rc && long_normalized(p)) rc = long2_norm_plan(p, want_gradX != 0, want_gradY != 0, long_yx(p), pl, np);
        return rc;
    });
}
// the two-sided bandwidth launch: the scratch also where neither coordinate gradient is wanted (the paired one's workspace is
// pair_workspace's with the gradient: the scratch alone)
int long2_h_workspace(const LongProblem &p, int want_gradX, int want_gradY, size_t *bytes)
{
    return ring_plan_total<Long2Plan>(bytes, [&](Long2Plan &pl) {
        return long2_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_gradX != 0, want_gradY != 0, long_yx(p), pl, true);
    });
}
int long_part_workspace(const LongProblem &p, int off, int stride, size_t *bytes)
{
    return ring_plan_total<PartPlan>(
        bytes, [&](PartPlan &pl) { return part_make_plan(p.A, p.TX, p.d, p.n, off, stride, long_fold(p), pl); });
}
// the partial mode's tile: R rows x JC columns, the same for every rank of `stride` (host only)
int long_part_tiles(const LongProblem &p, int stride, int *R, int *JC)
{
    PartPlan pl;
    const int rc = part_make_plan(p.A, p.TX, p.d, p.n, -1, stride, true, pl);
    if (rc) return rc;
    *R = pl.R;
    *JC = pl.JC;
    return SIGSVGD_OK;
}

// gradX_out == NULL: forward only
int long_launch(const LongProblem &p)
{
    const bool want_grad = p.gradX_out != nullptr;
    LongPlan pl;
    LongArgs a;
    int rc = long_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_grad, pl);
    if (!rc) rc = long_args("gram_long", pl, p, p.B, a);
    if (!rc) rc = family_launch<LongFamily<false>>(p.dtype, p.kind, long_naive(p), want_grad, pl, p.stream, a, long_mode(p));
    if (!rc && want_grad) // a row's slabs in chunk order
        rc = long2_reduce(p, a.partials, p.gradX_out, p.A, pl.nchunks, p.TX * p.d, 0, "launch long2_reduce_kernel (rows)");
    return rc;
}

// ---- the paired mode's schedule: one wavefront per pair (gram_long_kernel) or a workgroup per pair (pair_bands.hip) --------
namespace {
PairGeom pair_geom(const LongPlan &pl)
{
    return PairGeom{pl.r, pl.P, pl.Q, pl.nbands, pl.nsteps, pl.nrow, pl.grid, pl.per_wave / sizeof(float)};
}
// Whether a paired launch runs the band-parallel kernel under plan bp.  SIGSVGD_PAIR_MODE=serial|bands (read per launch; tests
// and measurements only, the results have the same bits; any other value is ignored) pins it wherever the plan has two waves
// or more.  Default rule: bands where its dependent steps, over the rounds the launch takes, are
// fewer than a third of the serial schedule's,
//   3 * rounds_bands * phases * 16  <  rounds_serial * nbands * nsteps,      rounds = ceil(A / workgroups or waves in flight).
// The 3 is the measured cost of a band-parallel step against a serial one (2.2 - 2.6: two waves share a SIMD, and a barrier
// every 16 steps), rounded up.  Few bands per pair, or pairs enough to fill the device in both schedules, stay serial.
bool pair_use_bands(int A, const LongPlan &pl, const PairBandsPlan &bp)
{
    if (bp.NB < 2) return false;
    const char *e = getenv("SIGSVGD_PAIR_MODE");
    if (e && !strcmp(e, "serial")) return false;
    if (e && !strcmp(e, "bands")) return true;
    const long long rounds_b = (A + bp.grid - 1) / bp.grid, rounds_s = (A + pl.grid - 1) / pl.grid;
    return 3 * rounds_b * bp.phases * 16 < rounds_s * (long long)pl.nbands * pl.nsteps;
}
} // namespace

// what a paired launch would run now (host only): waves per pair, workgroups, LDS bytes per workgroup
int pair_schedule(const LongProblem &p, int want_grad, int *waves_per_pair, int *grid, size_t *lds_bytes)
{
    LongPlan pl;
    pl.log_k = long_log_k(p);
    const int rc = pair_make_plan(p.A, p.TX, p.TY, p.d, p.n, want_grad, pl);
    if (rc) return rc;
    PairBandsPlan bp;
    pair_bands_plan(p.A, p.TX, p.TY, p.d, p.n, pair_geom(pl), bp);
    // (the exact adjoint has the one-wavefront kernel only: pair_bands.hip has its own sweep)
    // (and so have launches with NaN-marked tails, whose pairs differ in their bands, and log-domain launches)
    const bool bands = !(want_grad && long_exact(p)) && !long_nan_tails(p) && !long_log_k(p) && pair_use_bands(p.A, pl, bp);
    *waves_per_pair = bands ? bp.NB : 1;
    *grid = bands ? bp.grid : pl.grid;
    *lds_bytes = bands ? bp.lds : pl.lds;
    return SIGSVGD_OK;
}

// gradX_out and gradY_out both NULL: forward only
int pair_launch(const LongProblem &p)
{
    const bool want_grad = p.gradX_out != nullptr || p.gradY_out != nullptr;
    LongPlan pl;
    PairArgs a;
    long_set_lengths(p, p.A, pl);
    int rc = pair_make_plan(p.A, p.TX, p.TY, p.d, p.n, want_grad, pl);
    if (!rc) rc = long_args("pair", pl, p, 1, a);
    if (rc) return rc;
    PairBandsPlan bp;
    pair_bands_plan(p.A, p.TX, p.TY, p.d, p.n, pair_geom(pl), bp);
    const bool exact = want_grad && long_exact(p); // (the one-wavefront schedule, as the bandwidth launch)
    if (!exact && !long_nan_tails(p) && !long_log_k(p) && pair_use_bands(p.A, pl, bp))
        return pair_bands_launch(p, pair_geom(pl), bp, a.wsk); // the same scratch slots, fewer used
    a.gradX = p.gradX_out; a.gradY = p.gradY_out;
    rc = long_find_lengths(p, p.A, pl, a);
    if (rc) return rc;
    return family_launch<LongFamily<true>>(p.dtype, p.kind, long_naive(p), want_grad, pl, p.stream, a, long_mode(p));
}

// The paired launch with the bandwidth derivative: dk_out[A] = dK_i / d inv_h.  Always the one-wavefront
// schedule (pair_bands.hip has no bandwidth pass) with the reverse sweep; gradX_out and gradY_out may both be NULL.
int pair_h_launch(const LongProblem &p, void *dk_out)
{
    LongPlan pl;
    PairHArgs a;
    int rc = pair_make_plan(p.A, p.TX, p.TY, p.d, p.n, 1, pl);
    if (!rc) rc = long_args("pair", pl, p, 1, a);
    if (rc) return rc;
    a.gradX = p.gradX_out; a.gradY = p.gradY_out; a.dK_dinvh = dk_out;
    return family_launch<PairHFamily>(p.dtype, p.kind, long_naive(p), true, pl, p.stream, a, long_mode(p));
}

// The two-sided launch, with the bandwidth derivative where dk_out is given (dk_out[A][B] =
// dK_ij / d inv_h; the reverse sweep then runs whatever gradients are wanted, and the plan of the gradients' slabs and tiles is
// the one the launch without dk_out makes).
// gradX_out and gradY_out both NULL: forward only.  Y_IS_X: A == B, TX == TY, no gradY_out; gradX_out then gets both sides of
// every unordered pair.
namespace {
// A diagonal pass of a normalised launch (DESIGN.md sections 5.22, 5.23): `rows` paths of T points in both slots on the paired
// log-domain plan dp, the paired NormIO kernel on problem p's stream with its dtype, kind, order and bandwidth.  ln_out[rows] gets
// ln K(x, x) unrounded, grad[rows][T][d] (where given) the pair's unit-weight gradient in both slots, both fp64; wsk: the
// launch's scratch (not the head of p's workspace, where the long route keeps the logarithms), dp.wsk_bytes of it at least.
int norm_diagonal_pass(const LongProblem &p, const LongPlan &dp, const void *paths, int rows, int T, float *wsk, double *ln_out,
                       double *grad)
{
    LongProblem q = p;
    q.X = q.Y = paths; q.A = rows; q.TX = q.TY = T; q.grad_out = nullptr; q.K_out = ln_out;
    PairArgs da;
    const int rc = long_args("gram_long", dp, q, 1, da);
    if (rc) return rc;
    da.wsk = wsk;
    da.gradX = grad; da.gradY = nullptr;
    return family_launch<LongFamily<true>>(p.dtype, p.kind, false, grad != nullptr, dp, p.stream, da, LongMode::Normalized);
}

// The launch with SIGSVGD_FLAG_NORMALIZED on plan pl + np with the two-sided arguments a, all on the
// caller's stream: the diagonal passes (the paired NormIO kernel on (X, X) and, unless yx, on (Y, Y): ln K unrounded to the head
// of the workspace, the pairs' unit-weight gradients where wanted), the two-sided NormIO kernel (each pair solved once; K^ stored,
// the slabs weighted by U = w K^, which it files too; yx: the diagonal pairs by 0), the row and column sums of U, and the slab
// reductions that add -1/2 sum times the diagonal's gradient.
int long2_norm_launch(const LongProblem &p, const Long2Plan &pl, const NormPlan &np, const Long2Args &a)
{
    const bool yx = long_yx(p), want_row = p.gradX_out != nullptr, want_gradY = p.gradY_out != nullptr;
    unsigned char *scratch = reinterpret_cast<unsigned char *>(a.wsk);
    double *lnA = reinterpret_cast<double *>(scratch - norm_log_bytes(p.A, yx ? 0 : p.B)), *lnB = lnA + p.A;
    const double *U = reinterpret_cast<const double *>(scratch - pl.len_bytes); // (gradient launches: norm_weights)
    unsigned char *tail = scratch + pl.wsk_bytes + pl.partial_bytes + pl.col_bytes;
    double *diagX = reinterpret_cast<double *>(tail), *diagY = reinterpret_cast<double *>(tail + np.diagX_bytes);
    double *sumX = reinterpret_cast<double *>(tail + np.diagX_bytes + np.diagY_bytes);
    double *sumY = reinterpret_cast<double *>(tail + np.diagX_bytes + np.diagY_bytes + np.sumX_bytes);
    int rc = norm_diagonal_pass(p, np.dx, p.X, p.A, p.TX, a.wsk, lnA, want_row ? diagX : nullptr);
    if (!rc && !yx) rc = norm_diagonal_pass(p, np.dy, p.Y, p.B, p.TY, a.wsk, lnB, want_gradY ? diagY : nullptr);
    if (!rc)
        rc = family_launch<Long2Family>(p.dtype, p.kind, false, a.want_row || a.want_col, pl, p.stream, a, LongMode::Normalized);
    if (rc || (!want_row && !want_gradY)) return rc;
    hipError_t e = long_norm_sums(U, p.A, p.B, want_row ? sumX : nullptr, want_gradY ? sumY : nullptr, p.stream);
    if (e != hipSuccess) return hip_fail(e, "launch long_norm_sums_kernel");
    if (want_row) { // yx: a row's nti + 1 slabs, column side first
        e = long_norm_reduce(p.dtype, a.partials, p.gradX_out, p.A, yx ? pl.nti + 1 : pl.nchunks, p.TX * p.d, yx ? pl.IC : 0, sumX,
                             diagX, p.stream);
        if (e != hipSuccess) return hip_fail(e, "launch long_norm_reduce_kernel (rows)");
    }
    if (want_gradY) {
        e = long_norm_reduce(p.dtype, a.colpart, p.gradY_out, p.B, pl.nti, p.TY * p.d, 0, sumY, diagY, p.stream);
        if (e != hipSuccess) return hip_fail(e, "launch long_norm_reduce_kernel (columns)");
    }
    return SIGSVGD_OK;
}

template <bool BW>
int long2_launch_any(const LongProblem &p, void *dk_out)
{
    const bool yx = long_yx(p), want_row = p.gradX_out != nullptr, want_col = p.gradY_out != nullptr || (yx && want_row);
    Long2Plan pl;
    std::conditional_t<BW, Long2HArgs, Long2Args> a;
    long_set_lengths(p, yx ? 0 : p.B, pl); // (BW: the entry points refuse the flag)
    int rc = long2_make_plan(p.A, p.B, p.TX, p.TY, p.d, p.n, want_row, p.gradY_out != nullptr, yx, pl, BW);
    [[maybe_unused]] NormPlan np;
    if constexpr (!BW) {
        if (!rc && long_normalized(p)) rc = long2_norm_plan(p, want_row, p.gradY_out != nullptr, yx, pl, np);
    }
    if (!rc) rc = long_args("gram_long", pl, p, p.B, a);
    if (rc) return rc;
    a.colpart = long_colpart(pl, a);
    a.IC = pl.IC; a.nti = pl.nti; a.yx = yx ? 1 : 0; a.want_row = want_row ? 1 : 0; a.want_col = want_col ? 1 : 0;
    if constexpr (!BW) {
        if (long_normalized(p)) return long2_norm_launch(p, pl, np, a);
    }
    if constexpr (BW) {
        a.dK_dinvh = dk_out;
        rc = family_launch<Long2HFamily>(p.dtype, p.kind, long_naive(p), true, pl, p.stream, a, long_mode(p));
    } else {
        rc = long_find_lengths(p, yx ? 0 : p.B, pl, a);
        if (!rc)
            rc = family_launch<Long2Family>(p.dtype, p.kind, long_naive(p), want_row || want_col, pl, p.stream, a, long_mode(p));
    }
    if (!rc && want_row) // yx: a row's nti + 1 slabs, column side first
        rc = long2_reduce(p, a.partials, p.gradX_out, p.A, yx ? pl.nti + 1 : pl.nchunks, p.TX * p.d, yx ? pl.IC : 0,
                          "launch long2_reduce_kernel (rows)");
    if (!rc && p.gradY_out)
        rc = long2_reduce(p, a.colpart, p.gradY_out, p.B, pl.nti, p.TY * p.d, 0, "launch long2_reduce_kernel (columns)");
    return rc;
}
} // namespace
int long2_launch(const LongProblem &p) { return long2_launch_any<false>(p, nullptr); }
int long2_h_launch(const LongProblem &p, void *dk_out) { return long2_launch_any<true>(p, dk_out); }

// The diagonal pass for the fused Gram route (SIGSVGD_FLAG_NORMALIZED_FUSED; capi.hip).
// norm_diag_workspace: the bytes of its scratch (alignment slack included; the plan's refusals and messages) for `rows` paths of
// T points.  norm_diag_launch: p.X = the paths, p.A = the rows, p.TX = the points, p.ws / p.ws_bytes = that scratch; ln_out and
// grad (NULL: forward only) as norm_diagonal_pass takes them.
int norm_diag_workspace(int rows, int T, int d, int n, int want_grad, size_t *bytes)
{
    return ring_plan_total<LongPlan>(bytes, [&](LongPlan &pl) {
        pl.log_k = true;
        return pair_make_plan(rows, T, T, d, n, want_grad, pl);
    });
}
int norm_diag_launch(const LongProblem &p, double *ln_out, double *grad)
{
    LongPlan dp;
    dp.log_k = true;
    int rc = pair_make_plan(p.A, p.TX, p.TX, p.d, p.n, grad != nullptr, dp);
    unsigned char *base = nullptr;
    if (!rc) rc = ring_ws_base("gram_norm_fused (diagonal pass)", p.ws, p.ws_bytes, dp.total(), base);
    if (rc) return rc;
    return norm_diagonal_pass(p, dp, p.X, p.A, p.TX, reinterpret_cast<float *>(base), ln_out, grad);
}

// The share of rank `off` of `stride` (Y = X: B = A, TY = TX).  K_out gets the owned pairs and their mirror images, gradX_out
// (fp64 whatever the dtype) is overwritten whole; a rank that owns no tile launches the reduction alone, which writes zeros.
int long_part_launch(const LongProblem &p, int off, int stride)
{
    PartPlan pl;
    PartArgs a;
    int rc = part_make_plan(p.A, p.TX, p.d, p.n, off, stride, long_fold(p), pl);
    if (!rc) rc = long_args("gram_long_sym_partial", pl, p, p.A, a);
    if (rc) return rc;
    a.colpart = long_colpart(pl, a);
    a.tm = pl.tm; a.R = pl.R; a.nfull = pl.nfull;
    if (pl.items > 0) rc = family_launch<PartFamily>(p.dtype, p.kind, long_naive(p), true, pl, p.stream, a);
    if (rc) return rc;
    hipLaunchKernelGGL(long_part_reduce_kernel, dim3(p.A), dim3(256), 0, p.stream, a.partials, a.colpart,
                       static_cast<double *>(p.gradX_out), p.A, p.TX * p.d, pl.R, pl.JC, pl.tm);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch long_part_reduce_kernel");
    return SIGSVGD_OK;
}


} // namespace sigsvgd
