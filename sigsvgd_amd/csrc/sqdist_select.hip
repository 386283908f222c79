// Exact order statistic of the squared distances between the points of two batches of paths,
//     { |X_ip - Y_jq|^2 : i < A, j < B, p < TX, q < TY },
// without the [A, B, TX, TY] tensor (sigsvgd_sqdist_select, include/sigsvgd_hip.h).  The median of
// this multiset is the reference's default bandwidth (bw_median, src/utils/math.py:28-34).
//
// Values.  fp64 in difference form, sum_k (x_k - y_k)^2 in channel order, fp32 inputs converted exactly.  The sum starts
// from +0 and adds squares, so it is never negative and never -0 and its bit pattern as a 64-bit unsigned integer orders like
// the number; (x - y)^2 and (y - x)^2 are the same bits, so the value of (i, j, p, q) is the value of (j, i, q, p).
//
// Selection.  A radix select on the pattern, most significant digit first: 12 + 12 + 12 + 12 + 12 + 4 bits, six passes at
// the most whatever the input.  Pass t (select_pass_kernel) counts, among the elements whose leading bits equal the prefix
// chosen so far, the values of digit t; select_pick_kernel (one workgroup) then finds the digit that holds the wanted rank,
// appends it to the prefix and lowers the rank by the count below it.  The state stays in the workspace: there is no host
// read-back, the six pass / pick launches are enqueued unconditionally and each reads what to do.  A pass recomputes every
// distance until the bucket of the prefix fits the candidate buffer (and is sparse enough to be worth writing); the next pass then also writes the bucket's
// patterns to a candidate buffer, and the passes after it count over that buffer alone.  After the last digit the prefix is
// the value.
//
// Counts.  Integer, so the result does not depend on arrival order: per-workgroup 32-bit LDS bins (flushed before they can
// wrap), added to 64-bit global bins with vector atomics; the rank and every prefix sum are 64-bit.
//
// Concentrated digits.  The leading digit is the exponent: nearly every element of a launch falls into two or three bins, and
// one LDS atomic per lane and element would serialise on them.  Each lane keeps ONE register counter for the bin it saw last
// and touches the LDS only when the bin changes (and once at the end): on a concentrated digit that is a handful of LDS adds
// per lane and launch, on a spread digit (mantissa bits) one per matching element, where the lanes' bins differ and do not
// collide.  The same counter makes the all-equal multiset and integer-valued data (every later digit in one bin) cheap.
#include "sig_common.h"

namespace sigsvgd {

namespace {
typedef unsigned long long u64;

constexpr int kSelThreads = 256;
constexpr int kDigitBits = 12;
constexpr int kBins = 1 << kDigitBits;
constexpr int kSelPasses = 6;                 // 5 x 12 + 4 bits
constexpr unsigned kCandCap = 1u << 20;       // candidate elements: a pattern and how often it counts
constexpr unsigned kDenseCap = 1u << 16;      // a bucket above this is gathered only where it is sparse: 1 / 64 of the elements
constexpr unsigned kLdsCand = 512;            // candidates a workgroup collects in LDS before it claims room for them
constexpr int kTileBytes = 28 * 1024;         // LDS of the two staged point sets
constexpr int kRowBlock = 4, kColBlock = 4;   // the rows x columns a lane accumulates at once
typedef double d4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));
constexpr int kMaxCols = 512;                 // columns of a work item at the most
constexpr int kPickThreads = 1024;
constexpr size_t kLdsHist = kBins * sizeof(unsigned);
constexpr size_t kLdsFixed = kLdsHist + kLdsCand * (sizeof(u64) + 1) + 16; // bins, candidates and their weights, two counters
static_assert(kLdsFixed % 16 == 0 && kLdsCand % 16 == 0, "LDS areas keep 16-B alignment");

enum : unsigned { MODE_COUNT = 0, MODE_GATHER = 1, MODE_CAND = 2 };

// the select's state, at the (256-B aligned) start of the workspace; sigsvgd_amd/ops.py reads `passes` for scripts/median_time.py
struct SelState {
    u64 prefix;      // the leading bits chosen so far, right-aligned
    u64 rank;        // the wanted rank inside the prefix's bucket
    u64 count;       // elements in the bucket
    unsigned mode;   // what the next pass does: count over all elements / that and gather the bucket / count over the candidates
    unsigned passes; // passes that recomputed the distances
    unsigned ncand;  // candidates written by the gathering pass (at most kCandCap: the bucket's count bounds them)
    unsigned pad;
    u64 total;       // n, the elements of the multiset
};
constexpr size_t kStateBytes = 256;
constexpr size_t kHistBytes = (size_t)kSelPasses * kBins * sizeof(u64);
constexpr size_t kCandBytes = (size_t)kCandCap * (sizeof(u64) + 1); // patterns, then one byte of weight each
constexpr size_t kSelWsBytes = kStateBytes + kHistBytes + kCandBytes + 256;

__host__ __device__ inline int digit_shift(int t) { return t < 5 ? 52 - kDigitBits * t : 0; }
__host__ __device__ inline int digit_bits(int t) { return t < 5 ? kDigitBits : 4; }

struct SelGeom {
    int PB, CG, DB, nd, QC; // rows of a tile (64, 128 or 256), column groups of its lanes (256 / (PB / 4)), channels staged at
                            // once, channel blocks, columns of a tile (a multiple of 4 CG)
    long long npb, nch;    // row blocks of a path of X, column chunks of a row's columns
    long long NO;          // paths of Y a row of X meets (Y_IS_X: itself and the next A / 2, cyclically)
    long long items;
    int grid;
};

SelGeom select_geometry(int A, int B, int TX, int TY, int d, bool yx)
{
    SelGeom g;
    g.PB = TX <= 64 ? 64 : (TX <= 128 ? 128 : 256);
    g.CG = kSelThreads / (g.PB / kRowBlock);
    const int mincols = kColBlock * g.CG;
    const int fit = kTileBytes / 8 / (g.PB + mincols); // channels that fit beside the smallest column chunk
    g.DB = d < fit ? d : fit;
    g.nd = (d + g.DB - 1) / g.DB;
    g.NO = yx ? (long long)A / 2 + 1 : (long long)B;
    const long long cols = g.NO * TY;
    if (g.nd == 1) {
        long long qc = (kTileBytes / 8 / d - g.PB) / mincols * mincols;
        if (qc > kMaxCols) qc = kMaxCols;
        const long long need = (cols + mincols - 1) / mincols * mincols;
        if (qc > need) qc = need;
        g.QC = (int)qc;
    } else {
        g.QC = mincols; // wide paths: the accumulators of one column block live across the channel blocks
    }
    g.npb = (TX + g.PB - 1) / g.PB;
    g.nch = (cols + g.QC - 1) / g.QC;
    g.items = (long long)A * g.npb * g.nch;
    const long long resident = (long long)device_cu_count() * 3;
    g.grid = (int)(g.items < resident ? g.items : resident);
    return g;
}

struct SelArgs {
    const void *X, *Y;
    int A, B, TX, TY, d, dtype, yx;
    SelGeom g;
    SelState *st;
    u64 *hist; // [kSelPasses][kBins]
    u64 *cand; // [kCandCap]
    unsigned char *candw; // [kCandCap]
    double *out;
    int pass;
};

__device__ __forceinline__ double load_point(const void *P, long long idx, int dtype)
{
    return dtype == SIGSVGD_F64 ? static_cast<const double *>(P)[idx] : (double)static_cast<const float *>(P)[idx];
}

// one lane's run counter: the bin seen last and how many elements of it are not in the LDS bins yet
struct Run {
    int bin = 0;
    unsigned cnt = 0;
};
__device__ __forceinline__ void run_flush(Run &r, unsigned *s_hist)
{
    if (r.cnt) atomicAdd(&s_hist[r.bin], r.cnt);
    r.cnt = 0;
}
__device__ __forceinline__ void run_add(Run &r, unsigned *s_hist, int bin, unsigned w)
{
    if (bin != r.bin) {
        run_flush(r, s_hist);
        r.bin = bin;
    }
    r.cnt += w;
}

// the workgroup's LDS bins into the global ones (and zero again); every thread calls it
__device__ void flush_bins(Run &r, unsigned *s_hist, u64 *hist, int nbins)
{
    run_flush(r, s_hist);
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += kSelThreads) {
        const unsigned c = s_hist[b];
        if (c) {
            atomicAdd(&hist[b], (u64)c);
            s_hist[b] = 0;
        }
    }
    __syncthreads();
}

// the workgroup's collected candidates to the global buffer: one returning atomic claims their room; every thread calls it
__device__ void flush_cands(const SelArgs &a, const u64 *s_cand, const unsigned char *s_cw, unsigned *s_nc, unsigned *s_base)
{
    __syncthreads();
    const unsigned n = *s_nc < kLdsCand ? *s_nc : kLdsCand;
    if (threadIdx.x == 0 && n) *s_base = atomicAdd(&a.st->ncand, n);
    __syncthreads();
    const unsigned base = *s_base;
    for (unsigned e = threadIdx.x; e < n; e += kSelThreads)
        if (base + e < kCandCap) {
            a.cand[base + e] = s_cand[e];
            a.candw[base + e] = s_cw[e];
        }
    __syncthreads();
    if (threadIdx.x == 0) *s_nc = 0;
    __syncthreads();
}

__global__ __launch_bounds__(kSelThreads) void select_pass_kernel(SelArgs a)
{
    // all LDS in the dynamic region, every offset a multiple of 16 B: the 16-B reads of the inner loop need their alignment
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    unsigned *s_hist = reinterpret_cast<unsigned *>(s_mem);                       // [kBins]
    u64 *s_cand = reinterpret_cast<u64 *>(s_mem + kLdsHist);                      // [kLdsCand]
    unsigned char *s_cw = s_mem + kLdsHist + kLdsCand * sizeof(u64);              // [kLdsCand]
    unsigned *s_ctl = reinterpret_cast<unsigned *>(s_cw + kLdsCand);              // candidates collected, their global base
    unsigned &s_nc = s_ctl[0], &s_base = s_ctl[1];
    const SelGeom &g = a.g;
    double *Xs = reinterpret_cast<double *>(s_mem + kLdsFixed); // [DB][PB]
    double *Ys = Xs + (size_t)g.DB * g.PB;       // [DB][QC]
    int *Ws = reinterpret_cast<int *>(Ys + (size_t)g.DB * g.QC); // [QC] how often a column's elements count; 0: no column

    const int tid = threadIdx.x;
    const int t = a.pass;
    const int shift = digit_shift(t), bits = digit_bits(t), nbins = 1 << bits;
    const SelState st = *a.st;
    const unsigned mode = st.mode;
    const int pshift = shift + bits;
    const u64 prefmask = pshift >= 64 ? 0ull : ~0ull << pshift;
    const u64 prefval = pshift >= 64 ? 0ull : st.prefix << pshift;
    u64 *hist = a.hist + (size_t)t * kBins;

    for (int b = tid; b < kBins; b += kSelThreads) s_hist[b] = 0;
    if (tid == 0) s_nc = 0;
    __syncthreads();
    Run run;

    if (mode == MODE_CAND) { // the bucket was gathered by an earlier pass: count over its patterns
        const unsigned nc = st.ncand < kCandCap ? st.ncand : kCandCap;
        for (unsigned i = blockIdx.x * kSelThreads + tid; i < nc; i += gridDim.x * kSelThreads) {
            const u64 pat = a.cand[i];
            if ((pat & prefmask) == prefval) run_add(run, s_hist, (int)((pat >> shift) & (nbins - 1)), (unsigned)a.candw[i]);
        }
        flush_bins(run, s_hist, hist, nbins);
        return;
    }

    const bool gather = mode == MODE_GATHER;
    // a lane owns kRowBlock rows and, of every block of 4 CG columns, kColBlock columns: per channel it reads 4 + 4 values
    // from the LDS for 16 elements (one row per lane against broadcast columns made the LDS the limit of the pass)
    const int cg = tid % g.CG, rg = tid / g.CG;
    const int cbw = kColBlock * g.CG;
    const int lane = tid & (kWave - 1);
    const u64 lt = (1ull << lane) - 1ull;
    u64 pending = 0; // an upper bound of what the LDS bins and the lanes' counters hold
    const u64 item_weight = (u64)g.PB * g.QC * 2;

    for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
        const long long ch = item % g.nch;
        const long long ipb = item / g.nch;
        const int pb = (int)(ipb % g.npb);
        const int i = (int)(ipb / g.npb);
        const int rows_ok = a.TX - (pb * g.PB + kRowBlock * rg); // rows of this lane inside the path: r < rows_ok
        const long long col0 = ch * g.QC;

        if (pending + item_weight >= (1ull << 31)) {
            flush_bins(run, s_hist, hist, nbins);
            pending = 0;
        }
        pending += item_weight;
        if (gather) { // (the barrier makes the count uniform: every lane has left the last item, and none adds to the
                      // count again before the barriers of this item's staging)
            __syncthreads();
            if (s_nc >= kLdsCand / 2) flush_cands(a, s_cand, s_cw, &s_nc, &s_base);
        }

        double acc[kRowBlock][kColBlock];
        for (int cb = 0; cb < g.QC; cb += cbw) { // (wide paths: QC == cbw, one turn)
#pragma unroll
            for (int r = 0; r < kRowBlock; ++r)
#pragma unroll
                for (int u = 0; u < kColBlock; ++u) acc[r][u] = 0.0;
            for (int db = 0; db < g.nd; ++db) {
                const int k0 = db * g.DB;
                const int dcur = a.d - k0 < g.DB ? a.d - k0 : g.DB;
                if (g.nd > 1 || cb == 0) { // stage the two point sets: once per item, or once per channel block
                    __syncthreads();
                    for (int idx = tid; idx < dcur * g.PB; idx += kSelThreads) {
                        const int k = idx / g.PB, pp = idx - k * g.PB;
                        const int r = pb * g.PB + pp;
                        Xs[idx] = r < a.TX ? load_point(a.X, ((long long)i * a.TX + r) * a.d + k0 + k, a.dtype) : 0.0;
                    }
                    for (int c = tid; c < g.QC; c += kSelThreads) {
                        const long long col = col0 + c;
                        const long long o = col / a.TY;
                        int w = 0;
                        if (o < g.NO) {
                            const int q = (int)(col - o * a.TY);
                            // Y_IS_X: row i meets paths i, i + 1, .., i + A / 2 (mod A): every unordered pair once, counted
                            // twice -- except the pair with itself and, for even A, the opposite path, which both ends visit
                            const long long j = a.yx ? (i + o) % a.A : o;
                            w = a.yx ? ((o == 0 || 2 * o == a.A) ? 1 : 2) : 1;
                            const long long base = (j * a.TY + q) * a.d + k0;
                            for (int k = 0; k < dcur; ++k) Ys[(size_t)k * g.QC + c] = load_point(a.Y, base + k, a.dtype);
                        } else {
                            for (int k = 0; k < dcur; ++k) Ys[(size_t)k * g.QC + c] = 0.0;
                        }
                        if (db == 0) Ws[c] = w;
                    }
                    __syncthreads();
                }
                for (int k = 0; k < dcur; ++k) {
                    const d4 x = *reinterpret_cast<const d4 *>(Xs + k * g.PB + kRowBlock * rg);
                    const d4 y = *reinterpret_cast<const d4 *>(Ys + (size_t)k * g.QC + cb + kColBlock * cg);
#pragma unroll
                    for (int r = 0; r < kRowBlock; ++r)
#pragma unroll
                        for (int u = 0; u < kColBlock; ++u) {
                            const double df = x[r] - y[u];
                            acc[r][u] = __builtin_fma(df, df, acc[r][u]);
                        }
                }
            }
            const i4 wv = *reinterpret_cast<const i4 *>(Ws + cb + kColBlock * cg);
#pragma unroll
            for (int r = 0; r < kRowBlock; ++r)
#pragma unroll
                for (int u = 0; u < kColBlock; ++u) {
                    const unsigned w = (unsigned)wv[u];
                    const u64 pat = (u64)__double_as_longlong(acc[r][u]);
                    const bool m = r < rows_ok && w != 0 && (pat & prefmask) == prefval;
                    if (m) run_add(run, s_hist, (int)((pat >> shift) & (nbins - 1)), w);
                    if (gather) { // the bucket's elements: into the workgroup's LDS buffer, past its end straight to the
                                  // global one (dense buckets: one returning atomic per wave and turn)
                        bool over = false;
                        if (m) {
                            const unsigned slot = atomicAdd(&s_nc, 1u);
                            over = slot >= kLdsCand;
                            if (!over) {
                                s_cand[slot] = pat;
                                s_cw[slot] = (unsigned char)w;
                            }
                        }
                        const u64 mo = __ballot(over);
                        if (mo) {
                            const int leader = __ffsll((long long)mo) - 1;
                            unsigned base = 0;
                            if (lane == leader) base = atomicAdd(&a.st->ncand, (unsigned)__popcll(mo));
                            base = __shfl(base, leader);
                            const unsigned mine = base + (unsigned)__popcll(mo & lt);
                            if (over && mine < kCandCap) {
                                a.cand[mine] = pat;
                                a.candw[mine] = (unsigned char)w;
                            }
                        }
                    }
                }
        }
    }
    if (gather) flush_cands(a, s_cand, s_cw, &s_nc, &s_base);
    flush_bins(run, s_hist, hist, nbins);
}

// The workgroup between two passes: the digit whose bin holds the rank, the rank inside it, the bucket's size; what the next
// pass does; after the last digit the value.
__global__ __launch_bounds__(kPickThreads) void select_pick_kernel(SelState *stp, const u64 *hist_all, double *out, int t)
{
    __shared__ u64 s_scan[kPickThreads];
    const int tid = threadIdx.x;
    const int bits = digit_bits(t), nbins = 1 << bits;
    const u64 *hist = hist_all + (size_t)t * kBins;
    const SelState st = *stp;
    constexpr int per = kBins / kPickThreads;
    u64 mine[per], sum = 0;
#pragma unroll
    for (int u = 0; u < per; ++u) {
        const int b = tid * per + u;
        mine[u] = b < nbins ? hist[b] : 0;
        sum += mine[u];
    }
    s_scan[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kPickThreads; off <<= 1) {
        const u64 v = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    const u64 incl = s_scan[tid];
    u64 below = incl - sum;
    if (below <= st.rank && st.rank < incl) { // one thread: the bins of all others lie below or above the rank
        int u_sel = 0;
        bool found = false;
#pragma unroll
        for (int u = 0; u < per; ++u) {
            if (!found) {
                if (st.rank < below + mine[u] || u == per - 1) {
                    u_sel = u;
                    found = true;
                } else {
                    below += mine[u];
                }
            }
        }
        u64 cnt = 0;
#pragma unroll
        for (int u = 0; u < per; ++u) cnt = u == u_sel ? mine[u] : cnt;
        const int b = tid * per + u_sel;
        SelState n = st;
        n.prefix = (st.prefix << bits) | (u64)b;
        n.rank = st.rank - below;
        n.count = cnt;
        if (st.mode != MODE_CAND) n.passes = st.passes + 1;
        // gather the bucket next if the buffer holds it -- and, above kDenseCap, only if it is a small part of the elements:
        // appending most of what a pass computes costs more than counting one more digit first
        if (st.mode == MODE_COUNT && n.count <= kCandCap && (n.count <= kDenseCap || n.count * 64 <= st.total))
            n.mode = MODE_GATHER;
        if (st.mode == MODE_GATHER) n.mode = MODE_CAND;
        n.ncand = *(volatile unsigned *)&stp->ncand;
        *stp = n;
        if (t == kSelPasses - 1) *out = __longlong_as_double((long long)n.prefix);
    }
}

// the entry point's own clearing of its counters, and the first state
__global__ __launch_bounds__(kPickThreads) void select_init_kernel(SelState *stp, u64 *hist, double *out, u64 rank, u64 n)
{
    for (int b = threadIdx.x; b < kSelPasses * kBins; b += kPickThreads) hist[b] = 0;
    if (threadIdx.x == 0) {
        SelState s;
        s.prefix = 0;
        s.rank = rank;
        s.count = n;
        s.mode = n <= kDenseCap ? MODE_GATHER : MODE_COUNT;
        s.passes = 0;
        s.ncand = 0;
        s.pad = 0;
        s.total = n;
        *stp = s;
        *out = 0.0; // (overwritten by the last pick; a defined value whatever the input)
    }
}
} // namespace

size_t select_workspace_bytes() { return kSelWsBytes; }

int select_launch(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, unsigned flags,
                  unsigned long long rank, unsigned long long n, double *out, void *ws, size_t ws_bytes, hipStream_t stream)
{
    if (!ws || ws_bytes < kSelWsBytes) {
        set_error("sqdist_select: workspace of %zu B, required %zu B", ws ? ws_bytes : (size_t)0, kSelWsBytes);
        return SIGSVGD_E_WORKSPACE;
    }
    unsigned char *base = reinterpret_cast<unsigned char *>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    SelArgs a;
    a.X = X;
    a.Y = Y;
    a.A = A, a.B = B, a.TX = TX, a.TY = TY, a.d = d, a.dtype = dtype;
    a.yx = (flags & SIGSVGD_FLAG_Y_IS_X) ? 1 : 0;
    a.g = select_geometry(A, B, TX, TY, d, a.yx != 0);
    a.st = reinterpret_cast<SelState *>(base);
    a.hist = reinterpret_cast<u64 *>(base + kStateBytes);
    a.cand = reinterpret_cast<u64 *>(base + kStateBytes + kHistBytes);
    a.candw = reinterpret_cast<unsigned char *>(a.cand + kCandCap);
    a.out = out;
    const size_t lds = kLdsFixed + ((size_t)a.g.DB * (a.g.PB + a.g.QC)) * sizeof(double) + (size_t)a.g.QC * sizeof(int);
    select_init_kernel<<<1, kPickThreads, 0, stream>>>(a.st, a.hist, out, rank, n);
    for (int t = 0; t < kSelPasses; ++t) {
        a.pass = t;
        select_pass_kernel<<<a.g.grid, kSelThreads, lds, stream>>>(a);
        select_pick_kernel<<<1, kPickThreads, 0, stream>>>(a.st, a.hist, out, t);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sqdist_select launch");
    return SIGSVGD_OK;
}

} // namespace sigsvgd
