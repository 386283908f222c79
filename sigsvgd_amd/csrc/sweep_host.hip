// The launch tail every fp32-sweep family shares (gram_fast, gram_quad, gram_dyad, gram_band; pair_bands and capi size grids
// with device_cu_count): the compute-unit count, the tile map and gradient geometry, the fixed-order gradient reduction
// kernel and its launch, ws_base and finish_launch.  Declared in sig_common.h; no sweep statements, so no EXEC debug getter.
#include <atomic>

#include "sig_common.h"

namespace sigsvgd {

// ---- fixed-order reduction of the gradient partials -----------------------------------------------------------------
// One thread per output element (i, t, c).  Row side: the segments of row i's tile, one per workgroup whose item range
// met the tile, in workgroup order.  Column side (symmetric launches): the items (tile, column i) of every owned tile
// whose first row is <= i, in tile order.  fp64 sums; the order is a function of the launch geometry only, so two
// launches on the same input give the same bits.
struct GradReduceArgs {
    const double *rseg;
    const float *cslab;
    void *out; // [A][T*d]: the I/O type, or fp64 for the sharded partial solve
    int out64, A, B, TD, NW, sym, grid;
    TileMap tm;
    long long nitems;
};
// grid (ceil(T*d / (64 V)), A), 4 wavefronts: a workgroup serves 64 V elements of one row i, so everything that depends on
// the row only -- its tile, the tile's item range, the workgroups that met it, the slab row of column i in every owned
// tile -- is wave-uniform SCALAR arithmetic, and the slab rows are walked incrementally (a tile's items follow the
// previous tile's: one 64-bit add per tile; evaluating the closed forms per load made the kernel scalar-bound: 27.5 us
// at N=128, T=32, d=7 -- a third of the iteration -- and 100-137 us per C4 launch whatever the thread layout).  An
// element is a sum over up to N / NW slab rows (column side) and one segment per workgroup that met the row's tile (row
// side: a handful in large launches, up to ~100 in small ones, where a workgroup owns one or two columns): wavefront w
// adds the w-th quarter of each list and the four partial sums are joined in wavefront order.
// V: elements per thread.  V = 1 takes any T*d (4-byte loads, sixteen in flight).  V = 4 -- T*d a multiple of 4 and every
// base aligned to 4 of its elements, grad_reduce_launch decides -- gives a thread 4 consecutive elements of the block: one 16-byte load
// per slab row (two per fp64 segment), eight slab rows in flight, a quarter of the scalar work per byte.  Each element
// sees the same fp64 additions in the same order under either V: same bits.
constexpr int RED_W = 4; // (8 wavefronts of half the share each: 78 us instead of 66 at C4)
template <int V> struct RedVec;
template <> struct RedVec<1> { using F = float; using D = double; };
template <> struct RedVec<4> {
    using F = __attribute__((ext_vector_type(4))) float;
    using D = __attribute__((ext_vector_type(4))) double;
};
template <int V> __device__ __forceinline__ double red_elem(const typename RedVec<V>::D &v, int k) { return v[k]; }
template <> __device__ __forceinline__ double red_elem<1>(const double &v, int) { return v; }
template <int V> __device__ __forceinline__ float red_elem(const typename RedVec<V>::F &v, int k) { return v[k]; }
template <> __device__ __forceinline__ float red_elem<1>(const float &v, int) { return v; }

template <int V>
__global__ __launch_bounds__(RED_W * 64) void grad_reduce_kernel(GradReduceArgs r)
{
    using FV = typename RedVec<V>::F;
    using DV = typename RedVec<V>::D;
    constexpr int UR = (V == 1) ? 8 : 4, UC = (V == 1) ? 16 : 8; // segments / slab rows in flight per thread
    __shared__ double part[RED_W][V][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e = (blockIdx.x * 64 + lane) * V;
    const int i = r.A - 1 - (int)blockIdx.y; // rows with the longest column sums first (66 -> 60 us at C4)
    const bool live = e < r.TD;              // (V = 4: T*d is a multiple of 4, a live thread has all four)
    double s[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s[k] = 0.0;
    if (live) {
        // row side: the segments of the row's tile, one per workgroup whose item range met it
        const int ti = i / r.NW, wv = i % r.NW;
        const int kqr = r.tm.kq_of_tile(ti);
        if (kqr >= 0) {
            const long long S0 = r.tm.start(kqr, r.B, r.NW, r.sym);
            const long long cn = r.sym ? r.B - ti * r.NW : r.B;
            // workgroup w works on the items [nitems*w/grid, nitems*(w+1)/grid): the one holding item x is
            const int wlo = (int)(((S0 + 1) * r.grid - 1) / r.nitems), whi = (int)(((S0 + cn) * r.grid - 1) / r.nitems);
            const int nseg = whi - wlo + 1, per = (nseg + RED_W - 1) / RED_W;
            const int w0 = wlo + wave * per, w1 = min(whi + 1, w0 + per);
            const size_t sstride = (size_t)r.NW * r.TD;
            const double *base = r.rseg + ((size_t)kqr * r.NW + wv) * r.TD + e + (size_t)w0 * sstride;
            for (int w = w0; w < w1; w += UR, base += UR * sstride) {
                DV v[UR];
#pragma unroll
                for (int u = 0; u < UR; ++u) v[u] = (w + u < w1) ? *reinterpret_cast<const DV *>(base + u * sstride) : DV(0.0);
#pragma unroll
                for (int u = 0; u < UR; ++u)
#pragma unroll
                    for (int k = 0; k < V; ++k) s[k] += red_elem<V>(v[u], k);
            }
        }
        // column side: the items (owned tile, column i) of the tiles whose first row is <= i, in the order of the enumeration
        if (r.sym) {
            const int per = (r.tm.owned + RED_W - 1) / RED_W;
            const int k0 = wave * per, k1 = min(r.tm.owned, k0 + per);
            // slab row of item (tile kq, column i) = start(kq) + i - tile * NW; start(kq + 1) = start(kq) + B - tile * NW
            const float *row = r.cslab + (size_t)(k0 < k1 ? r.tm.start(k0, r.B, r.NW, 1) : 0) * r.TD + e;
            for (int kq = k0; kq < k1; kq += UC) {
                FV v[UC];
#pragma unroll
                for (int u = 0; u < UC; ++u) {
                    const bool have = kq + u < k1;
                    const int first = have ? r.tm.tile_of(kq + u) * r.NW : r.B; // first row of the tile
                    const bool in = first <= i;
                    v[u] = in ? *reinterpret_cast<const FV *>(row + (size_t)(in ? i - first : 0) * r.TD) : FV(0.f);
                    row += have ? (size_t)(r.B - first) * r.TD : 0;
                }
#pragma unroll
                for (int u = 0; u < UC; ++u)
#pragma unroll
                    for (int k = 0; k < V; ++k) s[k] += (double)red_elem<V>(v[u], k);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) part[wave][k][lane] = s[k];
    __syncthreads();
    if (wave != 0 || !live) return;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        s[k] = part[0][k][lane];
#pragma unroll
        for (int w = 1; w < RED_W; ++w) s[k] += part[w][k][lane];
    }
    const size_t idx = (size_t)i * r.TD + e;
    if (r.out64) {
        DV o;
        if constexpr (V == 1) o = s[0];
        else
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = s[k];
        *reinterpret_cast<DV *>(static_cast<double *>(r.out) + idx) = o;
    } else {
        FV o;
        if constexpr (V == 1) o = (float)s[0];
        else
#pragma unroll
            for (int k = 0; k < V; ++k) o[k] = (float)s[k];
        *reinterpret_cast<FV *>(static_cast<float *>(r.out) + idx) = o;
    }
}

// ---- host side ---------------------------------------------------------------------------------
// compute units of the current device (256 on MI355X); the persistent grids are sized from it
int device_cu_count()
{
    static std::atomic<int> cache[64]; // per device ordinal (zero-initialised: not queried yet)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < 64) {
        const int c = cache[dev].load(std::memory_order_relaxed);
        if (c > 0) return c;
    }
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    if (dev >= 0 && dev < 64) cache[dev].store(v, std::memory_order_relaxed);
    return v;
}

TileMap make_tilemap(int ntile, int off, int stride, bool fold)
{
    TileMap t;
    t.off = off; t.stride = stride; t.ntile = ntile; t.fold = fold ? 1 : 0;
    auto count_upto = [&](int hi) { return hi >= off ? (hi - off) / stride + 1 : 0; }; // tiles off + k*stride <= hi
    if (!fold) {
        t.m0 = t.owned = count_upto(ntile - 1);
    } else {
        t.m0 = count_upto((ntile - 1) / 2);                        // p <= ntile-1-p
        t.owned = t.m0 + (ntile >= 2 ? count_upto((ntile - 2) / 2) : 0); // mirror images of the p < ntile-1-p
    }
    return t;
}

// Geometry of a gradient launch of the register-resident / quadrant kernels: NW rows per tile, `resident` workgroups on
// the chip; the kernels and grad_reduce_kernel derive items, ranges and segments from the same numbers.
GradGeom grad_geometry(int A, int B, int TD, bool sym, int off, int stride, bool fold, int NW, long long resident)
{
    GradGeom g;
    g.NW = NW;
    g.tm = make_tilemap((A + NW - 1) / NW, off, stride, fold);
    g.nitems = g.tm.start(g.tm.owned, B, NW, sym ? 1 : 0);
    g.grid = (int)(g.nitems < resident ? g.nitems : resident);
    g.rseg_bytes = (((size_t)(g.tm.owned + g.grid) * NW * TD * sizeof(double)) + 255) & ~(size_t)255;
    g.cslab_bytes = sym ? (((size_t)g.nitems * TD * sizeof(float)) + 255) & ~(size_t)255 : 0;
    return g;
}

int grad_reduce_launch(const GradGeom &g, const double *rseg, const float *cslab, void *out, int out64, int A, int B, int TD,
                       bool sym, hipStream_t stream)
{
    GradReduceArgs r;
    r.rseg = rseg; r.cslab = cslab; r.out = out; r.out64 = out64;
    r.A = A; r.B = B; r.TD = TD; r.NW = g.NW; r.tm = g.tm;
    r.sym = sym ? 1 : 0; r.grid = g.grid > 0 ? g.grid : 1; r.nitems = g.nitems > 0 ? g.nitems : 1;
    if (A > 65535) {
        set_error("gradient reduction: %d rows exceed the grid limit", A);
        return SIGSVGD_E_UNSUPPORTED;
    }
    // four elements per thread where every 4-element access is aligned: T*d a multiple of 4 (the rows of the slab, of the
    // segments and of the output then start on multiples of 4 elements) and bases aligned to 4 elements of their type
    // (16 B of floats, 32 B of doubles; the workspace areas are 256-B aligned); any other shape one per thread
    auto aligned = [](const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; };
    const bool vec4 = TD % 4 == 0 && aligned(rseg, 32) && aligned(cslab, 16) && aligned(out, out64 ? 32 : 16);
    if (vec4)
        hipLaunchKernelGGL(grad_reduce_kernel<4>, dim3((unsigned)((TD + 255) / 256), (unsigned)A), dim3(RED_W * 64), 0, stream, r);
    else
        hipLaunchKernelGGL(grad_reduce_kernel<1>, dim3((unsigned)((TD + 63) / 64), (unsigned)A), dim3(RED_W * 64), 0, stream, r);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch grad_reduce_kernel");
    return SIGSVGD_OK;
}

int ws_base(const GramProblem &p, const WsPlan &w, const char *family, unsigned char *&base)
{
    if (w.end && (!p.ws || p.ws_bytes < w.total())) {
        set_error("%s: workspace %zu B < required %zu B", family, p.ws_bytes, w.total());
        return SIGSVGD_E_WORKSPACE;
    }
    base = reinterpret_cast<unsigned char *>((reinterpret_cast<uintptr_t>(p.ws) + 255) & ~(uintptr_t)255);
    return SIGSVGD_OK;
}

int finish_launch(const GramProblem &p, const WsPlan &w, unsigned char *base, bool sym, const TileMap &tm, int tile_rows,
                  void *out, int out64)
{
    if (w.kflag.bytes) { // exact fp64 pass of the coverage kernel over the flagged pairs (a few microseconds when there are none)
        const int rc = generic_repair_launch(p, base + w.kflag.off, sym, tm, tile_rows);
        if (rc) return rc;
    }
    if (!out) return SIGSVGD_OK;
    return grad_reduce_launch(w.g, ws_at<double>(base, w.rseg), ws_at<float>(base, w.cslab), out, out64, p.A, p.B, p.T * p.d,
                              sym, p.stream);
}

} // namespace sigsvgd
