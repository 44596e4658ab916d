// lt_tallystats.hip -- the statistical error of the voxel tally from batch moments (lt_stats_*).  Beside the grid a ctx keeps
// `prev` (the grid as it stood when the last batch was closed, in the tally's type) and `m2` (f64: the sum over the closed
// batches of the squared batch contribution).  Three streaming passes, all HBM-bound, none with a global atomic:
//   k_stats_fold     closes a batch: d = grid - prev, m2 += d * d, prev = grid.  A 16-byte group whose grid and prev bits are
//                    equal (away from the beam: almost every one) writes nothing and does not read m2
//   k_stats_relerr   R per voxel (rel_err below) as f64
//   k_stats_classes  every voxel classed by R against ascending edges; voxels and weight per class in per-workgroup LDS
//                    bins, flushed once per workgroup into partial sums that k_sum_finish (lt_tallysum.hip) adds in a fixed order
// Built with -ffp-contract=off: m2 + d * d is ONE rounded multiply and ONE rounded add, and every line of rel_err a single
// IEEE double operation, so that a NumPy restatement gives the same bits.
#include <hip/hip_runtime.h>

#include "lt_tally.hpp"

#pragma clang fp contract(off)

namespace ltk {
namespace {

// 16 bytes of the grid: compared as two words, used as 16 / sizeof(T) elements
template <typename T> union alignas(16) Bits16 { u64 q[2]; T v[16 / sizeof(T)]; };
template <int K> struct alignas(16) F64xK { double v[K]; };     // the m2 (or R) of one such group

// A workgroup takes chunks of kFoldDepth x 256 adjacent 16-byte groups (16 KiB of the grid, as much of prev, twice that of m2 in
// f32): lane l loads groups l, l + 256, ... of the chunk from every stream before it looks at any -- 32 KiB in flight per
// workgroup in the fold.  Chunks of one piece measured 0.75 of the time of the same loads strided over the whole launch (512^3
// grid, every voxel changed: 1100 -> 895 us): a chunk's reads and writes stay within a few DRAM pages.
constexpr uint32_t kFoldDepth = 4;
constexpr uint32_t kCopies = 32;         // k_stats_classes: copies of every LDS bin; a lane adds to copy (lane & 31)
constexpr uint32_t kMaxClasses = kMaxStatEdges + 2;

__device__ __forceinline__ double batch_diff(u64 g, u64 p) { return (double)(g - p) * (1.0 / LT_FX_SCALE); }
__device__ __forceinline__ double batch_diff(double g, double p) { return g - p; }
__device__ __forceinline__ double batch_diff(float g, float p) { return (double)g - (double)p; }

// Relative standard error of the mean over N equal batches (lt.h): S1 the voxel's weight, m2 its sum of squared batch
// contributions.  One IEEE operation per line; both readouts go through here, so a voxel's class is the class of its R.
__device__ __forceinline__ double rel_err(double N, double m2, double S1)
{
    if (S1 == 0.0) return __builtin_nan("");
    const double a = N * m2;
    const double b = S1 * S1;
    const double q = a / b;
    double v = q - 1.0;
    if (v < 0.0) v = 0.0;
    const double w = v / (N - 1.0);
    return sqrt(w);
}

template <typename T>
__device__ __forceinline__ void fold_one(T g, T& p, double& m)
{
    const double d = batch_diff(g, p);
    const double dd = d * d;
    m = m + dd;
    p = g;
}

// Workgroup b owns the chunks b, b + gridDim, ... and lane l the groups l, l + 256, ... of each: which lane folds which voxel
// depends on the grid's size alone.  A changed group's m2 is read only once the group is known to have changed; asking for the
// m2 of all four groups up front cost 22 registers and ran 15 % slower.  The last n % kV voxels go one by one.
template <typename T>
__global__ void __launch_bounds__(256) k_stats_fold(const T* __restrict__ grid, T* __restrict__ prev, double* __restrict__ m2, size_t n)
{
    constexpr int kV = 16 / sizeof(T);
    const size_t nvec = n / kV, stride = (size_t)gridDim.x * 256;
    const Bits16<T>* pg = reinterpret_cast<const Bits16<T>*>(grid);
    Bits16<T>* pp = reinterpret_cast<Bits16<T>*>(prev);
    F64xK<kV>* pm = reinterpret_cast<F64xK<kV>*>(m2);
    for (size_t i0 = (size_t)blockIdx.x * (256 * kFoldDepth) + threadIdx.x; i0 < nvec; i0 += stride * kFoldDepth) {
        Bits16<T> g[kFoldDepth], p[kFoldDepth];
#pragma unroll
        for (uint32_t u = 0; u < kFoldDepth; u++) {
            const size_t i = i0 + u * 256;
            if (i < nvec) { g[u] = pg[i]; p[u] = pp[i]; }
            else { g[u].q[0] = g[u].q[1] = p[u].q[0] = p[u].q[1] = 0; }
        }
#pragma unroll
        for (uint32_t u = 0; u < kFoldDepth; u++) {
            if (g[u].q[0] == p[u].q[0] && g[u].q[1] == p[u].q[1]) continue;      // (a group past the end: both zero)
            const size_t i = i0 + u * 256;
            F64xK<kV> m = pm[i];
#pragma unroll
            for (int k = 0; k < kV; k++) fold_one(g[u].v[k], p[u].v[k], m.v[k]);
            pm[i] = m;
            pp[i] = g[u];
        }
    }
    const size_t t = nvec * kV + threadIdx.x;
    if (blockIdx.x == 0 && t < n) {
        T p = prev[t];
        double m = m2[t];
        fold_one(grid[t], p, m);
        m2[t] = m; prev[t] = p;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_stats_relerr(const T* __restrict__ prev, const double* __restrict__ m2, size_t n, double N,
                                                       double* __restrict__ out)
{
    constexpr int kV = 16 / sizeof(T);
    const size_t nvec = n / kV, stride = (size_t)gridDim.x * 256;
    const Bits16<T>* pp = reinterpret_cast<const Bits16<T>*>(prev);
    const F64xK<kV>* pm = reinterpret_cast<const F64xK<kV>*>(m2);
    F64xK<kV>* po = reinterpret_cast<F64xK<kV>*>(out);
#pragma unroll 4
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        const Bits16<T> p = pp[i];
        const F64xK<kV> m = pm[i];
        F64xK<kV> r;
#pragma unroll
        for (int k = 0; k < kV; k++) r.v[k] = rel_err(N, m.v[k], as_weight(p.v[k]));
        po[i] = r;
    }
    const size_t t = nvec * kV + threadIdx.x;
    if (blockIdx.x == 0 && t < n) out[t] = rel_err(N, m2[t], as_weight(prev[t]));
}

struct StatEdges { double e[kMaxStatEdges + 1]; };     // ascending, padded with NaN (never <= R) to 64

// Class of a voxel = number of edges <= R (0 .. n_edges), found by bisection of the edges in LDS; class n_cls - 1 collects the
// voxels with S1 == 0 (no estimate).  part_cnt / part_w [workgroup][n_cls]: voxels and weight (u64 fixed point: the integer sum)
// per class.  Most of a traced grid is empty and most of the rest falls in one or two classes, so one LDS bin per class would
// serialise every wave on one address: empty voxels are counted in a register (a group that is all zero does not read m2 at
// all), and every class has kCopies bins side by side -- a lane adds to copy (lane & 31), the flush adds the copies in order.
template <typename T>
__global__ void __launch_bounds__(256) k_stats_classes(const T* __restrict__ prev, const double* __restrict__ m2, size_t n, double N,
                                                        StatEdges E, uint32_t n_cls, u64* __restrict__ part_cnt,
                                                        typename AccOf<T>::type* __restrict__ part_w)
{
    typedef typename AccOf<T>::type A;
    constexpr int kV = 16 / sizeof(T);
    __shared__ double s_edge[kMaxStatEdges + 1];
    __shared__ u64 s_cnt[kMaxClasses * kCopies];
    __shared__ A s_w[kMaxClasses * kCopies];
    if (threadIdx.x <= kMaxStatEdges) s_edge[threadIdx.x] = E.e[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < n_cls * kCopies; i += 256) { s_cnt[i] = 0; s_w[i] = 0; }
    __syncthreads();
    const uint32_t copy = threadIdx.x & (kCopies - 1);
    u64 n_empty = 0;
    auto book = [&](T s1, double m) {
        const double R = rel_err(N, m, as_weight(s1));
        uint32_t c = 0;
#pragma unroll
        for (uint32_t step = (kMaxStatEdges + 1) / 2; step; step >>= 1)
            if (s_edge[c + step - 1] <= R) c += step;
        lds_add(&s_cnt[c * kCopies + copy], (u64)1);
        lds_add(&s_w[c * kCopies + copy], (A)s1);
    };
    const size_t nvec = n / kV, stride = (size_t)gridDim.x * 256;
    const Bits16<T>* pp = reinterpret_cast<const Bits16<T>*>(prev);
    const F64xK<kV>* pm = reinterpret_cast<const F64xK<kV>*>(m2);
    for (size_t i0 = (size_t)blockIdx.x * (256 * kFoldDepth) + threadIdx.x; i0 < nvec; i0 += stride * kFoldDepth) {
        Bits16<T> p[kFoldDepth];
#pragma unroll
        for (uint32_t u = 0; u < kFoldDepth; u++) {
            const size_t i = i0 + u * 256;
            if (i < nvec) p[u] = pp[i];
            else p[u].q[0] = p[u].q[1] = 0;
        }
        bool filled[kFoldDepth];
        F64xK<kV> m[kFoldDepth];
#pragma unroll
        for (uint32_t u = 0; u < kFoldDepth; u++) {      // (a group past the end is zero: no load)
            filled[u] = (p[u].q[0] | p[u].q[1]) != 0;
            if (filled[u]) m[u] = pm[i0 + u * 256];
        }
#pragma unroll
        for (uint32_t u = 0; u < kFoldDepth; u++) {
            if (i0 + u * 256 >= nvec) continue;
            if (!filled[u]) { n_empty += kV; continue; }
#pragma unroll
            for (int k = 0; k < kV; k++) {
                if (p[u].v[k] == (T)0) n_empty++;
                else book(p[u].v[k], m[u].v[k]);
            }
        }
    }
    const size_t t = nvec * kV + threadIdx.x;
    if (blockIdx.x == 0 && t < n) {
        const T s1 = prev[t];
        if (s1 == (T)0) n_empty++;
        else book(s1, m2[t]);
    }
    if (n_empty) lds_add(&s_cnt[(n_cls - 1) * kCopies + copy], n_empty);
    __syncthreads();
    if (threadIdx.x < n_cls) {
        u64 cnt = 0;
        A w = 0;
        for (uint32_t k = 0; k < kCopies; k++) { cnt += s_cnt[threadIdx.x * kCopies + k]; w += s_w[threadIdx.x * kCopies + k]; }
        part_cnt[(size_t)blockIdx.x * n_cls + threadIdx.x] = cnt;
        part_w[(size_t)blockIdx.x * n_cls + threadIdx.x] = w;
    }
}

// grid of a pass whose lanes each take `depth` 16-byte groups of voxels per round
uint32_t stats_blocks(size_t n_vox, size_t elem_bytes, uint32_t depth) { return blocks_for(n_vox, (size_t)256 * depth * (16 / elem_bytes)); }

}  // namespace

hipError_t launch_stats_fold(const void* grid, void* prev, double* m2, int tally, size_t n, hipStream_t s)
{
    with_tally_type(tally, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_stats_fold<T>, dim3(stats_blocks(n, sizeof(T), kFoldDepth)), dim3(256), 0, s, (const T*)grid, (T*)prev, m2, n);
    });
    return hipGetLastError();
}

hipError_t launch_stats_relerr(const void* prev, const double* m2, int tally, size_t n, uint64_t batches, double* out, hipStream_t s)
{
    const double N = (double)batches;
    with_tally_type(tally, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_stats_relerr<T>, dim3(stats_blocks(n, sizeof(T), 4)), dim3(256), 0, s, (const T*)prev, m2, n, N, out);
    });
    return hipGetLastError();
}

uint32_t stats_summary_parts(size_t n_vox, int tally) { return stats_blocks(n_vox, tally_elem_bytes(tally), kFoldDepth); }

hipError_t launch_stats_summary(const void* prev, const double* m2, int tally, size_t n, uint64_t batches, const double* edges,
                                int n_edges, void* partials, double* out, hipStream_t s)
{
    u64* raw = (u64*)out;
    const double N = (double)batches;
    const uint32_t n_cls = (uint32_t)n_edges + 2, P = stats_summary_parts(n, tally);
    StatEdges E;
    for (int i = 0; i <= kMaxStatEdges; i++) E.e[i] = i < n_edges ? edges[i] : __builtin_nan("");
    u64* part_cnt = (u64*)partials;
    void* part_w = part_cnt + (size_t)P * n_cls;
    with_tally_type(tally, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_stats_classes<T>, dim3(P), dim3(256), 0, s, (const T*)prev, m2, n, N, E, n_cls, part_cnt, (typename AccOf<T>::type*)part_w);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // out, n_cls 8-byte words each: weight (f64), raw weight (u64 fixed point only), voxels (u64), unused (the voxels as if they were fixed point)
    e = launch_tally_sum_finish(part_cnt, 1, P, n_cls, out + 3 * (size_t)n_cls, raw + 2 * (size_t)n_cls, s);
    if (e != hipSuccess) return e;
    return launch_tally_sum_finish(part_w, tally == LT_TALLY_U64FX, P, n_cls, out, tally == LT_TALLY_U64FX ? raw + n_cls : nullptr, s);
}

}  // namespace ltk
