// lt_tallysum.hip -- every whole-grid pass over the voxel tally: the read-out as f64 (k_grid_to_f64), grid += grid
// (k_grid_add), and the sums taken on the device (lt_tally_sum_axes, lt_tally_sum_columns): depth profiles, projections,
// r-z maps.  The sums are pure streaming reductions: every voxel is read once, and nothing but partial sums (some MiB where
// the output is small and the summed axis long; never a second grid) and the output is written.
//
// Everything is summed in an accumulator type A: u64 for the fixed-point tally (integer sums: exact, any order), f64 for the
// f32 and f64 tallies (every voxel widened first).  Three kernels write PARTIAL sums, laid out [part][output], and
// k_sum_finish adds the parts of every output in a fixed order and converts:
//   k_sum_rows    outputs whose voxels are contiguous in memory (x is summed): one wave per (row, part of the row)
//   k_sum_cols    outputs strided in memory (x is kept): one lane per 16 bytes of columns, looping over a part of the rows
//   k_sum_bins    per z, the (y, x) columns binned by a table: LDS bins per workgroup, flushed once per (z, part of the plane)
// Which wave sums what, and in which order, depends on the grid's shape alone (never on the device or on timing), so the
// axis sums of a float tally are the same bits on every call.  k_sum_bins adds to its LDS bins with atomics: exact for the
// integer tally, order-dependent in the last bits for float tallies.
#include <hip/hip_runtime.h>

#include "lt_tally.hpp"

namespace ltk {
namespace {

template <typename T> struct alignas(sizeof(T)) VecEl { T v[16 / sizeof(T)]; };    // 16 bytes at element alignment (rows of odd length)

constexpr uint32_t kRowPart = 4096;       // k_sum_rows: elements of a row that one wave sums
constexpr uint32_t kWaveTarget = 8192;    // k_sum_cols: rows are split until this many waves have work ...
constexpr uint32_t kMinRows = 8;          //             ... or a part is down to this many rows
constexpr uint32_t kBinPart = 2048;       // k_sum_bins: least voxels of a plane per workgroup (or four per bin, if that is more)
constexpr uint32_t kBinGroups = 2048;     //             planes are split until this many workgroups have work
constexpr uint32_t kFinishSerial = 32;    // k_sum_finish: up to this many parts one lane adds them, beyond it a wave does

template <typename A>
__device__ __forceinline__ A wave_sum(A v)      // fixed tree; lane 0 holds the total
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// in: n_rows rows of L contiguous elements.  partial[p * n_rows + r] = sum of part p (kRowPart elements) of row r.
// A part starts wherever its row does, so a wave takes up to 16 / sizeof(T) - 1 single elements at either end and 16-byte
// vectors in between (the grid is hipMalloc'ed: element index = a multiple of the vector width <=> 16-byte aligned).
template <typename T>
__global__ void __launch_bounds__(256) k_sum_rows(const T* __restrict__ in, size_t n_rows, size_t L, uint32_t P,
                                                   typename AccOf<T>::type* __restrict__ partial)
{
    typedef typename AccOf<T>::type A;
    constexpr size_t kV = 16 / sizeof(T);
    const uint32_t lane = threadIdx.x & 63u;
    const size_t n_items = n_rows * P, n_waves = (size_t)gridDim.x * 4;
    for (size_t it = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < n_items; it += n_waves) {
        const size_t r = it / P, p = it - r * P;
        const size_t a = r * L + p * kRowPart;
        const size_t b = (p + 1) * (size_t)kRowPart < L ? a + kRowPart : r * L + L;
        size_t va = (a + kV - 1) / kV * kV;
        if (va > b) va = b;
        const size_t nvec = (b - va) / kV, vb = va + nvec * kV;
        A acc = 0;
        if (a + lane < va) acc += (A)in[a + lane];
        const Vec16<T>* pv = reinterpret_cast<const Vec16<T>*>(in + va);
#pragma unroll 4
        for (size_t i = lane; i < nvec; i += 64) {
            const Vec16<T> v = pv[i];
#pragma unroll
            for (size_t k = 0; k < kV; k++) acc += (A)v.v[k];
        }
        if (vb + lane < b) acc += (A)in[vb + lane];
        acc = wave_sum(acc);
        if (lane == 0) partial[p * n_rows + r] = acc;
    }
}

// in: B matrices of R rows x Cn columns, contiguous.  partial[(rp * B + b) * Cn + c] = sum over part rp of the rows of
// in[b][r][c].  A wave owns 64 x (16 / sizeof(T)) adjacent columns, a lane 16 bytes of them; rows start at any element (Cn
// may be odd), so the loads are 16 bytes wide at element alignment.  The last Cn % (16 / sizeof(T)) columns go one by one.
template <typename T>
__global__ void __launch_bounds__(256) k_sum_cols(const T* __restrict__ in, size_t B, size_t R, size_t Cn, uint32_t RP,
                                                   size_t rows_per_part, typename AccOf<T>::type* __restrict__ partial)
{
    typedef typename AccOf<T>::type A;
    constexpr size_t kV = 16 / sizeof(T);
    const uint32_t lane = threadIdx.x & 63u;
    const size_t n_cb = (Cn + 64 * kV - 1) / (64 * kV);
    const size_t n_items = B * RP * n_cb, n_waves = (size_t)gridDim.x * 4;
    for (size_t it = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < n_items; it += n_waves) {
        const size_t cb = it % n_cb, q = it / n_cb, rp = q % RP, b = q / RP;     // neighbouring waves read neighbouring kilobytes
        const size_t c0 = (cb * 64 + lane) * kV;
        if (c0 >= Cn) continue;
        const size_t r0 = rp * rows_per_part, r1 = r0 + rows_per_part < R ? r0 + rows_per_part : R;
        const T* src = in + (b * R + r0) * Cn + c0;
        A* dst = partial + (rp * B + b) * Cn + c0;
        if (c0 + kV <= Cn) {
            A acc[kV];
#pragma unroll
            for (size_t k = 0; k < kV; k++) acc[k] = 0;
#pragma unroll 4
            for (size_t r = r0; r < r1; r++, src += Cn) {
                const VecEl<T> v = *reinterpret_cast<const VecEl<T>*>(src);
#pragma unroll
                for (size_t k = 0; k < kV; k++) acc[k] += (A)v.v[k];
            }
#pragma unroll
            for (size_t k = 0; k < kV; k++) dst[k] = acc[k];
        } else {
            for (size_t k = 0; c0 + k < Cn; k++) {
                A acc = 0;
                for (size_t r = 0; r < r1 - r0; r++) acc += (A)src[r * Cn + k];
                dst[k] = acc;
            }
        }
    }
}

// grid: nz planes of `plane` voxels; bins[plane]: the bin of every (y, x) column, -1 = left out (the host has checked that
// every entry is in -1 .. n_bins - 1).  partial[(pp * nz + z) * n_bins + bin] = what part pp of plane z adds to the bin.
// One workgroup per (z, part): bins in LDS (8 bytes each: <= 32 KiB), zeroed, added to with LDS atomics, written out once.
// Voxels that hold nothing (most of a grid, away from the beam) are skipped.
template <typename T>
__global__ void __launch_bounds__(256) k_sum_bins(const T* __restrict__ grid, const int32_t* __restrict__ bins, size_t plane,
                                                   uint32_t nz, uint32_t PP, size_t part_len, uint32_t n_bins,
                                                   typename AccOf<T>::type* __restrict__ partial)
{
    typedef typename AccOf<T>::type A;
    constexpr size_t kV = 16 / sizeof(T);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    A* lds = reinterpret_cast<A*>(lds_raw);
    const size_t n_items = (size_t)nz * PP;
    for (size_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const size_t z = it / PP, pp = it - z * PP;
        for (uint32_t i = threadIdx.x; i < n_bins; i += 256) lds[i] = 0;
        __syncthreads();
        const size_t a = pp * part_len, b = a + part_len < plane ? a + part_len : plane;      // columns [a, b) of the plane
        const size_t g0 = z * plane;                                                         // ... are voxels g0 + [a, b)
        size_t va = (g0 + a + kV - 1) / kV * kV - g0;
        if (va > b) va = b;
        const size_t nvec = (b - va) / kV, vb = va + nvec * kV;
        if (a + threadIdx.x < va) {
            const int32_t bn = bins[a + threadIdx.x];
            const T v = grid[g0 + a + threadIdx.x];
            if (bn >= 0 && v != (T)0) lds_add(&lds[bn], (A)v);
        }
        const Vec16<T>* pv = reinterpret_cast<const Vec16<T>*>(grid + g0 + va);
        for (size_t i = threadIdx.x; i < nvec; i += 256) {
            const Vec16<T> v = pv[i];
            const int32_t* pb = bins + va + i * kV;
#pragma unroll
            for (size_t k = 0; k < kV; k++) {
                const int32_t bn = pb[k];
                if (bn >= 0 && v.v[k] != (T)0) lds_add(&lds[bn], (A)v.v[k]);
            }
        }
        if (vb + threadIdx.x < b) {
            const int32_t bn = bins[vb + threadIdx.x];
            const T v = grid[g0 + vb + threadIdx.x];
            if (bn >= 0 && v != (T)0) lds_add(&lds[bn], (A)v);
        }
        __syncthreads();
        A* dst = partial + (pp * nz + z) * n_bins;
        for (uint32_t i = threadIdx.x; i < n_bins; i += 256) dst[i] = lds[i];
        __syncthreads();
    }
}

__device__ __forceinline__ void store_raw(u64* raw, size_t i, u64 v) { if (raw) raw[i] = v; }
__device__ __forceinline__ void store_raw(u64*, size_t, double) {}

// out[i] = partial[0][i] + partial[1][i] + ... : by one lane part after part (few parts), or by a wave whose lane l adds
// parts l, l + 64, ... before the fixed tree (many parts).  raw (may be null): the integer sums as they are.
template <typename A>
__global__ void __launch_bounds__(256) k_sum_finish(const A* __restrict__ partial, uint32_t P, size_t n_out,
                                                     double* __restrict__ out, u64* __restrict__ raw)
{
    if (P <= kFinishSerial) {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (size_t)gridDim.x * 256) {
            A acc = 0;
            for (uint32_t p = 0; p < P; p++) acc += partial[p * n_out + i];
            out[i] = as_weight(acc);
            store_raw(raw, i, acc);
        }
    } else {
        const uint32_t lane = threadIdx.x & 63u;
        for (size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n_out; i += (size_t)gridDim.x * 4) {
            A acc = 0;
            for (uint32_t p = lane; p < P; p += 64) acc += partial[p * n_out + i];
            acc = wave_sum(acc);
            if (lane == 0) {
                out[i] = as_weight(acc);
                store_raw(raw, i, acc);
            }
        }
    }
}

struct RowPlan { size_t n_rows, L; uint32_t P; size_t elems() const { return n_rows * P; } };
RowPlan plan_rows(size_t n_rows, size_t L) { return RowPlan{n_rows, L, (uint32_t)((L + kRowPart - 1) / kRowPart)}; }

struct ColPlan { size_t B, R, Cn, rows_per_part; uint32_t RP; size_t elems() const { return (size_t)RP * B * Cn; } };
ColPlan plan_cols(size_t B, size_t R, size_t Cn, size_t elem_bytes)
{
    const size_t kV = 16 / elem_bytes, n_cb = (Cn + 64 * kV - 1) / (64 * kV);
    size_t want = (kWaveTarget + B * n_cb - 1) / (B * n_cb), most = (R + kMinRows - 1) / kMinRows;
    if (want > most) want = most;
    if (want < 1) want = 1;
    const size_t rpp = (R + want - 1) / want;
    return ColPlan{B, R, Cn, rpp, (uint32_t)((R + rpp - 1) / rpp)};
}

// the passes of one axis sum: rows, columns, rows then columns over the rows' partial sums (y alone is kept), or rows twice
// (the grid total: one row of up to 2^31 voxels leaves thousands of parts, which are a row themselves -- one wave adding them
// all in k_sum_finish took as long as the pass over a 1 GiB grid)
struct AxesPlan { bool rows, cols, rows2; RowPlan rp, rp2; ColPlan cp; size_t n_out; uint32_t last_parts; };
AxesPlan plan_axes(size_t nx, size_t ny, size_t nz, int keep, size_t elem_bytes)
{
    AxesPlan a{};
    switch (keep) {
    case 0:
        a.rows = true; a.rp = plan_rows(1, nx * ny * nz); a.n_out = 1;
        if (a.rp.P > kFinishSerial) { a.rows2 = true; a.rp2 = plan_rows(1, a.rp.P); }
        break;
    case 4: a.rows = true; a.rp = plan_rows(nz, nx * ny); a.n_out = nz; break;
    case 6: a.rows = true; a.rp = plan_rows(nz * ny, nx); a.n_out = nz * ny; break;
    case 2: a.rows = a.cols = true; a.rp = plan_rows(nz * ny, nx); a.cp = plan_cols(1, a.rp.P * nz, ny, 8); a.n_out = ny; break;
    case 3: a.cols = true; a.cp = plan_cols(1, nz, ny * nx, elem_bytes); a.n_out = ny * nx; break;
    case 5: a.cols = true; a.cp = plan_cols(nz, ny, nx, elem_bytes); a.n_out = nz * nx; break;
    default: a.cols = true; a.cp = plan_cols(1, nz * ny, nx, elem_bytes); a.n_out = nx; break;      // 1
    }
    a.last_parts = a.cols ? a.cp.RP : (a.rows2 ? a.rp2.P : a.rp.P);
    return a;
}

struct BinPlan { size_t plane, part_len; uint32_t PP; };
BinPlan plan_bins(size_t plane, size_t nz, size_t n_bins)
{
    // a part flushes n_bins partial sums: with at least four voxels per bin the partials stay under a quarter of the grid
    const size_t least = 4 * n_bins > kBinPart ? 4 * n_bins : kBinPart;
    size_t want = (kBinGroups + nz - 1) / nz, most = (plane + least - 1) / least;
    if (want > most) want = most;
    if (want < 1) want = 1;
    const size_t len = (plane + want - 1) / want;
    return BinPlan{plane, len, (uint32_t)((plane + len - 1) / len)};
}

template <typename T>
void run_rows(const T* in, const RowPlan& p, typename AccOf<T>::type* partial, hipStream_t s)
{
    hipLaunchKernelGGL(k_sum_rows<T>, dim3(blocks_for(p.elems(), 4)), dim3(256), 0, s, in, p.n_rows, p.L, p.P, partial);
}
template <typename T>
void run_cols(const T* in, const ColPlan& p, typename AccOf<T>::type* partial, hipStream_t s)
{
    const size_t kV = 16 / sizeof(T), n_cb = (p.Cn + 64 * kV - 1) / (64 * kV);
    hipLaunchKernelGGL(k_sum_cols<T>, dim3(blocks_for(p.B * p.RP * n_cb, 4)), dim3(256), 0, s, in, p.B, p.R, p.Cn, p.RP,
                       p.rows_per_part, partial);
}
template <typename A>
void run_finish(const A* partial, uint32_t P, size_t n_out, double* out, u64* raw, hipStream_t s)
{
    hipLaunchKernelGGL(k_sum_finish<A>, dim3(blocks_for(n_out, P <= kFinishSerial ? 256 : 4)), dim3(256), 0, s, partial, P, n_out, out, raw);
}

template <typename T>
void sum_axes_t(const T* grid, const AxesPlan& a, void* partials, double* out, u64* raw, hipStream_t s)
{
    typedef typename AccOf<T>::type A;
    A* p1 = (A*)partials;
    const A* last = p1;
    if (a.rows) run_rows<T>(grid, a.rp, p1, s);
    if (a.rows && a.cols) { A* p2 = p1 + a.rp.elems(); run_cols<A>(p1, a.cp, p2, s); last = p2; }
    else if (a.rows2) { A* p2 = p1 + (a.rp.elems() + 1) / 2 * 2; run_rows<A>(p1, a.rp2, p2, s); last = p2; }
    else if (a.cols) run_cols<T>(grid, a.cp, p1, s);
    run_finish<A>(last, a.last_parts, a.n_out, out, raw, s);
}

template <typename T>
void sum_bins_t(const T* grid, const int32_t* bins, const BinPlan& b, uint32_t nz, uint32_t n_bins, void* partials, double* out,
                u64* raw, hipStream_t s)
{
    typedef typename AccOf<T>::type A;
    hipLaunchKernelGGL(k_sum_bins<T>, dim3(blocks_for((size_t)nz * b.PP, 1)), dim3(256), (size_t)n_bins * sizeof(A), s, grid, bins,
                       b.plane, nz, b.PP, b.part_len, n_bins, (A*)partials);
    run_finish<A>((const A*)partials, b.PP, (size_t)nz * n_bins, out, raw, s);
}

}  // namespace

// the grid as f64 weights (lt_read_grid_f64)
__global__ void k_grid_to_f64(const void* grid, int tally, size_t n, double* out)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (tally == LT_TALLY_F32) out[i] = as_weight(reinterpret_cast<const float*>(grid)[i]);
        else if (tally == LT_TALLY_F64) out[i] = reinterpret_cast<const double*>(grid)[i];
        else out[i] = as_weight(reinterpret_cast<const u64*>(grid)[i]);
    }
}

// dst += src over whole grids, 16 bytes per lane (the grids are hipMalloc'ed: 256-byte aligned).  Joins the private
// grid of an overlapped launch's second lane into the ctx grid: HBM-bound, 3 x grid bytes.
template <typename T>
__global__ void __launch_bounds__(256) k_grid_add(T* __restrict__ dst, const T* __restrict__ src, size_t n)
{
    constexpr size_t kV = 16 / sizeof(T);
    typedef Vec16<T> V;
    const size_t nv = n / kV;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
        V a = reinterpret_cast<V*>(dst)[i];
        const V b = reinterpret_cast<const V*>(src)[i];
#pragma unroll
        for (size_t k = 0; k < kV; k++) a.v[k] += b.v[k];
        reinterpret_cast<V*>(dst)[i] = a;
    }
    for (size_t i = nv * kV + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] += src[i];
}

hipError_t launch_grid_to_f64(const void* grid, int tally, size_t n, double* out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_grid_to_f64, dim3(kMaxBlocks), dim3(256), 0, s, grid, tally, n, out);
    return hipGetLastError();
}

hipError_t launch_grid_add(void* dst, const void* src, int tally, size_t n, hipStream_t s)
{
    with_tally_type(tally, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_grid_add<T>, dim3(kMaxBlocks), dim3(256), 0, s, (T*)dst, (const T*)src, n);
    });
    return hipGetLastError();
}

size_t tally_sum_axes_plan(int nx, int ny, int nz, int keep_mask, int tally, size_t* partial_bytes)
{
    const AxesPlan a = plan_axes((size_t)nx, (size_t)ny, (size_t)nz, keep_mask, tally_elem_bytes(tally));
    if (partial_bytes) *partial_bytes = ((a.rows ? a.rp.elems() : 0) + (a.cols ? a.cp.elems() : 0) + (a.rows2 ? a.rp2.elems() + 1 : 0)) * 8;
    return a.n_out;
}

hipError_t launch_tally_sum_axes(const void* grid, int tally, int nx, int ny, int nz, int keep_mask, void* partials, double* out,
                                 unsigned long long* raw, hipStream_t s)
{
    const AxesPlan a = plan_axes((size_t)nx, (size_t)ny, (size_t)nz, keep_mask, tally_elem_bytes(tally));
    with_tally_type(tally, [&](auto t) { sum_axes_t((const decltype(t)*)grid, a, partials, out, raw, s); });
    return hipGetLastError();
}

size_t tally_sum_columns_plan(int nx, int ny, int nz, int n_bins)
{
    return (size_t)plan_bins((size_t)nx * (size_t)ny, (size_t)nz, (size_t)n_bins).PP * (size_t)nz * (size_t)n_bins * 8;
}

hipError_t launch_tally_sum_columns(const void* grid, int tally, int nx, int ny, int nz, const int32_t* bins, int n_bins, void* partials,
                                    double* out, unsigned long long* raw, hipStream_t s)
{
    const BinPlan b = plan_bins((size_t)nx * (size_t)ny, (size_t)nz, (size_t)n_bins);
    with_tally_type(tally, [&](auto t) { sum_bins_t((const decltype(t)*)grid, bins, b, (uint32_t)nz, (uint32_t)n_bins, partials, out, raw, s); });
    return hipGetLastError();
}

hipError_t launch_tally_sum_finish(const void* partial, int integer, uint32_t P, size_t n_out, double* out, unsigned long long* raw,
                                   hipStream_t s)
{
    if (integer) run_finish<u64>((const u64*)partial, P, n_out, out, raw, s);
    else run_finish<double>((const double*)partial, P, n_out, out, nullptr, s);
    return hipGetLastError();
}

}  // namespace ltk
