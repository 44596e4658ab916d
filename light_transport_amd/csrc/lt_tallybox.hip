// lt_tallybox.hip -- a part of the voxel tally read out on the device (lt_tally_box): a box of the grid, every bx x by x bz
// voxels of it summed into one output voxel (the last block of an axis clipped to the box), as f64 weight and, for the
// fixed-point tally, as the exact integer sums.  A slice is a box one voxel thick, a coarser grid the whole grid with bin > 1.
// Every voxel of the box is read once; nothing but the output is written, and there are no partial sums in global memory.
//
// Sums are taken in the accumulator type of lt_tally.hpp (u64 for the fixed-point tally, f64 for f32 and f64).  Two kernels:
//   k_box_rows    SMALL blocks, many outputs.  A wave owns one row of output voxels (k, j) and a span of x of up to 64 lanes x
//                 16 bytes, cut to a multiple of bx.  A lane loads 16 bytes of every one of the by x bz grid rows of its
//                 outputs (at element alignment: a box starts at any x, rows may be odd) and adds them element by element in
//                 registers; the wave then puts its accumulators into LDS, and one lane per output adds the bx neighbours
//                 in ascending x.  The lane across the span's end takes its elements one by one.
//   k_box_blocks  LARGE blocks, any number of outputs.  One workgroup per output voxel: its 256 threads are laid over the
//                 block as (lanes along x) x (rows of the block), every thread adds its 16-byte pieces in a fixed sequence,
//                 then the fixed tree of wave_sum and the four wave totals in ascending order.
// THE RULE (box_is_large, on the host, from size and bin alone): with b = min(bin, size) per axis -- a bin beyond the box is
// the box -- k_box_blocks when a full block holds bx * by * bz >= kBoxLargeVoxels = 512 voxels, or when bx > kBoxSmallBx = 16
// (the neighbours of a span are added one after the other by a single lane); k_box_rows otherwise.  Below 512 voxels a
// workgroup per output would be mostly barrier, and a lane of the rows kernel adds at most 511 grid rows one after the other.
// Neither kernel uses atomics, and which thread adds what in which order follows from (grid shape, lo, size, bin) alone: the
// same call on an unchanged grid returns identical bits, for float tallies too.  With bin = (1, 1, 1) an output is 0 + voxel,
// converted: the weight exactly as lt_read_grid_f64 gives it (tallies hold no negative zero).
#include <hip/hip_runtime.h>

#include "lt_tally.hpp"

namespace ltk {
namespace {

template <typename T> struct alignas(sizeof(T)) VecEl { T v[16 / sizeof(T)]; };    // 16 bytes at element alignment

constexpr uint32_t kBoxLargeVoxels = 512, kBoxSmallBx = 16;

template <typename A>
__device__ __forceinline__ A wave_sum(A v)      // fixed tree; lane 0 holds the total
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ void store_raw(u64* raw, size_t i, u64 v) { if (raw) raw[i] = v; }
__device__ __forceinline__ void store_raw(u64*, size_t, double) {}

// the call, checked by the host: the box lies inside the grid, every size and bin is >= 1.  o = ceil(s / b) per axis.
struct Box {
    size_t nx, plane;                    // elements of a grid row and of a grid plane
    uint32_t lx, ly, lz, sx, sy, sz, bx, by, bz, ox, oy, oz;
};

__device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// One wave per (output row (k, j), chunk of `span` box columns); span is a multiple of b.bx and at most 64 x 16 / sizeof(T).
// The workgroup's four waves walk the items together (the barriers are reached by all), each with its own quarter of the LDS.
template <typename T>
__global__ void __launch_bounds__(256) k_box_rows(const T* __restrict__ grid, Box b, uint32_t span, uint32_t n_chunks,
                                                   double* __restrict__ out, u64* __restrict__ raw)
{
    typedef typename AccOf<T>::type A;
    constexpr uint32_t kV = 16 / sizeof(T);
    __shared__ A lds[4][64 * kV];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const size_t n_items = (size_t)b.oz * b.oy * n_chunks;
    for (size_t first = (size_t)blockIdx.x * 4; first < n_items; first += (size_t)gridDim.x * 4) {
        const size_t it = first + w;
        const bool live = it < n_items;
        uint32_t n = 0;          // box columns of this item
        size_t o0 = 0;           // its first output
        if (live) {
            const uint32_t c = (uint32_t)(it % n_chunks);
            const size_t q = it / n_chunks;
            const uint32_t j = (uint32_t)(q % b.oy), k = (uint32_t)(q / b.oy);
            const uint32_t xa = c * span, xb = min_u32(xa + span, b.sx);
            const uint32_t y0 = j * b.by, y1 = min_u32(y0 + b.by, b.sy), z0 = k * b.bz, z1 = min_u32(z0 + b.bz, b.sz);
            const uint32_t xe = xa + lane * kV;         // this lane's columns: xe .. xe + kV - 1, as far as they lie below xb
            A acc[kV];
#pragma unroll
            for (uint32_t e = 0; e < kV; e++) acc[e] = 0;
            const T* col = grid + (size_t)(b.lz + z0) * b.plane + (size_t)(b.ly + y0) * b.nx + b.lx + xe;
            if (xe + kV <= xb) {
                for (uint32_t z = z0; z < z1; z++, col += b.plane) {
                    const T* src = col;
#pragma unroll 4
                    for (uint32_t y = y0; y < y1; y++, src += b.nx) {
                        const VecEl<T> v = *reinterpret_cast<const VecEl<T>*>(src);
#pragma unroll
                        for (uint32_t e = 0; e < kV; e++) acc[e] += (A)v.v[e];
                    }
                }
            } else if (xe < xb) {
                for (uint32_t z = z0; z < z1; z++, col += b.plane) {
                    const T* src = col;
                    for (uint32_t y = y0; y < y1; y++, src += b.nx) {
#pragma unroll
                        for (uint32_t e = 0; e < kV; e++)
                            if (xe + e < xb) acc[e] += (A)src[e];
                    }
                }
            }
#pragma unroll
            for (uint32_t e = 0; e < kV; e++) lds[w][lane * kV + e] = acc[e];
            n = xb - xa;
            o0 = ((size_t)k * b.oy + j) * b.ox + xa / b.bx;
        }
        __syncthreads();
        const uint32_t n_o = (n + b.bx - 1) / b.bx;
        for (uint32_t q = lane; q < n_o; q += 64) {
            const uint32_t e0 = q * b.bx, e1 = min_u32(e0 + b.bx, n);
            A s = 0;
            for (uint32_t e = e0; e < e1; e++) s += lds[w][e];
            out[o0 + q] = as_weight(s);
            store_raw(raw, o0 + q, s);
        }
        __syncthreads();
    }
}

// One workgroup per output voxel.  Its block is hy x dz rows of wx contiguous voxels; the threads are 2^lx_log2 lanes along a
// row by 256 >> lx_log2 rows at a time.  A lane takes 16-byte pieces of its row at element alignment and the last wx % (16 /
// sizeof(T)) voxels one by one.
template <typename T>
__global__ void __launch_bounds__(256) k_box_blocks(const T* __restrict__ grid, Box b, uint32_t lx_log2, double* __restrict__ out,
                                                     u64* __restrict__ raw)
{
    typedef typename AccOf<T>::type A;
    constexpr uint32_t kV = 16 / sizeof(T);
    __shared__ A part[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t LX = 1u << lx_log2, tx = threadIdx.x & (LX - 1), ty = threadIdx.x >> lx_log2, RY = 256u >> lx_log2;
    const size_t n_out = (size_t)b.oz * b.oy * b.ox;
    for (size_t o = blockIdx.x; o < n_out; o += gridDim.x) {
        const uint32_t i = (uint32_t)(o % b.ox);
        const size_t q = o / b.ox;
        const uint32_t j = (uint32_t)(q % b.oy), k = (uint32_t)(q / b.oy);
        const uint32_t x0 = i * b.bx, wx = min_u32(b.bx, b.sx - x0), y0 = j * b.by, hy = min_u32(b.by, b.sy - y0);
        const uint32_t z0 = k * b.bz, dz = min_u32(b.bz, b.sz - z0);
        const uint32_t n_full = wx / kV, n_rows = hy * dz;       // (a block lies inside the grid: fewer than 2^31 voxels)
        const T* base = grid + (size_t)(b.lz + z0) * b.plane + (size_t)(b.ly + y0) * b.nx + b.lx + x0;
        A acc = 0;
        for (uint32_t r = ty; r < n_rows; r += RY) {
            const uint32_t rz = r / hy, ry = r - rz * hy;
            const T* row = base + (size_t)rz * b.plane + (size_t)ry * b.nx;
            for (uint32_t v = tx; v < n_full; v += LX) {
                const VecEl<T> x = *reinterpret_cast<const VecEl<T>*>(row + (size_t)v * kV);
#pragma unroll
                for (uint32_t e = 0; e < kV; e++) acc += (A)x.v[e];
            }
            for (uint32_t e = n_full * kV + tx; e < wx; e += LX) acc += (A)row[e];
        }
        acc = wave_sum(acc);
        if (lane == 0) part[w] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            A s = part[0];
            s += part[1];
            s += part[2];
            s += part[3];
            out[o] = as_weight(s);
            store_raw(raw, o, s);
        }
        __syncthreads();
    }
}

template <typename T>
void box_t(const T* grid, const Box& b, bool large, double* out, u64* raw, hipStream_t s)
{
    constexpr uint32_t kV = 16 / sizeof(T);
    if (large) {
        const uint32_t pieces = (b.bx + kV - 1) / kV;       // 16-byte pieces of a block's row
        uint32_t lx_log2 = 0;
        while (lx_log2 < 8 && (1u << lx_log2) < pieces) lx_log2++;
        hipLaunchKernelGGL(k_box_blocks<T>, dim3(blocks_for((size_t)b.oz * b.oy * b.ox, 1)), dim3(256), 0, s, grid, b, lx_log2, out, raw);
    } else {
        const uint32_t span = 64 * kV / b.bx * b.bx, n_chunks = (b.sx + span - 1) / span;
        hipLaunchKernelGGL(k_box_rows<T>, dim3(blocks_for((size_t)b.oz * b.oy * n_chunks, 4)), dim3(256), 0, s, grid, b, span, n_chunks, out, raw);
    }
}

bool box_is_large(const Box& b) { return (uint64_t)b.bx * b.by * b.bz >= kBoxLargeVoxels || b.bx > kBoxSmallBx; }

}  // namespace

hipError_t launch_tally_box(const void* grid, int tally, int nx, int ny, const int32_t lo[3], const int32_t size[3], const int32_t bin[3],
                            double* out, unsigned long long* raw, hipStream_t s)
{
    Box b;
    b.nx = (size_t)nx; b.plane = (size_t)nx * (size_t)ny;
    b.lx = (uint32_t)lo[0]; b.ly = (uint32_t)lo[1]; b.lz = (uint32_t)lo[2];
    b.sx = (uint32_t)size[0]; b.sy = (uint32_t)size[1]; b.sz = (uint32_t)size[2];
    // a bin beyond the box is the box: one block along that axis (and i * bin stays far below 2^32)
    b.bx = (uint32_t)(bin[0] < size[0] ? bin[0] : size[0]); b.by = (uint32_t)(bin[1] < size[1] ? bin[1] : size[1]);
    b.bz = (uint32_t)(bin[2] < size[2] ? bin[2] : size[2]);
    b.ox = (b.sx + b.bx - 1) / b.bx; b.oy = (b.sy + b.by - 1) / b.by; b.oz = (b.sz + b.bz - 1) / b.bz;
    const bool large = box_is_large(b);
    with_tally_type(tally, [&](auto t) { box_t((const decltype(t)*)grid, b, large, out, raw, s); });
    return hipGetLastError();
}

}  // namespace ltk
