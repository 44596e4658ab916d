// lt_tallyconv.hip -- the tally convolved in x and y on the device: the response of a laterally uniform medium to a beam of
// finite width from the pencil-beam tally (lt_tally_convolve, lt_tally_convolve_sep, lt_tally_convolve_at).
//
//   out[z][y][x] = sum over j, i of taps[j][i] * W[z][y - (j - kh/2)][x - (i - kw/2)],      W = 0 outside the grid
//
// The host hands the taps over FLIPPED in both axes (ft[j][i] = taps[kh-1-j][kw-1-i]), which turns the convolution into the
// correlation out[y][x] = sum ft[j][i] * W[y - kh/2 + j][x - kw/2 + i]: every index below only grows.
//
// k_conv_tile  one workgroup per 32 x 32 output tile of one plane.  The tile and its halo are widened to f64 weight once and
//              held in LDS; a tile whose input region holds nothing writes zeros and is done (most of a grid, away from the
//              beam).  A lane owns kR = 4 outputs adjacent in x and slides a register window along the row: kR LDS reads feed
//              kR x kR multiply-adds, and the tap of every multiply-add is a scalar operand (the tap index is uniform: the
//              taps are read through the scalar cache, never through LDS).  Rows of the LDS image are an ODD number of f64
//              apart, so the 32 lanes that one ds_read_b64 cycle serves (4 rows of 8 lanes, 8 banks from lane to lane) fall on
//              64 distinct banks.  The separable form is two launches of the same kernel: taps_x as a 1 x kw kernel into an
//              intermediate, then taps_y as a column (COLUMN: no window, one read per multiply-add -- that pass moves memory).
// k_conv_at    the convolved value at listed columns only: one wave per (z, column), lane l takes taps l, l + 64, ..., then the
//              fixed tree.
// No atomics anywhere: which lane adds what, in which order, follows from the shapes alone, so a call on an unchanged grid
// returns the same bits every time, and a plane's bits do not depend on which other planes were asked for.
#include <hip/hip_runtime.h>

#include "lt_tally.hpp"

namespace ltk {
namespace {

constexpr int kTX = 32, kTY = 32;              // output tile
constexpr int kR = kConvPad;                   // outputs per lane, adjacent in x; tap rows are padded to a multiple of it
constexpr int kLanesX = kTX / kR;
constexpr int kLoads = 8;                    // rows of the LDS image a lane fetches at once
static_assert(kLanesX * kTY == 256, "one lane per kR outputs of the tile");

// rows of the LDS image, in f64: the tile, the halo (kwp - 1 would do for the taps; the window reads one group of kR ahead) and
// one more where that is even
__host__ __device__ constexpr int conv_lds_width(int kwp, bool column) { return column ? kTX + 1 : kTX + kwp + 1; }

__device__ __forceinline__ double wave_sum(double v)      // fixed tree; lane 0 holds the total
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// in: planes [ny][nx] of T, plane z of the launch = the plane that out's plane z is computed from.  ft: flipped taps, [kh][kwp]
// with every row zero-padded from kw to kwp (COLUMN: [kh], kw = 1).  gridDim.x = ntx * nty * planes.
template <typename T, bool COLUMN>
__global__ void __launch_bounds__(256) k_conv_tile(const T* __restrict__ in, int nx, int ny, int ntx, int nty,
                                                    const double* __restrict__ ft, int kh, int kw, int kwp, double* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* lds = reinterpret_cast<double*>(lds_raw);
    const int lw = conv_lds_width(kwp, COLUMN), lh = kTY + kh - 1;
    uint32_t b = blockIdx.x;
    const int tx = (int)(b % (uint32_t)ntx);
    b /= (uint32_t)ntx;
    const int ty = (int)(b % (uint32_t)nty);
    const size_t z = b / (uint32_t)nty;
    const T* plane = in + z * (size_t)nx * (size_t)ny;
    const int gy0 = ty * kTY - kh / 2, gx0 = tx * kTX - kw / 2;
    const int w_real = kTX + kw - 1;      // columns of the image that the taps reach; the rest meets zero taps only and is zero itself

    // the image: a window that hangs over the grid's edge holds zeros there, and nothing beyond the plane is ever read
    int any = 0;
    const int c_step = COLUMN ? 32 : 64, r_step = 256 / c_step;
    for (int r0 = (int)threadIdx.x / c_step; r0 < lh; r0 += r_step * kLoads) {
        for (int c = (int)threadIdx.x % c_step; c < lw; c += c_step) {
            const int gx = gx0 + c;
            const bool col_in = c < w_real && gx >= 0 && gx < nx;
            const size_t gxc = (size_t)(gx < 0 ? 0 : (gx < nx ? gx : nx - 1));
            // kLoads rows in flight per lane: every load is issued (at coordinates clamped into the plane, so that none depends
            // on a branch), then the ones from outside the window are dropped
            T raw[kLoads];
#pragma unroll
            for (int u = 0; u < kLoads; u++) {
                const int gy = gy0 + r0 + u * r_step;
                raw[u] = plane[(size_t)(gy < 0 ? 0 : (gy < ny ? gy : ny - 1)) * (size_t)nx + gxc];
            }
#pragma unroll
            for (int u = 0; u < kLoads; u++) {
                const int r = r0 + u * r_step, gy = gy0 + r;
                if (r < lh) {
                    const double v = (col_in && gy >= 0 && gy < ny) ? as_weight(raw[u]) : 0.0;
                    lds[r * lw + c] = v;
                    any |= v != 0.0;
                }
            }
        }
    }
    any = __syncthreads_or(any);

    const int lx = ((int)threadIdx.x % kLanesX) * kR, ly = (int)threadIdx.x / kLanesX;
    double acc[kR];
#pragma unroll
    for (int r = 0; r < kR; r++) acc[r] = 0.0;
    if (any) {
        if (COLUMN) {
            const double* p = lds + ly * lw + lx;
            for (int j = 0; j < kh; j++, p += lw) {
                const double t = ft[j];
#pragma unroll
                for (int r = 0; r < kR; r++) acc[r] = fma(t, p[r], acc[r]);
            }
        } else {
            for (int j = 0; j < kh; j++) {
                const double* p = lds + (ly + j) * lw + lx;
                const double* tj = ft + j * kwp;
                double w[kR], n[kR];
#pragma unroll
                for (int r = 0; r < kR; r++) w[r] = p[r];
                for (int i0 = 0; i0 < kwp; i0 += kR) {
#pragma unroll
                    for (int r = 0; r < kR; r++) n[r] = p[i0 + kR + r];
#pragma unroll
                    for (int ii = 0; ii < kR; ii++) {
                        const double t = tj[i0 + ii];
#pragma unroll
                        for (int r = 0; r < kR; r++) acc[r] = fma(t, ii + r < kR ? w[(ii + r) % kR] : n[(ii + r) % kR], acc[r]);
                    }
#pragma unroll
                    for (int r = 0; r < kR; r++) w[r] = n[r];
                }
            }
        }
    }
    const int oy = ty * kTY + ly, ox = tx * kTX + lx;
    if (oy < ny) {
        double* dst = out + (z * (size_t)ny + (size_t)oy) * (size_t)nx + (size_t)ox;
#pragma unroll
        for (int r = 0; r < kR; r++)
            if (ox + r < nx) dst[r] = acc[r];
    }
}

// out[z * n_cols + c] = the convolved value at column cols[c] = (ix, iy) (inside the grid: checked by the caller) of plane z.
// taps [kh][kw] as the caller gave them.
template <typename T>
__global__ void __launch_bounds__(256) k_conv_at(const T* __restrict__ grid, int nx, int ny, int nz, const double* __restrict__ taps,
                                                  int kh, int kw, const int32_t* __restrict__ cols, int n_cols, double* __restrict__ out)
{
    const int lane = (int)(threadIdx.x & 63u);
    const size_t n_items = (size_t)nz * (size_t)n_cols, n_waves = (size_t)gridDim.x * 4;
    const int n_taps = kh * kw;
    for (size_t it = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < n_items; it += n_waves) {
        const size_t z = it / (size_t)n_cols, c = it - z * (size_t)n_cols;
        const int x = cols[2 * c], y = cols[2 * c + 1];
        const T* plane = grid + z * (size_t)nx * (size_t)ny;
        double acc = 0.0;
        for (int t = lane; t < n_taps; t += 64) {
            const int j = t / kw, i = t - j * kw;
            const int gy = y - (j - kh / 2), gx = x - (i - kw / 2);
            if (gy >= 0 && gy < ny && gx >= 0 && gx < nx) acc = fma(taps[t], as_weight(plane[(size_t)gy * (size_t)nx + (size_t)gx]), acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) out[it] = acc;
    }
}

template <typename T, bool COLUMN>
hipError_t run_tile(const T* in, int nx, int ny, size_t planes, const double* ft, int kh, int kw, int kwp, double* out, hipStream_t s)
{
    const int ntx = (nx + kTX - 1) / kTX, nty = (ny + kTY - 1) / kTY;
    const size_t blocks = (size_t)ntx * (size_t)nty * planes;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    const size_t lds = tally_conv_lds_bytes(kh, COLUMN ? 0 : kw);
    const void* fn = reinterpret_cast<const void*>(&k_conv_tile<T, COLUMN>);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_conv_tile<T, COLUMN>), dim3((uint32_t)blocks), dim3(256), lds, s, in, nx, ny, ntx, nty, ft, kh, kw, kwp, out);
    return hipGetLastError();
}

}  // namespace

size_t tally_conv_lds_bytes(int kh, int kw)
{
    return (size_t)conv_lds_width(conv_padded(kw), kw == 0) * (size_t)(kTY + kh - 1) * sizeof(double);
}

hipError_t launch_tally_convolve(const void* grid, int tally, int nx, int ny, int z0, int nz_out, const double* ft, int kh, int kw,
                                 double* out, hipStream_t s)
{
    const size_t skip = (size_t)z0 * (size_t)nx * (size_t)ny;
    return with_tally_type(tally, [&](auto t) {
        typedef decltype(t) T;
        return run_tile<T, false>((const T*)grid + skip, nx, ny, (size_t)nz_out, ft, kh, kw, conv_padded(kw), out, s);
    });
}

hipError_t launch_tally_convolve_sep(const void* grid, int tally, int nx, int ny, int z0, int nz_out, const double* ftx, int kw,
                                     const double* fty, int kh, double* mid, double* out, hipStream_t s)
{
    const size_t skip = (size_t)z0 * (size_t)nx * (size_t)ny;
    hipError_t e = with_tally_type(tally, [&](auto t) {
        typedef decltype(t) T;
        return run_tile<T, false>((const T*)grid + skip, nx, ny, (size_t)nz_out, ftx, 1, kw, conv_padded(kw), mid, s);
    });
    if (e != hipSuccess) return e;
    return run_tile<double, true>(mid, nx, ny, (size_t)nz_out, fty, kh, 1, 0, out, s);
}

hipError_t launch_tally_convolve_at(const void* grid, int tally, int nx, int ny, int nz, const double* taps, int kh, int kw,
                                    const int32_t* cols, int n_cols, double* out, hipStream_t s)
{
    with_tally_type(tally, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_conv_at<T>, dim3(blocks_for((size_t)nz * (size_t)n_cols, 4)), dim3(256), 0, s, (const T*)grid, nx, ny, nz,
                           taps, kh, kw, cols, n_cols, out);
    });
    return hipGetLastError();
}

}  // namespace ltk
