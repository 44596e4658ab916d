// lt_tallyrays.hip -- the voxel tally along arbitrary rays (lt_tally_rays, lt_tally_view): per ray the line integral of the
// tally, the largest voxel on the ray and the first voxel at or above a threshold.  One lane per ray, everything in f64, no
// atomics, nothing but the outputs written; built with -ffp-contract=off, so that every operation is rounded on its own.
//
// trace_ray is the one traversal both kernels call.  It clips the ray to the grid box with the slab test and then steps voxel
// to voxel (Amanatides-Woo).  The parameter of a grid plane is always the quotient
//     t(p) = ((origin_a + p * voxel_a) - o_a) / d_a
// of the plane's own coordinate, never a sum of increments: its error does not grow with the grid, and two voxels that share
// a plane see the same number.  A voxel's chord is (exit - entry) * |d| with entry the running parameter; a voxel whose chord
// rounds to <= 0 (a corner, an edge, a start within rounding of a plane) is stepped over and counts for nothing.
//
// The voxels a ray visits do not depend on what they hold, so a lane first works out its next kRayDepth (index, chord, entry)
// triples, issues their loads together and only then consumes them in the order walked: one exposed memory latency per
// kRayDepth voxels, not per voxel.  Past its end a lane repeats its last in-grid index with chord 0 (a load that is never used
// but never out of bounds).
//
// WHAT (a compile-time mask: 1 integral, 2 maximum, 4 first crossing) leaves out the registers and the work of what nobody asked
// for; the host instantiates 1, 2, 4 and 7 and takes 7 for any other combination.  The first-crossing-only form stops at the
// crossing.
//   k_tally_rays   ray r of the caller's arrays is lane r
//   k_tally_view   pinhole rays: a wave is an 8 x 8 pixel tile (a workgroup 16 x 16), so that its lanes read neighbouring voxels
#include <hip/hip_runtime.h>

#include <type_traits>

#include "lt_tally.hpp"

namespace ltk {
namespace {

constexpr int kRayDepth = 4;            // voxels a lane addresses before it consumes any
constexpr int kWantIntegral = 1, kWantMax = 2, kWantFirst = 4;

struct RayGrid {
    int n[3];                           // nx, ny, nz
    double org[3], vox[3];
};

struct RayResult {
    double integral, max_w, first_t;
    long long max_index, first_index;
};

__device__ __forceinline__ bool above(u64 a, u64 b) { return a > b; }
__device__ __forceinline__ bool above(double a, double b) { return a > b; }
__device__ __forceinline__ bool above(float a, float b) { return a > b; }

// the parameter of plane p of an axis (see the head of the file); d != 0
__device__ __forceinline__ double plane_t(double org, double vox, int p, double o, double d)
{
    return ((org + (double)p * vox) - o) / d;
}

template <typename T, int WHAT>
__device__ __forceinline__ RayResult trace_ray(const T* __restrict__ grid, const RayGrid& G, double ox, double oy, double oz, double dx,
                                               double dy, double dz, double t_lo, double t_hi, double threshold)
{
    RayResult R;
    R.integral = 0.0; R.max_w = 0.0; R.first_t = __builtin_inf(); R.max_index = -1; R.first_index = -1;
    const double o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
    const double inf = __builtin_inf();
    // the slab test; an axis the ray does not move along pins its index
    double t0 = t_lo, t1 = t_hi;
    int idx[3];
    bool miss = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        idx[a] = 0;
        if (d[a] == 0.0) {
            const double f = floor((o[a] - G.org[a]) / G.vox[a]);
            if (!(f >= 0.0 && f <= (double)(G.n[a] - 1))) miss = true;
            else idx[a] = (int)f;
        } else {
            const double ta = plane_t(G.org[a], G.vox[a], d[a] > 0.0 ? 0 : G.n[a], o[a], d[a]);
            const double tb = plane_t(G.org[a], G.vox[a], d[a] > 0.0 ? G.n[a] : 0, o[a], d[a]);
            t0 = fmax(t0, ta);
            t1 = fmin(t1, tb);
        }
    }
    if (miss || !(t0 < t1)) return R;
    const double len = sqrt(dx * dx + dy * dy + dz * dz);
    // the voxel at t0 (the walk's floor rule, clamped: on the plane it enters through the position is the plane's up to rounding),
    // and per axis the parameter of the next plane ahead
    int step[3], ahead[3];
    double tn[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        step[a] = d[a] > 0.0 ? 1 : -1;
        ahead[a] = d[a] > 0.0 ? 1 : 0;
        tn[a] = inf;
        if (d[a] != 0.0) {
            const double pos = o[a] + t0 * d[a];
            const double f = floor((pos - G.org[a]) / G.vox[a]);
            idx[a] = f >= (double)(G.n[a] - 1) ? G.n[a] - 1 : (f > 0.0 ? (int)f : 0);
            tn[a] = plane_t(G.org[a], G.vox[a], idx[a] + ahead[a], o[a], d[a]);
        }
    }
    // (the grid's numbers as values: selected between by the axis below, they must not turn into loads from the argument block)
    const int gnx = G.n[0], gny = G.n[1], gnz = G.n[2];
    const double gox = G.org[0], goy = G.org[1], goz = G.org[2], gvx = G.vox[0], gvy = G.vox[1], gvz = G.vox[2];
    int ix = idx[0], iy = idx[1], iz = idx[2];
    double tnx = tn[0], tny = tn[1], tnz = tn[2];
    const long long sy = G.n[0], sz = (long long)G.n[0] * G.n[1];
    long long flat = ((long long)iz * G.n[1] + iy) * G.n[0] + ix;
    const long long fx = step[0], fy = step[1] * sy, fz = step[2] * sz;
    double tcur = t0;
    bool done = false, have = false;
    T best = (T)0;
    while (!done) {
        long long vi[kRayDepth];
        double chord[kRayDepth], tin[kRayDepth];
        T w[kRayDepth];
#pragma unroll
        for (int u = 0; u < kRayDepth; u++) {
            vi[u] = flat; chord[u] = 0.0; tin[u] = tcur;
            if (!done) {
                const bool selx = tnx <= tny && tnx <= tnz, sely = !selx && tny <= tnz;
                const double tnext = selx ? tnx : (sely ? tny : tnz);
                const double tend = fmin(tnext, t1);
                if (tend > tcur) chord[u] = (tend - tcur) * len;
                tcur = fmax(tcur, tend);
                if (tnext >= t1) done = true;
                else {
                    const int i_new = (selx ? ix : (sely ? iy : iz)) + (selx ? step[0] : (sely ? step[1] : step[2]));
                    const int n_sel = selx ? gnx : (sely ? gny : gnz);
                    if ((unsigned)i_new >= (unsigned)n_sel) done = true;
                    else {
                        const double t_new = plane_t(selx ? gox : (sely ? goy : goz), selx ? gvx : (sely ? gvy : gvz),
                                                     i_new + (selx ? ahead[0] : (sely ? ahead[1] : ahead[2])), selx ? ox : (sely ? oy : oz),
                                                     selx ? dx : (sely ? dy : dz));
                        flat += selx ? fx : (sely ? fy : fz);
                        ix = selx ? i_new : ix; iy = sely ? i_new : iy; iz = (selx || sely) ? iz : i_new;
                        tnx = selx ? t_new : tnx; tny = sely ? t_new : tny; tnz = (selx || sely) ? tnz : t_new;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kRayDepth; u++) w[u] = grid[vi[u]];
#pragma unroll
        for (int u = 0; u < kRayDepth; u++) {
            if (!(chord[u] > 0.0)) continue;
            const double wd = as_weight(w[u]);
            if (WHAT & kWantIntegral) R.integral = R.integral + wd * chord[u];
            if (WHAT & kWantMax) {
                if (!have || above(w[u], best)) { best = w[u]; R.max_index = vi[u]; have = true; }
            }
            if (WHAT & kWantFirst) {
                if (R.first_index < 0 && wd >= threshold) {
                    R.first_index = vi[u]; R.first_t = tin[u];
                    if (WHAT == kWantFirst) done = true;
                }
            }
        }
    }
    if (WHAT & kWantMax) R.max_w = as_weight(best);
    return R;
}

struct RayOut {
    double* integral; double* max_w; long long* max_index; double* first_t; long long* first_index;
};

template <int WHAT>
__device__ __forceinline__ void store_ray(const RayOut& O, size_t r, const RayResult& R)
{
    if ((WHAT & kWantIntegral) && O.integral) O.integral[r] = R.integral;
    if (WHAT & kWantMax) {
        if (O.max_w) O.max_w[r] = R.max_w;
        if (O.max_index) O.max_index[r] = R.max_index;
    }
    if (WHAT & kWantFirst) {
        if (O.first_t) O.first_t[r] = R.first_t;
        if (O.first_index) O.first_index[r] = R.first_index;
    }
}

// o, d [n][3]; tr [n][2] or null = [0, +inf)
template <typename T, int WHAT>
__global__ void __launch_bounds__(256) k_tally_rays(const T* __restrict__ grid, RayGrid G, const double* __restrict__ o,
                                                     const double* __restrict__ d, const double* __restrict__ tr, size_t n, double threshold,
                                                     RayOut O)
{
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (size_t)gridDim.x * 256) {
        const double t_lo = tr ? tr[2 * r] : 0.0, t_hi = tr ? tr[2 * r + 1] : __builtin_inf();
        const RayResult R = trace_ray<T, WHAT>(grid, G, o[3 * r], o[3 * r + 1], o[3 * r + 2], d[3 * r], d[3 * r + 1], d[3 * r + 2], t_lo, t_hi,
                                               threshold);
        store_ray<WHAT>(O, r, R);
    }
}

struct RayCamera { double cam[3], f_distance; int W, H; };

// workgroup (bx, by) covers pixels 16 bx .. + 15 x 16 by .. + 15; wave w of it the 8 x 8 tile (w & 1, w >> 1)
template <typename T, int WHAT>
__global__ void __launch_bounds__(256) k_tally_view(const T* __restrict__ grid, RayGrid G, RayCamera C, const double* __restrict__ xs,
                                                     const double* __restrict__ ys, double threshold, RayOut O)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), i = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (i >= C.H || j >= C.W) return;
    const RayResult R = trace_ray<T, WHAT>(grid, G, C.cam[0], C.cam[1], C.cam[2], xs[j] - C.cam[0], ys[i] - C.cam[1], C.f_distance - C.cam[2],
                                           0.0, __builtin_inf(), threshold);
    store_ray<WHAT>(O, (size_t)i * C.W + j, R);
}

RayGrid ray_grid(const TallyRayGrid& g)
{
    RayGrid G;
    for (int a = 0; a < 3; a++) { G.n[a] = g.n[a]; G.org[a] = g.origin[a]; G.vox[a] = g.voxel[a]; }
    return G;
}

RayOut ray_out(const TallyRayOut& o)
{
    return RayOut{o.integral, o.max_w, (long long*)o.max_index, o.first_t, (long long*)o.first_index};
}

// f(T{}, mask) with the instantiated mask that covers what `out` asks for
template <typename F> void with_ray_form(int tally, const TallyRayOut& out, F&& f)
{
    const int want = tally_ray_mask(out);
    with_tally_type(tally, [&](auto t) {
        if (want == kWantIntegral) f(t, std::integral_constant<int, kWantIntegral>());
        else if (want == kWantMax) f(t, std::integral_constant<int, kWantMax>());
        else if (want == kWantFirst) f(t, std::integral_constant<int, kWantFirst>());
        else f(t, std::integral_constant<int, kWantIntegral | kWantMax | kWantFirst>());
    });
}

}  // namespace

int tally_ray_mask(const TallyRayOut& out)
{
    return (out.integral ? kWantIntegral : 0) | ((out.max_w || out.max_index) ? kWantMax : 0) | ((out.first_t || out.first_index) ? kWantFirst : 0);
}

hipError_t launch_tally_rays(const void* grid, int tally, const TallyRayGrid& g, const double* o, const double* d, const double* t_range,
                             size_t n, double threshold, const TallyRayOut& out, hipStream_t s)
{
    const RayGrid G = ray_grid(g);
    const RayOut O = ray_out(out);
    const uint32_t blocks = blocks_for(n, 256);
    with_ray_form(tally, out, [&](auto t, auto m) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_tally_rays<T, decltype(m)::value>), dim3(blocks), dim3(256), 0, s, (const T*)grid, G, o, d, t_range, n, threshold, O);
    });
    return hipGetLastError();
}

hipError_t launch_tally_view(const void* grid, int tally, const TallyRayGrid& g, int width, int height, const double camera[3],
                             double f_distance, const double* xs, const double* ys, double threshold, const TallyRayOut& out, hipStream_t s)
{
    const RayGrid G = ray_grid(g);
    const RayOut O = ray_out(out);
    RayCamera C;
    for (int a = 0; a < 3; a++) C.cam[a] = camera[a];
    C.f_distance = f_distance; C.W = width; C.H = height;
    const dim3 blocks((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
    with_ray_form(tally, out, [&](auto t, auto m) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((k_tally_view<T, decltype(m)::value>), blocks, dim3(256), 0, s, (const T*)grid, G, C, xs, ys, threshold, O);
    });
    return hipGetLastError();
}

}  // namespace ltk
