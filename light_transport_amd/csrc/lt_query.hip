// lt_query.hip -- the walk's __device__ functions one lane per query (lt_eval, lt_intersect_*, lt_rng_raw); the clearance- and march-grid builders
#include "lt_device.hpp"

namespace ltk {

// ---------------------------------------------------------------------------
// query kernels: the same __device__ functions, one lane per query (f64)
// ---------------------------------------------------------------------------
__global__ void k_intersect_rays(const TriD<double>* tris, const NodeD<double>* nodes, int n_tris, int n_nodes,
                                 const double* o, const double* d, const double* tmax, size_t n, int use_bvh,
                                 const MarchGrid G, const int16_t* links, int32_t* prim, double* t)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (use_bvh == 2) {     // the walk's wave-cooperative march (256 threads per workgroup: four waves)
        __shared__ MarchWave<double> mw[4];
        const bool want = i < n;
        const size_t k = want ? i : 0;
        int pi; double tt;
        march_service<double>(tris, nodes, n_nodes, G, &mw[threadIdx.x >> 6], want, o[3 * k], o[3 * k + 1], o[3 * k + 2], d[3 * k], d[3 * k + 1],
                              d[3 * k + 2], tmax ? tmax[k] : __builtin_huge_val(), 0.0, pi, tt);
        if (want) { prim[i] = pi; t[i] = tt; }
        return;
    }
    if (i >= n) return;
    double oo[3] = {o[3 * i], o[3 * i + 1], o[3 * i + 2]}, dd[3] = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    double tm = tmax ? tmax[i] : __builtin_huge_val();
    int pi; double tt;
    if (use_bvh == 4) nearest_bvh_ordered(tris, nodes, n_nodes, links + ray_octant(dd) * 2 * n_nodes, oo, dd, tm, pi, tt);   // front to back (the renderers' order)
    else if (use_bvh == 3) nearest_march(tris, nodes, n_nodes, G, oo, dd, tm, 0.0, pi, tt);      // the same march, lane by lane
    else if (use_bvh) nearest_bvh(tris, nodes, n_nodes, oo, dd, tm, pi, tt);
    else nearest_brute(tris, n_tris, oo, dd, tm, pi, tt);
    prim[i] = pi; t[i] = tt;
}

__global__ void k_triangle_intersect(const double* o, const double* d, const double* tris, size_t n, double* t)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // derive the PreComputedTriangle fields exactly as the host does
    // (S/primitives.py:105-111), without fused multiply-adds
    const double* a = tris + 9 * i; const double* b = a + 3; const double* c = a + 6;
    TriD<double> T;
    {
#pragma clang fp contract(off)
        for (int k = 0; k < 3; k++) { T.a[k] = a[k]; T.ab[k] = b[k] - a[k]; T.ac[k] = c[k] - a[k]; }
        double nn[3];
        nn[0] = T.ab[1] * T.ac[2] - T.ab[2] * T.ac[1];
        nn[1] = T.ab[2] * T.ac[0] - T.ab[0] * T.ac[2];
        nn[2] = T.ab[0] * T.ac[1] - T.ab[1] * T.ac[0];
        double l = ::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
        for (int k = 0; k < 3; k++) T.n[k] = nn[k] / l;
    }
    T.med_front = T.med_back = -1;
    double oo[3] = {o[3 * i], o[3 * i + 1], o[3 * i + 2]}, dd[3] = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    t[i] = tri_hit(oo, dd, &T);
}

__global__ void k_intersect_bounds(const double* o, const double* d, const double* tmax, const double* boxes,
                                   size_t n, int32_t* hit)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double oo[3] = {o[3 * i], o[3 * i + 1], o[3 * i + 2]};
    double inv[3] = {1.0 / d[3 * i], 1.0 / d[3 * i + 1], 1.0 / d[3 * i + 2]};
    double lo[3] = {boxes[6 * i], boxes[6 * i + 1], boxes[6 * i + 2]};
    double hi[3] = {boxes[6 * i + 3], boxes[6 * i + 4], boxes[6 * i + 5]};
    hit[i] = box_hit(lo, hi, oo, inv, tmax ? tmax[i] : __builtin_huge_val()) ? 1 : 0;
}

// one LT_FN_PLANE_REACH row: every value of it is representable in R (lt_eval narrowed the triangle; the caller rounds o, d, s)
template <typename R> LT_DEV void plane_reach_pair(const double* r, double* out)
{
    const R o[3] = {(R)r[0], (R)r[1], (R)r[2]}, d[3] = {(R)r[3], (R)r[4], (R)r[5]};
    TriD<R> T;
    for (int k = 0; k < 3; k++) { T.a[k] = (R)r[6 + k]; T.ab[k] = (R)r[9 + k]; T.ac[k] = (R)r[12 + k]; T.n[k] = (R)r[15 + k]; }
    T.med_front = T.med_back = -1;
    out[0] = plane_within_reach<R>(&T, o[0], o[1], o[2], d[0], d[1], d[2], (R)r[18], (R)r[20]) ? 1.0 : 0.0;
    out[1] = (double)tri_hit<R>(o, d, &T);
}

// one LT_FN_HG_WALK row: every value of it is representable in R (lt_layer_records made the record; the caller rounds xi)
template <typename R> LT_DEV void hg_walk_pair(const double* r, double* out)
{
    MedD<R> M;
    M.mu_t = (R)r[2]; M.inv_mu_t = (R)r[3]; M.absorb = (R)r[4]; M.g = (R)r[5];
    M.n = (R)r[6]; M.one_m_g2 = (R)r[7]; M.one_p_g2 = (R)r[8]; M.inv_2g = (R)r[9];
    M.dep = (R)r[10]; M.one_m_g = (R)r[11]; M.two_g = (R)r[12]; M.pad_ = 0;
    const R xi = (R)r[0];
    out[0] = (double)hg_sample_walk<R>(xi, &M);
    out[1] = (double)hg_sample_walk<R>(xi, M.two_g, M.one_m_g, M.one_m_g2, M.one_p_g2, M.inv_2g);
}

__global__ void k_eval(int fn, const double* in, size_t n, double* out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (fn) {
    case LT_FN_HG_PDF: out[i] = hg_pdf(in[2 * i], in[2 * i + 1]); break;
    case LT_FN_HG_SAMPLE: {
        double g = in[2 * i + 1];
        out[i] = hg_sample(in[2 * i], g, 1.0 - g * g, 1.0 + g * g, 1.0 / (2.0 * g));
    } break;
    case LT_FN_ONB: {
        double nn[3] = {in[3 * i], in[3 * i + 1], in[3 * i + 2]}, v2[3], v3[3];
        onb(nn, v2, v3);
        for (int k = 0; k < 3; k++) { out[6 * i + k] = v2[k]; out[6 * i + 3 + k] = v3[k]; }
    } break;
    case LT_FN_DISK: { double dd[2]; disk(in[2 * i], in[2 * i + 1], dd); out[2 * i] = dd[0]; out[2 * i + 1] = dd[1]; } break;
    case LT_FN_COSINE_HEMI: {
        double nn[3] = {in[8 * i], in[8 * i + 1], in[8 * i + 2]}, wi[3] = {in[8 * i + 3], in[8 * i + 4], in[8 * i + 5]}, o4[4];
        cosine_hemi(nn, wi, in[8 * i + 6], in[8 * i + 7], o4);
        for (int k = 0; k < 4; k++) out[4 * i + k] = o4[k];
    } break;
    case LT_FN_REFLECT: {
        double v[3] = {in[6 * i], in[6 * i + 1], in[6 * i + 2]}, nn[3] = {in[6 * i + 3], in[6 * i + 4], in[6 * i + 5]}, r[3];
        reflect(v, nn, r);
        for (int k = 0; k < 3; k++) out[3 * i + k] = r[k];
    } break;
    case LT_FN_BOUNDARY: {
        double dd[3] = {in[8 * i], in[8 * i + 1], in[8 * i + 2]}, nf[3] = {in[8 * i + 3], in[8 * i + 4], in[8 * i + 5]}, ct, refr[3];
        out[5 * i] = boundary(dd, nf, in[8 * i + 6], in[8 * i + 7], &ct, refr);
        out[5 * i + 1] = ct; out[5 * i + 2] = refr[0]; out[5 * i + 3] = refr[1]; out[5 * i + 4] = refr[2];
    } break;
    case LT_FN_SPIN: {
        double u[3] = {in[5 * i], in[5 * i + 1], in[5 * i + 2]};
        spin<double, true>(u, in[5 * i + 3], in[5 * i + 4], kWalkMathTab);
        for (int k = 0; k < 3; k++) out[3 * i + k] = u[k];
    } break;
    case LT_FN_WALK_MATH: {   // the walk's lean f64 primitives: -ln x, sin/cos(2 pi x), sqrt x, 1 / (1 + x)
        const double x = in[i];
        out[5 * i] = neg_log_tab(x, kWalkMathTab);
        sincos_turn_tab(x, kWalkMathTab, &out[5 * i + 1], &out[5 * i + 2]);
        out[5 * i + 3] = sqrt01(x);
        out[5 * i + 4] = fast_div(1.0, 1.0 + x);
    } break;
    case LT_FN_WALK_MATH_RAW: {   // ... and the forms the f64 XORWOW walk applies to the raw draw
        const unsigned k = (unsigned)in[i];
        out[3 * i] = neg_log_raw(k, kWalkMathTab);
        sincos_turn_raw(k, kWalkMathTab, &out[3 * i + 1], &out[3 * i + 2]);
    } break;
    case LT_FN_HG_WALK: {   // the walk's own deflection cosine, from the medium table and from the layer record, in walk precision
        const double* r = in + 14 * i;      // xi, f32, then a MedD record as the host built it for that precision
        if (r[1] != 0.0) hg_walk_pair<float>(r, out + 2 * i); else hg_walk_pair<double>(r, out + 2 * i);
    } break;
    case LT_FN_PLANE_REACH: {   // the walk's plane pre-test beside the triangle test it stands in front of, in walk precision
        const double* r = in + 21 * i;      // o[3], d[3], then the TriD fields a, ab, ac, n as the host filled them, s, f32, this triangle's reach_slack
        if (r[19] != 0.0) plane_reach_pair<float>(r, out + 2 * i); else plane_reach_pair<double>(r, out + 2 * i);
    } break;
    }
}

__global__ void k_rng_raw(unsigned long long seed, unsigned long long photon_id, unsigned count, uint32_t* out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    rocrand_state_xorwow st;
    photon_stream(seed, photon_id, &st);
    for (unsigned i = 0; i < count; i++) out[i] = rocrand(&st);
}

// ---------------------------------------------------------------------------
// clearance grid builder: per cell, min over triangles of the distance from the cell centre to the triangle
// (closest-point-on-triangle by regions), minus the half diagonal of the cell, shrunk by a safety margin
// ---------------------------------------------------------------------------
LT_DEV double point_tri_dist2(const double* p, const TriD<double>& T)
{
    const double ab[3] = {T.ab[0], T.ab[1], T.ab[2]}, ac[3] = {T.ac[0], T.ac[1], T.ac[2]};
    const double ap[3] = {p[0] - T.a[0], p[1] - T.a[1], p[2] - T.a[2]};
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    double q[3];
    if (d1 <= 0 && d2 <= 0) { q[0] = 0; q[1] = 0; q[2] = 0; }                       // vertex A
    else {
        const double bp[3] = {ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2]};
        const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
        const double cp[3] = {ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2]};
        const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
        const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        if (d3 >= 0 && d4 <= d3) { q[0] = ab[0]; q[1] = ab[1]; q[2] = ab[2]; }   // vertex B
        else if (vc <= 0 && d1 >= 0 && d3 <= 0) { const double v = d1 / (d1 - d3); for (int k = 0; k < 3; k++) q[k] = v * ab[k]; }
        else if (d6 >= 0 && d5 <= d6) { q[0] = ac[0]; q[1] = ac[1]; q[2] = ac[2]; }  // vertex C
        else if (vb <= 0 && d2 >= 0 && d6 <= 0) { const double w = d2 / (d2 - d6); for (int k = 0; k < 3; k++) q[k] = w * ac[k]; }
        else if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
            const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
            for (int k = 0; k < 3; k++) q[k] = ab[k] + w * (ac[k] - ab[k]);
        } else {
            const double den = 1.0 / (va + vb + vc), v = vb * den, w = vc * den;
            for (int k = 0; k < 3; k++) q[k] = v * ab[k] + w * ac[k];
        }
    }
    const double e[3] = {ap[0] - q[0], ap[1] - q[1], ap[2] - q[2]};
    return dot3(e, e);
}

// f16 <-> f32 for the clearance records (values >= 0; encode rounds toward zero so that the bound stays conservative)
LT_DEV unsigned half_down(double c)
{
    if (!(c > 0)) return 0u;
    if (!(c < 65504.0)) return c == __builtin_huge_val() ? 0x7c00u : 0x7bffu;
    _Float16 h = (_Float16)(float)c;
    unsigned short b = __builtin_bit_cast(unsigned short, h);
    if ((double)(float)h > c && b > 0) b--;
    return b;
}
LT_DEV float half_up(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(bits & 0xffffu)); }

__global__ void k_build_clearance(const TriD<double>* tris, int n_tris, int near_lists, uint4* clear, int nx, int ny, int nz,
                                  double ox, double oy, double oz, double hx, double hy, double hz)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nx * ny * nz) return;
    const int ix = (int)(i % nx), iy = (int)((i / nx) % ny), iz = (int)(i / ((size_t)nx * ny));
    const double p[3] = {ox + (ix + 0.5) * hx, oy + (iy + 0.5) * hy, oz + (iz + 0.5) * hz};
    // the five nearest triangles of the cell centre, nearest first (squared distances; ties keep the lower index first)
    const double inf = __builtin_huge_val();
    double best[5] = {inf, inf, inf, inf, inf};
    int id[5] = {-1, -1, -1, -1, -1};
    for (int t = 0; t < n_tris; t++) {
        double d2 = point_tri_dist2(p, tris[t]);
        int ti = t;
#pragma unroll
        for (int k = 0; k < 5; k++)
            if (d2 < best[k]) { const double sd = best[k]; const int si = id[k]; best[k] = d2; id[k] = ti; d2 = sd; ti = si; }
    }
    const double half_diag = 0.5 * ::sqrt(hx * hx + hy * hy + hz * hz);
    auto bound = [&](double d2) -> double {     // strictly conservative for every point of the cell
        if (d2 == inf) return inf;
        const double c = (::sqrt(d2) - half_diag) * (1.0 - 1e-6) - 1e-7 * (hx + hy + hz);
        return c > 0 ? c : 0.0;
    };
    const double c0 = bound(best[0]);
    float f = (float)c0;
    if ((double)f > c0 && f > 0) f = __uint_as_float(__float_as_uint(f) - 1u);      // round toward zero
    if (c0 == inf) f = 3.0e38f;
    unsigned y = 0, z = 0xffffffffu, w = 0xffffffffu;
    if (near_lists) {      // (ids are 16 bits: the host builds these records only for meshes whose tables fit LDS, <= ~1100 triangles, and refuses otherwise)
        y = half_down(bound(best[2])) | (half_down(bound(best[4])) << 16);
        z = (unsigned)(id[0] & 0xffff) | ((unsigned)(id[1] & 0xffff) << 16);      // (-1 & 0xffff = 0xffff: none)
        w = (unsigned)(id[2] & 0xffff) | ((unsigned)(id[3] & 0xffff) << 16);
    }
    clear[i] = make_uint4(__float_as_uint(f), y, z, w);
}

hipError_t launch_build_clearance(const void* tris_f64, int n_tris, int near_lists, void* clear_records, int nx, int ny, int nz,
                                  const double org[3], const double cell[3], hipStream_t s)
{
    const size_t n = (size_t)nx * ny * nz;
    if (n == 0 || n_tris <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_build_clearance, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const TriD<double>*>(tris_f64), n_tris, near_lists, reinterpret_cast<uint4*>(clear_records), nx, ny, nz,
                       org[0], org[1], org[2], cell[0], cell[1], cell[2]);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// march grid: c0 of every cell from the EXACT distance of the cell centre to the mesh, found by a nearest-point query in
// the BVH (a subtree is skipped when its box is not nearer than the best triangle so far).  Two levels: a coarse grid
// (cells 8 x 8 x 8 fine cells wide) is searched without a bound; a fine cell then starts from the bound its coarse cell
// implies, dist(p) <= dist(q) + |p - q|, so its search only opens the few subtrees around that sphere.  Cost ~ cells x
// tens of nodes instead of cells x triangles (k_build_clearance): 10^4 triangles get 128^3 cells instead of 58^3.
// ---------------------------------------------------------------------------
LT_DEV double point_box_dist2(const double* p, const NodeD<double>& nd)
{
    double s = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double e = __builtin_fmax(__builtin_fmax(nd.lo[k] - p[k], p[k] - nd.hi[k]), 0.0);
        s += e * e;
    }
    return s;
}
LT_DEV double mesh_dist2(const TriD<double>* tris, const NodeD<double>* nodes, int n_nodes, const double* p, double best)
{
    int cur = 0;
    while (cur < n_nodes) {
        const NodeD<double>& nd = nodes[cur];
        if (point_box_dist2(p, nd) <= best) {
            if (nd.n_prims > 0) {
                for (int k = 0; k < nd.n_prims; k++) best = __builtin_fmin(best, point_tri_dist2(p, tris[nd.offset + k]));
                cur = nd.skip;
            } else cur++;
        } else cur = nd.skip;
    }
    return best;
}
__global__ void k_march_coarse(const TriD<double>* tris, const NodeD<double>* nodes, int n_nodes, const MarchGrid G, int kx, int ky,
                               int kz, double* coarse)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)kx * ky * kz) return;
    const int ix = (int)(i % kx), iy = (int)((i / kx) % ky), iz = (int)(i / ((size_t)kx * ky));
    const double p[3] = {G.org[0] + (ix + 0.5) * 8.0 * G.h[0], G.org[1] + (iy + 0.5) * 8.0 * G.h[1], G.org[2] + (iz + 0.5) * 8.0 * G.h[2]};
    coarse[i] = ::sqrt(mesh_dist2(tris, nodes, n_nodes, p, __builtin_huge_val()));
}
__global__ void k_march_fine(const TriD<double>* tris, const NodeD<double>* nodes, int n_nodes, const MarchGrid G, int kx, int ky,
                             const double* coarse, uint2* cells)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)G.nx * G.ny * G.nz) return;
    const int ix = (int)(i % G.nx), iy = (int)((i / G.nx) % G.ny), iz = (int)(i / ((size_t)G.nx * G.ny));
    const double p[3] = {G.org[0] + (ix + 0.5) * G.h[0], G.org[1] + (iy + 0.5) * G.h[1], G.org[2] + (iz + 0.5) * G.h[2]};
    const int qx = ix >> 3, qy = iy >> 3, qz = iz >> 3;
    const double q[3] = {G.org[0] + (qx + 0.5) * 8.0 * G.h[0], G.org[1] + (qy + 0.5) * 8.0 * G.h[1], G.org[2] + (qz + 0.5) * 8.0 * G.h[2]};
    const double e[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    const double up = (coarse[((size_t)qz * ky + qy) * kx + qx] + ::sqrt(dot3(e, e))) * (1.0 + 1e-9);     // dist(p) <= this
    const double d2 = mesh_dist2(tris, nodes, n_nodes, p, up * up);
    const double half_diag = 0.5 * ::sqrt(G.h[0] * G.h[0] + G.h[1] * G.h[1] + G.h[2] * G.h[2]);
    // strictly conservative for every point of the cell (as k_build_clearance)
    double c0 = (::sqrt(d2) - half_diag) * (1.0 - 1e-6) - 1e-7 * (G.h[0] + G.h[1] + G.h[2]);
    if (!(c0 > 0)) c0 = 0.0;
    float f = (float)c0;
    if ((double)f > c0 && f > 0) f = __uint_as_float(__float_as_uint(f) - 1u);      // round toward zero
    cells[i].x = (__float_as_uint(f) & ~kMarchCountMask) | (cells[i].x & kMarchCountMask);      // the low bits hold the cell's candidate count
}
hipError_t launch_march_clearance(const void* tris_f64, const void* nodes_f64, int n_nodes, const MarchGrid& G, uint2* cells,
                                  double* coarse, hipStream_t s)
{
    const size_t n = (size_t)G.nx * G.ny * G.nz;
    if (n == 0 || n_nodes <= 0) return hipSuccess;
    const int kx = (G.nx + 7) / 8, ky = (G.ny + 7) / 8, kz = (G.nz + 7) / 8;
    const size_t nc = (size_t)kx * ky * kz;
    hipLaunchKernelGGL(k_march_coarse, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, s, reinterpret_cast<const TriD<double>*>(tris_f64),
                       reinterpret_cast<const NodeD<double>*>(nodes_f64), n_nodes, G, kx, ky, kz, coarse);
    hipLaunchKernelGGL(k_march_fine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const TriD<double>*>(tris_f64),
                       reinterpret_cast<const NodeD<double>*>(nodes_f64), n_nodes, G, kx, ky, coarse, cells);
    return hipGetLastError();
}

static inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

hipError_t launch_intersect_rays(const void* tris, const void* nodes, int n_tris, int n_nodes, const double* o,
                                 const double* d, const double* tmax, size_t n, int use_bvh, const MarchGrid* G, const int16_t* links,
                                 int32_t* prim, double* t, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    MarchGrid g;
    if (use_bvh == 4 && !links) use_bvh = 1;
    if (G) g = *G; else { memset(&g, 0, sizeof g); if (use_bvh == 2 || use_bvh == 3) use_bvh = 1; }
    hipLaunchKernelGGL(k_intersect_rays, dim3(nblk(n, 256)), dim3(256), 0, s,
                       reinterpret_cast<const TriD<double>*>(tris), reinterpret_cast<const NodeD<double>*>(nodes),
                       n_tris, n_nodes, o, d, tmax, n, use_bvh, g, links, prim, t);
    return hipGetLastError();
}
hipError_t launch_triangle_intersect(const double* o, const double* d, const double* tris, size_t n, double* t,
                                     hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_triangle_intersect, dim3(nblk(n, 256)), dim3(256), 0, s, o, d, tris, n, t);
    return hipGetLastError();
}
hipError_t launch_intersect_bounds(const double* o, const double* d, const double* tmax, const double* boxes,
                                   size_t n, int32_t* hit, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_intersect_bounds, dim3(nblk(n, 256)), dim3(256), 0, s, o, d, tmax, boxes, n, hit);
    return hipGetLastError();
}
hipError_t launch_eval(int fn, const double* in, size_t n, double* out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_eval, dim3(nblk(n, 256)), dim3(256), 0, s, fn, in, n, out);
    return hipGetLastError();
}
hipError_t launch_rng_raw(unsigned long long seed, unsigned long long photon_id, unsigned count, uint32_t* out,
                          hipStream_t s)
{
    hipLaunchKernelGGL(k_rng_raw, dim3(1), dim3(64), 0, s, seed, photon_id, count, out);
    return hipGetLastError();
}

}  // namespace ltk
