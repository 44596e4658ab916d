// lt_render.hip -- the two surface renderers (lt_render_surface) on the intersection and sampling functions of lt_device.hpp
#include "lt_device.hpp"

namespace ltk {

// ---------------------------------------------------------------------------
// surface path tracer: trace_path + render_scene of S/path_tracing_fix1.py:18-169,
// one lane per pixel, samples looped in the lane (no atomics: a pixel has one owner)
// ---------------------------------------------------------------------------
LT_DEV void mark_unused(double* rand_0, size_t base, int from, int D)  // :36-38, :64-66, :128-130
{
    for (int b = from; b < D; b++) rand_0[base + b] = __builtin_huge_val();
}

// cast_one_shadow_ray (S/light_samples.py:36-61): radiance * brdf * geometry term * area of light sample `choice`
// as seen from X (offset along n); false when the sample is occluded.
__device__ __forceinline__ bool shadow_direct(const RenderParams& P, const TriD<double>* tris, const NodeD<double>* nodes, const int16_t* links,
                                              const double X[3], const double n[3], const lt_surface_material& M,
                                              int choice, double out[3])
{
    const double eps = 1e-6, inv_pi = 0.3183098861837907, inf = __builtin_huge_val();
    const double so[3] = {X[0] + eps * n[0], X[1] + eps * n[1], X[2] + eps * n[2]};
    const lt_point_light lt = P.lights[choice];
    double v[3] = {lt.source[0] - so[0], lt.source[1] - so[1], lt.source[2] - so[2]};
    const double mag = ::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double sd[3] = {v[0] / mag, v[1] / mag, v[2] / mag};
    // (the reference takes the nearest hit of the shadow ray and asks whether it lies at mag - EPSILON or beyond, :49-52: the
    // sample is hidden exactly when SOME triangle is hit nearer than that, so the search stops at the first one it finds)
    int sp; double st;
    nearest_bvh_render(tris, nodes, P.n_nodes, links, so, sd, mag - eps, sp, st, true);
    (void)inf;
    if (sp >= 0) return false;
    const double cos_t = dot3(n, sd);
    const double nsd[3] = {-sd[0], -sd[1], -sd[2]};
    const double cos_p = dot3(lt.normal, nsd);
    const double geom = ::fabs(cos_t * cos_p) / (mag * mag);
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = (lt.radiance[k] * (M.diffuse[k] * inv_pi)) * geom * lt.total_area;
    return true;
}

// cos x for |x| <= 1 + rounding (the reference takes the cosine of a DOT PRODUCT of unit vectors, quirk B5): Taylor series to
// x^24 / 24!, truncation < 2e-26 -- OCML's general cos carries a Payne-Hanek reduction for huge arguments and its pow a log / exp pair with
// double-double arithmetic; inlined into the render kernels they cost ~100 VGPRs for one Schlick term
__device__ __forceinline__ double cos_unit(double x)
{
    const double z = x * x;
    double p = 1.6117373109360196e-24;                     //  1/24!
    p = __builtin_fma(p, z, -8.8967913924505741e-22);      // -1/22!
    p = __builtin_fma(p, z, 4.1103176233121648e-19);       //  1/20!
    p = __builtin_fma(p, z, -1.5619206968586225e-16);      // -1/18!
    p = __builtin_fma(p, z, 4.7794773323873853e-14);       //  1/16!
    p = __builtin_fma(p, z, -1.1470745597729725e-11);      // -1/14!
    p = __builtin_fma(p, z, 2.0876756987868099e-09);       //  1/12!
    p = __builtin_fma(p, z, -2.7557319223985891e-07);      // -1/10!
    p = __builtin_fma(p, z, 2.4801587301587302e-05);       //  1/8!
    p = __builtin_fma(p, z, -1.3888888888888889e-03);      // -1/6!
    p = __builtin_fma(p, z, 4.1666666666666664e-02);       //  1/4!
    p = __builtin_fma(p, z, -0.5);
    return __builtin_fma(p, z, 1.0);
}

// mirror (:82-85) and glass (:86-119, kept as written, quirk B5) branches of trace_path: new ray in o, d
__device__ __forceinline__ void specular_bounce(const lt_surface_material& M, const double X[3], const double n[3],
                                                bool inside, double r0, double o[3], double d[3])
{
    const double eps = 1e-6;
    if (!M.is_mirror) {
        const double n1 = inside ? M.ior : 1.0, n2 = inside ? 1.0 : M.ior;
        const double R0 = ((n1 - n2) / (n1 + n2)) * ((n1 - n2) / (n1 + n2));
        const double theta = dot3(d, n);
        // (theta is a dot product of unit vectors; x^5 by three products: within 2 ulp of pow(x, 5.0), the render's pins hold to 1e-9)
        const double om = 1 - cos_unit(theta), om2 = om * om;
        const double refl_prob = R0 + (1 - R0) * (om2 * om2 * om);
        double Nr = M.ior;
        if (theta > 0) Nr = 1 / Nr;
        Nr = 1 / Nr;
        const double cos_theta = -theta;
        const double rad = 1 - (Nr * Nr) * (1 - cos_theta * cos_theta);
        if (rad > 0 && r0 > refl_prob) {
            const double kk = Nr * cos_theta - ::sqrt(rad);
            double tr[3] = {d[0] * Nr + n[0] * kk, d[1] * Nr + n[1] * kk, d[2] * Nr + n[2] * kk};
            normalize3(tr);
#pragma unroll
            for (int k = 0; k < 3; k++) { o[k] = X[k] - eps * n[k]; d[k] = tr[k]; }
            return;
        }
    }
    double r[3]; reflect(d, n, r);
#pragma unroll
    for (int k = 0; k < 3; k++) { o[k] = X[k] + eps * n[k]; d[k] = r[k]; }
}


// One lane per PATH (pixel, sample), 256 lanes per workgroup: a workgroup owns PPB = max(1, 256 / S) whole pixels, its lanes
// trace their paths side by side, park the radiance in LDS, and one lane per pixel then adds its samples in ascending order --
// the reference's own order of summation (:148-164), so the image is what the sample loop of round 1-3's kernel gave, bit for
// bit.  (That kernel ran one lane per pixel over all its samples: 90 000 lanes for the notebook's 300 x 300 render, a third of
// the device's lanes for 50 sequential paths each.)  Pixels with more than 256 samples take several rounds.  The scene tables
// (triangles, BVH nodes, materials: 7 KB for the notebook's scene) are staged in LDS when they fit 48 KiB (LDS_TABLES) and
// lt_set_tuning "render_lds_tables" is not 0; the 2000 point lights (160 KB) and the random tables stay in global memory.
constexpr int kRenderThreads = 256;
#ifndef LT_RENDER_WAVES
#define LT_RENDER_WAVES 4      // waves per SIMD the register allocator leaves room for: 2 (172 VGPRs, no scratch) 7.1 ms, 3 (168 + 12 B)
                               // 5.2 ms, 4 (128 + 188 B of scratch) 4.6 ms for the 300 x 300 x 50 spp render (profiles/r04e_render_time.log)
#endif
template <bool LDS_TABLES>
__global__ void __launch_bounds__(kRenderThreads, LT_RENDER_WAVES) k_render_surface(const RenderParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char r_lds[];
    double* s_L = reinterpret_cast<double*>(r_lds);                                       // [256][3] radiance of the lanes' paths
    const size_t off_t = (size_t)kRenderThreads * 3 * sizeof(double);
    const size_t off_n = off_t + (size_t)P.n_tris * sizeof(TriD<double>), off_m = off_n + (size_t)P.n_nodes * sizeof(NodeD<double>);
    const TriD<double>* tris = LDS_TABLES ? reinterpret_cast<const TriD<double>*>(r_lds + off_t) : reinterpret_cast<const TriD<double>*>(P.tris);
    const NodeD<double>* nodes = LDS_TABLES ? reinterpret_cast<const NodeD<double>*>(r_lds + off_n) : reinterpret_cast<const NodeD<double>*>(P.nodes);
    const lt_surface_material* mats = LDS_TABLES ? reinterpret_cast<const lt_surface_material*>(r_lds + off_m) : P.mats;
    const size_t off_k = off_m + (size_t)P.n_tris * sizeof(lt_surface_material);
    const int16_t* links = LDS_TABLES ? reinterpret_cast<const int16_t*>(r_lds + off_k) : P.links;
    if constexpr (LDS_TABLES) {
        lds_copy(r_lds + off_k, P.links, (size_t)((16 * P.n_nodes * 2 + 3) / 4) * 4);
        lds_copy(r_lds + off_t, P.tris, (size_t)P.n_tris * sizeof(TriD<double>));
        lds_copy(r_lds + off_n, P.nodes, (size_t)P.n_nodes * sizeof(NodeD<double>));
        lds_copy(r_lds + off_m, P.mats, (size_t)P.n_tris * sizeof(lt_surface_material));
        __syncthreads();
    }
    const double eps = 1e-6, inv_pi = 0.3183098861837907, inf = __builtin_huge_val();
    const int tid = threadIdx.x;
    const int chunk = P.S < kRenderThreads ? P.S : kRenderThreads;       // samples of one pixel traced per round
    const int ppb = kRenderThreads / chunk;                              // whole pixels per workgroup
    const int pl = tid / chunk, sl = tid % chunk;                        // this lane's pixel (local) and sample slot
    const int pix = blockIdx.x * ppb + pl;
    const bool owner = tid < ppb && blockIdx.x * ppb + tid < P.W * P.H;  // lane tid sums local pixel tid
    double color[3] = {0, 0, 0};
    for (int s0 = 0; s0 < P.S; s0 += chunk) {
        const int smp = s0 + sl;
        double L[3] = {0, 0, 0};
        if (pl < ppb && pix < P.W * P.H && smp < P.S) {
            const int i = pix / P.W, j = pix % P.W;
            const size_t base = (((size_t)i * P.W + j) * P.S + smp) * (size_t)P.D;
            // camera ray, :152-160 (anti-alias jitter re-uses the bounce-0 uniform for x and y)
            double o[3] = {P.cam[0], P.cam[1], P.cam[2]};
            const double jit = P.rand_0[base];
            double d[3] = {P.xs[j] + jit / (double)P.W - o[0], P.ys[i] + jit / (double)P.H - o[1], P.f_distance - o[2]};
            normalize3(d);
            double thr[3] = {1, 1, 1};
            // ONE traversal site serves both kinds of ray: (o, d) is the ray the next search follows -- the path's own ray, or,
            // while `shadow`, the shadow ray of the diffuse hit (`hit`, `thit` on the stashed path ray po, pd) whose shading
            // is completed when the search returns.  Two inlined copies of the traversal cost the kernel 221 VGPRs; the
            // expressions evaluated are those of trace_path / cast_one_shadow_ray, in the same order.
            bool shadow = false;
            int hit = -1; double thit = 0, smag = 0;
            double po[3] = {0, 0, 0}, pd[3] = {0, 0, 1};
            for (int bounce = 0;;) {
                if (!shadow && bounce >= P.D) break;                        // :24-26
                int prim; double t;
                nearest_bvh_render(tris, nodes, P.n_nodes, links, o, d, shadow ? smag - eps : inf, prim, t, shadow);    // hit_object, :32 / cast_one_shadow_ray
                const double r0 = P.rand_0[base + bounce], r1 = P.rand_1[base + bounce];
                if (!shadow) {
                    if (prim < 0) { mark_unused(P.rand_0, base, bounce, P.D); break; }
                    const lt_surface_material M = mats[prim];
                    double n[3] = {tris[prim].n[0], tris[prim].n[1], tris[prim].n[2]};
                    const double X[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
                    if (M.is_light) { L[0] += M.emission * thr[0]; L[1] += M.emission * thr[1]; L[2] += M.emission * thr[2]; }
                    bool inside = false;
                    if (dot3(n, d) > 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; inside = true; }   // :48-51
                    if (M.is_diffuse) {
                        // direct light: cast_one_shadow_ray, S/light_samples.py:36-61 -- the shadow ray becomes the ray to follow
                        const lt_point_light lt = P.lights[P.light_choice[base + bounce]];
#pragma unroll
                        for (int k = 0; k < 3; k++) { po[k] = o[k]; pd[k] = d[k]; o[k] = X[k] + eps * n[k]; }
                        double v[3] = {lt.source[0] - o[0], lt.source[1] - o[1], lt.source[2] - o[2]};
                        smag = ::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                        d[0] = v[0] / smag; d[1] = v[1] / smag; d[2] = v[2] / smag;
                        hit = prim; thit = t; shadow = true;
                        continue;
                    } else if (M.is_mirror || M.transmission > 0.0) {           // :82-119
                        specular_bounce(M, X, n, inside, r0, o, d);
                    } else break;                                               // :121-123
                } else {
                    // the shadow ray is back: finish the diffuse hit it belongs to
                    shadow = false;
                    const lt_surface_material M = mats[hit];
                    double n[3] = {tris[hit].n[0], tris[hit].n[1], tris[hit].n[2]};
                    if (dot3(n, pd) > 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
                    const double X[3] = {po[0] + thit * pd[0], po[1] + thit * pd[1], po[2] + thit * pd[2]};
                    if (prim < 0) {      // nothing nearer than the light sample: radiance * brdf * geometry term * area, :53-61
                        const lt_point_light lt = P.lights[P.light_choice[base + bounce]];
                        const double cos_t = dot3(n, d);
                        const double nsd[3] = {-d[0], -d[1], -d[2]};
                        const double cos_p = dot3(lt.normal, nsd);
                        const double geom = ::fabs(cos_t * cos_p) / (smag * smag);
#pragma unroll
                        for (int k = 0; k < 3; k++) L[k] += thr[k] * ((lt.radiance[k] * (M.diffuse[k] * inv_pi)) * geom * lt.total_area);
                    }
                    // indirect: cosine lobe, :63-80
                    double o4[4];
                    cosine_hemi<double, true>(n, pd, r0, r1, o4);
                    if (o4[3] == 0) { mark_unused(P.rand_0, base, bounce + 1, P.D); break; }
                    const double cos_theta = o4[0] * n[0] + o4[1] * n[1] + o4[2] * n[2];
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        thr[k] *= (M.diffuse[k] * inv_pi) * cos_theta / o4[3];
                        o[k] = X[k] + eps * o4[k];
                        d[k] = o4[k];
                    }
                }
                if (bounce > 5) {                                           // russian roulette, :126-132
                    const double rr = ::fmax(0.05, 1 - thr[1]);
                    if (r0 < rr) { mark_unused(P.rand_0, base, bounce + 1, P.D); break; }
                    thr[0] /= 1 - rr; thr[1] /= 1 - rr; thr[2] /= 1 - rr;
                }
                bounce++;
            }
        }
        s_L[tid * 3] = L[0]; s_L[tid * 3 + 1] = L[1]; s_L[tid * 3 + 2] = L[2];
        __syncthreads();
        if (owner) {        // color += light, sample by sample (:162)
            const int ns = P.S - s0 < chunk ? P.S - s0 : chunk;
            for (int q = 0; q < ns; q++) {
                const double* l = s_L + (size_t)(tid * chunk + q) * 3;
                color[0] += l[0]; color[1] += l[1]; color[2] += l[2];
            }
        }
        __syncthreads();
    }
    if (owner) {
        const size_t px = (size_t)blockIdx.x * ppb + tid;
#pragma unroll
        for (int k = 0; k < 3; k++) {                                       // :164-166
            double c = color[k] / (double)P.S;
            c = c < 0 ? 0.0 : (c > 1 ? 1.0 : c);
            P.image[px * 3 + k] += 0.25 * c;
        }
    }
}

// path_tracing_old.py:17-171 -- the recursive ancestor of trace_path that examples/LTS.ipynb still calls.  A diffuse hit
// calls trace_path(ray, bounce + 1) on the SHARED ray and, once that returns, carries on from wherever the callee left
// the ray (:68-80); emission counts at bounce 0 only (:45), the direct term is not throughput-weighted (:80), roulette
// starts after bounce 3 (:127) and the pixel is overwritten with clip(mean) (:167).  The recursion is unrolled into an
// explicit per-lane stack of (throughput, light, direct, r0, bounce) frames, visited in the reference's depth-first
// order so that the +inf markers written into rand_0 are read back exactly where the reference reads them.
// One lane per PATH (pixel, sample) as in k_render_surface, one wave per workgroup; the frame being executed lives in
// registers, the frames of its callers in LDS ([depth][field][lane]: at most D of them, 45 KiB for the notebook's depth 8) --
// rounds 1-3 kept the whole stack of 25 frames in scratch memory (2288 B per lane) and looped over a pixel's samples in one lane.
constexpr int kOldThreads = 64, kOldFields = 11;      // thr[3], L[3], direct[3], r0, bounce
__global__ void __launch_bounds__(kOldThreads) k_render_surface_old(const RenderParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char r_lds[];
    double* s_L = reinterpret_cast<double*>(r_lds);                       // [64][3]
    double* s_st = s_L + kOldThreads * 3;                                 // [D][kOldFields][64]
    const TriD<double>* tris = reinterpret_cast<const TriD<double>*>(P.tris);
    const NodeD<double>* nodes = reinterpret_cast<const NodeD<double>*>(P.nodes);
    const double eps = 1e-6, inv_pi = 0.3183098861837907, inf = __builtin_huge_val();
    const int tid = threadIdx.x;
    const int chunk = P.S < kOldThreads ? P.S : kOldThreads, ppb = kOldThreads / chunk;
    const int pl = tid / chunk, sl = tid % chunk;
    const int pix = blockIdx.x * ppb + pl;
    const bool owner = tid < ppb && blockIdx.x * ppb + tid < P.W * P.H;
    double color[3] = {0, 0, 0};
    for (int s0 = 0; s0 < P.S; s0 += chunk) {
        const int smp = s0 + sl;
        double ret[3] = {0, 0, 0};
        if (pl < ppb && pix < P.W * P.H && smp < P.S) {
            const int i = pix / P.W, j = pix % P.W;
            const size_t sample = ((size_t)i * P.W + j) * P.S + smp;
            const size_t base = sample * (size_t)P.D;
            const int32_t* choice = P.light_choice + sample * (size_t)P.choices;
            unsigned n_shadow = 0;
            double o[3] = {P.cam[0], P.cam[1], P.cam[2]};
            const double jit = P.rand_0[base];                               // :158-159
            double d[3] = {P.xs[j] + jit / (double)P.W - o[0], P.ys[i] + jit / (double)P.H - o[1], P.f_distance - o[2]};
            normalize3(d);
            int depth = 0;
            bool resume = false;
            // the frame in execution
            double f_thr[3] = {1, 1, 1}, f_L[3] = {0, 0, 0}, f_direct[3] = {0, 0, 0}, f_r0 = 0.0;
            int f_bounce = 0;
            for (;;) {
                bool done = false;
                if (resume) {                                                // back from trace_path(bounce + 1), :78-80
                    resume = false;
#pragma unroll
                    for (int k = 0; k < 3; k++) f_L[k] += (f_direct[k] + f_thr[k] * ret[k]);
                } else if (f_bounce >= P.D) {                                // :24-25
                    done = true;
                } else {
                    const double r0 = P.rand_0[base + f_bounce], r1 = P.rand_1[base + f_bounce];
                    f_r0 = r0;
                    int prim; double t;
                    nearest_bvh_render(tris, nodes, P.n_nodes, P.links, o, d, inf, prim, t);
                    if (prim < 0) { mark_unused(P.rand_0, base, f_bounce, P.D); done = true; }
                    else {
                        const lt_surface_material M = P.mats[prim];
                        double n[3] = {tris[prim].n[0], tris[prim].n[1], tris[prim].n[2]};
                        const double X[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
                        if (M.is_light && f_bounce == 0) {                   // :45-46
#pragma unroll
                            for (int k = 0; k < 3; k++) f_L[k] += M.emission * f_thr[k];
                        }
                        bool inside = false;
                        if (dot3(n, d) > 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; inside = true; }
                        if (M.is_diffuse) {
                            if (!shadow_direct(P, tris, nodes, P.links, X, n, M, choice[n_shadow % (unsigned)P.choices], f_direct))
                                f_direct[0] = f_direct[1] = f_direct[2] = 0;
                            n_shadow++;
                            double o4[4];
                            cosine_hemi<double, true>(n, d, r0, r1, o4);
                            if (o4[3] == 0) { mark_unused(P.rand_0, base, f_bounce + 1, P.D); done = true; }
                            else {
                                const double cos_theta = o4[0] * n[0] + o4[1] * n[1] + o4[2] * n[2];
#pragma unroll
                                for (int k = 0; k < 3; k++) {
                                    f_thr[k] *= (M.diffuse[k] * inv_pi) * cos_theta / o4[3];
                                    o[k] = X[k] + eps * o4[k];
                                    d[k] = o4[k];
                                }
                                // trace_path(scene, ..., ray, bounce + 1, ...), :78 -- the caller's frame goes to LDS
                                double* fr = s_st + ((size_t)depth * kOldFields) * kOldThreads + tid;
#pragma unroll
                                for (int k = 0; k < 3; k++) {
                                    fr[(size_t)k * kOldThreads] = f_thr[k]; fr[(size_t)(3 + k) * kOldThreads] = f_L[k];
                                    fr[(size_t)(6 + k) * kOldThreads] = f_direct[k];
                                    f_thr[k] = 1; f_L[k] = 0; f_direct[k] = 0;
                                }
                                fr[(size_t)9 * kOldThreads] = f_r0; fr[(size_t)10 * kOldThreads] = (double)f_bounce;
                                f_r0 = 0.0; f_bounce = f_bounce + 1;
                                depth++;
                                continue;
                            }
                        } else if (M.is_mirror || M.transmission > 0.0) {
                            specular_bounce(M, X, n, inside, r0, o, d);
                        } else done = true;                                  // :122-124
                    }
                }
                if (!done && f_bounce > 3) {                                 // :127-133
                    const double rr = ::fmax(0.05, 1 - f_thr[1]);
                    if (f_r0 < rr) { mark_unused(P.rand_0, base, f_bounce + 1, P.D); done = true; }
                    else { f_thr[0] /= 1 - rr; f_thr[1] /= 1 - rr; f_thr[2] /= 1 - rr; }
                }
                if (!done) { f_bounce++; continue; }
                ret[0] = f_L[0]; ret[1] = f_L[1]; ret[2] = f_L[2];          // return light, :137
                if (depth == 0) break;
                depth--;                                                     // the caller's frame comes back
                const double* fr = s_st + ((size_t)depth * kOldFields) * kOldThreads + tid;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    f_thr[k] = fr[(size_t)k * kOldThreads]; f_L[k] = fr[(size_t)(3 + k) * kOldThreads];
                    f_direct[k] = fr[(size_t)(6 + k) * kOldThreads];
                }
                f_r0 = fr[(size_t)9 * kOldThreads]; f_bounce = (int)fr[(size_t)10 * kOldThreads];
                resume = true;
            }
        }
        s_L[tid * 3] = ret[0]; s_L[tid * 3 + 1] = ret[1]; s_L[tid * 3 + 2] = ret[2];
        __syncthreads();
        if (owner) {        // color += light, sample by sample (:163)
            const int ns = P.S - s0 < chunk ? P.S - s0 : chunk;
            for (int q = 0; q < ns; q++) {
                const double* l = s_L + (size_t)(tid * chunk + q) * 3;
                color[0] += l[0]; color[1] += l[1]; color[2] += l[2];
            }
        }
        __syncthreads();
    }
    if (owner) {
        const size_t px = (size_t)blockIdx.x * ppb + tid;
#pragma unroll
        for (int k = 0; k < 3; k++) {                                       // :166-167
            double c = color[k] / (double)P.S;
            c = c < 0 ? 0.0 : (c > 1 ? 1.0 : c);
            P.image[px * 3 + k] = c;
        }
    }
}

hipError_t launch_render_surface(const RenderParams& P, hipStream_t s)
{
    const int n = P.W * P.H;
    if (n <= 0) return hipSuccess;
    if (P.variant == 1) {
        const int chunk_o = P.S < kOldThreads ? P.S : kOldThreads, ppb_o = kOldThreads / chunk_o;
        const size_t lds_o = ((size_t)kOldThreads * 3 + (size_t)P.D * kOldFields * kOldThreads) * sizeof(double);      // D <= kRenderOldMaxDepth: <= 137 KiB
        if (lds_o > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_render_surface_old), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_o);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_render_surface_old, dim3((n + ppb_o - 1) / ppb_o), dim3(kOldThreads), lds_o, s, P);
        return hipGetLastError();
    }
    const int chunk = P.S < kRenderThreads ? P.S : kRenderThreads, ppb = kRenderThreads / chunk;
    const size_t tables = (size_t)P.n_tris * (sizeof(TriD<double>) + sizeof(lt_surface_material)) + (size_t)P.n_nodes * sizeof(NodeD<double>) +
                          (size_t)((16 * P.n_nodes * 2 + 3) / 4) * 4;
    const size_t lds_l = (size_t)kRenderThreads * 3 * sizeof(double);
    // (a mesh without link tables has more than 32767 nodes, 3 MB of tables: never in LDS; the check keeps lds_copy off a null P.links)
    if (tables <= 48 * 1024 && P.links && P.lds_tables != 0)
        hipLaunchKernelGGL(k_render_surface<true>, dim3((n + ppb - 1) / ppb), dim3(kRenderThreads), lds_l + tables, s, P);
    else
        hipLaunchKernelGGL(k_render_surface<false>, dim3((n + ppb - 1) / ppb), dim3(kRenderThreads), lds_l, s, P);
    return hipGetLastError();
}

}  // namespace ltk
