/*
 * lt_oracle.c -- CPU oracle (TEST INFRASTRUCTURE ONLY; see lt_oracle.h for the
 * pinning statement: reference functions pinned by golden vectors, the
 * volumetric walk PARITY UNPINNED vs the reference and pinned analytically).
 *
 * Build: make -C oracle   (gcc, -ffp-contract=off so that every operation is a
 * separately rounded IEEE operation as in the reference's NumPy float64 code).
 */
#define _GNU_SOURCE
#include "lt_oracle.h"

#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

/* ---- XORWOW, restating the published generator (Marsaglia 2003, "Xorshift
 * RNGs", xorwow) with rocRAND 3.x's seeding for (seed, subsequence 0, offset 0)
 * -- rocRAND is the third-party library the product calls on the device
 * (/opt/rocm/include/rocrand/rocrand_xorwow.h, ROCm 7.2); tests/ check this
 * restatement bit-for-bit against the device generator (lt_rng_raw). -------- */
typedef struct lto_xorwow { uint32_t x[5]; uint32_t d; } lto_xorwow;

static inline uint64_t lto_mix64(uint64_t z)
{   /* splitmix64's output function */
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static inline uint64_t lto_mix_seed(uint64_t seed, uint64_t photon_id)
{   /* one stream per (seed, photon id), hashed in two stages: the seed first, then the id into the hashed seed -- so
     * that no pair (seed + k*c, id - k) shares a stream with (seed, id), as a single hash of seed + (id + 1)*c would */
    return lto_mix64(lto_mix64(seed + 0x9E3779B97F4A7C15ULL) ^ ((photon_id + 1) * 0x9E3779B97F4A7C15ULL));
}

static inline void lto_xorwow_seed(lto_xorwow* s, uint64_t seed)
{
    s->x[0] = 123456789U; s->x[1] = 362436069U; s->x[2] = 521288629U;
    s->x[3] = 88675123U;  s->x[4] = 5783321U;   s->d = 6615241U;
    const uint32_t s0 = (uint32_t)seed ^ 0x2c7f967fU;
    const uint32_t s1 = (uint32_t)(seed >> 32) ^ 0xa03697cbU;
    const uint32_t t0 = 1228688033U * s0;
    const uint32_t t1 = 2073658381U * s1;
    s->x[0] += t0; s->x[1] ^= t0; s->x[2] += t1; s->x[3] ^= t1; s->x[4] += t0;
    s->d += t1 + t0;
}

static inline uint32_t lto_xorwow_next(lto_xorwow* s)
{
    const uint32_t t = s->x[0] ^ (s->x[0] >> 2);
    s->x[0] = s->x[1]; s->x[1] = s->x[2]; s->x[2] = s->x[3]; s->x[3] = s->x[4];
    s->x[4] = (s->x[4] ^ (s->x[4] << 4)) ^ (t ^ (t << 1));
    s->d += 362437U;
    return s->d + s->x[4];
}

/* One stream per photon: seed-only initialisation leaves three of the five state words offset by the SAME 32-bit
 * value (above), and the first draws of every photon -- its first step length and deflection -- inherit that
 * structure: at 10^8 photons the matched-slab benchmark came out 9e-5 off van de Hulst's Rd and Tt (10 sigma),
 * with a seed-to-seed scatter far below the statistical one.  Discarding LTO_RNG_WARMUP outputs after seeding
 * removes both effects (4, 8, 16 and 32 discards agree to 1e-5; profiles/r01e_rng_seeding.log). */
#define LTO_RNG_WARMUP 8
static inline void lto_photon_stream(lto_xorwow* s, uint64_t seed, uint64_t photon_id)
{
    lto_xorwow_seed(s, lto_mix_seed(seed, photon_id));
    for (int k = 0; k < LTO_RNG_WARMUP; k++) (void)lto_xorwow_next(s);
}

/* uniforms in (0,1]: rocrand_uniform_double (two draws, 53 bits) and
 * rocrand_uniform (one draw) -- rocrand_uniform.h:67,102-109 */
static inline double lto_uniform_f64(lto_xorwow* s)
{
    uint32_t v1 = lto_xorwow_next(s), v2 = lto_xorwow_next(s);
    uint64_t v = ((uint64_t)(v2 >> 11) << 32) | (uint64_t)v1;
    return 1.1102230246251565e-16 + (double)v * 1.1102230246251565e-16;
}
static inline double lto_uniform32_f64(lto_xorwow* s)   /* one draw, 32-bit resolution: rocrand_uniform.h:97-100 */
{
    uint32_t v = lto_xorwow_next(s);
    return 2.3283064365386963e-10 + (double)v * 2.3283064365386963e-10;
}
static inline float lto_uniform_f32(lto_xorwow* s)
{
    uint32_t v = lto_xorwow_next(s);
    return 2.3283064365386963e-10f + (float)v * 2.3283064365386963e-10f;
}
static inline float lto_uniform32_f32(lto_xorwow* s) { return lto_uniform_f32(s); }

static inline void lto_atomic_add_f64(double* p, double v)
{
    uint64_t* q = (uint64_t*)p;
    uint64_t old = __atomic_load_n(q, __ATOMIC_RELAXED), neu;
    do {
        double o; memcpy(&o, &old, 8); o += v; memcpy(&neu, &o, 8);
    } while (!__atomic_compare_exchange_n(q, &old, neu, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED));
}

/* PreComputedTriangle derived fields, S/primitives.py:99-112 (float64) */
int lto_triangle_fields(const double* tris, size_t n, double* out)
{
    for (size_t i = 0; i < n; i++) {
        const double* a = tris + i * 9; const double* b = a + 3; const double* c = a + 6;
        double* o = out + i * 16;
        double e1[3], e2[3], nn[3];
        for (int k = 0; k < 3; k++) {
            o[k] = (a[k] + b[k] + c[k]) / 3;   /* centroid :104 */
            e1[k] = b[k] - a[k];               /* edge_1 :107 */
            e2[k] = c[k] - a[k];               /* edge_2 :108 */
        }
        nn[0] = e1[1] * e2[2] - e1[2] * e2[1]; /* _normal :109 */
        nn[1] = e1[2] * e2[0] - e1[0] * e2[2];
        nn[2] = e1[0] * e2[1] - e1[1] * e2[0];
        double num = a[0] * nn[0] + a[1] * nn[1] + a[2] * nn[2]; /* num :111 */
        double l = sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
        for (int k = 0; k < 3; k++) { o[3 + k] = e1[k]; o[6 + k] = e2[k]; o[9 + k] = nn[k] / l; }
        o[12] = num; o[13] = o[14] = o[15] = 0;
    }
    return 0;
}

/* Test hook: while set, every scattering of the walks deflects by exactly 90 degrees (cos = 0) -- what the quotient form of
 * the Henyey-Greenstein sampling gave in float for every |g| <= 1e-8 before the walk took hg_sample_walk.  A test plants it to
 * show that its bound would have noticed (tests/test_hg_walk_cpu.py).  Not thread safe against running walks; off by default. */
static int g_plant_cos0 = 0;
void lto_plant_cos0(int on) { g_plant_cos0 = on; }

/* ---- instantiate the precision-generic body ------------------------------ */
#define R double
#define SFX(n) n##_f64
#define RLOG log
#define RSIN sin
#define RCOS cos
#define RSQRT sqrt
#define RFABS fabs
#define RFMA fma
#define RNEXT nextafter
#include "lt_walk.inc"
#undef R
#undef SFX
#undef RLOG
#undef RSIN
#undef RCOS
#undef RSQRT
#undef RFABS
#undef RFMA
#undef RNEXT

#define R float
#define SFX(n) n##_f32
#define RLOG logf
#define RSIN sinf
#define RCOS cosf
#define RSQRT sqrtf
#define RFABS fabsf
#define RFMA fmaf
#define RNEXT nextafterf
#include "lt_walk.inc"
#undef R
#undef SFX

/* ---- exports -------------------------------------------------------------- */
int lto_run(const lto_scene* sc, uint64_t n_photons, uint64_t photon_offset, uint64_t seed,
            const double* rng_table, uint64_t table_steps, int walk_f32, double* grid_f64,
            uint64_t* grid_fx, lt_counters* counters, int n_threads)
{
    if (!sc || !counters) return LT_E_INVALID;
    if ((sc->n_layers > 0) == (sc->n_tris > 0)) return LT_E_INVALID;
    if (walk_f32 && rng_table) return LT_E_UNSUPPORTED;
    return walk_f32
        ? run_f32(sc, n_photons, photon_offset, seed, rng_table, table_steps, grid_f64, grid_fx, counters, n_threads, NULL, NULL, 0)
        : run_f64(sc, n_photons, photon_offset, seed, rng_table, table_steps, grid_f64, grid_fx, counters, n_threads, NULL, NULL, 0);
}

/* f4: the same walk, also storing the first max_vertices vertices of every path */
int lto_run_capture(const lto_scene* sc, uint64_t n_photons, uint64_t photon_offset, uint64_t seed,
                    double* grid_f64, lt_counters* counters, lt_vertex* vertices, uint32_t* counts,
                    uint32_t max_vertices)
{
    if (!sc || !counters || !vertices || !counts || max_vertices == 0) return LT_E_INVALID;
    if ((sc->n_layers > 0) == (sc->n_tris > 0)) return LT_E_INVALID;
    return run_f64(sc, n_photons, photon_offset, seed, NULL, 0, grid_f64, NULL, counters, 1, vertices, counts, max_vertices);
}

int lto_rng_raw(uint64_t seed, uint64_t photon_id, uint32_t count, uint32_t* out)
{
    lto_xorwow s; lto_photon_stream(&s, seed, photon_id);
    for (uint32_t i = 0; i < count; i++) out[i] = lto_xorwow_next(&s);
    return 0;
}

int lto_eval(int fn, const double* in, size_t n, double* out)
{
    for (size_t i = 0; i < n; i++) {
        switch (fn) {
        case LT_FN_HG_PDF: out[i] = hg_pdf_f64(in[2 * i], in[2 * i + 1]); break;
        case LT_FN_HG_SAMPLE: out[i] = hg_sample_f64(in[2 * i], in[2 * i + 1]); break;
        case LT_FN_ONB: onb_f64(in + 3 * i, out + 6 * i, out + 6 * i + 3); break;
        case LT_FN_DISK: disk_f64(in[2 * i], in[2 * i + 1], out + 2 * i); break;
        case LT_FN_COSINE_HEMI: cosine_hemi_f64(in + 8 * i, in + 8 * i + 3, in[8 * i + 6], in[8 * i + 7], out + 4 * i); break;
        case LT_FN_REFLECT: reflect_f64(in + 6 * i, in + 6 * i + 3, out + 3 * i); break;
        case LT_FN_BOUNDARY: {
            double ct, refr[3];
            out[5 * i] = boundary_f64(in + 8 * i, in + 8 * i + 3, in[8 * i + 6], in[8 * i + 7], &ct, refr);
            out[5 * i + 1] = ct; out[5 * i + 2] = refr[0]; out[5 * i + 3] = refr[1]; out[5 * i + 4] = refr[2];
        } break;
        case LT_FN_SPIN: {
            double u[3] = {in[5 * i], in[5 * i + 1], in[5 * i + 2]};
            spin_f64(u, in[5 * i + 3], in[5 * i + 4]);
            out[3 * i] = u[0]; out[3 * i + 1] = u[1]; out[3 * i + 2] = u[2];
        } break;
        case LT_FN_HG_WALK: {   /* a row of the library's query: xi, f32, a 12-value medium record; the oracle takes its g (field 3) */
            const double* r = in + 14 * i;
            const double c = r[1] != 0.0 ? (double)hg_sample_walk_f32((float)r[0], (float)r[5]) : hg_sample_walk_f64(r[0], r[5]);
            out[2 * i] = out[2 * i + 1] = c;
        } break;
        default: return LT_E_INVALID;
        }
    }
    return 0;
}

static void make_tri(const double* v9, tri_f64* T)
{
    double f[16]; lto_triangle_fields(v9, 1, f);
    for (int k = 0; k < 3; k++) { T->a[k] = v9[k]; T->ab[k] = f[3 + k]; T->ac[k] = f[6 + k]; T->n[k] = f[9 + k]; }
    T->med_front = T->med_back = -1;
}

int lto_triangle_intersect(const double* origins, const double* dirs, const double* tris, size_t n, double* t_out)
{
    for (size_t i = 0; i < n; i++) {
        tri_f64 T; make_tri(tris + 9 * i, &T);
        t_out[i] = tri_hit_f64(origins + 3 * i, dirs + 3 * i, &T);
    }
    return 0;
}

int lto_intersect_bounds(const double* origins, const double* dirs, const double* tmax,
                         const double* boxes, size_t n, int32_t* hit_out)
{
    for (size_t i = 0; i < n; i++) {
        const double* d = dirs + 3 * i;
        double inv[3] = {1.0 / d[0], 1.0 / d[1], 1.0 / d[2]};
        hit_out[i] = box_hit_f64(boxes + 6 * i, boxes + 6 * i + 3, origins + 3 * i, inv, tmax ? tmax[i] : INFINITY);
    }
    return 0;
}

int lto_intersect_rays(const lto_scene* sc, const double* origins, const double* dirs, const double* tmax,
                       size_t n, int use_bvh, int32_t* prim_out, double* t_out)
{
    if (!sc || sc->n_tris <= 0) return LT_E_INVALID;
    world_f64 W; prepare_f64(&W, sc);
    for (size_t i = 0; i < n; i++) {
        int pi; double t; double tm = tmax ? tmax[i] : INFINITY;
        if (use_bvh) nearest_bvh_f64(W.tris, W.nodes, sc->n_nodes, origins + 3 * i, dirs + 3 * i, tm, &pi, &t);
        else nearest_brute_f64(W.tris, sc->n_tris, origins + 3 * i, dirs + 3 * i, tm, &pi, &t);
        prim_out[i] = pi; t_out[i] = t;
    }
    release_f64(&W);
    return 0;
}


/* ---- surface path tracer (f2), S/path_tracing_fix1.py ---------------------- */
static void mark_unused(double* rand_0, size_t base, int from, int D) /* :36-38, :64-66, :128-130 */
{
    for (int b = from; b < D; b++) rand_0[base + b] = INFINITY;
}

int lto_render_surface(const lto_scene* sc, const lt_surface_material* mats, const lt_point_light* lights,
                       int n_lights, int W, int H, int S, int D, const double camera[3], double f_distance,
                       const double* xs, const double* ys, double* rand_0, const double* rand_1,
                       const int32_t* light_choice, double* image)
{
    if (!sc || sc->n_tris <= 0 || !mats || !lights || n_lights <= 0) return LT_E_INVALID;
    world_f64 Wd; prepare_f64(&Wd, sc);
    const double eps = 1e-6, inv_pi = 0.3183098861837907;
    for (int i = 0; i < H; i++) for (int j = 0; j < W; j++) {
        double color[3] = {0, 0, 0};
        for (int smp = 0; smp < S; smp++) {
            const size_t base = (((size_t)i * W + j) * S + smp) * (size_t)D;
            double o[3] = {camera[0], camera[1], camera[2]};
            const double jit = rand_0[base];                                   /* :156-157 (quirk B6) */
            double d[3] = {xs[j] + jit / (double)W - o[0], ys[i] + jit / (double)H - o[1], f_distance - o[2]};
            normalize3_f64(d);
            double thr[3] = {1, 1, 1}, L[3] = {0, 0, 0};
            for (int bounce = 0;;) {
                if (bounce >= D) break;
                const double r0 = rand_0[base + bounce], r1 = rand_1[base + bounce];
                int prim; double t;
                nearest_bvh_f64(Wd.tris, Wd.nodes, sc->n_nodes, o, d, INFINITY, &prim, &t);
                if (prim < 0) { mark_unused(rand_0, base, bounce, D); break; }
                const lt_surface_material* M = &mats[prim];
                double n[3] = {Wd.tris[prim].n[0], Wd.tris[prim].n[1], Wd.tris[prim].n[2]};
                const double X[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
                if (M->is_light) for (int k = 0; k < 3; k++) L[k] += M->emission * thr[k];
                int inside = 0;
                if (dot3_f64(n, d) > 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; inside = 1; }
                if (M->is_diffuse) {
                    const double so[3] = {X[0] + eps * n[0], X[1] + eps * n[1], X[2] + eps * n[2]};
                    const lt_point_light* lt = &lights[light_choice[base + bounce]];
                    double v[3] = {lt->source[0] - so[0], lt->source[1] - so[1], lt->source[2] - so[2]};
                    const double mag = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                    const double sd[3] = {v[0] / mag, v[1] / mag, v[2] / mag};
                    int sp; double st;
                    nearest_bvh_f64(Wd.tris, Wd.nodes, sc->n_nodes, so, sd, INFINITY, &sp, &st);
                    if (st >= mag - eps) {                                     /* S/light_samples.py:53 */
                        const double cos_t = dot3_f64(n, sd);
                        const double nsd[3] = {-sd[0], -sd[1], -sd[2]};
                        const double cos_p = dot3_f64(lt->normal, nsd);
                        const double geom = fabs(cos_t * cos_p) / (mag * mag);
                        for (int k = 0; k < 3; k++)
                            L[k] += thr[k] * ((lt->radiance[k] * (M->diffuse[k] * inv_pi)) * geom * lt->total_area);
                    }
                    double o4[4];
                    cosine_hemi_f64(n, d, r0, r1, o4);
                    if (o4[3] == 0) { mark_unused(rand_0, base, bounce + 1, D); break; }
                    const double cos_theta = o4[0] * n[0] + o4[1] * n[1] + o4[2] * n[2];
                    for (int k = 0; k < 3; k++) {
                        thr[k] *= (M->diffuse[k] * inv_pi) * cos_theta / o4[3];
                        o[k] = X[k] + eps * o4[k];
                        d[k] = o4[k];
                    }
                } else if (M->is_mirror) {
                    double r[3]; reflect_f64(d, n, r);
                    for (int k = 0; k < 3; k++) { o[k] = X[k] + eps * n[k]; d[k] = r[k]; }
                } else if (M->transmission > 0.0) {                            /* :86-119, kept as written */
                    const double n1 = inside ? M->ior : 1.0, n2 = inside ? 1.0 : M->ior;
                    const double R0 = ((n1 - n2) / (n1 + n2)) * ((n1 - n2) / (n1 + n2));
                    const double theta = dot3_f64(d, n);
                    const double refl_prob = R0 + (1 - R0) * pow(1 - cos(theta), 5.0);
                    double Nr = M->ior;
                    if (theta > 0) Nr = 1 / Nr;
                    Nr = 1 / Nr;
                    const double cos_theta = -theta;
                    const double rad = 1 - (Nr * Nr) * (1 - cos_theta * cos_theta);
                    if (rad > 0 && r0 > refl_prob) {
                        const double kk = Nr * cos_theta - sqrt(rad);
                        double tr[3] = {d[0] * Nr + n[0] * kk, d[1] * Nr + n[1] * kk, d[2] * Nr + n[2] * kk};
                        normalize3_f64(tr);
                        for (int k = 0; k < 3; k++) { o[k] = X[k] - eps * n[k]; d[k] = tr[k]; }
                    } else {
                        double r[3]; reflect_f64(d, n, r);
                        for (int k = 0; k < 3; k++) { o[k] = X[k] + eps * n[k]; d[k] = r[k]; }
                    }
                } else break;
                if (bounce > 5) {
                    const double rr = fmax(0.05, 1 - thr[1]);
                    if (r0 < rr) { mark_unused(rand_0, base, bounce + 1, D); break; }
                    thr[0] /= 1 - rr; thr[1] /= 1 - rr; thr[2] /= 1 - rr;
                }
                bounce++;
            }
            color[0] += L[0]; color[1] += L[1]; color[2] += L[2];
        }
        for (int k = 0; k < 3; k++) {
            double c = color[k] / (double)S;
            c = c < 0 ? 0.0 : (c > 1 ? 1.0 : c);
            image[((size_t)i * W + j) * 3 + k] += 0.25 * c;
        }
    }
    release_f64(&Wd);
    return 0;
}


/* ---- the recursive ancestor, S/path_tracing_old.py (the integrator examples/LTS.ipynb calls) ---- */
typedef struct old_env {
    const world_f64* Wd; const lto_scene* sc;
    const lt_surface_material* mats; const lt_point_light* lights;
    double* rand_0; const double* rand_1;
    const int32_t* choice; int choices; unsigned n_shadow;
    size_t base; int D;
} old_env;

/* trace_path(scene, primitives, bvh, ray, bounce, rand_idx), :17-137; the ray (o, d) is the caller's object */
static void trace_path_old(old_env* E, double o[3], double d[3], int bounce, double L[3])
{
    const double eps = 1e-6, inv_pi = 0.3183098861837907;
    double thr[3] = {1, 1, 1};
    L[0] = L[1] = L[2] = 0;
    for (;;) {
        if (bounce >= E->D) break;                                             /* :24-25 */
        const double r0 = E->rand_0[E->base + bounce], r1 = E->rand_1[E->base + bounce];
        int prim; double t;
        nearest_bvh_f64(E->Wd->tris, E->Wd->nodes, E->sc->n_nodes, o, d, INFINITY, &prim, &t);
        if (prim < 0) { mark_unused(E->rand_0, E->base, bounce, E->D); break; }  /* :34-38 */
        const lt_surface_material* M = &E->mats[prim];
        double n[3] = {E->Wd->tris[prim].n[0], E->Wd->tris[prim].n[1], E->Wd->tris[prim].n[2]};
        const double X[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        if (M->is_light && bounce == 0) for (int k = 0; k < 3; k++) L[k] += M->emission * thr[k];   /* :45-46 */
        int inside = 0;
        if (dot3_f64(n, d) > 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; inside = 1; }
        if (M->is_diffuse) {
            double direct[3] = {0, 0, 0};                                      /* cast_one_shadow_ray, :56 */
            const double so[3] = {X[0] + eps * n[0], X[1] + eps * n[1], X[2] + eps * n[2]};
            const lt_point_light* lt = &E->lights[E->choice[E->n_shadow % (unsigned)E->choices]];
            E->n_shadow++;
            double v[3] = {lt->source[0] - so[0], lt->source[1] - so[1], lt->source[2] - so[2]};
            const double mag = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            const double sd[3] = {v[0] / mag, v[1] / mag, v[2] / mag};
            int sp; double st;
            nearest_bvh_f64(E->Wd->tris, E->Wd->nodes, E->sc->n_nodes, so, sd, INFINITY, &sp, &st);
            if (st >= mag - eps) {
                const double cos_t = dot3_f64(n, sd);
                const double nsd[3] = {-sd[0], -sd[1], -sd[2]};
                const double cos_p = dot3_f64(lt->normal, nsd);
                const double geom = fabs(cos_t * cos_p) / (mag * mag);
                for (int k = 0; k < 3; k++) direct[k] = (lt->radiance[k] * (M->diffuse[k] * inv_pi)) * geom * lt->total_area;
            }
            double o4[4];
            cosine_hemi_f64(n, d, r0, r1, o4);                                 /* :59 */
            if (o4[3] == 0) { mark_unused(E->rand_0, E->base, bounce + 1, E->D); break; }   /* :61-64 */
            const double cos_theta = o4[0] * n[0] + o4[1] * n[1] + o4[2] * n[2];
            for (int k = 0; k < 3; k++) {
                thr[k] *= (M->diffuse[k] * inv_pi) * cos_theta / o4[3];
                o[k] = X[k] + eps * o4[k];
                d[k] = o4[k];
            }
            double Lc[3];
            trace_path_old(E, o, d, bounce + 1, Lc);                           /* :78: same ray object */
            for (int k = 0; k < 3; k++) L[k] += (direct[k] + thr[k] * Lc[k]);  /* :78-80 */
        } else if (M->is_mirror) {
            double r[3]; reflect_f64(d, n, r);
            for (int k = 0; k < 3; k++) { o[k] = X[k] + eps * n[k]; d[k] = r[k]; }
        } else if (M->transmission > 0.0) {                                    /* :88-120 */
            const double n1 = inside ? M->ior : 1.0, n2 = inside ? 1.0 : M->ior;
            const double R0 = ((n1 - n2) / (n1 + n2)) * ((n1 - n2) / (n1 + n2));
            const double theta = dot3_f64(d, n);
            const double refl_prob = R0 + (1 - R0) * pow(1 - cos(theta), 5.0);
            double Nr = M->ior;
            if (theta > 0) Nr = 1 / Nr;
            Nr = 1 / Nr;
            const double cos_theta = -theta;
            const double rad = 1 - (Nr * Nr) * (1 - cos_theta * cos_theta);
            if (rad > 0 && r0 > refl_prob) {
                const double kk = Nr * cos_theta - sqrt(rad);
                double tr[3] = {d[0] * Nr + n[0] * kk, d[1] * Nr + n[1] * kk, d[2] * Nr + n[2] * kk};
                normalize3_f64(tr);
                for (int k = 0; k < 3; k++) { o[k] = X[k] - eps * n[k]; d[k] = tr[k]; }
            } else {
                double r[3]; reflect_f64(d, n, r);
                for (int k = 0; k < 3; k++) { o[k] = X[k] + eps * n[k]; d[k] = r[k]; }
            }
        } else break;
        if (bounce > 3) {                                                      /* :127-133 */
            const double rr = fmax(0.05, 1 - thr[1]);
            if (r0 < rr) { mark_unused(E->rand_0, E->base, bounce + 1, E->D); break; }
            thr[0] /= 1 - rr; thr[1] /= 1 - rr; thr[2] /= 1 - rr;
        }
        bounce++;
    }
}

int lto_render_surface_old(const lto_scene* sc, const lt_surface_material* mats, const lt_point_light* lights,
                           int n_lights, int W, int H, int S, int D, const double camera[3], double f_distance,
                           const double* xs, const double* ys, double* rand_0, const double* rand_1,
                           const int32_t* light_choice, int choices_per_sample, double* image)
{
    if (!sc || sc->n_tris <= 0 || !mats || !lights || n_lights <= 0 || choices_per_sample <= 0) return LT_E_INVALID;
    world_f64 Wd; prepare_f64(&Wd, sc);
    old_env E = {&Wd, sc, mats, lights, rand_0, rand_1, NULL, choices_per_sample, 0, 0, D};
    for (int i = 0; i < H; i++) for (int j = 0; j < W; j++) {
        double color[3] = {0, 0, 0};
        for (int smp = 0; smp < S; smp++) {
            const size_t sample = ((size_t)i * W + j) * S + smp;
            E.base = sample * (size_t)D;
            E.choice = light_choice + sample * (size_t)choices_per_sample;
            E.n_shadow = 0;
            double o[3] = {camera[0], camera[1], camera[2]};
            const double jit = rand_0[E.base];                                 /* :158-159 */
            double d[3] = {xs[j] + jit / (double)W - o[0], ys[i] + jit / (double)H - o[1], f_distance - o[2]};
            normalize3_f64(d);
            double L[3];
            trace_path_old(&E, o, d, 0, L);
            color[0] += L[0]; color[1] += L[1]; color[2] += L[2];
        }
        for (int k = 0; k < 3; k++) {                                          /* :166-167 */
            double c = color[k] / (double)S;
            image[((size_t)i * W + j) * 3 + k] = c < 0 ? 0.0 : (c > 1 ? 1.0 : c);
        }
    }
    release_f64(&Wd);
    return 0;
}
